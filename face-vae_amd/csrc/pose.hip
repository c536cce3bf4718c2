// Head pose estimator pieces (HPE_EDE, models.py:990-1037 of Luh1124/face-vae; ResBottleneck
// modules.py:138-152): the operators the ResNet-50-shaped trunk needs beyond the 1x1 / 3x3
// convolutions and batch norms of conv.hip / bn.hip.
//
//   fv_stem7s2_*        nn.Conv2d(3, cout, 7, 2, 3) on the NCHW fp32 image as an implicit GEMM on
//                       the matrix units (Frag / mma of conv_common.h: bf16 16x16x32, fp32 the
//                       exact 16x16x4).  k = (r*7 + s)*3 + ci, 147 valid of STEM_K = 160 columns,
//                       padded once in the weight image.  Every lane gathers its own im2col
//                       fragment from the image into registers (no LDS) and the wave walks the
//                       output-channel tiles; the BN record of a 16-pixel tile (sum, sum of
//                       squares) is reduced with DPP row sums.  The weight gradient is a GEMM over the pixels
//                       (both operands transposed into LDS), split over blocks into fp32 slabs
//                       that a second kernel sums in split order.
//   fv_maxpool3s2_*     nn.MaxPool2d(3, 2, 1) over NHWC with a recorded argmax tap; optional
//                       BN-apply + activation prologue.  Backward gathers.
//   fv_subsample2_*     every second pixel (the stride of a stride-2 1x1 conv).
//   fv_bn2_add_relu_fwd relu(BN(a) + BN(b)) (or + b) in one pass.
//   fv_pose_pool_fwd, fv_pose_head_*   global mean, five Linear layers, softmax expectation.
//
// No float atomics anywhere: every cross-thread sum has a fixed order, so reruns are bit-identical.
#include "conv_common.h"

namespace {

#define FV_SUPPORTED(cond, ...)                \
  do {                                         \
    if (!(cond)) {                             \
      fv_set_error(__VA_ARGS__);               \
      return FV_E_UNSUPPORTED;                 \
    }                                          \
  } while (0)

constexpr int NT = 256;
constexpr int STEM_K = 160;      // 7*7*3 = 147 padded to 5 MFMA k-steps of 32
constexpr int STEM_KV = 147;
constexpr int STEM_RM = 2;       // 16-pixel tiles per wave of the forward
constexpr int STEM_REC = 16;     // pixels per BN record (one MFMA pixel tile)
constexpr int STEM_WG_PIX = 64;  // pixels per weight-gradient chunk
constexpr int STEM_WG_MAXSPLIT = 512;

template <typename T> struct IsF32 { static constexpr bool v = false; };
template <> struct IsF32<float> { static constexpr bool v = true; };

struct StemArgs {
  const float* x;     // [N][3][H][W]
  const void* wk;     // [cpad][STEM_K]
  const float* bias;
  void* y;            // [N][Ho][Wo][Cout]
  float* stats;       // [nrec][2][Cout] or NULL
  int N, H, W, Ho, Wo, P, Cout, nct, nrec;
};

// Tap table of a block, in LDS: column k -> {offset of tap (r, s, ci) from the window's first
// element, (ci*H + r)*W + s; r | s << 16}.  The padding columns k >= 147 get offset 0 (their weights
// are zero, and element 0 of the window is a tap of the window anyway) and an r that fails every
// bounds check.  Filled by the first STEM_K threads; the caller syncs.
__device__ __forceinline__ void stem_tab_fill(int2* tab, int tid, int H, int W) {
  if (tid < STEM_K) {
    const int rs = tid / 3, ci = tid - rs * 3;
    const int r = rs / 7, s = rs - r * 7;
    tab[tid] = tid < STEM_KV ? make_int2((ci * H + r) * W + s, r | (s << 16)) : make_int2(0, 0x7fff);
  }
}
// value of im2col column k of the output pixel whose window starts at (iy0, ix0) = (2 oy - 3,
// 2 ox - 3), element pixbase of the image; 0 in the padding, for k >= 147 and for !valid.  The
// load is predicated by its address (element 0 when masked), never by a branch, so the unrolled
// gathers stay independent loads in flight.  INTERIOR: the whole window is inside the image.
template <bool INTERIOR>
__device__ __forceinline__ float stem_tap(const float* __restrict__ x, const int2* tab, int pixbase, int iy0, int ix0,
                                          int k, int H, int W, bool valid) {
  const int2 t = tab[k];
  if constexpr (INTERIOR) {
    return x[pixbase + t.x];
  } else {
    const bool ok = valid && (unsigned)(iy0 + (t.y & 0xffff)) < (unsigned)H && (unsigned)(ix0 + (t.y >> 16)) < (unsigned)W;
    const float v = x[ok ? pixbase + t.x : 0];
    return ok ? v : 0.f;
  }
}

__device__ __forceinline__ void frag_set(Frag<bf16>& fr, const float* f) {
#pragma unroll
  for (int j = 0; j < 8; ++j) fr.v[j] = (bf16)f[j];
}
__device__ __forceinline__ void frag_set(Frag<float>& fr, const float* f) {
#pragma unroll
  for (int j = 0; j < 8; ++j) fr.v[j] = f[j];
}

template <typename T>
__global__ void stem_weight_prep_kernel(const float* __restrict__ w, int cout, int cpad, T* __restrict__ wk) {
  const int i = blockIdx.x * NT + threadIdx.x;
  if (i >= cpad * STEM_K) return;
  const int co = i / STEM_K, k = i - co * STEM_K;
  float v = 0.f;
  if (co < cout && k < STEM_KV) {
    const int rs = k / 3, ci = k - rs * 3;
    const int r = rs / 7, s = rs - r * 7;
    v = w[((co * 3 + ci) * 7 + r) * 7 + s];
  }
  wk[i] = Elt<T>::from_f(v);
}

// One wave: STEM_RM tiles of 16 output pixels.  Lane (lr, lh) of the MFMA's pixel operand holds
// columns k = ks*32 + lh*8 + j of pixel lr -- 8 consecutive im2col columns per k-step -- so every
// lane gathers exactly its own 5 x 8 columns from the image into registers: no LDS, no barrier.
// The weight fragments of an output-channel tile are loaded once and used by all the wave's tiles.
template <typename T>
__global__ void __launch_bounds__(NT) stem_fwd_kernel(StemArgs a) {
  constexpr int KS = STEM_K / 32;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lh = lane >> 4;
  const int tile0 = (blockIdx.x * 4 + wave) * STEM_RM;
  __shared__ int2 tab[STEM_K];
  stem_tab_fill(tab, tid, a.H, a.W);
  __syncthreads();
  Frag<T> fb[STEM_RM][KS];
  bool pv[STEM_RM];
#pragma unroll
  for (int m = 0; m < STEM_RM; ++m) {
    const int pix = (tile0 + m) * STEM_REC + lr;
    pv[m] = pix < a.P;
    const int t = pix / a.Wo, ox = pix - t * a.Wo;
    const int n = t / a.Ho, oy = t - n * a.Ho;
    const int iy0 = 2 * oy - 3, ix0 = 2 * ox - 3;
    const int pixbase = (n * 3 * a.H + iy0) * a.W + ix0;
    // most tiles lie inside the image: no bounds checks there (the branch is uniform over the wave)
    const bool inter = __all(pv[m] && iy0 >= 0 && iy0 + 6 < a.H && ix0 >= 0 && ix0 + 6 < a.W);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      float f[8];
      if (inter) {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          f[j] = stem_tap<true>(a.x, tab, pixbase, iy0, ix0, ks * 32 + lh * 8 + j, a.H, a.W, true);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          f[j] = stem_tap<false>(a.x, tab, pixbase, iy0, ix0, ks * 32 + lh * 8 + j, a.H, a.W, pv[m]);
      }
      frag_set(fb[m][ks], f);
    }
  }
  const T* __restrict__ wk = reinterpret_cast<const T*>(a.wk);
  T* __restrict__ y = reinterpret_cast<T*>(a.y);
  for (int ct = 0; ct < a.nct; ++ct) {
    Frag<T> fa[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
      fa[ks].lds(reinterpret_cast<const char*>(wk + (long)(ct * 16 + lr) * STEM_K + ks * 32 + lh * 8));
    // accumulator element i: channel ct*16 + lh*4 + i, pixel lr
    const int cb = ct * 16 + lh * 4;
    const bool cv = cb < a.Cout;   // Cout % 8 == 0: all four channels or none
    float bv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) bv[i] = (a.bias && cv) ? a.bias[cb + i] : 0.f;
#pragma unroll
    for (int m = 0; m < STEM_RM; ++m) {
      f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) acc = mma(fa[ks], fb[m][ks], acc);
      const int rec = tile0 + m;
      float f[4], sv[4], qv[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        f[i] = acc[i] + bv[i];
        const float v = pv[m] ? f[i] : 0.f;
        sv[i] = row16_sum(v);
        qv[i] = row16_sum(v * v);
      }
      if (a.stats && rec < a.nrec && cv && lr == 0) {
        float* sp = a.stats + (long)rec * 2 * a.Cout + cb;
        *reinterpret_cast<float4*>(sp) = make_float4(sv[0], sv[1], sv[2], sv[3]);
        *reinterpret_cast<float4*>(sp + a.Cout) = make_float4(qv[0], qv[1], qv[2], qv[3]);
      }
      if (pv[m] && cv) store4<T>(y + (long)(rec * STEM_REC + lr) * a.Cout + cb, f);
    }
  }
}

struct StemWgArgs {
  const float* x;
  const void* dy;     // [P][Cout]
  float* slab;        // [nsplit][Cout][147]
  float* bslab;       // [nsplit][Cout]
  int N, H, W, Ho, Wo, P, Cout, nsplit, nchunk;
};

// block (split, 64-channel group): dW[co][k] partial = sum over the split's pixels of
// dy[p][co] * im2col[p][k].  k of the MFMA = pixels, so both operands sit transposed in LDS.
template <typename T>
__global__ void __launch_bounds__(NT) stem_wgrad_kernel(StemWgArgs a) {
  constexpr int LDP = IsF32<T>::v ? 68 : 72;
  __shared__ __attribute__((aligned(16))) T colT[STEM_K * LDP];
  __shared__ __attribute__((aligned(16))) T dyT[64 * LDP];
  __shared__ int2 tab[STEM_K];
  stem_tab_fill(tab, threadIdx.x, a.H, a.W);
  __syncthreads();
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lh = lane >> 4;
  const int co0 = blockIdx.y * 64;
  const T* __restrict__ dy = reinterpret_cast<const T*>(a.dy);
  const bool wave_on = co0 + wave * 16 < a.Cout;
  f32x4 acc[STEM_K / 16];
#pragma unroll
  for (int nt = 0; nt < STEM_K / 16; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
  float bacc = 0.f;
  for (int ch = blockIdx.x; ch < a.nchunk; ch += a.nsplit) {
    const int p0 = ch * STEM_WG_PIX;
    {
      const int m = tid & 63;
      const int pix = p0 + m;
      const bool valid = pix < a.P;
      const int t = pix / a.Wo, ox = pix - t * a.Wo;
      const int n = t / a.Ho, oy = t - n * a.Ho;
      const int iy0 = 2 * oy - 3, ix0 = 2 * ox - 3;
      const int pixbase = (n * 3 * a.H + iy0) * a.W + ix0;
#pragma unroll 8
      for (int k = tid >> 6; k < STEM_K; k += 4)
        colT[k * LDP + m] = Elt<T>::from_f(stem_tap<false>(a.x, tab, pixbase, iy0, ix0, k, a.H, a.W, valid));
    }
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int c8 = tid & 7, m = (tid >> 3) + it * 32;
      const int pix = p0 + m, co = co0 + c8 * 8;
      Chunk8<T> v;
      if (pix < a.P && co < a.Cout) v.load(dy + (long)pix * a.Cout + co);
      else v.zero();
#pragma unroll
      for (int j = 0; j < 8; ++j) dyT[(c8 * 8 + j) * LDP + m] = Elt<T>::from_f(v.get(j));
    }
    __syncthreads();
    if (tid < 64) {
      float s = 0.f;
      for (int m = 0; m < STEM_WG_PIX; ++m) s += Elt<T>::to_f(dyT[tid * LDP + m]);
      bacc += s;
    }
    if (wave_on) {
#pragma unroll
      for (int ks = 0; ks < STEM_WG_PIX / 32; ++ks) {
        Frag<T> fa;
        fa.lds(reinterpret_cast<const char*>(dyT + (wave * 16 + lr) * LDP + ks * 32 + lh * 8));
#pragma unroll
        for (int nt = 0; nt < STEM_K / 16; ++nt) {
          Frag<T> fb;
          fb.lds(reinterpret_cast<const char*>(colT + (nt * 16 + lr) * LDP + ks * 32 + lh * 8));
          acc[nt] = mma(fa, fb, acc[nt]);
        }
      }
    }
    __syncthreads();
  }
  // accumulator element i of tile nt: channel co0 + wave*16 + lh*4 + i, column nt*16 + lr
  if (wave_on) {
#pragma unroll
    for (int nt = 0; nt < STEM_K / 16; ++nt) {
      const int k = nt * 16 + lr;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int co = co0 + wave * 16 + lh * 4 + i;
        if (co < a.Cout && k < STEM_KV) a.slab[((long)blockIdx.x * a.Cout + co) * STEM_KV + k] = acc[nt][i];
      }
    }
  }
  if (tid < 64 && co0 + tid < a.Cout) a.bslab[(long)blockIdx.x * a.Cout + co0 + tid] = bacc;
}

// dW (parameter layout [cout][3][7][7]) and db from the slabs.  A block sums 16 consecutive
// elements: thread (g, e) adds the splits g, g + 16, ... of element e in that order (the loads of a
// thread are independent, 64-B coalesced over e), then thread e adds the 16 group sums in group
// order -- a fixed order, so reruns are bit-identical.
__global__ void __launch_bounds__(NT) stem_wgrad_reduce_kernel(const float* __restrict__ slab,
                                                               const float* __restrict__ bslab, int nsplit, int cout,
                                                               float* __restrict__ dw, float* __restrict__ db) {
  __shared__ float part[16][17];
  const int e = threadIdx.x & 15, g = threadIdx.x >> 4;
  const int i = blockIdx.x * 16 + e;
  const int nw = cout * STEM_KV;
  float s = 0.f;
  if (i < nw) {
#pragma unroll 4
    for (int sp = g; sp < nsplit; sp += 16) s += slab[(long)sp * nw + i];
  } else if (i < nw + cout) {
#pragma unroll 4
    for (int sp = g; sp < nsplit; sp += 16) s += bslab[(long)sp * cout + (i - nw)];
  }
  part[g][e] = s;
  __syncthreads();
  if (g != 0) return;
  float t = 0.f;
#pragma unroll
  for (int q = 0; q < 16; ++q) t += part[q][e];
  if (i < nw) {
    const int co = i / STEM_KV, k = i - co * STEM_KV;
    const int rs = k / 3, ci = k - rs * 3;
    const int r = rs / 7, c = rs - r * 7;
    dw[((co * 3 + ci) * 7 + r) * 7 + c] = t;
  } else if (i < nw + cout && db) {
    db[i - nw] = t;
  }
}

int stem_check(int dtype, int n, int h, int w, int cout) {
  FV_SUPPORTED(dtype == FV_F32 || dtype == FV_BF16, "stem7s2: dtype must be FV_F32 or FV_BF16");
  FV_SUPPORTED(n > 0 && h >= 2 && w >= 2 && h % 2 == 0 && w % 2 == 0, "stem7s2: h and w must be even (got %d x %d)",
               h, w);
  FV_SUPPORTED(cout > 0 && cout % 8 == 0, "stem7s2: cout must be a multiple of 8 (got %d)", cout);
  FV_SUPPORTED((long)n * 3 * h * w < (1L << 31) && (long)n * (h / 2) * (w / 2) * cout < (1L << 31),
               "stem7s2: tensor too large for 32-bit indexing");
  return FV_OK;
}

int stem_wg_split(int n, int h, int w) {
  const int nchunk = fv_cdiv((long)n * (h / 2) * (w / 2), STEM_WG_PIX);
  return nchunk < STEM_WG_MAXSPLIT ? nchunk : STEM_WG_MAXSPLIT;
}

// element index -> position in a dense NHWC tensor [n][rows][cols][C] walked in 8-channel chunks;
// 32-bit divisions (the entries reject tensors of 2^31 chunks or more)
struct Pix {
  int cc, x, y;
  long n, pix;
};
__device__ __forceinline__ Pix pix_of(unsigned idx, int C, int rows, int cols) {
  const unsigned cpc = (unsigned)C / 8;
  const unsigned pix = idx / cpc, t = pix / (unsigned)cols, n = t / (unsigned)rows;
  Pix q;
  q.cc = (int)(idx - pix * cpc) * 8;
  q.x = (int)(pix - t * (unsigned)cols);
  q.y = (int)(t - n * (unsigned)rows);
  q.n = n;
  q.pix = pix;
  return q;
}
__device__ __forceinline__ void ld8f(const float* p, float* f) {
  const float4 a = reinterpret_cast<const float4*>(p)[0], b = reinterpret_cast<const float4*>(p)[1];
  f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
}

// ---------------------------------------------------------------- max pool 3x3, stride 2 ----
template <typename T>
__global__ void maxpool3s2_fwd_kernel(const T* __restrict__ x, int H, int W, int C, const float* __restrict__ scale,
                                      const float* __restrict__ shift, float slope, T* __restrict__ y,
                                      uint8_t* __restrict__ am, long total) {
  const unsigned idx = blockIdx.x * NT + threadIdx.x;
  if (idx >= total) return;
  const int Ho = H / 2, Wo = W / 2;
  const Pix q_ = pix_of(idx, C, Ho, Wo);
  const int cc = q_.cc, ox = q_.x, oy = q_.y;
  const long pix = q_.pix, n = q_.n;
  float sc[8], sh[8];
  if (scale) {
    ld8f(scale + cc, sc);
    ld8f(shift + cc, sh);
  }
  float best[8];
  int bi[8];
  const int first = (oy == 0 ? 3 : 0) + (ox == 0 ? 1 : 0);   // first in-bounds tap (torch's start index)
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    best[q] = -INFINITY;
    bi[q] = first;
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const int iy = 2 * oy - 1 + r;
    if (iy < 0 || iy >= H) continue;
#pragma unroll
    for (int s = 0; s < 3; ++s) {
      const int ix = 2 * ox - 1 + s;
      if (ix < 0 || ix >= W) continue;
      Chunk8<T> v;
      v.load(x + ((n * H + iy) * W + ix) * C + cc);
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        float f = v.get(q);
        if (scale) f = Elt<T>::to_f(Elt<T>::from_f(fv_act(f * sc[q] + sh[q], slope)));
        if (f > best[q] || isnan(f)) {      // torch: val > maxval || isnan(val)
          best[q] = f;
          bi[q] = r * 3 + s;
        }
      }
    }
  }
  Chunk8<T> o;
  o.set8(best);
  o.store(y + pix * C + cc);
  uint2 pk;
  pk.x = (uint32_t)bi[0] | ((uint32_t)bi[1] << 8) | ((uint32_t)bi[2] << 16) | ((uint32_t)bi[3] << 24);
  pk.y = (uint32_t)bi[4] | ((uint32_t)bi[5] << 8) | ((uint32_t)bi[6] << 16) | ((uint32_t)bi[7] << 24);
  *reinterpret_cast<uint2*>(am + pix * C + cc) = pk;
}

// gather: input pixel (iy, ix) sums the gradients of the windows (at most 2 x 2) whose argmax it is
template <typename T>
__global__ void maxpool3s2_bwd_kernel(const T* __restrict__ g, const uint8_t* __restrict__ am, int H, int W, int C,
                                      T* __restrict__ dx, long total) {
  const unsigned idx = blockIdx.x * NT + threadIdx.x;
  if (idx >= total) return;
  const int Ho = H / 2, Wo = W / 2;
  const Pix q_ = pix_of(idx, C, H, W);
  const int cc = q_.cc, ix = q_.x, iy = q_.y;
  const long pix = q_.pix, n = q_.n;
  float s[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) s[q] = 0.f;
  const int oy1 = min((iy + 1) >> 1, Ho - 1), ox1 = min((ix + 1) >> 1, Wo - 1);
  for (int oy = iy >> 1; oy <= oy1; ++oy) {
    const int r = iy - (2 * oy - 1);
    for (int ox = ix >> 1; ox <= ox1; ++ox) {
      const int tap = r * 3 + (ix - (2 * ox - 1));
      const long o = ((n * Ho + oy) * Wo + ox) * C + cc;
      const uint2 pk = *reinterpret_cast<const uint2*>(am + o);
      Chunk8<T> gv;
      gv.load(g + o);
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int a = (int)(((q < 4 ? pk.x : pk.y) >> ((q & 3) * 8)) & 0xffu);
        if (a == tap) s[q] += gv.get(q);
      }
    }
  }
  Chunk8<T> o;
  o.set8(s);
  o.store(dx + pix * C + cc);
}

// ---------------------------------------------------------------- subsample by 2 ----
template <typename T>
__global__ void subsample2_fwd_kernel(const T* __restrict__ x, int H, int W, int C, T* __restrict__ y, long total) {
  const unsigned idx = blockIdx.x * NT + threadIdx.x;
  if (idx >= total) return;
  const int Ho = H / 2, Wo = W / 2;
  const Pix q_ = pix_of(idx, C, Ho, Wo);
  const int cc = q_.cc, ox = q_.x, oy = q_.y;
  const long pix = q_.pix, n = q_.n;
  Chunk8<T> v;
  v.load(x + ((n * H + 2 * oy) * W + 2 * ox) * C + cc);
  v.store(y + pix * C + cc);
}

template <typename T>
__global__ void subsample2_bwd_kernel(const T* __restrict__ g, int H, int W, int C, T* __restrict__ dx, long total) {
  const unsigned idx = blockIdx.x * NT + threadIdx.x;
  if (idx >= total) return;
  const int Ho = H / 2, Wo = W / 2;
  const Pix q_ = pix_of(idx, C, H, W);
  const int cc = q_.cc, ix = q_.x, iy = q_.y;
  const long pix = q_.pix, n = q_.n;
  Chunk8<T> v;
  if ((iy & 1) == 0 && (ix & 1) == 0) v.load(g + ((n * Ho + (iy >> 1)) * Wo + (ix >> 1)) * C + cc);
  else v.zero();
  v.store(dx + pix * C + cc);
}

// ---------------------------------------------------------------- bottleneck join ----
template <typename T>
__global__ void bn2_add_relu_kernel(const T* __restrict__ ya, const float* __restrict__ sa,
                                    const float* __restrict__ ha, const T* __restrict__ yb,
                                    const float* __restrict__ sb, const float* __restrict__ hb, int C,
                                    T* __restrict__ out, long total) {
  const unsigned idx = blockIdx.x * NT + threadIdx.x;
  if (idx >= total) return;
  const int cc = (int)(idx % ((unsigned)C / 8)) * 8;
  Chunk8<T> a, b;
  a.load(ya + (long)idx * 8);
  b.load(yb + (long)idx * 8);
  float fsa[8], fha[8], fsb[8], fhb[8];
  ld8f(sa + cc, fsa);
  ld8f(ha + cc, fha);
  if (sb) {
    ld8f(sb + cc, fsb);
    ld8f(hb + cc, fhb);
  }
  float o[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const float va = a.get(q) * fsa[q] + fha[q];
    const float vb = sb ? b.get(q) * fsb[q] + fhb[q] : b.get(q);
    o[q] = fv_act(va + vb, 0.f);
  }
  Chunk8<T> r;
  r.set8(o);
  r.store(out + (long)idx * 8);
}

// out = a + b: the two branch gradients of a bottleneck meeting at its input
template <typename T>
__global__ void add2_kernel(const T* __restrict__ a, const T* __restrict__ b, T* __restrict__ out, long total) {
  const long idx = (long)blockIdx.x * NT + threadIdx.x;
  if (idx >= total) return;
  Chunk8<T> va, vb, r;
  va.load(a + idx * 8);
  vb.load(b + idx * 8);
  float o[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) o[q] = va.get(q) + vb.get(q);
  r.set8(o);
  r.store(out + idx * 8);
}

// ---------------------------------------------------------------- pose head ----
template <typename T>
__global__ void pose_pool_kernel(const T* __restrict__ x, int hw, int C, float* __restrict__ feat, int total) {
  const int i = blockIdx.x * NT + threadIdx.x;
  if (i >= total) return;
  const int n = i / C, c = i - n * C;
  const T* p = x + (long)n * hw * C + c;
  float s = 0.f;
  for (int q = 0; q < hw; ++q) s += Elt<T>::to_f(p[(long)q * C]);
  feat[i] = s / (float)hw;
}

struct PoseHead {
  const float* w[5];
  const float* b[5];
  float* dw[5];
  float* db[5];
  int nb, R;    // R = 3 * nb + 4 rows in all
};

// row r of the stacked five Linear layers -> (head, row within the head)
__device__ __forceinline__ void pose_row(int r, int nb, int& head, int& j) {
  if (r < 3 * nb) {
    head = r / nb;
    j = r - head * nb;
  } else if (r < 3 * nb + 3) {
    head = 3;
    j = r - 3 * nb;
  } else {
    head = 4;
    j = 0;
  }
}

constexpr float POSE_DEG = 3.f * 3.14159265358979323846f / 180.f;

// one wave per (sample, row): logits of the angle heads into prob, t / scale into out[3..6]
__global__ void __launch_bounds__(NT) pose_linear_kernel(PoseHead h, const float* __restrict__ feat, int n, int C,
                                                         float* __restrict__ out, float* __restrict__ prob) {
  const int wv = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (wv >= n * h.R) return;
  const int s = wv / h.R, r = wv - s * h.R;
  int head, j;
  pose_row(r, h.nb, head, j);
  const float* wr = h.w[head] + (long)j * C;
  const float* f = feat + (long)s * C;
  float acc = 0.f;
  for (int c = lane; c < C; c += 64) acc += wr[c] * f[c];
  acc = wave_sum(acc);
  if (lane == 0) {
    const float v = acc + h.b[head][j];
    if (head < 3) prob[((long)s * 3 + head) * h.nb + j] = v;
    else out[s * 7 + 3 + (head - 3) * 3 + j] = v;    // head 3: t0..t2 at 3..5, head 4: scale at 6
  }
}

// one wave per (sample, angle head): softmax in place over nb logits, expectation, angle
__global__ void __launch_bounds__(NT) pose_softmax_kernel(int n, int nb, float* __restrict__ out,
                                                          float* __restrict__ prob) {
  const int wv = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (wv >= n * 3) return;
  float* p = prob + (long)wv * nb;
  float m = -INFINITY;
  for (int j = lane; j < nb; j += 64) m = fmaxf(m, p[j]);
  m = wave_max(m);
  float z = 0.f;
  for (int j = lane; j < nb; j += 64) z += expf(p[j] - m);
  z = wave_sum(z);
  float e = 0.f;
  for (int j = lane; j < nb; j += 64) {
    const float q = expf(p[j] - m) / z;
    p[j] = q;
    e += q * (float)j;
  }
  e = wave_sum(e);
  if (lane == 0) {
    const int s = wv / 3, head = wv - s * 3;
    out[s * 7 + head] = (e - (float)(nb / 2)) * POSE_DEG;
  }
}

// dlogit [n][R]: angle heads g * deg * p_j (j - E), t / scale rows the incoming gradient
__global__ void __launch_bounds__(NT) pose_dlogit_kernel(int n, int nb, int R, const float* __restrict__ g_out,
                                                         const float* __restrict__ prob, float* __restrict__ dl) {
  const int wv = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (wv >= n * 4) return;
  const int s = wv >> 2, head = wv & 3;
  if (head == 3) {
    if (lane < 4) dl[(long)s * R + 3 * nb + lane] = g_out[s * 7 + 3 + lane];
    return;
  }
  const float* p = prob + ((long)s * 3 + head) * nb;
  float e = 0.f;
  for (int j = lane; j < nb; j += 64) e += p[j] * (float)j;
  e = wave_sum(e);
  const float ge = g_out[s * 7 + head] * POSE_DEG;
  for (int j = lane; j < nb; j += 64) dl[(long)s * R + head * nb + j] = ge * p[j] * ((float)j - e);
}

// dW[r][c] = sum_n dlogit[n][r] feat[n][c], db[r] = sum_n dlogit[n][r] (sample order)
__global__ void pose_dw_kernel(PoseHead h, int n, int C, const float* __restrict__ dl,
                               const float* __restrict__ feat) {
  const int i = blockIdx.x * NT + threadIdx.x;
  if (i >= h.R * (C + 1)) return;
  const int r = i / (C + 1), c = i - r * (C + 1);
  int head, j;
  pose_row(r, h.nb, head, j);
  float s = 0.f;
  if (c < C) {
    for (int q = 0; q < n; ++q) s += dl[(long)q * h.R + r] * feat[(long)q * C + c];
    h.dw[head][(long)j * C + c] = s;
  } else {
    for (int q = 0; q < n; ++q) s += dl[(long)q * h.R + r];
    h.db[head][j] = s;
  }
}

// dfeat[n][c] / hw = sum_r dlogit[n][r] W[r][c] / hw (row order; the loads of a head's rows are
// independent of each other, so the unrolled loop keeps several in flight)
__global__ void pose_dfeat_kernel(PoseHead h, int n, int C, int hw, const float* __restrict__ dl,
                                  float* __restrict__ df) {
  const int i = blockIdx.x * NT + threadIdx.x;
  if (i >= n * C) return;
  const int s = i / C, c = i - s * C;
  const float* d = dl + (long)s * h.R;
  float acc = 0.f;
  int r0 = 0;
  for (int head = 0; head < 5; ++head) {
    const int rows = head < 3 ? h.nb : (head == 3 ? 3 : 1);
    const float* w = h.w[head] + c;
#pragma unroll 8
    for (int j = 0; j < rows; ++j) acc += d[r0 + j] * w[(long)j * C];
    r0 += rows;
  }
  df[i] = acc / (float)hw;
}

template <typename T>
__global__ void pose_dx_kernel(const float* __restrict__ df, int hw, int C, T* __restrict__ dx, long total) {
  const unsigned idx = blockIdx.x * NT + threadIdx.x;
  if (idx >= total) return;
  const unsigned cpc = (unsigned)C / 8, pix = idx / cpc;
  const int cc = (int)(idx - pix * cpc) * 8;
  const long n = pix / (unsigned)hw;
  Chunk8<T> o;
  o.set8(df + n * C + cc);
  o.store(dx + (long)idx * 8);
}

int nhwc_check(const char* what, int dtype, int n, int h, int w, int c, bool even) {
  FV_SUPPORTED(dtype == FV_F32 || dtype == FV_BF16, "%s: dtype must be FV_F32 or FV_BF16", what);
  FV_SUPPORTED(n > 0 && h > 0 && w > 0 && (!even || (h % 2 == 0 && w % 2 == 0)),
               "%s: h and w must be even (got %d x %d)", what, h, w);
  FV_SUPPORTED(c > 0 && c % 8 == 0, "%s: channels must be a multiple of 8 (got %d)", what, c);
  FV_SUPPORTED((long)n * h * w * (c / 8) < (1L << 31), "%s: tensor too large for 32-bit indexing", what);
  return FV_OK;
}

int pose_check(int n, int c, int n_bins) {
  FV_SUPPORTED(n > 0 && c > 0 && c % 8 == 0, "pose head: channels must be a multiple of 8 (got %d)", c);
  FV_SUPPORTED(n_bins > 0 && n_bins <= 4096, "pose head: n_bins must be in [1, 4096] (got %d)", n_bins);
  FV_SUPPORTED((long)n * (3 * n_bins + 4) < (1L << 24) && (long)n * c < (1L << 28) &&
                   (long)(3 * n_bins + 4) * (c + 1) < (1L << 31),
               "pose head: batch or layer too large");
  return FV_OK;
}

}  // namespace

#define DISPATCH(dtype, kernel, grid, s, ...)                                              \
  do {                                                                                     \
    if ((dtype) == FV_BF16) hipLaunchKernelGGL(kernel<bf16>, grid, dim3(NT), 0, s, __VA_ARGS__); \
    else hipLaunchKernelGGL(kernel<float>, grid, dim3(NT), 0, s, __VA_ARGS__);            \
  } while (0)

extern "C" {

size_t fv_stem7s2_wk_elems(int cout) {
  if (cout <= 0 || cout % 8) return 0;
  return (size_t)fv_cdiv(cout, 16) * 16 * STEM_K;
}

int fv_stem7s2_weight_prep(int dtype, const float* w, int cout, void* wk, void* stream) {
  int st = stem_check(dtype, 1, 2, 2, cout);
  if (st) return st;
  FV_REQUIRE(w && wk, "stem7s2_weight_prep: null pointer");
  const int cpad = fv_cdiv(cout, 16) * 16;
  const dim3 grid(fv_cdiv((long)cpad * STEM_K, NT));
  hipStream_t s = (hipStream_t)stream;
  if (dtype == FV_BF16) hipLaunchKernelGGL(stem_weight_prep_kernel<bf16>, grid, dim3(NT), 0, s, w, cout, cpad, (bf16*)wk);
  else hipLaunchKernelGGL(stem_weight_prep_kernel<float>, grid, dim3(NT), 0, s, w, cout, cpad, (float*)wk);
  return fv_check_launch("stem7s2_weight_prep");
}

int fv_stem7s2_stats_blocks(int n, int h, int w) {
  if (n <= 0 || h < 2 || w < 2 || h % 2 || w % 2) return 0;
  return fv_cdiv((long)n * (h / 2) * (w / 2), STEM_REC);
}

int fv_stem7s2_stats_block_pixels(void) { return STEM_REC; }

int fv_stem7s2_fwd(int dtype, const float* x, int n, int h, int w, int cout, const void* wk, const float* bias,
                   void* y, float* stats, void* stream) {
  int st = stem_check(dtype, n, h, w, cout);
  if (st) return st;
  FV_REQUIRE(x && wk && y, "stem7s2_fwd: null pointer");
  StemArgs a{};
  a.x = x; a.wk = wk; a.bias = bias; a.y = y; a.stats = stats;
  a.N = n; a.H = h; a.W = w; a.Ho = h / 2; a.Wo = w / 2; a.P = n * a.Ho * a.Wo; a.Cout = cout;
  a.nct = fv_cdiv(cout, 16);
  a.nrec = fv_cdiv(a.P, STEM_REC);
  const dim3 grid(fv_cdiv(a.P, 4 * STEM_RM * STEM_REC));
  DISPATCH(dtype, stem_fwd_kernel, grid, (hipStream_t)stream, a);
  return fv_check_launch("stem7s2_fwd");
}

size_t fv_stem7s2_wgrad_ws_bytes(int n, int h, int w, int cout) {
  if (n <= 0 || h < 2 || w < 2 || h % 2 || w % 2 || cout <= 0 || cout % 8) return 0;
  return (size_t)stem_wg_split(n, h, w) * cout * (STEM_KV + 1) * sizeof(float);
}

int fv_stem7s2_bwd_weight(int dtype, const float* x, const void* dy, int n, int h, int w, int cout, float* dw,
                          float* db, void* ws, void* stream) {
  int st = stem_check(dtype, n, h, w, cout);
  if (st) return st;
  FV_REQUIRE(x && dy && dw && ws, "stem7s2_bwd_weight: null pointer");
  StemWgArgs a{};
  a.x = x; a.dy = dy;
  a.N = n; a.H = h; a.W = w; a.Ho = h / 2; a.Wo = w / 2; a.P = n * a.Ho * a.Wo; a.Cout = cout;
  a.nchunk = fv_cdiv(a.P, STEM_WG_PIX);
  a.nsplit = stem_wg_split(n, h, w);
  a.slab = (float*)ws;
  a.bslab = a.slab + (size_t)a.nsplit * cout * STEM_KV;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(a.nsplit, fv_cdiv(cout, 64));
  DISPATCH(dtype, stem_wgrad_kernel, grid, s, a);
  if ((st = fv_check_launch("stem7s2_bwd_weight"))) return st;
  hipLaunchKernelGGL(stem_wgrad_reduce_kernel, dim3(fv_cdiv((long)cout * (STEM_KV + 1), 16)), dim3(NT), 0, s, a.slab,
                     a.bslab, a.nsplit, cout, dw, db);
  return fv_check_launch("stem7s2_wgrad_reduce");
}

int fv_maxpool3s2_fwd(int dtype, const void* x, int n, int h, int w, int c, const float* scale, const float* shift,
                      float slope, void* y, uint8_t* argmax, void* stream) {
  int st = nhwc_check("maxpool3s2_fwd", dtype, n, h, w, c, true);
  if (st) return st;
  FV_REQUIRE(x && y && argmax, "maxpool3s2_fwd: null pointer");
  FV_REQUIRE(!scale || (shift && fv_slope_ok(slope)), "maxpool3s2_fwd: prologue needs shift and a slope in [0, 1]");
  const long total = (long)n * (h / 2) * (w / 2) * (c / 8);
  const dim3 grid(fv_cdiv(total, NT));
  hipStream_t s = (hipStream_t)stream;
  if (dtype == FV_BF16)
    hipLaunchKernelGGL(maxpool3s2_fwd_kernel<bf16>, grid, dim3(NT), 0, s, (const bf16*)x, h, w, c, scale, shift, slope,
                       (bf16*)y, argmax, total);
  else
    hipLaunchKernelGGL(maxpool3s2_fwd_kernel<float>, grid, dim3(NT), 0, s, (const float*)x, h, w, c, scale, shift,
                       slope, (float*)y, argmax, total);
  return fv_check_launch("maxpool3s2_fwd");
}

int fv_maxpool3s2_bwd(int dtype, const void* g, const uint8_t* argmax, int n, int h, int w, int c, void* dx,
                      void* stream) {
  int st = nhwc_check("maxpool3s2_bwd", dtype, n, h, w, c, true);
  if (st) return st;
  FV_REQUIRE(g && argmax && dx, "maxpool3s2_bwd: null pointer");
  const long total = (long)n * h * w * (c / 8);
  const dim3 grid(fv_cdiv(total, NT));
  hipStream_t s = (hipStream_t)stream;
  if (dtype == FV_BF16)
    hipLaunchKernelGGL(maxpool3s2_bwd_kernel<bf16>, grid, dim3(NT), 0, s, (const bf16*)g, argmax, h, w, c, (bf16*)dx,
                       total);
  else
    hipLaunchKernelGGL(maxpool3s2_bwd_kernel<float>, grid, dim3(NT), 0, s, (const float*)g, argmax, h, w, c,
                       (float*)dx, total);
  return fv_check_launch("maxpool3s2_bwd");
}

int fv_subsample2_fwd(int dtype, const void* x, int n, int h, int w, int c, void* y, void* stream) {
  int st = nhwc_check("subsample2_fwd", dtype, n, h, w, c, true);
  if (st) return st;
  FV_REQUIRE(x && y, "subsample2_fwd: null pointer");
  const long total = (long)n * (h / 2) * (w / 2) * (c / 8);
  const dim3 grid(fv_cdiv(total, NT));
  hipStream_t s = (hipStream_t)stream;
  if (dtype == FV_BF16)
    hipLaunchKernelGGL(subsample2_fwd_kernel<bf16>, grid, dim3(NT), 0, s, (const bf16*)x, h, w, c, (bf16*)y, total);
  else
    hipLaunchKernelGGL(subsample2_fwd_kernel<float>, grid, dim3(NT), 0, s, (const float*)x, h, w, c, (float*)y, total);
  return fv_check_launch("subsample2_fwd");
}

int fv_subsample2_bwd(int dtype, const void* g, int n, int h, int w, int c, void* dx, void* stream) {
  int st = nhwc_check("subsample2_bwd", dtype, n, h, w, c, true);
  if (st) return st;
  FV_REQUIRE(g && dx, "subsample2_bwd: null pointer");
  const long total = (long)n * h * w * (c / 8);
  const dim3 grid(fv_cdiv(total, NT));
  hipStream_t s = (hipStream_t)stream;
  if (dtype == FV_BF16)
    hipLaunchKernelGGL(subsample2_bwd_kernel<bf16>, grid, dim3(NT), 0, s, (const bf16*)g, h, w, c, (bf16*)dx, total);
  else
    hipLaunchKernelGGL(subsample2_bwd_kernel<float>, grid, dim3(NT), 0, s, (const float*)g, h, w, c, (float*)dx, total);
  return fv_check_launch("subsample2_bwd");
}

int fv_bn2_add_relu_fwd(int dtype, const void* ya, const float* sa, const float* ha, const void* yb, const float* sb,
                        const float* hb, long pixels, int c, void* out, void* stream) {
  FV_SUPPORTED(pixels > 0 && pixels < (1L << 31), "bn2_add_relu: bad pixel count");
  int st = nhwc_check("bn2_add_relu_fwd", dtype, 1, 1, (int)pixels, c, false);
  if (st) return st;
  FV_REQUIRE(ya && sa && ha && yb && out && (!sb || hb), "bn2_add_relu_fwd: null pointer");
  const long total = pixels * (c / 8);
  const dim3 grid(fv_cdiv(total, NT));
  hipStream_t s = (hipStream_t)stream;
  if (dtype == FV_BF16)
    hipLaunchKernelGGL(bn2_add_relu_kernel<bf16>, grid, dim3(NT), 0, s, (const bf16*)ya, sa, ha, (const bf16*)yb, sb,
                       hb, c, (bf16*)out, total);
  else
    hipLaunchKernelGGL(bn2_add_relu_kernel<float>, grid, dim3(NT), 0, s, (const float*)ya, sa, ha, (const float*)yb,
                       sb, hb, c, (float*)out, total);
  return fv_check_launch("bn2_add_relu_fwd");
}

int fv_add2(int dtype, const void* a, const void* b, long n, void* out, void* stream) {
  FV_SUPPORTED(dtype == FV_F32 || dtype == FV_BF16, "add2: dtype must be FV_F32 or FV_BF16");
  FV_SUPPORTED(n > 0 && n % 8 == 0, "add2: the element count must be a multiple of 8 (got %ld)", n);
  FV_REQUIRE(a && b && out, "add2: null pointer");
  const long total = n / 8;
  FV_SUPPORTED(total < (long)NT * 0x7fffffffL, "add2: tensor too large");
  const dim3 grid(fv_cdiv(total, NT));
  hipStream_t s = (hipStream_t)stream;
  if (dtype == FV_BF16)
    hipLaunchKernelGGL(add2_kernel<bf16>, grid, dim3(NT), 0, s, (const bf16*)a, (const bf16*)b, (bf16*)out, total);
  else
    hipLaunchKernelGGL(add2_kernel<float>, grid, dim3(NT), 0, s, (const float*)a, (const float*)b, (float*)out, total);
  return fv_check_launch("add2");
}

int fv_pose_pool_fwd(int dtype, const void* x, int n, int hw, int c, float* feat, void* stream) {
  int st = nhwc_check("pose_pool_fwd", dtype, n, 1, hw, c, false);
  if (st) return st;
  FV_SUPPORTED((long)n * c < (1L << 28), "pose_pool_fwd: batch too large");
  FV_REQUIRE(x && feat, "pose_pool_fwd: null pointer");
  const int total = n * c;
  const dim3 grid(fv_cdiv(total, NT));
  hipStream_t s = (hipStream_t)stream;
  if (dtype == FV_BF16)
    hipLaunchKernelGGL(pose_pool_kernel<bf16>, grid, dim3(NT), 0, s, (const bf16*)x, hw, c, feat, total);
  else
    hipLaunchKernelGGL(pose_pool_kernel<float>, grid, dim3(NT), 0, s, (const float*)x, hw, c, feat, total);
  return fv_check_launch("pose_pool_fwd");
}

int fv_pose_head_fwd(const float* feat, int n, int c, int n_bins, const float* const* w, const float* const* b,
                     float* out, float* prob, void* stream) {
  int st = pose_check(n, c, n_bins);
  if (st) return st;
  FV_REQUIRE(feat && w && b && out && prob, "pose_head_fwd: null pointer");
  PoseHead h{};
  for (int i = 0; i < 5; ++i) {
    FV_REQUIRE(w[i] && b[i], "pose_head_fwd: null weight or bias");
    h.w[i] = w[i];
    h.b[i] = b[i];
  }
  h.nb = n_bins;
  h.R = 3 * n_bins + 4;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(pose_linear_kernel, dim3(fv_cdiv((long)n * h.R, 4)), dim3(NT), 0, s, h, feat, n, c, out, prob);
  if ((st = fv_check_launch("pose_linear"))) return st;
  hipLaunchKernelGGL(pose_softmax_kernel, dim3(fv_cdiv((long)n * 3, 4)), dim3(NT), 0, s, n, n_bins, out, prob);
  return fv_check_launch("pose_softmax");
}

size_t fv_pose_head_ws_bytes(int n, int c, int n_bins) {
  if (n <= 0 || c <= 0 || n_bins <= 0) return 0;
  return ((size_t)n * (3 * n_bins + 4) + (size_t)n * c) * sizeof(float);
}

int fv_pose_head_bwd(int dtype, const float* g_out, const float* feat, const float* prob, int n, int hw, int c,
                     int n_bins, const float* const* w, float* const* dw, float* const* db, void* dx, void* ws,
                     void* stream) {
  int st = pose_check(n, c, n_bins);
  if (st) return st;
  if ((st = nhwc_check("pose_head_bwd", dtype, n, 1, hw, c, false))) return st;
  FV_REQUIRE(g_out && feat && prob && w && dw && db && dx && ws, "pose_head_bwd: null pointer");
  PoseHead h{};
  for (int i = 0; i < 5; ++i) {
    FV_REQUIRE(w[i] && dw[i] && db[i], "pose_head_bwd: null weight or gradient");
    h.w[i] = w[i];
    h.dw[i] = dw[i];
    h.db[i] = db[i];
  }
  h.nb = n_bins;
  h.R = 3 * n_bins + 4;
  float* dl = (float*)ws;
  float* df = dl + (size_t)n * h.R;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(pose_dlogit_kernel, dim3(n), dim3(NT), 0, s, n, n_bins, h.R, g_out, prob, dl);
  if ((st = fv_check_launch("pose_dlogit"))) return st;
  hipLaunchKernelGGL(pose_dw_kernel, dim3(fv_cdiv((long)h.R * (c + 1), NT)), dim3(NT), 0, s, h, n, c, dl, feat);
  if ((st = fv_check_launch("pose_dw"))) return st;
  hipLaunchKernelGGL(pose_dfeat_kernel, dim3(fv_cdiv((long)n * c, NT)), dim3(NT), 0, s, h, n, c, hw, dl, df);
  if ((st = fv_check_launch("pose_dfeat"))) return st;
  const long total = (long)n * hw * (c / 8);
  const dim3 grid(fv_cdiv(total, NT));
  if (dtype == FV_BF16) hipLaunchKernelGGL(pose_dx_kernel<bf16>, grid, dim3(NT), 0, s, df, hw, c, (bf16*)dx, total);
  else hipLaunchKernelGGL(pose_dx_kernel<float>, grid, dim3(NT), 0, s, df, hw, c, (float*)dx, total);
  return fv_check_launch("pose_dx");
}

}  // extern "C"
