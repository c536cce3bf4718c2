// ========================================================================================
// fp8 (OCP e4m3) conv path: per-tensor scaled operands on v_mfma_scale_f32_16x16x128_f8f6f4
// (BASELINE config C5).  Forward and data gradient of the 3x3 convs with 128-multiple channel
// counts (ResBlock2D x 12 + Generator.in_conv: 58 % of the step's FLOPs) run on fp8 operands
// with fp32 accumulation; the weight gradient stays bf16 (its operands, the bf16 activations
// and gradients, are kept for it anyway).
//   Scaling: every fp8 tensor carries a power-of-two scale s = 2^floor(log2(448 / amax)) so
//   that |v * s| <= 448 (e4m3 max); dq = 1 / s is stored on the device and the conv epilogue
//   multiplies the fp32 accumulators by dq_x * dq_w (exact: powers of two).
//
// This file: the whole fp8 path -- the quantisation and delayed-scaling site kernels, the fp8
// weight preparation, conv3_halo_fp8 and conv3_wgrad_fp8, the two probes and every fv_*fp8*
// entry.  From conv.hip it calls check_desc, res_sched, sr_geometry and plan_wgrad (declared in
// conv_plan.h), and launch_wgrad_reduce of conv_wgrad.hip.
// ========================================================================================
#include "conv_plan.h"

// data-parallel fp8 (fv_fp8_set_deferred_roll): the *_site convs leave the in-flight amax in the
// site; the caller all-reduces (MAX) every site's amax once per step and rolls them together
static int g_fp8_defer_roll = 0;

namespace {

constexpr int FP8_NPART = 1024;   // amax partials (blocks of the amax pass)

// block bid of nblk: max |x| over its grid-stride share -> part[bid]
template <typename T>
__device__ __forceinline__ void amax_body(const T* __restrict__ x, long n, float* part, int bid, int nblk) {
  float m = 0.f;
  for (long i = bid * 256L + threadIdx.x; i * 8 < n; i += (long)nblk * 256) {
    const long e = i * 8;
    if (e + 8 <= n) {
      Chunk8<T> c;
      c.load(x + e);
#pragma unroll
      for (int j = 0; j < 8; ++j) m = fmaxf(m, fabsf(c.get(j)));
    } else {
      for (long j = e; j < n; ++j) m = fmaxf(m, fabsf(Elt<T>::to_f(x[j])));
    }
  }
  m = wave_max(m);
  __shared__ float red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) part[bid] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

template <typename T>
__global__ void __launch_bounds__(256) amax_kernel(const T* __restrict__ x, long n, float* part) {
  amax_body<T>(x, n, part, blockIdx.x, gridDim.x);
}

// every block reduces the partials itself (1024 floats from L2), block 0 publishes dq
__device__ __forceinline__ float amax_of_parts(const float* part, int np, float* sh) {
  float m = 0.f;
  for (int i = threadIdx.x; i < np; i += blockDim.x) m = fmaxf(m, part[i]);
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = m;
  __syncthreads();
  float r = 0.f;
  for (int w = 0; w < (int)(blockDim.x >> 6); ++w) r = fmaxf(r, sh[w]);
  return r;
}

template <typename T>
__global__ void __launch_bounds__(256) quantize_fp8_kernel(const T* __restrict__ x, long n, const float* part, int np,
                                                           uint8_t* __restrict__ y, float* dq) {
  __shared__ float sh[4];
  const float s = pow2_scale_of(amax_of_parts(part, np, sh));
  if (blockIdx.x == 0 && threadIdx.x == 0) dq[0] = 1.f / s;
  for (long i = blockIdx.x * 256L + threadIdx.x; i * 8 < n; i += (long)gridDim.x * 256) {
    const long e = i * 8;
    if (e + 8 <= n) {
      Chunk8<T> c;
      c.load(x + e);
      uint2 o;
      o.x = pack4_fp8(c.get(0) * s, c.get(1) * s, c.get(2) * s, c.get(3) * s);
      o.y = pack4_fp8(c.get(4) * s, c.get(5) * s, c.get(6) * s, c.get(7) * s);
      *reinterpret_cast<uint2*>(y + e) = o;
    } else {
      for (long j = e; j < n; ++j) {
        const int v = __builtin_amdgcn_cvt_pk_fp8_f32(Elt<T>::to_f(x[j]) * s, 0.f, 0, false);
        y[j] = (uint8_t)(v & 0xff);
      }
    }
  }
}

// ---- delayed scaling (per operand site: a conv's activation or output-gradient operand) ----
// site = uint32[FP8_SITE]: [0, 16) amax history (float bits), [16] amax of the call in flight
// (float bits, atomicMax: deterministic, max is order-free), [17] history write index, [18] dq
// of the call in flight.  A call quantizes with s = pow2 scale of max(history) in ONE pass
// (values beyond 448 / s saturate, as delayed scaling does) and accumulates its own amax; the
// conv consuming the operand moves that amax into the history (fp8_site_roll, block 0 at its
// start: every quantize block has finished by then and only dq is read concurrently).  The
// site's first call quantizes exactly (amax pass + quantize pass) and fills the history.
__device__ __forceinline__ void fp8_site_roll(unsigned* st) {
  const unsigned p = st[17] % FP8_HIST;
  st[p] = st[16];
  st[16] = 0u;
  st[17] = p + 1;
}
// exact first call: fills the whole history with this call's amax
__global__ void fp8_site_seed_kernel(const float* part, int np, unsigned* st) {
  __shared__ float sh[4];
  const float m = amax_of_parts(part, np, sh);
  if (threadIdx.x < FP8_HIST) st[threadIdx.x] = __float_as_uint(m);
  if (threadIdx.x == 0) {
    st[16] = 0u;
    st[17] = 0u;
  }
}

// data-parallel global scaling (fv_fp8_set_deferred_roll): the sites' in-flight amax words,
// gathered into one float vector (all-reduced MAX across ranks by the caller), then rolled into
// every site's history at once -- identical histories, so identical scales, on every rank
__global__ void fp8_sites_inflight_kernel(int n, const unsigned long long* __restrict__ sites, float* amax) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) amax[i] = __uint_as_float(reinterpret_cast<const unsigned*>(sites[i])[16]);
}
__global__ void fp8_sites_roll_kernel(int n, const unsigned long long* __restrict__ sites, const float* amax) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  unsigned* st = reinterpret_cast<unsigned*>(sites[i]);
  st[16] = __float_as_uint(amax[i]);
  fp8_site_roll(st);
}
// a site's first call under global scaling: the history filled with a given (all-reduced) amax
__global__ void fp8_site_seed_from_kernel(const float* amax, unsigned* st) {
  if (threadIdx.x < FP8_HIST) st[threadIdx.x] = __float_as_uint(amax[0]);
  if (threadIdx.x == 0) {
    st[16] = 0u;
    st[17] = 0u;
  }
}
// amax of the partials -> one float
__global__ void fp8_amax_final_kernel(const float* part, int np, float* out) {
  __shared__ float sh[4];
  const float m = amax_of_parts(part, np, sh);
  if (threadIdx.x == 0) out[0] = m;
}

template <typename T>
__global__ void __launch_bounds__(256) quantize_fp8_delayed_kernel(const T* __restrict__ x, long n, unsigned* st,
                                                                   uint8_t* __restrict__ y) {
  const float s = pow2_scale_of(site_hist_max(st));
  if (blockIdx.x == 0 && threadIdx.x == 0) st[18] = __float_as_uint(1.f / s);
  float m = 0.f;
  for (long i = blockIdx.x * 256L + threadIdx.x; i * 8 < n; i += (long)gridDim.x * 256) {
    const long e = i * 8;
    if (e + 8 <= n) {
      Chunk8<T> c;
      c.load(x + e);
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        v[j] = c.get(j);
        m = fmaxf(m, fabsf(v[j]));
        v[j] = fminf(fmaxf(v[j] * s, -448.f), 448.f);
      }
      uint2 o;
      o.x = pack4_fp8(v[0], v[1], v[2], v[3]);
      o.y = pack4_fp8(v[4], v[5], v[6], v[7]);
      *reinterpret_cast<uint2*>(y + e) = o;
    } else {
      for (long j = e; j < n; ++j) {
        const float f = Elt<T>::to_f(x[j]);
        m = fmaxf(m, fabsf(f));
        const int q = __builtin_amdgcn_cvt_pk_fp8_f32(fminf(fmaxf(f * s, -448.f), 448.f), 0.f, 0, false);
        y[j] = (uint8_t)(q & 0xff);
      }
    }
  }
  m = wave_max(m);
  __shared__ float red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0)
    atomicMax(st + 16, __float_as_uint(fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]))));
}

// fp8 weights: wk [rows][9 cin] (k = tap * cin + ci) and / or the transposed, flipped wt
// [rows_t][9 cout] (k = tap' * cout + co), both scaled by s = pow2 scale of amax(|w| / sigma);
// dq[0] = 1 / s.  The amax partials of |w| come from amax_kernel<float> over w_param.
__device__ __forceinline__ void weight_prep_fp8_body(const float* __restrict__ wp, const float* sigma,
                                                     const float* part, int np, uint8_t* wk, int rows, uint8_t* wt,
                                                     int rows_t, int cout, int cin, float* dq, int bid, int nblk) {
  __shared__ float sh[4];
  const float inv = sigma ? 1.f / sigma[0] : 1.f;
  const float s = pow2_scale_of(amax_of_parts(part, np, sh) * inv);
  if (bid == 0 && threadIdx.x == 0) dq[0] = 1.f / s;
  const long nk = wk ? (long)rows * 9 * cin : 0, nt = wt ? (long)rows_t * 9 * cout : 0;
  for (long e = bid * 256L + threadIdx.x; e < nk + nt; e += (long)nblk * 256) {
    float v = 0.f;
    uint8_t* dst;
    if (e < nk) {
      const int row = (int)(e / (9 * cin)), k = (int)(e - (long)row * 9 * cin);
      const int tap = k / cin, ci = k - tap * cin;
      if (row < cout) v = wp[((long)row * cin + ci) * 9 + tap];
      dst = wk + e;
    } else {
      const long e2 = e - nk;
      const int row = (int)(e2 / (9 * cout)), k = (int)(e2 - (long)row * 9 * cout);
      const int tap = k / cout, co = k - tap * cout;
      if (row < cin) v = wp[((long)co * cin + row) * 9 + (8 - tap)];
      dst = wt + e2;
    }
    const int q = __builtin_amdgcn_cvt_pk_fp8_f32(v * inv * s, 0.f, 0, false);
    *dst = (uint8_t)(q & 0xff);
  }
}

__global__ void __launch_bounds__(256) weight_prep_fp8_kernel(const float* __restrict__ wp, const float* sigma,
                                                              const float* part, int np, uint8_t* wk, int rows,
                                                              uint8_t* wt, int rows_t, int cout, int cin, float* dq) {
  weight_prep_fp8_body(wp, sigma, part, np, wk, rows, wt, rows_t, cout, cin, dq, blockIdx.x, gridDim.x);
}

// the e4m3 weights of many convs in two launches (fv_conv_weight_prep_fp8_multi): blockIdx.y
// selects the conv, its amax partials live at ws + y * stride
struct W8Job {
  const float* w;
  const float* sigma;
  uint8_t *wk, *wt;
  float* dq;
  long nw;
  int cout, cin, nb, nb2;
};
struct W8Multi {
  int n, stride;
  W8Job j[FV_WPREP_MAX];
};
__global__ void __launch_bounds__(256) amax_multi_kernel(W8Multi m, float* ws) {
  const W8Job& j = m.j[blockIdx.y];
  if ((int)blockIdx.x >= j.nb) return;
  amax_body<float>(j.w, j.nw, ws + (long)blockIdx.y * m.stride, blockIdx.x, j.nb);
}
__global__ void __launch_bounds__(256) weight_prep_fp8_multi_kernel(W8Multi m, const float* ws) {
  const W8Job& j = m.j[blockIdx.y];
  if ((int)blockIdx.x >= j.nb2) return;
  weight_prep_fp8_body(j.w, j.sigma, ws + (long)blockIdx.y * m.stride, j.nb, j.wk, j.cout, j.wt, j.cin, j.cout, j.cin,
                       j.dq, blockIdx.x, j.nb2);
}

typedef int v8i __attribute__((ext_vector_type(8)));

__device__ __forceinline__ f32x4 mma_f8(const v8i& a, const v8i& b, f32x4 c) {
  // OCP e4m3 x e4m3 (cbsz = blgp = 0), unit block scales (e8m0 127 = 2^0)
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, 0, 0, 0, 127, 0, 127);
}

// one 16 x 16 x 128 tile, fragments in the layout the conv kernel uses: lane (r = l & 15,
// g = l >> 4) holds k {16g .. 16g+15} U {64+16g .. 64+16g+15} of A row r and of B column r.
// a [16][128], b [16][128] (b stored column-major: b[col][k]); c [16][16] row-major.
__global__ void fp8_mfma_probe_kernel(const uint8_t* a, const uint8_t* b, float* c) {
  const int l = threadIdx.x, r = l & 15, g = l >> 4;
  v8i fa, fb;
  const uint4 a0 = *reinterpret_cast<const uint4*>(a + r * 128 + 16 * g);
  const uint4 a1 = *reinterpret_cast<const uint4*>(a + r * 128 + 64 + 16 * g);
  const uint4 b0 = *reinterpret_cast<const uint4*>(b + r * 128 + 16 * g);
  const uint4 b1 = *reinterpret_cast<const uint4*>(b + r * 128 + 64 + 16 * g);
  fa = v8i{(int)a0.x, (int)a0.y, (int)a0.z, (int)a0.w, (int)a1.x, (int)a1.y, (int)a1.z, (int)a1.w};
  fb = v8i{(int)b0.x, (int)b0.y, (int)b0.z, (int)b0.w, (int)b1.x, (int)b1.y, (int)b1.z, (int)b1.w};
  f32x4 acc = mma_f8(fa, fb, f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
  for (int i = 0; i < 4; ++i) c[(4 * g + i) * 16 + r] = acc[i];
}

// ds_read_b64_tr_b8 probe (tests/test_fp8_gpu.py pins its lane mapping before any kernel relies
// on it): LDS byte i = i & 255 over 4 KB, lane l reads 8 transposed bytes at lane_addr[l]
typedef int v2i_t __attribute__((ext_vector_type(2)));
__global__ void tr8_probe_kernel(const int* lane_addr, int* out) {
  __shared__ __attribute__((aligned(16))) unsigned char sm[4096];
  for (int i = threadIdx.x; i < 4096; i += 64) sm[i] = (unsigned char)(i & 255);
  __syncthreads();
  const v2i_t v = __builtin_amdgcn_ds_read_tr8_b64_v2i32((FV_LDS v2i_t*)(sm + lane_addr[threadIdx.x]));
  out[2 * threadIdx.x] = v[0];
  out[2 * threadIdx.x + 1] = v[1];
}

// fp8 3x3 conv, halo-staged input (the structure of conv3_halo_fwd with a 128-channel k step):
//   k step ks = (128-channel chunk c = ks / 9, tap t = ks % 9);
//   weights stage [BN rows][128 B] (one tap x 128 ci), 16-B chunks XOR swz8(row): fragment
//   chunks g and 4 + g (the conflict-free pattern of conv_fwd_v2's 128-B rows);
//   halo of chunk c = two images (ci 0-63 / 64-127) of [(TR+2) x 66 px][64 B], h3swz chunk
//   swizzle (conflict-free fragment reads from any start), double-buffered across chunks.
// Block: BN = 128 co x BM = 256 px (4 rows x 64), 8 waves 2 (co) x 4 (px), wave 64 x 64.
// NSW: weight stages in the ring, issued NSW - 1 taps ahead (2; 3 measured slower, r4: res fwd
// / dgrad at B = 64 195 / 177 -> 199-202 / 182-185 us, fp8 step 22.36 -> 22.69 ms)
// SCH bit 1 (stagger, bit-identical): waves NW/2.. keep a tap's fragments across the next
// barrier and run its MFMAs right after it, while their SIMD partners issue the DMA and read
// their fragments; they then issue their own DMA and reads under the partners' MFMAs.
// SCH bit 0: one static s_setprio 1 for waves NW/2.. instead of the flips around each cluster.
template <int WN, int WM, int RN, int RM, int NSW = 2, int SCH = 0>
__global__ void __launch_bounds__(64 * WN * WM, 1)
conv3_halo_fp8(ConvArgs a, unsigned x_bytes) {
  constexpr int NW = WN * WM;
  constexpr int BN = WN * RN * 16, BM = WM * RM * 16, TR = BM / 64;
  constexpr int HP = (TR + 2) * 66, HQ = (HP + 15) / 16;      // pieces per 64-B halo image
  constexpr int HALO = 2 * HQ * 1024;                          // both images of one chunk
  constexpr int QH = 2 * HQ, JH = (QH + NW - 1) / NW;
  constexpr int BST = BN * 128, QB = BN / 8, JB = QB / NW;
  static_assert(QB % NW == 0, "weight pieces per wave");
  constexpr int MAIN = 2 * HALO + NSW * BST, EPI = BM * BN * 2;
  static_assert(MAIN <= 163840, "LDS");
  __shared__ __attribute__((aligned(1024))) char smem[MAIN > EPI ? MAIN : EPI];

  // the delayed-scaling site of this launch's activation operand: its dq (read below by every
  // block) was fixed by the quantize pass; block 0 moves that pass's amax into the history
  if (a.roll && blockIdx.x == 0 && threadIdx.x == 0) fp8_site_roll(a.roll);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wn = wave % WN, wm = wave / WN;
  const int nblk = gridDim.x, bid = blockIdx.x;
  const int q8 = nblk / 8, r8 = nblk % 8, xcd = bid % 8;
  const int lid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + bid / 8;
  const int tn = lid % a.ntn, tm = lid / a.ntn;
  const int tiles_w = a.W >> 6, tiles_h = a.H / TR;
  const int tw = tm % tiles_w, th = (tm / tiles_w) % tiles_h, n = tm / (tiles_w * tiles_h);
  const int co0 = tn * BN;
  const int p0 = (n * a.H + th * TR) * a.W + tw * 64;

  const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.x), 0, (int)x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.w), 0, 0x7fffffff, 0x00020000);
  const unsigned sbase = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(lds_ptr_t)smem);

  // halo pieces of this wave: piece q -> image q / HQ, 16 pixels (q % HQ) * 16 + lane / 4,
  // 16-B chunk lane % 4 (source chunk XOR h3swz)
  unsigned hoff[JH];
#pragma unroll
  for (int j = 0; j < JH; ++j) {
    const int q = wave + j * NW;
    const int img = q / HQ, hp = (q - img * HQ) * 16 + (lane >> 2), lchk = lane & 3;
    const int hr = hp / 66, hc = hp - (hp / 66) * 66;
    const int ih = th * TR + hr - 1, iw = tw * 64 + hc - 1;
    const bool ok = q < QH && hp < HP && ih >= 0 && ih < a.H && iw >= 0 && iw < a.W;
    hoff[j] = ok ? (unsigned)(((n * a.H + ih) * a.W + iw) * a.Cin + img * 64 + ((lchk ^ h3swz(hp)) << 4))
                 : 0x80000000u;
  }
  const int nh = (QH - wave + NW - 1) / NW;        // halo pieces this wave issues (JH or JH - 1)
  unsigned wbase[JB];
#pragma unroll
  for (int j = 0; j < JB; ++j) {
    const int row = (wave + j * NW) * 8 + (lane >> 3);
    wbase[j] = (unsigned)((co0 + row) * a.Kpad + (((lane & 7) ^ swz8(row)) << 4));
  }
  auto issue_b = [&](int ks) {
    const int c = ks / 9, t = ks - c * 9;
    const unsigned Bs = sbase + 2 * HALO + (ks % NSW) * BST;
    const unsigned k0 = (unsigned)(t * a.Cin + c * 128);
#pragma unroll
    for (int j = 0; j < JB; ++j) dma16s(wr, Bs + (wave + j * NW) * 1024, wbase[j], k0);
  };
  auto issue_halo = [&](int c) {
    const unsigned Hs = sbase + (c & 1) * HALO;
#pragma unroll
    for (int j = 0; j < JH; ++j)
      if (j < JH - 1 || wave + j * NW < QH) dma16s(xr, Hs + (wave + j * NW) * 1024, hoff[j], (unsigned)(c * 128));
  };

  const int lr = lane & 15, lh = lane >> 4;
  int hpb[RM];
#pragma unroll
  for (int m = 0; m < RM; ++m) {
    const int loc = wm * RM * 16 + m * 16 + lr;
    hpb[m] = (loc >> 6) * 66 + (loc & 63);
  }
  f32x4 acc[RN][RM];
#pragma unroll
  for (int i = 0; i < RN; ++i)
#pragma unroll
    for (int m = 0; m < RM; ++m) acc[i][m] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nch = a.Cin >> 7, nks = 9 * nch;
  const bool stag = (SCH & 2) && wave >= NW / 2;
  v8i fa[RN], fb[RM];
  auto mfma_all = [&]() {
    if constexpr (!(SCH & 1)) __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int i = 0; i < RN; ++i)
#pragma unroll
      for (int m = 0; m < RM; ++m) acc[i][m] = mma_f8(fa[i], fb[m], acc[i][m]);
    if constexpr (!(SCH & 1)) __builtin_amdgcn_s_setprio(0);
  };
  if constexpr (SCH & 1) {
    if (wave >= NW / 2) __builtin_amdgcn_s_setprio(1);
  }
  issue_b(0);
  issue_halo(0);
  if (NSW == 3 && 1 < nks) issue_b(1);
  for (int ks = 0; ks < nks; ++ks) {
    const int c = ks / 9, t = ks - c * 9;
    if constexpr (NSW == 3) {
      // stage ks (issued two steps ago) must land; stage ks + 1 (last step) may stay in flight,
      // and at t == 1 the halo of chunk c + 1 issued after it at step 9c too
      const int younger = (ks + 1 < nks ? JB : 0) + (t == 1 && c + 1 < nch ? nh : 0);
      wait_vm_dyn(younger);
    } else if (t == 1 && c + 1 < nch) {
      // step 9c+1 may leave the halo of chunk c+1 (issued last, at step 9c) in flight
      if (nh == JH) wait_vm<JH>();
      else wait_vm<(JH > 0 ? JH - 1 : 0)>();
    } else {
      wait_vm<0>();
    }
    wait_lgkm0();
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if constexpr ((SCH & 2) != 0) {
      if (stag && ks > 0) mfma_all();          // the previous tap's fragments
    }
    if (ks + NSW - 1 < nks) issue_b(ks + NSW - 1);
    if (t == 0 && c + 1 < nch) issue_halo(c + 1);
    const int r = t / 3, s3 = t - (t / 3) * 3;
    const char* Hs = smem + (c & 1) * HALO;
    const char* Bs = smem + 2 * HALO + (ks % NSW) * BST;
#pragma unroll
    for (int i = 0; i < RN; ++i) {
      const int row = wn * RN * 16 + i * 16 + lr;
      const uint4 u0 = *reinterpret_cast<const uint4*>(Bs + row * 128 + ((lh ^ swz8(row)) << 4));
      const uint4 u1 = *reinterpret_cast<const uint4*>(Bs + row * 128 + (((4 + lh) ^ swz8(row)) << 4));
      fa[i] = v8i{(int)u0.x, (int)u0.y, (int)u0.z, (int)u0.w, (int)u1.x, (int)u1.y, (int)u1.z, (int)u1.w};
    }
#pragma unroll
    for (int m = 0; m < RM; ++m) {
      const int hp = hpb[m] + r * 66 + s3;
      const int off = hp * 64 + ((lh ^ h3swz(hp)) << 4);
      const uint4 u0 = *reinterpret_cast<const uint4*>(Hs + off);
      const uint4 u1 = *reinterpret_cast<const uint4*>(Hs + HQ * 1024 + off);
      fb[m] = v8i{(int)u0.x, (int)u0.y, (int)u0.z, (int)u0.w, (int)u1.x, (int)u1.y, (int)u1.z, (int)u1.w};
    }
    if (!stag) mfma_all();
  }
  if (stag) mfma_all();
  if constexpr (SCH & 1) __builtin_amdgcn_s_setprio(0);
  const float dq = a.dq0[0] * a.dq1[0];
#pragma unroll
  for (int i = 0; i < RN; ++i)
#pragma unroll
    for (int m = 0; m < RM; ++m) acc[i][m] *= dq;
  __syncthreads();
  conv_epilogue<bf16, WN, WM, RN, RM, true>(a, acc, smem, co0, p0, tm, wn, wm, lane, tid);
}

// ----------------------------------------------------------------------------------------
// fp8 (e4m3) weight gradient of the 3x3 convs (BASELINE config C5): the
// sliding-row structure of conv3_halo_wgrad2 on v_mfma_scale_f32_16x16x128_f8f6f4, fed by the
// e4m3 copies of x and dy the forward / data gradient already consumed (delayed scaling, dq =
// site word 18).  A block owns 128 co x 9 taps x 64 ci and walks ROW PAIRS of one 64-column strip
// (the MFMA K = 128 pixels = output rows h and h+1):
//   D[co][(tap, ci)] += sum_{p in rows h, h+1} dy[p][co] * x[p + tap offset][ci]
// A = dy^T (rows co, k = pixel), B = x^T (rows ci, k = pixel): both transposed reads of NHWC byte
// images, ds_read_b64_tr_b8 (8 pixels x 16 channels per 16-lane group; tests/test_fp8_gpu.py
// pins the lane mapping).  A fragment (lane r = l & 15, g = l >> 4: k 16g..16g+15 U 64+16g..+15)
// = 4 such reads: pixels 16g + {0, 8} of row h, the same of row h + 1.  The 8-byte channel blocks
// of a pixel row are XOR-swizzled by the pixel (swz8d / swz8x) so the 32 lanes of a read
// (16 pixels x 2 blocks) hit 64 distinct banks; the swizzle is even, so a lane's 16-B DMA slot
// is one contiguous 16-B source chunk.  Group i = {dy rows h0+2i, h0+2i+1; x rows h0+2i+1,
// h0+2i+2} (26 pieces) travels AHEAD groups ahead; rings dy AHEAD+1 groups, x 2 AHEAD+4 rows.
// 4 waves, one per SIMD (512 registers each: the 128 x 576 tile is 288 accumulators per wave,
// which two waves per SIMD -- 256 registers each -- spill): wave (wc, wk) owns 64 co x 18 k-tiles.
// Output: the slab layout of conv3_halo_wgrad2 (fv_conv2d_wgrad_reduce), scaled by dq_x dq_dy;
// bias gradient = sum of the e4m3 dy (an all-ones B operand, ci tile 0; k-wave wk sums the co
// tiles 2 wk, 2 wk + 1 of its four).
// ----------------------------------------------------------------------------------------
struct Wg8Args {
  const uint8_t* x8;
  const uint8_t* dy8;
  const float* dqx;
  const float* dqdy;
  float* slab;
  float* bslab;
  int H, W, Cin, Cout, nseg, rows, nct, nci;
  int N, ipb;            // images, images per split (the block walks them in turn, one slab)
  unsigned xbytes, dybytes;
};

__device__ __forceinline__ int swz8x(int px) { return (((px >> 2) & 1) | (((px >> 4) & 1) << 1)) << 1; }   // 64-B rows
__device__ __forceinline__ int swz8d(int px) { return (((px >> 1) & 3) | (((px >> 4) & 1) << 2)) << 1; }   // 128-B rows
// 32-B rows (CIB = 32): a half-wave's tr_b8 pixels are two runs of 8, 16 apart, which alias mod
// 8 pixels (256 B): the block pair flips with pixel bit 4
__device__ __forceinline__ int swz8x32(int px) { return ((px >> 4) & 1) << 1; }
template <int CIB>
__device__ __forceinline__ int swz8xc(int px) {
  if constexpr (CIB == 64) return swz8x(px);
  else return swz8x32(px);
}

__device__ __forceinline__ v2i_t tr8(const char* p) {
  return __builtin_amdgcn_ds_read_tr8_b64_v2i32((FV_LDS v2i_t*)(FV_LDS char*)(p));
}

// CIB (r6): input channels per block.  64: a wave owns 64 co x 18 k-tiles =
// 288 accumulators, more than the 256 AGPRs, so the compiler rotates accumulator tiles through
// VGPRs (~860 v_accvgpr moves per 72 MFMAs).  32: the block is 128 co x 9 taps x 32 ci and a
// wave owns 64 co x 9 k-tiles = 144 accumulators (no rotation), at twice the blocks (dy rows
// read by twice as many ci tiles, through the XCD's L2) and 13 fragment reads per 9 MFMAs
// instead of 22 per 18.
template <int AHEAD, int CIB = 64>
__global__ void __launch_bounds__(256, 1)
conv3_wgrad_fp8(Wg8Args a) {
  constexpr int BC = 128, NSD = AHEAD + 1, NSX = 2 * AHEAD + 4;
  constexpr int DYR = 64 * BC, DYB = 2 * DYR;         // 8 KB per dy row, 16 KB per group
  constexpr int XQ = (66 * CIB + 1023) / 1024, XB = XQ * 1024;   // x row: 66 px x CIB B (5 / 3 pieces)
  constexpr int NPC = 16 + 2 * XQ;                    // pieces per group (26)
  __shared__ __attribute__((aligned(1024))) char smem[NSD * DYB + NSX * XB];
  char* const dyr = smem;
  char* const xr_ = smem + NSD * DYB;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wc = wave & 1, wk = wave >> 1;
  const int li = lane & 15, g = lane >> 4;
  const int strips = a.W >> 6;
  const int nblk = gridDim.x, bid = blockIdx.x;
  const int q8 = nblk / 8, r8 = nblk % 8, xcd = bid % 8;
  const int blk = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + bid / 8;
  const int ntile = a.nct * a.nci;
  const int tile = blk % ntile, tc = tile % a.nct, tci = tile / a.nct;
  const int split = blk / ntile;
  const int seg = split % a.nseg, strip = (split / a.nseg) % strips, ng = split / (a.nseg * strips);
  int n = ng * a.ipb;                                 // the image being walked (issue_* read it)
  const int co0 = tc * BC, w0 = strip * 64, ci0 = tci * CIB;
  const int h0 = seg * a.rows, h1 = min(a.H, h0 + a.rows);
  const int nstep = (h1 - h0) >> 1;                   // row pairs (the host keeps segments even)
  constexpr int NWV = 4, JP = (NPC + NWV - 1) / NWV;  // 4 waves; <= 7 pieces per wave and group
  const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(a.x8), 0, (int)a.xbytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t dr = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(a.dy8), 0, (int)a.dybytes, 0x00020000);
  const unsigned sbase = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(lds_ptr_t)smem);

  // this wave's pieces of a group: q = wave + 4 j < 26 (q < 16: dy row q >> 3, piece q & 7; else
  // x row (q - 16) / 5, piece (q - 16) % 5); source offsets relative to the row start
  const int npw = (NPC - wave + NWV - 1) / NWV;
  unsigned poff[JP];
#pragma unroll
  for (int j = 0; j < JP; ++j) {
    const int q = wave + NWV * j;
    poff[j] = 0x80000000u;
    if (q < 16) {
      const int o = (q & 7) * 1024 + lane * 16;
      const int px = o >> 7, kk = (o >> 4) & 7;
      poff[j] = (unsigned)(px * a.Cout + co0 + ((kk ^ (swz8d(px) >> 1)) << 4));
    } else if (q < NPC) {
      const int o = ((q - 16) % XQ) * 1024 + lane * 16;
      const int px = o / CIB, kk = (o >> 4) & (CIB / 16 - 1);
      const int iw = w0 - 1 + px;
      if (px < 66 && iw >= 0 && iw < a.W) poff[j] = (unsigned)(iw * a.Cin + ci0 + ((kk ^ (swz8xc<CIB>(px) >> 1)) << 4));
    }
  }
  auto xslot = [&](int y) { return (y - h0 + 1) % NSX; };
  auto issue_x = [&](int y, int j, int q) {             // x piece (q - 16) % 5 of row y
    // (the resource is rebuilt from the kernel argument here: called from inside the image
    // loop the captured one was treated as divergent and put in VGPRs)
    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(a.x8), 0, (int)a.xbytes, 0x00020000);
    const bool rok = y >= 0 && y < a.H;
    dma16s(xr, sbase + NSD * DYB + xslot(y) * XB + ((q - 16) % XQ) * 1024, rok ? poff[j] : 0x80000000u,
           rok ? (unsigned)(((n * a.H + y) * a.W) * a.Cin) : 0u);
  };
  auto issue_group = [&](int i) {
    const __amdgpu_buffer_rsrc_t dr = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(a.dy8), 0, (int)a.dybytes, 0x00020000);
    const int h = h0 + 2 * i;
#pragma unroll
    for (int j = 0; j < JP; ++j) {
      const int q = wave + NWV * j;
      if (j < npw) {
        if (q < 16) {
          const int r = q >> 3;
          dma16s(dr, sbase + (i % NSD) * DYB + r * DYR + (q & 7) * 1024, poff[j],
                 (unsigned)(((n * a.H + h + r) * a.W + w0) * a.Cout));
        } else {
          issue_x(h + 1 + (q - 16) / XQ, j, q);
        }
      }
    }
  };
  // prologue of one image: x rows h0 - 1 (as row 0 of a group) and h0 (as row 1), the first
  // AHEAD groups
  auto prologue = [&]() {
#pragma unroll
    for (int j = 0; j < JP; ++j) {
      const int q = wave + NWV * j;
      if (j < npw && q >= 16) issue_x(h0 - 1 + (q - 16) / XQ, j, q);
    }
#pragma unroll
    for (int i = 0; i < AHEAD; ++i)
      if (i < nstep) issue_group(i);
  };
  prologue();

  constexpr int KTT = CIB / 16;                         // 16-ci k-tiles per tap
  constexpr int NK = 9 * KTT / 2;                       // k-tiles NK WK .. NK WK + NK - 1 of a wave
  f32x4 acc[4][NK];
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int j = 0; j < NK; ++j) acc[q][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  // bias gradient: k-wave WK sums co tiles 2 WK, 2 WK + 1 of its four (an all-ones e4m3 B operand)
  f32x4 accb[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
  const bool do_bias = a.bslab && tci == 0;
  const int pl = 16 * g + (li >> 1);                    // this lane's pixel row of a tr_b8 block
  // r6: a split may hold ipb images (B = 64: half the fp32 slabs); each image restarts the
  // rings once every wave has passed the previous image's last step (all its DMAs waited)
  for (int im = 0; im < a.ipb; ++im) {
    if (im > 0) {
      if (ng * a.ipb + im >= a.N) break;
      n = ng * a.ipb + im;
      wait_lgkm0();
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      prologue();
    }
    with_const<0, 2>(wk, [&](auto wkc) {
      constexpr int WK = decltype(wkc)::value;
      for (int i = 0; i < nstep; ++i) {
        const int younger = min(AHEAD - 1, nstep - 1 - i);
        wait_vm_dyn(younger * npw);
        wait_lgkm0();
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (i + AHEAD < nstep) issue_group(i + AHEAD);
        const char* d0 = dyr + (i % NSD) * DYB;
        const char* d1 = d0 + DYR;
        // the fragment offsets are recomputed every step (an opaque copy of the pixel row)
        // instead of being hoisted out of the loop: 26 loop-invariant offsets would spill the
        // accumulators
        int plv = pl;
        asm volatile("" : "+v"(plv));
        v8i af[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int cb = 2 * (wc * 4 + q) + (li & 1);   // 8-byte co block of the 128-co tile
          const int o0 = plv * BC + ((cb ^ swz8d(plv)) << 3), o1 = (plv + 8) * BC + ((cb ^ swz8d(plv + 8)) << 3);
          const v2i_t r0 = tr8(d0 + o0), r1 = tr8(d0 + o1), r2 = tr8(d1 + o0), r3 = tr8(d1 + o1);
          af[q] = v8i{r0[0], r0[1], r1[0], r1[1], r2[0], r2[1], r3[0], r3[1]};
        }
        // x fragment of k-tile j: tap (r, s), 16-ci block u; rows h - 1 + r (k < 64) and h + r
        auto xfrag = [&](int j) {
          const int kt = NK * WK + j, tap = kt / KTT, u = kt % KTT, r = tap / 3, s3 = tap - (tap / 3) * 3;
          const char* xa = xr_ + ((2 * i + r) % NSX) * XB;
          const char* xb = xr_ + ((2 * i + 1 + r) % NSX) * XB;
          const int cb = 2 * u + (li & 1);
          const int p0 = plv + s3, p1 = plv + 8 + s3;
          const int o0 = p0 * CIB + ((cb ^ swz8xc<CIB>(p0)) << 3), o1 = p1 * CIB + ((cb ^ swz8xc<CIB>(p1)) << 3);
          const v2i_t r0 = tr8(xa + o0), r1 = tr8(xa + o1), r2 = tr8(xb + o0), r3 = tr8(xb + o1);
          return v8i{r0[0], r0[1], r1[0], r1[1], r2[0], r2[1], r3[0], r3[1]};
        };
        v8i bcur = xfrag(0);
#pragma unroll
        for (int j = 0; j < NK; ++j) {
          v8i bnext = bcur;
          if (j + 1 < NK) bnext = xfrag(j + 1);
#pragma unroll
          for (int q = 0; q < 4; ++q) acc[q][j] = mma_f8(af[q], bcur, acc[q][j]);
          bcur = bnext;
        }
        if (do_bias) {
          const v8i ones = {0x38383838, 0x38383838, 0x38383838, 0x38383838, 0x38383838, 0x38383838, 0x38383838, 0x38383838};
          accb[0] = mma_f8(af[2 * WK], ones, accb[0]);
          accb[1] = mma_f8(af[2 * WK + 1], ones, accb[1]);
        }
      }
    });
  }
  with_const<0, 2>(wk, [&](auto wkc) {
    constexpr int WK = decltype(wkc)::value;
    const float dq = a.dqx[0] * a.dqdy[0], dqb = a.dqdy[0];
    const long KW = 9L * a.Cin;
    float* sl = a.slab + (long)split * a.Cout * KW;
#pragma unroll
    for (int j = 0; j < NK; ++j) {
      const int kt = NK * WK + j, tap = kt / KTT;
      const int kcol = tap * a.Cin + ci0 + (kt % KTT) * 16 + li;
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) sl[(long)(co0 + wc * 64 + q * 16 + 4 * g + jj) * KW + kcol] = acc[q][j][jj] * dq;
    }
    if (do_bias && li == 0) {
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj)
          a.bslab[(long)split * a.Cout + co0 + wc * 64 + (2 * WK + t) * 16 + 4 * g + jj] = accb[t][jj] * dqb;
    }
  });
}

// fp8 conv eligibility: 3x3, stride 1, 'same', channel counts multiples of 128 (in and out),
// W % 64 == 0, H % 4 == 0, bf16 NHWC output, operands < 2 GB
bool fp8_ok(const fv_conv_desc* d) {
  return d->ksize == 3 && !d->upsample && !d->pro_act && !d->epi_sigmoid && !d->out_nchw_f32 && d->cin % 128 == 0 &&
         d->cin_valid == d->cin && d->cout % 128 == 0 && d->ldy == d->cout && d->w % 64 == 0 && d->h % 4 == 0 &&
         (long)d->n * d->h * d->w * d->cin < (1L << 31) && (long)d->n * d->h * d->w * d->cout * 2 < (1L << 31);
}

int conv_fp8_run(const fv_conv_desc* d, int cin, int cout, const uint8_t* x8, const float* dq_x, const uint8_t* w8,
                 const float* dq_w, const float* bias, const void* res, void* y, float* stats, hipStream_t s,
                 unsigned* roll = nullptr, float* sprec = nullptr) {
  ConvArgs a{};
  // store-pass mode 1 (r6): (sum, sum of squares) of the stored, residual-added output in the
  // staged epilogue's store loop -- the records of fv_conv2d_fwd_sr, same geometry (256-pixel
  // tiles, one record per wave and tile: the bf16 res tile's count), so in fp8 mode the next
  // ResBlock's bn1 statistics need no tensor_stats pass either
  a.spm = sprec ? 1 : 0;
  a.sprec = sprec;
  a.x = x8; a.w = w8; a.bias = bias; a.res = res; a.y = y; a.stats = stats;
  a.nrec = stats ? fv_conv2d_fp8_stats_blocks(d) : 0;
  a.dq0 = dq_x; a.dq1 = dq_w;
  a.roll = roll;
  a.N = d->n; a.H = d->h; a.W = d->w; a.Hin = d->h; a.Win = d->w;
  a.P = d->n * d->h * d->w;
  a.Cin = cin; a.lgCin = fv_ilog2(cin);
  a.Cout = cout; a.ldy = cout;
  a.K = 9 * cin; a.Kpad = 9 * cin;
  a.lgtw = 6;
  a.ntn = cout / 128;
  const int nblk = a.ntn * d->n * (d->h / 4) * (d->w / 64);
  const unsigned xb = (unsigned)((long)d->n * d->h * d->w * cin);
  // (measured and not kept, r4: a 3-deep weight ring issued 3 steps ahead with the next tap's
  // fragments read under this tap's MFMAs and the barrier after them, conv3_halo_fwd2's schedule:
  // res fwd / dgrad at B = 64 188 / 172 -> 208 / 192 us: the two waves of a SIMD already hide
  // each other's fragment reads (16 KB per 16 MFMAs of 32 cycles, half the CU's 256 B/clk of
  // LDS at the fp8 peak).)
  switch (res_sched(3)) {
    case 1: hipLaunchKernelGGL((conv3_halo_fp8<2, 4, 4, 4, 2, 1>), dim3(nblk), dim3(512), 0, s, a, xb); break;
    case 2: hipLaunchKernelGGL((conv3_halo_fp8<2, 4, 4, 4, 2, 2>), dim3(nblk), dim3(512), 0, s, a, xb); break;
    case 3: hipLaunchKernelGGL((conv3_halo_fp8<2, 4, 4, 4, 2, 3>), dim3(nblk), dim3(512), 0, s, a, xb); break;
    default: hipLaunchKernelGGL((conv3_halo_fp8<2, 4, 4, 4>), dim3(nblk), dim3(512), 0, s, a, xb); break;
  }
  return fv_check_launch("conv2d_fp8");
}

}  // namespace

extern "C" {

size_t fv_fp8_ws_bytes(void) { return FP8_NPART * sizeof(float); }

int fv_quantize_fp8(int dtype_in, const void* x, long count, uint8_t* y, float* dq, void* ws, void* stream) {
  FV_REQUIRE(x && y && dq && ws && count > 0, "quantize_fp8: bad args");
  FV_REQUIRE(dtype_in == FV_BF16 || dtype_in == FV_F32, "quantize_fp8: input must be bf16 or f32");
  hipStream_t s = (hipStream_t)stream;
  const long chunks = (count + 7) / 8;
  const int nb = (int)std::min<long>(FP8_NPART, std::max<long>(1, (chunks + 255) / 256));
  if (dtype_in == FV_BF16) {
    hipLaunchKernelGGL(amax_kernel<bf16>, dim3(nb), dim3(256), 0, s, (const bf16*)x, count, (float*)ws);
    hipLaunchKernelGGL(quantize_fp8_kernel<bf16>, dim3(nb), dim3(256), 0, s, (const bf16*)x, count, (const float*)ws,
                       nb, y, dq);
  } else {
    hipLaunchKernelGGL(amax_kernel<float>, dim3(nb), dim3(256), 0, s, (const float*)x, count, (float*)ws);
    hipLaunchKernelGGL(quantize_fp8_kernel<float>, dim3(nb), dim3(256), 0, s, (const float*)x, count,
                       (const float*)ws, nb, y, dq);
  }
  return fv_check_launch("quantize_fp8");
}

size_t fv_fp8_site_bytes(void) { return FP8_SITE * sizeof(unsigned); }

int fv_fp8_set_deferred_roll(int on) {
  g_fp8_defer_roll = on ? 1 : 0;
  return FV_OK;
}

int fv_fp8_amax(int dtype_in, const void* x, long count, float* amax, void* ws, void* stream) {
  FV_REQUIRE(x && amax && ws && count > 0, "fp8_amax: bad args");
  FV_REQUIRE(dtype_in == FV_BF16 || dtype_in == FV_F32, "fp8_amax: input must be bf16 or f32");
  hipStream_t s = (hipStream_t)stream;
  const long chunks = (count + 7) / 8;
  const int nb = (int)std::min<long>(FP8_NPART, std::max<long>(1, (chunks + 255) / 256));
  if (dtype_in == FV_BF16)
    hipLaunchKernelGGL(amax_kernel<bf16>, dim3(nb), dim3(256), 0, s, (const bf16*)x, count, (float*)ws);
  else
    hipLaunchKernelGGL(amax_kernel<float>, dim3(nb), dim3(256), 0, s, (const float*)x, count, (float*)ws);
  hipLaunchKernelGGL(fp8_amax_final_kernel, dim3(1), dim3(256), 0, s, (const float*)ws, nb, amax);
  return fv_check_launch("fp8_amax");
}

int fv_fp8_site_seed(void* site, const float* amax, void* stream) {
  FV_REQUIRE(site && amax, "fp8_site_seed: bad args");
  hipLaunchKernelGGL(fp8_site_seed_from_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, amax, (unsigned*)site);
  return fv_check_launch("fp8_site_seed_from");
}

int fv_fp8_sites_inflight(int n, const uint64_t* sites, float* amax, void* stream) {
  FV_REQUIRE(n >= 0 && (n == 0 || (sites && amax)), "fp8_sites_inflight: bad args");
  if (n == 0) return FV_OK;
  hipLaunchKernelGGL(fp8_sites_inflight_kernel, dim3(fv_cdiv(n, 64)), dim3(64), 0, (hipStream_t)stream, n,
                     (const unsigned long long*)sites, amax);
  return fv_check_launch("fp8_sites_inflight");
}

int fv_fp8_sites_roll(int n, const uint64_t* sites, const float* amax, void* stream) {
  FV_REQUIRE(n >= 0 && (n == 0 || (sites && amax)), "fp8_sites_roll: bad args");
  if (n == 0) return FV_OK;
  hipLaunchKernelGGL(fp8_sites_roll_kernel, dim3(fv_cdiv(n, 64)), dim3(64), 0, (hipStream_t)stream, n,
                     (const unsigned long long*)sites, amax);
  return fv_check_launch("fp8_sites_roll");
}

int fv_quantize_fp8_site(int dtype_in, const void* x, long count, uint8_t* y, void* site, int seeded, void* ws,
                         void* stream) {
  FV_REQUIRE(x && y && site && ws && count > 0, "quantize_fp8_site: bad args");
  FV_REQUIRE(dtype_in == FV_BF16 || dtype_in == FV_F32, "quantize_fp8_site: input must be bf16 or f32");
  hipStream_t s = (hipStream_t)stream;
  unsigned* st = (unsigned*)site;
  const long chunks = (count + 7) / 8;
  const int nb = (int)std::min<long>(FP8_NPART, std::max<long>(1, (chunks + 255) / 256));
  if (!seeded) {
    // exact first call: amax pass, quantize pass (dq into the site), history filled
    int rc = fv_quantize_fp8(dtype_in, x, count, y, (float*)(st + 18), ws, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(fp8_site_seed_kernel, dim3(1), dim3(256), 0, s, (const float*)ws, nb, st);
    return fv_check_launch("fp8_site_seed");
  }
  if (dtype_in == FV_BF16)
    hipLaunchKernelGGL(quantize_fp8_delayed_kernel<bf16>, dim3(nb), dim3(256), 0, s, (const bf16*)x, count, st, y);
  else
    hipLaunchKernelGGL(quantize_fp8_delayed_kernel<float>, dim3(nb), dim3(256), 0, s, (const float*)x, count, st, y);
  return fv_check_launch("quantize_fp8_delayed");
}

int fv_conv2d_fp8_supported(const fv_conv_desc* d) {
  if (check_desc(d) != FV_OK) return 0;
  return fp8_ok(d) ? 1 : 0;
}

size_t fv_conv_fp8_wk_bytes(const fv_conv_desc* d) {
  if (check_desc(d) != FV_OK || !fp8_ok(d)) return 0;
  return (size_t)d->cout * 9 * d->cin;
}

size_t fv_conv_fp8_wt_bytes(const fv_conv_desc* d) {
  if (check_desc(d) != FV_OK || !fp8_ok(d)) return 0;
  return (size_t)d->cin * 9 * d->cout;
}

int fv_conv_weight_prep_fp8(const fv_conv_desc* d, const float* w_param, const float* sigma, uint8_t* wk,
                            uint8_t* wt, float* dq, void* ws, void* stream) {
  int st = check_desc(d);
  if (st) return st;
  FV_REQUIRE(fp8_ok(d), "fp8 conv: unsupported descriptor (k=%d cin=%d cout=%d %dx%d)", d->ksize, d->cin, d->cout,
             d->h, d->w);
  FV_REQUIRE(w_param && (wk || wt) && dq && ws, "null pointer");
  hipStream_t s = (hipStream_t)stream;
  const long nw = (long)d->cout * d->cin * 9;
  const int nb = (int)std::min<long>(FP8_NPART, std::max<long>(1, (nw / 8 + 255) / 256));
  hipLaunchKernelGGL(amax_kernel<float>, dim3(nb), dim3(256), 0, s, w_param, nw, (float*)ws);
  const long tot = (wk ? nw : 0) + (wt ? nw : 0);
  const int nb2 = (int)std::min<long>(2048, fv_cdiv(tot, 256));
  hipLaunchKernelGGL(weight_prep_fp8_kernel, dim3(nb2), dim3(256), 0, s, w_param, sigma, (const float*)ws, nb, wk,
                     d->cout, wt, d->cin, d->cout, d->cin, dq);
  return fv_check_launch("weight_prep_fp8");
}

int fv_conv_weight_prep_fp8_multi(int n, const fv_conv_desc* descs, const float* const* w_params,
                                  const float* const* sigmas, uint8_t* const* wks, uint8_t* const* wts,
                                  float* const* dqs, void* ws, void* stream) {
  FV_REQUIRE(n >= 1 && n <= FV_WPREP_MAX && descs && w_params && sigmas && wks && wts && dqs && ws,
             "weight_prep_fp8_multi: bad args");
  W8Multi m{};
  m.n = n;
  m.stride = FP8_NPART;
  int nb_max = 1, nb2_max = 1;
  for (int i = 0; i < n; ++i) {
    const fv_conv_desc* d = &descs[i];
    int st = check_desc(d);
    if (st) return st;
    FV_REQUIRE(fp8_ok(d), "weight_prep_fp8_multi: conv %d: unsupported descriptor", i);
    FV_REQUIRE(w_params[i] && (wks[i] || wts[i]) && dqs[i], "weight_prep_fp8_multi: null pointer (conv %d)", i);
    W8Job& j = m.j[i];
    j.w = w_params[i], j.sigma = sigmas[i], j.wk = wks[i], j.wt = wts[i], j.dq = dqs[i];
    j.nw = (long)d->cout * d->cin * 9;
    j.cout = d->cout, j.cin = d->cin;
    // the per-conv entry's grids (fv_conv_weight_prep_fp8): the same partials, the same bits
    j.nb = (int)std::min<long>(FP8_NPART, std::max<long>(1, (j.nw / 8 + 255) / 256));
    j.nb2 = (int)std::min<long>(2048, fv_cdiv((wks[i] ? j.nw : 0) + (wts[i] ? j.nw : 0), 256));
    nb_max = std::max(nb_max, j.nb);
    nb2_max = std::max(nb2_max, j.nb2);
  }
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(amax_multi_kernel, dim3(nb_max, n), dim3(256), 0, s, m, (float*)ws);
  hipLaunchKernelGGL(weight_prep_fp8_multi_kernel, dim3(nb2_max, n), dim3(256), 0, s, m, (const float*)ws);
  return fv_check_launch("weight_prep_fp8_multi");
}

int fv_conv2d_fwd_fp8(const fv_conv_desc* d, const uint8_t* x8, const float* x_dq, const uint8_t* wk,
                      const float* w_dq, const float* bias, const void* res, void* y, float* stats, void* stream) {
  int st = check_desc(d);
  if (st) return st;
  FV_REQUIRE(fp8_ok(d), "fp8 conv: unsupported descriptor");
  FV_REQUIRE(x8 && x_dq && wk && w_dq && y, "null pointer");
  FV_REQUIRE(!(res && stats), "fp8 conv: residual and BN statistics in one call are not supported");
  return conv_fp8_run(d, d->cin, d->cout, x8, x_dq, wk, w_dq, bias, res, y, stats, (hipStream_t)stream);
}

int fv_conv2d_fwd_fp8_site(const fv_conv_desc* d, const uint8_t* x8, void* site, const uint8_t* wk, const float* w_dq,
                           const float* bias, const void* res, void* y, float* stats, void* stream) {
  int st = check_desc(d);
  if (st) return st;
  FV_REQUIRE(fp8_ok(d), "fp8 conv: unsupported descriptor");
  FV_REQUIRE(x8 && site && wk && w_dq && y, "null pointer");
  FV_REQUIRE(!(res && stats), "fp8 conv: residual and BN statistics in one call are not supported");
  unsigned* sp = (unsigned*)site;
  return conv_fp8_run(d, d->cin, d->cout, x8, (const float*)(sp + 18), wk, w_dq, bias, res, y, stats,
                      (hipStream_t)stream, g_fp8_defer_roll ? nullptr : sp);
}

int fv_conv2d_fwd_fp8_site_sr(const fv_conv_desc* d, const uint8_t* x8, void* site, const uint8_t* wk,
                              const float* w_dq, const float* bias, const void* res, void* y, const fv_store_reduce* sr,
                              void* stream) {
  int st = check_desc(d);
  if (st) return st;
  FV_REQUIRE(fp8_ok(d), "fp8 conv: unsupported descriptor");
  FV_REQUIRE(x8 && site && wk && w_dq && y && sr && sr->mode == 1 && sr->records, "fwd_fp8_sr: null pointer or mode != 1");
  // the fp8 tile (128 co x 256 px, 8 waves) writes the records of the bf16 res tile (256 px,
  // 8 waves): the geometry query must describe exactly that
  int bp = 0;
  FV_REQUIRE(sr_geometry(d, &bp) == (int)((long)d->n * d->h * d->w / 256 * 8) && bp == 32,
             "fwd_fp8_sr: store-pass records unavailable for this shape");
  unsigned* sp = (unsigned*)site;
  return conv_fp8_run(d, d->cin, d->cout, x8, (const float*)(sp + 18), wk, w_dq, bias, res, y, nullptr,
                      (hipStream_t)stream, g_fp8_defer_roll ? nullptr : sp, sr->records);
}

int fv_conv2d_bwd_data_fp8_site(const fv_conv_desc* d, const uint8_t* dy8, void* site, const uint8_t* wt,
                                const float* wt_dq, void* dx, void* stream) {
  int st = check_desc(d);
  if (st) return st;
  FV_REQUIRE(fp8_ok(d), "fp8 conv: unsupported descriptor");
  FV_REQUIRE(dy8 && site && wt && wt_dq && dx, "null pointer");
  unsigned* sp = (unsigned*)site;
  return conv_fp8_run(d, d->cout, d->cin, dy8, (const float*)(sp + 18), wt, wt_dq, nullptr, nullptr, dx, nullptr,
                      (hipStream_t)stream, g_fp8_defer_roll ? nullptr : sp);
}

int fv_conv2d_bwd_data_fp8(const fv_conv_desc* d, const uint8_t* dy8, const float* dy_dq, const uint8_t* wt,
                           const float* wt_dq, void* dx, void* stream) {
  int st = check_desc(d);
  if (st) return st;
  FV_REQUIRE(fp8_ok(d), "fp8 conv: unsupported descriptor");
  FV_REQUIRE(dy8 && dy_dq && wt && wt_dq && dx, "null pointer");
  return conv_fp8_run(d, d->cout, d->cin, dy8, dy_dq, wt, wt_dq, nullptr, nullptr, dx, nullptr, (hipStream_t)stream);
}

// images per split of the fp8 weight gradient: about 512 blocks of (128 co x 32 ci) tiles x
// splits (B = 32 res: 1 image; B = 64: 2, half the slabs of the bf16 plan's one image per
// split); a divisor of N.  The slabs of fv_conv2d_bwd_weight_fp8
// are then fp8_wg_nsplit(d) (<= the bf16 plan's, so fv_conv2d_wgrad_slab_elems still sizes
// them) and fv_conv2d_wgrad_fp8_reduce sums exactly those.
static int fp8_wg_ipb(const fv_conv_desc* d) {
  const WgPlan t = plan_wgrad(d);
  const long blocks = (long)t.ntc * (d->cin / 32) * t.nsplit;
  int ipb = (int)(blocks / 512);
  if (ipb < 1) ipb = 1;
  if (ipb > d->n) ipb = d->n;
  while (d->n % ipb) --ipb;
  return ipb;
}
static int fp8_wg_nsplit(const fv_conv_desc* d) {
  const WgPlan t = plan_wgrad(d);
  return t.nsteps * (d->w / 64) * (d->n / fp8_wg_ipb(d));
}

int fv_conv2d_wgrad_fp8_supported(const fv_conv_desc* d) {
  if (check_desc(d) != FV_OK || !fp8_ok(d) || d->cin % 64 || d->cout % 128) return 0;
  const WgPlan t = plan_wgrad(d);
  return t.v2 == WG_H3S && t.ntk == d->cin / 64 && t.sps % 2 == 0 && d->h % t.sps == 0 ? 1 : 0;
}

// the reduce of fv_conv2d_bwd_weight_fp8's slabs: wgrad_reduce_kernel over fp8_wg_nsplit(d) splits
int fv_conv2d_wgrad_fp8_reduce(const fv_conv_desc* d, const float* slab, const float* bias_slab, float* dw_param,
                               float* db, void* stream) {
  int st = check_desc(d);
  if (st) return st;
  FV_REQUIRE(fv_conv2d_wgrad_fp8_supported(d), "fp8 weight gradient reduce: unsupported descriptor");
  FV_REQUIRE(slab && dw_param, "null pointer");
  FV_REQUIRE(!db || bias_slab, "db needs the bias slab");
  const WgPlan t = plan_wgrad(d);
  const int K = d->ksize * d->ksize * d->cin;
  const long tot = (long)d->cout * K;
  const int nb_main = fv_cdiv(tot, 64);
  const int nb_bias = db ? fv_cdiv(d->cout, 64) : 0;
  launch_wgrad_reduce(slab, bias_slab, dw_param, db, fp8_wg_nsplit(d), t.CW, t.KW, K, d->cout, d->cin_valid,
                      fv_ilog2(d->cin), d->ksize, nb_main, nb_bias, d->ksize, (hipStream_t)stream);
  return fv_check_launch("wgrad_reduce_fp8");
}

int fv_conv2d_bwd_weight_fp8(const fv_conv_desc* d, const uint8_t* x8, const float* x_dq, const uint8_t* dy8,
                             const float* dy_dq, float* slab, float* bias_slab, void* stream) {
  int st = check_desc(d);
  if (st) return st;
  FV_REQUIRE(fv_conv2d_wgrad_fp8_supported(d), "fp8 weight gradient: unsupported descriptor");
  FV_REQUIRE(x8 && x_dq && dy8 && dy_dq && slab, "null pointer");
  const WgPlan t = plan_wgrad(d);
  const long P = (long)d->n * d->h * d->w;
  Wg8Args a{};
  a.x8 = x8; a.dy8 = dy8; a.dqx = x_dq; a.dqdy = dy_dq; a.slab = slab; a.bslab = bias_slab;
  a.H = d->h; a.W = d->w; a.Cin = d->cin; a.Cout = d->cout;
  a.nseg = t.nsteps; a.rows = t.sps; a.nct = t.ntc;
  a.xbytes = (unsigned)(P * d->cin);
  a.dybytes = (unsigned)(P * d->cout);
  a.N = d->n;
  a.ipb = fp8_wg_ipb(d);
  const int nsplit = fp8_wg_nsplit(d);
  // 32-channel input tiles (144 accumulators per wave), 2 row-pair groups in flight (r6: res fp8
  // wgrad 198.8 -> 191.8 us against 3, step -0.05 ms)
  a.nci = d->cin / 32;
  hipLaunchKernelGGL((conv3_wgrad_fp8<2, 32>), dim3(t.ntc * a.nci * nsplit), dim3(256), 0, (hipStream_t)stream, a);
  return fv_check_launch("conv2d_bwd_weight_fp8");
}

// BN-statistics records of fv_conv2d_fwd_fp8: one per wave row of the 128 co x 256 px tile
// (WM = 4 rows of 64 pixels)
int fv_conv2d_fp8_stats_block_pixels(const fv_conv_desc* d) {
  if (check_desc(d) != FV_OK || !fp8_ok(d)) return 0;
  return 64;
}

int fv_conv2d_fp8_stats_blocks(const fv_conv_desc* d) {
  if (check_desc(d) != FV_OK || !fp8_ok(d)) return 0;
  return fv_cdiv((long)d->n * d->h * d->w, 64);
}

int fv_tr8_probe(const int* lane_addr, int* out, void* stream) {
  FV_REQUIRE(lane_addr && out, "tr8_probe: null pointer");
  hipLaunchKernelGGL(tr8_probe_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, lane_addr, out);
  return fv_check_launch("tr8_probe");
}

int fv_fp8_mfma_probe(const uint8_t* a, const uint8_t* b, float* c, void* stream) {
  FV_REQUIRE(a && b && c, "null pointer");
  hipLaunchKernelGGL(fp8_mfma_probe_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, a, b, c);
  return fv_check_launch("fp8_mfma_probe");
}

}  // extern "C"
