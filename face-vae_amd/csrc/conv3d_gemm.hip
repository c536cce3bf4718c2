// General-channel 3-D convolution as an implicit GEMM on the matrix units (fv_conv3dg_*): the
// MFE's hourglass convs, its 1x1x1 compress and its 7x7x7 mask conv (models.py:1052-1075 of
// Luh1124/face-vae; DownBlock3D / UpBlock3D modules.py:73-94).  Stride 1, padding ksize / 2,
// ksize 1 / 3 / 7, NDHWC activations, cin a multiple of 8, any cout, any d / h / w.
//
// Forward (conv3dg_fwd_kernel) follows conv_fwd_kernel of conv_fwd.hip: register-staged gather,
// double-buffered swizzled LDS, the Frag / mma helpers of conv_common.h (bf16:
// v_mfma_f32_16x16x32_bf16; fp32 parity mode: v_mfma_f32_16x16x4_f32).  The K loop walks
// (tap outer, 8-channel chunk inner), so the channel count need not be a power of two; UPS reads
// the input of a nearest (1, 2, 2) upsample at (d, h >> 1, w >> 1).  The data gradient is the
// same kernel on transposed, tap-flipped weights (its "input" dy may then have any channel count:
// the gather falls back to element loads when that count is no multiple of 8).
//
// Weight gradient (conv3dg_wgrad_kernel): GEMM over the voxels, one tap per block, the voxel
// range split into fp32 slabs that conv3dg_wgrad_reduce_kernel sums in split order -- no float
// atomics, so dW and db are bit-reproducible.
#include "conv_common.h"

namespace {

struct G3Args {
  const void* x;
  const void* w;
  const float* bias;
  void* y;
  int N, D, H, W;   // output volume
  int Hin, Win;     // input rows / columns (H / 2, W / 2 under UPS)
  int P;            // N * D * H * W
  int Cin;          // channels of x (its channel stride)
  int nch;          // 8-channel chunks per tap: cdiv(Cin, 8)
  int vec;          // Cin % 8 == 0: 8-channel vector gathers
  int Cout;
  int Kpad, nks, ntn;
  FastDiv fnch;
};

template <typename T, int KS, int WN, int WM, int RN, int RM, bool UPS>
__global__ void __launch_bounds__(64 * WN * WM)
conv3dg_fwd_kernel(G3Args a) {
  constexpr int NT = 64 * WN * WM;
  constexpr int BN = WN * RN * 16;   // output channels per block
  constexpr int BM = WM * RM * 16;   // voxels per block
  constexpr int PAD = KS / 2;
  constexpr int TAPS = KS * KS * KS;
  constexpr int ES = sizeof(T);
  constexpr int ROWB = BK * ES;
  constexpr int CA = BM * 4 / NT;
  constexpr int NBCH = BN * 4;
  constexpr int CB = (NBCH + NT - 1) / NT;
  static_assert((BM * 4) % NT == 0, "A staging");
  __shared__ __attribute__((aligned(16))) char smem[2 * (BM + BN) * ROWB];

  const T* __restrict__ x = reinterpret_cast<const T*>(a.x);
  const T* __restrict__ wk = reinterpret_cast<const T*>(a.w);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wn = wave % WN, wm = wave / WN;
  const int tn = blockIdx.x % a.ntn, tm = blockIdx.x / a.ntn;
  const int co0 = tn * BN, p0 = tm * BM;
  const int kc = tid & 3;

  int rd[CA], rh[CA], rw[CA], rn[CA];
  bool rv[CA];
#pragma unroll
  for (int i = 0; i < CA; ++i) {
    const int pix = p0 + (tid >> 2) + i * (NT / 4);
    rv[i] = pix < a.P;
    int t = pix / a.W;
    rw[i] = pix - t * a.W;
    int u = t / a.H;
    rh[i] = t - u * a.H;
    rn[i] = u / a.D;
    rd[i] = u - rn[i] * a.D;
  }

  Chunk8<T> ra[CA], rbw[CB];

  auto gload = [&](int ks) {
    const unsigned q = (unsigned)ks * 4 + kc;
    const unsigned tap = fdiv(q, a.fnch);
    const int ci = (int)(q - tap * a.nch) * 8;
    const bool kin = tap < (unsigned)TAPS;
    const int td = (int)tap / (KS * KS), tr = (int)tap - td * KS * KS;
    const int th = tr / KS, tw = tr - th * KS;
#pragma unroll
    for (int i = 0; i < CA; ++i) {
      const int dd = rd[i] + td - PAD, hh = rh[i] + th - PAD, ww = rw[i] + tw - PAD;
      const bool ok = kin && rv[i] && dd >= 0 && dd < a.D && hh >= 0 && hh < a.H && ww >= 0 && ww < a.W;
      const int hs = UPS ? hh >> 1 : hh, ws = UPS ? ww >> 1 : ww;
      if (ok) {
        const T* p = x + ((((long)rn[i] * a.D + dd) * a.Hin + hs) * a.Win + ws) * a.Cin + ci;
        if (a.vec) {
          ra[i].load(p);
        } else {
          float f[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) f[j] = ci + j < a.Cin ? Elt<T>::to_f(p[j]) : 0.f;
          ra[i].set8(f);
        }
      } else {
        ra[i].zero();
      }
    }
#pragma unroll
    for (int j = 0; j < CB; ++j) {
      const int qq = tid + j * NT;
      if (qq < NBCH) rbw[j].load(wk + (long)(co0 + (qq >> 2)) * a.Kpad + ks * BK + kc * 8);
    }
  };

  auto lstore = [&](int buf) {
    char* As = smem + buf * (BM + BN) * ROWB;
    char* Bs = As + BM * ROWB;
#pragma unroll
    for (int i = 0; i < CA; ++i) {
      const int row = (tid >> 2) + i * (NT / 4);
      ra[i].store(reinterpret_cast<T*>(As + row * ROWB + ((kc ^ rswz<T>(row)) * 8 * ES)));
    }
#pragma unroll
    for (int j = 0; j < CB; ++j) {
      const int qq = tid + j * NT;
      if (qq < NBCH) {
        const int row = qq >> 2;
        rbw[j].store(reinterpret_cast<T*>(Bs + row * ROWB + ((kc ^ rswz<T>(row)) * 8 * ES)));
      }
    }
  };

  f32x4 acc[RN][RM];
#pragma unroll
  for (int n = 0; n < RN; ++n)
#pragma unroll
    for (int m = 0; m < RM; ++m) acc[n][m] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int lr = lane & 15, lh = lane >> 4;
  auto compute = [&](int buf) {
    const char* As = smem + buf * (BM + BN) * ROWB;
    const char* Bs = As + BM * ROWB;
    Frag<T> af[RN], bfm[RM];
#pragma unroll
    for (int n = 0; n < RN; ++n) {
      const int row = wn * RN * 16 + n * 16 + lr;
      af[n].lds(Bs + row * ROWB + ((lh ^ rswz<T>(row)) * 8 * ES));
    }
#pragma unroll
    for (int m = 0; m < RM; ++m) {
      const int row = wm * RM * 16 + m * 16 + lr;
      bfm[m].lds(As + row * ROWB + ((lh ^ rswz<T>(row)) * 8 * ES));
    }
#pragma unroll
    for (int n = 0; n < RN; ++n)
#pragma unroll
      for (int m = 0; m < RM; ++m) acc[n][m] = mma(af[n], bfm[m], acc[n][m]);
  };

  gload(0);
  lstore(0);
  __syncthreads();
  for (int ks = 0; ks < a.nks; ++ks) {
    const int cur = ks & 1;
    if (ks + 1 < a.nks) gload(ks + 1);
    compute(cur);
    if (ks + 1 < a.nks) lstore(cur ^ 1);
    __syncthreads();
  }

  // epilogue: bias, then store (accumulator element i of tile (n, m): channel lh * 4 + i, voxel lr)
  T* __restrict__ y = reinterpret_cast<T*>(a.y);
  const bool v4 = (a.Cout & 3) == 0;
#pragma unroll
  for (int n = 0; n < RN; ++n) {
    const int cb = co0 + wn * RN * 16 + n * 16 + lh * 4;
    float bv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) bv[i] = (a.bias && cb + i < a.Cout) ? a.bias[cb + i] : 0.f;
#pragma unroll
    for (int m = 0; m < RM; ++m) {
      const int pix = p0 + wm * RM * 16 + m * 16 + lr;
      if (pix >= a.P || cb >= a.Cout) continue;
      float f[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) f[i] = acc[n][m][i] + bv[i];
      T* yp = y + (long)pix * a.Cout + cb;
      if (v4) {
        store4<T>(yp, f);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (cb + i < a.Cout) yp[i] = Elt<T>::from_f(f[i]);
      }
    }
  }
}

// ---- weight gradient ----
struct G3WArgs {
  const void* x;
  const void* dy;
  float* slab;      // [nsplit][Cout][taps][Cin]
  int N, D, H, W, Hin, Win, P;
  int Cin, Cout, ks, ups, taps;
  int nci, nco, nsplit, vper;   // vper: voxels per split, a multiple of BK
  int dyvec;                    // Cout % 8 == 0
  FastDiv fW, fH, fD;
};

// one block: TCO output channels x TCI input channels of one tap over one voxel split.  k of the
// MFMA = voxels, so both operands are transposed on their way into LDS (rows = channels).
template <typename T, int WCO, int WCI, int RCO, int RCI>
__global__ void __launch_bounds__(64 * WCO * WCI)
conv3dg_wgrad_kernel(G3WArgs a) {
  constexpr int NT = 64 * WCO * WCI;
  constexpr int TCO = WCO * RCO * 16, TCI = WCI * RCI * 16;
  constexpr int ES = sizeof(T);
  constexpr int ROWB = BK * ES;
  constexpr int DC8 = TCO / 8, XC8 = TCI / 8;
  constexpr int NDY = DC8 * BK, NX = XC8 * BK;
  constexpr int CD = (NDY + NT - 1) / NT, CX = (NX + NT - 1) / NT;
  __shared__ __attribute__((aligned(16))) char smem[2 * (TCO + TCI) * ROWB];

  const T* __restrict__ x = reinterpret_cast<const T*>(a.x);
  const T* __restrict__ dy = reinterpret_cast<const T*>(a.dy);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wci = wave % WCI, wco = wave / WCI;
  int b = blockIdx.x;
  const int tco = b % a.nco;
  b /= a.nco;
  const int tci = b % a.nci;
  b /= a.nci;
  const int tap = b % a.taps, split = b / a.taps;
  const int co0 = tco * TCO, ci0 = tci * TCI;
  const int pad = a.ks / 2;
  const int td = tap / (a.ks * a.ks), tr = tap - td * a.ks * a.ks;
  const int od = td - pad, oh = tr / a.ks - pad, ow = tr % a.ks - pad;
  const long v0 = (long)split * a.vper;
  const long v1 = v0 + a.vper < (long)a.P ? v0 + a.vper : (long)a.P;
  const int nsteps = v1 > v0 ? (int)((v1 - v0 + BK - 1) / BK) : 0;

  Chunk8<T> rdy[CD], rx[CX];

  auto gload = [&](int step) {
    const long vb = v0 + (long)step * BK;
#pragma unroll
    for (int i = 0; i < CD; ++i) {
      const int q = tid + i * NT;
      if (q >= NDY) break;
      const int c8 = q % DC8, kv = q / DC8;
      const long v = vb + kv;
      const int co = co0 + c8 * 8;
      rdy[i].zero();
      if (v < v1 && co < a.Cout) {
        const T* p = dy + v * a.Cout + co;
        if (a.dyvec) {
          rdy[i].load(p);
        } else {
          float f[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) f[j] = co + j < a.Cout ? Elt<T>::to_f(p[j]) : 0.f;
          rdy[i].set8(f);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < CX; ++i) {
      const int q = tid + i * NT;
      if (q >= NX) break;
      const int c8 = q % XC8, kv = q / XC8;
      const long v = vb + kv;
      const int ci = ci0 + c8 * 8;
      rx[i].zero();
      if (v < v1 && ci < a.Cin) {
        const unsigned uv = (unsigned)v;
        const unsigned t = fdiv(uv, a.fW);
        const int w = (int)(uv - t * a.W);
        const unsigned u = fdiv(t, a.fH);
        const int h = (int)(t - u * a.H);
        const unsigned n = fdiv(u, a.fD);
        const int d = (int)(u - n * a.D);
        const int dd = d + od, hh = h + oh, ww = w + ow;
        if (dd >= 0 && dd < a.D && hh >= 0 && hh < a.H && ww >= 0 && ww < a.W) {
          const int hs = a.ups ? hh >> 1 : hh, ws = a.ups ? ww >> 1 : ww;
          rx[i].load(x + ((((long)n * a.D + dd) * a.Hin + hs) * a.Win + ws) * a.Cin + ci);
        }
      }
    }
  };

  auto lstore = [&](int buf) {
    char* Ds = smem + buf * (TCO + TCI) * ROWB;
    char* Xs = Ds + TCO * ROWB;
#pragma unroll
    for (int i = 0; i < CD; ++i) {
      const int q = tid + i * NT;
      if (q >= NDY) break;
      const int c8 = q % DC8, kv = q / DC8;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int row = c8 * 8 + j;
        *reinterpret_cast<T*>(Ds + row * ROWB + ((((kv >> 3) ^ rswz<T>(row)) * 8 + (kv & 7)) * ES)) =
            Elt<T>::from_f(rdy[i].get(j));
      }
    }
#pragma unroll
    for (int i = 0; i < CX; ++i) {
      const int q = tid + i * NT;
      if (q >= NX) break;
      const int c8 = q % XC8, kv = q / XC8;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int row = c8 * 8 + j;
        *reinterpret_cast<T*>(Xs + row * ROWB + ((((kv >> 3) ^ rswz<T>(row)) * 8 + (kv & 7)) * ES)) =
            Elt<T>::from_f(rx[i].get(j));
      }
    }
  };

  f32x4 acc[RCI][RCO];
#pragma unroll
  for (int n = 0; n < RCI; ++n)
#pragma unroll
    for (int m = 0; m < RCO; ++m) acc[n][m] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int lr = lane & 15, lh = lane >> 4;
  auto compute = [&](int buf) {
    const char* Ds = smem + buf * (TCO + TCI) * ROWB;
    const char* Xs = Ds + TCO * ROWB;
    Frag<T> xf[RCI], df[RCO];
#pragma unroll
    for (int n = 0; n < RCI; ++n) {
      const int row = wci * RCI * 16 + n * 16 + lr;
      xf[n].lds(Xs + row * ROWB + ((lh ^ rswz<T>(row)) * 8 * ES));
    }
#pragma unroll
    for (int m = 0; m < RCO; ++m) {
      const int row = wco * RCO * 16 + m * 16 + lr;
      df[m].lds(Ds + row * ROWB + ((lh ^ rswz<T>(row)) * 8 * ES));
    }
#pragma unroll
    for (int n = 0; n < RCI; ++n)
#pragma unroll
      for (int m = 0; m < RCO; ++m) acc[n][m] = mma(xf[n], df[m], acc[n][m]);
  };

  if (nsteps > 0) {
    gload(0);
    lstore(0);
  }
  __syncthreads();
  for (int st = 0; st < nsteps; ++st) {
    const int cur = st & 1;
    if (st + 1 < nsteps) gload(st + 1);
    compute(cur);
    if (st + 1 < nsteps) lstore(cur ^ 1);
    __syncthreads();
  }

  // accumulator element i of tile (n, m): input channel lh * 4 + i, output channel lr
#pragma unroll
  for (int n = 0; n < RCI; ++n) {
    const int ci = ci0 + wci * RCI * 16 + n * 16 + lh * 4;
#pragma unroll
    for (int m = 0; m < RCO; ++m) {
      const int co = co0 + wco * RCO * 16 + m * 16 + lr;
      if (co < a.Cout && ci < a.Cin)   // Cin % 8 == 0: ci .. ci + 3 are all inside
        *reinterpret_cast<float4*>(a.slab + (((long)split * a.Cout + co) * a.taps + tap) * a.Cin + ci) =
            make_float4(acc[n][m][0], acc[n][m][1], acc[n][m][2], acc[n][m][3]);
    }
  }
}

// dw [cout][cin][taps] = sum over the splits, in split order, of slab [split][cout][taps][cin]
__global__ void conv3dg_wgrad_reduce_kernel(const float* __restrict__ slab, int nsplit, int cout, int cin, int taps,
                                            float* __restrict__ dw) {
  const long total = (long)cout * taps * cin;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int ci = (int)(idx % cin);
  const long t = idx / cin;
  const int tap = (int)(t % taps);
  const int co = (int)(t / taps);
  float s = 0.f;
  for (int k = 0; k < nsplit; ++k) s += slab[(long)k * total + idx];
  dw[((long)co * cin + ci) * taps + tap] = s;
}

// bias gradient in two fixed-order stages: part [nparts][cout], then db [cout]
template <typename T>
__global__ void conv3dg_db_partial_kernel(const T* __restrict__ dy, long P, int cout, long vper,
                                          float* __restrict__ part) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= cout) return;
  const long v0 = (long)blockIdx.y * vper;
  const long v1 = v0 + vper < P ? v0 + vper : P;
  float s = 0.f;
  for (long v = v0; v < v1; ++v) s += Elt<T>::to_f(dy[v * cout + c]);
  part[(long)blockIdx.y * cout + c] = s;
}
__global__ void conv3dg_db_final_kernel(const float* __restrict__ part, int nparts, int cout, float* __restrict__ db) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= cout) return;
  float s = 0.f;
  for (int p = 0; p < nparts; ++p) s += part[(long)p * cout + c];
  db[c] = s;
}

// backward of the nearest (1, 2, 2) upsample: out [rows][w][c] = the sum of the 2x2 phases of
// g [2 rows][2 w][c] (rows = n * d * h of the low-resolution volume; h even keeps a row pair inside
// one depth slice); one thread per 8-channel chunk, fp32 sum in a fixed order
template <typename T>
__global__ void conv3dg_upsample_bwd_kernel(const T* __restrict__ g, long rows, int w, int c, T* __restrict__ out) {
  const int c8n = c / 8;
  const long total = rows * w * c8n;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int c8 = (int)(idx % c8n);
  const long t = idx / c8n;
  const int x = (int)(t % w);
  const long r = t / w;
  float f[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] = 0.f;
#pragma unroll
  for (int ph = 0; ph < 4; ++ph) {
    Chunk8<T> v;
    v.load(g + (((2 * r + (ph >> 1)) * (2L * w) + 2 * x + (ph & 1)) * c) + c8 * 8);
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] += v.get(j);
  }
  Chunk8<T> o;
  o.set8(f);
  o.store(out + (r * w + x) * c + c8 * 8);
}

// reference layout w [cout][cin][taps] fp32 -> GEMM rows [rows_pad][kpad] of T, k = tap * 8 nch + c
// (zero padded).  transpose = 0: rows = cout, c = cin (forward); 1: rows = cin, c = cout, taps
// flipped (data gradient)
template <typename T>
__global__ void conv3dg_weight_prep_kernel(const float* __restrict__ w, int cout, int cin, int taps, int rows_pad,
                                           int nch, int kpad, int transpose, T* __restrict__ out) {
  const long total = (long)rows_pad * kpad;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int row = (int)(idx / kpad), k = (int)(idx - (long)row * kpad);
  const int tap = k / (nch * 8), c = k - tap * nch * 8;
  float v = 0.f;
  if (tap < taps) {
    if (!transpose) {
      if (row < cout && c < cin) v = w[((long)row * cin + c) * taps + tap];
    } else {
      if (row < cin && c < cout) v = w[((long)c * cin + row) * taps + (taps - 1 - tap)];
    }
  }
  out[idx] = Elt<T>::from_f(v);
}

// ---------------------------------------------------------------------------------------- host

constexpr int G3_ROWPAD = 64;   // weight rows are padded to the largest BN

int unsupported(const char* msg, int v) {
  fv_set_error(msg, v);
  return FV_E_UNSUPPORTED;
}

int checkg(const fv_conv3dg_desc* d) {
  FV_REQUIRE(d, "null conv3dg descriptor");
  FV_REQUIRE(d->dtype == FV_F32 || d->dtype == FV_BF16, "conv3dg dtype must be f32 or bf16");
  FV_REQUIRE(d->n > 0 && d->d > 0 && d->h > 0 && d->w > 0 && d->cout > 0, "bad conv3dg size");
  if (d->cin <= 0 || d->cin % 8) return unsupported("conv3dg: cin must be a positive multiple of 8 (got %d)", d->cin);
  if (d->ksize != 1 && d->ksize != 3 && d->ksize != 7) return unsupported("conv3dg: ksize 1, 3 or 7 (got %d)", d->ksize);
  if (d->upsample && (d->h % 2 || d->w % 2))
    return unsupported("conv3dg: an upsampled conv needs even output h and w (w = %d)", d->w);
  if ((long)d->n * d->d * d->h * d->w >= (1L << 31) - 4096)
    return unsupported("conv3dg: too many voxels (n = %d)", d->n);
  return FV_OK;
}

int taps_of(const fv_conv3dg_desc* d) { return d->ksize * d->ksize * d->ksize; }
int rows_pad(int rows) { return fv_cdiv(rows, G3_ROWPAD) * G3_ROWPAD; }
int nch_of(int c) { return fv_cdiv(c, 8); }
// k extent of a weight row: taps * (channels padded to 8), padded to the k step
int kpad_of(int taps, int c) { return fv_cdiv((long)taps * nch_of(c) * 8, BK) * BK; }
size_t esize(const fv_conv3dg_desc* d) { return d->dtype == FV_BF16 ? 2 : 4; }

template <typename T, int KS, bool UPS>
void launch_g3_t(const G3Args& a0, hipStream_t s) {
  G3Args a = a0;
  const int ntm = fv_cdiv(a.P, 128);
  if (a.Cout <= 16) {
    a.ntn = fv_cdiv(a.Cout, 16);
    hipLaunchKernelGGL((conv3dg_fwd_kernel<T, KS, 1, 4, 1, 2, UPS>), dim3(a.ntn * ntm), dim3(256), 0, s, a);
  } else if (a.Cout <= 32) {
    a.ntn = 1;
    hipLaunchKernelGGL((conv3dg_fwd_kernel<T, KS, 2, 2, 1, 4, UPS>), dim3(a.ntn * ntm), dim3(256), 0, s, a);
  } else if ((long)fv_cdiv(a.Cout, 64) * ntm < 256) {
    // the deep hourglass levels (64-512 voxels): the 64 x 128 tile leaves most of the 256 CUs
    // without a block, so a 32 x 64 tile gives four times the blocks
    a.ntn = fv_cdiv(a.Cout, 32);
    hipLaunchKernelGGL((conv3dg_fwd_kernel<T, KS, 2, 2, 1, 2, UPS>), dim3(a.ntn * fv_cdiv(a.P, 64)), dim3(256), 0, s, a);
  } else {
    a.ntn = fv_cdiv(a.Cout, 64);
    hipLaunchKernelGGL((conv3dg_fwd_kernel<T, KS, 2, 2, 2, 4, UPS>), dim3(a.ntn * ntm), dim3(256), 0, s, a);
  }
}

template <typename T>
void launch_g3(const G3Args& a, int ks, int ups, hipStream_t s) {
  if (ks == 1) {
    if (ups) launch_g3_t<T, 1, true>(a, s);
    else launch_g3_t<T, 1, false>(a, s);
  } else if (ks == 3) {
    if (ups) launch_g3_t<T, 3, true>(a, s);
    else launch_g3_t<T, 3, false>(a, s);
  } else {
    if (ups) launch_g3_t<T, 7, true>(a, s);
    else launch_g3_t<T, 7, false>(a, s);
  }
}

// x [n][d][hin][win][cx] * rows [cy][taps][cx] -> y [n][d][h][w][cy]
int run_g3(const fv_conv3dg_desc* d, int cx, int cy, int ups, const void* x, const void* w, const float* bias, void* y,
           hipStream_t s) {
  G3Args a{};
  a.x = x; a.w = w; a.bias = bias; a.y = y;
  a.N = d->n; a.D = d->d; a.H = d->h; a.W = d->w;
  a.Hin = ups ? d->h / 2 : d->h;
  a.Win = ups ? d->w / 2 : d->w;
  a.P = d->n * d->d * d->h * d->w;
  a.Cin = cx;
  a.nch = nch_of(cx);
  a.vec = cx % 8 == 0;
  a.Cout = cy;
  a.Kpad = kpad_of(taps_of(d), cx);
  a.nks = a.Kpad / BK;
  a.fnch = make_fastdiv((uint32_t)a.nch);
  if (d->dtype == FV_BF16) launch_g3<bf16>(a, d->ksize, ups, s);
  else launch_g3<float>(a, d->ksize, ups, s);
  return FV_OK;
}

struct WgPlan {
  int tco, tci, nco, nci, nsplit, vper, nparts;
  long dbper;
};
WgPlan wg_plan(const fv_conv3dg_desc* d) {
  WgPlan p;
  p.tco = d->cout <= 16 ? 16 : 64;
  p.tci = 64;
  p.nco = fv_cdiv(d->cout, p.tco);
  p.nci = fv_cdiv(d->cin, p.tci);
  const long P = (long)d->n * d->d * d->h * d->w;
  const long base = (long)p.nco * p.nci * taps_of(d);
  const long steps = (P + BK - 1) / BK;
  long ns = std::max(1L, 2048 / base);
  ns = std::min(ns, std::max(1L, steps / 4));
  const long slab = (long)d->cout * taps_of(d) * d->cin * 4;
  while (ns > 1 && ns * slab > (512L << 20)) ns /= 2;
  long vper = (P + ns - 1) / ns;
  vper = (vper + BK - 1) / BK * BK;
  p.vper = (int)vper;
  p.nsplit = (int)((P + vper - 1) / vper);
  p.nparts = (int)std::min(1024L, (P + 255) / 256);
  p.dbper = (P + p.nparts - 1) / p.nparts;
  p.nparts = (int)((P + p.dbper - 1) / p.dbper);
  return p;
}

}  // namespace

extern "C" {

int fv_conv3dg_check(const fv_conv3dg_desc* d) { return checkg(d); }

size_t fv_conv3dg_wk_bytes(const fv_conv3dg_desc* d) {
  if (checkg(d)) return 0;
  return (size_t)rows_pad(d->cout) * kpad_of(taps_of(d), d->cin) * esize(d);
}

size_t fv_conv3dg_wt_bytes(const fv_conv3dg_desc* d) {
  if (checkg(d)) return 0;
  return (size_t)rows_pad(d->cin) * kpad_of(taps_of(d), d->cout) * esize(d);
}

int fv_conv3dg_weight_prep(const fv_conv3dg_desc* d, const float* w, void* wk, void* wt, void* stream) {
  int st = checkg(d);
  if (st) return st;
  FV_REQUIRE(w, "null weight");
  hipStream_t s = (hipStream_t)stream;
  const int taps = taps_of(d);
  if (wk) {
    const int rp = rows_pad(d->cout), nch = nch_of(d->cin), kp = kpad_of(taps, d->cin);
    const int nb = fv_cdiv((long)rp * kp, 256);
    if (d->dtype == FV_BF16)
      hipLaunchKernelGGL(conv3dg_weight_prep_kernel<bf16>, dim3(nb), dim3(256), 0, s, w, d->cout, d->cin, taps, rp, nch,
                         kp, 0, (bf16*)wk);
    else
      hipLaunchKernelGGL(conv3dg_weight_prep_kernel<float>, dim3(nb), dim3(256), 0, s, w, d->cout, d->cin, taps, rp, nch,
                         kp, 0, (float*)wk);
    if ((st = fv_check_launch("conv3dg_weight_prep"))) return st;
  }
  if (wt) {
    const int rp = rows_pad(d->cin), nch = nch_of(d->cout), kp = kpad_of(taps, d->cout);
    const int nb = fv_cdiv((long)rp * kp, 256);
    if (d->dtype == FV_BF16)
      hipLaunchKernelGGL(conv3dg_weight_prep_kernel<bf16>, dim3(nb), dim3(256), 0, s, w, d->cout, d->cin, taps, rp, nch,
                         kp, 1, (bf16*)wt);
    else
      hipLaunchKernelGGL(conv3dg_weight_prep_kernel<float>, dim3(nb), dim3(256), 0, s, w, d->cout, d->cin, taps, rp, nch,
                         kp, 1, (float*)wt);
    if ((st = fv_check_launch("conv3dg_weight_prep_t"))) return st;
  }
  return FV_OK;
}

int fv_conv3dg_fwd(const fv_conv3dg_desc* d, const void* x, const void* wk, const float* bias, void* y, void* stream) {
  int st = checkg(d);
  if (st) return st;
  FV_REQUIRE(x && wk && y, "conv3dg_fwd: null pointer");
  run_g3(d, d->cin, d->cout, d->upsample, x, wk, bias, y, (hipStream_t)stream);
  return fv_check_launch("conv3dg_fwd");
}

int fv_conv3dg_bwd_data(const fv_conv3dg_desc* d, const void* dy, const void* wt, void* dx, void* stream) {
  int st = checkg(d);
  if (st) return st;
  FV_REQUIRE(dy && wt && dx, "conv3dg_bwd_data: null pointer");
  run_g3(d, d->cout, d->cin, 0, dy, wt, nullptr, dx, (hipStream_t)stream);
  return fv_check_launch("conv3dg_bwd_data");
}

int fv_conv3dg_upsample_bwd(const fv_conv3dg_desc* d, const void* g, void* out, void* stream) {
  int st = checkg(d);
  if (st) return st;
  FV_REQUIRE(g && out && d->upsample, "conv3dg_upsample_bwd: null pointer or not an upsampled conv");
  const long rows = (long)d->n * d->d * (d->h / 2);
  const int w = d->w / 2;
  const int nb = fv_cdiv(rows * w * (d->cin / 8), 256);
  hipStream_t s = (hipStream_t)stream;
  if (d->dtype == FV_BF16)
    hipLaunchKernelGGL(conv3dg_upsample_bwd_kernel<bf16>, dim3(nb), dim3(256), 0, s, (const bf16*)g, rows, w, d->cin,
                       (bf16*)out);
  else
    hipLaunchKernelGGL(conv3dg_upsample_bwd_kernel<float>, dim3(nb), dim3(256), 0, s, (const float*)g, rows, w, d->cin,
                       (float*)out);
  return fv_check_launch("conv3dg_upsample_bwd");
}

size_t fv_conv3dg_wgrad_ws_bytes(const fv_conv3dg_desc* d) {
  if (checkg(d)) return 0;
  const WgPlan p = wg_plan(d);
  return ((size_t)p.nsplit * d->cout * taps_of(d) * d->cin + (size_t)p.nparts * d->cout) * sizeof(float);
}

int fv_conv3dg_bwd_weight(const fv_conv3dg_desc* d, const void* x, const void* dy, float* dw, float* db, void* ws,
                          void* stream) {
  int st = checkg(d);
  if (st) return st;
  FV_REQUIRE(x && dy && dw && ws, "conv3dg_bwd_weight: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const WgPlan p = wg_plan(d);
  const int taps = taps_of(d);
  G3WArgs a{};
  a.x = x; a.dy = dy; a.slab = (float*)ws;
  a.N = d->n; a.D = d->d; a.H = d->h; a.W = d->w;
  a.Hin = d->upsample ? d->h / 2 : d->h;
  a.Win = d->upsample ? d->w / 2 : d->w;
  a.P = d->n * d->d * d->h * d->w;
  a.Cin = d->cin; a.Cout = d->cout; a.ks = d->ksize; a.ups = d->upsample; a.taps = taps;
  a.nci = p.nci; a.nco = p.nco; a.nsplit = p.nsplit; a.vper = p.vper;
  a.dyvec = d->cout % 8 == 0;
  a.fW = make_fastdiv((uint32_t)d->w);
  a.fH = make_fastdiv((uint32_t)d->h);
  a.fD = make_fastdiv((uint32_t)d->d);
  const long nblk = (long)p.nco * p.nci * taps * p.nsplit;
  FV_REQUIRE(nblk < (1L << 31), "conv3dg_bwd_weight: grid too large");
  const dim3 g((unsigned)nblk), bl(256);
  if (d->dtype == FV_BF16) {
    if (p.tco == 16) hipLaunchKernelGGL((conv3dg_wgrad_kernel<bf16, 1, 4, 1, 1>), g, bl, 0, s, a);
    else hipLaunchKernelGGL((conv3dg_wgrad_kernel<bf16, 2, 2, 2, 2>), g, bl, 0, s, a);
  } else {
    if (p.tco == 16) hipLaunchKernelGGL((conv3dg_wgrad_kernel<float, 1, 4, 1, 1>), g, bl, 0, s, a);
    else hipLaunchKernelGGL((conv3dg_wgrad_kernel<float, 2, 2, 2, 2>), g, bl, 0, s, a);
  }
  if ((st = fv_check_launch("conv3dg_wgrad"))) return st;
  const long total = (long)d->cout * taps * d->cin;
  hipLaunchKernelGGL(conv3dg_wgrad_reduce_kernel, dim3(fv_cdiv(total, 256)), dim3(256), 0, s, a.slab, p.nsplit, d->cout,
                     d->cin, taps, dw);
  if ((st = fv_check_launch("conv3dg_wgrad_reduce"))) return st;
  if (db) {
    float* part = a.slab + (size_t)p.nsplit * total;
    const dim3 gp(fv_cdiv(d->cout, 256), p.nparts);
    if (d->dtype == FV_BF16)
      hipLaunchKernelGGL(conv3dg_db_partial_kernel<bf16>, gp, dim3(256), 0, s, (const bf16*)dy, (long)a.P, d->cout,
                         p.dbper, part);
    else
      hipLaunchKernelGGL(conv3dg_db_partial_kernel<float>, gp, dim3(256), 0, s, (const float*)dy, (long)a.P, d->cout,
                         p.dbper, part);
    if ((st = fv_check_launch("conv3dg_db_partial"))) return st;
    hipLaunchKernelGGL(conv3dg_db_final_kernel, dim3(fv_cdiv(d->cout, 256)), dim3(256), 0, s, part, p.nparts, d->cout, db);
    if ((st = fv_check_launch("conv3dg_db"))) return st;
  }
  return FV_OK;
}

}  // extern "C"
