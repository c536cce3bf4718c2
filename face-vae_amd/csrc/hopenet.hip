// The frozen Hopenet teacher (trainer.py:16-88 of Luh1124/face-vae; a ResNet-50 run on 3 B images
// per generator step, trainer.py:278-280): the two operators its inference path needs beyond the
// stem, pool, 3x3 conv and pose-head entries.
//
//   fv_hopenet_prep_fwd   F.interpolate(apply_imagenet_normalization(x), size=(ho, wo)) (nearest,
//                         utils.py:182-186) in one pass: y = (x[src] - mean[c]) / std[c], true fp32
//                         subtraction and IEEE division (bit-equal to torch on the CPU), with ATen's
//                         legacy nearest source index min((int)floorf(dst * scale), in - 1),
//                         scale = (float)in / (float)out.  One thread per output pixel, W fastest; the
//                         source index is shared by the 3 planes.  NCHW fp32 in and out.
//   fv_pw_infer_*         a 1x1 convolution of a frozen network as a GEMM on the matrix units:
//                         y[p][co] = out_act(sum_ci in_act(x[src(p)][ci]) wk[co][ci] + shift[co] + res[p][co])
//                         with wk = w * scale[co] (the folded batch norm) rounded once to the storage
//                         dtype, the stride of a stride-2 1x1 conv folded into the pixel row address,
//                         ReLU of the input folded into the LDS staging and the residual add and the
//                         output ReLU into the store.  No BN records, nothing saved: no gradient.
//
// pw_infer_kernel is the LDS-staged form of conv_fwd_kernel (conv_fwd.hip) specialised to K = cin:
// BM pixels x BN channels per block of 4 waves, 32 k per step, global loads of step k + 1 in flight
// over the MFMAs of step k, two LDS buffers, one barrier per step.  Pixel rows past P and channel
// rows past cout are predicated: they load nothing (zeros are staged) and store nothing.  The weight
// rows are staged in a permuted order so that every lane ends up with 8 consecutive output channels of
// a pixel, stored (and the residual read) as 16-B accesses without a pass through LDS.
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

// ------------------------------------------------------------------------------------
// preprocessing
// ------------------------------------------------------------------------------------
struct Prep3 {
  float mean[3], std[3];
};

__global__ void __launch_bounds__(NT) hopenet_prep_kernel(const float* __restrict__ x, int H, int W, int Ho, int Wo,
                                                          float sh, float sw, Prep3 c, float* __restrict__ y) {
#pragma clang fp contract(off)
  const int n = blockIdx.y;
  const int HWo = Ho * Wo;                         // < 2^31 - NT (checked by the entry)
  const int pix = blockIdx.x * NT + threadIdx.x;
  if (pix >= HWo) return;
  const int oi = pix / Wo, oj = pix - oi * Wo;
  const int si = min((int)floorf((float)oi * sh), H - 1);
  const int sj = min((int)floorf((float)oj * sw), W - 1);
  const long HW = (long)H * W;
  const float* xp = x + (long)n * 3 * HW + (long)si * W + sj;
  float* yp = y + (long)n * 3 * HWo + pix;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) yp[(long)ch * HWo] = __fdiv_rn(xp[ch * HW] - c.mean[ch], c.std[ch]);
}

// ------------------------------------------------------------------------------------
// pointwise inference GEMM
// ------------------------------------------------------------------------------------
struct PwArgs {
  const void* x;
  const void* wk;
  const float* shift;
  const void* res;
  void* y;
  int P;              // output pixels n * ho * wo
  int Ho, Wo, Win;    // output plane and the input row length
  long HWin;          // input pixels per sample
  int stride;
  int Cin, Cout, nks, ntn;
  int in_relu, out_relu;
};

template <typename T>
__global__ void __launch_bounds__(NT) pw_weight_prep_kernel(const float* __restrict__ w, const float* __restrict__ scale,
                                                            int cin, long total, T* __restrict__ wk) {
#pragma clang fp contract(off)
  const long i = (long)blockIdx.x * NT + threadIdx.x;
  if (i >= total) return;
  const float s = scale ? scale[i / cin] : 1.f;
  wk[i] = Elt<T>::from_f(w[i] * s);
}

template <typename T, int WN, int WM, int RN, int RM>
__global__ void __launch_bounds__(64 * WN * WM) pw_infer_kernel(PwArgs a) {
  constexpr int NTK = 64 * WN * WM;
  constexpr int BN = WN * RN * 16;   // output channels per block
  constexpr int BM = WM * RM * 16;   // pixels per block
  constexpr int ES = sizeof(T);
  constexpr int ROWB = BK * ES;
  constexpr int CA = BM * 4 / NTK;
  constexpr int CB = BN * 4 / NTK;
  static_assert((BM * 4) % NTK == 0 && (BN * 4) % NTK == 0, "staging");
  __shared__ __attribute__((aligned(16))) char smem[2 * (BM + BN) * ROWB];

  const T* __restrict__ x = reinterpret_cast<const T*>(a.x);
  const T* __restrict__ wk = reinterpret_cast<const T*>(a.wk);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wn = wave % WN, wm = wave / WN;
  const int tn = blockIdx.x % a.ntn, tm = blockIdx.x / a.ntn;
  const int co0 = tn * BN, p0 = tm * BM;
  const int kc = tid & 3;

  // the input row of each staged pixel: src(p) = (n, stride * i, stride * j); -1: past the last pixel
  long xrow[CA];
#pragma unroll
  for (int i = 0; i < CA; ++i) {
    const int pix = p0 + (tid >> 2) + i * (NTK / 4);
    xrow[i] = -1;
    if (pix < a.P) {
      const int hwo = a.Ho * a.Wo;
      const int n = pix / hwo, rem = pix - n * hwo;
      const int oi = rem / a.Wo, oj = rem - oi * a.Wo;
      xrow[i] = ((long)n * a.HWin + (long)(oi * a.stride) * a.Win + oj * a.stride) * a.Cin;
    }
  }
  // LDS row -> output channel, permuted inside each group of 32 rows (two MFMA row tiles t = 0, 1 of
  // 16 rows r): row 16 t + r holds channel 8 (r >> 2) + 4 t + (r & 3).  A lane's 4 accumulator rows
  // 4 lh + i of the two tiles are then the 8 CONSECUTIVE channels 8 lh .. 8 lh + 7 of the group, which
  // the epilogue moves as one 16-B (bf16) or two 16-B (fp32) accesses per pixel; the fragment reads
  // keep their consecutive, conflict-free rows.
  long wrow[CB];
#pragma unroll
  for (int j = 0; j < CB; ++j) {
    const int row = (tid >> 2) + j * (NTK / 4);
    const int r = row & 15, t = (row >> 4) & 1;
    const int co = co0 + (row & ~31) + (r >> 2) * 8 + t * 4 + (r & 3);
    wrow[j] = co < a.Cout ? (long)co * a.Cin : -1;
  }

  Chunk8<T> ra[CA], rb[CB];
  auto gload = [&](int ks) {
    const int k = ks * BK + kc * 8;
#pragma unroll
    for (int i = 0; i < CA; ++i) {
      if (xrow[i] >= 0) ra[i].load(x + xrow[i] + k);
      else ra[i].zero();
    }
#pragma unroll
    for (int j = 0; j < CB; ++j) {
      if (wrow[j] >= 0) rb[j].load(wk + wrow[j] + k);
      else rb[j].zero();
    }
  };
  auto lstore = [&](int buf) {
    char* As = smem + buf * (BM + BN) * ROWB;
    char* Bs = As + BM * ROWB;
#pragma unroll
    for (int i = 0; i < CA; ++i) {
      const int row = (tid >> 2) + i * (NTK / 4);
      Chunk8<T> c = ra[i];
      if (a.in_relu) {
        float f[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) f[j] = fmaxf(c.get(j), 0.f);
        c.set8(f);
      }
      c.store(reinterpret_cast<T*>(As + row * ROWB + ((kc ^ rswz<T>(row)) * 8 * ES)));
    }
#pragma unroll
    for (int j = 0; j < CB; ++j) {
      const int row = (tid >> 2) + j * (NTK / 4);
      rb[j].store(reinterpret_cast<T*>(Bs + row * ROWB + ((kc ^ rswz<T>(row)) * 8 * ES)));
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

  // epilogue: acc[2 q + t][m][i] is channel co0 + wn RN 16 + 32 q + 8 lh + 4 t + i of pixel
  // p0 + (wm RM + m) 16 + lr (the row permutation above).  cout is a multiple of 32, so a group of 32
  // channels is valid or invalid as a whole.
  static_assert(RN % 2 == 0, "channel tiles come in pairs");
  T* __restrict__ y = reinterpret_cast<T*>(a.y);
  const T* __restrict__ res = reinterpret_cast<const T*>(a.res);
#pragma unroll
  for (int q = 0; q < RN / 2; ++q) {
    const int cb = co0 + wn * RN * 16 + q * 32 + lh * 8;
    if (cb >= a.Cout) continue;
    float sv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (a.shift) {
      const float4 s0 = *reinterpret_cast<const float4*>(a.shift + cb);
      const float4 s1 = *reinterpret_cast<const float4*>(a.shift + cb + 4);
      sv[0] = s0.x; sv[1] = s0.y; sv[2] = s0.z; sv[3] = s0.w;
      sv[4] = s1.x; sv[5] = s1.y; sv[6] = s1.z; sv[7] = s1.w;
    }
#pragma unroll
    for (int m = 0; m < RM; ++m) {
      const int pix = p0 + wm * RM * 16 + m * 16 + lr;
      if (pix >= a.P) continue;
      const long o = (long)pix * a.Cout + cb;
      float f[8];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        f[i] = acc[2 * q][m][i] + sv[i];
        f[4 + i] = acc[2 * q + 1][m][i] + sv[4 + i];
      }
      if (res) {
        Chunk8<T> r;
        r.load(res + o);
#pragma unroll
        for (int i = 0; i < 8; ++i) f[i] += r.get(i);
      }
      if (a.out_relu) {
#pragma unroll
        for (int i = 0; i < 8; ++i) f[i] = fmaxf(f[i], 0.f);
      }
      Chunk8<T> c;
      c.set8(f);
      c.store(y + o);
    }
  }
}

int pw_check(const fv_pw_desc* d) {
  FV_REQUIRE(d, "pw_infer: null descriptor");
  FV_SUPPORTED(d->dtype == FV_F32 || d->dtype == FV_BF16, "pw_infer: dtype must be FV_F32 or FV_BF16");
  FV_SUPPORTED(d->n >= 1 && d->h >= 1 && d->w >= 1, "pw_infer: n, h, w must be at least 1 (got %d, %d x %d)", d->n, d->h,
               d->w);
  FV_SUPPORTED(d->stride == 1 || d->stride == 2, "pw_infer: stride must be 1 or 2 (got %d)", d->stride);
  FV_SUPPORTED(d->stride == 1 || (d->h % 2 == 0 && d->w % 2 == 0), "pw_infer: stride 2 needs even h, w (got %d x %d)",
               d->h, d->w);
  FV_SUPPORTED(d->cin >= 32 && d->cin <= 4096 && d->cin % 32 == 0, "pw_infer: cin must be a multiple of 32 in [32, 4096] (got %d)",
               d->cin);
  FV_SUPPORTED(d->cout >= 32 && d->cout <= 4096 && d->cout % 32 == 0,
               "pw_infer: cout must be a multiple of 32 in [32, 4096] (got %d)", d->cout);
  // 32-bit pixel and block indices: input and output pixel counts, and the grid of the smallest tile
  FV_SUPPORTED((long)d->n * d->h * d->w < (1L << 31) - 256, "pw_infer: n * h * w must be below 2^31 - 256");
  return FV_OK;
}

bool overlaps(const void* a, size_t na, const void* b, size_t nb) {
  const char* pa = (const char*)a;
  const char* pb = (const char*)b;
  return pa < pb + nb && pb < pa + na;
}

template <typename T>
void pw_launch(const PwArgs& a0, hipStream_t s) {
  PwArgs a = a0;
  // 128-channel tiles where the output divides into them and there are pixel tiles enough to fill the
  // chip; else the 64-channel tile (every cout is a multiple of 32: the last tile may be half empty)
  if (a.Cout % 128 == 0 && (long)fv_cdiv(a.P, 128) * (a.Cout / 128) >= 256) {
    a.ntn = a.Cout / 128;
    hipLaunchKernelGGL((pw_infer_kernel<T, 2, 2, 4, 4>), dim3(a.ntn * fv_cdiv(a.P, 128)), dim3(256), 0, s, a);
  } else {
    a.ntn = fv_cdiv(a.Cout, 64);
    hipLaunchKernelGGL((pw_infer_kernel<T, 2, 2, 2, 4>), dim3(a.ntn * fv_cdiv(a.P, 128)), dim3(256), 0, s, a);
  }
}

}  // namespace

extern "C" {

int fv_hopenet_prep_fwd(const float* x, int n, int h, int w, int ho, int wo, const float* mean, const float* std, float* y,
                        void* stream) {
  FV_SUPPORTED(n >= 1 && n <= 65535, "hopenet_prep_fwd: N must be in [1, 65535] (got %d)", n);
  FV_SUPPORTED(h >= 1 && w >= 1 && ho >= 1 && wo >= 1, "hopenet_prep_fwd: every size must be at least 1 (got %d x %d -> %d x %d)",
               h, w, ho, wo);
  FV_SUPPORTED((long)h * w < 0x7fffffffL - 256 && (long)ho * wo < 0x7fffffffL - 256,
               "hopenet_prep_fwd: H * W of the input and of the output must be below 2^31 - 256");
  FV_REQUIRE(x && y && mean && std, "hopenet_prep_fwd: null pointer");
  Prep3 c;
  for (int i = 0; i < 3; ++i) {
    c.mean[i] = mean[i];
    c.std[i] = std[i];
  }
  const float sh = (float)h / (float)ho, sw = (float)w / (float)wo;
  const dim3 grid(fv_cdiv((long)ho * wo, NT), n);
  hipLaunchKernelGGL(hopenet_prep_kernel, grid, dim3(NT), 0, (hipStream_t)stream, x, h, w, ho, wo, sh, sw, c, y);
  return fv_check_launch("hopenet_prep_fwd");
}

size_t fv_pw_infer_wk_elems(const fv_pw_desc* d) {
  if (pw_check(d) != FV_OK) return 0;
  return (size_t)d->cout * d->cin;
}

int fv_pw_infer_weight_prep(const fv_pw_desc* d, const float* w, const float* scale, void* wk, void* stream) {
  const int st = pw_check(d);
  if (st) return st;
  FV_REQUIRE(w && wk, "pw_infer_weight_prep: null pointer");
  const long total = (long)d->cout * d->cin;
  const dim3 grid(fv_cdiv(total, NT));
  hipStream_t s = (hipStream_t)stream;
  if (d->dtype == FV_BF16) hipLaunchKernelGGL(pw_weight_prep_kernel<bf16>, grid, dim3(NT), 0, s, w, scale, d->cin, total, (bf16*)wk);
  else hipLaunchKernelGGL(pw_weight_prep_kernel<float>, grid, dim3(NT), 0, s, w, scale, d->cin, total, (float*)wk);
  return fv_check_launch("pw_infer_weight_prep");
}

int fv_pw_infer_fwd(const fv_pw_desc* d, const void* x, const void* wk, const float* shift, const void* res, void* y,
                    void* stream) {
  const int st = pw_check(d);
  if (st) return st;
  FV_REQUIRE(x && wk && y, "pw_infer_fwd: null pointer");
  const size_t es = d->dtype == FV_BF16 ? 2 : 4;
  const int ho = d->h / d->stride, wo = d->w / d->stride;
  const size_t xbytes = (size_t)d->n * d->h * d->w * d->cin * es;
  const size_t ybytes = (size_t)d->n * ho * wo * d->cout * es;
  FV_REQUIRE(!overlaps(y, ybytes, x, xbytes), "pw_infer_fwd: y must not alias x");
  FV_REQUIRE(!res || !overlaps(y, ybytes, res, ybytes), "pw_infer_fwd: y must not alias res");
  PwArgs a{};
  a.x = x; a.wk = wk; a.shift = shift; a.res = res; a.y = y;
  a.P = d->n * ho * wo;
  a.Ho = ho; a.Wo = wo; a.Win = d->w; a.HWin = (long)d->h * d->w;
  a.stride = d->stride;
  a.Cin = d->cin; a.Cout = d->cout; a.nks = d->cin / BK;
  a.in_relu = d->in_relu != 0; a.out_relu = d->out_relu != 0;
  if (d->dtype == FV_BF16) pw_launch<bf16>(a, (hipStream_t)stream);
  else pw_launch<float>(a, (hipStream_t)stream);
  return fv_check_launch("pw_infer_fwd");
}

}  // extern "C"
