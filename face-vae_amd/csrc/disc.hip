// Patch-discriminator operators for gfx950 that the FaceVAE path has no kernel for
// (Discriminator, models.py:1114-1139): instance norm + LeakyReLU over NHWC activations and the
// discriminator's input assembly (image + keypoint heatmaps).  The stride-2 convolutions are in
// conv.hip (fv_conv2d_s2_*).
//
// Instance norm (nn.InstanceNorm2d(C, affine=True), modules.py:21): statistics per (n, c) over
// the H*W plane, biased variance, eps inside the square root, no running statistics.  Every sum
// is a fixed-order two-level reduction (per-thread fp32 over at most IN_RUN pixels, then fp64
// through LDS and a partials buffer): no atomics, so results are bit-reproducible and a sample
// never sees another sample's data.
#include "common.h"

namespace {

constexpr int IN_NT = 256;    // threads per block of the reductions
constexpr int IN_RUN = 8;     // pixels a thread sums in fp32 before the fp64 levels
constexpr int IN_MAXS = 64;   // splits of a plane

// splits of one H*W plane: a block covers rpb = IN_NT / (C / 8) pixel rows per pass
int in_splits(long hw, int c) {
  const long rpb = IN_NT / (c / 8);
  long s = (hw + rpb * IN_RUN - 1) / (rpb * IN_RUN);
  return (int)(s < 1 ? 1 : (s > IN_MAXS ? IN_MAXS : s));
}

int in_check(int dtype, int n, int h, int w, int c) {
  FV_REQUIRE(dtype == FV_F32 || dtype == FV_BF16, "instance norm: dtype must be f32 or bf16");
  FV_REQUIRE(n > 0 && h > 0 && w > 0, "instance norm: bad size");
  FV_REQUIRE(fv_ilog2(c) >= 3 && c <= 512, "instance norm: channels must be a power of two in [8, 512] (got %d)", c);
  FV_REQUIRE((long)n * h * w * c < (1L << 31), "instance norm: tensor larger than 2^31 elements");
  return FV_OK;
}

// Two sums per (n, split, c) over the split's pixels of plane n, into part[n][split][2][C] (fp64).
// MODE 0: (x, x^2).  MODE 1: (g, g * xhat) with g = dout * leaky'(gamma * xhat + beta),
// xhat = (x - mean[n][c]) * invstd[n][c].
// Block (n, split): thread t owns the 8-channel chunk t % (C / 8) of pixel rows t / (C / 8) + k * rpb.
template <typename T, int MODE>
__global__ void __launch_bounds__(IN_NT)
in_reduce_kernel(const T* __restrict__ x, const T* __restrict__ dout, int HW, int C, int S, const float* mean,
                 const float* invstd, const float* gamma, const float* beta, float slope, double* part) {
  __shared__ double red[IN_NT][17];   // (+1: rows of 16 doubles would all start on one bank group)
  const int n = blockIdx.x / S, sp = blockIdx.x - n * S;
  const int c8 = C >> 3, rpb = IN_NT / c8;
  const int tid = threadIdx.x, ch = tid % c8, row = tid / c8;
  const int per = (HW + S - 1) / S;
  const int p0 = sp * per, p1 = min(HW, p0 + per);
  const int c0 = ch * 8;
  float mu[8], is[8], ga[8], be[8];
  if constexpr (MODE == 1) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      mu[j] = mean[n * C + c0 + j];
      is[j] = invstd[n * C + c0 + j];
      ga[j] = gamma[c0 + j];
      be[j] = beta[c0 + j];
    }
  }
  double a0[8], a1[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) a0[j] = a1[j] = 0.0;
  float f0[8], f1[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) f0[j] = f1[j] = 0.f;
  int run = 0;
  for (int p = p0 + row; p < p1; p += rpb) {
    const long off = ((long)n * HW + p) * C + c0;
    Chunk8<T> v;
    v.load(x + off);
    if constexpr (MODE == 0) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float e = v.get(j);
        f0[j] += e;
        f1[j] += e * e;
      }
    } else {
      Chunk8<T> dv;
      dv.load(dout + off);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float xh = (v.get(j) - mu[j]) * is[j];
        const float d = dv.get(j);
        const float g = ga[j] * xh + be[j] > 0.f ? d : d * slope;
        f0[j] += g;
        f1[j] += g * xh;
      }
    }
    if (++run == IN_RUN) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        a0[j] += (double)f0[j];
        a1[j] += (double)f1[j];
        f0[j] = f1[j] = 0.f;
      }
      run = 0;
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    red[tid][j] = a0[j] + (double)f0[j];
    red[tid][8 + j] = a1[j] + (double)f1[j];
  }
  __syncthreads();
  for (int idx = tid; idx < 2 * C; idx += IN_NT) {
    const int which = idx / C, c = idx - which * C;
    const int col = which * 8 + (c & 7), chunk = c >> 3;
    double t = 0.0;
    for (int r = 0; r < rpb; ++r) t += red[r * c8 + chunk][col];
    part[((long)(n * S + sp) * 2 + which) * C + c] = t;
  }
}

// statistics of plane (n, c) from its S partials: mean, invstd = 1 / sqrt(biased var + eps)
__global__ void in_stats_finalize_kernel(const double* __restrict__ part, int NC, int C, int S, double hw, float eps,
                                         float* mean, float* invstd) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= NC) return;
  const int n = i / C, c = i - n * C;
  double s = 0.0, q = 0.0;
  for (int sp = 0; sp < S; ++sp) {
    s += part[((long)(n * S + sp) * 2) * C + c];
    q += part[((long)(n * S + sp) * 2 + 1) * C + c];
  }
  const double m = s / hw;
  double var = q / hw - m * m;
  if (var < 0.0) var = 0.0;
  mean[i] = (float)m;
  invstd[i] = (float)(1.0 / sqrt(var + (double)eps));
}

// backward sums of plane (n, c): k[n][0][c] = mean(g), k[n][1][c] = mean(g * xhat), and the
// plane totals tot[n][2][C] (fp64) the parameter gradients are summed from
__global__ void in_bwd_finalize_kernel(const double* __restrict__ part, int NC, int C, int S, double hw, float* k,
                                       double* tot) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= NC) return;
  const int n = i / C, c = i - n * C;
  double s = 0.0, q = 0.0;
  for (int sp = 0; sp < S; ++sp) {
    s += part[((long)(n * S + sp) * 2) * C + c];
    q += part[((long)(n * S + sp) * 2 + 1) * C + c];
  }
  k[(long)(n * 2) * C + c] = (float)(s / hw);
  k[(long)(n * 2 + 1) * C + c] = (float)(q / hw);
  tot[(long)(n * 2) * C + c] = s;
  tot[(long)(n * 2 + 1) * C + c] = q;
}

// dgamma[c] = sum_n sum(g * xhat), dbeta[c] = sum_n sum(g), samples in order
__global__ void in_param_grad_kernel(const double* __restrict__ tot, int N, int C, float* dgamma, float* dbeta) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double s = 0.0, q = 0.0;
  for (int n = 0; n < N; ++n) {
    s += tot[(long)(n * 2) * C + c];
    q += tot[(long)(n * 2 + 1) * C + c];
  }
  dgamma[c] = (float)q;
  dbeta[c] = (float)s;
}

// MODE 0: y = leaky(gamma * xhat + beta).  MODE 1: dx = gamma * invstd * (g - mean(g) - xhat * mean(g xhat)).
// One thread per 8-channel chunk.
template <typename T, int MODE>
__global__ void in_apply_kernel(const T* __restrict__ x, const T* __restrict__ dout, long nchunks, int HW, int lgc8,
                                const float* __restrict__ mean, const float* __restrict__ invstd,
                                const float* __restrict__ gamma, const float* __restrict__ beta, float slope,
                                const float* __restrict__ k, T* __restrict__ out) {
  const int C = 8 << lgc8;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < nchunks; e += (long)gridDim.x * blockDim.x) {
    const long pix = e >> lgc8;
    const int c0 = (int)(e & ((1 << lgc8) - 1)) * 8;
    const int n = (int)(pix / HW);
    Chunk8<T> v;
    v.load(x + e * 8);
    float f[8];
    if constexpr (MODE == 0) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float xh = (v.get(j) - mean[n * C + c0 + j]) * invstd[n * C + c0 + j];
        f[j] = fv_act(gamma[c0 + j] * xh + beta[c0 + j], slope);
      }
    } else {
      Chunk8<T> dv;
      dv.load(dout + e * 8);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float is = invstd[n * C + c0 + j];
        const float xh = (v.get(j) - mean[n * C + c0 + j]) * is;
        const float d = dv.get(j);
        const float g = gamma[c0 + j] * xh + beta[c0 + j] > 0.f ? d : d * slope;
        f[j] = gamma[c0 + j] * is * (g - k[(n * 2) * C + c0 + j] - xh * k[(n * 2 + 1) * C + c0 + j]);
      }
    }
    Chunk8<T> o;
    o.set8(f);
    o.store(out + e * 8);
  }
}

// Discriminator input (models.py:1131-1132, utils.py:79-88, 121-127): NHWC [N, H, W, Cp],
// channels 0-2 the NCHW fp32 image, channel 3 + k the keypoint heatmap
// exp(-0.5 ((gx - kp_x)^2 + (gy - kp_y)^2) / 0.01) on the [-1, 1] grid (kp[..., 0] pairs with
// the width axis), the padding channels 0.  One thread per pixel.
constexpr int DISC_MAXC = 32;
template <typename T>
__global__ void disc_input_kernel(const float* __restrict__ img, const float* __restrict__ kp, int N, int H, int W,
                                  int K, int kpd, int Cp, T* __restrict__ out) {
  const long P = (long)N * H * W;
  const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  const int HW = H * W;
  const int n = (int)(p / HW), rem = (int)(p - (long)n * HW);
  const int h = rem / W, w = rem - h * W;
  const float gx = 2.f * ((float)w / (float)(W - 1)) - 1.f;
  const float gy = 2.f * ((float)h / (float)(H - 1)) - 1.f;
  float f[DISC_MAXC];
#pragma unroll
  for (int c = 0; c < DISC_MAXC; ++c) f[c] = 0.f;
#pragma unroll
  for (int c = 0; c < 3; ++c) f[c] = img[((long)n * 3 + c) * HW + rem];
#pragma unroll
  for (int c = 3; c < DISC_MAXC; ++c) {
    const int q = c - 3;
    if (q < K) {
      const float dx = gx - kp[((long)n * K + q) * kpd], dy = gy - kp[((long)n * K + q) * kpd + 1];
      f[c] = expf(-0.5f * (dx * dx + dy * dy) / 0.01f);
    }
  }
#pragma unroll
  for (int c8 = 0; c8 < DISC_MAXC / 8; ++c8) {
    if (c8 * 8 < Cp) {
      Chunk8<T> o;
      o.set8(f + c8 * 8);
      o.store(out + p * Cp + c8 * 8);
    }
  }
}

template <typename T, int MODE>
void launch_in_reduce(const void* x, const void* dout, int n, int hw, int c, int S, const float* mean,
                      const float* invstd, const float* gamma, const float* beta, float slope, double* part,
                      hipStream_t s) {
  hipLaunchKernelGGL((in_reduce_kernel<T, MODE>), dim3(n * S), dim3(IN_NT), 0, s, (const T*)x, (const T*)dout, hw, c, S,
                     mean, invstd, gamma, beta, slope, part);
}

template <typename T, int MODE>
void launch_in_apply(const void* x, const void* dout, int n, int hw, int c, const float* mean, const float* invstd,
                     const float* gamma, const float* beta, float slope, const float* k, void* out, hipStream_t s) {
  const long nchunks = (long)n * hw * (c / 8);
  const int nb = (int)(nchunks + 255 < 256L * 8192 ? (nchunks + 255) / 256 : 8192);
  hipLaunchKernelGGL((in_apply_kernel<T, MODE>), dim3(nb), dim3(256), 0, s, (const T*)x, (const T*)dout, nchunks, hw,
                     fv_ilog2(c / 8), mean, invstd, gamma, beta, slope, k, (T*)out);
}

}  // namespace

extern "C" {

size_t fv_in_ws_bytes(int n, int h, int w, int c) {
  if (n <= 0 || h <= 0 || w <= 0 || fv_ilog2(c) < 3 || c > 512) return 0;
  return ((size_t)n * in_splits((long)h * w, c) * 2 * c + (size_t)n * 2 * c) * sizeof(double);
}

int fv_in_stats(int dtype, const void* x, int n, int h, int w, int c, float eps, float* mean, float* invstd, void* ws,
                void* stream) {
  int st = in_check(dtype, n, h, w, c);
  if (st) return st;
  FV_REQUIRE(x && mean && invstd && ws, "null pointer");
  hipStream_t s = (hipStream_t)stream;
  const int hw = h * w, S = in_splits(hw, c);
  double* part = (double*)ws;
  if (dtype == FV_BF16) launch_in_reduce<bf16, 0>(x, nullptr, n, hw, c, S, nullptr, nullptr, nullptr, nullptr, 0.f, part, s);
  else launch_in_reduce<float, 0>(x, nullptr, n, hw, c, S, nullptr, nullptr, nullptr, nullptr, 0.f, part, s);
  if ((st = fv_check_launch("in_stats"))) return st;
  hipLaunchKernelGGL(in_stats_finalize_kernel, dim3(fv_cdiv((long)n * c, 256)), dim3(256), 0, s, part, n * c, c, S,
                     (double)hw, eps, mean, invstd);
  return fv_check_launch("in_stats_finalize");
}

int fv_in_act_fwd(int dtype, const void* x, int n, int h, int w, int c, const float* mean, const float* invstd,
                  const float* gamma, const float* beta, float slope, void* y, void* stream) {
  int st = in_check(dtype, n, h, w, c);
  if (st) return st;
  FV_REQUIRE(x && mean && invstd && gamma && beta && y, "null pointer");
  FV_REQUIRE(fv_slope_ok(slope), "slope must be in [0, 1] (got %g)", (double)slope);
  if (dtype == FV_BF16)
    launch_in_apply<bf16, 0>(x, nullptr, n, h * w, c, mean, invstd, gamma, beta, slope, nullptr, y, (hipStream_t)stream);
  else
    launch_in_apply<float, 0>(x, nullptr, n, h * w, c, mean, invstd, gamma, beta, slope, nullptr, y, (hipStream_t)stream);
  return fv_check_launch("in_act_fwd");
}

int fv_in_act_bwd_reduce(int dtype, const void* dout, const void* x, int n, int h, int w, int c, const float* mean,
                         const float* invstd, const float* gamma, const float* beta, float slope, float* dgamma,
                         float* dbeta, float* k, void* ws, void* stream) {
  int st = in_check(dtype, n, h, w, c);
  if (st) return st;
  FV_REQUIRE(dout && x && mean && invstd && gamma && beta && dgamma && dbeta && k && ws, "null pointer");
  FV_REQUIRE(fv_slope_ok(slope), "slope must be in [0, 1] (got %g)", (double)slope);
  hipStream_t s = (hipStream_t)stream;
  const int hw = h * w, S = in_splits(hw, c);
  double* part = (double*)ws;
  double* tot = part + (size_t)n * S * 2 * c;
  if (dtype == FV_BF16) launch_in_reduce<bf16, 1>(x, dout, n, hw, c, S, mean, invstd, gamma, beta, slope, part, s);
  else launch_in_reduce<float, 1>(x, dout, n, hw, c, S, mean, invstd, gamma, beta, slope, part, s);
  if ((st = fv_check_launch("in_act_bwd_reduce"))) return st;
  hipLaunchKernelGGL(in_bwd_finalize_kernel, dim3(fv_cdiv((long)n * c, 256)), dim3(256), 0, s, part, n * c, c, S,
                     (double)hw, k, tot);
  hipLaunchKernelGGL(in_param_grad_kernel, dim3(fv_cdiv(c, 64)), dim3(64), 0, s, tot, n, c, dgamma, dbeta);
  return fv_check_launch("in_act_bwd_finalize");
}

int fv_in_act_bwd_apply(int dtype, const void* dout, const void* x, int n, int h, int w, int c, const float* mean,
                        const float* invstd, const float* gamma, const float* beta, float slope, const float* k,
                        void* dx, void* stream) {
  int st = in_check(dtype, n, h, w, c);
  if (st) return st;
  FV_REQUIRE(dout && x && mean && invstd && gamma && beta && k && dx, "null pointer");
  FV_REQUIRE(fv_slope_ok(slope), "slope must be in [0, 1] (got %g)", (double)slope);
  if (dtype == FV_BF16)
    launch_in_apply<bf16, 1>(x, dout, n, h * w, c, mean, invstd, gamma, beta, slope, k, dx, (hipStream_t)stream);
  else
    launch_in_apply<float, 1>(x, dout, n, h * w, c, mean, invstd, gamma, beta, slope, k, dx, (hipStream_t)stream);
  return fv_check_launch("in_act_bwd_apply");
}

int fv_disc_input_fwd(int dtype, const float* img, const float* kp, int n, int h, int w, int k, int kp_stride, int ldc,
                      void* out, void* stream) {
  FV_REQUIRE(dtype == FV_F32 || dtype == FV_BF16, "disc input: dtype must be f32 or bf16");
  FV_REQUIRE(img && out && n > 0 && h > 1 && w > 1, "disc input: null pointer or bad size (h, w >= 2)");
  FV_REQUIRE(k >= 0 && 3 + k <= DISC_MAXC, "disc input: 3 + K must be <= %d (got K = %d)", DISC_MAXC, k);
  FV_REQUIRE(k == 0 || (kp && kp_stride >= 2), "disc input: keypoints need a stride >= 2");
  FV_REQUIRE(fv_ilog2(ldc) >= 3 && ldc >= 3 + k && ldc <= DISC_MAXC, "disc input: channel stride must be a power of two "
             "in [8, %d] holding 3 + K channels (got %d)", DISC_MAXC, ldc);
  FV_REQUIRE((long)n * h * w * ldc < (1L << 31), "disc input: tensor larger than 2^31 elements");
  const long P = (long)n * h * w;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == FV_BF16)
    hipLaunchKernelGGL(disc_input_kernel<bf16>, dim3(fv_cdiv(P, 256)), dim3(256), 0, s, img, kp, n, h, w, k, kp_stride,
                       ldc, (bf16*)out);
  else
    hipLaunchKernelGGL(disc_input_kernel<float>, dim3(fv_cdiv(P, 256)), dim3(256), 0, s, img, kp, n, h, w, k, kp_stride,
                       ldc, (float*)out);
  return fv_check_launch("disc_input_fwd");
}

}  // extern "C"
