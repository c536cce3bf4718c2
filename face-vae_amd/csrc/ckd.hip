// Canonical keypoint detector pieces (CKD, models.py:948-987 of Luh1124/face-vae; out2heatmap /
// heatmap2kp utils.py:106-118): the head and the tail around the existing conv / BN kernels.
//
//   fv_ckd_resize_fwd       F.interpolate(bilinear, align_corners=False, recompute_scale_factor=True)
//                           of the NCHW fp32 image, written as the first conv's input: dense NHWC
//                           in the storage dtype with the 3 channels zero-padded to 8.  One thread
//                           per output pixel, one 16 / 32 byte store each.
//   fv_ckd_softargmax_fwd   kp = sum_v softmax_v(z / T) g(v) over the D*H*W voxels of the NDHWC
//                           logits [N][V][K], the heatmap never written.  Launch 1: per (sample,
//                           voxel chunk) one block walks the chunk's contiguous V*K elements with
//                           TA = (256 / K) * K active threads, so thread t always meets keypoint
//                           t % K and consecutive threads read consecutive elements, whatever the
//                           alignment of the K-element rows.  Every thread keeps an online-softmax
//                           partial (m, s, s*x, s*y, s*z; the sums in fp64) over batches of 8
//                           loads in flight; the threads of a keypoint are merged through LDS in
//                           thread order.  Launch
//                           2: one wave per (sample, keypoint) merges the chunks: lane l takes
//                           chunks l, l + 64, ... in ascending order, then a fixed xor tree.
//   fv_ckd_softargmax_bwd   dz = (1 / T) p sum_j G_j (g_j(v) - kp_j), p recomputed from the saved
//                           (max, sum); one elementwise pass in the logits' layout.
//
// The maximum is tracked on z, not on z / T, and the exponent is (z - max z) / T: the difference is
// exact (or rounded relative to its own size), so an offset common to all logits costs no accuracy.
// expf, fp32 coordinates and products, fp64 running sums; no float atomics: reruns are bit-identical.
#include <float.h>

#include "common.h"

namespace {

#define FV_SUPPORTED(cond, ...)                \
  do {                                         \
    if (!(cond)) {                             \
      fv_set_error(__VA_ARGS__);               \
      return FV_E_UNSUPPORTED;                 \
    }                                          \
  } while (0)

constexpr int NT = 256;
constexpr int SAM_U = 8;            // loads in flight per thread
constexpr int SAM_MAXCHUNK = 512;   // voxel chunks per sample at most
constexpr int SAM_BWD_U = 4;

// ------------------------------------------------------------------------------------
// bilinear resize
// ------------------------------------------------------------------------------------
struct Tap {
  int i0, i1;
  float l0, l1;
};
// ATen's area_pixel_compute_source_index (align_corners = false) + guard_index_and_lambda
__device__ __forceinline__ Tap resize_tap(float scale, int o, int in) {
#pragma clang fp contract(off)
  float src = scale * ((float)o + 0.5f) - 0.5f;
  src = src < 0.f ? 0.f : src;
  Tap t;
  t.i0 = min((int)src, in - 1);
  t.i1 = min(t.i0 + 1, in - 1);
  t.l1 = fminf(fmaxf(src - (float)t.i0, 0.f), 1.f);
  t.l0 = 1.f - t.l1;
  return t;
}

template <typename T>
__global__ void __launch_bounds__(NT) ckd_resize_kernel(const float* __restrict__ x, int H, int W, int Ho, int Wo,
                                                        float sh, float sw, T* __restrict__ y, long total) {
#pragma clang fp contract(off)
  const long idx = (long)blockIdx.x * NT + threadIdx.x;
  if (idx >= total) return;
  const int ox = (int)(idx % Wo);
  const long t = idx / Wo;
  const int oy = (int)(t % Ho);
  const long n = t / Ho;
  const Tap ty = resize_tap(sh, oy, H), tx = resize_tap(sw, ox, W);
  float f[8];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float* p = x + (n * 3 + c) * (long)H * W;
    const float a = p[(long)ty.i0 * W + tx.i0], b = p[(long)ty.i0 * W + tx.i1];
    const float cc = p[(long)ty.i1 * W + tx.i0], d = p[(long)ty.i1 * W + tx.i1];
    f[c] = ty.l0 * (tx.l0 * a + tx.l1 * b) + ty.l1 * (tx.l0 * cc + tx.l1 * d);
  }
#pragma unroll
  for (int c = 3; c < 8; ++c) f[c] = 0.f;
  Chunk8<T> o;
  o.set8(f);
  o.store(y + idx * 8);
}

// ------------------------------------------------------------------------------------
// soft-argmax
// ------------------------------------------------------------------------------------
struct SamGeo {
  int V, K, D, H, W;
  int vps;      // voxels per block step = NT / K
  int cvox;     // voxels per chunk (a multiple of vps * SAM_U)
  int nchunk;
  float invT;
  FastDiv dW, dH;
};

// make_coordinate_grid_3d (utils.py:91-103): 2 * (i / (n - 1)) - 1, x along W first
__device__ __forceinline__ void sam_coords(const SamGeo& g, int v, float& gx, float& gy, float& gz) {
#pragma clang fp contract(off)
  const uint32_t r = fdiv((uint32_t)v, g.dW);
  const int w = v - (int)r * g.W;
  const uint32_t d = fdiv(r, g.dH);
  const int h = (int)r - (int)d * g.H;
  gx = 2.f * ((float)w / (float)(g.W - 1)) - 1.f;
  gy = 2.f * ((float)h / (float)(g.H - 1)) - 1.f;
  gz = 2.f * ((float)(int)d / (float)(g.D - 1)) - 1.f;
}

// part [N][nchunk][K][5] fp64 = (max z, sum e, sum e x, sum e y, sum e z), e = exp((z - max z) / T).
// The exponentials and coordinates are fp32; the four sums are carried in fp64: with a peaked
// heatmap kp sits within 1e-3 of the peak's coordinate, and the backward's (grid - kp) would
// otherwise lose the digits an fp32 sum drops beside the peak's e = 1.
template <typename T>
__global__ void __launch_bounds__(NT) ckd_sam_part_kernel(const T* __restrict__ z, SamGeo g, double* __restrict__ part) {
  const int tid = threadIdx.x;
  const int K = g.K, vps = g.vps;
  const int sub = tid / K, k = tid - sub * K;
  const bool active = sub < vps;
  const int chunk = blockIdx.x, n = blockIdx.y;
  const int v0 = chunk * g.cvox, vend = min(g.V, v0 + g.cvox);
  const T* zn = z + (long)n * g.V * K;
  float m = -FLT_MAX;
  double s = 0., sx = 0., sy = 0., sz = 0.;
  for (int base = v0; base < vend; base += vps * SAM_U) {
    float x[SAM_U];
    bool ok[SAM_U];
#pragma unroll
    for (int u = 0; u < SAM_U; ++u) {
      const int v = base + u * vps + sub;
      ok[u] = active && v < vend;
      x[u] = ok[u] ? Elt<T>::to_f(zn[(long)v * K + k]) : -FLT_MAX;
    }
    float mn = m;
#pragma unroll
    for (int u = 0; u < SAM_U; ++u) mn = fmaxf(mn, x[u]);
    const double sc = (double)expf((m - mn) * g.invT);     // 1 when the maximum stands, 0 from the initial -FLT_MAX
    s *= sc; sx *= sc; sy *= sc; sz *= sc;
    m = mn;
#pragma unroll
    for (int u = 0; u < SAM_U; ++u) {
      const int v = ok[u] ? base + u * vps + sub : v0;
      float gx, gy, gz;
      sam_coords(g, v, gx, gy, gz);
      const double e = ok[u] ? (double)expf((x[u] - m) * g.invT) : 0.;
      s += e; sx += e * (double)gx; sy += e * (double)gy; sz += e * (double)gz;
    }
  }
  __shared__ float redm[NT];
  __shared__ double red[NT * 4];
  redm[tid] = m;
  red[tid * 4 + 0] = s; red[tid * 4 + 1] = sx; red[tid * 4 + 2] = sy; red[tid * 4 + 3] = sz;
  __syncthreads();
  if (tid < K) {
    float M = -FLT_MAX;
    for (int j = 0; j < vps; ++j) M = fmaxf(M, redm[j * K + tid]);
    double a = 0., ax = 0., ay = 0., az = 0.;
    for (int j = 0; j < vps; ++j) {
      const double* r = red + (j * K + tid) * 4;
      const double sc = (double)expf((redm[j * K + tid] - M) * g.invT);
      a += r[0] * sc; ax += r[1] * sc; ay += r[2] * sc; az += r[3] * sc;
    }
    double* o = part + (((long)n * g.nchunk + chunk) * K + tid) * 5;
    o[0] = (double)M; o[1] = a; o[2] = ax; o[3] = ay; o[4] = az;
  }
}

// one wave per (n, k): kp [N][K][3]; stat [N][K][8] = (max z, sum e, kp as fp32 pairs hi[3], lo[3]:
// hi = kp, hi + lo = the fp64 quotient to 2^-48)
__global__ void __launch_bounds__(NT) ckd_sam_merge_kernel(const double* __restrict__ part, int NK, int K, int nchunk,
                                                           float invT, float* __restrict__ kp, float* __restrict__ stat) {
  const int lane = threadIdx.x & 63;
  const int nk = blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
  if (nk >= NK) return;                      // uniform over the wave
  const int n = nk / K, k = nk - n * K;
  const double* p = part + ((long)n * nchunk * K + k) * 5;
  const long stride = (long)K * 5;
  float M = -FLT_MAX;
  for (int c = lane; c < nchunk; c += 64) M = fmaxf(M, (float)p[c * stride]);
  M = wave_max(M);
  double a = 0., ax = 0., ay = 0., az = 0.;
  for (int c = lane; c < nchunk; c += 64) {
    const double* r = p + c * stride;
    const double sc = (double)expf(((float)r[0] - M) * invT);
    a += r[1] * sc; ax += r[2] * sc; ay += r[3] * sc; az += r[4] * sc;
  }
  a = wave_sum_d(a); ax = wave_sum_d(ax); ay = wave_sum_d(ay); az = wave_sum_d(az);
  if (lane == 0) {
    const double q[3] = {ax / a, ay / a, az / a};
    float* st = stat + (long)nk * 8;
    st[0] = M;
    st[1] = (float)a;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const float hi = (float)q[j];
      kp[nk * 3 + j] = hi;
      st[2 + j] = hi;
      st[5 + j] = (float)(q[j] - (double)hi);
    }
  }
}

// cst (LDS) [K][8] = (max z, 1 / sum, G.x, G.y, G.z) and, as fp64 [K][3] behind them, kp
template <typename T>
__global__ void __launch_bounds__(NT) ckd_sam_bwd_kernel(const T* __restrict__ z, SamGeo g, const float* __restrict__ G,
                                                         const float* __restrict__ stat, T* __restrict__ dz) {
  extern __shared__ double cst64[];
  const int tid = threadIdx.x, n = blockIdx.y, K = g.K;
  double* ckp = cst64;                                  // [K][3]
  float* cst = reinterpret_cast<float*>(cst64 + 3 * K);  // [K][5]
  for (int k = tid; k < K; k += NT) {
    const long nk = (long)n * K + k;
    const float* st = stat + nk * 8;
    cst[k * 5 + 0] = st[0];
    cst[k * 5 + 1] = 1.f / st[1];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      cst[k * 5 + 2 + j] = G[nk * 3 + j];
      ckp[k * 3 + j] = (double)st[2 + j] + (double)st[5 + j];
    }
  }
  __syncthreads();
  const long VK = (long)g.V * K;
  const T* zn = z + n * VK;
  T* dn = dz + n * VK;
  const long e0 = (long)blockIdx.x * (NT * SAM_BWD_U) + tid;
  float x[SAM_BWD_U];
#pragma unroll
  for (int u = 0; u < SAM_BWD_U; ++u) {
    const long e = e0 + u * NT;
    x[u] = e < VK ? Elt<T>::to_f(zn[e]) : 0.f;
  }
#pragma unroll
  for (int u = 0; u < SAM_BWD_U; ++u) {
    const long e = e0 + u * NT;
    if (e >= VK) continue;
    const int v = (int)((uint32_t)e / (uint32_t)K), k = (int)(e - (long)v * K);   // V * K < 2^31
    const float* c = cst + k * 5;
    const double* q = ckp + k * 3;
    float gx, gy, gz;
    sam_coords(g, v, gx, gy, gz);
    const float p = expf((x[u] - c[0]) * g.invT) * c[1];
    // (grid - kp) in fp64: the two nearly cancel at a peaked heatmap's dominant voxel
    const float t = (float)((double)c[2] * ((double)gx - q[0]) + (double)c[3] * ((double)gy - q[1]) +
                            (double)c[4] * ((double)gz - q[2]));
    dn[e] = Elt<T>::from_f(p * t * g.invT);
  }
}

int sam_geo(const char* what, int dtype, int n, int k, int d, int h, int w, float temperature, SamGeo& g) {
  FV_SUPPORTED(dtype == FV_F32 || dtype == FV_BF16, "%s: dtype must be FV_F32 or FV_BF16", what);
  FV_SUPPORTED(d >= 2 && h >= 2 && w >= 2,
               "%s: D, H and W must each be at least 2 (the coordinate grid divides by size - 1; got %d x %d x %d)", what,
               d, h, w);
  FV_SUPPORTED(k >= 1 && k <= NT,
               "%s: K must be in [1, %d] (one thread per keypoint of a voxel row; no per-thread array over K; got %d)",
               what, NT, k);
  FV_SUPPORTED(n >= 1 && n <= 65535, "%s: N must be in [1, 65535] (got %d)", what, n);
  const long V = (long)d * h * w;
  FV_SUPPORTED(V * k < (1L << 31), "%s: D * H * W * K must be below 2^31", what);
  FV_SUPPORTED(temperature > 0.f && temperature <= FLT_MAX, "%s: the temperature must be positive and finite", what);
  g.V = (int)V; g.K = k; g.D = d; g.H = h; g.W = w;
  g.vps = NT / k;
  const int step = g.vps * SAM_U;
  g.cvox = step * fv_cdiv(fv_cdiv(V, step), SAM_MAXCHUNK);
  g.nchunk = fv_cdiv(V, g.cvox);
  g.invT = (float)(1.0 / (double)temperature);
  g.dW = make_fastdiv((uint32_t)w);
  g.dH = make_fastdiv((uint32_t)h);
  return FV_OK;
}

}  // namespace

extern "C" {

int fv_ckd_resize_fwd(int dtype, const float* x, int n, int h, int w, int ho, int wo, void* y, void* stream) {
  FV_SUPPORTED(dtype == FV_F32 || dtype == FV_BF16, "ckd_resize_fwd: dtype must be FV_F32 or FV_BF16");
  FV_SUPPORTED(n > 0 && h > 0 && w > 0 && ho > 0 && wo > 0, "ckd_resize_fwd: sizes must be positive (%d x %d -> %d x %d)",
               h, w, ho, wo);
  FV_SUPPORTED((long)n * 3 * h * w < (1L << 40) && (long)n * ho * wo < (long)NT * 0x7fffffffL,
               "ckd_resize_fwd: tensor too large");
  FV_REQUIRE(x && y, "ckd_resize_fwd: null pointer");
  const long total = (long)n * ho * wo;
  const float sh = (float)h / (float)ho, sw = (float)w / (float)wo;
  const dim3 grid(fv_cdiv(total, NT));
  hipStream_t s = (hipStream_t)stream;
  if (dtype == FV_BF16)
    hipLaunchKernelGGL(ckd_resize_kernel<bf16>, grid, dim3(NT), 0, s, x, h, w, ho, wo, sh, sw, (bf16*)y, total);
  else
    hipLaunchKernelGGL(ckd_resize_kernel<float>, grid, dim3(NT), 0, s, x, h, w, ho, wo, sh, sw, (float*)y, total);
  return fv_check_launch("ckd_resize_fwd");
}

size_t fv_ckd_softargmax_ws_bytes(int n, int k, int d, int h, int w) {
  SamGeo g{};
  if (sam_geo("ckd_softargmax_ws_bytes", FV_F32, n, k, d, h, w, 1.f, g)) return 0;
  return (size_t)n * g.nchunk * k * 5 * sizeof(double);
}

int fv_ckd_softargmax_fwd(int dtype, const void* z, int n, int k, int d, int h, int w, float temperature, float* kp,
                          float* stat, void* ws, void* stream) {
  SamGeo g{};
  int st = sam_geo("ckd_softargmax_fwd", dtype, n, k, d, h, w, temperature, g);
  if (st) return st;
  FV_REQUIRE(z && kp && stat && ws, "ckd_softargmax_fwd: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(g.nchunk, n);
  if (dtype == FV_BF16) hipLaunchKernelGGL(ckd_sam_part_kernel<bf16>, grid, dim3(NT), 0, s, (const bf16*)z, g, (double*)ws);
  else hipLaunchKernelGGL(ckd_sam_part_kernel<float>, grid, dim3(NT), 0, s, (const float*)z, g, (double*)ws);
  if ((st = fv_check_launch("ckd_softargmax_part"))) return st;
  hipLaunchKernelGGL(ckd_sam_merge_kernel, dim3(fv_cdiv((long)n * k, NT / 64)), dim3(NT), 0, s, (const double*)ws, n * k, k,
                     g.nchunk, g.invT, kp, stat);
  return fv_check_launch("ckd_softargmax_merge");
}

int fv_ckd_softargmax_bwd(int dtype, const void* z, const float* g_kp, const float* stat, int n, int k, int d, int h,
                          int w, float temperature, void* dz, void* stream) {
  SamGeo g{};
  int st = sam_geo("ckd_softargmax_bwd", dtype, n, k, d, h, w, temperature, g);
  if (st) return st;
  FV_REQUIRE(z && g_kp && stat && dz, "ckd_softargmax_bwd: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(fv_cdiv((long)g.V * k, NT * SAM_BWD_U), n);
  const size_t lds = (size_t)k * (3 * sizeof(double) + 5 * sizeof(float));
  if (dtype == FV_BF16)
    hipLaunchKernelGGL(ckd_sam_bwd_kernel<bf16>, grid, dim3(NT), lds, s, (const bf16*)z, g, g_kp, stat, (bf16*)dz);
  else
    hipLaunchKernelGGL(ckd_sam_bwd_kernel<float>, grid, dim3(NT), lds, s, (const float*)z, g, g_kp, stat, (float*)dz);
  return fv_check_launch("ckd_softargmax_bwd");
}

}  // extern "C"
