// Expression feature extractor pieces (EFE_conv5, models.py:724-799 of Luh1124/face-vae): the
// concatenation of out_conv's logits with the Gaussian heatmaps of the posed keypoints,
// torch.cat((x, kp2gaussian_3d(kpc, x.shape[2:])), 1) (models.py:790-791, utils.py:130-136), between
// the existing 3-D conv kernels.
//
//   fv_efe_kpcat_fwd   out [N][V][Cp], Cp = the 2K channels padded to 8 * 2^k: channels [0, K) the
//                      logits z [N][V][K] bit for bit, [K, 2K) exp(-0.5 |grid(v) - kp|^2 / var)
//                      computed in fp32 and rounded once, [2K, Cp) zero.  One lane per 8-channel
//                      piece of a row (one 16 / 32 byte store); the K-element rows of z are read
//                      element by element, whatever their alignment.  No heatmap tensor is written.
//   fv_efe_kpcat_bwd   dz [N][V][K] = channels [0, K) of g, and
//                      dkpc[n][k][j] = sum_v g[n][v][K + k] G (grid_j(v) - kp_j) / var with G
//                      recomputed in fp32 from kpc.  Launch 1: per (sample, voxel chunk) one block
//                      walks the chunk with TA = (256 / K) * K active threads, thread t always
//                      meeting keypoint t % K (consecutive threads read consecutive elements of a
//                      row); every thread keeps three fp64 sums, merged per keypoint through LDS
//                      in thread order.  Launch 2: one wave per (sample, keypoint) merges the
//                      chunks: lane l takes chunks l, l + 64, ... in ascending order, then a fixed
//                      xor tree.  No float atomics: reruns are bit-identical.
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
constexpr int KPC_U = 4;            // voxel rows in flight per thread in the backward
constexpr int KPC_MAXCHUNK = 512;   // voxel chunks per sample at most

struct KpcGeo {
  int V, K, Cp, D, H, W;
  int cshift;   // log2(Cp / 8): 8-channel pieces per row
  int vps;      // voxels per block step of the backward = NT / K
  int cvox;     // voxels per chunk (a multiple of vps * KPC_U)
  int nchunk;
  float var;
  FastDiv dW, dH;
};

// make_coordinate_grid_3d (utils.py:91-103): 2 * (i / (n - 1)) - 1, x along W first
__device__ __forceinline__ void kpc_coords(const KpcGeo& g, int v, float& gx, float& gy, float& gz) {
#pragma clang fp contract(off)
  const uint32_t r = fdiv((uint32_t)v, g.dW);
  const int w = v - (int)r * g.W;
  const uint32_t d = fdiv(r, g.dH);
  const int h = (int)r - (int)d * g.H;
  gx = 2.f * ((float)w / (float)(g.W - 1)) - 1.f;
  gy = 2.f * ((float)h / (float)(g.H - 1)) - 1.f;
  gz = 2.f * ((float)(int)d / (float)(g.D - 1)) - 1.f;
}

// kp2gaussian_3d (utils.py:134-135): exp(-0.5 * sum((grid - kp)^2) / var), fp32 in the reference's order
__device__ __forceinline__ float kpc_gauss(float dx, float dy, float dz, float var) {
#pragma clang fp contract(off)
  const float s = dx * dx + dy * dy + dz * dz;
  return expf(-0.5f * s / var);
}

template <typename T>
__global__ void __launch_bounds__(NT) efe_kpcat_fwd_kernel(const T* __restrict__ z, const float* __restrict__ kpc,
                                                           KpcGeo g, T* __restrict__ out) {
  extern __shared__ float skp[];               // [K][3]
  const int tid = threadIdx.x, n = blockIdx.y, K = g.K;
  for (int i = tid; i < K * 3; i += NT) skp[i] = kpc[(long)n * K * 3 + i];
  __syncthreads();
  const long piece = (long)blockIdx.x * NT + tid;
  const long v = piece >> g.cshift;
  if (v >= g.V) return;
  const int c0 = (int)(piece - (v << g.cshift)) * 8;
  const T* zr = z + ((long)n * g.V + v) * K;
  float gx = 0.f, gy = 0.f, gz = 0.f;
  if (c0 + 8 > K && c0 < 2 * K) kpc_coords(g, (int)v, gx, gy, gz);
  alignas(32) T t[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = c0 + j;
    if (c < K) {
      t[j] = zr[c];
    } else if (c < 2 * K) {
      const float* q = skp + (c - K) * 3;
      t[j] = Elt<T>::from_f(kpc_gauss(gx - q[0], gy - q[1], gz - q[2], g.var));
    } else {
      t[j] = Elt<T>::from_f(0.f);
    }
  }
  Chunk8<T> o;
  o.load(t);
  o.store(out + ((long)n * g.V + v) * g.Cp + c0);
}

// part [N][nchunk][K][3] fp64
template <typename T>
__global__ void __launch_bounds__(NT) efe_kpcat_bwd_kernel(const T* __restrict__ gout, const float* __restrict__ kpc,
                                                           KpcGeo g, T* __restrict__ dz, double* __restrict__ part) {
  const int tid = threadIdx.x;
  const int K = g.K, vps = g.vps;
  const int sub = tid / K, k = tid - sub * K;
  const bool active = sub < vps;
  const int chunk = blockIdx.x, n = blockIdx.y;
  const int v0 = chunk * g.cvox, vend = min(g.V, v0 + g.cvox);
  const T* gn = gout + (long)n * g.V * g.Cp;
  T* dn = dz + (long)n * g.V * K;
  const float* q = kpc + ((long)n * K + k) * 3;
  const float kx = q[0], ky = q[1], kz = q[2];
  const float ivar = 1.f / g.var;
  double sx = 0., sy = 0., sz = 0.;
  for (int base = v0; base < vend; base += vps * KPC_U) {
    T a[KPC_U], b[KPC_U];
    bool ok[KPC_U];
#pragma unroll
    for (int u = 0; u < KPC_U; ++u) {
      const int v = base + u * vps + sub;
      ok[u] = active && v < vend;
      const long e = (long)(ok[u] ? v : v0) * g.Cp + k;
      a[u] = gn[e];
      b[u] = gn[e + K];
    }
#pragma unroll
    for (int u = 0; u < KPC_U; ++u) {
      if (!ok[u]) continue;
      const int v = base + u * vps + sub;
      dn[(long)v * K + k] = a[u];
      float gx, gy, gz;
      kpc_coords(g, v, gx, gy, gz);
      const float dx = gx - kx, dy = gy - ky, dzz = gz - kz;
      const float t = Elt<T>::to_f(b[u]) * kpc_gauss(dx, dy, dzz, g.var) * ivar;
      sx += (double)(t * dx); sy += (double)(t * dy); sz += (double)(t * dzz);
    }
  }
  __shared__ double red[NT * 3];
  red[tid * 3 + 0] = sx; red[tid * 3 + 1] = sy; red[tid * 3 + 2] = sz;
  __syncthreads();
  if (tid < K) {
    double ax = 0., ay = 0., az = 0.;
    for (int j = 0; j < vps; ++j) {
      const double* r = red + (j * K + tid) * 3;
      ax += r[0]; ay += r[1]; az += r[2];
    }
    double* o = part + (((long)n * g.nchunk + chunk) * K + tid) * 3;
    o[0] = ax; o[1] = ay; o[2] = az;
  }
}

// one wave per (n, k): dkpc [N][K][3]
__global__ void __launch_bounds__(NT) efe_kpcat_merge_kernel(const double* __restrict__ part, int NK, int K, int nchunk,
                                                             float* __restrict__ dkpc) {
  const int lane = threadIdx.x & 63;
  const int nk = blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
  if (nk >= NK) return;                      // uniform over the wave
  const int n = nk / K, k = nk - n * K;
  const double* p = part + ((long)n * nchunk * K + k) * 3;
  const long stride = (long)K * 3;
  double ax = 0., ay = 0., az = 0.;
  for (int c = lane; c < nchunk; c += 64) {
    const double* r = p + c * stride;
    ax += r[0]; ay += r[1]; az += r[2];
  }
  ax = wave_sum_d(ax); ay = wave_sum_d(ay); az = wave_sum_d(az);
  if (lane == 0) {
    dkpc[(long)nk * 3 + 0] = (float)ax;
    dkpc[(long)nk * 3 + 1] = (float)ay;
    dkpc[(long)nk * 3 + 2] = (float)az;
  }
}

int efe_pad_pow2(int c) {
  int p = 8;
  while (p < c) p *= 2;
  return p;
}

int kpc_geo(const char* what, int dtype, int n, int k, int cp, int d, int h, int w, float var, KpcGeo& g) {
  FV_SUPPORTED(dtype == FV_F32 || dtype == FV_BF16, "%s: dtype must be FV_F32 or FV_BF16", what);
  FV_SUPPORTED(d >= 2 && h >= 2 && w >= 2,
               "%s: D, H and W must each be at least 2 (the coordinate grid divides by size - 1; got %d x %d x %d)", what,
               d, h, w);
  FV_SUPPORTED(k >= 1 && k <= NT,
               "%s: K must be in [1, %d] (one thread per keypoint of a voxel row; got %d)", what, NT, k);
  FV_SUPPORTED(cp == efe_pad_pow2(2 * k),
               "%s: Cp must be the 2K channels padded to 8 * a power of two (%d for K = %d; got %d)", what,
               efe_pad_pow2(2 * k), k, cp);
  FV_SUPPORTED(n >= 1 && n <= 65535, "%s: N must be in [1, 65535] (got %d)", what, n);
  const long V = (long)d * h * w;
  FV_SUPPORTED(V * cp < (1L << 31), "%s: D * H * W * Cp must be below 2^31", what);
  FV_SUPPORTED(var > 0.f && var <= 3.0e38f, "%s: kp_variance must be positive and finite", what);
  g.V = (int)V; g.K = k; g.Cp = cp; g.D = d; g.H = h; g.W = w;
  g.cshift = fv_ilog2(cp / 8);
  g.vps = NT / k;
  const int step = g.vps * KPC_U;
  g.cvox = step * fv_cdiv(fv_cdiv(V, step), KPC_MAXCHUNK);
  g.nchunk = fv_cdiv(V, g.cvox);
  g.var = var;
  g.dW = make_fastdiv((uint32_t)w);
  g.dH = make_fastdiv((uint32_t)h);
  return FV_OK;
}

}  // namespace

extern "C" {

int fv_efe_kpcat_fwd(int dtype, const void* z, const float* kpc, int n, int k, int cp, int d, int h, int w,
                     float kp_variance, void* out, void* stream) {
  KpcGeo g{};
  int st = kpc_geo("efe_kpcat_fwd", dtype, n, k, cp, d, h, w, kp_variance, g);
  if (st) return st;
  FV_REQUIRE(z && kpc && out, "efe_kpcat_fwd: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(fv_cdiv((long)g.V << g.cshift, NT), n);
  const size_t lds = (size_t)k * 3 * sizeof(float);
  if (dtype == FV_BF16)
    hipLaunchKernelGGL(efe_kpcat_fwd_kernel<bf16>, grid, dim3(NT), lds, s, (const bf16*)z, kpc, g, (bf16*)out);
  else
    hipLaunchKernelGGL(efe_kpcat_fwd_kernel<float>, grid, dim3(NT), lds, s, (const float*)z, kpc, g, (float*)out);
  return fv_check_launch("efe_kpcat_fwd");
}

size_t fv_efe_kpcat_ws_bytes(int n, int k, int cp, int d, int h, int w) {
  KpcGeo g{};
  if (kpc_geo("efe_kpcat_ws_bytes", FV_F32, n, k, cp, d, h, w, 1.f, g)) return 0;
  return (size_t)n * g.nchunk * k * 3 * sizeof(double);
}

int fv_efe_kpcat_bwd(int dtype, const void* g_out, const float* kpc, int n, int k, int cp, int d, int h, int w,
                     float kp_variance, void* dz, float* dkpc, void* ws, void* stream) {
  KpcGeo g{};
  int st = kpc_geo("efe_kpcat_bwd", dtype, n, k, cp, d, h, w, kp_variance, g);
  if (st) return st;
  FV_REQUIRE(g_out && kpc && dz && dkpc && ws, "efe_kpcat_bwd: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(g.nchunk, n);
  if (dtype == FV_BF16)
    hipLaunchKernelGGL(efe_kpcat_bwd_kernel<bf16>, grid, dim3(NT), 0, s, (const bf16*)g_out, kpc, g, (bf16*)dz,
                       (double*)ws);
  else
    hipLaunchKernelGGL(efe_kpcat_bwd_kernel<float>, grid, dim3(NT), 0, s, (const float*)g_out, kpc, g, (float*)dz,
                       (double*)ws);
  if ((st = fv_check_launch("efe_kpcat_bwd"))) return st;
  hipLaunchKernelGGL(efe_kpcat_merge_kernel, dim3(fv_cdiv((long)n * k, NT / 64)), dim3(NT), 0, s, (const double*)ws,
                     n * k, k, g.nchunk, dkpc);
  return fv_check_launch("efe_kpcat_merge");
}

}  // extern "C"
