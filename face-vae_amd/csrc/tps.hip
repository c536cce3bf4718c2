// The random equivariance transform (Transform, trainer.py:91-129 of Luh1124/face-vae; FOMM's
// affine + thin-plate-spline warp): the coordinate map and the frame warp built on it.
//
//   T(p) = theta[:, :2] p + theta[:, 2] + r(p) (1, 1),   r(p) = sum_q c_q d_q^2 log(d_q + 1e-6),
//   d_q = |x - qx| + |y - qy| over the pts x pts control lattice make_coordinate_grid_2d((pts, pts))
//   (utils.py:79-88; x fastest), summed in ascending q.
//
//   fv_tps_warp_frame_fwd    transform_frame (trainer.py:106-110): per output pixel the grid
//                            point, T of it, and F.grid_sample(bilinear, align_corners=True,
//                            padding_mode="reflection") in ATen's arithmetic.  One thread per
//                            output pixel, W fastest: the coordinate is computed once and shared
//                            by the C planes, whose stores are coalesced.  NCHW fp32 in and out.
//   fv_tps_warp_coords_fwd   warp_coordinates (trainer.py:112-129) of [N][M][2] points, one
//                            thread per point.
//   fv_tps_warp_coords_bwd   its gradient in the points (theta and the control parameters are
//                            random constants): g_p = theta[:, :2]^T g + (g_x + g_y) grad r,
//                            dr/dx = sum_q c_q (2 d log(d + 1e-6) + d^2 / (d + 1e-6)) sign(x - qx),
//                            sign(0) = 0 as torch's abs backward.
//
// A block works on one sample: theta [2][3], the pts^2 control parameters and the pts lattice
// coordinates are staged in LDS once per block (read from device memory at run time, so a
// captured step may refresh them in place).  |y - qy| takes pts values per point, not pts^2:
// it is formed once per lattice row.  fp32 throughout, the products and sums in the
// reference's order without contraction, logf; no atomics: reruns are bit-identical.
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
constexpr int TPS_MAXPTS = 16;                        // pts^2 <= 256 staged control parameters
constexpr int TPS_MAXQ = TPS_MAXPTS * TPS_MAXPTS;
constexpr float TPS_EPS = 1e-6f;

struct TpsLds {
  float c[TPS_MAXQ];      // control parameters of the block's sample
  float q[TPS_MAXPTS];    // lattice coordinates 2 * (i / (pts - 1)) - 1
  float th[6];
};

// all threads of the block; ends in a barrier
__device__ __forceinline__ void tps_stage(TpsLds& s, const float* __restrict__ theta, const float* __restrict__ cparams,
                                          int n, int pts) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x, P = pts * pts;
  for (int k = tid; k < P; k += NT) s.c[k] = cparams[(long)n * P + k];
  if (tid < pts) s.q[tid] = 2.f * ((float)tid / (float)(pts - 1)) - 1.f;
  if (tid < 6) s.th[tid] = theta[(long)n * 6 + tid];
  __syncthreads();
}

// r(p): ((d * d) * log(d + eps)) * c as trainer.py:123-125, summed over q ascending.  At d = 0 the
// term is 0 * log(1e-6) = -0: finite, and exactly zero.
__device__ __forceinline__ float tps_r(const TpsLds& s, int pts, float x, float y) {
#pragma clang fp contract(off)
  float r = 0.f;
  for (int i = 0; i < pts; ++i) {
    const float ay = fabsf(y - s.q[i]);
    const float* c = s.c + i * pts;
    for (int j = 0; j < pts; ++j) {
      const float d = fabsf(x - s.q[j]) + ay;
      r += ((d * d) * logf(d + TPS_EPS)) * c[j];
    }
  }
  return r;
}

__device__ __forceinline__ void tps_map(const TpsLds& s, int pts, float x, float y, float& ox, float& oy) {
#pragma clang fp contract(off)
  const float r = tps_r(s, pts, x, y);
  ox = ((s.th[0] * x + s.th[1] * y) + s.th[2]) + r;
  oy = ((s.th[3] * x + s.th[4] * y) + s.th[5]) + r;
}

__device__ __forceinline__ float tps_sign(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }

// grad r
__device__ __forceinline__ void tps_r_grad(const TpsLds& s, int pts, float x, float y, float& rx, float& ry) {
#pragma clang fp contract(off)
  rx = 0.f;
  ry = 0.f;
  for (int i = 0; i < pts; ++i) {
    const float dy = y - s.q[i];
    const float ay = fabsf(dy), sy = tps_sign(dy);
    const float* c = s.c + i * pts;
    for (int j = 0; j < pts; ++j) {
      const float dx = x - s.q[j];
      const float d = fabsf(dx) + ay;
      const float de = d + TPS_EPS;
      const float t = c[j] * ((2.f * d) * logf(de) + (d * d) / de);
      rx += t * tps_sign(dx);
      ry += t * sy;
    }
  }
}

// ATen's grid_sampler_compute_source_index(align_corners = true, padding = reflection):
// unnormalise, reflect about 0 and size - 1, clip.  The result lies in [0, size - 1] for every
// input, NaN included (fmaxf / fminf return the other operand).
__device__ __forceinline__ float tps_source_index(float g, int size) {
#pragma clang fp contract(off)
  float v = ((g + 1.f) / 2.f) * (float)(size - 1);
  const float span = (float)(size - 1);         // twice_low = 0, twice_high = 2 * (size - 1)
  if (span == 0.f) {
    v = 0.f;
  } else {
    v = fabsf(v);
    const float extra = fmodf(v, span);
    const int flips = (int)floorf(v / span);
    v = (flips % 2 == 0) ? extra : span - extra;
  }
  return fminf((float)(size - 1), fmaxf(v, 0.f));
}

__global__ void __launch_bounds__(NT) tps_warp_frame_kernel(const float* __restrict__ x, const float* __restrict__ theta,
                                                            const float* __restrict__ cparams, int C, int H, int W, int pts,
                                                            float* __restrict__ y) {
#pragma clang fp contract(off)
  __shared__ TpsLds s;
  const int n = blockIdx.y;
  tps_stage(s, theta, cparams, n, pts);
  const int HW = H * W;                          // < 2^31 (checked by the entry)
  const int pix = blockIdx.x * NT + threadIdx.x;
  if (pix >= HW) return;
  const int i = pix / W, j = pix - i * W;
  const float px = 2.f * ((float)j / (float)(W - 1)) - 1.f;
  const float py = 2.f * ((float)i / (float)(H - 1)) - 1.f;
  float gx, gy;
  tps_map(s, pts, px, py, gx, gy);
  const float ix = tps_source_index(gx, W), iy = tps_source_index(gy, H);
  const float fx = floorf(ix), fy = floorf(iy);
  const int x0 = (int)fx, y0 = (int)fy;          // in [0, W - 1] x [0, H - 1]
  const int x1 = x0 + 1, y1 = y0 + 1;
  const float ex = (fx + 1.f) - ix, ey = (fy + 1.f) - iy;      // ix_se - ix, iy_se - iy
  const float wx = ix - fx, wy = iy - fy;
  const float nw = ex * ey, ne = wx * ey, sw = ex * wy, se = wx * wy;
  const bool inx1 = x1 < W, iny1 = y1 < H;       // a corner outside the image contributes 0
  const long o00 = (long)y0 * W + x0;
  const float* xp = x + (long)n * C * HW;
  float* yp = y + (long)n * C * HW + pix;
  for (int c = 0; c < C; ++c, xp += HW, yp += HW) {
    float acc = xp[o00] * nw;
    if (inx1) acc += xp[o00 + 1] * ne;
    if (iny1) acc += xp[o00 + W] * sw;
    if (inx1 && iny1) acc += xp[o00 + W + 1] * se;
    *yp = acc;
  }
}

__global__ void __launch_bounds__(NT) tps_warp_coords_fwd_kernel(const float* __restrict__ coords,
                                                                 const float* __restrict__ theta,
                                                                 const float* __restrict__ cparams, int M, int pts,
                                                                 float* __restrict__ out) {
  __shared__ TpsLds s;
  const int n = blockIdx.y;
  tps_stage(s, theta, cparams, n, pts);
  const int m = blockIdx.x * NT + threadIdx.x;
  if (m >= M) return;
  const long e = ((long)n * M + m) * 2;
  float ox, oy;
  tps_map(s, pts, coords[e], coords[e + 1], ox, oy);
  out[e] = ox;
  out[e + 1] = oy;
}

__global__ void __launch_bounds__(NT) tps_warp_coords_bwd_kernel(const float* __restrict__ coords,
                                                                 const float* __restrict__ g_out,
                                                                 const float* __restrict__ theta,
                                                                 const float* __restrict__ cparams, int M, int pts,
                                                                 float* __restrict__ g_coords) {
#pragma clang fp contract(off)
  __shared__ TpsLds s;
  const int n = blockIdx.y;
  tps_stage(s, theta, cparams, n, pts);
  const int m = blockIdx.x * NT + threadIdx.x;
  if (m >= M) return;
  const long e = ((long)n * M + m) * 2;
  float rx, ry;
  tps_r_grad(s, pts, coords[e], coords[e + 1], rx, ry);
  const float gx = g_out[e], gy = g_out[e + 1];
  const float gs = gx + gy;
  g_coords[e] = (s.th[0] * gx + s.th[3] * gy) + gs * rx;
  g_coords[e + 1] = (s.th[1] * gx + s.th[4] * gy) + gs * ry;
}

int tps_check(const char* what, int n, int pts) {
  FV_SUPPORTED(pts >= 2 && pts <= TPS_MAXPTS,
               "%s: points_tps must be in [2, %d] (the lattice divides by pts - 1; pts^2 staged parameters; got %d)", what,
               TPS_MAXPTS, pts);
  FV_SUPPORTED(n >= 1 && n <= 65535, "%s: N must be in [1, 65535] (got %d)", what, n);
  return FV_OK;
}

int tps_coords_check(const char* what, int n, int m, int pts) {
  const int st = tps_check(what, n, pts);
  if (st) return st;
  FV_SUPPORTED(m >= 1 && m <= 0x7fffffff - NT, "%s: M must be in [1, 2^31 - %d) (got %d)", what, NT + 1, m);
  return FV_OK;
}

}  // namespace

extern "C" {

int fv_tps_warp_frame_fwd(const float* x, const float* theta, const float* cparams, int n, int c, int h, int w, int pts,
                          float* y, void* stream) {
  const int st = tps_check("tps_warp_frame_fwd", n, pts);
  if (st) return st;
  FV_SUPPORTED(h >= 2 && w >= 2, "tps_warp_frame_fwd: H and W must each be at least 2 (the grid divides by size - 1; got %d x %d)",
               h, w);
  FV_SUPPORTED(c >= 1, "tps_warp_frame_fwd: C must be at least 1 (got %d)", c);
  FV_SUPPORTED((long)h * w <= 0x7fffffffL - NT, "tps_warp_frame_fwd: H * W must be below 2^31 - %d", NT);
  FV_REQUIRE(x && theta && cparams && y, "tps_warp_frame_fwd: null pointer");
  const dim3 grid(fv_cdiv((long)h * w, NT), n);
  hipLaunchKernelGGL(tps_warp_frame_kernel, grid, dim3(NT), 0, (hipStream_t)stream, x, theta, cparams, c, h, w, pts, y);
  return fv_check_launch("tps_warp_frame_fwd");
}

int fv_tps_warp_coords_fwd(const float* coords, const float* theta, const float* cparams, int n, int m, int pts, float* out,
                           void* stream) {
  const int st = tps_coords_check("tps_warp_coords_fwd", n, m, pts);
  if (st) return st;
  FV_REQUIRE(coords && theta && cparams && out, "tps_warp_coords_fwd: null pointer");
  hipLaunchKernelGGL(tps_warp_coords_fwd_kernel, dim3(fv_cdiv(m, NT), n), dim3(NT), 0, (hipStream_t)stream, coords, theta,
                     cparams, m, pts, out);
  return fv_check_launch("tps_warp_coords_fwd");
}

int fv_tps_warp_coords_bwd(const float* coords, const float* g_out, const float* theta, const float* cparams, int n, int m,
                           int pts, float* g_coords, void* stream) {
  const int st = tps_coords_check("tps_warp_coords_bwd", n, m, pts);
  if (st) return st;
  FV_REQUIRE(coords && g_out && theta && cparams && g_coords, "tps_warp_coords_bwd: null pointer");
  hipLaunchKernelGGL(tps_warp_coords_bwd_kernel, dim3(fv_cdiv(m, NT), n), dim3(NT), 0, (hipStream_t)stream, coords, g_out,
                     theta, cparams, m, pts, g_coords);
  return fv_check_launch("tps_warp_coords_bwd");
}

}  // extern "C"
