// Inference-only motion kernels of the Animator (animate.py) for gfx950: the MFE's hourglass input,
// the mask blend + warp of the appearance volume, and the uint8 frame output.  No backward, nothing
// saved.  Conventions of warp.hip: channels-last rows, lanes along channels, fp32 coordinate
// arithmetic; ident() / src_index() / gauss() and the corner loop are the expressions used there,
// so the results compare against the unfused path term by term.  HBM / gather bound (no MFMA).
//
// Reference behaviour replaced (file:line in Luh1124/face-vae):
//   MFE.forward up to the hourglass input   models.py:1066-1071 (utils.py:130-179)
//   mask softmax, deformation sum           models.py:1076-1078
//   F.grid_sample(fs, deformation)          models.py:1103
//   cat(dim=3), clip(0, 1), (255 * a).astype(uint8)   evaluate.py:39-44
//   img_as_float32 of the uint8 frames       dataset.py (skimage): x * fp32(1 / 255)
//   transform_kp, transform_kp_with_new_pose, Rs inv(Rd)   utils.py:53-76, 146
#include "common.h"

namespace {

__device__ __forceinline__ float ld(const float* p) { return *p; }
__device__ __forceinline__ float ld(const bf16* p) { return (float)*p; }

// align_corners=True source index: ((g + 1) / 2) * (size - 1)
__device__ __forceinline__ float src_index(float g, int size) { return (g + 1.f) * 0.5f * (float)(size - 1); }

// make_coordinate_grid_3d (utils.py:91-103): (x over W, y over H, z over D) in [-1, 1].  warp.hip's
// ident() with the voxel index split by multiply-shift divisions (the host requires < 2^31 lanes, where
// FastDiv is exact) instead of three 64-bit divisions per lane
struct VoxDiv {
  FastDiv w, h;
};
__device__ __forceinline__ void ident(unsigned v, VoxDiv vd, int D, int H, int W, float& gx, float& gy, float& gz) {
  const unsigned t = fdiv(v, vd.w), d = fdiv(t, vd.h);
  const int w = (int)(v - t * W), h = (int)(t - d * H);
  gx = 2.f * ((float)w / (float)(W - 1)) - 1.f;
  gy = 2.f * ((float)h / (float)(H - 1)) - 1.f;
  gz = 2.f * ((float)(int)d / (float)(D - 1)) - 1.f;
}

__device__ __forceinline__ float gauss(float gx, float gy, float gz, const float* kp, float var) {
  const float a = gx - kp[0], b = gy - kp[1], c = gz - kp[2];
  return expf(-0.5f * (a * a + b * b + c * c) / var);
}

// create_sparse_motions (utils.py:139-152) at one voxel: J (id - kp_d) + kp_s
__device__ __forceinline__ void motion(float gx, float gy, float gz, const float* ks, const float* kd, const float* j,
                                       float& m0, float& m1, float& m2) {
  const float c0 = gx - kd[0], c1 = gy - kd[1], c2 = gz - kd[2];
  m0 = j[0] * c0 + j[1] * c1 + j[2] * c2 + ks[0];
  m1 = j[3] * c0 + j[4] * c1 + j[5] * c2 + ks[1];
  m2 = j[6] * c0 + j[7] * c1 + j[8] * c2 + ks[2];
}

// trilinear cell of a grid point: base corner and fractions
struct Cell {
  int x0, y0, z0;
  float tx, ty, tz;
};
__device__ __forceinline__ Cell cell_of(float gx, float gy, float gz, int D, int H, int W) {
  const float ix = src_index(gx, W), iy = src_index(gy, H), iz = src_index(gz, D);
  const float fx = floorf(ix), fy = floorf(iy), fz = floorf(iz);
  Cell c;
  c.x0 = (int)fx, c.y0 = (int)fy, c.z0 = (int)fz;
  c.tx = ix - fx, c.ty = iy - fy, c.tz = iz - fz;
  return c;
}

// ---- fv_mfe_input_fwd ------------------------------------------------------------------------
// One lane per (voxel, motion k): its C2 + 1 output channels [heat_k, fc sampled at motion k] are
// the contiguous elements [gid * (C2 + 1), (gid + 1) * (C2 + 1)) of the output, so a block's 256
// lanes own one contiguous span.  It is assembled in LDS and leaves as 16-byte stores.
constexpr int MI_MAXCH = 16;   // C2 + 1 at most

// one NDHWC row of 4 channels as a single 8-byte (bf16) / 16-byte (fp32) load
template <typename T> struct Row4;
template <> struct Row4<float> {
  float4 r;
  __device__ __forceinline__ void load(const float* p) { r = *reinterpret_cast<const float4*>(p); }
  __device__ __forceinline__ float get(int j) const { return (&r.x)[j]; }
};
template <> struct Row4<bf16> {
  uint2 r;
  __device__ __forceinline__ void load(const bf16* p) { r = *reinterpret_cast<const uint2*>(p); }
  __device__ __forceinline__ float get(int j) const {
    const uint32_t w = (&r.x)[j >> 1];
    return __uint_as_float((j & 1) ? (w & 0xffff0000u) : (w << 16));
  }
};

struct MiDiv {
  FastDiv k1, v;
  VoxDiv vox;
};

// ROW4: C2 == 4 (the default MFE), a corner's row is one vector load; the sums per channel run over
// the corners in the same order either way
template <typename T, bool ROW4>
__global__ void __launch_bounds__(256) mfe_input_fwd(const T* __restrict__ fc, const float* __restrict__ kps,
                                                     const float* __restrict__ kpd, const float* __restrict__ J,
                                                     T* __restrict__ out, unsigned total, MiDiv dv, int Ns, int K,
                                                     int C2, int D, int H, int W, float var) {
  __shared__ __attribute__((aligned(16))) T tile[256 * MI_MAXCH];
  const int K1 = K + 1, CH = C2 + 1;
  const unsigned V = (unsigned)D * H * W;
  const unsigned gid = blockIdx.x * 256u + threadIdx.x;
  if (gid < total) {
    const unsigned nv = fdiv(gid, dv.k1);
    const int k = (int)(gid - nv * K1);
    const int n = (int)fdiv(nv, dv.v);
    const unsigned v = nv - (unsigned)n * V;
    const int ns = Ns == 1 ? 0 : n;
    float gx, gy, gz;
    ident(v, dv.vox, D, H, W, gx, gy, gz);
    float heat = 0.f, m0 = gx, m1 = gy, m2 = gz;
    if (k) {
      const float* kd = kpd + ((long)n * K + k - 1) * 3;
      const float* ks = kps + ((long)ns * K + k - 1) * 3;
      heat = gauss(gx, gy, gz, kd, var) - gauss(gx, gy, gz, ks, var);
      motion(gx, gy, gz, ks, kd, J + (long)n * 9, m0, m1, m2);
    }
    T* o = tile + threadIdx.x * CH;
    o[0] = Elt<T>::from_f(heat);
    const Cell cl = cell_of(m0, m1, m2, D, H, W);
    const T* base = fc + (long)ns * V * C2;
    if constexpr (ROW4) {
      float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int dx = i & 1, dy = (i >> 1) & 1, dz = i >> 2;
        const int xx = cl.x0 + dx, yy = cl.y0 + dy, zz = cl.z0 + dz;
        if ((unsigned)xx < (unsigned)W && (unsigned)yy < (unsigned)H && (unsigned)zz < (unsigned)D) {
          const float w = (dx ? cl.tx : 1.f - cl.tx) * (dy ? cl.ty : 1.f - cl.ty) * (dz ? cl.tz : 1.f - cl.tz);
          Row4<T> r;
          r.load(base + (((long)zz * H + yy) * W + xx) * 4);
#pragma unroll
          for (int c = 0; c < 4; ++c) acc[c] += w * r.get(c);
        }
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) o[1 + c] = Elt<T>::from_f(acc[c]);
    } else {
      for (int c = 0; c < C2; ++c) {
        float acc = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int dx = i & 1, dy = (i >> 1) & 1, dz = i >> 2;
          const int xx = cl.x0 + dx, yy = cl.y0 + dy, zz = cl.z0 + dz;
          if ((unsigned)xx < (unsigned)W && (unsigned)yy < (unsigned)H && (unsigned)zz < (unsigned)D) {
            const float w = (dx ? cl.tx : 1.f - cl.tx) * (dy ? cl.ty : 1.f - cl.ty) * (dz ? cl.tz : 1.f - cl.tz);
            acc += w * ld(base + (((long)zz * H + yy) * W + xx) * C2 + c);
          }
        }
        o[1 + c] = Elt<T>::from_f(acc);
      }
    }
  }
  __syncthreads();
  // the block's span: elements [e0, e0 + ne); e0 * sizeof(T) is a multiple of 512 bytes
  const long e0 = (long)blockIdx.x * 256 * CH;
  const long left = (long)total * CH - e0;
  const int ne = left < 256L * CH ? (int)left : 256 * CH;
  constexpr int PER16 = 16 / (int)sizeof(T);
  const int n16 = ne / PER16;
  const uint4* s16 = reinterpret_cast<const uint4*>(tile);
  uint4* d16 = reinterpret_cast<uint4*>(out + e0);
  for (int i = threadIdx.x; i < n16; i += 256) d16[i] = s16[i];
  for (int i = n16 * PER16 + threadIdx.x; i < ne; i += 256) out[e0 + i] = tile[i];
}

// ---- fv_motion_warp_fwd ----------------------------------------------------------------------
// C / 8 lanes per voxel, each sampling one 8-channel chunk (warp.hip's grid_sample3d_fwd8).  Every
// lane of a voxel forms the softmax over the voxel's K + 1 logits (one contiguous NDHWC row) and the
// blended deformation, with the motions recomputed from the keypoints; lane 0 of the voxel writes the
// deformation and, when asked for, the probabilities.
struct MwDiv {
  FastDiv c8, v;
  VoxDiv vox;
};

template <typename T>
__global__ void __launch_bounds__(256) motion_warp_fwd(const T* __restrict__ logits, const T* __restrict__ fs,
                                                       const float* __restrict__ kps, const float* __restrict__ kpd,
                                                       const float* __restrict__ J, T* __restrict__ out,
                                                       float* __restrict__ def, float* __restrict__ prob,
                                                       unsigned nvox, MwDiv dv, int Ns, int K, int C, int D, int H,
                                                       int W) {
  const int C8 = C >> 3, K1 = K + 1;
  const unsigned V = (unsigned)D * H * W;
  const unsigned gid = blockIdx.x * 256u + threadIdx.x;
  const unsigned nv = fdiv(gid, dv.c8);
  const int q = (int)(gid - nv * C8);
  if (nv >= nvox) return;
  const int n = (int)fdiv(nv, dv.v);
  const unsigned v = nv - (unsigned)n * V;
  const int ns = Ns == 1 ? 0 : n;
  const T* l = logits + (long)nv * K1;
  float m = -INFINITY;
  for (int k = 0; k < K1; ++k) m = fmaxf(m, ld(l + k));
  float z = 0.f;
  for (int k = 0; k < K1; ++k) z += expf(ld(l + k) - m);
  const float iz = 1.f / z;
  float gx, gy, gz;
  ident(v, dv.vox, D, H, W, gx, gy, gz);
  const float* j = J + (long)n * 9;
  float d0 = 0.f, d1 = 0.f, d2 = 0.f;
  for (int k = 0; k < K1; ++k) {
    const float p = expf(ld(l + k) - m) * iz;
    if (prob && q == 0) prob[((long)n * K1 + k) * V + v] = p;
    float s0 = gx, s1 = gy, s2 = gz;
    if (k) motion(gx, gy, gz, kps + ((long)ns * K + k - 1) * 3, kpd + ((long)n * K + k - 1) * 3, j, s0, s1, s2);
    d0 += p * s0;
    d1 += p * s1;
    d2 += p * s2;
  }
  if (q == 0) {
    def[(long)nv * 3] = d0;
    def[(long)nv * 3 + 1] = d1;
    def[(long)nv * 3 + 2] = d2;
  }
  const Cell cl = cell_of(d0, d1, d2, D, H, W);
  const T* base = fs + (long)ns * V * C + q * 8;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int dx = i & 1, dy = (i >> 1) & 1, dz = i >> 2;
    const int xx = cl.x0 + dx, yy = cl.y0 + dy, zz = cl.z0 + dz;
    if ((unsigned)xx < (unsigned)W && (unsigned)yy < (unsigned)H && (unsigned)zz < (unsigned)D) {
      const float w = (dx ? cl.tx : 1.f - cl.tx) * (dy ? cl.ty : 1.f - cl.ty) * (dz ? cl.tz : 1.f - cl.tz);
      Chunk8<T> c;
      c.load(base + (((long)zz * H + yy) * W + xx) * C);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += w * c.get(e);
    }
  }
  Chunk8<T> o;
  o.set8(acc);
  o.store(out + (long)nv * C + q * 8);
}

// ---- fv_frames_u8 ----------------------------------------------------------------------------
// out [N][H][2W][3] uint8: driving | generated, byte = trunc(255.0f * min(max(x, 0), 1)).  One lane
// per 4 output bytes (one 32-bit store); byte b of the output is channel b % 3 of pixel b / 3.
__device__ __forceinline__ unsigned frame_byte(const float* __restrict__ drv, const float* __restrict__ gen, long b,
                                               int H, int W) {
  const int c = (int)(b % 3);
  long p = b / 3;
  const int x = (int)(p % (2 * W));
  p /= 2 * W;
  const int y = (int)(p % H);
  const long n = p / H;
  const float* src = x < W ? drv : gen;
  const float val = src[((n * 3 + c) * H + y) * W + (x < W ? x : x - W)];
  const float clipped = fminf(fmaxf(val, 0.f), 1.f);
  return (unsigned)(int)__fmul_rn(255.0f, clipped);
}

__global__ void __launch_bounds__(256) frames_u8(const float* __restrict__ drv, const float* __restrict__ gen,
                                                 uint8_t* __restrict__ out, long nbytes, int H, int W) {
  const long b0 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (b0 >= nbytes) return;
  if (b0 + 4 <= nbytes) {
    unsigned word = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) word |= frame_byte(drv, gen, b0 + i, H, W) << (8 * i);
    *reinterpret_cast<unsigned*>(out + b0) = word;
  } else {
    for (long b = b0; b < nbytes; ++b) out[b] = (uint8_t)frame_byte(drv, gen, b, H, W);
  }
}

// ---- fv_frames_from_u8 -----------------------------------------------------------------------
// in [T][H][W][3] uint8 -> out [T][3][H][W] fp32 = x * fp32(1 / 255): one rounded multiply, as numpy's
// np.multiply(a, float32(1 / 255), dtype=float32).  One lane per 4 input bytes (one 32-bit load when the
// input is 4-byte aligned); byte b of the input is channel b % 3 of pixel b / 3.
__device__ __forceinline__ void frame_float(float* __restrict__ out, unsigned byte, long b, long HW) {
  const int c = (int)(b % 3);
  const long p = b / 3;               // pixel index over [T][H][W]
  const long n = p / HW;
  out[(n * 3 + c) * HW + (p - n * HW)] = __fmul_rn((float)byte, (float)(1.0 / 255.0));
}

template <bool ALIGNED>
__global__ void __launch_bounds__(256) frames_from_u8(const uint8_t* __restrict__ in, float* __restrict__ out,
                                                      long nbytes, long HW) {
  const long b0 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (b0 >= nbytes) return;
  if (ALIGNED && b0 + 4 <= nbytes) {
    const unsigned word = *reinterpret_cast<const unsigned*>(in + b0);
#pragma unroll
    for (int i = 0; i < 4; ++i) frame_float(out, (word >> (8 * i)) & 0xffu, b0 + i, HW);
  } else {
    const long b1 = b0 + 4 < nbytes ? b0 + 4 : nbytes;
    for (long b = b0; b < b1; ++b) frame_float(out, in[b], b, HW);
  }
}

// ---- fv_pose_kp_fwd / fv_pose_kp_new_fwd -------------------------------------------------------
// transform_kp / transform_kp_with_new_pose (utils.py:53-76) and the motion Jacobian Rs inv(R) of
// create_sparse_motions (utils.py:146).  A few hundred keypoints at most: latency, not bandwidth.  Every
// lane rebuilds its sample's 3x3 matrices from the angles (sinf / cosf); nothing is exchanged but the
// z-sum of the new-pose kernel.
struct Mat3 {
  float m[9];
};

__device__ __forceinline__ Mat3 mul3(const Mat3& a, const Mat3& b) {
  Mat3 r;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
      r.m[i * 3 + j] = a.m[i * 3] * b.m[j] + a.m[i * 3 + 1] * b.m[3 + j] + a.m[i * 3 + 2] * b.m[6 + j];
  return r;
}

// Ry(pitch) Rx(yaw) Rz(roll) in the reference's naming of the axes (utils.py:5-57)
__device__ __forceinline__ Mat3 rotation(float yaw, float pitch, float roll) {
  const float cy = cosf(yaw), sy = sinf(yaw), cp = cosf(pitch), sp = sinf(pitch), cr = cosf(roll), sr = sinf(roll);
  const Mat3 rx = {{cy, 0.f, sy, 0.f, 1.f, 0.f, -sy, 0.f, cy}};
  const Mat3 ry = {{1.f, 0.f, 0.f, 0.f, cp, -sp, 0.f, sp, cp}};
  const Mat3 rz = {{cr, -sr, 0.f, sr, cr, 0.f, 0.f, 0.f, 1.f}};
  return mul3(mul3(ry, rx), rz);
}

// the general inverse (adjugate over determinant), as torch.inverse: not the transpose
__device__ __forceinline__ Mat3 inverse3(const Mat3& a) {
  const float* m = a.m;
  const float c00 = m[4] * m[8] - m[5] * m[7], c01 = m[5] * m[6] - m[3] * m[8], c02 = m[3] * m[7] - m[4] * m[6];
  const float id = 1.f / (m[0] * c00 + m[1] * c01 + m[2] * c02);
  Mat3 r;
  r.m[0] = c00 * id;
  r.m[1] = (m[2] * m[7] - m[1] * m[8]) * id;
  r.m[2] = (m[1] * m[5] - m[2] * m[4]) * id;
  r.m[3] = c01 * id;
  r.m[4] = (m[0] * m[8] - m[2] * m[6]) * id;
  r.m[5] = (m[2] * m[3] - m[0] * m[5]) * id;
  r.m[6] = c02 * id;
  r.m[7] = (m[1] * m[6] - m[0] * m[7]) * id;
  r.m[8] = (m[0] * m[4] - m[1] * m[3]) * id;
  return r;
}

__device__ __forceinline__ void apply3(const Mat3& a, float x, float y, float z, float* o) {
#pragma unroll
  for (int i = 0; i < 3; ++i) o[i] = a.m[i * 3] * x + a.m[i * 3 + 1] * y + a.m[i * 3 + 2] * z;
}

// lane 0 of a sample: R and, for a non-null Rs, J = Rs inv(R)
__device__ __forceinline__ void store_R_J(const Mat3& R, const float* __restrict__ Rs, int ns, float* __restrict__ Rout,
                                          float* __restrict__ J, int n) {
#pragma unroll
  for (int i = 0; i < 9; ++i) Rout[(long)n * 9 + i] = R.m[i];
  if (Rs) {
    Mat3 s;
#pragma unroll
    for (int i = 0; i < 9; ++i) s.m[i] = Rs[(long)ns * 9 + i];
    const Mat3 j = mul3(s, inverse3(R));
#pragma unroll
    for (int i = 0; i < 9; ++i) J[(long)n * 9 + i] = j.m[i];
  }
}

// one lane per (sample, keypoint)
__global__ void __launch_bounds__(256) pose_kp_fwd(const float* __restrict__ kp_c, const float* __restrict__ yaw,
                                                   const float* __restrict__ pitch, const float* __restrict__ roll,
                                                   const float* __restrict__ t, const float* __restrict__ scale,
                                                   const float* __restrict__ Rs, float* __restrict__ kp,
                                                   float* __restrict__ Rout, float* __restrict__ J, int N, int Nc, int Ns,
                                                   int K) {
  const int gid = blockIdx.x * 256 + threadIdx.x;
  if (gid >= N * K) return;
  const int n = gid / K, k = gid - n * K;
  const Mat3 R = rotation(yaw[n], pitch[n], roll[n]);
  const float* c = kp_c + ((long)(Nc == 1 ? 0 : n) * K + k) * 3;
  const float s = scale[n];
  float o[3];
  apply3(R, s * c[0], s * c[1], s * c[2], o);
#pragma unroll
  for (int i = 0; i < 3; ++i) kp[(long)gid * 3 + i] = o[i] + t[n * 3 + i];
  if (k == 0) store_R_J(R, Rs, Ns == 1 ? 0 : n, Rout, J, n);
}

// One block.  Lane l owns keypoints l, l + 256, ...: it writes their unshifted coordinates, sums its z in
// that order, the 256 partial sums are added by one fixed tree in LDS, and every lane then shifts the z it
// wrote itself.  The order of the sum depends on N K alone.
constexpr int PN_THREADS = 256;
constexpr int PN_MAX_KP = 1 << 16;   // 256 keypoints per lane: keeps the single block's loop short

__global__ void __launch_bounds__(PN_THREADS) pose_kp_new_fwd(
    const float* __restrict__ kp_in, const float* __restrict__ yaw, const float* __restrict__ pitch,
    const float* __restrict__ roll, const float* __restrict__ t, const float* __restrict__ delta,
    const float* __restrict__ nyaw, const float* __restrict__ npitch, const float* __restrict__ nroll,
    const float* __restrict__ Rs, float* __restrict__ kp, float* __restrict__ Rout, float* __restrict__ J, int N,
    int Ns, int K) {
  __shared__ float part[PN_THREADS];
  const int total = N * K;
  float zsum = 0.f;
  for (int g = threadIdx.x; g < total; g += PN_THREADS) {
    const int n = g / K, k = g - n * K;
    const Mat3 Rn = rotation(nyaw[n], npitch[n], nroll[n]);
    const Mat3 Rrel = mul3(Rn, inverse3(rotation(yaw[n], pitch[n], roll[n])));
    const float* c = kp_in + (long)g * 3;
    const float* d = delta + (long)g * 3;
    float a[3], b[3];
    apply3(Rn, c[0], c[1], c[2], a);
    apply3(Rrel, d[0], d[1], d[2], b);
#pragma unroll
    for (int i = 0; i < 3; ++i) a[i] = a[i] + t[n * 3 + i] + b[i];
    kp[(long)g * 3] = a[0];
    kp[(long)g * 3 + 1] = a[1];
    kp[(long)g * 3 + 2] = a[2];
    zsum += a[2];
    if (k == 0) store_R_J(Rn, Rs, Ns == 1 ? 0 : n, Rout, J, n);
  }
  part[threadIdx.x] = zsum;
  __syncthreads();
  for (int s = PN_THREADS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
    __syncthreads();
  }
  const float shift = 0.33f - part[0] / (float)total;
  for (int g = threadIdx.x; g < total; g += PN_THREADS) kp[(long)g * 3 + 2] += shift;
}

bool motion_args_ok(const void* a, const void* b, const float* kp_s, const float* kp_d, const float* J, int N, int Ns,
                    int K, int D, int H, int W) {
  return a && b && kp_s && kp_d && J && N > 0 && (Ns == 1 || Ns == N) && K > 0 && D > 1 && H > 1 && W > 1;
}

}  // namespace

extern "C" {

int fv_mfe_input_fwd(int dtype, const void* fc, const float* kp_s, const float* kp_d, const float* J, int N, int Ns,
                     int K, int C2, int D, int H, int W, float var, void* out, void* stream) {
  FV_REQUIRE(motion_args_ok(fc, out, kp_s, kp_d, J, N, Ns, K, D, H, W) && C2 > 0, "mfe_input: bad argument");
  FV_REQUIRE(dtype == FV_F32 || dtype == FV_BF16, "mfe_input: f32 or bf16");
  FV_REQUIRE(C2 + 1 <= MI_MAXCH, "mfe_input: C2 + 1 <= %d (got C2 = %d)", MI_MAXCH, C2);
  FV_REQUIRE(((uintptr_t)out & 15) == 0, "mfe_input: the output must be 16-byte aligned");
  const long total = (long)N * D * H * W * (K + 1);
  FV_REQUIRE(total < (1L << 31) - 256, "mfe_input: N D H W (K + 1) must stay below 2^31 - 256 (got %ld)", total);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)((total + 255) / 256));
  const MiDiv dv = {make_fastdiv((uint32_t)(K + 1)), make_fastdiv((uint32_t)(D * H * W)),
                    {make_fastdiv((uint32_t)W), make_fastdiv((uint32_t)H)}};
#define MI_LAUNCH(T, R4)                                                                                          \
  hipLaunchKernelGGL((mfe_input_fwd<T, R4>), grid, dim3(256), 0, s, (const T*)fc, kp_s, kp_d, J, (T*)out,          \
                     (unsigned)total, dv, Ns, K, C2, D, H, W, var)
  if (dtype == FV_BF16) {
    if (C2 == 4) MI_LAUNCH(bf16, true); else MI_LAUNCH(bf16, false);
  } else {
    if (C2 == 4) MI_LAUNCH(float, true); else MI_LAUNCH(float, false);
  }
#undef MI_LAUNCH
  return fv_check_launch("mfe_input_fwd");
}

int fv_motion_warp_fwd(int dtype, const void* logits, const void* fs, const float* kp_s, const float* kp_d,
                       const float* J, int N, int Ns, int K, int C, int D, int H, int W, void* out, float* deformation,
                       float* prob, void* stream) {
  FV_REQUIRE(motion_args_ok(logits, fs, kp_s, kp_d, J, N, Ns, K, D, H, W) && out && deformation,
             "motion_warp: bad argument");
  FV_REQUIRE(dtype == FV_F32 || dtype == FV_BF16, "motion_warp: f32 or bf16");
  FV_REQUIRE(C > 0 && C % 8 == 0, "motion_warp: C must be a multiple of 8 (got %d)", C);
  const long nvox = (long)N * D * H * W;
  FV_REQUIRE(nvox * (C / 8) < (1L << 31) - 256, "motion_warp: N D H W C / 8 must stay below 2^31 - 256 (got %ld)",
             nvox * (C / 8));
  const long nblk = (nvox * (C / 8) + 255) / 256;
  const MwDiv dv = {make_fastdiv((uint32_t)(C / 8)), make_fastdiv((uint32_t)(D * H * W)),
                    {make_fastdiv((uint32_t)W), make_fastdiv((uint32_t)H)}};
  hipStream_t s = (hipStream_t)stream;
  if (dtype == FV_BF16)
    hipLaunchKernelGGL(motion_warp_fwd<bf16>, dim3((unsigned)nblk), dim3(256), 0, s, (const bf16*)logits,
                       (const bf16*)fs, kp_s, kp_d, J, (bf16*)out, deformation, prob, (unsigned)nvox, dv, Ns, K, C, D, H,
                       W);
  else
    hipLaunchKernelGGL(motion_warp_fwd<float>, dim3((unsigned)nblk), dim3(256), 0, s, (const float*)logits,
                       (const float*)fs, kp_s, kp_d, J, (float*)out, deformation, prob, (unsigned)nvox, dv, Ns, K, C, D, H,
                       W);
  return fv_check_launch("motion_warp_fwd");
}

int fv_frames_u8(const float* driving, const float* generated, int N, int H, int W, void* out, void* stream) {
  FV_REQUIRE(driving && generated && out && N > 0 && H > 0 && W > 0, "frames_u8: bad argument");
  FV_REQUIRE(((uintptr_t)out & 3) == 0, "frames_u8: the output must be 4-byte aligned");
  const long nbytes = (long)N * H * W * 6;
  const long nblk = ((nbytes + 3) / 4 + 255) / 256;
  FV_REQUIRE(nblk < (1L << 31), "frames_u8: too many pixels");
  hipLaunchKernelGGL(frames_u8, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, driving, generated,
                     (uint8_t*)out, nbytes, H, W);
  return fv_check_launch("frames_u8");
}

int fv_frames_from_u8(const void* frames, int T, int H, int W, float* out, void* stream) {
  FV_REQUIRE(frames && out && T > 0 && H > 0 && W > 0, "frames_from_u8: bad argument");
  const long HW = (long)H * W, nbytes = (long)T * HW * 3;
  const long nblk = ((nbytes + 3) / 4 + 255) / 256;
  FV_REQUIRE(nblk < (1L << 31), "frames_from_u8: too many pixels");
  const dim3 grid((unsigned)nblk);
  hipStream_t s = (hipStream_t)stream;
  if (((uintptr_t)frames & 3) == 0)
    hipLaunchKernelGGL(frames_from_u8<true>, grid, dim3(256), 0, s, (const uint8_t*)frames, out, nbytes, HW);
  else
    hipLaunchKernelGGL(frames_from_u8<false>, grid, dim3(256), 0, s, (const uint8_t*)frames, out, nbytes, HW);
  return fv_check_launch("frames_from_u8");
}

int fv_pose_kp_fwd(const float* kp_c, const float* yaw, const float* pitch, const float* roll, const float* t,
                   const float* scale, const float* Rs, int N, int Nc, int Ns, int K, float* kp, float* R, float* J,
                   void* stream) {
  FV_REQUIRE(kp_c && yaw && pitch && roll && t && scale && kp && R && N > 0 && K > 0, "pose_kp: bad argument");
  FV_REQUIRE(Nc == 1 || Nc == N, "pose_kp: kp_c holds 1 or N = %d samples (got %d)", N, Nc);
  FV_REQUIRE(!Rs || (J && (Ns == 1 || Ns == N)), "pose_kp: Rs needs J and 1 or N = %d samples (got %d)", N, Ns);
  FV_REQUIRE((long)N * K < (1L << 31) - 256, "pose_kp: N K must stay below 2^31 - 256");
  hipLaunchKernelGGL(pose_kp_fwd, dim3((unsigned)((N * K + 255) / 256)), dim3(256), 0, (hipStream_t)stream, kp_c, yaw,
                     pitch, roll, t, scale, Rs, kp, R, J, N, Nc, Ns, K);
  return fv_check_launch("pose_kp_fwd");
}

int fv_pose_kp_new_fwd(const float* kp_in, const float* yaw, const float* pitch, const float* roll, const float* t,
                       const float* delta, const float* new_yaw, const float* new_pitch, const float* new_roll,
                       const float* Rs, int N, int Ns, int K, float* kp, float* R, float* J, void* stream) {
  FV_REQUIRE(kp_in && yaw && pitch && roll && t && delta && new_yaw && new_pitch && new_roll && kp && R && N > 0 &&
                 K > 0, "pose_kp_new: bad argument");
  FV_REQUIRE(!Rs || (J && (Ns == 1 || Ns == N)), "pose_kp_new: Rs needs J and 1 or N = %d samples (got %d)", N, Ns);
  FV_REQUIRE((long)N * K <= PN_MAX_KP,
             "pose_kp_new: N K <= %d (got %ld): the z-mean over the call is one block's fixed-order sum", PN_MAX_KP,
             (long)N * K);
  hipLaunchKernelGGL(pose_kp_new_fwd, dim3(1), dim3(PN_THREADS), 0, (hipStream_t)stream, kp_in, yaw, pitch, roll, t,
                     delta, new_yaw, new_pitch, new_roll, Rs, kp, R, J, N, Ns, K);
  return fv_check_launch("pose_kp_new_fwd");
}

}  // extern "C"
