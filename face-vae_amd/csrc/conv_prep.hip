// Weight preparation of the 2-D convolution: the kernels that re-lay a parameter [co][ci][r][s]
// (x 1/sigma) into the images the forward and data-gradient kernels read, and the four weight
// kernels of ConvTranspose2dELR (norm, phase images, slab reduction, weight backward; the
// mapping they implement is described above fv_convt_supported in conv.hip).  One host launcher
// per kernel family, declared in conv_plan.h: the entries in conv.hip (fv_conv_weight_prep*,
// fv_conv2d_s2_weight_prep, fv_convt_*) choose the layout, the sizes and the grid; a launcher only
// picks the instantiation.  No planner call, no environment switch and no exported entry here.
#include "conv_plan.h"

namespace {

// the weights of conv7_n3_fwd2 (conv_shapes.hip), wn [32][448]: n = co * 7 + s (co < cout, s < 7),
// k = r * 64 + ci
__global__ void weight_prep_c7n_kernel(const float* __restrict__ wp, const float* sigma, bf16* wn, int cout) {
  const float inv = sigma ? 1.f / sigma[0] : 1.f;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < 32 * 448; e += gridDim.x * blockDim.x) {
    const int nn = e / 448, k = e - nn * 448;
    const int co = nn / 7, s = nn - co * 7, r = k >> 6, ci = k & 63;
    const float v = co < cout ? wp[((co * 64 + ci) * 7 + r) * 7 + s] * inv : 0.f;
    wn[e] = (bf16)v;
  }
}

// ----------------------------------------------------------------------------------------
// weight re-layout (+ 1/sigma)
// ----------------------------------------------------------------------------------------
// smaj 2: the packed 7x7 layout of conv7c4_fwd ([row][224], 2 taps x 4 channels per 16 B).
// smaj 1 (the layout conv3_halo_fwd3 reads, h3s_layout): stage-major [u = c * 9 + tap][row][32]
// with c the 32-channel chunk, so every 16-row DMA piece of a weight stage is one contiguous
// 1 KB (8 whole 128-B lines) instead of 16 row segments of 64 B.  Requires KS == 3,
// Kpad == 9 * Cin and Cin % 32 == 0.
template <typename T>
__device__ __forceinline__ void weight_prep_body(const float* __restrict__ wp, const float* sigma, T* wk, int rows,
                                                 int Kpad, int cout, int cin_valid, int lgCin, int KS, int K,
                                                 int transposed, int bid, int nblk, int smaj = 0) {
  // 32-bit index math (a weight image is < 2^31 elements; the 64-bit divisions per element
  // dominated the batched launch)
  const int total = rows * Kpad;
  const float inv = sigma ? 1.f / sigma[0] : 1.f;
  for (int e = bid * (int)blockDim.x + threadIdx.x; e < total; e += nblk * (int)blockDim.x) {
    int row, k;
    bool kin;
    int tap, c;
    if (smaj == 2) {            // conv7c4_fwd: [row][224], k = r * 32 + s * 4 + ci (s = 7: zero)
      row = e / C74_K;
      k = e - row * C74_K;
      const int sk = (k >> 2) & 7;
      kin = sk < 7;
      tap = (k >> 5) * 7 + sk;
      c = k & 3;
    } else {
      if (smaj) {
        const int q = e >> 5, u = q / rows;
        row = q - u * rows;
        const int cc = u / 9, t = u - cc * 9;
        k = (t << lgCin) + cc * 32 + (e & 31);
      } else {
        row = e / Kpad;
        k = e - row * Kpad;
      }
      kin = k < K;
      tap = k >> lgCin;
      c = k & ((1 << lgCin) - 1);
    }
    float v = 0.f;
    if (kin) {
      const int r = tap / KS, s = tap - (tap / KS) * KS;
      if (!transposed) {        // wk[co][(r,s,ci)] = W[co][ci][r][s]
        if (row < cout && c < cin_valid) v = wp[(((long)row * cin_valid + c) * KS + r) * KS + s];
      } else {                  // wt[ci][(r',s',co)] = W[co][ci][KS-1-r'][KS-1-s']
        if (row < cin_valid && c < cout)
          v = wp[(((long)c * cin_valid + row) * KS + (KS - 1 - r)) * KS + (KS - 1 - s)];
      }
    }
    wk[e] = Elt<T>::from_f(v * inv);
  }
}

template <typename T>
__global__ void weight_prep_kernel(const float* __restrict__ wp, const float* sigma, T* wk,
                                   int rows, int Kpad, int cout, int cin_valid, int lgCin, int KS,
                                   int K, int transposed, int smaj) {
  weight_prep_body<T>(wp, sigma, wk, rows, Kpad, cout, cin_valid, lgCin, KS, K, transposed, blockIdx.x, gridDim.x,
                      smaj);
}

// Data-gradient weights of the stride-2 3x3 conv (conv_fwd_kernel S2 == 2): four phase images
// [phase = 2 pa + pb][rows][Kph], Kph = 4 * cin_t (the (1 + pa)(1 + pb) * cin_t live k of a phase
// first, zeros behind).  dx[2h + pa][2w + pb] = sum of dy[h + r][w + s] W[co][ci][kr][kc] over
// the taps with 2 (h + r) + kr - 1 = 2h + pa: an even row (pa = 0) meets only kr = 1 at r = 0,
// an odd row kr = 2 at r = 0 and kr = 0 at r = 1; columns alike.
template <typename T>
__global__ void weight_prep_s2t_kernel(const float* __restrict__ wp, const float* sigma, T* wt, int rows, int Kph,
                                       int cout, int cin_valid, int lgC) {
  const int total = 4 * rows * Kph;
  const float inv = sigma ? 1.f / sigma[0] : 1.f;
  for (int e = blockIdx.x * (int)blockDim.x + threadIdx.x; e < total; e += gridDim.x * (int)blockDim.x) {
    const int ph = e / (rows * Kph), q = e - ph * rows * Kph;
    const int row = q / Kph, k = q - row * Kph;
    const int pa = ph >> 1, pb = ph & 1;
    const int tap = k >> lgC, c = k & ((1 << lgC) - 1);
    const int r = tap >> pb, s = tap & pb;
    float v = 0.f;
    if (tap < (1 + pa) * (1 + pb) && row < cin_valid && c < cout) {
      const int kr = pa ? 2 - 2 * r : 1, kc = pb ? 2 - 2 * s : 1;
      v = wp[(((long)c * cin_valid + row) * 3 + kr) * 3 + kc];
    }
    wt[e] = Elt<T>::from_f(v * inv);
  }
}

// both layouts in one launch: blocks [0, nb1) write wk, the rest wt (WPrepJob: conv_plan.h)
template <typename T>
__global__ void weight_prep2_kernel(const float* __restrict__ wp, const float* sigma, int cout, int cin_valid, int KS,
                                    WPrepJob j0, WPrepJob j1) {
  const bool second = (int)blockIdx.x >= j0.nb;
  const WPrepJob& j = second ? j1 : j0;
  weight_prep_body<T>(wp, sigma, (T*)j.out, j.rows, j.Kpad, cout, cin_valid, j.lgCin, KS, j.K, j.transposed,
                      second ? blockIdx.x - j0.nb : blockIdx.x, j.nb, j.smaj);
}

// one launch for the generic weight layouts of many convs (fv_conv_weight_prep_multi; WPrepMulti:
// conv_plan.h).  grid (max nb, jobs): blockIdx.y selects the job directly (a per-block search over the job
// list in kernel-argument memory cost more than the launches it replaced)
template <typename T>
__global__ void weight_prep_multi_kernel(WPrepMulti m) {
  const WPrepMJob& j = m.j[blockIdx.y];
  if ((int)blockIdx.x >= j.nb) return;
  weight_prep_body<T>(j.w, j.sigma, (T*)j.out, j.rows, j.Kpad, j.cout, j.cin_valid, j.lgCin, j.KS, j.K, j.transposed,
                      blockIdx.x, j.nb, j.smaj);
}

// sub-pixel phase weights of an upsample + 3x3 conv: for phase (pa, pb) the 2x2 tap (r', s')
// sums the 3x3 taps that land on the same low-res input pixel (rows r in [lo, hi] with
// lo = r' ? 1 + pa : 0, hi = r' ? 2 : pa; columns alike).  wk [4][rows][Kpad], k = (r'*2+s')*cin + ci.
template <typename T>
__global__ void weight_prep_subpix_kernel(const float* __restrict__ wp, const float* sigma, T* wk, int rows, int Kpad,
                                          int cout, int cin_valid, int lgCin) {
  const long per = (long)rows * Kpad, total = 4 * per;
  const float inv = sigma ? 1.f / sigma[0] : 1.f;
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const int ph = (int)(e / per);
    const long e2 = e - ph * per;
    const int row = (int)(e2 / Kpad), k = (int)(e2 - (long)row * Kpad);
    const int pa = ph >> 1, pb = ph & 1;
    const int tap = k >> lgCin, c = k & ((1 << lgCin) - 1);
    float v = 0.f;
    if (tap < 4 && row < cout && c < cin_valid) {
      const int rr = tap >> 1, ss = tap & 1;
      const int r0 = rr ? 1 + pa : 0, r1 = rr ? 2 : pa;
      const int s0 = ss ? 1 + pb : 0, s1 = ss ? 2 : pb;
      const float* w = wp + ((long)row * cin_valid + c) * 9;
      for (int r = r0; r <= r1; ++r)
        for (int q = s0; q <= s1; ++q) v += w[r * 3 + q];
    }
    wk[e] = Elt<T>::from_f(v * inv);
  }
}

// stride-2 4x4 weights of the low-res data gradient of an upsample + 3x3 conv:
// wt[ci][(tr*4 + tc)*cin_t + co] = sum of W[co][ci][r][s] over r in [max(0, 2-tr), min(2, 3-tr)]
// and s alike (dy row 2u + tr - 1 reaches low-res row u through those taps).
template <typename T>
__global__ void weight_prep_s2_kernel(const float* __restrict__ wp, const float* sigma, T* wt, int rows, int Kpad,
                                      int cout, int cin_valid, int lgCt) {
  const long total = (long)rows * Kpad;
  const float inv = sigma ? 1.f / sigma[0] : 1.f;
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const int row = (int)(e / Kpad), k = (int)(e - (long)row * Kpad);
    const int tap = k >> lgCt, co = k & ((1 << lgCt) - 1);
    float v = 0.f;
    if (tap < 16 && row < cin_valid && co < cout) {
      const int tr = tap >> 2, tc = tap & 3;
      const int r0 = max(0, 2 - tr), r1 = min(2, 3 - tr), s0 = max(0, 2 - tc), s1 = min(2, 3 - tc);
      const float* w = wp + ((long)co * cin_valid + row) * 9;
      for (int r = r0; r <= r1; ++r)
        for (int q = s0; q <= s1; ++q) v += w[r * 3 + q];
    }
    wt[e] = Elt<T>::from_f(v * inv);
  }
}

// Weight images of conv3_halo_fwd3 MODE 1 / 2: unit u = chunk c * 4 + q, a [rows][32] block per
// unit (stage-major, as weight_prep_body smaj 1), q = (q >> 1, q & 1).
//   MODE 1 (sub-pixel forward, wk): rows = 4 cout, row = tn * 256 + phase * 64 + co % 64 for
//     co = tn * 64 + co % 64; element k = input channel c * 32 + k: phase (pa, pb)'s 2x2 tap
//     (rr, ss) = q, the folded 3x3 sum of weight_prep_subpix_kernel.
//   MODE 2 (low-res data gradient, wt): rows = the tile rows (cin of the conv), chunk c = (plane
//     (py, px) = c / cpp, 32 output channels (c % cpp) * 32 + k); q = (a, b) is the stride-2
//     tap (tr, tc) = (2a + 1 - py, 2b + 1 - px) of weight_prep_s2_kernel.
// CONVT: the ConvTranspose2dELR k4 s2 p1 weights w [ci][co][4][4] (x gain (x cinv[co], demod))
// on the same kernels: phase (pa, pb) tap (rr, ss) SELECTS Weff[ci][co][3 - pa - 2 rr][3 - pb - 2 ss]
// (convt_weight_prep_kernel's map), and the stride-2 data-gradient tap (tr, tc) is Weff[ci][co][tr][tc].
template <int MODE, bool CONVT = false>
__global__ void weight_prep_phase_kernel(const float* __restrict__ wp, const float* sigma, bf16* out, int rows,
                                         int units, int cout, int cin_valid, int cpp, const float* cinv = nullptr,
                                         float gain = 1.f) {
  const int total = units * rows * 32;
  const float inv = sigma ? 1.f / sigma[0] : 1.f;
  for (int e = blockIdx.x * (int)blockDim.x + threadIdx.x; e < total; e += gridDim.x * (int)blockDim.x) {
    const int k = e & 31, qe = e >> 5, u = qe / rows, row = qe - u * rows;
    const int c = u >> 2, q = u & 3;
    int co, ci, r0, r1, s0, s1;
    if constexpr (MODE == 1) {
      const int ph = (row >> 6) & 3, pa = ph >> 1, pb = ph & 1, rr = q >> 1, ss = q & 1;
      co = (row >> 8) * 64 + (row & 63);
      ci = c * 32 + k;
      r0 = rr ? 1 + pa : 0; r1 = rr ? 2 : pa;
      s0 = ss ? 1 + pb : 0; s1 = ss ? 2 : pb;
    } else {
      const int pl = c / cpp, tr = 2 * (q >> 1) + 1 - (pl >> 1), tc = 2 * (q & 1) + 1 - (pl & 1);
      co = (c - pl * cpp) * 32 + k;
      ci = row;
      r0 = max(0, 2 - tr); r1 = min(2, 3 - tr);
      s0 = max(0, 2 - tc); s1 = min(2, 3 - tc);
    }
    float v = 0.f;
    if (co < cout && ci < cin_valid) {
      if constexpr (CONVT) {
        int tr, tc;
        if constexpr (MODE == 1) {
          tr = 3 - ((row >> 7) & 1) - 2 * (q >> 1);
          tc = 3 - ((row >> 6) & 1) - 2 * (q & 1);
        } else {
          const int pl = c / cpp;
          tr = 2 * (q >> 1) + 1 - (pl >> 1);
          tc = 2 * (q & 1) + 1 - (pl & 1);
        }
        v = wp[((long)ci * cout + co) * 16 + tr * 4 + tc] * (cinv ? gain * cinv[co] : gain);
      } else {
        const float* w = wp + ((long)co * cin_valid + ci) * 9;
        for (int r = r0; r <= r1; ++r)
          for (int t = s0; t <= s1; ++t) v += w[r * 3 + t];
      }
    }
    out[e] = Elt<bf16>::from_f(CONVT ? v : v * inv);
  }
}

// ----------------------------------------------------------------------------------------
// ConvTranspose2dELR, kernel 4 / stride 2 / padding 1: its weight kernels (the mapping to the
// upsample-conv kernels is described with the fv_convt_* entries in conv.hip)
// ----------------------------------------------------------------------------------------
// one wave per output channel: inv[co] = 1 / max(||W[:, co, :, :]||_2, 1e-12)
__global__ void convt_norm_kernel(const float* __restrict__ w, int cin, int cout, float* inv) {
  const int co = blockIdx.x, l = threadIdx.x;
  float s = 0.f;
  for (int e = l; e < cin * 16; e += 64) {
    const float v = w[((long)(e >> 4) * cout + co) * 16 + (e & 15)];
    s += v * v;
  }
  s = wave_sum(s);
  if (l == 0) inv[co] = 1.f / fmaxf(sqrtf(s), 1e-12f);
}

__device__ __forceinline__ float convt_scale(const float* inv, int co, float gain) {
  return inv ? gain * inv[co] : gain;
}

// wk [4][rows][Kpad] (k = (r'*2 + s')*cin + ci) and wt [rows_t][16*cin_t] (k = (tr*4 + tc)*cin_t + co)
__global__ void convt_weight_prep_kernel(const float* __restrict__ w, const float* __restrict__ inv, float gain,
                                         bf16* wk, int rows, int Kpad, int lgCin, bf16* wt, int rows_t,
                                         int lgCt, int cin_valid, int cout) {
  const long nk = wk ? 4L * rows * Kpad : 0;
  const long nt = wt ? (long)rows_t * (16L << lgCt) : 0;
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < nk + nt; e += (long)gridDim.x * blockDim.x) {
    float v = 0.f;
    if (e < nk) {
      const long per = (long)rows * Kpad;
      const int ph = (int)(e / per);
      const long e2 = e - ph * per;
      const int co = (int)(e2 / Kpad), k = (int)(e2 - (long)co * Kpad);
      const int tap = k >> lgCin, ci = k & ((1 << lgCin) - 1);
      if (tap < 4 && co < cout && ci < cin_valid) {
        const int tr = 3 - (ph >> 1) - 2 * (tap >> 1), tc = 3 - (ph & 1) - 2 * (tap & 1);
        v = w[((long)ci * cout + co) * 16 + tr * 4 + tc] * convt_scale(inv, co, gain);
      }
      wk[e] = (bf16)v;
    } else {
      const long e2 = e - nk;
      const int Kt = 16 << lgCt;
      const int ci = (int)(e2 / Kt), k = (int)(e2 - (long)ci * Kt);
      const int tap = k >> lgCt, co = k & ((1 << lgCt) - 1);
      if (ci < cin_valid && co < cout)
        v = w[((long)ci * cout + co) * 16 + tap] * convt_scale(inv, co, gain);
      wt[e2] = (bf16)v;
    }
  }
}

// phase slabs [4][nsplit][CW][KW] (rows co, k = ((r'*2 + s') << lgCin) + ci) -> G [ci][co][4][4]
// = dL/dWeff, one wave per 64 outputs, 4 lanes per output summing interleaved splits; + db.
__global__ void convt_wgrad_reduce_kernel(const float* __restrict__ slab, const float* __restrict__ bslab, float* dw,
                                          float* db, int nsplit, int CW, int KW, int cout, int cin_valid, int lgCin,
                                          int nb_main) {
  const int sg = threadIdx.x >> 6, l = threadIdx.x & 63;
  __shared__ float red[4][64];
  float g = 0.f;
  long dst = -1;
  if ((int)blockIdx.x < nb_main) {
    const long e = (long)blockIdx.x * 64 + l;
    if (e < (long)cin_valid * cout * 16) {
      dst = e;
      const int t = (int)(e & 15), co = (int)((e >> 4) % cout), ci = (int)((e >> 4) / cout);
      const int tr = t >> 2, tc = t & 3;
      const int ph = (1 - (tr & 1)) * 2 + (1 - (tc & 1));
      const int tap = (tr < 2) * 2 + (tc < 2);
      for (int sp = sg; sp < nsplit; sp += 4)
        g += slab[((long)(ph * nsplit + sp) * CW + co) * KW + ((tap << lgCin) + ci)];
    }
  } else {
    const int co = ((int)blockIdx.x - nb_main) * 64 + l;
    if (co < cout) {
      dst = co;
      for (int t = sg; t < 4 * nsplit; t += 4) g += bslab[(long)t * CW + co];
    }
  }
  red[sg][l] = g;
  __syncthreads();
  if (sg == 0 && dst >= 0) {
    const float v = (red[0][l] + red[1][l]) + (red[2][l] + red[3][l]);
    if ((int)blockIdx.x < nb_main) dw[dst] = v;
    else db[dst] = v;
  }
}

// in place, one wave per co: G = dL/dWeff -> dL/dW.  demod: Wn = W * inv,
// dW = gain * inv * (G - Wn <Wn, G>) (the max(norm, eps) clamp: dW = gain * inv * G); else gain * G.
__global__ void convt_weight_bwd_kernel(const float* __restrict__ w, const float* __restrict__ inv, float gain,
                                        float* g, int cin, int cout) {
  const int co = blockIdx.x, l = threadIdx.x;
  const float iv = inv ? inv[co] : 1.f;
  float dot = 0.f;
  if (inv && iv < 1e12f) {
    for (int e = l; e < cin * 16; e += 64) {
      const long a = ((long)(e >> 4) * cout + co) * 16 + (e & 15);
      dot += w[a] * iv * g[a];
    }
    dot = wave_sum(dot);
  }
  for (int e = l; e < cin * 16; e += 64) {
    const long a = ((long)(e >> 4) * cout + co) * 16 + (e & 15);
    g[a] = gain * iv * (g[a] - (inv ? w[a] * iv * dot : 0.f));
  }
}

}  // namespace

// ---- launchers (conv_plan.h): nblk blocks of 256 threads unless said otherwise ----
void launch_wprep_c7n(const float* wp, const float* sigma, bf16* wn, int cout, int nblk, hipStream_t s) {
  hipLaunchKernelGGL(weight_prep_c7n_kernel, dim3(nblk), dim3(256), 0, s, wp, sigma, wn, cout);
}

int launch_wprep(int dtype, const float* wp, const float* sigma, void* wk, int rows, int Kpad, int cout, int cin_valid,
                 int lgCin, int KS, int K, int transposed, int smaj, int nblk, hipStream_t s) {
  if (dtype == FV_BF16)
    hipLaunchKernelGGL(weight_prep_kernel<bf16>, dim3(nblk), dim3(256), 0, s, wp, sigma, (bf16*)wk, rows, Kpad, cout,
                       cin_valid, lgCin, KS, K, transposed, smaj);
  else if (dtype == FV_F32)
    hipLaunchKernelGGL(weight_prep_kernel<float>, dim3(nblk), dim3(256), 0, s, wp, sigma, (float*)wk, rows, Kpad, cout,
                       cin_valid, lgCin, KS, K, transposed, smaj);
  else return FV_E_UNSUPPORTED;
  return FV_OK;
}

int launch_wprep_s2t(int dtype, const float* wp, const float* sigma, void* wt, int rows, int Kph, int cout,
                     int cin_valid, int lgC, int nblk, hipStream_t s) {
  if (dtype == FV_BF16)
    hipLaunchKernelGGL(weight_prep_s2t_kernel<bf16>, dim3(nblk), dim3(256), 0, s, wp, sigma, (bf16*)wt, rows, Kph, cout,
                       cin_valid, lgC);
  else if (dtype == FV_F32)
    hipLaunchKernelGGL(weight_prep_s2t_kernel<float>, dim3(nblk), dim3(256), 0, s, wp, sigma, (float*)wt, rows, Kph, cout,
                       cin_valid, lgC);
  else return FV_E_UNSUPPORTED;
  return FV_OK;
}

int launch_wprep2(int dtype, const float* wp, const float* sigma, int cout, int cin_valid, int KS, const WPrepJob& j0,
                  const WPrepJob& j1, int nblk, hipStream_t s) {
  if (dtype == FV_BF16)
    hipLaunchKernelGGL(weight_prep2_kernel<bf16>, dim3(nblk), dim3(256), 0, s, wp, sigma, cout, cin_valid, KS, j0, j1);
  else if (dtype == FV_F32)
    hipLaunchKernelGGL(weight_prep2_kernel<float>, dim3(nblk), dim3(256), 0, s, wp, sigma, cout, cin_valid, KS, j0, j1);
  else return FV_E_UNSUPPORTED;
  return FV_OK;
}

int launch_wprep_multi(int dtype, const WPrepMulti& m, int nbx, hipStream_t s) {
  if (dtype == FV_BF16) hipLaunchKernelGGL(weight_prep_multi_kernel<bf16>, dim3(nbx, m.n), dim3(256), 0, s, m);
  else if (dtype == FV_F32) hipLaunchKernelGGL(weight_prep_multi_kernel<float>, dim3(nbx, m.n), dim3(256), 0, s, m);
  else return FV_E_UNSUPPORTED;
  return FV_OK;
}

void launch_wprep_subpix(const float* wp, const float* sigma, bf16* wk, int rows, int Kpad, int cout, int cin_valid,
                         int lgCin, int nblk, hipStream_t s) {
  hipLaunchKernelGGL(weight_prep_subpix_kernel<bf16>, dim3(nblk), dim3(256), 0, s, wp, sigma, wk, rows, Kpad, cout,
                     cin_valid, lgCin);
}

void launch_wprep_s2(const float* wp, const float* sigma, bf16* wt, int rows, int Kpad, int cout, int cin_valid,
                     int lgCt, int nblk, hipStream_t s) {
  hipLaunchKernelGGL(weight_prep_s2_kernel<bf16>, dim3(nblk), dim3(256), 0, s, wp, sigma, wt, rows, Kpad, cout,
                     cin_valid, lgCt);
}

int launch_wprep_phase(int mode, bool convt, const float* wp, const float* sigma, bf16* out, int rows, int units,
                       int cout, int cin_valid, int cpp, const float* cinv, float gain, int nblk, hipStream_t s) {
  if (mode == 1 && !convt)
    hipLaunchKernelGGL(weight_prep_phase_kernel<1>, dim3(nblk), dim3(256), 0, s, wp, sigma, out, rows, units, cout,
                       cin_valid, cpp, cinv, gain);
  else if (mode == 2 && !convt)
    hipLaunchKernelGGL(weight_prep_phase_kernel<2>, dim3(nblk), dim3(256), 0, s, wp, sigma, out, rows, units, cout,
                       cin_valid, cpp, cinv, gain);
  else if (mode == 1)
    hipLaunchKernelGGL((weight_prep_phase_kernel<1, true>), dim3(nblk), dim3(256), 0, s, wp, sigma, out, rows, units,
                       cout, cin_valid, cpp, cinv, gain);
  else if (mode == 2)
    hipLaunchKernelGGL((weight_prep_phase_kernel<2, true>), dim3(nblk), dim3(256), 0, s, wp, sigma, out, rows, units,
                       cout, cin_valid, cpp, cinv, gain);
  else return FV_E_UNSUPPORTED;
  return FV_OK;
}

// one wave (64 threads) per output channel: nblk = cout
void launch_convt_norm(const float* w, int cin, int cout, float* inv, int nblk, hipStream_t s) {
  hipLaunchKernelGGL(convt_norm_kernel, dim3(nblk), dim3(64), 0, s, w, cin, cout, inv);
}

void launch_convt_wprep(const float* w, const float* inv, float gain, bf16* wk, int rows, int Kpad, int lgCin, bf16* wt,
                        int rows_t, int lgCt, int cin_valid, int cout, int nblk, hipStream_t s) {
  hipLaunchKernelGGL(convt_weight_prep_kernel, dim3(nblk), dim3(256), 0, s, w, inv, gain, wk, rows, Kpad, lgCin, wt,
                     rows_t, lgCt, cin_valid, cout);
}

void launch_convt_wgrad_reduce(const float* slab, const float* bslab, float* dw, float* db, int nsplit, int CW, int KW,
                               int cout, int cin_valid, int lgCin, int nb_main, int nb_bias, hipStream_t s) {
  hipLaunchKernelGGL(convt_wgrad_reduce_kernel, dim3(nb_main + nb_bias), dim3(256), 0, s, slab, bslab, dw, db, nsplit,
                     CW, KW, cout, cin_valid, lgCin, nb_main);
}

// one wave (64 threads) per output channel: nblk = cout
void launch_convt_weight_bwd(const float* w, const float* inv, float gain, float* g, int cin, int cout, int nblk,
                             hipStream_t s) {
  hipLaunchKernelGGL(convt_weight_bwd_kernel, dim3(nblk), dim3(64), 0, s, w, inv, gain, g, cin, cout);
}
