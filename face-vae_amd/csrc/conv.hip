// Implicit-GEMM convolution for gfx950 (CDNA4): forward (+ backward-data via transposed
// weights) and backward-weight.  NHWC activations, MFMA 16x16x32 bf16 (fast mode) or
// 16x16x4 f32 (exact fp32 parity mode), fp32 accumulation.
//
// Reference behaviour replaced: F.conv2d as called by _ConvBlock / nn.Conv2d
// (modules.py:32-42; models.py:932-934, 1095-1099) in the FaceVAE path, plus the fused
// pieces around it (nearest x2 upsample modules.py:81, NAC BN-apply+act modules.py:13,
// residual add modules.py:125, sigmoid models.py:1110, BN statistics modules.py:19).
//
// Forward GEMM orientation:  D[co][pixel] = W[co][k] * im2col(x)[k][pixel]
//   MFMA A operand = weight tile (rows = output channels), B operand = activation tile
//   (cols = pixels).  The accumulator layout then gives each lane 4 consecutive output
//   channels of one pixel -> contiguous NHWC stores.  K = (tap, ci), ci fastest, chunks
//   of 8 k never straddle a tap (cin is a power of two >= 8).
//
// This file: weight preparation, the planners, the exported entries, the ConvTranspose block and
// the fp8 kernels; it holds no bf16 / fp32 forward kernel.  The generic forward kernels are in
// conv_fwd.hip and conv_fwd_v2.hip, the halo-staged 3x3 forwards in conv_halo3.hip, the
// special-shape forwards in conv_shapes.hip, the weight-gradient kernels and slab reductions in
// conv_wgrad.hip, reached through the launchers declared in conv_common.h and conv_plan.h with
// the helpers and types the files share.
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

// both layouts in one launch: blocks [0, nb1) write wk, the rest wt
struct WPrepJob { void* out; int rows, Kpad, lgCin, K, transposed, nb, smaj; };
template <typename T>
__global__ void weight_prep2_kernel(const float* __restrict__ wp, const float* sigma, int cout, int cin_valid, int KS,
                                    WPrepJob j0, WPrepJob j1) {
  const bool second = (int)blockIdx.x >= j0.nb;
  const WPrepJob& j = second ? j1 : j0;
  weight_prep_body<T>(wp, sigma, (T*)j.out, j.rows, j.Kpad, cout, cin_valid, j.lgCin, KS, j.K, j.transposed,
                      second ? blockIdx.x - j0.nb : blockIdx.x, j.nb, j.smaj);
}

// one launch for the generic weight layouts of many convs (fv_conv_weight_prep_multi): job j
// owns blocks [blk0, blk0 + nb); at most 2 * FV_WPREP_MAX jobs, passed by value
struct WPrepMJob {
  const float* w;
  const float* sigma;
  void* out;
  int rows, Kpad, lgCin, K, transposed, nb, cout, cin_valid, KS, blk0, smaj;
};
struct WPrepMulti {
  int n;
  WPrepMJob j[2 * FV_WPREP_MAX];
};
// grid (max nb, jobs): blockIdx.y selects the job directly (a per-block search over the job
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
// host dispatch
// ----------------------------------------------------------------------------------------
FwdTile fwd_tile(int rows_needed) {
  if (rows_needed > 64) return {128, 128};
  if (rows_needed > 32) return {64, 128};
  if (rows_needed > 16) return {32, 128};
  return {16, 128};
}

int pad_pow2_8(int c) {
  int p = 8;
  while (p < c) p <<= 1;
  return p;
}

// v2 (DMA-fed bf16) path: bf16, no BN prologue, cin a multiple of 64, input < 2 GB
bool use_v2(const fv_conv_desc* d) {
  if (d->dtype != FV_BF16 || d->pro_act || d->cin % 64) return false;
  if (d->out_nchw_f32 || d->epi_sigmoid || d->cout % 8 || d->ldy % 8) return false;   // staged NHWC epilogue
  if (d->w % 8) return false;   // a DMA piece (8 pixels) must lie in one image row
  const long hin = d->upsample ? d->h / 2 : d->h, win = d->upsample ? d->w / 2 : d->w;
  return (long)d->n * hin * win * d->cin * 2 < (1L << 31);
}

// 3x3 halo path (conv3_halo_fwd2 / fwd3): co per block (256 / 128 / 64), 0 when not eligible
int halo3_bn(const fv_conv_desc* d) {
  if (!use_v2(d) || d->ksize != 3 || d->upsample || d->w % 64 || d->h % 4) return 0;
  if ((long)d->n * d->h * d->w * d->ldy * 2 >= (1L << 31)) return 0;
  // co % 256: the pipelined pair-of-taps kernel (3 % over conv_fwd_v2's 256 x 256 tile on
  // the res convs) -- unless its 256-pixel x 256-co tiles leave CUs idle (fewer tiles than the
  // 256 CUs, e.g. the 64x64 latent convs at B <= 8: the SURVEY 8(f) path's Generator), where the
  // 128-co tiles double the grid.  Only for >= 256 input channels (the latent-resolution
  // convs), so AFE.down2 (128 -> 256) keeps one kernel at every batch size.
  if (d->cout % 256 == 0)
    return d->cin < 256 || (long)d->n * (d->h / 4) * (d->w / 64) * (d->cout / 256) >= 256 ? 256 : 128;
  // AFE.down1's forward (64 -> 128 channels, K = 576): conv_fwd_v2's 128 x 256 tile measured
  // 500 us against 543 (pipelined halo) / 579 (single-tap halo) at 256x256, B=32
  // (r3, stage-major weights: still 527 vs 503 us in alternating convbench runs)
  if (d->cin == 64 && d->cout == 128) return 0;
  return d->cout % 128 == 0 ? 128 : d->cout % 64 == 0 ? 64 : 0;
}


// v2 tile configs: id -> (co per block, pixels per block); waves/layout in launch_v2_ks
struct V2Cfg { int bn, bm; };
constexpr V2Cfg kV2Cfg[] = {
    {128, 128},   // 0: 4 waves 2x2, wave 64co x 64px
    {64, 256},    // 1: 4 waves 1x4, wave 64co x 64px
    {16, 256},    // 2: 4 waves 1x4, wave 16co x 64px
    {256, 256},   // 3: 8 waves 4x2, wave 64co x 128px
    {128, 256},   // 4: 8 waves 2x4, wave 64co x 64px
    {256, 128},   // 5: 8 waves 4x2, wave 64co x 64px
};
int v2_cfg(int rows_needed) {
  if (rows_needed % 256 == 0) return 3;
  if (rows_needed > 64) return 0;
  if (rows_needed > 16) return 1;
  return 2;
}
FwdTile fwd_tile_v2(int rows_needed) {
  const V2Cfg c = kV2Cfg[v2_cfg(rows_needed)];
  return {c.bn, c.bm};
}
// rows of a prepared weight image (forward wk: cout; data-gradient wt: cin): a whole number
// of co tiles of EVERY kernel that may read it -- the v1 tiles (fwd_tile) and the v2 tiles
// (fwd_tile_v2) differ for 17..32 rows (32 vs 64), and the v2 kernels' weight DMA reads the
// whole tile (found by a 1x1 32 -> 128 conv's data gradient reading 32 rows past its wt).
int wrows(int rows_needed) {
  const int b1 = fwd_tile(rows_needed).bn, b2 = fwd_tile_v2(rows_needed).bn;
  const int b = b1 > b2 ? b1 : b2;
  return fv_cdiv(rows_needed, b) * b;
}

// upsample + 3x3 conv as 4 sub-pixel phases of a 2x2 conv over the low-res input (bf16 v2
// path; FV_DISABLE_SUBPIX=1 keeps the folded-upsample 3x3 kernel).  2.25x fewer MACs than the
// reference formulation (reported utilisation still uses the reference FLOPs).
static int g_disable_subpix = -1;
bool use_subpix(const fv_conv_desc* d) {
  if (g_disable_subpix < 0) {
    const char* e = getenv("FV_DISABLE_SUBPIX");
    g_disable_subpix = (e && e[0] == '1') ? 1 : 0;
  }
  if (g_disable_subpix || !d->upsample || d->ksize != 3 || !use_v2(d)) return false;
  const int hl = d->h / 2, wl = d->w / 2;
  if (fv_ilog2(hl) < 0 || fv_ilog2(wl) < 0 || wl % 16) return false;
  const long pl = (long)d->n * hl * wl;
  return pl % fwd_tile_v2(d->cout).bm == 0;
}

// SIMD-partner schedule of the halo 3x3 kernels (conv3_halo_fwd3 / conv3_halo_fp8 SCH):
// FV_RES_SCHED = 0 (prio flips, lockstep), 1 (static prio for waves 4-7), 2 (stagger), 3
// (both); unset: the measured default of each kernel (dflt).  conv3_halo_fwd3 keeps 0 and 2
// (1 / 3 measured no better, below).  Read per call (tests compare the
// schedules bit for bit in one process).  r5, alternating convbench runs on one box, B=32 bf16
// res fwd / dgrad: 0: 130 / 122, 1: 124 / 118, 2: 120 / 115, 3: 126 / 119 us; B=64 fp8 res
// fwd / dgrad: 0: 175 / 166, 1: 173 / 163, 2: 172 / 155, 3: 165 / 155 us.
// data-parallel fp8 (fv_fp8_set_deferred_roll): the *_site convs leave the in-flight amax in the
// site; the caller all-reduces (MAX) every site's amax once per step and rolls them together
static int g_fp8_defer_roll = 0;

static int res_sched(int dflt) {
  const char* e = getenv("FV_RES_SCHED");
  return (e && e[0] >= '0' && e[0] <= '3') ? e[0] - '0' : dflt;
}

// data gradient of an upsample + 3x3 conv computed directly at the low resolution as a
// stride-2 4x4 conv over dy (bf16 v2 path; replaces dgrad at the high resolution followed by
// the 2x2 sum of fv_upsample2x_bwd: 0.44x the MACs, one pass fewer)
bool use_dgrad_lowres(const fv_conv_desc* d) {
  if (g_disable_subpix < 0) use_subpix(d);     // reads FV_DISABLE_SUBPIX
  if (g_disable_subpix || !d->upsample || d->ksize != 3 || d->dtype != FV_BF16) return false;
  const int ct = pad_pow2_8(d->cout);
  if (ct % 64 || d->cin % 8 || (d->w / 2) % 16) return false;
  return (long)d->n * d->h * d->w * ct * 2 < (1L << 31);
}

// UpBlock2D forward with a 128-channel input on the sliding-band kernel (conv3up_band_fwd).
// Its weights are the plain sub-pixel layout.
static bool use_upband(const fv_conv_desc* d) {
  if (d->dtype != FV_BF16 || !use_subpix(d)) return false;
  const int hl = d->h / 2, wl = d->w / 2;
  return d->cin == 128 && d->cin_valid == 128 && d->cout % 64 == 0 && wl % 32 == 0 && hl % 8 == 0 &&
         !d->out_nchw_f32 && !d->epi_sigmoid && !d->pro_act && d->ldy % 8 == 0 &&
         (long)d->n * hl * wl * 128 * 2 < (1L << 31) && (long)d->n * d->h * d->w * d->ldy * 2 < (1L << 31);
}
// the other UpBlock2D convs on the halo kernel (conv3_halo_fwd3 MODE 1 forward; MODE 2 low-res
// data gradient: dgrad_halo_bn); shapes outside these conditions run conv_fwd_v2 MODE 2 / 3
static bool use_subpix_halo(const fv_conv_desc* d) {
  if (!use_subpix(d) || use_upband(d)) return false;
  const int hl = d->h / 2, wl = d->w / 2;
  return d->cout % 64 == 0 && d->cin % 32 == 0 && d->cin >= 64 && d->cin_valid == d->cin && wl % 64 == 0 &&
         hl % 4 == 0 && !d->out_nchw_f32 && !d->epi_sigmoid && !d->pro_act && d->ldy % 8 == 0 &&
         (long)d->n * hl * wl * d->cin * 2 < (1L << 31) && (long)d->n * d->h * d->w * d->ldy * 2 < (1L << 31);
}
// co tile (256 / 128 rows) of the low-res data gradient on the halo kernel, 0 = not on it
static int dgrad_halo_bn(const fv_conv_desc* d) {
  if (!use_dgrad_lowres(d)) return 0;
  const int hl = d->h / 2, wl = d->w / 2;
  if (pad_pow2_8(d->cout) != d->cout || d->cout % 32 || wl % 64 || hl % 4 || d->cin_valid != d->cin) return 0;
  if ((long)d->n * d->h * d->w * d->cout * 2 >= (1L << 31)) return 0;
  return d->cin % 256 == 0 ? 256 : d->cin % 128 == 0 ? 128 : 0;
}
// elements of the phase weight images (weight_prep_phase_kernel): the one size both the
// queries and the launches use
static long phase_wk_elems(const fv_conv_desc* d) { return 4L * (d->cin / 32) * 4 * d->cout * 32; }
static long phase_wt_elems(const fv_conv_desc* d) { return 4L * (4 * d->cout / 32) * d->cin * 32; }

// Generator.out_conv shape: 7x7, 64 -> <= 4 channels, NCHW fp32 output (bf16 operands)
bool use_c7n(const fv_conv_desc* d) {
  return d->dtype == FV_BF16 && d->ksize == 7 && d->cin == 64 && d->cin_valid == 64 &&
         d->cout <= 4 && !d->pro_act && !d->upsample && d->w % 64 == 0 && d->h % C7_TR == 0 &&
         (long)d->n * d->h * d->w * 64 * 2 < (1L << 31);
}

// band of output rows per block of the sliding out_conv forward (conv7_n3_fwd2): the largest
// of 128/64/32/16/8/4 dividing H that still gives >= 256 blocks (else the smallest dividing;
// use_c7n guarantees H % 4 == 0).  FV_C7_BAND=b forces a band (tests: multi-group rings on
// small images); read per call.
static int c7n_band(const fv_conv_desc* d) {
  if (const char* e = getenv("FV_C7_BAND")) {
    const int b = atoi(e);
    if (b >= 4 && b % 4 == 0 && d->h % b == 0) return b;
  }
  int pick = 0;
  for (int band : {128, 64, 32, 16, 8, 4}) {
    if (d->h % band) continue;
    pick = band;
    if ((long)d->n * (d->w / 64) * (d->h / band) >= 256) return band;
  }
  return pick;
}

// 3x3 weight gradient with the halo-staged input, rows sliding down a segment
// (conv3_halo_wgrad2; its tile-per-row-segment predecessor ran 518 us against 262 us for
// AFE.down1)
bool use_h3w(const fv_conv_desc* d) {
  // measured against conv_wgrad_v2 (tools/convbench.py): 12 % faster on AFE.down1 (64 -> 128,
  // whose v2 tile is 128 x 128).  Wider inputs run it as 64-channel input tiles (r4: the res /
  // down2 weight gradients)
  // (a BN-apply prologue runs the generic kernels)
  if (d->pro_act) return false;
  return d->dtype == FV_BF16 && d->ksize == 3 && !d->upsample && d->cin % 64 == 0 &&
         d->cin_valid == d->cin && d->cout % 128 == 0 && d->w % 64 == 0;
}

// out_conv weight gradient as "row taps in N" (conv7_n3_wgrad)
bool use_c7w(const fv_conv_desc* d) {
  return d->dtype == FV_BF16 && d->ksize == 7 && d->cin == 64 && d->cin_valid == 64 &&
         d->cout <= 4 && !d->pro_act && !d->upsample && d->w % 64 == 0 &&
         (long)d->n * d->h * d->w * 64 * 2 < (1L << 31);
}

int check_desc(const fv_conv_desc* d) {
  FV_REQUIRE(d, "null conv descriptor");
  FV_REQUIRE(d->dtype == FV_F32 || d->dtype == FV_BF16, "conv dtype must be f32 or bf16");
  FV_REQUIRE(d->ksize == 1 || d->ksize == 3 || d->ksize == 7, "ksize must be 1, 3 or 7");
  FV_REQUIRE(d->n > 0 && d->h > 0 && d->w > 0, "bad spatial size");
  FV_REQUIRE(fv_ilog2(d->cin) >= 3, "cin must be a power of two >= 8 (got %d)", d->cin);
  FV_REQUIRE(d->cin_valid > 0 && d->cin_valid <= d->cin, "bad cin_valid");
  FV_REQUIRE(d->cout > 0, "bad cout");
  FV_REQUIRE(!d->upsample || (d->h % 2 == 0 && d->w % 2 == 0), "upsample needs even h, w");
  FV_REQUIRE(!d->upsample || d->ksize == 3, "upsample only with 3x3");
  FV_REQUIRE(!d->pro_act || d->ksize != 7, "BN prologue not supported for 7x7");
  FV_REQUIRE(!d->pro_act || fv_slope_ok(d->pro_slope), "prologue slope must be in [0, 1] (got %g)", (double)d->pro_slope);
  return FV_OK;
}

int kpad_of(int ks, int cin) { return fv_cdiv((long)ks * ks * cin, BK) * BK; }

// 7x7 halo wgrad: in_conv (cin 8 -> 64, dy stride 64) or out_conv (cin 64 -> cout <= 8, dy stride 8)
// the in_conv weight gradient in the packed k layout (conv_halo_wgrad PK); FV_WG7_PACK=0 keeps
// the 8-channel padded layout (A/B).  Read per call.
static bool halo_wg_pk(const fv_conv_desc* d) {
  const char* e = getenv("FV_WG7_PACK");
  if (e && e[0] == '0') return false;
  return d->ksize == 7 && d->cin == 8 && d->cin_valid <= 4;
}
static int halo_wg_tr(const fv_conv_desc* d) {
  if (d->ksize != 7 || d->upsample || d->pro_act || d->w % 64) return 0;
  int tr = 0;
  if (d->cin == 8 && d->cout == 64) tr = 4;
  else if (d->cin == 64 && d->cout <= 8) tr = 2;
  return (tr && d->h % tr == 0) ? tr : 0;
}

int wg2_cfg(const fv_conv_desc* d, int K) {
  const int bc = d->cout > 128 ? 256 : d->cout > 64 ? 128 : d->cout > 16 ? 64 : 16;
  // defaults from the FaceVAE-shape tile sweep (r1): 384 x 64 tiles for the
  // 64-channel layers (K = 1152 splits exactly), 32-pixel stages 3-deep when K is not a
  // multiple of 256 at 256 channels
  if (bc == 16) return 5;
  if (bc == 64) return (K % 384 == 0 && d->w % 64 == 0) ? 7 : 4;
  const bool k256 = fv_cdiv(K, 256) * 256 <= fv_cdiv(K, 128) * 128;
  // (r3, alternating convbench runs on one box, res wgrad at B=32: cfg 0 150-153 us, cfg 6
  // (32-pixel stages, 3 in flight) 168, cfg 1 (128 x 256 tiles, 3 stages) 202-207)
  if (bc == 256) return K % 256 == 0 ? 0 : (d->ksize == 3 && d->w % 32 == 0 ? 6 : 1);
  return k256 ? 2 : 3;
}
// UpBlock2D weight gradient on conv3_up_wgrad: bf16 nearest-x2 + 3x3, 64-channel multiples,
// 64-column output strips (other shapes: the conv_wgrad_v2 sub-pixel path)
static bool use_upw(const fv_conv_desc* d) {
  return d->dtype == FV_BF16 && d->upsample && d->ksize == 3 && !d->pro_act && d->cin % 64 == 0 &&
         d->cin_valid == d->cin && d->cout % 64 == 0 && d->w % 64 == 0 && d->h % 4 == 0;
}

WgPlan plan_wgrad(const fv_conv_desc* d) {
  WgPlan p{};
  const int K = d->ksize * d->ksize * d->cin;
  const long P = (long)d->n * d->h * d->w;
  const long hin = d->upsample ? d->h / 2 : d->h, win = d->upsample ? d->w / 2 : d->w;
  // 32-bit buffer offsets: x and dy (channel stride = cout padded to a power of two >= 8, as
  // every caller passes; fv_conv2d_bwd_weight re-checks the real stride) must stay < 2 GB
  const bool fits = d->dtype == FV_BF16 && (long)d->n * hin * win * d->cin * 2 < (1L << 31) &&
                   P * pad_pow2_8(d->cout) * 2 < (1L << 31);
  p.v2 = fits && !d->pro_act;
  // out_conv 7x7 64 -> <= 4 (v2 == 3): blocks = (image, 64-column strip, row segment), about
  // 2 per CU (r6: 1024 -> 512 blocks halves the 58.7 MB of slabs; out_conv weight gradient
  // 98.4 -> 90.4 us + reduce 15 -> 10.6 us, step -0.03 ms; 256 blocks: 114 us;
  // profiles/r6/r6k_ab_wgrad_blocks.log); slab [block][32 (r, co)][448 (s, ci)]
  if (p.v2 && use_c7w(d)) {
    const int strips = d->w / 64;
    int nseg = fv_cdiv(512, d->n * strips);
    if (nseg > fv_cdiv(d->h, 8)) nseg = fv_cdiv(d->h, 8);
    if (nseg < 1) nseg = 1;
    p.v2 = 3;
    p.sps = fv_cdiv(d->h, nseg);                 // rows per segment
    p.nsteps = fv_cdiv(d->h, p.sps);             // segments
    p.nsplit = d->n * strips * p.nsteps;
    p.CW = 32;
    p.KW = 448;
    p.ntk = p.ntc = 1;
    return p;
  }
  // 3x3 sliding-row wgrad (v2 == 5, conv3_halo_wgrad2): blocks = (image, 64-column strip,
  // row segment) x co tiles of 128, ~1 block per CU; splits = image x strip x segment
  if (fits && use_h3w(d)) {
    const int strips = d->w / 64;
    p.v2 = 5;
    p.ntc = d->cout / 128;
    p.ntk = d->cin / 64;               // 64-channel input tiles
    int nseg = (256 / (p.ntc * p.ntk) + d->n * strips / 2) / (d->n * strips);
    if (nseg < 1) nseg = 1;
    if (nseg > d->h / 4) nseg = d->h / 4 > 0 ? d->h / 4 : 1;
    p.sps = fv_cdiv(d->h, nseg);                  // rows per segment
    p.nsteps = fv_cdiv(d->h, p.sps);              // segments
    p.nsplit = d->n * strips * p.nsteps;
    p.CW = d->cout;
    p.KW = K;
    return p;
  }
  // 7x7 halo path (v2 == 2): one persistent block per CU, ntk = 1 (all k in one tile)
  const int htr = halo_wg_tr(d);
  if (p.v2 && htr) {
    const int nt = d->cin == 8 ? 4 : 1;
    p.v2 = 2;
    p.bkt = halo_wg_pk(d) ? 7 * 32 : fv_cdiv(K, 16) * 16;
    p.bc = nt * 16;
    p.px = htr * 64;
    p.ntk = 1;
    p.ntc = 1;
    p.nsteps = (int)(P / p.px);                  // pixel tiles
    p.nsplit = p.nsteps < 256 ? p.nsteps : 256;  // persistent blocks
    p.sps = fv_cdiv(p.nsteps, p.nsplit);
    p.KW = p.bkt;
    p.CW = p.bc;
    return p;
  }
  if (fits && use_upw(d)) {
    // sub-pixel sliding-row weight gradient (v2 == 6, conv3_up_wgrad): blocks = (co tile, ci
    // tile) x splits of `sps` consecutive (image, 64-column output strip) units, ~one block per
    // CU; slab [phase][split][co][4 cin] as the v2 sub-pixel path
    p.sub = 1;
    p.v2 = 6;
    p.ntc = d->cout / 64;
    p.ntk = d->cin / 64;
    const int units = d->n * (d->w / 64), tiles = p.ntc * p.ntk;
    p.sps = (units * tiles + 128) / 256;
    // FV_UPW_SPB=k: k units per block (tests: ragged last split at small shapes)
    if (const char* e = getenv("FV_UPW_SPB")) p.sps = atoi(e);
    if (p.sps < 1) p.sps = 1;
    p.nsteps = units;
    p.nsplit = fv_cdiv(units, p.sps);
    p.CW = d->cout;
    p.KW = 4 * d->cin;
    return p;
  }
  if (p.v2 && use_subpix(d) && (d->w / 2) % 64 == 0) {
    // weight gradient of the 4 sub-pixel phases (2x2 taps over the low-res input, 0.44x the
    // MACs of the upsampled 3x3 formulation); wgrad_reduce folds the phases back into 3x3
    p.sub = 1;
    p.cfg = d->cout > 64 ? (d->cout > 128 ? 0 : 2) : 8;
    const Wg2Cfg& c = kWg2Cfg[p.cfg];
    p.bkt = c.bkt;
    p.bc = c.bc;
    p.px = c.px;
    const int K2 = 4 * d->cin;
    const long P2 = (long)d->n * (d->h / 2) * (d->w / 2);
    p.ntk = fv_cdiv(K2, p.bkt);
    p.ntc = fv_cdiv(d->cout, p.bc);
    p.nsteps = (int)(P2 / p.px);
    const int ntile = p.ntk * p.ntc;
    int ns = (64 + ntile / 2) / ntile;         // x4 phases ~ one block per CU
    if (ns < 1) ns = 1;
    if (ns > p.nsteps) ns = p.nsteps;
    p.sps = fv_cdiv(p.nsteps, ns);
    p.nsplit = fv_cdiv(p.nsteps, p.sps);
    p.KW = p.ntk * p.bkt;
    p.CW = p.ntc * p.bc;
    return p;
  }
  if (p.v2) {
    p.cfg = wg2_cfg(d, K);
    const Wg2Cfg& c = kWg2Cfg[p.cfg];
    p.bkt = c.bkt;
    p.bc = c.bc;
    p.px = c.px;
  } else {
    p.bc = d->cout > 64 ? 128 : (d->cout > 16 ? 64 : 16);
    p.bkt = 128;
    p.px = 32;
  }
  p.ntk = fv_cdiv(K, p.bkt);
  p.ntc = fv_cdiv(d->cout, p.bc);
  p.nsteps = fv_cdiv(P, p.px);
  const int ntile = p.ntk * p.ntc;
  // v2: about 256 blocks (128: 1x1 weight gradients 45 / 33 -> 67 / 40 us)
  int ns = p.v2 ? (256 + ntile / 2) / ntile : 768 / ntile;
  if (ns < 1) ns = 1;
  if (ns > p.nsteps) ns = p.nsteps;
  p.sps = fv_cdiv(p.nsteps, ns);
  p.nsplit = fv_cdiv(p.nsteps, p.sps);
  p.KW = p.ntk * p.bkt;
  p.CW = p.ntc * p.bc;
  return p;
}

// the weight gradient's plan: the generic kernel's tiles (plan_wgrad's fp32 branch) for both dtypes
WgPlan plan_wgrad_s2(const fv_conv_desc* d) {
  WgPlan p{};
  const int K = 9 * d->cin;
  const long P = (long)d->n * d->h * d->w;
  p.bc = d->cout > 64 ? 128 : (d->cout > 16 ? 64 : 16);
  p.bkt = 128;
  p.px = 32;
  p.ntk = fv_cdiv(K, p.bkt);
  p.ntc = fv_cdiv(d->cout, p.bc);
  p.nsteps = fv_cdiv(P, p.px);
  const int ntile = p.ntk * p.ntc;
  int ns = 768 / ntile;
  if (ns < 1) ns = 1;
  if (ns > p.nsteps) ns = p.nsteps;
  p.sps = fv_cdiv(p.nsteps, ns);
  p.nsplit = fv_cdiv(p.nsteps, p.sps);
  p.KW = p.ntk * p.bkt;
  p.CW = p.ntc * p.bc;
  return p;
}
// descriptor and size checks shared by the fv_conv2d_s2_* entries
int check_s2(const fv_conv_desc* d) {
  int st = check_desc(d);
  if (st) return st;
  if (d->ksize != 3 || d->upsample || d->pro_act || d->epi_sigmoid || d->out_nchw_f32) {
    fv_set_error("stride-2 conv: 3x3, no upsample / BN prologue / sigmoid / NCHW output");
    return FV_E_UNSUPPORTED;
  }
  FV_REQUIRE(4L * d->n * d->h * d->w < (1L << 31), "stride-2 conv: more than 2^31 input pixels");
  return FV_OK;
}
int check_s2_in(const fv_conv_desc* d, int in_h, int in_w) {
  if (in_h != 2 * d->h || in_w != 2 * d->w) {
    fv_set_error("stride-2 conv: the input must be (2h, 2w) = %d x %d for a %d x %d output, odd sizes are not "
                 "supported (got %d x %d)", 2 * d->h, 2 * d->w, d->h, d->w, in_h, in_w);
    return FV_E_UNSUPPORTED;
  }
  return FV_OK;
}

}  // namespace

extern "C" {

size_t fv_conv_wk_elems(const fv_conv_desc* d) {
  if (check_desc(d) != FV_OK) return 0;
  const size_t rows = (size_t)wrows(d->cout);
  if (use_c7n(d)) return 32 * 448;
  if (use_subpix_halo(d)) return (size_t)phase_wk_elems(d);
  if (use_subpix(d)) return 4 * rows * kpad_of(2, d->cin);
  return rows * kpad_of(d->ksize, d->cin);
}

size_t fv_conv_wt_elems(const fv_conv_desc* d) {
  if (check_desc(d) != FV_OK) return 0;
  const int cin_t = pad_pow2_8(d->cout);
  const size_t rows = (size_t)wrows(d->cin);
  if (dgrad_halo_bn(d)) return (size_t)phase_wt_elems(d);
  if (use_dgrad_lowres(d)) return rows * 16 * cin_t;
  return rows * kpad_of(d->ksize, cin_t);
}

int fv_conv2d_dgrad_lowres(const fv_conv_desc* d) {
  if (check_desc(d) != FV_OK) return 0;
  return use_dgrad_lowres(d) ? 1 : 0;
}

// 7x7 halo path: (cin 8 -> cout 64, TR 8, weights in LDS) or (cin 64 -> cout <= 16, TR 2)
static int halo_tr(const fv_conv_desc* d) {
  if (d->dtype != FV_BF16 || d->ksize != 7 || d->pro_act || d->upsample || d->w % 64) return 0;
  int tr = 0;
  // (8-row tiles for the 8-channel side, 16 MFMAs per 8 LDS reads per wave, measured 13.28 ->
  // 13.33 ms/step in an A/B: not kept)
  if (d->cin == 8 && d->cout == 64) tr = 4;
  else if (d->cin == 64 && d->cout <= 16) tr = 2;
  if (!tr || d->h % tr) return 0;
  if ((long)d->n * d->h * d->w * d->cin * 2 >= (1L << 31)) return 0;
  return tr;
}

// the launch of forward-conv descriptor fd runs conv7c4_fwd (packed 7x7 weights, smaj 2)
static bool use_c74(const fv_conv_desc* fd) {
  return halo_tr(fd) == 4 && fd->cin == 8 && fd->cin_valid <= 4 && fd->cout == 64 && fd->ldy == 64 &&
         !fd->epi_sigmoid && !fd->out_nchw_f32;
}
// conv7c4_fwd's persistent grid: G blocks (<= 512, two per CU) of c74_tiles_per_block tiles
// each (block b: tiles b, b + G, ...); G = the BN record count (one record per block)
static int c74_tiles_per_block(const fv_conv_desc* d) {
  const int ntiles = d->n * (d->h / C74_TR) * (d->w / 64);
  return fv_cdiv(ntiles, 512);
}
static int c74_grid(const fv_conv_desc* d) {
  return fv_cdiv(d->n * (d->h / C74_TR) * (d->w / 64), c74_tiles_per_block(d));
}
// the launch of forward-conv descriptor fd runs conv3c64_fwd (64 input channels, sliding band,
// weights in registers; plain [co][Kpad] weights)
static bool use_c64(const fv_conv_desc* fd) {
  return fd->dtype == FV_BF16 && fd->ksize == 3 && !fd->upsample && !fd->pro_act && fd->cin == 64 &&
         fd->cin_valid == 64 && fd->cout % 64 == 0 && fd->ldy % 8 == 0 && !fd->epi_sigmoid && !fd->out_nchw_f32 &&
         fd->w % 64 == 0 && fd->h % 32 == 0 && (long)fd->n * fd->h * fd->w * 64 * 2 < (1L << 31) &&
         (long)fd->n * fd->h * fd->w * fd->ldy * 2 < (1L << 31);
}
// bands per (image, strip, 64-channel group): about one block per CU, bands of 32k rows
static int c64_bands(const fv_conv_desc* d) {
  const long base = (long)d->n * (d->w / 64) * (d->cout / 64);
  int nb = 1;
  while (base * nb < 256 && d->h % (nb * 64) == 0) nb *= 2;
  return nb;
}
static FwdTile plan_tile(const fv_conv_desc* d) {
  const int tr = halo_tr(d);
  if (tr) return {d->cout <= 16 ? 16 : 64, tr * 64};
  return use_v2(d) ? fwd_tile_v2(d->cout) : fwd_tile(d->cout);
}

// pixels per BN-statistics record = the pixels of one wave row of the tile (BM / WM)
static int stats_record_pixels(const fv_conv_desc* d) {
  if (use_c7n(d)) return 64;
  if (use_upband(d)) return UPB_G * 2 * 32;                  // (block, 4 iterations, phase)
  if (use_subpix_halo(d)) return 128;                         // (tile, wave row, phase): RM * 16                                  // one 64-pixel row segment
  if (use_c74(d)) return c74_tiles_per_block(d) * C74_TR * 64;   // one record per block
  if (use_c64(d)) return C64_G * 64;                          // 8 iterations x one wave's row
  if (halo_tr(d)) return plan_tile(d).bm / 8;                 // 8 waves stacked over pixels
  const FwdTile t = plan_tile(d);
  if (const int bn = halo3_bn(d)) return bn == 256 ? 128 : 64;   // RM * 16 pixels per wave row
  if (use_v2(d)) {
    if (t.bn == 64 || t.bn == 16 || (t.bn == 128 && t.bm == 256)) return t.bm / 4;
    return t.bm / 2;                                          // 128x128, 256x256, 256x128
  }
  return t.bn == 16 ? t.bm / 4 : t.bm / 2;                    // v1 layouts (launch_fwd_ks)
}

int fv_conv2d_stats_block_pixels(const fv_conv_desc* d) {
  if (check_desc(d) != FV_OK) return 0;
  return stats_record_pixels(d);
}

int fv_conv2d_stats_blocks(const fv_conv_desc* d) {
  if (check_desc(d) != FV_OK) return 0;
  return fv_cdiv((long)d->n * d->h * d->w, stats_record_pixels(d));
}

static fv_conv_desc dgrad_desc(const fv_conv_desc* d);

// the launch of forward-conv descriptor fd runs a halo 3x3 kernel (conv_run's halo3 branch:
// conv3_halo_fwd3 / fwd2), whose weights are prepared stage-major (weight_prep_body smaj) with
// wk_rows(fd) rows per tap unit
static bool h3s_layout(const fv_conv_desc* fd) {
  return !use_c7n(fd) && !halo_tr(fd) && !use_subpix(fd) && !use_c64(fd) && halo3_bn(fd) != 0;
}
static int wk_rows(const fv_conv_desc* fd) {
  return wrows(fd->cout);
}
static int lay_of(const fv_conv_desc* fd) { return use_c74(fd) ? 2 : h3s_layout(fd) ? 1 : 0; }
// ... for the forward weights (wk) and the data gradient's transposed weights (wt) of conv d
static int smaj_wk(const fv_conv_desc* d) { return lay_of(d); }
static int smaj_wt(const fv_conv_desc* d) {
  if (use_dgrad_lowres(d)) return 0;
  const fv_conv_desc t = dgrad_desc(d);
  return lay_of(&t);
}
// row length of a prepared image: the packed 7x7 layout's rows are C74_K long
static int kpad_lay(int lay, int kpad) { return lay == 2 ? C74_K : kpad; }

int fv_conv_weight_prep(const fv_conv_desc* d, const float* w_param, const float* sigma, void* wk,
                        void* wt, void* stream) {
  int st = check_desc(d);
  if (st) return st;
  hipStream_t s = (hipStream_t)stream;
  const int ks = d->ksize;
  const bool generic_wk = wk && !use_c7n(d) && !use_subpix(d);
  const bool generic_wt = wt && !use_dgrad_lowres(d);
  if (generic_wk && generic_wt) {
    // the common case: forward and transposed layouts in one launch
    const int cin_t = pad_pow2_8(d->cout);
    WPrepJob j0{wk, wrows(d->cout), kpad_lay(smaj_wk(d), kpad_of(ks, d->cin)), fv_ilog2(d->cin),
                ks * ks * d->cin, 0, 0, smaj_wk(d)};
    WPrepJob j1{wt, wrows(d->cin), kpad_lay(smaj_wt(d), kpad_of(ks, cin_t)), fv_ilog2(cin_t),
                ks * ks * cin_t, 1, 0, smaj_wt(d)};
    j0.nb = (int)std::min<long>(fv_cdiv((long)j0.rows * j0.Kpad, 256), 4096);
    j1.nb = (int)std::min<long>(fv_cdiv((long)j1.rows * j1.Kpad, 256), 4096);
    if (d->dtype == FV_BF16)
      hipLaunchKernelGGL(weight_prep2_kernel<bf16>, dim3(j0.nb + j1.nb), dim3(256), 0, s, w_param, sigma, d->cout,
                         d->cin_valid, ks, j0, j1);
    else
      hipLaunchKernelGGL(weight_prep2_kernel<float>, dim3(j0.nb + j1.nb), dim3(256), 0, s, w_param, sigma, d->cout,
                         d->cin_valid, ks, j0, j1);
    return fv_check_launch("weight_prep2");
  }
  if (wk && use_c7n(d)) {
    hipLaunchKernelGGL(weight_prep_c7n_kernel, dim3(56), dim3(256), 0, s, w_param, sigma, (bf16*)wk, d->cout);
    if ((st = fv_check_launch("weight_prep_c7n"))) return st;
  } else if (wk && use_subpix_halo(d)) {
    const int nb = (int)std::min<long>(fv_cdiv(phase_wk_elems(d), 256), 4096);
    hipLaunchKernelGGL(weight_prep_phase_kernel<1>, dim3(nb), dim3(256), 0, s, w_param, sigma, (bf16*)wk,
                       4 * d->cout, 4 * (d->cin / 32), d->cout, d->cin_valid, 0);
    if ((st = fv_check_launch("weight_prep_phase1"))) return st;
  } else if (wk && use_subpix(d)) {
    const int rows = wrows(d->cout), Kp = kpad_of(2, d->cin);
    const long tot = 4L * rows * Kp;
    const int nb = (int)std::min<long>(fv_cdiv(tot, 256), 4096);
    hipLaunchKernelGGL(weight_prep_subpix_kernel<bf16>, dim3(nb), dim3(256), 0, s, w_param, sigma, (bf16*)wk, rows, Kp,
                       d->cout, d->cin_valid, fv_ilog2(d->cin));
    if ((st = fv_check_launch("weight_prep_subpix"))) return st;
  } else if (wk) {
    const int rows = wrows(d->cout), Kp = kpad_lay(smaj_wk(d), kpad_of(ks, d->cin));
    const long tot = (long)rows * Kp;
    const int nb = (int)std::min<long>(fv_cdiv(tot, 256), 4096);
    if (d->dtype == FV_BF16)
      hipLaunchKernelGGL(weight_prep_kernel<bf16>, dim3(nb), dim3(256), 0, s, w_param, sigma, (bf16*)wk,
                         rows, Kp, d->cout, d->cin_valid, fv_ilog2(d->cin), ks, ks * ks * d->cin, 0, smaj_wk(d));
    else
      hipLaunchKernelGGL(weight_prep_kernel<float>, dim3(nb), dim3(256), 0, s, w_param, sigma, (float*)wk,
                         rows, Kp, d->cout, d->cin_valid, fv_ilog2(d->cin), ks, ks * ks * d->cin, 0, 0);
    if ((st = fv_check_launch("weight_prep"))) return st;
  }
  if (wt && dgrad_halo_bn(d)) {
    const int nb = (int)std::min<long>(fv_cdiv(phase_wt_elems(d), 256), 4096);
    hipLaunchKernelGGL(weight_prep_phase_kernel<2>, dim3(nb), dim3(256), 0, s, w_param, sigma, (bf16*)wt, d->cin,
                       4 * (4 * d->cout / 32), d->cout, d->cin_valid, d->cout / 32);
    if ((st = fv_check_launch("weight_prep_phase2"))) return st;
  } else if (wt && use_dgrad_lowres(d)) {
    const int cin_t = pad_pow2_8(d->cout);
    const int rows = wrows(d->cin), Kp = 16 * cin_t;
    const long tot = (long)rows * Kp;
    const int nb = (int)std::min<long>(fv_cdiv(tot, 256), 4096);
    hipLaunchKernelGGL(weight_prep_s2_kernel<bf16>, dim3(nb), dim3(256), 0, s, w_param, sigma, (bf16*)wt, rows, Kp,
                       d->cout, d->cin_valid, fv_ilog2(cin_t));
    if ((st = fv_check_launch("weight_prep_s2"))) return st;
  } else if (wt) {
    const int cin_t = pad_pow2_8(d->cout);
    const int rows = wrows(d->cin), Kp = kpad_lay(smaj_wt(d), kpad_of(ks, cin_t));
    const long tot = (long)rows * Kp;
    const int nb = (int)std::min<long>(fv_cdiv(tot, 256), 4096);
    if (d->dtype == FV_BF16)
      hipLaunchKernelGGL(weight_prep_kernel<bf16>, dim3(nb), dim3(256), 0, s, w_param, sigma, (bf16*)wt,
                         rows, Kp, d->cout, d->cin_valid, fv_ilog2(cin_t), ks, ks * ks * cin_t, 1, smaj_wt(d));
    else
      hipLaunchKernelGGL(weight_prep_kernel<float>, dim3(nb), dim3(256), 0, s, w_param, sigma, (float*)wt,
                         rows, Kp, d->cout, d->cin_valid, fv_ilog2(cin_t), ks, ks * ks * cin_t, 1, 0);
    if ((st = fv_check_launch("weight_prep_t"))) return st;
  }
  return FV_OK;
}

int fv_conv_weight_prep_batchable(const fv_conv_desc* d) {
  if (check_desc(d) != FV_OK) return 0;
  return !use_c7n(d) && !use_subpix(d) && !use_dgrad_lowres(d);
}

int fv_conv_weight_prep_multi(int n, const fv_conv_desc* descs, const float* const* w_params,
                              const float* const* sigmas, void* const* wks, void* const* wts, void* stream) {
  FV_REQUIRE(n >= 1 && n <= FV_WPREP_MAX && descs && w_params && sigmas && wks && wts, "weight_prep_multi: bad args");
  WPrepMulti m{};
  int nb_total = 0;
  const int dtype = descs[0].dtype;
  for (int i = 0; i < n; ++i) {
    const fv_conv_desc* d = &descs[i];
    int st = check_desc(d);
    if (st) return st;
    FV_REQUIRE(d->dtype == dtype, "weight_prep_multi: one dtype per call");
    FV_REQUIRE(fv_conv_weight_prep_batchable(d), "weight_prep_multi: conv %d needs a special layout", i);
    FV_REQUIRE(w_params[i] && wks[i], "weight_prep_multi: null pointer (conv %d)", i);
    const int ks = d->ksize;
    WPrepMJob j0{w_params[i], sigmas[i], wks[i], wrows(d->cout), kpad_lay(smaj_wk(d), kpad_of(ks, d->cin)),
                 fv_ilog2(d->cin),
                 ks * ks * d->cin, 0, 0, d->cout, d->cin_valid, ks, 0, smaj_wk(d)};
    j0.nb = (int)std::min<long>(fv_cdiv((long)j0.rows * j0.Kpad, 256), 256);
    nb_total = std::max(nb_total, j0.nb);
    m.j[m.n++] = j0;
    if (wts[i]) {
      const int cin_t = pad_pow2_8(d->cout);
      WPrepMJob j1{w_params[i], sigmas[i], wts[i], wrows(d->cin), kpad_lay(smaj_wt(d), kpad_of(ks, cin_t)),
                   fv_ilog2(cin_t),
                   ks * ks * cin_t, 1, 0, d->cout, d->cin_valid, ks, 0, smaj_wt(d)};
      j1.nb = (int)std::min<long>(fv_cdiv((long)j1.rows * j1.Kpad, 256), 256);
      nb_total = std::max(nb_total, j1.nb);
      m.j[m.n++] = j1;
    }
  }
  hipStream_t s = (hipStream_t)stream;
  if (dtype == FV_BF16)
    hipLaunchKernelGGL(weight_prep_multi_kernel<bf16>, dim3(nb_total, m.n), dim3(256), 0, s, m);
  else
    hipLaunchKernelGGL(weight_prep_multi_kernel<float>, dim3(nb_total, m.n), dim3(256), 0, s, m);
  return fv_check_launch("weight_prep_multi");
}

// store-pass record geometry (fv_store_reduce) of the launch `d` takes: records and pixels per
// record, 0 when that path has none.  The halo-staged 3x3 kernels only: 256-pixel tiles of 8
// waves (co tiles of 256 / 128) or 4 waves (co tiles of 64), one record per (tile, wave).
static int sr_geometry(const fv_conv_desc* d, int* bp) {
  if (d->dtype != FV_BF16 || use_c7n(d) || halo_tr(d) || use_subpix(d) || use_c64(d)) return 0;
  const int bn = halo3_bn(d);
  const long P = (long)d->n * d->h * d->w;
  if (!bn || d->cout % bn || P % 256) return 0;
  const int nw = bn == 64 ? 4 : 8;
  if (bp) *bp = 256 / nw;
  return (int)(P / 256 * nw);
}

extern "C++" {
// CUs of the current device (persistent grids), queried once
static int cu_count() {
  static int n = 0;
  if (!n) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        n <= 0)
      n = 256;
  }
  return n;
}
// What conv_epilogue's HALO form (conv3_halo_fwd2 / fwd3 MODE 0 and 2) takes for granted, checked
// next to every such launch: tiles of tr whole 64-pixel row segments and bn channels cover the
// N x H x W x Cout output exactly and store to it in place (no sub-pixel phase, NHWC), so that
// no stored element needs a bounds test (P % (tr * 64) == 0 and Cout % bn == 0 follow)
static bool halo_epi_ok(const ConvArgs& a, int bn, int tr) {
  return a.lgtw == 6 && !a.sub && !a.nchw && a.W % 64 == 0 && a.H % tr == 0 && a.P == a.N * a.H * a.W &&
         a.ntn * bn == a.Cout && a.ldy >= a.Cout;
}
// one conv3_halo_fwd3 launch over ntiles tiles: schedule SCH 2 (stagger) unless FV_RES_SCHED
// says 0 / 1 (-> 0), persistent (one block per CU) when there are more tiles than CUs
// (bn, mode: launch_halo3_fwd3; non-zero when that combination is not instantiated)
static int launch_h3(int bn, int mode, int ntiles, hipStream_t s, const ConvArgs& a, unsigned xb) {
  const int sch = res_sched(2) >= 2 ? 2 : 0;
  // FV_PERS_GRID=k caps the persistent grid at k blocks (tests: several tiles per block at
  // small shapes)
  const char* e = getenv("FV_PERS_GRID");
  const int cap = (e && atoi(e) > 0) ? atoi(e) : cu_count();
  // (the 256-row co tiles spill ~130 registers in the persistent form -- the epilogue's
  // read-back beside the carried tile state -- and ran res fwd 120 -> 166 us, r5; kept to the
  // smaller co tiles: AFE.down1's data gradient 366 -> 348 us)
  const bool pers = bn < 256 && ntiles > cap;
  if (!launch_halo3_fwd3(a, bn, mode, sch, pers, pers ? cap : ntiles, xb, ntiles, s)) return FV_OK;
  fv_set_error("halo 3x3 conv variant unsupported (co tile %d, mode %d)", bn, mode);
  return FV_E_BADARG;
}
// one conv3_halo_fwd2 launch of nblk tiles of 4 rows x 64 px x bn channels
static int launch_h2(int bn, int nblk, hipStream_t s, const ConvArgs& a, unsigned xb) {
  if (!launch_halo3_fwd2(a, bn, nblk, xb, s)) return FV_OK;
  fv_set_error("halo 3x3 conv variant unsupported (co tile %d)", bn);
  return FV_E_BADARG;
}
}  // extern "C++"

// 1x1 convs with K = 256 / 512 input channels and whole 256-channel output groups (the mid
// convs and their data gradients) on the pixel-stream kernel conv1x1_stream; FV_C1S=0 keeps
// conv_fwd_v2 (A/B).  Read per call.
static bool use_c1s(const fv_conv_desc* d) {
  const char* e = getenv("FV_C1S");
  if (e && e[0] == '0') return false;
  if (!use_v2(d) || d->ksize != 1 || d->upsample || d->pro_act) return false;
  if ((d->cin != 256 && d->cin != 512) || d->cout % 256 || d->ldy != d->cout) return false;
  const long P = (long)d->n * d->h * d->w;
  return P % (32768 / d->cin) == 0 && P * d->cout * 2 < (1L << 31);   // (both tile sizes)
}

static int conv_run(const fv_conv_desc* d, const void* x, const void* wk, const float* bias,
                    const float* psc, const float* psh, const void* res, void* y, float* stats,
                    hipStream_t s, const fv_store_reduce* sr = nullptr) {
  ConvArgs a{};
  if (sr && sr->mode) {
    FV_REQUIRE(sr_geometry(d, nullptr) > 0, "store-pass records not available for this conv (query fv_conv2d_sr_records)");
    FV_REQUIRE(sr->records, "store-pass records: null buffer");
    FV_REQUIRE(sr->mode == 1 || (sr->mode == 2 && sr->bn_input && sr->mean && sr->invstd && sr->gamma && sr->beta && !res),
               "store-pass records: bad mode / BN arguments");
    FV_REQUIRE(!stats, "store-pass records and accumulator statistics in one call are not supported");
    a.spm = sr->mode;
    a.sprec = sr->records;
    a.bnm = sr->mean; a.bni = sr->invstd; a.bng = sr->gamma; a.bnb = sr->beta; a.bns = sr->slope;
    if (sr->mode == 2) res = sr->bn_input;        // prefetched as a residual, not added
  }
  const FwdTile t = fwd_tile(d->cout);
  a.x = x; a.w = wk; a.bias = bias; a.psc = psc; a.psh = psh; a.slope = d->pro_slope;
  a.res = res; a.y = y; a.stats = stats;
  a.nrec = stats ? fv_conv2d_stats_blocks(d) : 0;
  a.N = d->n; a.H = d->h; a.W = d->w;
  a.Hin = d->upsample ? d->h / 2 : d->h;
  a.Win = d->upsample ? d->w / 2 : d->w;
  a.P = d->n * d->h * d->w;
  a.Cin = d->cin; a.lgCin = fv_ilog2(d->cin);
  a.Cout = d->cout; a.ldy = d->ldy;
  a.K = d->ksize * d->ksize * d->cin; a.Kpad = kpad_of(d->ksize, d->cin); a.nks = a.Kpad / BK;
  a.sigmoid = d->epi_sigmoid; a.nchw = d->out_nchw_f32;
  a.ntn = fv_cdiv(d->cout, t.bn);
  int st;
  // the weight image the caller sized with fv_conv_wk_elems(d) (fv_conv_wt_elems for a data
  // gradient: the same function of the transposed descriptor) must hold every row and k this
  // launch's weight DMA reads: rows = the co tiles it covers, k = its K per row (r4 fault: a
  // tile larger than the image read past its end)
  const long wk_have = (long)fv_conv_wk_elems(d);
  auto wext = [&](long rows, long kk, const char* what) {
    if (rows * kk > wk_have) {
      fv_set_error("conv %s: weight DMA extent %ld x %ld > weight image %ld elements", what, rows, kk, wk_have);
      return FV_E_BADARG;
    }
    return FV_OK;
  };
  if (use_c7n(d)) {
    FV_REQUIRE(!res, "out_conv kernel: no residual");
    const unsigned xb = (unsigned)((long)d->n * d->h * d->w * 64 * 2);
    const int band = c7n_band(d);
    const int nblk = d->n * (d->h / band) * (d->w / 64);
    launch_c7n(a, nblk, xb, band, s);
    return fv_check_launch("conv2d_fwd_c7n2");
  }
  // the 64-channel band kernel has no residual / store-pass epilogue: such a launch (a 64-channel
  // ResBlock conv) runs conv_fwd_v2, which reads the same plain [co][Kpad] weights (lay_of)
  const bool c64 = use_c64(d);
  if (c64 && !res && !a.spm) {
    if ((st = wext(d->cout, kpad_of(3, 64), "c64"))) return st;
    const int nb = c64_bands(d);
    const int nblk = d->n * (d->w / 64) * (d->cout / 64) * nb;
    const unsigned xb = (unsigned)((long)d->n * d->h * d->w * 64 * 2);
    launch_c64(a, nblk, xb, nb, s);
    return fv_check_launch("conv2d_fwd_c64");
  }
  if (use_c74(d)) {
    FV_REQUIRE(!res, "packed 7x7 conv: no residual");
    const int ntiles = d->n * (d->h / C74_TR) * (d->w / 64);
    const unsigned xb = (unsigned)((long)d->n * d->h * d->w * d->cin * 2);
    FV_REQUIRE(!a.stats || a.nrec == c74_grid(d), "packed 7x7 conv: %d BN records for %d blocks", a.nrec, c74_grid(d));
    launch_c74(a, c74_grid(d), xb, ntiles, s);
    return fv_check_launch("conv2d_fwd_c74");
  }
  if (const int tr = halo_tr(d)) {
    if ((st = wext(plan_tile(d).bn, kpad_of(7, d->cin), "halo7"))) return st;
    a.lgtw = 6;
    const int nblk = d->n * (d->h / tr) * (d->w / 64);
    const unsigned xb = (unsigned)((long)d->n * d->h * d->w * d->cin * 2);
    if (launch_halo7(a, d->cin, nblk, xb, s)) {
      fv_set_error("7x7 halo conv variant unsupported (cin=%d)", d->cin);
      return FV_E_BADARG;
    }
    return fv_check_launch("conv2d_fwd_halo");
  }
  if (use_upband(d)) {
    FV_REQUIRE(!res && !a.spm, "sub-pixel band conv: no residual / store-pass records");
    a.Ho = d->h; a.Wo = d->w;
    a.Kpad = kpad_of(2, d->cin);
    a.wphase = wrows(d->cout) * a.Kpad;
    if ((st = wext(4L * wrows(d->cout), a.Kpad, "upband"))) return st;
    const int hl = d->h / 2, wl = d->w / 2;
    const long base = (long)d->n * (wl / 32) * (d->cout / 64);
    int nb = 1;
    while (base * nb < 256 && hl % (nb * 16) == 0) nb *= 2;      // bands of a multiple of 8 rows
    const int nblk = (int)(base * nb);
    const unsigned xb = (unsigned)((long)d->n * hl * wl * 128 * 2);
    launch_upband(a, nblk, xb, nb, s);
    return fv_check_launch("conv2d_fwd_upband");
  }
  if (use_subpix_halo(d)) {
    FV_REQUIRE(!res && !a.spm, "sub-pixel conv: no residual / store-pass records");
    a.H = a.Hin; a.W = a.Win;                       // tile space = the low-res input image
    a.Ho = d->h; a.Wo = d->w;
    a.P = d->n * a.H * a.W;
    a.lgtw = 6;
    a.wus = 4 * d->cout * 64;                       // one unit = 4 phases x cout rows of 64 B
    a.ntn = d->cout / 64;
    const int nblk = a.ntn * d->n * (a.H / 4) * (a.W / 64);
    const unsigned xb = (unsigned)((long)d->n * a.H * a.W * d->cin * 2);
    // the weight DMA of the last unit ends inside the image the queries size
    FV_REQUIRE((long)4 * (d->cin / 32) * a.wus / 2 <= phase_wk_elems(d), "sub-pixel halo conv: weight image");
    if ((st = launch_h3(256, 1, nblk, s, a, xb))) return st;
    return fv_check_launch("conv2d_fwd_subpix_halo");
  }
  if (use_subpix(d)) {
    FV_REQUIRE(!res, "sub-pixel conv: no residual");
    const FwdTile t2 = fwd_tile_v2(d->cout);
    a.H = a.Hin; a.W = a.Win;                       // tile space = the low-res input image
    a.Ho = d->h; a.Wo = d->w;
    a.P = d->n * a.H * a.W;
    a.lgw = fv_ilog2(a.W); a.lghw = fv_ilog2(a.H * a.W);
    a.Kpad = kpad_of(2, d->cin);
    a.nks = a.Kpad / BK2;
    a.ntn = fv_cdiv(d->cout, t2.bn);
    a.wphase = wrows(d->cout) * a.Kpad;
    if ((st = wext(4L * a.ntn * t2.bn, a.Kpad, "subpix"))) return st;
    const int nblk2 = 4 * a.ntn * (a.P / t2.bm);
    const long xb = (long)d->n * a.Hin * a.Win * d->cin * 2;
    st = launch_v2(a, 2, t2, 2, nblk2, (unsigned)xb, s);
    if (st) {
      fv_set_error("sub-pixel conv variant unsupported (cout=%d)", d->cout);
      return st;
    }
    return fv_check_launch("conv2d_fwd_subpix");
  }
  if (const int bn = c64 ? 0 : halo3_bn(d)) {
    FV_REQUIRE(!(res && stats), "conv v2: residual and BN statistics in one call are not supported");
    a.lgtw = 6;
    a.wus = wk_rows(d) * 64;
    a.ntn = d->cout / bn;
    // stage-major: units of wk_rows(d) rows x 32; the tiles read rows [0, ntn * bn) of each
    if ((st = wext(a.ntn * bn, 9L * d->cin, "halo3")) || (st = wext(wk_rows(d), 9L * d->cin, "halo3 units")))
      return st;
    const int nblk = a.ntn * d->n * (d->h / 4) * (d->w / 64);
    const unsigned xb = (unsigned)((long)d->n * d->h * d->w * d->cin * 2);
    // linear-halo pair-of-taps kernel (conv3_halo_fwd3) for the 256 / 128-channel co tiles;
    // conv3_halo_fwd2 (XOR-swizzled halo) for 64-channel co tiles (AFE.down1's data gradient:
    // 448 us against 667 us on fwd3) and channel counts that are not a multiple of 64.
    // (measured and not kept, r2: the single-tap halo loop -- down2 dgrad 369 vs 324 us,
    // down1 dgrad 433 vs 414 us; a 3-deep weight ring for the 256-channel tiles, 2.5 % slower;
    // 8-row tiles for the 64-channel co tile, 418 -> 420 us; weight-DMA pieces spread between
    // the MFMA rows as conv_wgrad_v2 does, res conv forward 134 -> 160 us.  r3, res conv forward
    // in alternating runs on one box: halo chunks issued after the weight stage and left in
    // flight one step longer 126 -> 133 us; a ping-pong schedule (waves 4-7 one phase behind,
    // each wave's fragment reads + DMA issue beside its SIMD partner's MFMAs, 3-stage ring,
    // 2 barriers per step) 134 -> 142 us; 128 co x 512 px tiles, 25 instead of 40 KB of LDS-DMA
    // per step, 153 -> 157 (fwd2) / 161 us (ping-pong).  The clock-stamp build (build.py --diag)
    // puts the step at ~3400 cycles against 2048 of MFMA issue; with the MFMAs removed the
    // ping-pong loop still took 92 % of its time, with the fragment reads removed 65 %.
    // Stage-major weights (every DMA piece one contiguous KB, weight_prep_body smaj): res
    // fwd / dgrad 127 / 121.5 -> 122 / 117 us, down2 dgrad 317 -> 301 us (kept).  The weights
    // off the LDS-DMA path -- each wave's A fragments loaded to registers two / one taps ahead,
    // the halo register-staged, one barrier per 32-channel chunk: 126 -> 134 us (not kept).
    // r4: the 256 x 256 tile on 4 waves of 128 co x 128 px (one wave per SIMD, 512 registers,
    // a third fewer LDS fragment bytes per MFMA): res fwd / dgrad 133 / 127 -> 162 / 153 us,
    // the SIMD partner's MFMAs no longer cover a wave's fragment reads and barrier waits.  The B
    // fragments of the column-shifted taps (s = 1, 2) made from the previous tap's in registers
    // by DPP lane shifts (row_shl:1 | row_shr:15 of the next fragment, the row-end pixel read
    // as a broadcast: 2 instead of 8 B reads per tap): res fwd / dgrad 132-135 / 125-128 ->
    // 136-138 / 131-132 us, step +0.14 ms.  The weight stages after the first two through
    // registers (buffer_load_dwordx4 a step ahead, ds_write_b128 after the next barrier) instead
    // of LDS-DMA: res fwd / dgrad 147 / 136 -> 150.5 / 141 us, Generator.in_conv 147-152 ->
    // 160-162 us, step +0.17 ms.)
    // the epilogue's HALO form tests no bounds: tiles of tr rows x 64 pixels x bn channels cover
    // the output exactly (halo3_bn chose bn | cout for h % 4 == 0, w % 64 == 0)
    const int tr = (bn == 64 && d->h % 8 == 0 && a.Cin % 64 == 0) ? 8 : 4;
    FV_REQUIRE(halo_epi_ok(a, bn, tr), "halo 3x3 conv: %dx%d, cout %d is not whole tiles of %d rows x 64 px x %d co", d->h,
               d->w, d->cout, tr, bn);
    if (bn >= 128 && a.Cin % 64 == 0) {
      st = launch_h3(bn, 0, nblk, s, a, xb);
    } else if (bn >= 128) {
      st = launch_h2(bn, nblk, s, a, xb);
    } else if (d->h % 8 == 0 && a.Cin % 64 == 0) {
      // 64-channel co tile (AFE.down1's data gradient): 8 waves over 8 rows x 64 px, the
      // linear-halo kernel (fwd2's XOR-swizzled halo addressing was its VALU
      // limiter); waves 0-3 issue the 4 weight pieces of a tap
      const int nblk8 = a.ntn * d->n * (d->h / 8) * (d->w / 64);
      st = launch_h3(64, 0, nblk8, s, a, xb);
    } else {
      st = launch_h2(64, nblk, s, a, xb);
    }
    if (st) return st;
    return fv_check_launch("conv2d_fwd_halo3");
  }
  if (use_c1s(d) && !res && !stats && !a.spm) {
    if ((st = wext(d->cout, a.Kpad, "c1s"))) return st;
    FV_REQUIRE(a.Kpad == d->cin, "1x1 stream conv: K %d != Kpad %d", d->cin, a.Kpad);
    const int ncg = d->cout / 256;
    const int grid = std::max(8 * ncg, cu_count() / (8 * ncg) * (8 * ncg));
    const unsigned xb = (unsigned)((long)a.P * d->cin * 2);
    // FV_C1S_BP=64 / 128: pixels per tile for K = 256 (halved for K = 512): 4 slots of 32 KB
    // or 2 of 64 KB (A/B; read per call)
    const char* e = getenv("FV_C1S_BP");
    const bool big = e && atoi(e) == 128;
    const int bpx = (big ? 128 : 64) * 256 / d->cin;
    if (launch_c1s(a, d->cin, bpx, grid, xb, s)) {
      fv_set_error("1x1 stream conv variant unsupported (K=%d, %d px)", d->cin, bpx);
      return FV_E_BADARG;
    }
    return fv_check_launch("conv2d_fwd_c1s");
  }
  if (use_v2(d)) {
    FV_REQUIRE(!(res && stats), "conv v2: residual and BN statistics in one call are not supported");
    const FwdTile t2 = fwd_tile_v2(d->cout);
    a.ntn = fv_cdiv(d->cout, t2.bn);
    a.nks = a.Kpad / BK2;            // 64-deep steps; the 32-deep kernels double it themselves
    if ((st = wext((long)a.ntn * t2.bn, a.Kpad, "v2"))) return st;
    const int nblk2 = a.ntn * fv_cdiv(a.P, t2.bm);
    const long xb = (long)d->n * a.Hin * a.Win * d->cin * 2;
    st = launch_v2(a, d->ksize, t2, d->upsample, nblk2, (unsigned)xb, s);
    if (st) {
      fv_set_error("conv v2 variant unsupported (k=%d ups=%d)", d->ksize, d->upsample);
      return st;
    }
    return fv_check_launch("conv2d_fwd_v2");
  }
  const int nblk = a.ntn * fv_cdiv(a.P, t.bm);
  if ((st = wext((long)a.ntn * t.bn, a.Kpad, "v1"))) return st;
  st = d->dtype == FV_BF16 ? launch_fwd<bf16>(a, d->ksize, t, d->pro_act, d->upsample, nblk, s)
                           : launch_fwd<float>(a, d->ksize, t, d->pro_act, d->upsample, nblk, s);
  if (st) {
    fv_set_error("conv variant unsupported (k=%d pro=%d ups=%d)", d->ksize, d->pro_act, d->upsample);
    return st;
  }
  return fv_check_launch("conv2d_fwd");
}

int fv_conv2d_fwd(const fv_conv_desc* d, const void* x, const void* wk, const float* bias,
                  const float* pro_scale, const float* pro_shift, const void* res, void* y,
                  float* stats, void* stream) {
  int st = check_desc(d);
  if (st) return st;
  FV_REQUIRE(x && wk && y, "null pointer");
  FV_REQUIRE(!d->pro_act || (pro_scale && pro_shift), "prologue needs scale/shift");
  FV_REQUIRE(d->out_nchw_f32 || d->ldy >= d->cout, "ldy < cout");
  FV_REQUIRE(!res || d->ldy % 4 == 0, "residual needs ldy % 4 == 0");
  FV_REQUIRE(d->out_nchw_f32 || d->cout % 4 == 0 || d->ldy >= d->cout, "bad ldy");
  return conv_run(d, x, wk, bias, pro_scale, pro_shift, res, y, stats, (hipStream_t)stream);
}

// the forward-conv descriptor the data gradient of `d` runs as (transposed, flipped weights)
static fv_conv_desc dgrad_desc(const fv_conv_desc* d) {
  fv_conv_desc t{};
  t.dtype = d->dtype;
  t.n = d->n; t.h = d->h; t.w = d->w;
  t.cin = pad_pow2_8(d->cout);
  t.cin_valid = d->cout;
  t.cout = d->cin;   // every (padded) input channel; padded ones come out 0
  t.ldy = d->cin;
  t.ksize = d->ksize;
  return t;
}

int fv_conv2d_sr_records(const fv_conv_desc* d, int dgrad, int* record_pixels) {
  if (check_desc(d) != FV_OK) return 0;
  if (dgrad) {
    if (d->upsample) return 0;
    const fv_conv_desc t = dgrad_desc(d);
    return sr_geometry(&t, record_pixels);
  }
  return sr_geometry(d, record_pixels);
}

int fv_conv2d_fwd_sr(const fv_conv_desc* d, const void* x, const void* wk, const float* bias, const void* res, void* y,
                     const fv_store_reduce* sr, void* stream) {
  int st = check_desc(d);
  if (st) return st;
  FV_REQUIRE(x && wk && y && sr && sr->mode == 1, "fwd_sr: null pointer or mode != 1");
  FV_REQUIRE(!d->pro_act && !d->out_nchw_f32 && d->ldy == d->cout, "fwd_sr: plain NHWC output only");
  return conv_run(d, x, wk, bias, nullptr, nullptr, res, y, nullptr, (hipStream_t)stream, sr);
}

int fv_conv2d_bwd_data_sr(const fv_conv_desc* d, const void* dy, int ldy_dy, const void* wt, void* dx,
                          const fv_store_reduce* sr, void* stream) {
  int st = check_desc(d);
  if (st) return st;
  FV_REQUIRE(dy && wt && dx && sr && sr->mode == 2 && !d->upsample, "bwd_data_sr: bad argument");
  const fv_conv_desc t = dgrad_desc(d);
  FV_REQUIRE(ldy_dy == t.cin, "bwd_data: dy channel stride must be %d (got %d)", t.cin, ldy_dy);
  return conv_run(&t, dy, wt, nullptr, nullptr, nullptr, nullptr, dx, nullptr, (hipStream_t)stream, sr);
}

int fv_conv2d_bwd_data(const fv_conv_desc* d, const void* dy, int ldy_dy, const void* wt, void* dx,
                       void* stream) {
  int st = check_desc(d);
  if (st) return st;
  const fv_conv_desc t = dgrad_desc(d);
  FV_REQUIRE(ldy_dy == t.cin, "bwd_data: dy channel stride must be %d (got %d)", t.cin, ldy_dy);
  if (const int bn = dgrad_halo_bn(d)) {
    FV_REQUIRE(dy && wt && dx, "null pointer");
    ConvArgs a{};
    a.x = dy; a.w = wt; a.y = dx;
    a.N = d->n; a.H = d->h / 2; a.W = d->w / 2; a.Hin = d->h; a.Win = d->w;
    a.Ho = a.H; a.Wo = a.W;
    a.P = d->n * a.H * a.W;
    a.Cin = 4 * d->cout;                            // the 4 phase planes of dy as input channels
    a.K = d->cout;                                  // dy's channel stride
    a.Cout = d->cin; a.ldy = d->cin;
    a.lgtw = 6;
    a.wus = d->cin * 64;
    a.ntn = d->cin / bn;
    const int nblk = a.ntn * d->n * (a.H / 4) * (a.W / 64);
    const unsigned xb = (unsigned)((long)d->n * d->h * d->w * d->cout * 2);
    FV_REQUIRE((long)(a.Cin / 32) * 4 * a.wus / 2 <= phase_wt_elems(d), "low-res halo dgrad: weight image");
    FV_REQUIRE(halo_epi_ok(a, bn, 4), "low-res halo dgrad: %dx%d, cin %d is not whole tiles of 4 rows x 64 px x %d co", a.H,
               a.W, d->cin, bn);
    if ((st = launch_h3(bn, 2, nblk, (hipStream_t)stream, a, xb))) return st;
    return fv_check_launch("conv2d_bwd_data_lowres_halo");
  }
  if (use_dgrad_lowres(d)) {
    FV_REQUIRE(dy && wt && dx, "null pointer");
    ConvArgs a{};
    const FwdTile t2 = fwd_tile_v2(d->cin);
    a.x = dy; a.w = wt; a.y = dx;
    a.N = d->n; a.H = d->h / 2; a.W = d->w / 2; a.Hin = d->h; a.Win = d->w;
    a.Ho = a.H; a.Wo = a.W;
    a.P = d->n * a.H * a.W;
    a.Cin = t.cin; a.lgCin = fv_ilog2(t.cin);
    a.Cout = d->cin; a.ldy = d->cin;
    a.Kpad = 16 * t.cin; a.K = a.Kpad; a.nks = a.Kpad / BK2;
    a.ntn = fv_cdiv(d->cin, t2.bn);
    const int nblk = a.ntn * fv_cdiv(a.P, t2.bm);
    const long xb = (long)d->n * d->h * d->w * t.cin * 2;
    const int st = launch_v2(a, 4, t2, 3, nblk, (unsigned)xb, (hipStream_t)stream);
    if (st) {
      fv_set_error("low-res dgrad variant unsupported (cin=%d)", d->cin);
      return st;
    }
    return fv_check_launch("conv2d_bwd_data_lowres");
  }
  return conv_run(&t, dy, wt, nullptr, nullptr, nullptr, nullptr, dx, nullptr, (hipStream_t)stream);
}

int fv_conv2d_wgrad_nsplit(const fv_conv_desc* d) {
  if (check_desc(d) != FV_OK) return 0;
  return plan_wgrad(d).nsplit;
}

size_t fv_conv2d_wgrad_slab_elems(const fv_conv_desc* d) {
  if (check_desc(d) != FV_OK) return 0;
  const WgPlan p = plan_wgrad(d);
  return (size_t)(p.sub ? 4 : 1) * p.nsplit * p.CW * p.KW;
}

size_t fv_conv2d_wgrad_bias_slab_elems(const fv_conv_desc* d) {
  if (check_desc(d) != FV_OK) return 0;
  const WgPlan p = plan_wgrad(d);
  return (size_t)(p.sub ? 4 : 1) * p.nsplit * p.CW;
}

int fv_conv2d_bwd_weight(const fv_conv_desc* d, const void* x, const float* pro_scale,
                         const float* pro_shift, const void* dy, int ldy_dy, float* slab,
                         float* bias_slab, void* stream) {
  int st = check_desc(d);
  if (st) return st;
  FV_REQUIRE(x && dy && slab, "null pointer");
  FV_REQUIRE(ldy_dy % 8 == 0 && ldy_dy >= d->cout, "wgrad: dy channel stride must be a multiple of 8 >= cout");
  FV_REQUIRE(!d->pro_act || (pro_scale && pro_shift), "prologue needs scale/shift");
  const WgPlan t = plan_wgrad(d);
  const int Hin = d->upsample ? d->h / 2 : d->h, Win = d->upsample ? d->w / 2 : d->w;
  const long P = (long)d->n * d->h * d->w;
  if (t.v2 == 5) {
    FV_REQUIRE(P * ldy_dy * 2 < (1L << 31) && P * d->cin * 2 < (1L << 31), "wgrad: operand larger than 2 GB");
    H3Wg2Args a{};
    a.x = x; a.dy = dy; a.slab = slab; a.bslab = bias_slab;
    a.H = d->h; a.W = d->w; a.Cout = d->cout; a.ldd = ldy_dy;
    a.nseg = t.nsteps; a.rows = t.sps; a.nct = t.ntc;
    a.ldx = d->cin; a.nci = t.ntk;
    a.xbytes = (unsigned)(P * d->cin * 2);
    a.dybytes = (unsigned)(P * ldy_dy * 2);
    launch_h3_wg2(a, t.ntc * t.ntk * t.nsplit, (hipStream_t)stream);
    return fv_check_launch("conv2d_bwd_weight_halo3s");
  }
  if (t.v2 == 6) {
    FV_REQUIRE(P * ldy_dy * 2 < (1L << 31) && (long)d->n * Hin * Win * d->cin * 2 < (1L << 31),
               "wgrad: operand larger than 2 GB");
    UpWgArgs a{};
    a.x = x; a.dy = dy; a.slab = slab; a.bslab = bias_slab;
    a.Hin = Hin; a.Win = Win; a.Cout = d->cout; a.Cin = d->cin; a.ldd = ldy_dy;
    a.nct = t.ntc; a.nci = t.ntk; a.units = t.nsteps; a.spb = t.sps; a.nsplit = t.nsplit;
    a.xbytes = (unsigned)((long)d->n * Hin * Win * d->cin * 2);
    a.dybytes = (unsigned)(P * ldy_dy * 2);
    launch_up_wg(a, t.ntc * t.ntk * t.nsplit, (hipStream_t)stream);
    return fv_check_launch("conv2d_bwd_weight_up");
  }
  if (t.v2 == 3) {
    FV_REQUIRE(ldy_dy == 8, "wgrad (out_conv 7x7): dy channel stride must be 8 (got %d)", ldy_dy);
    W7Args a{};
    a.x = x; a.dy = dy; a.slab = slab; a.bslab = bias_slab;
    a.H = d->h; a.W = d->w; a.ldd = ldy_dy; a.cout = d->cout;
    a.seg_rows = t.sps; a.nseg = t.nsteps;
    a.xbytes = (unsigned)(P * 64 * 2);
    a.dybytes = (unsigned)(P * 8 * 2);
    launch_c7_wg(a, t.nsplit, (hipStream_t)stream);
    return fv_check_launch("conv2d_bwd_weight_c7");
  }
  if (t.v2 == 2) {
    const int ldd_need = d->cin == 8 ? 64 : 8;
    FV_REQUIRE(ldy_dy == ldd_need, "wgrad (7x7 halo): dy channel stride must be %d (got %d)", ldd_need, ldy_dy);
    HaloWgArgs a{};
    a.x = x; a.dy = dy; a.slab = slab; a.bslab = bias_slab;
    a.H = d->h; a.W = d->w; a.ldd = ldy_dy; a.K = d->ksize * d->ksize * d->cin;
    a.KW = t.KW; a.CW = t.CW; a.ntiles = t.nsteps; a.cout = d->cout;
    a.xbytes = (unsigned)(P * d->cin * 2);
    a.dybytes = (unsigned)(P * ldy_dy * 2);
    FV_REQUIRE(t.KW == (halo_wg_pk(d) ? 224 : fv_cdiv(a.K, 16) * 16), "7x7 halo wgrad: slab row length");
    launch_halo_wg(a, d->cin, halo_wg_pk(d), t.nsplit, (hipStream_t)stream);
    return fv_check_launch("conv2d_bwd_weight_halo");
  }
  if (t.sub) {
    FV_REQUIRE(P * ldy_dy * 2 < (1L << 31), "wgrad: dy larger than 2 GB");
    Wg2Args a{};
    a.x = x; a.dy = dy; a.slab = slab; a.bslab = bias_slab;
    a.H = Hin; a.W = Win; a.Hin = Hin; a.Win = Win; a.P = d->n * Hin * Win;
    a.Ho = d->h; a.Wo = d->w; a.nsplit = t.nsplit;
    a.lgCin = fv_ilog2(d->cin);
    a.K = 4 * d->cin;
    a.KW = t.KW; a.ldd = ldy_dy; a.CW = t.CW;
    a.ntk = t.ntk; a.ntc = t.ntc; a.nsteps = t.nsteps; a.sps = t.sps;
    a.fhw = make_fastdiv((uint32_t)(Hin * Win));
    a.fw = make_fastdiv((uint32_t)Win);
    a.fh = make_fastdiv((uint32_t)Hin);
    a.rowal = 1;
    a.il = 1;
    a.xbytes = (unsigned)((long)d->n * Hin * Win * d->cin * 2);
    a.dybytes = (unsigned)(P * ldy_dy * 2);
    const int nblk = 4 * t.ntk * t.ntc * t.nsplit;
    st = launch_wg2(a, 2, t, 0, nblk, (hipStream_t)stream);
    if (st) {
      fv_set_error("sub-pixel wgrad variant unsupported (cfg %d)", t.cfg);
      return st;
    }
    return fv_check_launch("conv2d_bwd_weight_subpix");
  }
  if (t.v2) {
    FV_REQUIRE(P * ldy_dy * 2 < (1L << 31), "wgrad: dy larger than 2 GB");
    Wg2Args a{};
    a.x = x; a.dy = dy; a.slab = slab; a.bslab = bias_slab;
    a.H = d->h; a.W = d->w; a.Hin = Hin; a.Win = Win; a.P = (int)P;
    a.lgCin = fv_ilog2(d->cin);
    a.K = d->ksize * d->ksize * d->cin;
    a.KW = t.KW; a.ldd = ldy_dy; a.CW = t.CW;
    a.ntk = t.ntk; a.ntc = t.ntc; a.nsteps = t.nsteps; a.sps = t.sps;
    a.fhw = make_fastdiv((uint32_t)(d->h * d->w));
    a.fw = make_fastdiv((uint32_t)d->w);
    a.fh = make_fastdiv((uint32_t)d->h);
    a.rowal = (d->w % t.px) == 0;
    a.il = 1;
    a.xbytes = (unsigned)((long)d->n * Hin * Win * d->cin * 2);
    a.dybytes = (unsigned)(P * ldy_dy * 2);
    const int nblk = t.ntk * t.ntc * t.nsplit;
    st = launch_wg2(a, d->ksize, t, d->upsample, nblk, (hipStream_t)stream);
    if (st) {
      fv_set_error("wgrad v2 variant unsupported (k=%d ups=%d bkt=%d bc=%d)", d->ksize, d->upsample, t.bkt, t.bc);
      return st;
    }
    return fv_check_launch("conv2d_bwd_weight_v2");
  }
  WgArgs a{};
  a.x = x; a.psc = pro_scale; a.psh = pro_shift; a.slope = d->pro_slope;
  a.dy = dy; a.slab = slab; a.bslab = bias_slab;
  a.N = d->n; a.H = d->h; a.W = d->w;
  a.Hin = Hin;
  a.Win = Win;
  a.P = (int)P;
  a.Cin = d->cin; a.lgCin = fv_ilog2(d->cin);
  a.K = d->ksize * d->ksize * d->cin;
  a.ntk = t.ntk; a.KW = t.KW;
  a.Cout = d->cout; a.ldd = ldy_dy;
  a.ntc = t.ntc; a.CW = t.CW;
  a.nsteps = t.nsteps;
  a.steps_per_split = t.sps;
  const int nblk = t.ntk * t.ntc * t.nsplit;
  st = d->dtype == FV_BF16 ? launch_wg<bf16>(a, d->ksize, t, d->pro_act, d->upsample, nblk, (hipStream_t)stream)
                           : launch_wg<float>(a, d->ksize, t, d->pro_act, d->upsample, nblk, (hipStream_t)stream);
  if (st) {
    fv_set_error("wgrad variant unsupported (k=%d pro=%d ups=%d)", d->ksize, d->pro_act, d->upsample);
    return st;
  }
  return fv_check_launch("conv2d_bwd_weight");
}

int fv_conv2d_wgrad_reduce(const fv_conv_desc* d, const float* slab, const float* bias_slab,
                           float* dw_param, float* db, void* stream) {
  int st = check_desc(d);
  if (st) return st;
  FV_REQUIRE(slab && dw_param, "null pointer");
  FV_REQUIRE(!db || bias_slab, "db needs the bias slab");
  const WgPlan t = plan_wgrad(d);
  if (t.v2 == 3) {
    launch_w7_reduce(const_cast<float*>(slab), const_cast<float*>(bias_slab), t.nsplit, d->cout, dw_param, db,
                     (hipStream_t)stream);
    return fv_check_launch("wgrad_reduce_c7");
  }
  if (t.sub && t.v2 == 6) {
    // many splits: split sums (in place), then the phase fold
    const long rowlen = (long)t.CW * t.KW;
    const int nb1 = (int)fv_cdiv(4 * rowlen, 64), nbb1 = db ? fv_cdiv(4L * t.CW, 64) : 0;
    launch_subpix_split_sum(const_cast<float*>(slab), const_cast<float*>(bias_slab), t.nsplit, rowlen, t.CW, nb1, nbb1,
                            (hipStream_t)stream);
    if ((st = fv_check_launch("wgrad_reduce_subpix_splits"))) return st;
    const int nb2 = fv_cdiv((long)d->cout * d->cin_valid * 9, 256), nbb2 = db ? fv_cdiv(d->cout, 256) : 0;
    launch_subpix_fold(slab, bias_slab, dw_param, db, t.nsplit, t.CW, t.KW, d->cout, d->cin_valid, fv_ilog2(d->cin), nb2,
                       nbb2, (hipStream_t)stream);
    return fv_check_launch("wgrad_reduce_subpix_fold");
  }
  if (t.sub) {
    const int nb_main = fv_cdiv((long)d->cout * d->cin_valid * 9, 64);
    const int nb_bias = db ? fv_cdiv(d->cout, 64) : 0;
    launch_wgrad_reduce_subpix(slab, bias_slab, dw_param, db, t.nsplit, t.CW, t.KW, d->cout, d->cin_valid,
                               fv_ilog2(d->cin), nb_main, nb_bias, (hipStream_t)stream);
    return fv_check_launch("wgrad_reduce_subpix");
  }
  // (the packed 7x7 slab rows: k = r * 32 + s * 4 + ci, i.e. 4 "channels" x 8 "taps" per row)
  const bool pk = t.v2 == 2 && halo_wg_pk(d);
  const int K = pk ? 7 * 32 : d->ksize * d->ksize * d->cin;
  const long tot = (long)d->cout * K;
  const int nb_main = fv_cdiv(tot, 64);
  const int nb_bias = db ? fv_cdiv(d->cout, 64) : 0;
  launch_wgrad_reduce(slab, bias_slab, dw_param, db, t.nsplit, t.CW, t.KW, K, d->cout, d->cin_valid,
                      pk ? 2 : fv_ilog2(d->cin), d->ksize, nb_main, nb_bias, pk ? 8 : d->ksize, (hipStream_t)stream);
  return fv_check_launch("wgrad_reduce");
}

// ---- stride-2 3x3 conv, padding 1 (the discriminator's down blocks, models.py:1120-1124) ----
size_t fv_conv2d_s2_wk_elems(const fv_conv_desc* d) {
  if (check_s2(d) != FV_OK) return 0;
  return (size_t)wrows(d->cout) * kpad_of(3, d->cin);
}

size_t fv_conv2d_s2_wt_elems(const fv_conv_desc* d) {
  if (check_s2(d) != FV_OK) return 0;
  return (size_t)4 * wrows(d->cin) * 4 * pad_pow2_8(d->cout);
}

int fv_conv2d_s2_weight_prep(const fv_conv_desc* d, const float* w_param, const float* sigma, void* wk, void* wt,
                             void* stream) {
  int st = check_s2(d);
  if (st) return st;
  FV_REQUIRE(w_param, "null pointer");
  hipStream_t s = (hipStream_t)stream;
  if (wk) {
    const int rows = wrows(d->cout), Kp = kpad_of(3, d->cin);
    const int nb = (int)std::min<long>(fv_cdiv((long)rows * Kp, 256), 4096);
    if (d->dtype == FV_BF16)
      hipLaunchKernelGGL(weight_prep_kernel<bf16>, dim3(nb), dim3(256), 0, s, w_param, sigma, (bf16*)wk, rows, Kp,
                         d->cout, d->cin_valid, fv_ilog2(d->cin), 3, 9 * d->cin, 0, 0);
    else
      hipLaunchKernelGGL(weight_prep_kernel<float>, dim3(nb), dim3(256), 0, s, w_param, sigma, (float*)wk, rows, Kp,
                         d->cout, d->cin_valid, fv_ilog2(d->cin), 3, 9 * d->cin, 0, 0);
    if ((st = fv_check_launch("s2_weight_prep"))) return st;
  }
  if (wt) {
    const int cin_t = pad_pow2_8(d->cout);
    const int rows = wrows(d->cin), Kph = 4 * cin_t;
    const int nb = (int)std::min<long>(fv_cdiv(4L * rows * Kph, 256), 4096);
    if (d->dtype == FV_BF16)
      hipLaunchKernelGGL(weight_prep_s2t_kernel<bf16>, dim3(nb), dim3(256), 0, s, w_param, sigma, (bf16*)wt, rows, Kph,
                         d->cout, d->cin_valid, fv_ilog2(cin_t));
    else
      hipLaunchKernelGGL(weight_prep_s2t_kernel<float>, dim3(nb), dim3(256), 0, s, w_param, sigma, (float*)wt, rows,
                         Kph, d->cout, d->cin_valid, fv_ilog2(cin_t));
    if ((st = fv_check_launch("s2_weight_prep_t"))) return st;
  }
  return FV_OK;
}

int fv_conv2d_s2_fwd(const fv_conv_desc* d, int in_h, int in_w, const void* x, const void* wk, const float* bias,
                     void* y, void* stream) {
  int st = check_s2(d);
  if (st) return st;
  if ((st = check_s2_in(d, in_h, in_w))) return st;
  FV_REQUIRE(x && wk && y, "null pointer");
  FV_REQUIRE(d->ldy >= d->cout, "ldy < cout");
  ConvArgs a{};
  const FwdTile t = fwd_tile(d->cout);
  a.x = x; a.w = wk; a.bias = bias; a.y = y;
  a.N = d->n; a.H = d->h; a.W = d->w; a.Hin = in_h; a.Win = in_w;
  a.P = d->n * d->h * d->w;
  a.Cin = d->cin; a.lgCin = fv_ilog2(d->cin);
  a.Cout = d->cout; a.ldy = d->ldy;
  a.K = 9 * d->cin; a.Kpad = kpad_of(3, d->cin); a.nks = a.Kpad / BK;
  a.ntn = fv_cdiv(d->cout, t.bn);
  FV_REQUIRE((long)a.ntn * t.bn <= wrows(d->cout), "stride-2 conv: weight rows");
  const int nblk = a.ntn * fv_cdiv(a.P, t.bm);
  if (d->dtype == FV_BF16) launch_s2_fwd<bf16, 1>(a, t, nblk, (hipStream_t)stream);
  else launch_s2_fwd<float, 1>(a, t, nblk, (hipStream_t)stream);
  return fv_check_launch("conv2d_s2_fwd");
}

int fv_conv2d_s2_bwd_data(const fv_conv_desc* d, int in_h, int in_w, const void* dy, int ldy_dy, const void* wt,
                          void* dx, void* stream) {
  int st = check_s2(d);
  if (st) return st;
  if ((st = check_s2_in(d, in_h, in_w))) return st;
  FV_REQUIRE(dy && wt && dx, "null pointer");
  const int cin_t = pad_pow2_8(d->cout);
  FV_REQUIRE(ldy_dy == cin_t, "stride-2 bwd_data: dy channel stride must be %d (got %d)", cin_t, ldy_dy);
  const FwdTile t = fwd_tile(d->cin);
  const int rows = wrows(d->cin);
  const long wphase = (long)rows * 4 * cin_t;
  const size_t es = d->dtype == FV_BF16 ? 2 : 4;
  for (int ph = 0; ph < 4; ++ph) {
    const int nt = (1 + (ph >> 1)) * (1 + (ph & 1));
    ConvArgs a{};
    a.x = dy; a.w = (const char*)wt + (size_t)ph * wphase * es; a.y = dx;
    a.N = d->n; a.H = d->h; a.W = d->w; a.Hin = d->h; a.Win = d->w;
    a.Ho = in_h; a.Wo = in_w;
    a.P = d->n * d->h * d->w;
    a.sub = 1 + ph;
    a.Cin = cin_t; a.lgCin = fv_ilog2(cin_t);
    a.Cout = d->cin; a.ldy = d->cin;         // every (padded) input channel; padded ones come out 0
    a.K = nt * cin_t; a.Kpad = 4 * cin_t; a.nks = fv_cdiv(a.K, BK);
    a.ntn = fv_cdiv(d->cin, t.bn);
    FV_REQUIRE((long)a.ntn * t.bn <= rows && a.nks * BK <= a.Kpad, "stride-2 bwd_data: weight image");
    const int nblk = a.ntn * fv_cdiv(a.P, t.bm);
    if (d->dtype == FV_BF16) launch_s2_fwd<bf16, 2>(a, t, nblk, (hipStream_t)stream);
    else launch_s2_fwd<float, 2>(a, t, nblk, (hipStream_t)stream);
  }
  return fv_check_launch("conv2d_s2_bwd_data");
}

size_t fv_conv2d_s2_wgrad_slab_elems(const fv_conv_desc* d) {
  if (check_s2(d) != FV_OK) return 0;
  const WgPlan p = plan_wgrad_s2(d);
  return (size_t)p.nsplit * p.CW * p.KW;
}

size_t fv_conv2d_s2_wgrad_bias_slab_elems(const fv_conv_desc* d) {
  if (check_s2(d) != FV_OK) return 0;
  const WgPlan p = plan_wgrad_s2(d);
  return (size_t)p.nsplit * p.CW;
}

int fv_conv2d_s2_bwd_weight(const fv_conv_desc* d, int in_h, int in_w, const void* x, const void* dy, int ldy_dy,
                            float* slab, float* bias_slab, void* stream) {
  int st = check_s2(d);
  if (st) return st;
  if ((st = check_s2_in(d, in_h, in_w))) return st;
  FV_REQUIRE(x && dy && slab, "null pointer");
  FV_REQUIRE(ldy_dy % 8 == 0 && ldy_dy >= d->cout, "wgrad: dy channel stride must be a multiple of 8 >= cout");
  const WgPlan t = plan_wgrad_s2(d);
  WgArgs a{};
  a.x = x; a.dy = dy; a.slab = slab; a.bslab = bias_slab;
  a.N = d->n; a.H = d->h; a.W = d->w; a.Hin = in_h; a.Win = in_w;
  a.P = d->n * d->h * d->w;
  a.Cin = d->cin; a.lgCin = fv_ilog2(d->cin);
  a.K = 9 * d->cin;
  a.ntk = t.ntk; a.KW = t.KW;
  a.Cout = d->cout; a.ldd = ldy_dy;
  a.ntc = t.ntc; a.CW = t.CW;
  a.nsteps = t.nsteps;
  a.steps_per_split = t.sps;
  const int nblk = t.ntk * t.ntc * t.nsplit;
  if (d->dtype == FV_BF16) launch_s2_wg<bf16>(a, t, nblk, (hipStream_t)stream);
  else launch_s2_wg<float>(a, t, nblk, (hipStream_t)stream);
  return fv_check_launch("conv2d_s2_bwd_weight");
}

int fv_conv2d_s2_wgrad_reduce(const fv_conv_desc* d, const float* slab, const float* bias_slab, float* dw_param,
                              float* db, void* stream) {
  int st = check_s2(d);
  if (st) return st;
  FV_REQUIRE(slab && dw_param, "null pointer");
  FV_REQUIRE(!db || bias_slab, "db needs the bias slab");
  const WgPlan t = plan_wgrad_s2(d);
  const int K = 9 * d->cin;
  const int nb_main = fv_cdiv((long)d->cout * K, 64);
  const int nb_bias = db ? fv_cdiv(d->cout, 64) : 0;
  launch_wgrad_reduce(slab, bias_slab, dw_param, db, t.nsplit, t.CW, t.KW, K, d->cout, d->cin_valid, fv_ilog2(d->cin), 3,
                      nb_main, nb_bias, 3, (hipStream_t)stream);
  return fv_check_launch("s2_wgrad_reduce");
}

}  // extern "C"

// ----------------------------------------------------------------------------------------
// ConvTranspose2dELR, kernel 4 / stride 2 / padding 1 (models_utils.py:404-516).
// out[o] = sum_j x[j] W[ci][co][o + 1 - 2j]: output phase pa (o = 2i + pa) reads the two
// low-res rows {i - 1, i} (pa = 0) or {i, i + 1} (pa = 1) -- the same 2x2 window per phase as
// the sub-pixel decomposition of nearest-x2 + 3x3 (weight_prep_subpix_kernel), with tap
// t = 3 - pa - 2 r' selected instead of folded.  So the transposed conv runs on the
// upsample-conv kernels unchanged (descriptor upsample = 1, ksize = 3, h/w = output size):
// forward = the sub-pixel phases, data gradient = the low-res stride-2 4x4 conv over dy
// (wt[ci][(tr*4 + tc)*cin_t + co] = Weff[ci][co][tr][tc]), weight gradient = the per-phase
// 2x2 slabs, mapped back to 4x4 taps here.  Weff = gain * W (* 1/max(||W[:, co]||, 1e-12)
// with norm == "demod", F.normalize over dims [0, 2, 3]: models_utils.py:461-470).
// ----------------------------------------------------------------------------------------
namespace {

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

extern "C" {

int fv_convt_supported(const fv_conv_desc* d) {
  if (check_desc(d) != FV_OK) return 0;
  if (!d->upsample || d->ksize != 3 || d->dtype != FV_BF16 || d->pro_act || d->epi_sigmoid || d->out_nchw_f32 ||
      pad_pow2_8(d->cout) != d->cout || d->ldy != d->cout)
    return 0;
  return (use_subpix(d) && use_dgrad_lowres(d) && plan_wgrad(d).sub) ? 1 : 0;
}

int fv_convt_weight_prep(const fv_conv_desc* d, const float* w, int demod, float gain, float* inv, void* wk,
                         void* wt, void* stream) {
  int st = check_desc(d);
  if (st) return st;
  FV_REQUIRE(fv_convt_supported(d), "conv_transpose2d k4 s2 p1: unsupported descriptor (cin=%d cout=%d %dx%d)",
             d->cin, d->cout, d->h, d->w);
  FV_REQUIRE(w && (!demod || inv), "null pointer");
  hipStream_t s = (hipStream_t)stream;
  if (demod) {
    hipLaunchKernelGGL(convt_norm_kernel, dim3(d->cout), dim3(64), 0, s, w, d->cin_valid, d->cout, inv);
    if ((st = fv_check_launch("convt_norm"))) return st;
  }
  // the halo kernels' phase layouts (conv3_halo_fwd3 MODE 1 / 2) where those kernels take the launch
  const float* cinv = demod ? inv : nullptr;
  if (wk && use_subpix_halo(d)) {
    const int nb1 = (int)std::min<long>(fv_cdiv(phase_wk_elems(d), 256), 4096);
    hipLaunchKernelGGL((weight_prep_phase_kernel<1, true>), dim3(nb1), dim3(256), 0, s, w, nullptr, (bf16*)wk,
                       4 * d->cout, 4 * (d->cin / 32), d->cout, d->cin_valid, 0, cinv, gain);
    if ((st = fv_check_launch("convt_weight_prep_phase1"))) return st;
    wk = nullptr;
  }
  if (wt && dgrad_halo_bn(d)) {
    const int nb2 = (int)std::min<long>(fv_cdiv(phase_wt_elems(d), 256), 4096);
    hipLaunchKernelGGL((weight_prep_phase_kernel<2, true>), dim3(nb2), dim3(256), 0, s, w, nullptr, (bf16*)wt, d->cin,
                       4 * (4 * d->cout / 32), d->cout, d->cin_valid, d->cout / 32, cinv, gain);
    if ((st = fv_check_launch("convt_weight_prep_phase2"))) return st;
    wt = nullptr;
  }
  if (!wk && !wt) return FV_OK;
  const int cin_t = pad_pow2_8(d->cout);
  const int rows = wrows(d->cout), Kp = kpad_of(2, d->cin);
  const int rows_t = wrows(d->cin);
  const long tot = (wk ? 4L * rows * Kp : 0) + (wt ? (long)rows_t * 16 * cin_t : 0);
  const int nb = (int)std::min<long>(fv_cdiv(tot, 256), 4096);
  hipLaunchKernelGGL(convt_weight_prep_kernel, dim3(nb), dim3(256), 0, s, w, demod ? inv : nullptr, gain, (bf16*)wk,
                     rows, Kp, fv_ilog2(d->cin), (bf16*)wt, rows_t, fv_ilog2(cin_t), d->cin_valid, d->cout);
  return fv_check_launch("convt_weight_prep");
}

int fv_convt_wgrad_reduce(const fv_conv_desc* d, const float* slab, const float* bias_slab, const float* w,
                          int demod, float gain, const float* inv, float* dw, float* db, void* stream) {
  int st = check_desc(d);
  if (st) return st;
  FV_REQUIRE(fv_convt_supported(d), "conv_transpose2d k4 s2 p1: unsupported descriptor");
  FV_REQUIRE(slab && w && dw && (!demod || inv) && (!db || bias_slab), "null pointer");
  const WgPlan t = plan_wgrad(d);
  hipStream_t s = (hipStream_t)stream;
  const int nb_main = fv_cdiv((long)d->cout * d->cin_valid * 16, 64);
  const int nb_bias = db ? fv_cdiv(d->cout, 64) : 0;
  hipLaunchKernelGGL(convt_wgrad_reduce_kernel, dim3(nb_main + nb_bias), dim3(256), 0, s, slab, bias_slab, dw, db,
                     t.nsplit, t.CW, t.KW, d->cout, d->cin_valid, fv_ilog2(d->cin), nb_main);
  if ((st = fv_check_launch("convt_wgrad_reduce"))) return st;
  hipLaunchKernelGGL(convt_weight_bwd_kernel, dim3(d->cout), dim3(64), 0, s, w, demod ? inv : nullptr, gain, dw,
                     d->cin_valid, d->cout);
  return fv_check_launch("convt_weight_bwd");
}

}  // extern "C"

// ========================================================================================
// fp8 (OCP e4m3) conv path: per-tensor scaled operands on v_mfma_scale_f32_16x16x128_f8f6f4
// (BASELINE config C5).  Forward and data gradient of the 3x3 convs with 128-multiple channel
// counts (ResBlock2D x 12 + Generator.in_conv: 58 % of the step's FLOPs) run on fp8 operands
// with fp32 accumulation; the weight gradient stays bf16 (its operands, the bf16 activations
// and gradients, are kept for it anyway).
//   Scaling: every fp8 tensor carries a power-of-two scale s = 2^floor(log2(448 / amax)) so
//   that |v * s| <= 448 (e4m3 max); dq = 1 / s is stored on the device and the conv epilogue
//   multiplies the fp32 accumulators by dq_x * dq_w (exact: powers of two).
// ========================================================================================
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
  return t.v2 == 5 && t.ntk == d->cin / 64 && t.sps % 2 == 0 && d->h % t.sps == 0 ? 1 : 0;
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
