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
// This file: the planners and switches, the argument checks and the exported bf16 / fp32 entries
// (weight preparation and ConvTranspose entries included) with their dispatch; it holds no kernel
// and no launch site.  The generic forward kernels are in conv_fwd.hip and conv_fwd_v2.hip, the
// halo-staged 3x3 forwards in conv_halo3.hip, the special-shape forwards in conv_shapes.hip, the
// weight-gradient kernels and slab reductions in conv_wgrad.hip, the weight re-layout and
// ConvTranspose weight kernels in conv_prep.hip, reached through the launchers declared in
// conv_common.h and conv_plan.h with the helpers and types the files share.  The fp8 path
// (kernels and entries) is conv_fp8.hip; it calls check_desc, res_sched, sr_geometry and
// plan_wgrad, which are defined here and declared in conv_plan.h.
#include "conv_plan.h"

namespace {

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
bool subpix_disabled() {     // FV_DISABLE_SUBPIX, read once
  static const bool off = [] { const char* e = getenv("FV_DISABLE_SUBPIX"); return e && e[0] == '1'; }();
  return off;
}
bool use_subpix(const fv_conv_desc* d) {
  if (subpix_disabled() || !d->upsample || d->ksize != 3 || !use_v2(d)) return false;
  const int hl = d->h / 2, wl = d->w / 2;
  if (fv_ilog2(hl) < 0 || fv_ilog2(wl) < 0 || wl % 16) return false;
  const long pl = (long)d->n * hl * wl;
  return pl % fwd_tile_v2(d->cout).bm == 0;
}

}  // namespace

// (declared in conv_plan.h: conv_fp8.hip calls it too)
// SIMD-partner schedule of the halo 3x3 kernels (conv3_halo_fwd3 / conv3_halo_fp8 SCH):
// FV_RES_SCHED = 0 (prio flips, lockstep), 1 (static prio for waves 4-7), 2 (stagger), 3
// (both); unset: the measured default of each kernel (dflt).  conv3_halo_fwd3 keeps 0 and 2
// (1 / 3 measured no better, below).  Read per call (tests compare the
// schedules bit for bit in one process).  r5, alternating convbench runs on one box, B=32 bf16
// res fwd / dgrad: 0: 130 / 122, 1: 124 / 118, 2: 120 / 115, 3: 126 / 119 us; B=64 fp8 res
// fwd / dgrad: 0: 175 / 166, 1: 173 / 163, 2: 172 / 155, 3: 165 / 155 us.
int res_sched(int dflt) {
  const char* e = getenv("FV_RES_SCHED");
  return (e && e[0] >= '0' && e[0] <= '3') ? e[0] - '0' : dflt;
}

namespace {

// data gradient of an upsample + 3x3 conv computed directly at the low resolution as a
// stride-2 4x4 conv over dy (bf16 v2 path; replaces dgrad at the high resolution followed by
// the 2x2 sum of fv_upsample2x_bwd: 0.44x the MACs, one pass fewer)
bool use_dgrad_lowres(const fv_conv_desc* d) {
  if (subpix_disabled() || !d->upsample || d->ksize != 3 || d->dtype != FV_BF16) return false;
  const int ct = pad_pow2_8(d->cout);
  if (ct % 64 || d->cin % 8 || (d->w / 2) % 16) return false;
  return (long)d->n * d->h * d->w * ct * 2 < (1L << 31);
}

// UpBlock2D forward with a 128-channel input on the sliding-band kernel (conv3up_band_fwd).
// Its weights are the plain sub-pixel layout.  (This and use_subpix_halo: given use_subpix(d).)
static bool use_upband(const fv_conv_desc* d) {
  const int hl = d->h / 2, wl = d->w / 2;
  return d->cin == 128 && d->cin_valid == 128 && d->cout % 64 == 0 && wl % 32 == 0 && hl % 8 == 0 &&
         !d->out_nchw_f32 && !d->epi_sigmoid && !d->pro_act && d->ldy % 8 == 0 &&
         (long)d->n * hl * wl * 128 * 2 < (1L << 31) && (long)d->n * d->h * d->w * d->ldy * 2 < (1L << 31);
}
// the other UpBlock2D convs on the halo kernel (conv3_halo_fwd3 MODE 1 forward; MODE 2 low-res
// data gradient: dgrad_halo_bn); shapes outside these conditions run conv_fwd_v2 MODE 2 / 3
static bool use_subpix_halo(const fv_conv_desc* d) {
  const int hl = d->h / 2, wl = d->w / 2;
  return d->cout % 64 == 0 && d->cin % 32 == 0 && d->cin >= 64 && d->cin_valid == d->cin && wl % 64 == 0 &&
         hl % 4 == 0 && !d->out_nchw_f32 && !d->epi_sigmoid && !d->pro_act && d->ldy % 8 == 0 &&
         (long)d->n * hl * wl * d->cin * 2 < (1L << 31) && (long)d->n * d->h * d->w * d->ldy * 2 < (1L << 31);
}
// co tile (256 / 128 rows) of the low-res data gradient on the halo kernel, 0 = not on it
// (given use_dgrad_lowres(d))
static int dgrad_halo_bn(const fv_conv_desc* d) {
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

}  // namespace

// (declared in conv_plan.h: conv_fp8.hip's entries check their descriptors with it too)
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

namespace {

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
// the register-staged kernel's tile, and the tiles, splits and slab of a plan whose tile is set
// (the tail of plan_wgrad and all of plan_wgrad_s2)
void wg_v1_tile(WgPlan* p, int cout) {
  p->bc = cout > 64 ? 128 : (cout > 16 ? 64 : 16);
  p->bkt = 128;
  p->px = 32;
}
void wg_split(WgPlan* p, int K, int cout, long P) {
  p->ntk = fv_cdiv(K, p->bkt);
  p->ntc = fv_cdiv(cout, p->bc);
  p->nsteps = fv_cdiv(P, p->px);
  const int ntile = p->ntk * p->ntc;
  // v2: about 256 blocks (128: 1x1 weight gradients 45 / 33 -> 67 / 40 us)
  int ns = p->v2 ? (256 + ntile / 2) / ntile : 768 / ntile;
  if (ns < 1) ns = 1;
  if (ns > p->nsteps) ns = p->nsteps;
  p->sps = fv_cdiv(p->nsteps, ns);
  p->nsplit = fv_cdiv(p->nsteps, p->sps);
  p->KW = p->ntk * p->bkt;
  p->CW = p->ntc * p->bc;
}

}  // namespace

// (declared in conv_plan.h: the fp8 weight gradient of conv_fp8.hip takes its slab geometry from it)
WgPlan plan_wgrad(const fv_conv_desc* d) {
  WgPlan p{};
  const int K = d->ksize * d->ksize * d->cin;
  const long P = (long)d->n * d->h * d->w;
  const long hin = d->upsample ? d->h / 2 : d->h, win = d->upsample ? d->w / 2 : d->w;
  // 32-bit buffer offsets: x and dy (channel stride = cout padded to a power of two >= 8, as
  // every caller passes; fv_conv2d_bwd_weight re-checks the real stride) must stay < 2 GB
  const bool fits = d->dtype == FV_BF16 && (long)d->n * hin * win * d->cin * 2 < (1L << 31) &&
                   P * pad_pow2_8(d->cout) * 2 < (1L << 31);
  p.v2 = fits && !d->pro_act ? WG_V2 : WG_V1;
  // out_conv 7x7 64 -> <= 4 (WG_C7): blocks = (image, 64-column strip, row segment), about
  // 2 per CU (r6: 1024 -> 512 blocks halves the 58.7 MB of slabs; out_conv weight gradient
  // 98.4 -> 90.4 us + reduce 15 -> 10.6 us, step -0.03 ms; 256 blocks: 114 us;
  // profiles/r6/r6k_ab_wgrad_blocks.log); slab [block][32 (r, co)][448 (s, ci)]
  if (p.v2 && use_c7w(d)) {
    const int strips = d->w / 64;
    int nseg = fv_cdiv(512, d->n * strips);
    if (nseg > fv_cdiv(d->h, 8)) nseg = fv_cdiv(d->h, 8);
    if (nseg < 1) nseg = 1;
    p.v2 = WG_C7;
    p.sps = fv_cdiv(d->h, nseg);                 // rows per segment
    p.nsteps = fv_cdiv(d->h, p.sps);             // segments
    p.nsplit = d->n * strips * p.nsteps;
    p.CW = 32;
    p.KW = 448;
    p.ntk = p.ntc = 1;
    return p;
  }
  // 3x3 sliding-row wgrad (WG_H3S, conv3_halo_wgrad2): blocks = (image, 64-column strip,
  // row segment) x co tiles of 128, ~1 block per CU; splits = image x strip x segment
  if (fits && use_h3w(d)) {
    const int strips = d->w / 64;
    p.v2 = WG_H3S;
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
  // 7x7 halo path (WG_HALO7): one persistent block per CU, ntk = 1 (all k in one tile)
  const int htr = halo_wg_tr(d);
  if (p.v2 && htr) {
    const int nt = d->cin == 8 ? 4 : 1;
    p.v2 = WG_HALO7;
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
    // sub-pixel sliding-row weight gradient (WG_UP, conv3_up_wgrad): blocks = (co tile, ci
    // tile) x splits of `sps` consecutive (image, 64-column output strip) units, ~one block per
    // CU; slab [phase][split][co][4 cin] as the v2 sub-pixel path
    p.sub = 1;
    p.v2 = WG_UP;
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
    wg_v1_tile(&p, d->cout);
  }
  wg_split(&p, K, d->cout, P);
  return p;
}

namespace {

// the stride-2 weight gradient's plan: the generic kernel's tiles (plan_wgrad's fp32 branch) for both dtypes
WgPlan plan_wgrad_s2(const fv_conv_desc* d) {
  WgPlan p{};
  wg_v1_tile(&p, d->cout);
  wg_split(&p, 9 * d->cin, d->cout, (long)d->n * d->h * d->w);
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

// The forward plan: the use_*() conditions above are asked here, in the order of the launch, and
// nowhere else.  Everything but `kind` is a function of the descriptor alone (FV_C1S only swaps
// V2 and C1S, which share tile, records and weight image).
FwdPlan plan_fwd(const fv_conv_desc* d) {
  FwdPlan p{};
  const long P = (long)d->n * d->h * d->w;
  auto set = [&p](FwdKind k, int bn, int tr, int bm, int rec_px) {
    p.kind = k; p.bn = bn; p.tr = tr; p.bm = bm; p.rec_px = rec_px;
  };
  // BN-statistics records of the generic kernels: the pixels of one wave row of the tile (BM / WM)
  auto set_v2 = [&](FwdKind k, int rec_px) {
    const FwdTile t = fwd_tile_v2(d->cout);
    const bool wm4 = t.bn == 64 || t.bn == 16 || (t.bn == 128 && t.bm == 256);   // else 128x128, 256x256, 256x128
    set(k, t.bn, 0, t.bm, rec_px ? rec_px : wm4 ? t.bm / 4 : t.bm / 2);
  };
  // the generic image [rows][Kpad]: whole co tiles of every kernel that may read it (wrows)
  p.wrows = wrows(d->cout);
  p.wlen = kpad_of(d->ksize, d->cin);
  p.welems = (long)p.wrows * p.wlen;
  if (use_c7n(d)) {
    set(FV_CONVK_C7N, 4, 0, 0, 64);                                  // one 64-pixel row segment
    p.wrows = p.wlen = 0;
    p.welems = 32 * 448;
  } else if (use_c64(d)) {
    set_v2(FV_CONVK_C64, C64_G * 64);                                // 8 iterations x one wave's row
  } else if (const int tr = halo_tr(d)) {
    if (use_c74(d)) {
      set(FV_CONVK_C74, 64, C74_TR, C74_TR * 64, c74_tiles_per_block(d) * C74_TR * 64);   // one record per block
      p.wlay = 2;
      p.wlen = C74_K;       // the packed rows are C74_K long (the image keeps the generic size)
    } else {
      set(FV_CONVK_HALO7, d->cout <= 16 ? 16 : 64, tr, tr * 64, tr * 64 / 8);   // 8 waves stacked over pixels
    }
  } else if (use_subpix(d)) {
    p.wlen = kpad_of(2, d->cin);                                      // 4 phase images of 2x2 taps
    p.welems = 4L * p.wrows * p.wlen;
    if (use_upband(d)) {
      set(FV_CONVK_UPBAND, 64, 0, 0, UPB_G * 2 * 32);                // (block, 4 iterations, phase)
    } else if (use_subpix_halo(d)) {
      set(FV_CONVK_SUBPIX_HALO, 64, 4, 256, 128);                    // (tile, wave row, phase): RM * 16
      p.wrows = p.wlen = 0;
      p.welems = phase_wk_elems(d);
    } else {
      set_v2(FV_CONVK_SUBPIX_V2, 0);
    }
  } else if (const int bn = halo3_bn(d)) {
    // conv3_halo_fwd3 for the 256 / 128-channel co tiles and the 8-row form of the 64-channel one,
    // conv3_halo_fwd2 otherwise (the measurements: conv_run)
    const bool c64k = d->cin % 64 == 0;
    const int tr = (bn == 64 && d->h % 8 == 0 && c64k) ? 8 : 4;
    set((bn >= 128 ? c64k : tr == 8) ? FV_CONVK_HALO3_FWD3 : FV_CONVK_HALO3_FWD2, bn, tr, tr * 64,
        bn == 256 ? 128 : 64);                                        // RM * 16 pixels per wave row
    p.wlay = 1;             // stage-major (weight_prep_body smaj): units of wrows rows x 32
    // store-pass records: 256-pixel tiles of 8 waves (co tiles of 256 / 128) or 4 waves (co tiles
    // of 64), one record per (tile, wave)
    if (d->cout % bn == 0 && P % 256 == 0) {
      const int nw = bn == 64 ? 4 : 8;
      p.sr_px = 256 / nw;
      p.sr_n = (int)(P / 256 * nw);
    }
  } else if (use_v2(d)) {
    set_v2(use_c1s(d) ? FV_CONVK_C1S : FV_CONVK_V2, 0);
  } else {
    const FwdTile t = fwd_tile(d->cout);
    set(FV_CONVK_V1, t.bn, 0, t.bm, t.bn == 16 ? t.bm / 4 : t.bm / 2);   // launch_fwd_ks
  }
  return p;
}

// The data gradient: directly at the low resolution for an upsample conv that qualifies, else the
// forward of the transposed descriptor.
FwdPlan plan_dgrad(const fv_conv_desc* d) {
  if (!use_dgrad_lowres(d)) {
    const fv_conv_desc t = dgrad_desc(d);
    return plan_fwd(&t);
  }
  FwdPlan p{};
  if (const int bn = dgrad_halo_bn(d)) {
    p.kind = FV_CONVK_DGRAD_LOWRES_HALO;
    p.bn = bn; p.tr = 4; p.bm = 256;
    p.welems = phase_wt_elems(d);
  } else {
    const FwdTile t = fwd_tile_v2(d->cin);
    p.kind = FV_CONVK_DGRAD_LOWRES_V2;
    p.bn = t.bn; p.bm = t.bm;
    p.wrows = wrows(d->cin);
    p.wlen = 16 * pad_pow2_8(d->cout);                                // 4x4 taps
    p.welems = (long)p.wrows * p.wlen;
  }
  return p;
}

// What one call launches.  The 64-channel band kernel has no residual / store-pass epilogue and
// the 1x1 stream kernel no residual, statistics or store pass: such a call runs conv_fwd_v2.  It
// may, because the plan gives both kinds conv_fwd_v2's tile and the plain [rows][Kpad] image that
// covers whole tiles of it (wrows), and every use_c64 / use_c1s descriptor passes use_v2.
FwdKind fwd_kind(const FwdPlan& p, bool res, bool stats, int sr_mode) {
  if (p.kind == FV_CONVK_C64 && (res || sr_mode)) return FV_CONVK_V2;
  if (p.kind == FV_CONVK_C1S && (res || stats || sr_mode)) return FV_CONVK_V2;
  return p.kind;
}

// store-pass record geometry (fv_store_reduce) of the launch `d` takes: records and pixels per
// record, 0 when that path has none (the halo-staged 3x3 kernels only have them).
// (declared in conv_plan.h: fv_conv2d_fwd_fp8_site_sr of conv_fp8.hip checks its records with it)
int sr_geometry(const fv_conv_desc* d, int* bp) {
  const FwdPlan p = plan_fwd(d);
  if (bp && p.sr_n) *bp = p.sr_px;
  return p.sr_n;
}

// the image is one the generic re-layout kernels (weight_prep_kernel and its batched forms) write
static bool wprep_generic(const FwdPlan& p) {
  switch (p.kind) {
    case FV_CONVK_C7N: case FV_CONVK_UPBAND: case FV_CONVK_SUBPIX_HALO: case FV_CONVK_SUBPIX_V2:
    case FV_CONVK_DGRAD_LOWRES_HALO: case FV_CONVK_DGRAD_LOWRES_V2: return false;
    default: return true;
  }
}

extern "C" {

size_t fv_conv_wk_elems(const fv_conv_desc* d) {
  return check_desc(d) == FV_OK ? (size_t)plan_fwd(d).welems : 0;
}

size_t fv_conv_wt_elems(const fv_conv_desc* d) {
  return check_desc(d) == FV_OK ? (size_t)plan_dgrad(d).welems : 0;
}

int fv_conv2d_dgrad_lowres(const fv_conv_desc* d) {
  return check_desc(d) == FV_OK && plan_dgrad(d).kind >= FV_CONVK_DGRAD_LOWRES_HALO ? 1 : 0;
}

int fv_conv2d_fwd_kernel(const fv_conv_desc* d, int dgrad, int has_res, int has_stats, int sr_mode) {
  if (check_desc(d) != FV_OK) return -1;
  return fwd_kind(dgrad ? plan_dgrad(d) : plan_fwd(d), has_res, has_stats, sr_mode);
}

int fv_conv2d_stats_block_pixels(const fv_conv_desc* d) {
  return check_desc(d) == FV_OK ? plan_fwd(d).rec_px : 0;
}

int fv_conv2d_stats_blocks(const fv_conv_desc* d) {
  return check_desc(d) == FV_OK ? fv_cdiv((long)d->n * d->h * d->w, plan_fwd(d).rec_px) : 0;
}

int fv_conv_weight_prep(const fv_conv_desc* d, const float* w_param, const float* sigma, void* wk,
                        void* wt, void* stream) {
  int st = check_desc(d);
  if (st) return st;
  hipStream_t s = (hipStream_t)stream;
  const int ks = d->ksize;
  const int cin_t = pad_pow2_8(d->cout);
  const FwdPlan pk = plan_fwd(d), pt = plan_dgrad(d);
  if (wk && wt && wprep_generic(pk) && wprep_generic(pt)) {
    // the common case: forward and transposed layouts in one launch
    WPrepJob j0{wk, pk.wrows, pk.wlen, fv_ilog2(d->cin), ks * ks * d->cin, 0, 0, pk.wlay};
    WPrepJob j1{wt, pt.wrows, pt.wlen, fv_ilog2(cin_t), ks * ks * cin_t, 1, 0, pt.wlay};
    j0.nb = (int)std::min<long>(fv_cdiv((long)j0.rows * j0.Kpad, 256), 4096);
    j1.nb = (int)std::min<long>(fv_cdiv((long)j1.rows * j1.Kpad, 256), 4096);
    FV_REQUIRE(!launch_wprep2(d->dtype, w_param, sigma, d->cout, d->cin_valid, ks, j0, j1, j0.nb + j1.nb, s),
               "weight prep: dtype %d unsupported", d->dtype);
    return fv_check_launch("weight_prep2");
  }
  // (the stage-major / packed layouts are bf16 layouts: every kind that has one is a bf16 kind,
  // so the fp32 images are plain)
  if (wk && pk.kind == FV_CONVK_C7N) {
    launch_wprep_c7n(w_param, sigma, (bf16*)wk, d->cout, 56, s);
    if ((st = fv_check_launch("weight_prep_c7n"))) return st;
  } else if (wk && pk.kind == FV_CONVK_SUBPIX_HALO) {
    const int nb = (int)std::min<long>(fv_cdiv(pk.welems, 256), 4096);
    FV_REQUIRE(!launch_wprep_phase(1, false, w_param, sigma, (bf16*)wk, 4 * d->cout, 4 * (d->cin / 32), d->cout,
                                   d->cin_valid, 0, nullptr, 1.f, nb, s),
               "weight prep: phase layout unsupported");
    if ((st = fv_check_launch("weight_prep_phase1"))) return st;
  } else if (wk && !wprep_generic(pk)) {     // SUBPIX_V2, UPBAND: the plain sub-pixel images
    const int nb = (int)std::min<long>(fv_cdiv(pk.welems, 256), 4096);
    launch_wprep_subpix(w_param, sigma, (bf16*)wk, pk.wrows, pk.wlen, d->cout, d->cin_valid, fv_ilog2(d->cin), nb, s);
    if ((st = fv_check_launch("weight_prep_subpix"))) return st;
  } else if (wk) {
    const int nb = (int)std::min<long>(fv_cdiv((long)pk.wrows * pk.wlen, 256), 4096);
    FV_REQUIRE(!launch_wprep(d->dtype, w_param, sigma, wk, pk.wrows, pk.wlen, d->cout, d->cin_valid, fv_ilog2(d->cin),
                             ks, ks * ks * d->cin, 0, pk.wlay, nb, s),
               "weight prep: dtype %d unsupported", d->dtype);
    if ((st = fv_check_launch("weight_prep"))) return st;
  }
  if (wt && pt.kind == FV_CONVK_DGRAD_LOWRES_HALO) {
    const int nb = (int)std::min<long>(fv_cdiv(pt.welems, 256), 4096);
    FV_REQUIRE(!launch_wprep_phase(2, false, w_param, sigma, (bf16*)wt, d->cin, 4 * (4 * d->cout / 32), d->cout,
                                   d->cin_valid, d->cout / 32, nullptr, 1.f, nb, s),
               "weight prep: phase layout unsupported");
    if ((st = fv_check_launch("weight_prep_phase2"))) return st;
  } else if (wt && pt.kind == FV_CONVK_DGRAD_LOWRES_V2) {
    const int nb = (int)std::min<long>(fv_cdiv(pt.welems, 256), 4096);
    launch_wprep_s2(w_param, sigma, (bf16*)wt, pt.wrows, pt.wlen, d->cout, d->cin_valid, fv_ilog2(cin_t), nb, s);
    if ((st = fv_check_launch("weight_prep_s2"))) return st;
  } else if (wt) {
    const int nb = (int)std::min<long>(fv_cdiv((long)pt.wrows * pt.wlen, 256), 4096);
    FV_REQUIRE(!launch_wprep(d->dtype, w_param, sigma, wt, pt.wrows, pt.wlen, d->cout, d->cin_valid, fv_ilog2(cin_t),
                             ks, ks * ks * cin_t, 1, pt.wlay, nb, s),
               "weight prep: dtype %d unsupported", d->dtype);
    if ((st = fv_check_launch("weight_prep_t"))) return st;
  }
  return FV_OK;
}

int fv_conv_weight_prep_batchable(const fv_conv_desc* d) {
  return check_desc(d) == FV_OK && wprep_generic(plan_fwd(d)) && wprep_generic(plan_dgrad(d));
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
    const FwdPlan pk = plan_fwd(d);
    WPrepMJob j0{w_params[i], sigmas[i], wks[i], pk.wrows, pk.wlen, fv_ilog2(d->cin),
                 ks * ks * d->cin, 0, 0, d->cout, d->cin_valid, ks, 0, pk.wlay};
    j0.nb = (int)std::min<long>(fv_cdiv((long)j0.rows * j0.Kpad, 256), 256);
    nb_total = std::max(nb_total, j0.nb);
    m.j[m.n++] = j0;
    if (wts[i]) {
      const int cin_t = pad_pow2_8(d->cout);
      const FwdPlan pt = plan_dgrad(d);
      WPrepMJob j1{w_params[i], sigmas[i], wts[i], pt.wrows, pt.wlen, fv_ilog2(cin_t),
                   ks * ks * cin_t, 1, 0, d->cout, d->cin_valid, ks, 0, pt.wlay};
      j1.nb = (int)std::min<long>(fv_cdiv((long)j1.rows * j1.Kpad, 256), 256);
      nb_total = std::max(nb_total, j1.nb);
      m.j[m.n++] = j1;
    }
  }
  hipStream_t s = (hipStream_t)stream;
  FV_REQUIRE(!launch_wprep_multi(dtype, m, nb_total, s), "weight_prep_multi: dtype %d unsupported", dtype);
  return fv_check_launch("weight_prep_multi");
}

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

// one forward launch of descriptor d by its plan p (plan_fwd(d), or plan_dgrad of the conv that d
// is the transposed descriptor of)
static int conv_run(const fv_conv_desc* d, const FwdPlan& p, const void* x, const void* wk, const float* bias,
                    const float* psc, const float* psh, const void* res, void* y, float* stats,
                    hipStream_t s, const fv_store_reduce* sr = nullptr) {
  ConvArgs a{};
  if (sr && sr->mode) {
    FV_REQUIRE(p.sr_n > 0, "store-pass records not available for this conv (query fv_conv2d_sr_records)");
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
  a.nrec = stats ? fv_cdiv((long)d->n * d->h * d->w, p.rec_px) : 0;
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
  const long wk_have = p.welems;
  auto wext = [&](long rows, long kk, const char* what) {
    if (rows * kk > wk_have) {
      fv_set_error("conv %s: weight DMA extent %ld x %ld > weight image %ld elements", what, rows, kk, wk_have);
      return FV_E_BADARG;
    }
    return FV_OK;
  };
  switch (fwd_kind(p, res != nullptr, stats != nullptr, a.spm)) {
  case FV_CONVK_C7N: {
    FV_REQUIRE(!res, "out_conv kernel: no residual");
    const unsigned xb = (unsigned)((long)d->n * d->h * d->w * 64 * 2);
    const int band = c7n_band(d);
    const int nblk = d->n * (d->h / band) * (d->w / 64);
    launch_c7n(a, nblk, xb, band, s);
    return fv_check_launch("conv2d_fwd_c7n2");
  }
  case FV_CONVK_C64: {
    if ((st = wext(d->cout, kpad_of(3, 64), "c64"))) return st;
    const int nb = c64_bands(d);
    const int nblk = d->n * (d->w / 64) * (d->cout / 64) * nb;
    const unsigned xb = (unsigned)((long)d->n * d->h * d->w * 64 * 2);
    launch_c64(a, nblk, xb, nb, s);
    return fv_check_launch("conv2d_fwd_c64");
  }
  case FV_CONVK_C74: {
    FV_REQUIRE(!res, "packed 7x7 conv: no residual");
    const int ntiles = d->n * (d->h / C74_TR) * (d->w / 64);
    const unsigned xb = (unsigned)((long)d->n * d->h * d->w * d->cin * 2);
    FV_REQUIRE(!a.stats || a.nrec == c74_grid(d), "packed 7x7 conv: %d BN records for %d blocks", a.nrec, c74_grid(d));
    launch_c74(a, c74_grid(d), xb, ntiles, s);
    return fv_check_launch("conv2d_fwd_c74");
  }
  case FV_CONVK_HALO7: {
    const int tr = p.tr;
    if ((st = wext(p.bn, kpad_of(7, d->cin), "halo7"))) return st;
    a.lgtw = 6;
    const int nblk = d->n * (d->h / tr) * (d->w / 64);
    const unsigned xb = (unsigned)((long)d->n * d->h * d->w * d->cin * 2);
    if (launch_halo7(a, d->cin, nblk, xb, s)) {
      fv_set_error("7x7 halo conv variant unsupported (cin=%d)", d->cin);
      return FV_E_BADARG;
    }
    return fv_check_launch("conv2d_fwd_halo");
  }
  case FV_CONVK_UPBAND: {
    FV_REQUIRE(!res && !a.spm, "sub-pixel band conv: no residual / store-pass records");
    a.Ho = d->h; a.Wo = d->w;
    a.Kpad = kpad_of(2, d->cin);
    a.wphase = p.wrows * a.Kpad;
    if ((st = wext(4L * p.wrows, a.Kpad, "upband"))) return st;
    const int hl = d->h / 2, wl = d->w / 2;
    const long base = (long)d->n * (wl / 32) * (d->cout / 64);
    int nb = 1;
    while (base * nb < 256 && hl % (nb * 16) == 0) nb *= 2;      // bands of a multiple of 8 rows
    const int nblk = (int)(base * nb);
    const unsigned xb = (unsigned)((long)d->n * hl * wl * 128 * 2);
    launch_upband(a, nblk, xb, nb, s);
    return fv_check_launch("conv2d_fwd_upband");
  }
  case FV_CONVK_SUBPIX_HALO: {
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
    FV_REQUIRE((long)4 * (d->cin / 32) * a.wus / 2 <= p.welems, "sub-pixel halo conv: weight image");
    if ((st = launch_h3(256, 1, nblk, s, a, xb))) return st;
    return fv_check_launch("conv2d_fwd_subpix_halo");
  }
  case FV_CONVK_SUBPIX_V2: {
    FV_REQUIRE(!res, "sub-pixel conv: no residual");
    const FwdTile t2{p.bn, p.bm};
    a.H = a.Hin; a.W = a.Win;                       // tile space = the low-res input image
    a.Ho = d->h; a.Wo = d->w;
    a.P = d->n * a.H * a.W;
    a.lgw = fv_ilog2(a.W); a.lghw = fv_ilog2(a.H * a.W);
    a.Kpad = kpad_of(2, d->cin);
    a.nks = a.Kpad / BK2;
    a.ntn = fv_cdiv(d->cout, t2.bn);
    a.wphase = p.wrows * a.Kpad;
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
  case FV_CONVK_HALO3_FWD3:
  case FV_CONVK_HALO3_FWD2: {
    const int bn = p.bn, tr = p.tr;
    FV_REQUIRE(!(res && stats), "conv v2: residual and BN statistics in one call are not supported");
    a.lgtw = 6;
    a.wus = p.wrows * 64;
    a.ntn = d->cout / bn;
    // stage-major: units of p.wrows rows x 32; the tiles read rows [0, ntn * bn) of each
    if ((st = wext(a.ntn * bn, 9L * d->cin, "halo3")) || (st = wext(p.wrows, 9L * d->cin, "halo3 units")))
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
    FV_REQUIRE(halo_epi_ok(a, bn, tr), "halo 3x3 conv: %dx%d, cout %d is not whole tiles of %d rows x 64 px x %d co", d->h,
               d->w, d->cout, tr, bn);
    if (p.kind == FV_CONVK_HALO3_FWD2) {
      st = launch_h2(bn, nblk, s, a, xb);
    } else if (tr == 8) {
      // 64-channel co tile (AFE.down1's data gradient): 8 waves over 8 rows x 64 px, the
      // linear-halo kernel (fwd2's XOR-swizzled halo addressing was its VALU
      // limiter); waves 0-3 issue the 4 weight pieces of a tap
      const int nblk8 = a.ntn * d->n * (d->h / 8) * (d->w / 64);
      st = launch_h3(64, 0, nblk8, s, a, xb);
    } else {
      st = launch_h3(bn, 0, nblk, s, a, xb);
    }
    if (st) return st;
    return fv_check_launch("conv2d_fwd_halo3");
  }
  case FV_CONVK_C1S: {
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
  case FV_CONVK_V2: {
    FV_REQUIRE(!(res && stats), "conv v2: residual and BN statistics in one call are not supported");
    const FwdTile t2{p.bn, p.bm};
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
  case FV_CONVK_V1: {
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
  default:      // the low-res data-gradient kinds launch from fv_conv2d_bwd_data
    fv_set_error("conv: no forward launch of kind %d", (int)p.kind);
    return FV_E_BADARG;
  }
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
  return conv_run(d, plan_fwd(d), x, wk, bias, pro_scale, pro_shift, res, y, stats, (hipStream_t)stream);
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
  return conv_run(d, plan_fwd(d), x, wk, bias, nullptr, nullptr, res, y, nullptr, (hipStream_t)stream, sr);
}

int fv_conv2d_bwd_data_sr(const fv_conv_desc* d, const void* dy, int ldy_dy, const void* wt, void* dx,
                          const fv_store_reduce* sr, void* stream) {
  int st = check_desc(d);
  if (st) return st;
  FV_REQUIRE(dy && wt && dx && sr && sr->mode == 2 && !d->upsample, "bwd_data_sr: bad argument");
  const fv_conv_desc t = dgrad_desc(d);
  FV_REQUIRE(ldy_dy == t.cin, "bwd_data: dy channel stride must be %d (got %d)", t.cin, ldy_dy);
  return conv_run(&t, plan_fwd(&t), dy, wt, nullptr, nullptr, nullptr, nullptr, dx, nullptr, (hipStream_t)stream, sr);
}

int fv_conv2d_bwd_data(const fv_conv_desc* d, const void* dy, int ldy_dy, const void* wt, void* dx,
                       void* stream) {
  int st = check_desc(d);
  if (st) return st;
  const fv_conv_desc t = dgrad_desc(d);
  FV_REQUIRE(ldy_dy == t.cin, "bwd_data: dy channel stride must be %d (got %d)", t.cin, ldy_dy);
  const FwdPlan p = plan_dgrad(d);
  if (p.kind == FV_CONVK_DGRAD_LOWRES_HALO) {
    const int bn = p.bn;
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
    FV_REQUIRE((long)(a.Cin / 32) * 4 * a.wus / 2 <= p.welems, "low-res halo dgrad: weight image");
    FV_REQUIRE(halo_epi_ok(a, bn, 4), "low-res halo dgrad: %dx%d, cin %d is not whole tiles of 4 rows x 64 px x %d co", a.H,
               a.W, d->cin, bn);
    if ((st = launch_h3(bn, 2, nblk, (hipStream_t)stream, a, xb))) return st;
    return fv_check_launch("conv2d_bwd_data_lowres_halo");
  }
  if (p.kind == FV_CONVK_DGRAD_LOWRES_V2) {
    FV_REQUIRE(dy && wt && dx, "null pointer");
    ConvArgs a{};
    const FwdTile t2{p.bn, p.bm};
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
  return conv_run(&t, p, dy, wt, nullptr, nullptr, nullptr, nullptr, dx, nullptr, (hipStream_t)stream);
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
  if (t.v2 == WG_H3S) {
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
  if (t.v2 == WG_UP) {
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
  if (t.v2 == WG_C7) {
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
  if (t.v2 == WG_HALO7) {
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
  if (t.v2 == WG_C7) {
    launch_w7_reduce(const_cast<float*>(slab), const_cast<float*>(bias_slab), t.nsplit, d->cout, dw_param, db,
                     (hipStream_t)stream);
    return fv_check_launch("wgrad_reduce_c7");
  }
  if (t.sub && t.v2 == WG_UP) {
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
  const bool pk = t.v2 == WG_HALO7 && halo_wg_pk(d);
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
    FV_REQUIRE(!launch_wprep(d->dtype, w_param, sigma, wk, rows, Kp, d->cout, d->cin_valid, fv_ilog2(d->cin), 3,
                             9 * d->cin, 0, 0, nb, s),
               "stride-2 weight prep: dtype %d unsupported", d->dtype);
    if ((st = fv_check_launch("s2_weight_prep"))) return st;
  }
  if (wt) {
    const int cin_t = pad_pow2_8(d->cout);
    const int rows = wrows(d->cin), Kph = 4 * cin_t;
    const int nb = (int)std::min<long>(fv_cdiv(4L * rows * Kph, 256), 4096);
    FV_REQUIRE(!launch_wprep_s2t(d->dtype, w_param, sigma, wt, rows, Kph, d->cout, d->cin_valid, fv_ilog2(cin_t), nb, s),
               "stride-2 weight prep: dtype %d unsupported", d->dtype);
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
// 2x2 slabs, mapped back to 4x4 taps by convt_wgrad_reduce_kernel.  Weff = gain * W (* 1/max(||W[:, co]||, 1e-12)
// with norm == "demod", F.normalize over dims [0, 2, 3]: models_utils.py:461-470).
// ----------------------------------------------------------------------------------------
extern "C" {

int fv_convt_supported(const fv_conv_desc* d) {
  if (check_desc(d) != FV_OK) return 0;
  if (!d->upsample || d->ksize != 3 || d->dtype != FV_BF16 || d->pro_act || d->epi_sigmoid || d->out_nchw_f32 ||
      pad_pow2_8(d->cout) != d->cout || d->ldy != d->cout)
    return 0;
  const FwdKind k = plan_fwd(d).kind;
  const bool subpix = k == FV_CONVK_SUBPIX_V2 || k == FV_CONVK_SUBPIX_HALO || k == FV_CONVK_UPBAND;
  return (subpix && plan_dgrad(d).kind >= FV_CONVK_DGRAD_LOWRES_HALO && plan_wgrad(d).sub) ? 1 : 0;
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
    launch_convt_norm(w, d->cin_valid, d->cout, inv, d->cout, s);
    if ((st = fv_check_launch("convt_norm"))) return st;
  }
  // the halo kernels' phase layouts (conv3_halo_fwd3 MODE 1 / 2) where those kernels take the launch
  const float* cinv = demod ? inv : nullptr;
  const FwdPlan pk = plan_fwd(d), pt = plan_dgrad(d);
  if (wk && pk.kind == FV_CONVK_SUBPIX_HALO) {
    const int nb1 = (int)std::min<long>(fv_cdiv(pk.welems, 256), 4096);
    FV_REQUIRE(!launch_wprep_phase(1, true, w, nullptr, (bf16*)wk, 4 * d->cout, 4 * (d->cin / 32), d->cout,
                                   d->cin_valid, 0, cinv, gain, nb1, s),
               "conv_transpose2d weight prep: phase layout unsupported");
    if ((st = fv_check_launch("convt_weight_prep_phase1"))) return st;
    wk = nullptr;
  }
  if (wt && pt.kind == FV_CONVK_DGRAD_LOWRES_HALO) {
    const int nb2 = (int)std::min<long>(fv_cdiv(pt.welems, 256), 4096);
    FV_REQUIRE(!launch_wprep_phase(2, true, w, nullptr, (bf16*)wt, d->cin, 4 * (4 * d->cout / 32), d->cout,
                                   d->cin_valid, d->cout / 32, cinv, gain, nb2, s),
               "conv_transpose2d weight prep: phase layout unsupported");
    if ((st = fv_check_launch("convt_weight_prep_phase2"))) return st;
    wt = nullptr;
  }
  if (!wk && !wt) return FV_OK;
  const int cin_t = pad_pow2_8(d->cout);
  const int rows = wrows(d->cout), Kp = kpad_of(2, d->cin);
  const int rows_t = wrows(d->cin);
  const long tot = (wk ? 4L * rows * Kp : 0) + (wt ? (long)rows_t * 16 * cin_t : 0);
  const int nb = (int)std::min<long>(fv_cdiv(tot, 256), 4096);
  launch_convt_wprep(w, demod ? inv : nullptr, gain, (bf16*)wk, rows, Kp, fv_ilog2(d->cin), (bf16*)wt, rows_t,
                     fv_ilog2(cin_t), d->cin_valid, d->cout, nb, s);
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
  launch_convt_wgrad_reduce(slab, bias_slab, dw, db, t.nsplit, t.CW, t.KW, d->cout, d->cin_valid, fv_ilog2(d->cin),
                            nb_main, nb_bias, s);
  if ((st = fv_check_launch("convt_wgrad_reduce"))) return st;
  launch_convt_weight_bwd(w, demod ? inv : nullptr, gain, dw, d->cin_valid, d->cout, d->cout, s);
  return fv_check_launch("convt_weight_bwd");
}

}  // extern "C"
