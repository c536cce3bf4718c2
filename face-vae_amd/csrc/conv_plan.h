// Internal header of the 2-D convolution's translation units, for what only they share (not
// pose.hip or conv3d_gemm.hip, which include conv_common.h): the weight-gradient family's
// argument structs, the job structs of the weight re-layout kernels, the plan types that
// conv.hip's planners fill, the tile constants of the special-shape kernels that the planners
// read, every launcher of conv_halo3.hip, conv_shapes.hip, conv_wgrad.hip and conv_prep.hip, and
// the checks and planners of conv.hip, four of which conv_fp8.hip calls.  Everything declared here that has
// linkage is hidden.
#pragma once
#include "conv_common.h"

#pragma GCC visibility push(hidden)

// ---- tile constants of conv_shapes.hip's kernels that conv.hip's planners and weight prep read ----
constexpr int C74_TR = 4;     // conv7c4_fwd: output rows per tile (x 64 columns)
constexpr int C74_K = 224;    // conv7c4_fwd: row length of the packed 7x7 weight image (7 x 32)
constexpr int C64_G = 8;      // conv3c64_fwd: iterations (4 rows each) per BN record group
constexpr int UPB_G = 4;      // conv3up_band_fwd: iterations (2 low-res rows each) per BN record group
constexpr int C7_TR = 4;      // conv7_n3_fwd2: output rows per band step (H % C7_TR == 0)

// ---- launchers of conv_halo3.hip: they pick the instantiation, the caller decides the rest.
// Non-zero for a combination that is not instantiated. ----
// conv3_halo_fwd3: bn = co tile (256 / 128 on 4 rows, 64 on 8 rows), mode 0 / 1 / 2 (bn 256), 0 / 2
// (128), 0 (64), sch 0 / 2, pers only below bn 256; grid blocks over ntiles tiles
int launch_halo3_fwd3(const ConvArgs& a, int bn, int mode, int sch, bool pers, int grid, unsigned xb, int ntiles,
                      hipStream_t s);
int launch_halo3_fwd2(const ConvArgs& a, int bn, int nblk, unsigned xb, hipStream_t s);   // bn 256 / 128 / 64

// ---- launchers of conv_shapes.hip, one per kernel ----
int launch_halo7(const ConvArgs& a, int cin, int nblk, unsigned xb, hipStream_t s);          // conv_halo_fwd, cin 8 / 64
void launch_c74(const ConvArgs& a, int grid, unsigned xb, int ntiles, hipStream_t s);        // conv7c4_fwd
void launch_c64(const ConvArgs& a, int nblk, unsigned xb, int nbands, hipStream_t s);        // conv3c64_fwd
void launch_upband(const ConvArgs& a, int nblk, unsigned xb, int nbands, hipStream_t s);     // conv3up_band_fwd
int launch_c1s(const ConvArgs& a, int k, int bpx, int grid, unsigned xb, hipStream_t s);     // conv1x1_stream<k, bpx>
void launch_c7n(const ConvArgs& a, int nblk, unsigned xb, int band, hipStream_t s);          // conv7_n3_fwd2

// ---- job structs of the weight re-layout kernels (conv_prep.hip), filled by conv.hip's entries ----
// weight_prep2_kernel: both layouts in one launch, blocks [0, j0.nb) write wk, the rest wt
struct WPrepJob { void* out; int rows, Kpad, lgCin, K, transposed, nb, smaj; };
// weight_prep_multi_kernel: one launch for the generic weight layouts of many convs
// (fv_conv_weight_prep_multi): job j owns blocks [blk0, blk0 + nb); at most 2 * FV_WPREP_MAX
// jobs, passed by value
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

// ---- launchers of conv_prep.hip, one per kernel family: the caller decides the grid (nblk blocks
// of the kernel's block size) and every argument; a launcher that has a dtype (FV_BF16 / FV_F32)
// or a (mode, convt) to choose from returns non-zero for one that is not instantiated ----
void launch_wprep_c7n(const float* wp, const float* sigma, bf16* wn, int cout, int nblk, hipStream_t s);
int launch_wprep(int dtype, const float* wp, const float* sigma, void* wk, int rows, int Kpad, int cout, int cin_valid,
                 int lgCin, int KS, int K, int transposed, int smaj, int nblk, hipStream_t s);   // weight_prep_kernel
int launch_wprep_s2t(int dtype, const float* wp, const float* sigma, void* wt, int rows, int Kph, int cout,
                     int cin_valid, int lgC, int nblk, hipStream_t s);
int launch_wprep2(int dtype, const float* wp, const float* sigma, int cout, int cin_valid, int KS, const WPrepJob& j0,
                  const WPrepJob& j1, int nblk, hipStream_t s);
int launch_wprep_multi(int dtype, const WPrepMulti& m, int nbx, hipStream_t s);                  // grid (nbx, m.n)
void launch_wprep_subpix(const float* wp, const float* sigma, bf16* wk, int rows, int Kpad, int cout, int cin_valid,
                         int lgCin, int nblk, hipStream_t s);
void launch_wprep_s2(const float* wp, const float* sigma, bf16* wt, int rows, int Kpad, int cout, int cin_valid,
                     int lgCt, int nblk, hipStream_t s);
// weight_prep_phase_kernel<mode, convt>: mode 1 / 2; cinv and gain are read with convt only
int launch_wprep_phase(int mode, bool convt, const float* wp, const float* sigma, bf16* out, int rows, int units,
                       int cout, int cin_valid, int cpp, const float* cinv, float gain, int nblk, hipStream_t s);
void launch_convt_norm(const float* w, int cin, int cout, float* inv, int nblk, hipStream_t s);
void launch_convt_wprep(const float* w, const float* inv, float gain, bf16* wk, int rows, int Kpad, int lgCin, bf16* wt,
                        int rows_t, int lgCt, int cin_valid, int cout, int nblk, hipStream_t s);
void launch_convt_wgrad_reduce(const float* slab, const float* bslab, float* dw, float* db, int nsplit, int CW, int KW,
                               int cout, int cin_valid, int lgCin, int nb_main, int nb_bias, hipStream_t s);
void launch_convt_weight_bwd(const float* w, const float* inv, float gain, float* g, int cin, int cout, int nblk,
                             hipStream_t s);

// ---- argument structs of the weight-gradient kernels (conv_wgrad.hip) ----
struct WgArgs {
  const void* x;
  const float* psc;
  const float* psh;
  float slope;
  const void* dy;
  float* slab;
  float* bslab;
  int N, H, W, Hin, Win, P;
  int lgCin, Cin;
  int K, KW;          // KW = slab row stride (>= Kpad, multiple of the k tile)
  int Cout, ldd;      // valid output channels, channel stride of dy
  int CW;             // slab co rows
  int ntk, ntc, steps_per_split, nsteps;
};

struct Wg2Args {
  const void* x;
  const void* dy;
  float* slab;
  float* bslab;
  int H, W, Hin, Win, P;
  int lgCin, K, KW, ldd, CW;
  int ntk, ntc, nsteps, sps;
  FastDiv fhw, fw, fh;
  unsigned xbytes, dybytes;
  int rowal;   // W % PX == 0: each stage lies in one image row
  // sub-pixel phases of an upsample + 3x3 conv (SUB): pixels are the LOW-res image (H x W),
  // the block's phase (pa, pb) pairs low-res pixel (n, i, j) with dy pixel (n, 2i+pa, 2j+pb)
  // of the Ho x Wo image; phase slabs follow each other ([4][nsplit][CW][KW])
  int Ho, Wo, nsplit;
  int il;      // row-aligned stages: spread the next stage's DMA pieces between MFMAs
};

struct H3Wg2Args {
  const void* x;
  const void* dy;
  float* slab;
  float* bslab;
  int H, W, Cout, ldd, nseg, rows, nct;
  int ldx, nci;          // x channel stride (= Cin) and 64-channel input tiles (Cin / 64)
  unsigned xbytes, dybytes;
};

struct UpWgArgs {
  const void* x;
  const void* dy;
  float* slab;
  float* bslab;
  int Hin, Win, Cout, Cin, ldd;
  int nct, nci, units, spb, nsplit;     // units = images x output strips; spb units per block
  unsigned xbytes, dybytes;
};

struct W7Args {
  const void* x;
  const void* dy;
  float* slab;
  float* bslab;
  int H, W, ldd, cout, seg_rows, nseg;
  unsigned xbytes, dybytes;
};

struct HaloWgArgs {
  const void* x;
  const void* dy;
  float* slab;
  float* bslab;
  int H, W, ldd, K, KW, CW, ntiles, cout;
  unsigned xbytes, dybytes;
};

// wgrad plan: which kernel family (v2), its tiles and its slab geometry
enum WgKind {
  WG_V1 = 0,      // conv_wgrad_kernel, register-staged (fp32 / BN prologue / operands >= 2 GB)
  WG_V2 = 1,      // conv_wgrad_v2 (bf16 DMA-fed, 8 waves; with sub: the 4 sub-pixel phases)
  WG_HALO7 = 2,   // conv_halo_wgrad (7x7 in_conv / out_conv halo)
  WG_C7 = 3,      // conv7_n3_wgrad (out_conv 7x7, 64 -> <= 4)
  WG_H3S = 5,     // conv3_halo_wgrad2 (3x3 sliding rows)
  WG_UP = 6,      // conv3_up_wgrad (sub-pixel sliding rows)
};
struct WgPlan {
  int v2, bkt, bc, px, ntk, ntc, nsplit, nsteps, sps, KW, CW, cfg, sub;
};

// forward plan (plan_fwd; plan_dgrad for a data gradient): the one decision the launch, the
// weight preparation and every geometry query of a descriptor read.  The kinds are the
// FV_CONVK_* constants of facevae.h, which fv_conv2d_fwd_kernel reports.
using FwdKind = fv_conv_kernel;
struct FwdPlan {
  // the kind by the descriptor (and FV_C1S); what a call launches: fwd_kind()
  FwdKind kind;
  // co tile, output rows and pixels per tile.  FV_CONVK_C64 and FV_CONVK_C1S carry conv_fwd_v2's
  // tile, the one their fallback launches (their own tiles are fixed: 64 / 256 co).
  int bn, tr, bm;
  // ---- functions of the descriptor alone: weights are prepared once, buffers sized once ----
  int rec_px;          // pixels per BN-statistics record
  int wlay;            // weight image: 0 plain [rows][wlen], 1 stage-major, 2 packed 7x7
  int wrows, wlen;     // its rows and row length (0: the phase / out_conv images, sized by welems alone)
  long welems;         // elements of the image (fv_conv_wk_elems / fv_conv_wt_elems)
  int sr_n, sr_px;     // store-pass records and pixels per record, 0 when the kind has none
};

// wgrad v2 tile configs: k rows x co cols per block, 8 waves as wk x wc, pixels per stage,
// LDS ring depth.  The 32-B-block XOR swizzle of the transposed images needs bkt % 128 == 0.
struct Wg2Cfg { int bkt, bc, wk, wc, px, ns; };
constexpr Wg2Cfg kWg2Cfg[] = {
    {256, 256, 2, 4, 64, 2},   // 0  (64 KB stages)
    {128, 256, 2, 4, 64, 3},   // 1
    {256, 128, 4, 2, 64, 3},   // 2
    {128, 128, 2, 4, 64, 4},   // 3
    {128, 64, 8, 1, 64, 4},    // 4
    {256, 16, 8, 1, 64, 2},    // 5
    {256, 256, 2, 4, 32, 4},   // 6  (32 KB stages, 3 in flight)
    {384, 64, 8, 1, 64, 2},    // 7
    {256, 64, 8, 1, 64, 3},    // 8  (sub-pixel phases of the 64-channel up conv, K = 512)
};
constexpr int kNumWg2Cfg = sizeof(kWg2Cfg) / sizeof(kWg2Cfg[0]);

// ---- launchers of conv_wgrad.hip: conv_wgrad_v2, conv_wgrad_kernel (T = bf16 / float), ... ----
int launch_wg2(const Wg2Args& a, int ks, const WgPlan& p, int ups, int nblk, hipStream_t s);
template <typename T>
int launch_wg(const WgArgs& a, int ks, const WgPlan& t, int pro, int ups, int nblk, hipStream_t s);
template <typename T>
void launch_s2_wg(const WgArgs& a, const WgPlan& t, int nblk, hipStream_t s);
void launch_h3_wg2(const H3Wg2Args& a, int nblk, hipStream_t s);                         // conv3_halo_wgrad2
void launch_up_wg(const UpWgArgs& a, int nblk, hipStream_t s);                           // conv3_up_wgrad
void launch_c7_wg(const W7Args& a, int nblk, hipStream_t s);                             // conv7_n3_wgrad
void launch_halo_wg(const HaloWgArgs& a, int cin, bool pk, int nblk, hipStream_t s);     // conv_halo_wgrad
void launch_w7_reduce(float* slab, float* bslab, int nsplit, int cout, float* dw, float* db, hipStream_t s);
void launch_subpix_split_sum(float* slab, float* bslab, int nsplit, long rowlen, int CW, int nb_main, int nb_bias,
                             hipStream_t s);
void launch_subpix_fold(const float* slab, const float* bslab, float* dw, float* db, int nsplit, int CW, int KW, int cout,
                        int cin_valid, int lgCin, int nb_main, int nb_bias, hipStream_t s);
void launch_wgrad_reduce_subpix(const float* slab, const float* bslab, float* dw, float* db, int nsplit, int CW, int KW,
                                int cout, int cin_valid, int lgCin, int nb_main, int nb_bias, hipStream_t s);
void launch_wgrad_reduce(const float* slab, const float* bslab, float* dw, float* db, int nsplit, int CW, int KW, int K,
                         int cout, int cin_valid, int lgCin, int KS, int nb_main, int nb_bias, int KSL, hipStream_t s);

// ---- what conv_fp8.hip calls of conv.hip's checks, switches and planners (defined there, once) ----
int check_desc(const fv_conv_desc* d);                 // FV_OK or the error of a bad descriptor
int res_sched(int dflt);                               // FV_RES_SCHED, read per call; dflt when unset
int sr_geometry(const fv_conv_desc* d, int* bp);       // store-pass records (and pixels per record) of d's launch
WgPlan plan_wgrad(const fv_conv_desc* d);
FwdPlan plan_fwd(const fv_conv_desc* d);               // the forward of d
FwdPlan plan_dgrad(const fv_conv_desc* d);             // its data gradient: a low-res kind or plan_fwd(dgrad_desc(d))
FwdKind fwd_kind(const FwdPlan& p, bool res, bool stats, int sr_mode);   // the kernel one call launches

#pragma GCC visibility pop
