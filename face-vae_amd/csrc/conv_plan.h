// Internal header of the 2-D convolution's translation units, for what only they share (not
// pose.hip or conv3d_gemm.hip, which include conv_common.h): the weight-gradient family's
// argument structs, the plan types that conv.hip's planners fill, and every launcher of
// conv_wgrad.hip.  Everything declared here that has linkage is hidden.
#pragma once
#include "conv_common.h"

#pragma GCC visibility push(hidden)

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

// wgrad plan: v2 (bf16 DMA-fed, 8 waves), halo (7x7), or the register-staged v1 (fp32 / BN prologue)
struct WgPlan {
  int v2, bkt, bc, px, ntk, ntc, nsplit, nsteps, sps, KW, CW, cfg, sub;
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

#pragma GCC visibility pop
