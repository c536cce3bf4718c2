// Internal header of the 2-D convolution's translation units (conv.hip, conv_fwd.hip,
// conv_fwd_v2.hip, conv_halo3.hip, conv_shapes.hip, conv_wgrad.hip, conv_prep.hip, conv_fp8.hip):
// the forward kernels' argument struct, the device helpers the kernel families share, and the
// declarations of the generic forward families' host launchers (the halo 3x3, special-shape,
// weight-gradient and weight-preparation launchers, their argument structs and the plan types:
// conv_plan.h).
// Kernels have internal linkage, so a kernel is launched only from its own file, through a
// launcher.  Everything declared here that has linkage is hidden: the library exports the fv_*
// entries only.
#pragma once
#include <stdlib.h>

#include <algorithm>
#include <type_traits>

#include "common.h"

#pragma GCC visibility push(hidden)

struct ConvArgs {
  const void* x;
  const void* w;
  const float* bias;
  const float* psc;
  const float* psh;
  float slope;
  const void* res;
  void* y;
  float* stats;
  int N, H, W, Hin, Win, P;
  int lgCin, Cin;
  int Cout, ldy;
  int K, Kpad, nks;
  int sigmoid, nchw;
  int ntn;
  int lgtw;       // > 0: a block's pixels are a (BM >> lgtw) x (1 << lgtw) rectangle at p0
  // sub-pixel phase of an upsample-conv (v2 MODE 2): the tile space is the LOW-res image
  // (H x W = Hin x Win, powers of two: lgw, lghw) and tile pixel (n, h, w) of phase
  // (pa, pb) stores to output pixel (n, 2h + pa, 2w + pb) of the Ho x Wo image
  int sub;        // 0 = none, else 1 + 2 * pa + pb (set per block)
  int lgw, lghw, Ho, Wo;
  int wphase;     // elements per phase block of the weight buffer (MODE 2)
  const float* dq0;   // fp8 path: per-tensor dequant factors of the two operands (device)
  const float* dq1;
  // store-pass records (STAGED epilogue, fv_store_reduce): per (m-tile, wave) and output
  // channel, 1 = (sum, sum of squares) of the stored (bf16, residual-added) output -- the next
  // BN's statistics; 2 = BN-backward sums (g, g * yhat) of the stored gradient v with
  // g = v * act'(gamma * yhat + beta), yhat = (res - mean) * invstd (`res` = the BN input,
  // prefetched like a residual, not added)
  int spm;
  float* sprec;
  const float *bnm, *bni, *bng, *bnb;
  float bns;
  int wus;        // halo 3x3 kernels: bytes per tap unit of the stage-major weights (rows * 64)
  unsigned* roll; // fp8: the operand's delayed-scaling site, rolled by block 0 (fp8_site_roll)
  int nrec;       // BN records the caller sized `stats` for (fv_conv2d_stats_blocks / fp8): every
                  // record write is bounded by it (not only by the kernel's own tiling)
};

struct FwdTile { int bn, bm; };   // output channels x pixels per block

// ---- launchers: conv_fwd_kernel (conv_fwd.hip: T = bf16 / float, S2 = 1 / 2) ----
template <typename T>
int launch_fwd(const ConvArgs& a, int ks, FwdTile t, int pro, int ups, int nblk, hipStream_t s);
template <typename T, int S2>
void launch_s2_fwd(const ConvArgs& a, FwdTile t, int nblk, hipStream_t s);
// ---- launcher: conv_fwd_v2 (conv_fwd_v2.hip) ----
int launch_v2(const ConvArgs& a, int ks, FwdTile t, int ups, int nblk, unsigned xb, hipStream_t s);

#pragma GCC visibility pop

namespace {

constexpr int BK = 32;  // k per main-loop step (one bf16 MFMA K, eight f32 MFMA K=4)

// output pixel of tile-space pixel p (identity unless a sub-pixel phase is set)
// GSUB: the tile space is any H x W image (divisions), not a power-of-two one (lgw, lghw):
// the phases of the stride-2 conv's data gradient (conv_fwd_kernel S2 == 2)
template <bool GSUB = false>
__device__ __forceinline__ int out_pix(const ConvArgs& a, int p) {
  if (!a.sub) return p;
  const int ph = a.sub - 1, pa = ph >> 1, pb = ph & 1;
  if constexpr (GSUB) {
    const int hw = a.H * a.W;
    const int n = p / hw, rem = p - n * hw;
    const int h = rem / a.W, w = rem - h * a.W;
    return (n * a.Ho + 2 * h + pa) * a.Wo + 2 * w + pb;
  }
  const int n = p >> a.lghw, rem = p & ((1 << a.lghw) - 1);
  const int h = rem >> a.lgw, w = rem & ((1 << a.lgw) - 1);
  return (n * a.Ho + 2 * h + pa) * a.Wo + 2 * w + pb;
}

// 16-B chunk swizzle of a 64-B bf16 LDS row (4 chunks): conflict-free ds_read_b128 for the
// MFMA fragment read (16 consecutive rows, chunk = lane>>4).  f(row) = [0,2,3,1][(row>>2)&3].
template <typename T>
__device__ __forceinline__ int rswz(int row) {
  if constexpr (sizeof(T) == 2) return (0x1320 >> (((row >> 2) & 3) * 4)) & 3;
  else return 0;
}

template <typename T>
__device__ __forceinline__ void load4(const T* p, float* f);
template <>
__device__ __forceinline__ void load4<float>(const float* p, float* f) {
  float4 v = *reinterpret_cast<const float4*>(p);
  f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w;
}
template <>
__device__ __forceinline__ void load4<bf16>(const bf16* p, float* f) {
  uint2 v = *reinterpret_cast<const uint2*>(p);
  f[0] = __uint_as_float(v.x << 16); f[1] = __uint_as_float(v.x & 0xffff0000u);
  f[2] = __uint_as_float(v.y << 16); f[3] = __uint_as_float(v.y & 0xffff0000u);
}
template <typename T>
__device__ __forceinline__ void store4(T* p, const float* f);
template <>
__device__ __forceinline__ void store4<float>(float* p, const float* f) {
  *reinterpret_cast<float4*>(p) = make_float4(f[0], f[1], f[2], f[3]);
}
template <>
__device__ __forceinline__ void store4<bf16>(bf16* p, const float* f) {
  bf16 t[4] = {(bf16)f[0], (bf16)f[1], (bf16)f[2], (bf16)f[3]};
  *reinterpret_cast<uint2*>(p) = *reinterpret_cast<const uint2*>(t);
}

// one MFMA step over a 32-deep k slice for a 16x16 tile
template <typename T>
struct Frag;
template <>
struct Frag<bf16> {
  bf16x8 v;
  __device__ __forceinline__ void lds(const char* p) { v = *reinterpret_cast<const bf16x8*>(p); }
};
template <>
struct Frag<float> {
  float v[8];
  __device__ __forceinline__ void lds(const char* p) {
    float4 a = reinterpret_cast<const float4*>(p)[0];
    float4 b = reinterpret_cast<const float4*>(p)[1];
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  }
};
__device__ __forceinline__ f32x4 mma(const Frag<bf16>& a, const Frag<bf16>& b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.v, b.v, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mma(const Frag<float>& a, const Frag<float>& b, f32x4 c) {
  // k-slot h (= lane>>4) of MFMA j carries k = 8h + j: same map for A and B.
#pragma unroll
  for (int j = 0; j < 8; ++j) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.v[j], b.v[j], c, 0, 0, 0);
  return c;
}

typedef float f32x2 __attribute__((ext_vector_type(2)));
// c + a * b with the product rounded before the add (never contracted to an FMA)
__device__ __forceinline__ f32x2 mul_then_add(f32x2 a, f32x2 b, f32x2 c) {
#pragma clang fp contract(off)
  const f32x2 p = a * b;
  return c + p;
}

// shared epilogue: bias [+ residual] -> BN partials -> [sigmoid] -> store (NHWC T or NCHW f32)
// STAGED (bf16 NHWC only): after bias and BN partials the tile is rounded to bf16, written
// to LDS (16-B chunks XOR-swizzled by pixel row) and stored with coalesced 16-B row
// segments; the residual (if any) is added in that pass.  smem must hold BM*BN*2 bytes.
// mid (persistent kernels): with a callable other than NoMid, every thread reads its store
// chunks back into registers, the block syncs (LDS free again) and mid() runs -- it issues
// the next tile's LDS-DMA prologue -- before the stores, which then drain under that DMA.
// HALO (STAGED, the 3x3 halo kernels conv3_halo_fwd2 / fwd3): the block's pixels are whole
// 64-pixel image rows (lgtw == 6), no sub-pixel phase, and the host checked that the tiles cover
// the output exactly (halo_epi_ok: P % BM == 0, Cout % BN == 0).  Then no element needs a bounds
// test, a thread's store-pass chunks are one per-lane byte offset (its chunk of tile row 0) from a
// wave-uniform 64-bit base that advances by whole pixels / image rows, and the wave's RN * 16
// bias values are one coalesced load, handed out by lane permutes.  Same operands, same order:
// bit-identical to the general path.
struct NoMid {
  __device__ void operator()() const {}
};
template <typename T, int WN, int WM, int RN, int RM, bool STAGED = false, typename Mid = NoMid, bool GSUB = false,
          bool HALO = false>
__device__ __forceinline__ void conv_epilogue(const ConvArgs& a, f32x4 (&acc)[RN][RM], char* smem, int co0, int p0,
                                              int tm, int wn, int wm, int lane, int tid, Mid mid = Mid{}) {
  constexpr bool kMid = !std::is_same<Mid, NoMid>::value;
  constexpr int NT = 64 * WN * WM;
  constexpr int BN = WN * RN * 16;
  constexpr int BM = WM * RM * 16;
  const int HW = a.H * a.W;
  const int lr = lane & 15, lh = lane >> 4;
  // STAGED + residual: this thread's residual chunks of the store pass are loaded first, so
  // their HBM latency hides under the BN partials and the LDS staging (loaded inside the
  // store loop they were serialised behind its stores: +22 us per res conv at 64x64, B=32)
  constexpr int SCPR = BN / 8, NRES = STAGED ? (BM * SCPR + NT - 1) / NT : 1;
  // HALO: a thread keeps its 16-B chunk column (NT % SCPR == 0) and moves PS tile pixels per
  // store-pass iteration; PS divides the 64-pixel tile row, so iteration `it` is image row
  // (it * PS) >> 6, column + (it * PS) & 63 of the tile for every thread
  constexpr int PS = NT / SCPR;
  static_assert(!HALO || (STAGED && !GSUB && RN * 16 == 64 && NT % SCPR == 0 && PS <= 64 && 64 % PS == 0 &&
                          (BM * SCPR) % NT == 0),
                "halo epilogue: tile geometry");
  float hbias = 0.f;
  if constexpr (HALO) {
    // (first: the bias add is the epilogue's first consumer of a load)
    if (a.bias) hbias = a.bias[co0 + wn * 64 + lane];
  }
  // (per-thread constants from an opaque copy of tid: as invariants of a persistent kernel's
  // tile loop they would be hoisted out of it and held in registers through the main loop)
  int htid = tid;
  if constexpr (HALO) asm volatile("" : "+v"(htid));
  const int hpl = htid / SCPR, hch = htid % SCPR;      // this thread's tile pixel (of PS) and chunk column
  const unsigned hvo = HALO ? (unsigned)((hpl * a.ldy + hch * 8) * 2) : 0u;
  const long hub = HALO ? ((long)p0 * a.ldy + co0) * 2 : 0L;
  // address of this thread's chunk `it`: uniform base + uniform pixel step + per-lane offset
  auto haddr = [&](const void* base, int it) -> char* {
    const int pl = it * PS;
    const char* ub = reinterpret_cast<const char*>(base) + hub + ((long)(pl >> 6) * a.W + (pl & 63)) * a.ldy * 2;
    return const_cast<char*>(ub) + hvo;
  };
  // LDS byte offset of that chunk in the staged tile: pl = hpl + it * PS, and the bits it * PS
  // adds to pl & (SCPR - 1) lie above hpl < PS, so they XOR into the swizzle as a constant; the
  // iteration's offset it * PS * BN * 2 is an immediate below 64 KB from one of two bases
  const int hsw = hch ^ (hpl & (SCPR - 1));
  int hl[2] = {hpl * BN * 2, hpl * BN * 2 + 65536};
  if constexpr (HALO && BM * BN * 2 > 65536) asm volatile("" : "+v"(hl[1]));
  auto hlds = [&](int it) -> int {
    constexpr int kRow = PS * BN * 2;
    return (hl[(it * kRow) >> 16] | ((hsw ^ ((it * PS) & (SCPR - 1))) << 4)) + ((it * kRow) & 0xffff);
  };
  uint4 rpre[NRES];
  // (with a mid hook the residual chunks are loaded after the LDS read-back instead, when the
  // accumulators are dead: their registers and the read-back's cannot all be live at once)
  auto load_res = [&]() {
    if constexpr (HALO) {
      if (a.res) {
#pragma unroll
        for (int it = 0; it < NRES; ++it) rpre[it] = *reinterpret_cast<const uint4*>(haddr(a.res, it));
      }
    } else if (a.res) {
#pragma unroll
      for (int it = 0; it < NRES; ++it) {
        const int idx = tid + it * NT;
        const int pl = idx / SCPR, ch = idx - (idx / SCPR) * SCPR;
        const int tp = a.lgtw ? p0 + (pl >> a.lgtw) * a.W + (pl & ((1 << a.lgtw) - 1)) : p0 + pl;
        const int co = co0 + ch * 8;
        rpre[it] = make_uint4(0, 0, 0, 0);
        if (idx < BM * SCPR && tp < a.P && co < a.Cout)
          rpre[it] = *reinterpret_cast<const uint4*>(reinterpret_cast<const bf16*>(a.res) +
                                                      (long)out_pix<GSUB>(a, tp) * a.ldy + co);
      }
    }
  };
  if constexpr (STAGED && !kMid) load_res();
  float bv[RN][4];
#pragma unroll
  for (int n = 0; n < RN; ++n)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if constexpr (HALO) {
        // lane l holds bias[wave's channel l]: this lane's 4 channels of tile n start at n * 16 + lh * 4
        bv[n][i] = __int_as_float(__builtin_amdgcn_ds_bpermute((lh * 4 + n * 16 + i) << 2, __float_as_int(hbias)));
      } else {
        const int co = co0 + wn * RN * 16 + n * 16 + lh * 4 + i;
        bv[n][i] = (a.bias && co < a.Cout) ? a.bias[co] : 0.f;
      }
    }
  bool pv[RM];
  int pix_of[RM];
#pragma unroll
  for (int m = 0; m < RM; ++m) {
    const int loc = wm * RM * 16 + m * 16 + lr;
    const int tp = a.lgtw ? p0 + (loc >> a.lgtw) * a.W + (loc & ((1 << a.lgtw) - 1)) : p0 + loc;
    pv[m] = HALO || tp < a.P;
    pix_of[m] = out_pix<GSUB>(a, tp);
  }
#pragma unroll
  for (int n = 0; n < RN; ++n) {
    const int cb = co0 + wn * RN * 16 + n * 16 + lh * 4;
#pragma unroll
    for (int m = 0; m < RM; ++m) {
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[n][m][i] += bv[n][i];
      if (!STAGED && a.res && pv[m]) {
        const T* rp = reinterpret_cast<const T*>(a.res) + (long)pix_of[m] * a.ldy + cb;
        if (cb + 3 < a.Cout) {
          float f[4];
          load4<T>(rp, f);
#pragma unroll
          for (int i = 0; i < 4; ++i) acc[n][m][i] += f[i];
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (cb + i < a.Cout) acc[n][m][i] += Elt<T>::to_f(rp[i]);
        }
      }
    }
  }

  // (records past cdiv(output pixels, RM*16) -- the empty wave rows of a partial last pixel
  // tile -- are not written: the caller sized the buffer with that many, fv_conv2d_stats_blocks;
  // the sub-pixel launches number records over the 4 phases of a low-res a.P, hence Ho x Wo)
  const long pout = a.Ho ? (long)a.N * a.Ho * a.Wo : (long)a.P;
  if (a.stats && (long)(tm * WM + wm) < (pout + RM * 16 - 1) / (RM * 16) && tm * WM + wm < a.nrec) {
    // BN statistics partials, one record per wave row (RM*16 pixels, record index
    // tm*WM + wm): per output channel (sum, sum of squares) over the record's valid pixels,
    // reduced over the 16 pixel lanes of each m-tile by shuffles -- no LDS, no barrier.
    const int rec = tm * WM + wm;
#pragma unroll
    for (int n = 0; n < RN; ++n) {
      float sv[4], qv[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float t = 0.f, q = 0.f;
#pragma unroll
        for (int m = 0; m < RM; ++m) {
          const float v = pv[m] ? acc[n][m][i] : 0.f;
          t += v;
          q += v * v;
        }
        sv[i] = row16_sum(t);
        qv[i] = row16_sum(q);
      }
      // every lane of a 16-lane row holds the row's 4 channel sums: lanes 0-3 store the sums,
      // lanes 4-7 the squares (one store instruction per n, 4 x 2 x 16 B)
      const int cb = co0 + wn * RN * 16 + n * 16 + lh * 4;
      const int ii = lr & 3;
      const float s01 = ii & 1 ? sv[1] : sv[0], s23 = ii & 1 ? sv[3] : sv[2];
      const float q01 = ii & 1 ? qv[1] : qv[0], q23 = ii & 1 ? qv[3] : qv[2];
      const float val = lr < 4 ? (ii & 2 ? s23 : s01) : (ii & 2 ? q23 : q01);
      if (lr < 8 && (HALO || cb + ii < a.Cout)) a.stats[(long)(rec * 2 + (lr >> 2)) * a.Cout + cb + ii] = val;
    }
  }

  if constexpr (STAGED) {
    static_assert(sizeof(T) == 2, "staged epilogue is bf16 NHWC");
    constexpr int CPR = BN / 8;                         // 16-B chunks per pixel row
    __syncthreads();                                    // stats scratch / last k-step reads done
#pragma unroll
    for (int n = 0; n < RN; ++n) {
      const int cl = wn * RN * 16 + n * 16 + lh * 4;    // local channel of this lane's 4 values
#pragma unroll
      for (int m = 0; m < RM; ++m) {
        const int pl = wm * RM * 16 + m * 16 + lr;
        bf16 t4[4] = {(bf16)acc[n][m][0], (bf16)acc[n][m][1], (bf16)acc[n][m][2], (bf16)acc[n][m][3]};
        char* dst = smem + pl * BN * 2 + (((cl >> 3) ^ (pl & (CPR - 1))) << 4) + ((cl & 4) << 1);
        *reinterpret_cast<uint2*>(dst) = *reinterpret_cast<const uint2*>(t4);
      }
    }
    __syncthreads();
    uint4 vv[kMid ? NRES : 1];
    if constexpr (kMid) {
#pragma unroll
      for (int it = 0; it < NRES; ++it) {
        const int idx = tid + it * NT;
        const int pl = idx / CPR, ch = idx - (idx / CPR) * CPR;
        if constexpr (HALO) vv[it] = *reinterpret_cast<const uint4*>(smem + hlds(it));
        else if (idx < BM * CPR) vv[it] = *reinterpret_cast<const uint4*>(smem + pl * BN * 2 + ((ch ^ (pl & (CPR - 1))) << 4));
      }
      __syncthreads();
      load_res();
      mid();
    }
    auto chunk = [&](int it, int pl, int ch) -> uint4 {
      if constexpr (kMid) return vv[it];
      else if constexpr (HALO) return *reinterpret_cast<const uint4*>(smem + hlds(it));
      else return *reinterpret_cast<const uint4*>(smem + pl * BN * 2 + ((ch ^ (pl & (CPR - 1))) << 4));
    };
    if constexpr (HALO) {
      // the store pass without bounds tests or per-chunk address arithmetic; its form -- residual
      // added or not (ADD), records (REC = a.spm) -- is chosen once, not per chunk, so each form
      // is one straight run of NRES chunks
      static_assert(CPR <= 64 && 64 % CPR == 0, "store-pass records: chunks per row must divide a wave");
      const int c = co0 + hch * 8;
      // the sums as channel pairs (packed f32 adds / FMAs: no MFMA runs beside them here)
      f32x2 sacc[4], qacc[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) sacc[k] = qacc[k] = f32x2{0.f, 0.f};
      auto pass = [&](auto add, auto recs) {
        constexpr bool ADD = decltype(add)::value;
        constexpr int REC = decltype(recs)::value;
        f32x2 bm_[4], bi_[4], bg_[4], bb_[4];
        if constexpr (REC == 2) {
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            bm_[k] = f32x2{a.bnm[c + 2 * k], a.bnm[c + 2 * k + 1]};
            bi_[k] = f32x2{a.bni[c + 2 * k], a.bni[c + 2 * k + 1]};
            bg_[k] = f32x2{a.bng[c + 2 * k], a.bng[c + 2 * k + 1]};
            bb_[k] = f32x2{a.bnb[c + 2 * k], a.bnb[c + 2 * k + 1]};
          }
        }
#pragma unroll
        for (int it = 0; it < NRES; ++it) {
          Chunk8<bf16> v, r;
          v.raw = chunk(it, 0, 0);
          if constexpr (ADD || REC == 2) r.raw = rpre[it];
          if constexpr (REC == 2) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              const f32x2 rr = {r.get(2 * k), r.get(2 * k + 1)}, gv = {v.get(2 * k), v.get(2 * k + 1)};
              const f32x2 yh = (rr - bm_[k]) * bi_[k];
              const f32x2 t = bg_[k] * yh + bb_[k];
              const f32x2 gs = gv * a.bns;
              const f32x2 g = {t.x > 0.f ? gv.x : gs.x, t.y > 0.f ? gv.y : gs.y};
              sacc[k] += g;
              // sum of g * yhat: one FMA per term for channels 0-5 of the chunk, a rounded product
              // and an add for channels 6, 7 -- the forms the general path's code compiles to,
              // written out so that the records stay the same bit for bit
              if (k < 3) qacc[k] = f32x2{__builtin_fmaf(g.x, yh.x, qacc[k].x), __builtin_fmaf(g.y, yh.y, qacc[k].y)};
              else qacc[k] = mul_then_add(g, yh, qacc[k]);
            }
          } else {
            if constexpr (ADD) {
              float f[8];
#pragma unroll
              for (int j = 0; j < 8; ++j) f[j] = v.get(j) + r.get(j);
              v.set8(f);
            }
            if constexpr (REC == 1) {
              // (sums of the stored, bf16-rounded values)
#pragma unroll
              for (int k = 0; k < 4; ++k) {
                const f32x2 o = {v.get(2 * k), v.get(2 * k + 1)};
                sacc[k] += o;
                qacc[k] += o * o;
              }
            }
          }
          v.store(reinterpret_cast<bf16*>(haddr(a.y, it)));
          // (the chunks stay in order, each chunk's terms summed before the next: left free, the
          // NRES bodies of this one block are interleaved and the terms kept for a late sum, until
          // the 256-co tile and the persistent kernels spill)
          if constexpr (REC != 0) {
#pragma unroll
            for (int k = 0; k < 4; ++k) asm volatile("" : "+v"(sacc[k]), "+v"(qacc[k]));
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      };
      using No = std::false_type;
      using Yes = std::true_type;
      if (!a.spm) {
        // the plain store pass (kept free of the record code: +2-3 us per res conv)
        if (a.res) pass(Yes{}, std::integral_constant<int, 0>{});
        else pass(No{}, std::integral_constant<int, 0>{});
        return;
      }
      if (a.spm == 2) pass(No{}, std::integral_constant<int, 2>{});       // (res = the BN input, not added)
      else if (a.res) pass(Yes{}, std::integral_constant<int, 1>{});
      else pass(No{}, std::integral_constant<int, 1>{});
      float ssum[8], qsum[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        ssum[j] = sacc[j >> 1][j & 1];
        qsum[j] = qacc[j >> 1][j & 1];
      }
#pragma unroll
      for (int o = CPR; o < 64; o <<= 1)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          ssum[j] += __shfl_xor(ssum[j], o, 64);
          qsum[j] += __shfl_xor(qsum[j], o, 64);
        }
      if (lane < CPR) {
        const long rec = (long)tm * (NT / 64) + (tid >> 6);
        float* r0 = a.sprec + (rec * 2) * a.Cout + c;
        float* r1 = a.sprec + (rec * 2 + 1) * a.Cout + c;
        *reinterpret_cast<float4*>(r0) = make_float4(ssum[0], ssum[1], ssum[2], ssum[3]);
        *reinterpret_cast<float4*>(r0 + 4) = make_float4(ssum[4], ssum[5], ssum[6], ssum[7]);
        *reinterpret_cast<float4*>(r1) = make_float4(qsum[0], qsum[1], qsum[2], qsum[3]);
        *reinterpret_cast<float4*>(r1 + 4) = make_float4(qsum[4], qsum[5], qsum[6], qsum[7]);
      }
      return;
    }
    if (!a.spm) {
      // the plain store pass (kept free of the record code below: +2-3 us per res conv)
#pragma unroll
      for (int it = 0; it < NRES; ++it) {
        const int idx = tid + it * NT;
        if (idx >= BM * CPR) break;
        const int pl = idx / CPR, ch = idx - (idx / CPR) * CPR;
        const int tp = a.lgtw ? p0 + (pl >> a.lgtw) * a.W + (pl & ((1 << a.lgtw) - 1)) : p0 + pl;
        const int co = co0 + ch * 8;
        if (tp >= a.P || co >= a.Cout) continue;
        const int pix = out_pix<GSUB>(a, tp);
        Chunk8<bf16> v;
        v.raw = chunk(it, pl, ch);
        T* yp = reinterpret_cast<T*>(a.y) + (long)pix * a.ldy + co;
        if (a.res) {
          Chunk8<bf16> r;
          r.raw = rpre[it];
          float f[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) f[j] = v.get(j) + r.get(j);
          v.set8(f);
        }
        v.store(reinterpret_cast<bf16*>(yp));
      }
      return;
    }
    // store-pass records: NT % CPR == 0 keeps every thread on one 8-channel chunk for all its
    // iterations (the host enables spm only for such tiles, with P % BM == 0)
    const int sch = tid % CPR;
    float sacc[8], qacc[8], bm_[8], bi_[8], bg_[8], bb_[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) sacc[j] = qacc[j] = 0.f;
    if (a.spm == 2) {
      const int c = co0 + sch * 8;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const bool ok = c + j < a.Cout;
        bm_[j] = ok ? a.bnm[c + j] : 0.f;
        bi_[j] = ok ? a.bni[c + j] : 0.f;
        bg_[j] = ok ? a.bng[c + j] : 0.f;
        bb_[j] = ok ? a.bnb[c + j] : 0.f;
      }
    }
#pragma unroll
    for (int it = 0; it < NRES; ++it) {
      const int idx = tid + it * NT;
      if (idx >= BM * CPR) break;
      const int pl = idx / CPR, ch = idx - (idx / CPR) * CPR;
      const int tp = a.lgtw ? p0 + (pl >> a.lgtw) * a.W + (pl & ((1 << a.lgtw) - 1)) : p0 + pl;
      const int co = co0 + ch * 8;
      if (tp >= a.P || co >= a.Cout) continue;
      const int pix = out_pix<GSUB>(a, tp);
      Chunk8<bf16> v;
      v.raw = chunk(it, pl, ch);
      T* yp = reinterpret_cast<T*>(a.y) + (long)pix * a.ldy + co;
      Chunk8<bf16> r;
      r.raw = rpre[it];
      if (a.spm == 2) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float yh = (r.get(j) - bm_[j]) * bi_[j];
          const float gv = v.get(j);
          const float g = bg_[j] * yh + bb_[j] > 0.f ? gv : gv * a.bns;
          sacc[j] += g;
          qacc[j] += g * yh;
        }
      } else {
        if (a.res) {
          float f[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) f[j] = v.get(j) + r.get(j);
          v.set8(f);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float o = v.get(j);
          sacc[j] += o;
          qacc[j] += o * o;
        }
      }
      v.store(reinterpret_cast<bf16*>(yp));
    }
    {
      static_assert(CPR <= 64 && 64 % CPR == 0, "store-pass records: chunks per row must divide a wave");
#pragma unroll
      for (int o = CPR; o < 64; o <<= 1)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          sacc[j] += __shfl_xor(sacc[j], o, 64);
          qacc[j] += __shfl_xor(qacc[j], o, 64);
        }
      const int c = co0 + sch * 8;
      if (lane < CPR && c < a.Cout) {
        const long rec = (long)tm * (NT / 64) + (tid >> 6);
        float* r0 = a.sprec + (rec * 2) * a.Cout + c;
        float* r1 = a.sprec + (rec * 2 + 1) * a.Cout + c;
        *reinterpret_cast<float4*>(r0) = make_float4(sacc[0], sacc[1], sacc[2], sacc[3]);
        *reinterpret_cast<float4*>(r0 + 4) = make_float4(sacc[4], sacc[5], sacc[6], sacc[7]);
        *reinterpret_cast<float4*>(r1) = make_float4(qacc[0], qacc[1], qacc[2], qacc[3]);
        *reinterpret_cast<float4*>(r1 + 4) = make_float4(qacc[4], qacc[5], qacc[6], qacc[7]);
      }
    }
    return;
  }
#pragma unroll
  for (int n = 0; n < RN; ++n) {
    const int cb = co0 + wn * RN * 16 + n * 16 + lh * 4;
#pragma unroll
    for (int m = 0; m < RM; ++m) {
      if (!pv[m]) continue;
      float f[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        f[i] = acc[n][m][i];
        if (a.sigmoid) f[i] = 1.f / (1.f + expf(-f[i]));
      }
      if (a.nchw) {
        float* yp = reinterpret_cast<float*>(a.y);
        const int img = pix_of[m] / HW, hw = pix_of[m] - img * HW;
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (cb + i < a.Cout) yp[((long)img * a.Cout + cb + i) * HW + hw] = f[i];
      } else {
        T* yp = reinterpret_cast<T*>(a.y) + (long)pix_of[m] * a.ldy + cb;
        if (cb + 3 < a.Cout) {
          store4<T>(yp, f);
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (cb + i < a.Cout) yp[i] = Elt<T>::from_f(f[i]);
        }
      }
    }
  }
}

template <int N>
__device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
// wave-uniform count -> the matching immediate (counts above 15 wait for 15: stricter, safe)
__device__ __forceinline__ void wait_vm_dyn(int n) {
  switch (n) {
    case 0: wait_vm<0>(); break;
    case 1: wait_vm<1>(); break;
    case 2: wait_vm<2>(); break;
    case 3: wait_vm<3>(); break;
    case 4: wait_vm<4>(); break;
    case 5: wait_vm<5>(); break;
    case 6: wait_vm<6>(); break;
    case 7: wait_vm<7>(); break;
    case 8: wait_vm<8>(); break;
    case 9: wait_vm<9>(); break;
    case 10: wait_vm<10>(); break;
    case 11: wait_vm<11>(); break;
    case 12: wait_vm<12>(); break;
    case 13: wait_vm<13>(); break;
    case 14: wait_vm<14>(); break;
    default: wait_vm<15>(); break;
  }
}

constexpr int BK2 = 64;
__device__ __forceinline__ int swz8(int row) { return (row >> 1) & 7; }
// 16-B chunk swizzle of the 64-B halo pixels of conv3_halo_fwd2 (conv_halo3.hip) and the fp8 halo
// kernels (conv_fp8.hip): a fragment read of 16 consecutive halo pixels from any start is conflict free
__device__ __forceinline__ int h3swz(int hp) { return ((hp >> 2) & 1) << 1; }

typedef __attribute__((address_space(3))) void* lds_ptr_t;

// 16 B per lane, buffer -> LDS (wave-uniform LDS byte address in M0, lane-linear
// destination), byte offset voffset + soffset (an out-of-range voffset of 0x80000000 stays
// out of range for any soffset < 2^31, so the hardware returns zeros).
// Issued as inline asm on purpose: hipcc cannot tell that the ds_reads of the buffer being
// computed do not alias the stage in flight and would put an s_waitcnt vmcnt(0) in front
// of them, serialising the ring.  Ordering is therefore explicit: counted vmcnt + barrier.
// The asm has NO outputs (M0 is declared clobbered): hipcc models an inline asm containing a
// VMEM op as writing its outputs asynchronously and waits vmcnt(0) before such a register is
// reused -- with an output, every DMA of a loop waited for the previous one.
// lgkmcnt(0) as the s_waitcnt builtin, not inline asm: the compiler's wait-count pass sees it
// and knows every LDS read issued before it has landed.  After an inline-asm wait the pass
// still counts those reads as outstanding, and with more than 15 reads in flight (the 4-bit
// lgkm counter) it waits for the NEWEST reads before the first use of an old fragment: in
// the pair-of-taps loops every step's second MFMA cluster waited for the next tap's 12
// fragment reads (lgkmcnt(7) .. (0) in front of its first 8 MFMAs).
__device__ __forceinline__ void wait_lgkm0() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_waitcnt(0xC07F);       // vmcnt(63) expcnt(7) lgkmcnt(0)
}

__device__ __forceinline__ void dma16s(__amdgpu_buffer_rsrc_t r, unsigned lds, unsigned voff, unsigned soff) {
  // lds / soff are wave-uniform at every call site (the "s" operands); readfirstlane states it
  // for values the compiler merges across uniform branches into a VGPR phi (a no-op on an SGPR)
  lds = __builtin_amdgcn_readfirstlane(lds);
  soff = __builtin_amdgcn_readfirstlane(soff);
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %1, %3 offen lds"
               :
               : "v"(voff), "s"(r), "s"(lds), "s"(soff)
               : "memory", "m0");
}
__device__ __forceinline__ void dma16(__amdgpu_buffer_rsrc_t r, const void* lds, unsigned voff) {
  dma16s(r, __builtin_amdgcn_readfirstlane((unsigned)(size_t)(lds_ptr_t)lds), voff, 0u);
}

// f(integral_constant<S>) for the run-time, wave-uniform s in [0, N): a scalar branch to
// one of N instantiations, so register arrays are only ever indexed by constants
template <int S, int N, typename F>
__device__ __forceinline__ void with_const(int s, F&& f) {
  if constexpr (S + 1 == N) {
    f(std::integral_constant<int, S>{});
  } else {
    if (s == S) f(std::integral_constant<int, S>{});
    else with_const<S + 1, N>(s, f);
  }
}

// BKS = k per stage: 64 (128-B rows, 8 chunks) or 32 (64-B rows, 4 chunks; half the LDS, so
// the 4-wave tiles run 4 blocks per CU and hide each other's DMA latency and epilogue).
template <int BKS>
__device__ __forceinline__ int swzk(int row) {
  if constexpr (BKS == 64) return swz8(row);
  else return rswz<bf16>(row);
}

}  // namespace
