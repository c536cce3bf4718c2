// The bf16 / fp32 weight-gradient kernels of the 2-D convolution, the slab reductions and their
// launchers (argument structs: conv_plan.h).  Planners and entries: conv.hip.
#include "conv_plan.h"

namespace {

// ----------------------------------------------------------------------------------------
// backward-weight:  D[k][co] = sum_p im2col(x)[p][k] * dy[p][co], split over pixels
// MFMA A operand = im2col^T (rows = k), B operand = dy (cols = co); both are k-slot =
// pixel, i.e. COLUMN reads of the [pixel][channel] LDS images -> ds_read_b64_tr_b16.
// ----------------------------------------------------------------------------------------
// 8-B granule swizzle for the transposed-read images (cols >= 64): conflict-free
// ds_read_b64_tr_b16 over rows {8g+q} (wgrad).
__device__ __forceinline__ int gswz(int row) { return (((row >> 1) & 1) | (((row >> 3) & 1) << 1)) << 2; }

template <int COLS>
__device__ __forceinline__ int tr_off(int row, int col) {  // byte offset of (row, col) bf16
  if constexpr (COLS >= 64) return row * COLS * 2 + (((col >> 2) ^ gswz(row)) << 3) + (col & 3) * 2;
  else return row * COLS * 2 + col * 2;
}

template <typename T, int COLS>
__device__ __forceinline__ void colfrag(const char* base, int cbase, int lane, Frag<T>& f) {
  const int g = lane >> 4, li = lane & 15;
  if constexpr (sizeof(T) == 2) {
    const int q = li >> 2, pp = li & 3;
    const int c = cbase + 4 * pp;
    FV_LDS char* lb = (FV_LDS char*)(base);   // generic -> LDS address-space cast
    s16x4 t0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((FV_LDS s16x4*)(lb + tr_off<COLS>(8 * g + q, c)));
    s16x4 t1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((FV_LDS s16x4*)(lb + tr_off<COLS>(8 * g + 4 + q, c)));
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    s16x8 v = {t0[0], t0[1], t0[2], t0[3], t1[0], t1[1], t1[2], t1[3]};
    f.v = __builtin_bit_cast(bf16x8, v);
  } else {
    const float* fb = reinterpret_cast<const float*>(base);
#pragma unroll
    for (int j = 0; j < 8; ++j) f.v[j] = fb[(8 * g + j) * COLS + cbase + li];
  }
}

// S2 = 1: the stride-2 3x3 conv (pixels = the H x W output, x read at 2 * out + tap - 1)
template <typename T, int KS, int WK, int WC, int RK, int RC, bool PRO, bool UPS, int S2 = 0>
__global__ void __launch_bounds__(64 * WK * WC)
conv_wgrad_kernel(WgArgs a) {
  constexpr int NT = 64 * WK * WC;
  constexpr int BKT = WK * RK * 16;  // k columns per block
  constexpr int BC = WC * RC * 16;   // output channels per block
  constexpr int PAD = KS / 2;
  constexpr int ES = sizeof(T);
  constexpr int PX = 32;             // pixels per step
  constexpr int ABYTES = PX * BKT * ES, DBYTES = PX * BC * ES;
  constexpr int KCH = BKT / 8, CCH = BC / 8;     // 8-element chunks per row
  constexpr int CA = (PX * KCH + NT - 1) / NT;
  constexpr int CD = (PX * CCH + NT - 1) / NT;
  static_assert(NT % KCH == 0 && NT % CCH == 0, "chunk map");
  __shared__ __attribute__((aligned(16))) char smem[2 * (ABYTES + DBYTES)];

  const T* __restrict__ x = reinterpret_cast<const T*>(a.x);
  const T* __restrict__ dy = reinterpret_cast<const T*>(a.dy);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wk = wave % WK, wc = wave / WK;
  const int per = a.ntk * a.ntc;
  const int split = blockIdx.x / per;
  const int rem = blockIdx.x - split * per;
  const int tc = rem % a.ntc, tk = rem / a.ntc;
  const int k0 = tk * BKT, c0 = tc * BC;
  const int s_begin = split * a.steps_per_split;
  const int s_end = min(a.nsteps, s_begin + a.steps_per_split);
  const int HW = a.H * a.W;

  // fixed per-thread k chunk (gather) and co chunk (dy)
  const int kq = tid % KCH;
  const int kk = k0 + kq * 8;
  const bool kin = kk < a.K;
  const int tap = kk >> a.lgCin, ci = kk & (a.Cin - 1);
  const int rr = tap / KS, ss = tap - (tap / KS) * KS;
  const int cq = tid % CCH;
  const int cc = c0 + cq * 8;
  const bool cin_ok = cc < a.ldd;

  Chunk8<T> ra[CA], rd[CD];
  unsigned okm = 0;

  auto gload = [&](int st) {
    const int pbase = st * PX;
    okm = 0;
#pragma unroll
    for (int i = 0; i < CA; ++i) {
      const int q = tid + i * NT;
      const int prow = q / KCH;
      const int pix = pbase + prow;
      bool ok = kin && (q < PX * KCH) && pix < a.P;
      int n = pix / HW, r2 = pix - n * HW;
      int h = r2 / a.W, w = r2 - h * a.W;
      int hh = (S2 ? 2 * h : h) + rr - PAD, ww = (S2 ? 2 * w : w) + ss - PAD;
      int hs, ws;
      if constexpr (UPS) {
        ok = ok && hh >= 0 && hh < a.H && ww >= 0 && ww < a.W;
        hs = hh >> 1;
        ws = ww >> 1;
      } else {
        ok = ok && hh >= 0 && hh < a.Hin && ww >= 0 && ww < a.Win;
        hs = hh;
        ws = ww;
      }
      if (ok) {
        ra[i].load(x + ((long)(n * a.Hin * a.Win + hs * a.Win + ws) << a.lgCin) + ci);
        okm |= 1u << i;
      } else {
        ra[i].zero();
      }
    }
#pragma unroll
    for (int i = 0; i < CD; ++i) {
      const int q = tid + i * NT;
      const int pix = pbase + q / CCH;
      if (cin_ok && q < PX * CCH && pix < a.P) rd[i].load(dy + (long)pix * a.ldd + cc);
      else rd[i].zero();
    }
  };

  auto chunk_off = [&](int row, int col, int cols) -> int {  // byte offset of an 8-elt chunk
    if constexpr (ES == 2) {
      if (cols >= 64) return row * cols * 2 + (((col >> 2) ^ gswz(row)) << 3);
      return row * cols * 2 + col * 2;
    } else {
      return (row * cols + col) * 4;
    }
  };

  auto lstore = [&](int buf) {
    char* As = smem + buf * (ABYTES + DBYTES);
    char* Ds = As + ABYTES;
#pragma unroll
    for (int i = 0; i < CA; ++i) {
      const int q = tid + i * NT;
      if (q < PX * KCH) {
        Chunk8<T> c = ra[i];
        if constexpr (PRO) {
          if (okm & (1u << i)) {
            float f[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) f[j] = fv_act(c.get(j) * a.psc[ci + j] + a.psh[ci + j], a.slope);
            c.set8(f);
          }
        }
        c.store(reinterpret_cast<T*>(As + chunk_off(q / KCH, kq * 8, BKT)));
      }
    }
#pragma unroll
    for (int i = 0; i < CD; ++i) {
      const int q = tid + i * NT;
      if (q < PX * CCH) rd[i].store(reinterpret_cast<T*>(Ds + chunk_off(q / CCH, cq * 8, BC)));
    }
  };

  f32x4 acc[RK][RC];
#pragma unroll
  for (int i = 0; i < RK; ++i)
#pragma unroll
    for (int j = 0; j < RC; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // bias-gradient partial (only the k-tile-0 blocks): thread -> column tid % BC
  const bool do_bias = (tk == 0) && a.bslab;
  constexpr int BROWS = NT / BC > 0 ? NT / BC : 1;
  float bsum = 0.f;

  auto compute = [&](int buf) {
    const char* As = smem + buf * (ABYTES + DBYTES);
    const char* Ds = As + ABYTES;
    Frag<T> af[RK], bfr[RC];
#pragma unroll
    for (int i = 0; i < RK; ++i) colfrag<T, BKT>(As, wk * RK * 16 + i * 16, lane, af[i]);
#pragma unroll
    for (int j = 0; j < RC; ++j) colfrag<T, BC>(Ds, wc * RC * 16 + j * 16, lane, bfr[j]);
#pragma unroll
    for (int i = 0; i < RK; ++i)
#pragma unroll
      for (int j = 0; j < RC; ++j) acc[i][j] = mma(af[i], bfr[j], acc[i][j]);
    if (do_bias && tid < BROWS * BC) {
      const int col = tid % BC, part = tid / BC;
      for (int r = part; r < PX; r += BROWS) {
        if constexpr (ES == 2) bsum += (float)*reinterpret_cast<const bf16*>(Ds + tr_off<BC>(r, col));
        else bsum += reinterpret_cast<const float*>(Ds)[r * BC + col];
      }
    }
  };

  if (s_begin < s_end) {
    gload(s_begin);
    lstore(0);
    __syncthreads();
    for (int st = s_begin; st < s_end; ++st) {
      const int cur = (st - s_begin) & 1;
      if (st + 1 < s_end) gload(st + 1);
      compute(cur);
      if (st + 1 < s_end) lstore(cur ^ 1);
      __syncthreads();
    }
  }

  // D[k][co]: lane holds k = kb + 4*(lane>>4) + i for co = cb + (lane & 15)
  const int lr = lane & 15, lh = lane >> 4;
  float* slab = a.slab + (long)split * a.CW * a.KW;
#pragma unroll
  for (int i = 0; i < RK; ++i) {
    const int kb = k0 + wk * RK * 16 + i * 16 + lh * 4;
#pragma unroll
    for (int j = 0; j < RC; ++j) {
      const int co = c0 + wc * RC * 16 + j * 16 + lr;
      *reinterpret_cast<float4*>(slab + (long)co * a.KW + kb) =
          make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]);
    }
  }
  if (do_bias) {
    float* red = reinterpret_cast<float*>(smem);
    if (tid < BROWS * BC) red[tid] = bsum;
    __syncthreads();
    if (tid < BC) {
      float t = 0.f;
      for (int p = 0; p < BROWS; ++p) t += red[p * BC + tid];
      a.bslab[(long)split * a.CW + c0 + tid] = t;
    }
  }
}

// ----------------------------------------------------------------------------------------
// backward-weight v2 (bf16): D[k][co] = sum_p im2col(x)[p][k] * dy[p][co] as a pixel-K GEMM.
// 8 waves, block tile BKT (k) x BC (co), PX pixels per stage, NS-stage LDS ring filled by
// buffer_load ... lds (the DMA destination is lane-linear, so the 32-B-block XOR swizzle
// that makes the transposed fragment reads conflict-free is applied to the SOURCE
// address), counted vmcnt + raw s_barrier so NS-1 stages stay in flight.  Fragments are
// read with ds_read_b64_tr_b16 (pixels are the MFMA K).  Zero padding (image border,
// k >= K, co >= ldd, pixel >= P) comes from the buffer range check (offset 0x80000000).
// The bias gradient sum_p dy[p][co] rides along as one extra MFMA per co tile with an
// all-ones A operand (k-tile-0 blocks, k-wave 0 only).  Output: per-split fp32 slabs.
// ----------------------------------------------------------------------------------------
// 32-B-block XOR of a [row][NCOL] bf16 image: the 8 rows {0-3, 8-11} (and {4-7, 12-15}) one
// ds_read_b64_tr_b16 lane group touches land on 8 distinct 32-B bank slots.
template <int NCOL>
__device__ __forceinline__ int tswz(int row) {
  if constexpr (NCOL >= 128) return (row & 3) | (((row >> 3) & 1) << 2);
  else if constexpr (NCOL == 64) return ((row >> 1) & 1) | (((row >> 3) & 1) << 1);
  else if constexpr (NCOL == 32) return (row >> 3) & 1;   // rows r and r + 8 in different halves
  else return 0;
}
template <int NCOL>
__device__ __forceinline__ int timg_off(int row, int col) {  // col % 4 == 0
  return row * NCOL * 2 + ((((col >> 4) ^ tswz<NCOL>(row)) << 5) | ((col & 15) << 1));
}
// 16 columns x 32 rows (rows r0..r0+31) -> MFMA K-fragment of column (cbase + lane & 15)
template <int NCOL>
__device__ __forceinline__ bf16x8 tfrag(const char* base, int r0, int cbase, int lane) {
  const int g = lane >> 4, li = lane & 15;
  // NCOL < 16 (8 staged channels): lanes of columns >= NCOL re-read valid columns; the
  // caller ignores those outputs (every lane must take part in a transposed read)
  const int c = (cbase + 4 * (li & 3)) & (NCOL >= 16 ? ~0 : NCOL - 1);
  FV_LDS char* lb = (FV_LDS char*)(base);
  const s16x4 t0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((FV_LDS s16x4*)(lb + timg_off<NCOL>(r0 + 8 * g + (li >> 2), c)));
  const s16x4 t1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((FV_LDS s16x4*)(lb + timg_off<NCOL>(r0 + 8 * g + 4 + (li >> 2), c)));
  typedef short s16x8 __attribute__((ext_vector_type(8)));
  const s16x8 v = {t0[0], t0[1], t0[2], t0[3], t1[0], t1[1], t1[2], t1[3]};
  return __builtin_bit_cast(bf16x8, v);
}

// ring wait: retire the oldest stage while `ahead` (0 .. NS-2, run-time) younger ones stay in flight
template <int NS, int PW, int A = NS - 2>  // vmcnt immediate <= 63: (NS - 2) * PW must fit
__device__ __forceinline__ void wait_ahead(int ahead) {
  if constexpr (A <= 0) {
    wait_vm<0>();
  } else {
    if (ahead >= A) wait_vm<A * PW>();
    else wait_ahead<NS, PW, A - 1>(ahead);
  }
}

template <int KS, int BKT, int BC, int WK, int WC, int PX, int NS, bool UPS, bool SUB = false>
__global__ void __launch_bounds__(512, 2)
conv_wgrad_v2(Wg2Args a) {
  static_assert(!SUB || (KS == 2 && !UPS), "sub-pixel wgrad: 2x2 taps, no upsample");
  static_assert(WK * WC == 8, "8 waves");
  constexpr int RK = BKT / (16 * WK), RC = BC / (16 * WC);
  static_assert(RK * 16 * WK == BKT && RC * 16 * WC == BC, "wave tiling");
  constexpr int PAD = KS / 2;
  constexpr int SA = PX * BKT * 2, SB = PX * BC * 2, STAGE = SA + SB;
  constexpr int QA = SA / 1024, QB = SB / 1024;            // 1-KB DMA pieces per stage
  static_assert(QA * 1024 == SA && QB * 1024 == SB, "pieces");
  constexpr int JA = (QA + 7) / 8, JB = (QB + 7) / 8;      // pieces per wave
  constexpr int PW = JA + JB;                              // upper bound of DMAs per wave per stage
  constexpr int CPA = BKT / 8, CPB = BC / 8;               // 16-B chunks per row
  __shared__ __attribute__((aligned(1024))) char smem[NS * STAGE];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wk = wave % WK, wc = wave / WK;
  // XCD-aware order: the blocks of one pixel split (all k/co tiles: same dy rows, overlapping
  // x rows) share an XCD's L2.  Bijective remap; speed only.
  const int nblk = gridDim.x, bid = blockIdx.x;
  const int q8 = nblk / 8, r8 = nblk % 8, xcd = bid % 8;
  const int lid0 = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + bid / 8;
  const int phase = SUB ? (lid0 & 3) : 0;      // the 4 phases of a split are neighbours
  const int lid = SUB ? (lid0 >> 2) : lid0;
  const int pa = phase >> 1, pb = phase & 1;
  const int ntile = a.ntk * a.ntc;
  const int split = lid / ntile, tile = lid - split * ntile;
  const int tc = tile % a.ntc, tk = tile / a.ntc;
  const int k0 = tk * BKT, c0 = tc * BC;
  const int s_begin = split * a.sps;
  const int nst = min(a.nsteps, s_begin + a.sps) - s_begin;

  const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.x), 0, (int)a.xbytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t dr = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.dy), 0, (int)a.dybytes, 0x00020000);

  // per-piece constants: row in the stage image and the (tap, ci) of this lane's chunk
  int arow[JA], adh[JA], adw[JA], aci[JA];
  bool akin[JA];
#pragma unroll
  for (int j = 0; j < JA; ++j) {
    const int q = wave + j * 8;
    const int L = q * 64 + lane;
    const int row = L / CPA, dch = L % CPA;
    const int sc = (((dch >> 1) ^ tswz<BKT>(row)) << 1) | (dch & 1);
    const int k = k0 + sc * 8;
    const int tap = k >> a.lgCin;
    const int r = tap / KS, s = tap - (tap / KS) * KS;
    arow[j] = row;
    adh[j] = SUB ? r + pa - 1 : r - PAD;
    adw[j] = SUB ? s + pb - 1 : s - PAD;
    aci[j] = k & ((1 << a.lgCin) - 1);
    akin[j] = (QA % 8 == 0 || q < QA) && k < a.K;
  }
  int brow[JB], bco[JB];
  bool bok[JB];
#pragma unroll
  for (int j = 0; j < JB; ++j) {
    const int q = wave + j * 8;
    const int L = q * 64 + lane;
    const int row = L / CPB, dch = L % CPB;
    const int sc = CPB >= 4 ? ((((dch >> 1) ^ tswz<BC>(row)) << 1) | (dch & 1)) : dch;
    brow[j] = row;
    bco[j] = c0 + sc * 8;
    bok[j] = (QB % 8 == 0 || q < QB) && bco[j] < a.ldd;
  }

  // row-aligned stages (W % PX == 0, so P % PX == 0 too): a stage is one image-row segment
  // (n, h, w0 wave-uniform).  The lane's part of its im2col source offset is precomputed
  // relative to (h, w0) -- per h parity when upsampling -- so a piece costs an add, two
  // range compares and a select; the dy pieces are a fixed per-lane offset + soffset.
  int cwA[JA], cA0[JA], cA1[JA];
#pragma unroll
  for (int j = 0; j < JA; ++j) {
    const int cw = akin[j] ? arow[j] + adw[j] : 0x40000000;   // column relative to w0
    cwA[j] = cw;
    if (UPS) {
      cA0[j] = (((((adh[j] >> 1) * a.Win) + (cw >> 1)) << a.lgCin) + aci[j]) * 2;
      cA1[j] = (((((1 + adh[j]) >> 1) * a.Win + (cw >> 1)) << a.lgCin) + aci[j]) * 2;
    } else {
      cA0[j] = cA1[j] = (((adh[j] * a.Win + cw) << a.lgCin) + aci[j]) * 2;
    }
  }
  unsigned cB[JB];
#pragma unroll
  for (int j = 0; j < JB; ++j) cB[j] = bok[j] ? (unsigned)(brow[j] * (SUB ? 2 : 1) * a.ldd + bco[j]) * 2u : 0x80000000u;
  const unsigned sbase = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(lds_ptr_t)smem);

  // row-aligned stage: wave-uniform state once per stage, then one DMA piece at a time, so
  // the pieces can be spread between MFMAs (a piece costs ~60 cycles among MFMAs, 100-185
  // back to back; issued as a block, both waves of a SIMD stall on them together)
  struct RowSt {
    unsigned As, Bs, dpo;
    int S, h, w0;
    bool sok, odd;
  };
  auto rowal_state = [&](int st, int buf) {
    RowSt r;
    const int pbase = (s_begin + st) * PX;
    r.As = sbase + buf * STAGE;
    r.Bs = r.As + SA;
    const int hrow = (int)fdiv((uint32_t)pbase, a.fw);
    r.w0 = pbase - hrow * a.W;
    const int n = (int)fdiv((uint32_t)hrow, a.fh);
    r.h = hrow - n * a.H;
    r.sok = pbase < a.P;
    r.S = UPS ? ((((n * a.Hin + (r.h >> 1)) * a.Win + (r.w0 >> 1)) << a.lgCin) * 2)
              : ((((n * a.Hin + r.h) * a.Win + r.w0) << a.lgCin) * 2);
    r.odd = UPS && (r.h & 1);
    // dy pixel of the stage's first pixel: itself, or (n, 2h+pa, 2*w0+pb) for a phase
    const unsigned dp = SUB ? (unsigned)((n * a.Ho + 2 * r.h + pa) * a.Wo + 2 * r.w0 + pb) : (unsigned)pbase;
    r.dpo = dp * (unsigned)a.ldd * 2u;
    return r;
  };
  // piece q in [0, JA + JB): x pieces first, then dy (compile-time q after unrolling)
  auto rowal_piece = [&](const RowSt& r, int q) {
    if (q < JA) {
      const int j = q, qq = wave + j * 8;
      if (QA % 8 == 0 || qq < QA) {
        const bool ok = r.sok && (unsigned)(r.h + adh[j]) < (unsigned)a.H && (unsigned)(r.w0 + cwA[j]) < (unsigned)a.W;
        const int c = r.odd ? cA1[j] : cA0[j];
        dma16s(xr, r.As + qq * 1024, ok ? (unsigned)(r.S + c) : 0x80000000u, 0u);
      }
    } else {
      const int j = q - JA, qq = wave + j * 8;
      if (QB % 8 == 0 || qq < QB) {
        if (r.sok) dma16s(dr, r.Bs + qq * 1024, cB[j], r.dpo);
        else dma16s(dr, r.Bs + qq * 1024, 0x80000000u, 0u);
      }
    }
  };
  auto issue_rowal = [&](int st, int buf) {
    const RowSt r = rowal_state(st, buf);
#pragma unroll
    for (int q = 0; q < JA + JB; ++q) rowal_piece(r, q);
  };

  auto issue = [&](int st, int buf) {
    if (SUB || a.rowal) {        // SUB: the host only launches row-aligned stages
      issue_rowal(st, buf);
      return;
    }
    const int pbase = (s_begin + st) * PX;
    char* As = smem + buf * STAGE;
    char* Bs = As + SA;
#pragma unroll
    for (int j = 0; j < JA; ++j) {
      const int q = wave + j * 8;
      if (QA % 8 == 0 || q < QA) {
        const int p = pbase + arow[j];
        const int n = (int)fdiv((uint32_t)p, a.fhw);
        const int rem = p - n * a.H * a.W;
        const int h = (int)fdiv((uint32_t)rem, a.fw);
        const int w = rem - h * a.W;
        const int hh = h + adh[j], ww = w + adw[j];
        bool ok = akin[j] && p < a.P && hh >= 0 && hh < a.H && ww >= 0 && ww < a.W;
        const int hs = UPS ? (hh >> 1) : hh, ws = UPS ? (ww >> 1) : ww;
        const unsigned off = ok ? ((unsigned)(((n * a.Hin + hs) * a.Win + ws) << a.lgCin) + (unsigned)aci[j]) * 2u
                                : 0x80000000u;
        dma16(xr, As + q * 1024, off);
      }
    }
#pragma unroll
    for (int j = 0; j < JB; ++j) {
      const int q = wave + j * 8;
      if (QB % 8 == 0 || q < QB) {
        const int p = pbase + brow[j];
        const bool ok = bok[j] && p < a.P;
        const unsigned off = ok ? ((unsigned)p * (unsigned)a.ldd + (unsigned)bco[j]) * 2u : 0x80000000u;
        dma16(dr, Bs + q * 1024, off);
      }
    }
  };
  // a counted vmcnt needs every wave to issue exactly PW DMAs per stage
  static_assert((QA % 8 == 0 && QB % 8 == 0) || NS == 2, "uneven DMA split needs NS == 2 (vmcnt(0))");

  f32x4 acc[RK][RC];
#pragma unroll
  for (int i = 0; i < RK; ++i)
#pragma unroll
    for (int j = 0; j < RC; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const bool do_bias = a.bslab && tk == 0 && wk == 0;
  f32x4 accb[RC];
#pragma unroll
  for (int j = 0; j < RC; ++j) accb[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  bf16x8 ones;
#pragma unroll
  for (int i = 0; i < 8; ++i) ones[i] = (bf16)1.0f;

  // hook(i): called after MFMA row i of the first 32-pixel slice (the DMA pieces of the
  // next stage go there)
  auto compute_h = [&](int buf, auto&& hook) {
    const char* As = smem + buf * STAGE;
    const char* Bs = As + SA;
#pragma unroll
    for (int kk = 0; kk < PX / 32; ++kk) {
      bf16x8 af[RK], bfr[RC];
#pragma unroll
      for (int j = 0; j < RC; ++j) bfr[j] = tfrag<BC>(Bs, kk * 32, wc * RC * 16 + j * 16, lane);
#pragma unroll
      for (int i = 0; i < RK; ++i) af[i] = tfrag<BKT>(As, kk * 32, wk * RK * 16 + i * 16, lane);
#pragma unroll
      for (int i = 0; i < RK; ++i) {
#pragma unroll
        for (int j = 0; j < RC; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
        if (kk == 0) hook(i);
      }
      if (do_bias) {
#pragma unroll
        for (int j = 0; j < RC; ++j) accb[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, bfr[j], accb[j], 0, 0, 0);
      }
    }
  };

  // ring: NS-1 stages in flight; stage `it` is waited for with a counted vmcnt, then one
  // raw barrier publishes it (and retires every wave's reads of the buffer re-filled next).
#pragma unroll
  for (int i = 0; i < NS - 1; ++i)
    if (i < nst) issue(i, i);
  if ((SUB || a.rowal) && a.il) {
    // the next stage's pieces spread over the first slice's MFMA rows (all issued within the
    // iteration, in piece order: the counted waits are unchanged)
    for (int it = 0; it < nst; ++it) {
      const int ahead = min(NS - 2, nst - 1 - it);
      wait_ahead<NS, PW>(ahead);
      wait_lgkm0();
      __builtin_amdgcn_s_barrier();
      const bool more = it + NS - 1 < nst;
      const RowSt r = rowal_state(it + NS - 1, (it + NS - 1) % NS);
      compute_h(it % NS, [&](int i) {
#pragma unroll
        for (int q = i * (JA + JB) / RK; q < (i + 1) * (JA + JB) / RK; ++q)
          if (more) rowal_piece(r, q);
      });
    }
  } else {
    for (int it = 0; it < nst; ++it) {
      const int ahead = min(NS - 2, nst - 1 - it);   // younger stages allowed in flight
      wait_ahead<NS, PW>(ahead);
      wait_lgkm0();
      __builtin_amdgcn_s_barrier();
      if (it + NS - 1 < nst) issue(it + NS - 1, (it + NS - 1) % NS);
      compute_h(it % NS, [](int) {});
    }
  }

  // D[k][co]: lane holds k = kb + 4*(lane>>4) + i for co = cb + (lane & 15)
  const int lr = lane & 15, lh = lane >> 4;
  float* slab = a.slab + (long)(SUB ? phase * a.nsplit + split : split) * a.CW * a.KW;
#pragma unroll
  for (int i = 0; i < RK; ++i) {
    const int kb = k0 + wk * RK * 16 + i * 16 + lh * 4;
#pragma unroll
    for (int j = 0; j < RC; ++j) {
      const int co = c0 + wc * RC * 16 + j * 16 + lr;
      *reinterpret_cast<float4*>(slab + (long)co * a.KW + kb) =
          make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]);
    }
  }
  if (do_bias && lh == 0) {
#pragma unroll
    for (int j = 0; j < RC; ++j)
      a.bslab[(long)(SUB ? phase * a.nsplit + split : split) * a.CW + c0 + wc * RC * 16 + j * 16 + lr] = accb[j][0];
  }
}

// ----------------------------------------------------------------------------------------
// Sliding-row weight gradient of a 3x3 conv with 64 input channels (AFE.down1 64 -> 128 at
// full resolution), each operand byte read from HBM once: a block owns 128 co x ALL 9 taps x
// 64 ci (= 128 x 576, 36 accumulators per wave) and walks the rows [h0, h1) of one 64-column
// strip of one image.  Per row h it needs dy row h and x rows h-1, h, h+1; dy rows stream
// through a 3-deep ring, x rows through a 5-deep ring where each row lands once and stays for
// the three rows that read it (its tile-per-segment predecessor restaged dy per 32-channel
// k-tile and a fresh 3-row halo per segment: 2.76x the algorithmic bytes).  A "group" i = {dy row h0+i, x row
// h0+i+1} is issued two rows ahead; a wave's DMAs of a group are counted (wave 0 issues 4 of
// the 25 pieces, the others 3) so the wait for group i leaves group i+1 in flight.
//   8 waves = 2 (64 co) x 4 (9 of the 36 k-tiles of 16 = (tap, 16 ci)).
// Output: slab [block][cout][576] (k = tap * 64 + ci: wgrad_reduce_kernel's layout) and the
// bias slab [block][cout] (sum of dy by an all-ones MFMA operand, k-wave 0).
// ----------------------------------------------------------------------------------------
// (measured r5, not kept: one static s_setprio 1 for waves 4-7 instead of the per-half flips,
// and the second k-half's dy fragments read under the first half's last MFMA group -- res /
// down2 / down1 143 / 288 / 355 us either way, the prefetch variant spills at 256 VGPRs;
// profiles/r5/r5c_*)
template <int AHEAD>
__global__ void __launch_bounds__(512, 1)
conv3_halo_wgrad2(H3Wg2Args a) {
  // AHEAD groups in flight: group i + AHEAD is issued in row step i (HBM latency under load
  // is several row steps of MFMA work); rings: dy AHEAD + 1 deep, x AHEAD + 3 deep
  constexpr int XA = 1;                               // group i carries x row h0 + i + XA
  constexpr int BC = 128, NSD = AHEAD + 1, NSX = AHEAD + 2 + XA;
  constexpr int DYB = 64 * BC * 2;                    // 16 KB, 16 pieces
  constexpr int XQ = (66 * 128 + 1023) / 1024;        // 9 pieces per x row (66 px x 64 ci)
  constexpr int XB = XQ * 1024;
  constexpr int NPC = 16 + XQ;                        // pieces per group (25)
  __shared__ __attribute__((aligned(1024))) char smem[NSD * DYB + NSX * XB];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wc = wave & 1, wk = wave >> 1;
  const int li = lane & 15, g = lane >> 4;
  const int strips = a.W >> 6;
  // XCD-aware order (bijective remap, speed only): the nct x nci tiles of one (image, strip,
  // segment) -- the same dy and x rows -- are consecutive lids, dealt to one XCD's L2
  const int nblk = gridDim.x, bid = blockIdx.x;
  const int q8 = nblk / 8, r8 = nblk % 8, xcd = bid % 8;
  const int blk = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + bid / 8;
  const int ntile = a.nct * a.nci;
  const int tile = blk % ntile, tc = tile % a.nct, tci = tile / a.nct;
  const int split = blk / ntile;
  const int seg = split % a.nseg, strip = (split / a.nseg) % strips, n = split / (a.nseg * strips);
  const int co0 = tc * BC, w0 = strip * 64, ci0 = tci * 64;
  const int h0 = seg * a.rows, h1 = min(a.H, h0 + a.rows);
  const int nrow = h1 - h0;
  const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.x), 0, (int)a.xbytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t dr = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.dy), 0, (int)a.dybytes, 0x00020000);
  const unsigned sbase = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(lds_ptr_t)smem);

  // per-lane constants of this wave's pieces: piece q = wave + 8 j of a group (q < 16: dy,
  // else x piece q - 16); source offsets relative to the row start (0x80000000: outside)
  const int npw = wave == 0 ? 4 : 3;                  // pieces of a group this wave issues
  unsigned poff[4];
  int pisx[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int q = wave + 8 * j;
    pisx[j] = q >= 16;
    if (q < 16) {
      const int o = q * 1024 + lane * 16;
      const int px = o / (BC * 2), b = o - px * (BC * 2);
      const int co = ((((b >> 5) ^ tswz<BC>(px)) << 4) | (((b >> 4) & 1) << 3));
      poff[j] = (unsigned)((px * a.ldd + co0 + co) * 2);          // + row base * ldd * 2
    } else if (q < NPC) {
      const int o = (q - 16) * 1024 + lane * 16;
      const int px = o >> 7, b = o & 127;
      const int ci = ((((b >> 5) ^ tswz<64>(px)) << 4) | (((b >> 4) & 1) << 3));
      const int iw = w0 - 1 + px;
      poff[j] = (px < 66 && iw >= 0 && iw < a.W) ? (unsigned)((iw * a.ldx + ci0 + ci) * 2) : 0x80000000u;
    } else {
      poff[j] = 0x80000000u;
    }
  }
  // x row y (image row, may be outside) -> ring slot (y - h0 + 1) % NSX; dy row h -> (h - h0) % NSD
  auto issue_x = [&](int y, int j) {          // the wave's j-th piece when it is an x piece
    const int slot = (y - h0 + 1) % NSX;
    const int q = wave + 8 * j - 16;
    const bool rok = y >= 0 && y < a.H;               // wave-uniform (the column test is in poff)
    dma16s(xr, sbase + NSD * DYB + slot * XB + q * 1024, rok ? poff[j] : 0x80000000u,
           rok ? (unsigned)(((n * a.H + y) * a.W) * a.ldx * 2) : 0u);
  };
  // pieces q = wave + 8 j: j = 0, 1 are dy pieces (q < 16), j = 2 the x piece wave, j = 3 x
  // piece 8 for wave 0 only (pisx / npw as compile-time structure: no per-piece branches)
  auto issue_group = [&](int i) {             // dy row h0 + i, x row h0 + i + XA
    const int h = h0 + i;
    const unsigned dbase = sbase + (i % NSD) * DYB;
    const unsigned drow = (unsigned)((((n * a.H + h) * a.W + w0) * a.ldd) * 2);
    dma16s(dr, dbase + wave * 1024, poff[0], drow);
    dma16s(dr, dbase + (wave + 8) * 1024, poff[1], drow);
    issue_x(h + XA, 2);
    if (wave == 0) issue_x(h + XA, 3);
  };
  auto issue_xonly = [&](int y) {             // prologue rows h0 - 1 .. h0 + XA - 1
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < npw && pisx[j]) issue_x(y, j);
  };

#pragma unroll
  for (int y = -1; y < XA; ++y) issue_xonly(h0 + y);
#pragma unroll
  for (int i = 0; i < AHEAD; ++i)
    if (i < nrow) issue_group(i);
  // the wave's k-wave index as a compile-time constant (its 9 k-tiles, and the bias MFMAs of
  // k-wave 0, then need no registers)
  with_const<0, 4>(wk, [&](auto wkc) {
    constexpr int WK = decltype(wkc)::value;
    constexpr bool BIAS_W = WK == 0;
    f32x4 acc[4][9];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int j = 0; j < 9; ++j) acc[q][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 accb[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) accb[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    const bool do_bias = BIAS_W && a.bslab && tci == 0;
    bf16x8 ones;
#pragma unroll
    for (int i = 0; i < 8; ++i) ones[i] = (bf16)1.0f;
    // transposed-read lane constants, hoisted out of the row loop: both images' swizzles have
    // a 16-row period and every fragment starts at kk * 32 (+ the tap column for x), so a
    // read's address is slot base + lane constant (per fragment and 4-row half) + an immediate
    // (the same addresses as tfrag: bit-identical)
    unsigned lcd[4][2], lcx[9][2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int rl = 8 * g + 4 * h + (li >> 2);
#pragma unroll
      for (int q = 0; q < 4; ++q) lcd[q][h] = (unsigned)timg_off<BC>(rl, wc * 64 + q * 16 + 4 * (li & 3));
#pragma unroll
      for (int j = 0; j < 9; ++j) {
        const int kt = 9 * WK + j, tap = kt >> 2;
        lcx[j][h] = (unsigned)timg_off<64>(tap % 3 + rl, (kt & 3) * 16 + 4 * (li & 3));
      }
    }
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    auto frag2 = [](const char* base, unsigned l0, unsigned l1, int off) {
      FV_LDS char* lb = (FV_LDS char*)(base) + off;
      const s16x4 t0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((FV_LDS s16x4*)(lb + l0));
      const s16x4 t1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((FV_LDS s16x4*)(lb + l1));
      const s16x8 v = {t0[0], t0[1], t0[2], t0[3], t1[0], t1[1], t1[2], t1[3]};
      return __builtin_bit_cast(bf16x8, v);
    };
    // ring slots of the step's dy row and x rows h - 1 .. h + 1, advanced with a wrap (scalar):
    // each read address is then lane constant + slot base (one add per distinct address and
    // step, the two k-halves by immediate offsets) -- the compiler's strength-reduced
    // (i + r) % NSX took ~100 vector adds per step (r6)
    int sd = 0, sx = 0;
    for (int i = 0; i < nrow; ++i) {
      // group i landed; the younger groups issued so far (up to AHEAD - 1) may stay in flight:
      // steady state 3 (AHEAD - 1) groups of npw pieces, counted at compile time per npw
      if (i + AHEAD - 1 < nrow) {
        if (npw == 4) wait_vm<4 * (AHEAD - 1)>();
        else wait_vm<3 * (AHEAD - 1)>();
      } else {
        wait_vm_dyn((nrow - 1 - i) * npw);
      }
      wait_lgkm0();
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      if (i + AHEAD < nrow) issue_group(i + AHEAD);
      unsigned bd = (unsigned)(sd * DYB), bx[3];
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const int t = sx + r;
        bx[r] = (unsigned)(NSD * DYB + (t >= NSX ? t - NSX : t) * XB);
      }
      asm volatile("" : "+s"(bd), "+s"(bx[0]), "+s"(bx[1]), "+s"(bx[2]));
      sd = sd + 1 == NSD ? 0 : sd + 1;
      sx = sx + 1 == NSX ? 0 : sx + 1;
      unsigned ad[4][2], ax[9][2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int q = 0; q < 4; ++q) ad[q][h] = lcd[q][h] + bd;
#pragma unroll
        for (int j = 0; j < 9; ++j) ax[j][h] = lcx[j][h] + bx[((9 * WK + j) >> 2) / 3];
      }
      const char* const dys = smem;
      // x fragment of k-tile j of k-half kk (tap row / column constant after unrolling)
      auto xfrag = [&](int j, int kk) { return frag2(smem, ax[j][0], ax[j][1], kk * 32 * 128); };
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        bf16x8 af[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) af[q] = frag2(dys, ad[q][0], ad[q][1], kk * 32 * BC * 2);
        // the next x fragment is read before the current one's 4 MFMAs so the LDS latency hides
        // under them
        bf16x8 bcur = xfrag(0, kk);
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int j = 0; j < 9; ++j) {
          bf16x8 bnext = bcur;
          if (j + 1 < 9) bnext = xfrag(j + 1, kk);
#pragma unroll
          for (int q = 0; q < 4; ++q) acc[q][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[q], bcur, acc[q][j], 0, 0, 0);
          bcur = bnext;
        }
        if (do_bias) {
#pragma unroll
          for (int q = 0; q < 4; ++q) accb[q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[q], ones, accb[q], 0, 0, 0);
        }
        __builtin_amdgcn_s_setprio(0);
      }
    }
    // slab[split][co][tap * Cin + ci]: lane holds D[co = 4g + jj][k-col = li]
    const long KW = 9L * a.ldx;
    float* sl = a.slab + (long)split * a.Cout * KW;
#pragma unroll
    for (int j = 0; j < 9; ++j) {
      const int kt = 9 * WK + j, tap = kt >> 2;
      const int kcol = tap * a.ldx + ci0 + (kt & 3) * 16 + li;
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) sl[(long)(co0 + wc * 64 + q * 16 + 4 * g + jj) * KW + kcol] = acc[q][j][jj];
    }
    if (do_bias && li == 0) {
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj)
          a.bslab[(long)split * a.Cout + co0 + wc * 64 + q * 16 + 4 * g + jj] = accb[q][jj];
    }
  });
}

// ----------------------------------------------------------------------------------------
// Sub-pixel weight gradient of the UpBlock2D convs (nearest x2 upsample + 3x3, modules.py:78-89;
// VERDICT r4 item 2) on the sliding-row structure of conv3_halo_wgrad2: output row Y = 2h + pa,
// column X = 2w + pb reads the low-res rows h + pa + rr - 1 and columns w + pb + ss - 1
// (rr, ss in {0, 1}), so the gradient of the 4 phases' 2x2 weights is
//   D[pa pb][co][(rr ss), ci] = sum_{h, w} dy[2h + pa][2w + pb][co] * x[h + pa + rr - 1][w + pb + ss - 1][ci]
// (4/9 of the MACs of the upsampled 3x3; wgrad_reduce_subpix folds the phases back).  A block
// owns 64 co x 64 ci x all 16 (phase, tap) pairs and walks the low-res rows of `spb` consecutive
// (image, 64-column output strip) units.  Step h = output rows 2h, 2h + 1 (one dy group, 2 x 8
// KB) and the low-res x rows h - 1 .. h + 1 (a ring; one new 34-pixel row per step).  The dy
// rows land PHASE-MAJOR in LDS -- LDS row pb * 32 + w holds output pixel 2w + pb (the per-lane
// DMA source chooses the pixel) -- so a phase's A fragment (16 co x 32 pixels) is one
// transposed read pair, like every x fragment (16 ci x 32 low-res pixels at column shift
// pb + ss).  Wave (pa, pb, rr) = wave bits (0, 1, 2): 4 co tiles x 2 ss x 4 ci tiles = 32
// accumulators, 4 A + 8 B fragments per 32 MFMAs.  Output: the sub-pixel slab layout of
// conv_wgrad_v2 <SUB> ([phase][split][co][(rr * 2 + ss) * Cin + ci]) and the per-phase bias slab
// (dy sums by an all-ones operand, the rr = 0 waves of ci tile 0).
// ----------------------------------------------------------------------------------------
template <int AHEAD>
__global__ void __launch_bounds__(512, 1)
conv3_up_wgrad(UpWgArgs a) {
  // a step = 2 low-res rows (4 dy rows): 64 MFMAs per wave between barriers (one low-res row per
  // step measured 170 us per UpBlock2D conv at B = 32: the per-step barrier, waits and DMA issue
  // were not amortised over 32 MFMAs)
  constexpr int RPS = 2;
  constexpr int BC = 64, NSD = AHEAD + 1, NSX = (AHEAD + 1) * RPS + 2;
  constexpr int DYR = 64 * BC * 2, DYB = 2 * RPS * DYR; // one dy row 8 KB (8 pieces), a group 32 KB
  constexpr int XQ = 5, XB = XQ * 1024;               // x row: 34 px x 128 B = 4352 B -> 5 pieces
  constexpr int NDY = 16 * RPS, NPC = NDY + XQ * RPS; // pieces per group: dy rows, then x rows
  __shared__ __attribute__((aligned(1024))) char smem[NSD * DYB + NSX * XB];
  char* const dyr = smem;
  char* const xr_ = smem + NSD * DYB;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int pa = wave & 1, pb = (wave >> 1) & 1, rr = wave >> 2;
  const int li = lane & 15, g = lane >> 4;
  // XCD-aware order: the nct x nci tiles of one split (the same dy and x rows) are consecutive
  const int nblk = gridDim.x, bid = blockIdx.x;
  const int q8 = nblk / 8, r8 = nblk % 8, xcd = bid % 8;
  const int blk = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + bid / 8;
  const int ntile = a.nct * a.nci;
  const int tile = blk % ntile, tc = tile % a.nct, tci = tile / a.nct;
  const int split = blk / ntile;
  const int co0 = tc * BC, ci0 = tci * 64;
  const int Wo = 2 * a.Win, strips = Wo >> 6;
  const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.x), 0, (int)a.xbytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t dr = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.dy), 0, (int)a.dybytes, 0x00020000);
  const unsigned sbase = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(lds_ptr_t)smem);

  // this wave's pieces of a group: piece `wave` of each of the 2 RPS dy rows (one lane offset
  // for all of them: the lane's source pixel / channel within the strip row), and x pieces
  // xq = wave (+ 8 for waves 0, 1) of the group's RPS x rows (row xq / XQ, piece xq % XQ).  Few
  // wave-uniform values: per-piece conditions and offsets kept in SGPRs spilled 169 of them
  static_assert(NDY == 8 * 2 * RPS && XQ * RPS <= 16, "piece assignment");
  constexpr int NXP = XQ * RPS;
  const int nxw = (NXP - wave + 7) / 8;               // x pieces of this wave (1 or 2)
  const int npw = 2 * RPS + nxw;
  unsigned dyoff;
  {
    const int o = wave * 1024 + lane * 16;
    const int rho = o >> 7, b = o & 127;
    const int co = (((b >> 5) ^ tswz<BC>(rho)) << 4) | (((b >> 4) & 1) << 3);
    const int px = 2 * (rho & 31) + (rho >> 5);       // phase-major rows
    dyoff = (unsigned)((px * a.ldd + co0 + co) * 2);
  }
  int xrho[2], xci[2];
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const int xq = wave + 8 * m;
    const int o = (xq % XQ) * 1024 + lane * 16;
    const int rho = o >> 7, b = o & 127;
    xci[m] = ci0 + ((((b >> 5) ^ tswz<64>(rho)) << 4) | (((b >> 4) & 1) << 3));
    xrho[m] = rho;                                    // < 34: a pixel of the row
  }

  // lane constants of the transposed reads (rows: the phase's 32 pixels; x rows shifted by
  // pb + ss), as conv3_halo_wgrad2's lcd / lcx
  unsigned lcd[4][2], lcx[2][4][2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int rl = 8 * g + 4 * h + (li >> 2);
#pragma unroll
    for (int q = 0; q < 4; ++q) lcd[q][h] = (unsigned)timg_off<BC>(pb * 32 + rl, q * 16 + 4 * (li & 3));
#pragma unroll
    for (int ss = 0; ss < 2; ++ss)
#pragma unroll
      for (int u = 0; u < 4; ++u) lcx[ss][u][h] = (unsigned)timg_off<64>(pb + ss + rl, u * 16 + 4 * (li & 3));
  }
  typedef short s16x8 __attribute__((ext_vector_type(8)));
  auto frag2 = [](const char* base, unsigned l0, unsigned l1) {
    FV_LDS char* lb = (FV_LDS char*)(base);
    const s16x4 t0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((FV_LDS s16x4*)(lb + l0));
    const s16x4 t1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((FV_LDS s16x4*)(lb + l1));
    const s16x8 v = {t0[0], t0[1], t0[2], t0[3], t1[0], t1[1], t1[2], t1[3]};
    return __builtin_bit_cast(bf16x8, v);
  };

  f32x4 acc[4][2][4];
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int ss = 0; ss < 2; ++ss)
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[q][ss][u] = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 accb[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) accb[q] = f32x4{0.f, 0.f, 0.f, 0.f};
  const bool do_bias = a.bslab && tci == 0 && rr == 0;
  bf16x8 ones;
#pragma unroll
  for (int i = 0; i < 8; ++i) ones[i] = (bf16)1.0f;

  const int u0 = split * a.spb, u1 = min(a.units, u0 + a.spb);
  const int nstep = a.Hin / RPS;
  for (int un = u0; un < u1; ++un) {
    const int n = un / strips, w0 = (un % strips) * 64, wl0 = w0 >> 1;
    if (un > u0) __syncthreads();                    // the previous unit's last reads of the rings
    // per unit: the x pieces' source offsets with the strip's column validity (0x80000000 =
    // zero fill: halo columns outside the image, LDS rows past the 34 pixels)
    unsigned xv[2];
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const int col = wl0 - 1 + xrho[m];
      xv[m] = (xrho[m] < 34 && col >= 0 && col < a.Win) ? (unsigned)((col * a.Cin + xci[m]) * 2) : 0x80000000u;
    }
    // x row y (low-res; -1 and Hin are the zero padding) -> ring slot (y + 1) % NSX
    auto issue_x = [&](int y, int m) {
      const int xq = wave + 8 * m;
      const bool rok = y >= 0 && y < a.Hin;
      dma16s(xr, sbase + NSD * DYB + ((y + 1) % NSX) * XB + (xq % XQ) * 1024, rok ? xv[m] : 0x80000000u,
             rok ? (unsigned)((n * a.Hin + y) * a.Win) * (unsigned)a.Cin * 2u : 0u);
    };
    // group i: dy rows 2 RPS i .. + 2 RPS - 1, x rows RPS i + 1 .. RPS i + RPS
    auto issue_group = [&](int i) {
      const unsigned rb = (unsigned)(((n * 2 * a.Hin + 2 * RPS * i) * Wo + w0) * a.ldd) * 2u;
      const unsigned rs = (unsigned)(Wo * a.ldd) * 2u;
#pragma unroll
      for (int k = 0; k < 2 * RPS; ++k)
        dma16s(dr, sbase + (i % NSD) * DYB + k * DYR + wave * 1024, dyoff, rb + k * rs);
#pragma unroll
      for (int m = 0; m < 2; ++m)
        if (m < nxw) issue_x(RPS * i + 1 + (wave + 8 * m) / XQ, m);
    };
    // prologue: x rows -1 .. RPS - 2 = "group -1"'s x rows
#pragma unroll
    for (int m = 0; m < 2; ++m)
      if (m < nxw) issue_x(1 - RPS + (wave + 8 * m) / XQ, m);
#pragma unroll
    for (int i = 0; i < AHEAD; ++i)
      if (i < nstep) issue_group(i);

    for (int i = 0; i < nstep; ++i) {
      // group i landed; the younger groups issued so far (up to AHEAD - 1) may stay in flight
      const int younger = min(AHEAD - 1, nstep - 1 - i);
      wait_vm_dyn(younger * npw);
      wait_lgkm0();
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      if (i + AHEAD < nstep) issue_group(i + AHEAD);
#pragma unroll
      for (int hh = 0; hh < RPS; ++hh) {
        const int h = RPS * i + hh;
        const char* dys = dyr + (i % NSD) * DYB + (2 * hh + pa) * DYR;   // dy row 2h + pa
        const char* xs = xr_ + ((h + pa + rr) % NSX) * XB;              // low-res row h + pa + rr - 1
        bf16x8 af[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) af[q] = frag2(dys, lcd[q][0], lcd[q][1]);
        bf16x8 bcur = frag2(xs, lcx[0][0][0], lcx[0][0][1]);
#pragma unroll
        for (int t = 0; t < 8; ++t) {
          const int ss = t >> 2, u = t & 3;
          bf16x8 bnext = bcur;
          if (t + 1 < 8) bnext = frag2(xs, lcx[(t + 1) >> 2][(t + 1) & 3][0], lcx[(t + 1) >> 2][(t + 1) & 3][1]);
#pragma unroll
          for (int q = 0; q < 4; ++q) acc[q][ss][u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[q], bcur, acc[q][ss][u], 0, 0, 0);
          bcur = bnext;
        }
        if (do_bias) {
#pragma unroll
          for (int q = 0; q < 4; ++q) accb[q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[q], ones, accb[q], 0, 0, 0);
        }
      }
    }
  }
  // slab[(phase * nsplit + split)][co][(rr * 2 + ss) * Cin + ci]: lane holds D[co = 4g + jj][ci = li]
  const int ph = pa * 2 + pb;
  const long KW = 4L * a.Cin;
  float* sl = a.slab + (long)(ph * a.nsplit + split) * a.Cout * KW;
#pragma unroll
  for (int ss = 0; ss < 2; ++ss)
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int kcol = (rr * 2 + ss) * a.Cin + ci0 + u * 16 + li;
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) sl[(long)(co0 + q * 16 + 4 * g + jj) * KW + kcol] = acc[q][ss][u][jj];
    }
  if (do_bias && li == 0) {
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) a.bslab[(long)(ph * a.nsplit + split) * a.Cout + co0 + q * 16 + 4 * g + jj] = accb[q][jj];
  }
}

// ----------------------------------------------------------------------------------------
// Weight gradient of the 7x7 64 -> <= 4 channel conv (Generator.out_conv), "row taps in N":
//   D[(s, ci)][(r, co)] = sum_{x row h, column w} x[h][w + s - 3][ci] * dy[h - r + 3][w][co]
//                      = dW[co][ci][r][s]
// M = 7 column taps x 64 ci = 448 (28 m-tiles), N = 7 row taps x 4 co = 28 of 32 (2 n-tiles),
// K = x pixels: 3.5x fewer MFMAs than M = 3136, N = 3 -> 16.  A block walks the x rows of a
// 64-column strip segment: per row the x row (70 columns incl. the column halo) lands in LDS
// by DMA (double buffered) and the dy row 3 below it is transposed into a ring of 8
// channel-major dy rows, from which a B fragment (8 consecutive columns of one (r, co)) is a
// single ds_read_b128; A fragments are transposed reads (pixels are the MFMA K) of the x row.
// Output: per-block fp32 slabs [block][32][448] (n = r*4 + co, m = s*64 + ci) + bias sums.
// ----------------------------------------------------------------------------------------
__global__ void __launch_bounds__(512, 2)
conv7_n3_wgrad(W7Args a) {
  constexpr int XROW = 9 * 1024;                            // 70 px x 128 B, padded to whole pieces
  constexpr int XQ = 70 * 128 / 1024 + 1;                    // 9 pieces (the last one partly past 70 px)
  __shared__ __attribute__((aligned(1024))) char smem[2 * XROW + 2 * 1024 + 8 * 512];
  char* xb = smem;                                           // [2][70 px][64 ci] (timg_off<64> layout)
  char* dys = smem + 2 * XROW;                               // [2][64 px][8 ch] as stored in dy
  bf16* dyT = reinterpret_cast<bf16*>(smem + 2 * XROW + 2 * 1024);   // [8 rows][4 co][64 w]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, g = lane >> 4;
  const int strips = a.W / 64;
  const int blk = blockIdx.x;
  const int seg = blk % a.nseg, strip = (blk / a.nseg) % strips, n = blk / (a.nseg * strips);
  const int w0 = strip * 64;
  const int hb = seg * a.seg_rows, he = min(a.H, hb + a.seg_rows);
  const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.x), 0, (int)a.xbytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t dr = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.dy), 0, (int)a.dybytes, 0x00020000);

  // x row h -> xb[buf] (pixel p = column w0 - 3 + p; 32-B blocks XOR-swizzled, timg_off<64>)
  auto issue_x = [&](int h, int buf) {
    for (int q = wave; q < XQ; q += 8) {
      const int o = q * 1024 + lane * 16;
      const int p = o >> 7, b = o & 127;
      const int ci = ((((b >> 5) ^ tswz<64>(p)) << 4) | (((b >> 4) & 1) << 3));
      const int ww = w0 - 3 + p;
      const bool ok = p < 70 && h >= 0 && h < a.H && ww >= 0 && ww < a.W;
      dma16(xr, xb + buf * XROW + q * 1024,
            ok ? (unsigned)((((n * a.H + h) * a.W + ww) * 64 + ci) * 2) : 0x80000000u);
    }
  };
  // dy row y (64 px x ldd = 8 channels = 1 KB) -> dys[buf], one piece by wave 0
  auto issue_dy = [&](int y, int buf) {
    if (wave == 0) {
      const bool ok = y >= 0 && y < a.H;
      dma16(dr, dys + buf * 1024, ok ? (unsigned)((((n * a.H + y) * a.W + w0) * 8) * 2 + lane * 16) : 0x80000000u);
    }
  };
  // dys[buf] -> dyT[y & 7] (channel-major; zero rows outside the image / channels >= cout)
  auto transpose_dy = [&](int y, int buf) {
    if (tid < 256) {
      const int w = tid & 63, co = tid >> 6;
      const bf16 v = (y >= 0 && y < a.H && co < a.cout) ? reinterpret_cast<const bf16*>(dys + buf * 1024)[w * 8 + co]
                                                          : (bf16)0.f;
      dyT[((y & 7) * 4 + co) * 64 + w] = v;
    }
  };

  // prologue: dy rows hb-3 .. hb+2 straight into the ring (plain loads), first x / dy DMAs
  for (int e = tid; e < 6 * 256; e += 512) {
    const int y = hb - 3 + e / 256, w = e & 63, co = (e >> 6) & 3;
    bf16 v = (bf16)0.f;
    if (y >= 0 && y < a.H && co < a.cout)
      v = reinterpret_cast<const bf16*>(a.dy)[((long)(n * a.H + y) * a.W + w0 + w) * 8 + co];
    dyT[((y & 7) * 4 + co) * 64 + w] = v;
  }
  issue_x(hb, 0);
  issue_dy(hb + 3, 0);

  // this wave's m-tiles: w, w + 8, w + 16, w + 24 (< 28), each with both n-tiles
  const int nmt = wave < 4 ? 4 : 3;
  f32x4 acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i][0] = acc[i][1] = f32x4{0.f, 0.f, 0.f, 0.f};
  float bsum = 0.f;                                          // bias gradient: this thread's (w, co)

  for (int h = hb; h < he; ++h) {
    const int buf = (h - hb) & 1;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();                                         // x row h, dy row h+3 landed; step h-1 done
    transpose_dy(h + 3, buf);
    if (h + 1 < he) {
      issue_x(h + 1, buf ^ 1);
      issue_dy(h + 4, buf ^ 1);
    }
    __syncthreads();                                         // dy row h+3 visible in the ring
    if (tid < 256) {
      const int w = tid & 63, co = tid >> 6;
      bsum += (float)dyT[((h & 7) * 4 + co) * 64 + w];
    }
    const char* xbuf = xb + buf * XROW;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      bf16x8 bfr[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int nn = t * 16 + li, r = nn >> 2, co = nn & 3;
        const int y = h - r + 3;
        bf16x8 v = *reinterpret_cast<const bf16x8*>(dyT + ((y & 7) * 4 + co) * 64 + kk * 32 + g * 8);
        if (r > 6) v = bf16x8{};
        bfr[t] = v;
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (i < nmt) {
          const int mt = wave + 8 * i, s7 = mt >> 2, cb = (mt & 3) * 16;
          const bf16x8 afr = tfrag<64>(xbuf, kk * 32 + s7, cb, lane);
          acc[i][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afr, bfr[0], acc[i][0], 0, 0, 0);
          acc[i][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afr, bfr[1], acc[i][1], 0, 0, 0);
        }
      }
    }
  }
  // slab[blk][n][m]: lane holds D[m = mt*16 + 4g + j][n = t*16 + li]
  float* sl = a.slab + (long)blk * 32 * 448;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (i < nmt) {
      const int mt = wave + 8 * i;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) sl[(t * 16 + li) * 448 + mt * 16 + 4 * g + j] = acc[i][t][j];
    }
  }
  // bias: sum over the 64 columns of each co (waves 0..3 hold co = wave)
  if (a.bslab && tid < 256) {
    const float t = wave_sum(bsum);
    if (lane == 0) a.bslab[blk * 4 + wave] = t;
  }
}

// slabs [nblk][32][448] + [nblk][4] -> dW[co][64][7][7], db[co] in two deterministic passes.
// Pass 1: block (column chunk, group g) sums the slab rows [g*rpg, (g+1)*rpg) of 64 columns
// (4 waves x rows strided by 4, 4 loads in flight per lane) and stores the partial in place
// over row g*rpg.  Pass 2 sums the G partials in order.  Column e < 12544 is slab element
// (n = e / 448, m = e % 448); e in [12544, 12548) is bias co = e - 12544.
constexpr int W7_COLS = 28 * 448;
__device__ __forceinline__ float* w7_elem(float* slab, float* bslab, int b, int e) {
  return e < W7_COLS ? slab + (long)b * 32 * 448 + e : bslab + b * 4 + (e - W7_COLS);
}

__global__ void __launch_bounds__(256)
w7_reduce1_kernel(float* slab, float* bslab, int nblk, int rpg, int ncol) {
  const int e = blockIdx.x * 64 + (threadIdx.x & 63), sg = threadIdx.x >> 6;
  const int b0 = blockIdx.y * rpg, b1 = min(nblk, b0 + rpg);
  __shared__ float red[4][64];
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  if (e < ncol) {
    int b = b0 + sg;
    for (; b + 12 < b1; b += 16) {
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[u] += *w7_elem(slab, bslab, b + 4 * u, e);
    }
    for (; b < b1; b += 4) acc[0] += *w7_elem(slab, bslab, b, e);
  }
  red[sg][threadIdx.x & 63] = (acc[0] + acc[1]) + (acc[2] + acc[3]);
  __syncthreads();
  if (sg == 0 && e < ncol && b0 < b1)
    *w7_elem(slab, bslab, b0, e) = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

__global__ void w7_reduce2_kernel(float* slab, float* bslab, int nblk, int rpg, int cout, float* dw, float* db) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= W7_COLS + (db ? cout : 0)) return;
  const int nn = e / 448, co = nn & 3;
  if (e < W7_COLS && co >= cout) return;
  float v = 0.f;
  for (int b = 0; b < nblk; b += rpg) v += *w7_elem(slab, bslab, b, e);
  if (e < W7_COLS) {
    const int r = nn >> 2, m = e - nn * 448, s7 = m >> 6, ci = m & 63;
    dw[((co * 64 + ci) * 7 + r) * 7 + s7] = v;
  } else {
    db[e - W7_COLS] = v;
  }
}

// ----------------------------------------------------------------------------------------
// Halo-tiled 7x7 weight gradient (bf16): Generator.out_conv 64->3 and AFE.in_conv 3->64.
//   dW[co][k = (tap, ci)] = sum_p dy[p][co] * x[p + off(tap)][ci]      (M = k, N = co, K = p)
// Persistent blocks (one per CU) walk TR x 64 pixel tiles; per tile the input halo and the
// dy tile land in LDS by DMA (double-buffered: tile t+1 streams in while t is computed),
// and every tap's A fragment is a transposed read (ds_read_b64_tr_b16) of the halo at the
// tap's shift -- the input is read from HBM ~once instead of 49x.  Accumulators stay in
// registers across tiles; one fp32 slab per block, reduced by wgrad_reduce_kernel.  The
// bias gradient uses the all-ones A operand trick (wave 0).
// Wave w owns n-tile (w % NT) and m-tiles w/NT, w/NT + 8/NT, ...  (NT = co tiles).
// ----------------------------------------------------------------------------------------
// PK (AFE.in_conv, <= 4 valid input channels of the 8 staged per pixel): k packed as
// k = r * 32 + s * 4 + ci (s = 7 a padding column, ci = 3 the zero channel), the weight layout
// conv7c4_fwd's forward reads -- 14 m-tiles instead of 25 (49 taps x 8 padded channels): a
// lane's 4 k are ci 0..3 of one tap = the first 8 B of the halo pixel at that tap's shift.
// The slab rows are these k (KW = 224); wgrad_reduce_kernel maps them back (KSL = 8).
template <int KS, int CIN, int NT, int TR, bool PK = false>
__global__ void __launch_bounds__(512, 2)
conv_halo_wgrad(HaloWgArgs a) {
  static_assert(!PK || (CIN == 8 && KS == 7), "packed 7x7 weight gradient: 8 staged channels");
  constexpr int PAD = KS / 2, TW = 64;
  constexpr int HR = TR + KS - 1, HW = TW + KS - 1;
  constexpr int CPP = CIN / 8;
  constexpr int HCH = HR * HW * CPP;
  constexpr int HQ = (HCH + 63) / 64;
  constexpr int LDD = NT == 1 ? 8 : NT * 16;       // dy channels staged per pixel
  constexpr int DCH = TR * TW * LDD / 8;
  constexpr int DQ = (DCH + 63) / 64;
  constexpr int HB = HQ * 1024, DB = DQ * 1024, BUF = HB + DB;
  constexpr int KT = PK ? KS * 32 : KS * KS * CIN;  // valid k
  constexpr int MTT = (KT + 15) / 16;               // m-tiles (16 k rows)
  // every wave owns m-tiles {wave, wave + 8, ...} and ALL NT n-tiles: the A fragment of an
  // m-tile (two transposed 8-B halo reads) feeds NT MFMAs.  (One n-tile per wave, as before,
  // paid two LDS reads per MFMA: LDS-bound at 21 % MFMA busy on AFE.in_conv, NT = 4.)
  constexpr int RMW = (MTT + 7) / 8;                // m-tiles per wave (max)
  constexpr int NKG = TR * TW / 32;                 // 32-pixel k-groups per tile
  __shared__ __attribute__((aligned(1024))) char smem[2 * BUF];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int mw = wave;
  const int li = lane & 15, g = lane >> 4, q4 = li >> 2, pp = li & 3;
  const int tiles_w = a.W / TW, tiles_h = a.H / TR;

  const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.x), 0, (int)a.xbytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t dr = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.dy), 0, (int)a.dybytes, 0x00020000);

  auto issue = [&](int tile, int buf) {
    const int n = tile / (tiles_h * tiles_w);
    const int rem = tile - n * tiles_h * tiles_w;
    const int h0 = (rem / tiles_w) * TR, w0 = (rem % tiles_w) * TW;
    char* halo = smem + buf * BUF;
    char* dys = halo + HB;
    for (int q = wave; q < HQ; q += 8) {
      const int L = q * 64 + lane;
      const int hp = L / CPP, ch = L - (L / CPP) * CPP;
      const int hr = hp / HW, hc = hp - (hp / HW) * HW;
      const int hh = h0 + hr - PAD, ww = w0 + hc - PAD;
      const int sc = ch ^ (hp & (CPP - 1));
      const bool ok = L < HCH && hh >= 0 && hh < a.H && ww >= 0 && ww < a.W;
      const unsigned off = ok ? (unsigned)((((n * a.H + hh) * a.W + ww) * CIN + sc * 8) * 2) : 0x80000000u;
      dma16(xr, halo + q * 1024, off);
    }
    for (int q = wave; q < DQ; q += 8) {
      const int L = q * 64 + lane;
      constexpr int CPR = LDD / 8;
      const int row = L / CPR, dch = L - (L / CPR) * CPR;
      const int sc = CPR >= 4 ? ((((dch >> 1) ^ tswz<LDD>(row)) << 1) | (dch & 1)) : dch;
      const int p = (n * a.H + h0 + row / TW) * a.W + w0 + (row % TW);
      const bool ok = L < DCH && sc * 8 < a.ldd;
      const unsigned off = ok ? (unsigned)((p * a.ldd + sc * 8) * 2) : 0x80000000u;
      dma16(dr, dys + q * 1024, off);
    }
  };

  // this lane's constant part of each A fragment: (tap offset, byte offset in the pixel)
  int aoff[RMW], akx[RMW];
  bool aok[RMW];
#pragma unroll
  for (int j = 0; j < RMW; ++j) {
    const int mt = mw + j * 8;
    const int k = mt * 16 + 4 * pp;                 // first of this lane's 4 k (same tap, same chunk)
    aok[j] = mt < MTT;                              // wave-uniform (transposed reads need EXEC = all)
    if constexpr (PK) {
      // s = 7 reads one column past the tap window (the next halo row's first pixel, or the
      // dy image after the last row): finite junk in rows the reduce never maps
      aoff[j] = k < KT ? (k >> 5) * HW + ((k >> 2) & 7) : 0;
      akx[j] = 0;
    } else {
      const int tap = k / CIN, ci = k - (k / CIN) * CIN;
      const int r = tap / KS, s = tap - (tap / KS) * KS;
      aoff[j] = k < KT ? r * HW + s : 0;            // k >= K rows: finite junk, never stored
      akx[j] = k < KT ? ci : 0;
    }
  }
  f32x4 acc[RMW][NT];
#pragma unroll
  for (int j = 0; j < RMW; ++j)
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[j][n] = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 accb[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) accb[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  const bool do_bias = a.bslab && wave == 7;        // a wave with the fewest m-tiles
  bf16x8 ones;
#pragma unroll
  for (int i = 0; i < 8; ++i) ones[i] = (bf16)1.0f;

  // fragments of k-group kg (B: dy[32 px][16 co] of every n-tile; A: the halo at each m-tile's
  // tap shift), all reads issued together before the k-group's MFMAs (one m-tile's 2 reads
  // right before its 4 MFMAs left the LDS latency exposed: AFE.in_conv 140.7 -> 131.4 us; the
  // k-groups double-buffered as well spill at 256 registers: 145.7)
  auto load_kg = [&](const char* halo, int kg, bf16x8 (&bfr)[NT], bf16x8 (&afr)[RMW]) {
    const char* dys = halo + HB;
    FV_LDS char* hl = (FV_LDS char*)(halo);
#pragma unroll
    for (int n = 0; n < NT; ++n) bfr[n] = tfrag<LDD>(dys, kg * 32, n * 16, lane);   // co >= LDD lanes: ignored
    // pixel rows 8g+q4 and 8g+4+q4 of this k-group -> halo pixel at tap (0,0)
    const int p0 = kg * 32 + 8 * g + q4, p1 = p0 + 4;
    const int hb0 = (p0 / TW) * HW + (p0 % TW), hb1 = (p1 / TW) * HW + (p1 % TW);
#pragma unroll
    for (int j = 0; j < RMW; ++j) {
      afr[j] = bf16x8{};
      if (aok[j]) {
        const int ha = hb0 + aoff[j], hb = hb1 + aoff[j];
        const int ca = ((akx[j] >> 3) ^ (ha & (CPP - 1))) * 16 + (akx[j] & 7) * 2;
        const int cb = ((akx[j] >> 3) ^ (hb & (CPP - 1))) * 16 + (akx[j] & 7) * 2;
        const s16x4 t0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((FV_LDS s16x4*)(hl + ha * CIN * 2 + ca));
        const s16x4 t1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((FV_LDS s16x4*)(hl + hb * CIN * 2 + cb));
        typedef short s16x8 __attribute__((ext_vector_type(8)));
        const s16x8 v = {t0[0], t0[1], t0[2], t0[3], t1[0], t1[1], t1[2], t1[3]};
        afr[j] = __builtin_bit_cast(bf16x8, v);
      }
    }
  };
  auto mfma_kg = [&](const bf16x8 (&bfr)[NT], const bf16x8 (&afr)[RMW]) {
#pragma unroll
    for (int j = 0; j < RMW; ++j)
#pragma unroll
      for (int n = 0; n < NT; ++n) acc[j][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afr[j], bfr[n], acc[j][n], 0, 0, 0);
    if (do_bias) {
#pragma unroll
      for (int n = 0; n < NT; ++n) accb[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, bfr[n], accb[n], 0, 0, 0);
    }
  };
  auto compute = [&](int buf) {
    const char* halo = smem + buf * BUF;
    if constexpr (RMW * NT <= 16) {
      for (int kg = 0; kg < NKG; ++kg) {
        bf16x8 b0[NT], a0[RMW];
        load_kg(halo, kg, b0, a0);
        mfma_kg(b0, a0);
      }
    } else {
      // many m-tiles per wave (64-channel input): each A fragment read right before its MFMAs
      const char* dys = halo + HB;
      FV_LDS char* hl = (FV_LDS char*)(halo);
      for (int kg = 0; kg < NKG; ++kg) {
        bf16x8 bfr[NT];
#pragma unroll
        for (int n = 0; n < NT; ++n) bfr[n] = tfrag<LDD>(dys, kg * 32, n * 16, lane);
        const int p0 = kg * 32 + 8 * g + q4, p1 = p0 + 4;
        const int hb0 = (p0 / TW) * HW + (p0 % TW), hb1 = (p1 / TW) * HW + (p1 % TW);
#pragma unroll
        for (int j = 0; j < RMW; ++j) {
          bf16x8 af = bf16x8{};
          if (aok[j]) {
            const int ha = hb0 + aoff[j], hb = hb1 + aoff[j];
            const int ca = ((akx[j] >> 3) ^ (ha & (CPP - 1))) * 16 + (akx[j] & 7) * 2;
            const int cb = ((akx[j] >> 3) ^ (hb & (CPP - 1))) * 16 + (akx[j] & 7) * 2;
            const s16x4 t0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((FV_LDS s16x4*)(hl + ha * CIN * 2 + ca));
            const s16x4 t1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((FV_LDS s16x4*)(hl + hb * CIN * 2 + cb));
            typedef short s16x8 __attribute__((ext_vector_type(8)));
            const s16x8 v = {t0[0], t0[1], t0[2], t0[3], t1[0], t1[1], t1[2], t1[3]};
            af = __builtin_bit_cast(bf16x8, v);
          }
#pragma unroll
          for (int n = 0; n < NT; ++n) acc[j][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bfr[n], acc[j][n], 0, 0, 0);
        }
        if (do_bias) {
#pragma unroll
          for (int n = 0; n < NT; ++n) accb[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, bfr[n], accb[n], 0, 0, 0);
        }
      }
    }
  };

  int tile = blockIdx.x;
  if (tile < a.ntiles) issue(tile, 0);
  for (int it = 0; tile < a.ntiles; ++it, tile += gridDim.x) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    wait_lgkm0();
    __builtin_amdgcn_s_barrier();
    if (tile + (int)gridDim.x < a.ntiles) issue(tile + gridDim.x, (it + 1) & 1);
    compute(it & 1);
  }

  // D[k][co]: lane holds k = mt*16 + 4*(lane>>4) + i for co = nt*16 + (lane & 15)
  float* slab = a.slab + (long)blockIdx.x * a.CW * a.KW;
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    const int co = n * 16 + li;
    if (co < a.cout) {
#pragma unroll
      for (int j = 0; j < RMW; ++j) {
        const int mt = mw + j * 8;
        if (mt < MTT)
          *reinterpret_cast<float4*>(slab + (long)co * a.KW + mt * 16 + g * 4) =
              make_float4(acc[j][n][0], acc[j][n][1], acc[j][n][2], acc[j][n][3]);
      }
      if (do_bias && g == 0) a.bslab[(long)blockIdx.x * a.CW + co] = accb[n][0];
    }
  }
}

// sub-pixel phase slabs [4][nsplit][CW][KW] (k = (r'*2+s')*cin + ci) -> dW [co][ci][3][3]:
// each 3x3 tap r takes, per phase row pa, the 2x2 tap r' whose folded range holds it
// (pa = 0: r' = r > 0; pa = 1: r' = r == 2), columns alike; + db from the bias slabs.
// One wave per 64 outputs, 4 lanes per output summing interleaved splits.
__global__ void wgrad_reduce_subpix_kernel(const float* __restrict__ slab, const float* __restrict__ bslab, float* dw,
                                           float* db, int nsplit, int CW, int KW, int cout, int cin_valid,
                                           int lgCin, int nb_main) {
  const int sg = threadIdx.x >> 6, l = threadIdx.x & 63;
  __shared__ float red[4][64];
  float g = 0.f;
  long dst = -1;
  const int nterm = 4 * nsplit;
  if ((int)blockIdx.x < nb_main) {
    const long e = (long)blockIdx.x * 64 + l;
    const long tot = (long)cout * cin_valid * 9;
    if (e < tot) {
      dst = e;
      const int rs = (int)(e % 9), ci = (int)((e / 9) % cin_valid), co = (int)(e / (9L * cin_valid));
      const int r = rs / 3, sc = rs % 3;
      for (int t = sg; t < nterm; t += 4) {
        const int ph = t / nsplit, sp = t - ph * nsplit;
        const int pa = ph >> 1, pb = ph & 1;
        const int rr = pa ? (r == 2) : (r > 0), ss = pb ? (sc == 2) : (sc > 0);
        g += slab[((long)(ph * nsplit + sp) * CW + co) * KW + (((rr * 2 + ss) << lgCin) + ci)];
      }
    }
  } else {
    const int co = ((int)blockIdx.x - nb_main) * 64 + l;
    if (co < cout) {
      dst = co;
      for (int t = sg; t < nterm; t += 4) g += bslab[(long)t * CW + co];
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

// Sub-pixel slabs of many splits (conv3_up_wgrad: ~one block per CU, 4 x 128 splits at
// 256^2), in two passes instead of the gather above (whose 9 (r, s) neighbours read 4 rows a
// cin apart: 117 us for the two UpBlock2D convs at B = 32):
// pass 1 sums each phase's splits over 64 consecutive slab elements x 4 split lanes (coalesced,
// fixed order) and writes the sum in place into the phase's split-0 row (every element is read
// by its own block only); blocks >= nb_main do the same for the bias slab.
__global__ void subpix_split_sum_kernel(float* __restrict__ slab, float* __restrict__ bslab, int nsplit, long rowlen,
                                        int CW, int nb_main) {
  const int sg = threadIdx.x >> 6, l = threadIdx.x & 63;
  __shared__ float red[4][64];
  float g = 0.f;
  float* base = nullptr;
  long stride = 0, e = -1;
  if ((int)blockIdx.x < nb_main) {
    e = (long)blockIdx.x * 64 + l;                   // element of the [phase][rowlen] sums
    if (e < 4 * rowlen) {
      const long ph = e / rowlen, k = e - ph * rowlen;
      base = slab + ph * nsplit * rowlen + k;
      stride = rowlen;
    }
  } else {
    e = (long)((int)blockIdx.x - nb_main) * 64 + l;
    if (e < 4L * CW) {
      const long ph = e / CW, co = e - ph * CW;
      base = bslab + ph * nsplit * CW + co;
      stride = CW;
    }
  }
  if (base)
    for (int sp = sg; sp < nsplit; sp += 4) g += base[sp * stride];
  red[sg][l] = g;
  __syncthreads();
  if (sg == 0 && base) base[0] = (red[0][l] + red[1][l]) + (red[2][l] + red[3][l]);
}

// pass 2: dW[co][ci][r][s] = sum over the 4 phases of the phase tap (rr, ss) that (r, s) maps to
// (the map of wgrad_reduce_subpix_kernel), db = the 4 phase sums
__global__ void subpix_fold_kernel(const float* __restrict__ slab, const float* __restrict__ bslab, float* dw, float* db,
                                   int nsplit, int CW, int KW, int cout, int cin_valid, int lgCin, int nb_main) {
  const long rowlen = (long)CW * KW;
  if ((int)blockIdx.x < nb_main) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long)cout * cin_valid * 9) return;
    const int rs = (int)(e % 9), ci = (int)((e / 9) % cin_valid), co = (int)(e / (9L * cin_valid));
    const int r = rs / 3, sc = rs % 3;
    float g = 0.f;
#pragma unroll
    for (int ph = 0; ph < 4; ++ph) {
      const int pa = ph >> 1, pb = ph & 1;
      const int rr = pa ? (r == 2) : (r > 0), ss = pb ? (sc == 2) : (sc > 0);
      g += slab[(long)ph * nsplit * rowlen + (long)co * KW + (((rr * 2 + ss) << lgCin) + ci)];
    }
    dw[e] = g;
  } else {
    const int co = ((int)blockIdx.x - nb_main) * blockDim.x + threadIdx.x;
    if (co >= cout) return;
    db[co] = (bslab[co] + bslab[(long)nsplit * CW + co]) + (bslab[2L * nsplit * CW + co] + bslab[3L * nsplit * CW + co]);
  }
}

// sum of the per-split slabs -> dW in the reference layout [co][ci][r][s] (+ db).  Block =
// 64 consecutive outputs x 4 split lanes (4 independent partial sums each), so that large
// split counts do not serialise on load latency; blocks >= nb_main reduce the bias slab.
// KSL: taps per row in the slab's k layout (KS, or 8 for the packed 7x7 rows of conv_halo_wgrad
// PK, whose s = 7 column is padding)
__global__ void wgrad_reduce_kernel(const float* __restrict__ slab, const float* __restrict__ bslab,
                                    float* dw, float* db, int nsplit, int CW, int KW, int K,
                                    int cout, int cin_valid, int lgCin, int KS, int nb_main, int KSL) {
  const int sg = threadIdx.x >> 6, l = threadIdx.x & 63;
  __shared__ float red[4][64];
  float g = 0.f;
  bool valid;
  long dst = 0;
  const float* p = nullptr;
  long stride;
  if ((int)blockIdx.x < nb_main) {
    const long e = (long)blockIdx.x * 64 + l;
    const int co = (int)(e / K), k = (int)(e - (e / K) * K);
    const int tap = k >> lgCin, c = k & ((1 << lgCin) - 1);
    const int r = tap / KSL, sx = tap - (tap / KSL) * KSL;
    valid = e < (long)cout * K && c < cin_valid && sx < KS;
    dst = (((long)co * cin_valid + c) * KS + r) * KS + sx;
    p = slab + (long)co * KW + k;
    stride = (long)CW * KW;
  } else {
    const int co = ((int)blockIdx.x - nb_main) * 64 + l;
    valid = db != nullptr && co < cout;
    dst = co;
    p = bslab + co;
    stride = CW;
  }
  if (valid) {
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    int s = sg;
    for (; s + 12 < nsplit; s += 16) {
      a0 += p[(long)s * stride];
      a1 += p[(long)(s + 4) * stride];
      a2 += p[(long)(s + 8) * stride];
      a3 += p[(long)(s + 12) * stride];
    }
    for (; s < nsplit; s += 4) a0 += p[(long)s * stride];
    g = (a0 + a1) + (a2 + a3);
  }
  red[sg][l] = g;
  __syncthreads();
  if (sg == 0 && valid) {
    const float t = (red[0][l] + red[1][l]) + (red[2][l] + red[3][l]);
    if ((int)blockIdx.x < nb_main) dw[dst] = t;
    else db[dst] = t;
  }
}

}  // namespace

#pragma GCC visibility push(hidden)

template <int KS, int CFG>
int launch_wg2_t(const Wg2Args& a, int ups, int nblk, hipStream_t s) {
  constexpr Wg2Cfg c = kWg2Cfg[CFG];
  if constexpr (KS == 2) {     // sub-pixel phases only
    if constexpr (CFG == 0 || CFG == 2 || CFG == 8) {
      hipLaunchKernelGGL((conv_wgrad_v2<2, c.bkt, c.bc, c.wk, c.wc, c.px, c.ns, false, true>), dim3(nblk), dim3(512), 0,
                         s, a);
      return FV_OK;
    } else {
      return FV_E_UNSUPPORTED;
    }
  } else {
  if (ups) {
    if constexpr (KS == 3)
      hipLaunchKernelGGL((conv_wgrad_v2<KS, c.bkt, c.bc, c.wk, c.wc, c.px, c.ns, true>), dim3(nblk), dim3(512), 0, s, a);
    else return FV_E_UNSUPPORTED;
  } else {
    hipLaunchKernelGGL((conv_wgrad_v2<KS, c.bkt, c.bc, c.wk, c.wc, c.px, c.ns, false>), dim3(nblk), dim3(512), 0, s, a);
  }
  return FV_OK;
  }
}

template <int KS, int CFG = 0>
int launch_wg2_ks(const Wg2Args& a, const WgPlan& p, int ups, int nblk, hipStream_t s) {
  if constexpr (CFG < kNumWg2Cfg) {
    if constexpr (KS != 3 && KS != 2 && CFG > 5) return FV_E_UNSUPPORTED;   // configs 6-8: 3x3 and sub-pixel only
    if (p.cfg == CFG) return launch_wg2_t<KS, CFG>(a, ups, nblk, s);
    return launch_wg2_ks<KS, CFG + 1>(a, p, ups, nblk, s);
  }
  return FV_E_UNSUPPORTED;
}

int launch_wg2(const Wg2Args& a, int ks, const WgPlan& p, int ups, int nblk, hipStream_t s) {
  if (p.sub) return launch_wg2_ks<2>(a, p, 0, nblk, s);
  switch (ks) {
    case 1: return launch_wg2_ks<1>(a, p, ups, nblk, s);
    case 3: return launch_wg2_ks<3>(a, p, ups, nblk, s);
    case 7: return launch_wg2_ks<7>(a, p, ups, nblk, s);
  }
  return FV_E_UNSUPPORTED;
}

template <typename T, int KS, int WK, int WC, int RK, int RC>
int launch_wg_t(const WgArgs& a, int pro, int ups, int nblk, hipStream_t s) {
  dim3 g(nblk), b(64 * WK * WC);
  if (pro && ups) {
    if constexpr (KS == 3) hipLaunchKernelGGL((conv_wgrad_kernel<T, KS, WK, WC, RK, RC, true, true>), g, b, 0, s, a);
    else return FV_E_UNSUPPORTED;
  } else if (pro) {
    if constexpr (KS != 7) hipLaunchKernelGGL((conv_wgrad_kernel<T, KS, WK, WC, RK, RC, true, false>), g, b, 0, s, a);
    else return FV_E_UNSUPPORTED;
  } else if (ups) {
    if constexpr (KS == 3) hipLaunchKernelGGL((conv_wgrad_kernel<T, KS, WK, WC, RK, RC, false, true>), g, b, 0, s, a);
    else return FV_E_UNSUPPORTED;
  } else {
    hipLaunchKernelGGL((conv_wgrad_kernel<T, KS, WK, WC, RK, RC, false, false>), g, b, 0, s, a);
  }
  return FV_OK;
}

template <typename T, int KS>
int launch_wg_ks(const WgArgs& a, const WgPlan& t, int pro, int ups, int nblk, hipStream_t s) {
  if (t.bc == 128) return launch_wg_t<T, KS, 2, 2, 4, 4>(a, pro, ups, nblk, s);
  if (t.bc == 64) return launch_wg_t<T, KS, 2, 2, 4, 2>(a, pro, ups, nblk, s);
  return launch_wg_t<T, KS, 4, 1, 2, 1>(a, pro, ups, nblk, s);
}

template <typename T>
void launch_s2_wg(const WgArgs& a, const WgPlan& t, int nblk, hipStream_t s) {
  dim3 g(nblk), b(256);
  if (t.bc == 128) hipLaunchKernelGGL((conv_wgrad_kernel<T, 3, 2, 2, 4, 4, false, false, 1>), g, b, 0, s, a);
  else if (t.bc == 64) hipLaunchKernelGGL((conv_wgrad_kernel<T, 3, 2, 2, 4, 2, false, false, 1>), g, b, 0, s, a);
  else hipLaunchKernelGGL((conv_wgrad_kernel<T, 3, 4, 1, 2, 1, false, false, 1>), g, b, 0, s, a);
}

template <typename T>
int launch_wg(const WgArgs& a, int ks, const WgPlan& t, int pro, int ups, int nblk, hipStream_t s) {
  switch (ks) {
    case 1: return launch_wg_ks<T, 1>(a, t, pro, ups, nblk, s);
    case 3: return launch_wg_ks<T, 3>(a, t, pro, ups, nblk, s);
    case 7: return launch_wg_ks<T, 7>(a, t, pro, ups, nblk, s);
  }
  return FV_E_UNSUPPORTED;
}

template int launch_wg<bf16>(const WgArgs&, int, const WgPlan&, int, int, int, hipStream_t);
template int launch_wg<float>(const WgArgs&, int, const WgPlan&, int, int, int, hipStream_t);
template void launch_s2_wg<bf16>(const WgArgs&, const WgPlan&, int, hipStream_t);
template void launch_s2_wg<float>(const WgArgs&, const WgPlan&, int, hipStream_t);

void launch_h3_wg2(const H3Wg2Args& a, int nblk, hipStream_t s) {
  hipLaunchKernelGGL(conv3_halo_wgrad2<4>, dim3(nblk), dim3(512), 0, s, a);
}
void launch_up_wg(const UpWgArgs& a, int nblk, hipStream_t s) {
  hipLaunchKernelGGL(conv3_up_wgrad<2>, dim3(nblk), dim3(512), 0, s, a);
}
void launch_c7_wg(const W7Args& a, int nblk, hipStream_t s) {
  hipLaunchKernelGGL(conv7_n3_wgrad, dim3(nblk), dim3(512), 0, s, a);
}
void launch_halo_wg(const HaloWgArgs& a, int cin, bool pk, int nblk, hipStream_t s) {
  if (cin == 8 && pk)
    hipLaunchKernelGGL((conv_halo_wgrad<7, 8, 4, 4, true>), dim3(nblk), dim3(512), 0, s, a);
  else if (cin == 8)
    hipLaunchKernelGGL((conv_halo_wgrad<7, 8, 4, 4>), dim3(nblk), dim3(512), 0, s, a);
  else
    hipLaunchKernelGGL((conv_halo_wgrad<7, 64, 1, 2>), dim3(nblk), dim3(512), 0, s, a);
}

void launch_w7_reduce(float* slab, float* bslab, int nsplit, int cout, float* dw, float* db, hipStream_t s) {
  // the two passes reuse the slab rows in place (the slabs are dead after the reduce)
  const int ncol = W7_COLS + (db ? 4 : 0);
  const int G = nsplit >= 256 ? 16 : (nsplit >= 16 ? 4 : 1);
  const int rpg = fv_cdiv(nsplit, G);
  hipLaunchKernelGGL(w7_reduce1_kernel, dim3(fv_cdiv(ncol, 64), G), dim3(256), 0, s, slab, bslab, nsplit, rpg, ncol);
  hipLaunchKernelGGL(w7_reduce2_kernel, dim3(fv_cdiv(ncol, 256)), dim3(256), 0, s, slab, bslab, nsplit, rpg, cout, dw, db);
}
void launch_subpix_split_sum(float* slab, float* bslab, int nsplit, long rowlen, int CW, int nb_main, int nb_bias,
                             hipStream_t s) {
  hipLaunchKernelGGL(subpix_split_sum_kernel, dim3(nb_main + nb_bias), dim3(256), 0, s, slab, bslab, nsplit, rowlen, CW,
                     nb_main);
}
void launch_subpix_fold(const float* slab, const float* bslab, float* dw, float* db, int nsplit, int CW, int KW, int cout,
                        int cin_valid, int lgCin, int nb_main, int nb_bias, hipStream_t s) {
  hipLaunchKernelGGL(subpix_fold_kernel, dim3(nb_main + nb_bias), dim3(256), 0, s, slab, bslab, dw, db, nsplit, CW, KW,
                     cout, cin_valid, lgCin, nb_main);
}
void launch_wgrad_reduce_subpix(const float* slab, const float* bslab, float* dw, float* db, int nsplit, int CW, int KW,
                                int cout, int cin_valid, int lgCin, int nb_main, int nb_bias, hipStream_t s) {
  hipLaunchKernelGGL(wgrad_reduce_subpix_kernel, dim3(nb_main + nb_bias), dim3(256), 0, s, slab, bslab, dw, db, nsplit,
                     CW, KW, cout, cin_valid, lgCin, nb_main);
}
void launch_wgrad_reduce(const float* slab, const float* bslab, float* dw, float* db, int nsplit, int CW, int KW, int K,
                         int cout, int cin_valid, int lgCin, int KS, int nb_main, int nb_bias, int KSL, hipStream_t s) {
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(nb_main + nb_bias), dim3(256), 0, s, slab, bslab, dw, db, nsplit, CW, KW,
                     K, cout, cin_valid, lgCin, KS, nb_main, KSL);
}

#pragma GCC visibility pop
