// 2-D convolution, the DMA-fed generic forward kernel conv_fwd_v2 (bf16, cin % 64 == 0) with its
// launcher.
#include "conv_common.h"

namespace {

// ----------------------------------------------------------------------------------------
// v2 forward (bf16, cin % 64 == 0): both operands land in LDS by DMA (buffer/global_load
// ... lds, no VGPR staging, no ds_write), BK = 64 (one tap x 64 channels per step), 128-B
// rows XOR-swizzled through the SOURCE address (the DMA destination is lane-linear),
// double-buffered with one barrier per step.  Zero padding comes from the buffer range
// check: an out-of-image tap gets voffset >= num_records and the hardware returns 0.
// ----------------------------------------------------------------------------------------
// MODE 0: plain conv; 1: nearest-x2 upsample folded into the addressing (tile space =
// output); 2: one sub-pixel phase of an upsample + 3x3 conv = a 2x2 conv over the low-res
// input with phase-folded weights (tile space = low-res image, block phase = lid & 3,
// KS == 2, taps at offsets {-1, 0} or {0, +1} per phase coordinate); 3: stride-2 4x4 conv
// (input coordinate 2 * out + tap - 1): the data gradient of an upsample + 3x3 conv
// straight at the low resolution (tile space = low-res dx, input = high-res dy).
template <int KS, int WN, int WM, int RN, int RM, int MODE, int BKS>
__global__ void __launch_bounds__(64 * WN * WM, (BKS == 32 && WN * WM == 4) ? 4 : 2)
conv_fwd_v2(ConvArgs a, unsigned x_bytes) {
  constexpr bool UPS = MODE == 1;
  constexpr int NW = WN * WM;
  constexpr int BN = WN * RN * 16, BM = WM * RM * 16;
  constexpr int PAD = KS / 2;
  constexpr int ROWB = BKS * 2;
  constexpr int CH = BKS / 8, RPP = 64 / CH;         // 16-B chunks per row, rows per 1-KB piece
  constexpr int QA = BM / RPP, QB = BN / RPP;        // 1-KB DMA pieces per stage
  constexpr int JA = (QA + NW - 1) / NW, JB = (QB + NW - 1) / NW;
  constexpr int STAGE = (BM + BN) * ROWB;
  __shared__ __attribute__((aligned(1024))) char smem[2 * STAGE];

  const int tid = threadIdx.x, lane = tid & 63;
  const int nks = a.nks * (64 / BKS);   // a.nks counts 64-deep steps
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wn = wave % WN, wm = wave / WN;
  // XCD-aware tile order: blocks b, b+8, ... share an XCD (observed round-robin dispatch);
  // give each XCD a contiguous run of logical tiles (co tiles of a pixel tile, then its
  // neighbours, which share halo rows).  Bijective for any grid size.  Speed only.
  const int nblk = gridDim.x, bid = blockIdx.x;
  const int q8 = nblk / 8, r8 = nblk % 8, xcd = bid % 8;
  const int lid0 = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + bid / 8;
  // MODE 2: the 4 phases of one low-res tile are neighbours (same input rows)
  const int phase = MODE == 2 ? (lid0 & 3) : 0;
  const int lid = MODE == 2 ? (lid0 >> 2) : lid0;
  if constexpr (MODE == 2) a.sub = 1 + phase;
  const int pa = phase >> 1, pb = phase & 1;
  // row / column tap offset: centred (MODE 0/1), per phase (MODE 2), -1 after the stride (3)
  const int roff = MODE == 2 ? pa - 1 : MODE == 3 ? -1 : -PAD;
  const int coff = MODE == 2 ? pb - 1 : MODE == 3 ? -1 : -PAD;
  constexpr int STR = MODE == 3 ? 2 : 1;
  const int tn = lid % a.ntn, tm = lid / a.ntn;
  const int co0 = tn * BN, p0 = tm * BM;
  const int HW = a.H * a.W;

  const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.x), 0, (int)x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.w), 0, 0x7fffffff, 0x00020000);
  const unsigned sbase = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(lds_ptr_t)smem);
  const int lrow = lane / CH, lchk = lane % CH;
  // per-piece constants.  A piece is RPP consecutive pixels of ONE image row (W % RPP == 0,
  // so p0 + RPP*q never straddles a row) x CH 16-B chunks: its image row (n, h) is wave-uniform and
  // the row part of the source address goes to soffset (SALU only); the lane's column part
  // for each tap column s is precomputed once, 0x80000000 marking a column outside the
  // image (the buffer range check then returns 0).  A k-step costs no address VALU beyond
  // selecting the tap column's register.
  int prn[JA], prh[JA];
  bool pok[JA];
  unsigned vcol[JA][KS];
#pragma unroll
  for (int j = 0; j < JA; ++j) {
    const int q = wave + j * NW;
    const int pp = __builtin_amdgcn_readfirstlane(p0 + q * RPP);
    pok[j] = (QA % NW == 0 || q < QA) && pp < a.P;
    const int n = pp / HW, rem = pp - n * HW;
    const int h = rem / a.W, w0 = rem - h * a.W;
    prn[j] = n * a.Hin;
    prh[j] = h;
    const unsigned chunk = (unsigned)((lchk ^ swzk<BKS>(q * RPP + lrow)) << 3);
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int ww = STR * (w0 + lrow) + s + coff;
      const int sc = UPS ? (ww >> 1) : ww;
      const int wlim = UPS ? a.W : a.Win;
      vcol[j][s] = (ww >= 0 && ww < wlim) ? ((unsigned)(sc << a.lgCin) + chunk) * 2u : 0x80000000u;
    }
  }
  unsigned wbase[JB];
#pragma unroll
  for (int j = 0; j < JB; ++j) {
    const int row = (wave + j * NW) * RPP + lrow;
    wbase[j] = (unsigned)(((co0 + row) * a.Kpad + ((lchk ^ swzk<BKS>(row)) << 3)) * 2);
  }

  auto issue = [&](int ks, int buf) {
    const int k0 = ks * BKS;
    const unsigned As = sbase + buf * STAGE;
    const unsigned Bs = As + BM * ROWB;
    const int tap = k0 >> a.lgCin, ci0 = k0 & (a.Cin - 1);
    const int r = tap / KS, s = tap - (tap / KS) * KS;
    with_const<0, KS>(s, [&](auto sc) {
      constexpr int S = decltype(sc)::value;
#pragma unroll
      for (int j = 0; j < JA; ++j) {
        const int q = wave + j * NW;
        if (QA % NW == 0 || q < QA) {
          const int hh = STR * prh[j] + r + roff;
          const int srow = UPS ? (hh >> 1) : hh;
          if (pok[j] && hh >= 0 && hh < (UPS ? a.H : a.Hin))
            dma16s(xr, As + q * 1024, vcol[j][S], (unsigned)((((prn[j] + srow) * a.Win) << a.lgCin) + ci0) * 2u);
          else
            dma16s(xr, As + q * 1024, 0x80000000u, 0u);
        }
      }
    });
#pragma unroll
    for (int j = 0; j < JB; ++j) {
      const int q = wave + j * NW;
      if (QB % NW == 0 || q < QB) dma16s(wr, Bs + q * 1024, wbase[j], (unsigned)((k0 + phase * a.wphase) * 2));
    }
  };

  f32x4 acc[RN][RM];
#pragma unroll
  for (int n = 0; n < RN; ++n)
#pragma unroll
    for (int m = 0; m < RM; ++m) acc[n][m] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int lr = lane & 15, lh = lane >> 4;
  // fragments of one 32-deep k half-step (kk) of LDS buffer `buf`
  auto load_frags = [&](Frag<bf16> (&fa)[RN], Frag<bf16> (&fb)[RM], int buf, int kk) {
    const char* As = smem + buf * STAGE;
    const char* Bs = As + BM * ROWB;
#pragma unroll
    for (int n = 0; n < RN; ++n) {
      const int row = wn * RN * 16 + n * 16 + lr;
      fa[n].lds(Bs + row * ROWB + (((kk * 4 + lh) ^ swzk<BKS>(row)) << 4));
    }
#pragma unroll
    for (int m = 0; m < RM; ++m) {
      const int row = wm * RM * 16 + m * 16 + lr;
      fb[m].lds(As + row * ROWB + (((kk * 4 + lh) ^ swzk<BKS>(row)) << 4));
    }
  };
  // s_setprio(1) around each MFMA cluster keeps hipcc from moving MFMAs across the raw
  // barriers into the DMA / fragment-read sections (guide T5)
  constexpr bool prio = true;
  auto mfma_all = [&](const Frag<bf16> (&fa)[RN], const Frag<bf16> (&fb)[RM]) {
    if (prio) __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int n = 0; n < RN; ++n)
#pragma unroll
      for (int m = 0; m < RM; ++m) acc[n][m] = mma(fa[n], fb[m], acc[n][m]);
    if (prio) __builtin_amdgcn_s_setprio(0);
  };

  if (BKS == 64) {
    // Software-pipelined k loop: the fragments of the next half-step are read while the
    // MFMAs of the current one run, and the per-step barrier sits between the two MFMA
    // groups of a step, so after it the matrix pipe has the second group (already in
    // registers) to work on while the next step's first fragments and DMAs are issued.
    //   step ks:  read F1(ks) | MFMA F0(ks) | vmcnt(0)+lgkmcnt(0), barrier | DMA ks+2 -> buf,
    //             read F0(ks+1) | MFMA F1(ks)
    // The barrier publishes stage ks+1 (every wave waited for its own DMAs) and retires all
    // reads of buffer ks&1 (each wave drained its reads first), which DMA ks+2 then refills.
    Frag<bf16> fa0[RN], fb0[RM], fa1[RN], fb1[RM];
    issue(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (nks > 1) issue(1, 1);
    load_frags(fa0, fb0, 0, 0);
    // steady state without branches around the fragment reads (a read on one path only
    // makes the compiler drain every LDS read before the next MFMA group)
    for (int ks = 0; ks + 1 < nks; ++ks) {
      const int buf = ks & 1;
      load_frags(fa1, fb1, buf, 1);
      mfma_all(fa0, fb0);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      wait_lgkm0();
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      if (ks + 2 < nks) issue(ks + 2, buf);
      load_frags(fa0, fb0, buf ^ 1, 0);
      mfma_all(fa1, fb1);
    }
    load_frags(fa1, fb1, (nks - 1) & 1, 1);
    mfma_all(fa0, fb0);
    mfma_all(fa1, fb1);
  } else {
    // one barrier per step, fragments read per 32-deep half-step (the BKS = 32 loop)
    issue(0, 0);
    for (int ks = 0; ks < nks; ++ks) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (ks + 1 < nks) issue(ks + 1, (ks + 1) & 1);
#pragma unroll
      for (int kk = 0; kk < BKS / 32; ++kk) {
        Frag<bf16> af[RN], bfm[RM];
        load_frags(af, bfm, ks & 1, kk);
        mfma_all(af, bfm);
      }
    }
  }
  __syncthreads();
  conv_epilogue<bf16, WN, WM, RN, RM, true>(a, acc, smem, co0, p0, MODE == 2 ? tm * 4 + phase : tm, wn, wm, lane,
                                             tid);
}

// mode: 0 plain, 1 upsample folded (KS 3), 2 sub-pixel phases (KS 2)
template <int KS, int WN, int WM, int RN, int RM, int BKS>
int launch_v2_b(const ConvArgs& a, int mode, int nblk, unsigned xb, hipStream_t s) {
  dim3 g(nblk), b(64 * WN * WM);
  if (mode == 3) {
    if constexpr (KS == 4) hipLaunchKernelGGL((conv_fwd_v2<KS, WN, WM, RN, RM, 3, BKS>), g, b, 0, s, a, xb);
    else return FV_E_UNSUPPORTED;
  } else if (mode == 2) {
    if constexpr (KS == 2) hipLaunchKernelGGL((conv_fwd_v2<KS, WN, WM, RN, RM, 2, BKS>), g, b, 0, s, a, xb);
    else return FV_E_UNSUPPORTED;
  } else if (mode == 1) {
    if constexpr (KS == 3) hipLaunchKernelGGL((conv_fwd_v2<KS, WN, WM, RN, RM, 1, BKS>), g, b, 0, s, a, xb);
    else return FV_E_UNSUPPORTED;
  } else {
    if constexpr (KS != 2 && KS != 4) hipLaunchKernelGGL((conv_fwd_v2<KS, WN, WM, RN, RM, 0, BKS>), g, b, 0, s, a, xb);
    else return FV_E_UNSUPPORTED;
  }
  return FV_OK;
}

// 4-wave tiles stage 32-deep k slices when K is short (<= 640) or the input is upsampled:
// there the 4-blocks-per-CU occupancy beats the deeper k step (A/B on the FaceVAE shapes)
template <int KS, int WN, int WM, int RN, int RM>
int launch_v2_t(const ConvArgs& a, int mode, int nblk, unsigned xb, hipStream_t s) {
  if constexpr (WN * WM == 4) {
    if (a.W % 16 == 0 && (a.Kpad <= 640 || mode != 0))
      return launch_v2_b<KS, WN, WM, RN, RM, 32>(a, mode, nblk, xb, s);
  }
  return launch_v2_b<KS, WN, WM, RN, RM, 64>(a, mode, nblk, xb, s);
}

template <int KS>
int launch_v2_ks(const ConvArgs& a, FwdTile t, int mode, int nblk, unsigned xb, hipStream_t s) {
  const int ups = mode;
  if (t.bn == 128 && t.bm == 128) return launch_v2_t<KS, 2, 2, 4, 4>(a, ups, nblk, xb, s);
  if (t.bn == 64) return launch_v2_t<KS, 1, 4, 4, 4>(a, ups, nblk, xb, s);
  if (t.bn == 16) return launch_v2_t<KS, 1, 4, 1, 4>(a, ups, nblk, xb, s);
  if (t.bn == 256 && t.bm == 256) return launch_v2_t<KS, 4, 2, 4, 8>(a, ups, nblk, xb, s);
  if (t.bn == 128 && t.bm == 256) return launch_v2_t<KS, 2, 4, 4, 4>(a, ups, nblk, xb, s);
  if (t.bn == 256 && t.bm == 128) return launch_v2_t<KS, 4, 2, 4, 4>(a, ups, nblk, xb, s);
  return FV_E_UNSUPPORTED;
}

}  // namespace

int launch_v2(const ConvArgs& a, int ks, FwdTile t, int ups, int nblk, unsigned xb, hipStream_t s) {
  switch (ks) {
    case 2: return launch_v2_ks<2>(a, t, 2, nblk, xb, s);       // sub-pixel phases only
    case 4: return launch_v2_ks<4>(a, t, 3, nblk, xb, s);       // stride-2 low-res dgrad only
    case 1: return launch_v2_ks<1>(a, t, ups, nblk, xb, s);
    case 3: return launch_v2_ks<3>(a, t, ups, nblk, xb, s);
    case 7: return launch_v2_ks<7>(a, t, ups, nblk, xb, s);
  }
  return FV_E_UNSUPPORTED;
}
