// The halo-staged 3x3 forward kernels of the 2-D convolution, conv3_halo_fwd2 and
// conv3_halo_fwd3 (the res / down convs, their data gradients and the sub-pixel up convs), and
// their launchers (declared in conv_plan.h).  The launchers pick the instantiation and nothing
// else: planners, schedule and grid decisions and the entries are in conv.hip.
#include "conv_plan.h"

namespace {

// Diagnostic build only (build.py --diag -> libfacevae_diag.so, tools/convbench.py --diag):
// per-wave shader-clock stamps of the res conv kernel into a device table read back with
// fv_diag_read.  The production library compiles none of this.
#ifdef FV_DIAG
constexpr int DIAG_SLOTS = 8;
__device__ unsigned long long g_diag[4096 * 8 * DIAG_SLOTS];
#define FV_DIAG_T(var) const unsigned long long var = __builtin_amdgcn_s_memtime()
#define FV_DIAG_PUT(slot, val)                                                                     \
  do {                                                                                             \
    const unsigned long long v_ = (val);                                                           \
    if ((threadIdx.x & 63) == 0 && blockIdx.x < 4096)                                              \
      g_diag[((size_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * DIAG_SLOTS + (slot)] = v_; \
  } while (0)
// kernel entry / after the prologue barrier / around each main-loop wait + barrier / after
// the post-barrier issue block / after the main loop / at the end
#define FV_DIAG_BEGIN()                                                \
  FV_DIAG_T(d_t0);                                                     \
  const unsigned long long d_r0 = __builtin_amdgcn_s_memrealtime();    \
  unsigned long long d_tw = 0, d_ti = 0, d_wb = 0
#define FV_DIAG_PROLOGUE() FV_DIAG_T(d_t1)
#define FV_DIAG_WAIT_BEGIN() FV_DIAG_T(d_wa)
#define FV_DIAG_WAIT_END()                   \
  do {                                       \
    d_wb = __builtin_amdgcn_s_memtime();     \
    d_tw += d_wb - d_wa;                     \
  } while (0)
#define FV_DIAG_ISSUE_END() (d_ti += __builtin_amdgcn_s_memtime() - d_wb)
#define FV_DIAG_LOOP_END() FV_DIAG_T(d_t2)
#define FV_DIAG_END()                                                                       \
  do {                                                                                      \
    FV_DIAG_T(d_t3);                                                                        \
    unsigned xcc_;                                                                          \
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc_));                     \
    FV_DIAG_PUT(0, d_t0);                                                                   \
    FV_DIAG_PUT(1, d_t1);                                                                   \
    FV_DIAG_PUT(2, d_t2);                                                                   \
    FV_DIAG_PUT(3, d_t3);                                                                   \
    FV_DIAG_PUT(4, d_tw);                                                                   \
    FV_DIAG_PUT(5, d_ti);                                                                   \
    FV_DIAG_PUT(6, d_r0);                                                                   \
    FV_DIAG_PUT(7, ((unsigned long long)xcc_ << 32) | (unsigned)__builtin_amdgcn_s_memrealtime()); \
  } while (0)
#else
#define FV_DIAG_BEGIN()
#define FV_DIAG_PROLOGUE()
#define FV_DIAG_WAIT_BEGIN()
#define FV_DIAG_WAIT_END()
#define FV_DIAG_ISSUE_END()
#define FV_DIAG_LOOP_END()
#define FV_DIAG_END()
#endif

// ----------------------------------------------------------------------------------------
// 3x3 stride-1 conv with a halo-staged input (bf16 NHWC, cin % 64 == 0, W % 64 == 0):
// the res / down convs and their data gradients.  The per-tap DMA of conv_fwd_v2 moves 9
// copies of every input pixel into LDS; at 1 KB per ~30 CU-cycles that fill, not the MFMA,
// bounds the short-K layers (AFE.down1 forward: DMA alone 300 us of 530).  Here a block owns
// TR = 4 image rows x 64 columns; per 32-channel chunk the (TR+2) x 66 halo lands in LDS once
// and the 9 taps read their shifted windows from it, so a 32-deep k step moves the weight
// slice (BN x 64 B) plus 1/9 of a halo: 1.7x (BN 256) to 2.6x (BN 64) fewer bytes per MAC.
//   k step ks = (chunk c = ks / 9, tap t = ks % 9); weights [co][tap][ci] as in v2.
//   halo pixel hp = hr * 66 + hc at hp * 64 B, 16-B chunk XOR ((hp >> 2) & 1) * 2 (h3swz,
//   conv_common.h): a fragment read (16 consecutive halo pixels from ANY start) is
//   bank-conflict free (ds_read_b128 lane groups of the guide's table).
// ----------------------------------------------------------------------------------------
// wave-uniform count 0 .. 63 (gfx950's vmcnt range) -> the matching immediate
template <int N = 63>
__device__ __forceinline__ void wait_vm_upto(int n) {
  if constexpr (N == 0) {
    wait_vm<0>();
  } else {
    if (n >= N) wait_vm<N>();
    else wait_vm_upto<N - 1>(n);
  }
}

// Software-pipelined variant: a step is a PAIR of taps (64 k), the weight stage holds both
// taps' 32-channel slices, and the loop is conv_fwd_v2's: the fragments of the step's second
// tap are read while the first tap's MFMAs run and the barrier sits between the two MFMA
// groups.  Chunk c's halo goes into buffer c & 1 right after the barrier that retires the
// last read of chunk c - 2 (5 steps before its first use).  The weight stages form a ring of
// NSB buffers issued NSB - 1 steps ahead, so a DMA has NSB - 2 full steps to land.
template <int WN, int WM, int RN, int RM, int NSB>
__global__ void __launch_bounds__(64 * WN * WM, WN * RN * 16 >= 256 ? 1 : 2)
conv3_halo_fwd2(ConvArgs a, unsigned x_bytes) {
  constexpr int NW = WN * WM;
  constexpr int BN = WN * RN * 16, BM = WM * RM * 16, TR = BM / 64;
  constexpr int HP = (TR + 2) * 66, HQ = (HP + 15) / 16, JH = (HQ + NW - 1) / NW;
  constexpr int HALO = HQ * 1024;
  constexpr int QB = BN / 16, JB = QB / NW;
  static_assert(QB % NW == 0, "weight pieces per wave");
  constexpr int BST = BN * 64, STG = 2 * BST;
  constexpr int MAIN = 2 * HALO + NSB * STG, EPI = BM * BN * 2;
  __shared__ __attribute__((aligned(1024))) char smem[MAIN > EPI ? MAIN : EPI];

  FV_DIAG_BEGIN();
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
  const int lrow = lane >> 2, lchk = lane & 3;

  unsigned hoff[JH];
#pragma unroll
  for (int j = 0; j < JH; ++j) {
    const int hp = (wave + j * NW) * 16 + lrow;
    const int hr = hp / 66, hc = hp - (hp / 66) * 66;
    const int ih = th * TR + hr - 1, iw = tw * 64 + hc - 1;
    const bool ok = hp < HP && ih >= 0 && ih < a.H && iw >= 0 && iw < a.W;
    hoff[j] = ok ? (unsigned)(((((n * a.H + ih) * a.W + iw) << a.lgCin) + ((lchk ^ h3swz(hp)) << 3)) * 2) : 0x80000000u;
  }
  // stage-major weights (weight_prep_body smaj, as conv3_halo_fwd3): piece jb of tap unit u is
  // the contiguous KB at u * ustep + (co0 + (wave + jb * NW) * 16) * 64
  unsigned wbase[JB];
#pragma unroll
  for (int j = 0; j < JB; ++j) {
    const int row = (wave + j * NW) * 16 + lrow;
    wbase[j] = (unsigned)((co0 + row) * 64 + ((lchk ^ rswz<bf16>(row)) << 4));
  }
  const unsigned ustep = (unsigned)a.wus;
  const int nch = a.Cin >> 5, ntap = 9 * nch, nsteps = (ntap + 1) >> 1;
  auto issue_b = [&](int j, int buf) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int u = 2 * j + h;
      if (u < ntap) {
        const unsigned Bs = sbase + 2 * HALO + buf * STG + h * BST;
#pragma unroll
        for (int jb = 0; jb < JB; ++jb) dma16s(wr, Bs + (wave + jb * NW) * 1024, wbase[jb], (unsigned)u * ustep);
      }
    }
  };
  auto issue_halo = [&](int c) {
    const unsigned Hs = sbase + (c & 1) * HALO;
#pragma unroll
    for (int j = 0; j < JH; ++j)
      if (j < JH - 1 || wave + j * NW < HQ) dma16s(xr, Hs + (wave + j * NW) * 1024, hoff[j], (unsigned)(c * 64));
  };

  const int lr = lane & 15, lh = lane >> 4;
  int hpb[RM];
#pragma unroll
  for (int m = 0; m < RM; ++m) {
    const int loc = wm * RM * 16 + m * 16 + lr;
    hpb[m] = (loc >> 6) * 66 + (loc & 63);
  }
  auto load_frags = [&](Frag<bf16> (&fa)[RN], Frag<bf16> (&fb)[RM], int u, int buf) {
    const int c = u / 9, t = u - c * 9, r = t / 3, s3 = t - (t / 3) * 3;
    const char* Bs = smem + 2 * HALO + buf * STG + (u & 1) * BST;
    const char* Hs = smem + (c & 1) * HALO;
#pragma unroll
    for (int i = 0; i < RN; ++i) {
      const int row = wn * RN * 16 + i * 16 + lr;
      fa[i].lds(Bs + row * 64 + ((lh ^ rswz<bf16>(row)) << 4));
    }
#pragma unroll
    for (int m = 0; m < RM; ++m) {
      const int hp = hpb[m] + r * 66 + s3;
      fb[m].lds(Hs + hp * 64 + ((lh ^ h3swz(hp)) << 4));
    }
  };
  f32x4 acc[RN][RM];
#pragma unroll
  for (int i = 0; i < RN; ++i)
#pragma unroll
    for (int m = 0; m < RM; ++m) acc[i][m] = f32x4{0.f, 0.f, 0.f, 0.f};
  constexpr bool prio = true;
  auto mfma_all = [&](const Frag<bf16> (&fa)[RN], const Frag<bf16> (&fb)[RM]) {
    if (prio) __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int i = 0; i < RN; ++i)
#pragma unroll
      for (int m = 0; m < RM; ++m) acc[i][m] = mma(fa[i], fb[m], acc[i][m]);
    if (prio) __builtin_amdgcn_s_setprio(0);
  };

  Frag<bf16> fa0[RN], fb0[RM], fa1[RN], fb1[RM];
  auto bcnt = [&](int j) { return j < nsteps ? (2 * j + 1 < ntap ? 2 : 1) * JB : 0; };
  // ring of NSB weight stages: stage j in buffer j % NSB, issued NSB - 1 steps ahead; the
  // barrier of step j waits for stage j + 1 only (counted vmcnt: what this wave issued in
  // step j - 1 may stay in flight)
  issue_b(0, 0);
  issue_halo(0);
  if (nch > 1) issue_halo(1);
  for (int i = 1; i < NSB - 1; ++i)
    if (i < nsteps) issue_b(i, i);
  wait_vm<0>();
  __syncthreads();
  FV_DIAG_PROLOGUE();
  int pend = 0;                                 // DMAs this wave issued in the previous step
  if (NSB - 1 < nsteps) {
    issue_b(NSB - 1, NSB - 1);
    pend = bcnt(NSB - 1);
  }
  load_frags(fa0, fb0, 0, 0);
  int hn = 2, hstep = (9 * 2 - 10) / 2;         // next halo chunk and the step that issues it
  int bj = 0;                                   // buffer of stage j
  // No branch around the fragment reads: a read issued on one path only makes the compiler
  // drain ALL LDS reads (lgkmcnt(0)) before the next MFMA group, exposing the F1 read latency
  // every step.  An odd last tap re-reads a valid tap and skips its MFMAs.
  // The last step is peeled (its odd tap, if any, re-reads a valid tap and skips the MFMAs):
  // inside the loop its path (no barrier, no next-tap reads) merged into the loop's second
  // MFMA cluster and made the wait-count pass hold that cluster for the next tap's reads.
  for (int j = 0; j + 1 < nsteps; ++j) {
    load_frags(fa1, fb1, 2 * j + 1, bj);
    mfma_all(fa0, fb0);
    const int bn1 = bj + 1 == NSB ? 0 : bj + 1;
    // the weight stage is issued LAST in a step, so the count left in flight is that
    // stage's alone (a halo issued before it is waited for one step later)
    FV_DIAG_WAIT_BEGIN();
    if constexpr (NSB == 2) wait_vm<0>();     // stage j + 1 was the one issued last
    else if (pend == 2 * JB) wait_vm<2 * JB>();
    else wait_vm_dyn(pend);
    wait_lgkm0();
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    FV_DIAG_WAIT_END();
    if (hn < nch && j == hstep) {
      issue_halo(hn);
      ++hn;
      hstep = (9 * hn - 10) / 2;
    }
    pend = 0;
    if (j + NSB < nsteps) {
      issue_b(j + NSB, bj);
      pend = bcnt(j + NSB);
    }
    load_frags(fa0, fb0, 2 * j + 2, bn1);
    FV_DIAG_ISSUE_END();
    mfma_all(fa1, fb1);
    bj = bn1;
  }
  {
    const int j = nsteps - 1;
    const bool two = 2 * j + 1 < ntap;
    load_frags(fa1, fb1, two ? 2 * j + 1 : 2 * j, bj);
    mfma_all(fa0, fb0);
    if (two) mfma_all(fa1, fb1);
  }
  FV_DIAG_LOOP_END();
  __syncthreads();
  // (whole-row tiles that cover the output exactly, halo_epi_ok: the epilogue's HALO form)
  conv_epilogue<bf16, WN, WM, RN, RM, true, NoMid, false, true>(a, acc, smem, co0, p0, tm, wn, wm, lane, tid);
  FV_DIAG_END();
}

// Epilogue of conv3_halo_fwd3 MODE 1 (sub-pixel forward): tile columns are 4 phases x 64
// channels (wave column wn = phase (pa, pb)), rows the 256 low-res pixels (h0 + r, w0 + col).
// bias -> BN records -> bf16 through LDS -> 16-B stores to output pixel (2h + pa, 2w + pb).
// BN records: one per (tile, wave row, phase) = RM * 16 output pixels, record index
// ((tm * WM + wm) * 4 + wn) (stats_record_pixels: 128), so every output pixel is in one record.
template <int WM, int RM, typename Mid = NoMid>
__device__ __forceinline__ void subpix_epilogue(const ConvArgs& a, f32x4 (&acc)[4][RM], char* smem, int tn, int n,
                                                int h0, int w0, int tm, int wn, int wm, int lane, int tid,
                                                Mid mid = Mid{}) {
  constexpr bool kMid = !std::is_same<Mid, NoMid>::value;
  constexpr int RN = 4, NT = 64 * 4 * WM, BN = 256, BM = WM * RM * 16, CPR = BN / 8;
  const int lr = lane & 15, lh = lane >> 4;
  const int cb0 = tn * 64;
#pragma unroll
  for (int nn = 0; nn < RN; ++nn)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int co = cb0 + nn * 16 + lh * 4 + i;
      const float bv = a.bias ? a.bias[co] : 0.f;
#pragma unroll
      for (int m = 0; m < RM; ++m) acc[nn][m][i] += bv;
    }
  if (a.stats) {
    const int rec = (tm * WM + wm) * 4 + wn;
#pragma unroll
    for (int nn = 0; nn < RN; ++nn) {
      float sv[4], qv[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float t = 0.f, q = 0.f;
#pragma unroll
        for (int m = 0; m < RM; ++m) {
          t += acc[nn][m][i];
          q += acc[nn][m][i] * acc[nn][m][i];
        }
        sv[i] = row16_sum(t);
        qv[i] = row16_sum(q);
      }
      const int cb = cb0 + nn * 16 + lh * 4;
      const int ii = lr & 3;
      const float s01 = ii & 1 ? sv[1] : sv[0], s23 = ii & 1 ? sv[3] : sv[2];
      const float q01 = ii & 1 ? qv[1] : qv[0], q23 = ii & 1 ? qv[3] : qv[2];
      const float val = lr < 4 ? (ii & 2 ? s23 : s01) : (ii & 2 ? q23 : q01);
      if (lr < 8 && rec < a.nrec) a.stats[(long)(rec * 2 + (lr >> 2)) * a.Cout + cb + ii] = val;
    }
  }
  __syncthreads();
#pragma unroll
  for (int nn = 0; nn < RN; ++nn) {
    const int cl = wn * 64 + nn * 16 + lh * 4;
#pragma unroll
    for (int m = 0; m < RM; ++m) {
      const int pl = wm * RM * 16 + m * 16 + lr;
      bf16 t4[4] = {(bf16)acc[nn][m][0], (bf16)acc[nn][m][1], (bf16)acc[nn][m][2], (bf16)acc[nn][m][3]};
      char* dst = smem + pl * BN * 2 + (((cl >> 3) ^ (pl & (CPR - 1))) << 4) + ((cl & 4) << 1);
      *reinterpret_cast<uint2*>(dst) = *reinterpret_cast<const uint2*>(t4);
    }
  }
  __syncthreads();
  constexpr int NIT = BM * CPR / NT;
  static_assert(BM * CPR % NT == 0, "store pass");
  uint4 vv[kMid ? NIT : 1];
  if constexpr (kMid) {
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int idx = tid + it * NT;
      const int pl = idx / CPR, ch = idx - (idx / CPR) * CPR;
      vv[it] = *reinterpret_cast<const uint4*>(smem + pl * BN * 2 + ((ch ^ (pl & (CPR - 1))) << 4));
    }
    __syncthreads();
    mid();
  }
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int idx = tid + it * NT;
    const int pl = idx / CPR, ch = idx - (idx / CPR) * CPR;
    const int ph = ch >> 3, co = cb0 + (ch & 7) * 8;
    const int oh = 2 * (h0 + (pl >> 6)) + (ph >> 1), ow = 2 * (w0 + (pl & 63)) + (ph & 1);
    Chunk8<bf16> v;
    if constexpr (kMid) v.raw = vv[it];
    else v.raw = *reinterpret_cast<const uint4*>(smem + pl * BN * 2 + ((ch ^ (pl & (CPR - 1))) << 4));
    v.store(reinterpret_cast<bf16*>(a.y) + ((long)(n * a.Ho + oh) * a.Wo + ow) * a.ldy + co);
  }
}

// Linear-halo variant of conv3_halo_fwd2: every LDS fragment address is a per-lane base
// register plus an immediate.  In fwd2 the XOR swizzle of a 64-B halo pixel moves with the tap
// shift, so each of the 16 fragment reads of a step costs ~5 VALU (88 non-MFMA VALU per 64
// MFMAs): with two waves per SIMD that fills most of the vector issue slots the MFMAs leave.
// Here a halo pixel takes 96 B (64 B of channels + 32 B zero-filled by out-of-range DMA
// slots): 16 consecutive pixels read by ds_read_b128 from ANY start are conflict-free, and the
// address of pixel hp shifted by a tap is linear: a tap adds one wave-uniform offset to a
// per-lane base and the fragments of the step are immediate offsets from it (measured in the
// asm: 4 non-MFMA VALU per 64-MFMA step against 88).  LDS: [NSB weight stages][2 halo buffers].
//
// SCH (schedule of the two waves of a SIMD, waves w and w + NW / 2): bit 0 = one static
// s_setprio 1 for waves NW/2 .. NW-1 before the main loop instead of prio flips around every
// MFMA cluster; bit 1 = stagger: waves NW/2 .. NW-1 pass each step's barrier before the MFMAs
// of the tap whose fragments they hold, so they run those MFMAs while their partners issue the
// DMA and fragment reads after the barrier, and issue their own reads while the partners run
// MFMAs (same arithmetic, same order per accumulator: bit-identical).
//
// MODE (UpBlock2D's nearest-x2 upsample + 3x3 conv, modules.py:78-89, on this kernel's halo
// structure; the sub-pixel algebra of conv_fwd_v2 MODE 2 / 3):
//   1 = sub-pixel forward over the LOW-res input: the 256-row co tile is 4 phases (pa, pb) x 64
//       channels, wave column wn = phase; a 32-channel chunk has 4 tap units q = (rr, ss), the
//       phase's 2x2 folded taps, which read the halo window tap (pa + rr, pb + ss); the
//       epilogue stores phase wn of low-res pixel (h, w) to output pixel (2h + pa, 2w + pb).
//   2 = data gradient at the LOW resolution: dy viewed as 4 phase planes (py, px) of the low-res
//       grid, the conv input = [plane][Cout] channels (a.Cin = 4 Cout, a.K = dy's channel stride,
//       a.Hin x a.Win = dy's size); a chunk lies in one plane and its 4 units are the plane's 2x2
//       taps at window (1 - py + a, 1 - px + b); the halo DMA gathers plane pixels (2ih + py,
//       2iw + px) -- the stride-2 4x4 conv of conv_fwd_v2 MODE 3 without its 12 zero taps.
// Weights (weight_prep_phase_kernel): unit u = chunk * 4 + q, [rows][32] per unit.
//
// PERS (persistent, one block per CU): the block walks the tiles v = blockIdx.x + k * gridDim.x
// (the tiles its XCD runs in the one-tile-per-block grid of ntiles blocks).  After a tile's
// epilogue staged its output in LDS and read it back into registers, the next tile's
// prologue DMA (weight stage 0, halo chunks 0 / 1) is issued and THEN the stores: every CU
// reaches its epilogue at the same time, so a tile's 128 KB of stores (HBM-bound as a burst)
// drain under the next tile's prologue instead of after it.
template <int WN, int WM, int RN, int RM, int NSB, int SCH = 0, int MODE = 0, bool PERS = false>
__global__ void __launch_bounds__(64 * WN * WM, (WN * RN * 16 >= 256 || WN == 1) ? 1 : 2)
conv3_halo_fwd3(ConvArgs a, unsigned x_bytes, int ntiles) {
  static_assert(MODE != 1 || (WN == 4 && RN == 4), "sub-pixel forward: one phase of 64 channels per wave column");
  constexpr int UPC = MODE ? 4 : 9;                        // tap units per 32-channel chunk
  constexpr int NW = WN * WM;
  constexpr int BN = WN * RN * 16, BM = WM * RM * 16, TR = BM / 64;
  static_assert(RM % 4 == 0, "a wave's pixels start on an image-row boundary of the tile");
  constexpr int PXB = 96;                                  // LDS bytes per halo pixel
  constexpr int HP = (TR + 2) * 66, HSL = HP * (PXB / 16), HQ = (HSL + 63) / 64, JH = (HQ + NW - 1) / NW;
  constexpr int HALO = HQ * 1024;
  // weight DMA pieces (16 rows) per tap: JB per wave, or one per wave for waves < QB when the
  // co tile has fewer pieces than waves (the 64-channel tile on 8 waves)
  constexpr int QB = BN / 16, JB = QB >= NW ? QB / NW : 1;
  static_assert(QB % NW == 0 || NW % QB == 0, "weight pieces per wave");
  constexpr int BST = BN * 64, STG = 2 * BST, WOFF = NSB * STG;
  constexpr int MAIN = WOFF + 2 * HALO, EPI = BM * BN * 2;
  static_assert(MAIN <= 163840, "LDS");
  static_assert(STG * (NSB - 1) + BST + (BN - 16) * 64 < 65536, "weight fragment immediates");
  __shared__ __attribute__((aligned(1024))) char smem[MAIN > EPI ? MAIN : EPI];

  FV_DIAG_BEGIN();
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wn = wave % WN, wm = wave / WN;
  const int ntl = PERS ? ntiles : (int)gridDim.x;
  // tile of launch index v: the XCD-aware bijective remap (consecutive tiles on one XCD)
  auto remap = [&](int v) {
    const int q8 = ntl / 8, r8 = ntl % 8, x8 = v % 8;
    return (x8 < r8 ? x8 * (q8 + 1) : r8 * (q8 + 1) + (x8 - r8) * q8) + v / 8;
  };
  const int tiles_w = a.W >> 6, tiles_h = a.H / TR;
  const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.x), 0, (int)x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.w), 0, 0x7fffffff, 0x00020000);
  const unsigned sbase = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(lds_ptr_t)smem);
  const int lrow = lane >> 2, lchk = lane & 3;
  // Weights are stage-major (weight_prep_body smaj): tap unit u = c * 9 + t is a [Cout][32]
  // block, so the 16 rows of a DMA piece are one contiguous KB (8 whole 128-B lines; the
  // [co][Kpad] rows made every piece 16 separate 64-B segments).  Piece jb of unit u starts at
  // u * ustep + (co0 + (wave + jb * NW) * 16) * 64; the lane's source chunk carries the LDS
  // chunk swizzle.
  const unsigned wstep = (unsigned)(NW * 16 * 64);
  const unsigned ustep = (unsigned)a.wus;
  const int nch = a.Cin >> 5, nsteps = UPC * nch / 2;
  const int cpp = a.Cin >> 7;                               // MODE 2: chunks per phase plane

  struct Tile {
    int tn, tm, tw, th, n, co0, p0;
    unsigned wbase;
  };
  auto tile_of = [&](int v) {
    Tile t;
    const int lid = remap(v);
    t.tn = lid % a.ntn;
    t.tm = lid / a.ntn;
    t.tw = t.tm % tiles_w;
    t.th = (t.tm / tiles_w) % tiles_h;
    t.n = t.tm / (tiles_w * tiles_h);
    t.co0 = t.tn * BN;
    t.p0 = (t.n * a.H + t.th * TR) * a.W + t.tw * 64;
    t.wbase = (unsigned)((t.co0 + wave * 16 + lrow) * 64 + ((lchk ^ rswz<bf16>(lrow)) << 4));
    return t;
  };
  // halo slots of this wave: slot k = 16-B chunk k % 6 of halo pixel k / 6 (chunks 4, 5 pad)
  unsigned hoff[JH];
  auto mk_hoff = [&](const Tile& t) {
#pragma unroll
    for (int j = 0; j < JH; ++j) {
      const int k = (wave + j * NW) * 64 + lane;
      const int hp = k / 6, ch = k - (k / 6) * 6;
      const int hr = hp / 66, hc = hp - (hp / 66) * 66;
      const int ih = t.th * TR + hr - 1, iw = t.tw * 64 + hc - 1;
      const bool ok = hp < HP && ch < 4 && ih >= 0 && ih < a.H && iw >= 0 && iw < a.W;
      if constexpr (MODE == 2)     // plane (0, 0) pixel of dy; the chunk's plane is a uniform offset
        hoff[j] = ok ? (unsigned)((((t.n * a.Hin + 2 * ih) * a.Win + 2 * iw) * a.K + (ch << 3)) * 2) : 0x80000000u;
      else
        hoff[j] = ok ? (unsigned)(((((t.n * a.H + ih) * a.W + iw) << a.lgCin) + (ch << 3)) * 2) : 0x80000000u;
    }
  };
  auto issue_b = [&](unsigned wbase, int j, int buf) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int u = 2 * j + h;
      const unsigned Bs = sbase + buf * STG + h * BST;
#pragma unroll
      for (int jb = 0; jb < JB; ++jb)
        if (QB >= NW || wave < QB) dma16s(wr, Bs + (wave + jb * NW) * 1024, wbase, (unsigned)u * ustep + jb * wstep);
    }
  };
  // the step after whose barrier halo chunk c is issued: the last read of chunk c - 2 (same
  // buffer) was retired by it
  auto halo_step = [&](int c) { return MODE ? 2 * c - 3 : (9 * c - 10) / 2; };
  auto halo_soff = [&](int c) -> unsigned {
    if constexpr (MODE == 2) {
      const int pl = c / cpp, cc = c - pl * cpp;
      return (unsigned)((((pl >> 1) * a.Win + (pl & 1)) * a.K + cc * 32) * 2);
    } else {
      return (unsigned)(c * 64);
    }
  };
  auto issue_halo = [&](int c) {
    const unsigned Hs = sbase + WOFF + (c & 1) * HALO;
#pragma unroll
    for (int j = 0; j < JH; ++j)
      if (j < JH - 1 || wave + j * NW < HQ) dma16s(xr, Hs + (wave + j * NW) * 1024, hoff[j], halo_soff(c));
  };
  auto bcnt = [&](int j) { return j < nsteps && (QB >= NW || wave < QB) ? 2 * JB : 0; };
  // a tile's prologue DMA: weight stage 0, halo chunks 0 / 1, stages 1 .. NSB - 2
  auto issue_prologue = [&](const Tile& t) {
    issue_b(t.wbase, 0, 0);
    issue_halo(0);
    issue_halo(1);
    for (int i = 1; i < NSB - 1; ++i)
      if (i < nsteps) issue_b(t.wbase, i, i);
  };

  const int lr = lane & 15, lh = lane >> 4;
  // per-lane bases: weight row wn*RN*16 + lr (chunk swizzle is a function of lr only), halo
  // pixel of tile pixel wm*RM*16 + lr (RM*16 is a multiple of the 64-pixel tile row).  A tap
  // adds one wave-uniform offset to each (2 VALU per tap); the fragments are immediates.
  const int va = (wn * RN * 16 + lr) * 64 + ((lh ^ rswz<bf16>(lr)) << 4);
  const int vb = WOFF + ((wm * RM / 4) * 66 + lr) * PXB + lh * 16;
  auto load_frags = [&](Frag<bf16> (&fa)[RN], Frag<bf16> (&fb)[RM], int u, int buf) {
    int c, r, s3;
    if constexpr (MODE == 1) {
      c = u >> 2;
      r = (wn >> 1) + ((u >> 1) & 1);
      s3 = (wn & 1) + (u & 1);
    } else if constexpr (MODE == 2) {
      c = u >> 2;
      const int pl = c / cpp;
      r = ((u >> 1) & 1) + 1 - (pl >> 1);
      s3 = (u & 1) + 1 - (pl & 1);
    } else {
      c = u / 9;
      const int t = u - c * 9;
      r = t / 3;
      s3 = t - (t / 3) * 3;
    }
    const int pa = va + (buf * STG + (u & 1) * BST);
    const int pb = vb + ((c & 1) * HALO + (r * 66 + s3) * PXB);
#pragma unroll
    for (int i = 0; i < RN; ++i) fa[i].lds(smem + pa + i * 1024);
#pragma unroll
    for (int m = 0; m < RM; ++m) fb[m].lds(smem + pb + (((m * 16) >> 6) * 66 + ((m * 16) & 63)) * PXB);
  };
  const bool hi = wave >= NW / 2;                  // the second-dispatched wave of each SIMD
  const bool stag = (SCH & 2) && hi;

  int v = blockIdx.x;
  Tile t = tile_of(v);
  mk_hoff(t);
  issue_prologue(t);
  bool first = true;
  for (;;) {
    // the first reads need weight stage 0 and halo chunk 0 only: on the first tile the DMAs
    // issued after them (chunk 1, first read at unit UPC; stages 1 .. NSB - 2) stay in flight
    // past the prologue barrier and are waited for at the first step barriers; a later tile's
    // prologue was issued before the previous tile's stores, so all is waited for
    {
      const int nh1 = (JH - 1) + ((JH - 1) * NW + wave < HQ ? 1 : 0);
      int later = nh1;
      for (int i = 1; i < NSB - 1; ++i) later += bcnt(i);
      // a later tile: the previous epilogue's stores were issued after this prologue (vmcnt
      // retires in issue order on gfx9), so they may stay in flight too: NRES (+ 4 record
      // stores with store-pass records) per wave
      if (!first) later += BM * BN / (8 * NW * 64) + (MODE != 1 && a.spm ? 4 : 0);
      wait_vm_upto(later);
    }
    __syncthreads();
    FV_DIAG_PROLOGUE();
    f32x4 acc[RN][RM];
#pragma unroll
    for (int i = 0; i < RN; ++i)
#pragma unroll
      for (int m = 0; m < RM; ++m) acc[i][m] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto mfma_all = [&](const Frag<bf16> (&fa)[RN], const Frag<bf16> (&fb)[RM]) {
      if constexpr (!(SCH & 1)) __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int i = 0; i < RN; ++i)
#pragma unroll
        for (int m = 0; m < RM; ++m) acc[i][m] = mma(fa[i], fb[m], acc[i][m]);
      if constexpr (!(SCH & 1)) __builtin_amdgcn_s_setprio(0);
    };

    // the ring and halo schedule of conv3_halo_fwd2 (nch even: no odd last tap)
    Frag<bf16> fa0[RN], fb0[RM], fa1[RN], fb1[RM];
    int pend = 0;
    if (NSB - 1 < nsteps) {
      issue_b(t.wbase, NSB - 1, NSB - 1);
      pend = bcnt(NSB - 1);
    }
    load_frags(fa0, fb0, 0, 0);
    int hn = 2, hstep = halo_step(2);
    int bj = 0;
    if constexpr (SCH & 1) {
      if (hi) __builtin_amdgcn_s_setprio(1);
    }
    // barrier of step j: stage j + 1 landed (own DMAs counted, then the barrier publishes them),
    // and every wave's reads of stage j are done (its buffer is re-filled right after)
    auto step_barrier = [&]() {
      FV_DIAG_WAIT_BEGIN();
      if constexpr (NSB == 2) wait_vm<0>();
      else if (pend == 2 * JB) wait_vm<2 * JB>();
      else wait_vm_dyn(pend);
      wait_lgkm0();
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      FV_DIAG_WAIT_END();
    };
    // stagger (SCH bit 1): waves NW/2.. take the barrier BEFORE the MFMAs of tap 2j (their
    // fragments are in registers), the others after; every read still falls in the same barrier
    // interval as in the lockstep order, so the ring / halo hazards are unchanged.
    // The last step is peeled: with it inside the loop (no barrier, no next-tap reads) the
    // wait-count pass merged its state into the loop's second MFMA cluster and made that
    // cluster wait for the next tap's fragment reads every step (lgkmcnt(7) .. (0)).
    for (int j = 0; j + 1 < nsteps; ++j) {
      load_frags(fa1, fb1, 2 * j + 1, bj);
      if constexpr ((SCH & 2) != 0) {
        if (stag) step_barrier();
      }
      mfma_all(fa0, fb0);
      const int bn1 = bj + 1 == NSB ? 0 : bj + 1;
      if (!stag) step_barrier();
      if (hn < nch && j == hstep) {
        issue_halo(hn);
        ++hn;
        hstep = halo_step(hn);
      }
      pend = 0;
      if (j + NSB < nsteps) {
        issue_b(t.wbase, j + NSB, bj);
        pend = bcnt(j + NSB);
      }
      load_frags(fa0, fb0, 2 * j + 2, bn1);
      FV_DIAG_ISSUE_END();
      mfma_all(fa1, fb1);
      bj = bn1;
    }
    load_frags(fa1, fb1, 2 * nsteps - 1, bj);
    mfma_all(fa0, fb0);
    mfma_all(fa1, fb1);
    if constexpr (SCH & 1) __builtin_amdgcn_s_setprio(0);
    FV_DIAG_LOOP_END();
    __syncthreads();
    const int vn = v + (int)gridDim.x;
    const bool nxt = PERS && vn < ntl;
    const Tile cur = t;
    if constexpr (PERS) {
      // the next tile's geometry and prologue DMA, issued between the epilogue's LDS read-back
      // and its stores (conv_epilogue / subpix_epilogue `mid`)
      auto mid = [&]() {
        if (nxt) {
          t = tile_of(vn);
          mk_hoff(t);
          issue_prologue(t);
        }
      };
      if constexpr (MODE == 1)
        subpix_epilogue<WM, RM>(a, acc, smem, cur.tn, cur.n, cur.th * TR, cur.tw * 64, cur.tm, wn, wm, lane, tid, mid);
      else
        conv_epilogue<bf16, WN, WM, RN, RM, true, decltype(mid), false, true>(a, acc, smem, cur.co0, cur.p0, cur.tm, wn, wm,
                                                                              lane, tid, mid);
    } else {
      if constexpr (MODE == 1)
        subpix_epilogue<WM, RM>(a, acc, smem, cur.tn, cur.n, cur.th * TR, cur.tw * 64, cur.tm, wn, wm, lane, tid);
      else
        conv_epilogue<bf16, WN, WM, RN, RM, true, NoMid, false, true>(a, acc, smem, cur.co0, cur.p0, cur.tm, wn, wm, lane, tid);
    }
    FV_DIAG_END();
    if (!nxt) break;
    v = vn;
    first = false;
  }
}


// conv3_halo_fwd3 of one parameter set and MODE: the schedule and, below the 256-channel co tile
// (its persistent form spills, see launch_h3 in conv.hip), the persistent form
template <int WN, int WM, int RN, int RM, int NSB, int MODE>
int launch_fwd3_t(const ConvArgs& a, int sch, bool pers, int grid, unsigned xb, int ntiles, hipStream_t s) {
  const dim3 g(grid), b(64 * WN * WM);
  if (sch != 0 && sch != 2) return FV_E_UNSUPPORTED;
  if (pers) {
    if constexpr (WN * RN * 16 < 256) {
      if (sch == 2) hipLaunchKernelGGL((conv3_halo_fwd3<WN, WM, RN, RM, NSB, 2, MODE, true>), g, b, 0, s, a, xb, ntiles);
      else hipLaunchKernelGGL((conv3_halo_fwd3<WN, WM, RN, RM, NSB, 0, MODE, true>), g, b, 0, s, a, xb, ntiles);
      return FV_OK;
    }
    return FV_E_UNSUPPORTED;
  }
  if (sch == 2) hipLaunchKernelGGL((conv3_halo_fwd3<WN, WM, RN, RM, NSB, 2, MODE, false>), g, b, 0, s, a, xb, ntiles);
  else hipLaunchKernelGGL((conv3_halo_fwd3<WN, WM, RN, RM, NSB, 0, MODE, false>), g, b, 0, s, a, xb, ntiles);
  return FV_OK;
}

}  // namespace

// bn: the co tile, 256 / 128 on 4 rows x 64 px, 64 on 8 rows x 64 px.  mode: 0 plain, 1 sub-pixel
// forward, 2 stride-2 data gradient by phases (conv3_halo_fwd3's MODE)
int launch_halo3_fwd3(const ConvArgs& a, int bn, int mode, int sch, bool pers, int grid, unsigned xb, int ntiles,
                      hipStream_t s) {
  if (bn == 256) {
    if (mode == 0) return launch_fwd3_t<4, 2, 4, 8, 2, 0>(a, sch, pers, grid, xb, ntiles, s);
    if (mode == 1) return launch_fwd3_t<4, 2, 4, 8, 2, 1>(a, sch, pers, grid, xb, ntiles, s);
    if (mode == 2) return launch_fwd3_t<4, 2, 4, 8, 2, 2>(a, sch, pers, grid, xb, ntiles, s);
  } else if (bn == 128) {
    if (mode == 0) return launch_fwd3_t<2, 4, 4, 4, 3, 0>(a, sch, pers, grid, xb, ntiles, s);
    if (mode == 2) return launch_fwd3_t<2, 4, 4, 4, 3, 2>(a, sch, pers, grid, xb, ntiles, s);
  } else if (bn == 64) {
    if (mode == 0) return launch_fwd3_t<1, 8, 4, 4, 2, 0>(a, sch, pers, grid, xb, ntiles, s);
  }
  return FV_E_UNSUPPORTED;
}

// bn: the co tile (4 rows x 64 px), 256 / 128 on 8 waves, 64 on 4
int launch_halo3_fwd2(const ConvArgs& a, int bn, int nblk, unsigned xb, hipStream_t s) {
  if (bn == 256) hipLaunchKernelGGL((conv3_halo_fwd2<4, 2, 4, 8, 2>), dim3(nblk), dim3(512), 0, s, a, xb);
  else if (bn == 128) hipLaunchKernelGGL((conv3_halo_fwd2<2, 4, 4, 4, 3>), dim3(nblk), dim3(512), 0, s, a, xb);
  else if (bn == 64) hipLaunchKernelGGL((conv3_halo_fwd2<1, 4, 4, 4, 3>), dim3(nblk), dim3(256), 0, s, a, xb);
  else return FV_E_UNSUPPORTED;
  return FV_OK;
}

#ifdef FV_DIAG
extern "C" {
// diagnostic build: copy the stamp table (g_diag) to the host
int fv_diag_read(unsigned long long* host, int n) {
  const int cap = (int)(sizeof(g_diag) / sizeof(g_diag[0]));
  if (n > cap) n = cap;
  if (hipDeviceSynchronize() != hipSuccess) return 1;
  return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_diag), (size_t)n * sizeof(unsigned long long)) == hipSuccess ? 0 : 1;
}
int fv_diag_clear(void) {
  void* p = nullptr;
  if (hipGetSymbolAddress(&p, HIP_SYMBOL(g_diag)) != hipSuccess) return 1;
  return hipMemset(p, 0, sizeof(g_diag)) == hipSuccess ? 0 : 1;
}
}  // extern "C"
#endif
