// The special-shape forward kernels of the 2-D convolution -- conv_halo_fwd (7x7, small channel
// side), conv7c4_fwd, conv3c64_fwd, conv3up_band_fwd, conv1x1_stream, conv7_n3_fwd2 -- and one
// launcher per kernel (declared in conv_plan.h, with the tile constants the planners read).
// Which conv takes which kernel, the grids and every argument check: conv_run() in conv.hip.
#include "conv_plan.h"

namespace {

// ----------------------------------------------------------------------------------------
// Halo-tiled 7x7 forward for a small channel side (bf16): AFE.in_conv 3->64 forward,
// Generator.out_conv 64->3 forward and its 3->64 backward-data.  The block's TR x 64 output
// pixels plus the (KS-1)-pixel halo of the input are staged in LDS ONCE (DMA, per-lane
// source addressing, zero border from the buffer range check); every tap then reads its
// shifted window from LDS, instead of the 49x im2col re-read of the generic path.
//   A fragment (16 pixels x 32 k): lane (i, g) reads the 16-B chunk g of k-step ks at halo
//   pixel (pixel i + tap offset) -> one ds_read_b128; 16-B chunks inside a pixel are XOR-
//   swizzled by the pixel index (conflict-light reads of 128-B pixels).
//   B fragment (weights [co][Kpad]): from LDS with padded rows (WLDS) or straight from
//   global/L1 (3 output channels: 16 padded rows, 100 KB, cache-resident).
// 8 waves; wave w owns pixels [w*RM*16, (w+1)*RM*16) of the tile and all RN*16 channels.
// Requires W % 64 == 0 and H % TR == 0 (host checks).
// ----------------------------------------------------------------------------------------
template <int KS, int CIN, int RN, int TR, bool WLDS, bool KSPLIT>
__global__ void __launch_bounds__(512, 4)
conv_halo_fwd(ConvArgs a, unsigned x_bytes) {
  constexpr int PAD = KS / 2, TW = 64;
  constexpr int MT = TR * 4;                       // 16-pixel m-tiles per block
  // KSPLIT: every wave owns all MT m-tiles and 1/8 of the k-steps (partials summed in LDS);
  // otherwise wave w owns m-tiles [w*RM, (w+1)*RM) and all k-steps.
  constexpr int RM = KSPLIT ? MT : MT / 8;
  constexpr int HR = TR + KS - 1, HW = TW + KS - 1;
  constexpr int CPP = CIN / 8;                     // 16-B chunks per pixel
  constexpr int HCH = HR * HW * CPP;               // halo chunks
  constexpr int HQ = (HCH + 63) / 64;              // 1-KB pieces
  constexpr int KPAD = ((KS * KS * CIN + 31) / 32) * 32;
  constexpr int NKS = KPAD / 32;
  constexpr int KPW = (NKS + 7) / 8;               // k-steps per wave (KSPLIT)
  constexpr int WROW = KPAD / 8 + 1;               // padded weight row (16-B chunks)
  constexpr int WCH = RN * 16 * WROW;
  constexpr int WQ = WLDS ? (WCH + 63) / 64 : 0;
  constexpr int HB = HQ * 1024, WB = WQ * 1024;
  constexpr int SCR = 4096;                        // epilogue scratch (BN partials)
  static_assert(!KSPLIT || (RN == 1 && !WLDS && 8 * MT * 1024 <= HB), "k-split layout");
  __shared__ __attribute__((aligned(1024))) char smem[HB + WB + SCR];
  char* halo = smem;
  char* wlds = smem + HB;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tiles_w = a.W / TW, tiles_h = a.H / TR;
  const int tile = blockIdx.x;
  const int n = tile / (tiles_h * tiles_w);
  const int rem = tile - n * tiles_h * tiles_w;
  const int h0 = (rem / tiles_w) * TR, w0 = (rem % tiles_w) * TW;
  const int li = lane & 15, g = lane >> 4;
  const bf16* __restrict__ wk = reinterpret_cast<const bf16*>(a.w);

  const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.x), 0, (int)x_bytes, 0x00020000);
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
  if constexpr (WLDS) {
    const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.w), 0, 0x7fffffff, 0x00020000);
    for (int q = wave; q < WQ; q += 8) {
      const int L = q * 64 + lane;
      const int row = L / WROW, ch = L - (L / WROW) * WROW;
      const bool ok = L < WCH && ch < KPAD / 8;
      const unsigned off = ok ? (unsigned)((row * a.Kpad + ch * 8) * 2) : 0x80000000u;
      dma16(wr, wlds + q * 1024, off);
    }
  }
  const int ks0 = KSPLIT ? wave * KPW : 0;
  const int ks1 = KSPLIT ? min(NKS, ks0 + KPW) : NKS;
  bf16x8 bpre[KSPLIT ? KPW : 1];
  if constexpr (KSPLIT) {   // this wave's weight fragments, straight to registers
#pragma unroll
    for (int j = 0; j < KPW; ++j) {
      const int kc = (ks0 + j) * 4 + g;
      bpre[j] = (ks0 + j < NKS) ? *reinterpret_cast<const bf16x8*>(wk + (long)li * a.Kpad + kc * 8) : bf16x8{};
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  f32x4 acc[RN][RM];
#pragma unroll
  for (int i = 0; i < RN; ++i)
#pragma unroll
    for (int j = 0; j < RM; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  int hbase[RM];   // halo pixel of this lane's output pixel, per m-tile (tap (0,0))
#pragma unroll
  for (int m = 0; m < RM; ++m) {
    const int loc = (KSPLIT ? 0 : wave * RM * 16) + m * 16 + li;
    hbase[m] = (loc / TW) * HW + (loc % TW);
  }
  auto kstep = [&](int ks, const bf16x8 (&bfr)[RN]) {
    const int kc = ks * 4 + g;                 // this lane's 16-B k chunk
    const int tap = kc / CPP, ch = kc - (kc / CPP) * CPP;
    const bool kin = tap < KS * KS;
    const int r = tap / KS, s = tap - (tap / KS) * KS;
    const int toff = r * HW + s;
    bf16x8 afr[RM];
#pragma unroll
    for (int m = 0; m < RM; ++m) {
      const int hp = hbase[m] + toff;
      bf16x8 v = *reinterpret_cast<const bf16x8*>(halo + (hp * CPP + (ch ^ (hp & (CPP - 1)))) * 16);
      if (!kin) v = bf16x8{};
      afr[m] = v;
    }
#pragma unroll
    for (int nn = 0; nn < RN; ++nn)
#pragma unroll
      for (int m = 0; m < RM; ++m) acc[nn][m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[nn], afr[m], acc[nn][m], 0, 0, 0);
  };
  if constexpr (KSPLIT) {
#pragma unroll
    for (int j = 0; j < KPW; ++j) {
      if (ks0 + j < ks1) {
        const bf16x8 bfr[RN] = {bpre[j]};
        kstep(ks0 + j, bfr);
      }
    }
  } else {
#pragma unroll 2
    for (int ks = ks0; ks < ks1; ++ks) {
      const int kc = ks * 4 + g;
      bf16x8 bfr[RN];
#pragma unroll
      for (int nn = 0; nn < RN; ++nn) {
        if constexpr (WLDS) bfr[nn] = *reinterpret_cast<const bf16x8*>(wlds + ((nn * 16 + li) * WROW + kc) * 16);
        else bfr[nn] = *reinterpret_cast<const bf16x8*>(wk + (long)(nn * 16 + li) * a.Kpad + kc * 8);
      }
      kstep(ks, bfr);
    }
  }
  const int p0 = (n * a.H + h0) * a.W + w0;
  if constexpr (KSPLIT) {
    // sum the 8 waves' partial tiles through LDS (halo no longer needed); wave w finishes m-tile w
    __syncthreads();
    f32x4* red = reinterpret_cast<f32x4*>(halo);
#pragma unroll
    for (int m = 0; m < RM; ++m) red[(wave * RM + m) * 64 + lane] = acc[0][m];
    __syncthreads();
    f32x4 t[1][1];
    t[0][0] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int w = 0; w < 8; ++w) t[0][0] += red[(w * RM + wave) * 64 + lane];
    conv_epilogue<bf16, 1, 8, 1, 1>(a, t, smem + HB + WB, 0, p0, tile, 0, wave, lane, tid);
  } else {
    conv_epilogue<bf16, 1, 8, RN, RM>(a, acc, smem + HB + WB, 0, p0, tile, 0, wave, lane, tid);
  }
}

// ----------------------------------------------------------------------------------------
// conv7c4_fwd: 7x7, <= 4 valid input channels (stored as 8) -> 64 output channels:
// AFE.in_conv 3 -> 64 forward (models.py:932) and Generator.out_conv's data gradient (3 -> 64).
// conv_halo_fwd<7, 8, ...> pads K to 49 taps x 8 channels = 416 (62 % zeros) and restages the
// 54 KB weight image in every one of its 8192 blocks (the LDS-DMA of the weights, not the
// MFMAs, set its 153-191 us).  Here:
//  * K packs 2 taps x 4 channels per 16-B fragment chunk: k = r * 32 + s * 4 + ci (s = 7 and
//    ci >= cin_valid are zero weights), K = 7 x 32 = 224 -> 7 MFMA k-steps instead of 13; the
//    A fragment of lane (pixel i, chunk g) is halo pixels (i + 2g, i + 2g + 1) of row r, 8 B
//    each (two ds_read_b64 from the 16-B NHWC pixels);
//  * persistent blocks (2 per CU): the 64 x 224 weight image is staged ONCE per block, the
//    halos of the next two tiles are in flight (3-buffer ring) while the current one computes;
//  * a minimal epilogue (bias preloaded, NHWC bf16 stores widened to 16 B), so no load in the
//    loop waits behind the halo DMA; ONE BN (sum, sum^2) record per BLOCK (r6): every lane
//    keeps the running sums of its 16 channels over all the block's tiles (plain adds), reduced
//    across lanes and waves once at the end -- the per-tile record (32 DPP row sums per wave
//    and tile, an LDS exchange and a record store) made the in_conv forward 27 us slower than
//    the same kernel without statistics (104 vs 77 us in the replayed step).  Block b owns tiles
//    b, b + G, ... (C74 tiles per block, c74_grid), so record b covers exactly those pixels.
// Tile: 4 rows x 64 columns x 64 co; wave w owns pixels [32w, 32w + 32) x all 64 co.
// ----------------------------------------------------------------------------------------
// (C74_TR and C74_K: conv_plan.h)
constexpr int C74_HW = 71, C74_HR = C74_TR + 6;                      // halo row: 64 + 6 + 1 (zero) px
constexpr int C74_WCOL = C74_K / 8;                                  // 16-B chunks (k columns) per weight row
constexpr int C74_WQ = 64 * C74_WCOL / 64;                           // 1-KB weight pieces (28)
constexpr int C74_HQ = (C74_HR * C74_HW + 63) / 64;                  // 1-KB halo pieces (16 B / px)
__global__ void __launch_bounds__(512, 2)
conv7c4_fwd(ConvArgs a, unsigned x_bytes, int ntiles) {
  constexpr int WB = C74_WQ * 1024, HB = C74_HQ * 1024, NHB = 3;   // 3-deep halo ring
  __shared__ __attribute__((aligned(1024))) char smem[WB + NHB * HB];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, g = lane >> 4;
  const int tiles_w = a.W >> 6, tiles_h = a.H / C74_TR;
  const unsigned sbase = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(lds_ptr_t)smem);
  const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.x), 0, (int)x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.w), 0, 0x7fffffff, 0x00020000);

  // halo pieces of this wave (pixel L = q * 64 + lane of the 10 x 71 halo, 16 B each)
  auto issue_halo = [&](int tile, int buf) {
    const int n = tile / (tiles_h * tiles_w), rem = tile - n * tiles_h * tiles_w;
    const int h0 = (rem / tiles_w) * C74_TR, w0 = (rem % tiles_w) * 64;
    for (int q = wave; q < C74_HQ; q += 8) {
      const int L = q * 64 + lane;
      const int hr = L / C74_HW, hc = L - (L / C74_HW) * C74_HW;
      const int hh = h0 + hr - 3, ww = w0 + hc - 3;
      const bool ok = L < C74_HR * C74_HW && hh >= 0 && hh < a.H && ww >= 0 && ww < a.W;
      dma16s(xr, sbase + WB + buf * HB + q * 1024, ok ? (unsigned)((((n * a.H + hh) * a.W + ww) * 8) * 2) : 0x80000000u, 0u);
    }
  };
  // weight image [n-tile][k column][16 rows] of 16-B chunks: the 16 lanes of every ds_read_b128
  // lane group read 16 different rows of one column = 16 different bank slots (the padded
  // [row][29] image put 2 lanes of a group on one slot: 50 % of the LDS cycles were bank
  // conflicts, profiles/r6/r6_convpmc_7x7.txt)
  for (int q = wave; q < C74_WQ; q += 8) {
    const int L = q * 64 + lane;
    const int li = L & 15, t = L >> 4, col = t % C74_WCOL, row = (t / C74_WCOL) * 16 + li;
    dma16s(wr, sbase + q * 1024, (unsigned)((row * C74_K + col * 8) * 2), 0u);
  }
  int tile = blockIdx.x;
  if (tile < ntiles) issue_halo(tile, 0);
  if (tile + (int)gridDim.x < ntiles) issue_halo(tile + gridDim.x, 1);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  float bv[4][4];
#pragma unroll
  for (int nn = 0; nn < 4; ++nn)
#pragma unroll
    for (int i = 0; i < 4; ++i) bv[nn][i] = a.bias ? a.bias[nn * 16 + g * 4 + i] : 0.f;
  // halo pixel of this lane's output pixel (tap (0, 0)) per m-tile; the tile is 4 rows x 64
  int hbase[2];
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const int loc = wave * 32 + m * 16 + li;
    hbase[m] = (loc >> 6) * C74_HW + (loc & 63);
  }
  // BN running sums of this lane's channels nn * 16 + g * 4 + i over the block's pixels
  float bs[4][4], bq[4][4];
#pragma unroll
  for (int nn = 0; nn < 4; ++nn)
#pragma unroll
    for (int i = 0; i < 4; ++i) bs[nn][i] = bq[nn][i] = 0.f;
  int buf = 0;
  for (; tile < ntiles; tile += gridDim.x) {
    // the halo two tiles ahead goes into the buffer the previous tile released at its barrier
    const int ahead = tile + 2 * gridDim.x;
    if (ahead < ntiles) issue_halo(ahead, buf == 0 ? 2 : buf - 1);
    f32x4 acc[4][2];
#pragma unroll
    for (int nn = 0; nn < 4; ++nn)
#pragma unroll
      for (int m = 0; m < 2; ++m) acc[nn][m] = f32x4{0.f, 0.f, 0.f, 0.f};
    const char* hs = smem + WB + buf * HB;
#pragma unroll
    for (int r = 0; r < 7; ++r) {
      bf16x8 bfr[4], afr[2];
#pragma unroll
      for (int nn = 0; nn < 4; ++nn)
        bfr[nn] = *reinterpret_cast<const bf16x8*>(smem + ((nn * C74_WCOL + r * 4 + g) * 16 + li) * 16);
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        const char* p = hs + (hbase[m] + r * C74_HW + 2 * g) * 16;
        const uint2 lo = *reinterpret_cast<const uint2*>(p), hi = *reinterpret_cast<const uint2*>(p + 16);
        afr[m] = __builtin_bit_cast(bf16x8, make_uint4(lo.x, lo.y, hi.x, hi.y));
      }
#pragma unroll
      for (int nn = 0; nn < 4; ++nn)
#pragma unroll
        for (int m = 0; m < 2; ++m) acc[nn][m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[nn], afr[m], acc[nn][m], 0, 0, 0);
    }
    // epilogue: bias, BN records (one per 32-pixel wave row, as conv_epilogue), NHWC stores
    const int n = tile / (tiles_h * tiles_w), rem = tile - n * tiles_h * tiles_w;
    const int p0 = (n * a.H + (rem / tiles_w) * C74_TR) * a.W + (rem % tiles_w) * 64;
#pragma unroll
    for (int nn = 0; nn < 4; ++nn)
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[nn][m][i] += bv[nn][i];
    if (a.stats) {
#pragma unroll
      for (int nn = 0; nn < 4; ++nn)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float v0 = acc[nn][0][i], v1 = acc[nn][1][i];
          bs[nn][i] += v0 + v1;
          bq[nn][i] += v0 * v0 + v1 * v1;
        }
    }
    // 16-B stores (the guide's T21 widening, 16-lane rows): lane (li, g) holds channels
    // nt * 16 + g * 4 .. + 3 of every n-tile nt; one v_permlane16_swap per dword of an n-tile
    // pair (2q, 2q + 1) leaves lane g with the 8 contiguous channels (2q + (g & 1)) * 16 +
    // (g >> 1) * 8 .. + 7: 4 dwordx4 stores per lane and tile instead of 8 dwordx2
    auto pk = [](float lo, float hi) {
      const bf16 t[2] = {(bf16)lo, (bf16)hi};
      return *reinterpret_cast<const unsigned*>(t);
    };
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const int loc = wave * 32 + m * 16 + li;
      bf16* yp = reinterpret_cast<bf16*>(a.y) + (long)(p0 + (loc >> 6) * a.W + (loc & 63)) * a.ldy;
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const f32x4 va = acc[2 * q][m], vb = acc[2 * q + 1][m];
        const auto s0 = __builtin_amdgcn_permlane16_swap(pk(va[0], va[1]), pk(vb[0], vb[1]), false, false);
        const auto s1 = __builtin_amdgcn_permlane16_swap(pk(va[2], va[3]), pk(vb[2], vb[3]), false, false);
        *reinterpret_cast<uint4*>(yp + (2 * q + (g & 1)) * 16 + (g >> 1) * 8) = make_uint4(s0[0], s1[0], s0[1], s1[1]);
      }
    }
    // the next tile's halo was issued a whole tile earlier; younger than it are exactly the
    // previous tile's 4 stores, this tile's BN record store (waves 0-1), its halo DMA pieces
    // (2 / 1 per wave, when the tile two ahead exists) and its 4 stores: waiting for that count
    // leaves all of them in flight (vmcnt(8) made every tile wait for half of the previous
    // tile's stores); the barrier publishes it to all waves and releases this tile's buffer
    // (raw barrier: __syncthreads() would also drain the stores)
    {
      const int dpieces = ahead < ntiles ? (wave + 8 < C74_HQ ? 2 : 1) : 0;
      wait_vm_dyn(8 + dpieces);
    }
    wait_lgkm0();
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    buf = buf == 2 ? 0 : buf + 1;
  }
  if (a.stats) {
    // the block's record: lane sums over li (row16_sum), then the 8 waves in order through LDS
    // (the halo ring is free: every wave passed the last tile's barrier)
    float* sw = reinterpret_cast<float*>(smem + WB);
#pragma unroll
    for (int nn = 0; nn < 4; ++nn)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float sv = row16_sum(bs[nn][i]), qv = row16_sum(bq[nn][i]);
        if (li == 0) {
          sw[wave * 128 + nn * 16 + g * 4 + i] = sv;
          sw[wave * 128 + 64 + nn * 16 + g * 4 + i] = qv;
        }
      }
    __syncthreads();
    if (tid < 128 && (int)blockIdx.x < a.nrec) {
      float v = 0.f;
#pragma unroll
      for (int w = 0; w < 8; ++w) v += sw[w * 128 + tid];
      a.stats[(long)blockIdx.x * 128 + tid] = v;
    }
  }
}

// ----------------------------------------------------------------------------------------
// 3x3 conv with 64 input channels at full resolution (AFE.down1 forward, 64 -> 128 at 256^2),
// as a sliding band with the weights in registers.  A block of 8 waves owns 64 output channels
// of one 64-column strip of one image and walks a band of rows, 4 output rows per iteration:
// wave (rw, cg) computes output row h0 + rw x 64 pixels for the 32 channels cg of the block's
// 64, with its 2 x 18 A fragments (32 co x K = 576 = 9 taps x 64 ci) held in registers for the
// whole band (two waves per SIMD fit: ~240 registers each) -- the only LDS traffic is the input,
// 4 B fragments per 8 MFMAs.  Input rows (66 px incl. the halo columns) stream through a 10-row
// LDS ring by LDS-DMA (44 pieces per iteration spread over the waves and over the first k-steps)
// and are waited for one iteration later (counted vmcnt: the output stores issued after them
// stay in flight).  A halo pixel takes 160 B (128 B of channels + 32 B zero-filled by
// out-of-range DMA slots): 16 consecutive pixels read by ds_read_b128 are conflict-free from any
// start.  The two 64-channel halves of a strip are neighbours on one XCD, so the input is
// fetched from HBM about once.  Epilogue per iteration: bias, BN (sum, sum of squares) per lane
// over 8 iterations = one record of 512 pixels per (wave row, 8 iterations), 16-B bf16 stores
// (v_permlane16_swap pairs the two 16-channel fragments).  Replaces conv_fwd_v2's per-tap DMA.
// ----------------------------------------------------------------------------------------
constexpr int C64_PXB = 160, C64_ROWB = 11 * 1024, C64_NR = 10;   // (C64_G: conv_plan.h)
__global__ void __launch_bounds__(512, 1)
conv3c64_fwd(ConvArgs a, unsigned x_bytes, int nbands) {
  __shared__ __attribute__((aligned(1024))) char smem[C64_NR * C64_ROWB];
  __shared__ __attribute__((aligned(16))) float sbias[64];              // the block's 64 biases
  // per-lane BN partial sums of the current 8-iteration record group, [wave][16][lane] (kept
  // in LDS: their 16 registers double-buffer the B fragments instead)
  __shared__ __attribute__((aligned(16))) float sacc[8 * 16 * 64];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int cg = wave & 1, rw = wave >> 1;
  const int lr = lane & 15, lh = lane >> 4;
  // XCD-aware order: consecutive local ids (the co groups of one strip) share an XCD
  const int nblk = gridDim.x, bid = blockIdx.x;
  const int q8 = nblk / 8, r8 = nblk % 8, xcd = bid % 8;
  const int lid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + bid / 8;
  const int nco = a.Cout >> 6, strips = a.W >> 6;
  const int cgrp = lid % nco, rest = lid / nco;
  const int band = rest % nbands, strip = (rest / nbands) % strips, n = rest / (nbands * strips);
  const int BAND = a.H / nbands, hb = band * BAND, w0 = strip * 64;
  const int cw = cgrp * 64 + cg * 32;                       // this wave's first output channel

  const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.x), 0, (int)x_bytes, 0x00020000);
  const unsigned sbase = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(lds_ptr_t)smem);
  // DMA slots of a row: 16-B chunk k = piece * 64 + lane -> halo pixel k / 10, chunk k % 10
  // (recomputed per piece: a register table of the 11 offsets does not fit beside the weights)
  auto poff_of = [&](int p, int ln) {
    const int k = p * 64 + ln, px = k / 10, ch = k - px * 10;
    const int iw = w0 - 1 + px;
    return (px < 66 && ch < 8 && iw >= 0 && iw < a.W) ? (unsigned)((iw * 64 + ch * 8) * 2) : 0x80000000u;
  };
  auto row_slot = [&](int y) { return (y - hb + 1) % C64_NR; };
  // piece q (0 .. 11 * rows - 1) of the rows starting at y0: row y0 + q / 11, piece q % 11
  auto issue_piece = [&](int y0, int q) {                  // rows outside the image -> zeros
    const int y = y0 + q / 11, p = q % 11;
    const bool rok = y >= 0 && y < a.H;
    const unsigned v = poff_of(p, lane);
    dma16s(xr, sbase + row_slot(y) * C64_ROWB + p * 1024, rok ? v : 0x80000000u,
           rok ? (unsigned)((n * a.H + y) * a.W) * 128u : 0u);
  };

  // the wave's weights: A fragment (cf, ks) = 16 channels x 32 k, k = tap * 64 + ci
  bf16x8 wf[2][18];
  const bf16* wk = reinterpret_cast<const bf16*>(a.w);
#pragma unroll
  for (int cf = 0; cf < 2; ++cf)
#pragma unroll
    for (int ks = 0; ks < 18; ++ks)
      wf[cf][ks] = *reinterpret_cast<const bf16x8*>(wk + (long)(cw + cf * 16 + lr) * a.Kpad + ks * 32 + lh * 8);

  // prologue: input rows hb - 1 .. hb + 4 (66 pieces)
  for (int q = wave; q < 66; q += 8) issue_piece(hb - 1, q);
  // biases in LDS, read back per epilogue: 8 registers fewer beside the 144 weight registers
  // (loaded after the prologue DMA is on its way)
  if (tid < 64) sbias[tid] = a.bias ? a.bias[cgrp * 64 + tid] : 0.f;
  __syncthreads();

  float* const sa = sacc + wave * 16 * 64 + lane;         // element e at sa[e * 64]
  const int niter = BAND >> 2, ng = niter / C64_G;
  const int rec0 = ((n * strips + strip) * nbands + band) * (4 * ng);
  const int loff = lr * C64_PXB + lh * 16;
  auto pk = [](float lo, float hi) {
    const bf16 t[2] = {(bf16)lo, (bf16)hi};
    return *reinterpret_cast<const unsigned*>(t);
  };

  for (int it = 0; it < niter; ++it) {
    const int h0 = hb + 4 * it;
    // this iteration's rows landed; younger than them are at most the previous iteration's 4
    // output stores (+ 2 record stores), which stay in flight
    if (it == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    wait_lgkm0();
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    const bool more = it + 1 < niter;
    const int orow = h0 + rw;
    unsigned sb[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) sb[q] = (unsigned)(row_slot(orow - 1 + q) * C64_ROWB + loff);

    f32x4 acc[4][2];
#pragma unroll
    for (int pf = 0; pf < 4; ++pf)
#pragma unroll
      for (int cf = 0; cf < 2; ++cf) acc[pf][cf] = f32x4{0.f, 0.f, 0.f, 0.f};
    // B fragments double-buffered: k-step ks + 1's are read before k-step ks's MFMAs
    auto ldb = [&](bf16x8 (&fb)[4], int ks) {
      const int tap = ks >> 1, r = tap / 3, s = tap - (tap / 3) * 3, ch = ks & 1;
#pragma unroll
      for (int pf = 0; pf < 4; ++pf)
        fb[pf] = *reinterpret_cast<const bf16x8*>(smem + sb[r] + (pf * 16 + s) * C64_PXB + ch * 64);
    };
    bf16x8 fbq[2][4];
    ldb(fbq[0], 0);
#pragma unroll
    for (int ks = 0; ks < 18; ++ks) {
      if (ks + 1 < 18) ldb(fbq[(ks + 1) & 1], ks + 1);
      const bf16x8 (&fb)[4] = fbq[ks & 1];
      // the next iteration's rows h0 + 5 .. h0 + 8: pieces wave, wave + 8, ... < 44
      if (ks < 6 && more && wave + 8 * ks < 44) issue_piece(h0 + 5, wave + 8 * ks);
#pragma unroll
      for (int pf = 0; pf < 4; ++pf)
#pragma unroll
        for (int cf = 0; cf < 2; ++cf)
          acc[pf][cf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[cf][ks], fb[pf], acc[pf][cf], 0, 0, 0);
    }

    // epilogue: bias, BN partials, 16-B stores: lane (lr, lh) holds channels cf * 16 + lh * 4
    // .. + 3 of pixel lr; one v_permlane16_swap per dword pair leaves lane lh with the 8
    // contiguous channels (lh & 1) * 16 + (lh >> 1) * 8 .. + 7
    bf16* yp = reinterpret_cast<bf16*>(a.y) + ((long)(n * a.H + orow) * a.W + w0 + lr) * a.ldy + cw +
               (lh & 1) * 16 + (lh >> 1) * 8;
    float st[2][4], sq[2][4];
    const bool g0 = (it % C64_G) == 0;                    // the record group's first iteration
#pragma unroll
    for (int cf = 0; cf < 2; ++cf)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        st[cf][i] = g0 ? 0.f : sa[(cf * 4 + i) * 64];
        sq[cf][i] = g0 ? 0.f : sa[(8 + cf * 4 + i) * 64];
      }
#pragma unroll
    for (int pf = 0; pf < 4; ++pf) {
      float v[2][4];
#pragma unroll
      for (int cf = 0; cf < 2; ++cf)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          v[cf][i] = acc[pf][cf][i] + sbias[cg * 32 + cf * 16 + lh * 4 + i];
          st[cf][i] += v[cf][i];
          sq[cf][i] += v[cf][i] * v[cf][i];
        }
      const auto s0 = __builtin_amdgcn_permlane16_swap(pk(v[0][0], v[0][1]), pk(v[1][0], v[1][1]), false, false);
      const auto s1 = __builtin_amdgcn_permlane16_swap(pk(v[0][2], v[0][3]), pk(v[1][2], v[1][3]), false, false);
      *reinterpret_cast<uint4*>(yp + (long)pf * 16 * a.ldy) = make_uint4(s0[0], s1[0], s0[1], s1[1]);
    }
    if ((it % C64_G) != C64_G - 1) {
#pragma unroll
      for (int cf = 0; cf < 2; ++cf)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          sa[(cf * 4 + i) * 64] = st[cf][i];
          sa[(8 + cf * 4 + i) * 64] = sq[cf][i];
        }
    } else if (a.stats) {
      // record (block, 8-iteration group, wave row): lanes 0-3 of a 16-lane row store the 4
      // channel sums, lanes 4-7 the squares (conv_epilogue's record layout)
      const int rec = rec0 + (it / C64_G) * 4 + rw;
#pragma unroll
      for (int cf = 0; cf < 2; ++cf) {
        float sv[4], qv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          sv[i] = row16_sum(st[cf][i]);
          qv[i] = row16_sum(sq[cf][i]);
        }
        const int cb = cw + cf * 16 + lh * 4, ii = lr & 3;
        const float s01 = ii & 1 ? sv[1] : sv[0], s23 = ii & 1 ? sv[3] : sv[2];
        const float q01 = ii & 1 ? qv[1] : qv[0], q23 = ii & 1 ? qv[3] : qv[2];
        const float val = lr < 4 ? (ii & 2 ? s23 : s01) : (ii & 2 ? q23 : q01);
        if (lr < 8 && rec < a.nrec) a.stats[(long)(rec * 2 + (lr >> 2)) * a.Cout + cb + ii] = val;
      }
    }
  }
}

// ----------------------------------------------------------------------------------------
// conv3up_band_fwd: the UpBlock2D forward (nearest x2 upsample + 3x3 as 4 sub-pixel phases of a
// 2x2 conv over the low-res input, modules.py:78-89) for a 128-channel input, as a sliding band
// like conv3c64_fwd: a block owns (image, 32-column low-res strip = 64 output columns, 64 output
// channels, band of low-res rows); wave (phase pa pb, 32-channel group cg) keeps its phase's
// 32 co x K = 4 taps x 128 ci weights as MFMA A fragments in registers (128 VGPRs) for the whole
// band, so the only LDS traffic is the input: low-res rows (34 pixels incl. the column halo) land
// ONCE by LDS-DMA in a 6-row ring (272-B pixels: 16 consecutive pixels read by ds_read_b128 are
// conflict-free) -- the halo kernel (MODE 1) restaged a 4-row halo per 32-channel chunk for only
// 4 taps of work, bandwidth-bound.  An iteration = 2 low-res rows (4 output rows); wave (pa, pb)
// writes output rows 2h + pa, columns 2w + pb.  Epilogue: bias, BN records of 256 pixels
// (4 iterations x 2 rows x 32 columns of one phase; the two channel-group waves of the phase fill
// the record's 64 channels), 16-B stores (v_permlane16_swap pairs the 16-channel fragments).
// Weights: the sub-pixel layout of weight_prep_subpix_kernel, wk [4][rows][Kpad = 512].
// ----------------------------------------------------------------------------------------
constexpr int UPB_PXB = 272, UPB_ROWB = 10 * 1024, UPB_NR = 6;    // (UPB_G: conv_plan.h)
__global__ void __launch_bounds__(512, 1)
conv3up_band_fwd(ConvArgs a, unsigned x_bytes, int nbands) {
  __shared__ __attribute__((aligned(1024))) char smem[UPB_NR * UPB_ROWB];
  __shared__ __attribute__((aligned(16))) float sbias[64];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int cg = wave & 1, ph = wave >> 1, pa = ph >> 1, pb = ph & 1;
  const int lr = lane & 15, lh = lane >> 4;
  // XCD-aware order: consecutive local ids (the co groups of one strip) share an XCD
  const int nblk = gridDim.x, bid = blockIdx.x;
  const int q8 = nblk / 8, r8 = nblk % 8, xcd = bid % 8;
  const int lid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + bid / 8;
  const int nco = a.Cout >> 6, strips = a.Win >> 5;
  const int cgrp = lid % nco, rest = lid / nco;
  const int band = rest % nbands, strip = (rest / nbands) % strips, n = rest / (nbands * strips);
  const int BAND = a.Hin / nbands, hb = band * BAND, wl0 = strip * 32;
  const int cw = cgrp * 64 + cg * 32;                        // this wave's first output channel

  const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.x), 0, (int)x_bytes, 0x00020000);
  const unsigned sbase = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(lds_ptr_t)smem);
  // DMA slots of a row: 16-B chunk k = piece * 64 + lane -> LDS pixel k / 17 (low-res column
  // wl0 - 1 + k / 17), chunk k % 17 (chunk 16: the pad)
  auto poff_of = [&](int p, int ln) {
    const int k = p * 64 + ln, px = k / 17, ch = k - px * 17;
    const int iw = wl0 - 1 + px;
    return (px < 34 && ch < 16 && iw >= 0 && iw < a.Win) ? (unsigned)((iw * 128 + ch * 8) * 2) : 0x80000000u;
  };
  auto row_slot = [&](int y) { return (y - hb + 1) % UPB_NR; };
  // piece q (0 .. 10 * rows - 1) of the rows starting at y0: row y0 + q / 10, piece q % 10
  auto issue_piece = [&](int y0, int q) {                  // rows outside the image -> zeros
    const int y = y0 + q / 10, p = q % 10;
    const bool rok = y >= 0 && y < a.Hin;
    dma16s(xr, sbase + row_slot(y) * UPB_ROWB + p * 1024, rok ? poff_of(p, lane) : 0x80000000u,
           rok ? (unsigned)((n * a.Hin + y) * a.Win) * 256u : 0u);
  };

  // the wave's weights: A fragment (cf, ks) = 16 channels x 32 k, k = (rr * 2 + ss) * 128 + ci
  bf16x8 wf[2][16];
  const bf16* wk = reinterpret_cast<const bf16*>(a.w) + (long)ph * a.wphase;
#pragma unroll
  for (int cf = 0; cf < 2; ++cf)
#pragma unroll
    for (int ks = 0; ks < 16; ++ks)
      wf[cf][ks] = *reinterpret_cast<const bf16x8*>(wk + (long)(cw + cf * 16 + lr) * a.Kpad + ks * 32 + lh * 8);

  // prologue: low-res rows hb - 1 .. hb + 2 (40 pieces)
  for (int q = wave; q < 40; q += 8) issue_piece(hb - 1, q);
  if (tid < 64) sbias[tid] = a.bias ? a.bias[cgrp * 64 + tid] : 0.f;
  __syncthreads();

  float st[2][4], sq[2][4];
#pragma unroll
  for (int cf = 0; cf < 2; ++cf)
#pragma unroll
    for (int i = 0; i < 4; ++i) st[cf][i] = sq[cf][i] = 0.f;
  const int niter = BAND >> 1, ng = niter / UPB_G;
  const int rec0 = ((n * strips + strip) * nbands + band) * (4 * ng);
  auto pk = [](float lo, float hi) {
    const bf16 t[2] = {(bf16)lo, (bf16)hi};
    return *reinterpret_cast<const unsigned*>(t);
  };

  for (int it = 0; it < niter; ++it) {
    const int h0 = hb + 2 * it;
    // this iteration's rows landed; younger than them are at most the previous iteration's 4
    // output stores (+ record stores), which stay in flight
    if (it == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    wait_lgkm0();
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    const bool more = it + 1 < niter;
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      const int h = h0 + hh;
      // input rows h + pa - 1 + rr, LDS pixel of output column w: w + pb + ss (halo offset 1)
      unsigned sb[2];
#pragma unroll
      for (int rr = 0; rr < 2; ++rr) sb[rr] = (unsigned)(row_slot(h + pa - 1 + rr) * UPB_ROWB + (lr + pb) * UPB_PXB + lh * 16);
      auto ldb = [&](bf16x8 (&fb)[2], int ks) {
        const int tap = ks >> 2, rr = tap >> 1, ss = tap & 1, cc = ks & 3;
#pragma unroll
        for (int m = 0; m < 2; ++m)
          fb[m] = *reinterpret_cast<const bf16x8*>(smem + sb[rr] + (m * 16 + ss) * UPB_PXB + cc * 64);
      };
      f32x4 acc[2][2];
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int cf = 0; cf < 2; ++cf) acc[m][cf] = f32x4{0.f, 0.f, 0.f, 0.f};
      bf16x8 fbq[2][2];
      ldb(fbq[0], 0);
#pragma unroll
      for (int ks = 0; ks < 16; ++ks) {
        if (ks + 1 < 16) ldb(fbq[(ks + 1) & 1], ks + 1);
        // the next iteration's rows h0 + 3, h0 + 4: pieces wave, wave + 8, wave + 16 < 20
        if (hh == 0 && ks < 3 && more && wave + 8 * ks < 20) issue_piece(h0 + 3, wave + 8 * ks);
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
          for (int cf = 0; cf < 2; ++cf)
            acc[m][cf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[cf][ks], fbq[ks & 1][m], acc[m][cf], 0, 0, 0);
      }
      // epilogue of output row 2h + pa: lane (lr, lh) holds channels cf * 16 + lh * 4 .. + 3 of
      // column w = m * 16 + lr (output column 2 (wl0 + w) + pb)
      const int Y = 2 * h + pa;
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        float v[2][4];
#pragma unroll
        for (int cf = 0; cf < 2; ++cf)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            v[cf][i] = acc[m][cf][i] + sbias[cg * 32 + cf * 16 + lh * 4 + i];
            st[cf][i] += v[cf][i];
            sq[cf][i] += v[cf][i] * v[cf][i];
          }
        const auto s0 = __builtin_amdgcn_permlane16_swap(pk(v[0][0], v[0][1]), pk(v[1][0], v[1][1]), false, false);
        const auto s1 = __builtin_amdgcn_permlane16_swap(pk(v[0][2], v[0][3]), pk(v[1][2], v[1][3]), false, false);
        const int X = 2 * (wl0 + m * 16 + lr) + pb;
        bf16* yp = reinterpret_cast<bf16*>(a.y) + ((long)(n * a.Ho + Y) * a.Wo + X) * a.ldy + cw + (lh & 1) * 16 +
                   (lh >> 1) * 8;
        *reinterpret_cast<uint4*>(yp) = make_uint4(s0[0], s1[0], s0[1], s1[1]);
      }
    }
    if (a.stats && (it % UPB_G) == UPB_G - 1) {
      // record (block, 4-iteration group, phase): lanes 0-3 of a 16-lane row store the 4 channel
      // sums, lanes 4-7 the squares (conv_epilogue's record layout)
      const int rec = rec0 + (it / UPB_G) * 4 + ph;
#pragma unroll
      for (int cf = 0; cf < 2; ++cf) {
        float sv[4], qv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          sv[i] = row16_sum(st[cf][i]);
          qv[i] = row16_sum(sq[cf][i]);
          st[cf][i] = sq[cf][i] = 0.f;
        }
        const int cb = cw + cf * 16 + lh * 4, ii = lr & 3;
        const float s01 = ii & 1 ? sv[1] : sv[0], s23 = ii & 1 ? sv[3] : sv[2];
        const float q01 = ii & 1 ? qv[1] : qv[0], q23 = ii & 1 ? qv[3] : qv[2];
        const float val = lr < 4 ? (ii & 2 ? s23 : s01) : (ii & 2 ? q23 : q01);
        if (lr < 8 && rec < a.nrec) a.stats[(long)(rec * 2 + (lr >> 2)) * a.Cout + cb + ii] = val;
      }
    }
  }
}

// ----------------------------------------------------------------------------------------
// 1x1 conv as a pixel stream: AFE.mid_conv 256 -> 512 (models.py:934) and Generator.mid_conv
// 256 -> 256 (models.py:1096) forward, and their data gradients (the same GEMM with the
// transposed weights, K = Cout).  out[p][co] = bias[co] + sum_k x[p][k] W[co][k]: per output
// pixel 2 K bytes in and 2 Cout bytes out for 2 K Cout FLOP, so at K <= 512 the launch is
// HBM-bound (conv_fwd_v2's 256 x 256 tile, one block per CU, alternated load -> MFMA -> store
// phases across the whole chip: 3.4 TB/s).
// A block owns 256 output channels; wave w keeps rows [32 w, 32 w + 32) of W for the whole
// launch as MFMA A fragments in registers (K / 4 VGPRs) and the block walks pixel tiles of
// BP = 16384 / K pixels (32 KB of x) persistently.  The x tiles land by LDS-DMA in a 4-slot
// ring, 3 tiles in flight while one is computed (with 2 slots of 64 KB only one tile was in
// flight per CU: 3.3 TB/s); the staged epilogue's stores of tile t drain under the DMA of
// tile t + 4, issued into the slot tile t just freed.  LDS rows are K * 2 bytes with the 16-B chunks XOR-swizzled by (pixel & 15)
// through the per-lane DMA source, so a fragment read (16 pixels at one k) is conflict-free.
// Co groups of one pixel stream are neighbouring blocks of one XCD (x read once into its L2).
// Requires P % BP == 0, Cout % 256 == 0, dense NHWC (ldy = Cout), no residual / statistics.
// ----------------------------------------------------------------------------------------
template <int K, int BPX>
__global__ void __launch_bounds__(512, 1)
conv1x1_stream(ConvArgs a, unsigned x_bytes) {
  constexpr int ROWB = K * 2, BP = BPX, RM = BP / 16, RN = 2, NKS = K / 32;
  constexpr int SLOT = BP * ROWB;                   // 32 / 64 KB
  constexpr int NSL = 131072 / SLOT;                // ring slots in 128 KB: NSL - 1 tiles in flight
  constexpr int PPW = SLOT / 1024 / 8;              // DMA pieces per wave per tile
  constexpr int RPP = 1024 / ROWB;                  // pixel rows per piece (2 / 1)
  constexpr int NST = RM;                           // 16-B output stores per lane per tile
  static_assert(K == 256 || K == 512, "conv1x1_stream: K of 256 or 512");
  static_assert(NSL >= 2 && NSL <= 4 && (NSL - 1) * PPW + NSL * NST <= 63, "conv1x1_stream: ring / vmcnt");
  __shared__ __attribute__((aligned(1024))) char smem[NSL * SLOT];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lr = lane & 15, lh = lane >> 4;
  const int ncg = a.Cout / 256;
  const int bid = blockIdx.x, G = gridDim.x;
  const int cg = (bid / 8) % ncg;                   // the co groups of a stream share an XCD
  const int stream = bid % 8 + 8 * ((bid / 8) / ncg), nstream = G / ncg;
  const int co0 = cg * 256;
  const int ntp = a.P / BP;

  const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.x), 0, (int)x_bytes, 0x00020000);
  const unsigned sbase = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(lds_ptr_t)smem);
  // lane part of a DMA piece: byte l * 16 of the piece = (row l / (64 / RPP), physical chunk);
  // the source is logical chunk (physical ^ (pixel & 15)); the piece's pixel offset & 15 is
  // RPP * (wave + 8 i) & 15: constant over i for RPP = 2, alternating for RPP = 1
  unsigned voff[2];
#pragma unroll
  for (int par = 0; par < 2; ++par) {
    const int rip = lane / (64 / RPP), pc = lane % (64 / RPP);
    const int prow = (RPP * (wave + 8 * par) + rip) & 15;
    voff[par] = (unsigned)((rip * K + ((pc ^ prow) << 3)) * 2);
  }
  // tile t into `slot`; t >= ntp issues the same pieces out of range (zero fill, no branch:
  // a branch here made the compiler keep live arrays in scratch across it)
  auto issue = [&](int t, int slot) {
    const unsigned base = sbase + slot * SLOT;
    const bool ok = t < ntp;
#pragma unroll
    for (int i = 0; i < PPW; ++i) {
      const int q = wave + 8 * i;
      dma16s(xr, base + q * 1024, ok ? voff[RPP == 2 ? 0 : (i & 1)] : 0x80000000u,
             ok ? (unsigned)(((t * BP + q * RPP) * K) * 2) : 0u);
    }
  };
  // this wave's weights: rows co0 + 32 wave + 16 n + lr, k = 32 s + 8 lh .. + 7
  Frag<bf16> wa[NKS][RN];
  {
    const bf16* w = reinterpret_cast<const bf16*>(a.w);
#pragma unroll
    for (int ss = 0; ss < NKS; ++ss)
#pragma unroll
      for (int n = 0; n < RN; ++n)
        wa[ss][n].v = *reinterpret_cast<const bf16x8*>(w + (long)(co0 + 32 * wave + 16 * n + lr) * a.Kpad + 32 * ss + 8 * lh);
  }
  // this lane's biases (channels co0 + 32 wave + 16 n + 4 lh + i), for every tile
  float bv[RN][4];
#pragma unroll
  for (int n = 0; n < RN; ++n)
#pragma unroll
    for (int i = 0; i < 4; ++i) bv[n][i] = a.bias ? a.bias[co0 + 32 * wave + 16 * n + 4 * lh + i] : 0.f;
  // fragment read of k-step s, m-tile m: pixel m * 16 + lr, physical chunk (4 s + lh) ^ lr
  unsigned foff[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) foff[q] = (unsigned)(lr * ROWB + (((4 * q + lh) ^ lr) << 4));
  auto pk = [](float lo, float hi) {
    const bf16 t2[2] = {(bf16)lo, (bf16)hi};
    return *reinterpret_cast<const unsigned*>(t2);
  };
  bf16* const yw = reinterpret_cast<bf16*>(a.y) + co0 + 32 * wave + (lh & 1) * 16 + (lh >> 1) * 8;

  int t = stream;
  if (t >= ntp) return;
#pragma unroll
  for (int j = 0; j < NSL; ++j) issue(t + j * nstream, j);
  for (int i = 0; t < ntp; t += nstream, ++i) {
    const int slot = i % NSL;
    // tile t landed: every wave waits for its own pieces, the barrier publishes them.  Issued
    // after tile t's pieces, in order: the prologue's later tiles, then per finished tile u the
    // pieces of tile u + NSL (zero-fill past the last tile) and u's stores -- exactly
    // (NSL - 1) x PPW pieces and min(i, NSL) x NST stores
    const int ni = i < NSL ? i : NSL;
    if (ni == 0) wait_vm<(NSL - 1) * PPW>();
    else if (ni == 1) wait_vm<(NSL - 1) * PPW + NST>();
    else if (ni == 2) wait_vm<(NSL - 1) * PPW + 2 * NST>();
    else if (ni == 3) wait_vm<(NSL - 1) * PPW + 3 * NST>();
    else wait_vm<(NSL - 1) * PPW + 4 * NST>();
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    f32x4 acc[RN][RM];
#pragma unroll
    for (int n = 0; n < RN; ++n)
#pragma unroll
      for (int m = 0; m < RM; ++m) acc[n][m] = f32x4{0.f, 0.f, 0.f, 0.f};
    const char* xs = smem + slot * SLOT;
    // two fragment sets: k-step ss + 1's reads under k-step ss's MFMAs; the scheduling
    // barriers keep the compiler from hoisting every k-step's reads (all of them in flight
    // spilled ~54 registers beside the resident weights)
    Frag<bf16> f0[RM], f1[RM];
    auto rd = [&](Frag<bf16> (&f)[RM], int ss) {
#pragma unroll
      for (int m = 0; m < RM; ++m) f[m].lds(xs + foff[ss & 3] + (ss >> 2) * 256 + m * 16 * ROWB);
    };
    auto mm = [&](const Frag<bf16> (&f)[RM], int ss) {
#pragma unroll
      for (int m = 0; m < RM; ++m)
#pragma unroll
        for (int n = 0; n < RN; ++n) acc[n][m] = mma(wa[ss][n], f[m], acc[n][m]);
    };
    rd(f0, 0);
#pragma unroll
    for (int ss = 0; ss < NKS; ss += 2) {
      rd(f1, ss + 1);
      __builtin_amdgcn_sched_barrier(0);
      mm(f0, ss);
      __builtin_amdgcn_sched_barrier(0);
      if (ss + 2 < NKS) rd(f0, ss + 2);
      __builtin_amdgcn_sched_barrier(0);
      mm(f1, ss + 1);
      __builtin_amdgcn_sched_barrier(0);
    }
    // every wave's fragment reads of the slot are done: refill it with tile t + NSL at once,
    // then the stores of tile t straight from the accumulators -- + bias, bf16, the two
    // 16-channel n-tiles paired by v_permlane16_swap so lane (lr, lh) holds 8 contiguous
    // channels ((lh & 1) * 16 + (lh >> 1) * 8 of the wave's 32) of pixel m * 16 + lr: one
    // 16-B store per m-tile (4 lanes = one 64-B channel run of a pixel)
    wait_lgkm0();
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    issue(t + NSL * nstream, slot);
#pragma unroll
    for (int m = 0; m < RM; ++m) {
      const f32x4 va = acc[0][m], vb = acc[1][m];
      const auto s0 = __builtin_amdgcn_permlane16_swap(pk(va[0] + bv[0][0], va[1] + bv[0][1]),
                                                       pk(vb[0] + bv[1][0], vb[1] + bv[1][1]), false, false);
      const auto s1 = __builtin_amdgcn_permlane16_swap(pk(va[2] + bv[0][2], va[3] + bv[0][3]),
                                                       pk(vb[2] + bv[1][2], vb[3] + bv[1][3]), false, false);
      *reinterpret_cast<uint4*>(yw + (long)(t * BP + m * 16 + lr) * a.ldy) = make_uint4(s0[0], s1[0], s0[1], s1[1]);
    }
  }
  wait_vm<0>();      // the zero-fill pieces of the last tiles land before the workgroup's LDS is freed
}

// ----------------------------------------------------------------------------------------
// 7x7 conv with a 64-channel input and <= 4 output channels (Generator.out_conv 64 -> 3,
// models.py:1099 + sigmoid 1110), "column taps in N": for every input pixel w' of a row the
// block computes D[h][w'][(co, s)] = sum_{r, ci} x[h + r - 3][w'][ci] * W[co][ci][r][s]
// (M = pixels incl. the 3-pixel column halo, N = co x 7 taps = 21 of 32, K = 7 rows x 64 ci
// = 448), then out[h][w][co] = bias + sum_s D[h][w + s - 3][(co, s)].  3.5x fewer MFMAs than
// padding N = 3 to 16 with K = 3136, and each A fragment feeds two n-tiles.
// Block: TR = 4 output rows x 64 columns, 8 waves; halo [10 rows][70 cols][64 ci] in LDS.
// Wave w: row w >> 1 and five (m-tile, n-tile) pairs of that row's 5 m-tiles x 2 n-tiles.
// Weights wn [32][448] (n = co * 7 + s, k = r * 64 + ci, 28 KB) are staged in LDS with the halo.
// ----------------------------------------------------------------------------------------
// (C7_TR, the output rows per band step: conv_plan.h)

// ----------------------------------------------------------------------------------------
// conv7_n3_fwd2: the "column taps in N" out_conv forward, sliding down a band of rows.
// (Its per-tile predecessor staged a 10-row halo for every 4 output rows: 2.5x input re-read,
// 598 MB of HBM per launch for a 268 MB input, one block per CU; 189 -> 118 us.)  Here a block
// owns (image, 64-column strip, band of C7B_BAND output rows) and keeps a ring of 14 input
// rows in LDS (72 pixels x 128 B = 9 pieces of 1 KB per row, so a row is whole DMA pieces):
// while the 8 waves compute output rows 4j..4j+3 from ring rows 4j-3..4j+6, the DMA of rows
// 4j+7..4j+10 (the next group's) is in flight.  Input bytes per launch ~1.05x the tensor.
// The weights sit in registers as MFMA B fragments (14 k-steps x 2 n-tiles, 112 VGPRs).
// Per group: D[row][w'][n] (fp32, the 21 used columns) through LDS, then the 7-tap column
// sums + bias (+ sigmoid, + BN records).
// ----------------------------------------------------------------------------------------
constexpr int C7B_SLOTS = 14, C7B_ROWPX = 72, C7B_ROWB = C7B_ROWPX * 128;   // 9216 B
constexpr int C7B_DLD = 22;                                                // D row stride (floats)
__global__ void __launch_bounds__(512, 1)
conv7_n3_fwd2(ConvArgs a, unsigned x_bytes, int band) {
  constexpr int RING = C7B_SLOTS * C7B_ROWB;                // 129024
  constexpr int DB = C7_TR * 70 * C7B_DLD * 4;               // 24640
  __shared__ __attribute__((aligned(1024))) char smem[RING + DB];
  float* Dl = reinterpret_cast<float*>(smem + RING);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tiles_w = a.W / 64, bands = a.H / band;
  const int blk = blockIdx.x;
  const int n = blk / (bands * tiles_w);
  const int rem = blk - n * bands * tiles_w;
  const int hb = (rem / tiles_w) * band, w0 = (rem % tiles_w) * 64;
  const int li = lane & 15, g = lane >> 4;
  const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.x), 0, (int)x_bytes, 0x00020000);

  // ring row `rel` (input row hb - 3 + rel) -> slot rel % 14; 9 pieces per row
  auto issue_rows = [&](int rel0, int nrows) {
    for (int q = wave; q < nrows * 9; q += 8) {
      const int rr = q / 9, pc = q - rr * 9;
      const int rel = rel0 + rr;
      const int hh = hb - 3 + rel;
      const int L = pc * 64 + lane;                 // chunk within the row
      const int px = L >> 3, ch = L & 7;
      const int ww = w0 - 3 + px;
      const bool ok = px < 70 && hh >= 0 && hh < a.H && ww >= 0 && ww < a.W;
      // 16-B chunk swizzle by (px >> 1) & 7: 16 consecutive pixels (one fragment read) land on 16
      // different bank slots (by px & 7, pixels 8 apart shared one: 14 % bank conflicts)
      const unsigned off = ok ? (unsigned)((((n * a.H + hh) * a.W + ww) * 64 + ((ch ^ ((px >> 1) & 7)) << 3)) * 2)
                              : 0x80000000u;
      dma16(xr, smem + (rel % C7B_SLOTS) * C7B_ROWB + pc * 1024, off);
    }
  };
  issue_rows(0, 10);

  // weights wn [32][448] bf16 -> B fragments in registers
  const bf16* __restrict__ wn = reinterpret_cast<const bf16*>(a.w);
  bf16x8 bw[14][2];
#pragma unroll
  for (int ks = 0; ks < 14; ++ks)
#pragma unroll
    for (int t = 0; t < 2; ++t) bw[ks][t] = *reinterpret_cast<const bf16x8*>(wn + (t * 16 + li) * 448 + (ks * 4 + g) * 8);

  const int row = wave >> 1, half = wave & 1;
  const int mb = half ? 2 : 0;
  int apix[3];
#pragma unroll
  for (int t = 0; t < 3; ++t) apix[t] = min((mb + t) * 16 + li, C7B_ROWPX - 1);
  const int pm[5] = {half ? 2 : 0, half ? 3 : 0, half ? 3 : 1, half ? 4 : 1, half ? 4 : 2};
  const int pn[5] = {half ? 1 : 0, half ? 0 : 1, half ? 1 : 0, half ? 0 : 1, half ? 1 : 0};
  const int HWo = a.H * a.W;
  const int ngroups = band / C7_TR;
  float bias4[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) bias4[c] = (a.bias && c < a.Cout) ? a.bias[c] : 0.f;
  // the epilogue's store instructions per group of this wave (lane 0's two record stores per
  // output too when statistics are on): the wait at the next group's top leaves them in flight
  // (it was vmcnt(0): every group waited for the previous group's output stores)
  const int nout = C7_TR * 64 * a.Cout;
  const int nst = (nout > wave * 64 ? (nout - wave * 64 + 511) / 512 : 0) * (a.stats ? 3 : 1);

  for (int j = 0; j < ngroups; ++j) {
    // group j's rows (issued at group j - 1's top; only this wave's stores of group j - 1 are
    // younger) landed for this wave; the barrier publishes every wave's and retires group
    // j - 1's D reads
    if (j == 0) wait_vm<0>();
    else wait_vm_dyn(nst);
    wait_lgkm0();
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (j + 1 < ngroups) issue_rows(4 * j + 10, 4);
    f32x4 acc[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 7; ++r) {
      const char* slot = smem + ((4 * j + row + r) % C7B_SLOTS) * C7B_ROWB;
#pragma unroll
      for (int kh = 0; kh < 2; ++kh) {
        const int ks = r * 2 + kh, c = kh * 4 + g;
        bf16x8 afr[3];
#pragma unroll
        for (int t = 0; t < 3; ++t)
          afr[t] = *reinterpret_cast<const bf16x8*>(slot + (apix[t] * 8 + (c ^ ((apix[t] >> 1) & 7))) * 16);
        if (half == 0) {
          acc[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afr[0], bw[ks][0], acc[0], 0, 0, 0);
          acc[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afr[0], bw[ks][1], acc[1], 0, 0, 0);
          acc[2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afr[1], bw[ks][0], acc[2], 0, 0, 0);
          acc[3] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afr[1], bw[ks][1], acc[3], 0, 0, 0);
          acc[4] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afr[2], bw[ks][0], acc[4], 0, 0, 0);
        } else {
          acc[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afr[0], bw[ks][1], acc[0], 0, 0, 0);
          acc[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afr[1], bw[ks][0], acc[1], 0, 0, 0);
          acc[2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afr[1], bw[ks][1], acc[2], 0, 0, 0);
          acc[3] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afr[2], bw[ks][0], acc[3], 0, 0, 0);
          acc[4] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afr[2], bw[ks][1], acc[4], 0, 0, 0);
        }
      }
    }
    // D[row][w'][n]: pixel w' = m*16 + 4g + i (MFMA row), column n = nt*16 + li; keep n < 21, w' < 70
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      const int nn = pn[i] * 16 + li;
      if (nn < 21) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int wp = pm[i] * 16 + g * 4 + q;
          if (wp < 70) Dl[(row * 70 + wp) * C7B_DLD + nn] = acc[i][q];
        }
      }
    }
    wait_lgkm0();                              // D written (LDS only: the row DMA stays in flight)
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    const int h0 = hb + 4 * j;
    for (int o = tid; o < nout; o += 512) {
      const int co = o / (C7_TR * 64), rr = (o / 64) % C7_TR, w = o % 64;
      float v = co == 0 ? bias4[0] : co == 1 ? bias4[1] : co == 2 ? bias4[2] : bias4[3];
#pragma unroll
      for (int s7 = 0; s7 < 7; ++s7) v += Dl[(rr * 70 + w + s7) * C7B_DLD + co * 7 + s7];
      if (a.stats) {
        const float sv = wave_sum(v), qv = wave_sum(v * v);
        const int rec = ((n * a.H + h0 + rr) * a.W + w0) >> 6;
        if (lane == 0 && rec < a.nrec) {
          a.stats[(long)(rec * 2) * a.Cout + co] = sv;
          a.stats[(long)(rec * 2 + 1) * a.Cout + co] = qv;
        }
      }
      if (a.sigmoid) v = 1.f / (1.f + expf(-v));
      const int pix = (h0 + rr) * a.W + w0 + w;
      if (a.nchw) reinterpret_cast<float*>(a.y)[((long)(n * a.Cout + co)) * HWo + pix] = v;
      else reinterpret_cast<bf16*>(a.y)[((long)n * HWo + pix) * a.ldy + co] = (bf16)v;
    }
  }
}


}  // namespace

// cin: 8 (4 output rows per block, weights in LDS) or 64 (2 rows, k split over the waves)
int launch_halo7(const ConvArgs& a, int cin, int nblk, unsigned xb, hipStream_t s) {
  if (cin == 8) hipLaunchKernelGGL((conv_halo_fwd<7, 8, 4, 4, true, false>), dim3(nblk), dim3(512), 0, s, a, xb);
  else if (cin == 64) hipLaunchKernelGGL((conv_halo_fwd<7, 64, 1, 2, false, true>), dim3(nblk), dim3(512), 0, s, a, xb);
  else return FV_E_UNSUPPORTED;
  return FV_OK;
}

void launch_c74(const ConvArgs& a, int grid, unsigned xb, int ntiles, hipStream_t s) {
  hipLaunchKernelGGL(conv7c4_fwd, dim3(grid), dim3(512), 0, s, a, xb, ntiles);
}

void launch_c64(const ConvArgs& a, int nblk, unsigned xb, int nbands, hipStream_t s) {
  hipLaunchKernelGGL(conv3c64_fwd, dim3(nblk), dim3(512), 0, s, a, xb, nbands);
}

void launch_upband(const ConvArgs& a, int nblk, unsigned xb, int nbands, hipStream_t s) {
  hipLaunchKernelGGL(conv3up_band_fwd, dim3(nblk), dim3(512), 0, s, a, xb, nbands);
}

// (k, bpx): input channels and pixels per tile, (256, 64 / 128) or (512, 32 / 64)
int launch_c1s(const ConvArgs& a, int k, int bpx, int grid, unsigned xb, hipStream_t s) {
  if (k == 256 && bpx == 128) hipLaunchKernelGGL((conv1x1_stream<256, 128>), dim3(grid), dim3(512), 0, s, a, xb);
  else if (k == 256 && bpx == 64) hipLaunchKernelGGL((conv1x1_stream<256, 64>), dim3(grid), dim3(512), 0, s, a, xb);
  else if (k == 512 && bpx == 64) hipLaunchKernelGGL((conv1x1_stream<512, 64>), dim3(grid), dim3(512), 0, s, a, xb);
  else if (k == 512 && bpx == 32) hipLaunchKernelGGL((conv1x1_stream<512, 32>), dim3(grid), dim3(512), 0, s, a, xb);
  else return FV_E_UNSUPPORTED;
  return FV_OK;
}

void launch_c7n(const ConvArgs& a, int nblk, unsigned xb, int band, hipStream_t s) {
  hipLaunchKernelGGL(conv7_n3_fwd2, dim3(nblk), dim3(512), 0, s, a, xb, band);
}
