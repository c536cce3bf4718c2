// 2-D convolution, the register-staged generic forward kernel conv_fwd_kernel (fp32 / bf16, BN
// prologue, nearest-x2 upsample, stride-2 variants) with its launchers.
#include "conv_common.h"

namespace {

// S2 (stride-2 3x3 conv, padding 1; fv_conv2d_s2_*): 1 = forward, tile space = the H x W output,
// input (Hin, Win) = (2H, 2W) read at 2 * out + tap - 1; 2 = one phase (a.sub = 1 + 2 pa + pb) of
// its data gradient, a transposed conv: tile space = the H x W gradient image dy (the input),
// tile pixel (h, w) stores dx pixel (2h + pa, 2w + pb) and gathers only the phase's live taps,
// (1 + pa) x (1 + pb) of them at offsets {0, +1} (weights: weight_prep_s2t_kernel).
template <typename T, int KS, int WN, int WM, int RN, int RM, bool PRO, bool UPS, int S2 = 0>
__global__ void __launch_bounds__(64 * WN * WM)
conv_fwd_kernel(ConvArgs a) {
  constexpr int NT = 64 * WN * WM;
  constexpr int BN = WN * RN * 16;   // output channels per block
  constexpr int BM = WM * RM * 16;   // pixels per block
  constexpr int PAD = KS / 2;
  constexpr int ES = sizeof(T);
  constexpr int ROWB = BK * ES;
  constexpr int CA = BM * 4 / NT;
  constexpr int NBCH = BN * 4;
  constexpr int CB = (NBCH + NT - 1) / NT;
  static_assert((BM * 4) % NT == 0, "A staging");
  __shared__ __attribute__((aligned(16))) char smem[2 * (BM + BN) * ROWB];

  const T* __restrict__ x = reinterpret_cast<const T*>(a.x);
  const T* __restrict__ wk = reinterpret_cast<const T*>(a.w);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wn = wave % WN, wm = wave / WN;
  const int tn = blockIdx.x % a.ntn, tm = blockIdx.x / a.ntn;
  const int co0 = tn * BN, p0 = tm * BM;
  const int kc = tid & 3;
  const int HW = a.H * a.W;

  int rh[CA], rw[CA], rb[CA];
  bool rv[CA];
#pragma unroll
  for (int i = 0; i < CA; ++i) {
    const int pix = p0 + (tid >> 2) + i * (NT / 4);
    rv[i] = pix < a.P;
    const int n = pix / HW;
    const int rem = pix - n * HW;
    rh[i] = rem / a.W;
    rw[i] = rem - rh[i] * a.W;
    rb[i] = n * a.Hin * a.Win;
  }

  Chunk8<T> ra[CA], rbw[CB];
  unsigned okm = 0;
  int cur_ci = 0;

  auto gload = [&](int ks) {
    const int k = ks * BK + kc * 8;
    const bool kin = k < a.K;
    const int tap = k >> a.lgCin;
    const int ci = k & (a.Cin - 1);
    const int sdiv = S2 == 2 ? 1 + ((a.sub - 1) & 1) : KS;      // taps per row
    const int r = tap / sdiv, s = tap - (tap / sdiv) * sdiv;
    cur_ci = ci;
    okm = 0;
#pragma unroll
    for (int i = 0; i < CA; ++i) {
      const int hh = S2 == 2 ? rh[i] + r : (S2 == 1 ? 2 * rh[i] : rh[i]) + r - PAD;
      const int ww = S2 == 2 ? rw[i] + s : (S2 == 1 ? 2 * rw[i] : rw[i]) + s - PAD;
      bool ok = kin && rv[i];
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
        ra[i].load(x + ((long)(rb[i] + hs * a.Win + ws) << a.lgCin) + ci);
        okm |= 1u << i;
      } else {
        ra[i].zero();
      }
    }
#pragma unroll
    for (int j = 0; j < CB; ++j) {
      const int q = tid + j * NT;
      if (q < NBCH) rbw[j].load(wk + (long)(co0 + (q >> 2)) * a.Kpad + ks * BK + kc * 8);
    }
  };

  auto lstore = [&](int buf) {
    char* As = smem + buf * (BM + BN) * ROWB;
    char* Bs = As + BM * ROWB;
#pragma unroll
    for (int i = 0; i < CA; ++i) {
      const int row = (tid >> 2) + i * (NT / 4);
      Chunk8<T> c = ra[i];
      if constexpr (PRO) {
        if (okm & (1u << i)) {
          float f[8];
          const float4 s0 = *reinterpret_cast<const float4*>(a.psc + cur_ci);
          const float4 s1 = *reinterpret_cast<const float4*>(a.psc + cur_ci + 4);
          const float4 h0 = *reinterpret_cast<const float4*>(a.psh + cur_ci);
          const float4 h1 = *reinterpret_cast<const float4*>(a.psh + cur_ci + 4);
          const float sc[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
          const float sh[8] = {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w};
#pragma unroll
          for (int j = 0; j < 8; ++j) f[j] = fv_act(c.get(j) * sc[j] + sh[j], a.slope);
          c.set8(f);
        }
      }
      c.store(reinterpret_cast<T*>(As + row * ROWB + ((kc ^ rswz<T>(row)) * 8 * ES)));
    }
#pragma unroll
    for (int j = 0; j < CB; ++j) {
      const int q = tid + j * NT;
      if (q < NBCH) {
        const int row = q >> 2;
        rbw[j].store(reinterpret_cast<T*>(Bs + row * ROWB + ((kc ^ rswz<T>(row)) * 8 * ES)));
      }
    }
  };

  f32x4 acc[RN][RM];
#pragma unroll
  for (int n = 0; n < RN; ++n)
#pragma unroll
    for (int m = 0; m < RM; ++m) acc[n][m] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int lr = lane & 15, lh = lane >> 4;
  auto compute = [&](int buf) {
    const char* As = smem + buf * (BM + BN) * ROWB;
    const char* Bs = As + BM * ROWB;
    Frag<T> af[RN], bfm[RM];
#pragma unroll
    for (int n = 0; n < RN; ++n) {
      const int row = wn * RN * 16 + n * 16 + lr;
      af[n].lds(Bs + row * ROWB + ((lh ^ rswz<T>(row)) * 8 * ES));
    }
#pragma unroll
    for (int m = 0; m < RM; ++m) {
      const int row = wm * RM * 16 + m * 16 + lr;
      bfm[m].lds(As + row * ROWB + ((lh ^ rswz<T>(row)) * 8 * ES));
    }
#pragma unroll
    for (int n = 0; n < RN; ++n)
#pragma unroll
      for (int m = 0; m < RM; ++m) acc[n][m] = mma(af[n], bfm[m], acc[n][m]);
  };

  gload(0);
  lstore(0);
  __syncthreads();
  for (int ks = 0; ks < a.nks; ++ks) {
    const int cur = ks & 1;
    if (ks + 1 < a.nks) gload(ks + 1);
    compute(cur);
    if (ks + 1 < a.nks) lstore(cur ^ 1);
    __syncthreads();
  }

  conv_epilogue<T, WN, WM, RN, RM, false, NoMid, S2 == 2>(a, acc, smem, co0, p0, tm, wn, wm, lane, tid);
}

template <typename T, int KS, int WN, int WM, int RN, int RM>
int launch_fwd_t(const ConvArgs& a, int pro, int ups, int nblk, hipStream_t s) {
  dim3 g(nblk), b(64 * WN * WM);
  if (pro && ups) {
    if constexpr (KS == 3) hipLaunchKernelGGL((conv_fwd_kernel<T, KS, WN, WM, RN, RM, true, true>), g, b, 0, s, a);
    else return FV_E_UNSUPPORTED;
  } else if (pro) {
    if constexpr (KS != 7) hipLaunchKernelGGL((conv_fwd_kernel<T, KS, WN, WM, RN, RM, true, false>), g, b, 0, s, a);
    else return FV_E_UNSUPPORTED;
  } else if (ups) {
    if constexpr (KS == 3) hipLaunchKernelGGL((conv_fwd_kernel<T, KS, WN, WM, RN, RM, false, true>), g, b, 0, s, a);
    else return FV_E_UNSUPPORTED;
  } else {
    hipLaunchKernelGGL((conv_fwd_kernel<T, KS, WN, WM, RN, RM, false, false>), g, b, 0, s, a);
  }
  return FV_OK;
}

template <typename T, int KS>
int launch_fwd_ks(const ConvArgs& a, FwdTile t, int pro, int ups, int nblk, hipStream_t s) {
  if (t.bn == 128) return launch_fwd_t<T, KS, 2, 2, 4, 4>(a, pro, ups, nblk, s);
  if (t.bn == 64) return launch_fwd_t<T, KS, 2, 2, 2, 4>(a, pro, ups, nblk, s);
  if (t.bn == 32) return launch_fwd_t<T, KS, 2, 2, 1, 4>(a, pro, ups, nblk, s);
  return launch_fwd_t<T, KS, 1, 4, 1, 2>(a, pro, ups, nblk, s);
}

}  // namespace

template <typename T>
int launch_fwd(const ConvArgs& a, int ks, FwdTile t, int pro, int ups, int nblk, hipStream_t s) {
  switch (ks) {
    case 1: return launch_fwd_ks<T, 1>(a, t, pro, ups, nblk, s);
    case 3: return launch_fwd_ks<T, 3>(a, t, pro, ups, nblk, s);
    case 7: return launch_fwd_ks<T, 7>(a, t, pro, ups, nblk, s);
  }
  return FV_E_UNSUPPORTED;
}
template int launch_fwd<bf16>(const ConvArgs&, int, FwdTile, int, int, int, hipStream_t);
template int launch_fwd<float>(const ConvArgs&, int, FwdTile, int, int, int, hipStream_t);

// stride-2 3x3 conv on the generic kernels: forward (S2 = 1) / one data-gradient phase (S2 = 2)
template <typename T, int S2>
void launch_s2_fwd(const ConvArgs& a, FwdTile t, int nblk, hipStream_t s) {
  dim3 g(nblk);
  if (t.bn == 128) hipLaunchKernelGGL((conv_fwd_kernel<T, 3, 2, 2, 4, 4, false, false, S2>), g, dim3(256), 0, s, a);
  else if (t.bn == 64) hipLaunchKernelGGL((conv_fwd_kernel<T, 3, 2, 2, 2, 4, false, false, S2>), g, dim3(256), 0, s, a);
  else if (t.bn == 32) hipLaunchKernelGGL((conv_fwd_kernel<T, 3, 2, 2, 1, 4, false, false, S2>), g, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((conv_fwd_kernel<T, 3, 1, 4, 1, 2, false, false, S2>), g, dim3(256), 0, s, a);
}
template void launch_s2_fwd<bf16, 1>(const ConvArgs&, FwdTile, int, hipStream_t);
template void launch_s2_fwd<float, 1>(const ConvArgs&, FwdTile, int, hipStream_t);
template void launch_s2_fwd<bf16, 2>(const ConvArgs&, FwdTile, int, hipStream_t);
template void launch_s2_fwd<float, 2>(const ConvArgs&, FwdTile, int, hipStream_t);
