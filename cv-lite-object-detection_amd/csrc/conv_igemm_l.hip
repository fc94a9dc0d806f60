// Large-tile segmented implicit-GEMM convolution (forward / data-gradient) for gfx950.
//
// Same contract and math as conv_igemm.hip (see there; FCOS/fcos.py:6-110 Conv2D forward and
// backward-input), specialised for the launches that carry most of the step's FLOPs: the shared
// FCOS towers over all five FPN levels (M = 87,296 rows at bs 16, N = 256, K = 2,304), the FPN
// output convs and the wide ResNet stages — many M tiles, Npad % BN == 0, Cin % 64 == 0.
//
// Tile 256 x BN (128 or 64) x 64, 8 waves as 4 (M) x 2 (N), each a 64 x BN/2 block of
// v_mfma_f32_16x16x32_bf16 accumulators.  Both operands move global -> LDS by LDS-DMA
// (global_load_lds_dwordx4, 1 KiB lane-linear per wave-instruction; the XOR swizzle that keeps the
// ds_read_b128 fragment reads conflict-free is applied to the per-lane SOURCE address) through a
// 3-deep ring: tile k+2 is in flight while tile k is multiplied, the wait is a counted vmcnt (never
// 0 in steady state) and the barrier a raw s_barrier, so the DMA stays outstanding across it.
// Padding taps and rows past a segment's end read a 16-byte zero block.
#include "conv_common.h"
#include "conv_epilogue.h"

namespace {

constexpr int BM = 256;
constexpr int BK = 64;
constexpr int NT = 512;

__device__ __attribute__((aligned(16))) cvl_bf16 g_zero_l[8];

__device__ __forceinline__ int swz(int r) { return (r >> 1) & 7; }

__device__ __forceinline__ void glds16(const void* g, void* l) {
  __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1)))*)g,
                                   (void __attribute__((address_space(3)))*)l, 16, 0, 0);
}

// BN x WGM x NST: 128/64-wide tiles run 8 waves as 4 (M) x 2 (N) with a 3-deep ring; the
// 256-wide tile runs them as 2 x 4 (each wave 128 x 64: a quarter fewer LDS bytes per MFMA and
// half the DMA issues per FLOP) with a 2-deep ring (2 x 64 KiB).
// SW (round 5): swapped MFMA operands and conv_epilogue.h's register epilogue (sw_store: 16-B
// stores straight from the registers, BN statistics by DPP + one LDS combine) instead of the LDS C
// image; bf16 destination, no beta, no fused BN sums, tiles inside one image when statistics are on.
template <int BN, int WGM, int NST, bool DGRAD, bool PRIO, bool BSUM = false, bool SW = false>
__global__ void __launch_bounds__(NT) conv_igemm_l_kernel(ConvArgs a) {
  static_assert(!(SW && BSUM), "the fused BN sums keep the C-image epilogue");
  constexpr int WGN = 8 / WGM;
  constexpr int WM = BM / WGM, WN = BN / WGN;
  constexpr int TM = WM / 16, TN = WN / 16;
  constexpr int AP = BM * BK / (NT * 8);        // A pieces (16 B) per thread per K step: 4
  constexpr int BP = BN * BK / (NT * 8);        // B pieces per thread: 2 (BN 128) or 1 (BN 64)
  constexpr int GPW = AP + BP;                   // LDS-DMA instructions per wave per K step
  constexpr int STAGE = (BM + BN) * BK;          // bf16 elements per ring slot
  constexpr int LDS_C = BM * (BN + 8) + (WGM > 2 ? WGM * BN * 2 * 2 : 0);   // C image + per-wave stats
  constexpr int LDS_EL = SW ? NST * STAGE + WGM * BN * 4 : (NST * STAGE > LDS_C ? NST * STAGE : LDS_C);
  __shared__ __attribute__((aligned(16))) cvl_bf16 lds[LDS_EL];

  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  // 1-D grid, XCD-remapped: the N tiles of an M tile and neighbouring M tiles (3x3 halos) share
  // an XCD's L2
  const int ntn = a.Npad / BN;
  const int L = xcd_remap(blockIdx.x, gridDim.x);
  const int m_tile = L / ntn, n_tile = L % ntn;
  const int m0 = m_tile * BM, n0 = n_tile * BN;
  int sg = 0;
#pragma unroll
  for (int i = 1; i < kMaxSeg; ++i)
    if (i < a.nseg && m0 >= a.seg[i].m_start) sg = i;
  const ConvSeg& S = a.seg[sg];
  const int HWr = S.Hr * S.Wr;
  const int mloc0 = m0 - S.m_start;
  if (mloc0 >= S.rows) return;
  // z chunks of the fused BN-backward sums, fetched now so the main loop hides their latency
  s16x8 zpre[BnSumPre<BN, NT>::N];
  BnSumPar bpar;
  if constexpr (BSUM) bnsum_prefetch<BN, NT>(a, S, tid, n0, mloc0, zpre, bpar);

  // piece p of this thread: row p*64 + wave*8 + lane/8, chunk lane%8 (lane-linear 1 KiB image)
  const int prow = wave * 8 + (lane >> 3), ch = lane & 7;
  int a_img[AP], a_y[AP], a_x[AP];
  bool a_ok[AP];
#pragma unroll
  for (int p = 0; p < AP; ++p) {
    const int ml = mloc0 + p * 64 + prow;
    a_ok[p] = ml < S.rows;
    const int img = ml / HWr, q = ml - img * HWr;
    const int oy = q / S.Wr, ox = q - (q / S.Wr) * S.Wr;
    a_img[p] = img;
    if (DGRAD) { a_y[p] = oy + a.pad_t; a_x[p] = ox + a.pad_l; }
    else { a_y[p] = oy * a.stride - a.pad_t; a_x[p] = ox * a.stride - a.pad_l; }
  }
  const cvl_bf16* __restrict__ wsrc = S.w;
  const int Cin = a.Cin, KW = a.KW, Kdim = a.K, stride = a.stride;
  const int Hs = S.Hs, Ws = S.Ws;
  // per-piece source row pointers at tap (0, 0) (64-bit math once, 32-bit offsets in the loop)
  const cvl_bf16* a_base[AP];
#pragma unroll
  for (int p = 0; p < AP; ++p)
    a_base[p] = a.src + (S.src_base + (long)a_img[p] * S.src_img) * Cin + ((ch ^ swz(p * 64 + prow)) * 8);
  const cvl_bf16* b_base[BP];
#pragma unroll
  for (int p = 0; p < BP; ++p) {
    const int row = p * 64 + prow;
    b_base[p] = wsrc + (long)(n0 + row) * Kdim + ((ch ^ swz(row)) * 8);
  }

  auto issue = [&](int kt, int slot) {
    cvl_bf16* Ab = lds + slot * STAGE;
    cvl_bf16* Bb = Ab + BM * BK;
    const int k0 = kt * BK;
    const int tap = k0 / Cin;
    const int cb = k0 - tap * Cin;
    const int r = tap / KW, s = tap - (tap / KW) * KW;
#pragma unroll
    for (int p = 0; p < AP; ++p) {
      int iy, ix;
      bool ok = a_ok[p];
      if (DGRAD) {
        const int ty = a_y[p] - r, tx = a_x[p] - s;
        if (stride == 1) {
          iy = ty; ix = tx;
        } else {
          ok = ok && ty >= 0 && tx >= 0 && (ty % stride) == 0 && (tx % stride) == 0;
          iy = ty / stride; ix = tx / stride;
        }
      } else {
        iy = a_y[p] + r; ix = a_x[p] + s;
      }
      ok = ok && iy >= 0 && ix >= 0 && iy < Hs && ix < Ws;
      const int off = (iy * Ws + ix) * Cin + cb;
      const cvl_bf16* g = ok ? a_base[p] + off : g_zero_l;
      glds16(g, Ab + (p * 64 + wave * 8) * BK);
    }
#pragma unroll
    for (int p = 0; p < BP; ++p) glds16(b_base[p] + k0, Bb + (p * 64 + wave * 8) * BK);
  };

  const int wm = wave / WGN, wn = wave % WGN;
  const int lr = lane & 15, lg = lane >> 4;
  // the epilogue's bias, in flight under the main loop (the 256-wide form runs at the register
  // limit and loads it in the epilogue)
  float bcol[TN];
  float bq[SW ? TN : 1][4];
  if constexpr (SW) sw_bias<TN>(a, S, n0 + wn * WN, lg, bq);
  else if constexpr (BN <= 128) epi_bias<BN, WGM, TN>(a, S, n0, wn, lane, bcol);
  f32x4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nk = a.K / BK;
#pragma unroll
  for (int t = 0; t < NST - 1; ++t)
    if (t < nk) issue(t, t);
  int slot = 0;
  for (int kt = 0; kt < nk; ++kt) {
    // tile kt landed (this wave's DMA; with a 3-deep ring tile kt+1 may stay in flight), then
    // every wave's
    if (NST == 3 && kt + 1 < nk) wait_vm<GPW>();
    else wait_vm<0>();
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (kt + NST - 1 < nk) issue(kt + NST - 1, slot == 0 ? NST - 1 : slot - 1);   // slot read in step kt-1
    const cvl_bf16* Ac = lds + slot * STAGE;
    const cvl_bf16* Bc = Ac + BM * BK;
#pragma unroll
    for (int ks = 0; ks < BK / 32; ++ks) {
      const int chunk = ks * 4 + lg;
      s16x8 fa[TM], fb[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int r = wm * WM + i * 16 + lr;
        fa[i] = *reinterpret_cast<const s16x8*>(Ac + r * BK + ((chunk ^ swz(r)) * 8));
      }
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int r = wn * WN + j * 16 + lr;
        fb[j] = *reinterpret_cast<const s16x8*>(Bc + r * BK + ((chunk ^ swz(r)) * 8));
      }
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          acc[i][j] = SW ? __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, fb[j]),
                                                                    __builtin_bit_cast(bf16x8, fa[i]), acc[i][j], 0, 0, 0)
                         : __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, fa[i]),
                                                                    __builtin_bit_cast(bf16x8, fb[j]), acc[i][j], 0, 0, 0);
          if (PRIO && i == 0 && j == 0) {            // keep the MFMA cluster together (T5)
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_setprio(1);
            __builtin_amdgcn_sched_barrier(0);
          }
        }
      if (PRIO) {
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    asm volatile("" ::: "memory");
    slot = slot == NST - 1 ? 0 : slot + 1;
  }

  if constexpr (SW) {
    float ss1[TN][4], ss2[TN][4];
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) { ss1[j][e] = 0.f; ss2[j][e] = 0.f; }
    if (a.stats) {
      sw_store<TM, TN, true>(a, S, acc, bq, mloc0 + wm * WM, n0 + wn * WN, HWr, lane, ss1, ss2);
      sw_flush_stats<BN, WGM, TN>(a, reinterpret_cast<float*>(lds + NST * STAGE), tid, wm, wn * WN, mloc0 / HWr, n0,
                                  ss1, ss2);
    } else {
      sw_store<TM, TN, false>(a, S, acc, bq, mloc0 + wm * WM, n0 + wn * WN, HWr, lane, ss1, ss2);
    }
    return;
  }
  conv_l_epilogue<BN, WGM, TM, TN, NT, BSUM>(a, S, acc, lds, tid, wm, wn, n0, mloc0, HWr, zpre, bpar,
                                              BN <= 128 ? bcol : nullptr);
}

// The variants of one tile shape.  (Plain `if`s: the 256-wide SW and fused-sums forms are never
// planned, but stay instantiated as they always were.)
template <int BN_, int WGM_, int NST_>
void l_launch(const ConvPlan& p, const ConvArgs& a, hipStream_t s) {
  const dim3 grid(p.grid);
  if (p.sw && BN_ <= 128) {
    with_bool(p.dgrad, [&](auto DG) {
      hipLaunchKernelGGL((conv_igemm_l_kernel<BN_, WGM_, NST_, decltype(DG)::value, true, false, true>), grid, dim3(NT),
                         0, s, a);
    });
  } else if (p.dgrad && p.bsum) {
    hipLaunchKernelGGL((conv_igemm_l_kernel<BN_, WGM_, NST_, true, true, true>), grid, dim3(NT), 0, s, a);
  } else {
    with_bool(p.dgrad, [&](auto DG) {
      with_bool(p.prio, [&](auto PRIO) {
        hipLaunchKernelGGL((conv_igemm_l_kernel<BN_, WGM_, NST_, decltype(DG)::value, decltype(PRIO)::value>), grid,
                           dim3(NT), 0, s, a);
      });
    });
  }
}

}  // namespace

// Launches the L kernel the plan names (CVL_CK_L256 / L128 / L64).
int launch_l(const ConvPlan& p, const ConvArgs& a, hipStream_t s) {
  if (p.bn == 256) l_launch<256, 2, 2>(p, a, s);
  else if (p.bn == 128) l_launch<128, 4, 3>(p, a, s);
  else l_launch<64, 4, 3>(p, a, s);
  return cvl_launch_status();
}
