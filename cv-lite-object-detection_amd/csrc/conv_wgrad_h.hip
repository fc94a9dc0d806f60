// WH: 3x3 / stride 1 / pad 1 convolution WEIGHT gradient with the source staged as an LDS halo
// (gfx950, bf16 MFMA, fp32 accumulation) -- the Conv2DBackpropFilter + per-image gradient sum of
// FCOS/train_fcos.py:173-176 for the ResNet-50 3x3 units (Keras ResNet50 behind fcos.py:30-46) and
// the FPN 3x3 convs on maps of width 16..128:
//   dW[(r, s, c), co] = sum over the rows m (output pixels) of  X[m shifted by (r-1, s-1), c] * dY[m, co]
// The generic kernels stage nine shifted im2col tiles per 32-row step; here a 128-row step (whole
// image rows) stages its source pixels ONCE as a halo (rows y0-1 .. y0+R, W+2 pixels wide) and the
// nine taps read it at pixel offsets: 67 LDS-DMA pieces per 1,152 MFMAs (0.06 per MFMA).
// * Workgroup = (64 input channels) x (64 output channels) x all 9 taps = a 64 x 576 C tile, over a
//   chunk of 128-row steps; 8 waves as 2 (co halves) x 4 (16-channel quarters), each wave
//   2 x 9 v_mfma_f32_16x16x32_bf16 accumulators (co tile x tap).
// * Stage = halo [<= 432 px][64 ch] + dY [128 rows][64 co], 128-B rows, double-buffered (140 KiB).
//   A step is four 32-row sub-steps of 18 MFMAs per wave.  The step loop has two forms that run
//   the same MFMAs on the same operands in the same order (wh_loop_reads, the default, and
//   wh_loop_first, CVL_DISPATCH=wh_reads=0): see there for the schedule of reads, DMA and barriers.
// * Fragments by ds_read_b64_tr_b16 (the reduction index is the LDS row index): dY^T (co) is the
//   MFMA A operand, the shifted X^T (channels) the B operand.  16-B chunks are XOR-swizzled by
//   bits 1 and 3 of the pixel / row index (applied to the per-lane DMA SOURCE offset), which keeps
//   every 32-lane transposed read conflict-free under any tap shift.
// * Chunks of steps are spread over workgroups to fill the GPU; partial tiles go to fp32 slabs
//   summed in a fixed order (deterministic), or straight into dW (with beta) for one chunk.
#include <type_traits>
#include <utility>

#include "conv_common.h"

namespace {

constexpr int NT = 512, BCI = 64, BCO = 64, RS = 128;
constexpr int HPX = 448;                             // halo pixels per stage (W = 128: 3 x 144 used)
constexpr int HPW = HPX / 8 / 8;                     // halo DMA pieces (8 pixels each) per wave: 7
constexpr int HALO_B = HPX * 128;                    // bytes
constexpr int DY_B = RS * 128;
constexpr int STAGE_B = HALO_B + DY_B;               // 73,728 B
constexpr unsigned kOOB = 0x80000000u;

__device__ __forceinline__ int swz8(int p) { return ((((p >> 1) & 1) | (((p >> 3) & 1) << 1)) << 1); }

__device__ __forceinline__ void dma16(__amdgpu_buffer_rsrc_t r, const void* lds_dst, unsigned voff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (__attribute__((address_space(3))) void*)lds_dst, 16, (int)voff, 0,
                                           0, 0);
}


struct WhArgs {
  const cvl_bf16* x;
  const cvl_bf16* dy;
  float* out;                 // slab [nsplit][K][Cout] or dW (direct)
  long src_base, src_img, dst_base, dst_img;
  int B, H, W, Cin, Cout, ld_dy, dy_coff;
  int ci_tiles, co_tiles, steps, chunk, nsplit, direct;
  float beta;
};

// Batched form (round 6, cvl_conv_wgrad_batch): the 3x3 weight gradients of a ResNet stage's
// units in ONE launch; workgroup L (after the XCD remap) works on the problem whose [wg0, wg0 +
// tiles * nsplit) range holds it, with that problem's own arguments.
constexpr int kMaxWhProb = kWgHMaxProb;
struct WhBatch {
  WhArgs p[kMaxWhProb];
  int wg0[kMaxWhProb];
  int n;
};

// The first form of the step loop (CVL_DISPATCH=wh_reads=0).  Two phases per step (2 x 32-row
// sub-steps, 36 MFMAs per wave each); a phase's 44 fragment reads are all issued before the barrier
// that opens its MFMA segment; the wave groups (channel quarters 0-1 / 2-3) run one barrier apart;
// step s+1 is issued in phase 0 of step s into the buffer step s-1 used and waited for (vmcnt 0) at
// the start of phase 1.
__device__ __forceinline__ void wh_loop_first(const WhArgs& g, char* lds, int wave, int lane, int ci0, int co0, int s0,
                                              int s1, f32x4 (&acc)[2][9]) {
  const int W = g.W, H = g.H, HW = H * W;
  const int R = RS / W;                                // image rows per step
  const int P = (W + 2 + 15) & ~15;                    // halo pitch (pixels; % 16: a row shift keeps the swizzle)
  const int hpx = (R + 2) * P;
  const int ch = lane & 7;
  const int Cin2 = g.Cin * 2;

  // DMA pieces of this lane, straight-line per step: halo pieces k = wave + 8 j (j < HPW: halo
  // pixels 8k + lane / 8, chunk lane % 8; those past the halo write zeros into its tail), dY pieces
  // k = wave + 8 j (j < 2: rows 8k + lane / 8 of the step).  Per lane the halo pixel's row hy and
  // its offset relative to the step's first pixel are fixed; a step only adds its base and
  // checks its top / bottom image rows.
  int hy[HPW];
  bool hok[HPW];
  unsigned hlo[HPW], ylo[2];
#pragma unroll
  for (int j = 0; j < HPW; ++j) {
    const int hp = 8 * (wave + 8 * j) + (lane >> 3);
    const int y = hp / P, x = hp - y * P;
    hy[j] = y;
    hok[j] = hp < hpx && x >= 1 && x <= W;
    hlo[j] = (unsigned)(((y - 1) * W + (x - 1)) * Cin2 + ci0 * 2) + (unsigned)((ch ^ swz8(hp)) * 16);
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int m = 8 * (wave + 8 * j) + (lane >> 3);
    ylo[j] = (unsigned)((m * g.ld_dy + g.dy_coff + co0) * 2) + (unsigned)((ch ^ swz8(m)) * 16);
  }
  const __amdgpu_buffer_rsrc_t rsX = __builtin_amdgcn_make_buffer_rsrc((void*)g.x, (short)0, (int)kConvBufRecords, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsY = __builtin_amdgcn_make_buffer_rsrc((void*)g.dy, (short)0, (int)kConvBufRecords, 0x00020000);

  auto issue = [&](int s) {
    if (s >= s1) return;
    char* st = lds + (s & 1) * STAGE_B;
    const int m0 = s * RS;
    const int img = m0 / HW;
    const int y0 = (m0 - img * HW) / W;
    const unsigned xb = (unsigned)((g.src_base + (long)img * g.src_img + (long)y0 * W) * Cin2);
    const unsigned yb = (unsigned)((g.dst_base + (long)img * g.dst_img + (long)y0 * W) * g.ld_dy * 2);
    const bool top = y0 == 0, bot = y0 + R == H;
#pragma unroll
    for (int j = 0; j < HPW; ++j) {
      const bool ok = hok[j] && !(top && hy[j] == 0) && !(bot && hy[j] == R + 1);
      dma16(rsX, st + (wave + 8 * j) * 1024, ok ? xb + hlo[j] : kOOB);
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) dma16(rsY, st + HALO_B + (wave + 8 * j) * 1024, yb + ylo[j]);
  };

  const int wco = wave & 1, wk = wave >> 1, grp = wave >> 2;
  const int lr = lane & 15, lg = lane >> 4;
  const int q = lr >> 2, p = lr & 3;
  // per-lane transposed-read byte offsets (within a stage) for the rows of sub-step u (0..3):
  // lo = row 32u + 8lg + q, hi = lo + 4.  dY: co tile i; X: halo pixel of the row at dx = s
  // (the dy = r shift adds r * P * 128 bytes, which keeps the swizzle: P % 16 == 0)
  unsigned yof[4][2][2], xof[4][2][3];
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int m = 32 * u + 8 * lg + q + 4 * h;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int c16 = (wco * 32 + i * 16) / 8 + (p >> 1);     // 16-B chunk of the co column
        yof[u][h][i] = (unsigned)(HALO_B + m * 128 + ((c16 ^ swz8(m)) * 16) + (p & 1) * 8);
      }
      const int oy = m / W, ox = m - (m / W) * W;
      const int c16 = (wk * 16) / 8 + (p >> 1);
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        const int hp = oy * P + ox + s;
        xof[u][h][s] = (unsigned)(hp * 128 + ((c16 ^ swz8(hp)) * 16) + (p & 1) * 8);
      }
    }
  const unsigned rowb = (unsigned)(P * 128);

  auto bar = [&]() {
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  };
  const unsigned lds0 = lds_addr(lds);

  issue(s0);
  wait_vm<0>();
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  if (grp == 1) bar();            // stagger: waves 4-7 run one barrier behind

  for (int s = s0; s < s1; ++s) {
    const unsigned sb = lds0 + (unsigned)((s & 1) * STAGE_B);
    // both phases unrolled: the per-sub-step offset tables must stay in registers
#pragma unroll
    for (int ph = 0; ph < 2; ++ph) {
      if (ph == 0) issue(s + 1);
      else wait_vm<0>();                       // this wave's pieces of step s + 1 landed
      // transposed reads as inline asm (conv_common.h ds_tr16: the builtin would make the compiler
      // drain the in-flight DMA of step s + 1 before every read); pinned after the lgkmcnt wait
      s16x4 ylo[2][2], yhi[2][2], xlo[2][9], xhi[2][9];
#pragma unroll
      for (int uu = 0; uu < 2; ++uu) {
        const int u = 2 * ph + uu;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          ylo[uu][i] = ds_tr16(sb + yof[u][0][i]);
          yhi[uu][i] = ds_tr16(sb + yof[u][1][i]);
        }
#pragma unroll
        for (int t = 0; t < 9; ++t) {
          const int r = t / 3, c = t - 3 * (t / 3);
          xlo[uu][t] = ds_tr16(sb + xof[u][0][c] + r * rowb);
          xhi[uu][t] = ds_tr16(sb + xof[u][1][c] + r * rowb);
        }
      }
      bar();
      lgkm_wait();
#pragma unroll
      for (int uu = 0; uu < 2; ++uu) {
#pragma unroll
        for (int i = 0; i < 2; ++i) { tr_pin(ylo[uu][i]); tr_pin(yhi[uu][i]); }
#pragma unroll
        for (int t = 0; t < 9; ++t) { tr_pin(xlo[uu][t]); tr_pin(xhi[uu][t]); }
      }
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int uu = 0; uu < 2; ++uu)
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
          for (int i = 0; i < 2; ++i)
            acc[i][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                __builtin_bit_cast(bf16x8, tr_join(ylo[uu][i], yhi[uu][i])),
                __builtin_bit_cast(bf16x8, tr_join(xlo[uu][t], xhi[uu][t])), acc[i][t], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
      __builtin_amdgcn_sched_barrier(0);
      bar();
    }
  }
  if (grp == 0) bar();            // equal barrier counts for both groups
}

// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>): the index is a constant
// expression inside f (the reads' offset fields, the fragment registers)
template <class F, int... I>
__device__ __forceinline__ void static_for_(F&& f, std::integer_sequence<int, I...>) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  static_for_(f, std::make_integer_sequence<int, N>{});
}

// The geometry of a map width W (16 / 32 / 64 / 128: halo pitches 32 / 48 / 80 / 144): with it a
// compile-time constant every fragment read that differs from another by a lane-uniform shift is
// that read's address plus an immediate.
template <int W>
struct WhGeo {
  static constexpr int R = RS / W;                     // image rows per step
  static constexpr int P = (W + 2 + 15) & ~15;         // halo pitch (pixels)
  static constexpr int ROWB = P * 128;                 // a tap-row shift (bytes); P % 16 == 0 keeps the swizzle
  // halo byte shift of sub-step u's rows (32 u rows further: whole image rows and / or a multiple
  // of 32 pixels along the row, so the swizzle is kept too)
  static constexpr int xsh(int u) { return ((32 * u / W) * P + (32 * u) % W) * 128; }
  static_assert(xsh(3) + 2 * ROWB + 512 < 65536, "ds offset field");
};
constexpr int kSubReads = 22, kSubMfma = 18;           // per wave and 32-row sub-step
// Read r of the next sub-step goes into the gap after MFMA kReadGap(r) of this one: two reads in each
// of the first kTwoGaps gaps, one in the following ones, none behind the last MFMAs (their latency
// is covered by those).  DMA piece j of step s+2 goes into gap kDmaGap0 + j of a step's last sub-step.
constexpr int kTwoGaps = 6, kDmaGap0 = 6;
static_assert(kSubReads - kTwoGaps <= kSubMfma && kDmaGap0 + HPW + 2 <= kSubMfma, "gaps");

// The pipelined form of the step loop (the default).  A step is four 32-row sub-steps of 18 MFMAs
// per wave; while sub-step u's MFMAs issue, the wave reads sub-step u+1's 22 fragments into the
// other register set, in the MFMA gaps (across a step boundary: from the other stage buffer).  One
// barrier per step, in front of its last sub-step: there every wave has its reads of step s complete
// (lgkmcnt 0: the last ones were issued under sub-step 2) and its own pieces of step s+1 landed
// (vmcnt 0; they were issued a whole step earlier), so behind it step s+2 is issued into step s's
// buffer and step s+1's first fragments are read.  No wave-group stagger: both waves of a SIMD
// stream MFMAs all the time.  Every accumulator sees the same sub-steps in the same order as in the
// first form, so both write the same bits.
template <int W>
__device__ __forceinline__ void wh_loop_reads(const WhArgs& g, char* lds, int wave, int lane, int ci0, int co0, int s0,
                                              int s1, f32x4 (&acc)[2][9]) {
  using G = WhGeo<W>;
  constexpr int R = G::R, P = G::P, hpx = (R + 2) * P;
  const int H = g.H, HW = H * W;
  const int ch = lane & 7;
  const int Cin2 = g.Cin * 2;

  // DMA pieces of this lane (as in the first form): byte offset relative to the step's first pixel,
  // kOOB for a piece that is never fetched (halo padding columns, the stage's tail: zeros), and
  // which step kinds drop it: bit 0 a top step (halo row 0), bit 1 a bottom step (halo row R + 1),
  // bit 2 a step past the chunk's end.
  unsigned hlo[HPW], hfl[HPW], ylo[2];
#pragma unroll
  for (int j = 0; j < HPW; ++j) {
    const int hp = 8 * (wave + 8 * j) + (lane >> 3);
    const int y = hp / P, x = hp - y * P;
    const bool ok = hp < hpx && x >= 1 && x <= W;
    hlo[j] = ok ? (unsigned)(((y - 1) * W + (x - 1)) * Cin2 + ci0 * 2) + (unsigned)((ch ^ swz8(hp)) * 16) : kOOB;
    hfl[j] = ok ? 4u | (y == 0 ? 1u : 0u) | (y == R + 1 ? 2u : 0u) : 0u;
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int m = 8 * (wave + 8 * j) + (lane >> 3);
    ylo[j] = (unsigned)((m * g.ld_dy + g.dy_coff + co0) * 2) + (unsigned)((ch ^ swz8(m)) * 16);
  }
  const __amdgpu_buffer_rsrc_t rsX = __builtin_amdgcn_make_buffer_rsrc((void*)g.x, (short)0, (int)kConvBufRecords, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsY = __builtin_amdgcn_make_buffer_rsrc((void*)g.dy, (short)0, (int)kConvBufRecords, 0x00020000);

  // issue cursor: the next step to issue, its first image row and its two base offsets, advanced
  // by adds (a step is R whole image rows and never straddles an image)
  int cs = s0, cy;
  unsigned cxb, cyb;
  {
    const int m0 = s0 * RS;
    const int img = m0 / HW;
    cy = (m0 - img * HW) / W;
    cxb = (unsigned)((g.src_base + (long)img * g.src_img + (long)cy * W) * Cin2);
    cyb = (unsigned)((g.dst_base + (long)img * g.dst_img + (long)cy * W) * g.ld_dy * 2);
  }
  const unsigned dxb = (unsigned)(RS * Cin2), dyb = (unsigned)(RS * g.ld_dy * 2);
  const unsigned dxq = (unsigned)((g.src_img - HW) * Cin2), dyq = (unsigned)((g.dst_img - HW) * g.ld_dy * 2);
  unsigned vo[HPW + 2];                                // the buffer offsets of the step's pieces
  char* vst = lds;                                     // ... and its stage
  auto offsets = [&]() __attribute__((always_inline)) {
    const bool live = cs < s1;
    const unsigned drop = live ? (cy == 0 ? 1u : 0u) | (cy + R == H ? 2u : 0u) : 7u;
#pragma unroll
    for (int j = 0; j < HPW; ++j) vo[j] = (hfl[j] & drop) ? kOOB : cxb + hlo[j];
    const unsigned yb = live ? cyb : kOOB;
#pragma unroll
    for (int j = 0; j < 2; ++j) vo[HPW + j] = yb + ylo[j];
    vst = lds + (cs & 1) * STAGE_B;
    ++cs;
    cy += R;
    const bool wrap = cy == H;
    cy = wrap ? 0 : cy;
    cxb += dxb + (wrap ? dxq : 0u);
    cyb += dyb + (wrap ? dyq : 0u);
  };
  auto put = [&](int j) __attribute__((always_inline)) {
    if (j < HPW) dma16(rsX, vst + (wave + 8 * j) * 1024, vo[j]);
    else dma16(rsY, vst + HALO_B + (wave + 8 * (j - HPW)) * 1024, vo[j]);
  };

  const int wco = wave & 1, wk = wave >> 1;
  const int lr = lane & 15, lg = lane >> 4;
  const int q = lr >> 2, p = lr & 3;
  // Fragment read addresses of sub-step 0 in the stage being read: row m = 8 lg + q (lo; hi = m + 4).
  // dY: co tile i; hi is 4 rows = 512 B on (swz8 ignores bit 2), sub-step u 4096 u B on.  X: the
  // row's halo pixel at tap column c; hi is 4 pixels on, which keeps the swizzle where bits 0-3 of
  // the pixel do not carry into bit 3: always at c = 0 (q + 4 < 8), not for every lane at c = 1, 2,
  // which get an address each (xa[1], xa[2] and xa[3], xa[4]).  Tap row r and sub-step u are immediates.
  unsigned ya[2], xa[5];
  {
    const unsigned lds0 = lds_addr(lds) + (unsigned)((s0 & 1) * STAGE_B);
    const int m = 8 * lg + q;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c16 = (wco * 32 + i * 16) / 8 + (p >> 1);       // 16-B chunk of the co column
      ya[i] = lds0 + (unsigned)(HALO_B + m * 128 + ((c16 ^ swz8(m)) * 16) + (p & 1) * 8);
    }
    const int c16 = (wk * 16) / 8 + (p >> 1);
    auto xaddr = [&](int c, int h) {
      const int hp = (m / W) * P + m % W + 4 * h + c;
      return lds0 + (unsigned)(hp * 128 + ((c16 ^ swz8(hp)) * 16) + (p & 1) * 8);
    };
    xa[0] = xaddr(0, 0);
    xa[1] = xaddr(1, 0); xa[2] = xaddr(1, 1);
    xa[3] = xaddr(2, 0); xa[4] = xaddr(2, 1);
  }
  unsigned flip = (unsigned)((s0 & 1) ? -STAGE_B : STAGE_B);   // to the other stage

  s16x4 fy[2][2][2], fx[2][9][2];                      // [register set][co tile / tap][lo, hi]
  // read r of sub-step UN (within its step) into set S: the four dY reads, then the taps' (lo, hi)
  auto read = [&](auto UN_, auto S_, auto R_) __attribute__((always_inline)) {
    constexpr int un = decltype(UN_)::value, S = decltype(S_)::value, r = decltype(R_)::value;
    if constexpr (r < 4) {
      constexpr int i = r >> 1, h = r & 1;
      fy[S][i][h] = ds_tr16o<4096 * un + 512 * h>(ya[i]);
    } else {
      constexpr int t = (r - 4) >> 1, h = (r - 4) & 1, c = t % 3;
      constexpr int off = G::xsh(un) + (t / 3) * G::ROWB;
      if constexpr (c == 0) fx[S][t][h] = ds_tr16o<off + 512 * h>(xa[0]);
      else fx[S][t][h] = ds_tr16o<off>(xa[2 * c - 1 + h]);
    }
  };
  auto bar = [&]() __attribute__((always_inline)) {
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  };
  // sub-step U of a step: its MFMAs on set U & 1, the next sub-step's reads in their gaps
  auto sub = [&](auto U_) __attribute__((always_inline)) {
    constexpr int U = decltype(U_)::value, S = U & 1;
    lgkm_wait();                                       // this sub-step's fragments
    if constexpr (U == 3) {
#pragma unroll
      for (int i = 0; i < 2; ++i) ya[i] += flip;
#pragma unroll
      for (int i = 0; i < 5; ++i) xa[i] += flip;
      flip = 0u - flip;
      offsets();                                       // step s + 2: formed outside the MFMA stream
      __builtin_amdgcn_sched_barrier(0);               // ... on this side of the barrier
      wait_vm<0>();                                    // this wave's pieces of step s + 1
      bar();
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) { tr_pin(fy[S][i][0]); tr_pin(fy[S][i][1]); }
#pragma unroll
    for (int t = 0; t < 9; ++t) { tr_pin(fx[S][t][0]); tr_pin(fx[S][t][1]); }
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(1);
    static_for<kSubMfma>([&](auto K_) __attribute__((always_inline)) {
      constexpr int k = decltype(K_)::value, t = k >> 1, i = k & 1;
      acc[i][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          __builtin_bit_cast(bf16x8, tr_join(fy[S][i][0], fy[S][i][1])),
          __builtin_bit_cast(bf16x8, tr_join(fx[S][t][0], fx[S][t][1])), acc[i][t], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      constexpr int r0 = k < kTwoGaps ? 2 * k : k + kTwoGaps, nr = k < kTwoGaps ? 2 : 1;
      using UN = std::integral_constant<int, (U + 1) & 3>;
      using SN = std::integral_constant<int, S ^ 1>;
      if constexpr (r0 < kSubReads) read(UN{}, SN{}, std::integral_constant<int, r0>{});
      if constexpr (nr == 2 && r0 + 1 < kSubReads) read(UN{}, SN{}, std::integral_constant<int, r0 + 1>{});
      if constexpr (U == 3 && k >= kDmaGap0 && k < kDmaGap0 + HPW + 2) put(k - kDmaGap0);
      __builtin_amdgcn_sched_barrier(0);
    });
    __builtin_amdgcn_s_setprio(0);
  };

  // steps s0 and s0 + 1 issued; s0's pieces of every wave landed; its first fragments read
  offsets();
#pragma unroll
  for (int j = 0; j < HPW + 2; ++j) put(j);
  offsets();
#pragma unroll
  for (int j = 0; j < HPW + 2; ++j) put(j);
  wait_vm<HPW + 2>();
  bar();
  static_for<kSubReads>([&](auto R_) __attribute__((always_inline)) {
    read(std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{}, R_);
  });
  __builtin_amdgcn_sched_barrier(0);
  for (int s = s0; s < s1; ++s) {
    sub(std::integral_constant<int, 0>{});
    sub(std::integral_constant<int, 1>{});
    sub(std::integral_constant<int, 2>{});
    sub(std::integral_constant<int, 3>{});
  }
  // the last sub-step read fragments of a step past the end (nothing uses them): landed before the
  // epilogue takes their registers
  lgkm_wait();
#pragma unroll
  for (int i = 0; i < 2; ++i) { tr_pin(fy[0][i][0]); tr_pin(fy[0][i][1]); }
#pragma unroll
  for (int t = 0; t < 9; ++t) { tr_pin(fx[0][t][0]); tr_pin(fx[0][t][1]); }
  __builtin_amdgcn_sched_barrier(0);
}

// RD: the step loop, 0 the first form, 1 the pipelined one
template <typename Args, int RD>
__global__ void __launch_bounds__(NT) conv_wgrad_h_kernel(Args ga) {
  __shared__ __attribute__((aligned(16))) char lds[2 * STAGE_B];
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  int L = xcd_remap(blockIdx.x, gridDim.x);
  WhArgs g;
  if constexpr (std::is_same<Args, WhBatch>::value) {
    int pi = 0;
#pragma unroll
    for (int i = 1; i < kMaxWhProb; ++i)
      if (i < ga.n && L >= ga.wg0[i]) pi = i;
    L -= ga.wg0[pi];
    g = ga.p[pi];
  } else {
    g = ga;
  }
  const int tiles = g.ci_tiles * g.co_tiles;
  const int tile = L % tiles, split = L / tiles;      // the tiles of one chunk share an XCD's L2
  const int ci0 = (tile % g.ci_tiles) * BCI, co0 = (tile / g.ci_tiles) * BCO;
  const int s0 = split * g.chunk, s1 = min(s0 + g.chunk, g.steps);
  const int wco = wave & 1, wk = wave >> 1;
  const int lr = lane & 15, lg = lane >> 4;

  f32x4 acc[2][9];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[i][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  if constexpr (RD == 0) {
    wh_loop_first(g, lds, wave, lane, ci0, co0, s0, s1, acc);
  } else {
    // (workgroup-uniform: a batched launch mixes widths)
    if (g.W == 128) wh_loop_reads<128>(g, lds, wave, lane, ci0, co0, s0, s1, acc);
    else if (g.W == 64) wh_loop_reads<64>(g, lds, wave, lane, ci0, co0, s0, s1, acc);
    else if (g.W == 32) wh_loop_reads<32>(g, lds, wave, lane, ci0, co0, s0, s1, acc);
    else wh_loop_reads<16>(g, lds, wave, lane, ci0, co0, s0, s1, acc);
  }
  wait_vm<0>();
  // C[co][k] -> out[k][co] (HWIO), 4 consecutive co per lane
  const long K = 9L * g.Cin;
  float* out = g.direct ? g.out : g.out + (size_t)split * K * g.Cout;
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const long k = (long)t * g.Cin + ci0 + wk * 16 + lr;
      const int co = co0 + wco * 32 + i * 16 + 4 * lg;
      f32x4 v = acc[i][t];
      f32x4* po = reinterpret_cast<f32x4*>(out + k * g.Cout + co);
      if (g.direct && g.beta != 0.f) v += g.beta * *po;
      *po = v;
    }
}


// one problem's kernel arguments but the pointers and beta: its 128-row steps in chunks of `chunk`
void wh_args(const cvl_conv_desc& d, int chunk, int nsplit, WhArgs* g) {
  const cvl_conv_seg& q = d.seg[0];
  g->src_base = q.src_base; g->src_img = q.src_img; g->dst_base = q.dst_base; g->dst_img = q.dst_img;
  g->B = d.B; g->H = q.Hr; g->W = q.Wr; g->Cin = d.Cin; g->Cout = d.n_store;
  g->ld_dy = d.ld_dst; g->dy_coff = d.dst_coff;
  g->ci_tiles = d.Cin / BCI; g->co_tiles = d.n_store / BCO;
  g->steps = d.B * q.Hr * q.Wr / RS;
  g->chunk = chunk; g->nsplit = nsplit;
  g->direct = nsplit == 1;
}

}  // namespace

// What the halo kernel can run: bf16, 3x3 / stride 1 / pad 1, one dense segment of whole 128-row
// steps (map width 16 .. 128 dividing 128), 64-channel tiles on both sides, a halo that fits its
// LDS stage, 32-bit buffer offsets.
bool wg_h_fits(const cvl_conv_desc* d) {
  if (d->nseg != 1 || d->mode != CVL_CONV_FWD) return false;
  if (d->prec != CVL_PREC_BF16 || d->KH != 3 || d->KW != 3 || d->stride != 1 || d->pad_t != 1 || d->pad_l != 1 ||
      d->relu_in || d->Cin % BCI || d->n_store % BCO || d->ld_dst % 8 || d->dst_coff % 8)
    return false;
  const cvl_conv_seg& q = d->seg[0];
  const int W = q.Wr, HW = q.Hr * q.Wr;
  if (q.Hr != q.Hs || q.Wr != q.Ws || W < 16 || RS % W || HW % RS || q.src_img != HW || q.dst_img < HW) return false;
  if ((RS / W + 2) * ((W + 2 + 15) & ~15) > HPX) return false;
  const long src_end = (q.src_base + (long)d->B * q.src_img) * d->Cin * 2;
  const long dy_end = (q.dst_base + (long)d->B * q.dst_img) * d->ld_dst * 2;
  return src_end < (long)kConvBufRecords - 65536 && dy_end < (long)kConvBufRecords - 65536;
}

int launch_wg_h(const WgLaunch& l, const cvl_conv_desc& d, const void* x, const void* dy, float* const* dw, float beta,
                void* ws, hipStream_t s) {
  WhArgs g;
  wh_args(d, l.chunk, l.nsplit, &g);
  g.x = reinterpret_cast<const cvl_bf16*>(x);
  g.dy = reinterpret_cast<const cvl_bf16*>(dy);
  g.beta = beta;
  g.out = g.direct ? dw[0] : reinterpret_cast<float*>(ws);
  const dim3 grid(g.ci_tiles * g.co_tiles * l.nsplit);
  if (l.reads) hipLaunchKernelGGL((conv_wgrad_h_kernel<WhArgs, 1>), grid, dim3(NT), 0, s, g);
  else hipLaunchKernelGGL((conv_wgrad_h_kernel<WhArgs, 0>), grid, dim3(NT), 0, s, g);
  const int st = cvl_launch_status();
  if (st || g.direct) return st;
  return cvl_wgrad_reduce((const float*)ws, dw[0], dw[0], 9L * d.Cin * d.n_store / 4, l.nsplit, 1, beta, s);
}

// the 3x3 weight gradients of a ResNet stage's units in one launch, each problem in chunks of at
// most the group's common chunk
int launch_wg_h_batch(const WgBatchLaunch& b, const cvl_conv_desc* const* d, const void* const* x, const void* const* dy,
                      float* const* dw, float beta, char* ws, hipStream_t s) {
  static_assert(kMaxWhProb <= kWgXMaxProb, "WgBatchLaunch holds every problem of a launch");
  WhBatch a;
  int wg = 0;
  for (int i = 0; i < kMaxWhProb; ++i) {
    a.wg0[i] = 0x7fffffff;
    if (i >= b.n) continue;
    const int pi = b.idx[i];
    WhArgs& g = a.p[i];
    const int steps = d[pi]->B * d[pi]->seg[0].Hr * d[pi]->seg[0].Wr / RS;
    wh_args(*d[pi], b.chunk < steps ? b.chunk : steps, b.nsplit[i], &g);
    g.x = reinterpret_cast<const cvl_bf16*>(x[pi]);
    g.dy = reinterpret_cast<const cvl_bf16*>(dy[pi]);
    g.out = g.direct ? dw[pi] : reinterpret_cast<float*>(ws + b.slab_off[i]);
    g.beta = beta;
    a.wg0[i] = wg;
    wg += g.ci_tiles * g.co_tiles * g.nsplit;
  }
  a.n = b.n;
  if (b.reads) hipLaunchKernelGGL((conv_wgrad_h_kernel<WhBatch, 1>), dim3(wg), dim3(NT), 0, s, a);
  else hipLaunchKernelGGL((conv_wgrad_h_kernel<WhBatch, 0>), dim3(wg), dim3(NT), 0, s, a);
  int st = cvl_launch_status();
  for (int i = 0; !st && i < b.n; ++i) {
    const WhArgs& g = a.p[i];
    if (!g.direct) st = cvl_wgrad_reduce(g.out, dw[b.idx[i]], dw[b.idx[i]], 9L * g.Cin * g.Cout / 4, g.nsplit, 1, beta, s);
  }
  return st;
}
