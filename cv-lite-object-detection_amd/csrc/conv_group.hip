// Grouped 3x3 convolution on gfx950: the 32-group 3x3 of the ResNeXt bottleneck (the
// `backbone_model="resnext50" | "resnext101"` branch of RetinaNet/retinanet_module.py:53-66).
// NHWC bf16 activations at channel pitch C, fp32 master kernel [3][3][Cg][C] (output channel o
// belongs to group o / Cg and reads input channels (o / Cg) * Cg .. + Cg), fp32 accumulation,
// ZeroPadding2D(1) + "valid" (pad 1 top / left), stride 1 or 2.
//
// The op is HBM-bound (1/32 .. 1/8 of the dense conv's MACs on the same map), so MFMA waste is
// affordable: every 32-channel slab (64 contiguous bytes per pixel) runs as an independent dense
// 3x3 32 -> 32 conv on v_mfma_f32_16x16x32_bf16 with weights that are block-diagonal within the
// slab (exact at Cg = 32, 2x / 4x / 8x zero padding at Cg = 16 / 8 / 4).
//   * forward and stride-1 data gradient: one kernel on two packed weight images (the data-gradient
//     image is flipped and transposed within each group).  A workgroup owns one slab of one image and
//     walks a column of output tiles: the tile's input halo is staged once in LDS (80-byte pixel
//     rows: 64 + 16 pad), the slab's 9 x 32 x 32 weights stay in registers (72 VGPRs) for the walk.
//     The next tile's halo is fetched into registers before the current tile's MFMAs and lands
//     under them; workgroups are ordered slab-fastest through xcd_remap, so the slabs that share a
//     tile's 128-byte lines run side by side on one XCD's L2.
//     MFMA operands: A = weights [co][ci], B = halo pixels [ci][pixel], so a lane ends up with 8
//     consecutive output channels of one pixel and stores them as one 16-byte vector.  Optional BN
//     statistics (of the rounded bf16 outputs) ride on the epilogue.
//   * stride-2 data gradient: the four output-parity classes.  An M block is 16 dx pixels of one row
//     and one column parity, so the taps that meet a dY sample are wave-uniform (1, 2 or 4 of the 9)
//     and only those are multiplied; the dY halo is staged compactly (no zero insertion).
//   * weight gradient: per slab dW[tap][ci][co] = sum over pixels x[p + tap][ci] * dy[p][co] with the
//     pixels as the MFMA K dimension.  x and dy are transposed into LDS as [channel][pixel] images (x
//     once per kernel column kx, pre-shifted, so every fragment is one aligned 16-byte read for
//     stride 1 and 2 alike); a workgroup accumulates a run of pixel tiles in registers, writes the
//     block-diagonal entries of its partial, and a second kernel sums the partials in a fixed order
//     (no float atomics: bit-identical run to run).
#include "conv_common.h"

namespace {

constexpr int NT = 256;
constexpr int PITCH = 80;                 // LDS bytes per halo pixel (64 + 16: conflict-free b128 reads)
constexpr int PACK_SLAB = 9 * 32 * 32;    // packed bf16 elements per slab: [tap][out 32][in 32]

struct GcGeo {
  int B, Hs, Ws, Hd, Wd, C, nslab;        // source map, destination map
  int tiles_x, tiles_y, tpw, ychunks;     // destination tiles; y tiles per workgroup; chunks per column
  float beta;
  int slots;                              // BN accumulator mode
};

__device__ __forceinline__ f32x4 mfma16(s16x8 a, s16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0,
                                                 0);
}

// fp32 master [3][3][Cg][C] -> bf16 slab images [slab][tap][out][in] (zero off the group blocks):
// forward  Pf[tap][o][i] = w[tap][i % Cg][o]            (i, o in one group)
// dgrad    Pd[tap][i][o] = w[8 - tap][i % Cg][o]        (out = input channel i, in = output channel o)
__global__ void __launch_bounds__(NT) gc_pack_kernel(const float* __restrict__ w, cvl_bf16* __restrict__ pf,
                                                     cvl_bf16* __restrict__ pd, int C, int Cg, long n) {
  for (long e = blockIdx.x * (long)NT + threadIdx.x; e < n; e += (long)gridDim.x * NT) {
    const int in = (int)(e & 31), out = (int)((e >> 5) & 31);
    const int tap = (int)((e >> 10) % 9), slab = (int)((e >> 10) / 9);
    const bool same = in / Cg == out / Cg;
    if (pf) pf[e] = same ? f32_to_bf16(w[((long)tap * Cg + in % Cg) * C + slab * 32 + out]) : (cvl_bf16)0;
    if (pd) pd[e] = same ? f32_to_bf16(w[((long)(8 - tap) * Cg + out % Cg) * C + slab * 32 + in]) : (cvl_bf16)0;
  }
}

// MODE 0: dst(oy, ox) = sum_tap src(oy*S - 1 + ky, ox*S - 1 + kx) . P[tap]  (forward; stride-1 data
//         gradient on the flipped image).  Tile: TH rows x 16 pixels, an M block = one tile row.
// MODE 1: stride-2 data gradient, dst = dx, src = dy: dx(iy, ix) = sum over taps with (iy - 1 + ky) and
//         (ix - 1 + kx) even of dy((iy - 1 + ky) / 2, (ix - 1 + kx) / 2) . Pd[tap].  Tile: 8 rows x 32
//         pixels, an M block = one row and one column parity (16 pixels, ix = ix0 + 2 i + par).
template <int MODE, int S>
struct GcTile {
  static constexpr int TH = MODE == 1 ? 8 : (S == 1 ? 8 : 4);
  static constexpr int TW = MODE == 1 ? 32 : 16;
  static constexpr int HR = MODE == 1 ? TH / 2 + 1 : (TH - 1) * S + 3;     // halo rows / columns
  static constexpr int HC = MODE == 1 ? TW / 2 + 1 : 15 * S + 3;
  static constexpr int MB = MODE == 1 ? 2 * TH : TH;                       // M blocks per tile
};

template <int MODE, int S>
__global__ void __launch_bounds__(NT) gc_conv_kernel(const cvl_bf16* __restrict__ src, const cvl_bf16* __restrict__ wp,
                                                     cvl_bf16* __restrict__ dst, acc_u64* __restrict__ stats, GcGeo g) {
  using T = GcTile<MODE, S>;
  __shared__ __attribute__((aligned(16))) unsigned char halo[T::HR * T::HC * PITCH];
  __shared__ float red[4][32][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, lg = lane >> 4;
  // the slabs of one pixel tile share its 128-byte lines: consecutive logical ids, one XCD's L2
  int bid = xcd_remap(blockIdx.x, gridDim.x);
  const int slab = bid % g.nslab; bid /= g.nslab;
  const int tx = bid % g.tiles_x; bid /= g.tiles_x;
  const int yc = bid % g.ychunks;
  const int b = bid / g.ychunks;

  // the slab's weights: fragment (tap, h) row li is output channel 8 (li >> 2) + 4 h + (li & 3), so
  // accumulator registers 0..3 of half h are channels 8 lg + 4 h + 0..3 of the lane's pixel
  s16x8 wf[9][2];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int co = 8 * (li >> 2) + 4 * h + (li & 3);
      wf[t][h] = *reinterpret_cast<const s16x8*>(wp + ((long)slab * 9 + t) * 1024 + co * 32 + lg * 8);
    }

  float s1[8], s2[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) s1[u] = s2[u] = 0.f;

  const cvl_bf16* sb = src + (long)b * g.Hs * g.Ws * g.C + slab * 32;
  cvl_bf16* db = dst + (long)b * g.Hd * g.Wd * g.C + slab * 32;
  const int x0 = tx * T::TW;
  const int sx0 = MODE == 1 ? x0 / 2 : x0 * S - 1;
  // the halo of tile ty into registers (zero outside the map) / from registers into LDS: the next
  // tile's loads are issued before this tile's MFMAs and land under them
  constexpr int NCH = (T::HR * T::HC * 4 + NT - 1) / NT;
  s16x8 pre[NCH];
  auto fetch = [&](int ty) {
    const int sy0 = MODE == 1 ? ty * T::TH / 2 : ty * T::TH * S - 1;
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      const int i = tid + k * NT;
      const int px = i >> 2, q = i & 3;
      const int hr = px / T::HC, hc = px - hr * T::HC;
      const int sy = sy0 + hr, sx = sx0 + hc;
      pre[k] = s16x8{0, 0, 0, 0, 0, 0, 0, 0};
      if (i < T::HR * T::HC * 4 && sy >= 0 && sy < g.Hs && sx >= 0 && sx < g.Ws)
        pre[k] = *reinterpret_cast<const s16x8*>(sb + ((long)sy * g.Ws + sx) * g.C + q * 8);
    }
  };
  const int ty0 = yc * g.tpw;
  const int ty1 = ty0 + g.tpw < g.tiles_y ? ty0 + g.tpw : g.tiles_y;
  fetch(ty0);
  for (int ty = ty0; ty < ty1; ++ty) {
    const int y0 = ty * T::TH;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      const int i = tid + k * NT;
      if (i < T::HR * T::HC * 4) *reinterpret_cast<s16x8*>(halo + (i >> 2) * PITCH + (i & 3) * 16) = pre[k];
    }
    __syncthreads();
    if (ty + 1 < ty1) fetch(ty + 1);
    for (int m = wave; m < T::MB; m += 4) {
      f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
      int oy, ox;
      if (MODE == 0) {
        oy = y0 + m;
        ox = x0 + li;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
          for (int kx = 0; kx < 3; ++kx) {
            const int px = (m * S + ky) * T::HC + li * S + kx;
            const s16x8 xf = *reinterpret_cast<const s16x8*>(halo + px * PITCH + lg * 16);
            acc[0] = mfma16(wf[ky * 3 + kx][0], xf, acc[0]);
            acc[1] = mfma16(wf[ky * 3 + kx][1], xf, acc[1]);
          }
      } else {
        const int r = m >> 1, par = m & 1;
        oy = y0 + r;
        ox = x0 + 2 * li + par;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
          if ((r + 1 + ky) & 1) continue;                 // (iy - 1 + ky) odd: between dY rows (y0 even)
          const int hr = (r - 1 + ky) >> 1;
#pragma unroll
          for (int kx = 0; kx < 3; ++kx) {
            if ((par + 1 + kx) & 1) continue;
            const int px = hr * T::HC + li + ((par - 1 + kx) >> 1);
            const s16x8 xf = *reinterpret_cast<const s16x8*>(halo + px * PITCH + lg * 16);
            acc[0] = mfma16(wf[ky * 3 + kx][0], xf, acc[0]);
            acc[1] = mfma16(wf[ky * 3 + kx][1], xf, acc[1]);
          }
        }
      }
      if (oy < g.Hd && ox < g.Wd) {
        cvl_bf16* o = db + ((long)oy * g.Wd + ox) * g.C + lg * 8;
        float f[8] = {acc[0][0], acc[0][1], acc[0][2], acc[0][3], acc[1][0], acc[1][1], acc[1][2], acc[1][3]};
        if (g.beta != 0.f) {
          const s16x8 old = *reinterpret_cast<const s16x8*>(o);
#pragma unroll
          for (int u = 0; u < 8; ++u) f[u] += g.beta * bf16_to_f32((cvl_bf16)old[u]);
        }
        s16x8 v;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const cvl_bf16 h = f32_to_bf16(f[u]);
          v[u] = (short)h;
          const float rf = bf16_to_f32(h);
          s1[u] += rf;
          s2[u] += rf * rf;
        }
        *reinterpret_cast<s16x8*>(o) = v;
      }
    }
  }
  if (stats) {       // per-image sums of the rounded outputs: 16 pixel lanes, then the 4 waves, then atomics
#pragma unroll
    for (int u = 0; u < 8; ++u) {
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) {
        s1[u] += __shfl_xor(s1[u], o, 64);
        s2[u] += __shfl_xor(s2[u], o, 64);
      }
    }
    if (li == 0) {
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        red[wave][lg * 8 + u][0] = s1[u];
        red[wave][lg * 8 + u][1] = s2[u];
      }
    }
    __syncthreads();
    if (tid < 64) {
      const int c = tid >> 1, s = tid & 1;
      const float v = (red[0][c][s] + red[1][c][s]) + (red[2][c][s] + red[3][c][s]);
      acc_add(stats + acc_idx((long)b * g.C + slab * 32 + c, s, g.slots), v, g.slots);
    }
  }
}

// ---- weight gradient ----------------------------------------------------------------------------
template <int S>
struct GwTile {
  static constexpr int TH = S == 1 ? 8 : 4;            // output rows x 16 output columns per tile
  static constexpr int XR = (TH - 1) * S + 3;          // x rows of the tile
  static constexpr int XP = XR * 16 + 8;               // channel pitch of an x image (elements)
  static constexpr int DP = TH * 16 + 8;               // channel pitch of the dy image
};

struct GwGeo {
  int B, H, W, Ho, Wo, C, Cg, nslab;
  int tiles_x, tiles_y;
  long ntiles;
  int tpc;                                             // tiles per chunk
};

// part[chunk][tap][ci % Cg][C]: block-diagonal entries of the chunk's partial sums
template <int S>
__global__ void __launch_bounds__(NT) gc_wgrad_kernel(const cvl_bf16* __restrict__ x, const cvl_bf16* __restrict__ dy,
                                                      float* __restrict__ part, GwGeo g) {
  using T = GwTile<S>;
  __shared__ __attribute__((aligned(16))) cvl_bf16 xk[3][32][T::XP];     // [kx][ci][row][16 columns]
  __shared__ __attribute__((aligned(16))) cvl_bf16 dt[32][T::DP];        // [co][row][16 columns]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, lg = lane >> 4;
  const int cih = wave & 1, coh = wave >> 1;           // the wave's (ci, co) quadrant of the 32 x 32 block
  const int slab = blockIdx.x % g.nslab, chunk = blockIdx.x / g.nslab;
  f32x4 acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const long t0 = (long)chunk * g.tpc;
  const long t1 = t0 + g.tpc < g.ntiles ? t0 + g.tpc : g.ntiles;
  for (long t = t0; t < t1; ++t) {
    const int tx = (int)(t % g.tiles_x);
    const long rest = t / g.tiles_x;
    const int ty = (int)(rest % g.tiles_y), b = (int)(rest / g.tiles_y);
    const int oy0 = ty * T::TH, ox0 = tx * 16;
    const cvl_bf16* xb = x + (long)b * g.H * g.W * g.C + slab * 32;
    const cvl_bf16* db = dy + (long)b * g.Ho * g.Wo * g.C + slab * 32;
    __syncthreads();
    for (int i = tid; i < 3 * T::XR * 64; i += NT) {
      const int q = i & 3, c = (i >> 2) & 15;
      const int rr = i >> 6;
      const int kx = rr / T::XR, r = rr - kx * T::XR;
      const int sy = oy0 * S - 1 + r, sx = (ox0 + c) * S - 1 + kx;
      s16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
      if (sy >= 0 && sy < g.H && sx >= 0 && sx < g.W)
        v = *reinterpret_cast<const s16x8*>(xb + ((long)sy * g.W + sx) * g.C + q * 8);
#pragma unroll
      for (int j = 0; j < 8; ++j) xk[kx][q * 8 + j][r * 16 + c] = (cvl_bf16)v[j];
    }
    for (int i = tid; i < T::TH * 64; i += NT) {
      const int q = i & 3, c = (i >> 2) & 15, r = i >> 6;
      const int oy = oy0 + r, ox = ox0 + c;
      s16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
      if (oy < g.Ho && ox < g.Wo) v = *reinterpret_cast<const s16x8*>(db + ((long)oy * g.Wo + ox) * g.C + q * 8);
#pragma unroll
      for (int j = 0; j < 8; ++j) dt[q * 8 + j][r * 16 + c] = (cvl_bf16)v[j];
    }
    __syncthreads();
    // a K step = 32 output pixels = 2 tile rows: lane group lg holds row 2 ks + (lg >> 1), columns
    // 8 (lg & 1) .. + 8 of both operands
#pragma unroll
    for (int ks = 0; ks < T::TH / 2; ++ks) {
      const int r = 2 * ks + (lg >> 1), c = (lg & 1) * 8;
      const s16x8 bf = *reinterpret_cast<const s16x8*>(&dt[coh * 16 + li][r * 16 + c]);
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const s16x8 af = *reinterpret_cast<const s16x8*>(&xk[kx][cih * 16 + li][(r * S + ky) * 16 + c]);
          acc[ky * 3 + kx] = mfma16(af, bf, acc[ky * 3 + kx]);
        }
    }
  }
  // D[row = ci 4 lg + e][col = co li] of the quadrant
  const int co = coh * 16 + li;
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int ci = cih * 16 + 4 * lg + e;
      if (ci / g.Cg == co / g.Cg)
        part[(((long)chunk * 9 + t) * g.Cg + ci % g.Cg) * g.C + slab * 32 + co] = acc[t][e];
    }
}

// dw[i] = beta * dw[i] + sum over chunks of part[chunk][i], chunks in a fixed order
__global__ void __launch_bounds__(NT) gc_wgrad_reduce_kernel(const float* __restrict__ part, float* __restrict__ dw,
                                                             long n, int nchunk, float beta) {
  const long i = blockIdx.x * (long)NT + threadIdx.x;
  if (i >= n) return;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  int k = 0;
  for (; k + 3 < nchunk; k += 4) {
    a0 += part[(long)k * n + i];
    a1 += part[(long)(k + 1) * n + i];
    a2 += part[(long)(k + 2) * n + i];
    a3 += part[(long)(k + 3) * n + i];
  }
  for (; k < nchunk; ++k) a0 += part[(long)k * n + i];
  const float s = (a0 + a1) + (a2 + a3);
  dw[i] = (beta != 0.f ? beta * dw[i] : 0.f) + s;
}

bool gc_ok(int B, int H, int W, int C, int Cg, int stride, int Ho, int Wo) {
  return B > 0 && H > 0 && W > 0 && C > 0 && C % 32 == 0 && (Cg == 4 || Cg == 8 || Cg == 16 || Cg == 32) &&
         (stride == 1 || stride == 2) && Ho == (H - 1) / stride + 1 && Wo == (W - 1) / stride + 1;
}

// y tiles per workgroup: walk up to 4 tiles on one set of weight registers while that leaves the
// machine a few workgroups per CU
// (CVL_DISPATCH=gc_tpw=1|2|4: a test hook -- the walk at small sizes; a value above tiles_y is legal,
// the walk clamps at the column's last tile)
inline int gc_tpw(long wgs_at_1, int tiles_y) {
  const int forced = cvl_dispatch_int("gc_tpw", 0);
  if (forced == 1 || forced == 2 || forced == 4) return forced;
  int tpw = 1;
  while (tpw < 4 && tpw * 2 <= tiles_y && wgs_at_1 / (tpw * 2) >= 1024) tpw *= 2;
  return tpw;
}

// the tiling of one launch (the one place it is decided: gc_launch and cvl_gconv3x3_plan)
template <int MODE, int S>
GcGeo gc_geo(int B, int Hs, int Ws, int Hd, int Wd, int C) {
  using T = GcTile<MODE, S>;
  GcGeo g;
  g.B = B; g.Hs = Hs; g.Ws = Ws; g.Hd = Hd; g.Wd = Wd; g.C = C; g.nslab = C / 32;
  g.tiles_x = (Wd + T::TW - 1) / T::TW;
  g.tiles_y = (Hd + T::TH - 1) / T::TH;
  g.tpw = gc_tpw((long)g.tiles_x * g.tiles_y * B * g.nslab, g.tiles_y);
  g.ychunks = (g.tiles_y + g.tpw - 1) / g.tpw;
  g.beta = 0.f;
  g.slots = 0;
  return g;
}

template <int MODE, int S>
int gc_launch(const void* src, const void* wp, void* dst, acc_u64* stats, int B, int Hs, int Ws, int Hd, int Wd, int C,
              float beta, hipStream_t s) {
  GcGeo g = gc_geo<MODE, S>(B, Hs, Ws, Hd, Wd, C);
  g.beta = beta;
  g.slots = cvl_bn_acc_slots();
  const long wgs = (long)g.tiles_x * g.ychunks * B * g.nslab;
  CVL_CHECK_ARG(wgs <= 0x7fffffffL);
  hipLaunchKernelGGL((gc_conv_kernel<MODE, S>), dim3((unsigned)wgs), dim3(NT), 0, s, (const cvl_bf16*)src,
                     (const cvl_bf16*)wp, (cvl_bf16*)dst, stats, g);
  return cvl_launch_status();
}

struct GwPlan {
  GwGeo g;
  int nchunk;
};

GwPlan gw_plan(int B, int H, int W, int C, int Cg, int stride, int Ho, int Wo) {
  GwPlan p;
  GwGeo& g = p.g;
  const int th = stride == 1 ? GwTile<1>::TH : GwTile<2>::TH;
  g.B = B; g.H = H; g.W = W; g.Ho = Ho; g.Wo = Wo; g.C = C; g.Cg = Cg; g.nslab = C / 32;
  g.tiles_x = (Wo + 15) / 16;
  g.tiles_y = (Ho + th - 1) / th;
  g.ntiles = (long)B * g.tiles_x * g.tiles_y;
  // ~1024 workgroups (CVL_DISPATCH=gw_wgs=N, N >= 1: a test hook -- long chunks on a small map)
  int target = cvl_dispatch_int("gw_wgs", 1024);
  if (target < 1) target = 1024;
  long want = target / g.nslab;
  if (want < 1) want = 1;
  long tpc = (g.ntiles + want - 1) / want;
  if (tpc < 1) tpc = 1;
  if (tpc > 0x7fffffffL) tpc = 0x7fffffffL;
  g.tpc = (int)tpc;
  p.nchunk = (int)((g.ntiles + tpc - 1) / tpc);
  return p;
}

}  // namespace

#define S_ ((hipStream_t)stream)

extern "C" size_t cvl_gconv3x3_packed_bytes(int C) {
  return C > 0 && C % 32 == 0 ? (size_t)(C / 32) * PACK_SLAB * sizeof(cvl_bf16) : 0;
}

extern "C" int cvl_gconv3x3_pack(const float* w, int C, int Cg, void* w_fwd, void* w_dgrad, cvl_stream_t stream) {
  CVL_CHECK_ARG(w && (w_fwd || w_dgrad) && gc_ok(1, 1, 1, C, Cg, 1, 1, 1));
  const long n = (long)(C / 32) * PACK_SLAB;
  hipLaunchKernelGGL(gc_pack_kernel, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, S_, w, (cvl_bf16*)w_fwd,
                     (cvl_bf16*)w_dgrad, C, Cg, n);
  return cvl_launch_status();
}

extern "C" int cvl_gconv3x3_fwd(const void* x, const void* w_fwd, void* y, uint64_t* stats, int B, int H, int W, int C,
                                int Cg, int stride, int Ho, int Wo, cvl_stream_t stream) {
  CVL_CHECK_ARG(x && w_fwd && y && gc_ok(B, H, W, C, Cg, stride, Ho, Wo));
  if (stride == 1) return gc_launch<0, 1>(x, w_fwd, y, (acc_u64*)stats, B, H, W, Ho, Wo, C, 0.f, S_);
  return gc_launch<0, 2>(x, w_fwd, y, (acc_u64*)stats, B, H, W, Ho, Wo, C, 0.f, S_);
}

extern "C" int cvl_gconv3x3_dgrad(const void* dy, const void* w_dgrad, void* dx, int B, int H, int W, int C, int Cg,
                                  int stride, int Ho, int Wo, float beta, cvl_stream_t stream) {
  CVL_CHECK_ARG(dy && w_dgrad && dx && gc_ok(B, H, W, C, Cg, stride, Ho, Wo));
  if (stride == 1) return gc_launch<0, 1>(dy, w_dgrad, dx, nullptr, B, Ho, Wo, H, W, C, beta, S_);
  return gc_launch<1, 2>(dy, w_dgrad, dx, nullptr, B, Ho, Wo, H, W, C, beta, S_);
}

extern "C" int cvl_gconv3x3_plan(int kind, int B, int H, int W, int C, int Cg, int stride, int* tpw, int* ychunks,
                                 int* tiles_x, int* tiles_y, int* tpc, int* nchunk) {
  CVL_CHECK_ARG(kind >= 0 && kind <= 2 && (stride == 1 || stride == 2));
  const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  CVL_CHECK_ARG(gc_ok(B, H, W, C, Cg, stride, Ho, Wo));
  int v[6] = {0, 0, 0, 0, 0, 0};                       // tpw, ychunks, tiles_x, tiles_y, tpc, nchunk
  if (kind == 2) {
    const GwPlan p = gw_plan(B, H, W, C, Cg, stride, Ho, Wo);
    v[2] = p.g.tiles_x; v[3] = p.g.tiles_y; v[4] = p.g.tpc; v[5] = p.nchunk;
  } else {
    GcGeo g;
    if (kind == 0) g = stride == 1 ? gc_geo<0, 1>(B, H, W, Ho, Wo, C) : gc_geo<0, 2>(B, H, W, Ho, Wo, C);
    else g = stride == 1 ? gc_geo<0, 1>(B, Ho, Wo, H, W, C) : gc_geo<1, 2>(B, Ho, Wo, H, W, C);
    v[0] = g.tpw; v[1] = g.ychunks; v[2] = g.tiles_x; v[3] = g.tiles_y;
  }
  int* out[6] = {tpw, ychunks, tiles_x, tiles_y, tpc, nchunk};
  for (int i = 0; i < 6; ++i)
    if (out[i]) *out[i] = v[i];
  return CVL_OK;
}

extern "C" size_t cvl_gconv3x3_wgrad_workspace_size(int B, int H, int W, int C, int Cg, int stride) {
  if (!gc_ok(B, H, W, C, Cg, stride, (H - 1) / (stride > 0 ? stride : 1) + 1, (W - 1) / (stride > 0 ? stride : 1) + 1))
    return 0;
  const GwPlan p = gw_plan(B, H, W, C, Cg, stride, (H - 1) / stride + 1, (W - 1) / stride + 1);
  return (size_t)p.nchunk * 9 * Cg * C * sizeof(float);
}

extern "C" int cvl_gconv3x3_wgrad(const void* x, const void* dy, float* dw, float beta, int B, int H, int W, int C,
                                  int Cg, int stride, int Ho, int Wo, void* workspace, size_t workspace_bytes,
                                  cvl_stream_t stream) {
  CVL_CHECK_ARG(x && dy && dw && workspace && gc_ok(B, H, W, C, Cg, stride, Ho, Wo));
  CVL_CHECK_ARG(workspace_bytes >= cvl_gconv3x3_wgrad_workspace_size(B, H, W, C, Cg, stride));
  const GwPlan p = gw_plan(B, H, W, C, Cg, stride, Ho, Wo);
  const long wgs = (long)p.nchunk * p.g.nslab;
  CVL_CHECK_ARG(wgs <= 0x7fffffffL);
  float* part = reinterpret_cast<float*>(workspace);
  if (stride == 1)
    hipLaunchKernelGGL(gc_wgrad_kernel<1>, dim3((unsigned)wgs), dim3(NT), 0, S_, (const cvl_bf16*)x,
                       (const cvl_bf16*)dy, part, p.g);
  else
    hipLaunchKernelGGL(gc_wgrad_kernel<2>, dim3((unsigned)wgs), dim3(NT), 0, S_, (const cvl_bf16*)x,
                       (const cvl_bf16*)dy, part, p.g);
  const long n = 9L * Cg * C;
  hipLaunchKernelGGL(gc_wgrad_reduce_kernel, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, S_, (const float*)part, dw,
                     n, p.nchunk, beta);
  return cvl_launch_status();
}
