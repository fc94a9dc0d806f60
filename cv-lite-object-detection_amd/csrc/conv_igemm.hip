// Segmented implicit-GEMM convolution (forward and data-gradient) for gfx950, bf16 MFMA.
//
// Replaces the TF2 Conv2D forward/backward-input kernels of the reference model graph
// (FCOS/fcos.py:6-110 + Keras ResNet50; RetinaNet/retinanet_module.py:8-159):
//   C[m, n] = sum_k A[m, k] * Wp[n, k]         k = (r, s, c), c fastest (NHWC friendly)
// forward : m = output pixel (img, oy, ox); A gathers X[img, oy*st - pt + r, ox*st - pl + s, c]
// dgrad   : m = input pixel  (img, iy, ix); A gathers dY[img, (iy + pt - r)/st, (ix + pl - s)/st, c]
//           (tap valid only when divisible), Wp = weights packed [Cin][(r, s, Cout)].
// "Segments" let one launch cover several feature maps that share (or, per segment, swap) the
// weights: all five FPN levels of a shared FCOS tower, or the five per-level heads.  Each segment
// owns a BM-aligned slice of the M space, so a workgroup's rows never straddle segments.
//
// Tile: BM=128 rows x BN (128/64/32) channels x BK (64/32) per K step, 4 waves (2x2), each wave a
// (BM/2)x(BN/2) block of v_mfma_f32_16x16x32_bf16 accumulators.  Operands are register-staged
// global->LDS with 16-byte loads (issued one K step ahead) and an XOR swizzle that makes the
// ds_read_b128 fragment reads conflict-free.  Epilogue: +bias, ReLU, beta*old, per-(image,channel)
// sum / sum-of-squares for the following BatchNorm (double atomics), bf16 output staged through
// LDS for 16-byte coalesced stores, or fp32 output stored straight from the accumulators.
#include "conv_common.h"

namespace {

constexpr int BM = 128;
constexpr int NT = 256;

template <int BK>
__device__ __forceinline__ int swz(int r) {
  return BK == 128 ? (r & 15) : (BK == 64 ? ((r >> 1) & 7) : ((r >> 2) & 3));
}

__device__ __forceinline__ s16x8 relu_bf16x8(s16x8 v) {
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = v[i] < 0 ? (short)0 : v[i];   // bf16 sign bit = int16 sign
  return v;
}



template <int BN, int BK, bool DGRAD>
__global__ void __launch_bounds__(NT) conv_igemm_kernel(ConvArgs a) {
  constexpr int WM = BM / 2, WN = BN / 2;
  constexpr int TM = WM / 16, TN = WN / 16;
  constexpr int CPR = BK / 8;            // 16-byte chunks per row
  constexpr int RPP = NT / CPR;          // rows per load pass
  constexpr int AP = BM / RPP;
  constexpr int BROWS = BN < RPP ? BN : RPP;
  constexpr int BP = BN / BROWS;
  constexpr int LDS_AB = (BM + BN) * BK;
  constexpr int LDS_C = BM * (BN + 8);
  constexpr int LDS_EL = LDS_AB > LDS_C ? LDS_AB : LDS_C;
  __shared__ __attribute__((aligned(16))) cvl_bf16 lds[LDS_EL];
  cvl_bf16* As = lds;
  cvl_bf16* Bs = lds + BM * BK;

  const int tid = threadIdx.x;
  const int m_tile = blockIdx.x, n_tile = blockIdx.y;
  const int m0 = m_tile * BM, n0 = n_tile * BN;
  int sg = 0;
#pragma unroll
  for (int i = 1; i < kMaxSeg; ++i)
    if (i < a.nseg && m0 >= a.seg[i].m_start) sg = i;
  const ConvSeg& S = a.seg[sg];
  const int HWr = S.Hr * S.Wr;
  const int mloc0 = m0 - S.m_start;
  if (mloc0 >= S.rows) return;                       // padding tile of this segment

  // ---- per-thread A-row geometry (fixed for the whole K loop) ---------------------------------
  const int ch = tid % CPR, rr = tid / CPR;
  int a_img[AP], a_y[AP], a_x[AP];
  bool a_ok[AP];
#pragma unroll
  for (int p = 0; p < AP; ++p) {
    const int ml = mloc0 + p * RPP + rr;
    a_ok[p] = ml < S.rows;
    const int img = ml / HWr, q = ml - img * HWr;
    const int oy = q / S.Wr, ox = q - (q / S.Wr) * S.Wr;
    a_img[p] = img;
    if (DGRAD) { a_y[p] = oy + a.pad_t; a_x[p] = ox + a.pad_l; }
    else { a_y[p] = oy * a.stride - a.pad_t; a_x[p] = ox * a.stride - a.pad_l; }
  }
  const cvl_bf16* __restrict__ wsrc = S.w;
  const cvl_bf16* __restrict__ src = a.src;
  const int Cin = a.Cin;

  s16x8 ra[AP], rb[BP];
  auto load_tile = [&](int kt) {
    const int k0 = kt * BK;
    const int tap = k0 / Cin;
    const int c0 = k0 - tap * Cin + ch * 8;
    const int r = tap / a.KW, s = tap - (tap / a.KW) * a.KW;
#pragma unroll
    for (int p = 0; p < AP; ++p) {
      int iy, ix;
      bool ok = a_ok[p];
      if (DGRAD) {
        const int ty = a_y[p] - r, tx = a_x[p] - s;
        ok = ok && ty >= 0 && tx >= 0 && (ty % a.stride) == 0 && (tx % a.stride) == 0;
        iy = ty / a.stride; ix = tx / a.stride;
      } else {
        iy = a_y[p] + r; ix = a_x[p] + s;
      }
      ok = ok && iy >= 0 && ix >= 0 && iy < S.Hs && ix < S.Ws;
      if (ok) {
        const long row = S.src_base + (long)a_img[p] * S.src_img + (long)iy * S.Ws + ix;
        ra[p] = *reinterpret_cast<const s16x8*>(src + row * Cin + c0);
        if (a.relu_in) ra[p] = relu_bf16x8(ra[p]);
      } else {
        ra[p] = s16x8{0, 0, 0, 0, 0, 0, 0, 0};
      }
    }
#pragma unroll
    for (int p = 0; p < BP; ++p) {
      const int n = n0 + p * BROWS + tid / CPR;
      if (tid / CPR < BROWS)
        rb[p] = *reinterpret_cast<const s16x8*>(wsrc + (long)n * a.K + k0 + ch * 8);
    }
  };
  auto store_tile = [&]() {
#pragma unroll
    for (int p = 0; p < AP; ++p) {
      const int r = p * RPP + rr;
      *reinterpret_cast<s16x8*>(As + r * BK + ((ch ^ swz<BK>(r)) * 8)) = ra[p];
    }
#pragma unroll
    for (int p = 0; p < BP; ++p) {
      const int r = p * BROWS + tid / CPR;
      if (tid / CPR < BROWS) *reinterpret_cast<s16x8*>(Bs + r * BK + ((ch ^ swz<BK>(r)) * 8)) = rb[p];
    }
  };

  const int wave = tid >> 6, lane = tid & 63;
  const int wm = wave >> 1, wn = wave & 1;
  const int lr = lane & 15, lg = lane >> 4;
  f32x4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // split-K: this workgroup reduces K-steps [kt0, kt1)
  int kt0 = 0, kt1 = a.K / BK;
  if (a.splits > 1) {
    kt0 = blockIdx.z * a.ksteps_per_split;
    kt1 = min(kt1, kt0 + a.ksteps_per_split);
  }
  const int nk = kt1;
  load_tile(kt0);
  for (int kt = kt0; kt < nk; ++kt) {
    const cvl_bf16* Ac = As;
    const cvl_bf16* Bc = Bs;
    __syncthreads();
    store_tile();
    __syncthreads();
    if (kt + 1 < nk) load_tile(kt + 1);
#pragma unroll
    for (int ks = 0; ks < BK / 32; ++ks) {
      const int chunk = ks * 4 + lg;
      s16x8 fa[TM], fb[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int r = wm * WM + i * 16 + lr;
        fa[i] = *reinterpret_cast<const s16x8*>(Ac + r * BK + ((chunk ^ swz<BK>(r)) * 8));
      }
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int r = wn * WN + j * 16 + lr;
        fb[j] = *reinterpret_cast<const s16x8*>(Bc + r * BK + ((chunk ^ swz<BK>(r)) * 8));
      }
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              __builtin_bit_cast(bf16x8, fa[i]), __builtin_bit_cast(bf16x8, fb[j]), acc[i][j], 0, 0, 0);
    }
  }

  // ---- epilogue -------------------------------------------------------------------------------
  if (a.splits > 1) {   // raw fp32 partials; conv_splitk_finish applies the epilogue
    float* slab = a.slab + (size_t)blockIdx.z * a.m_total * a.Npad;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = m0 + wm * WM + i * 16 + lg * 4 + e;
          const int c = n0 + wn * WN + j * 16 + lr;
          slab[(size_t)r * a.Npad + c] = acc[i][j][e];
        }
    return;
  }
  const float* bias = S.bias;
  float bcol[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int n = n0 + wn * WN + j * 16 + lr;
    bcol[j] = (bias && n < a.n_store) ? bias[n] : 0.f;
  }
  const bool round_bf16 = !a.dst_f32;
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float v = acc[i][j][e] + bcol[j];
        if (a.relu_out) v = v > 0.f ? v : 0.f;
        if (round_bf16) v = bf16_to_f32(f32_to_bf16(v));
        acc[i][j][e] = v;
      }

  if (a.stats && (HWr % BM) != 0) {
    // small maps (H*W < BM): a tile spans several images; the 4 rows of an accumulator quad share
    // one image (host guarantees H*W % 4 == 0), so each lane adds its quad sums directly.
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int ml0 = mloc0 + wm * WM + i * 16 + lg * 4;
      if (ml0 >= S.rows) continue;
      const int img = ml0 / HWr;
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int n = n0 + wn * WN + j * 16 + lr;
        if (n >= a.n_store) continue;
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) { const float v = acc[i][j][e]; s1 += v; s2 += v * v; }
        acc_u64* st = a.stats + acc_idx((long)img * a.n_store + n, 0, a.acc_slots);
        acc_add(st, s1, a.acc_slots);
        acc_add(st + a.acc_slots, s2, a.acc_slots);
      }
    }
  } else if (a.stats) {   // one image per tile (H*W % BM == 0): reduce the tile's rows first
    const int img = mloc0 / HWr;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      float s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int ml = mloc0 + wm * WM + i * 16 + lg * 4 + e;
          const float v = ml < S.rows ? acc[i][j][e] : 0.f;
          s1 += v; s2 += v * v;
        }
      s1 += __shfl_xor(s1, 16, 64); s1 += __shfl_xor(s1, 32, 64);
      s2 += __shfl_xor(s2, 16, 64); s2 += __shfl_xor(s2, 32, 64);
      const int n = n0 + wn * WN + j * 16 + lr;
      if (lg == 0 && n < a.n_store) {
        acc_u64* st = a.stats + acc_idx((long)img * a.n_store + n, 0, a.acc_slots);
        acc_add(st, s1, a.acc_slots);
        acc_add(st + a.acc_slots, s2, a.acc_slots);
      }
    }
  }

  if (a.dst_f32) {
    float* dst = reinterpret_cast<float*>(a.dst);
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int ml = mloc0 + wm * WM + i * 16 + lg * 4 + e;
        if (ml >= S.rows) continue;
        const int img = ml / HWr, q = ml - img * HWr;
        const long drow = conv_dst_row(a, S, img, q);
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          const int n = n0 + wn * WN + j * 16 + lr;
          if (n >= a.n_store) continue;
          float* pd = dst + drow * a.ld_dst + a.dst_coff + n;
          *pd = a.beta != 0.f ? acc[i][j][e] + a.beta * *pd : acc[i][j][e];
        }
      }
    return;
  }

  // bf16: stage the BM x BN tile in LDS, then 16-byte coalesced row stores
  __syncthreads();
  constexpr int CP = BN + 8;
  cvl_bf16* Cs = lds;
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int r = wm * WM + i * 16 + lg * 4 + e;
        const int c = wn * WN + j * 16 + lr;
        Cs[r * CP + c] = f32_to_bf16(acc[i][j][e]);
      }
  __syncthreads();
  constexpr int CCH = BN / 8;               // 16-byte chunks per output row
  cvl_bf16* dst = reinterpret_cast<cvl_bf16*>(a.dst);
  for (int idx = tid; idx < BM * CCH; idx += NT) {
    const int r = idx / CCH, c8 = (idx - (idx / CCH) * CCH) * 8;
    const int ml = mloc0 + r;
    if (ml >= S.rows || n0 + c8 >= a.n_store) continue;
    const int img = ml / HWr, q = ml - img * HWr;
    const long drow = conv_dst_row(a, S, img, q);
    s16x8 v = *reinterpret_cast<const s16x8*>(Cs + r * CP + c8);
    s16x8* pd = reinterpret_cast<s16x8*>(dst + drow * a.ld_dst + a.dst_coff + n0 + c8);
    if (a.beta != 0.f) {
      const s16x8 o = *pd;
#pragma unroll
      for (int u = 0; u < 8; ++u)
        v[u] = (short)f32_to_bf16(bf16_to_f32((cvl_bf16)v[u]) + a.beta * bf16_to_f32((cvl_bf16)o[u]));
    }
    *pd = v;
  }
}

// Split-K epilogue for single-segment convs: sum the partial slabs (fixed split order), + bias,
// ReLU, beta*old, BN statistics, bf16/fp32 store.  Workgroup = (64-channel chunk, image, row part):
// 8 lanes of 8 channels x 32 row lanes, every load of a row issued before the row's sums; the BN
// sums of a chunk reduce over the row lanes in a fixed order through LDS, then ONE atomic pair per
// (image, channel, row part) -- a plain single contribution when the image is one row part.
constexpr int FIN_RL = NT / 8;                       // row lanes per workgroup
__global__ void __launch_bounds__(NT) conv_splitk_finish(ConvArgs a, int rows_per_blk) {
  const ConvSeg& S = a.seg[0];
  const int HW = S.Hr * S.Wr;
  const int img = blockIdx.y;
  const int cgi = threadIdx.x & 7, rl = threadIdx.x >> 3;
  const int c0 = blockIdx.z * 64 + cgi * 8;
  const bool cok = c0 < a.n_store;
  const int q0 = blockIdx.x * rows_per_blk;
  const int q1 = min(q0 + rows_per_blk, HW);
  __shared__ float red[FIN_RL][8][17];
  float s1[8], s2[8], bb[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) { s1[u] = 0.f; s2[u] = 0.f; bb[u] = (S.bias && cok) ? S.bias[c0 + u] : 0.f; }
  if (cok) {
    for (int q = q0 + rl; q < q1; q += FIN_RL) {
      const long ml = (long)img * HW + q;
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = bb[u];
      const f32x4* p = reinterpret_cast<const f32x4*>(a.slab + (size_t)ml * a.Npad + c0);
      const size_t zs = (size_t)a.m_total * a.Npad / 4;     // one split's slab, in float4s
      int z = 0;
      for (; z + 4 <= a.splits; z += 4) {                  // 8 loads in flight, then the adds in split order
        f32x4 x[4][2];
#pragma unroll
        for (int t = 0; t < 4; ++t) { x[t][0] = p[(z + t) * zs]; x[t][1] = p[(z + t) * zs + 1]; }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          v[0] += x[t][0][0]; v[1] += x[t][0][1]; v[2] += x[t][0][2]; v[3] += x[t][0][3];
          v[4] += x[t][1][0]; v[5] += x[t][1][1]; v[6] += x[t][1][2]; v[7] += x[t][1][3];
        }
      }
      for (; z < a.splits; ++z) {
        const f32x4 x0 = p[z * zs], x1 = p[z * zs + 1];
        v[0] += x0[0]; v[1] += x0[1]; v[2] += x0[2]; v[3] += x0[3];
        v[4] += x1[0]; v[5] += x1[1]; v[6] += x1[2]; v[7] += x1[3];
      }
      const long drow = conv_dst_row(a, S, img, q);
      if (a.dst_f32) {
        float* pd = reinterpret_cast<float*>(a.dst) + drow * a.ld_dst + a.dst_coff + c0;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          float o = v[u];
          if (a.relu_out) o = o > 0.f ? o : 0.f;
          s1[u] += o; s2[u] += o * o;
          if (a.beta != 0.f) o += a.beta * pd[u];
          pd[u] = o;
        }
      } else {
        s16x8* pd = reinterpret_cast<s16x8*>(reinterpret_cast<cvl_bf16*>(a.dst) + drow * a.ld_dst + a.dst_coff + c0);
        s16x8 old;
        if (a.beta != 0.f) old = *pd;
        s16x8 o;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          float x = v[u];
          if (a.relu_out) x = x > 0.f ? x : 0.f;
          x = bf16_to_f32(f32_to_bf16(x));
          s1[u] += x; s2[u] += x * x;
          if (a.beta != 0.f) x += a.beta * bf16_to_f32((cvl_bf16)old[u]);
          o[u] = (short)f32_to_bf16(x);
        }
        *pd = o;
      }
    }
  }
  if (a.stats) {
#pragma unroll
    for (int u = 0; u < 8; ++u) { red[rl][cgi][u] = s1[u]; red[rl][cgi][8 + u] = s2[u]; }
    __syncthreads();
    if (threadIdx.x < 64) {
      const int cg2 = threadIdx.x >> 3, u = threadIdx.x & 7;
      const int c = blockIdx.z * 64 + cg2 * 8 + u;
      if (c < a.n_store) {
        double t1 = 0.0, t2 = 0.0;
        for (int k = 0; k < FIN_RL; ++k) { t1 += red[k][cg2][u]; t2 += red[k][cg2][8 + u]; }
        acc_u64* st = a.stats + acc_idx((long)img * a.n_store + c, 0, a.acc_slots);
        acc_add_f64(st, t1, a.acc_slots);
        acc_add_f64(st + a.acc_slots, t2, a.acc_slots);
      }
    }
  }
}

// launch geometry of the finish: (row parts, images, 64-channel chunks), ~512 workgroups, >= 16 rows each
// (the 8x8 maps of P6 at bs 16 gave 64 workgroups of 64 rows with a 64-row floor: 15 us)
static int splitk_finish_launch(const ConvArgs& a, hipStream_t s) {
  const ConvSeg& S = a.seg[0];
  const int HW = S.Hr * S.Wr;
  const int nch = (a.n_store + 63) / 64;
  int parts = 512 / (a.B * nch);
  if (parts > HW / 16) parts = HW / 16;
  if (parts < 1) parts = 1;
  const int rpb = (HW + parts - 1) / parts;
  hipLaunchKernelGGL(conv_splitk_finish, dim3((HW + rpb - 1) / rpb, a.B, nch), dim3(NT), 0, s, a, rpb);
  return cvl_launch_status();
}

template <int BN, int BK>
void launch_bn_bk(const ConvPlan& p, const ConvArgs& a, hipStream_t s) {
  dim3 grid(a.m_tiles, a.Npad / BN, a.splits);
  with_bool(p.dgrad, [&](auto DG) {
    hipLaunchKernelGGL((conv_igemm_kernel<BN, BK, decltype(DG)::value>), grid, dim3(NT), 0, s, a);
  });
}

// (plain `if`: the 128-wide tile keeps its 128-deep instantiation, which is never planned)
template <int BN>
void launch_bn(const ConvPlan& p, const ConvArgs& a, hipStream_t s) {
  if (BN <= 64 && p.bk == 128) launch_bn_bk<BN, 128>(p, a, s);
  else if (p.bk == 64) launch_bn_bk<BN, 64>(p, a, s);
  else launch_bn_bk<BN, 32>(p, a, s);
}

}  // namespace

// sub[cls][n][t' = 2 r' + s'][c] from wd[n][(3 r + s) * Cin + c], 16-B chunks: the four 2x2
// sub-kernels of a 3x3 / stride-2 data gradient (conv_dispatch.hip: s2dgrad3_ok)
__global__ void s2dgrad3_pack_kernel(const cvl_bf16* __restrict__ wd, cvl_bf16* __restrict__ sub, int Npad, int Cin) {
  const int c8n = Cin / 8;
  const long total = 16L * Npad * c8n;
  for (long i = blockIdx.x * (long)NT + threadIdx.x; i < total; i += (long)gridDim.x * NT) {
    const int c8 = (int)(i % c8n);
    const long r1 = i / c8n;
    const int t = (int)(r1 & 3);
    const long r2 = r1 >> 2;
    const int n = (int)(r2 % Npad), cls = (int)(r2 / Npad);
    const int py = cls >> 1, px = cls & 1, rp = t >> 1, sp = t & 1;
    const int r = py ? (rp ? 1 : -1) : (rp ? 0 : 2);
    const int sx = px ? (sp ? 1 : -1) : (sp ? 0 : 2);
    s16x8 v = s16x8{0, 0, 0, 0, 0, 0, 0, 0};
    if (r >= 0 && sx >= 0) v = *reinterpret_cast<const s16x8*>(wd + (long)n * 9 * Cin + (r * 3 + sx) * Cin + c8 * 8);
    *reinterpret_cast<s16x8*>(sub + i * 8) = v;
  }
}

// the pixels a strided data gradient's scatter does not reach, zeroed: one block row per (image,
// map row) -- rows with y % s != 0 are all gaps, the others every x % s != 0 -- and threads over
// (x, 16-B column chunk), 32-bit index math (the flat 64-bit-division form was VALU-bound)
__global__ void zero_gaps_kernel(void* dst, int is_f32, long dst_base, long dst_img, int ld, int coff, int n,
                                 int B, int H, int W, int s) {
  const int n8 = is_f32 ? n : n / 8;
  for (int line = blockIdx.y; line < B * H; line += gridDim.y) {
    const int img = line / H, y = line - img * H;
    const bool full = y % s != 0;
    const long base = dst_base + (long)img * dst_img + (long)y * W;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < W * n8; i += gridDim.x * blockDim.x) {
      const int x = i / n8, c = i - x * n8;
      if (!full && x % s == 0) continue;
      const long row = base + x;
      if (is_f32) reinterpret_cast<float*>(dst)[row * ld + coff + c] = 0.f;
      else *reinterpret_cast<s16x8*>(reinterpret_cast<cvl_bf16*>(dst) + row * ld + coff + c * 8) = s16x8{0, 0, 0, 0, 0, 0, 0, 0};
    }
  }
}

namespace {

// the pass a plan asks for before its launch (d: the caller's descriptor)
int pre_pass(const ConvPlan& p, const cvl_conv_desc* d, void* dst, void* workspace, hipStream_t s) {
  if (p.pre == CVL_PRE_S2DG3_PACK) {
    const long b = (16L * d->Npad * (d->Cin / 8) + NT - 1) / NT;
    hipLaunchKernelGGL(s2dgrad3_pack_kernel, dim3((int)(b > 4096 ? 4096 : (b < 1 ? 1 : b))), dim3(NT), 0, s,
                       reinterpret_cast<const cvl_bf16*>(d->seg[0].w), reinterpret_cast<cvl_bf16*>(workspace), d->Npad,
                       d->Cin);
  } else if (p.pre == CVL_PRE_ZERO_GAPS) {
    const cvl_conv_seg& q = d->seg[0];
    const long line = (long)q.Wr * (d->dst_f32 ? d->n_store : d->n_store / 8);
    const int bx = (int)((line + NT - 1) / NT);
    const int by = d->B * q.Hr < 65535 ? d->B * q.Hr : 65535;
    hipLaunchKernelGGL(zero_gaps_kernel, dim3(bx < 1 ? 1 : bx, by), dim3(NT), 0, s, dst, d->dst_f32, q.dst_base,
                       q.dst_img, d->ld_dst, d->dst_coff, d->n_store, d->B, q.Hr, q.Wr, d->stride);
  } else {
    return CVL_OK;
  }
  return cvl_launch_status();
}

// what a call hands over beside its descriptor
struct ConvIo {
  const void* src;
  void* dst;
  acc_u64* stats;
  const BnSumArgs* bsum;     // read when the plan fuses the BN sums
  const void* ymask;         // read when the plan applies the ReLU mask
  void* workspace;
};

// The kernel arguments of a planned call: the plan's layout plus the call's pointers.
void fill_args(const ConvPlan& p, const ConvIo& io, ConvArgs* a) {
  *a = p.geo;
  a->src = reinterpret_cast<const cvl_bf16*>(io.src);
  a->dst = io.dst;
  a->stats = io.stats;
  if (p.bsum) {
    const BnSumArgs& b = *io.bsum;
    a->bz = b.z; a->bmr = b.mr; a->bga = b.gamma; a->bbe = b.beta; a->bsum = b.sums; a->bhi = b.hi;
    a->by = b.y;
    a->bbits = b.bits;
  }
  if (p.ymask) a->ymask = reinterpret_cast<const cvl_bf16*>(io.ymask);
  // bench.py's in-step timing: the tower kernel takes the call's armed slot
  if (p.kernel == CVL_CK_X32) a->probe = reinterpret_cast<unsigned long long*>(cvl_probe_current(true));
  a->dbg = p.dbg;
  a->splits = p.splits;
  a->ksteps_per_split = p.ksteps_per_split;
  char* ws = reinterpret_cast<char*>(io.workspace);
  if (p.splits > 1) a->slab = reinterpret_cast<float*>(ws + p.pack_bytes);
  if (p.pre == CVL_PRE_S2DG3_PACK)       // the four sub-kernel packs the pre-pass wrote
    for (int i = 0; i < kMaxSeg; ++i)
      a->seg[i].w = reinterpret_cast<const cvl_bf16*>(ws) + (size_t)(i < a->nseg ? i : 0) * a->Npad * a->K;
}

}  // namespace

thread_local int g_cvl_conv_last_kernel = CVL_CK_NONE;
thread_local int g_cvl_conv_last_ktile = 0;

extern "C" int cvl_conv_igemm_last_kernel(void) { return g_cvl_conv_last_kernel; }
extern "C" int cvl_conv_igemm_last_ktile(void) { return g_cvl_conv_last_ktile; }

// Launches the 128-row kernel as planned.
int launch_base(const ConvPlan& p, const ConvArgs& a, hipStream_t s) {
  if (p.bn == 128) launch_bn<128>(p, a, s);
  else if (p.bn == 64) launch_bn<64>(p, a, s);
  else launch_bn<32>(p, a, s);
  return cvl_launch_status();
}

namespace {
// A planned call: optional pre-pass, the launch, optional split-K finish.
int conv_run(const ConvPlan& p, const cvl_conv_desc* d, const ConvIo& io, hipStream_t s) {
  int st = pre_pass(p, d, io.dst, io.workspace, s);
  if (st) return st;
  ConvArgs a;
  fill_args(p, io, &a);
  switch (p.kernel) {
    case CVL_CK_P: st = launch_p(p, a, s); break;
    case CVL_CK_X32: st = launch_x(p, a, s); break;
    case CVL_CK_H64: st = launch_h(p, a, s); break;
    case CVL_CK_L64: case CVL_CK_L128: case CVL_CK_L256: st = launch_l(p, a, s); break;
    default: st = launch_base(p, a, s); break;
  }
  g_cvl_conv_last_kernel = p.kernel;
  g_cvl_conv_last_ktile = conv_plan_ktile(p);
  if (st || p.splits <= 1) return st;
  return splitk_finish_launch(a, s);
}
}  // namespace

extern "C" const char* cvl_conv_kernel_name(int code) {
  switch (code) {
    case CVL_CK_BASE: return "conv_igemm_kernel (128-row)";
    case CVL_CK_BASE_SPLITK: return "conv_igemm_kernel (128-row, split-K)";
    case CVL_CK_L64: return "conv_igemm_l_kernel<64> (256x64)";
    case CVL_CK_L128: return "conv_igemm_l_kernel<128> (256x128)";
    case CVL_CK_L256: return "conv_igemm_l_kernel<256> (256x256)";
    case CVL_CK_X256: return "conv_igemm_x_kernel (256x256, 4 phases per 64-deep K-tile)";
    case CVL_CK_X32: return "conv_igemm_x32_kernel (256x256, 5-slot ring of 32-deep K-tiles)";
    case CVL_CK_X32H: return "conv_igemm_x32h_kernel (256x256, 3x3 halo tile in LDS, 6-slot weight ring)";
    case CVL_CK_WG_SN: return "conv_wgrad_sn_kernel (Npad 32, taps on the dY side, chunk slabs)";
    case CVL_CK_WG_S: return "conv_wgrad_kernel (128-wide k tile)";
    case CVL_CK_WG_L128: return "conv_wgrad_l_kernel<128> (128x256)";
    case CVL_CK_WG_L256: return "conv_wgrad_l_kernel<256> (256x256)";
    case CVL_CK_WG_X: return "conv_wgrad_x_kernel (256x256, 5-slot ring of 32-row steps, grouped)";
    case CVL_CK_WG_H: return "conv_wgrad_h_kernel (64 ci x 64 co x 9 taps, 128-row halo steps)";
    case CVL_CK_H64: return "conv_igemm_h_kernel (256x64, 3x3 halo + 9-tap weight stage per channel block)";
    case CVL_CK_P: return "conv_igemm_p_kernel (persistent 1x1, K-tile stream across tiles)";
    default: return "none";
  }
}

int cvl_conv_f32(const cvl_conv_desc* d, const void* src, void* dst, acc_u64* bn_stats, hipStream_t s);
int cvl_relu_backward(const void* dy, const void* y, void* dx, long n, float beta, cvl_stream_t stream);

extern "C" size_t cvl_conv_igemm_workspace_size(const cvl_conv_desc* d) {
  if (!d) return 0;
  if (d->prec == CVL_PREC_F32) return 16;
  return conv_plan_workspace_bound(d);
}

extern "C" int cvl_conv_igemm(const cvl_conv_desc* d, const void* src, void* dst, uint64_t* bn_stats_acc,
                              void* workspace, size_t workspace_bytes, cvl_stream_t stream) {
  CVL_CHECK_ARG(d);
  acc_u64* bn_stats = reinterpret_cast<acc_u64*>(bn_stats_acc);
  if (d->prec == CVL_PREC_F32) return cvl_conv_f32(d, src, dst, bn_stats, (hipStream_t)stream);    // parity mode
  ConvPlan p;
  const int st = conv_plan(d, ConvCallOpts{bn_stats != nullptr, CVL_BSUM_NONE, false, workspace ? workspace_bytes : 0}, &p);
  if (st) return st;
  CVL_CHECK_ARG(src && dst);
  cvl_probe_enter_call();            // an armed probe slot belongs to this call and leaves with it
  const int rst = conv_run(p, d, ConvIo{src, dst, bn_stats, nullptr, nullptr, workspace}, (hipStream_t)stream);
  cvl_probe_leave_call();
  return rst;
}

// A data gradient through a ReLU (FPNDetector.trunk_backward: the heads' data gradients into the
// towers' ReLU outputs, fcos.py:16-27 / 76-101): dst = dgrad(src) * (y > 0), y laid out as dst.  The
// X32 register epilogue applies the mask; any other kernel's launch is followed by the separate
// ReLU backward (then dst must be dense: ld_dst == n_store, dst_coff 0 -- checked before anything
// is launched).  Bit-identical to cvl_conv_igemm + cvl_relu_backward either way.
extern "C" int cvl_conv_igemm_relu_mask(const cvl_conv_desc* d, const void* src, void* dst, const void* y,
                                        void* workspace, size_t workspace_bytes, cvl_stream_t stream) {
  CVL_CHECK_ARG(d && src && dst && y && d->mode == CVL_CONV_DGRAD && d->prec == CVL_PREC_BF16 && !d->dst_f32 &&
                d->beta == 0.f && !d->relu_out);
  ConvPlan p;
  int st = conv_plan(d, ConvCallOpts{false, CVL_BSUM_NONE, true, workspace ? workspace_bytes : 0}, &p);
  if (st) return st;
  if (!p.ymask) CVL_CHECK_ARG(d->ld_dst == d->n_store && d->dst_coff == 0);
  cvl_probe_enter_call();
  st = conv_run(p, d, ConvIo{src, dst, nullptr, nullptr, y, workspace}, (hipStream_t)stream);
  cvl_probe_leave_call();
  if (st || p.ymask) return st;
  long rows = 0;
  for (int i = 0; i < d->nseg; ++i) {
    const long e = d->seg[i].dst_base + (long)d->B * (d->seg[i].dst_img ? d->seg[i].dst_img : (long)d->seg[i].Hr * d->seg[i].Wr);
    rows = e > rows ? e : rows;
  }
  return cvl_relu_backward(dst, y, dst, rows * d->n_store, 0.f, stream);
}

namespace {
// what cvl_conv_igemm_res_relu accepts, and its plan (the ReLU after the accumulate offered)
int res_relu_plan(const cvl_conv_desc* d, size_t ws, ConvPlan* p) {
  CVL_CHECK_ARG(d && d->mode == CVL_CONV_FWD && d->prec == CVL_PREC_BF16 && !d->dst_f32 && d->beta == 1.f &&
                !d->relu_out);
  const int st = conv_plan(d, ConvCallOpts{false, CVL_BSUM_NONE, false, ws, true}, p);
  if (st) return st;
  // the separate ReLU pass runs over whole rows from dst
  if (!p->res_relu) CVL_CHECK_ARG(d->ld_dst == d->n_store && d->dst_coff == 0);
  return CVL_OK;
}
}  // namespace

// A residual unit with its BatchNorm folded into the conv (inference, ResNet50.forward(folded=True):
// the bottleneck's conv3): dst = relu(conv(src) + bias + dst), forward, bf16, beta 1.  The persistent
// 1x1 kernel's accumulate form applies the ReLU to the packed value right after the accumulate; any
// other plan runs the beta = 1 launch followed by the in-place ReLU (then dst must be dense: ld_dst ==
// n_store, dst_coff 0 -- checked before anything is launched).  ReLU of a bf16 value is exact: the two
// forms are bit-identical.
extern "C" int cvl_conv_igemm_res_relu(const cvl_conv_desc* d, const void* src, void* dst, void* workspace,
                                       size_t workspace_bytes, cvl_stream_t stream) {
  CVL_CHECK_ARG(src && dst);
  ConvPlan p;
  int st = res_relu_plan(d, workspace ? workspace_bytes : 0, &p);
  if (st) return st;
  cvl_probe_enter_call();
  st = conv_run(p, d, ConvIo{src, dst, nullptr, nullptr, nullptr, workspace}, (hipStream_t)stream);
  cvl_probe_leave_call();
  if (st || p.res_relu) return st;
  long lo = d->seg[0].dst_base, hi = 0;      // the rows the segments span
  for (int i = 0; i < d->nseg; ++i) {
    const long b = d->seg[i].dst_base;
    const long e = b + (long)d->B * (d->seg[i].dst_img ? d->seg[i].dst_img : (long)d->seg[i].Hr * d->seg[i].Wr);
    lo = b < lo ? b : lo;
    hi = e > hi ? e : hi;
  }
  return cvl_relu_(reinterpret_cast<cvl_bf16*>(dst) + lo * d->n_store, (hi - lo) * d->n_store, stream);
}

// Test and profiling hook: the kernel family a cvl_conv_igemm_res_relu call would use and whether its
// epilogue applies the ReLU (*fused 1) or the separate pass follows (0).  Host only, no launch.
extern "C" int cvl_conv_igemm_res_relu_plan(const cvl_conv_desc* d, size_t workspace_bytes, int32_t* kernel,
                                            int32_t* fused) {
  CVL_CHECK_ARG(kernel && fused);
  *kernel = CVL_CK_NONE;
  *fused = 0;
  ConvPlan p;
  const int st = res_relu_plan(d, workspace_bytes, &p);
  if (st) return st;
  *kernel = p.kernel;
  *fused = p.res_relu ? 1 : 0;
  return CVL_OK;
}

namespace {
// The form a fused BN-sums offer ends up with: the offer itself, the y form where only the bitmap
// form is declined, or CVL_BSUM_NONE.
int dgrad_bnsum_plan_form(const cvl_conv_desc* d, int offer, size_t ws, int32_t* form) {
  *form = CVL_BSUM_NONE;
  if (d->prec == CVL_PREC_F32) return CVL_OK;
  for (int f = offer; f != CVL_BSUM_NONE; f = f == CVL_BSUM_BITS ? CVL_BSUM_Y : CVL_BSUM_NONE) {
    ConvPlan p;
    const int st = conv_plan(d, ConvCallOpts{false, f, false, ws}, &p);
    if (st) return st;
    if (p.kernel != CVL_CK_NONE) { *form = f; break; }
  }
  return CVL_OK;
}

// The two fused BN-sums entries: plan with the sums offered; where no kernel can fuse them, plan
// the plain data gradient (*fused = 0: the caller then runs the two-pass BN backward).
int dgrad_bnsum_call(const cvl_conv_desc* d, const void* src, void* dst, int form, const BnSumArgs& b, int32_t* fused,
                     void* workspace, size_t workspace_bytes, cvl_stream_t stream) {
  *fused = 0;
  if (d->prec == CVL_PREC_F32) return cvl_conv_f32(d, src, dst, nullptr, (hipStream_t)stream);    // parity mode
  const size_t ws = workspace ? workspace_bytes : 0;
  ConvPlan p;
  int st = conv_plan(d, ConvCallOpts{false, form, false, ws}, &p);
  if (st) return st;
  const bool fuse = p.kernel != CVL_CK_NONE && src && dst;
  if (!fuse && (st = conv_plan(d, ConvCallOpts{false, CVL_BSUM_NONE, false, ws}, &p))) return st;
  CVL_CHECK_ARG(src && dst);
  // (an armed probe slot belongs to the next plain call: a fused launch leaves it armed)
  if (!fuse) cvl_probe_enter_call();
  st = conv_run(p, d, ConvIo{src, dst, nullptr, &b, nullptr, workspace}, (hipStream_t)stream);
  if (!fuse) cvl_probe_leave_call();
  *fused = fuse && st == CVL_OK ? 1 : 0;
  return st;
}
}  // namespace

// Data gradient whose epilogue also forms the first pass of the NEXT BN's backward (the dgrad
// result is dy of a BN -> ReLU unit without a residual): sums[img][c] += (sum g, sum g*xhat).
// Taken when a 256-row LDS-DMA kernel runs the launch with one image per tile; otherwise the
// plain data gradient runs and *fused = 0 (the caller then runs the two-pass BN backward).
extern "C" int cvl_conv_igemm_dgrad_bnsum(const cvl_conv_desc* d, const void* src, void* dst, const void* z,
                                          const float* mean_rstd, const float* gamma, const float* beta, float act_hi,
                                          uint64_t* sums, int32_t* fused, void* workspace, size_t workspace_bytes,
                                          cvl_stream_t stream) {
  CVL_CHECK_ARG(d && fused && z && mean_rstd && gamma && beta && sums);
  const BnSumArgs b{reinterpret_cast<const cvl_bf16*>(z), mean_rstd, gamma, beta, reinterpret_cast<acc_u64*>(sums),
                    act_hi, nullptr, nullptr};
  return dgrad_bnsum_call(d, src, dst, CVL_BSUM_Z, b, fused, workspace, workspace_bytes, stream);
}

// The residual-unit form: the dgrad result, accumulated into dst with d->beta (the block-input
// gradient a bottleneck's first 1x1 data gradient completes), is dy of a BN whose output passes
// through (+ shortcut) -> ReLU; the mask is y > 0 from that unit's output y.  1x1 launches on the
// persistent kernel only; otherwise the plain data gradient runs and *fused = 0.
extern "C" int cvl_conv_igemm_dgrad_bnsum_res(const cvl_conv_desc* d, const void* src, void* dst, const void* y,
                                              const void* z, const float* mean_rstd, const float* gamma,
                                              const float* beta, uint64_t* sums, int32_t* fused, void* workspace,
                                              size_t workspace_bytes, cvl_stream_t stream) {
  CVL_CHECK_ARG(d && fused && y && z && mean_rstd && gamma && beta && sums);
  const BnSumArgs b{reinterpret_cast<const cvl_bf16*>(z), mean_rstd, gamma, beta, reinterpret_cast<acc_u64*>(sums),
                    INFINITY, reinterpret_cast<const cvl_bf16*>(y), nullptr};
  return dgrad_bnsum_call(d, src, dst, CVL_BSUM_Y, b, fused, workspace, workspace_bytes, stream);
}

// The same with the mask read from y's ReLU sign bitmap (cvl_bn_finalize_apply_bits): one byte per
// 8-channel chunk instead of the 16-byte y chunk.  Where the planner declines the bitmap form
// (ld_dst / dst_coff not multiples of 8) the y form runs; *form (optional) reports which
// (CVL_BSUM_BITS 3 / CVL_BSUM_Y 2; 0 when not fused).
extern "C" int cvl_conv_igemm_dgrad_bnsum_res_bits(const cvl_conv_desc* d, const void* src, void* dst, const void* y,
                                                   const uint8_t* relu_bits, const void* z, const float* mean_rstd,
                                                   const float* gamma, const float* beta, uint64_t* sums,
                                                   int32_t* fused, int32_t* form, void* workspace,
                                                   size_t workspace_bytes, cvl_stream_t stream) {
  CVL_CHECK_ARG(d && fused && y && relu_bits && z && mean_rstd && gamma && beta && sums);
  const BnSumArgs b{reinterpret_cast<const cvl_bf16*>(z), mean_rstd, gamma, beta, reinterpret_cast<acc_u64*>(sums),
                    INFINITY, reinterpret_cast<const cvl_bf16*>(y), relu_bits};
  int32_t tmp = 0, *pf = form ? form : &tmp;
  *pf = 0;
  int st = dgrad_bnsum_plan_form(d, CVL_BSUM_BITS, workspace ? workspace_bytes : 0, pf);
  if (st) return st;
  st = dgrad_bnsum_call(d, src, dst, *pf ? *pf : CVL_BSUM_Y, b, fused, workspace, workspace_bytes, stream);
  if (st || !*fused) *pf = 0;
  return st;
}

// Test and profiling hook: the fused BN-sums form (*form: CVL_BSUM_* code, 0 = none, the plain data
// gradient runs) and kernel family / K-tile a cvl_conv_igemm_dgrad_bnsum* call offering `offer` would
// use (offer CVL_BSUM_BITS falls back to CVL_BSUM_Y as the entry does).  Host only, no launch.
extern "C" int cvl_conv_igemm_plan_bnsum(const cvl_conv_desc* d, int offer, size_t workspace_bytes, int32_t* form,
                                         int32_t* kernel, int32_t* ktile) {
  CVL_CHECK_ARG(d && form && kernel && ktile && offer >= CVL_BSUM_Z && offer <= CVL_BSUM_BITS);
  *form = 0;
  *kernel = CVL_CK_NONE;
  *ktile = 0;
  if (d->prec == CVL_PREC_F32) return CVL_OK;
  int st = dgrad_bnsum_plan_form(d, offer, workspace_bytes, form);
  if (st) return st;
  ConvPlan p;
  if ((st = conv_plan(d, ConvCallOpts{false, *form, false, workspace_bytes}, &p))) return st;
  *kernel = p.kernel;
  *ktile = conv_plan_ktile(p);
  return CVL_OK;
}

// Test hook: cvl_conv_igemm_plan (offer 0) / cvl_conv_igemm_plan_bnsum (offer 1..3) with the planned
// launch grid (*grid: workgroups per split) and N-tile width (*ntile) as well.  Host only, no launch.
extern "C" int cvl_conv_igemm_plan_grid(const cvl_conv_desc* d, int with_bn_stats, int bsum_offer, size_t workspace_bytes,
                                        int32_t* kernel, int32_t* ktile, int32_t* grid, int32_t* ntile) {
  CVL_CHECK_ARG(d && kernel && ktile && grid && ntile && bsum_offer >= CVL_BSUM_NONE && bsum_offer <= CVL_BSUM_BITS);
  *kernel = CVL_CK_NONE;
  *ktile = *grid = *ntile = 0;
  if (d->prec == CVL_PREC_F32) return CVL_OK;
  int32_t form = CVL_BSUM_NONE;
  int st = bsum_offer ? dgrad_bnsum_plan_form(d, bsum_offer, workspace_bytes, &form) : CVL_OK;
  if (st) return st;
  ConvPlan p;
  if ((st = conv_plan(d, ConvCallOpts{with_bn_stats != 0 && !form, form, false, workspace_bytes}, &p))) return st;
  *kernel = p.kernel;
  *ktile = conv_plan_ktile(p);
  *grid = p.grid;
  *ntile = p.bn;
  return CVL_OK;
}
