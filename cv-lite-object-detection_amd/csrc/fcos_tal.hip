// Task-aligned assignment for FCOS (Feng et al., ICCV 2021, "TOOD: Task-aligned One-stage Object
// Detection") on gfx950 -- an extension beyond the reference, the step after the geometric assigners of
// fcos_paper.hip / fcos_atss.hip: the network's own outputs choose its positives.
//   cvl_fcos_tal_assign   per box the topk inside cells with the largest sigmoid(class logit)^alpha *
//                         IoU(predicted box, box)^beta; per cell the selecting box with the largest IoU
//                         wins; the class target of a won cell is its metric rescaled so that the box's
//                         best cell carries the box's best IoU
//   cvl_fcos_tal_loss     Quality Focal Loss on the class logits against that target, GIoU weighted by
//                         it, both divided by the image's sum of targets; forward + backward in one pass
// The exact rules are stated in include/cvlite.h.  This file is compiled with -ffp-contract=off: a pair's
// values are one fp32 operation sequence (tal_pair) wherever a kernel needs them again.
//
// The assignment is four steps on the stream (plus two memset nodes: the contest keys, the counters):
//   select   one workgroup of 4 waves per (image, box): every thread walks its share of the P cells, and
//            a candidate's key (~metric bits << 32 | cell) goes into an LDS list; topk rounds of a
//            workgroup arg-min (atss_select.h's wave minimum, then across the 4 waves) over that list --
//            or, when a box has more candidates than the list holds, over the cells again, the keys
//            recomputed in every round; the selected pairs post (IoU bits << 32 | ~box) to their cells
//            by a 64-bit integer atomicMax
//   boxmax   one wave per (image, box): integer max of the metric and IoU bits over the cells it won
//   write    per 256-cell tile: decode the winner, recompute its pair, stage the [cells, 5+C] slab in
//            LDS and store it coalesced; positives per level by ballots and integer atomics
// Integer max and integer add are order-independent, and the order in which candidates enter the LDS
// list does not matter to a minimum over distinct keys: the result is bit-identical run to run.
#include "atss_select.h"
#include "cvl_common.h"
#include "fcos_focal.h"

#include <math.h>

namespace {

constexpr int kMaxBoxes = 256;   // per image
constexpr int kMaxTopk = 32;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kStage = 6144;     // candidate keys a workgroup stages (48 KB of LDS)
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------------------------
// assignment
// ---------------------------------------------------------------------------------------------
struct TalArgs {
  const float* boxes;
  const int32_t* nbox;
  const float* img_dim;
  const float* dist;
  const float* cls;
  float* targets;
  int32_t* num_targets;
  unsigned long long* keys;      // [B][P] contest keys, cleared to 0
  int32_t* sel_cell;             // [B][n_max][kMaxTopk] selected cell by rank, or -1
  float* sel_m;                  // ... its metric
  float* sel_u;                  // ... its IoU
  float* bmax;                   // [B][n_max][2] (max metric, max IoU) over the won cells
  int32_t* cand_cells;           // optional [B][n_max][topk]
  float* cand_metric;            // optional, the same shape
  float* cand_iou;               // optional, the same shape
  float* box_max;                // optional [B][n_max][2]
  int n_max, C, P, topk, ld_dist, ld_cls, clamp;
  float alpha, beta;
  int strides[5];
  int Ws[5], off[6];
};

struct TalBox {
  float y0, y1, x0, x1, area;
  int cls;                       // < 0: the box is skipped
};

// Box corners in pixels and the validity test of fcos_atss.hip's load_box.
__device__ __forceinline__ TalBox load_box(const float* r, float H, float W, int C) {
  const float yc = r[0] * H, xc = r[1] * W, hp = r[2] * H, wp = r[3] * W;
  TalBox bx;
  bx.y0 = yc - hp * 0.5f; bx.y1 = yc + hp * 0.5f;
  bx.x0 = xc - wp * 0.5f; bx.x1 = xc + wp * 0.5f;
  bx.area = hp * wp;
  const float lab = r[4];
  bx.cls = (lab > -1.0f && lab < (float)C && bx.area > 0.f) ? (int)lab : -1;
  return bx;
}

struct TalPair {
  float t, bt, l, r, sf;         // pixel distances of the cell's point to the box sides, the stride
  float u, m;                    // IoU of the predicted box, alignment metric (0 outside the box)
  bool in;
};

__device__ __forceinline__ float pow_or(float v, float e, float plain) { return e == plain ? v : powf(v, e); }

// The values of (box, cell p of image b): the one operation sequence every kernel here runs.  The
// predictions of a cell are read only when its point lies inside the box.
__device__ __forceinline__ TalPair tal_pair(const TalArgs& a, const TalBox& bx, int b, int p) {
  int lvl = 0;
  while (lvl < 4 && p >= a.off[lvl + 1]) ++lvl;
  const int q = p - a.off[lvl];
  const int Ws = a.Ws[lvl];
  const int cy = q / Ws, cx = q - (q / Ws) * Ws;
  TalPair o;
  const float sf = (float)a.strides[lvl];
  const float gy = ((float)cy + 0.5f) * sf, gx = ((float)cx + 0.5f) * sf;
  o.sf = sf;
  o.t = gy - bx.y0; o.bt = bx.y1 - gy; o.l = gx - bx.x0; o.r = bx.x1 - gx;
  o.in = o.t > 0.01f && o.bt > 0.01f && o.l > 0.01f && o.r > 0.01f;
  o.u = 0.f; o.m = 0.f;
  if (o.in) {
    const size_t cell = (size_t)b * a.P + p;
    const float* dv = a.dist + cell * a.ld_dist;
    float d[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) d[j] = a.clamp ? fmaxf(dv[j], 0.f) : dv[j];
    const float py0 = gy - d[0] * sf, py1 = gy + d[1] * sf, px0 = gx - d[2] * sf, px1 = gx + d[3] * sf;
    const float ih = fmaxf(fminf(bx.y1, py1) - fmaxf(bx.y0, py0), 0.f);
    const float iw = fmaxf(fminf(bx.x1, px1) - fmaxf(bx.x0, px0), 0.f);
    const float inter = ih * iw;
    const float uni = ((py1 - py0) * (px1 - px0) + bx.area) - inter;
    const float u = uni > 0.f ? (float)((double)inter / (double)uni) : 0.f;
    const float x = a.cls[cell * a.ld_cls + bx.cls];
    const float s = 1.0f / (1.0f + expf(-x));
    float ub;
    if (a.beta == 6.0f) {
      const float u2 = u * u;
      ub = (u2 * u2) * u2;
    } else {
      ub = powf(u, a.beta);
    }
    o.u = u;
    o.m = pow_or(s, a.alpha, 1.0f) * ub;
  }
  return o;
}

// The key the select rounds order by: the smallest key is the largest metric, ties to the lowest cell.
// All ones: not a candidate (outside the box, or a metric that is not > 0 -- a NaN is not).
__device__ __forceinline__ unsigned long long tal_key(const TalArgs& a, const TalBox& bx, int b, int p) {
  const TalPair pr = tal_pair(a, bx, b, p);
  if (!(pr.in && pr.m > 0.f)) return ~0ull;
  return ((unsigned long long)(~__float_as_uint(pr.m)) << 32) | (unsigned)p;
}

__global__ void __launch_bounds__(kThreads) fcos_tal_select_kernel(TalArgs a) {
  const int b = blockIdx.y, i = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int topk = a.topk;

  __shared__ unsigned long long s_keys[kStage];
  __shared__ unsigned long long s_red[2][kWaves];
  __shared__ unsigned long long s_sel[kMaxTopk];
  __shared__ int s_n;

  int n = a.nbox[b];
  n = n < 0 ? 0 : (n > a.n_max ? a.n_max : n);
  const float H = a.img_dim[2 * b + 0];
  const float W = a.img_dim[2 * b + 1];
  const size_t bi = (size_t)b * a.n_max + i;
  TalBox bx;
  bx.cls = -1;
  if (i < n) bx = load_box(a.boxes + bi * 5, H, W, a.C);
  int k = 0;
  if (bx.cls >= 0) {                           // uniform over the workgroup
    if (tid == 0) s_n = 0;
    __syncthreads();
    // ---- candidates: every thread walks its cells; the list's order is arbitrary -------------------
    for (int p = tid; p < a.P; p += kThreads) {
      const unsigned long long key = tal_key(a, bx, b, p);
      if (key != ~0ull) {
        const int slot = atomicAdd(&s_n, 1);
        if (slot < kStage) s_keys[slot] = key;
      }
    }
    __syncthreads();
    const int ncand = s_n;
    const bool staged = ncand <= kStage;
    k = min(topk, ncand);
    // ---- k rounds of a workgroup arg-min: round j takes the smallest key above round j-1's ---------
    unsigned long long last = 0;
    for (int j = 0; j < k; ++j) {
      unsigned long long best = ~0ull;
      if (staged) {
        for (int e = tid; e < ncand; e += kThreads) {
          const unsigned long long key = s_keys[e];
          if ((j == 0 || key > last) && key < best) best = key;
        }
      } else {                                 // more candidates than the list holds: recompute per round
        for (int p = tid; p < a.P; p += kThreads) {
          const unsigned long long key = tal_key(a, bx, b, p);
          if ((j == 0 || key > last) && key < best) best = key;
        }
      }
      best = wave_min_u64(best);
      if (lane == 0) s_red[j & 1][w] = best;
      __syncthreads();
#pragma unroll
      for (int v = 0; v < kWaves; ++v) {
        const unsigned long long o = s_red[j & 1][v];
        best = o < best ? o : best;
      }
      last = best;
      if (tid == 0) s_sel[j] = best;
    }
    __syncthreads();
  }
  // ---- the selected pairs: recorded by rank, each posts its key to its cell -------------------------
  if (tid < kMaxTopk) {
    int cell = -1;
    float m = 0.f, u = 0.f;
    if (tid < k) {
      const unsigned long long key = s_sel[tid];
      cell = (int)(unsigned)key;
      const TalPair pr = tal_pair(a, bx, b, cell);
      m = pr.m;
      u = pr.u;
      const unsigned long long post = ((unsigned long long)__float_as_uint(u) << 32) | (0xFFFFFFFFu - (unsigned)i);
      atomicMax(&a.keys[(size_t)b * a.P + cell], post);
    }
    a.sel_cell[bi * kMaxTopk + tid] = cell;
    a.sel_m[bi * kMaxTopk + tid] = m;
    a.sel_u[bi * kMaxTopk + tid] = u;
    if (tid < topk) {
      if (a.cand_cells) a.cand_cells[bi * topk + tid] = cell;
      if (a.cand_metric) a.cand_metric[bi * topk + tid] = m;
      if (a.cand_iou) a.cand_iou[bi * topk + tid] = u;
    }
  }
}

// One wave per (image, box): the largest metric and the largest IoU over the cells the box won.  Both
// are >= 0, so their bit patterns order as the values do.
__global__ void __launch_bounds__(64) fcos_tal_boxmax_kernel(TalArgs a) {
  const int b = blockIdx.y, i = blockIdx.x, lane = threadIdx.x;
  const size_t bi = (size_t)b * a.n_max + i;
  unsigned mb = 0, ub = 0;
  if (lane < kMaxTopk) {
    const int cell = a.sel_cell[bi * kMaxTopk + lane];
    if (cell >= 0) {
      const unsigned long long key = a.keys[(size_t)b * a.P + cell];
      if ((int)(0xFFFFFFFFu - (unsigned)key) == i) {
        mb = __float_as_uint(a.sel_m[bi * kMaxTopk + lane]);
        ub = __float_as_uint(a.sel_u[bi * kMaxTopk + lane]);
      }
    }
  }
  mb = ~wave_min_u32(~mb);
  ub = ~wave_min_u32(~ub);
  if (lane < 2) {
    const float v = __uint_as_float(lane == 0 ? mb : ub);
    a.bmax[bi * 2 + lane] = v;
    if (a.box_max) a.box_max[bi * 2 + lane] = v;
  }
}

// One thread per cell of a blockDim.x-cell tile (level-major cell index p); the tile's [ncell, 5+C]
// slab is staged in LDS and written out coalesced (the shape of fcos_atss_write_kernel).
__global__ void __launch_bounds__(kThreads) fcos_tal_write_kernel(TalArgs a) {
  const int b = blockIdx.y;
  const int tid = threadIdx.x, nth = blockDim.x;
  const int C = a.C;
  const int row = 5 + C;

  __shared__ int lcount[5];
  extern __shared__ __attribute__((aligned(16))) float stage[];

  if (tid < 5) lcount[tid] = 0;
  __syncthreads();
  const float H = a.img_dim[2 * b + 0];
  const float W = a.img_dim[2 * b + 1];
  const int p0 = blockIdx.x * nth;
  const int p = p0 + tid;
  const int ncell = min(nth, a.P - p0);
  int lvl = 0;
  bool pos = false;
  if (p < a.P) {
    while (lvl < 4 && p >= a.off[lvl + 1]) ++lvl;
    float v0 = 0.f, v1 = 0.f, v2 = 0.f, v3 = 0.f, v4 = 0.f;
    int cls = -1;
    const unsigned long long key = a.keys[(size_t)b * a.P + p];
    if (key != 0ull) {
      const int i = (int)(0xFFFFFFFFu - (unsigned)key);       // < n_max: only valid boxes post keys
      const size_t bi = (size_t)b * a.n_max + i;
      const TalBox bx = load_box(a.boxes + bi * 5, H, W, C);
      const TalPair pr = tal_pair(a, bx, b, p);
      v0 = pr.t / pr.sf; v1 = pr.bt / pr.sf; v2 = pr.l / pr.sf; v3 = pr.r / pr.sf;
      const double max_m = a.bmax[bi * 2], max_u = a.bmax[bi * 2 + 1];
      v4 = (float)((double)pr.m * max_u / (max_m + 1e-9));
      cls = bx.cls;
      pos = true;
    }
    float* st = stage + (size_t)tid * row;
    st[0] = v0; st[1] = v1; st[2] = v2; st[3] = v3; st[4] = v4;
    for (int c = 0; c < C; ++c) st[5 + c] = c == cls ? 1.0f : 0.0f;
  }
  // positives per level: wave ballots -> LDS integer atomics -> one global integer atomic per level
  for (int l = 0; l < 5; ++l) {
    const unsigned long long m = __ballot(pos && lvl == l);
    if ((tid & 63) == 0 && m) atomicAdd(&lcount[l], __popcll(m));
  }
  __syncthreads();
  if (tid < 5 && lcount[tid]) atomicAdd(&a.num_targets[b * 5 + tid], lcount[tid]);
  // coalesced write-out of the tile's contiguous [ncell, 5+C] slab
  float* out = a.targets + ((size_t)b * a.P + p0) * row;
  const int total = ncell * row;
  for (int e = tid; e < total; e += nth) out[e] = stage[e];
}

// ---------------------------------------------------------------------------------------------
// deterministic block reduction of K sums in float64 -> partial[b][tile][K]
// ---------------------------------------------------------------------------------------------
template <int NTH, int K>
__device__ __forceinline__ void block_partials(double* partial, int tiles, const float (&s)[K]) {
  __shared__ double red[K][NTH / 64];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const double v = warp_sum_d((double)s[k]);
    if (lane == 0) red[k][w] = v;
  }
  __syncthreads();
  if (threadIdx.x < K) {
    double t = 0.0;
    for (int k = 0; k < NTH / 64; ++k) t += red[threadIdx.x][k];
    partial[((size_t)blockIdx.y * tiles + blockIdx.x) * K + threadIdx.x] = t;
  }
}

// ---------------------------------------------------------------------------------------------
// loss
// ---------------------------------------------------------------------------------------------
struct TalLossArgs {
  const float* reg;
  const float* cls;
  const float* tgt;
  const float* norm;   // [B, 2] or null
  void* dreg;
  void* dcls;
  double* partial;     // [B, tiles, 2]
  int ld_reg, ld_cls, ld_dreg, ld_dcls, dreg_bf16, dcls_bf16;
  int P, C, tiles;
  float grad_scale, beta, w_box;
};

__device__ __forceinline__ void store_g(void* base, size_t idx, float v, int is_bf16) {
  if (is_bf16) reinterpret_cast<cvl_bf16*>(base)[idx] = f32_to_bf16(v);
  else reinterpret_cast<float*>(base)[idx] = v;
}

// the image's gradient factors: gn = grad_scale / W on the class terms, gbox = grad_scale w_box / W on
// the positives' box terms, W = max(sum of the class targets, 1) (1 without a norm)
__device__ __forceinline__ void image_factors(const TalLossArgs& a, int b, float& gn, float& gbox) {
  const float Wn = a.norm ? fmaxf(a.norm[2 * b + 1], 1.0f) : 1.0f;
  gn = a.grad_scale / Wn;
  gbox = a.grad_scale * a.w_box / Wn;
}

// The box term of a positive cell: that * (1 - GIoU) on d_j = max(p_j, 0), the expressions of
// fcos_paper.hip's cell_rest; g receives the four scaled gradients.
__device__ __forceinline__ float box_term(const float (&tt)[4], const float (&pp)[4], float that, float gbox,
                                          float (&g)[4]) {
  float d[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) d[j] = fmaxf(pp[j], 0.f);
  const float th = tt[0] + tt[1], tw = tt[2] + tt[3], ph = d[0] + d[1], pw = d[2] + d[3];
  const float ih = fminf(tt[0], d[0]) + fminf(tt[1], d[1]), iw = fminf(tt[2], d[2]) + fminf(tt[3], d[3]);
  const float eh = fmaxf(tt[0], d[0]) + fmaxf(tt[1], d[1]), ew = fmaxf(tt[2], d[2]) + fmaxf(tt[3], d[3]);
  const float I = ih * iw;
  const float U = th * tw + ph * pw - I + 1.0e-12f;
  const float E = eh * ew + 1.0e-12f;
  const float giou = I / U - (E - U) / E;
  // GIoU = I/U - 1 + U/E
  const float dGdI = 1.0f / U, dGdU = 1.0f / E - I / (U * U), dGdE = -U / (E * E);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float oi = j < 2 ? iw : ih;      // the other side of the intersection
    const float op = j < 2 ? pw : ph;      // ... of the predicted box
    const float oe = j < 2 ? ew : eh;      // ... of the enclosing box
    const float dI = d[j] < tt[j] ? oi : 0.f;
    const float dE = d[j] > tt[j] ? oe : 0.f;
    const float dG = dGdI * dI + dGdU * (op - dI) + dGdE * dE;
    g[j] = pp[j] > 0.f ? -that * dG * gbox : 0.f;
  }
  return that * (1.0f - giou);
}

// Row-pointer form (any C, any layout): a thread walks its cell's rows in global memory.  NTH is the
// tile of the LDS form it stands in for, so the per-tile partials are the same sums.
template <int NTH>
__global__ void __launch_bounds__(NTH) fcos_tal_loss_rows_kernel(TalLossArgs a) {
  const int b = blockIdx.y;
  const int p = blockIdx.x * NTH + threadIdx.x;
  const int C = a.C;
  float gn, gbox;
  image_factors(a, b, gn, gbox);
  float s[2] = {0.f, 0.f};
  if (p < a.P) {
    const size_t cell = (size_t)b * a.P + p;
    const float* t = a.tgt + cell * (5 + C);
    const float* xc = a.cls + cell * a.ld_cls;
    const float that = t[4];
    bool pos = false;
    for (int c = 0; c < C; ++c) {
      const bool hot = t[5 + c] >= 1.0f;        // some class is hot exactly when the cell is positive
      pos = pos || hot;
      float g;
      s[0] += qfl_term(hot ? that : 0.f, xc[c], a.beta, &g);
      if (a.dcls) store_g(a.dcls, cell * a.ld_dcls + c, g * gn, a.dcls_bf16);
    }
    float g[4] = {0.f, 0.f, 0.f, 0.f};
    if (pos) {
      const float* xr = a.reg + cell * a.ld_reg;
      const float tt[4] = {t[0], t[1], t[2], t[3]};
      const float pp[4] = {xr[0], xr[1], xr[2], xr[3]};
      s[1] = box_term(tt, pp, that, gbox, g);
    }
    if (a.dcls)
      for (int c = C; c < a.ld_dcls; ++c) store_g(a.dcls, cell * a.ld_dcls + c, 0.f, a.dcls_bf16);
    if (a.dreg)
      for (int j = 0; j < a.ld_dreg; ++j) store_g(a.dreg, cell * a.ld_dreg + j, j < 4 ? g[j] : 0.f, a.dreg_bf16);
  }
  block_partials<NTH, 2>(a.partial, a.tiles, s);
}

// LDS-staged form, four lanes per cell (the shape of fcos_paper.hip's fcos_paper_loss_lds4_kernel): the
// block's CPB cells' target and class rows are loaded cooperatively (coalesced) into rows of odd pitch
// R = targets | class logits | box gradients; the C class terms of a cell are spread over its 4 lanes
// (class c on lane c % 4), each term parked in the cell's target slot 5 + c; the owner lane sums them in
// class order (the fp32 sequence of the row form) and, for a positive cell only, reads the four box
// outputs from global memory and runs the box term; the gradient rows leave as 16-byte stores of whole
// rows (padding columns zero).  The block sums take the owners' values in the row form's lane order, so
// the results are bit-identical to fcos_tal_loss_rows_kernel<CPB>.
template <int CPB>
__global__ void __launch_bounds__(4 * CPB) fcos_tal_loss_lds4_kernel(TalLossArgs a, int R) {
  constexpr int NTH = 4 * CPB;
  extern __shared__ float rows[];
  float* csum = rows + CPB * R;                       // per-cell (s_cls, s_box)
  const int b = blockIdx.y, p0 = blockIdx.x * CPB;
  const int ncell = min(CPB, a.P - p0);
  const int C = a.C;
  const int T5 = 5 + C;
  const int OC = T5, OR = T5 + C;
  const size_t cell0 = (size_t)b * a.P + p0;
  float gn, gbox;
  image_factors(a, b, gn, gbox);
  {
    const float* tg = a.tgt + cell0 * T5;
    for (int i = threadIdx.x; i < ncell * T5; i += NTH) {
      const int r = i / T5;
      rows[r * R + (i - r * T5)] = tg[i];
    }
    const float* cg = a.cls + cell0 * a.ld_cls;
    for (int i = threadIdx.x; i < ncell * C; i += NTH) {
      const int r = i / C, c = i - r * C;
      rows[r * R + OC + c] = cg[(size_t)r * a.ld_cls + c];
    }
  }
  __syncthreads();
  const int cell = threadIdx.x >> 2, sub = threadIdx.x & 3;
  const bool live = cell < ncell;
  float* row = rows + cell * R;
  int any_hot = 0;
  if (live) {
    const float that = row[4];
    for (int c = sub; c < C; c += 4) {
      const bool hot = row[5 + c] >= 1.0f;
      any_hot |= hot ? 1 : 0;
      float g;
      row[5 + c] = qfl_term(hot ? that : 0.f, row[OC + c], a.beta, &g);   // the term, in its target slot
      row[OC + c] = g * gn;
    }
  }
  any_hot |= __shfl_xor(any_hot, 1, 64);     // every lane of the wave takes part in the exchange
  any_hot |= __shfl_xor(any_hot, 2, 64);
  const bool pos = any_hot != 0;
  __syncthreads();
  if (sub == 0) {
    float s_cls = 0.f, s_box = 0.f;
    if (live) {
      for (int c = 0; c < C; ++c) s_cls += row[5 + c];
      float g[4] = {0.f, 0.f, 0.f, 0.f};
      if (pos) {
        const float* xr = a.reg + (cell0 + cell) * a.ld_reg;
        const float tt[4] = {row[0], row[1], row[2], row[3]};
        const float pp[4] = {xr[0], xr[1], xr[2], xr[3]};
        s_box = box_term(tt, pp, row[4], gbox, g);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) row[OR + j] = g[j];
    }
    csum[cell * 2] = s_cls;
    csum[cell * 2 + 1] = s_box;
  }
  __syncthreads();
  // gradient rows: whole rows in 16-byte pieces (8 bf16 or 4 fp32 columns), padding columns zero
  auto grad_rows = [&](void* dst, int ld, int is_bf16, int base, int ncol) {
    const int wv = is_bf16 ? 8 : 4, npc = ld / wv;
    for (int i = threadIdx.x; i < ncell * npc; i += NTH) {
      const int r = i / npc, c0 = (i - r * npc) * wv;
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int c = c0 + u;
        v[u] = (u < wv && c < ncol) ? rows[r * R + base + c] : 0.f;
      }
      if (is_bf16) {
        s16x8 o;
#pragma unroll
        for (int u = 0; u < 8; ++u) o[u] = (short)f32_to_bf16(v[u]);
        *reinterpret_cast<s16x8*>(reinterpret_cast<cvl_bf16*>(dst) + (cell0 + r) * ld + c0) = o;
      } else {
        *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(dst) + (cell0 + r) * ld + c0) = f32x4{v[0], v[1], v[2], v[3]};
      }
    }
  };
  if (a.dcls) grad_rows(a.dcls, a.ld_dcls, a.dcls_bf16, OC, C);
  if (a.dreg) grad_rows(a.dreg, a.ld_dreg, a.dreg_bf16, OR, 4);
  // lanes 0 .. CPB-1 carry cells 0 .. CPB-1 as the row form's threads do; the other waves add zeros
  const bool own = (int)threadIdx.x < CPB;
  const float s[2] = {own ? csum[threadIdx.x * 2] : 0.f, own ? csum[threadIdx.x * 2 + 1] : 0.f};
  block_partials<NTH, 2>(a.partial, a.tiles, s);
}

// fixed-order second pass; the per-image divisor and the box weight are applied here, in float64
__global__ void fcos_tal_loss_finalize(const double* partial, const float* norm, float* losses, int tiles,
                                       float w_box) {
  const int b = blockIdx.x;
  const int k = threadIdx.x;   // 0..2
  if (k < 2) {
    double s = 0.0;
    for (int i = 0; i < tiles; ++i) s += partial[((size_t)b * tiles + i) * 2 + k];
    const float Wn = norm ? fmaxf(norm[2 * b + 1], 1.0f) : 1.0f;
    losses[b * 3 + k] = (float)((k == 0 ? 1.0 : (double)w_box) * s / (double)Wn);
  } else if (k == 2) {
    losses[b * 3 + 2] = 0.f;
  }
}

template <int CPB>
void launch_lds4(const TalLossArgs& a, int B, int R, hipStream_t s) {
  const size_t lds = ((size_t)CPB * R + CPB * 2) * sizeof(float);
  hipLaunchKernelGGL((fcos_tal_loss_lds4_kernel<CPB>), dim3(a.tiles, B), dim3(4 * CPB), lds, s, a, R);
}

template <int NTH>
void launch_rows(const TalLossArgs& a, int B, hipStream_t s) {
  hipLaunchKernelGGL((fcos_tal_loss_rows_kernel<NTH>), dim3(a.tiles, B), dim3(NTH), 0, s, a);
}

size_t align8(size_t v) { return (v + 7) & ~(size_t)7; }

}  // namespace

extern "C" size_t cvl_fcos_tal_workspace_size(int B, int P, int n_max) {
  if (B <= 0 || P <= 0 || n_max <= 0) return 0;
  const size_t pairs = (size_t)B * (size_t)n_max;
  return (size_t)B * (size_t)P * sizeof(unsigned long long) + pairs * kMaxTopk * 3 * sizeof(float) +
         align8(pairs * 2 * sizeof(float));
}

extern "C" int cvl_fcos_tal_assign(const float* boxes, const int32_t* nbox, const float* img_dim, int B, int n_max,
                                   int pad_h, int pad_w, int num_classes, const int32_t* strides, const float* dist,
                                   int ld_dist, int clamp, const float* cls_pred, int ld_cls, int topk, float alpha,
                                   float beta, float* targets, int32_t* num_targets, int32_t* cand_cells,
                                   float* cand_metric, float* cand_iou, float* box_max, void* workspace,
                                   size_t workspace_bytes, cvl_stream_t stream) {
  CVL_CHECK_ARG(boxes && nbox && img_dim && targets && num_targets && strides && workspace && dist && cls_pred);
  CVL_CHECK_ARG(B > 0 && n_max > 0 && n_max <= kMaxBoxes && pad_h > 0 && pad_w > 0);
  CVL_CHECK_ARG(num_classes > 0 && num_classes <= 256);
  CVL_CHECK_ARG(topk >= 1 && topk <= kMaxTopk);
  CVL_CHECK_ARG(alpha >= 0.f && beta >= 0.f);          // a NaN exponent fails both
  CVL_CHECK_ARG(ld_dist >= 4 && ld_cls >= num_classes);
  CVL_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 7) == 0);
  TalArgs a;
  a.boxes = boxes; a.nbox = nbox; a.img_dim = img_dim; a.dist = dist; a.cls = cls_pred;
  a.targets = targets; a.num_targets = num_targets;
  a.cand_cells = cand_cells; a.cand_metric = cand_metric; a.cand_iou = cand_iou; a.box_max = box_max;
  a.n_max = n_max; a.C = num_classes; a.topk = topk; a.ld_dist = ld_dist; a.ld_cls = ld_cls;
  a.clamp = clamp ? 1 : 0; a.alpha = alpha; a.beta = beta;
  a.off[0] = 0;
  for (int l = 0; l < 5; ++l) {
    CVL_CHECK_ARG(strides[l] > 0);
    a.strides[l] = strides[l];
    const int Hs = pad_h / strides[l];
    a.Ws[l] = pad_w / strides[l];
    CVL_CHECK_ARG(Hs > 0 && a.Ws[l] > 0);
    a.off[l + 1] = a.off[l] + Hs * a.Ws[l];
  }
  a.P = a.off[5];
  CVL_CHECK_ARG(workspace_bytes >= cvl_fcos_tal_workspace_size(B, a.P, n_max));
  const size_t pairs = (size_t)B * (size_t)n_max;
  a.keys = (unsigned long long*)workspace;
  a.sel_cell = (int32_t*)(a.keys + (size_t)B * a.P);
  a.sel_m = (float*)(a.sel_cell + pairs * kMaxTopk);
  a.sel_u = a.sel_m + pairs * kMaxTopk;
  a.bmax = a.sel_u + pairs * kMaxTopk;
  // the tile of cvl_fcos_paper_assign: the largest whose staged [cells, 5+C] slab fits 56 KB of LDS
  int nth = 0;
  for (int n = kThreads; n >= 64 && !nth; n /= 2)
    if ((size_t)n * (5 + num_classes) * sizeof(float) <= 56 * 1024) nth = n;
  CVL_CHECK_ARG(nth > 0);                              // C <= 219
  const size_t lds = (size_t)nth * (5 + num_classes) * sizeof(float);
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(a.keys, 0, sizeof(unsigned long long) * (size_t)B * a.P, s) != hipSuccess)
    return cvl_launch_status();
  if (hipMemsetAsync(num_targets, 0, sizeof(int32_t) * 5 * B, s) != hipSuccess) return cvl_launch_status();
  hipLaunchKernelGGL(fcos_tal_select_kernel, dim3(n_max, B), dim3(kThreads), 0, s, a);
  int st = cvl_launch_status();
  if (st) return st;
  hipLaunchKernelGGL(fcos_tal_boxmax_kernel, dim3(n_max, B), dim3(64), 0, s, a);
  st = cvl_launch_status();
  if (st) return st;
  hipLaunchKernelGGL(fcos_tal_write_kernel, dim3((a.P + nth - 1) / nth, B), dim3(nth), lds, s, a);
  return cvl_launch_status();
}

extern "C" int cvl_fcos_tal_loss(const float* reg_pred, int ld_reg, const float* cls_pred, int ld_cls,
                                 const float* targets, const float* norm, int B, int P, int num_classes,
                                 float grad_scale, float qfl_beta, float w_box, float* losses, void* d_reg,
                                 int ld_dreg, int dreg_dtype, void* d_cls, int ld_dcls, int dcls_dtype,
                                 void* workspace, size_t workspace_bytes, cvl_stream_t stream) {
  CVL_CHECK_ARG(reg_pred && cls_pred && targets && losses && workspace);
  CVL_CHECK_ARG(B > 0 && P > 0 && num_classes > 0);
  CVL_CHECK_ARG(workspace_bytes >= cvl_fcos_loss_workspace_size(B, P));
  CVL_CHECK_ARG(qfl_beta >= 0.f);
  CVL_CHECK_ARG(ld_reg >= 5 && ld_cls >= num_classes);
  CVL_CHECK_ARG(!d_reg || ld_dreg >= 5);
  CVL_CHECK_ARG(!d_cls || ld_dcls >= num_classes);
  CVL_CHECK_ARG((dreg_dtype == 0 || dreg_dtype == 1) && (dcls_dtype == 0 || dcls_dtype == 1));
  TalLossArgs a;
  a.reg = reg_pred; a.cls = cls_pred; a.tgt = targets; a.norm = norm;
  a.dreg = d_reg; a.dcls = d_cls; a.partial = (double*)workspace;
  a.ld_reg = ld_reg; a.ld_cls = ld_cls; a.ld_dreg = ld_dreg; a.ld_dcls = ld_dcls;
  a.dreg_bf16 = dreg_dtype; a.dcls_bf16 = dcls_dtype;
  a.P = P; a.C = num_classes; a.grad_scale = grad_scale; a.beta = qfl_beta; a.w_box = w_box;
  // the tile: the most cells (256 / 128 / 64) whose rows (pitch R floats, odd) and per-cell sums fit the
  // LDS next to the block sums' static part; 0 when even 64 cells do not (C too large to stage)
  const int R = (5 + num_classes + num_classes + 4) | 1;
  int cpb = 0;
  for (int n = 256; n >= 64 && !cpb; n /= 2)
    if (((size_t)n * R + n * 2) * sizeof(float) <= 63 * 1024) cpb = n;
  // the LDS-staged form needs gradient rows that take 16-byte stores; CVL_DISPATCH=loss_rows forces the
  // row-pointer form on the same tiles
  auto vec_ok = [](const void* p, int ld, int bf16) {
    return !p || ((reinterpret_cast<uintptr_t>(p) & 15) == 0 && ld % (bf16 ? 8 : 4) == 0);
  };
  const bool lds = cpb && vec_ok(d_reg, ld_dreg, dreg_dtype) && vec_ok(d_cls, ld_dcls, dcls_dtype) &&
                   !cvl_dispatch_flag("loss_rows");
  const int tile = cpb ? cpb : kThreads;
  a.tiles = (P + tile - 1) / tile;
  hipStream_t s = (hipStream_t)stream;
  if (lds) {
    if (cpb == 256) launch_lds4<256>(a, B, R, s);
    else if (cpb == 128) launch_lds4<128>(a, B, R, s);
    else launch_lds4<64>(a, B, R, s);
  } else {
    if (tile == 256) launch_rows<256>(a, B, s);
    else if (tile == 128) launch_rows<128>(a, B, s);
    else launch_rows<64>(a, B, s);
  }
  int st = cvl_launch_status();
  if (st) return st;
  hipLaunchKernelGGL(fcos_tal_loss_finalize, dim3(B), dim3(64), 0, s, (const double*)workspace, norm, losses,
                     a.tiles, w_box);
  return cvl_launch_status();
}
