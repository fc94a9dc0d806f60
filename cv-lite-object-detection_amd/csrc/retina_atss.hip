// ATSS target assignment and the normalised loss for RetinaNet (Zhang et al., CVPR 2020) on gfx950 --
// an extension beyond the reference, next to fcos_atss.hip, whose structure it takes:
//   cvl_retina_atss_assign  per box the topk anchors nearest its centre on every level (the A anchors of a
//                           cell tie, so these are the ceil(topk / A) nearest cells), their IoUs with the
//                           box, threshold mean + std of those IoUs; per anchor the positive pair with
//                           the largest IoU wins.  Targets are compact: 8 floats per anchor, in the row
//                           order of the head outputs [P][A]
//   cvl_retina_atss_loss    focal + smooth-L1 on those rows, divided by the image's positive anchors
// The exact rules are stated in include/cvlite.h.  This file is compiled with -ffp-contract=off: the
// assignment is a fixed operation sequence that tests/retina_atss_ref.py restates bit for bit.
//
// Assign, three steps on the stream (plus two memset nodes: the contest keys and the level counters):
//   select   one workgroup per (image, box), one wave per level: ceil(topk / A) rounds of a wave arg-min
//            over the window about the box centre, a separable check that no cell outside the window can
//            displace a selected one (else the rounds run over the whole level), the anchor IoUs, the
//            serial float64 statistics, and one 64-bit integer atomicMax per positive pair into the
//            anchor's contest key (IoU bits << 32 | ~box)
//   write    per 64-cell tile: decode the winners, compute their rows, stage [cells][A][8] in LDS and
//            store 16 bytes per lane; positives per level by integer atomics
// Integer max and integer add are order-independent, so the result is bit-identical run to run.
#include "atss_select.h"
#include "cvl_common.h"
#include "fcos_focal.h"
#include "smooth_l1.h"

#include <math.h>

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

constexpr int kMaxBoxes = 256;   // per image
constexpr int kMaxTopk = 144;
constexpr int kMaxCells = 16;    // ceil(topk / A)
constexpr int kMaxAnchors = 16;
constexpr int kLevels = 5;
constexpr int kThreads = 256;
constexpr int kTileCells = 64;   // write kernel: cells per workgroup
constexpr int kLossCells = 16;   // loss kernel: cells per workgroup

struct RAtssArgs {
  const float* boxes;
  const int32_t* nbox;
  const float* img_dim;
  const float* adims;            // [5][A][2] (h, w)
  float* targets;                // [B][P][A][8]
  int32_t* num_targets;          // [B][5]
  unsigned long long* keys;      // [B][P*A] contest keys, cleared to 0
  int32_t* cand_idx;             // optional [B][n_max][5*topk]
  float* cand_iou;               // optional [B][n_max][5*topk]
  double* cand_thr;              // optional [B][n_max]
  int n_max, C, A, P, topk, kc;  // kc = ceil(topk / A)
  int strides[5], S[5], off[6];
};

struct RBox {
  float y0, y1, x0, x1, yc, xc, hp, wp, area;
  int cls;                       // < 0: the box is skipped
};

// Box corners in pixels: the operation order of cvl_fcos_atss_assign's load_box.
__device__ __forceinline__ RBox load_box(const float* r, float H, float W, int C) {
  const float yc = r[0] * H, xc = r[1] * W, hp = r[2] * H, wp = r[3] * W;
  RBox bx;
  bx.yc = yc; bx.xc = xc; bx.hp = hp; bx.wp = wp;
  bx.y0 = yc - hp * 0.5f; bx.y1 = yc + hp * 0.5f;
  bx.x0 = xc - wp * 0.5f; bx.x1 = xc + wp * 0.5f;
  bx.area = hp * wp;
  const float lab = r[4];
  bx.cls = (lab > -1.0f && lab < (float)C && bx.area > 0.f) ? (int)lab : -1;
  return bx;
}

__global__ void __launch_bounds__(64 * kLevels) retina_atss_select_kernel(RAtssArgs a) {
  const int b = blockIdx.y, i = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, lvl = tid >> 6;
  const int topk = a.topk, A = a.A;
  const int slots = kLevels * topk;

  __shared__ int s_idx[kLevels * kMaxTopk];
  __shared__ float s_iou[kLevels * kMaxTopk];
  __shared__ int s_in[kLevels * kMaxTopk];     // the anchor centre lies more than 0.01 px inside the box

  int n = a.nbox[b];
  n = n < 0 ? 0 : (n > a.n_max ? a.n_max : n);
  const float H = a.img_dim[2 * b + 0];
  const float W = a.img_dim[2 * b + 1];
  const size_t bi = (size_t)b * a.n_max + i;
  RBox bx;
  bx.cls = -1;
  if (i < n) bx = load_box(a.boxes + bi * 5, H, W, a.C);
  if (bx.cls < 0) {                            // the whole workgroup: a skipped box has no candidates
    for (int t = tid; t < slots; t += 64 * kLevels) {
      if (a.cand_idx) a.cand_idx[bi * slots + t] = -1;
      if (a.cand_iou) a.cand_iou[bi * slots + t] = 0.f;
    }
    if (a.cand_thr && tid == 0) a.cand_thr[bi] = 0.0;
    return;
  }

  // ---- candidate cells of this wave's level -----------------------------------------------------
  const int S = a.S[lvl], s = a.strides[lvl];
  const float sf = (float)s;
  const int kl = min(topk, A * S * S);         // candidate anchors of the level
  const int kcell = (kl + A - 1) / A;          // ... which are these many nearest cells (<= S*S, <= kc)
  // the rounds run over the window of kc cells either side of the centre's cell, checked (atss_select.h);
  // the grid offset is 0: anchors sit at (u * s, v * s)
  unsigned long long mine = 0;
  atss_select_cells(kcell, a.kc, S, S, sf, [s](int q) { return (float)(q * s); }, bx.yc, bx.xc, lane, mine);

  // ---- IoU of the level's candidates: rank j is anchor j % A of the cell of rank j / A -------------
  const int myq = (int)(unsigned)mine;         // lane r < kcell: the cell of rank r
  for (int j0 = 0; j0 < topk; j0 += 64) {      // uniform over the wave: the shuffle needs every lane
    const int j = j0 + lane;
    const int r = j / A;
    const int q = __shfl(myq, r < 64 ? r : 0, 64);
    if (j < topk) {
      int idx = -1, in = 0;
      float iou = 0.f;
      if (j < kl) {
        const int an = j - r * A;
        const int u = q / S, v = q - (q / S) * S;
        const float c0f = (float)(u * s), c1f = (float)(v * s);
        const float ah = a.adims[(lvl * A + an) * 2], aw = a.adims[(lvl * A + an) * 2 + 1];
        const float ih = fmaxf(fminf(bx.y1, c0f + ah * 0.5f) - fmaxf(bx.y0, c0f - ah * 0.5f), 0.f);
        const float iw = fmaxf(fminf(bx.x1, c1f + aw * 0.5f) - fmaxf(bx.x0, c1f - aw * 0.5f), 0.f);
        const float inter = ih * iw;
        const float uni = (ah * aw + bx.area) - inter;
        iou = (float)((double)inter / (double)uni);
        const float t = c0f - bx.y0, bt = bx.y1 - c0f, l = c1f - bx.x0, rr = bx.x1 - c1f;
        in = (t > 0.01f && bt > 0.01f && l > 0.01f && rr > 0.01f) ? 1 : 0;
        idx = (a.off[lvl] + q) * A + an;
      }
      const int slot = lvl * topk + j;
      s_idx[slot] = idx;
      s_iou[slot] = iou;
      s_in[slot] = in;
    }
  }
  __syncthreads();

  // ---- threshold: float64, level-major then by rank; every thread sums the same LDS values ----------
  int cnt = 0;
  double sum = 0.0;
  for (int l = 0; l < kLevels; ++l) {
    const int k = min(topk, A * a.S[l] * a.S[l]);
    for (int j = 0; j < k; ++j) sum += (double)s_iou[l * topk + j];
    cnt += k;
  }
  const double mean = sum / (double)cnt;                 // cnt >= 5: every level has a cell
  double qq = 0.0;
  for (int l = 0; l < kLevels; ++l) {
    const int k = min(topk, A * a.S[l] * a.S[l]);
    for (int j = 0; j < k; ++j) {
      const double d = (double)s_iou[l * topk + j] - mean;
      qq += d * d;
    }
  }
  const double thr = mean + sqrt(qq / (double)(cnt - 1));
  if (a.cand_thr && tid == 0) a.cand_thr[bi] = thr;

  // ---- contest: every positive pair posts its key to its anchor ------------------------------------
  for (int t = tid; t < slots; t += 64 * kLevels) {
    const int idx = s_idx[t];
    const float iou = s_iou[t];
    if (a.cand_idx) a.cand_idx[bi * slots + t] = idx;
    if (a.cand_iou) a.cand_iou[bi * slots + t] = iou;
    if (idx >= 0 && s_in[t] && (double)iou >= thr) {
      const unsigned long long key = ((unsigned long long)__float_as_uint(iou) << 32) | (0xFFFFFFFFu - (unsigned)i);
      atomicMax(&a.keys[(size_t)b * a.P * A + idx], key);
    }
  }
}

// A workgroup owns kTileCells cells (level-major cell index p) = ncell * A consecutive target rows; a
// thread resolves rows tid, tid + 256, ...; the slab is staged in LDS and leaves as 16-byte stores.
__global__ void __launch_bounds__(kThreads) retina_atss_write_kernel(RAtssArgs a) {
  const int b = blockIdx.y;
  const int tid = threadIdx.x;
  const int A = a.A;
  extern __shared__ __attribute__((aligned(16))) float stage[];          // [ncell * A][8], then 5 counters
  int* lcount = reinterpret_cast<int*>(stage + kTileCells * A * 8);

  if (tid < 5) lcount[tid] = 0;
  __syncthreads();
  const float H = a.img_dim[2 * b + 0];
  const float W = a.img_dim[2 * b + 1];
  const int p0 = blockIdx.x * kTileCells;
  const int ncell = min(kTileCells, a.P - p0);
  const int rows = ncell * A;
  const unsigned long long* keys = a.keys + ((size_t)b * a.P + p0) * A;
  for (int r = tid; r < rows; r += kThreads) {
    const int cell = r / A, an = r - cell * A;
    f32x4 lo = {0.f, 0.f, 0.f, 0.f}, hi = {-1.f, 0.f, -1.f, 0.f};
    const unsigned long long key = keys[r];
    if (key != 0ull) {
      const int p = p0 + cell;
      int lvl = 0;
      while (lvl < 4 && p >= a.off[lvl + 1]) ++lvl;
      const int i = (int)(0xFFFFFFFFu - (unsigned)key);       // < n_max: only valid boxes post keys
      const RBox bx = load_box(a.boxes + ((size_t)b * a.n_max + i) * 5, H, W, a.C);
      const int q = p - a.off[lvl];
      const int S = a.S[lvl], s = a.strides[lvl];
      const int u = q / S, v = q - (q / S) * S;
      const float c0f = (float)(u * s), c1f = (float)(v * s);
      const float ah = a.adims[(lvl * A + an) * 2], aw = a.adims[(lvl * A + an) * 2 + 1];
      // cvl_retina_assign's linear box targets, in float64
      lo[0] = (float)(((double)c0f - (double)bx.yc) / (double)ah);
      lo[1] = (float)(((double)c1f - (double)bx.xc) / (double)aw);
      lo[2] = (float)((double)bx.hp / (double)ah);
      lo[3] = (float)((double)bx.wp / (double)aw);
      hi[0] = (float)bx.cls;
      hi[1] = __uint_as_float((unsigned)(key >> 32));
      hi[2] = (float)i;
      atomicAdd(&lcount[lvl], 1);
    }
    reinterpret_cast<f32x4*>(stage)[2 * r] = lo;
    reinterpret_cast<f32x4*>(stage)[2 * r + 1] = hi;
  }
  __syncthreads();
  if (tid < 5 && lcount[tid]) atomicAdd(&a.num_targets[b * 5 + tid], lcount[tid]);
  f32x4* out = reinterpret_cast<f32x4*>(a.targets + ((size_t)b * a.P + p0) * A * 8);
  for (int e = tid; e < rows * 2; e += kThreads) out[e] = reinterpret_cast<const f32x4*>(stage)[e];
}

// ---- loss ----------------------------------------------------------------------------------------
struct RAtssLossArgs {
  const float* reg;
  const float* cls;
  const float* tgt;
  const int32_t* ntgt;
  const float* img_w;
  double* partial;
  void* dreg;
  void* dcls;
  int ld_reg, ld_cls, ld_dreg, ld_dcls, dreg_bf16, dcls_bf16, reg_vec;
  int P, A, C, tiles;
  float grad_scale, alpha, gamma;
};

__device__ __forceinline__ int image_positives(const int32_t* ntgt, int b) {
  int n = 0;
#pragma unroll
  for (int l = 0; l < 5; ++l) n += ntgt[b * 5 + l];
  return n > 1 ? n : 1;
}

// V consecutive gradient values at element offset o: one 16-byte (fp32) or 8-byte (bf16) store for V = 4
template <int V>
__device__ __forceinline__ void store_grads(void* dst, size_t o, const float* g, int bf16) {
  if constexpr (V == 4) {
    if (bf16) {
      s16x4 v;
#pragma unroll
      for (int t = 0; t < 4; ++t) v[t] = (short)f32_to_bf16(g[t]);
      *reinterpret_cast<s16x4*>(reinterpret_cast<cvl_bf16*>(dst) + o) = v;
    } else {
      *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(dst) + o) = f32x4{g[0], g[1], g[2], g[3]};
    }
  } else {
#pragma unroll
    for (int t = 0; t < V; ++t) {
      if (bf16) reinterpret_cast<cvl_bf16*>(dst)[o + t] = f32_to_bf16(g[t]);
      else reinterpret_cast<float*>(dst)[o + t] = g[t];
    }
  }
}

// A workgroup owns kLossCells cells of one image: their A*8 target floats are staged in LDS with
// 16-byte loads; then the A*C contiguous logits of each prediction row are walked V channels per lane,
// consecutive lanes on consecutive channels (V = 4: 16-byte loads, when A*C, the leading dimensions and
// the pointers allow it), the class target formed from the anchor's label; then one thread per anchor
// does the four box elements of a positive.  No one-hot row exists anywhere.
template <int V>
__global__ void __launch_bounds__(kThreads) retina_atss_loss_kernel(RAtssLossArgs a) {
  extern __shared__ __attribute__((aligned(16))) float tg[];             // [ncell * A][8], then the block sums
  double* red = reinterpret_cast<double*>(tg + kLossCells * a.A * 8);    // [2][kThreads / 64]
  const int b = blockIdx.y, tid = threadIdx.x;
  const int A = a.A, C = a.C;
  const int p0 = blockIdx.x * kLossCells;
  const int ncell = min(kLossCells, a.P - p0);
  const int rows = ncell * A;
  const size_t cell0 = (size_t)b * a.P + p0;
  {
    const f32x4* src = reinterpret_cast<const f32x4*>(a.tgt + cell0 * A * 8);
    for (int e = tid; e < rows * 2; e += kThreads) reinterpret_cast<f32x4*>(tg)[e] = src[e];
  }
  __syncthreads();
  const float wb = a.img_w ? a.img_w[b] : 1.0f;
  const float gs = (a.grad_scale * wb) / (float)image_positives(a.ntgt, b);
  float s_cls = 0.f, s_reg = 0.f;
  // class part
  const int AC = A * C, ipr = AC / V;          // V divides A*C
  for (int it = tid; it < ncell * ipr; it += kThreads) {
    const int cell = it / ipr;
    const int ch = (it - cell * ipr) * V;
    int an = ch / C, c = ch - (ch / C) * C;
    const float* xp = a.cls + (cell0 + cell) * a.ld_cls + ch;
    float x[V], g[V];
    if constexpr (V == 4) {
      const f32x4 xv = *reinterpret_cast<const f32x4*>(xp);
      x[0] = xv[0]; x[1] = xv[1]; x[2] = xv[2]; x[3] = xv[3];
    } else {
      x[0] = xp[0];
    }
#pragma unroll
    for (int t = 0; t < V; ++t) {
      const float label = tg[(cell * A + an) * 8 + 4];
      float gg;
      s_cls += focal_term(label == (float)c ? 1.0f : 0.0f, x[t], a.alpha, a.gamma, &gg);
      g[t] = gg * gs;
      if (++c == C) { c = 0; ++an; }
    }
    if (a.dcls) store_grads<V>(a.dcls, (cell0 + cell) * a.ld_dcls + ch, g, a.dcls_bf16);
  }
  // box part: one thread per anchor
  for (int r = tid; r < rows; r += kThreads) {
    const int cell = r / A, an = r - cell * A;
    float g[4] = {0.f, 0.f, 0.f, 0.f};
    if (tg[r * 8 + 4] >= 0.f) {                // a positive anchor
      const float* xp = a.reg + (cell0 + cell) * a.ld_reg + an * 4;
      float x[4];
      if (a.reg_vec) {
        const f32x4 xv = *reinterpret_cast<const f32x4*>(xp);
        x[0] = xv[0]; x[1] = xv[1]; x[2] = xv[2]; x[3] = xv[3];
      } else {
        x[0] = xp[0]; x[1] = xp[1]; x[2] = xp[2]; x[3] = xp[3];
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float gg;
        s_reg += sl1_elem(tg[r * 8 + j], x[j], &gg);
        g[j] = gg * gs;
      }
    }
    if (a.dreg) {
      const size_t o = (cell0 + cell) * a.ld_dreg + an * 4;
      if (a.reg_vec) {
        store_grads<4>(a.dreg, o, g, a.dreg_bf16);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) store_grads<1>(a.dreg, o + j, g + j, a.dreg_bf16);
      }
    }
  }
  // the tile's float64 partial sums, in a fixed order
  const double v0 = warp_sum_d((double)s_cls), v1 = warp_sum_d((double)s_reg);
  const int w = tid >> 6, lane = tid & 63;
  if (lane == 0) { red[w] = v0; red[kThreads / 64 + w] = v1; }
  __syncthreads();
  if (tid < 2) {
    double sacc = 0.0;
    for (int k = 0; k < kThreads / 64; ++k) sacc += red[tid * (kThreads / 64) + k];
    a.partial[((size_t)b * a.tiles + blockIdx.x) * 2 + tid] = sacc;
  }
}

// losses[b][k] = (float)(wb * sum_i partial[b][i][k] / N_b): one 256-thread block per image; thread t sums
// tiles t, t + 256, ..., then a fixed-shape LDS tree (deterministic, no atomics)
__global__ void __launch_bounds__(kThreads) retina_atss_loss_finalize(const double* partial, const int32_t* ntgt,
                                                                      const float* img_w, float* losses, int tiles) {
  const int b = blockIdx.x, t = threadIdx.x;
  double s0 = 0.0, s1 = 0.0;
  for (int i = t; i < tiles; i += kThreads) {
    s0 += partial[((size_t)b * tiles + i) * 2];
    s1 += partial[((size_t)b * tiles + i) * 2 + 1];
  }
  __shared__ double red[2][kThreads];
  red[0][t] = s0;
  red[1][t] = s1;
  __syncthreads();
  for (int w = kThreads / 2; w > 0; w >>= 1) {
    if (t < w) {
      red[0][t] += red[0][t + w];
      red[1][t] += red[1][t + w];
    }
    __syncthreads();
  }
  if (t < 2) {
    const double wb = img_w ? (double)img_w[b] : 1.0;
    losses[b * 2 + t] = (float)(wb * red[t][0] / (double)image_positives(ntgt, b));
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" size_t cvl_retina_atss_workspace_size(int B, int P, int n_anchors) {
  if (B <= 0 || P <= 0 || n_anchors <= 0) return 0;
  return (size_t)B * (size_t)P * (size_t)n_anchors * sizeof(unsigned long long);
}

extern "C" int cvl_retina_atss_assign(const float* boxes, const int32_t* nbox, const float* img_dim, int B, int n_max,
                                      int pad, int num_classes, const float* anchor_dims, int n_anchors,
                                      const int32_t* strides, int topk, float* targets, int32_t* num_targets,
                                      int32_t* cand_idx, float* cand_iou, double* cand_thr, void* workspace,
                                      size_t workspace_bytes, cvl_stream_t stream) {
  CVL_CHECK_ARG(boxes && nbox && img_dim && anchor_dims && targets && num_targets && strides && workspace);
  CVL_CHECK_ARG(B > 0 && n_max > 0 && n_max <= kMaxBoxes);
  CVL_CHECK_ARG(pad > 0 && pad % 128 == 0);
  CVL_CHECK_ARG(num_classes >= 1 && num_classes <= 256);
  CVL_CHECK_ARG(n_anchors >= 1 && n_anchors <= kMaxAnchors);
  CVL_CHECK_ARG(topk >= 1 && topk <= kMaxTopk && (topk + n_anchors - 1) / n_anchors <= kMaxCells);
  CVL_CHECK_ARG(aligned16(targets) && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0);
  RAtssArgs a;
  a.boxes = boxes; a.nbox = nbox; a.img_dim = img_dim; a.adims = anchor_dims;
  a.targets = targets; a.num_targets = num_targets;
  a.keys = (unsigned long long*)workspace;
  a.cand_idx = cand_idx; a.cand_iou = cand_iou; a.cand_thr = cand_thr;
  a.n_max = n_max; a.C = num_classes; a.A = n_anchors; a.topk = topk;
  a.kc = (topk + n_anchors - 1) / n_anchors;
  a.off[0] = 0;
  for (int l = 0; l < 5; ++l) {
    CVL_CHECK_ARG(strides[l] > 0 && pad / strides[l] > 0 && pad % strides[l] == 0);
    a.strides[l] = strides[l];
    a.S[l] = pad / strides[l];
    a.off[l + 1] = a.off[l] + a.S[l] * a.S[l];
  }
  a.P = a.off[5];
  CVL_CHECK_ARG(workspace_bytes >= cvl_retina_atss_workspace_size(B, a.P, n_anchors));
  const size_t lds = (size_t)kTileCells * n_anchors * 8 * sizeof(float) + 32;
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(a.keys, 0, sizeof(unsigned long long) * (size_t)B * a.P * n_anchors, s) != hipSuccess)
    return cvl_launch_status();
  if (hipMemsetAsync(num_targets, 0, sizeof(int32_t) * 5 * B, s) != hipSuccess) return cvl_launch_status();
  hipLaunchKernelGGL(retina_atss_select_kernel, dim3(n_max, B), dim3(64 * kLevels), 0, s, a);
  int st = cvl_launch_status();
  if (st) return st;
  hipLaunchKernelGGL(retina_atss_write_kernel, dim3((a.P + kTileCells - 1) / kTileCells, B), dim3(kThreads), lds, s, a);
  return cvl_launch_status();
}

extern "C" size_t cvl_retina_atss_loss_workspace_size(int B, int P, int n_anchors) {
  if (B <= 0 || P <= 0 || n_anchors <= 0) return 0;
  return (size_t)B * ((size_t)(P + kLossCells - 1) / kLossCells) * 2 * sizeof(double);
}

extern "C" int cvl_retina_atss_loss(const float* reg_pred, int ld_reg, const float* cls_pred, int ld_cls,
                                    const float* targets, const int32_t* num_targets, const float* img_weight, int B,
                                    int P, int n_anchors, int num_classes, float grad_scale, float alpha, float gamma,
                                    float* losses, void* d_reg, int ld_dreg, int dreg_dtype, void* d_cls, int ld_dcls,
                                    int dcls_dtype, void* workspace, size_t workspace_bytes, cvl_stream_t stream) {
  CVL_CHECK_ARG(reg_pred && cls_pred && targets && num_targets && losses && workspace);
  CVL_CHECK_ARG(B > 0 && P > 0 && n_anchors >= 1 && n_anchors <= kMaxAnchors && num_classes >= 1 && num_classes <= 256);
  CVL_CHECK_ARG(workspace_bytes >= cvl_retina_atss_loss_workspace_size(B, P, n_anchors));
  CVL_CHECK_ARG(gamma >= 0.f);
  CVL_CHECK_ARG(ld_reg >= 4 * n_anchors && ld_cls >= n_anchors * num_classes);
  CVL_CHECK_ARG(!d_reg || ld_dreg >= 4 * n_anchors);
  CVL_CHECK_ARG(!d_cls || ld_dcls >= n_anchors * num_classes);
  CVL_CHECK_ARG((dreg_dtype == 0 || dreg_dtype == 1) && (dcls_dtype == 0 || dcls_dtype == 1));
  CVL_CHECK_ARG(aligned16(targets) && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0);
  RAtssLossArgs a;
  a.reg = reg_pred; a.cls = cls_pred; a.tgt = targets; a.ntgt = num_targets; a.img_w = img_weight;
  a.partial = (double*)workspace; a.dreg = d_reg; a.dcls = d_cls;
  a.ld_reg = ld_reg; a.ld_cls = ld_cls; a.ld_dreg = ld_dreg; a.ld_dcls = ld_dcls;
  a.dreg_bf16 = dreg_dtype; a.dcls_bf16 = dcls_dtype;
  a.P = P; a.A = n_anchors; a.C = num_classes;
  a.grad_scale = grad_scale; a.alpha = alpha; a.gamma = gamma;
  a.tiles = (P + kLossCells - 1) / kLossCells;
  // four channels per lane when every row of four starts on a 16-byte boundary (8 for a bf16 gradient)
  a.reg_vec = aligned16(reg_pred) && ld_reg % 4 == 0 && (!d_reg || (aligned16(d_reg) && ld_dreg % 4 == 0));
  const bool cls_vec = (n_anchors * num_classes) % 4 == 0 && aligned16(cls_pred) && ld_cls % 4 == 0 &&
                       (!d_cls || (aligned16(d_cls) && ld_dcls % 4 == 0));
  const size_t lds = (size_t)kLossCells * n_anchors * 8 * sizeof(float) + 2 * (kThreads / 64) * sizeof(double);
  hipStream_t s = (hipStream_t)stream;
  if (cls_vec) hipLaunchKernelGGL(retina_atss_loss_kernel<4>, dim3(a.tiles, B), dim3(kThreads), lds, s, a);
  else hipLaunchKernelGGL(retina_atss_loss_kernel<1>, dim3(a.tiles, B), dim3(kThreads), lds, s, a);
  int st = cvl_launch_status();
  if (st) return st;
  hipLaunchKernelGGL(retina_atss_loss_finalize, dim3(B), dim3(kThreads), 0, s, (const double*)workspace, num_targets,
                     img_weight, losses, a.tiles);
  return cvl_launch_status();
}
