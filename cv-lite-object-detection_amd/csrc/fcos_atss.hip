// ATSS target assignment for FCOS (Zhang et al., CVPR 2020) on gfx950 -- an extension beyond the
// reference, next to the FCOS papers' recipe in fcos_paper.hip, whose target norm and loss it feeds:
//   cvl_fcos_atss_assign   per box the topk grid points nearest its centre on every level, the IoU of
//                          their square anchors with the box, threshold mean + std of those IoUs;
//                          per cell the positive pair with the largest IoU wins
// The exact rule is stated in include/cvlite.h.  This file is compiled with -ffp-contract=off: the
// assignment is a fixed operation sequence that tests/fcos_atss_ref.py restates bit for bit.
//
// Three steps on the stream (plus two memset nodes: the contest keys and the per-level counters):
//   select   one workgroup per (image, box), one wave per level: topk rounds of a wave arg-min over the
//            (2 topk + 1)^2 window about the box centre, a separable check that no cell outside the
//            window can displace a selected one (else the rounds run over the whole level), the
//            anchor IoUs, the serial float64 statistics (every wave, from registers), and one 64-bit
//            integer atomicMax per positive pair into the cell's contest key (IoU bits << 32 | ~box)
//   write    per 256-cell tile: decode the winner, recompute its values, stage the [cells, 5+C] slab
//            in LDS and store it coalesced; positives per level by ballots and integer atomics
// Integer max and integer add are order-independent, so the result is bit-identical run to run.
#include "atss_select.h"
#include "cvl_common.h"

#include <math.h>

namespace {

constexpr int kMaxBoxes = 256;   // per image
constexpr int kMaxTopk = 16;
constexpr int kThreads = 256;
constexpr int kLevels = 5;

struct AtssArgs {
  const float* boxes;
  const int32_t* nbox;
  const float* img_dim;
  float* targets;
  int32_t* num_targets;
  unsigned long long* keys;      // [B][P] contest keys, cleared to 0
  int32_t* cand_cells;           // optional [B][n_max][5*topk]
  float* cand_iou;               // optional [B][n_max][5*topk]
  double* cand_thr;              // optional [B][n_max]
  int n_max, C, P, topk;
  float anchor_scale;
  int strides[5];
  int Hs[5], Ws[5], off[6];
};

struct AtssBox {
  float y0, y1, x0, x1, yc, xc, area;
  int cls;                       // < 0: the box is skipped
};

// Box corners in pixels: the operation order of fcos_paper_assign_kernel.  The label test is
// (int)label in [0, C) without converting a NaN.
__device__ __forceinline__ AtssBox load_box(const float* r, float H, float W, int C) {
  const float yc = r[0] * H, xc = r[1] * W, hp = r[2] * H, wp = r[3] * W;
  AtssBox bx;
  bx.yc = yc; bx.xc = xc;
  bx.y0 = yc - hp * 0.5f; bx.y1 = yc + hp * 0.5f;
  bx.x0 = xc - wp * 0.5f; bx.x1 = xc + wp * 0.5f;
  bx.area = hp * wp;
  const float lab = r[4];
  bx.cls = (lab > -1.0f && lab < (float)C && bx.area > 0.f) ? (int)lab : -1;
  return bx;
}

__global__ void __launch_bounds__(64 * kLevels) fcos_atss_select_kernel(AtssArgs a) {
  const int b = blockIdx.y, i = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, lvl = tid >> 6;
  const int topk = a.topk;
  const int slots = kLevels * topk;

  __shared__ int s_cell[kLevels * kMaxTopk];
  __shared__ float s_iou[kLevels * kMaxTopk];
  __shared__ int s_in[kLevels * kMaxTopk];     // the grid point lies more than 0.01 px inside the box

  int n = a.nbox[b];
  n = n < 0 ? 0 : (n > a.n_max ? a.n_max : n);
  const float H = a.img_dim[2 * b + 0];
  const float W = a.img_dim[2 * b + 1];
  const size_t bi = (size_t)b * a.n_max + i;
  AtssBox bx;
  bx.cls = -1;
  if (i < n) bx = load_box(a.boxes + bi * 5, H, W, a.C);
  if (bx.cls < 0) {                            // the whole workgroup: a skipped box has no candidates
    if (a.cand_cells && tid < slots) a.cand_cells[bi * slots + tid] = -1;
    if (a.cand_iou && tid < slots) a.cand_iou[bi * slots + tid] = 0.f;
    if (a.cand_thr && tid == 0) a.cand_thr[bi] = 0.0;
    return;
  }

  // ---- candidates of this wave's level ---------------------------------------------------------
  const int Hs = a.Hs[lvl], Ws = a.Ws[lvl];
  const float sf = (float)a.strides[lvl];
  const int k = min(topk, Hs * Ws);
  // the rounds run over the window of topk cells either side of the centre's cell, checked (atss_select.h)
  unsigned long long mine = 0;
  atss_select_cells(k, topk, Hs, Ws, sf, [sf](int q) { return ((float)q + 0.5f) * sf; }, bx.yc, bx.xc, lane, mine);

  // ---- anchor IoU of lane j's candidate ----------------------------------------------------------
  if (lane < topk) {
    const int slot = lvl * topk + lane;
    int cell = -1, in = 0;
    float iou = 0.f;
    if (lane < k) {
      const int q = (int)(unsigned)mine;
      const int cy = q / Ws, cx = q - (q / Ws) * Ws;
      const float gy = ((float)cy + 0.5f) * sf, gx = ((float)cx + 0.5f) * sf;
      const float ha = a.anchor_scale * sf * 0.5f;
      const float ih = fmaxf(fminf(bx.y1, gy + ha) - fmaxf(bx.y0, gy - ha), 0.f);
      const float iw = fmaxf(fminf(bx.x1, gx + ha) - fmaxf(bx.x0, gx - ha), 0.f);
      const float inter = ih * iw;
      const float uni = ((ha + ha) * (ha + ha) + bx.area) - inter;
      iou = (float)((double)inter / (double)uni);
      const float t = gy - bx.y0, bt = bx.y1 - gy, l = gx - bx.x0, r = bx.x1 - gx;
      in = (t > 0.01f && bt > 0.01f && l > 0.01f && r > 0.01f) ? 1 : 0;
      cell = a.off[lvl] + q;
    }
    s_cell[slot] = cell;
    s_iou[slot] = iou;
    s_in[slot] = in;
  }
  __syncthreads();

  // ---- threshold: float64, level-major then by rank ---------------------------------------------
  // Every wave computes it, redundantly: the slots' IoUs sit in two registers per lane (slots 0..63
  // and 64..79) and are read back one at a time with a uniform lane index, so the serial sum has the
  // stated order without a chain of LDS reads.  Only the k_l real candidates of a level are visited.
  const float iou_lo = lane < slots ? s_iou[lane] : 0.f;
  const float iou_hi = 64 + lane < slots ? s_iou[64 + lane] : 0.f;
  auto slot_iou = [&](int s) {
    const int bits = s < 64 ? __builtin_amdgcn_readlane(__float_as_int(iou_lo), s)
                            : __builtin_amdgcn_readlane(__float_as_int(iou_hi), s - 64);
    return (double)__int_as_float(bits);
  };
  int cnt = 0;
  double sum = 0.0;
  for (int l = 0; l < kLevels; ++l) {
    const int kl = min(topk, a.Hs[l] * a.Ws[l]);
    for (int j = 0; j < kl; ++j) sum += slot_iou(l * topk + j);
    cnt += kl;
  }
  const double mean = sum / (double)cnt;                 // cnt >= 5: every level has a cell
  double q = 0.0;
  for (int l = 0; l < kLevels; ++l) {
    const int kl = min(topk, a.Hs[l] * a.Ws[l]);
    for (int j = 0; j < kl; ++j) {
      const double d = slot_iou(l * topk + j) - mean;
      q += d * d;
    }
  }
  const double thr = mean + sqrt(q / (double)(cnt - 1));
  if (a.cand_thr && tid == 0) a.cand_thr[bi] = thr;

  // ---- contest: every positive pair posts its key to its cell --------------------------------------
  if (tid < slots) {
    const int cell = s_cell[tid];
    const float iou = s_iou[tid];
    if (a.cand_cells) a.cand_cells[bi * slots + tid] = cell;
    if (a.cand_iou) a.cand_iou[bi * slots + tid] = iou;
    if (cell >= 0 && s_in[tid] && (double)iou >= thr) {
      const unsigned long long key = ((unsigned long long)__float_as_uint(iou) << 32) | (0xFFFFFFFFu - (unsigned)i);
      atomicMax(&a.keys[(size_t)b * a.P + cell], key);
    }
  }
}

// One thread per cell of a blockDim.x-cell tile (level-major cell index p); the tile's [ncell, 5+C]
// slab is staged in LDS and written out coalesced (the shape of fcos_paper_assign_kernel).
__global__ void __launch_bounds__(kThreads) fcos_atss_write_kernel(AtssArgs a) {
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
      const AtssBox bx = load_box(a.boxes + ((size_t)b * a.n_max + i) * 5, H, W, C);
      const int q = p - a.off[lvl];
      const int Ws = a.Ws[lvl];
      const int cy = q / Ws, cx = q - (q / Ws) * Ws;
      const float sf = (float)a.strides[lvl];
      const float gy = ((float)cy + 0.5f) * sf, gx = ((float)cx + 0.5f) * sf;
      const float t = gy - bx.y0, bt = bx.y1 - gy, l = gx - bx.x0, r = bx.x1 - gx;
      v0 = t / sf; v1 = bt / sf; v2 = l / sf; v3 = r / sf;
      const double dt = t, db = bt, dl = l, dr = r;
      v4 = (float)sqrt((fmin(dt, db) / fmax(dt, db)) * (fmin(dl, dr) / fmax(dl, dr)));
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

}  // namespace

extern "C" size_t cvl_fcos_atss_workspace_size(int B, int P) {
  if (B <= 0 || P <= 0) return 0;
  return (size_t)B * (size_t)P * sizeof(unsigned long long);
}

extern "C" int cvl_fcos_atss_assign(const float* boxes, const int32_t* nbox, const float* img_dim, int B, int n_max,
                                    int pad_h, int pad_w, int num_classes, const int32_t* strides, int topk,
                                    float anchor_scale, float* targets, int32_t* num_targets, int32_t* cand_cells,
                                    float* cand_iou, double* cand_thr, void* workspace, size_t workspace_bytes,
                                    cvl_stream_t stream) {
  CVL_CHECK_ARG(boxes && nbox && img_dim && targets && num_targets && strides && workspace);
  CVL_CHECK_ARG(B > 0 && n_max > 0 && n_max <= kMaxBoxes && pad_h > 0 && pad_w > 0);
  CVL_CHECK_ARG(num_classes > 0 && num_classes <= 256);
  CVL_CHECK_ARG(topk >= 1 && topk <= kMaxTopk);
  CVL_CHECK_ARG(anchor_scale > 0.f);
  CVL_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 7) == 0);
  AtssArgs a;
  a.boxes = boxes; a.nbox = nbox; a.img_dim = img_dim; a.targets = targets; a.num_targets = num_targets;
  a.keys = (unsigned long long*)workspace;
  a.cand_cells = cand_cells; a.cand_iou = cand_iou; a.cand_thr = cand_thr;
  a.n_max = n_max; a.C = num_classes; a.topk = topk; a.anchor_scale = anchor_scale;
  a.off[0] = 0;
  for (int l = 0; l < 5; ++l) {
    CVL_CHECK_ARG(strides[l] > 0);
    a.strides[l] = strides[l];
    a.Hs[l] = pad_h / strides[l];
    a.Ws[l] = pad_w / strides[l];
    CVL_CHECK_ARG(a.Hs[l] > 0 && a.Ws[l] > 0);
    a.off[l + 1] = a.off[l] + a.Hs[l] * a.Ws[l];
  }
  a.P = a.off[5];
  CVL_CHECK_ARG(workspace_bytes >= cvl_fcos_atss_workspace_size(B, a.P));
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
  hipLaunchKernelGGL(fcos_atss_select_kernel, dim3(n_max, B), dim3(64 * kLevels), 0, s, a);
  int st = cvl_launch_status();
  if (st) return st;
  hipLaunchKernelGGL(fcos_atss_write_kernel, dim3((a.P + nth - 1) / nth, B), dim3(nth), lds, s, a);
  return cvl_launch_status();
}
