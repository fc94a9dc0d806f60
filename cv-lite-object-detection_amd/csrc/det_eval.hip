// Detection evaluation on MI355X: VOC AP (VOCdevkit VOCevaldet) and COCO-style mAP (pycocotools
// evaluateImg / accumulate, area range "all"), resident on the device.
//   cvl_eval_match   one batch of detections + ground truths -> per-detection records (score, class,
//                    order key, TP / ignored bit sets over the IoU thresholds) and npos[c]
//   cvl_eval_ap      the records sorted by (class, score descending, order key) -> ap [K][C] and the
//                    final TP counts
//   cvl_eval_match_areas   the COCO matching once per area range (pycocotools evaluateImg per areaRng):
//                    bit sets [n][A], the rank of each detection inside its (image, class), npos [A][C]
//   cvl_eval_ap_views      the COCO AP walk over R (area range, rank prefix) views in one launch: the
//                    small / medium / large ranges and AR@1 / 10 / 100
// The reference publishes no evaluator; the semantics are the project's own contract
// (INTEGRATION.md "Evaluation"), restated in numpy by tests/eval_ref.py.
//
// Arithmetic: IoU in float64 from the fp32 corners, one IEEE operation per step (this file is built
// with -ffp-contract=off): ih = max(0, min(y2d, y2g) - max(y1d, y1g)), iw likewise, inter = ih * iw,
// ad = (y2d - y1d) * (x2d - x1d), ag likewise, iou = inter / ((ad + ag) - inter), 0 when the
// denominator is <= 0; against a COCO crowd iou = inter / ad, 0 when ad <= 0.  Boxes are continuous:
// there is no "+1 pixel" as in the VOC devkit.  max(a, b) / min(a, b) are "b if b > a else a" /
// "b if b < a else a".  Recall levels are compared in integers: a point reaches k / n iff
// n * tp >= k * npos.
#include "cvl_common.h"

namespace {

constexpr int MT = 256;                      // match workgroup (one per image)
constexpr int AT = 256;                      // AP workgroup (one per (class, threshold))
constexpr int ITEMS = 4;                     // records per thread and chunk
constexpr int CHUNK = AT * ITEMS;            // = CVL_EVAL_AP_CHUNK

static_assert(CHUNK == CVL_EVAL_AP_CHUNK, "header constant out of date");

struct MatchArgs {
  const float* boxes;
  const float* scores;
  const float* classes;
  const int32_t* valid;
  const float* gt_boxes;
  const int32_t* gt_labels;
  const uint8_t* gt_flags;
  const int32_t* gt_count;
  const int64_t* image_ids;
  float* rec_score;
  int32_t* rec_class;
  int64_t* rec_key;
  uint16_t* rec_tp;
  uint16_t* rec_ign;
  int32_t* npos;
  int64_t rec_offset;
  int T, G, C, K, protocol, max_dets;
  double thr[CVL_EVAL_MAX_THRESHOLDS];
};

__device__ __forceinline__ double dmax(double a, double b) { return b > a ? b : a; }
__device__ __forceinline__ double dmin(double a, double b) { return b < a ? b : a; }

__device__ __forceinline__ double box_iou(const float* d, const float* g, bool crowd) {
  const double y1d = d[0], x1d = d[1], y2d = d[2], x2d = d[3];
  const double y1g = g[0], x1g = g[1], y2g = g[2], x2g = g[3];
  const double ih = dmax(0.0, dmin(y2d, y2g) - dmax(y1d, y1g));
  const double iw = dmax(0.0, dmin(x2d, x2g) - dmax(x1d, x1g));
  const double inter = ih * iw;
  const double ad = (y2d - y1d) * (x2d - x1d);
  if (crowd) return ad <= 0.0 ? 0.0 : inter / ad;
  const double ag = (y2g - y1g) * (x2g - x1g);
  const double den = (ad + ag) - inter;
  return den <= 0.0 ? 0.0 : inter / den;
}

// LDS carve-up of the match kernel, in bytes: 4-byte elements first, then 2-byte, then bytes, so every
// piece is aligned to its element (the host sizes the launch by the same function).
struct MatchLds {
  size_t gbox, dscore, glab, dcls, present, bits, order, crank, gflag, used, total;
};
__host__ __device__ inline MatchLds match_lds(int T, int G, int K) {
  MatchLds m;
  size_t o = 0;
  m.gbox = o;    o += (size_t)G * 16;
  m.dscore = o;  o += (size_t)T * 4;
  m.glab = o;    o += (size_t)G * 4;
  m.dcls = o;    o += (size_t)T * 4;
  m.present = o; o += (size_t)T * 4;
  m.bits = o;    o += (size_t)T * 4;
  m.order = o;   o += (size_t)T * 2;
  m.crank = o;   o += (size_t)T * 2;
  m.gflag = o;   o += (size_t)G;
  m.used = o;    o += (size_t)K * G;
  m.total = (o + 15) & ~(size_t)15;
  return m;
}

__global__ void __launch_bounds__(MT) eval_match_kernel(MatchArgs a) {
  extern __shared__ __align__(16) unsigned char lds[];
  __shared__ int n_kept, n_present;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int T = a.T, G = a.G, C = a.C, K = a.K;
  const MatchLds m = match_lds(T, G, K);
  float* gbox = reinterpret_cast<float*>(lds + m.gbox);
  float* dscore = reinterpret_cast<float*>(lds + m.dscore);
  int32_t* glab = reinterpret_cast<int32_t*>(lds + m.glab);
  int32_t* dcls = reinterpret_cast<int32_t*>(lds + m.dcls);
  int32_t* present = reinterpret_cast<int32_t*>(lds + m.present);
  uint32_t* bits = reinterpret_cast<uint32_t*>(lds + m.bits);      // TP bits low half, ignored bits high half
  uint16_t* order = reinterpret_cast<uint16_t*>(lds + m.order);    // order[rank] = slot
  uint16_t* crank = reinterpret_cast<uint16_t*>(lds + m.crank);    // rank inside the slot's class
  uint8_t* gflag = lds + m.gflag;
  uint8_t* used = lds + m.used;                                    // [K][G]

  int nv = a.valid[b];
  nv = nv < 0 ? 0 : (nv > T ? T : nv);
  int ng = G > 0 ? a.gt_count[b] : 0;
  ng = ng < 0 ? 0 : (ng > G ? G : ng);
  if (tid == 0) { n_kept = 0; n_present = 0; }

  // ground truths of the image; labels outside [0, C) never match and are not counted
  for (int g = tid; g < ng; g += MT) {
    const float* p = a.gt_boxes + ((size_t)b * G + g) * 4;
    gbox[4 * g + 0] = p[0]; gbox[4 * g + 1] = p[1]; gbox[4 * g + 2] = p[2]; gbox[4 * g + 3] = p[3];
    int lab = a.gt_labels[(size_t)b * G + g];
    if (lab < 0 || lab >= C) lab = -1;
    const uint8_t fl = (a.gt_flags != nullptr && a.gt_flags[(size_t)b * G + g] != 0) ? 1 : 0;
    glab[g] = lab;
    gflag[g] = fl;
    if (lab >= 0 && !fl) atomicAdd(&a.npos[lab], 1);
  }
  for (int i = tid; i < K * G; i += MT) used[i] = 0;
  // detections: dropped = past the valid count, NaN score, class outside [0, C)
  for (int t = tid; t < T; t += MT) {
    const float s = a.scores[(size_t)b * T + t];
    const float c = a.classes[(size_t)b * T + t];
    const bool keep = t < nv && !(s != s) && c >= 0.0f && c < (float)C;
    dcls[t] = keep ? (int32_t)c : -1;
    dscore[t] = keep ? s : 0.0f;
    bits[t] = 0u;
  }
  __syncthreads();

  // rank by counting: score descending, lower slot first among equal scores
  for (int t = tid; t < T; t += MT) {
    const int c = dcls[t];
    if (c < 0) continue;
    const float s = dscore[t];
    int r = 0, rc = 0;
    for (int u = 0; u < T; ++u) {
      const int cu = dcls[u];
      if (cu < 0) continue;
      const float su = dscore[u];
      const int before = (su > s || (su == s && u < t)) ? 1 : 0;
      r += before;
      rc += (cu == c) ? before : 0;
    }
    order[r] = (uint16_t)t;
    crank[t] = (uint16_t)rc;
    atomicAdd(&n_kept, 1);
    if (rc == 0) present[atomicAdd(&n_present, 1)] = c;
  }
  __syncthreads();
  // COCO: at most max_dets detections per (image, class); the rest are dropped
  if (a.protocol == CVL_EVAL_COCO) {
    for (int t = tid; t < T; t += MT)
      if (dcls[t] >= 0 && (int)crank[t] >= a.max_dets) { dcls[t] = -1; dscore[t] = 0.0f; }
    __syncthreads();
  }

  // one lane per (class present, threshold): its own greedy chain over the ranked detections
  const int nk = n_kept, npairs = n_present * K;
  for (int pair = tid; pair < npairs; pair += MT) {
    const int c = present[pair / K], k = pair - (pair / K) * K;
    const double thr = a.thr[k];
    uint8_t* usedk = used + (size_t)k * G;
    for (int r = 0; r < nk; ++r) {
      const int t = order[r];
      if (dcls[t] != c) continue;
      const float* dp = a.boxes + ((size_t)b * T + t) * 4;
      const float d[4] = {dp[0], dp[1], dp[2], dp[3]};
      int mres = 0;                           // 0 FP, 1 TP, 2 ignored
      if (a.protocol == CVL_EVAL_VOC) {
        double ovmax = -1.0;                  // IoU >= 0: the first ground truth of the class always enters
        int jmax = -1;
        for (int g = 0; g < ng; ++g) {
          if (glab[g] != c) continue;
          const double ov = box_iou(d, gbox + 4 * g, false);
          if (ov > ovmax) { ovmax = ov; jmax = g; }
        }
        if (jmax >= 0 && ovmax >= thr) {
          if (gflag[jmax]) mres = 2;
          else if (!usedk[jmax]) { mres = 1; usedk[jmax] = 1; }
        }
      } else {
        double best = dmin(thr, 1.0 - 1e-10);
        int mg = -1;
        for (int pass = 0; pass < 2; ++pass) {          // non-crowd first, then crowd
          if (pass == 1 && mg >= 0) break;              // a non-crowd match is not displaced by a crowd
          for (int g = 0; g < ng; ++g) {
            if (glab[g] != c || (int)gflag[g] != pass) continue;
            if (pass == 0 && usedk[g]) continue;
            const double ov = box_iou(d, gbox + 4 * g, pass == 1);
            if (ov < best) continue;
            best = ov;
            mg = g;
          }
        }
        if (mg >= 0) {
          usedk[mg] = 1;
          mres = gflag[mg] ? 2 : 1;
        }
      }
      if (mres == 1) atomicOr(&bits[t], 1u << k);
      else if (mres == 2) atomicOr(&bits[t], 1u << (16 + k));
    }
  }
  __syncthreads();

  const int64_t id = a.image_ids[b];
  for (int t = tid; t < T; t += MT) {
    const int64_t i = a.rec_offset + (int64_t)b * T + t;
    const int c = dcls[t];
    a.rec_score[i] = dscore[t];
    a.rec_class[i] = c >= 0 ? c : C;
    a.rec_key[i] = (int64_t)(((uint64_t)id << 32) | (uint32_t)t);
    a.rec_tp[i] = (uint16_t)(bits[t] & 0xffffu);
    a.rec_ign[i] = (uint16_t)(bits[t] >> 16);
  }
}

// ---- COCO matching per area range ------------------------------------------------------------------
// cvl_eval_match's COCO chain once per area range.  One lane per (class present, threshold), as above,
// but a lane no longer scans every ranked detection and every ground truth for its class: the
// detections of a class are linked in rank order (dhead / dnext) and its ground truths in the given
// order (ghead / gnext), so the lanes of a wave step through their own classes' lists side by side.
// Per detection the lane walks the A ranges serially: bit a of the used byte [K][G] is range a's used
// flag (a byte belongs to one (class, threshold), so to one lane), a ground truth's flag byte holds
// crowd (bit 0) and "area outside range a" (bit 1 + a), and the detection bits are one word per (slot,
// range).  Class values and links are uint16 (0xffff = none; num_classes <= 65535, T, G <= 1024) and
// the scores, needed for the ranking only, lie where the detection bits go afterwards: the carve-up
// is 63 KiB at T = G = 1024, K = 16, A = 4, inside the 64 KiB a workgroup has without raising the
// kernel's dynamic-LDS limit.
struct MatchAreaArgs {
  MatchArgs m;
  const float* gt_area;
  const float* area_scale;
  uint16_t* rec_rank;
  int A;
  double lo[CVL_EVAL_MAX_AREAS], hi[CVL_EVAL_MAX_AREAS];
};

constexpr uint16_t NONE = 0xffff;
constexpr size_t LDS_DEFAULT = 64 * 1024;              // per workgroup, static + dynamic, without opting in to more

struct MatchAreaLds {
  size_t gbox, bits, glab, gnext, ghead, dcls, crank, dnext, dhead, gflag, used, total;
};
__host__ __device__ inline MatchAreaLds match_area_lds(int T, int G, int K, int A) {
  MatchAreaLds m;
  size_t o = 0;
  m.gbox = o;    o += (size_t)G * 16;
  m.bits = o;    o += (size_t)T * A * 4;               // the first T * 4 bytes: the scores, until the ranking is done
  m.glab = o;    o += (size_t)G * 2;
  m.gnext = o;   o += (size_t)G * 2;
  m.ghead = o;   o += (size_t)T * 2;
  m.dcls = o;    o += (size_t)T * 2;
  m.crank = o;   o += (size_t)T * 2;
  m.dnext = o;   o += (size_t)T * 2;
  m.dhead = o;   o += (size_t)T * 2;
  m.gflag = o;   o += (size_t)G;
  m.used = o;    o += (size_t)K * G;
  m.total = (o + 15) & ~(size_t)15;
  return m;
}

__global__ void __launch_bounds__(MT) eval_match_areas_kernel(MatchAreaArgs aa) {
  extern __shared__ __align__(16) unsigned char lds[];
  __shared__ int n_present;
  __shared__ double lo[CVL_EVAL_MAX_AREAS], hi[CVL_EVAL_MAX_AREAS];
  const MatchArgs& a = aa.m;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int T = a.T, G = a.G, C = a.C, K = a.K, A = aa.A;
  const MatchAreaLds m = match_area_lds(T, G, K, A);
  float* gbox = reinterpret_cast<float*>(lds + m.gbox);
  uint32_t* bits = reinterpret_cast<uint32_t*>(lds + m.bits);      // [T][A]: TP bits low half, ignored bits high half
  float* dscore = reinterpret_cast<float*>(lds + m.bits);          // [T], dead before bits is zeroed
  uint16_t* glab = reinterpret_cast<uint16_t*>(lds + m.glab);
  uint16_t* gnext = reinterpret_cast<uint16_t*>(lds + m.gnext);    // the next ground truth of the same class
  uint16_t* ghead = reinterpret_cast<uint16_t*>(lds + m.ghead);    // [present class]: its first ground truth
  uint16_t* dcls = reinterpret_cast<uint16_t*>(lds + m.dcls);
  uint16_t* crank = reinterpret_cast<uint16_t*>(lds + m.crank);    // rank inside the slot's class
  uint16_t* dnext = reinterpret_cast<uint16_t*>(lds + m.dnext);    // the slot ranked next in the same class
  uint16_t* dhead = reinterpret_cast<uint16_t*>(lds + m.dhead);    // [present class]: its best-ranked slot
  uint8_t* gflag = lds + m.gflag;                                  // bit 0 crowd, bit 1 + a: area outside range a
  uint8_t* used = lds + m.used;                                    // [K][G], bit a: used in range a

  int nv = a.valid[b];
  nv = nv < 0 ? 0 : (nv > T ? T : nv);
  int ng = G > 0 ? a.gt_count[b] : 0;
  ng = ng < 0 ? 0 : (ng > G ? G : ng);
  if (tid == 0) n_present = 0;
  if (tid < CVL_EVAL_MAX_AREAS) { lo[tid] = aa.lo[tid]; hi[tid] = aa.hi[tid]; }
  __syncthreads();
  const bool scaled = aa.area_scale != nullptr;
  const double scale = scaled ? (double)aa.area_scale[b] : 1.0;

  // ground truths of the image; labels outside [0, C) never match and are not counted
  for (int g = tid; g < ng; g += MT) {
    const float* p = a.gt_boxes + ((size_t)b * G + g) * 4;
    const float y1 = p[0], x1 = p[1], y2 = p[2], x2 = p[3];
    gbox[4 * g + 0] = y1; gbox[4 * g + 1] = x1; gbox[4 * g + 2] = y2; gbox[4 * g + 3] = x2;
    int lab = a.gt_labels[(size_t)b * G + g];
    if (lab < 0 || lab >= C) lab = -1;
    const bool crowd = a.gt_flags != nullptr && a.gt_flags[(size_t)b * G + g] != 0;
    double ag;
    if (aa.gt_area != nullptr) {
      ag = (double)aa.gt_area[(size_t)b * G + g];
    } else {
      ag = ((double)y2 - (double)y1) * ((double)x2 - (double)x1);
      if (scaled) ag = ag * scale;
    }
    uint8_t fl = crowd ? 1 : 0;
    for (int r = 0; r < A; ++r) {
      const bool outside = ag < lo[r] || ag > hi[r];
      if (outside) fl |= (uint8_t)(2u << r);
      if (lab >= 0 && !crowd && !outside) atomicAdd(&a.npos[(size_t)r * C + lab], 1);
    }
    glab[g] = lab >= 0 ? (uint16_t)lab : NONE;
    gflag[g] = fl;
  }
  for (int i = tid; i < K * G; i += MT) used[i] = 0;
  // detections: dropped = past the valid count, NaN score, class outside [0, C)
  for (int t = tid; t < T; t += MT) {
    const float s = a.scores[(size_t)b * T + t];
    const float c = a.classes[(size_t)b * T + t];
    const bool keep = t < nv && !(s != s) && c >= 0.0f && c < (float)C;
    dcls[t] = keep ? (uint16_t)(int32_t)c : NONE;
    dscore[t] = keep ? s : 0.0f;
    crank[t] = NONE;
  }
  __syncthreads();

  for (int g = tid; g < ng; g += MT) {
    const uint16_t lab = glab[g];
    int nx = g + 1;
    while (nx < ng && glab[nx] != lab) ++nx;
    gnext[g] = nx < ng ? (uint16_t)nx : NONE;
  }
  // rank by counting: score descending, lower slot first among equal scores; the slot ranked next in
  // the class is the best of those ranked after this one
  for (int t = tid; t < T; t += MT) {
    const uint16_t c = dcls[t];
    if (c == NONE) continue;
    const float s = dscore[t];
    int rc = 0, nx = -1;
    float sn = 0.0f;
    for (int u = 0; u < T; ++u) {
      if (dcls[u] != c || u == t) continue;
      const float su = dscore[u];
      if (su > s || (su == s && u < t)) {
        ++rc;
      } else if (nx < 0 || su > sn || (su == sn && u < nx)) {
        nx = u;
        sn = su;
      }
    }
    crank[t] = (uint16_t)rc;
    dnext[t] = nx >= 0 ? (uint16_t)nx : NONE;
    if (rc == 0) {
      const int p = atomicAdd(&n_present, 1);
      int g = 0;
      while (g < ng && glab[g] != c) ++g;
      dhead[p] = (uint16_t)t;
      ghead[p] = g < ng ? (uint16_t)g : NONE;
    }
  }
  __syncthreads();
  // the scores are done with: their place becomes the detection bits.  At most max_dets detections
  // per (image, class), the same cut for every range: the slots past it are dropped
  for (int i = tid; i < T * A; i += MT) bits[i] = 0u;
  for (int t = tid; t < T; t += MT)
    if (dcls[t] != NONE && (int)crank[t] >= a.max_dets) { dcls[t] = NONE; crank[t] = NONE; }
  __syncthreads();

  const int npairs = n_present * K;
  for (int pair = tid; pair < npairs; pair += MT) {
    const int p = pair / K, k = pair - (pair / K) * K;
    const double thr = a.thr[k];
    const int g0 = ghead[p];
    uint8_t* usedk = used + (size_t)k * G;
    int t = dhead[p];
    for (int i = 0; t != NONE && i < a.max_dets; ++i, t = dnext[t]) {
      const float* dp = a.boxes + ((size_t)b * T + t) * 4;
      const float d[4] = {dp[0], dp[1], dp[2], dp[3]};
      double ad = ((double)d[2] - (double)d[0]) * ((double)d[3] - (double)d[1]);
      if (scaled) ad = ad * scale;
      for (int ar = 0; ar < A; ++ar) {
        const uint8_t ubit = (uint8_t)(1u << ar), ibits = (uint8_t)(1u | (2u << ar));
        double best = dmin(thr, 1.0 - 1e-10);
        int mg = -1;
        for (int pass = 0; pass < 2; ++pass) {          // not ignored in this range first, then ignored
          if (pass == 1 && mg >= 0) break;              // a counted match is not displaced by an ignored one
          for (int g = g0; g != NONE; g = gnext[g]) {
            const uint8_t fl = gflag[g];
            if ((int)((fl & ibits) != 0) != pass) continue;
            const bool crowd = (fl & 1) != 0;
            if (!crowd && (usedk[g] & ubit)) continue;
            const double ov = box_iou(d, gbox + 4 * g, crowd);
            if (ov < best) continue;
            best = ov;
            mg = g;
          }
        }
        int mres;                                       // 0 FP, 1 TP, 2 ignored
        if (mg >= 0) {
          usedk[mg] |= ubit;
          mres = (gflag[mg] & ibits) ? 2 : 1;
        } else {
          mres = (ad < lo[ar] || ad > hi[ar]) ? 2 : 0;
        }
        if (mres == 1) atomicOr(&bits[(size_t)t * A + ar], 1u << k);
        else if (mres == 2) atomicOr(&bits[(size_t)t * A + ar], 1u << (16 + k));
      }
    }
  }
  __syncthreads();

  const int64_t id = a.image_ids[b];
  for (int t = tid; t < T; t += MT) {
    const int64_t i = a.rec_offset + (int64_t)b * T + t;
    const uint16_t c = dcls[t];
    a.rec_score[i] = c != NONE ? a.scores[(size_t)b * T + t] : 0.0f;
    a.rec_class[i] = c != NONE ? (int32_t)c : C;
    a.rec_key[i] = (int64_t)(((uint64_t)id << 32) | (uint32_t)t);
    aa.rec_rank[i] = crank[t];
    for (int ar = 0; ar < A; ++ar) {
      a.rec_tp[i * A + ar] = (uint16_t)(bits[(size_t)t * A + ar] & 0xffffu);
      a.rec_ign[i * A + ar] = (uint16_t)(bits[(size_t)t * A + ar] >> 16);
    }
  }
}

// ---- AP over one sorted class segment -------------------------------------------------------------
// recall levels reached by tp true positives out of np: #{k in [0, n] : k * np <= n * tp}
__device__ __forceinline__ int64_t levels(int64_t tp, int64_t np, int64_t n) {
  const int64_t q = (n * tp) / np;
  return (q > n ? n : q) + 1;
}

// Where a (class, threshold) walk reads its records: the plain bit sets of cvl_eval_ap, or one view of
// cvl_eval_ap_views (the bit sets of area range a, [n][A]; a record past the view's rank prefix counts
// as ignored).
struct PlainRecords {
  const uint16_t* tpb;
  const uint16_t* igb;
  int k;
  __device__ __forceinline__ int tp(int64_t i) const { return (tpb[i] >> k) & 1; }
  __device__ __forceinline__ int ignored(int64_t i) const { return (igb[i] >> k) & 1; }
};
struct ViewRecords {
  const uint16_t* tpb;
  const uint16_t* igb;
  const uint16_t* rank;
  int k, a, A, max_rank;
  __device__ __forceinline__ int tp(int64_t i) const { return (tpb[i * A + a] >> k) & 1; }
  __device__ __forceinline__ int ignored(int64_t i) const {
    return (((igb[i * A + a] >> k) & 1) != 0 || (int)rank[i] >= max_rank) ? 1 : 0;
  }
};

// One workgroup: AP and the final TP count of the records [seg[c], seg[c + 1]) against np positives.
template <class Records>
__device__ __forceinline__ void ap_segment(const Records rec, const int64_t* seg, int c, int64_t np,
                                           int64_t n_records, int mode, double* ap_out, int32_t* tp_out) {
  __shared__ int s_tp[AT], s_fp[AT];
  __shared__ double s_mx[AT];
  const int tid = threadIdx.x;
  int64_t s = seg[c], e = seg[c + 1];
  s = s < 0 ? 0 : (s > n_records ? n_records : s);
  e = e < s ? s : (e > n_records ? n_records : e);

  // forward: the segment's TP / FP totals (ignored detections are skipped)
  int ltp = 0, lfp = 0;
  for (int64_t i = s + tid; i < e; i += AT) {
    if (rec.ignored(i)) continue;
    const int tp = rec.tp(i);
    ltp += tp;
    lfp += 1 - tp;
  }
  s_tp[tid] = ltp;
  s_fp[tid] = lfp;
  __syncthreads();
  for (int o = AT / 2; o > 0; o >>= 1) {
    if (tid < o) { s_tp[tid] += s_tp[tid + o]; s_fp[tid] += s_fp[tid + o]; }
    __syncthreads();
  }
  int64_t rem_tp = s_tp[0], rem_fp = s_fp[0];          // cumulative counts at the end of the current chunk
  __syncthreads();
  if (tid == 0) *tp_out = (int32_t)rem_tp;
  if (np <= 0) {                                       // no positives: AP undefined, left out of the means
    if (tid == 0) *ap_out = __longlong_as_double(0x7ff8000000000000LL);
    return;
  }

  // backward in fixed chunks: suffix counts give each point's cumulative (tp, fp); the envelope is
  // the running maximum of the precision from the right
  const int64_t nlev = mode == CVL_EVAL_AP_COCO ? 100 : 10;
  const int64_t nchunks = (e - s + CHUNK - 1) / CHUNK;
  double carry = 0.0, acc = 0.0;
  for (int64_t ch = nchunks - 1; ch >= 0; --ch) {
    const int64_t base = s + ch * CHUNK + (int64_t)tid * ITEMS;
    int tpj[ITEMS], okj[ITEMS];
    int ctp = 0, cfp = 0;
#pragma unroll
    for (int j = 0; j < ITEMS; ++j) {
      const int64_t i = base + j;
      const bool in = i < e;
      const int ig = in ? rec.ignored(i) : 1;
      tpj[j] = in ? rec.tp(i) : 0;
      okj[j] = ig ? 0 : 1;
      ctp += okj[j] & tpj[j];
      cfp += okj[j] & (1 - tpj[j]);
    }
    // inclusive suffix sums over the threads
    s_tp[tid] = ctp;
    s_fp[tid] = cfp;
    __syncthreads();
    for (int o = 1; o < AT; o <<= 1) {
      const int at = tid + o < AT ? s_tp[tid + o] : 0;
      const int af = tid + o < AT ? s_fp[tid + o] : 0;
      __syncthreads();
      s_tp[tid] += at;
      s_fp[tid] += af;
      __syncthreads();
    }
    const int chunk_tp = s_tp[0], chunk_fp = s_fp[0];
    // cumulative counts at this thread's last item = end of chunk minus what later threads hold
    int64_t cum_tp = rem_tp - (s_tp[tid] - ctp);
    int64_t cum_fp = rem_fp - (s_fp[tid] - cfp);
    double prec[ITEMS], lmax[ITEMS];
    int64_t ctpj[ITEMS], cnj[ITEMS];
    double run = -1.0;
#pragma unroll
    for (int j = ITEMS - 1; j >= 0; --j) {
      ctpj[j] = cum_tp;
      cnj[j] = cum_tp + cum_fp;
      prec[j] = okj[j] ? (double)cum_tp / (double)(cum_tp + cum_fp) : -1.0;
      run = prec[j] > run ? prec[j] : run;
      lmax[j] = run;
      cum_tp -= okj[j] & tpj[j];
      cum_fp -= okj[j] & (1 - tpj[j]);
    }
    // inclusive suffix maximum over the threads
    s_mx[tid] = run;
    __syncthreads();
    for (int o = 1; o < AT; o <<= 1) {
      const double am = tid + o < AT ? s_mx[tid + o] : -1.0;
      __syncthreads();
      s_mx[tid] = am > s_mx[tid] ? am : s_mx[tid];
      __syncthreads();
    }
    const double later = tid + 1 < AT ? s_mx[tid + 1] : -1.0;
    const double chunk_mx = s_mx[0];
    const double outer = later > carry ? later : carry;
#pragma unroll
    for (int j = 0; j < ITEMS; ++j) {
      if (!okj[j]) continue;
      const double env = lmax[j] > outer ? lmax[j] : outer;
      if (mode == CVL_EVAL_AP_VOC12) {
        if (tpj[j]) acc += env;                        // (tp_i - tp_prev) * envelope_i; / npos at the end
      } else {
        // the levels whose first reaching point this is
        const int64_t prev = cnj[j] == 1 ? 0 : levels(ctpj[j] - tpj[j], np, nlev);
        const int64_t cnt = levels(ctpj[j], np, nlev) - prev;
        if (cnt > 0) acc += (double)cnt * env;
      }
    }
    rem_tp -= chunk_tp;
    rem_fp -= chunk_fp;
    carry = chunk_mx > carry ? chunk_mx : carry;
    __syncthreads();
  }
  s_mx[tid] = acc;
  __syncthreads();
  for (int o = AT / 2; o > 0; o >>= 1) {
    if (tid < o) s_mx[tid] += s_mx[tid + o];
    __syncthreads();
  }
  if (tid == 0) *ap_out = s_mx[0] / (mode == CVL_EVAL_AP_VOC12 ? (double)np : (double)(nlev + 1));
}

__global__ void __launch_bounds__(AT) eval_ap_kernel(const uint16_t* tpb, const uint16_t* igb, const int64_t* seg,
                                                     const int32_t* npos, int64_t n_records, int C, int mode,
                                                     double* ap, int32_t* tp_total) {
  const int c = blockIdx.x, k = blockIdx.y;
  const PlainRecords rec = {tpb, igb, k};
  ap_segment(rec, seg, c, (int64_t)npos[c], n_records, mode, ap + (size_t)k * C + c, tp_total + (size_t)k * C + c);
}

struct ApViews {
  int32_t area[CVL_EVAL_MAX_VIEWS], max_rank[CVL_EVAL_MAX_VIEWS];
};

// grid (class, threshold, view)
__global__ void __launch_bounds__(AT) eval_ap_views_kernel(const uint16_t* tpb, const uint16_t* igb,
                                                           const uint16_t* rank, const int64_t* seg,
                                                           const int32_t* npos, int64_t n_records, int C, int A,
                                                           ApViews v, double* ap, int32_t* tp_total) {
  const int c = blockIdx.x, k = blockIdx.y, r = blockIdx.z, K = gridDim.y;
  const int a = v.area[r];
  const ViewRecords rec = {tpb, igb, rank, k, a, A, v.max_rank[r]};
  const size_t o = ((size_t)r * K + k) * C + c;
  ap_segment(rec, seg, c, (int64_t)npos[(size_t)a * C + c], n_records, CVL_EVAL_AP_COCO, ap + o, tp_total + o);
}

}  // namespace

extern "C" int cvl_eval_match(const float* boxes, const float* scores, const float* classes, const int32_t* valid,
                              const float* gt_boxes, const int32_t* gt_labels, const uint8_t* gt_flags,
                              const int32_t* gt_count, const int64_t* image_ids, int B, int T, int G,
                              int num_classes, const double* thresholds, int K, int protocol, int max_dets,
                              float* rec_score, int32_t* rec_class, int64_t* rec_key, uint16_t* rec_tp,
                              uint16_t* rec_ign, int64_t rec_offset, int32_t* npos, cvl_stream_t stream) {
  CVL_CHECK_ARG(B >= 1 && B <= CVL_EVAL_MAX_B);
  CVL_CHECK_ARG(T >= 1 && T <= CVL_EVAL_MAX_T && G >= 0 && G <= CVL_EVAL_MAX_G);
  CVL_CHECK_ARG(K >= 1 && K <= CVL_EVAL_MAX_THRESHOLDS && thresholds != nullptr);
  CVL_CHECK_ARG(num_classes >= 1 && num_classes <= CVL_EVAL_MAX_CLASSES);
  CVL_CHECK_ARG(protocol == CVL_EVAL_VOC || protocol == CVL_EVAL_COCO);
  CVL_CHECK_ARG(max_dets >= 1 && rec_offset >= 0);
  CVL_CHECK_ARG(boxes && scores && classes && valid && image_ids && npos);
  CVL_CHECK_ARG(G == 0 || (gt_boxes && gt_labels && gt_count));
  CVL_CHECK_ARG(rec_score && rec_class && rec_key && rec_tp && rec_ign);
  MatchArgs a;
  a.boxes = boxes; a.scores = scores; a.classes = classes; a.valid = valid;
  a.gt_boxes = gt_boxes; a.gt_labels = gt_labels; a.gt_flags = gt_flags; a.gt_count = gt_count;
  a.image_ids = image_ids;
  a.rec_score = rec_score; a.rec_class = rec_class; a.rec_key = rec_key; a.rec_tp = rec_tp; a.rec_ign = rec_ign;
  a.npos = npos;
  a.rec_offset = rec_offset;
  a.T = T; a.G = G; a.C = num_classes; a.K = K; a.protocol = protocol; a.max_dets = max_dets;
  for (int k = 0; k < CVL_EVAL_MAX_THRESHOLDS; ++k) a.thr[k] = k < K ? thresholds[k] : 2.0;
  const size_t lds = match_lds(T, G, K).total;         // 57 KiB at the limits
  hipLaunchKernelGGL(eval_match_kernel, dim3(B), dim3(MT), lds, (hipStream_t)stream, a);
  return cvl_launch_status();
}

extern "C" int cvl_eval_ap(const uint16_t* rec_tp, const uint16_t* rec_ign, const int64_t* seg_offsets,
                           const int32_t* npos, int64_t n_records, int num_classes, int K, int mode, double* ap,
                           int32_t* tp_total, cvl_stream_t stream) {
  CVL_CHECK_ARG(n_records >= 0 && num_classes >= 1 && num_classes <= CVL_EVAL_MAX_CLASSES);
  CVL_CHECK_ARG(K >= 1 && K <= CVL_EVAL_MAX_THRESHOLDS);
  CVL_CHECK_ARG(mode == CVL_EVAL_AP_VOC07 || mode == CVL_EVAL_AP_VOC12 || mode == CVL_EVAL_AP_COCO);
  CVL_CHECK_ARG(seg_offsets && npos && ap && tp_total && (n_records == 0 || (rec_tp && rec_ign)));
  hipLaunchKernelGGL(eval_ap_kernel, dim3(num_classes, K), dim3(AT), 0, (hipStream_t)stream, rec_tp, rec_ign,
                     seg_offsets, npos, n_records, num_classes, mode, ap, tp_total);
  return cvl_launch_status();
}

extern "C" int cvl_eval_match_areas(const float* boxes, const float* scores, const float* classes,
                                    const int32_t* valid, const float* gt_boxes, const int32_t* gt_labels,
                                    const uint8_t* gt_flags, const int32_t* gt_count, const int64_t* image_ids, int B,
                                    int T, int G, int num_classes, const double* thresholds, int K, int protocol,
                                    int max_dets, const double* area_ranges, int A, const float* gt_area,
                                    const float* area_scale, float* rec_score, int32_t* rec_class, int64_t* rec_key,
                                    uint16_t* rec_tp, uint16_t* rec_ign, uint16_t* rec_rank, int64_t rec_offset,
                                    int32_t* npos, cvl_stream_t stream) {
  CVL_CHECK_ARG(B >= 1 && B <= CVL_EVAL_MAX_B);
  CVL_CHECK_ARG(T >= 1 && T <= CVL_EVAL_MAX_T && G >= 0 && G <= CVL_EVAL_MAX_G);
  CVL_CHECK_ARG(K >= 1 && K <= CVL_EVAL_MAX_THRESHOLDS && thresholds != nullptr);
  CVL_CHECK_ARG(A >= 1 && A <= CVL_EVAL_MAX_AREAS && area_ranges != nullptr);
  CVL_CHECK_ARG(num_classes >= 1 && num_classes <= CVL_EVAL_MAX_CLASSES);
  CVL_CHECK_ARG(protocol == CVL_EVAL_COCO);
  CVL_CHECK_ARG(max_dets >= 1 && rec_offset >= 0);
  CVL_CHECK_ARG(boxes && scores && classes && valid && image_ids && npos);
  CVL_CHECK_ARG(G == 0 || (gt_boxes && gt_labels && gt_count));
  CVL_CHECK_ARG(rec_score && rec_class && rec_key && rec_tp && rec_ign && rec_rank);
  MatchAreaArgs aa;
  MatchArgs& a = aa.m;
  a.boxes = boxes; a.scores = scores; a.classes = classes; a.valid = valid;
  a.gt_boxes = gt_boxes; a.gt_labels = gt_labels; a.gt_flags = gt_flags; a.gt_count = gt_count;
  a.image_ids = image_ids;
  a.rec_score = rec_score; a.rec_class = rec_class; a.rec_key = rec_key; a.rec_tp = rec_tp; a.rec_ign = rec_ign;
  a.npos = npos;
  a.rec_offset = rec_offset;
  a.T = T; a.G = G; a.C = num_classes; a.K = K; a.protocol = protocol; a.max_dets = max_dets;
  for (int k = 0; k < CVL_EVAL_MAX_THRESHOLDS; ++k) a.thr[k] = k < K ? thresholds[k] : 2.0;
  aa.gt_area = gt_area; aa.area_scale = area_scale; aa.rec_rank = rec_rank; aa.A = A;
  for (int r = 0; r < CVL_EVAL_MAX_AREAS; ++r) {
    aa.lo[r] = r < A ? area_ranges[2 * r] : 0.0;
    aa.hi[r] = r < A ? area_ranges[2 * r + 1] : 0.0;
  }
  const size_t lds = match_area_lds(T, G, K, A).total;  // 63 KiB at the limits (T = G = 1024, K = 16, A = 4)
  CVL_CHECK_ARG(lds + 256 <= LDS_DEFAULT);              // + the kernel's static variables; holds at the limits
  hipLaunchKernelGGL(eval_match_areas_kernel, dim3(B), dim3(MT), lds, (hipStream_t)stream, aa);
  return cvl_launch_status();
}

extern "C" int cvl_eval_ap_views(const uint16_t* rec_tp, const uint16_t* rec_ign, const uint16_t* rec_rank,
                                 const int64_t* seg_offsets, const int32_t* npos, int64_t n_records, int num_classes,
                                 int K, int A, const int32_t* views, int R, double* ap, int32_t* tp_total,
                                 cvl_stream_t stream) {
  CVL_CHECK_ARG(n_records >= 0 && num_classes >= 1 && num_classes <= CVL_EVAL_MAX_CLASSES);
  CVL_CHECK_ARG(K >= 1 && K <= CVL_EVAL_MAX_THRESHOLDS);
  CVL_CHECK_ARG(A >= 1 && A <= CVL_EVAL_MAX_AREAS && R >= 1 && R <= CVL_EVAL_MAX_VIEWS && views != nullptr);
  CVL_CHECK_ARG(seg_offsets && npos && ap && tp_total && (n_records == 0 || (rec_tp && rec_ign && rec_rank)));
  ApViews v;
  for (int r = 0; r < CVL_EVAL_MAX_VIEWS; ++r) {
    v.area[r] = r < R ? views[2 * r] : 0;
    v.max_rank[r] = r < R ? views[2 * r + 1] : 1;
    CVL_CHECK_ARG(v.area[r] >= 0 && v.area[r] < A && v.max_rank[r] >= 1);
  }
  hipLaunchKernelGGL(eval_ap_views_kernel, dim3(num_classes, K, R), dim3(AT), 0, (hipStream_t)stream, rec_tp,
                     rec_ign, rec_rank, seg_offsets, npos, n_records, num_classes, A, v, ap, tp_total);
  return cvl_launch_status();
}
