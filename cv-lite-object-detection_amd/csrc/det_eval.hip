// Detection evaluation on MI355X: VOC AP (VOCdevkit VOCevaldet) and COCO-style mAP (pycocotools
// evaluateImg / accumulate, area range "all"), resident on the device.
//   cvl_eval_match   one batch of detections + ground truths -> per-detection records (score, class,
//                    order key, TP / ignored bit sets over the IoU thresholds) and npos[c]
//   cvl_eval_ap      the records sorted by (class, score descending, order key) -> ap [K][C] and the
//                    final TP counts
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

// ---- AP over one sorted class segment -------------------------------------------------------------
// recall levels reached by tp true positives out of np: #{k in [0, n] : k * np <= n * tp}
__device__ __forceinline__ int64_t levels(int64_t tp, int64_t np, int64_t n) {
  const int64_t q = (n * tp) / np;
  return (q > n ? n : q) + 1;
}

__global__ void __launch_bounds__(AT) eval_ap_kernel(const uint16_t* tpb, const uint16_t* igb, const int64_t* seg,
                                                     const int32_t* npos, int64_t n_records, int C, int mode,
                                                     double* ap, int32_t* tp_total) {
  __shared__ int s_tp[AT], s_fp[AT];
  __shared__ double s_mx[AT];
  const int c = blockIdx.x, k = blockIdx.y, tid = threadIdx.x;
  int64_t s = seg[c], e = seg[c + 1];
  s = s < 0 ? 0 : (s > n_records ? n_records : s);
  e = e < s ? s : (e > n_records ? n_records : e);
  const int64_t np = npos[c];

  // forward: the segment's TP / FP totals (ignored detections are skipped)
  int ltp = 0, lfp = 0;
  for (int64_t i = s + tid; i < e; i += AT) {
    if ((igb[i] >> k) & 1) continue;
    const int tp = (tpb[i] >> k) & 1;
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
  if (tid == 0) tp_total[(size_t)k * C + c] = (int32_t)rem_tp;
  if (np <= 0) {                                       // no positives: AP undefined, left out of the means
    if (tid == 0) ap[(size_t)k * C + c] = __longlong_as_double(0x7ff8000000000000LL);
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
      const int ig = in ? ((igb[i] >> k) & 1) : 1;
      tpj[j] = in ? ((tpb[i] >> k) & 1) : 0;
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
  if (tid == 0) ap[(size_t)k * C + c] = s_mx[0] / (mode == CVL_EVAL_AP_VOC12 ? (double)np : (double)(nlev + 1));
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
