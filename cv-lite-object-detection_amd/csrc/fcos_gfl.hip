// Generalized Focal Loss for the FCOS head (Li et al., NeurIPS 2020) on gfx950 -- an extension beyond
// the reference, the step after the ATSS targets of fcos_atss.hip:
//   cvl_fcos_gfl_norm     (number of positives, sum of their sigmoid(max class logit)) per image
//   cvl_fcos_gfl_loss     Quality Focal Loss on the class logits (target = IoU of the decoded box),
//                         GIoU on the expectation of the per-side distributions, Distribution Focal
//                         Loss on the distributions; forward + backward in one pass
//   cvl_fcos_gfl_decode   the per-side expectations, the (t, b, l, r) that cvl_fcos_detect reads
// The exact rules are stated in include/cvlite.h.  This file is compiled with -ffp-contract=off, so
// the LDS-staged and the row-pointer form of the loss run one fp32 operation sequence per cell.
//
// Work: the loss is HBM read + write bound -- targets and class logits read once, both gradient rows
// written once; only the positive cells (a few per cent) read their 4(R+1) box logits, every other
// cell writes a zero box-gradient row.  The norm is one more read of the targets and class logits.
#include "cvl_common.h"
#include "fcos_focal.h"

#include <math.h>

namespace {

constexpr int kThreads = 256;
constexpr int kMaxRegMax = 16;
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

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

__device__ __forceinline__ float sigmoid_f(float x) {
  const float e = expf(-fabsf(x));
  return x >= 0.f ? 1.0f / (1.0f + e) : e / (1.0f + e);
}

// ---------------------------------------------------------------------------------------------
// one side's distribution: z(i), i = 0..R
// ---------------------------------------------------------------------------------------------
struct Side {
  float m, s, d, lse;   // max logit, sum exp(z - m), expectation sum i p_i, log-sum-exp
};

template <class ZF>
__device__ __forceinline__ Side side_forward(ZF z, int R) {
  Side o;
  o.m = z(0);
  for (int i = 1; i <= R; ++i) o.m = fmaxf(o.m, z(i));
  float s = 0.f, n = 0.f;
  for (int i = 0; i <= R; ++i) {
    const float e = expf(z(i) - o.m);
    s += e;
    n += (float)i * e;
  }
  o.s = s;
  o.d = n / s;
  o.lse = o.m + logf(s);
  return o;
}

// the DFL target of one side: the two bins about the clamped distance and their weights
struct Dfl {
  int il;
  float wl, wr, val;
};

template <class ZF>
__device__ __forceinline__ Dfl dfl_side(ZF z, int R, float t, float lse) {
  Dfl f;
  const float tc = fminf(fmaxf(t, 0.f), (float)R - 0.1f);
  const float yl = floorf(tc);
  f.il = (int)yl;
  f.wl = (yl + 1.0f) - tc;
  f.wr = tc - yl;
  f.val = f.wl * (lse - z(f.il)) + f.wr * (lse - z(f.il + 1));
  return f;
}

// gradient of one side's logits: gb * d(expectation)/dz + gd * d(DFL)/dz, written through put(i, g);
// z(i) is read before put(i, .), so both may name one buffer
template <class ZF, class PF>
__device__ __forceinline__ void side_backward(ZF z, PF put, int R, const Side& sd, const Dfl& f, float gb, float gd) {
  for (int i = 0; i <= R; ++i) {
    const float p = expf(z(i) - sd.m) / sd.s;
    const float hot = i == f.il ? f.wl : (i == f.il + 1 ? f.wr : 0.f);
    put(i, gb * (p * ((float)i - sd.d)) + gd * (p - hot));
  }
}

// GIoU of ltrb boxes about one grid point (the expressions of fcos_paper.hip's cell_rest) and its
// derivative in each predicted distance
struct Giou {
  float iou, giou, dG[4];
};

__device__ __forceinline__ Giou giou_terms(const float (&tt)[4], const float (&d)[4]) {
  Giou o;
  const float th = tt[0] + tt[1], tw = tt[2] + tt[3], ph = d[0] + d[1], pw = d[2] + d[3];
  const float ih = fminf(tt[0], d[0]) + fminf(tt[1], d[1]), iw = fminf(tt[2], d[2]) + fminf(tt[3], d[3]);
  const float eh = fmaxf(tt[0], d[0]) + fmaxf(tt[1], d[1]), ew = fmaxf(tt[2], d[2]) + fmaxf(tt[3], d[3]);
  const float I = ih * iw;
  const float U = th * tw + ph * pw - I + 1.0e-12f;
  const float E = eh * ew + 1.0e-12f;
  o.iou = I / U;
  o.giou = I / U - (E - U) / E;
  // GIoU = I/U - 1 + U/E
  const float dGdI = 1.0f / U, dGdU = 1.0f / E - I / (U * U), dGdE = -U / (E * E);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float oi = j < 2 ? iw : ih;      // the other side of the intersection
    const float op = j < 2 ? pw : ph;      // ... of the predicted box
    const float oe = j < 2 ? ew : eh;      // ... of the enclosing box
    const float dI = d[j] < tt[j] ? oi : 0.f;
    const float dE = d[j] > tt[j] ? oe : 0.f;
    o.dG[j] = dGdI * dI + dGdU * (op - dI) + dGdE * dE;
  }
  return o;
}

// ---------------------------------------------------------------------------------------------
// norm
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) fcos_gfl_norm_kernel(const float* cls, int ld_cls, const float* tgt,
                                                                 double* partial, int P, int C, int tiles) {
  const int p = blockIdx.x * kThreads + threadIdx.x;
  float s[2] = {0.f, 0.f};
  if (p < P) {
    const size_t cell = (size_t)blockIdx.y * P + p;
    const float* t = tgt + cell * (5 + C);
    float tmax = 0.f;
    for (int c = 0; c < C; ++c) tmax = fmaxf(tmax, t[5 + c]);
    if (tmax >= 1.0f) {
      const float* x = cls + cell * ld_cls;
      float xmax = x[0];
      for (int c = 1; c < C; ++c) xmax = fmaxf(xmax, x[c]);
      s[0] = 1.0f;
      s[1] = sigmoid_f(xmax);
    }
  }
  block_partials<kThreads, 2>(partial, tiles, s);
}

__global__ void fcos_gfl_norm_finalize(const double* partial, float* norm, int tiles) {
  const int b = blockIdx.x, k = threadIdx.x;
  if (k < 2) {
    double s = 0.0;
    for (int i = 0; i < tiles; ++i) s += partial[((size_t)b * tiles + i) * 2 + k];
    norm[b * 2 + k] = (float)s;
  }
}

// ---------------------------------------------------------------------------------------------
// loss
// ---------------------------------------------------------------------------------------------
struct GflLossArgs {
  const float* reg;
  const float* cls;
  const float* tgt;
  const float* norm;   // [B, 2] or null
  void* dreg;
  void* dcls;
  double* partial;     // [B, tiles, 3]
  int ld_reg, ld_cls, ld_dreg, ld_dcls, dreg_bf16, dcls_bf16;
  int P, C, R, tiles;
  float grad_scale, beta, w_box, w_dfl;
};

__device__ __forceinline__ void store_g(void* base, size_t idx, float v, int is_bf16) {
  if (is_bf16) reinterpret_cast<cvl_bf16*>(base)[idx] = f32_to_bf16(v);
  else reinterpret_cast<float*>(base)[idx] = v;
}

// the image's gradient factors: gn = grad_scale / N on the QFL terms, gbox = grad_scale w_box / Wsum and
// gdfl = grad_scale w_dfl / Wsum on the positives' terms (N = Wsum = 1 without a norm)
__device__ __forceinline__ void image_factors(const GflLossArgs& a, int b, float& gn, float& gbox, float& gdfl) {
  float N = 1.0f, Wsum = 1.0f;
  if (a.norm) {
    N = fmaxf(a.norm[2 * b], 1.0f);
    Wsum = fmaxf(a.norm[2 * b + 1], 1.0e-6f);
  }
  gn = a.grad_scale / N;
  gbox = a.grad_scale * a.w_box / Wsum;
  gdfl = a.grad_scale * a.w_dfl / Wsum;
}

// Row-pointer form (any C, any layout): a thread walks its cell's rows in global memory.  NTH is the
// tile of the LDS form it stands in for, so the per-tile partials are the same sums.
template <int NTH>
__global__ void __launch_bounds__(NTH) fcos_gfl_loss_rows_kernel(GflLossArgs a) {
  const int b = blockIdx.y;
  const int p = blockIdx.x * NTH + threadIdx.x;
  const int C = a.C, R = a.R, R1 = R + 1, NB = 4 * R1;
  float gn, gbox, gdfl;
  image_factors(a, b, gn, gbox, gdfl);
  float s[3] = {0.f, 0.f, 0.f};
  if (p < a.P) {
    const size_t cell = (size_t)b * a.P + p;
    const float* t = a.tgt + cell * (5 + C);
    const float* xc = a.cls + cell * a.ld_cls;
    const float* zr = a.reg + cell * a.ld_reg;
    float tmax = 0.f, xmax = -INFINITY;
    for (int c = 0; c < C; ++c) {
      tmax = fmaxf(tmax, t[5 + c]);
      xmax = fmaxf(xmax, xc[c]);
    }
    const bool pos = tmax >= 1.0f;
    float q = 0.f;
    if (pos) {
      Side sd[4];
      float tt[4], d[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float* z = zr + j * R1;
        sd[j] = side_forward([&](int i) { return z[i]; }, R);
        d[j] = sd[j].d;
        tt[j] = t[j];
      }
      const Giou G = giou_terms(tt, d);
      const float w = sigmoid_f(xmax);
      q = G.iou;
      float dv[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float* z = zr + j * R1;
        auto zf = [&](int i) { return z[i]; };
        const Dfl f = dfl_side(zf, R, tt[j], sd[j].lse);
        dv[j] = f.val;
        if (a.dreg)
          side_backward(zf, [&](int i, float g) { store_g(a.dreg, cell * a.ld_dreg + j * R1 + i, g, a.dreg_bf16); },
                        R, sd[j], f, -w * G.dG[j] * gbox, w * 0.25f * gdfl);
      }
      s[1] = w * (1.0f - G.giou);
      s[2] = w * (0.25f * (((dv[0] + dv[1]) + dv[2]) + dv[3]));
    } else if (a.dreg) {
      for (int i = 0; i < NB; ++i) store_g(a.dreg, cell * a.ld_dreg + i, 0.f, a.dreg_bf16);
    }
    for (int c = 0; c < C; ++c) {
      const float y = (pos && t[5 + c] >= 1.0f) ? q : 0.f;
      float g;
      s[0] += qfl_term(y, xc[c], a.beta, &g);
      if (a.dcls) store_g(a.dcls, cell * a.ld_dcls + c, g * gn, a.dcls_bf16);
    }
    if (a.dcls)
      for (int c = C; c < a.ld_dcls; ++c) store_g(a.dcls, cell * a.ld_dcls + c, 0.f, a.dcls_bf16);
    if (a.dreg)
      for (int i = NB; i < a.ld_dreg; ++i) store_g(a.dreg, cell * a.ld_dreg + i, 0.f, a.dreg_bf16);
  }
  block_partials<NTH, 3>(a.partial, a.tiles, s);
}

// LDS-staged form, four lanes per cell (the shape of fcos_paper.hip's fcos_paper_loss_lds4_kernel): the
// block's CPB cells' target and class rows are loaded cooperatively (coalesced) into rows of odd pitch
// RP = targets | class logits | box logits; a positive cell's lane j copies side j's R+1 logits into the
// box part, forms its softmax statistics there and, after the four expectations have crossed the quad
// for the GIoU, overwrites them with the side's gradients.  The C QFL terms of a cell are spread over
// its 4 lanes (class c on lane c % 4), each term parked in the cell's target slot 5 + c; the owner lane
// sums them in class order (the fp32 sequence of the row form).  Target slot 4, which the rule does not
// read, carries the cell's positive flag to the write-out: gradient rows leave as 16-byte stores of whole
// rows, padding columns and the box rows of non-positive cells zero (their box logits are never read).
// The block sums take the owners' values in the row form's lane order, so the results are bit-identical
// to fcos_gfl_loss_rows_kernel<CPB>.
template <int CPB>
__global__ void __launch_bounds__(4 * CPB) fcos_gfl_loss_lds4_kernel(GflLossArgs a, int RP) {
  constexpr int NTH = 4 * CPB;
  extern __shared__ float rows[];
  float* csum = rows + CPB * RP;                      // per-cell (s_qfl, s_box, s_dfl)
  const int b = blockIdx.y, p0 = blockIdx.x * CPB;
  const int ncell = min(CPB, a.P - p0);
  const int C = a.C, R = a.R, R1 = R + 1, NB = 4 * R1;
  const int T5 = 5 + C;
  const int OC = T5, OB = T5 + C;
  const size_t cell0 = (size_t)b * a.P + p0;
  float gn, gbox, gdfl;
  image_factors(a, b, gn, gbox, gdfl);
  {
    const float* tg = a.tgt + cell0 * T5;
    for (int i = threadIdx.x; i < ncell * T5; i += NTH) {
      const int r = i / T5;
      rows[r * RP + (i - r * T5)] = tg[i];
    }
    const float* cg = a.cls + cell0 * a.ld_cls;
    for (int i = threadIdx.x; i < ncell * C; i += NTH) {
      const int r = i / C, c = i - r * C;
      rows[r * RP + OC + c] = cg[(size_t)r * a.ld_cls + c];
    }
  }
  __syncthreads();
  const int cell = threadIdx.x >> 2, sub = threadIdx.x & 3;
  const bool live = cell < ncell;
  float* row = rows + cell * RP;
  float tmax = 0.f, xmax = -INFINITY;
  if (live)
    for (int c = sub; c < C; c += 4) {
      tmax = fmaxf(tmax, row[5 + c]);
      xmax = fmaxf(xmax, row[OC + c]);
    }
  tmax = fmaxf(tmax, __shfl_xor(tmax, 1, 64));
  tmax = fmaxf(tmax, __shfl_xor(tmax, 2, 64));
  xmax = fmaxf(xmax, __shfl_xor(xmax, 1, 64));
  xmax = fmaxf(xmax, __shfl_xor(xmax, 2, 64));
  const bool pos = live && tmax >= 1.0f;
  // this lane's side: logits into LDS, softmax statistics
  float* zl = row + OB + sub * R1;
  auto zf = [&](int i) { return zl[i]; };
  Side sd;
  sd.m = 0.f; sd.s = 1.0f; sd.d = 0.f; sd.lse = 0.f;
  if (pos) {
    const float* zg = a.reg + (cell0 + cell) * a.ld_reg + sub * R1;
    for (int i = 0; i <= R; ++i) zl[i] = zg[i];
    sd = side_forward(zf, R);
  }
  // the four expectations cross the quad (every lane of the wave takes part in the exchange)
  float d[4], tt[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    d[j] = __shfl(sd.d, j, 4);
    tt[j] = pos ? row[j] : 0.f;
  }
  float q = 0.f, w = 0.f, giou = 0.f, dval = 0.f;
  if (pos) {
    const Giou G = giou_terms(tt, d);
    q = G.iou;
    giou = G.giou;
    w = sigmoid_f(xmax);
    const float dGj = sub == 0 ? G.dG[0] : (sub == 1 ? G.dG[1] : (sub == 2 ? G.dG[2] : G.dG[3]));
    const float tj = sub == 0 ? tt[0] : (sub == 1 ? tt[1] : (sub == 2 ? tt[2] : tt[3]));
    const Dfl f = dfl_side(zf, R, tj, sd.lse);
    dval = f.val;
    if (a.dreg) side_backward(zf, [&](int i, float g) { zl[i] = g; }, R, sd, f, -w * dGj * gbox, w * 0.25f * gdfl);
  }
  float dv[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) dv[j] = __shfl(dval, j, 4);
  if (live)
    for (int c = sub; c < C; c += 4) {
      const float y = (pos && row[5 + c] >= 1.0f) ? q : 0.f;
      float g;
      row[5 + c] = qfl_term(y, row[OC + c], a.beta, &g);   // the term, in its target slot
      row[OC + c] = g * gn;
    }
  __syncthreads();
  if (sub == 0) {
    float s_qfl = 0.f, s_box = 0.f, s_dfl = 0.f;
    if (live) {
      for (int c = 0; c < C; ++c) s_qfl += row[5 + c];
      if (pos) {
        s_box = w * (1.0f - giou);
        s_dfl = w * (0.25f * (((dv[0] + dv[1]) + dv[2]) + dv[3]));
      }
      row[4] = pos ? 1.0f : 0.f;
    }
    csum[cell * 3] = s_qfl;
    csum[cell * 3 + 1] = s_box;
    csum[cell * 3 + 2] = s_dfl;
  }
  __syncthreads();
  // gradient rows: whole rows in 16-byte pieces (8 bf16 or 4 fp32 columns), padding columns zero;
  // gated: the row's columns are valid only where target slot 4 says so (the box rows of positives)
  auto grad_rows = [&](void* dst, int ld, int is_bf16, int base, int ncol, bool gated) {
    const int wv = is_bf16 ? 8 : 4, npc = ld / wv;
    for (int i = threadIdx.x; i < ncell * npc; i += NTH) {
      const int r = i / npc, c0 = (i - r * npc) * wv;
      const bool on = !gated || rows[r * RP + 4] != 0.f;
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int c = c0 + u;
        v[u] = (on && u < wv && c < ncol) ? rows[r * RP + base + c] : 0.f;
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
  if (a.dcls) grad_rows(a.dcls, a.ld_dcls, a.dcls_bf16, OC, C, false);
  if (a.dreg) grad_rows(a.dreg, a.ld_dreg, a.dreg_bf16, OB, NB, true);
  // lanes 0 .. CPB-1 carry cells 0 .. CPB-1 as the row form's threads do; the other waves add zeros
  const bool own = (int)threadIdx.x < CPB;
  const float s[3] = {own ? csum[threadIdx.x * 3] : 0.f, own ? csum[threadIdx.x * 3 + 1] : 0.f,
                      own ? csum[threadIdx.x * 3 + 2] : 0.f};
  block_partials<NTH, 3>(a.partial, a.tiles, s);
}

// fixed-order second pass; the per-image divisors and the term weights are applied here, in float64
__global__ void fcos_gfl_loss_finalize(const double* partial, const float* norm, float* losses, int tiles,
                                       float w_box, float w_dfl) {
  const int b = blockIdx.x;
  const int k = threadIdx.x;   // 0..2
  if (k < 3) {
    double s = 0.0;
    for (int i = 0; i < tiles; ++i) s += partial[((size_t)b * tiles + i) * 3 + k];
    float N = 1.0f, Wsum = 1.0f;
    if (norm) {
      N = fmaxf(norm[2 * b], 1.0f);
      Wsum = fmaxf(norm[2 * b + 1], 1.0e-6f);
    }
    const double wk = k == 0 ? 1.0 : (k == 1 ? (double)w_box : (double)w_dfl);
    losses[b * 3 + k] = (float)(wk * s / (double)(k == 0 ? N : Wsum));
  }
}

template <int CPB>
void launch_lds4(const GflLossArgs& a, int B, int RP, hipStream_t s) {
  const size_t lds = ((size_t)CPB * RP + CPB * 3) * sizeof(float);
  hipLaunchKernelGGL((fcos_gfl_loss_lds4_kernel<CPB>), dim3(a.tiles, B), dim3(4 * CPB), lds, s, a, RP);
}

template <int NTH>
void launch_rows(const GflLossArgs& a, int B, hipStream_t s) {
  hipLaunchKernelGGL((fcos_gfl_loss_rows_kernel<NTH>), dim3(a.tiles, B), dim3(NTH), 0, s, a);
}

// one thread per (row, side): the expectation of the side's distribution; the thread also zeroes the
// row's columns 4 + side, 8 + side, ...
__global__ void __launch_bounds__(kThreads) fcos_gfl_decode_kernel(const float* reg, int ld_reg, int rows, int R,
                                                                   float* out, int ld_out) {
  const size_t idx = (size_t)blockIdx.x * kThreads + threadIdx.x;
  const size_t r = idx >> 2;
  const int j = (int)(idx & 3);
  if (r >= (size_t)rows) return;
  const float* z = reg + r * ld_reg + j * (R + 1);
  const Side sd = side_forward([&](int i) { return z[i]; }, R);
  float* o = out + r * ld_out;
  o[j] = sd.d;
  for (int c = 4 + j; c < ld_out; c += 4) o[c] = 0.f;
}

}  // namespace

extern "C" size_t cvl_fcos_gfl_norm_workspace_size(int B, int P) {
  if (B <= 0 || P <= 0) return 0;
  return (size_t)B * ((size_t)(P + kThreads - 1) / kThreads) * 2 * sizeof(double);
}

extern "C" int cvl_fcos_gfl_norm(const float* cls_pred, int ld_cls, const float* targets, int B, int P,
                                 int num_classes, float* norm, void* workspace, size_t workspace_bytes,
                                 cvl_stream_t stream) {
  CVL_CHECK_ARG(cls_pred && targets && norm && workspace && B > 0 && P > 0 && num_classes > 0);
  CVL_CHECK_ARG(ld_cls >= num_classes);
  CVL_CHECK_ARG(workspace_bytes >= cvl_fcos_gfl_norm_workspace_size(B, P));
  const int tiles = (P + kThreads - 1) / kThreads;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(fcos_gfl_norm_kernel, dim3(tiles, B), dim3(kThreads), 0, s, cls_pred, ld_cls, targets,
                     (double*)workspace, P, num_classes, tiles);
  int st = cvl_launch_status();
  if (st) return st;
  hipLaunchKernelGGL(fcos_gfl_norm_finalize, dim3(B), dim3(64), 0, s, (const double*)workspace, norm, tiles);
  return cvl_launch_status();
}

extern "C" size_t cvl_fcos_gfl_loss_workspace_size(int B, int P) {
  if (B <= 0 || P <= 0) return 0;
  return (size_t)B * ((size_t)(P + 63) / 64) * 3 * sizeof(double);   // per-tile partials of the smallest tiles
}

extern "C" int cvl_fcos_gfl_loss(const float* reg_pred, int ld_reg, const float* cls_pred, int ld_cls,
                                 const float* targets, const float* norm, int B, int P, int num_classes,
                                 int reg_max, float grad_scale, float beta, float w_box, float w_dfl,
                                 float* losses, void* d_reg, int ld_dreg, int dreg_dtype, void* d_cls, int ld_dcls,
                                 int dcls_dtype, void* workspace, size_t workspace_bytes, cvl_stream_t stream) {
  CVL_CHECK_ARG(reg_pred && cls_pred && targets && losses && workspace);
  CVL_CHECK_ARG(B > 0 && P > 0 && num_classes > 0);
  CVL_CHECK_ARG(reg_max >= 1 && reg_max <= kMaxRegMax);
  CVL_CHECK_ARG(workspace_bytes >= cvl_fcos_gfl_loss_workspace_size(B, P));
  CVL_CHECK_ARG(beta >= 0.f);
  const int NB = 4 * (reg_max + 1);
  CVL_CHECK_ARG(ld_reg >= NB && ld_cls >= num_classes);
  CVL_CHECK_ARG(!d_reg || ld_dreg >= NB);
  CVL_CHECK_ARG(!d_cls || ld_dcls >= num_classes);
  CVL_CHECK_ARG((dreg_dtype == 0 || dreg_dtype == 1) && (dcls_dtype == 0 || dcls_dtype == 1));
  GflLossArgs a;
  a.reg = reg_pred; a.cls = cls_pred; a.tgt = targets; a.norm = norm;
  a.dreg = d_reg; a.dcls = d_cls; a.partial = (double*)workspace;
  a.ld_reg = ld_reg; a.ld_cls = ld_cls; a.ld_dreg = ld_dreg; a.ld_dcls = ld_dcls;
  a.dreg_bf16 = dreg_dtype; a.dcls_bf16 = dcls_dtype;
  a.P = P; a.C = num_classes; a.R = reg_max;
  a.grad_scale = grad_scale; a.beta = beta; a.w_box = w_box; a.w_dfl = w_dfl;
  // the tile: the most cells (256 / 128 / 64) whose rows (pitch RP floats, odd) and per-cell sums fit the
  // LDS next to the block sums' static part; 0 when even 64 cells do not (C too large to stage)
  const int RP = (5 + num_classes + num_classes + NB) | 1;
  int cpb = 0;
  for (int n = 256; n >= 64 && !cpb; n /= 2)
    if (((size_t)n * RP + n * 3) * sizeof(float) <= 63 * 1024) cpb = n;
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
    if (cpb == 256) launch_lds4<256>(a, B, RP, s);
    else if (cpb == 128) launch_lds4<128>(a, B, RP, s);
    else launch_lds4<64>(a, B, RP, s);
  } else {
    if (tile == 256) launch_rows<256>(a, B, s);
    else if (tile == 128) launch_rows<128>(a, B, s);
    else launch_rows<64>(a, B, s);
  }
  int st = cvl_launch_status();
  if (st) return st;
  hipLaunchKernelGGL(fcos_gfl_loss_finalize, dim3(B), dim3(64), 0, s, (const double*)workspace, norm, losses,
                     a.tiles, w_box, w_dfl);
  return cvl_launch_status();
}

extern "C" int cvl_fcos_gfl_decode(const float* reg_pred, int ld_reg, int rows, int reg_max, float* out, int ld_out,
                                   cvl_stream_t stream) {
  CVL_CHECK_ARG(reg_pred && out && rows > 0);
  CVL_CHECK_ARG(reg_max >= 1 && reg_max <= kMaxRegMax);
  CVL_CHECK_ARG(ld_reg >= 4 * (reg_max + 1) && ld_out >= 8);
  const size_t nth = (size_t)rows * 4;
  hipLaunchKernelGGL(fcos_gfl_decode_kernel, dim3((unsigned)((nth + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                     (hipStream_t)stream, reg_pred, ld_reg, rows, reg_max, out, ld_out);
  return cvl_launch_status();
}
