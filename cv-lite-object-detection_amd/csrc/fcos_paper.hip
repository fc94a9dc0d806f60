// The FCOS recipe of the FCOS papers (Tian et al., ICCV 2019 / TPAMI 2020) on gfx950 -- an extension
// beyond the reference, whose own recipe stays in fcos_assign.hip / fcos_loss.hip:
//   cvl_fcos_paper_assign   per-level regress range on max(l,t,r,b), centre sampling, smallest-area
//                           disambiguation, sqrt centerness, one-hot class
//   cvl_fcos_target_norm    (number of positives, sum of their centerness targets) per image
//   cvl_fcos_paper_loss     focal / N, centerness-weighted GIoU / sum(centerness), BCE centerness on
//                           positives / N; forward + backward in one pass
// The exact rules are stated in include/cvlite.h.  This file is compiled with -ffp-contract=off: the
// assignment is a fixed fp32 operation sequence that tests/fcos_paper_ref.py restates bit for bit.
//
// Work: assign is HBM-write bound ((5+C)*4 bytes per cell), the loss HBM read+write bound (targets and
// predictions read once, gradients written once), the norm one more read of the targets.
#include "cvl_common.h"
#include "fcos_focal.h"

#include <math.h>

namespace {

constexpr int kMaxBoxes = 256;   // per image
constexpr int kThreads = 256;
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------------------------
// assignment
// ---------------------------------------------------------------------------------------------
struct PaperAssignArgs {
  const float* boxes;
  const int32_t* nbox;
  const float* img_dim;
  float* targets;
  int32_t* num_targets;
  int n_max, C, P;
  float radius;
  int strides[5];
  float lo[5], hi[5];
  int Ws[5], off[6];
};

struct PaperBox {
  float y0, y1, x0, x1, yc, xc, area;
  int cls;                       // < 0: the box is skipped (label outside [0, C))
};

__device__ __forceinline__ float min4(float a, float b, float c, float d) { return fminf(fminf(a, b), fminf(c, d)); }
__device__ __forceinline__ float max4(float a, float b, float c, float d) { return fmaxf(fmaxf(a, b), fmaxf(c, d)); }

// One thread per cell of a blockDim.x-cell tile (level-major cell index p); the tile's [ncell, 5+C]
// slab is staged in LDS and written out coalesced.
__global__ void __launch_bounds__(kThreads) fcos_paper_assign_kernel(PaperAssignArgs a) {
  const int b = blockIdx.y;
  const int tid = threadIdx.x, nth = blockDim.x;
  const int C = a.C;
  const int row = 5 + C;

  __shared__ PaperBox box[kMaxBoxes];
  __shared__ int lcount[5];
  extern __shared__ __attribute__((aligned(16))) float stage[];

  int n = a.nbox[b];
  n = n < 0 ? 0 : (n > a.n_max ? a.n_max : n);
  n = n > kMaxBoxes ? kMaxBoxes : n;
  const float H = a.img_dim[2 * b + 0];
  const float W = a.img_dim[2 * b + 1];

  if (tid < 5) lcount[tid] = 0;
  // ---- phase 1: box corners in pixels, once per workgroup ------------------------------------
  for (int i = tid; i < n; i += nth) {
    const float* r = a.boxes + ((size_t)b * a.n_max + i) * 5;
    const float yc = r[0] * H, xc = r[1] * W, hp = r[2] * H, wp = r[3] * W;
    PaperBox bx;
    bx.yc = yc; bx.xc = xc;
    bx.y0 = yc - hp * 0.5f; bx.y1 = yc + hp * 0.5f;
    bx.x0 = xc - wp * 0.5f; bx.x1 = xc + wp * 0.5f;
    bx.area = hp * wp;
    const int cls = (int)r[4];
    bx.cls = (cls >= 0 && cls < C) ? cls : -1;
    box[i] = bx;
  }
  __syncthreads();

  // ---- phase 2: the winner of this thread's cell ----------------------------------------------
  const int p0 = blockIdx.x * nth;
  const int p = p0 + tid;
  const int ncell = min(nth, a.P - p0);
  int lvl = 0;
  bool pos = false;
  if (p < a.P) {
    while (lvl < 4 && p >= a.off[lvl + 1]) ++lvl;
    const int q = p - a.off[lvl];
    const int Ws = a.Ws[lvl];
    const int cy = q / Ws, cx = q - (q / Ws) * Ws;
    const float sf = (float)a.strides[lvl];
    const float gy = ((float)cy + 0.5f) * sf, gx = ((float)cx + 0.5f) * sf;
    const float lo = a.lo[lvl], hi = a.hi[lvl];
    const float rs = a.radius * sf;
    int best = -1;
    float best_area = 0.f;
    for (int i = 0; i < n; ++i) {
      const PaperBox& bx = box[i];
      if (bx.cls < 0) continue;
      const float t = gy - bx.y0, bt = bx.y1 - gy, l = gx - bx.x0, r = bx.x1 - gx;
      const float m = max4(t, bt, l, r);
      if (!(lo <= m && m <= hi)) continue;
      float in;
      if (a.radius <= 0.f) {
        in = min4(t, bt, l, r);
      } else {
        const float sy0 = fmaxf(bx.y0, bx.yc - rs), sy1 = fminf(bx.y1, bx.yc + rs);
        const float sx0 = fmaxf(bx.x0, bx.xc - rs), sx1 = fminf(bx.x1, bx.xc + rs);
        in = min4(gy - sy0, sy1 - gy, gx - sx0, sx1 - gx);
      }
      if (!(in > 0.f)) continue;
      if (best < 0 || bx.area < best_area) {     // smallest area; ties keep the lowest index
        best = i;
        best_area = bx.area;
      }
    }
    float v0 = 0.f, v1 = 0.f, v2 = 0.f, v3 = 0.f, v4 = 0.f;
    int cls = -1;
    if (best >= 0) {
      const PaperBox& bx = box[best];
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
// target norm
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) fcos_target_norm_kernel(const float* tgt, double* partial, int P, int C,
                                                                    int tiles) {
  const int p = blockIdx.x * kThreads + threadIdx.x;
  float s[2] = {0.f, 0.f};
  if (p < P) {
    const float* t = tgt + ((size_t)blockIdx.y * P + p) * (5 + C);
    float tmax = 0.f;
    for (int c = 0; c < C; ++c) tmax = fmaxf(tmax, t[5 + c]);
    if (tmax >= 1.0f) { s[0] = 1.0f; s[1] = t[4]; }
  }
  block_partials<kThreads, 2>(partial, tiles, s);
}

__global__ void fcos_target_norm_finalize(const double* partial, float* norm, int tiles) {
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
struct PaperLossArgs {
  const float* reg;
  const float* cls;
  const float* tgt;
  const float* norm;   // [B, 2] or null
  float* losses;
  void* dreg;
  void* dcls;
  double* partial;     // [B, tiles, 3]
  int ld_reg, ld_cls, ld_dreg, ld_dcls, dreg_bf16, dcls_bf16;
  int P, C, tiles;
  float grad_scale, alpha, gamma;
};

__device__ __forceinline__ void store_g(void* base, size_t idx, float v, int is_bf16) {
  if (is_bf16) reinterpret_cast<cvl_bf16*>(base)[idx] = f32_to_bf16(v);
  else reinterpret_cast<float*>(base)[idx] = v;
}

// the image's divisors: N = max(n_pos, 1), Wsum = max(sum centerness, 1e-6); 1 without a norm
__device__ __forceinline__ void image_norm(const PaperLossArgs& a, int b, float& N, float& Wsum) {
  N = 1.0f; Wsum = 1.0f;
  if (a.norm) {
    N = fmaxf(a.norm[2 * b], 1.0f);
    Wsum = fmaxf(a.norm[2 * b + 1], 1.0e-6f);
  }
}

// Centerness and box terms of one cell: t(i) targets[i], xr(j) box / centerness prediction j < 5;
// putr(j, g) receives the scaled gradients.  gn = grad_scale / N, gw = grad_scale / Wsum.  Only
// positive cells contribute; the others get zero gradients.
template <class TF, class XRF, class PR>
__device__ __forceinline__ void cell_rest(TF t, XRF xr, PR putr, bool pos, float gn, float gw, float& s_reg,
                                          float& s_cen) {
  float g[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  if (pos) {
    const float t4 = t(4);
    {
      // BCE with logits on the centerness target: max(x,0) - x t4 + log(1 + e^-|x|); d/dx = sigmoid(x) - t4
      const float x = xr(4);
      const float e = expf(-fabsf(x));
      const float sg = x >= 0.f ? 1.0f / (1.0f + e) : e / (1.0f + e);
      s_cen += fmaxf(x, 0.f) - x * t4 + log1pf(e);
      g[4] = (sg - t4) * gn;
    }
    // GIoU of ltrb boxes about the same grid point, on d_j = max(p_j, 0): min / max of the distances
    // give the intersection and the enclosing box directly
    const float tt[4] = {t(0), t(1), t(2), t(3)};
    const float pp[4] = {xr(0), xr(1), xr(2), xr(3)};
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
    s_reg += t4 * (1.0f - giou);
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
      g[j] = pp[j] > 0.f ? -t4 * dG * gw : 0.f;
    }
  }
#pragma unroll
  for (int j = 0; j < 5; ++j) putr(j, g[j]);
}

// Row-pointer form (any layout): a thread walks its cell's rows in global memory.
__global__ void __launch_bounds__(kThreads) fcos_paper_loss_kernel(PaperLossArgs a) {
  const int b = blockIdx.y;
  const int p = blockIdx.x * kThreads + threadIdx.x;
  float N, Wsum;
  image_norm(a, b, N, Wsum);
  const float gn = a.grad_scale / N, gw = a.grad_scale / Wsum;
  float s[3] = {0.f, 0.f, 0.f};
  if (p < a.P) {
    const size_t cell = (size_t)b * a.P + p;
    const float* t = a.tgt + cell * (5 + a.C);
    const float* xr = a.reg + cell * a.ld_reg;
    const float* xc = a.cls + cell * a.ld_cls;
    float tmax = 0.f;
    for (int c = 0; c < a.C; ++c) {
      const float y = t[5 + c];
      tmax = fmaxf(tmax, y);
      float g;
      s[0] += focal_term(y, xc[c], a.alpha, a.gamma, &g);
      if (a.dcls) store_g(a.dcls, cell * a.ld_dcls + c, g * gn, a.dcls_bf16);
    }
    cell_rest([&](int i) { return t[i]; }, [&](int j) { return xr[j]; },
              [&](int j, float v) {
                if (a.dreg) store_g(a.dreg, cell * a.ld_dreg + j, v, a.dreg_bf16);
              },
              tmax >= 1.0f, gn, gw, s[1], s[2]);
    if (a.dcls)
      for (int c = a.C; c < a.ld_dcls; ++c) store_g(a.dcls, cell * a.ld_dcls + c, 0.f, a.dcls_bf16);
    if (a.dreg)
      for (int j = 5; j < a.ld_dreg; ++j) store_g(a.dreg, cell * a.ld_dreg + j, 0.f, a.dreg_bf16);
  }
  block_partials<kThreads, 3>(a.partial, a.tiles, s);
}

// LDS-staged form, four lanes per cell (the shape of fcos_loss.hip's fcos_loss_lds4_kernel): the
// block's CPB cells' target, class and box rows are loaded cooperatively (coalesced) into rows of odd
// pitch R = targets | class logits | box; the C focal terms of a cell are spread over its 4 lanes
// (class c on lane c % 4), each term parked in the cell's target slot 5 + c; the owner lane sums them in
// class order (the fp32 sequence of the row form) and runs the rest of the cell, writing the scaled
// gradients back in place; the gradient rows leave as 16-byte stores of whole rows (padding columns
// zero).  At CPB = 256 the block sums take the owners' values in the row form's lane order, so the
// results are bit-identical to fcos_paper_loss_kernel.
template <int CPB>
__global__ void __launch_bounds__(4 * CPB) fcos_paper_loss_lds4_kernel(PaperLossArgs a, int R) {
  constexpr int NTH = 4 * CPB;
  extern __shared__ float rows[];
  float* csum = rows + CPB * R;                       // per-cell (s_cls, s_reg, s_cen)
  const int b = blockIdx.y, p0 = blockIdx.x * CPB;
  const int ncell = min(CPB, a.P - p0);
  const int T5 = 5 + a.C;
  const int OC = T5, OR = T5 + a.C;
  const size_t cell0 = (size_t)b * a.P + p0;
  float N, Wsum;
  image_norm(a, b, N, Wsum);
  const float gn = a.grad_scale / N, gw = a.grad_scale / Wsum;
  {
    const float* tg = a.tgt + cell0 * T5;
    for (int i = threadIdx.x; i < ncell * T5; i += NTH) {
      const int r = i / T5;
      rows[r * R + (i - r * T5)] = tg[i];
    }
    const float* cg = a.cls + cell0 * a.ld_cls;
    for (int i = threadIdx.x; i < ncell * a.C; i += NTH) {
      const int r = i / a.C, c = i - r * a.C;
      rows[r * R + OC + c] = cg[(size_t)r * a.ld_cls + c];
    }
    const float* rg = a.reg + cell0 * a.ld_reg;
    for (int i = threadIdx.x; i < ncell * 5; i += NTH) {
      const int r = i / 5, j = i - r * 5;
      rows[r * R + OR + j] = rg[(size_t)r * a.ld_reg + j];
    }
  }
  __syncthreads();
  const int cell = threadIdx.x >> 2, sub = threadIdx.x & 3;
  float tmax = 0.f;
  if (cell < ncell) {
    float* row = rows + cell * R;
    for (int c = sub; c < a.C; c += 4) {
      const float y = row[5 + c];
      tmax = fmaxf(tmax, y);
      float g;
      row[5 + c] = focal_term(y, row[OC + c], a.alpha, a.gamma, &g);   // the term, in its target slot
      row[OC + c] = g * gn;
    }
  }
  tmax = fmaxf(tmax, __shfl_xor(tmax, 1, 64));
  tmax = fmaxf(tmax, __shfl_xor(tmax, 2, 64));
  __syncthreads();
  if (sub == 0) {
    float s_cls = 0.f, s_reg = 0.f, s_cen = 0.f;
    if (cell < ncell) {
      float* row = rows + cell * R;
      for (int c = 0; c < a.C; ++c) s_cls += row[5 + c];
      cell_rest([&](int i) { return row[i]; }, [&](int j) { return row[OR + j]; },
                [&](int j, float v) { row[OR + j] = v; }, tmax >= 1.0f, gn, gw, s_reg, s_cen);
    }
    csum[cell * 3] = s_cls;
    csum[cell * 3 + 1] = s_reg;
    csum[cell * 3 + 2] = s_cen;
  }
  __syncthreads();
  // gradient rows: whole rows in 16-byte pieces (8 bf16 or 4 fp32 columns), padding columns zero
  auto grad_rows = [&](void* dst, int ld, int is_bf16, int base, int ncol) {
    const int w = is_bf16 ? 8 : 4, npc = ld / w;
    for (int i = threadIdx.x; i < ncell * npc; i += NTH) {
      const int r = i / npc, c0 = (i - r * npc) * w;
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int c = c0 + u;
        v[u] = (u < w && c < ncol) ? rows[r * R + base + c] : 0.f;
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
  if (a.dcls) grad_rows(a.dcls, a.ld_dcls, a.dcls_bf16, OC, a.C);
  if (a.dreg) grad_rows(a.dreg, a.ld_dreg, a.dreg_bf16, OR, 5);
  // lanes 0 .. CPB-1 carry cells 0 .. CPB-1 as the row form's threads do; the other waves add zeros
  const bool own = (int)threadIdx.x < CPB;
  const float s[3] = {own ? csum[threadIdx.x * 3] : 0.f, own ? csum[threadIdx.x * 3 + 1] : 0.f,
                      own ? csum[threadIdx.x * 3 + 2] : 0.f};
  block_partials<NTH, 3>(a.partial, a.tiles, s);
}

// fixed-order second pass; the per-image divisors are applied here, in float64
__global__ void fcos_paper_loss_finalize(const double* partial, const float* norm, float* losses, int tiles) {
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
    losses[b * 3 + k] = (float)(s / (double)(k == 1 ? Wsum : N));
  }
}

template <int CPB>
void launch_lds4(const PaperLossArgs& a, int B, int R, hipStream_t s) {
  const size_t lds = ((size_t)CPB * R + CPB * 3) * sizeof(float);
  hipLaunchKernelGGL((fcos_paper_loss_lds4_kernel<CPB>), dim3(a.tiles, B), dim3(4 * CPB), lds, s, a, R);
}

}  // namespace

extern "C" int cvl_fcos_paper_assign(const float* boxes, const int32_t* nbox, const float* img_dim, int B,
                                     int n_max, int pad_h, int pad_w, int num_classes, const int32_t* strides,
                                     const float* size_bounds, float center_radius, float* targets,
                                     int32_t* num_targets, cvl_stream_t stream) {
  CVL_CHECK_ARG(boxes && nbox && img_dim && targets && num_targets && strides && size_bounds);
  CVL_CHECK_ARG(B > 0 && n_max > 0 && n_max <= kMaxBoxes && pad_h > 0 && pad_w > 0);
  CVL_CHECK_ARG(num_classes > 0 && num_classes <= 256);
  PaperAssignArgs a;
  a.boxes = boxes; a.nbox = nbox; a.img_dim = img_dim; a.targets = targets;
  a.num_targets = num_targets; a.n_max = n_max; a.C = num_classes; a.radius = center_radius;
  a.off[0] = 0;
  for (int l = 0; l < 5; ++l) {
    CVL_CHECK_ARG(strides[l] > 0);
    a.strides[l] = strides[l];
    const int Hs = pad_h / strides[l];
    a.Ws[l] = pad_w / strides[l];
    CVL_CHECK_ARG(Hs > 0 && a.Ws[l] > 0);
    a.off[l + 1] = a.off[l] + Hs * a.Ws[l];
    a.lo[l] = l == 0 ? -1.0f : size_bounds[l - 1];
    a.hi[l] = l == 4 ? INFINITY : size_bounds[l];
  }
  a.P = a.off[5];
  // the largest tile whose staged [cells, 5+C] slab leaves the 64 KB of LDS room for the box table
  int nth = 0;
  for (int n = kThreads; n >= 64 && !nth; n /= 2)
    if ((size_t)n * (5 + num_classes) * sizeof(float) <= 56 * 1024) nth = n;
  CVL_CHECK_ARG(nth > 0);                              // C <= 219
  const size_t lds = (size_t)nth * (5 + num_classes) * sizeof(float);
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(num_targets, 0, sizeof(int32_t) * 5 * B, s) != hipSuccess) return cvl_launch_status();
  hipLaunchKernelGGL(fcos_paper_assign_kernel, dim3((a.P + nth - 1) / nth, B), dim3(nth), lds, s, a);
  return cvl_launch_status();
}

extern "C" size_t cvl_fcos_target_norm_workspace_size(int B, int P) {
  if (B <= 0 || P <= 0) return 0;
  return (size_t)B * ((size_t)(P + kThreads - 1) / kThreads) * 2 * sizeof(double);
}

extern "C" int cvl_fcos_target_norm(const float* targets, int B, int P, int num_classes, float* norm,
                                    void* workspace, size_t workspace_bytes, cvl_stream_t stream) {
  CVL_CHECK_ARG(targets && norm && workspace && B > 0 && P > 0 && num_classes > 0);
  CVL_CHECK_ARG(workspace_bytes >= cvl_fcos_target_norm_workspace_size(B, P));
  const int tiles = (P + kThreads - 1) / kThreads;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(fcos_target_norm_kernel, dim3(tiles, B), dim3(kThreads), 0, s, targets, (double*)workspace, P,
                     num_classes, tiles);
  int st = cvl_launch_status();
  if (st) return st;
  hipLaunchKernelGGL(fcos_target_norm_finalize, dim3(B), dim3(64), 0, s, (const double*)workspace, norm, tiles);
  return cvl_launch_status();
}

extern "C" int cvl_fcos_paper_loss(const float* reg_pred, int ld_reg, const float* cls_pred, int ld_cls,
                                   const float* targets, const float* norm, int B, int P, int num_classes,
                                   float grad_scale, float alpha, float gamma, float* losses, void* d_reg,
                                   int ld_dreg, int dreg_dtype, void* d_cls, int ld_dcls, int dcls_dtype,
                                   void* workspace, size_t workspace_bytes, cvl_stream_t stream) {
  CVL_CHECK_ARG(reg_pred && cls_pred && targets && losses && workspace);
  CVL_CHECK_ARG(B > 0 && P > 0 && num_classes > 0);
  CVL_CHECK_ARG(workspace_bytes >= cvl_fcos_loss_workspace_size(B, P));
  CVL_CHECK_ARG(gamma >= 0.f);
  CVL_CHECK_ARG(ld_reg >= 5 && ld_cls >= num_classes);
  CVL_CHECK_ARG(!d_reg || ld_dreg >= 5);
  CVL_CHECK_ARG(!d_cls || ld_dcls >= num_classes);
  CVL_CHECK_ARG((dreg_dtype == 0 || dreg_dtype == 1) && (dcls_dtype == 0 || dcls_dtype == 1));
  PaperLossArgs a;
  a.reg = reg_pred; a.cls = cls_pred; a.tgt = targets; a.norm = norm; a.losses = losses;
  a.dreg = d_reg; a.dcls = d_cls; a.partial = (double*)workspace;
  a.ld_reg = ld_reg; a.ld_cls = ld_cls; a.ld_dreg = ld_dreg; a.ld_dcls = ld_dcls;
  a.dreg_bf16 = dreg_dtype; a.dcls_bf16 = dcls_dtype;
  a.P = P; a.C = num_classes; a.grad_scale = grad_scale; a.alpha = alpha; a.gamma = gamma;
  // the LDS-staged form when its rows fit (pitch R floats, odd) and the gradient rows take 16-B stores
  const int R = (5 + num_classes + num_classes + 5) | 1;
  auto vec_ok = [](const void* p, int ld, int bf16) {
    return !p || ((reinterpret_cast<uintptr_t>(p) & 15) == 0 && ld % (bf16 ? 8 : 4) == 0);
  };
  int cpb = 0;
  if (vec_ok(d_reg, ld_dreg, dreg_dtype) && vec_ok(d_cls, ld_dcls, dcls_dtype) && !cvl_dispatch_flag("loss_rows"))
    for (int n = 256; n >= 64 && !cpb; n /= 2)
      if (((size_t)n * R + n * 3) * sizeof(float) <= 63 * 1024) cpb = n;   // + the block sums' static LDS
  a.tiles = (P + (cpb ? cpb : kThreads) - 1) / (cpb ? cpb : kThreads);
  hipStream_t s = (hipStream_t)stream;
  if (cpb == 256) launch_lds4<256>(a, B, R, s);
  else if (cpb == 128) launch_lds4<128>(a, B, R, s);
  else if (cpb == 64) launch_lds4<64>(a, B, R, s);
  else hipLaunchKernelGGL(fcos_paper_loss_kernel, dim3(a.tiles, B), dim3(kThreads), 0, s, a);
  int st = cvl_launch_status();
  if (st) return st;
  hipLaunchKernelGGL(fcos_paper_loss_finalize, dim3(B), dim3(64), 0, s, (const double*)workspace, norm, losses,
                     a.tiles);
  return cvl_launch_status();
}
