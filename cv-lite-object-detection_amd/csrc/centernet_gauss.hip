// CenterNet as "Objects as Points" (Zhou et al., 2019) trains it, on gfx950 -- an extension beyond the
// reference, whose hourglass recipe (one-hot centres, full-weight negatives, plain sums) stays in
// det_targets.hip:
//   cvl_centernet_gauss_assign   Gaussian heat about every centre (radius: mmdet's gaussian_radius),
//                                the reference's box channels at the centre cells
//   cvl_centernet_gauss_norm     number of (cell, class) entries equal to 1.0f per image
//   cvl_centernet_gauss_loss     penalty-reduced focal loss + L1 on the centres, divided by that
//                                number; forward + backward in one pass
// The exact rules are stated in include/cvlite.h.  This file is compiled with -ffp-contract=off.
//
// Work: all three are HBM bound.  The assign writes the map once, one thread per output element; the
// norm reads it once; the loss reads targets and predictions once and writes the bf16 gradient once,
// every global access with consecutive lanes on consecutive addresses of a row.
#include "cvl_common.h"

#include <math.h>

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBox = 256;
constexpr int kMaxClasses = 256;
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------------------------
// assign
// ---------------------------------------------------------------------------------------------
struct GaussAssignArgs {
  const float* boxes;
  const int32_t* nbox;
  const float* img_dim;
  float* out;
  int n_max, C, hm, wm, stride;
  float pad_h, pad_w;
  double m;
};

// mmdet's gaussian_radius (the corrected roots) in float64 on the box's size in cells
__device__ __forceinline__ int gauss_radius(double h, double w, double m) {
  const double b1 = h + w;
  const double c1 = w * h * (1.0 - m) / (1.0 + m);
  const double r1 = (b1 - sqrt(b1 * b1 - 4.0 * c1)) / 2.0;
  const double b2 = 2.0 * (h + w);
  const double c2 = (1.0 - m) * w * h;
  const double r2 = (b2 - sqrt(b2 * b2 - 16.0 * c2)) / 8.0;
  const double a3 = 4.0 * m;
  const double b3 = -2.0 * m * (h + w);
  const double c3 = (m - 1.0) * w * h;
  const double r3 = (b3 + sqrt(b3 * b3 - 4.0 * a3 * c3)) / (2.0 * a3);
  const int r = (int)fmin(fmin(r1, r2), r3);
  return r > 0 ? r : 0;
}

// One thread per output element (cell, channel): the image's box records sit in LDS in ascending-area
// rank order (every block rebuilds them: n <= 256 boxes, a few in practice); a box-channel thread takes
// the last record on its cell, a class-channel thread the maximum heat over the records of its class.
__global__ void __launch_bounds__(kThreads) centernet_gauss_assign_kernel(GaussAssignArgs a) {
  const int b = blockIdx.y;
  const int tid = threadIdx.x;
  __shared__ float area[kMaxBox];
  __shared__ int order[kMaxBox];
  __shared__ int cy[kMaxBox], cx[kMaxBox], rr[kMaxBox], cc[kMaxBox];   // cc = -1: the box is skipped
  __shared__ float ts2[kMaxBox];
  __shared__ float off4[kMaxBox][4];
  int n = a.nbox[b];
  n = n < 0 ? 0 : (n > a.n_max ? a.n_max : n);
  const float H = a.img_dim[2 * b], W = a.img_dim[2 * b + 1];
  const float* bx = a.boxes + (size_t)b * a.n_max * 5;
  // stable ascending-area rank, the expressions of cvl_centernet_assign
  for (int i = tid; i < n; i += kThreads) area[i] = (bx[i * 5 + 2] * H) * (bx[i * 5 + 3] * W);
  __syncthreads();
  for (int i = tid; i < n; i += kThreads) {
    int r = 0;
    for (int j = 0; j < n; ++j) r += (area[j] < area[i]) || (area[j] == area[i] && j < i);
    order[r] = i;
  }
  __syncthreads();
  const float sf = (float)a.stride;
  const float py = (float)(int)((a.pad_h - H) / 2.0f), px = (float)(int)((a.pad_w - W) / 2.0f);
  for (int k = tid; k < n; k += kThreads) {
    const float* r = bx + order[k] * 5;
    const float c0 = (r[0] - 0.5f * r[2]) * H, c1 = (r[1] - 0.5f * r[3]) * W;
    const float c2 = (r[0] + 0.5f * r[2]) * H, c3 = (r[1] + 0.5f * r[3]) * W;
    const float ycf = (c0 + c2) / 2.0f, xcf = (c1 + c3) / 2.0f;
    const int yc = (int)((py + ycf) / sf), xc = (int)((px + xcf) / sf);
    const float lab = r[4];
    const int cls = (lab >= 0.f && lab < (float)a.C) ? (int)lab : -1;
    const bool keep = cls >= 0 && yc >= 0 && yc < a.hm && xc >= 0 && xc < a.wm;
    cy[k] = yc; cx[k] = xc; cc[k] = keep ? cls : -1;
    off4[k][0] = (float)((double)yc + 0.5) - (py + c0) / sf;
    off4[k][1] = ((py + c2) / sf - (float)yc) - 0.5f;
    off4[k][2] = (float)((double)xc + 0.5) - (px + c1) / sf;
    off4[k][3] = ((px + c3) / sf - (float)xc) - 0.5f;
    const float hc = ceilf((c2 - c0) / sf), wc = ceilf((c3 - c1) / sf);
    const int rad = gauss_radius((double)hc, (double)wc, a.m);
    const float sigma = (float)(2 * rad + 1) / 6.0f;
    rr[k] = rad;
    ts2[k] = 2.0f * sigma * sigma;
  }
  __syncthreads();
  const int row = 4 + a.C;
  const int total = a.hm * a.wm * row;
  float* out = a.out + (size_t)b * total;
  for (int e = blockIdx.x * kThreads + tid; e < total; e += gridDim.x * kThreads) {
    const int cell = e / row, ch = e - cell * row;
    const int y = cell / a.wm, x = cell - y * a.wm;
    float v = 0.f;
    if (ch < 4) {
      for (int k = 0; k < n; ++k)
        if (cc[k] >= 0 && cy[k] == y && cx[k] == x) v = off4[k][ch];
    } else {
      const int c = ch - 4;
      for (int k = 0; k < n; ++k) {
        if (cc[k] != c) continue;
        const int dy = y - cy[k], dx = x - cx[k], r = rr[k];
        if (dy < -r || dy > r || dx < -r || dx > r) continue;
        v = fmaxf(v, expf(-(float)(dy * dy + dx * dx) / ts2[k]));
      }
    }
    out[e] = v;
  }
}

// ---------------------------------------------------------------------------------------------
// norm: npos[b] = number of class entries equal to 1.0f (integer sums: any order gives the same count)
// ---------------------------------------------------------------------------------------------
template <bool VEC>
__global__ void __launch_bounds__(kThreads) centernet_gauss_norm_kernel(const float* tgt, int32_t* npos, int total,
                                                                        int row) {
  const int b = blockIdx.y;
  const float* t = tgt + (size_t)b * total;
  int cnt = 0;
  if (VEC) {
    const int nv = total >> 2;
    for (int i = blockIdx.x * kThreads + threadIdx.x; i < nv; i += gridDim.x * kThreads) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(t + 4 * (size_t)i);
      int ch = (4 * i) % row;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        cnt += (ch >= 4 && v[u] == 1.0f) ? 1 : 0;
        ch = ch + 1 == row ? 0 : ch + 1;
      }
    }
  } else {
    for (int e = blockIdx.x * kThreads + threadIdx.x; e < total; e += gridDim.x * kThreads)
      cnt += (e % row >= 4 && t[e] == 1.0f) ? 1 : 0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  __shared__ int red[kThreads / 64];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
    for (int k = 0; k < kThreads / 64; ++k) s += red[k];
    if (s) atomicAdd(&npos[b], s);
  }
}

// ---------------------------------------------------------------------------------------------
// loss
// ---------------------------------------------------------------------------------------------
struct GaussLossArgs {
  const float* pred;
  const float* tgt;
  const int32_t* npos;
  double* partial;     // [B][tiles][2]
  cvl_bf16* d;
  int ld_pred, ld_d, P, C, tiles, cpb;
  float alpha, beta, cls_scale, reg_scale;
};

__device__ __forceinline__ float pow_sel(float v, float e) {
  if (e == 2.0f) return v * v;
  if (e == 4.0f) return (v * v) * (v * v);
  return powf(v, e);
}

// one penalty-reduced focal element in the stable form of det_targets.hip's focal_elem:
//   y == 1:  (1-p)^alpha * -log p          d/dx = -(1-p)^alpha (alpha p (-log p) + (1-p))
//   else  :  (1-y)^beta p^alpha * -log(1-p)  d/dx = (1-y)^beta p^alpha (alpha (1-p) (-log(1-p)) + p)
__device__ __forceinline__ float gauss_focal_elem(float y, float x, float alpha, float beta, float* g) {
  const float e = expf(-fabsf(x));
  const float L = log1pf(e);
  const float p1 = x >= 0.f ? 1.0f / (1.0f + e) : e / (1.0f + e);
  const float q1 = x >= 0.f ? e / (1.0f + e) : 1.0f / (1.0f + e);
  const float nlp = L - fminf(x, 0.f), nlq = L + fmaxf(x, 0.f);
  if (y == 1.0f) {
    const float qa = pow_sel(q1, alpha);
    *g = -(qa * (alpha * p1 * nlp + q1));
    return qa * nlp;
  }
  const float w = pow_sel(1.0f - y, beta) * pow_sel(p1, alpha);
  *g = w * (alpha * q1 * nlq + p1);
  return w * nlq;
}

// A tile of cpb cells: the target rows (contiguous in memory) are staged in LDS by flat coalesced
// loads, each (cell, class) entry equal to 1.0f raising its cell's positive flag on the way; then the
// tile's prediction rows are walked in pieces of 8 channels (VEC: two 16-byte loads, one 16-byte bf16
// store per piece, consecutive lanes on consecutive pieces) or channel by channel.  A thread's terms
// are added in float64; the block's sums are a fixed-shape reduction.
template <bool VEC>
__global__ void __launch_bounds__(kThreads) centernet_gauss_loss_kernel(GaussLossArgs a) {
  extern __shared__ float rows[];
  const int b = blockIdx.y, p0 = blockIdx.x * a.cpb;
  const int ncell = min(a.cpb, a.P - p0);
  const int row = 4 + a.C;
  int* pos = reinterpret_cast<int*>(rows + a.cpb * row);
  const size_t cell0 = (size_t)b * a.P + p0;
  for (int i = threadIdx.x; i < ncell; i += kThreads) pos[i] = 0;
  __syncthreads();
  {
    const float* tg = a.tgt + cell0 * row;
    const int nelem = ncell * row;
    if (VEC && (row & 3) == 0) {
      for (int i = threadIdx.x; i < (nelem >> 2); i += kThreads) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(tg + 4 * i);
        *reinterpret_cast<f32x4*>(rows + 4 * i) = v;
        const int r = (4 * i) / row, c = 4 * i - r * row;    // row % 4 == 0: the four stay in one row
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (c + u >= 4 && v[u] == 1.0f) pos[r] = 1;
      }
    } else {
      for (int i = threadIdx.x; i < nelem; i += kThreads) {
        const float v = tg[i];
        rows[i] = v;
        const int r = i / row;
        if (i - r * row >= 4 && v == 1.0f) pos[r] = 1;
      }
    }
  }
  __syncthreads();
  const float N = (float)max(a.npos[b], 1);
  const float gc = a.cls_scale / N, gr = a.reg_scale / N;
  const int nch = 4 + a.C;
  double s_cls = 0.0, s_reg = 0.0;
  // one element: its loss term goes to the sums, its gradient is returned
  auto elem = [&](int r, int c, float x, float& lc, float& lr) -> float {
    const float t = rows[r * row + c];
    if (c >= 4) {
      float g;
      lc += gauss_focal_elem(t, x, a.alpha, a.beta, &g);
      return g * gc;
    }
    if (pos[r]) {                                   // by selection: a non-positive cell's x is not used
      lr += fabsf(t - x);
      return x > t ? gr : (x < t ? -gr : 0.f);
    }
    return 0.f;
  };
  if (VEC) {
    const int npc = a.ld_d >> 3;
    for (int i = threadIdx.x; i < ncell * npc; i += kThreads) {
      const int r = i / npc, c0 = (i - r * npc) << 3;
      const float* x = a.pred + (cell0 + r) * a.ld_pred + c0;
      f32x4 x0 = {0.f, 0.f, 0.f, 0.f}, x1 = {0.f, 0.f, 0.f, 0.f};
      if (c0 < nch) x0 = *reinterpret_cast<const f32x4*>(x);            // ld_pred % 4 == 0 and >= nch
      if (c0 + 4 < nch) x1 = *reinterpret_cast<const f32x4*>(x + 4);
      float lc = 0.f, lr = 0.f;
      s16x8 o;
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int c = c0 + u;
        const float xv = u < 4 ? x0[u & 3] : x1[u & 3];
        const float g = c < nch ? elem(r, c, xv, lc, lr) : 0.f;
        o[u] = (short)f32_to_bf16(g);
      }
      *reinterpret_cast<s16x8*>(a.d + (cell0 + r) * a.ld_d + c0) = o;
      s_cls += (double)lc;
      s_reg += (double)lr;
    }
  } else {
    for (int i = threadIdx.x; i < ncell * a.ld_d; i += kThreads) {
      const int r = i / a.ld_d, c = i - r * a.ld_d;
      float lc = 0.f, lr = 0.f, g = 0.f;
      if (c < nch) g = elem(r, c, a.pred[(cell0 + r) * a.ld_pred + c], lc, lr);
      a.d[(cell0 + r) * a.ld_d + c] = f32_to_bf16(g);
      s_cls += (double)lc;
      s_reg += (double)lr;
    }
  }
  __shared__ double red[2][kThreads / 64];
  const double v0 = warp_sum_d(s_cls), v1 = warp_sum_d(s_reg);
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) { red[0][w] = v0; red[1][w] = v1; }
  __syncthreads();
  if (threadIdx.x < 2) {
    double s = 0.0;
    for (int k = 0; k < kThreads / 64; ++k) s += red[threadIdx.x][k];
    a.partial[((size_t)b * a.tiles + blockIdx.x) * 2 + threadIdx.x] = s;
  }
}

// losses[b][k] = (sum_i partial[b][i][k]) / N: the fixed-order second pass of det_loss_finalize
__global__ void __launch_bounds__(kThreads) centernet_gauss_loss_finalize(const double* partial, const int32_t* npos,
                                                                          float* losses, int tiles) {
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
  if (t < 2) losses[b * 2 + t] = (float)(red[t][0] / (double)max(npos[b], 1));
}

// the tile: the most cells (256 / 128 / 64, and 32 for the widest rows) whose target rows and flags fit
// the LDS next to the block sums' static part
int loss_tile(int num_classes) {
  for (int n = 256; n >= 32; n /= 2)
    if ((size_t)n * (4 + num_classes + 1) * sizeof(float) <= 63 * 1024) return n;
  return 0;
}

}  // namespace

extern "C" int cvl_centernet_gauss_assign(const float* boxes, const int32_t* nbox, const float* img_dim, int B,
                                          int n_max, int pad_h, int pad_w, int num_classes, int stride,
                                          float min_overlap, float* targets, cvl_stream_t stream) {
  CVL_CHECK_ARG(boxes && nbox && img_dim && targets && B > 0 && n_max > 0 && n_max <= kMaxBox);
  CVL_CHECK_ARG(num_classes > 0 && num_classes <= kMaxClasses && stride > 0 && pad_h >= stride && pad_w >= stride);
  CVL_CHECK_ARG(min_overlap > 0.f && min_overlap < 1.0f);
  GaussAssignArgs a;
  a.boxes = boxes; a.nbox = nbox; a.img_dim = img_dim; a.out = targets; a.n_max = n_max;
  a.C = num_classes; a.stride = stride;
  a.hm = pad_h / stride;
  a.wm = pad_w / stride;
  a.pad_h = (float)pad_h; a.pad_w = (float)pad_w;
  a.m = (double)min_overlap;
  const long long total = (long long)a.hm * a.wm * (4 + num_classes);
  CVL_CHECK_ARG(total < (1ll << 31) - 256 * kThreads);
  int gx = (int)((total + kThreads - 1) / kThreads);
  gx = gx > 256 ? 256 : gx;
  hipLaunchKernelGGL(centernet_gauss_assign_kernel, dim3(gx, B), dim3(kThreads), 0, (hipStream_t)stream, a);
  return cvl_launch_status();
}

extern "C" int cvl_centernet_gauss_norm(const float* targets, int B, int P, int num_classes, int32_t* npos,
                                        cvl_stream_t stream) {
  CVL_CHECK_ARG(targets && npos && B > 0 && P > 0 && num_classes > 0);
  const int row = 4 + num_classes;
  const long long total = (long long)P * row;
  CVL_CHECK_ARG(total < (1ll << 31) - 4 * 256 * kThreads);
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(npos, 0, sizeof(int32_t) * B, s);
  if (e != hipSuccess) return CVL_EHIP + (int)e;
  const bool vec = total % 4 == 0 && (reinterpret_cast<uintptr_t>(targets) & 15) == 0;
  const long long work = vec ? total / 4 : total;
  int gx = (int)((work + kThreads - 1) / kThreads);
  gx = gx > 256 ? 256 : gx;
  if (vec)
    hipLaunchKernelGGL(centernet_gauss_norm_kernel<true>, dim3(gx, B), dim3(kThreads), 0, s, targets, npos,
                       (int)total, row);
  else
    hipLaunchKernelGGL(centernet_gauss_norm_kernel<false>, dim3(gx, B), dim3(kThreads), 0, s, targets, npos,
                       (int)total, row);
  return cvl_launch_status();
}

extern "C" size_t cvl_centernet_gauss_loss_workspace_size(int B, int P) {
  if (B <= 0 || P <= 0) return 0;
  return (size_t)B * ((size_t)(P + 31) / 32) * 2 * sizeof(double);   // per-tile partials of the smallest tiles
}

extern "C" int cvl_centernet_gauss_loss(const float* pred, int ld_pred, const float* targets, const int32_t* npos,
                                        int B, int P, int num_classes, float alpha, float beta, float cls_scale,
                                        float reg_scale, float* losses, void* d_pred, int ld_d, void* workspace,
                                        cvl_stream_t stream) {
  CVL_CHECK_ARG(pred && targets && npos && losses && d_pred && workspace && B > 0 && P > 0 && num_classes > 0);
  CVL_CHECK_ARG(ld_pred >= 4 + num_classes && ld_d >= 4 + num_classes);
  CVL_CHECK_ARG(alpha >= 0.f && beta >= 0.f);
  CVL_CHECK_ARG((long long)B * P * (long long)(ld_pred > ld_d ? ld_pred : ld_d) < (1ll << 40));
  GaussLossArgs a;
  a.cpb = loss_tile(num_classes);
  CVL_CHECK_ARG(a.cpb > 0);
  a.pred = pred; a.tgt = targets; a.npos = npos; a.partial = (double*)workspace; a.d = (cvl_bf16*)d_pred;
  a.ld_pred = ld_pred; a.ld_d = ld_d; a.P = P; a.C = num_classes;
  a.tiles = (P + a.cpb - 1) / a.cpb;
  a.alpha = alpha; a.beta = beta; a.cls_scale = cls_scale; a.reg_scale = reg_scale;
  const size_t lds = (size_t)a.cpb * (4 + num_classes + 1) * sizeof(float);
  // 16-byte accesses need rows that start on 16 bytes; CVL_DISPATCH=loss_rows forces the element form
  const bool vec = ld_d % 8 == 0 && ld_pred % 4 == 0 && (reinterpret_cast<uintptr_t>(d_pred) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(pred) & 15) == 0 && (reinterpret_cast<uintptr_t>(targets) & 15) == 0 &&
                   !cvl_dispatch_flag("loss_rows");
  hipStream_t s = (hipStream_t)stream;
  if (vec)
    hipLaunchKernelGGL(centernet_gauss_loss_kernel<true>, dim3(a.tiles, B), dim3(kThreads), lds, s, a);
  else
    hipLaunchKernelGGL(centernet_gauss_loss_kernel<false>, dim3(a.tiles, B), dim3(kThreads), lds, s, a);
  int st = cvl_launch_status();
  if (st) return st;
  hipLaunchKernelGGL(centernet_gauss_loss_finalize, dim3(B), dim3(kThreads), 0, s, (const double*)workspace, npos,
                     losses, a.tiles);
  return cvl_launch_status();
}
