// `bn_data`: the BatchNormalization(scale=False) that the ResNeXt backbones apply to the fp32 input
// image before conv0 (the `backbone_model="resnext50" | "resnext101"` branch of
// RetinaNet/retinanet_module.py:53-66).  Training-mode statistics per image and channel over the
// fp32 [B][H][W][3] image, the normalised fp32 image + beta, and the moving statistics.
//   * cvl_bn_data_stats: float64 partial (sum, sumsq) per (image, pixel chunk, channel), then one
//     small block sums the chunks in a fixed order, writes (mean, rstd) and runs the moving-average
//     update over the images in order (deterministic, no atomics);
//   * cvl_bn_data_apply: out = (img - mean) * rstd + beta, a 16-byte stream.
#include "cvl_common.h"
#include "bn_acc.h"

namespace {

constexpr int NT = 256;
constexpr int NCHUNK = 64;       // pixel chunks per image

// part[b][chunk][c][2] (float64)
__global__ void __launch_bounds__(NT) bn_data_partial_kernel(const float* __restrict__ img, double* __restrict__ part,
                                                             long HW) {
  const int b = blockIdx.y, chunk = blockIdx.x;
  const long per = (HW + NCHUNK - 1) / NCHUNK;
  const long p0 = chunk * per, p1 = p0 + per < HW ? p0 + per : HW;
  const float* src = img + (long)b * HW * 3;
  double s[3] = {0.0, 0.0, 0.0}, q[3] = {0.0, 0.0, 0.0};
  for (long p = p0 + threadIdx.x; p < p1; p += NT) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double v = (double)src[p * 3 + c];
      s[c] += v;
      q[c] += v * v;
    }
  }
  __shared__ double red[NT / 64][6];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    s[c] = warp_sum_d(s[c]);
    q[c] = warp_sum_d(q[c]);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      red[threadIdx.x >> 6][2 * c] = s[c];
      red[threadIdx.x >> 6][2 * c + 1] = q[c];
    }
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    double t = 0.0;
    for (int w = 0; w < NT / 64; ++w) t += red[w][threadIdx.x];
    part[((long)b * NCHUNK + chunk) * 6 + threadIdx.x] = t;
  }
}

// one block: thread (b, c) -> mean_rstd[b][c][2]; then thread c < 3 the moving statistics over b in order
__global__ void __launch_bounds__(NT) bn_data_finalize_kernel(const double* __restrict__ part, float* __restrict__ mr,
                                                              float* __restrict__ run_mean, float* __restrict__ run_var,
                                                              int B, long HW, float eps, float momentum) {
  for (int c = threadIdx.x; c < 3; c += NT) {
    float rm = run_mean ? run_mean[c] : 0.f, rv = run_var ? run_var[c] : 0.f;
    for (int b = 0; b < B; ++b) {
      double s1 = 0.0, s2 = 0.0;
      for (int k = 0; k < NCHUNK; ++k) {
        s1 += part[((long)b * NCHUNK + k) * 6 + 2 * c];
        s2 += part[((long)b * NCHUNK + k) * 6 + 2 * c + 1];
      }
      const double m = s1 / (double)HW;
      double var = s2 / (double)HW - m * m;
      var = var > 0.0 ? var : 0.0;
      mr[((long)b * 3 + c) * 2] = (float)m;
      mr[((long)b * 3 + c) * 2 + 1] = (float)(1.0 / sqrt(var + (double)eps));
      const double uvar = HW > 1 ? var * (double)HW / ((double)HW - 1.0) : var;    // as bn_running (bn_acc.h)
      rm = rm * momentum + (float)m * (1.f - momentum);
      rv = rv * momentum + (float)uvar * (1.f - momentum);
    }
    if (run_mean) run_mean[c] = rm;
    if (run_var) run_var[c] = rv;
  }
}

// 4 floats per thread: the channel of flat element e is e % 3
__global__ void __launch_bounds__(NT) bn_data_apply_kernel(const float* __restrict__ img, const float* __restrict__ mr,
                                                           const float* __restrict__ beta, float* __restrict__ out,
                                                           long n_img) {
  const int b = blockIdx.y;
  const float* src = img + (long)b * n_img;
  float* dst = out + (long)b * n_img;
  float m[3], rs[3], be[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    m[c] = mr[(b * 3 + c) * 2];
    rs[c] = mr[(b * 3 + c) * 2 + 1];
    be[c] = beta[c];
  }
  for (long e = (blockIdx.x * (long)NT + threadIdx.x) * 4; e < n_img; e += (long)gridDim.x * NT * 4) {
    int c = (int)(e % 3);
    if (e + 4 <= n_img && ((((size_t)(src + e)) | ((size_t)(dst + e))) & 15) == 0) {
      const float4 v = *reinterpret_cast<const float4*>(src + e);
      float f[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float mm = c == 0 ? m[0] : (c == 1 ? m[1] : m[2]);
        const float rr = c == 0 ? rs[0] : (c == 1 ? rs[1] : rs[2]);
        const float bb = c == 0 ? be[0] : (c == 1 ? be[1] : be[2]);
        f[u] = (f[u] - mm) * rr + bb;
        c = c == 2 ? 0 : c + 1;
      }
      *reinterpret_cast<float4*>(dst + e) = make_float4(f[0], f[1], f[2], f[3]);
    } else {
      for (long k = e; k < e + 4 && k < n_img; ++k) {
        const int ck = (int)(k % 3);
        dst[k] = (src[k] - m[ck]) * rs[ck] + be[ck];
      }
    }
  }
}

}  // namespace

#define S_ ((hipStream_t)stream)

extern "C" size_t cvl_bn_data_stats_workspace_size(int B) {
  return B > 0 ? (size_t)B * NCHUNK * 6 * sizeof(double) : 0;
}

extern "C" int cvl_bn_data_stats(const float* img, int B, int H, int W, float eps, float momentum, float* mean_rstd,
                                 float* run_mean, float* run_var, void* workspace, size_t workspace_bytes,
                                 cvl_stream_t stream) {
  CVL_CHECK_ARG(img && mean_rstd && workspace && B > 0 && B <= 65535 && H > 0 && W > 0);
  CVL_CHECK_ARG(((size_t)workspace & 7) == 0 && workspace_bytes >= cvl_bn_data_stats_workspace_size(B));
  double* part = reinterpret_cast<double*>(workspace);
  const long HW = (long)H * W;
  hipLaunchKernelGGL(bn_data_partial_kernel, dim3(NCHUNK, B), dim3(NT), 0, S_, img, part, HW);
  hipLaunchKernelGGL(bn_data_finalize_kernel, dim3(1), dim3(NT), 0, S_, (const double*)part, mean_rstd, run_mean,
                     run_var, B, HW, eps, momentum);
  return cvl_launch_status();
}

extern "C" int cvl_bn_data_apply(const float* img, const float* mean_rstd, const float* beta, float* out, int B, int H,
                                 int W, cvl_stream_t stream) {
  CVL_CHECK_ARG(img && mean_rstd && beta && out && B > 0 && B <= 65535 && H > 0 && W > 0);
  const long n_img = (long)H * W * 3;
  long blocks = (n_img / 4 + NT - 1) / NT;
  if (blocks < 1) blocks = 1;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(bn_data_apply_kernel, dim3((unsigned)blocks, B), dim3(NT), 0, S_, img, mean_rstd, beta, out, n_img);
  return cvl_launch_status();
}
