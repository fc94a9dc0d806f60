// Inference with BatchNorm folded into the convolutions (ConvBN.fold / ResNet50.fold_bn): BN with
// the moving statistics is the per-channel affine map y = s * z + t, s = gamma / sqrt(var + eps), so
// conv -> BN is one conv with weights w * s[co] and bias (b - mean) * s + beta.  Here: the batched
// forward re-pack of the scaled weights, and the in-place ReLU that follows a residual conv whose plan
// has no fused relu(conv + bias + old) epilogue (cvl_conv_igemm_res_relu).
#include "conv_common.h"

namespace {

constexpr int NT = 256;

// One workgroup per 64 (ci) x 64 (co) block of one tap of one item, as the unscaled batched pack
// (nn_ops.hip pack_multi_kernel): coalesced fp32 reads of the HWIO slab [ci][co] into LDS, one fp32
// multiply by scale[co], then 16-byte bf16 stores of the forward image [co][tap * Cin_k + ci].
// Rows co >= Cout and channels ci >= Cin are written as zeros.
__global__ void __launch_bounds__(NT) pack_scaled_multi_kernel(const cvl_pack_scaled_item* __restrict__ items,
                                                               const int4* __restrict__ tiles) {
  const int4 t = tiles[blockIdx.x];
  const cvl_pack_scaled_item it = items[t.x];
  const int tap = t.y, ci0 = t.z, co0 = t.w;
  __shared__ float tile[64][65];
  const float* src = it.w + (long)tap * it.Cin * it.Cout;
  const int col = threadIdx.x & 63, r0 = threadIdx.x >> 6;
  const int co_l = co0 + col;
  const float sc = co_l < it.Cout ? it.scale[co_l] : 0.f;
#pragma unroll 4
  for (int j = 0; j < 16; ++j) {
    const int r = r0 + 4 * j, ci = ci0 + r;
    tile[r][col] = (ci < it.Cin && co_l < it.Cout) ? src[(long)ci * it.Cout + co_l] * sc : 0.f;
  }
  __syncthreads();
  const long K = (long)it.KHW * it.Cin_k;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int idx = threadIdx.x + j * NT;
    const int r = idx >> 3, c8 = (idx & 7) * 8;
    const int co = co0 + r, ci = ci0 + c8;       // row co, channels ci .. ci + 7 of tap
    if (co < it.Npad && ci < it.Cin_k) {
      s16x8 v;
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = (short)f32_to_bf16(tile[c8 + u][r]);
      *reinterpret_cast<s16x8*>(reinterpret_cast<cvl_bf16*>(it.w_fwd) + co * K + (long)tap * it.Cin_k + ci) = v;
    }
  }
}

// x = max(x, 0) on bf16 bits, 8 elements (16 bytes) per thread and step
__global__ void __launch_bounds__(NT) relu_inplace_kernel(cvl_bf16* x, long n8, long n) {
  s16x8* xv = reinterpret_cast<s16x8*>(x);
  const long step = (long)gridDim.x * NT;
  for (long i = blockIdx.x * (long)NT + threadIdx.x; i < n8; i += step) {
    s16x8 v = xv[i];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = relu_bf16_bits(v[u]);
    xv[i] = v;
  }
  // the n % 8 elements after the last whole vector
  const long t = n8 * 8 + blockIdx.x * (long)NT + threadIdx.x;
  if (t < n) x[t] = (cvl_bf16)relu_bf16_bits((short)x[t]);
}

// the same element by element (a pointer off the 16-byte grid)
__global__ void __launch_bounds__(NT) relu_inplace_scalar_kernel(cvl_bf16* x, long n) {
  for (long i = blockIdx.x * (long)NT + threadIdx.x; i < n; i += (long)gridDim.x * NT)
    x[i] = (cvl_bf16)relu_bf16_bits((short)x[i]);
}

inline int grid_for(long n, int cap = 8192) {
  const long b = (n + NT - 1) / NT;
  return (int)(b > cap ? cap : (b < 1 ? 1 : b));
}

}  // namespace

extern "C" int cvl_pack_conv_weights_scaled_multi(const cvl_pack_scaled_item* items, const int32_t* tiles, int ntiles,
                                                  cvl_stream_t stream) {
  CVL_CHECK_ARG(items && tiles && ntiles >= 0);
  if (ntiles == 0) return CVL_OK;
  hipLaunchKernelGGL(pack_scaled_multi_kernel, dim3(ntiles), dim3(NT), 0, (hipStream_t)stream, items,
                     reinterpret_cast<const int4*>(tiles));
  return cvl_launch_status();
}

extern "C" int cvl_relu_(void* x, long n, cvl_stream_t stream) {
  CVL_CHECK_ARG(x && n >= 0 && ((uintptr_t)x & 1) == 0);
  if (n == 0) return CVL_OK;
  cvl_bf16* p = reinterpret_cast<cvl_bf16*>(x);
  if ((uintptr_t)x & 15) {
    hipLaunchKernelGGL(relu_inplace_scalar_kernel, dim3(grid_for(n)), dim3(NT), 0, (hipStream_t)stream, p, n);
  } else {
    hipLaunchKernelGGL(relu_inplace_kernel, dim3(grid_for(n / 8)), dim3(NT), 0, (hipStream_t)stream, p, n / 8, n);
  }
  return cvl_launch_status();
}
