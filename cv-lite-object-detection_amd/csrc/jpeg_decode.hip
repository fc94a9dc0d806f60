// Batched baseline-JPEG decode on MI355X (include/cvlite.h "JPEG decode").
//
// Hybrid, as the established GPU decoders are: the serial Huffman bit stream is decoded on the host
// (jpeg_host.h, several images at once on std::threads) into int16 coefficients in a pinned staging
// buffer; one copy moves the whole batch; two launches cover every image of the batch:
//
//   jpeg_idct_kernel    dequantise + libjpeg's "islow" 8x8 inverse DCT -> uint8 component planes
//   jpeg_colour_kernel  fancy (triangle) chroma upsampling + YCbCr -> RGB + crop -> [H][W][3] uint8
//
// All arithmetic is 32-bit integer with arithmetic right shifts, in libjpeg's order, so the pixels
// are the bytes PIL's Image.convert("RGB") returns (tests/test_gpu_jpeg.py compares for equality).
#include "cvl_common.h"
#include "jpeg_host.h"

#include <atomic>
#include <vector>
#include <thread>

namespace {

using cvl_jpeg::Header;

// One image of the batch, as both kernels see it (built on the host in the staging buffer, read
// from the workspace copy).  Offsets are bytes from the workspace base.
struct JpegDesc {
  uint64_t coef_off;              // int16 [blocks][64], component-planar
  uint64_t qt_off;                // uint16 [3][64]
  uint64_t plane_off;             // uint8 planes; component c's starts blk_start[c] * 64 bytes in
  uint8_t* out;                   // [height][width][3]
  int32_t width, height, ncomp, hs, vs;
  int32_t bw[3], blk_start[3];    // blocks per row / first block of each component
  int32_t nblocks;                // 0: the image is skipped
};
static_assert(sizeof(JpegDesc) == 80, "descriptor layout");

constexpr size_t ALIGN = 256;
constexpr size_t align_up(size_t v) { return (v + ALIGN - 1) / ALIGN * ALIGN; }
constexpr size_t staging_bytes_of(size_t coef_count) { return align_up(coef_count * 2 + 3 * 64 * 2); }

// ---- dequantise + inverse DCT ----------------------------------------------------------------
constexpr int IDCT_THREADS = 256;
constexpr int IDCT_BLOCKS = IDCT_THREADS / 8;        // 8 lanes per 8x8 block

// libjpeg jidctint.c, 13-bit fixed point
constexpr int C0_298 = 2446, C0_390 = 3196, C0_541 = 4433, C0_765 = 6270, C0_899 = 7373, C1_175 = 9633,
              C1_501 = 12299, C1_847 = 15137, C1_961 = 16069, C2_053 = 16819, C2_562 = 20995, C3_072 = 25172;

// one 8-point pass; the caller descales
__device__ __forceinline__ void idct8(const int* x, int* y) {
  int z1 = (x[2] + x[6]) * C0_541;
  const int t2 = z1 - x[6] * C1_847;
  const int t3 = z1 + x[2] * C0_765;
  const int t0 = (x[0] + x[4]) * 8192;
  const int t1 = (x[0] - x[4]) * 8192;
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  int a0 = x[7], a1 = x[5], a2 = x[3], a3 = x[1];
  z1 = a0 + a3;
  int z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
  const int z5 = (z3 + z4) * C1_175;
  a0 *= C0_298; a1 *= C2_053; a2 *= C3_072; a3 *= C1_501;
  z1 *= -C0_899;
  z2 *= -C2_562;
  z3 = z3 * -C1_961 + z5;
  z4 = z4 * -C0_390 + z5;
  a0 += z1 + z3; a1 += z2 + z4; a2 += z2 + z3; a3 += z1 + z4;
  y[0] = t10 + a3; y[1] = t11 + a2; y[2] = t12 + a1; y[3] = t13 + a0;
  y[4] = t13 - a0; y[5] = t12 - a1; y[6] = t11 - a2; y[7] = t10 - a3;
}

// grid (ceil(max blocks per image / IDCT_BLOCKS), images).  Lane j of a block's 8 loads coefficient
// row j (16 bytes) and its quantisation row, the block is transposed through LDS for the column
// pass and back for the row pass, and lane j stores output row j (8 bytes).
__global__ void __launch_bounds__(IDCT_THREADS) jpeg_idct_kernel(uint8_t* ws) {
  __shared__ int tile[IDCT_BLOCKS][8][9];
  const JpegDesc& d = reinterpret_cast<const JpegDesc*>(ws)[blockIdx.y];
  const int nblocks = d.nblocks;
  if ((int)blockIdx.x * IDCT_BLOCKS >= nblocks) return;      // whole workgroup: no barrier is skipped
  const int lb = threadIdx.x >> 3, j = threadIdx.x & 7;
  const int g = (int)blockIdx.x * IDCT_BLOCKS + lb;
  const bool live = g < nblocks;
  int c = 0;
  if (live) {
    c = g >= d.blk_start[1] && d.ncomp > 1 ? (g >= d.blk_start[2] ? 2 : 1) : 0;
    const int4 cv = *reinterpret_cast<const int4*>(ws + d.coef_off + (uint64_t)g * 128 + j * 16);
    const int4 qv = *reinterpret_cast<const int4*>(ws + d.qt_off + c * 128 + j * 16);
    const int cw[4] = {cv.x, cv.y, cv.z, cv.w}, qw[4] = {qv.x, qv.y, qv.z, qv.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      tile[lb][j][2 * k] = (int)(int16_t)(cw[k] & 0xffff) * (qw[k] & 0xffff);
      tile[lb][j][2 * k + 1] = (cw[k] >> 16) * (int)((uint32_t)qw[k] >> 16);
    }
  }
  __syncthreads();
  int x[8], y[8];
  if (live) {
#pragma unroll
    for (int r = 0; r < 8; ++r) x[r] = tile[lb][r][j];       // column j
    idct8(x, y);
  }
  __syncthreads();
  if (live) {
#pragma unroll
    for (int r = 0; r < 8; ++r) tile[lb][r][j] = (y[r] + (1 << 10)) >> 11;
  }
  __syncthreads();
  if (live) {
#pragma unroll
    for (int k = 0; k < 8; ++k) x[k] = tile[lb][j][k];       // row j
    idct8(x, y);
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int v = min(255, max(0, ((y[k] + (1 << 17)) >> 18) + 128));
      if (k < 4) lo |= (uint32_t)v << (8 * k);
      else hi |= (uint32_t)v << (8 * (k - 4));
    }
    const int local = g - d.blk_start[c];
    const int brow = local / d.bw[c], bcol = local - brow * d.bw[c];
    uint8_t* plane = ws + d.plane_off + (uint64_t)d.blk_start[c] * 64;
    *reinterpret_cast<uint2*>(plane + ((uint64_t)(brow * 8 + j) * d.bw[c] + bcol) * 8) = make_uint2(lo, hi);
  }
}

// ---- upsample + colour + crop ------------------------------------------------------------------
constexpr int COL_RUN = 4;                           // pixels per lane
constexpr int COL_TX = 64, COL_TY = 4;               // lanes across / rows per workgroup

// chroma sample for pixel (y, x): libjpeg's fancy upsampling (jdsample.c h2v1 / h2v2 fancy) on the
// plane cropped to dw x dh, neighbours outside it being the edge sample; planes of at most two
// columns are replicated instead, as libjpeg does.
__device__ __forceinline__ int chroma_at(const uint8_t* p, int stride, int dw, int dh, int hs, int vs, int y, int x) {
  if (hs == 1) return p[(size_t)y * stride + x];
  const int i = x >> 1;
  if (dw <= 2) return p[(size_t)(vs == 2 ? y >> 1 : y) * stride + i];
  const int in = (x & 1) ? min(i + 1, dw - 1) : max(i - 1, 0);
  if (vs == 1) {
    const uint8_t* row = p + (size_t)y * stride;
    return (3 * row[i] + row[in] + 1 + (x & 1)) >> 2;
  }
  const int r = y >> 1;
  const int rn = (y & 1) ? min(r + 1, dh - 1) : max(r - 1, 0);
  const uint8_t* r0 = p + (size_t)r * stride;
  const uint8_t* r1 = p + (size_t)rn * stride;
  const int t = 3 * r0[i] + r1[i], tn = 3 * r0[in] + r1[in];
  return (3 * t + tn + 8 - (x & 1)) >> 4;
}

// grid (ceil(max width / (COL_TX * COL_RUN)), ceil(max height / COL_TY), images); a lane writes
// COL_RUN adjacent pixels (12 bytes: three dword stores when the address allows it).
__global__ void __launch_bounds__(COL_TX * COL_TY) jpeg_colour_kernel(const uint8_t* ws) {
  const JpegDesc& d = reinterpret_cast<const JpegDesc*>(ws)[blockIdx.z];
  if (d.nblocks == 0) return;
  const int W = d.width, H = d.height;
  const int y = (int)blockIdx.y * COL_TY + (int)(threadIdx.x / COL_TX);
  const int x0 = ((int)blockIdx.x * COL_TX + (int)(threadIdx.x % COL_TX)) * COL_RUN;
  if (y >= H || x0 >= W) return;
  const uint8_t* planes = ws + d.plane_off;
  const uint8_t* py = planes;
  const int sy = d.bw[0] * 8;
  const int nx = min(COL_RUN, W - x0);
  uint8_t px[COL_RUN * 3];
  if (d.ncomp == 1) {
    for (int k = 0; k < nx; ++k) px[3 * k] = px[3 * k + 1] = px[3 * k + 2] = py[(size_t)y * sy + x0 + k];
  } else {
    const uint8_t* pcb = planes + (size_t)d.blk_start[1] * 64;
    const uint8_t* pcr = planes + (size_t)d.blk_start[2] * 64;
    const int sc = d.bw[1] * 8;
    const int dw = (W + d.hs - 1) / d.hs, dh = (H + d.vs - 1) / d.vs;
    for (int k = 0; k < nx; ++k) {
      const int x = x0 + k;
      const int Y = py[(size_t)y * sy + x];
      const int cb = chroma_at(pcb, sc, dw, dh, d.hs, d.vs, y, x) - 128;
      const int cr = chroma_at(pcr, sc, dw, dh, d.hs, d.vs, y, x) - 128;
      px[3 * k] = (uint8_t)min(255, max(0, Y + ((91881 * cr + 32768) >> 16)));
      px[3 * k + 1] = (uint8_t)min(255, max(0, Y + ((-22554 * cb - 46802 * cr + 32768) >> 16)));
      px[3 * k + 2] = (uint8_t)min(255, max(0, Y + ((116130 * cb + 32768) >> 16)));
    }
  }
  uint8_t* o = d.out + ((size_t)y * W + x0) * 3;
  if (nx == COL_RUN && ((uintptr_t)o & 3) == 0) {
    uint32_t* o4 = reinterpret_cast<uint32_t*>(o);
#pragma unroll
    for (int k = 0; k < 3; ++k)
      o4[k] = px[4 * k] | (uint32_t)px[4 * k + 1] << 8 | (uint32_t)px[4 * k + 2] << 16 | (uint32_t)px[4 * k + 3] << 24;
  } else {
    for (int k = 0; k < nx * 3; ++k) o[k] = px[k];
  }
}

int jpeg_threads() {
  const char* v = getenv("CVL_JPEG_THREADS");
  const int t = (v && v[0]) ? atoi(v) : 8;
  return t < 1 ? 1 : (t > 16 ? 16 : t);
}

}  // namespace

extern "C" int cvl_jpeg_info(const uint8_t* data, size_t nbytes, int32_t* info) {
  return cvl_jpeg::info(data, nbytes, info);
}

extern "C" int cvl_jpeg_entropy_decode(const uint8_t* data, size_t nbytes, int16_t* coef, size_t coef_cap,
                                       uint16_t* qt) {
  return cvl_jpeg::decode_coefficients(data, nbytes, coef, coef_cap, qt);
}

extern "C" int cvl_jpeg_batch_sizes(const int32_t* coef_counts, int n, size_t* staging_bytes,
                                    size_t* workspace_bytes) {
  CVL_CHECK_ARG(coef_counts && n > 0 && n <= CVL_JPEG_MAX_BATCH && staging_bytes && workspace_bytes);
  size_t st = align_up((size_t)n * sizeof(JpegDesc)), planes = 0;
  for (int i = 0; i < n; ++i) {
    CVL_CHECK_ARG(coef_counts[i] >= 0 && coef_counts[i] % 64 == 0);
    if (coef_counts[i] == 0) continue;
    st += staging_bytes_of((size_t)coef_counts[i]);
    planes += align_up((size_t)coef_counts[i]);
  }
  *staging_bytes = st;
  *workspace_bytes = st + planes;
  return CVL_OK;
}

extern "C" int cvl_jpeg_decode_batch(const uint8_t* const* data, const size_t* nbytes, int n, uint8_t* const* out,
                                     void* staging, size_t staging_bytes, void* workspace, size_t workspace_bytes,
                                     int32_t* status, cvl_stream_t stream) {
  CVL_CHECK_ARG(data && nbytes && out && staging && workspace && status && n > 0 && n <= CVL_JPEG_MAX_BATCH);
  CVL_CHECK_ARG(((uintptr_t)staging & 15) == 0 && ((uintptr_t)workspace & 15) == 0);
  // 1. headers: the layout of the staging buffer and of the workspace
  std::vector<Header> hdr((size_t)n);
  JpegDesc* desc = static_cast<JpegDesc*>(staging);
  size_t used = align_up((size_t)n * sizeof(JpegDesc));
  CVL_CHECK_ARG(used <= staging_bytes);
  int max_blocks = 0, max_w = 0, max_h = 0, n_ok = 0;
  for (int i = 0; i < n; ++i) {
    status[i] = data[i] ? cvl_jpeg::parse_header(data[i], nbytes[i], &hdr[i]) : CVL_JPEG_UNSUPPORTED;
    if (status[i] == CVL_OK && !out[i]) status[i] = CVL_EINVAL;
    JpegDesc& d = desc[i];
    memset(&d, 0, sizeof(d));
    if (status[i] != CVL_OK) continue;
    const Header& h = hdr[i];
    const size_t cc = h.coef_count();
    CVL_CHECK_ARG(used + staging_bytes_of(cc) <= staging_bytes);
    d.coef_off = used;
    d.qt_off = used + cc * 2;
    used += staging_bytes_of(cc);
    d.out = out[i];
    d.width = h.width; d.height = h.height; d.ncomp = h.ncomp; d.hs = h.hmax; d.vs = h.vmax;
    for (int c = 0; c < 3; ++c) { d.bw[c] = h.bw[c]; d.blk_start[c] = h.blk_start[c]; }
    d.nblocks = h.blk_start[h.ncomp];
    ++n_ok;
  }
  size_t wused = used;
  for (int i = 0; i < n; ++i) {
    if (status[i] != CVL_OK) continue;
    desc[i].plane_off = wused;
    wused += align_up((size_t)desc[i].nblocks * 64);
  }
  CVL_CHECK_ARG(wused <= workspace_bytes);
  if (n_ok == 0) return CVL_OK;
  // 2. entropy decode on the host threads; the next image is taken from a shared counter
  std::atomic<int> next(0);
  auto work = [&]() {
    for (int i = next.fetch_add(1); i < n; i = next.fetch_add(1)) {
      if (status[i] != CVL_OK) continue;
      uint8_t* base = static_cast<uint8_t*>(staging);
      const int st = cvl_jpeg::entropy_decode(data[i], nbytes[i], hdr[i], reinterpret_cast<int16_t*>(base + desc[i].coef_off),
                                              reinterpret_cast<uint16_t*>(base + desc[i].qt_off));
      if (st != CVL_OK) {
        status[i] = st;
        desc[i].nblocks = 0;
      }
    }
  };
  const int nthreads = n_ok < jpeg_threads() ? n_ok : jpeg_threads();
  if (nthreads <= 1) {
    work();
  } else {
    std::vector<std::thread> pool;
    pool.reserve((size_t)nthreads);
    for (int t = 0; t < nthreads; ++t) pool.emplace_back(work);
    for (auto& t : pool) t.join();
  }
  for (int i = 0; i < n; ++i) {
    if (desc[i].nblocks == 0) continue;
    max_blocks = desc[i].nblocks > max_blocks ? desc[i].nblocks : max_blocks;
    max_w = desc[i].width > max_w ? desc[i].width : max_w;
    max_h = desc[i].height > max_h ? desc[i].height : max_h;
  }
  if (max_blocks == 0) return CVL_OK;
  // 3. one copy, two launches
  const hipStream_t s = (hipStream_t)stream;
  const hipError_t e = hipMemcpyAsync(workspace, staging, used, hipMemcpyHostToDevice, s);
  if (e != hipSuccess) return CVL_EHIP + (int)e;
  hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)((max_blocks + IDCT_BLOCKS - 1) / IDCT_BLOCKS), (unsigned)n),
                     dim3(IDCT_THREADS), 0, s, static_cast<uint8_t*>(workspace));
  hipLaunchKernelGGL(jpeg_colour_kernel,
                     dim3((unsigned)((max_w + COL_TX * COL_RUN - 1) / (COL_TX * COL_RUN)),
                          (unsigned)((max_h + COL_TY - 1) / COL_TY), (unsigned)n),
                     dim3(COL_TX * COL_TY), 0, s, static_cast<const uint8_t*>(workspace));
  return cvl_launch_status();
}
