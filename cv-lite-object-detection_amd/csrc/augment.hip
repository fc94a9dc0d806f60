// Batched training augmentation on MI355X (cvlite extension, beyond the reference; DESIGN.md
// "Batched augmentation"): zoom-out, crop, flip, resize, colour, normalise and pad of a whole
// batch of decoded images of different sizes in ONE launch over a per-image descriptor table
// (cvl_augment_desc, include/cvlite.h) in device memory -- the host fills a pinned table, one copy
// moves it (the pattern of jpeg_decode.hip).  The draws are the caller's (cvlite/augment.py).
//
// Per image the result is DEFINED as this staged fp32 pipeline (restated in tests/augment_ref.py):
//   1. zoom-out  the source [H][W][3] at integer offset (oy, ox) on a canvas ch x cw of fill[3]
//   2. crop      the integer rectangle (y0, x0, hh, ww) of the canvas
//   3. flip      the crop mirrored left-right when flip is set
//   4. resize    TF-style bilinear to oh x ow, exactly resize_pad_kernel's arithmetic (preprocess.hip):
//                half-pixel centres, scale = in / out in fp32, taps clamped to the crop's border,
//                top = tl + (tr - tl) * xl, bottom = bl + (br - bl) * xl, v = top + (bottom - top) * yl
//   5. colour    v' = M v + t per pixel, evaluated as ((m0 * r + m1 * g) + m2 * b) + t per row
//   6. normalise / 127.5 - 1, zero padded bottom / right to ph x pw
// The kernel fuses the stages: per output pixel four taps, each either a source pixel or fill, the
// lerp, one mat-vec, the store; no canvas or crop is ever materialised.  THE FILL GOES THROUGH THE
// COLOUR MAP LIKE ANY OTHER PIXEL (stage 5 follows stage 1), and there is no clipping.  Built with
// -ffp-contract=off so no FMA changes a rounding; no atomics, so the output is deterministic.
//
// Work split: a tile is AUG_TILE = 1024 consecutive pixels of an image's padded ph x pw plane, the grid
// is (tiles of the largest image) x B and a workgroup whose image has fewer tiles exits at once.  The
// descriptor is indexed by blockIdx.y alone, so its reads are wave-uniform (scalar loads).  The
// output is 12 B per pixel: where pw % 4 == 0 and the destination is 16-byte aligned a lane owns 4
// consecutive pixels of one row (48 B) and writes them as three 16-B stores; otherwise a lane owns
// one pixel per pass and writes three dwords (the scalar path).
#include "cvl_common.h"

static_assert(sizeof(cvl_augment_desc) == 144, "descriptor layout");

namespace {

constexpr int PT = 256;
constexpr int AUG_VEC = 4;                     // pixels per lane on the 16-B path
constexpr int AUG_TILE = PT * AUG_VEC;         // pixels per workgroup, both paths

// the descriptor's pointers are device-memory pointers: told so, the compiler emits global_* accesses
// for them instead of flat_* ones
#define AUG_GLOBAL __attribute__((address_space(1)))
typedef float aug_f4 __attribute__((ext_vector_type(4)));      // a 16-byte store through such a pointer

// one tap of the crop at canvas position (Y, X): the source pixel when the position lies on the source,
// else fill.  A uint8 pixel is one unaligned 4-byte load (its 3 bytes and the next pixel's first) wherever
// those 4 bytes lie inside the source, and three byte loads at the image's last pixel.
template <bool U8>
__device__ __forceinline__ void load_tap(const cvl_augment_desc& d, int Y, int X, float v[3]) {
  const int sy = Y - d.oy, sx = X - d.ox;
  if (sy >= 0 && sy < d.H && sx >= 0 && sx < d.W) {
    const long o = ((long)sy * d.W + sx) * 3;
    if (U8) {
      const AUG_GLOBAL uint8_t* s = (const AUG_GLOBAL uint8_t*)d.src + o;
      if (o + 4 <= (long)d.H * d.W * 3) {
        uint32_t u;
        __builtin_memcpy(&u, (const void*)s, 4);
        v[0] = (float)(u & 255u); v[1] = (float)((u >> 8) & 255u); v[2] = (float)((u >> 16) & 255u);
      } else {
        v[0] = s[0]; v[1] = s[1]; v[2] = s[2];
      }
    } else {
      const AUG_GLOBAL float* s = (const AUG_GLOBAL float*)d.src + o;
      v[0] = s[0]; v[1] = s[1]; v[2] = s[2];
    }
  } else {
    v[0] = d.fill[0]; v[1] = d.fill[1]; v[2] = d.fill[2];
  }
}

// pixel (y, x) of the padded plane -> o[3]
template <bool U8>
__device__ __forceinline__ void pixel(const cvl_augment_desc& d, int y, int x, float o[3]) {
  if (y >= d.oh || x >= d.ow) {
    o[0] = o[1] = o[2] = 0.0f;
    return;
  }
  const float sy = (float)d.hh / (float)d.oh, sx = (float)d.ww / (float)d.ow;
  const float iny = ((float)y + 0.5f) * sy - 0.5f, inx = ((float)x + 0.5f) * sx - 0.5f;
  const float fy = floorf(iny), fx = floorf(inx);
  const int r0 = fy > 0.f ? (int)fy : 0, q0 = fx > 0.f ? (int)fx : 0;
  const int r1 = (int)ceilf(iny) < d.hh - 1 ? (int)ceilf(iny) : d.hh - 1;
  const int q1 = (int)ceilf(inx) < d.ww - 1 ? (int)ceilf(inx) : d.ww - 1;
  const float yl = iny - fy, xl = inx - fx;
  // crop column -> canvas column (the mirror acts on the crop), crop row -> canvas row
  const int X0 = d.x0 + (d.flip ? d.ww - 1 - q0 : q0), X1 = d.x0 + (d.flip ? d.ww - 1 - q1 : q1);
  const int Y0 = d.y0 + r0, Y1 = d.y0 + r1;
  float tl[3], tr[3], bl[3], br[3], v[3];
  load_tap<U8>(d, Y0, X0, tl);
  load_tap<U8>(d, Y0, X1, tr);
  load_tap<U8>(d, Y1, X0, bl);
  load_tap<U8>(d, Y1, X1, br);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float top = tl[c] + (tr[c] - tl[c]) * xl;
    const float bot = bl[c] + (br[c] - bl[c]) * xl;
    v[c] = top + (bot - top) * yl;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float w = ((d.m[c * 3] * v[0] + d.m[c * 3 + 1] * v[1]) + d.m[c * 3 + 2] * v[2]) + d.t[c];
    o[c] = w / 127.5f - 1.0f;
  }
}

template <bool U8>
__device__ __forceinline__ void tile(const cvl_augment_desc& d, long base, long npix, bool vec) {
  if (vec) {                                    // pw % 4 == 0: the lane's 4 pixels share a row
    const long p = base + (long)threadIdx.x * AUG_VEC;
    if (p >= npix) return;
    const int y = (int)(p / d.pw), x = (int)(p - (long)y * d.pw);
    float o[AUG_VEC * 3];
#pragma unroll
    for (int k = 0; k < AUG_VEC; ++k) pixel<U8>(d, y, x + k, o + k * 3);
    AUG_GLOBAL aug_f4* dst = (AUG_GLOBAL aug_f4*)(d.dst + p * 3);
    dst[0] = aug_f4{o[0], o[1], o[2], o[3]};
    dst[1] = aug_f4{o[4], o[5], o[6], o[7]};
    dst[2] = aug_f4{o[8], o[9], o[10], o[11]};
    return;
  }
#pragma unroll
  for (int k = 0; k < AUG_VEC; ++k) {
    const long p = base + (long)k * PT + threadIdx.x;
    if (p >= npix) return;
    const int y = (int)(p / d.pw), x = (int)(p - (long)y * d.pw);
    float o[3];
    pixel<U8>(d, y, x, o);
    AUG_GLOBAL float* dst = (AUG_GLOBAL float*)(d.dst + p * 3);
    dst[0] = o[0]; dst[1] = o[1]; dst[2] = o[2];
  }
}

__global__ void __launch_bounds__(PT) augment_batch_kernel(const cvl_augment_desc* __restrict__ table) {
  const cvl_augment_desc& d = table[blockIdx.y];           // wave-uniform
  const long npix = (long)d.ph * d.pw;
  const long base = (long)blockIdx.x * AUG_TILE;
  if (base >= npix) return;                                 // an image with fewer tiles
  const bool vec = (d.pw % AUG_VEC) == 0 && ((uintptr_t)d.dst & 15) == 0;
  if (d.src_u8)
    tile<true>(d, base, npix, vec);
  else
    tile<false>(d, base, npix, vec);
}

}  // namespace

extern "C" int cvl_augment_batch(const cvl_augment_desc* table, const cvl_augment_desc* table_dev, int B,
                                 cvl_stream_t stream) {
  CVL_CHECK_ARG(table && table_dev && B >= 1 && B <= CVL_AUGMENT_MAX_BATCH);
  long max_tiles = 0;
  for (int i = 0; i < B; ++i) {
    const cvl_augment_desc& d = table[i];
    CVL_CHECK_ARG(d.src && d.dst && (d.src_u8 == 0 || d.src_u8 == 1) && (d.flip == 0 || d.flip == 1));
    CVL_CHECK_ARG(d.H > 0 && d.W > 0 && d.ch > 0 && d.cw > 0 && d.ch <= CVL_AUGMENT_MAX_SIDE && d.cw <= CVL_AUGMENT_MAX_SIDE);
    // the source lies inside the canvas, the crop lies inside the canvas
    CVL_CHECK_ARG(d.oy >= 0 && d.ox >= 0 && d.oy <= d.ch - d.H && d.ox <= d.cw - d.W);
    CVL_CHECK_ARG(d.y0 >= 0 && d.x0 >= 0 && d.hh > 0 && d.ww > 0 && d.y0 <= d.ch - d.hh && d.x0 <= d.cw - d.ww);
    CVL_CHECK_ARG(d.oh > 0 && d.ow > 0 && d.oh <= d.ph && d.ow <= d.pw && d.ph <= CVL_AUGMENT_MAX_SIDE &&
                  d.pw <= CVL_AUGMENT_MAX_SIDE && (long)d.ph * d.pw < (1L << 31));
    const long tiles = ((long)d.ph * d.pw + AUG_TILE - 1) / AUG_TILE;
    max_tiles = tiles > max_tiles ? tiles : max_tiles;
  }
  hipLaunchKernelGGL(augment_batch_kernel, dim3((unsigned)max_tiles, (unsigned)B), dim3(PT), 0, (hipStream_t)stream,
                     table_dev);
  return cvl_launch_status();
}
