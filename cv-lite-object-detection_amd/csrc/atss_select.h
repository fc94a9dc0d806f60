// The candidate selection shared by the two ATSS assignments (fcos_atss.hip, retina_atss.hip): the key a
// squared distance orders by, the wave minimum by DPP moves, the select rounds that chain it, and the
// window about the box centre with its check.  The two callers differ in where a level's grid lines lie
// (`pos`: FCOS points sit at (q + 0.5) * stride, RetinaNet anchors at q * stride) and in how many cells
// they take.  Internal header: not part of the C ABI.
#pragma once
#include "cvl_common.h"

constexpr unsigned kNanKey = 0x7FC00000u;     // orders a NaN distance above +inf

// a squared distance (>= 0, or NaN) as the unsigned integer that orders as the rule does
__device__ __forceinline__ unsigned ord_bits(float v) { return v != v ? kNanKey : __float_as_uint(v); }

// Wave minimum by DPP moves (register-to-register, no LDS round trip as a shuffle has; the select
// rounds are a chain of these): a scan within each row of 16 lanes by row_shr 1, 2, 4, 8, then
// row_bcast:15 into rows 1 and 3 and row_bcast:31 into rows 2 and 3 leave the minimum in lane 63.  A
// lane without a source takes the identity, all ones.  Every lane of the wave must be active.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ unsigned dpp_or_ones(unsigned v) {
  return (unsigned)__builtin_amdgcn_update_dpp(-1, (int)v, CTRL, ROW_MASK, 0xF, false);
}

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ unsigned long long min_step_u64(unsigned long long v) {
  const unsigned lo = dpp_or_ones<CTRL, ROW_MASK>((unsigned)v);
  const unsigned hi = dpp_or_ones<CTRL, ROW_MASK>((unsigned)(v >> 32));
  const unsigned long long u = ((unsigned long long)hi << 32) | lo;
  return u < v ? u : v;
}

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ unsigned min_step_u32(unsigned v) {
  const unsigned u = dpp_or_ones<CTRL, ROW_MASK>(v);
  return u < v ? u : v;
}

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
  v = min_step_u64<0x111, 0xF>(v);      // row_shr:1
  v = min_step_u64<0x112, 0xF>(v);      // row_shr:2
  v = min_step_u64<0x114, 0xF>(v);      // row_shr:4
  v = min_step_u64<0x118, 0xF>(v);      // row_shr:8
  v = min_step_u64<0x142, 0xA>(v);      // row_bcast:15
  v = min_step_u64<0x143, 0xC>(v);      // row_bcast:31
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, 63);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), 63);
  return ((unsigned long long)hi << 32) | lo;
}

__device__ __forceinline__ unsigned wave_min_u32(unsigned v) {
  v = min_step_u32<0x111, 0xF>(v);
  v = min_step_u32<0x112, 0xF>(v);
  v = min_step_u32<0x114, 0xF>(v);
  v = min_step_u32<0x118, 0xF>(v);
  v = min_step_u32<0x142, 0xA>(v);
  v = min_step_u32<0x143, 0xC>(v);
  return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}

constexpr int kSelectCache = 18;              // keys per lane of the widest window: ceil(33 * 33 / 64)

// k rounds of a wave arg-min of (d2 bits << 32 | row-major cell index) over the rows r0..r1, columns
// c0..c1 of a level, d2 = (pos(row) - yc)^2 + (pos(col) - xc)^2; round j's key lands in lane j's `mine`.
// The keys are distinct, so round j takes the smallest key above round j-1's.  Returns the last round's
// key.
template <class Pos>
__device__ __forceinline__ unsigned long long atss_select_rounds(int k, int r0, int r1, int c0, int c1, int Ws, Pos pos,
                                                                 float yc, float xc, int lane,
                                                                 unsigned long long& mine) {
  const int wc = c1 - c0 + 1;
  const int nwin = (r1 - r0 + 1) * wc;
  auto key_of = [&](int e) {
    const int cy = r0 + e / wc, cx = c0 + e % wc;
    const float gy = pos(cy), gx = pos(cx);
    const float dy = gy - yc, dx = gx - xc;
    const float d2 = dy * dy + dx * dx;
    return ((unsigned long long)ord_bits(d2) << 32) | (unsigned)(cy * Ws + cx);
  };
  unsigned long long last = 0;
  if (nwin <= 64 * kSelectCache) {
    // the window's keys are computed once and held in registers (kSelectCache per lane)
    const int ne = (nwin + 63) / 64;
    unsigned long long kk[kSelectCache];
#pragma unroll
    for (int u = 0; u < kSelectCache; ++u) {
      const int e = u * 64 + lane;
      kk[u] = (u < ne && e < nwin) ? key_of(e) : ~0ull;
    }
    for (int j = 0; j < k; ++j) {
      unsigned long long best = ~0ull;
#pragma unroll
      for (int u = 0; u < kSelectCache; ++u)
        if (u < ne) {
          const unsigned long long key = kk[u];
          if ((j == 0 || key > last) && key < best) best = key;
        }
      best = wave_min_u64(best);
      if (lane == j) mine = best;
      last = best;
    }
    return last;
  }
  // a larger range (the whole of a large level): the keys are computed again in every round
  for (int j = 0; j < k; ++j) {
    unsigned long long best = ~0ull;
    for (int e = lane; e < nwin; e += 64) {
      const unsigned long long key = key_of(e);
      if ((j == 0 || key > last) && key < best) best = key;
    }
    best = wave_min_u64(best);
    if (lane == j) mine = best;
    last = best;
  }
  return last;
}

// The smallest squared distance along one axis over the cells outside [w0, w1] (`out`) and over all
// n cells (`all`), as ord_bits.
template <class Pos>
__device__ __forceinline__ void atss_axis_minima(int n, int w0, int w1, Pos pos, float c, int lane, unsigned& out,
                                                 unsigned& all) {
  unsigned mo = kNanKey, ma = kNanKey;
  for (int q = lane; q < n; q += 64) {
    const float g = pos(q);
    const float d = g - c;
    const unsigned v = ord_bits(d * d);
    ma = v < ma ? v : ma;
    if (q < w0 || q > w1) mo = v < mo ? v : mo;
  }
  out = wave_min_u32(mo);
  all = wave_min_u32(ma);
}

// The k <= 64 cells of an Hs x Ws level nearest (yc, xc), ties to the lowest row-major index, by one
// wave: lane j's `mine` gets the key of rank j.  The rounds run over the window of `half` cells either
// side of the clamped cell of the centre (a NaN centre clamps to 0).  d2 = fl(a_r + b_s) is monotone in
// a_r = dy^2 and b_s = dx^2, so the smallest d2 outside the window is the smaller of
// fl(min a outside + min b) and fl(min a + min b outside).  Unless that is strictly above the k-th
// selected d2 (a far-off centre whose distances round together), the rounds run again over the whole
// level.  Every lane of the wave must be active.
template <class Pos>
__device__ __forceinline__ void atss_select_cells(int k, int half, int Hs, int Ws, float sf, Pos pos, float yc,
                                                  float xc, int lane, unsigned long long& mine) {
  const int ry = (int)fminf(fmaxf(floorf(yc / sf), 0.f), (float)(Hs - 1));
  const int rx = (int)fminf(fmaxf(floorf(xc / sf), 0.f), (float)(Ws - 1));
  const int r0 = max(ry - half, 0), r1 = min(ry + half, Hs - 1);
  const int c0 = max(rx - half, 0), c1 = min(rx + half, Ws - 1);
  const unsigned long long kth = atss_select_rounds(k, r0, r1, c0, c1, Ws, pos, yc, xc, lane, mine);
  if (r0 > 0 || r1 < Hs - 1 || c0 > 0 || c1 < Ws - 1) {
    unsigned ao, aa, bo, ba;
    atss_axis_minima(Hs, r0, r1, pos, yc, lane, ao, aa);
    atss_axis_minima(Ws, c0, c1, pos, xc, lane, bo, ba);
    const unsigned m1 = ord_bits(__uint_as_float(ao) + __uint_as_float(ba));
    const unsigned m2 = ord_bits(__uint_as_float(aa) + __uint_as_float(bo));
    const unsigned outside = m1 < m2 ? m1 : m2;
    if (!(outside > (unsigned)(kth >> 32))) atss_select_rounds(k, 0, Hs - 1, 0, Ws - 1, Ws, pos, yc, xc, lane, mine);
  }
}
