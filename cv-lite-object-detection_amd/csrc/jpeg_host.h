// Host half of the batched JPEG decoder (include/cvlite.h "JPEG decode"): the marker parser and the
// baseline Huffman decoder.  Plain C++17, no HIP: jpeg_decode.hip includes it for the C entry
// points and tools/jpeg_host_check.cpp builds it alone under the host sanitizers.
//
// The bytes come from files, so every length, table id, code count and coefficient index is
// bounded before it is used, and the bit reader never reads past `end`.  Anything the GPU half
// could not reproduce bit for bit against libjpeg (a stream libjpeg would only warn about and
// patch up) is reported as corrupt, so the caller falls back to the host decoder.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/cvlite.h"

namespace cvl_jpeg {

constexpr int MAX_DIM = 8192;
// largest |coef * qt| accepted.  The DCT is orthonormal, so 8-bit samples give |F| <= 8 * 128 = 1024
// and a dequantised value within qt / 2 of it, at most 1151; a damaged stream can hold far more, and
// there libjpeg builds differ among themselves (the C IDCT wraps its range table, the SIMD ones
// saturate 16-bit intermediates), so such a stream is refused rather than decoded some third way.
constexpr int MAX_DEQUANT = 4095;

static const uint8_t NATURAL[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,
                                    12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
                                    58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct HuffSpec {                 // a DHT table as stored in the file
  uint8_t present;
  uint8_t bits[17];               // bits[l] = number of codes of length l (1..16)
  uint8_t vals[256];
  int nvals;
};

struct Header {
  int width, height, ncomp;
  int hs[3], vs[3], tq[3], td[3], ta[3], id[3];
  int hmax, vmax, restart;
  int mcux, mcuy;                 // MCUs across / down
  int bw[3], bh[3];               // blocks per component, padded to whole MCUs
  int blk_start[4];               // first block of component c in the planar layout; [ncomp] = total
  uint8_t qt_present[4];
  uint16_t qt[4][64];             // natural order
  HuffSpec dc[4], ac[4];
  size_t scan_pos;                // first byte of entropy-coded data
  size_t coef_count() const { return (size_t)blk_start[ncomp] * 64; }
};

static inline int rd16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

// Parses every segment up to and including SOS.  CVL_OK: `h` is complete and the file is in the
// supported set; CVL_JPEG_UNSUPPORTED: a well-formed file outside it (or not a JPEG at all);
// CVL_JPEG_CORRUPT: a JPEG whose segments are truncated or inconsistent.
static inline int parse_header(const uint8_t* d, size_t n, Header* h) {
  memset(h, 0, sizeof(*h));
  if (!d || n < 4 || d[0] != 0xFF || d[1] != 0xD8) return CVL_JPEG_UNSUPPORTED;
  size_t p = 2;
  bool sof = false, jfif = false, adobe = false;
  int adobe_tf = 0;
  for (;;) {
    if (p >= n || d[p] != 0xFF) return CVL_JPEG_CORRUPT;
    while (p < n && d[p] == 0xFF) ++p;                       // marker prefix and fill bytes
    if (p >= n) return CVL_JPEG_CORRUPT;
    const int m = d[p++];
    if (m == 0xD9 || m == 0xD8 || m == 0x00 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) return CVL_JPEG_CORRUPT;
    if (p + 2 > n) return CVL_JPEG_CORRUPT;
    const size_t len = (size_t)rd16(d + p);
    if (len < 2 || p + len > n) return CVL_JPEG_CORRUPT;
    const uint8_t* s = d + p + 2;                            // payload, plen bytes
    const size_t plen = len - 2;
    p += len;
    if (m == 0xC0) {
      if (sof) return CVL_JPEG_CORRUPT;
      if (plen < 6) return CVL_JPEG_CORRUPT;
      const int prec = s[0], nf = s[5];
      if (plen != (size_t)6 + 3 * (size_t)nf) return CVL_JPEG_CORRUPT;
      if (prec != 8 || (nf != 1 && nf != 3)) return CVL_JPEG_UNSUPPORTED;
      h->height = rd16(s + 1);
      h->width = rd16(s + 3);
      if (h->width < 1 || h->height < 1 || h->width > MAX_DIM || h->height > MAX_DIM) return CVL_JPEG_UNSUPPORTED;
      h->ncomp = nf;
      for (int c = 0; c < nf; ++c) {
        h->id[c] = s[6 + 3 * c];
        h->hs[c] = s[7 + 3 * c] >> 4;
        h->vs[c] = s[7 + 3 * c] & 15;
        h->tq[c] = s[8 + 3 * c];
        if (h->hs[c] < 1 || h->hs[c] > 4 || h->vs[c] < 1 || h->vs[c] > 4 || h->tq[c] > 3) return CVL_JPEG_CORRUPT;
      }
      sof = true;
    } else if (m == 0xC4) {
      size_t q = 0;
      while (q < plen) {
        if (q + 17 > plen) return CVL_JPEG_CORRUPT;
        const int tc = s[q] >> 4, th = s[q] & 15;
        if (tc > 1 || th > 3) return CVL_JPEG_CORRUPT;
        HuffSpec* t = tc ? &h->ac[th] : &h->dc[th];
        int cnt = 0;
        t->bits[0] = 0;
        for (int l = 1; l <= 16; ++l) {
          t->bits[l] = s[q + l];
          cnt += s[q + l];
        }
        q += 17;
        if (cnt > 256 || q + (size_t)cnt > plen) return CVL_JPEG_CORRUPT;
        memcpy(t->vals, s + q, (size_t)cnt);
        t->nvals = cnt;
        t->present = 1;
        q += (size_t)cnt;
      }
    } else if (m == 0xDB) {
      size_t q = 0;
      while (q < plen) {
        const int pq = s[q] >> 4, tq = s[q] & 15;
        if (pq > 1 || tq > 3) return CVL_JPEG_CORRUPT;
        if (pq == 1) return CVL_JPEG_UNSUPPORTED;            // 16-bit quantisation table
        if (q + 65 > plen) return CVL_JPEG_CORRUPT;
        for (int i = 0; i < 64; ++i) h->qt[tq][NATURAL[i]] = s[q + 1 + i];
        h->qt_present[tq] = 1;
        q += 65;
      }
    } else if (m == 0xDD) {
      if (plen != 2) return CVL_JPEG_CORRUPT;
      h->restart = rd16(s);
    } else if (m == 0xE0) {
      if (plen >= 5 && memcmp(s, "JFIF", 5) == 0) jfif = true;
    } else if (m == 0xEE) {
      if (plen >= 12 && memcmp(s, "Adobe", 5) == 0) {
        adobe = true;
        adobe_tf = s[11];
      }
    } else if ((m >= 0xE1 && m <= 0xEF) || m == 0xFE) {
      // APPn / COM: skipped
    } else if (m == 0xDA) {
      if (!sof || plen < 1) return CVL_JPEG_CORRUPT;
      const int ns = s[0];
      if (ns < 1 || ns > 4 || plen != (size_t)4 + 2 * (size_t)ns) return CVL_JPEG_CORRUPT;
      if (ns != h->ncomp) return CVL_JPEG_UNSUPPORTED;       // one scan of several
      for (int c = 0; c < ns; ++c) {
        if (s[1 + 2 * c] != h->id[c]) return CVL_JPEG_UNSUPPORTED;
        h->td[c] = s[2 + 2 * c] >> 4;
        h->ta[c] = s[2 + 2 * c] & 15;
        if (h->td[c] > 3 || h->ta[c] > 3) return CVL_JPEG_CORRUPT;
      }
      const uint8_t* e = s + 1 + 2 * ns;
      if (e[0] != 0 || e[1] != 63 || e[2] != 0) return CVL_JPEG_UNSUPPORTED;
      h->scan_pos = p;
      break;
    } else {
      return CVL_JPEG_UNSUPPORTED;                           // other SOFn, DAC, DNL, JPGn, ...
    }
  }
  if (h->ncomp == 3) {
    // libjpeg's colour-space rule: JFIF means YCbCr; else the Adobe transform byte; else the ids
    if (!jfif) {
      if (adobe) {
        if (adobe_tf != 1) return CVL_JPEG_UNSUPPORTED;
      } else if (h->id[0] == 'R' && h->id[1] == 'G' && h->id[2] == 'B') {
        return CVL_JPEG_UNSUPPORTED;
      }
    }
    if (h->hs[1] != 1 || h->vs[1] != 1 || h->hs[2] != 1 || h->vs[2] != 1) return CVL_JPEG_UNSUPPORTED;
    const int hv = h->hs[0] * 10 + h->vs[0];
    if (hv != 11 && hv != 21 && hv != 22) return CVL_JPEG_UNSUPPORTED;
  } else {
    h->hs[0] = h->vs[0] = 1;                                 // a one-component scan is not interleaved
  }
  h->hmax = h->hs[0];
  h->vmax = h->vs[0];
  h->mcux = (h->width + 8 * h->hmax - 1) / (8 * h->hmax);
  h->mcuy = (h->height + 8 * h->vmax - 1) / (8 * h->vmax);
  int start = 0;
  for (int c = 0; c < h->ncomp; ++c) {
    if (!h->qt_present[h->tq[c]] || !h->dc[h->td[c]].present || !h->ac[h->ta[c]].present) return CVL_JPEG_CORRUPT;
    h->bw[c] = h->mcux * h->hs[c];
    h->bh[c] = h->mcuy * h->vs[c];
    h->blk_start[c] = start;
    start += h->bw[c] * h->bh[c];
  }
  for (int c = h->ncomp; c < 4; ++c) h->blk_start[c] = start;
  return CVL_OK;
}

// ---- Huffman decode ------------------------------------------------------------------------------
constexpr int LOOK = 9;

struct HuffTable {
  uint16_t look[1 << LOOK];       // (length << 8) | symbol for codes of <= LOOK bits, 0 otherwise
  int32_t maxcode[18];            // largest code of length l, -1 if none; [17] ends every search
  int32_t valoff[17];             // index of the first symbol of length l minus its first code
  const uint8_t* vals;
  int nvals;
};

static inline bool build_table(const HuffSpec& s, HuffTable* t) {
  memset(t->look, 0, sizeof(t->look));
  t->vals = s.vals;
  t->nvals = s.nvals;
  int code = 0, k = 0;
  for (int l = 1; l <= 16; ++l) {
    const int cnt = s.bits[l];
    t->valoff[l] = k - code;
    if (cnt) {
      if (code + cnt > (1 << l)) return false;               // over-subscribed code space
      for (int i = 0; i < cnt; ++i, ++k, ++code) {
        if (l <= LOOK) {
          const int base = code << (LOOK - l);
          for (int j = 0; j < (1 << (LOOK - l)); ++j) t->look[base + j] = (uint16_t)((l << 8) | s.vals[k]);
        }
      }
      t->maxcode[l] = code - 1;
    } else {
      t->maxcode[l] = -1;
    }
    code <<= 1;
  }
  t->maxcode[17] = 0x7fffffff;
  return true;
}

// MSB-first bit reader over the entropy-coded segment.  fill() removes stuffed zero bytes and stops
// at a marker or at `end`; from there it supplies zero bits and counts them in `pad`, and a caller
// that finds bits < pad has consumed bits that were not in the file.
struct BitReader {
  const uint8_t* p;
  const uint8_t* end;
  uint64_t acc;
  int bits, pad;
  void reset() { acc = 0; bits = 0; pad = 0; }
  inline void fill() {
    while (bits <= 56) {
      uint32_t b = 0;
      if (pad == 0 && p < end) {
        b = *p;
        if (b != 0xFF) {
          ++p;
        } else if (p + 1 < end && p[1] == 0) {
          p += 2;
        } else {
          b = 0;
          pad = 8;
        }
      } else {
        pad += 8;
      }
      acc = (acc << 8) | b;
      bits += 8;
    }
  }
  inline uint32_t peek(int nb) const { return (uint32_t)(acc >> (bits - nb)) & ((1u << nb) - 1); }
  inline void skip(int nb) { bits -= nb; }
  inline bool overrun() const { return bits < pad; }
};

// One Huffman symbol; -1 for a code that is in no table.  Needs >= 16 bits in the reader.
static inline int decode_symbol(BitReader& br, const HuffTable& t) {
  const uint32_t e = t.look[br.peek(LOOK)];
  if (e) {
    br.skip((int)(e >> 8));
    return (int)(e & 255);
  }
  const int32_t v16 = (int32_t)br.peek(16);
  int l = LOOK + 1;
  while (l <= 16 && (v16 >> (16 - l)) > t.maxcode[l]) ++l;
  if (l > 16) return -1;
  const int idx = (v16 >> (16 - l)) + t.valoff[l];
  if (idx < 0 || idx >= t.nvals) return -1;
  br.skip(l);
  return t.vals[idx];
}

static inline int extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

// Entropy-decodes the scan of a parsed file into coef [comp][block_row][block_col][64] (int16, not
// dequantised, natural order, h.coef_count() elements) and qt [3][64] (per component, natural order;
// unused components zero).  CVL_OK or CVL_JPEG_CORRUPT; on failure coef / qt hold partial data.
static inline int entropy_decode(const uint8_t* d, size_t n, const Header& h, int16_t* coef, uint16_t* qt) {
  HuffTable dct[3], act[3];
  for (int c = 0; c < 3; ++c) {
    if (c < h.ncomp) {
      if (!build_table(h.dc[h.td[c]], &dct[c]) || !build_table(h.ac[h.ta[c]], &act[c])) return CVL_JPEG_CORRUPT;
      memcpy(qt + 64 * c, h.qt[h.tq[c]], 128);
    } else {
      memset(qt + 64 * c, 0, 128);
    }
  }
  BitReader br;
  br.p = d + h.scan_pos;
  br.end = d + n;
  br.reset();
  int pred[3] = {0, 0, 0};
  int todo = h.restart, rst = 0;
  const int nmcu = h.mcux * h.mcuy;
  for (int mcu = 0; mcu < nmcu; ++mcu) {
    const int my = mcu / h.mcux, mx = mcu - my * h.mcux;
    for (int c = 0; c < h.ncomp; ++c) {
      const uint16_t* q = h.qt[h.tq[c]];
      for (int by = 0; by < h.vs[c]; ++by) {
        for (int bx = 0; bx < h.hs[c]; ++bx) {
          int16_t* blk = coef + ((size_t)h.blk_start[c] + (size_t)(my * h.vs[c] + by) * h.bw[c] + (mx * h.hs[c] + bx)) * 64;
          memset(blk, 0, 128);
          br.fill();
          int s = decode_symbol(br, dct[c]);
          if (s < 0 || s > 11) return CVL_JPEG_CORRUPT;
          if (s) {
            const int v = (int)br.peek(s);
            br.skip(s);
            pred[c] += extend(v, s);
          }
          if (pred[c] > 2047 || pred[c] < -2048) return CVL_JPEG_CORRUPT;
          if (pred[c] * (int)q[0] > MAX_DEQUANT || pred[c] * (int)q[0] < -MAX_DEQUANT) return CVL_JPEG_CORRUPT;
          blk[0] = (int16_t)pred[c];
          for (int k = 1; k < 64;) {
            br.fill();
            const int rs = decode_symbol(br, act[c]);
            if (rs < 0) return CVL_JPEG_CORRUPT;
            const int r = rs >> 4;
            s = rs & 15;
            if (s == 0) {
              if (r != 15) break;                            // EOB
              k += 16;                                       // ZRL
              continue;
            }
            k += r;
            if (k > 63 || s > 10) return CVL_JPEG_CORRUPT;
            const int v = extend((int)br.peek(s), s);
            br.skip(s);
            const int nat = NATURAL[k];
            if (v * (int)q[nat] > MAX_DEQUANT || v * (int)q[nat] < -MAX_DEQUANT) return CVL_JPEG_CORRUPT;
            blk[nat] = (int16_t)v;
            ++k;
          }
        }
      }
    }
    if (br.overrun()) return CVL_JPEG_CORRUPT;
    if (h.restart && --todo == 0 && mcu + 1 < nmcu) {
      // the interval ends: only padding bits may remain, then RSTn
      if (br.bits - br.pad >= 8) return CVL_JPEG_CORRUPT;
      const uint8_t* p = br.p;
      if (p >= br.end || *p != 0xFF) return CVL_JPEG_CORRUPT;
      while (p < br.end && *p == 0xFF) ++p;
      if (p >= br.end || *p != 0xD0 + rst) return CVL_JPEG_CORRUPT;
      br.p = p + 1;
      br.reset();
      rst = (rst + 1) & 7;
      todo = h.restart;
      pred[0] = pred[1] = pred[2] = 0;
    }
  }
  // the scan must be followed by EOI
  if (br.bits - br.pad >= 8) return CVL_JPEG_CORRUPT;
  const uint8_t* p = br.p;
  if (p >= br.end || *p != 0xFF) return CVL_JPEG_CORRUPT;
  while (p < br.end && *p == 0xFF) ++p;
  if (p >= br.end || *p != 0xD9) return CVL_JPEG_CORRUPT;
  return CVL_OK;
}

// The two host-only entry points of the C ABI (include/cvlite.h), shared by the library and the
// stand-alone check program.
static inline int info(const uint8_t* d, size_t n, int32_t* out) {
  if (!out) return CVL_EINVAL;
  Header h;
  const int st = d ? parse_header(d, n, &h) : CVL_JPEG_UNSUPPORTED;
  memset(out, 0, 8 * sizeof(int32_t));
  out[0] = st;
  if (st == CVL_OK) {
    out[1] = h.width;
    out[2] = h.height;
    out[3] = h.ncomp;
    out[4] = h.hmax;
    out[5] = h.vmax;
    out[6] = h.restart;
    out[7] = (int32_t)h.coef_count();
  }
  return st;
}

static inline int decode_coefficients(const uint8_t* d, size_t n, int16_t* coef, size_t coef_cap, uint16_t* qt) {
  if (!coef || !qt) return CVL_EINVAL;
  Header h;
  const int st = d ? parse_header(d, n, &h) : CVL_JPEG_UNSUPPORTED;
  if (st != CVL_OK) return st;
  if (coef_cap < h.coef_count()) return CVL_EINVAL;
  return entropy_decode(d, n, h, coef, qt);
}

}  // namespace cvl_jpeg
