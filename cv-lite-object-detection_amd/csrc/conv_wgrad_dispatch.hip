// The launch planner of the convolution weight gradients: which kernel family runs a call (or each
// group of it), with which tile, step, chunk and split count, and how many workspace bytes that
// takes.  Host code only -- nothing here touches a stream -- and the one place that reads this
// family's cvl_dispatch_* / cvl_tune_* keys (the measurement stamps / ablation bits of
// conv_wgrad_x.hip stay with the CVL_MEASURE code they arm).
//
// wgrad_plan() validates the descriptor, then walks the families in their order of preference:
//   SN (Npad 32: the per-level output heads; every source row read once, the taps on the dY side --
//       48 us per FCOS head on the generic kernels' 9x re-reads)
//   -> WH (3x3 stride 1, one segment, one group: the source staged once per 128-row step as a halo)
//   -> X covering all groups in one launch (up to kWgXMaxGroups: a tower layer's cls + reg pair).
// Failing those, each group runs on its own, one after another on the same workspace:
//   X -> L (128 x 256 / 256 x 256 LDS-DMA tiles) -> S (the register-staged 128-wide kernel).
// Each family has one predicate for what its kernel CAN run (wg_*_fits, next to the geometry it
// tests); the split models below carry the measurements they were fitted to.  The launchers
// (launch_wg_*) only instantiate what the plan says.
//
// wgrad_batch_plan() does the same for cvl_conv_wgrad_batch: WH launches of at most kWgHMaxProb 3x3
// problems, X launches of at most kWgXMaxProb 1x1 problems per tile width (256-wide first), the rest
// as calls of their own; the workspace holds each launch group's slabs in that order.
#include "conv_common.h"

namespace {

constexpr int SEGM = kWgSegM;
constexpr int X_BR = 32;                      // X: rows of one MFMA sub-step (conv_wgrad_x.hip BR)
constexpr int S_BR = 64, S_BKK = 128;         // S: reduction rows per step, k columns per tile (conv_wgrad.hip)
constexpr int L_BKK = 256;                    // L: k columns per tile (conv_wgrad_l.hip)
constexpr int H_BC = 64, H_RS = 128;          // WH: channel tile (ci and co), rows per step (conv_wgrad_h.hip)
constexpr int SN_BR = 64, SN_CI = 128;        // SN: source rows per step, input channels per workgroup

int device_cus() {
  static const int n = cvl_device_cus();
  return n;
}

int round_up(int v, int m) { return (v + m - 1) / m * m; }

// chunk (a multiple of SEGM, so no step straddles a segment) and split count of `want` splits over m rows
void set_chunks(WgLaunch* l, int m, int want) {
  l->chunk = round_up((m + want - 1) / want, SEGM);
  l->nsplit = (m + l->chunk - 1) / l->chunk;
}

// ---- SN ---------------------------------------------------------------------------------------------
// ~256 workgroups (one per CU: the 156-KiB LDS ring); a chunk is whole 64-row steps, at least four.
// Every chunk writes its partial dW to a slab [T][Cin][n_store rounded up to 4].
bool plan_sn(const cvl_conv_desc* d, int ngroups, WgLaunch* l) {
  if (cvl_tune_flag("CVL_WGRAD_NO_SN") || !wg_sn_fits(d, ngroups)) return false;
  long rows = 0;
  for (int i = 0; i < d->nseg; ++i) rows += (long)d->B * d->seg[i].Hr * d->seg[i].Wr;
  l->kernel = CVL_CK_WG_SN;
  l->tile = 32;
  l->tiles = d->Cin / SN_CI;
  static const int wgs = cvl_tune_int("CVL_SN_WGS", 256);
  const long want = wgs / l->tiles;
  long ch = (rows + want - 1) / want;
  ch = ((ch + SN_BR - 1) / SN_BR) * SN_BR;
  if (ch < 4 * SN_BR) ch = 4 * SN_BR;
  l->chunk = (int)ch;
  int c = 0;
  for (int i = 0; i < d->nseg; ++i) {
    l->cbase[i] = c;
    c += (int)(((long)d->B * d->seg[i].Hr * d->seg[i].Wr + ch - 1) / ch);
  }
  for (int i = d->nseg; i <= kMaxSeg; ++i) l->cbase[i] = c;
  l->nsplit = c;
  l->slab_bytes = (size_t)c * d->KH * d->KW * d->Cin * ((d->n_store + 3) & ~3) * sizeof(float);
  return true;
}

// ---- WH ---------------------------------------------------------------------------------------------
// one workgroup per CU (134 KiB of LDS): ~256 workgroups, >= 4 steps each
bool plan_h(const cvl_conv_desc* d, int ngroups, WgLaunch* l) {
  if (cvl_dispatch_flag("wg_no_h") || ngroups != 1 || !wg_h_fits(d)) return false;
  l->kernel = CVL_CK_WG_H;
  l->tile = H_BC;
  l->tiles = (d->Cin / H_BC) * (d->n_store / H_BC);
  l->steps = d->B * d->seg[0].Hr * d->seg[0].Wr / H_RS;
  l->reads = cvl_dispatch_int("wh_reads", 1) != 0;   // 0: the first form of the step loop (conv_wgrad_h.hip)
  int ns = (cvl_tune_int("CVL_WGH_WGS", 256) + l->tiles - 1) / l->tiles;
  if (ns > l->steps / 4) ns = l->steps / 4;
  if (ns < 1) ns = 1;
  l->chunk = (l->steps + ns - 1) / ns;
  l->nsplit = (l->steps + l->chunk - 1) / l->chunk;
  l->slab_bytes = l->nsplit > 1 ? (size_t)l->nsplit * 9 * d->Cin * d->n_store * sizeof(float) : 0;
  return true;
}

// ---- X ----------------------------------------------------------------------------------------------
// Modelled time of s splits at tile width T: rounds of 256 workgroups (one per CU; 512 for the 32-row
// 128-wide tile, 80 KiB of LDS) x 32-row steps per chunk (CVL_WGX_STEP, 0.01 us; ~0.8 us measured on
// the tower shape; CVL_WGX_STEP128 for the 128-wide tile: also ~0.8 us measured -- two per CU, the
// step is bound by its DMA / barrier overheads, not its MFMA work: the tower at 0.3 us picked 128
// and took 323 us vs 232) + the fp32 slab round trip.  The 128-wide tile serves the 1x1 /
// small-output launches (e.g. 1x1 256->1024 @ 32x32: 4 tiles of 256 -> 64 splits, 64 MiB of slabs;
// 16 tiles of 128 -> 16 splits, 16 MiB).  K below one 256-deep tile (1x1 convs with Cin 128) leaves
// half of every 256 tile idle.
bool plan_x(const cvl_conv_desc* d, int ngroups, const ConvArgs& a, WgLaunch* l) {
  if (cvl_dispatch_flag("wg_no_x") || !wg_x_fits(d, ngroups, a)) return false;
  const int spg = d->nseg / ngroups;
  int mg = 0;
  for (int gq = 0; gq < kWgXMaxGroups; ++gq) {
    l->g_m0[gq] = l->g_m1[gq] = 0;
    if (gq >= ngroups) continue;
    l->g_m0[gq] = a.seg[gq * spg].m_start;
    l->g_m1[gq] = (gq + 1) * spg < a.nseg ? a.seg[(gq + 1) * spg].m_start : a.m_total;
    mg = l->g_m1[gq] - l->g_m0[gq] > mg ? l->g_m1[gq] - l->g_m0[gq] : mg;
  }
  const int forced_t = cvl_tune_int("CVL_WGX_T", 0);
  const bool sr64 = cvl_tune_int("CVL_WGX_SR", 64) == 64;
  double best_t = 1e30, t128 = 1e30;
  int best_s = 0, best_T = 0, s256 = 0, tg256 = 0, s128 = 0;
  for (int T = 256; T >= 128; T /= 2) {
    if (forced_t && forced_t != T) continue;
    // T = 128 also takes 64-channel outputs (half of each tile idle: the stem's and the 1x1 ->64
    // weight gradients, on the generic kernel at 149 / 44 / 37 us before)
    if ((T == 256 && a.Npad % T) || a.K < cvl_tune_int(T == 256 ? "CVL_WGX_MIN_K" : "CVL_WGX_MIN_K128", T == 256 ? 256 : 64))
      continue;
    const int tg = ((a.Npad + T - 1) / T) * ((a.K + T - 1) / T) * ngroups;
    const double step_us =
        T == 256 ? cvl_tune_int("CVL_WGX_STEP", 80) / 100.0
                 : (sr64 ? cvl_tune_int("CVL_WGX_STEP64", 120) / 200.0 : cvl_tune_int("CVL_WGX_STEP128", 80) / 100.0);
    const double slab_us = (double)T * T * 4 * 2 / 5.0e6 * cvl_tune_int("CVL_WGX_SLAB_PCT", 100) / 100.0;
    int max_s = mg / 512;
    if (max_s < 1) max_s = 1;
    if (max_s > 2048 / tg) max_s = 2048 / tg > 1 ? 2048 / tg : 1;
    const int per_round = T == 256 || sr64 ? 256 : 512;
    for (int s = 1; s <= max_s; ++s) {
      const int rounds = (tg * s + per_round - 1) / per_round;
      const int chunk = ((mg + s - 1) / s + SEGM - 1) / SEGM * SEGM;
      const double t = rounds * (chunk / X_BR) * step_us + (s > 1 ? tg * s * slab_us : 0.0);
      if (t < best_t) { best_t = t; best_s = s; best_T = T; }
      if (T == 256 && best_T == 256) { s256 = best_s; tg256 = tg; }
      if (T == 128 && t < t128) { t128 = t; s128 = s; }
    }
  }
  // a 256-wide plan that cannot occupy every CU (tiles x splits < 256: the 1x1 / small-output
  // launches, capped by the 512-row minimum chunk) loses to the 128-wide one in the per-shape
  // sweep (1x1 256->1024 @ 32x32: 38 -> 31 us; 3x3 s2 2048->256 @ 8x8: 45 -> 34 us); the tower
  // (18 tiles x 14 splits) keeps 256 (230 vs 322 us)
  if (best_T == 256 && s128 && tg256 * s256 < 240 && !cvl_tune_flag("CVL_WGX_KEEP256")) {
    best_T = 128;
    best_s = s128;
  }
  if (!best_T) return false;
  l->kernel = CVL_CK_WG_X;
  l->tile = best_T;
  // 64-row steps on the 128-wide tile (CVL_WGX_SR=32 reverts): one workgroup per CU, half the
  // splits of the 32-row form at the same workgroup count per CU-round -- half the slab bytes (in-step
  // trace: the reductions 90 -> 63 / 133 -> 100 us per batch, the kernels +1-3 us; FCOS +0.6 %)
  l->rows = best_T == 128 && sr64 ? 64 : 32;
  l->pf = !cvl_dispatch_flag("wg_no_pf") && (best_T == 256 || l->rows == 64);   // (no 32-row 128-wide PF form)
  l->reads = cvl_dispatch_int("wgx_reads", 1) != 0;   // 0: the PF loop's first read placement (conv_wgrad_x.hip)
  l->co_tiles = (a.Npad + best_T - 1) / best_T;
  l->tiles = l->co_tiles * ((a.K + best_T - 1) / best_T);
  const int forced = cvl_tune_int("CVL_WGX_SPLITS", 0);
  set_chunks(l, mg, forced > 0 ? forced : best_s);
  l->slab_bytes = l->nsplit > 1 ? (size_t)ngroups * l->nsplit * a.K * d->n_store * sizeof(float) : 0;
  return true;
}

// ---- L ----------------------------------------------------------------------------------------------
// One workgroup per CU (134-150 KiB LDS).  Modelled time of (tile width, split count s): rounds of
// 256 workgroups x 64-row blocks per workgroup (measured on the FCOS P3 tower shape: ~2.8 us per
// block at the 128-wide co tile, ~4.4 us at the 256-wide one) + the fp32 slab round trip (write +
// read at ~5 TB/s); the cheapest plan wins.
double wl_time(int tiles, int m_total, int bco, int* best_s) {
  int max_s = m_total / 512;
  if (max_s < 1) max_s = 1;
  if (max_s > 4096 / tiles) max_s = 4096 / tiles > 1 ? 4096 / tiles : 1;
  // sweep knobs: slab cost in percent, block times in 0.1 us
  const double slab_us = (double)bco * L_BKK * 4 * 2 / 5.0e6 * cvl_tune_int("CVL_WGL_SLAB_PCT", 100) / 100.0;
  const double blk_us = bco == 256 ? cvl_tune_int("CVL_WGL_BLK256", 44) / 10.0 : cvl_tune_int("CVL_WGL_BLK128", 28) / 10.0;
  double best_t = 1e30;
  *best_s = 1;
  for (int s = 1; s <= max_s; ++s) {
    const int rounds = (tiles * s + 255) / 256;
    const int blocks = (m_total / s + 63) / 64;
    const double t = rounds * blocks * blk_us + (s > 1 ? tiles * s * slab_us : 0.0);
    if (t < best_t) { best_t = t; *best_s = s; }
  }
  return best_t;
}

// Npad 128 (one 128-wide co tile) runs faster on the register-staged 128 x 128 kernel (at bs 16:
// 3x3 128->128 @ 64x64 85 -> 72 us, 1x1 512->128 65 -> 46 us): CVL_WGL_MIN_NPAD
bool plan_l(const cvl_conv_desc* d, const ConvArgs& a, WgLaunch* l) {
  if (cvl_dispatch_flag("wg_no_l") || !wg_l_fits(d, a) || a.Npad < cvl_tune_int("CVL_WGL_MIN_NPAD", 256)) return false;
  const int kt = (a.K + L_BKK - 1) / L_BKK;
  int s128 = 1, s256 = 1;
  const double t128 = wl_time((a.Npad / 128) * kt, a.m_total, 128, &s128);
  double t256 = 1e30;
  if (a.Npad % 256 == 0 && !cvl_tune_flag("CVL_WGRAD_NO_256")) t256 = wl_time((a.Npad / 256) * kt, a.m_total, 256, &s256);
  l->tile = t256 < t128 ? 256 : 128;
  l->kernel = l->tile == 256 ? CVL_CK_WG_L256 : CVL_CK_WG_L128;
  l->co_tiles = a.Npad / l->tile;
  l->tiles = l->co_tiles * kt;
  set_chunks(l, a.m_total, l->tile == 256 ? s256 : s128);
  l->slab_bytes = l->nsplit > 1 ? (size_t)l->nsplit * a.K * d->n_store * sizeof(float) : 0;
  return true;
}

// ---- S ----------------------------------------------------------------------------------------------
// 2 workgroups per CU at this kernel's occupancy (512 slots); modelled time = rounds x steps per
// workgroup (~0.8 us per 64-row step) + the fp32 slab round trip; the cheapest split wins.  Rows
// per split at least 128 (one segment granule) lets small-M launches (CenterNet 16x16 maps at bs 8:
// 2048 rows) spread over more workgroups: CenterNet 488 -> 510 img/s vs 512.
void plan_s(const cvl_conv_desc* d, const ConvArgs& a, WgLaunch* l) {
  l->kernel = CVL_CK_WG_S;
  l->tile = a.Npad % 128 == 0 ? 128 : (a.Npad % 64 == 0 ? 64 : 32);
  // 128-row steps (twice the MFMA work per barrier pair and loads in flight); the chunks are
  // multiples of 128 rows, so a step never straddles a segment either way
  l->rows = cvl_tune_flag("CVL_WG_BR128") ? 128 : 64;
  l->co_tiles = a.Npad / l->tile;
  l->tiles = l->co_tiles * ((a.K + S_BKK - 1) / S_BKK);
  int max_s = a.m_total / cvl_tune_int("CVL_WG_MIN_CHUNK", 128);
  if (max_s < 1) max_s = 1;
  if (max_s > 8192 / l->tiles) max_s = 8192 / l->tiles > 1 ? 8192 / l->tiles : 1;
  const double slab_us = (double)l->tile * S_BKK * 4 * 2 / 5.0e6;
  int best = 1;
  double best_t = 1e30;
  for (int s = 1; s <= max_s; ++s) {
    const int rounds = (l->tiles * s + 511) / 512;
    const int steps = (a.m_total / s + S_BR - 1) / S_BR;
    const double t = rounds * steps * 0.8 * l->tile / 128.0 + (s > 1 ? l->tiles * s * slab_us : 0.0);
    if (t < best_t) { best_t = t; best = s; }
  }
  set_chunks(l, a.m_total, best);
  // sized for the split count asked for -- rounding the chunk to whole segments granules can leave fewer
  // splits -- which is what the size query has always reported for this kernel
  l->slab_bytes = best > 1 ? (size_t)best * a.K * d->n_store * sizeof(float) : 0;
}

// what cvl_conv_wgrad_grouped checks of its descriptor (the pointers apart)
int check_wgrad_desc(const cvl_conv_desc* d, int ngroups, ConvArgs* pa) {
  ConvArgs& a = *pa;
  const int st = cvl_conv_prepare(d, SEGM, &a);
  if (st) return st;
  CVL_CHECK_ARG(d->prec == CVL_PREC_BF16 && d->mode == CVL_CONV_FWD);
  CVL_CHECK_ARG(ngroups >= 1 && d->nseg % ngroups == 0);
  CVL_CHECK_ARG(d->Cin % 8 == 0 && a.Npad % 32 == 0);
  CVL_CHECK_ARG(d->ld_dst % 8 == 0 && d->dst_coff % 8 == 0 && d->ld_dst >= d->dst_coff + a.Npad);
  const int spg = d->nseg / ngroups;
  for (int i = 0; i < d->nseg; ++i) CVL_CHECK_ARG(d->seg[i].w == d->seg[i / spg * spg].w);   // a group shares its weights
  return CVL_OK;
}

}  // namespace

int wgrad_plan(const cvl_conv_desc* d, int ngroups, WgradPlan* p) {
  ConvArgs a;
  const int st = check_wgrad_desc(d, ngroups, &a);
  if (st) return st;
  p->nlaunch = 1;
  p->workspace_bytes = 16;
  WgLaunch& all = p->l[0];
  all = WgLaunch{};
  all.nseg = d->nseg;
  all.ngroups = ngroups;
  if (plan_sn(d, ngroups, &all) || plan_h(d, ngroups, &all) || plan_x(d, ngroups, a, &all)) {
    if (all.slab_bytes > p->workspace_bytes) p->workspace_bytes = all.slab_bytes;
    return CVL_OK;
  }
  p->nlaunch = ngroups;
  for (int gq = 0; gq < ngroups; ++gq) {
    WgLaunch& l = p->l[gq];
    l = WgLaunch{};
    l.nseg = d->nseg / ngroups;
    l.seg0 = gq * l.nseg;
    l.ngroups = 1;
    const cvl_conv_desc gd = wgrad_launch_desc(d, l);
    cvl_conv_prepare(&gd, SEGM, &a);
    if (!plan_l(&gd, a, &l)) plan_s(&gd, a, &l);
    if (l.slab_bytes > p->workspace_bytes) p->workspace_bytes = l.slab_bytes;
    // With one group X has just declined these very arguments.  Of several groups (more than
    // kWgXMaxGroups) X takes each it can, but the size the call has always reported is the one of L / S
    // above.  X's slabs are the smaller ones wherever a model uses this; where they are not (e.g. 3
    // groups of 3x3 stride 2 256 -> 2048 at 32x32 and 16x16, B 16: 75 MB against L's 57 MB) the entry
    // rejects the workspace, as it always has.  Goes away when one X launch covers any number of groups.
    if (ngroups > 1) plan_x(&gd, 1, a, &l);
  }
  return CVL_OK;
}

// ---- cvl_conv_wgrad_batch -----------------------------------------------------------------------------
namespace {

// Common chunk of one batched launch, by the cost model of plan_x: rounds of one workgroup per CU x
// (fixed cost + steps) + the fp32 slab round trip of split problems, over chunks c0, 2 c0, ... up to
// the largest problem.  units[i]: problem i's rows (X) or 128-row steps (WH); a step is `per` units.
int batch_chunk(const int* tiles, const int* units, int n, int c0, double fix, int per, double step, double slab_us) {
  int maxu = 1;
  for (int i = 0; i < n; ++i) maxu = units[i] > maxu ? units[i] : maxu;
  const int ncu = device_cus();
  int best_c = maxu;
  double best_t = 1e30;
  for (int c = c0;; c *= 2) {
    const int cc = c < maxu ? c : maxu;
    long w = 0, sl = 0;
    for (int i = 0; i < n; ++i) {
      const int sp = (units[i] + cc - 1) / cc;
      w += (long)tiles[i] * sp;
      if (sp > 1) sl += (long)tiles[i] * sp;
    }
    const double t = (double)((w + ncu - 1) / ncu) * (fix + (cc / per) * step) + sl * slab_us;
    if (t < best_t) {
      best_t = t;
      best_c = cc;
    }
    if (cc >= maxu) break;
  }
  return best_c;
}

// tile width of a batched 1x1 problem: 256 (the tower kernel's tile, ~2x its MFMA rate per CU) when
// both GEMM sides fill it (Npad % 256 == 0, Cin >= 256: the conv4_x / conv5_x 1x1 convs and the
// 256 -> 512 projections), else 128; one launch per tile width
int batch_tile(const cvl_conv_desc* d) {
  return (d->Npad % 256 == 0 && d->Cin >= 256 && !cvl_dispatch_flag("wgb_no_256")) ? 256 : 128;
}

// One launch group over problems b->idx[0..n): chunk, splits and slab offsets.  X, measured (1x1
// 1024->256 @ 32x32 at 16 / 8 / 4 / 2 / 1 splits: 20.6 / 29.5 / 48.2 / 89.1 / 171 us): ~7.2 us per
// workgroup round + ~0.64 us per 64-row step of the 128-wide tile; 256-wide ~0.54 us per 32-row
// step (the tower's weight gradient: 390 steps in ~210 us).  WH: CVL_WGHB_FIX / _STEP, us x 100.
void plan_batch_group(const cvl_conv_desc* const* d, WgBatchLaunch* b) {
  const bool wh = b->kernel == CVL_CK_WG_H;
  const int T = b->tile;
  int tiles[kWgXMaxProb], units[kWgXMaxProb];
  for (int i = 0; i < b->n; ++i) {
    const cvl_conv_desc* q = d[b->idx[i]];
    const int rows = q->B * q->seg[0].Hr * q->seg[0].Wr;
    tiles[i] = wh ? (q->Cin / H_BC) * (q->n_store / H_BC) : ((q->Npad + T - 1) / T) * ((q->Cin + T - 1) / T);
    units[i] = wh ? rows / H_RS : round_up(rows, SEGM);
  }
  if (wh) {
    b->chunk = batch_chunk(tiles, units, b->n, 1, cvl_tune_int("CVL_WGHB_FIX", 800) / 100.0, 1,
                           cvl_tune_int("CVL_WGHB_STEP", 300) / 100.0, (double)9 * H_BC * H_BC * 4 * 2 / 5.0e6);
    const int forced = cvl_tune_int("CVL_WGHB_CHUNK", 0);
    if (forced > 0) b->chunk = forced;
  } else {
    const double step = T == 256 ? cvl_tune_int("CVL_WGB_STEP256", 54) / 100.0 : cvl_tune_int("CVL_WGB_STEP", 64) / 100.0;
    b->chunk = batch_chunk(tiles, units, b->n, SEGM, cvl_tune_int("CVL_WGB_FIX", 720) / 100.0,
                           T == 256 ? X_BR : 64, step, (double)T * T * 4 * 2 / 5.0e6);
    const int forced = cvl_tune_int("CVL_WGB_CHUNK", 0);   // measurement: rows per workgroup
    if (forced > 0) b->chunk = round_up(forced, SEGM);
  }
  b->ws_bytes = 0;
  for (int i = 0; i < b->n; ++i) {
    const cvl_conv_desc* q = d[b->idx[i]];
    const int c = wh && b->chunk > units[i] ? units[i] : b->chunk;
    b->nsplit[i] = (units[i] + c - 1) / c;
    b->slab_off[i] = b->ws_bytes;
    if (b->nsplit[i] > 1)
      b->ws_bytes += ((size_t)b->nsplit[i] * q->KH * q->KW * q->Cin * q->n_store * sizeof(float) + 255) & ~(size_t)255;
  }
}

}  // namespace

int wgrad_batch_plan(const cvl_conv_desc* const* d, int n, WgradBatchPlan* p) {
  CVL_CHECK_ARG(d && n >= 1);
  // 0: a call of its own, 3: WH, 128 / 256: X at that tile width
  std::vector<int> cls(n);
  const bool no_h = cvl_dispatch_flag("wgb_no_h") || cvl_dispatch_flag("wg_no_h");
  ConvArgs a;
  for (int i = 0; i < n; ++i) {
    CVL_CHECK_ARG(d[i]);
    cls[i] = wg_x_batch_fits(d[i], &a) ? batch_tile(d[i]) : (!no_h && wg_h_fits(d[i])) ? 3 : 0;
  }
  p->l.clear();
  size_t used = 0;
  for (int c : {3, 256, 128}) {
    const int cap = c == 3 ? kWgHMaxProb : kWgXMaxProb;
    WgBatchLaunch b{};
    auto close = [&]() {
      plan_batch_group(d, &b);
      b.ws_off = used;
      used += b.ws_bytes;
      p->l.push_back(b);
      b.n = 0;
    };
    b.kernel = c == 3 ? CVL_CK_WG_H : CVL_CK_WG_X;
    b.tile = c == 3 ? H_BC : c;
    b.reads = cvl_dispatch_int(c == 3 ? "wh_reads" : "wgx_reads", 1) != 0;
    for (int i = 0; i < n; ++i) {
      if (cls[i] != c) continue;
      b.idx[b.n++] = i;
      if (b.n == cap) close();
    }
    if (b.n) close();
  }
  for (int i = 0; i < n; ++i) {
    if (cls[i]) continue;
    WgBatchLaunch b{};
    b.kernel = CVL_CK_NONE;
    b.n = 1;
    b.idx[0] = i;
    b.single.nlaunch = 0;
    if (d[i]->prec == CVL_PREC_F32) {
      b.single.workspace_bytes = cvl_conv_wgrad_f32_workspace(d[i], 1);
    } else {
      const int st = wgrad_plan(d[i], 1, &b.single);
      if (st) return st;
    }
    b.ws_off = used;
    b.ws_bytes = (b.single.workspace_bytes + 255) & ~(size_t)255;
    used += b.ws_bytes;
    p->l.push_back(b);
  }
  p->workspace_bytes = used > 16 ? used : 16;
  return CVL_OK;
}

// Test and profiling hooks: what a weight-gradient call would launch.  Host only: no device memory, no
// launch.  The last launch of the plan is described, as cvl_conv_igemm_last_kernel shows it after the call.
extern "C" int cvl_conv_wgrad_plan(const cvl_conv_desc* d, int ngroups, int32_t* kernel, int32_t* tile, int32_t* nsplit,
                                   size_t* workspace) {
  CVL_CHECK_ARG(d && kernel && tile && nsplit && workspace);
  *kernel = CVL_CK_NONE;
  *tile = *nsplit = 0;
  *workspace = 0;
  if (d->prec == CVL_PREC_F32) return CVL_OK;      // parity mode: its own kernels
  WgradPlan p;
  const int st = wgrad_plan(d, ngroups, &p);
  if (st) return st;
  const WgLaunch& l = p.l[p.nlaunch - 1];
  *kernel = l.kernel;
  *tile = l.tile;
  *nsplit = l.nsplit;
  *workspace = p.workspace_bytes;
  return CVL_OK;
}

// ... and per problem of a cvl_conv_wgrad_batch call: its kernel, the index of the launch group that
// runs it (in launch order) and its split count
extern "C" int cvl_conv_wgrad_batch_plan(const cvl_conv_desc* const* d, int n, int32_t* kernel_of, int32_t* launch_of,
                                         int32_t* nsplit_of) {
  CVL_CHECK_ARG(kernel_of && launch_of && nsplit_of);
  WgradBatchPlan p;
  const int st = wgrad_batch_plan(d, n, &p);
  if (st) return st;
  for (size_t g = 0; g < p.l.size(); ++g) {
    const WgBatchLaunch& b = p.l[g];
    const WgLaunch* one = b.kernel == CVL_CK_NONE && b.single.nlaunch ? &b.single.l[b.single.nlaunch - 1] : nullptr;
    for (int i = 0; i < b.n; ++i) {
      kernel_of[b.idx[i]] = one ? one->kernel : b.kernel;
      launch_of[b.idx[i]] = (int32_t)g;
      nsplit_of[b.idx[i]] = one ? one->nsplit : b.kernel == CVL_CK_NONE ? 0 : b.nsplit[i];
    }
  }
  return CVL_OK;
}
