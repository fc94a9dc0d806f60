// The launch planner of the forward / data-gradient convolutions: which kernel family runs a call,
// in which variant, on which grid, with which workspace.  Host code only -- nothing here touches a
// stream -- and the one place that reads this family's cvl_dispatch_* / cvl_tune_* keys.
//
// conv_plan() first rewrites a strided data gradient (s2dgrad_transform, s2dgrad3_*), validates the
// descriptor, then walks the families in their order of preference:
//   H64 32-wide (the FCOS heads' forward)  ->  P (1x1)  ->  X32 on 32-channel sources  ->  H64  ->
//   X32  ->  L256 / L128 / L64  ->  the 128-row kernel (with split-K on small grids).
// Each family has one predicate that says whether the kernel CAN run the launch (geometry,
// alignment, bounds: p_fits, x32_fits, cvl_conv_h_fits, large_fits); the measured crossovers sit in the
// sequence itself, next to the measurements they came from.  The launchers (launch_base / _l / _x /
// _h / _p) only instantiate what the plan says.
#include "conv_common.h"

namespace {

constexpr int BM_BASE = 128, NT_BASE = 256;   // the 128-row kernel's tile rows / threads (conv_igemm.hip)
constexpr int BM = 256;                       // tile rows of L / X32 / H64 / P
constexpr int H_BN = 64, H_BK = 32;           // H64's default N tile and channel block

// compute units of the device.  Cached at the first call (as the launchers always did): a process that
// switched devices afterwards would keep the first device's count.
int device_cus() {
  static const int n = cvl_device_cus();
  return n;
}

int pick_bn(int npad) { return npad % 128 == 0 ? 128 : (npad % 64 == 0 ? 64 : 32); }

// split-K factor of the 128-row kernel: only for grids that cannot fill the chip (small M, e.g.
// conv5 / c6 at 16x16).  Sized with 64-deep K steps (32 when Cin % 64) even where the launch then
// runs 128-deep ones; conv_plan_set_splits normalises it to the launch's own K steps.
int base_split_want(const ConvArgs& a) {
  if (a.nseg != 1) return 1;
  const int BN_ = pick_bn(a.Npad), BK_ = a.Cin % 64 == 0 ? 64 : 32;
  const int tiles = a.m_tiles * (a.Npad / BN_);
  const int nk = a.K / BK_;
  const int max_tiles = cvl_tune_int("CVL_KSPLIT_MAX_TILES", 192);
  const int target = cvl_tune_int("CVL_KSPLIT_TARGET", 384);   // workgroups a split launch aims for
  // short-K small launches split too (>= 4 K steps, >= 2 per split): the hourglass's 16x16 / 32x32
  // levels at bs 8, CenterNet 546 -> 554 img/s (8 / 4: the previous rule; 2 / 1 and a 768 target: less)
  const int min_nk = cvl_dispatch_int("ksplit_min_nk", 4);     // K steps a split needs at least
  if (tiles >= max_tiles || nk < min_nk) return 1;
  int s = (target + tiles - 1) / tiles;
  const int per = cvl_tune_int("CVL_KSPLIT_MIN_PER", 2);       // K steps per split at least
  if (s > nk / per) s = nk / per;
  return s < 1 ? 1 : s;
}

// split factor H64 wants for a grid that leaves CUs idle (1: none); a: the 256-row layout
int h_split_want(const ConvArgs& a) {
  const int tiles = a.m_tiles * (a.Npad / H_BN);
  const int target = cvl_tune_int("CVL_CONV_H_SPLIT_TARGET", 256);
  if (tiles >= target) return 1;
  int splits = (target + tiles - 1) / tiles;
  if (splits > (a.Cin / H_BK) / 2) splits = (a.Cin / H_BK) / 2;
  return splits < 1 ? 1 : splits;
}

size_t slab_bytes(const ConvArgs& a, int splits) { return (size_t)splits * a.m_total * a.Npad * sizeof(float); }

// 1x1 strided data-gradient: only every stride-th dX pixel receives a gradient, so instead of a
// DGRAD gather that finds no valid tap for (s^2-1)/s^2 of the rows, run a dense 1x1 GEMM over the
// dY pixels whose epilogue writes row (y, x) to dX pixel (y*s, x*s); the other pixels are zeroed
// (beta == 0) or keep their accumulated value (beta != 0: they receive + 0).
bool s2dgrad_transform(const cvl_conv_desc* d, cvl_conv_desc* out, int* up, int* upw) {
  if (d->mode != CVL_CONV_DGRAD || d->KH != 1 || d->KW != 1 || d->stride < 2 || d->nseg != 1 ||
      d->pad_t != 0 || d->pad_l != 0 || d->relu_in || cvl_tune_flag("CVL_CONV_NO_S2DG"))
    return false;
  const cvl_conv_seg& q = d->seg[0];
  if ((q.Hs - 1) * d->stride >= q.Hr || (q.Ws - 1) * d->stride >= q.Wr) return false;
  *out = *d;
  out->mode = CVL_CONV_FWD;
  out->stride = 1;
  out->seg[0].Hr = q.Hs;
  out->seg[0].Wr = q.Ws;
  *up = d->stride;
  *upw = q.Wr;
  return true;
}

// 3x3 / stride-2 data gradient with zero leading pads on an even map (TF 'same': the FPN's P6 / P7
// convs, fcos.py:66-72; conv2d_backprop_input of a stride-2 kernel) as ONE 4-segment forward launch
// over the dY map.  Input pixel (2k + py, 2k' + px) receives dY[k - 1 + r'][k' - 1 + s'] through
// the 2x2 sub-kernel of its parity class: tap r' = 1 is r = 0 (py even) / r = 1 (odd), r' = 0 is
// r = 2 (even) / nothing (odd) -- the same along x.  The four sub-kernels are gathered from the
// dgrad pack into the workspace (missing taps zero) and the results scatter by dst_up = 2 at offset
// py * W + px.  K = 4 * Cout instead of the 9 * Cout of the direct form, most of whose taps meet dY
// rows that do not exist at the pixel's parity (c6 dgrad 256 -> 2048 @ 16^2: 82 us).
bool s2dgrad3_ok(const cvl_conv_desc* d) {
  if (!d || d->mode != CVL_CONV_DGRAD || d->KH != 3 || d->KW != 3 || d->stride != 2 || d->pad_t || d->pad_l ||
      d->nseg != 1 || d->relu_in || d->prec != CVL_PREC_BF16 || d->Cin % 32 || d->Npad % 32 ||
      cvl_dispatch_flag("no_s2dg3"))
    return false;
  const cvl_conv_seg& q = d->seg[0];
  // small maps (P7's 8x8 at bs 16: 1024 rows) keep the direct form, whose split-K fills the GPU
  // (the 4-segment launch has no split-K: 16 workgroups, 22 -> 37 us)
  return q.Hr == 2 * q.Hs && q.Wr == 2 * q.Ws && q.w &&
         (long)d->B * q.Hr * q.Wr >= cvl_dispatch_int("s2dg3_min_rows", 4096);
}

size_t s2dgrad3_pack_bytes(const cvl_conv_desc* d) {
  return ((size_t)4 * d->Npad * 4 * d->Cin * sizeof(cvl_bf16) + 255) / 256 * 256;
}

// the 4-segment forward descriptor over the packs at `sub` (the plan lays it out over a placeholder;
// the call points the segments at its workspace)
cvl_conv_desc s2dgrad3_desc(const cvl_conv_desc* d, const cvl_bf16* sub) {
  cvl_conv_desc dd = *d;
  const cvl_conv_seg q = d->seg[0];
  dd.mode = CVL_CONV_FWD;
  dd.KH = dd.KW = 2;
  dd.stride = 1;
  dd.pad_t = dd.pad_l = 1;
  dd.nseg = 4;
  for (int cls = 0; cls < 4; ++cls) {
    cvl_conv_seg& g = dd.seg[cls];
    g = q;
    g.Hr = q.Hs;
    g.Wr = q.Ws;
    g.w = sub + (size_t)cls * d->Npad * 4 * d->Cin;
    g.bias = nullptr;
    g.dst_base = q.dst_base + (long)(cls >> 1) * q.Wr + (cls & 1);
  }
  return dd;
}
const cvl_bf16* const kPackPlaceholder = reinterpret_cast<const cvl_bf16*>(16);

bool dst_chunks8(const cvl_conv_desc* d) { return d->n_store % 8 == 0 && d->ld_dst % 8 == 0 && d->dst_coff % 8 == 0; }

// every segment's map a whole number of 256-row tiles (a tile inside one image); dense: and its
// destination images back to back (the fused BN sums index z by destination row)
bool tiles_in_images(const ConvArgs& a, bool dense) {
  for (int i = 0; i < a.nseg; ++i) {
    const long hw = (long)a.seg[i].Hr * a.seg[i].Wr;
    if (hw % BM || (dense && a.seg[i].dst_img != hw)) return false;
  }
  return true;
}

// every source / weight byte offset below the buffer-resource bound of the X / H / P operand fetches
bool buffer_bounds_ok(const ConvArgs& a) {
  for (int i = 0; i < a.nseg; ++i) {
    const ConvSeg& q = a.seg[i];
    const long src_bytes = (q.src_base + (long)a.B * q.src_img) * a.Cin * 2;
    if (src_bytes >= (long)kConvBufRecords - 65536) return false;
  }
  return (long)a.Npad * a.K * 2 < (long)kConvBufRecords;
}

// ---- X32 ----------------------------------------------------------------------------------------
bool x32_fits(const cvl_conv_desc* d, const ConvArgs& a) {
  const bool dg = d->mode == CVL_CONV_DGRAD;
  if (a.Npad % 256 || a.Cin % 32 || a.K / 32 < 1 || d->KH * d->KW > 32 || a.relu_in || (dg && d->stride != 1) ||
      a.dst_up != 1)
    return false;
  return buffer_bounds_ok(a);
}

bool plan_x(const cvl_conv_desc* d, const ConvArgs& a, const ConvCallOpts& o, ConvPlan* p) {
  if (cvl_dispatch_flag("no_x") || !x32_fits(d, a)) return false;
  p->kernel = CVL_CK_X32;
  p->bn = 256;
  p->bk = 32;
  p->grid = a.m_tiles * (a.Npad / 256);
  p->dbg = cvl_tune_int("CVL_X_ABLATE", 0);     // measurement builds (tools/x32_*.py): ablation bits
  // SW epilogue: bf16 destination in 8-channel chunks, no BN statistics, no beta
  p->sw = !a.dst_f32 && !o.bn_stats && a.beta == 0.f && dst_chunks8(d) && !cvl_dispatch_flag("x_no_sw");
  // the ReLU mask in the register epilogue
  p->ymask = p->sw && o.ymask && !a.relu_out && !cvl_dispatch_flag("no_relu_mask_fuse");
  return true;
}

// ---- P ------------------------------------------------------------------------------------------
bool p_fits(const cvl_conv_desc* d, const ConvArgs& a, const ConvCallOpts& o) {
  if (d->KH != 1 || d->KW != 1 || d->pad_t || d->pad_l || a.relu_in || a.nseg != 1 || a.K % 32) return false;
  // bsum forms: z-mask without beta; y-mask (residual unit) with the beta accumulate
  // (the residual form also on the strided data gradient's scatter, dst_up 2: the gap pixels' dy is 0,
  // so the scattered rows' sums are the map's)
  const bool by = o.bsum == CVL_BSUM_Y || o.bsum == CVL_BSUM_BITS;
  // (the bitmap holds one byte per 8-channel chunk of a y row: whole chunks only)
  if (o.bsum == CVL_BSUM_BITS && (a.ld_dst % 8 || a.dst_coff % 8)) return false;
  if (o.bsum && ((d->mode != CVL_CONV_DGRAD && a.dst_up == 1) || a.dst_f32 || (a.beta != 0.f) != by ||
                 (a.dst_up != 1 && !by) || o.bn_stats || (a.seg[0].Hr * a.seg[0].Wr) % BM ||
                 (a.dst_up == 1 && a.seg[0].dst_img != (long)a.seg[0].Hr * a.seg[0].Wr) || a.Npad % 64))
    return false;
  if (d->mode == CVL_CONV_DGRAD && d->stride != 1) return false;
  const ConvSeg& q = a.seg[0];
  if (d->stride == 1 && (q.Hs != q.Hr || q.Ws != q.Wr)) return false;
  if (a.dst_f32 ? (a.n_store % 4 || a.ld_dst % 4 || a.dst_coff % 4) : !dst_chunks8(d)) return false;
  if (o.bn_stats && (a.dst_f32 || (q.Hr * q.Wr) % BM)) return false;
  return buffer_bounds_ok(a);
}

bool plan_p(const cvl_conv_desc* d, const ConvArgs& a, const ConvCallOpts& o, ConvPlan* p) {
  if (cvl_dispatch_flag("no_p") || !p_fits(d, a, o)) return false;
  if (o.bsum && cvl_tune_flag("CVL_CONV_P_NO_BSUM")) return false;
  // N tile: 128 for short K (<= 256: fwd 1x1 64->256 @ 128^2 44 -> 36 us, 128->512 @ 64^2 31 -> 26,
  // 256->1024 @ 32^2 25 -> 21), 64 for long K (1024->256 @ 32^2 20.5 vs 23, 2048->512 @ 16^2 29.5
  // vs 35; tools/p_probe.py)
  // ... and 128 where the output is much wider than K (512->2048 @ 16^2 fwd 22.4 -> 18.9 us; the
  // same GEMM shape as conv5_x's 2048->512 data gradient), 64 for the long-K narrow ones
  const bool wide = a.K <= 256 || (a.Npad >= 2 * a.K && cvl_dispatch_int("p_wide128", 1));
  const int bn = wide && a.Npad % 128 == 0 ? 128 : (a.Npad % 64 == 0 ? 64 : 0);
  const int fbn = cvl_dispatch_int("p_bn", 0);
  const int use = o.bsum ? 64 : (fbn && a.Npad % fbn == 0 ? fbn : bn);
  if (!use) return false;
  const int ntiles = a.m_tiles * (a.Npad / use);
  const int ntn = a.Npad / use;
  // (CVL_DISPATCH=p_wgs: a test hook -- several tiles per workgroup at small sizes; 1 .. 256)
  const int wgs = cvl_dispatch_int("p_wgs", 256);
  int grid = cvl_tune_int("CVL_CONV_P_WGS", wgs > 256 ? 256 : (wgs < 1 ? 1 : wgs));
  if (grid >= ntiles) grid = ntiles;
  else grid -= grid % ntn;                      // every workgroup keeps one N tile
  if (grid < 1) return false;
  p->kernel = CVL_CK_P;
  p->bn = use;
  // 64-deep K-tiles (128-B operand rows) wherever K allows; the 256-wide tile's ring has no room
  p->bk = a.K % 64 == 0 && use != 256 && cvl_dispatch_int("p_k64", 1) ? 64 : 32;
  p->grid = grid;
  p->dbg = cvl_tune_int("CVL_P_ABLATE", 0);
  p->bsum = o.bsum;
  p->acc = a.beta != 0.f && !cvl_tune_flag("CVL_P_NO_ACC");
  // relu(conv + bias + old) (cvl_conv_igemm_res_relu): the accumulate form's 64- and 128-wide tiles
  p->res_relu = o.res_relu && p->acc && use != 256 && !cvl_dispatch_flag("no_res_relu_fuse");
  return true;
}

// ---- H64 ----------------------------------------------------------------------------------------
// `ws_bytes`: the split-K workspace on offer (0: no split)
bool plan_h(const cvl_conv_desc* d, const ConvArgs& a, const ConvCallOpts& o, size_t ws_bytes, ConvPlan* p) {
  int halo_px = 0;
  if (cvl_dispatch_flag("no_h") || !cvl_conv_h_fits(d, a, &halo_px)) return false;
  // three stages for the 32-wide tiles when every segment's halo fits 512 pixels (CVL_DISPATCH=h_no_3stage: two)
  const bool stg3 = !cvl_dispatch_flag("h_no_3stage") && halo_px <= 512;
  const bool bs = o.bsum != CVL_BSUM_NONE;
  p->kernel = CVL_CK_H64;
  p->bk = H_BK;
  p->bsum = o.bsum;
  if (a.Npad == 32) {          // 256 x 32 tiles (the FCOS heads' forward): persistent, no split, fp32 epilogue
    if (o.bn_stats || bs) return false;
    p->bn = 32;
    p->stages = stg3 ? 3 : 2;
    p->grid = a.m_tiles < device_cus() ? a.m_tiles : device_cus();
    return true;
  }
  // 32-wide tiles (round 6) for the SW-epilogue launches whose 64-wide grid fills at most half of the
  // CUs (the conv5_x 3x3 units at 512 / bs 16, forward and data gradient: 128 tiles -> 256): every CU
  // gets a tile and no launch splits its channel blocks into fp32 slabs
  const int tiles = a.m_tiles * (a.Npad / H_BN);
  // SW epilogue (registers -> 16-B stores, statistics per (image, N tile)): every tile inside one
  // image, bf16 destination in 8-channel chunks, no beta, statistics OR fused BN sums
  const bool sw_ok = !d->dst_f32 && d->beta == 0.f && dst_chunks8(d) && !(o.bn_stats && bs) && tiles_in_images(a, bs);
  if (!cvl_dispatch_flag("h_no_n32") && a.Npad % H_BN == 0 && 2 * tiles <= device_cus() && sw_ok) {
    p->bn = 32;
    p->sw = true;
    p->stages = stg3 ? 3 : 2;
    p->grid = 2 * tiles;
    return true;
  }
  const int ncb = a.Cin / H_BK;
  // split the channel blocks of grids that leave CUs idle (fp32 slabs, single segment, no fused
  // BN-backward sums: the finish kernel forms BN statistics but not those)
  int splits = 1;
  if (a.nseg == 1 && !bs && ws_bytes && d->n_store % 8 == 0 && d->dst_coff % 8 == 0 &&
      (d->dst_f32 || d->ld_dst % 8 == 0) && d->n_store / 8 <= 256) {
    splits = h_split_want(a);
    if (slab_bytes(a, splits) > ws_bytes) splits = 1;
  }
  if (splits > 1) conv_plan_set_splits(p, ncb, splits);
  // persistent: one workgroup per CU walks a contiguous chunk of tiles (split launches: one tile
  // per workgroup, the K splits on blockIdx.z)
  const int per_cu = cvl_tune_int("CVL_CONV_H_WG_PER_CU", 1);
  p->grid = p->splits > 1 ? tiles : (tiles < device_cus() * per_cu ? tiles : device_cus() * per_cu);
  p->bn = H_BN;
  p->stages = 2;
  p->wres = p->splits <= 1 && a.Npad == H_BN && ncb <= kConvHWresCb && a.nseg == 1 && !cvl_dispatch_flag("h_no_wres");
  p->sw = p->splits <= 1 && sw_ok && !cvl_dispatch_flag("h_no_sw");
  p->stamps = cvl_tune_flag("CVL_H_STAMPS") && p->splits <= 1 && p->grid <= kConvHStampWgs;
  return true;
}

// ---- the 256-row families: H64 / P / X32 / L ------------------------------------------------------
// what P, X32, H64 (64 wide) and L share: 32-channel K steps, no ReLU on the source, 16-B bf16 stores
// (fp32 destinations store element-wise: any n_store % 4, the RetinaNet box heads: 9 anchors x 4 =
// 36; no BN statistics from them)
bool large_fits(const cvl_conv_desc* d, const ConvCallOpts& o) {
  if (d->Cin % 32 != 0 || d->relu_in) return false;
  return d->dst_f32 ? (d->n_store % 4 == 0 && !o.bn_stats) : dst_chunks8(d);
}

// false: none of them takes the launch (the 128-row kernel does; a fused BN-sums offer is declined)
bool plan_large(const cvl_conv_desc* d, const ConvArgs& a, const ConvCallOpts& o, ConvPlan* p) {
  if (cvl_dispatch_flag("no_l")) return false;
  const bool bs = o.bsum != CVL_BSUM_NONE, by = o.bsum == CVL_BSUM_Y || o.bsum == CVL_BSUM_BITS;
  // the residual form on a strided 1x1 data gradient's scatter (the descriptor rewritten as the dense
  // forward GEMM over the dY grid, dst_up 2): the persistent kernel only, whose predicate provides
  // for it (offered by CVL_DISPATCH=bnsum_res_s2 only)
  const bool scat = by && a.dst_up != 1 && d->KH == 1 && d->KW == 1 && d->mode == CVL_CONV_FWD;
  if (bs && !scat &&
      (d->mode != CVL_CONV_DGRAD || d->dst_f32 || (d->beta != 0.f && !by) || a.dst_up != 1 || o.bn_stats))
    return false;
  if (scat && (d->dst_f32 || o.bn_stats)) return false;
  // the residual (y-mask) form exists on the 1x1 persistent kernel only
  if (by && (d->KH != 1 || d->KW != 1)) return false;
  // 3x3 / stride 1 forwards 32 wide into fp32 (the FCOS heads, 256 -> 20 / 5 over the five levels,
  // fcos.py:85-88, 99-101): the halo kernel with 256 x 32 tiles -- one halo stage per 32-channel
  // block feeds all nine taps, where the 128-row generic kernel re-gathers nine im2col tiles
  if (d->Npad == 32 && d->KH == 3 && d->KW == 3 && d->mode == CVL_CONV_FWD && d->dst_f32 && !o.bn_stats &&
      !bs && a.dst_up == 1 && d->Cin % 32 == 0 && !d->relu_in && !cvl_dispatch_flag("no_h32"))
    return plan_h(d, a, o, 0, p);
  if (!large_fits(d, o)) return false;
  if (d->dst_f32 && (cvl_tune_flag("CVL_CONV_L_F32_N8") || cvl_tune_flag("CVL_CONV_L_NO_F32"))) return false;   // A/B knobs
  const bool l_cin = d->Cin % 64 == 0;          // the L / X kernels: 64-channel K steps
  // 256-wide tiles (forward and data-gradient) for launches with >= CVL_CONV_L256_MIN_TILES of
  // them.  A single FCOS tower's dgrad (341 tiles) lost 35 % on them (tools/conv_ab.py); the
  // paired cls+reg tower dgrad (682 tiles) gains: whole step 813 -> 827 img/s
  // (tools/gpu_knob_sweep.sh).  CVL_CONV_NO_DGRAD_256=1 restores forward-only.
  const bool w256 = d->Npad % 256 == 0 && !cvl_dispatch_flag("no_256") &&
                    (d->mode == CVL_CONV_FWD || !cvl_tune_flag("CVL_CONV_NO_DGRAD_256"));
  const int bn = w256 ? 256 : (d->Npad % 128 == 0 ? 128 : (d->Npad % 64 == 0 ? 64 : 0));
  if (!bn) return false;
  if (l_cin && d->KH * d->KW * d->Cin < cvl_tune_int("CVL_CONV_L_MIN_K", 0) && !bs) return false;   // A/B knob
  // below 128 tiles the 128-row kernel with split-K fills the 256 CUs better (tests lower the
  // bar).  Whole-step sweep (tools/gpu_knob_sweep.sh, FCOS bs=16): 384 -> 773, 256 -> 785,
  // 192 -> 785, 128 -> 807, 1 -> 789 img/s (conv4_x 3x3 sits at exactly 128 tiles).  A launch
  // with too few 256-wide tiles drops to the 128-wide tile first (since the X32 kernel: 256 tiles,
  // e.g. one tower's 341-tile data gradient into F, FCOS 989 -> 995 img/s; 128: within noise).
  // 1x1 launches: the persistent streaming kernel (conv_igemm_p.hip)
  if (d->KH == 1 && d->KW == 1) {
    if (plan_p(d, a, o, p)) return true;
    if (by) return false;
  }
  const long min_tiles = cvl_dispatch_int("l_min_tiles", 128);
  int use_bn = bn;
  if (use_bn == 256 && (long)a.m_tiles * (a.Npad / 256) < cvl_dispatch_int("l256_min_tiles", 256)) use_bn = 128;
  // short-K launches are HBM-bound: 128-wide tiles (more of them) beat the 256-wide ones (FCOS +0.6 %,
  // CenterNet +0.4 % at K < 512)
  const int w256_min_k = cvl_dispatch_int("w256_min_k", 512);
  if (use_bn == 256 && a.K < w256_min_k) use_bn = 128;
  // a launch that would leave CUs idle with 128-wide tiles takes 64-wide ones (twice the tiles),
  // also when that lifts it over min_tiles (from the split-K 128-row kernel): FCOS A/B 970 -> 983
  // img/s at 256 for the 128-tile conv4_x launches, -> 988 with the conv5_x ones (512: 966, 1024: 941)
  const int fill = cvl_tune_int("CVL_CONV_L64_FILL", 256);
  const bool fill_pre = !cvl_tune_flag("CVL_CONV_L64_NO_FILL_PRE");
  const bool to64 = fill && use_bn == 128 && (long)a.m_tiles * (a.Npad / 128) < fill && a.Npad % 64 == 0 &&
                    !(bs && cvl_tune_flag("CVL_BSUM_NO_FILL"));
  // 32-channel sources into 256-wide outputs (the FCOS heads' data gradient, K = 9 x 32): the X32
  // ring kernel reads 64-B rows, i.e. one 32-channel block per K-tile (head dgrad 44.2 -> 30.7 us
  // per head vs the H64 halo kernel; step +0.25 %)
  if (!l_cin && d->Cin == 32 && bn == 256 && !bs && !o.bn_stats && cvl_dispatch_int("x_cin32", 1) &&
      plan_x(d, a, o, p))
    return true;
  // 3x3 / stride 1 launches that would run 64-wide tiles: the halo-staged 256 x 64 kernel
  // (conv_igemm_h.hip), whose A traffic is one halo per channel block instead of nine im2col tiles.
  // Not where the 256 x 128 tiles fill the chip: there the L kernel reads each A tile once for 128
  // columns (128 -> 128 @ 64^2, bs 16: L 33 / 47 us fwd / dgrad vs H64 41 / 52 us)
  const bool h_width = use_bn == 64 || to64 || !l_cin || cvl_tune_flag("CVL_CONV_H_ANY_N");
  if (h_width && use_bn != 256 && (!bs || ((a.seg[0].Hr * a.seg[0].Wr) % BM == 0 && !o.bn_stats)) &&
      (!bs || tiles_in_images(a, true)) && plan_h(d, a, o, o.workspace_bytes, p))
    return true;
  if (!l_cin) return false;
  // (as found, kept: with fill_pre the 64-wide tile count is what meets min_tiles, without it the
  // 128-wide one, and the launch still runs 64 wide)
  if (fill_pre && to64) use_bn = 64;
  if ((long)a.m_tiles * (a.Npad / use_bn) < min_tiles) return false;
  if (to64) use_bn = 64;
  if (o.bn_stats)
    for (int i = 0; i < a.nseg; ++i)
      if ((a.seg[i].Hr * a.seg[i].Wr) % 4) return false;
  // fused sums: one image per 256-row tile; the 256-wide tiles keep their own epilogue budget
  if (bs && (use_bn == 256 || !tiles_in_images(a, true))) return false;
  // the 256 x 256 ring kernel when it applies
  if (use_bn == 256 && plan_x(d, a, o, p)) return true;
  p->kernel = use_bn == 256 ? CVL_CK_L256 : (use_bn == 128 ? CVL_CK_L128 : CVL_CK_L64);
  p->bn = use_bn;
  p->bk = 64;
  p->grid = a.m_tiles * (a.Npad / use_bn);
  p->bsum = o.bsum;
  p->prio = !cvl_tune_flag("CVL_CONV_NO_PRIO");
  // SW epilogue: bf16 destination in 8-channel chunks, no beta / scatter / fused sums; with BN
  // statistics every tile inside one image
  p->sw = !a.dst_f32 && a.beta == 0.f && !bs && a.dst_up == 1 && dst_chunks8(d) && !cvl_dispatch_flag("l_no_sw") &&
          (!o.bn_stats || tiles_in_images(a, false));
  return true;
}

// the 128-row kernel: any valid descriptor
void plan_base(const cvl_conv_desc* d, const ConvArgs& a, const ConvCallOpts& o, ConvPlan* p) {
  p->bn = pick_bn(a.Npad);
  // narrow outputs (the FCOS / RetinaNet heads, N <= 64): 128-deep K steps -- twice the bytes per
  // register-staged load round in flight (these launches are bound by the load latency, not MFMA)
  p->bk = p->bn <= 64 && a.Cin % 128 == 0 && cvl_dispatch_int("base_bk128", 1) ? 128 : (a.Cin % 64 == 0 ? 64 : 32);
  const int sp = base_split_want(a);
  const bool split = sp > 1 && (d->n_store / 8 <= NT_BASE) && o.workspace_bytes >= slab_bytes(a, sp) &&
                     d->n_store % 8 == 0 && d->dst_coff % 8 == 0 && (d->dst_f32 || d->ld_dst % 8 == 0);
  if (split) conv_plan_set_splits(p, a.K / p->bk, sp);
  p->kernel = split ? CVL_CK_BASE_SPLITK : CVL_CK_BASE;
  p->grid = a.m_tiles * (a.Npad / p->bn);
}

// whether the entry's fused BN-sums offer is worth planning at all (the switches and floors of
// cvl_conv_igemm_dgrad_bnsum / _res)
bool bsum_offer_ok(const cvl_conv_desc* d, int form) {
  if (cvl_tune_flag("CVL_NO_BNSUM_FUSE") || d->prec != CVL_PREC_BF16 || d->mode != CVL_CONV_DGRAD || d->dst_f32 ||
      d->Cin % 32 || d->Npad % 32 || !dst_chunks8(d))
    return false;
  const long hw = (long)d->seg[0].Hr * d->seg[0].Wr;
  if (form == CVL_BSUM_Z)
    // (CVL_BNSUM_MIN_HW: A/B knob; unlike the residual form this one pays on every stage -- a 64x64
    // floor cost 0.6 %, 32x32 was neutral)
    return d->beta == 0.f && hw >= cvl_tune_int("CVL_BNSUM_MIN_HW", 0);
  return !cvl_tune_flag("CVL_NO_BNSUM_RES") && d->beta != 0.f && d->KH == 1 && d->KW == 1 &&
         (d->stride == 1 || !cvl_dispatch_flag("no_bnsum_res_s2")) &&
         // map-size floor (dispatch knob bnsum_res_min_hw): 4096 kept conv4_x / conv5_x on the plain
         // launch + separate pass in round 5; after round 6's kernel changes 256 (all ResNet-50 stages at
         // 512 px) wins, FCOS step same box 1381.1-1382.8 -> 1385.2-1388.6 img/s over 6 alternating runs
         hw >= cvl_dispatch_int("bnsum_res_min_hw", 256);
}

}  // namespace

// Plans one call.  CVL_EINVAL: the descriptor is invalid (nothing may be launched).  A fused BN-sums
// offer (o.bsum) that no kernel can take comes back as CVL_OK with p->kernel == CVL_CK_NONE: the
// caller plans again without it.
int conv_plan(const cvl_conv_desc* d, const ConvCallOpts& o, ConvPlan* p) {
  CVL_CHECK_ARG(d && p && d->prec == CVL_PREC_BF16);
  *p = ConvPlan{};
  p->kernel = CVL_CK_NONE;
  p->splits = 1;
  size_t ws_bytes = o.workspace_bytes;
  int up = 1, upw = 0;
  if (o.bsum) {
    // the z-mask form has no scatter; the residual form runs a strided data gradient (a stage's first
    // block accumulating onto its shortcut's) as the dense GEMM over the dY grid with the scatter
    // (dst_up): it accumulates (beta 1), so the gaps keep the zeros the first launch wrote and
    // contribute nothing to the sums
    if (!d->nseg || !bsum_offer_ok(d, o.bsum)) return CVL_OK;
    const bool tr = s2dgrad_transform(d, &p->desc, &up, &upw);
    if (o.bsum == CVL_BSUM_Z ? tr : (d->stride != 1 && !tr)) return CVL_OK;
    if (!tr) p->desc = *d;
  } else if (s2dgrad3_ok(d) && ws_bytes >= s2dgrad3_pack_bytes(d)) {
    CVL_CHECK_ARG(!o.bn_stats);
    CVL_CHECK_ARG(d->dst_f32 || dst_chunks8(d));
    p->pre = CVL_PRE_S2DG3_PACK;
    p->pack_bytes = s2dgrad3_pack_bytes(d);
    p->desc = s2dgrad3_desc(d, kPackPlaceholder);
    up = 2;
    upw = d->seg[0].Wr;
    ws_bytes -= p->pack_bytes;
  } else if (s2dgrad_transform(d, &p->desc, &up, &upw)) {
    CVL_CHECK_ARG(!o.bn_stats);
    CVL_CHECK_ARG(d->dst_f32 || dst_chunks8(d));
    if (d->beta == 0.f) {              // the pixels the scatter does not reach are zeroed first
      const cvl_conv_seg& q = d->seg[0];
      const long line = (long)q.Wr * (d->dst_f32 ? d->n_store : d->n_store / 8);
      CVL_CHECK_ARG(line < (1l << 31) && (long)d->B * q.Hr < (1l << 31));
      p->pre = CVL_PRE_ZERO_GAPS;
    }
  } else {
    p->desc = *d;
  }
  d = &p->desc;
  p->dgrad = d->mode == CVL_CONV_DGRAD;
  ConvCallOpts oo = o;
  oo.workspace_bytes = ws_bytes;
  ConvArgs base;
  const int st = cvl_conv_prepare(d, BM_BASE, &base);
  if (st) return o.bsum ? CVL_OK : st;
  if (!o.bsum) {
    CVL_CHECK_ARG(d->Cin % 32 == 0 && d->Npad % 32 == 0);
    if (!d->dst_f32) CVL_CHECK_ARG(dst_chunks8(d));
    if (o.bn_stats) {
      for (int i = 0; i < base.nseg; ++i) {
        const int hw = base.seg[i].Hr * base.seg[i].Wr;
        CVL_CHECK_ARG(hw % BM_BASE == 0 || hw % 4 == 0);   // quads of rows never straddle images
      }
    }
  }
  if (cvl_conv_prepare(d, BM, &p->geo) == CVL_OK) {
    p->geo.dst_up = up;
    p->geo.dst_w = upw;
    ConvPlan q = *p;                   // a family that declines late leaves no trace in the plan
    if (plan_large(d, p->geo, oo, &q)) *p = q;
  }
  if (p->kernel == CVL_CK_NONE) {
    if (o.bsum) return CVL_OK;         // the 128-row kernel has no fused form
    p->geo = base;
    p->geo.dst_up = up;
    p->geo.dst_w = upw;
    plan_base(d, p->geo, oo, p);
  }
  p->workspace_bytes = p->pack_bytes + (p->splits > 1 ? slab_bytes(p->geo, p->splits) : 0);
  return CVL_OK;
}

// The workspace cvl_conv_igemm_workspace_size reports: what the most demanding plan of this
// descriptor could use -- the 128-row kernel's split-K slabs or H64's, whichever is larger (callers
// size shared workspaces from it, whichever kernel then runs), after the s2dgrad3 packs.
size_t conv_plan_workspace_bound(const cvl_conv_desc* d) {
  if (s2dgrad3_ok(d)) {            // the sub-kernel packs, then the 4-segment launch's own needs
    const cvl_conv_desc dd = s2dgrad3_desc(d, kPackPlaceholder);
    return s2dgrad3_pack_bytes(d) + conv_plan_workspace_bound(&dd);
  }
  cvl_conv_desc dd;
  int up = 1, upw = 0;
  if (s2dgrad_transform(d, &dd, &up, &upw)) d = &dd;
  ConvArgs a;
  if (cvl_conv_prepare(d, BM_BASE, &a)) return 0;
  const int sp = base_split_want(a);
  size_t n = sp > 1 ? slab_bytes(a, sp) : 16;
  ConvArgs a256;                                   // the halo kernel's split-K slabs (256-row tiles)
  int halo_px = 0;
  if (cvl_conv_prepare(d, BM, &a256) == CVL_OK && a256.nseg == 1 && a256.Npad % H_BN == 0 &&
      cvl_conv_h_fits(d, a256, &halo_px)) {
    const int hs = h_split_want(a256);
    if (hs > 1 && slab_bytes(a256, hs) > n) n = slab_bytes(a256, hs);
  }
  return n;
}

// Test and profiling hook: the family and K-tile depth a cvl_conv_igemm call with these options
// would use.  Host only: no device memory, no launch.
extern "C" int cvl_conv_igemm_plan(const cvl_conv_desc* d, int with_bn_stats, size_t workspace_bytes, int32_t* kernel,
                                   int32_t* ktile) {
  CVL_CHECK_ARG(d && kernel && ktile);
  *kernel = CVL_CK_NONE;
  *ktile = 0;
  if (d->prec == CVL_PREC_F32) return CVL_OK;      // parity mode: its own kernels
  ConvPlan p;
  const int st = conv_plan(d, ConvCallOpts{with_bn_stats != 0, CVL_BSUM_NONE, false, workspace_bytes}, &p);
  if (st) return st;
  *kernel = p.kernel;
  *ktile = conv_plan_ktile(p);
  return CVL_OK;
}
