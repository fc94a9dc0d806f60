// Internal: segmented-conv argument block shared by the fwd/dgrad and wgrad kernels.
#pragma once
#include "cvl_common.h"
#include "bn_acc.h"
#include <type_traits>
#include <vector>

typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kMaxSeg = CVL_CONV_MAX_SEG;

// ReLU of a bf16 value on its bits: sign set -> +0 (exact; the fused residual epilogue and cvl_relu_
// share it, so the two forms of cvl_conv_igemm_res_relu agree bit for bit)
__device__ __forceinline__ short relu_bf16_bits(short v) { return v < 0 ? (short)0 : v; }

// kernel variant of the last cvl_conv_igemm call on this host thread (cvl_conv_igemm_last_kernel);
// the forward / data-gradient family sets it from the launch's ConvPlan (conv_igemm.hip: conv_run)
extern thread_local int g_cvl_conv_last_kernel;
// K-tile depth (32 / 64) of the last X or P launch on this host thread (cvl_conv_igemm_last_ktile)
extern thread_local int g_cvl_conv_last_ktile;

// Workgroups are dispatched round-robin over the 8 XCDs (hardware id b runs on XCD b % 8).  This
// bijective remap gives consecutive LOGICAL ids to the workgroups of one XCD, so tiles that read
// the same rows (the N tiles of an M tile, the (co, k) tiles of one reduction chunk) share that
// XCD's L2.
__device__ __forceinline__ int xcd_remap(int b, int nwg) {
  const int q = nwg / 8, r = nwg % 8, x = b % 8;
  return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + b / 8;
}

// s_waitcnt with only vmcnt constrained (gfx9 encoding: vmcnt[3:0] + vmcnt[5:4] at [15:14],
// expcnt [6:4] and lgkmcnt [11:8] left at their maxima)
template <int N>
__device__ __forceinline__ void wait_vm() {
  __builtin_amdgcn_s_waitcnt((N & 15) | ((N >> 4) << 14) | (7 << 4) | (15 << 8));
}

// ds_read_b64_tr_b16 (gfx950 transposed LDS read, 4 rows x 16 bf16 columns per 16-lane group) as
// inline asm, address = LDS byte address.  Through the builtin, the compiler's waitcnt pass cannot
// tell the read from LDS-DMA writes still in flight and drains vmcnt(0) before every read, which
// empties a DMA ring each step.  The compiler does not track these reads, so a caller orders its
// DMA itself (counted vmcnt + barriers) and, after the reads, calls lgkm_wait() and then tr_pin() on
// every result: the pins are volatile asm ordered after the wait and every use (copies included)
// depends on a pin, so nothing reads a fragment register before the data landed.
__device__ __forceinline__ s16x4 ds_tr16(unsigned addr) {
  s16x4 v;
  asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(v) : "v"(addr));
  return v;
}
// ds_tr16 with the instruction's 16-bit byte offset: one address register serves every read a
// lane-uniform constant apart
template <int OFF>
__device__ __forceinline__ s16x4 ds_tr16o(unsigned addr) {
  static_assert(OFF >= 0 && OFF < 65536 && OFF % 8 == 0, "ds offset field");
  s16x4 v;
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF));
  return v;
}
__device__ __forceinline__ void lgkm_wait() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
__device__ __forceinline__ void tr_pin(s16x4& v) { asm volatile("" : "+v"(v)); }
__device__ __forceinline__ s16x8 tr_join(s16x4 l, s16x4 h) {
  return s16x8{l[0], l[1], l[2], l[3], h[0], h[1], h[2], h[3]};
}

__device__ __forceinline__ unsigned lds_addr(const void* p) {
  return (unsigned)(size_t)(const __attribute__((address_space(3))) void*)p;
}

struct ConvSeg {
  int Hr, Wr, Hs, Ws;
  long src_base, src_img, dst_base, dst_img;
  int m_start;   // first row of this segment in the BM-padded M space
  int rows;      // valid rows = B * Hr * Wr
  const cvl_bf16* w;
  const float* bias;
};

struct ConvArgs {
  const cvl_bf16* src;
  void* dst;
  acc_u64* stats;     // BN statistics accumulators [B][n_store][2][acc_slots] (bn_acc.h) or null
  int acc_slots;      // the BN accumulators' mode: kAccSlots (exact) or 1 (float64 atomics)
  int nseg, B;
  ConvSeg seg[kMaxSeg];
  int Cin, KH, KW, stride, pad_t, pad_l;
  int K, Npad, n_store, ld_dst, dst_coff, dst_f32, relu_out, relu_in;
  float beta;
  int m_tiles, m_total;
  float* slab;      // split-K partial sums [splits][m_total][Npad] (fp32) or null
  int splits, ksteps_per_split;
  int dbg;            // kernel ablation bits for measurement (CVL_X_ABLATE), 0 in production
  int dst_up, dst_w;  // output pixel (y, x) of the GEMM grid lands at (y*dst_up, x*dst_up) of a
                      // dst_w-wide map (1x1 strided data-gradient as a dense GEMM); 1 = identity
  // BN-backward first pass fused into a data-gradient epilogue (cvl_conv_igemm_dgrad_bnsum): the
  // result is dy of a BN -> ReLU unit whose pre-BN z / (mean, rstd) / gamma / beta are given;
  // bsum[img][c] += (sum g, sum g * xhat), g = dy * (0 < bn(z) < bhi).  bsum null = off.
  const cvl_bf16* bz;
  const float* bmr;
  const float* bga;
  const float* bbe;
  acc_u64* bsum;
  float bhi;
  const cvl_bf16* by;     // non-null: the ReLU mask comes from y > 0 (a residual unit's output), not bn(z)
  const uint8_t* bbits;   // ... or from y's ReLU sign bitmap (uint8 [rows][ld_dst / 8], bit u = y[8c + u] > 0)
  unsigned long long* probe;   // cvl_probe_arm slot of this launch (kernels that support it), or null
  const cvl_bf16* ymask;       // data gradient through a ReLU: outputs where ymask <= 0 stored as 0 (X32 SW only)
};

// cvl_probe_arm (probe.hip): the slot armed for the current cvl_conv_igemm call (taken at its entry;
// take = clear it, so one armed slot times at most one launch)
uint64_t* cvl_probe_current(bool take);
void cvl_probe_enter_call();
void cvl_probe_leave_call();

// In-kernel launch timing into a cvl_probe_arm slot (u64 [4]: start, sum of ticks, launches, done
// workgroups): workgroup 0 stamps the start; every workgroup counts itself done after a barrier;
// the last one adds (now - start) and resets the counter.  Relaxed device-scope atomics only (no
// fences: a release fence at agent scope writes the L2 back and cost the tower launch ~15 %);
// workgroup 0 stores the start at its entry and counts itself done at its end, so the last
// workgroup reads a start stamp written long before.
__device__ __forceinline__ void probe_enter(unsigned long long* p) {
  if (blockIdx.x == 0 && threadIdx.x == 0) __hip_atomic_store(p, wall_clock64(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void probe_leave(unsigned long long* p) {
  __syncthreads();
  if (threadIdx.x == 0) {
    if (atomicAdd(p + 3, 1ull) == (unsigned long long)gridDim.x - 1) {
      const unsigned long long t = wall_clock64();
      const unsigned long long t0 = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      atomicAdd(p + 1, t - t0);
      atomicAdd(p + 2, 1ull);
      __hip_atomic_store(p + 3, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// an exact-mode BN accumulator buffer decoded in place (nn_ops.hip; no-op in the float64 mode)
int cvl_bn_acc_prepare(uint64_t* acc, long nstat, hipStream_t s);

// split-M weight-gradient reductions (conv_wgrad_defer.hip): queued while cvl_wgrad_defer(1) is on
int cvl_wgrad_reduce(const float* slab, float* dst0, float* dst1, long n4, int splits, int groups, float beta,
                     hipStream_t s);
int cvl_wgrad_defer_guard(const float* dst, hipStream_t s);
int cvl_wgrad_reduce_lanes(long elems4, int splits);

// host-side bundle of the fused BN-backward sums arguments (cvl_conv_igemm_dgrad_bnsum)
struct BnSumArgs {
  const cvl_bf16* z;
  const float* mr;
  const float* gamma;
  const float* beta;
  acc_u64* sums;
  float hi;
  const cvl_bf16* y;      // residual unit: mask y > 0 (null: rebuilt from z)
  const uint8_t* bits;    // residual unit: y's ReLU sign bitmap (CVL_BSUM_BITS), laid out as y / 8
};

// ---- forward / data-gradient dispatch (conv_dispatch.hip) ---------------------------------------
// What a call offers beyond its descriptor.
// fused BN-backward sums: mask from bn(z) / from y / from y's ReLU sign bitmap (planned as the y form)
enum { CVL_BSUM_NONE = 0, CVL_BSUM_Z = 1, CVL_BSUM_Y = 2, CVL_BSUM_BITS = 3 };
struct ConvCallOpts {
  bool bn_stats;            // BN statistics requested
  int bsum;                 // fused BN-backward sums offered (CVL_BSUM_*)
  bool ymask;               // a ReLU mask offered (cvl_conv_igemm_relu_mask)
  size_t workspace_bytes;   // 0: no workspace
  bool res_relu;            // ReLU after the beta accumulate offered (cvl_conv_igemm_res_relu)
};

enum { CVL_PRE_NONE = 0, CVL_PRE_ZERO_GAPS = 1, CVL_PRE_S2DG3_PACK = 2 };   // pass before the launch

// Everything the host decides for one call, computed once by conv_plan (host only, launches nothing,
// the one reader of the family's cvl_dispatch_* / cvl_tune_* keys).  The launchers instantiate and
// launch what it says and decide nothing.
struct ConvPlan {
  int kernel;               // CVL_CK_* family
  int bn, bk;               // N-tile width, K-tile depth
  bool dgrad;
  bool sw;                  // register (SW) epilogue instead of the LDS C image
  bool wres;                // H64: weights resident
  bool prio, acc, stamps;   // L: s_setprio around the MFMA cluster; P: beta-accumulate form; H64: measurement stamps
  int stages;               // H64 ring stages (2 / 3)
  int bsum;                 // fused BN sums applied (CVL_BSUM_*; NONE when offered but not fusable)
  bool ymask;               // the ReLU mask is applied in the epilogue
  bool res_relu;            // P: ReLU after the beta accumulate in the epilogue (relu(conv + bias + old))
  int splits, ksteps_per_split;
  int grid;                 // workgroups (per split)
  size_t workspace_bytes;   // workspace this plan uses (pack + split-K slabs)
  int pre;                  // CVL_PRE_*
  size_t pack_bytes;        // CVL_PRE_S2DG3_PACK: the sub-kernel packs at the head of the workspace
  int dbg;                  // measurement builds: the kernel's ablation bits
  cvl_conv_desc desc;       // the descriptor the kernel runs (a strided data gradient rewritten)
  ConvArgs geo;             // its segment layout, dst_up / dst_w set, no pointers but the weights'
};

int conv_plan(const cvl_conv_desc* d, const ConvCallOpts& o, ConvPlan* p);
size_t conv_plan_workspace_bound(const cvl_conv_desc* d);
// splits / ksteps_per_split of `want` splits over nk K steps (no empty split)
static inline void conv_plan_set_splits(ConvPlan* p, int nk, int want) {
  p->ksteps_per_split = (nk + want - 1) / want;
  p->splits = (nk + p->ksteps_per_split - 1) / p->ksteps_per_split;
}
// what the K-tile query reports: the depth of an X or P launch, else 0
static inline int conv_plan_ktile(const ConvPlan& p) { return p.kernel == CVL_CK_X32 || p.kernel == CVL_CK_P ? p.bk : 0; }

// the launchers: conv_igemm.hip (128-row kernel), conv_igemm_{l,x,h,p}.hip; return the launch status
int launch_base(const ConvPlan& p, const ConvArgs& a, hipStream_t s);
int launch_l(const ConvPlan& p, const ConvArgs& a, hipStream_t s);
int launch_x(const ConvPlan& p, const ConvArgs& a, hipStream_t s);
int launch_h(const ConvPlan& p, const ConvArgs& a, hipStream_t s);
int launch_p(const ConvPlan& p, const ConvArgs& a, hipStream_t s);

// H64's geometry predicate (conv_igemm_h.hip, next to the halo geometry it tests); *halo_px: the
// largest segment halo in pixels
bool cvl_conv_h_fits(const cvl_conv_desc* d, const ConvArgs& a, int* halo_px);
constexpr int kConvHWresCb = 2;             // H64 weights-resident form: channel blocks at most (WRES_CB)
constexpr int kConvHStampWgs = 4096;        // H64 measurement stamps: workgroups at most (kHStampWgs)
constexpr unsigned kConvBufRecords = 0x7fffffffu;   // buffer-resource bound of the X / H / P operand fetches

// runtime bool -> template argument: with_bool(b, [&](auto B) { f<decltype(B)::value>(); })
template <class F>
static inline void with_bool(bool b, F&& f) {
  if (b) f(std::true_type{});
  else f(std::false_type{});
}

// ---- weight-gradient dispatch (conv_wgrad_dispatch.hip) -------------------------------------------
constexpr int kWgSegM = 128;        // segment / chunk alignment of the M space, every weight-gradient kernel
constexpr int kWgXMaxGroups = 2;    // groups one X launch covers
constexpr int kWgXMaxProb = 16, kWgHMaxProb = 12;   // problems per batched X / WH launch (kernel-argument bytes)

// One launch of a weight-gradient call: the kernel, the segments it covers and the family's parameters.
struct WgLaunch {
  int kernel;               // CVL_CK_WG_*
  int seg0, nseg, ngroups;  // segments [seg0, seg0 + nseg) of the call's descriptor, in ngroups equal groups
  int tile;                 // co tile width: S 32 / 64 / 128, L 128 / 256, X 128 / 256
  int rows;                 // reduction rows per step: S 64 / 128, X 32 / 64
  bool pf;                  // X: the next step's fragments are read under this step's MFMAs
  bool reads;               // X, pf: those reads placed one per MFMA gap (false: all x reads after the first row);
                            // WH: the pipelined step loop (false: the first form)
  int tiles, co_tiles;      // output tiles per (group, split) and along co; SN: input-channel tiles
  int chunk, nsplit;        // rows per split (WH: 128-row steps) and splits; SN: chunk rows, chunks of all segments
  int steps;                // WH: 128-row steps of the problem
  int g_m0[kWgXMaxGroups], g_m1[kWgXMaxGroups];   // X: M range of each group
  int cbase[kMaxSeg + 1];   // SN: first chunk of each segment
  size_t slab_bytes;        // fp32 partial sums this launch keeps in the workspace (0: it writes dW)
};

// Everything the host decides for one cvl_conv_wgrad[_grouped] call, computed once by wgrad_plan
// (host only, the one reader of the family's cvl_dispatch_* / cvl_tune_* keys): one launch over all
// groups, or one per group.  The launches run one after another on one workspace.
struct WgradPlan {
  int nlaunch;
  WgLaunch l[kMaxSeg];
  size_t workspace_bytes;
};
int wgrad_plan(const cvl_conv_desc* d, int ngroups, WgradPlan* p);

// the descriptor a launch runs: its segments of the call's descriptor
static inline cvl_conv_desc wgrad_launch_desc(const cvl_conv_desc* d, const WgLaunch& l) {
  cvl_conv_desc s = *d;
  s.nseg = l.nseg;
  for (int i = 0; i < l.nseg; ++i) s.seg[i] = d->seg[l.seg0 + i];
  return s;
}

// One launch group of cvl_conv_wgrad_batch: n problems in one WH or X launch with a common chunk, or
// (kernel CVL_CK_NONE) one problem that runs as its own call with the plan `single`.
struct WgBatchLaunch {
  int kernel, tile;                 // CVL_CK_WG_H / CVL_CK_WG_X (tile 256 / 128) / CVL_CK_NONE
  int n, idx[kWgXMaxProb];          // the problems, as indices into the call's list
  bool reads;                       // as WgLaunch::reads
  int chunk;                        // rows (WH: steps) per workgroup, common to the group
  int nsplit[kWgXMaxProb];
  size_t slab_off[kWgXMaxProb];     // byte offset of each problem's slabs from ws_off
  size_t ws_off, ws_bytes;          // the group's byte range in the workspace
  WgradPlan single;
};
struct WgradBatchPlan {
  std::vector<WgBatchLaunch> l;     // in launch order
  size_t workspace_bytes;
};
int wgrad_batch_plan(const cvl_conv_desc* const* d, int n, WgradBatchPlan* p);

// per-family predicates, next to the kernel geometry they test (a: the kWgSegM-padded layout of d)
bool wg_sn_fits(const cvl_conv_desc* d, int ngroups);
bool wg_h_fits(const cvl_conv_desc* d);
bool wg_x_fits(const cvl_conv_desc* d, int ngroups, const ConvArgs& a);
bool wg_x_batch_fits(const cvl_conv_desc* d, ConvArgs* a);
bool wg_l_fits(const cvl_conv_desc* d, const ConvArgs& a);

// the launchers: conv_wgrad{_sn,_h,_x,_l,}.hip.  d: the launch's own descriptor (wgrad_launch_desc), dw: its
// groups' outputs, ws: the call's workspace.  They fill the kernel arguments and return the launch status.
int launch_wg_sn(const WgLaunch& l, const cvl_conv_desc& d, const void* x, const void* dy, float* const* dw, float beta,
                 void* ws, hipStream_t s);
int launch_wg_h(const WgLaunch& l, const cvl_conv_desc& d, const void* x, const void* dy, float* const* dw, float beta,
                void* ws, hipStream_t s);
int launch_wg_x(const WgLaunch& l, const cvl_conv_desc& d, const void* x, const void* dy, float* const* dw, float beta,
                void* ws, hipStream_t s);
int launch_wg_l(const WgLaunch& l, const cvl_conv_desc& d, const void* x, const void* dy, float* const* dw, float beta,
                void* ws, hipStream_t s);
int launch_wg_s(const WgLaunch& l, const cvl_conv_desc& d, const void* x, const void* dy, float* const* dw, float beta,
                void* ws, hipStream_t s);
// the batched ones: problem i of the group is d[b.idx[i]] with x / dy / dw of the same index
int launch_wg_x_batch(const WgBatchLaunch& b, const cvl_conv_desc* const* d, const void* const* x, const void* const* dy,
                      float* const* dw, float beta, char* ws, hipStream_t s);
int launch_wg_h_batch(const WgBatchLaunch& b, const cvl_conv_desc* const* d, const void* const* x, const void* const* dy,
                      float* const* dw, float beta, char* ws, hipStream_t s);
// a whole planned call (conv_wgrad.hip): its launches in order, last kernel set from the plan
int wgrad_run(const WgradPlan& p, const cvl_conv_desc* d, const void* x, const void* dy, float* const* dw, float beta,
              void* ws, hipStream_t s);

// fp32 parity mode (parity_f32.hip)
size_t cvl_conv_wgrad_f32_workspace(const cvl_conv_desc* d, int ngroups);
int cvl_conv_wgrad_f32(const cvl_conv_desc* d, int ngroups, const void* x, const void* dy, float* const* dw,
                       float beta, void* workspace, size_t workspace_bytes, hipStream_t s);

// destination row of GEMM row q (within image img) of segment S
__device__ __forceinline__ long conv_dst_row(const ConvArgs& a, const ConvSeg& S, int img, int q) {
  long r = q;
  if (a.dst_up != 1) {
    const int y = q / S.Wr, x = q - (q / S.Wr) * S.Wr;
    r = (long)y * a.dst_up * a.dst_w + (long)x * a.dst_up;
  }
  return S.dst_base + (long)img * S.dst_img + r;
}

// Validate a public descriptor and lay its segments out in a BM-padded M space.
static inline int cvl_conv_prepare(const cvl_conv_desc* d, int bm, ConvArgs* a) {
  CVL_CHECK_ARG(d);
  CVL_CHECK_ARG(d->nseg >= 1 && d->nseg <= kMaxSeg && d->B >= 1);
  CVL_CHECK_ARG(d->Cin > 0 && d->KH > 0 && d->KW > 0 && d->stride > 0);
  CVL_CHECK_ARG(d->mode == CVL_CONV_FWD || d->mode == CVL_CONV_DGRAD);
  CVL_CHECK_ARG(d->Npad > 0 && d->n_store > 0 && d->n_store <= d->Npad);
  CVL_CHECK_ARG(d->ld_dst >= d->dst_coff + d->n_store);
  a->slab = nullptr;
  a->splits = 1;
  a->ksteps_per_split = 0;
  a->dst_up = 1;
  a->dst_w = 0;
  a->dbg = 0;
  a->bz = nullptr; a->bmr = nullptr; a->bga = nullptr; a->bbe = nullptr; a->bsum = nullptr; a->bhi = 0.f;
  a->by = nullptr;
  a->bbits = nullptr;
  a->probe = nullptr;
  a->ymask = nullptr;
  a->acc_slots = cvl_bn_acc_slots();
  a->nseg = d->nseg;
  a->B = d->B;
  a->Cin = d->Cin; a->KH = d->KH; a->KW = d->KW; a->stride = d->stride;
  a->pad_t = d->pad_t; a->pad_l = d->pad_l;
  a->K = d->KH * d->KW * d->Cin;
  a->Npad = d->Npad; a->n_store = d->n_store; a->ld_dst = d->ld_dst; a->dst_coff = d->dst_coff;
  a->dst_f32 = d->dst_f32; a->relu_out = d->relu_out; a->relu_in = d->relu_in; a->beta = d->beta;
  int m = 0;
  for (int i = 0; i < kMaxSeg; ++i) {
    ConvSeg& s = a->seg[i];
    if (i >= d->nseg) {
      s = a->seg[0];
      s.m_start = 0x7fffffff;
      continue;
    }
    const cvl_conv_seg& q = d->seg[i];
    CVL_CHECK_ARG(q.Hr > 0 && q.Wr > 0 && q.Hs > 0 && q.Ws > 0 && q.w);
    s.Hr = q.Hr; s.Wr = q.Wr; s.Hs = q.Hs; s.Ws = q.Ws;
    s.src_base = q.src_base; s.src_img = q.src_img; s.dst_base = q.dst_base; s.dst_img = q.dst_img;
    s.w = reinterpret_cast<const cvl_bf16*>(q.w);
    s.bias = q.bias;
    s.m_start = m;
    s.rows = d->B * q.Hr * q.Wr;
    m += ((s.rows + bm - 1) / bm) * bm;
  }
  a->m_total = m;
  a->m_tiles = m / bm;
  return CVL_OK;
}
