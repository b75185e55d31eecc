// mgp_common.h -- handle, workspace arena, error plumbing shared by the translation units.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/mgp.h"
#include "mgp_math.h"

struct mgp_handle {
  int device = 0;
  hipStream_t stream = nullptr;
  // mgp_set_stream with another stream: recorded on the outgoing stream, waited for by the incoming one, so that the
  // work enqueued through this handle runs in call order (the arenas below are shared by every call and invisible to
  // the caller).  Created with the handle, destroyed with it; an unchanged stream never touches it.
  hipEvent_t order_ev = nullptr;
  char err[512] = {0};
  // device workspace (partials of the two-stage reductions, CG state); grown on demand
  void* ws = nullptr;
  size_t ws_bytes = 0;
  // CG state arena, separate from ws so operator applications inside the solve can use ws
  void* cg = nullptr;
  size_t cg_bytes = 0;
  // operator scratch (u = K_nm p and the [Bt,M] partial of the SGPR operator)
  void* opws = nullptr;
  size_t opws_bytes = 0;
  // symmetric self-product scratch (kxx.hip): packed set, weights, running sum, slots of the band launches
  void* kxx = nullptr;
  size_t kxx_bytes = 0;
  int kxx_mode = 0;  // mgp_kxx_matvec / MGP_OP_KXX_NOISE: 0 = symmetric kernel where it serves (fp64, D <= 32, N >=
                     // kxx_min_n), 1 = wherever it can (MGP_KXX=sym), 2 = the plain sweep mgp_sweep(X, X) + s2 V (MGP_KXX=plain)
  long kxx_min_n = 1L << 16;  // MGP_KXX_MIN_N
  // symmetric operator above 32 dimensions (MGP_OP_KXX_NOISE_SYM_ANYD, kxx_sym_anyd.hip): the X whose pack stands at the
  // front of kxx for the solve under way (SymHold); null outside a solve, where every application packs for itself
  const void* sym_pack_src = nullptr;
  long sym_pack_n = 0;
  // hyper-parameter bilinear forms of k(X,X) (kxx_grad.hip): packed rows, packed columns, workgroup partials -- or,
  // on the panel route, one row panel of G = U V^T
  void* kgrad = nullptr;
  size_t kgrad_bytes = 0;
  int kxx_grad_mode = 0;  // mgp_kxx_grad: 0 = fused pair kernel where it serves (fp64, D <= 32; MGP_KXX_GRAD=fused),
                          // 2 = row panels through mgp_k_dense_vjp everywhere (MGP_KXX_GRAD=panel)
  // pivoted Cholesky of k(X,X) and the low-rank preconditioner application (pivchol.hip): the residual diagonal and
  // the step partials of a build, or the column-chunk partials of r B^T
  void* pch = nullptr;
  size_t pch_bytes = 0;
  // wide projection k(Xs, X) R (project.hip): the per-split partial tiles of the fused kernel -- or, on the generic
  // route, R^T, one row panel of k(Xs, X) and one chunk of the product
  void* prj = nullptr;
  size_t prj_bytes = 0;
  // many-column (K_mm + Lambda) operator (MGP_OP_KMM_LAMBDA_WIDE, project.hip): the Z whose pack stands at the front of
  // prj for the solve under way (WideHold); null outside a solve, where every application packs for itself
  const void* wide_pack_src = nullptr;
  long wide_pack_m = 0;
  // generic-D scratch (transposed multipliers, kernel panel, chunk output)
  void* gen = nullptr;
  size_t gen_bytes = 0;
  // packed streamed points of the fp64 SE fast sweep (sweep.hip).  Two slots: a solve alternates the K_nm
  // direction (streamed set Z) and the K_mn direction (streamed set X).  A pack is reused only while
  // `pack_hold` is set -- inside mgp_pcg_solve, where the operator's X, Z and kernel cannot change.
  struct PackSlot {
    void* buf = nullptr;
    size_t bytes = 0;
    const void* src = nullptr;
    long n = 0;
    int D = 0;
    double inv_ls[MGP_FUSED_MAX_D] = {0};
    bool valid = false;
  } pack[2];
  int pack_next = 0;
  bool pack_hold = false;
  // mgp_create_ex: one caller-sized block that serves every arena above; no hipMalloc/hipFree after create
  void* pool = nullptr;
  size_t pool_bytes = 0, pool_used = 0;
  // pinned host word for the convergence poll
  int* host_flag = nullptr;
  hipEvent_t poll_ev[2] = {nullptr, nullptr};  // one polled batch of the dense one-RHS CG in flight (cg.hip)
  // SGPR operator, one right-hand side: the s2*Kmm.p slab product runs on a stream of its own beside the K_nm sweep
  // (it reads Kmm from HBM while the sweep is bound by vector-ALU issue) and enters the K_mn sweep as its addend
  // (MGP_SGPR_KMM_ASIDE=0: on the solve's stream after both sweeps, as rounds 1-3; 1: for slabs of 48 MB and more; 2: always)
  int kmm_aside = 1;
  hipStream_t aside_stream = nullptr;
  hipEvent_t aside_ev[2] = {nullptr, nullptr};  // fork (p is ready), join (Kmm.p is ready)
  // most right-hand sides the tile scheme takes (MGP_CG_DENSE1_COLS: 1 = one only, as round 3; up to 8); 0 = by size,
  // where it was measured faster than the skinny product + fused update: 4 for n <= 4096, 6 above
  int cg_dense1_cols = 0;
  int d1_first_poll_sleep = 16;  // register-resident dense CG, owners: x 64 cycles before the first poll of the slots (MGP_D1_FIRST_POLL)
  int d1_inject_absent = -1;  // test only (MGP_D1_INJECT_ABSENT=<workgroup>): that workgroup of the register-resident solve leaves at once
  int d1_owner_spread = 1;  // super-block form, several columns: the columns of a chunk owned by different workgroups (MGP_D1_OWNER_SPREAD=0: by one)
  int poll_pipeline = 1;  // MGP_CG_PIPELINE_POLLS=0: drain the stream at every poll (round 3)
  void* ones = nullptr;  // device constants: double 1.0 at +0, float 1.0f at +8
  void* e2tabs = nullptr;  // exp2 tables of the fast fp64 sweep (8192 + 2048 entries, sweep.hip: mgp_build_e2tabs)
  double* dparams = nullptr;  // device copy of c/lengthscale_d for the generic-D kernels [MGP_MAX_D]
  // the same for the fused any-D sweeps (sweep_anyd.hip), with the host copy of what stands there: uploaded on change
  double* anyd_sc = nullptr;
  double anyd_sc_host[MGP_MAX_D] = {0};
  int anyd_sc_n = 0;  // entries of anyd_sc that are valid (0: none)
  int num_cus = 256;
  // 0 = fused sweeps on the VALU (sweep.hip, default: measured faster), 1 = fp64 distance
  // cross-term on the matrix cores (sweep_mfma.hip); MGP_SWEEP=mfma selects 1 for A/B runs
  int sweep_mode = 0;
  // fp64 sweeps: sweep_fast_kernel (scalar-loaded packed points, integer exponent scaling) with 1 = 256 threads /
  // 2048-entry table (one right-hand side only), 2 = 512 threads / 8192-entry table and a one-instruction table
  // offset at D <= 16; 0 = the LDS-tile kernel it replaced (MGP_SWEEP_FAST, for A/B runs)
  int sweep_fast = 2;
  int pf_trips = 16, pf_ahead = 6144;  // L2 prefetch of streamed rows: every pf_trips loop trips (power of two), pf_ahead bytes on
  // chunking of the streamed set aims at this many 256-thread workgroups per CU (MGP_SWEEP_TARGET).  16 since the
  // per-workgroup timeline of round 2: the two workgroups of a CU do not share it, the older one runs at full speed
  // and the younger fills its stalls, so each CU ends with one workgroup running alone at ~0.82 of the rate of two --
  // the shorter the workgroups, the shorter that tail (C3: 4.75 -> 4.66 ms per CG step against 8)
  int sweep_target_per_cu = 16;
  int sweep_chunk_gran = 0;  // fast kernel: streamed points per chunk are a multiple of this (MGP_SWEEP_GRAN: 64, 128, 256); 0 = the tile size TB of the shape
  int sweep_fast_rpt32 = 2;  // the same for 16 < D <= 32: 2 (2 waves/SIMD) or 1 (4 waves/SIMD) -- MGP_SWEEP_RPT32
  int sweep_fast_rpt_rc = 2;  // owned points per lane with 2 or 4 right-hand sides at D <= 8 (2 or 3) -- MGP_SWEEP_RPT_RC
  int sweep_fast_rpt = 4;  // owned points per lane of the fast kernel: 4 (4 waves/SIMD), 3 (5), 2 (8) -- MGP_SWEEP_RPT
  // K^T panel size per launch of the two-stage contraction: small enough to stay in the 256 MiB
  // Infinity Cache between its write (k_dense) and its ~33 re-reads (MGP_CONTRACT_PANEL_MB)
  size_t contract_panel_mb = 2048;
  int contract_nz = 16;
  // one-RHS symmetric product on the upper triangle (dense.hip); sizes below tri_min_n use the
  // row-streaming GEMV (MGP_TRI_MIN_N)
  long tri_min_n = 1024;
  // form of that product's tile kernel: 1 = row sums by a cross-lane reduce-scatter (2 KB of LDS), 0 = round 1's
  // LDS-staged row sums (35 KB, four workgroups per CU) -- MGP_TRI_FORM
  int tri_form = 1;
  void* tri_tab = nullptr;  // (I, J) of the upper-triangle tiles in launch order, for tri_tab_nt tile rows
  size_t tri_tab_bytes = 0;
  int tri_tab_nt = 0;
  // one-right-hand-side dense CG (the reference's literal loop, conjugate_gradient.py:65-84): 3 = for n <= 4096 the
  // whole solve in ONE launch with the upper triangle of A held in registers (cg_dense1.hip, round 4) and the
  // two-launch iteration above that, 1 = two launches per iteration everywhere, 0 = product (tile kernel + slot
  // reduce) + fused update launch (MGP_CG_DENSE1)
  int cg_dense1 = 3;
  int kdense_ta = 0;  // rows of A per block of k_dense_kernel: 0 = by shape (16, or 64 at D > 8), else 16 or 64 (MGP_KDENSE_TA)
  int gemm_ksplit = 1;  // mid-size GEMMs: 128x128 tiles x K slices instead of 64x64 tiles (MGP_GEMM_KSPLIT=0 disables)
  int skinny_blocks_per_cu = 0;  // k slices of the skinny product: workgroups per CU to aim for; 0 = by panel width (MGP_SKINNY_BPC)
  int skinny_stagger = 0;  // experiment (MGP_SKINNY_STAGGER): start-up delay units between workgroup phases
  int fuse_agree = 1;  // MGP_FUSE_AGREE=0: put_gate_word_kernel + finish_allreduce_kernel as launches of their own
  int skinny_defer = 1;  // MGP_SKINNY_DEFER=0 keeps the separate reduce launch inside the CG loop
  int skinny_pipe = 1;  // software-pipelined form of the LDS-staged product when n % 64 == 0 and Bt <= 64 (MGP_SKINNY_PIPE=0: the round-1 form)
  int skinny_mode = 1;  // 2 <= Bt <= 128 product: 1 = P staged through LDS, 0 = register operands (MGP_SKINNY=reg)
  int nosplit_per_cu = 4;  // owned-side workgroups per CU above which the streamed set is not split (MGP_NOSPLIT_PER_CU)
  // bench-only: event pairs around sweep launches (mgp_profile_enable / mgp_profile_read)
  bool prof_on = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_ev;
  size_t prof_used = 0;
  // bench-only: clock stamps of the profiled sweep launches (mgp_profile_read_clocks): 16 slots of 4 words each
  void* prof_clk = nullptr;
  size_t prof_clk_bytes = 0;
  size_t prof_clk_launches = 0;
};

// scope guard of mgp_pcg_solve: packs made during the solve are reused by its later iterations
struct PackHold {
  mgp_handle* h;
  explicit PackHold(mgp_handle* hh) : h(hh) {
    h->pack[0].valid = h->pack[1].valid = false;
    h->pack_hold = true;
  }
  ~PackHold() {
    h->pack_hold = false;
    h->pack[0].valid = h->pack[1].valid = false;
  }
};

// scope guard of mgp_pcg_solve on MGP_OP_KMM_LAMBDA_WIDE and MGP_OP_KMM_LAMBDA_WIDE_ANYD: Z is packed once, before the loop, and held until the solve ends
struct WideHold {
  mgp_handle* h;
  explicit WideHold(mgp_handle* hh) : h(hh) { release(); }
  void hold(const void* Z, long M) {
    h->wide_pack_src = Z;
    h->wide_pack_m = M;
  }
  void release() {
    h->wide_pack_src = nullptr;
    h->wide_pack_m = 0;
  }
  ~WideHold() { release(); }
};

// the same guard for MGP_OP_KXX_NOISE_SYM_ANYD: X is packed once at the front of the kxx arena and held until the solve ends
struct SymHold {
  mgp_handle* h;
  explicit SymHold(mgp_handle* hh) : h(hh) { release(); }
  void hold(const void* X, long N) {
    h->sym_pack_src = X;
    h->sym_pack_n = N;
  }
  void release() {
    h->sym_pack_src = nullptr;
    h->sym_pack_n = 0;
  }
  ~SymHold() { release(); }
};

constexpr int MGP_PROF_CLK_WORDS = 64;       // per profiled launch: 16 slots x (real0, clk0, real1, clk1)
constexpr int MGP_PROF_CLK_LAUNCHES = 8192;  // launches with stamps between two mgp_profile_enable(1) calls

// the stamp slot block of the NEXT profiled launch (nullptr when profiling is off or the block is used up)
inline unsigned long long* mgp_prof_clk_next(mgp_handle* h) {
  if (!h->prof_on || !h->prof_clk || h->prof_clk_launches >= (size_t)MGP_PROF_CLK_LAUNCHES) return nullptr;
  return (unsigned long long*)h->prof_clk + (h->prof_clk_launches++) * MGP_PROF_CLK_WORDS;
}

// which = 0 at the start of a workgroup, 1 when its loop has ended: 16 evenly spaced workgroups of the launch stamp
// (constant 100 MHz counter, shader-clock counter).  One lane, two scalar reads, one 16-byte store; nothing is kept
// in registers in between.
__device__ __forceinline__ void mgp_prof_stamp(unsigned long long* clk, int which) {
  if (clk == nullptr) return;
  const unsigned stride = gridDim.x >= 16 ? gridDim.x >> 4 : 1;
  const unsigned slot = blockIdx.x / stride;
  if (blockIdx.x == slot * stride && slot < 16 && threadIdx.x == 0) {
    clk[4 * slot + 2 * which] = __builtin_amdgcn_s_memrealtime();
    clk[4 * slot + 2 * which + 1] = __builtin_amdgcn_s_memtime();
  }
}

// returns the stop event to record after the launch (nullptr when profiling is off)
inline hipEvent_t mgp_prof_begin(mgp_handle* h) {
  if (!h->prof_on) return nullptr;
  if (h->prof_used == h->prof_ev.size()) {
    hipEvent_t a, b;
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return nullptr;
    h->prof_ev.emplace_back(a, b);
  }
  auto& pr = h->prof_ev[h->prof_used++];
  (void)hipEventRecord(pr.first, h->stream);
  return pr.second;
}
inline void mgp_prof_end(mgp_handle* h, hipEvent_t stop) {
  if (stop) (void)hipEventRecord(stop, h->stream);
}

inline int mgp_fail(mgp_handle* h, int code, const char* fmt, ...) {
  if (h) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(h->err, sizeof(h->err), fmt, ap);
    va_end(ap);
  }
  return code;
}

#define MGP_HIP(h, call)                                                                  \
  do {                                                                                    \
    hipError_t e__ = (call);                                                              \
    if (e__ != hipSuccess)                                                                \
      return mgp_fail((h), MGP_E_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e__), \
                      __FILE__, __LINE__);                                                \
  } while (0)

#define MGP_TRY(call)          \
  do {                         \
    int rc__ = (call);         \
    if (rc__ != MGP_OK) return rc__; \
  } while (0)

#define MGP_LAUNCH_CHECK(h) MGP_HIP((h), hipGetLastError())

// grow-only arenas; never called during stream capture (callers size up front).  With a fixed
// workspace (mgp_create_ex) an arena that must grow takes a fresh region of the pool (its old one is
// not reused) and the request fails when the pool is exhausted -- the library never allocates then.
inline int mgp_reserve(mgp_handle* h, void** p, size_t* have, size_t need) {
  if (need <= *have) return MGP_OK;
  if (h->pool) {
    const size_t at = (h->pool_used + 255) & ~(size_t)255;
    if (at + need > h->pool_bytes)
      return mgp_fail(h, MGP_E_NOMEM, "fixed workspace exhausted: %zu bytes requested, %zu of %zu in use "
                      "(size it with mgp_workspace_bytes on a growing handle)", need, h->pool_used, h->pool_bytes);
    if (*p) MGP_HIP(h, hipStreamSynchronize(h->stream));  // the old region may still be read by queued work
    *p = (char*)h->pool + at;
    *have = need;
    h->pool_used = at + need;
    return MGP_OK;
  }
  if (*p) {
    MGP_HIP(h, hipStreamSynchronize(h->stream));
    MGP_HIP(h, hipFree(*p));
    *p = nullptr;
    *have = 0;
  }
  size_t want = need + (need >> 2) + 4096;
  hipError_t e = hipMalloc(p, want);
  if (e != hipSuccess) return mgp_fail(h, MGP_E_NOMEM, "workspace hipMalloc(%zu) failed: %s", want,
                                        hipGetErrorString(e));
  *have = want;
  return MGP_OK;
}

// value of `v` in lane `src` (wave-uniform) as a scalar operand: v_readlane, no LDS-pipe traffic
__device__ __forceinline__ double mgp_read_lane(double v, int src) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), src);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ float mgp_read_lane(float v, int src) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src));
}

// sum over the 64 lanes of a wave, the result in every lane: xor butterfly, offsets 32 .. 1
template <typename T>
__device__ __forceinline__ T mgp_wave_sum(T v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// Run-time kernel kind, input dimension and dtype as compile-time constants of a generic lambda: the one place
// where the kind switch and the padded-dimension ladder are written.  f receives std::integral_constant<int, V>
// (read as decltype(arg)::value) or a value of the element type, and returns the entry point's int.
template <typename F>
inline int mgp_with_kind(int kind, F&& f) {
  switch (kind) {
    case MGP_SE: return f(std::integral_constant<int, 0>{});
    case MGP_MATERN12: return f(std::integral_constant<int, 1>{});
    case MGP_MATERN32: return f(std::integral_constant<int, 2>{});
    default: return f(std::integral_constant<int, 3>{});
  }
}
// DP = the smallest of {2, 4, 8, 16, 32} that is >= max(D, MIN_DP); paddings below MIN_DP are not instantiated
template <int MIN_DP = 2, typename F>
inline int mgp_with_dp(int D, F&& f) {
  if constexpr (MIN_DP <= 2)
    if (D <= 2) return f(std::integral_constant<int, 2>{});
  if constexpr (MIN_DP <= 4)
    if (D <= 4) return f(std::integral_constant<int, 4>{});
  if constexpr (MIN_DP <= 8)
    if (D <= 8) return f(std::integral_constant<int, 8>{});
  if constexpr (MIN_DP <= 16)
    if (D <= 16) return f(std::integral_constant<int, 16>{});
  return f(std::integral_constant<int, 32>{});
}
template <typename F>
inline int mgp_with_dtype(int dtype, F&& f) {
  return dtype == MGP_F64 ? f(double{}) : f(float{});
}

int mgp_build_e2tabs(mgp_handle* h);  // sweep.hip
// dense.hip: slots Q[nt][n] (h->ws) and the (I, J) table of the one-RHS upper-triangle product, nt = ceil(n/64);
// Q[k][i] = contribution of chunk k to output element i, summed by the caller in k order
int mgp_symm_gemv_tri_prepare(mgp_handle* h, int dtype, int64_t n, void** Q, const void** tab);

// Where an operator form left A.p for the CG update (dense.hip, cg.hip): {out, 1, 0} when the product was finished into
// the caller's `out`; 2..8 unreduced contraction slices of the skinny product, slice z at src + z * stride; or the
// collective SGPR operator's all-reduced partial in place with the agreement word behind it (`agree`, compared with
// `world`).  Only an entry point handed a non-null MgpApLoc* may leave A.p unfinished; the handle carries no per-call state.
struct MgpApLoc {
  const void* src;
  int slices;
  long stride;
  const void* agree;
  int world;
};

// cg_dense1.hip: up to eight right-hand sides on a dense matrix, two launches per iteration or (n <= 4096) one per solve
struct MgpCgCtrl {
  int active;
  int iters;
  unsigned ticket;  // arrivals of the fused update kernel's workgroups (reset by the last one)
  int pad;
};
struct MgpDense1 {
  int dtype = 0, nt = 0, max_it = 0;
  int64_t n = 0;
  long ntiles = 0;
  const void* A = nullptr;
  const void* dinv = nullptr;
  // Q: the product's slots [bt][nt][n] -- dense.hip's for one right-hand side, a block of the arena for several
  void *V = nullptr, *r = nullptr, *Q = nullptr, *tpart = nullptr, *cpart = nullptr, *scal = nullptr;
  void* pb[2] = {nullptr, nullptr};
  // register-resident form (cg_dense1.hip, round 4): published z, the workgroups' shares of p.Ap, the hand-off flags
  int persist = 0, bt = 1;  // bt: right-hand sides, 1 .. 8
  void *zpub = nullptr, *sync = nullptr, *gran = nullptr;
  const void* tab = nullptr;
  MgpCgCtrl* ctrl = nullptr;
  double thr = 0, min_float = 0;
};
size_t mgp_dense1_bytes(const mgp_handle* h, int dtype, int64_t n, int64_t bt);
bool mgp_dense1_eligible(const mgp_handle* h, int64_t n);
bool mgp_dense1_persist_eligible(const mgp_handle* h, int64_t n, int64_t bt);
int mgp_dense1_begin(mgp_handle* h, MgpDense1* st, int dtype, const void* A, int64_t n, const void* B, const void* av,
                     void* V, void* r, const void* dinv, MgpCgCtrl* ctrl, void* arena, double thr, double min_float,
                     int64_t max_it, int persist, int bt);
int mgp_dense1_persist_run(mgp_handle* h, const MgpDense1* st);
int mgp_dense1_step(mgp_handle* h, const MgpDense1* st, int64_t k);
int mgp_dense1_finish(mgp_handle* h, MgpDense1* st, void* rz, void* err, int* over);

inline size_t mgp_elem(int dtype) { return dtype == MGP_F64 ? 8 : 4; }

inline int mgp_check_kernel(mgp_handle* h, const mgp_kernel* k) {
  if (!h) return MGP_E_BADARG;
  if (!k) return mgp_fail(h, MGP_E_BADARG, "kernel is NULL");
  if (k->kind < MGP_SE || k->kind > MGP_MATERN52) return mgp_fail(h, MGP_E_BADARG, "bad kernel kind %d", k->kind);
  if (k->dtype != MGP_F32 && k->dtype != MGP_F64) return mgp_fail(h, MGP_E_DTYPE, "bad dtype %d", k->dtype);
  if (k->D < 1 || k->D > MGP_MAX_D) return mgp_fail(h, MGP_E_SHAPE, "D=%d outside [1,%d]", k->D, MGP_MAX_D);
  if (!(k->variance > 0.0)) return mgp_fail(h, MGP_E_BADARG, "variance must be > 0");
  for (int d = 0; d < k->D; ++d)
    if (!(k->lengthscales[d] > 0.0)) return mgp_fail(h, MGP_E_BADARG, "lengthscale[%d] must be > 0", d);
  return MGP_OK;
}

// Scaled kernel parameters passed by value to device code.
struct SweepParams {
  double inv_ls[MGP_FUSED_MAX_D];  // c_kind / lengthscale_d (fused kernels only: D <= 32)
  double variance;
  double clamp;  // c_kind^2 * 1e-36
};

inline SweepParams mgp_make_params(const mgp_kernel* k) {
  SweepParams p;
  const double c = mgp_profile_scale(k->kind);
  for (int d = 0; d < MGP_FUSED_MAX_D; ++d) p.inv_ls[d] = d < k->D ? c / k->lengthscales[d] : 0.0;
  p.variance = k->variance;
  p.clamp = c * c * 1e-36;
  return p;
}

// internal cross-TU entry points (layout-generic forms of the public calls)
struct VecView {  // element (i, r) of a batch of vectors lives at base[i*si + r*sr]
  const void* base;
  int64_t si, sr;
};
struct VecViewMut {
  void* base;
  int64_t si, sr;
};
inline VecView mgp_view(const void* p, int64_t n, int64_t R, int layout) {
  return layout == MGP_COLS ? VecView{p, R, 1} : VecView{p, 1, n};
}
inline VecViewMut mgp_view_mut(void* p, int64_t n, int64_t R, int layout) {
  return layout == MGP_COLS ? VecViewMut{p, R, 1} : VecViewMut{p, 1, n};
}

// out(i,r) = variance * sum_j k(a_i, b_j) w(j,r) [+ alpha * addend(i,r)];  gate: device int, skip if 0
int mgp_sweep(mgp_handle* h, const mgp_kernel* k, const void* A, int64_t na, const void* B, int64_t nb,
              VecView W, int32_t R, VecViewMut out, double alpha, VecView addend, const int* gate);
// kxx.hip: out(i,r) = variance * sum_j k(x_i, x_j) v(j,r) + s2 v(i,r), each unordered pair evaluated once
int mgp_kxx(mgp_handle* h, const mgp_kernel* k, const void* X, int64_t N, double s2, VecView V, int32_t R,
            VecViewMut out, const int* gate);
// project.hip: the many-column form of out[Bt, M] = P[Bt, M] (k(Z, Z) + diag lambda), fp64 and D <= MGP_FUSED_MAX_D
// (mgp_kmm_wide_serves).  prepare reserves the prj arena for Bt right-hand sides and packs Z at its front; apply packs
// for itself unless a WideHold names this Z.  gate: device int, every kernel of the route skips if 0
bool mgp_kmm_wide_serves(const mgp_kernel* k);
int mgp_kmm_wide_prepare(mgp_handle* h, const mgp_kernel* k, const void* Z, int64_t M, int64_t Bt, const int* gate);
int mgp_kmm_wide_apply(mgp_handle* h, const mgp_kernel* k, const void* Z, int64_t M, const void* lambda, const void* P,
                       int64_t Bt, void* out, const int* gate);
// kmm_wide_anyd.hip (MGP_OP_KMM_LAMBDA_WIDE_ANYD, include/mgp_sweep_anyd.h): the same operator and the same
// prepare / apply / WideHold protocol at fp64 and D > MGP_FUSED_MAX_D (mgp_kmm_wide_anyd_serves), the distance tiles on
// the matrix cores with K in slices
bool mgp_kmm_wide_anyd_serves(const mgp_kernel* k);
int mgp_kmm_wide_anyd_prepare(mgp_handle* h, const mgp_kernel* k, const void* Z, int64_t M, int64_t Bt, const int* gate);
int mgp_kmm_wide_anyd_apply(mgp_handle* h, const mgp_kernel* k, const void* Z, int64_t M, const void* lambda,
                            const void* P, int64_t Bt, void* out, const int* gate);
// kxx_sym_anyd.hip (MGP_OP_KXX_NOISE_SYM_ANYD, include/mgp.h): out[Bt, N] = P[Bt, N] (k(X, X) + s2 I), each unordered
// pair once on the matrix cores, at fp64 and D > MGP_FUSED_MAX_D (mgp_kxx_sym_anyd_serves); elsewhere mgp_kxx itself.
// prepare reserves the kxx arena for Bt right-hand sides and packs X at its front; the product packs for itself unless
// a SymHold names this X.  gate: device int, every kernel of the route skips if 0
bool mgp_kxx_sym_anyd_serves(const mgp_kernel* k);
int mgp_kxx_sym_anyd_prepare(mgp_handle* h, const mgp_kernel* k, const void* X, int64_t N, int64_t Bt, const int* gate);
int mgp_kxx_sym_anyd(mgp_handle* h, const mgp_kernel* k, const void* X, int64_t N, double s2, const void* P,
                     int64_t Bt, void* out, const int* gate);
// rff_anyd.hip (MGP_RFF_ANYD, include/mgp_pathwise.h): the fused prior sample and its backward pass at fp64,
// MGP_FUSED_MAX_D < D <= MGP_MAX_D and 1 <= S <= 8 (mgp_rff_anyd_serves), on arguments rff.hip / rff_grad.hip have checked
bool mgp_rff_anyd_serves(int dtype, int D, int S);
int mgp_rff_anyd_sample(mgp_handle* h, const double* X, long N, int D, const double* theta, long L, const double* W,
                        int S, double scale, double* out, int layout);
int mgp_rff_anyd_vjp(mgp_handle* h, const double* X, long N, int D, const double* theta, long L, const double* W, int S,
                     double scale, const double* G, long g_sn, long g_ss, double* dtheta, double* dX);
// generic-D forms (generic.hip): explicit panels + NT GEMM, any D <= MGP_MAX_D
int mgp_k_dense_generic(mgp_handle* h, const mgp_kernel* k, const void* A, int64_t na, const void* B, int64_t nb,
                        void* out, int64_t ld, double jitter, const void* diag_add, const int* gate);
int mgp_sweep_generic(mgp_handle* h, const mgp_kernel* k, const void* A, int64_t na, const void* B, int64_t nb,
                      VecView W, int32_t R, VecViewMut out, double alpha, VecView addend, const int* gate);
int mgp_nearest_generic(mgp_handle* h, const mgp_kernel* k, int dist_type, const void* X, int64_t N, const void* Z,
                        int64_t M, int64_t* idx, void* best);
int mgp_k_dense_vjp_generic(mgp_handle* h, const mgp_kernel* k, const void* A, int64_t na, const void* B, int64_t nb,
                            const void* G, int64_t ldg, double* dvariance, double* dlengthscales);
int mgp_kmn_sq_colsum_generic(mgp_handle* h, const mgp_kernel* k, const void* X, int64_t N, const void* Z, int64_t M,
                              void* out);
int mgp_gemm_nt(mgp_handle* h, int dtype, const void* P, int64_t ldp, int64_t m, const void* A, int64_t lda, int64_t n,
                int64_t K, void* out, int64_t ldo, int accumulate, const int* gate);
// sweep_anyd.hip (include/mgp_sweep_anyd.h): mgp_sweep's contract on the matrix cores with K in slices, fp64 and
// D > MGP_FUSED_MAX_D (mgp_sweep_anyd_serves); mgp_sweep_anyd / mgp_kxx_anyd take it where it serves and are mgp_sweep /
// mgp_kxx otherwise
bool mgp_sweep_anyd_serves(const mgp_kernel* k);
int mgp_sweep_fused_anyd(mgp_handle* h, const mgp_kernel* k, const void* A, int64_t na, const void* B, int64_t nb,
                         VecView W, int32_t R, VecViewMut out, double alpha, VecView addend, const int* gate);
int mgp_sweep_anyd(mgp_handle* h, const mgp_kernel* k, const void* A, int64_t na, const void* B, int64_t nb, VecView W,
                   int32_t R, VecViewMut out, double alpha, VecView addend, const int* gate);
int mgp_kxx_anyd(mgp_handle* h, const mgp_kernel* k, const void* X, int64_t N, double s2, VecView V, int32_t R,
                 VecViewMut out, const int* gate);
int mgp_sweep_mfma_f64(mgp_handle* h, const mgp_kernel* k, const double* A, long na, const double* B, long nb,
                       const double* W, long w_sj, long w_sr, int R, double* out, long o_si, long o_sr,
                       double alpha, const double* addend, long ad_si, long ad_sr, const int* gate);
int mgp_syrk_nt_upper(mgp_handle* h, int dtype, const void* Kt, int64_t n, int64_t K, int64_t ld, void* out,
                      int accumulate, int nz, const int* tile_tab, int ntiles);
int mgp_mirror_upper(mgp_handle* h, int dtype, void* out, const void* slices, int nz, int64_t n, double scale);
int mgp_symm_gemv_assign(mgp_handle* h, int dtype, const void* A, int64_t n, const void* p, void* out, const int* gate);
int mgp_symm_gemv_rows_acc(mgp_handle* h, int dtype, const void* A, int64_t n, const void* p, int64_t rb, int64_t re,
                           double alpha, void* out, const int* gate, void* word = nullptr);
// comm.hip: the operator's all-reduce on the handle's stream (errors land in the handle)
int mgp_comm_allreduce_on(mgp_handle* h, mgp_comm* comm, void* buf, size_t count, int dtype);
int mgp_symm_matmul_gated(mgp_handle* h, int dtype, const void* A, int64_t n, const void* P, int64_t Bt,
                          void* out, const int* gate, MgpApLoc* loc = nullptr);
// pivchol.hip: Z[Bt, n] = diag_inv o R - (R B^T) B, B [k, n]; gate: device int, skip if 0
int mgp_lowrank_apply_gated(mgp_handle* h, int dtype, const void* diag_inv, const void* B, int64_t k, int64_t n,
                            const void* R, int64_t Bt, void* Z, const int* gate);
// the many-column form (MGP_PRE_LOWRANK_WIDE): groups of at most 256 rows of R, both products on the fp64 matrix cores;
// fp32 takes the code above
int mgp_lowrank_wide_apply_gated(mgp_handle* h, int dtype, const void* diag_inv, const void* B, int64_t k, int64_t n,
                                 const void* R, int64_t Bt, void* Z, const int* gate);

// kmn_grad.hip, shared with kmn_grad_generic.hip (include/mgp_anyd.h).  mgp_kvjp_check: the argument checks of
// mgp_kmn_knm_vjp with the largest D the caller serves; zeroes the host outputs, handles N = 0 (*done = 1: nothing is
// left to do).  mgp_kvjp_fused_d: the D <= MGP_FUSED_MAX_D implementation on checked arguments; panel_rows = 0 is the
// 256 MiB rule (64 MiB of pack on the fused rank-P form), > 0 that many rows per panel.  mgp_kvjp_symmetrize:
// G2 = Gq + Gq^T, exactly symmetric.
int mgp_kvjp_check(mgp_handle* h, const mgp_kernel* k, const void* X, int64_t N, const void* Z, int64_t M,
                   const void* Gq, const void* Y, const void* Gb, int32_t P, int max_d, double* dvariance,
                   double* dlengthscales, void* dZ, int* done);
int mgp_kvjp_fused_d(mgp_handle* h, const mgp_kernel* k, const double* X, long N, const double* Z, long M,
                     const double* Gq, const double* Y, const double* Gb, int P, long panel_rows, double* dvariance,
                     double* dlengthscales, double* dZ);
int mgp_kvjp_symmetrize(mgp_handle* h, const double* Gq, long M, double* G2);

// Host tail of a kernel-block VJP.  part [nblocks][width] on the device holds per-workgroup sums: width - 1
// lengthscale sums (the first k->D count), then the variance sum.  They are copied to the host and added in block
// order (deterministic), then *dvar = tot[width - 1] and dls[d] = variance (-2 / l_d) tot[d].  carry [width], when
// given, holds the running sums: they continue from it and are left in it, so a caller that launches in several
// groups (kxx_grad.hip's right-hand-side groups) gets one sum over all blocks of all groups, scaled once.
// Synchronises the stream.
inline int mgp_fold_vjp_partials(mgp_handle* h, const double* part, long nblocks, int width, const mgp_kernel* k,
                                 double* dvar, double* dls, double* carry = nullptr) {
  std::vector<double> host((size_t)nblocks * width), own(carry ? 0 : width, 0.0);
  MGP_HIP(h, hipMemcpyAsync(host.data(), part, host.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  MGP_HIP(h, hipStreamSynchronize(h->stream));
  double* tot = carry ? carry : own.data();
  for (long b = 0; b < nblocks; ++b)
    for (int d = 0; d < width; ++d) tot[d] += host[(size_t)b * width + d];
  *dvar = tot[width - 1];  // sum G f == sum G k / variance
  for (int d = 0; d < k->D; ++d) dls[d] = k->variance * (-2.0 / k->lengthscales[d]) * tot[d];
  return MGP_OK;
}
