// sweep_anyd.hip -- fp64 fused kernel products at any input dimension MGP_FUSED_MAX_D < D <= MGP_MAX_D.
//
// Same contract as sweep.hip:  out(i,r) = variance * sum_j k(a_i, b_j) w(j,r) [+ alpha*addend(i,r)].
// As in sweep_mfma.hip a 16x16 tile of  -s_ij = 2 a_i.b_j - |a_i|^2 - |b_j|^2  comes out of
// v_mfma_f64_16x16x4_f64 by augmenting the K dimension:
//     A row (owned point)    = [ a_1 .. a_D,  |a|^2,  1,      0.. ]
//     B col (streamed point) = [2b_1 .. 2b_D, -1,    -|b|^2,  0.. ]      K = 4*KS >= D + 2,  a = x c / l
// but K no longer fits in registers: it is walked in slices of kKSL k-steps (32 columns), GEMM style.  A workgroup
// owns kOwn = 128 rows (4 waves x 2 row tiles of 16) and streams tiles of kTile = 64 points (4 column tiles); every
// wave keeps its 2 x 4 accumulator tiles (Acc4) across the slices of a streamed tile, k ascending, and applies the
// profile only after the last slice.  Per slice the streamed fragments go through LDS already in MFMA fragment order
// (frag[(jt*kKSL + ks)*64 + lane]: one conflict-free ds_read_b64 per lane), staged by the wave of that column tile;
// the owned fragments are used by one wave only and are loaded by it straight into registers (16 rows x 32 bytes per
// load: Z, or one tile of X, stays in L2).  |a|^2 and |b|^2 are fma chains over d ascending, taken once per call by
// a kernel of their own.
//
// Column passes: R goes in passes of 8, 4, 2, 1 columns (the ladder of sweep_rc).  Chunk rule: that of launch_mfma
// with this file's tile sizes: nblk = ceil(na / 128); one chunk when nblk >= 4 CUs, else ceil(8 CUs / nblk) chunks,
// at most ceil(nb / 64); a chunk is a multiple of 64 streamed points.  Chunk partials [chunk][r][i] are added in
// chunk order by a second kernel; the 16 lanes of a row are summed by xor-shuffles: no atomics anywhere.
// Padding: owned rows past na repeat row na - 1 and are never stored; streamed slots past the chunk end are exact
// zeros in every fragment and every multiplier (profile(0) * 0 = 0), whatever lies in memory behind W, A or B.
//
// Scratch: the ws arena alone,
//     bytes = 8 * (na + nb + (nchunks > 1 ? nchunks * na * RC0 : 0)),   RC0 = the widest pass = largest of 8, 4, 2, 1 <= R
// (squared norms of the owned and of the streamed points, then the partials).  The gen arena is never touched.  The
// scaled inverse lengthscales c / l_d live in a 4 KB buffer of the handle (mgp_create), uploaded when they change.
#include "../../include/mgp_sweep_anyd.h"
#include "mgp_common.h"

namespace {

using Acc4 = __attribute__((ext_vector_type(4))) double;

constexpr int kThreadsA = 256;
constexpr int kTRa = 2;                // 16-row tiles owned by one wave
constexpr int kOwn = 4 * kTRa * 16;    // owned points per workgroup
constexpr int kNJT = 4;                // 16-column tiles per streamed tile: one per wave to stage
constexpr int kTile = kNJT * 16;       // streamed points per LDS tile
constexpr int kKSL = 8;                // k-steps of 4 per K slice

// nrm[i] = sum_d (p_id * sc_d)^2, d ascending
__global__ __launch_bounds__(256) void anyd_sqnorm_kernel(const double* __restrict__ P, long n, int D,
                                                          const double* __restrict__ sc, double* __restrict__ nrm,
                                                          const int* __restrict__ gate) {
  if (gate != nullptr && *gate == 0) return;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double s = 0;
  for (int d = 0; d < D; ++d) {
    const double v = P[i * D + d] * sc[d];
    s = mgp_fma(v, v, s);
  }
  nrm[i] = s;
}

template <int KIND, int RC>
__global__ __launch_bounds__(kThreadsA, RC <= 4 ? 2 : 1) void sweep_anyd_kernel(
    const double* __restrict__ A, long na, const double* __restrict__ nrmA, const double* __restrict__ B, long nb,
    const double* __restrict__ nrmB, long b_chunk, const double* __restrict__ W, long w_sj, long w_sr,
    double* __restrict__ out, long o_si, long o_sr, long o_chunk, int D, const double* __restrict__ sc, double variance,
    double clamp, double alpha, const double* __restrict__ addend, long ad_si, long ad_sr,
    const int* __restrict__ gate) {
  if (gate != nullptr && *gate == 0) return;
  __shared__ __attribute__((aligned(16))) double frag[kNJT * kKSL * 64];  // one K slice of the streamed tile
  __shared__ __attribute__((aligned(16))) double wl[kTile * RC];         // multipliers of the streamed tile
  __shared__ double e2tab[MGP_EXP2_TAB_SIZE];                             // 2^(i/2048) for mgp_exp2_tab
  static_assert(kNJT * 64 == kThreadsA, "one wave stages one column tile");

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int l15 = lane & 15, kq = lane >> 4;
  const long base = (long)blockIdx.x * kOwn;
  for (int e = t; e < MGP_EXP2_TAB_SIZE; e += kThreadsA) e2tab[e] = mgp_exp2_tab_entry(e);
  const E2Tab<true> e2{e2tab};

  const int KS = (D + 2 + 3) >> 2;  // k-steps in all
  // the row of each owned tile this lane loads fragments of (rows past na repeat the last one; never stored)
  const double* arow[kTRa];
  double anrm[kTRa];
#pragma unroll
  for (int tr = 0; tr < kTRa; ++tr) {
    long i = base + (wave * kTRa + tr) * 16 + l15;
    if (i >= na) i = na - 1;
    arow[tr] = A + i * D;
    anrm[tr] = nrmA[i];
  }

  double acc[kTRa][4][RC];
#pragma unroll
  for (int tr = 0; tr < kTRa; ++tr)
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4)
#pragma unroll
      for (int r = 0; r < RC; ++r) acc[tr][r4][r] = 0.0;

  const long jb = (long)blockIdx.y * b_chunk;
  const long je = (jb + b_chunk < nb) ? jb + b_chunk : nb;

  for (long j0 = jb; j0 < je; j0 += kTile) {
    Acc4 c[kTRa][kNJT];
#pragma unroll
    for (int tr = 0; tr < kTRa; ++tr)
#pragma unroll
      for (int jt = 0; jt < kNJT; ++jt) c[tr][jt] = Acc4{0, 0, 0, 0};
    // the streamed point this lane stages fragments of: column tile `wave`, column l15
    const long js = j0 + wave * 16 + l15;
    const bool jlive = js < je;
    const double* brow = B + (jlive ? js : jb) * D;
    const double bnrm = jlive ? nrmB[js] : 0.0;

    for (int s0 = 0; s0 < KS; s0 += kKSL) {
      const int nks = KS - s0 < kKSL ? KS - s0 : kKSL;  // k-steps of this slice (wave-uniform)
      double af[kTRa][kKSL];
#pragma unroll
      for (int ks = 0; ks < kKSL; ++ks) {
        if (ks < nks) {
          const int k = 4 * (s0 + ks) + kq;
          const double scale = k < D ? sc[k] : 0.0;
#pragma unroll
          for (int tr = 0; tr < kTRa; ++tr)
            af[tr][ks] = k < D ? arow[tr][k] * scale : (k == D ? anrm[tr] : (k == D + 1 ? 1.0 : 0.0));
        } else {
#pragma unroll
          for (int tr = 0; tr < kTRa; ++tr) af[tr][ks] = 0.0;
        }
      }
      __syncthreads();  // the previous slice's fragments (and the previous tile's multipliers) fully consumed
#pragma unroll
      for (int ks = 0; ks < kKSL; ++ks) {
        if (ks < nks) {
          const int k = 4 * (s0 + ks) + kq;
          double v = 0.0;
          if (jlive) {
            if (k < D) {
              const double x = brow[k] * sc[k];
              v = x + x;
            } else {
              v = k == D ? -1.0 : (k == D + 1 ? -bnrm : 0.0);
            }
          }
          frag[(wave * kKSL + ks) * 64 + lane] = v;
        }
      }
      if (s0 == 0 && t < kTile) {
        const long jw = j0 + t;
#pragma unroll
        for (int r = 0; r < RC; ++r) wl[t * RC + r] = jw < je ? W[jw * w_sj + r * w_sr] : 0.0;
      }
      __syncthreads();
#pragma unroll
      for (int jt = 0; jt < kNJT; ++jt)
#pragma unroll
        for (int ks = 0; ks < kKSL; ++ks)
          if (ks < nks) {
            const double bf = frag[(jt * kKSL + ks) * 64 + lane];
#pragma unroll
            for (int tr = 0; tr < kTRa; ++tr)
              c[tr][jt] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[tr][ks], bf, c[tr][jt], 0, 0, 0);
          }
    }

    // ---- the profile, once per pair, and the RC accumulate fmas
#pragma unroll
    for (int jt = 0; jt < kNJT; ++jt) {
      double w[RC];
#pragma unroll
      for (int r = 0; r < RC; ++r) w[r] = wl[(jt * 16 + l15) * RC + r];
#pragma unroll
      for (int tr = 0; tr < kTRa; ++tr)
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
          const double kv = mgp_profile<KIND, double, E2Tab<true>>(c[tr][jt][r4], clamp, e2);
#pragma unroll
          for (int r = 0; r < RC; ++r) acc[tr][r4][r] = mgp_fma(kv, w[r], acc[tr][r4][r]);
        }
    }
  }

  // ---- epilogue: sum the 16 lanes (columns) of every owned row, lane (l & 15) == 0 stores
  double* o = out + (long)blockIdx.y * o_chunk;
#pragma unroll
  for (int tr = 0; tr < kTRa; ++tr)
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4)
#pragma unroll
      for (int r = 0; r < RC; ++r) {
        double v = acc[tr][r4][r];
        v += __shfl_xor(v, 1, 64);
        v += __shfl_xor(v, 2, 64);
        v += __shfl_xor(v, 4, 64);
        v += __shfl_xor(v, 8, 64);
        const long i = base + (wave * kTRa + tr) * 16 + kq + 4 * r4;
        if (l15 == 0 && i < na) {
          v *= variance;
          if (addend != nullptr) v = mgp_fma(alpha, addend[i * ad_si + r * ad_sr], v);
          o[i * o_si + r * o_sr] = v;
        }
      }
}

// out(i, r) = sum_c part[c][r][i] (+ alpha * addend), c ascending
__global__ __launch_bounds__(256) void anyd_reduce_partials_kernel(const double* __restrict__ part, long na, int R,
                                                                   int nchunks, double* __restrict__ out, long o_si,
                                                                   long o_sr, double alpha,
                                                                   const double* __restrict__ addend, long ad_si,
                                                                   long ad_sr, const int* __restrict__ gate) {
  if (gate != nullptr && *gate == 0) return;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= na * R) return;
  const long r = idx / na, i = idx - r * na;
  double s = 0;
  const long stride = na * R;
  for (int c = 0; c < nchunks; ++c) s += part[(long)c * stride + idx];
  if (addend != nullptr) s = mgp_fma(alpha, addend[i * ad_si + r * ad_sr], s);
  out[i * o_si + r * o_sr] = s;
}

// out(i, r) = alpha * addend(i, r) (or 0): the product over an empty streamed set, as mgp_sweep gives it
__global__ __launch_bounds__(256) void anyd_empty_sum_kernel(double* __restrict__ out, long o_si, long o_sr, long na,
                                                             int R, double alpha, const double* __restrict__ addend,
                                                             long ad_si, long ad_sr, const int* __restrict__ gate) {
  if (gate != nullptr && *gate == 0) return;
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= na * R) return;
  const long i = e / R, r = e - i * R;
  out[i * o_si + r * o_sr] = addend != nullptr ? alpha * addend[i * ad_si + r * ad_sr] : 0.0;
}

struct AnydPlan {
  long nblk, nchunks, b_chunk;
};

// the chunk rule of the header comment
AnydPlan anyd_plan(long na, long nb, int num_cus) {
  AnydPlan p;
  p.nblk = (na + kOwn - 1) / kOwn;
  const long target = 8L * num_cus;
  long nchunks = p.nblk >= 4L * num_cus ? 1 : (target + p.nblk - 1) / p.nblk;
  const long max_chunks = (nb + kTile - 1) / kTile;
  if (nchunks > max_chunks) nchunks = max_chunks;
  if (nchunks < 1) nchunks = 1;
  long b_chunk = (nb + nchunks - 1) / nchunks;
  b_chunk = (b_chunk + kTile - 1) / kTile * kTile;
  p.b_chunk = b_chunk;
  p.nchunks = (nb + b_chunk - 1) / b_chunk;
  return p;
}

int anyd_widest_pass(int R) { return R >= 8 ? 8 : (R >= 4 ? 4 : (R >= 2 ? 2 : 1)); }

// c / l_d on the device: uploaded when the kernel's scales differ from the ones already there
int anyd_upload_scales(mgp_handle* h, const mgp_kernel* k) {
  const double c = mgp_profile_scale(k->kind);
  double host[MGP_MAX_D];
  for (int d = 0; d < k->D; ++d) host[d] = c / k->lengthscales[d];
  if (h->anyd_sc_n == k->D && memcmp(host, h->anyd_sc_host, (size_t)k->D * sizeof(double)) == 0) return MGP_OK;
  h->anyd_sc_n = 0;
  memcpy(h->anyd_sc_host, host, (size_t)k->D * sizeof(double));
  // stream-ordered behind the launches that read the old scales; anyd_sc_host may change again on the next call
  MGP_HIP(h, hipMemcpyAsync(h->anyd_sc, h->anyd_sc_host, (size_t)k->D * sizeof(double), hipMemcpyHostToDevice, h->stream));
  MGP_HIP(h, hipStreamSynchronize(h->stream));
  h->anyd_sc_n = k->D;
  return MGP_OK;
}

template <int KIND, int RC>
int launch_anyd(mgp_handle* h, const mgp_kernel* k, const AnydPlan& pl, const double* A, long na, const double* nrmA,
                const double* B, long nb, const double* nrmB, double* part, const double* W, long w_sj, long w_sr,
                double* out, long o_si, long o_sr, double alpha, const double* addend, long ad_si, long ad_sr,
                const int* gate) {
  const double c = mgp_profile_scale(k->kind);
  const double clamp = c * c * 1e-36;
  dim3 grid((unsigned)pl.nblk, (unsigned)pl.nchunks);
  if (pl.nchunks == 1) {
    hipEvent_t stop = mgp_prof_begin(h);
    hipLaunchKernelGGL((sweep_anyd_kernel<KIND, RC>), grid, dim3(kThreadsA), 0, h->stream, A, na, nrmA, B, nb, nrmB,
                       pl.b_chunk, W, w_sj, w_sr, out, o_si, o_sr, 0L, k->D, (const double*)h->anyd_sc, k->variance,
                       clamp, alpha, addend, ad_si, ad_sr, gate);
    mgp_prof_end(h, stop);
    MGP_LAUNCH_CHECK(h);
    return MGP_OK;
  }
  hipEvent_t stop = mgp_prof_begin(h);
  hipLaunchKernelGGL((sweep_anyd_kernel<KIND, RC>), grid, dim3(kThreadsA), 0, h->stream, A, na, nrmA, B, nb, nrmB,
                     pl.b_chunk, W, w_sj, w_sr, part, 1L, na, na * (long)RC, k->D, (const double*)h->anyd_sc,
                     k->variance, clamp, 0.0, (const double*)nullptr, 0L, 0L, gate);
  mgp_prof_end(h, stop);
  MGP_LAUNCH_CHECK(h);
  const long tot = na * RC;
  hipLaunchKernelGGL(anyd_reduce_partials_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, h->stream,
                     (const double*)part, na, RC, (int)pl.nchunks, out, o_si, o_sr, alpha, addend, ad_si, ad_sr, gate);
  MGP_LAUNCH_CHECK(h);
  return MGP_OK;
}

template <int KIND>
int anyd_rc(mgp_handle* h, const mgp_kernel* k, const double* A, long na, const double* B, long nb, const double* W,
            long w_sj, long w_sr, int R, double* out, long o_si, long o_sr, double alpha, const double* addend,
            long ad_si, long ad_sr, const int* gate) {
  const AnydPlan pl = anyd_plan(na, nb, h->num_cus);
  if (pl.nchunks > 65535) return mgp_fail(h, MGP_E_SHAPE, "sweep_anyd: too many chunks");
  if (pl.nblk > 2147483647L) return mgp_fail(h, MGP_E_SHAPE, "sweep_anyd: grid too large");
  const size_t need = ((size_t)na + (size_t)nb +
                       (pl.nchunks > 1 ? (size_t)pl.nchunks * na * anyd_widest_pass(R) : (size_t)0)) * sizeof(double);
  MGP_TRY(mgp_reserve(h, &h->ws, &h->ws_bytes, need));
  double* nrmA = (double*)h->ws;
  double* nrmB = nrmA + na;
  double* part = nrmB + nb;
  const double* sc = (const double*)h->anyd_sc;
  hipLaunchKernelGGL(anyd_sqnorm_kernel, dim3((unsigned)((na + 255) / 256)), dim3(256), 0, h->stream, A, na, k->D, sc,
                     nrmA, gate);
  MGP_LAUNCH_CHECK(h);
  hipLaunchKernelGGL(anyd_sqnorm_kernel, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, h->stream, B, nb, k->D, sc,
                     nrmB, gate);
  MGP_LAUNCH_CHECK(h);
  int r0 = 0;
  while (r0 < R) {
    const int left = R - r0;
    const double* Wr = W + (long)r0 * w_sr;
    double* outr = out + (long)r0 * o_sr;
    const double* adr = addend ? addend + (long)r0 * ad_sr : nullptr;
#define MGP_ANYD_PASS(RCV)                                                                                          \
  MGP_TRY((launch_anyd<KIND, RCV>(h, k, pl, A, na, nrmA, B, nb, nrmB, part, Wr, w_sj, w_sr, outr, o_si, o_sr, alpha, \
                                  adr, ad_si, ad_sr, gate)))
    const int rc = anyd_widest_pass(left);
    if (rc == 8) {
      MGP_ANYD_PASS(8);
    } else if (rc == 4) {
      MGP_ANYD_PASS(4);
    } else if (rc == 2) {
      MGP_ANYD_PASS(2);
    } else {
      MGP_ANYD_PASS(1);
    }
#undef MGP_ANYD_PASS
    r0 += rc;
  }
  return MGP_OK;
}

}  // namespace

// mgp_sweep's contract (sweep.hip), fp64 and MGP_FUSED_MAX_D < D <= MGP_MAX_D only
int mgp_sweep_fused_anyd(mgp_handle* h, const mgp_kernel* k, const void* A, int64_t na, const void* B, int64_t nb,
                         VecView W, int32_t R, VecViewMut out, double alpha, VecView addend, const int* gate) {
  MGP_TRY(mgp_check_kernel(h, k));
  if (k->dtype != MGP_F64) return mgp_fail(h, MGP_E_DTYPE, "sweep_anyd: fp64 only");
  if (k->D <= MGP_FUSED_MAX_D) return mgp_fail(h, MGP_E_SHAPE, "sweep_anyd: D=%d is served by the fused sweeps", k->D);
  if (na < 0 || nb < 0 || R < 0) return mgp_fail(h, MGP_E_SHAPE, "negative size");
  if (na == 0 || R == 0) return MGP_OK;
  if (!A || !out.base || (nb > 0 && (!B || !W.base))) return mgp_fail(h, MGP_E_BADARG, "NULL data pointer");
  if (nb == 0) {
    const long tot = (long)na * R;
    hipLaunchKernelGGL(anyd_empty_sum_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, h->stream,
                       (double*)out.base, out.si, out.sr, (long)na, R, alpha, (const double*)addend.base, addend.si,
                       addend.sr, gate);
    MGP_LAUNCH_CHECK(h);
    return MGP_OK;
  }
  MGP_TRY(anyd_upload_scales(h, k));
  return mgp_with_kind(k->kind, [&](auto kind) {
    return anyd_rc<decltype(kind)::value>(h, k, (const double*)A, na, (const double*)B, nb, (const double*)W.base,
                                          W.si, W.sr, R, (double*)out.base, out.si, out.sr, alpha,
                                          (const double*)addend.base, addend.si, addend.sr, gate);
  });
}

bool mgp_sweep_anyd_serves(const mgp_kernel* k) {
  return k != nullptr && k->dtype == MGP_F64 && k->D > MGP_FUSED_MAX_D;
}

// the sweep of the *_anyd names and kinds: the fused kernel where it serves, else exactly mgp_sweep
int mgp_sweep_anyd(mgp_handle* h, const mgp_kernel* k, const void* A, int64_t na, const void* B, int64_t nb, VecView W,
                   int32_t R, VecViewMut out, double alpha, VecView addend, const int* gate) {
  if (mgp_sweep_anyd_serves(k)) return mgp_sweep_fused_anyd(h, k, A, na, B, nb, W, R, out, alpha, addend, gate);
  return mgp_sweep(h, k, A, na, B, nb, W, R, out, alpha, addend, gate);
}

// (k(X, X) + s2 I) V: mgp_kxx's checks; the fused sweep with s2 V as its addend where it serves, else mgp_kxx itself
int mgp_kxx_anyd(mgp_handle* h, const mgp_kernel* k, const void* X, int64_t N, double s2, VecView V, int32_t R,
                 VecViewMut out, const int* gate) {
  if (!mgp_sweep_anyd_serves(k)) return mgp_kxx(h, k, X, N, s2, V, R, out, gate);
  MGP_TRY(mgp_check_kernel(h, k));
  if (N < 0 || R < 0) return mgp_fail(h, MGP_E_SHAPE, "negative size");
  if (N == 0 || R == 0) return MGP_OK;
  if (!X || !V.base || !out.base) return mgp_fail(h, MGP_E_BADARG, "NULL data pointer");
  if (!(s2 >= 0.0)) return mgp_fail(h, MGP_E_BADARG, "s2 must be >= 0");
  return mgp_sweep_fused_anyd(h, k, X, N, X, N, V, R, out, s2, V, gate);
}

extern "C" int mgp_knm_matvec_anyd(mgp_handle* h, const mgp_kernel* k, const void* X, int64_t N, const void* Z,
                                   int64_t M, const void* V, int32_t R, int v_layout, void* out, int out_layout) {
  if (!h) return MGP_E_BADARG;
  return mgp_sweep_anyd(h, k, X, N, Z, M, mgp_view(V, M, R, v_layout), R, mgp_view_mut(out, N, R, out_layout), 0.0,
                        VecView{nullptr, 0, 0}, nullptr);
}

extern "C" int mgp_kmn_matvec_anyd(mgp_handle* h, const mgp_kernel* k, const void* X, int64_t N, const void* Z,
                                   int64_t M, const void* W, int32_t R, int w_layout, void* out, int out_layout) {
  if (!h) return MGP_E_BADARG;
  return mgp_sweep_anyd(h, k, Z, M, X, N, mgp_view(W, N, R, w_layout), R, mgp_view_mut(out, M, R, out_layout), 0.0,
                        VecView{nullptr, 0, 0}, nullptr);
}

extern "C" int mgp_kxx_matvec_anyd(mgp_handle* h, const mgp_kernel* k, const void* X, int64_t N, double s2,
                                   const void* V, int32_t R, int v_layout, void* out, int out_layout) {
  if (!h) return MGP_E_BADARG;
  if ((v_layout != MGP_COLS && v_layout != MGP_ROWS) || (out_layout != MGP_COLS && out_layout != MGP_ROWS))
    return mgp_fail(h, MGP_E_BADARG, "bad layout");
  return mgp_kxx_anyd(h, k, X, N, s2, mgp_view(V, N, R, v_layout), R, mgp_view_mut(out, N, R, out_layout), nullptr);
}
