"""Which launches a fixed-step CG solve on a dense matrix takes, and the cases that reach each of them.

Two rules of the library are restated here (host arithmetic only, no torch, no library):

* the tier rule of the fused update kernel (csrc/cg.hip, `kFusedTiers`): (elements per thread, threads) by n,
  and the block size of the generic update kernel (256 threads per right-hand side up to n = 8192, 1024 beyond);
* the slice rule of the skinny product (csrc/dense.hip, `symm_skinny_lds_launch`): how many contraction slices
  A.p is computed in.  2..8 slices are left for the fused update to add (`MgpApLoc`), 1 goes straight to the
  output, more than 8 are added by a launch of their own.

tests/test_cg_route_plan.py checks on the CPU that CASES reaches every tier on both sides of its edge, a deferred
and a reduced product in each thread-count family, both block sizes and all six modes of the generic update kernel;
tests/test_gpu_cg_routes.py runs the cases against oracle/cg.py.  Every case has more right-hand sides than the
tile scheme of csrc/cg_dense1.hip takes (8), a preconditioner it does not take, or is a recording solve.

The cases stop before any breakdown guard fires.  tests/guard_plan.py holds the systems and cases on which they do fire
(columns frozen from step 0, frozen after converging beside live ones, either guard alone, other floors) for the same
kernel sites and for the forms of csrc/cg_dense1.hip.
"""

from collections import namedtuple

import numpy as np

from switch_forms import NUM_CUS

# (largest n, elements per thread, threads)
FUSED_TIERS = [(256, 1, 256), (512, 2, 256), (1024, 1, 1024), (2048, 2, 1024), (4096, 4, 1024), (8192, 8, 1024)]
FUSED_MAX_N = FUSED_TIERS[-1][0]
DENSE1_MAX_COLS = 8  # the most right-hand sides the tile scheme ever takes (MGP_CG_DENSE1_COLS)


def fused_tier(n):
    """(EPT, NT) of cg_update_fused_kernel for n, None beyond the last tier."""
    for top, ept, nt in FUSED_TIERS:
        if n <= top:
            return ept, nt
    return None


def update_threads(n):
    """Block size of cg_update_kernel."""
    return 1024 if n > 8192 else 256


def skinny_slices(n, Bt, esize=8, num_cus=NUM_CUS):
    """Contraction slices of the LDS-staged skinny product, 2 <= Bt <= 128 (default switches)."""
    assert 2 <= Bt <= 128
    nbt = 1 if Bt <= 16 else 2 if Bt <= 32 else 4 if Bt <= 64 else 8
    kw = 64 if nbt * 16 * 64 * 2 * esize <= 65536 else 32
    jg = -(-n // 64)
    bpc = 2 if nbt <= 1 else 1
    ks = max(1, min(16, bpc * num_cus // jg))
    kr_len = -(-(-(-n // ks)) // kw) * kw
    return -(-n // kr_len)


def deferred(ks):
    """The product leaves its slices for the fused update."""
    return 2 <= ks <= 8


class Case(namedtuple("Case", "id n Bt k cycle pre start dtype record note")):
    """pre: eye | jacobi | block | dense; start: zero | v0; cycle None = longer than the solve (no refresh)."""

    def __repr__(self):
        return self.id

    @property
    def max_steps_cycle(self):
        return self.k + 1 if self.cycle is None else self.cycle

    @property
    def resets(self):
        c = self.max_steps_cycle
        return [i for i in range(self.k) if i % c == c - 1]

    @property
    def fused(self):
        """cg_update_fused_kernel serves the steps without a refresh."""
        return self.pre in ("eye", "jacobi") and self.n <= FUSED_MAX_N

    @property
    def takes_dense1(self):
        """Necessary conditions of the tile scheme (csrc/cg.hip, pcg_solve_t); its size rule is left out, so this
        errs on the side of saying yes."""
        return (self.Bt <= DENSE1_MAX_COLS and self.pre in ("eye", "jacobi") and self.cycle is None
                and not self.record)

    @property
    def modes(self):
        """Modes of cg_update_kernel the solve launches."""
        out = set()
        plain = [i for i in range(self.k) if i not in self.resets]
        if self.pre == "dense":
            out.add(5)  # start-up
            if plain:
                out |= {3, 4}
            if self.resets:
                out |= {1, 5}
        else:
            if plain and not self.fused:
                out.add(0)
            if self.resets:
                out |= {1, 2}
        return out

    @property
    def slices(self):
        return skinny_slices(self.n, self.Bt, 8 if self.dtype == "f64" else 4)


def _case(id, n, pre="eye", Bt=9, k=5, cycle=None, start="zero", dtype="f64", record=False, note=""):
    return Case(id, n, Bt, k, cycle, pre, start, dtype, record, note)


FUSED_N = [64, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4096, 4097, 8192]  # 64: one slice in the 256-thread family
CASES = []
for _n in FUSED_N:
    for _pre in ("eye", "jacobi"):
        CASES.append(_case(f"fused-{_n}-{_pre}", _n, _pre))
# generic update kernel at 1024 threads, and the block preconditioner at both block sizes
CASES += [_case("generic-8193-eye", 8193), _case("generic-8193-jacobi", 8193, "jacobi"),
          _case("block-512", 512, "block"), _case("block-8200", 8200, "block")]
# residual refresh on steps 1 and 3 from a non-zero start
CASES += [_case("refresh-257", 257, "eye", cycle=2, start="v0"), _case("refresh-2049", 2049, "jacobi", cycle=2, start="v0"),
          _case("refresh-8193", 8193, "jacobi", cycle=2, start="v0")]
# z from outside the update kernels: Pinv = I / 2 + W W^T / n (any cheap SPD matrix, not an inverse)
CASES += [_case(f"dense-{_n}-{'refresh' if _c else 'plain'}", _n, "dense", Bt=3, cycle=_c)
          for _n in (333, 8200) for _c in (None, 2)]
CASES += [_case("record-513", 513, record=True)]
# fp32: one case per (EPT, NT) pair up to n = 2049, three steps.  The bar of a case is four times the distance of
# oracle/cg.py on float32 copies from its own float64 run (both sum in trees, in different orders); `note` holds that
# distance as measured once with numpy's pairwise sums: (iterate, relative to its largest entry; 0.5 rz, relative)
CASES += [_case("f32-250", 250, "eye", k=3, dtype="f32", note=(6.4e-07, 6.6e-07)),
          _case("f32-512", 512, "jacobi", k=3, dtype="f32", note=(7.0e-07, 5.3e-06)),
          _case("f32-1023", 1023, "eye", k=3, dtype="f32", note=(7.7e-07, 2.4e-06)),
          _case("f32-2048", 2048, "jacobi", k=3, dtype="f32", note=(8.5e-07, 1.5e-05)),
          _case("f32-2049", 2049, "eye", k=3, dtype="f32", note=(9.8e-07, 1.7e-06))]


# ---------------------------------------------------------------- the systems
def matrix(n):
    """A = 2 I + U U^T / n, U [n, 32] standard normal, seeded by n."""
    U = np.random.default_rng(n).standard_normal((n, 32))
    A = U @ U.T / n
    A[np.diag_indices(n)] += 2.0
    return A


def rhs(case):
    return np.random.default_rng(10 ** 6 + case.n).standard_normal((case.Bt, case.n))


def start(case):
    if case.start == "zero":
        return np.zeros((case.Bt, case.n))
    return 0.1 * np.random.default_rng(2 * 10 ** 6 + case.n).standard_normal((case.Bt, case.n))


def block_indices(n):
    """Three blocks of eight indices scattered over [0, n)."""
    return np.sort(np.random.default_rng(3 * 10 ** 6 + n).permutation(n)[:24]).reshape(8, 3).T.copy()


def dense_pinv(n):
    W = np.random.default_rng(4 * 10 ** 6 + n).standard_normal((n, 16))
    P = W @ W.T / n
    P[np.diag_indices(n)] += 0.5
    return P
