"""`mgp_rff_sample_vjp` (csrc/rff_grad.hip, include/mgp_pathwise.h) against the long-double reference of
tests/rff_vjp_reference.py.

Bound (the header states it; `rff_vjp_reference.bounds` evaluates it; nothing in it is fitted to the kernel's output):
    |dtheta[l, d] - exact| <= u (8 (1 + max_nl sum_d |x_nd theta_ld|) + 2 S + D + len + chunks + 4)
                              |scale| sum_n sum_s |G(s, n)| (|W[s, l]| + |W[s, L + l]|) |x_n[d]|
and the same for dX with |theta_l[d]| and the sum over l: the per-feature bound 8 u (1 + sum_d |x_d theta_d|) of the
forward pass, the roundings of the 2 S + D products, the longest chain of additions behind one output (`len` fmas of
a streamed chunk, then `chunks` partial sums) and 4 for q's two products, the final scaling and theta / (2 pi) 2 pi.
The long-double reference's own error (u_ld = 2^-64 times the same sums) is 2^-11 of that.

Worst measured error / bound on an MI355X over every case of this file: 0.113 (dtheta), 0.066 (dX).
"""

import ctypes
import math

import numpy as np
import pytest
import torch

import rff_vjp_reference as rr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
MGP_E_BADARG, MGP_E_DTYPE, MGP_E_NOMEM = -1, -3, -6  # include/mgp.h


def T(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def num_cus():
    return torch.cuda.get_device_properties(DEV).multi_processor_count


def make(N, L, D, S, seed, kind="se", lscale=1.0, zero_g=False):
    from cggp import kernels, rff
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, D))
    if kind == "se":
        theta = rng.standard_normal((L, D)) / lscale
    else:  # Matern-1/2 law: Cauchy-tailed frequencies
        theta = rff.basis_theta_parameter(kernels.Matern12(lengthscales=[lscale] * D), L, rng).numpy()
    W = rng.standard_normal((S, 2 * L))
    G = np.zeros((S, N)) if zero_g else rng.standard_normal((S, N))
    return X, theta, W, math.sqrt(1.7 / L), G


def run(X, theta, W, scale, G, layout, which):
    """(dtheta, dX) numpy or None; G is [S, N] and handed over in `layout`."""
    from cggp import ops
    Gd = T(G) if layout == ops.ROWS else T(G.T)
    dt, dx = ops.rff_sample_vjp(T(X), T(theta), T(W), scale, Gd, layout, want_dtheta=which != "dX",
                                want_dX=which != "dtheta")
    torch.cuda.synchronize()
    return (None if dt is None else dt.cpu().numpy()), (None if dx is None else dx.cpu().numpy())


def check(X, theta, W, scale, G, layout, which, report=None):
    dt, dx = run(X, theta, W, scale, G, layout, which)
    rt, rx = rr.vjp(X, theta, W, scale, G)
    bt, bx = rr.bounds(X, theta, W, scale, G, num_cus())
    assert (dt is None) == (which == "dX") and (dx is None) == (which == "dtheta")
    worst = {}
    for name, got, ref, bound in (("dtheta", dt, rt, bt), ("dX", dx, rx, bx)):
        if got is None:
            continue
        assert got.shape == ref.shape and np.all(np.isfinite(got))
        err = np.abs(got - ref.astype(np.float64))
        ratio = float(np.max(err / np.where(bound > 0, bound, 1.0))) if err.size else 0.0
        worst[name] = ratio
        print(f"{name}: worst error / bound {ratio:.3g} (N={X.shape[0]} L={theta.shape[0]} D={X.shape[1]} "
              f"S={W.shape[0]})")
        assert np.all(err <= bound), (name, ratio)
    if report is not None:
        report.update(worst)
    return dt, dx


# (N, L, D, S): every D of {1, 2, 3, 5, 8, 9, 17, 32} (each padded width 4, 8, 16, 32 at its edge and inside), S of
# {1, 5, 8}, L of {1, 255, 257} (one owner block short of full, and a second block of one lane at D > 8), N of
# {1, 255, 257, 33 (one streamed chunk of 32 and one row more: two chunks), 70 (three chunks, 24 + 24 + 22)}.  The streamed
# side of dX is L: 255 and 257 bases go in 8 and 9 chunks.
CASES = [
    (1, 1, 1, 1), (255, 255, 2, 5), (257, 257, 3, 8), (33, 257, 5, 5), (70, 1, 8, 1), (257, 255, 9, 8),
    (33, 257, 17, 5), (70, 255, 32, 8), (1, 257, 32, 1), (255, 1, 17, 5),
]


@pytest.mark.parametrize("which", ["dtheta", "dX", "both"])
@pytest.mark.parametrize("case", CASES, ids=["N%d_L%d_D%d_S%d" % c for c in CASES])
def test_vjp_against_long_double(case, which):
    from cggp import ops
    N, L, D, S = case
    layout = ops.ROWS if (N + D + S) % 2 else ops.COLS
    check(*make(N, L, D, S, seed=N + 3 * L + 5 * D + 7 * S), layout, which)


@pytest.mark.parametrize("layout", ["rows", "cols"])
def test_both_layouts_same_bits(layout):
    from cggp import ops
    args = make(257, 255, 5, 5, seed=11)
    a = check(*args, ops.ROWS if layout == "rows" else ops.COLS, "both")
    b = run(*args, ops.COLS if layout == "rows" else ops.ROWS, "both")
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])  # the layout only changes where G is read


@pytest.mark.parametrize("D,S", [(8, 5), (32, 8)])
def test_matern12_large_phases(D, S):
    """Cauchy frequencies at lengthscale 1e-3: phases of 1e4-1e6 rad, reduced exactly in revolutions as in the
    forward pass."""
    from cggp import ops
    X, theta, W, scale, G = make(257, 255, D, S, seed=21, kind="matern12", lscale=1e-3)
    assert 1e4 < float(np.max(np.abs(X @ theta.T)))
    assert float(np.median(np.abs(X @ theta.T))) < 1e6
    check(X, theta, W, scale, G, ops.ROWS, "both")


def test_zero_cotangent_and_empty_sides():
    from cggp import ops
    X, theta, W, scale, G = make(70, 33, 3, 5, seed=5, zero_g=True)
    dt, dx = run(X, theta, W, scale, G, ops.ROWS, "both")
    assert not dt.any() and not dx.any()
    e = lambda *s: torch.empty(s, dtype=torch.float64, device=DEV)
    dt, dx = ops.rff_sample_vjp(e(0, 3), T(theta), T(W), scale, e(5, 0), ops.ROWS, want_dX=True)  # N = 0
    assert dt.shape == (33, 3) and torch.count_nonzero(dt) == 0 and dx.shape == (0, 3)
    dt, dx = ops.rff_sample_vjp(T(X), e(0, 3), e(5, 0), scale, T(G), ops.ROWS, want_dX=True)  # L = 0
    assert dx.shape == (70, 3) and torch.count_nonzero(dx) == 0 and dt.shape == (0, 3)


def test_two_calls_bit_identical():
    from cggp import ops
    for N, L, D, S in ((257, 257, 8, 5), (3001, 255, 17, 8)):
        args = make(N, L, D, S, seed=N)
        a, b = run(*args, ops.ROWS, "both"), run(*args, ops.ROWS, "both")
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_values_on_both_sides_of_a_chunk_cut():
    """Cotangent on the last row of the first streamed chunk and the first row of the second only: dtheta is the sum
    of two terms that reach it through two partials; likewise two bases either side of a cut for dX."""
    from cggp import ops
    N, L, D, S = 70, 255, 3, 5
    X, theta, W, scale, G = make(N, L, D, S, seed=9)
    length, chunks = rr.chunk_plan(N, L, D, num_cus())
    assert (length, chunks) == (24, 3)
    keep = np.zeros(N, dtype=bool)
    keep[[length - 1, length]] = True
    check(X, theta, W, scale, G * keep[None, :], ops.ROWS, "dtheta")
    length, chunks = rr.chunk_plan(L, N, D, num_cus())
    assert chunks == 8 and length == 32
    Wk = W.copy()
    mask = np.zeros(L, dtype=bool)
    mask[[length - 1, length]] = True
    Wk[:, :L] *= mask[None, :]
    Wk[:, L:] *= mask[None, :]
    check(X, theta, Wk, scale, G, ops.ROWS, "dX")


def test_refusals():
    from cggp import _hip, ops
    hd = _hip.get_handle(DEV)
    lib, p = hd.lib, _hip.ptr
    call = lambda dtype, D, S, dth, dx, X, th, W, G: lib.mgp_rff_sample_vjp(
        hd.h, dtype, p(X), 5, D, p(th), 4, p(W), S, 1.0, p(G), _hip.ROWS, p(dth), p(dx))
    o = lambda *s: torch.ones(s, dtype=torch.float64, device=DEV)
    X, th, W, G, dth, dx = o(5, 3), o(4, 3), o(2, 8), o(2, 5), o(4, 3), o(5, 3)
    assert call(_hip.F64, 3, 2, dth, dx, X, th, W, G) == 0
    assert call(_hip.F32, 3, 2, dth, dx, X, th, W, G) == MGP_E_DTYPE
    assert call(_hip.F64, 3, 2, None, None, X, th, W, G) == MGP_E_BADARG
    assert b"both NULL" in lib.mgp_last_error(hd.h)
    assert call(_hip.F64, 33, 2, o(4, 33), None, o(5, 33), o(4, 33), W, G) == MGP_E_BADARG
    assert b"33" in lib.mgp_last_error(hd.h)
    assert call(_hip.F64, 3, 9, dth, None, X, th, o(9, 8), o(9, 5)) == MGP_E_BADARG
    assert b"S = 9" in lib.mgp_last_error(hd.h)
    assert call(_hip.F64, 0, 2, dth, None, X, th, W, G) == MGP_E_BADARG
    torch.cuda.synchronize()
    # the wrapper: fp32 tensors reach libmgp and are refused there; a wrong cotangent shape never gets that far
    f = lambda t: t.float()
    with pytest.raises(_hip.MgpError):
        ops.rff_sample_vjp(f(X), f(th), f(W), 1.0, f(G))
    with pytest.raises(ValueError):
        ops.rff_sample_vjp(X, th, W, 1.0, G.t().contiguous())
    with pytest.raises(ValueError):
        ops.rff_sample_vjp(X, th, W, 1.0, G, want_dtheta=False)


def test_fixed_pool_one_byte_short_is_nomem():
    """A fixed pool of exactly the bytes the call takes serves it with the same bits; one byte less is MGP_E_NOMEM
    (never an allocation)."""
    from cggp import _hip
    lib = _hip.load_library()
    X, theta, W, scale, G = make(300, 257, 8, 5, seed=13)
    Xd, td, Wd, Gd = T(X), T(theta), T(W), T(G)
    stream = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)

    def attempt(pool):
        h = ctypes.c_void_p()
        assert lib.mgp_create_ex(ctypes.byref(h), 0, pool) == 0
        try:
            lib.mgp_set_stream(h, stream)
            base = int(lib.mgp_workspace_bytes(h))
            dt, dx = torch.empty_like(td), torch.empty_like(Xd)
            rc = lib.mgp_rff_sample_vjp(h, _hip.F64, _hip.ptr(Xd), 300, 8, _hip.ptr(td), 257, _hip.ptr(Wd), 5, scale,
                                        _hip.ptr(Gd), _hip.ROWS, _hip.ptr(dt), _hip.ptr(dx))
            torch.cuda.synchronize()
            return rc, base, int(lib.mgp_workspace_bytes(h)), lib.mgp_last_error(h), dt, dx
        finally:
            torch.cuda.synchronize()
            lib.mgp_destroy(h)

    rc, base, used, _, dt0, dx0 = attempt(64 << 20)
    assert rc == 0 and used > base
    rc, _, used2, _, dt1, dx1 = attempt(used)
    assert rc == 0 and used2 == used and torch.equal(dt0, dt1) and torch.equal(dx0, dx1)
    rc, _, _, msg, _, _ = attempt(used - 1)
    assert rc == MGP_E_NOMEM and b"fixed workspace exhausted" in msg
