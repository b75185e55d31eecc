"""tests/rff_anyd_reference.py held honest (no GPU needed): its split plan and tile ladder against the expressions in
csrc/rff_anyd.hip, its scratch formula against worked sizes, and the phase term of its bounds against an fp64
emulation of the matrix-core sum -- k-steps of four products ascending, every order of the four products inside a
step, with and without a rounding of each product."""

import itertools
import os

import numpy as np

import rff_anyd_reference as ra

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "conjugate-gradient-sparse-gp_amd", "csrc", "rff_anyd.hip")


def test_plan_is_the_kernel_files():
    text = " ".join(open(SRC).read().split())
    for expr in ("constexpr int kAOwn = 64;", "constexpr int kSL = 8;", "constexpr int kAGroup = 256;",
                 "p.nblk = (owned + kAOwn - 1) / kAOwn;", "const long wg = p.nblk * groups;",
                 "const long stiles = (streamed + 15) / 16;", "if (wg < 2L * num_cus) {",
                 "ns = (2L * num_cus + wg - 1) / wg;", "const long cap = (stiles + 15) / 16;",
                 "if (ns > cap) ns = cap;", "if (ns > 256) ns = 256;", "if (ns < 1) ns = 1;",
                 "p.tps = (stiles + ns - 1) / ns;", "p.nsplit = (stiles + p.tps - 1) / p.tps;",
                 "inline int rff_anyd_ks(int D) { return (D + 3) >> 2; }",
                 "inline int rff_anyd_groups(int D) { return (D + kAGroup - 1) / kAGroup; }",
                 "per = ((D + 15) / 16 + groups - 1) / groups;", "for (int nt : {3, 4, 5, 6, 8, 10, 12}) if (per <= nt) return nt;",
                 "size_t b = a256(512 * KS * To) + a256(512 * KS * Ts);",
                 "b += vjp ? a256(2048 * To) + a256(2048 * Ts) : a256(4096 * Ts);",
                 "if (pl.nsplit > 1) b += a256(8 * (size_t)pl.nsplit * owned * PW);",
                 "const size_t PW = vjp ? (size_t)(D + 15) / 16 * 16 : 8;"):
        assert expr in text, expr
    assert ra.GROUP == 256 and ra.NT_LADDER == (3, 4, 5, 6, 8, 10, 12, 16)


def test_split_plan_properties():
    for cus in (32, 256, 304):
        for owned in (1, 40, 64, 65, 1000, 1 << 15, 1 << 20):
            for streamed in (1, 16, 17, 255, 256, 257, 1000, 4096, 1 << 20):
                for groups in (1, 2):
                    ns, tps = ra.split_plan(owned, streamed, groups, cus)
                    stiles = -(-streamed // 16)
                    assert 1 <= ns <= 256 and tps >= 1 and (ns - 1) * tps < stiles <= ns * tps  # every split non-empty
                    if ns > 1:
                        assert tps >= 8 and -(-owned // 64) * groups < 2 * cus  # >= 128 points each, CUs were idle
                    assert ra.cuts(owned, streamed, groups, cus) == [16 * tps * z for z in range(1, ns)]
    assert ra.split_plan(40, 1000, 1, 256) == (4, 16) and ra.split_plan(1 << 20, 1024, 1, 256) == (1, 64)
    assert ra.split_plan(1024, 1 << 20, 1, 256) == (32, 2048)


def test_tile_ladder_and_groups():
    assert [ra.nt_of(D) for D in (33, 48, 49, 64, 65, 77, 90, 128, 129, 160, 192, 193, 256)] == \
        [3, 3, 4, 4, 5, 5, 6, 8, 10, 10, 12, 16, 16]
    assert [(ra.groups_of(D), ra.nt_of(D)) for D in (257, 300, 512)] == [(2, 10), (2, 10), (2, 16)]
    for D in range(33, 513):
        assert ra.groups_of(D) * 16 * ra.nt_of(D) >= D and ra.nt_of(D) <= 16  # every dimension has a tile


def test_scratch_formula_on_worked_sizes():
    # N = 40 rows, L = 1000 bases, D = 77: KS = 20, To = 3, Ts = 63, four splits
    assert ra.ks_of(77) == 20
    assert ra.scratch_bytes(40, 1000, 77, 256, "forward") == 512 * 20 * 3 + 512 * 20 * 63 + 4096 * 63 + ra.a256(64 * 4 * 40)
    assert ra.scratch_bytes(40, 1000, 77, 256, "dX") == (512 * 20 * 3 + 512 * 20 * 63 + 2048 * 3 + 2048 * 63
                                                         + 8 * 4 * 40 * 80)
    assert ra.scratch_bytes(40, 1000, 77, 256, "dtheta") == 512 * 20 * 63 + 512 * 20 * 3 + 2048 * 63 + 2048 * 3
    assert ra.scratch_bytes(40, 1000, 77, 256, "both") == ra.scratch_bytes(40, 1000, 77, 256, "dX")
    # no panel: at N = 2^20, L = 1024, D = 77 the forward's scratch is the two packs, 0.65 GB against 17 GB of panel
    assert ra.scratch_bytes(1 << 20, 1024, 77, 256, "forward") < 0.7e9


def _phase_sums(x, th, order, round_products):
    """fp64 emulation of the accumulator of one (row, basis) pair: k-steps ascending, the four products of a step
    added to the accumulator in `order`; round_products=False is a chain of exact-product fmas (emulated in long
    double per step), True rounds each product first."""
    K = x.shape[0]
    acc = np.float64(0.0)
    for k0 in range(0, K, 4):
        for j in order:
            if round_products:
                acc = np.float64(acc + np.float64(x[k0 + j] * th[k0 + j]))
            else:
                acc = np.float64(np.longdouble(acc) + np.longdouble(x[k0 + j]) * np.longdouble(th[k0 + j]))
    return acc


def test_phase_bound_covers_every_order_of_a_k_step():
    """|2 pi t - theta . x| <= (K + 2) u sum_d |x_d theta_d| for the emulated t, and for a step summed pairwise before
    it joins the accumulator."""
    rng = np.random.default_rng(0)
    two_pi = 6.283185307179586476925
    worst = 0.0
    for D, scale in ((33, 1.0), (77, 1.0), (77, 1e4), (130, 30.0)):
        K = 4 * ra.ks_of(D)
        for _ in range(6):
            x = np.zeros(K)
            th = np.zeros(K)
            x[:D] = rng.standard_normal(D)
            th[:D] = rng.standard_normal(D) * scale
            thp = th / two_pi  # theta', rounded once
            exact = np.sum(x.astype(np.longdouble) * th.astype(np.longdouble))
            bound = (K + 2) * ra.U * float(np.sum(np.abs(x * th)))
            ts = [_phase_sums(x, thp, order, rp) for order in itertools.permutations(range(4)) for rp in (False, True)]
            pair = np.float64(0.0)  # ((p0 + p1) + (p2 + p3)) + acc
            for k0 in range(0, K, 4):
                p = [np.float64(x[k0 + j] * thp[k0 + j]) for j in range(4)]
                pair = np.float64(pair + np.float64(np.float64(p[0] + p[1]) + np.float64(p[2] + p[3])))
            for t in ts + [pair]:
                err = abs(float(np.longdouble(t) * np.longdouble(two_pi) - exact))
                worst = max(worst, err / bound)
                assert err <= bound
    assert 0 < worst < 1
    assert ra.phase_factor(77, 2.5) == 8 + 82 * 2.5


def test_bounds_have_the_shapes_and_the_sums_of_the_plain_call():
    import rff_vjp_reference as rr
    rng = np.random.default_rng(1)
    N, L, D, S = 50, 40, 40, 3
    X, theta, W, G = (rng.standard_normal(s) for s in ((N, D), (L, D), (S, 2 * L), (S, N)))
    bt, bx = ra.vjp_bounds(X, theta, W, 0.7, G, 256)
    pt, px = rr.bounds(X, theta, W, 0.7, G, 256)
    assert bt.shape == (L, D) and bx.shape == (N, D) and ra.forward_bound(X, theta, W, 0.7, 256).shape == (S, N)
    # the same sums of absolute terms: the ratio to the plain call's bound is one number per output
    for mine, plain in ((bt, pt), (bx, px)):
        r = mine / plain
        assert np.allclose(r, r.flat[0], rtol=1e-12) and r.flat[0] > 1
    # forward and vjp are rff_vjp_reference's
    assert ra.forward is rr.forward and ra.vjp is rr.vjp
