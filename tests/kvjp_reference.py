"""Long-double reference of `mgp_kmn_knm_vjp_anyd` straight from the formulas of csrc/kmn_grad.hip:4-12, with the
companion sums of absolute terms the derived error bound is measured against.

With K = k(X, Z) [N, M], a = x / l, b = z / l, r2_nm = sum_d (a_nd - b_md)^2 (direct differences), f = k / variance and
f' = df/dr2 (the four profiles; Matern: r = sqrt(max(r2, 1e-36)) and f' = 0 at that floor):
    W         = K (Gq + Gq^T) + Y Gb^T                     (Gq = None: Y Gb^T alone)
    dvariance = sum_nm W_nm f_nm
    dl_d      = variance (-2 / l_d) sum_nm W_nm f'_nm (a_nd - b_md)^2
    dZ_md     = variance (-2 / l_d) sum_n  W_nm f'_nm (a_nd - b_md)
Companions: for W itself Wa_nm = sum_j |K_nj| |G2_jm| + sum_p |Y_np| |Gb_mp| (>= |W_nm|: what a computed W's rounding is
relative to), and per output the same sum with every term replaced by Wa |term|."""

from collections import namedtuple

import numpy as np

LD = np.longdouble

KvjpRef = namedtuple("KvjpRef", "dv dl dZ sv sl sz W Wa")


def profile(name, r2):
    """(f, f') in long double at the scaled squared distance r2"""
    r2 = np.asarray(r2, dtype=LD)
    if name == "se":
        f = np.exp(LD(-0.5) * r2)
        return f, LD(-0.5) * f
    floor = ~(r2 > LD(1e-36))
    r = np.sqrt(np.where(floor, LD(1e-36), r2))
    if name == "matern12":
        f = np.exp(-r)
        return f, np.where(floor, LD(0), -f / (LD(2) * r))
    if name == "matern32":
        s3 = np.sqrt(LD(3))
        e = np.exp(-s3 * r)
        return (LD(1) + s3 * r) * e, np.where(floor, LD(0), LD(-1.5) * e)
    if name == "matern52":
        s5 = np.sqrt(LD(5))
        e = np.exp(-s5 * r)
        return ((LD(1) + s5 * r + LD(5) / LD(3) * r2) * e,
                np.where(floor, LD(0), LD(-5) / LD(6) * (LD(1) + s5 * r) * e))
    raise ValueError(name)


def kvjp_reference(name, variance, lengthscales, X, Z, Gq, Y=None, Gb=None, block=64):
    """KvjpRef(dv, dl [D], dZ [M, D], their companions sv, sl [D], sz [M, D], W [N, M], Wa [N, M]), all long double"""
    X, Z = np.asarray(X, dtype=LD), np.asarray(Z, dtype=LD)
    (N, D), M = X.shape, Z.shape[0]
    ls = np.asarray(lengthscales, dtype=LD).reshape(-1)
    if ls.shape[0] == 1:
        ls = np.repeat(ls, D)
    var = LD(variance)
    Xs, Zs = X / ls, Z / ls
    G2 = None if Gq is None else np.asarray(Gq, dtype=LD) + np.asarray(Gq, dtype=LD).T
    coef = var * LD(-2) / ls
    dv, dl, dZ = LD(0), np.zeros(D, dtype=LD), np.zeros((M, D), dtype=LD)
    sv, sl, sz = LD(0), np.zeros(D, dtype=LD), np.zeros((M, D), dtype=LD)
    Wall, Waall = np.zeros((N, M), dtype=LD), np.zeros((N, M), dtype=LD)
    for i0 in range(0, N, block):
        diff = Xs[i0:i0 + block, None, :] - Zs[None, :, :]
        f, fp = profile(name, (diff * diff).sum(axis=2))
        W, Wa = np.zeros(f.shape, dtype=LD), np.zeros(f.shape, dtype=LD)
        if G2 is not None:
            K = var * f
            W, Wa = K @ G2, np.abs(K) @ np.abs(G2)
        if Y is not None:
            Yb, Gbl = np.asarray(Y[i0:i0 + block], dtype=LD), np.asarray(Gb, dtype=LD)
            W, Wa = W + Yb @ Gbl.T, Wa + np.abs(Yb) @ np.abs(Gbl).T
        Wall[i0:i0 + block], Waall[i0:i0 + block] = W, Wa
        dv += np.sum(W * f)
        sv += np.sum(Wa * np.abs(f))
        g, ga = (W * fp)[:, :, None], (Wa * np.abs(fp))[:, :, None]
        dl += (g * diff * diff).sum(axis=(0, 1)) * coef
        sl += (ga * diff * diff).sum(axis=(0, 1)) * np.abs(coef)
        dZ += (g * diff).sum(axis=0) * coef
        sz += (ga * np.abs(diff)).sum(axis=0) * np.abs(coef)
    return KvjpRef(dv, dl, dZ, sv, sl, sz, Wall, Waall)
