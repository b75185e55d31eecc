"""Long-double reference for `mgp_k_dense_vjp_points` (include/mgp_points.h): the four outputs of the VJP of a dense
kernel block K = k(A, B) at a dense cotangent G, every pair evaluated with direct differences, and for each output the
sum of |terms| the tests measure rounding against.  Extends `k_dense_vjp_reference` of sgpr_grad_reference.py (whose
scalars it reproduces) by the point gradients."""

import numpy as np

from lml_reference import _profile
from sgpr_grad_reference import LD

VJP_BAR = 1e-10  # the project's fp64 VJP bar: |got - ref| <= VJP_BAR * sum |terms|, per output element


def k_dense_vjp_points_reference(name, variance, lengthscales, A, B, G, block=None):
    """dict of long-double arrays: dv, dl [D], dA [na, D], dB [nb, D] and sv, sl, sA, sB, the same sums over |terms|.
    `block`: rows of A per step (default: about 2^20 pair-dimensions per temporary)."""
    A, B, G = np.asarray(A, dtype=LD), np.asarray(B, dtype=LD), np.asarray(G, dtype=LD)
    ls = np.asarray(lengthscales, dtype=LD).reshape(-1)
    if ls.shape[0] == 1:
        ls = np.repeat(ls, A.shape[1])
    As, Bs = A / ls, B / ls
    var = LD(variance)
    cl, cp = var * LD(-2) / ls, var * LD(2) / ls
    (na, D), nb = A.shape, B.shape[0]
    block = block or max(1, (1 << 20) // max(1, nb * D))
    out = dict(dv=LD(0), sv=LD(0), dl=np.zeros(D, dtype=LD), sl=np.zeros(D, dtype=LD),
               dA=np.zeros((na, D), dtype=LD), sA=np.zeros((na, D), dtype=LD),
               dB=np.zeros((nb, D), dtype=LD), sB=np.zeros((nb, D), dtype=LD))
    for i0 in range(0, na, block):
        diff = As[i0:i0 + block, None, :] - Bs[None, :, :]
        f, fp = _profile(name, (diff * diff).sum(axis=2))
        Gb = G[i0:i0 + block]
        out["dv"] += np.sum(Gb * f)
        out["sv"] += np.sum(np.abs(Gb * f))
        h = (Gb * fp)[:, :, None]
        wl = h * diff * diff * cl
        out["dl"] += wl.sum(axis=(0, 1))
        out["sl"] += np.abs(wl).sum(axis=(0, 1))
        wp = h * diff * cp
        out["dA"][i0:i0 + block] = wp.sum(axis=1)
        out["sA"][i0:i0 + block] = np.abs(wp).sum(axis=1)
        out["dB"] -= wp.sum(axis=0)
        out["sB"] += np.abs(wp).sum(axis=0)
    return out


def excess(got, ref, scale, bar=VJP_BAR):
    """max over the elements of |got - ref| / (bar * scale): <= 1 passes.  Elements whose scale is 0 must be exactly 0
    in both (no term contributes), which counts as 0 and anything else as inf."""
    got, ref, scale = (np.atleast_1d(np.asarray(x, dtype=LD)) for x in (got, ref, scale))
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(scale > 0, err / (LD(bar) * scale), np.where(err == 0, LD(0), LD(np.inf)))
    return float(q.max()) if q.size else 0.0
