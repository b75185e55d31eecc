"""MGP_OP_KMM_LAMBDA_WIDE_ANYD at the C boundary (no GPU needed): the kind is an enum block of its own in
include/mgp_sweep_anyd.h with the value 8, the header still compiles as plain C and prints it, cggp/_hip.py binds the
same value, no function and no header was added, every signature table and the library version are untouched; and
the `wide_anyd` setting is checked where it enters."""

import os
import re
import shutil
import subprocess

import pytest

from test_abi import ROOT, declared_symbols, lib  # noqa: F401  (`lib` is the module fixture of test_abi)
from test_anyd_abi import anyd_symbols
from test_sweep_anyd_abi import NAMES as SWEEP_ANYD_NAMES
from test_sweep_anyd_abi import sweep_anyd_symbols

_PROBE = r"""
#include <stdio.h>
#include "mgp_sweep_anyd.h"
int main(void) {
  printf("%d %d %d %d\n", MGP_OP_KMM_LAMBDA_WIDE, MGP_OP_KMM_LAMBDA_ANYD, MGP_OP_KMM_LAMBDA_WIDE_ANYD, mgp_version());
  return 0;
}
"""


def _header(strip_comments=True):
    text = open(os.path.join(ROOT, "include", "mgp_sweep_anyd.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S) if strip_comments else text


def test_enum_value_in_a_block_of_its_own():
    from cggp import _hip
    blocks = re.findall(r"enum\s*\{([^}]*)\}", _header())
    mine = [b for b in blocks if "MGP_OP_KMM_LAMBDA_WIDE_ANYD" in b]
    assert len(mine) == 1 and len(blocks) == 2
    vals = {k.strip(): int(v) for k, v in (item.split("=") for item in mine[0].split(","))}
    assert vals == {"MGP_OP_KMM_LAMBDA_WIDE_ANYD": 8}
    assert _hip.OP_KMM_LAMBDA_WIDE_ANYD == 8
    kinds = (_hip.OP_DENSE, _hip.OP_SGPR, _hip.OP_KMM_LAMBDA, _hip.OP_KXX_NOISE, _hip.OP_KMM_LAMBDA_WIDE,
             _hip.OP_SGPR_ANYD, _hip.OP_KMM_LAMBDA_ANYD, _hip.OP_KXX_NOISE_ANYD, _hip.OP_KMM_LAMBDA_WIDE_ANYD)
    assert kinds == tuple(range(9))


def test_header_comment_states_the_contract():
    text = re.sub(r"\s*\n \*\s*", " ", _header(strip_comments=False))
    for phrase in ("those of MGP_OP_KMM_LAMBDA;", "exactly the code of MGP_OP_KMM_LAMBDA_WIDE, and its bits",
                   "fp32: exactly the code of MGP_OP_KMM_LAMBDA, and its bits", "the `prj` arena of the handle alone",
                   "align256(8 * 64 * KS * ceil(M / 16)) + align256(8 * nsplit * 64 * ceil(M / 64) * RP)",
                   "u (terms + nsplit + 3)", "two calls give the same bits", "MGP_E_NOMEM"):
        assert phrase in text, phrase


def test_header_compiles_as_c_and_prints_the_value(lib, tmp_path):  # noqa: F811
    from cggp import _hip
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "kmm_wide_anyd_probe.c"
    src.write_text(_PROBE)
    exe = tmp_path / "kmm_wide_anyd_probe"
    libdir = os.path.dirname(_hip.lib_path())
    cmd = ["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o",
           str(exe), "-L", libdir, "-l:libmgp.so", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib",
           "-Wl,--allow-shlib-undefined"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ["4", "6", "8", str(_hip.MGP_VERSION)]


def test_no_function_and_no_header_was_added():
    from cggp import _hip
    assert sweep_anyd_symbols() == SWEEP_ANYD_NAMES == sorted(_hip.SWEEP_ANYD_SIGNATURES)
    names = declared_symbols()
    assert sorted(_hip.SIGNATURES) == names
    assert anyd_symbols() == sorted(_hip.ANYD_SIGNATURES) == ["mgp_kmn_knm_vjp_anyd"]
    tables = [getattr(_hip, t) for t in dir(_hip) if t.endswith("SIGNATURES")]
    assert sum(len(t) for t in tables) == len(set().union(*tables))  # pairwise disjoint
    assert not [n for t in tables for n in t if "wide_anyd" in n]
    assert sorted(os.listdir(os.path.join(ROOT, "include"))) == [
        "mgp.h", "mgp_anyd.h", "mgp_pathwise.h", "mgp_points.h", "mgp_predict.h", "mgp_sweep_anyd.h"]
    assert _hip.MGP_VERSION == 210
    text = open(os.path.join(ROOT, "include", "mgp.h")).read()
    assert re.search(r"#define MGP_VERSION (\d+)", text).group(1) == "210"


def test_library_exports_no_wide_anyd_symbol(lib):  # noqa: F811
    from cggp import _hip
    if shutil.which("nm") is None:
        pytest.skip("no nm")
    out = subprocess.run(["nm", "-D", "--defined-only", _hip.lib_path()], capture_output=True, text=True, check=True)
    exported = {line.split()[-1] for line in out.stdout.splitlines() if line.strip()}
    assert not [s for s in exported if "wide_anyd" in s and not s.startswith("_Z")]


def test_wide_anyd_setting_is_checked():
    import torch

    from cggp import conjugate_gradient as cgm
    from cggp import models, training
    for ok in (False, True, "auto"):
        assert cgm.check_wide_anyd(ok) is ok or cgm.check_wide_anyd(ok) == ok
    for bad in (None, 1, 0, "yes", "Auto"):
        with pytest.raises(ValueError, match="wide_anyd"):
            cgm.check_wide_anyd(bad)
    f64 = torch.float64
    assert not cgm.wide_anyd_auto(torch.float32, 77, 256, 1 << 16) and not cgm.wide_anyd_auto(f64, 32, 256, 1 << 16)
    # the refusals come before any device call: host tensors and a kernel that must not be asked
    class _Kernel:
        variance = 1.0

        def spec(self, D):
            raise AssertionError("the refusal comes first")

    M = 12
    Z, lam = torch.zeros((M, 40), dtype=f64), torch.ones(M, dtype=f64)
    with pytest.raises(ValueError, match="wide_anyd must be"):
        cgm.KmmLambdaOperator(_Kernel(), Z, lam, wide_anyd="on")
    for matrix_free, setting, err in ((False, True, "matrix_free=True"), (False, "auto", "matrix_free=True"),
                                      (True, 2, "wide_anyd must be")):
        with pytest.raises(ValueError, match=err):
            models.CGGP(_Kernel(), 0.3, Z, None, matrix_free=matrix_free, wide_anyd=setting)
        with pytest.raises(ValueError, match=err):
            models.cdgp_class(_Kernel(), 0.3, Z, matrix_free=matrix_free, wide_anyd=setting)
        with pytest.raises(ValueError, match=err):
            training.TrainableCGGP(_Kernel(), 0.3, Z, pseudo_u=lam, cluster_counts=lam, matrix_free=matrix_free,
                                   wide_anyd=setting)
