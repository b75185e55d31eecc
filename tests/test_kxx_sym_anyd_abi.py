"""MGP_OP_KXX_NOISE_SYM_ANYD at the C boundary (no GPU needed): the kind is a value of include/mgp.h's operator-kind
enum, the header still compiles as plain C and prints it, cggp/_hip.py binds the same value, no function and no header
was added, every signature table and the library version are untouched; and the `sym_anyd` setting is checked where
it enters, before any device call."""

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
#include "mgp.h"
int main(void) {
  printf("%d %d %d\n", MGP_OP_KXX_NOISE, MGP_OP_KXX_NOISE_SYM_ANYD, mgp_version());
  return 0;
}
"""


def _header(name="mgp.h"):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_enum_value_in_the_operator_kind_enum():
    from cggp import _hip
    blocks = [b for b in re.findall(r"enum\s*\{([^}]*)\}", _header()) if "MGP_OP_KXX_NOISE_SYM_ANYD" in b]
    assert len(blocks) == 1
    vals = {k.strip(): int(v) for k, v in (item.split("=") for item in blocks[0].split(","))}
    assert vals == {"MGP_OP_DENSE": 0, "MGP_OP_SGPR": 1, "MGP_OP_KMM_LAMBDA": 2, "MGP_OP_KXX_NOISE": 3,
                    "MGP_OP_KMM_LAMBDA_WIDE": 4, "MGP_OP_KXX_NOISE_SYM_ANYD": 9}
    assert _hip.OP_KXX_NOISE_SYM_ANYD == 9
    kinds = [getattr(_hip, n) for n in dir(_hip) if n.startswith("OP_")]
    assert sorted(kinds) == list(range(10))  # every kind once, none reused
    # the enum blocks of the other headers are as they were
    assert len(re.findall(r"enum\s*\{", _header("mgp_sweep_anyd.h"))) == 2
    assert "SYM_ANYD" not in _header("mgp_sweep_anyd.h") and "SYM_ANYD" not in _header("mgp_pathwise.h")


def test_header_compiles_as_c_and_prints_the_value(lib, tmp_path):  # noqa: F811
    from cggp import _hip
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "kxx_sym_anyd_probe.c"
    src.write_text(_PROBE)
    exe = tmp_path / "kxx_sym_anyd_probe"
    libdir = os.path.dirname(_hip.lib_path())
    cmd = ["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o",
           str(exe), "-L", libdir, "-l:libmgp.so", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib",
           "-Wl,--allow-shlib-undefined"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ["3", "9", str(_hip.MGP_VERSION)]


def test_no_function_and_no_header_was_added():
    from cggp import _hip
    assert sweep_anyd_symbols() == SWEEP_ANYD_NAMES == sorted(_hip.SWEEP_ANYD_SIGNATURES)
    assert sorted(_hip.SIGNATURES) == declared_symbols()
    assert anyd_symbols() == sorted(_hip.ANYD_SIGNATURES) == ["mgp_kmn_knm_vjp_anyd"]
    tables = [getattr(_hip, t) for t in dir(_hip) if t.endswith("SIGNATURES")]
    assert sum(len(t) for t in tables) == len(set().union(*tables))  # pairwise disjoint
    assert not [n for t in tables for n in t if "sym_anyd" in n]
    assert sorted(os.listdir(os.path.join(ROOT, "include"))) == [
        "mgp.h", "mgp_anyd.h", "mgp_pathwise.h", "mgp_points.h", "mgp_predict.h", "mgp_sweep_anyd.h"]
    assert _hip.MGP_VERSION == 210
    text = open(os.path.join(ROOT, "include", "mgp.h")).read()
    assert re.search(r"#define MGP_VERSION (\d+)", text).group(1) == "210"


def test_library_exports_no_sym_anyd_symbol(lib):  # noqa: F811
    from cggp import _hip
    if shutil.which("nm") is None:
        pytest.skip("no nm")
    out = subprocess.run(["nm", "-D", "--defined-only", _hip.lib_path()], capture_output=True, text=True, check=True)
    exported = {line.split()[-1] for line in out.stdout.splitlines() if line.strip()}
    assert not [s for s in exported if "sym_anyd" in s and not s.startswith("_Z")]


def test_sym_anyd_setting_is_checked_before_any_device_call():
    import torch

    from cggp import conjugate_gradient as cgm
    from cggp import models, training
    for ok in (False, True, "auto"):
        assert cgm.check_sym_anyd(ok) is ok or cgm.check_sym_anyd(ok) == ok
    for bad in (None, 1, 0, "yes", "Auto"):
        with pytest.raises(ValueError, match="sym_anyd"):
            cgm.check_sym_anyd(bad)
    f64 = torch.float64
    assert not cgm.sym_anyd_auto(torch.float32, 77, 16, 1 << 17) and not cgm.sym_anyd_auto(f64, 32, 16, 1 << 17)

    # the refusals come before any device call: host tensors and a kernel that must not be asked
    class _Kernel:
        variance = 1.0
        name = "se"
        lengthscales = [1.0]

        def spec(self, D):
            raise AssertionError("the refusal comes first")

    N = 12
    X, Y = torch.zeros((N, 40), dtype=f64), torch.zeros((N, 1), dtype=f64)
    for bad in ("on", 2, None):
        with pytest.raises(ValueError, match="sym_anyd must be"):
            cgm.KxxNoiseOperator(_Kernel(), X, 0.1, sym_anyd=bad)
        with pytest.raises(ValueError, match="sym_anyd must be"):
            models.GPR((X, Y), _Kernel(), 0.1, sym_anyd=bad)
        with pytest.raises(ValueError, match="sym_anyd must be"):
            models.gpr_class((X, Y), _Kernel(), models.Gaussian(0.1), sym_anyd=bad)
        with pytest.raises(ValueError, match="sym_anyd must be"):
            models.create_gpr_model((X, Y), lambda dim: _Kernel(), sym_anyd=bad)
        with pytest.raises(ValueError, match="sym_anyd must be"):
            training.TrainableGPR(_Kernel(), 0.1, X, Y, sym_anyd=bad)
    # accepted settings are kept and handed on (host tensors: no device call is made by a constructor)
    from cggp import kernels
    kern = kernels.SquaredExponential(1.0, [1.0] * 40)
    assert models.GPR((X, Y), kern, 0.1, sym_anyd="auto").sym_anyd == "auto"
    assert models.gpr_class((X, Y), kern, models.Gaussian(0.1), sym_anyd=True).sym_anyd is True
    t = training.TrainableGPR(kern, 0.1, X, Y, sym_anyd=True)
    assert t.sym_anyd is True and t.frozen_model().sym_anyd is True
