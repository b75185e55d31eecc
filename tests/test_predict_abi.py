"""include/mgp_predict.h: the header compiles as plain C, libmgp.so exports exactly what it declares, cggp/_hip.py
binds it through PREDICT_SIGNATURES with the declared argument count, the other headers' symbol sets and the library
version are untouched, and the `fused_variance` setting is checked (no GPU needed)."""

import os
import re
import shutil
import subprocess

import pytest

from test_abi import ROOT, declared_symbols, lib  # noqa: F401  (`lib` is the module fixture of test_abi)
from test_anyd_abi import anyd_symbols
from test_sweep_anyd_abi import sweep_anyd_symbols

_PROBE = r"""
#include <stdio.h>
#include "mgp_predict.h"
int main(void) {
  /* a NULL handle is refused before anything is touched */
  int a = mgp_knm_quadform(NULL, NULL, NULL, 0, NULL, 0, NULL, 0, NULL);
  printf("%d %d\n", a, mgp_version());
  return 0;
}
"""

NAMES = ["mgp_knm_quadform"]


def _header_text():
    text = open(os.path.join(ROOT, "include", "mgp_predict.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def predict_symbols():
    return sorted(set(re.findall(r"^\s*(?:int|int64_t|size_t|double|void|const char\*)\s+(mgp_\w+)\s*\(",
                                 _header_text(), flags=re.M)))


def test_symbols_exported_and_bound(lib):  # noqa: F811
    from cggp import _hip
    assert predict_symbols() == NAMES
    assert sorted(_hip.PREDICT_SIGNATURES) == NAMES
    for n in NAMES:
        fn = getattr(lib, n)  # exported
        assert fn.argtypes == _hip.PREDICT_SIGNATURES[n][1] and fn.restype is _hip.PREDICT_SIGNATURES[n][0]
        decl = re.search(rf"{n}\s*\((.*?)\)\s*;", _header_text(), flags=re.S).group(1)
        assert len(decl.split(",")) == len(_hip.PREDICT_SIGNATURES[n][1]) == 9


def test_library_exports_no_other_quadform_symbol(lib):  # noqa: F811
    from cggp import _hip
    if shutil.which("nm") is None:
        pytest.skip("no nm")
    out = subprocess.run(["nm", "-D", "--defined-only", _hip.lib_path()], capture_output=True, text=True, check=True)
    exported = {line.split()[-1] for line in out.stdout.splitlines() if line.strip()}
    assert sorted(s for s in exported if "quadform" in s and not s.startswith("_Z")) == NAMES


def test_other_headers_symbol_sets_untouched():
    from cggp import _hip
    names = declared_symbols()
    assert not set(NAMES) & set(names) and "mgp_knm_project" in names
    assert sorted(_hip.SIGNATURES) == names
    assert anyd_symbols() == sorted(_hip.ANYD_SIGNATURES) == ["mgp_kmn_knm_vjp_anyd"]
    assert sweep_anyd_symbols() == sorted(_hip.SWEEP_ANYD_SIGNATURES)
    tables = (_hip.SIGNATURES, _hip.EXT_SIGNATURES, _hip.ANYD_SIGNATURES, _hip.SWEEP_ANYD_SIGNATURES,
              _hip.PREDICT_SIGNATURES)
    assert sum(len(t) for t in tables) == len(set().union(*tables))  # pairwise disjoint
    assert _hip.MGP_VERSION == 210
    text = open(os.path.join(ROOT, "include", "mgp.h")).read()
    assert re.search(r"#define MGP_VERSION (\d+)", text).group(1) == "210"


def test_header_compiles_as_c(lib, tmp_path):  # noqa: F811
    from cggp import _hip
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "predict_probe.c"
    src.write_text(_PROBE)
    exe = tmp_path / "predict_probe"
    libdir = os.path.dirname(_hip.lib_path())
    cmd = ["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o",
           str(exe), "-L", libdir, "-l:libmgp.so", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib",
           "-Wl,--allow-shlib-undefined"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ["-1", str(_hip.MGP_VERSION)]


def test_null_handle_is_badarg(lib):  # noqa: F811
    assert lib.mgp_knm_quadform(None, None, None, 0, None, 0, None, 0, None) == -1


def test_fused_variance_setting_is_checked():
    from cggp import conjugate_gradient as cgm
    import torch
    for ok in (False, True, "auto"):
        assert cgm.check_fused_variance(ok) is ok or cgm.check_fused_variance(ok) == ok
    for bad in (None, 1, 0, "yes", "Auto"):
        with pytest.raises(ValueError):
            cgm.check_fused_variance(bad)
    # fp32 and D > 32 never qualify for "auto"; True is True everywhere (libmgp takes its generic route by itself)
    assert not cgm.fused_variance_auto(torch.float32, 8, 1 << 13) and not cgm.fused_variance_auto(torch.float64, 33, 1 << 13)
    assert cgm.use_fused_variance(True, torch.float32, 8, 10) and not cgm.use_fused_variance(False, torch.float64, 8, 1 << 13)
    for M in (1, 1024, 4096, 8192):
        assert cgm.use_fused_variance("auto", torch.float64, 8, M) == cgm.fused_variance_auto(torch.float64, 8, M)
    # the rule is monotone in M: a threshold, or nowhere
    took = [cgm.fused_variance_auto(torch.float64, 8, M) for M in (1, 512, 1024, 4096, 8192, 1 << 15)]
    assert took == sorted(took)
    if cgm.FUSED_VARIANCE_AUTO_MIN_M is None:
        assert not any(took)
