"""include/mgp_points.h: the header compiles as plain C, libmgp.so exports exactly what it declares, cggp/_hip.py binds
it through POINTS_SIGNATURES with the declared argument count, and the other headers' symbol sets and the library
version are untouched (no GPU needed)."""

import os
import re
import shutil
import subprocess

import pytest

from test_abi import ROOT, declared_symbols, lib  # noqa: F401  (`lib` is the module fixture of test_abi)
from test_anyd_abi import anyd_symbols
from test_predict_abi import predict_symbols
from test_sweep_anyd_abi import sweep_anyd_symbols

_PROBE = r"""
#include <stdio.h>
#include "mgp_points.h"
int main(void) {
  /* a NULL handle is refused before anything is touched */
  int a = mgp_k_dense_vjp_points(NULL, NULL, NULL, 0, NULL, 0, NULL, 0, 0, NULL, NULL, NULL, NULL);
  printf("%d %d\n", a, mgp_version());
  return 0;
}
"""

NAMES = ["mgp_k_dense_vjp_points"]


def _header_text():
    text = open(os.path.join(ROOT, "include", "mgp_points.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def points_symbols():
    return sorted(set(re.findall(r"^\s*(?:int|int64_t|size_t|double|void|const char\*)\s+(mgp_\w+)\s*\(",
                                 _header_text(), flags=re.M)))


def test_symbols_exported_and_bound(lib):  # noqa: F811
    from cggp import _hip
    assert points_symbols() == NAMES
    assert sorted(_hip.POINTS_SIGNATURES) == NAMES
    for n in NAMES:
        fn = getattr(lib, n)  # exported
        assert fn.argtypes == _hip.POINTS_SIGNATURES[n][1] and fn.restype is _hip.POINTS_SIGNATURES[n][0]
        decl = re.search(rf"{n}\s*\((.*?)\)\s*;", _header_text(), flags=re.S).group(1)
        assert len(decl.split(",")) == len(_hip.POINTS_SIGNATURES[n][1]) == 13


def test_library_exports_no_other_points_symbol(lib):  # noqa: F811
    from cggp import _hip
    if shutil.which("nm") is None:
        pytest.skip("no nm")
    out = subprocess.run(["nm", "-D", "--defined-only", _hip.lib_path()], capture_output=True, text=True, check=True)
    exported = {line.split()[-1] for line in out.stdout.splitlines() if line.strip()}
    assert sorted(s for s in exported if "points" in s and not s.startswith("_Z")) == NAMES


def test_other_headers_symbol_sets_untouched():
    from cggp import _hip
    names = declared_symbols()
    assert not set(NAMES) & set(names) and "mgp_k_dense_vjp" in names
    assert sorted(_hip.SIGNATURES) == names
    assert anyd_symbols() == sorted(_hip.ANYD_SIGNATURES) == ["mgp_kmn_knm_vjp_anyd"]
    assert sweep_anyd_symbols() == sorted(_hip.SWEEP_ANYD_SIGNATURES)
    assert predict_symbols() == sorted(_hip.PREDICT_SIGNATURES) == ["mgp_knm_quadform"]
    tables = (_hip.SIGNATURES, _hip.EXT_SIGNATURES, _hip.ANYD_SIGNATURES, _hip.SWEEP_ANYD_SIGNATURES,
              _hip.PREDICT_SIGNATURES, _hip.POINTS_SIGNATURES)
    assert sum(len(t) for t in tables) == len(set().union(*tables))  # pairwise disjoint
    assert _hip.MGP_VERSION == 210
    text = open(os.path.join(ROOT, "include", "mgp.h")).read()
    assert re.search(r"#define MGP_VERSION (\d+)", text).group(1) == "210"


def test_header_compiles_as_c(lib, tmp_path):  # noqa: F811
    from cggp import _hip
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "points_probe.c"
    src.write_text(_PROBE)
    exe = tmp_path / "points_probe"
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
    assert lib.mgp_k_dense_vjp_points(None, None, None, 0, None, 0, None, 0, 0, None, None, None, None) == -1
