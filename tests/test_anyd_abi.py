"""include/mgp_anyd.h: the header compiles as plain C, libmgp.so exports what it declares, cggp/_hip.py binds it through
ANYD_SIGNATURES with the same argument count, and the other two headers' symbol sets are untouched (no GPU needed)."""

import os
import re
import shutil
import subprocess

import pytest

from test_abi import ROOT, declared_symbols, lib  # noqa: F401  (`lib` is the module fixture of test_abi)

_PROBE = r"""
#include <stdio.h>
#include "mgp_anyd.h"
int main(void) {
  /* a NULL handle is refused before anything is touched */
  double dv = 0.0, dl[MGP_MAX_D];
  int rc = mgp_kmn_knm_vjp_anyd(NULL, NULL, NULL, 0, NULL, 1, NULL, NULL, NULL, 0, 0, &dv, dl, NULL);
  printf("%d %d\n", rc, mgp_version());
  return 0;
}
"""


def _header_text():
    text = open(os.path.join(ROOT, "include", "mgp_anyd.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def anyd_symbols():
    return sorted(set(re.findall(r"^\s*(?:int|int64_t|size_t|double|void|const char\*)\s+(mgp_\w+)\s*\(",
                                 _header_text(), flags=re.M)))


def test_anyd_symbols_exported_and_bound(lib):  # noqa: F811
    from cggp import _hip
    names = anyd_symbols()
    assert names == ["mgp_kmn_knm_vjp_anyd"]
    assert sorted(_hip.ANYD_SIGNATURES) == names
    for n in names:
        fn = getattr(lib, n)  # exported
        assert fn.argtypes == _hip.ANYD_SIGNATURES[n][1] and fn.restype is _hip.ANYD_SIGNATURES[n][0]
    # the same argument count as the C declaration: mgp_kmn_knm_vjp's 13 and panel_rows
    decl = re.search(r"mgp_kmn_knm_vjp_anyd\s*\((.*?)\)\s*;", _header_text(), flags=re.S).group(1)
    assert len(decl.split(",")) == len(_hip.ANYD_SIGNATURES["mgp_kmn_knm_vjp_anyd"][1]) == 14
    assert len(_hip.SIGNATURES["mgp_kmn_knm_vjp"][1]) == 13


def test_other_headers_symbol_sets_untouched():
    from cggp import _hip
    names = declared_symbols()
    assert "mgp_kmn_knm_vjp_anyd" not in names and "mgp_kmn_knm_vjp" in names
    assert sorted(_hip.SIGNATURES) == names
    assert not set(_hip.ANYD_SIGNATURES) & (set(_hip.SIGNATURES) | set(_hip.EXT_SIGNATURES))
    assert _hip.MGP_VERSION == 210


def test_anyd_header_compiles_as_c(lib, tmp_path):  # noqa: F811
    from cggp import _hip
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "anyd_probe.c"
    src.write_text(_PROBE)
    exe = tmp_path / "anyd_probe"
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
    assert lib.mgp_kmn_knm_vjp_anyd(None, None, None, 0, None, 1, None, None, None, 0, 0, None, None, None) == -1
