"""include/mgp_pathwise.h: the header compiles as plain C, libmgp.so exports what it declares, cggp/_hip.py binds it
through EXT_SIGNATURES, and include/mgp.h's own symbol set is untouched (no GPU needed)."""

import os
import shutil
import subprocess

import pytest

from test_abi import ROOT, declared_symbols, lib  # noqa: F401  (`lib` is the module fixture of test_abi)

_PROBE = r"""
#include <stdio.h>
#include "mgp_pathwise.h"
int main(void) {
  /* a NULL handle is refused before anything is touched */
  int rc = mgp_rff_sample_vjp(NULL, MGP_F64, NULL, 0, 1, NULL, 0, NULL, 1, 1.0, NULL, MGP_ROWS, NULL, NULL);
  printf("%d %d\n", rc, mgp_version());
  return 0;
}
"""


def pathwise_symbols():
    import re
    text = open(os.path.join(ROOT, "include", "mgp_pathwise.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"^\s*(?:int|int64_t|size_t|double|void|const char\*)\s+(mgp_\w+)\s*\(", text,
                                 flags=re.M)))


def test_pathwise_symbols_exported_and_bound(lib):  # noqa: F811
    from cggp import _hip
    names = pathwise_symbols()
    assert names == ["mgp_rff_sample_vjp"]
    assert sorted(_hip.EXT_SIGNATURES) == names
    for n in names:
        fn = getattr(lib, n)  # exported
        assert fn.argtypes == _hip.EXT_SIGNATURES[n][1] and fn.restype is _hip.EXT_SIGNATURES[n][0]
    assert len(_hip.EXT_SIGNATURES["mgp_rff_sample_vjp"][1]) == 14


def test_mgp_h_symbol_set_untouched():
    from cggp import _hip
    names = declared_symbols()
    assert "mgp_rff_sample_vjp" not in names and "mgp_rff_sample" in names
    assert sorted(_hip.SIGNATURES) == names
    assert not set(_hip.SIGNATURES) & set(_hip.EXT_SIGNATURES)
    assert _hip.MGP_VERSION == 210


def test_pathwise_header_compiles_as_c(lib, tmp_path):  # noqa: F811
    from cggp import _hip
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "pathwise_probe.c"
    src.write_text(_PROBE)
    exe = tmp_path / "pathwise_probe"
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
    assert lib.mgp_rff_sample_vjp(None, 1, None, 0, 1, None, 0, None, 1, 1.0, None, 1, None, None) == -1
