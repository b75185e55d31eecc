"""include/mgp_sweep_anyd.h: the header compiles as plain C, libmgp.so exports exactly what it declares, cggp/_hip.py
binds it through SWEEP_ANYD_SIGNATURES with the declared argument counts, and the other headers' symbol sets and the
library version are untouched (no GPU needed)."""

import os
import re
import shutil
import subprocess

import pytest

from test_abi import ROOT, declared_symbols, lib  # noqa: F401  (`lib` is the module fixture of test_abi)
from test_anyd_abi import anyd_symbols

_PROBE = r"""
#include <stdio.h>
#include "mgp_sweep_anyd.h"
int main(void) {
  /* a NULL handle is refused before anything is touched */
  int a = mgp_knm_matvec_anyd(NULL, NULL, NULL, 0, NULL, 0, NULL, 0, MGP_COLS, NULL, MGP_COLS);
  int b = mgp_kmn_matvec_anyd(NULL, NULL, NULL, 0, NULL, 0, NULL, 0, MGP_ROWS, NULL, MGP_ROWS);
  int c = mgp_kxx_matvec_anyd(NULL, NULL, NULL, 0, 0.0, NULL, 0, MGP_COLS, NULL, MGP_COLS);
  printf("%d %d %d %d %d %d %d\n", a, b, c, MGP_OP_SGPR_ANYD, MGP_OP_KMM_LAMBDA_ANYD, MGP_OP_KXX_NOISE_ANYD, mgp_version());
  return 0;
}
"""

NAMES = ["mgp_kmn_matvec_anyd", "mgp_knm_matvec_anyd", "mgp_kxx_matvec_anyd"]


def _header_text():
    text = open(os.path.join(ROOT, "include", "mgp_sweep_anyd.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def sweep_anyd_symbols():
    return sorted(set(re.findall(r"^\s*(?:int|int64_t|size_t|double|void|const char\*)\s+(mgp_\w+)\s*\(",
                                 _header_text(), flags=re.M)))


def test_symbols_exported_and_bound(lib):  # noqa: F811
    from cggp import _hip
    assert sweep_anyd_symbols() == NAMES
    assert sorted(_hip.SWEEP_ANYD_SIGNATURES) == NAMES
    for n in NAMES:
        fn = getattr(lib, n)  # exported
        assert fn.argtypes == _hip.SWEEP_ANYD_SIGNATURES[n][1] and fn.restype is _hip.SWEEP_ANYD_SIGNATURES[n][0]
        decl = re.search(rf"{n}\s*\((.*?)\)\s*;", _header_text(), flags=re.S).group(1)
        plain = n[:-len("_anyd")]
        # the declared argument count, which is the plain name's
        assert len(decl.split(",")) == len(_hip.SWEEP_ANYD_SIGNATURES[n][1]) == len(_hip.SIGNATURES[plain][1])
        assert _hip.SWEEP_ANYD_SIGNATURES[n] == _hip.SIGNATURES[plain]
    assert len(_hip.SWEEP_ANYD_SIGNATURES["mgp_knm_matvec_anyd"][1]) == 11
    assert len(_hip.SWEEP_ANYD_SIGNATURES["mgp_kxx_matvec_anyd"][1]) == 10


def test_library_exports_no_other_anyd_sweep_symbol(lib):  # noqa: F811
    from cggp import _hip
    if shutil.which("nm") is None:
        pytest.skip("no nm")
    out = subprocess.run(["nm", "-D", "--defined-only", _hip.lib_path()], capture_output=True, text=True, check=True)
    exported = {line.split()[-1] for line in out.stdout.splitlines() if line.strip()}
    mine = sorted(s for s in exported if re.fullmatch(r"mgp_k(nm|mn|xx)_matvec\w*", s))
    assert mine == sorted(NAMES + [n[:-len("_anyd")] for n in NAMES])
    # the internal forms stay internal: no unmangled sweep_anyd symbol beyond the three
    assert not [s for s in exported if "sweep" in s and "anyd" in s and not s.startswith("_Z")]


def test_operator_kinds():
    from cggp import _hip
    enum = re.search(r"enum\s*\{([^}]*MGP_OP_SGPR_ANYD[^}]*)\}", _header_text()).group(1)
    vals = {k.strip(): int(v) for k, v in (item.split("=") for item in enum.split(","))}
    assert vals == {"MGP_OP_SGPR_ANYD": 5, "MGP_OP_KMM_LAMBDA_ANYD": 6, "MGP_OP_KXX_NOISE_ANYD": 7}
    assert (_hip.OP_SGPR_ANYD, _hip.OP_KMM_LAMBDA_ANYD, _hip.OP_KXX_NOISE_ANYD) == (5, 6, 7)
    assert (_hip.OP_DENSE, _hip.OP_SGPR, _hip.OP_KMM_LAMBDA, _hip.OP_KXX_NOISE, _hip.OP_KMM_LAMBDA_WIDE) == (0, 1, 2, 3, 4)


def test_other_headers_symbol_sets_untouched():
    from cggp import _hip
    names = declared_symbols()
    assert not set(NAMES) & set(names) and "mgp_knm_matvec" in names
    assert sorted(_hip.SIGNATURES) == names
    assert anyd_symbols() == sorted(_hip.ANYD_SIGNATURES) == ["mgp_kmn_knm_vjp_anyd"]
    tables = (_hip.SIGNATURES, _hip.EXT_SIGNATURES, _hip.ANYD_SIGNATURES, _hip.SWEEP_ANYD_SIGNATURES)
    assert sum(len(t) for t in tables) == len(set().union(*tables))  # pairwise disjoint
    assert _hip.MGP_VERSION == 210
    text = open(os.path.join(ROOT, "include", "mgp.h")).read()
    assert re.search(r"#define MGP_VERSION (\d+)", text).group(1) == "210"


def test_header_compiles_as_c(lib, tmp_path):  # noqa: F811
    from cggp import _hip
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "sweep_anyd_probe.c"
    src.write_text(_PROBE)
    exe = tmp_path / "sweep_anyd_probe"
    libdir = os.path.dirname(_hip.lib_path())
    cmd = ["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o",
           str(exe), "-L", libdir, "-l:libmgp.so", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib",
           "-Wl,--allow-shlib-undefined"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ["-1", "-1", "-1", "5", "6", "7", str(_hip.MGP_VERSION)]


def test_null_handle_is_badarg(lib):  # noqa: F811
    assert lib.mgp_knm_matvec_anyd(None, None, None, 0, None, 0, None, 0, 0, None, 0) == -1
    assert lib.mgp_kmn_matvec_anyd(None, None, None, 0, None, 0, None, 0, 0, None, 0) == -1
    assert lib.mgp_kxx_matvec_anyd(None, None, None, 0, 0.0, None, 0, 0, None, 0) == -1


def test_fused_anyd_setting_is_checked():
    from cggp import conjugate_gradient as cgm
    import torch
    for ok in (False, True, "auto"):
        assert cgm.check_fused_anyd(ok) is ok or cgm.check_fused_anyd(ok) == ok
    for bad in (None, 1, 0, "yes", "Auto"):
        with pytest.raises(ValueError):
            cgm.check_fused_anyd(bad)
    # fp32 and D <= 32 never qualify for "auto"; True is True everywhere (libmgp falls back by itself)
    assert not cgm.fused_anyd_auto(torch.float32, 77) and not cgm.fused_anyd_auto(torch.float64, 32)
    assert cgm.use_fused_anyd(True, torch.float32, 8) and not cgm.use_fused_anyd(False, torch.float64, 77)
    assert cgm.use_fused_anyd("auto", torch.float64, 77) == cgm.fused_anyd_auto(torch.float64, 77)
