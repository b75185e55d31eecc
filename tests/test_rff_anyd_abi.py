"""MGP_RFF_ANYD at the C boundary (no GPU needed): the flag is an enum block of its own in include/mgp_pathwise.h with
the value 16, the header still compiles as plain C and prints it, cggp/_hip.py binds the same value, the header states
the contract, no function, header or signature table was added and the library version is untouched; the `rff_anyd`
setting is checked where it enters, before any device call; and the constants of `rff.rff_anyd_auto` are what
tools/run_rff_anyd.py derives from profiles/rff_anyd_times.json."""

import importlib.util
import os
import re
import shutil
import subprocess

import pytest

from test_abi import ROOT, declared_symbols, lib  # noqa: F401  (`lib` is the module fixture of test_abi)
from test_abi_pathwise import pathwise_symbols

_PROBE = r"""
#include <stdio.h>
#include "mgp_pathwise.h"
int main(void) {
  printf("%d %d %d\n", MGP_RFF_ANYD, MGP_ROWS | MGP_RFF_ANYD, MGP_COLS | MGP_RFF_ANYD);
  return 0;
}
"""


def _header(strip_comments=True):
    text = open(os.path.join(ROOT, "include", "mgp_pathwise.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S) if strip_comments else text


def test_enum_value_in_a_block_of_its_own():
    from cggp import _hip
    blocks = re.findall(r"enum\s*\{([^}]*)\}", _header())
    assert len(blocks) == 1
    vals = {k.strip(): int(v) for k, v in (item.split("=") for item in blocks[0].split(","))}
    assert vals == {"MGP_RFF_ANYD": 16}
    assert _hip.RFF_ANYD == 16 and not _hip.RFF_ANYD & (_hip.ROWS | _hip.COLS)


def test_header_compiles_as_c_and_prints_the_value(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "rff_anyd_probe.c"
    src.write_text(_PROBE)
    exe = tmp_path / "rff_anyd_probe"
    cmd = ["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o",
           str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.split() == ["16", "17", "16"]


def test_header_comment_states_the_contract():
    text = re.sub(r"\s*\n \*\s*", " ", _header(strip_comments=False))
    for phrase in ("OR into out_layout of mgp_rff_sample or g_layout of mgp_rff_sample_vjp",
                   "any other bit: MGP_E_BADARG", "MGP_FUSED_MAX_D < D <= MGP_MAX_D and 1 <= S <= 8",
                   "exactly that of the plain call, with its bits and its refusals",
                   "mgp_rff_sample_vjp still refuses D > MGP_FUSED_MAX_D",
                   "v_mfma_f64_16x16x4_f64", "slices of 8 k-steps, k ascending",
                   "groups = ceil(D / 256)", "every group recomputes the phases",
                   "wg      = ceil(owned / 64) * groups",
                   "nsplit  = wg >= 2 CUs ? 1 : max(1, min(ceil(2 CUs / wg), ceil(stiles / 16), 256))",
                   "tps     = ceil(stiles / nsplit),  nsplit = ceil(stiles / tps),  len = 16 tps",
                   'the arena "gen" alone', "a(512 KS To) + a(512 KS Ts) + a(4096 Ts)",
                   "a(512 KS To) + a(512 KS Ts) + a(2048 To) + a(2048 Ts)", "a(8 nsplit owned DT)",
                   "No float atomics: two calls give the same bits",
                   "MGP_E_NOMEM from a fixed pool that is too small, never an allocation",
                   "u (8 + (K + 2) P + 2 len + nsplit + 2)", "u (8 + (K + 2) P + S + len + nsplit + 4)",
                   "nothing is kept on the handle between calls"):
        assert phrase in text, phrase


def test_no_function_header_or_signature_table_was_added():
    from cggp import _hip
    assert pathwise_symbols() == ["mgp_rff_sample_vjp"] == sorted(_hip.EXT_SIGNATURES)
    assert sorted(_hip.SIGNATURES) == declared_symbols()
    tables = sorted(t for t in dir(_hip) if t.endswith("SIGNATURES"))
    assert tables == ["ANYD_SIGNATURES", "EXT_SIGNATURES", "POINTS_SIGNATURES", "PREDICT_SIGNATURES", "SIGNATURES",
                      "SWEEP_ANYD_SIGNATURES"]
    assert not [n for t in tables for n in getattr(_hip, t) if "rff_anyd" in n]
    assert len(_hip.SIGNATURES["mgp_rff_sample"][1]) == 12 and len(_hip.EXT_SIGNATURES["mgp_rff_sample_vjp"][1]) == 14
    assert sorted(os.listdir(os.path.join(ROOT, "include"))) == [
        "mgp.h", "mgp_anyd.h", "mgp_pathwise.h", "mgp_points.h", "mgp_predict.h", "mgp_sweep_anyd.h"]
    assert _hip.MGP_VERSION == 210
    text = open(os.path.join(ROOT, "include", "mgp.h")).read()
    assert re.search(r"#define MGP_VERSION (\d+)", text).group(1) == "210"


def test_library_exports_no_rff_anyd_symbol(lib):  # noqa: F811
    from cggp import _hip
    if shutil.which("nm") is None:
        pytest.skip("no nm")
    out = subprocess.run(["nm", "-D", "--defined-only", _hip.lib_path()], capture_output=True, text=True, check=True)
    exported = {line.split()[-1] for line in out.stdout.splitlines() if line.strip()}
    assert not [s for s in exported if "rff_anyd" in s and not s.startswith("_Z")]


def test_kernel_file_is_built_and_only_dispatched_to():
    csrc = os.path.join(ROOT, "conjugate-gradient-sparse-gp_amd", "csrc")
    srcs = re.search(r"^SRCS := (.*)$", open(os.path.join(csrc, "Makefile")).read(), flags=re.M).group(1).split()
    assert "rff_anyd.hip" in srcs
    assert "mgp_rff_anyd_sample(" in open(os.path.join(csrc, "rff.hip")).read()
    assert "mgp_rff_anyd_vjp(" in open(os.path.join(csrc, "rff_grad.hip")).read()


def test_rff_anyd_setting_is_checked_before_any_device_call():
    import torch

    from cggp import models, rff, training
    for ok in (False, True, "auto"):
        assert rff.check_rff_anyd(ok) is ok or rff.check_rff_anyd(ok) == ok
    for bad in (None, 1, 0, "yes", "Auto"):
        with pytest.raises(ValueError, match="rff_anyd"):
            rff.check_rff_anyd(bad)
    f64 = torch.float64

    class _Kernel:  # a kernel that must not be asked: the refusal comes first
        variance = 1.0
        name = "se"

        def spec(self, D):
            raise AssertionError("the refusal comes first")

        @property
        def lengthscales(self):
            raise AssertionError("the refusal comes first")

    M = 12
    Z, lam = torch.zeros((M, 40), dtype=f64), torch.ones(M, dtype=f64)
    with pytest.raises(ValueError, match="rff_anyd must be"):
        rff.rff_sample(Z, _Kernel(), 8, 2, rff_anyd="on")
    with pytest.raises(ValueError, match="rff_anyd must be"):
        models.PathwiseClusterGP(_Kernel(), 0.3, Z, pseudo_u=lam, cluster_counts=lam, rff_anyd=2)
    for term, setting, err in (("batch", True, "data_term='pathwise'"), ("trace", "auto", "data_term='pathwise'"),
                               ("pathwise", 2, "rff_anyd must be"), ("batch", "on", "rff_anyd must be")):
        with pytest.raises(ValueError, match=err):
            models.CGGP(_Kernel(), 0.3, Z, None, data_term=term, rff_anyd=setting)
        with pytest.raises(ValueError, match=err):
            models.cdgp_class(_Kernel(), 0.3, Z, data_term=term, rff_anyd=setting)
        with pytest.raises(ValueError, match=err):
            training.TrainableCGGP(_Kernel(), 0.3, Z, pseudo_u=lam, cluster_counts=lam, data_term=term,
                                   rff_anyd=setting)
    # where True sends a call: only where libmgp serves the flag
    assert rff.use_rff_anyd(True, f64, 33, 8, 10, 10) and rff.use_rff_anyd(True, f64, 512, 1, 10, 10, "dX")
    assert not rff.use_rff_anyd(True, f64, 32, 5, 10, 10) and not rff.use_rff_anyd(True, f64, 77, 9, 10, 10)
    assert not rff.use_rff_anyd(True, torch.float32, 77, 5, 10, 10) and not rff.use_rff_anyd(False, f64, 77, 5, 10, 10)


def _tool():
    spec = importlib.util.spec_from_file_location("run_rff_anyd", os.path.join(ROOT, "tools", "run_rff_anyd.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_auto_constants_are_those_of_the_profile():
    """`rff.RFF_ANYD_AUTO` is the table tools/run_rff_anyd.py derives from the committed measurements by the house rule
    (at most 0.9 of the old route's time at every measured point of a region), and `rff_anyd_auto` follows it."""
    import torch

    from cggp import rff
    tool = _tool()
    doc = tool.load(os.path.join(ROOT, "profiles", "rff_anyd_times.json"))
    rows = doc["rows"]
    assert rows and all(r["old_ms"] > 0 and r["new_ms"] > 0 for r in rows)
    rule = tool.derive_rule(rows)
    assert rule == doc["rule"] and rule["margin"] == 0.9
    table = tool.auto_table(rule)
    assert table == rff.RFF_ANYD_AUTO
    for (op, S), (max_d, min_nl) in table.items():
        pts = [r for r in rows if r["op"] == op and r["S"] == S and r["D"] <= max_d and r["N"] * r["L"] >= min_nl]
        assert pts and all(r["new_over_old"] <= 0.9 for r in pts)
        assert rff.rff_anyd_auto(torch.float64, max_d, S, min_nl, 1, op)
        assert not rff.rff_anyd_auto(torch.float64, max_d + 1, S, min_nl, 1, op)
        assert not rff.rff_anyd_auto(torch.float64, max_d, S, min_nl - 1, 1, op)
        assert not rff.rff_anyd_auto(torch.float32, max_d, S, min_nl, 1, op)
        assert not rff.rff_anyd_auto(torch.float64, 32, S, min_nl, 1, op)
    assert not rff.rff_anyd_auto(torch.float64, 77, 3, 1 << 20, 1 << 12)  # a sample count that was not measured


def test_rule_on_made_up_rows():
    tool = _tool()
    row = lambda op, D, N, L, S, ratio: {"op": op, "D": D, "N": N, "L": L, "S": S, "new_over_old": ratio}
    rows = [row("forward", 77, 1 << 14, 1024, 5, 0.95), row("forward", 77, 1 << 17, 1024, 5, 0.5),
            row("forward", 128, 1 << 17, 1024, 5, 0.6), row("forward", 512, 1 << 17, 1024, 5, 1.2),
            row("dtheta", 77, 1 << 17, 1024, 5, 0.91)]
    rule = tool.derive_rule(rows)
    assert rule["regions"]["forward 5"] == {"max_d": 128, "min_nl": (1 << 17) * 1024, "points": 2}
    assert rule["regions"]["dtheta 5"] is None
    assert tool.auto_table(rule) == {("forward", 5): (128, (1 << 17) * 1024)}
