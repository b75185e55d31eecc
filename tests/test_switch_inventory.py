"""Every environment switch libmgp reads is documented and tested (CPU).

Scans csrc/ for getenv("MGP_...") and checks each name against DESIGN section 4.8 and against the table of
tests/switch_forms.py (rows run by tests/test_gpu_switch_forms.py) or its exemption map, whose values name a
covering test that must exist or give a reason.  A switch added later without a test fails here.
"""

import glob
import os
import re
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "conjugate-gradient-sparse-gp_amd", "csrc")
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import switch_forms as sf  # noqa: E402


def csrc_switches():
    names = set()
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.cpp"))):
        with open(path) as f:
            names.update(re.findall(r'getenv\("(MGP_[A-Z0-9_]+)"\)', f.read()))
    return names


def design_switch_section():
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        text = f.read()
    start = text.index("### 4.8 ")
    end = text.index("\n## ", start)
    return text[start:end]


def test_the_scan_finds_the_switches():
    names = csrc_switches()
    assert len(names) >= 30 and {"MGP_SWEEP", "MGP_CONTRACT", "MGP_RFF_ROUTE", "MGP_D1_TRACE"} <= names


@pytest.mark.parametrize("name", sorted(csrc_switches()))
def test_switch_has_a_design_row(name):
    rows = [ln for ln in design_switch_section().splitlines() if ln.startswith("|")]
    assert any(f"`{name}`" in ln.split("|")[1] for ln in rows), f"{name} has no row in DESIGN.md section 4.8"


@pytest.mark.parametrize("name", sorted(csrc_switches()))
def test_switch_is_tested_or_exempt(name):
    in_table = name in sf.table_switches()
    assert in_table or name in sf.EXEMPT, f"{name} has no row in tests/switch_forms.py and no exemption"
    assert not (in_table and name in sf.EXEMPT), f"{name} is both a table row and exempt"


@pytest.mark.parametrize("name", sorted(sf.EXEMPT))
def test_exemption_names_an_existing_test_or_a_reason(name):
    why = sf.EXEMPT[name]
    assert name in csrc_switches(), f"exemption for {name}, which csrc/ does not read"
    if "::" in why:
        path, test = why.split("::")
        with open(os.path.join(ROOT, path)) as f:
            assert re.search(rf"^def {re.escape(test)}\(", f.read(), re.M), why
    else:
        assert len(why.split()) >= 4, f"{name}: a reason, not a word"


def test_table_rows_set_only_switches_csrc_reads():
    unknown = sf.table_switches() - csrc_switches()
    assert not unknown, unknown
    ids = [row["id"] for row in sf.FORMS]
    assert len(ids) == len(set(ids))
    for row in sf.FORMS:
        assert row["cases"] and row["entry"] and row["routes"] and row["ref"] and row["bar"], row["id"]


@pytest.mark.parametrize("case", sf.CHUNK_CASES, ids=lambda c: f"{c[6]}")
def test_chunk_cases_take_the_block_decode_they_name(case):
    env, _, D, N, M, R, branch = case
    assert sf.decode_branch(sf.fast_chunks(env, D, N, M, R)) == branch


def test_chunk_cases_cover_every_decode_with_one_and_several_columns():
    seen = {(c[6], c[5] > 1) for c in sf.CHUNK_CASES}
    assert seen == {(b, m) for b in ("xcd8", "few", "linear") for m in (False, True)}
