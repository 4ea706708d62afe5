"""The thin family's picks (csrc/conv_thin.hip: thin_conv_pick, thin_wgrad_pick) against a recorded table, on the CPU.

The plan path of the thin family is host arithmetic on the descriptor: dg_conv_plan / dg_wgrad_plan / dg_wgrad_has_sample_map
launch nothing and dereference none of the pointers, so every row carries non-null integers for them.  tests/golden/
thin_plans.json holds, per row, every descriptor field, the `force` code and what the library returned when the table was
recorded (tests/golden/make_thin_plans.py: the rows, each chosen to sit on one branch of the selection - kernel, template
range, grid cap, pass count, refusal).  Every row must come back exactly as recorded."""
import ctypes as C
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
TABLE = os.path.join(HERE, "golden", "thin_plans.json")
CONV_PLAN = ("family", "thin_mfma", "mask_bits", "dbias_rows", "sum_parts")
WGRAD_PLAN = ("variant", "splits", "ws_floats")


def fill(struct, desc):
    """a descriptor with exactly the recorded fields (every field of the struct is recorded)"""
    p = struct()
    names = [f[0] for f in struct._fields_]
    assert sorted(desc) == sorted(names), sorted(set(desc) ^ set(names))
    for k in names:
        setattr(p, k, desc[k])       # (pointers are recorded as integers, 0 = NULL)
    return p


def record(struct, p):
    return {f[0]: (getattr(p, f[0]) or 0) for f in struct._fields_}


def answer(L, lib, row):
    """what the library says about one row: the values the table records"""
    if row["pass"] == "conv":
        p, pl = fill(L.DgConv, row["desc"]), L.DgConvPlan()
        out = {"rc": lib.dg_conv_plan(C.byref(p), row["force"], 0, C.byref(pl))}
        out.update({k: getattr(pl, k) for k in CONV_PLAN})
        return out
    p, pl = fill(L.DgWgrad, row["desc"]), L.DgWgradPlan()
    out = {"rc": lib.dg_wgrad_plan(C.byref(p), row["accumulate"], row["force"], C.byref(pl))}
    out.update({k: getattr(pl, k) for k in WGRAD_PLAN})
    out["has_sample_map"] = lib.dg_wgrad_has_sample_map(C.byref(p), row["force"])
    return out


@pytest.fixture(scope="module")
def built():
    from dusty_gan_amd import _lib
    _lib.build()  # hipcc cross-compiles gfx950 without a GPU; a no-op when up to date
    return _lib


def test_thin_plans_match_the_recorded_table(built):
    rows = json.load(open(TABLE))
    lib = built.lib()
    assert sum(r["pass"] == "conv" for r in rows) >= 30 and sum(r["pass"] == "wgrad" for r in rows) >= 30
    bad = []
    for r in rows:
        got = answer(built, lib, r)
        if got != r["expect"]:
            bad.append((r["name"], r["force"], got, r["expect"]))
    assert not bad, bad
    # the table reaches every kernel of the family and both kinds of refusal-free fall-back
    thin = [r["expect"] for r in rows if r["force"] == built.DG_FORCE_THIN]
    assert {e["thin_mfma"] for e in thin if "thin_mfma" in e and e["rc"] == 0} == {0, 1, 2}
    assert {e["variant"] for e in thin if "variant" in e} == {0, built.DG_WGRAD_VARIANT_THIN, built.DG_WGRAD_VARIANT_THIN_MFMA}
    assert any(r["force"] == built.DG_FORCE_AUTO for r in rows)
