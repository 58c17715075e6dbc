"""The shape-bound plan is byte for byte the plan it was, checked without a GPU (stcd_configure touches no device).

tests/golden/plan_layout.json holds, for every row of tests/lifecycle_spec.py at its S1 with stcd_set_debug 0 and 1, what the
ABI shows of the plan: workspace bytes, dropout floats, output floats, the number of named workspace tensors and a SHA-256 over
the canonical text of tests/_util.plan_values (every Dropout2d row, every named workspace tensor with its offset, ChangeFormer's
output layout and dropout sites, the gradient stage ranges).  A change of the plan builders (the geometry constructors, the
workspace planner, a configure_*) that moves one byte of a workspace without meaning to fails here, on the CPU, before it is an
out-of-bounds access on a GPU.
"""
import json
import os

import pytest

from stcd_amd import _lib
from tests import lifecycle_spec as L
from tests._util import plan_layout

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan_layout.json")
with open(GOLDEN) as _f:
    EXPECTED = json.load(_f)


@pytest.mark.parametrize("debug", [0, 1])
@pytest.mark.parametrize("row", L.ROWS, ids=[r.id for r in L.ROWS])
def test_plan_layout_is_the_recorded_one(row, debug):
    case = f"{row.id}/debug{debug}"
    l = _lib.lib()
    m = row.make()
    h = m._engine._h
    _lib.check(l.stcd_set_debug(h, debug))
    assert l.stcd_configure(h, *row.s1) == 0, f"{case}: stcd_configure{row.s1} refused: {l.stcd_last_error().decode()}"
    got = plan_layout(m)
    assert case in EXPECTED, f"{case}: no recorded plan; record it with `python tests/golden/make_plan_layout.py`"
    assert got == EXPECTED[case], (
        f"{case}: the plan at {row.s1} is not the recorded one: got {got}, recorded {EXPECTED[case]}.  If the workspace plan is "
        f"MEANT to change, regenerate with `python tests/golden/make_plan_layout.py` and say so in the change.")


def test_every_recorded_case_is_still_a_row():
    assert set(EXPECTED) == {f"{r.id}/debug{d}" for r in L.ROWS for d in (0, 1)}
