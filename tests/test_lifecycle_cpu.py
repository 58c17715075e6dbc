"""The shape-bound plan of a reused engine, checked without a GPU (stcd_configure touches no device).

Every row of tests/lifecycle_spec.py is created through the C ABI and configured S1, S2, S1: every call succeeds (so the table of
shapes is one the GPU test can run), the plan differs between S1 and S2, and the second S1 reproduces the first S1's plan exactly
-- workspace bytes, the Dropout2d table, every named workspace tensor, ChangeFormer's output layout and dropout sites, the
gradient stage ranges.  stcd_configure resets the dozen vectors and counters every configure_* rebuilds in one place
(reset_plan); a vector left out of that reset lets a table grow and fails here (tried: without `e.ws_tensors.clear()` all 32
cases fail).
The two lifecycle guards that need no device answer as well.
"""
import ctypes as C

import pytest

from stcd_amd import _lib
from tests import lifecycle_spec as L
from tests._util import plan_values


@pytest.mark.parametrize("debug", [0, 1])
@pytest.mark.parametrize("row", L.ROWS, ids=[r.id for r in L.ROWS])
def test_configure_s1_s2_s1_reproduces_the_plan(row, debug):
    """debug = 1 is stcd_set_debug(1): every layer's input gradient in a buffer of its own, the plan the in-place tests read.
    Families without Dropout2d (SNUNet, SegCD, ResNet, BIT; ChangeFormer's masks are hashed per site) have an empty table at every
    shape; where there is a table its rows and offsets follow the batch, and ChangeFormer's sites follow the map size."""
    l = _lib.lib()
    m = row.make()
    h = m._engine._h
    _lib.check(l.stcd_set_debug(h, debug))
    seen = []
    for shape in (row.s1, row.s2, row.s1):
        assert l.stcd_configure(h, *shape) == 0, f"{row.id}: stcd_configure{shape} refused: {l.stcd_last_error().decode()}"
        seen.append(plan_values(m))
    a, b, c = seen
    assert row.s1[0] != row.s2[0] and row.s1[1:] != row.s2[1:]
    assert a["workspace_bytes"] > 0 and a["workspace_bytes"] != b["workspace_bytes"]
    if row.pin == "masks":
        assert a["dropout"] and [(n, r, o) for n, r, _, o in a["dropout"]] != [(n, r, o) for n, r, _, o in b["dropout"]]
        assert [n for n, *_ in a["dropout"]] == [n for n, *_ in b["dropout"]]
    else:
        assert a["dropout"] == [] and b["dropout"] == []
    if m._engine.arch == "changeformer":
        assert a["cf_sites"] and a["cf_sites"] != b["cf_sites"] and a["cf_outputs"] != b["cf_outputs"]
        assert len(a["cf_sites"]) == len(b["cf_sites"])
    if a["ws_tensors"]:
        assert len(a["ws_tensors"]) == len(b["ws_tensors"]) and a["ws_tensors"] != b["ws_tensors"]
        assert len({t[0] for t in a["ws_tensors"]}) == len(a["ws_tensors"]), "a workspace tensor is listed twice"
    for k in a:
        assert a[k] == c[k], f"{row.id}: {k} of the second S1 configuration differs from the first"


def test_the_two_guards_that_need_no_device_answer():
    l = _lib.lib()
    h = C.c_void_p()
    assert l.stcd_create(_lib.ARCH_DIFF, 3, 2, _lib.DTYPE_BF16, C.byref(h)) == 0
    try:
        assert l.stcd_forward(h, None, None, None, None, None, 0, 1, None, None, None) != 0
        assert b"not configured" in l.stcd_last_error()
        assert l.stcd_configure(h, 2, 32, 32) == 0
        for stage in (-1, 0, 1):
            assert l.stcd_backward(h, None, None, None, None, stage, None) != 0
            assert b"backward requires a preceding training-mode forward" in l.stcd_last_error()
    finally:
        l.stcd_destroy(h)
