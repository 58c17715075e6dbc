#!/usr/bin/env python3
"""Generate tests/golden/plan_layout.json: what the ABI shows of the engine's shape-bound plan, per lifecycle row.

Reads nothing but the built library (stcd_configure touches no device, so no GPU is needed):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_plan_layout.py

One entry per (row of tests/lifecycle_spec.ROWS, stcd_set_debug 0 / 1), configured at the row's S1: workspace bytes, dropout
floats, output floats, the number of named workspace tensors and a SHA-256 over tests/_util.plan_values (see plan_layout there).
Regenerate ONLY with a change that is meant to move bytes of the workspace plan, and say so in that change: a refactor of the
plan builders must reproduce this file as it is (tests/test_plan_layout_cpu.py).
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
sys.dont_write_bytecode = True

from stcd_amd import _lib                               # noqa: E402
from tests import lifecycle_spec as L                   # noqa: E402
from tests._util import plan_layout                     # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "plan_layout.json")


def record(row, debug):
    l = _lib.lib()
    m = row.make()
    _lib.check(l.stcd_set_debug(m._engine._h, debug))
    _lib.check(l.stcd_configure(m._engine._h, *row.s1))
    return plan_layout(m)


def main():
    out = {f"{row.id}/debug{debug}": record(row, debug) for row in L.ROWS for debug in (0, 1)}
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {OUT}: {len(out)} cases")


if __name__ == "__main__":
    main()
