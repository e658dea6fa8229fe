#!/usr/bin/env python
"""Writes tests/golden/render.npz and tests/golden/render_lut.npy from the statement (tests/render_ref.py) over the seeded cases of
tests/render_cases.py:

    python tools/make_render_golden.py

render.npz holds, per case, the array operands and the canvas the statement gives; render_lut.npy the default 256 x 3 table.
Nothing here comes from the reference project or from a GPU: tests/test_render.py regenerates every array and compares."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import render_cases as K      # noqa: E402
from tests import render_ref as P        # noqa: E402


def arrays(name, case):
    out = {}
    for key in ("sizes", "lines", "count", "order", "scores", "kinds", "region_map"):
        if case[key] is not None:
            out["%s.%s" % (name, key)] = np.asarray(case[key])
    for key in ("planes", "label_planes"):
        for i, v in enumerate(case[key]):
            out["%s.%s%d" % (name, key, i)] = np.asarray(v)
    for b, f in enumerate(case["frames"] or []):
        out["%s.frame%d" % (name, b)] = f
    out["%s.canvas" % name] = K.statement(case)
    return out


def main():
    gold = {}
    for name, make in K.CASES.items():
        gold.update(arrays(name, make()))
    os.makedirs(os.path.dirname(P.GOLDEN), exist_ok=True)
    np.savez_compressed(P.GOLDEN, **gold)
    np.save(P.GOLDEN_LUT, P.jet_table())
    print("%s: %d arrays, %d bytes; %s: %d bytes" % (P.GOLDEN, len(gold), os.path.getsize(P.GOLDEN), P.GOLDEN_LUT, os.path.getsize(P.GOLDEN_LUT)))


if __name__ == "__main__":
    main()
