#!/usr/bin/env python
"""Writes tests/golden/point_cloud.npz from the statement (tests/cloud_ref.py) over the seeded scene of tests/cloud_cases.py:

    python tools/make_cloud_golden.py

It holds the scene's operands and, for the configurations of cloud_cases.RECORDED, the cloud and offsets the statement gives.
Nothing here comes from the reference project or from a GPU: tests/test_point_cloud.py regenerates every array and compares."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import cloud_cases as K       # noqa: E402


def main():
    sc = K.scene()
    gold = K.arrays(sc)
    for cfg in K.RECORDED:
        out = K.statement(sc, cfg)
        gold["%s.cloud" % K.config_id(cfg)] = out["cloud"]
        gold["%s.cloud_offsets" % K.config_id(cfg)] = out["cloud_offsets"]
    os.makedirs(os.path.dirname(K.GOLDEN), exist_ok=True)
    np.savez_compressed(K.GOLDEN, **gold)
    print("%s: %d arrays, %d bytes" % (K.GOLDEN, len(gold), os.path.getsize(K.GOLDEN)))


if __name__ == "__main__":
    main()
