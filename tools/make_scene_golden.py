"""Writes tests/golden/scene_map.npz from the statement (tests/scene_ref.py): the clouds that tests/cloud_ref.py makes of the
point-cloud fixture, merged at the three voxel sizes, in one call and frame by frame.  Run from the repository root:
    python tools/make_scene_golden.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import scene_cases as K  # noqa: E402
from tests import scene_ref as S  # noqa: E402


def main():
    whole, parts = K.fixture_clouds()
    out = {}
    for voxel in K.VOXELS:
        for split in (False, True):
            res = S.merge(parts if split else [whole], voxel, K.FIXTURE_MAX_VOXELS, K.ORIGIN)
            kept = int(res["cloud_offsets"][1])
            assert not res["cloud"][kept:].any() and not res["voxel_stats"][kept:].any()
            out["%s.cloud" % K.golden_id(voxel, split)] = res["cloud"][:kept]          # the zero tail is not stored
            out["%s.voxel_stats" % K.golden_id(voxel, split)] = res["voxel_stats"][:kept]
    np.savez_compressed(K.GOLDEN, **out)
    print("%s: %d bytes, voxels %s" % (K.GOLDEN, os.path.getsize(K.GOLDEN), {k: v.shape[0] for k, v in out.items() if k.endswith("cloud")}))


if __name__ == "__main__":
    main()
