"""The CPU stand-in of tests/test_frames_post.py with the three calls of csrc/regions.hip added, from their restatement
(tests/regions_ref.py): ops.glass_regions and the session's plumbing around it run end to end without a GPU.  The product never does
this."""
import torch

from gw_depth_amd import hip
from tests import regions_ref as R
from tests.test_frames_post import FramesFakeDevice


class RegionsFakeDevice(FramesFakeDevice):
    def __init__(self):
        super().__init__()
        self.region_calls = []

    def workspace_bytes(self, op, *dims):
        if op == hip.WS_REGIONS:
            return 256
        return super().workspace_bytes(op, *dims)

    def glass_regions(self, labels, depth_mm, sizes, max_regions, min_area, connectivity, max_candidates, lo_mm, hi_mm, workspace,
                      region_map, region_count, region_total, records):
        self.region_calls.append(("glass_regions", dict(max_regions=max_regions, min_area=min_area, connectivity=connectivity,
                                                        max_candidates=max_candidates, lo_mm=lo_mm, hi_mm=hi_mm)))
        self.range = (lo_mm, hi_mm)
        out = R.glass_regions(labels.numpy(), depth_mm.numpy(), sizes.numpy(), max_regions, min_area, connectivity, lo_mm, hi_mm, max_candidates)
        for dst, k in ((region_map, "region_map"), (region_count, "region_count"), (region_total, "region_total"), (records, "regions")):
            dst.copy_(torch.from_numpy(out[k]))

    def region_planes(self, region_map, depth_mm, sizes, region_count, records, lo_mm, hi_mm, workspace, planes):
        self.region_calls.append(("region_planes", {}))
        planes.copy_(torch.from_numpy(R.region_planes(region_map.numpy(), depth_mm.numpy(), region_count.numpy(), planes.shape[1], lo_mm, hi_mm)))

    def depth_planar(self, region_map, depth_mm, depth, sizes, region_count, planes, dmin, dmax, depth_planar, depth_planar_mm):
        self.region_calls.append(("depth_planar", {"from_depth": depth is not None}))
        d, mm, _, _ = R.depth_planar(region_map.numpy(), depth_mm.numpy(), None if depth is None else depth.numpy(), sizes.numpy(),
                                     region_count.numpy(), planes.numpy(), dmin, dmax)
        depth_planar.copy_(torch.from_numpy(d))
        depth_planar_mm.copy_(torch.from_numpy(mm))
