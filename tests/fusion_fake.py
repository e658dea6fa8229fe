"""The CPU stand-in of tests/regions_fake.py with the three calls of csrc/fusion.hip added, from their restatement
(tests/fusion_ref.py): ops.sensor_fusion and the session's plumbing around it run end to end without a GPU.  The product never does
this."""
import numpy as np
import torch

from gw_depth_amd import hip
from tests import fusion_ref as F
from tests.regions_fake import RegionsFakeDevice


class FusionFakeDevice(RegionsFakeDevice):
    def __init__(self):
        super().__init__()
        self.fusion_calls = []

    def workspace_bytes(self, op, *dims):
        if op == hip.WS_FUSION:
            return 256
        return super().workspace_bytes(op, *dims)

    def fusion_ring(self, labels, sensor_mm, depth_mm, sizes, region_map, region_count, max_regions, ring, gap, lo_mm, hi_mm, align,
                    min_align, workspace, fusion_ring, fusion_scale):
        self.fusion_calls.append(("fusion_ring", dict(max_regions=max_regions, ring=ring, gap=gap, lo_mm=lo_mm, hi_mm=hi_mm, align=align,
                                                      min_align=min_align)))
        self.ring_args = dict(ring=ring, gap=gap, lo_mm=lo_mm, hi_mm=hi_mm)
        for b, (fh, fw) in enumerate(sizes.numpy().tolist()):
            K = min(max(int(region_count[b]), 0), max_regions)
            cut = (b, slice(0, fh), slice(0, fw))
            ring_b, near = F.ring_map(labels.numpy()[cut], sensor_mm.numpy()[cut], region_map.numpy()[cut], K, ring, gap, lo_mm, hi_mm)
            fusion_ring[b].zero_()
            fusion_ring[b, :fh, :fw] = torch.from_numpy(ring_b)
            n, sp, pp = F.scale_sums(labels.numpy()[cut], sensor_mm.numpy()[cut], depth_mm.numpy()[cut], near, lo_mm, hi_mm)
            fusion_scale[b] = torch.tensor([F.scale_of(n, sp, pp, align, min_align), n, sp, pp], dtype=torch.float64)

    def fusion_planes(self, fusion_ring, sensor_mm, sizes, region_count, records, ring, lo_mm, hi_mm, trim, min_ring, max_rms, workspace,
                      fusion_planes):
        self.fusion_calls.append(("fusion_planes", dict(ring=ring, trim=trim, min_ring=min_ring, max_rms=max_rms)))
        fusion_planes.zero_()
        for b, (fh, fw) in enumerate(sizes.numpy().tolist()):
            for r in range(min(max(int(region_count[b]), 0), fusion_planes.shape[1])):
                x, y, w = F.ring_samples(fusion_ring.numpy()[b, :fh, :fw], sensor_mm.numpy()[b, :fh, :fw], r)
                fusion_planes[b, r] = torch.from_numpy(F.fit_region(x, y, w, trim, min_ring, max_rms))

    def fusion_depth(self, labels, sensor_mm, depth, sizes, region_map, region_count, fusion_planes, fusion_scale, lo_mm, hi_mm, dmin,
                     dmax, depth_fused, depth_fused_mm, fused_source):
        self.fusion_calls.append(("fusion_depth", dict(lo_mm=lo_mm, hi_mm=hi_mm, min_depth=dmin, max_depth=dmax)))
        for t in (depth_fused, depth_fused_mm, fused_source):
            t.zero_()
        for b, (fh, fw) in enumerate(sizes.numpy().tolist()):
            K = min(max(int(region_count[b]), 0), fusion_planes.shape[1])
            cut = (b, slice(0, fh), slice(0, fw))
            d, mm, src, _ = F.fused_depth(labels.numpy()[cut], sensor_mm.numpy()[cut], depth.numpy()[cut], region_map.numpy()[cut], K,
                                          fusion_planes.numpy()[b], float(fusion_scale[b, 0]), lo_mm, hi_mm, dmin, dmax)
            depth_fused[b, :fh, :fw] = torch.from_numpy(d)
            depth_fused_mm[b, :fh, :fw] = torch.from_numpy(mm)
            fused_source[b, :fh, :fw] = torch.from_numpy(src)
