"""The CPU stand-in of tests/regions_fake.py (and tests/line_nms_fake.py) with gwd_line_profiles added, from its statement
(tests/line_profile_ref.py): ops.line_profiles and the session's plumbing around it run end to end without a GPU.  The product never
does this."""
import torch

from tests import line_profile_ref as P
from tests.line_nms_fake import LineNmsFakeDevice
from tests.regions_fake import RegionsFakeDevice


class LineProfileFakeDevice(RegionsFakeDevice, LineNmsFakeDevice):
    def __init__(self):
        super().__init__()
        self.profile_calls = []

    def line_profiles(self, lines, count, order, labels, depth_mm, sizes, region_map, intrinsics, offset, max_samples, lo_mm, hi_mm,
                      hi, lo, counts, fits, kind, line_points):
        self.profile_calls.append(dict(rows=tuple(lines.shape[:2]), dtype=lines.dtype, order=order is not None, region_map=region_map is not None,
                                       intrinsics=intrinsics is not None, offset=offset, max_samples=max_samples, lo_mm=lo_mm, hi_mm=hi_mm,
                                       hi=hi, lo=lo, after=len(self.region_calls)))
        n = lambda t: None if t is None else t.numpy()
        out = P.line_profiles(n(lines), n(count), n(labels), n(depth_mm), n(sizes), n(order), n(region_map), n(intrinsics), offset,
                              max_samples, lo_mm, hi_mm, hi, lo)
        for dst, k in ((counts, "profile_counts"), (fits, "profile_fits"), (kind, "profile_kind"), (line_points, "line_points")):
            if dst is not None:
                dst.copy_(torch.from_numpy(out[k]))
