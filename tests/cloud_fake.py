"""The CPU stand-in of tests/render_fake.py with gwd_point_cloud added from its statement (tests/cloud_ref.py): ops.point_cloud and the
session's plumbing around it run end to end without a GPU.  The existing stand-ins are composed, not edited.  The product never does
this."""
import numpy as np
import torch

from gw_depth_amd import hip
from tests import cloud_ref as C
from tests.render_fake import RenderFakeDevice


class CloudFakeDevice(RenderFakeDevice):
    def __init__(self):
        super().__init__()
        self.cloud_calls = []

    def workspace_bytes(self, op, *dims):
        if op == hip.WS_CLOUD:
            return 256
        return super().workspace_bytes(op, *dims)

    def point_cloud(self, depth, labels, sizes, intrinsics, frames, region_map, region_count, planes, source, poses, frame_sizes, stride,
                    min_depth, max_depth, edge, normals, keep, workspace, cloud, cloud_offsets):
        d = hip.HipLibrary.cloud_desc(depth, labels, sizes, intrinsics, frames, region_map, region_count, planes, source, poses, frame_sizes,
                                      stride, min_depth, max_depth, edge, normals, keep, workspace, cloud, cloud_offsets)       # the binding's own checks
        if hip.HipLibrary.cloud_worst_case(d) > d.capacity:
            raise ValueError("gwd_point_cloud: capacity")
        self.cloud_calls.append(dict(depth=depth, shape=tuple(depth.shape), frames=frames is not None, region_map=region_map is not None,
                                     source=source is not None, poses=poses is not None, frame_sizes=frame_sizes, stride=stride,
                                     min_depth=min_depth, max_depth=max_depth, edge=edge, normals=normals, keep=keep,
                                     capacity=int(cloud.shape[0]),
                                     after=(len(self.region_calls), len(self.profile_calls), len(self.fusion_calls), len(self.render_calls))))
        n = lambda t: None if t is None else t.numpy()
        ext = np.array([(d.ext_h[b], d.ext_w[b]) for b in range(d.B)], dtype=np.int32)      # sizes is clamped to what the host knows
        out = C.point_cloud(n(depth), n(labels), np.clip(n(sizes), 0, ext), n(intrinsics), None if frames is None else [n(f) for f in frames], n(region_map),
                            n(region_count), n(planes), n(source), n(poses), stride, min_depth, max_depth, edge, normals, keep,
                            capacity_rows=cloud.shape[0])
        cloud.copy_(torch.from_numpy(out["cloud"]))
        cloud_offsets.copy_(torch.from_numpy(out["cloud_offsets"]))
