"""The CPU stand-in of tests/scene_fake.py with gwd_cloud_view added from its statement (tests/view_ref.py): ops.cloud_view,
cloud.SceneMap.view and the session's scene_view= plumbing run end to end without a GPU.  The existing stand-ins are composed, not
edited.  The product never does this."""
import torch

from gw_depth_amd import hip
from tests import view_ref as W
from tests.scene_fake import SceneFakeDevice


class ViewFakeDevice(SceneFakeDevice):
    def __init__(self):
        super().__init__()
        self.view_calls = []

    def workspace_bytes(self, op, *dims):
        if op == hip.WS_VIEW:
            V, Fh, Fw = dims
            return (V * Fh * Fw * 8 + 15) // 16 * 16
        return super().workspace_bytes(op, *dims)

    def cloud_view(self, cloud, cloud_offsets, sizes, intrinsics, poses, view_sizes, min_depth, max_depth, footprint, max_splat, keep,
                   workspace, view_depth, view_index, view_labels, view_rgb):
        d = hip.HipLibrary.view_desc(cloud, cloud_offsets, sizes, intrinsics, poses, view_sizes, min_depth, max_depth, footprint, max_splat,
                                     keep, workspace, view_depth, view_index, view_labels, view_rgb)      # the binding's own checks
        if workspace.numel() < self.workspace_bytes(hip.WS_VIEW, d.V, d.Fh, d.Fw):
            raise ValueError("gwd_cloud_view: workspace")
        self.view_calls.append(dict(after=(len(self.cloud_calls), len(self.scene_calls)), rows=int(cloud.shape[0]), V=d.V, plane=(d.Fh, d.Fw),
                                    ext=[(d.ext_h[v], d.ext_w[v]) for v in range(d.V)], footprint=d.footprint, max_splat=d.max_splat,
                                    keep=keep, min_depth=d.min_depth, max_depth=d.max_depth))
        out = W.cloud_view(cloud.numpy(), cloud_offsets.numpy(), intrinsics.numpy(), sizes.numpy(), None if poses is None else poses.numpy(),
                           d.Fh, d.Fw, min_depth=d.min_depth, max_depth=d.max_depth, footprint=d.footprint, max_splat=d.max_splat, keep=keep,
                           ext=self.view_calls[-1]["ext"])
        for dst, k in ((view_depth, "view_depth"), (view_index, "view_index"), (view_labels, "view_labels"), (view_rgb, "view_rgb")):
            dst.copy_(torch.from_numpy(out[k]))
