"""The CPU stand-in of tests/cloud_fake.py with gwd_scene_reset / gwd_scene_integrate / gwd_scene_extract added from their statement
(tests/scene_ref.py): cloud.SceneMap, ops.scene_merge and the session's plumbing around them run end to end without a GPU.  A map's
contents live in a statement object keyed by the address of its state block; the state block itself is written as the kernels write
it.  The existing stand-ins are composed, not edited.  The product never does this."""
import torch

from gw_depth_amd import hip
from tests import scene_ref as S
from tests.cloud_fake import CloudFakeDevice


class SceneFakeDevice(CloudFakeDevice):
    def __init__(self):
        super().__init__()
        self.scene_calls = []
        self.maps = {}

    def workspace_bytes(self, op, *dims):
        if op == hip.WS_SCENE:
            return 64
        return super().workspace_bytes(op, *dims)

    def _note(self, what, desc, tensors, **kw):
        hip.HipLibrary.scene_desc(*tensors, desc.voxel, list(desc.origin))      # the binding's own checks (no device work)
        self.scene_calls.append(dict(what=what, after=(len(self.cloud_calls), len(self.render_calls)), **kw))
        return desc.state

    def _publish(self, tensors, ref):
        st = ref.state()
        tensors[4].copy_(torch.tensor([st[k] for k in hip.SCENE_STATE] + [0, 0, 0], dtype=torch.int64))

    def scene_reset(self, desc, tensors):
        at = self._note("reset", desc, tensors)
        self.maps[at] = S.SceneMap(desc.voxel, desc.max_voxels, tuple(desc.origin))
        self._publish(tensors, self.maps[at])

    def scene_integrate(self, desc, tensors, cloud, cloud_offsets, workspace):
        hip.HipLibrary.scene_cloud_check("gwd_scene_integrate", cloud, cloud_offsets)
        if cloud.shape[0] < 1 or workspace.numel() < self.workspace_bytes(hip.WS_SCENE, cloud.shape[0], desc.max_voxels):
            raise ValueError("gwd_scene_integrate: rows / workspace")
        at = self._note("integrate", desc, tensors, cloud=cloud, rows=int(cloud.shape[0]))
        self.maps[at].integrate(cloud.numpy(), cloud_offsets.numpy())
        self._publish(tensors, self.maps[at])

    def scene_extract(self, desc, tensors, min_obs, keep, workspace, cloud, cloud_offsets, voxel_stats):
        hip.HipLibrary.scene_cloud_check("gwd_scene_extract", cloud, cloud_offsets)
        if tuple(cloud.shape) != (desc.max_voxels, 32) or tuple(voxel_stats.shape) != (desc.max_voxels, 4) or cloud_offsets.numel() != 2:
            raise ValueError("gwd_scene_extract: operand sizes")
        at = self._note("extract", desc, tensors, min_obs=min_obs, keep=keep)
        out = self.maps[at].extract(min_obs, keep)
        for dst, k in ((cloud, "cloud"), (cloud_offsets, "cloud_offsets"), (voxel_stats, "voxel_stats")):
            dst.copy_(torch.from_numpy(out[k]))
