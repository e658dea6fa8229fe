"""The CPU stand-in of tests/fusion_fake.py and tests/line_profile_fake.py together, with gwd_render_frames added from its statement
(tests/render_ref.py): ops.render_frames and the session's plumbing around it run end to end without a GPU.  The existing stand-ins
are composed, not edited.  The product never does this."""
import torch

from gw_depth_amd import hip
from tests import render_ref as P
from tests.fusion_fake import FusionFakeDevice
from tests.line_profile_fake import LineProfileFakeDevice


class RenderFakeDevice(FusionFakeDevice, LineProfileFakeDevice):
    def __init__(self):
        super().__init__()
        self.render_calls = []

    def render_frames(self, canvas, sizes, tables, panels, frames, planes, label_planes, region_map, lines, count, order, scores, kinds, opts):
        hip.HipLibrary.render_desc(canvas, sizes, tables, panels, frames, planes, label_planes, region_map, lines, count, order, scores, kinds,
                                   opts)                  # the binding's own checks (no device work)
        self.render_calls.append(dict(shape=tuple(canvas.shape), panels=[dict(p) for p in panels], frames=frames is not None,
                                      planes=len(planes), label_planes=len(label_planes), region_map=region_map is not None,
                                      rows=None if lines is None else tuple(lines.shape[:2]), dtype=None if lines is None else lines.dtype,
                                      order=order is not None, scores=scores is not None, kinds=kinds is not None, opts=dict(opts),
                                      tables=int(tables.shape[0]),
                                      after=(len(self.region_calls), len(self.profile_calls), len(self.fusion_calls))))
        n = lambda t: None if t is None else t.numpy()
        views = lambda v: None if v is None else [n(t) for t in v]
        out = P.render(tuple(canvas.shape[:4]), n(sizes), n(tables), panels, views(frames), [views(v) for v in planes],
                       [views(v) for v in label_planes], views(region_map), n(lines), n(count), n(order), n(scores), n(kinds), opts)
        canvas.copy_(torch.from_numpy(out))
