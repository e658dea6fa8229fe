"""The CPU stand-in of tests/test_frames_post.py with gwd_line_nms added, from its restatement (tests/line_nms_ref.py): the session's
plumbing around the new call runs end to end without a GPU.  The product never does this."""
import torch

from tests import line_nms_ref as N
from tests.test_frames_post import FramesFakeDevice


class LineNmsFakeDevice(FramesFakeDevice):
    def __init__(self):
        super().__init__()
        self.nms_calls = []

    def line_nms(self, logits, lines, sizes, order, threshold, min_score, nms_lines, nms_scores, nms_ids, nms_count, twin):
        self.nms_calls.append({"threshold": threshold, "by_order": order is not None, "min_score": min_score, "twin": twin,
                               "sizes": sizes.tolist()})
        scores = torch.softmax(logits, -1)[..., 0].numpy()
        out = N.line_nms(scores, lines.numpy(), sizes.numpy(), threshold, None if order is None else order.numpy(), min_score, twin)
        for dst, src in zip((nms_lines, nms_scores, nms_ids, nms_count), out):
            dst.copy_(torch.from_numpy(src))
