"""The CPU stand-in of tests/fake_device.py with the three calls of csrc/health.hip added, from their restatement
(tests/health_ref.py), and a record of the optimizer calls a TrainStep makes: the plumbing around the guarded step runs end to end
without a GPU.  The product never does this."""
import numpy as np
import torch

from gw_depth_amd import health as H
from gw_depth_amd import hip
from tests import health_ref as R
from tests.fake_device import FakeDevice


def _records(buf, dtype):
    """A writable numpy record view of a CPU uint8 tensor."""
    return buf.numpy().view(dtype)


class HealthFakeDevice(FakeDevice):
    def __init__(self):
        super().__init__()
        self.calls = []                     # names of the optimizer-side calls, in order
        self.bias_corrections = []          # (bc1, bc2) of every AdamW launch that stored something

    def workspace_bytes(self, op, *dims):
        if op == hip.WS_HEALTH:
            return max(int(dims[0]), 1) * hip.HEALTH_RECORD_BYTES
        return super().workspace_bytes(op, *dims)

    def sqnorm(self, g, sq, n):
        self.calls.append("sqnorm")
        super().sqnorm(g, sq, n)

    def adamw_step(self, p, g, m, v, p16, sq, n, lr, b1, b2, eps, wd, bc1, bc2, max_norm, grad_scale):
        self.calls.append("adamw_step")
        self.bias_corrections.append((bc1, bc2))
        super().adamw_step(p, g, m, v, p16, sq, n, lr, b1, b2, eps, wd, bc1, bc2, max_norm, grad_scale)

    def segment_stats(self, x, seg_begin, seg_end, chunks, partial, out):
        self.calls.append("segment_stats")
        ch = _records(chunks.reshape(-1).view(torch.uint8), H.CHUNK_DTYPE)
        H.check_tables(seg_begin.tolist(), seg_end.tolist(), ch, x.numel())
        rec = _records(out, H.STAT_DTYPE)
        for s, (sumsq, absmax, nonfinite) in enumerate(R.segment_stats(x, seg_begin.tolist(), seg_end.tolist(), exact=False)):
            rec[s] = (sumsq, absmax, nonfinite)

    def health_decide(self, stats, S, loss, ctl, ring, ring_len, bad, beta1, beta2, max_norm, grad_scale):
        self.calls.append("health_decide")
        rec = _records(stats, H.STAT_DTYPE)[:S]
        c = _records(ctl, H.CTL_DTYPE)
        old = {k: c[0][k].item() for k in H.CTL_DTYPE.names if k != "reserved"}
        new, r, bad_new = R.decide([(float(x["sumsq"]), float(x["absmax"]), int(x["nonfinite"])) for x in rec], old,
                                   None if loss is None else float(loss), beta1, beta2, max_norm, grad_scale)
        for k, val in new.items():
            c[k][0] = val
        _records(ring, H.RING_DTYPE)[(r["step"] - 1) % ring_len] = (r["step"], r["grad_norm"], r["clip_coef"], r["loss"], int(r["apply"]),
                                                                    r["nonfinite_total"])
        if bad_new is not None:
            bad[:S] = torch.tensor(bad_new, dtype=torch.int32)

    def adamw_step_guarded(self, p, g, m, v, p16, ctl, n, lr, b1, b2, eps, wd, max_norm, grad_scale):
        self.calls.append("adamw_step_guarded")
        c = _records(ctl, H.CTL_DTYPE)[0]
        if not c["apply"]:
            return
        self.bias_corrections.append((float(c["bc1"]), float(c["bc2"])))
        FakeDevice.adamw_step(self, p, g, m, v, p16, torch.tensor([float(c["sq"])], dtype=torch.float64), n, lr, b1, b2, eps, wd,
                              float(c["bc1"]), float(c["bc2"]), max_norm, grad_scale)
