"""tests/health_fake.py with the two calls of csrc/ema.hip added: the host side of the weight average (engine.TrainStep(ema_decay=...),
checkpoint.py) runs end to end without a GPU.  The product never does this."""
import numpy as np
import torch

from gw_depth_amd import health as H
from tests import ema_ref as E
from tests.fake_device import FakeDevice
from tests.health_fake import HealthFakeDevice, _records


class EmaFakeDevice(HealthFakeDevice):
    def __init__(self):
        super().__init__()
        self.ema_calls = []                 # one dict per adamw_step_ema call: guarded, ema_t, t (None when skipped), n, decay, warmup

    def adamw_step_ema(self, p, g, m, v, p16, ema, sq, ctl, n, lr, b1, b2, eps, wd, bc1, bc2, max_norm, grad_scale, ema_decay, ema_warmup,
                       ema_t):
        self.calls.append("adamw_step_ema")
        assert 0.0 < ema_decay < 1.0 and ema.dtype == torch.float32
        rec = {"guarded": ctl is not None, "ema_t": int(ema_t), "t": None, "n": int(n), "decay": ema_decay, "warmup": bool(ema_warmup)}
        self.ema_calls.append(rec)
        if ctl is not None:
            c = _records(ctl, H.CTL_DTYPE)[0]
            if not c["apply"]:
                return                      # nothing is stored, the average included
            sq, bc1, bc2 = torch.tensor([float(c["sq"])], dtype=torch.float64), float(c["bc1"]), float(c["bc2"])
            t = int(c["applied"]) - int(ema_t)
        else:
            t = int(ema_t)
        rec["t"] = t
        self.bias_corrections.append((bc1, bc2))
        FakeDevice.adamw_step(self, p, g, m, v, p16, sq, n, lr, b1, b2, eps, wd, bc1, bc2, max_norm, grad_scale)
        omd = E.omd_at(t, ema_decay, ema_warmup)
        e = ema[:n]
        diff = (p[:n] - e).double()         # the kernel's fmaf(omd, fl32(p' - ema), ema): a zero difference keeps ema bit for bit
        e.copy_((e.double() + float(np.float32(omd)) * diff).float())

    def ema_swap(self, p, ema, p16, n):
        self.calls.append("ema_swap")
        keep = p[:n].clone()
        p[:n].copy_(ema[:n])
        ema[:n].copy_(keep)
        if p16 is not None:
            p16[:n].copy_(p[:n])
