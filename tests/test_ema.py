"""CPU: the host side of the weight average (engine.TrainStep(ema_decay=...), use_ema(), checkpoint.py) over tests/ema_fake.py, the
fp64 restatement (tests/ema_ref.py) on hand cases, the declarations, and the refusals of the two entry points through ctypes."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from gw_depth_amd import hip
from gw_depth_amd.checkpoint import FlatAdamW, load_checkpoint, save_checkpoint
from gw_depth_amd.engine import TrainStep
from tests import ema_ref as E
from tests.ema_fake import EmaFakeDevice
from tests.golden_check import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PASS = hip.EMA_PASS                          # elements per grid-stride pass of the two kernels (GWD_EMA_PASS)


@pytest.fixture()
def fake():
    dev = EmaFakeDevice()
    hip.set_library(dev)
    yield dev
    hip.set_library(None)


def _fake_grads(step, seed):
    g = torch.Generator().manual_seed(seed)
    r = torch.randn(step.flat_g.shape, generator=g) * 1e-3
    step.flat_g.zero_()
    for n, p in step.params.items():
        o = step.offsets[n]
        step.flat_g[o:o + p.numel()].copy_(r[o:o + p.numel()])


def _bufs(step):
    return [step.flat_p, step.flat_e, step.flat_m, step.flat_v] + ([] if step.flat_p16 is None else [step.flat_p16])


def _bits(step):
    return [t.clone() for t in _bufs(step)]


def _same(step, saved):
    return all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(_bufs(step), saved))


# ------------------------------------------------------------------------------------------------------------ the reference
def test_decay_on_hand_cases():
    assert E.decay_at(1, 0.9998, True) == 2.0 / 11.0
    assert E.omd_at(1, 0.9998, True) == float(np.float32(1.0 - 2.0 / 11.0))
    # the warm-up ramp (1 + t) / (10 + t) crosses 0.9998 at t = 44990: the ramp below it, the decay above it
    assert E.decay_at(44989, 0.9998, True) == 44990.0 / 44999.0 < 0.9998
    assert abs(E.decay_at(44990, 0.9998, True) - 0.9998) < 1e-15
    assert E.decay_at(44991, 0.9998, True) == 0.9998 < 44992.0 / 45001.0
    assert E.decay_at(1, 0.9998, False) == 0.9998 and E.decay_at(10 ** 6, 0.5, False) == 0.5
    assert E.omd_at(7, 0.9998, False) == float(np.float32(1.0 - 0.9998))
    assert E.decay_at(1, 0.1, True) == 0.1                       # a decay below the ramp's first value is never raised


def test_reference_update_and_bound_on_hand_cases():
    e, p = torch.tensor([1.0, -2.0, 3.0]), torch.tensor([2.0, -2.0, 1e-8])
    ref = E.ema_update(e, p, 0.25)
    assert ref.tolist() == [1.25, -2.0, 3.0 + 0.25 * (float(np.float32(1e-8)) - 3.0)]
    assert E.ulp32(torch.tensor([1.0, 1.5, 2.0, 0.0, 1e-45], dtype=torch.float64)).tolist() == [2.0 ** -23, 2.0 ** -23, 2.0 ** -22, 0.0, 2.0 ** -149]
    b = E.ema_bound(e, p, 0.25)
    assert float(b[0]) == 0.5 * 2.0 ** -23 * 0.25 + 0.5 * 2.0 ** -23 + 4 * 2.0 ** -53 * 3.0
    assert float(b[1]) == 0.5 * 2.0 ** -22 + 4 * 2.0 ** -53 * 4.0        # a still parameter: no rounding of the difference
    v = E.ema_values(4096, 3)
    assert bool((v > 0).any()) and bool((v < 0).any()) and 1e-8 <= float(v.abs().min()) < 1e-7 and 1e3 < float(v.abs().max()) <= 1e4


# ------------------------------------------------------------------------------------------------------------ TrainStep
def test_constructor_arguments(fake):
    cfg, model, crits = build()
    for bad in (0.0, 1.0, 1.5, -0.1):
        with pytest.raises(ValueError):
            TrainStep(model, crits, cfg, ema_decay=bad)
    step = TrainStep(model, crits, cfg)
    assert step.flat_e is None
    for call in (step.use_ema().__enter__, step.ema_state_dict, step.reset_ema, step.ema_updates):
        with pytest.raises(RuntimeError):
            call()


def test_unguarded_step_calls_the_fused_kernel_once_per_group(fake):
    cfg, model, crits = build()
    step = TrainStep(model, crits, cfg, ema_decay=0.999)
    assert step.flat_e.dtype == torch.float32 and torch.equal(step.flat_e, step.flat_p) and step.flat_e.data_ptr() != step.flat_p.data_ptr()
    _fake_grads(step, 1)
    step.optimizer_step()
    assert fake.calls == ["sqnorm", "adamw_step_ema", "adamw_step_ema"]
    assert [(c["guarded"], c["ema_t"], c["t"], c["n"]) for c in fake.ema_calls] == [(False, 1, 1, step.split), (False, 1, 1, step.total - step.split)]
    assert all(c["decay"] == 0.999 and c["warmup"] for c in fake.ema_calls)
    assert fake.bias_corrections[0] == (1 - 0.9 ** 1, 1 - 0.999 ** 1)
    step.optimizer_step()
    assert [c["t"] for c in fake.ema_calls[2:]] == [2, 2] and step.ema_updates() == 2
    assert not torch.equal(step.flat_e, step.flat_p)


def test_the_average_obeys_the_recurrence(fake):
    cfg, model, crits = build()
    step = TrainStep(model, crits, cfg, compute_dtype=torch.bfloat16, ema_decay=0.5, ema_warmup=False)
    for t in (1, 2, 3):
        _fake_grads(step, t)
        before = step.flat_e.clone()
        step.optimizer_step()
        assert E.check(step.flat_e, before, step.flat_p, E.omd_at(t, 0.5, False), "step %d" % t) <= 1.0
    idle = next(n for n in step.names if n in step.idle)         # never receives a gradient: only the decoupled decay moves it
    assert not torch.equal(step.flat_e, step.flat_p) and step.params[idle].numel() > 0


def test_guarded_step_passes_the_control_block(fake):
    cfg, model, crits = build()
    step = TrainStep(model, crits, cfg, guard="skip", ema_decay=0.999)
    _fake_grads(step, 1)
    step.optimizer_step()
    assert fake.calls == ["segment_stats", "health_decide", "adamw_step_ema", "adamw_step_ema"]
    assert [(c["guarded"], c["ema_t"], c["t"]) for c in fake.ema_calls] == [(True, 0, 1), (True, 0, 1)]
    assert step.ema_updates() == 1


def test_a_poisoned_step_leaves_the_average_alone(fake):
    cfg, model, crits = build()
    step = TrainStep(model, crits, cfg, compute_dtype=torch.bfloat16, guard="skip", ema_decay=0.5, ema_warmup=False)
    _fake_grads(step, 1)
    step.optimizer_step()
    assert step.ema_updates() == 1
    saved = _bits(step)
    _fake_grads(step, 2)
    victim = step.names[5]
    step.flat_g[step.offsets[victim] + step.params[victim].numel() - 1] = float("inf")
    step.optimizer_step(torch.tensor(2.5))
    assert _same(step, saved)                                    # parameters, the average, both moments and the bf16 shadow
    assert step.ema_updates() == 1 and step.step_count == 2 and fake.ema_calls[-1]["t"] is None
    _fake_grads(step, 3)
    before = step.flat_e.clone()
    step.optimizer_step()
    assert not _same(step, saved) and step.ema_updates() == 2 and fake.ema_calls[-1]["t"] == 2      # the unshifted count
    assert E.check(step.flat_e, before, step.flat_p, E.omd_at(2, 0.5, False)) <= 1.0


def _moved_step(fake, **kw):
    cfg, model, crits = build()
    step = TrainStep(model, crits, cfg, compute_dtype=torch.bfloat16, ema_decay=0.5, ema_warmup=False, **kw)
    for seed in (1, 2):
        _fake_grads(step, seed)
        step.optimizer_step()
    return cfg, model, step


def test_use_ema_swaps_and_restores_every_bit(fake):
    cfg, model, step = _moved_step(fake)
    p0, e0, s0 = step.flat_p.clone(), step.flat_e.clone(), step.flat_p16.clone()
    ptrs = [t.data_ptr() for t in _bufs(step)]
    name = step.names[0]
    del fake.calls[:]
    with step.use_ema() as inside:
        assert inside is step and fake.calls == ["ema_swap"]     # one call over the whole buffer
        assert torch.equal(step.flat_p, e0) and torch.equal(step.flat_e, p0) and torch.equal(step.flat_p16, e0.to(torch.bfloat16))
        assert torch.equal(dict(model.named_parameters())[name].data.reshape(-1), e0[step.offsets[name]:step.offsets[name] + step.params[name].numel()])
        with pytest.raises(RuntimeError, match="nest"):
            with step.use_ema():
                pass
        for call in (step.optimizer_step, lambda: step.forward_backward(None), lambda: step(None), step.reset_ema):
            with pytest.raises(RuntimeError, match="use_ema"):
                call()
        assert torch.equal(step.flat_p, e0) and step.step_count == 2          # the refusals touched nothing
    assert fake.calls == ["ema_swap", "ema_swap"]
    assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip((step.flat_p, step.flat_e, step.flat_p16), (p0, e0, s0)))
    assert [t.data_ptr() for t in _bufs(step)] == ptrs           # contents move, addresses never do
    with pytest.raises(KeyError):
        with step.use_ema():
            raise KeyError("inside")
    assert torch.equal(step.flat_p, p0) and torch.equal(step.flat_e, e0) and torch.equal(step.flat_p16, s0)
    _fake_grads(step, 3)
    step.optimizer_step()                                        # and the step runs again


def test_ema_state_dict_has_the_models_keys_and_shapes(fake):
    cfg, model, step = _moved_step(fake)
    sd, ref = step.ema_state_dict(), model.state_dict()
    assert list(sd) == list(ref) and all(sd[k].shape == ref[k].shape and sd[k].dtype == ref[k].dtype for k in ref)
    name = next(n for n in step.names if n not in step.idle)
    assert not torch.equal(sd[name], ref[name]) and sd[name].data_ptr() != ref[name].data_ptr()
    o, k = step.offsets[name], step.params[name].numel()
    assert torch.equal(dict(model.named_parameters())[name].data.reshape(-1), step.flat_p[o:o + k])     # the model is back on its weights
    cfg2, model2, crits2 = build()
    model2.load_state_dict(sd)                                   # loads as any state dict of the model does
    step.reset_ema()
    assert torch.equal(step.flat_e, step.flat_p) and step.ema_updates() == 0


def test_checkpoint_round_trip_carries_the_average(fake, tmp_path):
    cfg, model, crits = build()
    step = TrainStep(model, crits, cfg, ema_decay=0.5, ema_warmup=True)
    opt = FlatAdamW(step)
    sched = torch.optim.lr_scheduler.StepLR(opt, 2)
    for seed in (1, 2, 3):
        _fake_grads(step, seed)
        opt.step()
    path = os.path.join(tmp_path, "checkpoint.pth")
    save_checkpoint(path, model, opt, sched, epoch=1, args=None)
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    assert ckpt["ema_updates"] == 3 and list(ckpt["model_ema"]) == list(ckpt["model"])
    assert all(not v.is_cuda for v in ckpt["model_ema"].values())

    cfg2, model2, crits2 = build()
    step2 = TrainStep(model2, crits2, cfg2, ema_decay=0.5, ema_warmup=True)
    opt2 = FlatAdamW(step2)
    sched2 = torch.optim.lr_scheduler.StepLR(opt2, 2)
    assert load_checkpoint(path, model2, opt2, sched2, None, log=None) == 2
    assert torch.equal(step2.flat_e, step.flat_e) and torch.equal(step2.flat_p, step.flat_p) and step2.ema_updates() == 3
    for s, o in ((step, opt), (step2, opt2)):
        _fake_grads(s, 4)
        o.step()
    assert fake.ema_calls[-1]["t"] == 4 and fake.ema_calls[-3]["t"] == 4           # the warm-up continues where it was
    assert torch.equal(step2.flat_e, step.flat_e) and torch.equal(step2.flat_p, step.flat_p)

    # without the key, and with --no_opt: seeded from the loaded weights, the warm-up restarts
    for drop, args in ((True, None), (False, type("A", (), {"no_opt": True})())):
        cfg3, model3, crits3 = build()
        step3 = TrainStep(model3, crits3, cfg3, ema_decay=0.5)
        opt3 = FlatAdamW(step3)
        sched3 = torch.optim.lr_scheduler.StepLR(opt3, 2)
        step3.flat_e.fill_(7.0)
        c = {k: v for k, v in ckpt.items() if not (drop and k in ("model_ema", "ema_updates"))}
        load_checkpoint(c, model3, opt3, sched3, args, log=None)
        assert torch.equal(step3.flat_p, ckpt_flat(step3, ckpt["model"])) and torch.equal(step3.flat_e, step3.flat_p) and step3.ema_updates() == 0

    # a step without EMA loads a checkpoint that carries one; a checkpoint of such a step is today's dict
    cfg4, model4, crits4 = build()
    step4 = TrainStep(model4, crits4, cfg4)
    opt4 = FlatAdamW(step4)
    sched4 = torch.optim.lr_scheduler.StepLR(opt4, 2)
    assert load_checkpoint(ckpt, model4, opt4, sched4, None, log=None) == 2 and step4.flat_e is None
    assert torch.equal(step4.flat_p, ckpt_flat(step4, ckpt["model"]))
    save_checkpoint(path, model4, opt4, sched4, epoch=1, args=None)
    assert sorted(torch.load(path, map_location="cpu", weights_only=False)) == ["args", "epoch", "lr_scheduler", "model", "optimizer"]


def ckpt_flat(step, sd):
    """The flat parameter buffer a model state dict loads into (through a fresh load, layouts included)."""
    keep = step.flat_p.clone()
    step.model.load_state_dict(sd, strict=False)
    out = step.flat_p.clone()
    step.flat_p.copy_(keep)
    return out


# --------------------------------------------------------------------------------------------------------- declarations, refusals
def test_header_and_binding_declare_the_two_symbols():
    text = open(os.path.join(ROOT, "include", "gwdepth.h")).read()
    assert re.search(r"#define\s+GWD_VERSION\s+10\b", text)
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("gwd_adamw_step_ema", "gwd_ema_swap"):
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in hip.ENTRY_POINTS
    assert re.search(r"#define\s+GWD_EMA_PASS\s+%d\b" % PASS, text)
    src = open(os.path.join(ROOT, "gw_depth_amd", "csrc", "ema.hip")).read()
    threads, unroll, blocks = (int(re.search(r"constexpr int %s = (\d+);" % k, src).group(1)) for k in ("EMA_THREADS", "EMA_UNROLL", "EMA_MAX_BLOCKS"))
    assert blocks * threads * unroll * 4 == PASS
    assert "ema.hip" in open(os.path.join(ROOT, "gw_depth_amd", "csrc", "Makefile")).read()
    for kernel_file in ("optim.hip", "health.hip", "ema.hip"):   # one element function, called by all three kernels
        body = open(os.path.join(ROOT, "gw_depth_amd", "csrc", kernel_file)).read()
        assert "adamw_element(" in body and "adamw_coef(" in body and '#include "adamw.h"' in body, kernel_file


@pytest.fixture(scope="module")
def raw():
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(hip.LIB_PATH)
    vp, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float
    lib.gwd_adamw_step_ema.argtypes = [vp] * 8 + [i64] + [f32] * 9 + [ctypes.c_double, i32, i64, vp]
    lib.gwd_ema_swap.argtypes = [vp, vp, vp, i64, vp]
    lib.gwd_adamw_step_ema.restype = lib.gwd_ema_swap.restype = ctypes.c_int
    return lib


def test_entry_points_refuse_bad_arguments_before_any_launch(raw):
    """Addresses only: every call here returns before a kernel is launched, so no device is needed (and none is touched)."""
    A = 0x7f0000001000                                           # a 16-byte aligned "address" per buffer, 1 MiB apart
    P, G, M, V, S, Em = (A + (i << 20) for i in range(6))
    hyper = (1e-4, 0.9, 0.999, 1e-8, 1e-4, 0.1, 0.001, 0.1, 1.0)

    def step(p=P, g=G, m=M, v=V, s=S, e=Em, n=64, decay=0.999):
        return raw.gwd_adamw_step_ema(p, g, m, v, s, e, None, None, n, *hyper, decay, 1, 1, None)

    for null in ("p", "g", "m", "v", "e"):
        assert step(**{null: None}) == -1, null
    assert step(n=-1) == -1
    for decay in (0.0, 1.0, 1.5, -0.5, float("nan")):
        assert step(decay=decay) == -1, decay
    assert step(n=0) == 0 and step(n=0, s=None) == 0
    assert step(decay=0.0, n=0) == -1                            # the arguments are judged before the size
    for shifted in ("g", "m", "v", "e"):                         # one fp32 range at another offset from a 16-byte boundary
        assert step(**{shifted: {"g": G, "m": M, "v": V, "e": Em}[shifted] + 4}) == -3, shifted
    assert step(p=P + 4) == -3 and step(p=P + 2, g=G + 2, m=M + 2, v=V + 2, e=Em + 2, s=None) == -3
    assert step(s=S + 2) == -3 and step(s=S + 8 + 2) == -3       # the shadow: the same ELEMENT offset, so 2 bytes per 4

    assert raw.gwd_ema_swap(None, Em, S, 64, None) == -1 and raw.gwd_ema_swap(P, None, S, 64, None) == -1
    assert raw.gwd_ema_swap(P, Em, S, -1, None) == -1 and raw.gwd_ema_swap(P, Em, S, 0, None) == 0 and raw.gwd_ema_swap(P, Em, None, 0, None) == 0
    assert raw.gwd_ema_swap(P + 4, Em, None, 64, None) == -3 and raw.gwd_ema_swap(P, Em + 12, S, 64, None) == -3
    assert raw.gwd_ema_swap(P + 4, Em + 4, S, 64, None) == -3 and raw.gwd_ema_swap(P + 1, Em + 1, None, 64, None) == -3


def test_binding_checks_its_arguments():
    lib = object.__new__(hip.HipLibrary)                         # the argument checks run before the library is touched
    f = lambda n=8, dt=torch.float32: torch.zeros(n, dtype=dt)
    ok = dict(p=f(), g=f(), m=f(), v=f(), p16=f(8, torch.bfloat16), ema=f(), sq=None, ctl=None, n=8, lr=1e-4, b1=0.9, b2=0.999, eps=1e-8, wd=1e-4,
              bc1=0.1, bc2=0.001, max_norm=0.1, grad_scale=1.0, ema_decay=0.999, ema_warmup=True, ema_t=1)
    for bad in (dict(ema=f(8, torch.float64)), dict(ema=f(4)), dict(p16=f(8, torch.float16)), dict(p=f(7))):
        with pytest.raises(ValueError):
            lib.adamw_step_ema(**dict(ok, **bad))
    for decay in (0.0, 1.0, 1.5):
        with pytest.raises(ValueError):
            lib.adamw_step_ema(**dict(ok, ema_decay=decay))
    with pytest.raises(ValueError):
        lib.adamw_step_ema(**dict(ok, ctl=torch.zeros(32, dtype=torch.uint8)))
    with pytest.raises(TypeError):
        lib.adamw_step_ema(**dict(ok, sq=torch.zeros(1)))
    with pytest.raises(ValueError):
        lib.ema_swap(f(), f(4), None, 8)
    with pytest.raises(ValueError):
        lib.ema_swap(f(), f(), f(8, torch.float16), 8)
