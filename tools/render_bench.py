#!/usr/bin/env python
"""Rendering of predict_frames' results on the MI355X (gwd_render_frames):

    python tools/render_bench.py [--frames 8] [--height 720] [--width 1280] [--steps N] [--warmup K] [--min-seconds 2]

  call            ops.render_frames, 3 panels (frame + tint + outlines + lines by score; depth; labels) of the labels / depth_mm /
                  region_map that predict_frames returned, at 100 and at 1024 seeded lines per frame: device events over back-to-back
                  calls and the kernel's own time from the profiler's records; the canvas bytes stored over that time, next to the
                  rate of a device-to-device copy of the same canvas in the same run;
  arms            predict_frames of a session without render= (the launches and keys of the parent commit) and with it, alternated
                  in one process;
  host            the route it replaces: frames' results copied to the host, a numpy table lookup per panel, PIL.ImageDraw lines
                  (host clock around it, the copies included), 100 lines per frame;
  png             PNG encoding of one call's canvas on the host (render.save_panels), timed on its own: it dominates saving.
Prints one JSON line and writes it to profiles/render_bench.json; fails without a GPU."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--steps", type=int, default=3, help="calls per timed window")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--min-seconds", type=float, default=2.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("render_bench: needs the MI355X (no GPU found); a timing from anything else says nothing")
    from PIL import Image, ImageDraw
    from torch.profiler import ProfilerActivity, profile

    from gw_depth_amd import Config, build_model, hip, ops, render
    from gw_depth_amd.infer import InferenceSession
    from gw_depth_amd.synth import det_fill_
    assert not getattr(hip.library(), "is_fake", False)
    B, fh, fw, steps = args.frames, args.height, args.width, args.steps

    def event_ms(fn, reps=20, windows=5):
        fn()
        times = []
        for _ in range(windows):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0.record()
            for _ in range(reps):
                fn()
            t1.record()
            t1.synchronize()
            times.append(t0.elapsed_time(t1) / reps)
        return statistics.median(times)

    def kernel_ms(fn, reps=10):
        """ms per launch of render_frames_kernel from the profiler's kernel records; None where this host has no tracer."""
        fn()
        torch.cuda.synchronize()
        try:
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                for _ in range(reps):
                    fn()
                torch.cuda.synchronize()
            for e in prof.key_averages():
                if "render_frames_kernel" in e.key:
                    return round(e.device_time_total / max(e.count, 1) / 1e3, 5)
        except Exception:
            pass
        return None

    cfg = Config(device="cuda", dropout=0.0, log_depth_error=True)
    model, _, _ = build_model(cfg)
    model.load_state_dict(det_fill_({k: v.detach().cpu().clone() for k, v in model.state_dict().items()}, seed=0))
    model.cuda().eval()
    kw = dict(compute_dtype=torch.bfloat16, graph=True, line_nms=0.01, regions=True)
    plain = InferenceSession(model, **kw)
    with_render = InferenceSession(model, render=True, **kw)
    g = torch.Generator().manual_seed(1)
    frames = []
    for _ in range(B):
        low = torch.rand(1, 3, 9, 16, generator=g)
        frames.append((torch.nn.functional.interpolate(low, size=(fh, fw), mode="bicubic", align_corners=False)[0].clamp(0, 1) * 255)
                      .permute(1, 2, 0).to(torch.uint8).contiguous())
    res = with_render.predict_frames(frames)
    torch.cuda.synchronize()
    labels, mm, sizes, rmap = res["labels"], res["depth_mm"], res["sizes"], res["region_map"]
    on_dev = [f.cuda() for f in frames]
    panels = [{"base": "frame", "tint": 0, "outlines": True, "lines": "score"}, ("depth", 0), ("labels", 0)]
    canvas_bytes = int(res["canvas"].numel())
    out = {"tool": "render_bench", "frames": B, "frame_height": fh, "frame_width": fw, "panels": len(panels), "canvas_bytes": canvas_bytes,
           "device": torch.cuda.get_device_name(0),
           "predicted": {"nms_count": res["nms_count"].tolist(), "region_count": res["region_count"].tolist()}, "call": {}}

    src, dst = res["canvas"].clone(), torch.empty_like(res["canvas"])
    copy_ms = event_ms(lambda: dst.copy_(src))
    out["copy"] = {"ms": round(copy_ms, 5), "gb_per_s_stored": round(canvas_bytes / copy_ms / 1e6, 1),
                   "note": "torch copy_ of the same canvas, device to device: bytes stored (as many again are read) over device-event time"}
    rng = np.random.default_rng(2)
    operands = {}
    for C in (100, 1024):
        lines = torch.from_numpy(rng.uniform(0.0, 1.0, (B, C, 4)) * np.array([fw, fh, fw, fh])).cuda()
        scores = torch.from_numpy(rng.uniform(0.92, 1.02, (B, C)).astype(np.float32)).cuda()
        count = torch.full((B,), C, dtype=torch.int32, device="cuda")
        operands[C] = (lines, scores, count)
        fn = lambda: ops.render_frames(sizes, panels, frames=on_dev, planes=mm, label_planes=labels, region_map=rmap, lines=lines, count=count,
                                       scores=scores)
        call_ms, k_ms = event_ms(fn), kernel_ms(fn)
        out["call"][str(C)] = {"lines": B * C, "call_ms": round(call_ms, 5), "kernel_ms": k_ms,
                               "gb_per_s_stored": None if not k_ms else round(canvas_bytes / k_ms / 1e6, 1)}
    out["call"]["note"] = ("call_ms: device events over 20 back-to-back ops.render_frames calls, allocation and launch gaps included; "
                           "gb_per_s_stored: canvas bytes over kernel_ms (the reads - frames, three planes, tables - come on top)")

    calls = {"predict_frames": lambda: plain.predict_frames(frames), "predict_frames_render": lambda: with_render.predict_frames(frames)}
    for a in calls:
        for _ in range(max(args.warmup, 1)):
            calls[a]()
        torch.cuda.synchronize()
    windows = {a: [] for a in calls}
    arms, rounds = list(calls), 0
    while any(len(windows[a]) < 3 or sum(windows[a]) * steps / 1e3 < args.min_seconds for a in arms):
        k = rounds % len(arms)
        rounds += 1
        for a in arms[k:] + arms[:k]:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0.record()
            for _ in range(steps):
                calls[a]()
            t1.record()
            t1.synchronize()
            windows[a].append(t0.elapsed_time(t1) / steps)
    out["arms"] = {a: {"ms_per_call": round(statistics.median(w), 4), "ms_min": round(min(w), 4), "ms_max": round(max(w), 4), "windows": len(w)}
                   for a, w in windows.items()}
    out["arms"]["note"] = "predict_frames: a session without render= issues the parent commit's launches; both with line_nms=0.01, regions=True"

    lines, scores, count = operands[100]
    jet, pal = render.jet_table(), render.voc_palette()

    def host_route():
        """What a preview costs without the kernel: four copies, a table lookup per panel, a Python loop that draws the lines."""
        lab, dmm, ln, sc = labels.cpu().numpy(), mm.cpu().numpy(), lines.cpu().numpy(), scores.cpu().numpy()
        depth = jet[np.clip((510 * dmm.astype(np.int64) + 8500) // 17000, 0, 255)]
        seg = pal[lab]
        shown = []
        for b in range(B):
            im = Image.fromarray(frames[b].numpy())
            draw = ImageDraw.Draw(im)
            for r in range(ln.shape[1]):
                c = jet[min(max(int((sc[b, r] - 0.92) * 2560.0), 0), 255)]
                draw.line([tuple(ln[b, r, :2]), tuple(ln[b, r, 2:])], fill=tuple(int(v) for v in c), width=2)
            shown.append(np.asarray(im))
        return depth, seg, shown

    host = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host_route()
        host.append((time.perf_counter() - t0) * 1e3)
    out["host"] = {"lines": B * 100, "ms_per_call": round(statistics.median(host), 3), "ms_min": round(min(host), 3), "ms_max": round(max(host), 3),
                   "windows": len(host), "note": "labels / depth_mm / lines / scores .cpu(), numpy table lookups, PIL.ImageDraw lines; no tint, no outlines"}

    canvas = ops.render_frames(sizes, panels, frames=on_dev, planes=mm, label_planes=labels, region_map=rmap, lines=lines, count=count, scores=scores)
    torch.cuda.synchronize()
    png = {}
    with tempfile.TemporaryDirectory() as tmp:
        for layout in ("row", "files"):
            t0 = time.perf_counter()
            written = render.save_panels(canvas, [(fh, fw)] * B, [os.path.join(tmp, "%s%d.png" % (layout, b)) for b in range(B)], layout=layout)
            png[layout] = {"ms": round((time.perf_counter() - t0) * 1e3, 2), "files": len(written), "bytes": sum(os.path.getsize(p) for p in written)}
    t0 = time.perf_counter()
    canvas.cpu()
    png["copy_to_host_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    png["note"] = "render.save_panels of one call's canvas (4 threads, Pillow's default compression): the copy to the host and the PNG encoding"
    out["png"] = png
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
