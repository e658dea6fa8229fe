"""From decoded camera frames to results at frame size: InferenceSession.predict_frames against the route a user had before it,
in ONE process.

    python tools/frames_bench.py [--frames 8] [--height 720] [--width 1280] [--steps N] [--warmup K] [--min-seconds 2]

8 uint8 host frames of 720 x 1280, bf16, graph session, weights det_fill_ seed 0.  Arms:
  today, today_ensemble    Pillow resize (BILINEAR, RandomResize([1024], max_size=1024)) + ToTensor + Normalize on the host, the
                           batch to the device, the session's forward (the raw outputs of the captured graph), then per frame
                           F.interpolate(bilinear, align_corners=False) of depth and logits to the frame's size, the clamp, the
                           millimetres and the argmax; the ensemble forwards the mirrored images in the same batch, mirrors their
                           outputs back and averages;
  frames, frames_ensemble  sess.predict_frames(frames) and (..., ensemble=True).
The arms are alternated round-robin, one window of --steps calls each, until every arm has at least --min-seconds of timed work
and three windows; a window is timed by device events and ends in a synchronise (so the host work of `today` counts, as it does
for its user).  The new kernel alone is timed on the raw outputs of the last call: ms per launch and bytes/s from the 7 bytes it
stores per output pixel.  Prints one JSON line and writes it to profiles/frames_bench.json; fails without a GPU."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--steps", type=int, default=3, help="calls per timed window")
    ap.add_argument("--warmup", type=int, default=2, help="untimed calls per arm before the first window")
    ap.add_argument("--min-seconds", type=float, default=2.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frames_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    import torch.nn.functional as F
    from PIL import Image
    if not torch.cuda.is_available():
        sys.exit("frames_bench: needs the MI355X (no GPU found); a timing from anything else says nothing")
    from gw_depth_amd import Config, build_model, data, hip, ops
    from gw_depth_amd.infer import InferenceSession
    from gw_depth_amd.model import nested_tensor_from_tensor_list
    from gw_depth_amd.synth import det_fill_

    assert not getattr(hip.library(), "is_fake", False)
    B, fh, fw, steps = args.frames, args.height, args.width, args.steps
    cfg = Config(device="cuda", dropout=0.0, log_depth_error=True)
    model, _, _ = build_model(cfg)
    model.load_state_dict(det_fill_({k: v.detach().cpu().clone() for k, v in model.state_dict().items()}, seed=0))
    model.cuda().eval()
    sess = InferenceSession(model, compute_dtype=torch.bfloat16, graph=True)
    g = torch.Generator().manual_seed(1)
    frames = [torch.randint(0, 256, (fh, fw, 3), dtype=torch.uint8, generator=g) for _ in range(B)]
    nh, nw = data.resized_shape(fw, fh, 1024, 1024)
    mean, std = torch.tensor(data.MEAN).view(3, 1, 1), torch.tensor(data.STD).view(3, 1, 1)

    def today(ensemble):
        imgs = []
        for f in frames:
            small = np.asarray(Image.fromarray(f.numpy()).resize((nw, nh), Image.BILINEAR))
            imgs.append(((torch.from_numpy(small).permute(2, 0, 1).float() / 255.0 - mean) / std).to(torch.bfloat16))
        x = torch.stack(imgs).pin_memory().cuda(non_blocking=True)
        if ensemble:
            x = torch.cat([x, x.flip(-1)])
        raw = sess(nested_tensor_from_tensor_list(x))
        d, s = raw["pred_depth"][-1].float()[:, :, :nh, :nw], raw["pred_seg"].float()[:, :, :nh, :nw]
        d = torch.where(torch.isnan(d), torch.full_like(d, sess.min_depth), d.clamp(sess.min_depth, sess.max_depth))
        if ensemble:
            d, s = 0.5 * (d[:B] + d[B:].flip(-1)), s[:B] + s[B:].flip(-1)
        d = F.interpolate(d, size=(fh, fw), mode="bilinear", align_corners=False)[:, 0]
        s = F.interpolate(s, size=(fh, fw), mode="bilinear", align_corners=False)
        return d, torch.round(d * 1000.0).clamp(max=65535.0).to(torch.uint16), s.argmax(1).to(torch.uint8)

    calls = {"today": lambda: today(False), "today_ensemble": lambda: today(True),
             "frames": lambda: sess.predict_frames(frames), "frames_ensemble": lambda: sess.predict_frames(frames, ensemble=True)}
    arms = list(calls)
    for a in arms:
        for _ in range(max(args.warmup, 1)):
            calls[a]()
        torch.cuda.synchronize()
    assert all(v["captured"] for v in sess.graphs.values()), "capture was refused: %r" % dict(sess.graphs)

    windows = {a: [] for a in arms}
    rounds = 0
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

    res = {"tool": "frames_bench", "frames": B, "frame_height": fh, "frame_width": fw, "net_height": nh, "net_width": nw, "dtype": "bf16",
           "calls_per_window": steps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "arms": {}}
    for a in arms:
        w = windows[a]
        med = statistics.median(w)
        res["arms"][a] = {"ms_per_call": round(med, 4), "ms_min": round(min(w), 4), "ms_max": round(max(w), 4), "windows": len(w),
                          "frames_per_s": round(B * 1e3 / med, 2)}
    for a, base in (("frames", "today"), ("frames_ensemble", "today_ensemble")):
        res["arms"][a]["speedup_vs_" + base] = round(res["arms"][base]["ms_per_call"] / res["arms"][a]["ms_per_call"], 4)

    # the new kernel alone, on the raw outputs of a plain and of an ensemble pass
    sizes = torch.tensor([[nh, nw]] * B, dtype=torch.int32, device="cuda")
    fsz = torch.tensor([[fh, fw]] * B, dtype=torch.int32, device="cuda")
    for name, ensemble in (("resized_post", False), ("resized_post_ensemble", True)):
        sess.predict_frames(frames, ensemble=ensemble)
        raw = sess._graphs[(2 * B if ensemble else B, nh, nw)]["result"][0]
        d, s = raw["pred_depth"][-1], raw["pred_seg"]
        out = ops.dense_postprocess_resized(d, s, sizes, fsz, (fh, fw), sess.min_depth, sess.max_depth, twin=B if ensemble else 0)
        times = []
        for _ in range(5):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0.record()
            for _ in range(20):
                ops.dense_postprocess_resized(d, s, sizes, fsz, (fh, fw), sess.min_depth, sess.max_depth, twin=B if ensemble else 0, out=out)
            t1.record()
            t1.synchronize()
            times.append(t0.elapsed_time(t1) / 20)
        ms = statistics.median(times)
        stored = 7 * B * fh * fw
        res[name] = {"ms_per_launch": round(ms, 5), "ms_min": round(min(times), 5), "ms_max": round(max(times), 5), "bytes_stored": stored,
                     "stored_bytes_per_s": round(stored / (ms * 1e-3), 1), "note": "20 back-to-back launches per window, launch gaps included"}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
