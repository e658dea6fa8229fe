"""Evaluation path: mirror of evaluate() (/root/reference/src/engine_glassrgbd.py:174-345) with the dense metrics
accumulated ON THE DEVICE (gwd_eval_accumulate) instead of per-image device->host copies + numpy.

`DenseMetrics` is the device-side accumulator (clamp + validity mask :249-253, compute_depth_errors
src/util/metrics.py:198-218, confusion counts :37-74, running sums :262-263); `evaluate` keeps the reference's
signature and returns the same stats keys (`Background, Glass, Pixel accuracy, Mean accuracy, Mean IU, silog, abs_rel,
log10, rms, sq_rel, log_rms, d1, d2, d3`, plus the line-loss terms with --with_line).  Unlike the reference it accepts
batches of more than one image: the depth measures are per image either way, padded pixels are excluded through the
NestedTensor masks.  The visualisation switches (save_dense / save_line) are outside the accelerated path.

`LineMetrics` scores the line detector the way the reference does offline (structural AP and F-score at 5 / 10 / 15 after L-CNN's
line NMS; evaluation/eval_post_online.py, eval-sAP-glassrgbd.py, eval-fscore-glassrgbd.py), accumulated on the device by
gwd_line_score, one launch per batch; `evaluate` feeds it when args.line_ap is set together with --with_line.

`FrameMetrics` scores what InferenceSession.predict_frames returns - depth and labels at every frame's own size, with or without
the mirror ensemble - against the ground truth as the loaders keep it (millimetres and raw label bytes), by region (all / glass /
non-glass / GT-depth bins), one gwd_eval_frames launch per call, per-image records kept and mergeable across ranks;
`evaluate_frames` walks a dataset.FrameStore or StreamSource through both.
"""
import numpy as np
import torch

from . import hip

METRIC_NAMES = ["silog", "abs_rel", "log10", "rms", "sq_rel", "log_rms", "d1", "d2", "d3"]     # engine_glassrgbd.py:204
SEG_LABELS = ["Background", "Glass"]                                                            # util/metrics.py:10-11


def _lib():
    return hip.library()


class DenseMetrics:
    """Running depth / segmentation metrics of an evaluation pass, kept in HBM until compute()."""

    def __init__(self, device, min_depth_eval=1e-3, max_depth_eval=10.0):
        self.device = torch.device(device)
        self.min_d, self.max_d = float(min_depth_eval), float(max_depth_eval)
        self.running = torch.zeros(10, dtype=torch.float64, device=self.device)       # depth_eval_measures (:203)
        self.confusion = torch.zeros(4, dtype=torch.int64, device=self.device)        # confusion_matrix (metrics.py:60)
        self._ws = None

    def reset(self):
        self.running.zero_()
        self.confusion.zero_()

    def update(self, pred_depth=None, gt_depth=None, pred_seg=None, seg_gt=None):
        """pred_depth (B,1,H,W) or (B,H,W) fp32/bf16 metres, gt_depth same shape; pred_seg (B,2,H,W) logits in ANY
        strides whose two pixel dims collapse (the model's pixel-major view qualifies), seg_gt (B,1,H,W)/(B,H,W) int64
        with 255 = ignore.  Either pair may be None.  Returns the (B,9) per-image measures (device, f64) or None."""
        lib = _lib()
        B = (pred_depth if pred_depth is not None else pred_seg).shape[0]
        pred = gt = seg = tgt = measures = None
        strides = (0, 0, 0)
        if pred_depth is not None:
            pred = pred_depth.reshape(B, -1).contiguous()
            gt = gt_depth.reshape(B, -1).to(torch.float32).contiguous()
            if pred.shape != gt.shape:
                raise ValueError("pred_depth %s and gt_depth %s differ" % (tuple(pred_depth.shape), tuple(gt_depth.shape)))
            HW = pred.shape[1]
            measures = torch.empty(B, 9, dtype=torch.float64, device=pred.device)
        if pred_seg is not None:
            if pred_seg.dim() != 4 or pred_seg.shape[1] != 2:
                raise ValueError("pred_seg must be (B, 2, H, W) logits, got %s" % (tuple(pred_seg.shape),))
            Hs, Ws = pred_seg.shape[-2:]
            if Hs > 1 and pred_seg.stride(2) != Ws * pred_seg.stride(3):
                pred_seg = pred_seg.contiguous()
            seg = pred_seg
            strides = (seg.stride(0), seg.stride(3), seg.stride(1))
            tgt = seg_gt.reshape(B, -1).to(torch.int64).contiguous()
            if tgt.shape[1] != Hs * Ws or (pred is not None and HW != Hs * Ws):
                raise ValueError("seg_gt / pred_seg / pred_depth pixel counts differ")
            HW = Hs * Ws
        need = lib.workspace_bytes(hip.WS_EVAL, B, HW)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.running.device)
        lib.eval_accumulate(pred, gt, seg, strides, tgt, self._ws, measures, self.running, self.confusion, B, HW,
                            self.min_d, self.max_d)
        return measures

    def compute(self):
        """One device->host copy; the closing arithmetic of compute_mean_ioU (metrics.py:76-98) and of evaluate()
        (:313-319) on 14 numbers."""
        run = self.running.cpu()
        conf = self.confusion.cpu().to(torch.float64).reshape(2, 2)
        out = {}
        if float(conf.sum()) > 0:
            pos, res, tp = conf.sum(1), conf.sum(0), conf.diagonal()
            iou = tp / torch.clamp(pos + res - tp, min=1.0) * 100
            for lab, v in zip(SEG_LABELS, iou):
                out[lab] = float(v)
            out["Pixel accuracy"] = float(tp.sum() / pos.sum() * 100)
            out["Mean accuracy"] = float((tp / torch.clamp(pos, min=1.0)).mean() * 100)
            out["Mean IU"] = float(iou.mean())
        if float(run[9]) > 0:
            for k, name in enumerate(METRIC_NAMES):
                out[name] = float(run[k] / run[9])
        return out


class LineMetrics:
    """Structural AP / F-score of the detected lines over an evaluation pass; flags and scores stay in HBM until compute().

    Per image (gwd_line_score, include/gwdepth.h): softmax score, duplicate trim, L-CNN line NMS at every `nms_thresholds` (fractions
    of the image diagonal) with the lines in QUERY order, rescale to 128 x 128, msTPFP against the ground truth at every
    `sap_thresholds`.  Precision is pinned to f64 after the fp32 pixel scaling.  The ground truth is the targets' normalised lines
    times 128; the reference's scripts read the data set's own lpos files, which no vector here pins.

    Equal scores: the reference's np.argsort(-scores) leaves their order open; here it is image order, then line order."""

    def __init__(self, device, nms_thresholds=(0.010, 0.015), sap_thresholds=(5, 10, 15), capacity_images=256):
        self.device = torch.device(device)
        self.nms_thresholds = tuple(float(t) for t in nms_thresholds)
        self.sap_thresholds = tuple(float(t) for t in sap_thresholds)
        if not (1 <= len(self.nms_thresholds) <= 4 and 1 <= len(self.sap_thresholds) <= 4):
            raise ValueError("LineMetrics takes one to four thresholds of either kind")
        self.capacity = max(int(capacity_images), 1)
        self.images_seen = 0
        self.Q = None
        self._flag = self._kept = self._score = self._gt_seen = None

    def reset(self):
        self.images_seen = 0

    def _reserve(self, images, Q):
        """Room for `images` image slots of Q queries.  Sizes come from shapes, so growing costs device copies and no sync."""
        if self.Q is None:
            self.Q = int(Q)
        if Q != self.Q:
            raise ValueError("LineMetrics was started with %d queries per image, got %d" % (self.Q, Q))
        if self._flag is not None and images <= self.capacity:
            return
        while self.capacity < images:
            self.capacity *= 2
        T, S, n, dev = len(self.nms_thresholds), len(self.sap_thresholds), self.images_seen, self.device
        old = (self._flag, self._kept, self._score, self._gt_seen)
        self._flag = torch.empty(T, S, self.capacity, self.Q, dtype=torch.uint8, device=dev)
        self._kept = torch.empty(T, self.capacity, self.Q, 4, dtype=torch.float64, device=dev)
        self._score = torch.empty(self.capacity, self.Q, dtype=torch.float32, device=dev)
        self._gt_seen = torch.empty(self.capacity, dtype=torch.int32, device=dev)
        if old[0] is not None and n:
            self._flag[:, :, :n] = old[0][:, :, :n]
            self._kept[:, :n] = old[1][:, :n]
            self._score[:n] = old[2][:n]
            self._gt_seen[:n] = old[3][:n]

    def update(self, pred_logits, pred_lines, sizes, gt_lines, gt_counts):
        """pred_logits (B,Q,2), pred_lines (B,Q,4|6) normalised, sizes (B,2) int32 (h, w), gt_lines (B,G,4) fp32 normalised
        (x1, y1, x2, y2) padded to G rows, gt_counts (B,) int32 - all on the device.  Writes image slots images_seen .. + B - 1
        with one launch (fp32 contiguous inputs are used as they are)."""
        B, Q = pred_logits.shape[:2]
        self._reserve(self.images_seen + B, Q)
        _lib().line_score(pred_logits.float().contiguous(), pred_lines.float().contiguous(), sizes.contiguous(),
                          gt_lines.float().contiguous(), gt_counts.contiguous(), self.nms_thresholds, self.sap_thresholds,
                          self._flag, self._kept, self._score, self._gt_seen, self.images_seen)
        self.images_seen += B

    def kept_lines(self):
        """(T, images_seen, Q, 4) f64 (y1, x1, y2, x2) in the 128 x 128 space, zeros where a query was not kept."""
        return self._kept[:, :self.images_seen]

    def compute(self):
        """One stable descending sort of all scores on the device, one device->host copy (the sorted flags with the ground-truth
        counts behind them), then the closing arithmetic of eval-sAP-glassrgbd.py:66-73, lcnn/metric.py:11-21 (ap) and
        eval-fscore-glassrgbd.py:35-43 (f_score) in numpy f64.  Values are times 100, as the scripts print them; an evaluation
        without ground-truth lines returns zeros."""
        n, T, S = self.images_seen, len(self.nms_thresholds), len(self.sap_thresholds)
        if n == 0:
            return {}
        order = torch.sort(self._score[:n].reshape(-1), descending=True, stable=True).indices
        flags = self._flag[:, :, :n].reshape(T * S, n * self.Q)[:, order]
        host = torch.cat([flags.reshape(-1), self._gt_seen[:n].contiguous().view(torch.uint8)]).cpu().numpy()
        flags = host[:T * S * n * self.Q].reshape(T, S, n * self.Q)
        n_gt = int(host[T * S * n * self.Q:].view(np.int32).sum())
        out = {"n_gt": n_gt}
        for t, thr in enumerate(self.nms_thresholds):
            for s, st in enumerate(self.sap_thresholds):
                ap, f = close_line_scores(flags[t, s], n_gt)
                tag = "%g_nms%s" % (st, ("%.3f" % thr).replace(".", "_"))
                out["sAP" + tag], out["sF" + tag] = ap, f
        return out


def _measures_from_sums(s):
    """(..., 10) raw sums -> (..., 9) measures (METRIC_NAMES order), NaN where the count is zero: the closing step of the kernel."""
    with np.errstate(all="ignore"):
        n = s[..., 0]
        me, me2 = s[..., 7] / n, s[..., 8] / n
        return np.stack([np.sqrt(me2 - me * me) * 100.0, s[..., 5] / n, s[..., 9] / n, np.sqrt(s[..., 4] / n), s[..., 6] / n,
                         np.sqrt(me2), s[..., 1] / n, s[..., 2] / n, s[..., 3] / n], axis=-1)


class FrameMetrics:
    """Depth / segmentation metrics of predict_frames results at frame size, by region, kept per image (gwd_eval_frames).

    Regions: "all", "glass" (GT label > 0), "nonglass", and "bin0".. for depth_bins = ascending edges in metres (bin k holds
    edges[k] <= GT depth < edges[k+1]; at most 8 bins).  Every image fills one record (raw sums, measures, confusion) in HBM;
    `running` (R,10) and `confusion` (4,) are the device-side totals in the order the images were fed - an image whose region has
    no valid pixel is left out of that region's mean, and running[:, 9] counts the images that entered.  compute() reads the records
    back once and folds them in ascending id order, so its result does not depend on how the images were split over calls or ranks."""

    def __init__(self, device, min_depth_eval=1e-3, max_depth_eval=10.0, depth_bins=None, capacity_images=4096):
        self.device = torch.device(device)
        self.min_d, self.max_d = float(min_depth_eval), float(max_depth_eval)
        self.edges = tuple(float(e) for e in (depth_bins if depth_bins is not None else ()))
        if len(self.edges) == 1 or len(self.edges) > hip.EVAL_FRAMES_MAX_BINS + 1:
            raise ValueError("depth_bins: 2..%d ascending edges (or none), got %d" % (hip.EVAL_FRAMES_MAX_BINS + 1, len(self.edges)))
        if any(not b >= a for a, b in zip(self.edges, self.edges[1:])):
            raise ValueError("depth_bins must ascend, got %r" % (self.edges,))
        self.n_bins = max(len(self.edges) - 1, 0)
        self.regions = ["all", "glass", "nonglass"] + ["bin%d" % k for k in range(self.n_bins)]
        self.capacity = int(capacity_images)
        if self.capacity < 1:
            raise ValueError("capacity_images must be positive")
        R, dev = len(self.regions), self.device
        self.sums = torch.empty(self.capacity, R, 10, dtype=torch.float64, device=dev)
        self.measures = torch.empty(self.capacity, R, 9, dtype=torch.float64, device=dev)
        self.conf = torch.empty(self.capacity, 4, dtype=torch.int64, device=dev)
        self.running = torch.zeros(R, 10, dtype=torch.float64, device=dev)
        self.confusion = torch.zeros(4, dtype=torch.int64, device=dev)
        self._ws = torch.zeros(hip.EVAL_FRAMES_WS_BYTES, dtype=torch.uint8, device=dev)      # the tickets start as zeros, once
        self.images_seen = 0
        self._ids = []
        self._host = None              # a merged object: (ids, sums, measures, conf) host arrays instead of device records

    def reset(self):
        self.running.zero_()
        self.confusion.zero_()
        self.images_seen, self._ids, self._host = 0, [], None

    def update(self, result, gt, ids=None):
        """result: the dict of predict_frames ("depth" (B,Fh,Fw) fp32, "labels" (B,Fh,Fw) uint8); gt: [(depth_mm (fh,fw), labels
        (fh,fw) uint8)] per frame, on the device - int32 millimetres as FrameStore.frames() gives them, or the 16-bit plane of a
        record (uint16 / int16 view, FrameStore.record_gt); ids: one integer per frame (default: the running image count).  The
        (fh, fw) of every pair are checked on the host against the planes of the result (each fits, the largest fills them).  One
        launch, nothing to wait for."""
        if self._host is not None:
            raise RuntimeError("a merged FrameMetrics takes no updates")
        depth, labels = result["depth"], result["labels"]
        if depth.dim() != 3 or depth.dtype != torch.float32 or labels.dtype != torch.uint8 or labels.shape != depth.shape:
            raise ValueError("FrameMetrics.update: depth (B,Fh,Fw) fp32 and labels (B,Fh,Fw) uint8 expected, got %s %s / %s %s"
                             % (tuple(depth.shape), depth.dtype, tuple(labels.shape), labels.dtype))
        B, Fh, Fw = depth.shape
        if not 0 < B <= hip.EVAL_FRAMES_BATCH or len(gt) != B:
            raise ValueError("FrameMetrics.update: 1..%d frames per call with one ground-truth pair each, got %d and %d"
                             % (hip.EVAL_FRAMES_BATCH, B, len(gt)))
        pairs = []
        for i, (dmm, lab) in enumerate(gt):
            if dmm.dtype not in (torch.int32, torch.uint16, torch.int16) or lab.dtype != torch.uint8:
                raise TypeError("FrameMetrics.update: frame %d: depth_mm int32 / uint16 / int16 and labels uint8 expected, got %s, %s"
                                % (i, dmm.dtype, lab.dtype))
            if dmm.dim() != 2 or lab.shape != dmm.shape or dmm.shape[0] < 1 or dmm.shape[1] < 1 or dmm.shape[0] > Fh or dmm.shape[1] > Fw:
                raise ValueError("FrameMetrics.update: frame %d: ground truth %s / %s does not fit the %d x %d result"
                                 % (i, tuple(dmm.shape), tuple(lab.shape), Fh, Fw))
            if dmm.element_size() != gt[0][0].element_size():
                raise TypeError("FrameMetrics.update: the depth planes of one call have one width")
            pairs.append((dmm.contiguous(), lab.contiguous()))
        if (max(d.shape[0] for d, _ in pairs), max(d.shape[1] for d, _ in pairs)) != (Fh, Fw):
            raise ValueError("FrameMetrics.update: predict_frames sizes its planes by the largest frame of the call, %d x %d; the "
                             "ground truth's largest is %d x %d - these are not the same frames"
                             % (Fh, Fw, max(d.shape[0] for d, _ in pairs), max(d.shape[1] for d, _ in pairs)))
        ids = list(range(self.images_seen, self.images_seen + B)) if ids is None else [int(i) for i in ids]
        if len(ids) != B:
            raise ValueError("FrameMetrics.update: %d ids for %d frames" % (len(ids), B))
        if self.images_seen + B > self.capacity:
            raise RuntimeError("FrameMetrics: %d images exceed capacity_images = %d" % (self.images_seen + B, self.capacity))
        rc = _lib().eval_frames(depth.contiguous(), labels.contiguous(), pairs, self.min_d, self.max_d, self.edges, self._ws,
                                self.images_seen, self.sums, self.measures, self.conf, self.running, self.confusion)
        if rc != 0:
            raise RuntimeError("gwd_eval_frames failed with status %d" % rc)
        self.images_seen += B
        self._ids += ids

    # ---------------------------------------------------------------------------------------------- host side
    def _records(self):
        """(ids, sums, measures, conf) host arrays in feeding order: ONE device->host copy."""
        if self._host is not None:
            return self._host
        n, R = self.images_seen, len(self.regions)
        ids = np.asarray(self._ids, dtype=np.int64)
        if n == 0:
            return ids, np.zeros((0, R, 10)), np.zeros((0, R, 9)), np.zeros((0, 4), dtype=np.int64)
        flat = torch.cat([self.sums[:n].reshape(-1), self.measures[:n].reshape(-1), self.conf[:n].view(torch.float64).reshape(-1)])
        host = flat.cpu().numpy()
        a, b = n * R * 10, n * R * 19
        return ids, host[:a].reshape(n, R, 10), host[a:b].reshape(n, R, 9), host[b:].view(np.int64).reshape(n, 4)

    def per_image(self):
        """Host arrays {"ids" (n,), "sums" (n,R,10), "measures" (n,R,9), "confusion" (n,4)} in feeding order."""
        ids, sums, measures, conf = self._records()
        return {"ids": ids.copy(), "sums": sums.copy(), "measures": measures.copy(), "confusion": conf.copy()}

    def state(self):
        """A picklable host snapshot of the per-image records (numpy arrays and plain values) for FrameMetrics.merge."""
        out = self.per_image()
        out.update(min_depth_eval=self.min_d, max_depth_eval=self.max_d, depth_bins=self.edges)
        return out

    @classmethod
    def merge(cls, states):
        """One metrics object over the records of several state()s (ranks, or calls): compute() folds them in ascending id order.
        The states must share depth range and bins; an id that occurs twice raises."""
        states = list(states)
        if not states:
            raise ValueError("FrameMetrics.merge: no states")
        key = lambda s: (float(s["min_depth_eval"]), float(s["max_depth_eval"]), tuple(float(e) for e in s["depth_bins"]))
        if any(key(s) != key(states[0]) for s in states[1:]):
            raise ValueError("FrameMetrics.merge: the states were taken with different depth ranges or bins")
        ids = np.concatenate([np.asarray(s["ids"], dtype=np.int64) for s in states])
        if len(set(ids.tolist())) != ids.size:
            seen, dup = set(), set()
            for i in ids.tolist():
                (dup if i in seen else seen).add(i)
            raise ValueError("FrameMetrics.merge: image ids occur twice: %s" % sorted(dup)[:8])
        m = cls.__new__(cls)
        m.device = torch.device("cpu")
        m.min_d, m.max_d, m.edges = key(states[0])
        m.n_bins = max(len(m.edges) - 1, 0)
        m.regions = ["all", "glass", "nonglass"] + ["bin%d" % k for k in range(m.n_bins)]
        m._host = (ids, np.concatenate([s["sums"] for s in states]), np.concatenate([s["measures"] for s in states]),
                   np.concatenate([s["confusion"] for s in states]))
        m.images_seen, m._ids, m.capacity = int(ids.size), ids.tolist(), int(ids.size)
        return m

    def compute(self):
        """One device->host copy of the records; they are folded in ascending id order with the kernel's rule (an image enters a
        region's mean when it has a valid pixel there).  Region "all" under the reference's keys (METRIC_NAMES and the five
        segmentation scores, closed as DenseMetrics.compute does), the others as "glass/rms", "bin0/rms", ...; "pixel/<key>" are the
        pixel-weighted variants (the measures of the summed raw sums); "n_images": images per region."""
        ids, sums, measures, conf = self._records()
        order = np.argsort(ids, kind="stable")
        R = len(self.regions)
        run, total = np.zeros((R, 10)), np.zeros((R, 10))
        for i in order:                                        # sequential f64 adds: the kernel's own order when ids ascend
            for r in range(R):
                if sums[i, r, 0] != 0:
                    run[r, :9] += measures[i, r]
                    run[r, 9] += 1
            total += sums[i]
        out = {}
        c = torch.from_numpy(conf.sum(0)).to(torch.float64).reshape(2, 2)
        if float(c.sum()) > 0:
            pos, res, tp = c.sum(1), c.sum(0), c.diagonal()
            iou = tp / torch.clamp(pos + res - tp, min=1.0) * 100
            for lab, v in zip(SEG_LABELS, iou):
                out[lab] = float(v)
            out["Pixel accuracy"] = float(tp.sum() / pos.sum() * 100)
            out["Mean accuracy"] = float((tp / torch.clamp(pos, min=1.0)).mean() * 100)
            out["Mean IU"] = float(iou.mean())
        pix = _measures_from_sums(total)
        for r, name in enumerate(self.regions):
            pre = "" if r == 0 else name + "/"
            for k, m in enumerate(METRIC_NAMES):
                if run[r, 9] > 0:
                    out[pre + m] = float(run[r, k] / run[r, 9])
                if total[r, 0] > 0:
                    out["pixel/" + pre + m] = float(pix[r, k])
        out["n_images"] = {name: int(run[r, 9]) for r, name in enumerate(self.regions)}
        return out

    def worst(self, k, key="rms", region="all"):
        """The k images with the largest `key` in `region` as (id, value) pairs, largest first (ties: lower id first); images
        without a value there (NaN) are left out."""
        ids, _, measures, _ = self._records()
        v = measures[:, self.regions.index(region), METRIC_NAMES.index(key)]
        keep = np.nonzero(~np.isnan(v))[0]
        keep = keep[np.lexsort((ids[keep], -v[keep]))]
        return [(int(ids[i]), float(v[i])) for i in keep[:max(int(k), 0)]]


@torch.no_grad()
def evaluate_frames(session, source, indices=None, batch=8, ensemble=False, size=1024, max_size=1024, pad_to=None, depth_bins=None,
                    metrics=None, planar=False, sensor=None, fused=False, save_dir=None):
    """Scores the samples `indices` (default: all) of a dataset.FrameStore / StreamSource through session.predict_frames at the
    frames' own resolution: `batch` frames per call (at most 16, 8 with ensemble=True), one gwd_eval_frames launch behind each,
    no host sync before the closing copy.  A device-resident FrameStore hands its 16-bit depth planes over in place (record_gt).
    planar=True (a session built with regions= and its planar depth): the metrics are fed depth_planar - the depth with every fitted
    glass region projected onto its plane in inverse depth, the prior GW-Depth's ground truth on glass was built with - in place of
    depth; compare the glass rows of both runs.  Pixels outside the kept regions are the same in both.
    fused=True (a session built with fusion=) with sensor=callable: sensor(indices) returns the RGB-D camera's depth planes of those
    samples as predict_frames(sensor_depth=) takes them, and the metrics are fed depth_fused - the sensor's depth completed behind
    glass - in place of depth.
    save_dir=path: per sample the panels the reference's save_dense_pred and vis_pred_lines show, drawn on the device by ONE
    gwd_render_frames launch per batch (ops.render_frames; the session needs no render=) and written as PNGs by render.save_panels:
    <name>.png (the frame), <name>_depth.png, <name>_seg.png (the prediction: the depth that was scored, the labels),
    <name>_gt-depth.png, <name>_gt-seg.png (the ground truth, read where record_gt / the source left it) and <name>_lines.png (the
    frame with the glass tinted, the regions outlined and the detected lines).  The metrics are the same bit for bit.
    -> metrics.compute() plus "names": {sample index: name} for FrameMetrics.worst.  Pass `metrics` to keep the accumulator."""
    if planar and not (getattr(session, "regions", None) or {}).get("planar"):
        raise ValueError("evaluate_frames(planar=True) needs an InferenceSession built with regions= (and planar=True in it)")
    if fused and planar:
        raise ValueError("evaluate_frames: planar=True and fused=True score different depths; pick one")
    if fused and getattr(session, "fusion", None) is None:
        raise ValueError("evaluate_frames(fused=True) needs an InferenceSession built with fusion= (and regions=)")
    if fused != (sensor is not None) or (sensor is not None and not callable(sensor)):
        raise ValueError("evaluate_frames: fused=True and sensor=callable(indices) go together")
    indices = list(range(len(source))) if indices is None else [int(i) for i in indices]
    limit = hip.EVAL_FRAMES_BATCH // 2 if ensemble else hip.EVAL_FRAMES_BATCH
    if not 0 < int(batch) <= limit:
        raise ValueError("evaluate_frames: 1..%d frames per call%s, got %r" % (limit, " with ensemble=True" if ensemble else "", batch))
    if metrics is None:
        metrics = FrameMetrics(session._device(), session.min_depth, session.max_depth, depth_bins=depth_bins,
                               capacity_images=max(len(indices), 1))
    in_place = getattr(source, "where", None) == "device" and hasattr(source, "record_gt")
    for at in range(0, len(indices), int(batch)):
        idx = indices[at:at + int(batch)]
        if in_place:                                           # views of the records: no widen launch, no copy
            rgb, gt = source.record_rgb(idx), source.record_gt(idx)
        else:
            frames = source.frames(idx)
            rgb, gt = [f[0] for f in frames], [(f[1], f[2]) for f in frames]
        if save_dir is not None:                               # the frames go up once: predict_frames uses a device frame where it is
            rgb = [session._upload_frame(f, session._device()) for f in rgb]
        if fused:
            res = session.predict_frames(rgb, size=size, max_size=max_size, ensemble=ensemble, pad_to=pad_to, sensor_depth=sensor(idx))
            res = dict(res, depth=res["depth_fused"])
        else:
            res = session.predict_frames(rgb, size=size, max_size=max_size, ensemble=ensemble, pad_to=pad_to)
        if planar:
            res = dict(res, depth=res["depth_planar"])
        metrics.update(res, gt, ids=idx)
        if save_dir is not None:
            _save_frames(session, res, rgb, gt, [source.name(i) for i in idx], save_dir,
                         "depth_fused_mm" if fused else "depth_planar_mm" if planar else "depth_mm")
    out = metrics.compute()
    out["names"] = {i: source.name(i) for i in indices}
    return out


SAVE_SUFFIXES = ("", "_depth", "_seg", "_gt-depth", "_gt-seg", "_lines")      # the reference's five files and the lines


def _save_frames(session, res, rgb, gt, names, save_dir, depth_key):
    """Six panels per frame of one predict_frames call, one launch, one copy to the host, PNGs from a thread pool."""
    import os

    from . import ops, render
    dev = res["labels"].device
    B = len(rgb)
    gt_mm = [d if d.dtype == torch.uint16 else d.clamp(0, 65535).to(torch.uint16) for d in (g[0].to(dev) for g in gt)]
    gt_lab = [g[1].to(dev) if g[1].dtype == torch.uint8 else g[1].to(dev).clamp(0, 255).to(torch.uint8) for g in gt]
    nms = getattr(session, "line_nms", None) is not None
    kinds = res.get("profile_kind")
    overlay = {"base": "frame", "tint": 0, "outlines": "region_map" in res, "lines": "kind" if kinds is not None else "score"}
    panels = ["frame", ("depth", 0), ("labels", 0), ("depth", 1), ("labels", 1), overlay]
    canvas = ops.render_frames(res["sizes"], panels, frames=rgb, planes=[res[depth_key], gt_mm], label_planes=[res["labels"], gt_lab],
                               region_map=res.get("region_map"), lines=res["nms_lines" if nms else "lines"],
                               count=res["nms_count" if nms else "count"], order=None if nms else res["order"],
                               scores=res["nms_scores" if nms else "scores"], kinds=kinds, canvas_size=tuple(res["labels"].shape[1:]))
    os.makedirs(save_dir, exist_ok=True)
    paths = [os.path.join(save_dir, str(n).replace(os.sep, "_") + ".png") for n in names]
    return render.save_panels(canvas, [(int(f.shape[0]), int(f.shape[1])) for f in rgb], paths, layout="files", suffixes=SAVE_SUFFIXES)


def close_line_scores(sorted_flags, n_gt):
    """(sAP, sF) times 100 from one column of flags in descending score order (0 false positive, 1 true positive, 2 not scored)."""
    f = np.asarray(sorted_flags)
    f = f[f != 2]
    if n_gt <= 0 or f.size == 0:
        return 0.0, 0.0
    tp = np.cumsum((f == 1).astype(np.float64)) / n_gt                                  # eval-sAP-glassrgbd.py:70-71
    fp = np.cumsum((f == 0).astype(np.float64)) / n_gt
    rec = np.concatenate(([0.0], tp, [1.0]))
    prec = np.concatenate(([0.0], tp / np.maximum(tp + fp, 1e-9), [0.0]))
    env = np.maximum.accumulate(prec[::-1])[::-1]                                       # ap: the precision envelope ...
    step = np.nonzero(rec[1:] != rec[:-1])[0]
    ap = np.sum((rec[step + 1] - rec[step]) * env[step + 1])                            # ... summed where the recall moves
    f_score = np.max(2 * prec * rec / (prec + rec + 1e-10))
    return 100 * float(ap), 100 * float(f_score)


def _line_batch(outputs, targets, samples, device):
    """The LineMetrics.update operands of one evaluate() batch: sizes are the batch tensor's (H, W) - the reference's im.shape -
    and the targets' lines are padded into one (B, G, 4) tensor (shapes only: no device value is read)."""
    logits, lines = outputs["pred_logits"], outputs["pred_lines"]
    B = logits.shape[0]
    H, W = (samples.tensors if hasattr(samples, "tensors") else samples).shape[-2:]
    sizes = torch.tensor([[H, W]] * B, dtype=torch.int32, device=device)
    counts = [int(t["lines"].shape[0]) for t in targets]
    gt = torch.zeros(B, max(max(counts), 1), 4, dtype=torch.float32, device=device)
    for b, t in enumerate(targets):
        if counts[b]:
            gt[b, :counts[b]] = t["lines"][:, :4]
    return logits, lines, sizes, gt, torch.tensor(counts, dtype=torch.int32, device=device)


@torch.no_grad()
def evaluate(model, criterions, postprocessors, data_loader, base_ds, device, output_dir, args, save_dir=None, epoch=0,
             save_dense=False, save_line=False):
    """Same signature and stats as the reference's evaluate() (engine_glassrgbd.py:174-345).  `model` is the module or an
    infer.InferenceSession over it (frozen weight copies, graph replay): each batch's outputs are consumed before the next call.
    With args.line_ap (default off) and --with_line the stats also hold LineMetrics' sAP / sF values and n_gt."""
    if save_dense or save_line:
        raise NotImplementedError("save_dense / save_line write visualisations; outside the accelerated path (SURVEY.md §2)")
    model.eval()
    criterion = criterions[0]
    if getattr(args, "with_line", False) and criterion is not None:
        criterion.eval()
    dm = DenseMetrics(device, getattr(args, "min_depth_eval", 1e-3), getattr(args, "max_depth_eval", 10.0))
    line_sums, n_batches = {}, 0
    lm = LineMetrics(device) if getattr(args, "line_ap", False) and getattr(args, "with_line", False) else None
    for samples, depth_gt, seg_gt, targets, img_name in data_loader:
        samples = samples.to(device)
        targets = [{k: (v.to(device) if torch.is_tensor(v) else v) for k, v in t.items()} for t in targets]
        outputs = model(samples, reflc_mat=None, img_name=img_name[0].strip() if img_name else None)
        if getattr(args, "with_line", False) and criterion is not None:
            loss = criterion(outputs, targets)                                   # :221-229
            wd = criterion.weight_dict
            for k, v in loss.items():
                line_sums[k + "_unscaled"] = line_sums.get(k + "_unscaled", 0.0) + v.detach().double()
                if k in wd:
                    line_sums[k] = line_sums.get(k, 0.0) + v.detach().double() * wd[k]
            line_sums["loss"] = line_sums.get("loss", 0.0) + sum(v.detach().double() * wd[k] for k, v in loss.items() if k in wd)
            n_batches += 1
        if lm is not None:
            lm.update(*_line_batch(outputs, targets, samples, device))
        if getattr(args, "with_dense", True):
            pd = outputs["pred_depth"][-1] if isinstance(outputs["pred_depth"], (list, tuple)) else outputs["pred_depth"]
            ps = outputs["pred_seg"][-1] if isinstance(outputs["pred_seg"], (list, tuple)) else outputs["pred_seg"]
            g = depth_gt.tensors.to(device)
            s = seg_gt.tensors.to(device)
            if depth_gt.mask is not None and bool(depth_gt.mask.any()):          # batches > 1: padding is not evaluated
                pad = depth_gt.mask.to(device).unsqueeze(1)
                g = g.masked_fill(pad, 0.0)
                s = s.masked_fill(pad, 255)
            dm.update(pd, g, ps, s)
    stats = {k: float(v / n_batches) for k, v in line_sums.items()}
    stats.update(dm.compute())
    if lm is not None:
        stats.update(lm.compute())
    return stats
