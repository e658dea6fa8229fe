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
