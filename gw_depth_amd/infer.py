"""Inference session: what engine.TrainStep is for training, for the forward alone.

The plain path (`model.eval(); model(samples)` under no_grad) makes every bf16 / BN-folded weight copy again on every call,
launches every kernel from Python and ends at raw tensors.  An InferenceSession

* freezes the weight copies: it owns an ops.WeightCache(frozen=True) over the storage of every parameter and buffer, so a
  copy is made when its weight is first seen (the first call) and stays; refresh() rewrites all of them in place with one launch;
* replays a captured HIP graph per input signature (B, H, W): forward and post-processing, on one private stream, out of one
  memory pool, least recently used signature dropped beyond graphs.MAX_GRAPHS;
* finishes on the device: the un-padded sizes from the pad mask, the dense post-processing (gwd_dense_postprocess), the line
  post-processing with a ranking (gwd_line_postprocess) and - where asked for (line_nms=) - L-CNN's line NMS over the queries
  (gwd_line_nms), all inside the captured graph, no host sync anywhere.
"""
import contextlib
from collections import OrderedDict

import numpy as np
import torch

from . import data, graphs, hip, ops
from .model import NestedTensor, nested_tensor_from_tensor_list

RESULT_KEYS = ("depth", "depth_mm", "labels", "scores", "lines", "order", "count", "sizes")
NMS_KEYS = ("nms_lines", "nms_scores", "nms_ids", "nms_count")          # added to a result by a session built with line_nms=
_REGION_OPTIONS = ("max_regions", "min_area", "connectivity", "min_depth", "max_depth", "planes", "planar", "max_candidates")
REGION_KEYS = ops.REGION_KEYS                                          # added to predict_frames' result by a session built with regions=
_PROFILE_OPTIONS = ("offset", "max_samples", "min_depth", "max_depth", "hi", "lo")
PROFILE_KEYS = ops.PROFILE_KEYS                                        # ... with line_profiles= (line_points only when intrinsics are passed)
_FUSION_OPTIONS = ("ring", "gap", "trim", "min_ring", "max_rms", "align", "min_align", "min_depth", "max_depth")
FUSION_KEYS = ops.FUSION_KEYS                                          # ... with fusion=, by a call that passes sensor_depth=
_RENDER_OPTIONS = ("panels", "width", "end_radius", "min_score", "score_range")
RENDER_KEYS = ops.RENDER_KEYS                                          # ... with render=
_CLOUD_OPTIONS = ("stride", "edge", "normals", "keep", "depth", "min_depth", "max_depth")
_CLOUD_DEPTHS = ("auto", "depth", "depth_planar", "depth_fused")
CLOUD_KEYS = ops.CLOUD_KEYS                                            # ... with cloud=, by a call that passes intrinsics=
_SCENE_OPTIONS = ("voxel", "max_voxels", "origin", "slots")
_SCENE_VIEW_OPTIONS = ("min_obs", "keep", "footprint", "max_splat")
SCENE_VIEW_KEYS = ("scene_depth", "scene_labels", "scene_index", "scene_rgb", "scene_cloud", "scene_cloud_offsets", "scene_stats")      # ... with scene_view=
_SCENE_VIEW_SOURCE = ("view_depth", "view_labels", "view_index", "view_rgb", "cloud", "cloud_offsets", "voxel_stats")


class InferenceSession:
    """sess = InferenceSession(model, compute_dtype=torch.bfloat16, graph=True, min_depth=..., max_depth=..., score_thresh=0.6)

    sess(samples, reflc_mat=None, img_name=None, taps=None) -> the model's own output dict (the call signature is the
    model's, so a session can stand where the reference passes `model`; .eval() returns the session, .train() raises).
    sess.predict(samples, target_sizes=None, copy=False) -> dict(depth (B,H,W) fp32 clamped to [min_depth, max_depth],
    depth_mm uint16, labels uint8, scores (B,Q), lines (B,Q,4) pixels, order (B,Q) int32, count (B,) int32, sizes (B,2) int32).
    `samples`: NestedTensor, (B,3,H,W) tensor or list of (3,h,w) tensors.  A call leaves the model in eval mode.

    LIFETIME OF OUTPUTS.  With graph=True the results of a replayed signature are the graph's static tensors: they are valid
    until the next call with the same signature (B, H, W), which overwrites them in place (or until more than graphs.MAX_GRAPHS
    other signatures have pushed it out of the cache).  Clone what must live longer, or use
    predict(..., copy=True), which returns fresh tensors.  Eager calls (graph=False, a call with taps, a refused capture)
    return fresh tensors anyway.

    FROZEN WEIGHTS.  compute_dtype=torch.bfloat16: the kernel-side copies are made once.  After load_state_dict or optimizer
    steps call refresh(): one gwd_weight_prep_batch launch rewrites the copies in place, so captured graphs (which read them
    by address) stay valid.  The cache is keyed by address: parameter storage must not move after the session is built -
    TrainStep.__init__ moves every parameter into its flat buffer, so build the session AFTER the TrainStep; refresh() checks
    and raises.  compute_dtype=torch.float32 has no copies to freeze (the kernels read the parameters themselves).
    A session built inside TrainStep.use_ema() keeps the averaged weights after that block has ended: it clones the flat parameter
    buffer and runs on the clone (every parameter, not only the matrices behind the frozen copies); refresh() re-clones.

    sess.predict_frames(frames, size=1024, max_size=1024, ensemble=False, pad_to=None, copy=False): decoded uint8 (h,w,3) camera
    frames in, the same results at every frame's OWN size out (see the method).

    LINE NMS.  line_nms=None (the default): the line results are the raw queries, as above.  line_nms=t (the reference's consumers
    use 0.010 and 0.015 of the image diagonal): predict / predict_frames also return NMS_KEYS - nms_lines (B,C,4) float64
    (x1, y1, x2, y2) pixels at the size `lines` are scaled to, nms_scores (B,C), nms_ids (B,C) int32, nms_count (B,) int32:
    row r of an image is its r-th kept (clipped) line, rows from nms_count on hold 0 / 0 / -1 (ops.line_nms).  The queries are
    taken by score (line_nms_order="score", the ranking `order`) or in query order as the reference's script takes them
    ("query"); line_nms_min_score=s lets only queries with score > s take part.  C = Q; with predict_frames(ensemble=True)
    the mirrored twin's queries, mirrored back, take part as well: C = 2 Q and ids >= Q name the twin's queries.

    GLASS REGIONS.  regions=None (the default): nothing is allocated and predict_frames issues the launches and returns the keys it
    always did.  regions=True or a dict of ops.glass_regions' keyword arguments (max_regions, min_area, connectivity, planes,
    planar, max_candidates; min_depth / max_depth default to the session's): predict_frames also returns REGION_KEYS (those the
    switches ask for, ops.region_keys) - the connected glass regions of every frame, their records, their planes in inverse depth
    and the depth those planes predict - computed from its own labels / depth_mm / depth / sizes behind the resized
    post-processing, on the session's stream, as fresh tensors, with no host sync.  predict() does not take part.

    LINE PROFILES.  line_profiles=None (the default): nothing is allocated, predict_frames issues the launches and returns the keys
    it always did.  line_profiles=True or a dict of ops.line_profiles' options (offset, max_samples, hi, lo; min_depth / max_depth
    default to the session's): predict_frames also returns PROFILE_KEYS - every detected line walked through the frame's own labels /
    depth_mm (and region_map, with regions=) in one launch behind them: the depth of its two ends, the side the glass lies on, the
    pane it frames.  With line_nms the rows are the NMS survivors (nms_lines, nms_count; the mirrored twin's candidates included
    under ensemble=True), without it the count[b] lines above score_thresh, reached through `order`.  predict_frames(intrinsics=)
    adds line_points, the ends in camera coordinates.  predict() does not take part.

    SENSOR FUSION.  fusion=None (the default): nothing is allocated, predict_frames issues the launches and returns the keys it always
    did.  fusion=True or a dict of ops.sensor_fusion's options (ring, gap, trim, min_ring, max_rms, align, min_align; min_depth /
    max_depth default to the session's) needs regions=: predict_frames(sensor_depth=...) - the depth planes of an RGB-D camera,
    uint16 millimetres, 0 = no reading, registered to the frames - also returns FUSION_KEYS: the sensor's depth with every glass
    region rewritten to the plane fitted from the depth measured on its frame, the network's depth scaled to the sensor where no
    plane can be fitted and in the sensor's holes, and where each pixel came from; computed behind the regions on the session's
    stream, as fresh tensors, with no host sync.  A call without sensor_depth returns what it returns today.  predict() does not
    take part.

    RENDER.  render=None (the default): nothing is allocated, predict_frames issues the launches and returns the keys it always did.
    render=True or a dict (panels, and ops.render_frames' options width, end_radius, min_score, score_range): predict_frames also
    returns RENDER_KEYS - canvas (B, P, Fh, Fw, 3) uint8, RGB panels of the call's own frames and results at frame size, drawn by ONE
    launch (gwd_render_frames) behind everything else on the session's stream, a fresh tensor, no host sync; render.save_panels
    writes it out.  The default panels: the frame with the glass tinted, the regions outlined (with regions=) and the lines on top -
    the NMS survivors with line_nms, else the lines above score_thresh through `order`; coloured by profile_kind with
    line_profiles=, else by score; the depth (depth_fused_mm when the call fused, else depth_mm); the labels.  Panels of one's own
    are ops.render_frames' with the planes named: base ("depth", "depth_mm" | "depth_planar_mm" | "depth_fused_mm" | "depth" = the
    default choice) or ("labels", "labels" | "region_map" | "fused_source" | "fusion_ring"), tint: such a uint8 name.  A panel that
    names a plane the session does not produce raises here.  predict() does not take part.

    POINT CLOUD.  cloud=None (the default): nothing is allocated, predict_frames issues the launches and returns the keys it always did.
    cloud=True or a dict (ops.point_cloud's options stride, edge, normals, keep; min_depth / max_depth default to the session's; depth:
    "auto" - depth_fused when the call fused, else depth_planar when the session makes it, else depth - or one of those three by name;
    a depth this session does not produce raises here): predict_frames(intrinsics=..., poses=None) also returns CLOUD_KEYS - the valid
    pixels of every frame unprojected, packed frame after frame in raster order as 32-byte records (position, normal, the frame's
    colour, label, region, fused_source, frame, flags: gw_depth_amd.cloud.fields) with their exclusive prefix, in three launches
    (gwd_point_cloud) behind fusion and profiles and before render, on the session's stream, as fresh tensors, no host sync; the
    uploaded frames are read where they lie, region_map / planes (pane normals) and fused_source take part when the session produces
    them.  A call without intrinsics returns what it returns today.  predict() does not take part.

    SCENE MAP.  scene=None (the default): nothing is allocated or launched, predict_frames returns the keys it always did.  scene=a
    gw_depth_amd.cloud.SceneMap, or a dict (voxel, max_voxels, origin, slots) from which one is built on the model's device, needs
    cloud=: predict_frames(intrinsics=..., poses=...) integrates the call's cloud into sess.scene (five launches, gwd_scene_integrate)
    behind the cloud and before render, on the session's stream, no host sync; the returned keys do not change - sess.scene.extract()
    gives the merged map whenever it is wanted.  A call with intrinsics but without poses raises: camera-frame clouds share no world.
    A call without intrinsics returns what it returns today and leaves the map alone.  predict() does not take part.

    SCENE VIEW.  scene_view=None (the default): nothing is allocated, launched or returned that is not there without it.  scene_view=True
    or a dict (min_obs, keep, footprint - None: the map's voxel - max_splat) needs scene=: predict_frames(intrinsics=..., poses=...)
    first looks at sess.scene from the call's own cameras - its intrinsics, poses and frame sizes, the session's min_depth / max_depth,
    the result planes' Fh x Fw - BEFORE this call's cloud is integrated (SceneMap.view: six launches, gwd_scene_extract +
    gwd_cloud_view, no host sync) and adds SCENE_VIEW_KEYS: scene_depth / scene_labels / scene_index / scene_rgb - what the earlier
    calls said about every pixel of these frames (0 / 255 / -1 / 0 where they said nothing; all of it on the first call) - and
    scene_cloud / scene_cloud_offsets / scene_stats, the extraction scene_index points into.  A call without intrinsics returns what
    it returns today.  predict() does not take part.

    A ragged batch is top-left aligned (nested_tensor_from_tensor_list), so the un-padded (h, w) of each image are counted
    from the pad mask on the device; padding comes out as depth 0 / millimetres 0 / label 255."""

    def __init__(self, model, compute_dtype=torch.bfloat16, graph=True, min_depth=1e-3, max_depth=10.0, score_thresh=0.6,
                 line_nms=None, line_nms_order="score", line_nms_min_score=None, regions=None, line_profiles=None, fusion=None,
                 render=None, cloud=None, scene=None, scene_view=None):
        if compute_dtype not in (torch.float32, torch.bfloat16):
            raise TypeError("compute_dtype must be torch.float32 or torch.bfloat16")
        if line_nms_order not in ("score", "query"):
            raise ValueError("line_nms_order must be 'score' or 'query', got %r" % (line_nms_order,))
        if line_nms is not None and not float(line_nms) >= 0.0:
            raise ValueError("line_nms must be None or a fraction of the image diagonal >= 0, got %r" % (line_nms,))
        self.line_nms = None if line_nms is None else float(line_nms)
        self.line_nms_order = line_nms_order
        self.line_nms_min_score = None if line_nms_min_score is None else float(line_nms_min_score)
        self.model = model
        self.compute_dtype = compute_dtype
        self.use_graph = bool(graph)
        self.min_depth, self.max_depth, self.score_thresh = float(min_depth), float(max_depth), float(score_thresh)
        if regions is not None and regions is not True and not isinstance(regions, dict):
            raise TypeError("regions must be None, True or a dict of ops.glass_regions' keyword arguments, got %r" % (regions,))
        if isinstance(regions, dict) and set(regions) - set(_REGION_OPTIONS):
            raise TypeError("regions: unknown option(s) %s (known: %s)" % (sorted(set(regions) - set(_REGION_OPTIONS)), ", ".join(_REGION_OPTIONS)))
        self.regions = None if regions is None else ops.check_region_options(
            **dict({"min_depth": self.min_depth, "max_depth": self.max_depth}, **(regions if isinstance(regions, dict) else {})))
        if line_profiles is not None and line_profiles is not True and not isinstance(line_profiles, dict):
            raise TypeError("line_profiles must be None, True or a dict of ops.line_profiles' options, got %r" % (line_profiles,))
        if isinstance(line_profiles, dict) and set(line_profiles) - set(_PROFILE_OPTIONS):
            raise TypeError("line_profiles: unknown option(s) %s (known: %s)"
                            % (sorted(set(line_profiles) - set(_PROFILE_OPTIONS)), ", ".join(_PROFILE_OPTIONS)))
        self.line_profiles = None if line_profiles is None else ops.check_line_profile_options(
            **dict({"min_depth": self.min_depth, "max_depth": self.max_depth}, **(line_profiles if isinstance(line_profiles, dict) else {})))
        if fusion is not None and fusion is not True and not isinstance(fusion, dict):
            raise TypeError("fusion must be None, True or a dict of ops.sensor_fusion's options, got %r" % (fusion,))
        if isinstance(fusion, dict) and set(fusion) - set(_FUSION_OPTIONS):
            raise TypeError("fusion: unknown option(s) %s (known: %s)" % (sorted(set(fusion) - set(_FUSION_OPTIONS)), ", ".join(_FUSION_OPTIONS)))
        if fusion is not None and self.regions is None:
            raise ValueError("fusion= needs a session built with regions= (the panes it completes are the glass regions)")
        self.fusion = None if fusion is None else ops.check_fusion_options(
            **dict({"min_depth": self.min_depth, "max_depth": self.max_depth}, **(fusion if isinstance(fusion, dict) else {})))
        self.render = self._check_render(render)
        self.cloud = self._check_cloud(cloud)
        self.scene = self._check_scene(scene)
        self.scene_view = self._check_scene_view(scene_view)
        self._cache = graphs.GraphCache()                  # every signature is captured at its first sight
        self._graphs = self._cache.entries                 # signature -> {"graph": chain of one, or None, ...}, least recently used first
        self._side = graphs.GraphSide()
        self._addr = self._addresses()
        spans = [(t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()) for t in self._storage() if t.numel()]
        # built inside TrainStep.use_ema(): the averaged weights leave the parameters when that block ends, so the session keeps a copy
        # of the flat buffer and runs every forward on it (biases and norms are read in place, not through the frozen copies)
        ts = getattr(model, "_gwd_ema_step", None)
        self._own = None if ts is None else (ts, ts.flat_p.clone())
        if self._own is not None:
            flat = self._own[1]
            spans.append((flat.data_ptr(), flat.data_ptr() + flat.numel() * flat.element_size()))
        self.weights = ops.WeightCache(spans, frozen=True) if compute_dtype == torch.bfloat16 else None

    # ------------------------------------------------------------------ render=
    def _check_render(self, render):
        """render= -> None or dict(panels, options); every panel checked against what this session produces."""
        from . import render as R
        if render is None:
            return None
        if render is not True and not isinstance(render, dict):
            raise TypeError("render must be None, True or a dict of panels and ops.render_frames' options, got %r" % (render,))
        given = render if isinstance(render, dict) else {}
        if set(given) - set(_RENDER_OPTIONS):
            raise TypeError("render: unknown option(s) %s (known: %s)" % (sorted(set(given) - set(_RENDER_OPTIONS)), ", ".join(_RENDER_OPTIONS)))
        R.check_options(**{k: v for k, v in given.items() if k != "panels"})
        planar = self.regions is not None and "depth_planar_mm" in ops.region_keys(self.regions["planes"], self.regions["planar"])
        depth_names = ("depth", "depth_mm") + (("depth_planar_mm",) if planar else ()) + (("depth_fused_mm",) if self.fusion is not None else ())
        label_names = ("labels",) + (("region_map",) if self.regions is not None else ()) + \
            (("fused_source", "fusion_ring") if self.fusion is not None else ())
        panels = given.get("panels")
        if panels is None:
            panels = [{"base": "frame", "tint": "labels", "outlines": self.regions is not None,
                       "lines": "kind" if self.line_profiles is not None else "score"},
                      {"base": ("depth", "depth")}, {"base": ("labels", "labels")}]
        if isinstance(panels, dict) or not isinstance(panels, (list, tuple)):
            raise ValueError("render: panels is a list of panels")
        named = []
        for k, p in enumerate(panels):
            p = dict(p) if isinstance(p, dict) else {"base": p}
            base = p.get("base", "black")
            if isinstance(base, str) and base in ("depth", "labels"):
                base = (base, base)
            if isinstance(base, tuple) and len(base) == 2 and base[0] in ("depth", "labels"):
                names = depth_names if base[0] == "depth" else label_names
                if base[1] not in names:
                    raise ValueError("render: panel %d names the %s plane %r, this session produces %s" % (k, base[0], base[1], ", ".join(names)))
            if p.get("tint") is not None and p["tint"] not in label_names:
                raise ValueError("render: panel %d tints by %r, this session produces %s" % (k, p["tint"], ", ".join(label_names)))
            if p.get("outlines") and self.regions is None:
                raise ValueError("render: panel %d draws region outlines: that needs a session built with regions=" % k)
            if p.get("lines") == "kind" and self.line_profiles is None:
                raise ValueError("render: panel %d colours lines by kind: that needs a session built with line_profiles=" % k)
            p["base"] = base
            named.append(p)
        # the rest of every panel is checked as ops.render_frames will check it (indices stand in for the names)
        stand_in = lambda p: dict(p, base=(p["base"][0], 0) if isinstance(p["base"], tuple) and len(p["base"]) == 2 else p["base"],
                                  tint=None if p.get("tint") is None else 0)
        R.check_panels([stand_in(p) for p in named])
        return dict(panels=named, options={k: v for k, v in given.items() if k != "panels"})

    def _render(self, frames, res, post, B, fused):
        """The canvas of one predict_frames call from the tensors it already holds: planes are handed over by name."""
        nms = self.line_nms is not None
        planes, label_planes, panels = [], [], []

        def index(names, pool, name):
            if name == "depth":
                name = "depth_fused_mm" if fused else "depth_mm"
            if name not in res:
                raise ValueError("predict_frames: a render panel names %r, which this call did not produce (sensor_depth=?)" % name)
            if name not in names:
                names.append(name)
                pool.append(res[name])
            return names.index(name)

        depth_names, label_names = [], []
        for p in self.render["panels"]:
            p = dict(p)
            if isinstance(p["base"], tuple):
                kind, name = p["base"]
                p["base"] = (kind, index(depth_names, planes, name) if kind == "depth" else index(label_names, label_planes, name))
            if p.get("tint") is not None:
                p["tint"] = index(label_names, label_planes, p["tint"])
            panels.append(p)
        return ops.render_frames(res["sizes"], panels, frames=frames, planes=planes, label_planes=label_planes,
                                 region_map=res.get("region_map"), lines=post["nms_lines" if nms else "lines"][:B],
                                 count=post["nms_count" if nms else "count"][:B], order=None if nms else post["order"][:B],
                                 scores=post["nms_scores" if nms else "scores"][:B], kinds=res.get("profile_kind"),
                                 canvas_size=tuple(res["labels"].shape[1:]), **self.render["options"])

    # ------------------------------------------------------------------ cloud=
    def _check_cloud(self, cloud):
        """cloud= -> None or dict(depth, options); the depth checked against what this session produces."""
        if cloud is None:
            return None
        if cloud is not True and not isinstance(cloud, dict):
            raise TypeError("cloud must be None, True or a dict of ops.point_cloud's options and depth, got %r" % (cloud,))
        given = cloud if isinstance(cloud, dict) else {}
        if set(given) - set(_CLOUD_OPTIONS):
            raise TypeError("cloud: unknown option(s) %s (known: %s)" % (sorted(set(given) - set(_CLOUD_OPTIONS)), ", ".join(_CLOUD_OPTIONS)))
        depth = given.get("depth", "auto")
        planar = self.regions is not None and "depth_planar" in ops.region_keys(self.regions["planes"], self.regions["planar"])
        names = ("depth",) + (("depth_planar",) if planar else ()) + (("depth_fused",) if self.fusion is not None else ())
        if depth not in _CLOUD_DEPTHS:
            raise ValueError("cloud: depth must be one of %s, got %r" % (", ".join(_CLOUD_DEPTHS), depth))
        if depth != "auto" and depth not in names:
            raise ValueError("cloud: depth names %r, this session produces %s" % (depth, ", ".join(names)))
        options = ops.check_cloud_options(**dict({"min_depth": self.min_depth, "max_depth": self.max_depth},
                                                 **{k: v for k, v in given.items() if k != "depth"}))
        return dict(depth=depth, planar=planar, options=options)

    def _cloud(self, frames, frame_sizes, res, intrinsics, poses):
        """The cloud of one predict_frames call from the tensors it already holds."""
        name = self.cloud["depth"]
        if name == "auto":
            name = "depth_fused" if "depth_fused" in res else "depth_planar" if self.cloud["planar"] else "depth"
        if name not in res:
            raise ValueError("predict_frames: cloud= names %r, which this call did not produce (sensor_depth=?)" % name)
        panes = "planes" in res
        Fh, Fw = res["labels"].shape[1:]
        rows = ops.cloud_capacity(len(frames), Fh, Fw, self.cloud["options"]["stride"], frame_sizes)      # exact: the sizes are known here
        return ops.point_cloud(res[name], res["labels"], res["sizes"], intrinsics, frames=frames,
                               region_map=res["region_map"] if panes else None, region_count=res["region_count"] if panes else None,
                               planes=res["planes"] if panes else None, source=res.get("fused_source"), poses=poses,
                               frame_sizes=frame_sizes, capacity=rows, **self.cloud["options"])

    # ------------------------------------------------------------------ scene=
    def _check_scene(self, scene):
        """scene= -> None or a cloud.SceneMap (the one handed over, or one built from a dict of its parameters)."""
        from . import cloud as PC
        if scene is None:
            return None
        if not isinstance(scene, (dict, PC.SceneMap)):
            raise TypeError("scene must be None, a gw_depth_amd.cloud.SceneMap or a dict of its parameters, got %r" % (scene,))
        if self.cloud is None:
            raise ValueError("scene= needs a session built with cloud= (the map is made of the calls' clouds)")
        if isinstance(scene, PC.SceneMap):
            return scene
        if set(scene) - set(_SCENE_OPTIONS):
            raise TypeError("scene: unknown option(s) %s (known: %s)" % (sorted(set(scene) - set(_SCENE_OPTIONS)), ", ".join(_SCENE_OPTIONS)))
        if "voxel" not in scene or "max_voxels" not in scene:
            raise TypeError("scene: a dict names voxel and max_voxels")
        return PC.SceneMap(device=self._device(), **scene)      # validates before anything is allocated or launched

    # ------------------------------------------------------------------ the reference passes `model`
    def eval(self):
        return self

    def train(self, mode=True):
        if mode:
            raise RuntimeError("an InferenceSession does not train; use engine.TrainStep on the model")
        return self

    def to(self, *a, **k):
        raise RuntimeError("an InferenceSession is bound to the addresses of its model's parameters; move the model first, "
                           "then build the session")

    # ------------------------------------------------------------------ weights
    def _storage(self):
        return [p.data for p in self.model.parameters()] + [b for b in self.model.buffers() if b.is_floating_point()]

    def _addresses(self):
        return [t.data_ptr() for t in self._storage()]

    def refresh(self):
        """The weights changed in place (load_state_dict, optimizer steps): bring the frozen copies up to date - the folded
        FrozenBN scale / shift pairs and, in ONE launch, every bf16 weight copy - on the session's stream, in place."""
        if self._addresses() != self._addr:
            raise RuntimeError("gw_depth_amd: parameter storage moved after the InferenceSession was built (a TrainStep built "
                               "later moves every parameter into its flat buffer; model.to() re-allocates): build a new session")
        if self._own is not None:                          # a session with its own weights takes what the parameters hold now
            self._own[1].copy_(self._own[0].flat_p)
        with torch.no_grad(), self._on_stream(), self._own_weights():
            for m in self.model.modules():
                if hasattr(m, "folded"):
                    m.folded()
            if self.weights is not None:
                self.weights.refresh()
        return self

    @contextlib.contextmanager
    def _own_weights(self):
        """A session built inside TrainStep.use_ema(): for the length of a forward every trainable parameter is a view of the session's
        own copy of the flat buffer (host-side pointer moves only: nothing is launched, a captured graph keeps the copy's addresses)."""
        if self._own is None:
            yield
            return
        ts, flat = self._own
        keep = []
        try:
            for n, p in ts.params.items():
                keep.append((p, p.data))
                o = ts.offsets[n]
                p.data = flat[o:o + p.numel()].view(p.shape)
            yield
        finally:
            for p, d in keep:
                p.data = d

    # ------------------------------------------------------------------ one sync-free pass
    def _forward(self, images, mask, taps=None):
        model = self.model
        if model.training:
            model.eval()
        keep = model.compute_dtype
        model.compute_dtype = self.compute_dtype
        weights = self.weights if (self.weights is not None and images.is_cuda) else contextlib.nullcontext()
        try:
            with weights, torch.no_grad(), self._own_weights():
                return model(NestedTensor(images, mask), taps=taps)
        finally:
            model.compute_dtype = keep

    def _post(self, out, mask, target, twin=0):
        """Device post-processing of one forward.  target (B,2) int32: the size the lines are scaled to, rows < 0 = the
        un-padded input size.  twin (line NMS only): images twin .. 2 twin - 1 are the mirrored copies of the first twin images."""
        with torch.no_grad():
            sizes = torch.stack([(~mask[:, :, 0]).sum(1, dtype=torch.int32), (~mask[:, 0, :]).sum(1, dtype=torch.int32)], dim=1)
            depth, mm, labels = ops.dense_postprocess(out["pred_depth"][-1], out["pred_seg"], sizes, self.min_depth, self.max_depth)
            lsz = torch.where(target >= 0, target, sizes)
            raw_logits, raw_lines = out["pred_logits"], out["pred_lines"]
            if self.line_nms is not None:                  # two consumers: widen the bf16 outputs once, not once per consumer
                raw_logits, raw_lines = raw_logits.float().contiguous(), raw_lines.float().contiguous()
            scores, lines, order, count = ops.line_postprocess(raw_logits, raw_lines, lsz, self.score_thresh)
            res = {"depth": depth, "depth_mm": mm, "labels": labels, "scores": scores, "lines": lines, "order": order,
                   "count": count, "sizes": sizes}
            if self.line_nms is not None:
                nms = ops.line_nms(raw_logits, raw_lines, lsz[:lsz.shape[0] - twin], self.line_nms,
                                   order=order if self.line_nms_order == "score" else None, min_score=self.line_nms_min_score,
                                   twin=twin)
                res.update(zip(NMS_KEYS, nms))
        return res

    def _pass(self, st):
        out = self._forward(st["images"], st["mask"])
        return out, self._post(out, st["mask"], st["target"], st["twin"])

    # ------------------------------------------------------------------ graphs
    def _on_stream(self):
        """Everything a graph-mode session launches runs on its one private stream (graphs.GraphSide.handover); an eager session
        stays on the caller's stream."""
        return self._side.handover(self.use_graph and torch.cuda.is_available())

    def _count_memsets(self, st):
        return graphs.count_memsets(lambda: self._pass(st))

    def _graph_entry(self, images, mask, twin=0):
        key = tuple(int(images.shape[i]) for i in (0, 2, 3)) + (("twin",) if twin else ())
        verdict, ent = self._cache.lookup(key)
        if verdict != "capture":
            return ent
        static = lambda: {"images": images.clone(), "mask": mask.clone(),
                          "target": torch.full((key[0], 2), -1, dtype=torch.int32, device=images.device), "twin": twin}
        return self._side.attempt(self._cache, key, static, lambda st, cut: self._pass(st), lambda st: self._count_memsets(st),
                                  "input", "forward")

    @property
    def graphs(self):
        """{(B, H, W): {"captured": bool, "reason": why not}} for every signature in the cache, oldest first (a session with
        line_nms keeps the ensemble passes of predict_frames under (2B, H, W, "twin"): their NMS pairs the images up)."""
        return OrderedDict((k, {"captured": e["graph"] is not None, "reason": e.get("reason")}) for k, e in self._graphs.items())

    # ------------------------------------------------------------------ calls
    @staticmethod
    def _decompose(samples):
        if isinstance(samples, (list, tuple, torch.Tensor)):
            samples = nested_tensor_from_tensor_list(samples)
        images, mask = samples.decompose()
        if mask is None:
            mask = torch.zeros((images.shape[0],) + tuple(images.shape[-2:]), dtype=torch.bool, device=images.device)
        return images, mask

    def _target(self, target_sizes, B, device):
        if target_sizes is None:
            return None
        t = torch.as_tensor(target_sizes).to(device=device, dtype=torch.int32, non_blocking=True)
        if tuple(t.shape) != (B, 2):
            raise ValueError("target_sizes must be (B, 2) = (h, w) per image, got %s" % (tuple(t.shape),))
        return t

    def _run(self, samples, target_sizes, want_post, taps=None, twin=0):
        images, mask = self._decompose(samples)
        B = images.shape[0]
        target = self._target(target_sizes, B, images.device)
        if self.use_graph and images.is_cuda and taps is None:
            ent = self._graph_entry(images, mask, twin)
            if ent["graph"] is not None:
                st = ent["static"]
                with self._on_stream():
                    st["images"].copy_(images, non_blocking=True)
                    st["mask"].copy_(mask, non_blocking=True)
                    if target is None:
                        st["target"].fill_(-1)
                    else:
                        st["target"].copy_(target, non_blocking=True)
                    for g, _ in ent["graph"]:
                        g.replay()
                return ent["result"]
        with self._on_stream():
            out = self._forward(images, mask, taps=taps)
            post = None
            if want_post:
                if target is None:
                    target = torch.full((B, 2), -1, dtype=torch.int32, device=images.device)
                post = self._post(out, mask, target, twin)
        return out, post

    def __call__(self, samples, reflc_points=None, reflc_mat=None, img_name=None, taps=None):
        """The model's own output dict.  reflc_points / reflc_mat / img_name are accepted as the model accepts them (unused)."""
        return self._run(samples, None, False, taps=taps)[0]

    forward = __call__

    def predict(self, samples, target_sizes=None, copy=False):
        """Post-processed results (RESULT_KEYS, and NMS_KEYS from a session with line_nms).  target_sizes (B,2) = (h, w): scale
        the lines to another size than the un-padded input (the reference passes orig_size for evaluation).  copy=False: see
        LIFETIME OF OUTPUTS."""
        res = self._run(samples, target_sizes, True)[1]
        if copy:
            res = {k: v.clone() for k, v in res.items()}
        return res

    # ------------------------------------------------------------------ from camera frames to results at frame size
    def _device(self):
        return next(self.model.parameters()).device

    @staticmethod
    def _upload_frame(frame, device):
        """A host frame reaches the device through pinned memory, without blocking; a device frame is used where it is."""
        if frame.device == device:
            return frame
        if device.type == "cuda" and frame.device.type == "cpu":
            frame = frame.pin_memory()
        return frame.to(device, non_blocking=True)

    @staticmethod
    def _sensor_plane(sensor_depth, frame_sizes, device):
        """sensor_depth -> one zeroed (B, Fh, Fw) uint16 plane on the device with every frame's readings top-left, as the dense
        results lie.  Host planes go through pinned memory; nothing waits for the device."""
        B = len(frame_sizes)
        Fh, Fw = max(s[0] for s in frame_sizes), max(s[1] for s in frame_sizes)
        if torch.is_tensor(sensor_depth):
            if sensor_depth.dtype != torch.uint16 or tuple(sensor_depth.shape) != (B, Fh, Fw):
                raise ValueError("predict_frames: sensor_depth as one tensor must be uint16 %s, got %s %s"
                                 % ((B, Fh, Fw), sensor_depth.dtype, tuple(sensor_depth.shape)))
            return InferenceSession._upload_frame(sensor_depth, device).contiguous()
        if not isinstance(sensor_depth, (list, tuple)) or len(sensor_depth) != B:
            raise ValueError("predict_frames: sensor_depth is a list of %d uint16 (h, w) tensors or one (B, Fh, Fw) tensor" % B)
        for k, (t, (h, w)) in enumerate(zip(sensor_depth, frame_sizes)):
            if not torch.is_tensor(t) or t.dtype != torch.uint16 or tuple(t.shape) != (h, w):
                raise ValueError("predict_frames: sensor_depth[%d] must be a uint16 (%d, %d) tensor like frame %d, got %s"
                                 % (k, h, w, k, "%s %s" % (t.dtype, tuple(t.shape)) if torch.is_tensor(t) else type(t).__name__))
        plane = torch.zeros((B, Fh, Fw), dtype=torch.uint16, device=device)
        for k, (t, (h, w)) in enumerate(zip(sensor_depth, frame_sizes)):
            plane[k, :h, :w].copy_(InferenceSession._upload_frame(t, device), non_blocking=True)
        return plane

    def _check_scene_view(self, scene_view):
        """scene_view= -> None or SceneMap.view's options as a dict."""
        if scene_view is None:
            return None
        if scene_view is not True and not isinstance(scene_view, dict):
            raise TypeError("scene_view must be None, True or a dict of %s, got %r" % (", ".join(_SCENE_VIEW_OPTIONS), scene_view))
        if self.scene is None:
            raise ValueError("scene_view= needs a session built with scene= (it is the map that is looked at)")
        given = scene_view if isinstance(scene_view, dict) else {}
        if set(given) - set(_SCENE_VIEW_OPTIONS):
            raise TypeError("scene_view: unknown option(s) %s (known: %s)" % (sorted(set(given) - set(_SCENE_VIEW_OPTIONS)), ", ".join(_SCENE_VIEW_OPTIONS)))
        from . import cloud as PC
        opt = dict(given)
        footprint = opt.pop("footprint", None)
        extract = PC.check_extract_options(opt.pop("min_obs", 1), opt.pop("keep", "all"))
        view = ops.check_view_options(min_depth=self.min_depth, max_depth=self.max_depth,
                                      footprint=self.scene.voxel if footprint is None else footprint, keep=extract["keep"], **opt)
        return dict(min_obs=extract["min_obs"], keep=extract["keep"], footprint=footprint, max_splat=view["max_splat"])

    def predict_frames(self, frames, size=1024, max_size=1024, ensemble=False, pad_to=None, copy=False, intrinsics=None,
                       sensor_depth=None, poses=None):
        """Decoded camera frames in, results at each frame's own size out.  frames: list of uint8 (h,w,3) tensors, host or device,
        of any sizes: at most hip.AUGMENT_BATCH (16) per call, half that with ensemble=True (the forward batch is 2B); no side
        above 16384.  The reference's evaluation transform (RandomResize([size], max_size), ToTensor, Normalize:
        src/datasets/coco.py:84-91) runs on the device (DeviceAugment(train=False) + device_collate(pad_to=pad_to)), the forward
        is predict()'s (one graph per (B or 2B, H, W)), and ONE kernel (gwd_dense_postprocess_resized) brings depth, millimetres
        and labels back to frame size: bilinear by F.interpolate(align_corners=False)'s rule over the un-padded network region.
        ensemble=True: the prediction of the mirrored frame, mirrored back, is averaged in (depth: mean; logits: sum) - the
        mirrored copies ride in the same resize launches and the same forward.

        A session with line_nms adds NMS_KEYS in frame pixels; with ensemble=True the mirrored frames' queries, mirrored back,
        are candidates too (C = 2 Q rows per frame).  Without line_nms the twin's lines stay unused.

        A session with regions= adds REGION_KEYS (GLASS REGIONS above), at frame size.

        A session with line_profiles= adds PROFILE_KEYS (LINE PROFILES above); intrinsics: (B,4) (fx, fy, cx, cy) per frame at frame
        size (a tensor or nested sequence) adds line_points - a session with neither line_profiles= nor cloud= raises.

        A session with fusion= and sensor_depth - a list of B uint16 (h, w) tensors at each frame's own size, host or device, or one
        (B, Fh, Fw) uint16 tensor, millimetres, 0 = no reading - adds FUSION_KEYS (SENSOR FUSION above); sensor_depth without
        fusion= raises, a plane of another size than its frame raises and names the frame.

        A session with cloud= and intrinsics adds CLOUD_KEYS (POINT CLOUD above); poses: (B,3,4) camera-to-world rows [R | t] per frame
        (a tensor or nested sequence) puts the points and normals into world coordinates - poses without cloud=, or without
        intrinsics, raise.  A session with scene= also integrates that cloud into sess.scene (SCENE MAP above) and takes no
        intrinsics without poses.

        A session with render= adds RENDER_KEYS (RENDER above).

        -> RESULT_KEYS + "net_sizes": depth / depth_mm / labels (B, Fh, Fw) with (Fh, Fw) the largest frame of the call (outside
        a frame 0 / 0 / 255), sizes (B,2) the FRAME sizes, net_sizes (B,2) the un-padded network sizes, scores / lines / order /
        count as predict() gives them for the B frames, lines in frame pixels.  The dense results, sizes and net_sizes are fresh
        tensors on every call; the four line results follow copy= as in predict() (LIFETIME OF OUTPUTS).  No host sync."""
        B = len(frames)
        limit = hip.AUGMENT_BATCH // 2 if ensemble else hip.AUGMENT_BATCH
        if not 0 < B <= limit:
            raise ValueError("predict_frames: 1..%d frames per call%s, got %d" % (limit, " with ensemble=True" if ensemble else "", B))
        for f in frames:
            if not torch.is_tensor(f) or f.dtype != torch.uint8 or f.dim() != 3 or f.shape[2] != 3 or 0 in f.shape:
                raise ValueError("predict_frames: frames are uint8 (h, w, 3) tensors")
        dev = self._device()
        if sensor_depth is not None and self.fusion is None:
            raise ValueError("predict_frames: sensor_depth needs a session built with fusion=")
        if intrinsics is not None:
            if self.line_profiles is None and self.cloud is None:
                raise ValueError("predict_frames: intrinsics need a session built with line_profiles= or cloud=")
            intrinsics = torch.as_tensor(intrinsics, dtype=torch.float64)
            if tuple(intrinsics.shape) != (B, 4):
                raise ValueError("predict_frames: intrinsics must be (%d, 4) = (fx, fy, cx, cy) per frame, got %s" % (B, tuple(intrinsics.shape)))
            intrinsics = intrinsics.to(dev, non_blocking=True)
        if poses is not None:
            if self.cloud is None:
                raise ValueError("predict_frames: poses need a session built with cloud=")
            if intrinsics is None:
                raise ValueError("predict_frames: poses place a cloud, and a cloud needs intrinsics")
            poses = poses.to(torch.float64) if torch.is_tensor(poses) else torch.from_numpy(np.asarray(poses, dtype=np.float64))
            if tuple(poses.shape) != (B, 3, 4):
                raise ValueError("predict_frames: poses must be (%d, 3, 4) = rows [R | t] per frame, got %s" % (B, tuple(poses.shape)))
            poses = poses.to(dev, non_blocking=True)
        if self.scene is not None and intrinsics is not None and poses is None:
            raise ValueError("predict_frames: a session with scene= needs poses with its intrinsics: camera-frame clouds share no world")
        aug = data.DeviceAugment(train=False, test_size=size, max_size=max_size)
        frame_sizes = [(int(f.shape[0]), int(f.shape[1])) for f in frames]
        net_sizes = [data.resized_shape(w, h, size, max_size) for h, w in frame_sizes]
        if max(max(s) for s in frame_sizes + net_sizes) > 16384:
            raise ValueError("predict_frames: frame and network sizes are limited to 16384 per side")
        sensor = None if sensor_depth is None else self._sensor_plane(sensor_depth, frame_sizes, dev)
        on_dev = [self._upload_frame(f, dev) for f in frames]
        params = [aug.params(w, h) for h, w in frame_sizes]
        if ensemble:                                       # the flip rides in the resize's read; collated behind the originals
            on_dev, params = on_dev * 2, params + [dict(p, flip="h") for p in params]
        no_lines = torch.zeros((0, 4))
        out, table = data.DeviceAugment.apply_batch([(f, None, None) for f in on_dev], [no_lines] * len(on_dev), params,
                                                    carry=np.asarray([frame_sizes, frame_sizes, net_sizes], dtype=np.int32))
        batch = data.device_collate([o[:3] for o in out], device=dev, dtype=self.compute_dtype, pad_to=pad_to)
        fsz, nsz = table[0], table[2]                      # the lines of all 2B images are scaled to their frame's size
        raw, post = self._run(NestedTensor(batch["images"], batch["pad_mask"]), table[:2].view(2 * B, 2) if ensemble else fsz, True,
                              twin=B if ensemble and self.line_nms is not None else 0)
        with torch.no_grad(), self._on_stream():
            depth, mm, labels = ops.dense_postprocess_resized(
                raw["pred_depth"][-1], raw["pred_seg"], nsz, fsz, (max(s[0] for s in frame_sizes), max(s[1] for s in frame_sizes)),
                self.min_depth, self.max_depth, twin=B if ensemble else 0)
            regions = None if self.regions is None else ops.glass_regions(labels, mm, fsz, depth=depth, **self.regions)
            fused = None
            if sensor is not None:
                fused = ops.sensor_fusion(sensor, labels, depth, mm, fsz, regions["region_map"], regions["region_count"],
                                          regions["regions"], **self.fusion)
            profiles = None
            if self.line_profiles is not None:             # the rows: the NMS survivors, or the lines above score_thresh through `order`
                nms = self.line_nms is not None
                profiles = ops.line_profiles(post["nms_lines" if nms else "lines"][:B], post["nms_count" if nms else "count"][:B], labels,
                                             mm, fsz, order=None if nms else post["order"][:B],
                                             region_map=None if regions is None else regions["region_map"], intrinsics=intrinsics,
                                             **self.line_profiles)
        res = {"depth": depth, "depth_mm": mm, "labels": labels, "sizes": fsz, "net_sizes": nsz}
        if regions is not None:
            res.update(regions)
        if profiles is not None:
            res.update(profiles)
        if fused is not None:
            res.update(fused)
        if self.cloud is not None and intrinsics is not None:      # behind fusion and profiles, before render; the frames are read where they lie
            with torch.no_grad(), self._on_stream():
                res.update(self._cloud(on_dev[:B], frame_sizes, res, intrinsics, poses))
                if self.scene_view is not None:            # what the earlier calls said about these frames: before this call's cloud goes in
                    seen = self.scene.view(intrinsics, fsz, poses=poses, plane=tuple(depth.shape[1:]), view_sizes=frame_sizes,
                                           min_depth=self.min_depth, max_depth=self.max_depth, **self.scene_view)
                    res.update({k: seen[src] for k, src in zip(SCENE_VIEW_KEYS, _SCENE_VIEW_SOURCE)})
                if self.scene is not None:                 # behind the cloud, before render; the map is the session's, not the call's
                    self.scene.integrate(res["cloud"], res["cloud_offsets"])
        if self.render is not None:                        # behind everything else, on the same stream; the uploaded frames are read where they are
            with torch.no_grad(), self._on_stream():
                res["canvas"] = self._render(on_dev[:B], res, post, B, fused is not None)
        for k in ("scores", "lines", "order", "count") + (NMS_KEYS if self.line_nms is not None else ()):
            res[k] = post[k][:B].clone() if copy else post[k][:B]
        return res
