"""Host side of ops.point_cloud: views of the 32-byte records, PLY files, and SceneMap - clouds merged into one voxel grid on the device.

A cloud is a (capacity, 32) uint8 tensor: float32 x y z nx ny nz, then uint8 red green blue label region source frame flags
(include/gwdepth.h, gwd_point_cloud).  fields() names the columns without copying; save_ply writes a binary PLY whose vertex element
IS the record, so saving is a header, one copy to the host and one write.  SceneMap owns the device memory of
a voxel map and issues gwd_scene_reset / gwd_scene_integrate / gwd_scene_extract on it; SceneMap.view looks at the map from posed cameras
(gwd_cloud_view, section 33)."""
import numpy as np
import torch

from . import hip

RECORD_BYTES = 32
FLOAT_FIELDS = ("x", "y", "z", "nx", "ny", "nz")
BYTE_FIELDS = ("red", "green", "blue", "label", "region", "source", "frame", "flags")
FLAG_POINT, FLAG_NORMAL, FLAG_PANE_NORMAL, FLAG_COLOUR = 1, 2, 4, 8
FLAG_MERGED = hip.SCENE_FLAG_MERGED                       # a record of SceneMap.extract: one voxel, not one pixel
SCENE_KEYS = ("cloud", "cloud_offsets", "voxel_stats")
RECORD_DTYPE = np.dtype([(n, "<f4") for n in FLOAT_FIELDS] + [(n, "u1") for n in BYTE_FIELDS])
assert RECORD_DTYPE.itemsize == RECORD_BYTES


def _check(cloud):
    if not torch.is_tensor(cloud) or cloud.dtype != torch.uint8 or cloud.dim() != 2 or cloud.shape[1] != RECORD_BYTES:
        raise TypeError("a cloud is a (rows, %d) uint8 tensor" % RECORD_BYTES)
    return cloud


def fields(cloud):
    """Zero-copy views of a cloud's columns: xyz and normal (rows, 3) float32, rgb (rows, 3) uint8, label / region / source / frame /
    flags (rows,) uint8.  Writing to a view writes the cloud."""
    cloud = _check(cloud)
    floats = cloud[:, :24].view(torch.float32)
    out = {"xyz": floats[:, 0:3], "normal": floats[:, 3:6], "rgb": cloud[:, 24:27]}
    for k, name in enumerate(BYTE_FIELDS[3:]):
        out[name] = cloud[:, 27 + k]
    return out


def _header(rows):
    lines = ["ply", "format binary_little_endian 1.0", "comment gw_depth_amd point cloud: flags 1 point, 2 normal, 4 pane normal, 8 colour",
             "element vertex %d" % rows]
    lines += ["property float %s" % n for n in FLOAT_FIELDS] + ["property uchar %s" % n for n in BYTE_FIELDS]
    return ("\n".join(lines + ["end_header"]) + "\n").encode("ascii")


def save_ply(path, cloud, offsets, frame=None):
    """Writes the points of a cloud - all of them, or those of one frame - as a binary_little_endian 1.0 PLY whose vertex element is
    the 32-byte record itself (all eight uchar properties named).  offsets: cloud_offsets.  One copy to the host (which waits for the
    device) and one write; -> the number of vertices."""
    cloud = _check(cloud)
    off = offsets.cpu().tolist() if torch.is_tensor(offsets) else [int(v) for v in offsets]
    B = len(off) - 1
    if B < 1 or any(b < a for a, b in zip(off, off[1:])) or off[0] != 0 or off[-1] > cloud.shape[0]:
        raise ValueError("save_ply: offsets %r are no exclusive prefix within %d rows" % (off, cloud.shape[0]))
    if frame is not None and not 0 <= int(frame) < B:
        raise ValueError("save_ply: frame %r of %d" % (frame, B))
    lo, hi = (0, off[-1]) if frame is None else (off[int(frame)], off[int(frame) + 1])
    body = cloud[lo:hi].contiguous().cpu().numpy()
    with open(path, "wb") as f:
        f.write(_header(hi - lo))
        f.write(body.tobytes())
    return hi - lo


def load_ply(path):
    """Reads a file save_ply wrote -> (rows, 32) uint8 tensor.  Any other PLY layout raises."""
    with open(path, "rb") as f:
        blob = f.read()
    end = blob.find(b"end_header\n")
    if end < 0:
        raise ValueError("load_ply: %s has no PLY header" % path)
    head = blob[:end].decode("ascii").split("\n")
    body = blob[end + len(b"end_header\n"):]
    lines = [ln for ln in head if ln and not ln.startswith("comment")]
    want = _header(0).decode("ascii").split("\n")
    want = [ln for ln in want if ln and not ln.startswith("comment") and ln != "end_header"]
    if len(lines) != len(want) or lines[:2] != want[:2] or lines[3:] != want[3:] or not lines[2].startswith("element vertex "):
        raise ValueError("load_ply: %s is not a point cloud of this package (its vertex element is not the 32-byte record)" % path)
    rows = int(lines[2].split()[2])
    if len(body) != rows * RECORD_BYTES:
        raise ValueError("load_ply: %s holds %d bytes for %d vertices" % (path, len(body), rows))
    return torch.from_numpy(np.frombuffer(body, dtype=np.uint8).reshape(rows, RECORD_BYTES).copy())


def _count(what, name, value, lo, hi):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
        raise TypeError("%s: %s must be an integer, got %r" % (what, name, value))
    if not lo <= int(value) <= hi:
        raise ValueError("%s: %d <= %s <= %d, got %r" % (what, lo, name, hi, value))
    return int(value)


def check_scene_parameters(voxel, max_voxels, origin=(0.0, 0.0, 0.0), slots=None):
    """Host validation of a map's parameters -> (voxel, max_voxels, origin, slots); slots defaults to the smallest power of two
    >= 2 * max_voxels."""
    if isinstance(voxel, bool) or not isinstance(voxel, (int, float, np.integer, np.floating)):
        raise TypeError("SceneMap: voxel must be a number of metres, got %r" % (voxel,))
    if not 0.0 < float(voxel) < float("inf"):
        raise ValueError("SceneMap: voxel must be finite and > 0, got %r" % (voxel,))
    max_voxels = _count("SceneMap", "max_voxels", max_voxels, 1, hip.SCENE_MAX_VOXELS)
    try:
        origin = tuple(float(v) for v in origin)
    except (TypeError, ValueError):
        raise TypeError("SceneMap: origin must be three numbers, got %r" % (origin,))
    if len(origin) != 3 or not all(abs(v) < float("inf") for v in origin):
        raise ValueError("SceneMap: origin must be three finite numbers, got %r" % (origin,))
    if slots is None:
        slots = 2
        while slots < 2 * max_voxels:
            slots *= 2
    slots = _count("SceneMap", "slots", slots, 2, 2 * hip.SCENE_MAX_VOXELS)
    if slots <= max_voxels or slots & (slots - 1):
        raise ValueError("SceneMap: slots must be a power of two > max_voxels = %d, got %d" % (max_voxels, slots))
    return float(voxel), max_voxels, origin, slots


def check_extract_options(min_obs=1, keep="all"):
    """Host validation of SceneMap.extract's options -> them as a dict."""
    min_obs = _count("extract", "min_obs", min_obs, 1, 2 ** 31 - 1)
    if keep not in hip.CLOUD_KEEP:
        raise ValueError("extract: keep must be one of %s, got %r" % (", ".join(repr(k) for k in hip.CLOUD_KEEP), keep))
    return dict(min_obs=min_obs, keep=keep)


def check_integrate_operands(cloud, cloud_offsets, device=None):
    """Host validation of what SceneMap.integrate takes; device: the map's, when there is one already."""
    _check(cloud)
    if not torch.is_tensor(cloud_offsets) or cloud_offsets.dtype != torch.int32:
        raise TypeError("integrate: cloud_offsets must be an int32 tensor (point_cloud's, on the device)")
    if cloud_offsets.dim() != 1 or cloud_offsets.numel() < 2:
        raise ValueError("integrate: cloud_offsets must be (B + 1,), got %s" % (tuple(cloud_offsets.shape),))
    if cloud_offsets.device != cloud.device or (device is not None and cloud.device != device):
        raise ValueError("integrate: the cloud lives on %s, its offsets on %s, the map on %s" % (cloud.device, cloud_offsets.device, device or cloud.device))
    if cloud.shape[0] > 2 ** 31 - 1:
        raise ValueError("integrate: at most 2^31 - 1 rows per call, got %d" % cloud.shape[0])


class SceneMap:
    """A persistent voxel map on the device (tests/scene_ref.py is the statement).

    m = SceneMap(voxel=0.05, max_voxels=1 << 20, origin=(0, 0, 0), slots=None, device="cuda")
    m.integrate(cloud, cloud_offsets)    the records of ops.point_cloud / predict_frames(poses=...) - world coordinates - or of another
                                         extraction, added to the voxels they fall into; five launches, no host sync; returns m.
    m.extract(min_obs=1, keep="all")     -> dict in SCENE_KEYS order, fresh tensors: cloud (max_voxels, 32) uint8 - one merged record
                                         per kept voxel (mean position, normalised mean normal, mean colour, majority label with
                                         ties to glass, flags 1 | FLAG_MERGED | normal | colour) in the order the voxels were first
                                         seen, zeros behind them - cloud_offsets (2,) int32 = [0, kept], voxel_stats (max_voxels, 4)
                                         int32 = n, n_glass, first_seen, last_seen; fields / save_ply / load_ply take the cloud as it
                                         is.  Three launches, no host sync; the map is unchanged.
    m.view(intrinsics, sizes, poses=None, plane=None, min_obs=1, keep="all", footprint=None, **options)
                                         the map seen from posed cameras: extract(min_obs, keep), then
                                         ops.cloud_view of the extraction - footprint=None: the map's voxel; options: min_depth,
                                         max_depth, max_splat - -> ops.VIEW_KEYS (view_depth, view_labels, view_index, view_rgb at
                                         frame size) + SCENE_KEYS, so view_index leads into voxel_stats.  Six launches, no host
                                         sync; the map is unchanged; an overflowed map gives empty planes, never a partial picture.
    m.reset()                            an empty map again; one launch.
    m.state()                            ONE copy to the host (waits for the device; off the path): dict of serial, count, points,
                                         dropped, status.
    m.check()                            raises RuntimeError when status != 0: a call would have brought count above max_voxels; the
                                         contents are undefined until reset() and extract returns an empty cloud, never a truncated one.
    Integrating A and then B gives the voxels, the order and the bytes of integrating A || B at once (first_seen / last_seen apart);
    results are bit-identical from run to run.  At most 2^31 - 1 observations per voxel and 2^31 - 1 calls between resets.
    Memory: 128 bytes per voxel + 20 per slot."""

    def __init__(self, voxel, max_voxels, origin=(0.0, 0.0, 0.0), slots=None, device="cuda"):
        self.voxel, self.max_voxels, self.origin, self.slots = check_scene_parameters(voxel, max_voxels, origin, slots)
        self.device = torch.device(device)
        new = lambda shape, dt: torch.empty(shape, dtype=dt, device=self.device)
        self._tensors = (new((self.slots,), torch.int64), new((self.slots,), torch.int64), new((self.slots,), torch.int32),
                         new((self.max_voxels, hip.SCENE_VOXEL_BYTES), torch.uint8), new((8,), torch.int64))
        self.device = self._tensors[0].device              # with its index, as a tensor reports it
        self._desc = hip.HipLibrary.scene_desc(*self._tensors, self.voxel, self.origin)
        self._one_row = torch.zeros((1, RECORD_BYTES), dtype=torch.uint8, device=self.device)       # stands in for a cloud of no rows
        self._ws = None
        self.reset()

    def _workspace(self, rows):
        need = hip.library().workspace_bytes(hip.WS_SCENE, rows, self.max_voxels)
        if self._ws is None or self._ws.numel() < need:    # grows with the largest cloud seen; reused in stream order
            self._ws = torch.empty((need,), dtype=torch.uint8, device=self.device)
        return self._ws

    def reset(self):
        hip.library().scene_reset(self._desc, self._tensors)
        return self

    def integrate(self, cloud, cloud_offsets):
        check_integrate_operands(cloud, cloud_offsets, self.device)
        cloud = self._one_row if cloud.shape[0] == 0 else cloud.contiguous()      # no rows: the total is clamped to what is there
        hip.library().scene_integrate(self._desc, self._tensors, cloud, cloud_offsets.contiguous(), self._workspace(cloud.shape[0]))
        return self

    def extract(self, min_obs=1, keep="all"):
        opt = check_extract_options(min_obs, keep)
        new = lambda shape, dt: torch.empty(shape, dtype=dt, device=self.device)
        res = {"cloud": new((self.max_voxels, RECORD_BYTES), torch.uint8), "cloud_offsets": new((2,), torch.int32),
               "voxel_stats": new((self.max_voxels, 4), torch.int32)}
        hip.library().scene_extract(self._desc, self._tensors, opt["min_obs"], opt["keep"], self._workspace(1), res["cloud"],
                                    res["cloud_offsets"], res["voxel_stats"])
        return res

    def view(self, intrinsics, sizes, poses=None, plane=None, min_obs=1, keep="all", footprint=None, view_sizes=None, **options):
        from . import ops
        if set(options) - {"min_depth", "max_depth", "max_splat"}:
            raise TypeError("view: unknown option(s) %s (known: min_depth, max_depth, max_splat)" % sorted(set(options) - {"min_depth", "max_depth", "max_splat"}))
        check_extract_options(min_obs, keep)
        opt = ops.check_view_options(footprint=self.voxel if footprint is None else footprint, **options)      # before anything is launched
        ext = self.extract(min_obs, keep)
        res = ops.cloud_view(ext["cloud"], ext["cloud_offsets"], intrinsics, sizes, poses=poses, plane=plane, view_sizes=view_sizes, **opt)
        res.update(ext)
        return res

    def state(self):
        host = self._tensors[4].cpu().tolist()
        return dict(zip(hip.SCENE_STATE, host))

    def check(self):
        st = self.state()
        if st["status"] != 0:
            raise RuntimeError("SceneMap: more than max_voxels = %d voxels (status %d after %d calls): the contents are undefined until "
                               "reset()" % (self.max_voxels, st["status"], st["serial"]))
        return st

    def save_ply(self, path, **extract_options):
        """extract(**extract_options) written as a PLY (save_ply); -> the number of vertices."""
        res = self.extract(**extract_options)
        return save_ply(path, res["cloud"], res["cloud_offsets"])
