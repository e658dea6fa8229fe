"""Host side of ops.point_cloud: views of the 32-byte records and PLY files.

A cloud is a (capacity, 32) uint8 tensor: float32 x y z nx ny nz, then uint8 red green blue label region source frame flags
(include/gwdepth.h, gwd_point_cloud).  fields() names the columns without copying; save_ply writes a binary PLY whose vertex element
IS the record, so saving is a header, one copy to the host and one write."""
import numpy as np
import torch

RECORD_BYTES = 32
FLOAT_FIELDS = ("x", "y", "z", "nx", "ny", "nz")
BYTE_FIELDS = ("red", "green", "blue", "label", "region", "source", "frame", "flags")
FLAG_POINT, FLAG_NORMAL, FLAG_PANE_NORMAL, FLAG_COLOUR = 1, 2, 4, 8
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
