"""The statement of the scene map (csrc/scene.hip, gw_depth_amd.cloud.SceneMap) in numpy: a plain dictionary
loop, fp64 with every operation rounded on its own and in the order written here, integers everywhere else.  The kernels, the stand-in
library (tests/scene_fake.py) and the fixture tests/golden/scene_map.npz are held to this file."""
import numpy as np

from tests.cloud_ref import HAS_COLOUR, HAS_NORMAL, KEEP, POINT, RECORD

MERGED = 16
INDEX_BIAS = 1 << 20                                      # a voxel index is -2^20 .. 2^20 - 1
MAX_VOXELS = 1 << 27
STATE_KEYS = ("serial", "count", "points", "dropped", "status")


def quantise(p, origin, voxel):
    """One axis of one point: (voxel index, sub-voxel offset in 1/65536), or None when the index is out of range."""
    with np.errstate(all="ignore"):
        t = (np.float64(p) - np.float64(origin)) / np.float64(voxel)
        i = np.floor(t)
        if not -INDEX_BIAS <= i < INDEX_BIAS:             # NaN and Inf fail both comparisons
            return None
        return int(i), int(np.floor((t - i) * np.float64(65536.0)))


def key_of(index):
    return (index[0] + INDEX_BIAS) | (index[1] + INDEX_BIAS) << 21 | (index[2] + INDEX_BIAS) << 42


class Voxel:
    def __init__(self, index, serial):
        self.index = index
        self.n = self.n_normal = self.n_colour = self.n_glass = 0
        self.sum_q, self.sum_n, self.sum_rgb = [0, 0, 0], [0, 0, 0], [0, 0, 0]
        self.first_seen = self.last_seen = serial


class SceneMap:
    """voxels: key -> Voxel; a dict keeps the order of insertion, which is the order of birth."""

    def __init__(self, voxel, max_voxels, origin=(0.0, 0.0, 0.0)):
        self.voxel, self.origin, self.max_voxels = float(voxel), tuple(float(v) for v in origin), int(max_voxels)
        assert np.isfinite(self.voxel) and self.voxel > 0.0 and np.isfinite(self.origin).all() and 1 <= self.max_voxels <= MAX_VOXELS
        self.reset()

    def reset(self):
        self.voxels = {}
        self.serial = self.points = self.dropped = self.status = 0

    def state(self):
        return dict(serial=self.serial, count=len(self.voxels), points=self.points, dropped=self.dropped, status=self.status)

    def integrate(self, cloud, cloud_offsets):
        """cloud: (rows, 32) uint8, cloud_offsets: int32, only its last entry is used."""
        serial, self.serial = self.serial, self.serial + 1
        if self.status != 0:
            return self
        rows = np.ascontiguousarray(cloud).view(RECORD).ravel()
        total = min(max(int(cloud_offsets[-1]), 0), len(rows))
        taken = []                                        # (row, its three (index, offset) pairs)
        for r in range(total):
            row, at = rows[r], None
            if int(row["flags"]) & POINT and np.isfinite(row["xyz"]).all():
                at = [quantise(row["xyz"][k], self.origin[k], self.voxel) for k in range(3)]
            if at is not None and None not in at:
                taken.append((row, at))
        born = {key_of([i for i, _ in at]) for _, at in taken} - set(self.voxels)
        if len(self.voxels) + len(born) > self.max_voxels:
            self.status = 1                               # nothing else changes; the contents are undefined until reset()
            return self
        self.points, self.dropped = self.points + len(taken), self.dropped + total - len(taken)
        for row, at in taken:
            index = tuple(i for i, _ in at)
            v = self.voxels.get(key_of(index))
            if v is None:
                v = self.voxels[key_of(index)] = Voxel(index, serial)
            v.n += 1
            v.first_seen, v.last_seen = min(v.first_seen, serial), max(v.last_seen, serial)
            for k in range(3):
                v.sum_q[k] += at[k][1]
            normal = row["normal"]
            with np.errstate(invalid="ignore"):
                bounded = bool((np.abs(normal) <= np.float32(2.0)).all())      # a unit normal's are <= 1; bounds the sums, NaN fails
            if int(row["flags"]) & HAS_NORMAL and bounded:
                v.n_normal += 1
                for k in range(3):
                    v.sum_n[k] += int(np.rint(np.float64(normal[k]) * np.float64(32767.0)))
            if int(row["flags"]) & HAS_COLOUR:
                v.n_colour += 1
                for k in range(3):
                    v.sum_rgb[k] += int(row["rgb"][k])
            if int(row["label"]) == 1:
                v.n_glass += 1
        return self

    def extract(self, min_obs=1, keep="all"):
        """-> dict(cloud (max_voxels, 32) uint8, cloud_offsets (2,) int32, voxel_stats (max_voxels, 4) int32)."""
        assert keep in KEEP and min_obs >= 1
        cloud = np.zeros(self.max_voxels, dtype=RECORD)
        stats = np.zeros((self.max_voxels, 4), dtype=np.int32)
        kept = 0
        for v in (self.voxels.values() if self.status == 0 else ()):
            label = 1 if 2 * v.n_glass >= v.n else 0
            if v.n < min_obs or (keep == "glass" and label != 1) or (keep == "non_glass" and label == 1):
                continue
            rec = cloud[kept]
            flags = POINT | MERGED
            for k in range(3):
                mean = np.float64(v.sum_q[k]) / np.float64(v.n) + np.float64(0.5)
                rec["xyz"][k] = np.float32(((np.float64(v.index[k]) + mean / np.float64(65536.0)) * np.float64(self.voxel))
                                           + np.float64(self.origin[k]))
            if v.n_normal > 0 and any(v.sum_n):
                s = [np.float64(c) for c in v.sum_n]
                length = np.sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2])
                for k in range(3):
                    rec["normal"][k] = np.float32(s[k] / length)
                flags |= HAS_NORMAL
            if v.n_colour > 0:
                for k in range(3):
                    rec["rgb"][k] = (2 * v.sum_rgb[k] + v.n_colour) // (2 * v.n_colour)
                flags |= HAS_COLOUR
            rec["label"], rec["flags"] = label, flags
            stats[kept] = (v.n, v.n_glass, v.first_seen, v.last_seen)
            kept += 1
        return {"cloud": cloud.view(np.uint8).reshape(self.max_voxels, 32), "cloud_offsets": np.array([0, kept], dtype=np.int32),
                "voxel_stats": stats}


def merge(clouds, voxel, max_voxels, origin=(0.0, 0.0, 0.0), min_obs=1, keep="all"):
    """The one-shot form: clouds = [(cloud, cloud_offsets), ...] integrated in order into a fresh map -> its extraction."""
    m = SceneMap(voxel, max_voxels, origin)
    for cloud, offsets in clouds:
        m.integrate(cloud, offsets)
    return m.extract(min_obs, keep)
