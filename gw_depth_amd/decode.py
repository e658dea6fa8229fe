"""Host half of the input pipeline: a GW-Depth directory on disk -> decoded planes in shared memory, by a pool of worker processes.

The reference opens three PNGs and one JSON per sample inside a torch DataLoader worker (src/datasets/glassrgbd_norhint.py:213-302).
Here the files are decoded by fresh interpreters that load neither torch nor the GPU runtime; each writes the planes of a sample as
ONE record (plane_layout) into a shared-memory slot, from which gw_depth_amd/dataset.py copies it to a pinned slab or to the resident
store.  This module imports json, os, numpy and PIL only - never torch.

    python -m gw_depth_amd.decode --worker          (started by DecodePool; requests on stdin, replies on stdout, one JSON per line)
"""
import atexit
import collections
import contextlib
import json
import os
import selectors
import subprocess
import sys
import time
from multiprocessing import shared_memory

import numpy as np
from PIL import Image

ALIGN = 256            # every plane of a record starts at a multiple of this: a view of it is aligned like a torch allocation
MAX_WORKERS = 16


class GlassRGBDIndex:
    """The file layout of DataLoadPreprocess (glassrgbd_norhint.py:216-251): sample names from the first token of every non-blank
    line of `filenames_file`; <data_path>/<name>.png, <gt_depth_path>/<name>.png, <gt_seg_path>/<name>.png, <gt_line_path>/<name>.json."""

    def __init__(self, data_path, gt_depth_path, gt_seg_path, gt_line_path, filenames_file, images_json=None):
        self.data_path, self.gt_depth_path, self.gt_seg_path = data_path, gt_depth_path, gt_seg_path
        self.gt_line_path = os.path.realpath(gt_line_path)                               # :242
        with open(filenames_file, "r") as f:
            self.names = [ln.split()[0] for ln in f if ln.strip()]
        self.id_to_img = {}
        if images_json is not None:                                                       # :230-233
            with open(images_json, "r") as f:
                for d in json.load(f)["images"]:
                    self.id_to_img[d["id"]] = d["file_name"].split(".")[0]
        self._sizes = {}

    @classmethod
    def from_args(cls, args, mode):
        """The reference's argument names; mode 'train' reads args.filenames_file_train, 'val' args.filenames_file_eval."""
        if mode not in ("train", "val"):
            raise ValueError("mode must be 'train' or 'val', got %r" % (mode,))
        return cls(args.data_path, args.gt_depth_path, args.gt_seg_path, args.gt_line_path,
                   args.filenames_file_train if mode == "train" else args.filenames_file_eval,
                   getattr(args, "glassrgbd_images_json", None))

    def __len__(self):
        return len(self.names)

    def name(self, i):
        return self.names[i]

    def paths(self, i):
        """(image, depth, segmentation, lines JSON) of sample i."""
        n = self.names[i]
        return (os.path.join(self.data_path, n + ".png"), os.path.join(self.gt_depth_path, n + ".png"),
                os.path.join(self.gt_seg_path, n + ".png"), os.path.join(self.gt_line_path, n + ".json"))

    def size(self, i):
        """(h, w) of sample i from the image's PNG header (nothing is decoded); cached."""
        s = self._sizes.get(i)
        if s is None:
            with Image.open(self.paths(i)[0]) as im:
                s = self._sizes[i] = (im.size[1], im.size[0])
        return s


def plane_layout(h, w):
    """(offset_rgb, offset_depth, offset_labels, total_bytes) of one sample's record: rgb u8 (h,w,3), depth u16 little-endian (h,w),
    labels u8 (h,w) back to back, each plane at the next multiple of ALIGN bytes."""
    h, w = int(h), int(w)
    if h <= 0 or w <= 0:
        raise ValueError("plane_layout: a positive frame size expected, got %r x %r" % (h, w))
    up = lambda n: -(-n // ALIGN) * ALIGN
    off_d = up(h * w * 3)
    off_l = up(off_d + h * w * 2)
    return 0, off_d, off_l, off_l + h * w


def _decode_files(paths, timings=None):
    """The three planes and the JSON of one sample, with the mode / size checks of decode_item."""
    clock = time.perf_counter
    t0 = clock()
    with Image.open(paths[0]) as im:
        if im.mode != "RGB":
            raise ValueError("%s: image mode %s, RGB expected" % (paths[0], im.mode))
        rgb = np.asarray(im)
    t1 = clock()
    with Image.open(paths[1]) as im:
        if im.mode == "I;16":
            depth = np.asarray(im)
        elif im.mode == "I":
            depth = np.asarray(im)
            if depth.size and (int(depth.min()) < 0 or int(depth.max()) >= 65536):
                raise ValueError("%s: depth values outside 16 bits" % paths[1])
        else:
            raise ValueError("%s: depth mode %s, I;16 expected" % (paths[1], im.mode))
        depth = depth.astype("<u2", copy=False)
    t2 = clock()
    with Image.open(paths[2]) as im:
        if im.mode not in ("L", "P"):
            raise ValueError("%s: label mode %s, L or P expected" % (paths[2], im.mode))
        labels = np.asarray(im)                                # mode P: the stored palette index
    t3 = clock()
    for p, a in ((paths[1], depth), (paths[2], labels)):
        if a.shape != rgb.shape[:2]:
            raise ValueError("%s: size %s differs from the image's %s" % (p, a.shape, rgb.shape[:2]))
    with open(paths[3], "r") as f:
        doc = json.load(f)
    t4 = clock()
    if timings is not None:
        timings.update(image=t1 - t0, depth=t2 - t1, labels=t3 - t2, json=t4 - t3)
    return rgb, depth, labels, doc["shapes"], doc["imageId"]


def decode_item(index, i):
    """(rgb uint8 (h,w,3), depth_mm uint16 (h,w), labels uint8 (h,w), shapes, image_id, name) of sample i: what
    DataLoadPreprocess.__getitem__ reads before its transforms.  ValueError naming the file for any mode but RGB / I;16 (or I within
    16 bits) / L or P, and for planes of different sizes."""
    return _decode_files(index.paths(i)) + (index.name(i),)


def record_views(buf, h, w):
    """(rgb, depth, labels) numpy views of a record laid out by plane_layout in `buf`."""
    o_r, o_d, o_l, _ = plane_layout(h, w)
    return (np.frombuffer(buf, np.uint8, h * w * 3, o_r).reshape(h, w, 3), np.frombuffer(buf, "<u2", h * w, o_d).reshape(h, w),
            np.frombuffer(buf, np.uint8, h * w, o_l).reshape(h, w))


def default_workers():
    return max(1, min(MAX_WORKERS, len(os.sched_getaffinity(0))) - 1)


Decoded = collections.namedtuple("Decoded", "rgb depth_mm labels shapes image_id name index record timings")
Decoded.__doc__ = """One pool result: decode_item's values (the arrays are VIEWS of a shared-memory slot, valid until the pool's next
next() / close()), the sample index, the record's bytes (plane_layout) and the worker's decode times in seconds."""


@contextlib.contextmanager
def _untracked():
    """multiprocessing's resource tracker is a helper PROCESS that adopts every block it hears of.  The pool owns its blocks - it
    unlinks them in close() - and a worker only borrows them, so neither side tells the tracker (Python >= 3.13 has `track=False`)."""
    from multiprocessing import resource_tracker
    real = resource_tracker.register
    resource_tracker.register = lambda *a, **k: None
    try:
        yield
    finally:
        resource_tracker.register = real


class _Block(shared_memory.SharedMemory):
    """A slot's block, created and unlinked by the pool alone."""

    def __init__(self, size):
        with _untracked():
            super().__init__(create=True, size=size)

    def unlink(self):
        try:
            os.unlink(os.path.join("/dev/shm", self.name.lstrip("/")))
        except FileNotFoundError:
            pass

    def __del__(self):                                         # a caller may still hold arrays over it: the mapping lives as long as they do
        try:
            super().__del__()
        except BufferError:
            pass


class DecodePool:
    """Decodes samples of `index` in `workers` fresh interpreters (no fork: the parent's modules, torch among them, never load in a
    worker; workers never open the GPU).  submit(i) queues a sample, next() returns the results in SUBMISSION order; at most `slots`
    samples are in flight (submitted and not yet handed back by a following next()), each in a shared-memory slot sized for its frame.
    Build the pool before the GPU is initialised: construction refuses once torch.cuda.is_initialized()."""

    def __init__(self, index, workers=None, slots=None, timeout=120.0):
        torch = sys.modules.get("torch")
        if torch is not None and torch.cuda.is_initialized():
            raise RuntimeError("DecodePool: the GPU is already initialised in this process; build the pool first and the model after")
        self.index = index
        self.workers = default_workers() if workers is None else max(1, min(MAX_WORKERS, int(workers)))
        self.n_slots = max(2 * self.workers, 2) if slots is None else max(1, int(slots))
        self.timeout = float(timeout)
        self._slots = [None] * self.n_slots                    # SharedMemory per slot, created / grown on demand
        self._free = list(range(self.n_slots))
        self._held = None                                      # slot of the result the caller is looking at
        self._seq_in = self._seq_out = 0
        self._pending = {}                                     # seq -> (i, slot, worker | None)
        self._done = {}                                        # seq -> reply
        self._procs, self._bufs, self._load = [], [], []
        self._sel = selectors.DefaultSelector()
        self.handshakes = []
        self._closed = False
        atexit.register(self.close)
        env = dict(os.environ)
        pkg_parent = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        env["PYTHONPATH"] = pkg_parent + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
        try:
            for k in range(self.workers):
                p = subprocess.Popen([sys.executable, "-m", "gw_depth_amd.decode", "--worker"], stdin=subprocess.PIPE,
                                     stdout=subprocess.PIPE, env=env, close_fds=True)
                os.set_blocking(p.stdout.fileno(), False)
                self._procs.append(p)
                self._bufs.append(b"")
                self._load.append(0)
                self._sel.register(p.stdout, selectors.EVENT_READ, k)
            deadline = time.monotonic() + self.timeout
            self.handshakes = [None] * self.workers
            while any(h is None for h in self.handshakes):
                for k, msg in self._poll(deadline, "the workers' start"):
                    if "ready" not in msg:
                        raise RuntimeError("DecodePool: worker %d answered %r instead of its handshake" % (k, msg))
                    self.handshakes[k] = msg
        except BaseException:
            self.close()
            raise

    # ---------------------------------------------------------------------------------------------------------------- plumbing
    def _poll(self, deadline, what):
        """Waits (up to the deadline) for output of any worker; returns the complete replies [(worker, dict)].  A worker that has
        exited raises instead of being waited for."""
        left = deadline - time.monotonic()
        if left <= 0:
            raise RuntimeError("DecodePool: timed out after %.0f s waiting for %s" % (self.timeout, what))
        out = []
        for key, _ in self._sel.select(min(left, 1.0)):
            k = key.data
            try:
                chunk = os.read(key.fileobj.fileno(), 1 << 16)
            except BlockingIOError:
                continue
            if not chunk:
                self._sel.unregister(key.fileobj)
                raise RuntimeError("DecodePool: worker %d (pid %d) closed its pipe (exit status %r) while %s was awaited"
                                   % (k, self._procs[k].pid, self._procs[k].poll(), what))
            self._bufs[k] += chunk
            *lines, self._bufs[k] = self._bufs[k].split(b"\n")
            out += [(k, json.loads(ln)) for ln in lines if ln.strip()]
        for k, p in enumerate(self._procs):
            if p.poll() is not None and (self._load[k] or self.handshakes[k] is None) and not any(w == k for w, _ in out):
                raise RuntimeError("DecodePool: worker %d (pid %d) died with exit status %r while %s was awaited" % (k, p.pid, p.returncode, what))
        return out

    def _slot_for(self, slot, nbytes):
        shm = self._slots[slot]
        if shm is None or shm.size < nbytes:
            if shm is not None:
                try:
                    shm.close()
                except BufferError:                            # a stale Decoded still looks at it
                    pass
                shm.unlink()
            shm = self._slots[slot] = _Block(nbytes)
        return shm

    @property
    def free_slots(self):
        return len(self._free)

    @property
    def in_flight(self):
        return self.n_slots - len(self._free)

    def shm_names(self):
        return [s.name for s in self._slots if s is not None]

    def pids(self):
        return [p.pid for p in self._procs]

    # ---------------------------------------------------------------------------------------------------------------- requests
    def submit(self, i):
        """Queues sample i.  RuntimeError when `slots` samples are in flight already."""
        if self._closed:
            raise RuntimeError("DecodePool is closed")
        if not self._free:
            raise RuntimeError("DecodePool: %d samples in flight already (slots=%d); take one with next() first" % (self.in_flight, self.n_slots))
        i = int(i)
        seq = self._seq_in
        slot = self._free.pop()
        try:
            h, w = self.index.size(i)
            shm = self._slot_for(slot, plane_layout(h, w)[3])
        except Exception as e:                                 # an unreadable header is this sample's failure, reported in order
            self._pending[seq] = (i, slot, None)
            self._done[seq] = {"seq": seq, "ok": False, "error": "%s: %s" % (type(e).__name__, e)}
            self._seq_in += 1
            return
        k = min(range(self.workers), key=lambda n: (self._load[n], (n - seq) % self.workers))
        req = {"seq": seq, "paths": self.index.paths(i), "slot": slot, "shm": shm.name, "size": shm.size}
        try:
            self._procs[k].stdin.write((json.dumps(req) + "\n").encode())
            self._procs[k].stdin.flush()
        except (BrokenPipeError, OSError) as e:
            self._free.append(slot)
            raise RuntimeError("DecodePool: worker %d (pid %d) is gone (%s) at sample %r" % (k, self._procs[k].pid, e, self.index.name(i)))
        self._load[k] += 1
        self._pending[seq] = (i, slot, k)
        self._seq_in += 1

    def release(self):
        """Gives back the slot of the result next() returned last (next() and close() do it themselves)."""
        if self._held is not None:
            self._free.append(self._held)
            self._held = None

    def next(self):
        """The oldest submitted sample's result (a Decoded), whatever order the workers finished in.  A sample that failed to decode
        raises RuntimeError naming it; a dead worker or a wait beyond `timeout` seconds raises too."""
        self.release()
        if self._seq_out == self._seq_in:
            raise RuntimeError("DecodePool.next(): nothing submitted")
        seq = self._seq_out
        i, slot, _ = self._pending[seq]
        name = self.index.name(i)
        deadline = time.monotonic() + self.timeout
        while seq not in self._done:
            for k, msg in self._poll(deadline, "sample %r" % name):
                self._load[k] -= 1
                self._done[msg["seq"]] = msg
        msg = self._done.pop(seq)
        del self._pending[seq]
        self._seq_out += 1
        if not msg["ok"]:
            self._free.append(slot)
            raise RuntimeError("DecodePool: sample %r failed to decode: %s" % (name, msg["error"]))
        self._held = slot
        h, w = msg["h"], msg["w"]
        total = plane_layout(h, w)[3]
        buf = self._slots[slot].buf
        rgb, depth, labels = record_views(buf, h, w)
        return Decoded(rgb, depth, labels, msg["shapes"], msg["image_id"], name, i, np.frombuffer(buf, np.uint8, total), msg.get("t", {}))

    def map(self, indices):
        """Decoded results of `indices` in order, keeping the pool as full as `slots` allows.  Each result's arrays are valid until
        the generator is advanced."""
        indices = [int(i) for i in indices]
        sent = 0
        for _ in indices:
            while sent < len(indices) and self._free:
                self.submit(indices[sent])
                sent += 1
            if self._seq_out == self._seq_in:                  # one slot, and the caller still holds it
                self.release()
                self.submit(indices[sent])
                sent += 1
            yield self.next()

    # ---------------------------------------------------------------------------------------------------------------- shutdown
    def close(self):
        """Stops the workers (closing their stdin ends their loop; one that does not leave in time is killed) and unlinks every
        shared-memory block."""
        if self._closed:
            return
        self._closed = True
        atexit.unregister(self.close)
        for p in self._procs:
            try:
                p.stdin.close()
            except OSError:
                pass
        for p in self._procs:
            try:
                p.wait(timeout=5.0)
            except subprocess.TimeoutExpired:
                p.kill()
                p.wait(timeout=5.0)
            try:
                self._sel.unregister(p.stdout)
            except (KeyError, ValueError):
                pass
            p.stdout.close()
        self._sel.close()
        self._held = None
        for k, shm in enumerate(self._slots):
            if shm is not None:
                try:
                    shm.close()
                except BufferError:                            # a caller still holds a view: the block is unlinked all the same
                    pass
                shm.unlink()
                self._slots[k] = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---------------------------------------------------------------------------------------------------------------------- worker side
def _attach(name):
    """The parent's block, borrowed."""
    with _untracked():
        return shared_memory.SharedMemory(name=name)


def _worker_main():
    out = sys.stdout.buffer
    out.write((json.dumps({"ready": True, "pid": os.getpid(), "torch_loaded": "torch" in sys.modules}) + "\n").encode())
    out.flush()
    blocks = {}
    for line in sys.stdin.buffer:
        if not line.strip():
            continue
        req = json.loads(line)
        reply = {"seq": req["seq"]}
        try:
            t = {}
            rgb, depth, labels, shapes, image_id = _decode_files(req["paths"], t)
            h, w = rgb.shape[:2]
            if plane_layout(h, w)[3] > req["size"]:
                raise ValueError("%s: frame %d x %d does not fit the %d-byte slot sized from its header" % (req["paths"][0], h, w, req["size"]))
            name, shm = blocks.get(req["slot"], (None, None))
            if name != req["shm"]:                             # the slot's first request, or the parent replaced a block that was too small
                if shm is not None:
                    shm.close()
                shm = _attach(req["shm"])
                blocks[req["slot"]] = (req["shm"], shm)
            t0 = time.perf_counter()
            v_rgb, v_depth, v_labels = record_views(shm.buf, h, w)
            v_rgb[...] = rgb
            v_depth[...] = depth
            v_labels[...] = labels
            del v_rgb, v_depth, v_labels
            t["copy"] = time.perf_counter() - t0
            reply.update(ok=True, h=h, w=w, shapes=shapes, image_id=image_id, t=t)
        except Exception as e:
            reply.update(ok=False, error="%s: %s" % (type(e).__name__, e))
        out.write((json.dumps(reply) + "\n").encode())
        out.flush()
    for _, shm in blocks.values():
        try:
            shm.close()
        except BufferError:
            pass


if __name__ == "__main__":
    if "--worker" in sys.argv[1:]:
        _worker_main()
    else:
        sys.exit("usage: python -m gw_depth_amd.decode --worker   (started by DecodePool)")
