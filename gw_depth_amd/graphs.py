"""Captured HIP graphs: which signatures hold one (GraphCache) and how a pass becomes one (GraphSide).

engine.TrainStep replays its forward/backward as a chain of graphs cut at bucket boundaries, infer.InferenceSession its forward and
post-processing as a chain of one.  Both go through the same protocol, written here once: static inputs, one warm-up pass, a second
pass audited for hipMemsetAsync, a refusal that carries its reason, the capture on one private stream out of one memory pool, a
least-recently-used bound on the captured signatures, and the stream hand-over around everything that runs in graph mode."""
import contextlib
import gc
import warnings
from collections import OrderedDict

import torch

MAX_GRAPHS = 6          # captured batch signatures kept (least recently used goes first); all share one memory pool


class GraphCache:
    """Which batch signatures of a graph-mode TrainStep hold a captured step: pure bookkeeping, no device.

    `entries` is the least-recently-used ordered table of the signatures that have been through a capture attempt (captured, or
    refused: {"graph": None, ...}); `seen` counts the sights of the signatures still waiting.  A signature is captured at its `capture_after`-th
    sight and runs eagerly before that, so a shape that shows up once in an epoch never pays the warm-up passes of a capture.  The
    bound is `max_graphs`, or the module's MAX_GRAPHS read at every call when it is None."""
    COUNTERS = ("replays", "captures", "eager_steps", "evictions", "refused", "host_matcher_steps")
    SEEN_MAX = 4096         # waiting signatures remembered

    def __init__(self, max_graphs=None, capture_after=1):
        if max_graphs is not None and int(max_graphs) < 1:
            raise ValueError("max_graphs must be >= 1, got %r" % (max_graphs,))
        if int(capture_after) < 1:
            raise ValueError("capture_after must be >= 1, got %r" % (capture_after,))
        self.max_graphs = None if max_graphs is None else int(max_graphs)
        self.capture_after = int(capture_after)
        self.entries = OrderedDict()
        self.seen = {}
        self.stats = dict.fromkeys(self.COUNTERS, 0)

    def bound(self):
        return MAX_GRAPHS if self.max_graphs is None else self.max_graphs

    def lookup(self, key):
        """One sight of `key` -> ("known", entry): it has been through a capture attempt (entry["graph"] is None if that was refused)
        and is the most recently used now; ("wait", None): run it eagerly; ("capture", None): capture it now and store() the entry."""
        ent = self.entries.get(key)
        if ent is not None:
            self.entries.move_to_end(key)
            return "known", ent
        n = self.seen.pop(key, 0) + 1                  # re-inserted at the young end
        if n >= self.capture_after:
            return "capture", None                     # its count is dropped: an evicted signature starts over
        self.seen[key] = n
        while len(self.seen) > self.SEEN_MAX:          # waiting signatures are bounded too: the one not seen for longest goes
            del self.seen[next(iter(self.seen))]
        return "wait", None

    def make_room(self):
        """Drop least recently used entries until one more fits; called BEFORE a capture, so the executables go first."""
        while len(self.entries) >= max(self.bound(), 1):
            self.entries.popitem(last=False)
            self.stats["evictions"] += 1

    def store(self, key, ent):
        self.make_room()
        self.entries[key] = ent
        self.stats["captures" if ent.get("graph") is not None else "refused"] += 1
        return ent

    def count(self, name, n=1):
        self.stats[name] += n


def count_memsets(fn):
    """Run fn() under the profiler and count the hipMemsetAsync runtime calls it makes (memset nodes do not replay correctly in HIP
    graphs on this ROCm).  -1: no tracer on this host - without the audit there is no capture; fn() has still run once."""
    from torch.profiler import ProfilerActivity, profile
    try:
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.name == "hipMemsetAsync")
    except Exception as exc:
        warnings.warn("gw_depth_amd: capture audit unavailable (%s)" % exc)
        fn()
        return -1


def refusal(memsets, caught=(), noun="step"):
    """Why a warmed-up pass must not be captured, or None.  memsets: what count_memsets() returned; caught: the warnings recorded
    during the warm-up (empty for a caller that records none, so the first rule is the train step's alone); noun: what the pass is
    called in the text ("step", "forward").  The first rule that holds gives the reason."""
    if any("AccumulateGrad node's stream does not match" in str(w.message) for w in caught):
        return ("an autograd graph built on another stream is still alive (e.g. the outputs of an eager step): its "
                "AccumulateGrad nodes would be captured on a forked stream")
    if memsets < 0:
        return "the capture audit (torch.profiler runtime-call trace) is not available on this host"
    if memsets:
        return ("%d hipMemsetAsync call(s) in the %s (ATen multi-block reductions zero their semaphores that way); "
                "memset nodes do not replay correctly in HIP graphs on this ROCm" % (memsets, noun))
    return None


@contextlib.contextmanager
def _recorded(on):
    """The warnings raised inside the block, as a list (and kept from the user), or () with the warnings left alone."""
    if not on:
        yield ()
        return
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        yield caught


class GraphSide:
    """The private stream and the memory pool of one owner's captured graphs, both made at first use."""

    def __init__(self):
        self._stream = self._pool = None

    def stream(self):
        """The one non-default stream every graph-mode pass of the owner runs on, warm-up, capture, replay and eager alike.  autograd
        binds each parameter's AccumulateGrad node to the stream it was created under and keeps it as long as any autograd
        graph referencing it is alive; if such a node predates the capture on another stream, its in-place gradient
        accumulation is captured on a forked branch whose input buffers the allocator recycles without ordering."""
        if self._stream is None:
            self._stream = torch.cuda.Stream()
        return self._stream

    @contextlib.contextmanager
    def handover(self, active=True):
        """Run the block on the side stream, ordered behind the caller's stream on the way in and in front of it on the way out (no
        host sync).  active=False (an eager session): the block stays on the caller's stream."""
        if not active:
            yield
            return
        side = self.stream()
        side.wait_stream(torch.cuda.current_stream())
        try:
            with torch.cuda.stream(side):
                yield
        finally:
            torch.cuda.current_stream().wait_stream(side)

    def capture(self, run, single_thread=False):
        """Capture res = run(cut) on the side stream out of the shared pool -> ([(graph, bucket ids)], res).  run may call
        cut(bucket_ids, final) any number of times: it ends the running graph, files it with the ids (what the owner launches once
        that graph has been enqueued) and, unless final, begins the next on the same stream and pool.  A pass that never cuts is one
        graph with ids []; a capture still open when run returns or raises is ended and filed the same way, so the chain never ends
        in an empty graph and an exception leaves no capture open.  single_thread: autograd runs its backward on the calling thread,
        which a cut from inside backward needs (thread-local capture mode: begin and end on one thread).  The caching allocator
        keeps the pool handle usable only while a graph captured out of it is alive (tests/test_graphs_gpu.py)."""
        if self._pool is None:
            self._pool = torch.cuda.graph_pool_handle()
        chain, cur = [], [None]

        def begin():
            g = torch.cuda.CUDAGraph()
            # thread_local: RCCL's watchdog / proxy threads may touch the runtime while this thread captures
            g.capture_begin(pool=self._pool, capture_error_mode="thread_local")
            cur[0] = g

        def cut(bucket_ids, final):
            cur[0].capture_end()
            chain.append((cur[0], list(bucket_ids)))
            cur[0] = None
            if not final:                              # the last buckets close the pass: nothing is enqueued after them
                begin()

        torch.cuda.synchronize()
        gc.collect()
        threads = torch.autograd.set_multithreading_enabled(False) if single_thread else contextlib.nullcontext()
        with torch.cuda.stream(self.stream()), threads:
            begin()
            try:
                res = run(cut)
            finally:
                if cur[0] is not None:
                    cur[0].capture_end()
                    chain.append((cur[0], []))
                    cur[0] = None
        return chain, res

    def attempt(self, cache, key, static, run, audit, what, noun, record=False, single_thread=False):
        """The capture attempt of a signature cache.lookup() said to capture -> the entry, stored in the cache:
        {"graph": chain, "static": st, "result": res}, or {"graph": None, "reason": why} with a warning when the capture was refused
        or failed (the owner then runs the signature eagerly).  static() builds the static inputs st, after the cache has made room;
        run(st, cut) is one pass (cut is None in the warm-up passes); audit(st) runs one pass and returns its memset count
        (count_memsets); what / noun name the signature and the pass in the texts.

        record: the warnings of both warm-up passes are recorded for the verdict and kept from the user, the capture-audit warning
        and every other one with them.  The train step does that (an AccumulateGrad stream mismatch refuses its capture); the
        inference session does not, and its warm-up warnings reach the user."""
        cache.make_room()                              # bounded cache; the executables go, the shared pool keeps the memory
        st = static()
        with self.handover(), _recorded(record) as caught:
            run(st, None)                              # allocator / lazily built caches / AccumulateGrad nodes / hook counts
            memsets = audit(st)                        # second warm-up pass, audited
        reason = refusal(memsets, caught, noun)
        if reason is not None:
            warnings.warn("gw_depth_amd: HIP-graph capture refused for %s signature %r, running eager: %s" % (what, key, reason))
            return cache.store(key, {"graph": None, "reason": reason})
        try:
            chain, res = self.capture(lambda cut: run(st, cut), single_thread)
        except RuntimeError as e:                      # capture invalidated: keep going, eagerly, and say so
            torch.cuda.synchronize()
            warnings.warn("gw_depth_amd: HIP-graph capture failed for %s signature %r, running eager: %s" % (what, key, e))
            return cache.store(key, {"graph": None, "reason": str(e)})
        return cache.store(key, {"graph": chain, "static": st, "result": res})
