"""Shape buckets and the captured-step cache policy, on the CPU: data.bucket_shape / padded_size, graphs.GraphCache (the pure
bookkeeping of TrainStep's graph mode) and the shape census of the training augmentation that motivates both."""
import functools

import pytest

from gw_depth_amd import graphs
from gw_depth_amd.data import bucket_shape, padded_size
from gw_depth_amd.graphs import GraphCache


def _census_tool():
    """tools/shape_census.py as a module (tools/ is a directory of scripts, not a package)."""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "shape_census.py")
    spec = importlib.util.spec_from_file_location("shape_census", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_bucket_shape_rounds_up_to_the_step():
    assert bucket_shape(64, 128) == (64, 128) and bucket_shape(640, 1024, 64) == (640, 1024)        # exact multiples stay
    assert bucket_shape(65, 129) == (128, 192) and bucket_shape(641, 1, 64) == (704, 64)            # one more goes a whole step up
    assert bucket_shape(90, 120, 32) == (96, 128) and bucket_shape(70, 101, 32) == (96, 128)
    for hw in ((1, 1), (90, 121), (719, 1280)):
        assert bucket_shape(*hw, step=1) == hw                                                      # step 1 is the identity
    for bad in (0, -64):
        with pytest.raises(ValueError):
            bucket_shape(10, 10, bad)


def test_padded_size_forms():
    assert padded_size(90, 120, None) == (90, 120)
    assert padded_size(90, 120, 32) == (96, 128)
    assert padded_size(90, 120, (128, 160)) == (128, 160) and padded_size(90, 120, (90, 120)) == (90, 120)
    for small in ((89, 160), (128, 119)):
        with pytest.raises(ValueError):
            padded_size(90, 120, small)


def _captured(cache, key):
    verdict, ent = cache.lookup(key)
    if verdict == "capture":
        ent = cache.store(key, {"graph": [key]})
    return verdict, ent


def test_cache_keeps_the_most_recently_used():
    c = GraphCache(max_graphs=3)
    for k in "abc":
        assert _captured(c, k)[0] == "capture"
    assert list(c.entries) == ["a", "b", "c"]
    verdict, ent = c.lookup("a")                                   # a hit moves the entry to the young end
    assert verdict == "known" and ent["graph"] == ["a"] and list(c.entries) == ["b", "c", "a"]
    assert _captured(c, "d")[0] == "capture"                       # the bound: the oldest ("b") goes
    assert list(c.entries) == ["c", "a", "d"] and c.stats["evictions"] == 1
    assert _captured(c, "b")[0] == "capture" and list(c.entries) == ["a", "d", "b"]
    assert c.stats["captures"] == 5 and c.stats["evictions"] == 2 and c.stats["refused"] == 0


def test_cache_bound_defaults_to_the_module_constant_at_call_time(monkeypatch):
    c = GraphCache()
    assert c.bound() == graphs.MAX_GRAPHS
    monkeypatch.setattr(graphs, "MAX_GRAPHS", 2)
    for k in "abc":
        _captured(c, k)
    assert list(c.entries) == ["b", "c"] and c.stats["evictions"] == 1
    assert GraphCache(max_graphs=16).bound() == 16
    for bad in ({"max_graphs": 0}, {"capture_after": 0}):
        with pytest.raises(ValueError):
            GraphCache(**bad)


def test_capture_after_defers_the_capture():
    c = GraphCache(max_graphs=4, capture_after=2)
    assert c.lookup("a") == ("wait", None) and not c.entries       # first sight: eager, and no entry
    assert c.lookup("b") == ("wait", None)
    assert _captured(c, "a")[0] == "capture"                       # second sight: captured
    assert c.lookup("a")[0] == "known"
    assert list(c.entries) == ["a"] and c.stats["captures"] == 1
    c3 = GraphCache(capture_after=3)
    assert [c3.lookup("x")[0] for _ in range(3)] == ["wait", "wait", "capture"]


def test_cache_counters():
    c = GraphCache(max_graphs=2)
    assert set(c.stats) == {"replays", "captures", "eager_steps", "evictions", "refused", "host_matcher_steps"} and not any(c.stats.values())
    c.lookup("a")
    c.store("a", {"graph": None, "reason": "refused"})             # a refused capture keeps its entry (no second attempt) and is counted apart
    assert c.lookup("a")[0] == "known" and c.stats["refused"] == 1 and c.stats["captures"] == 0
    c.count("replays")
    c.count("eager_steps", 2)
    c.count("host_matcher_steps")
    assert (c.stats["replays"], c.stats["eager_steps"], c.stats["host_matcher_steps"]) == (1, 2, 1)


@functools.lru_cache(maxsize=None)
def _stream(pad_to):
    return tuple(_census_tool().batch_shape_stream(1280, 720, 8, 2000, seed=0, pad_to=pad_to))


def test_census_of_the_training_augmentation():
    """720x1280 frames, B=8, 2000 batches of DeviceAugment(seed=0): hundreds of padded sizes as they come, at most 16 in buckets of 64,
    which an LRU of 16 captured steps serves almost always."""
    raw, b64 = _stream(None), _stream(64)
    assert len(set(raw)) > 300
    assert len(set(b64)) <= 16
    assert all(H % 64 == 0 and W % 64 == 0 and 0 <= H - h < 64 and 0 <= W - w < 64 for (H, W), (h, w) in zip(b64, raw))
    lru_hit_rate = _census_tool().lru_hit_rate
    assert lru_hit_rate(b64, 16) > 0.98
    assert lru_hit_rate(raw, 6) < 0.5                               # what the parent's cache of 6 makes of the raw stream
