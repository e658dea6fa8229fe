"""CPU: which kernel, grid, block, LDS size and scalar arguments every convolution descriptor gets - pinned without a GPU.

tests/dispatch_recorder.cpp links csrc/igemm.o, thinconv.o and tileconv.o against stubs of the HIP runtime and prints one record
per gwd_conv_forward / gwd_conv_wgrad / gwd_conv_wgrad_batch call of a descriptor grid.  tests/golden/conv_dispatch.txt holds
the SHA-256 of that stream (whole and per section) and the launch count of every kernel, generated from the objects of the commit
BEFORE the dispatcher was rewritten as selection + launch (`python tests/test_conv_dispatch.py --write-fixture` regenerates it from
the objects in csrc/ - only for a change that is MEANT to move a shape to another kernel)."""
import collections
import hashlib
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gw_depth_amd", "csrc")
OBJECTS = ["igemm.o", "thinconv.o", "tileconv.o"]
FIXTURE = os.path.join(ROOT, "tests", "golden", "conv_dispatch.txt")

# Kernels of the three objects that no descriptor can reach, as patterns over the mangled name.  tileconv.hip's launch_wgrad<64, 32>
# requests the LDS size for tconv_wgrad_kernel<64, 32, UP, TPW = 3> and then always launches the one-tap-per-wave variant (TPW = 1).
NOT_DISPATCHED = [r"tconv_wgrad_kernelILi64ELi32ELb[01]ELi3E"]


def llvm_tool(name):
    hipcc = os.path.realpath(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    for d in (os.path.join(os.path.dirname(os.path.dirname(hipcc)), "llvm", "bin"), os.path.join(os.path.dirname(os.path.dirname(hipcc)), "lib", "llvm", "bin"), "/opt/rocm/llvm/bin"):
        if os.path.exists(os.path.join(d, name)):
            return os.path.join(d, name)
    raise FileNotFoundError(name)


def object_paths(csrc=CSRC):
    paths = [os.path.join(csrc, o) for o in OBJECTS]
    if not all(os.path.exists(p) for p in paths):
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    return paths


def record(workdir, csrc=CSRC):
    """Builds the recorder against the objects of `csrc` and returns its output (bytes)."""
    env = {k: v for k, v in os.environ.items() if k != "GWD_IGEMM_DMA"}          # the one run-time switch of the dispatch: at its default
    exe = os.path.join(str(workdir), "dispatch_recorder")
    subprocess.check_call([llvm_tool("clang++"), "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "dispatch_recorder.cpp")] + object_paths(csrc) + ["-o", exe])
    return subprocess.run([exe], stdout=subprocess.PIPE, check=True, env=env).stdout


def device_stubs(csrc=CSRC):
    """Mangled names of every kernel the objects can launch (their host-side launch stubs)."""
    out = subprocess.run([llvm_tool("llvm-readelf"), "-s", "-W"] + object_paths(csrc), stdout=subprocess.PIPE, check=True).stdout.decode()
    return set(re.findall(r"\s(_Z\S*__device_stub__\S+)", out))


def kernel_key(mangled):
    """A kernel's mangled name and the name of its host-side launch stub, brought to one form (length prefix and stub marker dropped)."""
    key, n = re.subn(r"\d+(?:__device_stub__)?(?=[a-z](?:(?!__)[a-z_])*_kernel[IEvP])", "", mangled)
    assert n == 1, mangled
    return key


def summarize(stream):
    sections = []
    for part in re.split(rb"(?m)^(?=# )", stream):
        if part:
            title, _, body = part.partition(b"\n")
            sections.append((hashlib.sha256(part).hexdigest(), body.count(b"\n"), title[2:].decode()))
    counts = collections.Counter(re.findall(rb" \| (\S+)", stream))
    lines = ["sha256 %s records %d" % (hashlib.sha256(stream).hexdigest(), sum(s[1] for s in sections)), "[sections]"]
    lines += ["%s %7d %s" % s for s in sections]
    lines.append("[kernels]")
    lines += ["%8d %s" % (n, k.decode()) for k, n in sorted(counts.items())]
    return "\n".join(lines) + "\n", counts


@pytest.fixture(scope="module")
def stream(tmp_path_factory):
    return record(tmp_path_factory.mktemp("dispatch"))


def test_every_descriptor_gets_the_recorded_kernel(stream, tmp_path):
    got, _ = summarize(stream)
    want = open(FIXTURE).read()
    if got != want:
        dump = os.path.join(str(tmp_path), "conv_dispatch_stream.txt")
        open(dump, "wb").write(stream)
        g, w = got.splitlines(), want.splitlines()
        diff = [a for a in g if a not in set(w)][:12] + ["-- fixture has:"] + [b for b in w if b not in set(g)][:12]
        # the first records of the first section whose hash differs
        bad = [s for s in g[2:g.index("[kernels]")] if s not in set(w)]
        head = []
        if bad:
            title = ("# " + bad[0].split(None, 2)[2]).encode()
            at = stream.find(title)
            head = stream[at:at + 4000].decode().splitlines()[:12]
        raise AssertionError("dispatch differs from tests/golden/conv_dispatch.txt (full stream: %s)\n%s\nfirst records of the first differing section:\n%s"
                             % (dump, "\n".join(diff), "\n".join(head)))


def test_every_kernel_is_launched_or_listed(stream):
    _, counts = summarize(stream)
    launched = {kernel_key(k.decode()) for k in counts}
    stubs = {kernel_key(s) for s in device_stubs()}
    assert len(stubs) >= 270 and launched <= stubs
    missing = sorted(k for k in stubs - launched if not any(re.search(p, k) for p in NOT_DISPATCHED))
    assert not missing, "kernels no descriptor of the grid reaches:\n" + "\n".join(missing)
    for p in NOT_DISPATCHED:                          # the list holds nothing that IS launched, and nothing that does not exist
        assert any(re.search(p, k) for k in stubs) and not any(re.search(p, k) for k in launched), p


if __name__ == "__main__":
    import tempfile
    if sys.argv[1:2] == ["--write-fixture"]:
        csrc = sys.argv[2] if len(sys.argv) > 2 else CSRC
        with tempfile.TemporaryDirectory() as t:
            open(FIXTURE, "w").write(summarize(record(t, csrc))[0])
        print("wrote", FIXTURE)
