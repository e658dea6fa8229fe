"""The witness table of the convolution kernels (plain module, no GPU): tests/golden/conv_witnesses.txt holds, for every kernel the
dispatcher of csrc/igemm.hip, thinconv.hip and tileconv.hip can launch, ONE call that reaches it -

    <mangled kernel name> <call>

where <call> is a line of the `--stdin` mode of tests/dispatch_recorder.cpp (plain numbers, settings only):

    F <B Hi Wi Cin Cout k s gather dtype zero_page> <epilogue kind 0..11> <ln_C> <act_scale: 0 = 1.0 | 1 = 0.7>      gwd_conv_forward
    W <B Hi Wi Cin Cout k s gather dtype zero_page> <scaled 0|1>                      gwd_conv_wgrad
    B <n> <B Hi Wi Cin Cout k s gather dtype zero_page> <scaled 0|1>                  gwd_conv_wgrad_batch: n jobs, job i on B + i images

tools/make_conv_witnesses.py writes the table; tests/test_conv_witnesses.py keeps it honest on the CPU and
tests/test_conv_witnesses_gpu.py runs every line against the fp64 reference of tests/conv_ref.py."""
import os
import re
import subprocess
import types

from tests.test_conv_dispatch import ROOT, llvm_tool, object_paths

FIXTURE = os.path.join(ROOT, "tests", "golden", "conv_witnesses.txt")
KINDS = ["plain", "bn_relu", "gelu_z", "elu", "mult_res", "mult_relu", "mult_relu_z", "gate_relu", "gate_gelu", "convln", "convln_gelu", "bias_relu_res"]
GATHER_CONV, GATHER_TRANSPOSED, GATHER_UPSAMPLED = 0, 1, 2
F32, BF16 = 0, 1
ACT_SCALE = 0.699999988079071                    # 0.7f, what the recorder sets: no power of two, so the epilogue's multiply rounds
MAX_MACS = 4e10                                  # no witness above this: the fp64 reference of its compared rows has to fit a test


def build_recorder(workdir):
    exe = os.path.join(str(workdir), "dispatch_recorder")
    subprocess.check_call([llvm_tool("clang++"), "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "dispatch_recorder.cpp")] + object_paths() + ["-o", exe])
    return exe


def replay(exe, calls):
    """calls: lines as above -> one record (str) per call."""
    env = {k: v for k, v in os.environ.items() if k != "GWD_IGEMM_DMA"}
    out = subprocess.run([exe, "--stdin"], input=("\n".join(calls) + "\n").encode(), stdout=subprocess.PIPE, check=True, env=env).stdout.decode()
    records = out.splitlines()
    assert len(records) == len(calls), (len(records), len(calls))
    return records


def launches(record):
    """(return code, [(kernel, grid x)]) of a record."""
    rc = int(re.search(r" rc=(-?\d+)", record).group(1))
    return rc, [(k, int(g)) for k, g in re.findall(r" \| (\S+) (\d+),", record)]


def parse_call(call):
    """A call line -> a namespace with the descriptor fields as tests/dispatch_recorder.cpp's make_desc derives them."""
    f = call.split()
    c = types.SimpleNamespace(call=f[0], text=call, n=1, kind=0, ln_C=0, scaled=0, act_scale=1.0)
    v = [int(t) for t in f[1:]]
    if c.call == "B":
        c.n, v = v[0], v[1:]
    c.B, c.Hi, c.Wi, c.Cin, c.Cout, c.k, c.stride, c.gather, c.dtype, c.zero_page = v[:10]
    if c.call == "F":
        c.kind, c.ln_C = v[10], v[11]
        c.act_scale = ACT_SCALE if v[12] else 1.0
        if c.kind in (9, 10) and c.ln_C == 0:
            c.ln_C = c.Cout
    else:
        c.scaled = v[10]
    c.pad = c.k // 2 if c.k & 1 else 0
    k, s, p = c.k, c.stride, c.pad
    c.Hv = c.Wv = 0
    if c.gather == GATHER_CONV:
        c.Ho, c.Wo = (c.Hi + 2 * p - k) // s + 1, (c.Wi + 2 * p - k) // s + 1
    elif c.gather == GATHER_TRANSPOSED:
        op = 1 if (s == 2 and k & 1) else 0
        c.Ho, c.Wo = (c.Hi - 1) * s + k - 2 * p + op, (c.Wi - 1) * s + k - 2 * p + op
    else:
        c.Hv, c.Wv = 2 * c.Hi, 2 * c.Wi
        c.Ho, c.Wo = c.Hv + 2 * p - k + 1, c.Wv + 2 * p - k + 1
    c.K = k * k * c.Cin
    return c


def with_batch(c, i):
    """Job i of a batched call: the same layer on B + i images."""
    d = types.SimpleNamespace(**vars(c))
    d.B = c.B + i
    return d


def macs(c):
    return sum((c.B + i) * c.Ho * c.Wo * c.Cout * c.K for i in range(c.n))


def short_name(kernel):
    """igemm_dma_kernel<256,160,8,1,3,0,0,0,0,0,1,1,32,1,0> from the mangled name (test ids, reports)."""
    m = re.search(r"\d+([a-z_]+_kernel)(I(?:DF16b|f|L[ib]n?\d+E)+E)?", kernel)
    args = [{"DF16b": "bf16", "f": "f32"}.get(t, t[2:-1].replace("n", "-")) for t in re.findall(r"DF16b|f|L[ib]n?\d+E", m.group(2) or "")]
    return "%s<%s>" % (m.group(1), ",".join(args)) if args else m.group(1)


def family(kernel):
    return re.search(r"\d+([a-z_]+_kernel)", kernel).group(1)


def load(path=FIXTURE):
    """[(kernel, call namespace)] in file order."""
    rows = []
    for line in open(path):
        line = line.strip()
        if line and not line.startswith("#"):
            kernel, call = line.split(" ", 1)
            rows.append((kernel, parse_call(call)))
    return rows
