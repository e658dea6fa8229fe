"""The witness table of the row kernels (plain module, no GPU): tests/golden/row_witnesses.txt holds, for every kernel that the twelve
entry points of csrc/rowops.hip and csrc/inorm.hip can launch, ONE call that reaches it -

    <mangled kernel name> <call>

where <call> is a line of tests/row_recorder.cpp (plain numbers, settings only; a flag is 0 | 1):

    LF <dtype rows C ld> <gamma/beta residual gelu>                   gwd_layernorm_forward        (ld 0 = C)
    LB <dtype rows C ld> <gamma/beta gelu gskip elu_input dgamma>     gwd_layernorm_backward
    SF <dtype rows L>                                                 gwd_softmax_forward
    SB <dtype rows L>                                                 gwd_softmax_backward
    SM <dtype rows L> <mask rows_per_mask scale>                      gwd_softmax_masked_forward   (scale: 0 = 1.0 | 1 = 0.3)
    SS <dtype rows L> <scale>                                         gwd_softmax_scaled_backward
    AB <dtype rows C> <act act_scale per_channel_scale>               gwd_act_backward             (act_scale: 0 = 1.0 | 1 = 0.7)
    CS <dtype rows C>                                                 gwd_colsum
    CB <dtype n> <rows C> x n                                         gwd_colsum_batch
    AC <dtype rows C> <act act_scale mult>                            gwd_act_backward_colsum
    IF <dtype B L C S>                                                gwd_inorm_gelu_forward
    IB <dtype B L C S>                                                gwd_inorm_gelu_backward

The two inorm entry points launch two kernels each: a call may stand behind both of its kernels' lines.
tools/make_row_witnesses.py writes the table; tests/test_row_witnesses.py keeps it honest on the CPU and
tests/test_row_witnesses_gpu.py runs every line against the fp64 references of tests/row_ref.py."""
import os
import re
import subprocess
import sys
import types

from tests.test_conv_dispatch import CSRC, ROOT, llvm_tool

FIXTURE = os.path.join(ROOT, "tests", "golden", "row_witnesses.txt")
OBJECTS = ["rowops.o", "inorm.o"]
F32, BF16 = 0, 1
SCALE = 0.30000001192092896                      # 0.3f and 0.7f, what the recorder passes: no powers of two, so the multiply rounds
ACT_SCALE = 0.699999988079071
ACT_NONE, ACT_RELU, ACT_GELU, ACT_ELU, ACT_SIGMOID = 0, 1, 2, 3, 4
MAX_BYTES = 64 << 20                             # all operands of a witness together stay under this
FIELDS = {
    "LF": ("rows", "C", "ld", "affine", "residual", "gelu"),
    "LB": ("rows", "C", "ld", "affine", "gelu", "gskip", "elu", "dgamma"),
    "SF": ("rows", "L"), "SB": ("rows", "L"), "SM": ("rows", "L", "mask", "rpm", "scaled"), "SS": ("rows", "L", "scaled"),
    "AB": ("rows", "C", "act", "act_scaled", "chscale"), "CS": ("rows", "C"), "AC": ("rows", "C", "act", "act_scaled", "mult"),
    "IF": ("B", "L", "C", "S"), "IB": ("B", "L", "C", "S"),
}
FAMILY = {"LF": "layernorm", "LB": "layernorm", "SF": "softmax", "SB": "softmax", "SM": "softmax", "SS": "softmax", "AB": "act", "AC": "act",
          "CS": "colsum", "CB": "colsum", "IF": "inorm", "IB": "inorm"}


def object_paths():
    paths = [os.path.join(CSRC, o) for o in OBJECTS]
    if not all(os.path.exists(p) for p in paths):
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    return paths


def build_recorder(workdir):
    exe = os.path.join(str(workdir), "row_recorder")
    subprocess.check_call([llvm_tool("clang++"), "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "row_recorder.cpp")] + object_paths() + ["-o", exe])
    return exe


def replay(exe, calls):
    """calls: lines as above -> one record (str) per call."""
    out = subprocess.run([exe], input=("\n".join(calls) + "\n").encode(), stdout=subprocess.PIPE, check=True).stdout.decode()
    records = out.splitlines()
    assert len(records) == len(calls), (len(records), len(calls))
    return records


def launches(record):
    """(return code, [(kernel, grid x, block)]) of a record."""
    rc = int(re.search(r" rc=(-?\d+)", record).group(1))
    return rc, [(k, int(g), int(b)) for k, g, b in re.findall(r" \| (\S+) (\d+),\d+,\d+ (\d+)", record)]


def device_stubs():
    """Mangled names of every kernel the two objects can launch (their host-side launch stubs)."""
    out = subprocess.run([llvm_tool("llvm-readelf"), "-s", "-W"] + object_paths(), stdout=subprocess.PIPE, check=True).stdout.decode()
    return set(re.findall(r"\s(_Z\S*__device_stub__\S+)", out))


def parse_call(call):
    f = call.split()
    v = [int(t) for t in f[1:]]
    c = types.SimpleNamespace(call=f[0], text=call, dtype=v[0], family=FAMILY[f[0]])
    if c.call == "CB":
        c.jobs = [(v[2 + 2 * i], v[3 + 2 * i]) for i in range(v[1])]
        assert len(v) == 2 + 2 * v[1], call
    else:
        names = FIELDS[c.call]
        assert len(v) == 1 + len(names), call
        for n, x in zip(names, v[1:]):
            setattr(c, n, x)
    if c.call in ("LF", "LB"):
        c.pitch = c.ld or c.C
    if c.call in ("SM", "SS"):
        c.scale = SCALE if c.scaled else 1.0
    if c.call in ("AB", "AC"):
        c.act_scale = ACT_SCALE if c.act_scaled else 1.0
    return c


def esize(c):
    return 2 if c.dtype == BF16 else 4


def nbytes(c):
    """All operands of the call together."""
    e = esize(c)
    if c.call == "LF":
        return c.rows * c.pitch * e * (2 + c.residual) + 8 * c.rows
    if c.call == "LB":
        return c.rows * c.pitch * e * (3 + c.gskip) + 8 * c.rows
    if c.call in ("SF", "SM"):
        return c.rows * c.L * e * 2 + (c.rows * c.L // c.rpm if c.call == "SM" and c.mask else 0)
    if c.call in ("SB", "SS"):
        return c.rows * c.L * e * 3
    if c.call == "AB":
        return c.rows * c.C * e * 3
    if c.call == "AC":
        return c.rows * c.C * e * (3 + c.mult)
    if c.call == "CS":
        return c.rows * c.C * e
    if c.call == "CB":
        return sum(r * C * e for r, C in c.jobs)
    return c.B * c.L * c.C * e * 3 + c.B * c.S * c.C * 8


def short_name(kernel):
    m = re.search(r"\d+([a-z_]+_kernel)(I(?:DF16b|f|L[ib]n?\d+E)+E)?", kernel)
    args = [{"DF16b": "bf16", "f": "f32"}.get(t, t[2:-1].replace("n", "-")) for t in re.findall(r"DF16b|f|L[ib]n?\d+E", m.group(2) or "")]
    return "%s<%s>" % (m.group(1), ",".join(args)) if args else m.group(1)


def load(path=FIXTURE):
    """[(kernel, call namespace)] in file order."""
    rows = []
    for line in open(path):
        line = line.strip()
        if line and not line.startswith("#"):
            kernel, call = line.split(" ", 1)
            rows.append((kernel, parse_call(call)))
    return rows
