"""Write tests/golden/autograd_trace.txt, the launch-sequence witness of the conv-family autograd nodes (tests/autograd_trace.py).

    python tools/make_autograd_trace.py cpu            # the dry-mode sections, anywhere
    python tools/make_autograd_trace.py gpu            # the delegating-mode sections, on the MI355X
    (--out FILE: write there instead; the other mode's sections are carried over from the golden file)

Regenerate only after an INTENDED change of the launch sequence, and read the diff of the golden file: it is the change."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "autograd_trace.txt")


def main():
    from tests import autograd_trace as A
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["cpu", "gpu"])
    ap.add_argument("--out", default=GOLDEN)
    args = ap.parse_args()
    old = A.sections(open(GOLDEN).read()) if os.path.exists(GOLDEN) else {}
    new = {}
    for case in A.CASES:
        if args.mode == "cpu" and case.gpu_only:
            continue
        new["%s %s" % (args.mode, case.name)] = A.run_case(case, "cpu" if args.mode == "cpu" else "cuda")
        print("%s %s: %d lines" % (args.mode, case.name, len(new["%s %s" % (args.mode, case.name)])), flush=True)
    keep = {k: v for k, v in old.items() if not k.startswith(args.mode + " ")}
    both = dict(keep, **new)
    with open(args.out, "w") as f:
        for k in sorted(both, key=lambda k: (k.split()[0], list(both).index(k))):
            same = k.startswith("gpu ") and both[k] == both.get("cpu " + k[4:])       # the real answers took the scripted path
            f.write("== %s\n%s\n" % (k, A.SAME_AS_CPU if same else "\n".join(both[k])))


if __name__ == "__main__":
    main()
