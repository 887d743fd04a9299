"""Record tests/golden/conv_bits.json: SHA-256 of the outputs of every case of tests/conv_bits_cases.py (needs the GPU).

    python tools/make_golden_conv_bits.py --commit SHA

Like tests/golden/conv_dispatch.json this is recorded from the build of the commit BEFORE a change to the conv host code
(`--commit`, stored in the file) and not regenerated from the changed code: tests/test_gpu_conv_bits.py then proves that every
launch still produces the same bytes."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import conv_bits_cases as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit the loaded library was built from")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "conv_bits.json"))
    a = ap.parse_args()
    res = {"commit": a.commit, "cases": {}}
    for c in T.CASES:
        want, got = T.queries(c)
        assert want == c.classes, (c.name, got)
        first, again = T.run(c), T.run(c)
        assert first == again, (c.name, "two runs differ: not a fixed-order reduction")
        res["cases"][c.name] = first
        print(c.name, got, sorted(first), flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
