#!/usr/bin/env python3
"""Record the goldens of tests/test_gpu_nf_sites.py: tests/golden/nf_sites/<case>.npz.

usage (on the GPU): MRBO_LIB=/path/to/libmrbo.so python tools/record_nf_sites.py [case ...]
MRBO_LIB names the library whose bits are recorded -- a build of the commit that the test is to
hold later changes to (mrbo/_lib.py reads it); without it the tree's own library is recorded.  Every
case runs through the test module's run_case(), must report the plan.info() entries the test expects
and must pass its work assertions (check_work) before its file is written; one summary line per case
is printed.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_nf_sites as T  # noqa: E402


def main():
    from mrbo import _lib
    names = sys.argv[1:] or list(T.ALL_CASES)
    os.makedirs(T.GOLDEN_DIR, exist_ok=True)
    print("library:", _lib.LIB_PATH)
    bad = 0
    for name in names:
        info, out, g = T.run_case(name)
        want = T.expected_info(name)
        got = {k: info[k] for k in want}
        ev = out["evals"]
        line = f"{name}: info {info} status {sorted(set(out['status'].ravel().tolist()))} " \
               f"work max {ev.reshape(ev.shape[0], -1).max(axis=1).tolist()}"
        try:
            assert got == want, f"plan.info() {got}, expected {want}"
            T.check_work(name, out, g)
        except AssertionError as e:
            bad += 1
            print(line, "NOT RECORDED:", e)
            continue
        path = os.path.join(T.GOLDEN_DIR, f"{name}.npz")
        np.savez_compressed(path, **{k: out[k] for k in T.OUTPUTS})
        print(line, f"-> {os.path.getsize(path)} bytes")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
