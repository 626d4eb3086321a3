"""Regenerate tests/golden/rocco/rocco_*.npz from the COMPILED REFERENCE natives (`make -C oracle ref`; build image only).

    python tests/golden/make_rocco_golden.py

Every case of rocco_cases.cases() runs through the reference's `consenrich.cconsenrich` and through the pure-Python twin
(tests/twin_rocco.py); a fixture is written only if the two agree bit for bit on every case.  Fixtures hold data only: the
inputs are re-synthesised from the case table, the outputs are the packed mask, three float64 values and the count."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), HERE]

import rocco_cases  # noqa: E402
import twin_rocco  # noqa: E402
from oracle import ref_loader  # noqa: E402


def main() -> int:
    ref = ref_loader.load()
    if ref is None:
        print("the compiled reference is not available (make -C oracle ref)", file=sys.stderr)
        return 2
    groups, diffs = {}, 0
    for case in rocco_cases.cases():
        want = rocco_cases.run_case(ref, case)
        got = rocco_cases.run_case(twin_rocco, case)
        if not rocco_cases.same(want, got):
            diffs += 1
            print("twin differs from the reference:", case["name"], want["floats"], got["floats"], want["count"], got["count"])
        for field, arr in want.items():
            groups.setdefault(case["group"], {})[f"{case['name']}/{field}"] = arr
    # run bounds: the twin against the reference on the masks of the table
    rng = np.random.default_rng(3)
    for mask in (np.zeros(50, np.uint8), np.ones(50, np.uint8), (rng.random(3000) < 0.2).astype(np.uint8)):
        for gap in (0, 1, 3):
            a, b = ref.cBooleanRunBounds(mask, gap), twin_rocco.cBooleanRunBounds(mask, gap)
            if not (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])):
                diffs += 1
                print("run bounds differ", gap)
    print(f"{len(rocco_cases.cases())} cases, {diffs} differences between the twin and the reference")
    if diffs:
        return 1
    for group, arrs in groups.items():
        path = os.path.join(HERE, "rocco", f"rocco_{group}.npz")
        os.makedirs(os.path.dirname(path), exist_ok=True)
        np.savez_compressed(path, **arrs)
        print(path, os.path.getsize(path), "bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
