"""Regenerate tests/golden/dwb/dwb_*.npz from the COMPILED REFERENCE natives (`make -C oracle ref`; build image only).

    python tests/golden/make_dwb_golden.py

Every case of dwb_cases.cases() runs through the reference's `consenrich.cconsenrich` and through the pure-Python twin
(tests/twin_dwb.py); a fixture is written only if the two agree bit for bit on every case.  Fixtures hold outputs only: the
inputs are re-synthesised from the case table."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), HERE]

import dwb_cases  # noqa: E402
import twin_dwb  # noqa: E402
from oracle import ref_loader  # noqa: E402


def main() -> int:
    ref = ref_loader.load()
    if ref is None:
        print("the compiled reference is not available (make -C oracle ref)", file=sys.stderr)
        return 2
    groups, diffs = {}, 0
    for case in dwb_cases.cases():
        want = dwb_cases.run_case(ref, case)
        got = dwb_cases.run_case(twin_dwb, case)
        if not dwb_cases.same(want, got):
            diffs += 1
            print("twin differs from the reference:", case["name"])
        for field, arr in want.items():
            groups.setdefault(case["group"], {})[f"{case['name']}/{field}"] = arr
    # the error texts of the reference
    for f, args, text in ((ref.cGenerateDWBMultipliersFromNoise, (np.zeros(4), 2), "noise length is too short"),
                          (ref.cApplyStationaryNullDWB, (np.zeros(4), np.zeros(3)), "must have the same length"),
                          (ref.cGenerateDWBMultipliersFromNoise, (np.zeros(40), 2, "boxcar"), "Unknown DWB kernel: boxcar")):
        for g in (f, getattr(twin_dwb, f.__name__)):
            try:
                g(*args)
                diffs += 1
                print("no error:", f.__name__)
            except ValueError as e:
                if text not in str(e):
                    diffs += 1
                    print("other error text:", f.__name__, e)
    print(f"{len(dwb_cases.cases())} cases, {diffs} differences between the twin and the reference")
    if diffs:
        return 1
    for group, arrs in groups.items():
        path = os.path.join(HERE, "dwb", f"dwb_{group}.npz")
        os.makedirs(os.path.dirname(path), exist_ok=True)
        np.savez_compressed(path, **arrs)
        print(path, os.path.getsize(path), "bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
