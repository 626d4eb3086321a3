"""Regenerate tests/golden/ess/ess_*.npz from the COMPILED REFERENCE native (`make -C oracle ref`; build image only).

    python tests/golden/make_ess_golden.py

Every case of ess_cases.cases() runs through the reference's `cconsenrich.cEstimateEffectiveSampleSize` and through the pure-Python
twin (tests/twin_budget.py); a fixture is written only if the two agree bit for bit on every case and raise the same error texts.
Fixtures hold outputs only (and the reference's error texts): the inputs are re-synthesised from the case table."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), HERE]

import ess_cases  # noqa: E402
import twin_budget  # noqa: E402
from oracle import ref_loader  # noqa: E402


def main() -> int:
    ref = ref_loader.load()
    if ref is None:
        print("the compiled reference is not available (make -C oracle ref)", file=sys.stderr)
        return 2
    groups, diffs = {}, 0
    for case in ess_cases.cases():
        want = ess_cases.run_case(ref, case)
        got = ess_cases.run_case(twin_budget, case)
        if not ess_cases.same(want, got):
            diffs += 1
            print("twin differs from the reference:", case["name"], want, got)
        for field, arr in want.items():
            groups.setdefault(case["group"], {})[f"{case['name']}/{field}"] = arr
    texts = {}
    for case, text in ess_cases.error_cases():
        for mod in (ref, twin_budget):
            try:
                ess_cases.call(mod, case)
                diffs += 1
                print("no error:", case["name"], mod.__name__)
            except ValueError as e:
                if str(e) != text:
                    diffs += 1
                    print("other error text:", case["name"], mod.__name__, e)
                if mod is ref:
                    texts[case["name"]] = str(e)
    print(f"{len(ess_cases.cases())} cases, {len(texts)} errors, {diffs} differences between the twin and the reference")
    if diffs:
        return 1
    os.makedirs(os.path.join(HERE, "ess"), exist_ok=True)
    for group, arrs in groups.items():
        path = os.path.join(HERE, "ess", f"ess_{group}.npz")
        np.savez_compressed(path, **arrs)
        print(path, os.path.getsize(path), "bytes")
    path = os.path.join(HERE, "ess", "ess_errors.npz")
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in texts.items()})
    print(path, os.path.getsize(path), "bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
