"""Regenerate tests/golden/munc/munc_*.npz from the COMPILED REFERENCE natives (`make -C oracle ref`; build image only).

    python tests/golden/make_munc_golden.py

Every case of munc_cases runs through the reference's `cconsenrich.cMuncObservationMomentSeedPass` /
`cMuncSmoothDenseLocalEvidence` and through the pure-Python twin (tests/twin_munc.py); a fixture is written only if the two agree
bit for bit on every case and raise the same error texts.  Fixtures hold outputs only (and the reference's error texts): the
inputs are re-synthesised from the case table."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), HERE]

import munc_cases  # noqa: E402
import twin_munc  # noqa: E402
from oracle import ref_loader  # noqa: E402


def main() -> int:
    ref = ref_loader.load()
    if ref is None:
        print("the compiled reference is not available (make -C oracle ref)", file=sys.stderr)
        return 2
    groups, diffs, count = {}, 0, 0
    for cases, run in ((munc_cases.seed_cases(), munc_cases.run_seed), (munc_cases.smooth_cases(), munc_cases.run_smooth)):
        for case in cases:
            count += 1
            want, got = run(ref, case), run(twin_munc, case)
            if not munc_cases.same(want, got):
                diffs += 1
                print("twin differs from the reference:", case["name"])
            for field, arr in want.items():
                groups.setdefault(case["group"], {})[f"{case['name']}/{field}"] = arr
    texts = {}
    calls = [(name, lambda mod, a=a, k=k: mod.cMuncObservationMomentSeedPass(*a, **k), text)
             for name, a, k, text in munc_cases.seed_error_cases()]
    calls += [("smooth_" + name, lambda mod, l=l, w=w, mk=mk, e=e: mod.cMuncSmoothDenseLocalEvidence(l, w, excludeMask=mk, eps=e), text)
              for name, l, w, mk, e, text in munc_cases.smooth_error_cases()]
    for name, call, text in calls:
        for mod in (ref, twin_munc):
            try:
                call(mod)
                diffs += 1
                print("no error:", name, mod.__name__)
            except ValueError as e:
                if str(e) != text:
                    diffs += 1
                    print("other error text:", name, mod.__name__, e)
                if mod is ref:
                    texts[name] = str(e)
    print(f"{count} cases, {len(texts)} errors, {diffs} differences between the twin and the reference")
    if diffs:
        return 1
    os.makedirs(os.path.join(HERE, "munc"), exist_ok=True)
    for group, arrs in groups.items():
        path = os.path.join(HERE, "munc", f"munc_{group}.npz")
        np.savez_compressed(path, **arrs)
        print(path, os.path.getsize(path), "bytes")
    path = os.path.join(HERE, "munc", "munc_errors.npz")
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in texts.items()})
    print(path, os.path.getsize(path), "bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
