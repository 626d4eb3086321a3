"""Regenerate tests/golden/segments/segments_*.npz from the COMPILED REFERENCE native (`make -C oracle ref`; build image only).

    python tests/golden/make_segments_golden.py

Every case of segments_cases.cases() runs through the reference's `consenrich.cconsenrich.cMultiscaleCandidateSegmentStats` and
through the pure-Python twin (tests/twin_segments.py); a fixture is written only if the two agree bit for bit on every case (and
the bin-by-bin form of the twin on the short ones).  Fixtures hold outputs only: the inputs are re-synthesised from the case
table.  The facts about the cap case that tests/test_gpu_segments.py relies on are asserted here."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), HERE]

import segments_cases as SC  # noqa: E402
import twin_segments  # noqa: E402
from oracle import ref_loader  # noqa: E402


class _Loop:
    cMultiscaleCandidateSegmentStats = staticmethod(twin_segments.loop_native)


def check_cap_case():
    """What the cap test needs of its inputs; on a mismatch adjust segments_cases.SEED, not these assertions."""
    case = next(c for c in SC.cases() if c["name"] == "cap16_n8193")
    x, sc, thr, ns = SC.inputs(case)
    over = SC.cap_probe(x, sc, thr, ns, case["min_run"], case["gap"], case["cap"])
    finite = {k: v for k, v in over.items() if v[1]}
    print("views over the cap:", {k: v for k, v in sorted(over.items())})
    assert len(over) == 9 and len(finite) == 8, "nine of the 25 views over the cap, all but scale 1 at view 3 with finite scores"
    assert over[(1, 2)] == (24, True, True), "scale 2 at view 2: 24 candidates, a tie at rank 16"
    assert over[(0, 3)][0] == 52 and not over[(0, 3)][1], "scale 1 at view 3: 52 candidates, non-finite scores"
    assert any(not v[2] for v in finite.values()), "a capped view the device select decides"


def main() -> int:
    ref = ref_loader.load()
    if ref is None:
        print("the compiled reference is not available (make -C oracle ref)", file=sys.stderr)
        return 2
    check_cap_case()
    groups, diffs = {}, 0
    for case in SC.cases():
        want = SC.run_case(ref, case)
        if not twin_segments.same(want, SC.run_case(twin_segments, case)):
            diffs += 1
            print("twin differs from the reference:", case["name"])
        if case["n"] <= SC.TILE + 1 and not twin_segments.same(want, SC.run_case(_Loop, case)):
            diffs += 1
            print("bin-by-bin twin differs from the reference:", case["name"])
        for field, arr in SC.record(want).items():
            groups.setdefault(case["group"], {})[f"{case['name']}/{field}"] = arr
    for mod in (ref, twin_segments):
        try:
            mod.cMultiscaleCandidateSegmentStats(np.zeros(4), [1], [0.0, 1.0], [1.0])
            diffs += 1
            print("no error for different numbers of thresholds and null scales")
        except ValueError as e:
            if str(e) != "thresholds and nullScales must have the same length":
                diffs += 1
                print("other error text:", e)
    print(f"{len(SC.cases())} cases, {diffs} differences between the twin and the reference")
    if diffs:
        return 1
    for group, arrs in groups.items():
        path = os.path.join(HERE, "segments", f"segments_{group}.npz")
        os.makedirs(os.path.dirname(path), exist_ok=True)
        np.savez_compressed(path, **arrs)
        print(path, os.path.getsize(path), "bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
