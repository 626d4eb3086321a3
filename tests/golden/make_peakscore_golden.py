"""Regenerate tests/golden/peakscore/peakscore_*.npz from the REFERENCE's own functions (build image only: it needs the reference's
source tree, whose path is the first argument or $CONSENRICH_REFERENCE).

`consenrich.peaks` cannot be imported there (its `core` needs packages that are absent), so the file is parsed with `ast` and only
the five pure functions `_segmentScoreAgainstThresholdView`, `_bestSegmentScoreAcrossThresholdViews`,
`_empiricalReplaySegmentPValues`, `_replayFDRQValues` and `_thresholdViewsForNullReplay` are executed, in a namespace that holds
`np`, `npt`, `math`, `_TINY` and the typing names.  Nothing of the reference's text is written anywhere: the fixtures hold OUTPUTS
only, the inputs are re-synthesised from tests/peakscore_cases.py.  Each case also goes through both forms of the pure-Python twin
(tests/twin_peakscore.py); a fixture is written only if all three agree bit for bit on every case."""
import ast
import math
import os
import sys
import typing

import numpy as np
import numpy.typing as npt

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import peakscore_cases as PC  # noqa: E402
import twin_peakscore as T  # noqa: E402

WANTED = ("_segmentScoreAgainstThresholdView", "_bestSegmentScoreAcrossThresholdViews", "_empiricalReplaySegmentPValues",
          "_replayFDRQValues", "_thresholdViewsForNullReplay")


def load_reference(root):
    path = os.path.join(root, "src", "consenrich", "peaks.py")
    with open(path) as fh:
        tree = ast.parse(fh.read(), path)
    body = [node for node in tree.body if isinstance(node, ast.FunctionDef) and node.name in WANTED]
    missing = set(WANTED) - {node.name for node in body}
    if missing:
        raise SystemExit(f"{path} lacks {sorted(missing)}")
    ns = {k: getattr(typing, k) for k in ("Any", "Dict", "Iterable", "List", "Mapping", "Tuple", "Optional")}
    ns.update(np=np, npt=npt, math=math, _TINY=float(np.finfo(np.float64).tiny))
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)
    return ns


def segment_record(ref, case):
    x, (st, en), views = PC.track(case["n"]), PC.segments(case["n"]), PC.view_sets()[case["views"]]
    with np.errstate(all="ignore"):
        want = [ref["_bestSegmentScoreAcrossThresholdViews"](x, int(a), int(b), views) for a, b in zip(st, en)]
        steps = [T.best_score_steps(x, a, b, views) for a, b in zip(st, en)]
    live = [(k, v) for k, v in views.items() if isinstance(v, dict)]
    dev = T.details_from_arrays(T.segment_arrays_device(x, st, en, [v["threshold"] for _, v in live],
                                                        [v["null_scale"] for _, v in live]), views)
    if not (T.same_details(want, steps) and T.same_details(want, dev)):
        raise SystemExit(f"{case['name']}: the twin disagrees with the reference")
    keys = [k for k, _ in live]
    rec = {f"{case['name']}/{f}": np.asarray([w[f] for w in want], np.float64) for f in T.NUMERIC}
    rec[f"{case['name']}/view"] = np.asarray([keys.index(w["threshold_key"]) for w in want], np.int32)
    return rec


def pq_record(ref, case):
    obs, draws = PC.pq_inputs(case)
    p = ref["_empiricalReplaySegmentPValues"](obs, draws)
    q = ref["_replayFDRQValues"](obs, draws)
    pool = np.concatenate(draws) if draws else np.zeros(0)
    dp, dq, _ = T.pq_device(obs, pool, len(draws))
    for name, a, b, c in (("p", p, T.pvalues_steps(obs, draws), dp), ("q", q, T.qvalues_steps(obs, draws), dq)):
        if not (np.array_equal(T.bits(a), T.bits(b)) and np.array_equal(T.bits(a), T.bits(c))):
            raise SystemExit(f"{case['name']}: the twin's {name} values disagree with the reference")
    return {f"{case['name']}/p": np.asarray(p, np.float64), f"{case['name']}/q": np.asarray(q, np.float64)}


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("CONSENRICH_REFERENCE", "")
    if not root:
        raise SystemExit("usage: make_peakscore_golden.py <reference source tree>")
    ref = load_reference(root)
    # `_thresholdViewsForNullReplay`: thresholds relative to the null centre
    views = {"z2": dict(threshold_z=2.0, threshold=1.25, null_scale=0.5, null_center=0.25), "skip": 1}
    replay = ref["_thresholdViewsForNullReplay"](views)
    if set(replay) != {"z2"} or T.bits(replay["z2"]["threshold"]) != T.bits(1.25 - 0.25):
        raise SystemExit("`_thresholdViewsForNullReplay` is not what tests/twin_segments.py restates")
    # the scorer case (no fixture: its reference is the step-by-step twin, draw by draw) must be what the tests take it for
    scores, tmpls, scorer_views = PC.scorer_inputs()
    twin = PC.scorer_twin(scores, tmpls, scorer_views)
    facts = PC.scorer_case_facts(twin, PC.scorer_peaks(twin))
    if not all(facts.values()):
        raise SystemExit(f"the scorer case lacks {[k for k, v in facts.items() if not v]}")
    out = os.path.join(HERE, "peakscore")
    os.makedirs(out, exist_ok=True)
    seg, pq = {}, {}
    for case in PC.segment_cases():
        seg.update(segment_record(ref, case))
    for case in PC.pq_cases():
        pq.update(pq_record(ref, case))
    np.savez_compressed(os.path.join(out, "peakscore_segments.npz"), **seg)
    np.savez_compressed(os.path.join(out, "peakscore_pq.npz"), **pq)
    print(f"wrote {len(seg)} + {len(pq)} arrays to {out}")


if __name__ == "__main__":
    main()
