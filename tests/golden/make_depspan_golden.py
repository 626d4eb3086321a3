"""Regenerate tests/golden/depspan/depspan_*.npz from the COMPILED REFERENCE (`make -C oracle ref`; build image only).

    python tests/golden/make_depspan_golden.py

Every case of tests/depspan_cases.py runs through the reference's `cconsenrich.cchooseDependenceSpan`, through the FFT twin and
through the truth twin (tests/twin_depspan.py).  A fixture is written only if the FFT twin equals the reference on every discrete
field, on the scores, ranks, radii and bootstrap lists (exactly) and within 1e-12 on the continuous ones, and if the smallest
margin of the case -- the smallest |smoothed ACF - threshold| at a lag a persistence scan examined -- is at least 1e-9: the
decisions of such a case do not hang on the rounding of the lag sums.

A fixture holds the reference's result (JSON; floats round-trip exactly), the SHA-256 of the input bytes, and
  e_ref          the largest |pooled ACF (FFT route) - pooled ACF (truth)| over the evaluated windows,
  e_strength     the same for `oscillationStrength`, e_revival for `postCrossingRevival` (reference against the truth twin),
  min_margin     the smallest margin.
The error fixtures hold the reference's texts."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), HERE]

import depspan_cases as DC  # noqa: E402
import twin_depspan as T  # noqa: E402
from oracle import ref_loader  # noqa: E402

OUT = os.path.join(HERE, "depspan")


def main() -> int:
    ref = ref_loader.load()
    if ref is None:
        print("the compiled reference is not available (make -C oracle ref)", file=sys.stderr)
        return 2
    os.makedirs(OUT, exist_ok=True)
    bad, worst_e = 0, 0.0
    for case in DC.cases():
        names, mats = DC.build_any(case)
        want = T.strip(ref.cchooseDependenceSpan(names, mats, case["interval"], **case["kw"]))
        want = json.loads(json.dumps(want))
        fft, fb = T.run(names, mats, case["interval"], route="fft", **case["kw"])
        truth, tb = T.run(names, mats, case["interval"], route="truth", **case["kw"])
        fft, truth = json.loads(json.dumps(T.strip(fft))), json.loads(json.dumps(T.strip(truth)))
        diffs = T.discrete_differences(want, fft) + [f"truth: {d}" for d in T.discrete_differences(want, truth)]
        for field in T.CONTINUOUS_WINDOW:
            if T.continuous_error(want, fft, field) > 1.0e-12:
                diffs.append(f"{field}: the FFT twin is {T.continuous_error(want, fft, field)} from the reference")
        e_ref, min_margin = 0.0, np.inf
        for key, rec in fb.windows.items():
            other = tb.windows[key]
            both = np.isfinite(rec["pooled"]) & np.isfinite(other["pooled"])
            if np.any(both):
                e_ref = max(e_ref, float(np.max(np.abs(rec["pooled"][both] - other["pooled"][both]))))
            if rec["status"]:
                min_margin = min(min_margin, float(rec["margin"]))
        if min_margin < 1.0e-9:
            diffs.append(f"smallest margin {min_margin} is below 1e-9")
        e_strength = T.continuous_error(want, truth, "oscillationStrength")
        e_revival = T.continuous_error(want, truth, "postCrossingRevival")
        d = want[3]
        print(f"{case['name']}: candidates {d['candidateWindowCount']} evaluated {d['evaluatedCandidateWindowCount']} selected "
              f"{d['selectedWindowCount']} censored {d['rightCensoredWindowCount']} (support {d['supportCensoredWindowCount']}, "
              f"maxLag {d['capCensoredWindowCount']}) unique rows {d['uniqueRowCount']}/{d['inputRowCount']} tuple {want[:3]} "
              f"E_ref {e_ref:.3g} E_strength {e_strength:.3g} E_revival {e_revival:.3g} min margin {min_margin:.3g}")
        if diffs:
            bad += 1
            print("  NOT WRITTEN:", *diffs[:12], sep="\n    ")
            continue
        worst_e = max(worst_e, e_ref)
        np.savez_compressed(os.path.join(OUT, f"depspan_{case['name']}.npz"), result=np.asarray(json.dumps(want)),
                            sha=np.asarray(DC.input_sha(mats)), e_ref=np.float64(e_ref), e_strength=np.float64(e_strength),
                            e_revival=np.float64(e_revival), min_margin=np.float64(min_margin))
    texts = {}
    for name, names, mats, interval, kw, text in DC.value_error_cases():
        for mod, fn in (("reference", ref.cchooseDependenceSpan), ("twin", T.fft_twin)):
            try:
                fn(names if names is not None else 5, mats, interval, **kw)
                bad += 1
                print("no error:", name, mod)
            except ValueError as e:
                if str(e) != text:
                    bad += 1
                    print("other error text:", name, mod, e)
                if mod == "reference":
                    texts[name] = str(e)
    for case, text in DC.runtime_error_cases():
        for mod, fn in (("reference", ref.cchooseDependenceSpan), ("twin", T.fft_twin)):
            try:
                DC.call(fn, case)
                bad += 1
                print("no error:", case["name"], mod)
            except RuntimeError as e:
                if text not in str(e):
                    bad += 1
                    print("other error text:", case["name"], mod, e)
                if mod == "reference":
                    texts[case["name"]] = str(e)
    print(f"{len(DC.cases())} cases, {len(texts)} errors, {bad} refused; largest E_ref {worst_e:.3g}")
    if bad:
        return 1
    np.savez_compressed(os.path.join(OUT, "depspan_errors.npz"), **{k: np.asarray(v) for k, v in texts.items()})
    return 0


if __name__ == "__main__":
    sys.exit(main())
