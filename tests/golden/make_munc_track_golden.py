"""Regenerate tests/golden/munc_track/*.npz from the REFERENCE (build image only: `make -C oracle ref`, and the reference's source
tree for its pure-Python layer).

    python tests/golden/make_munc_track_golden.py [<reference source tree>]

The two natives, `cEvalPSplineLogVarianceTrend` and `cFinalizeMuncEBTrack`, are the compiled reference's (oracle.ref_loader).
`consenrich.core` cannot be imported there (it needs a package that is absent), so it is parsed with `ast` and only
`getMuncTrack`, `evalPSplineLogVarianceTrend`, `applyBlacklistMuncFloor` and the small pure functions they call are executed, in
a namespace that holds the reference's constants, NumPy, the compiled natives and silent stand-ins for the log helpers and the
runtime sizing (whose results the exercised branch only logs).  Nothing of the reference's text is written anywhere: the fixtures
hold OUTPUTS and error texts only, the inputs are re-synthesised from tests/munc_track_cases.py.  Every case also goes through
the twin (tests/twin_munc_track.py); the fixtures are written only if there is no difference."""
import ast
import logging
import math
import os
import sys
import types
import typing

import numpy as np
import numpy.typing as npt

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), HERE]

import munc_track_cases as MC  # noqa: E402
import twin_munc_track as T  # noqa: E402
from oracle import ref_loader  # noqa: E402

WANTED = ("getMuncTrack", "evalPSplineLogVarianceTrend", "applyBlacklistMuncFloor", "resolveMuncMinRFloor", "_muncTrendPredictor",
          "_coerceMuncCountModelVarianceFloor", "_coerceEBPriorStrength", "_normalizeMuncVarianceModel")
DIAG = ("supportCount", "supportFraction", "countFloorFiniteCount", "countFloorAddedCount", "countFloorMissingCount",
        "finalShrinkagePairCount", "finalShrinkagePairFraction")


def load_python_layer(root, natives):
    src = os.path.join(root, "src", "consenrich")
    ns = {k: getattr(typing, k) for k in ("Any", "Dict", "Iterable", "List", "Mapping", "Tuple", "Optional", "Final")}
    with open(os.path.join(src, "constants.py")) as fh:
        exec(compile(fh.read(), "constants.py", "exec"), ns)
    with open(os.path.join(src, "core.py")) as fh:
        tree = ast.parse(fh.read(), "core.py")
    body = [node for node in tree.body if isinstance(node, ast.FunctionDef) and node.name in WANTED]
    missing = set(WANTED) - {node.name for node in body}
    if missing:
        raise SystemExit(f"core.py lacks {sorted(missing)}")
    quiet = logging.getLogger("munc_track_golden")
    quiet.addHandler(logging.NullHandler())
    quiet.propagate = False
    sizing = types.SimpleNamespace(trendBlockIntervals=50, localWindowIntervals=25, trendBlockSizeBP=10000, localWindowSizeBP=5000,
                                   dependenceSpanIntervals=None)
    ns.update(np=np, npt=npt, math=math, logging=logging, logger=quiet, cconsenrich=natives, PSplineLogVarianceTrend=object,
              MuncAdditiveCovariateModel=object, _logAsciiBlock=lambda *a, **k: None,
              _resolveMuncRuntimeSizing=lambda **k: sizing, _formatMuncVarianceDiagnostics=lambda *a, **k: "",
              _formatPSplineTrendSummary=lambda *a, **k: "")
    exec(compile(ast.Module(body=body, type_ignores=[]), "core.py", "exec"), ns)
    return ns


def diag_array(d):
    return np.asarray([float(d[k]) for k in DIAG], dtype=np.float64)


def main() -> int:
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("CONSENRICH_REFERENCE", os.path.dirname(ref_loader.REF_SRC))
    ref = ref_loader.load()
    if ref is None:
        print("the compiled reference is not available (make -C oracle ref)", file=sys.stderr)
        return 2
    core = load_python_layer(root, ref)
    groups = {k: {} for k in ("eval", "final", "tracks", "blacklist")}
    diffs = count = 0

    def put(group, name, want, got):
        nonlocal diffs, count
        count += 1
        for field, arr in want.items():
            arr = np.asarray(arr)
            if not MC.same(arr, np.asarray(got[field])):
                diffs += 1
                print("twin differs from the reference:", group, name, field)
            groups[group][f"{name}/{field}"] = arr

    for case in MC.EVAL_CASES:
        trend, mean, eps, cap = MC.eval_inputs(case)
        lo, hi = T.log_bounds(eps, cap)
        pred = MC.eval_predictor(case, T)
        args = (pred, trend[0], trend[1], trend[2], trend[3], trend[4], lo, hi)
        put("eval", case[0], dict(out=ref.cEvalPSplineLogVarianceTrend(*args)), dict(out=T.cEvalPSplineLogVarianceTrend(*args)))
        # the Python layer on the float32 mean track (its own predictor)
        tr = types.SimpleNamespace(knots=trend[0], beta=trend[1], degree=trend[2], xMin=trend[3], xMax=trend[4])
        put("eval", case[0] + "/mean", dict(out=core["evalPSplineLogVarianceTrend"](tr, mean, eps=eps, maxVariance=cap)),
            dict(out=T.eval_pspline_log_variance_trend(trend, mean, eps=eps, maxVariance=cap)))
    for case in MC.FINAL_CASES:
        local, prior, floor, kw = MC.final_inputs(case)
        for eb in (True, False):
            w = ref.cFinalizeMuncEBTrack(local, prior if eb else None, floor, useEB=eb, **kw)
            g = T.cFinalizeMuncEBTrack(local, prior if eb else None, floor, useEB=eb, **kw)
            put("final", f"{case[0]}/{'eb' if eb else 'noeb'}", dict(out=w[0], diag=diag_array(w[1])), dict(out=g[0], diag=diag_array(g[1])))
    for case in MC.TRACK_CASES:
        a = MC.track_inputs(case)
        n = a["local"].shape[0]
        tr = types.SimpleNamespace(knots=a["trend"][0], beta=a["trend"][1], degree=a["trend"][2], xMin=a["trend"][3], xMax=a["trend"][4])
        w = core["getMuncTrack"]("chrT", np.arange(n, dtype=np.uint32) * 200, np.zeros(n, np.float32), 200, EB_use=a["use_eb"],
                                 eps=a["floor"], varianceFloor=a["floor"], varianceCap=a["cap"], pooledTrend=tr,
                                 priorMeanTrack=a["prior_mean"], priorVarianceTrack=a["prior_variance"],
                                 replicateVarianceFactor=a["factor"], EB_pooledNu0=a["nu0"], EB_effectiveNuL=a["nuL"],
                                 countModelVarianceFloor=a["count_floor"], localVarianceTrack=a["local"])
        g = T.get_munc_track(**a)
        put("tracks", case[0], dict(out=w[0], support=np.float64(w[1])), dict(out=g[0], support=np.float64(g[1])))
    for case in MC.BLACKLIST_CASES:
        x, mask, q = MC.blacklist_inputs(case)
        xw, xg = x.copy(), x.copy()
        fw = core["applyBlacklistMuncFloor"](xw, mask, 1.0e-12, q)
        fg = T.apply_blacklist_munc_floor(xg, mask, 1.0e-12, q)
        put("blacklist", case[0], dict(out=xw, floors=fw), dict(out=xg, floors=fg))
    texts = {}
    for name, a, k, text in MC.final_error_cases():
        for mod in (ref, T):
            try:
                mod.cFinalizeMuncEBTrack(*a, **k)
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
    out = os.path.join(HERE, "munc_track")
    os.makedirs(out, exist_ok=True)
    groups["errors"] = {k: np.asarray(v) for k, v in texts.items()}
    for group, arrs in groups.items():
        path = os.path.join(out, f"munc_track_{group}.npz")
        np.savez_compressed(path, **arrs)
        print(path, os.path.getsize(path), "bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
