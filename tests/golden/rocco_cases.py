"""Case table for the ROCCO natives: `csolvePenalizedChainROCCO`, `ccalibrateSelectionPenaltyROCCO` (pyx:8719-8874) and
`csolveChromROCCOExact` (pyx:8877-8958).  Inputs are re-synthesised from (gen, n, seed); the committed rocco/rocco_*.npz fixtures
(a directory of their own: tests/test_oracle_golden.py keeps a census of the *.npz files directly under tests/golden) hold
the REAL reference's outputs (tests/golden/make_rocco_golden.py), the mask as np.packbits.  Every comparison is exact."""
from __future__ import annotations

import numpy as np

TILE = 1024     # steps per LDS tile of the device kernel (csrc/csr_rocco.h ROCCO_TILE); a chain of n bins makes n - 1 steps
FIXED_N = (1, 2, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025, 1026, 2049, 2050, 4097)


def cases():
    cs = []
    # fixed penalty: Gaussian scores, penalties below / inside / above the score range
    for n in FIXED_N:
        for gamma in (0.0, 0.5, 50.0):
            for pen in (-10.0, 0.3, 10.0):
                cs.append(dict(group="fixed", name=f"fixed_n{n}_g{gamma:g}_p{pen:g}", kind="chrom", gen="gauss", n=n,
                               seed=100 + n, gamma=gamma, penalty=pen))
    for tag, s, p in (("gt", 1.5, 1.0), ("lt", 0.5, 1.0), ("eq", 1.0, 1.0)):
        cs.append(dict(group="fixed", name=f"fixed_n1_{tag}", kind="chrom", gen="literal", values=[s], n=1, seed=0,
                       gamma=0.5, penalty=p))
    cs.append(dict(group="fixed", name="fixed_nomode_n300", kind="chrom", gen="gauss", n=300, seed=5, gamma=0.5))
    # a NaN penalty is accepted by the reference: every comparison is false, nothing is selected, the penalty comes back as NaN
    for n in (1, 40):
        cs.append(dict(group="fixed", name=f"fixed_nanpen_n{n}", kind="chrom", gen="gauss", n=n, seed=6, gamma=0.5,
                       penalty=float("nan")))
    cs.append(dict(group="costs", name="costs_solve_nanpen", kind="solve", gen="gauss", n=40, seed=6, penalty=float("nan")))
    # ties: integer scores, integer / half-integer costs and penalties -- equal values occur constantly, the count rule decides
    for n in (257, 1500):
        for gamma in (0.0, 1.0, 2.0):
            for pen in (0.0, 0.5, 1.0):
                cs.append(dict(group="ties", name=f"ties_n{n}_g{gamma:g}_p{pen:g}", kind="chrom", gen="int", n=n,
                               seed=200 + n, gamma=gamma, penalty=pen))
    for gamma in (0.0, 1.0):
        for pen in (0.5, 1.0, 1.5):
            cs.append(dict(group="ties", name=f"ties_equal_g{gamma:g}_p{pen:g}", kind="chrom", gen="equal", n=100, seed=0,
                           gamma=gamma, penalty=pen))
            cs.append(dict(group="ties", name=f"ties_alt_g{gamma:g}_p{pen:g}", kind="chrom", gen="alt", n=101, seed=0,
                           gamma=gamma, penalty=pen - 1.0))
    for budget in (0.1, 0.5):
        cs.append(dict(group="ties", name=f"ties_budget{budget:g}", kind="chrom", gen="int", n=700, seed=7, gamma=1.0,
                       budget=budget, maxIter=60))
    # non-constant switch costs
    for n in (2, 33, 1025, 2049):
        cs.append(dict(group="costs", name=f"costs_solve_n{n}", kind="solve", gen="gauss", n=n, seed=300 + n, penalty=0.4))
        cs.append(dict(group="costs", name=f"costs_calib_n{n}", kind="calibrate", gen="gauss", n=n, seed=300 + n,
                       target=n // 4, maxIter=60))
    cs.append(dict(group="costs", name="costs_calib_int", kind="calibrate", gen="int", n=500, seed=9, target=60, maxIter=60))
    # calibration
    n = 1500
    for tag, budget in (("t0", 0.0), ("tn", 1.0), ("b001", 0.01), ("b03", 0.3), ("b099", 0.99), ("bneg", -0.5), ("bbig", 1.7)):
        cs.append(dict(group="calib", name=f"calib_{tag}", kind="chrom", gen="gauss", n=n, seed=41, gamma=0.5, budget=budget,
                       maxIter=60))
    for it in (0, 1, 7, 60, 100):
        cs.append(dict(group="calib", name=f"calib_iter{it}", kind="chrom", gen="gauss", n=n, seed=42, gamma=0.5, budget=0.3,
                       maxIter=it))
    cs.append(dict(group="calib", name="calib_n1", kind="chrom", gen="literal", values=[0.7], n=1, seed=0, gamma=0.5,
                   budget=0.5, maxIter=60))
    cs.append(dict(group="calib", name="calib_n4097", kind="chrom", gen="gauss", n=4097, seed=43, gamma=0.5, budget=0.03,
                   maxIter=60))
    # the expansion loop runs: lower = 1e17 - 0 - 1 rounds onto scoreMin, so lowerCount = 1 <= target
    cs.append(dict(group="calib", name="calib_expand", kind="calibrate", gen="literal", values=[1e17, 2e17], n=2, seed=0,
                   costs=[0.0], target=1, maxIter=60))
    return cs


def inputs(case):
    """(scores, switchCosts or None) of a case."""
    n, rng = case["n"], np.random.default_rng(case["seed"])
    if case["gen"] == "gauss":
        s = rng.normal(0.0, 1.0, n)
    elif case["gen"] == "int":
        s = rng.integers(-2, 4, n).astype(np.float64)
    elif case["gen"] == "equal":
        s = np.full(n, 1.0)
    elif case["gen"] == "alt":
        s = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    else:
        s = np.asarray(case["values"], np.float64)
    costs = None
    if case["kind"] != "chrom":
        if "costs" in case:
            costs = np.asarray(case["costs"], np.float64)
        elif case["gen"] == "int":
            costs = rng.integers(0, 3, max(n - 1, 0)).astype(np.float64)
        else:
            costs = 0.7 * np.abs(rng.normal(0.0, 1.0, max(n - 1, 0)))
    return s, costs


def run_case(mod, case):
    """The callable of `mod` the case names, on the case's inputs -> dict of arrays (mask packed)."""
    s, costs = inputs(case)
    if case["kind"] == "solve":
        sol, val, cnt = mod.csolvePenalizedChainROCCO(s, costs, case["penalty"])
        obj, pen = 0.0, case["penalty"]
    elif case["kind"] == "calibrate":
        pen, sol, val, cnt = mod.ccalibrateSelectionPenaltyROCCO(s, costs, case["target"], case["maxIter"])
        obj = 0.0
    else:
        sol, obj, val, cnt, pen = mod.csolveChromROCCOExact(s, budget=case.get("budget"), gamma=case["gamma"],
                                                            selectionPenalty=case.get("penalty"),
                                                            maxIter=case.get("maxIter", 60))
    sol = np.asarray(sol)
    assert sol.dtype == np.uint8 and sol.shape == (case["n"],)
    assert type(val) is float and type(cnt) is int and type(pen) is float
    return dict(mask=np.packbits(sol), floats=np.asarray([obj, val, pen], np.float64), count=np.asarray([cnt], np.int64))


def same(a, b):
    """Bit equality of two run_case results (floats compared as their 64-bit patterns)."""
    return (np.array_equal(a["mask"], b["mask"]) and np.array_equal(a["count"], b["count"]) and
            np.array_equal(np.asarray(a["floats"], np.float64).view(np.uint64), np.asarray(b["floats"], np.float64).view(np.uint64)))


def load_group(path):
    """{case name: result} of one rocco_<group>.npz."""
    out = {}
    with np.load(path) as z:
        for key in z.files:
            name, field = key.rsplit("/", 1)
            out.setdefault(name, {})[field] = z[key]
    return out
