"""What the oracle's live comparisons with the compiled reference feed both sides, and what the reference returned.

tests/test_oracle_{golden,background,uncertainty}.py compare the oracle with the compiled reference bit for bit where its
build exists.  Everywhere else they compare it with live_reference.json: for every array the reference returned its shape
and the SHA-256 of its values (widened to float64, NaN and signed zero made canonical, so that equal digests mean
np.array_equal(..., equal_nan=True)), for every scalar its value.  make_golden.py --live writes that record from the
reference (data only)."""
from __future__ import annotations

import hashlib
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
RECORD = os.path.join(HERE, "live_reference.json")

GOLDEN_CASES = ["fb_trend_n4096_m32", "fb_level_n333_m5_mask", "ecm_trend_n600_m6_converge", "ecm_level_n1000_m3_warm_qs",
                "fb_trend_n3000_m8_apn"]
UNC_CASE = dict(name="live", m=5, n=777, block_len=20, folds=3, rho=0.15, use_lam=True, f64=False, seed=99)
FOLD_SPEC_ARGS = (5, 777, 20, 3, 0.5, 100)


def background_inputs():
    """(key, (w, r, lam, zero_center, lam_first)) of the background solves compared."""
    rng = np.random.default_rng(3)
    for n in (6, 131, 4099):
        w = np.abs(rng.normal(50, 20, n))
        r = rng.normal(0, 10, n)
        for lam_first, lam in ((0.0, 0.0), (3.0, 0.0), (0.0, 40.0), (1e3, 1e7)):
            for zc in (False, True):
                yield f"n{n}_lamfirst{lam_first:g}_lam{lam:g}_zc{int(zc)}", (w, r, lam, zc, lam_first)


def entry(v) -> dict:
    if isinstance(v, np.ndarray):
        # values, as np.array_equal compares them: exactly widened to float64, one NaN, one zero
        a = np.ascontiguousarray(v, dtype=np.float64)
        a = np.where(np.isnan(a), np.nan, np.where(a == 0, 0.0, a))
        return {"sha256": hashlib.sha256(a.tobytes()).hexdigest(), "shape": list(a.shape)}
    return {"value": float(v)}


def record(outputs: dict) -> dict:
    return {str(k): entry(v) for k, v in outputs.items()}


def load() -> dict:
    with open(RECORD) as fh:
        return json.load(fh)


def check(group: str, key: str, outputs: dict, rel: float = 1e-12) -> None:
    """outputs == what the reference returned for (group, key): arrays bit for bit, scalars within `rel`."""
    want = load()[group][key]
    got = record(outputs)
    assert set(got) == set(want), (group, key, sorted(got), sorted(want))
    for k, w in want.items():
        if "value" in w:
            assert "value" in got[k] and abs(got[k]["value"] - w["value"]) <= rel * abs(w["value"]), (group, key, k)
        else:
            assert got[k] == w, (group, key, k)
