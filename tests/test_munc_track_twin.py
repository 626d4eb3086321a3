"""The twin of the finished-track stages (tests/twin_munc_track.py) against the compiled reference's fixtures
(tests/golden/munc_track), the host work on the block records (`munc_track.pooled_block_rows`) against the twin's own block loop,
the error texts, and the loud failure without a device.  No GPU."""
import os

import numpy as np
import pytest

import munc_track_cases as MC
import twin_munc_track as T
from consenrich_amd import _lib as L
from consenrich_amd import cconsenrich as cc
from consenrich_amd import munc_track as MT

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "munc_track")
DIAG = ("supportCount", "supportFraction", "countFloorFiniteCount", "countFloorAddedCount", "countFloorMissingCount",
        "finalShrinkagePairCount", "finalShrinkagePairFraction")


@pytest.fixture(scope="module")
def gold():
    g = {}
    for group in ("eval", "final", "tracks", "blacklist", "errors"):
        with np.load(os.path.join(GOLD, f"munc_track_{group}.npz")) as z:
            g[group] = {k: z[k] for k in z.files}
    return g


def test_fixtures_cover_the_case_table(gold):
    assert set(gold["eval"]) == {f"{c[0]}/out" for c in MC.EVAL_CASES} | {f"{c[0]}/mean/out" for c in MC.EVAL_CASES}
    assert set(gold["final"]) == {f"{c[0]}/{eb}/{f}" for c in MC.FINAL_CASES for eb in ("eb", "noeb") for f in ("out", "diag")}
    assert set(gold["tracks"]) == {f"{c[0]}/{f}" for c in MC.TRACK_CASES for f in ("out", "support")}
    assert set(gold["blacklist"]) == {f"{c[0]}/{f}" for c in MC.BLACKLIST_CASES for f in ("out", "floors")}
    assert set(gold["errors"]) == {c[0] for c in MC.final_error_cases()}


@pytest.mark.parametrize("case", MC.EVAL_CASES, ids=[c[0] for c in MC.EVAL_CASES])
def test_trend_twin_equals_reference(gold, case):
    trend, mean, eps, cap = MC.eval_inputs(case)
    lo, hi = T.log_bounds(eps, cap)
    got = T.cEvalPSplineLogVarianceTrend(MC.eval_predictor(case, T), trend[0], trend[1], trend[2], trend[3], trend[4], lo, hi)
    assert MC.same(gold["eval"][f"{case[0]}/out"], got)
    assert MC.same(gold["eval"][f"{case[0]}/mean/out"], T.eval_pspline_log_variance_trend(trend, mean, eps=eps, maxVariance=cap))
    assert (MT.log_bounds(eps, cap)) == (lo, hi)
    assert MC.same(MT.munc_trend_predictor(mean), T.predictor(mean))


def test_trend_cases_reach_both_log_bounds_and_the_knots(gold):
    out = gold["eval"]["deg2_clamps/out"]
    assert np.any(out == np.float32(0.5)) and np.any(out == np.float32(0.75)) and np.any((out > 0.5) & (out < 0.75))
    assert np.all(gold["eval"]["const_beta_inf/out"] == np.float32(9.0))
    assert np.any(gold["eval"]["deg3_beta_posinf/out"] == np.float32(MC.F32_MAX))
    assert gold["eval"]["deg3_n0/out"].shape == (0,)


@pytest.mark.parametrize("case", MC.FINAL_CASES, ids=[c[0] for c in MC.FINAL_CASES])
@pytest.mark.parametrize("eb", (True, False), ids=("eb", "noeb"))
def test_finalisation_twin_equals_reference(gold, case, eb):
    local, prior, floor, kw = MC.final_inputs(case)
    out, diag = T.cFinalizeMuncEBTrack(local, prior if eb else None, floor, useEB=eb, **kw)
    key = f"{case[0]}/{'eb' if eb else 'noeb'}"
    assert MC.same(gold["final"][f"{key}/out"], out)
    assert MC.same(gold["final"][f"{key}/diag"], np.asarray([float(diag[k]) for k in DIAG]))


def test_subnormal_values_survive(gold):
    out = gold["final"]["subnormal/noeb/out"]
    assert 0.0 < out[0] < np.finfo(np.float32).tiny and 0.0 < gold["final"]["subnormal/eb/out"][0] < np.finfo(np.float32).tiny


@pytest.mark.parametrize("case", MC.TRACK_CASES, ids=[c[0] for c in MC.TRACK_CASES])
def test_track_twin_equals_reference(gold, case):
    out, support, _diag = T.get_munc_track(**MC.track_inputs(case))
    assert MC.same(gold["tracks"][f"{case[0]}/out"], out)
    assert MC.same(gold["tracks"][f"{case[0]}/support"], np.float64(support))


@pytest.mark.parametrize("case", MC.BLACKLIST_CASES, ids=[c[0] for c in MC.BLACKLIST_CASES])
def test_blacklist_floor_twin_equals_reference(gold, case):
    x, mask, q = MC.blacklist_inputs(case)
    floors = T.apply_blacklist_munc_floor(x, mask, 1.0e-12, q)
    assert MC.same(gold["blacklist"][f"{case[0]}/out"], x)
    assert MC.same(gold["blacklist"][f"{case[0]}/floors"], floors)


def test_a_quantile_falls_between_two_order_statistics(gold):
    x, mask, q = MC.blacklist_inputs(next(c for c in MC.BLACKLIST_CASES if c[0] == "between_two"))
    row = np.sort(x[0][mask == 0])
    fl = gold["blacklist"]["between_two/floors"][0]
    assert fl not in row.astype(np.float64) and row[0] < fl < row[-1]


def test_error_texts(gold):
    for name, a, k, text in MC.final_error_cases():
        assert str(gold["errors"][name]) == text
        with pytest.raises(ValueError) as e:
            T.cFinalizeMuncEBTrack(*a, **k)
        assert str(e.value) == text


def test_parameter_errors_of_the_drop_ins_come_before_any_device_call(monkeypatch):
    """The checks the reference makes before its loop, in its order, need no device."""
    monkeypatch.setattr(L, "device_count", lambda: 0)
    assert cc.cFinalizeMuncEBTrack is MT.cFinalizeMuncEBTrack and cc.cEvalPSplineLogVarianceTrend is MT.cEvalPSplineLogVarianceTrend
    assert "cFinalizeMuncEBTrack" in cc.__all__ and "cEvalPSplineLogVarianceTrend" in cc.__all__
    for name, a, k, text in MC.final_error_cases():
        if name.startswith(("bad_", "two_", "three_", "prior_and", "no_eb_bad")):
            continue
        with pytest.raises(ValueError) as e:
            MT.cFinalizeMuncEBTrack(*a, **k)
        assert str(e.value) == text, name
    local = np.ones(5, np.float32)
    kw = dict(intervalSizeBP=200, localVarianceTrack=local, eps=1.0e-6)
    iv, vals = np.arange(5) * 200, np.zeros(5, np.float32)
    for extra, text in ((dict(replicateVarianceFactor=0.0), "replicateVarianceFactor must be positive and finite"),
                        (dict(muncVarianceModel="garch"), "unsupported MUNC variance model 'garch'; expected kalman"),
                        (dict(localVarianceTrack=None), "kalman MUNC requires localVarianceTrack"),
                        (dict(countModelVarianceFloor=np.full(5, -1.0)), "countModelVarianceFloor must be nonnegative where finite")):
        with pytest.raises(ValueError) as e:
            MT.get_munc_track("chrT", iv, vals, **dict(kw, **extra))
        assert str(e.value) == text
    for trend, text in (((np.zeros(20), np.zeros(8), 6, 0.0, 1.0), "degree 6"), ((np.zeros(700), np.zeros(600), 3, 0.0, 1.0), "600 basis"),
                        ((np.zeros(9), np.zeros(8), 3, 0.0, 1.0), "do not describe")):
        with pytest.raises(ValueError, match=text):
            MT.cEvalPSplineLogVarianceTrend(np.zeros(4), trend[0], trend[1], trend[2], trend[3], trend[4], -10.0, 10.0)
    with pytest.raises(ValueError, match="muncMatrix must be one- or two-dimensional"):
        MT.apply_blacklist_munc_floor(np.zeros((2, 2, 2), np.float32), np.zeros(2), 0.0)
    with pytest.raises(ValueError, match="blacklistMask length must match MUNC track length"):
        MT.apply_blacklist_munc_floor(np.zeros((2, 3), np.float32), np.zeros(2), 0.0)
    with pytest.raises(NotImplementedError):
        MT.apply_blacklist_munc_floor(np.zeros((2, 3), np.float32), np.ones(3), -1.0)
    assert MT.apply_blacklist_munc_floor(np.ones((2, 3), np.float32), np.zeros(3), 0.25).tolist() == [0.25, 0.25]   # no mask: no device


def test_no_device_fails_loudly(monkeypatch):
    """Without a device the drop-ins raise the library's error; nothing is computed on the host instead."""
    monkeypatch.setattr(L, "device_count", lambda: 0)
    local, prior, floor, kw = MC.final_inputs(MC.FINAL_CASES[0])
    trend, mean, eps, cap = MC.eval_inputs(MC.EVAL_CASES[0])
    x, mask, q = MC.blacklist_inputs(MC.BLACKLIST_CASES[2])
    a = MC.track_inputs(MC.TRACK_CASES[0])
    n = a["local"].shape[0]
    for call in (lambda: MT.cFinalizeMuncEBTrack(local, prior, floor, **kw),
                 lambda: MT.cEvalPSplineLogVarianceTrend(T.predictor(mean), trend[0], trend[1], trend[2], trend[3], trend[4], -10.0, 10.0),
                 lambda: MT.eval_pspline_log_variance_trend(trend, mean, eps=eps, maxVariance=cap),
                 lambda: MT.apply_blacklist_munc_floor(x, mask, 1.0e-12, q),
                 lambda: MT.get_munc_track("chrT", np.arange(n) * 200, np.zeros(n, np.float32), 200, localVarianceTrack=a["local"],
                                           pooledTrend=a["trend"], priorMeanTrack=a["prior_mean"], EB_pooledNu0=a["nu0"],
                                           EB_effectiveNuL=a["nuL"], eps=a["floor"])):
        with pytest.raises(L.ConsenrichAMDError, match="no CPU fallback"):
            call()


# -- the host work on the block records ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block_len", MC.BLOCK_LENGTHS)
def test_pooled_block_rows_equal_the_twins_loop(block_len):
    """`pooled_block_rows` sees the raw sums only (what the device hands back) and must reproduce what the reference's loop makes
    of them: the two quotients, the effective support, the validity mask and the pooled rows in the reference's order."""
    lens = (5 * block_len + 1, 3 * block_len + 2)       # a dropped last block of length 1, a kept one of length 2
    loops = [T.block_loop(*MC.block_chain(3, n, 800 + n, block_len), block_len, multiplier=2.0) for n in lens]
    assert loops[0]["raw"]["starts"].size == 5 and loops[1]["raw"]["starts"].size == (4 if block_len == 2 else 4)
    want = T.pooled_rows([loops[0], None, loops[1]], MC.planted_trigamma, chain_index=[4, 5, 9])
    got = MT.pooled_block_rows([loops[0]["raw"], None, loops[1]["raw"]], chain_index=[4, 5, 9], dependence_multiplier=2.0,
                               trigamma=MC.planted_trigamma)
    for key in ("means", "variances", "log_variance_noise", "sample_index", "chrom_index", "block_starts", "trend_weights"):
        assert MC.same(want[key], got[key]), key
    assert want["row_counts"] == got["row_counts"] and got["chains"][1] is None
    for c, lp in ((0, loops[0]), (2, loops[1])):
        for key in ("predictor", "evidence", "weight", "support"):
            assert MC.same(lp[key], got["chains"][c][key]), key
    assert want["means"].size > 0 and set(want["chrom_index"].tolist()) == {4, 9}
    s, e = MT.block_layout(lens[0], block_len)
    assert np.array_equal(s, loops[0]["raw"]["starts"]) and np.array_equal(e, loops[0]["raw"]["ends"])


def test_block_cases_hold_what_they_are_for():
    lp = T.block_loop(*MC.block_chain(3, 8 * 9 + 2, 801, 9), 9)
    raw = lp["raw"]
    assert raw["included"][0] == 0 and np.all(raw["valid"][:, 0] == 0)          # a block with every cell excluded
    assert np.all(raw["valid"][:, 1] == 0) and raw["included"][1] > 0            # a block whose weights are all zero
    assert np.all(raw["valid"][:, 2] <= raw["included"][2] - 2 + 2)              # the NaN and the infinite mean drop their cells
    assert np.all(np.isnan(lp["predictor"][:, :2])) and np.all(lp["support"][:, :2] == 0.0)


def test_default_trigamma_is_scipys_and_injectable():
    pytest.importorskip("scipy")
    from scipy.special import polygamma

    x = np.array([2.0, 2.5, 7.0, 100.0])
    assert MC.same(np.asarray(MT.default_trigamma(x), np.float64), np.asarray(polygamma(1, x), np.float64))
    lp = T.block_loop(*MC.block_chain(2, 41, 802, 8), 8)
    a = MT.pooled_block_rows([lp["raw"]])
    b = MT.pooled_block_rows([lp["raw"]], trigamma=lambda v: polygamma(1, v))
    assert MC.same(a["log_variance_noise"], b["log_variance_noise"]) and a["log_variance_noise"].size > 0
