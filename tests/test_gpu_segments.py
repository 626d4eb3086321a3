"""GPU tests of the multiscale candidate segments on the device (run with -m gpu).  Every float is compared by its 64-bit
pattern, every integer with ==.  References: the compiled reference's recorded outputs (tests/golden/segments/segments_*.npz) for
the native's case table and the per-view cap; the pure-Python twin (tests/twin_segments.py, pinned to those recordings by
tests/test_segments_twin.py) for the Python composition and, draw by draw on tests/twin_dwb.py's draws, for the null replays."""
import ctypes as C
import os

import numpy as np
import pytest

import cases
import segments_cases as SC
import twin_dwb
import twin_segments as T
from conftest import gpu_available

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(SC.__file__)), "segments")


@pytest.fixture(scope="module")
def product():
    if not gpu_available():
        pytest.fail("GPU tests selected but no HIP device / library: the product has no CPU fallback")
    from consenrich_amd import cconsenrich

    assert hasattr(cconsenrich, "cMultiscaleCandidateSegmentStats")
    return cconsenrich


@pytest.fixture(scope="module")
def golden():
    out = {}
    for g in SC.GROUPS:
        out.update(SC.load_group(os.path.join(GOLDEN, f"segments_{g}.npz")))
    return out


def _bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


# ---------------------------------------------------------------------------------------------------------------
# 1. the case table against the reference's recordings
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", ["table", "special"])
def test_case_table_equals_the_reference(product, golden, group):
    """table: n = 1, 2, around the walk's 64-value fetch and its 256-value tile, one past two tiles, one past 8 and 16 steps of a
    job's 1024-bin scan, x (minRun, gap) = (1, 0), (3, 2), (0, -1), scales (1, 2, 5, 17, n), five views of which the fourth has
    a null scale that clamps to DBL_MIN (inf and NaN propagate).  special: a scale of 0, a repeated one and one beyond n; a
    constant track at a threshold; a track below every threshold; a run that ends in the last bin; a gap wider than the track;
    n = 0, no views, no scales."""
    bad = {}
    for c in SC.cases():
        if c["group"] == group:
            d = SC.differences(SC.run_case(product, c), golden[c["name"]])
            if d:
                bad[c["name"]] = d
    assert bad == {}


def test_the_length_mismatch_is_the_references_error(product):
    with pytest.raises(ValueError, match="^thresholds and nullScales must have the same length$"):
        product.cMultiscaleCandidateSegmentStats(np.zeros(4), [1], [0.0, 1.0], [1.0])


# ---------------------------------------------------------------------------------------------------------------
# 2. the per-view cap: device select, and NumPy on the host for the views the values do not decide
# ---------------------------------------------------------------------------------------------------------------
def test_cap_equals_the_reference_with_both_paths_taken(product, golden):
    """n = 8193, cap 16: nine of the 25 views are over the cap; scale 2 at view 2 (24 candidates) ties at rank 16 and scale 1 at
    view 3 (52 candidates) has non-finite scores -- both go to NumPy on the host; the others are decided by the device select."""
    from consenrich_amd import segments

    case = next(c for c in SC.cases() if c["name"] == "cap16_n8193")
    got = SC.run_case(product, case)
    stats = segments.last_run_stats()
    print("capped views", stats["capped_views"], "fallback views", stats["fallback_views"])
    assert SC.differences(got, golden[case["name"]]) == []
    assert stats["capped_views"] == int(got[9]) == 9
    assert stats["fallback_views"] >= 2
    assert stats["fallback_views"] < stats["capped_views"]
    for name in ("cap16_n8193_run3_gap2", "cap1_n513"):
        case = next(c for c in SC.cases() if c["name"] == name)
        assert SC.differences(SC.run_case(product, case), golden[name]) == [], name


# ---------------------------------------------------------------------------------------------------------------
# 3. the Python composition against the twin
# ---------------------------------------------------------------------------------------------------------------
def _views(null_scales=(1.3, 1.3, 0.05, 0.7, 2.0)):
    return {f"z{z:g}": dict(threshold_z=z, threshold=t, null_scale=s, null_center=SC.CENTER)
            for z, t, s in zip(SC.Z, SC.THRESHOLDS, null_scales)}


def test_multiscale_candidates_equals_the_twin_with_a_total_cap_that_binds(product):
    from consenrich_amd import segments

    x = SC.scores(SC.CAP_N)
    views = _views()
    views["not a view"] = 3.0       # skipped, as in the reference
    for kw in (dict(scale_bins=(1, 2, 5, 5, 17, 10 ** 6), max_segments=40, max_segments_per_view=16),
               dict(scale_bins=None, max_segments=40, max_segments_per_view=0, min_run_bins=3, max_gap_bins=2),
               dict(scale_bins=(2,), max_segments=None, max_segments_per_view=None)):
        got = segments.multiscale_candidates(x, views, **kw)
        ref = T.multiscale_candidates(x, {k: v for k, v in views.items() if isinstance(v, dict)}, **kw)
        assert T.same_candidates(got, ref), kw
    got = segments.multiscale_candidates(x, views, scale_bins=(1, 2, 5, 5, 17, 10 ** 6), max_segments=40, max_segments_per_view=16)
    assert got[1]["total_cap_hit"] and got[1]["candidate_count"] == 40 and got[1]["per_view_cap_hit_count"] > 0


# ---------------------------------------------------------------------------------------------------------------
# 4. null replays: a third phase of the DWB panel
# ---------------------------------------------------------------------------------------------------------------
LENS = (129, 8193, 16385)
BWS = (2, 17, 5)
CENTERS = (0.25, -0.5, 1.0)
SCALES = (0.8, 1.5, 0.05)
Z_GRID = (0.0, 1.5, 2.0, 2.5, 3.0)
SEED, B, R = 21, 9, 8
VIEW_CAP, TOTAL_CAP = 16, 60


def _inputs():
    rng = np.random.default_rng(404)
    scores = [rng.normal(CENTERS[c], 1.3, n) for c, n in enumerate(LENS)]
    tmpls = [rng.normal(0.0, 1.0, n) * (1.0 + 0.5 * np.sin(np.arange(n) / 50.0)) for n in LENS]
    return scores, tmpls


def _twin_replays(scores, tmpls, views, bws, seed, scale_bins=None, min_run=1, gap=0):
    """Per chain: observed (candidates, diagnostics) and, draw by draw, what the replay loop of the reference computes."""
    strides = [t.shape[0] + 2 * twin_dwb.max_lag(max(bw, 2), 0) for t, bw in zip(tmpls, bws)]
    noise = twin_dwb.stream(seed, R * max(strides))
    out = []
    for c, t in enumerate(tmpls):
        vw = {str(i): v for i, v in enumerate(views[c])}
        rv = {k: dict(threshold_z=v["threshold_z"], threshold=float(v["threshold"] - v["null_center"]), null_scale=v["null_scale"])
              for k, v in vw.items()}
        sc = T.resolve_scales(t.shape[0], scale_bins, bws[c])
        kw = dict(scale_bins=sc, min_run_bins=min_run, max_gap_bins=gap, max_segments=TOTAL_CAP, max_segments_per_view=VIEW_CAP)
        reps = []
        for b in range(R):
            draw = twin_dwb.draw_fast(t, max(bws[c], 2), noise[b * strides[c]:(b + 1) * strides[c]], "bartlett")
            reps.append(T.multiscale_candidates(draw, rv, **kw))
        out.append(dict(observed=T.multiscale_candidates(scores[c], vw, **kw), replays=reps, scale_bins=sc))
    return out


def _same_replays(got, ref):
    bad = []
    for c in range(len(ref)):
        if got[c]["scale_bins"] != ref[c]["scale_bins"]:
            bad.append((c, "scale_bins"))
        if not T.same_candidates(got[c]["observed"], ref[c]["observed"]):
            bad.append((c, "observed"))
        for b, (cands, diag) in enumerate(ref[c]["replays"]):
            g = got[c]["replays"][b]
            if g["candidate_count"] != len(cands) or g["diagnostics"] != diag:
                bad.append((c, b, "count / diagnostics"))
            for key in ("score", "integrated_excess", "max_excess"):
                if not np.array_equal(_bits(g[key]), _bits([k[key] for k in cands])):
                    bad.append((c, b, key))
    return bad


@pytest.fixture(scope="module")
def panel_views(product):
    """per-chain views from a stationary_null_panel run (B = 9)"""
    from consenrich_amd import dwb

    scores, tmpls = _inputs()
    return dwb.stationary_null_panel(scores, tmpls, CENTERS, SCALES, threshold_z_grid=Z_GRID, bandwidths=BWS, num_bootstrap=B,
                                     random_seed=SEED)


@pytest.fixture(scope="module")
def reference_replays(panel_views):
    scores, tmpls = _inputs()
    return _twin_replays(scores, tmpls, panel_views, BWS, SEED)


@pytest.mark.parametrize("group", [1, 7, 9])
def test_null_replays_equal_the_twin_draw_by_draw(product, panel_views, reference_replays, group):
    """Three chains of different length and bandwidth, per-chain scales (from the bandwidth) and views (from the panel), the
    first 8 draws of the seed's stream; groups of 1, 7 (a last group of one) and 9 (all at once) give the same."""
    from consenrich_amd import dwb

    scores, tmpls = _inputs()
    got = dwb.null_replay_candidates(scores, tmpls, panel_views, bandwidths=BWS, num_replay=R, random_seed=SEED,
                                     max_segments=TOTAL_CAP, max_segments_per_view=VIEW_CAP, draws_per_group=group)
    assert _same_replays(got, reference_replays) == []
    assert got[0]["draws_per_group"] == min(group, R)
    assert any(r["diagnostics"]["per_view_cap_hit_count"] > 0 for c in got for r in c["replays"])
    assert any(r["diagnostics"]["total_cap_hit"] for c in got for r in c["replays"])


def test_replays_of_a_batch_read_the_resident_scores_and_change_nothing(product):
    from consenrich_amd import _lib as L
    from consenrich_amd.batch import DeviceBatch, ModelParams

    n_list, m = [3000, 65, 9000], 3
    names = ("D", "xf", "Pf", "pnoise", "xs", "Ps", "lag")
    rng = np.random.default_rng(77)
    tmpls = [rng.normal(0.0, 1.0, n) for n in n_list]
    centers, scales, bws = [0.0, 0.1, -0.2], [1.0, 0.5, 2.0], [3, 2, 9]
    with DeviceBatch(0) as b:
        b.configure(ModelParams(state_dim=2), m, n_list)
        for c, n in enumerate(n_list):
            b.upload(c, *cases.synth(n, m, 4500 + c))
        b.stats()
        b.forward_backward(L.RETURN_NLL)
        b.export(L.EXPORT_FORWARD | L.EXPORT_SMOOTH)
        b.rocco_scores("state")
        before = {(c, a): b.download(c, a) for c in range(len(n_list)) for a in names}
        scores = [b.download_scores(c) for c in range(len(n_list))]
        rocco_before = b.rocco(budget=0.1, gamma=0.5)
        masks_before = [b.rocco_solution(c) for c in range(len(n_list))]
        views = b.dwb_panel(tmpls, centers, scales, threshold_z_grid=Z_GRID[1:], bandwidths=bws, num_bootstrap=B, random_seed=3)
        ref = _twin_replays(scores, tmpls, views, bws, 3, min_run=2, gap=1)
        # the observed side alone ...
        obs = b.segment_candidates(views, dependence_spans=bws, min_run_bins=2, max_gap_bins=1, max_segments=TOTAL_CAP,
                                   max_segments_per_view=VIEW_CAP)
        for c in range(len(n_list)):
            assert T.same_candidates(obs[c], ref[c]["observed"]), c
        # ... and with the replays
        got = b.dwb_replay(tmpls, views, bandwidths=bws, num_replay=R, random_seed=3, min_run_bins=2, max_gap_bins=1,
                           max_segments=TOTAL_CAP, max_segments_per_view=VIEW_CAP)
        assert _same_replays(got, ref) == []
        for (c, a), v in before.items():
            assert np.array_equal(b.download(c, a).view(np.uint32), v.view(np.uint32)), (c, a)
        for c in range(len(n_list)):
            assert np.array_equal(_bits(b.download_scores(c)), _bits(scores[c]))
            assert np.array_equal(b.rocco_solution(c), masks_before[c])
        rocco_after = b.rocco(budget=0.1, gamma=0.5)
        for c in range(len(n_list)):
            assert rocco_after[c]["selected_count"] == rocco_before[c]["selected_count"]
            assert np.array_equal(_bits([rocco_after[c][k] for k in ("objective", "penalized_objective", "selection_penalty")]),
                                  _bits([rocco_before[c][k] for k in ("objective", "penalized_objective", "selection_penalty")]))
            assert np.array_equal(b.rocco_solution(c), masks_before[c])
    with DeviceBatch(0) as b:
        b.configure(ModelParams(state_dim=2), 2, [10])
        with pytest.raises(L.ConsenrichAMDError, match="has no scores"):
            b.segment_candidates([_views()])


# ---------------------------------------------------------------------------------------------------------------
# 5. the C ABI
# ---------------------------------------------------------------------------------------------------------------
def test_the_c_abi_answers_value_errors_before_any_launch_and_keeps_its_phases_in_order(product):
    from consenrich_amd import _lib as L
    from consenrich_amd.batch import DeviceBatch, ModelParams

    lib = L.lib()
    x, sc = SC.scores(300), np.array([1, 2], np.int64)
    thr, ns = np.array(SC.THRESHOLDS[:2]), np.array([1.0, 1.0])
    rows, cnt, fl = np.zeros(1, np.int64), np.zeros(3, np.int64), C.c_int32(0)
    i64 = lambda a: a.ctypes.data_as(L.I64P)  # noqa: E731
    i32 = lambda a: a.ctypes.data_as(L.I32P)  # noqa: E731
    assert lib.csr_segments_run(None, L.dp(x), 300, 2, i64(sc), 2, L.dp(thr), 1, L.dp(ns), 1, 0, 0, i64(rows), i64(cnt),
                                C.byref(fl)) == L.SEG_ERR_VALUE
    assert L.last_error() == "thresholds and nullScales must have the same length"
    # n, scale count or view count <= 0: no rows, zero counters
    rows[:], cnt[:] = 7, 7
    assert lib.csr_segments_run(None, L.dp(x), 0, 2, i64(sc), 2, L.dp(thr), 2, L.dp(ns), 1, 0, 0, i64(rows), i64(cnt), C.byref(fl)) == 0
    assert rows[0] == 0 and list(cnt) == [0, 0, 0] and fl.value == 0
    assert lib.csr_segments_fetch(None, None, None, None, None, None, None, None, None) == 0
    # more scales than the device takes
    many = np.arange(1, 18, dtype=np.int64)
    assert lib.csr_segments_run(None, L.dp(x), 300, 17, i64(many), 2, L.dp(thr), 2, L.dp(ns), 1, 0, 0, i64(rows), i64(cnt),
                                C.byref(fl)) == -1
    assert "scales" in L.last_error()
    # a panel phase without a panel
    one32, g_rows, g_cnt = np.array([2], np.int32), np.zeros(1, np.int64), np.zeros(3, np.int64)
    assert lib.csr_dwb_panel_segments(None, 0, 1, i32(one32), i64(sc), i32(one32), L.dp(thr), L.dp(ns), 1, 0, 16, i64(g_rows),
                                      i64(g_cnt), C.byref(fl)) == -1
    assert "csr_dwb_panel_begin" in L.last_error()
    # ... with a panel: the cap is required, and the draws must lie inside a group
    n = np.array([300], np.int64)
    bw = np.array([3], np.int32)
    z = np.random.default_rng(1).standard_normal(4 * 306)
    assert lib.csr_dwb_panel_begin(None, 1, i64(n), i32(bw), b"bartlett", L.dp(x), L.dp(z), z.shape[0], 4, 2) == 0
    try:
        args = (i32(one32), i64(sc), i32(one32), L.dp(thr), L.dp(ns), 1, 0)
        assert lib.csr_dwb_panel_segments(None, 0, 2, *args, 0, i64(g_rows), i64(g_cnt), C.byref(fl)) == -1
        assert "max_segments_per_view" in L.last_error()
        two_rows, two_cnt = np.zeros(3, np.int64), np.zeros(9, np.int64)
        assert lib.csr_dwb_panel_segments(None, 0, 3, *args, 16, i64(two_rows), i64(two_cnt), C.byref(fl)) == -1
        assert lib.csr_dwb_panel_segments(None, 3, 2, *args, 16, i64(two_rows), i64(two_cnt), C.byref(fl)) == -1
        assert "out of range" in L.last_error()
        assert lib.csr_dwb_panel_segments(None, 2, 2, *args, 16, i64(two_rows), i64(two_cnt), C.byref(fl)) == 0
    finally:
        assert lib.csr_dwb_panel_end(None) == 0
    assert lib.csr_dwb_panel_segments(None, 0, 1, *args, 16, i64(g_rows), i64(g_cnt), C.byref(fl)) == -1
    # phase 2 without phase 1, and with a flagged view left unresolved
    with DeviceBatch(0) as b:
        b.configure(ModelParams(state_dim=2), 2, [300])
        assert lib.csr_segments_fetch(b._ctx, i64(rows), i64(rows), i64(rows), i64(rows), L.dp(x), L.dp(x), L.dp(x), L.dp(x)) == -1
        assert "no segment run" in L.last_error()
        b.upload_scores(0, np.r_[np.tile([5.0, 0.0], 100), np.zeros(100)])      # 100 one-bin runs with the same score
        one_v = np.array([1], np.int32)
        t1, s1, w1 = np.array([1.0]), np.array([1.0]), np.array([1], np.int64)
        assert lib.csr_batch_segments_run(b._ctx, i32(one_v), i64(w1), i32(one_v), L.dp(t1), L.dp(s1), 1, 0, 10, i64(rows), i64(cnt),
                                          C.byref(fl)) == 0
        assert rows[0] == 10 and list(cnt) == [100, 1, 90] and fl.value == 1
        out_i = [np.zeros(10, np.int64) for _ in range(4)]
        out_f = [np.zeros(10, np.float64) for _ in range(4)]
        assert lib.csr_segments_fetch(b._ctx, *[i64(a) for a in out_i], *[L.dp(a) for a in out_f]) == -1
        assert "not been resolved" in L.last_error()
        tr, si, vw, nc = C.c_int32(9), C.c_int32(9), C.c_int32(9), C.c_int64(0)
        assert lib.csr_segments_flagged(b._ctx, 0, C.byref(tr), C.byref(si), C.byref(vw), C.byref(nc)) == 0
        assert (tr.value, si.value, vw.value, nc.value) == (0, 0, 0, 100)
        assert lib.csr_segments_flagged(b._ctx, 1, C.byref(tr), C.byref(si), C.byref(vw), C.byref(nc)) == -1
        score, start = np.zeros(100), np.zeros(100, np.int64)
        assert lib.csr_segments_flagged_fetch(b._ctx, 0, L.dp(score), i64(start)) == 0
        assert np.all(score == 4.0) and list(start) == list(range(0, 200, 2))
        pick = np.arange(90, 100, dtype=np.int64)
        assert lib.csr_segments_flagged_select(b._ctx, 0, 9, i64(pick)) == -1
        assert lib.csr_segments_flagged_select(b._ctx, 0, 10, i64(pick + 1)) == -1
        assert lib.csr_segments_flagged_select(b._ctx, 0, 10, i64(pick)) == 0
        assert lib.csr_segments_fetch(b._ctx, *[i64(a) for a in out_i], *[L.dp(a) for a in out_f]) == 0
        assert list(out_i[0]) == list(range(180, 200, 2)) and list(out_i[1]) == list(out_i[0]) and np.all(out_f[0] == 4.0)
        assert np.all(out_i[2] == 1) and np.all(out_i[3] == 0) and np.all(out_f[3] == 4.0)
