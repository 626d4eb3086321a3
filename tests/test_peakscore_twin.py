"""CPU: both forms of the pure-Python twin of the DWB peak scoring (tests/twin_peakscore.py) equal the reference's recorded outputs
(tests/golden/peakscore/peakscore_*.npz) and each other, bit for bit; the product's host-side merge equals the twin's dict merge;
what the product checks before any GPU call."""
import os

import numpy as np
import pytest

import peakscore_cases as PC
import twin_peakscore as T

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "peakscore")


@pytest.fixture(scope="module")
def golden():
    out = {}
    for name in ("segments", "pq"):
        with np.load(os.path.join(GOLDEN, f"peakscore_{name}.npz")) as z:
            out.update({k: z[k] for k in z.files})
    return out


def _live(views):
    return [(k, v) for k, v in views.items() if isinstance(v, dict)]


@pytest.mark.parametrize("case", PC.segment_cases(), ids=lambda c: c["name"])
def test_segment_scores_of_both_twin_forms_equal_the_reference(golden, case):
    x, (st, en), views = PC.track(case["n"]), PC.segments(case["n"]), PC.view_sets()[case["views"]]
    live = _live(views)
    with np.errstate(all="ignore"):
        steps = [T.best_score_steps(x, a, b, views) for a, b in zip(st, en)]
    dev = T.segment_arrays_device(x, st, en, [v["threshold"] for _, v in live], [v["null_scale"] for _, v in live])
    assert T.same_details(steps, T.details_from_arrays(dev, views))
    keys = [k for k, _ in live]
    for i, f in enumerate(T.NUMERIC):
        want = golden[f"{case['name']}/{f}"]
        assert np.array_equal(T.bits([s[f] for s in steps]), T.bits(want)), f
        assert np.array_equal(T.bits(dev[i]), T.bits(want)), f
    assert [keys.index(s["threshold_key"]) for s in steps] == list(golden[f"{case['name']}/view"]) == list(dev[4])


def test_the_view_cases_do_what_they_are_there_for(golden):
    """views4: the tie keeps the first view, the NaN view never wins, the DBL_MIN view wins with inf where a value exceeds its
    threshold; nan_first: a NaN in front stays; every empty segment is all zeros at view 0."""
    view, score = golden[f"seg_n{PC.N_TRACK}_views4/view"], golden[f"seg_n{PC.N_TRACK}_views4/score"]
    assert set(view) == {0, 3} and np.isinf(score[view == 3]).any() and np.isfinite(score[view == 0]).all()
    st, en = PC.segments()
    empty = np.minimum(en, PC.N_TRACK - 1) < np.maximum(st, 0)
    assert empty.sum() == 4 and not score[empty].any() and not view[empty].any()
    nan_first = golden[f"seg_n{PC.N_TRACK}_nan_first/score"]
    assert np.isnan(nan_first[~empty]).all() and not golden[f"seg_n{PC.N_TRACK}_nan_first/view"].any()
    assert sorted(set((en - st + 1)[:22])) == list(PC.LENGTHS)


def test_the_leaf_list_fits_the_kernel():
    """A chunk's pairwise tree has at most 128 leaves of at most 128 values and is at most 8 levels deep below the root."""
    for n in list(range(1, 1100)) + [4095, 4096, 4097, 8185, 8191, 8192]:
        leaves = T.tree_leaves(n)
        assert len(leaves) <= 128 and max(m for _, m in leaves) <= 128 and sum(m for _, m in leaves) == n
        assert [lo for lo, _ in leaves] == list(np.cumsum([0] + [m for _, m in leaves][:-1]))
    x = np.random.default_rng(1).standard_normal(3 * T.CHUNK + 77)
    for n in (1, 7, 8, 129, 1000, T.CHUNK, T.CHUNK + 1, x.size):
        assert T.bits(T.numpy_sum_device(x[:n])) == T.bits(np.sum(x[:n])), n


@pytest.mark.parametrize("case", PC.pq_cases(), ids=lambda c: c["name"])
def test_p_and_q_values_of_both_twin_forms_equal_the_reference(golden, case):
    obs, draws = PC.pq_inputs(case)
    pool = np.concatenate(draws) if draws else np.zeros(0)
    p, q, c = T.pq_device(obs, pool, len(draws))
    assert np.array_equal(T.bits(T.pvalues_steps(obs, draws)), T.bits(golden[f"{case['name']}/p"]))
    assert np.array_equal(T.bits(T.qvalues_steps(obs, draws)), T.bits(golden[f"{case['name']}/q"]))
    assert np.array_equal(T.bits(p), T.bits(golden[f"{case['name']}/p"]))
    assert np.array_equal(T.bits(q), T.bits(golden[f"{case['name']}/q"]))
    assert list(c) == [int(np.sum(pool >= v)) for v in obs]
    # the pool's order does not matter
    p2, q2, _ = T.pq_device(obs, pool[::-1], len(draws))
    assert np.array_equal(T.bits(p2), T.bits(p)) and np.array_equal(T.bits(q2), T.bits(q))


def test_the_pq_cases_do_what_they_are_there_for():
    obs, draws = PC.pq_inputs(dict(k=4097, draws="r5"))
    pool = np.concatenate(draws)
    assert pool.size == PC.SORT_TILE + 1 and any(d.size == 0 for d in draws)
    assert np.isin(obs, pool).sum() > 1000 and np.unique(obs).size < obs.size
    assert np.signbit(obs[obs == 0.0]).any() and not np.signbit(obs[obs == 0.0]).all()
    assert np.signbit(pool[pool == 0.0]).any() and not np.signbit(pool[pool == 0.0]).all()
    assert obs.max() > pool.max() and obs.min() < pool.min()


def test_the_twin_raises_the_references_errors():
    with pytest.raises(ValueError, match=f"^{T.P_TEXT}$"):
        T.pvalues_steps([1.0, np.nan], [[1.0]])
    with pytest.raises(ValueError, match=f"^{T.Q_TEXT}$"):
        T.qvalues_steps([1.0], [[1.0], [np.inf]])
    assert list(T.pvalues_steps([np.nan], [[]])) == [1.0]      # without a pooled value the reference never looks


def test_the_merge_equals_the_dict_merge_and_the_last_arg_max_by_span():
    from consenrich_amd import peakscore

    cands, spans, details, n = PC.merge_inputs()
    want = T.merge_steps([dict(c) for c in cands], spans, details, n)
    got = peakscore.merge_candidate_regions(cands, spans, details, n)
    assert len(got) == len(want) < len(cands) + len(spans)
    for g, w in zip(got, want):
        assert set(g) == set(w)
        for k in w:
            if isinstance(w[k], float):
                assert T.bits(g[k]) == T.bits(w[k]), (w["start_idx"], w["end_idx"], k)
            else:
                assert g[k] == w[k], (w["start_idx"], w["end_idx"], k)
    numeric = T.merge_numeric_device(cands, spans, details, n)
    assert set(numeric) == {(w["start_idx"], w["end_idx"]) for w in want}
    for w in want:
        rec = numeric[(w["start_idx"], w["end_idx"])]
        assert all(T.bits(rec[k]) == T.bits(w[k]) for k in T.NUMERIC) and rec["threshold_key"] == w["threshold_key"]
    assert sum(w["exported"] for w in want) == len(set(spans))
    assert any(w["exported"] and "multiscale_threshold_run" in w["candidate_sources"] for w in want)
    assert any(w.get("overlapping_multiscale_candidate_count", 0) > 1 for w in want)
    assert any(w["exported"] and "overlapping_multiscale_candidate_count" not in w for w in want)
    # with coordinates
    iv, ends = np.arange(n) * 25 + 1000, np.arange(n) * 25 + 1025
    got = peakscore.merge_candidate_regions(cands, spans, details, n, iv, ends)
    want = T.merge_steps(cands, spans, details, n, iv, ends)
    assert [(g["start"], g["end"]) for g in got] == [(w["start"], w["end"]) for w in want]


def test_what_the_product_answers_before_any_gpu_call():
    from consenrich_amd import peakscore

    assert peakscore.empirical_replay_segment_pvalues([], [[1.0]]).shape == (0,)
    assert peakscore.replay_fdr_qvalues([], [[np.nan]]).shape == (0,)
    assert list(peakscore.empirical_replay_segment_pvalues([np.nan, 2.0], [[], []])) == [1.0, 1.0]
    assert peakscore.best_segment_scores(np.zeros(4), [0, 1], [2, 3], {"skip": 1.0}) == [dict(T.ZERO), dict(T.ZERO)]
    assert peakscore.best_segment_scores(np.zeros(4), [], [], {"a": dict(threshold=0.0)}) == []
    with pytest.raises(ValueError, match="same length"):
        peakscore.best_segment_scores(np.zeros(4), [0], [1, 2], {"a": dict(threshold=0.0)})
    with pytest.raises(ValueError, match="threshold views"):
        peakscore.best_segment_scores(np.zeros(4), [0], [1], {str(i): dict(threshold=0.0) for i in range(17)})


def test_the_scorer_case_does_what_it_is_there_for_and_both_twin_forms_agree_on_it():
    """Chain 0: every replay draw exceeds the total cap; chain 1: every draw stays under it; an exported peak coincides with an
    observed candidate; the pooled-count form of p, max(q, p) and the exceedances equals the per-draw form on every region."""
    scores, tmpls, views = PC.scorer_inputs()
    twin = PC.scorer_twin(scores, tmpls, views)
    peaks = PC.scorer_peaks(twin)
    assert all(d["total_cap_hit"] and len(rc) == PC.SCORER_TOTAL_CAP for rc, d in twin[0]["replays"])
    assert all(not d["total_cap_hit"] and 0 < len(rc) < PC.SCORER_TOTAL_CAP for rc, d in twin[1]["replays"])
    assert any(d["per_view_cap_hit_count"] > 0 for rc, d in twin[0]["replays"])
    assert PC.scorer_case_facts(twin, peaks) == dict(draw_over_the_total_cap_with_a_tie_across_the_cut=True,
                                                     draw_under_the_total_cap=True, peak_on_an_observed_candidate=True)
    for c in range(2):
        spans = {(k["start_idx"], k["end_idx"]) for k in twin[c]["observed"][0]}
        assert any(p in spans for p in peaks[c]) and any(p not in spans for p in peaks[c])
        res = T.score_steps(scores[c], twin[c]["views"], twin[c]["observed"], twin[c]["replays"], peaks[c], scale_bins=twin[c]["scale_bins"],
                            dependence_span=PC.SCORER_BWS[c], random_seed=PC.SCORER_SEED)
        assert res["enabled"] and len(res["peaks"]) == len(peaks[c]) and res["summary"]["num_candidate_regions"] == len(res["candidate_details"])
        assert sum(d["exported"] for d in res["candidate_details"]) == len(peaks[c])
        for metric, src in T.SOURCES:
            obs = [d[metric] for d in res["candidate_details"]]
            pool = np.concatenate([[k[src] for k in rc] for rc, _ in twin[c]["replays"]])
            p, q, exc = T.pq_device(obs, pool, PC.SCORER_REPLAYS)
            assert np.array_equal(T.bits(p), T.bits([d[f"{metric}_p"] for d in res["candidate_details"]]))
            assert np.array_equal(T.bits(np.maximum(q, p)), T.bits([d[f"{metric}_q"] for d in res["candidate_details"]]))
            if metric == "width_adjusted_mass":
                assert list(exc) == [d["dwb_peak_null_exceedances"] for d in res["candidate_details"]]
        assert T.differences(res, res) == [] and T.differences(res, dict(res, enabled=1)) != []
    assert T.score_steps(scores[0], twin[0]["views"], twin[0]["observed"], twin[0]["replays"], [], scale_bins=(), dependence_span=2,
                         random_seed=0) == dict(enabled=False, reason="no_peaks", num_peaks=0)
