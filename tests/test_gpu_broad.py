"""Broad mode on the device against the fixtures made from the reference's own functions (tests/golden/make_broad_golden.py), bit
for bit: integers exactly, floats by bit pattern, strings, key order and Python types exactly.

  1. the drop-ins (host arrays) on every case of tests/broad_cases.py, against the fixtures, with the cap on host decisions;
  2. the gap sums of every gap length of the table against the reference's own NumPy expression;
  3. csr_broad_rows of three chains in one call -- parents of two cases side by side and an empty chain between them -- equal to the
     single-chain calls, with the parent mask;
  4. DeviceBatch.broad_parents and broadpeak_rows from uploaded resident scores, strong and weak masks of a fitted batch: the six
     chains of tests/broad_cases.py `parents_cases` in one call each (one masked out, one with empty masks, one with coordinate
     breaks, one taking the envelope fallback, one of 21 000 bins), the parents against the fixtures and the reference-steps twin,
     the rows against the twin fed with the downloaded tracks (the signal and the uncertainty are the fit's own, which no fixture
     made without a GPU can hold); `rocco_weak` against `rocco`; nothing resident changes;
  5. a fitted batch through first_pass_peaks_batch -> nested_peaks_batch -> broad_peaks_batch -> score_peaks_batch, both state
     models, equal to the twin fed with the downloaded tracks; the scorer is handed the broad parents."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import broad_cases as BC  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(HERE, "golden", "broad")
MERGE, ROWS = BC.merge_cases(), BC.rows_cases()


def golden(file, name):
    with np.load(os.path.join(GOLD, file)) as z:
        return BC.unpack(z[name])


def bits(a):
    return np.asarray(a, np.float64).view(np.uint64).tolist()


@pytest.fixture(scope="module")
def product():
    from consenrich_amd import _lib, broad

    _lib.require_gpu()
    return broad


@pytest.mark.parametrize("case", MERGE, ids=lambda c: c["name"])
def test_merge_drop_in_equals_the_reference(product, case):
    got = product.merge_broad_runs_by_objective(**case["kw"])
    assert BC.differences(BC.canon(got), golden("broad_merge.npz", case["name"])) == []


@pytest.mark.parametrize("fraction", [0.5, 1.0, 0.25])
def test_gap_sums_equal_numpy(product, fraction):
    kw = BC.case(MERGE, "gap_lengths_soft")["kw"]
    rs, re = np.asarray(kw["runs"], np.int64).T
    starts, lens = np.ascontiguousarray(re[:-1] + 1), np.ascontiguousarray(rs[1:] - re[:-1] - 1)
    assert sorted(lens.tolist()) == sorted(BC.GAP_LENGTHS + (0,))
    s = kw["scores"]
    got = product._device_gap_sums(s, 0.5, fraction, starts, lens)
    want = []
    for a, k in zip(starts.tolist(), lens.tolist()):
        ex = np.asarray(s[a:a + k] - 0.5, dtype=np.float64)
        want.append(float(np.sum(np.where(ex < 0.0, fraction * ex, ex))) if k else 0.0)
    assert bits(got) == bits(want)


@pytest.mark.parametrize("case", ROWS, ids=lambda c: c["name"])
def test_rows_drop_in_equals_the_reference(product, case):
    kw = case["kw"]
    before = dict(product.STATS)
    with np.errstate(invalid="ignore"):
        got = product.solution_to_chrom_broadpeak_rows(**kw)
    assert type(got) is tuple and len(got) == (4 if kw["returnExportDetails"] else 3)
    assert BC.differences(BC.canon(got), golden("broad_rows.npz", case["name"])) == []
    # the cap on host decisions: the NaN chain and no other
    assert product.STATS["decided_on_host"] - before["decided_on_host"] == int(case["name"] in BC.HOST_DECIDED)


def test_rows_of_several_chains_in_one_call(product):
    from consenrich_amd import _lib as L

    kws = [BC.case(ROWS, "lengths")["kw"], None, BC.case(ROWS, "filters")["kw"]]
    single, runs = [], []
    for kw in kws:
        if kw is None:
            single.append(None)
            runs.append((np.zeros(0, np.int64),) * 2)
            continue
        ps, pe = product.coordinate_runs(kw["parentSolution"], kw["intervals"], kw["ends"])
        single.append(product._device_records(kw["state"], kw["scores"], kw["uncertainty"], 2.0, ps, pe))
        runs.append((ps, pe))
    lens = np.asarray([0 if kw is None else kw["scores"].size for kw in kws], np.int64)
    cat = lambda key: np.ascontiguousarray(np.concatenate([kw[key] for kw in kws if kw is not None]))    # noqa: E731
    par = np.zeros(sum(r[0].size for r in runs), product.PARENT)
    par["start"], par["end"] = np.concatenate([r[0] for r in runs]), np.concatenate([r[1] for r in runs])
    par["chain"] = np.concatenate([np.full(r[0].size, c, np.int32) for c, r in enumerate(runs)])
    cfg = np.asarray([(2.0, 1, 0), (2.0, 1, 0), (2.0, 1, 0)], product.CFG)
    rec = np.zeros(par.size, product.REC)
    mask = np.zeros(int(lens.sum()), np.uint8)
    L.check_value(L.lib().csr_broad_rows(3, L._i64p(lens), L.dp(cat("state")), L.dp(cat("scores")), L.dp(cat("uncertainty")),
                                         cfg.ctypes.data_as(C.c_void_p), par.size, par.ctypes.data_as(C.c_void_p),
                                         mask.ctypes.data_as(C.POINTER(C.c_uint8)), rec.ctypes.data_as(C.c_void_p)))
    want = np.concatenate([single[0][0], single[2][0]])
    want["chain"][single[0][0].size:] = 2
    assert rec.tobytes() == want.tobytes()
    assert np.array_equal(mask, np.concatenate([single[0][1], single[2][1]]))
    assert np.array_equal(mask, (cat("parentSolution") > 0).astype(np.uint8))


# ---------------------------------------------------------------------------------------------------------------
# the resident form: six chains of a fitted batch through one broad_parents and one broadpeak_rows call
# ---------------------------------------------------------------------------------------------------------------
FIT = ("D", "xf", "Pf", "pnoise", "xs", "Ps", "lag")


def _tracks(b, c):
    return b.download(c, "xs")[:, 0].astype(np.float64), np.sqrt(b.download(c, "Ps")[:, 0, 0]).astype(np.float64)


def test_broad_parents_and_rows_of_resident_tracks(product):
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import cases
    import twin_broad as T
    from consenrich_amd import _lib as L
    from consenrich_amd.batch import DeviceBatch, ModelParams

    cases6 = BC.parents_cases()[:6]
    chs = [c["kw"] for c in cases6]
    lens = [ch["scores"].size for ch in chs]
    nc = len(chs)
    take = [True, False, True, True, True, True]
    names = [ch["chromosome"] for ch in chs]
    pens, costs, gaps = ([ch[k] for ch in chs] for k in ("selection_penalty", "boundary_cost", "max_gap_bp"))
    blacklist = chs[0]["blacklist"]
    THRESHOLD = BC.SUPPORT_THRESHOLD
    with DeviceBatch(0) as b:
        b.configure(ModelParams(state_dim=2), 2, lens)
        for c, n in enumerate(lens):
            b.upload(c, *cases.synth(n, 2, 880 + c))
        b.stats()
        b.forward_backward(L.RETURN_NLL)
        b.export(L.EXPORT_FORWARD | L.EXPORT_SMOOTH)
        for c, ch in enumerate(chs):
            b.upload_scores(c, ch["scores"])
        b.rocco(budget=0.1, gamma=0.5)
        # the weak pass is the strong pass with another destination: the same arguments give the same mask, and the strong one stays
        strong0 = [b.rocco_solution(c) for c in range(nc)]
        out_s = b.rocco(budget=0.2, gamma=1.0, chains=[True, False, False, False, False, False])
        want_weak = b.rocco_solution(0)
        b.upload_solution(0, strong0[0])
        out_w = b.rocco_weak(budget=0.2, gamma=1.0, chains=[True, False, False, False, False, False])
        assert out_w[0] == out_s[0] and out_w[1] is None
        assert np.array_equal(b.weak_solution(0), want_weak) and want_weak.any()
        assert np.array_equal(b.rocco_solution(0), strong0[0])
        with pytest.raises(L.ConsenrichAMDError, match="chain 2 has no weak ROCCO solution"):
            b.weak_solution(2)
        for c, ch in enumerate(chs):
            b.upload_solution(c, ch["strong"])
            b.upload_weak_solution(c, ch["weak"])
            b.upload_template(c, BC.wave(lens[c], 40 + c))
        fit = {(c, a): b.download(c, a) for c in range(nc) for a in FIT}
        tmpls = [b.download_template(c) for c in range(nc)]
        common = dict(intervals=[ch["intervals"] for ch in chs], ends=[ch["ends"] for ch in chs], chroms=names, chains=take)

        got = b.broad_parents(THRESHOLD, pens, costs, max_gap_bp=gaps, blacklist=blacklist, run_penalty=0.0, **common)
        rows = b.broadpeak_rows(prefix="bp", **common)
        assert got[1] is None and rows[1] is None
        merged_any = kept = 0
        for c in (0, 2, 3, 4, 5):
            ch = chs[c]
            want = T.parents(ch["scores"], ch["strong"], ch["weak"], THRESHOLD, ch["intervals"], ch["ends"], names[c], pens[c], costs[c],
                             gaps[c], blacklist)
            g = got[c]
            assert BC.differences(BC.canon({k: v for k, v in want.items() if k != "mask"}), golden("broad_parents.npz", names[c])) == [], c
            assert (g["starts"].tolist(), g["ends"].tolist()) == (want["starts"], want["ends"]), c
            assert BC.differences(BC.canon(g["merge_details"]), BC.canon(want["merge_details"])) == [], c
            assert (g["weak_support_run_count"], g["weak_support_touching_run_count"], g["envelope_fallback"]) == \
                   (want["weak_support_run_count"], want["weak_support_touching_run_count"], want["envelope_fallback"]), c
            assert np.array_equal(b.broad_parent_solution(c), want["mask"]), c
            x, u = _tracks(b, c)
            rw = T.rows(names[c], ch["intervals"], ch["ends"], x, ch["scores"], want["mask"], ch["strong"], "bp", uncertainty=u,
                        returnExportDetails=True)
            r = rows[c]
            assert BC.differences(BC.canon((r["broad_rows"], r["gapped_rows"], r["peak_meta"], r["export_details"])), BC.canon(rw)) == [], c
            assert r["decided_on_host"] is False
            merged_any += want["merge_details"].get("num_gaps_merged", 0)
            kept += len(rw[0])
        # the table does what it is there for
        assert got[2]["envelope_fallback"] and got[2]["starts"].size == 0 and len(got[2]["merge_details"]) == 10
        assert got[2]["weak_support_run_count"] > 0 and rows[2]["broad_rows"] == []
        assert got[4]["envelope_fallback"] and got[4]["weak_support_run_count"] == 0 and got[4]["weak_support_touching_run_count"] == 2
        assert 1024 in got[3]["starts"].tolist() and 1000 not in got[3]["starts"].tolist()      # the piece in front of the break does not touch
        assert got[3]["weak_support_touching_run_count"] == 4 and got[3]["merge_details"]["num_gaps_merged"] == 1    # (0 bins, 75 bp)
        assert got[0]["merge_details"]["num_gaps_blocked_by_blacklist"] == 1 and got[0]["merge_details"]["num_gaps_blocked_by_distance"] >= 1
        assert got[5]["starts"][0] == 0 and got[5]["ends"][-1] == lens[5] - 1
        assert merged_any >= 3 and kept >= 6
        assert b.broad_stats["decided_on_host"] == 0 and b.broad_stats["chains"] == 5 and b.broad_stats["rows"] == kept
        # without the uncertainty, on one chain
        plain = b.broadpeak_rows(prefix="bp", use_uncertainty=False, intervals=common["intervals"], ends=common["ends"], chroms=names,
                                 chains=[True] + [False] * 5)
        x, _ = _tracks(b, 0)
        rw = T.rows(names[0], chs[0]["intervals"], chs[0]["ends"], x, chs[0]["scores"], b.broad_parent_solution(0), chs[0]["strong"], "bp",
                    returnExportDetails=True)
        assert BC.differences(BC.canon((plain[0]["broad_rows"], plain[0]["gapped_rows"], plain[0]["peak_meta"], plain[0]["export_details"])),
                              BC.canon(rw)) == []
        assert rw[3]["median_signal_local_p_filter_active"] is False
        with pytest.raises(ValueError, match="`exportFilterUncertaintyMultiplier` must be finite and non-negative"):
            b.broadpeak_rows(prefix="bp", multiplier=-1.0, **common)
        # nothing resident has changed
        for c, ch in enumerate(chs):
            assert np.array_equal(b.rocco_solution(c), ch["strong"]), c
            assert np.array_equal(b.weak_solution(c), ch["weak"]), c
            assert bits(b.download_scores(c)) == bits(ch["scores"]), c
            assert bits(b.download_template(c)) == bits(tmpls[c]), c
        for (c, a), v in fit.items():
            assert np.array_equal(b.download(c, a).view(np.uint32), v.view(np.uint32)), (c, a)
        # new scores drop the weak mask and the parent mask with the strong one
        b.upload_scores(4, chs[4]["scores"])
        for f in (b.weak_solution, b.broad_parent_solution, b.rocco_solution):
            with pytest.raises(L.ConsenrichAMDError, match="chain 4 has no"):
                f(4)
        with pytest.raises(L.ConsenrichAMDError, match="chain 4 has no broad parents"):
            b.broadpeak_rows(prefix="bp", intervals=common["intervals"], ends=common["ends"], chroms=names, chains=[False] * 4 + [True, False])


@pytest.mark.parametrize("state_dim", [2, 1])
def test_broad_peaks_batch_between_the_refinement_and_the_scorer(product, state_dim):
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import cases
    import twin_broad as T
    from consenrich_amd import _lib as L
    from consenrich_amd import driver, ess
    from consenrich_amd.batch import DeviceBatch, ModelParams

    lens, m, spans, seed, replays, step = [3001, 2049], 3, [6, 3], 5, 4, 25
    grid = (1.5, 2.0, 2.5, 3.0)
    names = ["chrA", "chrB"]
    mp = ModelParams(state_dim=2) if state_dim == 2 else ModelParams(state_dim=1, Q0=((1e-3, 0), (0, 0)))
    with DeviceBatch(0) as b:
        b.configure(mp, m, lens)
        for c, n in enumerate(lens):
            b.upload(c, *cases.synth(n, m, 990 + c))
        b.stats()
        b.forward_backward(L.RETURN_NLL)
        b.export(L.EXPORT_FORWARD | L.EXPORT_SMOOTH)
        first = driver.first_pass_peaks_batch(b, dependence_spans=spans, threshold_z=2.0, threshold_z_grid=grid, num_bootstrap=9,
                                              random_seed=seed, gamma=-1.0, gamma_scale=0.5, score_mode="state", z=1.0, max_gap_bins=0)
        scores = [b.download_scores(c) for c in range(2)]
        # chain 0's first pass may select nothing: plant the upper fifth of its scores instead, so that there are children
        b.upload_solution(0, (scores[0] > np.quantile(scores[0], 0.8)).astype(np.uint8))
        first[0]["starts"], first[0]["ends"] = b.rocco_runs(0)
        nested = driver.nested_peaks_batch(b, first, interval_bp=step)
        fit = {(c, a): b.download(c, a) for c in range(2) for a in ("xs", "Ps", "xf", "Pf")}
        masks = [b.rocco_solution(c) for c in range(2)]
        tmpls = [b.download_template(c) for c in range(2)]
        got = driver.broad_peaks_batch(b, nested, dependence_spans=spans, threshold_z=2.0, threshold_z_grid=grid, num_bootstrap=9,
                                       random_seed=seed, interval_bp=step, chroms=names, prefix="cs")
        kept = 0
        for c in range(2):
            iv = np.arange(lens[c], dtype=np.int64) * step
            r, bp = got[c], got[c]["broad_parent"]
            assert bp["weak_gamma"] == 2.0 * nested[c]["gamma"] and bp["weak_threshold_z"] == 1.2816
            assert bp["weak_support_threshold"] <= nested[c]["budget_details"]["threshold"]
            assert bp["weak_budget"] >= nested[c]["budget"]
            assert bp["max_gap_bp"] == 4 * spans[c] * step
            weak = b.weak_solution(c)
            assert int(weak.sum()) == bp["weak_solve_details"]["selected_count"]
            want = T.parents(scores[c], masks[c], weak, bp["weak_support_threshold"], iv, iv + step, names[c],
                             bp["weak_solve_details"]["selection_penalty"], bp["weak_gamma"], bp["max_gap_bp"])
            assert (bp["parent_starts"].tolist(), bp["parent_ends"].tolist()) == (want["starts"], want["ends"]), c
            assert BC.differences(BC.canon(bp["merge_details"]), BC.canon(want["merge_details"])) == [], c
            assert (bp["weak_support_run_count"], bp["weak_support_touching_run_count"], bp["envelope_fallback"]) == \
                   (want["weak_support_run_count"], want["weak_support_touching_run_count"], want["envelope_fallback"]), c
            assert np.array_equal(b.broad_parent_solution(c), want["mask"]), c
            x, u = _tracks(b, c)
            rw = T.rows(names[c], iv, iv + step, x, scores[c], want["mask"], masks[c], "cs", uncertainty=u, returnExportDetails=True)
            assert BC.differences(BC.canon((r["broad_rows"], r["gapped_rows"], r["peak_meta"], r["export_details"])), BC.canon(rw)) == [], c
            assert r["decided_on_host"] == int(bp["weak_solve_details"]["budget_fallback_window"])
            assert r["starts"].tolist() == [q["start_idx"] for q in rw[2]] and r["ends"].tolist() == [q["end_idx"] for q in rw[2]]
            assert r["gamma"] == nested[c]["gamma"] and r["nested_rocco_stop_reason"] == nested[c]["nested_rocco_stop_reason"]
            kept += len(rw[0])
            print("chain", c, want["merge_details"], rw[3])
        assert kept >= 1
        # the scorer takes the broad parents, not the mask's runs
        views = b.dwb_panel(threshold_z_grid=ess.resolve_z_grid(2.0, grid), bandwidths=spans, num_bootstrap=9, random_seed=seed,
                            calibration_quantile=0.9)
        scored = driver.score_peaks_batch(b, got, views, dependence_spans=spans, random_seed=seed, num_replay=replays)
        direct = b.dwb_peak_scoring(views, bandwidths=spans, peaks=[(r["starts"], r["ends"]) for r in got], num_replay=replays,
                                    random_seed=seed)
        for c in range(2):
            assert BC.differences(BC.canon(_plain(scored[c])), BC.canon(_plain(direct[c]))) == [], c
        for (c, a), v in fit.items():
            assert np.array_equal(b.download(c, a).view(np.uint32), v.view(np.uint32)), (c, a)
        for c in range(2):
            assert np.array_equal(b.rocco_solution(c), masks[c])
            assert bits(b.download_scores(c)) == bits(scores[c]), c
            assert bits(b.download_template(c)) == bits(tmpls[c]), c


def _plain(v):
    """NumPy arrays and scalars as Python values, so that two results of the scorer compare in the canonical form"""
    if isinstance(v, dict):
        return {k: _plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    if isinstance(v, np.ndarray):
        return [_plain(x) for x in v.tolist()]
    if isinstance(v, np.generic):
        return v.item()
    return v
