"""The massive sub-peak clean-up from the RESIDENT fit: `DeviceBatch.narrowpeak_rows(width_policy=...)` on a fitted batch of six
short chains in one call, and `driver.cleanup_peaks_batch` between `export_peaks_batch` and `score_peaks_batch`.  The expected rows
are the steps form of the twin (tests/twin_cleanup.py `rows`, held equal to the reference by the fixtures) fed with the downloaded
tracks.  No resident array changes."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(HERE, "golden")]
import cases  # noqa: E402
import cleanup_cases as CC  # noqa: E402
import twin_cleanup as T  # noqa: E402
import twin_narrowpeak as TNP  # noqa: E402

pytestmark = pytest.mark.gpu
FIT = ("xs", "Ps", "xf", "Pf")


def _tracks(b, c):
    return b.download(c, "xs")[:, 0].astype(np.float64), np.sqrt(b.download(c, "Ps")[:, 0, 0]).astype(np.float64)


def _resident(b, nc):
    return ({(c, a): b.download(c, a) for c in range(nc) for a in FIT}, [b.download_scores(c) for c in range(nc)],
            [b.rocco_solution(c) for c in range(nc)], [b.download_template(c) for c in range(nc)])


def _unchanged(b, before):
    fit, scores, masks, tmpls = before
    for (c, a), v in fit.items():
        assert np.array_equal(b.download(c, a).view(np.uint32), v.view(np.uint32)), (c, a)
    for c in range(len(scores)):
        assert np.array_equal(b.rocco_solution(c), masks[c]), c
        assert np.array_equal(TNP.bits(b.download_scores(c)), TNP.bits(scores[c])), c
        assert np.array_equal(TNP.bits(b.download_template(c)), TNP.bits(tmpls[c])), c


def test_narrowpeak_rows_with_a_width_policy_on_a_fitted_batch():
    from consenrich_amd import _lib as L
    from consenrich_amd import cleanup as K
    from consenrich_amd.batch import DeviceBatch, ModelParams

    # six chains: plain, with coordinate gaps (one in front of a candidate), another track, one masked out, one with an empty mask,
    # one whose runs are all below the threshold
    tr = [CC._row_track("rows", ()), CC._row_track("rows", (24, 140)), CC._row_track("rows2", ()), CC._row_track("rows3", ()),
          CC._row_track("rows4", ()), CC._row_track("rows5", ())]
    tr[4]["solution"] = np.zeros_like(tr[4]["solution"])
    keep = np.zeros_like(tr[5]["solution"])
    keep[10:22] = keep[100:115] = 1
    tr[5]["solution"] = keep * tr[5]["solution"]
    lens = [t["scores"].size for t in tr]
    nc = len(tr)
    policy = dict(CC.FULL_POLICY)
    with DeviceBatch(0) as b:
        b.configure(ModelParams(state_dim=2), 2, lens)
        for c, n in enumerate(lens):
            b.upload(c, *cases.synth(n, 2, 880 + c))
        b.stats()
        b.forward_backward(L.RETURN_NLL)
        b.export(L.EXPORT_FORWARD | L.EXPORT_SMOOTH)
        for c, t in enumerate(tr):
            b.upload_scores(c, t["scores"])
        b.rocco(budget=0.1, gamma=0.5)
        for c, t in enumerate(tr):
            b.upload_solution(c, t["solution"])
            b.upload_template(c, np.cos(np.arange(lens[c]) * 0.1))
        before = _resident(b, nc)
        names = [f"chr{c + 1}" for c in range(nc)]
        take = [True, True, True, False, True, True]
        coords = dict(intervals=[t["intervals"] for t in tr], ends=[t["ends"] for t in tr])

        def expect(c, iv, en, pol, unc=True, cleanup=True):
            x, u = _tracks(b, c)
            return T.rows(names[c], iv, en, x, tr[c]["scores"], tr[c]["solution"], "np", 0.5, uncertainty=u if unc else None,
                          trimScoreFloor=0.0, subpeakSelectionPenalty=0.3, subpeakBoundaryCost=0.25, minSubpeakBins=3,
                          massiveSubpeakCleanup=cleanup, massiveSubpeakWidthPolicy=pol, returnExportDetails=True, form="steps")

        def same(got, want, what):
            assert T.differences((got["rows"], got["peak_meta"], got["export_details"]), want) == [], what

        for unc in (True, False):       # (without the median filter more of the cleaned peaks are kept)
            got = b.narrowpeak_rows(0.3, 1.0, chroms=names, prefix="np", min_subpeak_bins=3, chains=take, width_policy=policy,
                                    use_uncertainty=unc, **coords)
            assert got[3] is None
            for c in (0, 1, 2, 4, 5):
                same(got[c], expect(c, tr[c]["intervals"], tr[c]["ends"], policy, unc), (c, unc))
                assert got[c]["decided_on_host"] is False
            assert got[4]["rows"] == [] and got[4]["export_details"]["massive_subpeak_cleanup_active"] is True
            assert got[1]["export_details"]["num_coordinate_gap_splits"] == 2
            assert got[5]["export_details"]["num_massive_subpeak_candidates"] == 0
            stats = dict(b.narrowpeak_stats)
            assert stats["decided_on_host"] == 0 and stats["chains"] == 5
            assert stats["candidates"] == sum(got[c]["export_details"]["num_massive_subpeak_candidates"] for c in (0, 1, 2, 4, 5)) > 0
            assert stats["contracts"] + stats["splits"] > 0
        modes = {m["massive_subpeak_cleanup_mode"] for c in (0, 1, 2) for m in got[c]["peak_meta"]}
        assert len(modes - {None}) >= 2, modes
        # the chain without a candidate: the first pass's records plus the policy fields
        plain = b.narrowpeak_rows(0.3, 1.0, chroms=names, prefix="np", min_subpeak_bins=3, chains=take, use_uncertainty=False, **coords)
        strip = lambda m: {k: v for k, v in m.items() if k not in ("massive_subpeak_width_p", "massive_subpeak_width_threshold_bp")}     # noqa: E731
        assert [strip(m) for m in got[5]["peak_meta"]] == [strip(m) for m in plain[5]["peak_meta"]] and got[5]["rows"] == plain[5]["rows"]
        assert all(m["massive_subpeak_width_threshold_bp"] == 2000 and type(m["massive_subpeak_width_p"]) is float for m in got[5]["peak_meta"])
        # width_policy=None is the existing call: the same records as the drop-in without a policy makes of the downloaded tracks
        for c in (0, 1, 2, 4, 5):
            x, _ = _tracks(b, c)
            want = TNP.rows(names[c], tr[c]["intervals"], tr[c]["ends"], x, tr[c]["scores"], tr[c]["solution"], "np", 0.5, trimScoreFloor=0.0,
                            subpeakSelectionPenalty=0.3, subpeakBoundaryCost=0.25, minSubpeakBins=3, returnExportDetails=True, form="steps")
            same(plain[c], want, c)
        assert not any(k in b.narrowpeak_stats for k in K.COUNTERS)
        # equally wide bins travel as a step: identical to the edges of the same coordinates
        iv = [np.arange(n, dtype=np.int64) * 100 for n in lens]
        step = b.narrowpeak_rows(0.3, 1.0, interval_bp=100, chroms=names, prefix="np", min_subpeak_bins=3, chains=take, width_policy=policy)
        edge = b.narrowpeak_rows(0.3, 1.0, intervals=iv, ends=[v + 100 for v in iv], chroms=names, prefix="np", min_subpeak_bins=3, chains=take,
                                 width_policy=policy)
        for c in (0, 1, 2, 4, 5):
            same(step[c], expect(c, iv[c], iv[c] + 100, policy), c)
            same(edge[c], (step[c]["rows"], step[c]["peak_meta"], step[c]["export_details"]), c)
        # an inactive policy and a clean-up that is switched off: the first pass's peak set, the policy fields filled
        for pol, kw in ((dict(policy, active=False), {}), (policy, {"massive_subpeak_cleanup": False})):
            off = b.narrowpeak_rows(0.3, 1.0, chroms=names, prefix="np", min_subpeak_bins=3, chains=take, width_policy=pol, **kw, **coords)
            for c in (0, 1, 2, 4, 5):
                same(off[c], expect(c, tr[c]["intervals"], tr[c]["ends"], pol, cleanup=not kw), c)
        _unchanged(b, before)


def _plant(n, seed, wide):
    """scores and mask of one chain of 100 bp bins: short humps of 6-12 bins, and (wide) ONE plateau of 80-110 bins with a shallow
    dip in the middle -- a child of 7500 bp and more.  One, because the policy admits a cluster of at most max(1, 0.5 %) of the
    peaks above a log gap."""
    rng = np.random.default_rng(seed)
    s = -1.0 + 0.1 * rng.standard_normal(n)
    mask = np.zeros(n, np.uint8)
    at = 20
    spots = []
    while at + 140 < n:
        spots.append(at)
        at += int(rng.integers(45, 70))
    for k, a in enumerate(spots):
        if wide and k == 3:
            m = int(rng.integers(80, 111))
            if any(a < q < a + m + 5 for q in spots[k + 1:]):
                spots[k + 1:] = [q for q in spots[k + 1:] if q >= a + m + 5]
            s[a:a + m] = 5.0 + 0.2 * rng.standard_normal(m)
            s[a + m // 2 - 6:a + m // 2 + 6] = 3.5 + 0.1 * rng.standard_normal(12)
        else:
            m = int(rng.integers(6, 13))
            s[a:a + m] = 3.0 + 0.5 * rng.standard_normal(m)
        mask[a:a + m] = 1
    return np.ascontiguousarray(s), mask


@pytest.mark.parametrize("wide", [True, False], ids=["active_policy", "inactive_policy"])
@pytest.mark.parametrize("state_dim", [2, 1])
def test_cleanup_peaks_batch_between_the_export_and_the_scorer(state_dim, wide):
    from consenrich_amd import _lib as L
    from consenrich_amd import driver, ess
    from consenrich_amd.batch import DeviceBatch, ModelParams

    lens, m, spans, seed, replays, step = [3001, 2049], 3, [6, 3], 5, 4, 100
    grid = (1.5, 2.0, 2.5, 3.0)
    mp = ModelParams(state_dim=2) if state_dim == 2 else ModelParams(state_dim=1, Q0=((1e-3, 0), (0, 0)))
    names = ["chrA", "chrB"]
    with DeviceBatch(0) as b:
        b.configure(mp, m, lens)
        for c, n in enumerate(lens):
            b.upload(c, *cases.synth(n, m, 990 + c))
        b.stats()
        b.forward_backward(L.RETURN_NLL)
        b.export(L.EXPORT_FORWARD | L.EXPORT_SMOOTH)
        first = driver.first_pass_peaks_batch(b, dependence_spans=spans, threshold_z=2.0, threshold_z_grid=grid, num_bootstrap=9,
                                              random_seed=seed, gamma=-1.0, gamma_scale=0.5, score_mode="state", z=1.0, max_gap_bins=0)
        views = b.dwb_panel(threshold_z_grid=ess.resolve_z_grid(2.0, grid), bandwidths=spans, num_bootstrap=9, random_seed=seed,
                            calibration_quantile=0.9)
        # planted scores and masks: enough short peaks for a policy to be learned, and (wide) children of 7500 bp and more
        for c, n in enumerate(lens):
            s, mask = _plant(n, 40 + c, wide and c == 0)
            b.upload_scores(c, s)
            b.upload_solution(c, mask)
            first[c]["starts"], first[c]["ends"] = b.rocco_runs(c)
        nested = driver.nested_peaks_batch(b, first, interval_bp=step)
        before = _resident(b, 2)
        scores, masks = before[1], before[2]
        exported = driver.export_peaks_batch(b, nested, interval_bp=step, chroms=names, prefix="cs", use_uncertainty=False)
        cleaned, policy = driver.cleanup_peaks_batch(b, exported, interval_bp=step, chroms=names, use_uncertainty=False)
        widths = [m_["end"] - m_["start"] for r in exported for m_ in r["peak_meta"]]
        print("kept", len(widths), "widest", max(widths) if widths else None, "policy", policy)
        assert T.differences(policy, T_policy(widths)) == [] and list(policy) == list(T_policy(widths))
        assert len(widths) >= 25 and bool(policy["active"]) is wide
        for c in range(2):
            iv = np.arange(lens[c], dtype=np.int64) * step
            x, _ = _tracks(b, c)
            r = cleaned[c]
            if wide:
                want = T.rows(names[c], iv, iv + step, x, scores[c], masks[c], "consenrichROCCO", 0.5, trimScoreFloor=0.0,
                              subpeakSelectionPenalty=nested[c]["selection_penalty"], subpeakBoundaryCost=0.25 * nested[c]["gamma"],
                              minSubpeakBins=5, massiveSubpeakCleanup=True, massiveSubpeakWidthPolicy=policy, returnExportDetails=True,
                              form="steps")
                assert T.differences((r["rows"], r["peak_meta"], r["export_details"]), want) == [], c
                assert r["starts"].tolist() == [q["start_idx"] for q in want[1]] and r["ends"].tolist() == [q["end_idx"] for q in want[1]]
            else:       # the pass-through branch: the first pass's records, the policy in the details
                assert r["rows"] == exported[c]["rows"] and T.differences(r["peak_meta"], exported[c]["peak_meta"]) == []
                assert r["export_details"] == dict(exported[c]["export_details"], massive_subpeak_width_policy=policy)
                assert r["export_details"]["massive_subpeak_width_policy"] is not policy
                assert np.array_equal(r["starts"], exported[c]["starts"])
            assert r["gamma"] == nested[c]["gamma"]
        if wide:
            assert sum(r["export_details"]["num_massive_subpeak_candidates"] for r in cleaned) >= 1
            assert any(not np.array_equal(r["starts"], e["starts"]) or not np.array_equal(r["ends"], e["ends"]) for r, e in zip(cleaned, exported))
        # the scorer takes the cleaned peaks
        got = driver.score_peaks_batch(b, cleaned, views, dependence_spans=spans, random_seed=seed, num_replay=replays)
        direct = b.dwb_peak_scoring(views, bandwidths=spans, peaks=[(r["starts"], r["ends"]) for r in cleaned], num_replay=replays,
                                    random_seed=seed)
        for c in range(2):
            assert TNP.TN.differences(got[c], direct[c]) == [], c
        _unchanged(b, before)


def T_policy(widths):
    """the policy the reference learns from these widths: the package's host drop-in, held equal to it by the policy fixtures"""
    from consenrich_amd import cleanup as K

    return K.learn_massive_subpeak_width_policy(widths)
