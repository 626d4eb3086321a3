"""CPU: the case table of tests/second_level_cases.py reaches what it claims, and the references the GPU tests of
tests/test_gpu_second_level.py lean on agree with each other.  Everything is computed from the inputs; nothing here runs a kernel.

  * the sizes: more than 1024 blocks of 1024 (a second and a third carry round), more than 65 536 mask runs, more than 1024 support
    runs, more than 64 and more than 1024 kept runs, more than 1024 breaks, more than 64 chunks of 8192 values;
  * the two statements of `cBooleanRunBounds` (the twin's walk, the derivation from the set bins) on every mask of the table and on
    random ones;
  * the vectorised support runs against the twin's bin-by-bin form on every chain, the twin's two forms of `parents` against each
    other, and the branches the chains must take."""
import numpy as np
import pytest

import second_level_cases as SC
import twin_broad as TB
import twin_rocco

CHAINS = SC.broad_chains()


def _chain(name):
    return next(c for c in CHAINS if c["name"] == name)


def _blocks(n):
    return -(-n // SC.SCAN_BLOCK)


def _rounds(n):
    return -(-_blocks(n) // SC.SCAN_ROUND)


# ---------------------------------------------------------------------------------------------------------------
# A
# ---------------------------------------------------------------------------------------------------------------
def test_run_lengths_cross_the_carry_rounds():
    assert [_rounds(n) for n in SC.RUN_LENGTHS] == [1, 2, 2, 3]
    assert [_blocks(n) for n in SC.RUN_LENGTHS] == [SC.SCAN_ROUND, SC.SCAN_ROUND + 1, SC.SCAN_ROUND + 2, 2 * SC.SCAN_ROUND + 1]
    assert _blocks(SC.RUN_LENGTHS[1]) > 1024
    # every second bin of the longest chain: more runs than the first call of rocco_runs holds, and more than 2^19
    n_runs = SC.run_bounds_numpy(SC.run_mask("every_second", SC.RUN_LENGTHS[-1]))[0].size
    assert n_runs > SC.RUNS_CAP and n_runs > 65536 and n_runs > 1 << 19
    assert [_blocks(n) for n in SC.DIRECT_LENGTHS] == [3, SC.SCAN_ROUND + 1]
    assert SC.LOOK_BEHIND["max_gap_bins"] > SC.SCAN_BLOCK


def test_the_sparse_masks_hold_their_edges():
    E = SC.ROUND
    for n in SC.RUN_LENGTHS[1:]:
        across, beside = SC.run_mask("across", n), SC.run_mask("beside", n)
        assert across[0] and across[n - 1] and beside[0] and beside[n - 1]
        assert across[E - 1] and across[E]
        if n > E + 2:
            assert beside[E - 1] and not beside[E] and beside[E + 1]
            # the start at E + 1 looks behind across the round edge: alone at gap 0, fused with the run in front from gap 1 on
            assert E + 1 in SC.run_bounds_numpy(beside, 0)[0] and E + 1 not in SC.run_bounds_numpy(beside, 1)[0]
        st, en = SC.run_bounds_numpy(across, 0)
        k = int(np.searchsorted(st, E, "right")) - 1
        assert st[k] < E <= en[k] and k > 1000          # a run over the edge, a thousand runs in front of it
    third = SC.run_mask("across", SC.RUN_LENGTHS[-1])
    assert third[2 * E - 1] and third[2 * E]


@pytest.mark.parametrize("name,n,kind,gaps", SC.run_cases(), ids=[c[0] for c in SC.run_cases()])
def test_the_two_run_bound_references_agree(name, n, kind, gaps):
    mask = SC.run_mask(kind, n)
    for gap in gaps:
        a, b = twin_rocco.cBooleanRunBounds(mask, gap), SC.run_bounds_numpy(mask, gap)
        assert b[0].dtype == np.int64 and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), gap


def test_the_two_run_bound_references_agree_on_small_and_random_masks():
    mask = SC.look_behind_mask()
    gap = SC.LOOK_BEHIND["max_gap_bins"]
    for g in (0, gap - 1, gap, gap + 1, -3):
        a, b = twin_rocco.cBooleanRunBounds(mask, g), SC.run_bounds_numpy(mask, g)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), g
    assert SC.run_bounds_numpy(mask, gap)[0].tolist() == [0, 700 + 2 * (gap + 1) + 1]      # (the gap of gap + 2 bins alone cuts)
    for seed, n in enumerate((1, 2, 3, 64, 1023, 1024, 1025, 5003, 70001)):
        m = SC.run_mask("random", n, seed)
        for g in (0, 1, 3, 7):
            a, b = twin_rocco.cBooleanRunBounds(m, g), SC.run_bounds_numpy(m, g)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (n, g)
    for m in (np.zeros(9, np.uint8), np.ones(9, np.uint8)):
        a, b = twin_rocco.cBooleanRunBounds(m, 2), SC.run_bounds_numpy(m, 2)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---------------------------------------------------------------------------------------------------------------
# B
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def device_form():
    """per chain the twin's device form (walked bin by bin) with its branches"""
    out = {}
    for ch in CHAINS:
        TB.reset_branches()
        got = TB.parents(form="device", **ch["kw"])
        out[ch["name"]] = (got, dict(TB.BRANCHES))
    TB.reset_branches()
    return out


def test_the_chains_take_the_second_level(device_form):
    total = {}
    for _, br in device_form.values():
        for k, v in br.items():
            total[k] = total.get(k, 0) + v
    assert [k for k in SC.NEEDED_SECOND_LEVEL if not total.get(k)] == [], total
    counts = {name: (got["weak_support_run_count"], got["weak_support_touching_run_count"], got["envelope_fallback"])
              for name, (got, _) in device_form.items()}
    K, W = SC.SCAN_BLOCK, SC.GAP_WAVE
    assert counts["runs_1023"] == (K - 1, W - 1, False) and counts["runs_1024"] == (K, W, False)
    assert counts["runs_1025"] == (K + 1, W + 1, False) and counts["runs_2049"] == (2 * K + 1, K + 1, False)
    assert counts["envelope_1500"] == (0, 1500, True)
    assert counts["breaks"][0] > 1100 + 1000 and counts["breaks"][1] > W and not counts["breaks"][2]
    assert counts["long"][0] > K and counts["long"][1] > W and counts["long3"][0] > 2 * K and counts["long3"][1] > W
    # where each branch is taken
    assert device_form["runs_1025"][1].get("support_runs_over_block") and not device_form["runs_1024"][1].get("support_runs_over_block")
    assert device_form["runs_1025"][1].get("kept_runs_over_wave") and not device_form["runs_1024"][1].get("kept_runs_over_wave")
    assert device_form["runs_2049"][1].get("kept_runs_over_block") and device_form["envelope_1500"][1].get("kept_runs_over_block")
    assert device_form["long"][1].get("bins_over_carry_round") and device_form["breaks"][1].get("breaks_over_block")
    assert -(-_chain("long")["kw"]["scores"].size // K) > 1024
    assert _rounds(_chain("long")["kw"]["scores"].size) == 2 and _rounds(_chain("long3")["kw"]["scores"].size) == 3


def test_kept_and_dropped_runs_on_both_sides_of_the_second_workgroup():
    K = SC.SCAN_BLOCK
    for name in ("runs_1025", "runs_2049"):
        ch = next(c for c in CHAINS if c["name"] == name)
        kw = ch["kw"]
        support, kept = SC.kept_runs_numpy(kw["scores"], kw["weak"], kw["strong"], kw["threshold"], kw["intervals"], kw["ends"])
        kept = set(kept)
        assert support[K - 1] in kept and support[K] in kept            # the last of workgroup 0, the first of workgroup 1
        assert support[K - 2] not in kept and (len(support) == K + 1 or support[K + 1] not in kept)
    ch = next(c for c in CHAINS if c["name"] == "breaks")
    iv, en = ch["kw"]["intervals"], ch["kw"]["ends"]
    breaks = np.flatnonzero(en[:-1] != iv[1:])
    s = ch["kw"]["scores"] >= ch["kw"]["threshold"]
    assert breaks.size >= 1025
    assert not s[breaks[0]] and s[breaks[0] + 1] and s[breaks[-1]] and not s[breaks[-1] + 1]       # on a run's edge
    assert np.count_nonzero(s[breaks] & s[breaks + 1]) >= 1024                                      # inside a run


@pytest.mark.parametrize("name,E", [("long", SC.ROUND), ("long3", SC.ROUND), ("long3", 2 * SC.ROUND)])
def test_the_long_chains_hold_their_edges(name, E):
    ch = _chain(name)
    kw = ch["kw"]
    n = kw["scores"].size
    assert n == (E if name == "long" else 2 * SC.ROUND) + SC.SCAN_BLOCK + 1
    support, fallback, rec = SC.kept_records(kw)
    assert not fallback
    runs, _ = SC.kept_runs_numpy(kw["scores"], kw["weak"], kw["strong"], kw["threshold"], kw["intervals"], kw["ends"])
    across = [r for r in runs if r[0] < E <= r[1]]
    assert across == [(E - 3, E + 2)] and all(r[:2] != across[0] for r in rec)          # a support run over the edge, not kept
    k = max(i for i, r in enumerate(rec) if r[1] < E)
    left, right = rec[k], rec[k + 1]
    assert left[1] < E - 3 and right[0] > E + 2 and left[2] != 0.0                      # the gap spans the edge and is summed
    bound = kw["max_gap_bp"] // 25
    gaps = [b[0] - a[1] - 1 for a, b in zip(rec[:-1], rec[1:])]
    assert right[0] - left[1] - 1 <= bound and sum(g > bound for g in gaps) >= 1
    assert all(r[2] == 0.0 for r, g in zip(rec, gaps) if g > bound)
    assert rec[0][0] == 0 and rec[-1][1] == n - 1 and rec[-1][0] // SC.SCAN_BLOCK != rec[-1][1] // SC.SCAN_BLOCK


@pytest.mark.parametrize("chain", CHAINS, ids=[c["name"] for c in CHAINS])
def test_the_vectorised_support_runs_equal_the_twins(chain, device_form):
    kw = chain["kw"]
    env = (kw["weak"] > 0) | (kw["strong"] > 0)
    breaks = np.flatnonzero(kw["ends"][:-1] != kw["intervals"][1:]).tolist()
    n = kw["scores"].size
    for envelope in (False, True):
        if n > SC.ROUND and envelope:
            continue                # (the long chain's envelope runs are not what any test reads)
        want = TB._device_kept_runs(kw["scores"], env, float(kw["threshold"]), breaks, n, envelope)
        got = SC.kept_runs_numpy(kw["scores"], kw["weak"], kw["strong"], kw["threshold"], kw["intervals"], kw["ends"], envelope)
        assert got[0] == want[0] and got[1] == want[1], envelope
    TB.reset_branches()
    # the records' runs are the runs the twin bridges; its two forms agree on the result
    got, _ = device_form[chain["name"]]
    support, fallback, rec = SC.kept_records(kw)
    assert (support, len(rec), fallback) == (got["weak_support_run_count"], got["weak_support_touching_run_count"], got["envelope_fallback"])
    steps = TB.parents(form="steps", **kw)
    for key in ("starts", "ends", "merge_details", "weak_support_run_count", "weak_support_touching_run_count", "envelope_fallback"):
        assert steps[key] == got[key], key
    assert np.array_equal(steps["mask"], got["mask"])


def test_summed_gaps_lie_in_the_second_workgroup_of_the_gap_sums():
    """runs_1025 holds the issue's count of 65 kept runs, but the 65th is the last one and its gap sum is 0.0 by definition: the
    second workgroup of k_broad_run_gaps is held to a value by the chains with a summed gap at kept index 64 or beyond"""
    W = SC.GAP_WAVE
    beyond = {ch["name"]: sum(1 for r in SC.kept_records(ch["kw"])[2][W:] if r[2] != 0.0) for ch in CHAINS}
    assert beyond["runs_1025"] == 0
    assert beyond["runs_2049"] > 100 and beyond["envelope_1500"] > 100 and beyond["long"] >= 1 and beyond["long3"] >= 1


def test_the_gaps_of_the_table_are_decided_both_ways(device_form):
    merged = sum(got["merge_details"].get("num_gaps_merged", 0) for got, _ in device_form.values())
    far = sum(got["merge_details"].get("num_gaps_blocked_by_distance", 0) for got, _ in device_form.values())
    open_ = sum(got["merge_details"].get("num_gaps_evaluated", 0) for got, _ in device_form.values())
    assert merged > 100 and far > 100 and open_ - merged - far > 100
    long = device_form["long"][0]
    E = SC.ROUND
    assert any(a < E <= b for a, b in zip(long["starts"], long["ends"]))        # a bridged parent over the round edge


# ---------------------------------------------------------------------------------------------------------------
# C
# ---------------------------------------------------------------------------------------------------------------
def test_the_writer_track_crosses_the_round_edge():
    from test_oracle_writers import edge_values

    n = SC.WRITER_ROWS
    assert _blocks(n) == SC.SCAN_ROUND + 2 > 1024 and -(-n // SC.SECTION_ITEMS) > 1024
    assert _rounds(n) == 2 and _rounds(SC.WRITER_ROWS_3) == 3
    assert SC.WRITER_START0 + n * SC.WRITER_STEP < 1 << 32
    for finite_only in (False, True):
        v = SC.writer_values(finite_only)
        table = edge_values()
        table = table[np.isfinite(table)] if finite_only else table
        assert v.dtype == np.float32 and v.size == n and np.all(np.isfinite(v)) == finite_only
        assert set(v.view(np.uint32).tolist()) == set(table.view(np.uint32).tolist())
        assert len(table) % SC.SCAN_BLOCK
        # the literal head of the table (its longest and shortest texts) lies on both sides of the round edge
        head = np.flatnonzero(v.view(np.uint32) == table[:1].view(np.uint32)[0])
        assert head[0] < SC.ROUND < head[-1]


# ---------------------------------------------------------------------------------------------------------------
# D
# ---------------------------------------------------------------------------------------------------------------
def test_the_sums_reach_a_second_grid_block():
    for n in SC.SUM_SIZES + (max(SC.NULL_CHAINS),):
        assert -(-n // SC.NP_CHUNK) > SC.CHUNKS_PER_BLOCK > 0 and -(-n // SC.NP_CHUNK) > 64
    assert [-(-(-(-n // SC.NP_CHUNK)) // SC.CHUNKS_PER_BLOCK) for n in SC.SUM_SIZES] == [2, 3]
    assert min(SC.NULL_CHAINS) < SC.NP_CHUNK < sorted(SC.NULL_CHAINS)[1] < SC.SUM_BLOCK
    tiles = [-(-n // SC.NULL_TILE) for n in SC.SUM_SIZES]
    assert all(t > 64 and t & (t - 1) for t in tiles)           # neither small nor a power of two


def test_the_selection_gathers_one_value_into_the_second_block():
    n_runs, starts, ends = SC.selected_runs()
    s0, e0 = starts[:n_runs[0]], ends[:n_runs[0]]
    lens = e0 - s0 + 1
    assert np.all(s0[1:] > e0[:-1] + 1) and e0[-1] < SC.SELECT_CHAINS[0] and n_runs[0] > 2000
    assert int(lens.sum()) == SC.SUM_BLOCK + 1 and len(set(lens.tolist())) > 100
    gathered_end = np.cumsum(lens) - 1
    assert gathered_end[-2] == SC.SUM_BLOCK - 1 and gathered_end[-1] - lens[-1] + 1 == SC.SUM_BLOCK
    assert n_runs[1] == 3 and ends[-1] == SC.SELECT_CHAINS[1] - 1


# ---------------------------------------------------------------------------------------------------------------
# E
# ---------------------------------------------------------------------------------------------------------------
def test_the_further_cases_cross_their_thresholds():
    pairs = -(-SC.TAIL_BINS // SC.NP_CHUNK) * len(SC.TAIL_Z_GRID)
    assert pairs == SC.TAIL_PAIRS + 1 > 64                       # one (chunk, z) pair in the second workgroup of k_dwb_tail
    assert len(SC.MANY_TRACKS) > SC.TRACK_LANES == 64 and min(SC.MANY_TRACKS) >= 16     # (16: no track is decided on the host)
    import peakscore_cases as PC

    n = PC.track().size             # the track the GPU test scores
    st, en = SC.many_segments(n)
    assert st.size == SC.SEGMENT_LANES + 1 > 64 and np.all(en >= st) and en.max() < n


def test_the_export_case_holds_more_parents_and_children_than_a_workgroup():
    """the parents are the runs of the planted mask; the children come from the scores alone (the sub-peak programme reads nothing
    else), so the twin counts them here with a stand-in signal and no uncertainty: nothing is filtered"""
    import twin_narrowpeak as TNP

    kw = SC.many_parents()
    parents = SC.run_bounds_numpy(kw["solution"])[0].size
    assert parents == SC.EXPORT_LANES + 2 > 64
    rows, _, details = TNP.rows("chr1", kw["intervals"], kw["ends"], kw["state"], kw["scores"], kw["solution"], "np", 0.5,
                                trimScoreFloor=0.0, subpeakSelectionPenalty=SC.EXPORT_PENALTY,
                                subpeakBoundaryCost=0.25 * SC.EXPORT_GAMMA, minSubpeakBins=5, returnExportDetails=True, form="steps")
    assert details["num_candidate_segments"] > 64 and details["num_candidate_segments"] > parents      # some parent splits
    assert len(rows) == details["num_segments_kept"] == details["num_candidate_segments"]


def test_the_ramps_keep_their_scans_alive_into_the_later_rounds_of_lags():
    import twin_budget

    third = sum(SC.ESS_ROUNDS[:2]), sum(SC.ESS_ROUNDS[:3])          # the third round holds lags 768 .. 1791
    used = [twin_budget.cEstimateEffectiveSampleSize(SC.ess_ramp(n), n - 1)[2] for n in SC.ESS_RAMPS]
    assert third[0] <= used[0] < third[1]
    assert used[1] >= sum(SC.ESS_ROUNDS) and SC.ESS_ROUNDS[-1] == 4096         # past every doubling: a round of the capped size
