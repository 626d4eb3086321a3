"""GPU tests of the post-fit scans, compactions and sums past their first carry round and their first grid block (run with -m gpu).
The shapes come from tests/second_level_cases.py, which derives every size from the constant that decides it;
tests/test_second_level_refs.py proves on the CPU that they reach what they claim and holds the references equal to each other.
Every comparison is exact: integers with ==, floats by their 64-bit patterns, text byte for byte.

  A  run bounds of a planted resident mask of 2^20, 2^20 + 1, 2^20 + 1025 and 2 * 2^20 + 1 bins (one, two and three rounds of
     k_rocco_run_scan), more than 65 536 runs through the second call of DeviceBatch.rocco_runs, the capacity guard of
     k_rocco_run_write through direct calls; references: tests/twin_rocco.cBooleanRunBounds and a derivation from the set bins;
  B  broad mode's support runs with 1023 .. 2049 runs and 63 .. 1025 kept ones, the envelope fallback with 1500 runs, 1026 coordinate
     breaks, 2^20 + 1025 bins, and 2 * 2^20 + 1025 bins (a third round of k_broad_scan); references: tests/twin_broad.parents and NumPy's own sums of the gaps;
  C  the bedGraph text and the bigWig body of one planted track of 2^20 + 1025 rows; references: the reference's pandas call
     (oracle/writers.py) and tests/writer_refs.py; the text of 2 * 2^20 + 1 rows (a third round);
  D  the null of tracks of 64 * 8192 + 1 and 2 * 64 * 8192 + 1 values (a second and a third grid block of k_np_chunk_sums) against
     tests/twin_null.py, alone and in a batch beside short chains; the nested refinement's selected sum of 64 * 8192 + 1 gathered
     values against np.sum;
  E  what the audit of DESIGN.md 9b added: a DWB panel with 65 (chunk, z) pairs for k_dwb_tail, the null of 66 tracks in one call,
     the scores of 65 segments, narrowPeak rows of 66 parents and more than 64 children,
     ESS scans alive into the third round of lags and past the last doubling."""
import ctypes as C

import numpy as np
import pytest

import cases
import second_level_cases as SC
import twin_broad as TB
import twin_null as TN
import twin_rocco
import writer_refs as wr
from conftest import gpu_available

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def product():
    if not gpu_available():
        pytest.fail("GPU tests selected but no HIP device / library: the product has no CPU fallback")
    from consenrich_amd import cconsenrich

    return cconsenrich


def _bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


# ---------------------------------------------------------------------------------------------------------------------------
# A. run bounds of a resident mask
# ---------------------------------------------------------------------------------------------------------------------------
RUN_CHAINS = SC.RUN_LENGTHS + (SC.LOOK_BEHIND["n"], SC.DIRECT_LENGTHS[0])
RUN_CASES = SC.run_cases()


@pytest.fixture(scope="module")
def run_batch(product):
    """a batch that is configured but never fitted; one solve of the shortest chain makes the mask buffers, every mask is planted"""
    from consenrich_amd.batch import DeviceBatch, ModelParams

    b = DeviceBatch(0)
    b.configure(ModelParams(state_dim=2), 2, list(RUN_CHAINS))
    small = len(RUN_CHAINS) - 1
    b.upload_scores(small, np.random.default_rng(5).normal(0.0, 1.0, RUN_CHAINS[small]))
    b.rocco(gamma=0.1, selection_penalty=0.2, chains=[c == small for c in range(len(RUN_CHAINS))])
    yield b
    b.close()


def _same_runs(got, mask, gap, tag):
    assert got[0].dtype == np.int64 and got[1].dtype == np.int64, tag
    for name, ref in (("twin", twin_rocco.cBooleanRunBounds(mask, gap)), ("set bins", SC.run_bounds_numpy(mask, gap))):
        assert got[0].size == ref[0].size, (tag, name, got[0].size, ref[0].size)
        for side in (0, 1):
            bad = np.flatnonzero(got[side] != ref[side])
            assert bad.size == 0, (tag, name, ("starts", "ends")[side], bad[:5].tolist(), got[side][bad[:5]].tolist(), ref[side][bad[:5]].tolist())


@pytest.mark.parametrize("name,n,kind,gaps", RUN_CASES, ids=[c[0] for c in RUN_CASES])
def test_run_bounds_past_the_first_carry_round(run_batch, name, n, kind, gaps):
    b = run_batch
    chain = RUN_CHAINS.index(n)
    mask = SC.run_mask(kind, n)
    b.upload_solution(chain, mask)
    assert np.array_equal(b.rocco_solution(chain), mask)
    for gap in gaps:
        _same_runs(b.rocco_runs(chain, gap), mask, gap, (name, gap))
    if kind == "every_second" and n == SC.RUN_LENGTHS[-1]:
        assert b.rocco_runs(chain, 0)[0].size == (n + 1) // 2 > SC.RUNS_CAP       # the second call, with the counted capacity


def test_the_look_behind_of_a_start_past_a_whole_block(run_batch):
    b = run_batch
    chain, gap = RUN_CHAINS.index(SC.LOOK_BEHIND["n"]), SC.LOOK_BEHIND["max_gap_bins"]
    mask = SC.look_behind_mask()
    b.upload_solution(chain, mask)
    for g in (gap - 1, gap, gap + 1, 0):
        _same_runs(b.rocco_runs(chain, g), mask, g, g)
    assert b.rocco_runs(chain, gap)[0].size == 2


@pytest.mark.parametrize("n,kind", [(SC.DIRECT_LENGTHS[0], "random"), (SC.DIRECT_LENGTHS[1], "across"), (SC.DIRECT_LENGTHS[1], "every_second")])
def test_the_capacity_guard_of_the_run_writer(run_batch, n, kind):
    """csr_batch_rocco_runs itself: the count without buffers, a capacity below the count, buffers one element longer than the
    capacity"""
    from consenrich_amd import _lib as L

    b = run_batch
    chain = RUN_CHAINS.index(n)
    mask = SC.run_mask(kind, n, seed=3)
    b.upload_solution(chain, mask)
    f = b._lib.csr_batch_rocco_runs
    for gap in (0, 1):
        rs, re = SC.run_bounds_numpy(mask, gap)
        count = int(rs.size)
        assert count >= 1
        cnt = C.c_int64(-1)
        L.check(f(b._ctx, chain, gap, 0, C.byref(cnt), None, None))
        assert cnt.value == count, (gap, "count only")
        for cap in sorted({1, count // 2, count - 1, count, count + 3} - {0}):
            starts, ends = np.full(cap + 1, -7, np.int64), np.full(cap + 1, -9, np.int64)
            cnt = C.c_int64(-1)
            L.check(f(b._ctx, chain, gap, cap, C.byref(cnt), starts.ctypes.data_as(L.I64P), ends.ctypes.data_as(L.I64P)))
            take = min(cap, count)
            assert cnt.value == count, (gap, cap)
            assert np.array_equal(starts[:take], rs[:take]) and np.array_equal(ends[:take], re[:take]), (gap, cap)
            assert np.all(starts[take:] == -7) and np.all(ends[take:] == -9), (gap, cap)      # the sentinel and everything past the count


# ---------------------------------------------------------------------------------------------------------------------------
# B. support runs of broad mode
# ---------------------------------------------------------------------------------------------------------------------------
BROAD = SC.broad_chains()
BROAD_NAMES = [ch["name"] for ch in BROAD]


@pytest.fixture(scope="module")
def broad_reference():
    """per chain (the twin's parents in the reference's steps, the kept records): computed once, left unchanged"""
    return {ch["name"]: (TB.parents(**ch["kw"]), SC.kept_records(ch["kw"])) for ch in BROAD}


@pytest.fixture(scope="module")
def broad_batch(product):
    """resident chains with planted scores, strong and weak masks; the fit beneath them is there for broadpeak_rows alone, which
    fills the resident parent mask"""
    from consenrich_amd import _lib as L
    from consenrich_amd.batch import DeviceBatch, ModelParams

    lens = [ch["kw"]["scores"].size for ch in BROAD]
    b = DeviceBatch(0)
    b.configure(ModelParams(state_dim=2), 2, lens)
    for c, n in enumerate(lens):
        b.upload(c, *cases.synth(n, 2, 7700 + c))
    b.stats()
    b.forward_backward(L.RETURN_NLL)
    b.export(L.EXPORT_FORWARD | L.EXPORT_SMOOTH)
    for c, ch in enumerate(BROAD):
        b.upload_scores(c, ch["kw"]["scores"])
    b.rocco(gamma=0.5, selection_penalty=0.2, chains=[c == 0 for c in range(len(lens))])
    for c, ch in enumerate(BROAD):
        b.upload_solution(c, ch["kw"]["strong"])
        b.upload_weak_solution(c, ch["kw"]["weak"])
    common = dict(intervals=[ch["kw"]["intervals"] for ch in BROAD], ends=[ch["kw"]["ends"] for ch in BROAD], chroms=BROAD_NAMES)
    got = b.broad_parents([ch["kw"]["threshold"] for ch in BROAD], [ch["kw"]["selection_penalty"] for ch in BROAD],
                          [ch["kw"]["boundary_cost"] for ch in BROAD], max_gap_bp=[ch["kw"]["max_gap_bp"] for ch in BROAD], run_penalty=0.0,
                          **common)
    yield b, got, common
    b.close()


@pytest.mark.parametrize("c", range(len(BROAD)), ids=BROAD_NAMES)
def test_broad_parents_past_the_first_workgroup_of_runs(broad_batch, broad_reference, c):
    import broad_cases as BC

    _, got, _ = broad_batch
    g, want = got[c], broad_reference[BROAD_NAMES[c]][0]
    assert (g["weak_support_run_count"], g["weak_support_touching_run_count"], g["envelope_fallback"]) == \
           (want["weak_support_run_count"], want["weak_support_touching_run_count"], want["envelope_fallback"])
    assert g["starts"].size == len(want["starts"])
    bad = [k for k in range(len(want["starts"])) if (g["starts"][k], g["ends"][k]) != (want["starts"][k], want["ends"][k])]
    assert bad == [], (bad[:5], [(int(g["starts"][k]), int(g["ends"][k]), want["starts"][k], want["ends"][k]) for k in bad[:5]])
    assert BC.differences(BC.canon(g["merge_details"]), BC.canon(want["merge_details"])) == []
    filled = np.zeros(want["mask"].size, np.uint8)
    for a, e in zip(g["starts"].tolist(), g["ends"].tolist()):
        filled[a:e + 1] = 1
    assert np.array_equal(filled, want["mask"])


def test_the_kept_records_of_every_chain(broad_batch, broad_reference):
    """csr_batch_broad_runs + csr_batch_broad_runs_fetch themselves: the three counts, every kept run, its gap sum by bit pattern"""
    from consenrich_amd import broad as B

    b, _, _ = broad_batch
    nc = len(BROAD)
    cfg = np.zeros(nc, B.RUN_CFG)
    breaks, n_breaks = [], np.zeros(nc, np.int64)
    for c, ch in enumerate(BROAD):
        kw = ch["kw"]
        cfg[c] = (kw["threshold"], kw["selection_penalty"], kw["dip_penalty_fraction"], B.max_gap_bins(kw["intervals"], kw["ends"], kw["max_gap_bp"]))
        br = np.flatnonzero(kw["ends"][:-1] != kw["intervals"][1:]).astype(np.int64)
        breaks.append(br)
        n_breaks[c] = br.size
    flat = np.ascontiguousarray(np.concatenate(breaks), np.int64)
    counts, rec = B._device_run_records(b, cfg, None, n_breaks, flat)
    first = np.searchsorted(rec["chain"], np.arange(nc + 1), "left")
    assert first[-1] == rec.size and np.all(rec["reserved"] == 0)
    for c, name in enumerate(BROAD_NAMES):
        support, fallback, want = broad_reference[name][1]
        mine = rec[first[c]:first[c + 1]]
        assert (int(counts[c]["support_runs"]), int(counts[c]["touching_runs"]), bool(counts[c]["fallback"])) == (support, len(want), fallback), name
        assert mine.size == len(want), name
        ws, we, wg = (np.asarray([r[k] for r in want]) for k in range(3))
        bad = np.flatnonzero((mine["start"] != ws) | (mine["end"] != we) | (_bits(mine["gap_sum"]) != _bits(wg)))
        assert bad.size == 0, (name, bad[:5].tolist(), mine[bad[:5]].tolist(), [want[k] for k in bad[:5].tolist()])
        assert np.all(mine["chain"] == c), name


def test_the_resident_parent_mask_of_every_chain(broad_batch, broad_reference):
    b, _, common = broad_batch
    b.broadpeak_rows(prefix="bp", **common)
    for c, name in enumerate(BROAD_NAMES):
        assert np.array_equal(b.broad_parent_solution(c), broad_reference[name][0]["mask"]), name


# ---------------------------------------------------------------------------------------------------------------------------
# C. writers
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted(product):
    """a batch whose "kappa" array takes planted values: (batch, plant) with plant(finite_only) -> the values"""
    from consenrich_amd import _lib as L
    from consenrich_amd.batch import DeviceBatch, ModelParams

    m = 2
    b = DeviceBatch(0)
    b.configure(ModelParams(state_dim=2), m, [SC.WRITER_ROWS, SC.WRITER_ROWS_3])
    for c, n in enumerate((SC.WRITER_ROWS, SC.WRITER_ROWS_3)):
        b.upload(c, np.zeros((m, n), np.float32), np.ones((m, n), np.float32))
    b.upload_multipliers(1, kappa=SC.writer_values(False, SC.WRITER_ROWS_3))       # (chain 1: the third round, text only)

    def plant(finite_only):
        v = SC.writer_values(finite_only)
        b.upload_multipliers(0, kappa=v)
        b.export(L.EXPORT_MULT)
        assert np.array_equal(b.download(0, "kappa").view(np.uint32), v.view(np.uint32))
        return v

    yield b, plant
    b.close()


def test_bedgraph_text_past_the_first_round_of_block_sums(planted):
    from oracle import writers as ow

    b, plant = planted
    v = plant(False)
    n = len(v)
    end_cap = SC.WRITER_START0 + n * SC.WRITER_STEP - 37
    starts, ends = wr.fixed_intervals(n, SC.WRITER_START0, SC.WRITER_STEP, end_cap)
    assert ends[-1] == end_cap < 1 << 32
    with np.errstate(all="ignore"):
        ref = ow.bedgraph_bytes("chr7", starts, ends, v, None)
    got = b.bedgraph_bytes(0, "kappa", "chr7", SC.WRITER_START0, SC.WRITER_STEP, end_cap=end_cap, transform=None)
    if got != ref:
        g, r = got.split(b"\n"), ref.split(b"\n")
        bad = [k for k in range(min(len(g), len(r))) if g[k] != r[k]]
        pytest.fail(f"{len(got)} bytes for {len(ref)}, {len(g)} rows for {len(r)}: rows {bad[:5]}: {[(g[k], r[k]) for k in bad[:5]]}")


def test_bedgraph_text_into_a_third_round_of_block_sums(planted):
    """2 * 2^20 + 1 rows: the carry of the third round holds two rounds' totals"""
    from oracle import writers as ow

    b, plant = planted
    plant(False)
    v = SC.writer_values(False, SC.WRITER_ROWS_3)
    assert np.array_equal(b.download(1, "kappa").view(np.uint32), v.view(np.uint32))
    starts, ends = wr.fixed_intervals(len(v), SC.WRITER_START0, SC.WRITER_STEP, 0)
    with np.errstate(all="ignore"):
        ref = ow.bedgraph_bytes("chr7", starts, ends, v, None)
    got = b.bedgraph_bytes(1, "kappa", "chr7", SC.WRITER_START0, SC.WRITER_STEP)
    if got != ref:
        g, r = got.split(b"\n"), ref.split(b"\n")
        bad = [k for k in range(min(len(g), len(r))) if g[k] != r[k]]
        pytest.fail(f"{len(got)} bytes for {len(ref)}, {len(g)} rows for {len(r)}: rows {bad[:5]}: {[(g[k], r[k]) for k in bad[:5]]}")


def test_bigwig_body_with_more_than_1024_sections(planted):
    b, plant = planted
    v = plant(True)
    n = len(v)
    starts, ends = wr.fixed_intervals(n, SC.WRITER_START0, SC.WRITER_STEP, 0)
    piece = b.bigwig_track(0, "kappa", 5, SC.WRITER_START0, SC.WRITER_STEP, zoom_bases=[10 * SC.WRITER_STEP])
    wr.check_piece(piece, 5, starts, ends, v, [10], SC.WRITER_STEP, "second level")
    hdr = wr.section_headers(piece.sections, n)
    assert len(hdr) == -(-n // SC.SECTION_ITEMS) > 1024 and hdr[-1][7] == n - SC.SECTION_ITEMS * (len(hdr) - 1) and hdr[-1][2] == ends[-1]


# ---------------------------------------------------------------------------------------------------------------------------
# D. NumPy-order sums and the null at a second grid block
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def N(product):
    from consenrich_amd import null

    return null


def _drop_in(N, z, q=0.60):
    """The three host-array drop-ins composed as peaks.py:1153-1162 composes the reference's (as tests/test_gpu_null.py does)"""
    center, scale, details = N.estimateROCCONull(z, q)
    template, meta = N.prepare_null_residual_template(z, center, scale, q)
    return dict(null_center=center, null_scale=scale, details=details, template_meta=meta, template=template,
                decided_on_host=N.null_and_template(z, q)["decided_on_host"])


@pytest.mark.parametrize("n", SC.SUM_SIZES)
@pytest.mark.parametrize("kind", TN.KINDS)
def test_the_null_of_a_track_past_one_grid_block_of_chunk_sums(N, kind, n):
    z = TN.track(kind, n)
    got, ref = _drop_in(N, z), TN.plain_all(z)
    assert TN.same(got, ref), TN.first_difference(got, ref)
    assert not got["decided_on_host"]
    assert _bits(N.estimate_template_scale(ref["template"])) == _bits(TN.plain_scale(ref["template"]))


@pytest.mark.parametrize("n", SC.SUM_SIZES)
def test_sort_scale_and_a_given_template_past_one_grid_block(N, n):
    z = TN.track("gauss", n, seed=13)
    assert np.array_equal(_bits(N.sort_values(z)), _bits(np.sort(z)))
    x = z * 0.7
    assert _bits(N.estimate_template_scale(x)) == _bits(TN.plain_scale(x))
    t, meta = N.prepare_null_residual_template(z, 0.25, 1.5, 0.5)
    rt, rmeta = TN.plain_template(z, 0.25, 1.5, 0.5)
    assert np.array_equal(_bits(t), _bits(rt))
    assert {k: _bits(v).tobytes() for k, v in meta.items()} == {k: _bits(v).tobytes() for k, v in rmeta.items()}


def test_a_batch_with_short_jobs_in_a_grid_sized_for_a_long_one(N):
    from consenrich_amd.batch import DeviceBatch, ModelParams

    tracks = [TN.track(("gauss", "rounded")[c % 2], n, seed=51 + c) for c, n in enumerate(SC.NULL_CHAINS)]
    with DeviceBatch(0) as b:
        b.configure(ModelParams(state_dim=2), 2, list(SC.NULL_CHAINS))
        for c, z in enumerate(tracks):
            b.upload_scores(c, z)
        got = b.rocco_null()
        tmpls = [b.download_template(c) for c in range(len(tracks))]
        for c, z in enumerate(tracks):
            ref = TN.plain_all(z)
            res = dict(got[c], template=tmpls[c])
            assert TN.same(res, ref), (z.size, TN.first_difference(res, ref))
        assert _bits(b.null_pooled_scale()) == _bits(TN.plain_scale(np.concatenate(tmpls)))
        take = [False, True, True, False]
        assert _bits(b.null_pooled_scale(chains=take)) == _bits(TN.plain_scale(np.concatenate(tmpls[1:3])))


def test_the_selected_sum_of_one_value_past_a_grid_block(product):
    from consenrich_amd import nested
    from consenrich_amd.batch import DeviceBatch, ModelParams, _NestedBackend

    scores = SC.select_scores()
    n_runs, starts, ends = SC.selected_runs()
    want, k = [], 0
    for c, s in enumerate(scores):
        mask = np.zeros(s.size, bool)
        for a, e in zip(starts[k:k + n_runs[c]].tolist(), ends[k:k + n_runs[c]].tolist()):
            mask[a:e + 1] = True
        k += int(n_runs[c])
        want.append(float(np.sum(s[mask])))
    assert int(n_runs[0]) > 2000
    zeros = [np.zeros(s.size, np.uint8) for s in scores]
    host = nested.HostBackend(scores, [None, None], zeros).selected_sums([True, True], n_runs, starts, ends)
    assert np.array_equal(_bits(host), _bits(want)), (host.tolist(), want)
    # a short job alone in the grid of the long one's call before: the same sums chain by chain
    only = nested.HostBackend(scores, [None, None], zeros).selected_sums([True, True], np.asarray([0, n_runs[1]], np.int64),
                                                                         starts[n_runs[0]:].copy(), ends[n_runs[0]:].copy())
    assert _bits(only[1]) == _bits(want[1]) and only[0] == 0.0
    with DeviceBatch(0) as b:
        b.configure(ModelParams(state_dim=2), 2, list(SC.SELECT_CHAINS))
        for c, s in enumerate(scores):
            b.upload_scores(c, s)
        resident = _NestedBackend(b).selected_sums([True, True], n_runs, starts, ends)
        assert np.array_equal(_bits(resident), _bits(want)), (resident.tolist(), want)


# ---------------------------------------------------------------------------------------------------------------------------
# E. further thresholds of the audit
# ---------------------------------------------------------------------------------------------------------------------------
def test_the_panel_with_one_tail_pair_in_a_second_workgroup(product):
    """13 chunks of 8192 values and 5 z: 65 (chunk, z) pairs, one more than a workgroup of k_dwb_tail takes"""
    import twin_dwb
    from consenrich_amd import dwb

    score, tmpl = SC.tail_inputs()
    got = dwb.stationary_null_panel([score], [tmpl], [0.25], [0.8], threshold_z_grid=SC.TAIL_Z_GRID, bandwidths=[5], num_bootstrap=8,
                                    random_seed=21)
    ref = twin_dwb.panel(score, tmpl, 0.25, 0.8, z_grid=SC.TAIL_Z_GRID, bandwidth=5, num_bootstrap=8, seed=21)
    assert twin_dwb.same_panel(got[0], ref) == []


def test_the_null_of_more_tracks_than_a_workgroup_of_track_lanes(N):
    from consenrich_amd.batch import DeviceBatch, ModelParams

    tracks = [TN.track(("gauss", "rounded", "constant")[c % 3], n, seed=71 + c) for c, n in enumerate(SC.MANY_TRACKS)]
    with DeviceBatch(0) as b:
        b.configure(ModelParams(state_dim=2), 2, list(SC.MANY_TRACKS))
        for c, z in enumerate(tracks):
            b.upload_scores(c, z)
        got = b.rocco_null()
        tmpls = [b.download_template(c) for c in range(len(tracks))]
        for c, z in enumerate(tracks):
            ref = TN.plain_all(z)
            res = dict(got[c], template=tmpls[c])
            assert TN.same(res, ref), (c, z.size, TN.first_difference(res, ref))
            assert not got[c]["decided_on_host"], c
        assert _bits(b.null_pooled_scale()) == _bits(TN.plain_scale(np.concatenate(tmpls)))


def test_segment_scores_of_more_segments_than_a_workgroup_picks(product):
    import peakscore_cases as PC
    import twin_peakscore as TP
    from consenrich_amd import peakscore

    x, views = PC.track(), PC.view_sets()["views4"]
    st, en = SC.many_segments(x.size)
    got = peakscore.best_segment_scores(x, st, en, views)
    with np.errstate(all="ignore"):
        assert TP.same_details(got, [TP.best_score_steps(x, a, b, views) for a, b in zip(st, en)])


def test_narrowpeak_rows_of_more_parents_and_children_than_a_workgroup(product):
    """66 planted parents on a small fitted chain, more than 64 children: the second workgroup of k_export_prep / k_export_finish
    (one lane per parent), of the sub-peak programme's lanes, and of k_export_child (one lane per child)"""
    import twin_narrowpeak as TNP
    from consenrich_amd import _lib as L
    from consenrich_amd.batch import DeviceBatch, ModelParams

    kw = SC.many_parents()
    n = kw["scores"].size
    pen, gamma = SC.EXPORT_PENALTY, SC.EXPORT_GAMMA
    with DeviceBatch(0) as b:
        b.configure(ModelParams(state_dim=2), 2, [n])
        b.upload(0, *cases.synth(n, 2, 7800))
        b.stats()
        b.forward_backward(L.RETURN_NLL)
        b.export(L.EXPORT_FORWARD | L.EXPORT_SMOOTH)
        b.upload_scores(0, kw["scores"])
        b.rocco(gamma=0.5, selection_penalty=0.2)
        b.upload_solution(0, kw["solution"])
        x, u = b.download(0, "xs")[:, 0].astype(np.float64), np.sqrt(b.download(0, "Ps")[:, 0, 0]).astype(np.float64)
        common = dict(intervals=[kw["intervals"]], ends=[kw["ends"]], chroms=["chr1"], prefix="np")
        for unc in (True, False):
            got = b.narrowpeak_rows([pen], [gamma], use_uncertainty=unc, **common)[0]
            want = TNP.rows("chr1", kw["intervals"], kw["ends"], x, kw["scores"], kw["solution"], "np", 0.5, uncertainty=u if unc else None,
                            trimScoreFloor=0.0, subpeakSelectionPenalty=pen, subpeakBoundaryCost=0.25 * gamma, minSubpeakBins=5,
                            returnExportDetails=True, form="steps")
            assert TNP.differences((got["rows"], got["peak_meta"], got["export_details"]), want) == [], unc
            assert want[2]["num_candidate_segments"] > SC.EXPORT_LANES and got["decided_on_host"] is False
        assert len(want[0]) > SC.EXPORT_LANES           # without the filter every child is a row


@pytest.mark.parametrize("n", SC.ESS_RAMPS)
def test_an_ess_scan_alive_into_the_later_rounds_of_lags(product, n):
    """a ramp of 3501 values breaks in the third round of lags, one of 24 001 values in the sixth, the first of the capped size"""
    import twin_budget
    from consenrich_amd import ess

    x = SC.ess_ramp(n)
    got, ref = ess.cEstimateEffectiveSampleSize(x, n - 1), twin_budget.cEstimateEffectiveSampleSize(x, n - 1)
    assert _bits(got[0]) == _bits(ref[0]) and _bits(got[1]) == _bits(ref[1]) and int(got[2]) == int(ref[2]), (got, ref)
