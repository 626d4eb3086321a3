"""Broad mode without a GPU: the new symbols and struct layouts, every argument check with the reference's message (they all come
before a device is touched), the two pure-host drop-ins against the fixtures, and the gap and parent routines of csrc/csr_broad.h
run on the CPU by a stand-alone program built with the address and undefined-behaviour sanitizers -- through the package's own
host half (coordinate breaks, the gap tests, the gain decision, blocks, assembly, the host decision), against the fixtures."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import broad_cases as BC  # noqa: E402

from consenrich_amd import _lib as L  # noqa: E402
from consenrich_amd import broad as B  # noqa: E402
from consenrich_amd import narrowpeak as P  # noqa: E402

ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden", "broad")
MERGE, ROWS = BC.merge_cases(), BC.rows_cases()


def golden(file, name):
    with np.load(os.path.join(GOLD, file)) as z:
        return BC.unpack(z[name])


def numpy_gap_sum(scores, penalty, fraction, start, length):
    """the reference's expression (peaks.py:1966-1979) of one gap"""
    if length <= 0:
        return 0.0
    ex = np.asarray(scores[start:start + length] - penalty, dtype=np.float64)
    return float(np.sum(np.where(ex < 0.0, fraction * ex, ex)))


def bits(a):
    return np.asarray(a, np.float64).view(np.uint64).tolist()


def test_symbols_and_struct_layouts():
    lib = L.lib()
    for name in ("csr_broad_gap_sums", "csr_broad_rows", "csr_batch_rocco_weak", "csr_batch_rocco_weak_upload",
                 "csr_batch_rocco_weak_download", "csr_batch_broad_parent_download", "csr_batch_broad_runs",
                 "csr_batch_broad_runs_fetch", "csr_batch_broad_rows"):
        assert hasattr(lib, name) and name in L.SYMBOLS
    assert lib.csr_abi_version() == 6
    for dt, st, size in ((B.CFG, L.BroadCfg, 16), (B.REC, L.BroadParent, 80), (B.PARENT, L.ExportParent, 24),
                         (B.RUN_CFG, L.BroadRunCfg, 32), (B.RUN_COUNTS, L.BroadRunCounts, 24), (B.RUN, L.BroadRun, 32)):
        assert dt.itemsize == C.sizeof(st) == size
        assert [(n, dt.fields[n][1]) for n in dt.names] == [(n, getattr(st, n).offset) for n, _ in st._fields_]
    with open(os.path.join(ROOT, "include", "consenrich_amd.h")) as fh:
        header = " ".join(fh.read().split())
    assert "CSR_BROAD_HAS_LOCAL_P = 1, CSR_BROAD_DROPPED_MEDIAN = 2, CSR_BROAD_NONFINITE = 4" in header
    assert (B.HAS_LOCAL_P, B.DROPPED_MEDIAN, B.NONFINITE) == (L.BROAD_HAS_LOCAL_P, L.BROAD_DROPPED_MEDIAN, L.BROAD_NONFINITE) == (1, 2, 4)
    assert "typedef struct csr_broad_parent { int64_t start, end, summit; /* bins of the chain */ int32_t chain, flags; double " \
           "median_state, local_median_p, max_state, max_score, mean_state, mean_score; } csr_broad_parent;" in header
    assert "typedef struct csr_broad_cfg { /* per chain */ double multiplier; int32_t filter, reserved; } csr_broad_cfg;" in header
    assert "typedef struct csr_broad_run { int64_t start, end; /* bins of the chain */ double gap_sum; int32_t chain, reserved; } " \
           "csr_broad_run;" in header
    assert "typedef struct csr_broad_run_counts { int64_t support_runs, touching_runs; int32_t fallback, reserved; } " \
           "csr_broad_run_counts;" in header
    assert "typedef struct csr_broad_run_cfg { /* per chain */ double threshold, selection_penalty, dip_fraction; int64_t max_gap_bins;" in header
    assert B.MIN_PEAK_BP == 1000 and B.MULTIPLIER == 2.0


def test_drop_in_argument_checks():
    good, errors = BC.rows_errors()
    for override, message in errors:
        with pytest.raises(ValueError) as e:
            B.solution_to_chrom_broadpeak_rows(**{**good, **override})
        assert str(e.value) == message, override
    good, errors = BC.merge_errors()
    for override, message in errors:
        with pytest.raises(ValueError) as e:
            B.merge_broad_runs_by_objective(**{**good, **override})
        assert str(e.value) == message, override
    with pytest.raises(ValueError) as e:
        B.selected_coordinate_run_bounds(np.ones(4), np.arange(4), np.arange(5))
    assert str(e.value) == "`intervals`, `ends`, and `mask` must match length"


def test_driver_argument_checks():
    """`solveRocco`'s checks of broadWeakThresholdZ and broadMaxGapBP, with its texts, before the batch is looked at"""
    from consenrich_amd import driver

    common = dict(dependence_spans=3, threshold_z=2.0, threshold_z_grid=(1.5, 2.0), num_bootstrap=4, random_seed=1, interval_bp=25)
    for kw, message in ((dict(weak_threshold_z=-0.1), "`broadWeakThresholdZ` must be finite and non-negative"),
                        (dict(weak_threshold_z=float("nan")), "`broadWeakThresholdZ` must be finite and non-negative"),
                        (dict(max_gap_bp=True), "`broadMaxGapBP` must be an integer or None"),
                        (dict(max_gap_bp=-1), "`broadMaxGapBP` must be a non-negative integer or None"),
                        (dict(max_gap_bp=2.5), "`broadMaxGapBP` must be a non-negative integer or None"),
                        (dict(weak_threshold_z=2.5), "`broadWeakThresholdZ` cannot exceed `thresholdZ`")):
        with pytest.raises(ValueError) as e:
            driver.broad_peaks_batch(None, [], **{**common, **kw})
        assert str(e.value) == message, kw
    assert driver.validate_broad_max_gap_bp(None) is None and driver.validate_broad_max_gap_bp(300.0) == 300


def test_library_argument_checks():
    """The library's own checks, called directly: the reference's text with CSR_ERR_VALUE, plain failures for what the reference has
    no word for, all with no device in sight."""
    n = 12
    x = np.linspace(-1.0, 1.0, n)
    lens = np.asarray([n], np.int64)

    def rows(mult=2.0, parents=((2, 9),)):
        cfg = np.asarray([(mult, 0, 0)], B.CFG)
        par = np.asarray([(a, b, c[0] if c else 0, 0) for a, b, *c in parents], B.PARENT)
        rec = np.zeros(par.size, B.REC)
        rc = L.lib().csr_broad_rows(1, L._i64p(lens), L.dp(x), L.dp(x), None, P._vp(cfg), par.size, P._vp(par), None, P._vp(rec))
        return rc, L.last_error()

    text = "`exportFilterUncertaintyMultiplier` must be finite and non-negative"
    assert rows(mult=-0.5) == (L.ERR_VALUE, text) and rows(mult=float("nan")) == (L.ERR_VALUE, text)
    assert rows(mult=float("inf")) == (L.ERR_VALUE, text)
    for parents, word in ((((3, 12),), "outside chain 0"), (((0, 5), (5, 9)), "disjoint and ascending"), (((5, 3),), "outside chain 0"),
                          (((0, 5, 1),), "chain index out of range"), (((-1, 3),), "outside chain 0")):
        rc, msg = rows(parents=parents)
        assert rc == -1 and word in msg, (parents, msg)

    def gaps(start, length):
        s, ln, out = np.asarray(start, np.int64), np.asarray(length, np.int64), np.zeros(len(start))
        rc = L.lib().csr_broad_gap_sums(n, L.dp(x), 0.5, 0.5, s.size, L._i64p(s), L._i64p(ln), L.dp(out))
        return rc, L.last_error(), out

    for start, length in (([3], [10]), ([-1], [2]), ([13], [0]), ([2], [-1]), ([0, 11], [1, 2])):
        rc, msg, _ = gaps(start, length)
        assert rc == -1 and "outside the scores" in msg, (start, length, msg)
    rc, _, out = gaps([0, 12, 5], [0, 0, 0])        # no bin in any gap: answered on the host
    assert rc == 0 and bits(out) == bits([0.0, 0.0, 0.0])


@pytest.mark.parametrize("name", [c["name"] for c in ROWS])
def test_host_drop_ins_match_the_reference(name):
    """`_selectedCoordinateRunBounds` of both masks and `_blocksForBroadParent` of every parent against ALL children"""
    kw = BC.case(ROWS, name)["kw"]
    pr = B.selected_coordinate_run_bounds(kw["parentSolution"], kw["intervals"], kw["ends"])
    cr = B.selected_coordinate_run_bounds(kw["childSolution"], kw["intervals"], kw["ends"])
    assert BC.differences(BC.canon((pr, cr)), golden("broad_host.npz", f"runs/{name}")) == []
    blocks = [B.blocks_for_broad_parent(a, b, cr, kw["intervals"], kw["ends"]) for a, b in pr]
    assert BC.differences(BC.canon(blocks), golden("broad_host.npz", f"blocks/{name}")) == []


@pytest.mark.parametrize("name", ["max_gap_zero", "one_run", "empty_soft", "empty_hard"])
def test_merges_that_need_no_sum(name):
    """No gap with a bin is left open: the library answers on the host, and the details take both of the reference's forms"""
    got = B.merge_broad_runs_by_objective(**BC.case(MERGE, name)["kw"])
    assert BC.differences(BC.canon(got), golden("broad_merge.npz", name)) == []


# ---------------------------------------------------------------------------------------------------------------
# the gap and parent routines on the CPU
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    tmp = tmp_path_factory.mktemp("broad")
    exe = str(tmp / "broad_host_check")
    subprocess.check_call([hipcc, "-O1", "-g", "--offload-arch=gfx950", "-ffp-contract=off", "-std=c++17", "-Xarch_host",
                           "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(HERE, "native", "broad_host_check.hip")])
    return exe, str(tmp)


def _run(exe, tmp, scores, state, uncertainty, penalty, fraction, multiplier, gaps, parents, runs=None):
    """runs: None, or (threshold, breaks, strong, weak, max_gap_bins) for the support-run stage"""
    src, dst = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    n = int(scores.size)
    gaps, parents = np.asarray(gaps, np.int64).reshape(-1, 2), np.asarray(parents, np.int64).reshape(-1, 2)
    threshold, breaks, strong, weak, bound = (0.0, np.zeros(0, np.int64), None, None, -1) if runs is None else runs
    with open(src, "wb") as fh:
        fh.write(np.asarray([n, len(gaps), len(parents), int(uncertainty is not None), len(breaks), int(runs is not None), bound],
                            np.int64).tobytes())
        fh.write(np.asarray([penalty, fraction, multiplier, threshold], np.float64).tobytes())
        for a in (scores, np.zeros(n) if state is None else state, np.zeros(n) if uncertainty is None else uncertainty):
            fh.write(np.ascontiguousarray(a, np.float64).tobytes())
        fh.write(gaps.tobytes())
        fh.write(parents.tobytes())
        if runs is not None:
            fh.write(np.ascontiguousarray(breaks, np.int64).tobytes())
            fh.write(np.ascontiguousarray(strong, np.uint8).tobytes())
            fh.write(np.ascontiguousarray(weak, np.uint8).tobytes())
    subprocess.check_call([exe, src, dst], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    with open(dst, "rb") as fh:
        buf = fh.read()
    sums = np.frombuffer(buf, np.float64, len(gaps)).copy()
    rec = np.frombuffer(buf, B.REC, len(parents), 8 * len(gaps)).copy()
    at = 8 * len(gaps) + B.REC.itemsize * len(parents)
    mask = np.frombuffer(buf, np.uint8, n, at).copy()
    if runs is None:
        return sums, rec, mask
    support, kept, fallback = np.frombuffer(buf, np.int64, 3, at + n).tolist()
    return (support, kept, fallback), np.frombuffer(buf, B.RUN, kept, at + n + 24).copy()


def cpu_gap_sums(exe, tmp):
    def run(scores, penalty, fraction, starts, lens):
        return _run(exe, tmp, scores, None, None, penalty, fraction, 0.0, np.stack([starts, lens], 1), [])[0]
    return run


def cpu_records(exe, tmp):
    def run(state, scores, uncertainty, multiplier, ps, pe):
        _, rec, mask = _run(exe, tmp, scores, state, uncertainty, 0.0, 0.0, multiplier, [], np.stack([ps, pe], 1))
        return rec, mask
    return run


@pytest.mark.parametrize("name", [c["name"] for c in MERGE])
def test_merge_on_the_cpu_matches_the_reference(host_check, monkeypatch, name):
    monkeypatch.setattr(B, "_device_gap_sums", cpu_gap_sums(*host_check))
    got = B.merge_broad_runs_by_objective(**BC.case(MERGE, name)["kw"])
    assert BC.differences(BC.canon(got), golden("broad_merge.npz", name)) == []


@pytest.mark.parametrize("fraction", [0.5, 1.0, 0.25])
def test_gap_sums_on_the_cpu_equal_numpy(host_check, fraction):
    """Every gap length of the table -- the leaf, the eight accumulators, the first split, the chunk fold -- and a gap without a bin,
    against the reference's own NumPy expression, bit for bit.  (A fraction of 0 turns every bin below the penalty into -0.0, and a
    sum of nothing but -0.0 carries a zero's sign that the gain, which adds 2 * boundaryCost >= +0.0 to it, never shows: the
    decisions under a fraction of 0 are the case gap_lengths_below_zero)"""
    kw = BC.case(MERGE, "gap_lengths_soft")["kw"]
    rs, re = np.asarray(kw["runs"], np.int64).T
    starts, lens = re[:-1] + 1, rs[1:] - re[:-1] - 1
    assert sorted(lens.tolist()) == sorted(BC.GAP_LENGTHS + (0,))
    got = cpu_gap_sums(*host_check)(kw["scores"], 0.5, fraction, starts, lens)
    want = [numpy_gap_sum(kw["scores"], 0.5, fraction, a, k) for a, k in zip(starts.tolist(), lens.tolist())]
    assert bits(got) == bits(want)


@pytest.mark.parametrize("name", [c["name"] for c in ROWS])
def test_rows_on_the_cpu_match_the_reference(host_check, monkeypatch, name):
    """The drop-in with the library's parent routine run on the CPU in place of the device call"""
    seen = {}
    run = cpu_records(*host_check)

    def records(state, scores, uncertainty, multiplier, ps, pe):
        seen["rec"], seen["mask"] = run(state, scores, uncertainty, multiplier, ps, pe)
        return seen["rec"].copy(), seen["mask"]

    monkeypatch.setattr(B, "_device_records", records)
    before = dict(B.STATS)
    kw = BC.case(ROWS, name)["kw"]
    with np.errstate(invalid="ignore"):
        got = B.solution_to_chrom_broadpeak_rows(**kw)
    assert BC.differences(BC.canon(got), golden("broad_rows.npz", name)) == []
    # the cap on host decisions: the NaN chain and no other
    assert B.STATS["decided_on_host"] - before["decided_on_host"] == int(name in BC.HOST_DECIDED)
    if "mask" in seen:      # the parent fill: the parent mask back (coordinate breaks cut runs, they clear no bin)
        assert np.array_equal(seen["mask"], (np.asarray(kw["parentSolution"]) > 0).astype(np.uint8))
        flagged = (seen["rec"]["flags"] & B.NONFINITE) != 0
        assert int(flagged.sum()) == int(name in BC.HOST_DECIDED)


# ---------------------------------------------------------------------------------------------------------------
# the support-run routines on the CPU, through the host half of the resident form
# ---------------------------------------------------------------------------------------------------------------
class _Batch:
    """What `broad.batch_parents` reads of a DeviceBatch"""
    def __init__(self, lens):
        self.chain_lens, self._ctx, self._broad_parents, self.broad_stats = list(lens), None, {}, None

    def _chain_mask(self, chains):
        take = [True] * len(self.chain_lens) if chains is None else [bool(t) for t in chains]
        return take, (None if chains is None else bytes(bytearray(int(t) for t in take)))


def cpu_run_records(exe, tmp, cases):
    """what stands in for consenrich_amd.broad._device_run_records: csr_batch_broad_runs and its fetch, chain after chain, from the
    stand-alone program"""
    def run(batch, cfg, mask, n_breaks, flat):
        counts, recs = np.zeros(cfg.size, B.RUN_COUNTS), []
        first = np.concatenate(([0], np.cumsum(n_breaks)))
        for c, case in enumerate(cases):
            if mask is not None and not mask[c]:
                continue
            kw, g = case["kw"], cfg[c]
            (support, kept, fallback), rec = _run(exe, tmp, kw["scores"], None, None, float(g["selection_penalty"]), float(g["dip_fraction"]),
                                                  0.0, [], [], runs=(float(g["threshold"]), flat[first[c]:first[c + 1]], kw["strong"],
                                                                     kw["weak"], int(g["max_gap_bins"])))
            rec["chain"] = c
            counts[c] = (support, kept, fallback, 0)
            recs.append(rec)
        return counts, np.concatenate(recs) if recs else np.zeros(0, B.RUN)
    return run


PARENTS = BC.parents_cases()


def _parents_of(cases, take=None):
    kws = [c["kw"] for c in cases]
    batch = _Batch([kw["scores"].size for kw in kws])
    blacklist = {}
    for kw in kws:
        blacklist.update(kw["blacklist"] or {})
    # (dip fraction and run penalty are one value per call)
    out = B.batch_parents(batch, [kw["threshold"] for kw in kws], [kw["selection_penalty"] for kw in kws],
                          [kw["boundary_cost"] for kw in kws], max_gap_bp=[kw["max_gap_bp"] for kw in kws],
                          intervals=[kw["intervals"] for kw in kws], ends=[kw["ends"] for kw in kws],
                          chroms=[kw["chromosome"] for kw in kws], blacklist=blacklist, dip_penalty_fraction=kws[0]["dip_penalty_fraction"],
                          run_penalty=kws[0]["run_penalty"], chains=take)
    return batch, out


def _same_parents(got, name):
    flat = {"starts": got["starts"].tolist(), "ends": got["ends"].tolist(), "merge_details": got["merge_details"],
            "weak_support_run_count": got["weak_support_run_count"],
            "weak_support_touching_run_count": got["weak_support_touching_run_count"], "envelope_fallback": got["envelope_fallback"]}
    return BC.differences(BC.canon(flat), golden("broad_parents.npz", name))


def test_support_runs_on_the_cpu_match_the_reference(host_check, monkeypatch):
    """The six chains of the resident test in one `batch_parents` call (one masked out), and the two with their own dip fraction and
    run penalty alone: flags, scans, touch, compaction and gap sums from the stand-alone program, the records through the host half"""
    monkeypatch.setattr(B, "_device_run_records", cpu_run_records(*host_check, PARENTS[:6]))
    take = [True, False, True, True, True, True]
    batch, out = _parents_of(PARENTS[:6], take)
    assert out[1] is None and sorted(batch._broad_parents) == [0, 2, 3, 4, 5]
    for c in (0, 2, 3, 4, 5):
        assert _same_parents(out[c], PARENTS[c]["name"]) == [], c
        assert (batch._broad_parents[c][0].tolist(), batch._broad_parents[c][1].tolist()) == (out[c]["starts"].tolist(), out[c]["ends"].tolist())
    assert len(out[2]["merge_details"]) == 10 and out[2]["envelope_fallback"] and out[4]["envelope_fallback"]
    assert batch.broad_stats["chains"] == 5
    for case in PARENTS[6:]:
        monkeypatch.setattr(B, "_device_run_records", cpu_run_records(*host_check, [case]))
        _, out = _parents_of([case])
        assert _same_parents(out[0], case["name"]) == [], case["name"]


def test_gaps_beyond_the_bound_are_not_summed(host_check):
    """The bound the host passes is the most bins a gap within maxGapBP can hold: with it the long gaps come back as 0.0, without it
    they are summed, and the gaps the distance test lets through have the same sum either way"""
    kw = PARENTS[0]["kw"]
    exe, tmp = host_check
    bound = B.max_gap_bins(kw["intervals"], kw["ends"], kw["max_gap_bp"])
    assert bound == kw["max_gap_bp"] // 25
    recs = [_run(exe, tmp, kw["scores"], None, None, 0.2, 0.5, 0.0, [], [], runs=(kw["threshold"], np.zeros(0, np.int64), kw["strong"],
                                                                                  kw["weak"], b))[1] for b in (bound, -1)]
    lens = recs[0]["start"][1:] - recs[0]["end"][:-1] - 1
    assert (lens > bound).any() and (lens <= bound).any()
    assert all(bits(r["gap_sum"][:-1][lens <= bound]) == bits(recs[1]["gap_sum"][:-1][lens <= bound]) for r in recs)
    assert bits(recs[0]["gap_sum"][:-1][lens > bound]) == bits(np.zeros(int((lens > bound).sum())))
    assert (recs[1]["gap_sum"][:-1][lens > bound] != 0.0).all()
    iv = kw["intervals"].copy()
    iv[5] -= 30         # overlapping bins: no bound
    assert B.max_gap_bins(iv, kw["ends"], 2000) == -1 and B.max_gap_bins(kw["intervals"], kw["intervals"], 2000) == -1
