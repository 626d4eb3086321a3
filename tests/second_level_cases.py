"""Case table of the second-level tests: the post-fit scans, compactions and sums at the first sizes at which a loop takes a second
round or a launch a second grid block.  Every size below is derived from the constant that decides it, named after the kernel line
that holds it: when a block size changes, the assertions of tests/test_second_level_refs.py show which case no longer does its
job.  Inputs are synthesised from seeds; nothing here is read from a file.

  A  run bounds of a resident mask          k_rocco_run_count / _scan / _write, DeviceBatch.rocco_runs
  B  support runs of broad mode             k_broad_run_count .. k_broad_run_gaps
  C  the text and bigWig writers            k_bgw_len / _scan_blocks / _scan_rows / _write
  D  NumPy-order sums, the null             k_np_chunk_sums, k_null_merge
  E  what the audit of DESIGN.md 9b added   k_dwb_tail, the per-track lanes of the null, k_peak_view_pick, k_export_*,
                                            the later rounds of the ESS lags"""
import numpy as np

from broad_cases import SUPPORT_THRESHOLD
from narrowpeak_cases import coords, runs_mask

SCAN_BLOCK = 1024       # bins (rows, runs) per workgroup of a flag or length pass: k_rocco_run_count (csrc/csr_rocco.h:306),
#                         k_broad_run_count / k_broad_keep_count (csrc/csr_broad.h:205, 250), k_bgw_len (csrc/csr_writers.h:132)
SCAN_ROUND = 1024       # block sums one round of the single-workgroup scans takes: k_rocco_run_scan (csrc/csr_rocco.h:318),
#                         k_broad_scan (csrc/csr_broad.h:218), k_bgw_scan_blocks (csrc/csr_writers.h:157)
ROUND = SCAN_BLOCK * SCAN_ROUND     # bins, rows or runs in one full round: one more takes the carry into a second round
RUNS_CAP = 1 << 16      # the capacity of DeviceBatch.rocco_runs' first call (consenrich_amd/batch.py:627)
GAP_WAVE = 64           # kept runs per workgroup of k_broad_run_gaps (csrc/csr_broad.h:273)
NP_CHUNK = 8192         # values per pairwise-tree chunk (csrc/csr_np_order.h:20)
CHUNKS_PER_BLOCK = 64   # chunks per workgroup of k_np_chunk_sums (csrc/csr_np_order.h:203)
SUM_BLOCK = NP_CHUNK * CHUNKS_PER_BLOCK     # values one grid block of k_np_chunk_sums sums
NULL_TILE = 2048        # keys per sorted tile in front of k_null_merge (csrc/csr_null.h:31)
SECTION_ITEMS = 1024    # items per bigWig data section (csrc/csr_writers.h k_bw_sections; tests/writer_refs.py)
TAIL_PAIRS = 64         # (chunk, z) pairs per workgroup of k_dwb_tail (csrc/csr_dwb.h:271)
TRACK_LANES = 64        # tracks, jobs or queries per workgroup of k_null_scan, k_np_fold, k_null_gather, k_null_search and
#                         k_null_abs_rank (csrc/csr_null.h:227, 276, 287, 312; csrc/csr_np_order.h:212)


# ---------------------------------------------------------------------------------------------------------------
# A. run bounds
# ---------------------------------------------------------------------------------------------------------------
RUN_LENGTHS = (ROUND,                       # exactly one full round
               ROUND + 1,                   # a second round of one block
               ROUND + SCAN_BLOCK + 1,      # a second round of two blocks
               2 * ROUND + 1)               # a third round
RUN_GAPS = (0, 1, 3)
LOOK_BEHIND = dict(n=5003, max_gap_bins=1500)       # the look-behind of a start reaches past a whole block


def run_bounds_numpy(mask, max_gap_bins=0):
    """`cBooleanRunBounds` derived from the set bins alone: a run breaks where two consecutive set bins lie more than gap + 1
    apart.  Shares no step with tests/twin_rocco.py's walk over the bins or with the kernels' flags and scans."""
    idx = np.flatnonzero(np.asarray(mask).ravel() != 0).astype(np.int64)
    if idx.size == 0:
        return idx, idx.copy()
    cut = np.diff(idx) > max(int(max_gap_bins), 0) + 1
    return idx[np.concatenate(([True], cut))], idx[np.concatenate((cut, [True]))]


def run_mask(kind, n, seed=0):
    """every_second: bins 0, 2, 4, ..; across: a run over bins ROUND - 1 | ROUND; beside: a run that ends at ROUND - 1 next to one
    that starts at ROUND + 1; both sparse kinds hold bin 0, the last bin, the same edges at the second round's end and a sprinkle of
    seeded runs so that the indices in front of the edge are not trivial"""
    m = np.zeros(n, np.uint8)
    if kind == "zeros":
        return m
    if kind == "ones":
        return m + 1
    if kind == "every_second":
        m[::2] = 1
        return m
    if kind == "random":
        return (np.random.default_rng(seed + n).random(n) < 0.3).astype(np.uint8)
    rng = np.random.default_rng(seed + n)
    for a in np.sort(rng.choice(n - 8, size=max(n // 997, 3), replace=False)).tolist():
        m[a:a + 1 + a % 5] = 1
    for edge in (ROUND, 2 * ROUND):
        lo, hi = max(edge - 12, 0), min(edge + 12, n)
        m[lo:hi] = 0
        runs = {"across": [(edge - 3, edge + 2)], "beside": [(edge - 4, edge - 1), (edge + 1, edge + 2)]}[kind]
        for a, b in runs:
            m[max(a, 0):max(min(b + 1, n), 0)] = 1
    m[0] = m[n - 1] = 1
    return m


def look_behind_mask():
    """single set bins a few hundred to a few thousand bins apart: some gaps below max_gap_bins + 1, some above it, one equal"""
    n, gap = LOOK_BEHIND["n"], LOOK_BEHIND["max_gap_bins"]
    m = np.zeros(n, np.uint8)
    m[[0, 700, 700 + gap + 1, 700 + 2 * (gap + 1) + 1, n - 3, n - 1]] = 1      # == gap + 1: bridged; gap + 2: not
    return m


def run_cases():
    """(name, n, mask kind, gaps)"""
    out = []
    for n in RUN_LENGTHS:
        out += [(f"every_second_{n}", n, "every_second", (0, 1)), (f"across_{n}", n, "across", RUN_GAPS),
                (f"beside_{n}", n, "beside", RUN_GAPS)]
    out += [(f"zeros_{ROUND + 1}", ROUND + 1, "zeros", (0, 3)), (f"ones_{ROUND + 1}", ROUND + 1, "ones", (0, 3))]
    return out


DIRECT_LENGTHS = (2 * SCAN_BLOCK + 5, ROUND + 1)      # a three-block mask and the first with a second round


# ---------------------------------------------------------------------------------------------------------------
# B. support runs of broad mode
# ---------------------------------------------------------------------------------------------------------------
HIGH, LOW = 0.8, -0.9       # about the threshold 0.5: no score within 0.02 of it (asserted in regular_chain)


def regular_chain(name, n_runs, kept, seed, period=5, run=2, lead=3, tail=4, breaks=(), envelope_only=False, loose=(), **kw):
    """Beside broad_cases.support_chain: `n_runs` support runs of `run` bins every `period` bins, the rest well below the threshold.
    kept: the indices of the runs that touch the envelope (a weak bin on the first bin of every second one, a strong bin on the
    last bin of the others).  loose: weak bins outside every run (they touch nothing).  envelope_only: no score reaches the
    threshold, the runs are runs of weak | strong (the fallback)."""
    n = lead + n_runs * period - (period - run) + tail
    rng = np.random.default_rng(seed)
    s = LOW + 0.1 * rng.uniform(-1.0, 1.0, n)
    first = lead + period * np.arange(n_runs)
    weak, strong = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    if envelope_only:
        for k, a in enumerate(first.tolist()):
            (weak, strong)[k % 2][a:a + run] = 1
            if k % 3 == 0:
                (strong, weak)[k % 2][a + run - 1] = 1          # both masks on one bin
    else:
        for a in first.tolist():
            s[a:a + run] = HIGH + 0.1 * rng.uniform(-1.0, 1.0, run)
        for j, k in enumerate(sorted(kept)):
            if j % 2 == 0:
                weak[first[k]] = 1
            else:
                strong[first[k] + run - 1] = 1
        for i in loose:
            assert s[i] < SUPPORT_THRESHOLD
            weak[i] = 1
    assert np.all(np.abs(s - SUPPORT_THRESHOLD) >= 0.02)
    iv, en = coords(n, 25, breaks)
    out = dict(scores=s, strong=strong, weak=weak, threshold=SUPPORT_THRESHOLD, intervals=iv, ends=en, chromosome=name,
               selection_penalty=0.2, boundary_cost=1.0, max_gap_bp=2000, blacklist=None, dip_penalty_fraction=0.5, run_penalty=0.0)
    out.update(kw)
    return dict(name=name, kw=out, first=first, run=run)


def _kept_indices(n_runs, count, seed, forced=()):
    """`count` run indices, the forced ones among them, never their direct neighbours (a dropped run on both sides of each)"""
    rng = np.random.default_rng(seed)
    banned = {f + d for f in forced for d in (-1, 1)} - set(forced)
    pool = [k for k in range(n_runs) if k not in banned and k not in forced]
    pick = rng.choice(len(pool), size=count - len(forced), replace=False)
    return sorted(set(forced) | {pool[i] for i in pick.tolist()})


def _long_chain(name="long", edges=(ROUND,), seed=77):
    """edges[-1] + SCAN_BLOCK + 1 bins: a round of two blocks behind the last edge in k_broad_scan over the bins' block sums (one
    edge: a second round; two: a third, whose carry holds two rounds' totals).  At every edge a support run lies across the edge bin
    and touches nothing; the kept runs on its two sides are 66 bins apart, so the gap between them spans the round edge and is
    summed (at most 80 bins fit into max_gap_bp); every other gap between kept runs is far longer than that and is left unsummed."""
    n = edges[-1] + SCAN_BLOCK + 1
    rng = np.random.default_rng(seed)
    s = LOW + 0.1 * rng.uniform(-1.0, 1.0, n)
    support, weak, strong = [(0, 4)], [(2, 2), (n - 1, n - 1)], [(n - 2, n - 1)]
    for E in edges:
        support += [(E - 40, E - 36), (E - 3, E + 2), (E + 31, E + 35)]
        weak.append((E - 38, E - 38))
        strong.append((E + 33, E + 34))
    support.append((n - 3, n - 1))                       # (over a block edge)
    regular = [a for a in range(5000, edges[-1] - 5000, 997) if all(abs(a - E) > 1000 for E in edges)]
    support += [(a, a + 2) for a in regular]            # more than 1024 runs in front of every edge
    weak += [(a + 1, a + 1) for a in regular[::9]]
    for a, b in support:
        s[a:b + 1] = HIGH + 0.1 * rng.uniform(-1.0, 1.0, b - a + 1)
    assert np.all(np.abs(s - SUPPORT_THRESHOLD) >= 0.02)
    iv, en = coords(n, 25)
    kw = dict(scores=s, strong=runs_mask(n, strong), weak=runs_mask(n, weak), threshold=SUPPORT_THRESHOLD, intervals=iv, ends=en,
              chromosome=name, selection_penalty=0.2, boundary_cost=30.0, max_gap_bp=2000, blacklist=None, dip_penalty_fraction=0.5,
              run_penalty=0.0)
    return dict(name=name, kw=kw)


def _breaks_chain():
    """1100 support runs of 4 bins every 7; a coordinate break in the middle of each of the first 1024, one on the left edge of the
    first run (the first of the list) and one on the right edge of run 1024 (the last): 1026 breaks, 2124 runs"""
    period, run, lead = 7, 4, 3
    first = lead + period * np.arange(1100)
    breaks = [lead - 1] + [int(a) + 1 for a in first[:SCAN_BLOCK]] + [int(first[SCAN_BLOCK]) + run - 1]
    kept = _kept_indices(1100, 90, 5, forced=(0, SCAN_BLOCK - 1, SCAN_BLOCK))
    return regular_chain("breaks", 1100, kept, 15, period=period, run=run, lead=lead, breaks=tuple(breaks), max_gap_bp=400)


def broad_chains():
    """The chains of the resident batch, in its order"""
    K = SCAN_BLOCK
    return [
        regular_chain("runs_1023", K - 1, _kept_indices(K - 1, GAP_WAVE - 1, 1, forced=(0, K - 2)), 11, loose=(1, 5 * 40 + 1), boundary_cost=5.0),
        regular_chain("runs_1024", K, _kept_indices(K, GAP_WAVE, 2, forced=(K - 1,)), 12, boundary_cost=5.0),
        # a kept run that is the last of workgroup 0 and one that is the first of workgroup 1; the 65th kept run is the only one of the
        # second workgroup of k_broad_run_gaps
        regular_chain("runs_1025", K + 1, _kept_indices(K + 1, GAP_WAVE + 1, 3, forced=(K - 1, K)), 13, boundary_cost=5.0, max_gap_bp=700),
        # every second run kept, with 1023 in place of 1022: 1025 kept runs out of three workgroups of the compaction, runs 1023 and 1024
        # both kept with a dropped run on their other side; gaps of 3 and 8 bins whose gains lie about zero
        regular_chain("runs_2049", 2 * K + 1, sorted((set(range(0, 2 * K + 1, 2)) - {K - 2}) | {K - 1}), 14, boundary_cost=1.05),
        regular_chain("envelope_1500", 1500, (), 16, envelope_only=True, boundary_cost=0.825, max_gap_bp=75),
        _breaks_chain(),
        _long_chain(),
        _long_chain("long3", edges=(ROUND, 2 * ROUND), seed=78),      # beyond the issue's table: a third round of k_broad_scan
    ]


NEEDED_SECOND_LEVEL = ("support_runs_over_block", "kept_runs_over_wave", "kept_runs_over_block", "bins_over_carry_round",
                       "breaks_over_block", "envelope_fallback", "piece_touching", "piece_not_touching")


def kept_runs_numpy(scores, weak, strong, threshold, intervals, ends, envelope=False):
    """The support runs and the touching ones of tests/twin_broad.py `_device_kept_runs` on whole vectors (the twin walks bin by
    bin): (support runs, kept runs) as lists of (first, last).  tests/test_second_level_refs.py holds the two equal."""
    s = np.asarray(scores, np.float64)
    iv, en = np.asarray(intervals, np.int64), np.asarray(ends, np.int64)
    env = (np.asarray(weak) > 0) | (np.asarray(strong) > 0)
    pred = env if envelope else s >= float(threshold)
    cut = en[:-1] != iv[1:]
    starts = np.flatnonzero(pred & np.concatenate(([True], ~pred[:-1] | cut)))
    last = np.flatnonzero(pred & np.concatenate((~pred[1:] | cut, [True])))
    inside = np.concatenate(([0], np.cumsum(env)))
    touch = np.ones(starts.size, bool) if envelope else inside[last + 1] - inside[starts] > 0
    runs = list(zip(starts.tolist(), last.tolist()))
    return runs, [r for r, t in zip(runs, touch.tolist()) if t]


def kept_records(kw):
    """What csr_batch_broad_runs hands out for one chain: (support run count, fallback, [(start, end, gap sum)]).  The gap sum is
    NumPy's own np.sum of the dip-weighted excess, 0.0 behind the last run, for a gap without a bin and for one of more bins than
    max_gap_bp can hold (consenrich_amd/broad.py max_gap_bins)."""
    args = (kw["scores"], kw["weak"], kw["strong"], kw["threshold"], kw["intervals"], kw["ends"])
    support, kept = kept_runs_numpy(*args)
    fallback = not kept
    if fallback:
        _, kept = kept_runs_numpy(*args, envelope=True)
    s = np.asarray(kw["scores"], np.float64)
    narrowest = int(np.min(kw["ends"] - kw["intervals"]))
    bound = int(max(int(kw["max_gap_bp"]), 0)) // narrowest
    f, pen = float(np.clip(kw["dip_penalty_fraction"], 0.0, 1.0)), float(max(kw["selection_penalty"], 0.0))
    out = []
    for k, (a, b) in enumerate(kept):
        total = 0.0
        if k + 1 < len(kept):
            nxt = kept[k + 1][0]
            if 0 < nxt - b - 1 <= bound:
                ex = np.asarray(s[b + 1:nxt] - pen, dtype=np.float64)
                total = float(np.sum(np.where(ex < 0.0, f * ex, ex)))
        out.append((a, b, total))
    return len(support), fallback, out


# ---------------------------------------------------------------------------------------------------------------
# C. writers
# ---------------------------------------------------------------------------------------------------------------
WRITER_ROWS = ROUND + SCAN_BLOCK + 1        # a second round of two blocks in k_bgw_scan_blocks; 1026 bigWig sections
WRITER_START0, WRITER_STEP = 999_990, 3000  # starts pass from 6 to 7, 8, 9 and 10 digits along the track; the last end < 2^32


WRITER_ROWS_3 = 2 * ROUND + 1               # a third round of k_bgw_scan_blocks (text only: the ends pass 2^32, which bigWig cannot hold)


def writer_values(finite_only, rows=WRITER_ROWS):
    """The edge table of the text writer (tests/test_oracle_writers.edge_values) cycled through WRITER_ROWS rows.  Its length
    is no multiple of the 1024 rows of a block, so every block holds another stretch of it; the literal head of the table (the longest and the
    shortest texts) starts three rows behind the round edge, the tail of the table ends in front of it."""
    from test_oracle_writers import edge_values

    v = edge_values()
    if finite_only:
        v = v[np.isfinite(v)]
    return v[(np.arange(rows) - (ROUND + 3)) % len(v)].astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------
# D. NumPy-order sums and the null
# ---------------------------------------------------------------------------------------------------------------
SUM_SIZES = (SUM_BLOCK + 1, 2 * SUM_BLOCK + 1)      # one chunk into the second grid block; one chunk into the third
NULL_CHAINS = (SUM_BLOCK + 1, 70, NP_CHUNK + 1, 2 * SUM_BLOCK + 1)     # short jobs in a grid sized for the long one
SELECT_CHAINS = (700_001, 9000)


def selected_runs():
    """Runs of chain 0 (1 to 300 bins, 1 to 80 bins apart) that select SUM_BLOCK + 1 bins: one run ends on gathered position
    SUM_BLOCK - 1, the next (one bin) starts on SUM_BLOCK; three runs of chain 1.  Returns (n_runs per chain, starts, ends)."""
    rng = np.random.default_rng(2024)
    starts, ends, pos, got = [], [], 7, 0
    while got < SUM_BLOCK:
        k = min(int(rng.integers(1, 301)), SUM_BLOCK - got)
        starts.append(pos)
        ends.append(pos + k - 1)
        got += k
        pos += k + int(rng.integers(1, 81))
    starts.append(pos)
    ends.append(pos)
    assert pos < SELECT_CHAINS[0]
    n0 = len(starts)
    other = [(0, 10), (4000, 4000), (8100, 8999)]
    starts += [a for a, _ in other]
    ends += [b for _, b in other]
    return np.asarray([n0, len(other)], np.int64), np.asarray(starts, np.int64), np.asarray(ends, np.int64)


def select_scores():
    rng = np.random.default_rng(99)
    return [rng.standard_normal(n) * np.exp(rng.uniform(-3.0, 3.0, n)) for n in SELECT_CHAINS]


# ---------------------------------------------------------------------------------------------------------------
# E. further thresholds the audit found ("Second levels of the post-fit kernels")
# ---------------------------------------------------------------------------------------------------------------
TAIL_Z_GRID = (0.0, 1.5, 2.0, 2.5, 3.0)
TAIL_BINS = (TAIL_PAIRS // len(TAIL_Z_GRID)) * NP_CHUNK + 1      # 13 chunks of 5 z: the 65th pair is alone in a second workgroup
MANY_TRACKS = tuple(16 + 7 * k for k in range(TRACK_LANES + 2))  # 66 short tracks in one call: a second workgroup of per-track lanes


SEGMENT_LANES = 64      # segments per workgroup of k_peak_view_pick (csrc/csr_peakscore.h:141)


def many_segments(n):
    """SEGMENT_LANES + 1 segments of a track of n bins, 1 to 130 bins long: the 65th is alone in a second workgroup"""
    rng = np.random.default_rng(8)
    st = np.sort(rng.choice(n - 200, size=SEGMENT_LANES + 1, replace=False)).astype(np.int64)
    return st, st + rng.integers(0, 130, st.size)


EXPORT_LANES = 64       # parents per workgroup of k_export_prep / k_export_finish and children per workgroup of k_export_child
#                         (csrc/csr_export.h:252, 256, 260; the grids of csrc/csr_host_export.inl:120, 131, 149)
EXPORT_PENALTY, EXPORT_GAMMA = 0.3, 1.0     # the sub-peak selection penalty and the chain's gamma (boundary cost 0.25 gamma)


def many_parents():
    """EXPORT_LANES + 2 parents in the manner of narrowpeak_cases._splits, in turn: three bumps (three children), one bump with poor
    tails (one child shorter than its parent), a parent kept whole -- so the children exceed a workgroup as well.  Returns the keyword
    arguments of narrowpeak_cases.base (the state is a stand-in: the GPU test reads the signal of its own fit)."""
    from narrowpeak_cases import base, layout, wave

    bump, valley = [2.0, 2.5, 3.0, 2.5, 2.0, 1.5, 2.0, 2.2], [-3.0] * 6
    kinds = (bump + valley + bump + valley + bump, [-2.0] * 4 + bump + [-2.0] * 5, [1.5, 1.75, 2.0, 2.5, 2.25, 2.0, 1.5, 1.25, 1.5])
    parts = [kinds[k % 3] for k in range(EXPORT_LANES + 2)]
    n, runs = layout([len(v) for v in parts], lead=1, tail=1)
    s = np.full(n, -1.0)
    for k, ((a, b), v) in enumerate(zip(runs, parts)):
        s[a:b + 1] = np.asarray(v) + 0.001 * (k % 7)          # (no two parents alike)
    return base("many_parents", n, runs, s, s + 0.25 * wave(n, 9, 1.1), step=50, subpeakSelectionPenalty=EXPORT_PENALTY,
                subpeakBoundaryCost=0.25 * EXPORT_GAMMA)["kw"]


ESS_ROUNDS = (256, 512, 1024, 2048, 4096)      # lags per round of the effective-sample-size scan: ESS_ROUND_FIRST doubling up to ESS_ROUND_MAX,
#                                                 then rounds of ESS_ROUND_MAX (csrc/csr_host_ess.inl:10, 98-184)
ESS_RAMPS = (3501, 24001)       # a ramp's autocorrelation stays positive for about 0.366 n lags: a scan alive into the third round,
#                                 and one alive past the last doubling (a sixth round, of the capped size)


def ess_ramp(n):
    return np.arange(n, dtype=np.float64) * 0.25


def tail_inputs():
    """(scores, template) of the DWB panel at TAIL_BINS, in the manner of tests/test_gpu_dwb.py"""
    rng = np.random.default_rng(505)
    return rng.normal(0.25, 1.3, TAIL_BINS), rng.normal(0.0, 1.0, TAIL_BINS) * (1.0 + 0.5 * np.sin(np.arange(TAIL_BINS) / 50.0))
