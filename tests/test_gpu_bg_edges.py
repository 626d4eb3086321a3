"""GPU tests of the background solve (csr_background.h: two-level partition of the pentadiagonal system) at every edge of its
partition, against a TRUTH solve (run with -m gpu).  Cases: tests/golden/bg_edge_cases.py; truth and condition number:
oracle/bg_truth.py (long-double LDL' of the system assembled from its definition, pinned to a 256-bit solve by
tests/test_bg_truth.py, which also asserts which partition classes the table holds).

(a) every case as one chain of one call, at its blockLen:  max|x - truth| / scale <= 4 * 2^-52 * cond2(A),
    scale = max(max|truth_plain|, max|truth_zc|) -- the centred solution can be far smaller than the uncentred one it is a
    difference of.  The oracle (the reference's sequential LDL') is held to the same gate in the same test.  Where the 4 comes
    from: both eliminations are Cholesky in some order, backward stable with an error of a small multiple of 2^-52 cond2; the
    worst the reference shows over the table is 0.53, 4 is 8 x that (and 2 x the device's distance measured at chromosome size,
    about 4 x the reference's).  Not derived from what the device returns here.
(b) all cases of one (Bp, penalty pair) as the chains of ONE call, in a fixed shuffled order: bit for bit what (a) returned.
(c) the pivot contract: a zero weight without penalties is reported at its chain-local index, with the oracle's message.
(d) the resident update (`DeviceBatch.background_update`, IRLS lock-step through the `active` mask) with block_len 8 and 64 on
    chains of 1 .. 4100 bins that stop after 0, 1 and >= 2 passes: against the oracle as test_batch_background_update_matches_oracle
    does it, and bit for bit against every chain alone in a batch of its own."""
import re

import numpy as np
import pytest

import bg_edge_cases as E
from conftest import gpu_available
from oracle import bg_truth as T

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
GATE = 4.0
CASES = E.edge_cases()
GROUPS = sorted({(c["bp"], c["span"]) for c in CASES}, key=lambda g: (g[0] == 0, g))
WORST = {"device": {}, "oracle": {}}      # (Bp, span, kind, zero-centre) -> worst err / (scale 2^-52 cond2); printed at the end (-s)
_TRUTH, _ALONE = {}, {}
PIVOT_MESSAGE = re.compile(r"pivot modification at index (\d+) \(pivot=([^,]+), floor=1e-12\)")


@pytest.fixture(scope="module")
def product():
    if not gpu_available():
        pytest.fail("GPU tests selected but no HIP device / library: the product has no CPU fallback")
    from consenrich_amd import cconsenrich

    yield cconsenrich
    for who in ("oracle", "device"):
        print(f"\nworst |{who} - truth| / (scale 2^-52 cond2) per (Bp, span, kind, zero-centre):")
        for key in sorted(WORST[who]):
            print("  ", key, f"{WORST[who][key]:.4f}")


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as orc

    orc.lib()
    return orc


def _group(bp, span):
    return [c for c in CASES if c["bp"] == bp and c["span"] == span]


def _truth(case):
    """(w, r, lam_first, lam, cond2, (truth_plain, truth_zc), scale), once per module"""
    if case["name"] not in _TRUTH:
        w, r = E.edge_inputs(case)
        lam_first, lam = E.edge_lams(case)
        pair = T.solve_truth_pair(w, r, lam_first, lam)
        scale = float(max(np.abs(pair[0]).max(), np.abs(pair[1]).max()))
        _TRUTH[case["name"]] = (w, r, lam_first, lam, T.cond2(w, lam_first, lam), pair, scale)
    return _TRUTH[case["name"]]


def _alone(product, case, zc):
    """the case as the only chain of one call at its blockLen, once per module"""
    key = (case["name"], zc)
    if key not in _ALONE:
        w, r = E.edge_inputs(case)
        lam_first, lam = E.edge_lams(case)
        _ALONE[key] = product.solveBackgroundBatch([w], [r], lam, zc, lam_first, blockLen=case["bp"])[0]
    return _ALONE[key]


def _outcome(fn):
    try:
        return np.asarray(fn()), None
    except RuntimeError as e:
        return None, str(e)


def partition(n, bp):
    """`bg_partition` (csr_host_rows.inl): (number of blocks K, length of the last block)"""
    k = -(-n // bp)
    k -= 1 if k > 1 and n - (k - 1) * bp < 4 else 0
    return k, n - (k - 1) * bp


# ---- (a) -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bp,span", GROUPS)
def test_each_case_alone_is_within_the_gate_of_the_truth(product, oracle, bp, span):
    failed = []
    for case in _group(bp, span):
        if case["singular"]:
            # no positive weight: the expected output is the reference's report of the last pivot (or its 0 for a centred single
            # bin).  The pivot itself is 0 in the reference and a rounding of 0 here (one division per step, csr_background.h).
            w, r = E.edge_inputs(case)
            lam_first, lam = E.edge_lams(case)
            for zc in (False, True):
                want = _outcome(lambda: oracle.csolveZeroCenteredBackground(w, r, lam, zc, lamFirst=lam_first))
                got = _outcome(lambda: product.solveBackgroundBatch([w], [r], lam, zc, lam_first, blockLen=bp)[0])
                if want[1] is None:
                    assert case["n"] == 1 and zc and got[1] is None and np.array_equal(got[0], want[0]), (case["name"], got, want)
                    continue
                m_want, m_got = (PIVOT_MESSAGE.search(s or "") for s in (want[1], got[1]))
                assert m_want and m_got, (case["name"], zc, got, want)
                assert int(m_got.group(1)) == int(m_want.group(1)) == case["n"] - 1 and float(m_want.group(2)) == 0.0
                assert abs(float(m_got.group(2))) <= 1.0e-12, (case["name"], zc, got[1])
            continue
        w, r, lam_first, lam, cond, pair, scale = _truth(case)
        for zc in (False, True):
            got = _alone(product, case, zc)
            ref = oracle.csolveZeroCenteredBackground(w, r, lam, zc, lamFirst=lam_first)
            assert got.dtype == np.float64 and got.shape == pair[zc].shape
            key = (bp, span, case["kind"], zc)
            for who, x in (("oracle", ref), ("device", got)):
                ratio = float(np.abs(x - pair[zc]).max()) / scale / (EPS * cond)
                WORST[who][key] = max(WORST[who].get(key, 0.0), ratio)
                if not ratio <= GATE:
                    failed.append((who, case["name"], zc, ratio))
            # the centred solution sums to zero: n entries, each within the gate of a truth that sums to n roundings of scale
            if zc and not abs(float(got.sum())) <= (GATE * EPS * cond + EPS) * scale * case["n"]:
                failed.append(("device sum", case["name"], zc, float(got.sum()) / scale))
    assert not failed, failed


# ---- (b) -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bp,span", GROUPS)
def test_cases_as_chains_of_one_call_are_bit_identical(product, bp, span):
    group = [c for c in _group(bp, span) if not c["singular"]]
    order = np.random.default_rng(1000 * bp + span).permutation(len(group))
    group = [group[i] for i in order]
    ws, rs = zip(*(E.edge_inputs(c) for c in group))
    lam_first, lam = E.edge_lams(group[0])
    # where the call has more than one 64-block group of k_bg_local, the groups cut through chains whose last blocks differ
    first, cut_lasts = 0, set()
    for c in group:
        k, last = partition(c["n"], E.block_len(bp))
        if first // 64 != (first + k - 1) // 64:
            cut_lasts.add(last)
        first += k
    assert first <= 64 or len(cut_lasts) >= 3, (first, cut_lasts)
    for zc in (False, True):
        got = product.solveBackgroundBatch(ws, rs, lam, zc, lam_first, blockLen=bp)
        diff = [c["name"] for c, g in zip(group, got) if not np.array_equal(g, _alone(product, c, zc))]
        assert not diff, (zc, diff)


# ---- (c) -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bp", [8, 64])
def test_zero_pivot_is_reported_at_its_chain_local_index(product, oracle, bp):
    n = 80 * bp + 1                                    # 80 blocks, the last one Bp + 1 bins long
    assert partition(n, bp) == (80, bp + 1)
    interior, sep0, sep1, last, late = 3 * bp + 2, 6 * bp - 2, 6 * bp - 1, n - 1, 70 * bp + 1
    # `late`: block 70, found in the second round of the 64-lane ballot of k_bg_reduced
    singles = [(n, interior), (n, sep0), (n, sep1), (n, last), (n, 79 * bp), (n, late), (n, 0), (2 * bp + 3, 2 * bp + 2),
               (bp + 3, bp + 2)]
    pairs = [(n, sep0, 6 * bp + 1), (n, sep1, 6 * bp), (n, interior, sep0), (n, late, last), (n, sep0, sep1), (n, 1, late),
             (n, 64 * bp - 1, 64 * bp), (n, 63 * bp + 1, late)]
    rng = np.random.default_rng(bp)
    for length, *zeros in singles + pairs:
        w = 1.0 + rng.random(length)
        w[list(zeros)] = 0.0
        r = rng.normal(0.0, 1.0, length)
        for zc in (False, True):
            with pytest.raises(RuntimeError) as want:
                oracle.csolveZeroCenteredBackground(w, r, 0.0, zc, lamFirst=0.0)
            assert f"at index {min(zeros)} (pivot=0, floor=1e-12)" in str(want.value)
            with pytest.raises(RuntimeError) as got:
                product.solveBackgroundBatch([w], [r], 0.0, zc, 0.0, blockLen=bp)
            assert str(got.value) == str(want.value), (length, zeros, zc)
    # the chain-local index, not the batch's: the same chain behind two healthy ones
    w = np.ones(n)
    w[late] = 0.0
    with pytest.raises(RuntimeError, match=rf"at index {late} \(pivot=0, floor=1e-12\)"):
        product.solveBackgroundBatch([np.ones(77), np.ones(5 * bp), w], [np.ones(77), np.ones(5 * bp), np.ones(n)], 0.0, False, 0.0,
                                     blockLen=bp)


# ---- (d) -----------------------------------------------------------------------------------------------------------------
def _fit_and_update(lens, ins, block_len, kw, lam_first, lam):
    from consenrich_amd import _lib as L
    from consenrich_amd.batch import DeviceBatch, ModelParams

    with DeviceBatch(0) as b:
        b.configure(ModelParams(state_dim=2), E.RESIDENT_M, lens)
        for c, (data, munc) in enumerate(ins):
            b.upload(c, data, munc)
        b.stats()
        b.forward_backward(L.RETURN_NLL)
        b.export(L.EXPORT_SMOOTH)
        xs = [b.download(c, "xs") for c in range(len(lens))]
        info = b.background_update(lam_first, lam, block_len=block_len, **kw)
        nxt = [b.download(c, "background_next") for c in range(len(lens))]
    return xs, info, nxt


@pytest.mark.parametrize("mode", ["irls", "zero_center"])
@pytest.mark.parametrize("block_len", [8, 64])
def test_resident_update_at_partition_edges(mode, block_len):
    if not gpu_available():
        pytest.fail("GPU tests selected but no HIP device / library: the product has no CPU fallback")
    from consenrich_amd import _lib as L
    from consenrich_amd.batch import ModelParams
    from oracle import background as bgo

    lens, ins = E.RESIDENT_LENS, E.resident_inputs()
    mp = ModelParams(state_dim=2)
    lam_first, lam = bgo.penalties(60, 2.0)
    kw = dict(zero_center=mode == "zero_center", use_nonnegative=True, negative_penalty_multiplier=2.0, use_lambda=False,
              use_initial=True)
    xs, info, nxt = _fit_and_update(lens, ins, block_len, kw, lam_first, lam)
    passes = []
    for c, (data, munc) in enumerate(ins):
        w, r, _, _ = bgo.weight_rhs_tracks(data, munc, xs[c][:, 0], np.float32(mp.pad), None, mp.lambda_bounds)
        ref, rinfo = bgo.solve_background(w, r, 0, zero_center=kw["zero_center"], use_nonnegative=True, multiplier=2.0,
                                          initial=np.zeros(lens[c], np.float32), penalties_override=(lam_first, lam),
                                          return_info=True)
        passes.append(rinfo["passes"])
        scale = max(float(np.abs(ref).max()), 1e-6)
        assert info[c]["status"] == L.BG_OK and info[c]["support"] == int(np.count_nonzero(w > 0)), (mode, c)
        assert info[c]["passes"] == rinfo["passes"], (mode, c)
        assert info[c]["weight_scale"] == float(np.median(w[w > 0.0])), (mode, c)
        assert float(np.abs(nxt[c] - ref).max()) <= max(1e-5, 10 * rinfo["roundoff_index"]) * scale + 1e-7, (mode, c)
    if mode == "irls":                  # chains leave the lock-step after different passes (tests/test_bg_truth.py, on the CPU)
        assert 0 in passes and 1 in passes and max(passes) >= 2, passes
    else:
        assert len(set(passes)) >= 2, passes
    for c in range(len(lens)):          # a chain's arithmetic does not depend on its neighbours
        xs1, info1, nxt1 = _fit_and_update([lens[c]], [ins[c]], block_len, kw, lam_first, lam)
        assert np.array_equal(xs1[0], xs[c]), (mode, c, "the fit itself differs: not the background's doing")
        assert np.array_equal(nxt1[0], nxt[c]), (mode, block_len, c, float(np.abs(nxt1[0] - nxt[c]).max()))
        assert info1[0] == info[c], (mode, block_len, c, info1[0], info[c])
