"""GPU tests of the gain summary's finite filter and radix select (csrc/csr_gain.h; run with -m gpu) at the places the two
whole-chain tests (tests/test_gpu_residency.py, tests/test_gpu_level_model.py: every gain finite, count == n) never reach: rows
that lose some or all of their values to the filter, the `hi = min(lo + 1, count - 1)` clamp at counts below four, heavy ties (all
six targets under one prefix through all eight passes), dropped elements on the edges of a workgroup's 4096-element chunk and a
chunk that contributes nothing.

The reference is the NumPy restatement those tests use (`_finalForwardReplicateGainContigSummary`, core.py:7671-7731: np.isfinite
filter, np.mean / np.median / np.std / np.quantile of the float64 gains), with their tolerances.

Gains are made non-finite without touching the fit: `gain_summary(use_lambda=True)` reads the resident lambda track whatever the
forward pass's flags were, and `upload_multipliers` takes what it is given -- so a lambda track with NaN at chosen bins, a forward
pass WITHOUT `USE_LAMBDA` (every test asserts that the covariance it hands out is finite everywhere), and the filter is the only
thing that removes a value.  +-inf in lambda is clipped to the bounds and stays counted."""
import math

import numpy as np
import pytest

import cases
from conftest import gpu_available

pytestmark = pytest.mark.gpu

M = 3
SEED = 9700
PAD = float(np.float32(1.0e-4))     # (a float32 value: `munc = -pad` then meets the 1e-12 floor exactly)
NAN = np.float32(np.nan)


@pytest.fixture(scope="module")
def product():
    if not gpu_available():
        pytest.fail("GPU tests selected but no HIP device / library: the product has no CPU fallback")
    from consenrich_amd import cconsenrich

    return cconsenrich


def _model(dim):
    from consenrich_amd.batch import ModelParams

    return ModelParams(state_dim=2) if dim == 2 else ModelParams(state_dim=1, Q0=((1e-3, 0), (0, 0)))


def _reference(p00, lam, bounds, munc_row, pad):
    prec = np.clip(lam.astype(np.float64), *bounds)             # (np.clip hands a NaN through)
    g = (p00 * prec) / np.maximum(munc_row.astype(np.float64) + pad, 1.0e-12)
    return g[np.isfinite(g)]


def _compare(got, j, g, tag):
    """one row of `DeviceBatch.gain_summary` against the finite gains `g` of that row"""
    assert got["count"][j] == g.size, tag
    if g.size == 0:
        for k in ("mean", "median", "sd", "iqr"):
            assert math.isnan(got[k][j]), (tag, k)
        return
    q25, q75 = np.quantile(g, [0.25, 0.75])
    assert got["median"][j] == float(np.median(g)), tag
    assert got["iqr"][j] == float(q75 - q25), tag
    assert got["mean"][j] == pytest.approx(float(np.mean(g)), rel=1e-12), tag
    assert got["sd"][j] == pytest.approx(float(np.std(g)), rel=1e-10, abs=1e-300), tag
    if g.size == 1:
        assert got["sd"][j] == 0.0 and got["iqr"][j] == 0.0 and got["median"][j] == float(g[0]), tag


def _run(dim, sets, lams, bounds_list, pad=PAD, filtered=None):
    """Fit (no lambda in the pass), then the summary of EVERY row of EVERY chain under each pair of lambda bounds against NumPy.
    Returns {(bounds index, chain, row): (count, n, finite gains)}; `filtered[c]` = (xf, Pf) of chain c where a dict is given."""
    from consenrich_amd import _lib as L
    from consenrich_amd.batch import DeviceBatch

    mp = _model(dim)
    n_list = [d_.shape[1] for d_, _ in sets]
    rows = {}
    with DeviceBatch(0) as b:
        b.configure(mp, M, n_list)
        for c, (d_, v_) in enumerate(sets):
            b.upload(c, d_, v_)
            b.upload_multipliers(c, lams[c], None, None)
        b.stats()
        b.forward(L.RETURN_NLL)
        b.export(L.EXPORT_FORWARD | L.EXPORT_MULT)
        for c, n in enumerate(n_list):
            Pf, lam = b.download(c, "Pf"), b.download(c, "lambda")
            assert Pf.shape == (n, dim, dim) and np.all(np.isfinite(Pf)), c         # the filter alone removes values
            assert np.array_equal(lam.view(np.uint32), lams[c].view(np.uint32)), c   # the track as uploaded, NaN and inf included
            if filtered is not None:
                filtered[c] = (b.download(c, "xf"), Pf)
            p00 = np.maximum(Pf.astype(np.float64)[:, 0, 0], 0.0)
            for k, bounds in enumerate(bounds_list):
                got = b.gain_summary(c, pad, use_lambda=True, lambda_bounds=bounds)
                for j in range(M):
                    g = _reference(p00, lam, bounds, sets[c][1][j], pad)
                    _compare(got, j, g, (dim, bounds, c, j))
                    rows[(k, c, j)] = (g.size, n, g)
    assert any(0 < cnt < n for cnt, n, _ in rows.values()) and any(cnt == 0 for cnt, _, _ in rows.values())
    return rows


def _lambda(n, seed, drop):
    """a finite lambda track that straddles the clamp, NaN at the bins `drop`"""
    lam = cases.multipliers(n, seed)[0].copy()
    lam[np.asarray(drop, np.int64)] = NAN
    return lam


@pytest.mark.parametrize("dim", [2, 1], ids=["levelTrend", "level"])
def test_small_finite_counts_and_empty_rows(product, dim):
    """Chains of 9 bins with 0, 1, ... 8 finite gains (the other bins' lambda is NaN): count == 0 gives NaN for every figure and
    unused targets, count == 1 a standard deviation and an inter-quartile range of exactly 0, counts below four clamp `hi` to the
    last element; an infinite lambda is clipped to a bound and stays counted."""
    rng = np.random.default_rng(SEED)
    n = 9
    sets = [cases.synth(n, M, SEED + c, mask_frac=0.05) for c in range(9)]
    lams = []
    for keep in range(9):
        lam = _lambda(n, SEED + keep, rng.permutation(n)[keep:])
        finite = np.flatnonzero(np.isfinite(lam))
        if keep in (5, 8):
            lam[finite[0]] = np.float32(np.inf)
        if keep in (2, 8):
            lam[finite[-1]] = np.float32(-np.inf)
        lams.append(lam)
    rows = _run(dim, sets, lams, [_model(dim).lambda_bounds])
    assert sorted({cnt for cnt, _, _ in rows.values()}) == list(range(9))


@pytest.mark.parametrize("dim", [2, 1], ids=["levelTrend", "level"])
def test_dropped_elements_on_chunk_edges_and_an_empty_chunk(product, dim):
    """A workgroup folds 256 x 16 = 4096 elements: chains of 4095, 4096, 4097 and 8193 bins with NaN at bins 0, 4095, 4096 and
    n - 1 where they exist; a second 8193-bin chain loses the whole chunk [4096, 8192) as well (one workgroup contributes nothing,
    the next holds one dropped element alone); a 4097-bin chain loses everything (no workgroup contributes)."""
    n_list = [4095, 4096, 4097, 8193, 8193, 4097]
    sets = [cases.synth(n, M, SEED + 20 + c, mask_frac=0.02, outlier_frac=0.01) for c, n in enumerate(n_list)]
    lams = []
    for c, n in enumerate(n_list):
        drop = [k for k in (0, 4095, 4096, n - 1) if k < n]
        if c == 4:
            drop += list(range(4096, 8192))
        if c == 5:
            drop = list(range(n))
        lams.append(_lambda(n, SEED + 20 + c, drop))
    rows = _run(dim, sets, lams, [_model(dim).lambda_bounds])
    want = [4095 - 2, 4096 - 2, 4097 - 3, 8193 - 4, 8193 - 4 - 4095, 0]
    assert [rows[(0, c, 0)][0] for c in range(len(n_list))] == want


@pytest.mark.parametrize("dim", [2, 1], ids=["levelTrend", "level"])
def test_ties_the_variance_floor_and_a_random_third_dropped(product, dim):
    """Heavy ties, the 1e-12 floor and a mixed row, each row against NumPy:

    * chain 4, replicate 1: every `munc` cell is +inf ("no observation"): the cell weighs exactly 0 in the statistics (the
      covariance stays finite, as the reference's division leaves it) and EVERY counted gain of the row is +0.0 -- the six
      targets share one prefix through all eight passes (one histogram serves them all).
    * lambda bounds (0, 0), all chains again: the precision factor of every counted bin is +0.0, the same ties in every row.
    * chain 0, replicate 2: `munc` takes the two values 1e30 and 2e30 (weights below the rounding of the other replicates' sum:
      the covariance does not see them) while the other two swap 0.25 and 0.5 from bin to bin (the same sum of weights in every
      bin) -- the covariance reaches its fixed point, the row's gains fall into two tied runs, 251 values in the lower one: the
      25 % position (250, 251 of 1001) lies ON the boundary between the runs, the median and the 75 % position inside the upper
      one.  (The other two rows hold two tied runs of 500 and 501: the median on their boundary.  No row is one constant: the
      deviation of such a row is the rounding of its mean, in NumPy as on the device, and the gate on `sd` is relative.)
    * chain 1, replicate 1: `munc` = -pad exactly: the variance is floored at 1e-12, gains of 1e12 times the covariance.
    * chain 2: 1031 bins, about 30 % of them dropped at random positions.  chain 3: nothing finite."""
    rng = np.random.default_rng(SEED + 40)
    n0, lead = 1601, 600
    d0, v0 = cases.synth(n0, M, SEED + 40)
    odd = (np.arange(n0) & 1) == 1
    v0[0] = np.where(odd, np.float32(0.5), np.float32(0.25))           # (the pair swaps from bin to bin: the sum of the two
    v0[1] = np.where(odd, np.float32(0.25), np.float32(0.5))           # weights is the same number in every bin)
    kept = np.arange(lead, n0)
    low = rng.permutation(kept)[:251]
    v0[2] = np.float32(1.0e30)
    v0[2, low] = np.float32(2.0e30)
    lam0 = np.ones(n0, np.float32)                      # (inside the bounds: the precision factor is exactly 1)
    lam0[:lead] = NAN                                   # the transient of the covariance from its initial 1000
    d1, v1 = cases.synth(300, M, SEED + 41, mask_frac=0.02)
    v1[1] = -np.float32(PAD)
    d2, v2 = cases.synth(1031, M, SEED + 42, mask_frac=0.02, outlier_frac=0.01)
    d3, v3 = cases.synth(9, M, SEED + 43)
    d4, v4 = cases.synth(517, M, SEED + 44, mask_frac=0.02)
    v4[1] = np.float32(np.inf)
    sets = [(d0, v0), (d1, v1), (d2, v2), (d3, v3), (d4, v4)]
    lams = [lam0, _lambda(300, SEED + 41, [7, 299]), _lambda(1031, SEED + 42, np.flatnonzero(rng.random(1031) < 0.3)),
            np.full(9, NAN, np.float32), _lambda(517, SEED + 44, [0, 256, 516])]
    bounds = _model(dim).lambda_bounds
    filtered = {}
    rows = _run(dim, sets, lams, [bounds, (0.0, 0.0)], filtered=filtered)
    for (k, c, j), (cnt, n, g) in rows.items():
        if k == 1 and cnt:                              # every counted gain is +0.0
            assert not np.any(g) and not np.any(np.signbit(g)), (c, j)
    cnt, _, g = rows[(0, 4, 1)]                          # the replicate without observations: 514 gains of +0.0
    assert cnt == 517 - 3 and not np.any(g) and not np.any(np.signbit(g))
    assert np.any(rows[(0, 4, 0)][2] > 0.0) and np.any(rows[(0, 4, 2)][2] > 0.0)     # (its neighbours see the covariance)
    if dim == 2:                                        # ... and the filter is the oracle's: the replicate weighs nothing
        from oracle import oracle as orc

        n4 = d4.shape[1]
        xf, Pf = np.zeros((n4, 2), np.float32), np.zeros((n4, 2, 2), np.float32)
        orc.cforwardPass(matrixData=d4, matrixPluginMuncInit=v4, matrixF=np.asarray(cases.F_TREND, np.float32),
                         matrixQ0=np.asarray(_model(2).Q0, np.float32), intervalToBlockMap=np.zeros(n4, np.int32), blockCount=1,
                         stateInit=0.0, stateCovarInit=1000.0, pad=PAD, stateForward=xf, stateCovarForward=Pf,
                         pNoiseForward=np.zeros((n4, 2, 2), np.float32), vectorD=np.zeros(n4, np.float32))
        assert np.all(np.isfinite(Pf)) and np.all(np.isfinite(xf))
        for got, ref, tag in zip(filtered[4], (xf, Pf), ("xf", "Pf")):      # (the parity suite's gate for the filtered arrays)
            np.testing.assert_allclose(got.astype(np.float64), ref.astype(np.float64), rtol=1e-5, atol=2e-6, err_msg=tag)
    cnt, _, g = rows[(0, 0, 2)]
    s = np.sort(g)
    assert cnt == 1001 and s[250] < s[251] and np.all(g[np.isin(kept, low)] <= s[250]), "the 25 % position lies between the two runs"
    assert np.unique(g).size <= cnt // 4, np.unique(g).size          # heavy ties: the covariance stands at its fixed point
    assert float(rows[(0, 1, 1)][2].min()) > 1.0e6 * float(rows[(0, 1, 0)][2].max())   # the floored row: gains of another magnitude
    assert 0.6 * 1031 < rows[(0, 2, 0)][0] < 0.8 * 1031
