"""CPU tests (no GPU) of the yardstick behind tests/test_gpu_bg_edges.py:

  * oracle/bg_truth.py `solve_truth` (long-double banded LDL' of the system assembled from its definition) against a 256-bit solve;
  * the oracle's `csolveZeroCenteredBackground` -- the reference's sequential LDL', pinned bit for bit to the compiled reference --
    against that truth over the whole table of tests/golden/bg_edge_cases.py, under the gate the device is held to:
        max|x - truth| / scale <= 4 * 2^-52 * cond2(A),   scale = max(max|truth_plain|, max|truth_zc|);
  * the table itself: the condition-number cap, and the partition classes (number of blocks, last-block length, separators) that
    its lengths are there for;
  * the pass counts of the resident fixture (0, 1 and >= 2 IRLS passes in one batch), with the oracle's own smoother for the level.

Every truth is computed once per module."""
import numpy as np
import pytest

import bg_edge_cases as E
from oracle import background as bgo
from oracle import bg_truth as T
from oracle import oracle as orc

EPS = 2.0 ** -52
GATE = 4.0
CASES = E.edge_cases()


@pytest.fixture(scope="module")
def table():
    """name -> (w, r, lam_first, lam, cond2, (truth_plain, truth_zc) in long double, scale); singular cases are not in it"""
    out = {}
    for c in CASES:
        if c["singular"]:
            continue
        w, r = E.edge_inputs(c)
        lam_first, lam = E.edge_lams(c)
        pair = T.solve_longdouble(w, r, lam_first, lam, True)
        scale = float(max(np.abs(pair[0]).max(), np.abs(pair[1]).max()))
        out[c["name"]] = (w, r, lam_first, lam, T.cond2(w, lam_first, lam), pair, scale)
    return out


def partition(n, bp):
    """`bg_partition` (csr_host_rows.inl): (number of blocks K, length of the last block)"""
    k = -(-n // bp)
    k -= 1 if k > 1 and n - (k - 1) * bp < 4 else 0
    return k, n - (k - 1) * bp


# ---- the truth against 256 bits ----------------------------------------------------------------------------------------
def _mp_solve(mp, w, r, lam_first, lam):
    """(plain, zero-centred) at the working precision of `mp`: the quadratic form written out row by row, Gaussian elimination
    without pivoting inside the band (A is SPD)"""
    n = len(w)
    A = [dict() for _ in range(n)]

    def add(i, j, v):
        A[i][j] = A[i].get(j, mp.mpf(0)) + v

    lf, l2 = mp.mpf(lam_first), mp.mpf(lam)
    for i in range(n):
        add(i, i, mp.mpf(float(w[i])))
    for i in range(n - 1):
        for a, ca in ((i, -1), (i + 1, 1)):
            for b, cb in ((i, -1), (i + 1, 1)):
                add(a, b, lf * ca * cb)
    for i in range(n - 2):
        for a, ca in ((i, 1), (i + 1, -2), (i + 2, 1)):
            for b, cb in ((i, 1), (i + 1, -2), (i + 2, 1)):
                add(a, b, l2 * ca * cb)
    rhs = [[mp.mpf(float(v)), mp.mpf(1)] for v in r]
    for i in range(n):
        piv = A[i][i]
        assert piv > 0
        for k in (i + 1, i + 2):
            if k < n and i in A[k]:
                f = A[k][i] / piv
                for j, v in A[i].items():
                    if j > i:
                        A[k][j] = A[k].get(j, mp.mpf(0)) - f * v
                rhs[k] = [rhs[k][q] - f * rhs[i][q] for q in range(2)]
    x = [None] * n
    for i in range(n - 1, -1, -1):
        acc = list(rhs[i])
        for j, v in A[i].items():
            if j > i:
                acc = [acc[q] - v * x[j][q] for q in range(2)]
        x[i] = [a / A[i][i] for a in acc]
    mu = mp.fsum(v[0] for v in x) / mp.fsum(v[1] for v in x)
    return [v[0] for v in x], [v[0] - mu * v[1] for v in x]


def _to_mp(mp, v):
    hi = float(v)
    return mp.mpf(hi) + mp.mpf(float(v - np.longdouble(hi)))          # a long double is the exact sum of two doubles


def test_truth_matches_256_bit_solve(table):
    """On n <= 80 and n = 513: the long-double solution is within 2^-60 cond2 of scale of the 256-bit one (about 16 long-double
    roundings times cond2 -- what a backward-stable banded LDL' of these lengths leaves), and `solve_truth` / `solve_truth_pair`
    return exactly its rounding to float64."""
    mpmath = pytest.importorskip("mpmath")
    mp = mpmath.mp.clone()
    mp.prec = 256
    worst, count = 0.0, 0
    for c in CASES:
        if c["singular"] or not (c["n"] <= 80 or c["n"] == 513):
            continue
        w, r, lam_first, lam, cond, pair, scale = table[c["name"]]
        want = _mp_solve(mp, w, r, lam_first, lam)
        for got, ref in zip(pair, want):
            err = max(abs(_to_mp(mp, g) - x) for g, x in zip(got, ref))
            ratio = float(err / (mp.mpf(2) ** -60 * cond * scale))
            worst = max(worst, ratio)
            assert ratio <= 1.0, (c["name"], ratio)
        count += 1
    assert count >= 140
    print(f"\nworst |long double - 256 bit| / (2^-60 cond2 scale) over {count} cases: {worst:.4f}")
    for name in ("bp8_n7_span30_masked", "bp8_n513_span100_plain"):
        w, r, lam_first, lam, _, pair, _ = table[name]
        both = T.solve_truth_pair(w, r, lam_first, lam)
        for zc in (False, True):
            one = T.solve_truth(w, r, lam_first, lam, zc)
            assert one.dtype == np.float64 and np.array_equal(one, pair[zc].astype(np.float64)) and np.array_equal(one, both[zc])


def test_truth_raises_without_a_positive_pivot():
    for c in CASES:
        if not c["singular"]:
            continue
        w, r = E.edge_inputs(c)
        assert not w.any()
        for zc in (False, True):
            with pytest.raises(np.linalg.LinAlgError, match="not positive"):
                T.solve_truth(w, r, *E.edge_lams(c), zc)
        if c["n"] == 1:      # (zero-centring a single bin returns 0 before anything is factorised, as in the reference)
            assert orc.csolveZeroCenteredBackground(w, r, E.edge_lams(c)[1], True, lamFirst=E.edge_lams(c)[0])[0] == 0.0
        with pytest.raises(RuntimeError, match=rf"pivot modification at index {c['n'] - 1} \(pivot=0, floor=1e-12\)"):
            orc.csolveZeroCenteredBackground(w, r, E.edge_lams(c)[1], False, lamFirst=E.edge_lams(c)[0])
    with pytest.raises(np.linalg.LinAlgError):
        T.cond2(np.zeros(5), 3.0, 7.0)


def test_truth_small_systems_by_hand():
    """n = 1, 2, 3 written out: the boundary rows of the definition (not of any stencil table)"""
    assert T.solve_truth([2.0], [8.0], 6.0, 9.0, False)[0] == 4.0
    lf, lam = 3.0, 5.0
    for w, A in (([2.0, 7.0], [[2 + lf, -lf], [-lf, 7 + lf]]),
                 ([2.0, 7.0, 4.0], [[2 + lf + lam, -lf - 2 * lam, lam], [-lf - 2 * lam, 7 + 2 * lf + 4 * lam, -lf - 2 * lam],
                                    [lam, -lf - 2 * lam, 4 + lf + lam]])):
        r = np.arange(1.0, len(w) + 1.0)
        A = np.asarray(A)
        x = np.linalg.solve(A, r)
        np.testing.assert_allclose(T.solve_truth(w, r, lf, lam, False), x, rtol=1e-14)
        u = np.linalg.solve(A, np.ones(len(w)))
        z = T.solve_truth(w, r, lf, lam, True)
        np.testing.assert_allclose(z, x - x.sum() / u.sum() * u, rtol=0, atol=1e-14 * np.abs(x).max())
        assert abs(z.sum()) <= 1e-15 * np.abs(x).max() * len(w)
        assert T.cond2(w, lf, lam) == pytest.approx(np.linalg.cond(A), rel=1e-12)


# ---- the table ---------------------------------------------------------------------------------------------------------
def test_every_case_is_under_the_condition_cap(table):
    worst = max(table.values(), key=lambda v: v[4])[4]
    for name, v in table.items():
        assert v[4] <= E.COND_CAP, (name, v[4])
    assert GATE * EPS * worst <= 2.0e-7
    assert len(table) + sum(c["singular"] for c in CASES) == len(CASES) == len({c["name"] for c in CASES})
    big = [c for c in CASES if c["n"] > E.LONG]
    assert big and all(c["span"] == 100 and c["kind"] == "masked" for c in big)


def test_banded_and_dense_condition_numbers_agree(table):
    w, _, lam_first, lam, cond = table["bp8_n1040_span100_masked"][:5]
    old, T.DENSE_MAX = T.DENSE_MAX, 100
    try:
        assert T.cond2(w, lam_first, lam) == pytest.approx(cond, rel=1e-6)
    finally:
        T.DENSE_MAX = old


def test_table_covers_the_partition_classes():
    """Each length tagged with (K blocks, last-block length, last block longer than Bp); what the table is there for."""
    tags = {}
    for c in CASES:
        bp = E.block_len(c["bp"])
        k, last = partition(c["n"], bp)
        assert (k - 1) * bp + last == c["n"] and (k == 1 or 4 <= last <= bp + 3) and last <= bp + 3
        tags.setdefault(c["bp"], set()).add((k, last - bp if k > 1 else None, last > bp))
    for bp in (8, 64):         # a last block of 4 bins, of exactly Bp, and of Bp + 1, 2, 3 behind a separator
        assert {d for k, d, _ in tags[bp] if k > 1} >= {4 - bp, 0, 1, 2, 3}, bp
        assert {k for k, _, _ in tags[bp]} >= {2, 64, 65, 66}, bp
    assert {d for k, d, _ in tags[0] if k > 1} >= {4 - 1024, 0, 1, 3} and {k for k, _, _ in tags[0]} == {2, 3}
    assert any(k == 1 and longer for k, _, longer in tags[8])                  # one block of Bp + 1 .. Bp + 3 bins, no separator
    ks = {k for t in tags.values() for k, _, _ in t}
    assert ks >= {1, 2, 64, 65, 66}
    assert {k - 1 for k in ks} >= {63, 64, 65, 128}                            # nsep: the 64-separator staging of k_bg_reduced
    # the 64-interior groups of k_bg_local fill up at K = 64 and spill at K = 65 with every last-block class behind them
    for bp in (8, 64):
        assert {d for k, d, _ in tags[bp] if k == 64} >= {0, 1, 3} and {d for k, d, _ in tags[bp] if k == 65} >= {4 - bp}


# ---- the reference's own distance from the truth -----------------------------------------------------------------------------
def test_oracle_meets_the_gate_over_the_whole_table(table):
    worst = {}
    for c in CASES:
        if c["singular"]:
            continue
        w, r, lam_first, lam, cond, pair, scale = table[c["name"]]
        for zc in (False, True):
            got = orc.csolveZeroCenteredBackground(w, r, lam, zc, lamFirst=lam_first)
            ratio = float(np.abs(got - pair[zc].astype(np.float64)).max()) / scale / (EPS * cond)
            key = (c["bp"], c["span"], c["kind"], zc)
            worst[key] = max(worst.get(key, 0.0), ratio)
            assert ratio <= GATE, (c["name"], zc, ratio)
    print("\nworst |oracle - truth| / (scale 2^-52 cond2) per (Bp, span, kind, zero-centre):")
    for key in sorted(worst):
        print("  ", key, f"{worst[key]:.4f}")


# ---- the resident fixture ------------------------------------------------------------------------------------------------
def test_resident_fixture_stops_after_0_1_and_more_passes():
    import cases

    lam_first, lam = bgo.penalties(60, 2.0)
    F, Q0 = np.asarray(cases.F_TREND, np.float32), np.asarray([[1.0e-3, 0.0], [0.0, 1.0e-4]], np.float32)
    passes = []
    for data, munc in E.resident_inputs():
        n = data.shape[1]
        xf, Pf, pn = np.zeros((n, 2), np.float32), np.zeros((n, 2, 2), np.float32), np.zeros((n, 2, 2), np.float32)
        orc.cforwardPass(matrixData=data, matrixPluginMuncInit=munc, matrixF=F, matrixQ0=Q0, intervalToBlockMap=np.zeros(n, np.int32),
                         blockCount=1, stateInit=0.0, stateCovarInit=1000.0, pad=1.0e-4, stateForward=xf, stateCovarForward=Pf,
                         pNoiseForward=pn, vectorD=np.zeros(n, np.float32))
        xs = orc.cbackwardPass(matrixData=data, matrixF=F, stateForward=xf, stateCovarForward=Pf, pNoiseForward=pn)[0]
        w, r, _, _ = bgo.weight_rhs_tracks(data, munc, xs[:, 0], np.float32(1.0e-4), None, (0.25, 4.0))
        _, info = bgo.solve_background(w, r, 0, zero_center=False, use_nonnegative=True, multiplier=2.0,
                                       initial=np.zeros(n, np.float32), penalties_override=(lam_first, lam), return_info=True)
        passes.append(info["passes"])
    assert 0 in passes and 1 in passes and max(passes) >= 2, passes
