"""GPU tests of the stationary-null DWB panel on the device (run with -m gpu).  Every float is compared by its 64-bit pattern,
every count with ==.  References: the compiled reference's recorded outputs (tests/golden/dwb/dwb_*.npz) for the natives' case
table; the pure-Python twin (tests/twin_dwb.py, pinned to those recordings and to NumPy by tests/test_dwb_twin.py) for the panel,
evaluated draw by draw with np.quantile / np.mean on whole draws."""
import ctypes as C
import os

import numpy as np
import pytest

import cases
import dwb_cases
import twin_dwb
from conftest import gpu_available

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(dwb_cases.__file__)), "dwb")
Z_GRID = (0.0, 1.5, 2.0, 2.5, 3.0)      # the default grid plus z = 0 (quantile 0.5, the `z > 0` branches)


@pytest.fixture(scope="module")
def product():
    if not gpu_available():
        pytest.fail("GPU tests selected but no HIP device / library: the product has no CPU fallback")
    from consenrich_amd import cconsenrich

    return cconsenrich


@pytest.fixture(scope="module")
def golden():
    out = {}
    for g in dwb_cases.GROUPS:
        out.update(dwb_cases.load_group(os.path.join(GOLDEN, f"dwb_{g}.npz")))
    return out


def _bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


@pytest.mark.parametrize("group", dwb_cases.GROUPS)
def test_case_table_equals_the_reference(product, golden, group):
    """mult: bartlett / parzen / qs x bandwidths 0, 1 (both -> 2), 2, 3, 17, 64 x n = 1 (noise exactly 2 maxLag + 1 long), 2, 3, 65;
    other spellings of the names; constant noise, all-zero noise and a NaN in the noise (multipliers 1.0).  tiles: n around the
    walk's 64-value fetch and the 256-value tile of the walk and the stencil (T-1, T, T+1, 2T+1), qs at bandwidth 64 (1025 taps).  draw: one draw from
    a caller's generator plus the next normal drawn afterwards; all-zero and constant templates.  apply: n = 0, 1, 65, 300."""
    bad = []
    for c in dwb_cases.cases():
        if c["group"] == group and not dwb_cases.same(dwb_cases.run_case(product, c), golden[c["name"]]):
            bad.append(c["name"])
    assert bad == []


def test_a_draw_leaves_the_callers_generator_where_the_reference_does(product):
    t = np.random.default_rng(1).normal(0.0, 1.0, 300)
    for kern, bw in (("bartlett", 7), ("qs", 3)):
        a, b = np.random.default_rng(99), np.random.default_rng(99)
        got, ref = product.cStationaryNullDWBDraw(t, bw, a, kern), twin_dwb.cStationaryNullDWBDraw(t, bw, b, kern)
        assert np.array_equal(_bits(got), _bits(ref))
        assert _bits(a.standard_normal()) == _bits(b.standard_normal())


def test_the_c_abi_answers_value_errors_before_any_launch(product):
    from consenrich_amd import _lib as L

    lib, z, out = L.lib(), np.zeros(64), np.zeros(64)
    assert lib.csr_dwb_multipliers(L.dp(z), 4, 2, b"bartlett", L.dp(out)) == L.DWB_ERR_VALUE
    assert L.last_error() == "noise length is too short for the requested DWB bandwidth"
    assert lib.csr_dwb_apply(L.dp(z), 4, L.dp(z), 3, L.dp(out)) == L.DWB_ERR_VALUE
    assert L.last_error() == "template and multipliers must have the same length"
    assert lib.csr_dwb_multipliers(L.dp(z), 40, 2, b"boxcar", L.dp(out)) == L.DWB_ERR_VALUE
    assert L.last_error() == "Unknown DWB kernel: boxcar"
    assert lib.csr_dwb_draw(L.dp(z), 10, 3, b"bartlett", L.dp(z), 15, L.dp(out)) == L.DWB_ERR_VALUE
    n = np.array([10], np.int64)
    bw = np.array([3], np.int32)
    assert lib.csr_dwb_panel_begin(None, 1, n.ctypes.data_as(L.I64P), bw.ctypes.data_as(C.POINTER(C.c_int32)), b"parzen", L.dp(z),
                                   L.dp(z), 8 * 16 - 1, 8, 0) == L.DWB_ERR_VALUE
    lag = C.c_int32(0)
    assert lib.csr_dwb_max_lag(64, b" Quadratic-Spectral ", C.byref(lag)) == 0 and lag.value == 512


# ---------------------------------------------------------------------------------------------------------------
# the panel against the twin
# ---------------------------------------------------------------------------------------------------------------
LENS = (129, 8193, 16385)       # below one reduction chunk of 8192, one past it, one past two
BWS = (2, 17, 5)
CENTERS = (0.25, -0.5, 1.0)
SCALES = (0.8, 1.5, 0.05)
SEED = 21


def _inputs():
    rng = np.random.default_rng(404)
    scores = [rng.normal(CENTERS[c], 1.3, n) for c, n in enumerate(LENS)]
    tmpls = [rng.normal(0.0, 1.0, n) * (1.0 + 0.5 * np.sin(np.arange(n) / 50.0)) for n in LENS]
    return scores, tmpls


def _floors():
    f = np.zeros((len(LENS), len(Z_GRID), 2))
    f[0, 2] = (5.0, 0.0)        # a threshold-offset floor that binds
    f[1, 3] = (0.0, 40.0)       # a null-scale floor that binds
    f[2, 1] = (1.0e-9, 1.0e-9)  # floors that do not
    return f


def _twin_panel(scores, tmpls, B, floors, kernel="bartlett", centers=CENTERS, scales=SCALES, bws=BWS, z_grid=Z_GRID, seed=SEED):
    strides = [t.shape[0] + 2 * twin_dwb.max_lag(max(bw, 2), twin_dwb.kernel_code(kernel)) for t, bw in zip(tmpls, bws)]
    noise = twin_dwb.stream(seed, max(int(B), 8) * max(strides))
    return [twin_dwb.panel(scores[c], tmpls[c], centers[c], scales[c], z_grid=z_grid, bandwidth=bws[c], num_bootstrap=B,
                           kernel=kernel, seed=seed, cal_q=0.9, floors=None if floors is None else floors[c], noise=noise)
            for c in range(len(tmpls))]


@pytest.fixture(scope="module")
def reference_panels():
    """the twin's panels, computed once per B and shared"""
    scores, tmpls = _inputs()
    return {B: _twin_panel(scores, tmpls, B, _floors()) for B in (8, 9, 65)}


@pytest.mark.parametrize("B", [8, 9, 65])
def test_panel_equals_the_twin(product, reference_panels, B):
    """Three chains of different length and bandwidth in one call, B across a wavefront of draw lanes (65), five z, pooled floors
    that bind and that do not."""
    from consenrich_amd import dwb

    scores, tmpls = _inputs()
    got = dwb.stationary_null_panel(scores, tmpls, CENTERS, SCALES, threshold_z_grid=Z_GRID, bandwidths=BWS, num_bootstrap=B,
                                    random_seed=SEED, pooled_floors=_floors())
    ref = reference_panels[B]
    for c in range(len(LENS)):
        assert twin_dwb.same_panel(got[c], ref[c]) == [], c
    assert got[0][2]["pooled_floor_applied"] and got[1][3]["pooled_floor_applied"] and not got[2][1]["pooled_floor_applied"]
    assert got[0][2]["threshold_offset"] == 5.0 and got[1][3]["null_scale"] == 40.0
    assert all(m["num_bootstrap"] == B for m in got[0])


@pytest.mark.parametrize("group", [1, 7, 9])
def test_the_result_does_not_depend_on_the_draws_per_group(product, reference_panels, group):
    from consenrich_amd import dwb

    scores, tmpls = _inputs()
    got = dwb.stationary_null_panel(scores, tmpls, CENTERS, SCALES, threshold_z_grid=Z_GRID, bandwidths=BWS, num_bootstrap=9,
                                    random_seed=SEED, pooled_floors=_floors(), draws_per_group=group)
    for c in range(len(LENS)):
        assert twin_dwb.same_panel(got[c], reference_panels[9][c]) == [], c


def test_num_bootstrap_is_raised_to_eight_and_the_quantile_clipped(product, reference_panels):
    from consenrich_amd import dwb

    scores, tmpls = _inputs()
    got = dwb.stationary_null_panel(scores[:1], tmpls[:1], CENTERS[:1], SCALES[:1], threshold_z_grid=Z_GRID, bandwidths=BWS[:1],
                                    num_bootstrap=3, random_seed=SEED, calibration_quantile=5.0)
    ref = twin_dwb.panel(scores[0], tmpls[0], CENTERS[0], SCALES[0], z_grid=Z_GRID, bandwidth=BWS[0], num_bootstrap=3, seed=SEED,
                         cal_q=5.0)
    assert twin_dwb.same_panel(got[0], ref) == [] and got[0][0]["num_bootstrap"] == 8 and got[0][0]["null_quantile"] == 0.999


@pytest.mark.parametrize("kernel", ["parzen", "qs"])
def test_panel_with_the_other_kernels_and_given_tail_quantiles(product, kernel):
    from consenrich_amd import dwb

    rng = np.random.default_rng(17)
    scores, tmpls = [rng.normal(0.0, 1.0, 700)], [rng.normal(0.0, 1.0, 700)]
    tq = (0.6, 0.95, 0.999)
    got = dwb.stationary_null_panel(scores, tmpls, [0.1], [1.0], threshold_z_grid=(0.5, 2.0, 3.0), tail_quantiles=tq,
                                    bandwidths=[3], num_bootstrap=10, kernel=kernel, random_seed=5)
    ref = twin_dwb.panel(scores[0], tmpls[0], 0.1, 1.0, z_grid=(0.5, 2.0, 3.0), bandwidth=3, num_bootstrap=10, kernel=kernel,
                         seed=5, tail_quantiles=tq)
    assert twin_dwb.same_panel(got[0], ref) == []


def test_ties_at_the_threshold(product):
    """Integer scores, null centre 1 and a binding threshold-offset floor of 2: the threshold is exactly 3.0 and many scores equal
    it; `>` is strict, the excess of a tie is 0."""
    from consenrich_amd import dwb

    rng = np.random.default_rng(23)
    n = 9001
    score = rng.integers(0, 6, n).astype(np.float64)
    tmpl = rng.normal(0.0, 0.2, n)
    floors = np.zeros((1, 2, 2))
    floors[0, :, 0] = 2.0
    got = dwb.stationary_null_panel([score], [tmpl], [1.0], [0.5], threshold_z_grid=(2.0, 3.0), bandwidths=[4], num_bootstrap=8,
                                    random_seed=2, pooled_floors=floors)
    ref = twin_dwb.panel(score, tmpl, 1.0, 0.5, z_grid=(2.0, 3.0), bandwidth=4, num_bootstrap=8, seed=2, floors=floors[0])
    assert twin_dwb.same_panel(got[0], ref) == []
    assert got[0][0]["threshold"] == 3.0 and np.count_nonzero(score == 3.0) > 1000
    assert got[0][0]["observed_tail_occupancy"] == np.count_nonzero(score > 3.0) / n


def _zeros_as_one(panel):
    """the same panel with every zero written +0.0"""
    return [{k: (v if isinstance(v, (bool, int)) else np.asarray(v, np.float64) + 0.0) for k, v in m.items()} for m in panel]


def test_an_all_zero_template(product):
    """Every draw is zeros of BOTH signs (0 * multiplier, minus a mean of +0.0), so every offset is 0 and every occupancy 0.  Which
    sign the zero at a given rank of such a draw has is not defined by its values: np.quantile takes whatever np.partition left
    there (measured with NumPy 2.2.6: -0.0 at q = 0.5 and 0.933, +0.0 at 0.977 and above, for one such draw of 129 values), the
    device orders -0.0 before +0.0.  The comparison with the twin is therefore exact in everything but the sign of a zero: both
    sides have every zero written as +0.0 first, then bit patterns are compared as everywhere else."""
    from consenrich_amd import dwb

    n = 129
    score = np.random.default_rng(4).normal(0.0, 1.0, n)
    tmpl = np.zeros(n)
    got = dwb.stationary_null_panel([score], [tmpl], [0.2], [0.7], threshold_z_grid=Z_GRID, bandwidths=[3], num_bootstrap=9,
                                    random_seed=6)
    ref = twin_dwb.panel(score, tmpl, 0.2, 0.7, z_grid=Z_GRID, bandwidth=3, num_bootstrap=9, seed=6)
    assert twin_dwb.same_panel(_zeros_as_one(got[0]), _zeros_as_one(ref)) == []
    for m in got[0]:
        assert np.all(m["upper_tail_offsets"] == 0.0) and m["threshold_offset"] == 0.0 and m["threshold"] == 0.2
        assert np.all(m["null_occupancies"] == 0.0) and np.all(m["null_soft_tails"] == 0.0)
        assert m["budget_occupancy_raw"] == m["observed_tail_occupancy"]


def test_the_tail_statistics_of_a_vector_follow_numpys_summation_order(product):
    """lengths around the 8-value, 128-value and 8192-value steps of NumPy's pairwise sum"""
    from consenrich_amd import dwb

    rng = np.random.default_rng(31)
    for n in (1, 7, 8, 9, 127, 128, 129, 136, 8191, 8192, 8193, 16385, 100003):
        x = rng.normal(0.0, 1.0, n) * 10.0 ** rng.integers(-3, 4, n)
        thr, sc = np.array([-0.5, 0.0, 0.7]), np.array([1.0, 0.0, 2.5])
        cnt, soft = dwb._tail_of_vector(x, thr, sc)
        for k in range(3):
            assert int(cnt[k]) == np.count_nonzero(x > thr[k])
            with np.errstate(over="ignore"):     # (a zero scale counts as the smallest normal number: the excesses overflow)
                want = np.mean(np.clip((x - thr[k]) / max(sc[k], twin_dwb.TINY), 0.0, None))
            assert _bits(soft[k]) == _bits(want), (n, k)


# ---------------------------------------------------------------------------------------------------------------
# on a batch: the observed statistics come from the resident scores
# ---------------------------------------------------------------------------------------------------------------
def test_dwb_panel_of_a_batch_reads_the_resident_scores_and_changes_nothing(product):
    from consenrich_amd import _lib as L
    from consenrich_amd.batch import DeviceBatch, ModelParams

    n_list, m = [3000, 65, 9000], 3
    names = ("D", "xf", "Pf", "pnoise", "xs", "Ps", "lag")
    rng = np.random.default_rng(77)
    tmpls = [rng.normal(0.0, 1.0, n) for n in n_list]
    centers, scales, bws = [0.0, 0.1, -0.2], [1.0, 0.5, 2.0], [3, 2, 9]
    with DeviceBatch(0) as b:
        b.configure(ModelParams(state_dim=2), m, n_list)
        for c, n in enumerate(n_list):
            b.upload(c, *cases.synth(n, m, 4500 + c))
        b.stats()
        b.forward_backward(L.RETURN_NLL)
        b.export(L.EXPORT_FORWARD | L.EXPORT_SMOOTH)
        b.rocco_scores("state")
        before = {(c, a): b.download(c, a) for c in range(len(n_list)) for a in names}
        scores = [b.download_scores(c) for c in range(len(n_list))]
        rocco_before = b.rocco(budget=0.1, gamma=0.5)
        masks_before = [b.rocco_solution(c) for c in range(len(n_list))]
        got = b.dwb_panel(tmpls, centers, scales, threshold_z_grid=Z_GRID, bandwidths=bws, num_bootstrap=9, random_seed=3)
        ref = _twin_panel(scores, tmpls, 9, None, centers=centers, scales=scales, bws=bws, seed=3)
        for c in range(len(n_list)):
            assert twin_dwb.same_panel(got[c], ref[c]) == [], c
        for (c, a), v in before.items():
            assert np.array_equal(b.download(c, a).view(np.uint32), v.view(np.uint32)), (c, a)
        for c in range(len(n_list)):
            assert np.array_equal(_bits(b.download_scores(c)), _bits(scores[c]))
            assert np.array_equal(b.rocco_solution(c), masks_before[c])
        rocco_after = b.rocco(budget=0.1, gamma=0.5)
        for c in range(len(n_list)):
            assert rocco_after[c]["selected_count"] == rocco_before[c]["selected_count"]
            assert np.array_equal(_bits([rocco_after[c][k] for k in ("objective", "penalized_objective", "selection_penalty")]),
                                  _bits([rocco_before[c][k] for k in ("objective", "penalized_objective", "selection_penalty")]))
            assert np.array_equal(b.rocco_solution(c), masks_before[c])
    with DeviceBatch(0) as b:
        b.configure(ModelParams(state_dim=2), 2, [10])
        with pytest.raises(L.ConsenrichAMDError, match="has no scores"):
            b.dwb_panel([np.ones(10)], 0.0, 1.0, threshold_z_grid=(2.0,), bandwidths=2)
