"""CPU: the pure-Python twin of the stationary-null DWB natives (tests/twin_dwb.py) equals the compiled reference's recorded
outputs on every case of the table, bit for bit; its restatements of NumPy's summation order and inverted-CDF quantile equal
NumPy; and the drop-in wrappers raise the reference's errors before any GPU call."""
import os

import numpy as np
import pytest

import dwb_cases
import twin_dwb

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(dwb_cases.__file__)), "dwb")
Z_GRID = (0.0, 1.5, 2.0, 2.5, 3.0)


def _bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def golden():
    out = {}
    for g in dwb_cases.GROUPS:
        out.update(dwb_cases.load_group(os.path.join(GOLDEN, f"dwb_{g}.npz")))
    return out


def test_every_case_has_a_fixture(golden):
    assert sorted(golden) == sorted(c["name"] for c in dwb_cases.cases())


@pytest.mark.parametrize("group", dwb_cases.GROUPS)
def test_twin_equals_the_reference(golden, group):
    bad = [c["name"] for c in dwb_cases.cases() if c["group"] == group
           and not dwb_cases.same(dwb_cases.run_case(twin_dwb, c), golden[c["name"]])]
    assert bad == []


def test_the_degenerate_cases_are_what_the_table_says(golden):
    for name in ("mult_const_n5", "mult_nan_n67", "mult_zero_n67", "mult_bartlett_bw0_n1", "mult_qs_bw64_n1"):
        assert np.array_equal(golden[name]["out"], np.ones_like(golden[name]["out"])), name
    assert np.all(golden["draw_zero_template"]["out"] == 0.0)
    assert golden["apply_n0"]["out"].shape == (0,)
    # bandwidths 0 and 1 count as 2
    for kern in dwb_cases.KERNELS:
        a = twin_dwb.cGenerateDWBMultipliersFromNoise(np.arange(70.0) ** 1.5, 0, kern)
        b = twin_dwb.cGenerateDWBMultipliersFromNoise(np.arange(70.0) ** 1.5, 2, kern)
        assert np.array_equal(_bits(a), _bits(b))


@pytest.mark.parametrize("n", [1, 7, 8, 9, 127, 128, 129, 136, 8191, 8192, 8193, 16385, 100003])
def test_np_order_sum_is_numpys_order(n):
    rng = np.random.default_rng(n)
    x = rng.normal(0.0, 1.0, n) * 10.0 ** rng.integers(-3, 4, n)
    assert _bits(twin_dwb.np_order_sum(x)) == _bits(np.sum(x))
    assert _bits(twin_dwb.np_order_sum(x) / n) == _bits(np.mean(x))
    flags = x > 0.3
    assert _bits(np.count_nonzero(flags) / n) == _bits(np.mean(flags))


@pytest.mark.parametrize("n", [1, 2, 8, 1001])
def test_the_lerp_between_two_order_statistics_is_np_quantile(n):
    x = np.random.default_rng(50 + n).normal(0.0, 1.0, n)
    for q in [twin_dwb.tail_quantile(z) for z in Z_GRID] + [0.9, 0.5, 0.999]:
        assert _bits(twin_dwb.small_quantile(x, q)) == _bits(np.quantile(x, q, method=twin_dwb.QMETHOD)), (n, q)


def test_successive_draws_are_slices_of_one_stream():
    strides = (777 + 4, 130, 9)
    rng = np.random.default_rng(12)
    parts = [rng.standard_normal(s) for s in strides]
    assert np.array_equal(_bits(np.concatenate(parts)), _bits(twin_dwb.stream(12, sum(strides))))
    # ... and a longer stream begins with the shorter one
    assert np.array_equal(_bits(twin_dwb.stream(12, 5000)[:916]), _bits(twin_dwb.stream(12, 916)))


def test_the_fast_draw_equals_the_looped_natives():
    rng = np.random.default_rng(3)
    for kern, bw, n in (("bartlett", 3, 777), ("parzen", 17, 300), ("qs", 2, 130), ("bartlett", 2, 1)):
        lag = twin_dwb.max_lag(bw, twin_dwb.kernel_code(kern))
        t, z = rng.normal(0.0, 2.0, n), rng.standard_normal(n + 2 * lag)
        want = twin_dwb.cApplyStationaryNullDWB(t, twin_dwb.cGenerateDWBMultipliersFromNoise(z, bw, kern))
        assert np.array_equal(_bits(twin_dwb.draw_fast(t, bw, z, kern)), _bits(want))


def test_twin_panel_equals_a_direct_draw_by_draw_evaluation():
    """n = 777, B = 9: the panel put together from order statistics and np_order_sum (the device's way) against the reference's
    own loop shape -- a generator seeded once, cStationaryNullDWBDraw per draw, np.quantile / np.mean on whole draws, re-seeded
    for the second loop."""
    n, B, bw, seed, cal_q = 777, 9, 5, 21, 0.9
    rng = np.random.default_rng(8)
    score = rng.normal(0.3, 1.2, n)
    tmpl = rng.normal(0.0, 1.0, n)
    center, scale = 0.25, 0.8
    floors = [(0.0, 0.0), (0.0, 0.0), (5.0, 0.0), (0.0, 3.0), (0.0, 0.0)]
    fast = twin_dwb.panel(score, tmpl, center, scale, z_grid=Z_GRID, bandwidth=bw, num_bootstrap=B, seed=seed, cal_q=cal_q,
                          floors=floors, fast=True)
    slow = twin_dwb.panel(score, tmpl, center, scale, z_grid=Z_GRID, bandwidth=bw, num_bootstrap=B, seed=seed, cal_q=cal_q,
                          floors=floors, fast=False)
    assert twin_dwb.same_panel(fast, slow) == []
    assert fast[2]["pooled_floor_applied"] and fast[3]["pooled_floor_applied"] and not fast[1]["pooled_floor_applied"]
    # direct: the loops of peaks.py:593-762
    gen = np.random.default_rng(seed)
    draws = [twin_dwb.cStationaryNullDWBDraw(tmpl, bw, gen) for _ in range(B)]
    gen = np.random.default_rng(seed)
    again = [twin_dwb.cStationaryNullDWBDraw(tmpl, bw, gen) for _ in range(B)]
    for k, z in enumerate(Z_GRID):
        upper = np.array([np.quantile(d, twin_dwb.tail_quantile(z), method=twin_dwb.QMETHOD) for d in draws])
        assert np.array_equal(_bits(upper), _bits(fast[k]["upper_tail_offsets"]))
        off = float(fast[k]["threshold"]) - center
        occ = np.array([float(np.mean(d > off)) for d in again])
        soft = np.array([float(np.mean(np.clip((d - off) / max(fast[k]["null_scale"], twin_dwb.TINY), 0.0, None))) for d in again])
        assert np.array_equal(_bits(occ), _bits(fast[k]["null_occupancies"]))
        assert np.array_equal(_bits(soft), _bits(fast[k]["null_soft_tails"]))
        assert _bits(fast[k]["observed_tail_occupancy"]) == _bits(float(np.mean(score > fast[k]["threshold"])))


@pytest.fixture(scope="module")
def product():
    from consenrich_amd import build

    build.build()
    from consenrich_amd import cconsenrich

    return cconsenrich


@pytest.mark.parametrize("who", ["product", "twin"])
def test_wrappers_raise_the_reference_errors_without_a_gpu(product, who):
    mod = product if who == "product" else twin_dwb
    with pytest.raises(ValueError, match="noise length is too short for the requested DWB bandwidth"):
        mod.cGenerateDWBMultipliersFromNoise(np.zeros(4), 2)
    with pytest.raises(ValueError, match="noise length is too short for the requested DWB bandwidth"):
        mod.cGenerateDWBMultipliersFromNoise(np.zeros(64), 3, "qs")
    with pytest.raises(ValueError, match="template and multipliers must have the same length"):
        mod.cApplyStationaryNullDWB(np.zeros(4), np.zeros(3))
    with pytest.raises(ValueError, match="Unknown DWB kernel: boxcar"):
        mod.cGenerateDWBMultipliersFromNoise(np.zeros(40), 2, "boxcar")
    with pytest.raises(ValueError, match="Unknown DWB kernel: boxcar"):
        mod.cStationaryNullDWBDraw(np.zeros(40), 2, np.random.default_rng(0), "boxcar")
    with pytest.raises(OverflowError, match="value too large to convert to int"):
        mod.cGenerateDWBMultipliersFromNoise(np.zeros(40), 2 ** 31)
    assert mod.cApplyStationaryNullDWB([], []).shape == (0,)


def test_the_panel_checks_its_arguments_without_a_gpu(product):
    from consenrich_amd import dwb

    s, t = [np.arange(20.0)], [np.ones(20)]
    kw = dict(threshold_z_grid=(2.0,), bandwidths=3)
    with pytest.raises(ValueError, match="Unknown DWB kernel: boxcar"):
        dwb.stationary_null_panel(s, t, 0.0, 1.0, kernel="boxcar", **kw)
    with pytest.raises(ValueError, match="noise length is too short for the requested DWB bandwidth"):
        dwb.stationary_null_panel(s, t, 0.0, 1.0, noise=np.zeros(8 * 26 - 1), num_bootstrap=2, **kw)
    with pytest.raises(ValueError, match="as long as its chain"):
        dwb.stationary_null_panel(s, [np.ones(19)], 0.0, 1.0, **kw)
    with pytest.raises(ValueError, match="threshold_z_grid"):
        dwb.stationary_null_panel(s, t, 0.0, 1.0, threshold_z_grid=(), bandwidths=3)
    assert dwb.quantile_ranks(1001, 0.5) == twin_dwb.quantile_ranks(1001, 0.5)
    assert dwb.max_lag(0) == 2 and dwb.max_lag(3, "qs") == 32 and dwb.max_lag(64, "quadratic-spectral") == 512


def test_the_callables_are_exported_by_the_drop_in_module(product):
    for name in ("cGenerateDWBMultipliersFromNoise", "cApplyStationaryNullDWB", "cStationaryNullDWBDraw"):
        assert name in product.__all__ and callable(getattr(product, name))
