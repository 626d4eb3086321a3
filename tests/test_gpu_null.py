"""GPU tests of the robust null on the device (run with -m gpu): centre, scale, DWB template and template scale of a score
track.  Every float is compared by its 64-bit pattern, every integer and string with ==.  Reference: the plain twin
(tests/twin_null.py: the reference's steps with NumPy / SciPy on whole vectors), held equal to the structured twin by
tests/test_null_twin.py."""
import numpy as np
import pytest

import cases
import twin_dwb
import twin_null as T
from conftest import gpu_available

pytestmark = pytest.mark.gpu

BIG = 131073            # one past 64 tiles of the sort and 16 chunks of the sums
SIZES = T.SIZES + (BIG,)


@pytest.fixture(scope="module")
def N():
    if not gpu_available():
        pytest.fail("GPU tests selected but no HIP device / library: the product has no CPU fallback")
    from consenrich_amd import null

    return null


@pytest.fixture(scope="module")
def reference():
    """(kind, n) -> plain twin, computed once and left unchanged; "short": the constructed short-support track at q = 0.05."""
    ref = {(k, n): T.plain_all(T.track(k, n)) for k in T.KINDS for n in SIZES}
    ref["short"] = T.plain_all(T.short_support_track(), 0.05)
    return ref


def _bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


def _drop_in(N, z, q=0.60):
    """The three host-array drop-ins composed as peaks.py:1153-1162 composes the reference's."""
    center, scale, details = N.estimateROCCONull(z, q)
    template, meta = N.prepare_null_residual_template(z, center, scale, q)
    return dict(null_center=center, null_scale=scale, details=details, template_meta=meta, template=template,
                decided_on_host=N.null_and_template(z, q)["decided_on_host"])


# ---------------------------------------------------------------------------------------------------------------
# 1. the drop-ins on host arrays
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", T.KINDS)
def test_drop_ins_equal_the_plain_twin(N, reference, kind):
    bad = {}
    for n in SIZES:
        got, ref = _drop_in(N, T.track(kind, n)), reference[kind, n]
        if not T.same(got, ref):
            bad[n] = T.first_difference(got, ref)
        assert got["decided_on_host"] == (ref["details"]["null_method"] == T.NEAREST), n
    assert bad == {}


def test_only_the_tiny_and_the_constructed_tracks_are_decided_on_the_host(N, reference):
    host = [key for key, r in reference.items() if r["decided_on_host"]]
    assert all(key == "short" or key[1] <= 17 for key in host)
    assert len(host) == 1 + 3 * 6            # the constructed track and n = 1, 2, 3, 4, 5, 15 of the three kinds
    z = T.short_support_track()
    got = _drop_in(N, z, 0.05)
    assert got["decided_on_host"] and T.same(got, reference["short"]), T.first_difference(got, reference["short"])
    # at the default quantile the same track has a central support: decided on the device
    got, ref = _drop_in(N, z), T.plain_all(z)
    assert not got["decided_on_host"] and T.same(got, ref), T.first_difference(got, ref)


def test_template_around_a_given_centre_and_scale(N):
    for n in (27, 129, 8193):
        z = T.track("gauss", n)
        t, meta = N.prepare_null_residual_template(z, 0.25, 1.5, 0.5)
        rt, rmeta = T.plain_template(z, 0.25, 1.5, 0.5)
        assert np.array_equal(_bits(t), _bits(rt)), n
        assert {k: _bits(v).tobytes() for k, v in meta.items()} == {k: _bits(v).tobytes() for k, v in rmeta.items()}, n


def test_template_scale_equals_the_plain_twin(N):
    rng = np.random.default_rng(3)
    for n in (1, 2, 3, 4, 5, 63, 2048, 2049, 8193, 20000):
        x = rng.standard_normal(n) * 0.7
        assert _bits(N.estimate_template_scale(x)) == _bits(T.plain_scale(x)), n
    assert N.estimate_template_scale(np.zeros(100)) == 1.0e-6


def test_the_sort_equals_numpys(N):
    rng = np.random.default_rng(9)
    ties = np.round(rng.standard_normal(50001), 1) + 0.0
    up = np.sort(rng.standard_normal(4097))
    for x in (ties, up, up[::-1].copy(), np.array([3.0]), rng.standard_normal(2048), rng.standard_normal(2049) * 1.0e300,
              np.r_[rng.standard_normal(6000), -rng.random(100) * 1.0e-310]):      # (subnormals sort too)
        assert np.array_equal(_bits(N.sort_values(x)), _bits(np.sort(x)))


def test_negative_zero_changes_at_most_the_sign_of_a_zero(N):
    z = T.track("rounded", 8193)
    z[z == 0.0] = 0.0
    z[::7][z[::7] == 0.0] = -0.0
    z[5] = -0.0
    got, ref = _drop_in(N, z), T.plain_all(z)
    assert got["null_center"] == ref["null_center"] and got["null_scale"] == ref["null_scale"]
    assert got["details"] == ref["details"] and got["template_meta"] == ref["template_meta"]
    assert np.array_equal(got["template"], ref["template"])
    assert np.array_equal(N.sort_values(z), np.sort(z))


def test_value_errors_arrive_before_any_launch(N):
    from consenrich_amd import _lib as L

    for bad, text in (([], "`scoreTrack` must be non-empty"), (np.zeros((2, 2)), "`scoreTrack` must be one-dimensional"),
                      ([1.0, np.nan], "`scoreTrack` contains non-finite values"), ([np.inf] * 20, "`scoreTrack` contains non-finite values")):
        with pytest.raises(ValueError, match=text):
            N.estimateROCCONull(bad)
    with pytest.raises(ValueError, match="`values` contains non-finite values"):
        N.prepare_null_residual_template([1.0, np.nan], 0.0, 1.0)
    for bad, text in (([], "`template` must be non-empty"), ([np.nan], "`template` contains non-finite values")):
        with pytest.raises(ValueError, match=text):
            N.estimate_template_scale(bad)
    # the C ABI itself: the reference's text, the value-error code, nothing launched
    lib, out, x = L.lib(), L.NullOut(), np.array([1.0, np.nan, 2.0])
    import ctypes as C

    assert lib.csr_null_prepare(L.dp(x), 3, 0.6, None, C.byref(out), None) == L.NULL_ERR_VALUE
    assert L.last_error() == "`scoreTrack` contains non-finite values"
    assert lib.csr_null_prepare(L.dp(x), 0, 0.6, None, C.byref(out), None) == L.NULL_ERR_VALUE
    assert L.last_error() == "`scoreTrack` must be non-empty"
    assert lib.csr_null_scale(L.dp(x), 3, L.dp(np.zeros(4))) == L.NULL_ERR_VALUE
    assert L.last_error() == "`template` contains non-finite values"


# ---------------------------------------------------------------------------------------------------------------
# 2. a batch: resident scores in, resident templates out
# ---------------------------------------------------------------------------------------------------------------
CHAINS = (8192, 1, 20000, 5, 16, BIG, 27, 63, 8193, 64, 65)     # short between long
ARRAYS = ("D", "xf", "Pf", "pnoise", "xs", "Ps", "lag")


def _chain_track(c, n):
    return T.track(("gauss", "rounded")[c % 2], n, seed=31 + c)


@pytest.fixture(scope="module")
def chain_reference():
    return [T.plain_all(_chain_track(c, n)) for c, n in enumerate(CHAINS)]


def test_a_batch_equals_the_drop_in_per_chain_and_changes_nothing_resident(N, chain_reference):
    from consenrich_amd import _lib as L
    from consenrich_amd.batch import DeviceBatch, ModelParams

    m = 2
    with DeviceBatch(0) as b:
        b.configure(ModelParams(state_dim=2), m, list(CHAINS))
        for c, n in enumerate(CHAINS):
            b.upload(c, *cases.synth(n, m, 900 + c))
        b.stats()
        b.forward_backward(L.RETURN_NLL)
        b.export(L.EXPORT_FORWARD | L.EXPORT_SMOOTH)
        with pytest.raises(L.ConsenrichAMDError, match="no scores"):
            b.rocco_null()
        for c, n in enumerate(CHAINS):
            b.upload_scores(c, _chain_track(c, n))
        before = {(c, a): b.download(c, a) for c in range(len(CHAINS)) for a in ARRAYS}
        with pytest.raises(L.ConsenrichAMDError, match="has no null template"):
            b.download_template(0)
        got = b.rocco_null()
        for c, n in enumerate(CHAINS):
            ref = chain_reference[c]
            res = dict(got[c], template=b.download_template(c))
            assert T.same(res, ref), (n, T.first_difference(res, ref))
            drop = _drop_in(N, _chain_track(c, n))
            assert T.same(res, drop), (n, T.first_difference(res, drop))
            assert got[c]["decided_on_host"] == (n < 16), n
        # a chain mask: new scores everywhere, but only the masked chains are taken again
        for c, n in enumerate(CHAINS):
            b.upload_scores(c, _chain_track(c, n) * 2.0 + 1.0)
        take = [c % 3 == 0 for c in range(len(CHAINS))]
        again = b.rocco_null(chains=take)
        for c, n in enumerate(CHAINS):
            t = b.download_template(c)
            if take[c]:
                ref = T.plain_all(_chain_track(c, n) * 2.0 + 1.0)
                res = dict(again[c], template=t)
                assert T.same(res, ref), (n, T.first_difference(res, ref))
            else:
                assert again[c] is None and np.array_equal(_bits(t), _bits(chain_reference[c]["template"])), n
        # neither the scores nor any array of the fit moved
        for c, n in enumerate(CHAINS):
            assert np.array_equal(_bits(b.download_scores(c)), _bits(_chain_track(c, n) * 2.0 + 1.0)), n
        for (c, a), v in before.items():
            assert np.array_equal(b.download(c, a).view(np.uint32), v.view(np.uint32)), (c, a)


def test_pooled_scale_runs_across_chain_boundaries(N):
    from consenrich_amd.batch import DeviceBatch, ModelParams

    lens = [8193, 70, 12001, 16, 100]       # no multiple of 64 or 8192 among the chains that enter
    with DeviceBatch(0) as b:
        b.configure(ModelParams(state_dim=2), 2, lens)
        for c, n in enumerate(lens):
            b.upload_scores(c, _chain_track(c, n))
        b.rocco_null()
        tmpls = [b.download_template(c) for c in range(len(lens))]
        assert _bits(b.null_pooled_scale()) == _bits(T.plain_scale(np.concatenate(tmpls)))
        assert _bits(b.null_pooled_scale()) == _bits(N.estimate_template_scale(np.concatenate(tmpls)))
        take = [True, True, False, False, True]
        want = T.plain_scale(np.concatenate([t for t, k in zip(tmpls, take) if k]))
        assert _bits(b.null_pooled_scale(chains=take)) == _bits(want)


def _same_views(a, b):
    bad = []
    for c in range(len(a)):
        bad += [(c, d) for d in twin_dwb.same_panel(a[c], b[c])]
    return bad


def test_panel_and_replays_from_the_resident_templates_equal_those_from_the_downloaded_ones(N):
    from consenrich_amd.batch import DeviceBatch, ModelParams

    lens, bws, z_grid = [3000, 65, 9001], [3, 2, 9], (1.5, 2.0, 3.0)
    with DeviceBatch(0) as b:
        b.configure(ModelParams(state_dim=2), 2, lens)
        for c, n in enumerate(lens):
            b.upload_scores(c, _chain_track(c, n))
        with pytest.raises(ValueError, match="rocco_null"):
            b.dwb_panel(threshold_z_grid=z_grid, bandwidths=bws, num_bootstrap=8)
        null = b.rocco_null()
        tmpls = [b.download_template(c) for c in range(len(lens))]
        centers, scales = [r["null_center"] for r in null], [r["null_scale"] for r in null]
        kw = dict(threshold_z_grid=z_grid, bandwidths=bws, num_bootstrap=12, random_seed=4)
        resident = b.dwb_panel(**kw)
        given = b.dwb_panel(tmpls, centers, scales, **kw)
        assert _same_views(resident, given) == []
        rkw = dict(bandwidths=bws, num_replay=3, random_seed=4, min_run_bins=2, max_gap_bins=1, max_segments_per_view=50)
        r_res = b.dwb_replay(None, resident, **rkw)
        r_giv = b.dwb_replay(tmpls, given, **rkw)
        for c in range(len(lens)):
            assert r_res[c]["observed"] == r_giv[c]["observed"], c
            for x, y in zip(r_res[c]["replays"], r_giv[c]["replays"]):
                assert x["candidate_count"] == y["candidate_count"] and x["diagnostics"] == y["diagnostics"]
                for k in ("score", "integrated_excess", "max_excess"):
                    assert np.array_equal(_bits(x[k]), _bits(y[k])), (c, k)
        # the templates are still there, unchanged
        for c in range(len(lens)):
            assert np.array_equal(_bits(b.download_template(c)), _bits(tmpls[c]))
