"""CPU: the two twins of the robust null (tests/twin_null.py) agree bit for bit -- the reference's steps with NumPy / SciPy calls
on whole vectors, and the device's decomposition into ranks of one sort, level-by-level arg-mins, chunked pairwise sums and a
compaction -- plus hand-derived answers for the half-sample mode and the branches the reference can take."""
import numpy as np
import pytest

import twin_null as T


@pytest.fixture(scope="module")
def table():
    """(kind, n) -> (plain, structured), computed once."""
    return {(k, n): (T.plain_all(T.track(k, n)), T.structured_all(T.track(k, n))) for k in T.KINDS for n in T.SIZES}


@pytest.mark.parametrize("kind", T.KINDS)
@pytest.mark.parametrize("n", T.SIZES)
def test_plain_equals_structured_bit_for_bit(table, kind, n):
    a, b = table[kind, n]
    assert T.same(a, b), T.first_difference(a, b)
    z = T.track(kind, n)
    assert np.float64(T.plain_scale(z)).tobytes() == np.float64(T.structured_scale(z)).tobytes()
    given = (0.25, 1.5)         # a template around a centre and a scale that are not the track's own
    t, meta = T.plain_template(z, *given)
    s = T.structured_all(z, given=given)
    assert t.tobytes() == s["template"].tobytes()
    assert {k: np.float64(v).tobytes() for k, v in meta.items()} == {k: np.float64(v).tobytes() for k, v in s["template_meta"].items()}


def test_the_tracks_hold_no_negative_zero_and_the_rounded_kind_has_ties():
    for k in T.KINDS:
        for n in T.SIZES:
            z = T.track(k, n)
            assert not np.any((z == 0.0) & np.signbit(z))
    z = T.track("rounded", 20000)
    assert np.unique(z).size < z.size // 10


@pytest.mark.parametrize("values, want", [
    ([2.5], 2.5),                                   # n = 1
    ([1.0, 4.0], 2.5),                              # n = 2: the mean
    ([1.0, 2.0, 4.0], 1.5),                         # n = 3: the left pair is narrower
    ([1.0, 3.0, 4.0], 3.5),                         # n = 3: the right pair is narrower
    ([1.0, 2.0, 3.0], 1.5),                         # n = 3: a tie goes to the left pair
    ([0.0, 1.0, 1.5, 9.0], 1.25),                   # n = 4: window 2, widths 1, 0.5, 7.5 -> (1, 1.5)
    ([0.0, 5.0, 6.0, 6.5, 20.0], 6.25),             # n = 5 (odd: window 3): widths 6, 1.5, 14 -> (5, 6, 6.5) -> right pair
    ([0.0, 1.0, 2.0, 10.0, 11.0, 12.0], 0.5),       # even window 3; the two windows (0,1,2) and (10,11,12) tie: the first wins
    ([0.0, 3.0, 4.0, 10.0, 10.5, 11.0], 10.25),     # even window 3: widths 4, 7, 6.5, 1 -> (10, 10.5, 11): a tie -> left pair
])
def test_half_sample_mode_known_answers(values, want):
    v = np.asarray(values, np.float64)
    assert T.plain_half_sample_mode(v) == want
    assert T.level_half_sample_mode(v) == want


def test_half_sample_mode_takes_the_first_of_equal_windows_at_every_level():
    v = np.arange(64) * 0.5             # every window of every level is equally wide: start 0 wins down to (0, 0.5)
    assert T.plain_half_sample_mode(v) == 0.25 == T.level_half_sample_mode(v)
    w = np.r_[np.arange(8) * 1.0, 100.0 + np.arange(9) * 1.0]      # 17 values, window 9: the upper nine are the only tight window
    assert T.plain_half_sample_mode(w) == T.level_half_sample_mode(w) == 100.5


def test_branches_of_the_sample_track(table):
    """Full-track bulk up to n = 26, the lower bulk from n = 27 (16 values at or below the 0.6 quantile need n >= 27); the median
    centre below 4 values; below 16 values the support can never reach minSupport."""
    for n in T.SIZES:
        d = table["gauss", n][0]["details"]
        source = "full_track" if n <= 26 else "lower_bulk"
        assert d["center_method"] == f"{source}_{'median' if n < 4 else 'half_sample_mode'}", n
        assert d["lower_bulk_size"] == n if n <= 26 else 16 <= d["lower_bulk_size"] < n, n
        if n < 16:
            assert d["null_method"] == T.NEAREST and d["support_size"] == n, n
        if n >= 26:
            assert d["null_method"] == T.CENTRAL, n
        assert table["gauss", n][0]["decided_on_host"] == (d["null_method"] == T.NEAREST)
        assert d["scale_method"] == "central_support_mad" and d["bulk_quantile"] == 0.6


def test_constant_track_hits_the_scale_floor_and_gives_a_zero_template(table):
    for n in T.SIZES:
        a = table["constant", n][0]
        assert a["null_center"] == 0.75 and a["null_scale"] == 1.0e-6
        assert a["details"]["support_scale"] == 1.0e-6 and a["details"]["support_radius"] == 2.5 * 1.0e-6
        assert not np.any(a["template"]) and a["template_meta"]["template_std"] == 0.0 == a["template_meta"]["template_mean"]
        assert a["template_meta"]["clip_abs"] == 1.0e-6


def test_short_central_support_takes_the_nearest_support_branch():
    z = T.short_support_track()
    a, b = T.plain_all(z, 0.05), T.structured_all(z, 0.05)
    assert T.same(a, b), T.first_difference(a, b)
    d = a["details"]
    assert d["null_method"] == T.NEAREST and a["decided_on_host"]
    assert d["center_method"] == "lower_bulk_half_sample_mode" and d["lower_bulk_size"] == 50 == d["support_size"]
    assert d["provisional_center"] == 0.0078125        # the first window wins at every level: the mean of the two lowest values
    assert np.count_nonzero(np.abs(z - d["provisional_center"]) <= d["support_radius"]) < 50


def test_fewer_than_four_support_values_clip_by_the_whole_centred_track():
    z = np.array([0.5, 3.0, -1.0])
    support, meta = T.plain_support(z)
    assert support.size == 3 and meta["center_method"] == "full_track_median" and meta["provisional_center"] == 0.5
    t, tmeta = T.plain_template(z, 0.5, 2.0)
    # |centred| = 0, 2.5, 1.5: the 0.95 quantile of three values is the largest (virtual index 1.85 -> lerp(1.5, 2.5, 0.85))
    assert tmeta["clip_abs"] == float(np.quantile(np.abs(z - 0.5), 0.95, method=T.QM)) > 2.0
    assert T.same(T.plain_all(z), T.structured_all(z))


def test_bulk_quantile_is_clipped_and_bad_input_raises_the_reference_texts():
    z = T.track("gauss", 129)
    assert T.plain_null(z, 0.0)[2]["bulk_quantile"] == 0.05 and T.plain_null(z, 2.0)[2]["bulk_quantile"] == 0.95
    for bad, text in (([], "`scoreTrack` must be non-empty"), (np.zeros((2, 2)), "`scoreTrack` must be one-dimensional"),
                      ([1.0, np.nan], "`scoreTrack` contains non-finite values"), ([1.0, np.inf], "`scoreTrack` contains non-finite values")):
        with pytest.raises(ValueError, match=text):
            T.plain_null(bad)
        with pytest.raises(ValueError, match=text):
            T.structured_all(bad)


def test_the_references_own_expectations_on_a_toy_track():
    """What the reference's suite asserts of `estimateROCCONull` on |state| + 3 of its toy chromosome, on a toy of our own: a
    smooth background with three enriched stretches."""
    rng = np.random.default_rng(5)
    state = 0.3 * rng.standard_normal(600)
    for lo, hi, h in ((80, 110, 4.0), (300, 360, 6.0), (500, 520, 3.0)):
        state[lo:hi] += h
    center, scale, d = T.plain_null(np.abs(state) + 3.0)
    assert d["null_method"] == "mode_centered_central_support"
    assert d["center_method"] == "lower_bulk_half_sample_mode"
    assert np.isfinite(center) and np.isfinite(scale) and scale > 0.0
    assert d["provisional_center"] > 2.5 and d["null_center"] > 2.5
    assert d["support_fraction"] > 0.25 and d["support_radius"] > 0.0
    assert T.same(T.plain_all(np.abs(state) + 3.0), T.structured_all(np.abs(state) + 3.0))
