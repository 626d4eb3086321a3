"""CPU: the independent statement of the bigWig body (tests/writer_refs.py: Python's correctly rounded "%.4f", struct.pack,
sums in index order) against the NumPy statement the host path writes files with (`bigwig.piece_from_arrays`), on the edge
table of the text writer.  Pins the reference of the GPU tests of the device writers where no GPU is needed."""
import numpy as np

import writer_refs as wr
from test_oracle_writers import edge_values

STEP = 200


def _finite_edge_values():
    v = edge_values()
    return v[np.isfinite(v)]


def _same_bits_but_zero_sign(got, want):
    gf, wf = got.view(np.float32), want.view(np.float32)
    zero = (gf == 0) & (wf == 0)
    return bool(np.array_equal(got[~zero], want[~zero]))


def test_the_edge_table_still_holds_its_cases():
    """a later edit of the table cannot empty them silently: the finite values, and among them the exact half-way ties at the
    fourth decimal (|v| * 10^4 is exact in float64 for a float32 v)"""
    v = _finite_edge_values()
    assert len(edge_values()) - len(v) == 3 and len(v) >= 5026
    t = np.abs(v.astype(np.float64)) * 10000.0
    ties = v[(t - np.floor(t)) == 0.5]
    assert len(ties) >= 10
    # every tie goes to the even neighbour, in both signs
    items = wr.text4(ties)
    for x, got in zip(ties.tolist(), items.tolist()):
        r = np.floor(abs(x) * 10000.0)
        even = r if r % 2 == 0 else r + 1.0
        assert got == np.float32(np.copysign(even / 10000.0, x)), x
    assert np.any(ties > 0) and np.any(ties < 0)
    # the huge values (an integer number of 10^-4 already), the zeros of either sign and what rounds to them are in
    assert np.any(np.abs(v) >= 9.0e14) and np.any(v == np.float32(3.4e38)) and np.any(v == np.float32(-3.4028235e38))
    z = wr.text4(v)
    assert np.any((z == 0) & np.signbit(z) & (v != 0)) and np.any((z == 0) & ~np.signbit(z) & (v != 0))


def test_the_independent_statement_equals_the_numpy_statement_on_the_edge_table():
    from consenrich_amd import bigwig as bw

    assert wr.ITEMS_PER_SECTION == bw.ITEMS_PER_SECTION
    v = _finite_edge_values()
    n = len(v)
    starts, ends = wr.fixed_intervals(n, 10_000, STEP, end_cap=10_000 + n * STEP - 37)
    bins = [1, 10, n - 1, n, n + 1]
    with np.errstate(over="ignore"):
        host = bw.piece_from_arrays(3, starts, ends, v, zoom_bases=[g * STEP for g in bins], step=STEP)
    items = wr.text4(v)
    assert np.array_equal(items.view(np.uint32), bw.text4_values(v).view(np.uint32))
    assert host.sections == wr.sections(3, starts, ends, items)
    hdr = wr.section_headers(host.sections, n)
    assert len(hdr) == -(-n // 1024) and hdr[-1][7] == n - 1024 * (len(hdr) - 1) and hdr[-1][2] == ends[-1]
    s = wr.summary(starts, ends, items)
    assert host.bases_covered == s["bases_covered"] == n * STEP - 37
    assert host.min_val == s["min"] and host.max_val == s["max"]
    assert abs(host.sum_data - s["sum_data"]) <= 1e-12 * abs(s["sum_data"])
    assert abs(host.sum_squares - s["sum_squares"]) <= 1e-12 * abs(s["sum_squares"])
    for g in bins:
        got = wr.zoom_fields(host.zooms[g * STEP])
        want = wr.zoom_fields(wr.zoom_records(3, starts, ends, items, g))
        assert got.shape == want.shape == (-(-n // g), 8)
        # coordinates, counts, minimum and maximum: bit for bit at every level, but for the sign of a zero (NumPy's minimum /
        # maximum keep whichever zero they met last, and its sum of the single term -0.0 is -0.0 where a sum that starts
        # from 0.0 is +0.0)
        assert np.array_equal(got[:, :4], want[:, :4]), g
        assert _same_bits_but_zero_sign(got[:, 4:6], want[:, 4:6]), g
        if g <= 10:
            # the two sums: NumPy adds ten terms in another order than the index order; both are within half an ulp of float64
            # per step, far below the float32 they are stored in -- bit for bit here
            assert _same_bits_but_zero_sign(got[:, 6:], want[:, 6:]), g
        else:
            with np.errstate(invalid="ignore"):
                np.testing.assert_allclose(got[:, 6:].view(np.float32), want[:, 6:].view(np.float32), rtol=2e-7)
    assert wr.zoom_fields(wr.zoom_records(3, starts, ends, items, 10)).shape[0] >= 503
