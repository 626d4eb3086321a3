"""GPU tests of the writers of resident tracks at their edges (run with -m gpu): every component of every exported array of a
levelTrend fit, planted float32 values (the edge table of the text writer, tests/test_oracle_writers.edge_values) around the
1024-row scan block of k_bgw_* and the 1024 items of a bigWig section, and coordinates at the 32-bit limit of the bigWig format.
References: the reference's own pandas call for the bedGraph text (oracle/writers.py), tests/writer_refs.py for the bigWig body
(Python's correctly rounded "%.4f", struct.pack, sums in index order; pinned on the CPU by tests/test_writer_refs.py).  Text
is compared byte for byte, records bit for bit."""
import numpy as np
import pytest

import cases
import writer_refs as wr
from conftest import gpu_available
from test_oracle_writers import edge_values

pytestmark = pytest.mark.gpu

STEP = 200
HEAD = 29                               # the literal head of the edge table (NaN, +-inf, ties, huge values, zeros of both signs)
PLANT_LENS = [1, 1023, 1024, 1025, 2049]


@pytest.fixture(scope="module")
def product():
    if not gpu_available():
        pytest.fail("GPU tests selected but no HIP device / library: the product has no CPU fallback")
    from consenrich_amd import cconsenrich

    return cconsenrich


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _column(raw, comp):
    return np.ascontiguousarray(raw.reshape(raw.shape[0], -1)[:, comp])


# ---------------------------------------------------------------------------------------------------------------------------
# every component of a levelTrend fit
# ---------------------------------------------------------------------------------------------------------------------------
COMPONENTS = [("xs", 0, None), ("xs", 1, None), ("Ps", 0, "sqrt"), ("Ps", 1, None), ("Ps", 2, None), ("Ps", 3, "sqrt"),
              ("xf", 1, None), ("Pf", 3, None)]


@pytest.fixture(scope="module")
def trend_fit(product):
    from consenrich_amd import _lib as L
    from consenrich_amd.batch import DeviceBatch, ModelParams

    n_list, m = [1, 1025, 2049], 3
    b = DeviceBatch(0)
    b.configure(ModelParams(state_dim=2), m, n_list)
    for c, n in enumerate(n_list):
        b.upload(c, *cases.synth(n, m, 5200 + c, mask_frac=0.02, outlier_frac=0.01))
    b.stats()
    b.forward_backward(L.RETURN_NLL)
    b.export(L.EXPORT_FORWARD | L.EXPORT_SMOOTH)
    yield b, n_list
    b.close()


@pytest.mark.parametrize("name,comp,transform", COMPONENTS, ids=[f"{a}{c}-{t}" for a, c, t in COMPONENTS])
def test_every_component_of_a_trend_fit_is_written_from_its_own_column(trend_fit, name, comp, transform):
    b, n_list = trend_fit
    for c, n in enumerate(n_list):
        raw = b.download(c, name)
        assert raw.reshape(n, -1).shape[1] == {"xs": 2, "xf": 2, "Ps": 4, "Pf": 4}[name]
        col = _column(raw, comp)
        if n > 1:   # the column is not another component's: a writer that ignored `comp` would print another track
            assert all(not np.array_equal(col, _column(raw, k)) for k in range(raw.reshape(n, -1).shape[1])
                       if k != comp and not (name in ("Ps", "Pf") and {k, comp} == {1, 2}))
        wr.check_resident_track(b, c, name, comp, transform, col, c + 1, 1000, STEP, 1000 + n * STEP - 13, (name, comp, c))


def test_a_component_past_the_last_is_refused(trend_fit):
    from consenrich_amd import _lib as L

    b, n_list = trend_fit
    for name, per in (("xs", 2), ("xf", 2), ("Ps", 4), ("Pf", 4)):
        for comp in (per, -1):
            with pytest.raises(L.ConsenrichAMDError, match="component out of range"):
                b.bedgraph_bytes(1, name, "chr1", 0, STEP, comp=comp)
            with pytest.raises(L.ConsenrichAMDError, match="component out of range"):
                b.bigwig_track(1, name, 0, 0, STEP, comp=comp)


# ---------------------------------------------------------------------------------------------------------------------------
# planted values
# ---------------------------------------------------------------------------------------------------------------------------
def _planted_values(finite_only):
    """One float32 track per chain of PLANT_LENS from the edge table, cycled to length: the literal head first (whole in every
    chain of 1023 or more bins), then the rest of the table from where the previous chain stopped, so that the batch as a whole
    holds every value of the table."""
    v = edge_values()
    head, rest = v[:HEAD], v[HEAD:]
    if finite_only:
        head, rest = head[np.isfinite(head)], rest[np.isfinite(rest)]
    out, pos = [], 0
    for n in PLANT_LENS:
        take = max(n - len(head), 0)
        idx = (pos + np.arange(take)) % len(rest)
        pos += take
        out.append(np.concatenate([head, rest[idx]])[:n].astype(np.float32))
    assert pos >= len(rest)
    return out


@pytest.fixture(scope="module")
def planted(product):
    """a batch whose "kappa" array takes planted values: (batch, plant) with plant(finite_only) -> the values per chain"""
    from consenrich_amd import _lib as L
    from consenrich_amd.batch import DeviceBatch, ModelParams

    m = 2
    b = DeviceBatch(0)
    b.configure(ModelParams(state_dim=2), m, PLANT_LENS)
    for c, n in enumerate(PLANT_LENS):
        b.upload(c, *cases.synth(n, m, 5300 + c))

    def plant(finite_only):
        vals = _planted_values(finite_only)
        for c, v in enumerate(vals):
            b.upload_multipliers(c, kappa=v)
        b.export(L.EXPORT_MULT)
        for c, v in enumerate(vals):      # the route carries the bits (NaN, the infinities, -0.0, subnormals) unchanged
            assert np.array_equal(_bits(b.download(c, "kappa")), _bits(v)), c
        return vals

    yield b, plant
    b.close()


def test_planted_tracks_hold_the_table():
    for finite_only in (False, True):
        vals = _planted_values(finite_only)
        table = edge_values()
        table = table[np.isfinite(table)] if finite_only else table
        assert [len(v) for v in vals] == PLANT_LENS
        assert set(_bits(np.concatenate(vals)).tolist()) == set(_bits(table).tolist())
        for v in vals[1:]:
            assert np.array_equal(_bits(v[:HEAD - 3 * finite_only]), _bits(table[:HEAD - 3 * finite_only]))
    assert np.isnan(edge_values()[:HEAD]).sum() == 1 and np.isinf(edge_values()[:HEAD]).sum() == 2


@pytest.mark.parametrize("transform", [None, "round4", "sqrt"])
def test_bedgraph_text_of_planted_edge_values(planted, transform):
    """every value of the edge table, at row counts 1, 1023, 1024, 1025 and 2049 (the 1024-row scan block from both sides, and a
    third block of one row); "sqrt" of a negative value is NaN and prints empty like the NaN of the table"""
    from oracle import writers as ow

    b, plant = planted
    vals = plant(False)
    for c, v in enumerate(vals):
        n = len(v)
        for end_cap in (0, 10_000 + n * STEP - 37):
            starts, ends = wr.fixed_intervals(n, 10_000, STEP, end_cap)
            with np.errstate(all="ignore"):
                ref = ow.bedgraph_bytes("chr7", starts, ends, v, transform)
            got = b.bedgraph_bytes(c, "kappa", "chr7", 10_000, STEP, end_cap=end_cap, transform=transform)
            if got != ref:
                g, r = got.split(b"\n"), ref.split(b"\n")
                bad = [k for k in range(min(len(g), len(r))) if g[k] != r[k]]
                pytest.fail(f"chain {c} transform {transform}: rows {bad[:5]}: {[(g[k], r[k]) for k in bad[:5]]}")
    if transform == "sqrt":
        assert b"\t\n" in ref and np.any(vals[-1] < 0)


def test_bigwig_body_of_planted_finite_edge_values(planted):
    """items, every section header (the last, partial one with its item count and end), total summary and the zoom records of
    1, 10, n - 1, n and n + 1 bins per record"""
    from consenrich_amd import _lib as L

    b, plant = planted
    vals = plant(True)
    for c, v in enumerate(vals):
        n = len(v)
        for end_cap in (0, 10_000 + n * STEP - 37):
            starts, ends = wr.fixed_intervals(n, 10_000, STEP, end_cap)
            bins = wr.zoom_bins(n)
            piece = b.bigwig_track(c, "kappa", 5, 10_000, STEP, end_cap=end_cap, zoom_bases=[g * STEP for g in bins])
            wr.check_piece(piece, 5, starts, ends, v, bins, STEP, (c, end_cap))
            hdr = wr.section_headers(piece.sections, n)
            assert len(hdr) == -(-n // 1024) and hdr[-1][7] == n - 1024 * (len(hdr) - 1) and hdr[-1][2] == ends[-1]
    with pytest.raises(L.ConsenrichAMDError, match="bins_per_record must be positive"):
        b.bigwig_track(0, "kappa", 5, 10_000, STEP, zoom_bases=[0])         # n - 1 of the one-bin chain


def test_a_planted_non_finite_value_is_refused_by_the_bigwig_writer(planted):
    from consenrich_amd import _lib as L

    b, plant = planted
    vals = plant(False)
    assert np.all(np.isfinite(vals[0])) and not np.all(np.isfinite(vals[1]))
    b.bigwig_track(0, "kappa", 0, 0, STEP)
    for c in range(1, len(vals)):
        with pytest.raises(ValueError, match="Non-finite"):
            b.bigwig_track(c, "kappa", 0, 0, STEP)
    for bad in (np.nan, np.inf, -np.inf):                                       # one value alone, in the last row of the last section
        v = np.ones(PLANT_LENS[3], np.float32)
        v[-1] = bad
        b.upload_multipliers(3, kappa=v)
        b.export(L.EXPORT_MULT)
        with pytest.raises(ValueError, match=r"Non-finite bedGraph value in chain 3 \(1 intervals\)"):
            b.bigwig_track(3, "kappa", 0, 0, STEP)


# ---------------------------------------------------------------------------------------------------------------------------
# coordinates at the edges of the format
# ---------------------------------------------------------------------------------------------------------------------------
def test_coordinates_up_to_the_last_32_bit_base(planted):
    """1025 intervals that cross 2^31 inside the second and end exactly at 2^32 - 1, the largest end a bigWig item can hold"""
    from consenrich_amd import _lib as L
    from oracle import writers as ow

    b, plant = planted
    vals = plant(True)
    c, n, step = 3, PLANT_LENS[3], 1 << 21
    last = (1 << 32) - 1
    start0 = last - n * step
    assert 0 <= start0 < (1 << 31) < start0 + 2 * step and ((1 << 31) - start0) % step and start0 + n * step == last
    for s0, end_cap in ((start0, 0), (start0 + 5, last)):        # the second: a last interval clipped at the limit
        starts, ends = wr.fixed_intervals(n, s0, step, end_cap)
        assert ends[-1] == last and ends[-1] > starts[-1]
        bins = wr.zoom_bins(n)
        piece = b.bigwig_track(c, "kappa", 7, s0, step, end_cap=end_cap, zoom_bases=[g * step for g in bins])
        wr.check_piece(piece, 7, starts, ends, vals[c], bins, step, (s0, end_cap))
        assert b.bedgraph_bytes(c, "kappa", "chr7", s0, step, end_cap=end_cap) == ow.bedgraph_bytes("chr7", starts, ends, vals[c])
    for s0 in (start0 + 1, start0 + step):
        with pytest.raises(L.ConsenrichAMDError, match="bigWig coordinates are 32-bit"):
            b.bigwig_track(c, "kappa", 7, s0, step)
        with pytest.raises(L.ConsenrichAMDError, match="bigWig coordinates are 32-bit"):
            b.bigwig_track(c, "kappa", 7, s0, step, zoom_bases=[10 * step], end_cap=last + 1)
    for end_cap in (start0 + (n - 1) * step, start0 + (n - 1) * step - 1):
        with pytest.raises(L.ConsenrichAMDError, match="end_cap leaves an empty last interval"):
            b.bigwig_track(c, "kappa", 7, start0, step, end_cap=end_cap)
    b.bigwig_track(c, "kappa", 7, start0, step, end_cap=start0 + (n - 1) * step + 1)        # one base is an interval
