"""TEST INFRASTRUCTURE ONLY -- an independent statement of the fixed-record body of a bigWig track (data sections, total summary,
zoom records), for the tests of the device writers (csrc/csr_writers.h: k_bw_sections, k_bw_zoom).

Nothing here is taken from `consenrich_amd.bigwig`: that module's `text4_values` is the kernel's own formula written again.
  * item values: Python's correctly rounded decimal formatting and parsing, np.float32(float("%.4f" % v)) -- what a reader of the
    reference's bedGraph text hands to pyBigWig (io.py:707);
  * section headers and items: `struct.pack` with the field list of the bbi format tables (Kent et al. 2010, supplement);
  * zoom records: plain loops that add in index order in float64, one rounding per operation (v * w, then v * v, then * w), the
    result rounded once to float32;
  * total summary: `math.fsum` (exactly rounded sums) of the same terms.
Minimum and maximum order the signed zeros (-0.0 < +0.0, IEEE 754-2019 `minimum` / `maximum`), so that they do not depend on
the order in which a record's values are visited.
tests/test_writer_refs.py pins this statement against `bigwig.piece_from_arrays` on the edge table where no GPU is needed.
"""
import math
import struct

import numpy as np

ITEMS_PER_SECTION = 1024
SECTION_HEADER = "<IIIIIBBH"    # chromId, chromStart, chromEnd, itemStep, itemSpan, type (1 = bedGraph), reserved, itemCount
SECTION_ITEM = "<IIf"           # chromStart, chromEnd, value
ZOOM_RECORD = "<IIIIffff"       # chromId, chromStart, chromEnd, validCount, minVal, maxVal, sumData, sumSquares


def text4(values) -> np.ndarray:
    """float32 of the decimal text "%.4f" % v of every (finite) float32 value"""
    v = np.asarray(values, np.float32)
    return np.asarray([np.float32(float("%.4f" % float(x))) for x in v.tolist()], np.float32)


def fixed_intervals(n: int, start0: int, step: int, end_cap: int = 0):
    """(starts, ends) as Python ints: interval k = [start0 + k step, start0 + (k + 1) step), the end clipped at end_cap > 0"""
    starts = [int(start0) + k * int(step) for k in range(n)]
    ends = [s + int(step) for s in starts]
    if end_cap > 0:
        ends = [min(e, int(end_cap)) for e in ends]
    return starts, ends


def _min(a: float, b: float) -> float:
    if a == b:
        return a if math.copysign(1.0, a) < 0.0 else b
    return a if a < b else b


def _max(a: float, b: float) -> float:
    if a == b:
        return b if math.copysign(1.0, a) < 0.0 else a
    return a if a > b else b


def _f32(x: float) -> float:
    with np.errstate(over="ignore"):
        return float(np.float32(x))        # one rounding to nearest-even; beyond the float32 range: +-inf


def sections(chrom_id: int, starts, ends, items) -> bytes:
    """the data sections back to back: ITEMS_PER_SECTION items each, the last one shorter"""
    n, out = len(items), bytearray()
    for a in range(0, n, ITEMS_PER_SECTION):
        b = min(n, a + ITEMS_PER_SECTION)
        out += struct.pack(SECTION_HEADER, chrom_id, starts[a], ends[b - 1], 0, 0, 1, 0, b - a)
        for k in range(a, b):
            out += struct.pack(SECTION_ITEM, starts[k], ends[k], float(items[k]))
    return bytes(out)


def section_headers(body: bytes, n: int):
    """[(chromId, start, end, itemStep, itemSpan, type, reserved, itemCount)] of a body of n items"""
    out, pos = [], 0
    for a in range(0, n, ITEMS_PER_SECTION):
        out.append(struct.unpack_from(SECTION_HEADER, body, pos))
        pos += 24 + 12 * (min(n, a + ITEMS_PER_SECTION) - a)
    assert pos == len(body)
    return out


def section_items(body: bytes, n: int):
    """[(start, end, value bits)] of a body of n items"""
    out, pos = [], 0
    for a in range(0, n, ITEMS_PER_SECTION):
        pos += 24
        for _ in range(a, min(n, a + ITEMS_PER_SECTION)):
            out.append(struct.unpack_from("<III", body, pos))
            pos += 12
    return out


def summary(starts, ends, items) -> dict:
    v = [float(x) for x in items]
    w = [float(e - s) for s, e in zip(starts, ends)]
    mn, mx = math.inf, -math.inf
    for x in v:
        mn, mx = _min(mn, x), _max(mx, x)
    return {"bases_covered": sum(e - s for s, e in zip(starts, ends)), "min": mn, "max": mx,
            "sum_data": math.fsum(x * y for x, y in zip(v, w)), "sum_squares": math.fsum(x * x * y for x, y in zip(v, w))}


def zoom_records(chrom_id: int, starts, ends, items, bins_per_record: int) -> bytes:
    n, g, out = len(items), int(bins_per_record), bytearray()
    for k0 in range(0, n, g):
        k1 = min(n, k0 + g)
        mn, mx, sm, sq, valid = math.inf, -math.inf, 0.0, 0.0, 0
        for k in range(k0, k1):
            dv, w = float(items[k]), float(ends[k] - starts[k])
            valid += ends[k] - starts[k]
            mn, mx = _min(mn, dv), _max(mx, dv)
            sm += dv * w
            sq += dv * dv * w
        out += struct.pack("<IIII", chrom_id, starts[k0], ends[k1 - 1], valid)
        out += np.asarray([_f32(mn), _f32(mx), _f32(sm), _f32(sq)], "<f4").tobytes()
    return bytes(out)


def zoom_fields(raw: bytes):
    """the eight fields of every record as unsigned 32-bit patterns, shape (records, 8)"""
    return np.frombuffer(raw, "<u4").reshape(-1, 8)


def zoom_bins(n: int):
    """bins per zoom record: 1, 10, and n - 1, n, n + 1 (a last record of one bin, one record, a record longer than the chain)"""
    return sorted({g for g in (1, 10, n - 1, n, n + 1) if g >= 1})


def check_resident_track(batch, chain, name, comp, transform, values, chrom_id, start0, step, end_cap, tag=""):
    """bedGraph text (against the reference's pandas call, oracle/writers.py) and bigWig body (against this module) of component
    `comp` of a resident array of one chain; `values` is that column of the download"""
    from oracle import writers as ow

    n = len(values)
    starts, ends = fixed_intervals(n, start0, step, end_cap)
    chrom = "chr%d" % chrom_id
    got = batch.bedgraph_bytes(chain, name, chrom, start0, step, end_cap=end_cap, comp=comp, transform=transform)
    assert got == ow.bedgraph_bytes(chrom, starts, ends, values, transform), tag
    bins = zoom_bins(n)
    piece = batch.bigwig_track(chain, name, chrom_id, start0, step, end_cap=end_cap, comp=comp, transform=transform,
                               zoom_bases=[g * step for g in bins])
    check_piece(piece, chrom_id, starts, ends, ow.transform_values(values, transform), bins, step, tag)


def check_piece(piece, chrom_id: int, starts, ends, values, zoom_bins, step: int, tag=""):
    """Every record of a `bigwig.TrackPiece` against this module: items, section headers and zoom records bit for bit, bases /
    min / max equal, the two sums of the total summary to 1e-12 relative (the device adds them as a tree of partial sums; the
    tolerance is the one tests/test_bigwig.py holds them to).  `values` are the float32 track values after the transform."""
    import pytest

    items = text4(values)
    n = len(items)
    assert piece.chrom_id == chrom_id and piece.n_items == n, tag
    ref = sections(chrom_id, starts, ends, items)
    assert len(piece.sections) == len(ref), tag
    assert section_headers(piece.sections, n) == section_headers(ref, n), tag
    got_items, ref_items = section_items(piece.sections, n), section_items(ref, n)
    bad = [k for k in range(n) if got_items[k] != ref_items[k]]
    assert not bad, (tag, bad[:5], [(got_items[k], ref_items[k], float(values[k])) for k in bad[:5]])
    assert piece.sections == ref, tag
    s = summary(starts, ends, items)
    assert piece.bases_covered == s["bases_covered"] and piece.min_val == s["min"] and piece.max_val == s["max"], tag
    assert piece.sum_data == pytest.approx(s["sum_data"], rel=1e-12), tag
    assert piece.sum_squares == pytest.approx(s["sum_squares"], rel=1e-12), tag
    assert sorted(piece.zooms) == sorted(g * step for g in set(zoom_bins)), tag
    for g in zoom_bins:
        got, want = zoom_fields(piece.zooms[g * step]), zoom_fields(zoom_records(chrom_id, starts, ends, items, g))
        assert got.shape == want.shape == (-(-n // g), 8), (tag, g)
        rows = np.nonzero(np.any(got != want, axis=1))[0]
        assert rows.size == 0, (tag, g, rows[:5], got[rows[:5]], want[rows[:5]])
