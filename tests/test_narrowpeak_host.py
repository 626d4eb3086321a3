"""narrowPeak export without a GPU: the new symbols and struct layouts, every argument check with the reference's message (they
all come before a device is touched), and the per-parent and per-child routines of csrc/csr_export.h run on the CPU by a
stand-alone program built with the address and undefined-behaviour sanitizers -- through the package's own host half
(coordinate gaps, assembly, the host decision), against the fixtures and the twin."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import narrowpeak_cases as NC  # noqa: E402
import twin_narrowpeak as T  # noqa: E402

from consenrich_amd import _lib as L  # noqa: E402
from consenrich_amd import narrowpeak as P  # noqa: E402

ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden", "narrowpeak", "narrowpeak_rows.npz")


def golden(name):
    with np.load(GOLD) as z:
        return {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(name + "/")}


def test_symbols_and_struct_sizes():
    lib = L.lib()
    for name in ("csr_export_peaks", "csr_batch_export_peaks", "csr_export_fetch"):
        assert hasattr(lib, name) and name in L.SYMBOLS
    assert lib.csr_abi_version() == 6
    for dt, st, size in ((P.CFG, L.ExportCfg, 48), (P.PARENT, L.ExportParent, 24), (P.PEAK, L.ExportPeak, 104)):
        assert dt.itemsize == C.sizeof(st) == size
        assert [(n, dt.fields[n][1]) for n in dt.names] == [(n, getattr(st, n).offset) for n, _ in st._fields_]
    with open(os.path.join(ROOT, "include", "consenrich_amd.h")) as fh:
        header = fh.read()
    assert f"#define CSR_NESTED_MAX_MIN_RUN {P.MAX_MIN_RUN}" in header
    for name, value in (("SPLIT_FROM_PARENT", L.EXPORT_SPLIT_FROM_PARENT), ("TRIMMED", L.EXPORT_TRIMMED),
                        ("HAS_LOCAL_P", L.EXPORT_HAS_LOCAL_P), ("DROPPED_MEDIAN", L.EXPORT_DROPPED_MEDIAN)):
        assert f"CSR_EXPORT_{name} = {value}" in header


def test_drop_in_argument_checks():
    """Both `ValueError`s of the reference's own body and those of the solver below it, each with the reference's text, from the
    drop-in and from the twin; and what the drop-in refuses because it is not built."""
    good, errors = NC.errors()
    for override, message in errors:
        for f in (P.solution_to_chrom_narrowpeak_rows, T.rows):
            with pytest.raises(ValueError) as e:
                f(**{**good, **override})
            assert str(e.value) == message, (override, f)
    with pytest.raises(ValueError, match="`massiveSubpeakWidthPolicy` is not supported"):
        P.solution_to_chrom_narrowpeak_rows(**{**good, "massiveSubpeakWidthPolicy": {"active": False}})
    with pytest.raises(ValueError, match="`nestedHierarchy` is not supported"):
        P.solution_to_chrom_narrowpeak_rows(**{**good, "nestedHierarchy": {"nodes": []}})
    with pytest.raises(ValueError, match="`nestedHierarchy` is not supported"):
        P.solution_to_chrom_narrowpeak_rows(**{**good, "nestedDetails": {"hierarchy": []}})
    with pytest.raises(ValueError, match="`minRunBins` 256 exceeds the supported maximum 255"):
        n = 600
        iv = np.arange(n, dtype=np.int64) * 25
        P.solution_to_chrom_narrowpeak_rows("c", iv, iv + 25, np.zeros(n), np.linspace(0, 1, n), np.ones(n, np.uint8), "p", 0.5,
                                            minSubpeakBins=256)
    with pytest.raises(ValueError, match="`segmentScores` and `segmentState` must match"):
        P.solve_parent_conditioned_subpeak_segments(np.zeros(4), np.zeros(5), 0, 3, 0.1, 0.1, 2)


def test_library_argument_checks():
    """The library's own checks, called directly: CSR_ERR_VALUE and the reference's text, with no device in sight."""
    n = 12
    x = np.linspace(-1.0, 1.0, n)
    lens = np.asarray([n], np.int64)
    count = C.c_int64(0)

    def call(scores=x, pen=0.2, cost=0.1, mult=2.0, min_run=3, split=1, parents=((2, 9),), ln=lens):
        cfg = np.asarray([(pen, cost, 0.0, mult, min_run, split, 1, 0)], P.CFG)
        par = np.asarray([(a, b, c[0] if c else 0, 0) for a, b, *c in parents], P.PARENT)
        rc = L.lib().csr_export_peaks(1, ln.ctypes.data_as(L.I64P), L.dp(x), L.dp(scores), None, P._vp(cfg), par.size, P._vp(par), None,
                                      C.byref(count))
        return rc, L.last_error()

    bad = x.copy()
    bad[5] = np.nan
    for got, message in (
            (call(scores=bad), "`scores` contains non-finite values"),
            (call(pen=float("inf")), "`selectionPenalty` must be finite"),
            (call(cost=float("nan")), "`boundaryCosts` must be finite and non-negative"),
            (call(mult=-0.5), "`exportFilterUncertaintyMultiplier` must be finite and non-negative"),
            (call(mult=float("nan")), "`exportFilterUncertaintyMultiplier` must be finite and non-negative")):
        assert got == (L.ERR_VALUE, message)
    big = np.asarray([600], np.int64)
    cfg = np.asarray([(0.0, 0.0, 0.0, 2.0, 256, 1, 1, 0)], P.CFG)
    par = np.asarray([(0, 599, 0, 0)], P.PARENT)
    z = np.zeros(600)
    assert (L.lib().csr_export_peaks(1, big.ctypes.data_as(L.I64P), L.dp(z), L.dp(z), None, P._vp(cfg), 1, P._vp(par), None, C.byref(count)),
            L.last_error()) == (L.ERR_VALUE, "`minRunBins` 256 exceeds the supported maximum 255")
    # what is no ValueError of the reference's: a plain failure, also before any device
    rc, msg = call(parents=((3, 12),))
    assert rc == -1 and "outside chain 0" in msg
    rc, msg = call(parents=((0, 5), (5, 9)))
    assert rc == -1 and "disjoint and ascending" in msg
    rc, msg = call(parents=((0, 5, 1),))
    assert rc == -1 and "chain index out of range" in msg


def test_cut_parents_counts_the_gaps_as_the_reference_does():
    iv, en = NC.coords(12, 10, gaps=(3, 7))
    ps, pe, cuts = P.cut_parents([1, 9], [7, 11], iv, en)
    assert (ps.tolist(), pe.tolist(), cuts) == ([1, 4, 9], [3, 7, 11], 1)       # the gap after bin 7 lies between two runs
    ps, pe, cuts = P.cut_parents([0], [11], iv, en)
    assert (ps.tolist(), pe.tolist(), cuts) == ([0, 4, 8], [3, 7, 11], 2)
    ps, pe, cuts = P.cut_parents([], [], iv, en)
    assert ps.size == 0 and cuts == 0


# ---------------------------------------------------------------------------------------------------------------
# the per-parent and per-child routines on the CPU
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    tmp = tmp_path_factory.mktemp("narrowpeak")
    exe = str(tmp / "narrowpeak_host_check")
    subprocess.check_call([hipcc, "-O1", "-g", "--offload-arch=gfx950", "-ffp-contract=off", "-std=c++17", "-Xarch_host",
                           "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(HERE, "native", "narrowpeak_host_check.hip")])
    return exe, str(tmp)


def _cpu_peaks(exe, tmp):
    """what stands in for consenrich_amd.narrowpeak._device_peaks: the same records, from the stand-alone program"""
    def run(state, scores, uncertainty, cfg_row, parents):
        cfg = np.asarray([cfg_row], P.CFG)[0]
        src, dst = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        n = int(scores.size)
        with open(src, "wb") as fh:
            fh.write(np.asarray([n, len(parents)], np.int64).tobytes())
            fh.write(np.asarray([cfg["selection_penalty"], cfg["boundary_cost"], cfg["trim_floor"], cfg["multiplier"]], np.float64).tobytes())
            fh.write(np.asarray([cfg["min_run"], cfg["split"], cfg["trim"], cfg["filter"], int(uncertainty is not None)], np.int64).tobytes())
            fh.write(np.ascontiguousarray(scores, np.float64).tobytes())
            fh.write(np.ascontiguousarray(state, np.float64).tobytes())
            fh.write(np.ascontiguousarray(np.zeros(n) if uncertainty is None else uncertainty, np.float64).tobytes())
            fh.write(np.asarray(parents, np.int64).reshape(-1, 2).tobytes())
        subprocess.check_call([exe, src, dst], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
        with open(dst, "rb") as fh:
            buf = fh.read()
        total = int(np.frombuffer(buf, np.int64, 1)[0])
        peaks = np.frombuffer(buf, P.PEAK, total, 8).copy()
        flags = np.frombuffer(buf, np.int32, len(parents), 8 + total * P.PEAK.itemsize).copy()
        return peaks, flags
    return run


HOST_CASES = [c["name"] for c in NC.CASES if c["name"] != "min_run_wide"]      # (the states-as-lanes kernel has no host form)


@pytest.mark.parametrize("name", HOST_CASES)
def test_export_on_the_cpu_matches_the_reference(host_check, monkeypatch, name):
    """The drop-in with the library's per-parent and per-child code run on the CPU in place of the device call."""
    monkeypatch.setattr(P, "_device_peaks", _cpu_peaks(*host_check))
    before = dict(P.STATS)
    kw = NC.inputs(NC.case(name))
    got = P.solution_to_chrom_narrowpeak_rows(**kw)
    with np.errstate(invalid="ignore"):
        want = T.rows(form="steps", **kw)
    assert type(got) is tuple and len(got) == len(want)
    assert T.differences(got, want) == []
    if len(got) == 3:
        assert T.same_flat(T.flatten(got), golden(name)) == []
    # the cap on host decisions: the NaN chain and no other
    assert P.STATS["decided_on_host"] - before["decided_on_host"] == int(name in NC.HOST_DECIDED)


def test_pieces_on_the_cpu_match_the_twin(host_check, monkeypatch):
    monkeypatch.setattr(P, "_device_peaks", _cpu_peaks(*host_check))
    for name in ("splits", "ties", "lengths_min5"):
        kw = NC.inputs(NC.case(name))
        for a, b in T.TN.run_bounds(kw["solution"] > 0):
            args = (kw["scores"][a:b + 1], kw["state"][a:b + 1], a, b, kw["subpeakSelectionPenalty"], kw["subpeakBoundaryCost"], 5)
            got, want = P.solve_parent_conditioned_subpeak_segments(*args), T.segments(*args)
            assert T.TN.differences(got, want) == [] and [list(g) for g in got] == [list(w) for w in want], (name, a)
    kw = NC.inputs(NC.case("trims"))
    s = kw["scores"]
    for a, b in T.TN.run_bounds(kw["solution"] > 0):
        for k in range(a - 1, b + 2):
            for floor in (0.0, 0.5, None, float("inf"), -9.0):
                assert P.trim_child_segment_around_summit(a, b, k, s, floor) == T.trim(a, b, k, s, floor), (a, k, floor)
