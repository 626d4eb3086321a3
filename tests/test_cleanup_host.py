"""The massive sub-peak clean-up without a GPU: the new symbol and struct layouts (NumPy dtype = ctypes = header), every argument
check of the library (they all come before a device is touched), and the recursion, the merge network, the scans and the packing of
csrc/csr_cleanup.h run on the CPU by a stand-alone program built with the address and undefined-behaviour sanitizers -- through
the package's own drop-ins, over the whole case table, against the fixtures."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cleanup_cases as CC  # noqa: E402
import cleanup_compare as CMP  # noqa: E402
import twin_cleanup as T  # noqa: E402

from consenrich_amd import _lib as L  # noqa: E402
from consenrich_amd import cleanup as K  # noqa: E402
from consenrich_amd import narrowpeak as P  # noqa: E402

ROOT = os.path.dirname(HERE)


def test_symbols_struct_layouts_and_constants():
    lib = L.lib()
    for name in ("csr_cleanup_plan", "csr_batch_cleanup_plan"):
        assert hasattr(lib, name) and name in L.SYMBOLS
    assert lib.csr_abi_version() == 6
    # the export structs keep their sizes
    for dt, st, size in ((P.CFG, L.ExportCfg, 48), (P.PARENT, L.ExportParent, 24), (P.PEAK, L.ExportPeak, 104)):
        assert dt.itemsize == C.sizeof(st) == size
    with open(os.path.join(ROOT, "include", "consenrich_amd.h")) as fh:
        header = fh.read()
    for dt, st, size, name in ((K.POLICY, L.CleanupPolicy, 48, "csr_cleanup_policy"), (K.CHILD, L.CleanupChild, 16, "csr_cleanup_child"),
                               (K.SEGMENT, L.CleanupSegment, 64, "csr_cleanup_segment"), (K.COUNTS, L.CleanupCounts, 32, "csr_cleanup_counts"),
                               (K.NODE, L.CleanupNode, 88, "csr_cleanup_node"),
                               (K.BATCH_CHILD, L.CleanupBatchChild, 32, "csr_cleanup_batch_child")):
        assert dt.itemsize == C.sizeof(st) == size
        assert [(n, dt.fields[n][1]) for n in dt.names] == [(n, getattr(st, n).offset) for n, _ in st._fields_]
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = [f.strip() for decl in body.split(";") for f in re.sub(r"^\s*(double|int64_t|int32_t)", "", decl.strip()).split(",") if f.strip()]
        assert fields == list(dt.names), name
    for name, value in (("MAX_SEGMENTS", K.MAX_SEGMENTS), ("MAX_DEPTH", K.MAX_DEPTH_SUPPORTED), ("SORT_TILE", K.SORT_TILE)):
        assert f"#define CSR_CLEANUP_{name} {value}" in header
    assert K.SORT_TILE == T.SORT_TILE == CC.SORT_TILE and K.MAX_SEGMENTS == T.MAX_SEGMENTS
    with open(os.path.join(ROOT, "consenrich_amd", "csrc", "csr_cleanup.h")) as fh:
        assert f"#define CLEANUP_SORT_TILE {K.SORT_TILE} " in fh.read()
    assert "CSR_CLEANUP_MODE_NONE = 0, CSR_CLEANUP_MODE_UNSPLIT = 1, CSR_CLEANUP_MODE_SPLIT = 2, CSR_CLEANUP_MODE_ADAPTIVE_CORE = 3" in header
    assert L.CLEANUP_MODES == T.MODES
    for name, value in (("CANDIDATE", L.CLEANUP_CANDIDATE), ("APPLIED", L.CLEANUP_APPLIED), ("HAS_SPLIT", L.CLEANUP_HAS_SPLIT),
                        ("HAS_CORE_WIDTH", L.CLEANUP_HAS_CORE_WIDTH), ("HAS_CORE_FLOOR", L.CLEANUP_HAS_CORE_FLOOR),
                        ("MOVED", L.CLEANUP_MOVED), ("SPLIT_FROM_PARENT", L.CLEANUP_SPLIT_FROM_PARENT)):
        assert f"CSR_CLEANUP_{name} = {value}" in header


def test_the_row_drop_in_still_refuses_a_policy():
    n = 40
    iv = np.arange(n, dtype=np.int64) * 25
    with pytest.raises(ValueError, match="the massive sub-peak clean-up is not built"):
        P.solution_to_chrom_narrowpeak_rows("c", iv, iv + 25, np.zeros(n), np.linspace(0, 1, n), np.ones(n, np.uint8), "p", 0.5,
                                            massiveSubpeakWidthPolicy={"active": False})


def test_library_argument_checks():
    """The library's own checks, called directly: CSR_ERR_VALUE and the reference's text where it has one, no device in sight."""
    n = 40
    x = np.linspace(-1.0, 1.0, n)
    edges = np.arange(n + 1, dtype=np.int64) * 100

    def call(op=L.CLEANUP_OP_FORCE, scores=x, e=edges, step=0, kids=((0, n - 1),), thr=2000.0, ct=1500.0, q=0.25, z=2.0, cost=0.5, depth=8,
             capacity=None):
        pol = np.asarray([(thr, ct, q, z, cost, 1, depth)], K.POLICY)
        ch = np.asarray(list(kids), K.CHILD)
        seg = np.zeros(K.MAX_SEGMENTS * max(len(kids), 1) if capacity is None else capacity, K.SEGMENT)
        cnt, nodes, total = np.zeros(len(kids), K.COUNTS), np.zeros(len(kids), K.NODE), C.c_int64(-1)
        rc = L.lib().csr_cleanup_plan(op, scores.size, L.dp(scores), None if e is None else e.ctypes.data_as(L.I64P), 0, step, ch.size,
                                      K._vp(ch), K._vp(pol), seg.size, K._vp(seg), C.byref(total), K._vp(cnt), K._vp(nodes))
        return rc, L.last_error()

    bad = x.copy()
    bad[5] = np.inf
    for got, message in (
            (call(scores=bad), "`scores` contains non-finite values"),
            (call(op=L.CLEANUP_OP_SPLIT, scores=bad), "`scores` contains non-finite values"),
            (call(op=L.CLEANUP_OP_CONTRACT, scores=bad), "`scores` contains non-finite values"),
            (call(depth=K.MAX_DEPTH_SUPPORTED + 1), f"`maxDepth` {K.MAX_DEPTH_SUPPORTED + 1} exceeds the supported maximum {K.MAX_DEPTH_SUPPORTED}"),
            (call(q=float("nan")), "`splitQuantile` must be finite"),
            (call(z=float("inf")), "`minSplitZ` must be finite"),
            (call(cost=float("nan")), "`boundaryCost` must be finite")):
        assert got == (L.ERR_VALUE, message)
    # what is no ValueError of the reference's: a plain failure, also before any device
    for got, text in ((call(op=7), "unknown clean-up operation"), (call(kids=((3, n),)), "outside the scores"),
                      (call(kids=((0, 9), (9, 20))), "disjoint and ascending"), (call(e=None, step=-25), "negative step"),
                      (call(e=edges[::-1].copy()), "must not decrease")):
        assert got[0] == -1 and text in got[1], got
    # the drop-in hands the library's ValueError on
    with pytest.raises(ValueError, match="`maxDepth` 33 exceeds the supported maximum 32"):
        K.force_massive_subpeak_segments(maxDepth=33, **{k: v for k, v in CC.force_inputs(CC.FORCE[0])[0].items() if k != "maxDepth"})


def test_drop_in_checks_that_need_no_device():
    kw = CC.force_inputs(CC.FORCE[0])[0]
    child = dict(kw["child"])
    got = K.force_massive_subpeak_segments(**{**kw, "widthPolicy": None})
    assert got == ([child], {k: 0 for k in K.COUNTERS}) and got[0][0] is not kw["child"]
    assert K.force_massive_subpeak_segments(**{**kw, "widthPolicy": {"width_threshold_bp": None}})[0] == [child]
    assert K.best_massive_subpeak_split(np.zeros(11), 0.5, 4) is None
    assert K.contract_massive_subpeak_segment(5, 200, kw["scores"], kw["intervals"], kw["ends"], 1500, 3) is None
    assert K.contract_massive_subpeak_segment(0, 79, kw["scores"], kw["intervals"], kw["ends"], float("inf"), 3) is None
    with pytest.raises(ValueError, match="`scores` contains non-finite values"):
        K.force_massive_subpeak_segments(**CC.nonfinite_inputs())
    gap_ends = kw["ends"].copy()
    gap_ends[10] += 5
    with pytest.raises(ValueError, match="coordinate gap"):
        K.force_massive_subpeak_segments(**{**kw, "ends": gap_ends})
    assert K.contract_threshold({"contract_width_bp": 5000}, 2000.0) == 2000.0
    assert K.contract_threshold({"min_bp": 1200}, 2000.0) == 1200.0
    assert K.contract_threshold({}, 9000.0) == 7500.0
    assert K.contract_threshold({"contract_width_bp": -1.0}, 9000.0) == 7500.0


# ---------------------------------------------------------------------------------------------------------------
# the recursion on the CPU
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    tmp = tmp_path_factory.mktemp("cleanup")
    exe = str(tmp / "cleanup_host_check")
    subprocess.check_call([hipcc, "-O1", "-g", "--offload-arch=gfx950", "-ffp-contract=off", "-std=c++17", "-Xarch_host",
                           "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(HERE, "native", "cleanup_host_check.hip")])
    return exe, str(tmp)


def _cpu_plan(exe, tmp):
    """what stands in for consenrich_amd.cleanup.plan: the same records, from the stand-alone program"""
    def run(op, scores, edges, origin, step, children, policy_row):
        s = np.ascontiguousarray(scores, np.float64)
        kids = np.ascontiguousarray(children, K.CHILD)
        src, dst = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        with open(src, "wb") as fh:
            fh.write(np.asarray([op, s.size, kids.size, int(edges is not None), origin, step], np.int64).tobytes())
            fh.write(np.asarray([policy_row], K.POLICY).tobytes())
            fh.write(s.tobytes())
            if edges is not None:
                fh.write(np.ascontiguousarray(edges, np.int64).tobytes())
            fh.write(kids.tobytes())
        subprocess.check_call([exe, src, dst], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
        with open(dst, "rb") as fh:
            buf = fh.read()
        if op != L.CLEANUP_OP_FORCE:
            return np.frombuffer(buf, K.NODE, kids.size).copy()
        total = int(np.frombuffer(buf, np.int64, 1)[0])
        return (np.frombuffer(buf, K.SEGMENT, total, 8).copy(),
                np.frombuffer(buf, K.COUNTS, kids.size, 8 + total * K.SEGMENT.itemsize).copy())
    return run


@pytest.mark.parametrize("coords", ["auto", "edges"])
@pytest.mark.parametrize("name", CMP.force_ids())
def test_force_on_the_cpu_matches_the_reference(host_check, monkeypatch, name, coords):
    """The drop-in with the library's recursion run on the CPU in place of the device call; equally wide bins travel as a step
    ("auto") or as edges, with identical records."""
    monkeypatch.setattr(K, "plan", _cpu_plan(*host_check))
    monkeypatch.setattr(K, "COORDS", coords)
    CMP.check_force(K.force_massive_subpeak_segments, name)


def test_pieces_on_the_cpu_match_the_reference(host_check, monkeypatch):
    monkeypatch.setattr(K, "plan", _cpu_plan(*host_check))
    for coords in ("auto", "edges"):
        monkeypatch.setattr(K, "COORDS", coords)
        CMP.check_splits(K.best_massive_subpeak_split)
        CMP.check_contracts(K.contract_massive_subpeak_segment)


def test_several_children_in_one_call_on_the_cpu(host_check):
    """One call, three children (the first in bin 0, the last ending in bin n - 1, the middle one no candidate): the packed records
    are those of three calls, in order, with the exclusive prefix sum of the counts as their bases."""
    plan = _cpu_plan(*host_check)
    case = next(c for c in CC.FORCE if c["name"] == "ends")
    iv, en = CC.coords(case["widths"])
    edges = np.concatenate((iv, en[-1:]))
    row = (1500.0, 1000.0, 0.25, 2.0, case["cost"], 1, 8)
    seg, cnt = plan(L.CLEANUP_OP_FORCE, case["scores"], edges, 0, 0, case["children"], row)
    assert cnt["n_segments"].sum() == seg.size and seg["child"].tolist() == np.repeat(np.arange(3), cnt["n_segments"]).tolist()
    at = 0
    for k, (a, b) in enumerate(case["children"]):
        one, c1 = plan(L.CLEANUP_OP_FORCE, case["scores"], edges, 0, 0, [(a, b)], row)
        mine = seg[at:at + one.size].copy()
        mine["child"] = 0
        assert mine.tobytes() == one.tobytes() and cnt[k].tobytes() == c1[0].tobytes()
        at += one.size
    assert int(cnt["candidates"][1]) == 0 and int(cnt["n_segments"][1]) == 1


# ---------------------------------------------------------------------------------------------------------------
# the rows under a policy on the CPU: all three device calls replaced by their stand-alone programs
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def export_check(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    tmp = tmp_path_factory.mktemp("cleanup_rows")
    exe = str(tmp / "narrowpeak_host_check")
    subprocess.check_call([hipcc, "-O1", "-g", "--offload-arch=gfx950", "-ffp-contract=off", "-std=c++17", "-Xarch_host",
                           "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(HERE, "native", "narrowpeak_host_check.hip")])
    return exe, str(tmp)


@pytest.mark.parametrize("name", CMP.row_ids())
def test_rows_under_a_policy_on_the_cpu_match_the_reference(host_check, export_check, monkeypatch, name):
    from test_narrowpeak_host import _cpu_peaks

    monkeypatch.setattr(K, "plan", _cpu_plan(*host_check))
    monkeypatch.setattr(P, "_device_peaks", _cpu_peaks(*export_check))
    before = dict(P.STATS)
    rows, meta, details = CMP.check_rows(K.solution_to_chrom_narrowpeak_rows, name)
    assert P.STATS["decided_on_host"] == before["decided_on_host"]
    assert details["massive_subpeak_width_policy"] is not next(c for c in CC.ROWS if c["name"] == name)["massiveSubpeakWidthPolicy"]
    modes = {m["massive_subpeak_cleanup_mode"] for m in meta}
    if name == "rows_active":
        assert {"adaptive_core", "width_capped_core"} <= modes and details["num_massive_subpeak_contracts"] > 0
    if name == "rows_no_split":     # (without the dynamic programme the forced splits have the plateaus to themselves)
        assert details["num_massive_subpeak_splits"] > 0 and any(m["massive_subpeak_split_gain"] is not None for m in meta)
    if name in ("rows_inactive_policy", "rows_cleanup_off"):
        assert modes == {None} and all(type(m["massive_subpeak_width_p"]) is float for m in meta)
        assert all(m["massive_subpeak_width_threshold_bp"] == 2000 for m in meta) and not details["massive_subpeak_cleanup_active"]


def test_rows_without_a_policy_are_the_existing_drop_ins(host_check, export_check, monkeypatch):
    from test_narrowpeak_host import _cpu_peaks

    monkeypatch.setattr(P, "_device_peaks", _cpu_peaks(*export_check))
    kw = {**CC.row_inputs(CC.ROWS[0]), "massiveSubpeakWidthPolicy": None}
    assert T.differences(K.solution_to_chrom_narrowpeak_rows(**kw), P.solution_to_chrom_narrowpeak_rows(**kw)) == []
    with pytest.raises(ValueError, match="`nestedHierarchy` is not supported"):
        K.solution_to_chrom_narrowpeak_rows(**{**CC.row_inputs(CC.ROWS[0]), "nestedHierarchy": {"nodes": []}})
