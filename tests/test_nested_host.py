"""Nested ROCCO refinement without a GPU: the new symbols and struct layouts, every argument check with the reference's message
(they all come before a device is touched), and the per-region routines of csrc/csr_nested.h run on the CPU by a stand-alone
program built with the address and undefined-behaviour sanitizers, against the twin."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import nested_cases as NC  # noqa: E402
import twin_nested as T  # noqa: E402

from consenrich_amd import _lib as L  # noqa: E402
from consenrich_amd import nested as N  # noqa: E402

ROOT = os.path.dirname(HERE)


def test_symbols_and_struct_sizes():
    lib = L.lib()
    for name in ("csr_nested_solve", "csr_nested_nodes", "csr_nested_layer", "csr_nested_children", "csr_nested_selected_sum",
                 "csr_batch_nested_nodes", "csr_batch_nested_layer", "csr_batch_nested_selected_sum"):
        assert hasattr(lib, name) and name in L.SYMBOLS
    assert lib.csr_abi_version() == 6
    for dt, st, size in ((N.REGION, L.NestedRegion, 24), (N.CFG, L.NestedCfg, 32), (N.REC, L.NestedRec, 112), (N.NODE, L.NestedNode, 40)):
        assert dt.itemsize == C.sizeof(st) == size
        assert [(n, dt.fields[n][1]) for n in dt.names] == [(n, getattr(st, n).offset) for n, _ in st._fields_]
    with open(os.path.join(ROOT, "include", "consenrich_amd.h")) as fh:
        header = fh.read()
    assert f"#define CSR_NESTED_MAX_MIN_RUN {N.MAX_MIN_RUN}" in header
    with open(os.path.join(ROOT, "consenrich_amd", "csrc", "csr_nested.h")) as fh:
        kernel = fh.read()
    assert f"NESTED_WORD = {NC.TILE};" in kernel and f"NESTED_REG_STATES = {NC.WIDE_MIN_RUN - 1};" in kernel


@pytest.mark.parametrize("which", ["solve", "refine"])
def test_drop_in_argument_checks(which):
    good, errors = NC.solve_errors() if which == "solve" else NC.refine_errors()
    fn = N.solve_parent_conditioned_subpeaks if which == "solve" else N.refine_nested_rocco_solution
    twin = T.solve if which == "solve" else T.refine
    for override, message in errors:
        for f in (fn, twin):
            with pytest.raises(ValueError) as e:
                f(**{**good, **override})
            assert str(e.value) == message, (override, f)


def _call(name, *args):
    rc = getattr(L.lib(), name)(*args)
    return rc, L.last_error()


def test_library_argument_checks():
    """The library's own checks, called directly: CSR_ERR_VALUE and the reference's text, with no device in sight."""
    x = np.linspace(-1.0, 1.0, 12)
    costs = np.full(13, 0.1)
    mask, rec = np.zeros(12, np.uint8), np.zeros(1, N.REC)
    mp = mask.ctypes.data_as(C.POINTER(C.c_uint8))

    def solve(scores=x, n=12, c=costs, pen=0.2, m=3, req=4, rp=0.1):
        return _call("csr_nested_solve", L.dp(scores), n, L.dp(c), pen, m, req, rp, mp, N._vp(rec))

    bad = x.copy()
    bad[5] = np.nan
    neg = costs.copy()
    neg[12] = -1.0
    for got, message in (
            (solve(n=0), "`scores` must be a non-empty one-dimensional array"),
            (solve(scores=bad), "`scores` contains non-finite values"),
            (solve(c=neg), "`boundaryCosts` must be finite and non-negative"),
            (solve(pen=float("inf")), "`selectionPenalty` must be finite"),
            (solve(rp=-0.5), "`runPenalty` must be finite and non-negative"),
            (solve(rp=float("nan")), "`runPenalty` must be finite and non-negative"),
            (solve(req=12), "`requiredIndex` is outside `scores`"),
            (solve(req=-2), "`requiredIndex` is outside `scores`")):
        assert got == (L.ERR_VALUE, message)
    big = np.zeros(600)
    assert _call("csr_nested_solve", L.dp(big), 600, L.dp(np.zeros(601)), 0.0, 256, 0, 0.0,
                 np.zeros(600, np.uint8).ctypes.data_as(C.POINTER(C.c_uint8)), N._vp(rec)) == \
        (L.ERR_VALUE, "`minRunBins` 256 exceeds the supported maximum 255")

    lens = np.asarray([12], np.int64)
    sol = np.ones(12, np.uint8)
    region = np.asarray([(0, 11, 0, 5)], N.REGION)
    count = C.c_int64(0)

    def layer(scores=x, raw=None, gamma=1.0, pen=0.3, scale=0.75, rg=region, ln=lens):
        cfg = np.asarray([(gamma, pen, scale, 0, 0)], N.CFG)
        return _call("csr_nested_layer", 1, ln.ctypes.data_as(L.I64P), L.dp(scores), L.dp(raw), sol.ctypes.data_as(C.POINTER(C.c_uint8)),
                     N._vp(cfg), rg.size, N._vp(rg), N._vp(rec), C.byref(count))

    for got, message in (
            (layer(scores=bad), "`scores` contains non-finite values"),
            (layer(raw=bad), "`rawScores` contains non-finite values"),
            (layer(ln=np.asarray([0], np.int64)), "`scores` must be non-empty"),
            (layer(gamma=-1.0), "`gamma` must be finite and non-negative"),
            (layer(gamma=float("nan")), "`gamma` must be finite and non-negative"),
            (layer(pen=float("inf")), "`selectionPenalty` must be finite"),
            (layer(scale=float("nan")), "`nestedRoccoBudgetScale` must be finite")):
        assert got == (L.ERR_VALUE, message)
    # what is no ValueError of the reference's: a plain failure, also before any device
    rc, msg = layer(rg=np.asarray([(3, 12, 0, 5)], N.REGION))
    assert rc == -1 and "outside chain 0" in msg
    rc, msg = layer(rg=np.asarray([(0, 5, 0, 5), (5, 9, 0, 5)], N.REGION))
    assert rc == -1 and "disjoint and ascending" in msg
    rc, msg = layer(rg=np.asarray([(0, 5, 1, 5)], N.REGION))
    assert rc == -1 and "chain index out of range" in msg
    n_runs = np.asarray([2], np.int64)
    out = np.zeros(1)
    rc, msg = _call("csr_nested_selected_sum", 1, lens.ctypes.data_as(L.I64P), L.dp(x), n_runs.ctypes.data_as(L.I64P),
                    np.asarray([4, 2], np.int64).ctypes.data_as(L.I64P), np.asarray([5, 3], np.int64).ctypes.data_as(L.I64P), L.dp(out))
    assert rc == -1 and "ascending, disjoint" in msg


# ---------------------------------------------------------------------------------------------------------------
# the per-region routines on the CPU
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path_factory.mktemp("nested") / "nested_host_check")
    subprocess.check_call([hipcc, "-O1", "-g", "--offload-arch=gfx950", "-ffp-contract=off", "-std=c++17", "-Xarch_host",
                           "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(HERE, "native", "nested_host_check.hip")])
    return exe


def _run_layer(exe, tmp, scores, raw, sol, regions, gamma, base, scale, use_floor):
    src, dst = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(src, "wb") as fh:
        fh.write(np.asarray([scores.size, len(regions)], np.int64).tobytes())
        fh.write(np.asarray([gamma, base, scale], np.float64).tobytes())
        fh.write(np.asarray([int(use_floor)], np.int64).tobytes())
        fh.write(np.ascontiguousarray(scores, np.float64).tobytes())
        fh.write(np.ascontiguousarray(raw, np.float64).tobytes())
        fh.write(np.ascontiguousarray(sol, np.uint8).tobytes())
        fh.write(np.asarray(regions, np.int64).reshape(-1, 3).tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    subprocess.check_call([exe, src, dst], env=env)
    with open(dst, "rb") as fh:
        buf = fh.read()
    nr = len(regions)
    rec = np.frombuffer(buf, N.REC, nr)
    pos = nr * N.REC.itemsize
    nk = int(np.frombuffer(buf, np.int64, 1, pos)[0])
    kids = np.frombuffer(buf, N.NODE, nk, pos + 8)
    out = np.frombuffer(buf, np.uint8, scores.size, pos + 8 + nk * N.NODE.itemsize)
    return rec, kids, out


HOST_CASES = ["planted40", "scale0", "scale1", "min_run1", "min_run2", "dyadic", "dyadic_scale1", "all_negative", "tile_edges",
              "short_regions", "required_ends", "raw_scores", "ragged", "tiny_children"]


@pytest.mark.parametrize("name", HOST_CASES)
def test_regions_on_the_cpu_match_the_twin(host_check, tmp_path, name):
    """Layer 1 and layer 2 of a case, region by region, through the library's own per-region code on the CPU."""
    case = next(c for c in NC.REFINE if c["name"] == name)
    kw = NC.refine_inputs(case)
    scores = kw["scores"]
    raw = kw.get("rawScores", scores)
    mbins = kw["minRegionBins"]
    sol = kw["solution"].copy()
    for layer in (1, 2):
        _, want = T.refine(form="device", **{**kw, "nestedRoccoIters": layer, "jaccardThreshold": 2.0})
        if want["completed_iters"] < layer:
            break
        parents = [n for n in want["hierarchy"] if n["layer"] == layer - 1 and n["decision"] not in ("leaf", "skipped_short")]
        parents.sort(key=lambda n: n["start_idx"])
        regions = [(n["start_idx"], n["end_idx"], mbins) for n in parents]
        if not regions:
            break
        first = layer == 1
        rec, kids, sol = _run_layer(host_check, str(tmp_path), scores, raw, sol, regions, kw["gamma"],
                                    kw["selectionPenalty"] if first else 0.0, kw["nestedRoccoBudgetScale"] if first else 1.0, not first)
        by_id = {n["id"]: n for n in want["hierarchy"]}
        for r, n in zip(rec, parents):
            assert N.DECISIONS[int(r["decision"])] == n["decision"]
            assert int(r["required"]) == n["required_idx"] and int(r["n_runs"]) == n["candidate_child_count"]
            for field, key in (("floor", "local_score_floor"), ("selection_penalty", "selection_penalty"), ("objective", "objective"),
                               ("penalized", "penalized_objective"), ("boundary_penalty", "boundary_penalty"),
                               ("run_penalty_total", "run_penalty_total"), ("parent_penalized", "parent_penalized_objective"),
                               ("split_gain", "split_gain")):
                assert T.bits(r[field])[()] == T.bits(n[key])[()], (n["id"], key)
            runs = kids[int(r["child_base"]):int(r["child_base"]) + int(r["n_runs"])]
            assert [int(e - a + 1) for a, e in zip(runs["start"], runs["end"])] == n["child_widths_bins"]
            for nd, cid in zip(runs, n["child_ids"]):
                kid = by_id[cid]
                assert (int(nd["start"]), int(nd["end"]), int(nd["required"])) == (kid["start_idx"], kid["end_idx"], kid["required_idx"])
                assert T.bits(nd["raw_score_max"])[()] == T.bits(kid["raw_score_max"])[()]
                assert T.bits(nd["score_sum"])[()] == T.bits(kid["score_sum"])[()]
        mask, _ = T.refine(form="device", **{**kw, "nestedRoccoIters": layer, "jaccardThreshold": 2.0})
        assert np.array_equal(sol, mask)
