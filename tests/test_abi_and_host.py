"""CPU: the C-ABI library loads and exports every symbol the header declares (no compute without a GPU), the product
fails loudly when it cannot run, the host-side mirror raises the reference's errors before any launch, and the
sharding logic is right."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    from consenrich_amd import build

    build.build()
    from consenrich_amd import _lib

    _lib.lib()
    return _lib


def _header_symbols():
    text = open(os.path.join(ROOT, "include", "consenrich_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(csr_[a-z_0-9]+)\s*\(", text)))


def test_library_exports_every_declared_symbol(L):
    import ctypes

    handle = ctypes.CDLL(L.LIB_PATH)
    declared = _header_symbols()
    assert len(declared) >= 25
    for name in declared:
        assert hasattr(handle, name), f"{name} declared in include/consenrich_amd.h but not exported"
    assert set(declared) == set(L.SYMBOLS), "ctypes binding and header disagree"
    assert L.lib().csr_abi_version() == 6


def test_struct_layouts_match_header(L):
    import ctypes as C

    assert C.sizeof(L.Model) == 8 + 8 * (4 + 4 + 3 + 4 + 5)
    assert C.sizeof(L.FwdIO) == 8 * 2 + 8 * 5 + 8 + 8 * 4
    assert C.sizeof(L.EcmCfg) == 8 * 4 + 4 * 4
    assert C.sizeof(L.EcmOut) == 8 * 7 + 4 * 4
    assert C.sizeof(L.RunStats) == 8 * 5 + 4 * 6 + 8 + 4 * 2 + 8 + 8 + 8


def _has_gpu(L):
    return L.device_count() > 0


def test_product_fails_loudly_without_gpu(L):
    if _has_gpu(L):
        pytest.skip("a GPU is present")
    from consenrich_amd import cconsenrich
    from consenrich_amd.batch import DeviceBatch

    assert L.lib().csr_create(0) is None and "no HIP device" in L.last_error()
    with pytest.raises(L.ConsenrichAMDError):
        DeviceBatch(0)
    n, m = 16, 2
    with pytest.raises(L.ConsenrichAMDError):
        cconsenrich.cforwardPass(matrixData=np.zeros((m, n), np.float32), matrixPluginMuncInit=np.ones((m, n), np.float32),
                                 matrixF=np.eye(2, dtype=np.float32), matrixQ0=np.eye(2, dtype=np.float32),
                                 intervalToBlockMap=np.zeros(n, np.int32), blockCount=1, stateInit=0.0,
                                 stateCovarInit=1.0)


def test_product_sources_never_touch_the_oracle():
    pkg = os.path.join(ROOT, "consenrich_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                text = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle", text, flags=re.M), f
                assert "libconsenrich_oracle" not in text, f


def _kw(n=12, m=2):
    return dict(matrixData=np.zeros((m, n), np.float32), matrixPluginMuncInit=np.full((m, n), 0.2, np.float32),
                matrixF=np.asarray([[1, 1], [0, 1]], np.float32), matrixQ0=np.diag([1e-3, 1e-4]).astype(np.float32),
                intervalToBlockMap=np.zeros(n, np.int32), blockCount=1, stateInit=0.0, stateCovarInit=1.0)


def test_reference_error_contract_is_enforced_before_any_launch(L):
    """Messages of pyx:6503-6561, 6624, 125-130, 143-151; all raised on the host, so they work without a GPU."""
    from consenrich_amd import cconsenrich as cc

    kw = _kw()
    with pytest.raises(ValueError, match="blockCount must be positive"):
        cc.cforwardPass(**{**kw, "blockCount": 0})
    with pytest.raises(ValueError, match="must match matrixData shape"):
        cc.cforwardPass(**{**kw, "matrixPluginMuncInit": np.ones((2, 5), np.float32)})
    with pytest.raises(ValueError, match="at least shape"):
        cc.cforwardPass(**{**kw, "matrixF": np.ones((1, 2), np.float32)})
    with pytest.raises(ValueError, match="observation precision multiplier bounds"):
        cc.cforwardPass(**kw, obsPrecisionMultiplierMin=0.0)
    with pytest.raises(ValueError, match="process precision multiplier bounds"):
        cc.cforwardPass(**kw, procPrecisionMultiplierMin=2.0, procPrecisionMultiplierMax=1.0)
    with pytest.raises(ValueError, match="intervalToBlockMap length"):
        cc.cforwardPass(**{**kw, "intervalToBlockMap": np.zeros(3, np.int32)})
    with pytest.raises(ValueError, match="out-of-range block id"):
        cc.cforwardPass(**{**kw, "intervalToBlockMap": np.full(12, 4, np.int32)})
    with pytest.raises(ValueError, match="lambdaExp length"):
        cc.cforwardPass(**kw, lambdaExp=np.ones(3, np.float32))
    with pytest.raises(ValueError, match="wrong number of dimensions"):
        cc.cforwardPass(**kw, lambdaExp=np.ones((2, 12), np.float32))
    with pytest.raises(ValueError, match="processQScale\\[0\\] must be 1.0"):
        cc.cforwardPass(**kw, processQScale=np.full(12, 2.0, np.float32))
    with pytest.raises(ValueError, match="positive finite"):
        cc.cforwardPass(**kw, processQScale=np.asarray([1.0] + [-1.0] * 11, np.float32))
    with pytest.raises(ValueError, match="vectorD length"):
        cc.cforwardPass(**kw, vectorD=np.empty(3, np.float32))
    with pytest.raises(ValueError, match="stateForward shape"):
        cc.cforwardPass(**kw, stateForward=np.empty((3, 2), np.float32), stateCovarForward=np.empty((12, 2, 2), np.float32),
                        pNoiseForward=np.empty((12, 2, 2), np.float32))
    with pytest.raises(ValueError, match="dtype mismatch"):
        cc.cforwardPass(**{**kw, "matrixData": np.zeros((2, 12), np.float64)})
    with pytest.raises(ValueError, match="not C-contiguous"):
        cc.cforwardPass(**{**kw, "matrixData": np.zeros((12, 2), np.float32).T})
    # caller-provided outputs are written in place by the device-to-host copy: a read-only buffer is refused up front (the
    # Cython original fails in its writable buffer acquisition; a copy into a read-only mapping would be a segfault)
    ro = np.empty(12, np.float32)
    ro.setflags(write=False)
    with pytest.raises(ValueError, match="read-only"):
        cc.cforwardPass(**kw, vectorD=ro)
    ro2 = np.empty((12, 2), np.float32)
    ro2.setflags(write=False)
    with pytest.raises(ValueError, match="read-only"):
        cc.cbackwardPass(matrixData=kw["matrixData"], matrixF=kw["matrixF"], stateForward=np.zeros((12, 2), np.float32),
                         stateCovarForward=np.zeros((12, 2, 2), np.float32), pNoiseForward=np.zeros((12, 2, 2), np.float32),
                         stateSmoothed=ro2)
    lv = {k: v for k, v in kw.items() if k != "matrixF"}
    with pytest.raises(ValueError, match=r"matrixQ0\[0, 0\] must be positive"):
        cc.cforwardPassLevel(**{**lv, "matrixQ0": np.zeros((1, 1), np.float32)})
    with pytest.raises(ValueError, match="matrixQ0 is singular"):
        cc.cfixedBackgroundECM(**{**kw, "matrixQ0": np.ones((2, 2), np.float32)}, logIterations=False)
    with pytest.raises(ValueError, match="lambdaExpInit length"):
        cc.cfixedBackgroundECM(**kw, lambdaExpInit=np.ones(3, np.float32), logIterations=False)
    with pytest.raises(ValueError, match="only finite values"):
        cc.cfixedBackgroundECM(**kw, processPrecExpInit=np.full(12, np.nan, np.float32), logIterations=False)
    with pytest.raises(ValueError, match=r"stateSmoothed must have shape \(n, 2\)"):
        cc.cExpectedTransitionResidualSums(np.zeros((4, 1)), np.zeros((4, 2, 2)), np.zeros((3, 2, 2)), np.eye(2))
    with pytest.raises(ValueError, match="lagCovSmoothed must have shape"):
        cc.cExpectedTransitionResidualSums(np.zeros((4, 2)), np.zeros((4, 2, 2)), np.zeros((1, 2, 2)), np.eye(2))


def test_empty_and_degenerate_inputs_follow_the_reference(L):
    from consenrich_amd import cconsenrich as cc

    kw = _kw(n=0)
    r = cc.cforwardPass(**kw, returnNLL=True)
    assert r[0] == 0.0 and r[1] == 0 and r[2].shape == (0,) and r[3] == 0.0
    assert cc.cExpectedTransitionResidualSums(np.zeros((1, 2)), np.zeros((1, 2, 2)), np.zeros((0, 2, 2)), np.eye(2)) == (0.0, 0.0, 0)
    assert cc.cExpectedTransitionResidualSumsLevel(np.zeros((1, 1)), np.zeros((1, 1, 1)), np.zeros((0, 1, 1))) == (0.0, 0.0, 0)
    out = cc.cfixedBackgroundECM(**kw, returnIntermediates=True, returnDiagnostics=True, logIterations=False)
    assert out[0] == 0 and out[1] == 0.0 and out[8]["skipped"] is True and out[8]["skip_reason"] == "empty_input"
    xs, Ps, lag, res = cc.cbackwardPass(matrixData=np.empty((2, 0), np.float32), matrixF=kw["matrixF"],
                                        stateForward=np.empty((0, 2), np.float32),
                                        stateCovarForward=np.empty((0, 2, 2), np.float32),
                                        pNoiseForward=np.empty((0, 2, 2), np.float32))
    assert xs.shape == (0, 2) and Ps.shape == (0, 2, 2) and lag.shape == (1, 2, 2) and res.shape == (0, 2)


def test_convergence_replay_matches_reference_bookkeeping():
    from consenrich_amd.cconsenrich import _replay_path

    rec = _replay_path("t", [100.0, 90.0, 89.99999, 89.99998, 89.9], 1e-6, False)
    assert [r["stable_iters"] for r in rec] == [0, 0, 1, 2, 0]
    assert rec[0]["reset_iteration"] and rec[0]["change"] is None
    assert rec[3]["converged"] and not rec[4]["converged"]
    assert rec[1]["relative_improvement"] == pytest.approx(10.0 / 100.0)


def test_lpt_sharding_of_hg38():
    from consenrich_amd.sharding import hg38_chain_lengths, lpt_assign, shard_bound

    lens = hg38_chain_lengths(200)
    assert len(lens) == 22 and sum(lens) == 14375018 and lens[0] == 1244783
    for w in (1, 2, 4, 8):
        owned = lpt_assign(lens, w)
        assert sorted(i for v in owned for i in v) == list(range(22))
    assert shard_bound(lens, 8) == pytest.approx(7.67, abs=0.01)
    assert shard_bound(lens, 4) == pytest.approx(3.89, abs=0.02)
    assert shard_bound(lens, 2) == pytest.approx(2.0, abs=0.01)
    assert sum(hg38_chain_lengths(50)) == 57500042


def test_header_is_plain_c_and_library_links_from_c(tmp_path):
    """The boundary is a C ABI: compile a strict-C99 translation unit against include/consenrich_amd.h, link it with the
    shared library, run it (no GPU needed) and compare the struct sizes it prints with the ctypes mirrors."""
    import shutil
    import subprocess

    from consenrich_amd import _lib as L

    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    L.lib()                                                        # builds the library if necessary
    exe = tmp_path / "abi_check"
    libdir = os.path.dirname(L.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "abi_check.c"), "-o", str(exe), "-L", libdir, "-lconsenrich_amd",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    fields = r.stdout.split()
    assert int(fields[1]) == L.lib().csr_abi_version()
    sizes = [int(v) for v in fields[5:11]]
    assert sizes == [C.sizeof(L.Model), C.sizeof(L.EcmCfg), C.sizeof(L.EcmOut), C.sizeof(L.BgCfg), C.sizeof(L.BgOut),
                     C.sizeof(L.RunStats)]


def test_step_groups_header_hands_out_chains_as_the_pipelined_step_expects(tmp_path):
    """consenrich_amd/csrc/csr_step_groups.h is plain C++17: tests/step_groups_check.cpp (runs of chains, their span of
    wavefront-groups, the thresholds / cap / remainder / bail-out of ChainSet, its scripted pick and what a script may hold) built
    stand-alone under the address and undefined-behaviour sanitizers."""
    import shutil
    import subprocess

    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "step_groups_check"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "consenrich_amd", "csrc"), os.path.join(ROOT, "tests", "step_groups_check.cpp"),
                           "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "step_groups_check ok" in r.stdout, (r.returncode, r.stdout, r.stderr)


def test_resid_form_header_bounds_the_lds_request_for_every_sample_count(tmp_path):
    """consenrich_amd/csrc/csr_resid_form.h is plain C++17: tests/resid_form_check.cpp (every m in 1 .. 65535: LDS request within
    64 KB, slabs of sample rows that tile [0, m) exactly, multiples of 4 in the 16-byte form; the one-slab forms at m = 4, 124,
    125, 128, 240, 251 as a literal table; 244, 252, 253, 256, 604, 631 bounded) built stand-alone under the address and
    undefined-behaviour sanitizers."""
    import shutil
    import subprocess

    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "resid_form_check"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "consenrich_amd", "csrc"), os.path.join(ROOT, "tests", "resid_form_check.cpp"),
                           "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "resid_form_check ok" in r.stdout, (r.returncode, r.stdout, r.stderr)


def test_chain_tracks_header_selects_chains_as_the_peak_stages_expect(tmp_path):
    """consenrich_amd/csrc/csr_chain_tracks.h is plain C++17: tests/chain_tracks_check.cpp (presence flags of a per-chain track,
    the chains a mask takes and the first of them without the track, the scatter of compact results) built stand-alone under
    the address and undefined-behaviour sanitizers."""
    import shutil
    import subprocess

    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "chain_tracks_check"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "consenrich_amd", "csrc"), os.path.join(ROOT, "tests", "chain_tracks_check.cpp"),
                           "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "chain_tracks_check ok" in r.stdout, (r.returncode, r.stdout, r.stderr)


NP_ORDER_LENS = [0, 1, 7, 8, 9, 15, 16, 17, 127, 128, 129, 135, 136, 137, 255, 256, 257, 8191, 8192, 8193, 16384, 16385, 24706]
NP_ORDER_FUNCTOR_LENS = [129, 8193, 16385]


def test_np_order_header_sums_keys_and_selects_as_numpy_does(tmp_path):
    """consenrich_amd/csrc/csr_np_order.h is __host__ __device__: tests/native/np_order_host_check.hip runs it on the CPU under the
    address and undefined-behaviour sanitizers.  np_sum_f against np.sum bit for bit at every length where the pairwise tree
    changes shape (leaf, split, chunk fold), with the identity, a shift and the excess-and-count element; the tree walked twice
    (leaves recorded, then leaf sums) against np_chunk_sum_f; the ordered keys and their inverse; the two serial steps of the
    radix select on hand-made histograms."""
    import shutil
    import subprocess

    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "np_order_host_check")
    subprocess.check_call([hipcc, "-O1", "-g", "--offload-arch=gfx950", "-ffp-contract=off", "-std=c++17", "-Xarch_host",
                           "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "native", "np_order_host_check.hip")])
    rng = np.random.default_rng(20261020)
    n = max(NP_ORDER_LENS)
    x = rng.standard_normal(n) * 10.0 ** rng.integers(-8, 8, n)
    c, off, s = 0.37, -0.25, 1.75

    def key_values(dtype, decades):
        fi = np.finfo(dtype)
        edges = [-np.inf, -fi.max, -1.0, -fi.smallest_subnormal, -0.0, 0.0, fi.smallest_subnormal, 1.0, fi.max, np.inf]
        return np.asarray(edges + list(rng.standard_normal(1000) * 10.0 ** rng.integers(-decades, decades, 1000)), dtype)

    kd, kf = key_values(np.float64, 300), key_values(np.float32, 30)

    def hist(counts):
        h = np.zeros(256, np.uint32)
        for digit, cnt in counts.items():
            h[digit] = cnt
        return h

    # (histogram, rank) -> (digit, count of the digits below it)
    picks = [(hist({3: 5, 9: 2}), 0, (3, 0)),                   # the rank at the first count
             (hist({3: 5, 9: 2}), 6, (9, 5)),                   # ... at the last
             (hist({3: 5, 9: 2}), 4, (3, 0)),                   # on the boundary between two digits: the last of digit 3
             (hist({3: 5, 9: 2}), 5, (9, 5)),                   # ... the first of digit 9
             (hist({0: 1, 1: 1, 2: 1}), 1, (1, 1)),
             (hist({255: 7}), 6, (255, 0)),                     # all mass in digit 255
             (hist({255: 7}), 0, (255, 0)),
             (hist({0: 4, 255: 4}), 4, (255, 4))]
    # (ranks, prefixes) -> the first target with the same prefix, -1 for an unused target
    groups = [([0, 5, 9], [0, 0, 0], [0, 0, 0]),
              ([0, 5, 9], [1, 2, 1], [0, 1, 0]),
              ([-1, 5, 9, 2], [7, 7, 7, 8], [-1, 1, 1, 3]),
              ([4, -1, 4, 4, 6, 6], [3, 3, 5, 3, 5, 9], [0, -1, 2, 0, 2, 5]),
              ([-1, -1], [0, 0], [-1, -1])]
    src = tmp_path / "np_order.bin"
    with open(src, "wb") as fh:
        for arr in (x, np.asarray(NP_ORDER_LENS, np.int64), np.asarray(NP_ORDER_FUNCTOR_LENS, np.int64)):
            fh.write(np.asarray([arr.size], np.int64).tobytes() + arr.tobytes())
        fh.write(np.asarray([c, off, s], np.float64).tobytes())
        for arr in (kd, kf):
            fh.write(np.asarray([arr.size], np.int64).tobytes() + arr.tobytes())
        fh.write(np.asarray([len(picks)], np.int64).tobytes())
        for h, rank, _ in picks:
            fh.write(h.tobytes() + np.asarray([rank], np.int64).tobytes())
        fh.write(np.asarray([len(groups)], np.int64).tobytes())
        for rank, prefix, _ in groups:
            fh.write(np.asarray([len(rank)], np.int64).tobytes() + np.asarray(rank, np.int64).tobytes()
                     + np.asarray(prefix, np.uint64).tobytes())
    r = subprocess.run([exe, str(src)], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    out = {}
    for line in r.stdout.splitlines():
        out.setdefault(line.split()[0], []).append(line.split()[1:])

    def b64(v):
        return int(np.asarray([v], np.float64).view(np.uint64)[0])

    assert [(int(a), int(b, 16)) for a, b in out["sum"]] == [(k, b64(np.sum(x[:k]))) for k in NP_ORDER_LENS]
    capped = [min(k, 8192) for k in NP_ORDER_LENS]
    assert [(int(a), int(b, 16), int(d, 16)) for a, b, d in out["tree"]] == [(k, b64(np.sum(x[:k])), b64(np.sum(x[:k]))) for k in capped]
    assert [(int(a), int(b, 16)) for a, b in out["shift"]] == [(k, b64(np.sum(x[:k] - c))) for k in NP_ORDER_FUNCTOR_LENS]
    assert [(int(a), int(b, 16), int(d)) for a, b, d in out["excess"]] == \
        [(k, b64(np.sum(np.clip((x[:k] - off) / s, 0, None))), int((x[:k] > off).sum())) for k in NP_ORDER_FUNCTOR_LENS]
    # sums of -0.0 alone.  Below 8 values the leaf starts from 0.0 and the sum is +0.0, as np.sum gives.  From 8 values on the
    # eight accumulators start from the values themselves and the tree keeps -0.0, where np.sum (2.2.6) answers +0.0: the one
    # known difference from NumPy, a zero's sign, in every stage since the first of them; pinned here as it is
    zeros = [(int(a), int(b, 16)) for a, b in out["zeros"]]
    assert zeros[:8] == [(k, b64(np.sum(np.full(k, -0.0)))) for k in range(8)] and all(b == 0 for _, b in zeros[:8])
    assert zeros[8:] == [(k, b64(-0.0)) for k in (8, 9, 130)]
    for name, vals, uint in (("keyd", kd, np.uint64), ("keyf", kf, np.uint32)):
        keys = np.asarray([int(a, 16) for a, _ in out[name]], uint)
        back = np.asarray([int(b, 16) for _, b in out[name]], uint)
        assert np.array_equal(back, vals.view(uint)), name                       # np_unkey(np_key(v)) is v bit for bit
        assert np.array_equal(vals[np.argsort(keys, kind="stable")], np.sort(vals)), name
        assert keys[4] < keys[5] and vals[4] == 0 and np.signbit(vals[4]) and not np.signbit(vals[5]), name     # -0.0 before +0.0
        assert np.unique(keys).size == np.unique(vals.view(uint)).size, name
    assert [(int(a), int(b)) for a, b in out["pick"]] == [want for _, _, want in picks]
    assert [[int(g) for g in row] for row in out["groups"]] == [want for _, _, want in groups]


def test_qseed_posterior_fails_loudly_without_a_gpu():
    """The grid posterior of the Q0 seed (pyx:1905-2146) runs on the device since round 2 (csr_qseed_post.h; its golden
    vectors are checked under -m gpu, tests/test_gpu_qseed.py): without a GPU the call must raise, not compute on the host."""
    import numpy as np
    import pytest

    import qseed_cases as qc
    from conftest import gpu_available
    from consenrich_amd import _lib as L
    from consenrich_amd import qseed

    if gpu_available():
        pytest.skip("a GPU is visible: the device path is covered by tests/test_gpu_qseed.py")
    case = next(c for c in qc.native_cases() if c["kind"] == "post")
    with pytest.raises(L.ConsenrichAMDError, match="no CPU fallback"):
        qc.run_native(qseed, case)


def test_qseed_mirror_argument_validation_without_a_gpu():
    """the Python-level validation of the Q0-seed natives (pyx:1532-1546, 1977-1996) happens before any device call"""
    import math

    import numpy as np
    import pytest

    from consenrich_amd import cconsenrich as amd

    data, act = np.zeros((2, 9)), np.ones((2, 9), bool)
    with pytest.raises(ValueError, match="signalPanelSize must be nonnegative"):
        amd.cEstimateSameTrackProcessNoiseTransitions(data, np.ones((2, 9)), act, 0.95, 20.0, 0, 32000, -1)
    with pytest.raises(ValueError, match=r"precisionCapQuantile must be in \[0, 1\]"):
        amd.cEstimateSameTrackProcessNoiseTransitions(data, np.ones((2, 9)), act, 1.5, 20.0)
    with pytest.raises(ValueError, match="precisionCapMultiplier must be positive"):
        amd.cEstimateSameTrackProcessNoiseTransitions(data, np.ones((2, 9)), act, 0.95, 0.0)
    with pytest.raises(ValueError, match="obsVar shape must match matrixData"):
        amd.cEstimateSameTrackProcessNoiseTransitions(data, np.ones((2, 8)), act, 0.95, 20.0)
    with pytest.raises(ValueError, match="matrixData must be a 2D array"):
        amd.cEstimatePooledProcessNoiseTransitions(np.zeros(9), np.ones(9), np.ones(9, bool))
    empty = amd.cEstimateSameTrackProcessNoiseTransitions(np.zeros((2, 1)), np.ones((2, 1)), np.ones((2, 1), bool), 0.95, 20.0)
    assert empty[0].size == 0 and math.isnan(empty[3]["precisionCap"])
    assert all(a.size == 0 for a in amd.cEstimatePooledProcessNoiseTransitions(np.zeros((2, 1)), np.ones((2, 1)), np.ones((2, 1), bool)))
    one = np.ones(8)
    tail = (1.0e-5, 8, math.log(4.0), 8.0, 64)
    for kwargs, msg in (((one, one[:3], one, 1e-5, 1.0, 8.0, "s") + tail, "same length"),
                        ((one, one, one, 0.0, 1.0, 8.0, "s") + tail, "qFloor must be positive finite"),
                        ((one, one, one, 1e-5, -1.0, 8.0, "s") + tail, "qCap must be positive or infinite"),
                        ((one, one, one, 1e-5, 1.0, 8.0, "s", 1e-5, 0, math.log(4.0), 8.0, 64), "minTransitions must be positive"),
                        ((one, one, one, 1e-5, 1.0, 8.0, "s", 1e-5, 8, math.log(4.0), 8.0, 0), "gridSize must be positive")):
        with pytest.raises(ValueError, match=msg):
            amd.cQSeedPosteriorFromTransitions(*kwargs)
    # (the data-dependent checks -- "samplingVariances must be nonnegative finite", ... -- are made by the device kernels:
    # tests/test_gpu_qseed.py)


def test_bench_fails_loudly_without_a_gpu():
    """No silent CPU path behind the benchmark either: without a device bench.py ends with the library's error."""
    import subprocess
    import sys

    from conftest import gpu_available

    if gpu_available():
        pytest.skip("a GPU is visible")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "1", "--warmup", "0", "--no-cpu-baseline",
                        "--no-extras"], capture_output=True, text=True, timeout=300, cwd=root)
    assert r.returncode != 0 and r.stdout.strip() == ""
    assert "no CPU fallback" in r.stderr or "no HIP device" in r.stderr, r.stderr[-1500:]



def test_bench_line_helpers_read_the_committed_records():
    """`throughput_mode.parity` of a bench line comes from the committed full-size parity record of that config (which arrays the
    2-ulp mode holds to 1e-5 on the workload, which it does not); `expected` at N > 1 from the model fitted to the emulated shards."""
    import importlib
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    bench = importlib.import_module("bench")
    for cfg in ("c2", "c3", "c4", "c5"):
        rec = bench.throughput_mode_parity(cfg)
        assert rec is not None and rec["source"].startswith("profiles/r0") and rec["source"].endswith("_ulp2.json"), cfg
        assert all(v <= 1e-5 for v in rec["holds_1e-5"].values()) and "level (xs, xf)" in rec["holds_1e-5"], (cfg, rec)
        nis = rec["outside_1e-5"]["NIS"]
        if cfg != "c3":                 # (the c3 test records the two output tracks only)
            assert 0.0 < nis["fraction_of_bins"] < 0.1, (cfg, rec)       # NIS is the array the mode does not hold
    assert bench.throughput_mode_parity("no such config") is None
    from consenrich_amd.sharding import hg38_chain_lengths, lpt_assign

    lengths = hg38_chain_lengths(200)
    bins = [sum(lengths[i] for i in part) for part in lpt_assign(lengths, 8)]
    exp = bench.expected_speedup(bins, sum(lengths))
    assert 1.5 < exp["default"]["speedup_vs_1gpu"] < 3.0 and 4.5 < exp["ulp2"]["speedup_vs_1gpu"] < 7.67, exp
    assert os.path.isfile(os.path.join(root, bench.TRAFFIC_FILES[0])) and os.path.isfile(os.path.join(root, bench.TRAFFIC_FILES[2]))


def test_bench_dump_is_a_fixed_sample_of_the_returned_arrays(tmp_path):
    """`bench.py --dump-outputs`: the rows written are the returned arrays' own rows at a seeded sample of bins (transitions for
    pNoise / lagCov), the same sample for the same batch, float32 / float64 only, within the 64 MB budget."""
    import importlib
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    bench = importlib.import_module("bench")

    class Batch:                # what dump_outputs reads of a DeviceBatch: d, m, download(chain, name)
        d, m = 2, 32
        lens = [700000, 1, 2, 300000, 5]

        def download(self, chain, name):
            n = self.lens[chain]
            rows = n - 1 if name in ("pnoise", "lag") else n
            shape = {"D": (), "xf": (2,), "xs": (2,), "resid": (self.m,)}.get(name, (2, 2))
            base = np.arange(rows, dtype=np.float64).reshape((rows,) + (1,) * len(shape))
            return np.broadcast_to(base + 1e6 * chain, (rows, *shape)).astype(np.float32)

    b = Batch()
    sums = (np.arange(5) * 1.5, np.arange(5) * -2.0)
    names = bench.dump_outputs(b, b.lens, False, sums, str(tmp_path / "a"))
    assert set(names) == {"D", "xf", "Pf", "pnoise", "xs", "Ps", "lag", "resid", "sumD", "sumNLL"}
    bench.dump_outputs(b, b.lens, False, sums, str(tmp_path / "b"))
    total = 0
    for n in names:
        a, c = np.load(tmp_path / "a" / f"{n}.npy"), np.load(tmp_path / "b" / f"{n}.npy")
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, c), n
        total += os.path.getsize(tmp_path / "a" / f"{n}.npy")
    assert total <= 64 * 2**20
    resid = np.load(tmp_path / "a" / "resid.npy")
    assert resid.shape == (bench.DUMP_MAX_ROWS, 32) and np.all(resid == resid[:, :1])
    # every sampled row IS a row of its chain's array (chain in the millions, bin index below), rows in bin order, no repeats
    D = np.load(tmp_path / "a" / "D.npy").astype(np.float64)
    chain, local = np.floor(D / 1e6), D % 1e6
    assert np.all(np.diff(D) > 0) and set(np.unique(chain)) <= set(range(5))
    assert all(local[chain == c].max() < b.lens[int(c)] for c in np.unique(chain))
    lag = np.load(tmp_path / "a" / "lag.npy")
    assert lag.shape == (bench.DUMP_MAX_ROWS, 2, 2) and 1 not in set(np.floor(lag[:, 0, 0] / 1e6).astype(int))
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "sumNLL.npy"), sums[1])
    # forward only: the forward exports alone
    fwd = bench.dump_outputs(b, b.lens, True, sums, str(tmp_path / "f"))
    assert set(fwd) == {"D", "xf", "Pf", "pnoise", "sumD", "sumNLL"}
