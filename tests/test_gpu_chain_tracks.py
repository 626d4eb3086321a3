"""GPU tests (run with -m gpu) of the contract the three resident per-chain tracks of a batch share -- scores, null template,
selection mask: presence, transfers at the padded chain offsets, which track invalidates which, the walk over the chains a
mask takes, the one value-error code of the peak stages, and the end of the tracks with their batch.  No fit is needed: the
entries want a configured batch only.  Chains of 1, 63, 64 and 65 bins: chain offsets are padded to 64 bins, so these are the
lengths at which a transfer can touch a neighbour or the padding."""
import ctypes as C

import numpy as np
import pytest

from conftest import gpu_available

pytestmark = pytest.mark.gpu

LENS = [1, 63, 64, 65]
U8P = C.POINTER(C.c_uint8)


@pytest.fixture(scope="module")
def L():
    if not gpu_available():
        pytest.fail("GPU tests selected but no HIP device / library: the product has no CPU fallback")
    from consenrich_amd import _lib

    return _lib


def _batch(lens=LENS):
    from consenrich_amd.batch import DeviceBatch, ModelParams

    b = DeviceBatch(0)
    b.configure(ModelParams(state_dim=2), 1, list(lens))
    return b


def _ptr(L, a):
    return a.ctypes.data_as(U8P) if a.dtype == np.uint8 else L.dp(a)


class Track:
    """One row of the table: the raw C entries of a track (the Python methods check shapes and values before the call), what
    its errors say, and values that encode (chain, bin)."""

    def __init__(self, name, up, down, missing, dtype, bad_value, bad_text):
        self.name, self.up, self.down, self.missing, self.dtype = name, up, down, missing, dtype
        self.bad_value, self.bad_text = bad_value, bad_text

    def prepare(self, b):
        # a mask can be planted once the batch has its ROCCO buffers, which the first scores make (as before the tracks shared a type)
        if self.name == "solution":
            b.upload_scores(0, np.zeros(b.chain_lens[0]))

    def values(self, chain, n, generation=0):
        if self.dtype == np.uint8:
            v = np.random.default_rng(100 * generation + chain).integers(0, 2, n).astype(np.uint8)
            v[0] = v[-1] = 1            # (the padding around a chain is zero)
            return v
        return 1000.0 * (chain + 1) + np.arange(n, dtype=np.float64) + 0.25 * generation

    def upload(self, L, b, chain, v):
        return getattr(L.lib(), self.up)(b._ctx, chain, _ptr(L, np.ascontiguousarray(v, self.dtype)))

    def download(self, L, b, chain, n=None):
        out = np.full(b.chain_lens[chain] if n is None else n, 77, self.dtype)
        return getattr(L.lib(), self.down)(b._ctx, chain, _ptr(L, out)), out


TRACKS = [
    Track("scores", "csr_batch_upload_scores", "csr_batch_download_scores", "has no scores", np.float64, np.nan,
          "`scores` contains non-finite values"),
    Track("template", "csr_batch_null_template_upload", "csr_batch_null_template_download", "has no null template", np.float64,
          np.inf, "`template` contains non-finite values"),
    Track("solution", "csr_batch_rocco_upload", "csr_batch_rocco_download", "has no ROCCO solution", np.uint8, 2,
          "a selection mask holds 0 and 1 only"),
]
track_param = pytest.mark.parametrize("t", TRACKS, ids=[t.name for t in TRACKS])


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@track_param
def test_a_chain_has_a_track_only_after_its_own_upload(L, t):
    with _batch() as b:
        t.prepare(b)
        for chain in (0, 3):
            rc, _ = t.download(L, b, chain)
            assert rc == -1 and L.last_error() == f"chain {chain} {t.missing}"
        assert t.upload(L, b, 0, t.values(0, LENS[0])) == 0
        assert t.download(L, b, 0)[0] == 0
        rc, _ = t.download(L, b, 3)
        assert rc == -1 and L.last_error() == f"chain 3 {t.missing}"
        for chain in (-1, 4):
            assert t.download(L, b, chain, 1)[0] == -1 and L.last_error() == "chain index out of range"
            assert t.upload(L, b, chain, t.values(0, 1)) == -1 and L.last_error() == "chain index out of range"


@track_param
def test_transfers_land_on_the_padded_chain_offsets_and_touch_no_neighbour(L, t):
    with _batch() as b:
        t.prepare(b)
        for chain in (3, 1, 0, 2):
            assert t.upload(L, b, chain, t.values(chain, LENS[chain])) == 0, L.last_error()
        first = []
        for chain, n in enumerate(LENS):
            rc, got = t.download(L, b, chain)
            assert rc == 0 and _same(got, t.values(chain, n)), (chain, got)
            first.append(got)
        # chain 1 alone again: the others keep every bit
        assert t.upload(L, b, 1, t.values(1, LENS[1], generation=1)) == 0
        for chain, n in enumerate(LENS):
            rc, got = t.download(L, b, chain)
            assert rc == 0 and _same(got, t.values(1, n, generation=1) if chain == 1 else first[chain]), chain
        assert not _same(t.values(1, LENS[1], generation=1), first[1])


@track_param
def test_a_rejected_upload_changes_neither_content_nor_presence(L, t):
    with _batch() as b:
        t.prepare(b)
        assert t.upload(L, b, 2, t.values(2, LENS[2])) == 0
        for chain in (2, 3):                        # a chain that has the track, and one that does not
            bad = t.values(chain, LENS[chain], generation=1).astype(t.dtype)
            bad[LENS[chain] // 2] = t.bad_value
            assert t.upload(L, b, chain, bad) == -1 and L.last_error() == t.bad_text
        rc, got = t.download(L, b, 2)
        assert rc == 0 and _same(got, t.values(2, LENS[2]))
        rc, _ = t.download(L, b, 3)
        assert rc == -1 and L.last_error() == f"chain 3 {t.missing}"


def test_new_scores_drop_the_chains_mask_and_keep_its_template(L):
    with _batch() as b:
        for chain, n in enumerate(LENS):
            b.upload_scores(chain, np.cos(np.arange(n) + chain))
        b.rocco(budget=0.5)
        tmpl = np.sin(np.arange(LENS[1]) + 0.5)
        b.upload_template(1, tmpl)
        mask0 = b.rocco_solution(0)
        b.upload_scores(1, np.ones(LENS[1]))
        with pytest.raises(L.ConsenrichAMDError, match="chain 1 has no ROCCO solution"):
            b.rocco_solution(1)
        assert _same(b.rocco_solution(0), mask0)
        assert _same(b.download_template(1), tmpl)


SELECTING = [
    ("rocco", lambda b, take: b.rocco(budget=0.5, chains=take)),
    ("rocco_null", lambda b, take: b.rocco_null(chains=take)),
    ("ess", lambda b, take: b.ess("occupancy", [0.0] * len(LENS), [1.0] * len(LENS), 4, chains=take)),
]


@pytest.mark.parametrize("name,call", SELECTING, ids=[s[0] for s in SELECTING])
def test_a_call_takes_the_masked_chains_and_names_the_first_one_without_scores(L, name, call):
    with _batch() as b:
        for chain in (0, 2):
            b.upload_scores(chain, np.cos(np.arange(LENS[chain]) + chain))
        got = call(b, [True, False, True, False])
        assert got[0] is not None and got[2] is not None and got[1] is None and got[3] is None
        with pytest.raises(L.ConsenrichAMDError, match="chain 1 has no scores"):
            call(b, [True, True, False, False])
        with pytest.raises(L.ConsenrichAMDError, match="chain 1 has no scores"):
            call(b, None)


def test_the_pooled_scale_takes_the_masked_chains_and_names_the_first_one_without_a_template(L):
    with _batch() as b:
        tmpls = {chain: np.sin(np.arange(LENS[chain]) * 0.7 + chain) for chain in (0, 2)}
        for chain, v in tmpls.items():
            b.upload_template(chain, v)
        from consenrich_amd import null as N

        got = b.null_pooled_scale(chains=[True, False, True, False])
        want = N.estimate_template_scale(np.concatenate([tmpls[0], tmpls[2]]))
        assert np.float64(got).tobytes() == np.float64(want).tobytes()
        with pytest.raises(L.ConsenrichAMDError, match="chain 1 has no null template"):
            b.null_pooled_scale(chains=[True, True, False, False])
        with pytest.raises(ValueError, match="`template` must be non-empty"):
            b.null_pooled_scale(chains=[False] * 4)


def test_every_peak_stage_answers_a_value_error_with_the_one_code_and_its_own_text(L):
    lib = L.lib()
    assert L.ERR_VALUE == 2
    assert L.ROCCO_ERR_VALUE == L.DWB_ERR_VALUE == L.SEG_ERR_VALUE == L.NULL_ERR_VALUE == L.ESS_ERR_VALUE == L.ERR_VALUE
    i64 = lambda a: a.ctypes.data_as(L.I64P)  # noqa: E731
    x = np.array([1.0, np.nan, 2.0, 0.5])
    with _batch() as b:
        assert lib.csr_batch_rocco_scores(b._ctx, L.ROCCO_SCORE_LOWER_CONFIDENCE, -1.0) == L.ERR_VALUE
        assert L.last_error() == "`uncertaintyScoreZ` must be finite and non-negative"
        with pytest.raises(ValueError, match="`uncertaintyScoreZ` must be finite and non-negative"):
            b.rocco_scores("lower_confidence", -1.0)
    assert lib.csr_dwb_apply(L.dp(x), 4, L.dp(x), 3, L.dp(np.zeros(4))) == L.ERR_VALUE
    assert L.last_error() == "template and multipliers must have the same length"
    assert lib.csr_null_scale(L.dp(x), 4, L.dp(np.zeros(4))) == L.ERR_VALUE
    assert L.last_error() == "`template` contains non-finite values"
    assert lib.csr_ess_scan(L.dp(x), 4, 3, None, 0, -1, C.byref(L.EssOut())) == L.ERR_VALUE
    assert L.last_error() == "windowIntervals must be nonnegative"
    sc, thr, ns = np.array([1, 2], np.int64), np.array([0.5, 1.0]), np.array([1.0])
    rows, cnt, fl = np.zeros(1, np.int64), np.zeros(3, np.int64), C.c_int32(0)
    assert lib.csr_segments_run(None, L.dp(x), 4, 2, i64(sc), 2, L.dp(thr), 1, L.dp(ns), 1, 0, 0, i64(rows), i64(cnt),
                                C.byref(fl)) == L.ERR_VALUE
    assert L.last_error() == "thresholds and nullScales must have the same length"


@track_param
def test_the_tracks_die_with_their_batch(L, t):
    with _batch() as b:
        t.prepare(b)
        for chain, n in enumerate(LENS):
            assert t.upload(L, b, chain, t.values(chain, n)) == 0
        from consenrich_amd.batch import ModelParams

        b.configure(ModelParams(state_dim=2), 1, [65, 2, 130])
        for chain in range(3):
            rc, _ = t.download(L, b, chain)
            assert rc == -1 and L.last_error() == f"chain {chain} {t.missing}"
        # ... and live again in the new batch, at its offsets
        t.prepare(b)
        for chain, n in ((2, 130), (0, 65), (1, 2)):
            assert t.upload(L, b, chain, t.values(chain, n)) == 0
        for chain, n in ((0, 65), (1, 2), (2, 130)):
            rc, got = t.download(L, b, chain)
            assert rc == 0 and _same(got, t.values(chain, n)), chain
