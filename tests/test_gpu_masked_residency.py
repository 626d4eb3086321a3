"""GPU tests of what a MASKED pass leaves resident for the chains outside its mask (run with -m gpu): the NIS / NLL track D, the
process-noise rows and the per-chain sums beside the filtered and smoothed arrays.  An unmasked pass may leave D (and xf / Pf) in
the reference layout only and stores no process-noise rows at all when the noise is one constant matrix; a masked pass rewrites the
blocked copies of ITS chains, and the export that follows converts the blocked copies of EVERY chain -- so the others must have
got theirs back first (csr_batch_forward_masked: 'the others keep their resident results'; csr_batch_ecm_masked: 'the others keep
the resident results of their last fit untouched').

The edge is chains that share one 64-block wavefront group and one 32-step tile with a chain of the other side of the mask, not
chain length: with block length B the chains are [3 B + 5, 4, B + 1, 2 B, 65 B + 7] bins -- group 0 holds blocks of four chains,
masked alternately, and the last chain crosses into group 1."""
import numpy as np
import pytest

import cases
from conftest import gpu_available
from test_gpu_parity import ATOL, RTOL
from test_gpu_residency import _close

pytestmark = pytest.mark.gpu

M = 3
SEED = 9400
FWD = ("D", "xf", "Pf", "pnoise")
SMOOTH = ("xs", "Ps", "lag")
EVERY = FWD + SMOOTH
MASKS = {"mask": [True, False, True, False, True], "complement": [False, True, False, True, False]}
SEQUENCES = ("step+forward_masked", "forward+export+forward_masked", "step+background+forward_masked", "step+ecm_masked",
             "step+two_disjoint_masks")


@pytest.fixture(scope="module")
def product():
    if not gpu_available():
        pytest.fail("GPU tests selected but no HIP device / library: the product has no CPU fallback")
    from consenrich_amd import cconsenrich

    return cconsenrich


def _chains(B):
    return [3 * B + 5, 4, B + 1, 2 * B, 65 * B + 7]


def _model(dim):
    from consenrich_amd.batch import ModelParams

    # (the level model as tests/test_gpu_level_model.py builds it)
    return ModelParams(state_dim=2) if dim == 2 else ModelParams(state_dim=1, Q0=((1e-3, 0), (0, 0)))


_SETS = {}


def _sets(B):
    if B not in _SETS:
        _SETS[B] = [cases.synth(n, M, SEED + c, outlier_frac=0.01) for c, n in enumerate(_chains(B))]
    return _SETS[B]


def _background(n, c):
    """a non-zero background track, the way the driver installs one between two outer passes"""
    t = np.arange(n, dtype=np.float64)
    return (0.25 + 0.2 * np.sin(t / 37.0 + c)).astype(np.float32)


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32 if x.dtype == np.float32 else np.uint64)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _new_batch(B, dim, xtol):
    from consenrich_amd.batch import DeviceBatch

    b = DeviceBatch(0, block_len=B, x_tol_ulps=xtol)
    b.configure(_model(dim), M, _chains(B))
    for c, (d_, v_) in enumerate(_sets(B)):
        b.upload(c, d_, v_)
    return b


@pytest.mark.parametrize("xtol", [0, 2], ids=["exact", "ulp2"])
@pytest.mark.parametrize("dim", [2, 1], ids=["levelTrend", "level"])
@pytest.mark.parametrize("which", sorted(MASKS))
@pytest.mark.parametrize("B", [64, 256])
@pytest.mark.parametrize("seq", SEQUENCES)
def test_chains_outside_a_masked_pass_keep_D_pnoise_and_their_sums(product, seq, B, which, dim, xtol):
    """Five call sequences, each ending in an export of every array of every chain:

    1. step, forward_masked, backward, export           2. forward, export, forward_masked, export (no step: csr_batch_forward
    3. step, new backgrounds for the masked chains,        writes D into the reference layout only as well)
       stats, forward_masked, backward, export          4. step, a masked ECM call with kappa (the step's process noise was one
    5. step, forward_masked(mask), forward_masked(          constant matrix: no blocked rows), export
       complement), export

    OUTSIDE the mask D, xf, Pf, the process-noise rows and the per-chain sums come back bit for bit as recorded before the sequence
    (after the ECM call the smoothed arrays too; after an unmasked backward() on unchanged inputs in the bit-exact mode too: one
    sequential recursion).  The recorded D of every such chain has non-zero entries: the blocked D these sequences start from is
    zeros, so a conversion of stale blocks cannot pass.  INSIDE the mask, sequence 3: every array equals a fresh batch with the same
    data and backgrounds that runs the unmasked statistics + forward + backward + export -- bit for bit in the exact mode, within
    the mode's gate (the one tests/test_gpu_residency.py holds against the oracle; D: the parity gate RTOL / ATOL) in the 2-ulp mode."""
    from consenrich_amd import _lib as L

    mask = MASKS[which]
    n_list = _chains(B)
    nc = len(n_list)
    flags = L.RETURN_NLL
    what = L.EXPORT_FORWARD | L.EXPORT_SMOOTH | L.EXPORT_RESID
    with _new_batch(B, dim, xtol) as b:
        # the resident fit every sequence starts from, and what it hands out
        if seq == "forward+export+forward_masked":
            b.stats()
            b.forward(flags)
            b.export(L.EXPORT_FORWARD)
            names = FWD
        else:
            b.step(flags, what)
            names = EVERY
        before = {(c, a): b.download(c, a) for c in range(nc) for a in names}
        sums_before = b.sums()
        final, outside = L.EXPORT_FORWARD | L.EXPORT_SMOOTH, [c for c in range(nc) if not mask[c]]
        untouched = set(FWD)
        if seq == "step+forward_masked":
            b.forward_masked(flags, mask)
            b.backward()
        elif seq == "forward+export+forward_masked":
            b.forward_masked(flags, mask)
            final = L.EXPORT_FORWARD
        elif seq == "step+background+forward_masked":
            for c in range(nc):
                if mask[c]:
                    b.set_background(c, _background(n_list[c], c))
            b.stats()
            b.forward_masked(flags, mask)
            b.backward()
        elif seq == "step+ecm_masked":
            outs, _ = b.ecm(max_iters=2, inner_iters=2, rtol=0.0, use_kappa=True, chain_mask=mask)
            assert [int(o.skipped) for o in outs] == [0 if mask[c] and n_list[c] > 5 else (1 if mask[c] else 2) for c in range(nc)]
            untouched = set(EVERY)
        else:
            b.forward_masked(flags, mask)
            b.forward_masked(flags, [not t for t in mask])
            final = L.EXPORT_FORWARD
            names = FWD
            outside = []                # (every chain is inside one of the two masks: checked as a whole below)
        b.export(final)
        after = {(c, a): b.download(c, a) for c in range(nc) for a in names}
        sums_after = b.sums()

    tag = (seq, B, which, dim, xtol)
    for c in outside:
        assert np.any(before[(c, "D")] != 0.0), (tag, c)
        for a in names:
            if a in untouched or xtol == 0:
                assert _same_bits(after[(c, a)], before[(c, a)]), (tag, "outside the mask", c, a)
        for k in range(2):
            assert _bits(np.float64(sums_after[k][c])) == _bits(np.float64(sums_before[k][c])), (tag, "sums", c, k)

    if seq in ("step+forward_masked", "forward+export+forward_masked") and xtol == 0:
        for c in range(nc):             # same data, same flags: the masked chains are recomputed to the same bits
            for a in names:
                assert _same_bits(after[(c, a)], before[(c, a)]), (tag, "inside the mask", c, a)

    if seq == "step+two_disjoint_masks":
        # every chain was recomputed once, from the same inputs: the same bits in the exact mode, the mode's gate otherwise; the
        # constant process-noise rows in any mode
        for c in range(nc):
            lvl = np.maximum(np.abs(before[(c, "xs")][:, :1].astype(np.float64)), 1.0)
            assert np.any(before[(c, "D")] != 0.0), (tag, c)
            assert _same_bits(after[(c, "pnoise")], before[(c, "pnoise")]), (tag, c)
            # (the float64 sums of a RECOMPUTED chain are not compared: the covariance chain accepts a block's double carry within
            # 1e-12, so the predicted variance behind log(1 + P S0) of another pass may differ far below float32)
            for a in names:
                if xtol == 0:
                    assert _same_bits(after[(c, a)], before[(c, a)]), (tag, c, a)
                elif a == "D":
                    np.testing.assert_allclose(after[(c, a)], before[(c, a)], rtol=RTOL, atol=ATOL, err_msg=str((tag, c, a)))
                else:
                    _close(after[(c, a)], before[(c, a)], lvl, (tag, c, a))

    if seq == "step+background+forward_masked":
        with _new_batch(B, dim, xtol) as f:
            for c in range(nc):
                if mask[c]:
                    f.set_background(c, _background(n_list[c], c))
            f.stats()
            f.forward_backward(flags)
            f.export(L.EXPORT_FORWARD | L.EXPORT_SMOOTH)
            fresh = {(c, a): f.download(c, a) for c in range(nc) if mask[c] for a in EVERY}
        for c in range(nc):
            if not mask[c]:
                continue
            # (the new background moved the level: the masked pass did compute something new)
            assert not np.array_equal(after[(c, "xf")], before[(c, "xf")]), (tag, c)
            lvl = np.maximum(np.abs(fresh[(c, "xs")][:, :1].astype(np.float64)), 1.0)
            for a in EVERY:
                got, ref = after[(c, a)], fresh[(c, a)]
                if xtol == 0:
                    assert _same_bits(got, ref), (tag, "inside the mask", c, a)
                elif a == "D":
                    np.testing.assert_allclose(got, ref, rtol=RTOL, atol=ATOL, err_msg=str((tag, "inside the mask", c, a)))
                else:
                    _close(got, ref, lvl, (tag, "inside the mask", c, a))
