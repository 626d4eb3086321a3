"""The NumPy / Python twin of the dense observation-variance seed natives (tests/twin_munc.py) against the compiled reference's
fixtures (tests/golden/munc), its two forms against each other, and the condition the GPU tests rely on: the benign rolling-mean
cases see no non-zero TwoSum residual, the planted ones at least one.  No GPU."""
import os

import numpy as np
import pytest

import munc_cases as MC
import twin_munc as T

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "munc")
SEED = {c["name"]: c for c in MC.seed_cases()}
SMOOTH = {c["name"]: c for c in MC.smooth_cases()}


@pytest.fixture(scope="module")
def gold():
    g = {}
    for group in MC.SEED_GROUPS + MC.SMOOTH_GROUPS:
        g.update(MC.load_group(os.path.join(GOLD, f"munc_{group}.npz")))
    with np.load(os.path.join(GOLD, "munc_errors.npz")) as z:
        g["__errors__"] = {k: str(z[k]) for k in z.files}
    return g


def test_fixtures_cover_the_case_table(gold):
    assert set(gold) - {"__errors__"} == set(SEED) | set(SMOOTH)
    names = {n for n, *_ in MC.seed_error_cases()} | {"smooth_" + n for n, *_ in MC.smooth_error_cases()}
    assert set(gold["__errors__"]) == names


@pytest.mark.parametrize("name", sorted(SEED))
def test_seed_pass_twin_equals_reference(gold, name):
    assert MC.same(gold[name], MC.run_seed(T, SEED[name]))


@pytest.mark.parametrize("name", sorted(SEED))
def test_seed_pass_device_form_equals_reference_form(gold, name):
    a, k = MC.seed_inputs(SEED[name])
    assert MC.same(gold[name], dict(zip(MC.SEED_FIELDS, T.seed_pass_device(*a, **k))))


@pytest.mark.parametrize("name", sorted(SMOOTH))
def test_smooth_twin_equals_reference(gold, name):
    assert MC.same(gold[name], MC.run_smooth(T, SMOOTH[name]))


@pytest.mark.parametrize("name", sorted(SMOOTH))
def test_smooth_device_form_and_its_residuals(gold, name):
    case = SMOOTH[name]
    local, window, mask = MC.smooth_inputs(case)
    out, redone, residuals = T.smooth_device(local, window, excludeMask=mask)
    assert MC.same(gold[name], dict(out=out))
    if case["fallback_rows"] is not None:
        assert redone == case["fallback_rows"]
        assert (residuals > 0) == (case["fallback_rows"] > 0)      # benign: none at all; planted: at least one


def test_subnormal_moment_survives(gold):
    m = gold["subnormal_m5"]["moment"][0, 0]
    assert 0.0 < m < np.finfo(np.float32).tiny
    loc = gold["subnormal_m5"]["local"][0, 0]
    assert 0.0 < loc < np.finfo(np.float32).tiny


def test_error_texts(gold):
    for name, a, k, text in MC.seed_error_cases():
        assert gold["__errors__"][name] == text
        with pytest.raises(ValueError) as e:
            T.cMuncObservationMomentSeedPass(*a, **k)
        assert str(e.value) == text
        with pytest.raises(ValueError) as e:
            T.seed_pass_device(*a, **k)
        assert str(e.value) == text
    for name, local, window, mask, eps, text in MC.smooth_error_cases():
        assert gold["__errors__"]["smooth_" + name] == text
        with pytest.raises(ValueError) as e:
            T.cMuncSmoothDenseLocalEvidence(local, window, excludeMask=mask, eps=eps)
        assert str(e.value) == text


def test_twin_glue_helpers_equal_their_numpy_expressions():
    """The per-cell glue of the twin against the reference's NumPy expressions written out (consenrich.py:7482-7503, 7557-7576,
    7938-7945) and `_backgroundPenaltyDiagonal` at its edge lengths.  These helpers are what tests/test_gpu_munc.py holds the
    device's per-cell kernels to; the fixtures cover the natives, not this glue."""
    rng = np.random.default_rng(7)
    total = rng.gamma(2.0, 0.5, (3, 11)).astype(np.float32)
    rho = rng.uniform(0.1, 1.1, (3, 11)).astype(np.float32)
    omega = rng.uniform(0.5, 1.1, 11).astype(np.float32)
    g = rng.gamma(2.0, 0.01, 11).astype(np.float32)
    w = T.seed_working_munc(total, omega, rho, g, 1.0e-4, True)
    want = np.maximum((total.astype(np.float64) + 1.0e-4) / np.maximum(omega.astype(np.float64)[None, :] * rho, 1.0e-12)
                      + g.astype(np.float64)[None, :] - 1.0e-4, 1.0e-12).astype(np.float32)
    assert np.array_equal(w.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(T.response_weight(rho, omega, True), rho * omega[None, :])
    assert np.array_equal(T.response_weight(rho, omega, False), np.ones_like(rho))
    tv = T.local_to_total_variance(total, rho, 1.0)
    assert np.array_equal(tv, np.maximum(np.minimum(total + rho, np.float32(1.0)), np.float32(1.0e-12))) and tv.dtype == np.float32
    assert np.array_equal(T.local_to_total_variance(total, None, None), np.maximum(total, np.float32(1.0e-12)))
    assert T.penalty_diagonal(1, 2.0, 3.0).tolist() == [0.0]
    assert T.penalty_diagonal(2, 2.0, 3.0).tolist() == [2.0, 2.0]
    assert T.penalty_diagonal(3, 2.0, 3.0).tolist() == [5.0, 16.0, 5.0]
    assert T.penalty_diagonal(4, 2.0, 3.0).tolist() == [5.0, 19.0, 19.0, 5.0]
    assert T.penalty_diagonal(6, 2.0, 3.0).tolist() == [5.0, 19.0, 22.0, 22.0, 19.0, 5.0]


def test_plain_c_restatement_equals_the_reference(gold, tmp_path):
    """scripts/ubench/munc_cpu.c, the one-core yardstick of scripts/munc_seed_bench.py, on every case of the table."""
    port = T.CPort(tmp_path)
    for name, case in SEED.items():
        assert MC.same(gold[name], MC.run_seed(port, case)), name
    for name, case in SMOOTH.items():
        assert MC.same(gold[name], MC.run_smooth(port, case)), name
    bad = [c for c in MC.seed_error_cases() if c[0].startswith("bad_")]
    for name, a, k, text in bad:
        with pytest.raises(ValueError) as e:
            port.cMuncObservationMomentSeedPass(*a, **k)
        assert str(e.value) == text, name
