"""The case table of the state-shrinkage tests.  Inputs are re-synthesised from seeds and never stored; the fixtures under
tests/golden/shrink/ hold what the compiled reference answered (tests/golden/make_shrink_golden.py).

A chunk is a spike-and-slab draw: 85 % of the bins are noise around zero with the bin's own variance, 15 % carry a signal of
standard deviation 3 on top.  The values are float64 and NOT float32-representable.  Invalid cells are planted at fixed places
(`planted`): NaN and Inf in the state, variance 0, negative, Inf and NaN, a variance of 1e-20 (valid, floored at 1e-12), and in
the cases marked `dead_block` a whole block without a valid bin.  Every bin of these cases has postSecond / postVariance far
below 1e6 (the generator asserts it), so the posterior sd is gated everywhere; `floor_case` is the one input made to sit on the
1e-12 floor of the posterior variance."""
from __future__ import annotations

import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shrink")
STUDENT, MIXTURE, NORMAL = "spikeAndStudentT", "adaptiveNormalMixture", "spikeAndNormal"

# name: (chunk lengths, block size, seed, dead_block)
INPUTS = {
    "a_b1": ((700, 1300, 257), 1, 11, False),
    "a_b64": ((700, 1300, 257), 64, 11, True),
    "b_b500": ((5000, 3000), 500, 12, False),
    "c_b7": ((64, 65, 1), 7, 13, True),
    "d_b50": ((20000,), 50, 14, False),
}
# (input, model, quadrature order): the whole fits; the first EM pass of each is the per-pass case of its slab count
FITS = [(inp, model, 16 if model == STUDENT else 0) for inp in INPUTS for model in (STUDENT, MIXTURE, NORMAL)]
FITS += [("a_b64", STUDENT, order) for order in (8, 12, 96)]
# the fits whose posterior tracks are stored (the 20 000-bin chain: the default model only)
POSTERIORS = [f for f in FITS if f[0] != "d_b50" or f[1] == STUDENT]


def fit_name(inp, model, order) -> str:
    return f"{inp}_{model}" + (f"_q{order}" if order else "")


def fixture_path(inp, model, order) -> str:
    return os.path.join(GOLDEN, f"shrink_{fit_name(inp, model, order)}.npz")


def synth_chunk(n: int, rng, dead_block=None):
    v = rng.uniform(0.09, 1.0, n)
    signal = rng.random(n) < 0.15
    x = rng.standard_normal(n) * np.sqrt(v + np.where(signal, 9.0, 0.0))
    if n >= 64:         # planted invalid cells (and one valid variance below the floor)
        x[3], x[17] = np.nan, np.inf
        v[5], v[9], v[21], v[33] = 0.0, -0.25, np.inf, np.nan
        v[40] = 1.0e-20
        x[40] = 1.0e-7
    if dead_block is not None:
        a, b = dead_block
        x[a:b:2] = np.nan
        v[a + 1:b:2] = -1.0
    return x, v


def make_input(name: str):
    """[(state, variance)] of an input, and its block size."""
    lens, block, seed, dead = INPUTS[name]
    rng = np.random.default_rng(seed)
    chunks = []
    for i, n in enumerate(lens):
        db = None
        if dead and i == 0:
            db = (block, 2 * block) if 2 * block <= n else None
        chunks.append(synth_chunk(n, rng, db))
    return chunks, block


def floor_case():
    """Large |x| with variances at and below the 1e-12 floor: the posterior variance sits on its own 1e-12 floor."""
    x = np.array([25.0, -40.0, 1.0e3, 7.5, -3.0e2, 12.0])
    v = np.array([1.0e-12, 1.0e-13, 1.0e-12, 1.0e-15, 1.0e-12, 1.0e-12])
    return x, v


def fit_kwargs(model, order) -> dict:
    kw = {"model": model}
    if order:
        kw["studentTQuadratureOrder"] = order
    return kw


def load_fixture(inp, model, order):
    with np.load(fixture_path(inp, model, order), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}
