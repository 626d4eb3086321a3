"""Case table for the background solve at the edges of its two-level partition (csr_background.h, `bg_partition`): chain lengths
around every block count and last-block length at which the partition, the 64-interior groups of `k_bg_local` or the 64-separator
staging of `k_bg_reduced` change shape.  Data generators only, in the style of bg_cases.py (lognormal weights around 128, sinusoid
plus noise on the right-hand side, seeded per case); the expected values come from oracle/bg_truth.py at test time.

kind "plain":  every weight positive.
kind "masked": 5 % zero weights plus a zero stretch of max(n // 20, 3) bins from n // 3, at most STRETCH_MAX = 128 bins (two
               whole blocks of the 64-bin partition, so an interior without any weight is in the table).  For n = 1 and n = 2
               that leaves no positive weight at all: the system is singular, the reference's factorisation reports a modified
               pivot, and the case is flagged `singular` -- its expected output is that report, not a solution.

A condition of the table (tests/test_bg_truth.py asserts it): every non-singular case has cond2(A) <= COND_CAP, so a gate of
4 * 2^-52 * cond2 never exceeds 2e-7.  Two things serve it.  (1) STRETCH_MAX: at span 100 the smallest eigenvalue under a zero
stretch of l bins falls with l whatever the seed (n = 4100: cond2 = 1.2e8, 1.5e8, 1.9e8, 2.3e8, 3.2e8 at l = 64, 100, 128, 160,
205), so the lengths above 2560 cannot keep n // 20.  (2) SEEDS: with n <= 5 the masked kind leaves one or two weights, and
cond2 ~ 9 lam n / sum(w) is under the cap only where they are drawn above ~140; those cases name their seed.  The span-750
regime (cond2 ~ 3e11) stays with bg_cases.py."""
from __future__ import annotations

import numpy as np

from bg_cases import penalties

COND_CAP = 2.0e8
PENALTY_PAIRS = ((5, 0.8), (30, 2.0), (100, 128.0))          # (span, smoothness) -> penalties()
LONG = 600                                                     # above: one penalty pair, masked only
LENGTHS = {
    8: list(range(1, 14)) + list(range(16, 22)) + list(range(72, 78)) + list(range(511, 518))
       + [520, 523, 524, 528, 529, 1032, 1040],
    64: list(range(127, 133)) + [4095, 4096, 4097, 4099, 4100, 4164, 4224],
    0: [2047, 2048, 2049, 2051, 2052],                         # blockLen 0 = the default partition, 1024 bins
}
SEED_BASE = 52000
STRETCH_MAX = 128
SEEDS = {"bp8_n3_span100_masked": 853146, "bp8_n4_span100_masked": 904153, "bp8_n5_span100_masked": 863160}


def block_len(bp):
    return bp if bp > 0 else 1024


def edge_cases():
    cs = []
    for bp, lengths in LENGTHS.items():
        for n in lengths:
            for span, smooth in (PENALTY_PAIRS if n <= LONG else PENALTY_PAIRS[-1:]):
                for kind in (("plain", "masked") if n <= LONG else ("masked",)):
                    name = f"bp{bp}_n{n}_span{span}_{kind}"
                    seed = SEED_BASE + 7 * n + span + (1 if kind == "masked" else 0) + 100003 * bp
                    cs.append(dict(name=name, bp=bp, n=n, span=span, smooth=smooth, kind=kind, seed=SEEDS.get(name, seed),
                                   singular=kind == "masked" and n <= 2))
    return cs


def edge_inputs(case):
    n = case["n"]
    rng = np.random.default_rng(case["seed"])
    w = 128.0 * np.exp(rng.normal(0.0, 0.3, n))
    hit = rng.random(n) < 0.05
    if case["kind"] == "masked":
        w[hit] = 0.0
        w[n // 3: n // 3 + min(max(n // 20, 3), STRETCH_MAX)] = 0.0
    base = 0.3 * np.sin(np.arange(n) / max(n / 7.0, 3.0)) + 0.05
    r = w * (base + rng.normal(0.0, 0.09, n))
    return w, r


def edge_lams(case):
    return penalties(case["span"], case["smooth"])


# ---- the resident update at partition edges: one batch of short and long chains ----------------------------------------
RESIDENT_LENS, RESIDENT_M, RESIDENT_SEED = [77, 12, 516, 1, 523, 4100, 9, 131], 3, 7300


def resident_inputs():
    """The data of test_gpu_parity's `_bg_batch_fixture` (cases.synth + a smooth additive background), with the (amplitude,
    offset) of the background per chain from RESIDENT_SHAPE, so that the asymmetric IRLS stops after 0, 1 and >= 2 passes in one
    batch."""
    import cases

    ins = []
    for c, n in enumerate(RESIDENT_LENS):
        amp, off = RESIDENT_SHAPE[c]
        data, munc = cases.synth(n, RESIDENT_M, RESIDENT_SEED + c, mask_frac=0.02, outlier_frac=0.0)
        bg = (amp * np.sin(np.arange(n) / max(n / 5.0, 8.0)) + off).astype(np.float32)
        ins.append(((data + bg[None, :]).astype(np.float32), munc))
    return ins


# The smoothed level absorbs most of what is planted, so the pass count is decided by the noise left in data - level; what was
# measured with the oracle's own smoother (tests/test_bg_truth.py asserts it): passes 2, 1, 3, 0, 3, 3, 1, 3.  The 1-bin chain stops
# at once because its level is the weighted mean shrunk towards 0 by R / (P0 + R) ~ 8e-5: the residual keeps the sign of the offset.
RESIDENT_SHAPE = [(0.3, 3.0) if n == 1 else (0.3, -0.1) for n in RESIDENT_LENS]
