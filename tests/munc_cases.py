"""Case table for the dense observation-variance seed natives `cMuncObservationMomentSeedPass` (pyx:4843-5351) and
`cMuncSmoothDenseLocalEvidence` (pyx:5577-5741).  Inputs are re-synthesised from seeds; the committed munc/munc_*.npz fixtures hold
the REAL reference's outputs and error texts (tests/golden/make_munc_golden.py).  Every comparison is exact: float32 by bit pattern.

Sizes are the edges of the device path (csrc/csr_munc.h), not workload sizes: m around the 16 tracks a lane keeps in registers and
above one wavefront's 64; n around a wavefront; n around the rolling mean's block of ROLL_BLOCK intervals."""
from __future__ import annotations

import numpy as np

ROLL_BLOCK = 128
F32 = np.float32
SEED_GROUPS = ("seed_shapes", "seed_branches", "seed_edges")
SMOOTH_GROUPS = ("smooth",)
SEED_FIELDS = ("moment", "rhoOut", "omegaRaw", "omegaOut", "local", "variance")
TINY = F32(2.0 ** -40 * 1.2345678)      # next to anything of unit scale its float64 sum is inexact
BIG = F32(1024.0 * 1.337)


# ---------------------------------------------------------------------------------------------------------------
# seed pass
# ---------------------------------------------------------------------------------------------------------------
def seed_inputs(case):
    """(positional arrays, keyword arguments) of a seed-pass call."""
    m, n, rng = case["m"], case["n"], np.random.default_rng(case["seed"])
    level = np.cumsum(rng.normal(0.0, 0.2, n)).astype(F32)
    bg = (0.3 * np.sin(np.arange(n) / 7.0)).astype(F32)
    data = (level[None, :] + bg[None, :] + rng.normal(0.0, 1.0, (m, n)) * rng.gamma(2.0, 0.5, (m, 1))).astype(F32)
    outl = rng.random((m, n)) < 0.05
    data[outl] += F32(25.0)
    munc = rng.gamma(2.0, 0.4, (m, n)).astype(F32) + F32(0.01)
    var = rng.gamma(2.0, 0.01, n).astype(F32)
    kw = dict(case.get("kw", {}))
    opt = case.get("opt", ())
    if "bg" in opt:
        kw["background"] = bg
    if "g" in opt:
        kw["gVariance"] = rng.gamma(2.0, 0.005, n).astype(F32)
    if "neg_var" in opt:                    # stateVariance + G below zero: clipped to 0
        var[::3] = F32(-0.5)
        kw["gVariance"] = np.full(n, 0.01, F32)
    if "floor0" in opt:
        kw["countFloor"] = np.zeros((m, n), F32)
    if "floor" in opt:
        kw["countFloor"] = rng.gamma(2.0, 0.1, (m, n)).astype(F32)
    if "omega" in opt:
        kw["omegaIn"] = rng.uniform(0.5, 1.5, n).astype(F32)
    if "rho" in opt:
        kw["rhoIn"] = rng.uniform(0.2, 1.1, (m, n)).astype(F32)
    if "mask1" in opt:
        a = (rng.random(n) < 0.7).astype(np.uint8)
        a[n // 2] = 0
        kw["activeMask"] = a
    if "mask2" in opt:
        a = (rng.random((m, n)) < 0.7).astype(np.uint8) * 3     # any nonzero byte is active
        a[:, n // 2] = 0                                        # an interval without an active cell
        a[0, 0] = 1
        kw["activeMask"] = a
    if "at_floor" in opt:                   # residual 0 and variance 0: local = -pad, floored
        data[0, 1] = level[1]
        kw.pop("background", None)
        var[1] = F32(0.0)
    if "at_cap" in opt:                     # one large residual against a small cap; a count floor above the cap: floor after cap
        kw["varianceCap"] = 5.0
        data[0, 0] += F32(40.0)
        cf = kw.get("countFloor", np.zeros((m, n), F32)).copy()
        cf[m - 1, n - 1] = F32(7.5)
        kw["countFloor"] = cf
    if "omega_bounds" in opt:               # every track far off at interval 0 (raw omega tiny), spot on at interval 1 (raw omega 1.125)
        data[:, 0] += F32(300.0)
        data[:, 1] = level[1] + (kw["background"][1] if "background" in kw else F32(0.0))
        kw.update(omegaMin=0.5, omegaMax=1.05)
    if "subnormal" in opt:                  # a moment of 1e-40: a float32 subnormal that must survive, through to local
        data[0, 0], level[0], var[0] = F32(1.0e-20), F32(0.0), F32(0.0)
        kw.pop("background", None)
        kw.update(pad=0.0, varianceFloor=1.0e-44)
    if "bad_inactive" in opt:               # invalid values in inactive cells only: must NOT raise
        a = np.ones((m, n), np.uint8)
        a[0, 2] = a[1, 0] = 0
        data[0, 2] = np.nan
        munc[1, 0] = F32(-3.0)
        kw["activeMask"] = a
    return (np.ascontiguousarray(data), np.ascontiguousarray(munc), level, var), kw


def seed_cases():
    cs = []

    def add(group, name, m, n, opt=(), **kw):
        cs.append(dict(group=group, name=name, m=m, n=n, opt=tuple(opt), kw=kw, seed=4000 + len(cs)))

    for m in (5, 17):
        for n in (2, 3, 63, 64, 65):
            add("seed_shapes", f"shape_m{m}_n{n}", m, n, ("bg", "g", "floor", "omega", "rho"))
    for m in (1, 2, 16, 70):
        for n in (3, 65):
            add("seed_shapes", f"shape_m{m}_n{n}", m, n, ("bg", "g", "floor", "omega", "rho"))
    add("seed_shapes", "shape_m5_n300", 5, 300, ("bg", "g", "floor", "omega", "rho", "mask2"))     # past one workgroup of lanes
    # every combination of the four switches, on the register path and past it
    for m in (5, 17):
        for enabled in (True, False):
            for use in (True, False):
                for st in (True, False):
                    for upd in (True, False):
                        add("seed_branches", f"sw_m{m}_e{int(enabled)}u{int(use)}s{int(st)}w{int(upd)}", m, 33,
                            ("bg", "g", "floor", "omega", "rho", "mask2"), enabled=enabled, useSeedWeights=use, studentT=st,
                            updateWeights=upd)
    for m in (5, 17):
        add("seed_edges", f"plain_m{m}", m, 33)
        add("seed_edges", f"omega_none_rho_none_noupdate_m{m}", m, 33, ("bg",), updateWeights=False)
        add("seed_edges", f"omega_1d_noupdate_m{m}", m, 33, ("omega",), updateWeights=False)
        add("seed_edges", f"mask1_m{m}", m, 33, ("bg", "mask1", "floor"))
        add("seed_edges", f"mask2_m{m}", m, 33, ("g", "mask2", "floor0", "rho"))
        add("seed_edges", f"mask2_noupdate_m{m}", m, 33, ("mask2", "rho", "omega"), updateWeights=False)
        add("seed_edges", f"at_floor_m{m}", m, 33, ("at_floor",))
        add("seed_edges", f"at_cap_m{m}", m, 33, ("floor", "at_cap"))
        add("seed_edges", f"at_cap_gauss_m{m}", m, 33, ("at_cap", "mask1"), useSeedWeights=False)
        add("seed_edges", f"omega_bounds_m{m}", m, 33, ("bg", "omega_bounds"))
        add("seed_edges", f"neg_var_m{m}", m, 33, ("neg_var",))
        add("seed_edges", f"subnormal_m{m}", m, 3, ("subnormal",))
        add("seed_edges", f"subnormal_gauss_m{m}", m, 3, ("subnormal",), useSeedWeights=False)
        add("seed_edges", f"bad_inactive_m{m}", m, 33, ("bad_inactive", "floor"))
    return cs


def _seed_error_table():
    z = lambda *s: np.zeros(s, F32)     # noqa: E731
    one = lambda *s: np.ones(s, F32)    # noqa: E731
    shape = [
        ("err_munc_shape", lambda a, k: ((a[0], one(5, 8), a[2], a[3]), k), "matrixMunc shape must match matrixData shape"),
        ("err_mean_len", lambda a, k: ((a[0], a[1], z(8), a[3]), k), "stateMean length must match interval count"),
        ("err_var_len", lambda a, k: ((a[0], a[1], a[2], z(8)), k), "stateVariance length must match interval count"),
        ("err_pad", lambda a, k: (a, dict(k, pad=-1.0)), "pad must be finite and nonnegative"),
        ("err_pad_nan", lambda a, k: (a, dict(k, pad=float("nan"))), "pad must be finite and nonnegative"),
        ("err_floor", lambda a, k: (a, dict(k, varianceFloor=0.0)), "varianceFloor must be positive and finite"),
        ("err_cap", lambda a, k: (a, dict(k, varianceCap=1.0e-13)), "varianceCap must be greater than or equal to varianceFloor"),
        ("err_cap_inf", lambda a, k: (a, dict(k, varianceCap=float("inf"))), "varianceCap must be greater than or equal to varianceFloor"),
        ("err_df", lambda a, k: (a, dict(k, studentTdf=0.0)), "seed weight parameters are invalid"),
        ("err_domega", lambda a, k: (a, dict(k, dOmega=-1.0)), "seed weight parameters are invalid"),
        ("err_omega_bounds", lambda a, k: (a, dict(k, omegaMin=2.0, omegaMax=1.0)), "seed weight parameters are invalid"),
        ("err_bg_len", lambda a, k: (a, dict(k, background=z(8))), "background length must match interval count"),
        ("err_g_len", lambda a, k: (a, dict(k, gVariance=z(8))), "gVariance length must match interval count"),
        ("err_floor_shape", lambda a, k: (a, dict(k, countFloor=z(5, 8))), "countFloor shape must match matrixData shape"),
        ("err_omega_len", lambda a, k: (a, dict(k, omegaIn=one(8))), "omegaIn length must match interval count"),
        ("err_omega_2d", lambda a, k: (a, dict(k, omegaIn=one(5, 9))), "omegaIn must be one-dimensional"),
        ("err_rho_shape", lambda a, k: (a, dict(k, rhoIn=one(5, 8))), "rhoIn shape must match matrixData shape"),
        ("err_mask_len", lambda a, k: (a, dict(k, activeMask=np.ones(8, np.uint8))), "activeMask length must match interval count"),
        ("err_mask_shape", lambda a, k: (a, dict(k, activeMask=np.ones((4, 9), np.uint8))), "activeMask shape must match matrixData shape"),
        ("err_mask_3d", lambda a, k: (a, dict(k, activeMask=np.ones((5, 9, 1), np.uint8))), "activeMask must be one- or two-dimensional"),
    ]
    bad = "active MUNC seed cells must be finite with positive denominators"

    def poke(which, i, value, **more):
        def f(a, k):
            a = [x.copy() for x in a]
            k = dict(k, **more)
            if isinstance(which, int):
                a[which][i] = value
            else:
                k[which] = k[which].copy()
                k[which][i] = value
            return tuple(a), k
        return f

    cells = [
        ("bad_mean", poke(2, 4, np.nan)), ("bad_var", poke(3, 4, np.inf)), ("bad_bg", poke("background", 4, np.nan)),
        ("bad_g", poke("gVariance", 4, -np.inf)), ("bad_data", poke(0, (2, 4), np.inf)), ("bad_munc", poke(1, (2, 4), -1.0)),
        ("bad_munc_nan", poke(1, (2, 4), np.nan)), ("bad_floor_neg", poke("countFloor", (2, 4), -0.5)),
        ("bad_floor_nan", poke("countFloor", (2, 4), np.nan)), ("bad_omega", poke("omegaIn", 4, 0.0)),
        ("bad_rho", poke("rhoIn", (2, 4), 0.0, updateWeights=False)),
    ]
    return shape + [(name, f, bad) for name, f in cells]


def seed_error_cases():
    """[(name, positional arrays, keyword arguments, text)] on a 5 x 9 base case with every optional input present."""
    base = dict(group="seed_errors", name="base", m=5, n=9, opt=("bg", "g", "floor", "omega", "rho"), kw={}, seed=4999)
    out = []
    for name, f, text in _seed_error_table():
        a, k = seed_inputs(base)
        a, k = f(a, k)
        out.append((name, a, k, text))
    return out


def run_seed(mod, case):
    a, k = seed_inputs(case)
    res = mod.cMuncObservationMomentSeedPass(*a, **k)
    assert isinstance(res, tuple) and len(res) == 6
    return dict(zip(SEED_FIELDS, res))


# ---------------------------------------------------------------------------------------------------------------
# rolling mean
# ---------------------------------------------------------------------------------------------------------------
def smooth_inputs(case):
    """(local, window, exclude mask or None).  Benign rows hold multiples of 1/8 below 128: every float64 sum of them is exact."""
    m, n, rng = case["m"], case["n"], np.random.default_rng(case["seed"])
    local = (rng.integers(1, 1024, (m, n)) / 8.0).astype(F32)
    mask = None
    kind = case.get("mask")
    if kind == "1d":
        mask = (rng.random(n) < 0.3).astype(np.uint8) * 2
    elif kind == "2d":
        mask = (rng.random((m, n)) < 0.3).astype(np.uint8)
    elif kind == "stretch":                 # a fully excluded window: count == 0 falls back to the cell's own value
        mask = np.zeros(n, np.uint8)
        mask[n // 4: n // 4 + 3 * case["window"] + 2] = 1
    for row, idx in case.get("plant", ()):
        local[row, idx] = TINY
        if idx + 1 < n:
            local[row, idx + 1] = BIG
    for row, idx in case.get("hide", ()):   # a non-positive cell under the mask
        local[row, idx] = F32(-1.0)
        if mask is None:
            mask = np.zeros((m, n), np.uint8)
        if mask.ndim == 1:
            mask[idx] = 1
        else:
            mask[row, idx] = 1
    return np.ascontiguousarray(local), case["window"], mask


def smooth_cases():
    cs = []
    B = ROLL_BLOCK

    def add(name, m, n, window, **kw):
        kw.setdefault("fallback_rows", 0)
        cs.append(dict(group="smooth", name=name, m=m, n=n, window=window, seed=6000 + len(cs), **kw))

    for n in (2, 3, 63, 64, 65, B - 1, B, B + 1, 2 * B + 1):
        for w in (1, 2, 5, n, n + 3):
            add(f"benign_n{n}_w{w}", 2, n, w)
    add("benign_m70", 70, B + 1, 5)
    add("benign_mask1d", 5, 2 * B + 1, 5, mask="1d")
    add("benign_mask2d", 5, 2 * B + 1, 4, mask="2d")
    add("excluded_window", 3, 2 * B + 1, 5, mask="stretch")
    add("hidden_bad_1d", 3, B + 1, 5, mask="1d", hide=((1, 70),))
    add("hidden_bad_2d", 3, B + 1, 5, hide=((1, 70),))
    # a 2^-40-scale cell (its float32 bits reach 2^-63) next to a 2^10-scale one: the running sum is inexact from where it enters.
    # window 5: cell k enters at interval k - 2.  Rows without a plant stay speculative.
    n = 2 * B + 1
    add("plant_first_block", 3, n, 5, plant=((1, 10),), fallback_rows=1)
    add("plant_block_edge_body", 3, n, 5, plant=((0, B + 2),), fallback_rows=1)        # enters at interval B: block 1's first step
    add("plant_block_edge_entry", 3, n, 5, plant=((2, B + 1),), fallback_rows=1)       # enters at B - 1: also in block 1's entry sum
    add("plant_entry_sum", 3, n, 9, plant=((1, B - 3),), fallback_rows=1)              # well inside the window at block 1's entry
    add("plant_last_block", 3, n, 5, plant=((0, n - 2),), fallback_rows=1)
    add("plant_every_row_wide", 70, n, n + 3, plant=tuple((r, 40) for r in range(70)), fallback_rows=70)
    add("plant_masked_1d", 4, n, 5, mask="1d", plant=((0, 30), (3, B + 40)), fallback_rows=None)   # (a plant may fall under the mask)
    return cs


SMOOTH_ERRORS = (
    ("err_window", dict(window=0), "windowIntervals must be positive"),
    ("err_eps", dict(eps=0.0), "eps must be positive and finite"),
    ("err_eps_inf", dict(eps=float("inf")), "eps must be positive and finite"),
    ("err_mask_len", dict(mask=np.zeros(8, np.uint8)), "excludeMask length must match interval count"),
    ("err_mask_shape", dict(mask=np.zeros((2, 9), np.uint8)), "excludeMask shape must match localEvidence shape"),
    ("err_mask_3d", dict(mask=np.zeros((3, 9, 1), np.uint8)), "excludeMask must be one- or two-dimensional"),
    ("bad_zero", dict(poke=0.0), "active local evidence cells must be positive and finite"),
    ("bad_nan", dict(poke=float("nan")), "active local evidence cells must be positive and finite"),
    ("bad_inf_under_other_mask", dict(poke=float("inf"), mask=np.array([1, 0, 0, 0, 0, 0, 0, 0, 0], np.uint8)),
     "active local evidence cells must be positive and finite"),
)


def smooth_error_cases():
    """[(name, local, window, mask, eps, text)] on a 3 x 9 benign base."""
    out = []
    for name, kw, text in SMOOTH_ERRORS:
        local, window, mask = smooth_inputs(dict(m=3, n=9, window=3, seed=6999))
        if "poke" in kw:
            local[1, 4] = kw["poke"]
        out.append((name, local, kw.get("window", window), kw.get("mask", mask), kw.get("eps", 1.0e-12), text))
    return out


def run_smooth(mod, case):
    local, window, mask = smooth_inputs(case)
    return dict(out=mod.cMuncSmoothDenseLocalEvidence(local, window, excludeMask=mask))


# ---------------------------------------------------------------------------------------------------------------
def same(a, b):
    """Bit equality of two result dicts of float32 arrays."""
    if set(a) != set(b):
        return False
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if x.dtype != np.float32 or y.dtype != np.float32 or x.shape != y.shape:
            return False
        if not np.array_equal(x.view(np.uint32), y.view(np.uint32)):
            return False
    return True


def load_group(path):
    out = {}
    with np.load(path) as z:
        for key in z.files:
            name, field = key.rsplit("/", 1)
            out.setdefault(name, {})[field] = z[key]
    return out
