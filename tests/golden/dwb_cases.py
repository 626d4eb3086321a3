"""Case table for the stationary-null DWB natives: `cGenerateDWBMultipliersFromNoise`, `cApplyStationaryNullDWB`,
`cStationaryNullDWBDraw` (pyx:9283-9424).  Inputs are re-synthesised from (gen, n, seed); the committed dwb/dwb_*.npz fixtures (a
directory of their own, like rocco/) hold the REAL reference's outputs (tests/golden/make_dwb_golden.py).  Every comparison is
exact: float64 values by their 64-bit patterns."""
from __future__ import annotations

import numpy as np

ST = 256        # outputs per workgroup of the device stencil and values per LDS tile of the device walk (csrc/csr_dwb.h DWB_ST, DWB_WT)
WT = 64         # values of a row the walk fetches at a time (one per lane)
KERNELS = ("bartlett", "parzen", "qs")
BANDWIDTHS = (0, 1, 2, 3, 17, 64)
GROUPS = ("mult", "tiles", "draw", "apply")


def _max_lag(bw, kernel):
    bw = max(bw, 2)
    qs = kernel.strip().lower().replace("-", "_") in ("qs", "quadratic_spectral", "quadraticspectral")
    return max(8 * bw, 32) if qs else bw


def cases():
    cs = []
    # multipliers: every kernel x bandwidth; n = 1 is a noise vector exactly 2 maxLag + 1 long (sd = 0 -> multipliers 1.0)
    for kern in KERNELS:
        for bw in BANDWIDTHS:
            for n in (1, 2, 3, WT + 1):
                cs.append(dict(group="mult", name=f"mult_{kern}_bw{bw}_n{n}", kind="mult", kernel=kern, bw=bw, n=n, gen="gauss",
                               seed=1000 + 7 * bw + n))
    # other spellings of the kernel names
    for kern in ("Triangle", " triangular ", "PARZEN", "quadratic-spectral", "quadraticspectral", "quadratic_spectral"):
        cs.append(dict(group="mult", name=f"mult_name_{kern.strip()}", kind="mult", kernel=kern, bw=3, n=40, gen="gauss", seed=7))
    for gen in ("const", "nan", "zero"):
        for n in (5, WT + 3):
            cs.append(dict(group="mult", name=f"mult_{gen}_n{n}", kind="mult", kernel="bartlett", bw=3, n=n, gen=gen, seed=8))
    # around the walk's 64-value fetch and the 256-value tile of the walk and the stencil
    for n in (WT - 1, WT, 2 * WT + 1, ST - 1, ST, ST + 1, 2 * ST + 1):
        cs.append(dict(group="tiles", name=f"tiles_mult_n{n}", kind="mult", kernel="bartlett", bw=5, n=n, gen="gauss", seed=2000 + n))
        cs.append(dict(group="tiles", name=f"tiles_draw_n{n}", kind="draw", kernel="parzen", bw=4, n=n, gen="gauss", seed=2100 + n,
                       tmpl="gauss"))
    cs.append(dict(group="tiles", name="tiles_qs_n257", kind="mult", kernel="qs", bw=64, n=ST + 1, gen="gauss", seed=2300))
    # one draw from a caller's generator (the next normal drawn afterwards is recorded too)
    for kern in KERNELS:
        for bw in (1, 17):
            for n in (1, 2, WT, ST + 1):
                cs.append(dict(group="draw", name=f"draw_{kern}_bw{bw}_n{n}", kind="draw", kernel=kern, bw=bw, n=n, gen="gauss",
                               seed=3000 + bw + n, tmpl="gauss"))
    cs.append(dict(group="draw", name="draw_zero_template", kind="draw", kernel="bartlett", bw=3, n=2 * WT + 1, gen="gauss", seed=31,
                   tmpl="zero"))
    cs.append(dict(group="draw", name="draw_const_template", kind="draw", kernel="bartlett", bw=3, n=WT + 1, gen="gauss", seed=32,
                   tmpl="const"))
    # apply alone: n = 0, constant and NaN-free multipliers of any kind
    for n in (0, 1, WT + 1, 300):
        cs.append(dict(group="apply", name=f"apply_n{n}", kind="apply", n=n, seed=4000 + n, tmpl="gauss"))
    cs.append(dict(group="apply", name="apply_zero_template", kind="apply", n=70, seed=41, tmpl="zero"))
    cs.append(dict(group="apply", name="apply_ones", kind="apply", n=70, seed=42, tmpl="gauss", ones=True))
    return cs


def template(case):
    n, rng = case["n"], np.random.default_rng(case["seed"] + 500000)
    if case["tmpl"] == "zero":
        return np.zeros(n)
    if case["tmpl"] == "const":
        return np.full(n, 2.5)
    return rng.normal(0.0, 1.0, n) * np.exp(rng.normal(0.0, 1.0, n))


def noise(case):
    n = case["n"] + 2 * _max_lag(case["bw"], case["kernel"])
    rng = np.random.default_rng(case["seed"])
    z = rng.standard_normal(n)
    if case["gen"] == "const":
        z[:] = 0.75
    elif case["gen"] == "zero":
        z[:] = 0.0
    elif case["gen"] == "nan":
        z[n // 2] = np.nan
    return z


def run_case(mod, case):
    """The callable of `mod` the case names, on the case's inputs -> dict of arrays."""
    if case["kind"] == "mult":
        out = mod.cGenerateDWBMultipliersFromNoise(noise(case), case["bw"], case["kernel"])
        extra = np.zeros(0)
    elif case["kind"] == "apply":
        rng = np.random.default_rng(case["seed"])
        mult = np.ones(case["n"]) if case.get("ones") else rng.normal(0.0, 1.0, case["n"])
        out = mod.cApplyStationaryNullDWB(template(case), mult)
        extra = np.zeros(0)
    else:
        rng = np.random.default_rng(case["seed"])
        out = mod.cStationaryNullDWBDraw(template(case), case["bw"], rng, case["kernel"])
        extra = np.asarray([rng.standard_normal()], np.float64)     # where the call left the caller's generator
    out = np.asarray(out)
    assert out.dtype == np.float64 and out.shape == (case["n"],)
    return dict(out=out, next=extra)


def same(a, b):
    return all(np.array_equal(np.asarray(a[k], np.float64).view(np.uint64), np.asarray(b[k], np.float64).view(np.uint64))
               for k in ("out", "next"))


def load_group(path):
    """{case name: result} of one dwb_<group>.npz."""
    out = {}
    with np.load(path) as z:
        for key in z.files:
            name, field = key.rsplit("/", 1)
            out.setdefault(name, {})[field] = z[key]
    return out
