"""Pure-Python twin of the state-shrinkage passes (test infrastructure), in two forms.

`SequentialPasses` restates the reference's natives step by step: per bin the same IEEE operations in the same order, `log` and
`exp` from the C library (`math.log` / `math.exp`, element by element -- NumPy's vectorised ones are not guaranteed to round like
them), every sum added bin after bin (np.cumsum adds in order).  It is bit-equal to the compiled reference;
tests/golden/make_shrink_golden.py writes no fixture otherwise.

`TreePasses` adds the same terms in the device's decomposition (csrc/csr_shrink.h): an invalid bin and a bin past the chain's end
add +0.0, the 64 lanes of a wavefront are halved six times, the four wavefronts of a 256-bin tile are added in order, the tiles
of a chain are added in order.  It also returns the sums of |terms|, which the per-pass gate is relative to.

Both are pass evaluators in the sense of consenrich_amd/shrink.py."""
from __future__ import annotations

import math

import numpy as np

TILE, WAVE = 256, 64
FLOOR = 1.0e-12
TWO_PI = 2.0 * 3.14159265358979323846


def _log(a):
    return np.array(list(map(math.log, a.tolist())), dtype=np.float64).reshape(a.shape)


def _exp(a):
    return np.array(list(map(math.exp, a.tolist())), dtype=np.float64).reshape(a.shape)


def valid_mask(x, v):
    with np.errstate(invalid="ignore"):
        return np.isfinite(x) & np.isfinite(v) & (v > 0.0)


def block_weights(valid, block):
    """1 / (valid bins of the bin's block) for every bin of one chunk (anything where the block has none)."""
    n = valid.shape[0]
    blk = np.arange(n) // int(block)
    counts = np.bincount(blk, weights=valid.astype(np.float64), minlength=(n + block - 1) // block if n else 0)
    with np.errstate(divide="ignore"):
        return (1.0 / counts)[blk] if n else np.zeros(0)


def _mixture(x, v, pi0, tau, lsp):
    """Per valid bin: (e0, e[K], denom, maxLog) with e = exp(log term - maxLog), as the natives form them."""
    x2 = x * x
    log_null = math.log(pi0) - 0.5 * (_log(TWO_PI * v) + x2 / v)
    logs = []
    max_log = log_null.copy()
    for j in range(tau.shape[0]):
        vt = v + tau[j]
        lv = lsp[j] - 0.5 * (_log(TWO_PI * vt) + x2 / vt)
        logs.append(lv)
        max_log = np.where(lv > max_log, lv, max_log)
    e0 = _exp(log_null - max_log)
    denom = e0.copy()
    es = []
    for lv in logs:
        e = _exp(lv - max_log)
        es.append(e)
        denom = denom + e
    return e0, es, denom, max_log


def initial_terms(x, v, null_z, block):
    """The terms of `cstateShrinkInitialSums` of one chunk over ALL bins (zero where invalid): [5][n]."""
    x, v = np.asarray(x, dtype=np.float64), np.asarray(v, dtype=np.float64)
    ok = valid_mask(x, v)
    w = block_weights(ok, block)
    out = np.zeros((5, x.shape[0]), dtype=np.float64)
    xs, vs, ws = x[ok], np.maximum(v[ok], FLOOR), w[ok]
    z = np.abs(xs) / np.sqrt(vs)
    out[0, ok] = ws
    out[1, ok] = np.where(z <= (null_z if null_z > FLOOR else FLOOR), ws, 0.0)
    out[2, ok] = ws * (xs * xs - vs)
    out[3, ok] = ws * vs
    out[4, ok] = 1.0
    return out, ok


def em_terms(x, v, pi0, tau, lsp, block):
    """The terms of `cstateShrinkMixtureEMStepPrepared` of one chunk over ALL bins: rows totalWeight, nullMass, logLikelihood,
    finiteCount, slabMass[K], slabSecond[K]."""
    x, v = np.asarray(x, dtype=np.float64), np.asarray(v, dtype=np.float64)
    tau, lsp = np.asarray(tau, dtype=np.float64), np.asarray(lsp, dtype=np.float64)
    k = tau.shape[0]
    ok = valid_mask(x, v)
    w = block_weights(ok, block)
    out = np.zeros((4 + 2 * k, x.shape[0]), dtype=np.float64)
    xs, vs, ws = x[ok], np.maximum(v[ok], FLOOR), w[ok]
    if xs.size:
        e0, es, denom, max_log = _mixture(xs, vs, pi0, tau, lsp)
        out[0, ok] = ws
        out[1, ok] = ws * (e0 / denom)
        out[2, ok] = ws * (max_log + _log(denom))
        out[3, ok] = 1.0
        for j in range(k):
            resp = es[j] / denom
            shrink = tau[j] / (tau[j] + vs)
            mean = shrink * xs
            out[4 + j, ok] = ws * resp
            out[4 + k + j, ok] = ws * resp * (shrink * vs + mean * mean)
    return out, ok


def posterior(x, v, pi0, tau, lsp, with_ratio=False):
    """`cstateShrinkMixturePosteriorPrepared`: the five float32 tracks (and postSecond / postVariance of the valid bins)."""
    x, v = np.asarray(x, dtype=np.float64).reshape(-1), np.asarray(v, dtype=np.float64).reshape(-1)
    tau, lsp = np.asarray(tau, dtype=np.float64), np.asarray(lsp, dtype=np.float64)
    ok = valid_mask(x, v)
    n = x.shape[0]
    with np.errstate(over="ignore", invalid="ignore"):
        outs = [x.astype(np.float32)] + [np.full(n, np.nan, dtype=np.float32) for _ in range(4)]
    ratio = np.zeros(0)
    xs, vs = x[ok], np.maximum(v[ok], FLOOR)
    if xs.size:
        e0, es, denom, _ = _mixture(xs, vs, pi0, tau, lsp)
        shrunk, second, weight = np.zeros_like(xs), np.zeros_like(xs), np.zeros_like(xs)
        for j in range(tau.shape[0]):
            resp = es[j] / denom
            shrink = tau[j] / (tau[j] + vs)
            mean = shrink * xs
            weight = weight + resp
            shrunk = shrunk + resp * mean
            second = second + resp * (shrink * vs + mean * mean)
        var = second - shrunk * shrunk
        var = np.where(~np.isfinite(var) | (var <= FLOOR), FLOOR, var)
        ratio = second / var
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            outs[0][ok] = shrunk.astype(np.float32)
            outs[1][ok] = np.sqrt(var).astype(np.float32)
            outs[2][ok] = (e0 / denom).astype(np.float32)
            outs[3][ok] = np.where(weight > FLOOR, shrunk / np.where(weight > FLOOR, weight, 1.0), 0.0).astype(np.float32)
            outs[4][ok] = weight.astype(np.float32)
    return (tuple(outs), ratio) if with_ratio else tuple(outs)


def sequential_sums(terms, ok):
    """Each row's valid terms added bin after bin."""
    return np.array([np.cumsum(row[ok])[-1] if np.any(ok) else 0.0 for row in terms], dtype=np.float64)


def tree_sums(terms):
    """Each row added in the device's tree (zeros where invalid and past the end)."""
    ns, n = terms.shape
    tiles = (n + TILE - 1) // TILE
    if tiles == 0:
        return np.zeros(ns)
    a = np.zeros((ns, tiles * TILE), dtype=np.float64)
    a[:, :n] = terms
    a = a.reshape(ns, tiles, TILE // WAVE, WAVE)
    d = WAVE // 2
    while d >= 1:
        a = a[..., :d] + a[..., d:2 * d]
        d //= 2
    a = a[..., 0]
    t = a[:, :, 0]
    for w in range(1, TILE // WAVE):
        t = t + a[:, :, w]
    return np.cumsum(t, axis=1)[:, -1]


def _initial_tuple(s):
    return float(s[0]), float(s[1]), float(s[2]), float(s[3]), int(s[4])


def _em_tuple(s, k):
    return float(s[0]), float(s[1]), np.array(s[4:4 + k]), np.array(s[4 + k:4 + 2 * k]), float(s[2]), int(s[3])


class _Passes:
    def __init__(self, chunks, block_size):
        self.chunks = [(np.asarray(x, dtype=np.float64).reshape(-1), np.asarray(v, dtype=np.float64).reshape(-1)) for x, v in chunks]
        self.block = int(block_size)
        self.lengths = tuple(int(x.shape[0]) for x, _ in self.chunks)
        self.passes = 0

    def initial_rows(self, null_z):
        return [self._sum(*initial_terms(x, v, null_z, self.block)) for x, v in self.chunks]

    def em_rows(self, pi0, tau, lsp):
        self.passes += 1
        return [self._sum(*em_terms(x, v, pi0, tau, lsp, self.block)) for x, v in self.chunks]

    def initial_sums(self, null_z):
        return [_initial_tuple(s) for s in self.initial_rows(null_z)]

    def em_step(self, pi0, tau, log_prior):
        k = len(tau)
        return [_em_tuple(s, k) for s in self.em_rows(pi0, tau, log_prior)]


class SequentialPasses(_Passes):
    """The reference's order of summation."""

    @staticmethod
    def _sum(terms, ok):
        return sequential_sums(terms, ok)


class TreePasses(_Passes):
    """The device's order of summation."""

    @staticmethod
    def _sum(terms, ok):
        return tree_sums(terms)

    def abs_rows(self, pi0, tau, lsp):
        """The sums of |terms| of an EM pass, chunk by chunk (what the per-pass gate is relative to)."""
        return [tree_sums(np.abs(em_terms(x, v, pi0, tau, lsp, self.block)[0])) for x, v in self.chunks]

    def abs_initial_rows(self, null_z):
        return [tree_sums(np.abs(initial_terms(x, v, null_z, self.block)[0])) for x, v in self.chunks]
