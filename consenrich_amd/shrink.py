"""Post-fit empirical-Bayes shrinkage of the state track on the device: drop-ins for the reference's five natives
(`cstateShrinkInitialSums`, `cstateShrinkMixtureEMStep[Prepared]`, `cstateShrinkMixturePosterior[Prepared]`, pyx:9791-10269) and
for the three functions around them (`fitStateShrinkagePrior`, `applyStateShrinkagePrior`, `shrinkStateEB`,
shrinkState.py:465-1155).

What runs where.  Every per-bin pass -- the block-weighted initial sums, the E-step sums of an EM pass and the posterior tracks --
is a kernel of csrc/csr_shrink.h.  Everything that is decided from those sums is scalar work and stays here, in plain Python: the
initial spike probability and scale, the slabs, the M-step, the sort of the slabs, the floors, the Student-t objective test with
its back-tracking trials, both stop rules, the iteration counter and the metadata.  The EM loop calls a PASS EVALUATOR, an object
with

    lengths                         the bins of every chunk
    initial_sums(null_z)            -> one (totalWeight, centralWeight, excessMomentSum, varianceSum, finiteCount) per chunk
    em_step(pi0, tau, log_prior)    -> one (totalWeight, nullMass, slabMass[K], slabSecond[K], logLikelihood, finiteCount) per chunk

and adds the chunk sums in chunk order, as the reference does.  `HostArrayPasses` evaluates on the device from host arrays,
`DeviceBatch.shrink_fit` from the resident fit; the tests inject a CPU twin, with which this loop reproduces the reference's
priors bit for bit.  There is no CPU fallback in the product.

Numerics.  The device adds float64 terms in a fixed tree (lanes, wavefronts, tiles, chains), the reference adds them one after
the other, and the two `log` / `exp` differ in the last place: sums agree to ~1e-15 relative, not bit for bit; a fit's iteration
count and parameters agree as far as the fit is stable against such noise (the adaptive mixture re-sorts its slabs in the M-step
and is, on some inputs, not: see README).  The same call returns the same bits every time.

SciPy is imported only where it is needed: `roots_genlaguerre` for the Student-t slabs unless the caller passes
`quadrature=(nodes, weights)`, `expit` for a spike odds multiplier other than 1.  The kernels take 1 to 96 slabs (the reference's
quadrature order ends there); the natives' drop-ins answer more with a ValueError.
"""
from __future__ import annotations

import ctypes as C
import math
from collections.abc import Mapping
from typing import Any, NamedTuple

import numpy as np

from . import _lib as L
from ._lib import _c_int

MODEL_ADAPTIVE_NORMAL_MIXTURE = "adaptiveNormalMixture"
MODEL_SPIKE_AND_NORMAL = "spikeAndNormal"
MODEL_SPIKE_AND_STUDENT_T = "spikeAndStudentT"
MODELS = (MODEL_ADAPTIVE_NORMAL_MIXTURE, MODEL_SPIKE_AND_NORMAL, MODEL_SPIKE_AND_STUDENT_T)
DEFAULT_MODEL = MODEL_SPIKE_AND_STUDENT_T
FLOOR = 1.0e-12                                 # the reference's positive floor and weight floor
MIN_NULL, MAX_NULL = 1.0e-2, 1.0 - 1.0e-4
# constants.py:305-314 (the function's own default quadrature order is 12; the CLI passes 16)
SPIKE_ODDS_MULTIPLIER = 2.0
SPIKE_PSEUDO_COUNT_FRACTION, SPIKE_PSEUDO_COUNT_MIN, SPIKE_PSEUDO_COUNT_MAX = 0.1, 1.0e-6, 1.0e6
SCALE_ANCHOR_WEIGHT_FRACTION, SCALE_ANCHOR_WEIGHT_MIN = 0.05, 25.0
MIXTURE_SCALE_MULTIPLIERS = (0.25, 0.5, 1.0, 2.0, 4.0)
STUDENT_T_FLOOR_FACTOR = 4.0
BACKTRACK_TRIALS = 12


class stateShrinkPrior(NamedTuple):
    """The genome-wide prior, field for field the reference's tuple."""
    model: str
    priorSpikeProp: float
    priorScale: float
    priorVariance: float
    blockSize: int
    metadata: dict
    slabVariance: tuple = ()
    slabWeight: tuple = ()
    componentWeights: tuple = ()


class stateShrinkResult(NamedTuple):
    """What applying a prior to one state vector returns, field for field the reference's tuple."""
    shrunkState: np.ndarray
    posteriorSd: np.ndarray
    spikeProp: np.ndarray
    slabPosteriorMean: np.ndarray
    slabPosteriorWeight: np.ndarray
    priorSpikeProp: float
    priorScale: float
    metadata: dict


# ---------------------------------------------------------------------------------------------------------------
# the natives
# ---------------------------------------------------------------------------------------------------------------
def _vec64(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1), dtype=np.float64)


def _check_pi0(pi0: float) -> None:
    if not math.isfinite(pi0) or pi0 <= 0.0 or pi0 >= 1.0:
        raise ValueError("priorSpikeProp must be finite with 0 < priorSpikeProp < 1")


def _slab_pair(slabVariance, other, other_name: str):
    """The two slab arrays of a native as it checks them, up to the spike probability's check."""
    tau, oth = np.asarray(slabVariance, dtype=np.float64), np.asarray(other, dtype=np.float64)
    if tau.ndim != 1:
        raise ValueError("slabVariance must be one-dimensional")
    if oth.ndim != 1:
        raise ValueError(f"{other_name} must be one-dimensional")
    tau, oth = np.ascontiguousarray(tau), np.ascontiguousarray(oth)
    if tau.shape[0] <= 0:
        raise ValueError("slab arrays must be nonempty")
    if oth.shape[0] != tau.shape[0]:
        raise ValueError(f"slabVariance and {other_name} must have the same length")
    return tau, oth


def _check_tau(tau: np.ndarray) -> None:
    if np.any(~np.isfinite(tau) | (tau <= 0.0)):
        raise ValueError("slabVariance must contain only positive finite values")


def _check_slab_count(k: int) -> None:
    if k > L.SHRINK_MAX_SLABS:
        raise ValueError(f"slab arrays must hold 1 to {L.SHRINK_MAX_SLABS} slabs")


def _prepared_from_weights(pi0: float, slabVariance, slabWeight):
    """pyx:9862-9912 / 10071-10121: the checks of the two natives that take weights, and `logSlabPrior` as they build it (the
    weights added in order, the C library's log)."""
    tau, w = _slab_pair(slabVariance, slabWeight, "slabWeight")
    _check_pi0(pi0)
    total = 0.0
    for j in range(tau.shape[0]):
        if not math.isfinite(tau[j]) or tau[j] <= 0.0:
            raise ValueError("slabVariance must contain only positive finite values")
        if not math.isfinite(w[j]) or w[j] < 0.0:
            total = -2.0
            break
        total += float(w[j])
    if total == -2.0 or total <= 0.0 or not math.isfinite(total):
        raise ValueError("slabWeight must contain only finite nonnegative values with positive sum")
    scale = math.log(1.0 - pi0) - math.log(total)
    lsp = np.array([scale + math.log(v) if v > 0.0 else -math.inf for v in w.tolist()], dtype=np.float64)
    return tau, lsp


_staged_by = None        # the HostArrayPasses whose chunks the default context holds (None: a single native's, or nothing)


def _stage(chunks, block: int, owner=None):
    """Host arrays onto the device (default context): the chunks one after the other, and their per-block valid counts."""
    global _staged_by
    _staged_by = None
    lens = np.array([x.shape[0] for x, _ in chunks], dtype=np.int64)
    xs = np.ascontiguousarray(np.concatenate([x for x, _ in chunks])) if len(chunks) != 1 else chunks[0][0]
    vs = np.ascontiguousarray(np.concatenate([v for _, v in chunks])) if len(chunks) != 1 else chunks[0][1]
    L.require_gpu()
    L.check_value(L.lib().csr_shrink_stage(len(chunks), L._i64p(lens), L.dp(xs), L.dp(vs), int(block)))
    _staged_by = owner
    return lens


def _initial_rows(ctx, n: int, null_z: float) -> np.ndarray:
    out = np.zeros((n, 5), dtype=np.float64)
    L.check_value(L.lib().csr_shrink_initial_sums(ctx, float(null_z), L.dp(out)))
    return out


def _em_rows(ctx, n: int, pi0: float, tau: np.ndarray, lsp: np.ndarray) -> np.ndarray:
    k = int(tau.shape[0])
    out = np.zeros((n, 4 + 2 * k), dtype=np.float64)
    L.check_value(L.lib().csr_shrink_em_step(ctx, float(pi0), k, L.dp(tau), L.dp(lsp), L.dp(out)))
    return out


def _initial_tuple(row) -> tuple:
    return float(row[0]), float(row[1]), float(row[2]), float(row[3]), int(row[4])


def _em_tuple(row, k: int) -> tuple:
    return float(row[0]), float(row[1]), np.array(row[4:4 + k]), np.array(row[4 + k:4 + 2 * k]), float(row[2]), int(row[3])


def _state_variance(state, variance):
    x, v = _vec64(state), _vec64(variance)
    if v.shape[0] != x.shape[0]:
        raise ValueError("state and variance must have the same length")
    return x, v


def cstateShrinkInitialSums(state, variance, nullZ, blockSize=1):
    """pyx:9791-9852: (totalWeight, centralWeight, excessMomentSum, varianceSum, finiteCount) of one chunk."""
    nullZ, blockSize = float(nullZ), _c_int(blockSize)
    x, v = _state_variance(state, variance)
    _stage([(x, v)], blockSize if blockSize > 0 else 1)
    return _initial_tuple(_initial_rows(None, 1, nullZ)[0])


def cstateShrinkMixtureEMStepPrepared(state, variance, priorSpikeProp, slabVariance, logSlabPrior, blockSize=1):
    """pyx:9922-10062: (totalWeight, nullMass, slabMass[K], slabSecond[K], logLikelihood, finiteCount) of one chunk."""
    pi0, blockSize = float(priorSpikeProp), _c_int(blockSize)
    x, v = _state_variance(state, variance)
    tau, lsp = _slab_pair(slabVariance, logSlabPrior, "logSlabPrior")
    _check_pi0(pi0)
    _check_tau(tau)
    _check_slab_count(tau.shape[0])
    _stage([(x, v)], blockSize if blockSize > 0 else 1)
    return _em_tuple(_em_rows(None, 1, pi0, tau, lsp)[0], tau.shape[0])


def cstateShrinkMixtureEMStep(state, variance, priorSpikeProp, slabVariance, slabWeight, blockSize=1):
    """pyx:9854-9920: the EM step from slab weights."""
    pi0, blockSize = float(priorSpikeProp), _c_int(blockSize)
    tau, lsp = _prepared_from_weights(pi0, slabVariance, slabWeight)
    return cstateShrinkMixtureEMStepPrepared(state, variance, pi0, tau, lsp, blockSize)


def cstateShrinkMixturePosteriorPrepared(state, variance, priorSpikeProp, slabVariance, logSlabPrior):
    """pyx:10130-10269: (shrunk, posterior sd, spike probability, slab mean, slab weight), float32; an invalid bin returns
    float32(state) and four NaNs."""
    pi0 = float(priorSpikeProp)
    x, v = _state_variance(state, variance)
    tau, lsp = _slab_pair(slabVariance, logSlabPrior, "logSlabPrior")
    _check_pi0(pi0)
    _check_tau(tau)
    _check_slab_count(tau.shape[0])
    n = x.shape[0]
    out = np.empty((5, n), dtype=np.float32)
    if n == 0:
        L.require_gpu()
        return tuple(out[i] for i in range(5))
    _stage([(x, v)], 1)
    L.check_value(L.lib().csr_shrink_posterior(pi0, int(tau.shape[0]), L.dp(tau), L.dp(lsp), L.fp(out)))
    return tuple(np.ascontiguousarray(out[i]) for i in range(5))


def cstateShrinkMixturePosterior(state, variance, priorSpikeProp, slabVariance, slabWeight):
    """pyx:10064-10128: the posterior tracks from slab weights."""
    pi0 = float(priorSpikeProp)
    tau, lsp = _prepared_from_weights(pi0, slabVariance, slabWeight)
    return cstateShrinkMixturePosteriorPrepared(state, variance, pi0, tau, lsp)


# ---------------------------------------------------------------------------------------------------------------
# pass evaluators
# ---------------------------------------------------------------------------------------------------------------
class HostArrayPasses:
    """The passes of a fit over host arrays on the device: the chunks are staged once (with their block counts), every pass is
    two kernels and one small download.  The default context holds one staged input: if a native was called in between, the
    chunks are staged again."""

    def __init__(self, chunks, block_size: int):
        self.chunks = [(_vec64(x), _vec64(v)) for x, v in chunks]
        self.block = int(block_size)
        self.lengths = tuple(int(x.shape[0]) for x, _ in self.chunks)

    def _ensure(self) -> None:
        if _staged_by is not self:
            _stage(self.chunks, self.block, self)

    def initial_sums(self, null_z: float) -> list:
        self._ensure()
        return [_initial_tuple(r) for r in _initial_rows(None, len(self.lengths), null_z)]

    def em_step(self, pi0: float, tau, log_prior) -> list:
        self._ensure()
        tau, lsp = _vec64(tau), _vec64(log_prior)
        return [_em_tuple(r, tau.shape[0]) for r in _em_rows(None, len(self.lengths), pi0, tau, lsp)]


# ---------------------------------------------------------------------------------------------------------------
# the fit (shrinkState.py:465-970)
# ---------------------------------------------------------------------------------------------------------------
def _meta_float(value):
    value = float(value)
    return value if np.isfinite(value) else None


def normalize_model(model) -> str:
    if model is None:
        return DEFAULT_MODEL
    if str(model) in MODELS:
        return str(model)
    raise ValueError(f"Unsupported state shrinkage model {model!r}; supported values: {', '.join(MODELS)}.")


def _float_vector(name: str, values) -> np.ndarray:
    arr = np.asarray(values)
    if arr.ndim != 1:
        raise ValueError(f"`{name}` must be one-dimensional")
    if arr.size == 0:
        raise ValueError(f"`{name}` must be non-empty")
    return arr


def load_chunk(item):
    """shrinkState.py:152-171: a mapping with `state` / `variance`, or a (state, variance) pair."""
    if isinstance(item, Mapping):
        xs, vs = item.get("state"), item.get("variance")
        if xs is None or vs is None:
            raise ValueError("state shrinkage item is missing `state`/`variance`")
    else:
        try:
            xs, vs = item
        except Exception as exc:
            raise TypeError("state shrinkage chunks must be mappings or (state, variance) pairs") from exc
    state, variance = _float_vector("state", xs), _float_vector("stateVariance", vs)
    if state.shape != variance.shape:
        raise ValueError("`state` and `stateVariance` must have the same length")
    return state, variance


def _null_bounds(min_null, max_null):
    lo, hi = float(np.clip(min_null, MIN_NULL, 0.5)), float(np.clip(max_null, 0.5, MAX_NULL))
    if lo >= hi:
        raise ValueError("`minNull` must be smaller than `maxNull`")
    return lo, hi


def sorted_positive_weights(slab_variance, slab_weight):
    """shrinkState.py:188-208: slabs in ascending (stable) order of variance, floored, the weights renormalised."""
    variance = np.asarray(slab_variance, dtype=np.float64).reshape(-1)
    weight = np.asarray(slab_weight, dtype=np.float64).reshape(-1)
    if variance.size == 0:
        raise ValueError("state shrinkage slabs must be non-empty one-dimensional arrays")
    if variance.shape != weight.shape:
        raise ValueError("state shrinkage slab variance and weight shapes differ")
    if np.any(~np.isfinite(variance)) or np.any(variance <= 0.0):
        raise ValueError("state shrinkage slab variances must be finite and positive")
    if np.any(~np.isfinite(weight)) or np.any(weight <= 0.0):
        raise ValueError("state shrinkage slab weights must be finite and positive")
    order = np.argsort(variance, kind="mergesort")
    variance = np.maximum(variance[order], FLOOR)
    weight = np.maximum(weight[order], FLOOR)
    return variance, weight / float(np.sum(weight))


_DF_TEXT = "`studentTDF` must be numeric with 1 <= studentTDF <= 30"
_ORDER_TEXT = "`studentTQuadratureOrder` must be an integer with 8 <= order <= 96"


def _student_t_df(value) -> float:
    if isinstance(value, bool):
        raise ValueError(_DF_TEXT)
    try:
        df = float(value)
    except (TypeError, ValueError) as exc:
        raise ValueError(_DF_TEXT) from exc
    if not np.isfinite(df) or df < 1.0 or df > 30.0:
        raise ValueError(_DF_TEXT)
    return df


def _quadrature_order(value) -> int:
    if isinstance(value, bool):
        raise ValueError(_ORDER_TEXT)
    try:
        as_float = float(value)
    except (TypeError, ValueError) as exc:
        raise ValueError(_ORDER_TEXT) from exc
    if not np.isfinite(as_float) or not as_float.is_integer() or not 8 <= int(as_float) <= 96:
        raise ValueError(_ORDER_TEXT)
    return int(as_float)


def _nonnegative(name: str, value) -> float:
    text = f"`{name}` must be nonnegative"
    if isinstance(value, bool):
        raise ValueError(text)
    try:
        out = float(value)
    except (TypeError, ValueError) as exc:
        raise ValueError(text) from exc
    if not np.isfinite(out) or out < 0.0:
        raise ValueError(text)
    return out


def laguerre_rule(order: int, alpha: float):
    """The generalised Gauss-Laguerre rule the Student-t slabs are built from (SciPy, imported here)."""
    from scipy import special

    return special.roots_genlaguerre(order, alpha)


def student_t_slabs(prior_scale, df, order, min_slab_variance, quadrature=None):
    """shrinkState.py:271-312: (slab variances, weights, multipliers, Student-t scale, alpha, order).  quadrature: the (nodes,
    weights) of the rule of this order and alpha = df / 2 - 1 as data, instead of SciPy."""
    scale = float(prior_scale)
    if not np.isfinite(scale) or scale <= 0.0:
        raise ValueError("`priorScale` must be finite and positive")
    df, order = _student_t_df(df), _quadrature_order(order)
    alpha = df / 2.0 - 1.0
    nodes, weights = laguerre_rule(order, alpha) if quadrature is None else quadrature
    nodes = np.asarray(nodes, dtype=np.float64).reshape(-1)
    weights = np.asarray(weights, dtype=np.float64).reshape(-1)
    if (nodes.size != order or weights.size != order or np.any(~np.isfinite(nodes)) or np.any(~np.isfinite(weights))
            or np.any(nodes <= 0.0) or np.any(weights <= 0.0)):
        raise ValueError("Student-t quadrature produced invalid nodes or weights")
    if df > 2.0:
        multiplier = (df - 2.0) / (2.0 * nodes)
        t_scale = scale * math.sqrt((df - 2.0) / df)
    else:
        multiplier = df / (2.0 * nodes)
        t_scale = scale
    variance = np.maximum(scale * scale * multiplier, max(float(min_slab_variance), FLOOR))
    weight = weights / float(np.sum(weights))
    order_index = np.argsort(variance, kind="mergesort")
    variance, weight, multiplier = variance[order_index], weight[order_index], multiplier[order_index]
    weight = np.maximum(weight, FLOOR)
    return variance, weight / float(np.sum(weight)), multiplier, t_scale, alpha, order


def _student_t_prior_variance(slab_variance, multiplier) -> float:
    return float(np.mean(np.asarray(slab_variance, dtype=np.float64) / np.asarray(multiplier, dtype=np.float64)))


def log_slab_prior(pi0, slab_weight) -> np.ndarray:
    """shrinkState.py:356-364."""
    pi0 = float(pi0)
    if not np.isfinite(pi0) or pi0 <= 0.0 or pi0 >= 1.0:
        raise ValueError("`priorSpikeProp` must be finite and strictly between 0 and 1")
    weight = np.asarray(slab_weight, dtype=np.float64).reshape(-1)
    total = float(np.sum(weight))
    if weight.size == 0 or total <= 0.0 or not np.isfinite(total):
        raise ValueError("state shrinkage slab weights must have positive total weight")
    return np.log(weight) + (math.log(1.0 - pi0) - math.log(total))


def _component_weights(pi0, slab_weight) -> tuple:
    pi0 = float(pi0)
    return tuple([pi0] + [float((1.0 - pi0) * w) for w in slab_weight])


def _penalty(*, pi0, slab_variance, multiplier, spike_pseudo, slab_pseudo, anchor_variance, anchor_weight) -> float:
    """shrinkState.py:430-462: what the Student-t objective adds to the log likelihood."""
    penalty = 0.0
    if spike_pseudo > 0.0:
        penalty += float(spike_pseudo) * math.log(max(float(pi0), FLOOR))
    if slab_pseudo > 0.0:
        penalty += float(slab_pseudo) * math.log(max(1.0 - float(pi0), FLOOR))
    if anchor_weight > 0.0:
        if multiplier is None:
            raise ValueError("Student-t slab multipliers are missing")
        scale_variance = max(_student_t_prior_variance(slab_variance, multiplier), FLOOR)
        anchor = max(float(anchor_variance), FLOOR)
        penalty += -0.5 * float(anchor_weight) * (math.log(scale_variance) + anchor / scale_variance)
    return penalty


def fit_state_shrinkage_prior(chunks=None, *, model=None, priorSpikeProp=None, priorScale=None,
                              stateShrinkageSpikePseudoCount=None, stateShrinkageScaleAnchorWeight=None, studentTDF=1.0,
                              studentTQuadratureOrder=12, maxIter=96, tol=1.0e-5, nullZ=1.5, minNull=MIN_NULL,
                              maxNull=MAX_NULL, blockSize=1, passes=None, quadrature=None) -> stateShrinkPrior:
    """`fitStateShrinkagePrior` (shrinkState.py:465-970) with the reference's arguments, tuple and metadata.

    chunks: mappings with `state` / `variance`, or (state, variance) pairs; they are evaluated on the device from host arrays.
    passes: a pass evaluator instead (module text) -- then `chunks` is not read and `blockSize` only names the evaluator's block
    size in the result.  quadrature: (nodes, weights) of the Laguerre rule as data (see `student_t_slabs`)."""
    model_ = normalize_model(model)
    student = model_ == MODEL_SPIKE_AND_STUDENT_T
    df = _student_t_df(studentTDF)
    order = _quadrature_order(studentTQuadratureOrder)
    block = 1 if blockSize is None else int(max(1, blockSize))
    if passes is None:
        items = list(chunks if chunks is not None else [])
        if not items:
            raise ValueError("state shrinkage prior fit requires at least one chunk")
        passes = HostArrayPasses([load_chunk(item) for item in items], block)
    elif not passes.lengths:
        raise ValueError("state shrinkage prior fit requires at least one chunk")
    lo_null, hi_null = _null_bounds(minNull, maxNull)

    total_weight = central_weight = excess_sum = variance_sum = 0.0
    finite_count = 0
    for tw, cw, em, vs, fc in passes.initial_sums(float(nullZ)):
        total_weight += float(tw)
        central_weight += float(cw)
        excess_sum += float(em)
        variance_sum += float(vs)
        finite_count += int(fc)
    chunk_count, interval_count = len(passes.lengths), int(sum(passes.lengths))
    if total_weight <= 0.0 or finite_count <= 0:
        raise ValueError("state shrinkage prior fit has no finite positive-variance intervals")

    if stateShrinkageSpikePseudoCount is None:
        spike_pseudo = float(np.clip(SPIKE_PSEUDO_COUNT_FRACTION * total_weight, SPIKE_PSEUDO_COUNT_MIN, SPIKE_PSEUDO_COUNT_MAX))
    else:
        spike_pseudo = _nonnegative("stateShrinkageSpikePseudoCount", stateShrinkageSpikePseudoCount)
    slab_pseudo = 0.0
    if stateShrinkageScaleAnchorWeight is None:
        anchor_weight = max(SCALE_ANCHOR_WEIGHT_MIN, SCALE_ANCHOR_WEIGHT_FRACTION * total_weight)
    else:
        anchor_weight = _nonnegative("stateShrinkageScaleAnchorWeight", stateShrinkageScaleAnchorWeight)

    estimate_pi0 = priorSpikeProp is None
    if estimate_pi0:
        expected_central = float(math.erf(float(max(nullZ, FLOOR)) / math.sqrt(2.0)))
        if not np.isfinite(expected_central) or expected_central <= 0.0:
            pi0 = 0.8
        else:
            pi0 = (central_weight / total_weight) / expected_central
    else:
        pi0 = float(priorSpikeProp)
        if not np.isfinite(pi0) or pi0 <= 0.0 or pi0 >= 1.0:
            raise ValueError("`priorSpikeProp` must be finite and strictly between 0 and 1")
    pi0 = float(np.clip(pi0, lo_null, hi_null))

    if priorScale is None:
        moment = excess_sum / max(total_weight, FLOOR)
        if not np.isfinite(moment) or moment <= FLOOR:
            moment = variance_sum / max(total_weight, FLOOR)
        if not np.isfinite(moment) or moment <= FLOOR:
            raise ValueError("state shrinkage prior fit has no positive moment scale")
        base_scale = float(math.sqrt(moment))
        estimate_scales = True
    else:
        base_scale = float(priorScale)
        if not np.isfinite(base_scale) or base_scale <= 0.0:
            raise ValueError("`priorScale` must be finite and positive")
        estimate_scales = False
    anchor_variance = max(float(base_scale * base_scale), FLOOR)
    state_variance_anchor = max(float(variance_sum / total_weight), FLOOR)
    t_floor = max(float(STUDENT_T_FLOOR_FACTOR * state_variance_anchor), FLOOR)

    t_scale = alpha = multiplier = None
    if student:
        tau, weight, multiplier, t_scale, alpha, order = student_t_slabs(base_scale, df, order, t_floor, quadrature)
        estimate_weights = False
    else:
        multipliers = np.asarray((1.0,) if model_ == MODEL_SPIKE_AND_NORMAL else MIXTURE_SCALE_MULTIPLIERS, dtype=np.float64)
        tau = np.maximum(np.square(float(base_scale) * multipliers), FLOOR)
        weight = np.full(tau.shape, 1.0 / float(tau.size), dtype=np.float64)
        tau, weight = sorted_positive_weights(tau, weight)
        estimate_weights = tau.size > 1

    def log_likelihood_of(pi0_, tau_, weight_) -> float:
        ll = 0.0
        for sums in passes.em_step(pi0_, tau_, log_slab_prior(pi0_, weight_)):
            ll += float(sums[4])
        return ll

    def objective_of(ll, pi0_, tau_) -> float:
        return ll + _penalty(pi0=pi0_, slab_variance=tau_, multiplier=multiplier, spike_pseudo=spike_pseudo,
                             slab_pseudo=slab_pseudo, anchor_variance=anchor_variance, anchor_weight=anchor_weight)

    converged, iterations, ll = False, 0, float("nan")
    tol_, max_iter = float(max(tol, 0.0)), int(max(maxIter, 1))
    if estimate_pi0 or estimate_scales or estimate_weights:
        for iteration in range(max_iter):
            iterations = iteration + 1
            em_weight = null_mass = 0.0
            slab_mass, slab_second = np.zeros_like(weight, dtype=np.float64), np.zeros_like(tau, dtype=np.float64)
            ll = 0.0
            for sums in passes.em_step(pi0, tau, log_slab_prior(pi0, weight)):
                em_weight += float(sums[0])
                null_mass += float(sums[1])
                slab_mass += np.asarray(sums[2], dtype=np.float64)
                slab_second += np.asarray(sums[3], dtype=np.float64)
                ll += float(sums[4])
            next_pi0, next_weight, next_tau = pi0, weight.copy(), tau.copy()
            if estimate_pi0 and em_weight > 0.0:
                next_pi0 = float(np.clip((null_mass + spike_pseudo) / (float(em_weight) + spike_pseudo + slab_pseudo),
                                         lo_null, hi_null))
            if estimate_weights:
                mass_total = float(np.sum(slab_mass))
                if mass_total > FLOOR:
                    next_weight = np.maximum(slab_mass / mass_total, FLOOR)
                    next_weight = next_weight / float(np.sum(next_weight))
            if estimate_scales:
                if student:
                    mass_total = float(np.sum(slab_mass))
                    if mass_total + anchor_weight > FLOOR:
                        moment_sum = float(np.sum(slab_second / multiplier))
                        next_variance = float((moment_sum + anchor_weight * anchor_variance) / (mass_total + anchor_weight))
                        next_variance = max(next_variance, FLOOR)
                        next_tau = np.maximum(next_variance * multiplier, t_floor)
                else:
                    active = slab_mass > FLOOR
                    next_tau[active] = slab_second[active] / slab_mass[active]
                    next_tau = np.maximum(next_tau, FLOOR)
                    bad = ~np.isfinite(next_tau)
                    next_tau[bad] = tau[bad]
            if not student:
                next_tau, next_weight = sorted_positive_weights(next_tau, next_weight)
            else:
                objective = objective_of(ll, pi0, tau)
                next_ll = log_likelihood_of(next_pi0, next_tau, next_weight)
                if objective_of(next_ll, next_pi0, next_tau) < objective - max(tol_, 1.0e-12):
                    accepted = False
                    if estimate_scales:
                        log_anchor = math.log(max(_student_t_prior_variance(tau, multiplier), FLOOR))
                        log_proposed = math.log(max(_student_t_prior_variance(next_tau, multiplier), FLOOR))
                        for step in range(BACKTRACK_TRIALS):
                            fraction = 0.5 ** float(step + 1)
                            trial_variance = math.exp(log_anchor + fraction * (log_proposed - log_anchor))
                            trial_tau = np.maximum(trial_variance * multiplier, t_floor)
                            trial_ll = log_likelihood_of(next_pi0, trial_tau, next_weight)
                            if objective_of(trial_ll, next_pi0, trial_tau) >= objective - max(tol_, 1.0e-12):
                                next_tau, next_ll, accepted = trial_tau, trial_ll, True
                                break
                    if not accepted:
                        next_pi0, next_tau, next_weight, next_ll = pi0, tau, weight, ll
                        converged = False
                ll = next_ll
            rel_pi = abs(next_pi0 - pi0) / max(abs(pi0), FLOOR)
            rel_weight = float(np.max(np.abs(next_weight - weight) / np.maximum(np.abs(weight), FLOOR)))
            rel_variance = float(np.max(np.abs(next_tau - tau) / np.maximum(np.abs(tau), FLOOR)))
            pi0, tau, weight = next_pi0, next_tau, next_weight
            if max(rel_pi, rel_weight, rel_variance) <= tol_:
                converged = True
                break
            if student and not converged and rel_pi == 0.0 and rel_weight == 0.0 and rel_variance == 0.0:
                break
    else:
        converged = True

    if student:
        scale_variance = _student_t_prior_variance(tau, multiplier)
        if not estimate_scales:
            scale_out = float(base_scale)
            defined = df > 2.0
            prior_variance = float(base_scale * base_scale) if defined else float("nan")
            t_scale = float(base_scale * math.sqrt((df - 2.0) / df)) if defined else float(base_scale)
        elif df > 2.0:
            prior_variance = scale_variance
            t_scale = math.sqrt(max(prior_variance, FLOOR) * (df - 2.0) / df)
            scale_out = float(math.sqrt(max(prior_variance, FLOOR)))
            defined = True
        else:
            prior_variance = float("nan")
            t_scale = math.sqrt(max(scale_variance, FLOOR))
            scale_out = float(t_scale)
            defined = False
    else:
        prior_variance = float(np.sum(weight * tau))
        scale_out = float(math.sqrt(max(prior_variance, FLOOR)))
        defined = True
    components = _component_weights(pi0, weight)
    metadata = {
        "model": model_,
        "slab_family": "studentTNormalScaleMixture" if student else "normalMixture",
        "has_point_mass": True,
        "scope": "genome",
        "chunk_count": int(chunk_count),
        "interval_count": int(interval_count),
        "finite_count": int(finite_count),
        "effective_block_count": _meta_float(total_weight),
        "block_size_intervals": int(block),
        "prior_spike_prop": _meta_float(pi0),
        "prior_scale": _meta_float(scale_out),
        "prior_variance": _meta_float(prior_variance),
        "prior_variance_defined": bool(defined),
        "slab_count": int(tau.size),
        "slab_variance": [float(v) for v in tau],
        "slab_weight": [float(v) for v in weight],
        "component_weights": [float(v) for v in components],
        "estimated_prior_spike_prop": bool(estimate_pi0),
        "spike_pseudo_count": _meta_float(spike_pseudo),
        "estimated_prior_scale": bool(estimate_scales),
        "estimated_slab_weights": bool(estimate_weights),
        "estimated_slab_scales": bool(estimate_scales),
        "scale_anchor_weight": _meta_float(anchor_weight),
        "state_variance_anchor": _meta_float(state_variance_anchor),
        "iterations": int(iterations),
        "converged": bool(converged),
        "log_likelihood": _meta_float(ll),
    }
    if student:
        metadata.update({
            "student_t_df": _meta_float(df),
            "student_t_scale": _meta_float(float(t_scale)),
            "student_t_quadrature_order": int(order),
            "student_t_quadrature_alpha": _meta_float(float(alpha)),
            "student_t_min_slab_variance": _meta_float(t_floor),
            "student_t_min_slab_scale": _meta_float(math.sqrt(t_floor)),
            "student_t_slab_variance_floor_factor": _meta_float(STUDENT_T_FLOOR_FACTOR),
            "slab_multiplier": [float(v) for v in multiplier],
        })
    return stateShrinkPrior(model=model_, priorSpikeProp=float(pi0), priorScale=scale_out, priorVariance=prior_variance,
                            blockSize=int(block), metadata=metadata, slabVariance=tuple(float(v) for v in tau),
                            slabWeight=tuple(float(v) for v in weight), componentWeights=components)


# ---------------------------------------------------------------------------------------------------------------
# applying a prior (shrinkState.py:992-1092)
# ---------------------------------------------------------------------------------------------------------------
_ODDS_TEXT = "`stateShrinkageSpikeOddsMultiplier` must be finite and positive"


def spike_odds_multiplier_value(value) -> float:
    if isinstance(value, (bool, np.bool_)):
        raise ValueError(_ODDS_TEXT)
    try:
        out = float(value)
    except (TypeError, ValueError) as exc:
        raise ValueError(_ODDS_TEXT) from exc
    if not np.isfinite(out) or out <= 0.0:
        raise ValueError(_ODDS_TEXT)
    return out


def effective_spike_prop(prior: stateShrinkPrior, multiplier: float) -> float:
    """The prior's spike probability with its odds multiplied (shrinkState.py:1010-1035)."""
    pi0 = float(prior.priorSpikeProp)
    if not np.isfinite(pi0) or pi0 <= 0.0 or pi0 >= 1.0:
        raise ValueError("`priorSpikeProp` must be finite and strictly between 0 and 1")
    if multiplier == 1.0:
        return pi0
    from scipy import special

    out = float(special.expit(math.log(pi0) - math.log1p(-pi0) + math.log(multiplier)))
    if not np.isfinite(out) or out <= 0.0 or out >= 1.0:
        raise ValueError("`stateShrinkageSpikeOddsMultiplier` makes effective prior spike probability invalid")
    return out


def prior_slabs(prior: stateShrinkPrior):
    if len(prior.slabVariance) and len(prior.slabWeight):
        return sorted_positive_weights(prior.slabVariance, prior.slabWeight)
    return sorted_positive_weights((prior.priorVariance,), (1.0,))


def apply_metadata(prior, *, interval_count, finite_count, multiplier, effective, tau, weight, medians) -> dict:
    """The metadata of one applied chunk (shrinkState.py:1051-1082); medians: |state| before, |state| after, spike probability,
    posterior sd over the valid bins (NaN without one)."""
    return {
        **dict(prior.metadata),
        "scope": "contig_apply",
        "has_point_mass": True,
        "interval_count": int(interval_count),
        "finite_count": int(finite_count),
        "spike_odds_multiplier": float(multiplier),
        "effective_prior_spike_prop": float(effective),
        "slab_count": int(tau.size),
        "slab_variance": [float(v) for v in tau],
        "slab_weight": [float(v) for v in weight],
        "component_weights": [float(v) for v in _component_weights(effective, weight)],
        "state_abs_median_before": _meta_float(medians[0]),
        "state_abs_median_after": _meta_float(medians[1]),
        "spike_prop_median": _meta_float(medians[2]),
        "posterior_sd_median": _meta_float(medians[3]),
    }


def apply_state_shrinkage_prior(state, stateVariance, prior: stateShrinkPrior, *,
                                stateShrinkageSpikeOddsMultiplier=SPIKE_ODDS_MULTIPLIER, posterior=None) -> stateShrinkResult:
    """`applyStateShrinkagePrior` (shrinkState.py:992-1092) for one state vector on host arrays.  posterior: what evaluates the
    posterior pass, `(state, variance, pi0, tau, log_prior) -> five float32 tracks` (default: the device)."""
    x, v = _float_vector("state", state), _float_vector("stateVariance", stateVariance)
    if x.shape != v.shape:
        raise ValueError("`state` and `stateVariance` must have the same length")
    multiplier = spike_odds_multiplier_value(stateShrinkageSpikeOddsMultiplier)
    effective = effective_spike_prop(prior, multiplier)
    tau, weight = prior_slabs(prior)
    run = cstateShrinkMixturePosteriorPrepared if posterior is None else posterior
    shrunk, sd, spike, slab_mean, slab_weight = run(x, v, float(effective), tau, log_slab_prior(effective, weight))
    valid = np.isfinite(x) & np.isfinite(v) & (v > 0.0)
    nan = float("nan")
    medians = [np.median(a[valid]) if np.any(valid) else nan for a in (np.abs(x), np.abs(shrunk), spike, sd)]
    metadata = apply_metadata(prior, interval_count=x.size, finite_count=int(np.count_nonzero(valid)), multiplier=multiplier,
                              effective=effective, tau=tau, weight=weight, medians=medians)
    return stateShrinkResult(np.asarray(shrunk, dtype=np.float32), np.asarray(sd, dtype=np.float32),
                             np.asarray(spike, dtype=np.float32), np.asarray(slab_mean, dtype=np.float32),
                             np.asarray(slab_weight, dtype=np.float32), float(prior.priorSpikeProp), float(prior.priorScale),
                             metadata)


def shrink_state_eb(state, stateVariance, *, stateShrinkageSpikeOddsMultiplier=SPIKE_ODDS_MULTIPLIER, **fit_arguments):
    """`shrinkStateEB` (shrinkState.py:1095-1155): fit on the one vector, then apply."""
    x, v = _float_vector("state", state), _float_vector("stateVariance", stateVariance)
    if x.shape != v.shape:
        raise ValueError("`state` and `stateVariance` must have the same length")
    multiplier = spike_odds_multiplier_value(stateShrinkageSpikeOddsMultiplier)
    prior = fit_state_shrinkage_prior([(x, v)], **fit_arguments)
    return apply_state_shrinkage_prior(x, v, prior, stateShrinkageSpikeOddsMultiplier=multiplier)


# the reference's names
fitStateShrinkagePrior = fit_state_shrinkage_prior
applyStateShrinkagePrior = apply_state_shrinkage_prior
shrinkStateEB = shrink_state_eb
