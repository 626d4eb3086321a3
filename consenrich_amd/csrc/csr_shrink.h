// csr_shrink.h -- the per-bin work of the post-fit empirical-Bayes state shrinkage (spike-and-slab prior, the reference's
// `cstateShrinkInitialSums`, `cstateShrinkMixtureEMStepPrepared` and `cstateShrinkMixturePosteriorPrepared`, pyx:9783-10269).
//
// Inputs go through ShrinkTrack: float64 arrays (the host-array drop-ins; the reference casts whatever it is given to float64),
// or the resident fit -- the state as float32 `stride` apart ((double) xs[:,0] of the reference layout) and a float32 variance
// track that k_shrink_prep makes.  A bin is valid iff isfinite(x) && isfinite(v) && v > 0; a valid variance at or below 1e-12
// counts as 1e-12.  Each chain is cut into blocks of `block` bins from its first bin; a valid bin weighs 1 / (valid bins of its
// block).
//
//   k_shrink_prep     one lane per bin: the variance track of a resident chain -- the float32 square root of Ps00 squared and
//                     floored at 1e-12 in float32, or the square of an uploaded float32 uncertainty, floored the same way -- and
//                     the valid count of the bin's block (an INTEGER atomic: the counts do not depend on the order).
//   k_shrink_initial  } one lane per bin, SHRINK_TILE bins per workgroup.  Per bin the reference's expressions as written
//   k_shrink_em       } (logPrior - 0.5 * (log(2 pi (v + tau)) + x^2 / (v + tau)), the running maximum from the null term,
//                     exp(. - maxLog)); -ffp-contract=off, IEEE division and square root.  Up to SHRINK_REG_K slabs a lane keeps
//                     the K exponentials in registers; above that it recomputes them where they are read again -- the same
//                     operations on the same operands, hence the same bits.
//   k_shrink_fold     one lane per quantity: a chain's tile partials added in tile order.
//   k_shrink_post     one lane per bin: the five float32 posterior tracks.
//
// Summation order, which is what the results are a function of: an invalid lane and a lane past the chain's end add +0.0; the 64
// lanes of a wavefront are halved six times (lane i += lane i + d, d = 32 .. 1), the four wavefronts of a tile are added in
// order, the tiles of a chain are added in order.  No float atomics: the same call returns the same bits.  tests/twin_shrink.py
// restates this tree.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace csr {

constexpr int SHRINK_TILE = 256;            // bins per workgroup = threads per workgroup
constexpr int SHRINK_WAVES = SHRINK_TILE / 64;
constexpr int SHRINK_MAX_K = 96;            // the quadrature order's upper bound
constexpr int SHRINK_REG_K = 16;            // up to here the slab terms of a bin stay in registers
constexpr int SHRINK_INIT_NS = 5;           // totalWeight, centralWeight, excessMomentSum, varianceSum, finiteCount
constexpr int SHRINK_EM_HEAD = 4;           // totalWeight, nullMass, logLikelihood, finiteCount; then slabMass[K], slabSecond[K]
constexpr double SHRINK_FLOOR = 1.0e-12;
constexpr double SHRINK_TWO_PI = 2.0 * 3.14159265358979323846;

struct ShrinkTrack {
    const double *xd, *vd;          // float64 state / variance, or
    const float *xf, *vf;           // float32 state `stride` apart and float32 variance
    int64_t stride;
    __device__ __forceinline__ double x(int64_t i) const { return xd ? xd[i] : (double)xf[i * stride]; }
    __device__ __forceinline__ double v(int64_t i) const { return vd ? vd[i] : (double)vf[i]; }
};
struct ShrinkChain {
    int64_t off, n;                 // the chain's first element in the tracks / outputs, its bins
    int64_t blk0, tile0;            // its first block count, its first tile partial
};
struct ShrinkPrior {                // one parameter set
    double logNullPrior;            // log(pi0)
    int32_t K, reserved;
    double tau[SHRINK_MAX_K], logPrior[SHRINK_MAX_K];
};

__device__ __forceinline__ bool shrink_valid(double x, double v) { return isfinite(x) && isfinite(v) && v > 0.0; }

// resident variance sources of k_shrink_prep
enum : int { SHRINK_VAR_GIVEN = 0, SHRINK_VAR_FIT = 1, SHRINK_VAR_UNCERTAINTY = 2 };
struct ShrinkPrepArgs {
    ShrinkTrack tr;
    const ShrinkChain *chains;
    const float *Ps;                // SHRINK_VAR_FIT: reference layout, psStride floats per bin
    const float *unc;               // SHRINK_VAR_UNCERTAINTY: float32 uncertainty, laid out like the variance track
    float *var;                     // the variance track to write (resident sources)
    int64_t psStride, block;
    int32_t source, reserved;
    int32_t *counts;
};
// grid (ceil(longest / 256), chains); counts zeroed by the caller
__global__ __launch_bounds__(SHRINK_TILE) void k_shrink_prep(ShrinkPrepArgs a) {
    const ShrinkChain ch = a.chains[blockIdx.y];
    const int64_t i = (int64_t)blockIdx.x * SHRINK_TILE + threadIdx.x;
    if (i >= ch.n) return;
    double v;
    if (a.source == SHRINK_VAR_GIVEN) v = a.tr.v(ch.off + i);
    else {
        float u;
        if (a.source == SHRINK_VAR_FIT) u = (float)__dsqrt_rn((double)a.Ps[(ch.off + i) * a.psStride]);  // correctly rounded float32 sqrt
        else u = a.unc[ch.off + i];
        float w = u * u;
        w = (w > 1.0e-12f || w != w) ? w : 1.0e-12f;        // np.maximum: a NaN stays
        a.var[ch.off + i] = w;
        v = (double)w;
    }
    if (shrink_valid(a.tr.x(ch.off + i), v)) atomicAdd(&a.counts[ch.blk0 + i / a.block], 1);
}

__device__ __forceinline__ double shrink_wave_sum(double v) {
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
    return v;
}
// quantity q of this lane's bin: reduced over the wavefront, lane 0 leaves it in the tile's LDS table [wave][ns]
__device__ __forceinline__ void shrink_put(double *sm, int ns, int q, double val) {
    const double s = shrink_wave_sum(val);
    if ((threadIdx.x & 63) == 0) sm[(threadIdx.x >> 6) * ns + q] = s;
}
// after every quantity is in: the tile's partials, the wavefronts added in order
__device__ __forceinline__ void shrink_store_tile(const double *sm, int ns, double *__restrict__ dst) {
    __syncthreads();
    for (int q = threadIdx.x; q < ns; q += SHRINK_TILE) {
        double s = sm[q];
        for (int w = 1; w < SHRINK_WAVES; ++w) s += sm[w * ns + q];
        dst[q] = s;
    }
}

struct ShrinkSumArgs {
    ShrinkTrack tr;
    const ShrinkChain *chains;
    const int32_t *counts;
    int64_t block;
    double nullZSafe;               // initial sums: max(nullZ, 1e-12)
    double *partial;                // [tile][ns]
};

// grid (ceil(longest / SHRINK_TILE), chains)
__global__ __launch_bounds__(SHRINK_TILE) void k_shrink_initial(ShrinkSumArgs a) {
    __shared__ double sm[SHRINK_WAVES * SHRINK_INIT_NS];
    const ShrinkChain ch = a.chains[blockIdx.y];
    const int64_t i = (int64_t)blockIdx.x * SHRINK_TILE + threadIdx.x;
    if ((int64_t)blockIdx.x * SHRINK_TILE >= ch.n) return;          // (the whole workgroup)
    double tw = 0.0, cw = 0.0, em = 0.0, vs = 0.0, fc = 0.0;
    if (i < ch.n) {
        const double x = a.tr.x(ch.off + i);
        double v = a.tr.v(ch.off + i);
        if (shrink_valid(x, v)) {
            const double weight = 1.0 / (double)a.counts[ch.blk0 + i / a.block];
            if (v <= SHRINK_FLOOR) v = SHRINK_FLOOR;
            const double x2 = x * x;
            const double z = fabs(x) / sqrt(v);
            tw = weight;
            if (z <= a.nullZSafe) cw = weight;
            em = weight * (x2 - v);
            vs = weight * v;
            fc = 1.0;
        }
    }
    shrink_put(sm, SHRINK_INIT_NS, 0, tw);
    shrink_put(sm, SHRINK_INIT_NS, 1, cw);
    shrink_put(sm, SHRINK_INIT_NS, 2, em);
    shrink_put(sm, SHRINK_INIT_NS, 3, vs);
    shrink_put(sm, SHRINK_INIT_NS, 4, fc);
    shrink_store_tile(sm, SHRINK_INIT_NS, a.partial + (ch.tile0 + blockIdx.x) * SHRINK_INIT_NS);
}

// the slab term of a bin: logPrior_j - 0.5 * (log(2 pi (v + tau_j)) + x^2 / (v + tau_j))
__device__ __forceinline__ double shrink_log_slab(const ShrinkPrior &p, int j, double v, double x2) {
    const double vPlusTau = v + p.tau[j];
    return p.logPrior[j] - 0.5 * (log(SHRINK_TWO_PI * vPlusTau) + x2 / vPlusTau);
}

// What a valid bin's mixture looks like: the null term, the maximum and the denominator.  REG: e[j] = exp(log_j - maxLog) of every
// slab is left in registers; otherwise shrink_resp recomputes it.
template <bool REG>
struct ShrinkBin {
    double logNull, maxLog, denomSum, nullExp;
    double e[REG ? SHRINK_REG_K : 1];
    __device__ __forceinline__ void eval(const ShrinkPrior &p, double x, double v, double x2) {
        logNull = p.logNullPrior - 0.5 * (log(SHRINK_TWO_PI * v) + x2 / v);
        maxLog = logNull;
        if (REG) {
#pragma unroll
            for (int j = 0; j < SHRINK_REG_K; ++j)
                if (j < p.K) {
                    e[j] = shrink_log_slab(p, j, v, x2);
                    if (e[j] > maxLog) maxLog = e[j];
                }
        } else {
            for (int j = 0; j < p.K; ++j) {
                const double l = shrink_log_slab(p, j, v, x2);
                if (l > maxLog) maxLog = l;
            }
        }
        nullExp = exp(logNull - maxLog);
        denomSum = nullExp;
        if (REG) {
#pragma unroll
            for (int j = 0; j < SHRINK_REG_K; ++j)
                if (j < p.K) {
                    e[j] = exp(e[j] - maxLog);
                    denomSum += e[j];
                }
        } else {
            for (int j = 0; j < p.K; ++j) denomSum += exp(shrink_log_slab(p, j, v, x2) - maxLog);
        }
    }
};

// grid (ceil(longest / SHRINK_TILE), chains); dynamic LDS: SHRINK_WAVES * (SHRINK_EM_HEAD + 2 K) doubles
template <bool REG>
__global__ __launch_bounds__(SHRINK_TILE) void k_shrink_em(ShrinkSumArgs a, const ShrinkPrior *__restrict__ prior) {
    extern __shared__ double smEm[];
    const ShrinkPrior &p = *prior;
    const int K = p.K, ns = SHRINK_EM_HEAD + 2 * K;
    const ShrinkChain ch = a.chains[blockIdx.y];
    const int64_t i = (int64_t)blockIdx.x * SHRINK_TILE + threadIdx.x;
    if ((int64_t)blockIdx.x * SHRINK_TILE >= ch.n) return;
    bool ok = false;
    double x = 0.0, v = 1.0, weight = 0.0;
    if (i < ch.n) {
        x = a.tr.x(ch.off + i);
        v = a.tr.v(ch.off + i);
        ok = shrink_valid(x, v);
        if (ok) {
            weight = 1.0 / (double)a.counts[ch.blk0 + i / a.block];
            if (v <= SHRINK_FLOOR) v = SHRINK_FLOOR;
        } else {
            x = 0.0;
            v = 1.0;
        }
    }
    const double x2 = x * x;
    ShrinkBin<REG> b;
    b.eval(p, x, v, x2);            // (an invalid lane evaluates a harmless bin and contributes +0.0 below)
    const double logDenom = b.maxLog + log(b.denomSum);
    shrink_put(smEm, ns, 0, ok ? weight : 0.0);
    shrink_put(smEm, ns, 1, ok ? weight * (b.nullExp / b.denomSum) : 0.0);
    shrink_put(smEm, ns, 2, ok ? weight * logDenom : 0.0);
    shrink_put(smEm, ns, 3, ok ? 1.0 : 0.0);
    auto slab = [&](int j, double ej) {
        const double resp = ej / b.denomSum;
        const double tau2 = p.tau[j];
        const double slabShrinkage = tau2 / (tau2 + v);
        const double slabMean = slabShrinkage * x;
        const double slabPosteriorVariance = slabShrinkage * v;
        shrink_put(smEm, ns, SHRINK_EM_HEAD + j, ok ? weight * resp : 0.0);
        shrink_put(smEm, ns, SHRINK_EM_HEAD + K + j, ok ? weight * resp * (slabPosteriorVariance + slabMean * slabMean) : 0.0);
    };
    if (REG) {
#pragma unroll
        for (int j = 0; j < SHRINK_REG_K; ++j)
            if (j < K) slab(j, b.e[j]);
    } else {
        for (int j = 0; j < K; ++j) slab(j, exp(shrink_log_slab(p, j, v, x2) - b.maxLog));
    }
    shrink_store_tile(smEm, ns, a.partial + (ch.tile0 + blockIdx.x) * ns);
}

// grid (chains), 256 threads: out[chain][q] = the chain's tile partials of quantity q added in tile order
__global__ __launch_bounds__(256) void k_shrink_fold(const ShrinkChain *__restrict__ chains, const double *__restrict__ partial, int ns,
                                                     double *__restrict__ out) {
    const ShrinkChain ch = chains[blockIdx.x];
    const int64_t tiles = (ch.n + SHRINK_TILE - 1) / SHRINK_TILE;
    for (int q = threadIdx.x; q < ns; q += 256) {
        double s = 0.0;
        for (int64_t t = 0; t < tiles; ++t) s += partial[(ch.tile0 + t) * ns + q];
        out[(int64_t)blockIdx.x * ns + q] = s;
    }
}

struct ShrinkPostArgs {
    ShrinkTrack tr;
    const ShrinkChain *chains;
    float *shrunk, *sd, *spike;     // chain i's bins at chains[i].off
    float *slabMean, *slabWeight;   // or both nullptr
};
// grid (ceil(longest / SHRINK_TILE), chains)
template <bool REG>
__global__ __launch_bounds__(SHRINK_TILE) void k_shrink_post(ShrinkPostArgs a, const ShrinkPrior *__restrict__ prior) {
    const ShrinkPrior &p = *prior;
    const ShrinkChain ch = a.chains[blockIdx.y];
    const int64_t i = (int64_t)blockIdx.x * SHRINK_TILE + threadIdx.x;
    if (i >= ch.n) return;
    const int64_t at = ch.off + i;
    const double x = a.tr.x(at);
    double v = a.tr.v(at);
    if (!shrink_valid(x, v)) {
        const float nanf_ = __int_as_float(0x7fc00000);
        a.shrunk[at] = (float)x;
        a.sd[at] = nanf_;
        a.spike[at] = nanf_;
        if (a.slabMean) {
            a.slabMean[at] = nanf_;
            a.slabWeight[at] = nanf_;
        }
        return;
    }
    if (v <= SHRINK_FLOOR) v = SHRINK_FLOOR;
    const double x2 = x * x;
    ShrinkBin<REG> b;
    b.eval(p, x, v, x2);
    const double nullProb = b.nullExp / b.denomSum;
    double shrunk = 0.0, postSecond = 0.0, slabPosteriorWeight = 0.0;
    auto slab = [&](int j, double ej) {
        const double resp = ej / b.denomSum;
        const double tau2 = p.tau[j];
        const double slabShrinkage = tau2 / (tau2 + v);
        const double slabMean = slabShrinkage * x;
        const double slabPosteriorVariance = slabShrinkage * v;
        slabPosteriorWeight += resp;
        shrunk += resp * slabMean;
        postSecond += resp * (slabPosteriorVariance + slabMean * slabMean);
    };
    if (REG) {
#pragma unroll
        for (int j = 0; j < SHRINK_REG_K; ++j)
            if (j < p.K) slab(j, b.e[j]);
    } else {
        for (int j = 0; j < p.K; ++j) slab(j, exp(shrink_log_slab(p, j, v, x2) - b.maxLog));
    }
    double postVariance = postSecond - shrunk * shrunk;
    if (!isfinite(postVariance) || postVariance <= SHRINK_FLOOR) postVariance = SHRINK_FLOOR;
    a.shrunk[at] = (float)shrunk;
    a.sd[at] = (float)sqrt(postVariance);
    a.spike[at] = (float)nullProb;
    if (a.slabMean) {
        a.slabMean[at] = slabPosteriorWeight > SHRINK_FLOOR ? (float)(shrunk / slabPosteriorWeight) : 0.0f;
        a.slabWeight[at] = (float)slabPosteriorWeight;
    }
}

// The four medians of the apply step are order statistics over the VALID bins, so they depend on the values alone: k_shrink_keys
// writes, per bin, the key of each median -- |state|, |shrunk|, spike probability, posterior sd -- or +inf for an invalid bin, so
// that after a sort the valid ones are the first finiteCount keys of a row.
struct ShrinkKeyArgs {
    ShrinkTrack tr;
    ShrinkChain ch;
    const float *shrunk, *sd, *spike;
    double *keys;                   // [4][n]
};
// grid (ceil(n / 256)): the four key rows of one chain
__global__ __launch_bounds__(256) void k_shrink_keys(ShrinkKeyArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.ch.n) return;
    const int64_t at = a.ch.off + i;
    const double x = a.tr.x(at);
    const bool ok = shrink_valid(x, a.tr.v(at));
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    a.keys[0 * a.ch.n + i] = ok ? fabs(x) : inf;
    a.keys[1 * a.ch.n + i] = ok ? (double)fabsf(a.shrunk[at]) : inf;
    a.keys[2 * a.ch.n + i] = ok ? (double)a.spike[at] : inf;
    a.keys[3 * a.ch.n + i] = ok ? (double)a.sd[at] : inf;
}

}  // namespace csr
