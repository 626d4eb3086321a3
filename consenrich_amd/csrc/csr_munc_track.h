// csr_munc_track.h -- from the seed loop's resident arrays to a finished observation-variance matrix: the per-cell work between
// `munc_seed_finish` and a finished `matrixMunc`.
//   k_munc_block_sums   the deterministic block summaries of consenrich.py:7981-8040 (valid count, sum q, sum q * predictor,
//                       sum q * evidence, sum q * q per (sample, block); non-excluded intervals per block)
//   k_munc_prior_track  `cEvalPSplineLogVarianceTrend` (pyx:5761-5894) on the trend predictor of a mean track
//   k_munc_finalize     `_finalizeMuncEBTrackLoop` (pyx:5364-5442) as `getMuncTrack` (core.py:8390-8880) calls it three times
//   k_munc_track_store  `applyBlacklistMuncFloor` (core.py:7183-7222) on the excluded cells and the clamp of consenrich.py:9107-9113
//
// Numerical contract.  The translation unit is built with -ffp-contract=off; everything but log1p (the predictor) and exp (the
// prior track) is float64 + - * /, comparisons and float32 casts, and equals the reference bit for bit.  The four sums of a block
// are np.sum of the compacted valid cells in NumPy's order (csr_np_order.h).
//
// Layout as in csr_munc.h: (m, n) arrays are row-major with `rowStride` floats between two tracks, chain c starts at chainOff[c].
//
// Block sums.  A wavefront takes one (sample, block): its lanes read consecutive intervals of the block (coalesced), the valid
// cells are compacted in index order through a ballot into the wavefront's part of the LDS (q, q * predictor, q * evidence as
// float64), and lanes 0..3 then sum one array each in NumPy's order.  A workgroup holds MUNC_BLOCK_WAVES such wavefronts.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "csr_munc.h"
#include "csr_np_order.h"

namespace csr {

constexpr int MUNC_TRACK_MAX_DEGREE = 5;
constexpr int MUNC_TRACK_MAX_BASIS = 512;
constexpr int MUNC_TRACK_MAX_KNOTS = MUNC_TRACK_MAX_BASIS + MUNC_TRACK_MAX_DEGREE + 1;
constexpr int MUNC_BLOCK_WAVES = 4;             // wavefronts (blocks of intervals) per workgroup of k_munc_block_sums
constexpr int MUNC_BLOCK_MAX = 2048;            // intervals per block at most: 3 float64 arrays of it per wavefront in the LDS
constexpr int MUNC_BLOCK_LDS_VALUES = 2048;     // float64 values per array and workgroup: MUNC_BLOCK_WAVES blocks of up to 512, or one longer

// `_muncTrendPredictor` (core.py:6309-6315): sign(x) * log1p(|x|), NaN where that is not finite
__device__ __forceinline__ double munc_trend_predictor(double x) {
    double p;
    if (x > 0.0) p = log1p(x);
    else if (x < 0.0) p = -log1p(-x);
    else p = x == 0.0 ? 0.0 : x;
    return np_finite(p) ? p : __builtin_nan("");
}

// ---------------------------------------------------------------------------------------------------------------
// block summaries
// ---------------------------------------------------------------------------------------------------------------
struct MuncBlockRec {           // = csr_munc_block_rec
    int64_t valid;
    double q, qp, qe, qq;
};
struct MuncBlockArgs {
    const float *evidence, *weight;             // (m, rowStride): seed_smooth, seed_weight
    const unsigned char *exclude;               // per interval or nullptr
    const float *mean;                          // the resident fit's xs[:,0], meanStride floats apart
    const double *mean64;                       // host arrays: the float64 mean track as given (then `mean` is not read)
    int64_t meanStride, rowStride;
    const int64_t *chainOff, *chainLen, *chainBlocks, *recOff, *inclOff;    // per taken chain
    int64_t blockLen;                           // intervals per block (the last kept block of a chain may be shorter)
    int m, waves;                               // waves: blocks per workgroup (MUNC_BLOCK_WAVES, or 1 for long blocks)
    MuncBlockRec *rec;                          // chain c: recOff[c] + sample * chainBlocks[c] + block
    int64_t *included;                          // chain c: inclOff[c] + block
};
struct MuncSquare {
    CSR_HD double operator()(double x) const { return x * x; }
};

// grid (ceil(most blocks / waves), m, taken chains), block 64 * waves
__global__ __launch_bounds__(64 * MUNC_BLOCK_WAVES) void k_munc_block_sums(const MuncBlockArgs a) {
    __shared__ double sQ[MUNC_BLOCK_LDS_VALUES], sP[MUNC_BLOCK_LDS_VALUES], sE[MUNC_BLOCK_LDS_VALUES];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int c = blockIdx.z, j = blockIdx.y;
    const int64_t b = (int64_t)blockIdx.x * a.waves + wv;
    const bool active = b < a.chainBlocks[c];
    const int64_t n = a.chainLen[c], g0 = a.chainOff[c], start = b * a.blockLen;
    const int64_t len = active ? (n - start < a.blockLen ? n - start : a.blockLen) : 0;
    const int slot = (MUNC_BLOCK_LDS_VALUES / a.waves) * wv;
    double *q = sQ + slot, *p = sP + slot, *e = sE + slot;
    int count = 0;
    int64_t allowed = 0;
    for (int64_t t = 0; t < len; t += 64) {     // (the wavefront's own loop: its lanes stay together)
        const int64_t i = t + lane;
        bool ok = false, open = false;
        double qv = 0.0, pv = 0.0, ev = 0.0;
        if (i < len) {
            const int64_t g = g0 + start + i;
            open = !(a.exclude && a.exclude[g] != 0);
            ev = (double)a.evidence[(int64_t)j * a.rowStride + g];
            qv = open ? (double)a.weight[(int64_t)j * a.rowStride + g] : 0.0;      // consenrich.py:7996
            pv = munc_trend_predictor(a.mean64 ? a.mean64[g] : (double)a.mean[g * a.meanStride]);
            ok = open && np_finite(pv) && np_finite(ev) && ev > 0.0 && np_finite(qv) && qv > 0.0;
        }
        const unsigned long long bal = __ballot(ok);
        allowed += __popcll(__ballot(open));
        if (ok) {
            const int at = count + __popcll(bal & ((1ull << lane) - 1ull));
            q[at] = qv;
            p[at] = qv * pv;
            e[at] = qv * ev;
        }
        count += __popcll(bal);
    }
    __syncthreads();
    if (!active) return;
    MuncBlockRec *r = a.rec + a.recOff[c] + (int64_t)j * a.chainBlocks[c] + b;
    if (lane == 0) {
        r->valid = count;
        r->q = np_sum_f(q, count, NpIdentity());
        if (j == 0) a.included[a.inclOff[c] + b] = allowed;
    } else if (lane == 1) {
        r->qp = np_sum_f(p, count, NpIdentity());
    } else if (lane == 2) {
        r->qe = np_sum_f(e, count, NpIdentity());
    } else if (lane == 3) {
        r->qq = np_sum_f(q, count, MuncSquare());
    }
}

// ---------------------------------------------------------------------------------------------------------------
// prior variance track
// ---------------------------------------------------------------------------------------------------------------
struct MuncPriorArgs {
    const double *predictor;                    // host arrays: the predictor track as given; nullptr: the predictor of `mean`
    const float *mean;                          // float32 mean track, meanStride floats apart
    int64_t meanStride;
    const double *knots, *beta;
    int nKnots, nBasis;
    double xMin, xMax, logFloor, logCap;
    float *out;
    const int64_t *chainOff, *chainLen;         // nullptr: one chain of n intervals at offset 0
    int64_t n;
};

// `_bsplineSpan` (pyx:5761-5784)
__device__ __forceinline__ int munc_bspline_span(const double *knots, int nBasis, int degree, double x) {
    int low = degree, high = nBasis;
    if (x <= knots[degree]) return degree;
    if (x >= knots[nBasis]) return nBasis - 1;
    while (low < high) {
        const int mid = low + ((high - low) >> 1);
        if (x < knots[mid]) high = mid;
        else if (x >= knots[mid + 1]) low = mid + 1;
        else return mid;
    }
    return nBasis - 1;
}
// `_deBoorValue` (pyx:5787-5818).  The host has checked nBasis >= DEGREE + 1 and nKnots >= nBasis + DEGREE + 1: every index below
// stays inside the two arrays
template <int DEGREE>
__device__ __forceinline__ double munc_de_boor(const double *knots, const double *beta, int nBasis, double x) {
    const int span = munc_bspline_span(knots, nBasis, DEGREE, x);
    double work[DEGREE + 1];
#pragma unroll
    for (int j = 0; j <= DEGREE; ++j) {
        int idx = span - DEGREE + j;
        idx = idx < 0 ? 0 : (idx >= nBasis ? nBasis - 1 : idx);
        work[j] = beta[idx];
    }
#pragma unroll
    for (int r = 1; r <= DEGREE; ++r) {
#pragma unroll
        for (int j = DEGREE; j >= r; --j) {
            const int idx = span - DEGREE + j;
            const double denom = knots[idx + DEGREE - r + 1] - knots[idx];
            const double alpha = denom == 0.0 ? 0.0 : (x - knots[idx]) / denom;
            work[j] = ((1.0 - alpha) * work[j - 1]) + (alpha * work[j]);
        }
    }
    return work[DEGREE];
}

// one lane per interval: grid (ceil(longest / 256), chains); knots and beta are staged in the LDS
template <int DEGREE>
__global__ __launch_bounds__(256) void k_munc_prior_track(const MuncPriorArgs a) {
    __shared__ double sK[MUNC_TRACK_MAX_KNOTS], sB[MUNC_TRACK_MAX_BASIS];
    for (int k = threadIdx.x; k < a.nKnots; k += 256) sK[k] = a.knots[k];
    for (int k = threadIdx.x; k < a.nBasis; k += 256) sB[k] = a.beta[k];
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t len = a.chainLen ? a.chainLen[blockIdx.y] : a.n;
    if (i >= len) return;
    const int64_t g = (a.chainOff ? a.chainOff[blockIdx.y] : 0) + i;
    double x = a.predictor ? a.predictor[g] : munc_trend_predictor((double)a.mean[g * a.meanStride]);
    double logOut;
    if (!np_finite(x)) {
        logOut = a.logFloor;
    } else {
        if (x < a.xMin) x = a.xMin;
        else if (x > a.xMax) x = a.xMax;
        logOut = munc_de_boor<DEGREE>(sK, sB, a.nBasis, x);
        if (!np_finite(logOut)) logOut = logOut > 0.0 ? a.logCap : a.logFloor;
    }
    if (logOut < a.logFloor) logOut = a.logFloor;
    else if (logOut > a.logCap) logOut = a.logCap;
    a.out[g] = (float)exp(logOut);
}

// ---------------------------------------------------------------------------------------------------------------
// finalisation
// ---------------------------------------------------------------------------------------------------------------
struct MuncTrackPrm {           // = csr_munc_track_prm, one per track
    double nu_local, nu_prior, posterior;       // posterior = nu_local + nu_prior, added on the host
    double factor;                              // replicate variance factor
    int32_t scale, reserved_;                   // scale: |factor - 1| > 1e-8, the prior is float32(float64(prior) * factor)
};
enum { MUNC_FLOOR_NONE = 0, MUNC_FLOOR_NATIVE = 1, MUNC_FLOOR_COERCED = 2 };
enum { MUNC_BAD_LOCAL = 0, MUNC_BAD_PRIOR = 1, MUNC_BAD_COUNT_FLOOR = 2, MUNC_BAD_KINDS = 3 };
enum { MUNC_CNT_SUPPORT = 0, MUNC_CNT_FLOOR_FINITE = 1, MUNC_CNT_FLOOR_ADDED = 2, MUNC_CNT_FLOOR_MISSING = 3, MUNC_CNT_KINDS = 4 };
struct MuncFinalArgs {
    const float *local;                         // (m, rowStride)
    const float *prior;                         // per interval (one prior track for all tracks; a track's factor scales it)
    const float *countFloor;                    // (m, rowStride) or nullptr
    float *out;                                 // (m, rowStride)
    int64_t rowStride;
    const MuncTrackPrm *prm;                    // per track
    double floorV, capV;
    int useEB;
    int floorMode;      // MUNC_FLOOR_NATIVE: NaN = missing, anything else not finite or negative is invalid (pyx:5423-5438);
                        // MUNC_FLOOR_COERCED: `_coerceMuncCountModelVarianceFloor` first (core.py:7388-7408): not finite = missing
    const int64_t *chainOff, *chainLen;         // nullptr: one chain of n intervals at offset 0
    int64_t n;
    unsigned long long *bad;                    // (chains, m, MUNC_BAD_KINDS): the lowest invalid index, ~0 if none (integer minimum)
    unsigned long long *count;                  // (chains, m, MUNC_CNT_KINDS)
};
__device__ __forceinline__ double munc_clamp(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

// one lane per cell: grid (ceil(longest / 256), m, chains).  An invalid cell only lowers its kind's index: the host raises what
// the sequential loop would have raised, and the outputs and counters of such a track are not used
__global__ __launch_bounds__(256) void k_munc_finalize(const MuncFinalArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t len = a.chainLen ? a.chainLen[blockIdx.z] : a.n;
    const int64_t slot = (int64_t)blockIdx.z * gridDim.y + blockIdx.y;
    unsigned int cnt[MUNC_CNT_KINDS] = {0u, 0u, 0u, 0u};
    if (i < len) {
        const int64_t g = (a.chainOff ? a.chainOff[blockIdx.z] : 0) + i;
        const int64_t idx = (int64_t)blockIdx.y * a.rowStride + g;
        const MuncTrackPrm prm = a.prm[blockIdx.y];
        unsigned long long *bad = a.bad + slot * MUNC_BAD_KINDS;
        double localValue = (double)a.local[idx];
        if (!np_finite(localValue) || localValue <= 0.0) atomicMin(&bad[MUNC_BAD_LOCAL], (unsigned long long)i);
        cnt[MUNC_CNT_SUPPORT] = localValue > a.floorV ? 1u : 0u;
        localValue = munc_clamp(localValue, a.floorV, a.capV);
        double outValue = localValue;
        if (a.useEB) {
            float prior32 = a.prior[g];
            if (prm.scale) prior32 = (float)((double)prior32 * prm.factor);     // core.py:8719-8722, then float32 (pyx:5472)
            double priorValue = (double)prior32;
            if (!np_finite(priorValue) || priorValue <= 0.0) atomicMin(&bad[MUNC_BAD_PRIOR], (unsigned long long)i);
            priorValue = munc_clamp(priorValue, a.floorV, a.capV);
            outValue = ((prm.nu_local * localValue) + (prm.nu_prior * priorValue)) / prm.posterior;
        }
        outValue = munc_clamp(outValue, a.floorV, a.capV);
        if (a.floorMode != MUNC_FLOOR_NONE) {
            const double cf = (double)a.countFloor[idx];
            const bool missing = a.floorMode == MUNC_FLOOR_COERCED ? !np_finite(cf) : cf != cf;
            if (!missing) {
                if (!np_finite(cf) || cf < 0.0) atomicMin(&bad[MUNC_BAD_COUNT_FLOOR], (unsigned long long)i);
                cnt[MUNC_CNT_FLOOR_FINITE] = 1u;
                outValue += cf;
                cnt[MUNC_CNT_FLOOR_ADDED] = cf > 0.0 ? 1u : 0u;
                outValue = munc_clamp(outValue, a.floorV, a.capV);
            } else {
                cnt[MUNC_CNT_FLOOR_MISSING] = 1u;
            }
        }
        a.out[idx] = (float)outValue;
    }
    __shared__ unsigned int part[MUNC_CNT_KINDS][4];
#pragma unroll
    for (int k = 0; k < MUNC_CNT_KINDS; ++k) {
        unsigned int v = cnt[k];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if ((threadIdx.x & 63) == 0) part[k][threadIdx.x >> 6] = v;
    }
    __syncthreads();
    if (threadIdx.x < MUNC_CNT_KINDS) {
        const unsigned int s = part[threadIdx.x][0] + part[threadIdx.x][1] + part[threadIdx.x][2] + part[threadIdx.x][3];
        if (s) atomicAdd(&a.count[slot * MUNC_CNT_KINDS + threadIdx.x], (unsigned long long)s);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// blacklist floor and clamp, in place
// ---------------------------------------------------------------------------------------------------------------
struct MuncStoreArgs {
    float *track;                               // (m, rowStride)
    int64_t rowStride;
    const unsigned char *exclude;               // per interval or nullptr
    const float *floors;                        // (chains, m): float32 of the track's blacklist floor; read where useFloor[chain]
    const unsigned char *useFloor;              // per chain: the chain's mask has a set byte (core.py:7203)
    float lo, hi;                               // the clamp of consenrich.py:9107-9113
    int useHi;
    const int64_t *chainOff, *chainLen;         // nullptr: one chain of n intervals at offset 0
    int64_t n;
    unsigned long long *nonFinite;              // per chain: cells that are not finite after the floor (consenrich.py:9100-9106)
    int clamp;                                  // 0: the floor alone (`applyBlacklistMuncFloor` on host arrays)
};
// one lane per cell: grid (ceil(longest / 256), m, chains)
__global__ __launch_bounds__(256) void k_munc_track_store(const MuncStoreArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t len = a.chainLen ? a.chainLen[blockIdx.z] : a.n;
    if (i >= len) return;
    const int64_t g = (a.chainOff ? a.chainOff[blockIdx.z] : 0) + i;
    const int64_t idx = (int64_t)blockIdx.y * a.rowStride + g;
    float v = a.track[idx];
    if (a.exclude && a.useFloor[blockIdx.z] && a.exclude[g] != 0) {
        const float f = a.floors[(int64_t)blockIdx.z * gridDim.y + blockIdx.y];
        v = np_finite(v) ? (f != f ? f : (v > f ? v : f)) : f;                 // np.where(isfinite, np.maximum(v, f), f)
    }
    if (a.clamp) {
        if (!np_finite(v)) atomicAdd(&a.nonFinite[blockIdx.z], 1ull);
        v = (v > a.lo || v != v) ? v : a.lo;                                   // np.maximum: a NaN stays
        if (a.useHi) v = (v < a.hi || v != v) ? v : a.hi;
    }
    a.track[idx] = v;
}

}  // namespace csr
