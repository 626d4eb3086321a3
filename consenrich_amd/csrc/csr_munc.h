// csr_munc.h -- the dense observation-variance ("munc") seed natives on the device: `cMuncObservationMomentSeedPass`
// (pyx:4843-5039, validation 4767-4840), `cMuncSmoothDenseLocalEvidence` (pyx:5577-5639) and the per-cell glue of the seed loop
// (consenrich.py:7482-7503 `_seedWorkingMunc`, 7557-7576 `_localEvidenceToTotalVariance`, 7938-7945 the response weight).
//
// Numerical contract: every output element equals the reference's bit for bit.  Nothing here calls libm: float64 + - * /,
// comparisons and float32 casts only, with IEEE division (the translation unit is built with -ffp-contract=off).
//
// Layout.  Every (m, n) array is row-major with `rowStride` floats between two tracks: n for a host array, the batch's Npad for a
// resident one, where chain c's intervals start at chainOff[c].  A launch covers `nChains` chains (blockIdx.y); a host array is one
// chain at offset 0.  Lanes of a wavefront take consecutive intervals, so every row is read coalesced.
//
// Rolling mean.  The reference keeps ONE running float64 sum per row, adding the entering and subtracting the leaving cell, so the
// value at interval i carries the rounding history of the whole row prefix.  k_munc_roll_spec cuts every row into blocks of
// MUNC_ROLL_BLOCK intervals.  A block starts from the window sum at its entry, accumulated in index order, and then walks like the
// reference; EVERY add and subtract, the entry accumulation included, is checked with the error-free TwoSum residual.  While all
// operations of a row prefix are exact, the running sum IS the real-number sum of the window's cells, and so is an exact in-order
// accumulation: a block whose residuals are all zero, behind a row prefix whose residuals are all zero, is final.  A block
// that sees a non-zero residual marks its row; k_munc_roll_fix then redoes such a row whole, one wavefront per
// row, in the reference's operation order.  DESIGN.md "Rolling mean of the local evidence".
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace csr {

constexpr int MUNC_ROLL_BLOCK = 128;    // intervals per speculative block of the rolling mean
constexpr int MUNC_REG_TRACKS = 16;     // up to this many tracks the float32-rounded (moment, rho) pair stays in registers

// mask modes of pyx:4746-4764: 0 none, 1 per interval, 2 per cell
__device__ __forceinline__ bool munc_mask_nonzero(const unsigned char *mask, int mode, int64_t maskStride, int64_t j, int64_t g) {
    return mode == 1 ? mask[g] != 0 : mask[j * maskStride + g] != 0;
}
__device__ __forceinline__ bool munc_finite(double v) { return __builtin_isfinite(v); }

struct MuncSeedArgs {
    const float *data, *munc;                   // (m, rowStride)
    const float *stateMean, *stateVar;          // per interval, meanStride / varStride floats apart (a resident fit: xs[:,0], Ps[:,0,0])
    int64_t meanStride, varStride;
    int clipVar;                                // stateVar is read as max(value, 0) in float32 (consenrich.py:7792-7795)
    const float *background, *gVariance;        // per interval or nullptr
    const float *countFloor;                    // (m, rowStride) or nullptr
    const float *omegaIn;                       // per interval or nullptr (omegaInMode 0)
    const float *rhoIn;                         // (m, rowStride) or nullptr = ones
    const unsigned char *active;                // nonzero = active
    int activeMode;
    int64_t maskStride;
    float *moment, *omegaRaw;                   // nullptr: not written
    float *rhoOut, *omegaOut, *local, *variance;
    int64_t rowStride;
    const int64_t *chainOff, *chainLen;         // nullptr: one chain of n intervals at offset 0
    int64_t n;
    int m;
    double pad, dS, dOmega, omegaMin, omegaMax, varianceFloor, varianceCap;
    int weighted;                               // useWeights and studentT
    int updateWeights;
    unsigned int *invalid;                      // set to 1 by any lane that meets an invalid active cell
};

// the floor / cap / floor cascade of pyx:5009-5018 and 5026-5035, in its order
__device__ __forceinline__ void munc_cascade(double &localValue, double &totalValue, double countValue, double floorV, double capV,
                                             bool floorFirst) {
    if (floorFirst) {
        totalValue = localValue + countValue;
        if (localValue < floorV) {
            localValue = floorV;
            totalValue = localValue + countValue;
        }
    } else {
        if (localValue < floorV) localValue = floorV;
        totalValue = localValue + countValue;
    }
    if (totalValue > capV) {
        totalValue = capV;
        localValue = totalValue - countValue;
        if (localValue < floorV) {
            localValue = floorV;
            totalValue = localValue + countValue;
        }
    }
}

// body(j) for the tracks j = 0..m-1 in order; REG: a fully unrolled loop, so that the per-track registers are indexed statically
#define MUNC_FOR_TRACKS(body)                                     \
    if (REG) {                                                    \
        _Pragma("unroll") for (int j = 0; j < MUNC_REG_TRACKS; ++j) \
            if (j < m) body(j);                                   \
    } else {                                                      \
        for (int j = 0; j < m; ++j) body(j);                      \
    }
// One lane per interval; the lane walks the tracks in order (dbar is a sequential float64 sum in j).  REG: m <= MUNC_REG_TRACKS.
template <bool REG>
__global__ __launch_bounds__(256) void k_munc_seed_pass(const MuncSeedArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t len = a.chainLen ? a.chainLen[blockIdx.y] : a.n;
    if (i >= len) return;
    const int64_t g = (a.chainOff ? a.chainOff[blockIdx.y] : 0) + i;
    const int m = a.m;
    const int64_t rs = a.rowStride;
    bool bad = false;

    float sv = a.stateVar[g * a.varStride];
    if (a.clipVar) sv = sv < 0.0f ? 0.0f : sv;      // (NaN stays NaN, like np.maximum)
    const double stateValue = (double)a.stateMean[g * a.meanStride];
    double momentVarianceBase = (double)sv;
    const double backgroundValue = a.background ? (double)a.background[g] : 0.0;
    // what the validation reads per interval; it counts only where the interval has an active cell (below)
    bool badInterval = !munc_finite(stateValue) || !munc_finite(momentVarianceBase) || !munc_finite(backgroundValue);
    if (a.gVariance) {
        const double gv = (double)a.gVariance[g];
        badInterval = badInterval || !munc_finite(gv);
        momentVarianceBase += gv;
    }
    if (momentVarianceBase < 0.0) momentVarianceBase = 0.0;
    double omegaInValue = 1.0;
    if (a.weighted && a.omegaIn) {
        omegaInValue = (double)a.omegaIn[g];
        badInterval = badInterval || !munc_finite(omegaInValue) || omegaInValue <= 0.0;
    }

    float momReg[REG ? MUNC_REG_TRACKS : 1], rhoReg[REG ? MUNC_REG_TRACKS : 1];
    double omegaValue = 1.0;
    if (a.weighted) {
        double omegaRawValue;
        if (a.updateWeights) {
            double dbar = 0.0;
            int64_t activeCount = 0;
            auto first = [&](int j) {
                const int64_t idx = (int64_t)j * rs + g;
                float mo = 0.0f, rh = 1.0f;
                if (a.activeMode == 0 || munc_mask_nonzero(a.active, a.activeMode, a.maskStride, j, g)) {
                    const double mu = (double)a.munc[idx] + a.pad;
                    const double x = (double)a.data[idx];
                    bad = bad || badInterval || !munc_finite(x) || !munc_finite(mu) || mu <= 0.0;
                    double baseVariance = mu;
                    if (baseVariance < a.varianceFloor) baseVariance = a.varianceFloor;
                    const double residual = x - backgroundValue - stateValue;
                    const double momentValue = residual * residual + momentVarianceBase;
                    const double rhoValue = (a.dS + 1.0) / (a.dS + omegaInValue * momentValue / baseVariance);
                    mo = (float)momentValue;
                    rh = (float)rhoValue;
                    dbar += momentValue / baseVariance;
                    ++activeCount;
                }
                if (a.moment) a.moment[idx] = mo;
                if (REG) { momReg[j] = mo; rhoReg[j] = rh; }
                else a.rhoOut[idx] = rh;
            };
            MUNC_FOR_TRACKS(first)
            if (activeCount > 0) {
                dbar = dbar / (double)activeCount;
                omegaRawValue = (a.dOmega + 1.0) / (a.dOmega + dbar);
                omegaValue = omegaRawValue < a.omegaMin ? a.omegaMin : (omegaRawValue > a.omegaMax ? a.omegaMax : omegaRawValue);
            } else {
                omegaRawValue = 1.0;
                omegaValue = 1.0;
            }
        } else {
            omegaRawValue = omegaInValue;
            omegaValue = omegaRawValue < a.omegaMin ? a.omegaMin : (omegaRawValue > a.omegaMax ? a.omegaMax : omegaRawValue);
        }
        if (a.omegaRaw) a.omegaRaw[g] = (float)omegaRawValue;
        a.omegaOut[g] = (float)omegaValue;
    } else {
        if (a.omegaRaw) a.omegaRaw[g] = 1.0f;
        a.omegaOut[g] = 1.0f;
    }

    const bool stashed = a.weighted && a.updateWeights;
    auto second = [&](int j) {
        const int64_t idx = (int64_t)j * rs + g;
        const double countValue = a.countFloor ? (double)a.countFloor[idx] : 0.0;
        double localValue, totalValue;
        float mo = 0.0f, rh = 1.0f;
        if (a.activeMode == 0 || munc_mask_nonzero(a.active, a.activeMode, a.maskStride, j, g)) {
            bad = bad || badInterval || (a.countFloor && (!munc_finite(countValue) || countValue < 0.0));
            if (!a.weighted) {
                const double mu = (double)a.munc[idx] + a.pad;
                const double x = (double)a.data[idx];
                bad = bad || !munc_finite(x) || !munc_finite(mu) || mu <= 0.0;
                const double residual = x - backgroundValue - stateValue;
                const double momentValue = residual * residual + momentVarianceBase;
                mo = (float)momentValue;
                localValue = momentValue - a.pad - countValue;
            } else {
                // the Student-t sweep reads back the float32 values just written (pyx:4995-4996)
                if (stashed) {
                    if (REG) { mo = momReg[j]; rh = rhoReg[j]; }
                    else {
                        rh = a.rhoOut[idx];
                        const double residual = (double)a.data[idx] - backgroundValue - stateValue;
                        mo = a.moment ? a.moment[idx] : (float)(residual * residual + momentVarianceBase);
                    }
                } else {
                    const double mu = (double)a.munc[idx] + a.pad;
                    const double x = (double)a.data[idx];
                    rh = a.rhoIn ? a.rhoIn[idx] : 1.0f;
                    const double rhoIn = (double)rh;
                    bad = bad || !munc_finite(x) || !munc_finite(mu) || mu <= 0.0 || !munc_finite(rhoIn) || rhoIn <= 0.0;
                    const double residual = x - backgroundValue - stateValue;
                    mo = (float)(residual * residual + momentVarianceBase);
                }
                localValue = omegaValue * (double)rh * (double)mo - a.pad - countValue;
            }
            munc_cascade(localValue, totalValue, countValue, a.varianceFloor, a.varianceCap, true);
        } else {
            localValue = (double)a.munc[idx] - countValue;
            munc_cascade(localValue, totalValue, countValue, a.varianceFloor, a.varianceCap, false);
        }
        if (a.moment && !(stashed)) a.moment[idx] = mo;
        if (!(stashed && !REG)) a.rhoOut[idx] = rh;
        a.local[idx] = (float)localValue;
        a.variance[idx] = (float)totalValue;
    };
    MUNC_FOR_TRACKS(second)
    if (bad) *a.invalid = 1u;       // (plain store of one value by any number of lanes)
}

#undef MUNC_FOR_TRACKS

// ---------------------------------------------------------------------------------------------------------------
// rolling mean of the local evidence
// ---------------------------------------------------------------------------------------------------------------
struct MuncRollArgs {
    const float *local;                 // (m, rowStride)
    const unsigned char *exclude;       // nonzero = excluded
    int excludeMode;
    int64_t maskStride;
    float *out;
    int64_t rowStride;
    const int64_t *chainOff, *chainLen; // nullptr: one chain of n intervals at offset 0
    int64_t n;
    int m;
    int64_t window;
    double eps;
    unsigned int *dirty;                // [chain][m]: 0 (zeroed by the host), or 1 = a block of the row saw an inexact operation
    unsigned int *invalid;
    unsigned long long *fallbackRows;   // rows k_munc_roll_fix redid
};

// the window [left, right) of interval i (pyx:5601-5608)
__device__ __forceinline__ void munc_window(int64_t i, int64_t n, int64_t window, int64_t &left, int64_t &right) {
    const int64_t half = window / 2;
    left = i >= half ? i - half : 0;
    right = left + window;
    if (right > n) {
        right = n;
        left = right >= window ? right - window : 0;
    }
}
// s := s + x, and whether the addition was exact (Knuth's TwoSum: the residual is the rounding error itself)
__device__ __forceinline__ bool munc_two_sum(double &s, double x) {
    const double t = s + x;
    const double bb = t - s;
    const double err = (s - (t - bb)) + (x - bb);
    s = t;
    return err == 0.0;
}

// the walk of pyx:5600-5639 over intervals [i0, i1) of one row from the state (left, right, sum, count), every cell validated once;
// returns whether every operation was exact
__device__ __forceinline__ bool munc_roll_walk(const MuncRollArgs &a, int64_t j, int64_t g0, int64_t n, int64_t i0, int64_t i1, int64_t left,
                                               int64_t right, double rollingSum, int64_t count, bool &bad) {
    const float *row = a.local + j * a.rowStride + g0;
    bool exact = true;
    for (int64_t i = i0; i < i1; ++i) {
        int64_t tl, tr;
        munc_window(i, n, a.window, tl, tr);
        for (; right < tr; ++right) {
            if (a.excludeMode != 0 && munc_mask_nonzero(a.exclude, a.excludeMode, a.maskStride, j, g0 + right)) continue;
            const double v = (double)row[right];
            exact = munc_two_sum(rollingSum, v) && exact;
            ++count;
        }
        for (; left < tl; ++left) {
            if (a.excludeMode != 0 && munc_mask_nonzero(a.exclude, a.excludeMode, a.maskStride, j, g0 + left)) continue;
            const double v = (double)row[left];
            exact = munc_two_sum(rollingSum, -v) && exact;
            --count;
        }
        const double self = (double)row[i];
        if (!(a.excludeMode != 0 && munc_mask_nonzero(a.exclude, a.excludeMode, a.maskStride, j, g0 + i)))
            bad = bad || !munc_finite(self) || self <= 0.0;     // pyx:5547-5574, every cell once
        double value = count > 0 ? rollingSum / (double)count : self;
        if (value < a.eps) value = a.eps;
        a.out[j * a.rowStride + g0 + i] = (float)value;
    }
    return exact;
}
// the state in front of interval i0 > 0 with the window's sum accumulated in index order; returns whether that was exact
__device__ __forceinline__ bool munc_roll_entry(const MuncRollArgs &a, int64_t j, int64_t g0, int64_t n, int64_t i0, int64_t &left,
                                                int64_t &right, double &sum, int64_t &count) {
    munc_window(i0 - 1, n, a.window, left, right);
    const float *row = a.local + j * a.rowStride + g0;
    bool exact = true;
    sum = 0.0;
    count = 0;
    for (int64_t k = left; k < right; ++k) {
        if (a.excludeMode != 0 && munc_mask_nonzero(a.exclude, a.excludeMode, a.maskStride, j, g0 + k)) continue;
        exact = munc_two_sum(sum, (double)row[k]) && exact;
        ++count;
    }
    return exact;
}

// grid (ceil(blocks of the longest chain / 64), m, nChains) x 64: lane = one block of one row
__global__ __launch_bounds__(64) void k_munc_roll_spec(const MuncRollArgs a) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t n = a.chainLen ? a.chainLen[blockIdx.z] : a.n;
    const int64_t i0 = b * MUNC_ROLL_BLOCK;
    if (i0 >= n) return;
    const int64_t g0 = a.chainOff ? a.chainOff[blockIdx.z] : 0;
    const int64_t j = blockIdx.y;
    const int64_t i1 = i0 + MUNC_ROLL_BLOCK < n ? i0 + MUNC_ROLL_BLOCK : n;
    int64_t left = 0, right = 0, count = 0;
    double sum = 0.0;
    bool bad = false;
    const bool entryExact = b == 0 ? true : munc_roll_entry(a, j, g0, n, i0, left, right, sum, count);
    const bool bodyExact = munc_roll_walk(a, j, g0, n, i0, i1, left, right, sum, count, bad);
    if (!(entryExact && bodyExact)) a.dirty[(int64_t)blockIdx.z * a.m + j] = 1u;       // (one value, any number of lanes)
    if (bad) *a.invalid = 1u;
}

// grid (m, nChains) x 64: one wavefront per row; a row with an inexact block is redone whole, in the reference's operation order.
// The reference's walk has a closed form: the first window [0, min(W, n)) is summed in index order (S_0, reached at interval 0 and
// kept up to interval W / 2); then n - W steps s = 1.. each add cell s + W - 1 and subtract cell s - 1, in that order (S_s, the value
// of interval s + W / 2); the last S stays to the row's end.  An excluded cell contributes an exact + 0.0 (the sum is never -0.0:
// its cells are positive and x - x rounds to +0.0), its count 0.  The lanes stage a chunk of entering and leaving cells in LDS
// (coalesced loads), lane 0 walks the chunk's add / subtract chain -- the only serial part -- and the lanes divide, clamp and store.
constexpr int MUNC_FIX_CHUNK = 512;
__global__ __launch_bounds__(64) void k_munc_roll_fix(const MuncRollArgs a) {
    const int64_t j = blockIdx.x;
    if (a.dirty[(int64_t)blockIdx.y * a.m + j] == 0u) return;
    const int64_t n = a.chainLen ? a.chainLen[blockIdx.y] : a.n;
    const int64_t g0 = a.chainOff ? a.chainOff[blockIdx.y] : 0;
    const int lane = threadIdx.x;
    const float *row = a.local + j * a.rowStride + g0;
    float *out = a.out + j * a.rowStride + g0;
    const int64_t W = a.window, half = W / 2;
    const int64_t w0 = W < n ? W : n, steps = n > W ? n - W : 0;
    __shared__ double sE[MUNC_FIX_CHUNK], sL[MUNC_FIX_CHUNK], sS[MUNC_FIX_CHUNK];
    __shared__ int sC[MUNC_FIX_CHUNK];
    __shared__ signed char sD[MUNC_FIX_CHUNK];
    __shared__ double sEdgeS;
    __shared__ int64_t sEdgeC;
    auto excluded = [&](int64_t k) { return a.excludeMode != 0 && munc_mask_nonzero(a.exclude, a.excludeMode, a.maskStride, j, g0 + k); };
    auto store = [&](int64_t i, double S, int64_t C) {
        double value = C > 0 ? S / (double)C : (double)row[i];
        if (value < a.eps) value = a.eps;
        out[i] = (float)value;
    };
    double S = 0.0;     // (lane 0's)
    int64_t C = 0;
    for (int64_t base = 0; base < w0; base += MUNC_FIX_CHUNK) {
        const int cnt = (int)(w0 - base < MUNC_FIX_CHUNK ? w0 - base : MUNC_FIX_CHUNK);
        for (int k = lane; k < cnt; k += 64) {
            const bool ex = excluded(base + k);
            sE[k] = ex ? 0.0 : (double)row[base + k];
            sD[k] = ex ? 0 : 1;
        }
        __syncthreads();
        if (lane == 0)
            for (int k = 0; k < cnt; ++k) {
                S = S + sE[k];
                C += sD[k];
            }
        __syncthreads();
    }
    if (lane == 0) { sEdgeS = S; sEdgeC = C; }
    __syncthreads();
    {
        const int64_t last = steps > 0 ? (half < n - 1 ? half : n - 1) : n - 1;
        const double S0 = sEdgeS;
        const int64_t C0 = sEdgeC;
        for (int64_t i = lane; i <= last; i += 64) store(i, S0, C0);
    }
    for (int64_t base = 1; base <= steps; base += MUNC_FIX_CHUNK) {
        const int cnt = (int)(steps - base + 1 < MUNC_FIX_CHUNK ? steps - base + 1 : MUNC_FIX_CHUNK);
        for (int k = lane; k < cnt; k += 64) {
            const int64_t in = base + k + W - 1, lo = base + k - 1;
            const bool exIn = excluded(in), exLo = excluded(lo);
            sE[k] = exIn ? 0.0 : (double)row[in];
            sL[k] = exLo ? 0.0 : (double)row[lo];
            sD[k] = (signed char)((exIn ? 0 : 1) - (exLo ? 0 : 1));
        }
        __syncthreads();
        if (lane == 0) {
#pragma unroll 8
            for (int k = 0; k < cnt; ++k) {
                S = S + sE[k];
                S = S - sL[k];
                C += sD[k];
                sS[k] = S;
                sC[k] = (int)C;
            }
        }
        __syncthreads();
        for (int k = lane; k < cnt; k += 64) store(base + k + half, sS[k], sC[k]);
    }
    if (steps > 0) {
        __syncthreads();
        if (lane == 0) { sEdgeS = S; sEdgeC = C; }
        __syncthreads();
        const double Sn = sEdgeS;
        const int64_t Cn = sEdgeC;
        for (int64_t i = steps + half + 1 + lane; i < n; i += 64) store(i, Sn, Cn);
    }
    if (lane == 0) atomicAdd(a.fallbackRows, 1ull);
}

// ---------------------------------------------------------------------------------------------------------------
// the per-cell glue of the seed loop.  One lane per cell: grid (ceil(longest / 256), m, nChains)
// ---------------------------------------------------------------------------------------------------------------
struct MuncCellArgs {
    const int64_t *chainOff, *chainLen;
    int64_t rowStride;
    const float *total, *rho, *countFloor, *local;      // (m, rowStride)
    const float *omega, *gVariance;                     // per interval
    float *out;
    double pad;
    float cap;
    int useWeights, useCap;
};
enum { MUNC_CELL_WORKING = 0, MUNC_CELL_TOTAL = 1, MUNC_CELL_WEIGHT = 2 };

template <int KIND>
__global__ __launch_bounds__(256) void k_munc_cell(const MuncCellArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.chainLen[blockIdx.z]) return;
    const int64_t g = a.chainOff[blockIdx.z] + i;
    const int64_t idx = (int64_t)blockIdx.y * a.rowStride + g;
    if (KIND == MUNC_CELL_WORKING) {            // consenrich.py:7482-7503, float64
        double working = (double)a.total[idx] + a.pad;
        if (a.useWeights) {
            double denom = (double)a.omega[g] * (double)a.rho[idx];
            denom = denom < 1.0e-12 ? 1.0e-12 : denom;
            working = working / denom;
        }
        working += (double)a.gVariance[g];
        working -= a.pad;
        a.out[idx] = (float)(working < 1.0e-12 ? 1.0e-12 : working);
    } else if (KIND == MUNC_CELL_TOTAL) {       // consenrich.py:7557-7576, float32
        float t = a.local[idx];
        if (a.countFloor) t = t + a.countFloor[idx];
        if (a.useCap) t = t > a.cap ? a.cap : t;
        a.out[idx] = t < 1.0e-12f ? 1.0e-12f : t;
    } else {                                    // consenrich.py:7938-7945, float32
        a.out[idx] = a.useWeights ? a.rho[idx] * a.omega[g] : 1.0f;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// the seed front of the background update (consenrich.py:7688-7777 `_updateSeedBackground`): what follows the solve
// ---------------------------------------------------------------------------------------------------------------
// float32 bit pattern -> unsigned key that orders like the value (negative values below positive ones, -0.0 just below +0.0, +inf
// on top of the finite values); munc_order_value is its inverse.  NaNs sort outside the infinities: a total with NaN cells is not
// NumPy's quantile (which is NaN then) unless enough of them reach the rank -- the seed pass refuses such cells where they are active
__host__ __device__ __forceinline__ unsigned int munc_order_key(unsigned int u) { return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__host__ __device__ __forceinline__ unsigned int munc_order_value(unsigned int k) { return (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k; }
// counts[2 c + r] += #cells of chain c whose order key is <= trial[2 c + r]: one pass of the bit-by-bit selection of two order
// statistics of the (m, n) cells of `x`.  grid (ceil(longest /
// (256 * MUNC_RANK_ITEMS)), m, nChains); a lane counts MUNC_RANK_ITEMS cells, the workgroup folds its lanes and adds once per
// rank (integer atomics only: a few thousand per pass and chain instead of one per wavefront of cells).
// perTrack: the two order statistics are those of every (chain, track) row by itself, slot c * m + track instead of c (the
// blacklist floor of csr_munc_track.h); exclude (per interval, or nullptr): cells of intervals with a set byte are left out;
// finiteOnly: so are cells that are not finite
constexpr int MUNC_RANK_ITEMS = 16;
__global__ __launch_bounds__(256) void k_munc_rank_count(const float *x, int64_t rowStride, const int64_t *chainOff, const int64_t *chainLen,
                                                         const unsigned int *trial, unsigned long long *counts,
                                                         const unsigned char *exclude, int perTrack, int finiteOnly) {
    const int c = blockIdx.z;
    const int64_t n = chainLen[c];
    const float *row = x + (int64_t)blockIdx.y * rowStride + chainOff[c];
    const unsigned char *ex = exclude ? exclude + chainOff[c] : nullptr;
    const int64_t slot = perTrack ? (int64_t)c * gridDim.y + blockIdx.y : c;
    const unsigned int t0 = trial[2 * slot], t1 = trial[2 * slot + 1];
    unsigned int c0 = 0, c1 = 0;
    for (int it = 0; it < MUNC_RANK_ITEMS; ++it) {
        const int64_t i = ((int64_t)blockIdx.x * MUNC_RANK_ITEMS + it) * 256 + threadIdx.x;
        if (i < n && !(ex && ex[i] != 0)) {
            const float v = row[i];
            if (finiteOnly && !(__builtin_fabsf(v) <= 3.402823466e+38f)) continue;
            const unsigned int key = munc_order_key(__float_as_uint(v));
            c0 += key <= t0 ? 1u : 0u;
            c1 += key <= t1 ? 1u : 0u;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        c0 += __shfl_xor(c0, o);
        c1 += __shfl_xor(c1, o);
    }
    __shared__ unsigned int part[2][4];
    if ((threadIdx.x & 63) == 0) { part[0][threadIdx.x >> 6] = c0; part[1][threadIdx.x >> 6] = c1; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned int s0 = part[0][0] + part[0][1] + part[0][2] + part[0][3], s1 = part[1][0] + part[1][1] + part[1][2] + part[1][3];
        if (s0) atomicAdd(&counts[2 * slot], (unsigned long long)s0);
        if (s1) atomicAdd(&counts[2 * slot + 1], (unsigned long long)s1);
    }
}

struct MuncGArgs {
    const int64_t *chainOff, *chainLen;
    const double *w64;          // float64 sum over the tracks of the float64 inverse variances, per interval
    const float *bgNext;        // the new background (float32, as the reference's solver returns it)
    const double *sel;          // per chain: [penalty of a negative background (0: none), clip = float64 q99 of total (or 1.0)]
    float *g, *gvar;
    double lamFirst, lamSecond;
    int proxy;                  // 0: G-uncertainty mode "disabled" (G = 0)
};
// g := the new background; G := clip(float32(1 / max(weight + `_backgroundPenaltyDiagonal` + penalty where g < 0, 1e-12)), 0, q99)
__global__ __launch_bounds__(256) void k_munc_g_proxy(const MuncGArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int c = blockIdx.y;
    const int64_t n = a.chainLen[c];
    if (i >= n) return;
    const int64_t g = a.chainOff[c] + i;
    const float bg = a.bgNext[g];
    a.g[g] = bg;
    float gv = 0.0f;
    if (a.proxy) {
        double pen = 0.0;       // core.py:7506-7528, in its order of additions
        if (n >= 2 && a.lamFirst > 0.0) pen += (i == 0 || i == n - 1) ? a.lamFirst : 2.0 * a.lamFirst;
        if (n >= 3 && a.lamSecond > 0.0) {
            if (n == 3) pen += (i == 1 ? 4.0 : 1.0) * a.lamSecond;
            else if (i == 0 || i == n - 1) pen += a.lamSecond;
            else if (i == 1 || i == n - 2) pen += 5.0 * a.lamSecond;
            else pen += 6.0 * a.lamSecond;
        }
        double diagonal = a.w64[g] + pen;
        if (bg < 0.0f) diagonal += a.sel[2 * c];
        gv = (float)(1.0 / (diagonal < 1.0e-12 ? 1.0e-12 : diagonal));
    }
    gv = gv < 0.0f ? 0.0f : gv;
    const float clip = (float)a.sel[2 * c + 1];
    a.gvar[g] = gv > clip ? clip : gv;
}

}  // namespace csr
