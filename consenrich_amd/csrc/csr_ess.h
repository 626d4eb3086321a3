// csr_ess.h -- the positive-autocorrelation effective sample size scan behind the ROCCO budget, bit for bit what the reference's
// native computes (pyx:9160-9279 `cEstimateEffectiveSampleSize`), and the three per-bin series the budget policy scans
// (peaks.py:1414-1434).
//
// What fixes the arithmetic: every sum of the native -- the mean, the sum of x[i]^2 and the sum of x[i] x[i + lag] of every lag --
// runs in index order with a separate multiply and add.  So each sum is one sequential walk of one lane, and
// the parallelism is across lags and tracks:
//   k_ess_series   parallel over bins: the raw series of a score track (0/1 tail indicator, clipped standardised excess, or the
//                  excess's mean over a z grid added in grid order), and, once the mean is known, the centred series x[i] - mean;
//   k_ess_mean     one wavefront per track: the in-order sum of the active values, staged through LDS;
//   k_ess_lags     one lane per (track, lag), 64 consecutive lags of a track per wavefront; lag 0 is the variance sum.  The
//                  centred series goes through two LDS tiles -- x[i .. i + T) and x[i + lag0 .. i + lag0 + T + 64) -- filled by
//                  coalesced 8-byte loads; the next pair of tiles is in flight in registers while this one is walked.  A lane
//                  reads x[i] at a broadcast address and x[i + lag] at consecutive addresses (no bank conflict).  With a mask
//                  both flags are tested and an integer pair count is kept per lane.  In a tile whose every pair exists for all 64
//                  lags (all tiles but the last one or two) only the multiply and the add are on the dependent path; the bounds
//                  select is paid in the remaining tiles.
// A skipped element is skipped by a select, never by a multiplication with a flag.  Every loop bound is known at launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "csr_np_order.h"

namespace csr {

constexpr int ESS_TILE = 512;               // values of i per LDS tile
constexpr int ESS_WAVE = 64;                // lags per wavefront = threads per workgroup
constexpr int ESS_A = ESS_TILE / ESS_WAVE;              // registers per lane that prefetch x[i ..)
constexpr int ESS_B = ESS_TILE / ESS_WAVE + 1;          // ... and x[i + lag0 ..), one more row for the 63 further lags
constexpr int ESS_MAX_Z = 16;               // (threshold, scale) pairs of an integrated-excess series: the stage's own limit (ess.MAX_Z)

enum : int { ESS_SERIES_GIVEN = 0, ESS_SERIES_OCCUPANCY = 1, ESS_SERIES_SOFT = 2, ESS_SERIES_INTEGRATED = 3 };

struct EssTrack {
    const double *src;              // the score track (series kinds 1-3) or the given series (kind 0), n values
    const unsigned char *mask;      // activeMask or nullptr: every value is active
    double *cen;                    // n values: the raw series, then the centred one
    int64_t n;
    int64_t slot;                   // first of the track's sums / pairs entries
    int64_t lagEnd;                 // the last lag wanted in this round (-1: none)
    int kind, nz;
    double mean;
    double thr[ESS_MAX_Z], den[ESS_MAX_Z];      // den = max(null scale, DBL_MIN)
};

// grid (ceil(longest / 256), tracks).  centre = 0: cen := the raw series (a given series is copied); 1: cen := cen - mean
__global__ __launch_bounds__(256) void k_ess_series(const EssTrack *__restrict__ tracks, int centre) {
    const EssTrack &tr = tracks[blockIdx.y];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= tr.n) return;
    if (centre) {
        tr.cen[i] = tr.cen[i] - tr.mean;
        return;
    }
    const double x = tr.src[i];
    double v;
    if (tr.kind == ESS_SERIES_OCCUPANCY) v = x > tr.thr[0] ? 1.0 : 0.0;
    else if (tr.kind == ESS_SERIES_SOFT) v = np_excess(x, tr.thr[0], tr.den[0]);
    else if (tr.kind == ESS_SERIES_INTEGRATED) {        // np.mean(np.vstack(parts), axis=0): the rows added in order, then / nz
        v = np_excess(x, tr.thr[0], tr.den[0]);
        for (int k = 1; k < tr.nz; ++k) v = v + np_excess(x, tr.thr[k], tr.den[k]);
        v = __ddiv_rn(v, (double)tr.nz);
    } else v = x;
    tr.cen[i] = v;
}

// grid (tracks), one wavefront each: out[track] = the active values of cen added in index order.  Every lane walks the same
// LDS tile (broadcast reads); lane 0 stores
__global__ __launch_bounds__(ESS_WAVE) void k_ess_mean(const EssTrack *__restrict__ tracks, double *__restrict__ out) {
    __shared__ double sX[ESS_TILE];
    __shared__ unsigned char sM[ESS_TILE];
    const EssTrack &tr = tracks[blockIdx.x];
    const int64_t n = tr.n;
    const double *x = tr.cen;
    const unsigned char *mask = tr.mask;
    const int lane = threadIdx.x;
    double rx[ESS_A];
    unsigned char rm[ESS_A];
    auto fetch = [&](int64_t t0) {
#pragma unroll
        for (int r = 0; r < ESS_A; ++r) {
            const int64_t i = t0 + r * ESS_WAVE + lane;
            const bool in = i < n;
            rx[r] = in ? x[i] : 0.0;
            rm[r] = in ? (mask ? mask[i] : (unsigned char)1) : (unsigned char)0;
        }
    };
    double acc = 0.0;
    fetch(0);
    for (int64_t t0 = 0; t0 < n; t0 += ESS_TILE) {
#pragma unroll
        for (int r = 0; r < ESS_A; ++r) {
            sX[r * ESS_WAVE + lane] = rx[r];
            sM[r * ESS_WAVE + lane] = rm[r];
        }
        __syncthreads();
        if (t0 + ESS_TILE < n) fetch(t0 + ESS_TILE);
        const int len = (int)(n - t0 < ESS_TILE ? n - t0 : ESS_TILE);
        // (unrolled: the LDS reads of sixteen steps go out ahead of the dependent adds)
        if (!mask) {        // (uniform) every value is active: the add alone is on the dependent path
#pragma unroll 16
            for (int k = 0; k < len; ++k) acc = acc + sX[k];
        } else {
#pragma unroll 16
            for (int k = 0; k < len; ++k) {
                const double s = acc + sX[k];
                acc = sM[k] ? s : acc;
            }
        }
        __syncthreads();
    }
    if (lane == 0) out[blockIdx.x] = acc;
}

// grid (ceil(lags of the round / 64), tracks): lane l of workgroup g walks lag = lag0 + 64 g + l of its track,
//   sums[slot + 64 g + l] = sum over i < n - lag, both active, of cen[i] * cen[i + lag]   (in index order)
//   pairs[slot + 64 g + l] = how many pairs entered
// A lag beyond the track's lagEnd or >= n enters no pair: sum 0, count 0.  MASK: some track of the launch has a mask (a track
// without one counts as all active).
template <bool MASK>
__global__ __launch_bounds__(ESS_WAVE) void k_ess_lags(const EssTrack *__restrict__ tracks, int64_t lag0, double *__restrict__ sums,
                                                        long long *__restrict__ pairs) {
    __shared__ double sA[ESS_TILE], sB[ESS_TILE + ESS_WAVE];
    __shared__ unsigned char mA[MASK ? ESS_TILE : 1], mB[MASK ? ESS_TILE + ESS_WAVE : 1];
    const EssTrack &tr = tracks[blockIdx.y];
    const int64_t n = tr.n, lagEnd = tr.lagEnd;
    const double *x = tr.cen;
    const unsigned char *mask = tr.mask;
    const int lane = threadIdx.x;
    const int64_t first = lag0 + (int64_t)blockIdx.x * ESS_WAVE;       // the wavefront's first lag
    const int64_t lag = first + lane;
    const int64_t mine = lag <= lagEnd && lag < n ? n - lag : 0;       // this lane's pairs (i, i + lag): i < mine
    const int64_t most = first <= lagEnd && first < n ? n - first : 0;  // the wavefront's longest walk (uniform)
    double ra[ESS_A], rb[ESS_B];
    unsigned char fa[ESS_A], fb[ESS_B];
    auto fetch = [&](int64_t t0) {
#pragma unroll
        for (int r = 0; r < ESS_A; ++r) {
            const int64_t i = t0 + r * ESS_WAVE + lane;
            const bool in = i < n;
            ra[r] = in ? x[i] : 0.0;
            if (MASK) fa[r] = in ? (mask ? mask[i] : (unsigned char)1) : (unsigned char)0;
        }
#pragma unroll
        for (int r = 0; r < ESS_B; ++r) {
            const int64_t i = t0 + first + r * ESS_WAVE + lane;
            const bool in = i < n;
            rb[r] = in ? x[i] : 0.0;
            if (MASK) fb[r] = in ? (mask ? mask[i] : (unsigned char)1) : (unsigned char)0;
        }
    };
    double acc = 0.0;
    long long cnt = 0;
    if (most > 0) fetch(0);
    for (int64_t t0 = 0; t0 < most; t0 += ESS_TILE) {
#pragma unroll
        for (int r = 0; r < ESS_A; ++r) {
            sA[r * ESS_WAVE + lane] = ra[r];
            if (MASK) mA[r * ESS_WAVE + lane] = fa[r];
        }
#pragma unroll
        for (int r = 0; r < ESS_B; ++r) {
            sB[r * ESS_WAVE + lane] = rb[r];
            if (MASK) mB[r * ESS_WAVE + lane] = fb[r];
        }
        __syncthreads();
        if (t0 + ESS_TILE < most) fetch(t0 + ESS_TILE);
        const int len = (int)(most - t0 < ESS_TILE ? most - t0 : ESS_TILE);
        const int64_t left = mine - t0;         // this lane's pairs from t0 on (may be <= 0)
        // (unrolled: the LDS reads of sixteen steps go out ahead of the dependent adds)
        if (t0 + len + (ESS_WAVE - 1) <= most) {
            // every pair of the tile exists for every lag the wavefront walks (uniform; all tiles but the last one or two): nothing
            // but the multiply and the add is on the dependent path.  A lane without a lag (mine == 0) adds what it reads and is
            // answered with zeros below
            if (MASK) {
#pragma unroll 16
                for (int k = 0; k < len; ++k) {
                    const double s = acc + sA[k] * sB[k + lane];
                    const bool take = mA[k] != 0 && mB[k + lane] != 0;
                    acc = take ? s : acc;
                    cnt += take;
                }
            } else {
#pragma unroll 16
                for (int k = 0; k < len; ++k) acc = acc + sA[k] * sB[k + lane];
            }
        } else {
#pragma unroll 16
            for (int k = 0; k < len; ++k) {
                const double s = acc + sA[k] * sB[k + lane];
                bool take = k < left;
                if (MASK) take = take && mA[k] != 0 && mB[k + lane] != 0;
                acc = take ? s : acc;
                cnt += take;
            }
        }
        __syncthreads();
    }
    const int64_t o = tr.slot + (int64_t)blockIdx.x * ESS_WAVE + lane;
    sums[o] = mine > 0 ? acc : 0.0;
    pairs[o] = MASK ? (mine > 0 ? cnt : 0) : mine;     // (without a mask every pair enters)
}

}  // namespace csr
