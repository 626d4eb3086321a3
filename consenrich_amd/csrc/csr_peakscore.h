// csr_peakscore.h -- the numeric side of the reference's DWB peak scoring, bit for bit (peaks.py:2295-2356
// `_segmentScoreAgainstThresholdView` / `_bestSegmentScoreAcrossThresholdViews`, 2182-2203 `_empiricalReplaySegmentPValues`,
// 2206-2257 `_replayFDRQValues`).
//
// Segment scores.  A segment [a, b] of a float64 track against a view (threshold, null scale): the clipped excess
// e[i] = clip((s[i] - thr) / scale, 0, inf), its np.sum, its np.max, sum / sqrt(len) and sum / len.
//   k_peak_view_score  one wavefront per (segment, view).  np.sum is the ascending fold of the pairwise sums of chunks of
//                      NP_CHUNK values; the pairwise tree of a chunk ends in leaves of 64..128 values (np_leaf_f).  Lane 0 walks
//                      the tree (np_tree) to list the leaves of the chunk in order, the lanes sum one leaf each, lane 0 walks it
//                      again with the leaf sums; the maximum rides along and is reduced across the lanes at the end;
//   k_peak_view_pick   one thread per segment: score and mean of every view, the first view is the best and a later one replaces
//                      it only if its score compares > (a NaN never replaces).
// Empirical p and q values.  Both read the replay pool only through counts c(x) = #(pool >= x): the per-draw counts of
// `_replayFDRQValues` enter through their mean, and their sum over the draws is c(x) of the pooled draws.  With the pool and the
// observed statistics sorted by the null's keys-only sort (csr_null.h):
//   k_pool_tail_counts one thread per (metric, observed statistic): lower_bound on `<` (so +0.0 and -0.0 are equal wherever the
//                      sort left them), c, p = clip((1 + c) / (N + 1), 0, 1);
//   k_replay_raw       one thread per (metric, position of the ascending observed statistics): obsAt = #(observed >= x) by
//                      lower_bound, raw = clip((c / R + pseudo) / max(obsAt, 1), 0, 1) -- a function of the value alone;
//   k_replay_scan      q(x) = min of raw over the observed values <= x: an inclusive prefix minimum along the ascending order
//                      (the reference's suffix minimum along the descending one), one workgroup per metric;
//   k_replay_scatter   back to the caller's order through one more lower_bound; max(q, p) if asked for;
//   k_peak_nonfinite   sets a flag word where a value is not finite (the reference's two ValueErrors).
// Nothing here waits on another workgroup: every dependency is a kernel boundary, every loop bound is known at launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "csr_np_order.h"

namespace csr {

constexpr int PS_MAX_VIEWS = 16;        // views per call
constexpr int PS_MAX_METRICS = 3;       // score, integrated excess, max excess
constexpr int PS_LEAVES = 128;          // leaves of the pairwise tree of one chunk: a block above 128 values splits into parts of >= 64
// a block above 128 values splits at n / 2 - (n / 2) % 8 >= 64, so every leaf holds at least 64 values: a chunk has at most
// NP_CHUNK / 64 leaves
static_assert(PS_LEAVES * 64 >= NP_CHUNK, "PS_LEAVES must hold the leaves of one chunk");

// ---- segment scores ---------------------------------------------------------------------------------------------------------
// np.max over values that are >= +0.0 or NaN (np_max_nan): a NaN stays.  Which NaN, when a segment holds NaNs of DIFFERENT bit
// patterns (a score track with several distinct NaNs), follows the lanes and not NumPy's index order; the sums add such NaNs in NumPy's order but take
// the hardware's choice of operand.  One NaN pattern per call -- a NaN threshold or null scale, np.nan in the track, an invalid
// operation -- comes back bit for bit; that is what is supported and tested.
// np.clip((x - off) / s, 0, None) of one element like np_excess, with every NaN bit for bit what the reference's host computes: a
// NaN operand comes through as it is, the first one if both are (here x - off is an add of the NEGATED threshold, which would flip
// the sign of a NaN threshold), and an invalid operation (inf - inf, 0 / 0, inf / inf) gives the negative default NaN
__device__ __forceinline__ double ps_excess(double x, double off, double s) {
    const double invalid = __longlong_as_double((long long)0xfff8000000000000ull);
    double d;
    if (x != x) d = x;
    else if (off != off) d = off;
    else {
        d = x - off;
        if (d != d) d = invalid;
    }
    double v;
    if (d != d) v = d;
    else if (s != s) v = s;
    else {
        v = __ddiv_rn(d, s);
        if (v != v) v = invalid;
    }
    return (v > 0.0 || v != v) ? v : 0.0;
}
// a / b for a finite b > 0: a NaN stays as it is
__device__ __forceinline__ double ps_div(double a, double b) { return a != a ? a : __ddiv_rn(a, b); }
struct PeakExcess {
    double off, s;
    double &mx;
    __device__ __forceinline__ double operator()(double x) {
        const double v = ps_excess(x, off, s);
        mx = np_max_nan(mx, v);
        return v;
    }
};
struct PeakScoreArgs {
    const double *x;                    // the track, n values
    int64_t n;
    const int64_t *starts, *ends;       // nSeg segments, inclusive; clamped to [0, n - 1] here (end < start: empty)
    int nSeg, nViews;
    const double *thr, *scale;          // nViews (scale already max(scale, DBL_MIN))
    double *stat;                       // [seg][view][2]: np.sum and np.max of the excess
    double *score, *integ, *mean, *mx;  // nSeg (k_peak_view_pick)
    int *view;
};
// grid (nSeg, nViews)
__global__ __launch_bounds__(64) void k_peak_view_score(PeakScoreArgs a) {
    __shared__ int sLo[PS_LEAVES], sLen[PS_LEAVES];
    __shared__ double sSum[PS_LEAVES];
    __shared__ int stLen[NP_STACK];
    __shared__ double stLeft[NP_STACK];
    __shared__ int sLeaves;
    const int seg = blockIdx.x, v = blockIdx.y, lane = threadIdx.x;
    int64_t s0 = a.starts[seg], e0 = a.ends[seg];
    if (s0 < 0) s0 = 0;
    if (e0 > a.n - 1) e0 = a.n - 1;
    double *out = a.stat + ((int64_t)seg * a.nViews + v) * 2;
    if (e0 < s0) {                      // (uniform per workgroup)
        if (lane == 0) {
            out[0] = 0.0;
            out[1] = 0.0;
        }
        return;
    }
    const int64_t len = e0 - s0 + 1;
    const double *x = a.x + s0;
    double mx = 0.0, total = 0.0;
    PeakExcess f{a.thr[v], a.scale[v], mx};
    for (int64_t c0 = 0; c0 < len; c0 += NP_CHUNK) {
        const int cl = (int)(len - c0 < NP_CHUNK ? len - c0 : NP_CHUNK);
        if (lane == 0) {                // the leaves of the chunk's tree, left to right
            int nl = 0;
            np_tree(cl, [&](int lo, int m) {
                if (nl < PS_LEAVES) {
                    sLo[nl] = lo;
                    sLen[nl] = m;
                }
                ++nl;
                return 0.0;
            }, stLen, stLeft);
            sLeaves = nl < PS_LEAVES ? nl : PS_LEAVES;
        }
        __syncthreads();
        const int nl = sLeaves;
        for (int k = lane; k < nl; k += 64) sSum[k] = np_leaf_f(x + c0 + sLo[k], sLen[k], f);
        __syncthreads();
        if (lane == 0) {                // the same walk with the leaf sums taken in order
            int next = 0;
            const double ret = np_tree(cl, [&](int, int) { return sSum[next++]; }, stLen, stLeft);
            total = c0 == 0 ? ret : total + ret;
        }
        __syncthreads();
    }
    for (int d = 32; d > 0; d >>= 1) mx = np_max_nan(mx, __shfl_xor(mx, d, 64));
    if (lane == 0) {
        out[0] = total;
        out[1] = mx;
    }
}
// one thread per segment
__global__ __launch_bounds__(64) void k_peak_view_pick(PeakScoreArgs a) {
    const int seg = blockIdx.x * 64 + threadIdx.x;
    if (seg >= a.nSeg) return;
    int64_t s0 = a.starts[seg], e0 = a.ends[seg];
    if (s0 < 0) s0 = 0;
    if (e0 > a.n - 1) e0 = a.n - 1;
    double bScore = 0.0, bInteg = 0.0, bMean = 0.0, bMax = 0.0;
    int bView = 0;
    if (e0 >= s0) {
        const double len = (double)(e0 - s0 + 1), root = __dsqrt_rn(len);
        for (int v = 0; v < a.nViews; ++v) {
            const double *st = a.stat + ((int64_t)seg * a.nViews + v) * 2;
            const double score = ps_div(st[0], root);
            if (v == 0 || score > bScore) {
                bScore = score;
                bInteg = st[0];
                bMean = ps_div(st[0], len);
                bMax = st[1];
                bView = v;
            }
        }
    }
    a.score[seg] = bScore;
    a.integ[seg] = bInteg;
    a.mean[seg] = bMean;
    a.mx[seg] = bMax;
    a.view[seg] = bView;
}

// ---- empirical p and q values -----------------------------------------------------------------------------------------------
// grid (ceil(n / 256)): *flag |= bit if a value is not finite
__global__ __launch_bounds__(256) void k_peak_nonfinite(const double *__restrict__ x, int64_t n, unsigned int *flag, unsigned int bit) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double v = x[i];
    if (!np_finite(v)) atomicOr(flag, bit);
}
// np.searchsorted(sorted, x, side="left")
__device__ __forceinline__ int64_t ps_lower_bound(const double *__restrict__ s, int64_t n, double x) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (s[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ double ps_clip01(double v) { return v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v); }
struct PoolPqArgs {
    int nMetrics;
    int64_t K, N, R;                    // observed statistics per metric, pool size per metric, replay draws (empty ones included)
    const double *obs;                  // [metric][K], the caller's order
    const double *obsSorted;            // metric m ascending at obsSorted + m * obsStride
    const double *poolSorted;           // ... at poolSorted + m * poolStride (N > 0)
    int64_t obsStride, poolStride;
    double *p, *q;                      // [metric][K]
    long long *exceed;                  // [metric][K]: c = #(pool >= x)
    double *raw;                        // [metric][K] work: raw FDR, then its prefix minimum, along the ascending order
    int combine;                        // q := max(q, p)
};
// grid (ceil(nMetrics K / 256))
__global__ __launch_bounds__(256) void k_pool_tail_counts(PoolPqArgs a) {
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= a.nMetrics * a.K) return;
    const int64_t m = id / a.K;
    const int64_t c = a.N > 0 ? a.N - ps_lower_bound(a.poolSorted + m * a.poolStride, a.N, a.obs[id]) : 0;
    a.exceed[id] = c;
    a.p[id] = a.N > 0 ? ps_clip01(__ddiv_rn(1.0 + (double)c, (double)(a.N + 1))) : 1.0;
}
__global__ __launch_bounds__(256) void k_replay_raw(PoolPqArgs a) {
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= a.nMetrics * a.K) return;
    const int64_t m = id / a.K, j = id % a.K;
    const double *so = a.obsSorted + m * a.obsStride;
    const double x = so[j];
    const int64_t obsAt = a.K - ps_lower_bound(so, a.K, x);
    const int64_t c = a.N > 0 ? a.N - ps_lower_bound(a.poolSorted + m * a.poolStride, a.N, x) : 0;
    const double expected = a.R > 0 ? __ddiv_rn((double)c, (double)a.R) : 0.0;
    const double pseudo = a.R > 0 ? __ddiv_rn(1.0, (double)(a.R + 1)) : 1.0;
    a.raw[id] = ps_clip01(__ddiv_rn(expected + pseudo, (double)(obsAt > 1 ? obsAt : 1)));
}
// grid (nMetrics): raw[m][j] := min(raw[m][0 .. j]).  Thread t owns a run of consecutive positions
__global__ __launch_bounds__(256) void k_replay_scan(PoolPqArgs a) {
    __shared__ double sM[256];
    double *r = a.raw + (int64_t)blockIdx.x * a.K;
    const int t = threadIdx.x;
    const int64_t per = (a.K + 255) / 256, j0 = t * per, j1 = j0 + per < a.K ? j0 + per : a.K;
    double mn = 1.0;                    // (raw <= 1)
    for (int64_t j = j0; j < j1; ++j) mn = r[j] < mn ? r[j] : mn;
    sM[t] = mn;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {     // inclusive prefix minimum of the threads' minima
        const double o = t >= d ? sM[t - d] : 1.0;
        __syncthreads();
        sM[t] = o < sM[t] ? o : sM[t];
        __syncthreads();
    }
    double run = t > 0 ? sM[t - 1] : 1.0;
    for (int64_t j = j0; j < j1; ++j) {
        run = r[j] < run ? r[j] : run;
        r[j] = run;
    }
}
__global__ __launch_bounds__(256) void k_replay_scatter(PoolPqArgs a) {
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= a.nMetrics * a.K) return;
    const int64_t m = id / a.K;
    const double *so = a.obsSorted + m * a.obsStride;
    const int64_t pos = ps_lower_bound(so, a.K, a.obs[id]);     // the first of the values equal to this one: raw is the same for all
    double q = ps_clip01(a.raw[m * a.K + (pos < a.K ? pos : a.K - 1)]);
    if (a.combine) q = a.p[id] > q ? a.p[id] : q;
    a.q[id] = q;
}

// ---- the replay pool ----------------------------------------------------------------------------------------------------------
// One workgroup per track (a draw of a chain) of a segment run whose rows are on the device: its three metric columns go to the
// chain's pool.  A track over the total cap keeps the first `keep` rows of Python's stable descending sort on score, i.e. the rows
// whose rank #(s[j] > s[i]) + #(s[j] == s[i], j < i) is below `keep`; the rank is also the row's place in the pool, so the order
// is a function of the values (rows^2 comparisons per track: a track holds at most scales x views x per-view cap rows).  A NaN
// score in such a track leaves the order to the caller: flag[track] = 1 and nothing is written.  outMax = np.max of the scores.
struct PoolTrack {
    int64_t rowBase, rows, keep;        // rows of the track in the run's output; keep = min(rows, total cap)
    double *dst[3];                     // where its `keep` values of score / integrated / max go
};
// grid (tracks); tracks without rows are not launched for
__global__ __launch_bounds__(256) void k_pool_append(const PoolTrack *__restrict__ tracks, const double *__restrict__ score,
                                                     const double *__restrict__ integ, const double *__restrict__ mx,
                                                     double *__restrict__ outMax, int *__restrict__ outFlag) {
    __shared__ double sM[256];
    __shared__ int sNan;
    const PoolTrack t = tracks[blockIdx.x];
    const int th = threadIdx.x;
    const double *s = score + t.rowBase, *g = integ + t.rowBase, *m = mx + t.rowBase;
    if (th == 0) sNan = 0;
    __syncthreads();
    double best = s[0];
    bool nan = false;
    for (int64_t i = th; i < t.rows; i += 256) {
        const double v = s[i];
        best = np_max_nan(best, v);
        nan = nan || v != v;
    }
    if (nan) atomicOr(&sNan, 1);
    sM[th] = best;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (th < h) sM[th] = np_max_nan(sM[th], sM[th + h]);
        __syncthreads();
    }
    const bool over = t.rows > t.keep, undecided = over && sNan != 0;
    if (th == 0) {
        outMax[blockIdx.x] = sM[0];
        outFlag[blockIdx.x] = undecided ? 1 : 0;
    }
    if (undecided) return;              // (uniform per workgroup)
    for (int64_t i = th; i < t.rows; i += 256) {
        int64_t r = i;
        if (over) {
            const double v = s[i];
            r = 0;
            for (int64_t j = 0; j < t.rows; ++j) {
                const double w = s[j];
                r += (w > v) || (w == v && j < i);
            }
            if (r >= t.keep) continue;
        }
        t.dst[0][r] = s[i];
        t.dst[1][r] = g[i];
        t.dst[2][r] = m[i];
    }
}

}  // namespace csr
