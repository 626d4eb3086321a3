// csr_depspan.h -- the device side of the dependence span (pyx:3360-4120 `cchooseDependenceSpan` and its helpers, pyx:2645-3357):
// which rows are byte-identical, the ranking score of every 100 kb window, and the masked autocorrelation of the sampled windows
// up to the crossing decision.
//
// A "matrix" is a device pointer to float32 rows with a row stride (DepMat): how a chain's data lies resident in a batch, and how
// a staged host array lies in work space.  A "window" is a pointer to its first bin with a row stride (DepWin).
//
// What fixes the arithmetic:
//   k_depspan_rowdiff  per pair of rows an any-difference flag over all bins, on the 32-bit patterns (-0.0 != 0.0, NaN payloads
//                      count): what SHA-256 plus array_equal(equal_nan=True) decides;
//   k_depspan_scores   one workgroup per (window, row): the finite values' max(v, 0) compacted stably (ballot scan), then NumPy's
//                      sum of one contiguous float64 array of any length (np_sum_f: the pairwise trees of chunks of 8192
//                      folded in ascending order), walked by one lane; windowBins / finiteCount * sum;
//   k_depspan_center   one workgroup per (window, row): finite count, the four order statistics np.quantile(.., [0.005, 0.995])
//                      reads (method "linear") by a bit-wise search on the ordered 32-bit keys, NumPy's lerp, the clip, np.mean in
//                      NumPy's order, the centring -- every value the reference's bit for bit; a bin that is not finite is left NaN;
//   k_depspan_lags     one lane per (window, row, lag): the pair count and the sum of products over pairs with both bins finite,
//                      in index order, as a compensated dot product (TwoSum plus the FMA product error): accurate to about an ulp
//                      of the exact sum whatever the launch shape.  The window goes through LDS tiles; a skipped pair is skipped
//                      by a select;
//   k_depspan_pool     one workgroup per window: admissibility, lagZero, quorum, the pooled ACF (np.nanmedian over rows), then
//                      one lane walks the prefix sums, the smoothed |ACF|, the persistence scan and the minima in the reference's
//                      order and leaves one record (DepRec = csr_depspan_window) with the margin of the scan.
// Nothing here waits on another workgroup; every loop bound is known at launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "csr_np_order.h"

namespace csr {

constexpr int DEP_TILE = 512;               // values of i per LDS tile of the lag walk
constexpr int DEP_WAVE = 64;                // lags per wavefront = threads per workgroup of the lag walk
constexpr int DEP_CMP = 2048;               // bins per workgroup of the row comparison

struct DepMat {
    const float *base;      // row r at base + r * stride
    int64_t stride, n;      // n bins per row
};
struct DepWin {
    const float *base;      // first bin of the window in row 0; row r at base + r * stride
    int64_t stride;
};
// the per-window record (the C ABI's csr_depspan_window has this layout)
struct DepRec {
    int32_t status;                 // 0: the reference answers None, 1: a result
    int32_t crossing_lag;           // -1: right-censored
    int32_t support_cap_lag, last_crossing_start, valid_rows, valid_rows_at_crossing;
    int32_t flags;                  // bit 0: a lagZero in the underflow range (the caller decides the window)
    int32_t reserved;
    double finite_pair_min, finite_pair_coverage_min;
    double revival;                 // NaN: none
    double margin;                  // min |smoothed ACF - threshold| over the lags the scan examined (inf: none examined)
};
struct DepCfg {
    int64_t windowBins;
    int32_t maxLag, smooth, persist, minPairs;
    double thr, minCov;
};

// grid (ceil(longest / DEP_CMP), pairs, matrices), 256 threads: diff[pair] |= rows (pi[pair], pj[pair]) differ somewhere
__global__ __launch_bounds__(256) void k_depspan_rowdiff(const DepMat *__restrict__ mats, const int *__restrict__ pi,
                                                          const int *__restrict__ pj, unsigned int *__restrict__ diff) {
    const DepMat mt = mats[blockIdx.z];
    const int64_t i0 = (int64_t)blockIdx.x * DEP_CMP;
    if (i0 >= mt.n) return;             // (uniform per workgroup: the grid is sized for the longest matrix)
    const int p = blockIdx.y;
    if (__hip_atomic_load(&diff[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) return;       // (already decided)
    const uint32_t *a = reinterpret_cast<const uint32_t *>(mt.base + (int64_t)pi[p] * mt.stride);
    const uint32_t *b = reinterpret_cast<const uint32_t *>(mt.base + (int64_t)pj[p] * mt.stride);
    bool d = false;
    for (int k = threadIdx.x; k < DEP_CMP; k += 256) {
        const int64_t i = i0 + k;
        if (i < mt.n) d = d || a[i] != b[i];
    }
    if (d) atomicOr(&diff[p], 1u);
}

struct DepScoreArgs {
    const float *base;          // the matrix; window w of the launch starts at bin (w0 + w) * windowBins
    int64_t stride;
    const int *rows;            // the retained rows
    int nRows;
    int64_t windowBins, w0;
    double rankMin;             // sqrt(minFinitePairCoverage)
    double *comp;               // [window of the launch][row][windowBins]
    double *score;              // [w0 + window][row]; NaN: the row does not contribute
};
// grid (windows of the launch, rows), 256 threads
__global__ __launch_bounds__(256) void k_depspan_scores(DepScoreArgs a) {
    __shared__ int sW[4];
    const int64_t wb = a.windowBins;
    const float *x = a.base + (int64_t)a.rows[blockIdx.y] * a.stride + (a.w0 + blockIdx.x) * wb;
    double *comp = a.comp + ((int64_t)blockIdx.x * a.nRows + blockIdx.y) * wb;
    int64_t n = 0;
    for (int64_t t0 = 0; t0 < wb; t0 += 256) {
        const int64_t i = t0 + threadIdx.x;
        const float v = i < wb ? x[i] : __uint_as_float(0x7fc00000u);
        const bool f = np_finite(v);
        int tot;
        const int at = wg_rank256(f, sW, &tot);
        if (f) comp[n + at] = fmax((double)v, 0.0);
        n += tot;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double s = __longlong_as_double(0x7ff8000000000000ll);
    if (n > 0 && (double)n / (double)wb >= a.rankMin) s = (double)wb / (double)n * np_sum_f(comp, n, NpIdentity{});
    a.score[(a.w0 + blockIdx.x) * a.nRows + blockIdx.y] = s;
}

struct DepAcfArgs {
    const DepWin *wins;         // the windows of the launch
    const int *rows;
    int nRows;
    DepCfg cfg;
    double *comp, *cen;         // [window][row][windowBins]: the compacted clipped values; the centred ones (NaN: not finite)
    int *nfin;                  // [window][row]
    double *sums;               // [window][row][maxLag + 1]
    int *pairs;
    double *pooled;             // [window][maxLag]
    int *contrib;               // [window][maxLag]
    double *minPair, *minCov;   // [window][maxLag]: over the contributing rows of a lag
    double *zero;               // [window][row]: lagZero of a valid row, else NaN
    double *med;                // [window][maxLag][row]: the contributing rows' ACF of a lag, ascending (the median's work space)
    double *prefix;             // [window][maxLag + 1]
    DepRec *rec;
};

// grid (windows, rows), 256 threads
__global__ __launch_bounds__(256) void k_depspan_center(DepAcfArgs a) {
    __shared__ int sW[4];
    __shared__ int sC[4][4];
    __shared__ double sMean;
    const int64_t wb = a.cfg.windowBins;
    const DepWin w = a.wins[blockIdx.x];
    const float *x = w.base + (int64_t)a.rows[blockIdx.y] * w.stride;
    const int64_t slot = (int64_t)blockIdx.x * a.nRows + blockIdx.y;
    double *comp = a.comp + slot * wb, *cen = a.cen + slot * wb;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    // c[0..3] summed over the workgroup, for every thread
    auto total4 = [&](int c[4]) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            for (int o = 32; o > 0; o >>= 1) c[j] += __shfl_down(c[j], o);
        __syncthreads();
        if (lane == 0)
            for (int j = 0; j < 4; ++j) sC[wv][j] = c[j];
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) c[j] = sC[0][j] + sC[1][j] + sC[2][j] + sC[3][j];
    };
    int c[4] = {0, 0, 0, 0};
    for (int64_t i = threadIdx.x; i < wb; i += 256) c[0] += np_finite(x[i]);
    total4(c);
    const int n = c[0];
    if (n < 2) {                // (uniform) the reference skips the row
        if (threadIdx.x == 0) a.nfin[slot] = n;
        for (int64_t i = threadIdx.x; i < wb; i += 256) cen[i] = nan;
        return;
    }
    // np.quantile(finite, [0.005, 0.995]), method "linear": virtual index (n - 1) q, the two neighbours, the lerp
    int64_t rk[4];
    double g[2];
    const double qs[2] = {0.005, 0.995};
    for (int j = 0; j < 2; ++j) {
        const double vi = (double)(n - 1) * qs[j];
        const double fl = floor(vi);
        g[j] = vi - fl;
        int64_t lo = (int64_t)fl, hi = lo + 1;
        if (vi >= (double)(n - 1)) lo = hi = n - 1;
        if (lo < 0) lo = 0;
        if (hi > n - 1) hi = n - 1;
        rk[2 * j] = lo;
        rk[2 * j + 1] = hi;
    }
    // the key of rank k is the largest K with count(key < K) <= k: one bit per pass, four ranks at once.  np_key puts -0.0 in front
    // of +0.0, NumPy's sort holds them equal: where a quantile's rank falls among zeros of both signs a clip bound may be the zero of
    // the other sign than the reference's.  A clipped value, and so every centred value and every sum, is the same number either way
    uint32_t cur[4] = {0u, 0u, 0u, 0u};
    for (int bit = 31; bit >= 0; --bit) {
        uint32_t cand[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            cand[j] = cur[j] | (1u << bit);
            c[j] = 0;
        }
        for (int64_t i = threadIdx.x; i < wb; i += 256) {
            const float v = x[i];
            const bool f = np_finite(v);
            const uint32_t k = np_key(v);
#pragma unroll
            for (int j = 0; j < 4; ++j) c[j] += f && k < cand[j];
        }
        total4(c);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if ((int64_t)c[j] <= rk[j]) cur[j] = cand[j];
    }
    const double lowerClip = np_lerp((double)np_unkey(cur[0]), (double)np_unkey(cur[1]), g[0]);
    const double upperClip = np_lerp((double)np_unkey(cur[2]), (double)np_unkey(cur[3]), g[1]);
    // np.clip = minimum(maximum(x, lower), upper), compacted for the mean and in place for the centring
    int64_t at0 = 0;
    for (int64_t t0 = 0; t0 < wb; t0 += 256) {
        const int64_t i = t0 + threadIdx.x;
        const float v = i < wb ? x[i] : __uint_as_float(0x7fc00000u);
        const bool f = np_finite(v);
        const double cl = fmin(fmax((double)v, lowerClip), upperClip);
        int tot;
        const int at = wg_rank256(f, sW, &tot);
        if (f) comp[at0 + at] = cl;
        if (i < wb) cen[i] = f ? cl : nan;
        at0 += tot;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        sMean = np_sum_f(comp, n, NpIdentity{}) / (double)n;
        a.nfin[slot] = n;
    }
    __syncthreads();
    const double mean = sMean;
    for (int64_t i = threadIdx.x; i < wb; i += 256) {
        const double v = cen[i];
        cen[i] = v == v ? v - mean : nan;
    }
}

// grid (ceil((maxLag + 1) / 64), rows, windows), 64 threads: lane l of workgroup g walks lag 64 g + l of its (window, row)
__global__ __launch_bounds__(DEP_WAVE) void k_depspan_lags(DepAcfArgs a) {
    __shared__ double sA[DEP_TILE], sB[DEP_TILE + DEP_WAVE];
    const int64_t wb = a.cfg.windowBins;
    const int64_t slot = (int64_t)blockIdx.z * a.nRows + blockIdx.y;
    const double *x = a.cen + slot * wb;
    const int lane = threadIdx.x;
    const int64_t first = (int64_t)blockIdx.x * DEP_WAVE, lag = first + lane;
    const int L = a.cfg.maxLag + 1;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    double acc = 0.0, low = 0.0;        // the running sum and what its roundings and the products' lost
    int cnt = 0;
    if (a.nfin[slot] >= 2) {            // (uniform)
        const int64_t most = wb - first;        // the wavefront's longest walk: pairs (i, i + first), i < most
        for (int64_t t0 = 0; t0 < most; t0 += DEP_TILE) {
            __syncthreads();
            for (int k = lane; k < DEP_TILE; k += DEP_WAVE) sA[k] = t0 + k < wb ? x[t0 + k] : nan;
            for (int k = lane; k < DEP_TILE + DEP_WAVE; k += DEP_WAVE) sB[k] = t0 + first + k < wb ? x[t0 + first + k] : nan;
            __syncthreads();
            const int len = (int)(most - t0 < DEP_TILE ? most - t0 : DEP_TILE);
#pragma unroll 8
            for (int k = 0; k < len; ++k) {
                const double u = sA[k], v = sB[k + lane];       // (beyond the window v is NaN: the pair does not exist)
                const bool take = u == u && v == v;
                const double p = u * v, e = fma(u, v, -p);
                const double s = acc + p, bb = s - acc;
                const double err = (acc - (s - bb)) + (p - bb);
                const double l2 = low + (err + e);
                acc = take ? s : acc;
                low = take ? l2 : low;
                cnt += take;
            }
        }
    }
    if (lag < L) {
        a.sums[slot * L + lag] = acc + low;
        a.pairs[slot * L + lag] = cnt;
    }
}

// grid (windows), 256 threads
__global__ __launch_bounds__(256) void k_depspan_pool(DepAcfArgs a) {
    __shared__ int sValid, sFlags;
    const DepCfg cf = a.cfg;
    const int64_t wb = cf.windowBins;
    const int R = a.nRows, L = cf.maxLag + 1, W = blockIdx.x;
    const double nan = __longlong_as_double(0x7ff8000000000000ll), inf = __longlong_as_double(0x7ff0000000000000ll);
    double *sZero = a.zero + (int64_t)W * R;
    if (threadIdx.x == 0) {
        int valid = 0, flags = 0;
        for (int r = 0; r < R; ++r) {
            const int64_t slot = (int64_t)W * R + r;
            double z = nan;
            if (a.nfin[slot] >= 2) {
                const double pc = (double)a.pairs[slot * L];
                if (pc >= (double)cf.minPairs && pc / (double)wb >= cf.minCov) z = a.sums[slot * L] / pc;
                if (!(np_finite(z) && z > 0.0)) z = nan;
                else if (z < 1.0e-290) flags |= 1;
            }
            sZero[r] = z;
            valid += z == z;
        }
        sValid = valid;
        sFlags = flags;
    }
    __syncthreads();
    const int valid = sValid;
    double *pooled = a.pooled + (int64_t)W * cf.maxLag;
    int *contrib = a.contrib + (int64_t)W * cf.maxLag;
    double *minPair = a.minPair + (int64_t)W * cf.maxLag, *minCov = a.minCov + (int64_t)W * cf.maxLag;
    for (int l = 1 + threadIdx.x; l < L; l += 256) {
        double *v = a.med + ((int64_t)W * cf.maxLag + (l - 1)) * R;
        int m = 0;
        double mp = inf, mc = inf;
        for (int r = 0; r < R; ++r) {
            const double z = sZero[r];
            if (!(z == z)) continue;
            const int64_t slot = (int64_t)W * R + r;
            const double pc = (double)a.pairs[slot * L + l];
            const double cov = pc / (double)(wb - l);
            if (!(pc >= (double)cf.minPairs && cov >= cf.minCov)) continue;
            const double acf = (a.sums[slot * L + l] / pc) / z;
            if (!np_finite(acf)) continue;
            // insertion into the ascending list
            int k = m++;
            while (k > 0 && v[k - 1] > acf) {
                v[k] = v[k - 1];
                --k;
            }
            v[k] = acf;
            mp = fmin(mp, pc);
            mc = fmin(mc, cov);
        }
        double med = nan;
        if (m > 0) med = (m & 1) ? v[m / 2] : (v[m / 2 - 1] + v[m / 2]) / 2.0;
        pooled[l - 1] = med;
        contrib[l - 1] = m;
        minPair[l - 1] = mp;
        minCov[l - 1] = mc;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    DepRec rc{};
    rc.crossing_lag = -1;
    rc.valid_rows = valid;
    rc.flags = sFlags;
    rc.revival = nan;
    rc.margin = inf;
    rc.finite_pair_min = rc.finite_pair_coverage_min = nan;
    auto done = [&](int status) {
        rc.status = status;
        a.rec[W] = rc;
    };
    if (valid <= 0) return done(0);
    const int quorum = (valid + 1) / 2;         // max(1, ceil(valid / 2))
    int cap = cf.maxLag;
    for (int k = 0; k < cf.maxLag; ++k)
        if (contrib[k] < quorum) {
            cap = k;
            break;
        }
    rc.support_cap_lag = cap;
    for (int k = cap; k < cf.maxLag; ++k) pooled[k] = nan;
    if (cap <= 0) return done(0);
    const int h = (cf.smooth - 1) / 2;
    const int lastStart = cap - h - cf.persist + 1;
    rc.last_crossing_start = lastStart;
    if (lastStart < 1 + h) return done(0);
    // np.cumsum of |pooled|, one running sum
    double *prefix = a.prefix + (int64_t)W * L;
    double run = 0.0;
    prefix[0] = 0.0;
    for (int k = 0; k < cap; ++k) {
        run = k == 0 ? fabs(pooled[0]) : run + fabs(pooled[k]);
        prefix[k + 1] = run;
    }
    auto smoothed = [&](int lag) { return (prefix[lag + h] - prefix[lag - h - 1]) / (double)cf.smooth; };
    int crossing = -1;
    for (int start = 1 + h; start <= lastStart && crossing < 0; ++start) {
        bool found = true;
        for (int k = 0; k < cf.persist; ++k) {
            const double cv = smoothed(start + k);
            if (!np_finite(cv)) {
                rc.margin = 0.0;
                found = false;
                break;
            }
            rc.margin = fmin(rc.margin, fabs(cv - cf.thr));
            if (cv >= cf.thr) {
                found = false;
                break;
            }
        }
        if (found) crossing = start;
    }
    rc.crossing_lag = crossing;
    int useEnd, s0, s1;
    if (crossing > 0) {
        useEnd = crossing + cf.persist - 1 + h;
        s0 = crossing - h;
        s1 = useEnd;
    } else {
        useEnd = cap;
        s0 = lastStart - h;
        s1 = cap;
    }
    double mp = inf, mc = inf;
    for (int k = 0; k < useEnd && k < cf.maxLag; ++k) {
        mp = fmin(mp, minPair[k]);
        mc = fmin(mc, minCov[k]);
    }
    if (!(mp < inf)) return done(0);            // (no contributing pair at all)
    rc.finite_pair_min = mp;
    rc.finite_pair_coverage_min = mc;
    int vr = 0x7fffffff;
    for (int k = s0 - 1; k < s1; ++k) vr = contrib[k] < vr ? contrib[k] : vr;
    rc.valid_rows_at_crossing = vr;
    if (crossing > 0) {
        const int r0 = crossing + cf.persist - 1;
        if (r0 < cap) {
            double mx = 0.0;
            for (int k = r0; k < cap; ++k) mx = fmax(mx, fabs(pooled[k]));
            rc.revival = mx;
        }
    }
    done(1);
}

}  // namespace csr
