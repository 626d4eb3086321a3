// csr_null.h -- the robust null of a ROCCO score track: centre, scale and the DWB residual template, bit for bit what the reference
// computes (peaks.py:312-339 `_halfSampleMode`, 418-496 `_selectRobustNullSupport`, 499-540 `estimateROCCONull`, 543-556
// `_estimateTemplateScale`, 1077-1122 `_prepareNullResidualTemplate`).
//
// A TRACK is one float64 vector on the device (a chain's resident scores, an uploaded host vector, gathered templates); all
// tracks of a call share one work-space layout in which track t owns the slots [slot, slot + padded n), padded to NULL_TILE.
//   k_null_sort_tile   the monotone keys (np_key) of a tile of NULL_TILE values, sorted by a bitonic network in LDS; slots past n
//                      hold the largest key, which no finite value has;
//   k_null_merge       one merge-path pass: every thread finds its diagonal of a pair of sorted runs by bisection and merges
//                      NULL_VT keys.  Keys only, so the output is a function of the values alone;
//   k_null_unkey       keys back to doubles, in place;
//   k_null_hsm         the half-sample mode of a sorted prefix: one workgroup per track, one parallel arg-min per level (the plain
//                      float64 subtraction, the LOWEST start among equal widths), until the window holds <= 3 values;
//   k_null_eval        one elementwise pass dst[i] = e(src[i]) of a NullExpr: the template;
//   (csr_np_order.h)   NumPy-order sums of e(src[i]): k_np_chunk_sums<NullJob>, one thread per chunk of 8192, evaluates NumPy's
//                      pairwise tree; k_np_fold<NullJob> adds the chunk sums in ascending order;
//   k_null_flag_count, k_null_scan, k_null_scatter   the stable compaction of the support |x - centre| <= radius (count per
//                      tile, exclusive scan over a track's tiles, scatter in track order);
//   k_null_gather, k_null_search   single values of a sorted track, and how many of its values satisfy (x - a) < b or <= b (one
//                      bisection per query: the predicate is monotone along a sorted track);
//   k_null_abs_rank    exact order statistics of |x - a| or |(x - a) - m| over a sorted range (MAD, the quantiles of the absolute
//                      residuals): the residuals of a sorted range are sorted, so nothing is materialised and nothing selected.
// Every dependency is a kernel boundary, every loop bound is known at launch, no workgroup waits on another.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "csr_np_order.h"

namespace csr {

constexpr int NULL_TILE = 2048;         // keys per bitonic tile (16 KiB of LDS)
constexpr int NULL_VT = 8;              // keys per thread of a merge pass
constexpr int NULL_HSM_T = 256;         // threads of the half-sample-mode workgroup

struct NullTrackDev {
    const double *src;      // the track, n values
    int64_t n;
    int64_t slot;           // first slot of the track in every work-space array (a multiple of NULL_TILE)
    int64_t padded;         // n rounded up to NULL_TILE
};

// an element expression: x - a, clipped to [-b, b], minus m, times f, minus m2, squared or absolute -- each step if its flag is set,
// in this order, every operation on its own (the library is built with -ffp-contract=off)
enum : int { NX_SUBA = 1, NX_CLIP = 2, NX_SUBM = 4, NX_SCALE = 8, NX_SUBM2 = 16, NX_SQ = 32, NX_ABS = 64, NX_ZERO = 128 };
struct NullExpr {
    int flags;
    double a, b, m, f, m2;
    __device__ __forceinline__ double operator()(double x) const {
        if (flags & NX_ZERO) return 0.0;
        double v = x;
        if (flags & NX_SUBA) v = v - a;
        if (flags & NX_CLIP) {          // np.clip = minimum(maximum(v, -b), b) on finite values
            const double lo = -b;
            v = v < lo ? lo : v;
            v = v > b ? b : v;
        }
        if (flags & NX_SUBM) v = v - m;
        if (flags & NX_SCALE) v = v * f;
        if (flags & NX_SUBM2) v = v - m2;
        if (flags & NX_SQ) v = v * v;
        if (flags & NX_ABS) v = fabs(v);
        return v;
    }
};

// ---- the sort -----------------------------------------------------------------------------------------------------------------
// grid (tiles of the longest track, tracks)
__global__ __launch_bounds__(256) void k_null_sort_tile(const NullTrackDev *__restrict__ tracks, unsigned long long *__restrict__ keys) {
    __shared__ unsigned long long s[NULL_TILE];
    const NullTrackDev tr = tracks[blockIdx.y];
    const int64_t i0 = (int64_t)blockIdx.x * NULL_TILE;
    if (i0 >= tr.padded) return;        // (uniform per workgroup)
    const int t = threadIdx.x;
    for (int k = t; k < NULL_TILE; k += 256) s[k] = i0 + k < tr.n ? np_key(tr.src[i0 + k]) : ~0ull;
    __syncthreads();
    for (int k = 2; k <= NULL_TILE; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int p = t; p < NULL_TILE / 2; p += 256) {
                const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1));    // the pair (i, i + j); bit j of i is clear
                const unsigned long long a = s[i], b = s[i + j];
                const bool up = (i & k) == 0;
                if ((a > b) == up) {
                    s[i] = b;
                    s[i + j] = a;
                }
            }
            __syncthreads();
        }
    for (int k = t; k < NULL_TILE; k += 256) keys[tr.slot + i0 + k] = s[k];
}

// grid (ceil(longest padded / (NULL_VT * 256)), tracks): sorted runs of `run` keys in `in` become sorted runs of 2 run keys in `out`
__global__ __launch_bounds__(256) void k_null_merge(const NullTrackDev *__restrict__ tracks, const unsigned long long *__restrict__ in,
                                                    unsigned long long *__restrict__ out, int64_t run) {
    const NullTrackDev tr = tracks[blockIdx.y];
    const int64_t o = ((int64_t)blockIdx.x * 256 + threadIdx.x) * NULL_VT;      // first output of this thread
    if (o >= tr.padded) return;
    const int64_t base = o / (2 * run) * (2 * run);
    const int64_t aEnd = base + run < tr.padded ? base + run : tr.padded;
    const int64_t bEnd = base + 2 * run < tr.padded ? base + 2 * run : tr.padded;
    const unsigned long long *A = in + tr.slot + base, *B = in + tr.slot + aEnd;
    const int64_t lenA = aEnd - base, lenB = bEnd - aEnd, diag = o - base;
    int64_t lo = diag > lenB ? diag - lenB : 0, hi = diag < lenA ? diag : lenA;
    while (lo < hi) {       // the number of keys of A among the first diag outputs
        const int64_t mid = (lo + hi) >> 1;
        if (A[mid] <= B[diag - 1 - mid]) lo = mid + 1;
        else hi = mid;
    }
    int64_t a = lo, b = diag - lo;
    unsigned long long *dst = out + tr.slot + o;
    // (lenA and lenB are multiples of NULL_VT: the two runs hold at least NULL_VT more keys)
#pragma unroll
    for (int k = 0; k < NULL_VT; ++k) {
        const bool takeA = b >= lenB || (a < lenA && A[a] <= B[b]);
        dst[k] = takeA ? A[a] : B[b];
        a += takeA;
        b += !takeA;
    }
}

// grid (ceil(longest padded / 256), tracks): keys -> doubles in place
__global__ __launch_bounds__(256) void k_null_unkey(const NullTrackDev *__restrict__ tracks, unsigned long long *__restrict__ keys) {
    const NullTrackDev tr = tracks[blockIdx.y];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= tr.padded) return;
    double *d = reinterpret_cast<double *>(keys) + tr.slot + i;
    *d = np_unkey(keys[tr.slot + i]);
}

// ---- the half-sample mode of sorted[slot .. slot + m[track]) --------------------------------------------------------------------
// grid (tracks); m[track] <= 0: the track is skipped
__global__ __launch_bounds__(NULL_HSM_T) void k_null_hsm(const NullTrackDev *__restrict__ tracks, const double *__restrict__ sorted,
                                                         const long long *__restrict__ m, double *__restrict__ out) {
    __shared__ double sW[NULL_HSM_T];
    __shared__ long long sS[NULL_HSM_T];
    const NullTrackDev tr = tracks[blockIdx.x];
    const double *v = sorted + tr.slot;
    long long lo = 0, len = m[blockIdx.x];
    if (len <= 0) return;
    const int t = threadIdx.x;
    while (len > 3) {       // (len halves: the number of levels follows from m)
        const long long w = (len + 1) / 2, starts = len - w + 1;
        double bw = 0.0;
        long long bs = -1;
        for (long long s = t; s < starts; s += NULL_HSM_T) {    // ascending starts: strict '<' keeps the first minimum
            const double width = v[lo + s + w - 1] - v[lo + s];
            if (bs < 0 || width < bw) {
                bw = width;
                bs = s;
            }
        }
        sW[t] = bw;
        sS[t] = bs;
        __syncthreads();
        for (int h = NULL_HSM_T / 2; h > 0; h >>= 1) {
            if (t < h) {
                const long long s2 = sS[t + h];
                const double w2 = sW[t + h];
                if (s2 >= 0 && (sS[t] < 0 || w2 < sW[t] || (w2 == sW[t] && s2 < sS[t]))) {
                    sW[t] = w2;
                    sS[t] = s2;
                }
            }
            __syncthreads();
        }
        lo += sS[0];
        len = w;
        __syncthreads();
    }
    if (t == 0) {
        double r;
        if (len == 1) r = v[lo];
        else if (len == 2) r = __ddiv_rn(v[lo] + v[lo + 1], 2.0);
        else {
            const double left = v[lo + 1] - v[lo], right = v[lo + 2] - v[lo + 1];
            r = left <= right ? __ddiv_rn(v[lo] + v[lo + 1], 2.0) : __ddiv_rn(v[lo + 1] + v[lo + 2], 2.0);
        }
        out[blockIdx.x] = r;
    }
}

// ---- elementwise passes and NumPy-order sums ------------------------------------------------------------------------------------
struct NullJob {
    const double *src;
    double *dst;            // k_null_eval only
    int64_t n;
    NullExpr e;
    __device__ const double *data(const double *) const { return src; }     // (a Job of k_np_chunk_sums / k_np_fold)
    __device__ NullExpr elem() const { return e; }
};
// grid (ceil(longest / 256), jobs)
__global__ __launch_bounds__(256) void k_null_eval(const NullJob *__restrict__ jobs) {
    const NullJob jb = jobs[blockIdx.y];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= jb.n) return;
    jb.dst[i] = jb.e(jb.src[i]);
}

// ---- stable compaction of the support ------------------------------------------------------------------------------------------
struct NullSupport {
    double centre, radius;
    int active;             // 0: the track is skipped
    int pad;
};
__device__ __forceinline__ bool null_in_support(double x, const NullSupport &s) { return fabs(x - s.centre) <= s.radius; }
// grid (tiles of the longest track, tracks): cnt[slot / NULL_TILE + tile] = members of the tile
__global__ __launch_bounds__(256) void k_null_flag_count(const NullTrackDev *__restrict__ tracks, const NullSupport *__restrict__ sup,
                                                         long long *__restrict__ cnt) {
    __shared__ int sC[256];
    const NullTrackDev tr = tracks[blockIdx.y];
    const NullSupport sp = sup[blockIdx.y];
    const int64_t i0 = (int64_t)blockIdx.x * NULL_TILE;
    if (!sp.active || i0 >= tr.padded) return;
    const int t = threadIdx.x;
    int c = 0;
    for (int k = t; k < NULL_TILE; k += 256)
        if (i0 + k < tr.n) c += null_in_support(tr.src[i0 + k], sp);
    sC[t] = c;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (t < h) sC[t] += sC[t + h];
        __syncthreads();
    }
    if (t == 0) cnt[tr.slot / NULL_TILE + blockIdx.x] = sC[0];
}
// one thread per track: cnt becomes its exclusive prefix over the track's tiles; total[track] = the support's size
__global__ __launch_bounds__(64) void k_null_scan(const NullTrackDev *__restrict__ tracks, int nTracks, const NullSupport *__restrict__ sup,
                                                  long long *__restrict__ cnt, long long *__restrict__ total) {
    const int j = blockIdx.x * 64 + threadIdx.x;
    if (j >= nTracks || !sup[j].active) return;
    const NullTrackDev tr = tracks[j];
    long long run = 0;
    for (int64_t k = 0; k < tr.padded / NULL_TILE; ++k) {
        const long long c = cnt[tr.slot / NULL_TILE + k];
        cnt[tr.slot / NULL_TILE + k] = run;
        run += c;
    }
    total[j] = run;
}
// grid (tiles of the longest track, tracks): comp[slot + rank in track order] = x.  Thread t owns the 8 consecutive values
// 8 t .. 8 t + 7 of the tile, so ranks ascend with the index
__global__ __launch_bounds__(256) void k_null_scatter(const NullTrackDev *__restrict__ tracks, const NullSupport *__restrict__ sup,
                                                      const long long *__restrict__ cnt, double *__restrict__ comp) {
    __shared__ int sC[256];
    const NullTrackDev tr = tracks[blockIdx.y];
    const NullSupport sp = sup[blockIdx.y];
    const int64_t i0 = (int64_t)blockIdx.x * NULL_TILE;
    if (!sp.active || i0 >= tr.padded) return;
    const int t = threadIdx.x;
    constexpr int PER = NULL_TILE / 256;
    double x[PER];
    bool in[PER];
    int c = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int64_t i = i0 + t * PER + k;
        x[k] = i < tr.n ? tr.src[i] : 0.0;
        in[k] = i < tr.n && null_in_support(x[k], sp);
        c += in[k];
    }
    sC[t] = c;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {     // inclusive scan of the threads' counts
        const int add = t >= d ? sC[t - d] : 0;
        __syncthreads();
        sC[t] += add;
        __syncthreads();
    }
    long long pos = cnt[tr.slot / NULL_TILE + blockIdx.x] + (sC[t] - c);
#pragma unroll
    for (int k = 0; k < PER; ++k)
        if (in[k]) comp[tr.slot + pos++] = x[k];
}

// ---- single values and counts of a sorted track ---------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_null_gather(const double *const *__restrict__ ptrs, int n, double *__restrict__ out) {
    const int j = blockIdx.x * 64 + threadIdx.x;
    if (j < n) out[j] = *ptrs[j];
}
struct NullQuery {
    const double *sorted;
    int64_t n;
    double a, b;
    int strict;             // 1: count (x - a) < b; 0: count (x - a) <= b
    int pad;
};
__global__ __launch_bounds__(64) void k_null_search(const NullQuery *__restrict__ qs, int n, long long *__restrict__ out) {
    const int j = blockIdx.x * 64 + threadIdx.x;
    if (j >= n) return;
    const NullQuery q = qs[j];
    int64_t lo = 0, hi = q.n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        const double v = q.sorted[mid] - q.a;
        const bool yes = q.strict ? v < q.b : v <= q.b;
        if (yes) lo = mid + 1;
        else hi = mid;
    }
    out[j] = lo;
}

// Exact order statistics of |e(x)| over a sorted range, e a NullExpr of subtractions only: e(sorted[i]) ascends with i (every
// rounding is monotone), so the absolute values are two ascending sequences -- the negatives read backwards, the rest forwards --
// and their k-th smallest is found like a merge-path diagonal, without making either.  One thread per (query, rank).
constexpr int NULL_ABS_RANKS = 4;
struct NullAbsQuery {
    const double *sorted;
    int64_t n;
    NullExpr e;                         // NX_SUBA / NX_SUBM / NX_SUBM2 only
    long long rank[NULL_ABS_RANKS];     // 0-based; outside [0, n): answered with NaN
};
__global__ __launch_bounds__(64) void k_null_abs_rank(const NullAbsQuery *__restrict__ qs, int nq, double *__restrict__ out) {
    const int j = blockIdx.x * 64 + threadIdx.x;
    if (j >= nq * NULL_ABS_RANKS) return;
    const NullAbsQuery &q = qs[j / NULL_ABS_RANKS];
    const long long k = q.rank[j % NULL_ABS_RANKS];
    if (k < 0 || k >= q.n) {
        out[j] = __longlong_as_double(0x7ff8000000000000ll);
        return;
    }
    const NullExpr e = q.e;
    const double *s = q.sorted;
    int64_t lo = 0, hi = q.n;
    while (lo < hi) {       // p = how many values are negative
        const int64_t mid = (lo + hi) >> 1;
        if (e(s[mid]) < 0.0) lo = mid + 1;
        else hi = mid;
    }
    const int64_t p = lo, lenA = p, lenB = q.n - p;
    // A(i) = -e(s[p - 1 - i]), i < lenA; B(i) = e(s[p + i]), i < lenB; both ascending
    lo = k > lenB ? k - lenB : 0;
    hi = k < lenA ? k : lenA;
    while (lo < hi) {       // how many of the k smallest come from A
        const int64_t mid = (lo + hi) >> 1;
        if (-e(s[p - 1 - mid]) <= e(s[p + (k - 1 - mid)])) lo = mid + 1;
        else hi = mid;
    }
    const int64_t a = lo, b = k - lo;
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    const double va = a < lenA ? -e(s[p - 1 - a]) : inf, vb = b < lenB ? e(s[p + b]) : inf;
    out[j] = fabs(va < vb ? va : vb);
}

}  // namespace csr
