// csr_segments.h -- multiscale candidate segments of a score track, bit for bit what the reference computes
// (pyx:9460-9669 `cMultiscaleCandidateSegmentStats`; called by peaks.py:2359-2481 on the observed track and on every null replay).
//
// A TRACK is one row of values of one chain (the score track, or one DWB draw).  Per track the native takes the float64 prefix of
// the values; per (track, view) the prefix of excess = max((x - threshold) / nullScale, 0); per (track, scale, view) -- a JOB --
// the runs of smooth > threshold bridged over at most `gap` false bins, their statistics, and the `cap` best of them.  The two
// prefixes are sums in index order and float64 addition is not associative; everything else is parallel:
//   k_seg_walk    ONE LANE per row walks it once, adding; SEG_WR rows of one chain per wavefront, staged through LDS in tiles of
//                 SEG_WT values with coalesced loads (lane = element), double-buffered through registers, read back transposed
//                 (lane = row) and written out as n + 1 prefix values per row, so that every later stage is a plain gather;
//   k_seg_excess  the excess values, division included, grid-wide, BEFORE their walk (the walks only add);
//   k_seg_count   per job: flag = smooth > threshold (smooth from two prefix values and one division) and the integer prefix
//                 count of the flags.  "No flag in [i - gap - 1, i)" is a difference of two counts: that is the reference's
//                 `i - lastTrue > gap + 1`, and the same test mirrored finds the last bin of a run;
//   k_seg_runs    per job: run starts and run ends from the counts, an integer scan of the starts, runs written in index order;
//   k_seg_stats   eight lanes per run: integrated / mean / score from two gathers of the excess prefix, the maximum of the excess
//                 by a segmented max (starting from 0.0 with `>`, so a NaN never enters, as in the reference), the minRun filter;
//   k_seg_select  per job over the cap: the cap-th largest score by a byte-wise radix select (as k_dwb_select), the counts above
//                 and at that value.  The job is FLAGGED when a candidate score is not finite or when rank cap and rank cap + 1
//                 hold the same value: then the reference's answer is whatever NumPy's introselect leaves, and the host asks NumPy;
//   k_seg_emit    per job: compaction of the chosen runs in start order into the output rows.
// A job's scans are made by ONE workgroup that steps through the bins SEG_CH at a time with a carry (jobs are plentiful: rows x
// scales x views per chain).  Nothing here waits on another workgroup: every dependency is a kernel boundary, every loop bound is
// known at launch or read from the result of an earlier kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "csr_np_order.h"

namespace csr {

constexpr int SEG_WT = 256;             // values per row and LDS tile of the walk (fetched 64 at a time: lane = element)
constexpr int SEG_WR = 16;              // rows per wavefront of the walk
constexpr int SEG_CH = 1024;            // bins per step of a job's scan (256 threads x 4)
constexpr int SEG_MAX_SCALES = 16;
constexpr int SEG_MAX_VIEWS = 16;
constexpr int SEG_STAT_BLOCKS = 16;     // workgroups of k_seg_stats per job (32 runs at a time each)

struct SegChain {
    int64_t off, n;         // bins [off, off + n) of a row of values
    int64_t pOff;           // n + 1 prefix values from pOff of a prefix row
    int64_t rOff;           // up to (n + 1) / 2 runs from rOff of a run row
    int nS, nV;
    int64_t w[SEG_MAX_SCALES];                      // scales clamped to [1, n]
    double thr[SEG_MAX_VIEWS], ns[SEG_MAX_VIEWS];   // thresholds; null scales raised to DBL_MIN
};
struct SegMeta {
    int nRuns, kept, capped, flagged, emit, pad;
};
// job j of a chain = (row * S + scale) * V + view; jobs per chain J = nRows * S * V; global job = chain * J + j
struct SegArgs {
    const SegChain *chains;
    const double *rows;
    int64_t rowLen;
    int nRows, S, V;
    int64_t pLen, rLen;
    double *prefix;             // [nRows][pLen]
    double *excess;             // [nRows * V][rowLen]
    double *exPrefix;           // [nRows * V][pLen]
    int *cnt;                   // [J][pLen]
    int *rStart, *rEnd;         // [J][rLen]
    unsigned char *keep;        // [J][rLen]: 1 = candidate, 3 = candidate that is emitted
    double *score, *integ, *mean, *mx;  // [J][rLen]
    int *runCount;              // [chains][J]
    SegMeta *meta;              // [chains][J]
    int minRun, gap, cap;
    const int64_t *jobBase;     // [chains][J]: first output row of the job
    int64_t *oStart, *oEnd;
    double *oScore, *oInteg, *oMean, *oMax;
};

struct SegWalkArgs {
    const SegChain *chains;
    const double *src;      // row r of a chain: src + r * srcLen + chain.off
    int64_t srcLen;
    double *dst;            // dst + r * dstLen + chain.pOff
    int64_t dstLen;
    int nWalk;              // rows per chain
    int perRow;             // 1, or V: row r is view r % V and is walked only if the chain has that view
};
__global__ __launch_bounds__(64) void k_seg_walk(SegWalkArgs a) {
    constexpr int K = SEG_WT / 64;
    __shared__ double sT[SEG_WR][SEG_WT + 1];
    const int64_t n = a.chains[blockIdx.y].n;
    const int nV = a.chains[blockIdx.y].nV;
    const int lane = threadIdx.x, g0 = blockIdx.x * SEG_WR;
    const int nl = a.nWalk - g0 < SEG_WR ? a.nWalk - g0 : SEG_WR;
    unsigned used = 0u;
    for (int r = 0; r < nl; ++r)
        if (a.perRow == 1 || (g0 + r) % a.perRow < nV) used |= 1u << r;
    const double *base = a.src + (int64_t)g0 * a.srcLen + a.chains[blockIdx.y].off;
    double *out = a.dst + (int64_t)g0 * a.dstLen + a.chains[blockIdx.y].pOff;
    const bool live = lane < SEG_WR && ((used >> lane) & 1u);
    double reg[SEG_WR * K];
    auto fetch = [&](int64_t t0) {
#pragma unroll
        for (int r = 0; r < SEG_WR; ++r)
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int64_t i = t0 + k * 64 + lane;
                reg[r * K + k] = (((used >> r) & 1u) && i < n) ? base[(int64_t)r * a.srcLen + i] : 0.0;
            }
    };
    auto stash = [&]() {
#pragma unroll
        for (int r = 0; r < SEG_WR; ++r)
#pragma unroll
            for (int k = 0; k < K; ++k) sT[r][k * 64 + lane] = reg[r * K + k];
    };
    if (live) out[(int64_t)lane * a.dstLen] = 0.0;
    double acc = 0.0;
    const int row = live ? lane : 0;
    fetch(0);
    for (int64_t t0 = 0; t0 < n; t0 += SEG_WT) {
        const int cnt = (int)(n - t0 < SEG_WT ? n - t0 : SEG_WT);
        stash();
        __syncthreads();
        if (t0 + SEG_WT < n) fetch(t0 + SEG_WT);        // in flight while this tile is walked
        if (live) {
            if (cnt == SEG_WT) {
#pragma unroll 32
                for (int j = 0; j < SEG_WT; ++j) {
                    acc = acc + sT[row][j];
                    sT[row][j] = acc;
                }
            } else
                for (int j = 0; j < cnt; ++j) {
                    acc = acc + sT[row][j];
                    sT[row][j] = acc;
                }
        }
        __syncthreads();
        for (int r = 0; r < nl; ++r) {
            if (!((used >> r) & 1u)) continue;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int64_t i = t0 + k * 64 + lane;
                if (i < n) out[(int64_t)r * a.dstLen + i + 1] = sT[r][k * 64 + lane];
            }
        }
        __syncthreads();
    }
}

// grid (ceil(longest / 256), nRows * V, chains)
__global__ __launch_bounds__(256) void k_seg_excess(SegArgs a) {
    const SegChain &ch = a.chains[blockIdx.z];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int r = blockIdx.y / a.V, v = blockIdx.y % a.V;
    if (i >= ch.n || v >= ch.nV) return;
    const double x = a.rows[(int64_t)r * a.rowLen + ch.off + i];
    double e = __ddiv_rn(x - ch.thr[v], ch.ns[v]);
    if (e < 0.0) e = 0.0;       // (a NaN stays a NaN)
    a.excess[(int64_t)blockIdx.y * a.rowLen + ch.off + i] = e;
}

struct SegJob {
    int r, s, v;
    int64_t j;
    bool idle;
};
__device__ __forceinline__ SegJob seg_job(const SegArgs &a, const SegChain &ch, int j) {
    SegJob q;
    q.j = j;
    q.v = j % a.V;
    q.s = (j / a.V) % a.S;
    q.r = j / (a.V * a.S);
    q.idle = q.s >= ch.nS || q.v >= ch.nV;
    return q;
}

__device__ __forceinline__ bool seg_flag(const double *x, const double *pf, int64_t n, int64_t w, int64_t i, double thr) {
    double sm;
    if (w <= 1 || n <= 1)
        sm = x[i];
    else {
        const int64_t leftPad = (w - 1) / 2, rightPad = w - 1 - leftPad;
        const int64_t s = i - leftPad < 0 ? 0 : i - leftPad;
        const int64_t e = i + rightPad + 1 > n ? n : i + rightPad + 1;
        sm = __ddiv_rn(pf[e] - pf[s], (double)w);
    }
    return sm > thr;
}

// grid (J, chains): cnt[i] = number of flags in [0, i), i = 0 .. n
__global__ __launch_bounds__(256) void k_seg_count(SegArgs a) {
    __shared__ int sW[4];
    const SegChain &ch = a.chains[blockIdx.y];
    const SegJob q = seg_job(a, ch, blockIdx.x);
    if (q.idle) return;
    const int64_t n = ch.n, w = ch.w[q.s];
    const double thr = ch.thr[q.v];
    const double *x = a.rows + (int64_t)q.r * a.rowLen + ch.off;
    const double *pf = a.prefix + (int64_t)q.r * a.pLen + ch.pOff;
    int *cnt = a.cnt + q.j * a.pLen + ch.pOff;
    const int t = threadIdx.x;
    if (t == 0) cnt[0] = 0;
    int carry = 0;
    for (int64_t b0 = 0; b0 < n; b0 += SEG_CH) {
        const int64_t i0 = b0 + t * 4;
        int f[4], sum = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            f[k] = (i0 + k < n && seg_flag(x, pf, n, w, i0 + k, thr)) ? 1 : 0;
            sum += f[k];
        }
        int total;
        int run = carry + wg_scan<256>(sum, sW, total) - sum;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (i0 + k < n) {
                run += f[k];
                cnt[i0 + k + 1] = run;
            }
        carry += total;
    }
}

// grid (J, chains): the runs of the job in index order
__global__ __launch_bounds__(256) void k_seg_runs(SegArgs a) {
    __shared__ int sW[4];
    const SegChain &ch = a.chains[blockIdx.y];
    const SegJob q = seg_job(a, ch, blockIdx.x);
    if (q.idle) return;
    const int64_t n = ch.n, G = a.gap;
    const int *cnt = a.cnt + q.j * a.pLen + ch.pOff;
    int *rs = a.rStart + q.j * a.rLen + ch.rOff, *re = a.rEnd + q.j * a.rLen + ch.rOff;
    const int t = threadIdx.x;
    int carry = 0;
    for (int64_t b0 = 0; b0 < n; b0 += SEG_CH) {
        const int64_t i0 = b0 + t * 4;
        int st[4], en[4], sum = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t i = i0 + k;
            st[k] = en[k] = 0;
            if (i < n) {
                const int c0 = cnt[i], c1 = cnt[i + 1];
                if (c1 != c0) {
                    const int64_t lo = i - G - 1 < 0 ? 0 : i - G - 1;
                    const int64_t hi = i + G + 2 > n ? n : i + G + 2;
                    st[k] = c0 == cnt[lo];
                    en[k] = cnt[hi] == c1;
                }
            }
            sum += st[k];
        }
        int total;
        int run = carry + wg_scan<256>(sum, sW, total) - sum;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (st[k]) rs[run] = (int)(i0 + k);
            run += st[k];
            if (en[k]) re[run - 1] = (int)(i0 + k);
        }
        carry += total;
    }
    if (t == 0) a.runCount[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = carry;
}

// grid (SEG_STAT_BLOCKS, J, chains); eight lanes per run
__global__ __launch_bounds__(256) void k_seg_stats(SegArgs a) {
    const SegChain &ch = a.chains[blockIdx.z];
    const SegJob q = seg_job(a, ch, blockIdx.y);
    if (q.idle) return;
    const int nr = a.runCount[(int64_t)blockIdx.z * gridDim.y + blockIdx.y];
    const int l = threadIdx.x & 7, groups = gridDim.x * 32;
    const int64_t ro = q.j * a.rLen + ch.rOff;
    const double *ex = a.excess + ((int64_t)q.r * a.V + q.v) * a.rowLen + ch.off;
    const double *ep = a.exPrefix + ((int64_t)q.r * a.V + q.v) * a.pLen + ch.pOff;
    for (int k = blockIdx.x * 32 + (threadIdx.x >> 3); k < nr; k += groups) {
        const int s = a.rStart[ro + k], e = a.rEnd[ro + k];
        double m = 0.0;
        for (int j = s + l; j <= e; j += 8) {
            const double v = ex[j];
            if (v > m) m = v;
        }
#pragma unroll
        for (int d = 1; d < 8; d <<= 1) {
            const double o = __shfl_xor(m, d, 64);
            if (o > m) m = o;
        }
        if (l == 0) {
            const int len = e - s + 1;
            const bool kept = len >= a.minRun;
            a.keep[ro + k] = kept ? 1 : 0;
            if (kept) {
                const double integ = ep[e + 1] - ep[s];
                a.integ[ro + k] = integ;
                a.mean[ro + k] = __ddiv_rn(integ, (double)len);
                a.score[ro + k] = __ddiv_rn(integ, __dsqrt_rn((double)len));
                a.mx[ro + k] = m;
            }
        }
    }
}

// grid (J, chains): which candidates of the job are emitted
__global__ __launch_bounds__(256) void k_seg_select(SegArgs a) {
    __shared__ unsigned int h[256];
    __shared__ int sKept, sBad, sGreater, sEqual;
    __shared__ unsigned long long pre;
    __shared__ long long rk;
    const SegChain &ch = a.chains[blockIdx.y];
    const SegJob q = seg_job(a, ch, blockIdx.x);
    if (q.idle) return;
    const int64_t job = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    const int nr = a.runCount[job], t = threadIdx.x;
    const int64_t ro = q.j * a.rLen + ch.rOff;
    unsigned char *keep = a.keep + ro;
    const double *score = a.score + ro;
    if (t == 0) sKept = sBad = sGreater = sEqual = 0;
    __syncthreads();
    int kc = 0, bad = 0;
    for (int k = t; k < nr; k += 256)
        if (keep[k]) {
            ++kc;
            if (!isfinite(score[k])) bad = 1;
        }
    if (kc) atomicAdd(&sKept, kc);
    if (bad) atomicOr(&sBad, 1);
    __syncthreads();
    const int K = sKept;
    if (a.cap <= 0 || K <= a.cap) {
        for (int k = t; k < nr; k += 256)
            if (keep[k]) keep[k] = 3;
        if (t == 0) a.meta[job] = SegMeta{nr, K, 0, 0, K, 0};
        return;
    }
    // the cap-th largest = ascending rank K - cap of the candidates' keys (x + 0.0: both zeros are one value, as for NumPy)
    if (t == 0) {
        pre = 0ull;
        rk = (long long)K - a.cap;
    }
    for (int pass = 0; pass < 8; ++pass) {
        h[t] = 0u;
        __syncthreads();
        const int shift = 56 - 8 * pass;
        const unsigned long long want = pre;
        for (int k = t; k < nr; k += 256)
            if (keep[k]) {
                const unsigned long long key = np_key(score[k] + 0.0);
                const unsigned long long hi = pass == 0 ? 0ull : key >> (shift + 8);
                if (hi == want) atomicAdd(&h[(unsigned int)(key >> shift) & 255u], 1u);
            }
        __syncthreads();
        if (t == 0) {
            long long before;
            const int digit = radix_pick_digit(h, rk, &before);
            pre = (pre << 8) | (unsigned long long)digit;
            rk -= before;
        }
        __syncthreads();
    }
    const unsigned long long T = pre;
    int g = 0, e = 0;
    for (int k = t; k < nr; k += 256)
        if (keep[k]) {
            const unsigned long long key = np_key(score[k] + 0.0);
            g += key > T;
            e += key == T;
        }
    if (g) atomicAdd(&sGreater, g);
    if (e) atomicAdd(&sEqual, e);
    __syncthreads();
    const bool flagged = sBad != 0 || sEqual > a.cap - sGreater;
    if (!flagged)
        for (int k = t; k < nr; k += 256)
            if (keep[k] && np_key(score[k] + 0.0) >= T) keep[k] = 3;
    if (t == 0) a.meta[job] = SegMeta{nr, K, 1, flagged ? 1 : 0, flagged ? 0 : a.cap, 0};
}

// grid (J, chains): the emitted candidates of the job, in start order, to output rows jobBase[job] ..
__global__ __launch_bounds__(256) void k_seg_emit(SegArgs a) {
    __shared__ int sW[4];
    const SegChain &ch = a.chains[blockIdx.y];
    const SegJob q = seg_job(a, ch, blockIdx.x);
    if (q.idle) return;
    const int64_t job = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    const SegMeta m = a.meta[job];
    if (m.emit <= 0) return;
    const int64_t ro = q.j * a.rLen + ch.rOff, base = a.jobBase[job];
    const int t = threadIdx.x;
    int carry = 0;
    for (int k0 = 0; k0 < m.nRuns; k0 += 256) {
        const int k = k0 + t;
        const bool f = k < m.nRuns && a.keep[ro + k] == 3;
        int total;
        const int pos = carry + wg_rank256(f, sW, &total);      // (a 0/1 flag: the ballot rank costs less than the scan)
        if (f && pos < m.emit) {
            const int64_t o = base + pos;
            a.oStart[o] = a.rStart[ro + k];
            a.oEnd[o] = a.rEnd[ro + k];
            a.oScore[o] = a.score[ro + k];
            a.oInteg[o] = a.integ[ro + k];
            a.oMean[o] = a.mean[ro + k];
            a.oMax[o] = a.mx[ro + k];
        }
        carry += total;
    }
}

}  // namespace csr
