// csr_broad.h -- broad mode, the per-bin arithmetic of two steps of the reference, bit for bit:
//   peaks.py:1898-2005 `_mergeBroadRunsByObjective`     the score of the gap between two runs,
//   peaks.py:5606-5818 `_solutionToChromBroadPeakRows`  the numbers of one broad parent.
//
// A GAP is bins [start, start + n) of a score array; its score is np.sum(np.where(ex < 0, f * ex, ex)) with ex = score - penalty,
// in NumPy's order (csr_np_order.h), and 0.0 where no bin lies between the runs.  In the reference every branch of the walk over
// the runs moves `activeEnd` to the next run's end, so a gap's decision depends on that gap alone: all gaps of a call are summed at
// once, one lane per gap: a gap is tens of bins.  The drop-in sends only the gaps that passed the host's distance and blacklist
// tests; the resident form sums the gap behind every kept run before the host has tested anything, so its caller passes the
// largest number of bins a gap within maxGapBP can hold and longer gaps are left unsummed (BroadRunArgs::maxGapBins).
//
// A PARENT is bins [start, end] of one chain without a coordinate gap; parents are thousands of bins long, so one WAVEFRONT takes
// one parent, all parents of all chains in one launch:
//   the signal goes to the parent's buffer once (LDS up to CLEANUP_SORT_TILE values, beyond that the parent's own bins of the
//   global work space: parents are disjoint, so are their bins), with the maximum, the leftmost arg-max, the maximum of the scores
//   and the non-finite flag as wavefront reductions on the way; np.sum of the signal and of the scores are walks in NumPy's order
//   that every lane makes over the same addresses (uniform loads, no divergence, nothing to broadcast); the median comes from the
//   cooperative sort of csr_cleanup.h; the finite uncertainty values are compacted in order with a ballot and sorted the same way.
//   Lane 0 stores the record with ordinary vector stores.  The parent's bins of the parent mask are set on the way.
//
// Signal and uncertainty are read through ExportTrack (csr_export.h).  Everything is a template over a TEAM and __host__
// __device__: tests/native/broad_host_check.hip runs the same code on the CPU -- the gap sums, the parents, and the support runs
// (broad_run_flags, broad_is_break, broad_env, broad_run_gap under a serial scan in place of the workgroup scans).  The zero caveat of csr_cleanup.h holds: a maximum
// or a median that is a zero may carry either sign where both zeros occur.
#pragma once
#include "csr_cleanup.h"

namespace csr {

enum { BROAD_HAS_LOCAL_P = 1, BROAD_DROPPED_MEDIAN = 2, BROAD_NONFINITE = 4 };
static_assert(BROAD_HAS_LOCAL_P == CSR_BROAD_HAS_LOCAL_P && BROAD_DROPPED_MEDIAN == CSR_BROAD_DROPPED_MEDIAN &&
              BROAD_NONFINITE == CSR_BROAD_NONFINITE, "csr_broad.h and consenrich_amd.h disagree");

// ---- gaps ----------------------------------------------------------------------------------------------------------------------------
struct BroadDip {
    double penalty, fraction;
    CSR_HD double operator()(double x) const {
        const double ex = x - penalty;
        return ex < 0.0 ? fraction * ex : ex;
    }
};
struct BroadGapArgs {
    const double *scores;
    const int64_t *start, *len;     // per gap: its first bin and its number of bins (0: none)
    double penalty, fraction;
    double *sums;
    int64_t nGaps;
};
CSR_HD void broad_gap_sum(const BroadGapArgs &a, int64_t g) {
    const int64_t n = a.len[g];
    BroadDip f;
    f.penalty = a.penalty;
    f.fraction = a.fraction;
    a.sums[g] = n > 0 ? np_sum_f(a.scores + a.start[g], n, f) : 0.0;
}

// ---- parents -------------------------------------------------------------------------------------------------------------------------
struct BroadChain {
    double multiplier;
    int32_t filter, reserved;
};
struct BroadJob {
    int64_t off, n, start;          // first bin in the call's arena, bins, first bin in the chain
    int32_t chain, reserved;
};
struct BroadArgs {
    const BroadJob *jobs;
    const BroadChain *cfg;
    const double *scores;
    ExportTrack sig, unc;
    double *work;                   // one double per bin of the arena
    unsigned char *mask;            // the parent mask (zeroed by the caller), or null
    csr_broad_parent *rec;
    int64_t nParents;
};

struct BroadHostTeam : CleanupHostTeam {
    CSR_HD void argmax(double &, int64_t &) const {}
    CSR_HD int below(unsigned long long) const { return 0; }
};
struct BroadWaveTeam : CleanupWaveTeam {
    __device__ void argmax(double &v, int64_t &i) const {           // the largest value, the leftmost index among equals
        int k = (int)i;
        for (int o = 32; o > 0; o >>= 1) {
            const double u = __shfl_xor(v, o);
            const int uk = __shfl_xor(k, o);
            if (u > v || (u == v && uk < k)) { v = u; k = uk; }
        }
        v = __shfl(v, 0);
        i = (int64_t)__shfl(k, 0);
    }
    __device__ int below(unsigned long long m) const { return __popcll(m & ((1ull << threadIdx.x) - 1ull)); }
};

template <class T>
CSR_HD void broad_parent(const T &tm, const BroadArgs &a, int64_t j) {
    const BroadJob jb = a.jobs[j];
    const BroadChain P = a.cfg[jb.chain];
    const int64_t n = jb.n;
    const double *x = a.scores + jb.off;
    double *w = n <= CLEANUP_SORT_TILE ? tm.tile() : a.work + jb.off;
    // the signal into the buffer; maxima, the leftmost arg-max, the non-finite flag
    double mxState = a.sig.at(jb.off), mxScore = x[0];
    int64_t summit = 0, bad = 0;
    for (int64_t i = tm.lane(); i < n; i += tm.width()) {
        const double v = a.sig.at(jb.off + i), sc = x[i];
        w[i] = v;
        if (v > mxState) { mxState = v; summit = i; }       // (a lane's indices ascend: its first maximum stays)
        mxScore = sc > mxScore ? sc : mxScore;
        bad += (np_finite(v) && np_finite(sc)) ? 0 : 1;
        if (a.mask) a.mask[jb.off + i] = 1;
    }
    // a lane that met nothing above sig[0] holds (sig[0], 0), which is the leftmost candidate of all
    tm.argmax(mxState, summit);
    mxScore = tm.max(mxScore);
    bad = tm.sum(bad);
    tm.sync();
    csr_broad_parent r;
    r.start = jb.start;
    r.end = jb.start + n - 1;
    r.summit = jb.start + summit;
    r.chain = jb.chain;
    r.flags = bad > 0 ? BROAD_NONFINITE : 0;
    r.max_state = mxState;
    r.max_score = mxScore;
    // np.mean: np.sum in NumPy's order over the count; the same walk in every lane
    r.mean_state = np_sum_f(w, n, NpIdentity{}) / (double)n;
    r.mean_score = np_sum_f(x, n, NpIdentity{}) / (double)n;
    tm.sync();      // every lane has read the unsorted signal
    cleanup_sort(tm, w, n);
    r.median_state = cleanup_sorted_median(w, n);
    r.local_median_p = 0.0;
    if (P.filter && a.unc.present()) {
        tm.sync();  // every lane has read the sorted signal
        int64_t cnt = 0;
        for (int64_t base = 0; base < n; base += tm.width()) {
            const int64_t i = base + tm.lane();
            const double u = i < n ? a.unc.at(jb.off + i) : 0.0;
            const bool keep = i < n && np_finite(u);
            const unsigned long long m = tm.ballot(keep);
            if (keep) w[cnt + tm.below(m)] = u;     // (cnt + rank <= i: inside the buffer)
            cnt += __builtin_popcountll(m);
        }
        tm.sync();
        if (cnt > 0) {
            cleanup_sort(tm, w, cnt);
            r.local_median_p = cleanup_sorted_median(w, cnt);
            r.flags |= BROAD_HAS_LOCAL_P;
            if (r.median_state < -P.multiplier * r.local_median_p) r.flags |= BROAD_DROPPED_MEDIAN;
        }
    }
    if (tm.lane() == 0) a.rec[j] = r;
}

// ---- support runs of one chain's resident tracks (peaks.py:6884-6908): flag -> scan -> compaction, twice -------------------------------
// The predicate is scores >= threshold, or (the fallback) weak | strong.  Bin i starts a run when it is set and bin i - 1 is not, or a
// coordinate break lies between them; it ends one the same way to the right.  The k-th start and the k-th end belong to the same run
// (counts travel as starts | ends << 32, the shape of k_rocco_run_*).  A run TOUCHES when one of its bins is in weak | strong: one
// wavefront per run.  The touching runs are compacted in order by a second scan, over runs; the gap sum to the next kept run is
// one lane per kept run.  No atomic counter, no sort of records.
struct BroadRunArgs {
    const double *scores;           // the chain's
    const unsigned char *weak, *strong;
    const int64_t *breaks;          // ascending bins g: a cut between g and g + 1
    int64_t nBreaks, n;
    double threshold, penalty, fraction;
    int64_t maxGapBins;             // a longer gap is not summed (the host's distance test blocks it); < 0: no bound
    int32_t envelope, chain;
    unsigned long long *blockSum;   // ceil(n / 1024) + 1
    int64_t *starts, *ends;         // nRuns each
    unsigned char *touch;           // nRuns
    unsigned long long *keepSum;    // ceil(nRuns / 1024) + 1
    csr_broad_run *rec;             // the kept runs
    int64_t nRuns;
};
CSR_HD bool broad_env(const BroadRunArgs &a, int64_t i) { return (a.weak[i] | a.strong[i]) != 0; }
CSR_HD bool broad_pred(const BroadRunArgs &a, int64_t i) { return a.envelope ? broad_env(a, i) : a.scores[i] >= a.threshold; }
CSR_HD bool broad_is_break(const BroadRunArgs &a, int64_t g) {
    int64_t lo = 0, hi = a.nBreaks;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (a.breaks[mid] < g) lo = mid + 1; else hi = mid;
    }
    return lo < a.nBreaks && a.breaks[lo] == g;
}
CSR_HD unsigned long long broad_run_flags(const BroadRunArgs &a, int64_t i) {
    if (i >= a.n || !broad_pred(a, i)) return 0ull;
    const bool st = i == 0 || !broad_pred(a, i - 1) || broad_is_break(a, i - 1);
    const bool en = i == a.n - 1 || !broad_pred(a, i + 1) || broad_is_break(a, i);
    return (st ? 1ull : 0ull) | (en ? (1ull << 32) : 0ull);
}
CSR_HD void broad_run_gap(const BroadRunArgs &a, int64_t g, int64_t kept) {
    double sum = 0.0;
    if (g + 1 < kept) {
        const int64_t first = a.rec[g].end + 1, len = a.rec[g + 1].start - first;
        BroadDip f;
        f.penalty = a.penalty;
        f.fraction = a.fraction;
        if (len > 0 && (a.maxGapBins < 0 || len <= a.maxGapBins)) sum = np_sum_f(a.scores + first, len, f);
    }
    a.rec[g].gap_sum = sum;
}

// ---- kernels -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void k_broad_run_count(BroadRunArgs a) {
    __shared__ unsigned long long sh[16];
    const int64_t i = (int64_t)blockIdx.x * 1024 + threadIdx.x;
    unsigned long long total;
    wg_scan<1024>(broad_run_flags(a, i), sh, total);
    if (threadIdx.x == 1023) a.blockSum[blockIdx.x] = total;
}
// exclusive scan of sums[0 .. nb) in place, the total to sums[nb]: one workgroup (the shape of k_rocco_run_scan)
__global__ __launch_bounds__(1024) void k_broad_scan(unsigned long long *sums, int64_t nb) {
    __shared__ unsigned long long sh[16];
    __shared__ unsigned long long carry;
    if (threadIdx.x == 0) carry = 0ull;
    __syncthreads();
    for (int64_t b0 = 0; b0 < nb; b0 += 1024) {
        const int64_t b = b0 + threadIdx.x;
        const unsigned long long v = b < nb ? sums[b] : 0ull;
        unsigned long long total;
        const unsigned long long inc = wg_scan<1024>(v, sh, total);
        const unsigned long long c = carry;
        if (b < nb) sums[b] = c + inc - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry = c + total;
        __syncthreads();
    }
    if (threadIdx.x == 0) sums[nb] = carry;
}
__global__ __launch_bounds__(1024) void k_broad_run_write(BroadRunArgs a) {
    __shared__ unsigned long long sh[16];
    const int64_t i = (int64_t)blockIdx.x * 1024 + threadIdx.x;
    const unsigned long long fl = broad_run_flags(a, i);
    unsigned long long total;
    const unsigned long long ex = wg_scan<1024>(fl, sh, total) - fl + a.blockSum[blockIdx.x];
    const int64_t ks = (int64_t)(ex & 0xffffffffull), ke = (int64_t)(ex >> 32);
    if ((fl & 1ull) && ks < a.nRuns) a.starts[ks] = i;
    if ((fl >> 32) && ke < a.nRuns) a.ends[ke] = i;
}
__global__ __launch_bounds__(64) void k_broad_run_touch(BroadRunArgs a) {
    const int64_t r = blockIdx.x;
    if (r >= a.nRuns) return;
    const int64_t s = a.starts[r], e = a.ends[r];
    bool any = false;
    for (int64_t i = s + threadIdx.x; i <= e; i += 64) any = any || broad_env(a, i);
    const unsigned long long m = __ballot(any);
    if (threadIdx.x == 0) a.touch[r] = m != 0ull ? 1 : 0;
}
__global__ __launch_bounds__(1024) void k_broad_keep_count(BroadRunArgs a) {
    __shared__ unsigned long long sh[16];
    const int64_t r = (int64_t)blockIdx.x * 1024 + threadIdx.x;
    unsigned long long total;
    wg_scan<1024>((unsigned long long)(r < a.nRuns && a.touch[r] ? 1 : 0), sh, total);
    if (threadIdx.x == 1023) a.keepSum[blockIdx.x] = total;
}
__global__ __launch_bounds__(1024) void k_broad_keep_write(BroadRunArgs a) {
    __shared__ unsigned long long sh[16];
    const int64_t r = (int64_t)blockIdx.x * 1024 + threadIdx.x;
    const unsigned long long fl = r < a.nRuns && a.touch[r] ? 1ull : 0ull;
    unsigned long long total;
    const unsigned long long pos = wg_scan<1024>(fl, sh, total) - fl + a.keepSum[blockIdx.x];
    if (fl) {       // (pos < the kept count <= nRuns: the records hold nRuns)
        csr_broad_run q;
        q.start = a.starts[r];
        q.end = a.ends[r];
        q.gap_sum = 0.0;
        q.chain = a.chain;
        q.reserved = 0;
        a.rec[pos] = q;
    }
}
__global__ __launch_bounds__(64) void k_broad_run_gaps(BroadRunArgs a, int64_t nb) {
    const int64_t kept = (int64_t)a.keepSum[nb];
    const int64_t g = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (g < kept) broad_run_gap(a, g, kept);
}
__global__ __launch_bounds__(64) void k_broad_gap_sums(BroadGapArgs a) {
    const int64_t g = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (g < a.nGaps) broad_gap_sum(a, g);
}
__global__ __launch_bounds__(64) void k_broad_parents(BroadArgs a) {
    __shared__ double tile[CLEANUP_SORT_TILE];
    BroadWaveTeam tm;
    tm.buf = tile;
    const int64_t j = blockIdx.x;
    if (j >= a.nParents) return;
    broad_parent(tm, a, j);
}

}  // namespace csr
