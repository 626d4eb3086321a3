// csr_cleanup.h -- the massive sub-peak clean-up, bit for bit what the reference makes of one child (peaks.py:4579-4786
// `_forceMassiveSubpeakSegments` with 3299-3352 `_bestMassiveSubpeakSplit` and 3355-3460 `_contractMassiveSubpeakSegment`).
//
// One work item is a CHILD: bins [start, end] of a score array that hold no coordinate gap, so that the n + 1 bin edges (an array,
// or origin + i * step) are everything the reference reads of `intervals` and `ends`.  One wavefront takes one child:
//
//   k_cleanup_plan   the reference's recursion with an explicit stack.  A child narrower than the threshold costs one width
//                    comparison and emits itself.  Per node of the recursion the order statistics (the split quantile, the median,
//                    the quartiles of the fallback scale) come from ONE cooperative sort of the node's scores, the MAD from one
//                    more of the absolute deviations: a merge network over the 64 lanes, in LDS up to CLEANUP_SORT_TILE values and
//                    beyond that in the node's own bins of the global work space (nodes are disjoint, so are their bins).  The
//                    maximum, the count and the k-th member of the tolerance mask and the first arg-min of |mid - centre| are
//                    wavefront reductions, the leftmost index winning.  Everything whose rounding depends on the order -- the
//                    running sums of the contrast, the gap scan, both expansion loops -- is a sequential walk in the reference's
//                    order: every lane makes the same walk over the same addresses (the loads are uniform, the control flow never
//                    diverges, nothing has to be broadcast) and lane 0 alone stores, with ordinary vector stores.
//
// The segments of a child go to its own CLEANUP_MAX_SEGMENTS records in left-to-right order; the host packs them with an exclusive
// prefix sum over the counts (the pattern of ExportArgs::base: no atomic counter, no sort of records).
//
// Everything is a template over a TEAM -- the wavefront on the device, one thread on the host -- and __host__ __device__:
// tests/native/cleanup_host_check.hip runs the same recursion, the same network and the same scans on the CPU.  A sort of finite
// doubles is determined by the values, apart from the order of -0.0 and +0.0, which NumPy's partition leaves open as well.  It can
// matter in one place only: an order statistic that is a zero may carry either sign, and where every score of a node is a zero too
// the sign travels into a zero deficit and from there into `z` (a +-0.0) of a split that is refused anyway (gain <= 0).
#pragma once
#include "csr_export.h"
#include "csr_np_order.h"

namespace csr {

#define CLEANUP_SORT_TILE 2048          // doubles of LDS per wavefront: 16 KiB, ten wavefronts' worth in a CU's 160 KiB
// A leaf of the recursion holds at least minBins >= ceil(0.05 L) bins of a child of L bins, a split is accepted only if both
// sides do, a contraction only shrinks a leaf, and leaves are disjoint: at most floor(L / ceil(0.05 L)) <= 20 segments.
#define CLEANUP_MAX_SEGMENTS 20
#define CLEANUP_MAX_BINS (((int64_t)1 << 31) - 2)     // of a call's score array: the wavefront's counts and indices are ints
#define CLEANUP_MIN_CHILD_BP 250.0      // _MASSIVE_SUBPEAK_MIN_CHILD_BP
#define CLEANUP_MIN_CHILD_FRACTION 0.05 // _MASSIVE_SUBPEAK_MIN_CHILD_FRACTION
static_assert(CLEANUP_MAX_SEGMENTS == CSR_CLEANUP_MAX_SEGMENTS, "csr_cleanup.h and consenrich_amd.h disagree");
static_assert(CLEANUP_SORT_TILE == CSR_CLEANUP_SORT_TILE, "csr_cleanup.h and consenrich_amd.h disagree");

struct CleanupCoords {
    const int64_t *edges;   // edge i of the score array (bin i is [edges[i], edges[i + 1])), or
    int64_t origin, step;   // origin + i * step
    int64_t shift;          // of a child whose edges are packed elsewhere: edge i is edges[i + shift]
    CSR_HD int64_t at(int64_t i) const { return edges ? edges[i + shift] : origin + i * step; }
    CSR_HD int64_t width(int64_t s, int64_t e) const {       // int(max(ends[e] - intervals[s], 0))
        const int64_t w = at(e + 1) - at(s);
        return w > 0 ? w : 0;
    }
    CSR_HD double mid(int64_t i) const { return 0.5 * ((double)at(i) + (double)at(i + 1)); }
};
struct CleanupArgs {
    const double *scores;
    double *work;                   // one double per bin of the score array
    CleanupCoords co;
    const csr_cleanup_child *kids;
    csr_cleanup_policy pol;
    csr_cleanup_segment *seg;       // CLEANUP_MAX_SEGMENTS per child
    csr_cleanup_counts *cnt;        // one per child
    csr_cleanup_node *node;         // one per child (the piece operations)
    int64_t nKids;
    int32_t op, reserved;
    // the batch call: per child the shift of its packed edges and its chain, per chain a policy (all null: co.shift and pol)
    const int64_t *shift;
    const int32_t *kidChain;
    const csr_cleanup_policy *pols;
};

// ---- the teams --------------------------------------------------------------------------------------------------------------------
struct CleanupHostTeam {
    double *buf;                    // CLEANUP_SORT_TILE doubles
    CSR_HD int lane() const { return 0; }
    CSR_HD int width() const { return 1; }
    CSR_HD void sync() const {}
    CSR_HD double *tile() const { return buf; }
    CSR_HD double max(double v) const { return v; }
    CSR_HD int64_t sum(int64_t v) const { return v; }
    CSR_HD void argmin(double &, int64_t &) const {}
    CSR_HD unsigned long long ballot(bool f) const { return f ? 1ull : 0ull; }
};
struct CleanupWaveTeam {
    double *buf;
    __device__ int lane() const { return (int)threadIdx.x; }
    __device__ int width() const { return 64; }
    __device__ void sync() const { __syncthreads(); }   // one wavefront per workgroup: orders its LDS and global accesses
    __device__ double *tile() const { return buf; }
    // butterflies; lane 0's result goes to all lanes, so that every lane holds the same bits (two zeros of either sign compare equal)
    __device__ double max(double v) const {
        for (int o = 32; o > 0; o >>= 1) {
            const double u = __shfl_xor(v, o);
            v = u > v ? u : v;
        }
        return __shfl(v, 0);
    }
    __device__ int64_t sum(int64_t v) const {
        int lo = (int)v;            // counts of bins: every host entry point refuses a score array of 2^31 - 1 bins or more (CLEANUP_MAX_BINS)
        for (int o = 32; o > 0; o >>= 1) lo += __shfl_xor(lo, o);
        return (int64_t)__shfl(lo, 0);
    }
    __device__ void argmin(double &v, int64_t &i) const {           // the smallest value, the leftmost index among equals
        int k = (int)i;
        for (int o = 32; o > 0; o >>= 1) {
            const double u = __shfl_xor(v, o);
            const int uk = __shfl_xor(k, o);
            if (u < v || (u == v && uk < k)) { v = u; k = uk; }
        }
        v = __shfl(v, 0);
        i = (int64_t)__shfl(k, 0);
    }
    __device__ unsigned long long ballot(bool f) const { return __ballot(f); }
};

// ---- the cooperative sort: ascending, any n --------------------------------------------------------------------------------------
// The merge network whose every compare-exchange puts the smaller value at the lower index (the first stage of a merge pairs i with
// its mirror in the block, the later ones i with i + j).  Values past n would be +inf at the top of every block and never move, so
// a pair that reaches past n is skipped and n needs no padding.
template <class T>
CSR_HD void cleanup_sort(const T &tm, double *w, int64_t n) {
    if (n < 2) return;
    int64_t half = 1;
    while (2 * half < n) half <<= 1;
    for (int64_t k = 2; (k >> 1) < n; k <<= 1) {
        const int64_t hk = k >> 1;
        for (int64_t t = tm.lane(); t < half; t += tm.width()) {
            const int64_t off = t & (hk - 1), i = 2 * (t - off) + off, l = 2 * (t - off) + (k - 1 - off);
            if (l < n) {
                const double a = w[i], b = w[l];
                if (a > b) { w[i] = b; w[l] = a; }
            }
        }
        tm.sync();
        for (int64_t j = hk >> 1; j > 0; j >>= 1) {
            for (int64_t t = tm.lane(); t < half; t += tm.width()) {
                const int64_t off = t & (j - 1), i = 2 * (t - off) + off, l = i + j;
                if (l < n) {
                    const double a = w[i], b = w[l];
                    if (a > b) { w[i] = b; w[l] = a; }
                }
            }
            tm.sync();
        }
    }
}
CSR_HD double cleanup_sorted_median(const double *w, int64_t m) {
    return (m & 1) ? w[m / 2] : (w[m / 2 - 1] + w[m / 2]) / 2.0;
}
// np.quantile(w, q), method "linear", of ascending w[0 .. m): the virtual index is (m - 1) q, the interpolation NumPy's _lerp
// (a + (b - a) t, and b - (b - a)(1 - t) from t = 0.5 on)
CSR_HD double cleanup_quantile(const double *w, int64_t m, double q) {
    const double vi = (double)(m - 1) * q;
    if (vi >= (double)(m - 1)) return w[m - 1];
    const double fl = ::floor(vi);
    const int64_t k = (int64_t)fl;
    const double a = w[k], b = w[k + 1], t = vi - fl, d = b - a;
    return t >= 0.5 ? b - d * (1.0 - t) : a + d * t;
}
CSR_HD double cleanup_clip01(double q) { return q < 0.0 ? 0.0 : (q > 1.0 ? 1.0 : q); }
CSR_HD double cleanup_sqrt(double v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __dsqrt_rn(v);
#else
    return ::sqrt(v);
#endif
}

// ---- the order statistics of a node: peaks.py:3310-3315 ---------------------------------------------------------------------------
// The scale falls back twice: the MAD (not finite or <= 1e-12), then IQR / 1.349, then 1.
struct CleanupStats {
    double low, scale;
};
template <class T>
CSR_HD CleanupStats cleanup_node_stats(const T &tm, const double *x, double *w, int64_t n, double q, bool wantScale) {
    CleanupStats r;
    tm.sync();      // whatever the lanes still read of the buffer's last use
    for (int64_t i = tm.lane(); i < n; i += tm.width()) w[i] = x[i];
    tm.sync();
    cleanup_sort(tm, w, n);
    r.low = cleanup_quantile(w, n, cleanup_clip01(q));
    r.scale = 1.0;
    if (!wantScale) return r;
    const double med = cleanup_sorted_median(w, n);
    const double iqr = cleanup_quantile(w, n, 0.75) - cleanup_quantile(w, n, 0.25);
    tm.sync();      // every lane has read the sorted scores
    for (int64_t i = tm.lane(); i < n; i += tm.width()) w[i] = fabs(x[i] - med);
    tm.sync();
    cleanup_sort(tm, w, n);
    double scale = 1.4826 * cleanup_sorted_median(w, n);
    if (!np_finite(scale) || scale <= 1.0e-12) scale = iqr / 1.349;
    if (!np_finite(scale) || scale <= 1.0e-12) scale = 1.0;
    r.scale = scale;
    tm.sync();
    return r;
}

// ---- peaks.py:3316-3352: the best low-score gap, a sequential walk ----------------------------------------------------------------
// prefix[k] is np.cumsum's running sum (its first term is contrast[0] itself, not 0.0 + contrast[0]); prefix[allowedStart] is a
// second running sum of the same additions, so no prefix array is stored.  range(2 minBins - 1, n - minBins) makes allowedStart >=
// minBins hold from the first step.  Strict < on the prefix and strict > on the gap sum: the first of two equals wins.
struct CleanupSplit {
    int64_t gs, ge;
    double baseline, scale, deficit, gain, z;
    int32_t found, gapBins;
};
CSR_HD CleanupSplit cleanup_split_scan(const double *x, int64_t n, int64_t minBins, double baseline, double scale, double cost) {
    CleanupSplit r;
    r.gs = r.ge = -1;
    r.baseline = baseline;
    r.scale = scale;
    r.deficit = r.gain = r.z = 0.0;
    r.found = 0;
    r.gapBins = 0;
    if (n < 3 * minBins) return r;
    double pa = 0.0;                    // prefix[allowedStart]
    for (int64_t i = 0; i < minBins; ++i) pa = i == 0 ? baseline - x[0] : pa + (baseline - x[i]);
    double pe = pa;                     // prefix[end + 1]
    for (int64_t i = minBins; i < 2 * minBins; ++i) pe += baseline - x[i];
    double bestSum = -INFINITY, bestPrefix = INFINITY;
    int64_t bestStart = -1, bestEnd = -1, bestIndex = -1;
    for (int64_t end = 2 * minBins - 1; end < n - minBins; ++end) {
        const int64_t as = end - minBins + 1;
        if (pa < bestPrefix) { bestPrefix = pa; bestIndex = as; }
        if (bestIndex >= 0) {
            const double gap = pe - bestPrefix;
            if (gap > bestSum) { bestSum = gap; bestStart = bestIndex; bestEnd = end; }
        }
        pa += baseline - x[as];
        pe += baseline - x[end + 1];    // (end + 1 <= n - minBins < n)
    }
    if (bestStart < 0 || bestEnd < bestStart) return r;
    r.found = 1;
    r.gs = bestStart;
    r.ge = bestEnd;
    r.gapBins = (int32_t)(bestEnd - bestStart + 1);
    r.deficit = bestSum;
    r.gain = bestSum - 2.0 * (cost > 0.0 ? cost : 0.0);
    r.z = bestSum / (scale * cleanup_sqrt((double)(r.gapBins > 1 ? r.gapBins : 1)));
    return r;
}

// ---- peaks.py:3355-3460: contraction of bins [s, s + n) to a core ------------------------------------------------------------------
struct CleanupCore {
    int64_t s, e, width;
    double floor;
    int32_t mode;       // 0: none
};
CSR_HD int cleanup_kth_bit(unsigned long long m, int r) {
    for (; r > 0; --r) m &= m - 1;
    return __builtin_ctzll(m);
}
template <class T>
CSR_HD CleanupCore cleanup_contract(const T &tm, const double *x, const CleanupCoords &co, int64_t s, int64_t n, double thr,
                                    int64_t minBins, double low) {
    CleanupCore r;
    r.s = r.e = -1;
    r.width = 0;
    r.floor = 0.0;
    r.mode = CSR_CLEANUP_MODE_NONE;
    const int64_t original = co.width(s, s + n - 1);
    if (!np_finite(thr) || thr <= 0.0) return r;
    // the maximum and its tolerance mask
    double mx = x[0];
    for (int64_t i = tm.lane(); i < n; i += tm.width()) mx = x[i] > mx ? x[i] : mx;
    mx = tm.max(mx);
    const double tol = 1.0e-12 > fabs(mx) * 1.0e-12 ? 1.0e-12 : fabs(mx) * 1.0e-12, bar = mx - tol;
    int64_t cnt = 0;
    for (int64_t i = tm.lane(); i < n; i += tm.width()) cnt += x[i] >= bar ? 1 : 0;
    cnt = tm.sum(cnt);
    // np.median of the mids of the mask: the mids ascend with the bins, so its two middle members are the mask's own
    const int64_t k1 = (cnt - 1) / 2, k2 = cnt / 2;
    int64_t i1 = 0, i2 = 0, seen = 0;
    for (int64_t base = 0; base < n; base += tm.width()) {
        const int64_t i = base + tm.lane();
        const unsigned long long m = tm.ballot(i < n && x[i] >= bar);
        const int64_t c = __builtin_popcountll(m);
        if (k1 >= seen && k1 < seen + c) i1 = base + cleanup_kth_bit(m, (int)(k1 - seen));
        if (k2 >= seen && k2 < seen + c) i2 = base + cleanup_kth_bit(m, (int)(k2 - seen));
        seen += c;
    }
    const double centre = cnt > 0 ? ((cnt & 1) ? co.mid(s + i1) : (co.mid(s + i1) + co.mid(s + i2)) / 2.0)
                                  : 0.5 * (double)(co.at(s) + co.at(s + n));
    // the first arg-min of |mid - centre|
    double dv = INFINITY;
    int64_t di = n;
    for (int64_t i = tm.lane(); i < n; i += tm.width()) {
        const double d = fabs(co.mid(s + i) - centre);
        if (d < dv) { dv = d; di = i; }
    }
    tm.argmin(dv, di);
    const int64_t c0 = di < n ? di : 0;
    // the adaptive core: tried only if maxScore - low > 1e-12 and the centre bin is kept
    const double dynamic = mx - low;
    if (np_finite(dynamic) && dynamic > 1.0e-12) {
        const double floor = low + 0.5 * dynamic;
        if (x[c0] >= floor) {
            int64_t left = c0, right = c0;
            while (left > 0 && x[left - 1] >= floor) --left;
            while (right + 1 < n && x[right + 1] >= floor) ++right;
            const int64_t width = co.width(s + left, s + right);
            if (right - left + 1 >= minBins && (double)width < thr && width < original) {
                r.s = s + left;
                r.e = s + right;
                r.width = width;
                r.floor = floor;
                r.mode = CSR_CLEANUP_MODE_ADAPTIVE_CORE;
                return r;
            }
        }
    }
    // the width-capped core: max over the tuples (score, -|mid - centre|, direction); equal score and distance pick the right side
    int64_t left = c0, right = c0;
    for (;;) {
        const bool canL = left > 0 && (double)co.width(s + left - 1, s + right) < thr;
        const bool canR = right + 1 < n && (double)co.width(s + left, s + right + 1) < thr;
        if (!canL && !canR) break;
        bool goRight = canR;
        if (canL && canR) {
            const double sl = x[left - 1], sr = x[right + 1];
            if (sl != sr) goRight = sr > sl;
            else {
                const double dl = -fabs(co.mid(s + left - 1) - centre), dr = -fabs(co.mid(s + right + 1) - centre);
                goRight = !(dl > dr);
            }
        }
        if (goRight) ++right; else --left;
    }
    const int64_t width = co.width(s + left, s + right);
    if (right - left + 1 < minBins || (double)width >= thr || width >= original) return r;
    r.s = s + left;
    r.e = s + right;
    r.width = width;
    r.mode = CSR_CLEANUP_MODE_WIDTH_CAPPED_CORE;
    return r;
}

// ---- peaks.py:4592-4786 of one child -------------------------------------------------------------------------------------------------
struct CleanupFrame {
    int64_t s, e;
    double gain, z;         // of the outermost accepted split above this node
    int32_t depth, outer, gapBins, reserved;
};
template <class T>
CSR_HD double *cleanup_buffer(const T &tm, const CleanupArgs &a, int64_t s, int64_t n) {
    return n <= CLEANUP_SORT_TILE ? tm.tile() : a.work + s;
}
template <class T>
CSR_HD void cleanup_plan_child(const T &tm, const CleanupArgs &a, int64_t c) {
    const csr_cleanup_child kid = a.kids[c];
    const csr_cleanup_policy P = a.pols ? a.pols[a.kidChain[c]] : a.pol;
    CleanupCoords co = a.co;
    if (a.shift) co.shift = a.shift[c];
    csr_cleanup_segment *out = a.seg + c * CLEANUP_MAX_SEGMENTS;
    const bool store = tm.lane() == 0;
    csr_cleanup_counts cn;
    cn.candidates = cn.splits = cn.segments_added = cn.evaluated = cn.contracts = cn.n_segments = cn.flags = cn.reserved = 0;
    auto emit = [&](const CleanupFrame &f, int64_t s, int64_t e, bool cand, bool applied, int mode, const CleanupSplit *sp,
                    const CleanupCore *core) {
        csr_cleanup_segment g;
        g.start = s;
        g.end = e;
        g.core_width_bp = core ? core->width : 0;
        g.gain = g.z = g.core_score_floor = 0.0;
        g.gap_bins = 0;
        g.mode = mode;
        g.flags = (cand ? CSR_CLEANUP_CANDIDATE : 0) | (applied ? CSR_CLEANUP_APPLIED : 0) | (core ? CSR_CLEANUP_HAS_CORE_WIDTH : 0);
        g.child = (int32_t)c;
        if (core && core->mode == CSR_CLEANUP_MODE_ADAPTIVE_CORE) {
            g.core_score_floor = core->floor;
            g.flags |= CSR_CLEANUP_HAS_CORE_FLOOR;
        }
        if (sp && sp->found) {      // a refused split's numbers travel into the contracted or kept segment
            g.gain = sp->gain;
            g.z = sp->z;
            g.gap_bins = sp->gapBins;
            g.flags |= CSR_CLEANUP_HAS_SPLIT;
        }
        if (f.outer) {              // below an accepted split: its numbers, and the outermost one's after all merges
            g.gain = f.gain;
            g.z = f.z;
            g.gap_bins = f.gapBins;
            g.flags |= CSR_CLEANUP_HAS_SPLIT | CSR_CLEANUP_CANDIDATE | CSR_CLEANUP_APPLIED;
            if (g.mode == CSR_CLEANUP_MODE_NONE) g.mode = CSR_CLEANUP_MODE_SPLIT;
        }
        if (s != kid.start || e != kid.end) g.flags |= CSR_CLEANUP_MOVED;
        if (store && cn.n_segments < CLEANUP_MAX_SEGMENTS) out[cn.n_segments] = g;
        if (cn.n_segments < CLEANUP_MAX_SEGMENTS) ++cn.n_segments;
        else cn.flags |= CSR_CLEANUP_OVERFLOW;
    };
    CleanupFrame root;
    root.s = kid.start;
    root.e = kid.end;
    root.gain = root.z = 0.0;
    root.depth = root.outer = root.gapBins = root.reserved = 0;
    const int64_t L = kid.end - kid.start + 1;
    const double *x0 = a.scores + kid.start;
    // not a candidate: one width comparison, and the child is its own segment
    if (!((double)co.width(kid.start, kid.end) >= P.threshold)) {
        emit(root, kid.start, kid.end, false, false, CSR_CLEANUP_MODE_NONE, nullptr, nullptr);
        if (store) a.cnt[c] = cn;
        return;
    }
    // a candidate with a non-finite score is the caller's (reachable only without the sub-peak split)
    {
        int64_t bad = 0;
        for (int64_t i = tm.lane(); i < L; i += tm.width()) bad += np_finite(x0[i]) ? 0 : 1;
        if (tm.sum(bad) > 0) {
            cn.flags |= CSR_CLEANUP_NONFINITE;
            emit(root, kid.start, kid.end, false, false, CSR_CLEANUP_MODE_NONE, nullptr, nullptr);
            if (store) a.cnt[c] = cn;
            return;
        }
    }
    // stepBP = max(int(np.median(positive bin widths of the ORIGINAL child)), 1), the same at every depth
    int64_t stepBP = 1;
    if (co.edges) {
        double *w = cleanup_buffer(tm, a, kid.start, L);
        int64_t pos = 0;
        for (int64_t i = tm.lane(); i < L; i += tm.width()) {
            const int64_t d = co.at(kid.start + i + 1) - co.at(kid.start + i);
            w[i] = d > 0 ? (double)d : INFINITY;
            pos += d > 0 ? 1 : 0;
        }
        pos = tm.sum(pos);
        tm.sync();
        cleanup_sort(tm, w, L);
        if (pos > 0) {
            const int64_t med = (int64_t)cleanup_sorted_median(w, pos);
            stepBP = med > 1 ? med : 1;
        }
        tm.sync();
    } else if (co.step > 1) {
        stepBP = co.step;
    }
    const int64_t minRun = P.min_run, byBP = (int64_t)ceil(CLEANUP_MIN_CHILD_BP / (double)stepBP),
                  byFrac = (int64_t)ceil((double)L * CLEANUP_MIN_CHILD_FRACTION);
    int64_t contractMin = minRun > byBP ? minRun : byBP;    // (no 5 % term)
    contractMin = contractMin > 1 ? contractMin : 1;
    const int64_t minBins = contractMin > byFrac ? contractMin : byFrac;
    const int maxDepth = P.max_depth > 0 ? P.max_depth : 0;
    CleanupFrame stack[CSR_CLEANUP_MAX_DEPTH + 2];      // depth-first, left before right: at most depth + 1 frames wait
    int sp = 0;
    stack[sp++] = root;
    while (sp > 0) {
        const CleanupFrame f = stack[--sp];
        const int64_t width = co.width(f.s, f.e), n = f.e - f.s + 1;
        const bool needsSplit = (double)width >= P.threshold;
        const bool needsContract = f.depth > 0 && (double)width >= P.contract_threshold;
        if (!needsSplit && !needsContract) {
            emit(f, f.s, f.e, false, false, CSR_CLEANUP_MODE_NONE, nullptr, nullptr);
            continue;
        }
        ++cn.candidates;
        ++cn.evaluated;
        const double *x = a.scores + f.s;
        double *w = cleanup_buffer(tm, a, f.s, n);
        const bool search = needsSplit && f.depth < maxDepth;
        const bool scan = search && n >= 3 * minBins;
        const CleanupStats st = cleanup_node_stats(tm, x, w, n, P.split_quantile, scan);
        CleanupSplit split;
        split.found = 0;
        if (scan) split = cleanup_split_scan(x, n, minBins, st.low, st.scale, P.boundary_cost);
        // refused on any of: None, gain <= 0, z < minSplitZ, a side shorter than minBins
        if (search && split.found && !(split.gain <= 0.0) && !(split.z < P.min_split_z) && split.gs >= minBins &&
            n - (split.ge + 1) >= minBins && sp + 2 <= CSR_CLEANUP_MAX_DEPTH + 2) {
            ++cn.splits;
            CleanupFrame kidF;
            kidF.depth = f.depth + 1;
            kidF.outer = 1;
            kidF.gain = f.outer ? f.gain : split.gain;
            kidF.z = f.outer ? f.z : split.z;
            kidF.gapBins = f.outer ? f.gapBins : split.gapBins;
            kidF.reserved = 0;
            kidF.s = f.s + split.ge + 1;
            kidF.e = f.e;
            stack[sp++] = kidF;     // the right side waits
            kidF.s = f.s;
            kidF.e = f.s + split.gs - 1;
            stack[sp++] = kidF;
            continue;
        }
        const CleanupCore core = cleanup_contract(tm, x, co, f.s, n, P.contract_threshold, contractMin, st.low);
        if (core.mode != CSR_CLEANUP_MODE_NONE) {
            ++cn.contracts;
            emit(f, core.s, core.e, true, true, core.mode, search ? &split : nullptr, &core);
        } else {
            emit(f, f.s, f.e, true, false, CSR_CLEANUP_MODE_UNSPLIT, search ? &split : nullptr, nullptr);
        }
    }
    cn.segments_added = cn.n_segments > 1 ? cn.n_segments - 1 : 0;
    if (store) a.cnt[c] = cn;
}

// ---- the pieces on their own: `_bestMassiveSubpeakSplit` of a child, `_contractMassiveSubpeakSegment` of a child -------------------
template <class T>
CSR_HD void cleanup_piece(const T &tm, const CleanupArgs &a, int64_t c) {
    const csr_cleanup_child kid = a.kids[c];
    const csr_cleanup_policy P = a.pols ? a.pols[a.kidChain[c]] : a.pol;
    const int64_t n = kid.end - kid.start + 1, minBins = P.min_run > 1 ? P.min_run : 1;
    const double *x = a.scores + kid.start;
    double *w = cleanup_buffer(tm, a, kid.start, n);
    CleanupCoords co = a.co;
    if (a.shift) co.shift = a.shift[c];
    csr_cleanup_node nd;
    memset(&nd, 0, sizeof(nd));
    if (a.op == CSR_CLEANUP_OP_SPLIT) {
        if (n >= 3 * minBins) {
            const CleanupStats st = cleanup_node_stats(tm, x, w, n, P.split_quantile, true);
            const CleanupSplit s = cleanup_split_scan(x, n, minBins, st.low, st.scale, P.boundary_cost);
            nd.found = s.found;
            nd.a = s.gs;
            nd.b = s.ge;
            nd.gap_bins = s.gapBins;
            nd.baseline = s.baseline;
            nd.scale = s.scale;
            nd.deficit = s.deficit;
            nd.gain = s.gain;
            nd.z = s.z;
        }
    } else {
        const CleanupStats st = cleanup_node_stats(tm, x, w, n, P.split_quantile, false);
        const CleanupCore core = cleanup_contract(tm, x, co, kid.start, n, P.contract_threshold, minBins, st.low);
        nd.found = core.mode != CSR_CLEANUP_MODE_NONE;
        nd.mode = core.mode;
        nd.a = core.s;
        nd.b = core.e;
        nd.width = core.width;
        nd.floor = core.floor;
    }
    if (tm.lane() == 0) a.node[c] = nd;
}

// ---- the host's share of a FORCE call: the exclusive prefix sum over the segment counts, the packed records, SPLIT_FROM_PARENT --------
enum { CLEANUP_PACK_OVERFLOW = 1, CLEANUP_PACK_NONFINITE = 2, CLEANUP_PACK_COUNT = 3, CLEANUP_PACK_CAPACITY = 4 };
inline int cleanup_pack(int64_t nk, const csr_cleanup_segment *seg, const csr_cleanup_counts *cnt, int64_t capacity,
                        csr_cleanup_segment *out, int64_t *total, int64_t *at) {
    int64_t base = 0;
    for (int64_t k = 0; k < nk; ++k) {
        const csr_cleanup_counts &c = cnt[k];
        *at = k;
        if (c.flags & CSR_CLEANUP_OVERFLOW) return CLEANUP_PACK_OVERFLOW;
        if (c.flags & CSR_CLEANUP_NONFINITE) return CLEANUP_PACK_NONFINITE;
        if (c.n_segments < 1 || c.n_segments > CLEANUP_MAX_SEGMENTS) return CLEANUP_PACK_COUNT;
        if (base + c.n_segments > capacity) return CLEANUP_PACK_CAPACITY;
        const csr_cleanup_segment *mine = seg + k * CLEANUP_MAX_SEGMENTS;
        bool moved = c.n_segments > 1;
        for (int s = 0; s < c.n_segments; ++s) moved = moved || (mine[s].flags & CSR_CLEANUP_MOVED) != 0;
        for (int s = 0; s < c.n_segments; ++s) {
            out[base + s] = mine[s];
            if (moved) out[base + s].flags |= CSR_CLEANUP_SPLIT_FROM_PARENT;
        }
        base += c.n_segments;
    }
    *total = base;
    return 0;
}

// ---- kernel: one wavefront per child ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_cleanup_plan(CleanupArgs a) {
    __shared__ double tile[CLEANUP_SORT_TILE];
    CleanupWaveTeam tm;
    tm.buf = tile;
    const int64_t c = blockIdx.x;
    if (c >= a.nKids) return;
    if (a.op == CSR_CLEANUP_OP_FORCE) cleanup_plan_child(tm, a, c);
    else cleanup_piece(tm, a, c);
}

}  // namespace csr
