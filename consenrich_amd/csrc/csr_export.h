// csr_export.h -- narrowPeak export, bit for bit what the reference makes of a solution mask's runs (peaks.py:5202-5567
// `_solutionToChromNarrowPeakRows` without a width policy and without a hierarchy; 4507-4576 `_solveParentConditionedSubpeakSegments`,
// 4789-4824 `_trimChildSegmentAroundSummit`).
//
// A PARENT is a run of the mask without a coordinate gap.  Its sub-peaks are the runs of the nested layer's dynamic programme
// (csr_nested.h: the same kernels, the same back-pointer words) in a third cost mode: ONE cost on all n + 1 boundaries, the
// caller's selection penalty, no floor and no run penalty.  All parents of all chains go through one call:
//
//   k_export_prep    one lane per parent: the leftmost arg-max of the scores (the required bin), the state the DP kernels start
//                    from, and whether the parent's scores or signal hold a non-finite value.
//   k_nested_dp_reg / k_nested_dp_wide   (csr_nested.h) for the parents of chains that split.
//   k_export_finish  one lane per parent: final pick, backtrace, `_parentConditionedSubpeakObjective` of the mask (selected scores
//                    compacted and summed in NumPy's order), and the number of children.
//   (host)           the exclusive prefix sum of the children counts: child k of parent j is peak base[j] + k, which is the
//                    reference's order without an atomic counter and without a sort of records.
//   k_export_child   one lane per child: its run of the parent's mask, the summit, the trim, and over the trimmed child the two
//                    medians (one heap sort each in the child's own bins of the work space: a median is two order statistics, so the
//                    result depends on the values alone), the two maxima and the filter flag.  The record goes out with ordinary
//                    vector stores.
//
// Signal and uncertainty are read through ExportTrack: a float64 array, or a float32 component of the reference-layout fit
// ((double) xs[:,0]; (double)(float) sqrt(Ps00), the values csr_batch_rocco_scores forms).  The per-parent and per-child routines
// are __host__ __device__: tests/native/narrowpeak_host_check.hip runs the same code on the CPU.
//
// What the reference does to these children under an active width policy -- `_forceMassiveSubpeakSegments`, the forced splits and
// the contraction of the widest ones -- is csr_cleanup.h: its plan kernel takes children as this file forms them (bins of a score
// array without a coordinate gap) and returns their final segments.  The second export pass then runs this file's call once more
// with the SEGMENTS as parents that do not split: k_export_child finishes a segment exactly as it finishes a child.
#pragma once
#include "csr_nested.h"
#include "csr_np_order.h"

namespace csr {

struct ExportTrack {
    const double *d;        // float64 values, or
    const float *f;         // float32 values `stride` apart
    int64_t stride;
    int32_t root;           // f: the float32 square root of the value
    int32_t reserved;
    CSR_HD bool present() const { return d != nullptr || f != nullptr; }
    CSR_HD double at(int64_t i) const {
        if (d) return d[i];
        const float v = f[i * stride];
        if (!root) return (double)v;
#if defined(__HIP_DEVICE_COMPILE__)
        return (double)(float)__dsqrt_rn((double)v);    // correctly rounded float32 sqrt (53 >= 2 * 24 + 2 bits), = np.sqrt
#else
        return (double)(float)::sqrt((double)v);
#endif
    }
};
struct ExportChain {
    double penalty, floor, multiplier;
    int32_t split, trim, filter, reserved;
};
enum { EXPORT_BAD_SCORES = 1, EXPORT_BAD_SIGNAL = 2, EXPORT_INFEASIBLE = 4 };
struct ExportParent {
    double penalized, boundary;     // of the parent's sub-peak solution (0 without a split)
    int32_t runs;                   // runs of the DP mask (0 without a split)
    int32_t count;                  // children: max(runs, 1)
    int32_t flags, reserved;
};
struct ExportArgs {
    NestedArgs na;                  // jobs, chains (internal = the boundary cost), scores, work, bt, wm, st
    const ExportChain *cfg;
    ExportTrack sig, unc;
    ExportParent *par;
    const int64_t *base;            // per parent: its first peak
    csr_export_peak *peaks;
    int64_t nParents, nPeaks;
};

CSR_HD bool export_keep(double score, double floor) { return score > floor; }
// np.median of w[0 .. m): sorts w
CSR_HD double export_median(double *w, int64_t m) {
    nested_heapsort(w, m);
    return (m & 1) ? w[m / 2] : (w[m / 2 - 1] + w[m / 2]) / 2.0;
}

// ---- peaks.py:4520-4527: the required bin, and what the DP kernels read of a region's state ------------------------------------
CSR_HD void export_prep_parent(const ExportArgs &a, int j) {
    const NestedJob jb = a.na.jobs[j];
    const ExportChain P = a.cfg[jb.chain];
    const double *x = a.na.scores + jb.off;
    NestedState s;
    s.floor = 0.0;
    s.penalty = P.penalty;
    s.extra = 0.0;
    s.runPenalty = 0.0;
    s.v0 = s.vM = 0.0;
    s.c0 = s.cM = 0;
    s.required = nested_argmax(x, jb.n);
    int flags = 0;
    for (int64_t i = 0; i < jb.n; ++i) {
        if (!np_finite(x[i])) flags |= EXPORT_BAD_SCORES;
        if (!np_finite(a.sig.at(jb.off + i))) flags |= EXPORT_BAD_SIGNAL;
    }
    a.na.st[j] = s;
    ExportParent r;
    r.penalized = r.boundary = 0.0;
    r.runs = 0;
    r.count = 1;
    r.flags = flags;
    r.reserved = 0;
    a.par[j] = r;
}

// ---- peaks.py:3657-3691 with a uniform cost, then 4528-4576: how many children ---------------------------------------------------
CSR_HD void export_finish_parent(const ExportArgs &a, int j) {
    const NestedJob jb = a.na.jobs[j];
    if (!a.cfg[jb.chain].split) return;
    const double cost = a.na.chains[jb.chain].internal;
    const NestedState s = a.na.st[j];
    const double *x = a.na.scores + jb.off;
    double *w = a.na.work + jb.off;
    unsigned char *m = a.na.wm + jb.off;
    const int64_t n = jb.n;
    const int M = jb.minRun;
    ExportParent r = a.par[j];
    // the final pick: max by (value, -count), the first of two equals
    const double last = s.vM - cost;
    const bool on = (last > s.v0) || (last == s.v0 && s.cM < s.c0);
    if (!np_finite(on ? last : s.v0)) {
        r.flags |= EXPORT_INFEASIBLE;
        for (int64_t i = 0; i < n; ++i) m[i] = 0;
        a.par[j] = r;
        return;
    }
    int st = on ? M : 0;
    unsigned long long word = 0ull;
    int64_t wi = -1;
    for (int64_t i = n - 1; i >= 0; --i) {
        m[i] = st > 0 ? 1 : 0;
        if (i / NESTED_WORD != wi) { wi = i / NESTED_WORD; word = a.na.bt[jb.word + wi]; }
        const unsigned int b = (unsigned int)(word >> (2 * (int)(i & (NESTED_WORD - 1)))) & 3u;
        if (st == 0) st = (b & 1u) ? M : 0;
        else if (st == M) st = (b & 2u) ? M : M - 1;
        else st -= 1;
    }
    int64_t cnt = 0;
    int runs = 0;
    bool prev = false;
    double bp = 0.0;
    for (int64_t i = 0; i < n; ++i) {
        const bool cur = m[i] != 0;
        if (cur != prev) {
            bp += cost;
            if (cur) ++runs;
        }
        if (cur) w[cnt++] = x[i];
        prev = cur;
    }
    if (prev) bp += cost;
    const double selected = np_sum_f(w, cnt, NpIdentity{});
    const double objective = (selected - bp) - 0.0 * (double)runs;
    r.penalized = objective - s.penalty * (double)cnt;
    r.boundary = bp;
    r.runs = runs;
    r.count = runs > 0 ? runs : 1;
    a.par[j] = r;
}

// ---- peaks.py:4552-4576 and 5382-5416 of one child ---------------------------------------------------------------------------
CSR_HD void export_child(const ExportArgs &a, int64_t t) {
    // the parent that holds peak t: the last one whose base is <= t
    int64_t lo = 0, hi = a.nParents - 1;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo + 1) / 2;
        if (a.base[mid] <= t) lo = mid; else hi = mid - 1;
    }
    const int j = (int)lo;
    const NestedJob jb = a.na.jobs[j];
    const ExportChain P = a.cfg[jb.chain];
    const ExportParent par = a.par[j];
    const double *x = a.na.scores + jb.off;
    const int64_t n = jb.n;
    // the child's bins of the parent: the k-th run of its mask, or all of it
    int64_t left = 0, right = n - 1;
    if (par.runs > 0) {
        const unsigned char *m = a.na.wm + jb.off;
        int64_t k = t - a.base[j], i = 0;
        while (i < n) {
            if (!m[i]) { ++i; continue; }
            int64_t e = i;
            while (e + 1 < n && m[e + 1]) ++e;
            if (k == 0) { left = i; right = e; break; }
            --k;
            i = e + 1;
        }
    }
    csr_export_peak p;
    p.chain = jb.chain;
    p.parent = j;
    p.num_subpeaks = par.runs > 0 ? par.runs : 1;
    p.flags = (par.runs > 0 && (par.runs > 1 || left > 0 || right < n - 1)) ? CSR_EXPORT_SPLIT_FROM_PARENT : 0;
    p.subpeak_objective = par.penalized;
    p.subpeak_boundary_penalty = par.boundary;
    // the summit: the leftmost arg-max of the signal over the untrimmed child
    int64_t summit = left;
    {
        double best = a.sig.at(jb.off + left);
        for (int64_t i = left + 1; i <= right; ++i) {
            const double v = a.sig.at(jb.off + i);
            if (v > best) { best = v; summit = i; }
        }
    }
    // the trim
    int64_t ts = left, te = right;
    if (P.trim && export_keep(x[summit], P.floor)) {
        ts = te = summit;
        while (ts > left && export_keep(x[ts - 1], P.floor)) --ts;
        while (te < right && export_keep(x[te + 1], P.floor)) ++te;
        if (ts != left || te != right) p.flags |= CSR_EXPORT_TRIMMED;
    }
    p.untrimmed_start = jb.start + left;
    p.untrimmed_end = jb.start + right;
    p.summit = jb.start + summit;
    p.start = jb.start + ts;
    p.end = jb.start + te;
    // over the trimmed child: both maxima, the median of the signal, the median of the finite uncertainty values
    double *w = a.na.work + jb.off + ts;
    const int64_t len = te - ts + 1;
    double mxState = a.sig.at(jb.off + ts), mxScore = x[ts];
    w[0] = mxState;
    for (int64_t i = 1; i < len; ++i) {
        const double v = a.sig.at(jb.off + ts + i), sc = x[ts + i];
        w[i] = v;
        mxState = v > mxState ? v : mxState;
        mxScore = sc > mxScore ? sc : mxScore;
    }
    p.max_state = mxState;
    p.max_score = mxScore;
    p.median_state = export_median(w, len);
    p.local_median_p = 0.0;
    if (P.filter && a.unc.present()) {
        int64_t cnt = 0;
        for (int64_t i = 0; i < len; ++i) {
            const double u = a.unc.at(jb.off + ts + i);
            if (np_finite(u)) w[cnt++] = u;
        }
        if (cnt > 0) {
            p.local_median_p = export_median(w, cnt);
            p.flags |= CSR_EXPORT_HAS_LOCAL_P;
            if (p.median_state < -P.multiplier * p.local_median_p) p.flags |= CSR_EXPORT_DROPPED_MEDIAN;
        }
    }
    a.peaks[t] = p;
}

// ---- kernels ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_export_prep(ExportArgs a, const int *__restrict__ order, int n) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t < n) export_prep_parent(a, order[t]);
}
__global__ __launch_bounds__(64) void k_export_finish(ExportArgs a, const int *__restrict__ order, int n) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t < n) export_finish_parent(a, order[t]);
}
__global__ __launch_bounds__(64) void k_export_child(ExportArgs a) {
    const int64_t t = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (t < a.nPeaks) export_child(a, t);
}

}  // namespace csr
