// csr_nested.h -- nested ROCCO refinement, bit for bit what the reference decides (peaks.py:3519-3720
// `_solveParentConditionedSubpeaks`, 2133-2160 `_parentConditionedSubpeakObjective`, 2089-2114 `_nestedSoftSelectionPenalty`,
// and the per-region body of `_refineNestedROCCOSolution`, peaks.py:4042-4172).
//
// One LAYER processes every frontier region of every chain at once.  A region is a short, strictly sequential float64
// recursion over minRun + 1 states whose comparison (`value > best + 1e-12, or |difference| <= 1e-12 and a smaller count`)
// is no total order: the ORDER of the candidate updates is part of the result, and no re-associated scan reproduces it.
// So a region is one lane that runs the recursion as written (the library is built with -ffp-contract=off), and the
// parallelism is the thousands of regions of a layer.  The host sorts the regions by length so that the lanes of a
// wavefront finish together.  Three launches:
//
//   k_nested_prep    one lane per region: the leftmost arg-max of the raw scores (the required bin), ONE sort of the region's
//                    scores in work space, and the order statistics read at its ranks -- the 25 % floor (layers >= 2) and the
//                    inter-quartile spread of the strictly positive solver scores (x - floor is monotone in x, so they are a
//                    suffix of the same order) -- with both branches of NumPy's `_lerp`.
//   k_nested_dp_reg  one lane per region, minRun <= NESTED_REG_STATES: the states live in registers; states 2 .. minRun have
//                    one predecessor each and are a shift register.  Only state 0 (stayed off, or a run just closed) and
//                    state minRun (grew into it, or stayed in it) choose: two back-pointer bits per bin, 32 bins to a 64-bit
//                    word written with an ordinary vector store, as the ROCCO backtrace packs them.
//   k_nested_dp_wide one workgroup per region, minRun up to NESTED_MAX_MIN_RUN: the states are the lanes, the shift goes
//                    through double-buffered LDS, one barrier per bin.
//   k_nested_finish  one lane per region: the final pick, the backtrace, the selected solver scores compacted into work space and
//                    summed in NumPy's order (np_sum_f of csr_np_order.h), the sequential boundary sum and run
//                    count, the same for the all-ones mask, split gain, the gates and the decision; every candidate run with its
//                    own required bin, raw maximum and NumPy-order score sum; and, when the region splits or shrinks, its bins
//                    of the solution mask.
//
// The per-region routines are __host__ __device__: tests/native/nested_host_check.hip runs the same code on the CPU.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "csr_np_order.h"

namespace csr {

constexpr int NESTED_WORD = 32;             // bins per back-pointer word
constexpr int NESTED_REG_STATES = 8;        // largest minRun of the register kernel
constexpr int NESTED_MAX_MIN_RUN = CSR_NESTED_MAX_MIN_RUN;
constexpr int NESTED_WIDE_T = 256;          // threads of the states-as-lanes kernel (>= NESTED_MAX_MIN_RUN)
constexpr double NESTED_EDGE = 1.0e-12;     // cost of a region's two outer boundaries
constexpr double NESTED_EPS = 1.0e-12;      // tolerance of the value comparison

// one region [off, off + n) of the concatenated arrays
struct NestedJob {
    int64_t off, n;
    int64_t start;          // the region's first bin within its chain (what the records report)
    int64_t word;           // first back-pointer word of the region
    int64_t required;       // solve mode: the required bin (-1: none); layer mode: set by k_nested_prep
    const double *costs;    // solve mode: n + 1 boundary costs; layer mode: nullptr (edge / internal)
    int32_t minRun;         // already clamped to [1, n]
    int32_t chain;          // row of the parameter table
    int32_t uniform;        // export mode (csr_export.h): `internal` is the cost of all n + 1 boundaries, the outer ones included
    int32_t reserved;
};
struct NestedChain {
    double internal;        // max(0.25 gamma, 1000 edge): cost of an inner boundary, and the run penalty
    double base;            // the layer's base selection penalty
    double scale;           // the layer's budget scale
    int32_t useFloor;       // layers >= 2: the solver scores are x - Q25(x)
    int32_t commitAlways;   // solve mode: the mask is the output whatever the decision
};
// what a region's lanes hand to each other
struct NestedState {
    double floor, penalty, extra, runPenalty;
    double v0, vM;          // the two states a path may end in
    int32_t c0, cM;
    int64_t required;       // local index, -1: none
};
struct NestedArgs {
    const NestedJob *jobs;
    const NestedChain *chains;
    const double *scores, *raw;
    double *work;               // one double per bin: the sort, then the compacted selection
    unsigned long long *bt;
    unsigned char *wm;          // the region's candidate mask
    unsigned char *sol;
    NestedState *st;
    csr_nested_rec *rec;
    csr_nested_node *kids;
    unsigned long long *kidCount;
    int64_t kidCap;
};

CSR_HD bool nested_better(double v, int c, double bv, int bc) {
    return (v > bv + NESTED_EPS) || (fabs(v - bv) <= NESTED_EPS && c < bc);
}
CSR_HD double nested_cost(const NestedJob &jb, double internal, int64_t i) {
    if (jb.costs) return jb.costs[i];
    if (jb.uniform) return internal;
    return (i == 0 || i == jb.n) ? NESTED_EDGE : internal;
}
struct NestedShift {
    double floor;
    CSR_HD double operator()(double x) const { return x - floor; }
};
// np.quantile(v, q), method "linear", of the m values w[lo .. lo + m) - floor (w ascending); q is a multiple of 1/4
CSR_HD double nested_quantile(const double *w, int64_t lo, int64_t m, double q, double floor) {
    const double vi = (double)m * q + (1.0 + q * -1.0) - 1.0;
    if (vi >= (double)(m - 1)) return w[lo + m - 1] - floor;    // (one value: the weight is 1, the upper branch returns it)
    const double fl = ::floor(vi);
    const int64_t k = (int64_t)fl;
    const double a = w[lo + k] - floor, b = w[lo + k + 1] - floor;
    return np_lerp(a, b, vi - fl);
}
CSR_HD void nested_heapsort(double *w, int64_t n) {
    auto sift = [&](int64_t root, int64_t end) {
        const double v = w[root];
        for (;;) {
            int64_t ch = 2 * root + 1;
            if (ch >= end) break;
            if (ch + 1 < end && w[ch] < w[ch + 1]) ++ch;
            if (!(v < w[ch])) break;
            w[root] = w[ch];
            root = ch;
        }
        w[root] = v;
    };
    for (int64_t i = n / 2 - 1; i >= 0; --i) sift(i, n);
    for (int64_t end = n - 1; end > 0; --end) {
        const double t = w[0];
        w[0] = w[end];
        w[end] = t;
        sift(0, end);
    }
}
// the leftmost arg-max of r[0 .. n)
CSR_HD int64_t nested_argmax(const double *r, int64_t n) {
    int64_t k = 0;
    double m = r[0];
    for (int64_t i = 1; i < n; ++i)
        if (r[i] > m) { m = r[i]; k = i; }
    return k;
}
// what `_addNode` records of bins [off, off + n) whose first bin is `start` in its chain
CSR_HD csr_nested_node nested_node(const double *scores, const double *raw, int64_t off, int64_t start, int64_t n) {
    csr_nested_node nd;
    const int64_t k = nested_argmax(raw + off, n);
    nd.start = start;
    nd.end = start + n - 1;
    nd.required = start + k;
    nd.raw_score_max = raw[off + k];
    nd.score_sum = np_sum_f(scores + off, n, NpIdentity{});
    return nd;
}

// ---- peaks.py:4056-4071: required bin, floor, soft selection penalty -----------------------------------------------------------
CSR_HD void nested_prep_region(const NestedArgs &a, int j) {
    const NestedJob jb = a.jobs[j];
    const NestedChain P = a.chains[jb.chain];
    const double *x = a.scores + jb.off;
    double *w = a.work + jb.off;
    NestedState s;
    s.required = nested_argmax(a.raw + jb.off, jb.n);
    for (int64_t i = 0; i < jb.n; ++i) w[i] = x[i];
    nested_heapsort(w, jb.n);
    s.floor = P.useFloor ? nested_quantile(w, 0, jb.n, 0.25, 0.0) : 0.0;
    // the strictly positive solver scores: w[lo ..) - floor
    int64_t lo = 0, hi = jb.n;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (w[mid] - s.floor > 0.0) hi = mid; else lo = mid + 1;
    }
    const int64_t np = jb.n - lo;
    double spread = 0.0;
    if (np > 1) spread = nested_quantile(w, lo, np, 0.75, s.floor) - nested_quantile(w, lo, np, 0.25, s.floor);
    if (!np_finite(spread) || spread < 0.0) spread = 0.0;
    const double scale = P.scale < 0.0 ? 0.0 : (P.scale > 1.0 ? 1.0 : P.scale);
    const double base = P.base > 0.0 ? P.base : 0.0;
    s.extra = (1.0 - scale) * spread;
    s.penalty = base + s.extra;
    s.runPenalty = P.internal;
    s.v0 = s.vM = 0.0;
    s.c0 = s.cM = 0;
    a.st[j] = s;
}

// ---- peaks.py:3587-3655, minRun <= NESTED_REG_STATES -------------------------------------------------------------------------
CSR_HD void nested_dp_region(const NestedArgs &a, int j) {
    constexpr int S = NESTED_REG_STATES;
    const NestedJob jb = a.jobs[j];
    const double internal = a.chains[jb.chain].internal;
    NestedState s = a.st[j];
    const double *x = a.scores + jb.off;
    const int M = jb.minRun;
    const int big = (int)jb.n + 1;
    double v[S + 1];
    int c[S + 1];
#pragma unroll
    for (int k = 0; k <= S; ++k) { v[k] = -INFINITY; c[k] = big; }
    v[0] = 0.0;
    c[0] = 0;
    unsigned long long w = 0ull;
    for (int64_t i = 0; i < jb.n; ++i) {
        const double adj = (x[i] - s.floor) - s.penalty;
        const double tc = nested_cost(jb, internal, i);
        const double p0 = v[0];
        const int c0 = c[0];
        double pM = v[1];
        int cM = c[1];
#pragma unroll
        for (int k = 2; k <= S; ++k)
            if (k == M) { pM = v[k]; cM = c[k]; }
        // state 0: stay off, then a run that closes here
        double n0v = -INFINITY;
        int n0c = big;
        unsigned long long b0 = 0ull, b1 = 0ull;
        if (i != s.required) {
            if (np_finite(p0)) { n0v = p0; n0c = c0; }
            if (np_finite(pM)) {
                const double cand = pM - tc;
                if (nested_better(cand, cM, n0v, n0c)) { n0v = cand; n0c = cM; b0 = 1ull; }
            }
        }
        // states 2 .. M: the shift, top down
#pragma unroll
        for (int k = S; k >= 2; --k)
            if (k <= M) {
                const bool fin = np_finite(v[k - 1]);
                v[k] = fin ? v[k - 1] + adj : -INFINITY;
                c[k] = fin ? c[k - 1] + 1 : big;
            }
        // state 1: a run that opens here
        {
            const bool fin = np_finite(p0);
            v[1] = fin ? ((p0 - tc) - s.runPenalty) + adj : -INFINITY;
            c[1] = fin ? c0 + 1 : big;
        }
        // state M: the run that was already minRun long goes on
        if (np_finite(pM)) {
            const double cand = pM + adj;
            const int cc = cM + 1;
#pragma unroll
            for (int k = 1; k <= S; ++k)
                if (k == M && nested_better(cand, cc, v[k], c[k])) { v[k] = cand; c[k] = cc; b1 = 1ull; }
        }
        v[0] = n0v;
        c[0] = n0c;
        w |= (b0 | (b1 << 1)) << (2 * (int)(i & (NESTED_WORD - 1)));
        if ((i & (NESTED_WORD - 1)) == NESTED_WORD - 1 || i == jb.n - 1) {
            a.bt[jb.word + i / NESTED_WORD] = w;
            w = 0ull;
        }
    }
    s.v0 = v[0];
    s.c0 = c[0];
    s.vM = v[1];
    s.cM = c[1];
#pragma unroll
    for (int k = 2; k <= S; ++k)
        if (k == M) { s.vM = v[k]; s.cM = c[k]; }
    a.st[j] = s;
}

// ---- peaks.py:3657-3720 and 4099-4172 ---------------------------------------------------------------------------------------
// reserve `n` child records; the host path (one thread) needs no atomic
CSR_HD unsigned long long nested_reserve(unsigned long long *counter, unsigned long long n) {
#if defined(__HIP_DEVICE_COMPILE__)
    return atomicAdd(counter, n);
#else
    const unsigned long long b = *counter;
    *counter = b + n;
    return b;
#endif
}
CSR_HD void nested_finish_region(const NestedArgs &a, int j) {
    const NestedJob jb = a.jobs[j];
    const NestedChain P = a.chains[jb.chain];
    const NestedState s = a.st[j];
    const double *x = a.scores + jb.off;
    double *w = a.work + jb.off;
    unsigned char *m = a.wm + jb.off;
    const int64_t n = jb.n;
    const int M = jb.minRun;
    csr_nested_rec r;
    r.required = s.required < 0 ? -1 : jb.start + s.required;
    r.floor = s.floor;
    r.selection_penalty = s.penalty;
    r.extra_penalty = s.extra;
    r.child_base = -1;
    r.reserved = 0;
    // the final pick: max by (value, -count), the first of two equals
    const double last = s.vM - nested_cost(jb, P.internal, n);
    const bool on = (last > s.v0) || (last == s.v0 && s.cM < s.c0);
    if (!np_finite(on ? last : s.v0)) {
        r.decision = CSR_NESTED_INFEASIBLE;
        r.selected_count = 0; r.n_runs = 0; r.widths_ok = 0;
        r.objective = r.penalized = r.boundary_penalty = r.run_penalty_total = r.parent_penalized = r.split_gain = 0.0;
        a.rec[j] = r;
        return;
    }
    // backtrace
    int st = on ? M : 0;
    unsigned long long word = 0ull;
    int64_t wi = -1;
    for (int64_t i = n - 1; i >= 0; --i) {
        m[i] = st > 0 ? 1 : 0;
        if (i / NESTED_WORD != wi) { wi = i / NESTED_WORD; word = a.bt[jb.word + wi]; }
        const unsigned int b = (unsigned int)(word >> (2 * (int)(i & (NESTED_WORD - 1)))) & 3u;
        if (st == 0) st = (b & 1u) ? M : 0;
        else if (st == M) st = (b & 2u) ? M : M - 1;
        else st -= 1;
    }
    // `_parentConditionedSubpeakObjective` of the mask: compaction, boundary sum, runs
    int64_t cnt = 0, run = 0;
    int runs = 0;
    bool prev = false, ok = true;
    double bp = 0.0;
    for (int64_t i = 0; i < n; ++i) {
        const bool cur = m[i] != 0;
        if (cur != prev) {
            bp += nested_cost(jb, P.internal, i);
            if (cur) { ++runs; run = 0; }
            else if (run < M) ok = false;
        }
        if (cur) { w[cnt++] = x[i] - s.floor; ++run; }
        prev = cur;
    }
    if (prev) {
        bp += nested_cost(jb, P.internal, n);
        if (run < M) ok = false;
    }
    const double selected = np_sum_f(w, cnt, NpIdentity{});
    const double rpt = s.runPenalty * (double)runs;
    r.objective = (selected - bp) - rpt;
    r.penalized = r.objective - s.penalty * (double)cnt;
    r.boundary_penalty = bp;
    r.run_penalty_total = rpt;
    r.selected_count = cnt;
    r.n_runs = runs;
    r.widths_ok = (runs >= 1 && ok) ? 1 : 0;
    // ... and of the whole region kept as it is
    {
        const double all = np_sum_f(x, n, NestedShift{s.floor});
        double bpa = 0.0;
        bpa += nested_cost(jb, P.internal, 0);
        bpa += nested_cost(jb, P.internal, n);
        const double obj = (all - bpa) - s.runPenalty * 1.0;
        r.parent_penalized = obj - s.penalty * (double)n;
    }
    r.split_gain = r.penalized - r.parent_penalized;
    const bool split = runs >= 2 && r.widths_ok && r.split_gain > 0.0;
    const bool shrink = runs == 1 && r.widths_ok && cnt != n && r.split_gain > 0.0;
    r.decision = split ? CSR_NESTED_SPLIT : (shrink ? CSR_NESTED_SHRINK : CSR_NESTED_KEEP_PARENT);
    // the candidate runs, with what a node made of one records
    if (runs > 0 && a.kids) {
        const unsigned long long base = nested_reserve(a.kidCount, (unsigned long long)runs);
        if ((int64_t)(base + (unsigned long long)runs) <= a.kidCap) {
            r.child_base = (int64_t)base;
            int64_t k = 0, i = 0;
            while (i < n) {
                if (!m[i]) { ++i; continue; }
                int64_t e = i;
                while (e + 1 < n && m[e + 1]) ++e;
                a.kids[base + k++] = nested_node(a.scores, a.raw, jb.off + i, jb.start + i, e - i + 1);
                i = e + 1;
            }
        }
    }
    if (split || shrink || P.commitAlways) {
        unsigned char *so = a.sol + jb.off;
        for (int64_t i = 0; i < n; ++i) so[i] = m[i];
    }
    a.rec[j] = r;
}

// ---- kernels ----------------------------------------------------------------------------------------------------------------
// `order` lists the jobs of a launch (sorted by length); one lane each
__global__ __launch_bounds__(64) void k_nested_prep(NestedArgs a, const int *__restrict__ order, int n) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t < n) nested_prep_region(a, order[t]);
}
__global__ __launch_bounds__(64) void k_nested_dp_reg(NestedArgs a, const int *__restrict__ order, int n) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t < n) nested_dp_region(a, order[t]);
}
__global__ __launch_bounds__(64) void k_nested_finish(NestedArgs a, const int *__restrict__ order, int n) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t < n) nested_finish_region(a, order[t]);
}
__global__ __launch_bounds__(64) void k_nested_nodes(const NestedJob *__restrict__ jobs, int n, const double *__restrict__ scores,
                                                     const double *__restrict__ raw, csr_nested_node *__restrict__ out) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t < n) out[t] = nested_node(scores, raw, jobs[t].off, jobs[t].start, jobs[t].n);
}

// one workgroup per region: thread t owns state t + 1, thread 0 state 0 as well
__global__ __launch_bounds__(NESTED_WIDE_T) void k_nested_dp_wide(NestedArgs a, const int *__restrict__ order) {
    __shared__ double sV[2][NESTED_WIDE_T + 1];
    __shared__ int sC[2][NESTED_WIDE_T + 1];
    __shared__ unsigned int sB1[2];
    const int j = order[blockIdx.x];
    const NestedJob jb = a.jobs[j];
    const double internal = a.chains[jb.chain].internal;
    const NestedState s = a.st[j];
    const double *x = a.scores + jb.off;
    const int M = jb.minRun, t = threadIdx.x;
    const int big = (int)jb.n + 1;
    if (t <= M) {
        sV[0][t] = t == 0 ? 0.0 : -INFINITY;
        sC[0][t] = t == 0 ? 0 : big;
    }
    if (t == 0) {       // (M can equal the thread count's last index + 1 only below the limit; state M is written by thread M - 1)
        sB1[0] = sB1[1] = 0u;
    }
    __syncthreads();
    unsigned long long w = 0ull;
    for (int64_t i = 0; i < jb.n; ++i) {
        const int b = (int)(i & 1);
        const double adj = (x[i] - s.floor) - s.penalty;
        const double tc = nested_cost(jb, internal, i);
        const double p0 = sV[b][0], pM = sV[b][M];
        const int c0 = sC[b][0], cM = sC[b][M];
        unsigned long long b0 = 0ull;
        if (t < M) {
            const int k = t + 1;
            double nv;
            int nc;
            if (k == 1) {
                const bool fin = np_finite(p0);
                nv = fin ? ((p0 - tc) - s.runPenalty) + adj : -INFINITY;
                nc = fin ? c0 + 1 : big;
            } else {
                const double pv = sV[b][k - 1];
                const int pc = sC[b][k - 1];
                const bool fin = np_finite(pv);
                nv = fin ? pv + adj : -INFINITY;
                nc = fin ? pc + 1 : big;
            }
            if (k == M) {
                unsigned int b1 = 0u;
                if (np_finite(pM)) {
                    const double cand = pM + adj;
                    if (nested_better(cand, cM + 1, nv, nc)) { nv = cand; nc = cM + 1; b1 = 1u; }
                }
                sB1[b] = b1;
            }
            sV[b ^ 1][k] = nv;
            sC[b ^ 1][k] = nc;
        }
        if (t == 0) {
            double n0v = -INFINITY;
            int n0c = big;
            if (i != s.required) {
                if (np_finite(p0)) { n0v = p0; n0c = c0; }
                if (np_finite(pM)) {
                    const double cand = pM - tc;
                    if (nested_better(cand, cM, n0v, n0c)) { n0v = cand; n0c = cM; b0 = 1ull; }
                }
            }
            sV[b ^ 1][0] = n0v;
            sC[b ^ 1][0] = n0c;
        }
        __syncthreads();
        if (t == 0) {
            w |= (b0 | ((unsigned long long)sB1[b] << 1)) << (2 * (int)(i & (NESTED_WORD - 1)));
            if ((i & (NESTED_WORD - 1)) == NESTED_WORD - 1 || i == jb.n - 1) {
                a.bt[jb.word + i / NESTED_WORD] = w;
                w = 0ull;
            }
        }
    }
    if (t == 0) {
        const int b = (int)(jb.n & 1);
        NestedState o = s;
        o.v0 = sV[b][0]; o.c0 = sC[b][0];
        o.vM = sV[b][M]; o.cM = sC[b][M];
        a.st[j] = o;
    }
}

// ---- `_roccoObjectiveForSolution`: the selected scores of a chain, compacted run by run, and their NumPy-order sum -----------
struct NestedRun {
    int64_t src, dst, n;    // scores[src .. src + n) -> comp[dst ..)
};
__global__ __launch_bounds__(256) void k_nested_gather(const NestedRun *__restrict__ runs, const double *__restrict__ scores,
                                                       double *__restrict__ comp) {
    const NestedRun r = runs[blockIdx.x];
    for (int64_t i = threadIdx.x; i < r.n; i += 256) comp[r.dst + i] = scores[r.src + i];
}
struct NestedSumJob {       // (a Job of k_np_chunk_sums / k_np_fold: "k_nested_sum", "k_nested_fold")
    int64_t src, n;         // comp[src .. src + n)
    __device__ const double *data(const double *comp) const { return comp + src; }
    __device__ NpIdentity elem() const { return NpIdentity{}; }
};

}  // namespace csr
