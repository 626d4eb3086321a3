// Stand-alone host check of the per-parent and per-child routines of csrc/csr_export.h (they are __host__ __device__): runs the
// narrowPeak export of one chain on the CPU, parent after parent and child after child, exactly as the lanes of k_export_prep /
// k_nested_dp_reg / k_export_finish / k_export_child do, with the library's own buffer sizes.  No GPU is touched.
// tests/test_narrowpeak_host.py builds it (host only, with the address and undefined-behaviour sanitizers), feeds it cases of
// tests/narrowpeak_cases.py and compares what it writes with the twin.
//
//   narrowpeak_host_check IN OUT
// IN:  int64 n, nParents; double penalty, cost, floor, multiplier; int64 minRun, split, trim, filter, hasUncertainty;
//      double scores[n], state[n], uncertainty[n]; int64 (start, end)[nParents]
// OUT: int64 nPeaks; csr_export_peak[nPeaks]; int32 parentFlags[nParents]
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/consenrich_amd.h"
#include "../../consenrich_amd/csrc/csr_export.h"

using namespace csr;

template <class T>
static bool get(FILE *f, T *p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }
template <class T>
static bool put(FILE *f, const T *p, size_t n) { return n == 0 || fwrite(p, sizeof(T), n, f) == n; }

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t n = 0, np = 0, sw[5] = {0, 0, 0, 0, 0};
    double par[4] = {0, 0, 0, 0};
    if (!get(f, &n, 1) || !get(f, &np, 1) || !get(f, par, 4) || !get(f, sw, 5)) return 3;
    std::vector<double> scores((size_t)n), state((size_t)n), unc((size_t)n), work((size_t)n);
    std::vector<unsigned char> wm((size_t)n);
    std::vector<int64_t> rg((size_t)(2 * np));
    if (!get(f, scores.data(), n) || !get(f, state.data(), n) || !get(f, unc.data(), n) || !get(f, rg.data(), 2 * np)) return 3;
    fclose(f);
    std::vector<NestedJob> jobs((size_t)np);
    int64_t words = 0;
    for (int64_t k = 0; k < np; ++k) {
        NestedJob &jb = jobs[(size_t)k];
        jb.off = jb.start = rg[2 * k];
        jb.n = rg[2 * k + 1] - rg[2 * k] + 1;
        jb.word = words;
        jb.required = -1;
        jb.costs = nullptr;
        jb.minRun = (int32_t)std::min<int64_t>(std::max<int64_t>(sw[0], 1), jb.n);
        jb.chain = 0;
        jb.uniform = 1;
        jb.reserved = 0;
        if (sw[1] && jb.minRun > NESTED_REG_STATES) return 4;     // the states-as-lanes kernel has no host form
        words += (jb.n + NESTED_WORD - 1) / NESTED_WORD;
    }
    NestedChain ch;
    memset(&ch, 0, sizeof(ch));
    ch.internal = par[1] > 0.0 ? par[1] : 0.0;
    ExportChain ec;
    memset(&ec, 0, sizeof(ec));
    ec.penalty = par[0];
    ec.floor = par[2];
    ec.multiplier = par[3];
    ec.split = sw[1] != 0;
    ec.trim = sw[2] != 0;
    ec.filter = sw[3] != 0;
    std::vector<unsigned long long> bt((size_t)words + 1);
    std::vector<NestedState> st((size_t)np);
    std::vector<ExportParent> prec((size_t)np);
    std::vector<int64_t> base((size_t)np);
    ExportArgs a;
    memset(&a, 0, sizeof(a));
    a.na.jobs = jobs.data(); a.na.chains = &ch; a.na.scores = a.na.raw = scores.data(); a.na.work = work.data(); a.na.bt = bt.data();
    a.na.wm = wm.data(); a.na.st = st.data();
    a.cfg = &ec;
    a.sig.d = state.data();
    if (sw[4]) a.unc.d = unc.data();
    a.par = prec.data();
    a.base = base.data();
    a.nParents = np;
    int64_t total = 0;
    for (int k = 0; k < (int)np; ++k) {
        export_prep_parent(a, k);
        if (ec.split) nested_dp_region(a.na, k);
        export_finish_parent(a, k);
        base[(size_t)k] = total;
        total += prec[(size_t)k].count;
    }
    std::vector<csr_export_peak> peaks((size_t)total);      // exactly what the library allocates: an overrun is an ASan report
    a.peaks = peaks.data();
    a.nPeaks = total;
    for (int64_t t = 0; t < total; ++t) export_child(a, t);
    std::vector<int32_t> flags((size_t)np);
    for (int64_t k = 0; k < np; ++k) flags[(size_t)k] = (prec[(size_t)k].flags & EXPORT_BAD_SIGNAL) ? CSR_EXPORT_NONFINITE_SIGNAL : 0;
    FILE *o = fopen(argv[2], "wb");
    if (!o) return 2;
    if (!put(o, &total, 1) || !put(o, peaks.data(), total) || !put(o, flags.data(), np)) return 3;
    fclose(o);
    return 0;
}
