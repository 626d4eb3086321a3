// Stand-alone host check of the run, gap and parent routines of csrc/csr_broad.h (they are __host__ __device__, the parents a
// template over a team): runs the gap sums and the parent records of one chain on the CPU with the host team, gap after gap and
// parent after parent, exactly as the lanes of k_broad_gap_sums and the wavefronts of k_broad_parents do, and the support runs of
// one chain the way csr_batch_broad_runs drives k_broad_run_* -- flags, exclusive scan, write, touch, keep scan, keep write, gap
// sums, and once more with the envelope as predicate where nothing is kept -- with a serial scan in place of the workgroup
// scans and the library's own buffer sizes.  No GPU is touched.  tests/test_broad_host.py builds it (host only, with the address
// and undefined-behaviour sanitizers), feeds it the cases of tests/broad_cases.py and compares what the package's host half makes
// of its output with the fixtures.
//
//   broad_host_check IN OUT
// IN:  int64 n, nGaps, nParents, hasUncertainty, nBreaks, doRuns, maxGapBins; double penalty, fraction, multiplier, threshold;
//      double scores[n], state[n], uncertainty[n]; int64 (start, len)[nGaps]; int64 (start, end)[nParents];
//      with doRuns: int64 breaks[nBreaks]; uint8 strong[n], weak[n]
// OUT: double sums[nGaps]; csr_broad_parent[nParents]; uint8 mask[n];
//      with doRuns: int64 supportRuns, keptRuns, fallback; csr_broad_run[keptRuns]
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/consenrich_amd.h"
#include "../../consenrich_amd/csrc/csr_broad.h"

using namespace csr;

template <class T>
static bool get(FILE *f, T *p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }
template <class T>
static bool put(FILE *f, const T *p, size_t n) { return n == 0 || fwrite(p, sizeof(T), n, f) == n; }

// broad_runs_chain (csr_host_broad.inl) of one chain: every buffer has exactly the library's size, an overrun is an ASan report
static bool support_runs(const std::vector<double> &scores, const std::vector<unsigned char> &strong, const std::vector<unsigned char> &weak,
                         const std::vector<int64_t> &breaks, const double *par, int64_t maxGapBins, bool envelope, int64_t *support,
                         std::vector<csr_broad_run> &kept) {
    const int64_t n = (int64_t)scores.size();
    *support = 0;
    if (n <= 0) return true;
    BroadRunArgs a;
    memset(&a, 0, sizeof(a));
    a.scores = scores.data();
    a.weak = weak.data();
    a.strong = strong.data();
    a.breaks = breaks.data();
    a.nBreaks = (int64_t)breaks.size();
    a.n = n;
    a.threshold = par[3];
    a.penalty = par[0];
    a.fraction = par[1];
    a.maxGapBins = maxGapBins;
    a.envelope = envelope ? 1 : 0;
    a.chain = 0;
    // k_broad_run_count + k_broad_scan: the totals (one thread per bin of whole 1024-bin blocks: the flags past n are 0)
    const int64_t nb = (n + 1023) / 1024;
    unsigned long long tot = 0;
    for (int64_t i = 0; i < nb * 1024; ++i) tot += broad_run_flags(a, i);
    const int64_t ns = (int64_t)(tot & 0xffffffffull), ne = (int64_t)(tot >> 32);
    if (ns != ne) return false;
    *support = ns;
    if (ns == 0) return true;
    std::vector<int64_t> starts((size_t)ns), ends((size_t)ns);
    std::vector<unsigned char> touch((size_t)ns);
    std::vector<csr_broad_run> rec((size_t)ns);
    a.starts = starts.data();
    a.ends = ends.data();
    a.touch = touch.data();
    a.rec = rec.data();
    a.nRuns = ns;
    // k_broad_run_write: the exclusive scan of the flags is the place of a start and of an end
    unsigned long long ex = 0;
    for (int64_t i = 0; i < nb * 1024; ++i) {
        const unsigned long long fl = broad_run_flags(a, i);
        const int64_t ks = (int64_t)(ex & 0xffffffffull), ke = (int64_t)(ex >> 32);
        if ((fl & 1ull) && ks < a.nRuns) a.starts[ks] = i;
        if ((fl >> 32) && ke < a.nRuns) a.ends[ke] = i;
        ex += fl;
    }
    // k_broad_run_touch (the envelope's own runs touch it)
    for (int64_t r = 0; r < ns; ++r) {
        bool any = envelope;
        for (int64_t i = a.starts[r]; !envelope && i <= a.ends[r]; ++i) any = any || broad_env(a, i);
        a.touch[r] = any ? 1 : 0;
    }
    // k_broad_keep_count / k_broad_scan / k_broad_keep_write
    int64_t pos = 0;
    for (int64_t r = 0; r < ns; ++r) {
        if (!a.touch[r]) continue;
        csr_broad_run q;
        q.start = a.starts[r];
        q.end = a.ends[r];
        q.gap_sum = 0.0;
        q.chain = a.chain;
        q.reserved = 0;
        a.rec[pos++] = q;
    }
    // k_broad_run_gaps
    for (int64_t g = 0; g < pos; ++g) broad_run_gap(a, g, pos);
    kept.insert(kept.end(), rec.begin(), rec.begin() + pos);
    return true;
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t hd[7] = {0, 0, 0, 0, 0, 0, 0};
    double par[4] = {0, 0, 0, 0};
    if (!get(f, hd, 7) || !get(f, par, 4)) return 3;
    const int64_t n = hd[0], ng = hd[1], np = hd[2];
    std::vector<double> scores((size_t)n), state((size_t)n), unc((size_t)n), work((size_t)n), tile(CLEANUP_SORT_TILE);
    std::vector<int64_t> gp((size_t)(2 * ng)), rg((size_t)(2 * np));
    if (!get(f, scores.data(), n) || !get(f, state.data(), n) || !get(f, unc.data(), n) || !get(f, gp.data(), 2 * ng) ||
        !get(f, rg.data(), 2 * np))
        return 3;
    const int64_t nbk = hd[4];
    std::vector<int64_t> breaks((size_t)nbk);
    std::vector<unsigned char> strong, weak;
    if (hd[5]) {
        strong.resize((size_t)n);
        weak.resize((size_t)n);
        if (!get(f, breaks.data(), nbk) || !get(f, strong.data(), n) || !get(f, weak.data(), n)) return 3;
    }
    fclose(f);
    // the gaps
    std::vector<int64_t> gs((size_t)ng), gl((size_t)ng);
    for (int64_t g = 0; g < ng; ++g) { gs[(size_t)g] = gp[2 * g]; gl[(size_t)g] = gp[2 * g + 1]; }
    std::vector<double> sums((size_t)ng);       // exactly what the library allocates: an overrun is an ASan report
    BroadGapArgs ga;
    memset(&ga, 0, sizeof(ga));
    ga.scores = scores.data();
    ga.start = gs.data();
    ga.len = gl.data();
    ga.penalty = par[0];
    ga.fraction = par[1];
    ga.sums = sums.data();
    ga.nGaps = ng;
    for (int64_t g = 0; g < ng; ++g) broad_gap_sum(ga, g);
    // the parents
    std::vector<BroadJob> jobs((size_t)np);
    for (int64_t k = 0; k < np; ++k) {
        BroadJob &jb = jobs[(size_t)k];
        jb.off = jb.start = rg[2 * k];
        jb.n = rg[2 * k + 1] - rg[2 * k] + 1;
        jb.chain = 0;
        jb.reserved = 0;
    }
    BroadChain ch;
    ch.multiplier = par[2];
    ch.filter = hd[3] != 0;
    ch.reserved = 0;
    std::vector<csr_broad_parent> rec((size_t)np);
    std::vector<unsigned char> mask((size_t)n, 0);
    BroadArgs a;
    memset(&a, 0, sizeof(a));
    a.jobs = jobs.data();
    a.cfg = &ch;
    a.scores = scores.data();
    a.sig.d = state.data();
    if (hd[3]) a.unc.d = unc.data();
    a.work = work.data();
    a.mask = mask.data();
    a.rec = rec.data();
    a.nParents = np;
    BroadHostTeam tm;
    tm.buf = tile.data();
    for (int64_t k = 0; k < np; ++k) broad_parent(tm, a, k);
    FILE *o = fopen(argv[2], "wb");
    if (!o) return 2;
    if (!put(o, sums.data(), ng) || !put(o, rec.data(), np) || !put(o, mask.data(), n)) return 3;
    if (hd[5]) {
        std::vector<csr_broad_run> kept;
        int64_t out3[3] = {0, 0, 0};
        if (!support_runs(scores, strong, weak, breaks, par, hd[6], false, &out3[0], kept)) return 4;
        if (kept.empty()) {
            int64_t runs = 0;
            out3[2] = 1;
            if (!support_runs(scores, strong, weak, breaks, par, hd[6], true, &runs, kept)) return 4;
        }
        out3[1] = (int64_t)kept.size();
        if (!put(o, out3, 3) || !put(o, kept.data(), kept.size())) return 3;
    }
    fclose(o);
    return 0;
}
