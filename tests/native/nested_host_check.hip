// Stand-alone host check of the per-region routines of csrc/csr_nested.h (they are __host__ __device__): runs one layer of the
// nested ROCCO refinement on the CPU, region after region, exactly as the lanes of k_nested_prep / k_nested_dp_reg /
// k_nested_finish do.  No GPU is touched.  tests/test_nested_host.py builds it (host only, with the address and undefined-behaviour
// sanitizers), feeds it cases of tests/nested_cases.py and compares what it writes with the twin.
//
//   nested_host_check IN OUT
// IN:  int64 n, nRegions; double gamma, base, scale; int64 useFloor; double scores[n], raw[n]; uint8 sol[n];
//      int64 (start, end, minRun)[nRegions]
// OUT: csr_nested_rec[nRegions]; int64 nKids; csr_nested_node[nKids]; uint8 sol[n]
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/consenrich_amd.h"
#include "../../consenrich_amd/csrc/csr_nested.h"

using namespace csr;

template <class T>
static bool get(FILE *f, T *p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }
template <class T>
static bool put(FILE *f, const T *p, size_t n) { return n == 0 || fwrite(p, sizeof(T), n, f) == n; }

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t n = 0, nr = 0, useFloor = 0;
    double gamma = 0, base = 0, scale = 0;
    if (!get(f, &n, 1) || !get(f, &nr, 1) || !get(f, &gamma, 1) || !get(f, &base, 1) || !get(f, &scale, 1) || !get(f, &useFloor, 1)) return 3;
    std::vector<double> scores((size_t)n), raw((size_t)n), work((size_t)n);
    std::vector<unsigned char> sol((size_t)n), wm((size_t)n);
    std::vector<int64_t> rg((size_t)(3 * nr));
    if (!get(f, scores.data(), n) || !get(f, raw.data(), n) || !get(f, sol.data(), n) || !get(f, rg.data(), 3 * nr)) return 3;
    fclose(f);
    std::vector<NestedJob> jobs((size_t)nr);
    int64_t words = 0, cap = 0;
    for (int64_t k = 0; k < nr; ++k) {
        NestedJob &jb = jobs[(size_t)k];
        jb.off = jb.start = rg[3 * k];
        jb.n = rg[3 * k + 1] - rg[3 * k] + 1;
        jb.word = words;
        jb.required = -1;
        jb.costs = nullptr;
        jb.minRun = (int32_t)std::min<int64_t>(std::max<int64_t>(rg[3 * k + 2], 1), jb.n);
        jb.chain = 0;
        if (jb.minRun > NESTED_REG_STATES) return 4;    // the states-as-lanes kernel has no host form
        words += (jb.n + NESTED_WORD - 1) / NESTED_WORD;
        cap += std::max<int64_t>(1, (jb.n + 1) / (jb.minRun + 1));
    }
    NestedChain p;
    memset(&p, 0, sizeof(p));
    p.internal = std::max(0.25 * gamma, 1000.0 * NESTED_EDGE);
    p.base = base;
    p.scale = scale;
    p.useFloor = useFloor != 0;
    std::vector<unsigned long long> bt((size_t)words + 1);
    std::vector<NestedState> st((size_t)nr);
    std::vector<csr_nested_rec> rec((size_t)nr);
    std::vector<csr_nested_node> kids((size_t)cap);     // exactly the bound the library allocates: an overrun is an ASan report
    unsigned long long nKids = 0;
    NestedArgs a;
    a.jobs = jobs.data(); a.chains = &p; a.scores = scores.data(); a.raw = raw.data(); a.work = work.data(); a.bt = bt.data();
    a.wm = wm.data(); a.sol = sol.data(); a.st = st.data(); a.rec = rec.data(); a.kids = kids.data(); a.kidCount = &nKids; a.kidCap = cap;
    for (int k = 0; k < (int)nr; ++k) {
        nested_prep_region(a, k);
        nested_dp_region(a, k);
        nested_finish_region(a, k);
    }
    FILE *o = fopen(argv[2], "wb");
    if (!o) return 2;
    const int64_t nk = (int64_t)nKids;
    if (!put(o, rec.data(), nr) || !put(o, &nk, 1) || !put(o, kids.data(), nk) || !put(o, sol.data(), n)) return 3;
    fclose(o);
    return 0;
}
