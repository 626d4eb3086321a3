// Stand-alone host check of csrc/csr_cleanup.h (its routines are __host__ __device__ templates over a team): runs the massive
// sub-peak clean-up of a list of children on the CPU with a team of one thread -- the same recursion with its explicit stack, the
// same merge network, the same scans and the library's own packing of the segment records, with the library's buffer sizes.  No GPU
// is touched.  tests/test_cleanup_host.py builds it (host only, with the address and undefined-behaviour sanitizers), feeds it the
// cases of tests/cleanup_cases.py and compares what it writes with the fixtures.
//
//   cleanup_host_check IN OUT
// IN:  int64 op, n, nChildren, hasEdges, origin, step; csr_cleanup_policy; double scores[n]; int64 edges[n + 1] (hasEdges);
//      int64 (start, end)[nChildren]
// OUT: FORCE: int64 nSegments; csr_cleanup_segment[nSegments]; csr_cleanup_counts[nChildren]
//      SPLIT, CONTRACT: csr_cleanup_node[nChildren]
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/consenrich_amd.h"
#include "../../consenrich_amd/csrc/csr_cleanup.h"

using namespace csr;

template <class T>
static bool get(FILE *f, T *p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }
template <class T>
static bool put(FILE *f, const T *p, size_t n) { return n == 0 || fwrite(p, sizeof(T), n, f) == n; }

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t hd[6] = {0, 0, 0, 0, 0, 0};
    csr_cleanup_policy pol;
    if (!get(f, hd, 6) || !get(f, &pol, 1)) return 3;
    const int64_t op = hd[0], n = hd[1], nk = hd[2];
    if (n <= 0 || nk < 0 || pol.max_depth > CSR_CLEANUP_MAX_DEPTH) return 4;
    std::vector<double> scores((size_t)n), work((size_t)n), tile(CLEANUP_SORT_TILE);
    std::vector<int64_t> edges((size_t)(hd[3] ? n + 1 : 0)), rg((size_t)(2 * nk));
    if (!get(f, scores.data(), n) || !get(f, edges.data(), edges.size()) || !get(f, rg.data(), 2 * nk)) return 3;
    fclose(f);
    std::vector<csr_cleanup_child> kids((size_t)nk);
    for (int64_t k = 0; k < nk; ++k) {
        kids[(size_t)k].start = rg[2 * k];
        kids[(size_t)k].end = rg[2 * k + 1];
        if (rg[2 * k] < 0 || rg[2 * k + 1] < rg[2 * k] || rg[2 * k + 1] >= n) return 4;
    }
    // exactly what the library allocates: an overrun is an ASan report
    std::vector<csr_cleanup_segment> seg((size_t)(CLEANUP_MAX_SEGMENTS * nk)), packed((size_t)(CLEANUP_MAX_SEGMENTS * nk));
    std::vector<csr_cleanup_counts> cnt((size_t)nk);
    std::vector<csr_cleanup_node> node((size_t)nk);
    CleanupArgs a;
    memset(&a, 0, sizeof(a));
    a.scores = scores.data();
    a.work = work.data();
    a.co.edges = hd[3] ? edges.data() : nullptr;
    a.co.origin = hd[4];
    a.co.step = hd[5];
    a.kids = kids.data();
    a.pol = pol;
    a.seg = seg.data();
    a.cnt = cnt.data();
    a.node = node.data();
    a.nKids = nk;
    a.op = (int32_t)op;
    CleanupHostTeam tm;
    tm.buf = tile.data();
    for (int64_t k = 0; k < nk; ++k) {
        if (op == CSR_CLEANUP_OP_FORCE) cleanup_plan_child(tm, a, k);
        else cleanup_piece(tm, a, k);
    }
    FILE *o = fopen(argv[2], "wb");
    if (!o) return 2;
    if (op == CSR_CLEANUP_OP_FORCE) {
        int64_t total = 0, at = -1;
        const int rc = cleanup_pack(nk, seg.data(), cnt.data(), (int64_t)packed.size(), packed.data(), &total, &at);
        if (rc != 0) return 10 + rc;
        if (!put(o, &total, 1) || !put(o, packed.data(), (size_t)total) || !put(o, cnt.data(), (size_t)nk)) return 3;
    } else if (!put(o, node.data(), (size_t)nk)) {
        return 3;
    }
    fclose(o);
    return 0;
}
