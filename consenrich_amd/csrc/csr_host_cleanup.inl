// csr_host_cleanup.inl -- part of csr_lib.hip (one translation unit; included after csr_host_export.inl): the piece-level call of
// the massive sub-peak clean-up over the wavefronts of csr_cleanup.h, on host arrays (default context).  Every check comes before a
// device is touched.  The work space is csr_ctx::cleanupWs: the staged scores and edges, one work double per bin, the children, and
// per child its CLEANUP_MAX_SEGMENTS segment records, its counters and its node record.

static int cleanup_check_policy(const csr_cleanup_policy &p) {
    if (p.max_depth > CSR_CLEANUP_MAX_DEPTH)
        return value_error("`maxDepth` %d exceeds the supported maximum %d", (int)p.max_depth, CSR_CLEANUP_MAX_DEPTH);
    if (!std::isfinite(p.split_quantile)) return value_error("`splitQuantile` must be finite");
    if (!std::isfinite(p.min_split_z)) return value_error("`minSplitZ` must be finite");
    if (!std::isfinite(p.boundary_cost)) return value_error("`boundaryCost` must be finite");
    return 0;
}

// cleanup_pack (csr_cleanup.h) with the library's messages
static int cleanup_pack_checked(int64_t nk, const csr_cleanup_segment *seg, const csr_cleanup_counts *cnt, int64_t capacity,
                                csr_cleanup_segment *out, int64_t *total) {
    int64_t at = -1;
    switch (cleanup_pack(nk, seg, cnt, capacity, out, total, &at)) {
    case 0: return 0;
    case CLEANUP_PACK_OVERFLOW: return fail("clean-up: child %lld ends in more than %d segments", (long long)at, CSR_CLEANUP_MAX_SEGMENTS);
    case CLEANUP_PACK_NONFINITE: return value_error("`scores` contains non-finite values");
    case CLEANUP_PACK_CAPACITY: return fail("clean-up: the segments do not fit the capacity %lld (child %lld)", (long long)capacity, (long long)at);
    default: return fail("clean-up: bad segment count (child %lld)", (long long)at);
    }
}

extern "C" int csr_cleanup_plan(int32_t op, int64_t n, const double *scores, const int64_t *edges, int64_t origin, int64_t step,
                                int64_t n_children, const csr_cleanup_child *children, const csr_cleanup_policy *policy, int64_t capacity,
                                csr_cleanup_segment *segments, int64_t *n_segments, csr_cleanup_counts *counts, csr_cleanup_node *nodes) {
    DEFAULT_CTX_GUARD;
    if (op != CSR_CLEANUP_OP_FORCE && op != CSR_CLEANUP_OP_SPLIT && op != CSR_CLEANUP_OP_CONTRACT) return fail("unknown clean-up operation %d", (int)op);
    if (n <= 0 || !scores || !policy || n_children < 0 || (n_children > 0 && !children)) return fail("null or empty argument");
    if (n > CLEANUP_MAX_BINS) return fail("too many bins: %lld (limit 2^31 - 2)", (long long)n);
    if (n_children >= (int64_t)1 << 30) return fail("too many children: %lld", (long long)n_children);
    if (op == CSR_CLEANUP_OP_FORCE) {
        if (!counts || !n_segments || capacity < 0 || (capacity > 0 && !segments)) return fail("null output argument");
        *n_segments = 0;
    } else if (!nodes) {
        return fail("null output argument");
    }
    CHECK(cleanup_check_policy(*policy));
    if (!edges && step < 0) return fail("negative step");
    if (edges)
        for (int64_t i = 0; i < n; ++i)
            if (edges[i + 1] < edges[i]) return fail("bin edges must not decrease (edge %lld)", (long long)(i + 1));
    CleanupCoords co;
    co.edges = edges;
    co.origin = origin;
    co.step = step;
    co.shift = 0;
    for (int64_t k = 0; k < n_children; ++k) {
        const csr_cleanup_child &r = children[k];
        if (r.start < 0 || r.end < r.start || r.end >= n) return fail("child %lld: bins [%lld, %lld] are outside the scores", (long long)k, (long long)r.start, (long long)r.end);
        if (k > 0 && children[k - 1].end >= r.start) return fail("child %lld: children must be disjoint and ascending", (long long)k);
        // the children the call evaluates: all of a piece operation, the candidates of the recursion
        bool evaluated = op != CSR_CLEANUP_OP_FORCE || (double)co.width(r.start, r.end) >= policy->threshold;
        if (op == CSR_CLEANUP_OP_CONTRACT && (!std::isfinite(policy->contract_threshold) || policy->contract_threshold <= 0.0)) evaluated = false;
        if (evaluated) CHECK(nested_value_vector("scores", scores + r.start, r.end - r.start + 1));
    }
    if (n_children == 0) return 0;
    csr_ctx *c = nullptr;
    CHECK(ctx_or_default(c));
    csr_ctx::CleanupWs &ws = c->cleanupWs;
    const size_t nk = (size_t)n_children, bytes = 8 * (size_t)n;
    CHECK(ws.arena.reserve(2 * bytes + 8 + 64));
    CHECK(ws.work.reserve(bytes + 64));
    CHECK(ws.kids.reserve(sizeof(csr_cleanup_child) * nk));
    CHECK(ws.seg.reserve(sizeof(csr_cleanup_segment) * CSR_CLEANUP_MAX_SEGMENTS * nk));
    CHECK(ws.cnt.reserve(sizeof(csr_cleanup_counts) * nk));
    CHECK(ws.node.reserve(sizeof(csr_cleanup_node) * nk));
    char *base = (char *)ws.arena.ptr;
    HIPOK(hipMemcpyAsync(base, scores, bytes, hipMemcpyHostToDevice, c->stream));
    if (edges) HIPOK(hipMemcpyAsync(base + bytes, edges, bytes + 8, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemcpyAsync(ws.kids.ptr, children, sizeof(csr_cleanup_child) * nk, hipMemcpyHostToDevice, c->stream));
    CleanupArgs a;
    memset(&a, 0, sizeof(a));
    a.scores = (const double *)base;
    a.work = (double *)ws.work.ptr;
    a.co = co;
    if (edges) a.co.edges = (const int64_t *)(base + bytes);
    a.kids = (const csr_cleanup_child *)ws.kids.ptr;
    a.pol = *policy;
    a.seg = (csr_cleanup_segment *)ws.seg.ptr;
    a.cnt = (csr_cleanup_counts *)ws.cnt.ptr;
    a.node = (csr_cleanup_node *)ws.node.ptr;
    a.nKids = n_children;
    a.op = op;
    CHECK(launch(c, "cleanup_plan", "k_cleanup_plan", k_cleanup_plan, dim3((unsigned)nk), dim3(64), 0, c->stream, a));
    if (op != CSR_CLEANUP_OP_FORCE) {
        HIPOK(hipMemcpyAsync(nodes, ws.node.ptr, sizeof(csr_cleanup_node) * nk, hipMemcpyDeviceToHost, c->stream));
        HIPOK(hipStreamSynchronize(c->stream));
        return 0;
    }
    std::vector<csr_cleanup_segment> seg(CSR_CLEANUP_MAX_SEGMENTS * nk);
    HIPOK(hipMemcpyAsync(counts, ws.cnt.ptr, sizeof(csr_cleanup_counts) * nk, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipMemcpyAsync(seg.data(), ws.seg.ptr, sizeof(csr_cleanup_segment) * seg.size(), hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    return cleanup_pack_checked(n_children, seg.data(), counts, capacity, segments, n_segments);
}

// batch context: the children's scores are the resident tracks; nothing resident changes.  Children ascending by (chain, start) and
// disjoint; child k's n_k + 1 edges start at edges[edge_base] (edges NULL: equally wide bins of `step`; only differences of
// coordinates and exact half-integers enter, so the origin does not).  Non-finite resident scores inside a candidate are found by
// the plan kernel and answered with the reference's text.
extern "C" int csr_batch_cleanup_plan(csr_ctx *c, const csr_cleanup_policy *policies, const unsigned char *chain_mask, int64_t n_children,
                                      const csr_cleanup_batch_child *children, int64_t n_edges, const int64_t *edges, int64_t step,
                                      int64_t capacity, csr_cleanup_segment *segments, int64_t *n_segments, csr_cleanup_counts *counts) {
    CHECK(need(c));
    if (!policies || !n_segments || n_children < 0 || (n_children > 0 && (!children || !counts)) || capacity < 0 || (capacity > 0 && !segments))
        return fail("null argument");
    if (n_children >= (int64_t)1 << 30) return fail("too many children: %lld", (long long)n_children);
    if (!edges && step < 0) return fail("negative step");
    if (edges && n_edges < 0) return fail("negative edge count");
    CHECK(settle(c));
    NestedLay L;
    CHECK(nested_batch_layout(c, chain_mask, false, L));
    if (L.total > CLEANUP_MAX_BINS) return fail("too many bins: %lld (limit 2^31 - 2)", (long long)L.total);
    const int nc = (int)L.len.size();
    for (int i = 0; i < nc; ++i)
        if (L.taken[(size_t)i]) CHECK(cleanup_check_policy(policies[i]));
    *n_segments = 0;
    if (n_children == 0) return 0;
    const size_t nk = (size_t)n_children;
    std::vector<csr_cleanup_child> kids(nk);
    std::vector<int64_t> shift(nk);
    std::vector<int32_t> chain(nk);
    for (size_t k = 0; k < nk; ++k) {
        const csr_cleanup_batch_child &r = children[k];
        if (r.chain < 0 || r.chain >= nc) return fail("child %zu: chain index out of range", k);
        if (!L.taken[(size_t)r.chain]) return fail("child %zu: chain %d is not part of this call", k, r.chain);
        if (r.start < 0 || r.end < r.start || r.end >= L.len[(size_t)r.chain])
            return fail("child %zu: bins [%lld, %lld] are outside chain %d", k, (long long)r.start, (long long)r.end, r.chain);
        if (k > 0 && (children[k - 1].chain > r.chain || (children[k - 1].chain == r.chain && children[k - 1].end >= r.start)))
            return fail("child %zu: children must be disjoint and ascending by (chain, start)", k);
        const int64_t len = r.end - r.start + 1;
        if (edges) {
            if (r.edge_base < 0 || r.edge_base + len + 1 > n_edges) return fail("child %zu: its edges are outside the edge array", k);
            for (int64_t i = 0; i < len; ++i)
                if (edges[r.edge_base + i + 1] < edges[r.edge_base + i]) return fail("bin edges must not decrease (child %zu)", k);
        }
        kids[k].start = L.off[(size_t)r.chain] + r.start;
        kids[k].end = L.off[(size_t)r.chain] + r.end;
        shift[k] = r.edge_base - kids[k].start;
        chain[k] = r.chain;
    }
    csr_ctx::CleanupWs &ws = c->cleanupWs;
    auto pad = [](size_t b) { return (b + 255) / 256 * 256; };
    const size_t oEdge = 0, oShift = pad(edges ? 8 * (size_t)n_edges : 0), oChain = oShift + pad(8 * nk), oPol = oChain + pad(4 * nk),
                 bytes = oPol + pad(sizeof(csr_cleanup_policy) * (size_t)nc);
    CHECK(ws.arena.reserve(bytes));
    CHECK(ws.work.reserve(8 * (size_t)L.total + 64));
    CHECK(ws.kids.reserve(sizeof(csr_cleanup_child) * nk));
    CHECK(ws.seg.reserve(sizeof(csr_cleanup_segment) * CSR_CLEANUP_MAX_SEGMENTS * nk));
    CHECK(ws.cnt.reserve(sizeof(csr_cleanup_counts) * nk));
    char *base = (char *)ws.arena.ptr;
    if (edges) HIPOK(hipMemcpyAsync(base + oEdge, edges, 8 * (size_t)n_edges, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemcpyAsync(base + oShift, shift.data(), 8 * nk, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemcpyAsync(base + oChain, chain.data(), 4 * nk, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemcpyAsync(base + oPol, policies, sizeof(csr_cleanup_policy) * (size_t)nc, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemcpyAsync(ws.kids.ptr, kids.data(), sizeof(csr_cleanup_child) * nk, hipMemcpyHostToDevice, c->stream));
    CleanupArgs a;
    memset(&a, 0, sizeof(a));
    a.scores = L.scores;
    a.work = (double *)ws.work.ptr;
    a.co.edges = edges ? (const int64_t *)(base + oEdge) : nullptr;
    a.co.step = step;
    a.kids = (const csr_cleanup_child *)ws.kids.ptr;
    a.seg = (csr_cleanup_segment *)ws.seg.ptr;
    a.cnt = (csr_cleanup_counts *)ws.cnt.ptr;
    a.nKids = n_children;
    a.op = CSR_CLEANUP_OP_FORCE;
    a.shift = (const int64_t *)(base + oShift);
    a.kidChain = (const int32_t *)(base + oChain);
    a.pols = (const csr_cleanup_policy *)(base + oPol);
    CHECK(launch(c, "cleanup_plan", "k_cleanup_plan", k_cleanup_plan, dim3((unsigned)nk), dim3(64), 0, c->stream, a));
    std::vector<csr_cleanup_segment> seg(CSR_CLEANUP_MAX_SEGMENTS * nk);
    HIPOK(hipMemcpyAsync(counts, ws.cnt.ptr, sizeof(csr_cleanup_counts) * nk, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipMemcpyAsync(seg.data(), ws.seg.ptr, sizeof(csr_cleanup_segment) * seg.size(), hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    CHECK(cleanup_pack_checked(n_children, seg.data(), counts, capacity, segments, n_segments));
    // the segments come back in chain bins
    for (int64_t s = 0; s < *n_segments; ++s) {
        const int64_t off = L.off[(size_t)chain[(size_t)segments[s].child]];
        segments[s].start -= off;
        segments[s].end -= off;
    }
    return 0;
}
