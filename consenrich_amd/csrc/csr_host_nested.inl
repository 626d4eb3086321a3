// csr_host_nested.inl -- part of csr_lib.hip (one translation unit; included in this order): nested ROCCO refinement -- the
// layer, node and selected-sum calls over the lanes of csr_nested.h, on host arrays (default context) and on a batch context's
// resident scores and solution masks.  Everything the reference answers with ValueError is checked before a context is touched.

// where the chains of a call live on the device
struct NestedLay {
    std::vector<int64_t> off, len;      // per chain: first bin in the device arrays, bins
    std::vector<unsigned char> taken;   // the chains the call may touch
    int64_t total = 0;                  // bins the device arrays span
    const double *scores = nullptr, *raw = nullptr;
    unsigned char *sol = nullptr;
};

static int nested_value_vector(const char *name, const double *x, int64_t n) {
    for (int64_t i = 0; i < n; ++i)
        if (!std::isfinite(x[i])) return value_error("`%s` contains non-finite values", name);
    return 0;
}
static int nested_check_cfg(const csr_nested_cfg &g) {
    if (!std::isfinite(g.gamma) || g.gamma < 0.0) return value_error("`gamma` must be finite and non-negative");
    if (!std::isfinite(g.selection_penalty)) return value_error("`selectionPenalty` must be finite");
    if (!std::isfinite(g.budget_scale)) return value_error("`nestedRoccoBudgetScale` must be finite");
    return 0;
}
// regions -> jobs: ascending by (chain, start), disjoint, inside their chain, of a chain the call takes
static int nested_jobs(const NestedLay &L, int64_t nr, const csr_nested_region *rg, std::vector<NestedJob> &jobs) {
    if (nr < 0 || (nr > 0 && !rg)) return fail("null or negative region list");
    if (nr >= (int64_t)1 << 30) return fail("too many regions: %lld", (long long)nr);
    jobs.resize((size_t)nr);
    int64_t words = 0;
    for (int64_t k = 0; k < nr; ++k) {
        const csr_nested_region &r = rg[k];
        if (r.chain < 0 || r.chain >= (int)L.len.size()) return fail("region %lld: chain index out of range", (long long)k);
        if (!L.taken[r.chain]) return fail("region %lld: chain %d is not part of this call", (long long)k, r.chain);
        if (r.start < 0 || r.end < r.start || r.end >= L.len[r.chain])
            return fail("region %lld: bins [%lld, %lld] are outside chain %d", (long long)k, (long long)r.start, (long long)r.end, r.chain);
        if (k > 0 && (rg[k - 1].chain > r.chain || (rg[k - 1].chain == r.chain && rg[k - 1].end >= r.start)))
            return fail("region %lld: regions must be disjoint and ascending by (chain, start)", (long long)k);
        const int64_t n = r.end - r.start + 1;
        const int64_t m = std::min<int64_t>(std::max<int64_t>(r.min_run, 1), n);
        if (m > NESTED_MAX_MIN_RUN)
            return value_error("`minRunBins` %lld exceeds the supported maximum %d", (long long)m, NESTED_MAX_MIN_RUN);
        NestedJob &jb = jobs[(size_t)k];
        jb.off = L.off[r.chain] + r.start;
        jb.n = n;
        jb.start = r.start;
        jb.word = words;
        jb.required = -1;
        jb.costs = nullptr;
        jb.minRun = (int32_t)m;
        jb.chain = r.chain;
        jb.uniform = 0;
        jb.reserved = 0;
        words += (n + NESTED_WORD - 1) / NESTED_WORD;
    }
    return 0;
}

// One layer (solve == nullptr), or one region with the caller's costs, penalty and required bin (its state in *solve).
static int nested_run(csr_ctx *c, const NestedLay &L, std::vector<NestedJob> &jobs, const std::vector<NestedChain> &chains,
                      const NestedState *solve, csr_nested_rec *rec, int64_t *nKids) {
    csr_ctx::NestedWs &ws = c->nestedWs;
    const int nj = (int)jobs.size();
    ws.nKids = 0;
    if (nKids) *nKids = 0;
    if (nj == 0) return 0;
    int64_t words = 0, kidCap = 0;
    for (const NestedJob &jb : jobs) {
        words += (jb.n + NESTED_WORD - 1) / NESTED_WORD;
        kidCap += std::max<int64_t>(1, (jb.n + 1) / (jb.minRun + 1));      // runs of >= minRun bins, a gap between two
    }
    // lanes in descending order of length: the lanes of a wavefront finish together
    std::vector<int> all((size_t)nj), reg, wide;
    for (int k = 0; k < nj; ++k) all[(size_t)k] = k;
    std::stable_sort(all.begin(), all.end(), [&](int a, int b) { return jobs[(size_t)a].n > jobs[(size_t)b].n; });
    for (int k : all) (jobs[(size_t)k].minRun <= NESTED_REG_STATES ? reg : wide).push_back(k);
    std::vector<int> order(all);
    order.insert(order.end(), reg.begin(), reg.end());
    order.insert(order.end(), wide.begin(), wide.end());
    // work space
    const size_t oJob = 0, oCh = (nj * sizeof(NestedJob) + 255) / 256 * 256, oOrd = oCh + (chains.size() * sizeof(NestedChain) + 255) / 256 * 256,
                 oCnt = oOrd + (order.size() * sizeof(int) + 255) / 256 * 256, tabBytes = oCnt + 256;
    CHECK(ws.jobBuf.reserve(tabBytes));
    CHECK(ws.work.reserve(8 * (size_t)L.total + 64));
    CHECK(ws.wm.reserve((size_t)L.total + 64));
    CHECK(ws.bt.reserve(8 * (size_t)words + 64));
    CHECK(ws.st.reserve(sizeof(NestedState) * (size_t)nj));
    CHECK(ws.rec.reserve(sizeof(csr_nested_rec) * (size_t)nj));
    CHECK(ws.kids.reserve(sizeof(csr_nested_node) * (size_t)kidCap));
    char *tab = (char *)ws.jobBuf.ptr;
    HIPOK(hipMemcpyAsync(tab + oJob, jobs.data(), nj * sizeof(NestedJob), hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemcpyAsync(tab + oCh, chains.data(), chains.size() * sizeof(NestedChain), hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemcpyAsync(tab + oOrd, order.data(), order.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemsetAsync(tab + oCnt, 0, 8, c->stream));
    if (solve) HIPOK(hipMemcpyAsync(ws.st.ptr, solve, sizeof(NestedState), hipMemcpyHostToDevice, c->stream));
    NestedArgs a;
    a.jobs = (const NestedJob *)(tab + oJob);
    a.chains = (const NestedChain *)(tab + oCh);
    a.scores = L.scores;
    a.raw = L.raw;
    a.work = (double *)ws.work.ptr;
    a.bt = (unsigned long long *)ws.bt.ptr;
    a.wm = (unsigned char *)ws.wm.ptr;
    a.sol = L.sol;
    a.st = (NestedState *)ws.st.ptr;
    a.rec = (csr_nested_rec *)ws.rec.ptr;
    a.kids = solve ? nullptr : (csr_nested_node *)ws.kids.ptr;
    a.kidCount = (unsigned long long *)(tab + oCnt);
    a.kidCap = kidCap;
    const int *dAll = (const int *)(tab + oOrd), *dReg = dAll + nj, *dWide = dReg + reg.size();
    const dim3 lanes((unsigned)((nj + 63) / 64));
    {
        Scope sc(c, "nested_layer");
        if (!solve) CHECK(launch(c, nullptr, "k_nested_prep", k_nested_prep, lanes, dim3(64), 0, c->stream, a, dAll, nj));
        if (!reg.empty())
            CHECK(launch(c, nullptr, "k_nested_dp_reg", k_nested_dp_reg, dim3((unsigned)((reg.size() + 63) / 64)), dim3(64), 0, c->stream, a,
                         dReg, (int)reg.size()));
        if (!wide.empty())
            CHECK(launch(c, nullptr, "k_nested_dp_wide", k_nested_dp_wide, dim3((unsigned)wide.size()), dim3(NESTED_WIDE_T), 0, c->stream, a,
                         dWide));
        CHECK(launch(c, nullptr, "k_nested_finish", k_nested_finish, lanes, dim3(64), 0, c->stream, a, dAll, nj));
    }
    unsigned long long kids = 0;
    HIPOK(hipMemcpyAsync(rec, ws.rec.ptr, sizeof(csr_nested_rec) * (size_t)nj, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipMemcpyAsync(&kids, tab + oCnt, 8, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    for (int k = 0; k < nj; ++k) {
        if (rec[k].decision == CSR_NESTED_INFEASIBLE) return fail("parent-conditioned subpeak DP found no feasible path (region %d)", k);
        if (!solve && rec[k].n_runs > 0 && rec[k].child_base < 0) return fail("nested ROCCO: child records overflowed (region %d)", k);
    }
    if (!solve) {
        ws.nKids = (int64_t)kids;
        if (nKids) *nKids = (int64_t)kids;
    }
    return 0;
}

static std::vector<NestedChain> nested_chain_table(int nc, const csr_nested_cfg *cfg, const std::vector<unsigned char> &taken) {
    std::vector<NestedChain> t((size_t)nc);
    for (int i = 0; i < nc; ++i) {
        NestedChain &p = t[(size_t)i];
        memset(&p, 0, sizeof(p));
        if (!taken[(size_t)i]) continue;
        p.internal = std::max(0.25 * cfg[i].gamma, 1000.0 * NESTED_EDGE);
        p.base = cfg[i].selection_penalty;
        p.scale = cfg[i].budget_scale;
        p.useFloor = cfg[i].subtract_floor != 0;
    }
    return t;
}

static int nested_nodes_run(csr_ctx *c, const NestedLay &L, const std::vector<NestedJob> &jobs, csr_nested_node *nodes) {
    const int nj = (int)jobs.size();
    if (nj == 0) return 0;
    csr_ctx::NestedWs &ws = c->nestedWs;
    CHECK(ws.jobBuf.reserve(nj * sizeof(NestedJob)));
    CHECK(ws.rec.reserve(nj * sizeof(csr_nested_node)));
    HIPOK(hipMemcpyAsync(ws.jobBuf.ptr, jobs.data(), nj * sizeof(NestedJob), hipMemcpyHostToDevice, c->stream));
    CHECK(launch(c, "nested_nodes", "k_nested_nodes", k_nested_nodes, dim3((unsigned)((nj + 63) / 64)), dim3(64), 0, c->stream,
                 (const NestedJob *)ws.jobBuf.ptr, nj, L.scores, L.raw, (csr_nested_node *)ws.rec.ptr));
    HIPOK(hipMemcpyAsync(nodes, ws.rec.ptr, nj * sizeof(csr_nested_node), hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    return 0;
}

// the runs of every taken chain: checked, and turned into copies into one compact array
static int nested_sum_plan(const NestedLay &L, const int64_t *n_runs, const int64_t *starts, const int64_t *ends,
                           std::vector<NestedRun> &runs, std::vector<NestedSumJob> &sums) {
    if (!n_runs) return fail("null argument");
    runs.clear();
    sums.assign(L.len.size(), NestedSumJob{0, 0});
    int64_t k = 0, dst = 0;
    for (size_t ch = 0; ch < L.len.size(); ++ch) {
        if (n_runs[ch] < 0) return fail("chain %d: negative run count", (int)ch);
        if (n_runs[ch] > 0 && (!starts || !ends)) return fail("null argument");
        if (n_runs[ch] > 0 && !L.taken[ch]) return fail("chain %d is not part of this call", (int)ch);
        sums[ch].src = dst;
        int64_t prev = -1;
        for (int64_t q = 0; q < n_runs[ch]; ++q, ++k) {
            if (starts[k] <= prev || ends[k] < starts[k] || ends[k] >= L.len[ch])
                return fail("chain %d: runs must be ascending, disjoint and inside the chain", (int)ch);
            prev = ends[k];
            const int64_t n = ends[k] - starts[k] + 1;
            runs.push_back(NestedRun{L.off[ch] + starts[k], dst, n});
            dst += n;
        }
        sums[ch].n = dst - sums[ch].src;
    }
    return 0;
}
static int nested_sum_run(csr_ctx *c, const NestedLay &L, const std::vector<NestedRun> &runs, const std::vector<NestedSumJob> &sums,
                          double *out) {
    const int nc = (int)sums.size();
    for (int i = 0; i < nc; ++i) out[i] = 0.0;
    if (runs.empty()) return 0;
    csr_ctx::NestedWs &ws = c->nestedWs;
    int64_t most = 1, total = 0;
    for (const NestedSumJob &s : sums) { most = std::max(most, s.n); total += s.n; }
    const int64_t maxChunks = (most + NP_CHUNK - 1) / NP_CHUNK;
    const size_t oRun = 0, oSum = (runs.size() * sizeof(NestedRun) + 255) / 256 * 256,
                 oOut = oSum + (nc * sizeof(NestedSumJob) + 255) / 256 * 256, tabBytes = oOut + 8 * (size_t)nc;
    CHECK(ws.jobBuf.reserve(tabBytes));
    CHECK(ws.work.reserve(8 * (size_t)total + 64));
    CHECK(ws.part.reserve(8 * (size_t)maxChunks * (size_t)nc));
    char *tab = (char *)ws.jobBuf.ptr;
    HIPOK(hipMemcpyAsync(tab + oRun, runs.data(), runs.size() * sizeof(NestedRun), hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemcpyAsync(tab + oSum, sums.data(), nc * sizeof(NestedSumJob), hipMemcpyHostToDevice, c->stream));
    {
        Scope sc(c, "nested_selected_sum");
        CHECK(launch(c, nullptr, "k_nested_gather", k_nested_gather, dim3((unsigned)runs.size()), dim3(256), 0, c->stream,
                     (const NestedRun *)(tab + oRun), L.scores, (double *)ws.work.ptr));
        CHECK(launch(c, nullptr, "k_nested_sum", k_np_chunk_sums<NestedSumJob>, dim3((unsigned)((maxChunks + 63) / 64), (unsigned)nc), dim3(64), 0, c->stream,
                     (const NestedSumJob *)(tab + oSum), (const double *)ws.work.ptr, (double *)ws.part.ptr, maxChunks));
        CHECK(launch(c, nullptr, "k_nested_fold", k_np_fold<NestedSumJob>, dim3((unsigned)((nc + 63) / 64)), dim3(64), 0, c->stream,
                     (const NestedSumJob *)(tab + oSum), nc, (const double *)ws.part.ptr, maxChunks, (double *)(tab + oOut)));
    }
    HIPOK(hipMemcpyAsync(out, tab + oOut, 8 * (size_t)nc, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// host arrays (default context)
// ---------------------------------------------------------------------------------------------------------------
static int nested_host_layout(int32_t n_chains, const int64_t *chain_len, const double *scores, const double *raw, NestedLay &L) {
    if (n_chains <= 0 || !chain_len || !scores) return fail("null or empty argument");
    L.off.resize((size_t)n_chains);
    L.len.assign(chain_len, chain_len + n_chains);
    L.taken.assign((size_t)n_chains, 1);
    L.total = 0;
    for (int i = 0; i < n_chains; ++i) {
        if (chain_len[i] <= 0) return value_error("`scores` must be non-empty");
        L.off[(size_t)i] = L.total;
        L.total += chain_len[i];
    }
    // (a region's counts are ints and n + 1 stands for "no path": the same limit as csr_nested_solve)
    if (L.total >= ((int64_t)1 << 31) - 1) return fail("too many bins: %lld (limit 2^31 - 2)", (long long)L.total);
    CHECK(nested_value_vector("scores", scores, L.total));
    if (raw) CHECK(nested_value_vector("rawScores", raw, L.total));
    return 0;
}
// arena: scores | raw scores | mask
static int nested_host_stage(csr_ctx *c, NestedLay &L, const double *scores, const double *raw, const uint8_t *solution) {
    const size_t oS = 0, oR = oS + 8 * (size_t)L.total, oM = oR + (raw ? 8 * (size_t)L.total : 0), total = oM + (size_t)L.total + 64;
    CHECK(c->nestedWs.arena.reserve(total));
    char *base = (char *)c->nestedWs.arena.ptr;
    HIPOK(hipMemcpyAsync(base + oS, scores, 8 * (size_t)L.total, hipMemcpyHostToDevice, c->stream));
    if (raw) HIPOK(hipMemcpyAsync(base + oR, raw, 8 * (size_t)L.total, hipMemcpyHostToDevice, c->stream));
    if (solution) HIPOK(hipMemcpyAsync(base + oM, solution, (size_t)L.total, hipMemcpyHostToDevice, c->stream));
    L.scores = (const double *)(base + oS);
    L.raw = raw ? (const double *)(base + oR) : L.scores;
    L.sol = (unsigned char *)(base + oM);
    return 0;
}

extern "C" int csr_nested_nodes(int32_t n_chains, const int64_t *chain_len, const double *scores, const double *raw_scores,
                                int64_t n_regions, const csr_nested_region *regions, csr_nested_node *nodes) {
    DEFAULT_CTX_GUARD;
    NestedLay L;
    CHECK(nested_host_layout(n_chains, chain_len, scores, raw_scores, L));
    if (n_regions > 0 && !nodes) return fail("null argument");
    std::vector<NestedJob> jobs;
    CHECK(nested_jobs(L, n_regions, regions, jobs));
    csr_ctx *c = nullptr;
    CHECK(ctx_or_default(c));
    CHECK(nested_host_stage(c, L, scores, raw_scores, nullptr));
    return nested_nodes_run(c, L, jobs, nodes);
}

extern "C" int csr_nested_layer(int32_t n_chains, const int64_t *chain_len, const double *scores, const double *raw_scores,
                                uint8_t *solution, const csr_nested_cfg *cfg, int64_t n_regions, const csr_nested_region *regions,
                                csr_nested_rec *rec, int64_t *n_children) {
    DEFAULT_CTX_GUARD;
    NestedLay L;
    CHECK(nested_host_layout(n_chains, chain_len, scores, raw_scores, L));
    if (!solution || !cfg || !n_children || (n_regions > 0 && !rec)) return fail("null argument");
    for (int i = 0; i < n_chains; ++i) CHECK(nested_check_cfg(cfg[i]));
    std::vector<NestedJob> jobs;
    CHECK(nested_jobs(L, n_regions, regions, jobs));
    csr_ctx *c = nullptr;
    CHECK(ctx_or_default(c));
    CHECK(nested_host_stage(c, L, scores, raw_scores, solution));
    CHECK(nested_run(c, L, jobs, nested_chain_table(n_chains, cfg, L.taken), nullptr, rec, n_children));
    HIPOK(hipMemcpyAsync(solution, L.sol, (size_t)L.total, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int csr_nested_children(csr_ctx *c, int64_t capacity, csr_nested_node *children) {
    DEFAULT_CTX_GUARD;
    if (capacity < 0 || (capacity > 0 && !children)) return fail("bad capacity / output buffer");
    CHECK(ctx_or_default(c));
    const int64_t take = std::min(capacity, c->nestedWs.nKids);
    if (take > 0) {
        HIPOK(hipMemcpyAsync(children, c->nestedWs.kids.ptr, sizeof(csr_nested_node) * (size_t)take, hipMemcpyDeviceToHost, c->stream));
        HIPOK(hipStreamSynchronize(c->stream));
    }
    return 0;
}

extern "C" int csr_nested_selected_sum(int32_t n_chains, const int64_t *chain_len, const double *scores, const int64_t *n_runs,
                                       const int64_t *starts, const int64_t *ends, double *sums) {
    DEFAULT_CTX_GUARD;
    NestedLay L;
    CHECK(nested_host_layout(n_chains, chain_len, scores, nullptr, L));
    if (!sums) return fail("null argument");
    std::vector<NestedRun> runs;
    std::vector<NestedSumJob> jobs;
    CHECK(nested_sum_plan(L, n_runs, starts, ends, runs, jobs));
    csr_ctx *c = nullptr;
    CHECK(ctx_or_default(c));
    CHECK(nested_host_stage(c, L, scores, nullptr, nullptr));
    return nested_sum_run(c, L, runs, jobs, sums);
}

extern "C" int csr_nested_solve(const double *scores, int64_t n, const double *boundary_costs, double selection_penalty,
                                int32_t min_run, int64_t required, double run_penalty, uint8_t *mask, csr_nested_rec *out) {
    DEFAULT_CTX_GUARD;
    if (!scores || n <= 0) return value_error("`scores` must be a non-empty one-dimensional array");
    if (!boundary_costs || !mask || !out) return fail("null argument");
    if (n >= ((int64_t)1 << 31) - 1) return fail("too many bins: %lld (limit 2^31 - 2)", (long long)n);
    CHECK(nested_value_vector("scores", scores, n));
    for (int64_t i = 0; i <= n; ++i)
        if (!std::isfinite(boundary_costs[i]) || boundary_costs[i] < 0.0) return value_error("`boundaryCosts` must be finite and non-negative");
    if (!std::isfinite(selection_penalty)) return value_error("`selectionPenalty` must be finite");
    if (!std::isfinite(run_penalty) || run_penalty < 0.0) return value_error("`runPenalty` must be finite and non-negative");
    if (required < -1 || required >= n) return value_error("`requiredIndex` is outside `scores`");
    NestedLay L;
    L.off = {0};
    L.len = {n};
    L.taken = {1};
    L.total = n;
    const csr_nested_region rg{0, n - 1, 0, min_run};
    std::vector<NestedJob> jobs;
    CHECK(nested_jobs(L, 1, &rg, jobs));
    csr_ctx *c = nullptr;
    CHECK(ctx_or_default(c));
    // arena: scores | mask | costs
    CHECK(nested_host_stage(c, L, scores, nullptr, nullptr));
    CHECK(c->nestedWs.costs.reserve(8 * (size_t)(n + 1)));
    HIPOK(hipMemcpyAsync(c->nestedWs.costs.ptr, boundary_costs, 8 * (size_t)(n + 1), hipMemcpyHostToDevice, c->stream));
    jobs[0].costs = (const double *)c->nestedWs.costs.ptr;
    NestedChain p;
    memset(&p, 0, sizeof(p));
    p.commitAlways = 1;
    NestedState s;
    memset(&s, 0, sizeof(s));
    s.penalty = selection_penalty;
    s.runPenalty = run_penalty;
    s.required = required;
    CHECK(nested_run(c, L, jobs, std::vector<NestedChain>{p}, &s, out, nullptr));
    HIPOK(hipMemcpyAsync(mask, L.sol, (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// batch context: the resident score tracks are read, the resident solution masks read and written
// ---------------------------------------------------------------------------------------------------------------
static int nested_batch_layout(csr_ctx *c, const unsigned char *chain_mask, bool needSol, NestedLay &L) {
    std::vector<int> idx;
    CHECK(select_chains(c, chain_mask, c->scores, idx, NO_SCORES));
    const size_t nc = c->chains.size();
    L.off.resize(nc);
    L.len.resize(nc);
    L.taken.assign(nc, 0);
    for (size_t i = 0; i < nc; ++i) { L.off[i] = c->chains[i].off; L.len[i] = c->chains[i].n; }
    for (int i : idx) {
        if (needSol && !c->sol.has(i)) return fail("chain %d has no ROCCO solution", i);
        L.taken[(size_t)i] = 1;
    }
    L.total = c->Npad + 64;
    L.scores = L.raw = c->scores.d;
    L.sol = c->sol.d;
    return 0;
}

extern "C" int csr_batch_nested_nodes(csr_ctx *c, int64_t n_regions, const csr_nested_region *regions, csr_nested_node *nodes) {
    CHECK(need(c));
    if (n_regions > 0 && !nodes) return fail("null argument");
    NestedLay L;
    std::vector<unsigned char> mask(c->chains.size(), 0);
    for (int64_t k = 0; k < n_regions && regions; ++k)
        if (regions[k].chain >= 0 && regions[k].chain < (int)mask.size()) mask[(size_t)regions[k].chain] = 1;
    CHECK(nested_batch_layout(c, mask.data(), false, L));
    std::vector<NestedJob> jobs;
    CHECK(nested_jobs(L, n_regions, regions, jobs));
    return nested_nodes_run(c, L, jobs, nodes);
}

extern "C" int csr_batch_nested_layer(csr_ctx *c, const csr_nested_cfg *cfg, const unsigned char *chain_mask, int64_t n_regions,
                                      const csr_nested_region *regions, csr_nested_rec *rec, int64_t *n_children) {
    CHECK(need(c));
    if (!cfg || !n_children || (n_regions > 0 && !rec)) return fail("null argument");
    const int nc = (int)c->chains.size();
    for (int i = 0; i < nc; ++i)
        if (!chain_mask || chain_mask[i]) CHECK(nested_check_cfg(cfg[i]));
    NestedLay L;
    CHECK(nested_batch_layout(c, chain_mask, true, L));
    std::vector<NestedJob> jobs;
    CHECK(nested_jobs(L, n_regions, regions, jobs));
    return nested_run(c, L, jobs, nested_chain_table(nc, cfg, L.taken), nullptr, rec, n_children);
}

extern "C" int csr_batch_nested_selected_sum(csr_ctx *c, const unsigned char *chain_mask, const int64_t *n_runs, const int64_t *starts,
                                             const int64_t *ends, double *sums) {
    CHECK(need(c));
    if (!sums) return fail("null argument");
    NestedLay L;
    CHECK(nested_batch_layout(c, chain_mask, false, L));
    std::vector<NestedRun> runs;
    std::vector<NestedSumJob> jobs;
    CHECK(nested_sum_plan(L, n_runs, starts, ends, runs, jobs));
    return nested_sum_run(c, L, runs, jobs, sums);
}
