// csr_host_export.inl -- part of csr_lib.hip (one translation unit; included after csr_host_nested.inl): the narrowPeak export call
// over the lanes of csr_export.h, on host arrays (default context) and on a batch context's resident score tracks and smoothed
// fit.  The job, order, state, mask, back-pointer and work buffers are the nested refinement's (csr_ctx::nestedWs); the parent
// records, the peak bases and the peaks are csr_ctx::exportWs.  The peaks stay on the device until csr_export_fetch.

static int export_check_cfg(const csr_export_cfg &g, bool hasParents) {
    if (!std::isfinite(g.multiplier) || g.multiplier < 0.0)
        return value_error("`exportFilterUncertaintyMultiplier` must be finite and non-negative");
    if (!hasParents || !g.split) return 0;
    if (!std::isfinite(g.boundary_cost)) return value_error("`boundaryCosts` must be finite and non-negative");
    if (!std::isfinite(g.selection_penalty)) return value_error("`selectionPenalty` must be finite");
    return 0;
}

// parents -> jobs: ascending by (chain, start), disjoint, inside their chain, of a chain the call takes
static int export_jobs(const NestedLay &L, const csr_export_cfg *cfg, int64_t np, const csr_export_parent *pa, std::vector<NestedJob> &jobs,
                       std::vector<unsigned char> &has) {
    if (np < 0 || (np > 0 && !pa)) return fail("null or negative parent list");
    if (np >= (int64_t)1 << 30) return fail("too many parents: %lld", (long long)np);
    jobs.resize((size_t)np);
    has.assign(L.len.size(), 0);
    int64_t words = 0;
    for (int64_t k = 0; k < np; ++k) {
        const csr_export_parent &r = pa[k];
        if (r.chain < 0 || r.chain >= (int)L.len.size()) return fail("parent %lld: chain index out of range", (long long)k);
        if (!L.taken[r.chain]) return fail("parent %lld: chain %d is not part of this call", (long long)k, r.chain);
        if (r.start < 0 || r.end < r.start || r.end >= L.len[r.chain])
            return fail("parent %lld: bins [%lld, %lld] are outside chain %d", (long long)k, (long long)r.start, (long long)r.end, r.chain);
        if (k > 0 && (pa[k - 1].chain > r.chain || (pa[k - 1].chain == r.chain && pa[k - 1].end >= r.start)))
            return fail("parent %lld: parents must be disjoint and ascending by (chain, start)", (long long)k);
        const int64_t n = r.end - r.start + 1;
        const int64_t m = std::min<int64_t>(std::max<int64_t>(cfg[r.chain].min_run, 1), n);
        if (cfg[r.chain].split && m > NESTED_MAX_MIN_RUN)
            return value_error("`minRunBins` %lld exceeds the supported maximum %d", (long long)m, NESTED_MAX_MIN_RUN);
        NestedJob &jb = jobs[(size_t)k];
        jb.off = L.off[r.chain] + r.start;
        jb.n = n;
        jb.start = r.start;
        jb.word = words;
        jb.required = -1;
        jb.costs = nullptr;
        jb.minRun = (int32_t)std::min<int64_t>(m, NESTED_MAX_MIN_RUN);
        jb.chain = r.chain;
        jb.uniform = 1;
        jb.reserved = 0;
        has[(size_t)r.chain] = 1;
        words += (n + NESTED_WORD - 1) / NESTED_WORD;
    }
    return 0;
}

static int export_run(csr_ctx *c, const NestedLay &L, const ExportTrack &sig, const ExportTrack &unc, const csr_export_cfg *cfg,
                      const std::vector<NestedJob> &jobs, int32_t *pflags, int64_t *count) {
    csr_ctx::NestedWs &ws = c->nestedWs;
    csr_ctx::ExportWs &ew = c->exportWs;
    const int nj = (int)jobs.size(), nc = (int)L.len.size();
    ew.nPeaks = 0;
    *count = 0;
    if (nj == 0) return 0;
    int64_t words = 0;
    for (const NestedJob &jb : jobs) words += (jb.n + NESTED_WORD - 1) / NESTED_WORD;
    std::vector<NestedChain> chains((size_t)nc);
    std::vector<ExportChain> ec((size_t)nc);
    for (int i = 0; i < nc; ++i) {
        memset(&chains[(size_t)i], 0, sizeof(NestedChain));
        memset(&ec[(size_t)i], 0, sizeof(ExportChain));
        if (!L.taken[(size_t)i]) continue;
        chains[(size_t)i].internal = cfg[i].boundary_cost > 0.0 ? cfg[i].boundary_cost : 0.0;
        ec[(size_t)i].penalty = cfg[i].selection_penalty;
        ec[(size_t)i].floor = cfg[i].trim_floor;
        ec[(size_t)i].multiplier = cfg[i].multiplier;
        ec[(size_t)i].split = cfg[i].split != 0;
        ec[(size_t)i].trim = cfg[i].trim != 0 && std::isfinite(cfg[i].trim_floor);
        ec[(size_t)i].filter = cfg[i].filter != 0;
    }
    // lanes in descending order of length; the DP lanes are the parents of chains that split
    std::vector<int> all((size_t)nj), reg, wide;
    for (int k = 0; k < nj; ++k) all[(size_t)k] = k;
    std::stable_sort(all.begin(), all.end(), [&](int a, int b) { return jobs[(size_t)a].n > jobs[(size_t)b].n; });
    for (int k : all)
        if (ec[(size_t)jobs[(size_t)k].chain].split) (jobs[(size_t)k].minRun <= NESTED_REG_STATES ? reg : wide).push_back(k);
    std::vector<int> order(all);
    order.insert(order.end(), reg.begin(), reg.end());
    order.insert(order.end(), wide.begin(), wide.end());
    auto pad = [](size_t b) { return (b + 255) / 256 * 256; };
    const size_t oJob = 0, oCh = pad(nj * sizeof(NestedJob)), oEc = oCh + pad(nc * sizeof(NestedChain)), oOrd = oEc + pad(nc * sizeof(ExportChain)),
                 tabBytes = oOrd + pad(order.size() * sizeof(int));
    CHECK(ws.jobBuf.reserve(tabBytes));
    CHECK(ws.work.reserve(8 * (size_t)L.total + 64));
    CHECK(ws.wm.reserve((size_t)L.total + 64));
    CHECK(ws.bt.reserve(8 * (size_t)words + 64));
    CHECK(ws.st.reserve(sizeof(NestedState) * (size_t)nj));
    CHECK(ew.par.reserve(sizeof(ExportParent) * (size_t)nj));
    CHECK(ew.base.reserve(8 * (size_t)nj));
    char *tab = (char *)ws.jobBuf.ptr;
    HIPOK(hipMemcpyAsync(tab + oJob, jobs.data(), nj * sizeof(NestedJob), hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemcpyAsync(tab + oCh, chains.data(), nc * sizeof(NestedChain), hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemcpyAsync(tab + oEc, ec.data(), nc * sizeof(ExportChain), hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemcpyAsync(tab + oOrd, order.data(), order.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    ExportArgs a;
    memset(&a, 0, sizeof(a));
    a.na.jobs = (const NestedJob *)(tab + oJob);
    a.na.chains = (const NestedChain *)(tab + oCh);
    a.na.scores = a.na.raw = L.scores;
    a.na.work = (double *)ws.work.ptr;
    a.na.bt = (unsigned long long *)ws.bt.ptr;
    a.na.wm = (unsigned char *)ws.wm.ptr;
    a.na.st = (NestedState *)ws.st.ptr;
    a.cfg = (const ExportChain *)(tab + oEc);
    a.sig = sig;
    a.unc = unc;
    a.par = (ExportParent *)ew.par.ptr;
    a.base = (const int64_t *)ew.base.ptr;
    a.nParents = nj;
    const int *dAll = (const int *)(tab + oOrd), *dReg = dAll + nj, *dWide = dReg + reg.size();
    const dim3 lanes((unsigned)((nj + 63) / 64));
    std::vector<ExportParent> par((size_t)nj);
    {
        Scope sc(c, "export_parents");
        CHECK(launch(c, nullptr, "k_export_prep", k_export_prep, lanes, dim3(64), 0, c->stream, a, dAll, nj));
        HIPOK(hipMemcpyAsync(par.data(), ew.par.ptr, sizeof(ExportParent) * (size_t)nj, hipMemcpyDeviceToHost, c->stream));
        HIPOK(hipStreamSynchronize(c->stream));
        for (int k = 0; k < nj; ++k)
            if ((par[(size_t)k].flags & EXPORT_BAD_SCORES) && ec[(size_t)jobs[(size_t)k].chain].split) return value_error("`scores` contains non-finite values");
        if (!reg.empty())
            CHECK(launch(c, nullptr, "k_nested_dp_reg", k_nested_dp_reg, dim3((unsigned)((reg.size() + 63) / 64)), dim3(64), 0, c->stream, a.na,
                         dReg, (int)reg.size()));
        if (!wide.empty())
            CHECK(launch(c, nullptr, "k_nested_dp_wide", k_nested_dp_wide, dim3((unsigned)wide.size()), dim3(NESTED_WIDE_T), 0, c->stream, a.na,
                         dWide));
        CHECK(launch(c, nullptr, "k_export_finish", k_export_finish, lanes, dim3(64), 0, c->stream, a, dAll, nj));
    }
    HIPOK(hipMemcpyAsync(par.data(), ew.par.ptr, sizeof(ExportParent) * (size_t)nj, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    std::vector<int64_t> base((size_t)nj);
    int64_t total = 0;
    for (int k = 0; k < nj; ++k) {
        const ExportParent &r = par[(size_t)k];
        if (r.flags & EXPORT_INFEASIBLE) return fail("parent-conditioned subpeak DP found no feasible path (parent %d)", k);
        if (r.count < 1 || (int64_t)r.count > jobs[(size_t)k].n) return fail("narrowPeak export: bad child count (parent %d)", k);
        if (pflags) pflags[k] = (r.flags & EXPORT_BAD_SIGNAL) ? CSR_EXPORT_NONFINITE_SIGNAL : 0;
        base[(size_t)k] = total;
        total += r.count;
    }
    CHECK(ew.peaks.reserve(sizeof(csr_export_peak) * (size_t)total));
    HIPOK(hipMemcpyAsync(ew.base.ptr, base.data(), 8 * (size_t)nj, hipMemcpyHostToDevice, c->stream));
    a.peaks = (csr_export_peak *)ew.peaks.ptr;
    a.nPeaks = total;
    CHECK(launch(c, "export_children", "k_export_child", k_export_child, dim3((unsigned)((total + 63) / 64)), dim3(64), 0, c->stream, a));
    HIPOK(hipStreamSynchronize(c->stream));
    ew.nPeaks = total;
    *count = total;
    return 0;
}

extern "C" int csr_export_fetch(csr_ctx *c, int64_t capacity, csr_export_peak *peaks) {
    DEFAULT_CTX_GUARD;
    if (capacity < 0 || (capacity > 0 && !peaks)) return fail("bad capacity / output buffer");
    CHECK(ctx_or_default(c));
    const int64_t take = std::min(capacity, c->exportWs.nPeaks);
    if (take > 0) {
        HIPOK(hipMemcpyAsync(peaks, c->exportWs.peaks.ptr, sizeof(csr_export_peak) * (size_t)take, hipMemcpyDeviceToHost, c->stream));
        HIPOK(hipStreamSynchronize(c->stream));
    }
    return 0;
}

// host arrays (default context).  arena: scores | state | uncertainty
extern "C" int csr_export_peaks(int32_t n_chains, const int64_t *chain_len, const double *state, const double *scores,
                                const double *uncertainty, const csr_export_cfg *cfg, int64_t n_parents, const csr_export_parent *parents,
                                int32_t *parent_flags, int64_t *count) {
    DEFAULT_CTX_GUARD;
    if (n_chains <= 0 || !chain_len || !state || !scores || !cfg || !count) return fail("null or empty argument");
    NestedLay L;
    L.off.resize((size_t)n_chains);
    L.len.assign(chain_len, chain_len + n_chains);
    L.taken.assign((size_t)n_chains, 1);
    L.total = 0;
    for (int i = 0; i < n_chains; ++i) {
        if (chain_len[i] < 0) return fail("chain %d: negative length", i);
        L.off[(size_t)i] = L.total;
        L.total += chain_len[i];
    }
    if (L.total >= ((int64_t)1 << 31) - 1) return fail("too many bins: %lld (limit 2^31 - 2)", (long long)L.total);
    std::vector<NestedJob> jobs;
    std::vector<unsigned char> has;
    CHECK(export_jobs(L, cfg, n_parents, parents, jobs, has));
    for (int i = 0; i < n_chains; ++i) CHECK(export_check_cfg(cfg[i], has[(size_t)i] != 0));
    for (const NestedJob &jb : jobs)
        if (cfg[jb.chain].split) CHECK(nested_value_vector("scores", scores + jb.off, jb.n));
    *count = 0;
    if (jobs.empty()) {
        csr_ctx *c0 = nullptr;
        CHECK(ctx_or_default(c0));
        c0->exportWs.nPeaks = 0;
        return 0;
    }
    csr_ctx *c = nullptr;
    CHECK(ctx_or_default(c));
    const size_t bytes = 8 * (size_t)L.total;
    CHECK(c->exportWs.arena.reserve(3 * bytes + 64));
    char *base = (char *)c->exportWs.arena.ptr;
    HIPOK(hipMemcpyAsync(base, scores, bytes, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemcpyAsync(base + bytes, state, bytes, hipMemcpyHostToDevice, c->stream));
    if (uncertainty) HIPOK(hipMemcpyAsync(base + 2 * bytes, uncertainty, bytes, hipMemcpyHostToDevice, c->stream));
    L.scores = L.raw = (const double *)base;
    ExportTrack sig, unc;
    memset(&sig, 0, sizeof(sig));
    memset(&unc, 0, sizeof(unc));
    sig.d = (const double *)(base + bytes);
    if (uncertainty) unc.d = (const double *)(base + 2 * bytes);
    return export_run(c, L, sig, unc, cfg, jobs, parent_flags, count);
}

// Which resident track the batch's export stages (narrowPeak, clean-up's second pass, broad rows) read as signal: the state
// (double) xs[:,0] of the reference-layout fit (the default), or the shrunk state csr_batch_shrink_posterior left (float32, one
// value per bin).  Belongs to the batch (csr_batch_configure puts it back to the state).
extern "C" int csr_batch_set_export_signal(csr_ctx *c, int32_t signal) {
    CHECK(need(c));
    if (signal != CSR_SIGNAL_STATE && signal != CSR_SIGNAL_SHRUNK) return fail("bad export signal %d", signal);
    c->exportSignal = signal;
    return 0;
}
// sig := that track; a taken chain without a shrunk track fails before any launch
template <class V>
static int batch_export_signal(csr_ctx *c, const V &taken, ExportTrack &sig) {
    if (c->exportSignal == CSR_SIGNAL_SHRUNK) {
        for (size_t i = 0; i < taken.size(); ++i)
            if (taken[i] && !c->shrunk.has((int)i)) return fail("chain %d has no %s", (int)i, c->shrunk.what);
        sig.f = c->shrunk.d;
        sig.stride = 1;
    } else {
        sig.f = c->nat[CSR_ARR_XS];
        sig.stride = c->mdl.state_dim;
    }
    return 0;
}

// batch context: the resident score tracks and the reference-layout copies of the smoothed fit are read; nothing resident changes
extern "C" int csr_batch_export_peaks(csr_ctx *c, const csr_export_cfg *cfg, const unsigned char *chain_mask, int64_t n_parents,
                                      const csr_export_parent *parents, int32_t *parent_flags, int64_t *count) {
    CHECK(need(c));
    if (!cfg || !count) return fail("null argument");
    CHECK(settle(c));
    NestedLay L;
    CHECK(nested_batch_layout(c, chain_mask, false, L));
    std::vector<NestedJob> jobs;
    std::vector<unsigned char> has;
    CHECK(export_jobs(L, cfg, n_parents, parents, jobs, has));
    for (size_t i = 0; i < L.len.size(); ++i)
        if (L.taken[i]) CHECK(export_check_cfg(cfg[i], has[i] != 0));
    *count = 0;
    c->exportWs.nPeaks = 0;
    if (jobs.empty()) return 0;
    if (!c->haveBwd) return fail("no smoothed results to export peaks from");
    // the conversion csr_batch_export(CSR_EXPORT_SMOOTH) makes, a no-op when the reference-layout copies are current
    CHECK(export_impl(c, CSR_EXPORT_SMOOTH));
    ExportTrack sig, unc;
    memset(&sig, 0, sizeof(sig));
    memset(&unc, 0, sizeof(unc));
    const int d = c->mdl.state_dim;
    CHECK(batch_export_signal(c, L.taken, sig));
    bool filter = false;
    for (size_t i = 0; i < L.len.size(); ++i) filter = filter || (L.taken[i] && cfg[i].filter);
    if (filter) {
        unc.f = c->nat[CSR_ARR_PS];
        unc.stride = (int64_t)d * d;
        unc.root = 1;
    }
    return export_run(c, L, sig, unc, cfg, jobs, parent_flags, count);
}
