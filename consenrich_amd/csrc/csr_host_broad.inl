// csr_host_broad.inl -- part of csr_lib.hip (one translation unit; included after csr_host_cleanup.inl): broad mode's gap sums and
// parent records over the lanes and wavefronts of csr_broad.h, on host arrays (default context) and on a batch context's resident
// tracks, and the batch's weak ROCCO pass and support runs.  Every argument check comes before a device is touched.  The work space
// is csr_ctx::broadWs: the staged arrays, one work double per bin, the job and chain tables, the parent mask, the records and the
// run tables.

static int broad_check_cfg(const csr_broad_cfg &g) {
    if (!std::isfinite(g.multiplier) || g.multiplier < 0.0)
        return value_error("`exportFilterUncertaintyMultiplier` must be finite and non-negative");
    return 0;
}

// parents -> jobs: ascending by (chain, start), disjoint, inside their chain
static int broad_jobs(const std::vector<int64_t> &off, const std::vector<int64_t> &len, const std::vector<char> *taken, int64_t np,
                      const csr_export_parent *pa, std::vector<BroadJob> &jobs) {
    if (np < 0 || (np > 0 && !pa)) return fail("null or negative parent list");
    if (np >= (int64_t)1 << 30) return fail("too many parents: %lld", (long long)np);
    jobs.resize((size_t)np);
    for (int64_t k = 0; k < np; ++k) {
        const csr_export_parent &r = pa[k];
        if (r.chain < 0 || r.chain >= (int)len.size()) return fail("parent %lld: chain index out of range", (long long)k);
        if (taken && !(*taken)[(size_t)r.chain]) return fail("parent %lld: chain %d is not part of this call", (long long)k, r.chain);
        if (r.start < 0 || r.end < r.start || r.end >= len[(size_t)r.chain])
            return fail("parent %lld: bins [%lld, %lld] are outside chain %d", (long long)k, (long long)r.start, (long long)r.end, r.chain);
        if (k > 0 && (pa[k - 1].chain > r.chain || (pa[k - 1].chain == r.chain && pa[k - 1].end >= r.start)))
            return fail("parent %lld: parents must be disjoint and ascending by (chain, start)", (long long)k);
        BroadJob &jb = jobs[(size_t)k];
        jb.off = off[(size_t)r.chain] + r.start;
        jb.n = r.end - r.start + 1;
        jb.start = r.start;
        jb.chain = r.chain;
        jb.reserved = 0;
    }
    return 0;
}

extern "C" int csr_broad_gap_sums(int64_t n, const double *scores, double selection_penalty, double dip_fraction, int64_t n_gaps,
                                  const int64_t *gap_start, const int64_t *gap_len, double *sums) {
    DEFAULT_CTX_GUARD;
    if (n < 0 || (n > 0 && !scores) || n_gaps < 0 || (n_gaps > 0 && (!gap_start || !gap_len || !sums))) return fail("null or negative argument");
    if (n > CLEANUP_MAX_BINS) return fail("too many bins: %lld (limit 2^31 - 2)", (long long)n);
    if (n_gaps >= (int64_t)1 << 30) return fail("too many gaps: %lld", (long long)n_gaps);
    bool any = false;
    for (int64_t g = 0; g < n_gaps; ++g) {
        if (gap_len[g] < 0 || gap_start[g] < 0 || gap_start[g] > n || gap_len[g] > n - gap_start[g])
            return fail("gap %lld: bins [%lld, %lld) are outside the scores", (long long)g, (long long)gap_start[g],
                        (long long)(gap_start[g] + gap_len[g]));
        any = any || gap_len[g] > 0;
    }
    if (!any) {     // (no bin between any two runs: nothing to sum)
        for (int64_t g = 0; g < n_gaps; ++g) sums[g] = 0.0;
        return 0;
    }
    csr_ctx *c = nullptr;
    CHECK(ctx_or_default(c));
    csr_ctx::BroadWs &ws = c->broadWs;
    const size_t ng = (size_t)n_gaps, bytes = 8 * (size_t)n;
    CHECK(ws.arena.reserve(bytes + 64));
    CHECK(ws.jobs.reserve(16 * ng + 64));
    CHECK(ws.rec.reserve(8 * ng + 64));
    HIPOK(hipMemcpyAsync(ws.arena.ptr, scores, bytes, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemcpyAsync(ws.jobs.ptr, gap_start, 8 * ng, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemcpyAsync((char *)ws.jobs.ptr + 8 * ng, gap_len, 8 * ng, hipMemcpyHostToDevice, c->stream));
    BroadGapArgs a;
    memset(&a, 0, sizeof(a));
    a.scores = (const double *)ws.arena.ptr;
    a.start = (const int64_t *)ws.jobs.ptr;
    a.len = a.start + ng;
    a.penalty = selection_penalty;
    a.fraction = dip_fraction;
    a.sums = (double *)ws.rec.ptr;
    a.nGaps = n_gaps;
    CHECK(launch(c, "broad_gap_sums", "k_broad_gap_sums", k_broad_gap_sums, dim3((unsigned)((ng + 63) / 64)), dim3(64), 0, c->stream, a));
    HIPOK(hipMemcpyAsync(sums, ws.rec.ptr, 8 * ng, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    return 0;
}

// the launch both forms share: tables up, one wavefront per parent, records down.  mask: zeroed by the caller where parents may lie
static int broad_rows_run(csr_ctx *c, const std::vector<BroadJob> &jobs, const std::vector<BroadChain> &ch, const double *scores,
                          const ExportTrack &sig, const ExportTrack &unc, int64_t total, unsigned char *mask, csr_broad_parent *records) {
    csr_ctx::BroadWs &ws = c->broadWs;
    const size_t nj = jobs.size(), nc = ch.size();
    auto pad = [](size_t b) { return (b + 255) / 256 * 256; };
    const size_t oCh = pad(nj * sizeof(BroadJob)), tabBytes = oCh + pad(nc * sizeof(BroadChain));
    CHECK(ws.work.reserve(8 * (size_t)total + 64));
    CHECK(ws.jobs.reserve(tabBytes));
    CHECK(ws.rec.reserve(sizeof(csr_broad_parent) * nj));
    char *tab = (char *)ws.jobs.ptr;
    HIPOK(hipMemcpyAsync(tab, jobs.data(), nj * sizeof(BroadJob), hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemcpyAsync(tab + oCh, ch.data(), nc * sizeof(BroadChain), hipMemcpyHostToDevice, c->stream));
    BroadArgs a;
    memset(&a, 0, sizeof(a));
    a.jobs = (const BroadJob *)tab;
    a.cfg = (const BroadChain *)(tab + oCh);
    a.scores = scores;
    a.sig = sig;
    a.unc = unc;
    a.work = (double *)ws.work.ptr;
    a.mask = mask;
    a.rec = (csr_broad_parent *)ws.rec.ptr;
    a.nParents = (int64_t)nj;
    CHECK(launch(c, "broad_parents", "k_broad_parents", k_broad_parents, dim3((unsigned)nj), dim3(64), 0, c->stream, a));
    HIPOK(hipMemcpyAsync(records, ws.rec.ptr, sizeof(csr_broad_parent) * nj, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    return 0;
}

// host arrays (default context).  arena: scores | state | uncertainty
extern "C" int csr_broad_rows(int32_t n_chains, const int64_t *chain_len, const double *state, const double *scores,
                              const double *uncertainty, const csr_broad_cfg *cfg, int64_t n_parents, const csr_export_parent *parents,
                              unsigned char *parent_mask, csr_broad_parent *records) {
    DEFAULT_CTX_GUARD;
    if (n_chains <= 0 || !chain_len || !state || !scores || !cfg || (n_parents > 0 && !records)) return fail("null or empty argument");
    std::vector<int64_t> off((size_t)n_chains), len(chain_len, chain_len + n_chains);
    int64_t total = 0;
    for (int i = 0; i < n_chains; ++i) {
        if (chain_len[i] < 0) return fail("chain %d: negative length", i);
        off[(size_t)i] = total;
        total += chain_len[i];
    }
    if (total > CLEANUP_MAX_BINS) return fail("too many bins: %lld (limit 2^31 - 2)", (long long)total);
    std::vector<BroadJob> jobs;
    CHECK(broad_jobs(off, len, nullptr, n_parents, parents, jobs));
    for (int i = 0; i < n_chains; ++i) CHECK(broad_check_cfg(cfg[i]));
    if (jobs.empty()) {
        if (parent_mask && total > 0) memset(parent_mask, 0, (size_t)total);
        return 0;
    }
    csr_ctx *c = nullptr;
    CHECK(ctx_or_default(c));
    csr_ctx::BroadWs &ws = c->broadWs;
    const size_t bytes = 8 * (size_t)total, nc = (size_t)n_chains;
    CHECK(ws.arena.reserve(3 * bytes + 64));
    CHECK(ws.mask.reserve((size_t)total + 64));
    std::vector<BroadChain> ch(nc);
    for (size_t i = 0; i < nc; ++i) {
        ch[i].multiplier = cfg[i].multiplier;
        ch[i].filter = cfg[i].filter != 0 && uncertainty != nullptr;
        ch[i].reserved = 0;
    }
    char *base = (char *)ws.arena.ptr;
    HIPOK(hipMemcpyAsync(base, scores, bytes, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemcpyAsync(base + bytes, state, bytes, hipMemcpyHostToDevice, c->stream));
    if (uncertainty) HIPOK(hipMemcpyAsync(base + 2 * bytes, uncertainty, bytes, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemsetAsync(ws.mask.ptr, 0, (size_t)total, c->stream));
    ExportTrack sig, unc;
    memset(&sig, 0, sizeof(sig));
    memset(&unc, 0, sizeof(unc));
    sig.d = (const double *)(base + bytes);
    if (uncertainty) unc.d = (const double *)(base + 2 * bytes);
    CHECK(broad_rows_run(c, jobs, ch, (const double *)base, sig, unc, total, (unsigned char *)ws.mask.ptr, records));
    if (parent_mask) {
        HIPOK(hipMemcpyAsync(parent_mask, ws.mask.ptr, (size_t)total, hipMemcpyDeviceToHost, c->stream));
        HIPOK(hipStreamSynchronize(c->stream));
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// batch context: the resident score tracks, masks and smoothed fit are read; the weak mask and the parent mask are written
// ---------------------------------------------------------------------------------------------------------------
extern "C" int csr_batch_rocco_weak(csr_ctx *c, const csr_rocco_cfg *cfg, const unsigned char *chain_mask, csr_rocco_out *out) {
    CHECK(need(c));
    if (!cfg || !out) return fail("null argument");
    std::vector<int> idx;
    const int missing = select_chains(c, chain_mask, c->scores, idx, NO_SCORES);
    std::vector<RoccoChainIn> chains;
    for (int i : idx) {
        CHECK(rocco_check_cfg(cfg[i], i, true));
        chains.push_back(RoccoChainIn{c->chains[i].off, c->chains[i].n, cfg[i].gamma, nullptr, cfg[i], &out[i]});
    }
    CHECK(missing);
    CHECK(rocco_buffers(c));
    CHECK(c->weak.ensure(c));
    RoccoDev dv{c->scores.d, nullptr, c->weak.d, c->rocco.bt};
    for (int i : idx) c->weak.set(i, false);
    CHECK(rocco_run(c, dv, chains));
    for (int i : idx) c->weak.set(i, true);
    return 0;
}

extern "C" int csr_batch_rocco_weak_upload(csr_ctx *c, int32_t chain, const unsigned char *solution) {
    CHECK(need_chain(c, chain, solution));
    if (!c->scores.has(chain)) return fail("chain %d has no scores", chain);
    for (int64_t i = 0; i < c->chains[chain].n; ++i)
        if (solution[i] > 1) return fail("a selection mask holds 0 and 1 only");
    return c->weak.upload(c, chain, solution);
}
extern "C" int csr_batch_rocco_weak_download(csr_ctx *c, int32_t chain, uint8_t *solution) {
    CHECK(need_chain(c, chain, solution));
    return c->weak.download(c, chain, solution);
}
extern "C" int csr_batch_broad_parent_download(csr_ctx *c, int32_t chain, uint8_t *mask) {
    CHECK(need_chain(c, chain, mask));
    return c->broadParent.download(c, chain, mask);
}

// one chain's support runs -> its kept records on the host (appended).  envelope: weak | strong as the predicate
static int broad_runs_chain(csr_ctx *c, int chain, const csr_broad_run_cfg &g, const int64_t *dBreaks, int64_t nBreaks, bool envelope,
                            int64_t *support, std::vector<csr_broad_run> &kept) {
    csr_ctx::BroadWs &ws = c->broadWs;
    const ChainInfo &ci = c->chains[chain];
    *support = 0;
    if (ci.n <= 0) return 0;
    const int64_t nb = (ci.n + 1023) / 1024;
    BroadRunArgs a;
    memset(&a, 0, sizeof(a));
    a.scores = c->scores.at(c, chain);
    a.weak = c->weak.at(c, chain);
    a.strong = c->sol.at(c, chain);
    a.breaks = dBreaks;
    a.nBreaks = nBreaks;
    a.n = ci.n;
    a.threshold = g.threshold;
    a.penalty = g.selection_penalty;
    a.fraction = g.dip_fraction;
    a.maxGapBins = g.max_gap_bins;
    a.envelope = envelope ? 1 : 0;
    a.chain = chain;
    CHECK(ws.mask.reserve(8 * (size_t)(nb + 1) + 64));      // (the block sums of the bins: the parent mask of a batch is resident)
    a.blockSum = (unsigned long long *)ws.mask.ptr;
    Scope sc(c, "broad_runs");
    CHECK(launch(c, nullptr, "k_broad_run_count", k_broad_run_count, dim3((unsigned)nb), dim3(1024), 0, c->stream, a));
    CHECK(launch(c, nullptr, "k_broad_scan", k_broad_scan, dim3(1), dim3(1024), 0, c->stream, a.blockSum, nb));
    unsigned long long tot = 0;
    HIPOK(hipMemcpyAsync(&tot, a.blockSum + nb, 8, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    const int64_t ns = (int64_t)(tot & 0xffffffffull), ne = (int64_t)(tot >> 32);
    if (ns != ne) return fail("support runs: %lld starts but %lld ends (chain %d)", (long long)ns, (long long)ne, chain);
    *support = ns;
    if (ns == 0) return 0;
    // runs: starts | ends | the block sums of the runs | touch flags; the records of the kept ones
    const int64_t rb = (ns + 1023) / 1024;
    auto pad = [](size_t b) { return (b + 255) / 256 * 256; };
    const size_t oE = pad(8 * (size_t)ns), oK = 2 * oE, oT = oK + pad(8 * (size_t)(rb + 1)), bytes = oT + pad((size_t)ns);
    CHECK(ws.runs.reserve(bytes));
    CHECK(ws.rec.reserve(sizeof(csr_broad_run) * (size_t)ns));
    char *base = (char *)ws.runs.ptr;
    a.starts = (int64_t *)base;
    a.ends = (int64_t *)(base + oE);
    a.keepSum = (unsigned long long *)(base + oK);
    a.touch = (unsigned char *)(base + oT);
    a.rec = (csr_broad_run *)ws.rec.ptr;
    a.nRuns = ns;
    CHECK(launch(c, nullptr, "k_broad_run_write", k_broad_run_write, dim3((unsigned)nb), dim3(1024), 0, c->stream, a));
    if (envelope) HIPOK(hipMemsetAsync(a.touch, 1, (size_t)ns, c->stream));      // (a run of the envelope touches it)
    else CHECK(launch(c, nullptr, "k_broad_run_touch", k_broad_run_touch, dim3((unsigned)ns), dim3(64), 0, c->stream, a));
    CHECK(launch(c, nullptr, "k_broad_keep_count", k_broad_keep_count, dim3((unsigned)rb), dim3(1024), 0, c->stream, a));
    CHECK(launch(c, nullptr, "k_broad_scan", k_broad_scan, dim3(1), dim3(1024), 0, c->stream, a.keepSum, rb));
    CHECK(launch(c, nullptr, "k_broad_keep_write", k_broad_keep_write, dim3((unsigned)rb), dim3(1024), 0, c->stream, a));
    CHECK(launch(c, nullptr, "k_broad_run_gaps", k_broad_run_gaps, dim3((unsigned)((ns + 63) / 64)), dim3(64), 0, c->stream, a, rb));
    unsigned long long nk = 0;
    HIPOK(hipMemcpyAsync(&nk, a.keepSum + rb, 8, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    if ((int64_t)nk > ns) return fail("support runs: %llu kept of %lld (chain %d)", nk, (long long)ns, chain);
    if (nk > 0) {
        const size_t at = kept.size();
        kept.resize(at + (size_t)nk);
        HIPOK(hipMemcpyAsync(kept.data() + at, a.rec, sizeof(csr_broad_run) * (size_t)nk, hipMemcpyDeviceToHost, c->stream));
        HIPOK(hipStreamSynchronize(c->stream));
    }
    return 0;
}

extern "C" int csr_batch_broad_runs(csr_ctx *c, const csr_broad_run_cfg *cfg, const unsigned char *chain_mask, const int64_t *n_breaks,
                                    const int64_t *breaks, csr_broad_run_counts *counts, int64_t *n_records) {
    CHECK(need(c));
    if (!cfg || !n_breaks || !counts || !n_records) return fail("null argument");
    std::vector<int> idx;
    CHECK(select_chains(c, chain_mask, c->scores, idx, NO_SCORES));
    const int nc = (int)c->chains.size();
    std::vector<int64_t> boff((size_t)nc + 1, 0);
    for (int i = 0; i < nc; ++i) {
        if (n_breaks[i] < 0) return fail("chain %d: negative break count", i);
        boff[(size_t)i + 1] = boff[(size_t)i] + n_breaks[i];
    }
    if (boff[(size_t)nc] > 0 && !breaks) return fail("null break list");
    for (int i : idx) {
        if (!c->sol.has(i)) return fail("chain %d has no ROCCO solution", i);
        if (!c->weak.has(i)) return fail("chain %d has no weak ROCCO solution", i);
        if (std::isnan(cfg[i].threshold)) return fail("chain %d: the support threshold is not a number", i);
        if (!std::isfinite(cfg[i].selection_penalty) || !std::isfinite(cfg[i].dip_fraction)) return fail("chain %d: non-finite bridging parameter", i);
        for (int64_t k = boff[(size_t)i]; k < boff[(size_t)i + 1]; ++k)
            if (breaks[k] < 0 || breaks[k] >= c->chains[i].n || (k > boff[(size_t)i] && breaks[k - 1] >= breaks[k]))
                return fail("chain %d: breaks must ascend strictly inside the chain", i);
    }
    csr_ctx::BroadWs &ws = c->broadWs;
    ws.kept.clear();
    *n_records = 0;
    CHECK(ws.jobs.reserve(8 * (size_t)boff[(size_t)nc] + 64));
    if (boff[(size_t)nc] > 0) HIPOK(hipMemcpyAsync(ws.jobs.ptr, breaks, 8 * (size_t)boff[(size_t)nc], hipMemcpyHostToDevice, c->stream));
    for (int i : idx) {
        csr_broad_run_counts &q = counts[i];
        q.support_runs = q.touching_runs = 0;
        q.fallback = q.reserved = 0;
        const int64_t *dB = (const int64_t *)ws.jobs.ptr + boff[(size_t)i];
        const size_t before = ws.kept.size();
        CHECK(broad_runs_chain(c, i, cfg[i], dB, n_breaks[i], false, &q.support_runs, ws.kept));
        if (ws.kept.size() == before) {     // no support run touches the envelope: the envelope's own runs
            int64_t runs = 0;
            q.fallback = 1;
            CHECK(broad_runs_chain(c, i, cfg[i], dB, n_breaks[i], true, &runs, ws.kept));
        }
        q.touching_runs = (int64_t)(ws.kept.size() - before);
    }
    *n_records = (int64_t)ws.kept.size();
    return 0;
}

extern "C" int csr_batch_broad_runs_fetch(csr_ctx *c, int64_t capacity, csr_broad_run *records) {
    CHECK(need(c));
    if (capacity < 0 || (capacity > 0 && !records)) return fail("bad capacity / output buffer");
    const size_t take = std::min((size_t)capacity, c->broadWs.kept.size());
    if (take > 0) memcpy(records, c->broadWs.kept.data(), sizeof(csr_broad_run) * take);
    return 0;
}

extern "C" int csr_batch_broad_rows(csr_ctx *c, const csr_broad_cfg *cfg, const unsigned char *chain_mask, int64_t n_parents,
                                    const csr_export_parent *parents, csr_broad_parent *records) {
    CHECK(need(c));
    if (!cfg || (n_parents > 0 && !records)) return fail("null argument");
    CHECK(settle(c));
    NestedLay L;
    CHECK(nested_batch_layout(c, chain_mask, false, L));
    if (L.total > CLEANUP_MAX_BINS) return fail("too many bins: %lld (limit 2^31 - 2)", (long long)L.total);
    std::vector<BroadJob> jobs;
    std::vector<char> taken(L.taken.begin(), L.taken.end());
    CHECK(broad_jobs(L.off, L.len, &taken, n_parents, parents, jobs));
    const size_t nc = L.len.size();
    bool filter = false;
    for (size_t i = 0; i < nc; ++i)
        if (L.taken[i]) {
            CHECK(broad_check_cfg(cfg[i]));
            filter = filter || cfg[i].filter != 0;
        }
    if (!jobs.empty() && !c->haveBwd) return fail("no smoothed results to make broad rows from");
    CHECK(c->broadParent.ensure(c));
    for (size_t i = 0; i < nc; ++i)
        if (L.taken[i] && L.len[i] > 0) HIPOK(hipMemsetAsync(c->broadParent.at(c, (int)i), 0, (size_t)L.len[i], c->stream));
    if (!jobs.empty()) {
        // the conversion csr_batch_export(CSR_EXPORT_SMOOTH) makes, a no-op when the reference-layout copies are current
        CHECK(export_impl(c, CSR_EXPORT_SMOOTH));
        std::vector<BroadChain> ch(nc);
        for (size_t i = 0; i < nc; ++i) {
            ch[i].multiplier = L.taken[i] ? cfg[i].multiplier : 0.0;
            ch[i].filter = L.taken[i] && cfg[i].filter != 0;
            ch[i].reserved = 0;
        }
        ExportTrack sig, unc;
        memset(&sig, 0, sizeof(sig));
        memset(&unc, 0, sizeof(unc));
        const int d = c->mdl.state_dim;
        CHECK(batch_export_signal(c, L.taken, sig));
        if (filter) {
            unc.f = c->nat[CSR_ARR_PS];
            unc.stride = (int64_t)d * d;
            unc.root = 1;
        }
        CHECK(broad_rows_run(c, jobs, ch, L.scores, sig, unc, L.total, c->broadParent.d, records));
    } else {
        HIPOK(hipStreamSynchronize(c->stream));
    }
    for (size_t i = 0; i < nc; ++i)
        if (L.taken[i]) c->broadParent.set((int)i, true);
    return 0;
}
