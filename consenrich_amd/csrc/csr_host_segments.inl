// csr_host_segments.inl -- part of csr_lib.hip (one translation unit; included in this order): multiscale candidate segments
// (pyx:9460-9669 `cMultiscaleCandidateSegmentStats`) with the kernels of csr_segments.h.  ONE core (seg_run) serves three
// entries: a host vector, the resident score tracks of a batch, and a group of draws of the DWB panel.  A run leaves its result
// in the context: the row counts and counters come back at once (phase 1), views whose chosen set the values do not determine
// are handed to the caller one by one (csr_segments_flagged*), and csr_segments_fetch copies the rows (phase 2).

// the device work space of the segment runs (the rows of the last run stay: they are host memory)
static void seg_release(csr_ctx *c) {
    csr_ctx::Seg &g = c->seg;
    for (DevBuf *b : {&g.chainBuf, &g.prefixBuf, &g.excessBuf, &g.exPrefixBuf, &g.cntBuf, &g.runBuf, &g.keepBuf, &g.statBuf, &g.metaBuf,
                      &g.baseBuf, &g.outBuf, &g.xBuf})
        b->release();
}

struct SegSpec {
    int nc;
    const int32_t *nS;          // per chain; scales one chain after the other
    const int64_t *scales;
    const int32_t *nV;          // per chain; thresholds / null scales one chain after the other
    const double *thr, *ns;
    int minRun, gap, cap;
};

static int seg_check_spec(const SegSpec &sp) {
    if (!sp.nS || !sp.nV) return fail("null argument");
    int64_t s = 0, v = 0;
    for (int i = 0; i < sp.nc; ++i) {
        if (sp.nS[i] < 0 || sp.nS[i] > SEG_MAX_SCALES) return fail("chain %d: the number of scales must be in 0..%d", i, SEG_MAX_SCALES);
        if (sp.nV[i] < 0 || sp.nV[i] > SEG_MAX_VIEWS) return fail("chain %d: the number of views must be in 0..%d", i, SEG_MAX_VIEWS);
        s += sp.nS[i];
        v += sp.nV[i];
    }
    if ((s && !sp.scales) || (v && (!sp.thr || !sp.ns))) return fail("null argument");
    return 0;
}

static void seg_empty(csr_ctx::Seg &g, int nTracks, int cap) {
    g.have = true;
    g.cap = cap;
    g.rowsPerTrack.assign((size_t)nTracks, 0);
    g.counters.assign(3 * (size_t)nTracks, 0);
    for (auto *v : {&g.oStart, &g.oEnd, &g.oScale, &g.oView}) v->clear();
    for (auto *v : {&g.oScore, &g.oInteg, &g.oMean, &g.oMax}) v->clear();
    g.flagged.clear();
}

// rows: nRows rows of rowLen values on the device; chain i = bins [off[i], off[i] + len[i]) of every row.  Track = chain * nRows + row.
static int seg_run(csr_ctx *c, const double *dRows, int64_t rowLen, int nRows, const int64_t *off, const int64_t *len,
                   const SegSpec &sp) {
    csr_ctx::Seg &g = c->seg;
    g.have = false;
    const int nc = sp.nc;
    const int minRun = sp.minRun > 1 ? sp.minRun : 1, gap = sp.gap > 0 ? sp.gap : 0, cap = sp.cap > 0 ? sp.cap : 0;
    std::vector<SegChain> chains((size_t)nc);
    int S = 0, V = 0;
    int64_t pLen = 0, rLen = 0, longest = 0, so = 0, vo = 0;
    for (int i = 0; i < nc; ++i) {
        SegChain &ch = chains[i];
        memset(&ch, 0, sizeof(ch));
        if (len[i] <= 0 || len[i] >= ((int64_t)1 << 31) - 64) return fail("chain %d: length out of range", i);
        ch.off = off[i];
        ch.n = len[i];
        ch.pOff = pLen;
        ch.rOff = rLen;
        pLen += (len[i] + 1 + 63) / 64 * 64;
        rLen += ((len[i] + 1) / 2 + 63) / 64 * 64;
        ch.nS = sp.nS[i];
        ch.nV = sp.nV[i];
        for (int s = 0; s < ch.nS; ++s) ch.w[s] = std::min<int64_t>(std::max<int64_t>(sp.scales[so + s], 1), len[i]);
        for (int v = 0; v < ch.nV; ++v) {
            ch.thr[v] = sp.thr[vo + v];
            const double ns = sp.ns[vo + v];
            ch.ns[v] = ns < DBL_MIN ? DBL_MIN : ns;     // (pyx:9578: a NaN stays)
        }
        so += ch.nS;
        vo += ch.nV;
        S = std::max(S, ch.nS);
        V = std::max(V, ch.nV);
        longest = std::max(longest, len[i]);
    }
    const int nTracks = nc * nRows;
    if (S == 0 || V == 0) {
        seg_empty(g, nTracks, cap);
        return 0;
    }
    const int64_t J = (int64_t)nRows * S * V;
    if (J > 65535) return fail("%lld (row, scale, view) jobs per chain exceed the limit of 65535", (long long)J);
    const size_t nJobs = (size_t)nc * (size_t)J;
    CHECK(g.chainBuf.reserve(sizeof(SegChain) * (size_t)nc));
    CHECK(g.prefixBuf.reserve(8 * (size_t)nRows * (size_t)pLen));
    CHECK(g.excessBuf.reserve(8 * (size_t)nRows * V * (size_t)rowLen));
    CHECK(g.exPrefixBuf.reserve(8 * (size_t)nRows * V * (size_t)pLen));
    CHECK(g.cntBuf.reserve(4 * (size_t)J * (size_t)pLen));
    CHECK(g.runBuf.reserve(8 * (size_t)J * (size_t)rLen));
    CHECK(g.keepBuf.reserve((size_t)J * (size_t)rLen));
    CHECK(g.statBuf.reserve(32 * (size_t)J * (size_t)rLen));
    const size_t oMeta = (4 * nJobs + 255) / 256 * 256;
    CHECK(g.metaBuf.reserve(oMeta + sizeof(SegMeta) * nJobs));
    CHECK(g.baseBuf.reserve(8 * nJobs));
    SegArgs a;
    memset(&a, 0, sizeof(a));
    a.chains = (const SegChain *)g.chainBuf.ptr;
    a.rows = dRows;
    a.rowLen = rowLen;
    a.nRows = nRows;
    a.S = S;
    a.V = V;
    a.pLen = pLen;
    a.rLen = rLen;
    a.prefix = (double *)g.prefixBuf.ptr;
    a.excess = (double *)g.excessBuf.ptr;
    a.exPrefix = (double *)g.exPrefixBuf.ptr;
    a.cnt = (int *)g.cntBuf.ptr;
    a.rStart = (int *)g.runBuf.ptr;
    a.rEnd = a.rStart + (size_t)J * (size_t)rLen;
    a.keep = (unsigned char *)g.keepBuf.ptr;
    a.score = (double *)g.statBuf.ptr;
    a.integ = a.score + (size_t)J * (size_t)rLen;
    a.mean = a.integ + (size_t)J * (size_t)rLen;
    a.mx = a.mean + (size_t)J * (size_t)rLen;
    a.runCount = (int *)g.metaBuf.ptr;
    a.meta = (SegMeta *)((char *)g.metaBuf.ptr + oMeta);
    a.minRun = minRun;
    a.gap = gap;
    a.cap = cap;
    a.jobBase = (const int64_t *)g.baseBuf.ptr;
    HIPOK(hipMemcpyAsync(g.chainBuf.ptr, chains.data(), sizeof(SegChain) * (size_t)nc, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemsetAsync(g.metaBuf.ptr, 0, oMeta + sizeof(SegMeta) * nJobs, c->stream));
    const dim3 jobs((unsigned)J, (unsigned)nc);
    {
        SegWalkArgs w{a.chains, dRows, rowLen, a.prefix, pLen, nRows, 1};
        CHECK(launch(c, "seg_walk_track", "k_seg_walk", k_seg_walk, dim3((unsigned)((nRows + SEG_WR - 1) / SEG_WR), (unsigned)nc), dim3(64), 0,
                     c->stream, w));
    }
    CHECK(launch(c, "seg_excess", "k_seg_excess", k_seg_excess, dim3((unsigned)((longest + 255) / 256), (unsigned)(nRows * V),
                 (unsigned)nc), dim3(256), 0, c->stream, a));
    {
        SegWalkArgs w{a.chains, a.excess, rowLen, a.exPrefix, pLen, nRows * V, V};
        CHECK(launch(c, "seg_walk_excess", "k_seg_walk", k_seg_walk, dim3((unsigned)((nRows * V + SEG_WR - 1) / SEG_WR), (unsigned)nc), dim3(64),
                     0, c->stream, w));
    }
    CHECK(launch(c, "seg_count", "k_seg_count", k_seg_count, jobs, dim3(256), 0, c->stream, a));
    CHECK(launch(c, "seg_runs", "k_seg_runs", k_seg_runs, jobs, dim3(256), 0, c->stream, a));
    CHECK(launch(c, "seg_stats", "k_seg_stats", k_seg_stats, dim3(SEG_STAT_BLOCKS, (unsigned)J, (unsigned)nc), dim3(256), 0, c->stream, a));
    CHECK(launch(c, "seg_select", "k_seg_select", k_seg_select, jobs, dim3(256), 0, c->stream, a));
    std::vector<SegMeta> meta(nJobs);
    {
        Scope sc(c, "seg_download");
        HIPOK(hipMemcpyAsync(meta.data(), a.meta, sizeof(SegMeta) * nJobs, hipMemcpyDeviceToHost, c->stream));
    }
    HIPOK(hipStreamSynchronize(c->stream));

    // output rows: track, then scale, then view, then start -- the order of the jobs
    seg_empty(g, nTracks, cap);
    g.have = false;             // (until the rows are here)
    std::vector<int64_t> base(nJobs, 0);
    int64_t total = 0;
    for (int i = 0; i < nc; ++i)
        for (int r = 0; r < nRows; ++r)
            for (int s = 0; s < chains[i].nS; ++s)
                for (int v = 0; v < chains[i].nV; ++v) {
                    const size_t job = (size_t)i * J + ((size_t)r * S + s) * V + v;
                    const SegMeta &m = meta[job];
                    const int t = i * nRows + r;
                    const int64_t rows = m.flagged ? cap : m.emit;
                    base[job] = total;
                    g.rowsPerTrack[t] += rows;
                    g.counters[3 * t + 0] += m.kept;
                    g.counters[3 * t + 1] += m.capped;
                    if (m.capped) g.counters[3 * t + 2] += m.kept - cap;
                    g.oScale.insert(g.oScale.end(), (size_t)rows, chains[i].w[s]);
                    g.oView.insert(g.oView.end(), (size_t)rows, (int64_t)v);
                    if (m.flagged) {
                        csr_ctx::Seg::Flagged f;
                        f.track = t;
                        f.scaleIndex = s;
                        f.view = v;
                        f.base = total;
                        f.resolved = false;
                        // the view's candidates, fetched for this view alone
                        const size_t nr = (size_t)m.nRuns;
                        const size_t ro = (((size_t)r * S + s) * V + v) * (size_t)rLen + (size_t)chains[i].rOff;
                        std::vector<int> rs(nr), re(nr);
                        std::vector<unsigned char> keep(nr);
                        std::vector<double> st(4 * nr);
                        Scope sc(c, "seg_flagged_download");
                        HIPOK(hipMemcpyAsync(rs.data(), a.rStart + ro, 4 * nr, hipMemcpyDeviceToHost, c->stream));
                        HIPOK(hipMemcpyAsync(re.data(), a.rEnd + ro, 4 * nr, hipMemcpyDeviceToHost, c->stream));
                        HIPOK(hipMemcpyAsync(keep.data(), a.keep + ro, nr, hipMemcpyDeviceToHost, c->stream));
                        const double *src[4] = {a.score + ro, a.integ + ro, a.mean + ro, a.mx + ro};
                        for (int k = 0; k < 4; ++k)
                            HIPOK(hipMemcpyAsync(st.data() + k * nr, src[k], 8 * nr, hipMemcpyDeviceToHost, c->stream));
                        HIPOK(hipStreamSynchronize(c->stream));
                        for (size_t k = 0; k < nr; ++k)
                            if (keep[k]) {
                                f.start.push_back(rs[k]);
                                f.end.push_back(re[k]);
                                f.score.push_back(st[k]);
                                f.integ.push_back(st[nr + k]);
                                f.mean.push_back(st[2 * nr + k]);
                                f.mx.push_back(st[3 * nr + k]);
                            }
                        if ((int64_t)f.start.size() != m.kept) return fail("flagged view: candidate count mismatch");
                        g.flagged.push_back(std::move(f));
                    }
                    total += rows;
                }
    const size_t n = (size_t)total;
    g.oStart.assign(n, 0);
    g.oEnd.assign(n, 0);
    g.oScore.assign(n, 0.0);
    g.oInteg.assign(n, 0.0);
    g.oMean.assign(n, 0.0);
    g.oMax.assign(n, 0.0);
    if (n) {
        const size_t slot = (8 * n + 255) / 256 * 256;
        CHECK(g.outBuf.reserve(6 * slot));
        char *ob = (char *)g.outBuf.ptr;
        a.oStart = (int64_t *)ob;
        a.oEnd = (int64_t *)(ob + slot);
        a.oScore = (double *)(ob + 2 * slot);
        a.oInteg = (double *)(ob + 3 * slot);
        a.oMean = (double *)(ob + 4 * slot);
        a.oMax = (double *)(ob + 5 * slot);
        HIPOK(hipMemcpyAsync(g.baseBuf.ptr, base.data(), 8 * nJobs, hipMemcpyHostToDevice, c->stream));
        CHECK(launch(c, "seg_emit", "k_seg_emit", k_seg_emit, jobs, dim3(256), 0, c->stream, a));
        if (!g.deviceOnly) {
            Scope sc(c, "seg_download");
            void *dst[6] = {g.oStart.data(), g.oEnd.data(), g.oScore.data(), g.oInteg.data(), g.oMean.data(), g.oMax.data()};
            for (int k = 0; k < 6; ++k) HIPOK(hipMemcpyAsync(dst[k], ob + k * slot, 8 * n, hipMemcpyDeviceToHost, c->stream));
        }
        HIPOK(hipStreamSynchronize(c->stream));
    }
    g.have = true;
    return 0;
}

static void seg_report(const csr_ctx::Seg &g, int64_t *rows, int64_t *counters, int32_t *n_flagged) {
    std::copy(g.rowsPerTrack.begin(), g.rowsPerTrack.end(), rows);
    std::copy(g.counters.begin(), g.counters.end(), counters);
    *n_flagged = (int32_t)g.flagged.size();
}

// ---------------------------------------------------------------------------------------------------------------
// phase 1 on a host vector / the resident scores of a batch / a group of draws of the DWB panel
// ---------------------------------------------------------------------------------------------------------------
extern "C" int csr_segments_run(csr_ctx *c, const double *scores, int64_t n, int32_t n_scales, const int64_t *scales,
                                int32_t n_thresholds, const double *thresholds, int32_t n_null_scales, const double *null_scales,
                                int32_t min_run_bins, int32_t max_gap_bins, int32_t max_segments_per_view, int64_t *n_rows,
                                int64_t *counters, int32_t *n_flagged) {
    DEFAULT_CTX_GUARD;
    if (n_thresholds != n_null_scales) return value_error("thresholds and nullScales must have the same length");
    if (!n_rows || !counters || !n_flagged) return fail("null argument");
    CHECK(ctx_or_default(c));
    csr_ctx::Seg &g = c->seg;
    g.have = false;
    if (n <= 0 || n_scales <= 0 || n_thresholds <= 0) {
        seg_empty(g, 1, std::max(max_segments_per_view, 0));
        seg_report(g, n_rows, counters, n_flagged);
        return 0;
    }
    if (!scores) return fail("null argument");
    SegSpec sp{1, &n_scales, scales, &n_thresholds, thresholds, null_scales, min_run_bins, max_gap_bins, max_segments_per_view};
    CHECK(seg_check_spec(sp));
    const double *dx = nullptr;
    CHECK(stage_vector(c, g.xBuf, scores, n, &dx));
    const int64_t off = 0;
    CHECK(seg_run(c, dx, (n + 63) / 64 * 64, 1, &off, &n, sp));
    seg_report(g, n_rows, counters, n_flagged);
    return 0;
}

// reads the chains' resident score tracks; changes nothing resident.  rows[chain], counters[chain][3]
extern "C" int csr_batch_segments_run(csr_ctx *c, const int32_t *n_scales, const int64_t *scales, const int32_t *n_views,
                                      const double *thresholds, const double *null_scales, int32_t min_run_bins,
                                      int32_t max_gap_bins, int32_t max_segments_per_view, int64_t *rows, int64_t *counters,
                                      int32_t *n_flagged) {
    CHECK(need(c));
    if (!rows || !counters || !n_flagged) return fail("null argument");
    const int nc = (int)c->chains.size();
    SegSpec sp{nc, n_scales, scales, n_views, thresholds, null_scales, min_run_bins, max_gap_bins, max_segments_per_view};
    CHECK(seg_check_spec(sp));
    std::vector<int> idx;
    CHECK(select_chains(c, nullptr, c->scores, idx));
    std::vector<int64_t> off((size_t)nc), len((size_t)nc);
    int64_t rowLen = 64;
    for (int i : idx) {
        off[i] = c->chains[i].off;
        len[i] = c->chains[i].n;
        rowLen = std::max(rowLen, (off[i] + len[i] + 63) / 64 * 64);
    }
    CHECK(seg_run(c, c->scores.d, rowLen, 1, off.data(), len.data(), sp));
    seg_report(c->seg, rows, counters, n_flagged);
    return 0;
}

// draws first_draw .. first_draw + n_draws - 1 of every chain of the panel (n_draws <= the panel's draws per group): the rows are
// made as in the other two phases, then read.  rows[chain][draw], counters[chain][draw][3]
extern "C" int csr_dwb_panel_segments(csr_ctx *c, int32_t first_draw, int32_t n_draws, const int32_t *n_scales, const int64_t *scales,
                                      const int32_t *n_views, const double *thresholds, const double *null_scales,
                                      int32_t min_run_bins, int32_t max_gap_bins, int32_t max_segments_per_view, int64_t *rows,
                                      int64_t *counters, int32_t *n_flagged) {
    DEFAULT_CTX_GUARD;
    if (!rows || !counters || !n_flagged) return fail("null argument");
    if (max_segments_per_view <= 0) return fail("the panel needs max_segments_per_view > 0");
    CHECK(ctx_or_default(c));
    csr_ctx::Dwb &d = c->dwb;
    if (!d.ready) return fail("no DWB panel: call csr_dwb_panel_begin first");
    if (first_draw < 0 || n_draws <= 0 || n_draws > d.group || (int64_t)first_draw + n_draws > d.nDraws)
        return fail("draws %d .. %d: out of range (the panel has %d draws, %d per group)", (int)first_draw,
                    (int)first_draw + (int)n_draws - 1, d.nDraws, d.group);
    const int nc = (int)d.chains.size();
    SegSpec sp{nc, n_scales, scales, n_views, thresholds, null_scales, min_run_bins, max_gap_bins, max_segments_per_view};
    CHECK(seg_check_spec(sp));
    std::vector<int64_t> off((size_t)nc), len((size_t)nc);
    for (int i = 0; i < nc; ++i) {
        off[i] = d.chains[i].off;
        len[i] = d.chains[i].n;
    }
    CHECK(dwb_make_rows(c, first_draw, n_draws, true, true, true));
    CHECK(seg_run(c, (const double *)d.rowBuf.ptr, d.rowLen, n_draws, off.data(), len.data(), sp));
    seg_report(c->seg, rows, counters, n_flagged);
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// flagged views and phase 2 (the result of the context's last run)
// ---------------------------------------------------------------------------------------------------------------
static int seg_result(csr_ctx *&c, int32_t k, bool indexed) {
    CHECK(ctx_or_default(c));
    if (!c->seg.have) return fail("no segment run on this context");
    if (indexed && (k < 0 || k >= (int)c->seg.flagged.size())) return fail("flagged view index out of range");
    return 0;
}
extern "C" int csr_segments_flagged(csr_ctx *c, int32_t k, int32_t *track, int32_t *scale_index, int32_t *view,
                                    int64_t *n_candidates) {
    DEFAULT_CTX_GUARD;
    CHECK(seg_result(c, k, true));
    if (!track || !scale_index || !view || !n_candidates) return fail("null argument");
    const csr_ctx::Seg::Flagged &f = c->seg.flagged[k];
    *track = f.track;
    *scale_index = f.scaleIndex;
    *view = f.view;
    *n_candidates = (int64_t)f.start.size();
    return 0;
}
extern "C" int csr_segments_flagged_fetch(csr_ctx *c, int32_t k, double *score, int64_t *start) {
    DEFAULT_CTX_GUARD;
    CHECK(seg_result(c, k, true));
    if (!score || !start) return fail("null argument");
    const csr_ctx::Seg::Flagged &f = c->seg.flagged[k];
    std::copy(f.score.begin(), f.score.end(), score);
    std::copy(f.start.begin(), f.start.end(), start);
    return 0;
}
// selected: the view's `cap` chosen candidates (indices into what flagged_fetch returned) in output order
extern "C" int csr_segments_flagged_select(csr_ctx *c, int32_t k, int64_t n_selected, const int64_t *selected) {
    DEFAULT_CTX_GUARD;
    CHECK(seg_result(c, k, true));
    csr_ctx::Seg &g = c->seg;
    csr_ctx::Seg::Flagged &f = g.flagged[k];
    if (!selected || n_selected != g.cap) return fail("a flagged view takes exactly %d selected candidates", g.cap);
    for (int64_t q = 0; q < n_selected; ++q)
        if (selected[q] < 0 || selected[q] >= (int64_t)f.start.size()) return fail("selected candidate out of range");
    for (int64_t q = 0; q < n_selected; ++q) {
        const size_t o = (size_t)(f.base + q), r = (size_t)selected[q];
        g.oStart[o] = f.start[r];
        g.oEnd[o] = f.end[r];
        g.oScore[o] = f.score[r];
        g.oInteg[o] = f.integ[r];
        g.oMean[o] = f.mean[r];
        g.oMax[o] = f.mx[r];
    }
    f.resolved = true;
    return 0;
}
extern "C" int csr_segments_fetch(csr_ctx *c, int64_t *start, int64_t *end, int64_t *scale, int64_t *view, double *score,
                                  double *integrated, double *mean, double *max_excess) {
    DEFAULT_CTX_GUARD;
    CHECK(seg_result(c, 0, false));
    const csr_ctx::Seg &g = c->seg;
    if (g.deviceOnly) return fail("the rows of this run stayed on the device: a replay pool is open (csr_dwb_panel_pool_append takes them)");
    for (const auto &f : g.flagged)
        if (!f.resolved) return fail("a flagged view has not been resolved (csr_segments_flagged_select)");
    if (g.oStart.empty()) return 0;
    if (!start || !end || !scale || !view || !score || !integrated || !mean || !max_excess) return fail("null argument");
    std::copy(g.oStart.begin(), g.oStart.end(), start);
    std::copy(g.oEnd.begin(), g.oEnd.end(), end);
    std::copy(g.oScale.begin(), g.oScale.end(), scale);
    std::copy(g.oView.begin(), g.oView.end(), view);
    std::copy(g.oScore.begin(), g.oScore.end(), score);
    std::copy(g.oInteg.begin(), g.oInteg.end(), integrated);
    std::copy(g.oMean.begin(), g.oMean.end(), mean);
    std::copy(g.oMax.begin(), g.oMax.end(), max_excess);
    return 0;
}
