// csr_host_peakscore.inl -- part of csr_lib.hip (one translation unit; included in this order): the numeric side of the reference's
// DWB peak scoring from the kernels of csr_peakscore.h -- the best score of many segments across threshold views (peaks.py:2295-2356)
// and the empirical p / q values of observed statistics against a pool of replay statistics (peaks.py:2182-2257).  The pool and the
// observed statistics are sorted by the null's keys-only sort (NullEngine, csr_host_null.inl) in work space; every count is one
// bisection.  The strings, the merge of candidates with exported peaks and the quantiles over the draws stay with the caller.

// The segments of one device track: out arrays of n_seg values each (host)
static int peakscore_device(csr_ctx *c, const double *dx, int64_t n, int64_t n_seg, const int64_t *starts, const int64_t *ends,
                            int32_t n_views, const double *thresholds, const double *null_scales, double *score, double *integrated,
                            double *mean, double *max_excess, int32_t *view) {
    if (n_seg <= 0) return 0;
    csr_ctx::PeakWs &w = c->peakWs;
    const size_t S = (size_t)n_seg, V = (size_t)n_views;
    // [starts | ends | thr | scale | stat | score | integ | mean | max | view]
    const size_t oStart = 0, oEnd = oStart + 8 * S, oThr = oEnd + 8 * S, oScale = oThr + 8 * V, oStat = oScale + 8 * V,
                 oScore = oStat + 16 * S * V, oInteg = oScore + 8 * S, oMean = oInteg + 8 * S, oMax = oMean + 8 * S, oView = oMax + 8 * S,
                 total = oView + 4 * S;
    CHECK(w.segBuf.reserve(total));
    char *base = (char *)w.segBuf.ptr;
    std::vector<double> sc(null_scales, null_scales + n_views);
    for (double &s : sc) s = std::max(s, DBL_MIN);      // (max(NaN, DBL_MIN) in Python's argument order keeps a NaN: std::max(s, ..) does too)
    HIPOK(hipMemcpyAsync(base + oStart, starts, 8 * S, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemcpyAsync(base + oEnd, ends, 8 * S, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemcpyAsync(base + oThr, thresholds, 8 * V, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemcpyAsync(base + oScale, sc.data(), 8 * V, hipMemcpyHostToDevice, c->stream));
    PeakScoreArgs a{};
    a.x = dx;
    a.n = n;
    a.starts = (const int64_t *)(base + oStart);
    a.ends = (const int64_t *)(base + oEnd);
    a.nSeg = (int)n_seg;
    a.nViews = n_views;
    a.thr = (const double *)(base + oThr);
    a.scale = (const double *)(base + oScale);
    a.stat = (double *)(base + oStat);
    a.score = (double *)(base + oScore);
    a.integ = (double *)(base + oInteg);
    a.mean = (double *)(base + oMean);
    a.mx = (double *)(base + oMax);
    a.view = (int *)(base + oView);
    {
        Scope scp(c, "peak_view_score");
        CHECK(launch(c, nullptr, "k_peak_view_score", k_peak_view_score, dim3((unsigned)n_seg, (unsigned)n_views), dim3(64), 0, c->stream, a));
        CHECK(launch(c, nullptr, "k_peak_view_pick", k_peak_view_pick, dim3((unsigned)((n_seg + 63) / 64)), dim3(64), 0, c->stream, a));
    }
    HIPOK(hipMemcpyAsync(score, a.score, 8 * S, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipMemcpyAsync(integrated, a.integ, 8 * S, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipMemcpyAsync(mean, a.mean, 8 * S, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipMemcpyAsync(max_excess, a.mx, 8 * S, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipMemcpyAsync(view, a.view, 4 * S, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    return 0;
}
static int peakscore_check(int64_t n, int64_t n_seg, const int64_t *starts, const int64_t *ends, int32_t n_views, const double *thresholds,
                           const double *null_scales, const void *o1, const void *o2, const void *o3, const void *o4, const void *o5) {
    if (n < 0 || n_seg < 0) return fail("negative size");
    if (n_seg > 0x7fffffffll) return fail("too many segments");
    if (n_views < 1 || n_views > PS_MAX_VIEWS) return fail("n_views must be in 1..%d", PS_MAX_VIEWS);
    if (!thresholds || !null_scales) return fail("null argument");
    if (n_seg > 0 && (!starts || !ends || !o1 || !o2 || !o3 || !o4 || !o5)) return fail("null argument");
    return 0;
}

extern "C" int csr_peakscore_segments(const double *scores, int64_t n, int64_t n_seg, const int64_t *starts, const int64_t *ends,
                                      int32_t n_views, const double *thresholds, const double *null_scales, double *score,
                                      double *integrated, double *mean, double *max_excess, int32_t *view) {
    DEFAULT_CTX_GUARD;
    CHECK(peakscore_check(n, n_seg, starts, ends, n_views, thresholds, null_scales, score, integrated, mean, max_excess, view));
    if (n > 0 && !scores) return fail("null argument");
    csr_ctx *c = nullptr;
    CHECK(ctx_or_default(c));
    const double *dx = nullptr;
    if (n > 0) CHECK(stage_vector(c, c->peakWs.xBuf, scores, n, &dx));       // (without a track every segment is empty)
    return peakscore_device(c, dx, n, n_seg, starts, ends, n_views, thresholds, null_scales, score, integrated, mean, max_excess, view);
}

// A chain's resident score track (csr_batch_rocco_scores / csr_batch_upload_scores), which is only read
extern "C" int csr_batch_peakscore_segments(csr_ctx *c, int32_t chain, int64_t n_seg, const int64_t *starts, const int64_t *ends,
                                            int32_t n_views, const double *thresholds, const double *null_scales, double *score,
                                            double *integrated, double *mean, double *max_excess, int32_t *view) {
    CHECK(need(c));
    CHECK(check_chain(c, chain));
    if (!c->scores.d) return fail("%s", NO_SCORES);
    if (!c->scores.has(chain)) return fail("chain %d has no %s", chain, c->scores.what);
    const int64_t n = c->chains[chain].n;
    CHECK(peakscore_check(n, n_seg, starts, ends, n_views, thresholds, null_scales, score, integrated, mean, max_excess, view));
    return peakscore_device(c, c->scores.at(c, chain), n, n_seg, starts, ends, n_views, thresholds, null_scales, score, integrated, mean,
                            max_excess, view);
}

// p, q and exceedance counts of observed[metric][K] against pool[metric][N]; R = the number of replay draws the pool was made of
// (empty ones included).  what: CSR_PEAK_P and / or CSR_PEAK_Q, CSR_PEAK_Q_MAX_P for q := max(q, p).
// pool: host values [metric][N], or (pool == nullptr, dev_cols != nullptr) one device column of N values per metric
static int peak_pq_core(csr_ctx *c, const double *observed, int64_t K, const double *pool, const double *const *dev_cols, int64_t N,
                        int64_t R, int32_t n_metrics, int32_t what, double *p_out, double *q_out, int64_t *exceed_out,
                        uint32_t *err_flags) {
    if (err_flags) *err_flags = 0;
    if (K < 0 || N < 0 || R < 0) return fail("negative size");
    if (n_metrics < 1 || n_metrics > PS_MAX_METRICS) return fail("n_metrics must be in 1..%d", PS_MAX_METRICS);
    const bool wantP = (what & CSR_PEAK_P) != 0, wantQ = (what & (CSR_PEAK_Q | CSR_PEAK_Q_MAX_P)) != 0;
    if (!wantP && !wantQ) return fail("`what` asks for nothing");
    if ((what & CSR_PEAK_Q_MAX_P) && !wantP) return fail("CSR_PEAK_Q_MAX_P needs CSR_PEAK_P");
    if (K == 0) return 0;
    if (!observed || (N > 0 && !pool && !dev_cols) || (wantP && !p_out) || (wantQ && !q_out)) return fail("null argument");
    if (N > 0 && R == 0) return fail("a pool of %lld values from no draws", (long long)N);
    csr_ctx::PeakWs &w = c->peakWs;
    const size_t M = (size_t)n_metrics, nObs = M * (size_t)K, nPool = pool ? M * (size_t)N : 0;
    // [observed | pool | p | q | raw | exceed | flag]
    const size_t oObs = 0, oPool = oObs + 8 * nObs, oP = oPool + 8 * nPool, oQ = oP + 8 * nObs, oRaw = oQ + 8 * nObs, oExc = oRaw + 8 * nObs,
                 oFlag = oExc + 8 * nObs, total = oFlag + 8;
    CHECK(w.pqBuf.reserve(total));
    char *base = (char *)w.pqBuf.ptr;
    const double *dObs = (const double *)(base + oObs), *dPool = (const double *)(base + oPool);
    unsigned int *dFlag = (unsigned int *)(base + oFlag);
    HIPOK(hipMemcpyAsync(base + oObs, observed, 8 * nObs, hipMemcpyHostToDevice, c->stream));
    if (N > 0 && pool) HIPOK(hipMemcpyAsync(base + oPool, pool, 8 * nPool, hipMemcpyHostToDevice, c->stream));
    std::vector<const double *> cols(M, nullptr);
    for (size_t m = 0; m < M && N > 0; ++m) cols[m] = pool ? dPool + m * (size_t)N : dev_cols[m];
    HIPOK(hipMemsetAsync(dFlag, 0, 8, c->stream));
    CHECK(launch(c, "peak_nonfinite", "k_peak_nonfinite", k_peak_nonfinite, dim3((unsigned)((nObs + 255) / 256)), dim3(256), 0, c->stream, dObs,
                 (int64_t)nObs, dFlag, (unsigned int)CSR_PEAK_BAD_OBSERVED));
    for (size_t m = 0; m < M && N > 0; ++m)
        CHECK(launch(c, "peak_nonfinite", "k_peak_nonfinite", k_peak_nonfinite, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, c->stream,
                     cols[m], N, dFlag, (unsigned int)CSR_PEAK_BAD_POOL));
    unsigned int flags = 0;
    HIPOK(hipMemcpyAsync(&flags, dFlag, 4, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    if (err_flags) *err_flags = flags;
    // the reference computes every p value first (peaks.py:2924-2940); without a pooled value it never looks at the observed ones
    if (flags && wantP && N > 0) return value_error("replay segment statistics contain non-finite values");
    if (flags && wantQ) return value_error("replay FDR statistics contain non-finite values");
    if (flags) {                        // p values without a pool: all ones whatever the observed values are; nothing sorts a NaN
        std::fill(p_out, p_out + nObs, 1.0);
        if (exceed_out) std::fill(exceed_out, exceed_out + nObs, (int64_t)0);
        return 0;
    }
    NullEngine E;
    E.c = c;
    std::vector<NullTrackHost> tracks;
    for (size_t m = 0; m < M; ++m) tracks.push_back(NullTrackHost{dObs + m * (size_t)K, K, nullptr, false, 0.0, 0.0});
    if (N > 0)
        for (size_t m = 0; m < M; ++m) tracks.push_back(NullTrackHost{cols[m], N, nullptr, false, 0.0, 0.0});
    CHECK(E.setup(tracks, false));
    CHECK(E.sort());
    PoolPqArgs a{};
    a.nMetrics = n_metrics;
    a.K = K;
    a.N = N;
    a.R = R;
    a.obs = dObs;
    a.obsSorted = E.sorted + E.tr[0].slot;
    a.obsStride = E.tr[0].padded;
    a.poolSorted = N > 0 ? E.sorted + E.tr[M].slot : nullptr;
    a.poolStride = N > 0 ? E.tr[M].padded : 0;
    a.p = (double *)(base + oP);
    a.q = (double *)(base + oQ);
    a.raw = (double *)(base + oRaw);
    a.exceed = (long long *)(base + oExc);
    a.combine = (what & CSR_PEAK_Q_MAX_P) != 0;
    const dim3 grid((unsigned)((nObs + 255) / 256));
    {
        Scope scp(c, "peak_pq");
        CHECK(launch(c, nullptr, "k_pool_tail_counts", k_pool_tail_counts, grid, dim3(256), 0, c->stream, a));
        if (wantQ) {
            CHECK(launch(c, nullptr, "k_replay_raw", k_replay_raw, grid, dim3(256), 0, c->stream, a));
            CHECK(launch(c, nullptr, "k_replay_scan", k_replay_scan, dim3((unsigned)n_metrics), dim3(256), 0, c->stream, a));
            CHECK(launch(c, nullptr, "k_replay_scatter", k_replay_scatter, grid, dim3(256), 0, c->stream, a));
        }
    }
    if (wantP) HIPOK(hipMemcpyAsync(p_out, a.p, 8 * nObs, hipMemcpyDeviceToHost, c->stream));
    if (wantQ) HIPOK(hipMemcpyAsync(q_out, a.q, 8 * nObs, hipMemcpyDeviceToHost, c->stream));
    if (exceed_out) HIPOK(hipMemcpyAsync(exceed_out, a.exceed, 8 * nObs, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int csr_peakscore_pq(const double *observed, int64_t K, const double *pool, int64_t N, int64_t R, int32_t n_metrics,
                                int32_t what, double *p_out, double *q_out, int64_t *exceed_out, uint32_t *err_flags) {
    DEFAULT_CTX_GUARD;
    csr_ctx *c = nullptr;
    CHECK(ctx_or_default(c));
    if (N > 0 && !pool) return fail("null argument");
    return peak_pq_core(c, observed, K, pool, nullptr, N, R, n_metrics, what, p_out, q_out, exceed_out, err_flags);
}

// ---------------------------------------------------------------------------------------------------------------
// the replay pool of a DWB panel: between csr_dwb_panel_begin and csr_dwb_panel_end
// ---------------------------------------------------------------------------------------------------------------
static void peak_pool_release(csr_ctx *c) {
    c->pool = csr_ctx::PeakPool{};      // (DevBuf members free what they own)
    c->seg.deviceOnly = false;
}
static int pool_need(csr_ctx *&c) {
    CHECK(ctx_or_default(c));
    if (!c->dwb.ready) return fail("no DWB panel: call csr_dwb_panel_begin first");
    if (!c->pool.active) return fail("no replay pool: call csr_dwb_panel_pool_begin first");
    return 0;
}
extern "C" int csr_dwb_panel_pool_begin(csr_ctx *c, int64_t max_segments) {
    DEFAULT_CTX_GUARD;
    CHECK(ctx_or_default(c));
    if (!c->dwb.ready) return fail("no DWB panel: call csr_dwb_panel_begin first");
    csr_ctx::PeakPool &P = c->pool;
    P = csr_ctx::PeakPool{};
    P.active = true;
    P.nc = (int)c->dwb.chains.size();
    P.nDraws = c->dwb.nDraws;
    P.totalCap = max_segments > 0 ? max_segments : 0;
    P.col.resize(3 * (size_t)P.nc);
    P.n.assign((size_t)P.nc, 0);
    P.cap.assign((size_t)P.nc, 0);
    const size_t cd = (size_t)P.nc * (size_t)P.nDraws;
    P.count.assign(cd, -1);
    P.before.assign(cd, -1);
    P.counters.assign(3 * cd, 0);
    P.mx.assign(cd, 0.0);
    c->seg.deviceOnly = true;
    c->seg.have = false;
    return 0;
}
// chain i's columns can take `want` values (kept values move along)
static int pool_grow(csr_ctx *c, int i, int64_t want) {
    csr_ctx::PeakPool &P = c->pool;
    if (want <= P.cap[i]) return 0;
    const int64_t cap = std::max<int64_t>(want, 2 * P.cap[i]);
    for (int k = 0; k < 3; ++k) {
        DevBuf nb;
        CHECK(nb.reserve(8 * (size_t)cap));
        if (P.n[i] > 0) HIPOK(hipMemcpyAsync(nb.ptr, P.col[3 * i + k].ptr, 8 * (size_t)P.n[i], hipMemcpyDeviceToDevice, c->stream));
        HIPOK(hipStreamSynchronize(c->stream));
        P.col[3 * i + k] = std::move(nb);
    }
    P.cap[i] = cap;
    return 0;
}
// The group of draws csr_dwb_panel_segments(first_draw, ..) just ran, every flagged view resolved: its candidates go to the pool
extern "C" int csr_dwb_panel_pool_append(csr_ctx *c, int32_t first_draw, int32_t *n_flagged) {
    DEFAULT_CTX_GUARD;
    CHECK(pool_need(c));
    csr_ctx::PeakPool &P = c->pool;
    csr_ctx::Seg &g = c->seg;
    if (!n_flagged) return fail("null argument");
    if (!g.have || !g.deviceOnly) return fail("no csr_dwb_panel_segments run since csr_dwb_panel_pool_begin");
    for (const auto &f : P.flagged)
        if (!f.resolved) return fail("a host-decided draw of the previous group has not been uploaded");
    for (const auto &f : g.flagged)
        if (!f.resolved) return fail("a flagged view has not been resolved (csr_segments_flagged_select)");
    const int nTracks = (int)g.rowsPerTrack.size();
    if (nTracks % P.nc != 0) return fail("the last segment run is not a group of this panel");
    const int nRows = nTracks / P.nc;
    if (first_draw < 0 || first_draw + nRows > P.nDraws) return fail("draws out of range");
    for (int i = 0; i < P.nc; ++i)
        for (int r = 0; r < nRows; ++r)
            if (P.count[(size_t)i * P.nDraws + first_draw + r] >= 0) return fail("draw %d is in the pool already", first_draw + r);
    P.flagged.clear();
    *n_flagged = 0;
    const size_t n = g.oStart.size();
    const size_t slot = (8 * n + 255) / 256 * 256;
    char *ob = (char *)g.outBuf.ptr;
    double *dScore = (double *)(ob + 2 * slot), *dInteg = (double *)(ob + 3 * slot), *dMax = (double *)(ob + 5 * slot);
    // the rows of the views the caller decided: only the host holds them (all six columns: a host-decided draw is fetched whole)
    for (const auto &f : g.flagged) {
        const size_t o = (size_t)f.base, k = (size_t)g.cap;
        const void *src[6] = {g.oStart.data() + o, g.oEnd.data() + o, g.oScore.data() + o, g.oInteg.data() + o, g.oMean.data() + o,
                              g.oMax.data() + o};
        for (int q = 0; q < 6; ++q) HIPOK(hipMemcpyAsync(ob + q * slot + 8 * o, src[q], 8 * k, hipMemcpyHostToDevice, c->stream));
    }
    // room first (a column may move), then the tracks' places
    for (int i = 0; i < P.nc; ++i) {
        int64_t add = 0;
        for (int r = 0; r < nRows; ++r) {
            const int64_t rows = g.rowsPerTrack[(size_t)i * nRows + r];
            add += P.totalCap > 0 ? std::min(rows, P.totalCap) : rows;
        }
        CHECK(pool_grow(c, i, P.n[i] + add));
    }
    std::vector<PoolTrack> jobs;
    std::vector<int> jobTrack;
    std::vector<int64_t> jobSlot;
    int64_t rowBase = 0;
    for (int i = 0; i < P.nc; ++i)
        for (int r = 0; r < nRows; ++r) {
            const int t = i * nRows + r;
            const size_t cd = (size_t)i * P.nDraws + first_draw + r;
            const int64_t rows = g.rowsPerTrack[t], keep = P.totalCap > 0 ? std::min(rows, P.totalCap) : rows;
            P.before[cd] = rows;
            P.count[cd] = keep;
            for (int k = 0; k < 3; ++k) P.counters[3 * cd + k] = g.counters[3 * (size_t)t + k];
            P.mx[cd] = 0.0;
            if (rows > 0) {
                PoolTrack j{};
                j.rowBase = rowBase;
                j.rows = rows;
                j.keep = keep;
                for (int k = 0; k < 3; ++k) j.dst[k] = (double *)P.col[3 * i + k].ptr + P.n[i];
                jobs.push_back(j);
                jobTrack.push_back(t);
                jobSlot.push_back(P.n[i]);
                P.n[i] += keep;
            }
            rowBase += rows;
        }
    if (jobs.empty()) return 0;
    const size_t nj = jobs.size();
    CHECK(P.jobBuf.reserve(sizeof(PoolTrack) * nj));
    CHECK(P.outBuf.reserve(16 * nj));
    double *dOutMax = (double *)P.outBuf.ptr;
    int *dOutFlag = (int *)((char *)P.outBuf.ptr + 8 * nj);
    HIPOK(hipMemcpyAsync(P.jobBuf.ptr, jobs.data(), sizeof(PoolTrack) * nj, hipMemcpyHostToDevice, c->stream));
    CHECK(launch(c, "pool_append", "k_pool_append", k_pool_append, dim3((unsigned)nj), dim3(256), 0, c->stream,
                 (const PoolTrack *)P.jobBuf.ptr, (const double *)dScore, (const double *)dInteg, (const double *)dMax, dOutMax, dOutFlag));
    std::vector<double> mx(nj);
    std::vector<int> fl(nj);
    HIPOK(hipMemcpyAsync(mx.data(), dOutMax, 8 * nj, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipMemcpyAsync(fl.data(), dOutFlag, 4 * nj, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    for (size_t q = 0; q < nj; ++q) {
        const int t = jobTrack[q], i = t / nRows, r = t % nRows;
        P.mx[(size_t)i * P.nDraws + first_draw + r] = mx[q];
        if (fl[q]) P.flagged.push_back(csr_ctx::PeakPool::Flagged{i, first_draw + r, jobs[q].rowBase, jobs[q].rows, jobSlot[q], false});
    }
    *n_flagged = (int32_t)P.flagged.size();
    return 0;
}
extern "C" int csr_dwb_panel_pool_flagged(csr_ctx *c, int32_t k, int32_t *chain, int32_t *draw, int64_t *n_rows) {
    DEFAULT_CTX_GUARD;
    CHECK(pool_need(c));
    if (k < 0 || k >= (int)c->pool.flagged.size() || !chain || !draw || !n_rows) return fail("host-decided draw index out of range");
    const auto &f = c->pool.flagged[k];
    *chain = f.chain;
    *draw = f.draw;
    *n_rows = f.rows;
    return 0;
}
// the rows of a host-decided draw (the only replay rows that leave the device): the eight columns of csr_segments_fetch
extern "C" int csr_dwb_panel_pool_flagged_fetch(csr_ctx *c, int32_t k, int64_t *start, int64_t *end, int64_t *scale, int64_t *view,
                                                double *score, double *integrated, double *mean, double *max_excess) {
    DEFAULT_CTX_GUARD;
    CHECK(pool_need(c));
    csr_ctx::Seg &g = c->seg;
    if (k < 0 || k >= (int)c->pool.flagged.size()) return fail("host-decided draw index out of range");
    if (!start || !end || !scale || !view || !score || !integrated || !mean || !max_excess) return fail("null argument");
    const auto &f = c->pool.flagged[k];
    const size_t n = g.oStart.size(), slot = (8 * n + 255) / 256 * 256, o = (size_t)f.rowBase, m = (size_t)f.rows;
    char *ob = (char *)g.outBuf.ptr;
    void *dst[6] = {start, end, score, integrated, mean, max_excess};
    for (int q = 0; q < 6; ++q) HIPOK(hipMemcpyAsync(dst[q], ob + q * slot + 8 * o, 8 * m, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    std::copy(g.oScale.begin() + o, g.oScale.begin() + o + m, scale);
    std::copy(g.oView.begin() + o, g.oView.begin() + o + m, view);
    c->pool.fetchedTracks++;
    return 0;
}
// what the caller kept of it: exactly the total cap's number of candidates
extern "C" int csr_dwb_panel_pool_flagged_upload(csr_ctx *c, int32_t k, int64_t n_values, const double *score, const double *integrated,
                                                 const double *max_excess) {
    DEFAULT_CTX_GUARD;
    CHECK(pool_need(c));
    csr_ctx::PeakPool &P = c->pool;
    if (k < 0 || k >= (int)P.flagged.size()) return fail("host-decided draw index out of range");
    auto &f = P.flagged[k];
    if (n_values != P.totalCap || !score || !integrated || !max_excess) return fail("a host-decided draw takes exactly %lld candidates", (long long)P.totalCap);
    const double *src[3] = {score, integrated, max_excess};
    for (int q = 0; q < 3; ++q)
        HIPOK(hipMemcpyAsync((double *)P.col[3 * f.chain + q].ptr + f.slot, src[q], 8 * (size_t)n_values, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    double best = score[0];             // np.max: a NaN stays
    for (int64_t i = 1; i < n_values; ++i) best = best != best ? best : (score[i] != score[i] ? score[i] : std::max(best, score[i]));
    P.mx[(size_t)f.chain * P.nDraws + f.draw] = best;
    f.resolved = true;
    return 0;
}
// per (chain, draw): candidates after and before the total cap, phase 1's three counters, np.max of the kept scores; fetched =
// how many draws' rows left the device (the host-decided ones)
extern "C" int csr_dwb_panel_pool_draw_stats(csr_ctx *c, int64_t *count, int64_t *before, int64_t *counters, double *max_score,
                                             int64_t *fetched_tracks) {
    DEFAULT_CTX_GUARD;
    CHECK(pool_need(c));
    const csr_ctx::PeakPool &P = c->pool;
    if (!count || !before || !counters || !max_score) return fail("null argument");
    for (int64_t v : P.count)
        if (v < 0) return fail("not every draw of the panel has been appended");
    for (const auto &f : P.flagged)
        if (!f.resolved) return fail("a host-decided draw has not been uploaded");
    std::copy(P.count.begin(), P.count.end(), count);
    std::copy(P.before.begin(), P.before.end(), before);
    std::copy(P.counters.begin(), P.counters.end(), counters);
    std::copy(P.mx.begin(), P.mx.end(), max_score);
    if (fetched_tracks) *fetched_tracks = P.fetchedTracks;
    return 0;
}
// csr_peakscore_pq of observed[3][K] (score, integrated excess, max excess) against one chain's pool
extern "C" int csr_dwb_panel_pool_pq(csr_ctx *c, int32_t chain, const double *observed, int64_t K, int32_t what, double *p_out,
                                     double *q_out, int64_t *exceed_out, uint32_t *err_flags) {
    DEFAULT_CTX_GUARD;
    CHECK(pool_need(c));
    const csr_ctx::PeakPool &P = c->pool;
    if (chain < 0 || chain >= P.nc) return fail("chain index out of range");
    for (const auto &f : P.flagged)
        if (!f.resolved) return fail("a host-decided draw has not been uploaded");
    const double *cols[3] = {(const double *)P.col[3 * chain].ptr, (const double *)P.col[3 * chain + 1].ptr,
                             (const double *)P.col[3 * chain + 2].ptr};
    return peak_pq_core(c, observed, K, nullptr, cols, P.n[chain], P.nDraws, 3, what, p_out, q_out, exceed_out, err_flags);
}
// a chain's pool as it stands (tests, callers that want the statistics themselves): *n values per column; the columns may be NULL
extern "C" int csr_dwb_panel_pool_download(csr_ctx *c, int32_t chain, int64_t *n, double *score, double *integrated, double *max_excess) {
    DEFAULT_CTX_GUARD;
    CHECK(pool_need(c));
    const csr_ctx::PeakPool &P = c->pool;
    if (chain < 0 || chain >= P.nc || !n) return fail("chain index out of range");
    *n = P.n[chain];
    double *dst[3] = {score, integrated, max_excess};
    for (int q = 0; q < 3; ++q)
        if (dst[q] && P.n[chain] > 0)
            HIPOK(hipMemcpyAsync(dst[q], P.col[3 * chain + q].ptr, 8 * (size_t)P.n[chain], hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    return 0;
}
extern "C" int csr_dwb_panel_pool_end(csr_ctx *c) {
    DEFAULT_CTX_GUARD;
    CHECK(ctx_or_default(c));
    HIPOK(hipStreamSynchronize(c->stream));
    peak_pool_release(c);
    return 0;
}
