// csr_host_depspan.inl -- part of csr_lib.hip (one translation unit; included in this order): the three device stages of the
// dependence span (pyx:3360-4120 `cchooseDependenceSpan`) from the kernels of csr_depspan.h -- which rows are byte-identical, the
// ranking score of every full window, and the masked autocorrelation of a list of windows up to the crossing decision.  One
// implementation serves both entries: the batch entry points at the RESIDENT data of the listed chains (c->p.data + off, stride
// Npad) and changes nothing resident; the host-array entry stages one chromosome (rows, scores) or one packed window set (ACF) in
// work space.  Windows go out in groups sized by the work space, so any window length and any number of windows run.

constexpr size_t DEP_WS_BYTES = (size_t)256 << 20;      // what the per-(window, row) work arrays of one group may take

static int depspan_check_rows(int64_t n_rows_total, int32_t n_rows, const int32_t *rows) {
    if (!rows || n_rows < 1) return fail("depspan: no rows");
    if (n_rows > 4096) return fail("depspan: at most 4096 rows (got %d)", n_rows);
    for (int r = 0; r < n_rows; ++r)
        if (rows[r] < 0 || rows[r] >= n_rows_total) return fail("depspan: row %d out of range", rows[r]);
    return 0;
}
static int depspan_upload_rows(csr_ctx *c, int32_t n_rows, const int32_t *rows, const int **dRows) {
    csr_ctx::DepWs &ws = c->depWs;
    CHECK(ws.rowBuf.reserve(sizeof(int) * (size_t)n_rows));
    HIPOK(hipMemcpyAsync(ws.rowBuf.ptr, rows, sizeof(int) * (size_t)n_rows, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    *dRows = (const int *)ws.rowBuf.ptr;
    return 0;
}

// ---- row equality: flags over all pairs i < j, OR-ed over the matrices given so far ----------------------------------------
struct DepUnique {
    csr_ctx *c;
    int nRows = 0;
    int64_t nPairs = 0;
    int begin(int n_rows) {
        nRows = n_rows;
        nPairs = (int64_t)n_rows * (n_rows - 1) / 2;
        if (nPairs == 0) return 0;
        csr_ctx::DepWs &ws = c->depWs;
        std::vector<int> tab((size_t)(2 * nPairs));
        int64_t p = 0;
        for (int j = 1; j < n_rows; ++j)
            for (int i = 0; i < j; ++i, ++p) {
                tab[(size_t)p] = i;
                tab[(size_t)(nPairs + p)] = j;
            }
        CHECK(ws.pairTab.reserve(sizeof(int) * tab.size()));
        CHECK(ws.diffBuf.reserve(sizeof(unsigned) * (size_t)nPairs));
        HIPOK(hipMemcpyAsync(ws.pairTab.ptr, tab.data(), sizeof(int) * tab.size(), hipMemcpyHostToDevice, c->stream));
        HIPOK(hipMemsetAsync(ws.diffBuf.ptr, 0, sizeof(unsigned) * (size_t)nPairs, c->stream));
        HIPOK(hipStreamSynchronize(c->stream));     // (tab dies here)
        return 0;
    }
    int add(const std::vector<DepMat> &mats) {
        if (nPairs == 0 || mats.empty()) return 0;
        csr_ctx::DepWs &ws = c->depWs;
        CHECK(ws.matBuf.reserve(sizeof(DepMat) * mats.size()));
        HIPOK(hipMemcpyAsync(ws.matBuf.ptr, mats.data(), sizeof(DepMat) * mats.size(), hipMemcpyHostToDevice, c->stream));
        int64_t longest = 0;
        for (const DepMat &m : mats) longest = std::max(longest, m.n);
        const int *pi = (const int *)ws.pairTab.ptr, *pj = pi + nPairs;
        for (int64_t p0 = 0; p0 < nPairs; p0 += 32768) {        // (grid.y is a 16-bit dimension)
            const int64_t np = std::min<int64_t>(32768, nPairs - p0);
            const dim3 grid((unsigned)((longest + DEP_CMP - 1) / DEP_CMP), (unsigned)np, (unsigned)mats.size());
            CHECK(launch(c, "depspan_rowdiff", "k_depspan_rowdiff", k_depspan_rowdiff, grid, dim3(256), 0, c->stream,
                         (const DepMat *)ws.matBuf.ptr, pi + p0, pj + p0, (unsigned *)ws.diffBuf.ptr + p0));
        }
        HIPOK(hipStreamSynchronize(c->stream));     // (mats may be a staged matrix the caller reuses)
        return 0;
    }
    // row j is dropped iff an earlier row equals it everywhere (equality is transitive: an earlier RETAINED row then does too)
    int end(int32_t *retained, int32_t *n_retained) {
        std::vector<unsigned> diff((size_t)nPairs);
        if (nPairs > 0) {
            HIPOK(hipMemcpyAsync(diff.data(), c->depWs.diffBuf.ptr, sizeof(unsigned) * (size_t)nPairs, hipMemcpyDeviceToHost, c->stream));
            HIPOK(hipStreamSynchronize(c->stream));
        }
        int kept = 0;
        int64_t p = 0;
        for (int j = 0; j < nRows; ++j) {
            bool dup = false;
            for (int i = 0; i < j; ++i, ++p) dup = dup || diff[(size_t)p] == 0;
            if (!dup) retained[kept++] = j;
        }
        *n_retained = kept;
        return 0;
    }
};

// ---- window scores of one matrix: score[w] = np.median of the contributing rows' scores (NaN: none), count[w] of them -----
static int depspan_scores_mat(csr_ctx *c, const DepMat &mt, const int *dRows, int nRows, int64_t wb, double rankMin, double *score,
                              int64_t *count) {
    const int64_t nW = mt.n / wb;
    if (nW <= 0) return 0;
    csr_ctx::DepWs &ws = c->depWs;
    const int64_t G = std::max<int64_t>(1, std::min<int64_t>(nW, (int64_t)(DEP_WS_BYTES / (8 * (size_t)nRows * (size_t)wb))));
    CHECK(ws.compBuf.reserve(8 * (size_t)G * nRows * wb));
    CHECK(ws.sumBuf.reserve(8 * (size_t)nW * nRows));
    DepScoreArgs a{};
    a.base = mt.base;
    a.stride = mt.stride;
    a.rows = dRows;
    a.nRows = nRows;
    a.windowBins = wb;
    a.rankMin = rankMin;
    a.comp = (double *)ws.compBuf.ptr;
    a.score = (double *)ws.sumBuf.ptr;
    for (int64_t w0 = 0; w0 < nW; w0 += G) {
        a.w0 = w0;
        const dim3 grid((unsigned)std::min<int64_t>(G, nW - w0), (unsigned)nRows);
        CHECK(launch(c, "depspan_scores", "k_depspan_scores", k_depspan_scores, grid, dim3(256), 0, c->stream, a));
    }
    std::vector<double> rs((size_t)nW * nRows);
    HIPOK(hipMemcpyAsync(rs.data(), ws.sumBuf.ptr, 8 * rs.size(), hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    std::vector<double> v;
    for (int64_t w = 0; w < nW; ++w) {
        v.clear();
        for (int r = 0; r < nRows; ++r) {
            const double s = rs[(size_t)w * nRows + r];
            if (s == s) v.push_back(s);
        }
        count[w] = (int64_t)v.size();
        score[w] = NAN;
        if (v.empty()) continue;
        std::sort(v.begin(), v.end());
        const size_t h = v.size() / 2;
        score[w] = (v.size() & 1) ? v[h] : (v[h - 1] + v[h]) / 2.0;     // np.median: the mean of the two middle values
    }
    return 0;
}

// ---- window ACF: one record and maxLag pooled values per window ---------------------------------------------------------
static int depspan_check_cfg(const csr_depspan_cfg *cfg) {
    if (!cfg) return fail("null argument");
    if (cfg->window_bins < 2) return fail("depspan: window_bins must be at least 2");
    if (cfg->max_lag_bins < 1 || cfg->max_lag_bins > cfg->window_bins / 2) return fail("depspan: max_lag_bins must be in [1, window_bins / 2]");
    if (cfg->smoothing_bins < 1 || (cfg->smoothing_bins & 1) == 0 || cfg->smoothing_bins > cfg->max_lag_bins)
        return fail("depspan: smoothing_bins must be odd and in [1, max_lag_bins]");
    if (cfg->persistence_bins < 1 || cfg->persistence_bins > cfg->max_lag_bins) return fail("depspan: persistence_bins must be in [1, max_lag_bins]");
    if (cfg->min_finite_pairs < 1) return fail("depspan: min_finite_pairs must be positive");
    if (!(cfg->acf_threshold > 0.0 && cfg->acf_threshold < 1.0)) return fail("depspan: acf_threshold must be in (0, 1)");
    if (!(cfg->min_finite_pair_coverage > 0.0 && cfg->min_finite_pair_coverage <= 1.0)) return fail("depspan: min_finite_pair_coverage must be in (0, 1]");
    return 0;
}
static int depspan_acf_run(csr_ctx *c, const std::vector<DepWin> &wins, const int *dRows, int nRows, const csr_depspan_cfg *cfg,
                           csr_depspan_window *rec, double *pooled) {
    static_assert(sizeof(DepRec) == sizeof(csr_depspan_window), "record layouts differ");
    const int64_t nWin = (int64_t)wins.size();
    if (nWin == 0) return 0;
    csr_ctx::DepWs &ws = c->depWs;
    const int64_t wb = cfg->window_bins;
    const int ML = cfg->max_lag_bins, L = ML + 1;
    // (per window and row: 16 bytes per bin, and 20 per lag -- the sums, the pair counts, the median's work space)
    const int64_t G = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(nWin, 32768), (int64_t)(DEP_WS_BYTES / (16 * (size_t)nRows * (size_t)wb))));
    CHECK(ws.winBuf.reserve(sizeof(DepWin) * (size_t)G));
    CHECK(ws.compBuf.reserve(8 * (size_t)G * nRows * wb));
    CHECK(ws.cenBuf.reserve(8 * (size_t)G * nRows * wb));
    CHECK(ws.nfinBuf.reserve(4 * (size_t)G * nRows));
    CHECK(ws.sumBuf.reserve(8 * (size_t)G * nRows * L));
    CHECK(ws.pairBuf.reserve(4 * (size_t)G * nRows * L));
    CHECK(ws.lagBuf.reserve((8 + 4 + 8 + 8) * (size_t)G * ML + 8 * (size_t)G * L));
    CHECK(ws.medBuf.reserve(8 * (size_t)G * ML * nRows + 8 * (size_t)G * nRows));
    CHECK(ws.recBuf.reserve(sizeof(DepRec) * (size_t)G));
    DepAcfArgs a{};
    a.wins = (const DepWin *)ws.winBuf.ptr;
    a.rows = dRows;
    a.nRows = nRows;
    a.cfg = DepCfg{wb, ML, cfg->smoothing_bins, cfg->persistence_bins, cfg->min_finite_pairs, cfg->acf_threshold, cfg->min_finite_pair_coverage};
    a.comp = (double *)ws.compBuf.ptr;
    a.cen = (double *)ws.cenBuf.ptr;
    a.nfin = (int *)ws.nfinBuf.ptr;
    a.sums = (double *)ws.sumBuf.ptr;
    a.pairs = (int *)ws.pairBuf.ptr;
    a.pooled = (double *)ws.lagBuf.ptr;                 // the doubles first, the ints last
    a.minPair = a.pooled + (size_t)G * ML;
    a.minCov = a.minPair + (size_t)G * ML;
    a.prefix = a.minCov + (size_t)G * ML;
    a.contrib = (int *)(a.prefix + (size_t)G * L);
    a.med = (double *)ws.medBuf.ptr;
    a.zero = a.med + (size_t)G * ML * nRows;
    a.rec = (DepRec *)ws.recBuf.ptr;
    for (int64_t g0 = 0; g0 < nWin; g0 += G) {
        const int64_t ng = std::min<int64_t>(G, nWin - g0);
        HIPOK(hipMemcpyAsync(ws.winBuf.ptr, wins.data() + g0, sizeof(DepWin) * (size_t)ng, hipMemcpyHostToDevice, c->stream));
        CHECK(launch(c, "depspan_center", "k_depspan_center", k_depspan_center, dim3((unsigned)ng, (unsigned)nRows), dim3(256), 0, c->stream, a));
        CHECK(launch(c, "depspan_lags", "k_depspan_lags", k_depspan_lags, dim3((unsigned)((L + DEP_WAVE - 1) / DEP_WAVE), (unsigned)nRows, (unsigned)ng),
                     dim3(DEP_WAVE), 0, c->stream, a));
        CHECK(launch(c, "depspan_pool", "k_depspan_pool", k_depspan_pool, dim3((unsigned)ng), dim3(256), 0, c->stream, a));
        HIPOK(hipMemcpyAsync(rec + g0, ws.recBuf.ptr, sizeof(DepRec) * (size_t)ng, hipMemcpyDeviceToHost, c->stream));
        HIPOK(hipMemcpyAsync(pooled + g0 * ML, a.pooled, 8 * (size_t)ng * ML, hipMemcpyDeviceToHost, c->stream));
        HIPOK(hipStreamSynchronize(c->stream));
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// host arrays (default context): mats[k] = n_rows x n_bins[k] float32, C order
// ---------------------------------------------------------------------------------------------------------------
static int depspan_check_mats(int32_t n_mats, const int64_t *n_bins, const float *const *mats, int64_t n_rows) {
    if (n_mats < 1 || !n_bins || !mats || n_rows < 1) return fail("depspan: no matrices");
    for (int k = 0; k < n_mats; ++k)
        if (!mats[k] || n_bins[k] < 1) return fail("depspan: matrix %d is empty", k);
    return 0;
}
// mt := matrix k staged in work space
static int depspan_stage(csr_ctx *c, const float *host, int64_t n_rows, int64_t n, DepMat &mt) {
    csr_ctx::DepWs &ws = c->depWs;
    CHECK(ws.stageBuf.reserve(4 * (size_t)n_rows * (size_t)n));
    HIPOK(hipMemcpyAsync(ws.stageBuf.ptr, host, 4 * (size_t)n_rows * (size_t)n, hipMemcpyHostToDevice, c->stream));
    mt = DepMat{(const float *)ws.stageBuf.ptr, n, n};
    return 0;
}

extern "C" int csr_depspan_unique_rows(int32_t n_mats, const int64_t *n_bins, const float *const *mats, int64_t n_rows,
                                       int32_t *retained, int32_t *n_retained) {
    DEFAULT_CTX_GUARD;
    CHECK(depspan_check_mats(n_mats, n_bins, mats, n_rows));
    if (!retained || !n_retained) return fail("null argument");
    if (n_rows > 4096) return fail("depspan: at most 4096 rows");
    csr_ctx *c = nullptr;
    CHECK(ctx_or_default(c));
    DepUnique U{c};
    CHECK(U.begin((int)n_rows));
    for (int k = 0; k < n_mats; ++k) {
        DepMat mt;
        CHECK(depspan_stage(c, mats[k], n_rows, n_bins[k], mt));
        CHECK(U.add({mt}));
    }
    return U.end(retained, n_retained);
}

extern "C" int csr_depspan_window_scores(int32_t n_mats, const int64_t *n_bins, const float *const *mats, int64_t n_rows_total,
                                         int32_t n_rows, const int32_t *rows, int64_t window_bins, double rank_coverage_min,
                                         double *score, int64_t *count) {
    DEFAULT_CTX_GUARD;
    CHECK(depspan_check_mats(n_mats, n_bins, mats, n_rows_total));
    CHECK(depspan_check_rows(n_rows_total, n_rows, rows));
    if (window_bins < 2) return fail("depspan: window_bins must be at least 2");
    if (!score || !count) return fail("null argument");
    csr_ctx *c = nullptr;
    CHECK(ctx_or_default(c));
    const int *dRows;
    CHECK(depspan_upload_rows(c, n_rows, rows, &dRows));
    int64_t at = 0;
    for (int k = 0; k < n_mats; ++k) {
        if (n_bins[k] < window_bins) continue;
        DepMat mt;
        CHECK(depspan_stage(c, mats[k], n_rows_total, n_bins[k], mt));
        CHECK(depspan_scores_mat(c, mt, dRows, n_rows, window_bins, rank_coverage_min, score + at, count + at));
        at += n_bins[k] / window_bins;
    }
    return 0;
}

extern "C" int csr_depspan_window_acf(int32_t n_mats, const int64_t *n_bins, const float *const *mats, int64_t n_rows_total,
                                      int32_t n_rows, const int32_t *rows, const csr_depspan_cfg *cfg, int64_t n_windows,
                                      const int32_t *win_mat, const int64_t *win_start, csr_depspan_window *rec, double *pooled) {
    DEFAULT_CTX_GUARD;
    CHECK(depspan_check_mats(n_mats, n_bins, mats, n_rows_total));
    CHECK(depspan_check_rows(n_rows_total, n_rows, rows));
    CHECK(depspan_check_cfg(cfg));
    if (n_windows < 0 || (n_windows > 0 && (!win_mat || !win_start || !rec || !pooled))) return fail("null argument");
    const int64_t wb = cfg->window_bins;
    for (int64_t w = 0; w < n_windows; ++w) {
        if (win_mat[w] < 0 || win_mat[w] >= n_mats) return fail("depspan: window %lld names matrix %d", (long long)w, win_mat[w]);
        if (win_start[w] < 0 || win_start[w] + wb > n_bins[win_mat[w]]) return fail("depspan: window %lld leaves its matrix", (long long)w);
    }
    if (n_windows == 0) return 0;
    csr_ctx *c = nullptr;
    CHECK(ctx_or_default(c));
    // the window set, packed: [window][retained row][window_bins]
    std::vector<float> pack((size_t)n_windows * n_rows * wb);
    for (int64_t w = 0; w < n_windows; ++w)
        for (int r = 0; r < n_rows; ++r)
            memcpy(&pack[((size_t)w * n_rows + r) * wb], mats[win_mat[w]] + (size_t)rows[r] * n_bins[win_mat[w]] + win_start[w], 4 * (size_t)wb);
    csr_ctx::DepWs &ws = c->depWs;
    CHECK(ws.stageBuf.reserve(4 * pack.size()));
    HIPOK(hipMemcpyAsync(ws.stageBuf.ptr, pack.data(), 4 * pack.size(), hipMemcpyHostToDevice, c->stream));
    std::vector<int32_t> ident((size_t)n_rows);
    for (int r = 0; r < n_rows; ++r) ident[r] = r;
    const int *dRows;
    CHECK(depspan_upload_rows(c, n_rows, ident.data(), &dRows));       // (synchronises: pack is on the device)
    std::vector<DepWin> wins((size_t)n_windows);
    for (int64_t w = 0; w < n_windows; ++w) wins[w] = DepWin{(const float *)ws.stageBuf.ptr + (size_t)w * n_rows * wb, wb};
    return depspan_acf_run(c, wins, dRows, n_rows, cfg, rec, pooled);
}

// ---------------------------------------------------------------------------------------------------------------
// batch context: the RESIDENT data of the listed chains (a fold chain is left out by not listing it); nothing resident changes
// ---------------------------------------------------------------------------------------------------------------
static int depspan_batch_mats(csr_ctx *c, int32_t n_listed, const int32_t *chains, std::vector<DepMat> &mats) {
    CHECK(need(c));
    if (n_listed < 1 || !chains) return fail("depspan: no chains listed");
    mats.clear();
    for (int k = 0; k < n_listed; ++k) {
        CHECK(check_chain(c, chains[k]));
        const ChainInfo &ci = c->chains[chains[k]];
        mats.push_back(DepMat{c->p.data + ci.off, c->Npad, ci.n});
    }
    return 0;
}

extern "C" int csr_batch_depspan_unique_rows(csr_ctx *c, int32_t n_listed, const int32_t *chains, int32_t *retained,
                                             int32_t *n_retained) {
    std::vector<DepMat> mats;
    CHECK(depspan_batch_mats(c, n_listed, chains, mats));
    if (!retained || !n_retained) return fail("null argument");
    if (c->m > 4096) return fail("depspan: at most 4096 rows");
    CHECK(ctx_select(c));
    DepUnique U{c};
    CHECK(U.begin((int)c->m));
    CHECK(U.add(mats));
    return U.end(retained, n_retained);
}

extern "C" int csr_batch_depspan_window_scores(csr_ctx *c, int32_t n_listed, const int32_t *chains, int32_t n_rows,
                                               const int32_t *rows, int64_t window_bins, double rank_coverage_min, double *score,
                                               int64_t *count) {
    std::vector<DepMat> mats;
    CHECK(depspan_batch_mats(c, n_listed, chains, mats));
    CHECK(depspan_check_rows(c->m, n_rows, rows));
    if (window_bins < 2) return fail("depspan: window_bins must be at least 2");
    if (!score || !count) return fail("null argument");
    CHECK(ctx_select(c));
    const int *dRows;
    CHECK(depspan_upload_rows(c, n_rows, rows, &dRows));
    int64_t at = 0;
    for (const DepMat &mt : mats) {
        if (mt.n < window_bins) continue;
        CHECK(depspan_scores_mat(c, mt, dRows, n_rows, window_bins, rank_coverage_min, score + at, count + at));
        at += mt.n / window_bins;
    }
    return 0;
}

extern "C" int csr_batch_depspan_window_acf(csr_ctx *c, int32_t n_listed, const int32_t *chains, int32_t n_rows, const int32_t *rows,
                                            const csr_depspan_cfg *cfg, int64_t n_windows, const int32_t *win_chain,
                                            const int64_t *win_start, csr_depspan_window *rec, double *pooled) {
    std::vector<DepMat> mats;
    CHECK(depspan_batch_mats(c, n_listed, chains, mats));
    CHECK(depspan_check_rows(c->m, n_rows, rows));
    CHECK(depspan_check_cfg(cfg));
    if (n_windows < 0 || (n_windows > 0 && (!win_chain || !win_start || !rec || !pooled))) return fail("null argument");
    std::vector<DepWin> wins((size_t)n_windows);
    for (int64_t w = 0; w < n_windows; ++w) {
        if (win_chain[w] < 0 || win_chain[w] >= n_listed) return fail("depspan: window %lld names listed chain %d", (long long)w, win_chain[w]);
        const DepMat &mt = mats[win_chain[w]];
        if (win_start[w] < 0 || win_start[w] + cfg->window_bins > mt.n) return fail("depspan: window %lld leaves its chain", (long long)w);
        wins[w] = DepWin{mt.base + win_start[w], mt.stride};
    }
    if (n_windows == 0) return 0;
    CHECK(ctx_select(c));
    const int *dRows;
    CHECK(depspan_upload_rows(c, n_rows, rows, &dRows));
    return depspan_acf_run(c, wins, dRows, n_rows, cfg, rec, pooled);
}
