// csr_host_ess.inl -- part of csr_lib.hip (one translation unit; included in this order): the effective sample size scan of
// pyx:9160-9279 `cEstimateEffectiveSampleSize` from the kernels of csr_ess.h.  The device walks the sums (the mean, the variance sum
// as lag 0, one covariance sum per lag); the host composes cov / pairs, rho, the break / taper rule, tau and the clamps in doubles --
// the same IEEE operations as the reference's C, in its order.  Lags go out in ROUNDS (256 lags of every track, then twice as many
// up to 4096): a track whose scan broke, or reached its last lag, asks for nothing in the next round, so a maxLag of n - 1 costs
// what the reference's scan costs up to its break, rounded up to a round.  A round costs one walk of the longest track whatever
// the number of lags in it, so when every scan of the call ends within 512 lags the first round holds them all (maxLag = 256, four
// dependence spans of 64, would otherwise pay a second walk for its last lag).

constexpr int64_t ESS_ROUND_FIRST = 256, ESS_ROUND_WHOLE = 512, ESS_ROUND_MAX = 4096;

struct EssSpec {
    const double *src = nullptr;            // device: the score track, or the given series
    const unsigned char *mask = nullptr;    // device, or nullptr
    int64_t n = 0;
    int kind = ESS_SERIES_GIVEN, nz = 0;
    double thr[ESS_MAX_Z] = {}, den[ESS_MAX_Z] = {};
    int64_t maxLag = 0;
    bool general = false;                   // the reference's second path (mask, log or window)
    int64_t window = 0;                     // windowIntervals (general path)
    int64_t active = 0;                     // general path: how many values are active
};

// outs[t] of every spec; status[t]: 0, or the index of the reference's late ValueError (1: variance, 2: autocorrelation)
static int ess_run(csr_ctx *c, const std::vector<EssSpec> &specs, csr_ess_out *outs, std::vector<int> &status) {
    const int ns = (int)specs.size();
    status.assign((size_t)ns, 0);
    struct St {
        int spec;
        int64_t count, maxLag, next = 1;    // count: the divisor of mean and variance; next: the first lag not composed yet
        double var = 0.0, tau = 1.0;
        int64_t used = 0;
        bool done = false;
    };
    std::vector<St> st;
    std::vector<EssTrack> tr;
    int64_t total = 0, longest = 0;
    bool anyMask = false;
    for (int s = 0; s < ns; ++s) {
        const EssSpec &sp = specs[s];
        const int64_t count = sp.general ? sp.active : sp.n;
        if (count < 2) {                    // pyx:9184-9185, 9229-9230
            outs[s] = csr_ess_out{(double)count, 1.0, 0};
            continue;
        }
        St x;
        x.spec = s;
        x.count = count;
        x.maxLag = std::max<int64_t>(1, std::min<int64_t>(sp.maxLag, sp.n - 1));
        if (sp.general && sp.window > 0 && sp.window - 1 < x.maxLag) x.maxLag = sp.window - 1;
        EssTrack t{};
        t.src = sp.src;
        t.mask = sp.mask;
        t.n = sp.n;
        t.kind = sp.kind;
        t.nz = sp.nz;
        for (int k = 0; k < ESS_MAX_Z; ++k) { t.thr[k] = sp.thr[k]; t.den[k] = sp.den[k]; }
        t.cen = nullptr;
        t.slot = (int64_t)tr.size() * ESS_ROUND_MAX;
        t.lagEnd = -1;
        total += sp.n;
        longest = std::max(longest, sp.n);
        anyMask = anyMask || sp.mask != nullptr;
        st.push_back(x);
        tr.push_back(t);
    }
    const int nt = (int)tr.size();
    if (nt == 0) return 0;
    csr_ctx::EssWs &ws = c->essWs;
    CHECK(ws.trackBuf.reserve(sizeof(EssTrack) * (size_t)nt));
    CHECK(ws.cenBuf.reserve(8 * (size_t)total));
    CHECK(ws.sumBuf.reserve(8 * (size_t)nt * ESS_ROUND_MAX));
    CHECK(ws.pairBuf.reserve(8 * (size_t)nt * ESS_ROUND_MAX));
    CHECK(ws.outBuf.reserve(8 * (size_t)nt));
    {
        int64_t at = 0;
        for (int t = 0; t < nt; ++t) {
            tr[t].cen = (double *)ws.cenBuf.ptr + at;
            at += tr[t].n;
        }
    }
    const EssTrack *dTr = (const EssTrack *)ws.trackBuf.ptr;
    auto upload_tracks = [&]() -> int {
        HIPOK(hipMemcpyAsync(ws.trackBuf.ptr, tr.data(), sizeof(EssTrack) * (size_t)nt, hipMemcpyHostToDevice, c->stream));
        HIPOK(hipStreamSynchronize(c->stream));     // (tr is reused by the next round)
        return 0;
    };
    const dim3 binGrid((unsigned)((longest + 255) / 256), (unsigned)nt);
    // -- the raw series and its mean
    CHECK(upload_tracks());
    CHECK(launch(c, "ess_series", "k_ess_series", k_ess_series, binGrid, dim3(256), 0, c->stream, dTr, 0));
    CHECK(launch(c, "ess_mean", "k_ess_mean", k_ess_mean, dim3((unsigned)nt), dim3(ESS_WAVE), 0, c->stream, dTr, (double *)ws.outBuf.ptr));
    std::vector<double> sums((size_t)nt);
    HIPOK(hipMemcpyAsync(sums.data(), ws.outBuf.ptr, 8 * (size_t)nt, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    for (int t = 0; t < nt; ++t) tr[t].mean = sums[t] / (double)st[t].count;
    // -- the centred series, then the lags in rounds; lag 0 of the first round is the variance sum
    int64_t lag0 = 0, width = ESS_ROUND_FIRST, widest = 0;
    for (const St &s : st) widest = std::max(widest, s.maxLag + 1);
    widest = (widest + ESS_WAVE - 1) / ESS_WAVE * ESS_WAVE;
    if (widest > width && widest <= ESS_ROUND_WHOLE) width = widest;
    std::vector<long long> pairs;
    bool centred = false;
    for (;;) {
        bool any = false;
        for (int t = 0; t < nt; ++t) {
            tr[t].lagEnd = st[t].done ? -1 : std::min<int64_t>(st[t].maxLag, lag0 + width - 1);
            any = any || !st[t].done;
        }
        if (!any) break;
        CHECK(upload_tracks());
        if (!centred) CHECK(launch(c, "ess_series", "k_ess_series", k_ess_series, binGrid, dim3(256), 0, c->stream, dTr, 1));
        centred = true;
        const dim3 grid((unsigned)(width / ESS_WAVE), (unsigned)nt);
        CHECK(launch(c, "ess_lags", "k_ess_lags", anyMask ? k_ess_lags<true> : k_ess_lags<false>, grid, dim3(ESS_WAVE), 0, c->stream, dTr,
                     lag0, (double *)ws.sumBuf.ptr, (long long *)ws.pairBuf.ptr));
        sums.resize((size_t)nt * ESS_ROUND_MAX);
        pairs.resize((size_t)nt * ESS_ROUND_MAX);
        // (the rows of a round lie ESS_ROUND_MAX apart: one copy of the used part of each array)
        const size_t span = (size_t)(nt - 1) * ESS_ROUND_MAX + (size_t)width;
        HIPOK(hipMemcpyAsync(sums.data(), ws.sumBuf.ptr, 8 * span, hipMemcpyDeviceToHost, c->stream));
        HIPOK(hipMemcpyAsync(pairs.data(), ws.pairBuf.ptr, 8 * span, hipMemcpyDeviceToHost, c->stream));
        HIPOK(hipStreamSynchronize(c->stream));
        for (int t = 0; t < nt; ++t) {
            St &s = st[t];
            if (s.done) continue;
            const EssSpec &sp = specs[s.spec];
            const double *sum = &sums[(size_t)t * ESS_ROUND_MAX];
            const long long *cnt = &pairs[(size_t)t * ESS_ROUND_MAX];
            if (lag0 == 0) {
                s.var = sum[0] / (double)s.count;
                if (!std::isfinite(s.var) && sp.general) {
                    status[s.spec] = 1;
                    s.done = true;
                    continue;
                }
                if (!std::isfinite(s.var) || s.var <= DBL_MIN) {
                    outs[s.spec] = csr_ess_out{(double)s.count, 1.0, 0};
                    s.done = true;
                    continue;
                }
            }
            const int64_t last = std::min<int64_t>(s.maxLag, lag0 + width - 1);
            for (int64_t lag = s.next; lag <= last && !s.done; ++lag) {
                double cov = sum[lag - lag0];
                if (!sp.general) {
                    cov /= (double)std::max<int64_t>(sp.n - lag, 1);
                    const double rho = cov / s.var;
                    if (!std::isfinite(rho) || rho <= 0.0) {
                        s.done = true;
                        break;
                    }
                    s.tau += 2.0 * rho;
                    s.used = lag;
                    continue;
                }
                const long long pc = cnt[lag - lag0];
                if (pc <= 0) continue;
                cov /= (double)pc;
                const double rho = cov / s.var;
                if (!std::isfinite(rho)) {
                    status[s.spec] = 2;
                    s.done = true;
                    break;
                }
                if (sp.window <= 0) {
                    if (rho <= 0.0) {
                        s.done = true;
                        break;
                    }
                    s.tau += 2.0 * rho;
                    s.used = lag;
                } else if (rho > 0.0) {
                    const double taper = 1.0 - ((double)lag / (double)sp.window);
                    if (taper > 0.0) {
                        s.tau += 2.0 * taper * rho;
                        s.used = lag;
                    }
                }
            }
            s.next = last + 1;
            if (last >= s.maxLag) s.done = true;
        }
        lag0 += width;
        width = std::min<int64_t>(2 * width, ESS_ROUND_MAX);
    }
    for (int t = 0; t < nt; ++t) {
        const St &s = st[t];
        if (status[s.spec] != 0) continue;
        if (!(std::isfinite(s.var) && s.var > DBL_MIN)) continue;       // answered above
        const EssSpec &sp = specs[s.spec];
        double tau = s.tau;
        if (tau < 1.0) tau = 1.0;
        if (sp.general && sp.window > 0 && tau > (double)sp.window) tau = (double)sp.window;
        outs[s.spec] = csr_ess_out{(double)s.count / tau, tau, s.used};
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// host arrays (default context).  values: after the caller's log when logPositive; general: the reference's second path
// ---------------------------------------------------------------------------------------------------------------
extern "C" int csr_ess_scan(const double *values, int64_t n, int64_t max_lag, const unsigned char *active_mask, int32_t general,
                            int64_t window_intervals, csr_ess_out *out) {
    DEFAULT_CTX_GUARD;
    if (!out || (n > 0 && !values) || n < 0) return fail("null argument");
    if (window_intervals < 0) return value_error("windowIntervals must be nonnegative");
    const bool gen = general != 0 || active_mask != nullptr || window_intervals != 0;
    int64_t active = 0;
    if (gen)
        for (int64_t i = 0; i < n; ++i) {
            if (active_mask && active_mask[i] == 0) continue;
            if (!std::isfinite(values[i])) return value_error("active values must be finite");
            ++active;
        }
    if ((gen ? active : n) < 2) {
        *out = csr_ess_out{(double)(gen ? active : n), 1.0, 0};
        return 0;
    }
    csr_ctx *c = nullptr;
    CHECK(ctx_or_default(c));
    csr_ctx::EssWs &ws = c->essWs;
    EssSpec sp;
    CHECK(stage_vector(c, ws.xBuf, values, n, &sp.src));
    if (active_mask) {
        CHECK(ws.maskBuf.reserve((size_t)n));
        HIPOK(hipMemcpyAsync(ws.maskBuf.ptr, active_mask, (size_t)n, hipMemcpyHostToDevice, c->stream));
    }
    sp.mask = active_mask ? (const unsigned char *)ws.maskBuf.ptr : nullptr;
    sp.n = n;
    sp.maxLag = max_lag;
    sp.general = gen;
    sp.window = window_intervals;
    sp.active = active;
    std::vector<int> status;
    CHECK(ess_run(c, {sp}, out, status));
    if (status[0] == 1) return value_error("variance estimate must be finite");
    if (status[0] == 2) return value_error("autocorrelation estimate must be finite");
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// batch context: what `estimateROCCOGamma` (peaks.py:1741-1751) needs of a resident score track -- how many scores exceed the
// reference level (score - level > 0) and the one or two middle order statistics of those.  The track is sorted with the null's
// sort; score - level is monotone along the sorted track, so the positive ones are its tail and their median lies at known ranks.
// mid[2 chain], mid[2 chain + 1]: the lower and upper middle SCORES (equal when the count is odd; untouched when it is 0)
// ---------------------------------------------------------------------------------------------------------------
extern "C" int csr_batch_rocco_excess_ranks(csr_ctx *c, const double *levels, const unsigned char *chain_mask, int64_t *count,
                                            double *mid) {
    CHECK(need(c));
    if (!levels || !count || !mid) return fail("null argument");
    std::vector<int> idx;
    const int missing = select_chains(c, chain_mask, c->scores, idx, NO_SCORES);
    std::vector<NullTrackHost> tracks;
    for (int i : idx) {         // (the chains in front of one without scores still answer for their own level first)
        if (!std::isfinite(levels[i])) return fail("chain %d: the reference level must be finite", i);
        tracks.push_back(NullTrackHost{c->scores.at(c, i), c->chains[i].n, nullptr, false, 0.0, 0.0});
    }
    CHECK(missing);
    if (tracks.empty()) return 0;
    NullEngine E;
    E.c = c;
    CHECK(E.setup(tracks, false));
    CHECK(E.sort());
    std::vector<NullQuery> qs;
    for (size_t k = 0; k < idx.size(); ++k)
        qs.push_back(NullQuery{E.sorted + E.tr[k].slot, tracks[k].n, levels[idx[k]], 0.0, 0, 0});     // how many (x - level) <= 0
    std::vector<long long> below;
    CHECK(E.search(qs, below));
    std::vector<const double *> gp;
    for (size_t k = 0; k < idx.size(); ++k) {
        const int64_t L = tracks[k].n - below[k];
        count[idx[k]] = L;
        if (L <= 0) continue;
        int64_t lo, hi;
        null_median_ranks(L, lo, hi);
        gp.push_back(E.sorted + E.tr[k].slot + below[k] + lo);
        gp.push_back(E.sorted + E.tr[k].slot + below[k] + hi);
    }
    std::vector<double> gv;
    CHECK(E.gather(gp, gv));
    for (size_t k = 0, g = 0; k < idx.size(); ++k) {
        if (count[idx[k]] <= 0) continue;
        mid[2 * idx[k]] = gv[g++];
        mid[2 * idx[k] + 1] = gv[g++];
    }
    return 0;
}

// the mask of one chain as the caller decided it (the contiguous-window fallback of `solveChromROCCO`, peaks.py:1812-1835): from
// then on csr_batch_rocco_download / csr_batch_rocco_runs serve it like a mask the solver left
extern "C" int csr_batch_rocco_upload(csr_ctx *c, int32_t chain, const unsigned char *solution) {
    CHECK(need_chain(c, chain, solution));
    if (!c->sol.d) return fail("no ROCCO solution buffers: call csr_batch_rocco first");
    for (int64_t i = 0; i < c->chains[chain].n; ++i)
        if (solution[i] > 1) return fail("a selection mask holds 0 and 1 only");
    return c->sol.upload(c, chain, solution);
}

// ---------------------------------------------------------------------------------------------------------------
// batch context: the series of peaks.py:1414-1434 from the RESIDENT score tracks, scanned on the reference's fast path (the only
// one the budget policy takes); thresholds / scales: [chain][n_z]; no resident array changes
// ---------------------------------------------------------------------------------------------------------------
extern "C" int csr_batch_ess(csr_ctx *c, int32_t kind, int32_t n_z, const double *thresholds, const double *scales,
                             const int64_t *max_lags, const unsigned char *chain_mask, csr_ess_out *out) {
    CHECK(need(c));
    if (!thresholds || !scales || !max_lags || !out) return fail("null argument");
    if (kind != ESS_SERIES_OCCUPANCY && kind != ESS_SERIES_SOFT && kind != ESS_SERIES_INTEGRATED) return fail("bad series kind %d", kind);
    if (n_z < 1 || n_z > ESS_MAX_Z) return fail("n_z must be in [1, %d]", ESS_MAX_Z);
    std::vector<int> idx;
    CHECK(select_chains(c, chain_mask, c->scores, idx, NO_SCORES));
    std::vector<EssSpec> specs;
    for (int i : idx) {
        EssSpec sp;
        sp.src = c->scores.at(c, i);
        sp.n = c->chains[i].n;
        sp.kind = kind;
        sp.nz = n_z;
        for (int k = 0; k < n_z; ++k) {
            sp.thr[k] = thresholds[(size_t)i * n_z + k];
            sp.den[k] = std::max(scales[(size_t)i * n_z + k], DBL_MIN);
        }
        sp.maxLag = max_lags[i];
        specs.push_back(sp);
    }
    if (specs.empty()) return 0;
    std::vector<csr_ess_out> res(specs.size());
    std::vector<int> status;
    CHECK(ess_run(c, specs, res.data(), status));
    scatter_chains(idx, res.data(), out);
    return 0;
}
