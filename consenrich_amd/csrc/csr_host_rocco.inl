// csr_host_rocco.inl -- part of csr_lib.hip (one translation unit; included in this order): budgeted chain peak selection
// (ROCCO) -- the calibration loop of pyx:8743-8844 driven from the host over the lanes of csr_rocco.h, on host arrays
// (default context) and on a batch context's resident scores.

// ---------------------------------------------------------------------------------------------------------------
// the engine: any number of chains of one concatenated device array, every chain at its own stage of the calibration
// ---------------------------------------------------------------------------------------------------------------
struct RoccoChainIn {
    int64_t off, n;                 // bins [off, off + n) of the device arrays; off is a multiple of 64
    double gamma;                   // constant switch cost (no cost array)
    const double *hostCosts;        // n - 1 switch costs on the host (for switchSum), or nullptr
    csr_rocco_cfg cfg;
    csr_rocco_out *out;
};
struct RoccoDev {
    const double *scores;
    const double *costs;            // device copy of the switch costs (same offsets), or nullptr = constant gamma
    unsigned char *sol;
    unsigned long long *bt;         // one 64-bit word per 32 bins of the concatenated layout
};

static int rocco_depth(const csr_ctx *c) { return c->roccoWs.depth > 0 ? c->roccoWs.depth : 6; }

static int rocco_run(csr_ctx *c, const RoccoDev &dv, std::vector<RoccoChainIn> &chains) {
    const int nc = (int)chains.size();
    if (nc == 0) return 0;
    const int D = rocco_depth(c);
    const int maxPen = (1 << D) - 1, jobsPer = (maxPen + 63) / 64;
    enum { INIT, EXPAND, BISECT, FINAL, DONE };
    struct St {
        int phase = INIT;
        int64_t target = 0;
        double lower = 0, upper = 0, bestVal = 0, finalPen = 0;
        int64_t lowerCount = 0, bestCount = 0;
        bool growLower = false, growUpper = false;
        int itersLeft = 0, depth = 0, grown = 0;
        int penOff = 0, nPen = 0;
        double mid[(1 << ROCCO_MAX_DEPTH) - 1];
    };
    std::vector<St> st((size_t)nc);
    // work space: jobs | penalties | results | (min, max) per chain
    const size_t nJobs = (size_t)nc * jobsPer, nPen = (size_t)nc * maxPen + 2 * (size_t)nc;
    const size_t oJob = 0, oPen = (nJobs * sizeof(RoccoJob) + 255) / 256 * 256, oRes = oPen + (nPen * 8 + 255) / 256 * 256,
                 oMm = oRes + (nPen * sizeof(RoccoRes) + 255) / 256 * 256, total = oMm + 16 * (size_t)nc;
    CHECK(c->roccoWs.work.reserve(total));
    char *base = (char *)c->roccoWs.work.ptr;
    RoccoJob *dJobs = (RoccoJob *)(base + oJob);
    double *dPen = (double *)(base + oPen);
    RoccoRes *dRes = (RoccoRes *)(base + oRes);
    double *dMm = (double *)(base + oMm);
    std::vector<RoccoJob> jobs;
    std::vector<double> pen(nPen);
    std::vector<RoccoRes> res(nPen);
    csr_rocco_stats &rs = c->roccoWs.stats;
    rs.depth = D;

    // which chains calibrate: clamp the target; target == n is one solve at penalty 0 (pyx:8773-8785)
    std::vector<int> cal;
    for (int i = 0; i < nc; ++i) {
        RoccoChainIn &ch = chains[i];
        St &s = st[i];
        if (ch.cfg.mode == CSR_ROCCO_FIXED_PENALTY) {
            s.phase = FINAL;
            s.finalPen = ch.cfg.penalty;
            continue;
        }
        int64_t tg = ch.cfg.target_count;
        tg = tg < 0 ? 0 : (tg > ch.n ? ch.n : tg);
        s.target = tg;
        if (tg == ch.n) {
            s.phase = FINAL;
            s.finalPen = 0.0;
            continue;
        }
        s.itersLeft = ch.cfg.max_iter > 1 ? ch.cfg.max_iter : 1;
        cal.push_back(i);
    }
    if (!cal.empty()) {
        jobs.clear();
        for (int i : cal) jobs.push_back(RoccoJob{chains[i].off, chains[i].n, 0.0, 0, 0});
        HIPOK(hipMemcpyAsync(dJobs, jobs.data(), jobs.size() * sizeof(RoccoJob), hipMemcpyHostToDevice, c->stream));
        CHECK(launch(c, "rocco_minmax", "k_rocco_minmax", k_rocco_minmax, dim3((unsigned)jobs.size()), dim3(256), 0, c->stream, dJobs,
                     dv.scores, dMm));
        std::vector<double> mm(2 * cal.size());
        HIPOK(hipMemcpyAsync(mm.data(), dMm, 16 * cal.size(), hipMemcpyDeviceToHost, c->stream));
        // switchSum: the reference's SEQUENTIAL float64 sum of the n - 1 costs (pyx:8794-8795), here while the reduction runs
        std::vector<double> sw(cal.size(), 0.0);
        for (size_t k = 0; k < cal.size(); ++k) {
            const RoccoChainIn &ch = chains[cal[k]];
            volatile double acc = 0.0;      // (no vectorised re-association by the host compiler)
            if (ch.hostCosts)
                for (int64_t i = 0; i + 1 < ch.n; ++i) acc = acc + ch.hostCosts[i];
            else
                for (int64_t i = 0; i + 1 < ch.n; ++i) acc = acc + ch.gamma;
            sw[k] = acc;
        }
        HIPOK(hipStreamSynchronize(c->stream));
        ++rs.launches;
        for (size_t k = 0; k < cal.size(); ++k) {
            St &s = st[cal[k]];
            s.lower = mm[2 * k] - sw[k] - 1.0;
            s.upper = mm[2 * k + 1] + sw[k] + 1.0;
        }
    }

    for (;;) {
        // ---- assemble this round's lanes
        jobs.clear();
        size_t np = 0, nCountJobs = 0;
        std::vector<RoccoJob> btJobs;
        for (int i = 0; i < nc; ++i) {
            St &s = st[i];
            const RoccoChainIn &ch = chains[i];
            if (s.phase == DONE) continue;
            s.penOff = (int)np;
            if (s.phase == FINAL) {
                s.nPen = 1;
                pen[np++] = s.finalPen;
                btJobs.push_back(RoccoJob{ch.off, ch.n, ch.gamma, s.penOff, 1});
                continue;
            }
            if (s.phase == INIT) {
                // solve(lower) and solve(upper) are independent of each other: two lanes of one walk
                pen[np++] = s.lower;
                pen[np++] = s.upper;
                s.nPen = 2;
            } else if (s.phase == EXPAND) {
                s.nPen = 0;
                if (s.growLower) { pen[np++] = s.lower; ++s.nPen; }
                if (s.growUpper) { pen[np++] = s.upper; ++s.nPen; }
            } else {
                // the midpoints the next `depth` bisection steps can visit, as a heap: node k's children are 2k+1 (its count
                // exceeded the target: lower = midpoint) and 2k+2 (upper = midpoint); same expression as pyx:8827
                s.depth = s.itersLeft < D ? s.itersLeft : D;
                const int nodes = (1 << s.depth) - 1;
                double lo[(1 << ROCCO_MAX_DEPTH) - 1], up[(1 << ROCCO_MAX_DEPTH) - 1];
                lo[0] = s.lower;
                up[0] = s.upper;
                for (int k = 0; k < nodes; ++k) {
                    const double mid = (lo[k] + up[k]) / 2.0;
                    s.mid[k] = mid;
                    if (2 * k + 2 < nodes) {
                        lo[2 * k + 1] = mid; up[2 * k + 1] = up[k];
                        lo[2 * k + 2] = lo[k]; up[2 * k + 2] = mid;
                    }
                    pen[np++] = mid;
                }
                s.nPen = nodes;
            }
            for (int k = 0; k < s.nPen; k += 64)
                jobs.push_back(RoccoJob{ch.off, ch.n, ch.gamma, s.penOff + k, s.nPen - k < 64 ? s.nPen - k : 64});
        }
        if (np == 0) break;
        nCountJobs = jobs.size();
        jobs.insert(jobs.end(), btJobs.begin(), btJobs.end());
        HIPOK(hipMemcpyAsync(dJobs, jobs.data(), jobs.size() * sizeof(RoccoJob), hipMemcpyHostToDevice, c->stream));
        HIPOK(hipMemcpyAsync(dPen, pen.data(), np * 8, hipMemcpyHostToDevice, c->stream));
        rs.h2d_bytes += (int64_t)(jobs.size() * sizeof(RoccoJob) + np * 8);
        // (the first template argument: the costs are derived from the scores, there is no cost track)
        if (nCountJobs) {
            CHECK(launch(c, "rocco_count", "k_rocco_chain (count)", dv.costs ? &k_rocco_chain<false, false> : &k_rocco_chain<true, false>,
                         dim3((unsigned)nCountJobs), dim3(64), 0, c->stream, dJobs, dv.scores, dv.costs, dPen, dRes, dv.bt, dv.sol));
            ++rs.launches;
        }
        if (!btJobs.empty()) {
            CHECK(launch(c, "rocco_backtrace", "k_rocco_chain (backtrace)", dv.costs ? &k_rocco_chain<false, true> : &k_rocco_chain<true, true>,
                         dim3((unsigned)btJobs.size()), dim3(64), 0, c->stream, dJobs + nCountJobs, dv.scores, dv.costs, dPen, dRes, dv.bt,
                         dv.sol));
            ++rs.launches;
        }
        HIPOK(hipMemcpyAsync(res.data(), dRes, np * sizeof(RoccoRes), hipMemcpyDeviceToHost, c->stream));
        HIPOK(hipStreamSynchronize(c->stream));
        rs.d2h_bytes += (int64_t)(np * sizeof(RoccoRes));
        ++rs.rounds;
        // ---- advance every chain exactly as the sequential loop would
        for (int i = 0; i < nc; ++i) {
            St &s = st[i];
            RoccoChainIn &ch = chains[i];
            if (s.phase == DONE) continue;
            const RoccoRes *r = &res[(size_t)s.penOff];
            rs.lane_steps += (int64_t)s.nPen * ch.n;
            if (s.phase == FINAL) {
                ch.out->selection_penalty = s.finalPen;
                ch.out->penalized_objective = r[0].val;
                ch.out->objective = r[0].objective;
                ch.out->selected_count = r[0].count;
                s.phase = DONE;
                continue;
            }
            if (s.phase == INIT || s.phase == EXPAND) {
                int k = 0;
                if (s.phase == INIT || s.growLower) s.lowerCount = r[k++].count;
                if (s.phase == INIT || s.growUpper) { s.bestVal = r[k].val; s.bestCount = r[k].count; ++k; }
                // pyx:8805-8824 (the two loops do not depend on each other: they advance side by side)
                s.growLower = s.lowerCount <= s.target;
                s.growUpper = s.bestCount > s.target;
                if (s.growLower) s.lower -= std::fmax(1.0, std::fabs(s.lower));
                if (s.growUpper) s.upper += std::fmax(1.0, std::fabs(s.upper));
                if (s.growLower || s.growUpper) {
                    if (++s.grown > 2200) return fail("ROCCO calibration: the penalty bracket does not close (chain of %lld bins)", (long long)ch.n);
                    s.phase = EXPAND;
                } else
                    s.phase = BISECT;
                continue;
            }
            // BISECT: walk `depth` levels with the counts, pyx:8833-8842
            int k = 0;
            for (int lv = 0; lv < s.depth; ++lv) {
                if (r[k].count > s.target) {
                    s.lower = s.mid[k];
                    k = 2 * k + 1;
                } else {
                    s.upper = s.mid[k];
                    s.bestVal = r[k].val;
                    s.bestCount = r[k].count;
                    k = 2 * k + 2;
                }
            }
            s.itersLeft -= s.depth;
            if (s.itersLeft <= 0) {
                s.phase = FINAL;        // the returned solution is solve(upper): re-solved with its backtrace
                s.finalPen = s.upper;
            }
        }
    }
    return 0;
}

static int rocco_check_cfg(const csr_rocco_cfg &g, int i, bool needGamma) {
    if (g.mode != CSR_ROCCO_FIXED_PENALTY && g.mode != CSR_ROCCO_TARGET_COUNT) return fail("chain %d: bad ROCCO mode %d", i, g.mode);
    if (needGamma && (!std::isfinite(g.gamma) || g.gamma < 0.0)) return fail("chain %d: `gamma` must be finite and non-negative", i);
    return 0;
}

extern "C" int csr_set_rocco_depth(csr_ctx *c, int32_t depth) {
    if (!c) c = default_ctx();      // NULL addresses the default context of the host-buffer entry points
    if (!c) return -1;
    if (depth < 0 || depth > ROCCO_MAX_DEPTH) return fail("ROCCO speculation depth must be in 0..%d", ROCCO_MAX_DEPTH);
    c->roccoWs.depth = depth;
    return 0;
}
extern "C" int csr_get_rocco_stats(csr_ctx *c, csr_rocco_stats *out) {
    if (!c) c = default_ctx();
    if (!c || !out) return fail("null argument");
    *out = c->roccoWs.stats;
    out->depth = rocco_depth(c);
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// host arrays (default context)
// ---------------------------------------------------------------------------------------------------------------
extern "C" int csr_rocco_solve(int32_t n_chains, const int64_t *chain_len, const double *scores, const double *switch_costs,
                               const csr_rocco_cfg *cfg, csr_rocco_out *out, uint8_t *solution) {
    DEFAULT_CTX_GUARD;
    if (n_chains <= 0 || !chain_len || !scores || !cfg || !out) return fail("null or empty argument");
    csr_ctx *c = nullptr;
    CHECK(ctx_or_default(c));
    int64_t tot = 0, pad = 0;
    std::vector<RoccoChainIn> chains((size_t)n_chains);
    for (int i = 0; i < n_chains; ++i) {
        if (chain_len[i] <= 0) return fail("`scores` cannot be empty (chain %d)", i);
        CHECK(rocco_check_cfg(cfg[i], i, switch_costs == nullptr));
        chains[i] = RoccoChainIn{pad, chain_len[i], switch_costs ? 0.0 : cfg[i].gamma, nullptr, cfg[i], &out[i]};
        tot += chain_len[i];
        pad += (chain_len[i] + 63) / 64 * 64;
    }
    if (pad >= (int64_t)1 << 31) return fail("too many bins: %lld (limit 2^31)", (long long)pad);
    CHECK(check_finite("scores", scores, tot));
    // device arena: scores | costs | mask | backtrace words
    const size_t oS = 0, oC = oS + 8 * (size_t)pad, oSol = oC + (switch_costs ? 8 * (size_t)pad : 0), oBt = oSol + (size_t)pad,
                 total = oBt + (size_t)pad / 4 + 64;
    CHECK(c->roccoWs.arena.reserve(total));
    char *base = (char *)c->roccoWs.arena.ptr;
    RoccoDev dv{(const double *)(base + oS), switch_costs ? (const double *)(base + oC) : nullptr, (unsigned char *)(base + oSol),
                (unsigned long long *)(base + oBt)};
    int64_t so = 0, co = 0;
    for (int i = 0; i < n_chains; ++i) {
        RoccoChainIn &ch = chains[i];
        HIPOK(hipMemcpyAsync(base + oS + 8 * ch.off, scores + so, 8 * (size_t)ch.n, hipMemcpyHostToDevice, c->stream));
        if (switch_costs) {
            ch.hostCosts = switch_costs + co;
            CHECK(check_finite("switchCosts", ch.hostCosts, ch.n - 1));
            if (ch.n > 1)
                HIPOK(hipMemcpyAsync(base + oC + 8 * ch.off, ch.hostCosts, 8 * (size_t)(ch.n - 1), hipMemcpyHostToDevice, c->stream));
            co += ch.n - 1;
        }
        so += ch.n;
    }
    c->roccoWs.stats.h2d_bytes += 8 * tot + (switch_costs ? 8 * (tot - n_chains) : 0);
    CHECK(rocco_run(c, dv, chains));
    if (solution) {
        so = 0;
        for (int i = 0; i < n_chains; ++i) {
            HIPOK(hipMemcpyAsync(solution + so, dv.sol + chains[i].off, (size_t)chains[i].n, hipMemcpyDeviceToHost, c->stream));
            so += chains[i].n;
        }
        HIPOK(hipStreamSynchronize(c->stream));
        c->roccoWs.stats.d2h_bytes += tot;
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// batch context: scores, masks and work space of their own (allocated at first use, freed with the batch); the resident
// arrays of the fit and the record of its last pass are only read
// ---------------------------------------------------------------------------------------------------------------
static int rocco_buffers(csr_ctx *c) {
    CHECK(c->scores.ensure(c));
    CHECK(c->sol.ensure(c));
    csr_ctx::Rocco &r = c->rocco;
    if (r.bt) return 0;
    const int64_t nc = (int64_t)c->chains.size();
    CHECK(dalloc(c, &r.bt, c->Npad / 32 + 64));
    CHECK(dalloc(c, &r.mx, nc));
    CHECK(dalloc(c, &r.bad, nc));
    return 0;
}

extern "C" int csr_batch_upload_scores(csr_ctx *c, int32_t chain, const double *scores) {
    CHECK(need_chain(c, chain, scores));
    CHECK(check_finite("scores", scores, c->chains[chain].n));
    CHECK(rocco_buffers(c));
    CHECK(c->scores.upload(c, chain, scores));
    scores_changed(c, chain);
    return 0;
}

extern "C" int csr_batch_rocco_scores(csr_ctx *c, int32_t mode, double z) {
    CHECK(need(c));
    CHECK(settle(c));
    if (mode != CSR_ROCCO_SCORE_STATE && mode != CSR_ROCCO_SCORE_LOWER_CONFIDENCE) return fail("bad score mode %d", mode);
    if (mode == CSR_ROCCO_SCORE_LOWER_CONFIDENCE && (!std::isfinite(z) || z < 0.0))
        return value_error("`uncertaintyScoreZ` must be finite and non-negative");
    if (!c->haveBwd) return fail("no smoothed results to score");
    // the scores are built from the reference-layout copies of xs / Ps: the conversion csr_batch_export(CSR_EXPORT_SMOOTH) makes,
    // a no-op when those copies are current; values and blocked copies stay what they are
    CHECK(export_impl(c, CSR_EXPORT_SMOOTH));
    CHECK(rocco_buffers(c));
    const int nc = (int)c->chains.size();
    csr_ctx::Rocco &r = c->rocco;
    std::vector<double> mx((size_t)nc, -INFINITY);
    HIPOK(hipMemcpyAsync(r.mx, mx.data(), 8 * (size_t)nc, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemsetAsync(r.bad, 0, 4 * (size_t)nc, c->stream));
    RoccoScoreArgs a;
    memset(&a, 0, sizeof(a));
    a.xs = c->nat[CSR_ARR_XS]; a.Ps = c->nat[CSR_ARR_PS]; a.d = c->mdl.state_dim;
    a.lower = mode == CSR_ROCCO_SCORE_LOWER_CONFIDENCE; a.z = z;
    a.off = c->dChainOff; a.len = c->dChainLen; a.active = nullptr;
    a.scores = c->scores.d; a.mx = r.mx; a.bad = r.bad;
    int64_t longest = 0;
    for (const ChainInfo &ci : c->chains) longest = std::max(longest, ci.n);
    const dim3 grid((unsigned)std::min<int64_t>((longest + 255) / 256, 1024), (unsigned)nc);
    {
        Scope sc(c, "rocco_scores");
        CHECK(launch(c, nullptr, "k_rocco_scores", k_rocco_scores, grid, dim3(256), 0, c->stream, a));
        if (a.lower) CHECK(launch(c, nullptr, "k_rocco_floor", k_rocco_floor, grid, dim3(256), 0, c->stream, a));
    }
    std::vector<int> bad((size_t)nc, 0);
    HIPOK(hipMemcpyAsync(bad.data(), r.bad, 4 * (size_t)nc, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    c->scores.clear_all();
    for (int i = 0; i < nc; ++i) scores_changed(c, i);
    for (int i = 0; i < nc; ++i)
        if (bad[i]) return value_error("`uncertainty` must be non-negative for lower_confidence (chain %d)", i);
    for (int i = 0; i < nc; ++i) c->scores.set(i, true);
    return 0;
}

extern "C" int csr_batch_download_scores(csr_ctx *c, int32_t chain, double *host_dst) {
    CHECK(need_chain(c, chain, host_dst));
    return c->scores.download(c, chain, host_dst);
}

extern "C" int csr_batch_rocco(csr_ctx *c, const csr_rocco_cfg *cfg, const unsigned char *chain_mask, csr_rocco_out *out) {
    CHECK(need(c));
    if (!cfg || !out) return fail("null argument");
    std::vector<int> idx;
    const int missing = select_chains(c, chain_mask, c->scores, idx, NO_SCORES);
    std::vector<RoccoChainIn> chains;
    for (int i : idx) {         // (the chains in front of one without scores still answer for their own arguments first)
        CHECK(rocco_check_cfg(cfg[i], i, true));
        chains.push_back(RoccoChainIn{c->chains[i].off, c->chains[i].n, cfg[i].gamma, nullptr, cfg[i], &out[i]});
    }
    CHECK(missing);
    RoccoDev dv{c->scores.d, nullptr, c->sol.d, c->rocco.bt};
    for (int i : idx) c->sol.set(i, false);
    CHECK(rocco_run(c, dv, chains));
    for (int i : idx) c->sol.set(i, true);
    return 0;
}

extern "C" int csr_batch_rocco_download(csr_ctx *c, int32_t chain, uint8_t *solution) {
    CHECK(need_chain(c, chain, solution));
    CHECK(c->sol.download(c, chain, solution));
    c->roccoWs.stats.d2h_bytes += c->chains[chain].n;
    return 0;
}

// Run bounds of a chain's mask.  *count receives the number of runs; starts / ends receive the first `capacity` of them (both
// may be NULL with capacity 0: count only).
extern "C" int csr_batch_rocco_runs(csr_ctx *c, int32_t chain, int32_t max_gap_bins, int64_t capacity, int64_t *count,
                                    int64_t *starts, int64_t *ends) {
    CHECK(need(c));
    CHECK(check_chain(c, chain));
    if (!count) return fail("null argument");
    if (capacity < 0 || (capacity > 0 && (!starts || !ends))) return fail("bad capacity / output buffers");
    if (!c->sol.has(chain)) return fail("chain %d has no ROCCO solution", chain);
    const ChainInfo &ci = c->chains[chain];
    const int64_t nb = (ci.n + 1023) / 1024;
    const size_t oB = 0, oS = (8 * (size_t)(nb + 1) + 255) / 256 * 256, oE = oS + (8 * (size_t)capacity + 255) / 256 * 256,
                 total = oE + 8 * (size_t)capacity + 256;
    CHECK(c->roccoWs.runBuf.reserve(total));
    char *base = (char *)c->roccoWs.runBuf.ptr;
    RoccoRunArgs a;
    a.sol = c->sol.at(c, chain);
    a.n = ci.n;
    a.gap = std::min<int64_t>(max_gap_bins > 0 ? max_gap_bins : 0, ci.n);
    a.blockSum = (unsigned long long *)(base + oB);
    a.starts = (int64_t *)(base + oS);
    a.ends = (int64_t *)(base + oE);
    a.capacity = capacity;
    {
        Scope sc(c, "rocco_runs");
        CHECK(launch(c, nullptr, "k_rocco_run_count", k_rocco_run_count, dim3((unsigned)nb), dim3(1024), 0, c->stream, a));
        CHECK(launch(c, nullptr, "k_rocco_run_scan", k_rocco_run_scan, dim3(1), dim3(1024), 0, c->stream, a, nb));
        if (capacity > 0) CHECK(launch(c, nullptr, "k_rocco_run_write", k_rocco_run_write, dim3((unsigned)nb), dim3(1024), 0, c->stream, a));
    }
    unsigned long long tot = 0;
    HIPOK(hipMemcpyAsync(&tot, a.blockSum + nb, 8, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    const int64_t ns = (int64_t)(tot & 0xffffffffull), ne = (int64_t)(tot >> 32);
    if (ns != ne) return fail("run bounds: %lld starts but %lld ends", (long long)ns, (long long)ne);
    *count = ns;
    const int64_t take = std::min(ns, capacity);
    if (take > 0) {
        HIPOK(hipMemcpyAsync(starts, a.starts, 8 * (size_t)take, hipMemcpyDeviceToHost, c->stream));
        HIPOK(hipMemcpyAsync(ends, a.ends, 8 * (size_t)take, hipMemcpyDeviceToHost, c->stream));
        HIPOK(hipStreamSynchronize(c->stream));
    }
    return 0;
}
