// csr_host_shrink.inl -- part of csr_lib.hip (one translation unit; included in this order): the per-bin passes of the post-fit
// empirical-Bayes state shrinkage from the kernels of csr_shrink.h -- the reference's three natives (pyx:9791-10269).  The EM
// control flow around them (`fitStateShrinkagePrior`) is scalar work and lives in consenrich_amd/shrink.py; this file evaluates
// one pass for one parameter set and returns the sums CHAIN BY CHAIN, which the caller adds in chain order as the reference adds
// its chunks.
//
// An input is prepared once per (input, block size) and then read by any number of passes:
//   csr_shrink_stage            host arrays (float64 state / variance, the chunks one after the other) into the default context;
//   csr_batch_shrink_prepare    the chains a mask takes of a resident fit: (double) xs[:,0] of the reference-layout copy and a
//                               float32 variance track made on the device.
// Both leave the per-block valid counts.  Every argument is checked before any launch.

static int shrink_check_prior(double pi0, int32_t K, const double *tau, const double *lsp) {
    if (K < 1 || K > SHRINK_MAX_K) return value_error("slab arrays must hold 1 to %d slabs", SHRINK_MAX_K);
    if (!tau || !lsp) return fail("null argument");
    if (!std::isfinite(pi0) || pi0 <= 0.0 || pi0 >= 1.0) return value_error("priorSpikeProp must be finite with 0 < priorSpikeProp < 1");
    for (int j = 0; j < K; ++j)
        if (!std::isfinite(tau[j]) || tau[j] <= 0.0) return value_error("slabVariance must contain only positive finite values");
    return 0;
}

static int shrink_upload_prior(csr_ctx *c, double pi0, int32_t K, const double *tau, const double *lsp, const ShrinkPrior **dev) {
    csr_ctx::ShrinkWs &ws = c->shrinkWs;
    ShrinkPrior p;
    memset(&p, 0, sizeof(p));
    p.logNullPrior = std::log(pi0);
    p.K = K;
    for (int j = 0; j < K; ++j) { p.tau[j] = tau[j]; p.logPrior[j] = lsp[j]; }
    CHECK(ws.priorBuf.reserve(sizeof(ShrinkPrior)));
    HIPOK(hipMemcpyAsync(ws.priorBuf.ptr, &p, sizeof(p), hipMemcpyHostToDevice, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));     // (p is a local)
    *dev = (const ShrinkPrior *)ws.priorBuf.ptr;
    return 0;
}

// the chain table of a prepared input: block and tile offsets, uploaded; counts zeroed
static int shrink_tables(csr_ctx *c, int64_t block) {
    csr_ctx::ShrinkWs &ws = c->shrinkWs;
    ws.block = block;
    ws.longest = ws.nTiles = ws.nBlocks = 0;
    for (ShrinkChain &ch : ws.chains) {
        ch.blk0 = ws.nBlocks;
        ch.tile0 = ws.nTiles;
        ws.nBlocks += (ch.n + block - 1) / block;
        ws.nTiles += (ch.n + SHRINK_TILE - 1) / SHRINK_TILE;
        ws.longest = std::max(ws.longest, ch.n);
    }
    const size_t nc = ws.chains.size();
    CHECK(ws.chainBuf.reserve(sizeof(ShrinkChain) * std::max<size_t>(nc, 1)));
    CHECK(ws.cntBuf.reserve(4 * (size_t)std::max<int64_t>(ws.nBlocks, 1)));
    if (nc) HIPOK(hipMemcpyAsync(ws.chainBuf.ptr, ws.chains.data(), sizeof(ShrinkChain) * nc, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemsetAsync(ws.cntBuf.ptr, 0, 4 * (size_t)std::max<int64_t>(ws.nBlocks, 1), c->stream));
    return 0;
}
static dim3 shrink_grid(const csr_ctx::ShrinkWs &ws) {
    return dim3((unsigned)std::max<int64_t>((ws.longest + SHRINK_TILE - 1) / SHRINK_TILE, 1), (unsigned)ws.chains.size());
}

extern "C" int csr_shrink_stage(int32_t n_chunks, const int64_t *lens, const double *state, const double *variance, int64_t block) {
    DEFAULT_CTX_GUARD;
    if (n_chunks < 0 || (n_chunks > 0 && !lens)) return fail("null argument");
    if (block < 1) return fail("block must be at least 1");
    int64_t total = 0;
    for (int i = 0; i < n_chunks; ++i) {
        if (lens[i] < 0) return fail("negative chunk length");
        total += lens[i];
    }
    if (total > 0 && (!state || !variance)) return fail("null argument");
    csr_ctx *c = nullptr;
    CHECK(ctx_or_default(c));
    csr_ctx::ShrinkWs &ws = c->shrinkWs;
    ws.ready = false;
    ws.fromBatch = false;
    ws.chains.clear();
    ws.idx.clear();
    int64_t off = 0;
    for (int i = 0; i < n_chunks; ++i) {
        ws.chains.push_back(ShrinkChain{off, lens[i], 0, 0});
        ws.idx.push_back(i);
        off += lens[i];
    }
    ws.total = total;
    ws.nOut = n_chunks;
    ws.tr = ShrinkTrack{nullptr, nullptr, nullptr, nullptr, 1};
    const size_t bytes = 8 * (size_t)std::max<int64_t>(total, 1);
    CHECK(ws.xBuf.reserve(bytes));
    CHECK(ws.vBuf.reserve(bytes));
    if (total > 0) {
        HIPOK(hipMemcpyAsync(ws.xBuf.ptr, state, 8 * (size_t)total, hipMemcpyHostToDevice, c->stream));
        HIPOK(hipMemcpyAsync(ws.vBuf.ptr, variance, 8 * (size_t)total, hipMemcpyHostToDevice, c->stream));
    }
    ws.tr.xd = (const double *)ws.xBuf.ptr;
    ws.tr.vd = (const double *)ws.vBuf.ptr;
    CHECK(shrink_tables(c, block));
    if (total > 0) {
        ShrinkPrepArgs a;
        memset(&a, 0, sizeof(a));
        a.tr = ws.tr;
        a.chains = (const ShrinkChain *)ws.chainBuf.ptr;
        a.block = block;
        a.source = SHRINK_VAR_GIVEN;
        a.counts = (int32_t *)ws.cntBuf.ptr;
        CHECK(launch(c, "shrink_prep", "k_shrink_prep", k_shrink_prep, shrink_grid(ws), dim3(SHRINK_TILE), 0, c->stream, a));
    }
    HIPOK(hipStreamSynchronize(c->stream));     // (the caller's arrays are free again)
    ws.ready = true;
    return 0;
}

static const char NO_SHRINK_INPUT[] = "no prepared shrinkage input: call csr_shrink_stage or csr_batch_shrink_prepare first";

// c: a batch context prepared by csr_batch_shrink_prepare, or NULL = the default context's staged host arrays
static int shrink_ws(csr_ctx *&c, bool batch) {
    if (batch) CHECK(need(c));
    else CHECK(ctx_or_default(c));
    if (!c->shrinkWs.ready || c->shrinkWs.fromBatch != batch) return fail("%s", NO_SHRINK_INPUT);
    return 0;
}

// folds the partials [tile][ns] chain by chain and hands the sums out: out[idx[k]][ns]
static int shrink_fold(csr_ctx *c, int ns, double *out) {
    csr_ctx::ShrinkWs &ws = c->shrinkWs;
    const size_t nc = ws.chains.size();
    CHECK(ws.outBuf.reserve(8 * nc * (size_t)ns));
    CHECK(launch(c, "shrink_fold", "k_shrink_fold", k_shrink_fold, dim3((unsigned)nc), dim3(256), 0, c->stream,
                 (const ShrinkChain *)ws.chainBuf.ptr, (const double *)ws.partBuf.ptr, ns, (double *)ws.outBuf.ptr));
    std::vector<double> host(nc * (size_t)ns);
    HIPOK(hipMemcpyAsync(host.data(), ws.outBuf.ptr, 8 * host.size(), hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    for (size_t k = 0; k < nc; ++k) std::copy(&host[k * ns], &host[k * ns] + ns, out + (size_t)ws.idx[k] * ns);
    return 0;
}
static ShrinkSumArgs shrink_sum_args(const csr_ctx::ShrinkWs &ws) {
    ShrinkSumArgs a;
    memset(&a, 0, sizeof(a));
    a.tr = ws.tr;
    a.chains = (const ShrinkChain *)ws.chainBuf.ptr;
    a.counts = (const int32_t *)ws.cntBuf.ptr;
    a.block = ws.block;
    a.partial = (double *)ws.partBuf.ptr;
    return a;
}

// out[chain][5]: totalWeight, centralWeight, excessMomentSum, varianceSum, finiteCount (an exact integer); the records of chains
// the input does not hold stay untouched
extern "C" int csr_shrink_initial_sums(csr_ctx *c, double null_z, double *out) {
    DEFAULT_CTX_GUARD;
    const bool batch = c != nullptr;
    if (!out) return fail("null argument");
    CHECK(shrink_ws(c, batch));
    csr_ctx::ShrinkWs &ws = c->shrinkWs;
    if (ws.chains.empty()) return 0;
    CHECK(ws.partBuf.reserve(8 * (size_t)std::max<int64_t>(ws.nTiles, 1) * SHRINK_INIT_NS));
    ShrinkSumArgs a = shrink_sum_args(ws);
    a.nullZSafe = null_z > SHRINK_FLOOR ? null_z : SHRINK_FLOOR;
    CHECK(launch(c, "shrink_initial", "k_shrink_initial", k_shrink_initial, shrink_grid(ws), dim3(SHRINK_TILE), 0, c->stream, a));
    return shrink_fold(c, SHRINK_INIT_NS, out);
}

// out[chain][4 + 2 K]: totalWeight, nullMass, logLikelihood, finiteCount, slabMass[K], slabSecond[K]
extern "C" int csr_shrink_em_step(csr_ctx *c, double pi0, int32_t K, const double *tau, const double *log_slab_prior, double *out) {
    DEFAULT_CTX_GUARD;
    const bool batch = c != nullptr;
    if (!out) return fail("null argument");
    CHECK(shrink_check_prior(pi0, K, tau, log_slab_prior));
    CHECK(shrink_ws(c, batch));
    csr_ctx::ShrinkWs &ws = c->shrinkWs;
    if (ws.chains.empty()) return 0;
    const int ns = SHRINK_EM_HEAD + 2 * K;
    CHECK(ws.partBuf.reserve(8 * (size_t)std::max<int64_t>(ws.nTiles, 1) * (size_t)ns));
    const ShrinkPrior *dp = nullptr;
    CHECK(shrink_upload_prior(c, pi0, K, tau, log_slab_prior, &dp));
    const ShrinkSumArgs a = shrink_sum_args(ws);
    CHECK(launch(c, "shrink_em", "k_shrink_em", K <= SHRINK_REG_K ? k_shrink_em<true> : k_shrink_em<false>, shrink_grid(ws),
                 dim3(SHRINK_TILE), sizeof(double) * SHRINK_WAVES * (size_t)ns, c->stream, a, dp));
    return shrink_fold(c, ns, out);
}

static int shrink_post_launch(csr_ctx *c, const ShrinkPostArgs &a, int32_t K, const ShrinkPrior *dp) {
    return launch(c, "shrink_post", "k_shrink_post", K <= SHRINK_REG_K ? k_shrink_post<true> : k_shrink_post<false>,
                  shrink_grid(c->shrinkWs), dim3(SHRINK_TILE), 0, c->stream, a, dp);
}

// the staged host arrays: out[5][total] = shrunk, posterior sd, spike probability, slab mean, slab weight of every bin
extern "C" int csr_shrink_posterior(double pi0, int32_t K, const double *tau, const double *log_slab_prior, float *out) {
    DEFAULT_CTX_GUARD;
    CHECK(shrink_check_prior(pi0, K, tau, log_slab_prior));
    csr_ctx *c = nullptr;
    CHECK(shrink_ws(c, false));
    csr_ctx::ShrinkWs &ws = c->shrinkWs;
    if (ws.total == 0) return 0;
    if (!out) return fail("null argument");
    CHECK(ws.postBuf.reserve(4 * 5 * (size_t)ws.total));
    const ShrinkPrior *dp = nullptr;
    CHECK(shrink_upload_prior(c, pi0, K, tau, log_slab_prior, &dp));
    float *o = (float *)ws.postBuf.ptr;
    ShrinkPostArgs a{ws.tr, (const ShrinkChain *)ws.chainBuf.ptr, o, o + ws.total, o + 2 * ws.total, o + 3 * ws.total, o + 4 * ws.total};
    CHECK(shrink_post_launch(c, a, K, dp));
    HIPOK(hipMemcpyAsync(out, o, 4 * 5 * (size_t)ws.total, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// batch context.  The state is (double) xs[:,0] of the reference-layout copy of the smoothed fit (the conversion and the side-effect
// rule of csr_batch_rocco_scores: no array of the fit changes); the variance track, the counts and the result tracks are the
// stage's own.
// ---------------------------------------------------------------------------------------------------------------
static ChainTrack<float> &shrink_track(csr_ctx *c, int which) {
    switch (which) {
    case CSR_SHRINK_SHRUNK: return c->shrunk;
    case CSR_SHRINK_POSTERIOR_SD: return c->shrunkSd;
    case CSR_SHRINK_SPIKE_PROP: return c->shrunkSpike;
    case CSR_SHRINK_SLAB_MEAN: return c->shrunkSlabMean;
    case CSR_SHRINK_SLAB_WEIGHT: return c->shrunkSlabWeight;
    default: return c->shrinkVar;
    }
}

// uncertainty: NULL = the variance of the fit ((float) sqrt(Ps00), squared and floored at 1e-12 in float32), or the float32
// uncertainty tracks of the taken chains one after the other (squared and floored the same way)
extern "C" int csr_batch_shrink_prepare(csr_ctx *c, const unsigned char *chain_mask, const float *uncertainty, int64_t block) {
    CHECK(need(c));
    CHECK(settle(c));
    if (block < 1) return fail("block must be at least 1");
    if (!c->haveBwd) return fail("no smoothed results to shrink");
    CHECK(export_impl(c, CSR_EXPORT_SMOOTH));
    csr_ctx::ShrinkWs &ws = c->shrinkWs;
    ws.ready = false;
    ws.fromBatch = true;
    ws.chains.clear();
    ws.idx.clear();
    CHECK(c->shrinkVar.ensure(c));
    const int nc = (int)c->chains.size();
    ws.total = 0;
    for (int i = 0; i < nc; ++i) {
        if (chain_mask && !chain_mask[i]) continue;
        if (uncertainty)
            HIPOK(hipMemcpyAsync(c->shrinkVar.at(c, i), uncertainty + ws.total, 4 * (size_t)c->chains[i].n, hipMemcpyHostToDevice, c->stream));
        ws.chains.push_back(ShrinkChain{c->chains[i].off, c->chains[i].n, 0, 0});
        ws.idx.push_back(i);
        ws.total += c->chains[i].n;
    }
    ws.nOut = nc;
    const int d = c->mdl.state_dim;
    ws.tr = ShrinkTrack{nullptr, nullptr, c->nat[CSR_ARR_XS], c->shrinkVar.d, d};
    CHECK(shrink_tables(c, block));
    if (!ws.chains.empty()) {
        ShrinkPrepArgs a;
        memset(&a, 0, sizeof(a));
        a.tr = ws.tr;
        a.chains = (const ShrinkChain *)ws.chainBuf.ptr;
        a.Ps = c->nat[CSR_ARR_PS];
        a.unc = c->shrinkVar.d;         // (in place: a lane reads its own element, then writes it)
        a.var = c->shrinkVar.d;
        a.psStride = (int64_t)d * d;
        a.block = block;
        a.source = uncertainty ? SHRINK_VAR_UNCERTAINTY : SHRINK_VAR_FIT;
        a.counts = (int32_t *)ws.cntBuf.ptr;
        CHECK(launch(c, "shrink_prep", "k_shrink_prep", k_shrink_prep, shrink_grid(ws), dim3(SHRINK_TILE), 0, c->stream, a));
    }
    HIPOK(hipStreamSynchronize(c->stream));
    for (int i : ws.idx) c->shrinkVar.set(i, true);
    ws.ready = true;
    return 0;
}

// the posterior tracks of the prepared chains, resident: shrunk, posterior sd, spike probability; with want_slab the two slab tracks
extern "C" int csr_batch_shrink_posterior(csr_ctx *c, double pi0, int32_t K, const double *tau, const double *log_slab_prior,
                                          int32_t want_slab) {
    CHECK(shrink_check_prior(pi0, K, tau, log_slab_prior));
    CHECK(shrink_ws(c, true));
    csr_ctx::ShrinkWs &ws = c->shrinkWs;
    if (ws.chains.empty()) return 0;
    const int last = want_slab ? CSR_SHRINK_SLAB_WEIGHT : CSR_SHRINK_SPIKE_PROP;
    for (int w = CSR_SHRINK_SHRUNK; w <= last; ++w) CHECK(shrink_track(c, w).ensure(c));
    const ShrinkPrior *dp = nullptr;
    CHECK(shrink_upload_prior(c, pi0, K, tau, log_slab_prior, &dp));
    ShrinkPostArgs a{ws.tr, (const ShrinkChain *)ws.chainBuf.ptr, c->shrunk.d, c->shrunkSd.d, c->shrunkSpike.d,
                     want_slab ? c->shrunkSlabMean.d : nullptr, want_slab ? c->shrunkSlabWeight.d : nullptr};
    CHECK(shrink_post_launch(c, a, K, dp));
    HIPOK(hipStreamSynchronize(c->stream));
    for (int i : ws.idx) {
        for (int w = CSR_SHRINK_SHRUNK; w <= last; ++w) shrink_track(c, w).set(i, true);
        if (!want_slab)         // (slab tracks of an earlier prior are not this prior's)
            for (int w = CSR_SHRINK_SLAB_MEAN; w <= CSR_SHRINK_SLAB_WEIGHT; ++w)
                if (shrink_track(c, w).d) shrink_track(c, w).set(i, false);
    }
    return 0;
}

extern "C" int csr_batch_shrink_download(csr_ctx *c, int32_t chain, int32_t which, float *host_dst) {
    CHECK(need_chain(c, chain, host_dst));
    if (which < CSR_SHRINK_SHRUNK || which > CSR_SHRINK_VARIANCE) return fail("bad shrinkage track %d", which);
    return shrink_track(c, which).download(c, chain, host_dst);
}

// What the four medians of `applyStateShrinkagePrior` read of the prepared chains that hold posterior tracks: count[chain] = the
// valid bins, mid[chain][4][2] = the lower and upper middle values (equal for an odd count, untouched for none) of |state|,
// |shrunk|, the spike probability and the posterior sd over the valid bins -- the caller averages them as np.median does.  The
// keys are sorted with the null's sort in work space (an invalid bin sorts behind every valid one); no resident array changes.
extern "C" int csr_batch_shrink_medians(csr_ctx *c, int64_t *count, double *mid) {
    if (!count || !mid) return fail("null argument");
    CHECK(shrink_ws(c, true));
    csr_ctx::ShrinkWs &ws = c->shrinkWs;
    for (int i : ws.idx)
        if (!c->shrunk.has(i)) return fail("chain %d has no %s", i, c->shrunk.what);
    if (ws.chains.empty()) return 0;
    std::vector<double> init(ws.nOut * (size_t)SHRINK_INIT_NS, 0.0);
    CHECK(csr_shrink_initial_sums(c, 1.0, init.data()));
    CHECK(ws.keyBuf.reserve(8 * 4 * (size_t)std::max<int64_t>(ws.total, 1)));
    std::vector<NullTrackHost> tracks;
    int64_t at = 0;
    for (size_t k = 0; k < ws.chains.size(); ++k) {
        const ShrinkChain &ch = ws.chains[k];
        count[ws.idx[k]] = (int64_t)init[(size_t)ws.idx[k] * SHRINK_INIT_NS + 4];
        if (ch.n == 0) continue;
        ShrinkKeyArgs a{ws.tr, ch, c->shrunk.d, c->shrunkSd.d, c->shrunkSpike.d, (double *)ws.keyBuf.ptr + 4 * at};
        CHECK(launch(c, "shrink_keys", "k_shrink_keys", k_shrink_keys, dim3((unsigned)((ch.n + 255) / 256)), dim3(256), 0, c->stream, a));
        for (int r = 0; r < 4; ++r) tracks.push_back(NullTrackHost{a.keys + r * ch.n, ch.n, nullptr, false, 0.0, 0.0});
        at += ch.n;
    }
    if (tracks.empty()) return 0;
    NullEngine E;
    E.c = c;
    CHECK(E.setup(tracks, false));
    CHECK(E.sort());
    std::vector<const double *> gp;
    size_t t = 0;
    for (size_t k = 0; k < ws.chains.size(); ++k) {
        if (ws.chains[k].n == 0) continue;
        const int64_t L = count[ws.idx[k]];
        for (int r = 0; r < 4; ++r, ++t) {
            if (L <= 0) continue;
            int64_t lo, hi;
            null_median_ranks(L, lo, hi);
            gp.push_back(E.sorted + E.tr[t].slot + lo);
            gp.push_back(E.sorted + E.tr[t].slot + hi);
        }
    }
    std::vector<double> gv;
    CHECK(E.gather(gp, gv));
    size_t g = 0;
    for (size_t k = 0; k < ws.chains.size(); ++k) {
        if (ws.chains[k].n == 0 || count[ws.idx[k]] <= 0) continue;
        for (int r = 0; r < 8; ++r) mid[(size_t)ws.idx[k] * 8 + r] = gv[g++];
    }
    return 0;
}
