// csr_host_munc_track.inl -- part of csr_lib.hip (one translation unit; included in this order): the kernels of csr_munc_track.h
// behind the C ABI.
//   csr_munc_eval_pspline / csr_munc_finalize_track / csr_munc_blacklist_floor     host arrays (default context): the drop-ins' engines
//   csr_batch_munc_block_sums / _prior_track / _track_finish                       the same kernels on the seed loop's resident arrays
// Invalid cells come back as the lowest index of each kind and counts; the caller raises the reference's error.
// csr_batch_munc_track_finish builds the track in an array of its own and copies it into the batch's munc at the end: a call whose
// caller has to raise leaves the batch as it was.

static const char NO_MUNC_FIT[] = "no smoothed results: the resident fit is gone (run forward_backward before this stage)";

// the chains a call takes, in chain order, every one a chain of the seed loop
struct MuncTaken {
    std::vector<int> idx;
    std::vector<int64_t> off, len;
    int64_t longest = 0;
};
static int munc_track_taken(csr_ctx *c, const unsigned char *mask, MuncTaken &t) {
    const BatchState::MuncSeed &S = c->seed;
    std::vector<char> inLoop(c->chains.size(), 0);
    for (int i : S.idx) inLoop[i] = 1;
    for (int i = 0; i < (int)c->chains.size(); ++i) {
        if (mask ? !mask[i] : !inLoop[i]) continue;
        if (!inLoop[i]) return fail("chain %d is not a chain of the seed loop (csr_batch_munc_seed_begin)", i);
        t.idx.push_back(i);
        t.off.push_back(c->chains[i].off);
        t.len.push_back(c->chains[i].n);
        t.longest = std::max(t.longest, c->chains[i].n);
    }
    if (t.idx.empty()) return fail("no chain taken");
    return 0;
}

// degree / sizes of a trend: *constant: the reference's fallback branch (pyx:5848)
static int munc_pspline_check(int64_t n_knots, int64_t n_basis, int32_t degree, const double *knots, const double *beta, bool *constant) {
    if (n_knots < 0 || n_basis < 0) return fail("bad shape");
    *constant = degree < 0 || n_knots == 0 || n_basis == 0;
    if (*constant) return (n_basis > 0 && !beta) ? fail("null argument") : 0;
    if (!knots || !beta) return fail("null argument");
    if (degree > MUNC_TRACK_MAX_DEGREE) return value_error("degree %d: the device evaluates B-splines up to degree %d", (int)degree, MUNC_TRACK_MAX_DEGREE);
    if (n_basis > MUNC_TRACK_MAX_BASIS) return value_error("%lld basis functions: the device evaluates up to %d", (long long)n_basis, MUNC_TRACK_MAX_BASIS);
    if (n_basis < degree + 1 || n_knots < n_basis + degree + 1)
        return value_error("knots and beta do not describe a B-spline of degree %d: need len(beta) >= degree + 1 and len(knots) >= len(beta) + degree + 1", (int)degree);
    return 0;
}
// the constant fallback's value (pyx:5849-5857), with the C library's exp
static float munc_pspline_constant(const double *beta, int64_t n_basis, double log_floor, double log_cap) {
    double logOut = n_basis > 0 ? beta[0] : log_floor;
    if (!std::isfinite(logOut)) logOut = logOut > 0.0 ? log_cap : log_floor;
    if (logOut < log_floor) logOut = log_floor;
    else if (logOut > log_cap) logOut = log_cap;
    return (float)std::exp(logOut);
}
static int munc_launch_prior(csr_ctx *c, const MuncPriorArgs &a, int32_t degree, int64_t longest, int nChains) {
    void (*k)(const MuncPriorArgs) = nullptr;
    switch (degree) {
        case 0: k = k_munc_prior_track<0>; break;
        case 1: k = k_munc_prior_track<1>; break;
        case 2: k = k_munc_prior_track<2>; break;
        case 3: k = k_munc_prior_track<3>; break;
        case 4: k = k_munc_prior_track<4>; break;
        default: k = k_munc_prior_track<5>; break;
    }
    return launch(c, "munc_prior_track", "k_munc_prior_track", k, dim3((unsigned)std::max<int64_t>((longest + 255) / 256, 1), (unsigned)nChains),
                  dim3(256), 0, c->stream, a);
}

// np.quantile(row, q) of the n float32 values a selection ranks, as NumPy 2 takes it on a float32 row with a Python float q: the
// virtual index (n - 1) q of the "linear" method, gamma and `_lerp` are float32 arithmetic.  lo / hi: the two 0-based ranks
struct MuncQuantileIndex {
    int64_t lo, hi;
    float gamma;
};
static MuncQuantileIndex munc_quantile_index(int64_t n, double quantile) {
    const float q = (float)quantile;
    const float vi = (float)(n - 1) * q;
    MuncQuantileIndex r;
    if (vi >= (float)(n - 1)) {         // `_get_indexes`: both at the last value
        r.lo = r.hi = n - 1;
        r.gamma = vi + 1.0f;
    } else if (vi < 0.0f) {
        r.lo = r.hi = 0;
        r.gamma = vi;
    } else {
        const float fl = std::floor(vi);
        r.lo = (int64_t)fl;
        r.hi = r.lo + 1;
        r.gamma = vi - fl;
    }
    return r;
}
static float munc_lerp_f32(float a, float b, float t) {
    const float d = b - a;
    if (t >= 0.5f) return b - d * (1.0f - t);
    return a + d * t;
}

// The blacklist floors of the (chain, track) rows of `x` (core.py:7201-7215): per row the `quantile` of the finite cells the mask
// leaves, not below base_floor; a chain whose mask has no set byte keeps base_floor and useFloor 0.  meta: dOff / dLen of the
// nChains chains; work: 2 words of trial and 2 of count per row.  Every cell of x is finite here or the caller does not use the result
static int munc_blacklist_floors(csr_ctx *c, const float *x, int64_t rowStride, int m, const unsigned char *exclude, const int64_t *dOff,
                                 const int64_t *dLen, const std::vector<int64_t> &len, int64_t longest, unsigned int *dTrial,
                                 unsigned long long *dCount, double base_floor, double quantile, std::vector<double> &floors,
                                 std::vector<unsigned char> &useFloor) {
    const int nChains = (int)len.size();
    const size_t rows = (size_t)nChains * (size_t)m;
    floors.assign(rows, base_floor);
    useFloor.assign((size_t)nChains, 0);
    if (!exclude) return 0;
    // how many cells each row's selection ranks: one counting pass with every key below the trial
    std::vector<unsigned int> all(2 * rows, 0xffffffffu);
    std::vector<unsigned long long> eligible(2 * rows);
    const int64_t perBlock = 256 * (int64_t)MUNC_RANK_ITEMS;
    const dim3 grid((unsigned)std::max<int64_t>((longest + perBlock - 1) / perBlock, 1), (unsigned)m, (unsigned)nChains);
    HIPOK(hipMemcpyAsync(dTrial, all.data(), 4 * all.size(), hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemsetAsync(dCount, 0, 8 * eligible.size(), c->stream));
    CHECK(launch(c, "munc_blacklist_count", "k_munc_rank_count", k_munc_rank_count, grid, dim3(256), 0, c->stream, x, rowStride, dOff, dLen,
                 (const unsigned int *)dTrial, dCount, exclude, 1, 1));
    HIPOK(hipMemcpyAsync(eligible.data(), dCount, 8 * eligible.size(), hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    // a chain has a mask where a row of it ranks fewer cells than it has; the count of masked intervals is the same for its rows
    std::vector<unsigned long long> want(2 * rows, 0ull);
    std::vector<MuncQuantileIndex> qi(rows);
    bool any = false;
    const double q = quantile < 0.0 ? 0.0 : (quantile > 1.0 ? 1.0 : quantile);
    for (int k = 0; k < nChains; ++k) {
        for (int j = 0; j < m; ++j) {
            const size_t r = (size_t)k * m + j;
            const int64_t ne = (int64_t)eligible[2 * r];
            if (ne < len[k]) useFloor[k] = 1;
            qi[r] = MuncQuantileIndex{-1, -1, 0.0f};
            if (ne <= 0) continue;
            qi[r] = munc_quantile_index(ne, q);
            want[2 * r] = (unsigned long long)qi[r].lo;
            want[2 * r + 1] = (unsigned long long)qi[r].hi;
        }
        any = any || useFloor[k];
    }
    if (!any) return 0;
    std::vector<unsigned int> ans;
    CHECK(munc_rank_select(c, "munc_blacklist_select", x, rowStride, m, exclude, 1, 1, dOff, dLen, nChains, longest, dTrial, dCount, want, ans));
    for (int k = 0; k < nChains; ++k) {
        if (!useFloor[k]) continue;
        for (int j = 0; j < m; ++j) {
            const size_t r = (size_t)k * m + j;
            if (qi[r].lo < 0) continue;
            float fa, fb;
            const unsigned int ua = munc_order_value(ans[2 * r]), ub = munc_order_value(ans[2 * r + 1]);
            memcpy(&fa, &ua, 4);
            memcpy(&fb, &ub, 4);
            floors[r] = std::max(base_floor, (double)munc_lerp_f32(fa, fb, qi[r].gamma));
        }
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// host arrays (default context)
// ---------------------------------------------------------------------------------------------------------------
extern "C" int csr_munc_eval_pspline(int64_t n, const double *predictor, const double *knots, int64_t n_knots, const double *beta,
                                     int64_t n_basis, int32_t degree, double x_min, double x_max, double log_floor, double log_cap,
                                     float *out) {
    DEFAULT_CTX_GUARD;
    if (n < 0) return fail("bad shape");
    if (n == 0) return 0;
    if (!predictor || !out) return fail("null argument");
    bool constant = false;
    CHECK(munc_pspline_check(n_knots, n_basis, degree, knots, beta, &constant));
    if (constant) {
        const float v = munc_pspline_constant(beta, n_basis, log_floor, log_cap);
        for (int64_t i = 0; i < n; ++i) out[i] = v;
        return 0;
    }
    csr_ctx *c = nullptr;
    CHECK(ctx_or_default(c));
    const int64_t nk = n_basis + degree + 1;
    CHECK(c->muncWs.in.reserve(8 * (size_t)(n + nk + n_basis)));
    CHECK(c->muncWs.out.reserve(4 * (size_t)n));
    double *dIn = (double *)c->muncWs.in.ptr;
    HIPOK(hipMemcpyAsync(dIn, predictor, 8 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemcpyAsync(dIn + n, knots, 8 * (size_t)nk, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemcpyAsync(dIn + n + nk, beta, 8 * (size_t)n_basis, hipMemcpyHostToDevice, c->stream));
    MuncPriorArgs a;
    memset(&a, 0, sizeof(a));
    a.predictor = dIn;
    a.knots = dIn + n;
    a.beta = dIn + n + nk;
    a.nKnots = (int)nk;
    a.nBasis = (int)n_basis;
    a.xMin = x_min; a.xMax = x_max; a.logFloor = log_floor; a.logCap = log_cap;
    a.out = (float *)c->muncWs.out.ptr;
    a.n = n;
    CHECK(munc_launch_prior(c, a, degree, n, 1));
    HIPOK(hipMemcpyAsync(out, a.out, 4 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    return 0;
}

// prm: posterior and scale filled in; the reference's parameter checks are the caller's (they interleave with its coercions)
static int munc_fill_prm(csr_munc_track_prm *prm, int m, int32_t use_eb) {
    for (int j = 0; j < m; ++j) {
        prm[j].posterior = prm[j].nu_local + prm[j].nu_prior;
        prm[j].scale = std::fabs(prm[j].factor - 1.0) > 1.0e-8 ? 1 : 0;
        prm[j].reserved_ = 0;
        if (use_eb && !(std::isfinite(prm[j].posterior) && prm[j].posterior > 0.0 && prm[j].nu_local > 0.0 && prm[j].nu_prior > 0.0))
            return value_error("posterior sample size must be positive and finite");
    }
    return 0;
}
static int munc_check_bounds(double floor, double cap) {
    if (floor <= 0.0 || !std::isfinite(floor)) return value_error("varianceFloor must be positive and finite");
    if (cap < floor || !std::isfinite(cap)) return value_error("varianceCap must be finite and at least varianceFloor");
    return 0;
}
// the kernel's words -> records; dBad / dCount: rows * MUNC_BAD_KINDS / MUNC_CNT_KINDS words, set up by the caller
static int munc_launch_finalize(csr_ctx *c, MuncFinalArgs a, int m, int64_t longest, int nChains, unsigned long long *dWords,
                                csr_munc_track_out *out) {
    const size_t rows = (size_t)nChains * (size_t)m;
    a.bad = dWords;
    a.count = dWords + rows * MUNC_BAD_KINDS;
    HIPOK(hipMemsetAsync(a.bad, 0xff, 8 * rows * MUNC_BAD_KINDS, c->stream));
    HIPOK(hipMemsetAsync(a.count, 0, 8 * rows * MUNC_CNT_KINDS, c->stream));
    CHECK(launch(c, "munc_finalize", "k_munc_finalize", k_munc_finalize,
                 dim3((unsigned)std::max<int64_t>((longest + 255) / 256, 1), (unsigned)m, (unsigned)nChains), dim3(256), 0, c->stream, a));
    std::vector<unsigned long long> h(rows * (MUNC_BAD_KINDS + MUNC_CNT_KINDS));
    HIPOK(hipMemcpyAsync(h.data(), dWords, 8 * h.size(), hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    for (size_t r = 0; r < rows; ++r) {
        const unsigned long long *b = &h[r * MUNC_BAD_KINDS], *n = &h[rows * MUNC_BAD_KINDS + r * MUNC_CNT_KINDS];
        auto index = [](unsigned long long v) { return v == ~0ull ? (int64_t)-1 : (int64_t)v; };
        out[r].invalid_local = index(b[MUNC_BAD_LOCAL]);
        out[r].invalid_prior = index(b[MUNC_BAD_PRIOR]);
        out[r].invalid_count_floor = index(b[MUNC_BAD_COUNT_FLOOR]);
        out[r].support = (int64_t)n[MUNC_CNT_SUPPORT];
        out[r].floor_finite = (int64_t)n[MUNC_CNT_FLOOR_FINITE];
        out[r].floor_added = (int64_t)n[MUNC_CNT_FLOOR_ADDED];
        out[r].floor_missing = (int64_t)n[MUNC_CNT_FLOOR_MISSING];
        out[r].blacklist_floor = 0.0;
    }
    return 0;
}
static size_t munc_final_words(int nChains, int m) { return (size_t)nChains * (size_t)m * (MUNC_BAD_KINDS + MUNC_CNT_KINDS); }

extern "C" int csr_munc_finalize_track(int64_t n, const float *local, const float *prior, const float *count_floor,
                                       const csr_munc_track_prm *prm_in, double floor, double cap, int32_t use_eb, float *out,
                                       csr_munc_track_out *res) {
    DEFAULT_CTX_GUARD;
    if (n < 0) return fail("bad shape");
    if (!res || !prm_in) return fail("null argument");
    CHECK(munc_check_bounds(floor, cap));
    csr_munc_track_prm prm = *prm_in;
    CHECK(munc_fill_prm(&prm, 1, use_eb));
    *res = csr_munc_track_out{-1, -1, -1, 0, 0, 0, 0, 0.0};
    if (n == 0) return 0;
    if (!local || !out || (use_eb && !prior)) return fail("null argument");
    csr_ctx *c = nullptr;
    CHECK(ctx_or_default(c));
    const size_t vn = 4 * (size_t)n;
    CHECK(c->muncWs.in.reserve(3 * vn + sizeof(prm) + 64));
    CHECK(c->muncWs.out.reserve(vn));
    CHECK(c->muncWs.flag.reserve(8 * munc_final_words(1, 1)));
    char *in = (char *)c->muncWs.in.ptr;
    MuncFinalArgs a;
    memset(&a, 0, sizeof(a));
    HIPOK(hipMemcpyAsync(in, &prm, sizeof(prm), hipMemcpyHostToDevice, c->stream));
    a.prm = (const MuncTrackPrm *)in;
    in += 64;
    static_assert(sizeof(csr_munc_track_prm) == sizeof(MuncTrackPrm) && sizeof(csr_munc_track_prm) <= 64, "one layout");
    HIPOK(hipMemcpyAsync(in, local, vn, hipMemcpyHostToDevice, c->stream));
    a.local = (const float *)in;
    in += vn;
    if (use_eb) {
        HIPOK(hipMemcpyAsync(in, prior, vn, hipMemcpyHostToDevice, c->stream));
        a.prior = (const float *)in;
    }
    in += vn;
    if (count_floor) {
        HIPOK(hipMemcpyAsync(in, count_floor, vn, hipMemcpyHostToDevice, c->stream));
        a.countFloor = (const float *)in;
    }
    a.out = (float *)c->muncWs.out.ptr;
    a.rowStride = n;
    a.floorV = floor; a.capV = cap;
    a.useEB = use_eb ? 1 : 0;
    a.floorMode = count_floor ? MUNC_FLOOR_NATIVE : MUNC_FLOOR_NONE;
    a.n = n;
    CHECK(munc_launch_finalize(c, a, 1, n, 1, (unsigned long long *)c->muncWs.flag.ptr, res));
    HIPOK(hipMemcpyAsync(out, a.out, vn, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int csr_munc_blacklist_floor(int64_t m, int64_t n, float *munc, const unsigned char *mask, double base_floor,
                                        double quantile, double *floors) {
    DEFAULT_CTX_GUARD;
    if (m < 0 || n < 0 || m > 65535) return fail("bad shape");
    if (!floors) return fail("null argument");
    if (!(base_floor >= 0.0) || !std::isfinite(base_floor)) return value_error("minR must be finite and nonnegative here");
    if (quantile != quantile) return value_error("Quantiles must be in the range [0, 1]");
    for (int64_t j = 0; j < m; ++j) floors[j] = base_floor;
    if (m == 0 || n == 0) return 0;
    if (!munc || !mask) return fail("null argument");
    csr_ctx *c = nullptr;
    CHECK(ctx_or_default(c));
    const size_t cells = (size_t)m * (size_t)n;
    CHECK(c->muncWs.in.reserve(4 * cells + (size_t)n + 64));
    CHECK(c->muncWs.out.reserve(4 * (size_t)m + 64));
    CHECK(c->muncWs.flag.reserve(64 + 24 * (size_t)m));
    float *dX = (float *)c->muncWs.in.ptr;
    unsigned char *dMask = (unsigned char *)c->muncWs.in.ptr + 4 * cells;
    int64_t *dMeta = (int64_t *)c->muncWs.flag.ptr;     // [0] offset, [1] length, [2] non-finite count, [3] use-floor byte
    unsigned long long *dCount = (unsigned long long *)(dMeta + 8);
    unsigned int *dTrial = (unsigned int *)(dCount + 2 * m);
    const int64_t meta[4] = {0, n, 0, 1};
    HIPOK(hipMemcpyAsync(dX, munc, 4 * cells, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemcpyAsync(dMask, mask, (size_t)n, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemcpyAsync(dMeta, meta, sizeof(meta), hipMemcpyHostToDevice, c->stream));
    std::vector<double> fl;
    std::vector<unsigned char> use;
    CHECK(munc_blacklist_floors(c, dX, n, (int)m, dMask, dMeta, dMeta + 1, std::vector<int64_t>{n}, n, dTrial, dCount, base_floor, quantile, fl, use));
    // a row with non-finite cells ranks fewer cells than it has without any masked interval: the mask itself decides (core.py:7203)
    bool anyMask = false;
    for (int64_t i = 0; i < n && !anyMask; ++i) anyMask = mask[i] != 0;
    if (!anyMask) return 0;
    std::vector<float> f32((size_t)m);
    for (int64_t j = 0; j < m; ++j) {
        floors[j] = fl[j];
        f32[j] = (float)fl[j];
    }
    HIPOK(hipMemcpyAsync(c->muncWs.out.ptr, f32.data(), 4 * (size_t)m, hipMemcpyHostToDevice, c->stream));
    MuncStoreArgs s;
    memset(&s, 0, sizeof(s));
    s.track = dX;
    s.rowStride = n;
    s.exclude = dMask;
    s.floors = (const float *)c->muncWs.out.ptr;
    s.useFloor = (const unsigned char *)(dMeta + 3);
    s.n = n;
    s.nonFinite = (unsigned long long *)(dMeta + 2);
    CHECK(launch(c, "munc_track_store", "k_munc_track_store", k_munc_track_store, dim3((unsigned)((n + 255) / 256), (unsigned)m, 1u), dim3(256), 0,
                 c->stream, s));
    HIPOK(hipMemcpyAsync(munc, dX, 4 * cells, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    return 0;
}

// blocks of L intervals of a chain of n (consenrich.py:7364-7373: a last block shorter than 2 is dropped)
static int64_t munc_block_count(int64_t n, int64_t L) {
    int64_t nb = (n + L - 1) / L;
    if (nb > 0 && n - (nb - 1) * L < 2) --nb;
    return nb;
}
static int munc_launch_block_sums(csr_ctx *c, MuncBlockArgs &a, int64_t most, int nChains) {
    a.waves = a.blockLen <= MUNC_BLOCK_LDS_VALUES / MUNC_BLOCK_WAVES ? MUNC_BLOCK_WAVES : 1;
    return launch(c, "munc_block_sums", "k_munc_block_sums", k_munc_block_sums,
                  dim3((unsigned)((most + a.waves - 1) / a.waves), (unsigned)a.m, (unsigned)nChains), dim3(64 * a.waves), 0, c->stream, a);
}

extern "C" int csr_munc_block_sums(int64_t m, int64_t n, const float *evidence, const float *weight, const unsigned char *exclude,
                                   const double *mean, int64_t block_intervals, csr_munc_block_rec *recs, int64_t *included) {
    DEFAULT_CTX_GUARD;
    if (m < 0 || n < 0 || m > 65535) return fail("bad shape");
    const int64_t L = std::max<int64_t>(2, block_intervals);
    if (L > MUNC_BLOCK_MAX) return value_error("block_intervals %lld: the device stages blocks of up to %d intervals", (long long)L, MUNC_BLOCK_MAX);
    const int64_t nb = munc_block_count(n, L);
    if (m == 0 || nb == 0) return 0;
    if (!evidence || !weight || !mean || !recs || !included) return fail("null argument");
    csr_ctx *c = nullptr;
    CHECK(ctx_or_default(c));
    const size_t cells = (size_t)m * (size_t)n, recBytes = sizeof(MuncBlockRec) * (size_t)(m * nb);
    CHECK(c->muncWs.in.reserve(8 * (size_t)n + 8 * cells + (size_t)n + 64));
    CHECK(c->muncWs.out.reserve(recBytes + 8 * (size_t)nb));
    CHECK(c->muncWs.flag.reserve(64));
    double *dMean = (double *)c->muncWs.in.ptr;
    float *dEv = (float *)(dMean + n), *dW = dEv + cells;
    unsigned char *dEx = (unsigned char *)(dW + cells);
    int64_t *dMeta = (int64_t *)c->muncWs.flag.ptr;
    const int64_t meta[5] = {0, n, nb, 0, 0};
    HIPOK(hipMemcpyAsync(dMean, mean, 8 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemcpyAsync(dEv, evidence, 4 * cells, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemcpyAsync(dW, weight, 4 * cells, hipMemcpyHostToDevice, c->stream));
    if (exclude) HIPOK(hipMemcpyAsync(dEx, exclude, (size_t)n, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemcpyAsync(dMeta, meta, sizeof(meta), hipMemcpyHostToDevice, c->stream));
    MuncBlockArgs a;
    memset(&a, 0, sizeof(a));
    a.evidence = dEv;
    a.weight = dW;
    a.exclude = exclude ? dEx : nullptr;
    a.mean64 = dMean;
    a.rowStride = n;
    a.chainOff = dMeta; a.chainLen = dMeta + 1; a.chainBlocks = dMeta + 2; a.recOff = dMeta + 3; a.inclOff = dMeta + 4;
    a.blockLen = L;
    a.m = (int)m;
    a.rec = (MuncBlockRec *)c->muncWs.out.ptr;
    a.included = (int64_t *)((char *)c->muncWs.out.ptr + recBytes);
    CHECK(munc_launch_block_sums(c, a, nb, 1));
    HIPOK(hipMemcpyAsync(recs, a.rec, recBytes, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipMemcpyAsync(included, a.included, 8 * (size_t)nb, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// batch context: the seed loop's resident arrays
// ---------------------------------------------------------------------------------------------------------------
static int munc_need_fit(csr_ctx *c) {
    CHECK(settle(c));
    if (!c->haveBwd) return fail("%s", NO_MUNC_FIT);
    return 0;
}
// the small per-call arrays of the taken chains, 8-byte words in muncWs.flag: rows of nt int64 each
static int munc_put_meta(csr_ctx *c, const std::vector<std::vector<int64_t>> &rows, size_t extraBytes, int64_t **dev, char **extra) {
    const size_t nt = rows[0].size();
    CHECK(c->muncWs.flag.reserve(8 * nt * rows.size() + extraBytes + 64));
    int64_t *d = (int64_t *)c->muncWs.flag.ptr;
    for (size_t r = 0; r < rows.size(); ++r)
        HIPOK(hipMemcpyAsync(d + r * nt, rows[r].data(), 8 * nt, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));     // (the rows may be temporaries)
    *dev = d;
    if (extra) *extra = (char *)(d + rows.size() * nt);
    return 0;
}

extern "C" int csr_batch_munc_block_sums(csr_ctx *c, int64_t block_intervals, const unsigned char *chain_mask, csr_munc_block_rec *recs,
                                         int64_t n_recs, int64_t *included, int64_t n_blocks) {
    CHECK(munc_need_seed(c));
    if (!recs || !included) return fail("null argument");
    const int64_t L = std::max<int64_t>(2, block_intervals);       // consenrich.py:7364
    if (L > MUNC_BLOCK_MAX) return value_error("block_intervals %lld: the device stages blocks of up to %d intervals", (long long)L, MUNC_BLOCK_MAX);
    MuncTaken t;
    CHECK(munc_track_taken(c, chain_mask, t));
    CHECK(munc_need_fit(c));
    const int nt = (int)t.idx.size();
    std::vector<int64_t> blocks((size_t)nt), recOff((size_t)nt), inclOff((size_t)nt);
    int64_t totalRecs = 0, totalBlocks = 0, most = 0;
    for (int k = 0; k < nt; ++k) {
        const int64_t nb = munc_block_count(t.len[k], L);
        blocks[k] = nb;
        recOff[k] = totalRecs;
        inclOff[k] = totalBlocks;
        totalRecs += nb * c->m;
        totalBlocks += nb;
        most = std::max(most, nb);
    }
    if (totalRecs != n_recs || totalBlocks != n_blocks)
        return fail("block sums: %lld records and %lld blocks, the caller expects %lld and %lld", (long long)totalRecs, (long long)totalBlocks,
                    (long long)n_recs, (long long)n_blocks);
    if (most == 0) return 0;
    CHECK(export_impl(c, CSR_EXPORT_SMOOTH));
    BatchState::MuncSeed &S = c->seed;
    int64_t *dMeta = nullptr;
    CHECK(munc_put_meta(c, {t.off, t.len, blocks, recOff, inclOff}, 0, &dMeta, nullptr));
    static_assert(sizeof(csr_munc_block_rec) == sizeof(MuncBlockRec), "one layout");
    const size_t recBytes = sizeof(MuncBlockRec) * (size_t)totalRecs, inclBytes = 8 * (size_t)totalBlocks;
    CHECK(c->muncWs.out.reserve(recBytes + inclBytes));
    MuncBlockArgs a;
    memset(&a, 0, sizeof(a));
    a.evidence = S.smooth;
    a.weight = S.weight;
    a.exclude = S.useExclude ? S.exclude : nullptr;
    a.mean = c->nat[CSR_ARR_XS];
    a.meanStride = c->mdl.state_dim;
    a.rowStride = c->Npad;
    a.chainOff = dMeta; a.chainLen = dMeta + nt; a.chainBlocks = dMeta + 2 * nt; a.recOff = dMeta + 3 * nt; a.inclOff = dMeta + 4 * nt;
    a.blockLen = L;
    a.m = (int)c->m;
    a.rec = (MuncBlockRec *)c->muncWs.out.ptr;
    a.included = (int64_t *)((char *)c->muncWs.out.ptr + recBytes);
    CHECK(munc_launch_block_sums(c, a, most, nt));
    HIPOK(hipMemcpyAsync(recs, a.rec, recBytes, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipMemcpyAsync(included, a.included, inclBytes, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int csr_batch_munc_prior_track(csr_ctx *c, const unsigned char *chain_mask, const double *knots, int64_t n_knots,
                                          const double *beta, int64_t n_basis, int32_t degree, double x_min, double x_max,
                                          double log_floor, double log_cap) {
    CHECK(munc_need_seed(c));
    bool constant = false;
    CHECK(munc_pspline_check(n_knots, n_basis, degree, knots, beta, &constant));
    MuncTaken t;
    CHECK(munc_track_taken(c, chain_mask, t));
    CHECK(munc_need_fit(c));
    CHECK(munc_track_array(c, CSR_MUNC_SEED_PRIOR));
    BatchState::MuncSeed &S = c->seed;
    const int nt = (int)t.idx.size();
    if (constant) {         // (x is not read: pyx:5848-5858)
        const float v = munc_pspline_constant(beta, n_basis, log_floor, log_cap);
        unsigned int bits;
        memcpy(&bits, &v, 4);
        for (int k = 0; k < nt; ++k) HIPOK(hipMemsetD32Async((hipDeviceptr_t)(S.prior + t.off[k]), (int)bits, (size_t)t.len[k], c->stream));
        HIPOK(hipStreamSynchronize(c->stream));
        return 0;
    }
    CHECK(export_impl(c, CSR_EXPORT_SMOOTH));
    const int64_t nk = n_basis + degree + 1;
    int64_t *dMeta = nullptr;
    char *extra = nullptr;
    CHECK(munc_put_meta(c, {t.off, t.len}, 8 * (size_t)(nk + n_basis), &dMeta, &extra));
    double *dK = (double *)extra, *dB = dK + nk;
    HIPOK(hipMemcpyAsync(dK, knots, 8 * (size_t)nk, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemcpyAsync(dB, beta, 8 * (size_t)n_basis, hipMemcpyHostToDevice, c->stream));
    MuncPriorArgs a;
    memset(&a, 0, sizeof(a));
    a.mean = c->nat[CSR_ARR_XS];
    a.meanStride = c->mdl.state_dim;
    a.knots = dK;
    a.beta = dB;
    a.nKnots = (int)nk;
    a.nBasis = (int)n_basis;
    a.xMin = x_min; a.xMax = x_max; a.logFloor = log_floor; a.logCap = log_cap;
    a.out = S.prior;
    a.chainOff = dMeta;
    a.chainLen = dMeta + nt;
    CHECK(munc_launch_prior(c, a, degree, t.longest, nt));
    HIPOK(hipStreamSynchronize(c->stream));     // (knots and beta are the caller's)
    return 0;
}

extern "C" int csr_batch_munc_track_finish(csr_ctx *c, const unsigned char *chain_mask, csr_munc_track_prm *prm, double floor, double cap,
                                           int32_t use_eb, int32_t use_count_floor, double base_floor, double quantile, double clamp_lo,
                                           double clamp_hi, csr_munc_track_out *out, int64_t *non_finite) {
    CHECK(munc_need_seed(c));
    if (!prm || !out || !non_finite) return fail("null argument");
    CHECK(munc_check_bounds(floor, cap));
    if (!(base_floor >= 0.0) || !std::isfinite(base_floor)) return value_error("minR must be finite and nonnegative here");
    if (quantile != quantile) return value_error("Quantiles must be in the range [0, 1]");
    BatchState::MuncSeed &S = c->seed;
    const int m = (int)c->m;
    CHECK(munc_fill_prm(prm, m, use_eb));
    if (use_eb && !S.prior) return fail("no prior variance track: call csr_batch_munc_prior_track (or upload it) first");
    if (use_count_floor && !S.trackFloor) return fail("no raw count floor: upload CSR_MUNC_SEED_TRACK_FLOOR first");
    MuncTaken t;
    CHECK(munc_track_taken(c, chain_mask, t));
    CHECK(settle(c));
    const int nt = (int)t.idx.size();
    const size_t rows = (size_t)nt * (size_t)m;
    if (!S.track) CHECK(dalloc(c, &S.track, c->m * c->Npad));
    // muncWs.flag: offsets, lengths, then [prm | finalize words | per-chain non-finite | trial | count | floors | use-floor bytes]
    const size_t prmBytes = sizeof(MuncTrackPrm) * (size_t)m, wordBytes = 8 * munc_final_words(nt, m);
    const size_t extraBytes = prmBytes + wordBytes + 8 * (size_t)nt + 8 * rows + 16 * rows + 4 * rows + (size_t)nt + 64;
    int64_t *dMeta = nullptr;
    char *extra = nullptr;
    CHECK(munc_put_meta(c, {t.off, t.len}, extraBytes, &dMeta, &extra));
    MuncTrackPrm *dPrm = (MuncTrackPrm *)extra;
    unsigned long long *dWords = (unsigned long long *)(extra + prmBytes);
    unsigned long long *dNonFinite = dWords + munc_final_words(nt, m);
    unsigned long long *dCount = dNonFinite + nt;
    unsigned int *dTrial = (unsigned int *)(dCount + 2 * rows);
    float *dFloors = (float *)(dTrial + 2 * rows);
    unsigned char *dUse = (unsigned char *)(dFloors + rows);
    HIPOK(hipMemcpyAsync(dPrm, prm, prmBytes, hipMemcpyHostToDevice, c->stream));
    MuncFinalArgs a;
    memset(&a, 0, sizeof(a));
    a.local = S.smooth;
    a.prior = S.prior;
    a.countFloor = use_count_floor ? S.trackFloor : nullptr;
    a.out = S.track;
    a.rowStride = c->Npad;
    a.prm = dPrm;
    a.floorV = floor; a.capV = cap;
    a.useEB = use_eb ? 1 : 0;
    a.floorMode = use_count_floor ? MUNC_FLOOR_COERCED : MUNC_FLOOR_NONE;
    a.chainOff = dMeta;
    a.chainLen = dMeta + nt;
    CHECK(munc_launch_finalize(c, a, m, t.longest, nt, dWords, out));
    for (int k = 0; k < nt; ++k) non_finite[k] = 0;
    for (size_t r = 0; r < rows; ++r) {
        out[r].blacklist_floor = base_floor;
        if (out[r].invalid_local >= 0 || out[r].invalid_prior >= 0 || out[r].invalid_count_floor >= 0) return 0;    // the caller raises
    }
    std::vector<double> floors;
    std::vector<unsigned char> use;
    CHECK(munc_blacklist_floors(c, S.track, c->Npad, m, S.useExclude ? S.exclude : nullptr, dMeta, dMeta + nt, t.len, t.longest, dTrial, dCount,
                                base_floor, quantile, floors, use));
    std::vector<float> f32(rows);
    for (size_t r = 0; r < rows; ++r) {
        out[r].blacklist_floor = floors[r];
        f32[r] = (float)floors[r];
    }
    HIPOK(hipMemcpyAsync(dFloors, f32.data(), 4 * rows, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemcpyAsync(dUse, use.data(), (size_t)nt, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemsetAsync(dNonFinite, 0, 8 * (size_t)nt, c->stream));
    MuncStoreArgs s;
    memset(&s, 0, sizeof(s));
    s.track = S.track;
    s.rowStride = c->Npad;
    s.exclude = S.useExclude ? S.exclude : nullptr;
    s.floors = dFloors;
    s.useFloor = dUse;
    s.lo = (float)clamp_lo;
    s.hi = (float)clamp_hi;
    s.useHi = clamp_hi > 0.0 ? 1 : 0;
    s.chainOff = dMeta;
    s.chainLen = dMeta + nt;
    s.nonFinite = dNonFinite;
    s.clamp = 1;
    CHECK(launch(c, "munc_track_store", "k_munc_track_store", k_munc_track_store,
                 dim3((unsigned)std::max<int64_t>((t.longest + 255) / 256, 1), (unsigned)m, (unsigned)nt), dim3(256), 0, c->stream, s));
    std::vector<unsigned long long> nf((size_t)nt);
    HIPOK(hipMemcpyAsync(nf.data(), dNonFinite, 8 * (size_t)nt, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    bool bad = false;
    for (int k = 0; k < nt; ++k) {
        non_finite[k] = (int64_t)nf[k];
        bad = bad || nf[k] != 0;
    }
    if (bad) return 0;      // the caller raises (consenrich.py:9100-9106)
    for (int k = 0; k < nt; ++k)
        HIPOK(hipMemcpy2DAsync(const_cast<float *>(c->p.munc) + t.off[k], 4 * (size_t)c->Npad, S.track + t.off[k], 4 * (size_t)c->Npad,
                               4 * (size_t)t.len[k], (size_t)m, hipMemcpyDeviceToDevice, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    c->statsValid = c->haveFwd = c->haveBwd = false;
    return 0;
}
