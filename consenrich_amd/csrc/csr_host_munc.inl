// csr_host_munc.inl -- part of csr_lib.hip (one translation unit; included in this order): the dense observation-variance seed
// natives of csr_munc.h behind the C ABI.
//   csr_munc_seed_pass / csr_munc_smooth_local      host arrays (default context): the drop-ins' engines, all outputs returned
//   csr_batch_munc_seed_*                           the same kernels on arrays that stay resident with the batch between the
//                                                   rounds of the seed loop (consenrich.py:7784-7945); a pass reads the resident
//                                                   smoothed fit (xs[:,0], max(Ps[:,0,0], 0)) and the batch's original data
// Invalid input is a flag the kernels reduce; the host then answers with the reference's ValueError text (it carries no index).
// A resident pass writes into the "next" copies of total / rho / omega, which csr_batch_munc_seed_swap makes current: a pass that
// raises leaves the current arrays as they were.

static const char MUNC_SEED_INVALID[] = "active MUNC seed cells must be finite with positive denominators";
static const char MUNC_LOCAL_INVALID[] = "active local evidence cells must be positive and finite";
static const char NO_MUNC_SEED[] = "no seed arrays: call csr_batch_munc_seed_begin first";

static int munc_check_cfg(const csr_munc_seed_cfg *cfg) {
    if (!cfg) return fail("null argument");
    // pyx:5116-5132, in its order
    if (cfg->pad < 0.0 || !std::isfinite(cfg->pad)) return value_error("pad must be finite and nonnegative");
    if (cfg->variance_floor <= 0.0 || !std::isfinite(cfg->variance_floor)) return value_error("varianceFloor must be positive and finite");
    if (!std::isfinite(cfg->variance_cap) || cfg->variance_cap < cfg->variance_floor)
        return value_error("varianceCap must be greater than or equal to varianceFloor");
    if (cfg->use_weights && cfg->student_t &&
        (cfg->student_t_df <= 0.0 || cfg->d_omega <= 0.0 || !std::isfinite(cfg->student_t_df) || !std::isfinite(cfg->d_omega) ||
         cfg->omega_min <= 0.0 || cfg->omega_max < cfg->omega_min || !std::isfinite(cfg->omega_min) || !std::isfinite(cfg->omega_max)))
        return value_error("seed weight parameters are invalid");
    return 0;
}
static void munc_fill_cfg(MuncSeedArgs &a, const csr_munc_seed_cfg *cfg) {
    a.pad = cfg->pad; a.dS = cfg->student_t_df; a.dOmega = cfg->d_omega; a.omegaMin = cfg->omega_min; a.omegaMax = cfg->omega_max;
    a.varianceFloor = cfg->variance_floor; a.varianceCap = cfg->variance_cap;
    a.weighted = (cfg->use_weights && cfg->student_t) ? 1 : 0;
    a.updateWeights = cfg->update_weights ? 1 : 0;
}
// one lane per interval of the longest chain, nChains rows of blocks; *bad: the invalid flag after the launch
static int munc_launch_seed(csr_ctx *c, const MuncSeedArgs &a, int64_t longest, int nChains, unsigned int *dFlag, bool *bad) {
    HIPOK(hipMemsetAsync(dFlag, 0, 4, c->stream));
    const dim3 grid((unsigned)std::max<int64_t>((longest + 255) / 256, 1), (unsigned)nChains);
    CHECK(launch(c, "munc_seed_pass", "k_munc_seed_pass", a.m <= MUNC_REG_TRACKS ? k_munc_seed_pass<true> : k_munc_seed_pass<false>, grid,
                 dim3(256), 0, c->stream, a));
    unsigned int h = 0;
    HIPOK(hipMemcpyAsync(&h, dFlag, 4, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    *bad = h != 0;
    return 0;
}
// speculative blocks, then the rows that saw an inexact operation; dWork: [0] invalid flag, [2..3] fallback rows (u64), [4..] one word per row
static int munc_launch_roll(csr_ctx *c, MuncRollArgs a, int64_t longest, int nChains, unsigned int *dWork, bool *bad, int64_t *fallback) {
    const size_t rows = (size_t)nChains * (size_t)a.m;
    HIPOK(hipMemsetAsync(dWork, 0, 16, c->stream));
    HIPOK(hipMemsetAsync(dWork + 4, 0, 4 * rows, c->stream));
    a.invalid = dWork;
    a.fallbackRows = reinterpret_cast<unsigned long long *>(dWork + 2);
    a.dirty = dWork + 4;
    const int64_t nb = std::max<int64_t>((longest + MUNC_ROLL_BLOCK - 1) / MUNC_ROLL_BLOCK, 1);
    CHECK(launch(c, "munc_roll_spec", "k_munc_roll_spec", k_munc_roll_spec, dim3((unsigned)((nb + 63) / 64), (unsigned)a.m, (unsigned)nChains),
                 dim3(64), 0, c->stream, a));
    CHECK(launch(c, "munc_roll_fix", "k_munc_roll_fix", k_munc_roll_fix, dim3((unsigned)a.m, (unsigned)nChains), dim3(64), 0,
                 c->stream, a));
    unsigned int h[4] = {0, 0, 0, 0};
    HIPOK(hipMemcpyAsync(h, dWork, 16, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    *bad = h[0] != 0;
    *fallback = (int64_t)(((unsigned long long)h[3] << 32) | h[2]);
    return 0;
}
static size_t munc_roll_work_bytes(int nChains, int64_t m) { return 16 + 4 * (size_t)nChains * (size_t)m; }

// ---------------------------------------------------------------------------------------------------------------
// host arrays (default context).  Shapes and parameters were checked by the caller in the reference's order; the parameter
// checks are repeated here for a C caller.  active_mode / exclude_mode: 0 none, 1 per interval, 2 per cell.
// ---------------------------------------------------------------------------------------------------------------
extern "C" int csr_munc_seed_pass(int64_t m, int64_t n, const float *data, const float *munc, const float *state_mean,
                                  const float *state_variance, const float *background, const float *g_variance, const float *count_floor,
                                  const float *omega_in, const float *rho_in, const unsigned char *active, int32_t active_mode,
                                  const csr_munc_seed_cfg *cfg, float *moment, float *rho_out, float *omega_raw, float *omega_out,
                                  float *local, float *variance) {
    DEFAULT_CTX_GUARD;
    if (m < 0 || n < 0 || m > 65535) return fail("bad shape");
    CHECK(munc_check_cfg(cfg));
    if (m == 0 || n == 0) return 0;
    if (!data || !munc || !state_mean || !state_variance || !moment || !rho_out || !omega_raw || !omega_out || !local || !variance)
        return fail("null argument");
    if (active_mode < 0 || active_mode > 2 || (active_mode != 0 && !active)) return fail("bad active mask mode");
    csr_ctx *c = nullptr;
    CHECK(ctx_or_default(c));
    const size_t cells = (size_t)m * (size_t)n, mn = 4 * cells, vn = 4 * (size_t)n;
    // inputs: data, munc, countFloor, rhoIn (cells); mean, var, bg, gvar, omegaIn (n); mask bytes.  outputs: 4 x cells + 2 x n
    const size_t maskBytes = active_mode == 2 ? cells : (active_mode == 1 ? (size_t)n : 0);
    CHECK(c->muncWs.in.reserve(4 * mn + 5 * vn + maskBytes + 64));
    CHECK(c->muncWs.out.reserve(4 * mn + 2 * vn));
    CHECK(c->muncWs.flag.reserve(64));
    char *in = (char *)c->muncWs.in.ptr;
    auto put = [&](const void *src, size_t bytes, const void **dev) -> int {
        *dev = nullptr;
        if (src) {
            HIPOK(hipMemcpyAsync(in, src, bytes, hipMemcpyHostToDevice, c->stream));
            *dev = in;
        }
        in += bytes;
        return 0;
    };
    MuncSeedArgs a;
    memset(&a, 0, sizeof(a));
    munc_fill_cfg(a, cfg);
    const void *p = nullptr;
    CHECK(put(data, mn, &p)); a.data = (const float *)p;
    CHECK(put(munc, mn, &p)); a.munc = (const float *)p;
    CHECK(put(count_floor, mn, &p)); a.countFloor = (const float *)p;
    CHECK(put(rho_in, mn, &p)); a.rhoIn = (const float *)p;
    CHECK(put(state_mean, vn, &p)); a.stateMean = (const float *)p;
    CHECK(put(state_variance, vn, &p)); a.stateVar = (const float *)p;
    CHECK(put(background, vn, &p)); a.background = (const float *)p;
    CHECK(put(g_variance, vn, &p)); a.gVariance = (const float *)p;
    CHECK(put(omega_in, vn, &p)); a.omegaIn = (const float *)p;
    CHECK(put(active_mode ? active : nullptr, maskBytes, &p)); a.active = (const unsigned char *)p;
    a.meanStride = a.varStride = 1;
    a.activeMode = active_mode;
    a.maskStride = n;
    a.rowStride = n;
    a.n = n;
    a.m = (int)m;
    float *out = (float *)c->muncWs.out.ptr;
    a.moment = out; a.rhoOut = out + cells; a.local = out + 2 * cells; a.variance = out + 3 * cells;
    a.omegaRaw = out + 4 * cells; a.omegaOut = out + 4 * cells + n;
    a.invalid = (unsigned int *)c->muncWs.flag.ptr;
    bool bad = false;
    CHECK(munc_launch_seed(c, a, n, 1, a.invalid, &bad));
    if (bad) return value_error("%s", MUNC_SEED_INVALID);
    float *dst[6] = {moment, rho_out, local, variance, omega_raw, omega_out};
    const float *src[6] = {a.moment, a.rhoOut, a.local, a.variance, a.omegaRaw, a.omegaOut};
    for (int k = 0; k < 6; ++k) HIPOK(hipMemcpyAsync(dst[k], src[k], k < 4 ? mn : vn, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int csr_munc_smooth_local(int64_t m, int64_t n, const float *local, int64_t window, const unsigned char *exclude,
                                     int32_t exclude_mode, double eps, float *out, int64_t *fallback_rows) {
    DEFAULT_CTX_GUARD;
    if (m < 0 || n < 0 || m > 65535) return fail("bad shape");
    if (window < 1) return value_error("windowIntervals must be positive");
    if (eps <= 0.0 || !std::isfinite(eps)) return value_error("eps must be positive and finite");
    if (fallback_rows) *fallback_rows = 0;
    if (m == 0 || n == 0) return 0;
    if (!local || !out) return fail("null argument");
    if (exclude_mode < 0 || exclude_mode > 2 || (exclude_mode != 0 && !exclude)) return fail("bad exclude mask mode");
    csr_ctx *c = nullptr;
    CHECK(ctx_or_default(c));
    const size_t cells = (size_t)m * (size_t)n;
    const size_t maskBytes = exclude_mode == 2 ? cells : (exclude_mode == 1 ? (size_t)n : 0);
    CHECK(c->muncWs.in.reserve(4 * cells + maskBytes + 64));
    CHECK(c->muncWs.out.reserve(4 * cells));
    CHECK(c->muncWs.flag.reserve(munc_roll_work_bytes(1, m)));
    HIPOK(hipMemcpyAsync(c->muncWs.in.ptr, local, 4 * cells, hipMemcpyHostToDevice, c->stream));
    unsigned char *dMask = (unsigned char *)c->muncWs.in.ptr + 4 * cells;
    if (maskBytes) HIPOK(hipMemcpyAsync(dMask, exclude, maskBytes, hipMemcpyHostToDevice, c->stream));
    MuncRollArgs a;
    memset(&a, 0, sizeof(a));
    a.local = (const float *)c->muncWs.in.ptr;
    a.exclude = maskBytes ? dMask : nullptr;
    a.excludeMode = exclude_mode;
    a.maskStride = n;
    a.out = (float *)c->muncWs.out.ptr;
    a.rowStride = n;
    a.n = n;
    a.m = (int)m;
    a.window = window;
    a.eps = eps;
    bool bad = false;
    int64_t fb = 0;
    CHECK(munc_launch_roll(c, a, n, 1, (unsigned int *)c->muncWs.flag.ptr, &bad, &fb));
    if (bad) return value_error("%s", MUNC_LOCAL_INVALID);
    HIPOK(hipMemcpyAsync(out, a.out, 4 * cells, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    if (fallback_rows) *fallback_rows = fb;
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// batch context: the arrays of the seed loop, resident with the batch
// ---------------------------------------------------------------------------------------------------------------
static int munc_need_seed(csr_ctx *c) {
    CHECK(need(c));
    if (!c->seed.ready) return fail("%s", NO_MUNC_SEED);
    return 0;
}
static int munc_fill_ones(csr_ctx *c, float *dst, size_t count) {
    HIPOK(hipMemsetD32Async((hipDeviceptr_t)dst, 0x3f800000, count, c->stream));
    return 0;
}

// total := the batch's resident munc (callers replace it chain by chain with csr_batch_munc_seed_upload), omega = rho = 1,
// background = background variance = 0; chain_mask: the chains the loop takes (n_chains bytes or NULL = all)
extern "C" int csr_batch_munc_seed_begin(csr_ctx *c, const unsigned char *chain_mask, int32_t use_count_floor, int32_t use_exclude) {
    CHECK(need(c));
    CHECK(settle(c));
    if (c->m > 65535) return fail("the seed loop takes at most 65535 tracks");
    BatchState::MuncSeed &S = c->seed;
    S.ready = false;
    const int nc = (int)c->chains.size();
    const int64_t cells = c->m * c->Npad;
    if (!S.total[0]) {
        for (int k = 0; k < 2; ++k) {
            CHECK(dalloc(c, &S.total[k], cells));
            CHECK(dalloc(c, &S.rho[k], cells));
            CHECK(dalloc(c, &S.omega[k], c->Npad));
        }
        CHECK(dalloc(c, &S.local, cells));
        CHECK(dalloc(c, &S.smooth, cells));
        CHECK(dalloc(c, &S.weight, cells));
        CHECK(dalloc(c, &S.g, c->Npad));
        CHECK(dalloc(c, &S.gvar, c->Npad));
        CHECK(dalloc(c, &S.dOff, nc));
        CHECK(dalloc(c, &S.dLen, nc));
        CHECK(dalloc(c, &S.work, (int64_t)(munc_roll_work_bytes(nc, c->m) / 4 + 1)));
    }
    if (use_count_floor && !S.countFloor) CHECK(dalloc(c, &S.countFloor, cells));
    if (use_exclude && !S.exclude) CHECK(dalloc(c, &S.exclude, c->Npad));
    S.useCountFloor = use_count_floor != 0;
    S.useExclude = use_exclude != 0;
    S.idx.clear();
    S.longest = 0;
    std::vector<int64_t> off, len;
    for (int i = 0; i < nc; ++i) {
        if (chain_mask && !chain_mask[i]) continue;
        S.idx.push_back(i);
        off.push_back(c->chains[i].off);
        len.push_back(c->chains[i].n);
        S.longest = std::max(S.longest, c->chains[i].n);
    }
    if (S.idx.empty()) return fail("the seed loop needs at least one chain");
    HIPOK(hipMemcpyAsync(S.dOff, off.data(), 8 * off.size(), hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemcpyAsync(S.dLen, len.data(), 8 * len.size(), hipMemcpyHostToDevice, c->stream));
    S.cur = 0;
    HIPOK(hipMemcpyAsync(S.total[0], c->p.munc, 4 * (size_t)cells, hipMemcpyDeviceToDevice, c->stream));
    for (float *z : {S.total[1], S.local, S.smooth, S.weight}) HIPOK(hipMemsetAsync(z, 0, 4 * (size_t)cells, c->stream));
    for (int k = 0; k < 2; ++k) {
        CHECK(munc_fill_ones(c, S.rho[k], (size_t)cells));
        CHECK(munc_fill_ones(c, S.omega[k], (size_t)c->Npad));
    }
    HIPOK(hipMemsetAsync(S.g, 0, 4 * (size_t)c->Npad, c->stream));
    HIPOK(hipMemsetAsync(S.gvar, 0, 4 * (size_t)c->Npad, c->stream));
    if (S.countFloor) HIPOK(hipMemsetAsync(S.countFloor, 0, 4 * (size_t)cells, c->stream));
    if (S.exclude) HIPOK(hipMemsetAsync(S.exclude, 0, (size_t)c->Npad, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));     // (off / len are locals)
    S.stats = csr_munc_seed_stats{};
    S.ready = true;
    return 0;
}

// the arrays of the finished tracks (csr_host_munc_track.inl) exist from their first use: the prior track is zero, the raw count
// floor NaN ("missing") until written
static int munc_track_array(csr_ctx *c, int32_t id) {
    BatchState::MuncSeed &S = c->seed;
    if (id == CSR_MUNC_SEED_PRIOR && !S.prior) {
        CHECK(dalloc(c, &S.prior, c->Npad));
        HIPOK(hipMemsetAsync(S.prior, 0, 4 * (size_t)c->Npad, c->stream));
    }
    if (id == CSR_MUNC_SEED_TRACK_FLOOR && !S.trackFloor) {
        CHECK(dalloc(c, &S.trackFloor, c->m * c->Npad));
        HIPOK(hipMemsetD32Async((hipDeviceptr_t)S.trackFloor, 0x7fc00000, (size_t)(c->m * c->Npad), c->stream));
    }
    return 0;
}

// the device array behind a CSR_MUNC_SEED_* id; *perCell: (m, n), else (n); *bytes: element size
static int munc_seed_array(csr_ctx *c, int32_t id, void **ptr, bool *perCell, size_t *bytes) {
    BatchState::MuncSeed &S = c->seed;
    *bytes = 4;
    *perCell = true;
    switch (id) {
        case CSR_MUNC_SEED_TOTAL: *ptr = S.total[S.cur]; break;
        case CSR_MUNC_SEED_TOTAL_NEXT: *ptr = S.total[1 - S.cur]; break;
        case CSR_MUNC_SEED_RHO: *ptr = S.rho[S.cur]; break;
        case CSR_MUNC_SEED_RHO_NEXT: *ptr = S.rho[1 - S.cur]; break;
        case CSR_MUNC_SEED_LOCAL: *ptr = S.local; break;
        case CSR_MUNC_SEED_SMOOTH: *ptr = S.smooth; break;
        case CSR_MUNC_SEED_WEIGHT: *ptr = S.weight; break;
        case CSR_MUNC_SEED_COUNT_FLOOR: *ptr = S.countFloor; break;
        case CSR_MUNC_SEED_OMEGA: *ptr = S.omega[S.cur]; *perCell = false; break;
        case CSR_MUNC_SEED_OMEGA_NEXT: *ptr = S.omega[1 - S.cur]; *perCell = false; break;
        case CSR_MUNC_SEED_G: *ptr = S.g; *perCell = false; break;
        case CSR_MUNC_SEED_GVAR: *ptr = S.gvar; *perCell = false; break;
        case CSR_MUNC_SEED_EXCLUDE: *ptr = S.exclude; *perCell = false; *bytes = 1; break;
        case CSR_MUNC_SEED_PRIOR: *ptr = S.prior; *perCell = false; break;
        case CSR_MUNC_SEED_TRACK_FLOOR: *ptr = S.trackFloor; break;
        default: return fail("bad seed array id %d", id);
    }
    if (!*ptr) return fail("seed array %d is not in use (csr_batch_munc_seed_begin)", id);
    return 0;
}
static int munc_seed_copy(csr_ctx *c, int32_t chain, int32_t id, void *host, bool up) {
    CHECK(munc_need_seed(c));
    CHECK(check_chain(c, chain));
    if (!host) return fail("null host buffer");
    if (up && (id == CSR_MUNC_SEED_PRIOR || id == CSR_MUNC_SEED_TRACK_FLOOR)) CHECK(munc_track_array(c, id));
    void *dev;
    bool perCell;
    size_t eb;
    CHECK(munc_seed_array(c, id, &dev, &perCell, &eb));
    const ChainInfo &ci = c->chains[chain];
    char *d = (char *)dev + eb * (size_t)ci.off;
    const size_t w = eb * (size_t)ci.n, rows = perCell ? (size_t)c->m : 1;
    if (up) HIPOK(hipMemcpy2DAsync(d, eb * (size_t)c->Npad, host, w, w, rows, hipMemcpyHostToDevice, c->stream));
    else HIPOK(hipMemcpy2DAsync(host, w, d, eb * (size_t)c->Npad, w, rows, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    return 0;
}
extern "C" int csr_batch_munc_seed_upload(csr_ctx *c, int32_t chain, int32_t array_id, const void *host_src) {
    return munc_seed_copy(c, chain, array_id, const_cast<void *>(host_src), true);
}
extern "C" int csr_batch_munc_seed_download(csr_ctx *c, int32_t chain, int32_t array_id, void *host_dst) {
    return munc_seed_copy(c, chain, array_id, host_dst, false);
}

static MuncCellArgs munc_cell_args(csr_ctx *c) {
    BatchState::MuncSeed &S = c->seed;
    MuncCellArgs a;
    memset(&a, 0, sizeof(a));
    a.chainOff = S.dOff;
    a.chainLen = S.dLen;
    a.rowStride = c->Npad;
    return a;
}
static dim3 munc_cell_grid(csr_ctx *c) {
    return dim3((unsigned)std::max<int64_t>((c->seed.longest + 255) / 256, 1), (unsigned)c->m, (unsigned)c->seed.idx.size());
}

// `_seedWorkingMunc` (consenrich.py:7482-7503) into the batch's own munc: what the next forward / backward pass reads
extern "C" int csr_batch_munc_seed_working(csr_ctx *c, double pad, int32_t use_weights) {
    CHECK(munc_need_seed(c));
    CHECK(settle(c));
    BatchState::MuncSeed &S = c->seed;
    MuncCellArgs a = munc_cell_args(c);
    a.total = S.total[S.cur];
    a.rho = S.rho[S.cur];
    a.omega = S.omega[S.cur];
    a.gVariance = S.gvar;
    a.out = const_cast<float *>(c->p.munc);
    a.pad = pad;
    a.useWeights = use_weights ? 1 : 0;
    CHECK(launch(c, "munc_working", "k_munc_cell", k_munc_cell<MUNC_CELL_WORKING>, munc_cell_grid(c), dim3(256), 0, c->stream, a));
    HIPOK(hipStreamSynchronize(c->stream));
    c->statsValid = c->haveFwd = c->haveBwd = false;
    return 0;
}

// `cMuncObservationMomentSeedPass` on the resident arrays: data = the batch's, munc = the current total, state = the resident
// smoothed fit, background / gVariance / countFloor / omegaIn / rhoIn = the seed arrays; rho, omega and total go to the "next"
// copies, local to the pointwise local array.  want_moment / want_omega_raw are not offered: both are log-only in the loop.
extern "C" int csr_batch_munc_seed_pass(csr_ctx *c, const csr_munc_seed_cfg *cfg) {
    CHECK(munc_need_seed(c));
    CHECK(munc_check_cfg(cfg));
    CHECK(settle(c));
    if (!c->haveBwd) return fail("no smoothed results for the seed pass");
    CHECK(export_impl(c, CSR_EXPORT_SMOOTH));
    BatchState::MuncSeed &S = c->seed;
    const int d = c->mdl.state_dim;
    MuncSeedArgs a;
    memset(&a, 0, sizeof(a));
    munc_fill_cfg(a, cfg);
    a.data = c->p.data;
    a.munc = S.total[S.cur];
    a.stateMean = c->nat[CSR_ARR_XS]; a.meanStride = d;
    a.stateVar = c->nat[CSR_ARR_PS]; a.varStride = (int64_t)d * d;
    a.clipVar = 1;
    a.background = S.g;
    a.gVariance = S.gvar;
    a.countFloor = S.useCountFloor ? S.countFloor : nullptr;
    a.omegaIn = S.omega[S.cur];
    a.rhoIn = S.rho[S.cur];
    a.rhoOut = S.rho[1 - S.cur];
    a.omegaOut = S.omega[1 - S.cur];
    a.local = S.local;
    a.variance = S.total[1 - S.cur];
    a.rowStride = a.maskStride = c->Npad;
    a.chainOff = S.dOff;
    a.chainLen = S.dLen;
    a.m = (int)c->m;
    a.invalid = S.work;
    bool bad = false;
    CHECK(munc_launch_seed(c, a, S.longest, (int)S.idx.size(), S.work, &bad));
    ++S.stats.passes;
    if (bad) return value_error("%s", MUNC_SEED_INVALID);
    return 0;
}

// what consenrich.py:7821-7827 does after a round: the pass's total, rho and omega become current (refill: weights disabled,
// omega and rho are 1 again)
extern "C" int csr_batch_munc_seed_swap(csr_ctx *c, int32_t refill_weights) {
    CHECK(munc_need_seed(c));
    BatchState::MuncSeed &S = c->seed;
    S.cur = 1 - S.cur;
    if (refill_weights) {
        CHECK(munc_fill_ones(c, S.rho[S.cur], (size_t)(c->m * c->Npad)));
        CHECK(munc_fill_ones(c, S.omega[S.cur], (size_t)c->Npad));
        HIPOK(hipStreamSynchronize(c->stream));
    }
    return 0;
}

// consenrich.py:7936-7945 after the pointwise pass: smooth = rolling mean of local, total = `_localEvidenceToTotalVariance`
// of it (cap <= 0: none), weight = rho * omega of the pass just made (the "next" copies), or ones without weights
extern "C" int csr_batch_munc_seed_finish(csr_ctx *c, int64_t window, double eps, double cap, int32_t use_weights) {
    CHECK(munc_need_seed(c));
    if (window < 1) return value_error("windowIntervals must be positive");
    if (eps <= 0.0 || !std::isfinite(eps)) return value_error("eps must be positive and finite");
    BatchState::MuncSeed &S = c->seed;
    MuncRollArgs r;
    memset(&r, 0, sizeof(r));
    r.local = S.local;
    r.exclude = S.useExclude ? S.exclude : nullptr;
    r.excludeMode = S.useExclude ? 1 : 0;
    r.maskStride = c->Npad;
    r.out = S.smooth;
    r.rowStride = c->Npad;
    r.chainOff = S.dOff;
    r.chainLen = S.dLen;
    r.m = (int)c->m;
    r.window = window;
    r.eps = eps;
    bool bad = false;
    int64_t fb = 0;
    CHECK(munc_launch_roll(c, r, S.longest, (int)S.idx.size(), S.work, &bad, &fb));
    ++S.stats.rolls;
    S.stats.roll_rows += (int64_t)S.idx.size() * c->m;
    S.stats.roll_fallback_rows += fb;
    S.stats.last_roll_fallback_rows = fb;
    if (bad) return value_error("%s", MUNC_LOCAL_INVALID);
    MuncCellArgs a = munc_cell_args(c);
    a.local = S.smooth;
    a.countFloor = S.useCountFloor ? S.countFloor : nullptr;
    a.useCap = cap > 0.0 ? 1 : 0;
    a.cap = (float)cap;
    a.out = S.total[S.cur];
    CHECK(launch(c, "munc_total", "k_munc_cell", k_munc_cell<MUNC_CELL_TOTAL>, munc_cell_grid(c), dim3(256), 0, c->stream, a));
    a.rho = S.rho[1 - S.cur];
    a.omega = S.omega[1 - S.cur];
    a.useWeights = use_weights ? 1 : 0;
    a.out = S.weight;
    CHECK(launch(c, "munc_weight", "k_munc_cell", k_munc_cell<MUNC_CELL_WEIGHT>, munc_cell_grid(c), dim3(256), 0, c->stream, a));
    HIPOK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int csr_batch_munc_seed_stats(csr_ctx *c, csr_munc_seed_stats *out) {
    CHECK(munc_need_seed(c));
    if (!out) return fail("null argument");
    *out = c->seed.stats;
    return 0;
}

// The counting selection of order statistics of float32 cells (k_munc_rank_count): want[2 s + r] is the 0-based rank of statistic
// r of slot s, ans[2 s + r] its order key (munc_order_value gives the float's bits), found bit by bit from the top in 32 passes
// over the cells.  Slots are the nChains chains of dOff / dLen with all their tracks (perTrack 0) or every (chain, track) row by
// itself (perTrack 1, slot chain * m + track); exclude / finiteOnly leave cells out.  dTrial / dCount: 2 words per slot
static int munc_rank_select(csr_ctx *c, const char *scope, const float *x, int64_t rowStride, int m, const unsigned char *exclude,
                            int perTrack, int finiteOnly, const int64_t *dOff, const int64_t *dLen, int nChains, int64_t longest, unsigned int *dTrial,
                            unsigned long long *dCount, const std::vector<unsigned long long> &want, std::vector<unsigned int> &ans) {
    const size_t words = want.size();
    std::vector<unsigned long long> cnt(words);
    std::vector<unsigned int> trial(words);
    ans.assign(words, 0u);
    const int64_t perBlock = 256 * (int64_t)MUNC_RANK_ITEMS;
    const dim3 grid((unsigned)std::max<int64_t>((longest + perBlock - 1) / perBlock, 1), (unsigned)m, (unsigned)nChains);
    Scope sc(c, scope);
    for (int bit = 31; bit >= 0; --bit) {
        for (size_t r = 0; r < words; ++r) trial[r] = ans[r] | ((bit ? (1u << bit) : 1u) - 1u);
        HIPOK(hipMemcpyAsync(dTrial, trial.data(), 4 * words, hipMemcpyHostToDevice, c->stream));
        HIPOK(hipMemsetAsync(dCount, 0, 8 * words, c->stream));
        CHECK(launch(c, nullptr, "k_munc_rank_count", k_munc_rank_count, grid, dim3(256), 0, c->stream, x, rowStride, dOff, dLen,
                     (const unsigned int *)dTrial, dCount, exclude, perTrack, finiteOnly));
        HIPOK(hipMemcpyAsync(cnt.data(), dCount, 8 * words, hipMemcpyDeviceToHost, c->stream));
        HIPOK(hipStreamSynchronize(c->stream));
        for (size_t r = 0; r < words; ++r)
            if (cnt[r] <= want[r]) ans[r] |= 1u << bit;
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// `_updateSeedBackground` (consenrich.py:7688-7777) from the resident arrays, after a seed pass and before the swap: the
// background solve of csr_batch_background_update fed with the seed's per-cell weights (CSR_BG_SEED_WEIGHTS: float32 of
// omega * rho / max(total + pad, 1e-12) of the CURRENT total / omega / rho, float32 residual = data - level of the resident fit),
// then G.  g_mode 0 ("disabled"): G = 0.  g_mode 1 ("proxy"): G = clip(float32(1 / max(D, 1e-12)), 0, q99) with D = the float64
// sum of the float64 weights + `_backgroundPenaltyDiagonal` + multiplier * max(median of the positive sums, 1e-12) where the new
// background is negative, and q99 = np.quantile(total, 0.99) of the chain's m * n cells (1.0 if not finite and positive): its two
// order statistics by 32 counting passes over the cells' order keys (munc_order_key), the median by the solver's own selection.
// cfg->use_initial and use_lambda are ignored (the loop passes no initial background and no lambda).  out: n_chains records.
// A chain whose solve the reference would answer with RuntimeError (status 2..4) leaves EVERY seed array as it was.
// On success SEED_G / SEED_GVAR hold the new pair and the batch's current background (what the next smoother subtracts) is g.
// ---------------------------------------------------------------------------------------------------------------
extern "C" int csr_batch_munc_seed_background(csr_ctx *c, const csr_bg_cfg *cfg_in, double pad, int32_t use_weights, int32_t g_mode,
                                              csr_bg_out *out) {
    CHECK(munc_need_seed(c));
    if (!cfg_in || !out) return fail("null argument");
    if (g_mode != 0 && g_mode != 1) return fail("g_mode must be 0 (disabled) or 1 (proxy)");
    BatchState::MuncSeed &S = c->seed;
    const int nc = (int)c->chains.size(), ns = (int)S.idx.size();
    if (!S.w64) {
        CHECK(dalloc(c, &S.w64, c->Npad));
        CHECK(dalloc(c, &S.gSel, 2 * (int64_t)nc));
        CHECK(dalloc(c, &S.rankCount, 2 * (int64_t)nc));
        CHECK(dalloc(c, &S.rankTrial, 2 * (int64_t)nc));
    }
    S.bgPad = pad;
    S.bgUseWeights = use_weights != 0;
    csr_bg_cfg cfg = *cfg_in;
    cfg.use_initial = CSR_BG_SEED_WEIGHTS;
    cfg.use_lambda = 0;
    CHECK(csr_batch_background_update(c, &cfg, out));
    for (int i : S.idx)
        if (out[i].status != CSR_BG_OK && out[i].status != CSR_BG_NO_SUPPORT) return 0;    // the caller raises the reference's error
    std::vector<double> sel(2 * (size_t)ns, 0.0);
    for (int k = 0; k < ns; ++k) sel[2 * k + 1] = 1.0;
    const double mult = cfg.negative_penalty_multiplier;
    if (g_mode == 1) {
        if (cfg.use_nonnegative && mult > 0.0) {        // consenrich.py:7742-7758 (a NaN multiplier is not > 0)
            BgBatch a = c->bg.bat;
            a.w = S.w64;
            Prm p = c->p;
            const int gridW = (a.NW + 3) / 4;
            auto wave_pass = [&](int what, int bit) -> int {
                CHECK(launch(c, nullptr, "k_bg_wave_pass", k_bg_wave_pass, dim3(gridW), dim3(256), 0, c->stream, p, a, what, bit,
                             (const unsigned char *)nullptr));
                return launch(c, nullptr, "k_bg_wave_fold", k_bg_wave_fold, dim3(nc), dim3(64), 0, c->stream, a, what, bit);
            };
            CHECK(wave_pass(0, 0));
            std::vector<double> cs(5 * (size_t)nc);
            HIPOK(hipMemcpyAsync(cs.data(), a.chainSum, 8 * 5 * nc, hipMemcpyDeviceToHost, c->stream));
            HIPOK(hipStreamSynchronize(c->stream));
            std::vector<long long> rank(2 * (size_t)nc, -1);
            for (int i : S.idx) {
                const long long sup = (long long)cs[5 * i + 1];
                if (sup <= 0) continue;
                rank[2 * i] = (sup - 1) / 2;
                rank[2 * i + 1] = sup / 2;
            }
            HIPOK(hipMemcpyAsync(c->bg.dSelRank, rank.data(), 8 * 2 * nc, hipMemcpyHostToDevice, c->stream));
            HIPOK(hipMemsetAsync(a.selAns, 0, 8 * 2 * nc, c->stream));
            {
                Scope sc(c, "munc_g_median_select");
                for (int bit = 62; bit >= 0; --bit) CHECK(wave_pass(1, bit));
            }
            std::vector<double> mid(2 * (size_t)nc, 0.0);
            HIPOK(hipMemcpyAsync(mid.data(), a.selAns, 8 * 2 * nc, hipMemcpyDeviceToHost, c->stream));
            HIPOK(hipStreamSynchronize(c->stream));
            for (int k = 0; k < ns; ++k) {
                const int i = S.idx[k];
                const double scale = rank[2 * i] >= 0 ? 0.5 * (mid[2 * i] + mid[2 * i + 1]) : 1.0;
                sel[2 * k] = mult * std::max(scale, 1.0e-12);
            }
        }
        // q99 of the current total: ranks floor((N - 1) 0.99) and the next one, NumPy's lerp
        std::vector<unsigned long long> want(2 * (size_t)ns);
        std::vector<unsigned int> ans;
        std::vector<double> frac((size_t)ns);
        for (int k = 0; k < ns; ++k) {
            const int64_t N = c->m * c->chains[S.idx[k]].n;
            const double vi = (double)(N - 1) * 0.99, fl = std::floor(vi);
            want[2 * k] = (unsigned long long)fl;
            want[2 * k + 1] = (unsigned long long)std::min<int64_t>((int64_t)fl + 1, N - 1);
            frac[k] = vi - fl;
        }
        CHECK(munc_rank_select(c, "munc_g_q99_select", S.total[S.cur], c->Npad, (int)c->m, nullptr, 0, 0, S.dOff, S.dLen, ns, S.longest, S.rankTrial,
                               S.rankCount, want, ans));
        for (int k = 0; k < ns; ++k) {
            float fa, fb;
            const unsigned int ua = munc_order_value(ans[2 * k]), ub = munc_order_value(ans[2 * k + 1]);
            memcpy(&fa, &ua, 4);
            memcpy(&fb, &ub, 4);
            const double a = fa, b = fb, t = frac[k], d = b - a;
            double q = t >= 0.5 ? b - d * (1.0 - t) : a + d * t;
            if (!std::isfinite(q) || q <= 0.0) q = 1.0;
            sel[2 * k + 1] = q;
        }
    }
    HIPOK(hipMemcpyAsync(S.gSel, sel.data(), 8 * sel.size(), hipMemcpyHostToDevice, c->stream));
    MuncGArgs g;
    memset(&g, 0, sizeof(g));
    g.chainOff = S.dOff; g.chainLen = S.dLen;
    g.w64 = S.w64;
    g.bgNext = c->nat[CSR_ARR_BACKGROUND_NEXT];
    g.sel = S.gSel;
    g.g = S.g; g.gvar = S.gvar;
    g.lamFirst = cfg.lam_first; g.lamSecond = cfg.lam;
    g.proxy = g_mode;
    CHECK(launch(c, "munc_g_proxy", "k_munc_g_proxy", k_munc_g_proxy, dim3((unsigned)std::max<int64_t>((S.longest + 255) / 256, 1), (unsigned)ns),
                 dim3(256), 0, c->stream, g));
    HIPOK(hipStreamSynchronize(c->stream));     // (sel is a local)
    std::vector<unsigned char> take((size_t)nc, 0);
    for (int i : S.idx) take[i] = 1;
    return csr_batch_background_apply(c, take.data());
}

// one chain's weight / rhs tracks of the last background update (float64, n each) and the float64 weight sums of the seed front
extern "C" int csr_batch_munc_seed_background_tracks(csr_ctx *c, int32_t chain, double *weight, double *rhs, double *weight64) {
    CHECK(munc_need_seed(c));
    CHECK(check_chain(c, chain));
    if (!c->bg.ready || !c->seed.w64) return fail("no seed background yet: call csr_batch_munc_seed_background first");
    const ChainInfo &ci = c->chains[chain];
    if (weight) HIPOK(hipMemcpyAsync(weight, c->bg.bat.w + ci.off, 8 * (size_t)ci.n, hipMemcpyDeviceToHost, c->stream));
    if (rhs) HIPOK(hipMemcpyAsync(rhs, c->bg.bat.rhs + ci.off, 8 * (size_t)ci.n, hipMemcpyDeviceToHost, c->stream));
    if (weight64) HIPOK(hipMemcpyAsync(weight64, c->seed.w64 + ci.off, 8 * (size_t)ci.n, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    return 0;
}
