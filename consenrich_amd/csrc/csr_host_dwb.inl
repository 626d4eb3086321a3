// csr_host_dwb.inl -- part of csr_lib.hip (one translation unit; included in this order): the stationary-null dependent wild
// bootstrap (DWB) panel behind the ROCCO budgets -- weights as pyx:9352-9359 on the host, then the kernels of csr_dwb.h.  The
// three natives on host arrays, a panel over any number of chains in two phases (order statistics, then tail statistics at the
// offsets the caller derives from them) and the tail statistics of one vector (host array or a batch's resident scores).
// Residency: the draws of a GROUP of draws are kept at a time; phase B makes them again (the code is deterministic), so the
// working set is draws_per_group x (padded bins of all chains) doubles whatever n_draws is, at the price of a second stencil and
// walk per draw.

static void seg_release(csr_ctx *c);     // csr_host_segments.inl

// pyx:9283-9291: 0 bartlett, 1 parzen, 2 quadratic spectral; CSR_ERR_VALUE for anything else
static int dwb_kernel_code(const char *kernel, int *code) {
    std::string s(kernel ? kernel : "");
    const char *ws = " \t\n\r\f\v";
    const size_t a = s.find_first_not_of(ws), b = s.find_last_not_of(ws);
    std::string name = a == std::string::npos ? std::string() : s.substr(a, b - a + 1);
    for (char &ch : name) ch = ch == '-' ? '_' : (char)tolower((unsigned char)ch);
    if (name == "bartlett" || name == "triangle" || name == "triangular") *code = 0;
    else if (name == "parzen") *code = 1;
    else if (name == "qs" || name == "quadratic_spectral" || name == "quadraticspectral") *code = 2;
    else return value_error("Unknown DWB kernel: %s", kernel ? kernel : "");
    return 0;
}
static int dwb_max_lag(int bandwidth, int code) {       // pyx:9294-9302
    const int bw = bandwidth >= 2 ? bandwidth : 2;
    if (code == 2) return std::max(8 * bw, 32);
    return bw;
}
static double dwb_kernel_value(int code, long lag, int bandwidth) {     // pyx:9305-9322
    const double bw = (double)(bandwidth >= 1 ? bandwidth : 1);
    const double ax = std::fabs((double)lag) / bw;
    if (code == 0) return ax <= 1.0 ? 1.0 - ax : 0.0;
    if (code == 1) {
        if (ax <= 0.5) return 1.0 - 6.0 * ax * ax + 6.0 * ax * ax * ax;
        if (ax <= 1.0) return 2.0 * (1.0 - ax) * (1.0 - ax) * (1.0 - ax);
        return 0.0;
    }
    if (ax < 1.0e-12) return 1.0;
    const double pi = 3.14159265358979323846;
    const double y = (6.0 * pi * ax) / 5.0;
    // ONE sincos call, as the reference's build (-fno-math-errno) makes of its sin(y) and cos(y): the C library's sincos and
    // sin differ by an ulp at isolated arguments (bandwidth 64, lag 88)
    double sinY, cosY;
    sincos(y, &sinY, &cosY);
    return (25.0 / (12.0 * pi * pi * ax * ax)) * ((sinY / std::fmax(y, 1.0e-12)) - cosY);
}
static void dwb_weights(int bandwidth, int code, std::vector<double> &w) {      // pyx:9352-9359
    const int bw = bandwidth >= 2 ? bandwidth : 2, maxLag = dwb_max_lag(bw, code);
    const size_t w0 = w.size();
    volatile double normSq = 0.0;
    for (int j = 0; j <= 2 * maxLag; ++j) {
        const double v = dwb_kernel_value(code, (long)j - (long)maxLag, bw);
        w.push_back(v);
        const double sq = v * v;
        normSq = normSq + sq;
    }
    const double norm = std::sqrt(std::fmax(normSq, DBL_MIN));
    for (size_t j = w0; j < w.size(); ++j) w[j] = w[j] / norm;
}

// chain table, weights and buffers of the context's panel
static int dwb_setup(csr_ctx *c, int nChains, const int64_t *len, const int32_t *bandwidth, int code) {
    csr_ctx::Dwb &d = c->dwb;
    d.ready = false;
    d.chains.assign((size_t)nChains, DwbChain{});
    std::vector<double> w;
    int64_t pad = 0;
    d.longest = 0;
    d.strideMax = 0;
    for (int i = 0; i < nChains; ++i) {
        const int maxLag = dwb_max_lag(bandwidth[i], code);
        if (maxLag > DWB_MAX_LAG) return fail("DWB bandwidth %d: %d lags exceed the limit of %d", (int)bandwidth[i], maxLag, DWB_MAX_LAG);
        DwbChain &ch = d.chains[i];
        ch.off = pad;
        ch.n = len[i];
        ch.stride = len[i] + 2 * (int64_t)maxLag;
        ch.maxLag = maxLag;
        ch.wOff = (int)w.size();
        dwb_weights(bandwidth[i], code, w);
        pad += (len[i] + 63) / 64 * 64;
        d.longest = std::max(d.longest, len[i]);
        d.strideMax = std::max(d.strideMax, ch.stride);
    }
    d.rowLen = std::max<int64_t>(pad, 64);
    d.maxChunks = std::max<int64_t>((d.longest + NP_CHUNK - 1) / NP_CHUNK, 1);
    CHECK(d.chainBuf.reserve(sizeof(DwbChain) * (size_t)nChains));
    CHECK(d.wtsBuf.reserve(8 * w.size()));
    HIPOK(hipMemcpyAsync(d.chainBuf.ptr, d.chains.data(), sizeof(DwbChain) * (size_t)nChains, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemcpyAsync(d.wtsBuf.ptr, w.data(), 8 * w.size(), hipMemcpyHostToDevice, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));     // (w leaves scope)
    return 0;
}

// rows 0 .. g-1 of the row buffer := draws d0 .. d0 + g - 1 of every chain (stencil, then the walk)
static int dwb_make_rows(csr_ctx *c, int64_t d0, int g, bool stencil, bool standardise, bool apply) {
    csr_ctx::Dwb &d = c->dwb;
    const int nc = (int)d.chains.size();
    if (stencil) {
        const dim3 grid((unsigned)((d.longest + DWB_ST - 1) / DWB_ST), (unsigned)g, (unsigned)nc);
        CHECK(launch(c, "dwb_movsum", "k_dwb_movsum", k_dwb_movsum, grid, dim3(DWB_ST), 0, c->stream, (const DwbChain *)d.chainBuf.ptr,
                     (const double *)d.noiseBuf.ptr, (const double *)d.wtsBuf.ptr, (double *)d.rowBuf.ptr, d.rowLen, d0));
    }
    DwbWalkArgs a;
    a.chains = (const DwbChain *)d.chainBuf.ptr;
    a.tmpl = (const double *)d.tmplBuf.ptr;
    a.rows = (double *)d.rowBuf.ptr;
    CHECK(d.meanBuf.reserve(8 * (size_t)nc * (size_t)g));
    a.means = (double *)d.meanBuf.ptr;
    a.rowLen = d.rowLen;
    a.nRows = g;
    a.standardise = standardise;
    a.apply = apply;
    {
        Scope sc(c, "dwb_walk");
        CHECK(launch(c, nullptr, "k_dwb_walk", k_dwb_walk, dim3((unsigned)((g + DWB_WR - 1) / DWB_WR), (unsigned)nc), dim3(64), 0, c->stream, a));
        if (apply)
            CHECK(launch(c, nullptr, "k_dwb_centre", k_dwb_centre, dim3((unsigned)((d.longest + 255) / 256), (unsigned)g, (unsigned)nc),
                         dim3(256), 0, c->stream, a.chains, a.rows, (const double *)a.means, a.rowLen, g));
    }
    return 0;
}

// tail statistics of rows 0 .. g-1 -> counts / soft [(chain * outRows + d0 + row) * nZ + z] on the device
static int dwb_tail_rows(csr_ctx *c, const double *rows, int64_t rowLen, const DwbChain *dChains, int nc, int64_t maxChunks, int g,
                         int nZ, const double *dOff, const double *dScale, long long *dCnt, double *dSoft, int64_t outRows,
                         int64_t d0) {
    csr_ctx::Dwb &d = c->dwb;
    const size_t slots = (size_t)nc * (size_t)g * (size_t)maxChunks * (size_t)nZ;
    CHECK(d.partBuf.reserve(16 * slots + 256));
    DwbTailArgs a;
    a.chains = dChains;
    a.rows = rows;
    a.rowLen = rowLen;
    a.off = dOff;
    a.scale = dScale;
    a.nZ = nZ;
    a.maxChunks = maxChunks;
    a.partSum = (double *)d.partBuf.ptr;
    a.partCnt = (long long *)((char *)d.partBuf.ptr + 8 * slots);
    a.nRows = g;
    a.cnt = dCnt;
    a.soft = dSoft;
    a.outRows = outRows;
    a.d0 = d0;
    {
        Scope sc(c, "dwb_tail");
        const dim3 grid((unsigned)((maxChunks * nZ + 63) / 64), (unsigned)g, (unsigned)nc);
        CHECK(launch(c, nullptr, "k_dwb_tail", k_dwb_tail, grid, dim3(64), 0, c->stream, a));
        const int64_t total = (int64_t)nc * g * nZ;
        CHECK(launch(c, nullptr, "k_dwb_tail_fold", k_dwb_tail_fold, dim3((unsigned)((total + 63) / 64)), dim3(64), 0, c->stream, a, nc));
    }
    return 0;
}

static int dwb_check_z(int32_t n_z, const double *offsets, const double *scales, const void *counts, const void *soft) {
    if (n_z <= 0 || n_z > DWB_MAX_Z) return fail("n_z must be in 1..%d", DWB_MAX_Z);
    if (!offsets || !scales || !counts || !soft) return fail("null argument");
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// the three natives on host arrays (default context)
// ---------------------------------------------------------------------------------------------------------------
extern "C" int csr_dwb_max_lag(int32_t bandwidth, const char *kernel, int32_t *max_lag) {
    int code = 0;
    CHECK(dwb_kernel_code(kernel, &code));
    if (!max_lag) return fail("null argument");
    *max_lag = dwb_max_lag(bandwidth, code);
    return 0;
}

// one chain, one row: noise (or multipliers) and template in, the row out
static int dwb_native(const double *noise, int64_t noise_len, const double *mult, const double *tmpl, int64_t n, int32_t bandwidth,
                      int code, double *out) {
    DEFAULT_CTX_GUARD;
    csr_ctx *c = nullptr;
    CHECK(ctx_or_default(c));
    csr_ctx::Dwb &d = c->dwb;
    CHECK(dwb_setup(c, 1, &n, &bandwidth, code));
    CHECK(d.rowBuf.reserve(8 * (size_t)d.rowLen));
    if (noise) {
        CHECK(d.noiseBuf.reserve(8 * (size_t)d.strideMax));
        HIPOK(hipMemcpyAsync(d.noiseBuf.ptr, noise, 8 * (size_t)d.strideMax, hipMemcpyHostToDevice, c->stream));
    } else
        HIPOK(hipMemcpyAsync(d.rowBuf.ptr, mult, 8 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    if (tmpl) {
        CHECK(d.tmplBuf.reserve(8 * (size_t)d.rowLen));
        HIPOK(hipMemcpyAsync(d.tmplBuf.ptr, tmpl, 8 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    }
    (void)noise_len;
    CHECK(dwb_make_rows(c, 0, 1, noise != nullptr, noise != nullptr, tmpl != nullptr));
    HIPOK(hipMemcpyAsync(out, d.rowBuf.ptr, 8 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int csr_dwb_multipliers(const double *noise, int64_t noise_len, int32_t bandwidth, const char *kernel, double *out) {
    int code = 0;
    CHECK(dwb_kernel_code(kernel, &code));
    const int bw = bandwidth >= 2 ? bandwidth : 2;
    const int64_t n = noise_len - 2 * (int64_t)dwb_max_lag(bw, code);
    if (n <= 0) return value_error("noise length is too short for the requested DWB bandwidth");
    if (!noise || !out) return fail("null argument");
    return dwb_native(noise, noise_len, nullptr, nullptr, n, bw, code, out);
}

extern "C" int csr_dwb_apply(const double *tmpl, int64_t n, const double *multipliers, int64_t n_multipliers, double *out) {
    if (n_multipliers != n) return value_error("template and multipliers must have the same length");
    if (n < 0) return fail("negative length");
    if (n == 0) return 0;
    if (!tmpl || !multipliers || !out) return fail("null argument");
    return dwb_native(nullptr, 0, multipliers, tmpl, n, 2, 0, out);
}

extern "C" int csr_dwb_draw(const double *tmpl, int64_t n, int32_t bandwidth, const char *kernel, const double *noise,
                            int64_t noise_len, double *out) {
    int code = 0;
    CHECK(dwb_kernel_code(kernel, &code));
    const int bw = bandwidth >= 2 ? bandwidth : 2;
    if (n < 0) return fail("negative length");
    if (n <= 0 || noise_len < n + 2 * (int64_t)dwb_max_lag(bw, code))
        return value_error("noise length is too short for the requested DWB bandwidth");
    if (noise_len != n + 2 * (int64_t)dwb_max_lag(bw, code)) return value_error("template and multipliers must have the same length");
    if (!tmpl || !noise || !out) return fail("null argument");
    return dwb_native(noise, noise_len, nullptr, tmpl, n, bw, code, out);
}

// ---------------------------------------------------------------------------------------------------------------
// the panel: begin (upload once per seed) -> order statistics (phase A) -> tail statistics (phase B) -> end
// ---------------------------------------------------------------------------------------------------------------
// templates[i]: chain i's template, on the host or on the device as `kind` says
static int dwb_panel_begin(csr_ctx *c, int32_t n_chains, const int64_t *chain_len, const int32_t *bandwidth, const char *kernel,
                           const double *const *templates, hipMemcpyKind kind, const double *noise, int64_t noise_len, int32_t n_draws,
                           int32_t draws_per_group) {
    DEFAULT_CTX_GUARD;
    int code = 0;
    CHECK(dwb_kernel_code(kernel, &code));
    if (n_chains <= 0 || !chain_len || !bandwidth || !templates || !noise) return fail("null or empty argument");
    if (n_draws <= 0) return fail("n_draws must be positive");
    if (draws_per_group < 0) return fail("draws_per_group must be non-negative (0 = default)");
    int64_t strideMax = 0;
    for (int i = 0; i < n_chains; ++i) {
        if (chain_len[i] <= 0) return fail("chain %d is empty", i);
        strideMax = std::max(strideMax, chain_len[i] + 2 * (int64_t)dwb_max_lag(bandwidth[i], code));
    }
    if (noise_len < (int64_t)n_draws * strideMax) return value_error("noise length is too short for the requested DWB bandwidth");
    CHECK(ctx_or_default(c));
    csr_ctx::Dwb &d = c->dwb;
    CHECK(dwb_setup(c, n_chains, chain_len, bandwidth, code));
    // default group: as many draws as fit 16 GiB of rows (chr1 x 128 draws: 1.3 GB; the 22 autosomes x 128: 14.7 GB, one group each)
    int g = draws_per_group > 0 ? draws_per_group : (int)std::max<int64_t>(1, ((int64_t)16 << 30) / (8 * d.rowLen));
    d.group = std::min<int>(g, n_draws);
    d.nDraws = n_draws;
    CHECK(d.rowBuf.reserve(8 * (size_t)d.rowLen * (size_t)d.group));
    CHECK(d.tmplBuf.reserve(8 * (size_t)d.rowLen));
    CHECK(d.noiseBuf.reserve(8 * (size_t)n_draws * (size_t)d.strideMax));
    for (int i = 0; i < n_chains; ++i)
        HIPOK(hipMemcpyAsync((double *)d.tmplBuf.ptr + d.chains[i].off, templates[i], 8 * (size_t)chain_len[i], kind, c->stream));
    HIPOK(hipMemcpyAsync(d.noiseBuf.ptr, noise, 8 * (size_t)n_draws * (size_t)d.strideMax, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    d.ready = true;
    return 0;
}

extern "C" int csr_dwb_panel_begin(csr_ctx *c, int32_t n_chains, const int64_t *chain_len, const int32_t *bandwidth,
                                   const char *kernel, const double *templates, const double *noise, int64_t noise_len,
                                   int32_t n_draws, int32_t draws_per_group) {
    if (n_chains <= 0 || !chain_len || !templates) {
        int code = 0;
        CHECK(dwb_kernel_code(kernel, &code));
        return fail("null or empty argument");
    }
    std::vector<const double *> tp((size_t)n_chains);
    int64_t so = 0;
    for (int i = 0; i < n_chains; ++i) {
        tp[i] = templates + so;
        so += chain_len[i];
    }
    return dwb_panel_begin(c, n_chains, chain_len, bandwidth, kernel, tp.data(), hipMemcpyHostToDevice, noise, noise_len, n_draws,
                           draws_per_group);
}

// ranks[chain][n_ranks] (-1 = unused: NaN comes back); out[chain][draw][rank]
extern "C" int csr_dwb_panel_order_stats(csr_ctx *c, int32_t n_ranks, const int64_t *ranks, double *out) {
    DEFAULT_CTX_GUARD;
    if (n_ranks <= 0 || n_ranks > DWB_MAX_RANKS) return fail("n_ranks must be in 1..%d", DWB_MAX_RANKS);
    if (!ranks || !out) return fail("null argument");
    CHECK(ctx_or_default(c));
    csr_ctx::Dwb &d = c->dwb;
    if (!d.ready) return fail("no DWB panel: call csr_dwb_panel_begin first");
    const int nc = (int)d.chains.size();
    for (int i = 0; i < nc; ++i)
        for (int q = 0; q < n_ranks; ++q)
            if (ranks[i * n_ranks + q] >= d.chains[i].n) return fail("chain %d: rank %lld out of range", i, (long long)ranks[i * n_ranks + q]);
    const size_t nOut = (size_t)nc * (size_t)d.nDraws * (size_t)n_ranks, oRank = (8 * nOut + 255) / 256 * 256;
    CHECK(d.outBuf.reserve(oRank + 8 * (size_t)nc * n_ranks));
    double *dOut = (double *)d.outBuf.ptr;
    long long *dRank = (long long *)((char *)d.outBuf.ptr + oRank);
    HIPOK(hipMemcpyAsync(dRank, ranks, 8 * (size_t)nc * n_ranks, hipMemcpyHostToDevice, c->stream));
    for (int64_t d0 = 0; d0 < d.nDraws; d0 += d.group) {
        const int g = (int)std::min<int64_t>(d.group, d.nDraws - d0);
        CHECK(dwb_make_rows(c, d0, g, true, true, true));
        CHECK(launch(c, "dwb_select", "k_dwb_select", k_dwb_select, dim3((unsigned)g, (unsigned)nc), dim3(256), 0, c->stream,
                     (const DwbChain *)d.chainBuf.ptr, (const double *)d.rowBuf.ptr, d.rowLen, (const long long *)dRank, (int)n_ranks,
                     dOut, (int64_t)d.nDraws, d0));
    }
    HIPOK(hipMemcpyAsync(out, dOut, 8 * nOut, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    return 0;
}

// offsets / scales [chain][n_z]; counts / soft [chain][draw][z]: count(draw > offset), mean(clip((draw - offset) / max(scale, DBL_MIN), 0, inf))
extern "C" int csr_dwb_panel_tail_stats(csr_ctx *c, int32_t n_z, const double *offsets, const double *scales, int64_t *counts,
                                        double *soft) {
    DEFAULT_CTX_GUARD;
    CHECK(dwb_check_z(n_z, offsets, scales, counts, soft));
    CHECK(ctx_or_default(c));
    csr_ctx::Dwb &d = c->dwb;
    if (!d.ready) return fail("no DWB panel: call csr_dwb_panel_begin first");
    const int nc = (int)d.chains.size();
    const size_t nOut = (size_t)nc * (size_t)d.nDraws * (size_t)n_z, nz = (size_t)nc * n_z;
    const size_t oSoft = (8 * nOut + 255) / 256 * 256, oOff = 2 * oSoft, oScale = oOff + (8 * nz + 255) / 256 * 256;
    CHECK(d.outBuf.reserve(oScale + 8 * nz));
    char *base = (char *)d.outBuf.ptr;
    std::vector<double> sc(scales, scales + nz);
    for (double &s : sc) s = std::fmax(s, DBL_MIN);
    HIPOK(hipMemcpyAsync(base + oOff, offsets, 8 * nz, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemcpyAsync(base + oScale, sc.data(), 8 * nz, hipMemcpyHostToDevice, c->stream));
    for (int64_t d0 = 0; d0 < d.nDraws; d0 += d.group) {
        const int g = (int)std::min<int64_t>(d.group, d.nDraws - d0);
        CHECK(dwb_make_rows(c, d0, g, true, true, true));
        CHECK(dwb_tail_rows(c, (const double *)d.rowBuf.ptr, d.rowLen, (const DwbChain *)d.chainBuf.ptr, nc, d.maxChunks, g, n_z,
                            (const double *)(base + oOff), (const double *)(base + oScale), (long long *)base, (double *)(base + oSoft),
                            d.nDraws, d0));
    }
    HIPOK(hipMemcpyAsync(counts, base, 8 * nOut, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipMemcpyAsync(soft, base + oSoft, 8 * nOut, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int csr_dwb_panel_end(csr_ctx *c) {
    DEFAULT_CTX_GUARD;
    CHECK(ctx_or_default(c));
    csr_ctx::Dwb &d = c->dwb;
    d.ready = false;
    HIPOK(hipStreamSynchronize(c->stream));
    for (DevBuf *b : {&d.rowBuf, &d.noiseBuf, &d.tmplBuf, &d.partBuf, &d.outBuf, &d.meanBuf}) b->release();
    seg_release(c);     // the work space of csr_dwb_panel_segments goes with the panel
    peak_pool_release(c);       // ... and so does its replay pool
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// tail statistics of ONE vector: a host array, or a chain's resident scores (the observed side of the panel)
// ---------------------------------------------------------------------------------------------------------------
static int dwb_vector_tail(csr_ctx *c, const double *dx, int64_t n, int32_t n_z, const double *offsets, const double *scales,
                           int64_t *counts, double *soft) {
    csr_ctx::Dwb &d = c->dwb;
    const size_t oOff = 256, oScale = oOff + 256, oCnt = oScale + 256, oSoft = oCnt + 256;
    CHECK(d.vecBuf.reserve(oSoft + 256));
    char *base = (char *)d.vecBuf.ptr;
    DwbChain ch{};
    ch.off = 0;
    ch.n = n;
    double sc[DWB_MAX_Z];
    for (int k = 0; k < n_z; ++k) sc[k] = std::fmax(scales[k], DBL_MIN);
    HIPOK(hipMemcpyAsync(base, &ch, sizeof(ch), hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemcpyAsync(base + oOff, offsets, 8 * (size_t)n_z, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemcpyAsync(base + oScale, sc, 8 * (size_t)n_z, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));     // (ch, sc leave scope)
    CHECK(dwb_tail_rows(c, dx, n, (const DwbChain *)base, 1, std::max<int64_t>((n + NP_CHUNK - 1) / NP_CHUNK, 1), 1, n_z,
                        (const double *)(base + oOff), (const double *)(base + oScale), (long long *)(base + oCnt),
                        (double *)(base + oSoft), 1, 0));
    HIPOK(hipMemcpyAsync(counts, base + oCnt, 8 * (size_t)n_z, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipMemcpyAsync(soft, base + oSoft, 8 * (size_t)n_z, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int csr_dwb_tail_stats(csr_ctx *c, const double *x, int64_t n, int32_t n_z, const double *offsets, const double *scales,
                                  int64_t *counts, double *soft) {
    DEFAULT_CTX_GUARD;
    CHECK(dwb_check_z(n_z, offsets, scales, counts, soft));
    if (!x || n <= 0) return fail("null or empty vector");
    CHECK(ctx_or_default(c));
    const double *dx = nullptr;
    CHECK(stage_vector(c, c->dwb.xBuf, x, n, &dx));
    return dwb_vector_tail(c, dx, n, n_z, offsets, scales, counts, soft);
}

// reads the chain's resident score track (csr_batch_rocco_scores / csr_batch_upload_scores); changes nothing resident
extern "C" int csr_batch_dwb_observed(csr_ctx *c, int32_t chain, int32_t n_z, const double *offsets, const double *scales,
                                      int64_t *counts, double *soft) {
    CHECK(need(c));
    CHECK(dwb_check_z(n_z, offsets, scales, counts, soft));
    CHECK(check_chain(c, chain));
    if (!c->scores.has(chain)) return fail("chain %d has no scores", chain);
    return dwb_vector_tail(c, c->scores.at(c, chain), c->chains[chain].n, n_z, offsets, scales, counts, soft);
}
