// csr_host_null.inl -- part of csr_lib.hip (one translation unit; included in this order): the robust null of a score track --
// centre, scale, DWB residual template and the scale of a template (peaks.py:312-339, 418-556, 1077-1122) -- from the kernels of
// csr_null.h.  The device sorts, ranks, compacts and sums; the host composes the scalars between the stages (lerps, the maxima
// of the three scale estimates, the radius) exactly as the reference's Python does, one round trip per stage for ALL tracks of a
// call.  A track whose central support falls short of minSupport is not decided here: the reference then orders the track by an
// unstable argsort, so the caller decides it with NumPy (csr_null_out::host_fallback).

// np.quantile(.., method="interpolated_inverted_cdf") on n sorted values = lerp(v[lo], v[hi], g)
static void null_qranks(int64_t n, double q, int64_t &lo, int64_t &hi, double &g) {
    const double v = (double)n * q - 1.0, fl = std::floor(v);
    g = v - fl;
    lo = (int64_t)std::min<double>(std::max<double>(fl, 0.0), (double)(n - 1));
    hi = (int64_t)std::min<double>(std::max<double>(fl + 1.0, 0.0), (double)(n - 1));
}
// np.percentile(.., method="linear")
static void null_pranks(int64_t n, double q, int64_t &lo, int64_t &hi, double &g) {
    const double v = (double)(n - 1) * q, fl = std::floor(v);
    g = v - fl;
    lo = (int64_t)fl;
    hi = std::min<int64_t>(lo + 1, n - 1);
}
static double null_lerp(double a, double b, double g) {
    const double d = b - a;
    if (g >= 0.5) {
        const double t = d * (1.0 - g);
        return b - t;
    }
    const double t = d * g;
    return a + t;
}
// np.median of L sorted values given the two middle ones
static double null_median2(int64_t L, double lo, double hi) { return (L & 1) ? hi : (lo + hi) / 2.0; }
static void null_median_ranks(int64_t L, int64_t &lo, int64_t &hi) {
    hi = L / 2;
    lo = (L & 1) ? hi : hi - 1;
}
static double null_max4(double a, double b, double c, double d) { return std::max(std::max(a, b), std::max(c, d)); }

struct NullTrackHost {
    const double *src;      // device
    int64_t n;
    double *tmplOut;        // device, n values: where the template goes (null_prepare_tracks needs one)
    bool given;             // the template is built around givenCenter / givenScale instead of the track's own null
    double givenCenter, givenScale;
};

struct NullEngine {
    csr_ctx *c = nullptr;
    std::vector<NullTrackDev> tr;
    int64_t total = 0, longest = 0, longestPadded = 0;
    const NullTrackDev *dTr = nullptr;
    double *sorted = nullptr, *comp = nullptr;

    int nt() const { return (int)tr.size(); }
    csr_ctx::NullWs &ws() { return c->nullWs; }

    int setup(const std::vector<NullTrackHost> &tracks, bool needComp) {
        tr.clear();
        total = longest = longestPadded = 0;
        for (const NullTrackHost &t : tracks) {
            NullTrackDev d{};
            d.src = t.src;
            d.n = t.n;
            d.slot = total;
            d.padded = std::max<int64_t>((t.n + NULL_TILE - 1) / NULL_TILE * NULL_TILE, NULL_TILE);
            total += d.padded;
            longest = std::max(longest, t.n);
            longestPadded = std::max(longestPadded, d.padded);
            tr.push_back(d);
        }
        CHECK(ws().trackBuf.reserve(sizeof(NullTrackDev) * tr.size()));
        CHECK(ws().keysA.reserve(8 * (size_t)total));
        CHECK(ws().keysB.reserve(8 * (size_t)total));
        if (needComp) {
            CHECK(ws().comp.reserve(8 * (size_t)total));
            CHECK(ws().cnt.reserve(8 * (size_t)(total / NULL_TILE) + 8 * tr.size()));
            comp = (double *)ws().comp.ptr;
        }
        HIPOK(hipMemcpyAsync(ws().trackBuf.ptr, tr.data(), sizeof(NullTrackDev) * tr.size(), hipMemcpyHostToDevice, c->stream));
        HIPOK(hipStreamSynchronize(c->stream));
        dTr = (const NullTrackDev *)ws().trackBuf.ptr;
        return 0;
    }

    // sorted[slot .. slot + n) := the track in ascending order
    int sort() {
        Scope sc(c, "null_sort");
        unsigned long long *a = (unsigned long long *)ws().keysA.ptr, *b = (unsigned long long *)ws().keysB.ptr;
        CHECK(launch(c, nullptr, "k_null_sort_tile", k_null_sort_tile, dim3((unsigned)(longestPadded / NULL_TILE), (unsigned)nt()), dim3(256),
                     0, c->stream, dTr, a));
        const dim3 grid((unsigned)((longestPadded / NULL_VT + 255) / 256), (unsigned)nt());
        for (int64_t run = NULL_TILE; run < longestPadded; run *= 2) {
            CHECK(launch(c, nullptr, "k_null_merge", k_null_merge, grid, dim3(256), 0, c->stream, dTr, (const unsigned long long *)a, b, run));
            std::swap(a, b);
        }
        CHECK(launch(c, nullptr, "k_null_unkey", k_null_unkey, dim3((unsigned)(longestPadded / 256), (unsigned)nt()), dim3(256), 0, c->stream,
                     dTr, a));
        sorted = reinterpret_cast<double *>(a);
        return 0;
    }

    // small tables go up through jobBuf, small results come back through outBuf
    template <class T>
    int up(const std::vector<T> &v, const T *&dev, size_t at = 0) {
        CHECK(ws().jobBuf.reserve(at + sizeof(T) * v.size() + 256));
        HIPOK(hipMemcpyAsync((char *)ws().jobBuf.ptr + at, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice, c->stream));
        dev = (const T *)((char *)ws().jobBuf.ptr + at);
        return 0;
    }
    template <class T>
    int down(std::vector<T> &v, size_t count) {
        v.resize(count);
        HIPOK(hipMemcpyAsync(v.data(), ws().outBuf.ptr, sizeof(T) * count, hipMemcpyDeviceToHost, c->stream));
        HIPOK(hipStreamSynchronize(c->stream));
        return 0;
    }

    int gather(const std::vector<const double *> &ptrs, std::vector<double> &out) {
        out.clear();
        if (ptrs.empty()) return 0;
        const double *const *dev = nullptr;
        CHECK(up(ptrs, dev));
        CHECK(ws().outBuf.reserve(8 * ptrs.size()));
        CHECK(launch(c, "null_gather", "k_null_gather", k_null_gather, dim3((unsigned)((ptrs.size() + 63) / 64)), dim3(64), 0, c->stream, dev,
                     (int)ptrs.size(), (double *)ws().outBuf.ptr));
        return down(out, ptrs.size());
    }
    int search(const std::vector<NullQuery> &qs, std::vector<long long> &out) {
        out.clear();
        if (qs.empty()) return 0;
        const NullQuery *dev = nullptr;
        CHECK(up(qs, dev));
        CHECK(ws().outBuf.reserve(8 * qs.size()));
        CHECK(launch(c, "null_search", "k_null_search", k_null_search, dim3((unsigned)((qs.size() + 63) / 64)), dim3(64), 0, c->stream, dev,
                     (int)qs.size(), (long long *)ws().outBuf.ptr));
        return down(out, qs.size());
    }
    int eval(const std::vector<NullJob> &jobs) {
        if (jobs.empty()) return 0;
        const NullJob *dev = nullptr;
        CHECK(up(jobs, dev));
        int64_t most = 1;
        for (const NullJob &j : jobs) most = std::max(most, j.n);
        CHECK(launch(c, "null_eval", "k_null_eval", k_null_eval, dim3((unsigned)((most + 255) / 256), (unsigned)jobs.size()), dim3(256), 0,
                     c->stream, dev));
        HIPOK(hipStreamSynchronize(c->stream));
        return 0;
    }
    // out[j] = np.sum of e(src[i]) in NumPy's order
    int sums(const std::vector<NullJob> &jobs, std::vector<double> &out) {
        out.clear();
        if (jobs.empty()) return 0;
        const NullJob *dev = nullptr;
        CHECK(up(jobs, dev));
        int64_t most = 1;
        for (const NullJob &j : jobs) most = std::max(most, j.n);
        const int64_t maxChunks = (most + NP_CHUNK - 1) / NP_CHUNK;
        CHECK(ws().part.reserve(8 * (size_t)maxChunks * jobs.size()));
        CHECK(ws().outBuf.reserve(8 * jobs.size()));
        {
            Scope sc(c, "null_sum");
            CHECK(launch(c, nullptr, "k_null_sum", k_np_chunk_sums<NullJob>, dim3((unsigned)((maxChunks + 63) / 64), (unsigned)jobs.size()),
                         dim3(64), 0, c->stream, dev, (const double *)nullptr, (double *)ws().part.ptr, maxChunks));
            CHECK(launch(c, nullptr, "k_null_fold", k_np_fold<NullJob>, dim3((unsigned)((jobs.size() + 63) / 64)), dim3(64), 0, c->stream, dev,
                         (int)jobs.size(), (const double *)ws().part.ptr, maxChunks, (double *)ws().outBuf.ptr));
        }
        return down(out, jobs.size());
    }
    // out[4 q + r] = the rank[r]-th smallest |e(x)| over query q's sorted range
    int abs_ranks(const std::vector<NullAbsQuery> &qs, std::vector<double> &out) {
        out.clear();
        if (qs.empty()) return 0;
        const NullAbsQuery *dev = nullptr;
        CHECK(up(qs, dev));
        const size_t cnt = qs.size() * NULL_ABS_RANKS;
        CHECK(ws().outBuf.reserve(8 * cnt));
        CHECK(launch(c, "null_abs_rank", "k_null_abs_rank", k_null_abs_rank, dim3((unsigned)((cnt + 63) / 64)), dim3(64), 0, c->stream, dev,
                     (int)qs.size(), (double *)ws().outBuf.ptr));
        return down(out, cnt);
    }
    int hsm(const std::vector<long long> &m, std::vector<double> &out) {
        const long long *dev = nullptr;
        CHECK(up(m, dev));
        CHECK(ws().outBuf.reserve(8 * m.size()));
        HIPOK(hipMemsetAsync(ws().outBuf.ptr, 0, 8 * m.size(), c->stream));
        CHECK(launch(c, "null_hsm", "k_null_hsm", k_null_hsm, dim3((unsigned)nt()), dim3(NULL_HSM_T), 0, c->stream, dTr, (const double *)sorted,
                     dev, (double *)ws().outBuf.ptr));
        return down(out, m.size());
    }
    // comp[slot ..) := the members of the support in track order; size[track] = how many (0 for an inactive track)
    int compact(const std::vector<NullSupport> &sup, std::vector<long long> &size) {
        const NullSupport *dev = nullptr;
        CHECK(up(sup, dev));
        long long *cnt = (long long *)ws().cnt.ptr, *tot = cnt + total / NULL_TILE;
        CHECK(ws().outBuf.reserve(8 * sup.size()));
        HIPOK(hipMemsetAsync(tot, 0, 8 * sup.size(), c->stream));
        const dim3 grid((unsigned)(longestPadded / NULL_TILE), (unsigned)nt());
        {
            Scope sc(c, "null_compact");
            CHECK(launch(c, nullptr, "k_null_flag_count", k_null_flag_count, grid, dim3(256), 0, c->stream, dTr, dev, cnt));
            CHECK(launch(c, nullptr, "k_null_scan", k_null_scan, dim3((unsigned)((nt() + 63) / 64)), dim3(64), 0, c->stream, dTr, nt(), dev, cnt,
                         tot));
            CHECK(launch(c, nullptr, "k_null_scatter", k_null_scatter, grid, dim3(256), 0, c->stream, dTr, dev, (const long long *)cnt, comp));
        }
        size.resize(sup.size());
        HIPOK(hipMemcpyAsync(size.data(), tot, 8 * sup.size(), hipMemcpyDeviceToHost, c->stream));
        HIPOK(hipStreamSynchronize(c->stream));
        return 0;
    }
};

static NullAbsQuery null_abs_query(const double *sorted, int64_t n, int flags, double a, double m, long long r0, long long r1,
                                   long long r2, long long r3) {
    NullAbsQuery q{};
    q.sorted = sorted;
    q.n = n;
    q.e.flags = flags;
    q.e.a = a;
    q.e.m = m;
    q.rank[0] = r0; q.rank[1] = r1; q.rank[2] = r2; q.rank[3] = r3;
    return q;
}

static NullJob null_job(const double *src, double *dst, int64_t n, int flags, double a = 0.0, double b = 0.0, double m = 0.0, double f = 0.0,
                        double m2 = 0.0) {
    NullJob j{};
    j.src = src;
    j.dst = dst;
    j.n = n;
    j.e.flags = flags;
    j.e.a = a; j.e.b = b; j.e.m = m; j.e.f = f; j.e.m2 = m2;
    return j;
}

// The null of every track.  Tracks below 16 values and tracks whose central support falls short come back with host_fallback = 1.
static int null_prepare_tracks(csr_ctx *c, const std::vector<NullTrackHost> &tracks, double bulk_quantile, csr_null_out *outs) {
    const int nt = (int)tracks.size();
    const double q = std::min(std::max(bulk_quantile, 0.05), 0.95);
    struct St {
        bool on = false;
        int64_t n = 0, minSupport = 0, m = 0, ns = 0, lo = 0;
        double c = 0, medR = 0, meanR = 0, mad = 0, iqr = 0, sd = 0, radius = 0, medC = 0, meanC = 0;
        double tc = 0, ts = 0, clipAbs = 0, meanT = 0, m2 = 0, f = 0, tm = 0;
        bool zero = false;
    };
    std::vector<St> st((size_t)nt);
    bool any = false;
    for (int t = 0; t < nt; ++t) {
        csr_null_out &o = outs[t];
        memset(&o, 0, sizeof(o));
        o.bulk_quantile = q;
        st[t].n = tracks[t].n;
        st[t].minSupport = std::max<int64_t>(16, (int64_t)std::ceil(0.05 * (double)tracks[t].n));
        st[t].on = tracks[t].n >= 16;       // below 16 values the support can never reach minSupport
        if (!st[t].on) {
            o.host_fallback = 1;
            o.null_method = CSR_NULL_NEAREST_SUPPORT;
        }
        any = any || st[t].on;
    }
    if (!any) return 0;
    NullEngine E;
    E.c = c;
    CHECK(E.setup(tracks, true));
    CHECK(E.sort());
    auto S = [&](int t) { return E.sorted + E.tr[t].slot; };
    std::vector<const double *> gp;
    std::vector<double> gv, sv, hv, ov;
    std::vector<long long> lv;
    std::vector<NullJob> jobs;
    // -- cutoff and lower bulk
    for (int t = 0; t < nt; ++t) {
        if (!st[t].on) continue;
        int64_t lo, hi;
        double g;
        null_qranks(st[t].n, q, lo, hi, g);
        gp.push_back(S(t) + lo);
        gp.push_back(S(t) + hi);
    }
    CHECK(E.gather(gp, gv));
    std::vector<NullQuery> qs;
    for (int t = 0, k = 0; t < nt; ++t) {
        if (!st[t].on) continue;
        int64_t lo, hi;
        double g;
        null_qranks(st[t].n, q, lo, hi, g);
        outs[t].bulk_cutoff = null_lerp(gv[2 * k], gv[2 * k + 1], g);
        ++k;
        qs.push_back(NullQuery{S(t), st[t].n, 0.0, outs[t].bulk_cutoff, 0, 0});
    }
    CHECK(E.search(qs, lv));
    std::vector<long long> mv((size_t)nt, 0);
    for (int t = 0, k = 0; t < nt; ++t) {
        if (!st[t].on) continue;
        st[t].m = lv[k++];
        outs[t].bulk_source = CSR_NULL_LOWER_BULK;
        if (st[t].m < st[t].minSupport) {
            st[t].m = st[t].n;
            outs[t].bulk_source = CSR_NULL_FULL_TRACK;
        }
        outs[t].lower_bulk_size = st[t].m;
        outs[t].center_method = CSR_NULL_HALF_SAMPLE_MODE;      // (m >= 16 here)
        mv[t] = st[t].m;
    }
    // -- provisional centre
    CHECK(E.hsm(mv, hv));
    // -- bulk residual statistics: r = sorted[0 .. m) - centre (sorted too)
    gp.clear();
    jobs.clear();
    for (int t = 0; t < nt; ++t) {
        if (!st[t].on) continue;
        st[t].c = hv[t];
        outs[t].provisional_center = outs[t].null_center = st[t].c;
        int64_t a, b, l, h;
        double g;
        null_median_ranks(st[t].m, a, b);
        gp.push_back(S(t) + a);
        gp.push_back(S(t) + b);
        for (double p : {0.25, 0.75}) {
            null_pranks(st[t].m, p, l, h, g);
            gp.push_back(S(t) + l);
            gp.push_back(S(t) + h);
        }
        jobs.push_back(null_job(S(t), nullptr, st[t].m, NX_SUBA, st[t].c));
    }
    CHECK(E.gather(gp, gv));
    CHECK(E.sums(jobs, sv));
    jobs.clear();
    std::vector<NullJob> ev;
    std::vector<NullAbsQuery> aq;
    for (int t = 0, k = 0; t < nt; ++t) {
        if (!st[t].on) continue;
        St &s = st[t];
        const double *v = &gv[6 * (size_t)k];
        s.medR = null_median2(s.m, v[0] - s.c, v[1] - s.c);
        int64_t l, h;
        double g25, g75;
        null_pranks(s.m, 0.25, l, h, g25);
        null_pranks(s.m, 0.75, l, h, g75);
        const double p25 = null_lerp(v[2] - s.c, v[3] - s.c, g25), p75 = null_lerp(v[4] - s.c, v[5] - s.c, g75);
        s.iqr = (p75 - p25) / 1.349;
        s.meanR = sv[k] / (double)s.m;
        ++k;
        jobs.push_back(null_job(S(t), nullptr, s.m, NX_SUBA | NX_SUBM | NX_SQ, s.c, 0.0, s.meanR));
        // the bulk is sorted, so are its residuals: |r - median(r)| at the median's ranks, |r| at the 0.50 quantile's
        int64_t a, b;
        double g;
        null_median_ranks(s.m, a, b);
        aq.push_back(null_abs_query(S(t), s.m, NX_SUBA | NX_SUBM, s.c, s.medR, a, b, -1, -1));
        null_qranks(s.m, 0.5, a, b, g);
        aq.push_back(null_abs_query(S(t), s.m, NX_SUBA, s.c, 0.0, -1, -1, a, b));
    }
    CHECK(E.abs_ranks(aq, ov));
    CHECK(E.sums(jobs, sv));
    std::vector<NullSupport> sup((size_t)nt, NullSupport{0.0, 0.0, 0, 0});
    qs.clear();
    for (int t = 0, k = 0; t < nt; ++t) {
        if (!st[t].on) continue;
        St &s = st[t];
        const double *r0 = &ov[8 * (size_t)k], *r1 = r0 + 4;
        s.mad = 1.4826 * null_median2(s.m, r0[0], r0[1]);
        int64_t a, b;
        double g;
        null_qranks(s.m, 0.5, a, b, g);
        const double q50 = null_lerp(r1[2], r1[3], g);
        s.sd = std::sqrt(sv[k] / (double)(s.m - 1));
        ++k;
        const double supportScale = null_max4(s.mad, s.iqr, s.sd, 1.0e-6);
        s.radius = std::max(std::max(2.5 * supportScale, q50), 1.0e-6);
        outs[t].support_scale = supportScale;
        outs[t].support_radius = s.radius;
        sup[t] = NullSupport{s.c, s.radius, 1, 0};
        qs.push_back(NullQuery{S(t), s.n, s.c, -s.radius, 1, 0});
    }
    // -- the support, in track order
    std::vector<long long> size;
    CHECK(E.compact(sup, size));
    CHECK(E.search(qs, lv));
    gp.clear();
    jobs.clear();
    for (int t = 0, k = 0; t < nt; ++t) {
        if (!st[t].on) continue;
        St &s = st[t];
        s.ns = size[t];
        s.lo = lv[k++];
        outs[t].support_size = s.ns;
        outs[t].support_fraction = (double)s.ns / (double)std::max<int64_t>(s.n, 1);
        if (s.ns < s.minSupport) {          // the reference's nearest-support branch: not determined by the values
            s.on = false;
            outs[t].host_fallback = 1;
            outs[t].null_method = CSR_NULL_NEAREST_SUPPORT;
            continue;
        }
        outs[t].null_method = CSR_NULL_CENTRAL_SUPPORT;
        int64_t a, b, l, h;
        double g;
        null_median_ranks(s.ns, a, b);
        gp.push_back(S(t) + s.lo + a);
        gp.push_back(S(t) + s.lo + b);
        for (double p : {0.25, 0.75}) {
            null_pranks(s.ns, p, l, h, g);
            gp.push_back(S(t) + s.lo + l);
            gp.push_back(S(t) + s.lo + h);
        }
        jobs.push_back(null_job(E.comp + E.tr[t].slot, nullptr, s.ns, NX_SUBA, s.c));
    }
    CHECK(E.gather(gp, gv));
    CHECK(E.sums(jobs, sv));
    // -- null scale and clip from the centred support
    jobs.clear();
    aq.clear();
    for (int t = 0, k = 0; t < nt; ++t) {
        if (!st[t].on) continue;
        St &s = st[t];
        const double *v = &gv[6 * (size_t)k];
        s.medC = null_median2(s.ns, v[0] - s.c, v[1] - s.c);
        int64_t l, h;
        double g25, g75;
        null_pranks(s.ns, 0.25, l, h, g25);
        null_pranks(s.ns, 0.75, l, h, g75);
        const double p25 = null_lerp(v[2] - s.c, v[3] - s.c, g25), p75 = null_lerp(v[4] - s.c, v[5] - s.c, g75);
        s.iqr = (p75 - p25) / 1.349;
        s.meanC = sv[k] / (double)s.ns;
        ++k;
        s.tc = tracks[t].given ? tracks[t].givenCenter : s.c;
        const double *cp = E.comp + E.tr[t].slot;
        jobs.push_back(null_job(cp, nullptr, s.ns, NX_SUBA | NX_SUBM | NX_SQ, s.c, 0.0, s.meanC));
        // as a set the support is sorted[lo .. lo + ns): its absolute deviations are ranked there, its std summed in track order
        int64_t a, b;
        double g;
        null_median_ranks(s.ns, a, b);
        aq.push_back(null_abs_query(S(t) + s.lo, s.ns, NX_SUBA | NX_SUBM, s.c, s.medC, a, b, -1, -1));
        null_qranks(s.ns, 0.95, a, b, g);
        aq.push_back(null_abs_query(S(t) + s.lo, s.ns, NX_SUBA, s.tc, 0.0, -1, -1, a, b));
    }
    CHECK(E.abs_ranks(aq, ov));
    CHECK(E.sums(jobs, sv));
    jobs.clear();
    for (int t = 0, k = 0; t < nt; ++t) {
        if (!st[t].on) continue;
        St &s = st[t];
        const double *r0 = &ov[8 * (size_t)k], *r1 = r0 + 4;
        s.mad = 1.4826 * null_median2(s.ns, r0[0], r0[1]);
        s.sd = std::sqrt(sv[k] / (double)(s.ns - 1));
        ++k;
        outs[t].null_scale = null_max4(s.mad, s.iqr, s.sd, 1.0e-6);
        int64_t a, b;
        double g;
        null_qranks(s.ns, 0.95, a, b, g);
        s.ts = tracks[t].given ? tracks[t].givenScale : outs[t].null_scale;
        s.clipAbs = std::max(std::max(null_lerp(r1[2], r1[3], g), s.ts), 1.0e-6);
        outs[t].clip_abs = s.clipAbs;
        jobs.push_back(null_job(tracks[t].src, nullptr, s.n, NX_SUBA | NX_CLIP, s.tc, s.clipAbs));
    }
    // -- the template: clip, centre, rescale
    CHECK(E.sums(jobs, sv));
    jobs.clear();
    for (int t = 0, k = 0; t < nt; ++t) {
        if (!st[t].on) continue;
        St &s = st[t];
        s.meanT = sv[k++] / (double)s.n;
        jobs.push_back(null_job(tracks[t].src, nullptr, s.n, NX_SUBA | NX_CLIP | NX_SUBM, s.tc, s.clipAbs, s.meanT));
    }
    CHECK(E.sums(jobs, sv));
    jobs.clear();
    for (int t = 0, k = 0; t < nt; ++t) {
        if (!st[t].on) continue;
        St &s = st[t];
        s.m2 = sv[k++] / (double)s.n;
        jobs.push_back(null_job(tracks[t].src, nullptr, s.n, NX_SUBA | NX_CLIP | NX_SUBM | NX_SUBM2 | NX_SQ, s.tc, s.clipAbs, s.meanT, 0.0, s.m2));
    }
    CHECK(E.sums(jobs, sv));
    jobs.clear();
    ev.clear();
    for (int t = 0, k = 0; t < nt; ++t) {
        if (!st[t].on) continue;
        St &s = st[t];
        const double tStd = std::sqrt(sv[k++] / (double)(s.n - 1));
        s.zero = !(std::isfinite(tStd) && tStd > DBL_MIN);
        s.f = s.zero ? 0.0 : s.ts / tStd;
        double *dst = tracks[t].tmplOut;
        ev.push_back(null_job(tracks[t].src, dst, s.n, s.zero ? NX_ZERO : (NX_SUBA | NX_CLIP | NX_SUBM | NX_SCALE), s.tc, s.clipAbs, s.meanT, s.f));
        jobs.push_back(null_job(dst, nullptr, s.n, 0));
    }
    CHECK(E.eval(ev));
    CHECK(E.sums(jobs, sv));
    jobs.clear();
    for (int t = 0, k = 0; t < nt; ++t) {
        if (!st[t].on) continue;
        St &s = st[t];
        s.tm = sv[k++] / (double)s.n;
        outs[t].template_mean = s.tm;
        const double *dst = tracks[t].tmplOut;
        jobs.push_back(null_job(dst, nullptr, s.n, NX_SUBM | NX_SQ, 0.0, 0.0, s.tm));
    }
    CHECK(E.sums(jobs, sv));
    for (int t = 0, k = 0; t < nt; ++t) {
        if (!st[t].on) continue;
        outs[t].template_std = std::sqrt(sv[k++] / (double)(st[t].n - 1));
    }
    return 0;
}

// `_estimateTemplateScale` of one device vector: out = {scale, mad-based, iqr-based, std}
static int null_scale_device(csr_ctx *c, const double *dx, int64_t n, double *out) {
    NullEngine E;
    E.c = c;
    std::vector<NullTrackHost> tracks{NullTrackHost{dx, n, nullptr, false, 0.0, 0.0}};
    CHECK(E.setup(tracks, false));
    CHECK(E.sort());
    const double *S = E.sorted;
    std::vector<const double *> gp;
    std::vector<double> gv, sv, ov;
    int64_t a, b, l, h;
    double g25 = 0.0, g75 = 0.0;
    null_median_ranks(n, a, b);
    gp.push_back(S + a);
    gp.push_back(S + b);
    if (n >= 4) {
        null_pranks(n, 0.25, l, h, g25);
        gp.push_back(S + l);
        gp.push_back(S + h);
        null_pranks(n, 0.75, l, h, g75);
        gp.push_back(S + l);
        gp.push_back(S + h);
    }
    CHECK(E.gather(gp, gv));
    const double med = null_median2(n, gv[0], gv[1]);
    const double iqr = n >= 4 ? (null_lerp(gv[4], gv[5], g75) - null_lerp(gv[2], gv[3], g25)) / 1.349 : 0.0;
    CHECK(E.abs_ranks({null_abs_query(S, n, NX_SUBA, med, 0.0, a, b, -1, -1)}, ov));
    const double mad = 1.4826 * null_median2(n, ov[0], ov[1]);
    double sd = 0.0;
    if (n >= 2) {
        CHECK(E.sums({null_job(dx, nullptr, n, 0)}, sv));
        const double mean = sv[0] / (double)n;
        CHECK(E.sums({null_job(dx, nullptr, n, NX_SUBM | NX_SQ, 0.0, 0.0, mean)}, sv));
        sd = std::sqrt(sv[0] / (double)(n - 1));
    }
    out[0] = null_max4(mad, iqr, sd, 1.0e-6);
    out[1] = mad;
    out[2] = iqr;
    out[3] = sd;
    return 0;
}

static int null_check_vector(const char *name, const double *x, int64_t n) {
    if (n <= 0) return value_error("`%s` must be non-empty", name);
    for (int64_t i = 0; i < n; ++i)
        if (!std::isfinite(x[i])) return value_error("`%s` contains non-finite values", name);
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// host arrays (default context)
// ---------------------------------------------------------------------------------------------------------------
extern "C" int csr_null_prepare(const double *scores, int64_t n, double bulk_quantile, const double *given, csr_null_out *out,
                                double *template_out) {
    DEFAULT_CTX_GUARD;
    if (!scores || !out) return fail("null argument");
    CHECK(null_check_vector("scoreTrack", scores, n));
    csr_ctx *c = nullptr;
    CHECK(ctx_or_default(c));
    const double *dx = nullptr;
    CHECK(c->nullWs.xBuf.reserve(16 * (size_t)n));      // the track, then its template
    CHECK(stage_vector(c, c->nullWs.xBuf, scores, n, &dx));
    double *dt = (double *)c->nullWs.xBuf.ptr + n;
    std::vector<NullTrackHost> tracks{NullTrackHost{dx, n, dt, given != nullptr, given ? given[0] : 0.0, given ? given[1] : 0.0}};
    CHECK(null_prepare_tracks(c, tracks, bulk_quantile, out));
    if (template_out && !out->host_fallback) {
        HIPOK(hipMemcpyAsync(template_out, dt, 8 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
        HIPOK(hipStreamSynchronize(c->stream));
    }
    return 0;
}

extern "C" int csr_null_scale(const double *x, int64_t n, double *out) {
    DEFAULT_CTX_GUARD;
    if (!x || !out) return fail("null argument");
    CHECK(null_check_vector("template", x, n));
    csr_ctx *c = nullptr;
    CHECK(ctx_or_default(c));
    const double *dx = nullptr;
    CHECK(stage_vector(c, c->nullWs.xBuf, x, n, &dx));
    return null_scale_device(c, dx, n, out);
}

// the device's ascending sort of one host vector (what every order statistic above is read from)
extern "C" int csr_null_sort(const double *x, int64_t n, double *out) {
    DEFAULT_CTX_GUARD;
    if (!x || !out) return fail("null argument");
    CHECK(null_check_vector("values", x, n));
    csr_ctx *c = nullptr;
    CHECK(ctx_or_default(c));
    const double *dx = nullptr;
    CHECK(stage_vector(c, c->nullWs.xBuf, x, n, &dx));
    NullEngine E;
    E.c = c;
    CHECK(E.setup({NullTrackHost{dx, n, nullptr, false, 0.0, 0.0}}, false));
    CHECK(E.sort());
    HIPOK(hipMemcpyAsync(out, E.sorted, 8 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// batch context: the resident score tracks in, one resident template per chain out (a buffer of its own, allocated at first use,
// freed with the batch); neither the scores nor any array of the fit changes
// ---------------------------------------------------------------------------------------------------------------
extern "C" int csr_batch_null_prepare(csr_ctx *c, double bulk_quantile, const unsigned char *chain_mask, csr_null_out *out) {
    CHECK(need(c));
    if (!out) return fail("null argument");
    std::vector<int> idx;
    CHECK(select_chains(c, chain_mask, c->scores, idx, NO_SCORES));
    CHECK(c->tmpl.ensure(c));
    std::vector<NullTrackHost> tracks;
    for (int i : idx) tracks.push_back(NullTrackHost{c->scores.at(c, i), c->chains[i].n, c->tmpl.at(c, i), false, 0.0, 0.0});
    if (tracks.empty()) return 0;
    std::vector<csr_null_out> res(tracks.size());
    for (int i : idx) c->tmpl.set(i, false);
    CHECK(null_prepare_tracks(c, tracks, bulk_quantile, res.data()));
    scatter_chains(idx, res.data(), out);
    for (int i : idx) c->tmpl.set(i, !out[i].host_fallback);
    return 0;
}

extern "C" int csr_batch_null_template_download(csr_ctx *c, int32_t chain, double *host_dst) {
    CHECK(need_chain(c, chain, host_dst));
    return c->tmpl.download(c, chain, host_dst);
}

extern "C" int csr_batch_null_template_upload(csr_ctx *c, int32_t chain, const double *tmpl) {
    CHECK(need_chain(c, chain, tmpl));
    CHECK(check_finite("template", tmpl, c->chains[chain].n));
    return c->tmpl.upload(c, chain, tmpl);
}

// `_estimateTemplateScale` of the selected chains' resident templates, concatenated in chain order (unpadded: NumPy's chunks of
// 8192 run across the chain boundaries)
extern "C" int csr_batch_null_pooled_scale(csr_ctx *c, const unsigned char *chain_mask, double *out) {
    CHECK(need(c));
    if (!out) return fail("null argument");
    std::vector<int> idx;
    CHECK(select_chains(c, chain_mask, c->tmpl, idx));
    int64_t total = 0;
    for (int i : idx) total += c->chains[i].n;
    if (total <= 0) return value_error("`template` must be non-empty");
    CHECK(c->nullWs.xBuf.reserve(8 * (size_t)total));
    double *dx = (double *)c->nullWs.xBuf.ptr;
    int64_t at = 0;
    for (int i : idx) {
        const int64_t n = c->chains[i].n;
        HIPOK(hipMemcpyAsync(dx + at, c->tmpl.at(c, i), 8 * (size_t)n, hipMemcpyDeviceToDevice, c->stream));
        at += n;
    }
    return null_scale_device(c, dx, total, out);
}

// A DWB panel over ALL chains of the batch whose templates are the resident ones (csr_batch_null_prepare /
// csr_batch_null_template_upload); everything else as csr_dwb_panel_begin
extern "C" int csr_batch_dwb_panel_begin(csr_ctx *c, const int32_t *bandwidth, const char *kernel, const double *noise, int64_t noise_len,
                                         int32_t n_draws, int32_t draws_per_group) {
    CHECK(need(c));
    std::vector<int> idx;
    CHECK(select_chains(c, nullptr, c->tmpl, idx));
    std::vector<int64_t> len;
    std::vector<const double *> tp;
    for (int i : idx) {
        len.push_back(c->chains[i].n);
        tp.push_back(c->tmpl.at(c, i));
    }
    return dwb_panel_begin(c, (int)idx.size(), len.data(), bandwidth, kernel, tp.data(), hipMemcpyDeviceToDevice, noise, noise_len, n_draws,
                           draws_per_group);
}
