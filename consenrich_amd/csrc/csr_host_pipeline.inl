// csr_host_pipeline.inl -- part of csr_lib.hip (one translation unit; included in this order): statistics, speculative chains with deferred validation, forward / backward / ECM, export
// clang-format off is NOT needed; this file is plain C++/HIP host code.

// ---------------------------------------------------------------------------------------------------------------
// compute
// ---------------------------------------------------------------------------------------------------------------
// natural-layout records of the superblock state chain ({gain}, {S0u, zbar}), allocated at first use
static int ensure_sb_nat(csr_ctx *c) {
    if (c->sbNatGain) return 0;
    CHECK(dalloc(c, &c->sbNatGain, c->Npad));
    return dalloc(c, &c->sbNatSZ, c->Npad);
}

extern "C" int csr_batch_stats(csr_ctx *c) {
    CHECK(need(c));
    CHECK(settle(c));
    // 2-ulp throughput mode: {S2c, log R} as one float32 pair (csr_device.h Prm::tS2L); the form is a property of the RESIDENT
    // statistics (a later csr_set_validation does not invalidate them: every reader goes through load_s2c / load_logr / load_s2l)
    c->p.statsF32 = c->xTolUlps > 0 ? 1 : 0;
    Prm p = c->p;
    // default mode with the superblock state chain: that chain reads {S0u, zbar} in the reference layout -- written here directly
    const bool natSZ = c->xTolUlps == 0 && c->mdl.state_dim == 2 && !c->seqState;
    p.natSZ = nullptr;
    if (natSZ) {
        CHECK(ensure_sb_nat(c));
        p.natSZ = reinterpret_cast<double2 *>(c->sbNatSZ);
    }
    // 16-byte loads, four bins per thread; 64-bin tiles (32 when the block length is not a multiple of 64)
    const int ts = (c->B % 64 == 0) ? 64 : 32;
    const int grid = (int)(c->NG * (c->B / ts) * (ts == 64 ? 4 : 2));
    void (*const kernel)(Prm) = ts == 64 ? &k_stats_v4<64, 4> : &k_stats_v4<32, 4>;
    CHECK(launch(c, "stats", "k_stats_v4", kernel, dim3(grid), dim3(256), 0, c->stream, p));
    c->statsValid = true;
    c->natSZValid = natSZ;
    c->haveFwd = c->haveBwd = false;
    return 0;
}

enum { ST_P = 0, ST_X = 1, ST_B = 2, ST_DEBUG = 3 };

// Host wait for the library's stream.  The waits on the pipeline's critical path are short (tens of microseconds at
// 1/8-genome batch sizes), where the wake-up latency of a blocking hipStreamSynchronize is a measurable share of the
// step: poll first, block only if the stream is still busy after ~200 us.
// OPT-IN (CONSENRICH_AMD_TIMER_SLACK=1; round 6: off by default -- a library call should not change an attribute of its caller's
// thread for 0.05 ms of a benchmark step): the calling thread's timer slack, lowered for the length of a wait loop (the kernel's
// default of 50 us turns a 20-us sleep into ~75); the caller's setting is put back on the way out.
static const bool g_timerSlackOptIn = [] { const char *e = getenv("CONSENRICH_AMD_TIMER_SLACK"); return e && atoi(e) != 0; }();
struct TimerSlack {
    long old = 0;
    TimerSlack() {
        if (!g_timerSlackOptIn) return;
        old = prctl(PR_GET_TIMERSLACK, 0UL, 0UL, 0UL, 0UL);
        if (old > 1000) (void)prctl(PR_SET_TIMERSLACK, 1000UL, 0UL, 0UL, 0UL);
    }
    ~TimerSlack() { if (g_timerSlackOptIn && old > 1000) (void)prctl(PR_SET_TIMERSLACK, (unsigned long)old, 0UL, 0UL, 0UL); }
};
// site: which wait of the pipeline this is (0 = the settle point's mailbox read, 1 = the state chain's verdict): each keeps its own
// estimate -- a step has both, of very different lengths
static hipError_t wait_stream(csr_ctx *c, int site = 0) {
    // a short burst of polls (the waits on a shard's critical path are tens of microseconds), then polls 20 us apart, then
    // a blocking wait: a rank never burns a core for the length of a latency-bound launch (8 ranks per node).  Two details
    // keep the wake-up from costing the step tens of microseconds: the calling thread's timer slack is lowered FOR THE LENGTH OF
    // THE WAIT (the kernel's default of 50 us turns a 20-us sleep into ~75; the caller's setting is put back on the way out),
    // and around the moment the PREVIOUS wait of this context ended (steps repeat) the loop polls without sleeping -- at most
    // ~0.4 ms of spinning per wait.
    TimerSlack slack;
    const auto t0 = std::chrono::steady_clock::now();
    auto elapsed_us = [&]() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count(); };
    for (int i = 0; i < 128; ++i) {
        const hipError_t q = hipStreamQuery(c->stream);
        if (q == hipSuccess) { c->lastWaitUs[site] = elapsed_us(); return hipSuccess; }
        if (q != hipErrorNotReady) return q;
    }
    const double expect = c->lastWaitUs[site];
    for (;;) {
        const double el = elapsed_us();
        if (el > 8000.0) break;
        const bool nearEnd = expect > 0.0 && el > expect - 150.0 && el < expect + 250.0;
        if (!nearEnd) std::this_thread::sleep_for(std::chrono::microseconds(20));
        const hipError_t q = hipStreamQuery(c->stream);
        if (q == hipSuccess) { c->lastWaitUs[site] = elapsed_us(); return hipSuccess; }
        if (q != hipErrorNotReady) return q;
    }
    const hipError_t r = hipStreamSynchronize(c->stream);
    c->lastWaitUs[site] = elapsed_us();
    return r;
}
// hand a pending folded check to the kernel about to be launched with `p` (or clear the fields)
static void take_pending_check(csr_ctx *c, Prm &p) {
    p.prevKind = CK_NONE;
    if (!c->pendChk.valid) return;
    unsigned int *cnt = reinterpret_cast<unsigned int *>(c->dMail);
    p.prevKind = c->pendChk.kind;
    p.prevCarryIn = c->pendChk.cin;
    p.prevCarryOut = c->pendChk.cout;
    p.prevCount = cnt + c->pendChk.stage;
    p.prevCountPass = cnt + MAIL_PASS0 + 4 * c->pendChk.stage;
    p.prevActive = c->pendChk.active;
    c->pendChk.valid = false;
}
// a stage that no speculative kernel followed: its check runs as a kernel of its own
static int flush_pending_check(csr_ctx *c) {
    if (!c->pendChk.valid) return 0;
    Prm p = c->p;
    p.xTolUlps = c->xTolUlps;           // the acceptance rule of the stage that is being checked
    take_pending_check(c, p);
    CHECK(launch(c, "chain_check", "k_chain_check", k_chain_check, dim3((int)c->NG), dim3(64), 0, c->stream, p));
    c->rs.fix_launches++;
    return 0;
}
static int read_mail(csr_ctx *c, size_t bytes) {
    CHECK(flush_pending_check(c));
    HIPOK(hipMemcpyAsync(c->hMail, c->dMail, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPOK(wait_stream(c));
    return 0;
}
static unsigned int take_fresh(csr_ctx *c, int stage) {
    const unsigned int now = reinterpret_cast<const unsigned int *>(c->hMail.ptr)[stage];
    const unsigned int fresh = now - c->lastCnt[stage];
    c->lastCnt[stage] = now;
    return fresh;
}
// adaptive warm-up: many first-pass mismatches mean the speculation window is too short for this data (longer filter
// memory); lengthen it for the following sweeps.  Results do not depend on it.
static void grow_warm(csr_ctx *c, int &warmRef, unsigned int fresh) {
    if (c->adaptWarm && (int64_t)fresh > std::max<int64_t>(4, c->NB / 256) && warmRef < 8192)
        warmRef = std::min(8192, warmRef * 2);
}
static int &stage_warm(csr_ctx *c, int stage) {
    if (stage == ST_P && c->fwdWindow) return *c->fwdWindow;        // fused forward chain with its own window
    if (stage == ST_B && c->bwdWindow) return *c->bwdWindow;        // warm-started smoother sweep
    return stage == ST_P ? c->warmP : (stage == ST_X ? c->warmX : c->warmB);
}
static int64_t &stage_reruns(csr_ctx *c, int stage) {
    return stage == ST_P ? c->rs.reruns_p : (stage == ST_X ? c->rs.reruns_x : c->rs.reruns_b);
}

// F = [[1, f], [0, 1]] (constructMatrixF, core.py:2164-2176): the UF instances of the levelTrend policies (csr_device.h)
static bool unit_f(const Prm &p) { return p.F00 == 1.0 && p.F10 == 0.0 && p.F11 == 1.0; }

// ---- launch idioms shared by the passes ---------------------------------------------------------------------------
// one workgroup per 32-bin tile of every wavefront-group (the tiled conversions between the two layouts)
static dim3 tile_grid(const csr_ctx *c) { return dim3((int)(c->NG * (c->B / 32))); }
// one more array for a tiled conversion launch (k_export_tiled): n of the E components of every `src` record go to `dst`
static ExpDesc &exp_add(ExpList &L, const float *src, float *dst, int E, int n, int skipLast = 0) {
    ExpDesc &d = L.d[L.count++];
    memset(&d, 0, sizeof(d));
    d.src = src;
    d.dst = dst;
    d.E = E;
    d.n = n;
    d.skipLast = skipLast;
    return d;
}
// the side stream continues from this point of the main stream
static int fork_side(csr_ctx *c, hipEvent_t ev) {
    HIPOK(hipEventRecord(ev, c->stream));
    HIPOK(hipStreamWaitEvent(c->side, ev, 0));
    return 0;
}
// NIS / NLL epilogue (D in the reference layout goes through one LDS tile per block)
// natXf: the previous filtered state is read in the reference layout, where the bit-exact state chain wrote it, instead of from the
// blocked xf (p.natD is set; the same tile, the same sums)
static int launch_dstat(csr_ctx *c, const Prm &p, hipStream_t st, const float *natXf = nullptr) {
    void (*kernel)(Prm) = p.natD ? &k_fwd_dstat<true> : &k_fwd_dstat<false>;
    const size_t lds = p.natD ? sizeof(float) * 64 * (c->B + 1) : 0;
    if (natXf == nullptr) return launch(c, "fwd_dstat", "k_fwd_dstat", kernel, dim3((int)c->NG), dim3(256), lds, st, p);
    if (p.natD == nullptr || c->mdl.state_dim != 2 || (c->B % 32) != 0) return fail("internal: NIS / NLL epilogue from the reference-layout xf");
    Prm q = p;
    q.natXfIn = reinterpret_cast<const float2 *>(natXf);
    kernel = &k_fwd_dstat<true, true>;
    return launch(c, "fwd_dstat", "k_fwd_dstat<natXf>", kernel, dim3((int)c->NG), dim3(256), lds, st, q);
}
// per-chain sums of the per-block sums the epilogue (or the chain itself) left
static int launch_chain_sums(csr_ctx *c, const Prm &p, hipStream_t st) {
    return launch(c, "chain_sums", "k_chain_sums", k_chain_sums, dim3((int)c->chains.size()), dim3(1024), 0, st, p, c->dChainFirst,
                  c->dChainNb);
}
// blocked copy of the filtered state from the reference-layout one (which the bit-exact state chain wrote), for `groups`
// wavefront-groups from g0 on; profiled = false: the launch is not counted under a profile scope
static int import_xf_blocked(csr_ctx *c, const Prm &p, hipStream_t st, int64_t g0, int64_t groups, bool profiled = true) {
    float *natXf;
    CHECK(nat_array(c, CSR_ARR_XF, &natXf));
    const dim3 grid((int)(groups * (c->B / 32)));
    return launch(c, profiled ? "state_reblock_out" : nullptr, "k_import_tiled<float2>", k_import_tiled<float2>, grid, dim3(256), 0, st, p,
                  reinterpret_cast<const float2 *>(natXf), p.tXf, g0);
}

// ---- which instance walks a chain ---------------------------------------------------------------------------------
// dynamic LDS of the LDS-DMA ring of a chain policy
template <class DCH>
static constexpr size_t ring_bytes() { return sizeof(unsigned) * DMA_R * DCH::NW * 64; }
struct SpecKernel {
    void (*fn)(Prm) = nullptr;
    size_t lds = 0;
};
// The speculative kernel of chain policy CH for the pass `p` describes (p.warm is set), and its dynamic LDS.  The first test that
// holds decides, and the order matters where noted; pcq (per-chain base process noise) disables every LDS-DMA and
// reference-layout-input form.
// (round 6: the LDS-DMA ring and the reference-layout-input forms exist for F = [[1, f], [0, 1]] only -- what the reference's
// constructMatrixF builds; any other `matrixF` runs the plain-load general instances: same results, fewer kernels to build)
template <class CH>
static SpecKernel spec_kernel(const csr_ctx *c, const Prm &p, bool pcq) {
    if constexpr (CH::DMA) {
        if (c->useDma) return {&k_chain_spec_dma<CH>, ring_bytes<CH>()};
        return {&k_chain_spec<CH>, 0};
    } else {
        const uint32_t mm = p.flags & (F_LAMBDA | F_KAPPA | F_QSCALE);      // which per-bin multipliers the ring carries
        if constexpr (CH::FAMILY == FAM_FWD_FUSED && CH::UNITF) {
            using D0 = FwdTrendFusedDma<0, true>;
            using D1 = FwdTrendFusedDma<1, true>;
            using D2 = FwdTrendFusedDma<2, true>;
            const size_t tl = sizeof(NatTilesFwd);
            if (c->useDmaFused && c->useDmaWarm && p.natOut && !pcq && p.warm > 0) {
                // reference-layout outputs: ring for the warm-up only, tile walker for the main phase
                if (mm == 0) return {&k_chain_spec_dmawarm_natfwd<D0>, std::max(ring_bytes<D0>(), tl)};
                if (mm == F_KAPPA) return {&k_chain_spec_dmawarm_natfwd<D1>, std::max(ring_bytes<D1>(), tl)};
                return {&k_chain_spec_dmawarm_natfwd<D2>, std::max(ring_bytes<D2>(), tl)};
            }
            if (c->useDmaFused && !p.natOut && !pcq && p.ckptOut != nullptr) {
                // warm-started ECM sweep (kappa only is the reference's default loop).  There is no instance without
                // multipliers: mm == 0 runs <2> like everything that is not kappa alone
                if (mm == F_KAPPA) return {&k_chain_spec_dma<D1, true>, ring_bytes<D1>()};
                return {&k_chain_spec_dma<D2, true>, ring_bytes<D2>()};
            }
            if (c->useDmaFused && !p.natOut && !pcq) {
                // ECM sweeps and other passes without reference-layout outputs: inputs through the LDS-DMA ring
                if (mm == 0) return {&k_chain_spec_dma<D0>, ring_bytes<D0>()};
                if (mm == F_KAPPA) return {&k_chain_spec_dma<D1>, ring_bytes<D1>()};
                return {&k_chain_spec_dma<D2>, ring_bytes<D2>()};
            }
        }
        if constexpr (CH::FAMILY == FAM_BWD_TREND && CH::UNITF) {
            using DQ = BwdTrendDma<true, true>;
            using DN = BwdTrendDma<false, true>;
            // reference-layout inputs AND outputs, both through the LDS tiles (the forward pass wrote no blocked xf / Pf): wins over
            // the ring warm-up below, whatever the window
            if (p.natIn && p.natOut && !pcq) {
                if (p.qFromMult) return {&k_smooth_natin<CH, false>, sizeof(NatTiles)};
                return {&k_smooth_natin<CH, true>, sizeof(NatTiles)};
            }
            // smoother with reference-layout outputs: warm-up through the ring, from 64-bin blocks on
            // (32-bin blocks: measured slower, 0.063 vs 0.057 ms -- the ring's fill and drain weigh more than they hide)
            if (c->useDmaFused && c->useDmaWarm && p.natOut && !pcq && p.warm > 0 && c->B >= 64) {
                if (p.qFromMult) return {&k_chain_spec_dmawarm_natbwd<DN>, std::max(ring_bytes<DN>(), sizeof(NatTiles))};
                return {&k_chain_spec_dmawarm_natbwd<DQ>, std::max(ring_bytes<DQ>(), sizeof(NatTiles))};
            }
        }
        if constexpr (CH::NATOUT || CH::NATOUT_FWD) {
            if (p.natOut) {
                if (pcq) return {&k_chain_spec<CH, true, true>, sizeof(NatTiles)};
                return {&k_chain_spec<CH, true, false>, sizeof(NatTiles)};
            }
        }
        if (pcq) return {&k_chain_spec<CH, false, true>, 0};
        // (recording checkpoints has an instance of its own only without per-chain Q: pcq is tested first)
        if (p.ckptOut != nullptr) return {&k_chain_spec<CH, false, false, true>, 0};
        return {&k_chain_spec<CH, false, false>, 0};
    }
}
// ... and the validation / fix-up kernel that goes with it
template <class CH>
static auto fix_kernel(const Prm &p, bool pcq) -> void (*)(Prm, int) {
    if constexpr (CH::NATOUT || CH::NATOUT_FWD) {
        if (p.natOut) return pcq ? &k_chain_fix<CH, true, true> : &k_chain_fix<CH, true, false>;
    }
    return pcq ? &k_chain_fix<CH, false, true> : &k_chain_fix<CH, false, false>;
}

// Speculative pass + validation/fix-up.  defer = true: launch the speculative pass and ONE validation pass and return
// without a host round trip (the stage's monotonic counter is checked at the next settle point); otherwise iterate
// validation passes to the fixed point here.
template <class CH>
static int run_chain(csr_ctx *c, Prm p, const char *name, const char *fixName, int stage, bool defer) {
    static_assert(sizeof(typename CH::Carry) <= 32, "carry buffers are sized for 32 bytes per block");
    int &warmRef = stage_warm(c, stage);
    p.warm = warmRef;
    p.xTolUlps = c->xTolUlps;
    p.rerunCount = reinterpret_cast<unsigned int *>(c->dMail) + stage;
    const int grid = (int)c->NG;
    const bool pcq = CH::USES_Q && p.chainQ != nullptr;      // per-chain base process noise: per-lane model copy
    // consecutive stages alternate between two carry sets; the previous stage's pending check (if any) rides in this
    // stage's speculative kernel
    const int cset = (c->carryToggle ^= 1);
    p.carryIn = c->carrySet[cset][0];
    p.carryOutA = c->carrySet[cset][1];
    take_pending_check(c, p);
    const SpecKernel spec = spec_kernel<CH>(c, p, pcq);
    CHECK(launch(c, name, name, spec.fn, dim3(grid), dim3(64), spec.lds, c->stream, p));
    int which = 0;
    unsigned int *const cnt = reinterpret_cast<unsigned int *>(c->dMail);
    void (*const fix)(Prm, int) = fix_kernel<CH>(p, pcq);
    auto launch_fix = [&](unsigned int *passCounter) -> int {
        p.rerunCountPass = passCounter;
        CHECK(launch(c, fixName, fixName, fix, dim3(grid), dim3(64), 0, c->stream, p, which));
        c->rs.fix_launches++;
        which ^= 1;
        return 0;
    };
    if (defer && c->nPasses[stage] <= 1) {
        // clean so far: no validation kernel -- the next speculative kernel (or read_mail) checks this stage's carries
        c->pendChk.valid = true;
        c->pendChk.kind = CH::KIND;
        c->pendChk.stage = stage;
        c->pendChk.cin = p.carryIn;
        c->pendChk.cout = p.carryOutA;
        c->pendChk.active = p.chainActive;
        c->launchedPasses[stage] = 1;
        return 0;
    }
    if (defer) {
        // optimistic: nPasses validation passes back to back, no host round trip; the stage stands iff the last one re-ran
        // nothing (checked at the next settle point through its own counter)
        p.debugForce = 0;
        const int np = std::max(1, std::min(MAX_DEFER_PASSES, c->nPasses[stage]));
        for (int j = 0; j < np; ++j) CHECK(launch_fix(cnt + MAIL_PASS0 + 4 * stage + j));
        c->launchedPasses[stage] = np;
        return 0;
    }
    // Validation passes are launched in bursts once the first one has re-run blocks: a correction travels one block per
    // pass (bit-exact state chains need hundreds of passes), and reading the counter after every pass costs a host round
    // trip each.  A burst whose passes re-ran nothing at all is the fixed point (a pass without re-runs copies the
    // carries unchanged, so all later ones are empty too); at most burst-1 empty passes are wasted.
    int burst = 1;
    for (int64_t it = 0; it <= c->NB + 1; ++it) {
        p.debugForce = 0;
        for (int rep = 0; rep < burst; ++rep) CHECK(launch_fix(cnt + MAIL_DUMMY));
        CHECK(read_mail(c, MAIL_HDR));
        const unsigned int fresh = take_fresh(c, stage);
        if (c->dbgLog) fprintf(stderr, "[csr] %s iter %lld reruns %u\n", fixName, (long long)it, fresh);
        if (fresh == 0) {
            // re-arm optimistic launches after a few clean synchronous runs in a row (a stage that fails every other time
            // would otherwise pay a pipeline replay every other time)
            if (it == 0 && (stage != ST_X || c->xTolUlps > 0)) {
                if (++c->cleanRuns[stage] >= 4 || c->nPasses[stage] < MAX_DEFER_PASSES) c->optimistic[stage] = true;
            } else if (it > 0) {
                c->cleanRuns[stage] = 0;
            }
            return 0;
        }
        stage_reruns(c, stage) += fresh;
        if (it == 0) grow_warm(c, warmRef, fresh);
        burst = it == 0 ? 2 : std::min(32, burst * 2);
    }
    return fail("%s: speculative fix-up did not reach a fixed point", name);
}

// The chain policy of the model: levelTrend with F = [[1, f], [0, 1]] runs TrendT<true>, any other levelTrend TrendT<false>, the
// level model Level
template <template <bool> class TrendT, class Level>
static int run_policy(csr_ctx *c, const Prm &p, const char *name, const char *fixName, int stage, bool defer) {
    if (c->mdl.state_dim != 2) return run_chain<Level>(c, p, name, fixName, stage, defer);
    if (unit_f(p)) return run_chain<TrendT<true>>(c, p, name, fixName, stage, defer);
    return run_chain<TrendT<false>>(c, p, name, fixName, stage, defer);
}

// ---- warm-started speculation of the ECM sweeps (Prm::ckptIn) -----------------------------------------------------
// Fills the checkpoint fields of `p` for the chain about to be launched in direction fwd / !fwd and returns the window
// variable to use (nullptr: the cold one).  Call ws_launched() after the launch.
static int ws_prepare(csr_ctx *c, Prm &p, bool fwd, int **window) {
    *window = nullptr;
    p.ckptIn = nullptr; p.ckptOut = nullptr; p.ckptSaveWarm = 0;
    if (!c->wsActive || !c->wsEnabled || c->xTolUlps == 0 || p.chainQ != nullptr) return 0;
    // Only the latency-bound batches gain: those the block-length rule gives 32-bin blocks (< 2 M bins: a 1/8-genome shard,
    // 0.64 -> 0.53 ms per ECM iteration).  Larger ones are bandwidth-bound, walk mostly their own block (64 .. 256 bins) and
    // have thousands of wavefront edges -- an edge block that fails costs a replay of the iteration: measured 0.88 -> 1.05 ms
    // on a quarter genome, 2.31 -> 2.46 ms on the genome.
    if (c->B > c->wsMaxBlock) return 0;
    int &warm = fwd ? c->wsWarmF : c->wsWarmB;
    if (warm >= (fwd ? c->warmFM : c->warmB)) return 0;       // widened up to the cold window: nothing left to gain
    void **ck = fwd ? c->ckF : c->ckB;
    for (int k = 0; k < 2; ++k)
        if (!ck[k]) { char *q; CHECK(dalloc(c, &q, c->NB * 32)); ck[k] = q; }
    const int saved = fwd ? c->wsSavedF : c->wsSavedB;
    const int sweep = fwd ? c->wsSweepF : c->wsSweepB;
    p.ckptOut = ck[(sweep + 1) & 1];
    p.ckptSaveWarm = warm;
    p.localFixCount = reinterpret_cast<unsigned int *>(c->dMail) + MAIL_LOCAL;
    if (!c->wsCold && saved == warm && saved > 0) {
        p.ckptIn = ck[sweep & 1];
        *window = &warm;
    }
    return 0;
}
static void ws_launched(csr_ctx *c, const Prm &p, bool fwd) {
    if (p.ckptOut == nullptr) return;
    if (fwd) { c->wsSavedF = p.ckptSaveWarm; c->wsSweepF += 1; }
    else { c->wsSavedB = p.ckptSaveWarm; c->wsSweepB += 1; }
}

// ---- superblock view of the batch (bit-exact state chain) -------------------------------------------------------
static int ensure_sb_view(csr_ctx *c) {
    csr_ctx::SbView &v = c->sb;
    if (v.ready) return 0;
    int B = c->sbBins;
    const int nc = (int)c->chains.size();
    if (!c->sbBinsPinned) {
        // one wavefront per superblock, at most one wavefront per SIMD: the shortest superblock (a multiple of 8192 bins) that
        // leaves no more superblocks than 5/8 of the device's SIMDs (measured at genome scale: 16 384 bins 7.2 ms, 24 576 / 32 768
        // bins 7.0 ms, 8 192 bins 8.3 ms per step -- fewer, longer repair passes win slightly while a pass costs the slowest
        // superblock's walk)
        hipDeviceProp_t prop;
        int simds = 1024;
        if (hipGetDeviceProperties(&prop, c->device) == hipSuccess && prop.multiProcessorCount > 0) simds = 4 * prop.multiProcessorCount * 5 / 8;
        for (;; B += 8192) {
            int64_t cnt = 0;
            for (int i = 0; i < nc; ++i) cnt += (c->chains[i].n + B - 1) / B;
            if (cnt <= simds || B >= (1 << 20)) break;
        }
    }
    std::vector<int64_t> first((size_t)nc);
    int64_t nb = 0;
    for (int i = 0; i < nc; ++i) {
        first[(size_t)i] = nb;
        nb += (c->chains[i].n + B - 1) / B;
    }
    std::vector<int4> blk((size_t)nb);
    std::vector<int> bch((size_t)nb);
    for (int i = 0; i < nc; ++i) {
        const ChainInfo &ci = c->chains[i];
        const int64_t cnt = (ci.n + B - 1) / B;
        for (int64_t k = 0; k < cnt; ++k) {
            int4 e;
            e.x = (int)(ci.off + k * B);
            e.y = (int)std::min<int64_t>(B, ci.n - k * B);
            e.z = (int)first[(size_t)i];
            e.w = (int)(first[(size_t)i] + cnt - 1);
            blk[(size_t)(first[(size_t)i] + k)] = e;
            bch[(size_t)(first[(size_t)i] + k)] = i;
        }
    }
    v.B = B; v.NB = nb; v.NG = (nb + 63) / 64; v.TN = v.NG * (int64_t)B * 64;
    CHECK(dalloc(c, &v.blk, nb)); CHECK(dalloc(c, &v.blkChain, nb)); CHECK(dalloc(c, &v.chainFirst, nc));
    HIPOK(hipMemcpyAsync(v.blk, blk.data(), sizeof(int4) * nb, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemcpyAsync(v.blkChain, bch.data(), sizeof(int) * nb, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemcpyAsync(v.chainFirst, first.data(), sizeof(int64_t) * nc, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));           // the host vectors go out of scope
    char *q[3];
    for (char *&x : q) CHECK(dalloc(c, &x, nb * 32));
    v.carryIn = q[0]; v.carryOutA = q[1]; v.carryOutB = q[2];
    v.ready = true;
    return 0;
}

// A reader needs the blocked copies of arrays whose resident result may stand in the reference layout only (xf / Pf in front of a
// smoother that reads blocks, xs / Ps / lag in front of a MASKED pass that rewrites the blocks of its own chains only): those that
// are not .blocked come back through LDS tiles.  (A masked import leaves the other chains stale.)
static int need_blocked(csr_ctx *c, std::initializer_list<int> ids, const unsigned char *active) {
    bool any = false;
    for (int id : ids) any = any || !c->where[id].blocked;
    if (!any) return 0;
    Prm p = c->p;
    p.chainActive = active;
    const dim3 grid = tile_grid(c);
    Scope sc(c, "state_reblock_out");
    for (int id : ids) {
        if (c->where[id].blocked) continue;
        const float *src = c->nat[id];
        if (id == CSR_ARR_D)
            CHECK(launch(c, nullptr, "k_import_tiled<float>", k_import_tiled<float>, grid, dim3(256), 0, c->stream, p, src, p.tD, (int64_t)0));
        else if (id == CSR_ARR_XF || id == CSR_ARR_XS)
            CHECK(launch(c, nullptr, "k_import_tiled<float2>", k_import_tiled<float2>, grid, dim3(256), 0, c->stream, p,
                         reinterpret_cast<const float2 *>(src), id == CSR_ARR_XF ? p.tXf : p.tXs, (int64_t)0));
        else
            CHECK(launch(c, nullptr, "k_import_tiled<float4>", k_import_tiled<float4>, grid, dim3(256), 0, c->stream, p,
                         reinterpret_cast<const float4 *>(src), id == CSR_ARR_PF ? p.tPf : (id == CSR_ARR_PS ? p.tPs : p.tLag), (int64_t)0));
        if (active == nullptr) c->where[id].blocked = true;
    }
    return 0;
}

// Bit-exact state chain, systolic form (k_sb_sys): the gain / statistics records go to the natural layout (one tiled
// conversion launch), one wavefront per superblock walks 64 bins per batch as a shift register and writes the filtered state
// straight into the reference-layout xf array; superblocks start from the cold prior and the validation / repair passes run
// to the fixed point (= the sequential recursion, whatever the superblock length); one tiled launch brings the filtered state
// back into the batch's blocked layout for the epilogue and the smoother.
static int early_cov_exports(csr_ctx *c, const Prm &p, uint32_t flags, bool withPf);
// The three forms of the chain, each in the instance of a pass's `mode`
static void (*const g_sbSys[3])(Prm, const float4 *, const float4 *, float2 *) = {&k_sb_sys<0>, &k_sb_sys<1>, &k_sb_sys<2>};
static void (*const g_sbDelta[3])(Prm, const float4 *, const float4 *, float2 *, int, int) = {&k_sb_delta<0>, &k_sb_delta<1>, &k_sb_delta<2>};
static void (*const g_sbAsync[3])(Prm, const float4 *, const float4 *, float2 *, SbAsync) = {&k_sb_async<0, false>, &k_sb_async<1, false>,
                                                                                            &k_sb_async<2, false>};
// The chain up to and including the launch of the barrier-free kernel (k_sb_async; CONSENRICH_AMD_SB_ASYNC=0: nothing is launched);
// c->sbp holds what sb_finish needs.  watch (step_pipelined, a step that pipelines its tail per chain): the kernel sets a host-visible
// "done" word per chain, the side stream continues from the point right in front of it, c->sbp.active says that the chain is in flight.
static int sb_begin(csr_ctx *c, const Prm &p, bool earlyExports, uint32_t flags, bool watch) {
    CHECK(ensure_sb_view(c));
    CHECK(flush_pending_check(c));
    csr_ctx::SbView &v = c->sb;
    CHECK(ensure_sb_nat(c));
    float *natXf;
    CHECK(nat_array(c, CSR_ARR_XF, &natXf));
    if (!(c->gainNat && c->natSZValid)) {
        ExpList L;
        memset(&L, 0, sizeof(L));
        // the gain records of this pass unless the covariance chain wrote them in the reference layout itself (forward_impl); the
        // statistics records {S0, zbar} only when the statistics changed since they were last converted (csr_batch_stats): the
        // sweeps of an ECM iteration share them
        if (!c->gainNat) exp_add(L, reinterpret_cast<const float *>(p.tXin), reinterpret_cast<float *>(c->sbNatGain), 4, 4);
        Prm pe = p;
        if (!c->natSZValid) {
            exp_add(L, reinterpret_cast<const float *>(p.tSZ), reinterpret_cast<float *>(c->sbNatSZ), 4, 4);
            pe.chainActive = nullptr;       // the statistics of EVERY chain (csr_batch_stats computed them all), whatever this pass masks
            c->natSZValid = true;
        }
        CHECK(launch(c, "state_records_natural", "k_export_tiled (state records)", k_export_tiled, tile_grid(c), dim3(256), 0, c->stream, pe, L));
    }
    if (earlyExports) CHECK(early_cov_exports(c, p, flags, true));
    csr_ctx::SbPending &s = c->sbp;
    s.active = s.launched = false;
    s.watch = watch;
    s.p = s.q = p;
    Prm &q = s.q;
    q.B = v.B; q.NB = v.NB; q.NG = v.NG; q.blk = v.blk; q.blkChain = v.blkChain;
    q.carryIn = v.carryIn; q.carryOutA = v.carryOutA; q.carryOutB = v.carryOutB;
    unsigned int *const cnt = reinterpret_cast<unsigned int *>(c->dMail);
    q.rerunCount = cnt + ST_X;
    q.rerunCountPass = cnt + MAIL_DUMMY;
    q.prevKind = CK_NONE; q.sbDbg = nullptr;
    s.mode = unit_f(p) ? (p.F01 == 1.0 ? 2 : 1) : 0;     // F01 == 1: the walker's predicted level is one float32 add
    s.grid = (int)((v.NB + 3) / 4);
    s.xf = reinterpret_cast<float2 *>(natXf);
    if (!c->sbAsync) return 0;
    // the whole chain in one launch, no barrier between passes (k_sb_async); a bail-out (a bounded wait ran out) makes sb_finish run
    // the pass form, which starts over from the cold prior
    if (!v.pub) { CHECK(dalloc(c, &v.pub, 2 * v.NB + 2)); }
    SbAsync a;
    a.carry = v.pub; a.vf = v.pub + v.NB; a.ctl = reinterpret_cast<unsigned int *>(v.pub + 2 * v.NB);
    a.spinLimit = c->sbSpinLimit;
    a.hostDone = nullptr;
    if (watch) {
        // (nothing of this context is in flight that writes these words: the previous launch was waited for)
        if (!c->hDone) {
            // (coherent = fine-grained: a system-scope store of the running kernel is visible to the polling host at once,
            // whatever HIP_HOST_COHERENT says)
            CHECK(c->hDone.alloc(c->chains.size(), hipHostMallocCoherent | hipHostMallocMapped));
            HIPOK(hipHostGetDevicePointer((void **)&c->dDone, c->hDone, 0));
        }
        for (size_t i = 0; i < c->chains.size(); ++i) c->hDone[i] = 0u;
        a.hostDone = c->dDone;
    }
    HIPOK(hipMemsetAsync(v.pub, 0, sizeof(unsigned long long) * (size_t)(2 * v.NB + 2), c->stream));
    // (the repair runs' LDS ring: > 64 KB of dynamic LDS has to be asked for once per kernel)
    if (!c->sbAsyncLdsRaised[s.mode]) {
        HIPOK(hipFuncSetAttribute(reinterpret_cast<const void *>(g_sbAsync[s.mode]), hipFuncAttributeMaxDynamicSharedMemorySize, (int)SB_ASYNC_LDS));
        c->sbAsyncLdsRaised[s.mode] = true;
    }
    // (a pipelined step's NIS / NLL epilogue groups run on the side stream while this launch runs: the side stream continues
    // from HERE, behind the statistics and the covariance chain the epilogue reads; a chain's done word is the rest)
    if (watch) CHECK(fork_side(c, c->evEpiFork));
    CHECK(launch(c, "fwd_state_chain", "k_sb_async", g_sbAsync[s.mode], dim3(s.grid), dim3(256), SB_ASYNC_LDS, c->stream, q, c->sbNatGain,
                 c->sbNatSZ, s.xf, a));
    s.ctl = a.ctl;
    s.launched = true;
    s.active = watch;
    return 0;
}

// Everything behind sb_begin: the verdict of the single launch (or, when it bailed out or never went out, the pass form k_sb_sys),
// the repair passes to the fixed point (= the sequential recursion, whatever the superblock length), and with `reblock` the blocked
// copy of the filtered state for the whole batch (a pipelined step makes it per group of chains, where one is needed at all).
static int sb_finish(csr_ctx *c, bool reblock) {
    csr_ctx::SbPending &s = c->sbp;
    const csr_ctx::SbView &v = c->sb;
    s.active = false;
    bool done = false;
    if (std::exchange(s.launched, false)) {
        unsigned int ctl[4];
        HIPOK(hipMemcpyAsync(ctl, s.ctl, sizeof(ctl), hipMemcpyDeviceToHost, c->stream));
        HIPOK(wait_stream(c, 1));
        c->rs.fix_launches++;
        if (ctl[1] == 0) {
            done = true;
            c->rs.reruns_x += ctl[2];
            if (c->dbgLog) fprintf(stderr, "[csr] fwd_state_chain (barrier-free superblocks): %u delta runs, %u abandoned; superblock %d bins, %lld superblocks\n",
                                   ctl[2], ctl[3], v.B, (long long)v.NB);
        } else {
            c->rs.sb_bailouts++;
            if (c->dbgLog) fprintf(stderr, "[csr] fwd_state_chain (barrier-free superblocks): bailed out, running the pass form\n");
            // (a pipelined step may have tails of finished chains in flight that read the track the pass form rewrites, and epilogue
            // groups on the side stream that read it: this is the one place that waits for them)
            if (s.watch) HIPOK(hipStreamSynchronize(c->tail));
            if (s.watch) HIPOK(hipStreamSynchronize(c->side));
        }
    }
    if (!done)
        CHECK(launch(c, "fwd_state_chain", "k_sb_sys", g_sbSys[s.mode], dim3(s.grid), dim3(256), 0, c->stream, s.q, c->sbNatGain, c->sbNatSZ, s.xf));
    int which = 0, burst = 2;
    const int adv = (c->sbAdvMin << 8) | (c->sbAdvFrom << 16);
    for (int64_t it = 0; it <= v.NB + 1 && !done; ++it) {
        {
            // repair passes in delta form (k_sb_delta): a burst of them under ONE profile scope
            Scope sc(c, "fwd_state_fix");
            for (int rep = 0; rep < burst; ++rep) {
                CHECK(launch(c, nullptr, "k_sb_delta", g_sbDelta[s.mode], dim3(s.grid), dim3(256), 0, c->stream, s.q, c->sbNatGain, c->sbNatSZ, s.xf,
                             which, adv));
                which ^= 1;
                c->rs.fix_launches++;
            }
        }
        CHECK(read_mail(c, MAIL_HDR));
        const unsigned int fresh = take_fresh(c, ST_X);
        if (c->dbgLog) fprintf(stderr, "[csr] fwd_state_fix (systolic superblocks) iter %lld reruns %u\n", (long long)it, fresh);
        if (fresh == 0) done = true;
        c->rs.reruns_x += fresh;
        burst = c->dbgLog ? 1 : std::min(32, burst * 2);
    }
    if (!done) return fail("fwd_state_chain (systolic superblocks): fix-up did not reach a fixed point");
    if (reblock) CHECK(import_xf_blocked(c, s.p, c->stream, 0, c->NG));
    produced(c, {CSR_ARR_XF}, W_BLOCKED | W_NAT);
    return 0;
}
static int state_chain_systolic(csr_ctx *c, const Prm &p, bool earlyExports, uint32_t flags) {
    CHECK(sb_begin(c, p, earlyExports, flags, false));
    return sb_finish(c, true);
}

// Join the side stream.  The per-chain sums (22 workgroups of 1024 threads, ~10 us) run on the main stream after the
// join: left on the side stream behind the epilogue they starve for whole-CU slots while a bandwidth-bound kernel of the
// main stream keeps the chip full (measured 0.64 ms instead of 0.01).
static int join_side(csr_ctx *c) {
    if (c->sidePending) {
        (void)hipStreamWaitEvent(c->stream, c->evJoin, 0);
        c->sidePending = false;
        if (c->sideSumsDone) { c->sideSumsDone = false; return 0; }    // the side stream ran the per-chain sums itself
        CHECK(launch_chain_sums(c, c->sidePrm, c->stream));
    }
    return 0;
}

// NIS/NLL epilogue; side = true runs it on the side stream (forked after the state chain) so that it overlaps the
// latency-bound smoother chain.
static int forward_epilogue(csr_ctx *c, const Prm &p, bool side) {
    hipStream_t st = c->stream;
    if (side) {
        CHECK(join_side(c));
        CHECK(fork_side(c, c->evFork));
        st = c->side;
    }
    CHECK(launch_dstat(c, p, st));
    if (side) {
        HIPOK(hipEventRecord(c->evJoin, c->side));
        c->sidePending = true;
        c->sidePrm = p;                 // k_chain_sums follows on the main stream at the join
        return 0;
    }
    return launch_chain_sums(c, p, st);
}

// main stream waits for the early covariance exports of the side stream (early_cov_exports)
static void join_pf(csr_ctx *c) {
    if (c->pfPending) {
        (void)hipStreamWaitEvent(c->stream, c->evPf, 0);
        c->pfPending = false;
    }
}
// constant process noise as rows of the reference-layout array (skipped when the array already holds exactly this fill)
static void pn_fill_values(const csr_ctx *c, const Prm &p, float q[4]) {
    q[0] = (float)p.Q00;
    q[1] = c->mdl.state_dim == 2 ? (float)p.Q01 : 0.f;
    q[2] = c->mdl.state_dim == 2 ? (float)p.Q10 : 0.f;
    q[3] = c->mdl.state_dim == 2 ? (float)p.Q11 : 0.f;
}
static bool pn_fill_current(const csr_ctx *c, const Prm &p) {
    float q[4];
    pn_fill_values(c, p, q);
    return c->pnFillValid && c->nat[CSR_ARR_PNOISE] != nullptr && memcmp(q, c->pnFillQ, sizeof(q)) == 0;
}
static int launch_pn_fill(csr_ctx *c, const Prm &p, float *dst, hipStream_t st) {
    const int nm = c->mdl.state_dim * c->mdl.state_dim;
    const unsigned grid = (unsigned)std::min<int64_t>((c->Npad + 255) / 256, 8192);
    float q[4];
    pn_fill_values(c, p, q);
    // (a level model's row is q[0] alone: pn_fill_values left the other three at zero)
    void (*const kernel)(float *, int64_t, float, float, float, float) = nm == 4 ? &k_fill_rows<4> : &k_fill_rows<1>;
    CHECK(launch(c, "export_natural", "k_fill_rows", kernel, dim3(grid), dim3(256), 0, st, dst, c->Npad, q[0], q[1], q[2], q[3]));
    memcpy(c->pnFillQ, q, sizeof(q));
    c->pnFillValid = true;
    return 0;
}
// the same rows in the blocked layout, for every chain (forward_impl: in front of a masked pass with per-bin process noise)
static int launch_pn_fill_blocked(csr_ctx *c) {
    float q[4];
    pn_fill_values(c, c->p, q);
    return launch(c, "pnoise_blocked_fill", "k_fill_blocked_q", k_fill_blocked_q, dim3(grid_slots(c)), dim3(256), 0, c->stream, c->p, c->p.tQ,
                  make_float4(q[0], q[1], q[2], q[3]));
}

// Bit-exact mode: the state chain keeps at most 5/8 of the SIMDs busy for milliseconds and is bound by latency, not by
// bandwidth.  The reference-layout outputs that depend on the covariance chain alone -- Pf, and the process noise when it
// is one constant matrix -- are written on the side stream underneath it instead of after the smoother.
static int early_cov_exports(csr_ctx *c, const Prm &p, uint32_t flags, bool withPf = true) {
    const int nm = c->mdl.state_dim * c->mdl.state_dim;
    const bool constFlags = !(flags & (F_APN | F_QSCALE | F_KAPPA));
    const bool constQ = constFlags && p.chainQ == nullptr;
    // (round 4: with Pf also the process noise that is NOT one constant matrix -- per-bin multipliers: the covariance chain
    // stored it; per-chain base matrices: a table -- so that a step with multipliers pipelines its tail as well)
    const bool convQ = withPf && !constQ;
    if (!withPf && !constQ) return 0;
    const bool doPf = withPf && !c->where[CSR_ARR_PF].nat;      // (the covariance chain may have written Pf in the reference layout itself)
    const bool fill = constQ && !pn_fill_current(c, p);
    if (constQ) produced(c, {CSR_ARR_PNOISE}, W_NAT);           // (filled below unless the array already holds this constant fill)
    if (!doPf && !fill && !convQ) return 0;
    // (a reference-layout array is allocated -- and zeroed ON THE MAIN STREAM -- at its first use: before the fork, so that the
    // side stream's writes are ordered behind the zeroing)
    float *dstPf = nullptr, *dstPn = nullptr;
    if (doPf) CHECK(nat_array(c, CSR_ARR_PF, &dstPf));
    if (fill || convQ) CHECK(nat_array(c, CSR_ARR_PNOISE, &dstPn));
    CHECK(fork_side(c, c->evFork2));
    if (doPf || convQ) {
        ExpList L;
        memset(&L, 0, sizeof(L));
        if (doPf) exp_add(L, reinterpret_cast<const float *>(p.tPf), dstPf, 4, nm);
        if (convQ) {            // (as export_impl describes it)
            ExpDesc &e = exp_add(L, constFlags ? nullptr : reinterpret_cast<const float *>(p.tQ), dstPn, 4, nm, 1);
            if (constFlags) pn_fill_values(c, p, e.cval);
        }
        CHECK(launch(c, "export_natural", "k_export_tiled (early Pf)", k_export_tiled, tile_grid(c), dim3(256), 0, c->side, p, L));
    }
    if (doPf) c->where[CSR_ARR_PF].nat = true;
    if (convQ) { produced(c, {CSR_ARR_PNOISE}, W_BLOCKED | W_NAT); c->pnFillValid = false; }
    if (fill) CHECK(launch_pn_fill(c, p, dstPn, c->side));
    HIPOK(hipEventRecord(c->evPf, c->side));
    c->pfPending = true;
    return 0;
}

// split: the caller pipelines everything behind the bit-exact state chain per group of chains (step_pipelined); if that chain
// went out as one barrier-free launch the pass returns right behind it (c->sbp.active) without the NIS / NLL epilogue.
static int forward_impl(csr_ctx *c, const FwdPass &pass) {
    const uint32_t flags = pass.flags;
    const bool wantD = pass.wantD, natOut = pass.natOut, side = pass.side, split = pass.split;
    const unsigned char *const active = pass.active;
    if (!c->statsValid) return fail("csr_batch_stats must run before the forward pass");
    // the resident statistics carry {S2c, log R} as a float32 pair (computed in the 2-ulp mode) and the context is back in the
    // bit-exact mode: that mode's D / NLL / lambda E-step promise float64 statistics -- recompute them
    if (c->p.statsF32 && c->xTolUlps == 0) CHECK(csr_batch_stats(c));
    // a MASKED pass rewrites the blocked xf / Pf of its own chains only: when the resident pass left them in the reference layout
    // alone, the chains outside the mask get their blocked copies back first (they keep their resident results)
    // (whether or not new statistics have invalidated those results since: the masked chains get new ones, the others keep the old)
    // (the same for the NIS / NLL track: an epilogue that wrote D straight into the reference layout left the blocked D of every
    // chain stale, and the next export converts the blocked D of every chain)
    if (active != nullptr) CHECK(need_blocked(c, {CSR_ARR_D, CSR_ARR_XF, CSR_ARR_PF}, nullptr));
    // ... and for the process noise: the resident pass ran with one constant matrix per chain and stored no rows; a masked pass
    // with per-bin process noise stores the rows of ITS chains, and the export that follows converts the blocked rows of every chain
    if (active != nullptr && const_q(c) && (flags & (F_APN | F_QSCALE | F_KAPPA))) CHECK(launch_pn_fill_blocked(c));
    c->sbp.active = false;
    join_pf(c);         // (an early export nobody asked for afterwards still reads the arrays this pass overwrites)
    new_forward_pass(c);
    c->gainNat = false;
    Prm p = c->p;
    p.flags = flags;
    p.chainActive = active;
    if (pass.kappaIn) p.tKap = pass.kappaIn;                          // ECM sweep: the kappa of the previous sweep's E-step
    p.qFromMult = (flags & (F_APN | F_QSCALE | F_KAPPA)) ? 0 : 1;     // constant process noise: pNoise is not stored
    // inner ECM sweeps: only the smoother reads this pass's pNoise (diagonal base process noise: its two diagonal entries,
    // 8 B instead of 16) and nobody its predicted variance (no NIS/NLL epilogue)
    p.qFromKappa = (pass.sweep && !p.qFromMult && !(flags & F_APN) && c->qDiagonal) ? 1 : 0;
    p.storePP = (wantD || !pass.sweep) ? 1 : 0;
    c->fwdQCompact = p.qFromKappa != 0;
    const bool defer = pass.defer && c->deferEnabled;
    c->last.fwd = pass;
    const bool seq = (flags & F_APN) && !(flags & F_QSCALE);
    if (seq) {
        CHECK(launch(c, "fwd_apn_sequential", "k_fwd_apn", k_fwd_apn, dim3(((int)c->chains.size() + 63) / 64), dim3(64), 0, c->stream, p,
                     c->dChainFirst, c->dChainNb));
    } else {
        bool dP = defer && c->optimistic[ST_P], dX = defer && c->optimistic[ST_X];
        bool nisInChain = false;
        if (wantD && natOut) {          // D straight into the reference layout
            const size_t tileBytes = sizeof(float) * 64 * (size_t)(c->B + 1);
            bool ok = true;
            if (tileBytes > 48 * 1024 && !c->dstatLdsRaised) {      // 256-bin blocks: 65.8 KB of dynamic LDS
                ok = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_fwd_dstat<true>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)tileBytes) == hipSuccess &&
                     hipFuncSetAttribute(reinterpret_cast<const void *>(&k_fwd_dstat<true, true>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)tileBytes) == hipSuccess;
                (void)hipGetLastError();
                c->dstatLdsRaised = ok;
            }
            if (ok) {
                CHECK(nat_array(c, CSR_ARR_D, &p.natD));
                produced(c, {CSR_ARR_D}, W_NAT);
            }
        }
        // Fused chain (tolerant mode).  Its state recursion warms up on SPECULATIVE gains (the split state chain reads the
        // validated ones), so with per-bin multipliers (the ECM loop: kappa per bin) a few blocks need about covariance-window +
        // state-window bins.  Round 1 ran every block with a 160-bin window for them (a failed validation cost a whole
        // pipeline).  With up to four confirmation passes per stage (check_stages) the few blocks that need more are simply
        // repaired: the window starts 16 bins above the plain one (96: ECM iteration 3.01 -> 2.85 ms at genome scale, 1.02 ->
        // 0.88 ms on a 1/8-genome shard) and widens itself like the others when many blocks fail.
        if (c->xTolUlps > 0) {
            // one stage (counter of the covariance stage; the window covers the state chain's needs too)
            const bool mult = (flags & (F_KAPPA | F_LAMBDA | F_QSCALE)) != 0;
            if (c->warmP < c->warmX) c->warmP = c->warmX;
            if (c->warmFM < c->warmP + 16 && !c->pinFM) c->warmFM = c->warmP + 16;
            c->fwdWindow = mult ? &c->warmFM : &c->warmP;
            dX = false;
            p.predCompact = c->mdl.state_dim == 2 ? 1 : 0;
            if (!natOut && mult && c->mdl.state_dim == 2) {        // ECM sweep: window from the previous sweep's carries
                int *w = nullptr;
                CHECK(ws_prepare(c, p, true, &w));
                if (w) c->fwdWindow = w;
            }
            if (natOut && c->mdl.state_dim == 2) {      // xf / Pf also in the reference layout
                CHECK(nat_array(c, CSR_ARR_XF, &p.natXs));
                CHECK(nat_array(c, CSR_ARR_PF, &p.natPs));
                p.natOut = 1;
                produced(c, {CSR_ARR_XF, CSR_ARR_PF}, W_BLOCKED | W_NAT);
                // the constant process noise depends on nothing: its reference-layout rows are filled on the side stream beside
                // the (latency-bound) forward chain instead of after the smoother
                if (active == nullptr) CHECK(early_cov_exports(c, p, flags, false));
                // NIS / NLL inside the chain's tile walker (csr_device.h FwdTrendFusedT::step_nis): no epilogue kernel, no
                // predicted-variance track.  (Per-bin NLL in D keeps the epilogue: its log terms belong off the serial path.)
                if (wantD && p.natD != nullptr && !(flags & F_NLL_IN_D)) {
                    p.nisInChain = 1;
                    p.storePP = 0;
                    nisInChain = true;
                }
                // constant process noise and nobody left to read the blocked xf / Pf but the smoother (which then reads the
                // reference-layout arrays through its tiles): the tile walker stores nothing in the blocked layout
                if (p.qFromMult && p.chainQ == nullptr && (nisInChain || !wantD) && (c->B % 8) == 0 && unit_f(p)) {
                    p.natOnly = 1;
                    produced(c, {CSR_ARR_XF, CSR_ARR_PF}, W_NAT);
                }
            }
            CHECK((run_policy<FwdTrendFusedT, FwdLevelFused>(c, p, "fwd_chain", "fwd_fix", ST_P, dP)));
            ws_launched(c, p, true);
            p.ckptIn = nullptr; p.ckptOut = nullptr; p.ckptSaveWarm = 0;
            c->lastFwdWindow = c->fwdWindow;
            c->fwdWindow = nullptr;
        } else if (c->mdl.state_dim == 2) {
            c->lastFwdWindow = nullptr;
            // bit-exact mode: the superblock state chain, or the sequential yardstick (CONSENRICH_AMD_SEQ_STATE=1)
            const bool seqX = c->seqState;
            // (the covariance chain is validated optimistically here too: a failed validation is as rare as in the 2-ulp mode and
            // costs the same replay of the pass.  The sequential yardstick keeps the host round trip.)
            if (seqX) dP = false;
            Prm pc = p;
            if (!seqX) {
                // the superblock state chain reads its records in the reference layout: the covariance chain writes the gain
                // records there itself (and Pf, when this pass's Pf is an output), through LDS tiles -- no conversion launch
                // between the two chains; the NIS epilogue reads P00pred from the compact track instead of the blocked record
                CHECK(ensure_sb_nat(c));
                p.predCompact = 1;
                pc = p;
                pc.natOut = 1;
                pc.natLag = reinterpret_cast<float *>(c->sbNatGain);
                pc.natPs = nullptr;
                if (natOut && active == nullptr) {
                    CHECK(nat_array(c, CSR_ARR_PF, &pc.natPs));
                    produced(c, {CSR_ARR_PF}, W_BLOCKED | W_NAT);
                    // a pipelined step with one constant process noise: the smoother of every group reads xf / Pf in the reference
                    // layout (k_smooth_natin) -- no blocked copy of Pf
                    if (split && p.qFromMult && p.chainQ == nullptr && (c->B % 8) == 0 && unit_f(p)) {
                        pc.natOnly = 1;
                        produced(c, {CSR_ARR_PF}, W_NAT);
                    }
                }
                c->gainNat = true;
            }
            CHECK((run_policy<FwdPTrendT, FwdPLevel>(c, pc, "fwd_cov_chain", "fwd_cov_fix", ST_P, dP)));     // (state_dim is 2 here)
            if (seqX) {
                // bit-exact mode: the state recursion cannot be validated speculatively in reasonable time (see
                // k_state_seq_trend) -- one wavefront per chain runs it sequentially on the validated gains
                void (*const kernel)(Prm, const int64_t *, const int64_t *) = unit_f(p) ? &k_state_seq_trend<true> : &k_state_seq_trend<false>;
                CHECK(launch(c, "fwd_state_seq", "k_state_seq_trend", kernel, dim3((unsigned)c->chains.size()), dim3(64), 0, c->stream, p,
                             c->dChainFirst, c->dChainNb));
                dX = false;
            } else {
                // (the early covariance exports fork off behind the state chain's own record conversion)
                const bool early = natOut && active == nullptr;
                if (split && c->sbAsync) CHECK(sb_begin(c, p, early, flags, true));
                else CHECK(state_chain_systolic(c, p, early, flags));
                dX = false;
            }
        } else {
            CHECK(run_chain<FwdPLevel>(c, p, "fwd_cov_chain", "fwd_cov_fix", ST_P, dP));
            CHECK(run_chain<FwdXLevel>(c, p, "fwd_state_chain", "fwd_state_fix", ST_X, dX));
        }
        if (wantD && nisInChain) {
            // the chain kernels left D and the per-block sums: only the per-chain reduction follows -- beside the smoother (side
            // stream) when one follows, so that its few microseconds leave the critical path
            CHECK(join_side(c));
            hipStream_t st = c->stream;
            if (side && c->deferEnabled) {
                CHECK(fork_side(c, c->evFork));
                st = c->side;
            }
            CHECK(launch_chain_sums(c, p, st));
            if (st == c->side) {
                HIPOK(hipEventRecord(c->evJoin, c->side));
                c->sidePending = true;
                c->sideSumsDone = true;         // join_side only waits
            }
        } else
        if (wantD && !c->sbp.active) CHECK(forward_epilogue(c, p, side && c->deferEnabled));
        if (dP || dX) c->last.fwdPending = true;
    }
    c->haveFwd = true;
    c->haveBwd = false;
    c->fwdInternal = true;
    return 0;
}

// (the lag-one covariance is produced by the smoother's own main phase: there is no pass without it)
static int backward_impl(csr_ctx *c, const BwdPass &pass) {
    if (!c->haveFwd) return fail("forward results are not resident: run csr_batch_forward first");
    const unsigned char *const active = pass.active;
    const int estep = pass.estep;
    const bool preferNatIn = pass.preferNatIn;
    Prm p = c->p;
    p.flags = c->last.fwd.flags;
    p.chainActive = active;
    p.estepKappa = estep != 0 ? 1 : 0;
    p.storeMoments = estep == 2 ? 0 : 1;
    if (pass.kappaIn) p.tKap = pass.kappaIn;
    p.tKapOut = pass.kappaOut ? pass.kappaOut : p.tKap;
    p.qFromKappa = c->fwdQCompact ? 1 : 0;       // the resident forward pass stored qf instead of pNoise
    c->last.bwd = pass;
    const bool natOut = pass.natOut && c->mdl.state_dim == 2;      // the smoother writes the reference layout directly
    if (natOut) {
        CHECK(nat_array(c, CSR_ARR_XS, &p.natXs));
        CHECK(nat_array(c, CSR_ARR_PS, &p.natPs));
        CHECK(nat_array(c, CSR_ARR_LAG, &p.natLag));
        p.natOut = 1;
    }
    // preferNatIn (a group's tail of a pipelined step): the reference-layout xf / Pf of these chains stand -- read them there
    // even though a blocked xf is on its way for the epilogue
    const csr_ctx::Where xfW = c->where[CSR_ARR_XF], pfW = c->where[CSR_ARR_PF];
    const bool need = !xfW.blocked || !pfW.blocked;
    if (need || preferNatIn) {
        const bool pcq = p.chainQ != nullptr;
        const bool natValid = pfW.nat && (xfW.nat || preferNatIn);
        if (c->natInEnabled && natOut && !pcq && !p.qFromKappa && natValid && (need || const_q(c)) && (stage_warm(c, ST_B) % 8) == 0 &&
            unit_f(p)) {
            float *natXf, *natPf;
            CHECK(nat_array(c, CSR_ARR_XF, &natXf));
            CHECK(nat_array(c, CSR_ARR_PF, &natPf));
            p.natIn = 1;
            p.natXfIn = reinterpret_cast<const float2 *>(natXf);
            p.natPfIn = reinterpret_cast<const float4 *>(natPf);
        } else {
            CHECK(need_blocked(c, {CSR_ARR_XF, CSR_ARR_PF}, active));
        }
    }
    new_smoothed_fit(c);
    if (natOut) produced(c, {CSR_ARR_XS, CSR_ARR_PS, CSR_ARR_LAG}, W_NAT);   // this smoother writes the reference layout only
    p.qFromMult = const_q(c) ? 1 : 0;       // constant process noise: the smoother need not read pNoise at all
    const bool dB = pass.defer && c->deferEnabled && c->optimistic[ST_B];
    if (!natOut && c->mdl.state_dim == 2 && estep != 0) {       // ECM sweep: window from the previous sweep's carries
        int *w = nullptr;
        CHECK(ws_prepare(c, p, false, &w));
        c->bwdWindow = w;
    }
    struct BwdWindowReset { csr_ctx *c; ~BwdWindowReset() { c->bwdWindow = nullptr; } } bwdWindowReset{c};
    if (p.qFromKappa && natOut) return fail("internal: compact process noise is only produced by ECM sweeps (no reference-layout outputs)");
    if (p.qFromKappa) CHECK((run_policy<BwdTrendQ2T, BwdLevelQ2>(c, p, "bwd_chain", "bwd_fix", ST_B, dB)));
    else CHECK((run_policy<BwdTrendT, BwdLevel>(c, p, "bwd_chain", "bwd_fix", ST_B, dB)));
    ws_launched(c, p, false);
    c->lastBwdWindow = c->bwdWindow;
    if (dB) c->last.bwdPending = true;
    c->haveBwd = true;
    return 0;
}

// Settle point: every optimistically launched stage is checked (one mailbox copy, one host sync).  If a stage re-ran
// blocks in its single validation pass, its results -- and everything computed from them -- are not yet the fixed
// point: the pipeline is re-run synchronously from that stage and the stage goes back to synchronous validation
// until a clean pass re-arms it.  After settle() the mailbox mirror holds the current per-chain sums.
// Consumes the stage counters of the mailbox mirror (which the caller has just refreshed).  Returns the first stage whose
// single optimistic validation pass re-ran blocks (-1: none did); such a stage goes back to synchronous validation and
// gets a wider window.
static int check_stages(csr_ctx *c) {
    int firstFail = -1;
    for (int stg = ST_P; stg <= ST_B; ++stg) {
        const unsigned int fresh = take_fresh(c, stg);
        unsigned int pass[MAX_DEFER_PASSES];
        for (int j = 0; j < MAX_DEFER_PASSES; ++j) pass[j] = take_fresh(c, MAIL_PASS0 + 4 * stg + j);
        const int np = c->launchedPasses[stg];
        if (fresh == 0) {
            // a long clean streak lets an extra confirmation pass go again
            if (np > 1 && ++c->cleanRuns[stg] >= 64) { c->nPasses[stg] = np - 1; c->cleanRuns[stg] = 0; }
            continue;
        }
        stage_reruns(c, stg) += fresh;
        int &wstage = (stg == ST_P && c->lastFwdWindow) ? *c->lastFwdWindow
                    : (stg == ST_B && c->lastBwdWindow) ? *c->lastBwdWindow : stage_warm(c, stg);
        if (&wstage == &c->wsWarmF || &wstage == &c->wsWarmB) {
            // a warm-started window (ECM sweeps) was too short at a wavefront's edge: widen IT (up to the cold window, where
            // warm starting switches itself off) and leave the stage's own policy alone
            const int npw = c->launchedPasses[stg];
            const bool stoodWs = npw > 1 && pass[npw - 1] == 0;
            if (c->dbgLog) fprintf(stderr, "[csr] settle: warm-started stage %d re-ran %u blocks, window %d -> %d\n", stg, fresh, wstage, wstage * 2);
            wstage = (wstage * 2 + 15) / 16 * 16;
            if (!stoodWs && firstFail < 0) firstFail = stg;
            continue;
        }
        c->cleanRuns[stg] = 0;
        grow_warm(c, wstage, pass[0]);
        const bool stands = np >= 1 && pass[np - 1] == 0;      // the last validation pass re-ran nothing: a fixed point
        if (c->dbgLog)
            fprintf(stderr, "[csr] settle: stage %d re-ran %u blocks (passes %u %u %u %u of %d) -> %s\n", stg, fresh, pass[0],
                    pass[1], pass[2], pass[3], np, stands ? "stands" : "replay");
        if (stands) continue;
        // failed: one more confirmation pass next time; at the limit the stage goes back to synchronous validation until a
        // few clean runs re-arm it, and its window widens by half (up to 4x the mode's default; beyond that the data simply
        // has long memory and repairing the few failing blocks is cheaper than a longer walk for every block)
        if (c->nPasses[stg] < MAX_DEFER_PASSES) c->nPasses[stg] += 1;
        else c->optimistic[stg] = false;
        if (c->adaptWarm) {
            int &w = wstage;
            const int cap = 4 * (c->xTolUlps > 0 ? 80 : 256);
            if (w < cap) w = std::min(cap, (w + w / 2 + 15) / 16 * 16);
        }
        if (firstFail < 0) firstFail = stg;
    }
    return firstFail;
}

static int settle(csr_ctx *c) {
    CHECK(join_side(c));
    join_pf(c);
    if (!anything_pending(c)) return 0;
    CHECK(read_mail(c, c->mailBytes));
    const bool pf = c->last.fwdPending, pb = c->last.bwdPending;
    const uint32_t pe = c->last.exports;
    drop_pending(c);
    const int firstFail = check_stages(c);
    if (firstFail < 0) return 0;
    c->rs.pipeline_redos += 1;     // pipelines re-run after a failed optimistic validation
    // the recorded passes again, in order, validated synchronously on this stream alone (copies: the passes record themselves)
    FwdPass fwd = c->last.fwd;
    fwd.defer = fwd.side = fwd.split = false;
    BwdPass bwd = c->last.bwd;
    bwd.defer = bwd.preferNatIn = false;
    if (firstFail <= ST_X && pf) {
        const bool bwdToo = pb || c->haveBwd;      // (a smoother that validated synchronously behind the failed stage ran on its results)
        if (!pb) bwd.active = fwd.active;
        CHECK(forward_impl(c, fwd));
        if (bwdToo) CHECK(backward_impl(c, bwd));
    } else if (pb) {
        CHECK(backward_impl(c, bwd));
    }
    if (pe) CHECK(export_impl(c, pe));      // arrays exported from the unvalidated results
    CHECK(read_mail(c, c->mailBytes));
    for (int stg = ST_P; stg <= ST_B; ++stg) (void)take_fresh(c, stg);
    return 0;
}

static int read_sums(csr_ctx *c, double *sum_d, double *sum_nll) {
    const size_t nc = c->chains.size();
    const bool pending = anything_pending(c);
    CHECK(settle(c));
    if (!pending) CHECK(read_mail(c, c->mailBytes));
    const double *hs = reinterpret_cast<const double *>(c->hMail + MAIL_HDR);
    if (sum_d) memcpy(sum_d, hs, sizeof(double) * nc);
    if (sum_nll) memcpy(sum_nll, hs + nc, sizeof(double) * nc);
    return 0;
}

extern "C" int csr_batch_forward(csr_ctx *c, uint32_t flags, double *sum_d, double *sum_nll) {
    CHECK(need(c));
    CHECK(settle(c));
    CHECK(forward_impl(c, {.flags = flags, .wantD = true, .defer = true, .natOut = true}));
    if (sum_d || sum_nll) CHECK(read_sums(c, sum_d, sum_nll));
    return 0;
}

// chain_mask[c] == 0: chain c's resident forward results stay untouched (its sums are not updated)
extern "C" int csr_batch_forward_masked(csr_ctx *c, uint32_t flags, const unsigned char *chain_mask, double *sum_d,
                                        double *sum_nll) {
    if (!chain_mask) return csr_batch_forward(c, flags, sum_d, sum_nll);
    CHECK(need(c));
    CHECK(settle(c));
    const int nc = (int)c->chains.size();
    std::vector<unsigned char> act(chain_mask, chain_mask + nc);
    HIPOK(hipMemcpyAsync(c->dActive, act.data(), nc, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    CHECK(forward_impl(c, {.flags = flags, .wantD = true, .active = c->dActive, .defer = true}));
    if (sum_d || sum_nll) CHECK(read_sums(c, sum_d, sum_nll));
    return 0;
}

extern "C" int csr_batch_backward(csr_ctx *c) {
    CHECK(need(c));
    CHECK(backward_impl(c, {.defer = true, .natOut = true}));
    return 0;       // validated at the next settle point
}

// forward (NIS, optional NLL) + backward as one pipeline: one host synchronisation, the NIS/NLL epilogue overlapped
// with the smoother chain.  Equivalent to csr_batch_forward followed by csr_batch_backward.
extern "C" int csr_batch_forward_backward(csr_ctx *c, uint32_t flags, double *sum_d, double *sum_nll) {
    CHECK(need(c));
    CHECK(settle(c));
    CHECK(forward_impl(c, {.flags = flags, .wantD = true, .defer = true, .side = true, .natOut = true}));
    CHECK(backward_impl(c, {.defer = true, .natOut = true}));
    if (sum_d || sum_nll) return read_sums(c, sum_d, sum_nll);
    return 0;       // validation stays pending until the next settle point (sums, download, synchronize, new inputs)
}

// ---------------------------------------------------------------------------------------------------------------
// ECM (pyx:7660-8442 / 7153-7657) over all chains in lock-step; converged chains are masked out
// ---------------------------------------------------------------------------------------------------------------
struct EcmState {
    double prev = 1.0e16, cur = 0.0;
    bool haveInit = false, done = false;
};

extern "C" int csr_batch_ecm_masked(csr_ctx *c, const csr_ecm_cfg *cfg, uint32_t flags, const unsigned char *chain_mask,
                                    csr_ecm_out *out, double *nll_path);
extern "C" int csr_batch_ecm(csr_ctx *c, const csr_ecm_cfg *cfg, uint32_t flags, csr_ecm_out *out, double *nll_path) {
    return csr_batch_ecm_masked(c, cfg, flags, nullptr, out, nll_path);
}

// chain_mask[c] == 0: chain c is left exactly as it is (results of its last fit stay resident); out[c].skipped = 2
extern "C" int csr_batch_ecm_masked(csr_ctx *c, const csr_ecm_cfg *cfg, uint32_t flags, const unsigned char *chain_mask,
                                    csr_ecm_out *out, double *nll_path) {
    CHECK(need(c));
    CHECK(settle(c));
    if (!cfg || !out) return fail("null argument");
    if (!c->statsValid) CHECK(csr_batch_stats(c));
    multipliers_changed(c);     // the E-steps rewrite the resident multipliers
    const int nc = (int)c->chains.size();
    uint32_t fl = flags & (F_QSCALE);
    if (cfg->use_lambda) fl |= F_LAMBDA;
    if (cfg->use_kappa) fl |= F_KAPPA;
    if (cfg->use_apn) fl |= F_APN;
    c->p.nu = cfg->nu;
    std::vector<EcmState> st(nc);
    std::vector<unsigned char> act(nc, 0);
    std::vector<double> nll(nc);
    for (int i = 0; i < nc; ++i) {
        csr_ecm_out &o = out[i];
        memset(&o, 0, sizeof(o));
    }
    auto push_active = [&]() -> int {
        HIPOK(hipMemcpyAsync(c->dActive, act.data(), nc, hipMemcpyHostToDevice, c->stream));
        HIPOK(hipStreamSynchronize(c->stream));
        return 0;
    };
    // tiny chains: filter + smoother + NLL only (pyx:7998-8129)
    bool anyTiny = false, anyBig = false;
    auto masked = [&](int i) { return chain_mask != nullptr && chain_mask[i] == 0; };
    bool anyMasked = false;
    for (int i = 0; i < nc; ++i) {
        if (masked(i)) { out[i].skipped = 2; anyMasked = true; continue; }
        if (c->chains[i].n <= 5) { act[i] = 1; anyTiny = true; out[i].skipped = 1; }
        else anyBig = true;
    }
    if (anyMasked && (anyTiny || anyBig)) CHECK(need_blocked(c, {CSR_ARR_XS, CSR_ARR_PS, CSR_ARR_LAG}, nullptr));
    if (anyTiny) {
        CHECK(push_active());
        CHECK(forward_impl(c, {.flags = fl | F_NLL, .wantD = true, .active = c->dActive, .defer = true}));
        CHECK(backward_impl(c, {.active = c->dActive, .defer = true}));
        CHECK(read_sums(c, nullptr, nll.data()));
        for (int i = 0; i < nc; ++i)
            if (act[i]) { out[i].final_nll = out[i].initial_nll = nll[i]; st[i].done = true; }
    }
    if (anyBig) {
        for (int i = 0; i < nc; ++i) act[i] = (c->chains[i].n > 5 && !masked(i)) ? 1 : 0;
        CHECK(push_active());
        bool fwdFresh = false;   // forward results already match the current multipliers
        struct SweepStateReset {     // also on the error paths
            csr_ctx *c;
            ~SweepStateReset() { c->wsActive = c->wsCold = false; }
        } sweepStateReset{c};
        c->wsSavedF = c->wsSavedB = 0;      // the first sweep of a call starts cold (the data / background may have changed)
        // kappa only (the reference CLI's default, constants.py:270-271): the smoother chain holds the moments of bins k
        // and k+1 and the lag covariance when it finishes bin k, so it evaluates the E-step itself; only the last inner
        // sweep's moments can become the result of this iteration, the others are not even stored.
        const bool fusedE = cfg->use_kappa && !cfg->use_lambda && !cfg->use_apn && c->mdl.state_dim == 2;
        if (fusedE) {
            // The fused E-step must not overwrite the kappa its own sweep's forward pass ran with: were that pass's
            // deferred validation to fail, its re-run would read the NEXT sweep's kappa (one E-step ahead of pyx:8222-8300).
            // Sweeps therefore ping-pong two scratch buffers; the resident kappa changes only when an iteration is validated.
            for (float *&q : c->kapScratch)
                if (!q) CHECK(dalloc(c, &q, c->TN + (int64_t)c->B * 64));      // + the look-ahead padding group
        }
        // One ECM iteration (pyx:8156-8300) as launches only: t_inner x [forward, smoother + kappa E-step] + NLL forward.
        // Returns the buffer holding the iteration's final kappa (nullptr: no sweep ran, the resident one is unchanged).
        float *iterKappa = nullptr;
        auto launch_iteration = [&](bool defer, bool skipFirstForward) -> int {
            c->wsActive = true;
            float *cur = nullptr;                   // nullptr = the resident kappa (the one this iteration starts from)
            for (int64_t inner = 0; inner < cfg->inner_iters; ++inner) {
                if (!(inner == 0 && skipFirstForward))
                    CHECK(forward_impl(c, {.flags = fl, .active = c->dActive, .defer = defer, .sweep = true, .kappaIn = cur}));
                float *const next = c->kapScratch[inner & 1];
                CHECK(backward_impl(c, {.active = c->dActive, .defer = defer, .estep = inner + 1 == cfg->inner_iters ? 1 : 2,
                                        .kappaIn = cur, .kappaOut = next}));
                cur = next;
            }
            // pyx:8300 (stores everything: it is the forward pass that stays resident)
            CHECK(forward_impl(c, {.flags = fl | F_NLL, .wantD = true, .active = c->dActive, .defer = defer, .kappaIn = cur}));
            c->wsActive = false;
            iterKappa = cur;
            return 0;
        };
        const double *mailSums = reinterpret_cast<const double *>(c->hMail + MAIL_HDR);
        for (int64_t it = 0; it < cfg->max_iters; ++it) {
            if (fusedE) {
                // ONE settle point per iteration: every stage of every sweep is validated optimistically; if any of them
                // re-ran blocks, the whole iteration is replayed with synchronous validation from the kappa it started with
                // (still resident: it is replaced only below, once the iteration stands).
                CHECK(launch_iteration(c->deferEnabled, fwdFresh));
                CHECK(read_mail(c, c->mailBytes));
                const bool hadPending = anything_pending(c);
                drop_pending(c);        // (the iteration is replayed here, as a whole, not pass by pass at a settle point)
                if (hadPending && check_stages(c) >= 0) {
                    c->rs.pipeline_redos += 1;
                    c->wsCold = true;               // the replay starts every window cold (and records fresh checkpoints)
                    const int rcReplay = launch_iteration(false, false);
                    c->wsCold = false;
                    CHECK(rcReplay);
                    CHECK(read_mail(c, c->mailBytes));
                    drop_pending(c);
                    for (int stg = ST_P; stg <= ST_B; ++stg) (void)take_fresh(c, stg);
                }
                if (iterKappa) {      // the iteration's kappa becomes the resident one (for the chains of this iteration)
                    bool everyChain = true;
                    for (int i = 0; i < nc; ++i) everyChain = everyChain && act[i] != 0;
                    if (everyChain) {
                        // every chain of the batch took part: the buffer the last sweep wrote BECOMES the resident one and the
                        // old resident buffer takes its place among the scratch buffers (no copy: 58 MB less per iteration at
                        // genome scale, one launch less on a shard)
                        float *old = c->p.tKap;
                        for (float *&q : c->kapScratch)
                            if (q == iterKappa) q = old;
                        c->p.tKap = iterKappa;
                        c->p.tKapOut = iterKappa;
                    } else {
                        Prm p = c->p;
                        p.chainActive = c->dActive;
                        CHECK(launch(c, "ecm_commit_kappa", "k_copy_active_f32", k_copy_active_f32, dim3(grid_slots(c)), dim3(256), 0, c->stream, p,
                                     iterKappa, c->p.tKap));
                    }
                }
                for (int i = 0; i < nc; ++i) nll[i] = mailSums[nc + i];
            } else {
                for (int64_t inner = 0; inner < cfg->inner_iters; ++inner) {
                    if (!fwdFresh) CHECK(forward_impl(c, {.flags = fl, .active = c->dActive, .defer = true, .sweep = true}));
                    fwdFresh = false;
                    CHECK(backward_impl(c, {.active = c->dActive, .defer = true}));
                    CHECK(settle(c));          // the E-step kernels consume validated results and update in place
                    Prm p = c->p;
                    p.flags = fl;
                    p.chainActive = c->dActive;
                    if (cfg->use_lambda)
                        CHECK(launch(c, "estep_lambda", "k_estep_lambda", k_estep_lambda, dim3(grid_slots(c)), dim3(256), 0, c->stream, p));
                    if (cfg->use_kappa)
                        CHECK(launch(c, "estep_kappa", "k_estep_kappa", k_estep_kappa, dim3(grid_slots(c)), dim3(256), 0, c->stream, p));
                }
                CHECK(forward_impl(c, {.flags = fl | F_NLL, .wantD = true, .active = c->dActive, .defer = true}));    // pyx:8300
                CHECK(read_sums(c, nullptr, nll.data()));
            }
            // the multipliers do not change until the next E-step: the next sweep may reuse this forward pass,
            // unless adaptive process noise made it depend on returnNLL-independent state only (it does not)
            fwdFresh = (cfg->inner_iters > 0);
            bool anyLeft = false, changed = false;
            for (int i = 0; i < nc; ++i) {
                if (!act[i]) continue;
                EcmState &s = st[i];
                csr_ecm_out &o = out[i];
                o.iters_done = it + 1;
                s.cur = nll[i];
                if (nll_path) nll_path[(int64_t)i * cfg->max_iters + it] = s.cur;
                const bool havePrev = s.haveInit;       // pyx:8337-8407
                if (!havePrev) { o.initial_nll = s.cur; s.haveInit = true; }
                else if (s.cur > s.prev + (1.0e-12 * std::fmax(std::fabs(s.prev), 1.0))) o.nll_increase_count += 1;
                double delta, scale;
                if (havePrev) { delta = std::fabs(s.cur - s.prev); scale = std::fabs(s.prev); }
                else { delta = 0.0; scale = std::fabs(s.cur); }
                if (std::fabs(s.cur) > scale) scale = std::fabs(s.cur);
                if (scale < 1.0) scale = 1.0;
                if (havePrev) { o.rel_improvement = (s.prev - s.cur) / scale; o.abs_rel_change = delta / scale; }
                else { o.rel_improvement = 0.0; o.abs_rel_change = 0.0; }
                const double tol = cfg->rtol * scale;
                s.prev = s.cur;
                if (havePrev && delta <= tol) o.stable_iters += 1; else o.stable_iters = 0;
                if (o.stable_iters >= 2) { o.converged = 1; s.done = true; act[i] = 0; changed = true; }
                else anyLeft = true;
            }
            if (!anyLeft) break;
            if (changed) CHECK(push_active());
        }
        for (int i = 0; i < nc; ++i) {
            if (c->chains[i].n <= 5 || masked(i)) continue;
            out[i].has_initial_nll = st[i].haveInit ? 1 : 0;
            out[i].final_nll = st[i].prev;
        }
    }
    c->last.fwd.flags = fl;     // the multipliers the resident fit stands for (nothing is pending here)
    c->haveFwd = c->haveBwd = true;
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// export / download
// ---------------------------------------------------------------------------------------------------------------

// Exports may be queued behind an optimistically validated pipeline: they are re-issued by settle() if it fails.
extern "C" int csr_batch_export(csr_ctx *c, uint32_t what) {
    CHECK(need(c));
    if (anything_pending(c)) reexport_on_replay(c, what);
    return export_impl(c, what);
}

extern "C" int csr_batch_sums(csr_ctx *c, double *sum_d, double *sum_nll) {
    CHECK(need(c));
    if (!c->haveFwd) return fail("no forward results");
    return read_sums(c, sum_d, sum_nll);
}

static int flush_export(csr_ctx *c, ExpList &L) {
    if (L.count == 0) return 0;
    CHECK(launch(c, "export_natural", "k_export_tiled", k_export_tiled, tile_grid(c), dim3(256), 0, c->stream, c->p, L));
    L.count = 0;
    return 0;
}
// The reference-layout copy of array `id` is needed: queue its conversion unless that copy is current already.  keep = false
// does not remember the conversion (every export of a forward pass converts D / xf / Pf / pNoise again unless the pass wrote them)
static int need_natural(csr_ctx *c, ExpList &L, int id, const float *src, int E, int n, int skipLast, bool keep = true) {
    if (c->where[id].nat) return 0;
    if (L.count == 8) CHECK(flush_export(c, L));       // one launch converts up to eight arrays
    float *dst;
    CHECK(nat_array(c, id, &dst));
    exp_add(L, src, dst, E, n, skipLast);
    c->where[id].nat = keep;
    return 0;
}
static int need_natural_xs(csr_ctx *c, ExpList &L) {
    return need_natural(c, L, CSR_ARR_XS, (const float *)c->p.tXs, 2, c->mdl.state_dim, 0);
}
static int need_natural_mult(csr_ctx *c, ExpList &L, int id) {
    return need_natural(c, L, id, id == CSR_ARR_LAMBDA ? c->p.tLam : (id == CSR_ARR_KAPPA ? c->p.tKap : c->p.tQs), 1, 1, 0);
}

// The form of the residual kernels for this batch (csr_resid_form.h): K 64-bin sub-tiles per workgroup, the sample rows staged in
// LDS all at once or, past 64 KB, in slabs
static ResidForm resid_form(const csr_ctx *c) { return resid_form(c->m); }
// residuals of the bins [off, off + nb) of the batch's natural layout (whole chains: off and nb are multiples of 64)
static int launch_resid(csr_ctx *c, int64_t off, int64_t nb, bool foldCheck) {
    const int d = c->mdl.state_dim;
    float *xs, *res;
    CHECK(nat_array(c, CSR_ARR_XS, &xs));
    CHECK(nat_array(c, CSR_ARR_RESID, &res));
    Prm pr = c->p;
    pr.xTolUlps = c->xTolUlps;
    pr.prevKind = CK_NONE;
    // grid x 256 threads >= blocks: Npad / (K * 64) workgroups, K <= 4, block length >= 32
    if (foldCheck && off == 0 && (int64_t)((nb + 255) / 256) * 256 >= c->NB) take_pending_check(c, pr);
    pr.data += off;
    if (pr.bg) pr.bg += off;
    xs += off * d;
    res += off * c->m;
    const ResidForm f = resid_form(c);
    void (*const kernel)(Prm, const float *, int, float *, int64_t) = f.v4 ? (f.K == 2 ? &k_resid_v4<2> : &k_resid_v4<1>) : &k_resid;
    const dim3 grid((unsigned)((nb + f.K * 64 - 1) / (f.K * 64)));
    return launch(c, "residuals", "k_resid", kernel, grid, dim3(256), f.lds, c->stream, pr, xs, d, res, nb);
}
// residuals of `n` runs of whole chains (host copy `runs`, wg0 filled in here; device copy `dRuns`, uploaded on c->stream from the
// pinned `runs`) in ONE launch: each workgroup does what it does in a launch over its run alone
static int launch_resid_runs(csr_ctx *c, ResidRun *runs, ResidRun *dRuns, int n) {
    if (n == 0) return 0;
    const int d = c->mdl.state_dim;
    float *xs, *res;
    CHECK(nat_array(c, CSR_ARR_XS, &xs));
    CHECK(nat_array(c, CSR_ARR_RESID, &res));
    Prm pr = c->p;
    pr.xTolUlps = c->xTolUlps;
    pr.prevKind = CK_NONE;
    const ResidForm f = resid_form(c);
    int64_t wgs = 0;
    for (int i = 0; i < n; ++i) { runs[i].wg0 = wgs; wgs += (runs[i].len + f.K * 64 - 1) / (f.K * 64); }
    HIPOK(hipMemcpyAsync(dRuns, runs, sizeof(ResidRun) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    void (*const kernel)(Prm, const float *, int, float *, const ResidRun *, int) =
        f.v4 ? (f.K == 2 ? &k_resid_v4_runs<2> : &k_resid_v4_runs<1>) : &k_resid_runs;
    return launch(c, "residuals", "k_resid_runs", kernel, dim3((unsigned)wgs), dim3(256), f.lds, c->stream, pr, (const float *)xs, d, res,
                  (const ResidRun *)dRuns, n);
}

static int export_impl(csr_ctx *c, uint32_t what) {
    const int d = c->mdl.state_dim;
    const Prm &p = c->p;
    const int nv = d, nm = d * d;      // exported components of state vectors / covariance matrices
    ExpList L;
    memset(&L, 0, sizeof(L));
    // The NIS/NLL track is the only export that depends on the side stream's epilogue: when that is still running it is
    // converted last, after the (long, bandwidth-bound) residual kernel, so the epilogue leaves the critical path.
    // (Small batches are launch-bound: there the extra conversion launch costs more than the overlap saves.)
    const bool natD = c->where[CSR_ARR_D].nat;
    const bool lateD = (what & CSR_EXPORT_FORWARD) && c->sidePending && (what & CSR_EXPORT_RESID) && !natD &&
                       c->Npad >= ((int64_t)4 << 20);
    // D is current in the reference layout (the epilogue wrote it there itself): nothing in this export depends on the side
    // stream; it is joined at the next settle point (sums, download, device_array, synchronize)
    if (!lateD && !natD) CHECK(join_side(c));
    if (what & CSR_EXPORT_FORWARD) {
        if (!c->haveFwd) return fail("no forward results to export");
        join_pf(c);
        if (!lateD) CHECK(need_natural(c, L, CSR_ARR_D, p.tD, 1, 1, 0, false));
        CHECK(need_natural(c, L, CSR_ARR_XF, (const float *)p.tXf, 2, nv, 0, false));
        CHECK(need_natural(c, L, CSR_ARR_PF, (const float *)p.tPf, 4, nm, 0, false));
        const bool constQ = const_q(c);
        if (c->where[CSR_ARR_PNOISE].nat) {
            // (the constant process noise was filled underneath the state chain as well)
        } else if (constQ && p.chainQ == nullptr) {
            // one Q0 for every bin of every chain: a streaming fill (rows past a chain's n-1 are padding nobody reads)
            if (!pn_fill_current(c, p)) {
                float *dst;
                CHECK(nat_array(c, CSR_ARR_PNOISE, &dst));
                CHECK(launch_pn_fill(c, p, dst, c->stream));
            }
        } else {
            CHECK(need_natural(c, L, CSR_ARR_PNOISE, constQ ? nullptr : (const float *)p.tQ, 4, nm, 1, false));
            c->pnFillValid = false;
            // (constant flags with per-chain base matrices: the descriptor just queued carries the model's row, as early_cov_exports' does)
            if (constQ) pn_fill_values(c, p, L.d[L.count - 1].cval);
        }
    }
    if (what & (CSR_EXPORT_SMOOTH | CSR_EXPORT_RESID)) {
        if (!c->haveBwd) return fail("no smoothed results to export");
        CHECK(need_natural_xs(c, L));
    }
    if (what & CSR_EXPORT_SMOOTH) {
        CHECK(need_natural(c, L, CSR_ARR_PS, (const float *)p.tPs, 4, nm, 0));
        CHECK(need_natural(c, L, CSR_ARR_LAG, (const float *)p.tLag, 4, nm, 1));
    }
    if (what & CSR_EXPORT_MULT)
        for (int id : {CSR_ARR_LAMBDA, CSR_ARR_KAPPA, CSR_ARR_QSCALE}) CHECK(need_natural_mult(c, L, id));
    CHECK(flush_export(c, L));
    if (what & CSR_EXPORT_RESID) CHECK(launch_resid(c, 0, c->Npad, true));
    if (lateD) {
        CHECK(join_side(c));
        CHECK(need_natural(c, L, CSR_ARR_D, p.tD, 1, 1, 0, false));
        CHECK(flush_export(c, L));
    }
    return 0;
}

// One pass of the hot path in one call: statistics + forward (NIS / NLL) + backward + export of `what` + per-chain sums.
// Same launches as csr_batch_stats / csr_batch_forward_backward / csr_batch_export / csr_batch_sums in sequence -- a
// convenience for callers; the four separate calls cost the same (0.411 vs 0.412 ms on a 1/8-genome shard: the host runs
// ahead of the device, only the final read-back is a round trip).
// one constant process noise: the smoother of a tail group reads xf / Pf of its chains in the reference layout (k_smooth_natin)
static bool tail_reads_nat(csr_ctx *c, const Prm &pf) {
    return c->natInEnabled && c->where[CSR_ARR_PF].nat && const_q(c) && pf.chainQ == nullptr && (c->B % 8) == 0 &&
           (stage_warm(c, ST_B) % 8) == 0 && unit_f(pf);
}
// The tail of the chains of `dmask` (device bytes; `runs`: their maximal runs), on c->stream: the smoother (behind a blocked copy of
// xf only where it reads blocks) and ONE residual launch over the runs (table `hRuns` / `dRuns`, launch_resid_runs).  The NIS / NLL
// epilogue runs in groups of its own (step_pipelined).
static int step_tail(csr_ctx *c, const Prm &pf, const unsigned char *dmask, const std::vector<ChainRun> &runs, uint32_t what,
                     ResidRun *hRuns, ResidRun *dRuns) {
    Prm pt = pf;
    pt.chainActive = dmask;
    pt.prevKind = CK_NONE;
    const bool natTail = tail_reads_nat(c, pf);
    if (!natTail && !runs.empty()) {
        const auto [g0, groups] = group_span(runs);
        CHECK(import_xf_blocked(c, pt, c->stream, g0, groups));
    }
    CHECK(backward_impl(c, {.active = dmask, .defer = true, .natOut = true, .preferNatIn = natTail}));
    CHECK(flush_pending_check(c));
    if (what & CSR_EXPORT_RESID) {
        int n = 0;
        for (const ChainRun &r : runs) hRuns[n++] = ResidRun{r.off, r.len, 0};
        CHECK(launch_resid_runs(c, hRuns, dRuns, n));
    }
    return 0;
}

// c->stream is `st` while one of these lives: what a tail group launches goes to the tail stream through the same functions that
// otherwise launch on the main stream (nat_array counts first uses in between, csr_run_stats.nat_first_use_off_main)
struct StreamScope {
    csr_ctx *c; hipStream_t old;
    StreamScope(csr_ctx *c_, hipStream_t st) : c(c_), old(c_->stream) { c->stream = st; }
    ~StreamScope() { c->stream = old; }
};

// Does this step pipeline its tail per chain?  Bit-exact levelTrend mode, barrier-free state chain, deferred validation, 2 to 4096 chains.
// (round 4: per-bin multipliers and per-chain base matrices pipeline as well -- their process noise goes to the reference
// layout underneath the state chain with Pf, early_cov_exports; the sequential APN pass has no state chain to hide behind)
static bool step_pipelines(const csr_ctx *c, uint32_t flags, uint32_t what) {
    return c->tailSplit && c->xTolUlps == 0 && c->mdl.state_dim == 2 && !c->seqState && c->sbAsync && c->deferEnabled &&
           !((flags & F_APN) && !(flags & F_QSCALE)) && !(what & CSR_EXPORT_MULT) && c->chains.size() >= 2 && c->chains.size() <= 4096;
}
// the forward pass is complete: the rest of the step in order
static int step_rest_in_order(csr_ctx *c, uint32_t what, bool *handled) {
    CHECK(backward_impl(c, {.defer = true, .natOut = true}));
    if (what) CHECK(csr_batch_export(c, what));
    *handled = true;
    return 0;
}

// A step of the bit-exact mode whose tail is PIPELINED PER CHAIN behind the barrier-free state chain.  That launch lasts as
// long as the slowest chain needs (3.7 ms at genome scale) while most chains are final a millisecond earlier, and it leaves the
// memory system idle.  The kernel sets a host-visible word per chain when the chain is final; the host watches those words and,
// whenever the newly finished chains make up tailFirstPct / tailNextPct per cent of the batch, launches their tail (smoother,
// residuals; every kernel under a chain mask) on a second stream; the remainder follows when the state chain has ended.  The
// NIS / NLL epilogue goes out in groups of its own on the side stream (epiPct per cent of the batch each; k_fwd_dstat<natXf> reads
// the previous filtered state where the state chain wrote it): it needs a chain's final xf and nothing of the smoother, and
// memory is idle under the state chain.  Same arithmetic, same results; a chain's tail simply starts when ITS filtered state stands.
static int step_pipelined(csr_ctx *c, uint32_t flags, uint32_t what, bool *handled) {
    *handled = false;
    if (!step_pipelines(c, flags, what)) return 0;
    CHECK(settle(c));
    CHECK(forward_impl(c, {.flags = flags, .wantD = true, .defer = true, .natOut = true, .split = true}));
    // the state chain did not go out as one launch: the pass is complete, carry on as usual
    if (!c->sbp.active) return step_rest_in_order(c, what, handled);
    const Prm pf = c->sbp.p;
    if (!(c->where[CSR_ARR_D].nat && c->where[CSR_ARR_PF].nat && c->where[CSR_ARR_PNOISE].nat)) {
        // an output of this pass still needs a conversion launch of its own (export_impl): no pipelining, finish in order
        CHECK(sb_finish(c, false));
        CHECK(import_xf_blocked(c, pf, c->stream, 0, c->NG, false));
        CHECK(forward_epilogue(c, pf, true));
        return step_rest_in_order(c, what, handled);
    }
    const int nc = (int)c->chains.size();
    CHECK(c->tailMasks.ensure(c, nc));
    const bool natTail = tail_reads_nat(c, pf);
    float *natXf = nullptr;
    CHECK(nat_array(c, CSR_ARR_XF, &natXf));
    CHECK(c->epiMasks.ensure(c, nc));
    CHECK(c->tailRuns.ensure(c, nc));
    // (groups are disjoint sets of chains, hence of blocks: their kernels share no data; every group leaves no folded check behind.
    // Each group uploads from the pinned slot it owns: no slot is written twice in a step)
    ChainSet tails(c->chains, MAX_EARLY_TAILS), epis(c->chains, MAX_EARLY_EPILOGUES);
    std::vector<unsigned char> grp((size_t)nc, 0), egrp((size_t)nc, 0);
    // a group's epilogue (the chains of `egrp`, side stream) and a group's tail (the chains of `grp`, c->stream)
    auto launch_epilogue = [&]() -> int {
        const int slot = epis.handed() - 1;
        CHECK(c->epiMasks.upload(slot, egrp.data(), c->side));
        Prm pe = pf;
        pe.chainActive = c->epiMasks.dev(slot);
        pe.prevKind = CK_NONE;
        return launch_dstat(c, pe, c->side, natXf);
    };
    auto launch_tail = [&]() -> int {
        const int slot = tails.handed() - 1;
        CHECK(c->tailMasks.upload(slot, grp.data(), c->stream));
        return step_tail(c, pf, c->tailMasks.dev(slot), chain_runs(c->chains, grp), what, c->tailRuns.host(slot), c->tailRuns.dev(slot));
    };
    // ---- while the state chain runs: the chains that are final, a group at a time (tails: tail stream; epilogues: side stream)
    // (the end of the launch is on the step's critical path -- the last tail starts behind it: the loop's sleeps run with a lowered
    // timer slack and, around the moment the PREVIOUS launch of this context ended, it polls without sleeping)
    TimerSlack slack;
    std::vector<unsigned> done((size_t)nc, 0u);
    const int32_t *const tailScript = c->tailScript.empty() ? nullptr : c->tailScript.data();
    const int32_t *const epiScript = c->epiScript.empty() ? nullptr : c->epiScript.data();
    const auto tLoop = std::chrono::steady_clock::now();
    const double expectEnd = c->lastSbLoopUs;
    for (;;) {
        const hipError_t qs = hipStreamQuery(c->stream);
        const double el = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - tLoop).count();
        if (qs == hipSuccess) { c->lastSbLoopUs = el; break; }
        if (qs != hipErrorNotReady) return fail("state chain: %s", hipGetErrorString(qs));
        // (bounded sleep-poll: the launch lasts milliseconds and a tail group is worth launching 20-50 us late; round 3 spun here)
        const bool nearEnd = expectEnd > 0.0 && el > expectEnd - 100.0 && el < expectEnd + 200.0;
        if (!nearEnd) std::this_thread::sleep_for(std::chrono::microseconds(20));
        for (int i = 0; i < nc; ++i) done[(size_t)i] = __atomic_load_n(&c->hDone[i], __ATOMIC_ACQUIRE);
        // (an epilogue group is an upload and a launch: never inside the interval in which the end of the state chain is expected)
        // (a scripted grouping, csr_batch_set_step_groups: the next group goes out when all its chains are final, whatever the clock says)
        if (epiScript ? epis.pick_scripted(done.data(), epiScript, egrp) : c->epiPct > 0 && !nearEnd && epis.pick(done.data(), c->epiPct, egrp))
            CHECK(launch_epilogue());
        if (tailScript ? tails.pick_scripted(done.data(), tailScript, grp)
                       : tails.pick(done.data(), tails.handed() == 0 ? c->tailFirstPct : c->tailNextPct, grp)) {
            StreamScope onTail(c, c->tail);
            CHECK(launch_tail());
        }
    }
    // ---- the launch has ended: its verdict (a bail-out runs the pass form and invalidates nothing that was final, but the
    // pass form rewrites the whole track from the cold prior: sb_finish waits for the groups already launched and everything is redone)
    const int64_t bail0 = c->rs.sb_bailouts;
    CHECK(sb_finish(c, false));
    const bool bailed = c->rs.sb_bailouts != bail0;
    if (bailed && tails.handed() + epis.handed() > 0) { tails.clear(); epis.clear(); }
    // ---- a scripted grouping is the same whatever the timing: every chain is final now, and the scripted groups the watch loop
    // did not reach go out one by one as it would have launched them (sb_finish waited for the main stream: nothing of the state
    // chain is in flight).  After a bail-out everything is one remainder, scripted or not.
    if (!bailed && (tailScript || epiScript)) {
        std::fill(done.begin(), done.end(), 1u);
        while (tailScript && tails.pick_scripted(done.data(), tailScript, grp)) {
            StreamScope onTail(c, c->tail);
            CHECK(launch_tail());
        }
        while (epiScript && epis.pick_scripted(done.data(), epiScript, egrp)) CHECK(launch_epilogue());
    }
    // ---- the remaining chains: on the main stream, behind the state chain and beside whatever the tail stream still has to do
    if (tails.rest(grp)) CHECK(launch_tail());
    // ---- the epilogue of the chains that have none yet, on the side stream (the state chain has ended: nothing to wait for)
    if (epis.rest(egrp)) CHECK(launch_epilogue());
    HIPOK(hipEventRecord(c->evEpiJoin, c->side));
    HIPOK(hipEventRecord(c->evTailJoin, c->tail));
    HIPOK(hipStreamWaitEvent(c->stream, c->evTailJoin, 0));
    HIPOK(hipStreamWaitEvent(c->stream, c->evEpiJoin, 0));
    // (no blocked copy of xf was made where the smoother read the reference layout: later readers of blocks bring it back)
    if (natTail) produced(c, {CSR_ARR_XF}, W_NAT);
    Prm ps = pf;
    ps.chainActive = nullptr;
    CHECK(launch_chain_sums(c, ps, c->stream));
    replay_covers_every_chain(c);
    if (c->last.bwdPending) reexport_on_replay(c, what);
    c->rs.tail_groups += tails.handed();
    *handled = true;
    return 0;
}

extern "C" int csr_batch_step(csr_ctx *c, uint32_t flags, uint32_t what, double *sum_d, double *sum_nll) {
    CHECK(csr_batch_stats(c));
    bool handled = false;
    CHECK(step_pipelined(c, flags, what, &handled));
    if (!handled) {
        CHECK(csr_batch_forward_backward(c, flags, nullptr, nullptr));
        if (what) CHECK(csr_batch_export(c, what));
    }
    if (sum_d || sum_nll) return csr_batch_sums(c, sum_d, sum_nll);
    return 0;
}

extern "C" int csr_batch_step_forward(csr_ctx *c, uint32_t flags, uint32_t what, double *sum_d, double *sum_nll) {
    CHECK(csr_batch_stats(c));
    CHECK(settle(c));
    CHECK(forward_impl(c, {.flags = flags, .wantD = true, .defer = true, .natOut = true}));
    if (what & CSR_EXPORT_FORWARD) CHECK(csr_batch_export(c, CSR_EXPORT_FORWARD));
    if (sum_d || sum_nll) return csr_batch_sums(c, sum_d, sum_nll);
    return 0;
}

extern "C" int csr_batch_device_array(csr_ctx *c, int32_t id, void **dev_ptr, int64_t *n_elems) {
    CHECK(need(c));
    CHECK(settle(c));
    if (id < 0 || id >= CSR_ARR_COUNT) return fail("bad array id");
    float *ptr;
    CHECK(nat_array(c, id, &ptr));
    if (dev_ptr) *dev_ptr = ptr;
    if (n_elems) *n_elems = arr_comps(c, id) * c->Npad;
    return 0;
}

extern "C" int csr_batch_download(csr_ctx *c, int32_t chain, int32_t id, void *host_dst) {
    CHECK(need(c));
    CHECK(settle(c));
    if (chain < 0 || chain >= (int)c->chains.size()) return fail("chain index out of range");
    if (id < 0 || id >= CSR_ARR_COUNT) return fail("bad array id");
    if (!host_dst) return fail("null host buffer");
    if (id == CSR_ARR_BACKGROUND && !c->nat[id]) {       // no background set yet: it is identically zero
        float *q;
        CHECK(nat_array(c, id, &q));
    }
    if (!c->nat[id]) return fail("array %d was not exported", id);
    const ChainInfo &ci = c->chains[chain];
    const int64_t per = arr_comps(c, id);
    int64_t rows = ci.n;
    if (id == CSR_ARR_PNOISE || id == CSR_ARR_LAG) rows = ci.n - 1;
    if (rows > 0)
        HIPOK(hipMemcpyAsync(host_dst, c->nat[id] + ci.off * per, sizeof(float) * per * rows, hipMemcpyDeviceToHost,
                             c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// synthetic fill (bench / scale tests)
// ---------------------------------------------------------------------------------------------------------------
extern "C" int csr_batch_synthesize(csr_ctx *c, uint64_t seed) {
    CHECK(need(c));
    CHECK(settle(c));
    if (!c->dLatent) CHECK(dalloc(c, &c->dLatent, c->Npad));
    std::vector<float> lat((size_t)c->Npad, 0.f);
    uint64_t s = seed * 0x9E3779B97F4A7C15ull + 12345;
    auto next = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
    for (size_t ch = 0; ch < c->chains.size(); ++ch) {
        const ChainInfo &ci = c->chains[ch];
        double x = 0.0;
        for (int64_t k = 0; k < ci.n; ++k) {
            // Irwin-Hall(12) normal approximation is plenty for a synthetic random walk
            double acc = 0.0;
            const uint64_t a = next(), b = next();
            for (int q = 0; q < 6; ++q) acc += (double)((a >> (q * 10)) & 1023) / 1024.0;
            for (int q = 0; q < 6; ++q) acc += (double)((b >> (q * 10)) & 1023) / 1024.0;
            x += 0.03 * (acc - 6.0);
            lat[(size_t)(ci.off + k)] = (float)x;
        }
    }
    HIPOK(hipMemcpy(c->dLatent, lat.data(), sizeof(float) * c->Npad, hipMemcpyHostToDevice));
    CHECK(launch(c, "synthesize", "k_synth", k_synth, dim3((int)((c->Npad + 255) / 256)), dim3(256), 0, c->stream, c->p, c->dLatent,
                 const_cast<float *>(c->p.data), const_cast<float *>(c->p.munc), seed, c->Npad));
    HIPOK(hipStreamSynchronize(c->stream));
    c->statsValid = c->haveFwd = c->haveBwd = false;
    return 0;
}

