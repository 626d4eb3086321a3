// csr_lib.hip -- host side of libconsenrich_amd.so: context, device memory, launch orchestration and the C ABI
// declared in include/consenrich_amd.h.  gfx950 only.  No CPU compute path exists here: without a GPU every entry
// point fails loudly.
#include "../../include/consenrich_amd.h"
#include "csr_device.h"
#include "csr_background.h"
#include "csr_writers.h"
#include "csr_folds.h"
#include "csr_qseed.h"
#include "csr_qseed_post.h"
#include "csr_objective.h"
#include "csr_gain.h"
#include "csr_rocco.h"
#include "csr_dwb.h"
#include "csr_null.h"
#include "csr_segments.h"
#include "csr_ess.h"
#include "csr_peakscore.h"
#include "csr_nested.h"
#include "csr_export.h"
#include "csr_cleanup.h"
#include "csr_broad.h"
#include "csr_depspan.h"
#include "csr_shrink.h"
#include "csr_munc.h"
#include "csr_munc_track.h"
#include "csr_step_groups.h"
#include "csr_chain_tracks.h"

#include <algorithm>
#include <array>
#include <cctype>
#include <cfloat>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <chrono>
#include <sys/prctl.h>
#include <thread>
#include <type_traits>
#include <utility>
#include <vector>

using namespace csr;

// ---------------------------------------------------------------------------------------------------------------
// error plumbing
// ---------------------------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";
static int fail(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return -1;
}
// an argument or input the reference answers with ValueError: its text, and CSR_ERR_VALUE instead of -1
static int value_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return CSR_ERR_VALUE;
}
#define HIPOK(expr)                                                                                       \
    do {                                                                                                  \
        hipError_t e_ = (expr);                                                                           \
        if (e_ != hipSuccess) return fail("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)
#define CHECK(expr)                \
    do {                           \
        int rc_ = (expr);          \
        if (rc_ != 0) return rc_;  \
    } while (0)

extern "C" const char *csr_last_error(void) { return g_err; }
extern "C" int csr_abi_version(void) { return CSR_ABI_VERSION; }
#ifndef CSR_SOURCE_HASH
#define CSR_SOURCE_HASH "unknown"
#endif
#ifndef CSR_BUILD_FLAGS
#define CSR_BUILD_FLAGS ""
#endif
#define CSR_STR2(x) #x
#define CSR_STR(x) CSR_STR2(x)
// (the marker in front lets consenrich_amd/build.py find the record in the file without loading the library)
static const char g_buildId[] = "CSR_BUILD_ID:abi " CSR_STR(CSR_ABI_VERSION) " src " CSR_SOURCE_HASH " " CSR_BUILD_FLAGS;
extern "C" const char *csr_build_id(void) { return g_buildId + 13; }
extern "C" int csr_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// ---------------------------------------------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------------------------------------------
constexpr size_t MAIL_HDR = 80;     // 20 x u32 counters
constexpr int MAIL_PASS0 = 4, MAIL_DUMMY = 16, MAIL_LOCAL = 17, MAX_DEFER_PASSES = 4;    // MAIL_LOCAL: blocks repaired inside speculative kernels

struct ProfEntry {
    int64_t launches = 0;
    double total_ms = 0.0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
};

// Growable device work space.  Owns its memory: whoever holds one as a member frees it by being destroyed or assigned to (the device
// must be selected at that moment, see csr_destroy)
struct DevBuf {
    void *ptr = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : ptr(o.ptr), cap(o.cap) { o.ptr = nullptr; o.cap = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) { release(); ptr = o.ptr; cap = o.cap; o.ptr = nullptr; o.cap = 0; }
        return *this;
    }
    ~DevBuf() { release(); }
    void release() {
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr;
        cap = 0;
    }
    int reserve(size_t bytes) {
        if (bytes <= cap) return 0;
        release();
        const size_t want = bytes + bytes / 8 + 256;
        hipError_t e = hipMalloc(&ptr, want);
        if (e != hipSuccess) return fail("hipMalloc(%zu bytes) failed: %s", want, hipGetErrorString(e));
        cap = want;
        return 0;
    }
};
// Pinned host memory of `count` elements (hipHostMalloc with the caller's flags), owned the same way; reads like the pointer it holds
template <class T>
struct PinBuf {
    T *ptr = nullptr;
    PinBuf() = default;
    PinBuf(const PinBuf &) = delete;
    PinBuf &operator=(const PinBuf &) = delete;
    PinBuf(PinBuf &&o) noexcept : ptr(o.ptr) { o.ptr = nullptr; }
    PinBuf &operator=(PinBuf &&o) noexcept {
        if (this != &o) { release(); ptr = o.ptr; o.ptr = nullptr; }
        return *this;
    }
    ~PinBuf() { release(); }
    void release() {
        if (ptr) (void)hipHostFree(ptr);
        ptr = nullptr;
    }
    int alloc(size_t count, unsigned flags) {
        release();
        hipError_t e = hipHostMalloc((void **)&ptr, sizeof(T) * count, flags);
        if (e != hipSuccess) { ptr = nullptr; return fail("hipHostMalloc(%zu bytes) failed: %s", sizeof(T) * count, hipGetErrorString(e)); }
        return 0;
    }
    operator T *() const { return ptr; }
};
// A resident per-chain track of the batch and which chains hold one (ChainFlags, csr_chain_tracks.h): Npad + 64 elements laid out
// like the reference-layout arrays (chain i at ChainInfo::off), from dalloc -- it dies with the batch -- allocated and zeroed at
// first use.  `what` is how the error texts name the track.
struct csr_ctx;
template <class T>
struct ChainTrack : ChainFlags {
    T *d = nullptr;
    const char *what;
    explicit ChainTrack(const char *what_) : what(what_) {}
    int ensure(csr_ctx *c);
    T *at(const csr_ctx *c, int chain) const;
    // the chain's n elements from / to the host, synchronised: upload marks the chain, download fails on a chain without the track
    int upload(csr_ctx *c, int chain, const T *host);
    int download(csr_ctx *c, int chain, T *host) const;
};
// N device arrays of one element per chain (dalloc: they die with the batch) and the pinned staging of their uploads, one slot each
// (an upload from pageable memory may hold the host): the masks and run tables of the groups of a pipelined step
struct csr_ctx;
template <class T, int N>
struct GroupSlots {
    T *d[N] = {};
    PinBuf<T> pin;
    size_t stride = 0;
    int ensure(csr_ctx *c, int nc);
    T *host(int i) const { return pin.ptr + (size_t)i * stride; }
    T *dev(int i) const { return d[i]; }
    // slot i := the stride elements at src, on stream st
    int upload(int i, const T *src, hipStream_t st) {
        std::copy(src, src + stride, host(i));
        HIPOK(hipMemcpyAsync(d[i], host(i), sizeof(T) * stride, hipMemcpyHostToDevice, st));
        return 0;
    }
};

// One forward pass / one smoother pass as its caller describes it (forward_impl, backward_impl).  Everything a pass depends on
// beyond the resident arrays is in here, so that settle() can replay the pass from the copy kept in csr_ctx::last.
struct FwdPass {
    uint32_t flags = 0;
    bool wantD = false;                     // NIS / NLL track and per-chain sums
    const unsigned char *active = nullptr;  // device chain mask (nullptr: every chain)
    bool defer = false;                     // optimistic validation, checked at the next settle point
    bool side = false;                      // a smoother follows: the epilogue runs beside it on the side stream
    bool natOut = false;                    // the outputs also go to the reference layout
    bool split = false;                     // step_pipelined: return right behind a barrier-free state chain
    bool sweep = false;                     // inner ECM sweep (Prm::qFromKappa, storePP)
    float *kappaIn = nullptr;               // ECM sweep: the kappa of the previous sweep's E-step (nullptr: the resident one)
};
// estep: 0 = plain smoother; 1 = ECM sweep whose kappa E-step is evaluated inside the smoother chain, moments stored;
//        2 = same, but the smoothed moments are not stored (an inner sweep nobody reads them from)
struct BwdPass {
    const unsigned char *active = nullptr;
    bool defer = false, natOut = false;
    int estep = 0;
    bool preferNatIn = false;               // a group's tail of a pipelined step: read xf / Pf in the reference layout
    float *kappaIn = nullptr, *kappaOut = nullptr;      // ECM sweep with the E-step inside the smoother (nullptr: the resident kappa)
};

// Everything that dies with the configured batch (DESIGN.md "Lifetimes"): the chain table, the kernel parameters, every pointer into
// memory that dalloc registers in `allocs` or into pinned memory sized by the batch, and every statement about the resident results.
// free_batch() frees `allocs` and assigns a default-constructed BatchState: a member declared here with its default needs no line
// anywhere else.
struct BatchState {
    bool configured = false;
    csr_model mdl{};
    int64_t m = 0;
    std::vector<ChainInfo> chains;
    int64_t Npad = 0, NB = 0, NG = 0, TN = 0;
    bool statsValid = false;
    bool haveFwd = false, haveBwd = false;
    // Resident copies.  Every result array has up to two copies: the blocked (tile-transposed) one the chains walk (Prm::t*) and
    // the reference-layout one callers download (nat[]).  where[id].blocked / .nat say which of them holds the resident result of
    // EVERY chain, at the boundaries of a C-ABI call (inside a pipelined step groups of chains are at different stages).  A pass
    // marks what it wrote (produced), an export converts only what is not .nat and a reader of the blocked layout imports only
    // what is not .blocked (need_natural, need_blocked); new inputs to a pass invalidate (new_forward_pass, new_smoothed_fit,
    // multipliers_changed).  A caller that asks chain by chain therefore converts the batch once, not once per chain.
    struct Where { bool blocked = true, nat = false; };
    std::array<Where, CSR_ARR_COUNT> where{};
    // The last forward pass and the last smoother pass, as launched: EVERY pass records itself here, deferred or not.  fwdPending /
    // bwdPending: its optimistic validation has not been read yet; exports: what was exported from the unvalidated results.
    // settle() replays from these descriptors (drop_pending, replay_covers_every_chain, reexport_on_replay are the only other writers).
    struct LastPass {
        FwdPass fwd;
        BwdPass bwd;
        bool fwdPending = false, bwdPending = false;
        uint32_t exports = 0;
    } last;
    bool sideSumsDone = false;          // the pending side-stream work already includes the per-chain sums (join_side only waits)
    bool fwdInternal = false;   // forward results were produced by this library (vs imported through csr_backward_pass)
    Prm p{};
    std::vector<void *> allocs;
    // device arrays not in Prm
    int64_t *dChainFirst = nullptr, *dChainNb = nullptr;
    int64_t *dChainOff = nullptr, *dChainLen = nullptr;     // natural offset / length of every chain (bins)
    unsigned char *dActive = nullptr;
    float *dLatent = nullptr;
    float *nat[CSR_ARR_COUNT] = {nullptr};
    // mailbox: [20 x u32 monotonic re-run counters: 0-3 cumulative per stage (covariance, state, smoother, debug), 4-15 per
    // stage and validation-pass index, 16 scratch | sumD[nchains] | sumNLL[nchains]] in device memory, mirrored into pinned
    // host memory with ONE copy per settle point
    char *dMail = nullptr;
    PinBuf<char> hMail;
    size_t mailBytes = 0;
    unsigned int lastCnt[20] = {0};
    // deferred validation launches nPasses[stage] validation passes back to back; the stage stands iff the LAST of them
    // re-ran nothing (then it was a fixed point).  Isolated speculation failures -- the normal case when the data has a
    // longer memory than the window (small Q0) -- are repaired by pass 1 and confirmed by pass 2 without a pipeline replay.
    int nPasses[3] = {1, 1, 1};
    int cleanRuns[3] = {0, 0, 0};
    // Warm-started speculation inside the ECM loop (csr_ctx::wsEnabled): what the resident checkpoints are
    bool wsActive = false;      // set by the ECM loop around its sweeps
    bool wsCold = false;        // replay of a failed iteration: record checkpoints, do not start from them
    int wsSavedF = 0, wsSavedB = 0;         // window length the resident checkpoints were recorded for (0: none)
    int wsSweepF = 0, wsSweepB = 0;         // parity of the double buffers
    void *ckF[2] = {nullptr, nullptr}, *ckB[2] = {nullptr, nullptr};
    bool natSZValid = false;    // sbNatSZ holds the current statistics of every chain
    bool gainNat = false;       // this forward pass's covariance chain wrote sbNatGain itself (walk_nat_gain)
    float4 *sbNatGain = nullptr, *sbNatSZ = nullptr;    // natural-layout records of the systolic walker (ensure_sb_nat)
    struct SbView {
        bool ready = false;
        int B = 0;
        int64_t NB = 0, NG = 0, TN = 0;
        int4 *blk = nullptr;
        int *blkChain = nullptr;
        int64_t *chainFirst = nullptr;
        void *carryIn = nullptr, *carryOutA = nullptr, *carryOutB = nullptr;
        unsigned long long *pub = nullptr;      // k_sb_async: carry[NB], {version, final}[NB], control words
    } sb;
    bool sidePending = false;
    double *dChainQ = nullptr;  // per-chain base process noise (csr_batch_set_chain_q)
    // ECM with the kappa E-step inside the smoother: a sweep's smoother writes kappa into a scratch buffer (BwdPass::kappaOut),
    // the next sweep's forward pass reads it (FwdPass::kappaIn); the resident tKap only changes when a whole iteration has been
    // validated.  Allocated on first use.
    float *kapScratch[2] = {nullptr, nullptr};
    bool fwdQCompact = false;   // the resident forward pass stored the diagonal of pNoise (tQ2) instead of pNoise (tQ)
    bool qDiagonal = true;      // the base process noise in use (model's, or every chain's) is diagonal
    bool modelQDiagonal = true, chainQDiagonal = true;
    Prm sidePrm{};              // parameters of the epilogue running on the side stream (its sums follow at the join)
    // device-resident background update (allocated on first use)
    struct BgState {
        bool ready = false, haveCur = false;
        int Bp = 0;
        BgPrm prm{};
        BgBatch bat{};
        int *dGroupChain = nullptr;
        double *out1 = nullptr;
        unsigned char *dActive = nullptr, *dHasSup = nullptr;
        double *dPen = nullptr;
        long long *dSelRank = nullptr;
    } bg;
    DevBuf bgBuf, wrBuf, textBuf;       // host-buffer background solver / bedGraph writer work space (this device)
    // Folded validation (Prm::prevKind): a clean optimistic stage leaves its check to the next speculative kernel; the two use
    // different carry sets.  pendChk = the check that has not been handed to a kernel yet (flushed by read_mail).
    struct PendingCheck {
        bool valid = false;
        int kind = 0, stage = 0;
        const void *cin = nullptr, *cout = nullptr;
        const unsigned char *active = nullptr;
    } pendChk;
    void *carrySet[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};   // [set][carryIn, carryOutA]
    int carryToggle = 0;
    // The state chain between sb_begin and sb_finish: `p` as the caller passed it, `q` / mode / grid / xf as the chain's kernels take
    // them.  launched: k_sb_async went out (ctl = its verdict words); watch: with per-chain done words for step_pipelined, which
    // finishes it -- `active` until then
    struct SbPending {
        bool active = false, launched = false, watch = false;
        Prm p{}, q{};
        int mode = 0, grid = 0;
        float2 *xf = nullptr;
        unsigned int *ctl = nullptr;
    } sbp;
    PinBuf<unsigned int> hDone;         // host-visible "chain is final" words (coherent, mapped) ...
    unsigned int *dDone = nullptr;      // ... and their device alias
    // step_pipelined: the chain mask of every tail group and of every NIS / NLL epilogue group (the early ones and the remainder's),
    // and the run table of every tail group's residual launch (k_resid_runs)
    GroupSlots<unsigned char, MAX_EARLY_TAILS + 1> tailMasks;
    GroupSlots<unsigned char, MAX_EARLY_EPILOGUES + 1> epiMasks;
    GroupSlots<ResidRun, MAX_EARLY_TAILS + 1> tailRuns;
    // csr_batch_set_step_groups (a test seam): the group of every chain, -1 = the remainder; empty = the watch loop groups the
    // chains by its thresholds as they become final
    std::vector<int32_t> tailScript, epiScript;
    bool pfPending = false;
    // the reference-layout process-noise array holds the constant fill of THESE values in every row (k_fill_rows): a step with the
    // same constant process noise does not write it again (a 1/8-genome step: one side-stream launch and two stream waits less)
    bool pnFillValid = false;
    float pnFillQ[4] = {0.f, 0.f, 0.f, 0.f};
    // The per-chain tracks of the peak stages (allocated at first use): the score track (csr_batch_rocco_scores / csr_batch_upload_scores),
    // the selection mask ROCCO leaves of it, and the DWB residual template of the robust null (csr_batch_null_prepare); which track
    // invalidates which is scores_changed()
    ChainTrack<double> scores{"scores"}, tmpl{"null template"};
    ChainTrack<unsigned char> sol{"ROCCO solution"};
    // broad mode (csr_host_broad.inl): the weak pass's mask and the mask of the bridged parents
    ChainTrack<unsigned char> weak{"weak ROCCO solution"}, broadParent{"broad parent mask"};
    // empirical-Bayes state shrinkage (csr_host_shrink.inl): the float32 variance track csr_batch_shrink_prepare makes and the
    // posterior tracks csr_batch_shrink_posterior leaves
    ChainTrack<float> shrinkVar{"shrinkage variance track"}, shrunk{"shrunk track"}, shrunkSd{"shrunk posterior sd track"},
        shrunkSpike{"shrunk spike probability track"}, shrunkSlabMean{"shrunk slab mean track"},
        shrunkSlabWeight{"shrunk slab weight track"};
    // the dense observation-variance seed loop (csr_host_munc.inl): its arrays in the batch's own layout ((m, Npad) per cell, Npad per
    // interval), from dalloc at the first csr_batch_munc_seed_begin.  total / rho / omega are double-buffered: a pass reads [cur] and
    // writes [1 - cur].  idx / dOff / dLen: the chains the loop takes; work: the invalid flag, the fallback count and one word per row
    struct MuncSeed {
        bool ready = false, useCountFloor = false, useExclude = false;
        int cur = 0;
        std::vector<int> idx;
        int64_t longest = 0;
        int64_t *dOff = nullptr, *dLen = nullptr;
        float *total[2] = {nullptr, nullptr}, *rho[2] = {nullptr, nullptr}, *omega[2] = {nullptr, nullptr};
        float *local = nullptr, *smooth = nullptr, *weight = nullptr, *g = nullptr, *gvar = nullptr, *countFloor = nullptr;
        unsigned char *exclude = nullptr;
        unsigned int *work = nullptr;
        double *w64 = nullptr, *gSel = nullptr;     // seed background: float64 weight track; per-chain penalty and clip of the G proxy
        unsigned long long *rankCount = nullptr;
        unsigned int *rankTrial = nullptr;
        double bgPad = 0.0;
        bool bgUseWeights = true;
        csr_munc_seed_stats stats{};
        // finished tracks (csr_host_munc_track.inl), each from dalloc at its first use: the prior variance track (per interval),
        // the caller's raw count floor with its NaNs ((m, Npad)) and the finished track before it becomes the batch's munc
        float *prior = nullptr, *trackFloor = nullptr, *track = nullptr;
    } seed;
    int exportSignal = 0;       // CSR_SIGNAL_*: what the export stages read as signal (csr_batch_set_export_signal)
    // ROCCO's work arrays without presence (csr_host_rocco.inl): backtrace words, per-chain maxima and flags; its growable work
    // space is csr_ctx::roccoWs
    struct Rocco {
        double *mx = nullptr;
        unsigned long long *bt = nullptr;
        int *bad = nullptr;
    } rocco;
    // stats
    csr_run_stats rs{};
};

// What lives as long as the context: the device, streams and events, tuning (given, or adapted from what earlier passes saw: it
// survives a reconfigure), profiling, and work space kept across batches (DevBuf members: they free themselves).
struct csr_ctx : BatchState {
    int device = 0;
    hipStream_t stream = nullptr;
    // tuning
    int B = 0;                 // block length; 0 = chosen from the batch size at configure time
    // speculative warm-up in bins (multiples of 16).  Defaults follow the validation mode (mode_warm_defaults): bitwise
    // coalescence of float32-rounded trajectories needs ~4x the window that k-ulp agreement does.
    int warmP = 256, warmX = 256, warmB = 128;
    bool pinP = false, pinX = false, pinB = false, pinFM = false;
    int warmFM = 96;            // fused forward chain with per-bin multipliers (see forward_impl)
    int *fwdWindow = nullptr;   // window variable of the forward stage being launched (see stage_warm)
    int *bwdWindow = nullptr;   // ... of the smoother stage (warm-started ECM sweeps)
    int *lastBwdWindow = nullptr;
    // Warm-started speculation inside the ECM loop (Prm::ckptIn): a sweep's chains start their windows from the carries the
    // previous sweep recorded (double-buffered per direction, BatchState::ckF / ckB), with windows of wsWarmF / wsWarmB bins
    // instead of the cold ones.  A failed validation at a wavefront's edge widens them; a window that changed since the
    // checkpoints were recorded makes the next sweep start cold once.
    bool wsEnabled = true;      // CONSENRICH_AMD_WARMSTART=0: off
    int wsWarmF = 32, wsWarmB = 32;         // warm-started windows (widen themselves when an edge block fails)
    static constexpr int wsMaxBlock = 32;   // largest block length (= batch size class) that warm-starts
    int *lastFwdWindow = nullptr;   // ... of the last forward stage launched (a failed settle widens that one)
    bool Bfixed = false;
    bool adaptWarm = true;
    bool useDmaWarm = true;    // ... and, with reference-layout outputs, for its warm-up phase
    bool useDmaFused = true;   // fused forward chain without reference-layout outputs: LDS-DMA ring
    bool useDma = true;        // LDS-DMA speculative kernels for the chains that provide them
    int xTolUlps = 0;           // carry validation: 0 = bit-exact sequential semantics (DEFAULT of every context since round 3: the
                                // only mode that holds the parity gate through the ECM loop on ill-conditioned data, tests/test_hard_data.py);
                                // k > 0 = k-ulp acceptance, the opt-in throughput mode (csr_set_validation / CONSENRICH_AMD_XTOL_ULPS)
    bool dstatLdsRaised = false;        // (both reference-layout-output instances of k_fwd_dstat)
    bool natInEnabled = true;           // CONSENRICH_AMD_NATIN=0 (tests): the smoother never reads the reference layout -- blocked copies
                                        // a forward pass did not write are brought back first (need_blocked)
    double lastSbLoopUs = 0.0;          // how long the host watched the previous single launch of the state chain (step_pipelined)
    double lastWaitUs[2] = {0.0, 0.0};  // how long the previous host wait for the stream lasted, per wait site (wait_stream polls around that moment)
    bool sbAsyncLdsRaised[3] = {false, false, false};   // per context = per device (HIP keeps the attribute per device)
    int launchedPasses[3] = {1, 1, 1};  // validation passes the last launch of a stage made (BatchState::nPasses)
    // deferred validation: a stage whose last synchronous run needed no re-run is launched optimistically (speculative
    // pass + one validation pass, no host round trip); the counters are checked at the next settle point and the
    // pipeline is re-run synchronously from the first stage that did re-run blocks.
    bool deferEnabled = true;
    bool seqState = false;      // bit-exact validation, levelTrend: one wavefront per chain walks the state chain sequentially (CONSENRICH_AMD_SEQ_STATE=1)
    // bit-exact validation, levelTrend (default): the state chain speculates on SUPERBLOCKS of sbBins bins with an sbWarm-bin
    // window -- two float32-rounded state trajectories need ~10^4 bins to coincide bit for bit (scripts/ubench/merge_time.c),
    // so the batch's own 32..256-bin blocks never validate; the gain / statistics records are re-blocked into a second view
    // of the batch (own block table and carries, BatchState::sb) for this one chain and the filtered state is re-blocked back
    // (CONSENRICH_AMD_SEQ_STATE=1 is the sequential yardstick)
    int sbBins = 8192;          // CONSENRICH_AMD_SB_BINS (default: chosen from the batch, ensure_sb_view)
    // k_sb_delta's fallback rule (CONSENRICH_AMD_SB_ADV = "min,from"): walk the rest of a batch when, from round `from` on, the
    // rounds have settled fewer than `min` bins each.  Measured flat between "give up after 20 rounds" (4,20) and "walk as soon
    // as a round is worth less than its six steps" (6,2): 3.75-3.95 ms of repairs either way (profiles/r03_sb_sweeps.txt) -- where
    // the levels flip densely a round and the steps it replaces cost the same.
    int sbAdvMin = 4, sbAdvFrom = 20;
    bool sbBinsPinned = false;  // CONSENRICH_AMD_SB_BINS given: no automatic choice of the superblock length
    // CONSENRICH_AMD_SB_ASYNC=0: speculative pass + repair passes as separate launches (k_sb_sys / k_sb_delta) instead of the
    // barrier-free single launch (k_sb_async); sbSpinLimit bounds every wait inside it (polls of ~2 us; then: bail out to the pass form)
    bool sbAsync = true;
    int sbSpinLimit = 1 << 19;
    // debugging switches, read once from the environment at creation (never on the launch path)
    bool dbgLog = false;
    bool optimistic[3] = {true, true, true};
    DevBuf qsBuf, qpBuf;                // Q0-seed work space (sampling / posterior)
    DevBuf stageBuf;                    // host -> device staging of per-bin vectors (csr_batch_upload_multipliers)
    hipStream_t side = nullptr;         // NIS/NLL epilogue runs here, concurrently with the smoother chain
    hipEvent_t evFork = nullptr, evJoin = nullptr;
    hipEvent_t evFork2 = nullptr, evPf = nullptr;      // early covariance exports on the side stream (bit-exact mode)
    // step_pipelined: tails of the chains whose filtered state stands, on a stream of their own while the state chain runs
    hipStream_t tail = nullptr;
    hipEvent_t evTailJoin = nullptr;
    // ... and their NIS / NLL epilogue in groups of its own on the side stream, which continues from the point of the main stream
    // right in front of the state chain (evEpiFork); the main stream waits for evEpiJoin before the per-chain sums
    hipEvent_t evEpiFork = nullptr, evEpiJoin = nullptr;
    // first-use zeroing of a reference-layout array (nat_array) runs HERE and is waited for by the host before the array is
    // handed out: it is ordered against no other stream, so it does not matter which stream the caller is on at that moment
    hipStream_t zeroStream = nullptr;
    hipStream_t mainStream = nullptr;   // what `stream` is outside step_pipelined's tail groups (csr_run_stats.nat_first_use_off_main)
    // CONSENRICH_AMD_TAIL_PCT="first,next": share of the batch's bins a group of finished chains must reach.  Round 4: 60 / 40 (round 3:
    // 50 / 15) -- tail kernels take issue slots from the walking wavefronts, so fewer, later groups win (profiles/r04_tail_sweep.txt)
    int tailFirstPct = 60, tailNextPct = 40;
    bool tailSplit = true;      // CONSENRICH_AMD_TAIL_SPLIT=0: a step's tail follows the state chain for all chains at once
    // CONSENRICH_AMD_EPILOGUE_PCT: share of the batch's bins that final chains without an epilogue must reach for an early epilogue
    // group (0: no early groups)
    int epiPct = 10;
    // ROCCO (csr_host_rocco.inl): tuning, counters and growable work space; the batch's tracks are BatchState::scores / sol
    struct RoccoWs {
        int depth = 0;          // speculation depth of the calibration (0 = default)
        DevBuf work, arena, runBuf;
        csr_rocco_stats stats{};
    } roccoWs;
    // nested ROCCO refinement (csr_host_nested.inl): growable work space of a call -- the staged host arrays, the job / parameter /
    // order tables, one double and one mask byte per bin, back-pointer words, per-region state and records, and the candidate runs
    // of the last layer, which stay until the next one so that the caller can fetch them
    struct NestedWs {
        DevBuf arena, jobBuf, work, wm, bt, st, rec, kids, part, costs;
        int64_t nKids = 0;
    } nestedWs;
    // narrowPeak export (csr_host_export.inl): the staged host tracks, the parent records, the first peak of every parent and the
    // peaks of the last call, which stay until the next one so that the caller can fetch them; the rest is nestedWs
    struct ExportWs {
        DevBuf arena, par, base, peaks;
        int64_t nPeaks = 0;
    } exportWs;
    // massive sub-peak clean-up (csr_host_cleanup.inl): the staged scores and edges, one work double per bin, the children and per
    // child its segment records, counters and node record
    struct CleanupWs {
        DevBuf arena, work, kids, seg, cnt, node;
    } cleanupWs;
    // broad mode (csr_host_broad.inl): the staged arrays, one work double per bin, the job and chain tables (or the gaps), the parent
    // mask and the records (or the gap sums)
    struct BroadWs {
        DevBuf arena, work, mask, jobs, rec, runs;
        std::vector<csr_broad_run> kept;    // the records of the last csr_batch_broad_runs (compact: they wait on the host)
    } broadWs;
    // stationary-null DWB panel (csr_host_dwb.inl): chain table, weights, templates, the seed's noise stream and the rows of one
    // group of draws; growable, the large ones given back by csr_dwb_panel_end
    struct Dwb {
        bool ready = false;
        std::vector<DwbChain> chains;
        int64_t rowLen = 0, longest = 0, strideMax = 0, maxChunks = 1;
        int nDraws = 0, group = 0;
        DevBuf chainBuf, wtsBuf, tmplBuf, noiseBuf, rowBuf, partBuf, outBuf, vecBuf, xBuf, meanBuf;
    } dwb;
    // robust null (csr_host_null.inl): growable work space of a call -- track table, the two key buffers of the sort, the compacted
    // supports and their tile counts, chunk sums, job tables, small results, uploaded host vectors
    struct NullWs {
        DevBuf trackBuf, keysA, keysB, comp, cnt, part, jobBuf, outBuf, xBuf;
    } nullWs;
    // effective sample size scan (csr_host_ess.inl): growable work space of a call -- track table, the centred series, the sums and
    // pair counts of a round of lags, the means, an uploaded host vector and its mask
    struct EssWs {
        DevBuf trackBuf, cenBuf, sumBuf, pairBuf, outBuf, xBuf, maskBuf;
    } essWs;
    // multiscale candidate segments (csr_host_segments.inl): growable work space and the result of the last run, which stays
    // until the next run so that the caller can resolve flagged views and fetch the rows
    struct Seg {
        DevBuf chainBuf, prefixBuf, excessBuf, exPrefixBuf, cntBuf, runBuf, keepBuf, statBuf, metaBuf, baseBuf, outBuf, xBuf;
        bool have = false;
        bool deviceOnly = false;    // a replay pool is open (csr_dwb_panel_pool_begin): a run's rows stay on the device
        int cap = 0;
        std::vector<int64_t> rowsPerTrack, counters;    // [track], [track][3]
        std::vector<int64_t> oStart, oEnd, oScale, oView;
        std::vector<double> oScore, oInteg, oMean, oMax;
        struct Flagged {        // a view over the cap whose chosen set the values alone do not determine
            int track, scaleIndex, view;
            int64_t base;       // its `cap` output rows
            std::vector<int64_t> start, end;
            std::vector<double> score, integ, mean, mx;
            bool resolved;
        };
        std::vector<Flagged> flagged;
    } seg;
    // dependence span (csr_host_depspan.inl): growable work space of a call -- a staged host matrix or window set, the matrix / window /
    // row / pair tables, the difference flags, and per (window, row) of a group the compacted and the centred values, the finite
    // counts, the lag sums and pair counts, the per-lag pooling arrays and the window records
    struct DepWs {
        DevBuf stageBuf, matBuf, winBuf, rowBuf, pairTab, diffBuf, compBuf, cenBuf, nfinBuf, sumBuf, pairBuf, lagBuf, medBuf, recBuf;
    } depWs;
    // empirical-Bayes state shrinkage (csr_host_shrink.inl): the prepared input -- staged host arrays (default context) or the chains
    // of the batch a mask took (fromBatch: it dies with the batch) -- with its chain table and per-block valid counts, and the work
    // space of a pass: tile partials, folded sums, the parameter set, posterior tracks of host arrays, median keys
    struct ShrinkWs {
        bool ready = false, fromBatch = false;
        std::vector<ShrinkChain> chains;
        std::vector<int> idx;               // where chain k's sums go in the caller's output
        ShrinkTrack tr{};
        int64_t block = 1, total = 0, longest = 0, nTiles = 0, nBlocks = 0;
        size_t nOut = 0;
        DevBuf xBuf, vBuf, chainBuf, cntBuf, partBuf, outBuf, priorBuf, postBuf, keyBuf;
    } shrinkWs;
    // dense observation-variance seed natives on host arrays (csr_host_munc.inl): the staged inputs, the outputs, flags and row words
    struct MuncWs {
        DevBuf in, out, flag;
    } muncWs;
    // DWB peak scoring (csr_host_peakscore.inl): growable work space of a call -- an uploaded host track, the segments, views and
    // results of a scoring call, the observed and pooled statistics with their p / q values (sorted through nullWs)
    struct PeakWs {
        DevBuf xBuf, segBuf, pqBuf;
    } peakWs;
    // the replay pool of a DWB panel (csr_dwb_panel_pool_*): per chain the three metric columns (score, integrated excess, max
    // excess) of every replay candidate that survives the total cap, appended group by group; freed by csr_dwb_panel_end
    struct PeakPool {
        bool active = false;
        int nc = 0, nDraws = 0;
        int64_t totalCap = 0;               // 0: no total cap
        std::vector<DevBuf> col;            // [chain][3]
        std::vector<int64_t> n, cap;        // values held / capacity per chain
        std::vector<int64_t> count, before; // [chain][draw]: candidates after / before the total cap (-1: draw not appended)
        std::vector<int64_t> counters;      // [chain][draw][3]: phase 1's (eligible, views over the cap, discarded by the per-view cap)
        std::vector<double> mx;             // [chain][draw]: np.max of the kept scores (0.0 without candidates)
        struct Flagged {                    // a draw over the total cap with a NaN score: the caller decides it
            int chain, draw;
            int64_t rowBase, rows, slot;    // its rows in the last run's output; where its `totalCap` values go in the pool
            bool resolved;
        };
        std::vector<Flagged> flagged;
        int64_t fetchedTracks = 0;
        DevBuf jobBuf, outBuf;
    } pool;
    // profiling
    bool profiling = false;
    std::map<std::string, ProfEntry> prof;
    std::vector<hipEvent_t> eventPool;
};

static int settle(csr_ctx *c);
static void peak_pool_release(csr_ctx *c);      // csr_host_peakscore.inl
static int export_impl(csr_ctx *c, uint32_t what);
static ChainTrack<float> &shrink_track(csr_ctx *c, int which);     // csr_host_shrink.inl

// The pass that just ran wrote these arrays in the given copies (and not in the other)
enum : unsigned { W_BLOCKED = 1u, W_NAT = 2u };
static void produced(csr_ctx *c, std::initializer_list<int> ids, unsigned copies) {
    for (int id : ids) c->where[id] = csr_ctx::Where{(copies & W_BLOCKED) != 0, (copies & W_NAT) != 0};
}
// New inputs: whatever the reference layout holds is no longer the resident result (the blocked copies are what the next pass writes)
static void new_forward_pass(csr_ctx *c) { produced(c, {CSR_ARR_D, CSR_ARR_XF, CSR_ARR_PF, CSR_ARR_PNOISE}, W_BLOCKED); }
static void new_smoothed_fit(csr_ctx *c) { produced(c, {CSR_ARR_XS, CSR_ARR_PS, CSR_ARR_LAG}, W_BLOCKED); }
static void multipliers_changed(csr_ctx *c) { produced(c, {CSR_ARR_LAMBDA, CSR_ARR_KAPPA, CSR_ARR_QSCALE}, W_BLOCKED); }

// Pending optimistic validations (csr_ctx::last)
static bool anything_pending(const csr_ctx *c) { return c->last.fwdPending || c->last.bwdPending; }
// the pending validations have been read (or their results are gone): nothing is left for settle() to replay
static void drop_pending(csr_ctx *c) {
    c->last.fwdPending = c->last.bwdPending = false;
    c->last.exports = 0;
}
// the smoother ran group by group under chain masks (step_pipelined): a replay after a failed validation covers every chain
static void replay_covers_every_chain(csr_ctx *c) { c->last.bwd.active = nullptr; }
// arrays exported from unvalidated results: settle() exports them again if it has to replay
static void reexport_on_replay(csr_ctx *c, uint32_t what) { c->last.exports |= what; }
// forward results that came in through csr_backward_pass: no pass of this library produced them (flags 0: no multipliers)
static void forward_imported(csr_ctx *c) {
    c->fwdInternal = false;
    c->fwdQCompact = false;
    c->last.fwd = FwdPass{};
}
// the resident forward pass ran with one constant process noise per chain (no kappa / qScale / adaptive noise)
static bool const_q(const csr_ctx *c) { return c->fwdInternal && !(c->last.fwd.flags & (F_APN | F_QSCALE | F_KAPPA)); }

static int ctx_select(csr_ctx *c) {
    HIPOK(hipSetDevice(c->device));
    return 0;
}

template <class T>
static int dalloc(csr_ctx *c, T **ptr, int64_t count) {
    void *q = nullptr;
    const size_t bytes = (size_t)std::max<int64_t>(count, 1) * sizeof(T);
    hipError_t e = hipMalloc(&q, bytes);
    if (e != hipSuccess) return fail("hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
    c->allocs.push_back(q);
    *ptr = reinterpret_cast<T *>(q);
    return 0;
}
template <class T, int N>
int GroupSlots<T, N>::ensure(csr_ctx *c, int nc) {
    if (pin) return 0;
    for (T *&x : d) CHECK(dalloc(c, &x, nc));
    stride = (size_t)nc;
    return pin.alloc((size_t)N * stride, hipHostMallocDefault);
}

template <class T>
int ChainTrack<T>::ensure(csr_ctx *c) {
    if (d) return 0;
    CHECK(dalloc(c, &d, c->Npad + 64));
    HIPOK(hipMemsetAsync(d, 0, sizeof(T) * (size_t)(c->Npad + 64), c->stream));
    have.assign(c->chains.size(), 0);
    return 0;
}
template <class T>
T *ChainTrack<T>::at(const csr_ctx *c, int chain) const { return d + c->chains[chain].off; }
template <class T>
int ChainTrack<T>::upload(csr_ctx *c, int chain, const T *host) {
    CHECK(ensure(c));
    HIPOK(hipMemcpyAsync(at(c, chain), host, sizeof(T) * (size_t)c->chains[chain].n, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    set(chain, true);
    return 0;
}
template <class T>
int ChainTrack<T>::download(csr_ctx *c, int chain, T *host) const {
    if (!has(chain)) return fail("chain %d has no %s", chain, what);
    HIPOK(hipMemcpyAsync(host, at(c, chain), sizeof(T) * (size_t)c->chains[chain].n, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    return 0;
}
// New scores of a chain: the selection mask made of the previous ones is dropped.  The chain's null template is NOT: it stays
// present although it came from the previous scores -- that is how the stages have behaved since they landed, kept as it is.
static void scores_changed(csr_ctx *c, int chain) {
    c->sol.set(chain, false);
    if (c->weak.d) c->weak.set(chain, false);
    if (c->broadParent.d) c->broadParent.set(chain, false);
}

static int need(csr_ctx *c);    // csr_host_batch.inl
static int check_chain(const csr_ctx *c, int chain) {
    if (chain < 0 || chain >= (int)c->chains.size()) return fail("chain index out of range");
    return 0;
}
// what every per-chain transfer entry checks first: a configured batch, the chain index, the caller's buffer
static int need_chain(csr_ctx *c, int chain, const void *host) {
    CHECK(need(c));
    CHECK(check_chain(c, chain));
    if (!host) return fail("null host buffer");
    return 0;
}
static int check_finite(const char *name, const double *x, int64_t n) {
    for (int64_t i = 0; i < n; ++i)
        if (!std::isfinite(x[i])) return fail("`%s` contains non-finite values", name);
    return 0;
}
// idx := the chains chain_mask takes (nullptr: every chain), in order.  A taken chain without the track fails with "chain i has no
// ..."; idx then holds the taken chains in front of it.  ifNone: what a batch that never held the track answers instead
static const char NO_SCORES[] = "no scores: call csr_batch_rocco_scores or csr_batch_upload_scores first";
template <class T>
static int select_chains(csr_ctx *c, const unsigned char *chain_mask, const ChainTrack<T> &track, std::vector<int> &idx,
                         const char *ifNone = nullptr) {
    idx.clear();
    if (ifNone && !track.d) return fail("%s", ifNone);
    const int missing = take_chains((int)c->chains.size(), chain_mask, track, idx);
    return missing < 0 ? 0 : fail("chain %d has no %s", missing, track.what);
}

// Ends the configured batch: its device memory is freed and every BatchState member is back at its default (DevBuf / PinBuf members
// free what they own when they are assigned to).  The device must be selected.
static void free_batch(csr_ctx *c) {
    if (c->tail) (void)hipStreamSynchronize(c->tail);
    if (c->side) (void)hipStreamSynchronize(c->side);
    for (void *q : c->allocs) (void)hipFree(q);
    static_cast<BatchState &>(*c) = BatchState{};
    if (c->shrinkWs.fromBatch) c->shrinkWs.ready = false;       // (its tracks were the batch's)
}

// Warm-up windows that gave zero re-runs on the bench workload with margin (hg38 x 32 synthetic: the state chain needs
// 64 bins at k = 2, the covariance chain 64, the smoother 48; exact mode 256 / 256 / 128).  run_chain lengthens them
// when the data has a longer filter memory; results never depend on them.
static void mode_warm_defaults(csr_ctx *c) {
    const bool tol = c->xTolUlps > 0;
    c->optimistic[1] = tol;     // bit-exact state chains re-run blocks on most calls: validate them synchronously
    if (!c->pinP) c->warmP = tol ? 80 : 256;
    if (!c->pinX) c->warmX = tol ? 80 : 256;
    if (!c->pinB) c->warmB = tol ? 64 : 128;
}

extern "C" csr_ctx *csr_create(int device_ordinal) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        fail("no HIP device visible: consenrich_amd has no CPU fallback");
        return nullptr;
    }
    if (device_ordinal < 0 || device_ordinal >= n) {
        fail("device ordinal %d out of range (0..%d)", device_ordinal, n - 1);
        return nullptr;
    }
    csr_ctx *c = new csr_ctx();
    c->device = device_ordinal;
    if (hipSetDevice(c->device) != hipSuccess || hipStreamCreate(&c->stream) != hipSuccess) {
        fail("cannot initialise device %d", device_ordinal);
        delete c;
        return nullptr;
    }
    c->mainStream = c->stream;
    if (hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&c->evFork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->evJoin, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->evFork2, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->evPf, hipEventDisableTiming) != hipSuccess ||
        hipStreamCreateWithFlags(&c->tail, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&c->zeroStream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&c->evTailJoin, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->evEpiFork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->evEpiJoin, hipEventDisableTiming) != hipSuccess) {
        fail("cannot create the side stream of device %d", device_ordinal);
        delete c;
        return nullptr;
    }
    const char *e;
    if ((e = getenv("CONSENRICH_AMD_BLOCK"))) { c->B = atoi(e); c->Bfixed = c->B != 0; }
    if ((e = getenv("CONSENRICH_AMD_WARM"))) {
        // "p,x,b[,fm]": warm-up windows (bins) of the covariance / state / smoother chains and of the fused forward chain with
        // per-bin multipliers; -1 leaves one at its default (csr_set_tuning is the API for the first three)
        int w[4] = {-1, -1, -1, -1};
        (void)sscanf(e, "%d,%d,%d,%d", &w[0], &w[1], &w[2], &w[3]);
        if (w[0] >= 0) { c->warmP = w[0]; c->pinP = true; }
        if (w[1] >= 0) { c->warmX = w[1]; c->pinX = true; }
        if (w[2] >= 0) { c->warmB = w[2]; c->pinB = true; }
        if (w[3] >= 0) { c->warmFM = w[3]; c->pinFM = true; }
    }
    if ((e = getenv("CONSENRICH_AMD_XTOL_ULPS"))) c->xTolUlps = atoi(e);
    if ((e = getenv("CONSENRICH_AMD_DEFER"))) c->deferEnabled = atoi(e) != 0;
    if ((e = getenv("CONSENRICH_AMD_NATIN"))) c->natInEnabled = atoi(e) != 0;
    if ((e = getenv("CONSENRICH_AMD_SEQ_STATE"))) c->seqState = atoi(e) != 0;
    if ((e = getenv("CONSENRICH_AMD_WARMSTART"))) c->wsEnabled = atoi(e) != 0;
    if ((e = getenv("CONSENRICH_AMD_SB_ADV"))) {
        int a = 4, f = 20;
        if (sscanf(e, "%d,%d", &a, &f) >= 1) { c->sbAdvMin = std::min(255, std::max(0, a)); c->sbAdvFrom = std::min(255, std::max(1, f)); }
    }
    if ((e = getenv("CONSENRICH_AMD_SB_BINS"))) { c->sbBins = std::max(64, (atoi(e) + 63) / 64 * 64); c->sbBinsPinned = true; }
    if ((e = getenv("CONSENRICH_AMD_SB_ASYNC"))) c->sbAsync = atoi(e) != 0;
    if ((e = getenv("CONSENRICH_AMD_TAIL_SPLIT"))) c->tailSplit = atoi(e) != 0;
    if ((e = getenv("CONSENRICH_AMD_TAIL_PCT"))) {
        int a = 60, b = 40;
        if (sscanf(e, "%d,%d", &a, &b) >= 1) { c->tailFirstPct = std::min(100, std::max(1, a)); c->tailNextPct = std::min(100, std::max(1, b)); }
    }
    if ((e = getenv("CONSENRICH_AMD_EPILOGUE_PCT"))) c->epiPct = std::min(100, std::max(0, atoi(e)));
    if ((e = getenv("CONSENRICH_AMD_SB_SPIN_LIMIT"))) c->sbSpinLimit = std::max(1, atoi(e));
    c->dbgLog = getenv("CONSENRICH_AMD_DEBUG") != nullptr;
    mode_warm_defaults(c);
    if ((e = getenv("CONSENRICH_AMD_DMA"))) c->useDma = c->useDmaFused = c->useDmaWarm = atoi(e) != 0;     // 0: the plain-load forms of the chains (yardstick of the LDS-DMA ring tests)
    if (c->B != 0 && (c->B < 32 || (c->B % 32) != 0)) c->B = 0;
    return c;
}

extern "C" void csr_destroy(csr_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    if (c->side) (void)hipStreamSynchronize(c->side);
    free_batch(c);
    for (auto &kv : c->prof)
        for (auto &pr : kv.second.pending) {
            (void)hipEventDestroy(pr.first);
            (void)hipEventDestroy(pr.second);
        }
    for (hipEvent_t ev : c->eventPool) (void)hipEventDestroy(ev);
    if (c->evFork) (void)hipEventDestroy(c->evFork);
    if (c->evJoin) (void)hipEventDestroy(c->evJoin);
    if (c->evFork2) (void)hipEventDestroy(c->evFork2);
    if (c->evPf) (void)hipEventDestroy(c->evPf);
    if (c->evTailJoin) (void)hipEventDestroy(c->evTailJoin);
    if (c->evEpiFork) (void)hipEventDestroy(c->evEpiFork);
    if (c->evEpiJoin) (void)hipEventDestroy(c->evEpiJoin);
    if (c->tail) { (void)hipStreamSynchronize(c->tail); (void)hipStreamDestroy(c->tail); }
    if (c->zeroStream) (void)hipStreamDestroy(c->zeroStream);
    if (c->side) (void)hipStreamDestroy(c->side);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;       // (the device is still selected: the work buffers free themselves)
}

extern "C" int csr_set_tuning(csr_ctx *c, int32_t block_len, int32_t warm_p, int32_t warm_x, int32_t warm_b) {
    if (!c) return fail("null context");
    if (block_len != 0) {
        if (block_len < 32 || (block_len % 32) != 0) return fail("block_len must be a positive multiple of 32");
        if (c->configured && block_len != c->B) return fail("block_len cannot change after csr_batch_configure");
        c->B = block_len;
        c->Bfixed = true;
    }
    if (warm_p >= 0 || warm_x >= 0 || warm_b >= 0) c->adaptWarm = false;   // explicit tuning pins the windows
    if (warm_p >= 0) { c->warmP = (warm_p + 15) / 16 * 16; c->pinP = true; }
    if (warm_x >= 0) { c->warmX = (warm_x + 15) / 16 * 16; c->pinX = true; }
    if (warm_b >= 0) { c->warmB = (warm_b + 15) / 16 * 16; c->pinB = true; }
    return 0;
}

static csr_ctx *default_ctx();
extern "C" int csr_set_validation(csr_ctx *c, int32_t x_tol_ulps) {
    if (!c) c = default_ctx();      // NULL addresses the default context of the reference-shaped entry points
    if (!c) return -1;
    if (x_tol_ulps < 0 || x_tol_ulps > 64) return fail("x_tol_ulps must be in [0, 64]");
    c->xTolUlps = x_tol_ulps;
    mode_warm_defaults(c);
    return 0;
}

extern "C" int csr_synchronize(csr_ctx *c) {
    if (!c) return fail("null context");
    CHECK(ctx_select(c));
    if (c->configured) CHECK(settle(c));
    HIPOK(hipStreamSynchronize(c->stream));
    HIPOK(hipDeviceSynchronize());      // side stream, other contexts of this process: nothing is in flight on the device
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// profiling helpers: HIP events on the library's stream around every kernel launch
// ---------------------------------------------------------------------------------------------------------------
static hipEvent_t get_event(csr_ctx *c) {
    if (!c->eventPool.empty()) {
        hipEvent_t e = c->eventPool.back();
        c->eventPool.pop_back();
        return e;
    }
    hipEvent_t e;
    (void)hipEventCreate(&e);
    return e;
}
// (name == nullptr: no scope -- the caller holds one around several launches, or the launch is not counted)
struct Scope {
    csr_ctx *c;
    ProfEntry *pe = nullptr;
    hipEvent_t a{}, b{};
    hipStream_t st;
    Scope(csr_ctx *c_, const char *name, hipStream_t st_ = nullptr) : c(c_), st(st_ ? st_ : c_->stream) {
        if (name && c->profiling) {
            pe = &c->prof[name];
            a = get_event(c);
            b = get_event(c);
            (void)hipEventRecord(a, st);
        }
    }
    ~Scope() {
        if (pe) {
            (void)hipEventRecord(b, st);
            pe->pending.emplace_back(a, b);
            pe->launches++;
        }
    }
};
static void prof_collect(csr_ctx *c) {
    (void)hipStreamSynchronize(c->stream);
    if (c->side) (void)hipStreamSynchronize(c->side);
    if (c->tail) (void)hipStreamSynchronize(c->tail);
    for (auto &kv : c->prof) {
        for (auto &pr : kv.second.pending) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) kv.second.total_ms += ms;
            c->eventPool.push_back(pr.first);
            c->eventPool.push_back(pr.second);
        }
        kv.second.pending.clear();
    }
}
extern "C" int csr_profile_enable(csr_ctx *c, int32_t on) {
    if (!c) c = default_ctx();      // NULL addresses the default context of the host-buffer entry points
    if (!c) return -1;
    CHECK(ctx_select(c));
    prof_collect(c);
    c->prof.clear();
    c->profiling = on != 0;
    return 0;
}
extern "C" int csr_profile_read(csr_ctx *c, csr_kernel_time *out, int32_t capacity, int32_t *n_out) {
    if (!c) c = default_ctx();
    if (!c) return -1;
    CHECK(ctx_select(c));
    prof_collect(c);
    int32_t k = 0;
    for (auto &kv : c->prof) {
        if (k < capacity && out) {
            memset(&out[k], 0, sizeof(out[k]));
            strncpy(out[k].name, kv.first.c_str(), sizeof(out[k].name) - 1);
            out[k].launches = kv.second.launches;
            out[k].total_ms = kv.second.total_ms;
        }
        ++k;
    }
    if (n_out) *n_out = k;
    return 0;
}
extern "C" int csr_get_run_stats(csr_ctx *c, csr_run_stats *out) {
    if (!c || !out) return fail("null argument");
    *out = c->rs;
    out->blocks = c->NB;
    out->block_len = c->B;
    out->warm_p = c->warmP;
    out->warm_x = c->warmX;
    out->warm_b = c->warmB;
    out->x_tol_ulps = c->xTolUlps;
    out->local_repairs = c->hMail ? (int64_t)reinterpret_cast<const unsigned int *>(c->hMail.ptr)[MAIL_LOCAL] : 0;
    out->ws_warm_f = c->wsWarmF;
    out->ws_warm_b = c->wsWarmB;
    return 0;
}

// Every kernel launch of the host layer: profile scope `scope` on the launch's stream (nullptr: none), the launch, and its
// own error check under the kernel's name `what`.  A site that chooses among template instances computes the pointer (and
// the dynamic LDS that goes with it) first and launches once.
template <class... P, class... A>
static int launch(csr_ctx *c, const char *scope, const char *what, void (*kernel)(P...), dim3 grid, dim3 block, size_t lds,
                  hipStream_t st, A &&...args) {
    {
        Scope sc(c, scope, st);
        hipLaunchKernelGGL(kernel, grid, block, lds, st, std::forward<A>(args)...);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail("launch %s failed: %s", what, hipGetErrorString(e));
    return 0;
}

// The rest of the host library, split by concern (same translation unit, order matters: later parts use earlier ones)
#include "csr_host_batch.inl"
#include "csr_host_pipeline.inl"
#include "csr_host_single.inl"
#include "csr_host_rows.inl"
#include "csr_host_qseed.inl"
#include "csr_host_comm.inl"
#include "csr_host_rocco.inl"
#include "csr_host_dwb.inl"
#include "csr_host_null.inl"
#include "csr_host_segments.inl"
#include "csr_host_ess.inl"
#include "csr_host_peakscore.inl"
#include "csr_host_nested.inl"
#include "csr_host_export.inl"
#include "csr_host_cleanup.inl"
#include "csr_host_broad.inl"
#include "csr_host_depspan.inl"
#include "csr_host_shrink.inl"
#include "csr_host_munc.inl"
#include "csr_host_munc_track.inl"
