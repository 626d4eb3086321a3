/*
 * consenrich_amd.h -- C ABI of the MI355X (gfx950) implementation of Consenrich's estimator hot path.
 *
 * The reference has no FFI/plugin registry: its hot path sits behind the Python module-attribute interface
 * `consenrich.cconsenrich.<name>` (core.py:30, looked up at call time: core.py:3286-3290, 4231-4321, 4351-4413,
 * 3451, 3483).  This library is what a replacement of those callables binds to: every entry point below names the
 * reference callable it replaces ("pyx" = src/consenrich/cconsenrich.pyx).  Plain C: pointers + sizes, no torch,
 * no exceptions.  All functions return 0 on success, nonzero on failure; csr_last_error() gives the message
 * (thread-local).  Host buffers are caller-owned, C-contiguous, and never retained across calls; device buffers
 * are owned by the library (one context per GPU/process).
 *
 * Two API levels:
 *   (1) reference-shaped single-chain calls on HOST buffers  (csr_forward_pass, csr_backward_pass,
 *       csr_fixed_background_ecm, csr_expected_transition_residual_sums) -- drop-in for the Cython callables;
 *   (2) a device-resident multi-chain BATCH (csr_batch_*) -- many chromosomes/contigs per launch, inputs kept in
 *       HBM across sweeps; used by the genome driver, bench.py and the multi-GPU sharding (one context per rank).
 */
#ifndef CONSENRICH_AMD_H
#define CONSENRICH_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CSR_ABI_VERSION 6

/* ---- model / flags ------------------------------------------------------------------------------------- */

typedef struct csr_model {
    int32_t state_dim;          /* 2 = levelTrend (pyx:291-529), 1 = level (pyx:538-707) */
    int32_t reserved_;
    double F[4];                /* row-major transition matrix (float32 values widened; pyx:6566-6569) */
    double Q0[4];               /* row-major base process noise (pyx:6570-6573); level uses Q0[0] */
    double state_init;          /* (double)(float) stateInit        (pyx:6593) */
    double state_covar_init;    /* (double)(float) stateCovarInit   (pyx:6594) */
    double pad;                 /* (double)(float) pad              (pyx:6595) */
    double w_min, w_max;        /* observation precision (lambda) clamp, pyx:433 */
    double k_min, k_max;        /* process precision (kappa) clamp, pyx:395 */
    double apn_min_q, apn_max_q, apn_thresh, apn_scale, apn_pc; /* adaptive process noise, pyx:510-527 */
} csr_model;

enum {
    CSR_USE_LAMBDA   = 1u << 0, /* useLambda        (pyx:6449) */
    CSR_USE_KAPPA    = 1u << 1, /* useProcPrec      (pyx:6453) */
    CSR_USE_QSCALE   = 1u << 2, /* useProcessQScale (pyx:6452) */
    CSR_USE_APN      = 1u << 3, /* ECM_useAPN after the qDiagBase veto (pyx:6575); sequential fallback path */
    CSR_RETURN_NLL   = 1u << 4, /* returnNLL */
    CSR_NLL_IN_D     = 1u << 5  /* storeNLLInD */
};

/* ---- (1) reference-shaped single-chain entry points (host buffers) ---------------------------------------- */

typedef struct csr_fwd_io {
    int64_t m, n;               /* trackCount, intervalCount */
    const float *data;          /* (m,n) C-order  matrixData */
    const float *munc;          /* (m,n) C-order  matrixPluginMuncInit */
    const float *lambda;        /* n or NULL */
    const float *kappa;         /* n or NULL */
    const float *qscale;        /* n or NULL */
    uint32_t flags;             /* CSR_USE_* / CSR_RETURN_NLL / CSR_NLL_IN_D; USE_x requires the pointer */
    uint32_t reserved_;
    float *D;                   /* n, always written (vectorD) */
    float *xf;                  /* (n,d)   or NULL: all three or none (doStore, pyx:6444) */
    float *Pf;                  /* (n,d,d) */
    float *pnoise;              /* (n,d,d): rows 0..n-2 written (pyx:504-508) */
} csr_fwd_io;

typedef struct csr_fwd_out {
    double sum_d;               /* sum of float32 D[k]  -> phiHat = sum_d/n (pyx:6627) */
    double sum_nll;             /* sumNLL (pyx:468) */
} csr_fwd_out;

/* replaces cforwardPass (pyx:6393-6632) and cforwardPassLevel (pyx:6853-7049).  intervalToBlockMap is validated by
 * the host wrapper (its only effect in the reference is the range check pyx:389-392). */
int csr_forward_pass(const csr_model *mdl, const csr_fwd_io *io, csr_fwd_out *out);

/* replaces cbackwardPass (pyx:6635-6850) and cbackwardPassLevel (pyx:7052-7150).
 * lag_rows = rows available in `lag` (>= max(n-1,1)); resid is (n,m). */
int csr_backward_pass(const csr_model *mdl, int64_t m, int64_t n, const float *data,
                      const float *xf, const float *Pf, const float *pnoise,
                      float *xs, float *Ps, float *lag, int64_t lag_rows, float *resid);

typedef struct csr_ecm_cfg {
    int64_t max_iters;          /* ECM_fixedBackgroundIters */
    int64_t inner_iters;        /* t_innerIters */
    double rtol;                /* (double)(float) ECM_fixedBackgroundRtol */
    double nu;                  /* (double)(float) ECM_robustTNu */
    int32_t use_lambda;         /* ECM_useObsPrecisionReweighting */
    int32_t use_kappa;          /* ECM_useProcessPrecisionReweighting && (!APN || qscale)  (pyx:7912) */
    int32_t use_apn;
    int32_t reserved_;
} csr_ecm_cfg;

typedef struct csr_ecm_out {
    int64_t iters_done;
    double final_nll;
    double initial_nll;
    double abs_rel_change;
    double rel_improvement;
    int64_t stable_iters;
    int64_t nll_increase_count;
    int32_t converged;
    int32_t skipped;            /* n <= 5 filter+smoother fallback (pyx:7998-8129) */
    int32_t has_initial_nll;
    int32_t reserved_;
} csr_ecm_out;

/* replaces cfixedBackgroundECM (pyx:7660-8442) and cfixedBackgroundECMLevel (pyx:7153-7657).
 * lambda / kappa: n, in/out (warm start already clipped by the caller, pyx:7899-7923), NULL when disabled.
 * nll_path: max_iters doubles or NULL (per-iteration NLL, the reference's optimization_path). */
int csr_fixed_background_ecm(const csr_model *mdl, const csr_ecm_cfg *cfg, int64_t m, int64_t n,
                             const float *data, const float *munc, const float *qscale,
                             float *lambda, float *kappa,
                             float *xs, float *Ps, float *lag, float *resid,
                             double *nll_path, csr_ecm_out *out);

/* replaces cExpectedTransitionResidualSums (pyx:710-815) and ...Level (pyx:818-863); float64 host inputs. */
int csr_expected_transition_residual_sums(int32_t state_dim, int64_t n, const double *xs, const double *Ps,
                                          const double *lag, const double *F,
                                          double *sum_level, double *sum_trend, int64_t *count);

/* ---- (2) device-resident multi-chain batch ---------------------------------------------------------------- */

typedef struct csr_ctx csr_ctx;

int csr_device_count(void);
csr_ctx *csr_create(int device_ordinal);    /* NULL on failure */
void csr_destroy(csr_ctx *ctx);
const char *csr_last_error(void);
int csr_abi_version(void);
/* "abi <n> src <sha256 of the library's sources, 16 hex digits> <compiler flags>": lets a caller (bench.py, __graft_entry__)
 * record WHICH build ran -- a prebuilt library that travelled with the tree is distinguishable from a rebuild of newer sources. */
const char *csr_build_id(void);

/* Speculative-block tuning: block_len (multiple of 32; 0 = keep / choose from the batch size) and warm-up lengths in
 * BINS (rounded up to a multiple of 16; negative = keep) for the forward covariance chain, the forward state chain and
 * the backward chain.  Results never depend on these beyond the documented validation tolerance. */
int csr_set_tuning(csr_ctx *ctx, int32_t block_len, int32_t warm_p, int32_t warm_x, int32_t warm_b);

/* Carry validation of the forward STATE chain.  0 (the default of every context, and of the default context the
 * reference-shaped single-chain entry points use, ctx == NULL): a speculative block is accepted only if its carry-in is
 * bit-equal to its predecessor's carry-out, so results == the sequential recursion bit for bit, reproducible and independent
 * of block length / warm-up.  This is the only mode that holds the 1e-5 parity gate through the ECM loop on ill-conditioned
 * data: there the reference's own arithmetic moves by several times the gate when a few inputs move by one float32 ulp
 * (tests/test_hard_data.py).  k > 0 opts into the throughput mode: a carry is also accepted when
 * |dx0| <= k and |F01||dx1| <= k float32 ulps of max(|level|, 1) -- ~1e-7 relative on the state track PER PASS, ~3 x faster;
 * the contract is per pass, not through an ECM loop.  CONSENRICH_AMD_XTOL_ULPS overrides the default of both. */
int csr_set_validation(csr_ctx *ctx, int32_t x_tol_ulps);

/* Describe a batch: n_chains independent chains (chromosomes) of chain_len[c] bins, m samples each. (Re)allocates.
 * Any m > 0: device memory alone bounds it.  No kernel's LDS request grows with m beyond 64 KB (the residual kernels walk the
 * samples in slabs past m = 240 / 252, csrc/csr_resid_form.h); tested up to m = 631.  The one call with a ceiling of its own
 * is csr_batch_gain_summary: m <= 65535. */
int csr_batch_configure(csr_ctx *ctx, const csr_model *mdl, int64_t m, int32_t n_chains,
                        const int64_t *chain_len);
/* Replace the model parameters (same state_dim) without reallocating or re-uploading. */
int csr_batch_set_model(csr_ctx *ctx, const csr_model *mdl);
/* Per-chain base process noise: q = n_chains x 4 doubles (row-major Q0 per chain, float32 values widened) or NULL = the
 * model's Q0 for every chain.  The reference seeds Q0 per chromosome (core.py:5667, csr_batch_qseed); F and the other
 * model parameters stay batch-wide. */
int csr_batch_set_chain_q(csr_ctx *ctx, const double *q);
/* H2D one chain's (m,n_c) C-order matrices. */
int csr_batch_upload(csr_ctx *ctx, int32_t chain, const float *data, const float *munc);
/* H2D optional per-bin multipliers (any may be NULL = leave as is).  After csr_batch_configure all multipliers are 1. */
int csr_batch_upload_multipliers(csr_ctx *ctx, int32_t chain, const float *lambda, const float *kappa,
                                 const float *qscale);
/* Fill every chain with the SURVEY 8(d) synthetic recipe directly in HBM (counter-based RNG). */
int csr_batch_synthesize(csr_ctx *ctx, uint64_t seed);
/* D2H of one chain's resident inputs, (m, n) float32 each (either pointer may be NULL). */
int csr_batch_download_inputs(csr_ctx *ctx, int32_t chain, float *data, float *munc);

/* a1: per-bin sufficient statistics of (data, munc, pad); must precede forward/ECM after any upload. */
int csr_batch_stats(csr_ctx *ctx);
/* a2-a5 over all chains.  sum_d / sum_nll: n_chains doubles each (may be NULL). */
int csr_batch_forward(csr_ctx *ctx, uint32_t flags, double *sum_d, double *sum_nll);
/* a6-a7 over all chains (uses the forward results resident on the device). */
int csr_batch_backward(csr_ctx *ctx);
/* csr_batch_forward + csr_batch_backward as ONE pipeline (core.py:4207 `_runForwardBackward` calls the two back to back):
 * a single host synchronisation; the NIS/NLL epilogue runs on a side stream concurrently with the smoother chain. */
int csr_batch_forward_backward(csr_ctx *ctx, uint32_t flags, double *sum_d, double *sum_nll);
/* One pass of the hot path in one call: csr_batch_stats + csr_batch_forward_backward +
 * csr_batch_export(what) (what = 0: none) + csr_batch_sums (both pointers NULL: none, validation stays pending).
 * Same kernels and results as the separate calls.  Knowing `what` in advance lets the bit-exact mode (constant process
 * noise, >= 2 chains) start the smoother / residuals of every chain as soon as THAT chain's filtered state stands, while the
 * state chain of slower chains is still running (csr_run_stats.tail_groups counts the groups). */
int csr_batch_step(csr_ctx *ctx, uint32_t flags, uint32_t what, double *sum_d, double *sum_nll);
/* A TEST SEAM, off unless set: which chains of such a step go out together.  By default the host groups the chains as they become
 * final (by its clock); with a script the grouping is the same whatever the timing -- only whether a group overlaps the running
 * state chain still depends on it.  tail_group / epilogue_group: n_chains entries each, the index of the chain's early group
 * (tails: below 6; NIS / NLL epilogues: below 8; the indices in use are 0..k-1 without a hole) or -1 = the remainder, which follows
 * the scripted groups.  A NULL array leaves that kind unscripted; both NULL clear the script.  The script belongs to the batch
 * (csr_batch_configure drops it) and holds for every later step; a step that does not pipeline its tail ignores it.  Results do
 * not depend on it.  A wrong n_chains or a bad index returns CSR_ERR_VALUE (csr_last_error says which) and changes nothing. */
int csr_batch_set_step_groups(csr_ctx *ctx, const int32_t *tail_group, const int32_t *epilogue_group, int32_t n_chains);
/* The FORWARD FILTER ALONE in one call (cforwardPass without cbackwardPass, pyx:6393-6632 -- BASELINE config 2): csr_batch_stats +
 * csr_batch_forward + csr_batch_export(what & CSR_EXPORT_FORWARD) + csr_batch_sums.  Same kernels and results as the separate
 * calls; no smoother, no residuals. */
int csr_batch_step_forward(csr_ctx *ctx, uint32_t flags, uint32_t what, double *sum_d, double *sum_nll);
/* Per-chain sumD / sumNLL of the resident forward pass (n_chains doubles each, either may be NULL).  Lets a caller
 * queue csr_batch_export behind csr_batch_forward_backward(…, NULL, NULL) and synchronise once, here. */
int csr_batch_sums(csr_ctx *ctx, double *sum_d, double *sum_nll);
/* a8-a9 over all chains in lock-step; out: n_chains entries; nll_path: n_chains*max_iters or NULL. */
int csr_batch_ecm(csr_ctx *ctx, const csr_ecm_cfg *cfg, uint32_t flags, csr_ecm_out *out, double *nll_path);
/* Same, restricted to the chains with chain_mask[c] != 0 (NULL: all); the others keep the resident results of their last
 * fit untouched (out[c].skipped = 2) -- chromosomes of a batch stop their outer background/ECM alternation independently.
 * (Every array csr_batch_export hands out, the process-noise rows of a constant-Q fit included, and the per-chain sums.) */
int csr_batch_ecm_masked(csr_ctx *ctx, const csr_ecm_cfg *cfg, uint32_t flags, const unsigned char *chain_mask,
                         csr_ecm_out *out, double *nll_path);

enum { /* arrays, reference (natural) layout */
    CSR_ARR_D = 0,      /* (n)      float32 */
    CSR_ARR_XF,         /* (n,d)    */
    CSR_ARR_PF,         /* (n,d,d)  */
    CSR_ARR_PNOISE,     /* (n,d,d), rows 0..n-2 valid */
    CSR_ARR_XS,         /* (n,d)    */
    CSR_ARR_PS,         /* (n,d,d)  */
    CSR_ARR_LAG,        /* (n,d,d), rows 0..n-2 valid */
    CSR_ARR_RESID,      /* (n,m)    */
    CSR_ARR_LAMBDA,     /* (n)      */
    CSR_ARR_KAPPA,      /* (n)      */
    CSR_ARR_QSCALE,     /* (n)      process-noise scale (exported with CSR_EXPORT_MULT) */
    CSR_ARR_SUMGAIN0,   /* (n)      diagnostics, see csr_batch_diagnostics */
    CSR_ARR_SUMGAIN1,   /* (n)      */
    CSR_ARR_EFFQ_LEVEL, /* (n)      */
    CSR_ARR_EFFQ_TREND, /* (n)      */
    CSR_ARR_MUNCTRACE,  /* (n)      */
    CSR_ARR_BACKGROUND,       /* (n) current background (subtracted from the data), see csr_batch_background_* */
    CSR_ARR_BACKGROUND_NEXT,  /* (n) proposal of the last csr_batch_background_update */
    CSR_ARR_COUNT
};
enum {
    CSR_EXPORT_FORWARD = 1u << 0,   /* D, xf, Pf, pnoise */
    CSR_EXPORT_SMOOTH  = 1u << 1,   /* xs, Ps, lag */
    CSR_EXPORT_RESID   = 1u << 2,   /* resid */
    CSR_EXPORT_MULT    = 1u << 3    /* lambda, kappa, qscale */
};
/* Convert device-internal (block-transposed) results into reference-layout device arrays. */
int csr_batch_export(csr_ctx *ctx, uint32_t what);
/* D2H one exported array of one chain. */
int csr_batch_download(csr_ctx *ctx, int32_t chain, int32_t array_id, void *host_dst);
/* Device pointer + element count of an exported array (all chains, chain c at csr_batch_chain_offset). */
int csr_batch_device_array(csr_ctx *ctx, int32_t array_id, void **dev_ptr, int64_t *n_elems);
int64_t csr_batch_chain_offset(csr_ctx *ctx, int32_t chain);   /* in bins, -1 on error */
int csr_synchronize(csr_ctx *ctx);

/* Instrumentation: kernel timing with HIP events on the library's stream. */
typedef struct csr_kernel_time {
    char name[48];
    int64_t launches;
    double total_ms;
} csr_kernel_time;
int csr_profile_enable(csr_ctx *ctx, int32_t on);          /* also clears accumulated times */
int csr_profile_read(csr_ctx *ctx, csr_kernel_time *out, int32_t capacity, int32_t *n_out);

/* ---- per-interval output diagnostics (core.py:7734-7878 `_perIntervalOutputDiagnosticTracks`,
 * a per-bin Python loop in the reference) ---------------------------------------------------------------------------
 * From the resident forward pass of every chain: sumGain0/1 (total Kalman gain on level / trend, re-derived from the
 * STORED float32 filtered covariance of the previous bin exactly as the reference does), effectiveQLevel/Trend and
 * muncTrace = sum_j max(v_j+pad,1e-12)/lambda.  flags: CSR_USE_LAMBDA / CSR_USE_KAPPA / CSR_USE_QSCALE select the
 * resident multipliers (absent = None in the reference call); without CSR_USE_KAPPA the forward pass's own pNoise is
 * the effective process noise (core.py:7826-7848).  Results: CSR_ARR_SUMGAIN0.. arrays (download / device_array).
 * The five remaining reference tracks (baseQ*, preKappaQ*, processQScale) are O(1)-per-bin functions of Q0 and qScale
 * and are formed by the host mirror. */
int csr_batch_diagnostics(csr_ctx *ctx, uint32_t flags);
/* Same on host buffers, shaped like the reference call (drop-in for core._perIntervalOutputDiagnosticTracks):
 * Pf (n,d,d), munc (m,n); lambda / kappa / qscale / pnoise may be NULL (pnoise: (>=n-1,d,d)); outputs (n) float32. */
int csr_output_diagnostics(const csr_model *mdl, int64_t m, int64_t n, const float *Pf, const float *munc,
                           const float *lambda, const float *kappa, const float *qscale, const float *pnoise,
                           float *sum_gain0, float *sum_gain1, float *effq_level, float *effq_trend,
                           float *munc_trace);

/* ---- natives of the background update between ECM phases ------------------------------------
 * csr_solve_background replaces cconsenrich.csolveZeroCenteredBackground (pyx:944-1096) for a BATCH of independent
 * chains: solves (diag(w) + lam_first D1'D1 + lam D2'D2) x = rhs per chain (pentadiagonal SPD, fp64), optionally with
 * the zero-sum Lagrange correction.  weight / rhs / out: the chains' vectors concatenated (chain c has n[c] entries).
 * The reference's sequential LDL' is replaced by an exact two-level partition (see csrc/csr_background.h);
 * block_len = 0 picks the default partition size.  bad_index[c] (chain-local) / bad_value[c]: first pivot that had to be
 * raised to the 1e-12 floor, or -1 -- the reference raises RuntimeError in that case; `out` is filled regardless. */
int csr_solve_background(int32_t n_chains, const int64_t *n, const double *weight, const double *rhs, double lam,
                         double lam_first, int32_t zero_center, int32_t block_len, double *out, int64_t *bad_index,
                         double *bad_value);
/* cconsenrich.cbackgroundWeightedStatsWithSupport (pyx:9700-9724): weight[i] = sum_j inv_var[j,i],
 * rhs[i] = sum_j inv_var[j,i]*resid[j,i] in fp64 over float32 (m,n) C-order matrices; *support = #{weight > 0}. */
int csr_background_weighted_stats(int64_t m, int64_t n, const float *resid, const float *inv_var, double *weight,
                                  double *rhs, int64_t *support);

/* Device-resident background update for a whole batch (core.py:5064-5137 + 8085-8378): weight / rhs tracks from the
 * resident ORIGINAL data, munc, smoothed level (and lambda), conditioning guard, the pentadiagonal solve and the
 * asymmetric-IRLS wrapper (<= max_passes re-solves with the negative-part penalty), all chains in lock-step.  Nothing
 * crosses PCIe but a few scalars per chain.  The proposal lands in CSR_ARR_BACKGROUND_NEXT; csr_batch_background_apply
 * makes it the current background, which csr_batch_stats / the residuals then subtract from the data in float32 exactly
 * like the reference's `dataAdjusted` (core.py:3253). */
typedef struct csr_bg_cfg {
    double lam_first, lam;              /* core.py:7478-7491 `_backgroundPenaltyWeightsFromSpan` */
    double negative_penalty_multiplier; /* fitParams.backgroundNegativePenaltyMultiplier; <= 0 / non-finite: plain solve */
    int32_t zero_center;                /* fitParams.ECM_zeroCenterBackground */
    int32_t use_nonnegative;            /* fitParams.useNonnegativeBackground */
    int32_t use_lambda;                 /* multiply 1/max(munc+pad,1e-8) by clip(lambda) (core.py:5065-5074) */
    int32_t use_initial;                /* bit 0 (CSR_BG_INIT_FROM_CURRENT): seed the first solve with the current background's
                                           negative mask (initialBackground, core.py:8306-8316); bit 1 (CSR_BG_ZERO_STATE):
                                           the smoothed level is taken as zero -- the background warm start from the weighted
                                           data, core.py:2809-2910 `_estimateBackgroundWarmStart` (no fit needs to be resident) */
    int32_t max_passes;                 /* reference: 5 */
    int32_t block_len;                  /* partition size of the solver, 0 = default */
} csr_bg_cfg;
enum { CSR_BG_INIT_FROM_CURRENT = 1, CSR_BG_ZERO_STATE = 2,
       CSR_BG_SEED_WEIGHTS = 4 /* the seed loop's per-cell weights: set by csr_batch_munc_seed_background only */ };
enum { CSR_BG_OK = 0, CSR_BG_NO_SUPPORT = 1, CSR_BG_BAD_PIVOT = 2, CSR_BG_UNRELIABLE = 3, CSR_BG_NONFINITE = 4 };
typedef struct csr_bg_out {
    int64_t support;                    /* bins with positive weight */
    double weight_sum, weight_scale;    /* sum of weights; median of the positive weights (IRLS penalty scale) */
    double roundoff_index;              /* eps * (1 + (4 lam_first + 16 lam) / mean positive weight), core.py:8160-8187 */
    double shift_rms;                   /* sqrt(sum w (next - current)^2 / sum w), core.py:5199-5215 */
    double proposal_rms, reference_rms; /* same weighting of next / current (core.py:5216-5240: shift tolerance scale) */
    int64_t bad_index;                  /* first modified pivot (CSR_BG_BAD_PIVOT) */
    double bad_value;
    int32_t passes;                     /* IRLS re-solves performed */
    int32_t status;                     /* CSR_BG_*: the reference raises for 2, 3, 4 and returns zeros for 1 */
} csr_bg_out;
int csr_batch_background_update(csr_ctx *ctx, const csr_bg_cfg *cfg, csr_bg_out *out /* n_chains */);
/* current background := last proposal for the chains with take[c] != 0 (NULL: all).  Invalidates the statistics. */
int csr_batch_background_apply(csr_ctx *ctx, const unsigned char *take);
/* H2D a background track for one chain (NULL: zeros). */
int csr_batch_set_background(csr_ctx *ctx, int32_t chain, const float *background);

/* ---- terms of the penalised objective of the outer stop rule (core.py:4418-4538) ---------------------------
 * For every chain, from the resident variances, multipliers and CURRENT background: robust precision penalties
 * 0.5 nu sum(x - log x) (core.py:3161-3179; kappa skips the first bin), roughness penalties 0.5 lam sum d^2
 * (core.py:3182-3204), negative-part penalty 0.5 mult median(positive weights) sum min(bg,0)^2 (core.py:4431-4463; float64
 * weight track sum_j clip(lambda)/max(munc+pad,1e-8)), effective observation count (core.py:2981-2986).  The caller adds
 * the forward NLL of (data - background) (csr_batch_stats + csr_batch_forward_masked) and divides by the count. */
typedef struct csr_objective_cfg {
    double nu, lam_first, lam, negative_penalty_multiplier, pad;
    int32_t use_lambda_penalty, use_kappa_penalty, use_lambda_weights, use_nonnegative;
} csr_objective_cfg;
typedef struct csr_objective_terms {
    double robust_observation_penalty, robust_process_penalty, first_difference_penalty, second_difference_penalty,
        negative_penalty, weight_median;
    int64_t effective_observation_count;
} csr_objective_terms;
int csr_batch_objective_terms(csr_ctx *ctx, const csr_objective_cfg *cfg, csr_objective_terms *out);
/* The two per-phase diagnostics of `runConsenrich` that read the (m, n) matrices, as per-bin float64 tracks of ONE chain from
 * the resident data / variances, the smoothed level of the last ECM phase and the CURRENT background:
 *   rel[i]  = level_i - sum_j (data_ji - bg_i) w_ji / sum_j w_ji with w_ji = 1 / max(munc_ji + pad, 1e-12), summed row by row in
 *             float64 over the cells with finite data and finite positive munc_ji + pad, NaN where there is none: the track whose
 *             sign changes per kb `_relativeSignChangePerKB` counts (core.py:2647-2700; called at core.py:4980, 5485);
 *   fit[i]  = sum_j iv_ji (r_ji - g_i)^2, cnt[i] = #cells with finite r and finite positive iv (both NULL: skipped), with the
 *             matrices of the background update (float32 iv = 1 / max(munc + pad, 1e-8) (* clip(lambda) if use_lambda), float32
 *             r = data - level, model pad; core.py:5064-5076) and g = the PROPOSAL of the last csr_batch_background_update:
 *             0.5 sum(fit) is `background_weighted_residual_objective`, sum(cnt) the effective observation count of
 *             `_scoreBackgroundFitObjective` (core.py:4540-4606; called at core.py:5161).
 * rel / fit: n doubles, cnt: n int32 (host).  The caller's part is O(n). */
int csr_batch_phase_tracks(csr_ctx *ctx, int32_t chain, int32_t use_lambda, double pad, double *rel, double *fit, int32_t *cnt);
/* The final forward gain summary of `runConsenrich`'s run diagnostics (`_finalForwardReplicateGainContigSummary`,
 * core.py:7671-7731) for one chain, from the resident forward pass: per replicate j the gains
 * g_k = max(Pf00_k, 0) * clip(lambda_k, lam_lo, lam_hi) / max(munc_jk + pad, 1e-12) in float64 (lambda = 1 unless use_lambda) and, over
 * the FINITE ones, out[j*9 + ...] = {count, mean, standard deviation (np.std), then the six order statistics x[lo], x[hi] around
 * the positions (count - 1) q of q = 0.25, 0.5, 0.75 (NumPy's 'linear' method interpolates between exactly these)}.  The
 * reference sorts m rows of n float64 values on the host; here a byte-wise radix select on the device (csrc/csr_gain.h), exact.
 * out: m * 9 doubles.  (ABI 6) */
int csr_batch_gain_summary(csr_ctx *ctx, int32_t chain, int32_t use_lambda, double pad, double lam_lo, double lam_hi, double *out);
/* csr_batch_forward for the chains with chain_mask[c] != 0 only (NULL: all); the others keep their resident results: the
 * NIS / NLL track, the filtered state and covariance, the process-noise rows and the per-chain sums.  (Whether the
 * process noise is one constant matrix is one property of the whole batch, taken from the LAST pass's flags: a masked pass that
 * turns kappa / qScale / adaptive process noise ON keeps the constant rows of the other chains; one that turns them OFF after
 * a resident pass that had them on makes the other chains' rows read as the constant matrix -- not supported.) */
int csr_batch_forward_masked(csr_ctx *ctx, uint32_t flags, const unsigned char *chain_mask, double *sum_d,
                             double *sum_nll);

/* ---- track writer ------------------------------------------------------------------------------
 * bedGraph text of one track, byte for byte what the reference emits (consenrich.py:9797-9805: pandas to_csv with
 * sep="\t", header=False, index=False, float_format="%.4f", lineterminator="\n"; NaN -> empty field, +-inf -> inf/-inf).
 * Rows: chrom \t start \t end \t value \n.  Intervals: starts/ends (n int64 each) or, if NULL, start0 + k*step with
 * end = min(start + step, end_cap) (end_cap <= 0: no cap).  transform: CSR_BGW_NONE, CSR_BGW_ROUND4 (np.round(x, 4) in
 * float32 = core.getPrimaryState, core.py:6145-6166) or CSR_BGW_SQRT (uncertainty = sqrt(P00), consenrich.py:9476).
 * Returns the number of bytes of the text; writes it to `out` if out != NULL and out_capacity is large enough (call
 * once with out = NULL to size the buffer).  Negative on error. */
enum { CSR_BGW_NONE = 0, CSR_BGW_ROUND4 = 1, CSR_BGW_SQRT = 2 };
int64_t csr_format_bedgraph(const char *chrom, int64_t n, const int64_t *starts, const int64_t *ends, int64_t start0,
                            int64_t step, int64_t end_cap, const float *values, int32_t transform, char *out,
                            int64_t out_capacity);
/* Same for component `comp` of an exported array of one chain of a batch (values never leave the device as floats). */
int64_t csr_batch_format_bedgraph(csr_ctx *ctx, int32_t chain, int32_t array_id, int32_t comp, int32_t transform,
                                  const char *chrom, int64_t start0, int64_t step, int64_t end_cap, char *out,
                                  int64_t out_capacity);

/* bigWig (io.py:530 `convertBedGraphToBigWig`, io.py:633-760 `_convertBedGraphToBigWigPyBigWig`: the reference converts its
 * bedGraph files with pyBigWig).  The fixed-record body of a bigWig file (Kent et al. 2010, BigWig/BigBed file format) for one
 * track of one chain, formatted on the device from the exported array like csr_batch_format_bedgraph:
 *   csr_batch_bigwig_sections  the UNCOMPRESSED data sections, back to back: 24-byte header (chromId, chromStart, chromEnd,
 *                              itemStep 0, itemSpan 0, type 1 = bedGraph, reserved, itemCount) + 12-byte items (start, end,
 *                              float32 value), items_per_section items each (the last one fewer), + the total summary;
 *   csr_batch_bigwig_zoom      reduction records of bins_per_record consecutive intervals (32 bytes: chromId, start, end,
 *                              validCount, min, max, sum, sumSquares as float32) for one zoom level.
 * An item's value is what the reference's file holds: float32 of the decimal text "%.4f" of the (transformed) track value --
 * pyBigWig receives the values parsed back from the bedGraph rows.  Both return the byte count (call with out = NULL to size
 * the buffer), negative on error.  Chromosome tree, R-tree index, zlib of the blocks and the headers are O(sections) host
 * work (consenrich_amd/writers.py). */
typedef struct csr_bw_summary {
    int64_t bases_covered, non_finite;      /* non_finite: items whose value is NaN / inf (the reference refuses such rows) */
    double min_val, max_val, sum_data, sum_squares;
} csr_bw_summary;
int64_t csr_batch_bigwig_sections(csr_ctx *ctx, int32_t chain, int32_t array_id, int32_t comp, int32_t transform,
                                  uint32_t chrom_id, int64_t start0, int64_t step, int64_t end_cap, int32_t items_per_section,
                                  unsigned char *out, int64_t out_capacity, csr_bw_summary *total);
int64_t csr_batch_bigwig_zoom(csr_ctx *ctx, int32_t chain, int32_t array_id, int32_t comp, int32_t transform,
                              uint32_t chrom_id, int64_t start0, int64_t step, int64_t end_cap, int64_t bins_per_record,
                              unsigned char *out, int64_t out_capacity);

/* ---- natives of the delete-block uncertainty calibration (cuncertainty.pyx) -------------------
 * csr_observation_total_information = cobservationTotalInformation (pyx:97-157); csr_fold_mask_and_information =
 * cmakeFoldMaskAndInformation (pyx:160-305) after its argument validation.  munc is float32 (munc_is_f64 = 0) or float64,
 * (m,n) C-order; active (m,n) uint8; lambda NULL = useLambda False; reps (block_count, slots) int64; nominal may be NULL.
 * Same summation orders as the reference, IEEE division / sqrt: the tracks are bit-identical. */
int csr_observation_total_information(int64_t m, int64_t n, const void *munc, int32_t munc_is_f64, const uint8_t *active,
                                      const double *lambda, double pad, double rho, double *total);
int csr_fold_mask_and_information(int64_t m, int64_t n, int64_t block_len, int64_t fold, const int32_t *block_fold,
                                  const int64_t *reps_count, const int64_t *reps, int64_t slots, const void *munc,
                                  int32_t munc_is_f64, const uint8_t *active, const double *total, const double *lambda,
                                  double pad, double rho, uint8_t *mask, double *kept, double *heldout, double *h,
                                  double *nominal);
/* A fold as an extra chain of a batch (uncertainty.py:1370-1419 runs one fit per fold): chain `dst` (same length as
 * `src`) receives src's data and src's variances with the fold's deleted cells set to masked_variance (the reference:
 * 1e30, constants.py:387); kept / heldout / h (n doubles each, host) as above with every cell active, total computed on
 * the fly.  Nothing but the fold spec and the three tracks crosses PCIe. */
int csr_batch_make_fold(csr_ctx *ctx, int32_t src, int32_t dst, int64_t block_len, int64_t fold, const int32_t *block_fold,
                        const int64_t *reps_count, const int64_t *reps, int64_t slots, int32_t use_lambda, double pad,
                        double rho, float masked_variance, double *kept, double *heldout, double *h);

/* ---- the initial process-noise (Q0) seed ---------------------------------------------------------
 * csr_qseed_same_track = cEstimateSameTrackProcessNoiseTransitions (cconsenrich.pyx:1441-1797), csr_qseed_pooled =
 * cEstimatePooledProcessNoiseTransitions (pyx:1800-1902), csr_qseed_posterior = cQSeedPosteriorFromTransitions
 * (pyx:1905-2146), all after the Python-level argument validation.  Matrices are (m,n) C-order float64 + uint8 mask, as
 * the reference's natives take them; outputs need capacity min(n-1, max_transition_samples > 0 ? that : n-1) (same
 * track) or n-1 (pooled).  Data-dependent errors return nonzero with the reference's message in csr_last_error().
 * The sampled columns are gathered and reduced on the device; the bounded tail (two quantiles of <= precision_sample_cap
 * precisions, the stable ordering of <= 32 000 signal levels, the 64-point grid posterior over <= 2048 transitions) is
 * host arithmetic inside the library, in the reference's operation order (bit-identical transitions). */
typedef struct csr_qseed_sample_cfg {
    double precision_cap_quantile, precision_cap_multiplier;   /* core.py:277-278: 0.95, 20 */
    int64_t max_transition_samples, precision_sample_cap, signal_panel_size;   /* core.py:273-276: 32000, 32000, 2048 */
} csr_qseed_sample_cfg;
typedef struct csr_qseed_sample_diag {
    int64_t pair_count, sampled_pair_count, precision_sample_count, scan_count, candidate_count, selected_count;
    int32_t capped_mode, reserved;
    double precision_cap, precision_cap_fraction, transition_sample_fraction;
} csr_qseed_sample_diag;
typedef struct csr_qseed_post_cfg {
    double q_floor, q_cap /* may be +inf */, robust_t_nu, q_seed_prior_level;
    int64_t min_transitions;        /* core.py:272: 8 */
    double prior_log_sd, default_t_nu;   /* core.py:279-280: log 4, 8 */
    int64_t grid_size;              /* core.py:275: 64 */
} csr_qseed_post_cfg;
typedef struct csr_qseed_post {
    int64_t transition_count;
    int32_t ok, reserved;
    double effective_transition_count, median_sampling_variance, prior_level, posterior_mode, posterior_median,
        posterior_q05, posterior_q95, transition_q90;
} csr_qseed_post;
int csr_qseed_same_track(int64_t m, int64_t n, const double *data, const double *obs_var, const uint8_t *active,
                         const csr_qseed_sample_cfg *cfg, double *deltas, double *sampling_var, double *weights,
                         int64_t *out_count, csr_qseed_sample_diag *diag);
int csr_qseed_pooled(int64_t m, int64_t n, const double *data, const double *obs_var, const uint8_t *active,
                     double *deltas, double *sampling_var, double *weights, int64_t *out_count);
int csr_qseed_posterior(int64_t count, const double *deltas, const double *sampling_var, const double *weights,
                        const csr_qseed_post_cfg *cfg, csr_qseed_post *out);
/* The caller `_estimateInitialProcessNoiseFromData` (core.py:3621-3780) for every chain of a batch, on the resident
 * float32 data / variance matrices (nothing is converted or masked on the host; only the sampled columns are read):
 * same-track estimate -> pooled fallback -> median-observation-variance fallback -> clamps.  out: n_chains records.
 * source: 0 sameTrackEB, 1 pooledEB, 2 observationVarianceFloor, 3 minQ; reason: 0 ok, 1 fallback_observation_variance,
 * 2 fallback_min_q, 3 insufficient_transition_support (never final).  state_dim 2 = levelTrend, 1 = level. */
typedef struct csr_qseed_cfg {
    csr_qseed_sample_cfg sample;
    double pad, min_q, max_q /* < 0 or non-finite: no cap */, delta_f, robust_t_nu /* NaN: default */, q_seed_prior_level;
    int64_t min_transitions;
    double prior_log_sd, default_t_nu;
    int64_t grid_size;
    int32_t state_dim, reserved;
} csr_qseed_cfg;
typedef struct csr_qseed_out {
    double q_level, q_trend;                 /* diagonal of matrixQ before its float32 cast (qSeedLevelFinal / TrendFinal) */
    double level_pre_clamp, trend_pre_clamp;
    int32_t source, reason;
    csr_qseed_sample_diag sample;            /* of the same-track scan */
    csr_qseed_post post;                     /* of the estimate that was used (ok = 0: none was) */
} csr_qseed_out;
int csr_batch_qseed(csr_ctx *ctx, const csr_qseed_cfg *cfg, csr_qseed_out *out);

/* ---- the one collective of the path -- final track gather over RCCL / xGMI ----------------------------------
 * The reference fits chromosomes in a sequential loop of one process (consenrich.py:8809) and has no communication at all;
 * here contigs are sharded over the GPUs of a node (one process and one csr_ctx per GPU, no data-path collective) and the
 * per-bin output tracks are gathered ONCE at the end.  RCCL is bound at run time (dlopen librccl.so.1): only these entry
 * points need it.  No PyTorch: rank 0 creates the 128-byte unique id, the caller's launcher distributes it (bench.py: a file
 * on the node), every rank creates its communicator on its context's device. */
typedef struct csr_comm csr_comm;
int csr_comm_unique_id(char *id128);                       /* ncclGetUniqueId; 128 bytes */
csr_comm *csr_comm_create(csr_ctx *ctx, const char *id128, int32_t world, int32_t rank);     /* NULL on failure */
void csr_comm_destroy(csr_comm *comm);
int csr_comm_world(csr_comm *comm);
int csr_comm_rank(csr_comm *comm);
/* *value := max over ranks (ncclAllReduce on the library's stream + stream synchronisation: also a barrier that completes
 * only when every rank's queue is drained). */
int csr_comm_allreduce_max(csr_comm *comm, double *value);
/* *value := sum over ranks: an all-reduce of 1.0 tells the caller how many ranks the communicator really spans. */
int csr_comm_allreduce_sum(csr_comm *comm, double *value);
int csr_comm_barrier(csr_comm *comm);
/* (smoothed level xs[:,0], its variance Ps[:,0,0]) of every bin of the rank's chains, packed chain after chain on the device
 * straight from the exported arrays (CSR_EXPORT_SMOOTH; no host bounce), then ncclAllGather: every rank ends with
 * world x cap_bins (level, variance) pairs; rank r's chains start at pair r * cap_bins.  cap_bins = max over ranks of the
 * rank's total bins (same value on every rank).  host_out: world * cap_bins * 2 floats, or NULL.  Fails when the exported
 * arrays are not those of the resident fit (a pass ran since the last CSR_EXPORT_SMOOTH). */
int csr_batch_gather_tracks(csr_ctx *ctx, csr_comm *comm, int64_t cap_bins, float *host_out);

/* ---- budgeted chain peak selection (ROCCO): pyx:8603-8958 `csolvePenalizedChainROCCO`, `ccalibrateSelectionPenaltyROCCO`,
 * `csolveChromROCCOExact`; pyx:9427-9457 `cBooleanRunBounds`; peaks.py:342-393 `consenrichStateScoreTrack` --------------------
 * Every value returned is the reference's bit for bit: the uint8 mask, the count, both objectives and the penalty the
 * count-driven bisection ends on.  One lane runs the reference's sequential recursion per (chain, penalty) pair; the chains of
 * a call and the 2^D - 1 midpoints the next D bisection steps can visit run side by side (D = the speculation depth, which
 * changes speed only).  Additive to ABI 6: new functions and structs, no change to existing ones. */
enum { CSR_ROCCO_FIXED_PENALTY = 0, CSR_ROCCO_TARGET_COUNT = 1 };
enum { CSR_ROCCO_SCORE_STATE = 0, CSR_ROCCO_SCORE_LOWER_CONFIDENCE = 1 };
/* return code of every peak-stage call: an argument or input the reference answers with ValueError (message: csr_last_error).  The
 * stages' own names below are the same value. */
enum { CSR_ERR_VALUE = 2 };
enum { CSR_ROCCO_ERR_VALUE = CSR_ERR_VALUE };
typedef struct csr_rocco_cfg {
    int32_t mode;               /* CSR_ROCCO_FIXED_PENALTY: one solve at `penalty`; CSR_ROCCO_TARGET_COUNT: calibrate (pyx:8773-8844) */
    int32_t max_iter;           /* bisection steps; max(max_iter, 1) are made */
    double penalty;
    int64_t target_count;       /* clamped to [0, n]; n = one solve at penalty 0 */
    double gamma;               /* constant switch cost of the chain (ignored where a cost array is given) */
} csr_rocco_cfg;
typedef struct csr_rocco_out {
    double selection_penalty, penalized_objective, objective;
    int64_t selected_count;
} csr_rocco_out;
typedef struct csr_rocco_stats {    /* cumulative per context */
    int64_t rounds;             /* host round trips of the calibration loop */
    int64_t launches;           /* kernel launches */
    int64_t lane_steps;         /* sum over lanes of the bins they walked */
    int64_t h2d_bytes, d2h_bytes;
    int32_t depth, reserved;
} csr_rocco_stats;
/* Chains on host arrays (default context).  scores: the chains' float64 scores one after the other (sum of chain_len values);
 * switch_costs: their n - 1 costs one after the other, or NULL = every chain's cfg.gamma; cfg / out: one record per chain;
 * solution: the chains' masks one after the other (may be NULL). */
int csr_rocco_solve(int32_t n_chains, const int64_t *chain_len, const double *scores, const double *switch_costs,
                    const csr_rocco_cfg *cfg, csr_rocco_out *out, uint8_t *solution);
/* The same on a batch context.  Scores are a float64 track per chain in buffers of their own (freed with the batch): uploaded
 * chain by chain, or built for every chain from the resident smoothed fit -- CSR_ROCCO_SCORE_STATE: (double) xs[:,0];
 * CSR_ROCCO_SCORE_LOWER_CONFIDENCE: (double) xs0 - z * (double)(float) sqrt(Ps00), floored at -2 max(xs0) when that maximum is
 * finite and positive; a negative variance or a bad z returns CSR_ROCCO_ERR_VALUE.  None of these calls changes the values of
 * a resident array of the fit or the record of its last pass; csr_batch_rocco_scores reads the reference-layout copies of xs / Ps
 * and, where those are not current, first makes them exactly as csr_batch_export with CSR_EXPORT_SMOOTH would (the only side effect:
 * the arrays count as exported afterwards). */
int csr_batch_upload_scores(csr_ctx *ctx, int32_t chain, const double *scores);
int csr_batch_rocco_scores(csr_ctx *ctx, int32_t mode, double z);
int csr_batch_download_scores(csr_ctx *ctx, int32_t chain, double *host_dst);
/* cfg / out: n_chains records; chain_mask (n_chains bytes or NULL = all): chains with 0 are not solved and keep their mask. */
int csr_batch_rocco(csr_ctx *ctx, const csr_rocco_cfg *cfg, const unsigned char *chain_mask, csr_rocco_out *out);
int csr_batch_rocco_download(csr_ctx *ctx, int32_t chain, uint8_t *solution);
/* `cBooleanRunBounds` of a chain's mask on the device (flag, scan, compaction): *count = number of runs; the first `capacity`
 * of them go to starts / ends (inclusive bin indices; both may be NULL with capacity 0). */
int csr_batch_rocco_runs(csr_ctx *ctx, int32_t chain, int32_t max_gap_bins, int64_t capacity, int64_t *count,
                         int64_t *starts, int64_t *ends);
/* Speculation depth D of the calibration (1..8, 0 = default 6); ctx NULL = the default context. */
int csr_set_rocco_depth(csr_ctx *ctx, int32_t depth);
int csr_get_rocco_stats(csr_ctx *ctx, csr_rocco_stats *out);

/* ---- stationary-null dependent wild bootstrap (DWB) behind the ROCCO budgets: pyx:9283-9424 `cGenerateDWBMultipliersFromNoise`,
 * `cApplyStationaryNullDWB`, `cStationaryNullDWBDraw`; the two bootstrap loops of peaks.py:593-762 ------------------------------
 * Every value equals the reference's bit for bit.  An argument the reference answers with ValueError returns CSR_DWB_ERR_VALUE
 * with the reference's message in csr_last_error; such checks run before any launch.  `kernel`: bartlett / triangle / triangular,
 * parzen, qs / quadratic_spectral (case, surrounding blanks and '-' for '_' do not matter).  A bandwidth below 2 counts as 2;
 * maxLag = bandwidth, or max(8 bandwidth, 32) for qs, at most 512. */
enum { CSR_DWB_ERR_VALUE = CSR_ERR_VALUE };
int csr_dwb_max_lag(int32_t bandwidth, const char *kernel, int32_t *max_lag);
/* The natives on host arrays (default context).  out: noise_len - 2 maxLag multipliers / n values. */
int csr_dwb_multipliers(const double *noise, int64_t noise_len, int32_t bandwidth, const char *kernel, double *out);
int csr_dwb_apply(const double *tmpl, int64_t n, const double *multipliers, int64_t n_multipliers, double *out);
int csr_dwb_draw(const double *tmpl, int64_t n, int32_t bandwidth, const char *kernel, const double *noise, int64_t noise_len,
                 double *out);
/* A panel: n_draws draws of every chain from ONE noise stream (draw b of a chain reads noise[b * stride, (b + 1) * stride),
 * stride = chain_len + 2 maxLag; noise_len >= n_draws * the largest stride).  ctx NULL = the default context; on a batch context
 * the panel has buffers of its own and changes neither a resident array of the fit nor the record of its last pass.  templates:
 * the chains' templates one after the other.  draws_per_group (0 = default: what fits 16 GiB) bounds the working set: the draws of
 * one group are resident at a time and the second phase makes them again; results do not depend on it.
 *   order_stats: ranks[chain][n_ranks] (0-based, -1 = unused, n_ranks <= 16) -> out[chain][draw][rank], exact order statistics;
 *   tail_stats:  offsets / scales [chain][n_z] (n_z <= 16) -> counts[chain][draw][z] = #(draw > offset),
 *                soft[chain][draw][z] = np.mean(np.clip((draw - offset) / max(scale, DBL_MIN), 0, None)) in NumPy's summation order.
 * panel_end frees the panel's device memory. */
int csr_dwb_panel_begin(csr_ctx *ctx, int32_t n_chains, const int64_t *chain_len, const int32_t *bandwidth, const char *kernel,
                        const double *templates, const double *noise, int64_t noise_len, int32_t n_draws, int32_t draws_per_group);
int csr_dwb_panel_order_stats(csr_ctx *ctx, int32_t n_ranks, const int64_t *ranks, double *out);
int csr_dwb_panel_tail_stats(csr_ctx *ctx, int32_t n_z, const double *offsets, const double *scales, int64_t *counts, double *soft);
int csr_dwb_panel_end(csr_ctx *ctx);
/* The same tail statistics of one vector: a host array, or a chain's resident score track (csr_batch_rocco_scores /
 * csr_batch_upload_scores), which is only read.  offsets / scales / counts / soft: n_z values. */
int csr_dwb_tail_stats(csr_ctx *ctx, const double *x, int64_t n, int32_t n_z, const double *offsets, const double *scales,
                       int64_t *counts, double *soft);
int csr_batch_dwb_observed(csr_ctx *ctx, int32_t chain, int32_t n_z, const double *offsets, const double *scales, int64_t *counts,
                           double *soft);

/* ---- multiscale candidate segments: pyx:9460-9669 `cMultiscaleCandidateSegmentStats`, which the reference's DWB peak scoring
 * (peaks.py:2359-2481, 2605-3020) calls on the observed score track and on every null replay ------------------------------------
 * Every returned value equals the reference's bit for bit.  A TRACK is one vector of values: the host vector, a chain's resident
 * score track, or one draw of one chain of the DWB panel.  Per track: scales (window widths in bins, clamped to [1, n]; at most
 * 16) and views ((threshold, null scale) pairs, null scales raised to DBL_MIN; at most 16).  min_run_bins below 1 counts as 1,
 * max_gap_bins below 0 as 0, max_segments_per_view <= 0 as "no cap".  Rows are ordered by track, scale, view, start; the `scale`
 * column holds the clamped width, the `view` column the index of the view.  counters: per track 3 values -- eligible candidates,
 * views that hit the cap, candidates the cap discarded.
 *
 * Two phases, so that no output size has to be guessed.  Phase 1 (a *_run entry, or csr_dwb_panel_segments) computes everything,
 * keeps the rows in the context and returns the row counts and counters.  Phase 2 (csr_segments_fetch) copies the eight row
 * arrays; it addresses the context's LAST run.  ctx NULL = the default context.
 *
 * The cap.  The reference keeps np.argpartition(-score, cap - 1)[:cap] of a view's candidates, ordered by start.  That set is
 * determined by the values only if every candidate score of the view is finite and the cap-th and (cap + 1)-th largest differ;
 * then the device selects it exactly.  Otherwise the view is FLAGGED: *n_flagged counts such views, csr_segments_flagged names
 * one (track, index into the track's scales, view, number of candidates), csr_segments_flagged_fetch returns its candidates'
 * score and start, and the caller passes the chosen `cap` candidates in output order to csr_segments_flagged_select (the Python
 * layer uses the reference's own two NumPy calls).  csr_segments_fetch fails while a flagged view is unresolved.
 *
 * Device memory of a run with R rows (tracks per chain), N bins per row (all chains), S scales and V views:
 * about R * N * (8 + 16 V + 24.5 S V) bytes (562 bytes per bin and row at 5 scales x 4 views): the arrays are sized for the worst
 * case of n / 2 runs per (row, scale, view).  It is kept for the next run and freed by csr_dwb_panel_end (with the panel's own
 * buffers) or with the context.  A run's maximum is taken by eight lanes, so a single run costs length / 8 dependent loads: one
 * run as long as a chromosome (a scale of n, or a threshold below the whole track) is a loop of n / 8 steps of one lane group.
 * R * S * V may not exceed 65535.  The reference's one ValueError (different numbers of thresholds and null scales) returns
 * CSR_SEG_ERR_VALUE before any launch; n, n_scales or n_thresholds <= 0 gives no rows and zero counters. */
enum { CSR_SEG_ERR_VALUE = CSR_ERR_VALUE };
int csr_segments_run(csr_ctx *ctx, const double *scores, int64_t n, int32_t n_scales, const int64_t *scales, int32_t n_thresholds,
                     const double *thresholds, int32_t n_null_scales, const double *null_scales, int32_t min_run_bins,
                     int32_t max_gap_bins, int32_t max_segments_per_view, int64_t *n_rows, int64_t *counters, int32_t *n_flagged);
/* The resident score tracks of a batch (every chain needs one: csr_batch_rocco_scores / csr_batch_upload_scores); they are only
 * read and no resident array changes.  n_scales / n_views: one count per chain; scales, thresholds and null_scales: the chains'
 * values one after the other.  rows[chain], counters[chain][3]; track = chain. */
int csr_batch_segments_run(csr_ctx *ctx, const int32_t *n_scales, const int64_t *scales, const int32_t *n_views,
                           const double *thresholds, const double *null_scales, int32_t min_run_bins, int32_t max_gap_bins,
                           int32_t max_segments_per_view, int64_t *rows, int64_t *counters, int32_t *n_flagged);
/* A third phase of the DWB panel, between csr_dwb_panel_begin and csr_dwb_panel_end, in any order with the other two: draws
 * first_draw .. first_draw + n_draws - 1 of every chain (n_draws at most the panel's draws per group) are made as in the other
 * phases and read.  Needs max_segments_per_view > 0.  rows[chain][draw], counters[chain][draw][3]; track = chain * n_draws + draw.
 * The caller resolves the flagged views of this group and fetches its rows before it asks for the next group. */
int csr_dwb_panel_segments(csr_ctx *ctx, int32_t first_draw, int32_t n_draws, const int32_t *n_scales, const int64_t *scales,
                           const int32_t *n_views, const double *thresholds, const double *null_scales, int32_t min_run_bins,
                           int32_t max_gap_bins, int32_t max_segments_per_view, int64_t *rows, int64_t *counters,
                           int32_t *n_flagged);
int csr_segments_flagged(csr_ctx *ctx, int32_t k, int32_t *track, int32_t *scale_index, int32_t *view, int64_t *n_candidates);
int csr_segments_flagged_fetch(csr_ctx *ctx, int32_t k, double *score, int64_t *start);
int csr_segments_flagged_select(csr_ctx *ctx, int32_t k, int64_t n_selected, const int64_t *selected);
int csr_segments_fetch(csr_ctx *ctx, int64_t *start, int64_t *end, int64_t *scale, int64_t *view, double *score,
                       double *integrated, double *mean, double *max_excess);

/* ---- the robust null of a ROCCO score track: peaks.py:312-339 `_halfSampleMode`, 418-496 `_selectRobustNullSupport`, 499-540
 * `estimateROCCONull`, 543-556 `_estimateTemplateScale`, 1077-1122 `_prepareNullResidualTemplate` ------------------------------
 * Every value equals the reference's bit for bit (a zero may differ in sign when the track holds -0.0: the device orders -0.0
 * before +0.0, np.sort does not).  The track is sorted on the device; order statistics, the half-sample mode, the stable
 * compaction of the support and NumPy-order sums come from kernels, the scalars between them are composed on the host.
 * host_fallback = 1: the central support holds fewer than max(16, ceil(0.05 n)) values (always so below 16 values).  The reference
 * then takes an UNSTABLE argsort of the track, whose tie order the values do not determine: the caller decides such a track with
 * NumPy; the fields up to support_size are filled as far as they were reached, no template is left.
 * A non-finite or empty vector returns CSR_NULL_ERR_VALUE with the reference's ValueError text, before any launch. */
enum { CSR_NULL_ERR_VALUE = CSR_ERR_VALUE };
enum { CSR_NULL_LOWER_BULK = 0, CSR_NULL_FULL_TRACK = 1 };                  /* bulk_source */
enum { CSR_NULL_HALF_SAMPLE_MODE = 0, CSR_NULL_MEDIAN = 1 };                /* center_method (after the bulk source) */
enum { CSR_NULL_CENTRAL_SUPPORT = 0, CSR_NULL_NEAREST_SUPPORT = 1 };        /* null_method */
typedef struct csr_null_out {
    double null_center, null_scale;
    double bulk_quantile, bulk_cutoff, provisional_center, support_radius, support_scale, support_fraction;
    double clip_abs, template_std, template_mean;
    int64_t support_size, lower_bulk_size;
    int32_t bulk_source, center_method, null_method, host_fallback;
} csr_null_out;
/* Host arrays (default context).  given: NULL, or {null centre, null scale} around which the template is built instead of the
 * track's own (the arguments of `_prepareNullResidualTemplate`).  template_out: n values or NULL.
 * csr_null_scale: out[4] = `_estimateTemplateScale`, then its MAD-, IQR- and std-based parts. */
int csr_null_prepare(const double *scores, int64_t n, double bulk_quantile, const double *given, csr_null_out *out,
                     double *template_out);
int csr_null_scale(const double *x, int64_t n, double *out);
/* The device's ascending sort of a finite vector (keys only: a function of the values alone), n values out. */
int csr_null_sort(const double *x, int64_t n, double *out);
/* The RESIDENT score tracks of a batch (csr_batch_rocco_scores / csr_batch_upload_scores) for the chains of chain_mask (n_chains
 * bytes or NULL = all); out: n_chains records, those of the other chains untouched.  The templates stay on the device in a buffer
 * of the batch's own; no array of the fit or of the scores changes.  template_upload plants a chain's template (a host-decided
 * chain's, a test's).  pooled_scale: csr_null_scale of the selected chains' templates concatenated in chain order. */
int csr_batch_null_prepare(csr_ctx *ctx, double bulk_quantile, const unsigned char *chain_mask, csr_null_out *out);
int csr_batch_null_template_download(csr_ctx *ctx, int32_t chain, double *host_dst);
int csr_batch_null_template_upload(csr_ctx *ctx, int32_t chain, const double *tmpl);
int csr_batch_null_pooled_scale(csr_ctx *ctx, const unsigned char *chain_mask, double *out);
/* csr_dwb_panel_begin over ALL chains of the batch with their resident templates (every chain needs one); the other panel calls
 * follow as usual. */
int csr_batch_dwb_panel_begin(csr_ctx *ctx, const int32_t *bandwidth, const char *kernel, const double *noise, int64_t noise_len,
                              int32_t n_draws, int32_t draws_per_group);

/* ---- the effective sample size scan behind the ROCCO budget: pyx:9160-9279 `cEstimateEffectiveSampleSize` ----------------------
 * (n_eff, tau, lags_used) equal the reference's bit for bit: the mean, the variance sum and the covariance sum of every lag are
 * walked in index order on the device (separate multiply and add), the host composes rho, the break / taper rule and the clamps.
 * Lags are scanned in rounds; a scan that broke asks for no further round.
 * csr_ess_scan (default context): values = the series, already log-transformed by the caller when the reference's logPositive is
 * set; general != 0, a mask or a window selects the reference's second path (finiteness check of the active values, pair counts,
 * taper).  The reference's ValueErrors return CSR_ESS_ERR_VALUE with its text: "windowIntervals must be nonnegative" and "active
 * values must be finite" before any launch; "variance estimate must be finite" and "autocorrelation estimate must be finite"
 * depend on the sums.
 * csr_batch_ess: the series of peaks.py:1414-1434 built on the device from the RESIDENT score tracks (kind 1: score > threshold
 * as 0 / 1; 2: max((score - threshold) / max(scale, DBL_MIN), 0); 3: those of n_z (threshold, scale) pairs added in order, / n_z),
 * scanned on the reference's fast path.  thresholds / scales: [chain][n_z] (n_z <= 16; kinds 1 and 2 read the first pair);
 * max_lags[chain]; chain_mask: n_chains bytes or NULL = all; out: n_chains records, those of the other chains untouched.  No
 * resident array changes. */
enum { CSR_ESS_ERR_VALUE = CSR_ERR_VALUE };
enum { CSR_ESS_OCCUPANCY = 1, CSR_ESS_SOFT = 2, CSR_ESS_INTEGRATED = 3 };
typedef struct csr_ess_out {
    double n_eff, tau;
    int64_t lags_used;
} csr_ess_out;
int csr_ess_scan(const double *values, int64_t n, int64_t max_lag, const unsigned char *active_mask, int32_t general,
                 int64_t window_intervals, csr_ess_out *out);
int csr_batch_ess(csr_ctx *ctx, int32_t kind, int32_t n_z, const double *thresholds, const double *scales, const int64_t *max_lags,
                  const unsigned char *chain_mask, csr_ess_out *out);
/* What `estimateROCCOGamma` (peaks.py:1741-1751) reads of a resident score track: count[chain] = how many scores have
 * score - levels[chain] > 0, and mid[2 chain], mid[2 chain + 1] = the lower and upper middle SCORES of those (equal for an odd
 * count, untouched for none) -- the caller subtracts the level and averages, as np.median does.  The tracks are sorted with the
 * null's sort in work space; no resident array changes. */
int csr_batch_rocco_excess_ranks(csr_ctx *ctx, const double *levels, const unsigned char *chain_mask, int64_t *count, double *mid);
/* Plants the selection mask (bytes 0 / 1) of one chain, decided by the caller (the contiguous-window fallback of
 * `solveChromROCCO`, peaks.py:1812-1835); csr_batch_rocco_download / csr_batch_rocco_runs then serve it.  Needs an earlier
 * csr_batch_rocco of the batch. */
int csr_batch_rocco_upload(csr_ctx *ctx, int32_t chain, const unsigned char *solution);

/* ---- the numeric side of the DWB peak scoring: peaks.py:2295-2356 `_segmentScoreAgainstThresholdView` and
 * `_bestSegmentScoreAcrossThresholdViews`, 2182-2203 `_empiricalReplaySegmentPValues`, 2206-2257 `_replayFDRQValues` ------------
 * Every value equals the reference's bit for bit.
 * Segment scores: n_seg segments [start, end] (inclusive; clamped to the track as the reference clamps them, end < start after
 * that: an empty segment, all zeros, view 0) of one float64 track -- a host vector (default context), or a chain's resident score
 * track, which is only read -- against n_views (threshold, null scale) pairs (1..16; null scales raised to DBL_MIN).  Per segment:
 * the excess e = clip((s - threshold) / scale, 0, inf) of the best view, integrated = np.sum(e) in NumPy's summation order,
 * score = integrated / sqrt(len), mean = integrated / len, max_excess = np.max(e), view = the index of that view.  The first view
 * is the best and a later one replaces it only if its score compares > (a NaN score never replaces).
 * p and q values: observed[n_metrics][K] statistics against pool[n_metrics][N], the statistics of all replay draws of a metric one
 * after the other in any order, n_draws = how many draws there were (empty ones count; N > 0 needs n_draws > 0).  Both are
 * sorted on the device (the null's keys-only sort); c = #(pool >= x) by bisection on `<`, so -0.0 and +0.0 are equal;
 *   exceed_out = c,  p_out = clip((1 + c) / (N + 1), 0, 1)  (all ones when N == 0),
 *   q_out = min over the observed y <= x of clip((c(y) / n_draws + pseudo) / max(#(observed >= y), 1), 0, 1),
 *           pseudo = 1 / (n_draws + 1), or 1 without draws -- c(y) / n_draws is the mean of the per-draw counts the reference takes.
 * what: CSR_PEAK_P and / or CSR_PEAK_Q; with CSR_PEAK_Q_MAX_P as well q_out = max(q, p), what the scorer keeps (peaks.py:2931-2940).
 * A non-finite value is found on the device: err_flags (may be NULL) names where, and the call returns CSR_PEAK_ERR_VALUE with the
 * reference's text before any result is written -- "replay segment statistics contain non-finite values" if p values were asked
 * for and N > 0, else "replay FDR statistics contain non-finite values" if q values were.  Outputs not asked for may be NULL. */
enum { CSR_PEAK_ERR_VALUE = CSR_ERR_VALUE };
enum { CSR_PEAK_P = 1, CSR_PEAK_Q = 2, CSR_PEAK_Q_MAX_P = 4 };              /* what */
enum { CSR_PEAK_BAD_OBSERVED = 1, CSR_PEAK_BAD_POOL = 2 };                  /* err_flags */
int csr_peakscore_segments(const double *scores, int64_t n, int64_t n_seg, const int64_t *starts, const int64_t *ends,
                           int32_t n_views, const double *thresholds, const double *null_scales, double *score, double *integrated,
                           double *mean, double *max_excess, int32_t *view);
int csr_batch_peakscore_segments(csr_ctx *ctx, int32_t chain, int64_t n_seg, const int64_t *starts, const int64_t *ends,
                                 int32_t n_views, const double *thresholds, const double *null_scales, double *score,
                                 double *integrated, double *mean, double *max_excess, int32_t *view);
int csr_peakscore_pq(const double *observed, int64_t K, const double *pool, int64_t N, int64_t n_draws, int32_t n_metrics,
                     int32_t what, double *p_out, double *q_out, int64_t *exceed_out, uint32_t *err_flags);
/* The replay pool of a DWB panel (ctx NULL = the default context), valid between csr_dwb_panel_begin and csr_dwb_panel_end: per
 * chain the three metric columns (score, integrated excess, max excess) of every replay candidate `compose` keeps, resident on
 * the device -- the panel's own memory, freed by csr_dwb_panel_end (or csr_dwb_panel_pool_end).  max_segments: the total cap per
 * draw (<= 0: none).  While a pool is open csr_dwb_panel_segments leaves its rows on the device (csr_segments_fetch fails; flagged
 * views are resolved as usual), so run the observed tracks before pool_begin.  After each csr_dwb_panel_segments group, with its
 * flagged views resolved, pool_append(first_draw) appends every (chain, draw) track of the group: a track over the total cap keeps
 * the first max_segments rows of the stable descending order on score -- rank #(s[j] > s[i]) + #(s[j] == s[i], j < i), which is
 * also the row's place in the pool -- and the pool grows by exactly what the group's row counts ask for.  *n_flagged: tracks over
 * the cap that hold a NaN score, whose order the values do not determine.  pool_flagged names one (chain, draw, rows),
 * pool_flagged_fetch returns its rows (the eight columns of csr_segments_fetch; the only replay rows that leave the device) and
 * the caller hands back the max_segments candidates it kept with pool_flagged_upload, before the next group.  draw_stats, once
 * every draw is in: per (chain, draw) the candidate count after and before the total cap, phase 1's three counters and np.max of
 * the kept scores (0.0 without candidates); *fetched_tracks (may be NULL) = how many draws' rows were fetched.  pool_pq:
 * csr_peakscore_pq of observed[3][K] (the pool's column order) against one chain's pool, n_draws = the panel's draws. */
int csr_dwb_panel_pool_begin(csr_ctx *ctx, int64_t max_segments);
int csr_dwb_panel_pool_append(csr_ctx *ctx, int32_t first_draw, int32_t *n_flagged);
int csr_dwb_panel_pool_flagged(csr_ctx *ctx, int32_t k, int32_t *chain, int32_t *draw, int64_t *n_rows);
int csr_dwb_panel_pool_flagged_fetch(csr_ctx *ctx, int32_t k, int64_t *start, int64_t *end, int64_t *scale, int64_t *view,
                                     double *score, double *integrated, double *mean, double *max_excess);
int csr_dwb_panel_pool_flagged_upload(csr_ctx *ctx, int32_t k, int64_t n_values, const double *score, const double *integrated,
                                      const double *max_excess);
int csr_dwb_panel_pool_draw_stats(csr_ctx *ctx, int64_t *count, int64_t *before, int64_t *counters, double *max_score,
                                  int64_t *fetched_tracks);
int csr_dwb_panel_pool_pq(csr_ctx *ctx, int32_t chain, const double *observed, int64_t K, int32_t what, double *p_out, double *q_out,
                          int64_t *exceed_out, uint32_t *err_flags);
/* A chain's pool as it stands: *n = values per column; the first *n of each column go to the non-NULL buffers. */
int csr_dwb_panel_pool_download(csr_ctx *ctx, int32_t chain, int64_t *n, double *score, double *integrated, double *max_excess);
int csr_dwb_panel_pool_end(csr_ctx *ctx);

/* ---- nested ROCCO refinement: peaks.py:3519-3720 `_solveParentConditionedSubpeaks`, 2133-2160
 * `_parentConditionedSubpeakObjective`, 2089-2114 `_nestedSoftSelectionPenalty`, and what `_refineNestedROCCOSolution`
 * (peaks.py:3763-4388) does per region, per new node and per layer -----------------------------------------------------------
 * Every value equals the reference's bit for bit.  The device works on regions: bins [start, end] (inclusive) of one chain,
 * given in ascending order of (chain, start) and disjoint.  The hierarchy (node ids, layers, history, the stop rule) and the
 * geometry (which regions are too short, `_minimumChildBinsForRegion`) are the caller's: they need intervals / ends, which are
 * host arrays, and compact records only.
 *   nodes          per region what `_addNode` records: the leftmost arg-max of the raw scores, that raw score, np.sum of the scores.
 *   layer          per region peaks.py:4042-4172: required bin, the 25 % floor (cfg.subtract_floor: layers >= 2), the soft selection
 *                  penalty (cfg.selection_penalty and cfg.budget_scale are the LAYER's: 0 and 1 from layer 2 on), the dynamic
 *                  programme with min_run + 1 states, both objectives, split gain, gates and decision.  A region that splits or
 *                  shrinks has its bins of the solution mask replaced.  *n_children = the candidate runs of all regions; region
 *                  k's are children[rec[k].child_base .. + rec[k].n_runs), each a node record, fetched with csr_nested_children
 *                  (ctx NULL = the default context of the host-array calls) until the next layer call of that context.
 *   selected_sum   per chain np.sum(scores[mask > 0]) for the mask that is the union of the given runs (n_runs[chain] of them,
 *                  ascending and disjoint, concatenated in starts / ends): the float part of `_roccoObjectiveForSolution`.
 *   solve          one region with general boundary costs (n + 1 of them), a required bin or none (-1): the mask and the record.
 * min_run is clamped to the region's length; above CSR_NESTED_MAX_MIN_RUN the call returns CSR_ERR_VALUE.  Arguments the
 * reference answers with ValueError return CSR_ERR_VALUE with its text, before any launch.  The host-array calls take the
 * chains one after the other (chain_len[n_chains], scores, raw_scores or NULL for the scores themselves, solution in and out); the
 * batch calls read the resident score tracks and read and write the resident solution masks of the chains chain_mask takes
 * (NULL: all; a region of a chain it leaves out is an error), and change no other resident array. */
enum { CSR_NESTED_KEEP_PARENT = 0, CSR_NESTED_SPLIT = 1, CSR_NESTED_SHRINK = 2, CSR_NESTED_INFEASIBLE = -1 };   /* decision */
#define CSR_NESTED_MAX_MIN_RUN 255
typedef struct csr_nested_region {
    int64_t start, end;
    int32_t chain, min_run;
} csr_nested_region;
typedef struct csr_nested_cfg {     /* per chain and layer */
    double gamma;               /* the PARENT's gamma: an inner boundary costs max(0.25 gamma, 1e-9) */
    double selection_penalty, budget_scale;
    int32_t subtract_floor, reserved;
} csr_nested_cfg;
typedef struct csr_nested_rec {     /* per region */
    int64_t required;           /* the required bin, as an index of the chain (-1: none) */
    int64_t selected_count;
    int64_t child_base;
    int32_t n_runs, decision, widths_ok, reserved;
    double floor, selection_penalty, extra_penalty;
    double objective, penalized, boundary_penalty, run_penalty_total, parent_penalized, split_gain;
} csr_nested_rec;
typedef struct csr_nested_node {
    int64_t start, end, required;   /* indices of the chain */
    double raw_score_max, score_sum;
} csr_nested_node;
int csr_nested_solve(const double *scores, int64_t n, const double *boundary_costs, double selection_penalty, int32_t min_run,
                     int64_t required, double run_penalty, uint8_t *mask, csr_nested_rec *out);
int csr_nested_nodes(int32_t n_chains, const int64_t *chain_len, const double *scores, const double *raw_scores, int64_t n_regions,
                     const csr_nested_region *regions, csr_nested_node *nodes);
int csr_nested_layer(int32_t n_chains, const int64_t *chain_len, const double *scores, const double *raw_scores, uint8_t *solution,
                     const csr_nested_cfg *cfg, int64_t n_regions, const csr_nested_region *regions, csr_nested_rec *rec,
                     int64_t *n_children);
int csr_nested_children(csr_ctx *ctx, int64_t capacity, csr_nested_node *children);
int csr_nested_selected_sum(int32_t n_chains, const int64_t *chain_len, const double *scores, const int64_t *n_runs,
                            const int64_t *starts, const int64_t *ends, double *sums);
int csr_batch_nested_nodes(csr_ctx *ctx, int64_t n_regions, const csr_nested_region *regions, csr_nested_node *nodes);
int csr_batch_nested_layer(csr_ctx *ctx, const csr_nested_cfg *cfg, const unsigned char *chain_mask, int64_t n_regions,
                           const csr_nested_region *regions, csr_nested_rec *rec, int64_t *n_children);
int csr_batch_nested_selected_sum(csr_ctx *ctx, const unsigned char *chain_mask, const int64_t *n_runs, const int64_t *starts,
                                  const int64_t *ends, double *sums);

/* ---- narrowPeak export: the numeric part of `_solutionToChromNarrowPeakRows` (peaks.py:5202-5567) without a width policy and
 * without a hierarchy -- `_solveParentConditionedSubpeakSegments` (4507-4576), `_trimChildSegmentAroundSummit` (4789-4824), the
 * two medians, the two maxima and the median filter ------------------------------------------------------------------------
 * Every value equals the reference's bit for bit.  A PARENT is a run of the solution mask that holds no coordinate gap: bins
 * [start, end] (inclusive) of one chain, ascending by (chain, start) and disjoint; cutting the mask's runs at gaps is the
 * caller's (it needs the coordinates).  Per parent (cfg.split): the required bin is the leftmost arg-max of the scores, the
 * dynamic programme of the nested layer runs with max(boundary_cost, 0) on ALL n + 1 boundaries, the given selection penalty,
 * min(max(min_run, 1), n) and no run penalty; its runs are the children, each with the parent's number of sub-peaks, penalized
 * objective and boundary penalty.  Without cfg.split the parent is its only child.  Per child: the summit (leftmost arg-max
 * of the signal over the untrimmed child), the trim (cfg.trim: the maximal stretch of scores > trim_floor around the summit,
 * none if the summit's score is not above it), and over the trimmed child np.median and np.max of the signal, np.max of the
 * scores, np.median of the finite uncertainty values (cfg.filter; CSR_EXPORT_HAS_LOCAL_P if there is one) and the flag
 * median < -multiplier * that median (CSR_EXPORT_DROPPED_MEDIAN: the child still comes back, the caller counts it).
 * *count = the children of all parents; csr_export_fetch hands them out in the reference's order (chain, parent, child from
 * left to right; ctx NULL = the default context of the host-array call) until the next export call of that context.
 * parent_flags (n_parents, may be NULL): CSR_EXPORT_NONFINITE_SIGNAL where the signal of a parent holds a non-finite value --
 * NumPy's maxima and medians then propagate NaN in ways no order statistic does; the caller decides such a chain on the host.
 * Non-finite scores inside a parent, a non-finite penalty, boundary cost or multiplier and a negative multiplier return
 * CSR_ERR_VALUE with the reference's text, a minimum run above CSR_NESTED_MAX_MIN_RUN the same CSR_ERR_VALUE as the nested
 * calls; the host-array call checks before any launch, the batch call finds non-finite resident scores in its first kernel and
 * ends there.  The host-array call takes float64 state / scores / uncertainty (NULL: none), the chains one after the other.  The
 * batch call reads the resident score tracks, as signal (double) xs[:,0] and as uncertainty (double)(float) sqrt(Ps00) of the
 * reference-layout copies of the smoothed fit -- the values and the side-effect rule of csr_batch_rocco_scores -- and changes no
 * resident array of the fit, score, mask or template.  Additive to ABI 6. */
enum { CSR_EXPORT_SPLIT_FROM_PARENT = 1, CSR_EXPORT_TRIMMED = 2, CSR_EXPORT_HAS_LOCAL_P = 4, CSR_EXPORT_DROPPED_MEDIAN = 8 };
enum { CSR_EXPORT_NONFINITE_SIGNAL = 1 };
typedef struct csr_export_cfg {     /* per chain */
    double selection_penalty, boundary_cost, trim_floor, multiplier;
    int32_t min_run;            /* minSubpeakBins; clamped to [1, n] per parent */
    int32_t split, trim, filter;    /* switches: sub-peaks; trim (off: floor None or non-finite); the median filter */
} csr_export_cfg;
typedef struct csr_export_parent {
    int64_t start, end;
    int32_t chain, reserved;
} csr_export_parent;
typedef struct csr_export_peak {
    int64_t start, end;                         /* the trimmed child, indices of the chain */
    int64_t untrimmed_start, untrimmed_end, summit;
    int32_t chain, parent;                      /* parent: index into the call's parent list */
    int32_t num_subpeaks, flags;
    double median_state, local_median_p, max_state, max_score, subpeak_objective, subpeak_boundary_penalty;
} csr_export_peak;
int csr_export_peaks(int32_t n_chains, const int64_t *chain_len, const double *state, const double *scores,
                     const double *uncertainty, const csr_export_cfg *cfg, int64_t n_parents, const csr_export_parent *parents,
                     int32_t *parent_flags, int64_t *count);
int csr_batch_export_peaks(csr_ctx *ctx, const csr_export_cfg *cfg, const unsigned char *chain_mask, int64_t n_parents,
                           const csr_export_parent *parents, int32_t *parent_flags, int64_t *count);
int csr_export_fetch(csr_ctx *ctx, int64_t capacity, csr_export_peak *peaks);

/* ---- the massive sub-peak clean-up: `_forceMassiveSubpeakSegments` (peaks.py:4579-4786) with `_bestMassiveSubpeakSplit`
 * (3299-3352) and `_contractMassiveSubpeakSegment` (3355-3460), piece level, on host arrays (default context) ----------------
 * Every value equals the reference's bit for bit.  A CHILD is bins [start, end] (inclusive) of the score array that hold no
 * coordinate gap; the children are disjoint and ascending.  The coordinates are the n + 1 bin edges (bin i is
 * [edges[i], edges[i + 1]), non-decreasing), or edges NULL and edge i = origin + i * step.  One wavefront takes one child.
 *   CSR_CLEANUP_OP_FORCE     the recursion of one child under the policy: forced splits at the best low-score gap, contraction
 *                            to an adaptive or width-capped core.  A child of L bins ends in at most CSR_CLEANUP_MAX_SEGMENTS
 *                            segments (every one holds at least ceil(0.05 L) bins); they come back packed, child after child and
 *                            left to right, *n_segments of them (capacity >= CSR_CLEANUP_MAX_SEGMENTS * n_children always
 *                            suffices), with counts[k].n_segments per child (the reference's num_subpeaks) and its five counters.
 *                            CSR_CLEANUP_SPLIT_FROM_PARENT is set where a child ends in several segments or in a moved one; the
 *                            caller ORs the child's own flag.  policy.contract_threshold is the caller's
 *                            min(contract_width_bp or min_bp or 7500, threshold).  A child narrower than the threshold (or any
 *                            child under a NaN threshold) is its own segment.
 *   CSR_CLEANUP_OP_SPLIT     nodes[k] = the best split of child k's scores with min_run as `minRunBins` (found 0: None).
 *   CSR_CLEANUP_OP_CONTRACT  nodes[k] = the contraction of child k with contract_threshold as `thresholdBP` and min_run as
 *                            `minRunBins` (found 0: None).
 * Checked before any launch: a non-finite score inside a child that the call would evaluate returns CSR_ERR_VALUE with the
 * reference's "`scores` contains non-finite values"; a max_depth above CSR_CLEANUP_MAX_DEPTH, a non-finite split quantile,
 * minimum z or boundary cost return CSR_ERR_VALUE.  Order statistics come from a sort that puts -0.0 and +0.0 in either order
 * (NumPy: equal): where every score of a node is a zero, `z` of its refused split may differ in the sign of a zero.
 * CSR_CLEANUP_SORT_TILE: node lengths up to it are sorted in LDS, longer ones in global memory.  Additive to ABI 6. */
#define CSR_CLEANUP_MAX_SEGMENTS 20
#define CSR_CLEANUP_MAX_DEPTH 32
#define CSR_CLEANUP_SORT_TILE 2048
enum { CSR_CLEANUP_OP_FORCE = 0, CSR_CLEANUP_OP_SPLIT = 1, CSR_CLEANUP_OP_CONTRACT = 2 };
enum { CSR_CLEANUP_MODE_NONE = 0, CSR_CLEANUP_MODE_UNSPLIT = 1, CSR_CLEANUP_MODE_SPLIT = 2, CSR_CLEANUP_MODE_ADAPTIVE_CORE = 3,
       CSR_CLEANUP_MODE_WIDTH_CAPPED_CORE = 4 };
enum { CSR_CLEANUP_CANDIDATE = 1, CSR_CLEANUP_APPLIED = 2, CSR_CLEANUP_HAS_SPLIT = 4, CSR_CLEANUP_HAS_CORE_WIDTH = 8,
       CSR_CLEANUP_HAS_CORE_FLOOR = 16, CSR_CLEANUP_MOVED = 32, CSR_CLEANUP_SPLIT_FROM_PARENT = 64 };
enum { CSR_CLEANUP_NONFINITE = 1, CSR_CLEANUP_OVERFLOW = 2 };    /* csr_cleanup_counts.flags */
typedef struct csr_cleanup_policy {
    double threshold, contract_threshold, split_quantile, min_split_z, boundary_cost;
    int32_t min_run, max_depth;
} csr_cleanup_policy;
typedef struct csr_cleanup_child {
    int64_t start, end;
} csr_cleanup_child;
typedef struct csr_cleanup_segment {
    int64_t start, end, core_width_bp;          /* core_width_bp: with CSR_CLEANUP_HAS_CORE_WIDTH */
    double gain, z, core_score_floor;           /* gain, z, gap_bins: with CSR_CLEANUP_HAS_SPLIT; the floor: HAS_CORE_FLOOR */
    int32_t gap_bins, mode, flags, child;
} csr_cleanup_segment;
typedef struct csr_cleanup_counts {
    int32_t candidates, splits, segments_added, evaluated, contracts, n_segments, flags, reserved;
} csr_cleanup_counts;
typedef struct csr_cleanup_node {
    int64_t a, b, width;                        /* split: the gap, local to the child; contract: the core's bins and width */
    double baseline, scale, deficit, gain, z, floor;
    int32_t found, mode, gap_bins, reserved;
} csr_cleanup_node;
/* The same recursion on the RESIDENT score tracks of a batch (no resident array changes): children as (chain, bins of the chain),
 * ascending by (chain, start) and disjoint, a policy per chain (those of chains the call takes are read), the coordinates as one
 * packed array -- child k's n_k + 1 edges start at edges[edge_base] -- or edges NULL and equally wide bins of `step`.  The segments
 * come back in bins of their chain.  A non-finite resident score inside a candidate returns CSR_ERR_VALUE with the reference's
 * text (found by the kernel). */
typedef struct csr_cleanup_batch_child {
    int64_t start, end, edge_base;
    int32_t chain, reserved;
} csr_cleanup_batch_child;
int csr_batch_cleanup_plan(csr_ctx *ctx, const csr_cleanup_policy *policies, const unsigned char *chain_mask, int64_t n_children,
                           const csr_cleanup_batch_child *children, int64_t n_edges, const int64_t *edges, int64_t step,
                           int64_t capacity, csr_cleanup_segment *segments, int64_t *n_segments, csr_cleanup_counts *counts);
int csr_cleanup_plan(int32_t op, int64_t n, const double *scores, const int64_t *edges, int64_t origin, int64_t step,
                     int64_t n_children, const csr_cleanup_child *children, const csr_cleanup_policy *policy, int64_t capacity,
                     csr_cleanup_segment *segments, int64_t *n_segments, csr_cleanup_counts *counts, csr_cleanup_node *nodes);

/* ---- broad mode: the per-bin arithmetic of `_mergeBroadRunsByObjective` (peaks.py:1898-2005) and of
 * `_solutionToChromBroadPeakRows` (5606-5818), on host arrays (default context) ----------------------------------------------
 * Every value equals the reference's bit for bit.
 *   csr_broad_gap_sums   sums[g] = np.sum(np.where(ex < 0, f * ex, ex)), ex = scores[gap_start[g] .. + gap_len[g]) -
 *                        selection_penalty, f = dip_fraction (the caller clips it to [0, 1]), in NumPy's order; 0.0 for a gap
 *                        of no bin.  The gaps may be given in any order and may overlap.  Distance, blacklist and the gain
 *                        decision are the caller's: they need coordinates, and each gap is decided on its own.
 *   csr_broad_rows       A PARENT is bins [start, end] (inclusive) of one chain without a coordinate gap, ascending by (chain,
 *                        start) and disjoint (csr_export_parent).  One wavefront takes one parent.  records[k]: np.median, the
 *                        leftmost arg-max (summit, a bin of the chain), np.max and np.mean of the signal, np.max and np.mean of
 *                        the scores, and with cfg.filter and an uncertainty array np.median of its finite values
 *                        (CSR_BROAD_HAS_LOCAL_P if there is one) and the flag median < -multiplier * that median
 *                        (CSR_BROAD_DROPPED_MEDIAN: the record still comes back, the caller counts it).
 *                        CSR_BROAD_NONFINITE: the parent's signal or scores hold a non-finite value, NumPy's maxima, medians
 *                        and means then propagate NaN in ways no order statistic does; the caller decides such a chain on the
 *                        host.  parent_mask (all bins of all chains, may be NULL): 1 inside a parent, 0 elsewhere.
 * A non-finite or negative multiplier returns CSR_ERR_VALUE with the reference's text; parents outside their chain or not
 * disjoint and ascending, and gaps outside the scores, fail plainly; every check comes before a device is touched.  Medians up
 * to CSR_CLEANUP_SORT_TILE values are sorted in LDS, longer ones in global memory.  A maximum or a median that is a zero may
 * carry either sign where both zeros occur.  Additive to ABI 6. */
enum { CSR_BROAD_HAS_LOCAL_P = 1, CSR_BROAD_DROPPED_MEDIAN = 2, CSR_BROAD_NONFINITE = 4 };
typedef struct csr_broad_cfg {      /* per chain */
    double multiplier;
    int32_t filter, reserved;
} csr_broad_cfg;
typedef struct csr_broad_parent {
    int64_t start, end, summit;     /* bins of the chain */
    int32_t chain, flags;
    double median_state, local_median_p, max_state, max_score, mean_state, mean_score;
} csr_broad_parent;
int csr_broad_gap_sums(int64_t n, const double *scores, double selection_penalty, double dip_fraction, int64_t n_gaps,
                       const int64_t *gap_start, const int64_t *gap_len, double *sums);
int csr_broad_rows(int32_t n_chains, const int64_t *chain_len, const double *state, const double *scores,
                   const double *uncertainty, const csr_broad_cfg *cfg, int64_t n_parents, const csr_export_parent *parents,
                   unsigned char *parent_mask, csr_broad_parent *records);

/* The same on the RESIDENT data of a batch.  Two more per-chain tracks live next to the scores, the template and the (strong)
 * solution mask: the WEAK solution and the BROAD PARENT mask; new scores of a chain drop both.  The fit's arrays, the scores, the
 * template and the strong mask are only read by every call below.
 *   csr_batch_rocco_weak        csr_batch_rocco with the weak track as destination (same arguments and results); the strong mask
 *                               and its flags stay untouched.  _upload / _download move one chain's weak mask (the caller's
 *                               fallback window), csr_batch_broad_parent_download one chain's parent mask.
 *   csr_batch_broad_runs        per taken chain (it needs scores, a strong and a weak mask): the runs of scores >= threshold, cut
 *                               after every bin of the chain's ascending `breaks` (n_breaks[chain] of them, the chains one after the
 *                               other; the caller forms them as flatnonzero(ends[:-1] != intervals[1:])); counts[chain].support_runs
 *                               of them.  Kept are the runs that hold a bin of weak | strong (touching_runs); where a chain keeps
 *                               none, the same kernels run once more with weak | strong as the predicate (fallback = 1).  Per kept
 *                               run one record, in order: its bins, and gap_sum = csr_broad_gap_sums of the bins between it and the
 *                               chain's next kept run under the chain's selection_penalty and dip_fraction (0.0 behind the last
 *                               one, and for a gap of more than max_gap_bins bins, which the caller's distance test blocks anyway:
 *                               no lane walks a gap that long).  *n_records = the records of all chains; csr_batch_broad_runs_fetch hands them out until the
 *                               next call.  Flag, scan and compaction, over bins and then over runs: no atomic counter, no sort.
 *   csr_batch_broad_rows        csr_broad_rows with the resident scores, as signal (double) xs[:,0] and as uncertainty
 *                               (double)(float) sqrt(Ps00) of the reference-layout copies of the smoothed fit (cfg.filter) -- the
 *                               values and the side-effect rule of csr_batch_rocco_scores.  It fills the parent mask of every
 *                               taken chain (0 outside the call's parents). */
typedef struct csr_broad_run_cfg {  /* per chain */
    double threshold, selection_penalty, dip_fraction;
    int64_t max_gap_bins;           /* a gap of more bins is not summed (gap_sum 0.0): the caller's distance test blocks it; < 0: none */
} csr_broad_run_cfg;
typedef struct csr_broad_run_counts {
    int64_t support_runs, touching_runs;
    int32_t fallback, reserved;
} csr_broad_run_counts;
typedef struct csr_broad_run {
    int64_t start, end;             /* bins of the chain */
    double gap_sum;
    int32_t chain, reserved;
} csr_broad_run;
int csr_batch_rocco_weak(csr_ctx *ctx, const csr_rocco_cfg *cfg, const unsigned char *chain_mask, csr_rocco_out *out);
int csr_batch_rocco_weak_upload(csr_ctx *ctx, int32_t chain, const unsigned char *solution);
int csr_batch_rocco_weak_download(csr_ctx *ctx, int32_t chain, uint8_t *solution);
int csr_batch_broad_parent_download(csr_ctx *ctx, int32_t chain, uint8_t *mask);
int csr_batch_broad_runs(csr_ctx *ctx, const csr_broad_run_cfg *cfg, const unsigned char *chain_mask, const int64_t *n_breaks,
                         const int64_t *breaks, csr_broad_run_counts *counts, int64_t *n_records);
int csr_batch_broad_runs_fetch(csr_ctx *ctx, int64_t capacity, csr_broad_run *records);
int csr_batch_broad_rows(csr_ctx *ctx, const csr_broad_cfg *cfg, const unsigned char *chain_mask, int64_t n_parents,
                         const csr_export_parent *parents, csr_broad_parent *records);

/* ---- the dependence span: the device stages of pyx:3360-4120 `cchooseDependenceSpan` (helpers pyx:2645-3357) ------------------
 * Three stages, each on host arrays (default context; mats[k] = n_rows x n_bins[k] float32 in C order, staged one chromosome or one
 * window set at a time) and on the RESIDENT data of the listed chains of a batch (chains[k]: a chain index; a fold chain is left
 * out by not listing it; no resident array changes).  The caller composes the rest (consenrich_amd/depspan.py).
 *   unique_rows    retained[0 .. *n_retained): row j is dropped iff an earlier row is byte-identical to it in every matrix (32-bit
 *                  patterns: -0.0 != 0.0, NaN payloads count) -- what `_dependenceUniqueRows` keeps.
 *   window_scores  for every full window of window_bins bins of every matrix that holds one, in matrix order: count[w] = the rows
 *                  with a finite count > 0 and finiteCount / window_bins >= rank_coverage_min, score[w] = np.median of their
 *                  window_bins / finiteCount * np.sum(np.maximum(v[finite], 0)) (NaN for count 0).  Bit for bit (pyx:3664-3703).
 *   window_acf     `_dependenceFinitePairWindow` (pyx:2916-3148) of the retained rows of every listed window (win_mat / win_chain:
 *                  index into the matrices / the chain list; win_start: first bin).  Up to the centred values every number equals
 *                  the reference's bit for bit; the lag sums are compensated dot products in index order, about an ulp from the
 *                  exact sums (the reference takes them from an FFT).  rec[w]: the decisions of the window; pooled[w][max_lag_bins]:
 *                  its pooled ACF (NaN from the support cap on).  margin: the smallest |smoothed ACF - acf_threshold| over the lags
 *                  the persistence scan examined -- a window whose margin is within the FFT's error is decided by the caller.
 * At most 4096 rows.  The order statistics behind the clip order -0.0 in front of +0.0 (NumPy: equal): a clip bound, and through it
 * a centred value, may differ from the reference's in the sign of a zero, in nothing else. */
typedef struct csr_depspan_cfg {
    int64_t window_bins;
    int32_t max_lag_bins, smoothing_bins, persistence_bins, min_finite_pairs;
    double acf_threshold, min_finite_pair_coverage;
} csr_depspan_cfg;
enum { CSR_DEPSPAN_TINY_LAG_ZERO = 1 };     /* flags: a row's lag-zero covariance lies in the underflow range */
typedef struct csr_depspan_window {
    int32_t status;                 /* 0: the reference answers None; 1: a result */
    int32_t crossing_lag;           /* -1: right-censored */
    int32_t support_cap_lag, last_crossing_start, valid_rows, valid_rows_at_crossing;
    int32_t flags, reserved;
    double finite_pair_min, finite_pair_coverage_min;
    double revival;                 /* max |pooled ACF| from crossing_lag + persistence_bins - 1 on (NaN: none) */
    double margin;
} csr_depspan_window;
int csr_depspan_unique_rows(int32_t n_mats, const int64_t *n_bins, const float *const *mats, int64_t n_rows, int32_t *retained,
                            int32_t *n_retained);
int csr_depspan_window_scores(int32_t n_mats, const int64_t *n_bins, const float *const *mats, int64_t n_rows_total, int32_t n_rows,
                              const int32_t *rows, int64_t window_bins, double rank_coverage_min, double *score, int64_t *count);
int csr_depspan_window_acf(int32_t n_mats, const int64_t *n_bins, const float *const *mats, int64_t n_rows_total, int32_t n_rows,
                           const int32_t *rows, const csr_depspan_cfg *cfg, int64_t n_windows, const int32_t *win_mat,
                           const int64_t *win_start, csr_depspan_window *rec, double *pooled);
int csr_batch_depspan_unique_rows(csr_ctx *ctx, int32_t n_listed, const int32_t *chains, int32_t *retained, int32_t *n_retained);
int csr_batch_depspan_window_scores(csr_ctx *ctx, int32_t n_listed, const int32_t *chains, int32_t n_rows, const int32_t *rows,
                                    int64_t window_bins, double rank_coverage_min, double *score, int64_t *count);
int csr_batch_depspan_window_acf(csr_ctx *ctx, int32_t n_listed, const int32_t *chains, int32_t n_rows, const int32_t *rows,
                                 const csr_depspan_cfg *cfg, int64_t n_windows, const int32_t *win_chain, const int64_t *win_start,
                                 csr_depspan_window *rec, double *pooled);

/* ---- post-fit empirical-Bayes state shrinkage ------------------------------------------------------------ */
/* The per-bin passes of the reference's spike-and-slab state shrinkage (pyx:9791-10269 `cstateShrinkInitialSums`,
 * `cstateShrinkMixtureEMStepPrepared`, `cstateShrinkMixturePosteriorPrepared`).  The EM control flow around them is scalar work
 * of the caller (consenrich_amd/shrink.py); a call here evaluates one pass for one parameter set.
 *
 * An input is prepared once per (input, block size): csr_shrink_stage takes host arrays (float64 state and variance, the chunks
 * one after the other, n_chunks lengths) into the default context; csr_batch_shrink_prepare takes the chains chain_mask selects
 * (NULL: all) of a resident smoothed fit -- the state is (double) xs[:,0] of the reference-layout copy (the conversion and the
 * side-effect rule of csr_batch_rocco_scores: no array of the fit changes), the float32 variance track is made on the device from
 * (float) sqrt(Ps00) squared and floored at 1e-12 in float32, or the same way from `uncertainty`: the float32 uncertainty tracks
 * of the taken chains one after the other.  Blocks of `block` bins restart at every chunk / chain.
 *
 * The sum passes (ctx NULL: the staged host arrays) return one record per chunk / chain, which the caller adds in order as the
 * reference adds its chunks; records of chains the prepared input does not hold stay untouched.
 *   initial sums   out[chain][5]: totalWeight, centralWeight, excessMomentSum, varianceSum, finiteCount;
 *   EM step        out[chain][4 + 2 K]: totalWeight, nullMass, logLikelihood, finiteCount, slabMass[K], slabSecond[K];
 * finiteCount is an exact integer.  The sums are float64 trees of a fixed shape (csr_shrink.h): two identical calls return
 * identical bits; against the reference's sequential sums they agree to rounding, not bit for bit.
 * The posterior pass writes five float32 tracks: for the staged host arrays into out[5][total bins] (shrunk, posterior sd, spike
 * probability, slab mean, slab weight); for a batch into resident per-chain tracks (the two slab tracks with want_slab), which
 * csr_batch_shrink_download hands out (which: CSR_SHRINK_*; a chain without the track: "chain i has no shrunk track").
 * csr_batch_shrink_medians: count[chain] = the valid bins, mid[chain][4][2] = the lower and upper middle value over the valid
 * bins of |state|, |shrunk|, spike probability and posterior sd (equal for an odd count, untouched for none).
 * Checked before any launch: K in 1..96, finite positive tau (CSR_ERR_VALUE with the reference's text), 0 < pi0 < 1 (the same),
 * block >= 1.  Additive to ABI 6. */
enum { CSR_SHRINK_SHRUNK = 0, CSR_SHRINK_POSTERIOR_SD = 1, CSR_SHRINK_SPIKE_PROP = 2, CSR_SHRINK_SLAB_MEAN = 3,
       CSR_SHRINK_SLAB_WEIGHT = 4, CSR_SHRINK_VARIANCE = 5 };
#define CSR_SHRINK_MAX_SLABS 96
/* csr_batch_format_bedgraph, csr_batch_bigwig_sections and csr_batch_bigwig_zoom take CSR_ARR_SHRINK_BASE + CSR_SHRINK_* as
 * array_id (component 0): the chain's resident shrinkage track, written without a download. */
#define CSR_ARR_SHRINK_BASE 64
int csr_shrink_stage(int32_t n_chunks, const int64_t *lens, const double *state, const double *variance, int64_t block);
int csr_batch_shrink_prepare(csr_ctx *ctx, const unsigned char *chain_mask, const float *uncertainty, int64_t block);
int csr_shrink_initial_sums(csr_ctx *ctx, double null_z, double *out);
int csr_shrink_em_step(csr_ctx *ctx, double pi0, int32_t n_slabs, const double *tau, const double *log_slab_prior, double *out);
int csr_shrink_posterior(double pi0, int32_t n_slabs, const double *tau, const double *log_slab_prior, float *out);
int csr_batch_shrink_posterior(csr_ctx *ctx, double pi0, int32_t n_slabs, const double *tau, const double *log_slab_prior,
                               int32_t want_slab);
int csr_batch_shrink_download(csr_ctx *ctx, int32_t chain, int32_t which, float *host_dst);
int csr_batch_shrink_medians(csr_ctx *ctx, int64_t *count, double *mid);
/* Which resident track csr_batch_export_peaks and csr_batch_broad_rows read as signal from now on: CSR_SIGNAL_STATE, the
 * (double) xs[:,0] of the smoothed fit (the default; csr_batch_configure puts it back), or CSR_SIGNAL_SHRUNK, the shrunk state
 * track (float32 -- it carries a NaN / Inf of the state through).  With the shrunk signal a taken chain without the track fails
 * with "chain i has no shrunk track" before any launch.  Scores, masks and uncertainty are read as before. */
enum { CSR_SIGNAL_STATE = 0, CSR_SIGNAL_SHRUNK = 1 };
int csr_batch_set_export_signal(csr_ctx *ctx, int32_t signal);

/* ---------------------------------------------------------------------------------------------------------------
 * Dense observation-variance ("munc") seed natives: `cMuncObservationMomentSeedPass` (pyx:4843-5351) and
 * `cMuncSmoothDenseLocalEvidence` (pyx:5577-5741), and the per-cell glue of the seed loop (consenrich.py:7482-7576, 7938-7945),
 * on host arrays (default context) and on arrays that stay resident with a batch between the loop's rounds.  Every output
 * element equals the reference's bit for bit.  Invalid cells and parameters return CSR_ERR_VALUE with the reference's text.
 * use_weights is the reference's `enabled and useSeedWeights`.  Masks: mode 0 none, 1 per interval (n bytes), 2 per cell
 * ((m, n) bytes); a nonzero byte means ACTIVE in the seed pass and EXCLUDED in the rolling mean, as in the reference.
 * --------------------------------------------------------------------------------------------------------------- */
typedef struct csr_munc_seed_cfg {
    double pad, student_t_df, d_omega, omega_min, omega_max, variance_floor, variance_cap;
    int32_t use_weights, student_t, update_weights, reserved_;
} csr_munc_seed_cfg;
typedef struct csr_munc_seed_stats {
    int64_t passes;                     /* resident seed passes since csr_batch_munc_seed_begin */
    int64_t rolls;                      /* rolling means since then ... */
    int64_t roll_rows;                  /* ... the rows they smoothed ... */
    int64_t roll_fallback_rows;         /* ... and those of them redone whole (one wavefront per row) after an inexact running-sum operation */
    int64_t last_roll_fallback_rows;    /* the same count of the last rolling mean alone */
} csr_munc_seed_stats;
/* (m, n) float32 arrays; background / g_variance / count_floor / omega_in / rho_in / active may be NULL (rho_in NULL = ones).
 * All six outputs are written: moment, rho_out, local, variance (m, n); omega_raw, omega_out (n). */
int csr_munc_seed_pass(int64_t m, int64_t n, const float *data, const float *munc, const float *state_mean,
                       const float *state_variance, const float *background, const float *g_variance, const float *count_floor,
                       const float *omega_in, const float *rho_in, const unsigned char *active, int32_t active_mode,
                       const csr_munc_seed_cfg *cfg, float *moment, float *rho_out, float *omega_raw, float *omega_out, float *local,
                       float *variance);
/* out (m, n); fallback_rows (may be NULL): rows redone whole, a wavefront per row, because an add or subtract of their running sum was inexact */
int csr_munc_smooth_local(int64_t m, int64_t n, const float *local, int64_t window, const unsigned char *exclude,
                          int32_t exclude_mode, double eps, float *out, int64_t *fallback_rows);
/* The arrays of the seed loop, resident in the batch's layout and freed with the batch.  total / rho / omega have a current and
 * a "next" copy: csr_batch_munc_seed_pass reads the current ones and writes the next ones, csr_batch_munc_seed_swap makes the
 * next ones current.  LOCAL is the pointwise local evidence a pass leaves, SMOOTH its rolling mean, WEIGHT the response weight
 * (both from csr_batch_munc_seed_finish).  G / GVAR: the seed background and its variance (zero unless uploaded). */
enum {
    CSR_MUNC_SEED_TOTAL = 0, CSR_MUNC_SEED_LOCAL, CSR_MUNC_SEED_RHO, CSR_MUNC_SEED_OMEGA, CSR_MUNC_SEED_G, CSR_MUNC_SEED_GVAR,
    CSR_MUNC_SEED_WEIGHT, CSR_MUNC_SEED_COUNT_FLOOR, CSR_MUNC_SEED_EXCLUDE, CSR_MUNC_SEED_SMOOTH, CSR_MUNC_SEED_TOTAL_NEXT,
    CSR_MUNC_SEED_RHO_NEXT, CSR_MUNC_SEED_OMEGA_NEXT,
    CSR_MUNC_SEED_PRIOR,        /* (n) float32: the prior variance track (csr_batch_munc_prior_track, or uploaded); zero before */
    CSR_MUNC_SEED_TRACK_FLOOR   /* (m, n) float32: the caller's RAW count floor, NaN = missing, for csr_batch_munc_track_finish */
};
/* total := the batch's resident munc, omega = rho = 1, everything else 0; chain_mask (n_chains bytes or NULL = all): the chains
 * the loop takes.  use_count_floor / use_exclude: the pass reads COUNT_FLOOR, the rolling mean reads EXCLUDE (per interval). */
int csr_batch_munc_seed_begin(csr_ctx *ctx, const unsigned char *chain_mask, int32_t use_count_floor, int32_t use_exclude);
/* one chain's part of a seed array: (m, n) float32, (n) float32 for OMEGA* / G / GVAR, (n) bytes for EXCLUDE */
int csr_batch_munc_seed_upload(csr_ctx *ctx, int32_t chain, int32_t array_id, const void *host_src);
int csr_batch_munc_seed_download(csr_ctx *ctx, int32_t chain, int32_t array_id, void *host_dst);
/* `_seedWorkingMunc` of the current total / omega / rho / GVAR into the batch's own munc (the next pass of the fit reads it) */
int csr_batch_munc_seed_working(csr_ctx *ctx, double pad, int32_t use_weights);
/* the seed pass on the batch's data, the current total as munc and the resident smoothed fit (xs[:,0], max(Ps[:,0,0], 0)) */
int csr_batch_munc_seed_pass(csr_ctx *ctx, const csr_munc_seed_cfg *cfg);    /* (moment and omegaRaw, log-only in the loop, are never written: no switches are offered) */
int csr_batch_munc_seed_swap(csr_ctx *ctx, int32_t refill_weights);
/* SMOOTH := rolling mean of LOCAL; TOTAL := min(SMOOTH + COUNT_FLOOR, cap) floored at 1e-12 in float32 (cap <= 0: none);
 * WEIGHT := RHO_NEXT * OMEGA_NEXT (use_weights 0: ones) */
int csr_batch_munc_seed_finish(csr_ctx *ctx, int64_t window, double eps, double cap, int32_t use_weights);
int csr_batch_munc_seed_stats(csr_ctx *ctx, csr_munc_seed_stats *out);
/* `_updateSeedBackground` (consenrich.py:7688-7777) after a seed pass and before the swap: csr_batch_background_update with the
 * seed's per-cell weights (float32 of omega * rho / max(total + pad, 1e-12) of the CURRENT total / omega / rho; use_weights 0:
 * 1 / max(total + pad, 1e-12)) and the residual data - level of the resident fit; cfg->use_initial and use_lambda are ignored.
 * g_mode 0 ("disabled"): G = 0; 1 ("proxy"): the diagonal proxy clipped to [0, q99 of the chain's total] (the total's cells ordered
 * like their values, negative ones and infinities included; NaN cells are not NumPy's quantile).  out: n_chains records;
 * a status of 2..4 on a chain of the loop leaves every seed array as it was.  On success G / GVAR hold the new pair and the
 * batch's current background (what the next forward / backward pass subtracts) is the new g for the loop's chains. */
int csr_batch_munc_seed_background(csr_ctx *ctx, const csr_bg_cfg *cfg, double pad, int32_t use_weights, int32_t g_mode, csr_bg_out *out);
/* the last update's float64 weight / rhs tracks of one chain and the float64 sums of the float64 weights (any may be NULL) */
int csr_batch_munc_seed_background_tracks(csr_ctx *ctx, int32_t chain, double *weight, double *rhs, double *weight64);

/* ---------------------------------------------------------------------------------------------------------------
 * Finished observation-variance tracks: what lies between csr_batch_munc_seed_finish and a finished matrixMunc, per cell.
 *   block summaries   consenrich.py:7981-8040: per (sample, block) the count of valid cells and np.sum of q, q * predictor,
 *                     q * evidence and q * q over them (NumPy's order), per block the non-excluded intervals
 *   prior track       `cEvalPSplineLogVarianceTrend` (pyx:5761-5894) on the predictor sign(x) log1p(|x|) of a mean track
 *   finalisation      `cFinalizeMuncEBTrack` (pyx:5364-5544) as `getMuncTrack` (core.py:8390-8880) chains it, then
 *                     `applyBlacklistMuncFloor` (core.py:7183-7222) and the clamp of consenrich.py:9100-9113
 * Everything equals the reference bit for bit except what passes through log1p (sum q * predictor) and exp (the prior track).
 * The P-spline is data: knots (n_knots), beta (n_basis), degree, x_min, x_max.  degree < 0, n_knots = 0 or n_basis = 0 is the
 * reference's constant fallback (evaluated on the host with the C library's exp).  Otherwise degree <= 5, n_basis <= 512,
 * n_basis >= degree + 1 and n_knots >= n_basis + degree + 1 (the reference reads past its arrays where the last two fail), else
 * CSR_ERR_VALUE.
 * --------------------------------------------------------------------------------------------------------------- */
typedef struct csr_munc_block_rec {
    int64_t valid;              /* cells of the block that pass `validResponse` */
    double q, qp, qe, qq;       /* np.sum over them of q, q * predictor, q * evidence, q * q */
} csr_munc_block_rec;
typedef struct csr_munc_track_prm {     /* one per track */
    double nu_local, nu_prior, posterior;   /* posterior: filled by the library (nu_local + nu_prior) */
    double factor;                          /* replicate variance factor */
    int32_t scale, reserved_;               /* filled by the library: |factor - 1| > 1e-8 */
} csr_munc_track_prm;
typedef struct csr_munc_track_out {     /* one per (chain, track) */
    int64_t invalid_local, invalid_prior, invalid_count_floor;     /* the lowest invalid index of each kind, -1: none */
    int64_t support, floor_finite, floor_added, floor_missing;     /* the native's counters */
    double blacklist_floor;                                         /* the track's blacklist floor (the base floor where none applies) */
} csr_munc_track_out;
/* host arrays (default context).  evidence / weight: C-order (m, n) float32; exclude: n bytes or NULL; mean: n float64 (the
 * predictor is taken of it); recs: (m, blocks) records, included: blocks, with blocks as for the resident form below */
int csr_munc_block_sums(int64_t m, int64_t n, const float *evidence, const float *weight, const unsigned char *exclude,
                        const double *mean, int64_t block_intervals, csr_munc_block_rec *recs, int64_t *included);
/* out (n) float32 */
int csr_munc_eval_pspline(int64_t n, const double *predictor, const double *knots, int64_t n_knots, const double *beta,
                          int64_t n_basis, int32_t degree, double x_min, double x_max, double log_floor, double log_cap, float *out);
/* one track of n intervals; prior / count_floor may be NULL (use_eb 0 / no floor: NaN = missing, pyx:5423-5438);
 * prm->nu_local / nu_prior are read with use_eb.  out (n) float32 and the counters are valid where no index of *res is >= 0 */
int csr_munc_finalize_track(int64_t n, const float *local, const float *prior, const float *count_floor,
                            const csr_munc_track_prm *prm, double floor, double cap, int32_t use_eb, float *out,
                            csr_munc_track_out *res);
/* `applyBlacklistMuncFloor` with a non-negative base floor on a C-order (m, n) float32 matrix, in place; mask: n bytes;
 * floors: m float64.  The quantile of a row is np.quantile's on a float32 row (NumPy 2: float32 index arithmetic and lerp) */
int csr_munc_blacklist_floor(int64_t m, int64_t n, float *munc, const unsigned char *mask, double base_floor, double quantile,
                             double *floors);
/* Resident forms, after csr_batch_munc_seed_finish.  chain_mask: n_chains bytes or NULL = the chains of the seed loop; a chain
 * outside the seed loop is an error.  Blocks: max(2, block_intervals) intervals (at most 2048), a last block shorter than 2 is
 * dropped.  recs: per taken chain, in order, (m, blocks of the chain) records; included: per taken chain its blocks; n_recs /
 * n_blocks: the sizes the caller computed (checked).  Reads SMOOTH, WEIGHT, EXCLUDE and xs[:,0] of the resident smoothed fit,
 * which must still be resident (an error before any launch otherwise). */
int csr_batch_munc_block_sums(csr_ctx *ctx, int64_t block_intervals, const unsigned char *chain_mask, csr_munc_block_rec *recs,
                              int64_t n_recs, int64_t *included, int64_t n_blocks);
/* PRIOR := the trend on the predictor of xs[:,0] of the resident smoothed fit, for the taken chains */
int csr_batch_munc_prior_track(csr_ctx *ctx, const unsigned char *chain_mask, const double *knots, int64_t n_knots,
                               const double *beta, int64_t n_basis, int32_t degree, double x_min, double x_max, double log_floor,
                               double log_cap);
/* Per (track, interval) of the taken chains: local = SMOOTH, prior = PRIOR (scaled by the track's factor), the native's
 * shrinkage with prm[track], the count floor TRACK_FLOOR (use_count_floor; `_coerceMuncCountModelVarianceFloor`: not finite =
 * missing, negative = invalid), then the blacklist floor of the seed loop's EXCLUDE mask (base_floor, quantile; skipped without
 * a mask) and the clamp to [float32(clamp_lo), float32(clamp_hi)] (clamp_hi <= 0: no upper clamp).  out: (taken chains, m)
 * records; non_finite: per taken chain.  Where a record has an invalid index, or non_finite is not zero, NOTHING of the batch
 * has changed and the caller raises the reference's error.  Otherwise the result is the batch's own munc for the taken chains
 * (as after csr_batch_munc_seed_working: the resident fit results are dropped). */
int csr_batch_munc_track_finish(csr_ctx *ctx, const unsigned char *chain_mask, csr_munc_track_prm *prm, double floor, double cap,
                                int32_t use_eb, int32_t use_count_floor, double base_floor, double quantile, double clamp_lo,
                                double clamp_hi, csr_munc_track_out *out, int64_t *non_finite);

typedef struct csr_run_stats {
    int64_t blocks;             /* speculative blocks in the batch */
    int64_t fix_launches;       /* validation/fix-up kernel launches so far */
    int64_t reruns_p, reruns_x, reruns_b;  /* blocks re-run because the speculative carry-in was not bit-equal */
    int32_t block_len, warm_p, warm_x, warm_b;
    int32_t x_tol_ulps;
    int32_t pipeline_redos;     /* optimistic (deferred) validations that failed and re-ran their pipeline synchronously */
    int64_t local_repairs;      /* blocks a warm-started ECM sweep validated against their neighbour INSIDE the speculative
                                   kernel, found wanting and re-ran there (as of the last read-back) */
    int32_t ws_warm_f, ws_warm_b;   /* windows (bins) of the warm-started ECM sweeps, forward / smoother */
    int64_t sb_bailouts;        /* bit-exact state chain: single launches (k_sb_async) that gave up on a bounded wait; the pass
                                   form then ran instead (same results) */
    int64_t tail_groups;        /* bit-exact steps: groups of chains whose smoother / residuals were launched on their own (the
                                   first ones while the state chain of the other chains was still running) */
    int64_t nat_first_use_off_main; /* reference-layout arrays whose first use (allocation + zeroing) happened while a tail group's
                                   stream was current; harmless since ABI 4 (the zeroing is waited for on the host before the
                                   array is handed out) -- counted so that a test can show the path was exercised */
} csr_run_stats;
int csr_get_run_stats(csr_ctx *ctx, csr_run_stats *out);

#ifdef __cplusplus
}
#endif
#endif
