"""Device-resident multi-chain batch: the genome-level driver above the C ABI (include/consenrich_amd.h, level 2).

The reference processes chromosomes sequentially (consenrich.py:8809); here every chain of a rank is packed into one
batch so a single launch covers ~10^4-10^5 speculative blocks.  Inputs stay in HBM across sweeps.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib as L


@dataclass
class ModelParams:
    """Estimator parameters that reach the hot path (defaults: reference constants.py:140-153, 247-249)."""
    state_dim: int = 2
    F: tuple = ((1.0, 1.0), (0.0, 1.0))
    Q0: tuple = ((1.0e-3, 0.0), (0.0, 1.0e-4))
    state_init: float = 0.0
    state_covar_init: float = 1000.0
    pad: float = 1.0e-4
    lambda_bounds: tuple = (0.25, 4.0)
    kappa_bounds: tuple = (5.0e-3, 5.0e3)
    apn: tuple = (1.0e-4, 1000.0, 5.0, 10.0, 2.0)

    def to_c(self) -> L.Model:
        f32 = lambda v: float(np.float32(v))  # noqa: E731
        mdl = L.Model()
        mdl.state_dim = int(self.state_dim)
        F = np.asarray(self.F, np.float32)
        Q = np.asarray(self.Q0, np.float32)
        mdl.F[:] = [float(F[0, 0]), float(F[0, 1]), float(F[1, 0]), float(F[1, 1])]
        mdl.Q0[:] = [float(Q[0, 0]), float(Q[0, 1]), float(Q[1, 0]), float(Q[1, 1])]
        mdl.state_init, mdl.state_covar_init, mdl.pad = f32(self.state_init), f32(self.state_covar_init), f32(self.pad)
        mdl.w_min, mdl.w_max = f32(self.lambda_bounds[0]), f32(self.lambda_bounds[1])
        mdl.k_min, mdl.k_max = f32(self.kappa_bounds[0]), f32(self.kappa_bounds[1])
        mdl.apn_min_q, mdl.apn_max_q, mdl.apn_thresh, mdl.apn_scale, mdl.apn_pc = (f32(v) for v in self.apn)
        return mdl


_ARR = {"D": L.ARR_D, "xf": L.ARR_XF, "Pf": L.ARR_PF, "pnoise": L.ARR_PNOISE, "xs": L.ARR_XS, "Ps": L.ARR_PS,
        "lag": L.ARR_LAG, "resid": L.ARR_RESID, "lambda": L.ARR_LAMBDA, "kappa": L.ARR_KAPPA, "qscale": L.ARR_QSCALE,
        "sumGain0": L.ARR_SUMGAIN0, "sumGain1": L.ARR_SUMGAIN1, "effectiveQLevel": L.ARR_EFFQ_LEVEL,
        "effectiveQTrend": L.ARR_EFFQ_TREND, "muncTrace": L.ARR_MUNCTRACE, "background": L.ARR_BACKGROUND,
        "background_next": L.ARR_BACKGROUND_NEXT}
# what the writers take besides: the resident shrinkage tracks of a chain (shrink_apply), by these names
_WRITER_ARR = dict(_ARR, shrunk=L.ARR_SHRINK_BASE + L.SHRINK_TRACKS["shrunk"],
                   shrunk_posterior_sd=L.ARR_SHRINK_BASE + L.SHRINK_TRACKS["posterior_sd"],
                   shrunk_spike_prop=L.ARR_SHRINK_BASE + L.SHRINK_TRACKS["spike_prop"])


class _NestedBackend:
    """What consenrich_amd.nested.refine_chains needs of a batch: its resident scores and solution masks."""

    def __init__(self, batch):
        self.batch, self.lens = batch, np.asarray(batch.chain_lens, np.int64)
        self._lib, self._ctx = batch._lib, batch._ctx

    def initial_runs(self, chain):
        return self.batch.rocco_runs(chain, 0)

    def nodes(self, regions):
        from . import nested as N

        out = np.zeros(regions.size, N.NODE)
        L.check_value(self._lib.csr_batch_nested_nodes(self._ctx, regions.size, N._vp(regions), N._vp(out)))
        return out

    def layer(self, cfg, take, regions):
        from . import nested as N

        rec, count = np.zeros(regions.size, N.REC), C.c_int64(0)
        L.check_value(self._lib.csr_batch_nested_layer(self._ctx, N._vp(cfg), bytes(bytearray(int(t) for t in take)), regions.size,
                                                       N._vp(regions), N._vp(rec), C.byref(count)))
        kids = np.zeros(int(count.value), N.NODE)
        L.check(self._lib.csr_nested_children(self._ctx, kids.size, N._vp(kids)))
        return rec, kids

    def selected_sums(self, take, n_runs, starts, ends):
        out = np.zeros(len(self.lens), np.float64)
        L.check_value(self._lib.csr_batch_nested_selected_sum(self._ctx, bytes(bytearray(int(t) for t in take)),
                                                              n_runs.ctypes.data_as(L.I64P), starts.ctypes.data_as(L.I64P),
                                                              ends.ctypes.data_as(L.I64P), L.dp(out)))
        return out


class DeviceBatch:
    """One GPU, many chains.  Thin, explicit wrapper: every method is one C-ABI call.

    `x_tol_ulps`: carry validation of the forward state chain (csr_set_validation).  None / 0 = the default, bit-exact
    sequential semantics; 2 = the opt-in throughput mode (a few float32 ulps per pass; not a contract through an ECM loop)."""

    def __init__(self, device: int = 0, block_len: int = 0, warm=(-1, -1, -1), x_tol_ulps=None):
        L.require_gpu()
        self._lib = L.lib()
        self._ctx = self._lib.csr_create(int(device))
        if not self._ctx:
            raise L.ConsenrichAMDError(L.last_error())
        L.check(self._lib.csr_set_tuning(self._ctx, int(block_len), int(warm[0]), int(warm[1]), int(warm[2])))
        if x_tol_ulps is not None:
            L.check(self._lib.csr_set_validation(self._ctx, int(x_tol_ulps)))
        self.chain_lens = []
        self.m = 0
        self.d = 2
        self._comms = []
        self._rocco_count = {}      # selected bins per chain of the last rocco() (an upper bound of its runs)
        self._broad_parents = {}    # merged runs per chain of the last broad_parents()
        self.broad_stats = None
        self._null = {}             # chain -> (null centre, null scale) of the last rocco_null()

    def _attach_comm(self, comm):
        self._comms.append(comm)

    def _detach_comm(self, comm):
        if comm in self._comms:
            self._comms.remove(comm)

    def set_validation(self, x_tol_ulps: int):
        L.check(self._lib.csr_set_validation(self._ctx, int(x_tol_ulps)))

    def close(self):
        if self._ctx:
            for comm in list(getattr(self, "_comms", [])):      # a communicator holds the context's device and stream
                comm.close()
            self._lib.csr_destroy(self._ctx)
            self._ctx = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- setup ---------------------------------------------------------------------------------------------------
    def configure(self, model: ModelParams, m: int, chain_lens):
        lens = np.ascontiguousarray(chain_lens, dtype=np.int64)
        mdl = model.to_c()
        L.check(self._lib.csr_batch_configure(self._ctx, C.byref(mdl), int(m), int(lens.size),
                                              lens.ctypes.data_as(L.I64P)))
        self.chain_lens = [int(v) for v in lens]
        self.m, self.d = int(m), int(model.state_dim)
        self.model = model
        self._null = {}             # the templates died with the previous batch
        self._broad_parents = {}    # ... and so did the masks the parents were made of

    def set_model(self, model: ModelParams):
        mdl = model.to_c()
        L.check(self._lib.csr_batch_set_model(self._ctx, C.byref(mdl)))
        self.model = model

    def set_chain_q(self, q_list):
        """Per-chain base process noise: one (2,2) (or (1,1) for the level model) matrix per chain, values taken as
        float32 like the reference's matrixQ0; None = the model's Q0 for every chain again."""
        if q_list is None:
            L.check(self._lib.csr_batch_set_chain_q(self._ctx, None))
            return
        if len(q_list) != len(self.chain_lens):
            raise ValueError("one Q0 per chain")
        flat = np.zeros((len(q_list), 4))
        for i, q in enumerate(q_list):
            q = np.asarray(q, np.float32).astype(np.float64)
            if q.shape == (1, 1):
                flat[i, 0] = q[0, 0]
            elif q.shape == (2, 2):
                flat[i] = q.reshape(-1)
            else:
                raise ValueError("Q0 must be (2,2) or (1,1)")
        L.check(self._lib.csr_batch_set_chain_q(self._ctx, L.dp(flat)))

    def set_step_groups(self, tail_groups=None, epilogue_groups=None):
        """A test seam (csr_batch_set_step_groups): the early group of every chain of a pipelined step -- one index per chain, -1 =
        the remainder -- for its tails and for its NIS / NLL epilogues; None leaves that kind to the host's clock, both None clear
        the script.  It holds until cleared or until the batch is configured again.  A bad script raises ValueError and leaves
        the previous one in force."""
        arrs = [None if g is None else np.ascontiguousarray(g, np.int32) for g in (tail_groups, epilogue_groups)]
        for a in arrs:
            if a is not None and a.ndim != 1:
                raise ValueError("one group index per chain")
        sizes = {int(a.size) for a in arrs if a is not None}
        if len(sizes) > 1:
            raise ValueError("tail and epilogue groups of different lengths")
        ptrs = [None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32)) for a in arrs]
        L.check_value(self._lib.csr_batch_set_step_groups(self._ctx, ptrs[0], ptrs[1], sizes.pop() if sizes else 0))

    def set_tuning(self, block_len=0, warm_p=-1, warm_x=-1, warm_b=-1):
        L.check(self._lib.csr_set_tuning(self._ctx, int(block_len), int(warm_p), int(warm_x), int(warm_b)))

    def upload(self, chain: int, data: np.ndarray, munc: np.ndarray):
        data = np.ascontiguousarray(data, np.float32)
        munc = np.ascontiguousarray(munc, np.float32)
        if data.shape != (self.m, self.chain_lens[chain]) or munc.shape != data.shape:
            raise ValueError("data/munc must have shape (m, chain_len)")
        L.check(self._lib.csr_batch_upload(self._ctx, chain, L.fp(data), L.fp(munc)))

    def upload_multipliers(self, chain: int, lam=None, kappa=None, qscale=None):
        arrs = [None if a is None else np.ascontiguousarray(a, np.float32) for a in (lam, kappa, qscale)]
        for a in arrs:
            if a is not None and a.shape != (self.chain_lens[chain],):
                raise ValueError("multiplier arrays must have shape (chain_len,)")
        L.check(self._lib.csr_batch_upload_multipliers(self._ctx, chain, *(L.fp(a) for a in arrs)))

    def synthesize(self, seed: int):
        L.check(self._lib.csr_batch_synthesize(self._ctx, int(seed)))

    def download_inputs(self, chain: int):
        """(data, munc) of one chain as resident on the device, (m, n) float32 each."""
        shape = (self.m, self.chain_lens[chain])
        data, munc = np.empty(shape, np.float32), np.empty(shape, np.float32)
        L.check(self._lib.csr_batch_download_inputs(self._ctx, int(chain), L.fp(data), L.fp(munc)))
        return data, munc

    # -- compute -------------------------------------------------------------------------------------------------
    def stats(self):
        L.check(self._lib.csr_batch_stats(self._ctx))

    def forward(self, flags: int = L.RETURN_NLL, want_sums: bool = True):
        nc = len(self.chain_lens)
        if not want_sums:
            L.check(self._lib.csr_batch_forward(self._ctx, int(flags), None, None))
            return None, None
        sd, sn = np.zeros(nc), np.zeros(nc)
        L.check(self._lib.csr_batch_forward(self._ctx, int(flags), L.dp(sd), L.dp(sn)))
        return sd, sn

    def backward(self):
        L.check(self._lib.csr_batch_backward(self._ctx))

    def forward_backward(self, flags: int = L.RETURN_NLL, want_sums: bool = True):
        """forward() + backward() as one pipeline (one host synchronisation; `_runForwardBackward`, core.py:4207)."""
        nc = len(self.chain_lens)
        if not want_sums:
            L.check(self._lib.csr_batch_forward_backward(self._ctx, int(flags), None, None))
            return None, None
        sd, sn = np.zeros(nc), np.zeros(nc)
        L.check(self._lib.csr_batch_forward_backward(self._ctx, int(flags), L.dp(sd), L.dp(sn)))
        return sd, sn

    def sums(self):
        """Per-chain (sumD, sumNLL) of the resident forward pass; synchronises (and validates) everything queued."""
        nc = len(self.chain_lens)
        sd, sn = np.zeros(nc), np.zeros(nc)
        L.check(self._lib.csr_batch_sums(self._ctx, L.dp(sd), L.dp(sn)))
        return sd, sn

    def ecm(self, max_iters=50, inner_iters=5, rtol=1.0e-6, nu=8.0, use_lambda=False, use_kappa=True,
            use_apn=False, use_qscale=False, chain_mask=None):
        """chain_mask: optional per-chain booleans; chains with False keep their resident results untouched."""
        nc = len(self.chain_lens)
        cfg = L.EcmCfg(int(max_iters), int(inner_iters), float(np.float32(rtol)), float(np.float32(nu)),
                       int(use_lambda), int(use_kappa), int(use_apn), 0)
        outs = (L.EcmOut * nc)()
        path = np.zeros(nc * max(int(max_iters), 1))
        mask = None if chain_mask is None else bytes(bytearray(int(bool(t)) for t in chain_mask))
        L.check(self._lib.csr_batch_ecm_masked(self._ctx, C.byref(cfg), L.USE_QSCALE if use_qscale else 0, mask, outs,
                                               L.dp(path)))
        return list(outs), path.reshape(nc, -1)

    def step(self, flags: int = L.RETURN_NLL, what: int = 0, want_sums: bool = True):
        """stats() + forward_backward(flags) + export(what) + sums() in one C-ABI call: same kernels, same results; in the
        bit-exact mode the tail of each chain (smoother, residuals) starts as soon as that chain's filtered state stands."""
        if not want_sums:
            L.check(self._lib.csr_batch_step(self._ctx, int(flags), int(what), None, None))
            return None, None
        nc = len(self.chain_lens)
        sd, sn = np.zeros(nc), np.zeros(nc)
        L.check(self._lib.csr_batch_step(self._ctx, int(flags), int(what), L.dp(sd), L.dp(sn)))
        return sd, sn

    def step_forward(self, flags: int = L.RETURN_NLL, what: int = L.EXPORT_FORWARD, want_sums: bool = True):
        """stats() + forward(flags) + export(what & EXPORT_FORWARD) + sums() in one C-ABI call: the forward filter alone
        (`cforwardPass` without `cbackwardPass`, pyx:6393-6632; BASELINE config 2)."""
        if not want_sums:
            L.check(self._lib.csr_batch_step_forward(self._ctx, int(flags), int(what), None, None))
            return None, None
        nc = len(self.chain_lens)
        sd, sn = np.zeros(nc), np.zeros(nc)
        L.check(self._lib.csr_batch_step_forward(self._ctx, int(flags), int(what), L.dp(sd), L.dp(sn)))
        return sd, sn

    def forward_masked(self, flags: int, chain_mask):
        """forward() for the chains with chain_mask[c] true only; returns (sum_d, sum_nll) (masked chains: stale)."""
        nc = len(self.chain_lens)
        sd, sn = np.zeros(nc), np.zeros(nc)
        mask = bytes(bytearray(int(bool(t)) for t in chain_mask))
        L.check(self._lib.csr_batch_forward_masked(self._ctx, int(flags), mask, L.dp(sd), L.dp(sn)))
        return sd, sn

    def phase_tracks(self, chain: int, pad: float, with_fit: bool = False, use_lambda: bool = False, out=None):
        """Per-bin float64 tracks of one chain behind the two per-phase diagnostics of `runConsenrich` that read the (m, n)
        matrices (csr_batch_phase_tracks): `rel` = smoothed level - weighted mean of the background-adjusted observations
        (core.py:2663-2697); with_fit (a background proposal is resident): `fit` = sum_j iv (r - proposal)^2 and `cnt` = its
        cell count (core.py:4546-4552, 4587-4596).  Returns (rel, fit or None, cnt or None)."""
        n = self.chain_lens[chain]
        if out is not None:                 # caller-owned (n,) float64 / float64 / int32 buffers (re-used: no first-touch faults)
            rel, fit, cnt = out[0], (out[1] if with_fit else None), (out[2] if with_fit else None)
            for a, t in ((rel, np.float64), (fit, np.float64), (cnt, np.int32)):
                if a is not None and (a.dtype != t or a.shape != (n,) or not a.flags.c_contiguous):
                    raise ValueError("phase_tracks: out buffers must be contiguous (n,) float64, float64, int32")
        else:
            rel = np.empty(n, np.float64)
            fit = np.empty(n, np.float64) if with_fit else None
            cnt = np.empty(n, np.int32) if with_fit else None
        L.check(self._lib.csr_batch_phase_tracks(self._ctx, int(chain), int(bool(use_lambda)), float(pad), L.dp(rel),
                                                 L.dp(fit) if with_fit else None,
                                                 cnt.ctypes.data_as(C.POINTER(C.c_int32)) if with_fit else None))
        return rel, fit, cnt

    def gain_summary(self, chain: int, pad: float, use_lambda: bool = False, lambda_bounds=(0.25, 4.0)) -> dict:
        """`_finalForwardReplicateGainContigSummary` (core.py:7671-7731) of one chain from the resident forward pass
        (csr_batch_gain_summary: moments and the six order statistics around the quartile positions per replicate, exact); the
        quartiles are interpolated here the way NumPy's 'linear' method does (np.median / np.quantile of the reference)."""
        out = np.empty((self.m, 9))
        L.check(self._lib.csr_batch_gain_summary(self._ctx, int(chain), int(bool(use_lambda)), float(pad), float(lambda_bounds[0]),
                                                 float(lambda_bounds[1]), L.dp(out)))
        cnt = out[:, 0].astype(np.int64)
        res = {"count": [int(v) for v in cnt], "mean": [], "median": [], "sd": [], "iqr": []}

        def lerp(a, b, t):          # numpy.lib._function_base_impl._lerp
            d = b - a
            v = a + d * t
            if t >= 0.5:
                v = b - d * (1.0 - t)
            return a if d == 0 else v

        for j in range(self.m):
            if cnt[j] == 0:
                for k in ("mean", "median", "sd", "iqr"):
                    res[k].append(float("nan"))
                continue
            q = []
            for i, frac in enumerate((0.25, 0.5, 0.75)):
                pos = (cnt[j] - 1) * frac
                t = pos - np.floor(pos)
                q.append(lerp(out[j, 3 + 2 * i], out[j, 4 + 2 * i], float(t)))
            lo, hi = out[j, 5], out[j, 6]
            res["mean"].append(float(out[j, 1]))
            res["median"].append(float(lo if cnt[j] % 2 else 0.5 * (lo + hi)))     # np.median: the mean of the two middle values
            res["sd"].append(float(out[j, 2]))
            res["iqr"].append(float(q[2] - q[0]))
        return res

    def objective_terms(self, nu: float, lam_first: float, lam: float, negative_penalty_multiplier=1.0, pad=1.0e-4,
                        use_lambda_penalty=False, use_kappa_penalty=True, use_lambda_weights=False, use_nonnegative=True):
        """Everything of the reference's penalised objective (core.py:4418-4538) except the forward NLL, per chain, from
        the resident variances / multipliers / current background; list of dicts."""
        nc = len(self.chain_lens)
        mult = float("nan") if negative_penalty_multiplier is None else float(negative_penalty_multiplier)
        cfg = L.ObjectiveCfg(float(nu), float(lam_first), float(lam), mult, float(pad), int(use_lambda_penalty),
                             int(use_kappa_penalty), int(use_lambda_weights), int(use_nonnegative))
        out = (L.ObjectiveTerms * nc)()
        L.check(self._lib.csr_batch_objective_terms(self._ctx, C.byref(cfg), out))
        return [{k: getattr(o, k) for k, _ in L.ObjectiveTerms._fields_} for o in out]

    def diagnostics(self, flags: int = 0):
        """Per-interval output diagnostics (core.py:7734-7878) of the resident forward pass; results are the arrays
        sumGain0, sumGain1, effectiveQLevel, effectiveQTrend, muncTrace (download()).  flags: USE_LAMBDA / USE_KAPPA /
        USE_QSCALE = which resident multipliers enter (None in the reference call otherwise)."""
        L.check(self._lib.csr_batch_diagnostics(self._ctx, int(flags)))

    # -- background update between ECM phases -----------------------------------------------------
    def background_update(self, lam_first: float, lam: float, zero_center=False, use_nonnegative=True,
                          negative_penalty_multiplier=1.0, use_lambda=False, use_initial=True, max_passes=5,
                          block_len=0, raise_on_error=True, zero_state=False):
        """core.py:5064-5137 + 8085-8378 for every chain, device-resident: weight / rhs tracks from the original data,
        munc and the smoothed level, conditioning guard, pentadiagonal solve with the asymmetric-IRLS wrapper.  The
        proposal is the array "background_next"; returns one dict per chain.  Errors the reference raises
        (pivot modification, float64 reliability, non-finite solution) raise RuntimeError here unless
        raise_on_error=False.  zero_state=True is the reference's background warm start from the weighted data
        (`_estimateBackgroundWarmStart`, core.py:2809-2910: residual = data, no fit needs to be resident)."""
        nc = len(self.chain_lens)
        cfg = L.BgCfg(float(lam_first), float(lam),
                      float("nan") if negative_penalty_multiplier is None else float(negative_penalty_multiplier),
                      int(bool(zero_center)), int(bool(use_nonnegative)), int(bool(use_lambda)),
                      (L.BG_INIT_FROM_CURRENT if use_initial else 0) | (L.BG_ZERO_STATE if zero_state else 0),
                      int(max_passes), int(block_len))
        outs = (L.BgOut * nc)()
        L.check(self._lib.csr_batch_background_update(self._ctx, C.byref(cfg), outs))
        res = [{k: getattr(o, k) for k, _ in L.BgOut._fields_} for o in outs]
        if raise_on_error:
            self._raise_background_errors(res)
        return res

    @staticmethod
    def _raise_background_errors(res, take=None):
        for c, o in enumerate(res):
            if take is not None and not take[c]:
                continue
            if o["status"] == L.BG_BAD_PIVOT:
                raise RuntimeError("roughness-penalized LDL factorization required pivot modification at index "
                                   f"{o['bad_index']} (pivot={o['bad_value']:.6g}, floor={1.0e-12:.6g}). [chain {c}]")
            if o["status"] == L.BG_UNRELIABLE:
                raise RuntimeError("roughness-penalized LDL system exceeds float64 reliability: "
                                   f"roundoffIndex={o['roundoff_index']:.6g} threshold=1 [chain {c}]")
            if o["status"] == L.BG_NONFINITE:
                raise RuntimeError(f"solver returned non-finite values [chain {c}]")

    def background_apply(self, take=None):
        """current background := last proposal (for the chains with take[c] true; default all)."""
        buf = None if take is None else bytes(bytearray(int(bool(t)) for t in take))
        L.check(self._lib.csr_batch_background_apply(self._ctx, buf))

    def set_background(self, chain: int, background=None):
        a = None if background is None else np.ascontiguousarray(background, np.float32)
        if a is not None and a.shape != (self.chain_lens[chain],):
            raise ValueError("background must have shape (chain_len,)")
        L.check(self._lib.csr_batch_set_background(self._ctx, chain, L.fp(a)))

    def bedgraph_bytes(self, chain: int, name: str, chrom: str, start0: int, step: int, end_cap: int = 0, comp: int = 0,
                       transform=None) -> bytes:
        """bedGraph text (consenrich.py:9797-9805 format) of component `comp` of an exported array of one chain,
        formatted on the device.  transform: None, "round4" (state track) or "sqrt" (uncertainty from a variance).  name may also
        be "shrunk", "shrunk_posterior_sd" or "shrunk_spike_prop": the chain's resident shrinkage track (`shrink_apply`), so
        that the reference's stateShrunk and stateShrunkUncertainty files are written without a download."""
        t = {None: 0, "none": 0, "round4": 1, "sqrt": 2}[transform]
        cn = str(chrom).encode("ascii")
        f = self._lib.csr_batch_format_bedgraph
        size = f(self._ctx, chain, _WRITER_ARR[name], comp, t, cn, int(start0), int(step), int(end_cap), None, 0)
        if size < 0:
            raise L.ConsenrichAMDError(L.last_error())
        if size == 0:
            return b""
        buf = C.create_string_buffer(int(size))
        if f(self._ctx, chain, _WRITER_ARR[name], comp, t, cn, int(start0), int(step), int(end_cap), buf, int(size)) != size:
            raise L.ConsenrichAMDError(L.last_error() or "bedGraph writer size mismatch")
        return buf.raw

    def bigwig_track(self, chain: int, name: str, chrom_id: int, start0: int, step: int, end_cap: int = 0, comp: int = 0,
                     transform=None, zoom_bases=()):
        """The fixed-record body of a bigWig file for component `comp` of an exported array of one chain, formatted on the
        device (io.py:530-790 is the reference's pyBigWig conversion of its bedGraph): data sections + total summary + one
        set of reduction records per entry of `zoom_bases` (bases per record, multiples of `step`).  Values = float32 of the
        "%.4f" text of the (transformed) track value, i.e. what the reference's file holds.  Returns a
        consenrich_amd.bigwig.TrackPiece for `bigwig.write_bigwig`."""
        from . import bigwig as BW

        t = {None: 0, "none": 0, "round4": 1, "sqrt": 2}[transform]
        f = self._lib.csr_batch_bigwig_sections
        args = (self._ctx, int(chain), _WRITER_ARR[name], int(comp), t, int(chrom_id), int(start0), int(step), int(end_cap))
        size = f(*args, BW.ITEMS_PER_SECTION, None, 0, None)
        if size < 0:
            raise L.ConsenrichAMDError(L.last_error())
        buf = C.create_string_buffer(int(size))
        summ = L.BwSummary()
        if f(*args, BW.ITEMS_PER_SECTION, buf, int(size), C.byref(summ)) != size:
            raise L.ConsenrichAMDError(L.last_error() or "bigWig sections size mismatch")
        if summ.non_finite:
            raise ValueError(f"Non-finite bedGraph value in chain {chain} ({summ.non_finite} intervals)")     # io.py:713-716
        zooms = {}
        for zb in zoom_bases:
            if int(zb) % int(step):
                raise ValueError("zoom levels must be multiples of the interval step")
            g = self._lib.csr_batch_bigwig_zoom
            zsize = g(*args, int(zb) // int(step), None, 0)
            if zsize < 0:
                raise L.ConsenrichAMDError(L.last_error())
            zbuf = C.create_string_buffer(int(zsize))
            if g(*args, int(zb) // int(step), zbuf, int(zsize)) != zsize:
                raise L.ConsenrichAMDError(L.last_error() or "bigWig zoom size mismatch")
            zooms[int(zb)] = zbuf.raw
        return BW.TrackPiece(int(chrom_id), buf.raw, self.chain_lens[chain], int(summ.bases_covered), float(summ.min_val),
                             float(summ.max_val), float(summ.sum_data), float(summ.sum_squares), zooms)

    def make_fold(self, src: int, dst: int, block_len: int, fold: int, block_fold, reps_count, reps, pad: float,
                  rho: float = 0.0, masked_variance: float = 1.0e30):
        """Delete-block calibration fold as an extra chain (uncertainty.py:1370-1419, cuncertainty.pyx:160-305): chain `dst`
        receives chain `src`'s data and variances with the fold's deleted (replicate, block) cells masked; returns the
        (kept, heldout, h) information tracks.  Fit all chains afterwards (ecm / driver.fit_batch)."""
        n = self.chain_lens[src]
        bf = np.ascontiguousarray(block_fold, np.int32)
        rc = np.ascontiguousarray(reps_count, np.int64)
        rb = np.ascontiguousarray(reps, np.int64)
        kept, held, h = np.empty(n), np.empty(n), np.empty(n)
        L.check(self._lib.csr_batch_make_fold(self._ctx, int(src), int(dst), int(block_len), int(fold),
                                              bf.ctypes.data_as(C.POINTER(C.c_int32)), rc.ctypes.data_as(L.I64P),
                                              rb.ctypes.data_as(L.I64P), rb.shape[1], 0, float(pad), float(rho),
                                              float(masked_variance), L.dp(kept), L.dp(held), L.dp(h)))
        return kept, held, h

    def qseed(self, *, pad: float, stateModel: str = "levelTrend", minQ: float = 1.0e-6, maxQ: float = 1000.0,
              deltaF: float = 1.0, robustTNu=8.0, qSeedPriorLevel: float = 1.0e-5):
        """Initial process-noise seed of every chain (core.py:3621-3780 `_estimateInitialProcessNoiseFromData`) from the
        resident float32 data / variance matrices: list of (matrixQ float32 (2,2), diagnostics dict), one per chain."""
        from . import qseed as Q

        for name, v in (("minQ", minQ), ("minQ", qSeedPriorLevel)):
            if not np.isfinite(v) or v <= 0.0:
                raise ValueError(f"`{name}` must be positive and finite")
        cfg = Q.seed_config(pad=pad, stateModel=stateModel, minQ=minQ, maxQ=maxQ, deltaF=deltaF, robustTNu=robustTNu,
                            qSeedPriorLevel=qSeedPriorLevel)
        out = (L.QseedOut * len(self.chain_lens))()
        Q._call(self._lib.csr_batch_qseed(self._ctx, C.byref(cfg), out))
        return [Q.seed_result(o, float(minQ)) for o in out]

    # -- budgeted chain peak selection (ROCCO, consenrich_amd/rocco.py) ----------------------------------------------------
    def rocco_scores(self, mode: str = "state", z: float = 1.0):
        """Score track of every chain from the resident smoothed fit (`consenrichStateScoreTrack`, peaks.py:342-393), kept on
        the device: "state" = float64 of xs[:,0]; "lower_confidence" = xs0 - z * sqrt(Ps00) (float32 square root), floored at
        -2 max(xs0) when that is finite and positive.  Reads the fit, changes none of its arrays."""
        modes = {"state": L.ROCCO_SCORE_STATE, "lower_confidence": L.ROCCO_SCORE_LOWER_CONFIDENCE}
        if mode not in modes:
            raise ValueError("`uncertaintyScoreMode` must be 'state' or 'lower_confidence'")
        # (a negative variance or a bad z comes back as the reference's ValueError)
        L.check_value(self._lib.csr_batch_rocco_scores(self._ctx, modes[mode], float(z)))
        self._broad_parents.clear()     # (new scores drop the masks on the device: the parents made of the old ones go with them)

    def upload_scores(self, chain: int, scores):
        s = np.ascontiguousarray(np.asarray(scores, dtype=np.float64).ravel())
        if s.shape != (self.chain_lens[chain],):
            raise ValueError("scores must have shape (chain_len,)")
        if not np.all(np.isfinite(s)):
            raise ValueError("`scores` contains non-finite values")
        L.check(self._lib.csr_batch_upload_scores(self._ctx, int(chain), L.dp(s)))
        self._broad_parents.pop(int(chain), None)

    def download_scores(self, chain: int) -> np.ndarray:
        out = np.empty(self.chain_lens[chain], np.float64)
        L.check(self._lib.csr_batch_download_scores(self._ctx, int(chain), L.dp(out)))
        return out

    def rocco(self, budget=None, gamma=0.5, selection_penalty=None, max_iter=60, chains=None):
        """`csolveChromROCCOExact` (pyx:8877-8958) of the chains' resident scores in ONE call: all chains, and the penalties a
        calibration can visit next, run side by side.  budget / gamma / selection_penalty / max_iter: a scalar for every chain
        or one value per chain (None entries allowed: the reference's three modes).  chains: optional per-chain booleans;
        chains with False are not solved and keep their previous mask.  Returns one dict per chain (None where not solved)
        with the reference's tuple values: objective, penalized_objective, selected_count, selection_penalty; the mask stays
        on the device (rocco_solution / rocco_runs)."""
        return self._rocco_into(False, budget, gamma, selection_penalty, max_iter, chains)

    def _rocco_into(self, weak, budget, gamma, selection_penalty, max_iter, chains):
        """The body of `rocco` and `rocco_weak`: the strong or the weak solution track as destination"""
        from . import rocco as R

        nc = len(self.chain_lens)

        def per_chain(v):
            if isinstance(v, (list, tuple, np.ndarray)):
                if len(v) != nc:
                    raise ValueError("one value per chain")
                return list(v)
            return [v] * nc

        b, g, p, it = per_chain(budget), per_chain(gamma), per_chain(selection_penalty), per_chain(max_iter)
        take = [True] * nc if chains is None else [bool(t) for t in chains]
        if len(take) != nc:
            raise ValueError("one mask entry per chain")
        cfg = (L.RoccoCfg * nc)()
        for i in range(nc):
            if take[i]:
                cfg[i] = R.chrom_config(self.chain_lens[i], b[i], g[i], p[i], int(it[i]))
        out = (L.RoccoOut * nc)()
        mask = None if chains is None else bytes(bytearray(int(t) for t in take))
        L.check((self._lib.csr_batch_rocco_weak if weak else self._lib.csr_batch_rocco)(self._ctx, cfg, mask, out))
        for i in range(nc):
            if take[i] and not weak:
                self._rocco_count[i] = int(out[i].selected_count)
        return [None if not take[i] else
                {"objective": float(out[i].objective), "penalized_objective": float(out[i].penalized_objective),
                 "selected_count": int(out[i].selected_count), "selection_penalty": float(out[i].selection_penalty)}
                for i in range(nc)]

    def rocco_weak(self, budget=None, gamma=0.5, selection_penalty=None, max_iter=60, chains=None):
        """`rocco` with the WEAK solution track as destination (broad mode's second pass: the same scores, the weak budget, twice the
        gamma): same arguments and return.  The strong mask, its run counts and everything else resident stay untouched; the mask
        is read by `broad_parents` and served by `weak_solution`."""
        return self._rocco_into(True, budget, gamma, selection_penalty, max_iter, chains)

    def weak_solution(self, chain: int) -> np.ndarray:
        """The uint8 weak selection mask of one chain."""
        out = np.empty(self.chain_lens[chain], np.uint8)
        L.check(self._lib.csr_batch_rocco_weak_download(self._ctx, int(chain), out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    def upload_weak_solution(self, chain: int, solution):
        """Plants the weak selection mask of one chain (a host-decided one: `solveChromROCCO`'s fallback window)."""
        s = np.ascontiguousarray(np.asarray(solution).astype(np.uint8).ravel())
        if s.shape != (self.chain_lens[chain],):
            raise ValueError("solution must have shape (chain_len,)")
        L.check(self._lib.csr_batch_rocco_weak_upload(self._ctx, int(chain), s.ctypes.data_as(C.POINTER(C.c_uint8))))

    def broad_parents(self, thresholds, selection_penalties, boundary_costs, *, max_gap_bp, intervals=None, ends=None, interval_bp=None,
                      chroms=None, blacklist=None, dip_penalty_fraction=0.5, run_penalty=0.0, chains=None):
        """Broad mode's envelope and bridging (peaks.py:6884-6932 with `_mergeBroadRunsByObjective`, 1898-2005) of every chain's
        RESIDENT scores, strong mask (`rocco` / `rocco_nested`) and weak mask (`rocco_weak`), in one device call for all chains:
        the runs of scores >= threshold cut at coordinate breaks, those that touch weak | strong (where none does: the runs of
        weak | strong), and per kept run the NumPy-order sum of the dip-weighted excess of the bins up to the next one.  The host
        decides every gap on its own from the compact records: distance (max_gap_bp, a value or one per chain), blacklist (a
        dict of per-chromosome (k, 2) arrays), and the gain gapScore + 2 boundary_cost + run_penalty > 0.  thresholds /
        selection_penalties / boundary_costs: one value per chain or one for all (the weak pass's threshold, selection penalty
        and gamma).  Returns per chain (None where not taken) a dict: starts, ends (the merged runs), merge_details (the reference's
        dict, both forms), weak_support_threshold, weak_support_run_count, weak_support_touching_run_count, envelope_fallback,
        broad_bridge_dip_penalty_fraction.  The merged runs wait for `broadpeak_rows`; nothing resident changes."""
        from . import broad as B

        return B.batch_parents(self, thresholds, selection_penalties, boundary_costs, max_gap_bp=max_gap_bp, intervals=intervals,
                               ends=ends, interval_bp=interval_bp, chroms=chroms, blacklist=blacklist,
                               dip_penalty_fraction=dip_penalty_fraction, run_penalty=run_penalty, chains=chains)

    def broad_parent_solution(self, chain: int) -> np.ndarray:
        """The uint8 mask of one chain's bridged parents, as the last `broadpeak_rows` filled it."""
        out = np.empty(self.chain_lens[chain], np.uint8)
        L.check(self._lib.csr_batch_broad_parent_download(self._ctx, int(chain), out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    def broadpeak_rows(self, *, intervals=None, ends=None, interval_bp=None, chroms=None, prefix="consenrich", multiplier=2.0,
                       use_uncertainty=True, min_peak_bp=1000, chains=None, signal="state"):
        """The reference's broadPeak and gappedPeak rows (`_solutionToChromBroadPeakRows`, peaks.py:5606-5818) of the parents
        `broad_parents` left, with the chain's strong mask as child mask: one wavefront per parent makes np.median, the leftmost
        arg-max, np.max and np.mean of the signal, np.max and np.mean of the scores, np.median of the finite uncertainty values
        and the median filter's flag from the resident scores and the smoothed fit (signal float64 of xs[:,0], uncertainty the
        float32 square root of Ps00), and fills the resident parent mask (`broad_parent_solution`).  The host does the coordinate
        work from compact records (consenrich_amd/broad.py).  A chain with a non-finite signal or score value inside a parent has
        its parent numbers redone with NumPy on its downloaded tracks (`decided_on_host`).  Returns per chain (None where not
        taken) a dict: broad_rows, gapped_rows, peak_meta, export_details, decided_on_host; `broad_stats` holds the counts and
        seconds of the last `broad_parents` and `broadpeak_rows`.  signal: "state" (default) or "shrunk", as in
        `narrowpeak_rows`; the host fallback uses the same signal."""
        from . import broad as B

        with self._export_signal(signal):
            return B.batch_rows(self, intervals=intervals, ends=ends, interval_bp=interval_bp, chroms=chroms, prefix=prefix,
                                multiplier=multiplier, use_uncertainty=use_uncertainty, min_peak_bp=min_peak_bp, chains=chains,
                                signal=signal)

    def rocco_solution(self, chain: int) -> np.ndarray:
        """The uint8 selection mask of one chain."""
        out = np.empty(self.chain_lens[chain], np.uint8)
        L.check(self._lib.csr_batch_rocco_download(self._ctx, int(chain), out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    def rocco_runs(self, chain: int, max_gap_bins: int = 0):
        """`cBooleanRunBounds(solution, maxGapBins)` (pyx:9427-9457) of one chain's mask, computed on the device: (starts, ends)
        int64, inclusive bin indices -- a caller fetches the peaks, not n bytes."""
        # one call: a mask of k selected bins has at most k runs (a second call only beyond 65 536 runs)
        cap = max(1, min(self._rocco_count.get(int(chain), 4096), 1 << 16))
        cnt = C.c_int64(0)
        f = self._lib.csr_batch_rocco_runs
        for _ in range(2):
            starts, ends = np.empty(cap, np.int64), np.empty(cap, np.int64)
            L.check(f(self._ctx, int(chain), int(max_gap_bins), cap, C.byref(cnt), starts.ctypes.data_as(L.I64P),
                      ends.ctypes.data_as(L.I64P)))
            if int(cnt.value) <= cap:
                break
            cap = int(cnt.value)
        k = int(cnt.value)
        return starts[:k].copy(), ends[:k].copy()

    def rocco_nested(self, gammas, selection_penalties, *, iters=3, budget_scale=0.75, jaccard_threshold=0.999, intervals=None,
                     ends=None, min_region_bp=None, min_region_bins=5, chains=None):
        """`_refineNestedROCCOSolution` (peaks.py:3763-4388) of the chains' RESIDENT scores and solution masks, all chains layer
        by layer in the same calls.  gammas / selection_penalties: one value per chain (or one for all) -- the first pass's.
        intervals / ends: None (bin mode), or per chain the bins' start / end coordinates (host arrays; an entry may be None).
        The refined mask REPLACES the chain's resident solution: rocco_solution, rocco_runs, best_segment_scores and
        dwb_peak_scoring (which take a chain's runs) see it; segment_candidates reads the score tracks only and is unaffected.
        A minimum child run above 255 bins is refused with ValueError before any launch (with mixed bin widths by a bound:
        ceil(min_region_bp / the smallest positive width inside a first-pass run)), so the masks are never left partly refined.  chains: optional per-chain booleans; a chain with False keeps its mask.  The scores and the
        arrays of the fit are only read.  Returns the reference's `details` per chain (None where not taken).  The device does
        the per-region and per-node arithmetic; the hierarchy, the stop rule and the geometry are decided on the host from compact
        records (consenrich_amd/nested.py)."""
        from . import nested as N

        take, _ = self._chain_mask(chains)
        nc = len(take)

        def per_chain(v):
            if isinstance(v, (list, tuple, np.ndarray)):
                if len(v) != nc:
                    raise ValueError("one value per chain")
                return list(v)
            return [v] * nc

        g, p = per_chain(gammas), per_chain(selection_penalties)
        iv = [None] * nc if intervals is None else list(intervals)
        en = [None] * nc if ends is None else list(ends)
        if len(iv) != nc or len(en) != nc:
            raise ValueError("one intervals / ends entry per chain")
        state = [N._Chain(i, self.chain_lens[i], g[i], p[i], iters, budget_scale, jaccard_threshold, iv[i], en[i], min_region_bp,
                          min_region_bins) for i in range(nc) if take[i]]
        details = N.refine_chains(_NestedBackend(self), state)
        out = [None] * nc
        for ch, d in zip(state, details):
            out[ch.index] = d
            self._rocco_count[ch.index] = int(d["final_selected_count"])
        return out

    def narrowpeak_rows(self, selection_penalties, gammas, *, intervals=None, ends=None, interval_bp=None, chroms=None,
                        prefix="consenrich", min_subpeak_bins=5, trim_score_floor=0.0, multiplier=2.0, use_uncertainty=True,
                        chains=None, split_subpeaks=True, width_policy=None, massive_subpeak_cleanup=True,
                        split_quantile=0.25, split_z=2.0, signal="state"):
        """The reference's first-pass narrowPeak rows (`_solutionToChromNarrowPeakRows`, peaks.py:5202-5567, without a width policy
        and without a hierarchy) of every chain's RESIDENT mask, in one device call for all parents of all chains: sub-peaks of
        every run with the min-run dynamic programme (selection penalty = the chain's, boundary cost = 0.25 gamma,
        `min_subpeak_bins`), the trim around each summit, the medians, the maxima and the median filter.  The device reads the
        resident score tracks, as signal float64 of xs[:,0] and as uncertainty the float32 square root of Ps00 (use_uncertainty) of
        the smoothed fit; no resident array changes.  intervals / ends: per chain the bins' coordinates (None: bins of interval_bp
        starting at 0); chroms: the chains' names (None: "chain<i>").  The host cuts the runs at coordinate gaps and does the
        coordinate work from compact records (consenrich_amd/narrowpeak.py).  A chain with a non-finite signal value inside a
        selected run has its signal-dependent numbers redone with NumPy on its downloaded tracks (`decided_on_host`).  Returns per
        chain (None where not taken) a dict: rows, peak_meta, export_details, decided_on_host; `narrowpeak_stats` holds the last
        call's counts and its time on the device and in all.

        width_policy (a dict of `cleanup.learn_massive_subpeak_width_policy`; None: the first pass above, unchanged): the export
        under the massive sub-peak clean-up, as `solveRocco`'s second pass makes it.  Still from resident data alone and without
        changing any: after the children, their final segments come from one `csr_batch_cleanup_plan` call for all chains (only if
        the policy is active and has a threshold; the coordinates travel as a step where `interval_bp` serves every chain,
        otherwise as the children's own edges), and the finishing step runs per SEGMENT -- `csr_batch_export_peaks` again with the
        segments as parents that do not split.  The meta keys and export details of the clean-up are filled as the reference fills
        them, for an inactive policy too; `narrowpeak_stats` gains the five counters.

        signal: "state" (default: xs[:,0]) or "shrunk" -- the resident shrunk state `shrink_apply` left (float32, stride 1), which
        is the reference's export signal in a default run; every taken chain then needs one.  The host fallback of a chain with
        a non-finite signal value downloads and uses the same signal."""
        with self._export_signal(signal):
            return self._narrowpeak_rows(selection_penalties, gammas, intervals, ends, interval_bp, chroms, prefix, min_subpeak_bins,
                                         trim_score_floor, multiplier, use_uncertainty, chains, split_subpeaks, width_policy,
                                         massive_subpeak_cleanup, split_quantile, split_z, signal)

    def _export_signal(self, signal):
        """Points the export stages at `signal` for the duration of a with block, and back at the state afterwards."""
        import contextlib

        if signal not in L.SIGNALS:
            raise ValueError(f"Unknown export signal: {signal!r}; supported values: state, shrunk")

        @contextlib.contextmanager
        def scope():
            L.check(self._lib.csr_batch_set_export_signal(self._ctx, L.SIGNALS[signal]))
            try:
                yield
            finally:
                L.check(self._lib.csr_batch_set_export_signal(self._ctx, L.SIGNALS["state"]))

        return scope()

    def _signal_track(self, chain: int, signal: str) -> np.ndarray:
        """The float64 signal of one chain as the export stages read it, downloaded."""
        if signal == "shrunk":
            return self.download_shrunk(chain, "shrunk").astype(np.float64)
        return self.download(chain, "xs")[:, 0].astype(np.float64)

    def _narrowpeak_rows(self, selection_penalties, gammas, intervals, ends, interval_bp, chroms, prefix, min_subpeak_bins,
                         trim_score_floor, multiplier, use_uncertainty, chains, split_subpeaks, width_policy,
                         massive_subpeak_cleanup, split_quantile, split_z, signal):
        import time

        from . import cleanup as K
        from . import narrowpeak as P

        t_start = time.perf_counter()
        take, mask = self._chain_mask(chains)
        nc = len(take)

        def per_chain(v):
            if isinstance(v, (list, tuple, np.ndarray)):
                if len(v) != nc:
                    raise ValueError("one value per chain")
                return list(v)
            return [v] * nc

        pen, gam = per_chain(selection_penalties), per_chain(gammas)
        uniform = intervals is None and ends is None        # every chain's bins are interval_bp wide
        mult = P.validate_multiplier(multiplier)
        names = [f"chain{i}" for i in range(nc)] if chroms is None else [str(c) for c in chroms]
        iv = [None] * nc if intervals is None else list(intervals)
        en = [None] * nc if ends is None else list(ends)
        if len(iv) != nc or len(en) != nc or len(names) != nc:
            raise ValueError("one intervals / ends / chroms entry per chain")
        cfg = np.zeros(nc, P.CFG)
        parents, spans, details = [], [], [None] * nc
        for c in range(nc):
            if not take[c]:
                continue
            n = self.chain_lens[c]
            if iv[c] is None or en[c] is None:
                if iv[c] is not None or en[c] is not None:
                    raise ValueError("`intervals` and `ends` must be supplied together")
                if interval_bp is None:
                    raise ValueError("`interval_bp` is needed where no coordinates are given")
                iv[c] = np.arange(n, dtype=np.int64) * int(interval_bp)
                en[c] = iv[c] + int(interval_bp)
            iv[c] = np.asarray(iv[c], dtype=np.int64).ravel()
            en[c] = np.asarray(en[c], dtype=np.int64).ravel()
            if iv[c].size != n or en[c].size != n:
                raise ValueError("`intervals`, `ends`, `state`, `scores`, and `solution` must match length")
            cfg[c] = P.chain_cfg(pen[c], 0.25 * float(gam[c]), trim_score_floor, mult, min_subpeak_bins, split_subpeaks, use_uncertainty)
            details[c] = P.export_details(mult, bool(use_uncertainty))
            ps, pe, cuts = P.cut_parents(*self.rocco_runs(c, 0), iv[c], en[c])
            details[c]["num_coordinate_gap_splits"] = cuts
            spans.append((c, len(parents), len(parents) + ps.size))
            parents += [(a, b, c, 0) for a, b in zip(ps.tolist(), pe.tolist())]
        par = np.asarray(parents, P.PARENT) if parents else np.zeros(0, P.PARENT)
        flags = np.zeros(par.size, np.int32)
        count = C.c_int64(0)
        t_device = time.perf_counter()
        L.check_value(self._lib.csr_batch_export_peaks(self._ctx, P._vp(cfg), mask, par.size, P._vp(par), P._vp(flags), C.byref(count)))
        peaks = np.zeros(int(count.value), P.PEAK)
        L.check(self._lib.csr_export_fetch(self._ctx, peaks.size, P._vp(peaks)))
        first = np.searchsorted(peaks["parent"], np.arange(par.size + 1), "left")      # (the peaks come in parent order)
        stats = {"chains": len(spans), "parents": int(par.size), "peaks": int(peaks.size), "decided_on_host": 0}
        by_start = [{} for _ in range(nc)]
        if width_policy is not None:
            active = bool(massive_subpeak_cleanup and bool(width_policy.get("active", False)))
            stats.update({k: 0 for k in K.COUNTERS})
            for c, _, _ in spans:
                details[c]["massive_subpeak_cleanup_active"] = active
                details[c]["massive_subpeak_width_policy"] = dict(width_policy)
            if active and width_policy.get("width_threshold_bp") is not None and peaks.size:
                # the children of all chains through one plan call, then the finishing step per segment
                pol = np.zeros(nc, K.POLICY)
                for c, _, _ in spans:
                    pol[c] = K.policy_row(width_policy, cfg[c]["boundary_cost"], int(max(int(min_subpeak_bins), 1)), split_quantile, split_z)
                kids = np.zeros(peaks.size, K.BATCH_CHILD)
                kids["start"], kids["end"], kids["chain"] = peaks["untrimmed_start"], peaks["untrimmed_end"], peaks["chain"]
                edges = None
                if not uniform:
                    lens = (kids["end"] - kids["start"] + 2).astype(np.int64)
                    kids["edge_base"] = np.concatenate(([0], np.cumsum(lens)[:-1]))
                    edges = np.ascontiguousarray(np.concatenate([np.concatenate((iv[int(k["chain"])][int(k["start"]):int(k["end"]) + 1],
                                                                                 en[int(k["chain"])][int(k["end"]):int(k["end"]) + 1]))
                                                                 for k in kids]), dtype=np.int64)
                seg = np.zeros(K.MAX_SEGMENTS * kids.size, K.SEGMENT)
                cnt = np.zeros(kids.size, K.COUNTS)
                total = C.c_int64(0)
                L.check_value(self._lib.csr_batch_cleanup_plan(
                    self._ctx, P._vp(pol), mask, kids.size, P._vp(kids), 0 if edges is None else edges.size,
                    None if edges is None else edges.ctypes.data_as(L.I64P), int(interval_bp) if edges is None else 0, seg.size,
                    P._vp(seg), C.byref(total), P._vp(cnt)))
                seg = seg[:int(total.value)]
                flat = cfg.copy()
                flat["split"] = 0
                spar = np.zeros(seg.size, P.PARENT)
                spar["start"], spar["end"], spar["chain"] = seg["start"], seg["end"], peaks["chain"][seg["child"]]
                sflags = np.zeros(spar.size, np.int32)
                L.check_value(self._lib.csr_batch_export_peaks(self._ctx, P._vp(flat), mask, spar.size, P._vp(spar), P._vp(sflags),
                                                               C.byref(count)))
                done = np.zeros(int(count.value), P.PEAK)
                L.check(self._lib.csr_export_fetch(self._ctx, done.size, P._vp(done)))
                if done.size != seg.size:
                    raise L.ConsenrichAMDError("narrowPeak clean-up: one record per segment expected")
                kid_chain = peaks["chain"][seg["child"]]
                for c, a, b in spans:
                    sel = np.flatnonzero(kid_chain == c)
                    if sel.size:
                        by_start[c] = K.finish_segments(done[sel[0]:sel[-1] + 1], seg[sel], cnt, peaks)
                    mine = cnt[first[a]:first[b]]
                    K.count_details(details[c], mine)
                    for k in K.COUNTERS:
                        stats[k] += int(mine[k].sum())
                # from here on the segments' records stand for the children's: parent order is kept
                peaks = done
                first = np.searchsorted(peaks["parent"], np.arange(par.size + 1), "left")
                stats["peaks"] = int(peaks.size)
        t_device = time.perf_counter() - t_device
        out = [None] * nc
        for c, a, b in spans:
            mine = peaks[first[a]:first[b]]
            host = bool(np.any(flags[a:b] & L.EXPORT_NONFINITE_SIGNAL))
            if host:
                state = self._signal_track(c, signal)
                unc = np.sqrt(self.download(c, "Ps")[:, 0, 0]).astype(np.float64) if use_uncertainty else None
                with np.errstate(invalid="ignore"):
                    P.redo_on_host(mine, state, self.download_scores(c), unc, cfg[c])
                stats["decided_on_host"] += 1
            rows, meta = P.assemble(names[c], iv[c], en[c], prefix, mine, mult, trim_score_floor, details[c])
            if width_policy is not None:
                K.fill_meta(meta, by_start[c], width_policy)
            out[c] = {"rows": rows, "peak_meta": meta, "export_details": details[c], "decided_on_host": host}
        # (device_seconds: the library call and the fetch of the records; the rest is the host's share: runs, gaps, assembly)
        stats["device_seconds"] = t_device
        stats["seconds"] = time.perf_counter() - t_start
        self.narrowpeak_stats = stats
        return out

    def rocco_objective(self, gammas, chains=None):
        """`_roccoObjectiveForSolution` (peaks.py:2017-2031) of every chain's resident mask and scores: np.sum of the selected
        scores in NumPy's order (on the device) minus max(gamma, 0) times the number of switches.  One float per chain (None where
        not taken)."""
        from . import nested as N

        take, _ = self._chain_mask(chains)
        nc = len(take)
        g = list(gammas) if isinstance(gammas, (list, tuple, np.ndarray)) else [gammas] * nc
        if len(g) != nc:
            raise ValueError("one value per chain")
        runs = {c: self.rocco_runs(c, 0) for c in range(nc) if take[c]}
        n_runs = np.asarray([runs[c][0].size if take[c] else 0 for c in range(nc)], np.int64)
        starts = np.ascontiguousarray(np.concatenate([runs[c][0] for c in range(nc) if take[c]] + [np.zeros(0, np.int64)]), np.int64)
        ends = np.ascontiguousarray(np.concatenate([runs[c][1] for c in range(nc) if take[c]] + [np.zeros(0, np.int64)]), np.int64)
        sums = _NestedBackend(self).selected_sums(take, n_runs, starts, ends)
        return [None if not take[c] else
                N.rocco_objective(float(sums[c]), list(zip(runs[c][0].tolist(), runs[c][1].tolist())), self.chain_lens[c], float(g[c]))
                for c in range(nc)]

    def set_rocco_depth(self, depth: int = 0):
        """Speculation depth D of the penalty calibration (1..8, 0 = default 6).  Changes speed only."""
        L.check(self._lib.csr_set_rocco_depth(self._ctx, int(depth)))

    def rocco_stats(self):
        rs = L.RoccoStats()
        L.check(self._lib.csr_get_rocco_stats(self._ctx, C.byref(rs)))
        return {k: getattr(rs, k) for k, _ in L.RoccoStats._fields_ if k != "reserved"}

    # -- stationary-null DWB panel behind the ROCCO budgets (consenrich_amd/dwb.py) -------------------------------------------
    # -- robust null of the resident scores: centre, scale and DWB template (consenrich_amd/null.py) --------------------------
    def _chain_mask(self, chains):
        nc = len(self.chain_lens)
        take = [True] * nc if chains is None else [bool(t) for t in chains]
        if len(take) != nc:
            raise ValueError("one mask entry per chain")
        return take, (None if chains is None else bytes(bytearray(int(t) for t in take)))

    def rocco_null(self, bulk_quantile: float = 0.60, chains=None):
        """`estimateROCCONull` and `_prepareNullResidualTemplate` (peaks.py:499-540, 1077-1122) of the chains' RESIDENT score
        tracks in one call.  chains: optional per-chain booleans; chains with False keep what they had.  Returns one dict per
        chain (None where not taken): null_center, null_scale, details (the reference's dict), template_meta (the reference's
        template dict) and decided_on_host.  The templates stay on the device (download_template; dwb_panel / dwb_replay with
        templates=None); neither the scores nor any array of the fit changes.  A chain whose central support falls short (see
        consenrich_amd.null) is decided by NumPy from its downloaded track and its template uploaded."""
        from . import null as N

        take, mask = self._chain_mask(chains)
        nc = len(take)
        out = (L.NullOut * nc)()
        L.check_value(self._lib.csr_batch_null_prepare(self._ctx, float(bulk_quantile), mask, out))
        res = [None] * nc
        for i in range(nc):
            if not take[i]:
                continue
            if out[i].host_fallback:
                res[i], template = N.host_result(self.download_scores(i), bulk_quantile)
                self.upload_template(i, template)
            else:
                res[i] = N.chain_result(out[i], self.chain_lens[i])
            self._null[i] = (res[i]["null_center"], res[i]["null_scale"])
        return res

    def download_template(self, chain: int) -> np.ndarray:
        out = np.empty(self.chain_lens[chain], np.float64)
        L.check(self._lib.csr_batch_null_template_download(self._ctx, int(chain), L.dp(out)))
        return out

    def upload_template(self, chain: int, template):
        t = np.ascontiguousarray(np.asarray(template, dtype=np.float64).ravel())
        if t.shape != (self.chain_lens[chain],):
            raise ValueError("template must have shape (chain_len,)")
        if not np.all(np.isfinite(t)):
            raise ValueError("`template` contains non-finite values")
        L.check(self._lib.csr_batch_null_template_upload(self._ctx, int(chain), L.dp(t)))

    def null_pooled_scale(self, chains=None) -> float:
        """`_estimateTemplateScale` (peaks.py:543-556) of the selected chains' resident templates concatenated in chain order
        (the pooled null floor, peaks.py:950-951), on the device."""
        _, mask = self._chain_mask(chains)
        out = np.empty(4, np.float64)
        L.check_value(self._lib.csr_batch_null_pooled_scale(self._ctx, mask, L.dp(out)))
        return float(out[0])

    def _resident_null(self, null_centers, null_scales):
        """None = what rocco_null left, for every chain."""
        nc = len(self.chain_lens)
        if (null_centers is None or null_scales is None) and any(i not in self._null for i in range(nc)):
            raise ValueError("null_centers / null_scales of None need a rocco_null() of every chain first")
        if null_centers is None:
            null_centers = [self._null[i][0] for i in range(nc)]
        if null_scales is None:
            null_scales = [self._null[i][1] for i in range(nc)]
        return null_centers, null_scales

    def dwb_panel(self, templates=None, null_centers=None, null_scales=None, *, threshold_z_grid, tail_quantiles=None, bandwidths,
                  num_bootstrap=128, kernel="bartlett", random_seed=0, calibration_quantile=0.9, pooled_floors=None,
                  draws_per_group=0, noise=None):
        """`dwb.stationary_null_panel` for the batch's chains with the observed statistics taken from the RESIDENT score tracks
        (rocco_scores / upload_scores): nothing of the fit is downloaded, and no resident array changes.  templates /
        null_centers / null_scales of None: what rocco_null left on the device (no template is uploaded)."""
        from . import dwb as W

        batch = self
        null_centers, null_scales = self._resident_null(null_centers, null_scales)

        class _Resident:
            def length(self, c):
                return batch.chain_lens[c]

            def __call__(self, c, thresholds, scales):
                nz = len(thresholds)
                off, sc = np.asarray(thresholds, np.float64), np.asarray(scales, np.float64)
                cnt, soft = np.zeros(nz, np.int64), np.zeros(nz, np.float64)
                L.check_value(batch._lib.csr_batch_dwb_observed(batch._ctx, int(c), nz, L.dp(off), L.dp(sc),
                                                                cnt.ctypes.data_as(L.I64P), L.dp(soft)))
                return cnt, soft

        return W._run_panel(self._ctx, _Resident(), list(self.chain_lens), templates, null_centers, null_scales,
                            threshold_z_grid=threshold_z_grid, tail_quantiles=tail_quantiles, bandwidths=bandwidths,
                            num_bootstrap=num_bootstrap, kernel=kernel, random_seed=random_seed,
                            calibration_quantile=calibration_quantile, pooled_floors=pooled_floors,
                            draws_per_group=draws_per_group, noise=noise)

    # -- dependence span from the resident matrices (consenrich_amd/depspan.py) ---------------------------------------------------
    def dependence_span(self, names, interval_bp, *, chains=None, **kw):
        """`cchooseDependenceSpan` (pyx:3360-4120) of the RESIDENT data: names[k] is the chromosome of chains[k] (default: every
        chain in order; a fold chain is left out by not listing it).  The keywords are the reference's (windowBP, windowCount,
        maxLagBP, ...) and `period_diagnostics`.  Returns (point, lower, upper, diagnostics) like the drop-in, from the same
        kernels; no resident array changes."""
        from . import depspan as D

        return D.batch_dependence_span(self, names, interval_bp, chains=chains, **kw)

    # -- ROCCO budget: effective sample size of a series of the resident scores, and the budget policy (consenrich_amd/ess.py) ----
    def ess(self, kind: str, thresholds, scales, max_lags, chains=None):
        """`cEstimateEffectiveSampleSize` (pyx:9160-9279, its fast path) of a series built on the device from every chain's RESIDENT
        score track, as peaks.py:1414-1434 builds it: kind "occupancy" = (score > threshold) as 0.0 / 1.0; "soft" =
        max((score - threshold) / max(scale, tiny), 0); "integrated" = the soft series of each (threshold, scale) pair added in
        the given order, divided by their number (how `np.mean(np.vstack(parts), axis=0)` adds).  thresholds / scales: per chain
        one value, or for "integrated" a sequence of up to 16; max_lags: one per chain (or one for all).  chains: optional
        per-chain booleans.  Returns (n_eff, tau, lags_used) per chain (None where not taken).  No resident array changes."""
        from . import ess as E

        if kind not in E.KINDS:
            raise ValueError(f"Unknown series kind: {kind}")
        take, mask = self._chain_mask(chains)
        nc = len(take)
        if len(thresholds) != nc or len(scales) != nc:
            raise ValueError("one threshold (sequence) and one scale (sequence) per chain")
        thr = [np.atleast_1d(np.asarray(t, np.float64)) for t in thresholds]
        sc = [np.atleast_1d(np.asarray(s, np.float64)) for s in scales]
        nz = thr[0].shape[0]
        if not 1 <= nz <= E.MAX_Z or any(t.shape != (nz,) or s.shape != (nz,) for t, s in zip(thr, sc)):
            raise ValueError(f"every chain needs the same number (1..{E.MAX_Z}) of thresholds and scales")
        if kind != "integrated" and nz != 1:
            raise ValueError("one threshold and one scale per chain for this series")
        lags = np.asarray([E._c_int(v) for v in (max_lags if np.ndim(max_lags) else [max_lags] * nc)], np.int64)
        if lags.shape != (nc,):
            raise ValueError("one maxLag per chain")
        t_all, s_all = np.ascontiguousarray(np.stack(thr)), np.ascontiguousarray(np.stack(sc))
        out = (L.EssOut * nc)()
        L.check_value(self._lib.csr_batch_ess(self._ctx, E.KINDS[kind], nz, L.dp(t_all), L.dp(s_all), lags.ctypes.data_as(L.I64P), mask,
                                              out))
        return [(float(out[i].n_eff), float(out[i].tau), int(out[i].lags_used)) if take[i] else None for i in range(nc)]

    def rocco_budget(self, panel, *, statistic="occupancy", threshold_z, threshold_z_grid, dependence_spans, budget_min=None,
                     budget_max=None):
        """`_estimateBudgetForPreparedROCCOScore` (peaks.py:1275-1516) for every chain from what `dwb_panel` returned: the
        statistic's aliases, the primary view (that of threshold_z, else of the first z of the resolved grid), the three raw and
        clipped budgets, and the effective sample size of the statistic's series over lags up to 4 * dependence span -- scanned
        on the device from the resident scores (`ess`).  budget_min / budget_max of None: the reference's constants.  Returns per
        chain the numeric fields of the reference's details from `statistic` through `ess_lags_used`, plus `budget`."""
        from . import ess as E

        nc = len(self.chain_lens)
        if len(panel) != nc:
            raise ValueError("one panel result per chain")
        spans = [E._c_int(s) for s in (dependence_spans if np.ndim(dependence_spans) else [dependence_spans] * nc)]
        if len(spans) != nc:
            raise ValueError("one dependence span per chain")
        lo = E.BUDGET_MIN if budget_min is None else budget_min
        hi = E.BUDGET_MAX if budget_max is None else budget_max
        pol = [E.budget_policy(panel[c], statistic=statistic, threshold_z=threshold_z, threshold_z_grid=threshold_z_grid,
                               budget_min=lo, budget_max=hi) for c in range(nc)]
        kind = E.SERIES_OF[pol[0]["statistic"]]
        thr = [[float(v["threshold"]) for v in p["series_views"]] for p in pol]
        sc = [[float(v["null_scale"]) for v in p["series_views"]] for p in pol]
        got = self.ess(kind, thr, sc, [max(4 * s, s) for s in spans])
        return [E.budget_details(pol[c], threshold_z, spans[c], got[c]) for c in range(nc)]

    def rocco_gamma(self, gamma=-1.0, *, dependence_spans, gamma_spans=None, gamma_scale=0.5, clip_min=0.5, clip_max=50.0,
                    null_centers=None, thresholds=None):
        """`estimateROCCOGamma` (peaks.py:1694-1780) for every chain: (gamma, details) per chain.  gamma of None (0.5) or >= 0
        comes back unchanged ("fixed"); a non-finite one raises the reference's error.  For gamma < 0 the boundary penalty is
        gamma_scale * gamma span * the median of (score - level) over its positive entries, clipped -- the level being the
        chain's threshold, else its null centre, else zero.  The median comes from ranks of the resident scores, sorted on the
        device with the null's sort: the count above the level and the one or two middle scores are fetched, the level
        subtracted and the two averaged here; without a positive entry the scale is 1.0.  dependence_spans: the span is an
        input (one per chain or one for all); gamma_spans of None: the span.  No resident array changes."""
        from . import ess as E

        nc = len(self.chain_lens)
        if gamma is None:
            return [(0.5, {"method": "fixed", "gamma": 0.5}) for _ in range(nc)]
        g = float(gamma)
        if not np.isfinite(g):
            raise ValueError("`gamma` must be finite")
        if g >= 0.0:
            return [(g, {"method": "fixed", "gamma": g}) for _ in range(nc)]

        def per_chain(v):
            return list(v) if np.ndim(v) else [v] * nc

        spans, gspans = per_chain(dependence_spans), per_chain(gamma_spans)
        cen, thr = per_chain(null_centers), per_chain(thresholds)
        if not len(spans) == len(gspans) == len(cen) == len(thr) == nc:
            raise ValueError("one value per chain")
        levels = [E.gamma_reference_level(thr[c], cen[c]) for c in range(nc)]
        lv = np.asarray([lvl for lvl, _ in levels], np.float64)
        count, mid = np.zeros(nc, np.int64), np.zeros(2 * nc, np.float64)
        L.check(self._lib.csr_batch_rocco_excess_ranks(self._ctx, L.dp(lv), None, count.ctypes.data_as(L.I64P), L.dp(mid)))
        out = []
        for c in range(nc):
            level = float(lv[c])
            if count[c] <= 0:
                scale = 1.0
            else:
                a, b = float(mid[2 * c]) - level, float(mid[2 * c + 1]) - level
                scale = b if count[c] % 2 else (a + b) / 2.0
            out.append(E.gamma_from_scale(scale, span=spans[c], gamma_span=gspans[c], gamma_scale=gamma_scale, clip_min=clip_min,
                                          clip_max=clip_max, level=level, method=levels[c][1]))
        return out

    def upload_solution(self, chain: int, solution):
        """Plants the selection mask of one chain (a host-decided one: the fallback window of `first_pass_peaks_batch`), so that
        rocco_solution / rocco_runs serve it."""
        s = np.ascontiguousarray(np.asarray(solution).astype(np.uint8).ravel())
        if s.shape != (self.chain_lens[chain],):
            raise ValueError("solution must have shape (chain_len,)")
        L.check(self._lib.csr_batch_rocco_upload(self._ctx, int(chain), s.ctypes.data_as(C.POINTER(C.c_uint8))))
        self._rocco_count[int(chain)] = int(np.count_nonzero(s))

    # -- multiscale candidate segments of the resident scores and of null replays (consenrich_amd/segments.py) --------------
    def _segment_tracks(self, views, scales, min_run, gap, total_cap, view_cap):
        from . import segments as S

        n_s, sc_all, n_v, thr_all, ns_all = S.pack(scales, [v.threshold for v in views], [v.null_scale for v in views])
        nc = len(self.chain_lens)
        rows, counters, flagged = np.zeros(nc, np.int64), np.zeros(3 * nc, np.int64), C.c_int32(0)
        cap = 0 if view_cap is None else view_cap
        L.check_value(self._lib.csr_batch_segments_run(self._ctx, n_s.ctypes.data_as(L.I32P), sc_all.ctypes.data_as(L.I64P),
                                                       n_v.ctypes.data_as(L.I32P), L.dp(thr_all), L.dp(ns_all), min_run, gap, cap,
                                                       rows.ctypes.data_as(L.I64P), counters.ctypes.data_as(L.I64P), C.byref(flagged)))
        tracks = S.collect(self._ctx, rows, counters, flagged.value, cap)
        return [S.compose(tracks[c], views[c], total_cap, view_cap) for c in range(nc)]

    def segment_candidates(self, threshold_views, *, scale_bins=None, dependence_spans=None, min_run_bins=1, max_gap_bins=0,
                           max_segments=20000, max_segments_per_view=1000):
        """`segments.multiscale_candidates` of every chain's RESIDENT score track (rocco_scores / upload_scores) in one call:
        (candidates, diagnostics) per chain.  threshold_views: one set per chain; scale_bins: for all chains, one list per
        chain, or None for the reference's five scales at the chain's dependence span.  Reads the tracks; no resident array
        changes and nothing of the fit is downloaded."""
        from . import segments as S

        nc = len(self.chain_lens)
        if len(threshold_views) != nc:
            raise ValueError("one set of threshold views per chain")
        views = [S.Views(v) for v in threshold_views]
        spans = dependence_spans if dependence_spans is not None and np.ndim(dependence_spans) else [dependence_spans] * nc
        per_chain = scale_bins is not None and len(scale_bins) > 0 and np.ndim(scale_bins[0]) > 0
        scales = [S.resolve_scales(self.chain_lens[c], scale_bins[c] if per_chain else scale_bins, spans[c]) for c in range(nc)]
        total_cap, view_cap = S._caps(max_segments, max_segments_per_view)
        return self._segment_tracks(views, scales, max(int(min_run_bins), 1), max(int(max_gap_bins), 0), total_cap, view_cap)

    def dwb_replay(self, templates=None, threshold_views=None, *, bandwidths, num_replay=64, kernel="bartlett", random_seed=0,
                   scale_bins=None, min_run_bins=1, max_gap_bins=0, max_segments=20000, max_segments_per_view=1000,
                   draws_per_group=0, noise=None):
        """`dwb.null_replay_candidates` for the batch's chains with the observed candidates taken from the RESIDENT score
        tracks; the replays use buffers of the panel's own.  No resident array changes.  templates=None: the resident
        templates rocco_null left."""
        from . import dwb as W

        if threshold_views is None:
            raise TypeError("dwb_replay() needs threshold_views")

        return W._run_replays(self._ctx, self._segment_tracks, list(self.chain_lens), templates, threshold_views,
                              bandwidths=bandwidths, num_replay=num_replay, kernel=kernel, random_seed=random_seed,
                              scale_bins=scale_bins, min_run_bins=min_run_bins, max_gap_bins=max_gap_bins,
                              max_segments=max_segments, max_segments_per_view=max_segments_per_view,
                              draws_per_group=draws_per_group, noise=noise)

    # -- the best score of segments across threshold views (consenrich_amd/peakscore.py) -----------------------------------
    def best_segment_scores(self, chain: int, threshold_views, starts=None, ends=None, *, max_gap_bins: int = 0):
        """`peakscore.best_segment_scores` of one chain's RESIDENT score track (rocco_scores / upload_scores): the reference's
        score dict per segment.  starts / ends None: the runs of the chain's ROCCO mask (rocco_runs), the exported peaks of a
        first pass.  Reads the track; no resident array changes and no track is downloaded."""
        from . import peakscore as P

        if (starts is None) != (ends is None):
            raise ValueError("starts and ends must be given together")
        if starts is None:
            starts, ends = self.rocco_runs(chain, max_gap_bins)
        views = P._Views(threshold_views)
        if not views.keys:
            return [dict(P._ZERO) for _ in range(len(starts))]
        return P.score_details(P.segment_score_arrays(self._ctx, int(chain), None, starts, ends, views), views)

    def dwb_peak_scoring(self, threshold_views, *, bandwidths, peaks=None, templates=None, num_replay=64, kernel="bartlett",
                         random_seed=0, scale_bins=None, min_run_bins=1, max_gap_bins=0, max_segments=20000,
                         max_segments_per_view=1000, draws_per_group=0, noise=None, num_bootstrap=None):
        """The numeric content of the reference's `_addDWBPeakScoringToPeakMeta` (peaks.py:2605-3157) for every chain:
        `peakscore.score_candidate_regions` of the chain's observed candidates and null replays (dwb_replay), with the exported
        peaks scored on the RESIDENT score track.  peaks: None = the runs of each chain's ROCCO mask, or (starts, ends) per
        chain.  num_replay <= 0 and a chain without peaks give the reference's early exits (enabled=False with its reason).
        Returns one dict per chain: enabled, candidate_details, peaks, summary.  No resident array changes, no track of the fit
        or of the scores is downloaded, and the rows of the replays stay on the device in a pool of the panel's own
        (`peakscore.ReplayPool`; `peakscore.last_pool_stats()` counts the draws that had to be decided on the host)."""
        from . import peakscore as P

        nc = len(self.chain_lens)
        if len(threshold_views) != nc or (peaks is not None and len(peaks) != nc):
            raise ValueError("one set of threshold views (and of peaks) per chain")
        spans = [(self.rocco_runs(c) if peaks is None else peaks[c]) for c in range(nc)]
        spans = [list(zip([int(a) for a in s[0]], [int(b) for b in s[1]])) for s in spans]
        if int(num_replay) <= 0:
            return [P.disabled("no_peaks", 0) if not spans[c] else P.disabled("no_bootstrap_draws", len(spans[c])) for c in range(nc)]
        if not any(spans):
            return [P.disabled("no_peaks", 0) for _ in range(nc)]
        pool = P.ReplayPool(self._ctx, list(self.chain_lens), templates, threshold_views, bandwidths=bandwidths, num_replay=num_replay,
                            kernel=kernel, random_seed=random_seed, scale_bins=scale_bins, min_run_bins=min_run_bins,
                            max_gap_bins=max_gap_bins, max_segments=max_segments, max_segments_per_view=max_segments_per_view,
                            draws_per_group=draws_per_group, noise=noise)
        # the observed side first: while the pool is open a segment run leaves its rows on the device
        observed = self._segment_tracks(pool.views, pool.scales, pool.min_run, pool.gap, pool.total_cap, pool.view_cap)
        scores = [self.best_segment_scores(c, threshold_views[c], [a for a, _ in spans[c]], [b for _, b in spans[c]]) if spans[c] else []
                  for c in range(nc)]
        out = []
        with pool:
            for c in range(nc):
                if not spans[c]:
                    out.append(P.disabled("no_peaks", 0))
                    continue
                out.append(P.score_candidate_regions(observed[c], None, spans[c], scores[c], self.chain_lens[c],
                                                     num_bootstrap=num_bootstrap, scale_bins=pool.scales[c], min_run_bins=min_run_bins,
                                                     dependence_span=int(pool.bws[c]), random_seed=random_seed, pool=pool.chain(c)))
        return out

    # -- empirical-Bayes shrinkage of the state track (consenrich_amd/shrink.py) ------------------------------------------------
    def _shrink_prepare(self, chains, variance, block_size):
        take, mask = self._chain_mask(chains)
        unc = None
        if not (isinstance(variance, str) and variance == "fit"):
            tracks = list(variance)
            if len(tracks) != len(take):
                raise ValueError("one uncertainty track (or None) per chain")
            parts = []
            for i, t in enumerate(tracks):
                if not take[i]:
                    continue
                a = np.ascontiguousarray(np.asarray(t, dtype=np.float32).ravel())
                if a.shape != (self.chain_lens[i],):
                    raise ValueError("an uncertainty track must have shape (chain_len,)")
                parts.append(a)
            unc = np.ascontiguousarray(np.concatenate(parts)) if parts else np.zeros(0, np.float32)
        L.check_value(self._lib.csr_batch_shrink_prepare(self._ctx, mask, L.fp(unc), int(max(1, int(block_size)))))
        return take

    def shrink_fit(self, *, chains=None, variance="fit", block_size, model=None, quadrature=None, **fit_arguments):
        """`fitStateShrinkagePrior` (shrinkState.py:465-970) over the chains `chains` takes (per-chain booleans; None: all -- leave
        the fold chains of a batch out of a genome-wide prior), from the RESIDENT smoothed fit: the state is float64 of xs[:,0],
        the variance the float32 square root of Ps00 squared and floored at 1e-12 in float32 (variance="fit": the three float32
        steps of the reference's CLI), or the same of per-chain float32 uncertainty tracks (an entry per chain; those of chains
        not taken are not read).  Every pass is two kernels over the resident tracks; the EM control flow is
        `shrink.fit_state_shrinkage_prior`'s, with its keyword arguments.  Returns the prior.  No array of the fit changes."""
        from . import shrink as S

        take = self._shrink_prepare(chains, variance, block_size)
        batch, nc = self, len(self.chain_lens)
        idx = [i for i in range(nc) if take[i]]

        class _Passes:
            lengths = tuple(batch.chain_lens[i] for i in idx)

            def initial_sums(self, null_z):
                rows = S._initial_rows(batch._ctx, nc, null_z)
                return [S._initial_tuple(rows[i]) for i in idx]

            def em_step(self, pi0, tau, log_prior):
                tau, lsp = S._vec64(tau), S._vec64(log_prior)
                rows = S._em_rows(batch._ctx, nc, pi0, tau, lsp)
                return [S._em_tuple(rows[i], tau.shape[0]) for i in idx]

        return S.fit_state_shrinkage_prior(passes=_Passes(), model=model, blockSize=int(max(1, int(block_size))),
                                           quadrature=quadrature, **fit_arguments)

    def shrink_apply(self, prior, *, spike_odds_multiplier=2.0, chains=None, variance="fit", want_slab=False):
        """`applyStateShrinkagePrior` (shrinkState.py:992-1092) to the chains `chains` takes: their shrunk state, posterior sd and
        spike probability (with want_slab the slab mean and weight too) become resident float32 tracks (`download_shrunk`; the
        export stages' signal="shrunk"); a chain not taken keeps what it had, or stays without.  variance: as in `shrink_fit`.
        Returns the reference's metadata per chain (None where not taken); its four medians are order statistics of the resident
        tracks taken on the device, the two middle values combined as np.median combines float32 values."""
        from . import shrink as S

        multiplier = S.spike_odds_multiplier_value(spike_odds_multiplier)
        effective = S.effective_spike_prop(prior, multiplier)
        tau, weight = S.prior_slabs(prior)
        if tau.shape[0] > L.SHRINK_MAX_SLABS:
            raise ValueError(f"slab arrays must hold 1 to {L.SHRINK_MAX_SLABS} slabs")
        lsp = S.log_slab_prior(effective, weight)
        take = self._shrink_prepare(chains, variance, prior.blockSize)
        nc = len(take)
        L.check_value(self._lib.csr_batch_shrink_posterior(self._ctx, float(effective), int(tau.shape[0]), L.dp(tau), L.dp(lsp),
                                                           int(bool(want_slab))))
        count, mid = np.zeros(nc, np.int64), np.full((nc, 4, 2), np.nan, np.float64)
        L.check(self._lib.csr_batch_shrink_medians(self._ctx, L._i64p(count), L.dp(mid)))
        out = [None] * nc
        for i in range(nc):
            if not take[i]:
                continue
            medians = [float(np.mean(mid[i, r].astype(np.float32))) if count[i] > 0 else float("nan") for r in range(4)]
            out[i] = S.apply_metadata(prior, interval_count=self.chain_lens[i], finite_count=int(count[i]), multiplier=multiplier,
                                      effective=effective, tau=tau, weight=weight, medians=medians)
        return out

    def download_shrunk(self, chain: int, name: str = "shrunk") -> np.ndarray:
        """One chain's resident shrinkage track: "shrunk", "posterior_sd", "spike_prop", "slab_mean", "slab_weight" or "variance"
        (the float32 variance track the passes read).  A chain without it raises ("chain i has no shrunk track")."""
        if name not in L.SHRINK_TRACKS:
            raise ValueError(f"Unknown shrinkage track: {name!r}")
        out = np.empty(self.chain_lens[chain], np.float32)
        L.check(self._lib.csr_batch_shrink_download(self._ctx, int(chain), L.SHRINK_TRACKS[name], L.fp(out)))
        return out

    # -- dense observation-variance seed loop (consenrich_amd/munc.py, csrc/csr_munc.h) -------------------------------------------
    def _seed_put(self, chain: int, name: str, arr):
        ident, per_cell, dtype = L.MUNC_SEED_ARRAYS[name]
        n = self.chain_lens[chain]
        arr = np.ascontiguousarray(arr, dtype=dtype)
        if arr.shape != ((self.m, n) if per_cell else (n,)):
            raise ValueError(f"{name}: expected shape {(self.m, n) if per_cell else (n,)}, got {arr.shape}")
        L.check(self._lib.csr_batch_munc_seed_upload(self._ctx, int(chain), ident, arr.ctypes.data_as(C.c_void_p)))

    def munc_seed_begin(self, seed_munc=None, count_floor=None, exclude=None, chains=None):
        """Opens the seed loop of consenrich.py:7784-7945 on the chains `chains` takes (per-chain booleans; None: all): its arrays
        stay on the device until the batch is configured again.  total starts from the batch's resident munc, or from
        seed_munc[chain] ((m, n) each; a dict or a list with one entry per chain, None entries keep the resident munc); omega and
        rho are 1, the seed background g and its variance G are 0.  count_floor[chain]: (m, n) count-model variance floors, NaN
        meaning none (consenrich.py:7354-7359, with the reference's two RuntimeErrors); exclude[chain]: (n,) bytes, nonzero =
        excluded from the rolling mean of `munc_seed_finish`."""
        nc = len(self.chain_lens)
        take = [True] * nc if chains is None else [bool(t) for t in chains]
        if len(take) != nc:
            raise ValueError("one entry per chain")

        def entries(x):
            if x is None:
                return {}
            items = x.items() if isinstance(x, dict) else enumerate(x)
            return {int(i): v for i, v in items if v is not None and take[int(i)]}

        seed_munc, count_floor, exclude = entries(seed_munc), entries(count_floor), entries(exclude)
        floors = {}
        for i, f in count_floor.items():
            work = np.asarray(f, dtype=np.float32).copy()
            if work.shape != (self.m, self.chain_lens[i]):
                raise RuntimeError("count-model floor matrix must align with MUNC evidence")
            finite = np.isfinite(work)
            if np.any(finite & (work < 0.0)):
                raise RuntimeError("count-model floor must be nonnegative")
            if np.any((~finite) & (~np.isnan(work))):
                raise RuntimeError("count-model floor must be finite or NaN")
            work[~finite] = 0.0
            floors[i] = work
        mask = bytes(bytearray(int(t) for t in take))
        self._seed_take = take
        L.check(self._lib.csr_batch_munc_seed_begin(self._ctx, mask, int(bool(floors)), int(bool(exclude))))
        for i, a in seed_munc.items():
            self._seed_put(i, "seed_total", a)
        for i, a in floors.items():
            self._seed_put(i, "seed_count_floor", a)
        for i, a in exclude.items():
            self._seed_put(i, "seed_exclude", a)

    def munc_seed_upload(self, chain: int, name: str, arr):
        """One chain's part of a resident seed array (`L.MUNC_SEED_ARRAYS`): planted inputs of a stage (a test's).  A planted
        "seed_g" is read by the seed pass only: the smoother subtracts the batch's own background (`set_background`)."""
        if name not in L.MUNC_SEED_ARRAYS:
            raise ValueError(f"Unknown seed array: {name!r}")
        self._seed_put(chain, name, arr)

    def munc_seed_working(self, pad: float, use_weights: bool = True):
        """`_seedWorkingMunc` (consenrich.py:7482-7503) of the current total, omega, rho and G INTO THE BATCH'S OWN munc: the next
        `forward_backward` runs on it, and the fit's resident results are dropped."""
        L.check(self._lib.csr_batch_munc_seed_working(self._ctx, float(pad), int(bool(use_weights))))

    def munc_seed_pass(self, pad: float, update_weights: bool, student_t_df: float = 8.0, omega_min: float = 0.01,
                       omega_max: float = 100.0, use_weights: bool = True, cap=None, student_t: bool = True):
        """`cMuncObservationMomentSeedPass` as the loop calls it (consenrich.py:7505-7541) on the resident arrays: the batch's data,
        the current total as matrixMunc, xs[:,0] and max(Ps[:,0,0], 0) of the resident smoothed fit, g, G, the count floor, the
        current omega and rho.  The new rho, omega and total go to the "next" copies (`munc_seed_swap`), the pointwise local
        evidence to "seed_local".  cap: the reference's maxR (None or <= 0: float32 max).  use_weights is the native's
        `enabled and useSeedWeights`, student_t its `studentT` (the loop passes seedWeightEnabled and seedWeightStudentT combined
        as use_weights and leaves studentT at True; Gaussian weights are use_weights=True, student_t=False: no reweighting).
        The log-only moment and omegaRaw are never written.  Raises the reference's ValueErrors."""
        from . import munc as M
        cap = M.F32_MAX if cap is None or not cap > 0.0 else M._f32(cap)
        cfg = M.seed_cfg(M._f32(pad), M._f32(student_t_df), 8.0, M._f32(omega_min), M._f32(omega_max), M._f32(1.0e-12), cap,
                         bool(use_weights), bool(student_t), bool(update_weights))
        L.check_value(self._lib.csr_batch_munc_seed_pass(self._ctx, C.byref(cfg)))

    def munc_seed_background(self, lam_first: float, lam: float, zero_center=False, use_nonnegative=True,
                             negative_penalty_multiplier=1.0, max_passes=5, block_len=0, *, pad: float, use_weights: bool = True,
                             g_uncertainty: str = "proxy"):
        """`_updateSeedBackground` (consenrich.py:7688-7777) after `munc_seed_pass` and before `munc_seed_swap`, with
        `background_update`'s arguments: the per-cell inverse variance omega * rho / max(total + pad, 1e-12) (float64, cast to
        float32; without weights 1 / max(total + pad, 1e-12)) of the CURRENT total, omega and rho, and the float32 residual data -
        level of the resident fit feed the weighted statistics, the pentadiagonal solve and its asymmetric IRLS unchanged.
        g_uncertainty "disabled": G = 0; "proxy": G = clip(float32(1 / max(sum of the float64 weights +
        `_backgroundPenaltyDiagonal` + multiplier * max(median of the positive sums, 1e-12) where g < 0, 1e-12)), 0, q99 of the
        chain's total).  "seed_g" / "seed_gvar" then hold the new pair and the batch's current background -- what the next
        smoother subtracts from the data -- is the new g.  The solver's errors on a chain of the loop raise RuntimeError as in
        `background_update`, and then no seed array has changed; the statistics and the solve also run over the chains the loop
        left out, whose records come back but whose errors do not raise.  Returns one dict per chain."""
        modes = {"disabled": 0, "proxy": 1}
        if g_uncertainty not in modes:
            raise RuntimeError(f"unsupported MUNC EB prior g uncertainty mode {g_uncertainty}")
        nc = len(self.chain_lens)
        cfg = L.BgCfg(float(lam_first), float(lam),
                      float("nan") if negative_penalty_multiplier is None else float(negative_penalty_multiplier),
                      int(bool(zero_center)), int(bool(use_nonnegative)), 0, 0, int(max_passes), int(block_len))
        outs = (L.BgOut * nc)()
        L.check(self._lib.csr_batch_munc_seed_background(self._ctx, C.byref(cfg), float(pad), int(bool(use_weights)),
                                                         modes[g_uncertainty], outs))
        res = [{k: getattr(o, k) for k, _ in L.BgOut._fields_} for o in outs]
        self._raise_background_errors(res, getattr(self, "_seed_take", None))      # (a chain the loop left out is not its error)
        return res

    def munc_seed_background_tracks(self, chain: int):
        """(weight, rhs, float64 weight sums) of one chain from the last `munc_seed_background`, float64 each."""
        n = self.chain_lens[chain]
        w, r, w64 = np.empty(n), np.empty(n), np.empty(n)
        L.check(self._lib.csr_batch_munc_seed_background_tracks(self._ctx, int(chain), L.dp(w), L.dp(r), L.dp(w64)))
        return w, r, w64

    def munc_seed_swap(self, use_weights: bool = True):
        """The end of a round (consenrich.py:7821-7827): the last pass's total, rho and omega become current; with weights disabled
        omega and rho are refilled with 1."""
        L.check(self._lib.csr_batch_munc_seed_swap(self._ctx, int(not use_weights)))

    def munc_seed_finish(self, window: int, eps: float = 1.0e-12, cap=None, use_weights: bool = True):
        """consenrich.py:7936-7945 after the pointwise pass: "seed_smooth" = `cMuncSmoothDenseLocalEvidence` of "seed_local" under
        the exclude mask, "seed_total" = `_localEvidenceToTotalVariance` of it, "seed_weight" = rho * omega of the pointwise pass
        (ones without weights)."""
        from . import munc as M
        L.check_value(self._lib.csr_batch_munc_seed_finish(self._ctx, int(window), M._f32(eps),
                                                           0.0 if cap is None or not cap > 0.0 else float(cap),
                                                           int(bool(use_weights))))

    def download_munc_seed(self, chain: int, name: str) -> np.ndarray:
        """One chain's part of a resident seed array: "seed_total", "seed_local" (pointwise), "seed_smooth" (local evidence),
        "seed_rho", "seed_omega", "seed_g", "seed_gvar", "seed_weight", "seed_count_floor", "seed_exclude", or the "_next" copies
        of total / rho / omega a pass wrote."""
        if name not in L.MUNC_SEED_ARRAYS:
            raise ValueError(f"Unknown seed array: {name!r}")
        ident, per_cell, dtype = L.MUNC_SEED_ARRAYS[name]
        n = self.chain_lens[chain]
        out = np.empty((self.m, n) if per_cell else (n,), dtype)
        L.check(self._lib.csr_batch_munc_seed_download(self._ctx, int(chain), ident, out.ctypes.data_as(C.c_void_p)))
        return out

    def munc_seed_stats(self) -> dict:
        """Counters since `munc_seed_begin`: passes, rolling means, the rows they smoothed and how many of those were redone
        whole, a wavefront per row, after an inexact running-sum operation (in all, and in the last rolling mean)."""
        st = L.MuncSeedStats()
        L.check(self._lib.csr_batch_munc_seed_stats(self._ctx, C.byref(st)))
        return {k: int(getattr(st, k)) for k, _ in L.MuncSeedStats._fields_}

    # -- finished observation-variance tracks (consenrich_amd/munc_track.py, csrc/csr_munc_track.h) ----------------------------
    def _track_take(self, chains):
        """The chains a stage after the seed loop takes: `chains`, or those of the seed loop."""
        seed = getattr(self, "_seed_take", None)
        if seed is None:
            raise L.ConsenrichAMDError("no seed arrays: call munc_seed_begin first")
        nc = len(self.chain_lens)
        take = list(seed) if chains is None else [bool(t) for t in chains]
        if len(take) != nc:
            raise ValueError("one entry per chain")
        return take, bytes(bytearray(int(t) for t in take))

    def munc_block_sums(self, block_intervals: int, chains=None):
        """The deterministic block summaries of consenrich.py:7981-8040 from the resident "seed_smooth" (local evidence),
        "seed_weight" (zero where "seed_exclude" is set) and the predictor sign(x) log1p(|x|) of xs[:,0] of the resident smoothed
        fit: blocks of max(2, block_intervals) intervals (at most 2048), a last block shorter than 2 dropped.  Returns one dict
        per chain (None where not taken): "valid" (int64), "q", "qp", "qe", "qq" (float64 np.sum of q, q * predictor,
        q * evidence, q * q over the valid cells), each (m, blocks); "included" (non-excluded intervals per block), "starts",
        "ends".  A chain without a block raises the reference's RuntimeError; a fit that is no longer resident is an error
        before any launch.  `munc_track.pooled_block_rows` turns the records into the pooled rows of the trend fit."""
        from . import munc_track as MT

        if max(2, int(block_intervals)) > L.MUNC_BLOCK_MAX:
            raise ValueError(f"block_intervals {int(block_intervals)}: the device stages blocks of up to {L.MUNC_BLOCK_MAX} intervals")
        take, mask = self._track_take(chains)
        layout = [MT.block_layout(n, block_intervals) if t else None for n, t in zip(self.chain_lens, take)]
        for i, lay in enumerate(layout):
            if lay is not None and lay[0].size == 0:
                raise RuntimeError(f"MUNC has no deterministic blocks for chain {i}")
        blocks = sum(lay[0].size for lay in layout if lay is not None)
        recs = np.zeros(blocks * self.m, dtype=L.MUNC_BLOCK_REC)
        included = np.zeros(blocks, dtype=np.int64)
        L.check_value(self._lib.csr_batch_munc_block_sums(self._ctx, int(block_intervals), mask, recs.ctypes.data_as(C.c_void_p),
                                                          recs.shape[0], L._i64p(included), blocks))
        out, at_rec, at_blk = [], 0, 0
        for lay in layout:
            if lay is None:
                out.append(None)
                continue
            nb = lay[0].size
            part = recs[at_rec:at_rec + nb * self.m].reshape(self.m, nb)
            rec = {k: np.ascontiguousarray(part[k]) for k in ("valid", "q", "qp", "qe", "qq")}
            rec.update(included=included[at_blk:at_blk + nb].copy(), starts=lay[0], ends=lay[1])
            out.append(rec)
            at_rec += nb * self.m
            at_blk += nb
        return out

    def munc_prior_track(self, trend, floor: float = 1.0e-12, cap=None, chains=None):
        """`evalPSplineLogVarianceTrend` (core.py:6628-6655) of the float32 level xs[:,0] of the resident smoothed fit (the prior
        mean track of consenrich.py:8163) into the resident per-interval "seed_prior".  trend: (knots, beta, degree, xMin, xMax) or
        an object with those attributes; floor / cap: the reference's eps / maxVariance.  The device evaluates degrees up to 5
        and up to 512 basis functions (ValueError beyond); degree < 0 or empty knots is the constant fallback."""
        from . import munc_track as MT

        knots, beta, degree, x_min, x_max = MT.trend_fields(trend)
        knots, beta = np.ascontiguousarray(knots.ravel()), np.ascontiguousarray(beta.ravel())
        MT.check_trend_limits(knots, beta, degree)
        log_floor, log_cap = MT.log_bounds(floor, cap)
        _take, mask = self._track_take(chains)
        L.check_value(self._lib.csr_batch_munc_prior_track(self._ctx, mask, L.dp(knots), knots.shape[0], L.dp(beta), beta.shape[0],
                                                           degree, x_min, x_max, log_floor, log_cap))

    def munc_track_finish(self, nu_local, nu_prior, replicate_factors=None, count_floor=None, floor: float = 1.0e-12, cap=None,
                          use_eb: bool = True, blacklist_quantile: float = 0.05, chains=None):
        """The finished `matrixMunc` of the taken chains INTO THE BATCH'S OWN munc (the next `forward_backward` runs on it; the
        fit's resident results are dropped).  Per (sample j, interval), as `getMuncTrack` (core.py:8390-8880) does with a pooled
        trend, a prior variance track, a pooled Nu_0 and an effective Nu_L: local = clamp("seed_smooth"), prior =
        clamp(float32(float64("seed_prior") * factor_j)) (no product where |factor_j - 1| <= 1e-8), (Nu_L local + Nu_0 prior) /
        (Nu_L + Nu_0) in float64, clamped, plus the count floor where it is finite, clamped, cast to float32.  Then
        `applyBlacklistMuncFloor` with minR = 1e-12 under the seed loop's exclude mask (skipped without one) and the clamp of
        consenrich.py:9107-9113.

        nu_local / nu_prior: scalars or one value per sample, the reference's EB_effectiveNuL (at least 4) and EB_pooledNu0
        (capped at 50 Nu_L here); replicate_factors: one per sample (None: 1); floor / cap: the reference's
        varianceFloorForTrend and maxR (None or <= 0: none); use_eb=False is the reference's no-EB branch (nu_* unused).
        count_floor[chain]: the caller's RAW (m, n) floor, NaN = missing ("seed_count_floor" has them zeroed); it is uploaded to
        "seed_track_floor".

        Raises what the reference raises, first chain and sample first: the count floor's ValueError of
        `_coerceMuncCountModelVarianceFloor`, then an invalid local value, then an invalid prior value (both under the native's
        "localVarianceTrack must contain finite positive values at index i", as `getMuncTrack` passes them), and the
        RuntimeError of consenrich.py:9100-9106.  Nothing of the batch changes then.

        Returns {"diagnostics": per chain (None where not taken) a list of the native's diagnostics dicts per sample,
        "floors": per chain the float64 blacklist floors per sample}."""
        from . import munc_track as MT

        m, nc = self.m, len(self.chain_lens)
        take, mask = self._track_take(chains)
        floor_, cap_, cap_kernel = MT.variance_bounds(floor, floor, cap if cap is not None and cap > 0.0 else None)
        floor32, cap32 = MT._f32(floor_), MT._f32(cap_kernel)
        factors = np.ones(m) if replicate_factors is None else np.asarray(replicate_factors, dtype=np.float64).reshape(-1)
        if factors.shape[0] != m:
            raise ValueError("one replicate factor per sample")
        if np.any(~np.isfinite(factors) | (factors <= 0.0)):
            raise ValueError("replicateVarianceFactor must be positive and finite")
        prm = (L.MuncTrackPrm * m)()
        if use_eb:
            nu_l = np.broadcast_to(np.asarray(nu_local, dtype=np.float64).reshape(-1), (m,))     # (a scalar, or one per sample)
            nu_0 = np.broadcast_to(np.asarray(nu_prior, dtype=np.float64).reshape(-1), (m,))
            for j in range(m):
                if not np.isfinite(nu_l[j]) or nu_l[j] < 4.0:
                    raise ValueError("EB_effectiveNuL must be finite and at least 4.0")
                if MT._prior_strength(nu_0[j]) is None:
                    raise ValueError("nu_prior must be finite and at least 4.0 (the branch that estimates Nu_0 is not built)")
                n0 = min(float(nu_0[j]), 50.0 * float(nu_l[j]))          # core.py:8796-8804
                prm[j] = L.MuncTrackPrm(MT._f32(nu_l[j]), MT._f32(n0), 0.0, float(factors[j]), 0, 0)
        else:
            for j in range(m):
                prm[j] = L.MuncTrackPrm(0.0, 0.0, 0.0, 1.0, 0, 0)
        floors_in = {}
        if count_floor is not None:
            items = count_floor.items() if isinstance(count_floor, dict) else enumerate(count_floor)
            floors_in = {int(i): v for i, v in items if v is not None and take[int(i)]}
        for i, f in floors_in.items():
            work = np.asarray(f)
            if work.shape != (m, self.chain_lens[i]):
                raise ValueError("countModelVarianceFloor must be a one-dimensional track matching the MUNC interval count")
            if work.dtype != np.float32:        # (the device sees float32: a negative value that rounds to -0.0 is caught here)
                work = np.asarray(work, dtype=np.float64)
                if np.any(np.isfinite(work) & (work < 0.0)):
                    raise ValueError("countModelVarianceFloor must be nonnegative where finite")
            self._seed_put(i, "seed_track_floor", work.astype(np.float32))
        if floors_in:
            for i in range(nc):
                if take[i] and i not in floors_in:
                    self._seed_put(i, "seed_track_floor", np.full((m, self.chain_lens[i]), np.nan, np.float32))
        taken = [i for i in range(nc) if take[i]]
        outs = (L.MuncTrackOut * (len(taken) * m))()
        non_finite = np.zeros(len(taken), dtype=np.int64)
        clamp_hi = float(cap) if cap is not None and np.isfinite(float(cap)) and float(cap) > MT.NUMERIC_VARIANCE_FLOOR else 0.0
        L.check_value(self._lib.csr_batch_munc_track_finish(self._ctx, mask, prm, floor32, cap32, int(bool(use_eb)), int(bool(floors_in)),
                                                            MT.NUMERIC_VARIANCE_FLOOR, float(np.clip(float(blacklist_quantile), 0.0, 1.0)),
                                                            MT.NUMERIC_VARIANCE_FLOOR, clamp_hi, outs, L._i64p(non_finite)))
        diagnostics, floors = [None] * nc, [None] * nc
        for k, i in enumerate(taken):
            n, diag, fl = self.chain_lens[i], [], []
            for j in range(m):
                res = MT._out_dict(outs[k * m + j])
                if res["invalid_count_floor"] >= 0:
                    raise ValueError("countModelVarianceFloor must be nonnegative where finite")
                for kind in ("invalid_local", "invalid_prior"):
                    if res[kind] >= 0:
                        raise ValueError(f"localVarianceTrack must contain finite positive values at index {res[kind]}")
                if res["floor_finite"] == 0:
                    res["floor_missing"] = 0        # core.py:7404-7405: a floor without a finite entry is no floor
                diag.append(MT.track_diagnostics(res, n, bool(use_eb)))
                fl.append(res["blacklist_floor"])
            diagnostics[i], floors[i] = diag, np.asarray(fl, dtype=np.float64)
        for k, i in enumerate(taken):
            if non_finite[k]:
                raise RuntimeError(f"MUNC matrix for chain {i} has {int(non_finite[k])} non-finite entries")
        return {"diagnostics": diagnostics, "floors": floors}

    def export(self, what: int):
        L.check(self._lib.csr_batch_export(self._ctx, int(what)))

    def synchronize(self):
        L.check(self._lib.csr_synchronize(self._ctx))

    # -- results -------------------------------------------------------------------------------------------------
    def download(self, chain: int, name: str, out=None) -> np.ndarray:
        n, d, m = self.chain_lens[chain], self.d, self.m
        shape = {"D": (n,), "xf": (n, d), "Pf": (n, d, d), "pnoise": (max(n - 1, 0), d, d), "xs": (n, d),
                 "Ps": (n, d, d), "lag": (max(n - 1, 0), d, d), "resid": (n, m)}.get(name, (n,))
        if out is None:
            out = np.empty(shape, np.float32)
        elif out.dtype != np.float32 or out.shape != shape or not out.flags.c_contiguous:
            raise ValueError(f"download({name!r}): out must be a contiguous float32 array of shape {shape}")
        L.check(self._lib.csr_batch_download(self._ctx, chain, _ARR[name], out.ctypes.data_as(C.c_void_p)))
        return out

    def device_array(self, name: str):
        ptr, cnt = C.c_void_p(), C.c_int64()
        L.check(self._lib.csr_batch_device_array(self._ctx, _ARR[name], C.byref(ptr), C.byref(cnt)))
        return ptr.value, int(cnt.value)

    def chain_offset(self, chain: int) -> int:
        return int(self._lib.csr_batch_chain_offset(self._ctx, chain))

    # -- instrumentation -----------------------------------------------------------------------------------------
    def profile(self, on: bool):
        L.check(self._lib.csr_profile_enable(self._ctx, int(on)))

    def kernel_times(self):
        buf = (L.KernelTime * 64)()
        n = C.c_int32()
        L.check(self._lib.csr_profile_read(self._ctx, buf, 64, C.byref(n)))
        return {buf[i].name.decode(): (int(buf[i].launches), float(buf[i].total_ms)) for i in range(min(n.value, 64))}

    def run_stats(self):
        rs = L.RunStats()
        L.check(self._lib.csr_get_run_stats(self._ctx, C.byref(rs)))
        return {k: getattr(rs, k) for k, _ in L.RunStats._fields_}
