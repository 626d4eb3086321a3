"""Writes tests/golden/shrink/shrink_*.npz from the compiled reference (`make -C oracle ref`, oracle.ref_loader); run it where
the reference exists:  python tests/golden/make_shrink_golden.py

Per fit of tests/shrink_cases.FITS a fixture holds OUTPUTS only (the inputs are re-synthesised from their seeds):
  init_sums / em_sums   the reference natives' per-chunk sums of the initial pass and of the fit's first EM pass (rows in the
                        layout of the C ABI: totalWeight, nullMass, logLikelihood, finiteCount, slabMass[K], slabSecond[K]);
  init_abs / em_abs     the sums of |terms| from the twin, which the per-pass gate is relative to;
  em_pi0, em_tau, em_lsp    the parameter set of that first pass;
  prior_json, meta_json     the reference's fitted prior and its metadata;
  stable                the reference's own loop with multiplicative noise of 1e-11 on every sum agrees with the clean fit
                        within 1e-9 and makes as many iterations (the adaptive mixture fails this on some inputs);
  nodes, weights        the Laguerre rule of a Student-t fit, as data;
  post, post_pi0, post_tau, post_lsp, apply_json    the five posterior tracks of every chunk (spike odds multiplier 2), their
                        parameter set and the per-chunk metadata (POSTERIORS only); ratio_max: the largest postSecond / postVariance.
A fixture is written only if the twin (tests/twin_shrink.py) and the product's EM loop with the sequential twin injected
reproduce the reference bit for bit."""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import shrink_cases as sc  # noqa: E402
import twin_shrink as tw  # noqa: E402
from consenrich_amd import shrink  # noqa: E402
from oracle import ref_loader  # noqa: E402


class RefPasses:
    """The reference's natives as a pass evaluator, optionally with multiplicative Gaussian noise on every sum."""

    def __init__(self, ref, chunks, block, noise=0.0, seed=0):
        self.ref, self.chunks, self.block, self.noise = ref, chunks, int(block), float(noise)
        self.lengths = tuple(int(x.shape[0]) for x, _ in chunks)
        self.rng = np.random.default_rng(seed)

    def _n(self, value):
        if self.noise == 0.0:
            return value
        return value * (1.0 + self.noise * self.rng.standard_normal(np.shape(value)))

    def initial_sums(self, null_z):
        out = []
        for x, v in self.chunks:
            s = self.ref.cstateShrinkInitialSums(x, v, float(null_z), self.block)
            out.append((float(self._n(s[0])), float(self._n(s[1])), float(self._n(s[2])), float(self._n(s[3])), int(s[4])))
        return out

    def em_step(self, pi0, tau, log_prior):
        out = []
        for x, v in self.chunks:
            s = self.ref.cstateShrinkMixtureEMStepPrepared(x, v, float(pi0), tau, log_prior, self.block)
            out.append((float(self._n(s[0])), float(self._n(s[1])), self._n(np.asarray(s[2])), self._n(np.asarray(s[3])),
                        float(self._n(s[4])), int(s[5])))
        return out


def rows_of_em(passes_out, k):
    return np.array([[s[0], s[1], s[4], float(s[5]), *s[2], *s[3]] for s in passes_out], dtype=np.float64)


def same_meta(a, b) -> bool:
    return json.dumps(a, sort_keys=True) == json.dumps(b, sort_keys=True)


def prior_dict(p) -> dict:
    return {"model": p.model, "priorSpikeProp": p.priorSpikeProp, "priorScale": p.priorScale, "priorVariance": p.priorVariance,
            "blockSize": p.blockSize, "slabVariance": list(p.slabVariance), "slabWeight": list(p.slabWeight),
            "componentWeights": list(p.componentWeights)}


def close(a, b, rel) -> bool:
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all(np.abs(a - b) <= rel * np.abs(b)))


def main() -> int:
    ref = ref_loader.load()
    if ref is None:
        print("the compiled reference is not available here")
        return 1
    from consenrich import shrinkState as rs

    os.makedirs(sc.GOLDEN, exist_ok=True)
    for inp, model, order in sc.FITS:
        name = sc.fit_name(inp, model, order)
        chunks, block = sc.make_input(inp)
        kw = sc.fit_kwargs(model, order)
        ref_prior = rs.fitStateShrinkagePrior(chunks, blockSize=block, **kw)
        quad = None
        out = {}
        if model == sc.STUDENT:
            meta = ref_prior.metadata
            from scipy import special

            quad = special.roots_genlaguerre(meta["student_t_quadrature_order"], meta["student_t_quadrature_alpha"])
            out["nodes"], out["weights"] = np.asarray(quad[0], dtype=np.float64), np.asarray(quad[1], dtype=np.float64)
        # the product's loop over the sequential twin, and over the reference's natives
        seq = tw.SequentialPasses(chunks, block)
        ours = shrink.fit_state_shrinkage_prior(passes=seq, blockSize=block, quadrature=quad, **kw)
        ours_ref = shrink.fit_state_shrinkage_prior(passes=RefPasses(ref, chunks, block), blockSize=block, quadrature=quad, **kw)
        for got, what in ((ours, "twin"), (ours_ref, "loop")):
            if prior_dict(got) != prior_dict(ref_prior) and not same_meta(prior_dict(got), prior_dict(ref_prior)):
                print(f"{name}: the {what} prior differs from the reference's -- no fixture")
                return 1
            if not same_meta(got.metadata, ref_prior.metadata):
                print(f"{name}: the {what} metadata differ from the reference's -- no fixture")
                return 1
        # stability of the reference's own loop against noise on the sums
        noisy = shrink.fit_state_shrinkage_prior(passes=RefPasses(ref, chunks, block, noise=1.0e-11, seed=5), blockSize=block,
                                                 quadrature=quad, **kw)
        stable = (noisy.metadata["iterations"] == ref_prior.metadata["iterations"]
                  and noisy.metadata["converged"] == ref_prior.metadata["converged"]
                  and close(noisy.priorSpikeProp, ref_prior.priorSpikeProp, 1e-9)
                  and close(noisy.slabVariance, ref_prior.slabVariance, 1e-9) and close(noisy.slabWeight, ref_prior.slabWeight, 1e-9))
        out["stable"] = np.array(bool(stable))
        # the first EM pass: the parameter set the loop starts from (a one-iteration fit stops right behind it)
        try:
            shrink.fit_state_shrinkage_prior(passes=_Recorder(seq), blockSize=block, quadrature=quad, **kw)
        except _Stop:
            pass
        first = _Recorder.last
        pi0, tau, lsp = first
        nat_init = RefPasses(ref, chunks, block).initial_sums(1.5)
        nat_em = RefPasses(ref, chunks, block).em_step(pi0, tau, lsp)
        init_rows = np.array([[*s[:4], float(s[4])] for s in nat_init], dtype=np.float64)
        em_rows = rows_of_em(nat_em, len(tau))
        if not (np.array_equal(init_rows, np.array(seq.initial_rows(1.5))) and np.array_equal(em_rows, np.array(seq.em_rows(pi0, tau, lsp)))):
            print(f"{name}: the sequential twin's sums differ from the natives' -- no fixture")
            return 1
        tree = tw.TreePasses(chunks, block)
        out.update(init_sums=init_rows, em_sums=em_rows, init_abs=np.array(tree.abs_initial_rows(1.5)),
                   em_abs=np.array(tree.abs_rows(pi0, tau, lsp)), em_pi0=np.array(pi0), em_tau=np.asarray(tau), em_lsp=np.asarray(lsp),
                   prior_json=np.array(json.dumps(prior_dict(ref_prior))), meta_json=np.array(json.dumps(ref_prior.metadata)))
        worst = 0.0
        if (inp, model, order) in sc.POSTERIORS:
            eff = shrink.effective_spike_prop(ref_prior, 2.0)
            ptau, pw = shrink.prior_slabs(ref_prior)
            plsp = shrink.log_slab_prior(eff, pw)
            tracks, metas = [], []
            for x, v in chunks:
                res = rs.applyStateShrinkagePrior(x, v, ref_prior, stateShrinkageSpikeOddsMultiplier=2.0)
                got = [res.shrunkState, res.posteriorSd, res.spikeProp, res.slabPosteriorMean, res.slabPosteriorWeight]
                twin, ratio = tw.posterior(x, v, eff, ptau, plsp, with_ratio=True)
                mine = shrink.apply_state_shrinkage_prior(x, v, ref_prior, stateShrinkageSpikeOddsMultiplier=2.0, posterior=tw.posterior)
                if not all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got, twin)):
                    print(f"{name}: the twin's posterior tracks differ from the reference's -- no fixture")
                    return 1
                if not same_meta(mine.metadata, res.metadata):
                    print(f"{name}: the applied metadata differ from the reference's -- no fixture")
                    return 1
                worst = max(worst, float(ratio.max()) if ratio.size else 0.0)
                tracks.append(np.stack(got))
                metas.append(res.metadata)
            if worst > 1.0e6:
                print(f"{name}: postSecond / postVariance reaches {worst:.3g} -- choose other inputs")
                return 1
            out.update(post=np.concatenate(tracks, axis=1), post_pi0=np.array(eff), post_tau=ptau, post_lsp=plsp,
                       apply_json=np.array(json.dumps(metas)), ratio_max=np.array(worst))
        np.savez_compressed(sc.fixture_path(inp, model, order), **out)
        m = ref_prior.metadata
        print(f"{name}: iterations {m['iterations']} converged {m['converged']} stable {bool(stable)} passes {seq.passes} "
              f"ratio_max {worst:.3g}")
    return 0


class _Stop(Exception):
    pass


class _Recorder:
    """Remembers the parameter set of the first EM pass it is asked for, and ends the fit there."""
    last = None

    def __init__(self, inner):
        self.inner, self.lengths = inner, inner.lengths

    def initial_sums(self, null_z):
        return self.inner.initial_sums(null_z)

    def em_step(self, pi0, tau, log_prior):
        _Recorder.last = (float(pi0), np.array(tau, dtype=np.float64), np.array(log_prior, dtype=np.float64))
        raise _Stop


if __name__ == "__main__":
    sys.exit(main())
