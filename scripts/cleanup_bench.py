"""Measure the export under the massive sub-peak clean-up (DeviceBatch.narrowpeak_rows(width_policy=...)) against the first-pass
export of the same batch and against the route a caller had before it.

    python scripts/cleanup_bench.py                 # 1 x MI355X: chr1 alone and the 22 autosomes
    python scripts/cleanup_bench.py --chr1-only

Writes profiles/cleanup_bench.json (--out).  Workload: that of scripts/narrowpeak_bench.py (hg38 autosomes at 200 bp, one sample,
the levelTrend fit of a synthetic chain, planted parents of 40..600 bins as the resident mask) plus a share of planted MASSIVE
parents in the free tail of every chain: --massive-share of the chain's parents, 300..2000 bins each (60..400 kb), 2-6 plateaus
with noise joined by valleys that stay above the trim floor.  gamma 1, selection penalty 0.3, minSubpeakBins 5, trim floor 0,
multiplier 2.  The policy is learned from the first pass's kept widths with the reference's constants, as
`driver.cleanup_peaks_batch` learns it; if it is not active on the planted widths, a hand-made one with the learned null and the
reference's 7500 bp takes its place (`policy_source`).

Timed with the host clock around whole calls (every call ends synchronised), after one untimed warm-up of each call, --repeats
times, every timing recorded, with the library calls' share and the host's share apart:
  first   narrowpeak_rows(width_policy=None): the first-pass export (the kernels and host code of the parent commit);
  policy  narrowpeak_rows(width_policy=policy): children, their segments, the finishing step per segment;
  before  the download of xs, Ps and the scores of every chain plus the reference-steps form of the pure-Python twin
          (tests/twin_cleanup.py `rows`), once.  The reference itself is not needed: the twin's steps form is held equal to it by
          the fixtures.
Rows, meta and details of `policy` and `before` are compared bit for bit (`identical`)."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "scripts")]

GAMMA, PENALTY, STEP = 1.0, 0.3, 200


def plant_massive(seed, scores, mask, count):
    """`count` massive parents into the free tail of a planted chain (in place); returns how many fitted"""
    rng = np.random.default_rng(seed)
    at = int(np.flatnonzero(mask)[-1]) + 60 if mask.any() else 60
    done = 0
    for _ in range(count):
        n = int(rng.integers(300, 2001))
        if at + n + 60 >= scores.size:
            break
        k = int(rng.integers(2, 7))
        cuts = np.sort(rng.choice(np.arange(20, n - 20), size=2 * k - 1, replace=False))
        level = np.empty(n)
        for j, (a, b) in enumerate(zip(np.concatenate(([0], cuts)), np.concatenate((cuts, [n])))):
            level[a:b] = rng.uniform(4.0, 6.0) if j % 2 == 0 else rng.uniform(1.0, 2.5)
        scores[at:at + n] = np.maximum(level + 0.3 * rng.standard_normal(n), 0.05)
        mask[at:at + n] = 1
        at += n + 60
        done += 1
    return done


def workload(name, lens, parents, args):
    import cases
    import twin_cleanup as T
    from consenrich_amd import _lib as L
    from consenrich_amd import cleanup as K
    from consenrich_amd.batch import DeviceBatch, ModelParams
    from nested_bench import plant

    nc = len(lens)
    share = [max(1, int(round(parents * n / float(sum(lens))))) for n in lens]
    planted = [plant(100 + c, lens[c], share[c]) for c in range(nc)]
    massive = sum(plant_massive(500 + c, planted[c][0], planted[c][1], max(1, int(round(args.massive_share * share[c])))) for c in range(nc))
    names = [f"chr{c + 1}" for c in range(nc)]
    with DeviceBatch(0) as b:
        b.configure(ModelParams(state_dim=2), 1, lens)
        for c in range(nc):
            b.upload(c, *cases.synth(lens[c], 1, 300 + c))
        b.stats()
        b.forward_backward(L.RETURN_NLL)
        b.export(L.EXPORT_SMOOTH)
        for c in range(nc):
            b.upload_scores(c, planted[c][0])
        b.rocco(budget=0.1, gamma=GAMMA, selection_penalty=PENALTY)
        for c in range(nc):
            b.upload_solution(c, planted[c][1])

        def timed(**kw):
            t_all, t_dev, out = [], [], None
            for rep in range(args.repeats + 1):         # the first one is the warm-up
                t0 = time.perf_counter()
                out = b.narrowpeak_rows(PENALTY, GAMMA, interval_bp=STEP, chroms=names, prefix="bench", **kw)
                if rep:
                    t_all.append(time.perf_counter() - t0)
                    t_dev.append(float(b.narrowpeak_stats["device_seconds"]))
            return out, t_all, t_dev, dict(b.narrowpeak_stats)

        first, t_first, d_first, s_first = timed()
        widths = [float(m["end"] - m["start"]) for r in first for m in r["peak_meta"]]
        policy = K.learn_massive_subpeak_width_policy(widths)
        source = "learned"
        if not policy["active"]:
            policy = dict(policy, active=True, width_threshold_bp=K.MIN_BP)
            source = "hand-made: the learned null, 7500 bp"
        new, t_new, d_new, s_new = timed(width_policy=policy)
        t0 = time.perf_counter()
        tracks = []
        for c in range(nc):
            x = b.download(c, "xs")[:, 0].astype(np.float64)
            u = np.sqrt(b.download(c, "Ps")[:, 0, 0]).astype(np.float64)
            tracks.append((x, u, b.download_scores(c)))
        t_download = time.perf_counter() - t0
    identical, t_twin = True, 0.0
    for c in range(nc):
        iv = np.arange(lens[c], dtype=np.int64) * STEP
        x, u, s = tracks[c]
        t0 = time.perf_counter()
        want = T.rows(names[c], iv, iv + STEP, x, s, planted[c][1], "bench", 0.5, uncertainty=u, trimScoreFloor=0.0,
                      subpeakSelectionPenalty=PENALTY, subpeakBoundaryCost=0.25 * GAMMA, minSubpeakBins=5, massiveSubpeakCleanup=True,
                      massiveSubpeakWidthPolicy=policy, returnExportDetails=True, form="steps")
        t_twin += time.perf_counter() - t0
        same = T.differences((new[c]["rows"], new[c]["peak_meta"], new[c]["export_details"]), want) == []
        identical = identical and same
        print(f"{name}: chain {c} identical {same}", flush=True)
    med = lambda v: float(np.median(v))     # noqa: E731
    out = dict(chains=nc, bins=int(sum(lens)), parents=int(s_first["parents"]), massive_parents=int(massive),
               first_pass_peaks=int(s_first["peaks"]), cleaned_peaks=int(s_new["peaks"]), kept_first=len(widths),
               kept_cleaned=int(sum(len(r["rows"]) for r in new)), policy_source=source, policy=policy,
               counters={k: int(s_new[k]) for k in K.COUNTERS}, decided_on_host=int(s_new["decided_on_host"]),
               first_pass_seconds=t_first, first_pass_seconds_median=med(t_first), first_pass_device_seconds=d_first,
               first_pass_host_share_median=med(t_first) - med(d_first),
               policy_call_seconds=t_new, policy_call_seconds_median=med(t_new), policy_call_device_seconds=d_new,
               policy_call_device_seconds_median=med(d_new), policy_call_host_share_median=med(t_new) - med(d_new),
               policy_over_first_pass=med(t_new) / med(t_first), download_tracks_seconds=t_download, twin_seconds=t_twin,
               before_route_seconds=t_download + t_twin, identical=bool(identical))
    doc = {}
    if os.path.exists(args.out):
        with open(args.out) as fh:
            doc = json.load(fh)
    doc[name] = out
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps({name: {k: v for k, v in out.items() if k != "policy"}}), flush=True)
    return identical


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cleanup_bench.json"))
    ap.add_argument("--parents", type=int, default=3000, help="planted parents on chr1")
    ap.add_argument("--genome-parents", type=int, default=34000, help="planted parents over the 22 autosomes")
    ap.add_argument("--massive-share", type=float, default=0.004, help="massive parents per planted parent")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--chr1-only", action="store_true")
    ap.add_argument("--bins", type=int, default=0, help="one chain of this many bins instead of the hg38 chains (a quick check)")
    args = ap.parse_args()
    from consenrich_amd import _lib as L
    from consenrich_amd.sharding import hg38_chain_lengths

    L.require_gpu()
    lens = [int(n) for n in hg38_chain_lengths(200)]
    if args.bins > 0:
        return 0 if workload(f"bins_{args.bins}", [args.bins], args.parents, args) else 1
    ok = workload("chr1", lens[:1], args.parents, args)
    if not args.chr1_only:
        ok = workload("genome_22_chains", lens, args.genome_parents, args) and ok
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
