"""Measure the robust null on the device (csrc/csr_null.h) against the host path it replaces.

    python scripts/null_bench.py            # 1 x MI355X, writes profiles/null_bench.json (--out)

One process, the 22 hg38 autosomes at 200 bp as one batch with planted score tracks (a Gaussian bulk plus a shifted tenth):
  (a) `DeviceBatch.rocco_null()` of the batch, after a warm-up call, ending in a synchronise; the library's own event timers
      (csr_profile_read) give the per-kernel split, and the sort's traffic (16 bytes per key and pass over the padded tracks)
      divided by its time the achieved bytes/s;
  (b) the host path: `download_scores` of every chain, the plain twin of tests/twin_null.py (the reference's steps, its
      half-sample mode a Python loop like the reference's) and the upload of the template a panel would make.  Also timed with
      the half-sample mode vectorised (consenrich_amd.null.host_result), the most a NumPy caller could do.
The templates of (a) and (b) are compared bit for bit on the way."""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]

TILE = 2048


def planted(n, seed):
    rng = np.random.default_rng(seed)
    z = rng.standard_normal(n)
    hot = rng.random(n) < 0.10
    z[hot] += 4.0
    return z + 0.0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "null_bench.json"))
    ap.add_argument("--chains", type=int, default=22, help="the first N autosomes")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-loop-twin", action="store_true", help="skip the plain twin (minutes of Python): vectorised host path only")
    args = ap.parse_args()

    import twin_null as T
    from consenrich_amd import _lib as L
    from consenrich_amd import null as N
    from consenrich_amd.batch import DeviceBatch, ModelParams
    from consenrich_amd.sharding import hg38_chain_lengths

    L.require_gpu()
    lens = [int(n) for n in hg38_chain_lengths(200)][:args.chains]
    tracks = [planted(n, 100 + c) for c, n in enumerate(lens)]
    with DeviceBatch(0) as b:
        b.configure(ModelParams(state_dim=2), 1, lens)
        for c, z in enumerate(tracks):
            b.upload_scores(c, z)
        b.rocco_null()                  # warm-up: work space, first launches
        b.synchronize()
        b.profile(True)
        wall = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            res = b.rocco_null()
            b.synchronize()
            wall.append(time.perf_counter() - t0)
        kt = b.kernel_times()
        b.profile(False)
        split = {k: dict(launches=v[0] // args.repeats, ms=v[1] / args.repeats) for k, v in sorted(kt.items()) if k.startswith("null_")}
        padded = [max((n + TILE - 1) // TILE * TILE, TILE) for n in lens]
        passes = 2 + max(0, math.ceil(math.log2(max(padded) / TILE)))       # tile sort, merge passes, keys -> doubles
        sort_bytes = 16.0 * sum(padded) * passes
        device_templates = [b.download_template(c) for c in range(len(lens))]

        def host_path(decide):
            t0 = time.perf_counter()
            out = []
            for c in range(len(lens)):
                z = b.download_scores(c)
                r = decide(z)
                b.upload_template(c, r["template"])
                out.append(r)
            b.synchronize()
            return time.perf_counter() - t0, out

        def vectorised(z):
            r, t = N.host_result(z, 0.60)
            return dict(r, template=t)

        t_vec, host = host_path(vectorised)
        same = all(np.array_equal(host[c]["template"].view(np.uint64), device_templates[c].view(np.uint64)) and
                   host[c]["null_center"] == res[c]["null_center"] and host[c]["null_scale"] == res[c]["null_scale"]
                   for c in range(len(lens)))
        t_loop = None
        if not args.no_loop_twin:
            t_loop, plain = host_path(lambda z: T.plain_all(z, 0.60))
            same = same and all(np.array_equal(plain[c]["template"].view(np.uint64), device_templates[c].view(np.uint64))
                                for c in range(len(lens)))
    doc = dict(chains=len(lens), bins=int(sum(lens)), repeats=args.repeats,
               device_rocco_null_seconds=min(wall), device_rocco_null_seconds_all=wall,
               host_path_plain_twin_seconds=t_loop, host_path_vectorised_seconds=t_vec,
               device_faster_than_host_path=bool(min(wall) < (t_loop if t_loop is not None else t_vec)),
               device_faster_than_vectorised_host_path=bool(min(wall) < t_vec),
               templates_identical=bool(same), decided_on_host=int(sum(r["decided_on_host"] for r in res)),
               device_ms=split, device_ms_total=sum(v["ms"] for v in split.values()),
               sort_passes=passes, sort_bytes=sort_bytes,
               sort_bytes_per_second=sort_bytes / (split["null_sort"]["ms"] * 1.0e-3) if "null_sort" in split else None,
               note="one process, one MI355X; host path = download_scores + NumPy + upload_template per chain, single-threaded")
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
