"""Time the dependence span on the device against the FFT twin (the reference's steps in NumPy) on the same box.

    python scripts/depspan_bench.py [--out profiles/depspan_bench.json] [--repeats 3] [--scale 1.0] [--no-device]

Two inputs at 25 bp with 32 rows, the reference's default settings (100 kb windows, 256 of them, 50 kb of lags): chr1 alone and the
22 autosomes of hg38.  Per input and per repeat: the three stages on their own (unique rows, window scores of every full window,
window ACF of the first windowCount + windowCount / 8 candidates in key order) through the host-array entry (each call stages
its data: the transfer is inside the time), through the batch entry on resident data where the batch fits, and through the FFT
twin (tests/twin_depspan.py); then the whole estimate, device and twin.  The data is synthetic: every window a moving average of
uniform noise whose width differs from window to window, every row a shifted and scaled copy on its own level.  The JSON is
rewritten after every section, so a run that is cut short leaves what it measured."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

HG38 = [248956422, 242193529, 198295559, 190214555, 181538259, 170805979, 159345973, 145138636, 138394717, 133797422, 135086622,
        133275309, 114364328, 107043718, 101991189, 90338345, 83257441, 80373285, 58617616, 64444167, 46709983, 50818468]
INTERVAL, ROWS, WINDOW_BINS = 25, 32, 4000


def chromosome(rng, n):
    base = np.empty(n, dtype=np.float32)
    for a in range(0, n, WINDOW_BINS):
        b = min(n, a + WINDOW_BINS)
        q = int(rng.integers(20, 400))
        c = np.cumsum(rng.random(b - a + q) - 0.5)
        base[a:b] = (c[q:] - c[:-q]) + 0.25 * float(rng.integers(0, 64))
    mat = np.empty((ROWS, n), dtype=np.float32)
    for r in range(ROWS):
        mat[r] = np.roll(base, 997 * r) * np.float32(0.5 + 0.03125 * r) + np.float32(0.125 * r)
    return mat


def timed(fn, repeats):
    out, times = None, []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t0)
    return out, times


def stages(backend, positions, st, D, repeats, windows=None):
    """Seconds per repeat of the three stages; returns (times, the window list used for the ACF stage)."""
    backend.open(positions)
    rows, t_rows = timed(backend.unique_rows, repeats)
    (score, count), t_scores = timed(lambda: backend.window_scores(rows), repeats)
    if windows is None:
        eligible = [(k + 1, "chr%d" % (k + 1), p) for k, p in enumerate(positions)]
        cand, _ = D.rank_candidates(st, eligible, backend_lengths(backend), score, count)
        windows = [(c[3], c[4]) for c in cand[:st.window_count + st.window_count // 8]]
    _, t_acf = timed(lambda: backend.window_acf(rows, windows), repeats)
    return {"unique_rows_s": t_rows, "window_scores_s": t_scores, "window_acf_s": t_acf, "acf_windows": len(windows),
            "retained_rows": len(rows), "windows_scored": int(len(score))}, windows


def backend_lengths(backend):
    return {p: int(n) for p, n in enumerate(getattr(backend, "_lengths"))}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depspan_bench.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="shrink every chromosome (a rehearsal)")
    ap.add_argument("--no-device", action="store_true")
    args = ap.parse_args()

    import twin_depspan as T
    from consenrich_amd import _lib as L
    from consenrich_amd import depspan as D

    kw = dict(bootstrapDraws=100)
    result = {"interval_bp": INTERVAL, "rows": ROWS, "window_bins": WINDOW_BINS, "repeats": args.repeats, "scale": args.scale,
              "settings": "reference defaults, bootstrapDraws=100", "build": None if args.no_device else L.build_id(), "inputs": {}}

    def save():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")

    rng = np.random.default_rng(2025)
    mats_all = []
    for label, count in (("chr1", 1), ("autosomes22", 22)):
        t0 = time.perf_counter()
        while len(mats_all) < count:
            mats_all.append(chromosome(rng, max(3 * WINDOW_BINS, int(HG38[len(mats_all)] * args.scale) // INTERVAL)))
        mats = mats_all[:count]
        names = ["chr%d" % (k + 1) for k in range(count)]
        st = T.settings(count, count, INTERVAL, kw)
        positions = list(range(count))
        rec = {"bins": int(sum(m.shape[1] for m in mats)), "synthesis_s": time.perf_counter() - t0}
        result["inputs"][label] = rec
        windows = None
        if not args.no_device:
            dev = D.HostArrayBackend(mats, st)
            dev._lengths = [m.shape[1] for m in mats]
            rec["device_host_arrays"], windows = stages(dev, positions, st, D, args.repeats)
            save()
            try:
                from consenrich_amd.batch import DeviceBatch, ModelParams

                with DeviceBatch(0) as b:
                    t0 = time.perf_counter()
                    b.configure(ModelParams(state_dim=2), ROWS, [m.shape[1] for m in mats])
                    for c, m in enumerate(mats):
                        b.upload(c, m, m)
                    b.synchronize()
                    rec["batch_upload_s"] = time.perf_counter() - t0
                    res = D.BatchBackend(b, positions, st)
                    res._lengths = [m.shape[1] for m in mats]
                    rec["device_resident"], _ = stages(res, positions, st, D, args.repeats, windows)
                    _, rec["device_resident_total_s"] = timed(lambda: b.dependence_span(names, INTERVAL, **kw), args.repeats)
            except Exception as exc:        # (a batch of this size may not fit beside the fit's own arrays)
                rec["device_resident_error"] = f"{type(exc).__name__}: {exc}"
            save()
            try:
                out, rec["device_host_arrays_total_s"] = timed(lambda: D.cchooseDependenceSpan(names, mats, INTERVAL, **kw), args.repeats)
                rec["device_result"] = [int(v) for v in out[:3]] + [int(out[3]["decided_on_host"]), int(out[3]["selectedWindowCount"])]
            except RuntimeError as exc:
                rec["device_total_error"] = str(exc)
            save()
        twin = T.TwinBackend(mats, st, "fft")
        twin._lengths = [m.shape[1] for m in mats]
        rec["fft_twin"], _ = stages(twin, positions, st, D, args.repeats, windows)
        save()
        try:
            out, rec["fft_twin_total_s"] = timed(lambda: T.fft_twin(names, mats, INTERVAL, **kw), 1)
            rec["fft_twin_result"] = [int(v) for v in out[:3]]
        except RuntimeError as exc:
            rec["fft_twin_total_error"] = str(exc)
        save()
        print(label, json.dumps({k: v for k, v in rec.items()}, indent=None)[:2000], flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
