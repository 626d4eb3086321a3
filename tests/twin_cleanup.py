"""Pure-Python twin of the massive sub-peak clean-up (`_forceMassiveSubpeakSegments`, `_bestMassiveSubpeakSplit`,
`_contractMassiveSubpeakSegment`, `_makeSubpeakSegment`), in two forms:

  form="steps"   the reference's steps in the reference's order: np.quantile / np.median / np.cumsum, a prefix array, recursion,
                 lists of dicts that are merged and overwritten on the way up;
  form="device"  the device's decomposition (csrc/csr_cleanup.h): per node ONE sort of the scores by the merge network (any n, no
                 padding) and the order statistics read off it with NumPy's interpolation rule, one more sort for the MAD, two
                 running sums in place of the prefix array, the mask's median as two members of the mask, an explicit stack whose
                 frames carry the outermost accepted split, segment RECORDS with enum modes and flag bits, the exclusive prefix sum
                 over the counts that packs them, and only then the dicts.

tests/golden/make_cleanup_golden.py writes a fixture only where the reference and both forms agree bit for bit.  BRANCHES (device
form) tells the fixture maker which branches a case took."""
import math

import numpy as np

import twin_narrowpeak as TNP

TN = TNP.TN
BRANCHES = {}
SORT_TILE = 2048
MAX_SEGMENTS = 20
MIN_BP = 7500
MIN_CHILD_BP = 250
MIN_CHILD_FRACTION = 0.05
MODES = (None, "unsplit", "split", "adaptive_core", "width_capped_core")
CANDIDATE, APPLIED, HAS_SPLIT, HAS_CORE_WIDTH, HAS_CORE_FLOOR, MOVED, SPLIT_FROM_PARENT = 1, 2, 4, 8, 16, 32, 64
COUNTERS = ("candidates", "splits", "segments_added", "evaluated", "contracts")
SEGMENT_KEYS = ("start_idx", "end_idx", "summit_idx", "segment_length_bins", "num_subpeaks", "split_from_parent", "subpeak_objective",
                "subpeak_boundary_penalty", "massive_subpeak_cleanup_candidate", "massive_subpeak_cleanup_applied",
                "massive_subpeak_cleanup_mode", "massive_subpeak_split_gain", "massive_subpeak_split_z", "massive_subpeak_gap_bins",
                "massive_subpeak_core_width_bp", "massive_subpeak_core_score_floor", "massive_subpeak_parent_start_idx",
                "massive_subpeak_parent_end_idx")


def reset_branches():
    BRANCHES.clear()


def took(name, n=1):
    BRANCHES[name] = BRANCHES.get(name, 0) + n


# ---------------------------------------------------------------------------------------------------------------
# form="steps"
# ---------------------------------------------------------------------------------------------------------------
def _scale_steps(v):
    scale = 1.4826 * float(np.median(np.abs(v - np.median(v))))
    if not math.isfinite(scale) or scale <= 1.0e-12:
        scale = float(np.quantile(v, 0.75) - np.quantile(v, 0.25)) / 1.349
    if not math.isfinite(scale) or scale <= 1.0e-12:
        scale = 1.0
    return scale


def _split_steps(scores, cost, min_run, q):
    v = np.asarray(scores, np.float64)
    n, m = int(v.size), int(max(int(min_run), 1))
    if n < 3 * m:
        return None
    baseline = float(np.quantile(v, float(np.clip(q, 0.0, 1.0))))
    scale = _scale_steps(v)
    prefix = np.concatenate(([0.0], np.cumsum(baseline - v, dtype=np.float64)))
    best, low, low_at, gap = -math.inf, math.inf, -1, (-1, -1)
    for end in range(2 * m - 1, n - m):
        a = end - m + 1
        if a >= m and float(prefix[a]) < low:
            low, low_at = float(prefix[a]), a
        if low_at < 0:
            continue
        total = float(prefix[end + 1] - low)
        if total > best:
            best, gap = total, (low_at, end)
    if gap[0] < 0 or gap[1] < gap[0]:
        return None
    bins = gap[1] - gap[0] + 1
    return {"gap_start_local": int(gap[0]), "gap_end_local": int(gap[1]), "gap_bins": int(bins), "baseline": baseline, "scale": float(scale),
            "deficit": float(best), "gain": float(best - 2.0 * max(float(cost), 0.0)),
            "z": float(best / (float(scale) * math.sqrt(max(bins, 1))))}


def _contract_steps(start, end, scores, iv, en, threshold, min_run, q):
    v = np.asarray(scores, np.float64)
    if start < 0 or end < start or end >= v.size:
        return None
    loc, a, b = v[start:end + 1], iv[start:end + 1], en[start:end + 1]
    n = int(loc.size)
    original = int(max(int(b[-1]) - int(a[0]), 0))
    thr = float(threshold)
    if not math.isfinite(thr) or thr <= 0.0:
        return None
    if not np.all(np.isfinite(loc)):
        raise ValueError("`scores` contains non-finite values")
    mids = 0.5 * (a.astype(np.float64) + b.astype(np.float64))
    top = float(np.max(loc))
    mask = loc >= top - max(1.0e-12, abs(top) * 1.0e-12)
    centre = float(np.median(mids[mask]))
    c = int(np.argmin(np.abs(mids - centre)))
    m = int(max(int(min_run), 1))
    low = float(np.quantile(loc, float(np.clip(q, 0.0, 1.0))))
    dynamic = float(top - low)
    if math.isfinite(dynamic) and dynamic > 1.0e-12:
        floor = float(low + 0.5 * dynamic)
        keep = loc >= floor
        if keep[c]:
            lo = hi = c
            while lo > 0 and keep[lo - 1]:
                lo -= 1
            while hi + 1 < n and keep[hi + 1]:
                hi += 1
            width = int(max(int(b[hi]) - int(a[lo]), 0))
            if hi - lo + 1 >= m and width < thr and width < original:
                return int(start + lo), int(start + hi), {"mode": "adaptive_core", "core_score_floor": floor, "core_width_bp": width}
    lo = hi = c
    while True:
        options = []
        if lo > 0 and int(max(int(b[hi]) - int(a[lo - 1]), 0)) < thr:
            options.append((float(loc[lo - 1]), -abs(float(mids[lo - 1]) - centre), -1))
        if hi + 1 < n and int(max(int(b[hi + 1]) - int(a[lo]), 0)) < thr:
            options.append((float(loc[hi + 1]), -abs(float(mids[hi + 1]) - centre), 1))
        if not options:
            break
        if max(options)[2] < 0:
            lo -= 1
        else:
            hi += 1
    width = int(max(int(b[hi]) - int(a[lo]), 0))
    if hi - lo + 1 < m or width >= thr or width >= original:
        return None
    return int(start + lo), int(start + hi), {"mode": "width_capped_core", "core_score_floor": None, "core_width_bp": width}


def _segment(start, end, state, o_start, o_end, n_sub, from_parent, objective, penalty, cand=False, applied=False, details=None,
             mode=None):
    d = {} if details is None else dict(details)
    opt = lambda key, kind: None if d.get(key) is None else kind(d[key])     # noqa: E731
    return dict(zip(SEGMENT_KEYS, (
        int(start), int(end), int(start + int(np.argmax(state[start:end + 1]))), int(max(end - start + 1, 0)), int(n_sub),
        bool(from_parent), float(objective), float(penalty), bool(cand), bool(applied), mode, opt("gain", float), opt("z", float),
        opt("gap_bins", int), opt("core_width_bp", int), opt("core_score_floor", float), int(o_start), int(o_end))))


def _limits(iv, en, o_start, o_end, min_run):
    widths = np.asarray(en[o_start:o_end + 1] - iv[o_start:o_end + 1], np.int64)
    widths = widths[widths > 0]
    step = int(max(int(np.median(widths)), 1)) if widths.size else 1
    by_bp = int(math.ceil(float(MIN_CHILD_BP) / float(step)))
    contract_min = int(max(int(min_run), by_bp, 1))
    return int(max(contract_min, int(math.ceil(float(o_end - o_start + 1) * float(MIN_CHILD_FRACTION))))), contract_min


def _contract_threshold(policy, threshold):
    ct = float(policy.get("contract_width_bp", policy.get("min_bp", MIN_BP)))
    if not math.isfinite(ct) or ct <= 0.0:
        ct = float(MIN_BP)
    return float(min(ct, threshold))


def _force_steps(child, v, x, iv, en, policy, cost, min_run, q, min_z, max_depth):
    threshold = float(policy["width_threshold_bp"])
    ct = _contract_threshold(policy, threshold)
    o_start, o_end = int(child["start_idx"]), int(child["end_idx"])
    min_bins, contract_min = _limits(iv, en, o_start, o_end, min_run)
    depth_cap = int(max(int(max_depth), 0))
    counts = {k: 0 for k in COUNTERS}
    objective, penalty = float(child.get("subpeak_objective", 0.0)), float(child.get("subpeak_boundary_penalty", 0.0))

    def settle(a, b, split):
        got = _contract_steps(a, b, v, iv, en, ct, contract_min, q)
        if got is None:
            return [_segment(a, b, x, o_start, o_end, 1, a != o_start or b != o_end, objective, penalty, True, False, split, "unsplit")]
        counts["contracts"] += 1
        return [_segment(got[0], got[1], x, o_start, o_end, 1, True, objective, penalty, True, True,
                         {**({} if split is None else split), **got[2]}, str(got[2]["mode"]))]

    def walk(a, b, depth):
        width = int(max(int(en[b]) - int(iv[a]), 0))
        search = width >= threshold
        if not (search or (depth > 0 and width >= ct)):
            return [_segment(a, b, x, o_start, o_end, 1, a != o_start or b != o_end, objective, penalty)]
        counts["candidates"] += 1
        counts["evaluated"] += 1
        if not search or depth >= depth_cap:
            return settle(a, b, None)
        split = _split_steps(v[a:b + 1], float(cost), min_bins, q)
        if split is None or split["gain"] <= 0.0 or split["z"] < float(min_z):
            return settle(a, b, split)
        left_end, right_start = a + split["gap_start_local"] - 1, a + split["gap_end_local"] + 1
        if left_end - a + 1 < min_bins or b - right_start + 1 < min_bins:
            return settle(a, b, split)
        counts["splits"] += 1
        both = walk(a, left_end, depth + 1) + walk(right_start, b, depth + 1)
        for seg in both:
            seg["massive_subpeak_cleanup_candidate"] = seg["massive_subpeak_cleanup_applied"] = True
            seg["massive_subpeak_cleanup_mode"] = seg.get("massive_subpeak_cleanup_mode") or "split"
            seg["massive_subpeak_split_gain"], seg["massive_subpeak_split_z"] = float(split["gain"]), float(split["z"])
            seg["massive_subpeak_gap_bins"] = int(split["gap_bins"])
        return both

    out = walk(o_start, o_end, 0)
    if len(out) > 1:
        counts["segments_added"] += len(out) - 1
    for seg in out:
        seg["num_subpeaks"] = len(out)
        seg["split_from_parent"] = bool(len(out) > 1 or seg["start_idx"] != o_start or seg["end_idx"] != o_end
                                        or bool(child.get("split_from_parent", False)))
    return out, counts


# ---------------------------------------------------------------------------------------------------------------
# form="device"
# ---------------------------------------------------------------------------------------------------------------
def network_sort(w):
    """csr::cleanup_sort with a team of one: ascending, in place, any n, a pair that reaches past n skipped"""
    n = len(w)
    if n < 2:
        return w
    half = 1
    while 2 * half < n:
        half <<= 1
    k = 2
    while (k >> 1) < n:
        hk = k >> 1
        for t in range(half):
            off = t & (hk - 1)
            i, j = 2 * (t - off) + off, 2 * (t - off) + (k - 1 - off)
            if j < n and w[i] > w[j]:
                w[i], w[j] = w[j], w[i]
        step = hk >> 1
        while step > 0:
            for t in range(half):
                off = t & (step - 1)
                i = 2 * (t - off) + off
                if i + step < n and w[i] > w[i + step]:
                    w[i], w[i + step] = w[i + step], w[i]
            step >>= 1
        k <<= 1
    return w


def quantile_sorted(w, q):
    """np.quantile, method "linear", of ascending w: NumPy's virtual index and its _lerp"""
    m = len(w)
    vi = float(m - 1) * q
    if vi >= float(m - 1):
        return w[m - 1]
    k = int(math.floor(vi))
    t = vi - math.floor(vi)
    took("quantile_integral" if t == 0.0 else "quantile_t_high" if t >= 0.5 else "quantile_t_low")
    d = w[k + 1] - w[k]
    return w[k + 1] - d * (1.0 - t) if t >= 0.5 else w[k] + d * t


def median_sorted(w, m):
    return w[m // 2] if m % 2 else (w[m // 2 - 1] + w[m // 2]) / 2.0


def node_stats(x, q, want_scale):
    n = len(x)
    took("sort_lds" if n <= SORT_TILE else "sort_global")
    for d in (-1, 0, 1):
        if n == SORT_TILE + d:
            took("node_len_tile" + ("_minus_1", "", "_plus_1")[d + 1])
    w = network_sort([float(v) for v in x])
    low = quantile_sorted(w, min(max(q, 0.0), 1.0))
    if not want_scale:
        return low, 1.0
    med = median_sorted(w, n)
    iqr = quantile_sorted(w, 0.75) - quantile_sorted(w, 0.25)
    dev = network_sort([abs(float(v) - med) for v in x])
    scale = 1.4826 * median_sorted(dev, n)
    kind = "scale_mad"
    if not math.isfinite(scale) or scale <= 1.0e-12:
        scale, kind = iqr / 1.349, "scale_iqr"
    if not math.isfinite(scale) or scale <= 1.0e-12:
        scale, kind = 1.0, "scale_one"
    took(kind)
    return low, scale


def split_scan(x, m, baseline, scale, cost):
    n = len(x)
    if n < 3 * m:
        return None
    pa = 0.0
    for i in range(m):
        pa = baseline - x[0] if i == 0 else pa + (baseline - x[i])
    pe = pa
    for i in range(m, 2 * m):
        pe += baseline - x[i]
    best, low, low_at, gs, ge = -math.inf, math.inf, -1, -1, -1
    for end in range(2 * m - 1, n - m):
        a = end - m + 1
        if pa < low:
            low, low_at = pa, a
        elif pa == low:
            took("prefix_tie")
        total = pe - low
        if total > best:
            best, gs, ge = total, low_at, end
        elif total == best:
            took("gap_tie")
        pa += baseline - x[a]
        pe += baseline - x[end + 1]
    if gs < 0 or ge < gs:
        return None
    bins = ge - gs + 1
    return dict(gs=gs, ge=ge, gap_bins=bins, baseline=baseline, scale=scale, deficit=best, gain=best - 2.0 * (cost if cost > 0.0 else 0.0),
                z=best / (scale * math.sqrt(float(max(bins, 1)))))


class Coords:
    def __init__(self, edges):
        self.e = [int(v) for v in edges]

    def width(self, s, e):
        return max(self.e[e + 1] - self.e[s], 0)

    def mid(self, i):
        return 0.5 * (float(self.e[i]) + float(self.e[i + 1]))


def contract(x, co, s, n, thr, m, low):
    """csr::cleanup_contract: (start, end, width, floor or None, mode) or None; x is the node's scores, s its first bin in `co`"""
    original = co.width(s, s + n - 1)
    if not math.isfinite(thr) or thr <= 0.0:
        return None
    top = x[0]
    for v in x:
        top = v if v > top else top
    bar = top - max(1.0e-12, abs(top) * 1.0e-12)
    members = [i for i in range(n) if x[i] >= bar]
    cnt = len(members)
    if cnt > 1:
        took("max_several")
    if cnt % 2 == 0:
        took("max_even_count")
    i1, i2 = members[(cnt - 1) // 2], members[cnt // 2]
    centre = co.mid(s + i1) if cnt % 2 else (co.mid(s + i1) + co.mid(s + i2)) / 2.0
    dv, c0 = math.inf, 0
    for i in range(n):
        d = abs(co.mid(s + i) - centre)
        if d < dv:
            dv, c0 = d, i
        elif d == dv and i > 0:
            took("argmin_tie")
    dynamic = top - low
    if math.isfinite(dynamic) and dynamic > 1.0e-12:
        floor = low + 0.5 * dynamic
        if x[c0] >= floor:
            lo = hi = c0
            while lo > 0 and x[lo - 1] >= floor:
                lo -= 1
            while hi + 1 < n and x[hi + 1] >= floor:
                hi += 1
            width = co.width(s + lo, s + hi)
            if hi - lo + 1 >= m and width < thr and width < original:
                took("adaptive_accepted")
                return s + lo, s + hi, width, floor, 3
            took("adaptive_too_wide" if not (width < thr and width < original) else "adaptive_too_few_bins")
        else:
            took("centre_not_kept")
    else:
        took("flat_scores")
    lo = hi = c0
    while True:
        can_l = lo > 0 and co.width(s + lo - 1, s + hi) < thr
        can_r = hi + 1 < n and co.width(s + lo, s + hi + 1) < thr
        if not can_l and not can_r:
            break
        right = can_r
        if can_l and can_r:
            if x[lo - 1] != x[hi + 1]:
                right = x[hi + 1] > x[lo - 1]
            else:
                dl, dr = -abs(co.mid(s + lo - 1) - centre), -abs(co.mid(s + hi + 1) - centre)
                took("capped_tie_score_distance" if dl == dr else "capped_tie_score")
                right = not dl > dr
        if right:
            hi += 1
        else:
            lo -= 1
    width = co.width(s + lo, s + hi)
    if hi - lo + 1 < m:
        took("contract_refused_bins")
        return None
    if width >= thr or width >= original:
        took("contract_refused_width")
        return None
    took("capped_accepted")
    return s + lo, s + hi, width, None, 4


def plan_child(x, co, kid, pol, uniform_step=None):
    """csr::cleanup_plan_child: (segment records, counts) of bins kid = (start, end) of x under pol = (threshold, contract threshold,
    split quantile, minimum z, boundary cost, minimum run, maximum depth)"""
    thr, ct, q, min_z, cost, min_run, max_depth = pol
    k_start, k_end = kid
    counts = {k: 0 for k in COUNTERS}
    out = []

    def emit(frame, s, e, cand, applied, mode, split, core):
        g = dict(start=s, end=e, core_width_bp=core[2] if core else 0, gain=0.0, z=0.0, core_score_floor=0.0, gap_bins=0, mode=mode,
                 flags=(CANDIDATE if cand else 0) | (APPLIED if applied else 0) | (HAS_CORE_WIDTH if core else 0))
        if core and core[4] == 3:
            g["core_score_floor"] = core[3]
            g["flags"] |= HAS_CORE_FLOOR
        if split is not None:
            g.update(gain=split["gain"], z=split["z"], gap_bins=split["gap_bins"])
            g["flags"] |= HAS_SPLIT
            if mode == 1:
                took("unsplit_with_details")
        if frame["outer"] is not None:
            if split is not None or core is not None:
                took("outer_overwrites_inner" if split is not None else "outer_over_core")
            g.update(gain=frame["outer"][0], z=frame["outer"][1], gap_bins=frame["outer"][2])
            g["flags"] |= HAS_SPLIT | CANDIDATE | APPLIED
            if g["mode"] == 0:
                g["mode"] = 2
        if s != k_start or e != k_end:
            g["flags"] |= MOVED
        assert len(out) < MAX_SEGMENTS
        out.append(g)

    root = dict(s=k_start, e=k_end, depth=0, outer=None)
    length = k_end - k_start + 1
    if not float(co.width(k_start, k_end)) >= thr:
        took("not_a_candidate")
        emit(root, k_start, k_end, False, False, 0, None, None)
        return out, counts
    if not all(math.isfinite(v) for v in x[k_start:k_end + 1]):      # flagged by the plan kernel, refused by the host before it
        raise ValueError("`scores` contains non-finite values")
    if uniform_step is None:
        widths = [co.e[i + 1] - co.e[i] for i in range(k_start, k_end + 1)]
        pos = network_sort([float(d) if d > 0 else math.inf for d in widths])
        m = sum(1 for d in widths if d > 0)
        step_bp = max(int(median_sorted(pos, m)), 1) if m else 1
        if len(set(widths)) > 1:
            took("uneven_widths")
    else:
        step_bp = uniform_step if uniform_step > 1 else 1
    by_bp = int(math.ceil(250.0 / float(step_bp)))
    by_frac = int(math.ceil(float(length) * 0.05))
    contract_min = max(min_run, by_bp, 1)
    min_bins = max(contract_min, by_frac)
    took("min_bins_by_fraction" if by_frac > contract_min else "min_bins_by_bp" if by_bp >= min_run else "min_bins_by_run")
    depth_cap = max(max_depth, 0)
    stack = [root]
    while stack:
        f = stack.pop()
        width, n = co.width(f["s"], f["e"]), f["e"] - f["s"] + 1
        needs_split = float(width) >= thr
        needs_contract = f["depth"] > 0 and float(width) >= ct
        if not needs_split and not needs_contract:
            took("leaf_below_thresholds")
            emit(f, f["s"], f["e"], False, False, 0, None, None)
            continue
        counts["candidates"] += 1
        counts["evaluated"] += 1
        node = [float(v) for v in x[f["s"]:f["e"] + 1]]
        search = needs_split and f["depth"] < depth_cap
        if needs_split and not search:
            took("max_depth_stop")
        if not needs_split:
            took("child_contract_depth")
        scan = search and n >= 3 * min_bins
        if search and not scan:
            took("split_too_short")
        low, scale = node_stats(node, q, scan)
        split = split_scan(node, min_bins, low, scale, cost) if scan else None
        if split is not None:
            if split["gain"] <= 0.0:
                took("split_gain_nonpos")
            elif split["z"] < min_z:
                took("split_z_below")
                if split["z"] == math.nextafter(min_z, -math.inf):
                    took("z_just_below")
            elif split["gs"] < min_bins or n - (split["ge"] + 1) < min_bins:
                took("split_side_short")
            else:
                took(f"split_accepted_depth{f['depth']}")
                if split["z"] == min_z:
                    took("z_at_threshold")
                counts["splits"] += 1
                outer = f["outer"] if f["outer"] is not None else (split["gain"], split["z"], split["gap_bins"])
                stack.append(dict(s=f["s"] + split["ge"] + 1, e=f["e"], depth=f["depth"] + 1, outer=outer))
                stack.append(dict(s=f["s"], e=f["s"] + split["gs"] - 1, depth=f["depth"] + 1, outer=outer))
                took(f"stack_{min(len(stack), 4)}")
                continue
        core = contract(node, co, f["s"], n, ct, contract_min, low)
        if core is not None:
            counts["contracts"] += 1
            emit(f, core[0], core[1], True, True, core[4], split if search else None, core)
        else:
            emit(f, f["s"], f["e"], True, False, 1, split if search else None, None)
    counts["segments_added"] = len(out) - 1 if len(out) > 1 else 0
    return out, counts


def pack(per_child):
    """the host's share: the exclusive prefix sum over the segment counts, the packed records, SPLIT_FROM_PARENT"""
    base, total = [], 0
    for segs, _ in per_child:
        base.append(total)
        total += len(segs)
    packed = [None] * total
    for k, (segs, _) in enumerate(per_child):
        moved = len(segs) > 1 or any(g["flags"] & MOVED for g in segs)
        for i, g in enumerate(segs):
            packed[base[k] + i] = dict(g, child=k, flags=g["flags"] | (SPLIT_FROM_PARENT if moved else 0))
    return packed, base


def record_dict(g, offset, state, o_start, o_end, n_sub, own, objective, penalty):
    a, b, fl = offset + g["start"], offset + g["end"], g["flags"]
    hs = bool(fl & HAS_SPLIT)
    return dict(zip(SEGMENT_KEYS, (
        int(a), int(b), int(a + TNP.leftmost_argmax(state[a:b + 1])), int(max(b - a + 1, 0)), int(n_sub),
        bool(fl & SPLIT_FROM_PARENT) or own, float(objective), float(penalty), bool(fl & CANDIDATE), bool(fl & APPLIED), MODES[g["mode"]],
        float(g["gain"]) if hs else None, float(g["z"]) if hs else None, int(g["gap_bins"]) if hs else None,
        int(g["core_width_bp"]) if fl & HAS_CORE_WIDTH else None, float(g["core_score_floor"]) if fl & HAS_CORE_FLOOR else None,
        int(o_start), int(o_end))))


def _edges(iv, en, start, end):
    a, b = iv[start:end + 1], en[start:end + 1]
    if np.any(b[:-1] != a[1:]):
        raise ValueError("a segment that holds a coordinate gap is not supported")
    return [int(v) for v in a] + [int(b[-1])]


def _force_device(child, v, x, iv, en, policy, cost, min_run, q, min_z, max_depth, coords="edges"):
    threshold = float(policy["width_threshold_bp"])
    start, end = int(child["start_idx"]), int(child["end_idx"])
    edges = _edges(iv, en, start, end)
    steps = {edges[i + 1] - edges[i] for i in range(len(edges) - 1)}
    uniform = steps.pop() if coords == "step" and len(steps) == 1 else None
    pol = (threshold, _contract_threshold(policy, threshold), float(q), float(min_z), float(cost), int(min_run), int(max(int(max_depth), 0)))
    if "contract_width_bp" not in policy:
        took("contract_width_missing")
    if float(policy.get("contract_width_bp", policy.get("min_bp", MIN_BP))) > threshold:
        took("contract_min_applies")
    segs, counts = plan_child([float(s) for s in v[start:end + 1]], Coords(edges), (0, end - start), pol, uniform)
    packed, _ = pack([(segs, counts)])
    own = bool(child.get("split_from_parent", False))
    return [record_dict(g, start, x, start, end, len(packed), own, float(child.get("subpeak_objective", 0.0)),
                        float(child.get("subpeak_boundary_penalty", 0.0))) for g in packed], counts


# ---------------------------------------------------------------------------------------------------------------
# the three entry points
# ---------------------------------------------------------------------------------------------------------------
def best_split(scores, boundaryCost, minRunBins, splitQuantile=0.25, form="steps"):
    if form == "steps":
        return _split_steps(scores, boundaryCost, minRunBins, splitQuantile)
    x = [float(v) for v in np.asarray(scores, np.float64)]
    m = int(max(int(minRunBins), 1))
    if len(x) < 3 * m:
        return None
    low, scale = node_stats(x, float(splitQuantile), True)
    r = split_scan(x, m, low, scale, float(boundaryCost))
    if r is None:
        return None
    return {"gap_start_local": int(r["gs"]), "gap_end_local": int(r["ge"]), "gap_bins": int(r["gap_bins"]), "baseline": float(r["baseline"]),
            "scale": float(r["scale"]), "deficit": float(r["deficit"]), "gain": float(r["gain"]), "z": float(r["z"])}


def contract_segment(startIdx, endIdx, scores, intervals, ends, thresholdBP, minRunBins, splitQuantile=0.25, form="steps"):
    iv, en = np.asarray(intervals, np.int64), np.asarray(ends, np.int64)
    v = np.asarray(scores, np.float64)
    start, end = int(startIdx), int(endIdx)
    if form == "steps":
        return _contract_steps(start, end, v, iv, en, thresholdBP, minRunBins, splitQuantile)
    if start < 0 or end < start or end >= v.size:
        return None
    thr = float(thresholdBP)
    if not math.isfinite(thr) or thr <= 0.0:
        return None
    if not np.all(np.isfinite(v[start:end + 1])):
        raise ValueError("`scores` contains non-finite values")
    x = [float(s) for s in v[start:end + 1]]
    low, _ = node_stats(x, float(splitQuantile), False)
    core = contract(x, Coords(_edges(iv, en, start, end)), 0, len(x), thr, int(max(int(minRunBins), 1)), low)
    if core is None:
        return None
    return int(start + core[0]), int(start + core[1]), {"mode": MODES[core[4]], "core_score_floor": None if core[3] is None else float(core[3]),
                                                        "core_width_bp": int(core[2])}


def force(child, scores, state, intervals, ends, widthPolicy, boundaryCost, minRunBins, splitQuantile=0.25, minSplitZ=2.0, maxDepth=8,
          form="steps", coords="edges"):
    threshold = None if widthPolicy is None else widthPolicy.get("width_threshold_bp")
    if threshold is None:
        return [dict(child)], {k: 0 for k in COUNTERS}
    v, x = np.asarray(scores, np.float64), np.asarray(state, np.float64)
    iv, en = np.asarray(intervals, np.int64), np.asarray(ends, np.int64)
    if form == "steps":
        return _force_steps(child, v, x, iv, en, widthPolicy, boundaryCost, minRunBins, float(splitQuantile), minSplitZ, maxDepth)
    return _force_device(child, v, x, iv, en, widthPolicy, boundaryCost, minRunBins, splitQuantile, minSplitZ, maxDepth, coords)


def differences(got, want):
    """Paths at which two results differ: floats by bit pattern, everything else with its type; dicts with their key order."""
    out = TN.differences(got, want)
    if not out:
        def keys(a, b):
            if isinstance(b, dict):
                if list(a) != list(b):
                    out.append("key order")
                for k in b:
                    keys(a[k], b[k])
            elif isinstance(b, (list, tuple)):
                for p, r in zip(a, b):
                    keys(p, r)
        keys(got, want)
    return out


# ---------------------------------------------------------------------------------------------------------------
# flattening (fixtures hold arrays only)
# ---------------------------------------------------------------------------------------------------------------
SEG_INTS = ("start_idx", "end_idx", "summit_idx", "segment_length_bins", "num_subpeaks", "split_from_parent",
            "massive_subpeak_cleanup_candidate", "massive_subpeak_cleanup_applied", "massive_subpeak_gap_bins",
            "massive_subpeak_core_width_bp", "massive_subpeak_parent_start_idx", "massive_subpeak_parent_end_idx")
SEG_FLOATS = ("subpeak_objective", "subpeak_boundary_penalty", "massive_subpeak_split_gain", "massive_subpeak_split_z",
              "massive_subpeak_core_score_floor")
SPLIT_INTS, SPLIT_FLOATS = ("gap_start_local", "gap_end_local", "gap_bins"), ("baseline", "scale", "deficit", "gain", "z")


def _types(d):
    return "\t".join(f"{k}:{type(v).__name__}" for k, v in d.items())


def flatten_force(result):
    segs, counts = result
    nan = float("nan")
    return {
        "seg_i": np.asarray([[-1 if s.get(k) is None else int(s[k]) for k in SEG_INTS] for s in segs], np.int64).reshape(len(segs), len(SEG_INTS)),
        "seg_f": np.asarray([[nan if s.get(k) is None else float(s[k]) for k in SEG_FLOATS] for s in segs], np.float64).reshape(
            len(segs), len(SEG_FLOATS)),
        "seg_none": np.asarray([[int(s.get(k) is None) for k in SEG_INTS + SEG_FLOATS] for s in segs], np.int64).reshape(
            len(segs), len(SEG_INTS + SEG_FLOATS)),
        "seg_mode": np.asarray([str(s.get("massive_subpeak_cleanup_mode")) for s in segs], dtype="U"),
        "seg_types": np.asarray([_types(s) for s in segs], dtype="U"),
        "counts": np.asarray([counts[k] for k in COUNTERS], np.int64),
        "count_types": np.asarray([_types(counts)], dtype="U"),
    }


def flatten_split(r):
    if r is None:
        return {"none": np.asarray([1], np.int64)}
    return {"none": np.asarray([0], np.int64), "i": np.asarray([r[k] for k in SPLIT_INTS], np.int64),
            "f": np.asarray([r[k] for k in SPLIT_FLOATS], np.float64), "types": np.asarray([_types(r)], dtype="U")}


def flatten_contract(r):
    if r is None:
        return {"none": np.asarray([1], np.int64)}
    a, b, d = r
    floor = d["core_score_floor"]
    return {"none": np.asarray([0], np.int64), "i": np.asarray([a, b, d["core_width_bp"], int(floor is None)], np.int64),
            "f": np.asarray([float("nan") if floor is None else floor], np.float64), "mode": np.asarray([d["mode"]], dtype="U"),
            "types": np.asarray([_types(d) + f"\t{type(a).__name__}\t{type(b).__name__}"], dtype="U")}


def flatten_policy(d):
    nan = float("nan")
    return {"values": np.asarray([nan if v is None else float(v) for k, v in d.items() if k != "method"], np.float64),
            "none": np.asarray([int(v is None) for v in d.values()], np.int64),
            "types": np.asarray([_types(d), str(d["method"])], dtype="U")}


def same_flat(a, b):
    return TNP.same_flat(a, b)


CLEAN_F = ("massive_subpeak_width_p", "massive_subpeak_width_q", "massive_subpeak_split_gain", "massive_subpeak_split_z",
           "massive_subpeak_core_score_floor")
CLEAN_I = ("massive_subpeak_cleanup_candidate", "massive_subpeak_cleanup_applied", "massive_subpeak_gap_bins",
           "massive_subpeak_core_width_bp", "massive_subpeak_width_threshold_bp")
DETAIL_COUNTS = ("num_massive_subpeak_candidates", "num_massive_subpeak_splits", "num_massive_subpeak_segments_added",
                 "num_massive_subpeak_evaluated", "num_massive_subpeak_contracts", "massive_subpeak_cleanup_active")


def flatten_rows(result):
    """(rows, meta, details) of the rows drop-in under a policy: what twin_narrowpeak.flatten keeps, and the clean-up's fields"""
    _, meta, details = result
    out = TNP.flatten(result)
    nan = float("nan")
    out["clean_f"] = np.asarray([[nan if m[k] is None else float(m[k]) for k in CLEAN_F] for m in meta], np.float64).reshape(len(meta), len(CLEAN_F))
    out["clean_i"] = np.asarray([[-1 if m[k] is None else int(m[k]) for k in CLEAN_I] for m in meta], np.int64).reshape(len(meta), len(CLEAN_I))
    out["clean_mode"] = np.asarray([str(m["massive_subpeak_cleanup_mode"]) for m in meta], dtype="U")
    out["clean_types"] = np.asarray([_types(m) for m in meta], dtype="U")
    out["clean_counts"] = np.asarray([int(details[k]) for k in DETAIL_COUNTS], np.int64)
    policy = details["massive_subpeak_width_policy"]
    out["policy_repr"] = np.asarray(["None" if policy is None else _types(policy) + "\t" + repr(sorted(policy.items(), key=lambda kv: kv[0]))], dtype="U")
    out["detail_types"] = np.asarray([_types({k: v for k, v in details.items() if k != "massive_subpeak_width_policy"})], dtype="U")
    return out


# ---------------------------------------------------------------------------------------------------------------
# `_solutionToChromNarrowPeakRows` under a width policy
# ---------------------------------------------------------------------------------------------------------------
def width_pvalue(width, policy):
    from scipy import stats

    centre, scale = policy.get("null_center"), policy.get("null_scale")
    if centre is None or scale is None or not math.isfinite(float(scale)) or float(scale) <= 0.0:
        return None
    z = (math.log(max(float(width), 1.0)) - float(centre)) / float(scale)
    return float(np.clip(float(stats.norm.sf(z)), 0.0, 1.0))


def rows(chromosome, intervals, ends, state, scores, solution, prefix, nullScale, uncertainty=None, splitSubpeaks=True,
         trimScoreFloor=0.0, subpeakSelectionPenalty=None, subpeakBoundaryCost=None, minSubpeakBins=1, massiveSubpeakCleanup=False,
         massiveSubpeakWidthPolicy=None, massiveSubpeakSplitQuantile=0.25, massiveSubpeakSplitZ=2.0,
         dropMedianSignalBelowNegativeLocalP=True, exportFilterUncertaintyMultiplier=2.0, scoreFloor=250.0, scoreCeil=1000.0,
         returnExportDetails=False, form="steps"):
    """The rows under a policy: parents, the dynamic programme's children (twin_narrowpeak), the forced segments of every child
    (`force` in the given form), and the finishing step per SEGMENT -- summit, trim, medians, maxima, the two filters -- with the
    clean-up's meta keys and export details."""
    policy = massiveSubpeakWidthPolicy
    iv, en = np.asarray(intervals, np.int64).ravel(), np.asarray(ends, np.int64).ravel()
    x, s = np.asarray(state, np.float64).ravel(), np.asarray(scores, np.float64).ravel()
    sol = np.asarray(solution, np.uint8).ravel()
    u = None if uncertainty is None else np.asarray(uncertainty, np.float64).ravel()
    mult = float(exportFilterUncertaintyMultiplier)
    filt = bool(dropMedianSignalBelowNegativeLocalP and u is not None)
    active = bool(massiveSubpeakCleanup and policy is not None and bool(policy.get("active", False)))
    details = {
        "num_candidate_segments": 0, "num_segments_dropped_median_signal_local_p": 0, "num_segments_dropped_min_peak_bp": 0,
        "min_peak_bp": TNP.MIN_PEAK_BP, "median_signal_local_p_multiplier": mult, "median_signal_local_p_filter_active": filt,
        "massive_subpeak_cleanup_active": active, "massive_subpeak_width_policy": None if policy is None else dict(policy),
        "num_massive_subpeak_candidates": 0, "num_massive_subpeak_splits": 0, "num_massive_subpeak_segments_added": 0,
        "num_massive_subpeak_evaluated": 0, "num_massive_subpeak_contracts": 0, "num_coordinate_gap_splits": 0,
    }
    fallback = float(max(float(nullScale), 0.0))
    penalty = fallback if subpeakSelectionPenalty is None else float(subpeakSelectionPenalty)
    cost = fallback if subpeakBoundaryCost is None else float(subpeakBoundaryCost)
    min_run = int(max(int(minSubpeakBins), 1))
    n, i, kept, meta = int(sol.size), 0, [], []
    while i < n:
        if sol[i] == 0:
            i += 1
            continue
        a = i
        while i + 1 < n and sol[i + 1] > 0 and en[i] == iv[i + 1]:
            i += 1
        b = i
        i += 1
        if b + 1 < n and sol[b + 1] > 0 and en[b] != iv[b + 1]:
            details["num_coordinate_gap_splits"] += 1
        if splitSubpeaks:
            kids = TNP.segments(s[a:b + 1], x[a:b + 1], a, b, penalty, cost, min_run, "steps")
        else:
            kids = [TNP.whole_parent(x[a:b + 1], a, b, "steps", dict(
                subpeak_objective=0.0, subpeak_boundary_penalty=0.0, massive_subpeak_cleanup_candidate=False,
                massive_subpeak_cleanup_applied=False, massive_subpeak_split_gain=None, massive_subpeak_split_z=None,
                massive_subpeak_gap_bins=None, massive_subpeak_parent_start_idx=int(a), massive_subpeak_parent_end_idx=int(b)))]
        if active:
            forced = []
            for kid in kids:
                segs, counts = force(kid, s, x, iv, en, policy, cost, min_run, float(massiveSubpeakSplitQuantile), float(massiveSubpeakSplitZ),
                                     form=form)
                for k in COUNTERS:
                    details[f"num_massive_subpeak_{k}"] += int(counts[k])
                forced += segs
            kids = forced
        for kid in kids:
            ua, ub, k = int(kid["start_idx"]), int(kid["end_idx"]), int(kid["summit_idx"])
            ca, cb, trimmed = TNP.trim(ua, ub, k, s, trimScoreFloor)
            cx, cs = x[ca:cb + 1], s[ca:cb + 1]
            details["num_candidate_segments"] += 1
            med = float(np.median(cx))
            local = thr = None
            if filt:
                p = u[ca:cb + 1]
                p = p[np.isfinite(p)]
                if p.size > 0:
                    local = float(np.median(p))
                    thr = float(-mult * local)
                    if med < thr:
                        details["num_segments_dropped_median_signal_local_p"] += 1
                        continue
            summit = int(iv[k] + max(1, int((en[k] - iv[k]) // 2)))
            cstart, cend = int(iv[ca]), int(en[cb])
            if cend - cstart < TNP.MIN_PEAK_BP:
                details["num_segments_dropped_min_peak_bp"] += 1
                continue
            name = f"{prefix}_{chromosome}_{len(kept) + 1}"
            opt = lambda key, kind: None if kid.get(key) is None else kind(kid[key])     # noqa: E731
            kept.append(dict(start=cstart, end=cend, signal=float(np.max(cx)), raw=float(np.max(cs)), peak=int(max(0, summit - cstart)), name=name))
            meta.append({
                "name": name, "chromosome": str(chromosome), "start": cstart, "end": cend, "summit": summit, "start_idx": int(ca),
                "end_idx": int(cb), "summit_idx": int(k), "untrimmed_start_idx": ua, "untrimmed_end_idx": ub,
                "segment_length_bins": int(kid["segment_length_bins"]), "median_state": med, "local_median_p": local,
                "median_signal_threshold": thr, "max_state": float(np.max(cx)), "max_score": float(np.max(cs)),
                "num_subpeaks": int(kid["num_subpeaks"]), "split_from_parent": bool(kid["split_from_parent"]),
                "subpeak_objective": float(kid["subpeak_objective"]), "subpeak_boundary_penalty": float(kid["subpeak_boundary_penalty"]),
                "massive_subpeak_cleanup_candidate": bool(kid.get("massive_subpeak_cleanup_candidate", False)),
                "massive_subpeak_cleanup_applied": bool(kid.get("massive_subpeak_cleanup_applied", False)),
                "massive_subpeak_cleanup_mode": kid.get("massive_subpeak_cleanup_mode"),
                "massive_subpeak_width_p": None if policy is None else width_pvalue(float(cend - cstart), policy),
                "massive_subpeak_width_q": None,
                "massive_subpeak_width_threshold_bp": (None if policy is None or policy.get("width_threshold_bp") is None
                                                       else int(policy["width_threshold_bp"])),
                "massive_subpeak_split_gain": opt("massive_subpeak_split_gain", float),
                "massive_subpeak_split_z": opt("massive_subpeak_split_z", float),
                "massive_subpeak_gap_bins": opt("massive_subpeak_gap_bins", int),
                "massive_subpeak_core_width_bp": opt("massive_subpeak_core_width_bp", int),
                "massive_subpeak_core_score_floor": opt("massive_subpeak_core_score_floor", float),
                "trimmed_from_parent": bool(trimmed), "trim_score_floor": None if trimScoreFloor is None else float(trimScoreFloor),
                "untrimmed_start": int(iv[ua]), "untrimmed_end": int(en[ub]),
            })
    if not kept:
        if returnExportDetails:
            details["num_segments_kept"] = 0
            return [], [], details
        return [], []
    raw = np.asarray([r["raw"] for r in kept], np.float64)
    lo, hi = float(np.min(raw)), float(np.max(raw))
    span = max(hi - lo, 1.0e-12)
    out = [[str(chromosome), r["start"], r["end"], r["name"], int(round(scoreFloor + (scoreCeil - scoreFloor) * ((float(r["raw"]) - lo) / span))),
            ".", float(r["signal"]), -1, -1, r["peak"]] for r in kept]
    details["num_segments_kept"] = len(out)
    return (out, meta, details) if returnExportDetails else (out, meta)
