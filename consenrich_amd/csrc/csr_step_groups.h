// csr_step_groups.h -- which chains of a pipelined step (step_pipelined, csr_host_pipeline.inl) go out together, and where they
// lie.  Plain C++17, standard library only: tests/step_groups_check.cpp compiles it without HIP.
#pragma once
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

struct ChainInfo { int64_t n, off, b0, nb; };      // bins, natural offset (multiple of 64), first block, number of blocks
struct ChainRun { int64_t off, len, b0, b1; };     // bins [off, off + len) of the natural layout = blocks [b0, b1) of the batch
// Early groups of a step while its state chain runs (the remainder is one more): the caps of the watch loop AND the number of
// device masks / run tables (BatchState, csr_lib.hip)
constexpr int MAX_EARLY_TAILS = 6, MAX_EARLY_EPILOGUES = 8;

// the maximal runs of consecutive chains among those marked in `grp` (a chain occupies [off, off + its length rounded up to 64))
inline std::vector<ChainRun> chain_runs(const std::vector<ChainInfo> &chains, const std::vector<unsigned char> &grp) {
    std::vector<ChainRun> runs;
    for (size_t i = 0; i < chains.size(); ++i) {
        if (!grp[i]) continue;
        const ChainInfo &ci = chains[i];
        const int64_t l = (ci.n + 63) / 64 * 64;
        if (!runs.empty() && runs.back().off + runs.back().len == ci.off && runs.back().b1 == ci.b0) {
            runs.back().len += l;
            runs.back().b1 = ci.b0 + ci.nb;
        } else runs.push_back(ChainRun{ci.off, l, ci.b0, ci.b0 + ci.nb});
    }
    return runs;
}
// {g0, groups}: the wavefront-groups (64 blocks each) from the first to the last block of `runs`.  ONE launch over them, the chain
// mask trims what lies between (round 4: a launch per run of chains serialised four 60-us launches behind the state chain for a
// scattered last group)
inline std::pair<int64_t, int64_t> group_span(const std::vector<ChainRun> &runs) {
    if (runs.empty()) return {0, 0};
    int64_t g0 = runs.front().b0 / 64, g1 = (runs.front().b1 + 63) / 64;
    for (const ChainRun &r : runs) { g0 = std::min(g0, r.b0 / 64); g1 = std::max(g1, (r.b1 + 63) / 64); }
    return {g0, g1 - g0};
}

// What is wrong with a scripted grouping of n chains (ChainSet::pick_scripted), or nullptr: every entry is -1 (remainder) or a group
// index below `cap`, and the indices in use are 0 .. k-1 without a hole
inline const char *script_error(const int32_t *script, int64_t n, int cap) {
    std::vector<unsigned char> used((size_t)cap, 0);
    for (int64_t i = 0; i < n; ++i) {
        if (script[i] < -1) return "a group index below -1";
        if (script[i] >= cap) return "a group index at or above the cap";
        if (script[i] >= 0) used[(size_t)script[i]] = 1;
    }
    for (int g = 1; g < cap; ++g)
        if (used[(size_t)g] && !used[(size_t)g - 1]) return "group indices with a hole";
    return nullptr;
}

// The chains of a batch, handed out in disjoint groups: at most `cap` early ones (pick) while the state chain runs, then whatever
// is left (rest).  The group just handed out owns mask / run-table slot handed() - 1.
class ChainSet {
    const std::vector<ChainInfo> &chains;
    std::vector<unsigned char> taken;
    int64_t total = 0;
    int cap, count = 0;
    bool take(const std::vector<unsigned char> &grp) {
        for (size_t i = 0; i < taken.size(); ++i) taken[i] |= grp[i];
        ++count;
        return true;
    }
public:
    ChainSet(const std::vector<ChainInfo> &chains_, int cap_) : chains(chains_), taken(chains_.size(), 0), cap(cap_) {
        for (const ChainInfo &ci : chains) total += ci.n;
    }
    int handed() const { return count; }        // groups handed out so far, the remainder included
    // grp := the chains that are final (done[i] != 0) and not taken; they are taken, as one group, iff they hold at least `pct` per
    // cent of the batch's bins (and any at all) and fewer than `cap` groups went out
    bool pick(const unsigned *done, int pct, std::vector<unsigned char> &grp) {
        if (count >= cap) return false;
        int64_t bins = 0;
        for (size_t i = 0; i < taken.size(); ++i) bins += (grp[i] = !taken[i] && done[i] != 0u) ? chains[i].n : 0;
        return bins > 0 && bins * 100 >= total * pct && take(grp);
    }
    // A SCRIPTED hand-out (csr_batch_set_step_groups, a test seam): script[i] is the group of chain i, -1 = the remainder.
    // grp := the chains of group handed(); they are taken iff there is such a group and every one of them is final -- no
    // threshold, no timing.  (The script is validated where it is set: groups 0 .. k-1 without a hole, k <= cap.  After clear()
    // the count goes on, so the groups handed out before it are not handed out again.)
    bool pick_scripted(const unsigned *done, const int32_t *script, std::vector<unsigned char> &grp) {
        if (count >= cap) return false;
        bool any = false, final = true;
        for (size_t i = 0; i < taken.size(); ++i) {
            grp[i] = script[i] == count && !taken[i];
            any = any || grp[i];
            final = final && (!grp[i] || done[i] != 0u);
        }
        return any && final && take(grp);
    }
    // grp := the chains not taken; they are taken as the final group (false: none is left)
    bool rest(std::vector<unsigned char> &grp) {
        bool any = false;
        for (size_t i = 0; i < taken.size(); ++i) any = (grp[i] = !taken[i]) || any;
        return any && take(grp);
    }
    // bail-out: every chain is to be done again.  (handed() goes on counting: the groups that were launched were launched, and no
    // slot is used twice in a step)
    void clear() { std::fill(taken.begin(), taken.end(), (unsigned char)0); }
};
