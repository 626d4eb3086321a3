// Stand-alone check of consenrich_amd/csrc/csr_step_groups.h (tests/test_abi_and_host.py compiles it with
// g++ -std=c++17 -fsanitize=address,undefined and runs it): runs of chains, their span of wavefront-groups, and the hand-out of
// groups of chains that a pipelined step's watch loop relies on.  No HIP, no GPU.
#include "csr_step_groups.h"

#include <cstdio>
#include <cstdlib>

#define REQUIRE(cond)                                                              \
    do {                                                                           \
        if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

using Mask = std::vector<unsigned char>;

// the chain table as csr_batch_configure lays it out: blocks of B bins, offsets in whole 64-bin units, chains back to back
static std::vector<ChainInfo> table(const std::vector<int64_t> &lens, int64_t B) {
    std::vector<ChainInfo> t;
    int64_t off = 0, b0 = 0;
    for (int64_t n : lens) {
        const int64_t nb = (n + B - 1) / B;
        t.push_back(ChainInfo{n, off, b0, nb});
        off += (n + 63) / 64 * 64;
        b0 += nb;
    }
    return t;
}
static bool same(const ChainRun &r, int64_t off, int64_t len, int64_t b0, int64_t b1) {
    return r.off == off && r.len == len && r.b0 == b0 && r.b1 == b1;
}

int main() {
    // chain:  0     1     2     3     4     5
    // bins:   1    63    64    65   128  4097
    // off:    0    64   128   192   320   448      (padded lengths 64 64 64 128 128 4160, end 4608)
    // blocks: 0     1     2   3-4   5-6  7-71      (72 blocks: wavefront-groups 0 and 1)
    const std::vector<ChainInfo> t = table({1, 63, 64, 65, 128, 4097}, 64);
    REQUIRE(t[3].off == 192 && t[3].b0 == 3 && t[3].nb == 2 && t[5].off == 448 && t[5].b0 == 7 && t[5].nb == 65);
    const int64_t total = 1 + 63 + 64 + 65 + 128 + 4097;      // 4418

    // ---- chain_runs / group_span
    {
        const auto r = chain_runs(t, Mask{1, 1, 1, 1, 1, 1});
        REQUIRE(r.size() == 1 && same(r[0], 0, 4608, 0, 72));
        REQUIRE(group_span(r) == std::make_pair((int64_t)0, (int64_t)2));
    }
    {
        const auto r = chain_runs(t, Mask{0, 0, 0, 0, 0, 0});
        REQUIRE(r.empty());
        REQUIRE(group_span(r) == std::make_pair((int64_t)0, (int64_t)0));
    }
    {
        const auto r = chain_runs(t, Mask{1, 0, 1, 0, 1, 0});
        REQUIRE(r.size() == 3 && same(r[0], 0, 64, 0, 1) && same(r[1], 128, 64, 2, 3) && same(r[2], 320, 128, 5, 7));
        REQUIRE(group_span(r) == std::make_pair((int64_t)0, (int64_t)1));
        const auto o = chain_runs(t, Mask{0, 1, 0, 1, 0, 1});
        REQUIRE(o.size() == 3 && same(o[0], 64, 64, 1, 2) && same(o[1], 192, 128, 3, 5) && same(o[2], 448, 4160, 7, 72));
        REQUIRE(group_span(o) == std::make_pair((int64_t)0, (int64_t)2));
    }
    {
        const auto r = chain_runs(t, Mask{1, 1, 0, 1, 1, 1});
        REQUIRE(r.size() == 2 && same(r[0], 0, 128, 0, 2) && same(r[1], 192, 4416, 3, 72));
        for (const ChainRun &x : r) REQUIRE(x.len % 64 == 0);
        REQUIRE(group_span(r) == std::make_pair((int64_t)0, (int64_t)2));
        // the last chain alone lies in both wavefront-groups; a chain that starts in the second one spans that one only
        REQUIRE(group_span(chain_runs(t, Mask{0, 0, 0, 0, 0, 1})) == std::make_pair((int64_t)0, (int64_t)2));
        const std::vector<ChainInfo> far = table({4096, 64, 65}, 64);         // blocks 0-63, 64, 65-66
        REQUIRE(group_span(chain_runs(far, Mask{0, 1, 1})) == std::make_pair((int64_t)1, (int64_t)1));
        REQUIRE(group_span(chain_runs(far, Mask{1, 0, 0})) == std::make_pair((int64_t)0, (int64_t)1));
    }
    {
        // bins contiguous, blocks not: two runs
        const std::vector<ChainInfo> s = {ChainInfo{64, 0, 0, 1}, ChainInfo{64, 64, 5, 1}};
        const auto r = chain_runs(s, Mask{1, 1});
        REQUIRE(r.size() == 2 && same(r[0], 0, 64, 0, 1) && same(r[1], 64, 64, 5, 6));
        // ... and blocks contiguous, bins not
        const std::vector<ChainInfo> u = {ChainInfo{64, 0, 0, 1}, ChainInfo{64, 128, 1, 1}};
        REQUIRE(chain_runs(u, Mask{1, 1}).size() == 2);
    }

    // ---- ChainSet::pick at the threshold: 100 bins in all, so that bins == pct
    {
        const std::vector<ChainInfo> h = table({39, 1, 60}, 64);
        const unsigned done[3] = {1u, 0u, 0u}, done2[3] = {1u, 1u, 0u};
        Mask g(3, 7);
        ChainSet a(h, 4);
        REQUIRE(!a.pick(done, 40, g) && a.handed() == 0);           // 39 bins: one short
        REQUIRE(g == (Mask{1, 0, 0}));                              // (marked all the same: final and not taken)
        REQUIRE(a.pick(done2, 40, g) && g == (Mask{1, 1, 0}) && a.handed() == 1);       // 40 * 100 == 100 * 40
        REQUIRE(!a.pick(done2, 1, g) && g == (Mask{0, 0, 0}));      // taken chains are not handed out again
        REQUIRE(!a.pick(done2, 0, g) && a.handed() == 1);           // pct 0, nothing new is final: no empty group
        REQUIRE(a.rest(g) && g == (Mask{0, 0, 1}) && a.handed() == 2);
        REQUIRE(!a.rest(g) && g == (Mask{0, 0, 0}) && a.handed() == 2);
        ChainSet z(h, 4);
        const unsigned none[3] = {0u, 0u, 0u};
        REQUIRE(!z.pick(none, 0, g) && z.handed() == 0);            // pct 0 with no final chain
    }
    // ---- the cap, and clear()
    {
        std::vector<unsigned> done(t.size(), 0u);
        Mask g(t.size(), 0), all(t.size(), 0);
        ChainSet s(t, 2);
        done[0] = 1u;
        REQUIRE(s.pick(done.data(), 0, g) && g == (Mask{1, 0, 0, 0, 0, 0}));
        done[2] = 1u;
        REQUIRE(s.pick(done.data(), 1, g) && g == (Mask{0, 0, 1, 0, 0, 0}));    // 64 of 4418 bins is 1.4 %
        for (unsigned &d : done) d = 1u;
        REQUIRE(!s.pick(done.data(), 1, g) && s.handed() == 2);     // the cap, although four chains are final
        REQUIRE(s.rest(g) && g == (Mask{0, 1, 0, 1, 1, 1}) && s.handed() == 3);
        s.clear();
        REQUIRE(s.rest(g) && g == (Mask{1, 1, 1, 1, 1, 1}) && s.handed() == 4);    // every chain again; the count goes on
        // below the cap, clear() makes pick hand the same chains out again
        ChainSet w(t, MAX_EARLY_TAILS);
        REQUIRE(w.pick(done.data(), 100, g) && g == (Mask{1, 1, 1, 1, 1, 1}));  // exactly 100 %
        REQUIRE(!w.pick(done.data(), 1, g) && !w.rest(g));
        w.clear();
        REQUIRE(w.pick(done.data(), 100, g) && g == (Mask{1, 1, 1, 1, 1, 1}) && w.handed() == 2);
        // every chain goes out exactly once, whatever the order in which they become final
        ChainSet e(t, MAX_EARLY_EPILOGUES);
        std::fill(done.begin(), done.end(), 0u);
        int64_t bins = 0;
        for (size_t i : {5u, 0u, 3u}) {
            done[i] = 1u;
            if (e.pick(done.data(), 1, g))
                for (size_t k = 0; k < t.size(); ++k) { REQUIRE(!(g[k] && all[k])); all[k] |= g[k]; bins += g[k] ? t[k].n : 0; }
        }
        if (e.rest(g))
            for (size_t k = 0; k < t.size(); ++k) { REQUIRE(!(g[k] && all[k])); all[k] |= g[k]; bins += g[k] ? t[k].n : 0; }
        REQUIRE(all == (Mask{1, 1, 1, 1, 1, 1}) && bins == total && e.handed() == 3);     // {5}, {0, 3} ({0} alone is under 1 %), the rest
    }
    // ---- ChainSet::pick_scripted (csr_batch_set_step_groups): the groups in the script's order, each when ALL its chains are final
    {
        // tails of the scattered script of tests/test_gpu_step_schedules.py on six chains: {0, 5}, {2, 3}, {1}; chain 4 remains
        const int32_t script[6] = {0, 2, 1, 1, -1, 0};
        REQUIRE(script_error(script, 6, MAX_EARLY_TAILS) == nullptr);
        std::vector<unsigned> done(t.size(), 0u);
        Mask g(t.size(), 7);
        ChainSet s(t, MAX_EARLY_TAILS);
        REQUIRE(!s.pick_scripted(done.data(), script, g) && s.handed() == 0);
        // groups 1 and 2 are final, group 0 is not: nothing goes out (the order is the script's, not the clock's)
        done[1] = done[2] = done[3] = done[4] = 1u;
        REQUIRE(!s.pick_scripted(done.data(), script, g) && s.handed() == 0);
        done[0] = 1u;                                               // one member of group 0 is final, the other is not
        REQUIRE(!s.pick_scripted(done.data(), script, g) && s.handed() == 0 && g == (Mask{1, 0, 0, 0, 0, 1}));
        done[5] = 1u;
        REQUIRE(s.pick_scripted(done.data(), script, g) && s.handed() == 1 && g == (Mask{1, 0, 0, 0, 0, 1}));
        {
            // a scattered group: two runs, the span over the whole batch, the mask trims what lies between
            const auto r = chain_runs(t, g);
            REQUIRE(r.size() == 2 && same(r[0], 0, 64, 0, 1) && same(r[1], 448, 4160, 7, 72));
            REQUIRE(group_span(r) == std::make_pair((int64_t)0, (int64_t)2));
        }
        REQUIRE(s.pick_scripted(done.data(), script, g) && s.handed() == 2 && g == (Mask{0, 0, 1, 1, 0, 0}));
        {
            const auto r = chain_runs(t, g);                        // two adjacent chains: one run
            REQUIRE(r.size() == 1 && same(r[0], 128, 192, 2, 5));
            REQUIRE(group_span(r) == std::make_pair((int64_t)0, (int64_t)1));
        }
        REQUIRE(s.pick_scripted(done.data(), script, g) && s.handed() == 3 && g == (Mask{0, 1, 0, 0, 0, 0}));
        REQUIRE(!s.pick_scripted(done.data(), script, g) && s.handed() == 3 && g == (Mask{0, 0, 0, 0, 0, 0}));     // no group 3
        REQUIRE(s.rest(g) && g == (Mask{0, 0, 0, 0, 1, 0}) && s.handed() == 4);
        REQUIRE(!s.rest(g) && s.handed() == 4);
    }
    {
        // a group whose runs lie in the second wavefront-group only, behind chains that are not in it
        const std::vector<ChainInfo> far = table({4096, 64, 65, 1}, 64);    // blocks 0-63, 64, 65-66, 67
        const int32_t script[4] = {-1, 0, -1, 0};
        const unsigned done[4] = {0u, 1u, 0u, 1u};
        Mask g(4, 0);
        ChainSet s(far, MAX_EARLY_TAILS);
        REQUIRE(s.pick_scripted(done, script, g) && g == (Mask{0, 1, 0, 1}));
        const auto r = chain_runs(far, g);
        REQUIRE(r.size() == 2 && same(r[0], 4096, 64, 64, 65) && same(r[1], 4288, 64, 67, 68));
        REQUIRE(group_span(r) == std::make_pair((int64_t)1, (int64_t)1));
        REQUIRE(s.rest(g) && g == (Mask{1, 0, 1, 0}));
    }
    {
        // every chain in group 0: it goes out when the last chain is final, and no remainder is left
        const int32_t script[6] = {0, 0, 0, 0, 0, 0};
        std::vector<unsigned> done(t.size(), 1u);
        Mask g(t.size(), 0);
        ChainSet s(t, MAX_EARLY_EPILOGUES);
        done[3] = 0u;
        REQUIRE(!s.pick_scripted(done.data(), script, g) && s.handed() == 0);
        done[3] = 1u;
        REQUIRE(s.pick_scripted(done.data(), script, g) && g == (Mask{1, 1, 1, 1, 1, 1}) && s.handed() == 1);
        REQUIRE(!s.pick_scripted(done.data(), script, g) && !s.rest(g) && s.handed() == 1);
        // ... and none: all -1, everything is the remainder
        const int32_t none[6] = {-1, -1, -1, -1, -1, -1};
        ChainSet z(t, MAX_EARLY_EPILOGUES);
        REQUIRE(script_error(none, 6, MAX_EARLY_EPILOGUES) == nullptr);
        REQUIRE(!z.pick_scripted(done.data(), none, g) && z.handed() == 0);
        REQUIRE(z.rest(g) && g == (Mask{1, 1, 1, 1, 1, 1}) && z.handed() == 1);
    }
    {
        // the cap: six singleton groups of six chains is what a script may hold for tails; a ChainSet with a smaller cap stops there
        const int32_t script[6] = {5, 4, 3, 2, 1, 0};
        REQUIRE(script_error(script, 6, MAX_EARLY_TAILS) == nullptr && script_error(script, 6, MAX_EARLY_TAILS - 1) != nullptr);
        std::vector<unsigned> done(t.size(), 1u);
        Mask g(t.size(), 0);
        ChainSet s(t, MAX_EARLY_TAILS);
        for (int k = 0; k < 6; ++k) {
            REQUIRE(s.pick_scripted(done.data(), script, g) && s.handed() == k + 1);
            for (int i = 0; i < 6; ++i) REQUIRE(g[(size_t)i] == (i == 5 - k));
        }
        REQUIRE(!s.pick_scripted(done.data(), script, g) && !s.rest(g) && s.handed() == 6);
        ChainSet small(t, 2);
        REQUIRE(small.pick_scripted(done.data(), script, g) && small.pick_scripted(done.data(), script, g));
        REQUIRE(!small.pick_scripted(done.data(), script, g) && small.handed() == 2);       // the cap, although group 2 is final
        REQUIRE(small.rest(g) && g == (Mask{1, 1, 1, 1, 0, 0}) && small.handed() == 3);
        // clear() after some groups (a bail-out): every chain is to be done again as ONE remainder; the count goes on, so the
        // scripted pick does not hand the groups that went out a second time and no slot is used twice
        ChainSet b(t, MAX_EARLY_TAILS);
        REQUIRE(b.pick_scripted(done.data(), script, g) && b.pick_scripted(done.data(), script, g) && b.handed() == 2);
        b.clear();
        REQUIRE(b.rest(g) && g == (Mask{1, 1, 1, 1, 1, 1}) && b.handed() == 3);
        ChainSet b2(t, MAX_EARLY_TAILS);
        REQUIRE(b2.pick_scripted(done.data(), script, g) && b2.handed() == 1);
        b2.clear();
        REQUIRE(b2.pick_scripted(done.data(), script, g) && g == (Mask{0, 0, 0, 0, 1, 0}) && b2.handed() == 2);   // group 1, not group 0 again
    }
    // ---- script_error: what csr_batch_set_step_groups rejects
    {
        const int32_t below[3] = {0, -2, -1}, atCap[3] = {0, 1, MAX_EARLY_TAILS}, hole[3] = {0, 2, -1}, noZero[3] = {1, -1, -1};
        const int32_t ok[3] = {1, 0, 1}, top[8] = {0, 1, 2, 3, 4, 5, 6, 7};
        REQUIRE(script_error(below, 3, MAX_EARLY_TAILS) != nullptr && script_error(atCap, 3, MAX_EARLY_TAILS) != nullptr);
        REQUIRE(script_error(hole, 3, MAX_EARLY_TAILS) != nullptr && script_error(noZero, 3, MAX_EARLY_TAILS) != nullptr);
        REQUIRE(script_error(ok, 3, MAX_EARLY_TAILS) == nullptr && script_error(atCap, 3, MAX_EARLY_EPILOGUES) != nullptr);   // (a hole under the larger cap)
        REQUIRE(script_error(top, 8, MAX_EARLY_EPILOGUES) == nullptr && script_error(top, 8, MAX_EARLY_TAILS) != nullptr);
        REQUIRE(script_error(ok, 0, MAX_EARLY_TAILS) == nullptr);
    }
    printf("step_groups_check ok\n");
    return 0;
}
