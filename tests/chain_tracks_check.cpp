// Stand-alone check of consenrich_amd/csrc/csr_chain_tracks.h (tests/test_abi_and_host.py compiles it with
// g++ -std=c++17 -fsanitize=address,undefined and runs it): the presence flags of a per-chain track, the walk over the chains a
// mask takes, and the scatter of compact results.  No HIP, no GPU.
#include "csr_chain_tracks.h"

#include <cstdio>
#include <cstdlib>

#define REQUIRE(cond)                                                              \
    do {                                                                           \
        if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

using Idx = std::vector<int>;

int main() {
    const int nc = 4;
    // a track nobody allocated: no chain has one, whatever is asked (out-of-range chains included)
    ChainFlags none;
    REQUIRE(!none.has(0) && !none.has(3) && !none.has(-1) && !none.has(4));
    Idx idx{7, 7};
    REQUIRE(take_chains(nc, nullptr, none, idx) == 0 && idx.empty());
    const unsigned char zero[nc] = {0, 0, 0, 0};
    REQUIRE(take_chains(nc, zero, none, idx) == -1 && idx.empty());      // nothing taken: nothing can be missing

    // every chain holds the track
    ChainFlags all;
    all.have.assign(nc, 0);
    REQUIRE(!all.has(0) && !all.has(3));
    for (int i = 0; i < nc; ++i) all.set(i, true);
    REQUIRE(all.has(0) && all.has(3) && !all.has(-1) && !all.has(nc));
    REQUIRE(take_chains(nc, nullptr, all, idx) == -1 && idx == (Idx{0, 1, 2, 3}));        // null mask: every chain, in order
    REQUIRE(take_chains(nc, zero, all, idx) == -1 && idx.empty());
    const unsigned char first[nc] = {1, 0, 0, 0}, last[nc] = {0, 0, 0, 1}, odd[nc] = {0, 5, 0, 255};
    REQUIRE(take_chains(nc, first, all, idx) == -1 && idx == (Idx{0}));
    REQUIRE(take_chains(nc, last, all, idx) == -1 && idx == (Idx{3}));
    REQUIRE(take_chains(nc, odd, all, idx) == -1 && idx == (Idx{1, 3}));                  // any non-zero byte takes

    // chains 1 and 3 lack the track
    ChainFlags some = all;
    some.set(1, false);
    some.set(3, false);
    REQUIRE(take_chains(nc, nullptr, some, idx) == 1 && idx == (Idx{0}));                 // WHICH chain: the first in order
    REQUIRE(take_chains(nc, last, some, idx) == 3 && idx.empty());
    const unsigned char even[nc] = {1, 0, 1, 0}, tail[nc] = {0, 0, 1, 1};
    REQUIRE(take_chains(nc, even, some, idx) == -1 && idx == (Idx{0, 2}));                // untaken chains may lack it
    REQUIRE(take_chains(nc, tail, some, idx) == 3 && idx == (Idx{2}));
    some.clear_all();
    REQUIRE(some.have.size() == (size_t)nc && !some.has(0) && !some.has(2));
    REQUIRE(take_chains(nc, first, some, idx) == 0);

    // the scatter writes the taken places and nothing else
    REQUIRE(take_chains(nc, odd, all, idx) == -1);
    const double compact[2] = {10.5, 30.5};
    double out[nc] = {-1.0, -2.0, -3.0, -4.0};
    scatter_chains(idx, compact, out);
    REQUIRE(out[0] == -1.0 && out[1] == 10.5 && out[2] == -3.0 && out[3] == 30.5);
    scatter_chains(Idx{}, compact, out);
    REQUIRE(out[0] == -1.0 && out[1] == 10.5 && out[2] == -3.0 && out[3] == 30.5);
    struct Rec { int a; double b; };
    const Rec rc[1] = {{4, 0.25}};
    Rec ro[nc] = {{0, 0.0}, {0, 0.0}, {0, 0.0}, {0, 0.0}};
    REQUIRE(take_chains(nc, last, all, idx) == -1);
    scatter_chains(idx, rc, ro);
    REQUIRE(ro[3].a == 4 && ro[3].b == 0.25 && ro[0].a == 0 && ro[2].a == 0);

    printf("chain_tracks_check ok\n");
    return 0;
}
