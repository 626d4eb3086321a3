// csr_chain_tracks.h -- which chains of a batch hold a resident per-chain track (scores, selection mask, null template) and which
// of them a call's chain mask takes.  Plain C++17, standard library only: tests/chain_tracks_check.cpp compiles it without HIP.
// The device array that goes with the flags is ChainTrack<T> (csr_lib.hip).
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>

// Presence of a track, chain by chain.  Empty until the track is allocated: no chain has one then.
struct ChainFlags {
    std::vector<char> have;
    bool has(int chain) const { return chain >= 0 && (size_t)chain < have.size() && have[(size_t)chain] != 0; }
    void set(int chain, bool on) { have[(size_t)chain] = on ? 1 : 0; }
    void clear_all() { std::fill(have.begin(), have.end(), (char)0); }
};

// idx := the chains of 0 .. nc-1 that chain_mask takes (nullptr: every chain), in order.  Returns -1, or the first taken chain
// without the track; idx then holds the taken chains in front of it.
inline int take_chains(int nc, const unsigned char *chain_mask, const ChainFlags &track, std::vector<int> &idx) {
    idx.clear();
    for (int i = 0; i < nc; ++i) {
        if (chain_mask && !chain_mask[i]) continue;
        if (!track.has(i)) return i;
        idx.push_back(i);
    }
    return -1;
}

// out[idx[k]] := compact[k]: the results of the taken chains go back to their places, the others stay untouched
template <class T>
inline void scatter_chains(const std::vector<int> &idx, const T *compact, T *out) {
    for (size_t k = 0; k < idx.size(); ++k) out[idx[k]] = compact[k];
}
