// The trie of trie-constrained generation (biogpt_hip_generate_beam_trie / biogpt_hip_generate_sample_trie; INTEGRATION.md, "Constrained
// decoding"): a closed set of token sequences in CSR form, built and walked on the host.  Host-only: no HIP header is included and no HIP call is
// made here; the engine uploads the arrays on first use on a device (trie_device, engine.hip) and leaves the copy with the handle.
#pragma once

#include "host_common.h"

// Node u's edges are [first[u], first[u + 1]) of tok (ascending) and child; node 0 is the root.  Nodes are numbered breadth first, so a node's
// children are consecutive.
struct biogpt_hip_trie {
    int32_t n_vocab = 0;
    int64_t n_entries = 0, max_depth = 0, max_fanout = 0;
    std::vector<int32_t> first;      // [n_nodes + 1]
    std::vector<int32_t> tok, child; // [n_edges]
    std::vector<uint8_t> term;       // [n_nodes]: 1 where an entry ends
    std::vector<uint32_t> used;      // one bit per token: it occurs in some entry
    // the device copies: one block per device, freed through the function the uploader left (this file makes no HIP call)
    struct DeviceCopy { int device; void *block; };
    std::vector<DeviceCopy> copies;
    void (*free_copy)(int device, void *block) = nullptr;

    int64_t n_nodes() const { return (int64_t)term.size(); }
    int64_t n_edges() const { return (int64_t)tok.size(); }
    bool uses(int32_t t) const { return t >= 0 && t < n_vocab && ((used[(size_t)t >> 5] >> (t & 31)) & 1u); }
};

namespace bg {

// the node the walk over gen[0 .. n_gen) ends at, -1 where it leaves the trie
int64_t trie_walk(const biogpt_hip_trie *t, const int32_t *gen, int32_t n_gen);

}  // namespace bg
