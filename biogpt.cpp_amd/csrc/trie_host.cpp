// The trie of trie-constrained generation on the host: build (sort, merge, CSR breadth first), info, the allowed set.  biogpt_hip_trie_allowed_host
// is the definition trie_rows_kernel (kernels_trie.hip.h) restates.  No HIP header, no HIP call.
#include "trie_host.h"

#include <algorithm>
#include <numeric>

namespace bg {

int64_t trie_walk(const biogpt_hip_trie *t, const int32_t *gen, int32_t n_gen) {
    int64_t u = 0;
    for (int32_t i = 0; i < n_gen; i++) {
        const int32_t *lo = t->tok.data() + t->first[(size_t)u], *hi = t->tok.data() + t->first[(size_t)u + 1];
        const int32_t *at = std::lower_bound(lo, hi, gen[i]);
        if (at == hi || *at != gen[i]) return -1;
        u = t->child[(size_t)(at - t->tok.data())];
    }
    return u;
}

}  // namespace bg

using bg::clear_error;

extern "C" {

biogpt_hip_trie *biogpt_hip_trie_build(const int32_t *seqs, const int32_t *lens, int32_t n_seqs, int32_t n_vocab) {
    clear_error();
    if (!seqs) BG_FAIL(nullptr, "seqs is NULL");
    if (!lens) BG_FAIL(nullptr, "lens is NULL");
    if (n_seqs < 1) BG_FAIL(nullptr, "n_seqs must be >= 1: a trie holds at least one entry");
    if (n_vocab < 1) BG_FAIL(nullptr, "n_vocab must be >= 1");
    std::vector<int64_t> off((size_t)n_seqs + 1, 0);
    for (int32_t s = 0; s < n_seqs; s++) {
        if (lens[s] < 1) BG_FAIL(nullptr, "lens[%d] = %d: an entry holds at least one token", s, lens[s]);
        off[(size_t)s + 1] = off[(size_t)s] + lens[s];
        if (off[(size_t)s + 1] > INT32_MAX) BG_FAIL(nullptr, "lens: the entries hold more than %d tokens together", INT32_MAX);
        for (int32_t i = 0; i < lens[s]; i++) {
            const int32_t t = seqs[off[(size_t)s] + i];
            if (t < 0 || t >= n_vocab) BG_FAIL(nullptr, "seqs: token %d of entry %d is %d, out of range [0, %d)", i, s, t, n_vocab);
        }
    }
    // the entries in lexicographic order (a prefix before its extensions), duplicates dropped
    auto less = [&](int32_t a, int32_t b) {
        return std::lexicographical_compare(seqs + off[(size_t)a], seqs + off[(size_t)a + 1], seqs + off[(size_t)b], seqs + off[(size_t)b + 1]);
    };
    auto same = [&](int32_t a, int32_t b) {
        return lens[a] == lens[b] && std::equal(seqs + off[(size_t)a], seqs + off[(size_t)a + 1], seqs + off[(size_t)b]);
    };
    std::vector<int32_t> order((size_t)n_seqs);
    std::iota(order.begin(), order.end(), 0);
    std::sort(order.begin(), order.end(), less);
    order.erase(std::unique(order.begin(), order.end(), same), order.end());

    biogpt_hip_trie *t = new biogpt_hip_trie();
    t->n_vocab = n_vocab;
    t->n_entries = (int64_t)order.size();
    t->used.assign(((size_t)n_vocab + 31) >> 5, 0u);
    // breadth first: a node is the run [lo, hi) of sorted entries that share its depth tokens; its children are the runs of equal next token
    struct Run { int32_t lo, hi, depth; };
    std::vector<Run> nodes{Run{0, (int32_t)order.size(), 0}};
    t->first.push_back(0);
    for (size_t u = 0; u < nodes.size(); u++) {
        const Run r = nodes[u];
        int32_t at = r.lo;
        uint8_t term = 0;
        if (lens[order[(size_t)at]] == r.depth) { term = 1; at++; }      // (the entry that ends here sorts first, and there is one at most)
        t->term.push_back(term);
        int64_t fan = 0;
        while (at < r.hi) {
            const int32_t tk = seqs[off[(size_t)order[(size_t)at]] + r.depth];
            int32_t end = at + 1;
            while (end < r.hi && seqs[off[(size_t)order[(size_t)end]] + r.depth] == tk) end++;
            t->tok.push_back(tk);
            t->child.push_back((int32_t)nodes.size());
            t->used[(size_t)tk >> 5] |= 1u << (tk & 31);
            nodes.push_back(Run{at, end, r.depth + 1});
            at = end;
            fan++;
        }
        t->first.push_back((int32_t)t->tok.size());
        t->max_fanout = std::max(t->max_fanout, fan);
        t->max_depth = std::max<int64_t>(t->max_depth, r.depth);
    }
    return t;
}

void biogpt_hip_trie_free(biogpt_hip_trie *trie) {
    if (!trie) return;
    for (const auto &c : trie->copies)
        if (trie->free_copy) trie->free_copy(c.device, c.block);
    delete trie;
}

int biogpt_hip_trie_info(const biogpt_hip_trie *trie, int64_t out[5]) {
    clear_error();
    if (!trie) BG_FAIL(-1, "trie is NULL");
    if (!out) BG_FAIL(-1, "out is NULL");
    out[0] = trie->n_entries; out[1] = trie->n_nodes(); out[2] = trie->n_edges(); out[3] = trie->max_depth; out[4] = trie->max_fanout;
    return 0;
}

int biogpt_hip_trie_allowed_host(const biogpt_hip_trie *trie, const int32_t *gen, int32_t n_gen, int32_t eos_id, int32_t *out_ids, int32_t cap) {
    clear_error();
    if (!trie) BG_FAIL(-1, "trie is NULL");
    if (n_gen < 0) BG_FAIL(-1, "n_gen must be >= 0");
    if (n_gen > 0 && !gen) BG_FAIL(-1, "gen is NULL with n_gen = %d", n_gen);
    if (eos_id < 0 || eos_id >= trie->n_vocab) BG_FAIL(-1, "eos_id %d out of range: must be in [0, %d)", eos_id, trie->n_vocab);
    if (cap < 0) BG_FAIL(-1, "cap must be >= 0");
    if (cap > 0 && !out_ids) BG_FAIL(-1, "out_ids is NULL with cap = %d", cap);
    int32_t n = 0;
    auto put = [&](int32_t id) { if (n < cap) out_ids[n] = id; n++; };
    const int64_t u = bg::trie_walk(trie, gen, n_gen);
    if (u < 0) { put(eos_id); return n; }      // the walk left the trie
    bool eos = trie->term[(size_t)u] != 0;      // EOS where an entry ends, merged into the ascending edge tokens
    for (int32_t e = trie->first[(size_t)u]; e < trie->first[(size_t)u + 1]; e++) {
        const int32_t tk = trie->tok[(size_t)e];
        if (eos && eos_id <= tk) { put(eos_id); eos = false; if (eos_id == tk) continue; }
        put(tk);
    }
    if (eos) put(eos_id);
    return n;
}

}  // extern "C"
