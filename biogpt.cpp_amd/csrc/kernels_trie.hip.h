// Trie-constrained generation (biogpt_hip_generate_beam_trie / biogpt_hip_generate_sample_trie): transformers' PrefixConstrainedLogitsProcessor over a
// closed set of token sequences, on the device, inside the captured step, between the forward pass and the selection ("Constrained
// decoding").  The trie is the CSR image of trie_host.h; biogpt_hip_trie_allowed_host is the definition restated here.
//
//   trie_rows_kernel     one workgroup per row (column) of logits_all, in place.  The row's generated tokens g (seq_gen; the prompt is no part of the
//                        walk) are walked from the root, one level per token: the whole workgroup searches the node's ascending edge tokens for g[i],
//                        LP_THREADS-ary -- one probe round where the node has at most LP_THREADS edges, one more per further factor of LP_THREADS --
//                        and the waves exchange the result through LDS (one barrier per round).  A row costs O(depth) dependent rounds.
//                          the walk ends at node u      A = {tokens of u's edges} + {EOS if an entry ends at u}
//                          the walk leaves the trie     A = {EOS}      (only a beam that took a candidate at -inf gets there)
//                        A becomes a bitmap of n_vocab bits in LDS (coalesced loads of the edge list, atomicOr), and ONE pass writes the row: -inf
//                        outside A; inside A the value as it is (mode 0: logits) or its log-probability (mode 1), (float)(((double)l - m) - log S)
//                        through lp_row_stats -- the expression of rules_rows_kernel and beam_group_rows_kernel, the sum over the UNMASKED row as in
//                        transformers' _beam_search.  Only the quads that hold a member of A are read in that pass.
//
// The grid is fixed and every value is read from device memory (TrieCtl, SeqState, the histories): the launch is capturable, and a captured step serves any
// trie.  No scratch.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "kernels.hip.h"
#include "kernels_score.hip.h"
#include "kernels_rules.hip.h"

namespace bgk {

// uploaded per call: where the trie's arrays lie on this device, and the call's EOS id and mode
struct TrieCtl {
    const int32_t *first;     // [n_nodes + 1]
    const int32_t *tok;       // [n_edges], ascending within a node
    const int32_t *child;     // [n_edges]
    const uint8_t *term;      // [n_nodes]
    int32_t n_nodes;
    int32_t eos_id;           // in [0, n_vocab), in no entry
    int32_t mode;             // 0: the rows are logits; 1: they become log-probabilities
    int32_t pad;
};

typedef const int32_t __attribute__((address_space(1))) *trie_gi32;      // (a pointer read from TrieCtl is generic: global loads have to be asked for)
typedef const uint8_t __attribute__((address_space(1))) *trie_gu8;

// The waves' exchange of one search round: `hit` holds in one thread of the workgroup at most, its `val` (>= 0) comes back to every thread, -1 without a
// hit.  One barrier; the rounds alternate between two sets of words, so a wave that runs ahead into the next round writes the other set.
__device__ __forceinline__ int trie_share(bool hit, int val, int &round, int (&s_w)[2][LP_THREADS / 64]) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long b = __ballot(hit);
    const int got = __shfl(val, b ? __ffsll(b) - 1 : 0, 64);
    if (lane == 0) s_w[round & 1][wv] = b ? got : -1;
    __syncthreads();
    int r = -1;
    for (int w = 0; w < LP_THREADS / 64; w++) r = max(r, s_w[round & 1][w]);
    round++;
    return r;
}

// rows: [gridDim.x][ldl], in place; seq: the rows' column states (n_gen = tokens generated); seq_gen: [row][gen_stride] generated tokens; skip: nullptr, or
// a word per row (skip_stride words apart) that, non-zero, leaves the row alone.  Dynamic LDS: (n_vocab + 31) / 32 words.
__global__ __launch_bounds__(LP_THREADS) void trie_rows_kernel(float *rows, int ldl, int n_vocab, const TrieCtl *ctl, const SeqState *seq, const int32_t *seq_gen,
                                                               int gen_stride, const int32_t *skip, int skip_stride) {
    extern __shared__ uint32_t trie_in[];      // the bitmap of A
    __shared__ int s_w[2][LP_THREADS / 64];
    __shared__ double s_ls;
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    if (skip && skip[(size_t)r * skip_stride]) return;
    float *row = rows + (size_t)r * ldl;
    const int32_t *gen = seq_gen + (size_t)r * gen_stride;
    const int n_gen = max(0, min(seq[r].n_gen, gen_stride));
    const trie_gi32 first = (trie_gi32)ctl->first, tok = (trie_gi32)ctl->tok, child = (trie_gi32)ctl->child;
    const int eos = ctl->eos_id, mode = ctl->mode;

    const int nw = (n_vocab + 31) >> 5;
    for (int w = tid; w < nw; w += LP_THREADS) trie_in[w] = 0u;

    // ---- the walk: every thread holds the same node u; -1 once the walk has left the trie ----
    int u = 0, round = 0;
    for (int i = 0; i < n_gen && u >= 0; i++) {
        const int g = gen[i];
        int lo = first[u], hi = first[u + 1];
        while (hi - lo > LP_THREADS) {      // thread t probes the edge t steps in: the probe that holds the last token <= g bounds the next range
            const int step = (hi - lo + LP_THREADS - 1) / LP_THREADS;
            const int p = lo + tid * step;
            const int v = p < hi ? tok[p] : 0x7fffffff;
            int nxt = __shfl_down(v, 1, 64);
            if (lane == 63) nxt = p + step < hi ? tok[p + step] : 0x7fffffff;
            const int at = trie_share(v <= g && g < nxt, tid, round, s_w);
            if (at < 0) { lo = hi = 0; break; }      // g lies in front of the node's first edge
            lo += at * step;
            hi = min(lo + step, hi);
        }
        const int e = lo + tid;
        const bool hit = e < hi && tok[e] == g;
        u = trie_share(hit, hit ? child[e] : 0, round, s_w);
    }
    __syncthreads();      // the bitmap is clear (and the last round's words are read)

    // ---- A as a bitmap ----
    bool with_eos = true;
    if (u >= 0) {
        const int lo = first[u], hi = first[u + 1];
        for (int e = lo + tid; e < hi; e += LP_THREADS) {
            const int t = tok[e];
            if (t >= 0 && t < n_vocab) atomicOr(&trie_in[t >> 5], 1u << (t & 31));
        }
        with_eos = ((trie_gu8)ctl->term)[u] != 0;
    }
    if (tid == 0 && with_eos && eos >= 0 && eos < n_vocab) atomicOr(&trie_in[eos >> 5], 1u << (eos & 31));

    double ls = 0.0, dm = 0.0;
    if (mode == 1) {
        float m;
        int bi;
        double S;
        lp_row_stats(row, n_vocab, m, bi, S);
        if (tid == 0) s_ls = log(S);
        __syncthreads();
        ls = s_ls; dm = (double)m;
    } else {
        __syncthreads();
    }

    // ---- one write pass (the walk of row_scan: head, 16-byte quads, tail): -inf outside A; a quad without a member of A is not read ----
    auto in = [&](int i) { return ((trie_in[i >> 5] >> (i & 31)) & 1u) != 0; };
    auto val = [&](float x) { return mode == 1 ? (float)(((double)x - dm) - ls) : x; };
    const int head = min(n_vocab, (int)(((16u - ((uint32_t)(uintptr_t)row & 15u)) & 15u) >> 2));
    const int nvec = (n_vocab - head) >> 2;
    const int tail0 = head + 4 * nvec;
    float4 *body = reinterpret_cast<float4 *>(row + head);
    if (tid < head) row[tid] = in(tid) ? val(row[tid]) : -INFINITY;
    for (int q = tid; q < nvec; q += LP_THREADS) {
        const int i = head + 4 * q;
        const bool b0 = in(i), b1 = in(i + 1), b2 = in(i + 2), b3 = in(i + 3);
        float4 e = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
        if (b0 || b1 || b2 || b3) {
            const float4 o = body[q];
            if (b0) e.x = val(o.x);
            if (b1) e.y = val(o.y);
            if (b2) e.z = val(o.z);
            if (b3) e.w = val(o.w);
        }
        body[q] = e;
    }
    if (tail0 + tid < n_vocab) row[tail0 + tid] = in(tail0 + tid) ? val(row[tail0 + tid]) : -INFINITY;
}

}  // namespace bgk
