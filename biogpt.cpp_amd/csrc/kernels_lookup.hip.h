// Prompt-lookup speculative decoding (biogpt_hip_generate_lookup; transformers' generate(prompt_lookup_num_tokens, max_matching_ngram_size)): the draft
// and the acceptance on the device, inside the captured step.  No reference counterpart (biogpt.cpp decodes one token per pass).
//
// Sequence s owns the K / V cache slot s and a text T = corpus ++ prompt ++ generated of length L in LookupBufs::text; T[L - 1] is its current token at
// position n_past (SeqState).  A step is
//
//   lookup_draft_kernel     one workgroup per sequence.  For n = max_ngram .. 1: the positions i in [0, L - n - 1] striped over the threads, each tests
//                           T[i .. i + n) against the tail T[L - n .. L) (the tail in LDS), a workgroup min-reduction gives the smallest matching i; the
//                           first n with a match wins.  The draft is T[i + n .. i + n + d), d = min(max_draft, L - (i + n), n_predict - n_gen - 1): every
//                           drafted position lies inside the sequence's cache.  Writes the 1 + max_draft packed column states of the sequence: column j <= d
//                           carries {j == 0 ? current token : draft[j - 1], n_past + j, slot s, t_vis = n_past + j + 1}; the columns beyond 1 + d are exact
//                           copies of column 0 (the grid of the pass is fixed: they write the same K / V row with the same values).  A finished sequence
//                           drafts nothing.
//   (the packed pass with every row's logits: ForwardPass::packed_verify)
//   lookup_accept_kernel    one workgroup per sequence.  a_j = arg-max of row j (row_argmax, kernels_rows.hip.h, as argmax_rows_kernel), for j = 0, 1, ... while
//                           j <= d and every draft before matched (the rows behind the first mismatch are never read).  a_0 .. a_m are appended to seq_gen
//                           and to T, cut at n_predict and behind the first eos_id; the column moves on by the number of tokens appended.  Counters:
//                           passes + 1, drafted + d, accepted + (tokens appended - 1: the drafted tokens that reached the output), so a sequence's
//                           output length is passes + accepted.  A sequence that finishes counts LookupCtl::n_live down; LookupCtl::max_pos follows the
//                           furthest position (the host bounds the attention of later steps by it).
//
// Rejected columns' K / V rows are not rolled back: position p's row is only visible to columns at positions >= p, and a pass that holds such a column
// of the sequence also holds its column at p, which rewrites the row first.  tests/lookup_ref.py restates both kernels.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "kernels.hip.h"
#include "kernels_rows.hip.h"

namespace bgk {

constexpr int LK_MAX_DRAFT = 15;      // drafted tokens of a pass per sequence, at most (16 columns)
constexpr int LK_MAX_NGRAM = 8;
constexpr int LK_DRAFT_THREADS = 256;
constexpr int LK_ACCEPT_THREADS = 1024;

struct LookupCtl {
    int32_t max_draft, max_ngram;
    int32_t eos_id;            // < 0: none
    int32_t n_predict;
    int32_t n_live;            // sequences still running: the host reads {n_live, max_pos} between groups of steps
    int32_t max_pos;           // the furthest n_past of any sequence
    int32_t pad[2];
};

struct LookupSeq {
    int32_t text_off;          // where the sequence's text starts in LookupBufs::text
    int32_t base_len;          // corpus + prompt tokens: L = base_len + n_gen
    int32_t finished;
    int32_t d;                 // drafted tokens of the pass in flight
    int32_t passes, drafted, accepted;
    int32_t pad;
    int32_t draft[LK_MAX_DRAFT + 1];   // -1 behind d
};

__global__ __launch_bounds__(LK_DRAFT_THREADS) void lookup_draft_kernel(const LookupCtl *ctl, LookupSeq *ls, const int32_t *text, const SeqState *seq,
                                                                        SeqState *cols) {
    __shared__ int32_t tail[LK_MAX_NGRAM];
    __shared__ int wmin[LK_DRAFT_THREADS / 64];
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    LookupSeq *q = ls + s;
    const SeqState cur = seq[s];
    const int md = ctl->max_draft;
    const int32_t *T = text + q->text_off;
    const int L = q->base_len + cur.n_gen;
    const int room = ctl->n_predict - cur.n_gen - 1;
    int best = -1, bn = 0;
    if (!q->finished && md > 0 && room > 0) {
        for (int n = min(ctl->max_ngram, L - 1); n >= 1; n--) {
            if (tid < n) tail[tid] = T[L - n + tid];
            __syncthreads();
            int mine = 0x7fffffff;
            for (int i = tid; i <= L - n - 1; i += LK_DRAFT_THREADS) {      // ascending i: the first match of a thread is its smallest
                bool eq = true;
                for (int k = 0; k < n && eq; k++) eq = T[i + k] == tail[k];
                if (eq) { mine = i; break; }
            }
            for (int off = 32; off > 0; off >>= 1) mine = min(mine, __shfl_xor(mine, off, 64));
            if (lane == 0) wmin[wv] = mine;
            __syncthreads();
            int m = wmin[0];
            for (int w = 1; w < LK_DRAFT_THREADS / 64; w++) m = min(m, wmin[w]);
            __syncthreads();      // tail / wmin are rewritten by the next n
            if (m != 0x7fffffff) { best = m; bn = n; break; }      // m is the same in every thread
        }
    }
    const int d = best < 0 ? 0 : max(0, min(md, min(L - (best + bn), room)));
    const int32_t *src = T + best + bn;      // read only where j < d
    if (tid <= LK_MAX_DRAFT) q->draft[tid] = tid < d ? src[tid] : -1;
    if (tid == 0) q->d = d;
    if (tid <= md) {
        SeqState c{};
        const int j = tid <= d ? tid : 0;
        c.token = j == 0 ? cur.token : src[j - 1];
        c.n_past = cur.n_past + j;
        c.seq_id = s;
        c.t_vis = cur.n_past + j + 1;
        cols[(size_t)s * (md + 1) + tid] = c;
    }
}

__global__ __launch_bounds__(LK_ACCEPT_THREADS) void lookup_accept_kernel(LookupCtl *ctl, LookupSeq *ls, int32_t *text, const float *logits, int ld, int n_vocab,
                                                                          SeqState *seq, int32_t *gen_ids, int gen_stride) {
    __shared__ int32_t am[LK_MAX_DRAFT + 1];
    const int s = blockIdx.x, tid = threadIdx.x;
    LookupSeq *q = ls + s;
    if (q->finished) return;
    const int md = ctl->max_draft, d = q->d;
    int m = 0;      // drafts accepted so far; rows 0 .. m get their arg-max
    for (int j = 0; j <= d; j++) {
        float bv;
        int bi;
        row_argmax<LK_ACCEPT_THREADS>(logits + ((size_t)s * (md + 1) + j) * ld, n_vocab, bv, bi);
        const int id = bi == ROW_NONE_I ? 0 : bi;      // (a row of NaNs only)
        if (tid == 0) am[j] = id;
        __syncthreads();      // row_argmax's words are written again by the next row
        if (!(j < d && q->draft[j] == id)) break;      // (the same pair in every thread)
        m = j + 1;
    }
    if (tid == 0) {
        SeqState *st = seq + s;
        const int g = st->n_gen, np = ctl->n_predict, eos = ctl->eos_id;
        int32_t *T = text + q->text_off + q->base_len;
        int e = 0, fin = 0;
        for (int j = 0; j <= m && g + e < np; j++) {
            const int32_t id = am[j];
            gen_ids[(size_t)s * gen_stride + g + e] = id;
            T[g + e] = id;
            e++;
            if (eos >= 0 && id == eos) { fin = 1; break; }
        }
        if (g + e >= np) fin = 1;
        q->passes += 1; q->drafted += d; q->accepted += e > 0 ? e - 1 : 0;
        if (e > 0) {
            st->n_gen = g + e;
            st->token = am[e - 1];
            st->n_past += e;
            atomicMax(&ctl->max_pos, st->n_past);
        }
        if (fin) { q->finished = 1; atomicSub(&ctl->n_live, 1); }
    }
}

}  // namespace bgk
