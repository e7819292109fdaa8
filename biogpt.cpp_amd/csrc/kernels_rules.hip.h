// Generation rules (biogpt_hip_generate_beam_rules / biogpt_hip_generate_sample_rules): transformers' logits processors of the same names on
// the device, inside the captured step, between the forward pass and the selection ("Generation rules").
//
//   rules_rows_kernel    one workgroup per row (column) of logits_all, in place.  The row's history h is its prompt (one copy per prompt in the
//                        rules buffer, shared by the prompt's samples and by all beams) followed by its generated tokens (seq_gen), L = len(h):
//                          mode 1 only    the row becomes its log-probabilities first: (float)(((double)l - m) - log S), the formula of
//                                         beam_group_rows_kernel through the same lp_row_stats (on the row kernels' shared pieces, kernels_rows.hip.h); its GIVEN form then takes the values as they are
//                          penalty        every DISTINCT token of h once: s < 0 ? s * p : s / p (f32, IEEE division).  A bitmap of n_vocab bits in
//                                         LDS, set with atomicOr: the thread that finds the bit clear applies the penalty
//                          n-gram         every position i in [0, L - n] whose n - 1 tokens equal the last n - 1 of h bans h[i + n - 1]
//                          min new / suppress   -inf at the EOS id while fewer than m tokens are generated / at every listed id
//                        The penalty comes first (a barrier apart); the bans only write -inf, in any order.
//   rules_apply_row      the penalty, the n-gram ban and the two -inf rules as a __device__ function of the row, the history accessor h(i), L, n_gen and the
//                        rule values: rules_rows_kernel runs it with the call's values, queue_req_rows_kernel (kernels_queue.hip.h) with a column's own.
//
// The grid is fixed and every value is read from device memory (RulesCtl, SeqState, the histories): the launch is capturable, and a captured
// step serves every call whose rule set switches the same kernels in.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "kernels.hip.h"
#include "kernels_score.hip.h"
#include "kernels_beam.hip.h"

namespace bgk {

constexpr int RULES_MAX_SUPPRESS = 256;
constexpr int RULES_MAX_VOCAB = 1 << 18;      // the bitmap: 32 KiB of LDS at most

// uploaded per call; then n_rows RulesRow, then the prompts' tokens
struct RulesCtl {
    float penalty;            // 1.0: off
    int32_t ngram;            // 0: off
    int32_t min_new;          // 0: off (and off without an EOS id)
    int32_t n_suppress;
    int32_t eos_id;           // < 0: none
    int32_t mode;             // 0: the rows are logits; 1: they become log-probabilities first
    int32_t pad[2];
    int32_t suppress[RULES_MAX_SUPPRESS];
};

struct RulesRow {
    int32_t off;              // first token of the row's prompt in the prompt words
    int32_t n_prompt;
};

// The rules on one row, by the THREADS threads of its workgroup: h(i) is token i of the row's history of L tokens, n_gen of them generated; seen: the
// bitmap, (n_vocab + 31) / 32 words of LDS.  rules_rows_kernel calls it with the call's values, queue_req_rows_kernel (kernels_queue.hip.h) with the
// column's own.  Every token used as an index is range-checked.
template <int THREADS, class Hist>
__device__ __forceinline__ void rules_apply_row(float *row, int n_vocab, uint32_t *seen, Hist h, int L, int n_gen, float p, int n, int min_new, int eos,
                                                int n_suppress, const int32_t *suppress) {
    const int tid = threadIdx.x;
    if (p != 1.0f) {
        const int nw = (n_vocab + 31) >> 5;
        for (int w = tid; w < nw; w += THREADS) seen[w] = 0u;
        __syncthreads();
        for (int i = tid; i < L; i += THREADS) {
            const int t = h(i);
            if (t < 0 || t >= n_vocab) continue;
            const uint32_t bit = 1u << (t & 31);
            if (atomicOr(&seen[t >> 5], bit) & bit) continue;      // another position of the same token came first
            const float s = row[t];
            row[t] = s < 0.0f ? s * p : __fdiv_rn(s, p);
        }
        __syncthreads();      // the bans below overwrite penalised entries
    }

    if (n > 0 && L + 1 >= n) {
        const int t0 = L - n + 1;      // the tail h[t0 .. L - 1]: n - 1 tokens
        for (int i = tid; i <= L - n; i += THREADS) {
            bool same = true;
            for (int j = 0; j < n - 1 && same; j++) same = h(i + j) == h(t0 + j);
            const int t = h(i + n - 1);
            if (same && t >= 0 && t < n_vocab) row[t] = -INFINITY;
        }
    }
    if (tid == 0 && eos >= 0 && eos < n_vocab && n_gen < min_new) row[eos] = -INFINITY;
    for (int i = tid; i < n_suppress; i += THREADS) {
        const int t = suppress[i];
        if (t >= 0 && t < n_vocab) row[t] = -INFINITY;
    }
}

// rows: [gridDim.x][ldl], in place; seq: the rows' column states (n_gen = tokens generated); seq_gen: [row][gen_stride] generated tokens;
// skip: nullptr, or a word per row (skip_stride words apart; 0: one word for all) that, non-zero, leaves the row alone (a finished sequence, a
// finished search: nothing reads the row).  Dynamic LDS: (n_vocab + 31) / 32 words.
__global__ __launch_bounds__(LP_THREADS) void rules_rows_kernel(float *rows, int ldl, int n_vocab, const RulesCtl *ctl, const RulesRow *rrow,
                                                                const int32_t *prompt_tok, const SeqState *seq, const int32_t *seq_gen, int gen_stride,
                                                                const int32_t *skip, int skip_stride) {
    extern __shared__ uint32_t seen[];
    __shared__ double s_ls;
    const int r = blockIdx.x, tid = threadIdx.x;
    if (skip && skip[(size_t)r * skip_stride]) return;
    float *row = rows + (size_t)r * ldl;
    const int n_prompt = rrow[r].n_prompt;
    const int32_t *pr = prompt_tok + rrow[r].off;
    const int32_t *gen = seq_gen + (size_t)r * gen_stride;
    const int n_gen = max(0, min(seq[r].n_gen, gen_stride));
    const int L = n_prompt + n_gen;
    auto h = [&](int i) { return i < n_prompt ? pr[i] : gen[i - n_prompt]; };

    if (ctl->mode == 1) {
        float m;
        int bi;
        double S;
        lp_row_stats(row, n_vocab, m, bi, S);
        if (tid == 0) s_ls = log(S);
        __syncthreads();
        const double ls = s_ls, dm = (double)m;
        for (int v = tid; v < n_vocab; v += LP_THREADS) row[v] = (float)(((double)row[v] - dm) - ls);
        __syncthreads();
    }

    rules_apply_row<LP_THREADS>(row, n_vocab, seen, h, L, n_gen, ctl->penalty, ctl->ngram, ctl->min_new, ctl->eos_id, ctl->n_suppress, ctl->suppress);
}

}  // namespace bgk
