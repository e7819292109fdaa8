// Log-probabilities of generated tokens (biogpt_hip_generate_greedy_batch_lp / biogpt_hip_generate_sample_lp): the selection of a column step that keeps
// what it knew about the row it chose from.  For the logits row l of a step (raw: temperature 1, no top-k / top-p cut), m = max l and
// S = sum_v exp(l[v] - m):
//
//   lp of an id   (l[id] - m) - log(S), in double, rounded once -- the arithmetic of logprob_rows_kernel (kernels_score.hip.h), with S from lp_row_stats /
//                 lp_row_sum themselves: S depends on which lane adds which element, so only the same walk by the same LP_THREADS threads gives the
//                 bits biogpt_hip_score gives
//   top K         the row's first K <= GENLP_MAX_TOP entries in the row kernels' order (kernels_rows.hip.h: value descending, equal values lower id
//                 first), by sample_topk (kernels_sample.hip.h: row_kth_bound + a second walk over the row, on chip by then), each with its lp
//
//   genlp_greedy_rows_kernel   argmax_rows_kernel + the arg-max's lp + the top K: one workgroup per row, one launch
//   sample_lp_rows_kernel      sample_rows_kernel's step (sample_rows_step) selecting max(top_k, K) candidates -- the first top_k are the plain kernel's,
//                              so the draw, the generator's stream and the ids are its own -- + S over the whole row (one more walk: the maximum is the
//                              first candidate) + the drawn token's lp + the top K
//
// Entry g (SeqState::n_gen, as seq_gen) of row r goes to lp[r * stride + g] and top_*[(r * stride + g) * n_top + j]: n_top and stride lie in device
// memory (GenLpCtl), so one captured step serves any K and the call's results are one contiguous block.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "kernels.hip.h"
#include "kernels_rows.hip.h"
#include "kernels_sample.hip.h"
#include "kernels_score.hip.h"

namespace bgk {

constexpr int GENLP_MAX_TOP = 8;
static_assert(SAMPLE_THREADS == LP_THREADS, "the selection and the sum run in one workgroup");
static_assert(GENLP_MAX_TOP <= SAMPLE_MAX_K, "the sampler's candidate list holds the top K");

// the call's request: top entries per token, entries per sequence (the call's n_predict as clamped)
struct GenLpCtl {
    int32_t n_top, stride;
    int32_t pad[2];
};

struct GenLpOut {
    const GenLpCtl *ctl;
    float *lp;            // [rows][stride]
    int32_t *top_ids;     // [rows][stride][n_top]
    float *top_lp;        // [rows][stride][n_top]
};

// Thread 0 (the one that holds S): entry g of row r.  v_id: the chosen id's logit; top_v / top_i: the row's best n_have entries in order.  An entry past
// the stride is dropped; a top entry the row does not have (NaNs are never selected) is (-1, 0).
__device__ __forceinline__ void genlp_write(const GenLpOut &o, int r, int g, float v_id, float m, double S, const float *top_v, const int *top_i, int n_have) {
    const int stride = o.ctl->stride, K = min(o.ctl->n_top, GENLP_MAX_TOP);
    if (g < 0 || g >= stride) return;
    const double log_s = log(S);
    const size_t at = (size_t)r * stride + g;
    o.lp[at] = (float)(((double)v_id - (double)m) - log_s);
    for (int j = 0; j < K; j++) {
        const bool have = j < n_have;
        o.top_ids[at * K + j] = have ? top_i[j] : -1;
        o.top_lp[at * K + j] = have ? (float)(((double)top_v[j] - (double)m) - log_s) : 0.0f;
    }
}

// logits: [rows][ld]; what argmax_rows_kernel does to seq / gen_ids (row r = sequence r), and the entry of out
__global__ __launch_bounds__(LP_THREADS) void genlp_greedy_rows_kernel(const float *logits, int ld, int n_vocab, SeqState *seq, int32_t *gen_ids, int gen_stride,
                                                                       int advance, GenLpOut out) {
    __shared__ float top_v[GENLP_MAX_TOP];
    __shared__ int top_i[GENLP_MAX_TOP];
    const int r = blockIdx.x;
    const float *row = logits + (size_t)r * ld;
    float m;
    int bi;
    double S;
    lp_row_stats(row, n_vocab, m, bi, S);
    const int K = min(min(out.ctl->n_top, GENLP_MAX_TOP), n_vocab);
    int n_have = 0;
    if (K > 0) n_have = sample_topk(row, n_vocab, K, top_v, top_i);      // (uniform; every thread is behind lp_row_sum's barrier)
    if (threadIdx.x == 0) {
        const int id = bi == ROW_NONE_I ? 0 : bi;
        SeqState *s = seq + r;
        const int g = s->n_gen;
        if (g < gen_stride) gen_ids[(size_t)r * gen_stride + g] = id;
        genlp_write(out, r, g, row[id], m, S, top_v, top_i, n_have);
        s->n_gen = g + 1;
        s->token = id;
        s->n_past += advance;
    }
}

// sample_rows_step's addition (SamplePlain, kernels_sample.hip.h)
struct SampleGenLp {
    GenLpOut out;
    float m = 0.0f;
    double S = 1.0;
    __device__ __forceinline__ int also_select() const { return min(out.ctl->n_top, GENLP_MAX_TOP); }
    __device__ __forceinline__ void row_stats(const float *row, int n_vocab, const float *top_v, int k_all) {
        if (k_all > 0) {      // (uniform)
            m = top_v[0];
            lp_row_sum(row, n_vocab, m, S);
        }
    }
    __device__ __forceinline__ void emit(int r, int g, int pick, const float *top_v, const int *top_i, int k_all) {
        genlp_write(out, r, g, k_all > 0 ? top_v[pick] : m, m, S, top_v, top_i, k_all);
    }
};

__global__ __launch_bounds__(SAMPLE_THREADS) void sample_lp_rows_kernel(const float *logits, int ldl, int n_vocab, SampleCtl *ctl, SampleSeq *sq, SeqState *seq,
                                                                        int32_t *seq_gen, int gen_stride, GenLpOut out) {
    sample_rows_step(logits, ldl, n_vocab, ctl, sq, seq, seq_gen, gen_stride, SampleGenLp{out});
}

}  // namespace bgk
