// The distribution at every scored position (biogpt_hip_score_stats / biogpt_hip_score_batch_stats) and the distance between two files on the same text
// (biogpt_hip_score_compare).  Row kernels over the logits rows a scoring pass leaves in logits_all: one workgroup of LP_THREADS per row, no workspace
// beyond the outputs, no atomics on memory, a row's results independent of what else is in the launch.  No reference counterpart.
//
//   score_stats_rows_kernel     logprob_rows_kernel's three outputs from lp_row_stats itself (the same walk by the same threads: the same bits), and
//                                 top K    sample_topk's first K <= GENLP_MAX_TOP entries in the row kernels' order, each with genlp_write's lp
//                                 rank     how many entries come before the target in that order; -1 without a target or where l[t] is NaN
//                                 entropy  H = log(S) - N / S,  S = sum_v e_v,  N = sum_v e_v d_v,  d_v = l[v] - m,  e_v = exp(d_v): all in double
//   score_compare_rows_kernel   two rows p, q of one width per workgroup: lp_row_stats of each (the lp score gives each file), then ONE walk over both,
//                                 kl_pq = A / S_p - log S_p + log S_q,  A = sum_v e_p,v (d_p,v - d_q,v);  kl_qp from the mirror sum B
//
// The walk behind the selection (the row is on chip by then) is row_scan's on a row that lies on a 16-byte boundary and lp_row_sum's fallback on one that
// does not: which lane adds which element follows from the element's index alone, so a row gives the same bits on all four alignments.  A lane holds an
// integer count and two doubles (compare: four doubles) in registers; waves combine through one LDS exchange per quantity behind one barrier.
// Conventions: a term whose weight e is 0 (the entry is -inf, or so far below m that exp gives 0) is skipped -- it contributes 0, not 0 x inf; a positive
// weight against -inf in the other row gives +inf; a NaN anywhere, a +inf anywhere (d = inf - inf) and a row of -inf only give NaN.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "kernels.hip.h"
#include "kernels_genlp.hip.h"
#include "kernels_rows.hip.h"
#include "kernels_sample.hip.h"
#include "kernels_score.hip.h"

namespace bgk {

// what score_stats_rows_kernel adds to logprob_rows_kernel's outputs, already offset to the pass's first column: rank / entropy [N] (either may be null),
// top_ids / top_lp [N][n_top] (read with n_top > 0 only)
struct ScoreStatsOut {
    int32_t n_top;
    int32_t *rank;
    float *entropy;
    int32_t *top_ids;
    float *top_lp;
};

// score_compare_rows_kernel's outputs, [N] each; kl_pq is always written, every other may be null
struct ScoreCmpOut {
    float *kl_pq, *kl_qp, *lp_p, *lp_q;
    int32_t *argmax_p, *argmax_q;
};

// quad(float4, first index) / one(value, index) over a row on any alignment, in the order row_scan gives a row on a 16-byte boundary
template <class Q, class O>
__device__ __forceinline__ void score_row_walk(const float *row, int n, Q quad, O one) {
    if ((((uint32_t)(uintptr_t)row) & 15u) == 0u) {
        row_scan<LP_THREADS>(row, n, quad, one);
    } else {
        const int tid = threadIdx.x, nvec = n >> 2;
        for (int i = tid; i < nvec; i += LP_THREADS) {
            const float *e = row + 4 * i;
            quad(make_float4(e[0], e[1], e[2], e[3]), 4 * i);
        }
        if (4 * nvec + tid < n) one(row[4 * nvec + tid], 4 * nvec + tid);
    }
}

// one entry's share of S and N: e = exp(d) in double; e == 0 contributes nothing
struct ScoreTerm { double e, n; };
__device__ __forceinline__ ScoreTerm score_term(float v, float m) {
    const double d = (double)v - (double)m, e = exp(d);
    return ScoreTerm{e, e != 0.0 ? e * d : 0.0};
}

// the waves' lane totals -> thread 0, in wave order (the other threads return their own wave's total); called by every thread, behind a barrier of its own
template <int NQ>
__device__ __forceinline__ void score_block_sums(double (&v)[NQ]) {
    __shared__ double s_q[NQ][LP_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
#pragma unroll
    for (int k = 0; k < NQ; k++) {
        v[k] = wave_sum_f64(v[k]);
        if (lane == 0) s_q[k][wv] = v[k];
    }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < NQ; k++) {
            v[k] = 0.0;
            for (int w = 0; w < LP_THREADS / 64; w++) v[k] += s_q[k][w];
        }
    }
}

// logits: [N][ldl] floats (N = gridDim.x); targets / lp_out / am_out / lg_out as for logprob_rows_kernel, and bit for bit its values
__global__ __launch_bounds__(LP_THREADS) void score_stats_rows_kernel(const float *logits, int ldl, int n_vocab, const int32_t *targets, float *lp_out,
                                                                      int32_t *am_out, float *lg_out, ScoreStatsOut st) {
    __shared__ float top_v[GENLP_MAX_TOP];
    __shared__ int top_i[GENLP_MAX_TOP];
    __shared__ int s_cnt[LP_THREADS / 64];
    const int col = blockIdx.x, tid = threadIdx.x;
    const float *row = logits + (size_t)col * ldl;
    float m;
    int bi;
    double S;
    lp_row_stats(row, n_vocab, m, bi, S);
    const int n_top = min(st.n_top, GENLP_MAX_TOP), K = min(n_top, n_vocab);
    int n_have = 0;
    if (K > 0) n_have = sample_topk(row, n_vocab, K, top_v, top_i);      // (uniform; every thread is behind lp_row_sum's barrier)
    const int t = targets[col];
    const bool scored = t >= 0 && t < n_vocab;
    const float lt = scored ? row[t] : 0.0f;
    if (tid == 0) {
        const double log_s = log(S);
        lp_out[col] = scored ? (float)(((double)lt - (double)m) - log_s) : 0.0f;
        lg_out[col] = lt;
        am_out[col] = bi == ROW_NONE_I ? 0 : bi;
        for (int j = 0; j < n_top; j++) {      // genlp_write's entries
            const bool have = j < n_have;
            st.top_ids[(size_t)col * n_top + j] = have ? top_i[j] : -1;
            st.top_lp[(size_t)col * n_top + j] = have ? (float)(((double)top_v[j] - (double)m) - log_s) : 0.0f;
        }
    }
    if (!st.rank && !st.entropy) return;      // (uniform)

    // ---- rank and entropy: one walk, an integer and two doubles per lane ----
    int cnt = 0;
    double acc[2] = {0.0, 0.0};      // S, N
    const bool ranked = scored && lt == lt;
    score_row_walk(
        row, n_vocab,
        [&](float4 q, int i) {
            const ScoreTerm x = score_term(q.x, m), y = score_term(q.y, m), z = score_term(q.z, m), w = score_term(q.w, m);
            acc[0] += (x.e + y.e) + (z.e + w.e);
            acc[1] += (x.n + y.n) + (z.n + w.n);
            cnt += (row_before(q.x, i, lt, t) ? 1 : 0) + (row_before(q.y, i + 1, lt, t) ? 1 : 0) + (row_before(q.z, i + 2, lt, t) ? 1 : 0) +
                   (row_before(q.w, i + 3, lt, t) ? 1 : 0);
        },
        [&](float v, int i) {
            const ScoreTerm x = score_term(v, m);
            acc[0] += x.e;
            acc[1] += x.n;
            cnt += row_before(v, i, lt, t) ? 1 : 0;
        });
    cnt = wave_xor_sum(cnt, 64);
    if ((tid & 63) == 0) s_cnt[tid >> 6] = cnt;
    score_block_sums(acc);      // (its barrier publishes s_cnt)
    if (tid == 0) {
        if (st.rank) {
            int r = 0;
            for (int w = 0; w < LP_THREADS / 64; w++) r += s_cnt[w];
            st.rank[col] = ranked ? r : -1;
        }
        if (st.entropy) st.entropy[col] = (float)(log(acc[0]) - acc[1] / acc[0]);
    }
}

// p: [N][ldp], q: [N][ldq] floats, rows of n_vocab (N = gridDim.x); targets [N] (negative: lp_p = lp_q = 0)
__global__ __launch_bounds__(LP_THREADS) void score_compare_rows_kernel(const float *p, int ldp, const float *q, int ldq, int n_vocab, const int32_t *targets,
                                                                        ScoreCmpOut out) {
    const int col = blockIdx.x, tid = threadIdx.x;
    const float *rp = p + (size_t)col * ldp, *rq = q + (size_t)col * ldq;
    float m_p, m_q;
    int bi_p, bi_q;
    double S_p, S_q;
    lp_row_stats(rp, n_vocab, m_p, bi_p, S_p);
    __syncthreads();      // block_best's and lp_row_sum's words are written again
    lp_row_stats(rq, n_vocab, m_q, bi_q, S_q);
    if (tid == 0) {
        const int t = targets[col];
        const bool scored = t >= 0 && t < n_vocab;
        if (out.lp_p) out.lp_p[col] = scored ? (float)(((double)rp[t] - (double)m_p) - log(S_p)) : 0.0f;
        if (out.lp_q) out.lp_q[col] = scored ? (float)(((double)rq[t] - (double)m_q) - log(S_q)) : 0.0f;
        if (out.argmax_p) out.argmax_p[col] = bi_p == ROW_NONE_I ? 0 : bi_p;
        if (out.argmax_q) out.argmax_q[col] = bi_q == ROW_NONE_I ? 0 : bi_q;
    }

    // ---- the fused walk: quad i of both rows to thread i % LP_THREADS, 16-byte loads where both rows lie on a boundary; S_p, S_q, A, B per lane ----
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    auto term = [&](float a, float b) {
        const double dp = (double)a - (double)m_p, dq = (double)b - (double)m_q;
        const double ep = exp(dp), eq = exp(dq);
        acc[0] += ep;
        acc[1] += eq;
        if (ep != 0.0) acc[2] += ep * (dp - dq);
        if (eq != 0.0) acc[3] += eq * (dq - dp);
    };
    const bool vec = ((((uint32_t)(uintptr_t)rp) | ((uint32_t)(uintptr_t)rq)) & 15u) == 0u;
    const int nvec = n_vocab >> 2;
    for (int i = tid; i < nvec; i += LP_THREADS) {
        float4 a, b;
        if (vec) {
            a = reinterpret_cast<const float4 *>(rp)[i];
            b = reinterpret_cast<const float4 *>(rq)[i];
        } else {
            const float *ea = rp + 4 * i, *eb = rq + 4 * i;
            a = make_float4(ea[0], ea[1], ea[2], ea[3]);
            b = make_float4(eb[0], eb[1], eb[2], eb[3]);
        }
        term(a.x, b.x); term(a.y, b.y); term(a.z, b.z); term(a.w, b.w);
    }
    if (4 * nvec + tid < n_vocab) term(rp[4 * nvec + tid], rq[4 * nvec + tid]);
    score_block_sums(acc);
    if (tid == 0) {
        const double ls_p = log(acc[0]), ls_q = log(acc[1]);
        out.kl_pq[col] = (float)((acc[2] / acc[0] - ls_p) + ls_q);
        if (out.kl_qp) out.kl_qp[col] = (float)((acc[3] / acc[1] - ls_q) + ls_p);
    }
}

}  // namespace bgk
