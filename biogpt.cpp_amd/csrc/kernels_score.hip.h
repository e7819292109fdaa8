// Sequence scoring (biogpt_hip_score / biogpt_hip_score_batch): the log-softmax of every logits row of a causal pass,
// with the target gathered from it.  No reference counterpart (biogpt.cpp returns the last row only, F8).
//
//   logprob_rows_kernel   one workgroup per column of the pass:
//                           pass 1  row maximum m and its arg-max (lowest id on ties, as np.argmax / argmax_rows_kernel)
//                           pass 2  S = sum_v exp(l[v] - m): f32 per lane, lanes and waves combined in double
//                           out     logprob = (l[t] - m) - log(S) (double arithmetic, rounded once), l[t], arg-max
//
// Both passes walk the row with row_scan and pass 1 is row_argmax (kernels_rows.hip.h; DESIGN.md "Row kernels").  The second pass re-reads a
// row the first one has just brought on chip.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.hip.h"
#include "kernels_rows.hip.h"

namespace bgk {

constexpr int LP_THREADS = 256;   // 4 waves per column; 42384 logits = 41 float4 per lane

// The second pass alone, for a caller that holds the row maximum m already (every thread the same; sample_lp_rows_kernel, kernels_genlp.hip.h, has it from its
// selection): thread 0 returns S = sum_v exp(l[v] - m).  One barrier; whatever shares LP_THREADS with it and came before has passed a barrier of its own.
__device__ __forceinline__ void lp_row_sum(const float *row, int n_vocab, float m, double &S) {
    __shared__ double s_sum[LP_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    // sum of exp(l - m): the quads (elements 4 q .. 4 q + 3, quad q to thread q % LP_THREADS, ascending), then the tail; each quad as (x + y) + (z + w).  Which
    // lane adds which element decides the sum's last bits, and it must follow from the element's INDEX alone: the rows of a pass whose vocabulary is no multiple
    // of 4 lie on all four 16-byte alignments, and score_batch owes score's bits whichever row of a pass a token is.  row_scan walks from the first 16-byte
    // boundary on, so a row that does not lie on one is walked here, by 4-byte loads, in the order row_scan gives a row that does.
    float s = 0.0f;
    if ((((uint32_t)(uintptr_t)row) & 15u) == 0u) {
        row_scan<LP_THREADS>(
            row, n_vocab, [&](float4 e, int) { s += (expf(e.x - m) + expf(e.y - m)) + (expf(e.z - m) + expf(e.w - m)); },
            [&](float v, int) { s += expf(v - m); });
    } else {
        const int nvec = n_vocab >> 2;
        for (int i = tid; i < nvec; i += LP_THREADS) {
            const float *e = row + 4 * i;
            s += (expf(e[0] - m) + expf(e[1] - m)) + (expf(e[2] - m) + expf(e[3] - m));
        }
        if (4 * nvec + tid < n_vocab) s += expf(row[4 * nvec + tid] - m);
    }
    const double ws = wave_sum_f64((double)s);
    if (lane == 0) s_sum[wv] = ws;
    __syncthreads();
    S = 0.0;
    if (tid == 0)
        for (int w = 0; w < LP_THREADS / 64; w++) S += s_sum[w];
}

// The two passes over one logits row by a workgroup of LP_THREADS threads (shared with beam_group_rows_kernel, kernels_beam.hip.h, and the selection kernels
// of kernels_genlp.hip.h).  Every thread returns the row maximum m and its lowest arg-max bi; thread 0 also the exponential sum S = sum_v exp(l[v] - m).
__device__ __forceinline__ void lp_row_stats(const float *row, int n_vocab, float &m, int &bi, double &S) {
    row_argmax<LP_THREADS>(row, n_vocab, m, bi);
    lp_row_sum(row, n_vocab, m, S);
}

// logits: [N][ldl] floats (N = gridDim.x); targets / lp_out / am_out / lg_out: [N], already offset to the pass's first column.
// targets[c] < 0: lp_out = lg_out = 0 (am_out is written for every column).
__global__ __launch_bounds__(LP_THREADS) void logprob_rows_kernel(const float *logits, int ldl, int n_vocab, const int32_t *targets,
                                                                 float *lp_out, int32_t *am_out, float *lg_out) {
    const int col = blockIdx.x;
    const float *row = logits + (size_t)col * ldl;
    float m;
    int bi;
    double S;
    lp_row_stats(row, n_vocab, m, bi, S);
    if (threadIdx.x == 0) {
        const int t = targets[col];
        float lp = 0.0f, lt = 0.0f;
        if (t >= 0 && t < n_vocab) {
            lt = row[t];
            lp = (float)(((double)lt - (double)m) - log(S));
        }
        lp_out[col] = lp;
        lg_out[col] = lt;
        am_out[col] = bi == ROW_NONE_I ? 0 : bi;
    }
}

}  // namespace bgk
