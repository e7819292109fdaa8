// Sequence scoring (biogpt_hip_score / biogpt_hip_score_batch): the log-softmax of every logits row of a causal pass,
// with the target gathered from it.  No reference counterpart (biogpt.cpp returns the last row only, F8).
//
//   logprob_rows_kernel   one workgroup per column of the pass:
//                           pass 1  row maximum m and its arg-max (lowest id on ties, as np.argmax / argmax_rows_kernel)
//                           pass 2  S = sum_v exp(l[v] - m): f32 per lane, lanes and waves combined in double
//                           out     logprob = (l[t] - m) - log(S) (double arithmetic, rounded once), l[t], arg-max
//
// The row is read as 16-byte loads from its first 16-byte-aligned element on, a scalar head and tail around them
// (n_vocab need not be a multiple of 4).  The second pass re-reads a row the first one has just brought on chip.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.hip.h"

namespace bgk {

constexpr int LP_THREADS = 256;   // 4 waves per column; 42384 logits = 41 float4 per lane

// keep (v, i) if it beats (bv, bi): larger value, or the same value at a lower id
__device__ __forceinline__ void lp_better(float v, int i, float &bv, int &bi) {
    if (v > bv || (v == bv && i < bi)) { bv = v; bi = i; }
}

// The two passes over one logits row by a workgroup of LP_THREADS threads (shared with beam_group_rows_kernel, kernels_beam.hip.h).
// Every thread returns the row maximum m and its lowest arg-max bi; thread 0 also the exponential sum S = sum_v exp(l[v] - m).
__device__ __forceinline__ void lp_row_stats(const float *row, int n_vocab, float &m, int &bi, double &S) {
    __shared__ float s_max[LP_THREADS / 64];
    __shared__ int s_idx[LP_THREADS / 64];
    __shared__ double s_sum[LP_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    // elements in front of the first 16-byte boundary, then whole float4s, then the tail
    const int head = min(n_vocab, (int)(((16u - ((uint32_t)(uintptr_t)row & 15u)) & 15u) >> 2));
    const int nvec = (n_vocab - head) >> 2;
    const int tail0 = head + 4 * nvec;
    const float4 *body = reinterpret_cast<const float4 *>(row + head);

    // ---- pass 1: maximum + lowest arg-max ----
    float bv = -INFINITY;
    bi = 0x7fffffff;
    if (tid < head) lp_better(row[tid], tid, bv, bi);
    for (int i = tid; i < nvec; i += 2 * LP_THREADS) {      // two 16-byte loads in flight per lane
        const int j = i + LP_THREADS;
        const float4 a = body[i];
        const float4 b = j < nvec ? body[j] : make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
        const int ia = head + 4 * i, ib = head + 4 * j;
        lp_better(a.x, ia, bv, bi); lp_better(a.y, ia + 1, bv, bi); lp_better(a.z, ia + 2, bv, bi); lp_better(a.w, ia + 3, bv, bi);
        if (j < nvec) { lp_better(b.x, ib, bv, bi); lp_better(b.y, ib + 1, bv, bi); lp_better(b.z, ib + 2, bv, bi); lp_better(b.w, ib + 3, bv, bi); }
    }
    if (tail0 + tid < n_vocab) lp_better(row[tail0 + tid], tail0 + tid, bv, bi);
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(bv, off, 64);
        const int oi = __shfl_xor(bi, off, 64);
        lp_better(ov, oi, bv, bi);
    }
    if (lane == 0) { s_max[wv] = bv; s_idx[wv] = bi; }
    __syncthreads();
    for (int w = 0; w < LP_THREADS / 64; w++) lp_better(s_max[w], s_idx[w], bv, bi);   // every thread: the same order, the same result
    m = bv;

    // ---- pass 2: sum of exp(l - m) ----
    float s = 0.0f;
    if (tid < head) s += expf(row[tid] - m);
    for (int i = tid; i < nvec; i += 2 * LP_THREADS) {
        const int j = i + LP_THREADS;
        const float4 a = body[i];
        const float4 b = j < nvec ? body[j] : make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
        s += (expf(a.x - m) + expf(a.y - m)) + (expf(a.z - m) + expf(a.w - m));
        s += (expf(b.x - m) + expf(b.y - m)) + (expf(b.z - m) + expf(b.w - m));   // exp(-inf) = 0 past the end
    }
    if (tail0 + tid < n_vocab) s += expf(row[tail0 + tid] - m);
    const double ws = wave_sum_f64((double)s);
    if (lane == 0) s_sum[wv] = ws;
    __syncthreads();
    S = 0.0;
    if (tid == 0)
        for (int w = 0; w < LP_THREADS / 64; w++) S += s_sum[w];
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
        am_out[col] = bi == 0x7fffffff ? 0 : bi;
    }
}

}  // namespace bgk
