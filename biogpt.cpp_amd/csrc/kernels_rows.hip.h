// What the kernels that run one workgroup per logits row share (logprob_rows_kernel, beam_group_rows_kernel, sample_rows_kernel, rules_rows_kernel,
// contrast_select_kernel, lookup_accept_kernel and argmax_rows_kernel below): the order of (value, id) pairs, the walk over a row, the workgroup's
// arg-max and the bound of a top-K selection.  THREADS is the workgroup's size, a multiple of 64.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "kernels.hip.h"

namespace bgk {

// ---- 1. the order: larger value first, equal values: lower id first.  A NaN is never before anything and nothing is before it. ----
constexpr float ROW_NONE_V = -INFINITY;      // the empty pair: every element of a row but a NaN comes before it
constexpr int ROW_NONE_I = 0x7fffffff;

__device__ __forceinline__ bool row_before(float av, int ai, float bv, int bi) { return av > bv || (av == bv && ai < bi); }
// keep (v, i) if it comes before the held pair
__device__ __forceinline__ void row_keep(float v, int i, float &bv, int &bi) {
    if (row_before(v, i, bv, bi)) { bv = v; bi = i; }
}

// ---- 2. the walk: one(value, index) for the elements in front of the first 16-byte boundary (thread t: element t), quad(float4, first index) for
//      the whole float4s behind it, one() for the tail.  Quad q belongs to thread q % THREADS, a thread's quads come in ascending order, DEPTH
//      (1 or 2) 16-byte loads in flight per lane: the order of the calls is the same for both.  n need not be a multiple of 4 and the row needs
//      no alignment beyond a float's. ----
template <int THREADS, int DEPTH = 2, class Q, class O>
__device__ __forceinline__ void row_scan(const float *row, int n, Q quad, O one) {
    static_assert(DEPTH == 1 || DEPTH == 2, "one or two loads in flight");
    const int tid = threadIdx.x;
    const int head = min(n, (int)(((16u - ((uint32_t)(uintptr_t)row & 15u)) & 15u) >> 2));
    const int nvec = (n - head) >> 2;
    const int tail0 = head + 4 * nvec;
    const float4 *body = reinterpret_cast<const float4 *>(row + head);
    if (tid < head) one(row[tid], tid);
    if constexpr (DEPTH == 1) {
        for (int i = tid; i < nvec; i += THREADS) quad(body[i], head + 4 * i);
    } else {
        for (int i = tid; i < nvec; i += 2 * THREADS) {
            const int j = i + THREADS;
            const float4 a = body[i];
            const float4 b = j < nvec ? body[j] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            quad(a, head + 4 * i);
            if (j < nvec) quad(b, head + 4 * j);
        }
    }
    if (tail0 + tid < n) one(row[tail0 + tid], tail0 + tid);
}
// f(value, index) for every element, a quad's in the order x, y, z, w
template <int THREADS, int DEPTH = 2, class F>
__device__ __forceinline__ void row_scan(const float *row, int n, F f) {
    row_scan<THREADS, DEPTH>(row, n, [&](float4 q, int i) { f(q.x, i); f(q.y, i + 1); f(q.z, i + 2); f(q.w, i + 3); }, f);
}

// ---- 3. the workgroup's arg-max: the first of the threads' pairs (bv, bi) in the order above, returned to every thread (each combines the waves'
//      pairs in the same order).  One barrier.  A caller that calls it again, or anything else that shares THREADS with it, puts a barrier in
//      between: the waves' words in LDS are read behind the barrier here and written in front of it there. ----
template <int THREADS>
__device__ __forceinline__ void block_best(float &bv, int &bi) {
    __shared__ float s_v[THREADS / 64];
    __shared__ int s_i[THREADS / 64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(bv, off, 64);
        const int oi = __shfl_xor(bi, off, 64);
        row_keep(ov, oi, bv, bi);
    }
    if (lane == 0) { s_v[wv] = bv; s_i[wv] = bi; }
    __syncthreads();
    for (int w = 0; w < THREADS / 64; w++) row_keep(s_v[w], s_i[w], bv, bi);
}

// the row's maximum and its lowest id, (ROW_NONE_V, ROW_NONE_I) for a row of NaNs only: to every thread, under block_best's contract
template <int THREADS>
__device__ __forceinline__ void row_argmax(const float *row, int n, float &bv, int &bi) {
    bv = ROW_NONE_V;
    bi = ROW_NONE_I;
    row_scan<THREADS>(row, n, [&](float v, int i) { row_keep(v, i, bv, bi); });
    block_best<THREADS>(bv, bi);
}

// ---- 4. the bound of a top-K selection, K <= THREADS: (mv, mi) is the first of the calling thread's own elements (the empty pair: it has none);
//      returned to every thread is the K-th of the threads' pairs.  K threads hold an element at least that good, so no element behind the bound
//      is among the row's first K, and a second walk hands only the few elements at or above it to the selection proper (else every wave would
//      run its insertion for nearly every element: with ~166 elements per lane, some lane of 64 almost always has a new entry).  Pairs with an
//      element are distinct, so one thread at most has rank K - 1; with fewer than K threads holding an element the bound stays the empty pair
//      and everything passes.  Two barriers (the first also publishes what the caller wrote to LDS before the call); called once per kernel. ----
template <int THREADS>
__device__ __forceinline__ void row_kth_bound(float mv, int mi, int K, float &thr_v, int &thr_i) {
    __shared__ float t_v[THREADS];
    __shared__ int t_i[THREADS];
    __shared__ float s_thr_v;
    __shared__ int s_thr_i;
    const int tid = threadIdx.x;
    t_v[tid] = mv; t_i[tid] = mi;
    if (tid == 0) { s_thr_v = ROW_NONE_V; s_thr_i = ROW_NONE_I; }
    __syncthreads();
    int rank = 0;
    for (int j = 0; j < THREADS; j++) rank += row_before(t_v[j], t_i[j], mv, mi) ? 1 : 0;
    if (rank == K - 1 && mi != ROW_NONE_I) { s_thr_v = mv; s_thr_i = mi; }
    __syncthreads();
    thr_v = s_thr_v;
    thr_i = s_thr_i;
}

constexpr int ARGMAX_ROWS_THREADS = 1024;

// Batched decode sampler: one workgroup of ARGMAX_ROWS_THREADS threads per sequence row of logits[rows][ld]; arg-max (lowest id wins ties, 0 for a row of NaNs only),
// appended to the sequence's id list, becomes its next input token; advance = 1 moves its position on.
__global__ __launch_bounds__(ARGMAX_ROWS_THREADS) void argmax_rows_kernel(const float *logits, int ld, int n_vocab, SeqState *seq, int seq0,
                                                           int32_t *gen_ids, int gen_stride, int advance) {
    const int row = blockIdx.x;
    float bv;
    int bi;
    row_argmax<ARGMAX_ROWS_THREADS>(logits + (size_t)row * ld, n_vocab, bv, bi);
    if (threadIdx.x == 0) {
        const int id = bi == ROW_NONE_I ? 0 : bi;
        SeqState *s = seq + seq0 + row;
        gen_ids[(size_t)(seq0 + row) * gen_stride + s->n_gen] = id;
        s->n_gen += 1;
        s->token = id;
        s->n_past += advance;
    }
}

}  // namespace bgk
