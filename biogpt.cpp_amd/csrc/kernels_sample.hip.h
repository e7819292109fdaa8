// Sampled generation (biogpt_hip_generate_sample): biogpt_sample_top_k_top_p (biogpt.cpp:908-980) on the device, inside the captured step.
// A step is the batched decode of the running sequences (one column and one K / V cache slot per sequence), then:
//
//   sample_rows_kernel   one workgroup per sequence row of logits_all:
//                          selection  the row's top k (value descending, equal values: lower id first -- the order of topk_kernel / host_topk).
//                                     Pass 1: the bound (row_kth_bound; the walk, the order and the arg-max are the row kernels' shared pieces,
//                                     kernels_rows.hip.h, DESIGN.md "Row kernels").  Pass 2 (the row is on chip by now): the few
//                                     elements at or above the bound go to a list in LDS; each finds its rank among them by counting.
//                                     A row with more than SAMPLE_CAND_CAP such elements (many of the best in few threads) takes k rounds
//                                     of a workgroup-wide arg-max instead: slow, and not what a model's logits look like.
//                          tail       sample_tail() below: scale, exp, normalise, top-p cut, renormalise, libstdc++'s discrete_distribution
//                                     (ONE generate_canonical<double, 53> = two mt19937 outputs, none with fewer than two candidates), all in
//                                     double.  The per-candidate operations run one per thread, the sums in candidate order on thread 0.
//                          append     the id to the sequence's history, its next token and position; an EOS sets the sequence's finished
//                                     flag instead: a finished column keeps its token and position (it recomputes the K / V row it has).
//                        The step is sample_rows_step<Extra>; sample_rows_kernel instantiates it with SamplePlain (nothing added), sample_lp_rows_kernel
//                        (kernels_genlp.hip.h) with the log-probabilities of the drawn token and of the row's best entries.  The generator's block and the
//                        append are functions of their own (sample_mt_refill, sample_append): sample_wide_rows_kernel (kernels_wide_sample.hip.h), the
//                        selection for any top_k with min-p, runs the same.
//   kv_share_kernel      before the first step of a call with several samples per prompt: the prompt's K / V rows from the slot of the
//                        prompt's first sample to the slots of the others (head-major cache: one contiguous run per (layer, head)).
//   kv_prefix_copy_kernel  a call behind a shared prefix whose steps know one slot per sequence: the prefix's shared rows from the slot they were
//                        evaluated into to the slot of every sequence.
//
// The random state is std::mt19937's: 624 words + the index, one per sequence in device memory, seeded on the host.  sample_tail and the
// generator are __host__ __device__: biogpt_hip_sample_candidates_host runs the same text on the CPU.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "kernels.hip.h"
#include "kernels_score.hip.h"

namespace bgk {

constexpr int SAMPLE_MAX_K = 64;          // top_k of a call (the limit of biogpt_hip_eval_topk)
constexpr int SAMPLE_THREADS = 256;       // 4 waves per row, as logprob_rows_kernel
constexpr int SAMPLE_CAND_CAP = 1024;     // candidates the LDS list holds
constexpr int MT_N = 624, MT_M = 397;

// the call's parameters and the count of unfinished sequences (the host polls it when an EOS id is given)
struct SampleCtl {
    int32_t top_k, eos_id;     // eos_id < 0: none
    int32_t n_live, pad;
    double top_p, temp;
};

struct SampleSeq {
    uint32_t mt[MT_N + 1];     // std::mt19937: the state words, then the index of the next output (624: regenerate first)
    int32_t finished;
    int32_t pad[2];
};

// ---- std::mt19937 ([rand.eng.mers]) ----------------------------------------------------------------------------------------------------
__host__ __device__ inline uint32_t mt_mix(uint32_t cur, uint32_t nxt, uint32_t far) {
    const uint32_t y = (cur & 0x80000000u) | (nxt & 0x7fffffffu);
    return far ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
}
__host__ __device__ inline void mt_seed(uint32_t seed, uint32_t *mt) {
    mt[0] = seed;
    for (int i = 1; i < MT_N; i++) mt[i] = 1812433253u * (mt[i - 1] ^ (mt[i - 1] >> 30)) + (uint32_t)i;
    mt[MT_N] = MT_N;
}
__host__ __device__ inline void mt_regenerate(uint32_t *mt) {
    for (int i = 0; i < MT_N - MT_M; i++) mt[i] = mt_mix(mt[i], mt[i + 1], mt[i + MT_M]);
    for (int i = MT_N - MT_M; i < MT_N - 1; i++) mt[i] = mt_mix(mt[i], mt[i + 1], mt[i + MT_M - MT_N]);
    mt[MT_N - 1] = mt_mix(mt[MT_N - 1], mt[0], mt[MT_M - 1]);
    mt[MT_N] = 0;
}
__host__ __device__ inline uint32_t mt_next(uint32_t *mt) {
    if (mt[MT_N] >= (uint32_t)MT_N) mt_regenerate(mt);
    uint32_t y = mt[mt[MT_N]];
    mt[MT_N] += 1;
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= y >> 18;
    return y;
}

// ---- the tail: k candidates in selection order -> the sampled candidate's index ----------------------------------------------------------
struct SampleWork {
    double total;
    int32_t n, pick;
};

struct SampleNoSync { __host__ __device__ void operator()() const {} };

// biogpt.cpp:938-980 over vals[0 .. k) (f32 logits, best first); p: k doubles of workspace.  `nl` callers with lane = 0 .. nl - 1 run it together, sync() making w
// visible between the steps; the host runs it with nl = 1.  Returns the index of the chosen candidate (every caller the same).
template <class Sync>
__host__ __device__ inline int sample_tail(const float *vals, int k, double top_p, double temp, uint32_t *mt, double *p, SampleWork &w, int lane, int nl, Sync sync) {
    const double scale = 1.0 / temp;
    double maxl = -INFINITY;
    for (int i = 0; i < k; i++) {
        const double v = (double)vals[i] * scale;
        maxl = v > maxl ? v : maxl;
    }
    for (int i = lane; i < k; i += nl) p[i] = exp((double)vals[i] * scale - maxl);
    sync();
    if (lane == 0) {
        double total = 0.0;
        for (int i = 0; i < k; i++) total += p[i];
        w.total = total;
    }
    sync();
    for (int i = lane; i < k; i += nl) p[i] = p[i] / w.total;
    sync();
    if (lane == 0) {      // the top-p cut at the first cumsum >= top_p; w.total: the renormalisation factor
        int n = k;
        double inv = 1.0;
        if (top_p < 1.0) {
            double cumsum = 0.0;
            for (int i = 0; i < k; i++) {
                cumsum += p[i];
                if (cumsum >= top_p) { n = i + 1; break; }
            }
            inv = 1.0 / cumsum;
        }
        w.n = n;
        w.total = inv;
    }
    sync();
    const int n = w.n;
    if (top_p < 1.0)
        for (int i = lane; i < n; i += nl) p[i] = p[i] * w.total;
    sync();
    // std::discrete_distribution (libstdc++): fewer than two probabilities -> 0 and no draw
    if (n < 2) return 0;
    if (lane == 0) {
        double total = 0.0;
        for (int i = 0; i < n; i++) total += p[i];
        w.total = total;
    }
    sync();
    for (int i = lane; i < n; i += nl) p[i] = p[i] / w.total;
    sync();
    if (lane == 0) {
        double run = 0.0;
        for (int i = 0; i < n; i++) { run += p[i]; p[i] = run; }
        p[n - 1] = 1.0;
        const double a = (double)mt_next(mt);      // generate_canonical<double, 53>: (a + b * 2^32) / 2^64
        const double b = (double)mt_next(mt);
        double u = (a + b * 4294967296.0) / 18446744073709551616.0;
        if (u >= 1.0) u = 0x1.fffffffffffffp-1;    // nextafter(1, 0)
        int lo = 0, hi = n;                        // std::lower_bound: the first partial sum >= u
        while (lo < hi) {
            const int mid = (lo + hi) / 2;
            if (p[mid] < u) lo = mid + 1; else hi = mid;
        }
        w.pick = lo;
    }
    sync();
    return w.pick;
}

struct SampleBlockSync { __device__ void operator()() const { __syncthreads(); } };

// The selection of sample_rows_kernel (and of contrast_select_kernel, kernels_contrast.hip.h): the row's best K <= SAMPLE_MAX_K elements into top_v / top_i
// (LDS of the caller), value descending, equal values lower id first; NaNs never.  Called by all SAMPLE_THREADS threads; returns how many there are
// (uniform), visible to every thread on return.
__device__ __forceinline__ int sample_topk(const float *row, int n_vocab, int K, float *top_v, int *top_i) {
    __shared__ float c_v[SAMPLE_CAND_CAP];
    __shared__ int c_i[SAMPLE_CAND_CAP];
    __shared__ int s_n;
    const int tid = threadIdx.x;
    // ---- pass 1: the bound (row_kth_bound, kernels_rows.hip.h; its first barrier publishes s_n) ----
    float mv = ROW_NONE_V, thr_v;
    int mi = ROW_NONE_I, thr_i;
    row_scan<SAMPLE_THREADS>(row, n_vocab, [&](float v, int i) { row_keep(v, i, mv, mi); });
    if (tid == 0) s_n = 0;
    row_kth_bound<SAMPLE_THREADS>(mv, mi, K, thr_v, thr_i);

    // ---- pass 2: the elements at or above the bound (NaNs never are, as in host_topk) ----
    row_scan<SAMPLE_THREADS>(row, n_vocab, [&](float v, int i) {
        if (v == v && !row_before(thr_v, thr_i, v, i)) {
            const int slot = atomicAdd(&s_n, 1);
            if (slot < SAMPLE_CAND_CAP) { c_v[slot] = v; c_i[slot] = i; }
        }
    });
    __syncthreads();
    const int n_c = s_n;
    int k_eff;
    if (n_c <= SAMPLE_CAND_CAP) {
        k_eff = min(K, n_c);
        for (int c = tid; c < n_c; c += SAMPLE_THREADS) {
            const float v = c_v[c];
            const int id = c_i[c];
            int rank = 0;
            for (int j = 0; j < n_c; j++) rank += row_before(c_v[j], c_i[j], v, id) ? 1 : 0;
            if (rank < K) { top_v[rank] = v; top_i[rank] = id; }
        }
        __syncthreads();
    } else {      // K rounds: the best element after the one picked before
        float pv = INFINITY;
        int pi = -1;
        k_eff = 0;
        for (int rd = 0; rd < K; rd++) {
            float bv = ROW_NONE_V;
            int bi = ROW_NONE_I;
            row_scan<SAMPLE_THREADS>(row, n_vocab, [&](float v, int i) {
                if (v == v && row_before(pv, pi, v, i)) row_keep(v, i, bv, bi);
            });
            block_best<SAMPLE_THREADS>(bv, bi);
            __syncthreads();      // block_best's words are written again by the next round
            if (bi == ROW_NONE_I) break;      // (uniform: every thread holds the same pair)
            if (tid == 0) { top_v[rd] = bv; top_i[rd] = bi; }
            pv = bv; pi = bi;
            k_eff = rd + 1;
        }
        __syncthreads();
    }

    return k_eff;
}

// ---- what a sampling step shares with the wide sampler (kernels_wide_sample.hip.h): the generator's block and the step's epilogue ----
// An exhausted block of outputs is regenerated by the whole workgroup of THREADS >= 227 threads (the words of [0, 227), [227, 454), [454, 623) and 623
// depend on the old block and on the ranges before them only).  mt_old / mt_new: MT_N words of LDS each.  Called by every thread.
template <int THREADS>
__device__ __forceinline__ void sample_mt_refill(SampleSeq *me, uint32_t *mt_old, uint32_t *mt_new) {
    static_assert(THREADS >= MT_N - MT_M, "one thread per word of a range");
    const int tid = threadIdx.x;
    if (me->mt[MT_N] == (uint32_t)MT_N) {
        constexpr int D = MT_N - MT_M;
        for (int i = tid; i < MT_N; i += THREADS) mt_old[i] = me->mt[i];
        __syncthreads();
        if (tid < D) mt_new[tid] = mt_mix(mt_old[tid], mt_old[tid + 1], mt_old[tid + MT_M]);
        __syncthreads();
        if (tid < D) mt_new[tid + D] = mt_mix(mt_old[tid + D], mt_old[tid + D + 1], mt_new[tid]);
        __syncthreads();
        if (tid < D && tid + 2 * D < MT_N - 1) mt_new[tid + 2 * D] = mt_mix(mt_old[tid + 2 * D], mt_old[tid + 2 * D + 1], mt_new[tid + D]);
        __syncthreads();
        if (tid == 0) mt_new[MT_N - 1] = mt_mix(mt_old[MT_N - 1], mt_new[0], mt_new[MT_M - 1]);
        __syncthreads();
        for (int i = tid; i < MT_N; i += THREADS) me->mt[i] = mt_new[i];
        if (tid == 0) me->mt[MT_N] = 0;
        __syncthreads();
    }
}

// The epilogue of row r's step, by one thread: the id to the sequence's history, its next token and position; an EOS sets the sequence's finished flag
// instead and takes it off the count of the unfinished.  emit(g): what the caller adds for entry g of the history.
template <class Emit>
__device__ __forceinline__ void sample_append(int r, int id, int eos_id, int32_t *n_live, SampleSeq *me, SeqState *seq, int32_t *seq_gen, int gen_stride, Emit emit) {
    SeqState *s = seq + r;
    const int g = s->n_gen;
    if (g < gen_stride) seq_gen[(size_t)r * gen_stride + g] = id;
    emit(g);
    s->n_gen = g + 1;
    if (eos_id >= 0 && id == eos_id) {
        me->finished = 1;
        atomicSub(n_live, 1);
    } else {
        s->token = id;
        s->n_past += 1;
    }
}

// What a kernel may add to the step of sample_rows_kernel without touching its draw (sample_lp_rows_kernel, kernels_genlp.hip.h: the log-probabilities of
// the drawn token and of the row's best): also_select() more candidates wanted than top_k (they follow the top_k in the same order, so the draw sees the
// candidates it would have seen); row_stats() by every thread behind the selection (k_all candidates in top_v, visible); emit() by thread 0 with the
// sequence's entry g and the drawn candidate's index.  This one adds nothing.
struct SamplePlain {
    __device__ __forceinline__ int also_select() const { return 0; }
    __device__ __forceinline__ void row_stats(const float *, int, const float *, int) {}
    __device__ __forceinline__ void emit(int, int, int, const float *, const int *, int) {}
};

// The step of one row, by the SAMPLE_THREADS threads of its workgroup.
// logits: [rows][ldl] (row r = column r = sequence r); seq / sq: the rows' states; seq_gen: [row][gen_stride] token histories
template <class Extra>
__device__ __forceinline__ void sample_rows_step(const float *logits, int ldl, int n_vocab, SampleCtl *ctl, SampleSeq *sq, SeqState *seq, int32_t *seq_gen,
                                                 int gen_stride, Extra extra) {
    __shared__ float top_v[SAMPLE_MAX_K];
    __shared__ int top_i[SAMPLE_MAX_K];
    __shared__ uint32_t mt_old[MT_N], mt_new[MT_N];
    __shared__ SampleWork work;
    __shared__ double work_p[SAMPLE_MAX_K];
    const int r = blockIdx.x, tid = threadIdx.x;
    SampleSeq *const me = sq + r;
    if (me->finished) return;
    const float *row = logits + (size_t)r * ldl;
    const int K = min(min(ctl->top_k, SAMPLE_MAX_K), n_vocab);

    sample_mt_refill<SAMPLE_THREADS>(me, mt_old, mt_new);

    const int k_all = sample_topk(row, n_vocab, max(K, min(min(extra.also_select(), SAMPLE_MAX_K), n_vocab)), top_v, top_i);
    const int k_eff = min(k_all, K);
    extra.row_stats(row, n_vocab, top_v, k_all);

    // ---- the draw ----
    int pick = 0, id = 0;
    if (k_eff > 0) {
        pick = sample_tail(top_v, k_eff, ctl->top_p, ctl->temp, me->mt, work_p, work, tid, SAMPLE_THREADS, SampleBlockSync());
        id = top_i[pick];
    }
    if (tid == 0) sample_append(r, id, ctl->eos_id, &ctl->n_live, me, seq, seq_gen, gen_stride, [&](int g) { extra.emit(r, g, pick, top_v, top_i, k_all); });
}

__global__ __launch_bounds__(SAMPLE_THREADS) void sample_rows_kernel(const float *logits, int ldl, int n_vocab, SampleCtl *ctl, SampleSeq *sq,
                                                                     SeqState *seq, int32_t *seq_gen, int gen_stride) {
    sample_rows_step(logits, ldl, n_vocab, ctl, sq, seq, seq_gen, gen_stride, SamplePlain());
}

// grid (n_layer * n_head, n_seqs, 2 [K, V]); seq_stride floats between two slots, P * dk between two heads.  Sequence r with r % n_samples != 0
// takes the rows [first_row, its position) -- the prompt without its last token -- from the slot of its prompt's first sample.  first_row > 0: the rows in
// front are those of a shared prefix (SeqState::pad[0] where the steps read them in the prefix's slot; kv_prefix_copy_kernel brings them where they do not):
// that range of the first sample's slot was never written and is not read here.
__global__ __launch_bounds__(256) void kv_share_kernel(const SeqState *seq, int n_samples, int first_row, float *kroot, float *vroot, int64_t seq_stride, int P, int dk) {
    const int r = blockIdx.y, j = r % n_samples;
    if (j == 0) return;
    const int rows = min(seq[r].n_past, P);
    const int first = min(max(first_row, 0), max(rows, 0));
    const size_t run0 = (size_t)blockIdx.x * P * dk;
    float *root = blockIdx.z == 0 ? kroot : vroot;
    const float4 *s4 = reinterpret_cast<const float4 *>(root + (size_t)(r - j) * seq_stride + run0);
    float4 *d4 = reinterpret_cast<float4 *>(root + (size_t)r * seq_stride + run0);
    const int n4 = rows > 0 ? rows * dk / 4 : 0;
    for (int i = first * dk / 4 + threadIdx.x; i < n4; i += blockDim.x) d4[i] = s4[i];
}

// grid (n_layer * n_head, n_seqs, 2 [K, V]), as kv_share_kernel: the rows [0, n_shared) of slot `slot` -- a shared prefix, evaluated once -- into the slot
// of every sequence r, for decode steps that know one slot per sequence (the column-per-XCD launches of 2 .. 8 sequences).
__global__ __launch_bounds__(256) void kv_prefix_copy_kernel(int n_shared, int slot, float *kroot, float *vroot, int64_t seq_stride, int P, int dk) {
    const int r = blockIdx.y;
    if (r == slot) return;
    const size_t run0 = (size_t)blockIdx.x * P * dk;
    float *root = blockIdx.z == 0 ? kroot : vroot;
    const float4 *s4 = reinterpret_cast<const float4 *>(root + (size_t)slot * seq_stride + run0);
    float4 *d4 = reinterpret_cast<float4 *>(root + (size_t)r * seq_stride + run0);
    const int n4 = min(n_shared, P) > 0 ? min(n_shared, P) * dk / 4 : 0;
    for (int i = threadIdx.x; i < n4; i += blockDim.x) d4[i] = s4[i];
}

}  // namespace bgk
