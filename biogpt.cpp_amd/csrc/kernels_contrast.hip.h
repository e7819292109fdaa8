// Contrastive search (biogpt_hip_generate_contrastive; Su et al. 2022, transformers' generate(penalty_alpha, top_k)): the degeneration penalty
// and the selection on the device, inside the captured step.  No reference counterpart (biogpt.cpp samples or takes the arg-max).
//
// G prompts, each a group of k columns and K / V cache slots [g * k, (g + 1) * k).  Group g keeps a context store: row i of H[g] is the f32 hidden row
// (after the final LayerNorm) of context token i, Hn[g][i] its squared norm as a double.  A step is the batched decode of all G * k columns -- column j
// of a group carries candidate j at position len(H[g]) -- with the final-LayerNorm rows of the columns as a second epilogue, then:
//
//   contrast_rank_kernel    grid (slab of CT_SLAB context positions, group).  The group's k candidate rows go to LDS once; every wave takes every
//                           fourth row of the slab: the row in registers (16-byte loads, the next row in flight), ONE load of it for all k candidates,
//                           k dots in double, sim = (float)(dot / sqrt(na * nb)), the running maximum of candidate j in lane j.  Writes k partial
//                           maxima per slab; slabs at or beyond the group's length, and finished groups, exit at once.
//   contrast_select_kernel  one workgroup per group: the slab maxima -> pen_j, score_j = (float)((1 - a) * p_j - a * pen_j), the winner (highest score,
//                           lowest j on ties); its id to seq_gen, its hidden row and norm appended to H[g]; lp_row_stats + sample_topk (both on the row kernels'
//                           shared pieces, kernels_rows.hip.h, DESIGN.md "Row kernels") of the winner's
//                           logits row -> the next k candidates and their probabilities; the k column states advance; an EOS finishes the group.
//                           A group's FIRST step is the same step: its k columns all carry the prompt's last token, so "candidate 0" wins by decree,
//                           nothing is written to seq_gen, and the row appended to H[g] is that token's.
//   contrast_kv_row_kernel  the winner's K / V row of the position just evaluated, all layers and heads, to the group's other k - 1 slots.
//   contrast_norms_kernel   after the prompt pass: the squared norms of the rows that pass left in H.
//
// The order of every dot (ct_row_dot): d / 4 float4 chunks, chunk c belongs to lane c % 64; a lane adds its products in ascending element order (chunk
// c, c + 64, ..., x y z w within a chunk) into one double, fused or not (an f32 x f32 product is exact in double: one rounding, the sum's); the 64 lane
// sums are combined by wave_sum_f64 (kernels.hip.h).  tests/contrast_ref.py restates it.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "kernels.hip.h"
#include "kernels_score.hip.h"
#include "kernels_sample.hip.h"

namespace bgk {

constexpr int CT_MAX_K = 16;          // top_k of a call
constexpr int CT_SLAB = 64;           // context positions per rank workgroup
constexpr int CT_THREADS = 256;       // = LP_THREADS = SAMPLE_THREADS: the select kernel calls lp_row_stats and sample_topk
constexpr int CT_MAX_D = 1024;        // row width the rank kernel holds in registers (4 float4 per lane)
constexpr int CT_NCH = CT_MAX_D / 4 / 64;
static_assert(CT_THREADS == LP_THREADS && CT_THREADS == SAMPLE_THREADS, "the select kernel shares lp_row_stats / sample_topk");

struct ContrastCtl {
    int32_t top_k, eos_id;     // eos_id < 0: none
    int32_t n_live, pad;       // groups still running (the host polls it when an EOS id is given)
    float alpha;
    int32_t pad2[3];
};

struct ContrastGroup {
    int32_t len;               // rows of H[g]
    int32_t finished;
    int32_t first;             // the next step is the group's first (the prompt's last token in all k columns)
    int32_t winner;            // column of the last selection
    int32_t copy_pos;          // position whose K / V row contrast_kv_row_kernel spreads from the winner's slot; -1: nothing to copy
    int32_t pad[3];
    float p[CT_MAX_K];         // the candidates of the next step: probability, id
    int32_t id[CT_MAX_K];
};

struct CtRow { float4 v[CT_NCH]; };

// chunk lane + 64 * i of a row of nch float4s; chunks past the end are zeros (they add nothing to a dot)
__device__ __forceinline__ CtRow ct_load_row(const float4 *row, int nch, int lane) {
    CtRow r;
#pragma unroll
    for (int i = 0; i < CT_NCH; i++) {
        const int ch = lane + 64 * i;
        r.v[i] = ch < nch ? row[ch] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    return r;
}
// this lane's part of a dot, in the order the header states
__device__ __forceinline__ double ct_lane_dot(const CtRow &a, const float4 *b, int nch, int lane) {
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < CT_NCH; i++) {
        const int ch = lane + 64 * i;
        if (ch < nch) {
            const float4 c = b[ch];
            acc = __builtin_fma((double)a.v[i].x, (double)c.x, acc);
            acc = __builtin_fma((double)a.v[i].y, (double)c.y, acc);
            acc = __builtin_fma((double)a.v[i].z, (double)c.z, acc);
            acc = __builtin_fma((double)a.v[i].w, (double)c.w, acc);
        }
    }
    return acc;
}
__device__ __forceinline__ double ct_lane_norm(const CtRow &a) {
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < CT_NCH; i++) {      // (zero chunks past the end: + 0.0 changes nothing)
        acc = __builtin_fma((double)a.v[i].x, (double)a.v[i].x, acc);
        acc = __builtin_fma((double)a.v[i].y, (double)a.v[i].y, acc);
        acc = __builtin_fma((double)a.v[i].z, (double)a.v[i].z, acc);
        acc = __builtin_fma((double)a.v[i].w, (double)a.v[i].w, acc);
    }
    return acc;
}
// squared norm of one row of d floats by one wave (uniform result)
__device__ __forceinline__ double ct_row_norm(const float *row, int d, int lane) {
    return wave_sum_f64(ct_lane_norm(ct_load_row(reinterpret_cast<const float4 *>(row), d >> 2, lane)));
}

// cand: [G * k][d] candidate rows; H: [G][P][d]; Hn: [G][P]; slab_max: [G][gridDim.x][CT_MAX_K].  Grid (ceil(P / CT_SLAB), G), CT_THREADS threads,
// k * d * 4 bytes of dynamic LDS (k <= CT_MAX_K, d <= CT_MAX_D, 4 | d).
__global__ __launch_bounds__(CT_THREADS) void contrast_rank_kernel(const float *cand, const float *H, const double *Hn, const ContrastGroup *grp, int k, int d, int P,
                                                                   float *slab_max) {
    extern __shared__ float4 s_c4[];      // [k][d / 4]; at the end [4 waves][CT_MAX_K] maxima
    const int slab = blockIdx.x, g = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int len = min(grp[g].len, P), r0 = slab * CT_SLAB;
    if (r0 >= len || grp[g].finished) return;
    const int nch = d >> 2, r1 = min(r0 + CT_SLAB, len);
    const float4 *c4 = reinterpret_cast<const float4 *>(cand + (size_t)g * k * d);
    for (int i = tid; i < k * nch; i += CT_THREADS) s_c4[i] = c4[i];
    __syncthreads();
    // lane j: the squared norm of candidate j (every wave computes all k)
    double na = 0.0;
    for (int j = 0; j < k; j++) {
        const double t = wave_sum_f64(ct_lane_norm(ct_load_row(s_c4 + j * nch, nch, lane)));
        if (lane == j) na = t;
    }
    const float4 *Hg = reinterpret_cast<const float4 *>(H + (size_t)g * P * d);
    const double *Hng = Hn + (size_t)g * P;
    float mx = -INFINITY;
    int r = r0 + wave;
    CtRow nxt = ct_load_row(Hg + (size_t)min(r, r1 - 1) * nch, nch, lane);
    for (; r < r1; r += 4) {
        const CtRow row = nxt;
        const double nb = Hng[r];
        nxt = ct_load_row(Hg + (size_t)min(r + 4, r1 - 1) * nch, nch, lane);      // (the last one re-reads a row of the slab: in bounds, unused)
        for (int j = 0; j < k; j++) {
            const double dot = wave_sum_f64(ct_lane_dot(row, s_c4 + j * nch, nch, lane));
            const double naj = __shfl(na, j, 64);
            const float sim = (naj == 0.0 || nb == 0.0) ? 0.0f : (float)(dot / sqrt(naj * nb));
            if (lane == j) mx = fmaxf(mx, sim);
        }
    }
    __syncthreads();      // the candidate rows are done with
    float *s_m = reinterpret_cast<float *>(s_c4);
    if (lane < k) s_m[wave * CT_MAX_K + lane] = mx;
    __syncthreads();
    if (tid < k)
        slab_max[((size_t)g * gridDim.x + slab) * CT_MAX_K + tid] =
            fmaxf(fmaxf(s_m[tid], s_m[CT_MAX_K + tid]), fmaxf(s_m[2 * CT_MAX_K + tid], s_m[3 * CT_MAX_K + tid]));
}

// Grid (ceil(P / CT_SLAB), G), CT_THREADS threads: Hn[g][r] for the rows r < grp[g].len
__global__ __launch_bounds__(CT_THREADS) void contrast_norms_kernel(const float *H, double *Hn, const ContrastGroup *grp, int d, int P) {
    const int g = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int len = min(grp[g].len, P), r1 = min((int)(blockIdx.x + 1) * CT_SLAB, len);
    for (int r = blockIdx.x * CT_SLAB + wave; r < r1; r += 4) {
        const double n = ct_row_norm(H + ((size_t)g * P + r) * d, d, lane);
        if (lane == 0) Hn[(size_t)g * P + r] = n;
    }
}

// Threads j < k of a workgroup: pen_j from the group's slab maxima (n_slabs rows of CT_MAX_K; no context row at all: 0), score_j into s_score[j].
// After the barrier every thread returns the winner: the highest score, the lowest j on ties.
__device__ __forceinline__ int contrast_pick(const float *slab_max_g, int len, int k, const float *p, float alpha, float *s_pen, float *s_score) {
    const int j = threadIdx.x;
    if (j < k) {
        float pen = len > 0 ? -INFINITY : 0.0f;
        for (int s = 0; s * CT_SLAB < len; s++) pen = fmaxf(pen, slab_max_g[s * CT_MAX_K + j]);
        s_pen[j] = pen;
        {
#pragma clang fp contract(off)      // two products, each rounded, then the difference: as the contract writes it
            const double keep = (1.0 - (double)alpha) * (double)p[j], off = (double)alpha * (double)pen;
            s_score[j] = (float)(keep - off);
        }
    }
    __syncthreads();
    int w = 0;
    for (int i = 1; i < k; i++) w = s_score[i] > s_score[w] ? i : w;
    return w;
}

// the rank + pick arithmetic alone (biogpt_hip_contrast_rank_device): one group, out = [pen k | score k | winner as int bits]
__global__ __launch_bounds__(CT_THREADS) void contrast_pick_kernel(const float *slab_max, const ContrastGroup *grp, int k, const float *p, float alpha, float *out) {
    __shared__ float s_pen[CT_MAX_K], s_score[CT_MAX_K];
    const int w = contrast_pick(slab_max, grp[0].len, k, p, alpha, s_pen, s_score);
    if (threadIdx.x < k) { out[threadIdx.x] = s_pen[threadIdx.x]; out[k + threadIdx.x] = s_score[threadIdx.x]; }
    if (threadIdx.x == 0) reinterpret_cast<int32_t *>(out)[2 * k] = w;
}

// One workgroup per group.  cand: [G * k][d] hidden rows of this step's columns; logits: [G * k][ldl]; seq: the column states; seq_gen: token histories
// ([column][gen_stride]; a group's output is the row of its first column, seq[g * k].n_gen its length); scores: [G][gen_stride].
__global__ __launch_bounds__(CT_THREADS) void contrast_select_kernel(const float *cand, const float *logits, int ldl, int n_vocab, ContrastCtl *ctl, ContrastGroup *grp,
                                                                     const float *slab_max, int n_slabs, float *H, double *Hn, int d, int P, SeqState *seq,
                                                                     int32_t *seq_gen, int gen_stride, float *scores) {
    __shared__ float s_pen[CT_MAX_K], s_score[CT_MAX_K];
    __shared__ float top_v[SAMPLE_MAX_K];
    __shared__ int top_i[SAMPLE_MAX_K];
    __shared__ double s_S;
    const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    ContrastGroup *const me = grp + g;
    if (me->finished) return;
    const int k = ctl->top_k, len = me->len, first = me->first;
    int w = contrast_pick(slab_max + (size_t)g * n_slabs * CT_MAX_K, len, k, me->p, ctl->alpha, s_pen, s_score);
    if (first) w = 0;
    SeqState *const s0 = seq + (size_t)g * k;
    const int id = first ? -1 : me->id[w];
    const int pos = s0->n_past;      // (all k columns stand at the same position)
    __syncthreads();                 // every thread has read the group's state
    if (!first && tid == 0) {
        const int n = s0->n_gen;
        if (n < gen_stride) { seq_gen[(size_t)g * k * gen_stride + n] = id; scores[(size_t)g * gen_stride + n] = s_score[w]; }
        s0->n_gen = n + 1;
    }
    if (!first && ctl->eos_id >= 0 && id == ctl->eos_id) {      // (uniform) the columns keep their tokens and positions, as the sampler's finished ones do
        if (tid == 0) { me->finished = 1; me->copy_pos = -1; atomicSub(&ctl->n_live, 1); }
        return;
    }
    // the winner's row joins the context
    if (len < P) {
        const float4 *src = reinterpret_cast<const float4 *>(cand + ((size_t)g * k + w) * d);
        float4 *dst = reinterpret_cast<float4 *>(H + ((size_t)g * P + len) * d);
        for (int i = tid; i < (d >> 2); i += CT_THREADS) dst[i] = src[i];
        if (wave == 0) {
            const double n = ct_row_norm(cand + ((size_t)g * k + w) * d, d, lane);
            if (lane == 0) Hn[(size_t)g * P + len] = n;
        }
    }
    // its logits row gives the next candidates
    const float *row = logits + ((size_t)g * k + w) * ldl;
    float m;
    int bi;
    double S;
    lp_row_stats(row, n_vocab, m, bi, S);
    if (tid == 0) s_S = S;
    const int k_eff = sample_topk(row, n_vocab, min(k, n_vocab), top_v, top_i);      // (its barriers publish s_S)
    if (tid < k) {
        const bool have = tid < k_eff;
        me->p[tid] = have ? (float)(exp((double)top_v[tid] - (double)m) / s_S) : 0.0f;
        me->id[tid] = have ? top_i[tid] : 0;
        SeqState *s = s0 + tid;
        s->token = have ? top_i[tid] : 0;
        s->n_past = pos + 1;
    }
    if (tid == 0) {
        me->len = min(len + 1, P);
        me->winner = w;
        me->copy_pos = first ? -1 : pos;      // (a first step wrote the same row into all k slots)
        me->first = 0;
    }
}

// Grid (n_layer * n_head, G), 256 threads: the dk floats of (layer, head, position copy_pos) of K and of V from the winner's slot to the group's others.
// Caches are head-major [slot][layer][head][P][dk]; seq_stride floats between two slots.
__global__ __launch_bounds__(256) void contrast_kv_row_kernel(const ContrastGroup *grp, int k, float *kroot, float *vroot, int64_t seq_stride, int P, int dk) {
    const int g = blockIdx.y, pos = grp[g].copy_pos, w = grp[g].winner;
    if (pos < 0 || pos >= P || grp[g].finished) return;
    const int n4 = dk >> 2;      // float4s per row
    const size_t at = ((size_t)blockIdx.x * P + pos) * dk;
    for (int i = threadIdx.x; i < 2 * k * n4; i += blockDim.x) {
        const int c = i % n4, j = (i / n4) % k;
        if (j == w) continue;
        float *root = i / (n4 * k) == 0 ? kroot : vroot;
        reinterpret_cast<float4 *>(root + (size_t)(g * k + j) * seq_stride + at)[c] =
            reinterpret_cast<const float4 *>(root + (size_t)(g * k + w) * seq_stride + at)[c];
    }
}

}  // namespace bgk
