// Evals of 2 .. 8 tokens of the context's own columns of block-quantized files that are NOT BioGPT-base (BioGPT-Large: 1600 / 6400 / 25 heads): the wide
// decode layer's flat walk (kernels_wdecode.hip.h) with the column as a second axis.  Seven dependent launches per layer, every width a run-time value:
//
//   (LayerNorm -> Q8)   lnq_wide_kernel on the N columns of x                                                                       biogpt.cpp:664-686
//   wchunk_qkv_kernel   the workgroup's q/k/v rows of N columns -> bias, Q scale, KV append at the column's position              biogpt.cpp:688-727
//   (attention)         attn_fast_kernel, which leaves out_proj's Q8 blocks per column                                              biogpt.cpp:729-764
//   wchunk_resid_kernel out_proj rows + bias + residual into [N][D]                                                                 biogpt.cpp:767-772
//   (LayerNorm -> Q8)   lnq_wide_kernel on the N columns of x1
//   wchunk_fc1_kernel   32 fc1 rows -> bias -> GELU table -> ONE Q8 block of fc2's activations per column                           biogpt.cpp:777-787
//   wchunk_resid_kernel fc2 rows + bias + residual                                                                                  biogpt.cpp:790-795
//
// The split is the decode layer's: workgroup g of G owns the contiguous rows [g M / G, (g + 1) M / G) (fc1: exactly 32 rows, one Q8 block of fc2's
// activation row), its threads walk the run's K / 32-weight units as one flat index u = tid, tid + NT, .., and the next pass's unit is requested before this
// pass's dots.  What is new is how a unit meets N columns:
//
//   activations through LDS   every stage reads Q8 blocks a producer launch wrote ([N][K] codes, [N][K / 32] scales and sums).  The workgroup copies the N
//                             columns' blocks into LDS ONCE, as one flat run of 16-byte words, while its first weight units are in flight; a lane then reads
//                             its unit's 32 codes x N from LDS (two ds_read_b128 per column) instead of N x 32 bytes per unit from L2.
//   weights unpacked once     a lane loads its unit once, settles it once (wchunk_settle: nibbles and high bits to bytes) and dots the settled unit against
//                             the N columns' blocks in a loop (wchunk_dot: 8 dot4 and the format's f32 expression -- unit_dot_quant's, per (unit, column)).
//                             Each f32 block term goes to LDS at [column][row][block]; no accumulator lives across columns, so N is a run-time bound.
//   finish                    after one workgroup barrier a finisher thread per (row, column) -- pair i on wave i % NW, lane i / NW, so consecutive pairs
//                             sit in different waves -- adds its row's terms in block order from 0.0f (wdec_row_sum) and applies the epilogue.
//
// A column's cache position is wchunk_col_pos: the one place that maps a column to where it lives (today: the context's own slot, position n_past + c).
#pragma once

#include "kernels_wdecode.hip.h"

namespace bgk {

constexpr int WCHUNK_MIN_COLS = 2, WCHUNK_MAX_COLS = 8;

struct WchunkParams {
    DevMatrix W;
    int32_t N;                 // columns, WCHUNK_MIN_COLS .. WCHUNK_MAX_COLS
    int32_t bpr;               // blocks per row, K / 32
    int32_t pstride;           // floats between two rows of block terms in LDS (wdec_pstride)
    int32_t max_rows;          // most rows of a workgroup: rows between two columns of block terms in LDS
    // the producer's blocks: [N][K] codes, [N][K / 32] scales and sums
    const int8_t *aq_q; const float *aq_d; const uint32_t *aq_s;
    const float *bias;         // [M]
    const float *resid;        // out_proj / fc2: [N][M]
    float *out;                // out_proj / fc2: [N][M]
    // q/k/v
    float *q_out, *kcache, *vcache;      // [N][D]; layer slices, head-major [H][P][64]
    int32_t D, P;
    float q_scale;
    const DevState *st;
    // fc1
    const uint16_t *gelu_tab;
    int8_t *oq_q; float *oq_d; uint32_t *oq_s;      // [N][M] codes, [N][M / 32] scales and sums
};

// LDS, in this order (every part at a multiple of 16 bytes): [codes N K | d N bpr | s N bpr | fc1: gelu N x 32 | block terms [N][max_rows][pstride]]
__host__ __device__ inline size_t wchunk_blocks_bytes(int N, int K) { return wdec_r16((size_t)N * K) + 2 * wdec_r16((size_t)N * (K / QK) * 4); }
__host__ __device__ inline size_t wchunk_smem_bytes(bool fc1, int N, int K, int max_rows) {
    return wchunk_blocks_bytes(N, K) + (fc1 ? (size_t)N * WDEC_FC1_ROWS * 4 : 0) + (size_t)N * max_rows * wdec_pstride(K / QK) * 4;
}
struct WchunkLds { uint32_t *xq; float *xd; uint32_t *xs; float *g; float *part; };
__device__ __forceinline__ WchunkLds wchunk_lds(unsigned char *smem, bool fc1, int N, int K) {
    WchunkLds l{};
    const size_t bq = wdec_r16((size_t)N * K), bd = wdec_r16((size_t)N * (K / QK) * 4);
    l.xq = reinterpret_cast<uint32_t *>(smem); l.xd = reinterpret_cast<float *>(smem + bq); l.xs = reinterpret_cast<uint32_t *>(smem + bq + bd);
    smem += bq + 2 * bd;
    l.g = reinterpret_cast<float *>(smem);
    if (fc1) smem += (size_t)N * WDEC_FC1_ROWS * 4;
    l.part = reinterpret_cast<float *>(smem);
    return l;
}

// where column c of the call lives: its position in the context's own cache slot
__device__ __forceinline__ int wchunk_col_pos(const WchunkParams &p, int c) { return p.st->n_past + c; }

// The N columns' blocks from the producer's rows into LDS: one flat run each (the columns lie one behind another).  No barrier: the walk's first one follows.
__device__ __forceinline__ void wchunk_stage_blocks(const WchunkParams &p, const WchunkLds &l) {
    const int NT = blockDim.x, n16 = (p.N * p.W.K) >> 4, nb = p.N * p.bpr;      // 32 | K: whole 16-byte words
    const uint4 *src = reinterpret_cast<const uint4 *>(p.aq_q);
    uint4 *dst = reinterpret_cast<uint4 *>(l.xq);
    for (int i = threadIdx.x; i < n16; i += NT) dst[i] = src[i];
    for (int i = threadIdx.x; i < nb; i += NT) { l.xd[i] = p.aq_d[i]; l.xs[i] = p.aq_s[i]; }
}

// "settle the unit": what of unit_dot_quant does not depend on the column -- the nibbles (and Q5's high bits) as 32 bytes, elements 0 .. 15 in q0, 16 .. 31 in
// q1 (expand_unit, kernels.hip.h).  Q8_0 units are bytes already.
template <int WT>
__device__ __forceinline__ void wchunk_settle(Unit<WT> &u) {
    if constexpr (WT != W_Q8_0) expand_unit<WT>(u);
}
// "dot a settled unit": 8 dot4 and the format's block term, unit_dot_quant's expressions element for element
template <int WT>
__device__ __forceinline__ float wchunk_dot(const Unit<WT> &u, const uint32_t *xq, float xd, uint32_t xs) {
    if constexpr (WT == W_Q8_0) return unit_dot_quant<WT>(u, xq, xd, __uint_as_float(xs), (int)xs);
    else return unit_dot_expanded<WT>(u, xq, xd, __uint_as_float(xs), (int)xs);
}

// The flat walk over the workgroup's nunits units (weights unit0 + u) against the N columns in LDS: block terms to part[column][row][block].  cur: unit tid,
// requested by the caller at kernel entry, in front of the copy of the blocks.  Ends with the workgroup barrier the finishers wait for.
template <int WT>
__device__ __forceinline__ void wchunk_terms(const WchunkParams &p, int64_t unit0, int nunits, Unit<WT> cur, const WchunkLds &l) {
    const int NT = blockDim.x, N = p.N, bpr = p.bpr, K4 = p.W.K >> 2, cstride = p.max_rows * p.pstride;
    __syncthreads();                                             // the blocks are in LDS
    for (int u = threadIdx.x; u < nunits; u += NT) {
        Unit<WT> nxt;
        if (u + NT < nunits) load_unit<WT>(nxt, p.W, unit0 + u + NT);
        wchunk_settle<WT>(cur);
        const int row = u / bpr, blk = u - row * bpr;
        const uint32_t *xq = l.xq + blk * 8;
        const float *xd = l.xd + blk;
        const uint32_t *xs = l.xs + blk;
        float *part = l.part + row * p.pstride + blk;
        for (int c = 0; c < N; c++) {
            part[0] = wchunk_dot<WT>(cur, xq, xd[0], xs[0]);
            xq += K4; xd += bpr; xs += bpr; part += cstride;
        }
        cur = nxt;
    }
    __syncthreads();
}

// the finisher of pair i = column * nrows + row of the workgroup: wave i % NW, lane i / NW (-1: this thread finishes no pair)
__device__ __forceinline__ int wchunk_fin_pair(int npairs) {
    const int NW = blockDim.x >> 6, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane * NW + wave;
    return i < npairs ? i : -1;
}

// ---- q/k/v: rows of the stacked 3 D x D matrix -> bias, Q scale, KV append.  grid G ----
template <int WT>
__global__ __launch_bounds__(1024) void wchunk_qkv_kernel(const WchunkParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int M = p.W.M;
    const WchunkLds l = wchunk_lds(smem, false, p.N, p.W.K);
    const int r0 = wdec_row0(blockIdx.x, gridDim.x, M), nrows = wdec_row0(blockIdx.x + 1, gridDim.x, M) - r0;
    const int nunits = nrows * p.bpr;
    const int64_t unit0 = (int64_t)r0 * p.bpr;
    Unit<WT> cur;
    if ((int)threadIdx.x < nunits) load_unit<WT>(cur, p.W, unit0 + threadIdx.x);
    wchunk_stage_blocks(p, l);
    const int fi = wchunk_fin_pair(nrows * p.N);
    const int c = fi >= 0 ? fi / nrows : 0, i = fi - c * nrows;
    float e_bias = 0.0f;
    int pos = 0;
    if (fi >= 0) { e_bias = p.bias[r0 + i]; pos = wchunk_col_pos(p, c); }
    wchunk_terms<WT>(p, unit0, nunits, cur, l);
    if (fi >= 0) {
        const float v = __fadd_rn(e_bias, wdec_row_sum(l.part + ((size_t)c * p.max_rows + i) * p.pstride, p.bpr));
        const int r = r0 + i, which = r / p.D, rr = r - which * p.D;
        if (which == 0) {
            p.q_out[(size_t)c * p.D + rr] = __fmul_rn(v, p.q_scale);      // Q scaled AFTER the bias (biogpt.cpp:708-710)
        } else {                                                           // KV append (biogpt.cpp:721-727), head-major cache
            float *cache = (which == 1) ? p.kcache : p.vcache;
            cache[((size_t)(rr >> 6) * p.P + pos) * 64 + (rr & 63)] = v;
        }
    }
}

// ---- out_proj / fc2: rows + bias + residual into [N][M].  grid G ----
template <int WT>
__global__ __launch_bounds__(1024) void wchunk_resid_kernel(const WchunkParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int M = p.W.M;
    const WchunkLds l = wchunk_lds(smem, false, p.N, p.W.K);
    const int r0 = wdec_row0(blockIdx.x, gridDim.x, M), nrows = wdec_row0(blockIdx.x + 1, gridDim.x, M) - r0;
    const int nunits = nrows * p.bpr;
    const int64_t unit0 = (int64_t)r0 * p.bpr;
    Unit<WT> cur;
    if ((int)threadIdx.x < nunits) load_unit<WT>(cur, p.W, unit0 + threadIdx.x);
    wchunk_stage_blocks(p, l);
    const int fi = wchunk_fin_pair(nrows * p.N);
    const int c = fi >= 0 ? fi / nrows : 0, i = fi - c * nrows;
    float e_bias = 0.0f, e_res = 0.0f;
    if (fi >= 0) { e_bias = p.bias[r0 + i]; e_res = p.resid[(size_t)c * M + r0 + i]; }
    wchunk_terms<WT>(p, unit0, nunits, cur, l);
    if (fi >= 0) p.out[(size_t)c * M + r0 + i] = __fadd_rn(__fadd_rn(wdec_row_sum(l.part + ((size_t)c * p.max_rows + i) * p.pstride, p.bpr), e_bias), e_res);
}

// ---- fc1: 32 rows -> bias -> GELU table -> their Q8 block of every column's fc2 activation row.  grid M / 32, at least 32 N threads ----
template <int WT>
__global__ __launch_bounds__(1024) void wchunk_fc1_kernel(const WchunkParams p) {
    using TI = TypeInfo<WT>;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int M = p.W.M;
    const WchunkLds l = wchunk_lds(smem, true, p.N, p.W.K);
    const int r0 = blockIdx.x * WDEC_FC1_ROWS;
    const int nunits = WDEC_FC1_ROWS * p.bpr;
    const int64_t unit0 = (int64_t)r0 * p.bpr;
    Unit<WT> cur;
    if ((int)threadIdx.x < nunits) load_unit<WT>(cur, p.W, unit0 + threadIdx.x);
    wchunk_stage_blocks(p, l);
    const int fi = wchunk_fin_pair(WDEC_FC1_ROWS * p.N);      // pair i = column * 32 + row: where the block's value i lies in l.g
    float e_bias = 0.0f;
    if (fi >= 0) e_bias = p.bias[r0 + (fi & (WDEC_FC1_ROWS - 1))];
    wchunk_terms<WT>(p, unit0, nunits, cur, l);
    if (fi >= 0) {
        const int c = fi / WDEC_FC1_ROWS, i = fi - c * WDEC_FC1_ROWS;
        l.g[fi] = h2f(p.gelu_tab[f2h(__fadd_rn(e_bias, wdec_row_sum(l.part + ((size_t)c * p.max_rows + i) * p.pstride, p.bpr)))]);      // ggml_gelu: fp16 table
    }
    __syncthreads();
    if ((int)threadIdx.x < WDEC_FC1_ROWS * p.N) {      // column c: lanes 32 c .. 32 c + 31, one aligned group of 32
        const int c = threadIdx.x / WDEC_FC1_ROWS, i = threadIdx.x & (WDEC_FC1_ROWS - 1);
        int8_t q8; float d8; uint32_t s8;
        q8_block32(l.g[threadIdx.x], TI::q81, q8, d8, s8);
        p.oq_q[(size_t)c * M + r0 + i] = q8;
        if (i == 0) { p.oq_d[(size_t)c * (M / QK) + blockIdx.x] = d8; p.oq_s[(size_t)c * (M / QK) + blockIdx.x] = s8; }
    }
}

}  // namespace bgk
