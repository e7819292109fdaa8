// Single-token decode of block-quantized files that are NOT BioGPT-base (any d_model % 64 == 0, d_ff % 32 == 0, heads of 64 -- BioGPT-Large: 1600 / 6400 /
// 25 heads): five dependent launches per layer like kernels_decode.hip.h, with every width a run-time value.
//
//   wdec_qkv_kernel    LayerNorm -> Q8 of the column ONCE per workgroup -> the workgroup's q/k/v rows -> bias, Q scale, KV append    biogpt.cpp:664-727
//   (attention)        dec_attn_kernel<LPK, 16> of kernels_decode.hip.h up to 256 keys: it indexes by head alone, nothing in it is 1024   biogpt.cpp:729-764
//   wdec_oproj_kernel  out_proj rows + bias + residual, Q8 activations from the attention launch                                     biogpt.cpp:767-772
//   wdec_fc1_kernel    LayerNorm -> Q8 once per workgroup -> 32 fc1 rows -> bias -> GELU table -> ONE Q8 block of fc2's activations   biogpt.cpp:777-787
//   wdec_fc2_kernel    fc2 rows + bias + residual, Q8 activations from fc1                                                           biogpt.cpp:790-795
//
// The split.  A row is K / 32 weight blocks ("units"): 50 at K = 1600, 200 at K = 6400, 6 and 5 in the small test files -- never a divisor of 64, so "lane =
// block" leaves lanes idle.  A workgroup therefore owns a CONTIGUOUS run of rows [r0, r1) and its threads walk the run's units as one flat index u = tid,
// tid + NT, ..: unit u is block u % bpr of row r0 + u / bpr, its weights are unit r0 * bpr + u of the matrix -- consecutive lanes load consecutive 16 / 32-byte
// units, and all lanes but the last pass's tail are busy.  Every unit's f32 block term (unit_dot_quant, the contract's expressions) goes to LDS at
// [row][block]; after ONE workgroup barrier a finisher thread per row adds the row's terms IN BLOCK ORDER from 0.0f (the reference's scalar vec_dot loop) and
// applies the epilogue.  The finishers of consecutive rows sit in different waves (row i: wave i % NW, lane i / NW), so the serial sums run on all SIMDs.
// Rows are dealt to workgroups evenly: workgroup g of G owns rows [g M / G, (g + 1) M / G) -- M need not be a multiple of anything, neighbouring workgroups
// differ by at most one row, none is idle.  G is 256 (one per compute unit) unless that leaves a workgroup less than a wave of units.  fc1 is the exception:
// its workgroup owns exactly one 32-row Q8 block of fc2's activation row (32 | d_ff), so the block is quantized where it is made.
//
// LayerNorm: the order of lnq_wide_kernel / matvec_kernel<PRO_LN> -- lane l adds the double sums of chunks l, l + 64, .. in that order, wave_sum_f64 over the 64
// lanes, (float)(s / (double)K) -- but shared: wave w computes the chunk sums of chunk rows w, w + NW, .. into LDS, wave 0 alone adds them per lane in chunk-row
// order and reduces, and hands mean (then 1 / std) to the others through LDS.  Same operands, same order, so the same doubles.  The Q8 forms are the three-
// instruction ones of kernels_decode.hip.h (bit for bit the divisions and roundf of the generic kernels, with their wave-uniform fall-back).
#pragma once

#include "kernels_decode.hip.h"

namespace bgk {

constexpr int WDEC_MAXCH = 2;          // float4 chunks of the column a thread holds: d_model <= 8 * WDEC_MAXCH * threads
constexpr int WDEC_FC1_ROWS = 32;      // fc1 rows per workgroup: one Q8 block

struct WdecParams {
    DevMatrix W;
    int32_t bpr;               // blocks per row, K / 32
    int32_t pstride;           // floats between two rows of block terms in LDS: bpr rounded up to 4, + 4
    // LayerNorm kernels: the f32 column
    const float *x, *ln_w, *ln_b;
    float eps;
    // Q8-in kernels: the producer's blocks
    const int8_t *aq_q; const float *aq_d; const uint32_t *aq_s;
    const float *bias, *resid;
    float *out;
    // q/k/v
    float *q_out, *kcache, *vcache;      // [D]; layer slices, head-major [H][P][64]
    int32_t D, P;
    float q_scale;
    const DevState *st;
    // fc1
    const uint16_t *gelu_tab;
    int8_t *oq_q; float *oq_d; uint32_t *oq_s;
};

// LDS of the kernels, in this order (every part at a multiple of 16 bytes): [codes K | d bpr | s bpr | chunk sums njj x 64 doubles | mean, 1 / std | gelu 32]
// for the LayerNorm kernels, then the block terms [max_rows][pstride] for all.
__host__ __device__ inline int wdec_pstride(int bpr) { return ((bpr + 3) & ~3) + 4; }
__host__ __device__ inline int wdec_njj(int K) { return ((K >> 2) + 63) >> 6; }
__host__ __device__ inline size_t wdec_r16(size_t b) { return (b + 15) & ~(size_t)15; }
__host__ __device__ inline size_t wdec_ln_bytes(int K) { return wdec_r16((size_t)K) + 2 * wdec_r16((size_t)(K / QK) * 4) + (size_t)wdec_njj(K) * 64 * 8 + 16 + 128; }
__host__ __device__ inline size_t wdec_smem_bytes(bool ln, int K, int max_rows) { return (ln ? wdec_ln_bytes(K) : 0) + (size_t)max_rows * wdec_pstride(K / QK) * 4; }

struct WdecLds {
    uint32_t *xq; float *xd; uint32_t *xs; double *cs; float *stat; float *g; float *part;
};
__device__ __forceinline__ WdecLds wdec_lds(unsigned char *smem, bool ln, int K) {
    WdecLds l{};
    if (ln) {
        const size_t bq = wdec_r16((size_t)K), bd = wdec_r16((size_t)(K / QK) * 4);
        l.xq = reinterpret_cast<uint32_t *>(smem); l.xd = reinterpret_cast<float *>(smem + bq); l.xs = reinterpret_cast<uint32_t *>(smem + bq + bd);
        l.cs = reinterpret_cast<double *>(smem + bq + 2 * bd);
        l.stat = reinterpret_cast<float *>(smem + bq + 2 * bd + (size_t)wdec_njj(K) * 64 * 8);
        l.g = l.stat + 4;
        smem += wdec_ln_bytes(K);
    }
    l.part = reinterpret_cast<float *>(smem);
    return l;
}

// rows of workgroup g of G: [g M / G, (g + 1) M / G)
__host__ __device__ inline int wdec_row0(int g, int G, int M) { return (int)((int64_t)g * M / G); }

// LayerNorm + Q8_0 / Q8_1 of the K-wide column into LDS, once per workgroup; every thread calls it; ends with a workgroup barrier.  blockDim.x * WDEC_MAXCH
// >= K / 4 (the launch sees to it): thread t holds chunks t, t + NT.
template <bool Q81>
__device__ __forceinline__ void wdec_ln_q8(const WdecParams &p, int K, const WdecLds &l) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, NT = blockDim.x, NW = NT >> 6;
    const int nchunks = K >> 2, njj = wdec_njj(K);
    float4 v[WDEC_MAXCH], lw[WDEC_MAXCH], lb[WDEC_MAXCH];
#pragma unroll
    for (int c = 0; c < WDEC_MAXCH; c++) {
        const int ch = tid + c * NT;
        const bool live = ch < nchunks;
        v[c] = live ? reinterpret_cast<const float4 *>(p.x)[ch] : make_float4(0.f, 0.f, 0.f, 0.f);
        lw[c] = live ? reinterpret_cast<const float4 *>(p.ln_w)[ch] : make_float4(0.f, 0.f, 0.f, 0.f);
        lb[c] = live ? reinterpret_cast<const float4 *>(p.ln_b)[ch] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    // chunk row i = wave + c * NW holds chunks i * 64 + lane = tid + c * NT
#pragma unroll
    for (int c = 0; c < WDEC_MAXCH; c++) {
        const int i = wave + c * NW;
        if (i < njj) l.cs[i * 64 + lane] = ((double)v[c].x + (double)v[c].y) + ((double)v[c].z + (double)v[c].w);      // (a chunk past the column: 0.0, as lnq_wide_kernel adds it)
    }
    __syncthreads();
    if (wave == 0) {
        double s1 = 0.0;
        for (int i = 0; i < njj; i++) s1 += l.cs[i * 64 + lane];
        s1 = wave_sum_f64(s1);
        if (lane == 0) l.stat[0] = (float)(s1 / (double)K);
    }
    __syncthreads();
    const float mean = l.stat[0];
#pragma unroll
    for (int c = 0; c < WDEC_MAXCH; c++) {
        const int i = wave + c * NW;
        v[c].x = __fsub_rn(v[c].x, mean); v[c].y = __fsub_rn(v[c].y, mean); v[c].z = __fsub_rn(v[c].z, mean); v[c].w = __fsub_rn(v[c].w, mean);
        if (i < njj) {
            const bool live = tid + c * NT < nchunks;
            const double s = ((double)__fmul_rn(v[c].x, v[c].x) + (double)__fmul_rn(v[c].y, v[c].y)) + ((double)__fmul_rn(v[c].z, v[c].z) + (double)__fmul_rn(v[c].w, v[c].w));
            l.cs[i * 64 + lane] = live ? s : 0.0;
        }
    }
    __syncthreads();
    if (wave == 0) {
        double s2 = 0.0;
        for (int i = 0; i < njj; i++) s2 += l.cs[i * 64 + lane];
        s2 = wave_sum_f64(s2);
        const float var = (float)(s2 / (double)K);
        const float scale = ln_inv_std(__fadd_rn(var, p.eps));
        if (lane == 0) l.stat[1] = scale;
    }
    __syncthreads();
    const float scale = l.stat[1];
#pragma unroll
    for (int c = 0; c < WDEC_MAXCH; c++) {
        const int i = wave + c * NW, ch = tid + c * NT;
        if (i >= njj) continue;                                  // (a whole wave)
        const bool live = ch < nchunks;                          // 8 | K / 4: uniform in a block's 8 lanes
        float a = 0.f, b = 0.f, cc = 0.f, d4 = 0.f;
        if (live) {
            a = __fadd_rn(__fmul_rn(lw[c].x, __fmul_rn(v[c].x, scale)), lb[c].x);
            b = __fadd_rn(__fmul_rn(lw[c].y, __fmul_rn(v[c].y, scale)), lb[c].y);
            cc = __fadd_rn(__fmul_rn(lw[c].z, __fmul_rn(v[c].z, scale)), lb[c].z);
            d4 = __fadd_rn(__fmul_rn(lw[c].w, __fmul_rn(v[c].w, scale)), lb[c].w);
        }
        // quantize_row_q8_0 / q8_1: one block = 8 consecutive lanes x 4 values
        const float amax = group8_max(fmaxf(fmaxf(fabsf(a), fabsf(b)), fmaxf(fabsf(cc), fabsf(d4))));
        float d, id;
        q8_scales(amax, d, id);
        const int q0 = q8_round(__fmul_rn(a, id)), q1 = q8_round(__fmul_rn(b, id)), q2 = q8_round(__fmul_rn(cc, id)), q3 = q8_round(__fmul_rn(d4, id));
        const int isum = group8_sum(q0 + q1 + q2 + q3);
        if (live) {
            l.xq[ch] = (uint32_t)(q0 & 0xFF) | ((uint32_t)(q1 & 0xFF) << 8) | ((uint32_t)(q2 & 0xFF) << 16) | ((uint32_t)(q3 & 0xFF) << 24);
            if ((ch & 7) == 0) {
                const int blk = ch >> 3;
                if (Q81) { l.xd[blk] = d; l.xs[blk] = __float_as_uint(__fmul_rn((float)isum, d)); }
                else { l.xd[blk] = h2f(f2h(d)); l.xs[blk] = (uint32_t)isum; }
            }
        }
    }
    __syncthreads();
}

// The flat walk over the workgroup's nunits units (weights unit0 + u): block terms to part[row][block].  cur: unit tid, loaded by the caller at kernel entry
// (in front of the LayerNorm); the next pass's unit is requested before this pass's dot.  LDSX: the activation blocks are in LDS (xq / xd / xs), else they
// are the producer launch's rows in memory.  Ends with a workgroup barrier.
template <int WT, bool LDSX>
__device__ __forceinline__ void wdec_terms(const WdecParams &p, int64_t unit0, int nunits, Unit<WT> cur, const uint32_t *xq, const float *xd, const uint32_t *xs, float *part) {
    const int NT = blockDim.x;
    for (int u = threadIdx.x; u < nunits; u += NT) {
        Unit<WT> nxt;
        if (u + NT < nunits) load_unit<WT>(nxt, p.W, unit0 + u + NT);
        const int row = u / p.bpr, blk = u - row * p.bpr;
        float t;
        if (LDSX) {
            const uint32_t s = xs[blk];
            t = unit_dot_quant<WT>(cur, xq + blk * 8, xd[blk], __uint_as_float(s), (int)s);
        } else {
            uint32_t ax[8];
            const uint4 *aq = reinterpret_cast<const uint4 *>(xq) + blk * 2;
            const uint4 a = aq[0], b = aq[1];
            ax[0] = a.x; ax[1] = a.y; ax[2] = a.z; ax[3] = a.w; ax[4] = b.x; ax[5] = b.y; ax[6] = b.z; ax[7] = b.w;
            const uint32_t s = xs[blk];
            t = unit_dot_quant<WT>(cur, ax, xd[blk], __uint_as_float(s), (int)s);
        }
        part[row * p.pstride + blk] = t;
        cur = nxt;
    }
    __syncthreads();
}

// sumf = 0; for b: sumf += c_b (ggml_vec_dot_q*_q8_* scalar order); the row's pad floats behind bpr are read and not added
__device__ __forceinline__ float wdec_row_sum(const float *part, int bpr) {
    const float4 *p4 = reinterpret_cast<const float4 *>(part);
    float s = 0.0f;
    int b = 0;
    for (; b + 16 <= bpr; b += 16) {
        float4 t[4];
#pragma unroll
        for (int j = 0; j < 4; j++) t[j] = p4[(b >> 2) + j];
#pragma unroll
        for (int j = 0; j < 4; j++) { s = __fadd_rn(s, t[j].x); s = __fadd_rn(s, t[j].y); s = __fadd_rn(s, t[j].z); s = __fadd_rn(s, t[j].w); }
    }
    for (; b < bpr; b += 4) {
        const float4 t = p4[b >> 2];
        s = __fadd_rn(s, t.x);
        if (b + 1 < bpr) s = __fadd_rn(s, t.y);
        if (b + 2 < bpr) s = __fadd_rn(s, t.z);
        if (b + 3 < bpr) s = __fadd_rn(s, t.w);
    }
    return s;
}
// the finisher of the workgroup's row i: wave i % NW, lane i / NW (-1: this thread finishes no row)
__device__ __forceinline__ int wdec_fin_row(int nrows) {
    const int NW = blockDim.x >> 6, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane * NW + wave;
    return i < nrows ? i : -1;
}

// ---- A: LayerNorm -> Q8 -> q/k/v rows -> bias, Q scale, KV append.  grid G, M = 3 D stacked rows ----
template <int WT>
__global__ __launch_bounds__(1024) void wdec_qkv_kernel(const WdecParams p) {
    using TI = TypeInfo<WT>;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int K = p.W.K, M = p.W.M;
    const WdecLds l = wdec_lds(smem, true, K);
    const int r0 = wdec_row0(blockIdx.x, gridDim.x, M), nrows = wdec_row0(blockIdx.x + 1, gridDim.x, M) - r0;
    const int nunits = nrows * p.bpr;
    const int64_t unit0 = (int64_t)r0 * p.bpr;
    Unit<WT> cur;
    if ((int)threadIdx.x < nunits) load_unit<WT>(cur, p.W, unit0 + threadIdx.x);
    const int fi = wdec_fin_row(nrows);
    float e_bias = 0.0f;
    int n_past = 0;
    if (fi >= 0) { e_bias = p.bias[r0 + fi]; n_past = p.st->n_past; }
    wdec_ln_q8<TI::q81>(p, K, l);
    wdec_terms<WT, true>(p, unit0, nunits, cur, l.xq, l.xd, l.xs, l.part);
    if (fi >= 0) {
        const float v = __fadd_rn(e_bias, wdec_row_sum(l.part + fi * p.pstride, p.bpr));
        const int r = r0 + fi, which = r / p.D, rr = r - which * p.D;
        if (which == 0) {
            p.q_out[rr] = __fmul_rn(v, p.q_scale);               // Q scaled AFTER the bias (biogpt.cpp:708-710)
        } else {                                                  // KV append (biogpt.cpp:721-727), head-major cache: where EPI_QKV puts the row
            float *cache = (which == 1) ? p.kcache : p.vcache;
            cache[((size_t)(rr >> 6) * p.P + n_past) * 64 + (rr & 63)] = v;
        }
    }
}

// ---- C / E: rows + bias + residual on the producer launch's Q8 blocks.  grid G ----
template <int WT>
__device__ __forceinline__ void wdec_resid_rows(const WdecParams &p, unsigned char *smem) {
    const int M = p.W.M;
    const WdecLds l = wdec_lds(smem, false, p.W.K);
    const int r0 = wdec_row0(blockIdx.x, gridDim.x, M), nrows = wdec_row0(blockIdx.x + 1, gridDim.x, M) - r0;
    const int nunits = nrows * p.bpr;
    const int64_t unit0 = (int64_t)r0 * p.bpr;
    Unit<WT> cur;
    if ((int)threadIdx.x < nunits) load_unit<WT>(cur, p.W, unit0 + threadIdx.x);
    const int fi = wdec_fin_row(nrows);
    float e_bias = 0.0f, e_res = 0.0f;
    if (fi >= 0) { e_bias = p.bias[r0 + fi]; e_res = p.resid[r0 + fi]; }
    wdec_terms<WT, false>(p, unit0, nunits, cur, reinterpret_cast<const uint32_t *>(p.aq_q), p.aq_d, p.aq_s, l.part);
    if (fi >= 0) p.out[r0 + fi] = __fadd_rn(__fadd_rn(wdec_row_sum(l.part + fi * p.pstride, p.bpr), e_bias), e_res);
}
// out_proj: short rows (d_model / 32 blocks), a few hundred threads
template <int WT>
__global__ __launch_bounds__(1024) void wdec_oproj_kernel(const WdecParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    wdec_resid_rows<WT>(p, smem);
}
// fc2: long rows (d_ff / 32 blocks): the same walk, up to two passes of it per thread at BioGPT-Large
template <int WT>
__global__ __launch_bounds__(1024) void wdec_fc2_kernel(const WdecParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    wdec_resid_rows<WT>(p, smem);
}

// ---- D: LayerNorm -> Q8 -> 32 fc1 rows -> bias -> GELU table -> their Q8 block for fc2.  grid d_ff / 32 ----
template <int WT>
__global__ __launch_bounds__(1024) void wdec_fc1_kernel(const WdecParams p) {
    using TI = TypeInfo<WT>;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int K = p.W.K;
    const WdecLds l = wdec_lds(smem, true, K);
    const int r0 = blockIdx.x * WDEC_FC1_ROWS;
    const int nunits = WDEC_FC1_ROWS * p.bpr;
    const int64_t unit0 = (int64_t)r0 * p.bpr;
    Unit<WT> cur;
    if ((int)threadIdx.x < nunits) load_unit<WT>(cur, p.W, unit0 + threadIdx.x);
    const int fi = wdec_fin_row(WDEC_FC1_ROWS);
    float e_bias = 0.0f;
    if (fi >= 0) e_bias = p.bias[r0 + fi];
    wdec_ln_q8<TI::q81>(p, K, l);
    wdec_terms<WT, true>(p, unit0, nunits, cur, l.xq, l.xd, l.xs, l.part);
    if (fi >= 0) l.g[fi] = h2f(p.gelu_tab[f2h(__fadd_rn(e_bias, wdec_row_sum(l.part + fi * p.pstride, p.bpr)))]);      // ggml_gelu: fp16 table
    __syncthreads();
    if (threadIdx.x < WDEC_FC1_ROWS) {      // (lanes 0-31 of wave 0: one aligned group of 32)
        int8_t q8; float d8; uint32_t s8;
        q8_block32(l.g[threadIdx.x], TI::q81, q8, d8, s8);
        p.oq_q[(size_t)blockIdx.x * 32 + threadIdx.x] = q8;
        if (threadIdx.x == 0) { p.oq_d[blockIdx.x] = d8; p.oq_s[blockIdx.x] = s8; }
    }
}

}  // namespace bgk
