// The many-column linear stage for block-quantized files that are NOT BioGPT-base (the "wide chain": BioGPT-Large's d_model 1600 / d_ff 6400, or any
// d_model % 64 == 0, d_ff % 32 == 0 with head size 64), on v_mfma_i32_16x16x32_i8.
//
// The arithmetic is kernels_mfma.hip.h's, so the results are bit-identical to the generic VALU kernel and to the oracle by construction:
//   per wave = one 16 x 16 output tile, for block b = 0 .. K/32-1 IN ORDER inside one lane:
//     C = A x B (int32, zero-initialised)   the exact integer dot of weight block b (expanded row-tiled image, retile_kernel) and activation block b
//     acc += mfma_block_term<WT>(...)        the reference's unfused mul / mul / add per type; the f32 sum in block order
// What differs is the frame.  kernels_mfma.hip.h is compiled per K (1024 or 4096: whole 1024-element phases, a 4-block software pipeline, DMA staging);
// here K, M and N are run-time values:
//   * K % 32 == 0.  The 16 activation columns of a workgroup are staged in LDS in phases of 1024 elements (32 blocks); the LAST phase may be partial
//     (K = 1600: 32 + 18 blocks; K = 6400: 6 x 32 + 8; K = 96: 3).  One buffer, two barriers per phase: 20.3 KB of LDS (22.4 KB with the Q8_1 sums), so
//     several workgroups share a compute unit and hide each other's staging.  No pipeline of its own: tools/wide_chain_bench.py says what one could win.
//   * any M: the image of a wide file holds ceil(M / 16) tiles, the last one zero-padded (an lm_head of 57717 rows = 3607 tiles + 5 rows); rows >= M are
//     computed on zeros and never stored.  A workgroup = 4 waves = 4 consecutive row tiles (64 rows) x 16 columns; waves past the last tile only keep the
//     barriers company.
//   * any N >= 1: idle columns of the last 16-column tile re-read column N - 1 and store nothing.
// Operand layouts (kernels_mfma.hip.h): A = 8 int8 of row (lane & 15), elements 8 g .. 8 g + 7 of the block (g = lane >> 4); B = the same elements of
// column (lane & 15); C/D = rows 4 g .. 4 g + 3 of column (lane & 15).
// The activations arrive as Q8 blocks ([N][K] int8, [N][K/32] scales and sums): lnq_wide_kernel (LayerNorm + Q8) and q8_rows_kernel (plain Q8) below
// restate the generic mat-vec kernel's prologue (matvec_kernel, PRO_LN / PRO_PLAIN) operation by operation, in its summation order.
#pragma once

#include "kernels_mfma.hip.h"

namespace bgk {

template <bool Q81>
struct WideLds {
    static constexpr int KP = 1024, BPP = KP / QK;
    static constexpr int PITCH = KP + 16;                    // bytes per activation column: the 8-byte operand reads of a 32-lane half cover all 64 banks (kernels_mfma.hip.h)
    static constexpr int SP = BPP + 1;                       // floats per column of block scales: lanes 0 .. 15 read 16 different banks
    static constexpr int OFF_Q = 0;
    static constexpr int OFF_D = OFF_Q + 16 * PITCH;
    static constexpr int OFF_S = OFF_D + 16 * SP * 4;
    static constexpr int BYTES = OFF_S + (Q81 ? 16 * SP * 4 : 0);
};

// EPI: EPI_QKV (column states: seq / col_mode / kv_seq_stride, head-major cache), EPI_RESID, EPI_GELU (f32 rows through the fp16 GELU table), EPI_LOGITS
template <int WT, int EPI>
__global__ __launch_bounds__(256) void matmul_wide_kernel(const MatvecParams p, const DevMatrix img) {
    using TI = TypeInfo<WT>;
    static_assert(TI::quant, "block-quantized weights");
    static_assert(EPI == EPI_QKV || EPI == EPI_RESID || EPI == EPI_GELU || EPI == EPI_LOGITS, "the wide chain's four sites");
    constexpr bool Q81 = TI::q81;
    using L = WideLds<Q81>;
    constexpr int SWF = Q81 ? 32 : 16;                       // floats per (tile, block) of weight scales: d[16 rows] (then m[16 rows])
    __shared__ __attribute__((aligned(16))) unsigned char smem[L::BYTES];
    float *const s_d = reinterpret_cast<float *>(smem + L::OFF_D);
    float *const s_s = reinterpret_cast<float *>(smem + L::OFF_S);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, g = lane >> 4;
    const int K = p.W.K, M = p.W.M, BPR = K / QK;
    const int ntile = (M + 15) >> 4;
    const int col0 = blockIdx.y * 16;
    const int tile = blockIdx.x * 4 + wave;
    const bool tile_ok = tile < ntile;
    const int tile_c = tile_ok ? tile : ntile - 1;

    const uint8_t *const aq = img.qs + ((size_t)tile_c * BPR * 16 + li) * 32 + 8 * g;                   // block b of the tile is 512 bytes further
    const float *const wsc = reinterpret_cast<const float *>(img.sc) + (size_t)tile_c * BPR * SWF + 4 * g;   // rows 4g .. 4g+3; block b is SWF floats further
    const unsigned char *const bq = smem + L::OFF_Q + li * L::PITCH + 8 * g;                            // block b of the phase is 32 bytes further
    const i32x4 zero = {0, 0, 0, 0};
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};

    auto block_steps = [&](int b0, int b, auto count) {
        constexpr int NB = decltype(count)::value;
        uint2 a[NB]; float4 dw[NB], mw[NB]; long xb[NB]; float xd[NB], xs[NB]; i32x4 d[NB];
#pragma unroll
        for (int j = 0; j < NB; j++) {
            a[j] = *reinterpret_cast<const uint2 *>(aq + (size_t)(b0 + b + j) * 512);
            dw[j] = *reinterpret_cast<const float4 *>(wsc + (size_t)(b0 + b + j) * SWF);
            mw[j] = Q81 ? *reinterpret_cast<const float4 *>(wsc + (size_t)(b0 + b + j) * SWF + 16) : make_float4(0.f, 0.f, 0.f, 0.f);
            xb[j] = *reinterpret_cast<const long *>(bq + (b + j) * QK);
            xd[j] = s_d[li * L::SP + b + j];
            xs[j] = Q81 ? s_s[li * L::SP + b + j] : 0.0f;
        }
#pragma unroll
        for (int j = 0; j < NB; j++) d[j] = __builtin_amdgcn_mfma_i32_16x16x32_i8((long)(((unsigned long)a[j].y << 32) | a[j].x), xb[j], zero, 0, 0, 0);
#pragma unroll
        for (int j = 0; j < NB; j++) {
            acc[0] = __fadd_rn(acc[0], mfma_block_term<WT>((float)d[j][0], dw[j].x, mw[j].x, xd[j], xs[j]));
            acc[1] = __fadd_rn(acc[1], mfma_block_term<WT>((float)d[j][1], dw[j].y, mw[j].y, xd[j], xs[j]));
            acc[2] = __fadd_rn(acc[2], mfma_block_term<WT>((float)d[j][2], dw[j].z, mw[j].z, xd[j], xs[j]));
            acc[3] = __fadd_rn(acc[3], mfma_block_term<WT>((float)d[j][3], dw[j].w, mw[j].w, xd[j], xs[j]));
        }
    };

    for (int b0 = 0; b0 < BPR; b0 += L::BPP) {
        const int nb = min(L::BPP, BPR - b0);                // blocks of this phase (the last one may be partial)
        if (b0 > 0) __syncthreads();                         // every wave is done with the phase before
        const int per = nb * 2;                              // 16-byte pieces per column
        for (int i = tid; i < 16 * per; i += 256) {
            const int c = i / per, o = i - c * per;
            const int cc = min(col0 + c, p.N - 1);           // idle columns re-read the last one
            *reinterpret_cast<uint4 *>(smem + L::OFF_Q + c * L::PITCH + o * 16) =
                *reinterpret_cast<const uint4 *>(p.aq_q + (size_t)cc * K + (size_t)b0 * QK + (size_t)o * 16);
        }
        for (int i = tid; i < 16 * nb; i += 256) {
            const int c = i / nb, b = i - c * nb;
            const int cc = min(col0 + c, p.N - 1);
            s_d[c * L::SP + b] = p.aq_d[(size_t)cc * BPR + b0 + b];
            if (Q81) s_s[c * L::SP + b] = __uint_as_float(p.aq_s[(size_t)cc * BPR + b0 + b]);
        }
        __syncthreads();
        if (!tile_ok) continue;
        // four blocks' operands are requested together (independent loads), then the four integer dots; the sums stay in block order
        int b = 0;
        for (; b + 4 <= nb; b += 4) block_steps(b0, b, std::integral_constant<int, 4>{});
        for (; b < nb; b++) block_steps(b0, b, std::integral_constant<int, 1>{});
    }

    const int col = col0 + li, orow = tile * 16 + 4 * g;     // this lane's outputs: rows orow .. orow + 3 of column col
    if (!tile_ok || col >= p.N) return;
    if (EPI == EPI_LOGITS) {                                 // n_vocab need not be a multiple of 4: row by row, rows >= M are never stored
#pragma unroll
        for (int r = 0; r < 4; r++)
            if (orow + r < M) p.out[(size_t)col * p.ldo + orow + r] = acc[r];
        return;
    }
    if (orow >= M) return;                                   // (16 | M at the three layer sites)
    const float4 eb = *reinterpret_cast<const float4 *>(p.bias + orow);
    if (EPI == EPI_QKV) {
        const int e_npast = p.seq ? p.seq[col].n_past : p.st->n_past + col;
        const int e_seq = (p.seq && p.col_mode) ? p.seq[col].seq_id : col;
        float4 v;
        v.x = __fadd_rn(eb.x, acc[0]); v.y = __fadd_rn(eb.y, acc[1]); v.z = __fadd_rn(eb.z, acc[2]); v.w = __fadd_rn(eb.w, acc[3]);
        const int which = orow / K, rr = orow - which * K;   // d_model == K for the q/k/v projection
        if (which == 0) {
            v.x = __fmul_rn(v.x, p.q_scale); v.y = __fmul_rn(v.y, p.q_scale); v.z = __fmul_rn(v.z, p.q_scale); v.w = __fmul_rn(v.w, p.q_scale);
            *reinterpret_cast<float4 *>(p.q_out + (size_t)col * K + rr) = v;
        } else {
            float *cache = ((which == 1) ? p.kcache : p.vcache) + (p.seq ? (size_t)e_seq * p.kv_seq_stride : 0);
            const int hh = rr >> p.dk_log2, dd = rr & (p.dk - 1);                                       // head-major cache: [H][P][dk]; 4 | dk
            *reinterpret_cast<float4 *>(cache + (((size_t)hh * p.P + e_npast) << p.dk_log2) + dd) = v;
        }
    } else if (EPI == EPI_RESID) {
        const float4 er = *reinterpret_cast<const float4 *>(p.resid + (size_t)col * p.ldr + orow);
        float4 v;
        v.x = __fadd_rn(__fadd_rn(acc[0], eb.x), er.x); v.y = __fadd_rn(__fadd_rn(acc[1], eb.y), er.y);
        v.z = __fadd_rn(__fadd_rn(acc[2], eb.z), er.z); v.w = __fadd_rn(__fadd_rn(acc[3], eb.w), er.w);
        *reinterpret_cast<float4 *>(p.out + (size_t)col * p.ldo + orow) = v;
    } else {                                                 // EPI_GELU
        float4 v;
        v.x = h2f(p.gelu_tab[f2h(__fadd_rn(eb.x, acc[0]))]); v.y = h2f(p.gelu_tab[f2h(__fadd_rn(eb.y, acc[1]))]);
        v.z = h2f(p.gelu_tab[f2h(__fadd_rn(eb.z, acc[2]))]); v.w = h2f(p.gelu_tab[f2h(__fadd_rn(eb.w, acc[3]))]);
        *reinterpret_cast<float4 *>(p.out + (size_t)col * p.ldo + orow) = v;
    }
}

// quantize_row_q8_0 / _q8_1 of one 4-element chunk whose 32-element block is 8 consecutive lanes (matvec_kernel's prologue): Q8_0 keeps the
// fp16-rounded d and the integer block sum, Q8_1 the f32 d and s = sum * d.  Every lane of the group calls it; `live` is uniform in the group.
template <bool Q81>
__device__ __forceinline__ void wide_q8_chunk(const float4 v, bool live, size_t col, int K, int ch, int8_t *oq_q, float *oq_d, uint32_t *oq_s) {
    const float amax = group8_max(fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
    const float d = amax / 127.0f;
    const float id = (d != 0.0f) ? 1.0f / d : 0.0f;
    const int q0 = (int)roundf(__fmul_rn(v.x, id)), q1 = (int)roundf(__fmul_rn(v.y, id));
    const int q2 = (int)roundf(__fmul_rn(v.z, id)), q3 = (int)roundf(__fmul_rn(v.w, id));
    const int isum = group8_sum(q0 + q1 + q2 + q3);
    if (!live) return;
    reinterpret_cast<uint32_t *>(oq_q + col * K)[ch] = (uint32_t)(q0 & 0xFF) | ((uint32_t)(q1 & 0xFF) << 8) | ((uint32_t)(q2 & 0xFF) << 16) | ((uint32_t)(q3 & 0xFF) << 24);
    if ((ch & 7) == 0) {
        const size_t b = col * (size_t)(K / QK) + (ch >> 3);
        if (Q81) { oq_d[b] = d; oq_s[b] = __float_as_uint(__fmul_rn((float)isum, d)); }
        else { oq_d[b] = h2f(f2h(d)); oq_s[b] = (uint32_t)isum; }
    }
}

// LayerNorm + Q8 of N columns of K values, any K % 32 == 0: one WAVE per column, four columns per workgroup.  matvec_kernel's PRO_LN prologue: lane l
// sums chunks l, l + 64, .. in that order in double, the wave sum, mean = (float)(s / (double)K) (K is no power of two), the variance likewise.
template <bool Q81>
__global__ __launch_bounds__(256) void lnq_wide_kernel(const float *x, int ldx, int K, int N, const float *ln_w, const float *ln_b, float eps,
                                                       int8_t *oq_q, float *oq_d, uint32_t *oq_s) {
    const int lane = threadIdx.x & 63, col = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (col >= N) return;                                    // (a whole wave)
    const int nchunks = K >> 2, njj = (nchunks + 63) >> 6;
    const float4 *xcol = reinterpret_cast<const float4 *>(x + (size_t)col * ldx);
    double s1 = 0.0;
    for (int i = 0; i < njj; i++) {
        const int ch = i * 64 + lane;
        const float4 v = ch < nchunks ? xcol[ch] : make_float4(0.f, 0.f, 0.f, 0.f);
        s1 += ((double)v.x + (double)v.y) + ((double)v.z + (double)v.w);
    }
    s1 = wave_sum_f64(s1);
    const float mean = (float)(s1 / (double)K);
    double s2 = 0.0;
    for (int i = 0; i < njj; i++) {
        const int ch = i * 64 + lane;
        if (ch < nchunks) {
            const float4 v = xcol[ch];
            const float a = __fsub_rn(v.x, mean), b = __fsub_rn(v.y, mean), c = __fsub_rn(v.z, mean), d = __fsub_rn(v.w, mean);
            s2 += ((double)__fmul_rn(a, a) + (double)__fmul_rn(b, b)) + ((double)__fmul_rn(c, c) + (double)__fmul_rn(d, d));
        }
    }
    s2 = wave_sum_f64(s2);
    const float var = (float)(s2 / (double)K);
    const float scale = 1.0f / sqrtf(__fadd_rn(var, eps));
    for (int i = 0; i < njj; i++) {
        const int ch = i * 64 + lane;
        const bool live = ch < nchunks;                      // 8 | K / 4: uniform in a block's 8 lanes
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (live) {
            const float4 xv = xcol[ch], w = reinterpret_cast<const float4 *>(ln_w)[ch], b = reinterpret_cast<const float4 *>(ln_b)[ch];
            v.x = __fadd_rn(__fmul_rn(w.x, __fmul_rn(__fsub_rn(xv.x, mean), scale)), b.x);
            v.y = __fadd_rn(__fmul_rn(w.y, __fmul_rn(__fsub_rn(xv.y, mean), scale)), b.y);
            v.z = __fadd_rn(__fmul_rn(w.z, __fmul_rn(__fsub_rn(xv.z, mean), scale)), b.z);
            v.w = __fadd_rn(__fmul_rn(w.w, __fmul_rn(__fsub_rn(xv.w, mean), scale)), b.w);
        }
        wide_q8_chunk<Q81>(v, live, (size_t)col, K, ch, oq_q, oq_d, oq_s);
    }
}

// plain Q8 of N f32 rows of K values (the attention output, the fc1 output): grid (ceil(K / 1024), N), a thread per 4-element chunk
template <bool Q81>
__global__ __launch_bounds__(256) void q8_rows_kernel(const float *x, int ldx, int K, int8_t *oq_q, float *oq_d, uint32_t *oq_s) {
    const int col = blockIdx.y, ch = blockIdx.x * 256 + threadIdx.x;
    const bool live = ch < (K >> 2);
    const float4 v = live ? reinterpret_cast<const float4 *>(x + (size_t)col * ldx)[ch] : make_float4(0.f, 0.f, 0.f, 0.f);
    wide_q8_chunk<Q81>(v, live, (size_t)col, K, ch, oq_q, oq_d, oq_s);
}

}  // namespace bgk
