// The many-column linear stage for F32 / F16 files (the "float chain"; opt-in per context, biogpt_hip_float_chain): passes over column states of a float
// file with heads of 64, d_model % 64 == 0, d_ff % 32 == 0.  The weights are read straight from the arena in the file's row-major layout: no second image.
//
// The arithmetic is the oracle's vec_dot_f32 / vec_dot_f16 (and fdec_kernel's, matvec_kernel's): every product rounded to f32 (__fmul_rn, never contracted),
// the running sum in double, ONE rounding to f32 at the end; with F16 weights the activation is first rounded through fp16 (ggml's fp32_to_fp16_row).  The
// association is this kernel's own -- like the two kernels named above it treats the double sum as order-insensitive at f32 precision:
//   a group of KS lanes shares RM rows x TN columns; lane ks of the group takes the 16-byte weight chunks ks, ks + KS, .. of every K phase in order, the
//   elements of a chunk in order, and keeps one double per (row, column); the KS partial sums meet in an xor butterfly.
// Frame: a workgroup = 4 waves = 256 / KS groups = TM = 256 / KS * RM consecutive rows x TN columns.  The TN columns are staged in LDS as f32 (fp16-rounded for
// F16 weights) in phases of FC_LDS_FLOATS / TN elements (32 KB a workgroup, the last phase may be partial: K % 32 == 0 is all the kernel asks), so a
// workgroup's weight bytes are loaded ONCE for the whole column tile, into registers, 16 bytes a lane.  Any M (rows >= M re-read row M - 1 and store
// nothing), any N >= 1 (idle columns re-stage column N - 1 and store nothing).
// Three tile shapes (FchainCfg), chosen by the launch from the grid they give (fchain_tu.hip; DESIGN.md 4.7 has the sweep): few columns want the whole
// chip on the K axis, many columns want a workgroup's weights to serve 16 columns.
// The epilogues are matmul_wide_kernel's, operation for operation, one output per store.
// fchain_ln_kernel is the producer: LayerNorm ONCE per column and site into f32 rows, matvec_kernel<PRO_LN>'s prologue operation for operation (lane l sums
// chunks l, l + 64, .. in double, the wave sum, (float)(s / K), 1.0f / sqrtf(var + eps), w * (x * scale) + b unfused), rounded through fp16 for F16 files.
// ln_rows_kernel (kernels_embed.hip.h) has the same arithmetic but one workgroup per column and no fp16 rounding; this one is a wave per column.
#pragma once

#include "kernels.hip.h"

namespace bgk {

constexpr int FC_LDS_FLOATS = 8192;      // staged activations of one phase: TN columns x (FC_LDS_FLOATS / TN) elements

// KS lanes per output group, RM rows per group, TN columns per workgroup
template <int KS_, int RM_, int TN_>
struct FchainCfg {
    static constexpr int KS = KS_, RM = RM_, TN = TN_;
    static constexpr int TM = 256 / KS * RM;             // rows per workgroup
    static constexpr int KP = FC_LDS_FLOATS / TN;        // elements per phase
    static constexpr int PITCH = KP + 4;                 // floats per staged column (16-byte aligned; columns start on different banks)
    static constexpr int LDS_BYTES = TN * PITCH * 4;
};
using FchainCfg0 = FchainCfg<64, 1, 8>;      // 4 rows x 8 columns: a wave per row
using FchainCfg1 = FchainCfg<16, 2, 8>;      // 32 rows x 8 columns
using FchainCfg2 = FchainCfg<8, 2, 16>;      // 64 rows x 16 columns

template <int WT, int EPI, typename C>
__global__ __launch_bounds__(256) void fchain_kernel(const MatvecParams p) {
    static_assert(WT == W_F32 || WT == W_F16, "float weights");
    static_assert(EPI == EPI_QKV || EPI == EPI_RESID || EPI == EPI_GELU || EPI == EPI_LOGITS, "the chain's four sites");
    constexpr int KS = C::KS, RM = C::RM, TN = C::TN, KP = C::KP, PITCH = C::PITCH;
    constexpr int CH = WT == W_F32 ? 4 : 8;                  // elements of a 16-byte weight chunk
    __shared__ __attribute__((aligned(16))) float s_x[TN * PITCH];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ks = lane % KS, g = wave * (64 / KS) + lane / KS;
    const int K = p.W.K, M = p.W.M;
    const int row0 = blockIdx.x * C::TM + g * RM, col0 = blockIdx.y * TN;

    const uint4 *wrow[RM];
#pragma unroll
    for (int r = 0; r < RM; r++) wrow[r] = reinterpret_cast<const uint4 *>(p.W.qs + (size_t)min(row0 + r, M - 1) * (size_t)K * (16 / CH));
    double acc[RM][TN];
#pragma unroll
    for (int r = 0; r < RM; r++)
#pragma unroll
        for (int c = 0; c < TN; c++) acc[r][c] = 0.0;

    for (int k0 = 0; k0 < K; k0 += KP) {
        const int ne = min(KP, K - k0);                      // elements of this phase (the last one may be partial; a multiple of 32)
        if (k0 > 0) __syncthreads();                         // every wave is done with the phase before
        const int per = ne >> 2;
        for (int i = tid; i < TN * per; i += 256) {
            const int c = i / per, o = i - c * per;
            const int cc = min(col0 + c, p.N - 1);           // idle columns re-stage the last one
            float4 v = *reinterpret_cast<const float4 *>(p.x + (size_t)cc * p.ldx + k0 + 4 * o);
            if (WT == W_F16) { v.x = h2f(f2h(v.x)); v.y = h2f(f2h(v.y)); v.z = h2f(f2h(v.z)); v.w = h2f(f2h(v.w)); }
            *reinterpret_cast<float4 *>(s_x + c * PITCH + 4 * o) = v;
        }
        __syncthreads();
        const int nch = ne / CH, ch0 = k0 / CH;
#pragma unroll 2
        for (int ch = ks; ch < nch; ch += KS) {
            uint4 w[RM];
#pragma unroll
            for (int r = 0; r < RM; r++) w[r] = wrow[r][ch0 + ch];
#pragma unroll
            for (int c = 0; c < TN; c++) {
                const float4 x0 = *reinterpret_cast<const float4 *>(s_x + c * PITCH + ch * CH);
                if (WT == W_F32) {
#pragma unroll
                    for (int r = 0; r < RM; r++) {
                        double a = acc[r][c];
                        a += (double)__fmul_rn(__uint_as_float(w[r].x), x0.x); a += (double)__fmul_rn(__uint_as_float(w[r].y), x0.y);
                        a += (double)__fmul_rn(__uint_as_float(w[r].z), x0.z); a += (double)__fmul_rn(__uint_as_float(w[r].w), x0.w);
                        acc[r][c] = a;
                    }
                } else {
                    const float4 x1 = *reinterpret_cast<const float4 *>(s_x + c * PITCH + ch * CH + 4);
#pragma unroll
                    for (int r = 0; r < RM; r++) {
                        double a = acc[r][c];
                        a += (double)__fmul_rn(h2f((uint16_t)(w[r].x & 0xFFFFu)), x0.x); a += (double)__fmul_rn(h2f((uint16_t)(w[r].x >> 16)), x0.y);
                        a += (double)__fmul_rn(h2f((uint16_t)(w[r].y & 0xFFFFu)), x0.z); a += (double)__fmul_rn(h2f((uint16_t)(w[r].y >> 16)), x0.w);
                        a += (double)__fmul_rn(h2f((uint16_t)(w[r].z & 0xFFFFu)), x1.x); a += (double)__fmul_rn(h2f((uint16_t)(w[r].z >> 16)), x1.y);
                        a += (double)__fmul_rn(h2f((uint16_t)(w[r].w & 0xFFFFu)), x1.z); a += (double)__fmul_rn(h2f((uint16_t)(w[r].w >> 16)), x1.w);
                        acc[r][c] = a;
                    }
                }
            }
        }
    }

    // the group's KS partial sums, then output j = r * TN + c of the group goes to its lane j % KS: one rounding to f32, the epilogue, one store
#pragma unroll
    for (int r = 0; r < RM; r++) {
#pragma unroll
        for (int c = 0; c < TN; c++) {
            const double tot = wave_xor_sum(acc[r][c], KS);
            if (((r * TN + c) % KS) != ks) continue;
            const int row = row0 + r, col = col0 + c;
            if (row >= M || col >= p.N) continue;            // rows beyond M and columns beyond N are never stored
            const float a = (float)tot;
            if (EPI == EPI_LOGITS) {
                p.out[(size_t)col * p.ldo + row] = a;
            } else if (EPI == EPI_QKV) {
                const int e_npast = p.seq ? p.seq[col].n_past : p.st->n_past + col;
                const int e_seq = (p.seq && p.col_mode) ? p.seq[col].seq_id : col;
                const float v = __fadd_rn(p.bias[row], a);
                const int which = row / K, rr = row - which * K;       // d_model == K for the q/k/v projection
                if (which == 0) {
                    p.q_out[(size_t)col * K + rr] = __fmul_rn(v, p.q_scale);
                } else {
                    float *cache = ((which == 1) ? p.kcache : p.vcache) + (p.seq ? (size_t)e_seq * p.kv_seq_stride : 0);
                    const int hh = rr >> p.dk_log2, dd = rr & (p.dk - 1);                                   // head-major cache: [H][P][dk]
                    cache[(((size_t)hh * p.P + e_npast) << p.dk_log2) + dd] = v;
                }
            } else if (EPI == EPI_RESID) {
                p.out[(size_t)col * p.ldo + row] = __fadd_rn(__fadd_rn(a, p.bias[row]), p.resid[(size_t)col * p.ldr + row]);
            } else {                                         // EPI_GELU
                p.out[(size_t)col * p.ldo + row] = h2f(p.gelu_tab[f2h(__fadd_rn(p.bias[row], a))]);
            }
        }
    }
}

// LayerNorm of N columns of K values (K % 4 == 0) into f32 rows out[N][K]: one WAVE per column, four columns per workgroup.  matvec_kernel's PRO_LN prologue:
// lane l sums chunks l, l + 64, .. in that order in double, the wave sum, mean = (float)(s / (double)K), the variance likewise.  F16: the rows are rounded
// through fp16 (what the mat-vec of an F16 file does to its activation row).
template <bool F16>
__global__ __launch_bounds__(256) void fchain_ln_kernel(const float *x, int ldx, int K, int N, const float *ln_w, const float *ln_b, float eps, float *out) {
    const int lane = threadIdx.x & 63, col = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (col >= N) return;                                    // (a whole wave)
    const int nchunks = K >> 2;
    const float4 *xcol = reinterpret_cast<const float4 *>(x + (size_t)col * ldx);
    double s1 = 0.0;
    for (int ch = lane; ch < nchunks; ch += 64) {
        const float4 v = xcol[ch];
        s1 += ((double)v.x + (double)v.y) + ((double)v.z + (double)v.w);
    }
    s1 = wave_sum_f64(s1);
    const float mean = (float)(s1 / (double)K);
    double s2 = 0.0;
    for (int ch = lane; ch < nchunks; ch += 64) {
        const float4 v = xcol[ch];
        const float a = __fsub_rn(v.x, mean), b = __fsub_rn(v.y, mean), c = __fsub_rn(v.z, mean), d = __fsub_rn(v.w, mean);
        s2 += ((double)__fmul_rn(a, a) + (double)__fmul_rn(b, b)) + ((double)__fmul_rn(c, c) + (double)__fmul_rn(d, d));
    }
    s2 = wave_sum_f64(s2);
    const float var = (float)(s2 / (double)K);
    const float scale = 1.0f / sqrtf(__fadd_rn(var, eps));
    for (int ch = lane; ch < nchunks; ch += 64) {
        const float4 xv = xcol[ch], w = reinterpret_cast<const float4 *>(ln_w)[ch], b = reinterpret_cast<const float4 *>(ln_b)[ch];
        float4 v;
        v.x = __fadd_rn(__fmul_rn(w.x, __fmul_rn(__fsub_rn(xv.x, mean), scale)), b.x);
        v.y = __fadd_rn(__fmul_rn(w.y, __fmul_rn(__fsub_rn(xv.y, mean), scale)), b.y);
        v.z = __fadd_rn(__fmul_rn(w.z, __fmul_rn(__fsub_rn(xv.z, mean), scale)), b.z);
        v.w = __fadd_rn(__fmul_rn(w.w, __fmul_rn(__fsub_rn(xv.w, mean), scale)), b.w);
        if (F16) { v.x = h2f(f2h(v.x)); v.y = h2f(f2h(v.y)); v.z = h2f(f2h(v.z)); v.w = h2f(f2h(v.w)); }
        reinterpret_cast<float4 *>(out + (size_t)col * K)[ch] = v;
    }
}

}  // namespace bgk
