// The many-column chain of the SIMD association (the "SIMD chain"; opt-in per context, biogpt_hip_assoc_chain): passes over column states of a context in
// mode 1 (biogpt_hip_assoc), in the summation order of an AVX2 build of ggml -- kernels_assoc.hip.h has the order and the oracle's names for it.  Three kernels:
//
//   schain_q8_kernel      the producer: the N activation columns of a linear stage -> Q8_0 / Q8_1 blocks in the context's side buffers, ONCE per stage, behind
//                         the LayerNorm where the site has one.  A workgroup per column; the arithmetic is simd_q8_column itself (called, not restated), so the
//                         bits are those every workgroup of matvec_simd_kernel computes for itself.
//   schain_kernel         the linear stage.  Per (row, column) exactly matvec_simd_kernel's arithmetic: d = d_w * d_y, the eight lanes a_l = fma(d, dot4_l, a_l)
//                         in block order, the Q4_1 / Q5_1 offsets summed apart and unfused, row = ((a0+a4)+(a2+a6)) + ((a1+a5)+(a3+a7)) + summs.  What differs is
//                         who owns what: with many columns a THREAD owns whole (row, column) pairs -- all eight accumulators of CN columns of one row -- so a
//                         row's eight serial fma chains times CN columns are 8 CN independent chains in one thread (they hide the fma latency; the quad split
//                         and its DPP adds were what ONE column forced), and a block's weight bytes are loaded and unpacked once for all CN columns.
//                         Frame: lane = row, a wave = 64 consecutive rows x CN columns, a workgroup = 4 waves on the SAME 64 rows = 64 rows x 4 CN columns (the
//                         four waves' weight loads meet in the L1).  The columns' codes and scales are staged in LDS in phases of SC_KP elements and read as
//                         wave-uniform (broadcast) 16-byte loads; the accumulators live across the phases, so a phase border touches no order.  Any M (rows >= M
//                         re-read row M - 1 and store nothing), any N >= 1 (idle columns re-stage column N - 1 and store nothing), any K % 32 == 0.  A column's
//                         bits depend on nothing but its own codes and the row: not on the tile, on N or on its neighbours.
//   attn_simd_cols_kernel attn_simd_kernel over column states: the column's own slot (seq_id x kv_seq_stride, or slot i), its own count (t_vis, or n_past + 1) and,
//                         SHARED, rows j < pad[0] from slot pad[1].  Where a key's row lies changes an address, never the order.  (A sibling and not template
//                         arguments of attn_simd_kernel: that kernel's code, and so its instantiation in engine.hip, stays as it is.)
#pragma once

#include "kernels_assoc.hip.h"

namespace bgk {

// ---- the producer ------------------------------------------------------------------------------------------------------------------------------------------
// codes oq [N][K] int8, od [N][K / 32] f32 (the value the dot reads: through f16 for Q8_0), os [N][K / 32] words (Q8_0: the integer sum; Q8_1: bits of d * sum)
struct SchainQ8Params {
    const float *x; int32_t ldx, K, N;
    const float *ln_w, *ln_b; float eps;
    int8_t *oq; float *od; uint32_t *os;
};
// grid N, 256 threads: the four waves share the column's 64-chunk groups (each wave has the LayerNorm's sums for itself, in simd_q8_column's one order)
template <bool Q81, bool LN>
__global__ __launch_bounds__(256) void schain_q8_kernel(const SchainQ8Params p) {
    const int n = blockIdx.x, nblk = p.K / QK;
    simd_q8_column<Q81, LN>(p.x + (size_t)n * p.ldx, p.K, p.ln_w, p.ln_b, p.eps, reinterpret_cast<uint32_t *>(p.oq + (size_t)n * p.K), p.od + (size_t)n * nblk,
                            p.os + (size_t)n * nblk, threadIdx.x >> 6, blockDim.x >> 6);
}

// ---- the linear stage --------------------------------------------------------------------------------------------------------------------------------------
constexpr int SC_KP = 1024;                // elements of a K phase
constexpr int SC_NB = SC_KP / QK;          // its blocks
constexpr int SC_TM = 64;                  // rows of a workgroup: one per lane

// CN columns per thread; a workgroup's four waves take 4 CN columns of the same 64 rows
template <int CN_>
struct SchainCfg {
    static constexpr int CN = CN_, TM = SC_TM, TN = 4 * CN_;
    static constexpr int LDS_BYTES = TN * SC_KP + 2 * TN * SC_NB * 4;      // codes, scales, sums (the sums of the Q8_1 forms only)
};
using SchainCfg0 = SchainCfg<1>;      // 64 rows x 4 columns
using SchainCfg1 = SchainCfg<4>;      // 64 rows x 16 columns
using SchainCfg2 = SchainCfg<8>;      // 64 rows x 32 columns

// One block of a row as the eight lanes see it: lane l = elements 4 l .. 4 l + 3 as int8 (load_lane_unit's nibble split and signed settling, for all of a
// quad's threads at once: low nibbles of dword t are lane t, high nibbles lane 4 + t)
template <int WT>
__device__ __forceinline__ void schain_lanes(const Unit<WT> &u, uint32_t (&w)[8]) {
    const uint32_t q[4] = {u.q0.x, u.q0.y, u.q0.z, u.q0.w};
    if (WT == W_Q8_0) {
        w[0] = u.q0.x; w[1] = u.q0.y; w[2] = u.q0.z; w[3] = u.q0.w; w[4] = u.q1.x; w[5] = u.q1.y; w[6] = u.q1.z; w[7] = u.q1.w;
        return;
    }
#pragma unroll
    for (int t = 0; t < 4; t++) {
        uint32_t lo = q[t] & 0x0F0F0F0Fu, hi = (q[t] >> 4) & 0x0F0F0F0Fu;
        if (WT == W_Q5_0 || WT == W_Q5_1) { lo |= spread4(u.qh >> (4 * t)); hi |= spread4(u.qh >> (16 + 4 * t)); }
        if (WT == W_Q4_0 || WT == W_Q5_0) {      // (b + 0x78) ^ 0x80 = b - 8, (b + 0x70) ^ 0x80 = b - 16 in every byte, no carry between bytes
            constexpr uint32_t B = WT == W_Q4_0 ? 0x78787878u : 0x70707070u;
            lo = (lo + B) ^ 0x80808080u; hi = (hi + B) ^ 0x80808080u;
        }
        w[t] = lo; w[4 + t] = hi;
    }
}

// grid (ceil(M / 64), ceil(N / C::TN)), 256 threads.  p.aq_q / aq_d / aq_s: the producer's rows [N][K], [N][K / 32], [N][K / 32].
template <int WT, int EPI, typename C>
__global__ __launch_bounds__(256) void schain_kernel(const MatvecParams p) {
    using TI = TypeInfo<WT>;
    static_assert(TI::quant, "block formats only");
    static_assert(EPI == EPI_QKV || EPI == EPI_RESID || EPI == EPI_GELU || EPI == EPI_LOGITS, "the chain's four sites");
    constexpr int CN = C::CN, TN = C::TN;
    __shared__ __attribute__((aligned(16))) uint32_t s_q[TN * (SC_KP / 4)];      // [column][dword of the phase]
    __shared__ __attribute__((aligned(16))) float s_d[SC_NB * TN];               // [block of the phase][column]
    __shared__ __attribute__((aligned(16))) float s_s[TI::q81 ? SC_NB * TN : 4];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = p.W.K, M = p.W.M, nblk = K / QK;
    const int row = blockIdx.x * SC_TM + lane, col0 = blockIdx.y * TN, cw = wave * CN;
    const int64_t ub = (int64_t)min(row, M - 1) * nblk;

    float a[CN][8], summs[CN];
#pragma unroll
    for (int c = 0; c < CN; c++) {
        summs[c] = 0.0f;
#pragma unroll
        for (int l = 0; l < 8; l++) a[c][l] = 0.0f;
    }

    for (int k0 = 0; k0 < K; k0 += SC_KP) {
        const int nb = min(SC_NB, (K - k0) / QK), b0 = k0 / QK;      // blocks of this phase (the last one may be partial)
        if (k0 > 0) __syncthreads();                                  // every wave is done with the phase before
        const int per = nb * 2;                                       // 16-byte chunks of a column's codes
        for (int i = tid; i < TN * per; i += 256) {
            const int c = i / per, o = i - c * per;
            const int cc = min(col0 + c, p.N - 1);                    // idle columns re-stage the last one
            *reinterpret_cast<uint4 *>(s_q + c * (SC_KP / 4) + 4 * o) = *reinterpret_cast<const uint4 *>(p.aq_q + (size_t)cc * K + k0 + 16 * o);
        }
        for (int i = tid; i < TN * nb; i += 256) {
            const int c = i / nb, b = i - c * nb;
            const size_t at = (size_t)min(col0 + c, p.N - 1) * nblk + b0 + b;
            s_d[b * TN + c] = p.aq_d[at];
            if (TI::q81) s_s[b * TN + c] = __uint_as_float(p.aq_s[at]);
        }
        __syncthreads();
#pragma unroll 2
        for (int b = 0; b < nb; b++) {
            Unit<WT> u;
            load_unit<WT>(u, p.W, ub + b0 + b);
            uint32_t w[8];
            schain_lanes<WT>(u, w);
            const float dw = h2f((uint16_t)(u.sc & 0xFFFFu));
#pragma unroll
            for (int c = 0; c < CN; c++) {
                const uint4 xa = *reinterpret_cast<const uint4 *>(s_q + (cw + c) * (SC_KP / 4) + b * 8);           // wave-uniform: a broadcast
                const uint4 xb = *reinterpret_cast<const uint4 *>(s_q + (cw + c) * (SC_KP / 4) + b * 8 + 4);
                const float d = __fmul_rn(dw, s_d[b * TN + cw + c]);      // F16(d_w) * F16(d_y) / F16(d_w) * d_y
                a[c][0] = __fmaf_rn(d, (float)dot4(w[0], xa.x, 0), a[c][0]);
                a[c][1] = __fmaf_rn(d, (float)dot4(w[1], xa.y, 0), a[c][1]);
                a[c][2] = __fmaf_rn(d, (float)dot4(w[2], xa.z, 0), a[c][2]);
                a[c][3] = __fmaf_rn(d, (float)dot4(w[3], xa.w, 0), a[c][3]);
                a[c][4] = __fmaf_rn(d, (float)dot4(w[4], xb.x, 0), a[c][4]);
                a[c][5] = __fmaf_rn(d, (float)dot4(w[5], xb.y, 0), a[c][5]);
                a[c][6] = __fmaf_rn(d, (float)dot4(w[6], xb.z, 0), a[c][6]);
                a[c][7] = __fmaf_rn(d, (float)dot4(w[7], xb.w, 0), a[c][7]);
                if (TI::q81) summs[c] = __fadd_rn(summs[c], __fmul_rn(h2f((uint16_t)(u.sc >> 16)), s_s[b * TN + cw + c]));
            }
        }
    }

    if (row >= M) return;                                    // rows beyond M are never stored (no barrier behind this line)
#pragma unroll
    for (int c = 0; c < CN; c++) {
        const int col = col0 + cw + c;
        if (col >= p.N) continue;                            // nor columns beyond N
        // hsum_float_8: (a0+a4, a1+a5, a2+a6, a3+a7), then (r0+r2, r1+r3), then their sum; + summs (0 for the symmetric formats: the add is the oracle's)
        const float r0 = __fadd_rn(a[c][0], a[c][4]), r1 = __fadd_rn(a[c][1], a[c][5]), r2 = __fadd_rn(a[c][2], a[c][6]), r3 = __fadd_rn(a[c][3], a[c][7]);
        float v = __fadd_rn(__fadd_rn(__fadd_rn(r0, r2), __fadd_rn(r1, r3)), summs[c]);
        if (EPI == EPI_LOGITS) {
            p.out[(size_t)col * p.ldo + row] = v;
        } else if (EPI == EPI_QKV) {
            const int e_npast = p.seq ? p.seq[col].n_past : p.st->n_past + col;
            const int e_seq = (p.seq && p.col_mode) ? p.seq[col].seq_id : col;
            v = __fadd_rn(p.bias[row], v);
            const int which = row / K, rr = row - which * K;       // d_model == K for the q/k/v projection
            if (which == 0) {
                p.q_out[(size_t)col * K + rr] = __fmul_rn(v, p.q_scale);
            } else {
                float *cache = ((which == 1) ? p.kcache : p.vcache) + (p.seq ? (size_t)e_seq * p.kv_seq_stride : 0);
                const int hh = rr >> p.dk_log2, dd = rr & (p.dk - 1);                                   // head-major cache: [H][P][dk]
                cache[(((size_t)hh * p.P + e_npast) << p.dk_log2) + dd] = v;
            }
        } else if (EPI == EPI_RESID) {
            p.out[(size_t)col * p.ldo + row] = __fadd_rn(__fadd_rn(v, p.bias[row]), p.resid[(size_t)col * p.ldr + row]);
        } else {                                             // EPI_GELU
            p.out[(size_t)col * p.ldo + row] = h2f(p.gelu_tab[f2h(__fadd_rn(p.bias[row], v))]);
        }
    }
}

// ---- attention over column states ------------------------------------------------------------------------------------------------------------------------------
// One workgroup of 256 threads per (head, query column); dk = 64, T <= SIMD_ATTN_MAXT; p.seq is the column states.  attn_simd_kernel's order, operation for
// operation: scores in 4 x 8 fma accumulators reduced 16 / 8 / 4 / pairs, max, fp16-table exp, double sum, (float)(1 / sum), PV with the accumulators j mod 32
// over T & ~31 and the keys beyond one by one, unfused.  Key row j of column i: slot pad[1] while SHARED and j < pad[0], else the column's own slot.
template <bool SHARED>
__global__ __launch_bounds__(256) void attn_simd_cols_kernel(const AttnParams p) {
    __shared__ __attribute__((aligned(16))) float s_q[64];
    __shared__ float s_p[SIMD_ATTN_MAXT];
    __shared__ float s_acc[32][64];
    __shared__ double s_red[16];
    const int h = blockIdx.x, i = blockIdx.y;
    constexpr int dk = 64;
    const int D = p.D, tid = threadIdx.x;
    const SeqState cs = p.seq[i];
    const int T = min(p.col_mode ? cs.t_vis : cs.n_past + 1, SIMD_ATTN_MAXT);
    const size_t head = (size_t)h * p.P * dk;                            // head-major cache: [H][P][dk]
    const size_t own = (size_t)(p.col_mode ? cs.seq_id : i) * p.kv_seq_stride + head;
    const int n_shared = SHARED ? cs.pad[0] : 0;
    const size_t shr = SHARED ? (size_t)cs.pad[1] * p.kv_seq_stride + head : own;
    const float *__restrict__ kown = p.kcache + own, *__restrict__ vown = p.vcache + own;
    const float *__restrict__ kshr = p.kcache + shr, *__restrict__ vshr = p.vcache + shr;
    if (tid < dk) s_q[tid] = p.q[(size_t)i * D + (size_t)h * dk + tid];
    __syncthreads();

    // ---- scores ----
    constexpr int MAXK = SIMD_ATTN_MAXT / 256;
    float sc[MAXK];
#pragma unroll
    for (int kk = 0; kk < MAXK; kk++) {
        const int j = tid + kk * 256;
        sc[kk] = -INFINITY;
        if (j < T) {
            const float4 *kr = reinterpret_cast<const float4 *>(((SHARED && j < n_shared) ? kshr : kown) + (size_t)j * dk);
            float a[32];
#pragma unroll
            for (int half = 0; half < 2; half++) {
#pragma unroll
                for (int c4 = 0; c4 < 8; c4++) {
                    const float4 kv = kr[half * 8 + c4];
                    const float4 qv = reinterpret_cast<const float4 *>(s_q)[half * 8 + c4];
                    a[4 * c4 + 0] = __fmaf_rn(kv.x, qv.x, half ? a[4 * c4 + 0] : 0.0f);
                    a[4 * c4 + 1] = __fmaf_rn(kv.y, qv.y, half ? a[4 * c4 + 1] : 0.0f);
                    a[4 * c4 + 2] = __fmaf_rn(kv.z, qv.z, half ? a[4 * c4 + 2] : 0.0f);
                    a[4 * c4 + 3] = __fmaf_rn(kv.w, qv.w, half ? a[4 * c4 + 3] : 0.0f);
                }
            }
            sc[kk] = simd_reduce32(a);
        }
    }

    // ---- softmax (ggml_soft_max: fp16-table exp, double sum, scale by (float)(1/sum)) ----
    float mx = sc[0];
#pragma unroll
    for (int kk = 1; kk < MAXK; kk++) mx = fmaxf(mx, sc[kk]);
    mx = block_max_f32(mx, reinterpret_cast<float *>(s_red));
    double sum = 0.0;
#pragma unroll
    for (int kk = 0; kk < MAXK; kk++) {
        const int j = tid + kk * 256;
        if (j < T) {
            const float val = h2f(p.exp_tab[f2h(__fsub_rn(sc[kk], mx))]);
            sc[kk] = val;
            sum += (double)val;
        }
    }
    sum = block_sum_f64(sum, s_red);
    const float inv = (float)(1.0 / sum);
#pragma unroll
    for (int kk = 0; kk < MAXK; kk++) {
        const int j = tid + kk * 256;
        if (j < T) s_p[j] = __fmul_rn(sc[kk], inv);
    }
    __syncthreads();

    // ---- PV ----
    const int d = tid & 63, sl = tid >> 6;
    const int Tfull = T & ~31;
    for (int r = sl; r < 32; r += 4) {
        float acc = 0.0f;
        for (int j = r; j < Tfull; j += 32) acc = __fmaf_rn(((SHARED && j < n_shared) ? vshr : vown)[(size_t)j * dk + d], s_p[j], acc);
        s_acc[r][d] = acc;
    }
    __syncthreads();
    if (tid < dk) {
        float a[32];
#pragma unroll
        for (int r = 0; r < 32; r++) a[r] = s_acc[r][tid];
        float o = simd_reduce32(a);
        for (int j = Tfull; j < T; j++) o = __fadd_rn(o, __fmul_rn(((SHARED && j < n_shared) ? vshr : vown)[(size_t)j * dk + tid], s_p[j]));
        p.out[(size_t)i * D + (size_t)h * dk + tid] = o;
    }
}

}  // namespace bgk
