// The SIMD association (biogpt_hip_assoc, mode 1): the forward pass in the summation order of an AVX2 build of ggml -- what the oracle computes with
// bo_opts.assoc = 3 (oracle/biogpt_oracle.c: quantize_block_q8_avx2, vec_dot_simd, vec_dot_f32_simd).  Three things differ from the scalar association
// of kernels.hip.h, and nothing else does:
//
//   activation rows   id = 127 / amax (one correctly rounded division, not 1 / fl(amax / 127)), codes rounded to nearest-even (not roundf)
//   block dot         eight f32 accumulators; per block, lane l takes the exact integer sum of the products of elements 4l .. 4l+3 (one v_dot4_i32_i8:
//                     what vpmaddubsw / vpmaddwd leave in a lane) as acc_l = fma(d, (float)q_l, acc_l); the Q4_1 / Q5_1 offsets m_w * s_y are summed apart,
//                     unfused, in block order; row = ((a0+a4)+(a2+a6)) + ((a1+a5)+(a3+a7)) + summs
//   attention         QK^T and PV are f32 dots of 32 accumulators (4 vectors x 8 lanes), fma in ascending order, reduced 16 / 8 / 4 / pairs; the
//                     keys beyond a multiple of 32 are added one by one, unfused
//
// Every rounding is spelled (__fmul_rn / __fadd_rn / __fmaf_rn / __fdiv_rn): the oracle is built without contraction, hipcc contracts a*b + c.
//
// matvec_simd_kernel: a row is eight serial fma chains over its K / 32 blocks, so a K-split is not available -- the parallelism is rows x lanes x columns.
// Four threads share a row: thread t owns the accumulators a_t and a_(t+4) in registers, i.e. elements 4t .. 4t+3 and 16+4t .. 16+4t+3 of every block.
// In all five formats both groups come out of dword t of the block's quants (low / high nibbles; dword t of either half of a Q8_0 block), so a thread
// loads 4 (8) bytes per block and the four threads of a row read its 16 (32) contiguous bytes.  The quad's final sums are two DPP steps.  (DESIGN.md 4.7
// says why not lane sums through LDS to an in-order finisher.)
#pragma once

#include "kernels.hip.h"

namespace bgk {

constexpr int SIMD_ATTN_MAXT = 1024;      // keys attn_simd_kernel holds
constexpr int SIMD_MAX_COLS = 8;          // columns per workgroup of matvec_simd_kernel

// LDS of matvec_simd_kernel: the activation layout of matvec_kernel -- [xq int8 [NC][K] | xd f32 [NC][K/32 + 4] | xs words [NC][K/32 + 4] | tail 256 B]
__host__ __device__ inline size_t matvec_simd_smem_bytes(int K, int NC) {
    return (((size_t)NC * K + 2 * (size_t)NC * (K / QK + 4) * 4 + 256) + 255) & ~(size_t)255;
}

// One activation column x [K] -> Q8_0 / Q8_1 blocks in LDS (xq: K / 4 dwords, xd / xs: one word per block), by ONE wave: behind the LayerNorm of
// matvec_kernel when LN (the same double sums in the same order: mode 0 and mode 1 normalise alike).  The wave converts the 64-chunk groups
// first, first + step, ...; a 32-block is 8 consecutive float4 chunks = 8 consecutive lanes.  Every lane of the wave must be here (DPP reductions).
template <bool Q81, bool LN>
__device__ __forceinline__ void simd_q8_column(const float *x, int K, const float *ln_w, const float *ln_b, float eps, uint32_t *xq, float *xd, uint32_t *xs,
                                               int first, int step) {
    const int lane = threadIdx.x & 63;
    const int nchunks = K >> 2;
    const float4 *xc = reinterpret_cast<const float4 *>(x);
    float mean = 0.0f, scale = 1.0f;
    if (LN) {
        // ggml_norm: mean and variance accumulate in double; y = (x-mean) * 1/sqrtf(var+eps); then *w, +b
        double s1 = 0.0;
        for (int ch = lane; ch < nchunks; ch += 64) {
            const float4 v = xc[ch];
            s1 += ((double)v.x + (double)v.y) + ((double)v.z + (double)v.w);
        }
        s1 = wave_sum_f64(s1);
        mean = (float)(s1 / (double)K);
        double s2 = 0.0;
        for (int ch = lane; ch < nchunks; ch += 64) {
            float4 v = xc[ch];
            v.x = __fsub_rn(v.x, mean); v.y = __fsub_rn(v.y, mean); v.z = __fsub_rn(v.z, mean); v.w = __fsub_rn(v.w, mean);
            s2 += ((double)__fmul_rn(v.x, v.x) + (double)__fmul_rn(v.y, v.y)) + ((double)__fmul_rn(v.z, v.z) + (double)__fmul_rn(v.w, v.w));
        }
        s2 = wave_sum_f64(s2);
        const float var = (float)(s2 / (double)K);
        scale = 1.0f / sqrtf(__fadd_rn(var, eps));
    }
    for (int base = first * 64; base < nchunks; base += step * 64) {      // wave-uniform
        const int ch = base + lane;
        const bool live = ch < nchunks;      // (8 | nchunks: a block's eight lanes are live together)
        float4 v = live ? xc[ch] : make_float4(0.f, 0.f, 0.f, 0.f);
        if (LN && live) {
            const float4 w = reinterpret_cast<const float4 *>(ln_w)[ch];
            const float4 b = reinterpret_cast<const float4 *>(ln_b)[ch];
            v.x = __fadd_rn(__fmul_rn(w.x, __fmul_rn(__fsub_rn(v.x, mean), scale)), b.x);
            v.y = __fadd_rn(__fmul_rn(w.y, __fmul_rn(__fsub_rn(v.y, mean), scale)), b.y);
            v.z = __fadd_rn(__fmul_rn(w.z, __fmul_rn(__fsub_rn(v.z, mean), scale)), b.z);
            v.w = __fadd_rn(__fmul_rn(w.w, __fmul_rn(__fsub_rn(v.w, mean), scale)), b.w);
        }
        // quantize_row_q8_0 / q8_1 of an AVX2 build: d = amax / 127, id = 127 / amax, nearest-even
        const float amax = group8_max(fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
        const float d = __fdiv_rn(amax, 127.0f);
        const float id = (amax != 0.0f) ? __fdiv_rn(127.0f, amax) : 0.0f;
        const int q0 = __float2int_rn(__fmul_rn(v.x, id)), q1 = __float2int_rn(__fmul_rn(v.y, id));
        const int q2 = __float2int_rn(__fmul_rn(v.z, id)), q3 = __float2int_rn(__fmul_rn(v.w, id));
        const int isum = group8_sum(q0 + q1 + q2 + q3);
        if (live) {
            xq[ch] = (uint32_t)(q0 & 0xFF) | ((uint32_t)(q1 & 0xFF) << 8) | ((uint32_t)(q2 & 0xFF) << 16) | ((uint32_t)(q3 & 0xFF) << 24);
            if ((ch & 7) == 0) {
                const int b = ch >> 3;
                if (Q81) {
                    xd[b] = d;                                                   // Q8_1 keeps f32 d
                    xs[b] = __float_as_uint(__fmul_rn(d, (float)isum));          // s = d * sum
                } else {
                    xd[b] = h2f(f2h(d));                                         // Q8_0 stores fp16 d
                    xs[b] = (uint32_t)isum;
                }
            }
        }
    }
}

// The rows alone (biogpt_hip_assoc_device, stage 0): one workgroup of 256 threads per row, through simd_q8_column and the LDS layout of the mat-vec;
// codes [N][K] int8, d [N][K/32] f32 (the value the dot reads: through f16 for Q8_0), s [N][K/32] words (Q8_0: the integer sum; Q8_1: bits of d * sum)
struct Q8SimdParams {
    const float *x; int32_t K, N, q81;
    const float *ln_w, *ln_b; float eps;
    int8_t *oq; float *od; uint32_t *os;
};
__global__ __launch_bounds__(256) void q8_simd_rows_kernel(const Q8SimdParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int K = p.K, nblk = K / QK, nblk_pad = nblk + 4;
    uint32_t *const s_xq = reinterpret_cast<uint32_t *>(smem_raw);
    float *const s_xd = reinterpret_cast<float *>(smem_raw + (size_t)K);
    uint32_t *const s_xs = reinterpret_cast<uint32_t *>(s_xd + nblk_pad);
    const int n = blockIdx.x, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    const float *x = p.x + (size_t)n * K;
    if (p.ln_w) {
        if (p.q81) simd_q8_column<true, true>(x, K, p.ln_w, p.ln_b, p.eps, s_xq, s_xd, s_xs, wave, nwaves);
        else simd_q8_column<false, true>(x, K, p.ln_w, p.ln_b, p.eps, s_xq, s_xd, s_xs, wave, nwaves);
    } else {
        if (p.q81) simd_q8_column<true, false>(x, K, nullptr, nullptr, 0.0f, s_xq, s_xd, s_xs, wave, nwaves);
        else simd_q8_column<false, false>(x, K, nullptr, nullptr, 0.0f, s_xq, s_xd, s_xs, wave, nwaves);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < K / 4; i += blockDim.x) reinterpret_cast<uint32_t *>(p.oq + (size_t)n * K)[i] = s_xq[i];
    for (int b = threadIdx.x; b < nblk; b += blockDim.x) { p.od[(size_t)n * nblk + b] = s_xd[b]; p.os[(size_t)n * nblk + b] = s_xs[b]; }
}

// What thread t of a row's quad holds of one block: its two groups of four weights as int8 dwords (signed for Q4_0 / Q5_0, as settle_unit: the block dot
// is sum (q_j - 8) y_j itself), and the scale word (fp16 d, or half2 {d, m})
struct LaneUnit { uint32_t lo, hi, sc; };
template <int WT>
__device__ __forceinline__ LaneUnit load_lane_unit(const DevMatrix &W, int64_t idx, int t) {
    using TI = TypeInfo<WT>;
    typedef const __attribute__((address_space(1))) uint32_t *gptr32;
    typedef const __attribute__((address_space(1))) uint16_t *gptr16;
    LaneUnit u;
    const gptr32 q = (gptr32)(W.qs + idx * TI::qbytes);
    if (WT == W_Q8_0) {
        u.lo = q[t]; u.hi = q[4 + t];
    } else {
        const uint32_t w = q[t];
        u.lo = w & 0x0F0F0F0Fu; u.hi = (w >> 4) & 0x0F0F0F0Fu;
        if (WT == W_Q5_0 || WT == W_Q5_1) {
            const uint32_t qh = ((gptr32)W.qh)[idx];
            u.lo |= spread4(qh >> (4 * t)); u.hi |= spread4(qh >> (16 + 4 * t));
        }
        if (WT == W_Q4_0 || WT == W_Q5_0) {      // (b + 0x78) ^ 0x80 = b - 8, (b + 0x70) ^ 0x80 = b - 16 in every byte, no carry between bytes
            constexpr uint32_t B = WT == W_Q4_0 ? 0x78787878u : 0x70707070u;
            u.lo = (u.lo + B) ^ 0x80808080u; u.hi = (u.hi + B) ^ 0x80808080u;
        }
    }
    u.sc = TI::q81 ? ((gptr32)W.sc)[idx] : (uint32_t)((gptr16)W.sc)[idx];
    return u;
}

// grid (ceil(M / p.rpw), ceil(N / NC)), 64 .. 256 threads; p.rpw: rows per workgroup, a multiple of blockDim / 4.  Dynamic LDS: matvec_simd_smem_bytes(K, NC).
template <int WT, int PRO, int EPI, int NC>
__global__ __launch_bounds__(256) void matvec_simd_kernel(const MatvecParams p) {
    using TI = TypeInfo<WT>;
    static_assert(TI::quant, "block formats only");
    static_assert(PRO == PRO_LN || PRO == PRO_PLAIN, "f32 activation columns");
    static_assert(NC >= 1 && NC <= SIMD_MAX_COLS, "1 .. 8 columns per workgroup");
    if (EPI == EPI_LOGITS) seq_forward(p.lineage, SEQ_LM_HEAD);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int K = p.W.K, M = p.W.M;
    const int nblk = K / QK, nblk_pad = nblk + 4;
    uint32_t *const s_xq = reinterpret_cast<uint32_t *>(smem_raw);
    float *const s_xd = reinterpret_cast<float *>(smem_raw + (size_t)NC * K);
    uint32_t *const s_xs = reinterpret_cast<uint32_t *>(s_xd + (size_t)NC * nblk_pad);
    float *const s_tail = reinterpret_cast<float *>(s_xs + (size_t)NC * nblk_pad);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = blockDim.x >> 6;
    const int col0 = blockIdx.y * NC;
    const int ncols = min(NC, p.N - col0);

    // ---- prologue: [LayerNorm] + Q8 rows into LDS.  One column: the waves share it; several: a wave owns whole columns ----
    if (NC == 1) {
        simd_q8_column<TI::q81, PRO == PRO_LN>(p.x + (size_t)col0 * p.ldx, K, p.ln_w, p.ln_b, p.eps, s_xq, s_xd, s_xs, wave, nwaves);
    } else {
        for (int c = wave; c < ncols; c += nwaves)
            simd_q8_column<TI::q81, PRO == PRO_LN>(p.x + (size_t)(col0 + c) * p.ldx, K, p.ln_w, p.ln_b, p.eps, s_xq + (size_t)c * (K / 4), s_xd + c * nblk_pad,
                                                   s_xs + c * nblk_pad, 0, 1);
    }
    __syncthreads();

    // ---- rows: thread t of a quad owns a_t and a_(t+4) of every column ----
    const int t = tid & 3;
    const int rstep = blockDim.x >> 2;
    const int64_t row_base = (int64_t)blockIdx.x * p.rpw;
    float best_val = -INFINITY;
    int best_idx = 0x7fffffff;
    for (int r0 = tid >> 2; r0 < p.rpw; r0 += rstep) {
        const int64_t row = row_base + r0;
        if (row >= M) break;      // (a quad shares its row: whole quads leave)
        float a_lo[NC], a_hi[NC], summs[NC];
#pragma unroll
        for (int c = 0; c < NC; c++) { a_lo[c] = 0.0f; a_hi[c] = 0.0f; summs[c] = 0.0f; }
        const int64_t ub = row * nblk;
#pragma unroll 4
        for (int b = 0; b < nblk; b++) {
            const LaneUnit u = load_lane_unit<WT>(p.W, ub + b, t);
            const float dw = h2f((uint16_t)(u.sc & 0xFFFFu));
#pragma unroll
            for (int c = 0; c < NC; c++) {
                if (c >= ncols) continue;
                const uint32_t *xq = s_xq + (size_t)c * (K / 4) + b * 8;
                const float d = __fmul_rn(dw, s_xd[c * nblk_pad + b]);      // F16(d_w) * F16(d_y) / F16(d_w) * d_y
                a_lo[c] = __fmaf_rn(d, (float)dot4(u.lo, xq[t], 0), a_lo[c]);
                a_hi[c] = __fmaf_rn(d, (float)dot4(u.hi, xq[4 + t], 0), a_hi[c]);
                if (TI::q81) summs[c] = __fadd_rn(summs[c], __fmul_rn(h2f((uint16_t)(u.sc >> 16)), __uint_as_float(s_xs[c * nblk_pad + b])));
            }
        }
        const int r = (int)row;
#pragma unroll
        for (int c = 0; c < NC; c++) {
            if (c >= ncols) continue;
            // hsum_float_8: (a0+a4, a1+a5, a2+a6, a3+a7), then (r0+r2, r1+r3), then their sum; + summs (0 for the symmetric formats: the add is the oracle's)
            float v = __fadd_rn(a_lo[c], a_hi[c]);
            v = __fadd_rn(v, dpp_f<DPP_QUAD_XOR2>(v));
            v = __fadd_rn(v, dpp_f<DPP_QUAD_XOR1>(v));
            v = __fadd_rn(v, summs[c]);
            if (t != 0) continue;
            const int col = col0 + c;
            if (EPI == EPI_QKV) {
                v = __fadd_rn(p.bias[r], v);
                const int which = r / p.D, rr = r - which * p.D;
                if (which == 0) {
                    p.q_out[(size_t)col * p.D + rr] = __fmul_rn(v, p.q_scale);
                } else {
                    float *cache = (which == 1) ? p.kcache : p.vcache;
                    const int hh = rr / p.dk, dd = rr - hh * p.dk;  // head-major cache: [H][P][dk]
                    cache[((size_t)hh * p.P + (p.st->n_past + col)) * p.dk + dd] = v;
                }
            } else if (EPI == EPI_RESID) {
                v = __fadd_rn(v, p.bias[r]);
                p.out[(size_t)col * p.ldo + r] = __fadd_rn(v, p.resid[(size_t)col * p.ldr + r]);
            } else if (EPI == EPI_GELU) {
                v = __fadd_rn(p.bias[r], v);
                p.out[(size_t)col * p.ldo + r] = h2f(p.gelu_tab[f2h(v)]);
            } else {
                p.out[(size_t)col * p.ldo + r] = v;
                if (c == 0 && (v > best_val || (v == best_val && r < best_idx))) { best_val = v; best_idx = r; }
            }
        }
    }

    if (EPI == EPI_LOGITS && p.pmax_val != nullptr) {
        // per-workgroup partial arg-max of column 0 (lowest index wins ties), finished by argmax_kernel
        for (int off = 32; off > 0; off >>= 1) {
            const float ov = __shfl_xor(best_val, off, 64);
            const int oi = __shfl_xor(best_idx, off, 64);
            if (ov > best_val || (ov == best_val && oi < best_idx)) { best_val = ov; best_idx = oi; }
        }
        float *sv = s_tail;
        int *si = reinterpret_cast<int *>(s_tail) + 8;
        if (lane == 0) { sv[wave] = best_val; si[wave] = best_idx; }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < nwaves; w++)
                if (sv[w] > best_val || (sv[w] == best_val && si[w] < best_idx)) { best_val = sv[w]; best_idx = si[w]; }
            p.pmax_val[blockIdx.x] = best_val;
            p.pmax_idx[blockIdx.x] = best_idx;
            if (blockIdx.x == 0 && p.st_adv != nullptr && p.adv != 0) { p.st_adv->n_past += p.adv; p.st_adv->n_gen += p.adv; }
        }
    }
}

// ggml_vec_dot_f32 with GGML_SIMD on AVX2: the reduce of the 4 x 8 accumulators a[i mod 32] -- 0 += 2, 1 += 3, 0 += 1, low + high half, two hadds
__device__ __forceinline__ float simd_reduce32(float (&a)[32]) {
#pragma unroll
    for (int i = 0; i < 16; i++) a[i] = __fadd_rn(a[i], a[i + 16]);
#pragma unroll
    for (int i = 0; i < 8; i++) a[i] = __fadd_rn(a[i], a[i + 8]);
    const float t0 = __fadd_rn(a[0], a[4]), t1 = __fadd_rn(a[1], a[5]), t2 = __fadd_rn(a[2], a[6]), t3 = __fadd_rn(a[3], a[7]);
    return __fadd_rn(__fadd_rn(t0, t1), __fadd_rn(t2, t3));
}

// One workgroup of 256 threads per (head, query column); dk = 64, T <= SIMD_ATTN_MAXT.  bo_attn_head with assoc & 1:
//   S_j = simd dot(K_j, q) ; p_j = f16tab_exp(S_j - max) * (float)(1/sum_double) ; o_d = simd dot over j of (V_jd, p_j)
// Scores: a thread owns whole keys and the 32 accumulators of a key's dot.  PV: thread (slice, d) owns the accumulators j mod 32 = slice, slice + 4, ...
// of dimension d; the 32 partial sums of a dimension meet in LDS, one thread reduces them and adds the keys beyond T & ~31 in order.
__global__ __launch_bounds__(256) void attn_simd_kernel(const AttnParams p) {
    __shared__ __attribute__((aligned(16))) float s_q[64];
    __shared__ float s_p[SIMD_ATTN_MAXT];
    __shared__ float s_acc[32][64];
    __shared__ double s_red[16];
    const int h = blockIdx.x, i = blockIdx.y;
    const int T = min(visible_keys(p.st, i, p.N), SIMD_ATTN_MAXT);
    constexpr int dk = 64;
    const int D = p.D, tid = threadIdx.x;
    const float *__restrict__ kbase = p.kcache + (size_t)h * p.P * dk;   // head-major cache: [H][P][dk]
    const float *__restrict__ vbase = p.vcache + (size_t)h * p.P * dk;
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
            const float4 *kr = reinterpret_cast<const float4 *>(kbase + (size_t)j * dk);
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
        for (int j = r; j < Tfull; j += 32) acc = __fmaf_rn(vbase[(size_t)j * dk + d], s_p[j], acc);
        s_acc[r][d] = acc;
    }
    __syncthreads();
    if (tid < dk) {
        float a[32];
#pragma unroll
        for (int r = 0; r < 32; r++) a[r] = s_acc[r][tid];
        float o = simd_reduce32(a);
        for (int j = Tfull; j < T; j++) o = __fadd_rn(o, __fmul_rn(vbase[(size_t)j * dk + tid], s_p[j]));
        p.out[(size_t)i * D + (size_t)h * dk + tid] = o;
    }
}

}  // namespace bgk
