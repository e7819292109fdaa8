// The decode launches' LayerNorm + Q8 stage and their activation quantizer ALONE (biogpt_hip_ln_q8_device), and the exhaustive check of the short
// arithmetic forms they use (biogpt_hip_q8_forms_device): q8_round, ln_inv_std and q8_scales of kernels_decode.hip.h against the expressions they
// stand for, over all 2^32 float bit patterns.  Only engine.hip includes this file.
#pragma once

#include "kernels_decode.hip.h"

namespace bgk {

// One workgroup of 512 threads per row of 1024, as the pipelined launches call the stage (kernels_xpipe.hip.h, stage A): thread t < 256 holds elements
// 4t .. 4t+3 of the row and of the gain / bias; the 32 activation blocks are copied out of LDS as the stage left them.  wb_stride: floats between two
// rows' gain / bias (0: one gain / bias for every row).  s_out is written only where the stage writes block sums.
template <bool Q81, bool SUM>
__global__ __launch_bounds__(512) void ln_q8_probe_kernel(const float *x, const float *ln_w, const float *ln_b, int wb_stride, float eps, uint32_t *q_out,
                                                          float *d_out, uint32_t *s_out) {
    __shared__ __attribute__((aligned(16))) uint32_t s_xq[256];
    __shared__ float s_xd[32];
    __shared__ uint32_t s_xs[32];
    __shared__ double s_red[8];
    const int tid = threadIdx.x;
    const size_t row = blockIdx.x;
    float4 xv = make_float4(0.f, 0.f, 0.f, 0.f), lnw = xv, lnb = xv;
    if (tid < 256) {
        xv = reinterpret_cast<const float4 *>(x + row * 1024)[tid];
        lnw = reinterpret_cast<const float4 *>(ln_w + row * (size_t)wb_stride)[tid];
        lnb = reinterpret_cast<const float4 *>(ln_b + row * (size_t)wb_stride)[tid];
    }
    ln4_q8_1024<Q81, SUM>(xv, lnw, lnb, eps, s_red, s_xq, s_xd, s_xs);
    if (tid < 256) q_out[row * 256 + tid] = s_xq[tid];
    if (tid < 32) {
        d_out[row * 32 + tid] = s_xd[tid];
        if (Q81 || SUM) s_out[row * 32 + tid] = s_xs[tid];
    }
}

// q8_block32 alone: block b's 32 values one per lane of an aligned group of 32 lanes, two blocks per wave (every lane takes part; the last wave's
// second group repeats the last block and stores nothing)
__global__ __launch_bounds__(64) void q8_block32_probe_kernel(const float *x, int n_blocks, int q81, int want_sum, int8_t *q_out, float *d_out, uint32_t *s_out) {
    const int lane = threadIdx.x, blk = blockIdx.x * 2 + (lane >> 5);
    const int src = blk < n_blocks ? blk : n_blocks - 1;
    int8_t q;
    float d;
    uint32_t s;
    q8_block32(x[(size_t)src * 32 + (lane & 31)], q81 != 0, q, d, s, want_sum != 0);
    if (blk < n_blocks) {
        q_out[(size_t)blk * 32 + (lane & 31)] = q;
        if ((lane & 31) == 0) { d_out[blk] = d; s_out[blk] = s; }
    }
}

// ---- all 2^32 bit patterns --------------------------------------------------------------------------------------------------------------------------
// Check c of Q8F_CHECKS: out[c] patterns tested, out[Q8F_CHECKS + c] of them with a result that differs from the reference expression (two NaNs count
// as equal), out[2 * Q8F_CHECKS + c] the lowest such pattern (~0 when there is none; preset by the host).
//   0  ln_inv_std_short(v) against 1.0f / sqrtf(v), every v with ln_inv_std_in_range(v)
//   1  ln_inv_std(v) against the same, every pattern (a wave holds 64 consecutive patterns, so the waves on the range's borders take the general form)
//   2  q8_round(x) against (int)roundf(x), |x| <= 2^22
//   3  the same for every other pattern (NaN and infinities included: the conversion's own saturation, the same instruction on both sides)
//   4  q8_scales_short(a) against d = a / 127, id = d != 0 ? 1 / d : 0, every a with q8_scales_in_range(a)
//   5  q8_scales(a) against the same, every pattern
constexpr int Q8F_CHECKS = 6;
constexpr int Q8F_BLOCKS = 4096, Q8F_THREADS = 256;       // 2^20 threads, 2^12 patterns each: pattern = iteration * 2^20 + thread

__device__ __forceinline__ bool same_f32(float a, float b) { return __float_as_uint(a) == __float_as_uint(b) || (a != a && b != b); }

__global__ __launch_bounds__(Q8F_THREADS) void q8_forms_kernel(unsigned long long *out) {
    __shared__ unsigned long long s_acc[3 * Q8F_CHECKS];
    if (threadIdx.x < 3 * Q8F_CHECKS) s_acc[threadIdx.x] = threadIdx.x < 2 * Q8F_CHECKS ? 0ull : ~0ull;
    __syncthreads();
    const uint32_t t = blockIdx.x * Q8F_THREADS + threadIdx.x;
    uint32_t tested[Q8F_CHECKS], bad[Q8F_CHECKS], first[Q8F_CHECKS];
#pragma unroll
    for (int c = 0; c < Q8F_CHECKS; c++) { tested[c] = 0u; bad[c] = 0u; first[c] = 0xFFFFFFFFu; }
    auto note = [&](int c, bool ok, uint32_t bits) {
        tested[c]++;
        if (!ok) { bad[c]++; first[c] = min(first[c], bits); }
    };
    for (uint32_t it = 0; it < 4096u; it++) {
        const uint32_t bits = it * (uint32_t)(Q8F_BLOCKS * Q8F_THREADS) + t;
        const float v = __uint_as_float(bits);
        const float inv_ref = 1.0f / sqrtf(v);
        if (ln_inv_std_in_range(v)) note(0, same_f32(ln_inv_std_short(v), inv_ref), bits);
        note(1, same_f32(ln_inv_std(v), inv_ref), bits);
        const bool round_ok = q8_round(v) == (int)roundf(v);
        if (fabsf(v) <= 0x1p22f) note(2, round_ok, bits);
        else note(3, round_ok, bits);
        float d_ref, id_ref, d, id;
        q8_scales_general(v, d_ref, id_ref);
        if (q8_scales_in_range(v)) {
            q8_scales_short(v, d, id);
            note(4, same_f32(d, d_ref) && same_f32(id, id_ref), bits);
        }
        q8_scales(v, d, id);
        note(5, same_f32(d, d_ref) && same_f32(id, id_ref), bits);
    }
#pragma unroll
    for (int c = 0; c < Q8F_CHECKS; c++) {
        atomicAdd(&s_acc[c], (unsigned long long)tested[c]);
        if (bad[c]) { atomicAdd(&s_acc[Q8F_CHECKS + c], (unsigned long long)bad[c]); atomicMin(&s_acc[2 * Q8F_CHECKS + c], (unsigned long long)first[c]); }
    }
    __syncthreads();
    if (threadIdx.x < 2 * Q8F_CHECKS) { if (s_acc[threadIdx.x]) atomicAdd(&out[threadIdx.x], s_acc[threadIdx.x]); }
    else if (threadIdx.x < 3 * Q8F_CHECKS && s_acc[threadIdx.x] != ~0ull) atomicMin(&out[threadIdx.x], s_acc[threadIdx.x]);
}

}  // namespace bgk
