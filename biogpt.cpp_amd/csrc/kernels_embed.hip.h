// Hidden states, pooled embeddings and classification heads (biogpt_hip_hidden / biogpt_hip_embed_batch): the final stage of a causal
// pass that stops in front of the lm_head.  No reference counterpart (biogpt.cpp returns logits only).
//
//   ln_rows_kernel      the final LayerNorm of N activation columns as f32 rows [N][K].  One workgroup per column; the arithmetic of
//                       lnq_kernel / matvec_fast_kernel<PRO_LN> up to the point where those quantize: mean and variance from double sums
//                       over the f32 row, each rounded to f32, 1.0f / sqrtf(var + eps), then sub, mul, mul, add in f32, un-fused.
//                       K = 1024: the row in registers, every wave sums it (no exchange), one 16-byte store per lane;
//                       K = 0: any width that is a multiple of 4, taken from the argument (the row is read twice, the second time from L1 / L2).
//   pool_rows_kernel    pooling over the columns of ONE pass.  A column's sequence and position are its SeqState (seq_id, n_past), the
//                       sequence's length lens[seq_id].  LAST: the column at position len - 1 copies its row.  MEAN: the first column of a
//                       sequence in the pass owns that sequence's accumulator row [W] of doubles for this launch and adds the rows of the
//                       columns that follow it (a sequence's columns are consecutive); passes are ordered by the stream: no atomics.
//   pool_finish_kernel  one workgroup per output row: (float)(sum / len) of a MEAN accumulator, and the optional L2 normalisation
//                       (sum of squares in double, (float)(x / sqrt(ss)), a zero row stays zero).
//   head_rows_kernel    out[r][o] = (float)(b[o] + sum_d (double)w[o][d] * (double)x[r][d]): every f32 x f32 product is exact in double,
//                       the sum is rounded once.  8 rows per workgroup in LDS, a wave per output, every w row read once per workgroup.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.hip.h"

namespace bgk {

enum PoolMode : int { POOL_NONE = 0, POOL_LAST = 1, POOL_MEAN = 2 };

// x: [N][ldx] floats (N = gridDim.x), out: [N][k] floats; inv_k = 1.0 / k.  cols != null: column i's row is row (cols[i].seq_id / slot_div) * P + cols[i].n_past
// of out (the context store of contrastive search: one run of P rows per group of slot_div cache slots)
template <int K>
__global__ __launch_bounds__(256) void ln_rows_kernel(const float *x, int ldx, int k, const float *ln_w, const float *ln_b, float eps, double inv_k,
                                                      float *out, const SeqState *cols, int slot_div, int P) {
    const int col = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t orow = cols ? (size_t)(cols[col].seq_id / slot_div) * P + cols[col].n_past : (size_t)col;
    const float4 *xcol = reinterpret_cast<const float4 *>(x + (size_t)col * ldx);
    if constexpr (K == 1024) {
        constexpr int NJJ = K / 4 / 64, NSHARE = NJJ / 4;
        float4 xr[NJJ], xs4[NSHARE], lw4[NSHARE], lb4[NSHARE];
#pragma unroll
        for (int i = 0; i < NJJ; i++) xr[i] = xcol[i * 64 + lane];
#pragma unroll
        for (int i = 0; i < NSHARE; i++) {
            const int ch = (wave + 4 * i) * 64 + lane;
            xs4[i] = xcol[ch];
            lw4[i] = reinterpret_cast<const float4 *>(ln_w)[ch];
            lb4[i] = reinterpret_cast<const float4 *>(ln_b)[ch];
        }
        double s1 = 0.0;
#pragma unroll
        for (int i = 0; i < NJJ; i++) s1 += ((double)xr[i].x + (double)xr[i].y) + ((double)xr[i].z + (double)xr[i].w);
        s1 = wave_sum_f64(s1);
        const float mean = (float)(s1 * inv_k);
        double s2 = 0.0;
#pragma unroll
        for (int i = 0; i < NJJ; i++) {
            const float a = __fsub_rn(xr[i].x, mean), b = __fsub_rn(xr[i].y, mean);
            const float c = __fsub_rn(xr[i].z, mean), d = __fsub_rn(xr[i].w, mean);
            s2 += ((double)__fmul_rn(a, a) + (double)__fmul_rn(b, b)) + ((double)__fmul_rn(c, c) + (double)__fmul_rn(d, d));
        }
        s2 = wave_sum_f64(s2);
        const float var = (float)(s2 * inv_k);
        const float scale = 1.0f / sqrtf(__fadd_rn(var, eps));
#pragma unroll
        for (int i = 0; i < NSHARE; i++) {
            const int ch = (wave + 4 * i) * 64 + lane;
            float4 v = xs4[i];
            v.x = __fadd_rn(__fmul_rn(lw4[i].x, __fmul_rn(__fsub_rn(v.x, mean), scale)), lb4[i].x);
            v.y = __fadd_rn(__fmul_rn(lw4[i].y, __fmul_rn(__fsub_rn(v.y, mean), scale)), lb4[i].y);
            v.z = __fadd_rn(__fmul_rn(lw4[i].z, __fmul_rn(__fsub_rn(v.z, mean), scale)), lb4[i].z);
            v.w = __fadd_rn(__fmul_rn(lw4[i].w, __fmul_rn(__fsub_rn(v.w, mean), scale)), lb4[i].w);
            reinterpret_cast<float4 *>(out + orow * K)[ch] = v;
        }
    } else {
        const int nch = k >> 2;
        double s1 = 0.0;
        for (int ch = lane; ch < nch; ch += 64) {      // every wave: the whole row
            const float4 v = xcol[ch];
            s1 += ((double)v.x + (double)v.y) + ((double)v.z + (double)v.w);
        }
        s1 = wave_sum_f64(s1);
        const float mean = (float)(s1 / (double)k);
        double s2 = 0.0;
        for (int ch = lane; ch < nch; ch += 64) {
            const float4 v = xcol[ch];
            const float a = __fsub_rn(v.x, mean), b = __fsub_rn(v.y, mean), c = __fsub_rn(v.z, mean), d = __fsub_rn(v.w, mean);
            s2 += ((double)__fmul_rn(a, a) + (double)__fmul_rn(b, b)) + ((double)__fmul_rn(c, c) + (double)__fmul_rn(d, d));
        }
        s2 = wave_sum_f64(s2);
        const float var = (float)(s2 / (double)k);
        const float scale = 1.0f / sqrtf(__fadd_rn(var, eps));
        for (int ch = threadIdx.x; ch < nch; ch += 256) {
            float4 v = xcol[ch];
            const float4 w = reinterpret_cast<const float4 *>(ln_w)[ch], b = reinterpret_cast<const float4 *>(ln_b)[ch];
            v.x = __fadd_rn(__fmul_rn(w.x, __fmul_rn(__fsub_rn(v.x, mean), scale)), b.x);
            v.y = __fadd_rn(__fmul_rn(w.y, __fmul_rn(__fsub_rn(v.y, mean), scale)), b.y);
            v.z = __fadd_rn(__fmul_rn(w.z, __fmul_rn(__fsub_rn(v.z, mean), scale)), b.z);
            v.w = __fadd_rn(__fmul_rn(w.w, __fmul_rn(__fsub_rn(v.w, mean), scale)), b.w);
            reinterpret_cast<float4 *>(out + orow * k)[ch] = v;
        }
    }
}

// One pass's columns.  rows: [n_cols][W] floats; cols: [n_cols] column states; lens: [n_seqs].  Grid (ceil(W / 64), n_cols), 256 threads:
// a workgroup covers 64 consecutive elements (16 lanes x 16 bytes) of one column's sequence, its 16 lane groups take every 16th row.
//   POOL_LAST   out: [n_seqs][W] floats
//   POOL_MEAN   acc: [n_seqs][W] doubles, zeroed at the start of the call
constexpr int POOL_GROUPS = 16;
__global__ __launch_bounds__(256) void pool_rows_kernel(const float *rows, int n_cols, int W, const SeqState *cols, const int32_t *lens, int mode,
                                                        float *out, double *acc) {
    __shared__ double s_part[POOL_GROUPS][64];
    const int col = blockIdx.y, grp = threadIdx.x >> 4, d = blockIdx.x * 64 + (threadIdx.x & 15) * 4;
    const int seq = cols[col].seq_id;
    if (mode == POOL_LAST) {
        if (cols[col].n_past != lens[seq] - 1 || grp != 0 || d >= W) return;
        *reinterpret_cast<float4 *>(out + (size_t)seq * W + d) = *reinterpret_cast<const float4 *>(rows + (size_t)col * W + d);
        return;
    }
    if (col > 0 && cols[col - 1].seq_id == seq) return;      // (workgroup-uniform) not the first column of its sequence in this pass
    const int end = min(n_cols, col + (lens[seq] - cols[col].n_past));      // the rest of the sequence follows it, as far as the pass goes
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    if (d < W)
        for (int r = col + grp; r < end; r += POOL_GROUPS) {
            const float4 v = *reinterpret_cast<const float4 *>(rows + (size_t)r * W + d);
            s0 += (double)v.x; s1 += (double)v.y; s2 += (double)v.z; s3 += (double)v.w;
        }
    const int e = (threadIdx.x & 15) * 4;
    s_part[grp][e] = s0; s_part[grp][e + 1] = s1; s_part[grp][e + 2] = s2; s_part[grp][e + 3] = s3;
    __syncthreads();
    if (threadIdx.x < 64 && blockIdx.x * 64 + threadIdx.x < W) {      // one owner per accumulator element
        double t = 0.0;
#pragma unroll
        for (int g = 0; g < POOL_GROUPS; g++) t += s_part[g][threadIdx.x];
        acc[(size_t)seq * W + blockIdx.x * 64 + threadIdx.x] += t;
    }
}

// One workgroup per output row r (gridDim.x rows of W floats in `out`).  acc != null: out[r] = (float)(acc[r] / lens[r]) first.
// normalize: out[r] = (float)(out[r] / sqrt(sum of squares)), unless the row is all zeros.
__global__ __launch_bounds__(256) void pool_finish_kernel(float *out, int W, const double *acc, const int32_t *lens, int normalize) {
    __shared__ double s_red[4];
    const int r = blockIdx.x;
    float *row = out + (size_t)r * W;
    double ss = 0.0;
    const double len = acc ? (double)lens[r] : 1.0;
    for (int d = threadIdx.x; d < W; d += 256) {
        float v;
        if (acc) { v = (float)(acc[(size_t)r * W + d] / len); row[d] = v; }
        else v = row[d];
        ss += (double)v * (double)v;
    }
    if (!normalize) return;
    ss = block_sum_f64(ss, s_red);
    if (ss == 0.0) return;
    const double nrm = sqrt(ss);
    for (int d = threadIdx.x; d < W; d += 256) row[d] = (float)((double)row[d] / nrm);      // (each thread re-reads what it wrote itself)
}

// x: [n_rows][W] floats, w: [n_out][W], b: [n_out] or null, out: [n_rows][n_out].  Grid ceil(n_rows / 8), 256 threads, 8 * W * 4 bytes of dynamic LDS.
constexpr int HEAD_ROWS = 8;
__global__ __launch_bounds__(256) void head_rows_kernel(const float *x, int n_rows, int W, const float *w, const float *b, int n_out, float *out) {
    extern __shared__ float4 s_x4[];      // [HEAD_ROWS][W / 4]
    const int r0 = blockIdx.x * HEAD_ROWS, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nch = W >> 2;
    for (int i = threadIdx.x; i < HEAD_ROWS * nch; i += 256) {
        const int r = r0 + i / nch;
        s_x4[i] = r < n_rows ? reinterpret_cast<const float4 *>(x + (size_t)r * W)[i % nch] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __syncthreads();
    for (int o = wave; o < n_out; o += 4) {
        const float4 *wrow = reinterpret_cast<const float4 *>(w + (size_t)o * W);
        double a[HEAD_ROWS];
#pragma unroll
        for (int r = 0; r < HEAD_ROWS; r++) a[r] = 0.0;
        for (int ch = lane; ch < nch; ch += 64) {
            const float4 wv = wrow[ch];
#pragma unroll
            for (int r = 0; r < HEAD_ROWS; r++) {
                const float4 xv = s_x4[r * nch + ch];
                a[r] = __builtin_fma((double)wv.x, (double)xv.x, a[r]);      // (the product is exact: fused or not, one rounding, that of the sum)
                a[r] = __builtin_fma((double)wv.y, (double)xv.y, a[r]);
                a[r] = __builtin_fma((double)wv.z, (double)xv.z, a[r]);
                a[r] = __builtin_fma((double)wv.w, (double)xv.w, a[r]);
            }
        }
        const double bo = b ? (double)b[o] : 0.0;
#pragma unroll
        for (int r = 0; r < HEAD_ROWS; r++) {
            const double t = wave_sum_f64(a[r]);
            if (lane == 0 && r0 + r < n_rows) out[(size_t)(r0 + r) * n_out + o] = (float)(bo + t);
        }
    }
}

}  // namespace bgk
