// The wide column layer: the many-column linear stage of the wide chain (kernels_mfma_wide.hip.h) for passes of 1 .. 16 column states -- the decode steps of
// generate_greedy_batch / generate_sample / generate_beam(_batch) / generate_queue on a BioGPT-Large file.
//
// matmul_wide_kernel gives a wave a 16 x 16 output tile and lets it walk all K / 32 blocks of its rows one after another: at N <= 16 an out_proj or fc2 of a
// Large file is 25 workgroups, each a serial chain of 50 .. 200 load -> MFMA -> term -> add rounds.  Here the K axis is what a workgroup splits:
//   * a workgroup = ONE 16-row tile x the pass's single 16-column tile, NW waves (4 or 8, by K at launch; bg_wcols_geometry);
//   * round r: wave w owns the R = 4 consecutive blocks r NW R + w R .. + 3.  Their operands are requested together -- the weight block and its row scales from
//     the row-tiled image, the activation block and its scale straight from the producer's Q8 rows ([N][K] int8: each (block, column) operand is read by exactly
//     one wave, once, so there is no LDS staging and none of matmul_wide_kernel's two barriers per phase) -- and the requests of round r + 1 are issued before
//     round r's are consumed.  Per block: v_mfma_i32_16x16x32_i8 on a zero accumulator, then mfma_block_term<WT> per output, the kernel's four per lane;
//   * f32 addition is not associative, so a wave may not pre-sum its slice.  The terms go to an LDS ring [2][NW R blocks][256 outputs] f32 (32 KB at NW 4, 64 KB
//     at NW 8); after ONE workgroup barrier per round thread t < 256 adds the round's terms of output t in block order onto its accumulator -- from 0.0f, the
//     association of matmul_wide_kernel, of the generic route and of the oracle -- while the waves already produce the next round into the other half.  The only
//     serial work left per output is one __fadd_rn per block; the loads, the MFMAs and the scale multiplies run NW-wide;
//   * at the end the 256 sums go through the ring's idle half back to the lanes of wave 0 in MFMA order (rows 4 g .. 4 g + 3 of column lane & 15) and wave 0
//     calls wide_epilogue<EPI>: the one copy of the four epilogues.  fc1 keeps writing f32 GELU rows; the chain's q8_rows_kernel behind it is unchanged.
// Edge cases by construction: a block index past the row (fewer blocks than NW R at K = 96; the partial last round of K = 1600 = 50 blocks) is clamped for the
// loads, and its terms are neither written nor added; the zero-padded last row tile (M = 77, 57717) is computed on zeros and its rows >= M never stored; idle
// columns re-read column N - 1 and store nothing.
#pragma once

#include "kernels_mfma_wide.hip.h"

namespace bgk {

constexpr int WCOLS_MAX_COLS = 16;      // the pass's single column tile
constexpr int WCOLS_R = 4;              // blocks of a wave per round
constexpr size_t wcols_smem_bytes(int nw) { return (size_t)2 * nw * WCOLS_R * 256 * 4; }

template <int WT, int EPI, int NW>
__global__ __launch_bounds__(64 * NW) void wcols_kernel(const MatvecParams p, const DevMatrix img) {
    using TI = TypeInfo<WT>;
    static_assert(TI::quant, "block-quantized weights");
    static_assert(NW == 4 || NW == 8, "four or eight waves");
    constexpr bool Q81 = TI::q81;
    constexpr int R = WCOLS_R, RB = NW * R;                  // blocks of a round
    constexpr int SWF = Q81 ? 32 : 16;                       // floats per (tile, block) of weight scales: d[16 rows] (then m[16 rows])
    extern __shared__ __attribute__((aligned(16))) unsigned char wcols_smem[];
    float *const ring = reinterpret_cast<float *>(wcols_smem);      // [2][RB][256]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, g = lane >> 4;
    const int K = p.W.K, BPR = K / QK;
    const int tile = blockIdx.x;                             // (grid = ceil(M / 16): every workgroup has a tile of the image)
    const int cc = min(li, p.N - 1);                         // idle columns re-read the last one
    const int rounds = (BPR + RB - 1) / RB;

    const uint8_t *const aq = img.qs + ((size_t)tile * BPR * 16 + li) * 32 + 8 * g;                     // block b of the tile is 512 bytes further
    const float *const wsc = reinterpret_cast<const float *>(img.sc) + (size_t)tile * BPR * SWF + 4 * g;     // rows 4g .. 4g+3; block b is SWF floats further
    const int8_t *const bq = p.aq_q + (size_t)cc * K + 8 * g;                                           // block b of the column is 32 bytes further
    const float *const bd = p.aq_d + (size_t)cc * BPR;
    const uint32_t *const bs = p.aq_s + (size_t)cc * BPR;
    const i32x4 zero = {0, 0, 0, 0};

    struct Ops { uint2 a[R]; float4 dw[R], mw[R]; long xb[R]; float xd[R], xs[R]; };
    auto load = [&](int r) {
        Ops o;
#pragma unroll
        for (int j = 0; j < R; j++) {
            const int b = min(r * RB + wave * R + j, BPR - 1);      // past the row: any block of the row, its terms are dropped
            o.a[j] = *reinterpret_cast<const uint2 *>(aq + (size_t)b * 512);
            o.dw[j] = *reinterpret_cast<const float4 *>(wsc + (size_t)b * SWF);
            o.mw[j] = Q81 ? *reinterpret_cast<const float4 *>(wsc + (size_t)b * SWF + 16) : make_float4(0.f, 0.f, 0.f, 0.f);
            o.xb[j] = *reinterpret_cast<const long *>(bq + (size_t)b * QK);
            o.xd[j] = bd[b];
            o.xs[j] = Q81 ? __uint_as_float(bs[b]) : 0.0f;
        }
        return o;
    };

    float acc = 0.0f;                                        // thread t < 256: output t = 4 * lane' + row of the tile's MFMA order
    Ops cur = load(0);
    for (int r = 0; r < rounds; r++) {
        Ops nxt = cur;
        if (r + 1 < rounds) nxt = load(r + 1);               // in flight while this round is consumed
        float *const half = ring + (size_t)(r & 1) * RB * 256;
        i32x4 d[R];
#pragma unroll
        for (int j = 0; j < R; j++) d[j] = __builtin_amdgcn_mfma_i32_16x16x32_i8((long)(((unsigned long)cur.a[j].y << 32) | cur.a[j].x), cur.xb[j], zero, 0, 0, 0);
#pragma unroll
        for (int j = 0; j < R; j++) {
            if (r * RB + wave * R + j >= BPR) continue;      // (a whole wave)
            float4 t;
            t.x = mfma_block_term<WT>((float)d[j][0], cur.dw[j].x, cur.mw[j].x, cur.xd[j], cur.xs[j]);
            t.y = mfma_block_term<WT>((float)d[j][1], cur.dw[j].y, cur.mw[j].y, cur.xd[j], cur.xs[j]);
            t.z = mfma_block_term<WT>((float)d[j][2], cur.dw[j].z, cur.mw[j].z, cur.xd[j], cur.xs[j]);
            t.w = mfma_block_term<WT>((float)d[j][3], cur.dw[j].w, cur.mw[j].w, cur.xd[j], cur.xs[j]);
            reinterpret_cast<float4 *>(half + (size_t)(wave * R + j) * 256)[lane] = t;
        }
        __syncthreads();                                     // the round's terms are in; the half of round r - 1 is free again behind this barrier
        if (tid < 256) {
            const int nb = min(RB, BPR - r * RB);
            for (int s = 0; s < nb; s++) acc = __fadd_rn(acc, half[s * 256 + tid]);      // block order
        }
        cur = nxt;
    }
    // the sums back to MFMA order through the half no round reads or writes any more (the last fold read the other one)
    float *const fin = ring + (size_t)(rounds & 1) * RB * 256;
    if (tid < 256) fin[tid] = acc;
    __syncthreads();
    if (wave != 0 || li >= p.N) return;
    const float4 v = reinterpret_cast<const float4 *>(fin)[lane];
    const float sums[4] = {v.x, v.y, v.z, v.w};
    wide_epilogue<EPI>(p, sums, li, tile * 16 + 4 * g);
}

}  // namespace bgk
