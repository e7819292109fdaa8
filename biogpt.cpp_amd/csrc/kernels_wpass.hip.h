// The wide pass layer's linear stage: passes of 9 or more of the context's own columns of a block-quantized file that is NOT BioGPT-base (BioGPT-Large's
// d_model 1600 / d_ff 6400 / n_vocab 57717, or any d_model % 64 == 0, d_ff % 32 == 0 with head size 64), on v_mfma_i32_16x16x32_i8.
//
// The arithmetic is kernels_mfma.hip.h's -- per block b of a row one integer dot on the matrix core from the row-tiled expanded image, then
// mfma_block_term<WT>, the f32 sum in block order inside one lane -- so the stage is bit-identical to matvec_kernel, matmul_wide_kernel and the oracle.
// The frame is this file's own:
//   * REGISTER BLOCKING.  A wave owns a UNIT of RT row tiles (RT = 2 at the fc1 site: 32 rows = one Q8 block of fc2's activation; 1 elsewhere) against CT
//     16-column tiles (CT = 2 wherever the pass has more than 16 columns).  One A operand (8 int8 per lane) and one quad of row scales feed CT MFMAs, one B
//     operand feeds RT: image bytes and scale loads per MFMA halve against a wave per 16 x 16 tile.  The A operands and row scales of the next four blocks are
//     requested from global memory before the four blocks in hand are multiplied.
//   * STAGING OVERLAPPED WITH COMPUTE, ONE BARRIER PER PHASE.  The 16 CT columns of a workgroup are staged in phases of 32 blocks (1024 elements of K); the last
//     phase may be partial (1600 = 32 + 18 blocks, 6400 = 6 x 32 + 8, 192 = 6, 160 = 5).  A register double buffer: every thread requests its share of phase
//     ph + 1 (Q8 codes, scales, Q8_1 sums) BEFORE the MFMAs of phase ph and writes it into the OTHER LDS buffer behind them; the barrier that follows is the
//     only one of the phase (the buffer written was last read in phase ph - 1, which every wave left before the barrier in between).
//   * RUN-TIME K, M, N.  K % 32 == 0; the image holds ceil(M / 16) tiles, the last one zero-padded: rows >= M are computed and never stored (the logits site;
//     16 | M at the layer sites, 32 | M at fc1).  Idle columns of the last tile re-read column N - 1 and store nothing.
//   * GEOMETRY FROM N (wpass_tu.hip): CT from N, and WPB = 1 or 4 waves per workgroup from the number of wave units against the device's compute units.
// LDS per workgroup: wpass_smem_bytes() = (1 or 2 buffers) x 16 CT columns x (1040 bytes of codes + 132 of scales (+ 132 of Q8_1 sums)):
//   CT = 1: 18.3 / 20.4 KB for rows of one phase, 36.6 / 40.8 KB beyond; CT = 2: 36.6 / 40.8 KB and 73.3 / 81.5 KB (Q8_0-side / Q8_1-side formats).
// Operand layouts (kernels_mfma.hip.h): A = 8 int8 of row (lane & 15), elements 8 g .. 8 g + 7 of the block (g = lane >> 4); B = the same elements of
// column (lane & 15); C/D = rows 4 g .. 4 g + 3 of column (lane & 15).
#pragma once

#include "kernels_mfma.hip.h"

namespace bgk {

constexpr int WPASS_MIN_COLS = 9;
constexpr int WPASS_BPP = 32;                                // blocks of a staged phase
constexpr int WPASS_PITCH = WPASS_BPP * QK + 16;             // bytes per staged column of codes: the 8-byte operand reads of a 32-lane half cover all 64 banks
constexpr int WPASS_SP = WPASS_BPP + 1;                      // floats per staged column of block scales: lanes 0 .. 15 read 16 different banks

using wpass_u4 = __attribute__((ext_vector_type(4))) unsigned int;      // a staged 16-byte piece (a plain vector: an array of them stays in registers)

struct WpassParams {
    const uint8_t *img_q;        // the matrix' row-tiled image: expanded blocks, then the f32 row scales (tile_image_place)
    const uint8_t *img_s;
    int32_t M, K, N;
    const int8_t *aq_q; const float *aq_d; const uint32_t *aq_s;      // the columns' Q8 blocks: [N][K], [N][K / 32]
    const float *bias;           // [M] (not at the logits site)
    const float *resid;          // EPI_RESID: [N][ldr]
    int32_t ldr;
    float *out;                  // EPI_RESID / EPI_LOGITS: [N][ldo]
    int32_t ldo;
    float *q_out;                // EPI_QKV: [N][D], and the layer's head-major cache slices [D / 64][P][64]
    float *kcache, *vcache;
    int32_t P, D;
    float q_scale;
    const DevState *st;          // column c is position st->n_past + c
    const uint16_t *gelu_tab;    // EPI_GELU_Q8
    int8_t *oq_q; float *oq_d; uint32_t *oq_s;      // EPI_GELU_Q8: fc2's Q8 blocks [N][M], [N][M / 32]
};

__host__ __device__ inline size_t wpass_col_bytes(bool q81) { return (size_t)WPASS_PITCH + (size_t)WPASS_SP * 4 * (q81 ? 2 : 1); }
__host__ __device__ inline size_t wpass_smem_bytes(bool q81, int ct, int K) { return (size_t)(K / QK > WPASS_BPP ? 2 : 1) * 16 * ct * wpass_col_bytes(q81); }

// EPI: EPI_QKV, EPI_RESID, EPI_GELU_Q8 (fc1: GELU table, then fc2's Q8 blocks in the wave), EPI_LOGITS.  grid (ceil(units / WPB), ceil(N / (16 CT))), 64 WPB threads.
template <int WT, int EPI, int CT, int WPB>
__global__ __launch_bounds__(64 * WPB) void wpass_kernel(const WpassParams p) {
    using TI = TypeInfo<WT>;
    static_assert(TI::quant, "block-quantized weights");
    static_assert(EPI == EPI_QKV || EPI == EPI_RESID || EPI == EPI_GELU_Q8 || EPI == EPI_LOGITS, "the wide pass layer's four sites");
    static_assert((CT == 1 || CT == 2) && (WPB == 1 || WPB == 4), "one or two column tiles per wave, one or four waves per workgroup");
    constexpr bool Q81 = TI::q81;
    constexpr int RT = EPI == EPI_GELU_Q8 ? 2 : 1;           // row tiles of a wave's unit
    constexpr int NC = 16 * CT, T = 64 * WPB;
    constexpr int SWF = Q81 ? 32 : 16;                       // floats per (tile, block) of row scales: d[16 rows] (then m[16 rows])
    constexpr int QP = NC * (WPASS_BPP * QK / 16) / T;       // 16-byte pieces of codes a thread stages per phase
    constexpr int DP = NC * WPASS_BPP / T;                   // block scales (and sums) a thread stages per phase
    constexpr int NB = (RT == 2 && CT == 2 && WPB == 1) ? 2 : 4;      // blocks of a step (four units' operands beside a lone wave's 160 staging registers: two, or the Q8_1-side formats spill)
    constexpr int COLB = WPASS_PITCH + WPASS_SP * 4 * (Q81 ? 2 : 1), BUFB = NC * COLB;
    constexpr int OFF_D = NC * WPASS_PITCH, OFF_S = OFF_D + NC * WPASS_SP * 4;
    extern __shared__ __attribute__((aligned(16))) unsigned char wpass_smem[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, g = lane >> 4;
    const int K = p.K, M = p.M, BPR = K / QK;
    const int ntile = (M + 15) >> 4, nunit = (ntile + RT - 1) / RT;
    const int col0 = blockIdx.y * NC;
    const int unit = blockIdx.x * WPB + wave;
    const bool unit_ok = unit < nunit;                       // waves past the last unit stage their share and keep the barriers company
    const int tile0 = (unit_ok ? unit : nunit - 1) * RT;     // (RT = 2: 32 | M, both tiles exist)

    const uint8_t *const aq = p.img_q + ((size_t)tile0 * BPR * 16 + li) * 32 + 8 * g;                  // block b is 512 bytes further, the unit's second tile BPR blocks
    const float *const wsc = reinterpret_cast<const float *>(p.img_s) + (size_t)tile0 * BPR * SWF + 4 * g;   // rows 4g .. 4g+3; block b is SWF floats further

    // ---- staging: this thread's share of a phase, global -> registers -> LDS (the lambdas are inlined by force: called twice, left as functions they put the register sets on the stack) ----
    wpass_u4 sq[QP]; float sd[DP]; uint32_t ss[Q81 ? DP : 1];
    auto stage_load = [&](int ph) __attribute__((always_inline)) {
        const int nb = min(WPASS_BPP, BPR - ph * WPASS_BPP), per = nb * 2;      // blocks of the phase; 16-byte pieces per column
#pragma unroll
        for (int i = 0; i < QP; i++) {
            const int idx = i * T + tid, c = idx >> 6, o = idx & 63;
            const int cc = min(col0 + c, p.N - 1);           // idle columns re-read the last one
            if (o < per) sq[i] = *reinterpret_cast<const wpass_u4 *>(p.aq_q + (size_t)cc * K + (size_t)ph * (WPASS_BPP * QK) + (size_t)o * 16);
        }
#pragma unroll
        for (int i = 0; i < DP; i++) {
            const int idx = i * T + tid, c = idx >> 5, b = idx & 31;
            const int cc = min(col0 + c, p.N - 1);
            if (b < nb) {
                sd[i] = p.aq_d[(size_t)cc * BPR + ph * WPASS_BPP + b];
                if (Q81) ss[i] = p.aq_s[(size_t)cc * BPR + ph * WPASS_BPP + b];
            }
        }
    };
    auto stage_store = [&](int ph) __attribute__((always_inline)) {
        unsigned char *const buf = wpass_smem + (ph & 1) * BUFB;
        const int nb = min(WPASS_BPP, BPR - ph * WPASS_BPP), per = nb * 2;
#pragma unroll
        for (int i = 0; i < QP; i++) {
            const int idx = i * T + tid, c = idx >> 6, o = idx & 63;
            if (o < per) *reinterpret_cast<wpass_u4 *>(buf + c * WPASS_PITCH + o * 16) = sq[i];
        }
#pragma unroll
        for (int i = 0; i < DP; i++) {
            const int idx = i * T + tid, c = idx >> 5, b = idx & 31;
            if (b < nb) {
                reinterpret_cast<float *>(buf + OFF_D)[c * WPASS_SP + b] = sd[i];
                if (Q81) reinterpret_cast<uint32_t *>(buf + OFF_S)[c * WPASS_SP + b] = ss[i];
            }
        }
    };

    // ---- A operands and row scales of a step of NB blocks (blocks past the row's end re-read the last one; their terms are not added) ----
    struct StepA { uint2 a[RT][NB]; float4 dw[RT][NB]; float4 mw[RT][NB]; };
    auto load_a = [&](int gb, StepA &s) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < NB; j++) {
            const size_t b = (size_t)min(gb + j, BPR - 1);
#pragma unroll
            for (int rt = 0; rt < RT; rt++) {
                const size_t bb = (size_t)rt * BPR + b;
                s.a[rt][j] = *reinterpret_cast<const uint2 *>(aq + bb * 512);
                s.dw[rt][j] = *reinterpret_cast<const float4 *>(wsc + bb * SWF);
                s.mw[rt][j] = Q81 ? *reinterpret_cast<const float4 *>(wsc + bb * SWF + 16) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
    };

    const i32x4 zero = {0, 0, 0, 0};
    float acc[RT][CT][4];
#pragma unroll
    for (int rt = 0; rt < RT; rt++)
#pragma unroll
        for (int ct = 0; ct < CT; ct++)
#pragma unroll
            for (int r = 0; r < 4; r++) acc[rt][ct][r] = 0.0f;

    StepA cur, nxt;
    stage_load(0);
    load_a(0, cur);
    stage_store(0);
    __syncthreads();

    const int nph = (BPR + WPASS_BPP - 1) / WPASS_BPP;
#pragma unroll 1
    for (int ph = 0; ph < nph; ph++) {
        const int b0 = ph * WPASS_BPP, nb = min(WPASS_BPP, BPR - b0);
        const bool more = ph + 1 < nph;
        if (more) stage_load(ph + 1);                        // on its way while this phase is multiplied
        const unsigned char *const buf = wpass_smem + (ph & 1) * BUFB;
        const unsigned char *const bq = buf + li * WPASS_PITCH + 8 * g;
        const float *const s_d = reinterpret_cast<const float *>(buf + OFF_D) + li * WPASS_SP;
        const float *const s_s = reinterpret_cast<const float *>(buf + OFF_S) + li * WPASS_SP;
        auto step = [&](int b, const StepA &use, StepA &fill) __attribute__((always_inline)) {
            load_a(b0 + b + NB, fill);                       // the next step's operands (clamped at the row's end), requested before this step's MFMAs
            long xb[CT][NB]; float xd[CT][NB], xs[CT][NB];
#pragma unroll
            for (int ct = 0; ct < CT; ct++)
#pragma unroll
                for (int j = 0; j < NB; j++) {
                    const int bj = min(b + j, nb - 1);
                    xb[ct][j] = *reinterpret_cast<const long *>(bq + ct * 16 * WPASS_PITCH + bj * QK);
                    xd[ct][j] = s_d[ct * 16 * WPASS_SP + bj];
                    xs[ct][j] = Q81 ? s_s[ct * 16 * WPASS_SP + bj] : 0.0f;
                }
            i32x4 d[RT][CT][NB];
#pragma unroll
            for (int j = 0; j < NB; j++)
#pragma unroll
                for (int rt = 0; rt < RT; rt++)
#pragma unroll
                    for (int ct = 0; ct < CT; ct++)
                        d[rt][ct][j] = __builtin_amdgcn_mfma_i32_16x16x32_i8((long)(((unsigned long)use.a[rt][j].y << 32) | use.a[rt][j].x), xb[ct][j], zero, 0, 0, 0);
#pragma unroll
            for (int j = 0; j < NB; j++) {
                if (b + j < nb) {                            // (uniform) the sums stay in block order
#pragma unroll
                    for (int rt = 0; rt < RT; rt++)
#pragma unroll
                        for (int ct = 0; ct < CT; ct++) {
                            const float4 dw = use.dw[rt][j], mw = use.mw[rt][j];
                            acc[rt][ct][0] = __fadd_rn(acc[rt][ct][0], mfma_block_term<WT>((float)d[rt][ct][j][0], dw.x, mw.x, xd[ct][j], xs[ct][j]));
                            acc[rt][ct][1] = __fadd_rn(acc[rt][ct][1], mfma_block_term<WT>((float)d[rt][ct][j][1], dw.y, mw.y, xd[ct][j], xs[ct][j]));
                            acc[rt][ct][2] = __fadd_rn(acc[rt][ct][2], mfma_block_term<WT>((float)d[rt][ct][j][2], dw.z, mw.z, xd[ct][j], xs[ct][j]));
                            acc[rt][ct][3] = __fadd_rn(acc[rt][ct][3], mfma_block_term<WT>((float)d[rt][ct][j][3], dw.w, mw.w, xd[ct][j], xs[ct][j]));
                        }
                }
            }
        };
#pragma unroll 1
        for (int b = 0; b < nb; b += 2 * NB) {               // two steps per turn: the operands alternate between two register sets, no copies
            step(b, cur, nxt);
            if (b + NB < nb) step(b + NB, nxt, cur);
            else cur = nxt;                                  // (an odd number of steps: once per phase)
        }
        if (more) {
            stage_store(ph + 1);
            __syncthreads();                                 // the phase's one barrier: phase ph + 1 is whole, every wave has left phase ph
        }
    }
    if (!unit_ok) return;

#pragma unroll
    for (int ct = 0; ct < CT; ct++) {
        const int col = col0 + 16 * ct + li;
        if (col >= p.N) continue;
        if (EPI == EPI_GELU_Q8) {
            // the unit's 32 rows are ONE Q8 block of fc2's activation column: element 16 rt + 4 g + r lives in lane group g -- quantize_row_q8_0 / _q8_1 with
            // wide_q8_chunk's d / id / roundf, amax and the integer sum over the lane's eight values and the four lane groups
            float v[2][4];
#pragma unroll
            for (int rt = 0; rt < RT; rt++) {
                const float4 eb = *reinterpret_cast<const float4 *>(p.bias + unit * 32 + 16 * rt + 4 * g);
                v[rt][0] = h2f(p.gelu_tab[f2h(__fadd_rn(eb.x, acc[rt][ct][0]))]); v[rt][1] = h2f(p.gelu_tab[f2h(__fadd_rn(eb.y, acc[rt][ct][1]))]);
                v[rt][2] = h2f(p.gelu_tab[f2h(__fadd_rn(eb.z, acc[rt][ct][2]))]); v[rt][3] = h2f(p.gelu_tab[f2h(__fadd_rn(eb.w, acc[rt][ct][3]))]);
            }
            float amax = fmaxf(fmaxf(fmaxf(fabsf(v[0][0]), fabsf(v[0][1])), fmaxf(fabsf(v[0][2]), fabsf(v[0][3]))),
                               fmaxf(fmaxf(fabsf(v[RT - 1][0]), fabsf(v[RT - 1][1])), fmaxf(fabsf(v[RT - 1][2]), fabsf(v[RT - 1][3]))));
            amax = fmaxf(amax, __shfl_xor(amax, 16, 64)); amax = fmaxf(amax, __shfl_xor(amax, 32, 64));
            const float d = amax / 127.0f;
            const float id = (d != 0.0f) ? 1.0f / d : 0.0f;
            int q[2][4], isum = 0;
#pragma unroll
            for (int rt = 0; rt < RT; rt++)
#pragma unroll
                for (int r = 0; r < 4; r++) { q[rt][r] = (int)roundf(__fmul_rn(v[rt][r], id)); isum += q[rt][r]; }
            isum += __shfl_xor(isum, 16, 64); isum += __shfl_xor(isum, 32, 64);
            const size_t blk = (size_t)col * (M / 32) + unit;      // [N][M / 32]
#pragma unroll
            for (int rt = 0; rt < RT; rt++)
                *reinterpret_cast<uint32_t *>(p.oq_q + blk * 32 + 16 * rt + 4 * g) =
                    (uint32_t)(q[rt][0] & 0xFF) | ((uint32_t)(q[rt][1] & 0xFF) << 8) | ((uint32_t)(q[rt][2] & 0xFF) << 16) | ((uint32_t)(q[rt][3] & 0xFF) << 24);
            if (g == 0) {
                if (Q81) { p.oq_d[blk] = d; p.oq_s[blk] = __float_as_uint(__fmul_rn((float)isum, d)); }
                else { p.oq_d[blk] = h2f(f2h(d)); p.oq_s[blk] = (uint32_t)isum; }
            }
            continue;
        }
        const int orow = unit * 16 + 4 * g;                  // this lane's outputs: rows orow .. orow + 3 of column col
        const float *const a4 = acc[0][ct];
        if (EPI == EPI_LOGITS) {                             // n_vocab need not be a multiple of 4: row by row, rows >= M are never stored
#pragma unroll
            for (int r = 0; r < 4; r++)
                if (orow + r < M) p.out[(size_t)col * p.ldo + orow + r] = a4[r];
            continue;
        }
        const float4 eb = *reinterpret_cast<const float4 *>(p.bias + orow);      // (16 | M at the layer sites)
        float4 v;
        if (EPI == EPI_QKV) {
            v.x = __fadd_rn(eb.x, a4[0]); v.y = __fadd_rn(eb.y, a4[1]); v.z = __fadd_rn(eb.z, a4[2]); v.w = __fadd_rn(eb.w, a4[3]);
            const int which = orow / K, rr = orow - which * K;      // d_model == K for the q/k/v projection
            if (which == 0) {
                v.x = __fmul_rn(v.x, p.q_scale); v.y = __fmul_rn(v.y, p.q_scale); v.z = __fmul_rn(v.z, p.q_scale); v.w = __fmul_rn(v.w, p.q_scale);
                *reinterpret_cast<float4 *>(p.q_out + (size_t)col * K + rr) = v;
            } else {
                float *const cache = (which == 1) ? p.kcache : p.vcache;
                const int hh = rr >> 6, dd = rr & 63;        // head-major cache: [H][P][64]
                *reinterpret_cast<float4 *>(cache + (((size_t)hh * p.P + p.st->n_past + col) << 6) + dd) = v;
            }
        } else {                                             // EPI_RESID
            const float4 er = *reinterpret_cast<const float4 *>(p.resid + (size_t)col * p.ldr + orow);
            v.x = __fadd_rn(__fadd_rn(a4[0], eb.x), er.x); v.y = __fadd_rn(__fadd_rn(a4[1], eb.y), er.y);
            v.z = __fadd_rn(__fadd_rn(a4[2], eb.z), er.z); v.w = __fadd_rn(__fadd_rn(a4[3], eb.w), er.w);
            *reinterpret_cast<float4 *>(p.out + (size_t)col * p.ldo + orow) = v;
        }
    }
}

}  // namespace bgk
