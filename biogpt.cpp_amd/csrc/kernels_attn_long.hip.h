// Attention at 1025 .. 2048 keys, head size 64, the context's own columns (device state: n_past / causal / chunk): the two kernels behind
// biogpt_hip_long_context.  The head-size-64 kernels of kernels_fast.hip.h end at 1024 keys; beyond, a pass had attn_kernel only, which writes no Q8 blocks
// for out_proj, so the wide decode / chunk / pass layers ended there too.  Built for gfx950 (160 KB of LDS per compute unit) in a unit of its own
// (attn_long_tu.hip, -ffp-contract=off).
//
// Arithmetic per (head, query): the oracle's bo_attn_head (tests/attn_ref.py restates it) --
//   score_j = fl32(double sum of the 64 f32-rounded products) ; max over the visible keys ; e_j = exp_tab[fp16(fl32(score_j - max))] ;
//   inv = fl32(1 / double sum of e_j) ; p_j = fl32(e_j * inv) ; out_d = fl32(double sum of fl32(v_jd * p_j)).
// Only the association of the three double sums is the kernels' own.  The table exponent needs the row's TRUE maximum before any e_j exists: every score of a
// row is in LDS before its softmax starts (no online softmax); f32 matrix instructions cannot round each product to f32 and add in double: none.
// No fused multiply-add anywhere: every product is a v_mul_f32 / v_pk_mul_f32, every sum a v_add_f64, and the reciprocal is refined by un-fused Newton steps.
//
// attn_long_tile_kernel -- 16 consecutive query columns of one head per workgroup, grid (H, ceil(N / 16)), 1024 threads = 16 waves.
//   LDS      S [t_cap][16] f32 (scores, then e, then p; 128 KB at 2048 keys; later the first 64 KB hold the PV partial sums) | Q [16][64] f32 | maxima [16][68] f32
//            | row sums [16 waves][16] f64: t_cap * 64 + 10 560 bytes of dynamic LDS (141 632 at 2048 keys), the opt-in attribute set once per device.  One workgroup
//            per compute unit is resident, so the workgroup brings the occupancy itself: 16 waves = four per SIMD in both MAC phases.
//   scores   thread = (1 of 256 key groups of 2 consecutive keys, 1 of 4 query groups of 4): 8 double accumulators, the 64 dims walked IN ORDER (the oracle's own
//            association); per 4 dims 2 K float4 straight from global / L2 into registers (each row clamped to P - 1 by itself: any table size) and 4 Q float4
//            from LDS.  (4 keys per thread, attn_tile_kernel's tile, spills 19 registers under the 128 of a 1024-thread workgroup once every row has its own
//            address.)  A sweep is 512 keys; a wave whose 32 keys lie past the tile's last visible key leaves the sweep.  The row maxima are taken while the
//            scores are in registers (DPP over the 4 key groups of a lane row -> one value per (wave, lane row, query)).
//   softmax  thread = (query, 1 of 64 key slots): table exponent, double row sum (fp16 values below 2^11: exact in any order), p = fl32(e * inv) written back.
//   PV       wave = key slice (j mod 16), lane = (4 queries, 4 dims): per key one V float4 (a wave reads whole 256-byte rows from global / L2) and one LDS float4
//            of 4 probabilities for 16 products into 16 double accumulators; K / V rows go through registers, no LDS ring (the ~19 KB left would hold one).
//   exchange the 16 slices' sums: waves 8 .. 15 park theirs in LDS (64 KB, the area of the scores), waves 0 .. 7 add their own on top, then wave q adds the 8
//            pairs of query q and stores it through store_head_output (f32 row + the two Q8 blocks of out_proj's activation row).
//   bounds   every loop ends at the visible keys of the workgroup's LAST column (they grow with the column), never at t_cap: a causal 2048-token pass does 16
//            keys of work in its first tile.  Visible keys are clamped to t_cap, row addresses to the table.
//
// attn_long_col_kernel -- one query column per workgroup, grid (H, N), 1024 threads: the single token and the columns of a chunk (and of a pass of few columns).
//   LDS      S [2048] f32 (8 KB) | PV partial sums [1024] f64 (8 KB) | two 16-entry exchange arrays: 16 576 bytes, static.
//   scores   4 lanes per key (lane s of a quad owns float4 s, 4 + s, 8 + s, 12 + s of the row; four double accumulators, quad DPP reduce: attn_fast_kernel's
//            association), 256 keys per pass, two passes' loads in flight, up to 8 passes; every load is guarded by the column's own visible keys.
//   softmax  thread = keys tid and tid + 1024: one block exchange for the maximum, one for the double sum; p = fl32(e * inv) written to S.
//   PV       wave = key slice (j mod 16), lane = dim: 8 V values in flight per thread, two double accumulators; the 16 slices are added by wave 0 through LDS.
//   A 2048-key head is 262 k MACs: one compute unit, no hand-off between workgroups, one launch.
//
// hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -Rpass-analysis=kernel-resource-usage (ROCm 7; DESIGN 4.4 quotes it):
//   attn_long_tile_kernel   VGPRs 126   AGPRs 0   SGPRs 59   scratch 0   spills 0   LDS 0 static (dynamic as above)   occupancy 4 waves / SIMD
//   attn_long_col_kernel    VGPRs  62   AGPRs 0   SGPRs 48   scratch 0   spills 0   LDS 16 576                        occupancy 8 waves / SIMD
// (the v_fma_f32 / v_fmac_f32 / v_div_fmas_f32 of either kernel's ISA are the expansion of the two IEEE f32 divisions of store_head_output, nothing else)
#pragma once

#include "kernels_fast.hip.h"

namespace bgk {

constexpr int LONG_ATTN_MAX_KEYS = 2048;      // the load bound of both kernels
constexpr int LONG_ATTN_THREADS = 1024, LONG_TILE_COLS = 16, LONG_TILE_MXP = 68;
constexpr int LONG_COL_LDS_BYTES = LONG_ATTN_MAX_KEYS * 4 + 1024 * 8 + 16 * 8 + 16 * 4;

// dynamic LDS of attn_long_tile_kernel: max(scores [t_cap][16] f32, parked partial sums [8][16][64] f64) + Q + maxima + row sums
__host__ __device__ inline size_t attn_long_tile_main_bytes(int t_cap) {
    const size_t sc = (size_t)t_cap * LONG_TILE_COLS * 4, po = (size_t)8 * LONG_TILE_COLS * 64 * 8;
    return sc > po ? sc : po;
}
__host__ __device__ inline size_t attn_long_tile_smem_bytes(int t_cap) {
    return attn_long_tile_main_bytes(t_cap) + (size_t)LONG_TILE_COLS * 64 * 4 + (size_t)LONG_TILE_COLS * LONG_TILE_MXP * 4 + (size_t)16 * LONG_TILE_COLS * 8 + 64;
}

// fl32(1 / s) without a fused multiply-add: v_rcp_f64 and two Newton steps r += r * (1 - s * r) in separately rounded operations.  s is a sum of fp16 values in
// [1, 2048]; s * r is within 2^-26 of 1, so 1 - fl(s * r) is exact and carries the product's rounding (2^-53) alone: r ends within 1.5 ulp(double) of the
// quotient, which rounds to the float of the IEEE division except where the quotient lies that close to the middle of two floats (~1e-8 of inputs).
__device__ __forceinline__ float long_inv_sum(double s) {
    double r = __builtin_amdgcn_rcp(s);
    r = __dadd_rn(r, __dmul_rn(r, __dsub_rn(1.0, __dmul_rn(s, r))));
    r = __dadd_rn(r, __dmul_rn(r, __dsub_rn(1.0, __dmul_rn(s, r))));
    return (float)r;
}

#ifndef BGK_ATTN_LONG_NO_KERNELS      // (kernels_attn_long_cols.hip.h reads the constants and helpers above in a unit of its own)
__global__ __launch_bounds__(1024) void attn_long_tile_kernel(const AttnParams p) {
    constexpr int DK = 64, NW = 16, G = LONG_TILE_COLS, MXP = LONG_TILE_MXP, NT = LONG_ATTN_THREADS, KT = 2;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int t_cap = min(min(p.t_cap, p.P), LONG_ATTN_MAX_KEYS);
    const size_t main_bytes = attn_long_tile_main_bytes(t_cap);
    float *const S = reinterpret_cast<float *>(smem_raw);                       // [key][G]: scores, then e, then probabilities
    double *const pvp = reinterpret_cast<double *>(smem_raw);                   // [8][G][DK] parked partial outputs (after the PV loop)
    float *const Qs = reinterpret_cast<float *>(smem_raw + main_bytes);         // [G][DK]
    float *const s_mx = Qs + G * DK;                                            // [G][MXP]: per query the maxima of the 64 (wave, lane row) key groups
    double *const s_sum = reinterpret_cast<double *>(s_mx + G * MXP);           // [16 waves][G]
    const int h = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N = p.N, D = p.D;
    // dispatch order as attn_tile_kernel's: the long half of the tiles first (longest first), then the short half ascending
    const int ny = (int)gridDim.y, yb = (int)blockIdx.y, nhalf = (ny + 1) / 2;
    const int i0 = ((yb < nhalf) ? ny - 1 - yb : yb - nhalf) * G;

    if (tid < 256) {
        const int q = tid >> 4, d4 = tid & 15;
        reinterpret_cast<float4 *>(Qs)[tid] = *reinterpret_cast<const float4 *>(p.q + (size_t)min(i0 + q, N - 1) * D + (size_t)h * DK + 4 * d4);
    }
    for (int i = tid; i < G * MXP; i += NT) s_mx[i] = -INFINITY;
    const int Tmax = min(visible_keys(p.st, min(i0 + G - 1, N - 1), N), t_cap);  // visibility grows with the column index
    __syncthreads();

    // ---- scores: a thread owns 4 queries x KT = 2 keys and walks the 64 dims in order ----
    {
        const int kg = tid >> 2, qg = tid & 3;
        const at_f4 *kbase = reinterpret_cast<const at_f4 *>(p.kcache + (size_t)h * p.P * DK);
        const at_f4 *qbase = reinterpret_cast<const at_f4 *>(Qs + 4 * qg * DK);
        for (int j0 = 0; j0 < Tmax; j0 += KT * 256) {
            if (j0 + KT * 16 * wave >= Tmax) break;                              // this wave's 32 keys are past every query's context
            const int jb = j0 + KT * kg;
            // each key row clamped into the table by itself (what is computed from a clamped row is never stored): any P
            const at_f4 *krow[KT];
#pragma unroll
            for (int c = 0; c < KT; c++) krow[c] = kbase + (size_t)min(jb + c, p.P - 1) * (DK / 4);
            double acc[4][KT];
#pragma unroll
            for (int qi = 0; qi < 4; qi++)
#pragma unroll
                for (int c = 0; c < KT; c++) acc[qi][c] = 0.0;
#pragma unroll 2
            for (int m = 0; m < DK / 4; m++) {
                at_f4 kv[KT], qv[4];
#pragma unroll
                for (int c = 0; c < KT; c++) kv[c] = krow[c][m];
#pragma unroll
                for (int qi = 0; qi < 4; qi++) qv[qi] = qbase[qi * (DK / 4) + m];
                // two dims of ONE (query, key) per packed multiply; the sums stay in dim order per accumulator
#pragma unroll
                for (int hf = 0; hf < 2; hf++) {
                    at_f2 pr2[4][KT];
#pragma unroll
                    for (int qi = 0; qi < 4; qi++)
#pragma unroll
                        for (int c = 0; c < KT; c++) pr2[qi][c] = (hf == 0 ? kv[c].lo : kv[c].hi) * (hf == 0 ? qv[qi].lo : qv[qi].hi);
#pragma unroll
                    for (int qi = 0; qi < 4; qi++)
#pragma unroll
                        for (int c = 0; c < KT; c++) acc[qi][c] += (double)pr2[qi][c].x;
#pragma unroll
                    for (int qi = 0; qi < 4; qi++)
#pragma unroll
                        for (int c = 0; c < KT; c++) acc[qi][c] += (double)pr2[qi][c].y;
                }
            }
            // the softmax's first pass, taken while the scores are in registers: per query the maximum of this thread's keys, then of the four key groups of its
            // lane row (lanes 4 apart: same query group) -> one value per (wave, lane row, query) in s_mx (preset to -inf: a wave without keys writes nothing)
            int Tq[4];                                                           // (after the MAC loop: not held in registers across it)
#pragma unroll
            for (int qi = 0; qi < 4; qi++) Tq[qi] = (i0 + 4 * qg + qi < N) ? min(visible_keys(p.st, i0 + 4 * qg + qi, N), t_cap) : 0;
            float mq[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
            for (int c = 0; c < KT; c++) {
                const int j = jb + c;
                if (j < t_cap) {
                    const float4 sc = make_float4(j < Tq[0] ? (float)acc[0][c] : -INFINITY, j < Tq[1] ? (float)acc[1][c] : -INFINITY,
                                                  j < Tq[2] ? (float)acc[2][c] : -INFINITY, j < Tq[3] ? (float)acc[3][c] : -INFINITY);
                    *reinterpret_cast<float4 *>(S + (size_t)j * G + 4 * qg) = sc;
                    mq[0] = fmaxf(mq[0], sc.x); mq[1] = fmaxf(mq[1], sc.y); mq[2] = fmaxf(mq[2], sc.z); mq[3] = fmaxf(mq[3], sc.w);
                }
            }
#pragma unroll
            for (int qi = 0; qi < 4; qi++) {
                mq[qi] = fmaxf(mq[qi], dpp_f<DPP_ROW_ROR4>(mq[qi]));
                mq[qi] = fmaxf(mq[qi], dpp_f<DPP_ROW_ROR8>(mq[qi]));
            }
            if ((lane & 12) == 0) {
                const int grp = wave * 4 + (lane >> 4);
#pragma unroll
                for (int qi = 0; qi < 4; qi++) {
                    float *const slot = s_mx + (4 * qg + qi) * MXP + grp;
                    *slot = (j0 == 0) ? mq[qi] : fmaxf(mq[qi], *slot);       // (the later sweeps: the same lane comes back to its slot)
                }
            }
        }
    }
    __syncthreads();

    // ---- softmax: thread = (query, one of 64 key slots) ----
    {
        const int q = tid & 15, slot = tid >> 4;
        const int Tw = (i0 + q < N) ? min(visible_keys(p.st, i0 + q, N), t_cap) : 0;
        float mx;
        {
            const at_f4 *mrow = reinterpret_cast<const at_f4 *>(s_mx + q * MXP);
            at_f4 m4 = mrow[0];
#pragma unroll
            for (int s2 = 1; s2 < 16; s2++) { const at_f4 t = mrow[s2]; m4.x = fmaxf(m4.x, t.x); m4.y = fmaxf(m4.y, t.y); m4.z = fmaxf(m4.z, t.z); m4.w = fmaxf(m4.w, t.w); }
            mx = fmaxf(fmaxf(m4.x, m4.y), fmaxf(m4.z, m4.w));
        }
        double sum = 0.0;
        for (int j = slot; j < Tw; j += 512) {
            float e[8];
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const int jj = j + 64 * u;
                e[u] = (jj < Tw) ? h2f(p.exp_tab[f2h(__fsub_rn(S[(size_t)jj * G + q], mx))]) : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const int jj = j + 64 * u;
                if (jj < Tw) { S[(size_t)jj * G + q] = e[u]; sum += (double)e[u]; }
            }
        }
        sum += __shfl_xor(sum, 16, 64); sum += __shfl_xor(sum, 32, 64);          // the wave's four slots of this query
        if (lane < 16) s_sum[wave * G + q] = sum;
        __syncthreads();
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < NW; w++) t += s_sum[w * G + q];
        const float inv = (Tw > 0) ? long_inv_sum(t) : 0.0f;
        for (int j = slot; j < Tmax; j += 512) {
            float pr[8];
#pragma unroll
            for (int u = 0; u < 8; u++) { const int jj = j + 64 * u; pr[u] = (jj < Tw) ? S[(size_t)jj * G + q] : 0.0f; }
#pragma unroll
            for (int u = 0; u < 8; u++) { const int jj = j + 64 * u; if (jj < Tmax) S[(size_t)jj * G + q] = __fmul_rn(pr[u], inv); }
        }
    }
    __syncthreads();

    // ---- PV: wave = key slice (j mod 16), lane = (4 queries, 4 dims) ----
    double acc[4][4];
#pragma unroll
    for (int qi = 0; qi < 4; qi++)
#pragma unroll
        for (int c = 0; c < 4; c++) acc[qi][c] = 0.0;
    const int qg = lane >> 4, dg = lane & 15;
    {
        auto mac4 = [&](const at_f4 &v, const at_f4 &pr) __attribute__((always_inline)) {
#pragma unroll
            for (int qi = 0; qi < 4; qi++) {
                const at_f2 pp = {pr[qi], pr[qi]};
                const at_f2 a = v.lo * pp, b = v.hi * pp;
                acc[qi][0] += (double)a.x; acc[qi][1] += (double)a.y; acc[qi][2] += (double)b.x; acc[qi][3] += (double)b.y;
            }
        };
        const at_f4 *vrow = reinterpret_cast<const at_f4 *>(p.vcache + (size_t)h * p.P * DK) + dg;
        const float *Sq = S + 4 * qg;
        int j = wave;
        // 4 keys of this slice per trip, all loads first; whole trips carry no guards (every key < Tmax <= t_cap <= P)
        for (; j + 3 * NW < Tmax; j += 4 * NW) {
            at_f4 v[4], pr[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                v[u] = vrow[(size_t)(j + NW * u) * (DK / 4)];
                pr[u] = *reinterpret_cast<const at_f4 *>(Sq + (size_t)(j + NW * u) * G);
            }
#pragma unroll
            for (int u = 0; u < 4; u++) mac4(v[u], pr[u]);
        }
        if (j < Tmax) {                                   // the last, partial trip
            at_f4 v[4], pr[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int jj = min(j + NW * u, Tmax - 1);
                v[u] = vrow[(size_t)jj * (DK / 4)];
                pr[u] = *reinterpret_cast<const at_f4 *>(Sq + (size_t)jj * G);
            }
#pragma unroll
            for (int u = 0; u < 4; u++)
                if (j + NW * u < Tmax) mac4(v[u], pr[u]);   // (a key past Tmax is not touched: its V row may never have been written)
        }
    }
    __syncthreads();                                      // every read of S is done: its first 64 KB become pvp
    // ---- the 16 slices' sums: waves 8 .. 15 park theirs, waves 0 .. 7 add their own on top, wave q finishes query q ----
    if (wave >= 8) {
#pragma unroll
        for (int qi = 0; qi < 4; qi++)
#pragma unroll
            for (int c = 0; c < 4; c++) pvp[((size_t)(wave - 8) * G + 4 * qg + qi) * DK + 4 * dg + c] = acc[qi][c];
    }
    __syncthreads();
    if (wave < 8) {
#pragma unroll
        for (int qi = 0; qi < 4; qi++)
#pragma unroll
            for (int c = 0; c < 4; c++) {
                double *const at = pvp + ((size_t)wave * G + 4 * qg + qi) * DK + 4 * dg + c;
                *at = acc[qi][c] + *at;
            }
    }
    __syncthreads();
    if (i0 + wave < N) {
        double t0 = 0.0, t1 = 0.0;
#pragma unroll
        for (int s2 = 0; s2 < 8; s2 += 2) {
            t0 += pvp[((size_t)s2 * G + wave) * DK + lane];
            t1 += pvp[((size_t)(s2 + 1) * G + wave) * DK + lane];
        }
        store_head_output(p, i0 + wave, h, lane, (float)(t0 + t1), p.oq_q != nullptr);
    }
}

__global__ __launch_bounds__(1024) void attn_long_col_kernel(const AttnParams p) {
    constexpr int DK = 64, NW = 16;
    __shared__ float S[LONG_ATTN_MAX_KEYS];
    __shared__ double pv[LONG_ATTN_THREADS];
    __shared__ double red[NW];
    __shared__ float redf[NW];
    const int h = blockIdx.x, i = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int D = p.D;
    // every load below is guarded by T: rows in [T, t_cap) are never touched
    const int T = min(visible_keys(p.st, i, p.N), min(min(p.t_cap, p.P), LONG_ATTN_MAX_KEYS));

    // ---- scores: 4 lanes per key, 256 keys per pass, two passes' loads in flight ----
    const int ksub = tid & 3, kidx = tid >> 2;
    const float4 *kbase = reinterpret_cast<const float4 *>(p.kcache + (size_t)h * p.P * DK) + ksub;       // [H][P][dk]
    const float4 *qp = reinterpret_cast<const float4 *>(p.q + (size_t)i * D + (size_t)h * DK) + ksub;
    float4 qv[4];
#pragma unroll
    for (int m = 0; m < 4; m++) qv[m] = qp[4 * m];
    float mx = -INFINITY;
    for (int j0 = 0; j0 < T; j0 += 512) {
        float4 kr[2][4];
#pragma unroll
        for (int ps = 0; ps < 2; ps++) {
            const int j = j0 + 256 * ps + kidx;
#pragma unroll
            for (int m = 0; m < 4; m++) kr[ps][m] = (j < T) ? kbase[(size_t)j * (DK / 4) + 4 * m] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
#pragma unroll
        for (int ps = 0; ps < 2; ps++) {
            const int j = j0 + 256 * ps + kidx;
            double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll
            for (int m = 0; m < 4; m++) {
                a0 += (double)__fmul_rn(kr[ps][m].x, qv[m].x); a1 += (double)__fmul_rn(kr[ps][m].y, qv[m].y);
                a2 += (double)__fmul_rn(kr[ps][m].z, qv[m].z); a3 += (double)__fmul_rn(kr[ps][m].w, qv[m].w);
            }
            double acc = (a0 + a1) + (a2 + a3);
            acc += dpp_d<DPP_QUAD_XOR1>(acc);
            acc += dpp_d<DPP_QUAD_XOR2>(acc);
            if (j < T) {
                const float sc = (float)acc;
                if (ksub == 0) S[j] = sc;
                mx = fmaxf(mx, sc);
            }
        }
    }
    mx = wave_max_f32(mx);
    if (lane == 0) redf[wave] = mx;
    __syncthreads();                                      // (also publishes S)
    mx = redf[0];
#pragma unroll
    for (int w = 1; w < NW; w++) mx = fmaxf(mx, redf[w]);

    // ---- softmax: thread = keys tid and tid + 1024 ----
    float e[2];
    double sum = 0.0;
#pragma unroll
    for (int u = 0; u < 2; u++) {
        const int j = tid + LONG_ATTN_THREADS * u;
        e[u] = (j < T) ? h2f(p.exp_tab[f2h(__fsub_rn(S[j], mx))]) : 0.0f;
        sum += (double)e[u];                              // (fp16 values: exact in any order)
    }
    sum = wave_sum_f64(sum);
    if (lane == 0) red[wave] = sum;
    __syncthreads();
    sum = 0.0;
#pragma unroll
    for (int w = 0; w < NW; w++) sum += red[w];
    const float inv = long_inv_sum(sum);
#pragma unroll
    for (int u = 0; u < 2; u++) {
        const int j = tid + LONG_ATTN_THREADS * u;
        if (j < T) S[j] = __fmul_rn(e[u], inv);
    }
    __syncthreads();

    // ---- PV: wave = key slice (j mod 16), lane = dim; 8 V values in flight ----
    const float *__restrict__ vbase = p.vcache + (size_t)h * p.P * DK + lane;
    double a0 = 0.0, a1 = 0.0;
    for (int j = wave; j < T; j += NW * 8) {
        float v8[8];
#pragma unroll
        for (int k = 0; k < 8; k++) v8[k] = (j + NW * k < T) ? vbase[(size_t)(j + NW * k) * DK] : 0.0f;
#pragma unroll
        for (int k = 0; k < 8; k += 2) {
            if (j + NW * k < T) a0 += (double)__fmul_rn(v8[k], S[j + NW * k]);
            if (j + NW * (k + 1) < T) a1 += (double)__fmul_rn(v8[k + 1], S[j + NW * (k + 1)]);
        }
    }
    pv[tid] = a0 + a1;
    __syncthreads();
    if (tid < DK) {
        double t0 = 0.0, t1 = 0.0;
#pragma unroll
        for (int s2 = 0; s2 < NW; s2 += 2) { t0 += pv[s2 * DK + tid]; t1 += pv[(s2 + 1) * DK + tid]; }
        store_head_output(p, i, h, tid, (float)(t0 + t1), p.oq_q != nullptr);
    }
}
#endif

}  // namespace bgk
