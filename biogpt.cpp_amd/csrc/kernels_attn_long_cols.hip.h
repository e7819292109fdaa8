// Attention at 1025 .. 2048 keys, head size 64, over COLUMN STATES (SeqState: a column's own cache slot, t_vis, shared rows through pad[0] / pad[1]): the two
// kernels behind the batched calls of a wide file beyond 1024 keys (score_batch, embed_batch, score_continuations, the column-generation calls and the queue).
// kernels_attn_long.hip.h serves the context's own columns (DevState) only; attn_fast_kernel, attn_prefix_kernel and attn_runs_kernel end at 1024 keys.  Built
// for gfx950 in a unit of its own (attn_long_cols_tu.hip, -ffp-contract=off).
//
// Arithmetic per (head, query): the oracle's bo_attn_head, as kernels_attn_long.hip.h states it -- every score of a row is in LDS before its softmax starts
// (no online softmax), every product is rounded to f32 and added in double (no matrix instructions), no fused multiply-add in the attention
// arithmetic.  Both kernels store through store_head_output (the f32 row, and out_proj's two Q8 blocks when asked).
//
// attn_long_seq_kernel<SHARED> -- the column form: one workgroup of 1024 threads per (head, column), grid (H, N).  Column i is SeqState i: its slot is
//   col_mode ? seq_id : i (times kv_seq_stride), its visible keys col_mode ? t_vis : n_past + 1, clamped to min(t_cap, P, 2048); SHARED: rows j < pad[0] are
//   read in slot pad[1].  The split of work and the association of the three double sums are EXACTLY attn_long_col_kernel's (scores: 4 lanes per key and the quad
//   DPP reduce; softmax: thread = keys tid and tid + 1024, two block exchanges; PV: wave = key slice j mod 16, lane = dim, the 16 slices added in order); only
//   the row addresses differ (a select between two bases per load, no branch around it).  So a column has the bits the context's own column has at the same
//   keys.  Every load is guarded by the column's OWN visible keys: a launch may mix a 5-key column with a 2048-key one, and each costs what it sees.
//   It serves the decode steps (Cols::PerSequence, shared or not) and every packed pass the run form does not take.  LDS as attn_long_col_kernel: 16 576 bytes.
//
// attn_long_runs_kernel -- the run form: attn_long_tile_kernel's register tiling over RUNS of packed columns (col_mode 1).  A run {c0, n} is up to 16
//   neighbouring columns with equal (seq_id, pad[0], pad[1]) -- the chunks of one prompt, the tokens of one continuation (the host planner, long_runs_plan in
//   engine.hip); the plan goes up behind the pass's column states.  One workgroup of 1024 threads = 16 waves per (head, run), grid (H, runs):
//   LDS      as attn_long_tile_kernel: S [t_cap][16] f32 | Q [16][64] | maxima [16][68] | row sums [16][16] f64 | the 16 queries' visible keys:
//            attn_long_runs_smem_bytes(t_cap) == attn_long_tile_smem_bytes(t_cap), 141 632 bytes at 2048 keys, opt-in attribute set once per device.
//   scores   thread = (2 consecutive keys, 4 queries), the 64 dims walked in order; K rows straight from global / L2, each row clamped into the table by
//            itself (any P); ONE pointer per row, chosen before the dim loop from the two wave-uniform bases (own slot / shared slot) by j < pad[0].
//   softmax  thread = (query, 1 of 64 key slots): table exponent, double row sum, p = fl32(e * inv) written back.
//   PV       wave = key slice (j mod 16), lane = (4 queries, 4 dims); the key of a trip is wave-uniform, so is the choice of its base.  Then the parked-sums
//            exchange of attn_long_tile_kernel, and wave q stores query q.
//   bounds   per query from t_vis (a query beyond the run's n has none and stores nothing); every loop ends at the LARGEST t_vis of the run -- the maximum
//            over its columns, not the last column's.
//   Because the association of every sum is attn_long_tile_kernel's, a function of the key index and the dim alone, a column's bits do not depend on the run it
//   sits in, on the run's length or on where the shared rows end (tests/test_gpu_attn_long_cols_kernels.py cuts one pass into runs two ways).
//
// hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -Rpass-analysis=kernel-resource-usage (ROCm 7; DESIGN 4.4 quotes it):
//   attn_long_seq_kernel<false>   VGPRs  62   AGPRs 0   SGPRs 47   scratch 0   spills 0   LDS 16 576                        occupancy 8 waves / SIMD
//   attn_long_seq_kernel<true>    VGPRs  66   AGPRs 0   SGPRs 48   scratch 0   spills 0   LDS 16 576                        occupancy 7 waves / SIMD
//   attn_long_runs_kernel         VGPRs 122   AGPRs 0   SGPRs 49   scratch 0   spills 0   LDS 0 static (dynamic as above)   occupancy 4 waves / SIMD
// (<true>: the selected row pointers cost 4 registers, so one workgroup of 16 waves is resident per compute unit, not two; held to 8 waves per SIMD it spills 12
// bytes per lane, which this header does not accept)
#pragma once

#define BGK_ATTN_LONG_NO_KERNELS      // the constants, the LDS sizes and long_inv_sum of kernels_attn_long.hip.h without its two kernels
#include "kernels_attn_long.hip.h"

namespace bgk {

constexpr int LONG_RUN_COLS = LONG_TILE_COLS;      // columns of a run: the queries of one workgroup

struct AttnLongRunsParams {
    AttnParams a;
    const int32_t *runs;                // [n_runs][2]: c0, n
};

// dynamic LDS of attn_long_runs_kernel: attn_long_tile_kernel's areas; the last 64 bytes hold the 16 queries' visible keys
__host__ __device__ inline size_t attn_long_runs_smem_bytes(int t_cap) { return attn_long_tile_smem_bytes(t_cap); }

template <bool SHARED>
__global__ __launch_bounds__(1024) void attn_long_seq_kernel(const AttnParams p) {
    constexpr int DK = 64, NW = 16;
    __shared__ float S[LONG_ATTN_MAX_KEYS];
    __shared__ double pv[LONG_ATTN_THREADS];
    __shared__ double red[NW];
    __shared__ float redf[NW];
    const int h = blockIdx.x, i = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int D = p.D;
    const SeqState cs = p.seq[i];
    // every load below is guarded by T: rows in [T, t_cap) are never touched
    const int T = max(0, min(p.col_mode ? cs.t_vis : cs.n_past + 1, min(min(p.t_cap, p.P), LONG_ATTN_MAX_KEYS)));
    const size_t head = (size_t)h * p.P * DK;
    const size_t own_off = (size_t)(p.col_mode ? cs.seq_id : i) * p.kv_seq_stride + head;
    // SHARED: the same bases in the shared slot, and the first row that is the column's own
    const int n_shared = SHARED ? cs.pad[0] : 0;
    const size_t shr_off = SHARED ? (size_t)cs.pad[1] * p.kv_seq_stride + head : own_off;

    // ---- scores: 4 lanes per key, 256 keys per pass, two passes' loads in flight ----
    const int ksub = tid & 3, kidx = tid >> 2;
    const float4 *kbase = reinterpret_cast<const float4 *>(p.kcache + own_off) + ksub;       // [H][P][dk]
    const float4 *kshr = reinterpret_cast<const float4 *>(p.kcache + shr_off) + ksub;
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
            const float4 *krow = ((SHARED && j < n_shared) ? kshr : kbase) + (size_t)j * (DK / 4);
#pragma unroll
            for (int m = 0; m < 4; m++) kr[ps][m] = (j < T) ? krow[4 * m] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
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
    const float *__restrict__ vbase = p.vcache + own_off + lane;
    const float *__restrict__ vshr = p.vcache + shr_off + lane;
    double a0 = 0.0, a1 = 0.0;
    for (int j = wave; j < T; j += NW * 8) {
        float v8[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int jj = j + NW * k;
            v8[k] = (jj < T) ? ((SHARED && jj < n_shared) ? vshr : vbase)[(size_t)jj * DK] : 0.0f;
        }
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

__global__ __launch_bounds__(1024) void attn_long_runs_kernel(const AttnLongRunsParams rp) {
    constexpr int DK = 64, NW = 16, G = LONG_RUN_COLS, MXP = LONG_TILE_MXP, NT = LONG_ATTN_THREADS, KT = 2;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const AttnParams &p = rp.a;
    const int t_cap = min(min(p.t_cap, p.P), LONG_ATTN_MAX_KEYS);
    const size_t main_bytes = attn_long_tile_main_bytes(t_cap);
    float *const S = reinterpret_cast<float *>(smem_raw);                       // [key][G]: scores, then e, then probabilities
    double *const pvp = reinterpret_cast<double *>(smem_raw);                   // [8][G][DK] parked partial outputs (after the PV loop)
    float *const Qs = reinterpret_cast<float *>(smem_raw + main_bytes);         // [G][DK]
    float *const s_mx = Qs + G * DK;                                            // [G][MXP]: per query the maxima of the 64 (wave, lane row) key groups
    double *const s_sum = reinterpret_cast<double *>(s_mx + G * MXP);           // [16 waves][G]
    int *const s_T = reinterpret_cast<int *>(s_sum + NW * G);                   // [G]: a query's visible keys (0: beyond the run)
    const int h = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N = p.N, D = p.D;
    // (the planner: 0 <= c0, 1 <= n <= 16, c0 + n <= N; clamped all the same, so that no table can send a load outside the pass)
    const int c0 = min(max(rp.runs[2 * (size_t)blockIdx.y], 0), N - 1);
    const int n = max(1, min(min(rp.runs[2 * (size_t)blockIdx.y + 1], G), N - c0));
    // the run's slots: every column of a run has the first column's (seq_id, pad[0], pad[1])
    const SeqState first = p.seq[c0];
    const int n_shared = first.pad[0];
    const size_t head = (size_t)h * p.P * DK;
    const size_t own_off = (size_t)first.seq_id * p.kv_seq_stride + head;
    const size_t shr_off = n_shared > 0 ? (size_t)first.pad[1] * p.kv_seq_stride + head : own_off;

    if (tid < 256) {
        const int q = tid >> 4, d4 = tid & 15;
        reinterpret_cast<float4 *>(Qs)[tid] = *reinterpret_cast<const float4 *>(p.q + (size_t)(c0 + min(q, n - 1)) * D + (size_t)h * DK + 4 * d4);
    }
    if (tid < G) s_T[tid] = tid < n ? max(0, min(p.seq[c0 + tid].t_vis, t_cap)) : 0;
    for (int i = tid; i < G * MXP; i += NT) s_mx[i] = -INFINITY;
    __syncthreads();
    int Tmax = 0;                                                               // the largest of the run, whichever column has it
#pragma unroll
    for (int q = 0; q < G; q++) Tmax = max(Tmax, s_T[q]);

    // ---- scores: a thread owns 4 queries x KT = 2 keys and walks the 64 dims in order ----
    {
        const int kg = tid >> 2, qg = tid & 3;
        const at_f4 *kown = reinterpret_cast<const at_f4 *>(p.kcache + own_off);
        const at_f4 *kshr = reinterpret_cast<const at_f4 *>(p.kcache + shr_off);
        const at_f4 *qbase = reinterpret_cast<const at_f4 *>(Qs + 4 * qg * DK);
        for (int j0 = 0; j0 < Tmax; j0 += KT * 256) {
            if (j0 + KT * 16 * wave >= Tmax) break;                              // this wave's 32 keys are past every query's context
            const int jb = j0 + KT * kg;
            // each key row clamped into the table by itself (what is computed from a clamped row is never stored): any P.  One pointer per row: the
            // slot's base is picked here, from two wave-uniform bases
            const at_f4 *krow[KT];
#pragma unroll
            for (int c = 0; c < KT; c++) krow[c] = (jb + c < n_shared ? kshr : kown) + (size_t)min(jb + c, p.P - 1) * (DK / 4);
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
            // the softmax's first pass, taken while the scores are in registers (attn_long_tile_kernel's): one maximum per (wave, lane row, query) in s_mx
            const int4 Tq = *reinterpret_cast<const int4 *>(s_T + 4 * qg);      // (after the MAC loop: not held in registers across it)
            float mq[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
            for (int c = 0; c < KT; c++) {
                const int j = jb + c;
                if (j < t_cap) {
                    const float4 sc = make_float4(j < Tq.x ? (float)acc[0][c] : -INFINITY, j < Tq.y ? (float)acc[1][c] : -INFINITY,
                                                  j < Tq.z ? (float)acc[2][c] : -INFINITY, j < Tq.w ? (float)acc[3][c] : -INFINITY);
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
        const int Tw = s_T[q];
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
        const at_f4 *vown = reinterpret_cast<const at_f4 *>(p.vcache + own_off) + dg;
        const at_f4 *vshr = reinterpret_cast<const at_f4 *>(p.vcache + shr_off) + dg;
        const float *Sq = S + 4 * qg;
        int j = wave;
        // 4 keys of this slice per trip, all loads first; whole trips carry no guards (every key < Tmax <= t_cap <= P).  A trip's keys are wave-uniform: so
        // is the choice of each row's slot
        for (; j + 3 * NW < Tmax; j += 4 * NW) {
            at_f4 v[4], pr[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int jj = j + NW * u;
                v[u] = (jj < n_shared ? vshr : vown)[(size_t)jj * (DK / 4)];
                pr[u] = *reinterpret_cast<const at_f4 *>(Sq + (size_t)jj * G);
            }
#pragma unroll
            for (int u = 0; u < 4; u++) mac4(v[u], pr[u]);
        }
        if (j < Tmax) {                                   // the last, partial trip
            at_f4 v[4], pr[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int jj = min(j + NW * u, Tmax - 1);
                v[u] = (jj < n_shared ? vshr : vown)[(size_t)jj * (DK / 4)];
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
    if (wave < n) {
        double t0 = 0.0, t1 = 0.0;
#pragma unroll
        for (int s2 = 0; s2 < 8; s2 += 2) {
            t0 += pvp[((size_t)s2 * G + wave) * DK + lane];
            t1 += pvp[((size_t)(s2 + 1) * G + wave) * DK + lane];
        }
        store_head_output(p, c0 + wave, h, lane, (float)(t0 + t1), p.oq_q != nullptr);
    }
}

}  // namespace bgk
