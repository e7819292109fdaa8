// attn_runs_kernel<8>: the attention of a packed pass (col_mode 1) whose neighbouring columns see the same first rows -- the passes of
// biogpt_hip_score_continuations_batch.  Included after kernels_fast.hip.h (AttnParams, store_head_output, inv_sum_f32, the DPP helpers).
#pragma once

namespace bgk {

// A RUN is up to 8 consecutive columns [c0, c0 + n) of the pass whose first R visible rows are the same rows [0, R) of ONE slot S; a column's rows
// [R, T_q) lie in its own slot seq_id.  Two kinds occur (the planner, attn_runs_plan in engine.hip, makes no other):
//   prefix runs        columns with pad[0] == 0 of one seq_id: 8 consecutive tokens of one prompt.  S = seq_id, R = the smallest t_vis of the run.
//   continuation runs  columns with equal (pad[0], pad[1]), pad[0] > 0: the candidates behind one prefix.  S = pad[1], R = pad[0].
// One workgroup per (head, run), 512 threads = 8 waves, column c0 + w is query w:
//   scores, shared   4 lanes per key, 128 keys per sweep: a K row of slot S is loaded ONCE and scored against the 8 queries (LDS)
//   scores, own      wave w: query w's rows [R, T_w) from its own slot, 16 keys per sweep
//   softmax          wave w: query w -- maximum, fp16-table exponent, double row sum (fp16 values: exact in any order), p = fl(e * inv_sum_f32(sum))
//   PV               wave s = slice s of 8, lane = dim: a V row of slot S is loaded once and goes into up to 8 double accumulators; own rows per query
// Per-element arithmetic is attn_fast_kernel's (__fmul_rn products, four double accumulators and the quad reduce for a score, the table exponent, a
// double row sum, inv_sum_f32).  The association of the double PV sum is a function of the key index alone: key j belongs to slice j mod 8 whichever
// side of R it lies on, a slice adds its keys in ascending j, and the 8 slices are combined in one fixed order.  So a column's output is a function of
// its query, its visible rows and T_q -- not of the run it sits in, of R, or of the pass (attn_prefix_kernel slices the own rows from n_shared: it has
// no such property).  Every load is bounded by min(t_cap, P, RUNS_MAX_KEYS) through T_q and R; the queries beyond a run's n have no keys and store
// nothing (wave-uniform).
constexpr int RUNS_MAX_KEYS = 1024;     // scores [keys][8] floats in LDS: 32 KB
constexpr int RUNS_MAX_COLS = 8;

struct AttnRunsParams {
    AttnParams a;
    const int32_t *runs;                // [n_runs][4]: c0, n, R, S
};

template <int G>
__global__ __launch_bounds__(512) void attn_runs_kernel(const AttnRunsParams rp) {
    static_assert(G == RUNS_MAX_COLS, "eight columns, one per wave");
    constexpr int DK = 64;
    __shared__ __attribute__((aligned(16))) float S[RUNS_MAX_KEYS * G];     // scores, then probabilities [key][query]; afterwards the PV partials [slice][query][dim] doubles
    __shared__ __attribute__((aligned(16))) float Q[G * DK];
    __shared__ int Tq[G];
    static_assert(sizeof(float) * RUNS_MAX_KEYS * G >= sizeof(double) * 8 * G * DK, "the PV partials fit the score area");
    const AttnParams &p = rp.a;
    const int h = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int cap = min(min(p.t_cap, p.P), RUNS_MAX_KEYS);
    const size_t head = (size_t)h * p.P * DK;
    const int32_t *run = rp.runs + 4 * (size_t)blockIdx.y;
    const int c0 = run[0], n = min(run[1], G);
    const int R = max(0, min(run[2], cap));
    const size_t shr_off = (size_t)run[3] * p.kv_seq_stride;
    const bool live = wv < n && c0 + wv < p.N;      // wave-uniform
    const int col = live ? c0 + wv : c0;

    // ---- queries and their visible keys into LDS (a query beyond the run: no keys) ----
    Q[wv * DK + lane] = live ? p.q[(size_t)col * p.D + (size_t)h * DK + lane] : 0.0f;
    if (lane == 0) Tq[wv] = live ? max(R, min(p.seq[col].t_vis, cap)) : 0;
    __syncthreads();

    const int ksub = tid & 3;
    // ---- scores over the shared rows: lane ksub of a quad owns float4 #(4m + ksub) of the key row ----
    {
        const float4 *kshr = reinterpret_cast<const float4 *>(p.kcache + shr_off + head) + ksub;
        for (int j = tid >> 2; j < R; j += 128) {
            float4 kr[4];
#pragma unroll
            for (int m = 0; m < 4; m++) kr[m] = kshr[(size_t)j * (DK / 4) + 4 * m];
#pragma unroll
            for (int q = 0; q < G; q++) {
                const float4 *qp = reinterpret_cast<const float4 *>(Q + q * DK) + ksub;
                double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll
                for (int m = 0; m < 4; m++) {
                    const float4 qv = qp[4 * m];
                    a0 += (double)__fmul_rn(kr[m].x, qv.x); a1 += (double)__fmul_rn(kr[m].y, qv.y);
                    a2 += (double)__fmul_rn(kr[m].z, qv.z); a3 += (double)__fmul_rn(kr[m].w, qv.w);
                }
                double acc = (a0 + a1) + (a2 + a3);
                acc += dpp_d<DPP_QUAD_XOR1>(acc);
                acc += dpp_d<DPP_QUAD_XOR2>(acc);
                if (ksub == 0) S[j * G + q] = (float)acc;
            }
        }
    }
    const size_t own_off = (size_t)p.seq[col].seq_id * p.kv_seq_stride;
    // ---- scores over a query's own rows: wave w, 16 keys per sweep ----
    {
        const int T = Tq[wv];
        const float4 *kown = reinterpret_cast<const float4 *>(p.kcache + own_off + head) + ksub;
        const float4 *qp = reinterpret_cast<const float4 *>(Q + wv * DK) + ksub;
        for (int j = R + (lane >> 2); j < T; j += 16) {
            double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll
            for (int m = 0; m < 4; m++) {
                const float4 kr = kown[(size_t)j * (DK / 4) + 4 * m], qv = qp[4 * m];
                a0 += (double)__fmul_rn(kr.x, qv.x); a1 += (double)__fmul_rn(kr.y, qv.y);
                a2 += (double)__fmul_rn(kr.z, qv.z); a3 += (double)__fmul_rn(kr.w, qv.w);
            }
            double acc = (a0 + a1) + (a2 + a3);
            acc += dpp_d<DPP_QUAD_XOR1>(acc);
            acc += dpp_d<DPP_QUAD_XOR2>(acc);
            if (ksub == 0) S[j * G + wv] = (float)acc;
        }
    }
    __syncthreads();

    // ---- softmax of query wv over its T keys (ggml_soft_max: fp16-table exp, double sum, scale by (float)(1/sum)) ----
    {
        const int T = Tq[wv];
        float mx = -INFINITY;
        for (int j = lane; j < T; j += 64) mx = fmaxf(mx, S[j * G + wv]);
        mx = wave_max_f32(mx);
        double sum = 0.0;
        for (int j = lane; j < T; j += 64) {
            const float val = h2f(p.exp_tab[f2h(__fsub_rn(S[j * G + wv], mx))]);
            S[j * G + wv] = val;
            sum += (double)val;
        }
        sum = wave_sum_f64(sum);
        const float inv = inv_sum_f32(sum);
        for (int j = lane; j < T; j += 64) S[j * G + wv] = __fmul_rn(S[j * G + wv], inv);
    }
    __syncthreads();

    // ---- PV: slice wv = the keys j with j mod 8 == wv, in ascending j across the border at R; dim lane ----
    double acc[G];
#pragma unroll
    for (int q = 0; q < G; q++) acc[q] = 0.0;
    {
        const float *__restrict__ vshr = p.vcache + shr_off + head + lane;
        int tq[G];
#pragma unroll
        for (int q = 0; q < G; q++) tq[q] = Tq[q];
        for (int j = wv; j < R; j += 32) {
            float v4[4];
#pragma unroll
            for (int k = 0; k < 4; k++) v4[k] = (j + 8 * k < R) ? vshr[(size_t)(j + 8 * k) * DK] : 0.0f;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int jj = j + 8 * k;
                if (jj < R) {
                    const float4 p0 = *reinterpret_cast<const float4 *>(S + jj * G), p1 = *reinterpret_cast<const float4 *>(S + jj * G + 4);
                    const float pr[G] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w};
#pragma unroll
                    for (int q = 0; q < G; q++)
                        if (jj < tq[q]) acc[q] += (double)__fmul_rn(v4[k], pr[q]);
                }
            }
        }
        const int j_own = R + ((wv - R) & 7);       // the first key from R on that belongs to this slice
#pragma unroll
        for (int q = 0; q < G; q++) {
            if (j_own >= tq[q]) continue;           // wave-uniform; also every query beyond the run (tq = 0)
            const size_t off_q = (size_t)p.seq[min(c0 + q, p.N - 1)].seq_id * p.kv_seq_stride;
            const float *__restrict__ vown = p.vcache + off_q + head + lane;
            for (int j = j_own; j < tq[q]; j += 8) acc[q] += (double)__fmul_rn(vown[(size_t)j * DK], S[j * G + q]);
        }
    }
    __syncthreads();      // every probability has been read: the area becomes the partials
    double *part = reinterpret_cast<double *>(S);
#pragma unroll
    for (int q = 0; q < G; q++) part[(wv * G + q) * DK + lane] = acc[q];
    __syncthreads();
    if (live) {
        double t0 = 0.0, t1 = 0.0;
#pragma unroll
        for (int s2 = 0; s2 < 8; s2 += 2) { t0 += part[(s2 * G + wv) * DK + lane]; t1 += part[((s2 + 1) * G + wv) * DK + lane]; }
        store_head_output(p, col, h, lane, (float)(t0 + t1), p.oq_q != nullptr);
    }
}

}  // namespace bgk
