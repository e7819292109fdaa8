// Beam search (biogpt_hip_generate_beam_batch; biogpt_hip_generate_beam is the call with one prompt): the selection of a beam step on the
// device, inside the captured step.  G independent searches of B beams run as one batched decode of G * B columns (one column and one K / V
// cache slot per beam).  Group g owns the columns and cache slots [g * B, (g + 1) * B) and one BeamCtl of an array of G; what a group's
// kernels touch is its own slice of every array, so the bodies below are written for one search and take the slice.  After the forward pass:
//
//   beam_group_rows_kernel    one workgroup per column (row of logits_all): the passes of logprob_rows_kernel (row maximum m,
//                             S = sum exp(l - m)) and the row's top K = 2B (logit, id), equal logits: lower id first (the order, the walk and the
//                             bound: kernels_rows.hip.h, DESIGN.md "Row kernels").  Writes K candidates
//                             {s_b + lp, column within the group, id} with lp = (l - m) - log(S) (double arithmetic, rounded once), s_b + lp
//                             in f32.  A finished group's rows and, at a group's first step, every row but its first return at once (the
//                             other beams have no score yet).  GIVEN: the row holds processed log-probabilities (generation rules).
//   beam_group_select_kernel  one workgroup per group: the top 2B of all candidates (score descending, parent rank ascending, id ascending),
//                             the next running beams, the finished pool and the stopping rules of transformers' _beam_search
//                             (INTEGRATION.md), the new column states and the group's forks.  Children are assigned to columns so that the
//                             column -> cache mapping stays the identity: the first child of a parent keeps the parent's column, further
//                             children take the columns of parents without children.  Fork sources and destinations are then disjoint
//                             sets.  The forks (column base added) are appended to ONE compacted list; the kernel also writes the
//                             per-column skip words of the rules kernel and counts the unfinished groups down.
//   kv_group_fork_kernel      grid (n_layer * n_head, BEAM_FORK_WGS, 2): for each fork, K and V rows [lo, hi) of every layer and head from
//                             the source slot to the destination slot (head-major cache: one contiguous run per (layer, head)), plus the
//                             token history.  The workgroups of a (layer, head, K | V) stride over the compacted list: the grid is fixed
//                             (capturable) and does not grow with G * (B - 1).
//
// Every slot of a group holds its prompt's rows before the first step (kv_share_kernel), so a fork copies generated rows only.  A finished
// group leaves everything alone: its columns keep token and position and recompute a K / V row they already hold.  Nothing here leaves the
// device; the host only reads the count of unfinished groups between groups of steps and the pools at the end.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.hip.h"
#include "kernels_score.hip.h"

namespace bgk {

constexpr int BEAM_MAX = 16;                   // beams per call; 2 * BEAM_MAX candidates per row
constexpr int BEAM_SELECT_THREADS = BEAM_MAX * 2 * BEAM_MAX;   // one thread per candidate of a full step
constexpr int BEAM_FORK_WGS = 8;               // copy workgroups per (layer, head, K | V), striding over the step's fork list

struct BeamCand {
    float score;    // accumulated log-probability, f32
    int32_t col;    // parent's column
    int32_t id;     // token
    int32_t pad;
};

// Device state of one search (group).  The first block is uploaded by the host per call; the rest is the kernels' own.
struct BeamCtl {
    int32_t n_beams, n_prompt, n_predict, eos_id;   // eos_id < 0: none
    float length_penalty;
    int32_t early_stopping;
    int32_t ids_stride;                             // words between two pool rows of pool_ids
    int32_t pad0;
    // running state
    int32_t done;          // set once the search has stopped: later steps change nothing
    int32_t step;          // tokens generated so far
    int32_t pool_n;        // finished hypotheses held (<= n_beams)
    int32_t heur_unsat;    // transformers' is_early_stop_heuristic_unsatisfied
    float run_score[BEAM_MAX];     // per column: accumulated score of the beam in it
    int32_t col_rank[BEAM_MAX];    // per column: that beam's rank among the running beams
    int32_t pool_order[BEAM_MAX];  // pool slots, best first
    int32_t pool_len[BEAM_MAX];    // per slot: generated tokens (EOS included)
    float pool_score[BEAM_MAX];    // per slot: normalized score
    int32_t fork_n, fork_hi, fork_gen;              // forks of the last step; rows [n_prompt, fork_hi) of K / V, fork_gen tokens of history
    int32_t fork_src[BEAM_MAX], fork_dst[BEAM_MAX];
};

// what the groups of a call share
struct BeamBatchHdr {
    int32_t n_live;        // groups still searching
    int32_t fork_n;        // entries of the fork list of this step (reset by the row kernel of the next)
    int32_t pad[2];
};

struct BeamFork {
    int32_t src, dst;      // cache slots (= columns)
    int32_t lo, hi;        // K / V rows [lo, hi)
    int32_t gen;           // tokens of history
    int32_t pad[3];
};

// insert (v, i) into the descending list (tv, ti): compile-time indices only, the list stays in registers
template <int KM>
__device__ __forceinline__ void beam_insert(float v, int i, float (&tv)[KM], int (&ti)[KM]) {
    if (!row_before(v, i, tv[KM - 1], ti[KM - 1])) return;
#pragma unroll
    for (int j = 0; j < KM; j++) {
        const bool b = row_before(v, i, tv[j], ti[j]);
        const float of = tv[j];
        const int oi = ti[j];
        tv[j] = b ? v : of; ti[j] = b ? i : oi;
        v = b ? of : v; i = b ? oi : i;
    }
}

// The body of beam_group_rows_kernel.  GIVEN = false: the row holds logits (the log-softmax is taken here).  GIVEN = true: it holds log-probabilities
// already, processed by rules_rows_kernel (kernels_rules.hip.h), and its values are taken as they are (an entry at -inf becomes a candidate only
// where fewer than K finite ones are left, which the argument check of the rules excludes).
// row: the row's n_vocab values; run_score: the accumulated score of the beam in this row; col: the column the candidates name as their parent;
// cand: the row's K candidates.
template <int KM, bool GIVEN>
__device__ __forceinline__ void beam_rows_body(const float *row, int n_vocab, const float *run_score, int col, int K, BeamCand *cand) {
    __shared__ float w_v[LP_THREADS / 64][KM];
    __shared__ int w_i[LP_THREADS / 64][KM];
    __shared__ double s_ls;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    float m = 0.0f;
    if constexpr (!GIVEN) {
        int bi;
        double S;
        lp_row_stats(row, n_vocab, m, bi, S);
        if (tid == 0) s_ls = log(S);
    }

    // this thread's top KM over its elements: the bound first (row_kth_bound, kernels_rows.hip.h), then the insertions of the few elements at or above it
    float tv[KM];
    int ti[KM];
#pragma unroll
    for (int j = 0; j < KM; j++) { tv[j] = ROW_NONE_V; ti[j] = ROW_NONE_I; }
    float mv = ROW_NONE_V, thr_v;
    int mi = ROW_NONE_I, thr_i;
    constexpr int DEPTH = 2;      // measured beside the KM-entry register lists (profiles/rows_kernels_ab.txt): <32, true> 80.6 us with two loads in flight, 88.5 with one
    row_scan<LP_THREADS, DEPTH>(row, n_vocab, [&](float v, int i) { row_keep(v, i, mv, mi); });
    row_kth_bound<LP_THREADS>(mv, mi, K, thr_v, thr_i);
    row_scan<LP_THREADS, DEPTH>(row, n_vocab, [&](float v, int i) { if (!row_before(thr_v, thr_i, v, i)) beam_insert<KM>(v, i, tv, ti); });

    // per wave: K rounds of a wave arg-max over the lanes' list heads; the winner pops its head (ids are unique)
    for (int r = 0; r < K; r++) {
        float bv = tv[0];
        int bidx = ti[0];
        for (int off = 32; off > 0; off >>= 1) {
            const float ov = __shfl_xor(bv, off, 64);
            const int oi = __shfl_xor(bidx, off, 64);
            row_keep(ov, oi, bv, bidx);
        }
        if (bidx != ROW_NONE_I && ti[0] == bidx) {
#pragma unroll
            for (int j = 0; j + 1 < KM; j++) { tv[j] = tv[j + 1]; ti[j] = ti[j + 1]; }
            tv[KM - 1] = ROW_NONE_V; ti[KM - 1] = ROW_NONE_I;
        }
        if (lane == 0) { w_v[wv][r] = bv; w_i[wv][r] = bidx; }
    }
    __syncthreads();
    // the four wave lists -> the row's top K: each entry finds its rank among all of them
    const int n_ent = (LP_THREADS / 64) * K;
    if (tid < n_ent) {
        const int ew = tid / K, er = tid - ew * K;
        const float v = w_v[ew][er];
        const int id = w_i[ew][er];
        if (id != ROW_NONE_I) {
            int rank = 0;
            for (int w = 0; w < LP_THREADS / 64; w++)
                for (int r = 0; r < K; r++) rank += row_before(w_v[w][r], w_i[w][r], v, id) ? 1 : 0;
            if (rank < K) {
                float lp = v;
                if constexpr (!GIVEN) lp = (float)(((double)v - (double)m) - s_ls);
                BeamCand c;
                c.score = *run_score + lp;
                c.col = col; c.id = id; c.pad = 0;
                cand[rank] = c;
            }
        }
    }
}

// logits: [G * B][ldl] (row r = column r); ctl: [G]; cand: [G * B][2 * B].  KM >= 2 * B.
template <int KM, bool GIVEN>
__global__ __launch_bounds__(LP_THREADS) void beam_group_rows_kernel(const float *logits, int ldl, int n_vocab, const BeamCtl *ctl, int B, BeamBatchHdr *hdr,
                                                                     BeamCand *cand) {
    const int col = blockIdx.x, g = col / B, j = col - g * B;
    if (col == 0 && threadIdx.x == 0) hdr->fork_n = 0;      // the copies of the step before are done (stream order)
    const BeamCtl *c = ctl + g;
    if (c->done || (c->step == 0 && j > 0)) return;         // (a group's first step expands its first row alone)
    beam_rows_body<KM, GIVEN>(logits + (size_t)col * ldl, n_vocab, &c->run_score[j], j, 2 * B, cand + (size_t)col * 2 * B);
}

// candidate order of a step: score descending, then the parent's rank, then the token id
__device__ __forceinline__ bool cand_before(const BeamCand &a, int ra, const BeamCand &b, int rb) {
    if (a.score != b.score) return a.score > b.score;
    if (ra != rb) return ra < rb;
    return a.id < b.id;
}

__device__ __forceinline__ float beam_norm(float s, int gen_len, float lp) { return (float)((double)s / pow((double)gen_len, (double)lp)); }

// n_rows beam rows (1 at the first step, n_beams after) of K = 2 * n_beams candidates each.  seq: the n_beams column states;
// seq_gen: [column][gen_stride] token histories; pool_ids: [slot][ctl->ids_stride].
// The search's part of beam_group_select_kernel; false: the search had stopped before this step and nothing was touched (uniform over the workgroup).
__device__ __forceinline__ bool beam_select_body(const BeamCand *cand, int n_rows, BeamCtl *ctl, SeqState *seq, int32_t *seq_gen, int gen_stride,
                                                 int32_t *pool_ids) {
    __shared__ BeamCand s_c[2 * BEAM_MAX];
    __shared__ int s_pend[BEAM_MAX];     // per pool slot: the candidate whose ids it takes in this step, -1 none
    __shared__ int s_run[BEAM_MAX], s_dest[BEAM_MAX], s_taken[BEAM_MAX];   // thread 0's lists (LDS: no scratch)
    __shared__ int s_k;
    const int tid = threadIdx.x;
    if (ctl->done) return false;
    const int B = ctl->n_beams, K = 2 * B, n = n_rows * K;
    if (tid < n) {   // rank of this candidate among all of them (a total order: (column, id) pairs are unique)
        const BeamCand c = cand[tid];
        const int rc = ctl->col_rank[c.col];
        int rank = 0;
        for (int j = 0; j < n; j++) {
            const BeamCand o = cand[j];
            rank += cand_before(o, ctl->col_rank[o.col], c, rc) ? 1 : 0;
        }
        if (rank < K) s_c[rank] = c;
    }
    if (tid < BEAM_MAX) s_pend[tid] = -1;
    __syncthreads();
    if (tid == 0) {
        const int k = ctl->step + 1;             // generated tokens, this step's included
        const float lpen = ctl->length_penalty;
        const int eos = ctl->eos_id;
        auto hit = [&](int i) { return (eos >= 0 && s_c[i].id == eos) || k >= ctl->n_predict; };
        // the next running beams: the first B candidates that do not stop
        int *const run = s_run;
        int nr = 0;
        for (int i = 0; i < K && nr < B; i++)
            if (!hit(i)) run[nr++] = i;
        // the finished pool (_update_finished_beams): candidates among the first B that stop, unless the pool is full under
        // early_stopping or the heuristic has tripped; best B by normalized score, earlier entries first on ties
        int pool_n = ctl->pool_n;
        if (!(pool_n == B && ctl->early_stopping) && ctl->heur_unsat) {
            for (int i = 0; i < B; i++) {
                if (!hit(i)) continue;
                const float sc = beam_norm(s_c[i].score, k, lpen);
                int pos = 0;
                while (pos < pool_n && ctl->pool_score[ctl->pool_order[pos]] >= sc) pos++;
                if (pos >= B) continue;
                int slot;
                if (pool_n < B) {
                    slot = pool_n;
                    for (int j = pool_n; j > pos; j--) ctl->pool_order[j] = ctl->pool_order[j - 1];
                    pool_n++;
                } else {
                    slot = ctl->pool_order[B - 1];   // the worst entry leaves
                    for (int j = B - 1; j > pos; j--) ctl->pool_order[j] = ctl->pool_order[j - 1];
                }
                ctl->pool_order[pos] = slot;
                ctl->pool_score[slot] = sc;
                ctl->pool_len[slot] = k;
                s_pend[slot] = i;
            }
            ctl->pool_n = pool_n;
        }
        // _check_early_stop_heuristic: only a full pool can trip it
        if (ctl->heur_unsat && pool_n == B && nr > 0)
            ctl->heur_unsat = beam_norm(s_c[run[0]].score, k, lpen) > ctl->pool_score[ctl->pool_order[B - 1]] ? 1 : 0;
        const int done = (!ctl->heur_unsat || (pool_n == B && ctl->early_stopping) || nr < B || k >= ctl->n_predict) ? 1 : 0;
        // columns: the first child of a parent stays in its column, further children take the columns of parents without children
        int *const taken = s_taken, *const dest = s_dest;
        for (int c = 0; c < BEAM_MAX; c++) taken[c] = 0;
        for (int r = 0; r < nr; r++) {
            const int p = s_c[run[r]].col;
            dest[r] = taken[p] ? -1 : p;
            taken[p] = 1;
        }
        int nf = 0, free_c = 0;
        for (int r = 0; r < nr; r++) {
            if (dest[r] >= 0) continue;
            while (taken[free_c]) free_c++;
            taken[free_c] = 1;
            dest[r] = free_c;
            ctl->fork_src[nf] = s_c[run[r]].col; ctl->fork_dst[nf] = free_c; nf++;
        }
        const int n_past = ctl->n_prompt - 1 + k;    // the position of the token each beam evaluates next
        for (int r = 0; r < nr; r++) {
            const int c = dest[r];
            ctl->run_score[c] = s_c[run[r]].score;
            ctl->col_rank[c] = r;
            SeqState &s = seq[c];
            s.token = s_c[run[r]].id;
            s.n_past = n_past;
            s.n_gen = k;
            seq_gen[(size_t)c * gen_stride + (k - 1)] = s_c[run[r]].id;
        }
        ctl->fork_n = nf;
        ctl->fork_hi = n_past;
        ctl->fork_gen = k - 1;
        ctl->step = k;
        ctl->done = done;
        s_k = k;
    }
    __syncthreads();
    // ids of the hypotheses that entered the pool: the parent's history, then the candidate's token
    const int k = s_k;
    for (int slot = 0; slot < B; slot++) {
        const int i = s_pend[slot];
        if (i < 0) continue;
        const int32_t *src = seq_gen + (size_t)s_c[i].col * gen_stride;
        int32_t *dst = pool_ids + (size_t)slot * ctl->ids_stride;
        for (int j = tid; j < k; j += blockDim.x) dst[j] = j + 1 < k ? src[j] : s_c[i].id;
    }
    return true;
}

// grid: G.  seq, seq_gen, col_skip: all G * B columns; pool_ids: [G * B][ctl->ids_stride]; forks: room for G * (B - 1) entries.
__global__ __launch_bounds__(BEAM_SELECT_THREADS) void beam_group_select_kernel(const BeamCand *cand, BeamCtl *ctl, int B, SeqState *seq, int32_t *seq_gen,
                                                                                int gen_stride, int32_t *pool_ids, BeamBatchHdr *hdr, BeamFork *forks,
                                                                                int32_t *col_skip) {
    const int g = blockIdx.x, base = g * B;
    BeamCtl *c = ctl + g;
    const int n_rows = c->step == 0 ? 1 : B;
    if (!beam_select_body(cand + (size_t)base * 2 * B, n_rows, c, seq + base, seq_gen + (size_t)base * gen_stride, gen_stride,
                          pool_ids + (size_t)base * c->ids_stride))
        return;
    if (threadIdx.x != 0) return;
    const int done = c->done;
    if (done) atomicSub(&hdr->n_live, 1);
    // every slot of the group holds the prompt's rows already (kv_share_kernel before the first step, then the step's own row): a fork
    // copies the generated rows only
    const int lo = c->n_prompt, hi = c->fork_hi, gen = c->fork_gen, nf = c->fork_n;
    if (!done && nf > 0 && (hi > lo || gen > 0)) {
        const int at = atomicAdd(&hdr->fork_n, nf);
        for (int f = 0; f < nf; f++) {
            BeamFork k;
            k.src = base + c->fork_src[f]; k.dst = base + c->fork_dst[f]; k.lo = lo; k.hi = hi; k.gen = gen;
            k.pad[0] = k.pad[1] = k.pad[2] = 0;
            forks[at + f] = k;
        }
    }
    for (int j = 0; j < B; j++) col_skip[base + j] = done;
}

// grid (n_layer * n_head, BEAM_FORK_WGS, 2 [K, V]); seq_stride floats between two slots, P * dk between two heads
__global__ __launch_bounds__(256) void kv_group_fork_kernel(const BeamBatchHdr *hdr, const BeamFork *forks, float *kroot, float *vroot, int64_t seq_stride,
                                                            int P, int dk, int32_t *seq_gen, int gen_stride) {
    const int n = hdr->fork_n;
    const size_t run0 = (size_t)blockIdx.x * P * dk;    // (layer, head) run; layers are n_head runs apart
    float *root = blockIdx.z == 0 ? kroot : vroot;
    for (int f = blockIdx.y; f < n; f += gridDim.y) {
        const BeamFork k = forks[f];
        const float4 *s4 = reinterpret_cast<const float4 *>(root + (size_t)k.src * seq_stride + run0 + (size_t)k.lo * dk);
        float4 *d4 = reinterpret_cast<float4 *>(root + (size_t)k.dst * seq_stride + run0 + (size_t)k.lo * dk);
        const int n4 = k.hi > k.lo ? (k.hi - k.lo) * dk / 4 : 0;
        for (int i = threadIdx.x; i < n4; i += blockDim.x) d4[i] = s4[i];
        if (blockIdx.x == 0 && blockIdx.z == 0)
            for (int j = threadIdx.x; j < k.gen; j += blockDim.x) seq_gen[(size_t)k.dst * gen_stride + j] = seq_gen[(size_t)k.src * gen_stride + j];
    }
}

// ---- the model of biogpt_hip_beam_table_device (tests of the three kernels above without a forward pass) ----
// What a decode step leaves for column c with token t at position p: its logits row, here row t % n_table_rows of a table, and its K / V row of
// position p in its own cache slot, here a stamp that names (token, position, head, K | V) in exact floats.  1 layer, TABLE_HEADS heads of TABLE_DK.
constexpr int TABLE_HEADS = 2, TABLE_DK = 4;

__device__ __forceinline__ float4 beam_table_stamp(int token, int pos, int head, int kv) {
    return make_float4((float)token, (float)pos, (float)(2 * head + kv), (float)((token + 7 * pos + 3 * head + kv) & 0xffff));
}

// grid: the columns.  table: [n_table_rows][n_vocab]; logits: [columns][n_vocab]; kroot / vroot: [columns][TABLE_HEADS][P][TABLE_DK].
__global__ __launch_bounds__(256) void beam_table_feed_kernel(const SeqState *seq, const float *table, int n_table_rows, int n_vocab, float *logits, float *kroot,
                                                              float *vroot, int P) {
    const int col = blockIdx.x;
    const SeqState s = seq[col];
    if (s.token < 0 || s.n_past < 0 || s.n_past >= P) return;      // (never: the select kernel's positions end at n_prompt - 1 + n_predict < P)
    const float *src = table + (size_t)(s.token % n_table_rows) * n_vocab;
    float *dst = logits + (size_t)col * n_vocab;
    for (int i = threadIdx.x; i < n_vocab; i += blockDim.x) dst[i] = src[i];
    if (threadIdx.x < 2 * TABLE_HEADS) {
        const int head = threadIdx.x >> 1, kv = threadIdx.x & 1;
        float *root = kv ? vroot : kroot;
        *reinterpret_cast<float4 *>(root + (((size_t)col * TABLE_HEADS + head) * P + s.n_past) * TABLE_DK) = beam_table_stamp(s.token, s.n_past, head, kv);
    }
}

}  // namespace bgk
