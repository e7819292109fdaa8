// Generation over a queue (biogpt_hip_generate_queue, biogpt_hip_generate_queue_prefix): a fixed set of columns, each with its own K / V cache slot, kept busy from a queue of requests.
// A step is the batched decode of the columns (one column and one slot per running request), then:
//
//   queue_rows_kernel    one workgroup per column: the step of sample_rows_kernel as it is (sample_rows_step<SamplePlain>, kernels_sample.hip.h), then
//                        thread 0 holds the column's generated length against the column's OWN limit: a column at its limit is finished exactly as one
//                        that drew the EOS id.  A column that finishes, either way, reports itself in the header the host reads behind a group of
//                        steps: fin[col] = 1, len[col] = its generated length, n_live one less.  A finished column keeps its token and position (it
//                        recomputes the K / V row it has) until the host refills it.
//   queue_rows_lp_kernel the same with sample_rows_step<SampleGenLp> (kernels_genlp.hip.h): entry n_gen of the column's row of the log-probability block
//                        beside the id.  The limit / report tail is one function of both (queue_report).
//   queue_admit_kernel   one workgroup per column the host refills, from a small uploaded list: the column's state at its prompt's LAST token (the
//                        first step re-evaluates it, as in every column call), its generator std::mt19937(seed) with the first block of outputs made
//                        (mt_seed, mt_regenerate: the text a closed call runs on the host), its limit; the header's entry cleared, n_live one more.
//                        Behind a shared prefix the record names the shared rows and their slot (SeqState::pad[0] / pad[1], what the decode steps
//                        behind a prefix read); the plain queue passes zeros.
//
//   queue_req_rows_kernel<Extra>   the step of a queue whose requests carry their own parameters (biogpt_hip_generate_queue_requests): one workgroup per
//                        column, one launch per step.  A column's record (QueueReqRec) holds its sampler, its EOS id, its rules and its stop sequences:
//                        the rules on the column's logits row in place (rules_apply_row, kernels_rules.hip.h -- the function rules_rows_kernel runs; skipped
//                        where the record has none), sample_rows_step with the record's SampleCtl, then by thread 0 the stop check on the token just
//                        appended -- the last len_i entries of the column's seq_gen row against each stop sequence, only where n_gen >= len_i, so a match
//                        never reaches into the prompt -- and queue_report.  The reason a column finished (QueueReqHdr::reason: 0 limit, 1 EOS, 2 + i stop
//                        sequence i) travels in the header behind QueueHdr.  The history the rules read is the call's prefix (one copy), the column's own
//                        prompt tokens (hist, one row per column) and its seq_gen row.
//   queue_req_admit_kernel   queue_admit_kernel's work (queue_admit_column, one function of both) and the column's record and prompt tokens, copied from the
//                        uploaded admit list: a refilled column inherits nothing from its predecessor.
//
// SampleCtl / SampleSeq live in a buffer of the queue's own: the captured steps of biogpt_hip_generate_sample keep their pointers.  Both kernels write
// plain vector stores and atomicAdd / atomicSub only.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.hip.h"
#include "kernels_genlp.hip.h"
#include "kernels_rules.hip.h"
#include "kernels_sample.hip.h"

namespace bgk {

constexpr int QUEUE_COLS = 512;           // columns of a call, at most
constexpr int QUEUE_ADMIT_THREADS = 64;

// what travels to the host behind every group of steps
struct QueueHdr {
    int32_t n_live, pad[3];
    int32_t fin[QUEUE_COLS];      // the column has finished (EOS or limit) and was not refilled yet
    int32_t len[QUEUE_COLS];      // ... with this many generated tokens
};

// one refilled column
struct QueueAdmit {
    int32_t col, last_token, len, limit;
    uint32_t seed;
    int32_t n_shared, shared_slot;      // the first n_shared K / V rows lie in slot shared_slot (0, 0: every row is the column's own)
    int32_t pad;
};
static_assert(sizeof(QueueAdmit) == 32, "the admit record keeps its size");

// Behind the step of column col, by thread 0 (it wrote the state it reads here): the column's generated length against its own limit, and the report of a
// column that has finished either way.
__device__ __forceinline__ void queue_report(int col, SampleSeq *sq, const SeqState *seq, const int32_t *limit, QueueHdr *hdr) {
    const int n_gen = seq[col].n_gen;
    int fin = sq[col].finished;
    if (!fin && n_gen >= limit[col]) { sq[col].finished = 1; fin = 1; }
    if (fin) {
        hdr->len[col] = n_gen;
        hdr->fin[col] = 1;
        atomicSub(&hdr->n_live, 1);
    }
}

// grid (columns); logits: [columns][ldl]; limit: [QUEUE_COLS] tokens a column's request may generate
__global__ __launch_bounds__(SAMPLE_THREADS) void queue_rows_kernel(const float *logits, int ldl, int n_vocab, SampleCtl *ctl, SampleSeq *sq, SeqState *seq,
                                                                    int32_t *seq_gen, int gen_stride, const int32_t *limit, QueueHdr *hdr) {
    const int col = blockIdx.x;
    if (col >= QUEUE_COLS || sq[col].finished) return;      // (uniform) a finished column was reported when it finished
    sample_rows_step(logits, ldl, n_vocab, ctl, sq, seq, seq_gen, gen_stride, SamplePlain());
    if (threadIdx.x == 0) queue_report(col, sq, seq, limit, hdr);
}

// the same, and entry n_gen of row col of out (the column's request starts at entry 0: queue_admit_kernel sets n_gen = 0)
__global__ __launch_bounds__(SAMPLE_THREADS) void queue_rows_lp_kernel(const float *logits, int ldl, int n_vocab, SampleCtl *ctl, SampleSeq *sq, SeqState *seq,
                                                                       int32_t *seq_gen, int gen_stride, const int32_t *limit, QueueHdr *hdr, GenLpOut out) {
    const int col = blockIdx.x;
    if (col >= QUEUE_COLS || sq[col].finished) return;      // (uniform) a finished column writes nothing
    sample_rows_step(logits, ldl, n_vocab, ctl, sq, seq, seq_gen, gen_stride, SampleGenLp{out});
    if (threadIdx.x == 0) queue_report(col, sq, seq, limit, hdr);
}

// One admitted column, by the QUEUE_ADMIT_THREADS threads of a workgroup; mt: MT_N + 1 words of LDS
__device__ __forceinline__ void queue_admit_column(const QueueAdmit &a, uint32_t *mt, SampleSeq *sq, SeqState *seq, int32_t *limit, QueueHdr *hdr) {
    if (threadIdx.x == 0) { mt_seed(a.seed, mt); mt_regenerate(mt); }
    __syncthreads();
    for (int i = threadIdx.x; i <= MT_N; i += QUEUE_ADMIT_THREADS) sq[a.col].mt[i] = mt[i];
    if (threadIdx.x == 0) {
        SeqState st{};
        st.n_past = a.len - 1; st.token = a.last_token; st.n_gen = 0; st.seq_id = a.col;
        st.pad[0] = a.n_shared; st.pad[1] = a.shared_slot;
        seq[a.col] = st;
        sq[a.col].finished = 0;
        limit[a.col] = a.limit;
        hdr->fin[a.col] = 0;
        hdr->len[a.col] = 0;
        atomicAdd(&hdr->n_live, 1);
    }
}

// grid (admitted columns), QUEUE_ADMIT_THREADS threads; list: [gridDim.x]
__global__ __launch_bounds__(QUEUE_ADMIT_THREADS) void queue_admit_kernel(const QueueAdmit *list, SampleSeq *sq, SeqState *seq, int32_t *limit, QueueHdr *hdr) {
    __shared__ uint32_t mt[MT_N + 1];
    const QueueAdmit a = list[blockIdx.x];
    if (a.col < 0 || a.col >= QUEUE_COLS) return;      // (uniform)
    queue_admit_column(a, mt, sq, seq, limit, hdr);
}

// ---- requests with their own parameters (biogpt_hip_generate_queue_requests) ----------------------------------------------------------------------------
constexpr int QUEUE_REQ_SUPPRESS = 64;      // suppress ids of a request
constexpr int QUEUE_REQ_STOPS = 4;          // stop sequences of a request
constexpr int QUEUE_REQ_STOP_LEN = 8;       // ... of this many ids each, at most

// a column's request: what the step reads instead of the call's one SampleCtl and RulesCtl
struct QueueReqRec {
    SampleCtl ctl;                          // the request's sampler and EOS id (n_live: a word sample_append counts down, read by nobody)
    float penalty;                          // the rules as RulesCtl holds them: 1.0 / 0 / 0 / 0 off
    int32_t ngram, min_new, n_suppress;
    int32_t rules_on;                       // one of the four is on: the step runs rules_apply_row
    int32_t n_prefix, n_own;                // the history in front of the generated tokens: n_prefix tokens of the call's prefix, then n_own of the column's hist row
    int32_t n_stop;
    int32_t stop_len[QUEUE_REQ_STOPS];
    int32_t stop[QUEUE_REQ_STOPS][QUEUE_REQ_STOP_LEN];
    int32_t suppress[QUEUE_REQ_SUPPRESS];
};
static_assert(sizeof(QueueReqRec) % 16 == 0, "records lie 16-byte aligned in the admit list");

// the header of this form: QueueHdr as the driver reads it, then why a finished column finished (0: its limit; 1: its EOS id; 2 + i: stop sequence i)
struct QueueReqHdr {
    QueueHdr q;
    int32_t reason[QUEUE_COLS];
};

// one entry of the admit list: the admit record, the request's record, then rec.n_own prompt tokens; entries lie `stride` bytes apart (a multiple of 16)
struct QueueReqAdmit {
    QueueAdmit a;
    QueueReqRec rec;
};

// The step of column blockIdx.x, by the SAMPLE_THREADS threads of its workgroup.  logits: [columns][ldl], a column's row is changed in place by its rules;
// rec: [QUEUE_COLS]; prefix_tok: the call's prefix (rec.n_prefix tokens of it are read); hist: [QUEUE_COLS][hist_stride] own prompt tokens; seen: the rules'
// bitmap, (n_vocab + 31) / 32 words of LDS
template <class Extra>
__device__ __forceinline__ void queue_req_rows_step(float *logits, int ldl, int n_vocab, QueueReqRec *rec, SampleSeq *sq, SeqState *seq, int32_t *seq_gen,
                                                    int gen_stride, const int32_t *limit, QueueReqHdr *hdr, const int32_t *prefix_tok, const int32_t *hist,
                                                    int hist_stride, uint32_t *seen, Extra extra) {
    const int col = blockIdx.x;
    if (col >= QUEUE_COLS || sq[col].finished) return;      // (uniform) a finished column was reported when it finished and writes nothing
    QueueReqRec *const me = rec + col;
    const int32_t *gen = seq_gen + (size_t)col * gen_stride;
    if (me->rules_on) {      // (uniform) most requests have none
        const int n_prefix = max(0, min(me->n_prefix, hist_stride)), n_prompt = n_prefix + max(0, min(me->n_own, hist_stride - n_prefix));
        const int32_t *own = hist + (size_t)col * hist_stride;
        const int n_gen = max(0, min(seq[col].n_gen, gen_stride));
        auto h = [&](int i) { return i < n_prefix ? prefix_tok[i] : i < n_prompt ? own[i - n_prefix] : gen[i - n_prompt]; };
        rules_apply_row<SAMPLE_THREADS>(logits + (size_t)col * ldl, n_vocab, seen, h, n_prompt + n_gen, n_gen, me->penalty, me->ngram, me->min_new, me->ctl.eos_id,
                                        max(0, min(me->n_suppress, QUEUE_REQ_SUPPRESS)), me->suppress);
        __syncthreads();      // the selection reads the row as the rules left it
    }
    sample_rows_step(logits, ldl, n_vocab, &me->ctl, sq, seq, seq_gen, gen_stride, extra);
    if (threadIdx.x == 0) {      // (it appended the token and wrote the state it reads here)
        int reason = sq[col].finished ? 1 : 0;      // an EOS comes first
        const int n_gen = max(0, min(seq[col].n_gen, gen_stride)), n_stop = max(0, min(me->n_stop, QUEUE_REQ_STOPS));
        for (int i = 0; i < n_stop && reason == 0; i++) {
            const int len = me->stop_len[i];
            if (len < 1 || len > QUEUE_REQ_STOP_LEN || n_gen < len) continue;
            bool same = true;
            for (int j = 0; j < len && same; j++) same = gen[n_gen - len + j] == me->stop[i][j];
            if (same) { sq[col].finished = 1; reason = 2 + i; }
        }
        queue_report(col, sq, seq, limit, &hdr->q);
        if (sq[col].finished) hdr->reason[col] = reason;
    }
}

// grid (columns), SAMPLE_THREADS threads, dynamic LDS: (n_vocab + 31) / 32 words.  Extra: SamplePlain, or SampleGenLp (entry n_gen of row col of its block
// beside the id, as queue_rows_lp_kernel)
template <class Extra>
__global__ __launch_bounds__(SAMPLE_THREADS) void queue_req_rows_kernel(float *logits, int ldl, int n_vocab, QueueReqRec *rec, SampleSeq *sq, SeqState *seq,
                                                                        int32_t *seq_gen, int gen_stride, const int32_t *limit, QueueReqHdr *hdr,
                                                                        const int32_t *prefix_tok, const int32_t *hist, int hist_stride, Extra extra) {
    extern __shared__ uint32_t queue_req_seen[];
    queue_req_rows_step(logits, ldl, n_vocab, rec, sq, seq, seq_gen, gen_stride, limit, hdr, prefix_tok, hist, hist_stride, queue_req_seen, extra);
}

// grid (admitted columns), QUEUE_ADMIT_THREADS threads; list: gridDim.x entries (QueueReqAdmit, then the tokens), `stride` bytes apart
__global__ __launch_bounds__(QUEUE_ADMIT_THREADS) void queue_req_admit_kernel(const uint8_t *list, int stride, SampleSeq *sq, SeqState *seq, int32_t *limit,
                                                                              QueueReqHdr *hdr, QueueReqRec *rec, int32_t *hist, int hist_stride) {
    __shared__ uint32_t mt[MT_N + 1];
    const QueueReqAdmit *e = reinterpret_cast<const QueueReqAdmit *>(list + (size_t)blockIdx.x * (size_t)stride);
    const QueueAdmit a = e->a;
    if (a.col < 0 || a.col >= QUEUE_COLS) return;      // (uniform)
    queue_admit_column(a, mt, sq, seq, limit, &hdr->q);
    const int32_t *src = reinterpret_cast<const int32_t *>(&e->rec);
    int32_t *dst = reinterpret_cast<int32_t *>(rec + a.col);
    for (int i = threadIdx.x; i < (int)(sizeof(QueueReqRec) / 4); i += QUEUE_ADMIT_THREADS) dst[i] = src[i];
    const int32_t *tok = reinterpret_cast<const int32_t *>(e + 1);
    const int n_own = max(0, min(min(e->rec.n_own, hist_stride), (stride - (int)sizeof(QueueReqAdmit)) / 4));
    for (int i = threadIdx.x; i < n_own; i += QUEUE_ADMIT_THREADS) hist[(size_t)a.col * hist_stride + i] = tok[i];
    if (threadIdx.x == 0) hdr->reason[a.col] = 0;
}

// ---- queue sessions (biogpt_hip_queue_open): what a look carries while steps run, and a way out of a running column --------------------------------------
// queue_stream_kernel   launched once behind a group of g steps of a streaming session.  Stateless: for column c it writes n_gen[c] (clamped to gen_stride) and
//                       the LAST w = min(g, n_gen[c]) entries of the column's seq_gen row into row c of a compact [C][g] block that lies behind the header and
//                       travels with it; the entries behind w read -1.  With log-probabilities the same window of the column's lp / top_ids / top_lp rows
//                       (0 / -1 / 0 behind w, and for an entry past the rows' stride, which genlp_write never wrote).  A column appends at most g tokens in g
//                       steps, so the window always holds what the host has not delivered yet -- the host knows how many tokens of a request it has
//                       delivered and takes the part beyond -- and a column refilled in between needs no reset.
// queue_cancel_kernel   one thread per entry of a small uploaded list of columns: a column that has not finished is finished in the words of queue_report
//                       (finished = 1, fin = 1, len = n_gen, n_live one less), so the step kernels return early on it from the next group on.  An entry out
//                       of range, or a column that has finished already, changes nothing; an entry named twice counts once (atomicExch on the flag).
constexpr int QUEUE_STREAM_THREADS = 64;

struct QueueStreamOut {
    int32_t *n_gen;       // [C]
    int32_t *ids;         // [C][g]
    float *lp;            // [C][g], or null: no log-probabilities
    int32_t *top_ids;     // [C][g][K]
    float *top_lp;        // [C][g][K]
};

// grid (C), QUEUE_STREAM_THREADS threads.  src_*: the log-probability block the selection writes, [columns][lp_stride] and [columns][lp_stride][K]
__global__ __launch_bounds__(QUEUE_STREAM_THREADS) void queue_stream_kernel(const SeqState *seq, const int32_t *seq_gen, int gen_stride, int C, int g, QueueStreamOut out,
                                                                            const float *src_lp, const int32_t *src_top_ids, const float *src_top_lp, int lp_stride,
                                                                            int K) {
    const int col = blockIdx.x;
    if (col >= C || col >= QUEUE_COLS || g < 1) return;      // (uniform)
    const int n = max(0, min(seq[col].n_gen, gen_stride)), w = min(g, n);
    if (threadIdx.x == 0) out.n_gen[col] = n;
    const int32_t *gen = seq_gen + (size_t)col * gen_stride;
    for (int j = threadIdx.x; j < g; j += QUEUE_STREAM_THREADS) out.ids[(size_t)col * g + j] = j < w ? gen[n - w + j] : -1;
    if (out.lp == nullptr) return;      // (uniform)
    for (int j = threadIdx.x; j < g; j += QUEUE_STREAM_THREADS) {
        const int e = n - w + j;
        const bool have = j < w && e < lp_stride;
        const size_t at = (size_t)col * lp_stride + (have ? e : 0), to = (size_t)col * g + j;
        out.lp[to] = have ? src_lp[at] : 0.0f;
        for (int t = 0; t < K; t++) {
            out.top_ids[to * K + t] = have ? src_top_ids[at * K + t] : -1;
            out.top_lp[to * K + t] = have ? src_top_lp[at * K + t] : 0.0f;
        }
    }
}

// grid (ceil(n / QUEUE_ADMIT_THREADS)), QUEUE_ADMIT_THREADS threads; cols: [n]
__global__ __launch_bounds__(QUEUE_ADMIT_THREADS) void queue_cancel_kernel(const int32_t *cols, int n, SampleSeq *sq, const SeqState *seq, QueueHdr *hdr) {
    const int i = blockIdx.x * QUEUE_ADMIT_THREADS + threadIdx.x;
    if (i >= n) return;
    const int col = cols[i];
    if (col < 0 || col >= QUEUE_COLS) return;
    if (atomicExch(&sq[col].finished, 1) != 0) return;      // finished already: it was reported then
    hdr->len[col] = seq[col].n_gen;
    hdr->fin[col] = 1;
    atomicSub(&hdr->n_live, 1);
}

}  // namespace bgk
