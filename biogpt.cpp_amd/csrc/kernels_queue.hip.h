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
// SampleCtl / SampleSeq live in a buffer of the queue's own: the captured steps of biogpt_hip_generate_sample keep their pointers.  Both kernels write
// plain vector stores and atomicAdd / atomicSub only.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.hip.h"
#include "kernels_genlp.hip.h"
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

// grid (admitted columns), QUEUE_ADMIT_THREADS threads; list: [gridDim.x]
__global__ __launch_bounds__(QUEUE_ADMIT_THREADS) void queue_admit_kernel(const QueueAdmit *list, SampleSeq *sq, SeqState *seq, int32_t *limit, QueueHdr *hdr) {
    __shared__ uint32_t mt[MT_N + 1];
    const QueueAdmit a = list[blockIdx.x];
    if (a.col < 0 || a.col >= QUEUE_COLS) return;      // (uniform)
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

}  // namespace bgk
