// Beam search over a queue (biogpt_hip_generate_beam_queue): S group slots of B columns each, every slot one search of kernels_beam.hip.h, kept busy from a
// queue of requests.  A step is the batched decode of the S * B columns, the three beam kernels as a closed call runs them (beam_group_rows,
// beam_group_select, kv_group_fork: unchanged, they touch their group's slice alone), then the report below.  Around the steps:
//
//   beam_slot_admit_kernel    one workgroup per slot the host refills, from a small uploaded list {slot, last_token, len, n_predict}: everything a closed
//                             call's start sets for that group and nothing of any other group --
//                               BeamCtl     every word: the call's n_beams, eos_id, length_penalty, early_stopping, ids_stride; the request's n_prompt and
//                                           n_predict; heur_unsat = 1; all else 0 (done, step, pool_n, run_score, col_rank, the pool lists, the forks);
//                               SeqState    of the B columns, at the prompt's LAST token: n_past = len - 1, n_gen = 0, seq_id = the column, all else 0;
//                               col_skip    0 for the group's first column, 1 for the others (the first step expands the first row alone);
//                               the report header's entry cleared, its n_live and BeamBatchHdr::n_live one more.
//                             pool_n = 0 hides the pool rows of the slot's last search; they are not cleared.
//   kv_share_slots_kernel     grid (n_layer * n_head, admitted * (B - 1), 2): kv_share_kernel for the admit list.  The prompt pass has filled the slot of the
//                             group's first column; rows [0, len - 1) go to the other B - 1 slots of that group only.  It reads the list alone, no state the
//                             admit kernel writes: either order is right.
//   beam_slot_report_kernel   one thread per slot, behind the select kernel of every step: a group whose done word is set and that was not reported yet
//                             writes fin[slot] = 1, steps[slot] = BeamCtl::step, n_live one less.  The host reads the header behind every group of steps.
//
// Plain vector stores and atomicAdd / atomicSub only.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "kernels.hip.h"
#include "kernels_beam.hip.h"

namespace bgk {

constexpr int BEAM_QUEUE_SLOTS = 512;          // group slots of a call, at most (n_beams = 1 at 512 columns)
constexpr int BEAM_QUEUE_ADMIT_THREADS = 64;   // >= BEAM_MAX: one thread per column of the group
constexpr int BEAM_QUEUE_REPORT_THREADS = 64;

// what travels to the host behind every group of steps
struct BeamQueueHdr {
    int32_t n_live, pad[3];
    int32_t fin[BEAM_QUEUE_SLOTS];        // the slot's search has stopped and the slot was not refilled yet
    int32_t steps[BEAM_QUEUE_SLOTS];      // ... after this many steps
};

// one refilled slot
struct BeamQueueAdmit {
    int32_t slot, last_token, len, n_predict;
};

// what every search of a call shares (beam_ctl_of's arguments beside the request's own)
struct BeamQueueCall {
    int32_t n_beams, eos_id;
    float length_penalty;
    int32_t early_stopping, ids_stride, n_slots;
};

// grid (admitted slots), BEAM_QUEUE_ADMIT_THREADS threads; list: [gridDim.x]; ctl: [n_slots]; seq, col_skip: [n_slots * n_beams]
__global__ __launch_bounds__(BEAM_QUEUE_ADMIT_THREADS) void beam_slot_admit_kernel(const BeamQueueAdmit *list, BeamQueueCall call, BeamCtl *ctl, SeqState *seq,
                                                                                    int32_t *col_skip, BeamBatchHdr *bhdr, BeamQueueHdr *hdr) {
    const BeamQueueAdmit a = list[blockIdx.x];
    const int B = call.n_beams, tid = threadIdx.x;
    if (a.slot < 0 || a.slot >= call.n_slots || a.slot >= BEAM_QUEUE_SLOTS || B < 1 || B > BEAM_MAX) return;      // (uniform)
    // the slot's BeamCtl word by word: beam_ctl_of's image (every word the host would upload, the running state at zero)
    int32_t *const w = reinterpret_cast<int32_t *>(ctl + a.slot);
    constexpr int n_words = (int)(sizeof(BeamCtl) / 4);
    for (int i = tid; i < n_words; i += BEAM_QUEUE_ADMIT_THREADS) {
        int32_t v = 0;
        switch (i * 4) {
            case offsetof(BeamCtl, n_beams): v = B; break;
            case offsetof(BeamCtl, n_prompt): v = a.len; break;
            case offsetof(BeamCtl, n_predict): v = a.n_predict; break;
            case offsetof(BeamCtl, eos_id): v = call.eos_id; break;
            case offsetof(BeamCtl, length_penalty): v = __float_as_int(call.length_penalty); break;
            case offsetof(BeamCtl, early_stopping): v = call.early_stopping; break;
            case offsetof(BeamCtl, ids_stride): v = call.ids_stride; break;
            case offsetof(BeamCtl, heur_unsat): v = 1; break;
            default: break;
        }
        w[i] = v;
    }
    if (tid < B) {
        const int col = a.slot * B + tid;
        SeqState st{};
        st.n_past = a.len - 1; st.token = a.last_token; st.n_gen = 0; st.seq_id = col;
        seq[col] = st;
        col_skip[col] = tid > 0 ? 1 : 0;
    }
    if (tid == 0) {
        hdr->fin[a.slot] = 0;
        hdr->steps[a.slot] = 0;
        atomicAdd(&hdr->n_live, 1);
        atomicAdd(&bhdr->n_live, 1);
    }
}

// grid (n_layer * n_head, admitted * (B - 1), 2 [K, V]), 256 threads; seq_stride floats between two slots, P * dk between two heads
__global__ __launch_bounds__(256) void kv_share_slots_kernel(const BeamQueueAdmit *list, int B, int n_slots, float *kroot, float *vroot, int64_t seq_stride, int P, int dk) {
    const int e = blockIdx.y / (B - 1), j = 1 + blockIdx.y % (B - 1);
    const BeamQueueAdmit a = list[e];
    if (a.slot < 0 || a.slot >= n_slots) return;      // (uniform)
    const int rows = min(a.len - 1, P);
    const size_t run0 = (size_t)blockIdx.x * P * dk;
    float *root = blockIdx.z == 0 ? kroot : vroot;
    const float4 *s4 = reinterpret_cast<const float4 *>(root + (size_t)a.slot * B * seq_stride + run0);
    float4 *d4 = reinterpret_cast<float4 *>(root + ((size_t)a.slot * B + j) * seq_stride + run0);
    const int n4 = rows > 0 ? rows * dk / 4 : 0;
    for (int i = threadIdx.x; i < n4; i += blockDim.x) d4[i] = s4[i];
}

// grid (ceil(n_slots / BEAM_QUEUE_REPORT_THREADS)); ctl: [n_slots]
__global__ __launch_bounds__(BEAM_QUEUE_REPORT_THREADS) void beam_slot_report_kernel(const BeamCtl *ctl, int n_slots, BeamQueueHdr *hdr) {
    const int slot = blockIdx.x * BEAM_QUEUE_REPORT_THREADS + threadIdx.x;
    if (slot >= n_slots || slot >= BEAM_QUEUE_SLOTS) return;
    if (!ctl[slot].done || hdr->fin[slot]) return;
    hdr->steps[slot] = ctl[slot].step;
    hdr->fin[slot] = 1;
    atomicSub(&hdr->n_live, 1);
}

}  // namespace bgk
