// MI355X-native BioGPT decoder engine: weight arena + repack, launch sequence, hipGraph capture,
// and the extern "C" entry points declared in include/biogpt_hip.h.
//
// Reference path replaced: biogpt_model_load (biogpt.cpp:27-453), biogpt_graph (:624-810),
// biogpt_eval (:812-847) and the greedy decode loop of examples/main/main.cpp:91-151.
//
// Device memory (sized for 288 GB of HBM3E, nothing is streamed or paged):
//   arena     all weights, repacked to the SoA block layout of kernels.hip.h, plus the two fp16
//             tables; ONE contiguous allocation so that a multi-GPU launcher can broadcast it with a
//             single RCCL collective
//   memory_k / memory_v   F32 [n_layer][n_positions][d_model], as biogpt.cpp:331-335 (F4)
//   scratch   x, x1, q, att [n_positions][d_model], h [n_positions][d_ff], logits
//   state     DevState + token ring (kernels read n_past / ids from HBM so the captured decode graph
//             advances itself)
#include <hip/hip_runtime.h>
#include <fcntl.h>
#include <sys/file.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <functional>
#include <memory>
#include <mutex>
#include <set>
#include <string>
#include <thread>
#include <vector>

#include "host_common.h"
#include "kernels.hip.h"
#include "kernels_fast.hip.h"
#include "kernels_assoc.hip.h"
#include "kernels_runs.hip.h"
#include "kernels_decode.hip.h"
#include "kernels_q8probe.hip.h"
#include "kernels_fdecode.hip.h"
#include "kernels_lmhead.hip.h"
#include "kernels_sweep.hip.h"
#include "kernels_xlong.hip.h"   // parameter blocks and layouts only: the pipelined kernels are instantiated in xpipe_tu.hip
#include "kernels_xcols.hip.h"   // (likewise: xcols_tu.hip)
#include "kernels_fpipe.hip.h"   // (likewise: fpipe_tu.hip)
#include "kernels_quant.hip.h"
#include "kernels_score.hip.h"
#include "kernels_embed.hip.h"
#include "kernels_beam.hip.h"
#include "kernels_sample.hip.h"
#include "kernels_wide_sample.hip.h"
#include "kernels_genlp.hip.h"
#include "kernels_rules.hip.h"
#include "kernels_trie.hip.h"
#include "kernels_contrast.hip.h"
#include "kernels_lookup.hip.h"
#include "kernels_queue.hip.h"
#include "kernels_beam_queue.hip.h"
#include "model_file.h"
#include "quant_host.h"
#include "trie_host.h"

using namespace bg;

#define HIP_TRY(ret, expr)                                                                  \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess) BG_FAIL(ret, "%s failed: %s", #expr, hipGetErrorString(e_));  \
    } while (0)

namespace {

constexpr size_t ALIGN = 256;
inline size_t align_up(size_t v) { return (v + ALIGN - 1) & ~(ALIGN - 1); }

// ---- arena plan -----------------------------------------------------------------------------------
struct MatSlot {  // offsets of one (possibly row-fused) matrix inside the arena
    int32_t type = 0;
    int64_t M = 0, K = 0;
    size_t qs = 0, sc = 0, qh = 0;
    size_t qs_bytes = 0, sc_bytes = 0, qh_bytes = 0;
    size_t xq = 0, xs = 0;      // offsets in the expanded row-tiled image of the MFMA kernels (ensure_tile_images; kernels_mfma.hip.h)
};

struct LayerSlots {
    MatSlot qkv, o, fc1, fc2;
    size_t qkv_b, o_b, ln0_w, ln0_b, ln1_w, ln1_b, fc1_b, fc2_b;
};

struct ArenaPlan {
    MatSlot lm_head, embed_tokens, embed_pos;
    size_t ln_w = 0, ln_b = 0, gelu_tab = 0, exp_tab = 0;
    std::vector<LayerSlots> layers;
    size_t total = 0;
};

size_t unit_bytes_qs(int32_t t, int64_t k) {  // bytes of the qs stream per row
    switch (t) {
        case T_F32: return (size_t)k * 4;
        case T_F16: return (size_t)k * 2;
        case T_Q8_0: return (size_t)(k / QK) * 32;
        default: return (size_t)(k / QK) * 16;
    }
}
size_t unit_bytes_sc(int32_t t, int64_t k) {
    switch (t) {
        case T_Q4_0: case T_Q5_0: case T_Q8_0: return (size_t)(k / QK) * 2;
        case T_Q4_1: case T_Q5_1: return (size_t)(k / QK) * 4;
        default: return 0;
    }
}
size_t unit_bytes_qh(int32_t t, int64_t k) { return (t == T_Q5_0 || t == T_Q5_1) ? (size_t)(k / QK) * 4 : 0; }

ArenaPlan plan_arena(const biogpt_hip_hparams &hp, int64_t pos_rows) {
    ArenaPlan pl;
    const int32_t wt = ftype_to_type(hp.ftype);
    const int64_t D = hp.d_model, F = hp.d_ff, V = hp.n_vocab;
    size_t off = 0;
    auto mat = [&](MatSlot &m, int64_t M, int64_t K) {
        m.type = wt; m.M = M; m.K = K;
        m.qs_bytes = unit_bytes_qs(wt, K) * (size_t)M;
        m.sc_bytes = unit_bytes_sc(wt, K) * (size_t)M;
        m.qh_bytes = unit_bytes_qh(wt, K) * (size_t)M;
        m.qs = off; off = align_up(off + m.qs_bytes);
        m.sc = off; off = align_up(off + m.sc_bytes);
        m.qh = off; off = align_up(off + m.qh_bytes);
    };
    auto vec = [&](size_t &slot, int64_t n) { slot = off; off = align_up(off + (size_t)n * 4); };
    mat(pl.embed_tokens, V, D);
    mat(pl.embed_pos, pos_rows, D);
    pl.layers.resize((size_t)hp.n_layer);
    for (auto &L : pl.layers) {
        vec(L.ln0_w, D); vec(L.ln0_b, D);
        mat(L.qkv, 3 * D, D); vec(L.qkv_b, 3 * D);
        mat(L.o, D, D); vec(L.o_b, D);
        vec(L.ln1_w, D); vec(L.ln1_b, D);
        mat(L.fc1, F, D); vec(L.fc1_b, F);
        mat(L.fc2, D, F); vec(L.fc2_b, D);
    }
    vec(pl.ln_w, D); vec(pl.ln_b, D);
    mat(pl.lm_head, V, D);
    pl.gelu_tab = off; off = align_up(off + 65536 * 2);
    pl.exp_tab = off; off = align_up(off + 65536 * 2);
    pl.total = off;
    return pl;
}

// ---- repack one tensor (file layout -> SoA device layout) into host staging buffers ---------------
void repack_rows(int32_t type, const uint8_t *src, int64_t rows, int64_t K, uint8_t *qs, uint8_t *sc, uint8_t *qh) {
    if (type == T_F32 || type == T_F16) {
        std::memcpy(qs, src, file_row_bytes(type, K) * (size_t)rows);
        return;
    }
    const size_t bb = file_block_bytes(type);
    const int64_t nblocks = rows * (K / QK);
    const unsigned nw = nblocks > (1 << 16) ? std::min(16u, std::max(1u, std::thread::hardware_concurrency())) : 1;
    std::vector<std::thread> pool;
    for (unsigned w = 0; w < nw; w++) {
        const int64_t b0 = nblocks * w / nw, b1 = nblocks * (w + 1) / nw;
        auto job = [=] {
            for (int64_t b = b0; b < b1; b++) {
                const uint8_t *p = src + (size_t)b * bb;
                switch (type) {
                    case T_Q4_0: std::memcpy(sc + b * 2, p, 2); std::memcpy(qs + b * 16, p + 2, 16); break;
                    case T_Q4_1: std::memcpy(sc + b * 4, p, 4); std::memcpy(qs + b * 16, p + 4, 16); break;
                    case T_Q5_0: std::memcpy(sc + b * 2, p, 2); std::memcpy(qh + b * 4, p + 2, 4); std::memcpy(qs + b * 16, p + 6, 16); break;
                    case T_Q5_1: std::memcpy(sc + b * 4, p, 4); std::memcpy(qh + b * 4, p + 4, 4); std::memcpy(qs + b * 16, p + 8, 16); break;
                    case T_Q8_0: std::memcpy(sc + b * 2, p, 2); std::memcpy(qs + b * 32, p + 2, 32); break;
                    default: break;
                }
            }
        };
        if (nw == 1) job(); else pool.emplace_back(job);
    }
    for (auto &t : pool) t.join();
}

inline float gelu_tanh_f32(float x) {  // ggml_gelu_f32 [SURVEY A.5]
    const float GELU_COEF_A = 0.044715f, SQRT_2_OVER_PI = 0.79788456080286535587989211986876f;
    return 0.5f * x * (1.0f + tanhf(SQRT_2_OVER_PI * x * (1.0f + GELU_COEF_A * x * x)));
}

// the fp16 GELU table, built the way ggml_init builds it [SURVEY A.5]: the loader's, and the probe's of single kernels (engine_probe.inc)
std::vector<uint16_t> gelu_table_f16() {
    std::vector<uint16_t> tg(65536);
    for (uint32_t i = 0; i < 65536; i++) tg[i] = f32_to_f16(gelu_tanh_f32(f16_to_f32((uint16_t)i)));
    return tg;
}

// the fp16 exp table of ggml_soft_max, built the same way: the loader's, and the attention probes' (engine_probe.inc)
std::vector<uint16_t> exp_table_f16() {
    std::vector<uint16_t> te(65536);
    for (uint32_t i = 0; i < 65536; i++) te[i] = f32_to_f16(expf(f16_to_f32((uint16_t)i)));
    return te;
}

int pow2ceil(int v) { int p = 1; while (p < v) p <<= 1; return p; }
int ilog2(int v) { int l = 0; while ((1 << l) < v) l++; return l; }

int env_int(const char *name, int dflt) {
    const char *s = std::getenv(name);
    return s ? std::atoi(s) : dflt;
}

}  // namespace

// Tuning / debugging switches.  Read from the environment ONCE, when a context is created (and again only on
// biogpt_hip_refresh_options): no getenv on any launch path.
struct EngineOptions {
    int dbg, prompt_cols, no_graph, causal, no_fused_decode, xpipe, xpipe_fault, xpipe_multi, xpipe_dual, xpipe_as_res, proc_lock, graph_contended, fault_stale, xcols,
        resident, resident_us, res_dbg, res_spec, no_fdec, lm_stream, hop_place, verbose, topk_blocks, fpipe, fpipe_stamps, fpipe_lead, fpipe_fault, prefix_attn, run_attn, float_chain, assoc, assoc_chain;
    void load() {
        auto get = [](const char *name, int dflt) { return env_int(name, dflt); };
        no_fdec = get("BIOGPT_HIP_NO_FDEC", 0);             // 1: float-weight decode mat-vecs on the generic kernel (A/B arm of kernels_fdecode.hip.h)
        dbg = get("BIOGPT_HIP_DBG", 0);
        prompt_cols = get("BIOGPT_HIP_PROMPT_COLS", 512);
        no_graph = get("BIOGPT_HIP_NO_GRAPH", 0);
        causal = get("BIOGPT_HIP_CAUSAL", 0);
        no_fused_decode = get("BIOGPT_HIP_NO_FUSED_DECODE", 0);
        resident = get("BIOGPT_HIP_RESIDENT", 1);           // biogpt_hip_eval with one token: the pipelined launch stays on the device and takes the next call's token from a pinned mailbox
        res_dbg = get("BIOGPT_HIP_RES_DBG", 0);              // measurement only (kernels_xpipe.hip.h XpParams::res_dbg)
        lm_stream = get("BIOGPT_HIP_LM_STREAM", 1);          // the stand-alone lm_head as lm_stream_kernel (0: matvec_fast_kernel<PRO_LN, EPI_LOGITS>)
        res_spec = get("BIOGPT_HIP_SPEC", 1);                // a resident launch may start the next token from its own arg-max (greedy callers; resident_eval)
        resident_us = get("BIOGPT_HIP_RESIDENT_US", 1000);   // ... for at most this long without a new token (the device is not shared meanwhile)
        hop_place = get("BIOGPT_HIP_HOP_PLACE", 1);        // the cross-XCD hand-off regions: 1 placed by a calibration launch (xpipe_place_hops), 0 first candidate, 2 the slower one (A/B)
        verbose = get("BIOGPT_HIP_VERBOSE", 0);
        topk_blocks = get("BIOGPT_HIP_TOPK_BLOCKS", 1);    // biogpt_hip_eval_topk behind a resident launch: select from the blocks whose maximum can hold a candidate (0: scan the whole row)
        xpipe_dual = get("BIOGPT_HIP_XPIPE_DUAL", 1);       // contexts of 257 .. 512 keys (multi-token launches, graph replays, resident launches): dec_xpipe_kernel with two workgroups per head (0: kernels_xlong.hip.h, as in round 3)
        fpipe_lead = get("BIOGPT_HIP_FPIPE_LEAD", -1);       // the persistent float launch: 64-clock units a polling wave lets pass between its own workgroup's publication and its first sweep (-1: 26 for F32 files, 16 for F16 -- the measured optima, profiles/fpipe_lead_scan_r6.txt)
        fpipe_fault = get("BIOGPT_HIP_FPIPE_FAULT", 0);     // test hook: the context's first persistent float launch never gets one workgroup's out_proj rows and drains with an error
        fpipe_stamps = get("BIOGPT_HIP_FPIPE_STAMPS", 0);   // diagnostics: the persistent launch records stage-border times of three workgroups (biogpt_hip_fpipe_stamps)
        fpipe = get("BIOGPT_HIP_FPIPE", 1);                 // single-token steps of F32 / F16 files as ONE persistent launch for all layers (kernels_fpipe.hip.h); 0: five launches per layer
        xcols = get("BIOGPT_HIP_XCOLS", 1);                 // evals of 2 .. 8 tokens (the reference's prompt chunks) as ONE persistent launch, one column per XCD (kernels_xcols.hip.h); 0: the launch chain of kernels_fast.hip.h
        xpipe_multi = get("BIOGPT_HIP_XPIPE_MULTI", 1);     // biogpt_hip_generate_greedy: all tokens of a context bucket in one pipelined launch
        xpipe_fault = get("BIOGPT_HIP_XPIPE_FAULT", 0);   // test hook: the first pipelined launch finds a 33rd workgroup on XCD 0 and drains
        xpipe = get("BIOGPT_HIP_XPIPE", 1);             // the XCD-pipelined single-launch decode step (kernels_xpipe.hip.h)
        graph_contended = get("BIOGPT_HIP_GRAPH_CONTENDED", 0);   // test switch: replay the five-launch eval graph even while ANOTHER context holds the pipeline slot (the arrangement of profiles/two_contexts_r4.txt)
        fault_stale = get("BIOGPT_HIP_FAULT_STALE", 0);           // test switch: every k-th replayed eval starts from the PREVIOUS mailbox slot (the stale-row symptom, injected)
        proc_lock = get("BIOGPT_HIP_PROC_LOCK", 1);               // one process per device drives the pipelined launches (engine_xpipe.inc, xpipe_process_lock)
        prefix_attn = get("BIOGPT_HIP_PREFIX_ATTN", -1);          // decode steps behind a shared prefix: -1 attn_prefix_kernel where it was measured faster (PREFIX_ATTN_MIN_*), 0 never, 1 always (A/B arms)
        run_attn = get("BIOGPT_HIP_RUN_ATTN", -1);                // the passes of biogpt_hip_score_continuations_batch (no other call looks at it): -1 attn_runs_kernel where it was measured faster (RUN_ATTN_MIN_*), 0 never, 1 in every pass of up to 1024 keys (A/B arms)
        float_chain = get("BIOGPT_HIP_FLOAT_CHAIN", 0);          // 1: a new context of an F32 / F16 file the float chain serves starts with it switched on (biogpt_hip_float_chain; kernels_fchain.hip.h)
        assoc_chain = get("BIOGPT_HIP_ASSOC_CHAIN", 0);            // 1: a new context of a file the SIMD association serves starts with the SIMD chain switched on (biogpt_hip_assoc_chain; kernels_schain.hip.h)
        assoc = get("BIOGPT_HIP_ASSOC", 0);                        // 1: a new context of a file the SIMD association serves starts in it (biogpt_hip_assoc; kernels_assoc.hip.h)
        xpipe_as_res = get("BIOGPT_HIP_XPIPE_AS_RES", 0);          // measurement only: ordinary pipelined launches through the RES instantiations (tests/test_gpu_resident.py)
    }
};

constexpr int GRAPH_BUCKETS = 6;      // the context buckets of a captured decode step: graph_bucket() is in [0, GRAPH_BUCKETS)

// The form of a step of column generation: everything but the call's shape and the context bucket that decides which launches the step is
struct StepForm {
    enum Selection { Plain, Rules, Trie, Wide, N_SELECTIONS };      // the mode's selection alone, rules or a trie in front of it, the whole-vocabulary sampler
    Selection sel = Plain;
    bool lp = false;          // the selection also writes log-probabilities (kernels_genlp.hip.h)
    bool shared = false;      // prefix rows are read in place (ForwardPass::decode_step_shared)
    bool xcols = false;       // the steps are column-per-XCD launches
};

// The captured steps of one mode of column generation, valid for the call shape (key_a, key_b) they were captured for -- sequences, or groups and beams.  A step
// is filed under its form and its context bucket; every combination of a form's fields has slots of its own, so no form replays another's step, whatever the
// modes' argument checks let through.  slot() alone knows the layout.
struct ColumnGraphs {
    static constexpr int N_SLOTS = StepForm::N_SELECTIONS * 2 * 2 * 2 * GRAPH_BUCKETS;
    hipGraphExec_t exec[N_SLOTS] = {};
    int key_a = 0, key_b = 0;
    static int slot(const StepForm &f, int bucket) { return ((((int)f.sel * 2 + (f.lp ? 1 : 0)) * 2 + (f.shared ? 1 : 0)) * 2 + (f.xcols ? 1 : 0)) * GRAPH_BUCKETS + bucket; }
};

// ---- context ----------------------------------------------------------------------------------------
struct biogpt_hip_ctx {
    EngineOptions opt{};
    biogpt_hip_hparams hp{};
    int device = 0;
    int n_tensors = 0;
    int64_t pos_rows = 0;
    std::vector<std::string> vocab, merges;
    biogpt_hip_vocab *tok_vocab = nullptr;   // token <-> id maps + merge ranks for the tokenizer entry points

    uint8_t *arena = nullptr;
    size_t arena_bytes = 0;
    bool owns_arena = false;
    ArenaPlan plan;

    float *memory_k = nullptr, *memory_v = nullptr;
    float *x = nullptr, *x1 = nullptr, *q = nullptr, *att = nullptr, *h = nullptr;
    // producer-quantized activations [columns][K]: [0] attention out (d_model), [1] fc1 out (d_ff), [2] LayerNorm out (d_model)
    int8_t *aq_q[3] = {nullptr, nullptr, nullptr};
    float *aq_d[3] = {nullptr, nullptr, nullptr};
    uint32_t *aq_s[3] = {nullptr, nullptr, nullptr};
    float *logits = nullptr;      // [n_vocab]
    float *logits_host = nullptr; // pinned staging for biogpt_hip_eval
    float *logits_all = nullptr;  // lazily [n][n_vocab]
    size_t logits_all_rows = 0;
    float *pmax_val = nullptr;
    float *sp_scores = nullptr, *sp_max = nullptr;   // key-split decode attention scratch (kernels_fast.hip.h)
    bool tile_img_failed = false;  // the image did not fit: passes stay on the VALU chain
    uint8_t *tile_img = nullptr;   // row-tiled copy of the chain matrices for the MFMA kernels (same offsets as the arena), built on first use
    double *sp_pv = nullptr;
    int32_t *pmax_idx = nullptr;
    int pmax_cap = 0;
    bgk::DevState *state = nullptr;  // device
    uint8_t *state_host = nullptr;   // pinned upload ring: STATE_SLOTS x (header + tokens)
    size_t state_bytes = 0;
    size_t slot_bytes = 0;
    int slot_idx = 0;

    // batched multi-sequence decode (biogpt_hip_generate_greedy_batch): per-sequence caches + state
    float *bk = nullptr, *bv = nullptr;   // [cap][n_layer][n_head][n_positions][dk]
    bgk::SeqState *seq = nullptr;         // [cap]
    bgk::SeqState *cols = nullptr;        // column states of a multi-sequence prompt pass
    size_t cols_cap = 0;
    // sequence scoring (biogpt_hip_score*): the call's targets and its three outputs {logprob, arg-max, target logit}, [3][sc_cap] words
    int32_t *sc_tgt = nullptr;
    uint32_t *sc_out = nullptr;
    size_t sc_cap = 0;
    int32_t pfxb_stats[4] = {0, 0, 0, 0};   // the last successful biogpt_hip_score_continuations_batch: prefix columns, continuation columns, passes, passes on attn_runs_kernel
    // hidden states / embeddings (biogpt_hip_hidden, biogpt_hip_embed_batch): one block that holds the call's output rows and what the call needs beside them
    uint8_t *emb_buf = nullptr;
    size_t emb_cap = 0;
    int32_t *seq_gen = nullptr;           // [cap][n_positions]
    int batch_cap = 0;
    std::set<const void *> lds_attr_done;     // kernels whose > 64 KB dynamic-LDS opt-in attribute is set on this device
    unsigned long long *tstamp = nullptr;     // profiling only (opt.dbg & 32)
    int launch_parity = 0;
    // column generation (greedy batch, sampling, beam search; the driver stands before generate_greedy_batch_once): the captured steps of each mode,
    // and the pinned word pair + event pair through which the host reads a mode's count of unfinished sequences / searches between groups of steps
    ColumnGraphs graphs_greedy, graphs_sample, graphs_beam, graphs_contrast, graphs_lookup, graphs_queue, graphs_bqueue, graphs_queue_req;
    int32_t *live_host = nullptr;
    hipEvent_t live_ev[2] = {};
    // sampled generation (biogpt_hip_generate_sample, kernels_sample.hip.h): the call's parameters + one generator state per sequence (SampleCtl, then
    // sample_cap SampleSeq)
    bgk::SampleCtl *sample_ctl = nullptr;
    int sample_cap = 0;
    // beam search (biogpt_hip_generate_beam_batch, kernels_beam.hip.h): one block of device state allocated once at its largest (bbatch_* offsets below:
    // captured steps keep their pointers)
    uint8_t *bbatch_buf = nullptr;
    // generation rules (kernels_rules.hip.h): RulesCtl, RULES_ROWS RulesRow, then the call's prompts (one copy per prompt); allocated once, at its
    // largest, so that captured steps keep their pointers
    uint8_t *rules_buf = nullptr;
    // trie-constrained generation (kernels_trie.hip.h): the call's TrieCtl; allocated once (captured steps keep the pointer, the trie's arrays are named in it)
    bgk::TrieCtl *trie_ctl = nullptr;
    // contrastive search (biogpt_hip_generate_contrastive, kernels_contrast.hip.h): the step's device state at its largest (contrast_* offsets below), allocated
    // at the first such call; the context store of contrast_groups groups -- [groups][n_positions][d_model] f32 rows, then their squared norms as doubles
    uint8_t *contrast_buf = nullptr;
    float *contrast_h = nullptr;
    int contrast_groups = 0;
    // prompt-lookup decoding (biogpt_hip_generate_lookup, kernels_lookup.hip.h): the step's device state at its largest (lookup_bufs_at), allocated at the
    // first such call -- captured steps keep their pointers
    uint8_t *lookup_buf = nullptr;
    // log-probabilities of generated tokens (biogpt_hip_generate_*_lp, kernels_genlp.hip.h): GenLpCtl and the three result arrays at their largest
    // (genlp_bufs_at), allocated at the first such call -- captured steps keep their pointers; a context that is never asked has none
    uint8_t *genlp_buf = nullptr;
    // generation over a queue (biogpt_hip_generate_queue, kernels_queue.hip.h): the step's device state at its largest (queue_bufs_at), allocated at the
    // first such call -- captured steps keep their pointers -- and its pinned twin: the header the host reads behind a group, the admit list it uploads
    uint8_t *queue_buf = nullptr;
    uint8_t *queue_host = nullptr;
    // ... whose requests carry their own parameters (biogpt_hip_generate_queue_requests): the same for that form (queue_req_bufs_at; its captured steps are
    // graphs_queue_req), and its pinned twin
    uint8_t *queue_req_buf = nullptr;
    uint8_t *queue_req_host = nullptr;
    // a queue session (biogpt_hip_queue_open) is open on this context: it has the columns, the slots and the captured steps to itself, and every other
    // evaluating call is refused (session_refuses) until biogpt_hip_queue_close
    struct biogpt_hip_queue_session *session = nullptr;
    // beam search over a queue (biogpt_hip_generate_beam_queue, kernels_beam_queue.hip.h): the searches' state is bbatch_buf; this block holds what the queue adds
    // (bqueue_bufs_at: the report header and the admit list), allocated at the first such call, and its pinned twin (BeamQueueHost, then the pool rows of
    // every slot as they come back)
    uint8_t *bqueue_buf = nullptr;
    uint8_t *bqueue_host = nullptr;

    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipGraphExec_t graph_step[2][2][6] = {};  // [pipelined][advance][context bucket: 64,128,192,256,512,P keys]; pipelined = captured with the XCD-pipelined launch (replayed only while this context holds the device's pipeline slot)
    hipGraphExec_t graph_eval[2][2][6][4] = {};   // [pipelined][form][bucket][segment] single-token biogpt_hip_eval*: the decode step with the token taken
                                               // from the state; form 0 = one graph, form 1 = a short first segment + the rest
    int graph_eval_segs[2] = {0, 0};
    // XCD-pipelined decode step (kernels_xpipe.hip.h): layer table, hand-off granules, {launch counter, error word}, pinned error mirror
    bgk::XpLayer *xp_layers = nullptr;
    bgk::xp_u64 *xp_gran = nullptr;
    bgk::xp_u64 *xp_hop = nullptr;         // the hand-off regions that cross XCDs (x1 and x of every layer): two 8 KB candidates each, xpipe_place_hops picks
    bgk::xp_u64 *xp_gran_l = nullptr;      // long-context variant (kernels_xlong.hip.h): scores and partial outputs of the key-range helpers
    bgk::xp_u64 *fp_gran = nullptr; bgk::FpLayer *fp_layers = nullptr; uint32_t *fp_ctl = nullptr;   // the float-weight persistent launch (kernels_fpipe.hip.h): hand-off granules, layer table, {tag, error word}
    int64_t fp_launches = 0;               // single-token steps enqueued (or captured) as the float-weight persistent launch (biogpt_hip_fpipe_launches)
    int fp_force = -1;                     // while a step is being CAPTURED: 1 the float-weight persistent launch, 0 five launches per layer (the graph is filed under that choice); -1: decided live
    int fp_state = 0;                      // 0 not prepared yet, 1 usable, -1 unavailable (shape, device, memory) or abandoned after a failed launch
    bgk::xp_u64 *xc_gran = nullptr;        // column-per-XCD chunk launches (kernels_xcols.hip.h): [8 columns][n_layer][XP_G_LAYER] granules, allocated (zeroed) at the first such eval
    int xc_lds = 0;                        // 0 not tried, 1 the kernels' LDS attribute is set, -1 it could not be set (such evals keep the launch chain)
    int state_n_past = 0, state_chunk = 0; // what the last upload_state put into the device state
    int64_t xc_launches = 0;               // evals that went through the chunk launch (biogpt_hip_chunk_launches)
    int64_t mfma_launches = 0;             // launches of the many-column chain that went to the matrix-core kernels (biogpt_hip_mfma_launches)
    int64_t wide_launches = 0;             // linear-stage launches of the wide chain (kernels_mfma_wide.hip.h; biogpt_hip_wide_launches)
    bool float_chain = false;              // the float chain is switched on (biogpt_hip_float_chain): passes over column states of this F32 / F16 file run on kernels_fchain.hip.h
    int64_t float_launches = 0;            // linear-stage launches of the float chain (biogpt_hip_float_launches)
    int assoc = 0;                         // 1: the SIMD association (biogpt_hip_assoc): every pass on the five-launch layer with the kernels of kernels_assoc.hip.h; no call over column states
    bool assoc_chain = false;              // the SIMD chain is switched on (biogpt_hip_assoc_chain): while assoc == 1, passes over column states run on kernels_schain.hip.h; nothing while assoc == 0
    int64_t simd_chain_launches = 0;       // linear-stage launches of the SIMD chain (biogpt_hip_simd_chain_launches)
    int32_t gen_launch_tokens[16] = {0}; int gen_launches = 0;   // the last biogpt_hip_generate_greedy: tokens of each multi-token pipelined launch (biogpt_hip_generate_launches)
    int32_t prefix_stats[4] = {0, 0, 0, 0};   // of the last biogpt_hip_generate_*_prefix call that generated tokens: shared rows, prompt columns evaluated, path (0 in place, 1 copied), columns
    int xc_batch = 0;                      // a column generation call with 2 .. 8 columns holds the device's pipeline slot (choose_column_path): its decode steps run as column-per-XCD launches (streams mode)
    uint32_t *xp_ctl = nullptr;
    bgk::xp_u64 *xp_samp = nullptr;        // arg-max partials handed from token t to token t + 1 inside a multi-token launch
    uint32_t *xp_err_host = nullptr;
    bool xp_proc_ref = false;              // this context counts in the process's hold on the device's lock file (guarded by g_xp_mu)
    bool xp_foreign = false;               // another process holds the device's lock file: no pipelined launches AND no replay of captured five-launch steps here
    bool xp_in_call = false;               // guarded by g_xp_mu: an API call of this context has taken the device's pipeline slot and has not returned yet
    bool xp_tripped = false;               // set by xpipe_check when the pipeline failed in the call that just synchronised: the API entry repeats the call once
    int xp_exp_n = 0;      // the exp table's non-zero negative slice the attention workgroups keep in LDS
    int xp_gelu_p = 0, xp_gelu_n = 0, xp_gelu_z = 0;   // the GELU table's slices every workgroup keeps in LDS (kernels_xpipe.hip.h)
    int xp_state = 0;                      // 0 not probed, 1 usable, -1 unusable on this device / model / after a failure
    uint8_t *topk_host = nullptr;          // pinned, device-visible [64 floats][64 ints][count]: biogpt_hip_eval_topk's kernel writes it directly
    int32_t *mbox_host = nullptr;          // pinned ring of 64 x {n_past, causal, token}: inputs of the graph-replayed single-token evals
    uint32_t *mbox_ctr = nullptr;          // device: replays consumed
    uint32_t *seq_dev = nullptr;           // device [4]: lineage words of a replayed single-token eval (kernels.hip.h, SEQ_*)
    uint32_t call_seq = 0;                 // host: sequence number of the last replayed eval (never 0)
    uint32_t dev_stamp_expect = 0; int32_t dev_stamp_tok = 0, dev_stamp_n_past = 0;   // the same for a row left on the device (biogpt_hip_eval_device + biogpt_hip_read_logits)
    uint32_t stamp_expect = 0;             // != 0: the pinned row of the eval in flight must carry this number (five-launch graph, form 1)
    int64_t stale_rows = 0, graph_evals = 0;   // rows found to be another call's and repaired / single-token evals replayed as five-launch graphs
    bool plain_inflight = false;           // (guarded by g_xp_mu) five-launch graphs of this context may be in flight: no OTHER context takes the pipeline slot meanwhile
    uint32_t mbox_sent = 0, mbox_synced = 0;
    int unsynced_from = -1;                // position of the first single-token eval enqueued since the stream was last synchronised (-1: none): what a tripped pipeline may have spoiled
    int lm_blocks = 0;
    // resident single-token evals (biogpt_hip_eval): a pipelined launch that is still on the device, fed through res_mbox
    int32_t *res_mbox = nullptr;           // pinned ring of 64 x 32 bytes, the first 8 = bgk::xp_post(seq, n_past, token, speculate-next)
    uint32_t *res_done = nullptr;          // pinned [256]: per lm_head workgroup, the sequence number of the last token whose logits rows it has written to logits_host
    bool res_live = false;                 // a resident launch is (or may still be) on the device
    uint32_t res_seq = 0;                  // sequence number of the last token / request posted
    int res_next = 0, res_left = 0;        // position the live launch expects next; tokens it will still take
    int res_nw = 0;                        // completion words to collect per token
    // speculative continuation (XpParams::spec_rec): passes with an odd sequence number write the *_alt row / partial buffers
    float *logits_alt = nullptr, *pmax_val_alt = nullptr;      // device
    int32_t *pmax_idx_alt = nullptr;
    float *logits_host_alt = nullptr;      // pinned
    unsigned long long *res_spec = nullptr;    // pinned: {sequence number << 32 | the device's arg-max of the token before}
    const float *row_cur = nullptr;        // the pinned row that holds the logits of the last biogpt_hip_eval / eval_inplace
    uint32_t res_acc = 0;                  // sequence number of the last pass the caller asked for (its parity says which buffers hold its results)
    bool spec_pending = false;             // the live launch starts the next position on its own account
    int spec_streak = 0, spec_need = 4;    // consecutive calls whose token was the device's arg-max; how many it takes to speculate (doubles with every miss)
    long spec_hits = 0, spec_misses = 0, spec_run = 0;
    double res_t_wait = 0.0, res_t_call = 0.0; long res_calls = 0;   // measurement only (BIOGPT_HIP_RES_DBG & 8)
    std::chrono::steady_clock::time_point res_t_last{};
    bool ready = false;  // weights present
};

static bool resident_stop(biogpt_hip_ctx *c);   // ends a resident single-token launch (defined with the eval entry points)
static void queue_session_orphan(biogpt_hip_ctx *c);   // a context freed under its open queue session: the session keeps its handle, and nothing else
// An entry point that enqueues work of its own (generate_*, eval_all, eval_prompt, the bench calls) makes the row of an EARLIER replayed single-token eval history: its lineage
// watch must not fire on a later biogpt_hip_read_logits (it would re-evaluate the old token at the old position over this call's K / V rows).  ADVICE r5.
static inline void disarm_lineage(biogpt_hip_ctx *c) { c->dev_stamp_expect = 0; c->stamp_expect = 0; }

static void drop_graphs(ColumnGraphs &gs) {
    for (auto &g : gs.exec) if (g) { (void)hipGraphExecDestroy(g); g = nullptr; }
}
// Captured column steps hold the pointers of seq / bk / bv / logits_all and launch shapes chosen from the options: whatever replaces one of those drops them all
static void drop_column_graphs(biogpt_hip_ctx *c) {
    for (ColumnGraphs *gs : {&c->graphs_greedy, &c->graphs_sample, &c->graphs_beam, &c->graphs_contrast, &c->graphs_lookup, &c->graphs_queue, &c->graphs_bqueue, &c->graphs_queue_req}) drop_graphs(*gs);
}

namespace {

bgk::DevMatrix dev_matrix(const biogpt_hip_ctx *c, const MatSlot &m) {
    bgk::DevMatrix d;
    d.qs = c->arena + m.qs;
    d.sc = c->arena + m.sc;
    d.qh = reinterpret_cast<const uint32_t *>(c->arena + m.qh);
    d.type = m.type;
    d.M = (int32_t)m.M;
    d.K = (int32_t)m.K;
    return d;
}
const float *dev_vec(const biogpt_hip_ctx *c, size_t off) { return reinterpret_cast<const float *>(c->arena + off); }

struct MvShape { int upr, lpr_log2, nit, rpw, nwaves, grid; };

// shape of the generic mat-vec launch (matvec_kernel): up to MATVEC_WAVES waves per workgroup while that keeps >= MATVEC_MIN_GRID
// workgroups, then row steps per wave until the grid is at most MATVEC_MAX_GRID workgroups (the sweep: tools/archive/sweep_matvec.py)
constexpr int MATVEC_WAVES = 4, MATVEC_MIN_GRID = 256, MATVEC_MAX_GRID = 1024;
MvShape mv_shape(int32_t type, int64_t M, int64_t K) {
    MvShape s;
    const int elems = (type == T_F32) ? 4 : (type == T_F16) ? 8 : 32;
    s.upr = (int)(K / elems);
    const int lpr = std::min(64, pow2ceil(s.upr));
    s.lpr_log2 = ilog2(lpr);
    s.nit = (s.upr + lpr - 1) / lpr;
    const int rps = 64 / lpr;
    int nw = MATVEC_WAVES;
    while (nw > 1 && (M + (int64_t)nw * rps - 1) / ((int64_t)nw * rps) < MATVEC_MIN_GRID) nw >>= 1;
    int steps = 1;
    while ( (M + (int64_t)nw * rps * steps - 1) / ((int64_t)nw * rps * steps) > MATVEC_MAX_GRID) steps++;
    s.nwaves = nw;
    s.rpw = rps * steps;
    s.grid = (int)((M + (int64_t)nw * s.rpw - 1) / ((int64_t)nw * s.rpw));
    return s;
}

template <int WT, int PRO, int EPI, int NC>
hipError_t launch_mv_kch(const bgk::MatvecParams &p, const MvShape &s, hipStream_t st) {
    // register chunks per lane the prologue needs: LN holds the whole column, plain only the wave's share
    const int njj = (p.W.K / 4 + 63) / 64;
    const int need = (PRO == bgk::PRO_LN || NC > 1) ? njj : (njj + s.nwaves - 1) / s.nwaves;  // chunks a wave holds per column
    const size_t sm = bgk::matvec_smem_bytes(WT, p.W.K, NC, s.upr, s.rpw, s.nwaves);
    const int gy = (p.N + NC - 1) / NC;
    if (need <= 4) {
        hipLaunchKernelGGL((bgk::matvec_kernel<WT, PRO, EPI, NC, 4>), dim3(s.grid, gy), dim3(s.nwaves * 64), sm, st, p);
    } else if (need <= 16) {
        hipLaunchKernelGGL((bgk::matvec_kernel<WT, PRO, EPI, NC, 16>), dim3(s.grid, gy), dim3(s.nwaves * 64), sm, st, p);
    } else {
        return hipErrorInvalidValue;  // K > 4096*nwaves: not a BioGPT shape
    }
    return hipGetLastError();
}

template <int WT, int PRO, int EPI>
hipError_t launch_mv_nc(const bgk::MatvecParams &p, const MvShape &s, hipStream_t st) {
    constexpr int NCW = bgk::TypeInfo<WT>::quant ? 8 : 4;
    // a column tile keeps whole activation columns in registers (<= 16 float4 chunks per lane, K <= 4096); wider
    // inputs (BioGPT-large fc2, K = 6400) go one column per workgroup row, where a wave only holds its share
    if (p.N == 1 || (p.W.K / 4 + 63) / 64 > 16) return launch_mv_kch<WT, PRO, EPI, 1>(p, s, st);
    return launch_mv_kch<WT, PRO, EPI, NCW>(p, s, st);
}

// ---- shape-specialised single-token path (kernels_fast.hip.h) --------------------------------------
// row steps per wave of the single-token lm_head: LM_ROW_STEPS, halved while the grid would have fewer than 128 workgroups (keep the chip covered);
// every other site takes one row step per wave.  rps: rows per wave step
constexpr int LM_ROW_STEPS = 8;
int lm_fast_steps(int M, int rps) {
    int steps = LM_ROW_STEPS;
    while (steps > 1 && (M + 4 * rps * steps - 1) / (4 * rps * steps) < 128) steps >>= 1;
    return steps;
}

// What a single-column launch of launch_mv was, as the launch itself reports it (null: not asked): 0 lm_stream_kernel, 1 matvec_fast_kernel, 2 matvec_kernel /
// fdec_kernel; its grid; the rows one workgroup's arg-max partial covers (EPI_LOGITS)
struct MvLaunch { int32_t kernel, grid, rows_per_part; };

template <int WT, int PRO, int EPI, int K>
hipError_t launch_fast_k(bgk::MatvecParams p, hipStream_t st, int *grid_out, MvLaunch *rep = nullptr) {
    constexpr int BPR = K / 32, LPR = BPR < 64 ? BPR : 64, RPS = 64 / LPR;
    const int steps = EPI == bgk::EPI_LOGITS ? lm_fast_steps(p.W.M, RPS) : 1;
    p.rpw = RPS * steps;
    const int grid = (p.W.M + 4 * p.rpw - 1) / (4 * p.rpw);
    if (grid_out) *grid_out = grid;
    if (rep) *rep = MvLaunch{1, grid, 4 * p.rpw};
    const size_t sm = bgk::matvec_fast_smem_bytes(K, p.rpw);
    if constexpr (EPI == bgk::EPI_LOGITS) {
        if (steps > 1) {
            hipLaunchKernelGGL((bgk::matvec_fast_kernel<WT, PRO, EPI, K, 4>), dim3(grid), dim3(256), sm, st, p);
            return hipGetLastError();
        }
    }
    hipLaunchKernelGGL((bgk::matvec_fast_kernel<WT, PRO, EPI, K, 1>), dim3(grid), dim3(256), sm, st, p);
    return hipGetLastError();
}

template <int WT, int PRO, int EPI>
bool try_launch_fast(const EngineOptions &o, const bgk::MatvecParams &p, hipStream_t st, hipError_t &err, int *grid_out, MvLaunch *rep = nullptr) {
    if (p.N != 1) return false;
    const int K = p.W.K;
    if (EPI == bgk::EPI_QKV && p.D != K) return false;
    if constexpr (EPI == bgk::EPI_LOGITS && PRO == bgk::PRO_LN) {
        // the single-token lm_head as one pass with all loads up front (kernels_lmhead.hip.h), when the partials are the 64-row blocks its consumers expect
        if (K == 1024 && o.lm_stream && p.W.M >= 64 * 128 && (p.dbg & 0xff & ~32) == 0) {
            constexpr int NB = 3;      // 64-row blocks per workgroup of 8 waves (2 x 8 and 3 / 4 x 16 waves measured: 8.9 / 6.8 / 8.4 us)
            const int blocks = (p.W.M + 63) / 64;
            hipLaunchKernelGGL((bgk::lm_stream_kernel<WT>), dim3((blocks + NB - 1) / NB), dim3(512), bgk::lm_stream_smem_bytes(bgk::TypeInfo<WT>::q81), st, p);
            err = hipGetLastError();
            if (grid_out) *grid_out = blocks;
            if (rep) *rep = MvLaunch{0, blocks, 64};
            return true;
        }
    }
    if (K == 1024) {
        err = launch_fast_k<WT, PRO, EPI, 1024>(p, st, grid_out, rep);
    } else if (K == 4096) {
        if constexpr (PRO == bgk::PRO_PLAIN) err = launch_fast_k<WT, PRO, EPI, 4096>(p, st, grid_out, rep);
        else return false;
    } else {
        return false;
    }
    return true;
}

// fast-chain launches with producer-quantized activations (attention -> out_proj, fc1 -> fc2; for
// prefill chunks also lnq_kernel -> q/k/v and -> fc1), NC = 1 (decode) or 8 columns per workgroup
// Which kernel a launch of the many-column linear chain is, and its geometry: what launch_chain and bg_mfma_launch report when asked.  The engine and the probe
// of single kernels (biogpt_hip_chain_device, engine_probe.inc) launch through the same helpers, so the probe's launch is the engine's.
using bgk::CK_VALU_1; using bgk::CK_VALU_8; using bgk::CK_MFMA_1; using bgk::CK_MFMA_2;      // (kernels.hip.h: mfma_tu.hip reports with the same enumerators)
struct ChainLaunch { int32_t kernel, threads, grid_x, grid_y, lds; };
static_assert(sizeof(ChainLaunch) == 5 * sizeof(int32_t), "crosses to mfma_tu.hip as five words");

template <int WT, int PRO, int EPI, int K, int PF, int NC>
hipError_t launch_fast_explicit(bgk::MatvecParams p, int steps, hipStream_t st, ChainLaunch *rep = nullptr) {
    constexpr int BPR = K / 32, LPR = BPR < 64 ? BPR : 64, RPS = 64 / LPR;
    p.rpw = RPS * steps;
    const int grid = (p.W.M + 4 * p.rpw - 1) / (4 * p.rpw);
    const int gy = (p.N + NC - 1) / NC;
    const size_t sm = bgk::matvec_fast_smem_bytes(K, p.rpw, NC, EPI == bgk::EPI_GELU_Q8);
    if (rep) *rep = ChainLaunch{NC == 1 ? CK_VALU_1 : CK_VALU_8, 256, grid, gy, (int32_t)sm};
    hipLaunchKernelGGL((bgk::matvec_fast_kernel<WT, PRO, EPI, K, PF, NC>), dim3(grid, gy), dim3(256), sm, st, p);
    return hipGetLastError();
}

enum ChainOp { CHAIN_QKV_Q8, CHAIN_OPROJ, CHAIN_FC1, CHAIN_FC1_Q8, CHAIN_FC2, CHAIN_LMHEAD_Q8 };
template <int WT, int NC>
hipError_t launch_chain_nc(ChainOp op, const bgk::MatvecParams &p, hipStream_t st, ChainLaunch *rep) {
    switch (op) {
        case CHAIN_QKV_Q8: return launch_fast_explicit<WT, bgk::PRO_Q8IN, bgk::EPI_QKV, 1024, 1, NC>(p, 1, st, rep);
        case CHAIN_OPROJ: return launch_fast_explicit<WT, bgk::PRO_Q8IN, bgk::EPI_RESID, 1024, 1, NC>(p, 1, st, rep);
        case CHAIN_FC1:   // decode: LayerNorm fused; 32 rows / workgroup = one Q8 block of fc2's input
            if constexpr (NC == 1) return launch_fast_explicit<WT, bgk::PRO_LN, bgk::EPI_GELU_Q8, 1024, 4, 1>(p, 4, st, rep);
            else return hipErrorInvalidValue;
        case CHAIN_FC1_Q8: return launch_fast_explicit<WT, bgk::PRO_Q8IN, bgk::EPI_GELU_Q8, 1024, 4, NC>(p, 4, st, rep);
        case CHAIN_FC2: return launch_fast_explicit<WT, bgk::PRO_Q8IN, bgk::EPI_RESID, 4096, 1, NC>(p, 1, st, rep);
        case CHAIN_LMHEAD_Q8:  // rows_per_wave * columns <= 64 finisher lanes: 4 row steps with 8 columns
            if constexpr (NC == 8) return launch_fast_explicit<WT, bgk::PRO_Q8IN, bgk::EPI_LOGITS, 1024, 4, 8>(p, 4, st, rep);
            else return hipErrorInvalidValue;
    }
    return hipErrorInvalidValue;
}
// many columns (prompt passes, batched sequences): the same chain on the int8 matrix cores, reading the row-tiled
// weight image (kernels_mfma.hip.h; the 25 kernels live in their own translation unit, mfma_tu.hip)
// report: null, or five words (a ChainLaunch) that the launch fills in
extern "C" int bg_mfma_launch(int wt, int op, const void *params, size_t params_bytes, const void *img, size_t img_bytes, hipStream_t st, int32_t *report);
extern "C" int bg_mfma_retile(int wt, const void *src, size_t src_bytes, uint8_t *dq, uint8_t *ds, hipStream_t st);
// the wide chain (kernels_mfma_wide.hip.h, mfma_wide_tu.hip): the many-column linear stage at any K % 32 == 0, and the Q8 producers in front of it
extern "C" int bg_wide_launch(int wt, int epi, const void *params, size_t params_bytes, const void *img, size_t img_bytes, hipStream_t st);
extern "C" int bg_wide_quantize(const float *x, int ldx, int K, int N, const float *ln_w, const float *ln_b, float eps, int q81, int8_t *oq_q, float *oq_d,
                                uint32_t *oq_s, hipStream_t st);
// Which many-column layer chain a file has (biogpt_hip_chain_kind).  1: BioGPT-base widths, every launch as before.  2: the wide chain -- any other block-quantized
// file with head size 64 whose widths the kernel's tiles divide; passes over column states only, the context's own columns stay on the generic kernels.
// 3: the float chain -- an F32 / F16 file with the wide chain's widths, and only while its context has it switched on (chain_kind; biogpt_hip_float_chain).
// 4: the SIMD chain -- a context in the SIMD association (biogpt_hip_assoc, mode 1) while it has the chain switched on (biogpt_hip_assoc_chain).
enum ChainKind : int { CHAIN_NONE = 0, CHAIN_BASE = 1, CHAIN_WIDE = 2, CHAIN_FLOAT = 3, CHAIN_SIMD = 4 };
inline int chain_kind_of(const biogpt_hip_hparams &hp) {
    if (!is_quantized(ftype_to_type(hp.ftype)) || hp.n_head < 1 || hp.d_model % hp.n_head != 0 || hp.d_model / hp.n_head != 64) return CHAIN_NONE;
    if (hp.d_model == 1024 && hp.d_ff == 4096) return CHAIN_BASE;
    return (hp.d_model % 64 == 0 && hp.d_ff >= 32 && hp.d_ff % 32 == 0) ? CHAIN_WIDE : CHAIN_NONE;
}
// the float chain (kernels_fchain.hip.h, fchain_tu.hip): the many-column linear stage on the row-major F32 / F16 weights of the arena, and the LayerNorm producer in
// front of it.  cfg: a tile shape, -1 the launch's own choice; report: null, or five words (threads, grid x, grid y, LDS bytes, cfg)
extern "C" int bg_fchain_launch(int wt, int epi, const void *params, size_t params_bytes, int cfg, hipStream_t st, int32_t *report);
extern "C" int bg_fchain_ln(int wt, const float *x, int ldx, int K, int N, const float *ln_w, const float *ln_b, float eps, float *out, hipStream_t st);
extern "C" int bg_fchain_cfg(int M, int N);
// why a file cannot have the float chain switched on (null: it can): the wide chain's width rules, on float weights
inline const char *float_chain_refusal(const biogpt_hip_hparams &hp) {
    const int32_t t = ftype_to_type(hp.ftype);
    if (t != T_F32 && t != T_F16) return "the weights are block-quantized (the float chain is for F32 / F16 files; a block-quantized file has the BioGPT-base or the wide chain)";
    if (hp.n_head < 1 || hp.d_model % hp.n_head != 0 || hp.d_model / hp.n_head != 64) return "the head size is not 64";
    if (hp.d_model % 64 != 0) return "d_model is no multiple of 64";
    if (hp.d_ff < 32 || hp.d_ff % 32 != 0) return "d_ff is no multiple of 32";
    return nullptr;
}
// why a file cannot have the SIMD association (null: it can): the oracle restates the AVX2 dot of the five block formats only (biogpt_hip_assoc)
inline const char *assoc_refusal(const biogpt_hip_hparams &hp) {
    const int32_t t = ftype_to_type(hp.ftype);
    if (t == T_F32) return "an F32 file (the oracle's AVX2 F32 dot is not built into the mat-vec yet)";
    if (t == T_F16) return "an F16 file (the oracle does not restate an AVX2 F16 dot: there is nothing to hold one to)";
    if (!is_quantized(t)) return "no block-quantized file";
    if (hp.n_head < 1 || hp.d_model % hp.n_head != 0 || hp.d_model / hp.n_head != 64) return "a head size other than 64";
    if (hp.d_model % 32 != 0 || hp.d_ff < 32 || hp.d_ff % 32 != 0) return "d_model or d_ff no multiple of 32";
    return nullptr;
}
// the SIMD chain (kernels_schain.hip.h, schain_tu.hip): the Q8 producer, the many-column linear stage and the attention over column states of a context in the
// SIMD association.  cfg: a tile shape, -1 the launch's own choice; report: null, or five words (threads, grid x, grid y, LDS bytes, cfg) / four for the other two
extern "C" int bg_schain_launch(int wt, int epi, const void *params, size_t params_bytes, int cfg, hipStream_t st, int32_t *report);
extern "C" int bg_schain_q8(int q81, const float *x, int ldx, int K, int N, const float *ln_w, const float *ln_b, float eps, int8_t *oq, float *od, uint32_t *os,
                            hipStream_t st, int32_t *report);
extern "C" int bg_schain_attn(const void *params, size_t params_bytes, int shared, int H, int N, hipStream_t st, int32_t *report);
extern "C" int bg_schain_cfg(int M, int N);
// the chain a CONTEXT's calls over column states run on: the file's, or the float chain while it is switched on; in the SIMD association the SIMD chain while
// that is switched on, else none
inline int chain_kind(const biogpt_hip_ctx *c) { return c->assoc ? (c->assoc_chain ? CHAIN_SIMD : CHAIN_NONE) : c->float_chain ? CHAIN_FLOAT : chain_kind_of(c->hp); }
template <int WT>
hipError_t launch_chain_mfma(ChainOp op, const bgk::MatvecParams &p, const bgk::DevMatrix &img, hipStream_t st, ChainLaunch *rep) {
    int site = -1;
    switch (op) {
        case CHAIN_QKV_Q8: site = 0; break;
        case CHAIN_OPROJ: site = 1; break;
        case CHAIN_FC1_Q8: site = 2; break;
        case CHAIN_FC2: site = 3; break;
        case CHAIN_LMHEAD_Q8: site = 4; break;
        default: return hipErrorInvalidValue;
    }
    return (hipError_t)bg_mfma_launch(WT, site, &p, sizeof(p), &img, sizeof(img), st, reinterpret_cast<int32_t *>(rep));
}
// the 1-column form: one column of the context's own, at the sites that have one (q/k/v, fc1 after lnq_kernel and the all-rows lm_head are 8-column kernels at any N)
inline bool chain_one_column(ChainOp op, int N, bool col_states) { return N == 1 && !col_states && op != CHAIN_LMHEAD_Q8 && op != CHAIN_QKV_Q8 && op != CHAIN_FC1_Q8; }
template <int WT>
hipError_t launch_chain_typed(ChainOp op, const bgk::MatvecParams &p, hipStream_t st, const bgk::DevMatrix *img, ChainLaunch *rep) {
    if constexpr (bgk::TypeInfo<WT>::quant) {
        if (img != nullptr && op != CHAIN_FC1) return launch_chain_mfma<WT>(op, p, *img, st, rep);
        if (chain_one_column(op, p.N, p.seq != nullptr)) return launch_chain_nc<WT, 1>(op, p, st, rep);
        return launch_chain_nc<WT, 8>(op, p, st, rep);
    }
    return hipErrorInvalidValue;
}
// rep: null, or what was launched
hipError_t launch_chain(ChainOp op, const bgk::MatvecParams &p, hipStream_t st, const bgk::DevMatrix *img = nullptr, ChainLaunch *rep = nullptr) {
    switch (p.W.type) {
        case T_Q4_0: return launch_chain_typed<bgk::W_Q4_0>(op, p, st, img, rep);
        case T_Q4_1: return launch_chain_typed<bgk::W_Q4_1>(op, p, st, img, rep);
        case T_Q5_0: return launch_chain_typed<bgk::W_Q5_0>(op, p, st, img, rep);
        case T_Q5_1: return launch_chain_typed<bgk::W_Q5_1>(op, p, st, img, rep);
        case T_Q8_0: return launch_chain_typed<bgk::W_Q8_0>(op, p, st, img, rep);
        default: return hipErrorInvalidValue;
    }
}
// LayerNorm + Q8 of N columns of 1024 values (lnq_kernel): a helper over pointers, for the engine's sites (below) and the probe
inline hipError_t launch_lnq(const float *x, int N, const float *ln_w, const float *ln_b, int q81, int8_t *oq_q, float *oq_d, uint32_t *oq_s, hipStream_t st) {
    const double inv_k = 1.0 / 1024.0;
    if (q81) hipLaunchKernelGGL((bgk::lnq_kernel<1024, true>), dim3(N), dim3(256), 0, st, x, 1024, ln_w, ln_b, 1e-5f, inv_k, oq_q, oq_d, oq_s);
    else hipLaunchKernelGGL((bgk::lnq_kernel<1024, false>), dim3(N), dim3(256), 0, st, x, 1024, ln_w, ln_b, 1e-5f, inv_k, oq_q, oq_d, oq_s);
    return hipGetLastError();
}
hipError_t launch_lnq(const biogpt_hip_ctx *c, const float *x, int N, size_t ln_w, size_t ln_b, int q81, hipStream_t st);

// ---- float weights, one column, BioGPT-base shapes (kernels_fdecode.hip.h): the whole matrix requested at t = 0 --------------------
template <int WT, int PRO, int EPI>
bool try_launch_fdec(const EngineOptions &o, const bgk::MatvecParams &p, hipStream_t st, hipError_t &err) {
    if constexpr (EPI == bgk::EPI_LOGITS || EPI == bgk::EPI_GELU_Q8 || PRO == bgk::PRO_Q8IN) {
        return false;
    } else {
        if (p.N != 1 || o.no_fdec || p.seq != nullptr || (p.dbg & 0xff) != 0) return false;
        const int K = p.W.K, M = p.W.M;
        if (EPI == bgk::EPI_QKV && (p.D != K || p.dk <= 0)) return false;
        if (K == 1024 && M == 3072 && PRO == bgk::PRO_LN && EPI == bgk::EPI_QKV) hipLaunchKernelGGL((bgk::fdec_kernel<WT, PRO, EPI, 1024, 3>), dim3(256), dim3(256), 0, st, p);
        else if (K == 1024 && M == 4096 && PRO == bgk::PRO_LN && EPI == bgk::EPI_GELU) hipLaunchKernelGGL((bgk::fdec_kernel<WT, PRO, EPI, 1024, 4>), dim3(256), dim3(256), 0, st, p);
        else if (K == 1024 && M == 1024 && PRO == bgk::PRO_PLAIN && EPI == bgk::EPI_RESID) hipLaunchKernelGGL((bgk::fdec_kernel<WT, PRO, EPI, 1024, 1>), dim3(256), dim3(256), 0, st, p);
        else if (K == 4096 && M == 1024 && PRO == bgk::PRO_PLAIN && EPI == bgk::EPI_RESID) {
            if constexpr (PRO == bgk::PRO_PLAIN) hipLaunchKernelGGL((bgk::fdec_kernel<WT, PRO, EPI, 4096, 1>), dim3(256), dim3(256), 0, st, p);
        } else return false;
        err = hipGetLastError();
        return true;
    }
}

template <int WT, int PRO, int EPI>
hipError_t launch_mv_typed(const EngineOptions &o, const bgk::MatvecParams &p, const MvShape &s, hipStream_t st, int *grid_out, MvLaunch *rep) {
    if (grid_out) *grid_out = s.grid;
    if (rep) *rep = MvLaunch{2, s.grid, s.nwaves * s.rpw};
    if constexpr (bgk::TypeInfo<WT>::quant) {
        hipError_t err = hipSuccess;
        if (try_launch_fast<WT, PRO, EPI>(o, p, st, err, grid_out, rep)) return err;
    } else {
        hipError_t err = hipSuccess;
        if (try_launch_fdec<WT, PRO, EPI>(o, p, st, err)) return err;
    }
    return launch_mv_nc<WT, PRO, EPI>(p, s, st);
}

// o: the options of the context whose launch this is (LM_STREAM, NO_FDEC)
template <int PRO, int EPI>
hipError_t launch_mv(const EngineOptions &o, const bgk::MatvecParams &p, const MvShape &s, hipStream_t st, int *grid_out = nullptr, MvLaunch *rep = nullptr) {
    switch (p.W.type) {
        case T_F32: return launch_mv_typed<bgk::W_F32, PRO, EPI>(o, p, s, st, grid_out, rep);
        case T_F16: return launch_mv_typed<bgk::W_F16, PRO, EPI>(o, p, s, st, grid_out, rep);
        case T_Q4_0: return launch_mv_typed<bgk::W_Q4_0, PRO, EPI>(o, p, s, st, grid_out, rep);
        case T_Q4_1: return launch_mv_typed<bgk::W_Q4_1, PRO, EPI>(o, p, s, st, grid_out, rep);
        case T_Q5_0: return launch_mv_typed<bgk::W_Q5_0, PRO, EPI>(o, p, s, st, grid_out, rep);
        case T_Q5_1: return launch_mv_typed<bgk::W_Q5_1, PRO, EPI>(o, p, s, st, grid_out, rep);
        case T_Q8_0: return launch_mv_typed<bgk::W_Q8_0, PRO, EPI>(o, p, s, st, grid_out, rep);
        default: return hipErrorInvalidValue;
    }
}

// ---- the SIMD association (kernels_assoc.hip.h): the launches of a context in mode 1, and of the probe of its kernels (biogpt_hip_assoc_device) ----
// What a launch of matvec_simd_kernel was: its geometry, the columns per workgroup and the rows one workgroup (and its arg-max partial) covers
struct SimdLaunch { int32_t threads, grid_x, grid_y, lds, nc, rows; };
// Four threads per row and one serial chain per thread: small matrices take small workgroups so that the chip sees enough of them (a workgroup repeats the
// prologue, which is short beside K / 32 dependent fma per row); then row steps until the grid is at most MATVEC_MAX_GRID workgroups (the arg-max
// partial buffer holds that many).  Columns per workgroup: 1, 4 or 8, what the LDS holds of them.
inline SimdLaunch simd_mv_geometry(int64_t M, int K, int N) {
    int threads = 256;
    while (threads > 64 && (M + threads / 4 - 1) / (threads / 4) < MATVEC_MIN_GRID) threads >>= 1;
    int steps = 1;
    while ((M + (int64_t)(threads / 4) * steps - 1) / ((int64_t)(threads / 4) * steps) > MATVEC_MAX_GRID) steps++;
    const int rows = threads / 4 * steps;
    int nc = N == 1 ? 1 : (N <= 4 ? 4 : 8);
    while (nc > 1 && bgk::matvec_simd_smem_bytes(K, nc) > 64 * 1024) nc = nc == 8 ? 4 : 1;
    return SimdLaunch{threads, (int32_t)((M + rows - 1) / rows), (N + nc - 1) / nc, (int32_t)bgk::matvec_simd_smem_bytes(K, nc), nc, rows};
}
template <int WT, int PRO, int EPI>
hipError_t launch_mv_simd_typed(bgk::MatvecParams p, hipStream_t st, int *grid_out, SimdLaunch *rep) {
    const SimdLaunch g = simd_mv_geometry(p.W.M, p.W.K, p.N);
    if (g.lds > 64 * 1024) return hipErrorInvalidValue;      // one column of K > 60 000 values: not a shape of any BioGPT
    p.rpw = g.rows;
    if (grid_out) *grid_out = g.grid_x;
    if (rep) *rep = g;
    const dim3 grid(g.grid_x, g.grid_y), block(g.threads);
    if (g.nc == 1) hipLaunchKernelGGL((bgk::matvec_simd_kernel<WT, PRO, EPI, 1>), grid, block, g.lds, st, p);
    else if (g.nc == 4) hipLaunchKernelGGL((bgk::matvec_simd_kernel<WT, PRO, EPI, 4>), grid, block, g.lds, st, p);
    else hipLaunchKernelGGL((bgk::matvec_simd_kernel<WT, PRO, EPI, 8>), grid, block, g.lds, st, p);
    return hipGetLastError();
}
template <int PRO, int EPI>
hipError_t launch_mv_simd(const bgk::MatvecParams &p, hipStream_t st, int *grid_out = nullptr, SimdLaunch *rep = nullptr) {
    switch (p.W.type) {
        case T_Q4_0: return launch_mv_simd_typed<bgk::W_Q4_0, PRO, EPI>(p, st, grid_out, rep);
        case T_Q4_1: return launch_mv_simd_typed<bgk::W_Q4_1, PRO, EPI>(p, st, grid_out, rep);
        case T_Q5_0: return launch_mv_simd_typed<bgk::W_Q5_0, PRO, EPI>(p, st, grid_out, rep);
        case T_Q5_1: return launch_mv_simd_typed<bgk::W_Q5_1, PRO, EPI>(p, st, grid_out, rep);
        case T_Q8_0: return launch_mv_simd_typed<bgk::W_Q8_0, PRO, EPI>(p, st, grid_out, rep);
        default: return hipErrorInvalidValue;
    }
}
// the Q8 rows alone (the probe's stage 0)
inline hipError_t launch_q8_simd_rows(const bgk::Q8SimdParams &q, hipStream_t st, SimdLaunch *rep = nullptr) {
    const size_t lds = bgk::matvec_simd_smem_bytes(q.K, 1);
    if (rep) *rep = SimdLaunch{256, q.N, 1, (int32_t)lds, 1, 0};
    hipLaunchKernelGGL(bgk::q8_simd_rows_kernel, dim3(q.N), dim3(256), lds, st, q);
    return hipGetLastError();
}

bgk::MatvecParams mv_base(const biogpt_hip_ctx *c, const MatSlot &m, const MvShape &s) {
    bgk::MatvecParams p{};
    p.W = dev_matrix(c, m);
    p.upr = s.upr; p.lpr_log2 = s.lpr_log2; p.nit = s.nit; p.rpw = s.rpw;
    p.eps = 1e-5f;  // NORM_EPS biogpt.cpp:24
    p.D = c->hp.d_model;
    p.dk = c->hp.d_model / c->hp.n_head;
    p.dk_log2 = ilog2(p.dk);
    p.P = c->hp.n_positions;
    p.st = c->state;
    p.gelu_tab = reinterpret_cast<const uint16_t *>(c->arena + c->plan.gelu_tab);
    p.dbg = c->opt.dbg | (c->launch_parity << 8);
    p.tstamp = c->tstamp;
    p.inv_k = 1.0 / (double)m.K;
    p.k_pow2 = (m.K & (m.K - 1)) == 0;
    return p;
}

// The token tail's launches as helpers over pointers: the engine's sites (enqueue_decode_fused, enqueue_xcols, enqueue_final; enqueue_argmax; eval_topk_once) and
// the probe of the tail alone (biogpt_hip_tail_device, engine_probe.inc) launch through them, so the probe's launch is the engine's.
// Final LayerNorm + lm_head of ONE column x [K] into out [M], with the arg-max partial of every workgroup's rows (pmax_val / pmax_idx, grid_out entries) --
// whichever kernel launch_mv picks for the type and shape.  p: the matrix and the site's own fields (mv_base; st_adv / adv / lineage where the site has them).
hipError_t launch_lm_head_row(const EngineOptions &o, bgk::MatvecParams p, const MvShape &s, const float *x, const float *ln_w, const float *ln_b, float *out,
                              float *pmax_val, int32_t *pmax_idx, hipStream_t st, int *grid_out, MvLaunch *rep = nullptr, bool simd = false) {
    p.ln_w = ln_w; p.ln_b = ln_b;
    p.ldx = p.W.K; p.ldo = p.W.M;
    p.x = x; p.N = 1; p.out = out;
    p.pmax_val = pmax_val; p.pmax_idx = pmax_idx;
    if (simd) {      // a context in the SIMD association (kernels_assoc.hip.h); kernel 3 of a report
        SimdLaunch g{};
        const hipError_t e = launch_mv_simd<bgk::PRO_LN, bgk::EPI_LOGITS>(p, st, grid_out, &g);
        if (rep) *rep = MvLaunch{3, g.grid_x, g.rows};
        return e;
    }
    return launch_mv<bgk::PRO_LN, bgk::EPI_LOGITS>(o, p, s, st, grid_out, rep);
}
// argmax_kernel over nparts partials: the id into the state block (next token, gen_ids), the position moved on by n_eval
hipError_t launch_argmax(const float *pmax_val, const int32_t *pmax_idx, int nparts, bgk::DevState *state, int n_eval, int n_positions, int n_vocab, hipStream_t st) {
    hipLaunchKernelGGL(bgk::argmax_kernel, dim3(1), dim3(256), 0, st, pmax_val, pmax_idx, nparts, state, n_eval, n_positions, n_vocab);
    return hipGetLastError();
}
// topk_kernel over a row of V logits and the nparts partial maxima its lm_head left: out_val / out_idx [64], out_n [1] (k, or -1: the caller takes topk_full_row)
hipError_t launch_topk(const float *logits, int V, int k, const float *pmax_val, int nparts, float *out_val, int32_t *out_idx, int32_t *out_n, hipStream_t st) {
    hipLaunchKernelGGL(bgk::topk_kernel, dim3(1), dim3(1024), 0, st, logits, V, k, pmax_val, nparts, out_val, out_idx, out_n);
    return hipGetLastError();
}

hipError_t launch_lnq(const biogpt_hip_ctx *c, const float *x, int N, size_t ln_w, size_t ln_b, int q81, hipStream_t st) {
    return launch_lnq(x, N, dev_vec(c, ln_w), dev_vec(c, ln_b), q81, c->aq_q[2], c->aq_d[2], c->aq_s[2], st);
}

// The fixed launch sequence for N tokens at the device-resident n_past (biogpt_graph's op order).
// lm_rows: 0 = last row only into c->logits (+ arg-max partials), else all N rows into logits_all.
// ---- row-tiled, expanded weight image for the MFMA kernels (kernels_mfma.hip.h) ---------------------------------
// Per block 32 int8 weights + the scale as f32 ({d, m} for Q4_1 / Q5_1): laid out matrix by matrix the first time a pass has enough columns
// (retile_kernel, from the SoA arena); 36 / 40 bytes per block -- 340 MB for BioGPT-base Q4_0, next to 288 GB of HBM.
bgk::DevMatrix tile_matrix(const biogpt_hip_ctx *c, const MatSlot &m) {
    bgk::DevMatrix d;
    d.qs = c->tile_img + m.xq;
    d.sc = c->tile_img + m.xs;
    d.qh = nullptr;
    d.type = m.type; d.M = (int32_t)m.M; d.K = (int32_t)m.K;
    return d;
}
// The image is addressed by whole 16-row tiles (retile_kernel, matmul_mfma_kernel): a matrix has one only when its rows are whole tiles.  Every layer matrix of the
// chain's shapes is; an lm_head of a vocabulary that is no multiple of 16 is not, and stays on the 8-column kernel (PassLaunch::tile).
// A wide file (chain_kind_of == CHAIN_WIDE) has no 8-column kernel to fall back to: its image holds ceil(M / 16) tiles of every matrix, the last one zero-padded.
inline bool tile_image_ok(const MatSlot &m, bool wide = false) { return is_quantized(m.type) && (wide || m.M % 16 == 0); }
// where a matrix's image lies: the 32-byte expanded blocks, then the f32 scales ({d, m} for Q4_1 / Q5_1), each part starting on 256 bytes; off: the running offset
inline void tile_image_place(int32_t type, int64_t M, int64_t K, size_t &off, size_t &xq, size_t &xs) {
    const size_t nblk = (size_t)((M + 15) / 16 * 16) * (size_t)(K / QK);      // whole tiles (M itself for every matrix of a BioGPT-base file)
    const bool q81 = type == T_Q4_1 || type == T_Q5_1;
    xq = off; off = (off + nblk * 32 + 255) & ~(size_t)255;
    xs = off; off = (off + nblk * (q81 ? 8 : 4) + 255) & ~(size_t)255;
}
bool ensure_tile_images(biogpt_hip_ctx *c) {
    if (c->tile_img || c->tile_img_failed) return true;
    size_t off = 0;
    const bool wide = chain_kind_of(c->hp) == CHAIN_WIDE;
    auto place = [&](MatSlot &m) {
        if (!tile_image_ok(m, wide)) return;
        tile_image_place(m.type, m.M, m.K, off, m.xq, m.xs);
    };
    for (auto &L : c->plan.layers) { place(L.qkv); place(L.o); place(L.fc1); place(L.fc2); }
    place(c->plan.lm_head);
    if (hipMalloc(&c->tile_img, std::max<size_t>(off, 256)) != hipSuccess) {
        // no room for the image (several contexts / replicas on one device): the passes stay on the VALU chain, which needs none
        (void)hipGetLastError();
        c->tile_img = nullptr; c->tile_img_failed = true;
        if (c->opt.verbose) fprintf(stderr, "biogpt_hip: no memory for the %zu-byte row-tiled weight image; many-column passes stay on the 8-column kernels\n", off);
        return true;
    }
    bool retile_ok = true;
    auto one = [&](const MatSlot &m) {
        if (!tile_image_ok(m, wide)) return;
        const bgk::DevMatrix src = dev_matrix(c, m);
        if (m.M % 16 != 0) {      // the rows the last tile has beyond the matrix: zero weights, zero scales
            const size_t nblk = (size_t)((m.M + 15) / 16 * 16) * (size_t)(m.K / QK);
            if (hipMemsetAsync(c->tile_img + m.xq, 0, nblk * 32, c->stream) != hipSuccess ||
                hipMemsetAsync(c->tile_img + m.xs, 0, nblk * ((m.type == T_Q4_1 || m.type == T_Q5_1) ? 8 : 4), c->stream) != hipSuccess) retile_ok = false;
        }
        if (bg_mfma_retile(m.type, &src, sizeof(src), c->tile_img + m.xq, c->tile_img + m.xs, c->stream) != (int)hipSuccess) retile_ok = false;
    };
    for (const auto &L : c->plan.layers) { one(L.qkv); one(L.o); one(L.fc1); one(L.fc2); }
    one(c->plan.lm_head);
    if (!retile_ok || hipGetLastError() != hipSuccess) {
        // a partially built image must never be used (the next call would find tile_img non-null and run the matrix-core chain on it): drop it, the passes stay on the VALU chain
        (void)hipStreamSynchronize(c->stream); (void)hipGetLastError();
        (void)hipFree(c->tile_img);
        c->tile_img = nullptr; c->tile_img_failed = true;
        if (c->opt.verbose) fprintf(stderr, "biogpt_hip: building the row-tiled weight image failed; many-column passes stay on the 8-column kernels\n");
        return true;
    }
    return true;
}

#include "engine_xpipe.inc"

// ---- fused single-token decode step (kernels_decode.hip.h): 3 launches per layer + lm_head ---------------------
// tok_src 1: the token is in the device state (an eval call); 2: arg-max of the previous step's lm_head partials.
// advance: the lm_head kernel moves the device-side position on by one when the step is done.
bool fused_decode_ok(const biogpt_hip_ctx *c, int t_max) {
    const auto &hp = c->hp;
    return is_quantized(ftype_to_type(hp.ftype)) && hp.d_model == 1024 && hp.d_ff == 4096 && hp.n_head == 16 && t_max <= 1024 &&
           hp.n_positions >= 64 && !c->opt.no_fused_decode && c->assoc == 0;      // (the SIMD association has the five launches per layer only)
}

// only: -1 = the five kernels of the layer in order; 0..4 = just that kernel (biogpt_hip_bench_matvec)
// Workgroup shapes: 8 waves each (same-process sweeps, profiles/decode_shapes_r2.txt: 8 waves beat 16 and 4); the attention takes
// 8 waves up to 128 keys and 16 beyond
template <int WT>
hipError_t launch_decode_layer(biogpt_hip_ctx *c, const bgk::DecQkvParams &a, const bgk::DecAttnParams &at, const bgk::DecOprojParams &op,
                               const bgk::DecFc1Params &f1, const bgk::DecFc2Params &f2, int only = -1) {
    hipStream_t st = c->stream;
    if (only < 0 || only == 0) hipLaunchKernelGGL((bgk::dec_qkv_kernel<WT, 8>), dim3(192), dim3(512), bgk::dec_qkv_smem_bytes(), st, a);
    if ((only < 0 || only == 1) && at.t_cap > 256) {
        // beyond 256 keys one workgroup per head would pull up to 512 KB of K / V through one compute unit: the keys of a head
        // are spread over H x T/64 workgroups in three dependent launches (attn_split_*_kernel, kernels_fast.hip.h)
        bgk::AttnParams sa{};
        sa.q = at.q; sa.kcache = at.kcache; sa.vcache = at.vcache; sa.out = c->att; sa.st = at.st; sa.exp_tab = at.exp_tab;
        sa.N = 1; sa.D = c->hp.d_model; sa.dk = 64; sa.P = at.P; sa.t_cap = at.t_cap;
        sa.oq_q = at.oq_q; sa.oq_d = at.oq_d; sa.oq_s = at.oq_s; sa.q81 = at.q81;
        sa.sp_scores = c->sp_scores; sa.sp_max = c->sp_max; sa.sp_pv = c->sp_pv;
        sa.n_split = (sa.t_cap + bgk::SPLIT_KEYS - 1) / bgk::SPLIT_KEYS;
        if (sa.n_split > bgk::SPLIT_MAX) BG_FAIL(hipErrorInvalidValue, "internal: %d key ranges exceed the %d the split attention kernels hold", sa.n_split, bgk::SPLIT_MAX);
        hipLaunchKernelGGL(bgk::attn_split_scores_kernel, dim3(16, sa.n_split), dim3(256), 0, st, sa);
        hipLaunchKernelGGL(bgk::attn_split_pv_kernel, dim3(16, sa.n_split), dim3(256), 0, st, sa);
        hipLaunchKernelGGL(bgk::attn_split_combine_kernel, dim3(16), dim3(64), 0, st, sa);
    } else if (only < 0 || only == 1) {
        if (at.t_cap <= 64) hipLaunchKernelGGL((bgk::dec_attn_kernel<8, 8>), dim3(16), dim3(512), 0, st, at);
        else if (at.t_cap <= 128) hipLaunchKernelGGL((bgk::dec_attn_kernel<4, 8>), dim3(16), dim3(512), 0, st, at);
        else hipLaunchKernelGGL((bgk::dec_attn_kernel<4, 16>), dim3(16), dim3(1024), 0, st, at);
    }
    if (only < 0 || only == 2) hipLaunchKernelGGL((bgk::dec_oproj_kernel<WT, 8>), dim3(64), dim3(512), bgk::dec_oproj_smem_bytes(8), st, op);
    if (only < 0 || only == 3) hipLaunchKernelGGL((bgk::dec_fc1_kernel<WT, 1, 8>), dim3(128), dim3(512), bgk::dec_fc1_smem_bytes<1>(), st, f1);
    if (only < 0 || only == 4) hipLaunchKernelGGL((bgk::dec_fc2_kernel<WT, 8>), dim3(128), dim3(512), bgk::dec_fc2_smem_bytes(8), st, f2);
    return hipGetLastError();
}

// grid of the single-token lm_head launch (launch_fast_k, K = 1024: 2 rows per wave step, 4 waves)
int fast_lm_grid(const biogpt_hip_ctx *c) {
    const int M = c->hp.n_vocab, steps = lm_fast_steps(M, 2);
    return (M + 8 * steps - 1) / (8 * steps);
}

// l0 / l1 / only: biogpt_hip_bench_matvec launches one kernel of one layer; the decode step is all layers + lm_head
// host_row (optional): pinned host buffer that also receives the logits row; *host_row_done tells whether the launch wrote it itself
// pl: -1 = go through the XCD pipeline if this context can take the device's slot now; 0 / 1 = the caller decided (graph capture: the
//     graph is replayed only in the matching state)
struct ResidentArgs { int32_t tok0, n_past0; uint32_t seq0; int32_t spec0; };
bool enqueue_decode_fused(biogpt_hip_ctx *c, int t_max, int tok_src, int advance, int l0 = 0, int l1 = -1, int only = -1, int n_tok = 1, float *host_row = nullptr,
                          bool *host_row_done = nullptr, int pl = -1, const ResidentArgs *ra = nullptr) {
    (void)hipGetLastError();
    const auto &hp = c->hp;
    const int D = hp.d_model, V = hp.n_vocab, P = hp.n_positions;
    const int lm_parts = fast_lm_grid(c);   // partials the previous step's lm_head left (same launch shape every step)
    if (lm_parts > c->pmax_cap) BG_FAIL(false, "internal: arg-max partial buffer too small (%d > %d)", lm_parts, c->pmax_cap);
    const int32_t wt = ftype_to_type(hp.ftype);
    const int q81 = (wt == T_Q4_1 || wt == T_Q5_1) ? 1 : 0;
    unsigned long long *const ts = (c->opt.dbg & 96) ? c->tstamp : nullptr;
    unsigned long long *const wall = (c->opt.dbg & 64) ? c->tstamp + 128 : nullptr;
    if (l1 < 0) l1 = hp.n_layer;
    const bool pipelined = only < 0 && l0 == 0 && l1 == hp.n_layer && tok_src != 0 && (pl < 0 ? xpipe_usable(c, t_max) : (pl == 1 && xpipe_bucket_ok(c, t_max)));
    bool lm_in_kernel = false;
    if (n_tok > 1 && !pipelined) BG_FAIL(false, "internal: multi-token launches exist on the XCD pipeline only");
    if (only == -2 && !pipelined) BG_FAIL(false, "the XCD-pipelined decode step is not available for this context");
    if (pipelined) {
        bgk::XpParams xp{};
        xp.layers = c->xp_layers; xp.n_layer = hp.n_layer; xp.gran = c->xp_gran; xp.gran_l = c->xp_gran_l; xp.ctl = c->xp_ctl; xp.err_host = c->xp_err_host;
        xp.st = c->state;
        xp.tok_emb = dev_matrix(c, c->plan.embed_tokens); xp.pos_emb = dev_matrix(c, c->plan.embed_pos);
        xp.embed_scale = sqrtf((float)D);
        xp.tok_src = tok_src; xp.as_res = c->opt.xpipe_as_res;
        xp.pmax_val = c->pmax_val; xp.pmax_idx = c->pmax_idx; xp.nparts = lm_parts;
        xp.n_positions = P; xp.n_vocab = V;
        xp.eps = 1e-5f; xp.q_scale = 1.0f / sqrtf(64.0f);
        xp.P = P; xp.t_cap = std::min(P, (t_max + 63) & ~63); xp.dual = (c->opt.xpipe_dual && c->xp_gran_l != nullptr) ? 1 : 0;
        xp.exp_tab = reinterpret_cast<const uint16_t *>(c->arena + c->plan.exp_tab);
        xp.gelu_tab = reinterpret_cast<const uint16_t *>(c->arena + c->plan.gelu_tab);
        xp.gelu_p = c->xp_gelu_p; xp.gelu_n = c->xp_gelu_n; xp.gelu_z = c->xp_gelu_z; xp.exp_n = c->xp_exp_n;
        xp.x_final = c->x;
        {   // lm_head inside the launch: its 64-row blocks (= the stand-alone launch's workgroups) three per workgroup of 7 XCDs
            const MatSlot &m = c->plan.lm_head;
            const bool fold = xpipe_lm_folds(c);
            xp.lm = fold ? 1 : 0;
            xp.lm_blocks = lm_parts; xp.adv = fold ? advance : 0; xp.n_tok = n_tok; xp.samp = c->xp_samp;   // no lm_head in here: the lm_head launch moves the position
            xp.Wlm = dev_matrix(c, m);
            xp.lm_ln_w = dev_vec(c, c->plan.ln_w); xp.lm_ln_b = dev_vec(c, c->plan.ln_b);
            xp.logits = c->logits; xp.logits_host = fold ? host_row : nullptr; xp.pmax_out_val = c->pmax_val; xp.pmax_out_idx = c->pmax_idx;
            lm_in_kernel = fold;
            if (host_row_done) *host_row_done = fold && host_row != nullptr;
            if (ra) {     // resident launch (biogpt_hip_eval): token 0 and its position travel in the parameter block, the following ones through the mailbox
                if (!(fold && host_row && advance == 0 && tok_src == 1 && xp.t_cap <= 1024 && (xp.t_cap <= 256 || xp.gran_l != nullptr))) BG_FAIL(false, "internal: a resident launch needs the lm_head inside the pipelined launch");
                xp.resident = 1; xp.mbox = c->res_mbox; xp.mbox_seq0 = ra->seq0; xp.done_host = c->res_done;
                xp.idle_ticks = (uint32_t)std::min(10000000, std::max(1, c->opt.resident_us)) * 100u;      // 100 MHz ticks; clamped to 10 s (the product must fit 32 bits)
                xp.res_tok0 = ra->tok0; xp.res_n_past0 = ra->n_past0; xp.res_dbg = c->opt.res_dbg;
                xp.res_spec0 = ra->spec0; xp.spec_rec = c->res_spec;
                xp.logits_alt = c->logits_alt; xp.logits_host_alt = c->logits_host_alt; xp.pmax_alt_val = c->pmax_val_alt; xp.pmax_alt_idx = c->pmax_idx_alt;
                if (!xp.spec_rec || !xp.logits_alt || !xp.logits_host_alt || !xp.pmax_alt_val || !xp.pmax_alt_idx) BG_FAIL(false, "internal: a resident launch without its alternate buffers");
            } else if (n_tok > 1 && !(fold && advance == 1 && tok_src == 2)) BG_FAIL(false, "internal: a multi-token launch needs the lm_head inside the pipeline");
        }
        xp.wall = ((c->opt.dbg & 128) || (ra && (c->opt.res_dbg & 32))) ? c->tstamp : nullptr;
        const hipError_t e = (hipError_t)bg_xpipe_launch(wt, xp.t_cap, bgk::xpipe_smem_bytes(xp.gelu_p + xp.gelu_n), c->stream, &xp, sizeof(xp));
        HIP_TRY(false, e);
    }
    for (int l = l0; l < l1 && !pipelined; l++) {
        const LayerSlots &L = c->plan.layers[(size_t)l];
        bgk::DecQkvParams a{};
        a.x = c->x; a.x_out = c->x;
        a.tok_emb = dev_matrix(c, c->plan.embed_tokens); a.pos_emb = dev_matrix(c, c->plan.embed_pos);
        a.embed_scale = sqrtf((float)D);
        a.tok_src = (l == 0) ? tok_src : 0;
        a.pmax_val = c->pmax_val; a.pmax_idx = c->pmax_idx; a.nparts = lm_parts;
        a.st = c->state; a.n_positions = P; a.n_vocab = V;
        a.ln_w = dev_vec(c, L.ln0_w); a.ln_b = dev_vec(c, L.ln0_b); a.eps = 1e-5f;
        a.Wqkv = dev_matrix(c, L.qkv); a.bqkv = dev_vec(c, L.qkv_b); a.q_scale = 1.0f / sqrtf(64.0f);
        a.q_out = c->q;
        a.kcache = c->memory_k + (size_t)l * P * D; a.vcache = c->memory_v + (size_t)l * P * D; a.P = P;
        a.tstamp = ts; a.wall = wall; a.wall_slot = 5 * l;
        bgk::DecAttnParams at{};
        at.q = c->q; at.kcache = a.kcache; at.vcache = a.vcache; at.st = c->state; at.P = P;
        at.t_cap = std::min(P, (t_max + 63) & ~63);
        at.exp_tab = reinterpret_cast<const uint16_t *>(c->arena + c->plan.exp_tab);
        at.oq_q = c->aq_q[0]; at.oq_d = c->aq_d[0]; at.oq_s = c->aq_s[0]; at.att_out = nullptr; at.q81 = q81;
        at.tstamp = ts ? ts + 16 : nullptr; at.wall = wall; at.wall_slot = 5 * l + 1;
        bgk::DecOprojParams op{};
        op.Wo = dev_matrix(c, L.o); op.aq_q = c->aq_q[0]; op.aq_d = c->aq_d[0]; op.aq_s = c->aq_s[0];
        op.bias = dev_vec(c, L.o_b); op.resid = c->x; op.out = c->x1;
        op.tstamp = ts ? ts + 32 : nullptr; op.wall = wall; op.wall_slot = 5 * l + 2;
        bgk::DecFc1Params f1{};
        f1.x1 = c->x1;
        f1.ln_w = dev_vec(c, L.ln1_w); f1.ln_b = dev_vec(c, L.ln1_b); f1.eps = 1e-5f;
        f1.W1 = dev_matrix(c, L.fc1); f1.b1 = dev_vec(c, L.fc1_b);
        f1.gelu_tab = reinterpret_cast<const uint16_t *>(c->arena + c->plan.gelu_tab);
        f1.oq_q = c->aq_q[1]; f1.oq_d = c->aq_d[1]; f1.oq_s = c->aq_s[1]; f1.q81 = q81;
        f1.tstamp = ts ? ts + 48 : nullptr; f1.wall = wall; f1.wall_slot = 5 * l + 3;
        bgk::DecFc2Params f2{};
        f2.W2 = dev_matrix(c, L.fc2); f2.aq_q = c->aq_q[1]; f2.aq_d = c->aq_d[1]; f2.aq_s = c->aq_s[1];
        f2.bias = dev_vec(c, L.fc2_b); f2.resid = c->x1; f2.out = c->x;
        f2.tstamp = ts ? ts + 64 : nullptr; f2.wall = wall; f2.wall_slot = 5 * l + 4;
        f2.seq = (l == hp.n_layer - 1) ? c->seq_dev : nullptr;
        hipError_t e = hipErrorInvalidValue;
        switch (wt) {
            case T_Q4_0: e = launch_decode_layer<bgk::W_Q4_0>(c, a, at, op, f1, f2, only); break;
            case T_Q4_1: e = launch_decode_layer<bgk::W_Q4_1>(c, a, at, op, f1, f2, only); break;
            case T_Q5_0: e = launch_decode_layer<bgk::W_Q5_0>(c, a, at, op, f1, f2, only); break;
            case T_Q5_1: e = launch_decode_layer<bgk::W_Q5_1>(c, a, at, op, f1, f2, only); break;
            case T_Q8_0: e = launch_decode_layer<bgk::W_Q8_0>(c, a, at, op, f1, f2, only); break;
            default: break;
        }
        HIP_TRY(false, e);
    }
    if (lm_in_kernel) { c->lm_blocks = lm_parts; return true; }   // the pipelined launch wrote the logits, the partials and moved the position
    if (only >= 0 || only == -2 || l1 < hp.n_layer) return true;   // one kernel (bench) or a leading segment of the step: no lm_head
    {  // final LayerNorm + lm_head (last row only, F8) + per-workgroup arg-max partials; block 0 advances the position
        const MatSlot &m = c->plan.lm_head;
        const MvShape s = mv_shape(m.type, m.M, m.K);
        bgk::MatvecParams p = mv_base(c, m, s);
        p.st_adv = c->state; p.adv = advance;
        p.lineage = c->seq_dev;
        int lm_grid = 0;
        HIP_TRY(false, launch_lm_head_row(c->opt, p, s, c->x, dev_vec(c, c->plan.ln_w), dev_vec(c, c->plan.ln_b), c->logits, c->pmax_val, c->pmax_idx, c->stream, &lm_grid));
        if (lm_grid != lm_parts) BG_FAIL(false, "internal: lm_head grid %d != expected %d", lm_grid, lm_parts);
        c->lm_blocks = lm_grid;
    }
    return true;
}

// ---- single-token steps of FLOAT weight files as ONE persistent launch for all layers (kernels_fpipe.hip.h, fpipe_tu.hip) ----
extern "C" int bg_fpipe_launch(int wt, hipStream_t st, const void *params, size_t params_bytes);
extern "C" int bg_fpipe_set_lds(void);
bool fpipe_prepare(biogpt_hip_ctx *c) {
    if (c->fp_state != 0) return c->fp_state == 1;
    c->fp_state = -1;
    const auto &hp = c->hp;
    if (!c->opt.fpipe || hp.d_model != 1024 || hp.d_ff != 4096 || hp.n_head != 16 || hp.n_layer < 1 || c->device < 0 || c->device >= 64) return false;
    int32_t wt = -1;
    for (const auto &L : c->plan.layers) {
        for (const MatSlot *m : {&L.qkv, &L.o, &L.fc1, &L.fc2}) {
            if (m->type != T_F32 && m->type != T_F16) return false;
            if (wt >= 0 && m->type != wt) return false;
            wt = m->type;
        }
        if (L.qkv.M != 3072 || L.qkv.K != 1024 || L.o.M != 1024 || L.o.K != 1024 || L.fc1.M != 4096 || L.fc1.K != 1024 || L.fc2.M != 1024 || L.fc2.K != 4096) return false;
    }
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(c->stream, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) { (void)hipGetLastError(); c->fp_state = 0; return false; }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, c->device) != hipSuccess || prop.multiProcessorCount != 256 || (size_t)prop.sharedMemPerBlockOptin < bgk::fpipe_smem_bytes()) { (void)hipGetLastError(); return false; }
    if (!xpipe_process_lock(c)) return false;      // a persistent launch: one process per device drives them (engine_xpipe.inc)
    const size_t P = (size_t)hp.n_positions, D = (size_t)hp.d_model;
    std::vector<bgk::FpLayer> tab((size_t)hp.n_layer);
    for (int l = 0; l < hp.n_layer; l++) {
        const LayerSlots &L = c->plan.layers[(size_t)l];
        bgk::FpLayer &y = tab[(size_t)l];
        y.ln0_w = dev_vec(c, L.ln0_w); y.ln0_b = dev_vec(c, L.ln0_b); y.ln1_w = dev_vec(c, L.ln1_w); y.ln1_b = dev_vec(c, L.ln1_b);
        y.bqkv = dev_vec(c, L.qkv_b); y.bo = dev_vec(c, L.o_b); y.b1 = dev_vec(c, L.fc1_b); y.b2 = dev_vec(c, L.fc2_b);
        y.Wqkv = dev_matrix(c, L.qkv).qs; y.Wo = dev_matrix(c, L.o).qs; y.W1 = dev_matrix(c, L.fc1).qs; y.W2 = dev_matrix(c, L.fc2).qs;
        y.kcache = c->memory_k + (size_t)l * P * D; y.vcache = c->memory_v + (size_t)l * P * D;
    }
    const size_t gbytes = (size_t)(1024 + 3072 + 1024 + 1024 + 4096) * 8;
    const uint32_t ctl0[2] = {1u, 0u};
    bool ok = hipMalloc(&c->fp_layers, tab.size() * sizeof(bgk::FpLayer)) == hipSuccess && hipMalloc(&c->fp_gran, gbytes) == hipSuccess && hipMalloc(&c->fp_ctl, 64 + 3 * 1024 * 8) == hipSuccess &&
              hipMemcpy(c->fp_layers, tab.data(), tab.size() * sizeof(bgk::FpLayer), hipMemcpyHostToDevice) == hipSuccess && hipMemset(c->fp_gran, 0, gbytes) == hipSuccess &&
              hipMemset(c->fp_ctl, 0, 64 + 3 * 1024 * 8) == hipSuccess && hipMemcpy(c->fp_ctl, ctl0, 8, hipMemcpyHostToDevice) == hipSuccess;
    if (ok && !c->xp_err_host) { ok = hipHostMalloc(reinterpret_cast<void **>(&c->xp_err_host), 64, hipHostMallocDefault) == hipSuccess; if (ok) *c->xp_err_host = 0u; }
    ok = ok && bg_fpipe_set_lds() == (int)hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        for (void *q : {(void *)c->fp_layers, (void *)c->fp_gran, (void *)c->fp_ctl}) if (q) (void)hipFree(q);
        c->fp_layers = nullptr; c->fp_gran = nullptr; c->fp_ctl = nullptr;
        return false;
    }
    c->fp_state = 1;
    return true;
}
bool fpipe_usable(biogpt_hip_ctx *c, int t_max) {
    if (t_max > bgk::FP_TMAX || !fpipe_prepare(c)) return false;
    return pipeline_slot_take(c);
}
// which form of a single-token step may be captured / replayed for this context bucket: 1 a persistent launch (the XCD pipeline; float files: kernels_fpipe.hip.h) -- the
// device's slot is then this context's until its next synchronisation --, 0 five launches per layer
int pipeline_pl(biogpt_hip_ctx *c, int t_max) {
    if (xpipe_usable(c, t_max)) return 1;
    return (c->fp_state >= 0 && !fused_decode_ok(c, t_max) && fpipe_usable(c, t_max)) ? 1 : 0;
}
// the token of the device state, embedded into c->x by the launch in front, through all layers; the final LayerNorm + lm_head launch follows
bool enqueue_fpipe(biogpt_hip_ctx *c) {
    const auto &hp = c->hp;
    bgk::FpParams fp{};
    fp.layers = c->fp_layers; fp.n_layer = hp.n_layer;
    fp.g_x = c->fp_gran; fp.g_qkv = fp.g_x + 1024; fp.g_att = fp.g_qkv + 3072; fp.g_x1 = fp.g_att + 1024; fp.g_h = fp.g_x1 + 1024;
    fp.ctl = c->fp_ctl; fp.err_host = c->xp_err_host;
    fp.st = c->state; fp.x_in = c->x; fp.x_out = c->x;
    fp.eps = 1e-5f; fp.q_scale = 1.0f / sqrtf(64.0f); fp.P = hp.n_positions;
    fp.exp_tab = reinterpret_cast<const uint16_t *>(c->arena + c->plan.exp_tab);
    fp.gelu_tab = reinterpret_cast<const uint16_t *>(c->arena + c->plan.gelu_tab);
    if (c->unsynced_from < 0) c->unsynced_from = c->state_n_past;
    fp.fault = (c->opt.fpipe_fault && c->fp_launches == 0) ? 1 : 0;
    fp.lead = c->opt.fpipe_lead >= 0 ? c->opt.fpipe_lead : (c->plan.layers[0].qkv.type == T_F32 ? 26 : 16);
    fp.stamps = c->opt.fpipe_stamps ? reinterpret_cast<unsigned long long *>(c->fp_ctl + 16) : nullptr;
    c->fp_launches++;
    HIP_TRY(false, (hipError_t)bg_fpipe_launch(c->plan.layers[0].qkv.type == T_F32 ? 0 : 1, c->stream, &fp, sizeof(fp)));
    return true;
}

// ---- biogpt_eval with 2 .. 8 tokens (the reference's prompt chunks, main.cpp:129-137) as ONE persistent launch: one column per XCD (kernels_xcols.hip.h) ----
extern "C" int bg_xcols_launch(int wt, int t_cap, size_t smem_bytes, hipStream_t st, const void *params, size_t params_bytes);
extern "C" int bg_xcols_set_lds(int wt, size_t smem_bytes);

// May this pass go through the chunk launch ?  It is one more launch of the context's pipeline (same control words and tag counter, all 256 compute units held):
// same conditions and the device's pipeline slot (taken here).  Not under the opt-in causal mask, not for columns that are several reference chunks (DevState::chunk).
// model / device / options fit, and the launch's buffers exist (allocated here: never inside a stream capture)
bool xcols_prepare(biogpt_hip_ctx *c, int N, int t_max) {
    const int32_t wt = ftype_to_type(c->hp.ftype);
    if (!c->opt.xcols || c->opt.causal || N < 2 || N > 8 || t_max > 512 || c->xc_lds < 0) return false;      // (257 .. 512 keys: the variant that requests the second half of a head's old rows inside the attention stage)
    if (!(wt == T_Q4_0 || wt == T_Q4_1 || wt == T_Q5_0 || wt == T_Q5_1 || wt == T_Q8_0)) return false;
    if (!fused_decode_ok(c, t_max) || c->xp_state != 1) return false;
    if (c->xc_gran && c->xc_lds == 1) return true;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(c->stream, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) { (void)hipGetLastError(); return false; }
    if (!c->xc_gran) {
        const size_t bytes = (size_t)8 * c->hp.n_layer * bgk::XP_G_LAYER * 8;
        if (hipMalloc(&c->xc_gran, bytes) != hipSuccess || hipMemsetAsync(c->xc_gran, 0, bytes, c->stream) != hipSuccess) {
            (void)hipGetLastError();
            if (c->xc_gran) (void)hipFree(c->xc_gran);
            c->xc_gran = nullptr; c->xc_lds = -1;
            return false;
        }
    }
    if (c->xc_lds == 0) {
        const size_t sm = bgk::xpipe_smem_bytes(c->xp_gelu_p + c->xp_gelu_n);
        c->xc_lds = (sm <= 64 * 1024 || bg_xcols_set_lds(wt, sm) == (int)hipSuccess) ? 1 : -1;
        (void)hipGetLastError();
        if (c->xc_lds < 0) return false;
    }
    return true;
}
bool xcols_usable(biogpt_hip_ctx *c, int N, int t_max) {
    if (c->state_chunk != 0 || !xcols_prepare(c, N, t_max)) return false;
    return xpipe_usable(c, std::min(t_max, 256));      // the device's pipeline slot (a chunk launch needs none of the long-context launch's regions)
}

// the N columns of the device state (upload_state) through all layers in one launch, then the ordinary final LayerNorm + lm_head launch on the LAST column (F8)
bool enqueue_xcols(biogpt_hip_ctx *c, int N, int t_max, bool streams = false) {
    (void)hipGetLastError();
    const auto &hp = c->hp;
    const int D = hp.d_model, V = hp.n_vocab, P = hp.n_positions;
    const int32_t wt = ftype_to_type(hp.ftype);
    bgk::XcParams xc{};
    xc.layers = c->xp_layers; xc.n_layer = hp.n_layer; xc.gran = c->xc_gran; xc.ctl = c->xp_ctl; xc.err_host = c->xp_err_host;
    xc.st = c->state;
    xc.tok_emb = dev_matrix(c, c->plan.embed_tokens); xc.pos_emb = dev_matrix(c, c->plan.embed_pos);
    xc.embed_scale = sqrtf((float)D);
    xc.n_positions = P; xc.n_vocab = V;
    xc.eps = 1e-5f; xc.q_scale = 1.0f / sqrtf(64.0f);
    xc.P = P; xc.t_cap = std::min(P, (t_max + 63) & ~63);
    xc.exp_tab = reinterpret_cast<const uint16_t *>(c->arena + c->plan.exp_tab);
    xc.gelu_tab = reinterpret_cast<const uint16_t *>(c->arena + c->plan.gelu_tab);
    xc.gelu_p = c->xp_gelu_p; xc.gelu_n = c->xp_gelu_n; xc.gelu_z = c->xp_gelu_z;
    xc.n_cols = N; xc.x_out = c->x;
    if (streams) { xc.seq = c->seq; xc.kroot = c->bk; xc.vroot = c->bv; xc.seq_stride = (int64_t)hp.n_layer * P * D; }
    if ((c->opt.dbg & 128) && !c->tstamp) {      // profiling builds: stage stamps (tools/xcols_timeline.py)
        HIP_TRY(false, hipMalloc(&c->tstamp, (size_t)4 << 20));
        HIP_TRY(false, hipMemset(c->tstamp, 0, (size_t)4 << 20));
    }
    xc.wall = (c->opt.dbg & 128) ? c->tstamp : nullptr;
    if (c->unsynced_from < 0) c->unsynced_from = streams ? 0 : c->state_n_past;      // what a disturbed launch would spoil: this chunk's K / V rows (and every later eval's until the next synchronisation)
    c->xc_launches++;
    HIP_TRY(false, (hipError_t)bg_xcols_launch(wt, xc.t_cap, bgk::xpipe_smem_bytes(xc.gelu_p + xc.gelu_n), c->stream, &xc, sizeof(xc)));
    if (streams) return true;      // every sequence's row: the caller's 8-column lm_head chain on c->x
    {  // final LayerNorm + lm_head of the last column + per-workgroup arg-max partials
        const MatSlot &m = c->plan.lm_head;
        const MvShape s = mv_shape(m.type, m.M, m.K);
        const bgk::MatvecParams p = mv_base(c, m, s);
        if (s.grid > c->pmax_cap) BG_FAIL(false, "internal: arg-max partial buffer too small (%d > %d)", s.grid, c->pmax_cap);
        int lm_grid = 0;
        HIP_TRY(false, launch_lm_head_row(c->opt, p, s, c->x + (size_t)(N - 1) * D, dev_vec(c, c->plan.ln_w), dev_vec(c, c->plan.ln_b), c->logits, c->pmax_val, c->pmax_idx,
                                          c->stream, &lm_grid));
        c->lm_blocks = lm_grid;
    }
    return true;
}

// Measured cross-overs of the many-column paths (HISTORY.md §4.7 / §4.8): the chain runs on the int8 matrix cores from 48 columns in the decode
// steps of many sequences and from 64 in passes (below, the 8-column VALU kernels are faster); a pass takes the grouped-query attention from
// 80 columns, a decode step of many sequences the slim attention kernel from 48; one query beyond 256 keys spreads its head over the chip
// attn_prefix_kernel<8> instead of attn_fast_kernel<.., SHARED> for a decode step behind a shared prefix: from this many columns and shared rows on.
// (2026-10-19, tools/prefix_gen_bench.py --ab: the in-place call, 24 layers, 16-token suffixes + 64 tokens, the kernel never / always taken, grouped / existing.
// 128 / 256 columns: 0.91 / 0.91 x behind 376 shared rows, 0.74 / 0.72 x behind 888, but 1.14 / 1.23 x behind 56.  16 / 48 / 64 columns: 1.70 / 1.42 / 1.36 x (56),
// 1.77 / 1.29 / 1.20 x (376), 1.87 / 1.20 / 1.05 x (888): it loses everywhere below 128 columns.  Between 56 and 376 shared rows and between 64 and 128 columns the
// call was not measured: the thresholds are the smallest measured wins.  Repeated stand-alone launches (--kernel, K / V in cache) flatter the kernel: there it
// already wins at 64 columns with 8 own rows.  DESIGN.md 4.7 has the tables.)
constexpr int PREFIX_ATTN_MIN_COLS = 128, PREFIX_ATTN_MIN_SHARED = 376;
constexpr int MFMA_MIN_DECODE_COLS = 48, MFMA_MIN_PASS_COLS = 64, GROUPED_ATTN_MIN_COLS = 80, SLIM_ATTN_MIN_COLS = 48, SPLIT_ATTN_ABOVE_KEYS = 256;

// ---- a forward pass, by name --------------------------------------------------------------------------------------------------------------
// Hidden rows (biogpt_hip_hidden / biogpt_hip_embed_batch): the first `layers` layers only, then the final LayerNorm of every column as f32 rows
// into ln_out; ln_out == null: no LayerNorm either, the rows are the residual stream c->x itself.
// scatter_div > 0 (packed columns): column i's row goes to row (seq_id / scatter_div) * n_positions + n_past of ln_out -- the context store of contrastive search.
struct HiddenStage { int layers; float *ln_out; int scatter_div = 0; };

// What enqueue_forward runs.  Only the named constructors build one, so a combination they do not name -- shared-prefix attention without column
// states, "logits from column k on" outside scoring -- cannot reach the launch code.
struct ForwardPass {
    enum class Cols {       // where the columns come from, and whose K / V cache they use
        Context,            // the context's own: c->state, memory_k / memory_v
        PerSequence,        // one column per sequence (a decode step of many sequences): c->seq, bk / bv
        Packed,             // packed column states (tokens of several sequences, each with its seq_id / t_vis): c->cols, bk / bv
    };
    enum class Rows {       // which rows are wanted at the end
        Last,               // the last column's logits into c->logits, with the arg-max partials
        AllGeneric,         // every column's logits into logits_all on the generic kernel (biogpt_hip_eval_all)
        All,                // every column's logits into logits_all on the fastest lm_head for the model: LayerNorm+Q8 once, then the 8-column / matrix-core
                            // lm_head where the many-column chain applies, the generic kernel otherwise (biogpt_hip_score*, the decode steps of many sequences)
        None,               // none: only the K / V rows matter (the caller gets the logits from the following decode step)
        Hidden,             // no logits at all: `hid`
    };
    int n_cols, t_max;
    Cols cols;
    Rows rows;
    HiddenStage hid;        // Rows::Hidden; with other rows and ln_out != null: the final-LayerNorm f32 rows of every column BESIDE those rows (contrastive search)
    // Packed columns (biogpt_hip_score_continuations, the prompts of biogpt_hip_generate_*_prefix) and the decode steps behind a shared prefix
    // (decode_step_shared): the columns read their first SeqState::pad[0] K / V rows from the slot SeqState::pad[1]
    // (attn_fast_kernel<.., SHARED>); packed columns with logits: only the columns from head_from on get logits (rows 0 .. n_cols - head_from of logits_all): the columns in
    // front of them are prefix columns whose K / V rows alone matter
    bool shared_prefix;
    int head_from;
    int shared_rows = 0;    // decode_step_shared
    const bgk::SeqState *col_states = nullptr;      // Packed: the column states where they are not c->cols (packed_verify)
    // packed_continuations of biogpt_hip_score_continuations_batch: the pass's run table on the device ([n_runs][4]: c0, n, R, S); n_runs > 0: the
    // attention of the pass is attn_runs_kernel.  No other call sets it.
    const int32_t *runs = nullptr;
    int n_runs = 0;

    // the context's own columns
    static ForwardPass last_row(int n, int t_max) { return {n, t_max, Cols::Context, Rows::Last}; }
    static ForwardPass every_row(int n, int t_max) { return {n, t_max, Cols::Context, Rows::AllGeneric}; }
    static ForwardPass scored(int n, int t_max) { return {n, t_max, Cols::Context, Rows::All}; }
    static ForwardPass hidden(int n, int t_max, HiddenStage hs) { return {n, t_max, Cols::Context, Rows::Hidden, hs}; }
    // one decode step of n_seqs sequences, every sequence's row
    static ForwardPass decode_step(int n_seqs, int t_max) { return {n_seqs, t_max, Cols::PerSequence, Rows::All}; }
    // the same behind a shared prefix: every sequence reads its first SeqState::pad[0] K / V rows in the slot SeqState::pad[1], where they were evaluated once
    // shared_rows: how many, for the choice of the attention kernel alone -- the kernels read the number from the column states, so a captured step stays
    // right (if not the fastest choice) for a call whose prefix has another length
    static ForwardPass decode_step_shared(int n_seqs, int t_max, int shared_rows) {
        ForwardPass p{n_seqs, t_max, Cols::PerSequence, Rows::All, HiddenStage{0, nullptr}, true};
        p.shared_rows = shared_rows;
        return p;
    }
    // the same, and every sequence's hidden row into ln_out [n_seqs][d_model]
    static ForwardPass decode_step_hidden(int n_seqs, int t_max, float *ln_out) { return {n_seqs, t_max, Cols::PerSequence, Rows::All, HiddenStage{0, ln_out}}; }
    // packed columns (c->cols)
    static ForwardPass packed_prompts(int n, int t_max) { return {n, t_max, Cols::Packed, Rows::None}; }
    // the same, and every column's hidden row scattered into store[(seq_id / per_prompt) * n_positions + n_past]; store == null: packed_prompts
    static ForwardPass packed_prompts_hidden(int n, int t_max, float *store, int per_prompt) {
        return {n, t_max, Cols::Packed, Rows::None, HiddenStage{0, store, per_prompt}};
    }
    static ForwardPass packed_scored(int n, int t_max) { return {n, t_max, Cols::Packed, Rows::All}; }
    // the same over column states a kernel of the captured step has written (prompt-lookup decoding: a sequence's current token and its drafted tokens at
    // consecutive positions, t_vis = position + 1); `cols` keeps its address for as long as a graph holds the pass
    static ForwardPass packed_verify(int n, int t_max, const bgk::SeqState *cols) {
        ForwardPass p{n, t_max, Cols::Packed, Rows::All};
        p.col_states = cols;
        return p;
    }
    static ForwardPass packed_hidden(int n, int t_max, HiddenStage hs) { return {n, t_max, Cols::Packed, Rows::Hidden, hs}; }
    // the first n_prefix columns are prefix columns (all of them: no lm_head at all), the others read the prefix in place
    static ForwardPass packed_continuations(int n, int t_max, int n_prefix) {
        return {n, t_max, Cols::Packed, n_prefix < n ? Rows::All : Rows::None, HiddenStage{0, nullptr}, true, n_prefix < n ? n_prefix : 0};
    }

private:
    ForwardPass(int n, int t, Cols c, Rows r, HiddenStage h = HiddenStage{0, nullptr}, bool shared = false, int from = 0)
        : n_cols(n), t_max(t), cols(c), rows(r), hid(h), shared_prefix(shared), head_from(from) {}
};

// what the launches of one pass share: derived once from the pass and the model (enqueue_forward)
struct PassLaunch {
    biogpt_hip_ctx *c;
    const ForwardPass &pass;
    hipStream_t st;
    int N, D, F, V, H, P, dk;
    int attn_threads;               // attention workgroup size of the generic kernel
    bool chain, pchain, mfma;       // the single-token fast chain; its many-column form; on the int8 matrix cores
    bool wchain;                    // the wide chain: a pass over column states of a block-quantized file that is not BioGPT-base (kernels_mfma_wide.hip.h)
    bool fchain;                    // the float chain: a pass over column states of an F32 / F16 file whose context has it switched on (kernels_fchain.hip.h)
    bool simd;                      // the context is in the SIMD association: the generic sites launch the kernels of kernels_assoc.hip.h
    bool schain;                    // the SIMD chain: a pass over column states of a context in the SIMD association that has it switched on (kernels_schain.hip.h)
    int q81;
    const bgk::SeqState *seq;       // column states of a pass over the per-sequence caches (null: the context's own columns)
    int col_mode;                   // 1: packed columns
    int64_t seq_stride;
    float *kroot, *vroot;
    bgk::DevMatrix img;
    // a matrix whose rows are no whole 16-row tiles (an lm_head of a vocabulary that is no multiple of 16) has no image: it stays on the 8-column kernel
    const bgk::DevMatrix *tile(const MatSlot &m) { if (!mfma || !tile_image_ok(m)) return nullptr; img = tile_matrix(c, m); return &img; }
    // a generic site's launch: whichever kernel launch_mv picks for the type and shape, or the SIMD association's mat-vec
    template <int PRO, int EPI>
    hipError_t mv(const bgk::MatvecParams &p, const MvShape &s) {
        return simd ? launch_mv_simd<PRO, EPI>(p, st) : launch_mv<PRO, EPI>(c->opt, p, s, st);
    }
    // one launch of the chain; counts the ones that went to the matrix cores
    hipError_t chain_launch(ChainOp op, const bgk::MatvecParams &p, const bgk::DevMatrix *image = nullptr) {
        ChainLaunch rep{};
        const hipError_t e = launch_chain(op, p, st, image, &rep);
        if (e == hipSuccess && rep.kernel >= CK_MFMA_1) c->mfma_launches++;
        return e;
    }
    // The wide chain's stage: the N columns' Q8 blocks into side buffer `slot` (LayerNorm first when ln_w is given), then the matrix-core kernel on the padded image.
    // x: the f32 rows [N][W.K] the stage reads
    hipError_t wide_stage(int epi, bgk::MatvecParams &p, const MatSlot &m, const float *x, int slot, const float *ln_w = nullptr, const float *ln_b = nullptr) {
        hipError_t e = (hipError_t)bg_wide_quantize(x, (int)m.K, (int)m.K, p.N, ln_w, ln_b, 1e-5f, q81, c->aq_q[slot], c->aq_d[slot], c->aq_s[slot], st);
        if (e != hipSuccess) return e;
        p.aq_q = c->aq_q[slot]; p.aq_d = c->aq_d[slot]; p.aq_s = c->aq_s[slot];
        img = tile_matrix(c, m);
        e = (hipError_t)bg_wide_launch(m.type, epi, &p, sizeof(p), &img, sizeof(img), st);
        if (e == hipSuccess) c->wide_launches++;
        return e;
    }
    // The float chain's stage on the row-major weights of the arena.  x: the f32 rows [N][W.K] the stage reads; ln_w given: LayerNorm ONCE per column first
    // (fchain_ln_kernel) into c->att, which no launch between a LayerNorm site and the stage behind it reads or writes (the attention output lives there from
    // the attention launch to out_proj only).  The fp16 rounding of an F16 file's activation rows is the stage's own staging loop's.
    hipError_t float_stage(int epi, bgk::MatvecParams &p, const MatSlot &m, const float *x, const float *ln_w = nullptr, const float *ln_b = nullptr) {
        if (ln_w) {
            const hipError_t e = (hipError_t)bg_fchain_ln(m.type, x, (int)m.K, (int)m.K, p.N, ln_w, ln_b, 1e-5f, c->att, st);
            if (e != hipSuccess) return e;
            x = c->att;
        }
        p.x = x; p.ldx = (int32_t)m.K;
        const hipError_t e = (hipError_t)bg_fchain_launch(m.type, epi, &p, sizeof(p), -1, st, nullptr);
        if (e == hipSuccess) c->float_launches++;
        return e;
    }
    // The SIMD chain's stage: the N columns' Q8 blocks in the SIMD association's form into side buffer `slot` by ONE producer launch (LayerNorm first when ln_w
    // is given), then schain_kernel on the arena's own block rows.  x: the f32 rows [N][W.K] the stage reads
    hipError_t simd_stage(int epi, bgk::MatvecParams &p, const MatSlot &m, const float *x, int slot, const float *ln_w = nullptr, const float *ln_b = nullptr) {
        hipError_t e = (hipError_t)bg_schain_q8(q81, x, (int)m.K, (int)m.K, p.N, ln_w, ln_b, 1e-5f, c->aq_q[slot], c->aq_d[slot], c->aq_s[slot], st, nullptr);
        if (e != hipSuccess) return e;
        p.aq_q = c->aq_q[slot]; p.aq_d = c->aq_d[slot]; p.aq_s = c->aq_s[slot];
        e = (hipError_t)bg_schain_launch(m.type, epi, &p, sizeof(p), -1, st, nullptr);
        if (e == hipSuccess) c->simd_chain_launches++;
        return e;
    }
};

// ---- the stand-alone attention launches ---------------------------------------------------------------------------------------------------
// Which kernel a launch is, and its geometry: what the launch helpers below report.  enqueue_attention and the probe of single kernels
// (biogpt_hip_attn_device, engine_probe.inc) launch through the same helpers, so the probe's launch is the engine's.
enum AttnKernel : int {
    AK_FAST_1 = 0, AK_FAST_2 = 1, AK_FAST_4 = 2, AK_FAST_SLIM = 3,      // attn_fast_kernel<1, true>, <2, false>, <4, false> at 1024 threads, <4, false> as the slim launch
    AK_FAST_SHARED = 4,                                                  // + the four above: their SHARED instantiations
    AK_PREFIX = 8, AK_SPLIT = 9, AK_GROUP = 10, AK_TILE_DMA = 11, AK_TILE = 12, AK_GENERIC = 13,
    AK_RUNS = 16,                                                        // attn_runs_kernel<8>: no route of biogpt_hip_attn_device (its probe is biogpt_hip_attn_runs_device)
    AK_SIMD = 17,                                                        // attn_simd_kernel: the SIMD association's (its probe is biogpt_hip_assoc_device)
};
struct AttnLaunch { int kernel, threads, grid_x, grid_y; size_t lds; };

// the load bound t_cap of a launch: a pass of many query columns takes its keys as they are; the per-column kernels whole waves (= P when the table is not a multiple of 64)
inline int attn_pass_t_cap(int P, int t_max) { return std::min(P, t_max); }
inline int attn_decode_t_cap(int P, int t_max) { return std::min(P, (t_max + 63) & ~63); }
// the tile kernel addresses a thread's four consecutive key rows from ONE base clamped to P - 4: that is only their own rows when 4 | P and P >= 4;
// any other table size takes the grouped kernel, 8 queries per workgroup, which clamps row by row
inline bool attn_tile_table_ok(int P) { return (P & 3) == 0 && P >= 4; }
// workgroup size of the generic kernel: a thread owns up to ATTN_MAXK whole keys, so T <= 4 * threads; ~1 key per thread when possible
inline int attn_generic_threads(int t_max) {
    int nt = 256;
    while (nt < 1024 && t_max > nt) nt <<= 1;
    return nt;
}
inline bool attn_generic_ok(int threads, int dk, int t_max) { return threads % dk == 0 && t_max <= bgk::ATTN_MAXK * threads; }

// attn_fast_kernel's launch table: 4 lanes per key, 16 prefetched V rows per lane
// slim: many (sequence, head) workgroups: throughput over latency -- one lane quad per 4 keys (4 key passes), a
// quarter of the threads, four times as many workgroups resident per compute unit
inline AttnLaunch attn_fast_geometry(int t_cap, bool slim, bool shared, int H, int N) {
    const int t64 = (t_cap + 63) & ~63, sh = shared ? AK_FAST_SHARED : 0;
    if (slim) return {AK_FAST_SLIM + sh, std::max(256, t64), H, N, 0};
    if (t_cap <= 256) return {AK_FAST_1 + sh, 4 * t64, H, N, 0};
    if (t_cap <= 512) return {AK_FAST_2 + sh, 1024, H, N, 0};
    return {AK_FAST_4 + sh, 1024, H, N, 0};
}
// SHARED: the instantiations that take a column's first rows from the shared slot
template <bool SHARED>
AttnLaunch launch_attn_fast(const bgk::AttnParams &a, bool slim, int H, int N, hipStream_t st) {
    const AttnLaunch g = attn_fast_geometry(a.t_cap, slim, SHARED, H, N);
    const dim3 grid(g.grid_x, g.grid_y), block(g.threads);
    switch (g.kernel & 3) {
    case AK_FAST_SLIM: hipLaunchKernelGGL((bgk::attn_fast_kernel<4, false, SHARED>), grid, block, 0, st, a); break;
    case AK_FAST_1: hipLaunchKernelGGL((bgk::attn_fast_kernel<1, true, SHARED>), grid, block, 0, st, a); break;
    case AK_FAST_2: hipLaunchKernelGGL((bgk::attn_fast_kernel<2, false, SHARED>), grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL((bgk::attn_fast_kernel<4, false, SHARED>), grid, block, 0, st, a); break;
    }
    return g;
}
// a decode step behind ONE shared prefix: eight columns per workgroup load a shared row once
inline AttnLaunch launch_attn_prefix(const bgk::AttnParams &a, int H, int N, hipStream_t st) {
    const AttnLaunch g{AK_PREFIX, 512, H, (N + 7) / 8, 0};
    hipLaunchKernelGGL((bgk::attn_prefix_kernel<8>), dim3(g.grid_x, g.grid_y), dim3(g.threads), 0, st, a);
    return g;
}
// packed columns in runs of up to eight that share their first rows (biogpt_hip_score_continuations_batch): one workgroup per (head, run)
inline AttnLaunch launch_attn_runs(const bgk::AttnParams &a, const int32_t *runs, int n_runs, int H, hipStream_t st) {
    const AttnLaunch g{AK_RUNS, 512, H, n_runs, 0};
    const bgk::AttnRunsParams rp{a, runs};
    hipLaunchKernelGGL((bgk::attn_runs_kernel<8>), dim3(g.grid_x, g.grid_y), dim3(g.threads), 0, st, rp);
    return g;
}
// The planner of attn_runs_kernel: the columns of a packed pass (col_mode 1), walked greedily into runs {c0, n, R, S} -- a run is cut at 8 columns or
// at the first column that does not fit.  A column without shared rows (pad[0] == 0) starts or joins a prefix run of its seq_id (S = seq_id, R = the
// smallest t_vis of the run); a column with pad[0] > 0 a continuation run of its (pad[0], pad[1]) (S = pad[1], R = pad[0]).  A column that sees fewer
// rows than pad[0] stands alone with R = t_vis.  Returns the number of runs; runs_out holds up to N.
inline int attn_runs_plan(const bgk::SeqState *st, int N, int32_t *runs_out) {
    int n_runs = 0;
    for (int i = 0; i < N;) {
        const bgk::SeqState &f = st[i];
        const bool pre = f.pad[0] <= 0;
        int n = 1, R = pre ? f.t_vis : std::min(f.pad[0], f.t_vis);
        if (pre || f.t_vis >= f.pad[0]) {
            for (; n < bgk::RUNS_MAX_COLS && i + n < N; n++) {
                const bgk::SeqState &c = st[i + n];
                if (pre ? !(c.pad[0] <= 0 && c.seq_id == f.seq_id) : !(c.pad[0] == f.pad[0] && c.pad[1] == f.pad[1] && c.t_vis >= c.pad[0])) break;
                if (pre) R = std::min(R, c.t_vis);
            }
        }
        int32_t *r = runs_out + 4 * (size_t)n_runs++;
        r[0] = i; r[1] = n; r[2] = R; r[3] = pre ? f.seq_id : f.pad[1];
        i += n;
    }
    return n_runs;
}
// a pass of many query columns: register-tiled kernel, 16 queries per workgroup share every K / V row they load (tables with attn_tile_table_ok)
// lds_done: the kernels whose > 64 KB dynamic-LDS opt-in attribute is set on this device
inline bool launch_attn_tile(const bgk::AttnParams &a, int H, int N, hipStream_t st, std::set<const void *> &lds_done, AttnLaunch *out) {
    // up to 640 keys the K / V rows of the two MAC loops travel through a ring in LDS, two steps ahead (global_load_lds); beyond, the ring has no room
    // beside the scores in a 2-workgroups-per-compute-unit footprint: loads at the top of each step
    const bool dma = bgk::attn_tile_dma_ok(a.t_cap);
    const size_t smb = bgk::attn_tile_smem_bytes<16>(a.t_cap);
    const void *fn = dma ? reinterpret_cast<const void *>(bgk::attn_tile_kernel<16, true>) : reinterpret_cast<const void *>(bgk::attn_tile_kernel<16, false>);
    if (smb > 64 * 1024 && !lds_done.count(fn)) {
        HIP_TRY(false, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bgk::attn_tile_smem_bytes<16>(a.P)));
        lds_done.insert(fn);
    }
    const AttnLaunch g{dma ? AK_TILE_DMA : AK_TILE, 512, H, (N + 15) / 16, smb};
    if (dma) hipLaunchKernelGGL((bgk::attn_tile_kernel<16, true>), dim3(g.grid_x, g.grid_y), dim3(g.threads), smb, st, a);
    else hipLaunchKernelGGL((bgk::attn_tile_kernel<16, false>), dim3(g.grid_x, g.grid_y), dim3(g.threads), smb, st, a);
    if (out) *out = g;
    return true;
}
inline AttnLaunch launch_attn_group(const bgk::AttnParams &a, int H, int N, hipStream_t st) {
    const AttnLaunch g{AK_GROUP, 512, H, (N + 7) / 8, bgk::attn_group_smem_bytes(a.t_cap)};
    hipLaunchKernelGGL((bgk::attn_group_kernel<8>), dim3(g.grid_x, g.grid_y), dim3(g.threads), g.lds, st, a);
    return g;
}
// long context, one query: spread the head's keys over the chip (three dependent launches); a.sp_* are the caller's scratch, a.n_split is set here
inline bool launch_attn_split(bgk::AttnParams &a, int H, hipStream_t st, AttnLaunch *out) {
    a.n_split = (a.t_cap + bgk::SPLIT_KEYS - 1) / bgk::SPLIT_KEYS;
    if (a.n_split > bgk::SPLIT_MAX) BG_FAIL(false, "internal: %d key ranges exceed the %d the split attention kernels hold", a.n_split, bgk::SPLIT_MAX);
    hipLaunchKernelGGL(bgk::attn_split_scores_kernel, dim3(H, a.n_split), dim3(256), 0, st, a);
    hipLaunchKernelGGL(bgk::attn_split_pv_kernel, dim3(H, a.n_split), dim3(256), 0, st, a);
    hipLaunchKernelGGL(bgk::attn_split_combine_kernel, dim3(H), dim3(64), 0, st, a);
    if (out) *out = {AK_SPLIT, 256, H, a.n_split, 0};
    return true;
}
inline AttnLaunch launch_attn_generic(const bgk::AttnParams &a, int H, int N, int threads, hipStream_t st) {
    const AttnLaunch g{AK_GENERIC, threads, H, N, bgk::attn_smem_bytes(a.P, a.dk, threads)};
    hipLaunchKernelGGL(bgk::attn_kernel, dim3(g.grid_x, g.grid_y), dim3(g.threads), g.lds, st, a);
    return g;
}
// the SIMD association's attention (kernels_assoc.hip.h): head size 64, up to SIMD_ATTN_MAXT keys; lds: its static LDS
inline AttnLaunch launch_attn_simd(const bgk::AttnParams &a, int H, int N, hipStream_t st) {
    const AttnLaunch g{AK_SIMD, 256, H, N, 64 * 4 + bgk::SIMD_ATTN_MAXT * 4 + 32 * 64 * 4 + 16 * 8};
    hipLaunchKernelGGL(bgk::attn_simd_kernel, dim3(g.grid_x, g.grid_y), dim3(g.threads), 0, st, a);
    return g;
}

// the attention launch(es) of layer l
bool enqueue_attention(PassLaunch &k, int l) {
    biogpt_hip_ctx *c = k.c;
    const int N = k.N, D = k.D, H = k.H, P = k.P, dk = k.dk, t_max = k.pass.t_max;
    const bool batch = k.seq != nullptr;
    hipStream_t st = k.st;
    bgk::AttnParams a{};
    a.q = c->q; a.kcache = k.kroot + (size_t)l * P * D; a.vcache = k.vroot + (size_t)l * P * D;
    if (batch) { a.seq = k.seq; a.col_mode = k.col_mode; a.kv_seq_stride = k.seq_stride; }
    a.out = c->att; a.st = c->state;
    a.exp_tab = reinterpret_cast<const uint16_t *>(c->arena + c->plan.exp_tab);
    a.N = N; a.D = D; a.dk = dk; a.P = P;
    a.dbg = c->opt.dbg; a.tstamp = c->tstamp;
    a.q81 = k.q81;
    if (k.chain) { a.oq_q = c->aq_q[0]; a.oq_d = c->aq_d[0]; a.oq_s = c->aq_s[0]; }
    if (k.simd) {      // (head size 64 and t_max <= SIMD_ATTN_MAXT: enqueue_forward)
        launch_attn_simd(a, H, N, st);
        return true;
    }
    if (k.schain) {    // (likewise; the columns' slots, counts and shared rows are the column states')
        HIP_TRY(false, (hipError_t)bg_schain_attn(&a, sizeof(a), k.pass.shared_prefix ? 1 : 0, H, N, st, nullptr));
        return true;
    }
    if (!(dk == 64 && t_max <= 1024)) {
        launch_attn_generic(a, H, N, k.attn_threads, st);
        return true;
    }
    if (!batch && N >= GROUPED_ATTN_MIN_COLS) {
        a.t_cap = attn_pass_t_cap(P, t_max);
        if (attn_tile_table_ok(P)) return launch_attn_tile(a, H, N, st, c->lds_attr_done, nullptr);
        launch_attn_group(a, H, N, st);
        return true;
    }
    // loads are bounded by t_cap
    a.t_cap = attn_decode_t_cap(P, t_max);
    if (N == 1 && !batch && a.t_cap > SPLIT_ATTN_ABOVE_KEYS) {
        a.sp_scores = c->sp_scores; a.sp_max = c->sp_max; a.sp_pv = c->sp_pv;
        return launch_attn_split(a, H, st, nullptr);
    }
    if (k.pass.n_runs > 0) {      // biogpt_hip_score_continuations_batch decided per pass (run_attn); t_cap <= 1024 here
        launch_attn_runs(a, k.pass.runs, k.pass.n_runs, H, st);
        return true;
    }
    const bool slim = batch && N >= SLIM_ATTN_MIN_COLS;
    const bool grouped = k.pass.shared_prefix && k.pass.cols == ForwardPass::Cols::PerSequence && a.t_cap <= bgk::PFX_MAX_KEYS &&
                         (c->opt.prefix_attn < 0 ? N >= PREFIX_ATTN_MIN_COLS && k.pass.shared_rows >= PREFIX_ATTN_MIN_SHARED : c->opt.prefix_attn == 1);
    if (grouped) launch_attn_prefix(a, H, N, st);
    else if (k.pass.shared_prefix) launch_attn_fast<true>(a, slim, H, N, st);
    else launch_attn_fast<false>(a, slim, H, N, st);
    return true;
}

// layer l on the chain of launches: q/k/v, attention, out_proj, fc1, fc2
bool enqueue_layer(PassLaunch &k, int l) {
    biogpt_hip_ctx *c = k.c;
    const int N = k.N, D = k.D, F = k.F, P = k.P;
    hipStream_t st = k.st;
    const LayerSlots &L = c->plan.layers[(size_t)l];
    {  // LN0 + fused q/k/v projection + bias + Q scale + KV append
        const MvShape s = mv_shape(L.qkv.type, L.qkv.M, L.qkv.K);
        bgk::MatvecParams p = mv_base(c, L.qkv, s);
        p.x = c->x; p.ldx = D; p.N = N;
        p.ln_w = dev_vec(c, L.ln0_w); p.ln_b = dev_vec(c, L.ln0_b);
        p.bias = dev_vec(c, L.qkv_b);
        p.q_out = c->q;
        p.kcache = k.kroot + (size_t)l * P * D;
        p.vcache = k.vroot + (size_t)l * P * D;
        if (k.seq) { p.seq = k.seq; p.col_mode = k.col_mode; p.kv_seq_stride = k.seq_stride; }
        p.q_scale = 1.0f / sqrtf((float)k.dk);
        if (k.schain) {
            HIP_TRY(false, k.simd_stage(bgk::EPI_QKV, p, L.qkv, c->x, 2, p.ln_w, p.ln_b));
        } else if (k.fchain) {
            HIP_TRY(false, k.float_stage(bgk::EPI_QKV, p, L.qkv, c->x, p.ln_w, p.ln_b));
        } else if (k.wchain) {
            HIP_TRY(false, k.wide_stage(bgk::EPI_QKV, p, L.qkv, c->x, 2, p.ln_w, p.ln_b));
        } else if (k.pchain) {
            HIP_TRY(false, launch_lnq(c, c->x, N, L.ln0_w, L.ln0_b, k.q81, st));
            p.aq_q = c->aq_q[2]; p.aq_d = c->aq_d[2]; p.aq_s = c->aq_s[2];
            HIP_TRY(false, k.chain_launch(CHAIN_QKV_Q8, p, k.tile(L.qkv)));
        } else {
            HIP_TRY(false, (k.mv<bgk::PRO_LN, bgk::EPI_QKV>(p, s)));
        }
    }
    if (!enqueue_attention(k, l)) return false;
    {  // out_proj + bias + residual
        const MvShape s = mv_shape(L.o.type, L.o.M, L.o.K);
        bgk::MatvecParams p = mv_base(c, L.o, s);
        p.x = c->att; p.ldx = D; p.N = N;
        p.bias = dev_vec(c, L.o_b);
        p.resid = c->x; p.ldr = D; p.out = c->x1; p.ldo = D;
        if (k.schain) {
            HIP_TRY(false, k.simd_stage(bgk::EPI_RESID, p, L.o, c->att, 0));
        } else if (k.fchain) {
            HIP_TRY(false, k.float_stage(bgk::EPI_RESID, p, L.o, c->att));
        } else if (k.wchain) {      // (the attention kernels wrote f32 rows: no Q8 side output without the base chain)
            HIP_TRY(false, k.wide_stage(bgk::EPI_RESID, p, L.o, c->att, 0));
        } else if (k.chain) {
            p.aq_q = c->aq_q[0]; p.aq_d = c->aq_d[0]; p.aq_s = c->aq_s[0];
            HIP_TRY(false, k.chain_launch(CHAIN_OPROJ, p, k.tile(L.o)));
        } else {
            HIP_TRY(false, (k.mv<bgk::PRO_PLAIN, bgk::EPI_RESID>(p, s)));
        }
    }
    {  // LN1 + fc1 + bias + GELU
        const MvShape s = mv_shape(L.fc1.type, L.fc1.M, L.fc1.K);
        bgk::MatvecParams p = mv_base(c, L.fc1, s);
        p.x = c->x1; p.ldx = D; p.N = N;
        p.ln_w = dev_vec(c, L.ln1_w); p.ln_b = dev_vec(c, L.ln1_b);
        p.bias = dev_vec(c, L.fc1_b);
        p.out = c->h; p.ldo = F;
        if (k.schain) {
            HIP_TRY(false, k.simd_stage(bgk::EPI_GELU, p, L.fc1, c->x1, 2, p.ln_w, p.ln_b));
        } else if (k.fchain) {
            HIP_TRY(false, k.float_stage(bgk::EPI_GELU, p, L.fc1, c->x1, p.ln_w, p.ln_b));
        } else if (k.wchain) {
            HIP_TRY(false, k.wide_stage(bgk::EPI_GELU, p, L.fc1, c->x1, 2, p.ln_w, p.ln_b));
        } else if (k.pchain) {
            HIP_TRY(false, launch_lnq(c, c->x1, N, L.ln1_w, L.ln1_b, k.q81, st));
            p.aq_q = c->aq_q[2]; p.aq_d = c->aq_d[2]; p.aq_s = c->aq_s[2];
            p.oq_q = c->aq_q[1]; p.oq_d = c->aq_d[1]; p.oq_s = c->aq_s[1];
            HIP_TRY(false, k.chain_launch(CHAIN_FC1_Q8, p, k.tile(L.fc1)));
        } else if (k.chain) {
            p.oq_q = c->aq_q[1]; p.oq_d = c->aq_d[1]; p.oq_s = c->aq_s[1];
            HIP_TRY(false, k.chain_launch(CHAIN_FC1, p));
        } else {
            HIP_TRY(false, (k.mv<bgk::PRO_LN, bgk::EPI_GELU>(p, s)));
        }
    }
    {  // fc2 + bias + residual
        const MvShape s = mv_shape(L.fc2.type, L.fc2.M, L.fc2.K);
        bgk::MatvecParams p = mv_base(c, L.fc2, s);
        p.x = c->h; p.ldx = F; p.N = N;
        p.bias = dev_vec(c, L.fc2_b);
        p.resid = c->x1; p.ldr = D; p.out = c->x; p.ldo = D;
        if (k.schain) {
            HIP_TRY(false, k.simd_stage(bgk::EPI_RESID, p, L.fc2, c->h, 1));
        } else if (k.fchain) {
            HIP_TRY(false, k.float_stage(bgk::EPI_RESID, p, L.fc2, c->h));
        } else if (k.wchain) {
            HIP_TRY(false, k.wide_stage(bgk::EPI_RESID, p, L.fc2, c->h, 1));
        } else if (k.chain) {
            p.aq_q = c->aq_q[1]; p.aq_d = c->aq_d[1]; p.aq_s = c->aq_s[1];
            HIP_TRY(false, k.chain_launch(CHAIN_FC2, p, k.tile(L.fc2)));
        } else {
            HIP_TRY(false, (k.mv<bgk::PRO_PLAIN, bgk::EPI_RESID>(p, s)));
        }
    }
    return true;
}

// ---- the launches of the embedding tail (kernels_embed.hip.h) ----
// enqueue_final, embed_batch_once and enqueue_head launch through these, and so does the probe of the four kernels alone (biogpt_hip_embed_device,
// engine_probe.inc): the probe's launch is the engine's.  rep: null, or what was launched (kernel: EK_*; for ln_rows_kernel the template argument).
enum EmbedKernel : int { EK_LN_GENERIC = 0, EK_POOL_ROWS = 1, EK_POOL_FINISH = 2, EK_HEAD_ROWS = 3, EK_LN_1024 = 1024 };
struct EmbedLaunch { int32_t kernel, threads, grid_x, grid_y, lds; };      // lds: dynamic LDS bytes
constexpr size_t HEAD_LDS_MAX = 65536;      // the dynamic LDS a launch gets without an attribute of its own
// head_rows_kernel keeps 8 rows of the width in LDS: the widths it can be launched at (no HIP call: an argument error of the call)
inline bool check_head_width(int W) {
    if ((size_t)bgk::HEAD_ROWS * (size_t)W * 4 > HEAD_LDS_MAX)
        BG_FAIL(false, "a head over rows of width %d needs %zu bytes of LDS (%d rows x 4 bytes): more than the %zu a launch gets (width at most %zu)", W,
                (size_t)bgk::HEAD_ROWS * (size_t)W * 4, bgk::HEAD_ROWS, HEAD_LDS_MAX, HEAD_LDS_MAX / 4 / bgk::HEAD_ROWS);
    return true;
}
inline hipError_t launch_ln_rows(hipStream_t st, const float *x, int ldx, int K, int N, const float *lw, const float *lb, float *out, const bgk::SeqState *cols,
                                 int slot_div, int P, EmbedLaunch *rep = nullptr) {
    if (rep) *rep = EmbedLaunch{K == 1024 ? EK_LN_1024 : EK_LN_GENERIC, 256, N, 1, 0};
    if (K == 1024) hipLaunchKernelGGL((bgk::ln_rows_kernel<1024>), dim3(N), dim3(256), 0, st, x, ldx, K, lw, lb, 1e-5f, 1.0 / 1024.0, out, cols, slot_div, P);
    else hipLaunchKernelGGL((bgk::ln_rows_kernel<0>), dim3(N), dim3(256), 0, st, x, ldx, K, lw, lb, 1e-5f, 1.0 / (double)K, out, cols, slot_div, P);
    return hipGetLastError();
}
inline hipError_t launch_pool_rows(hipStream_t st, const float *rows, int n_cols, int W, const bgk::SeqState *cols, const int32_t *lens, int mode, float *out,
                                   double *acc, EmbedLaunch *rep = nullptr) {
    const dim3 grid((unsigned)((W + 63) / 64), (unsigned)n_cols);
    if (rep) *rep = EmbedLaunch{EK_POOL_ROWS, 256, (int32_t)grid.x, (int32_t)grid.y, 0};
    hipLaunchKernelGGL(bgk::pool_rows_kernel, grid, dim3(256), 0, st, rows, n_cols, W, cols, lens, mode, out, acc);
    return hipGetLastError();
}
// does a call launch pool_finish_kernel at all: when there is a mean to take or a row to normalise
inline bool pool_needs_finish(const double *acc, int normalize) { return acc != nullptr || normalize != 0; }
inline hipError_t launch_pool_finish(hipStream_t st, float *out, int n_rows, int W, const double *acc, const int32_t *lens, int normalize, EmbedLaunch *rep = nullptr) {
    if (rep) *rep = EmbedLaunch{EK_POOL_FINISH, 256, n_rows, 1, 0};
    hipLaunchKernelGGL(bgk::pool_finish_kernel, dim3((unsigned)n_rows), dim3(256), 0, st, out, W, acc, lens, normalize);
    return hipGetLastError();
}
inline hipError_t launch_head_rows(hipStream_t st, const float *x, int n_rows, int W, const float *w, const float *b, int n_out, float *out, EmbedLaunch *rep = nullptr) {
    const int grid = (n_rows + bgk::HEAD_ROWS - 1) / bgk::HEAD_ROWS;
    const size_t lds = (size_t)bgk::HEAD_ROWS * W * 4;
    if (rep) *rep = EmbedLaunch{EK_HEAD_ROWS, 256, grid, 1, (int32_t)lds};
    hipLaunchKernelGGL(bgk::head_rows_kernel, dim3(grid), dim3(256), lds, st, x, n_rows, W, w, b, n_out, out);
    return hipGetLastError();
}

// the final stage of a pass on the residual stream c->x: the rows the pass names, LayerNorm + lm_head (or the hidden rows in front of it)
bool enqueue_final(PassLaunch &k) {
    using Rows = ForwardPass::Rows;
    biogpt_hip_ctx *c = k.c;
    const int N = k.N, D = k.D, V = k.V;
    hipStream_t st = k.st;
    const Rows rows = k.pass.rows;
    if (float *const ln_out = k.pass.hid.ln_out) {      // f32 rows in front of the lm_head (kernels_embed.hip.h)
        const float *lw = dev_vec(c, c->plan.ln_w), *lb = dev_vec(c, c->plan.ln_b);
        const int div = k.pass.hid.scatter_div;
        const bgk::SeqState *sc = div > 0 ? k.seq : nullptr;
        HIP_TRY(false, launch_ln_rows(st, c->x, D, D, N, lw, lb, ln_out, sc, div, k.P));
    }
    if (rows == Rows::None || rows == Rows::Hidden) return true;   // prompt columns: only the KV rows matter; hidden rows: no lm_head
    const MatSlot &m = c->plan.lm_head;
    const MvShape s = mv_shape(m.type, m.M, m.K);
    bgk::MatvecParams p = mv_base(c, m, s);
    if (rows == Rows::All && k.schain) {  // the SIMD chain: LayerNorm + Q8 of the columns that get a row, once, then the lm_head stage (any n_vocab)
        const int head_from = k.pass.head_from;
        p.N = N - head_from; p.out = c->logits_all; p.ldo = V;
        HIP_TRY(false, k.simd_stage(bgk::EPI_LOGITS, p, m, c->x + (size_t)head_from * D, 2, dev_vec(c, c->plan.ln_w), dev_vec(c, c->plan.ln_b)));
        return true;
    }
    if (rows == Rows::All && k.fchain) {  // the float chain: LayerNorm of the columns that get a row, once, then the lm_head stage (any n_vocab)
        const int head_from = k.pass.head_from;
        p.N = N - head_from; p.out = c->logits_all; p.ldo = V;
        HIP_TRY(false, k.float_stage(bgk::EPI_LOGITS, p, m, c->x + (size_t)head_from * D, dev_vec(c, c->plan.ln_w), dev_vec(c, c->plan.ln_b)));
        return true;
    }
    if (rows == Rows::All && k.wchain) {  // the wide chain: LayerNorm+Q8 of the columns that get a row, then the lm_head on the matrix cores (its last row tile may be partial)
        const int head_from = k.pass.head_from;
        p.N = N - head_from; p.out = c->logits_all; p.ldo = V;
        HIP_TRY(false, k.wide_stage(bgk::EPI_LOGITS, p, m, c->x + (size_t)head_from * D, 2, dev_vec(c, c->plan.ln_w), dev_vec(c, c->plan.ln_b)));
        return true;
    }
    if (rows == Rows::All && k.pchain) {  // every column needs its logits row: LayerNorm+Q8 once, then the 8-column mat-vec (matrix cores from 64 columns)
        // head_from > 0: the kernel a pass of n_rows columns alone would take.  Below 64 rows that is the 8-column VALU kernel, where score_batch of
        // the concatenation (64 columns or more) takes the matrix cores: the bit-for-bit promise of biogpt_hip_score_continuations rests on the two
        // lm_head kernels giving IDENTICAL f32 rows (exact int32 block sums, the same f32 scaling and block order in both) -- as score_batch ==
        // score already does across pass sizes.  A change to either kernel's arithmetic breaks that equality (tests/test_gpu_prefix.py, test_gpu_score.py).
        const int head_from = k.pass.head_from, n_rows = N - head_from;
        HIP_TRY(false, launch_lnq(c, c->x + (size_t)head_from * D, n_rows, c->plan.ln_w, c->plan.ln_b, k.q81, st));
        p.aq_q = c->aq_q[2]; p.aq_d = c->aq_d[2]; p.aq_s = c->aq_s[2];
        p.N = n_rows; p.out = c->logits_all; p.ldo = V;
        HIP_TRY(false, k.chain_launch(CHAIN_LMHEAD_Q8, p, (head_from > 0 && n_rows < MFMA_MIN_PASS_COLS) ? nullptr : k.tile(c->plan.lm_head)));
        return true;
    }
    // final LayerNorm + lm_head on the generic kernel; only the rows that are returned (F8)
    if (rows != Rows::Last) {   // eval_all; scoring of the other models
        p.ln_w = dev_vec(c, c->plan.ln_w); p.ln_b = dev_vec(c, c->plan.ln_b);
        p.ldx = D; p.ldo = V;
        p.x = c->x; p.N = N; p.out = c->logits_all;
        HIP_TRY(false, (k.mv<bgk::PRO_LN, bgk::EPI_LOGITS>(p, s)));
        return true;
    }
    if (s.grid > c->pmax_cap) BG_FAIL(false, "internal: arg-max partial buffer too small (%d > %d)", s.grid, c->pmax_cap);      // (the SIMD launch: at most MATVEC_MAX_GRID <= pmax_cap partials)
    int lm_grid = 0;
    HIP_TRY(false, launch_lm_head_row(c->opt, p, s, c->x + (size_t)(N - 1) * D, dev_vec(c, c->plan.ln_w), dev_vec(c, c->plan.ln_b), c->logits, c->pmax_val, c->pmax_idx, st, &lm_grid,
                                      nullptr, k.simd));
    c->lm_blocks = lm_grid;
    return true;
}

// One forward pass: the embedding, the layers, the final stage -- on the launch that fits the pass (the fused single-token launch and the 2 .. 8-column
// chunk launch for the context's own columns with the last row wanted; the column-per-XCD launch for a decode step of 2 .. 8 sequences; the persistent
// float launch for one token of a float file), otherwise five launches per layer.
bool enqueue_forward(biogpt_hip_ctx *c, const ForwardPass &pass) {
    using Cols = ForwardPass::Cols;
    using Rows = ForwardPass::Rows;
    (void)hipGetLastError();   // a failed call of some OTHER context / API leaves its code behind; the checks below are about these launches
    const int N = pass.n_cols, t_max = pass.t_max;
    // every row but the last is needed elsewhere: none of the launches that keep the activations on chip and compute the last row only
    const bool last_own = pass.cols == Cols::Context && pass.rows == Rows::Last;
    if (N < 1 || N > c->hp.n_positions) BG_FAIL(false, "internal: a pass of %d columns exceeds the %d-column activation scratch", N, c->hp.n_positions);
    if (N == 1 && last_own && fused_decode_ok(c, t_max)) return enqueue_decode_fused(c, t_max, 1, 0);
    if (N >= 2 && N <= 8 && last_own && xcols_usable(c, N, t_max)) return enqueue_xcols(c, N, t_max);
    const auto &hp = c->hp;
    const bool batch = pass.cols != Cols::Context;
    PassLaunch k{c, pass, c->stream};
    k.N = N; k.D = hp.d_model; k.F = hp.d_ff; k.V = hp.n_vocab; k.H = hp.n_head; k.P = hp.n_positions;
    k.dk = k.D / k.H;
    k.attn_threads = attn_generic_threads(t_max);
    if (!attn_generic_ok(k.attn_threads, k.dk, t_max))
        BG_FAIL(false, "context of %d tokens / head size %d not supported by the attention kernel", t_max, k.dk);

    // single-token fast chain: BioGPT-base shapes, block-quantized weights -> producer-side Q8 hand-offs
    const int32_t wt = ftype_to_type(hp.ftype);
    // the SIMD association: the context's own columns on the five launches per layer, no chain; the calls over column states were refused at their entry
    // (with the SIMD chain switched on, the passes over column states run on kernels_schain.hip.h: the same association on many columns)
    k.schain = c->assoc != 0 && batch && chain_kind(c) == CHAIN_SIMD;
    k.simd = c->assoc != 0 && !k.schain;
    if (k.simd && batch) BG_FAIL(false, "internal: a pass over column states reached a context in the SIMD association");
    if (k.schain && (pass.rows == Rows::Last || pass.rows == Rows::AllGeneric)) BG_FAIL(false, "internal: a SIMD chain pass with rows it does not serve");
    if (c->assoc != 0 && (k.dk != 64 || t_max > bgk::SIMD_ATTN_MAXT))
        BG_FAIL(false, "the SIMD association serves head size 64 and contexts of up to %d tokens (got head size %d, %d tokens)", bgk::SIMD_ATTN_MAXT, k.dk, t_max);
    k.chain = c->assoc == 0 && is_quantized(wt) && k.D == 1024 && k.F == 4096 && k.dk == 64 && t_max <= 1024;
    k.pchain = k.chain && (N > 1 || batch);   // several columns: LayerNorm+Q8 once per site (lnq_kernel), 8 columns per workgroup
    // enough columns to fill 16-wide MFMA tiles: the chain runs on the int8 matrix cores from the row-tiled weight image
    k.mfma = k.pchain && N >= (pass.cols == Cols::PerSequence ? MFMA_MIN_DECODE_COLS : MFMA_MIN_PASS_COLS) && c->tile_img != nullptr;
    // a pass over column states of any other block-quantized file with head size 64: the wide chain (the context's own columns stay on the generic kernels)
    k.wchain = !k.chain && !k.schain && batch && chain_kind_of(hp) == CHAIN_WIDE && t_max <= 1024;
    // a pass over column states of a float file whose context has the float chain switched on (the context's own columns stay on fdec_kernel / matvec_kernel)
    k.fchain = !k.chain && !k.wchain && batch && chain_kind(c) == CHAIN_FLOAT && t_max <= 1024;
    if (k.fchain && (pass.rows == Rows::Last || pass.rows == Rows::AllGeneric)) BG_FAIL(false, "internal: a float fast chain pass with rows it does not serve");
    if (batch && !k.chain && !k.wchain && !k.fchain && !k.schain)
        BG_FAIL(false, "batched decode needs the BioGPT-base fast chain (block-quantized weights, d_model 1024, d_ff 4096, head size 64) or the wide one (block-quantized weights, head size 64, d_model a multiple of 64, d_ff of 32)");
    if (k.wchain && (c->tile_img == nullptr || pass.rows == Rows::Last || pass.rows == Rows::AllGeneric))
        BG_FAIL(false, "internal: a wide fast chain pass without its row-tiled weight image, or with rows it does not serve");
    k.seq = pass.cols == Cols::Packed ? (pass.col_states ? pass.col_states : c->cols) : (batch ? c->seq : nullptr);
    k.col_mode = pass.cols == Cols::Packed ? 1 : 0;
    k.seq_stride = (int64_t)hp.n_layer * k.P * k.D;
    k.kroot = batch ? c->bk : c->memory_k;
    k.vroot = batch ? c->bv : c->memory_v;
    k.q81 = (wt == T_Q4_1 || wt == T_Q5_1) ? 1 : 0;

    // a decode step of 2 .. 8 sequences while the caller (biogpt_hip_generate_greedy_batch) holds the device's pipeline slot: embedding + all layers as ONE launch,
    // one sequence per XCD (kernels_xcols.hip.h, streams mode); the rows below on its output
    const bool xc_streams = pass.cols == Cols::PerSequence && c->xc_batch != 0 && t_max <= 256 && xcols_prepare(c, N, t_max);
    if (xc_streams) { if (!enqueue_xcols(c, N, t_max, true)) return false; }
    else
    hipLaunchKernelGGL(bgk::embed_kernel, dim3((k.D + 255) / 256, N), dim3(256), 0, k.st,
                       dev_matrix(c, c->plan.embed_tokens), dev_matrix(c, c->plan.embed_pos), c->state,
                       sqrtf((float)k.D), c->x, k.D, k.seq);
    // a single token of a float-weight file: all layers as ONE persistent launch (kernels_fpipe.hip.h) on the embedding the launch above left in c->x
    const bool fp_one = N == 1 && last_own && !k.chain &&
                        (c->fp_force >= 0 ? (c->fp_force == 1 && c->fp_state == 1 && t_max <= bgk::FP_TMAX) : fpipe_usable(c, t_max));
    if (fp_one && !enqueue_fpipe(c)) return false;
    const int n_run = pass.rows == Rows::Hidden ? pass.hid.layers : hp.n_layer;
    for (int l = 0; l < n_run && !xc_streams && !fp_one; l++)
        if (!enqueue_layer(k, l)) return false;
    return enqueue_final(k);
}

bool enqueue_argmax(biogpt_hip_ctx *c, int n_eval) {
    HIP_TRY(false, launch_argmax(c->pmax_val, c->pmax_idx, c->lm_blocks, c->state, n_eval, c->hp.n_positions, c->hp.n_vocab, c->stream));
    return true;
}

constexpr int STATE_SLOTS = 64;

// Async upload of {n_past, tokens} through a ring of pinned slots (a slot is only reused after the
// stream has drained, so an in-flight copy never sees a half-written slot).
bool upload_state(biogpt_hip_ctx *c, const int32_t *tokens, int n, int n_past, int chunk = 0) {
    if (c->slot_idx == STATE_SLOTS) {
        HIP_TRY(false, hipStreamSynchronize(c->stream));
        c->slot_idx = 0;
    }
    uint8_t *slot = c->state_host + (size_t)c->slot_idx++ * c->slot_bytes;
    auto *hs = reinterpret_cast<bgk::DevState *>(slot);
    hs->n_past = n_past;
    hs->n_gen = 0;
    hs->causal = c->opt.causal;
    hs->chunk = chunk;
    c->state_n_past = n_past; c->state_chunk = chunk;
    std::memcpy(slot + sizeof(bgk::DevState), tokens, (size_t)n * 4);
    HIP_TRY(false, hipMemcpyAsync(c->state, slot, sizeof(bgk::DevState) + (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    return true;
}

// While a queue session is open its context serves nothing else: the session's columns, K / V slots and captured steps persist between its calls
bool session_refuses(const biogpt_hip_ctx *c) {
    if (c->session) BG_FAIL(true, "a queue session is open on this context (biogpt_hip_queue_open): it has the context to itself until biogpt_hip_queue_close");
    return false;
}

bool check_eval_args(const biogpt_hip_ctx *c, const int32_t *tokens, int n, int n_past) {
    if (!c) BG_FAIL(false, "null context");
    if (!c->ready) BG_FAIL(false, "model has no tensors loaded (empty model): cannot evaluate");
    if (session_refuses(c)) return false;
    if (!tokens || n < 1) BG_FAIL(false, "no tokens to evaluate");
    if (n_past < 0 || n_past + n > c->hp.n_positions)
        BG_FAIL(false, "n_past (%d) + n_tokens (%d) exceeds n_positions (%d)", n_past, n, c->hp.n_positions);
    for (int i = 0; i < n; i++)
        if (tokens[i] < 0 || tokens[i] >= c->hp.n_vocab) BG_FAIL(false, "token id %d out of range [0, %d)", tokens[i], c->hp.n_vocab);
    return true;
}

bool alloc_runtime(biogpt_hip_ctx *c) {
    const auto &hp = c->hp;
    const size_t P = (size_t)hp.n_positions, D = (size_t)hp.d_model, F = (size_t)hp.d_ff, V = (size_t)hp.n_vocab;
    const size_t kv = (size_t)hp.n_layer * P * D * 4;
    HIP_TRY(false, hipMalloc(&c->memory_k, kv));
    HIP_TRY(false, hipMalloc(&c->memory_v, kv));
    HIP_TRY(false, hipMemset(c->memory_k, 0, kv));
    HIP_TRY(false, hipMemset(c->memory_v, 0, kv));
    HIP_TRY(false, hipMalloc(&c->x, P * D * 4));
    HIP_TRY(false, hipMalloc(&c->x1, P * D * 4));
    HIP_TRY(false, hipMalloc(&c->q, P * D * 4));
    HIP_TRY(false, hipMalloc(&c->att, P * D * 4));
    HIP_TRY(false, hipMalloc(&c->h, P * F * 4));
    HIP_TRY(false, hipMalloc(&c->logits, V * 4));
    for (int k = 0; k < 3; k++) {
        const size_t n = (k == 1 ? F : D) * P;
        HIP_TRY(false, hipMalloc(&c->aq_q[k], n));
        HIP_TRY(false, hipMalloc(&c->aq_d[k], n / 32 * 4 + 16));
        HIP_TRY(false, hipMalloc(&c->aq_s[k], n / 32 * 4 + 16));
    }
    c->pmax_cap = 4096;
    HIP_TRY(false, hipMalloc(&c->pmax_val, (size_t)c->pmax_cap * 4));
    HIP_TRY(false, hipMalloc(&c->sp_scores, (size_t)hp.n_head * hp.n_positions * 4));
    HIP_TRY(false, hipMalloc(&c->sp_max, (size_t)hp.n_head * bgk::SPLIT_MAX * 4));
    HIP_TRY(false, hipMalloc(&c->sp_pv, (size_t)hp.n_head * bgk::SPLIT_MAX * 64 * 8));
    HIP_TRY(false, hipMalloc(&c->pmax_idx, (size_t)c->pmax_cap * 4));
    HIP_TRY(false, hipMemset(c->pmax_val, 0, (size_t)c->pmax_cap * 4));
    HIP_TRY(false, hipMemset(c->pmax_idx, 0, (size_t)c->pmax_cap * 4));
    c->state_bytes = sizeof(bgk::DevState) + 2 * P * 4;
    HIP_TRY(false, hipMalloc(&c->state, c->state_bytes));
    HIP_TRY(false, hipMemset(c->state, 0, c->state_bytes));
    c->slot_bytes = (sizeof(bgk::DevState) + P * 4 + 63) & ~(size_t)63;
    HIP_TRY(false, hipHostMalloc(reinterpret_cast<void **>(&c->state_host), c->slot_bytes * STATE_SLOTS, hipHostMallocDefault));
    std::memset(c->state_host, 0, c->slot_bytes * STATE_SLOTS);
    HIP_TRY(false, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    HIP_TRY(false, hipEventCreate(&c->ev0));
    HIP_TRY(false, hipEventCreate(&c->ev1));
    HIP_TRY(false, hipHostMalloc(&c->live_host, 4 * sizeof(int32_t)));
    for (auto &e : c->live_ev) HIP_TRY(false, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    return true;
}

bool select_device(int device) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) BG_FAIL(false, "no HIP device available (%s): this engine has no CPU fallback", hipGetErrorString(e));
    if (device < 0 || device >= n) BG_FAIL(false, "HIP device %d out of range (found %d)", device, n);
    HIP_TRY(false, hipSetDevice(device));
    return true;
}

// read every tensor, validate against the expected directory (biogpt.cpp:394-417), repack, upload
bool upload_weights(biogpt_hip_ctx *c, const ModelFile &mf) {
    const auto &hp = c->hp;
    const int32_t wt = ftype_to_type(hp.ftype);
    const int64_t D = hp.d_model;
    const auto expected = expected_tensors(hp);
    // unknown tensors are an error (biogpt.cpp:394-397)
    for (const auto &t : mf.tensors) {
        bool known = false;
        for (const auto &e : expected) if (e.name == t.name) { known = true; break; }
        if (!known) BG_FAIL(false, "unknown tensor '%s' in model file", t.name.c_str());
    }
    if (mf.tensors.size() != expected.size())
        BG_FAIL(false, "ERROR not all tensors loaded from model file - expected %zu, got %zu", expected.size(), mf.tensors.size());

    std::vector<uint8_t> raw, qs, sc, qh;
    auto put_matrix = [&](const std::string &name, const MatSlot &slot, int64_t row0, int64_t rows, int64_t K, bool more_rows_ok = false) -> bool {
        const TensorEntry *t = mf.find(name);
        if (!t) BG_FAIL(false, "ERROR not all tensors loaded from model file - missing '%s'", name.c_str());
        if (t->ne0 != K || (more_rows_ok ? t->ne1 < rows : t->ne1 != rows))
            BG_FAIL(false, "tensor '%s' has wrong shape in model file: got [%lld, %lld], expected [%lld, %lld]", name.c_str(),
                    (long long)t->ne0, (long long)t->ne1, (long long)K, (long long)rows);
        if (t->type != wt) BG_FAIL(false, "tensor '%s' has wrong size in model file: type %s, expected %s", name.c_str(), type_name(t->type), type_name(wt));
        raw.resize(t->nbytes);
        if (!mf.read_payload(*t, raw.data())) return false;
        const size_t qb = unit_bytes_qs(wt, K) * (size_t)rows, sb = unit_bytes_sc(wt, K) * (size_t)rows, hb = unit_bytes_qh(wt, K) * (size_t)rows;
        qs.resize(qb); sc.resize(sb + 4); qh.resize(hb + 4);
        repack_rows(wt, raw.data(), rows, K, qs.data(), sc.data(), qh.data());
        HIP_TRY(false, hipMemcpy(c->arena + slot.qs + unit_bytes_qs(wt, K) * (size_t)row0, qs.data(), qb, hipMemcpyHostToDevice));
        if (sb) HIP_TRY(false, hipMemcpy(c->arena + slot.sc + unit_bytes_sc(wt, K) * (size_t)row0, sc.data(), sb, hipMemcpyHostToDevice));
        if (hb) HIP_TRY(false, hipMemcpy(c->arena + slot.qh + unit_bytes_qh(wt, K) * (size_t)row0, qh.data(), hb, hipMemcpyHostToDevice));
        return true;
    };
    auto put_vec = [&](const std::string &name, size_t off, int64_t elem0, int64_t n) -> bool {
        const TensorEntry *t = mf.find(name);
        if (!t) BG_FAIL(false, "ERROR not all tensors loaded from model file - missing '%s'", name.c_str());
        if (t->ne0 != n || t->ne1 != 1)
            BG_FAIL(false, "tensor '%s' has wrong shape in model file: got [%lld, %lld], expected [%lld, 1]", name.c_str(),
                    (long long)t->ne0, (long long)t->ne1, (long long)n);
        if (t->type != T_F32) BG_FAIL(false, "tensor '%s' has wrong size in model file: type %s, expected f32", name.c_str(), type_name(t->type));
        raw.resize(t->nbytes);
        if (!mf.read_payload(*t, raw.data())) return false;
        HIP_TRY(false, hipMemcpy(c->arena + off + (size_t)elem0 * 4, raw.data(), (size_t)n * 4, hipMemcpyHostToDevice));
        return true;
    };

    const ArenaPlan &pl = c->plan;
    if (!put_matrix("biogpt.embed_tokens.weight", pl.embed_tokens, 0, hp.n_vocab, D)) return false;
    if (!put_matrix("biogpt.embed_positions.weight", pl.embed_pos, 0, c->pos_rows, D, true)) return false;   // first n_positions + 2 rows
    for (int l = 0; l < hp.n_layer; l++) {
        const LayerSlots &L = pl.layers[(size_t)l];
        const std::string p = "biogpt.layers." + std::to_string(l) + ".";
        const char *proj[3] = {"q_proj", "k_proj", "v_proj"};
        for (int k = 0; k < 3; k++) {
            if (!put_matrix(p + "self_attn." + proj[k] + ".weight", L.qkv, (int64_t)k * D, D, D)) return false;
            if (!put_vec(p + "self_attn." + proj[k] + ".bias", L.qkv_b, (int64_t)k * D, D)) return false;
        }
        if (!put_matrix(p + "self_attn.out_proj.weight", L.o, 0, D, D)) return false;
        if (!put_vec(p + "self_attn.out_proj.bias", L.o_b, 0, D)) return false;
        if (!put_vec(p + "self_attn_layer_norm.weight", L.ln0_w, 0, D)) return false;
        if (!put_vec(p + "self_attn_layer_norm.bias", L.ln0_b, 0, D)) return false;
        if (!put_vec(p + "final_layer_norm.weight", L.ln1_w, 0, D)) return false;
        if (!put_vec(p + "final_layer_norm.bias", L.ln1_b, 0, D)) return false;
        if (!put_matrix(p + "fc1.weight", L.fc1, 0, hp.d_ff, D)) return false;
        if (!put_vec(p + "fc1.bias", L.fc1_b, 0, hp.d_ff)) return false;
        if (!put_matrix(p + "fc2.weight", L.fc2, 0, D, hp.d_ff)) return false;
        if (!put_vec(p + "fc2.bias", L.fc2_b, 0, D)) return false;
    }
    if (!put_vec("biogpt.layer_norm.weight", pl.ln_w, 0, D)) return false;
    if (!put_vec("biogpt.layer_norm.bias", pl.ln_b, 0, D)) return false;
    if (!put_matrix("output_projection.weight", pl.lm_head, 0, hp.n_vocab, D)) return false;

    // fp16 tables, built the way ggml_init builds them [SURVEY A.5]
    const std::vector<uint16_t> tg = gelu_table_f16(), te = exp_table_f16();
    HIP_TRY(false, hipMemcpy(c->arena + pl.gelu_tab, tg.data(), 65536 * 2, hipMemcpyHostToDevice));
    HIP_TRY(false, hipMemcpy(c->arena + pl.exp_tab, te.data(), 65536 * 2, hipMemcpyHostToDevice));
    return true;
}

void destroy(biogpt_hip_ctx *c) {
    if (!c) return;
    queue_session_orphan(c);
    (void)hipSetDevice(c->device);
    (void)resident_stop(c);
    if ((c->opt.res_dbg & 32) && c->tstamp && c->res_seq > 8) {      // device-side stamps: token seen by XCD 0's poller [s][0], lm_head workgroup 0's completion word [s][1]
        std::vector<unsigned long long> w(8192);
        if (hipMemcpy(w.data(), c->tstamp, w.size() * 8, hipMemcpyDeviceToHost) == hipSuccess) {
            double proc = 0.0, turn = 0.0; int np = 0, nt = 0;
            const uint32_t hi = c->res_seq < 4000u ? c->res_seq : 4000u;
            for (uint32_t q = 2; q + 1 < hi; q++) {
                const unsigned long long a = w[2 * q], b = w[2 * q + 1], a2 = w[2 * q + 2];
                if (a && b && b > a && b - a < 100000ull) { proc += (double)(b - a) * 0.01; np++; }
                if (b && a2 && a2 > b && a2 - b < 100000ull) { turn += (double)(a2 - b) * 0.01; nt++; }
            }
            fprintf(stderr, "resident launch, device clock: token seen -> completion word %.2f us (%d), completion word -> next token seen %.2f us (%d)\n", np ? proc / np : 0.0, np, nt ? turn / nt : 0.0, nt);
            std::vector<unsigned long long> e(4096 * 4);
            if (hipMemcpy(e.data(), c->tstamp + 32768, e.size() * 8, hipMemcpyDeviceToHost) == hipSuccess) {
                // [q][0] XCD 0's workgroup 0 is ready for the next token, [1] it has the arg-max of token q - 1, [2] token out (and the post of q - 1 checked), [3] lm workgroup 0 published its partials of token q
                double s01 = 0, s12 = 0, sp = 0, sdone = 0, sready = 0; int n = 0;
                for (uint32_t q = 3; q + 1 < hi; q++) {
                    const unsigned long long t0 = e[4 * q], t1 = e[4 * q + 1], t2 = e[4 * q + 2], pp = e[4 * (q - 1) + 3], dn = w[2 * (q - 1) + 1];
                    if (!t0 || !t1 || !t2 || !pp || !dn || t2 < t0 || t2 - t0 > 100000ull) continue;
                    s01 += (double)(long long)(t1 - t0) * 0.01; s12 += (double)(long long)(t2 - t1) * 0.01; sp += (double)(long long)(t1 - pp) * 0.01;
                    sdone += (double)(long long)(pp - dn) * 0.01; sready += (double)(long long)(t0 - dn) * 0.01; n++;
                }
                if (n) fprintf(stderr, "   XCD 0, workgroup 0: ready for the next token %.2f us after lm workgroup 0's completion word (its partials went out %.2f us after that word), arg-max %.2f us after ready = %.2f us after those partials, token out + post checked %.2f us later (%d)\n",
                               sready / n, sdone / n, s01 / n, sp / n, s12 / n, n);
            }
            std::vector<unsigned long long> d(64 * 256);
            if (hipMemcpy(d.data(), c->tstamp + 8192, d.size() * 8, hipMemcpyDeviceToHost) == hipSuccess) {
                double spread = 0.0, last_after_first = 0.0; int ns = 0; int late[8] = {};
                for (int q = 0; q < 64; q++) {
                    unsigned long long lo = ~0ull, hi2 = 0; int arg = -1;
                    for (int k = 0; k < c->res_nw && k < 256; k++) { const unsigned long long t = d[(size_t)q * 256 + k]; if (!t) continue; if (t < lo) lo = t; if (t > hi2) { hi2 = t; arg = k; } }
                    if (hi2 > lo && hi2 - lo < 100000ull) { spread += (double)(hi2 - lo) * 0.01; ns++; if (arg >= 0) late[(arg / 32) & 7]++; last_after_first += (double)(hi2 - d[(size_t)q * 256]) * 0.01; }
                }
                fprintf(stderr, "   completion words of one token: first -> last %.2f us, workgroup 0 -> last %.2f us (%d tokens); XCD group of the last one: %d %d %d %d %d %d\n",
                        ns ? spread / ns : 0.0, ns ? last_after_first / ns : 0.0, ns, late[0], late[1], late[2], late[3], late[4], late[5]);
            }
        }
    }
    if ((c->opt.res_dbg & 8) && c->res_calls > 0)
        fprintf(stderr, "resident evals: %ld calls, %.2f us waiting for the completion words, %.2f us between a return and the next post\n", c->res_calls, c->res_t_wait / c->res_calls * 1e6, c->res_t_call / c->res_calls * 1e6);
    for (auto &pl : c->graph_step) for (auto &row : pl) for (auto &g : row) if (g) (void)hipGraphExecDestroy(g);
    for (auto &pl : c->graph_eval) for (auto &f : pl) for (auto &row : f) for (auto &g : row) if (g) (void)hipGraphExecDestroy(g);
    drop_column_graphs(c);
    for (auto &e : c->live_ev) if (e) (void)hipEventDestroy(e);
    if (c->live_host) (void)hipHostFree(c->live_host);
    if (c->queue_host) (void)hipHostFree(c->queue_host);
    if (c->queue_req_host) (void)hipHostFree(c->queue_req_host);
    if (c->bqueue_host) (void)hipHostFree(c->bqueue_host);
    xpipe_release(c);
    if (c->topk_host) (void)hipHostFree(c->topk_host);
    if (c->mbox_host) (void)hipHostFree(c->mbox_host);
    if (c->mbox_ctr) (void)hipFree(c->mbox_ctr);
    if (c->seq_dev) (void)hipFree(c->seq_dev);
    plain_graph_end(c);
    for (void *p : {(void *)c->bk, (void *)c->bv, (void *)c->seq, (void *)c->seq_gen, (void *)c->cols, (void *)c->sc_tgt, (void *)c->sc_out, (void *)c->emb_buf, (void *)c->sample_ctl, (void *)c->rules_buf, (void *)c->trie_ctl, (void *)c->bbatch_buf, (void *)c->contrast_buf, (void *)c->contrast_h, (void *)c->lookup_buf, (void *)c->genlp_buf, (void *)c->queue_buf, (void *)c->bqueue_buf, (void *)c->queue_req_buf}) if (p) (void)hipFree(p);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->owns_arena && c->arena) (void)hipFree(c->arena);
    for (void *p : {(void *)c->memory_k, (void *)c->memory_v, (void *)c->x, (void *)c->x1, (void *)c->q, (void *)c->att,
                    (void *)c->h, (void *)c->logits, (void *)c->aq_q[0], (void *)c->aq_q[1], (void *)c->aq_q[2], (void *)c->aq_d[0], (void *)c->aq_d[1], (void *)c->aq_d[2], (void *)c->aq_s[0], (void *)c->aq_s[1], (void *)c->aq_s[2], (void *)c->logits_all, (void *)c->pmax_val, (void *)c->pmax_idx, (void *)c->sp_scores, (void *)c->sp_max, (void *)c->sp_pv, (void *)c->tile_img, (void *)c->state})
        if (p) (void)hipFree(p);
    if (c->state_host) (void)hipHostFree(c->state_host);
    if (c->logits_host) (void)hipHostFree(c->logits_host);
    if (c->logits_host_alt) (void)hipHostFree(c->logits_host_alt);
    if (c->res_spec) (void)hipHostFree(c->res_spec);
    for (void *p : {(void *)c->logits_alt, (void *)c->pmax_val_alt, (void *)c->pmax_idx_alt}) if (p) (void)hipFree(p);
    if (c->tstamp) (void)hipFree(c->tstamp);
    if (c->tok_vocab) bg::drop_vocab(c->tok_vocab);
    delete c;
}

biogpt_hip_ctx *load_impl(const char *fname, int device, int verbosity, void *ext_arena, size_t ext_bytes) {
    clear_error();
    if (!fname) BG_FAIL(nullptr, "null file name");
    fprintf(stderr, "%s: loading model from '%s'\n", "biogpt_hip_load", fname);
    ModelFile mf;
    if (!mf.open(fname)) return nullptr;
    if (!select_device(device)) return nullptr;

    std::unique_ptr<biogpt_hip_ctx, void (*)(biogpt_hip_ctx *)> c(new biogpt_hip_ctx(), destroy);
    c->opt.load();
    c->hp = mf.hp;
    c->float_chain = c->opt.float_chain == 1 && float_chain_refusal(c->hp) == nullptr;      // (the environment's default holds where the file can have it)
    c->assoc = (c->opt.assoc == 1 && assoc_refusal(c->hp) == nullptr) ? 1 : 0;      // (likewise BIOGPT_HIP_ASSOC)
    c->assoc_chain = c->opt.assoc_chain == 1 && assoc_refusal(c->hp) == nullptr;      // (and BIOGPT_HIP_ASSOC_CHAIN)
    c->device = device;
    c->n_tensors = (int)mf.tensors.size();
    c->vocab = mf.vocab;
    c->merges = mf.merges;
    c->tok_vocab = bg::make_vocab(mf.vocab, mf.merges);
    const auto &hp = c->hp;
    if (verbosity > 0) {
        fprintf(stderr, "biogpt_hip_load: n_vocab = %d d_ff = %d d_model = %d n_positions = %d n_head = %d n_layer = %d ftype = %d n_merges = %d\n",
                hp.n_vocab, hp.d_ff, hp.d_model, hp.n_positions, hp.n_head, hp.n_layer, hp.ftype, hp.n_merges);
    }
    const int dk = hp.d_model / hp.n_head;
    if (hp.d_model % 32 != 0 || hp.d_ff % 32 != 0) BG_FAIL(nullptr, "d_model (%d) and d_ff (%d) must be multiples of 32", hp.d_model, hp.d_ff);
    if (dk % 4 != 0 || (dk & (dk - 1)) != 0 || dk > 256) BG_FAIL(nullptr, "head size %d unsupported (needs a power of two in [4, 256])", dk);

    // F5: the file's embed_positions must cover n_positions + 2 rows; a longer table is cut to that (rows past it are
    // never indexed), so that the arena layout depends on the 7 header ints only -- a replica that attaches to a
    // broadcast arena computes the same offsets without the file
    c->pos_rows = (int64_t)hp.n_positions + 2;
    if (const TensorEntry *pe = mf.find("biogpt.embed_positions.weight")) {
        if (pe->ne1 < c->pos_rows)
            BG_FAIL(nullptr, "tensor 'biogpt.embed_positions.weight' has wrong shape in model file: got [%lld, %lld], expected [%d, >=%lld]",
                    (long long)pe->ne0, (long long)pe->ne1, hp.d_model, (long long)c->pos_rows);
    }
    c->plan = plan_arena(hp, c->pos_rows);
    if (ext_arena) {
        if (ext_bytes < c->plan.total) BG_FAIL(nullptr, "external arena too small: %zu < %zu bytes", ext_bytes, c->plan.total);
        c->arena = static_cast<uint8_t *>(ext_arena);
        c->owns_arena = false;
    } else {
        HIP_TRY(nullptr, hipMalloc(reinterpret_cast<void **>(&c->arena), c->plan.total));
        c->owns_arena = true;
    }
    c->arena_bytes = c->plan.total;
    if (!alloc_runtime(c.get())) return nullptr;

    if (mf.tensors.empty()) {  // biogpt.cpp:442-443
        fprintf(stderr, "biogpt_hip_load: WARN no tensors loaded from model file - assuming empty model for testing\n");
        c->ready = false;
        return c.release();
    }
    if (!upload_weights(c.get(), mf)) return nullptr;
    HIP_TRY(nullptr, hipDeviceSynchronize());
    c->ready = true;
    xpipe_prepare(c.get());
    (void)fpipe_prepare(c.get());      // (float files: the persistent launch of kernels_fpipe.hip.h, prepared outside any capture)
    if (verbosity > 0)
        fprintf(stderr, "biogpt_hip_load: weight arena = %.2f MB, KV cache = %.2f MB, %d tensors\n", c->plan.total / 1048576.0,
                2.0 * hp.n_layer * hp.n_positions * hp.d_model * 4 / 1048576.0, c->n_tensors);
    return c.release();
}

// The single-token decode step is captured once per context bucket (the attention workgroup size is a
// launch parameter, everything else reads n_past / the token from HBM) and replayed per token.
// context buckets of the captured decode graphs: 64 / 128 / 192 / 256 / 512 / n_positions keys
int graph_bucket(int T) { return T <= 256 ? (T - 1) / 64 : (T <= 512 ? 4 : 5); }
int bucket_tmax(const biogpt_hip_ctx *c, int b) {
    const int t = b < 4 ? 64 * (b + 1) : (b == 4 ? 512 : c->hp.n_positions);
    return std::min(t, c->hp.n_positions);
}

// pl: 1 = the step as the XCD-pipelined launch (the caller holds the device's pipeline slot), 0 = the five-launch layer
bool ensure_graph(biogpt_hip_ctx *c, int advance, int bucket, int pl) {
    if (c->graph_step[pl][advance][bucket]) return true;
    hipGraph_t g = nullptr;
    HIP_TRY(false, hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
    // fused step (contexts up to 256 keys): the sampler of the previous token is the first kernel's prologue and the
    // lm_head kernel advances the position; otherwise embed ... lm_head + the arg-max kernel
    const int tmax = bucket_tmax(c, bucket);
    c->fp_force = pl;
    bool ok = fused_decode_ok(c, tmax) ? enqueue_decode_fused(c, tmax, 2, advance, 0, -1, -1, 1, nullptr, nullptr, pl)
                                       : (enqueue_forward(c, ForwardPass::last_row(1, tmax)) && enqueue_argmax(c, advance));
    c->fp_force = -1;
    hipError_t e = hipStreamEndCapture(c->stream, &g);
    if (!ok) { if (g) (void)hipGraphDestroy(g); return false; }
    HIP_TRY(false, e);
    HIP_TRY(false, hipGraphInstantiate(&c->graph_step[pl][advance][bucket], g, nullptr, nullptr, 0));
    (void)hipGraphDestroy(g);
    return true;
}

}  // namespace

// ======================================== extern "C" ================================================
extern "C" {

const char *biogpt_hip_last_error(void) { return last_error(); }
const char *biogpt_hip_version(void) { return "biogpt-hip gfx950 r1"; }

biogpt_hip_ctx *biogpt_hip_load(const char *fname, int device, int verbosity) { return load_impl(fname, device, verbosity, nullptr, 0); }

biogpt_hip_ctx *biogpt_hip_load_into(const char *fname, int device, int verbosity, void *device_arena, size_t arena_bytes) {
    if (!device_arena) BG_FAIL(nullptr, "null arena");
    return load_impl(fname, device, verbosity, device_arena, arena_bytes);
}

size_t biogpt_hip_arena_bytes_for(const biogpt_hip_hparams *hp) {
    if (!hp || ftype_to_type(hp->ftype) == T_INVALID) return 0;
    return plan_arena(*hp, (int64_t)hp->n_positions + 2).total;
}

biogpt_hip_ctx *biogpt_hip_attach(const biogpt_hip_hparams *hp, int device, void *device_arena, size_t arena_bytes) {
    clear_error();
    if (!hp || !device_arena) BG_FAIL(nullptr, "null argument");
    if (ftype_to_type(hp->ftype) == T_INVALID) BG_FAIL(nullptr, "bad ftype value %d", hp->ftype);
    if (!select_device(device)) return nullptr;
    std::unique_ptr<biogpt_hip_ctx, void (*)(biogpt_hip_ctx *)> c(new biogpt_hip_ctx(), destroy);
    c->opt.load();
    c->hp = *hp;
    c->float_chain = c->opt.float_chain == 1 && float_chain_refusal(c->hp) == nullptr;
    c->assoc = (c->opt.assoc == 1 && assoc_refusal(c->hp) == nullptr) ? 1 : 0;
    c->assoc_chain = c->opt.assoc_chain == 1 && assoc_refusal(c->hp) == nullptr;
    c->device = device;
    c->pos_rows = (int64_t)hp->n_positions + 2;
    c->plan = plan_arena(*hp, c->pos_rows);
    if (arena_bytes < c->plan.total) BG_FAIL(nullptr, "external arena too small: %zu < %zu bytes", arena_bytes, c->plan.total);
    c->arena = static_cast<uint8_t *>(device_arena);
    c->arena_bytes = c->plan.total;
    c->owns_arena = false;
    c->n_tensors = 5 + 16 * hp->n_layer;
    if (!alloc_runtime(c.get())) return nullptr;
    c->ready = true;
    xpipe_prepare(c.get());
    (void)fpipe_prepare(c.get());      // (float files: the persistent launch of kernels_fpipe.hip.h, prepared outside any capture)
    return c.release();
}

void *biogpt_hip_arena_ptr(biogpt_hip_ctx *ctx) { return ctx ? ctx->arena : nullptr; }
size_t biogpt_hip_arena_bytes(const biogpt_hip_ctx *ctx) { return ctx ? ctx->arena_bytes : 0; }

void biogpt_hip_free(biogpt_hip_ctx *ctx) { destroy(ctx); }

int biogpt_hip_share_vocab(biogpt_hip_ctx *dst, const biogpt_hip_ctx *src) {
    if (!dst || !src) BG_FAIL(-1, "null context");
    if (dst == src) return 0;
    if (dst->tok_vocab) { bg::drop_vocab(dst->tok_vocab); dst->tok_vocab = nullptr; }
    dst->vocab = src->vocab;
    dst->merges = src->merges;
    dst->tok_vocab = bg::make_vocab(dst->vocab, dst->merges);
    return 0;
}

int biogpt_hip_refresh_options(biogpt_hip_ctx *ctx) {
    if (!ctx) BG_FAIL(-1, "null context");
    if (!resident_stop(ctx)) return -2;
    ctx->opt.load();
    // captured graphs bake launch shapes chosen from the options
    for (auto &pl : ctx->graph_step) for (auto &row : pl) for (auto &g : row) if (g) { (void)hipGraphExecDestroy(g); g = nullptr; }
    for (auto &pl : ctx->graph_eval) for (auto &f : pl) for (auto &row : f) for (auto &g : row) if (g) { (void)hipGraphExecDestroy(g); g = nullptr; }
    drop_column_graphs(ctx);
    // the pipelined path is rebuilt from the new options (GELU slice, fault hook, long-context buffers) -- which also re-arms a context that had abandoned the
    // path after a disturbed launch: an explicit call, not an automatic cool-down
    HIP_TRY(-2, hipSetDevice(ctx->device));
    HIP_TRY(-2, hipStreamSynchronize(ctx->stream));
    (void)xpipe_check(ctx);
    ctx->xp_tripped = false;
    xpipe_release(ctx);
    ctx->xp_state = 0; ctx->xp_gelu_p = 0; ctx->xp_gelu_n = 0; ctx->xp_gelu_z = 0; ctx->xp_exp_n = 0;
    xpipe_prepare(ctx);
    ctx->fp_state = 0;
    (void)fpipe_prepare(ctx);      // (float files: outside any capture)
    return 0;
}

int biogpt_hip_xpipe_state(const biogpt_hip_ctx *ctx) {
    if (!ctx) return -2;
    if (ctx->xp_state != 1 || !ctx->opt.xpipe || ctx->assoc) return ctx->xp_state == 1 ? 0 : ctx->xp_state;      // (the SIMD association takes no pipelined launch)
    std::lock_guard<std::mutex> lk(g_xp_mu);
    const biogpt_hip_ctx *owner = (ctx->device >= 0 && ctx->device < 64) ? g_xp_owner[ctx->device] : nullptr;
    return (owner == nullptr || owner == ctx) ? 1 : 0;
}

int biogpt_hip_get_hparams(const biogpt_hip_ctx *ctx, biogpt_hip_hparams *out) {
    if (!ctx || !out) BG_FAIL(-1, "null argument");
    *out = ctx->hp;
    return 0;
}
int biogpt_hip_n_tensors(const biogpt_hip_ctx *ctx) { return ctx ? ctx->n_tensors : -1; }
const biogpt_hip_vocab *biogpt_hip_ctx_vocab(const biogpt_hip_ctx *ctx) { return ctx ? ctx->tok_vocab : nullptr; }

int biogpt_hip_vocab_token(const biogpt_hip_ctx *ctx, int32_t id, const char **bytes, int32_t *len) {
    if (!ctx || id < 0 || (size_t)id >= ctx->vocab.size()) return -1;
    if (bytes) *bytes = ctx->vocab[(size_t)id].data();
    if (len) *len = (int32_t)ctx->vocab[(size_t)id].size();
    return 0;
}
int biogpt_hip_merge(const biogpt_hip_ctx *ctx, int32_t rank, const char **bytes, int32_t *len) {
    if (!ctx || rank < 0 || (size_t)rank >= ctx->merges.size()) return -1;
    if (bytes) *bytes = ctx->merges[(size_t)rank].data();
    if (len) *len = (int32_t)ctx->merges[(size_t)rank].size();
    return 0;
}

// how a call waits for its stream: asleep in the runtime, or polling -- the low-latency wait of a caller that is blocked on this token anyway
enum class Wait { Sleep, Poll };
static bool drain_stream(biogpt_hip_ctx *ctx, Wait how) {
    if (how == Wait::Sleep) { HIP_TRY(false, hipStreamSynchronize(ctx->stream)); return true; }
    for (;;) {
        const hipError_t q = hipStreamQuery(ctx->stream);
        if (q == hipSuccess) return true;
        if (q != hipErrorNotReady) HIP_TRY(false, q);
    }
}
// The end of a call that waits for its results: the stream has drained, so every mailbox slot sent has been read, and the pipeline says whether one of
// its launches was disturbed (false: the call's outputs are garbage, last_error says why -- the entry points return -2)
static bool wait_stream(biogpt_hip_ctx *ctx, Wait how = Wait::Sleep) {
    if (!drain_stream(ctx, how)) return false;
    ctx->mbox_synced = ctx->mbox_sent;
    return xpipe_check(ctx);
}

#include "engine_resident.inc"

// the k largest of the values offered so far, descending, equal values: lower index first when they are offered in index order (topk_kernel's order); NaNs are never taken
struct TopkInsert {
    float *vals; int32_t *ids; int k;
    int have = 0;
    float thr = -INFINITY;      // the k-th value once k are held
    void offer(float v, int i) {
        if ((have == k && !(v > thr)) || v != v) return;
        int pos = have < k ? have : k - 1;
        while (pos > 0 && vals[pos - 1] < v) { vals[pos] = vals[pos - 1]; ids[pos] = ids[pos - 1]; pos--; }
        vals[pos] = v; ids[pos] = i;
        if (have < k) have++;
        if (have == k) thr = vals[k - 1];
    }
};
// the k largest values of a row -- ONE pass: a block of 16 values is only looked at when its maximum beats the current k-th value.  Returns how many were
// found (< k only when the row holds NaNs)
static int host_topk(const float *row, int n, int k, float *vals, int32_t *ids) {
    TopkInsert top{vals, ids, k};
    int i = 0;
    for (; i < n && top.have < k; i++) top.offer(row[i], i);
    for (; i + 16 <= n; i += 16) {
        float m = -INFINITY;      // (not row[i]: a NaN there would hide the block -- every comparison with it is false)
        for (int j = 0; j < 16; j++) m = row[i + j] > m ? row[i + j] : m;
        if (m > top.thr)
            for (int j = 0; j < 16; j++) top.offer(row[i + j], i + j);
    }
    for (; i < n; i++) top.offer(row[i], i);
    return top.have;
}

// The same selection when the launch has left the maxima of the row's 64-row blocks behind it (a resident launch): the k-th largest block maximum t0 is a lower
// bound of the k-th largest logit (k blocks hold a value >= t0), so every candidate lies in a block whose maximum is >= t0 -- k blocks, give or take ties, instead of
// n / 64.  They are walked in index order with the same insertion rule, so values, ids and their order are those of host_topk (and of topk_kernel).
static int host_topk_blocks(const float *row, int n, int k, const float *bmax, int nblocks, float *vals, int32_t *ids) {
    if (nblocks < k || nblocks > 1024) return host_topk(row, n, k, vals, ids);
    float top[64];
    int have_b = 0;
    for (int b = 0; b < nblocks; b++) {      // the k largest block maxima, descending (insertion into <= 64 slots: ~700 compares for BioGPT's 663 blocks)
        const float v = bmax[b];
        if (v != v) return host_topk(row, n, k, vals, ids);
        if (have_b == k && !(v > top[k - 1])) continue;
        int pos = have_b < k ? have_b : k - 1;
        while (pos > 0 && top[pos - 1] < v) { top[pos] = top[pos - 1]; pos--; }
        top[pos] = v;
        if (have_b < k) have_b++;
    }
    const float t0 = top[k - 1];
    TopkInsert sel{vals, ids, k};
    for (int b = 0; b < nblocks; b++) {
        if (!(bmax[b] >= t0)) continue;
        const int i0 = b * 64, i1 = std::min(n, i0 + 64);
        for (int i = i0; i < i1; i++) sel.offer(row[i], i);
    }
    return sel.have;
}

// The degenerate rows of biogpt_hip_eval_topk (topk_kernel answered -1: more than TOPK_CAP logits reach its threshold, or fewer than k are comparable): a partial
// sort of the whole row by the tail's order -- larger value first, equal values: lower id first.  NaNs compare with nothing, so they are ordered behind every
// comparable value, among themselves by id (a strict weak order: std::partial_sort needs one) -- a row with fewer than k comparable values ends with NaN pairs.
static void topk_full_row(const float *row, int V, int k, float *vals, int32_t *ids) {
    std::vector<int32_t> order((size_t)V);
    for (int i = 0; i < V; i++) order[(size_t)i] = i;
    std::partial_sort(order.begin(), order.begin() + k, order.end(), [&](int32_t a, int32_t b) {
        const float va = row[(size_t)a], vb = row[(size_t)b];
        const bool na = va != va, nb = vb != vb;
        if (na || nb) return na == nb ? a < b : nb;
        return va > vb || (va == vb && a < b);
    });
    for (int i = 0; i < k; i++) { vals[i] = row[(size_t)order[(size_t)i]]; ids[i] = order[(size_t)i]; }
}

// A replayed five-launch eval carries the sequence number its FIRST node fetched, forwarded by the last layer and the lm_head as they started: any other
// number means that the result is not this call's (profiles/two_contexts_r4.txt, profiles/stale_row_r5.txt).  Repair: the device's replay counter is put
// right and the call is repeated on eager launches (same tokens, same position: the K / V rows are written again with the same values); refetch() then
// enqueues the fetch of the result again.  on_device: the row in question is the device's (biogpt_hip_eval_device), not the one returned to the caller.
extern "C++" template <class Refetch>
int repair_stale_row(biogpt_hip_ctx *ctx, const int32_t *tokens, int n, int n_past, uint32_t got, uint32_t want, bool on_device, Wait how, Refetch refetch) {
    ctx->stale_rows++;
    if (ctx->opt.verbose)
        fprintf(stderr, "biogpt_hip[%p]: the replayed eval at position %d %s the row of call %u instead of %u%s: repeated on eager launches\n", (void *)ctx, n_past,
                on_device ? "left" : "returned", got, want, on_device ? " on the device" : "");
    uint32_t *const fix = reinterpret_cast<uint32_t *>(ctx->mbox_host + 64 * 8);
    *fix = ctx->mbox_sent;
    HIP_TRY(-2, hipMemcpyAsync(ctx->mbox_ctr, fix, 4, hipMemcpyHostToDevice, ctx->stream));
    if (!upload_state(ctx, tokens, n, n_past) || !enqueue_forward(ctx, ForwardPass::last_row(n, n_past + n)) || !refetch()) return -2;
    // (not wait_stream: every mailbox slot was already read when the stale row was found, and the eager launches sent none)
    return (drain_stream(ctx, how) && xpipe_check(ctx)) ? 0 : -2;
}

static int eval_topk_once(biogpt_hip_ctx *ctx, const int32_t *tokens, int32_t n, int32_t n_past, int32_t k, float *vals_out, int32_t *ids_out) {
    if (!vals_out || !ids_out) BG_FAIL(-1, "null output buffer");
    if (!ctx) BG_FAIL(-1, "null context");
    if (k < 1 || k > 64) BG_FAIL(-1, "k must be in [1, 64]");
    k = std::min<int32_t>(k, ctx->hp.n_vocab);
    if (n == 1 && ctx->opt.resident && !ctx->opt.no_graph) {
        // a loop of single-token calls: the resident launch serves it (no launch per call -- the selection kernel could not run beside it anyway), the selection
        // runs over the pinned row on the host; the same k pairs in the same order as topk_kernel's
        XpCallScope xp_scope(ctx);
        clear_error();
        if (!check_eval_args(ctx, tokens, n, n_past)) return -1;
        if (!ctx->res_live) HIP_TRY(-2, hipSetDevice(ctx->device));
        const int r = resident_eval(ctx, tokens[0], n_past);
        if (r < 0) return r;
        if (r == 1) {
            const float *bmax = ctx->row_cur + bgk::xp_blockmax_offset(ctx->hp.n_vocab);
            const int got = ctx->opt.topk_blocks ? host_topk_blocks(ctx->row_cur, ctx->hp.n_vocab, k, bmax, ctx->lm_blocks, vals_out, ids_out)
                                                 : host_topk(ctx->row_cur, ctx->hp.n_vocab, k, vals_out, ids_out);
            if (got == k) return k;
            // NaNs in the row: the device path below has a defined answer for it (the position is evaluated again: same inputs, same K / V row)
        }
    }
    const int rc = biogpt_hip_eval_device(ctx, tokens, n, n_past);
    if (rc) return rc;
    if (!ctx->topk_host) HIP_TRY(-2, hipHostMalloc(reinterpret_cast<void **>(&ctx->topk_host), 64 * 8 + 16, hipHostMallocDefault));
    // the kernel writes its <= 64 pairs straight into pinned host memory: no copy command behind it
    float *out_val = reinterpret_cast<float *>(ctx->topk_host);
    int32_t *out_idx = reinterpret_cast<int32_t *>(ctx->topk_host + 64 * 4);
    auto select = [&]() -> bool {
        HIP_TRY(false, launch_topk(ctx->logits, ctx->hp.n_vocab, k, ctx->pmax_val, ctx->lm_blocks, out_val, out_idx, out_idx + 64, ctx->stream));
        return true;
    };
    if (!select()) return -2;
    uint32_t *const got = (ctx->dev_stamp_expect != 0 && ctx->mbox_host) ? reinterpret_cast<uint32_t *>(ctx->mbox_host + 64 * 8) + 1 : nullptr;
    if (got) HIP_TRY(-2, hipMemcpyAsync(got, ctx->seq_dev + bgk::SEQ_LM_HEAD, 4, hipMemcpyDeviceToHost, ctx->stream));   // the device row's lineage (a replayed five-launch step)
    if (!wait_stream(ctx, Wait::Poll)) return -2;
    if (got) {
        const uint32_t want = ctx->dev_stamp_expect;
        ctx->dev_stamp_expect = 0;
        if (*got != want) {      // the row is another call's: the call again on eager launches, the selection again
            const int fixed = repair_stale_row(ctx, tokens, n, n_past, *got, want, true, Wait::Poll, select);
            if (fixed != 0) return fixed;
        }
    }
    const float *hv = reinterpret_cast<const float *>(ctx->topk_host);
    const int32_t *hi = reinterpret_cast<const int32_t *>(ctx->topk_host + 64 * 4);
    if (hi[64] == k) {
        std::memcpy(vals_out, hv, (size_t)k * 4);
        std::memcpy(ids_out, hi, (size_t)k * 4);
        return k;
    }
    // degenerate row (thousands of logits tie with the k-th workgroup maximum, or NaNs): the full row and a host partial sort
    const size_t V = (size_t)ctx->hp.n_vocab;
    std::vector<float> row(V);
    HIP_TRY(-2, hipMemcpy(row.data(), ctx->logits, V * 4, hipMemcpyDeviceToHost));
    topk_full_row(row.data(), (int)V, k, vals_out, ids_out);
    return k;
}

const float *biogpt_hip_logits_device(const biogpt_hip_ctx *ctx) {
    if (!ctx) return nullptr;
    // a resident launch may hold the last accepted row in its alternate buffer (odd sequence numbers) and may be running one position ahead: it is stopped here -- its
    // results are folded into the ordinary buffers -- so that the pointer names the row of the last evaluated token, as the header says
    if (ctx->res_live || (ctx->res_acc & 1u)) (void)resident_stop(const_cast<biogpt_hip_ctx *>(ctx));
    return ctx->logits;
}

int biogpt_hip_read_logits(biogpt_hip_ctx *ctx, float *out) {
    if (!ctx || !out) BG_FAIL(-1, "null argument");
    clear_error();
    HIP_TRY(-2, hipSetDevice(ctx->device));
    if (!resident_stop(ctx)) return -2;
    HIP_TRY(-2, hipMemcpyAsync(out, ctx->logits, (size_t)ctx->hp.n_vocab * 4, hipMemcpyDeviceToHost, ctx->stream));
    uint32_t *const got = ctx->mbox_host ? reinterpret_cast<uint32_t *>(ctx->mbox_host + 64 * 8) + 1 : nullptr;
    if (ctx->dev_stamp_expect != 0 && got) HIP_TRY(-2, hipMemcpyAsync(got, ctx->seq_dev + bgk::SEQ_LM_HEAD, 4, hipMemcpyDeviceToHost, ctx->stream));
    if (!wait_stream(ctx)) return -2;
    if (ctx->dev_stamp_expect != 0 && got) {
        // the device row of a replayed five-launch eval (biogpt_hip_eval_device): the same lineage check as eval_once's, the same repair
        const uint32_t want = ctx->dev_stamp_expect;
        ctx->dev_stamp_expect = 0;
        const int32_t tok = ctx->dev_stamp_tok;
        if (*got != want)
            return repair_stale_row(ctx, &tok, 1, ctx->dev_stamp_n_past, *got, want, true, Wait::Sleep, [&]() -> bool {
                HIP_TRY(false, hipMemcpyAsync(out, ctx->logits, (size_t)ctx->hp.n_vocab * 4, hipMemcpyDeviceToHost, ctx->stream));
                return true;
            });
    }
    return 0;
}

// {single-token evals replayed as captured five-launch steps, rows found to be another call's and repeated} (kernels.hip.h: SEQ_*)
int biogpt_hip_lineage_stats(biogpt_hip_ctx *ctx, int64_t *out2) {
    if (!ctx || !out2) BG_FAIL(-1, "null argument");
    out2[0] = ctx->graph_evals; out2[1] = ctx->stale_rows;
    return 0;
}

int biogpt_hip_synchronize(biogpt_hip_ctx *ctx) {
    if (!ctx) BG_FAIL(-1, "null context");
    if (!resident_stop(ctx)) return -2;
    HIP_TRY(-2, hipStreamSynchronize(ctx->stream));
    if (!xpipe_check(ctx)) {      // reported to the caller here: there is no call to repeat, and a later, unrelated failure must not trigger a spurious retry
        ctx->xp_tripped = false;
        const int from = ctx->unsynced_from;
        ctx->unsynced_from = -1;
        if (from >= 0) BG_FAIL(-2, "the pipelined decode step failed; the evals from position %d on must be repeated (the context now uses the five-launch layer)", from);
        return -2;
    }
    return 0;
}

// logits_out == nullptr: the row stays in the context's pinned host buffer (biogpt_hip_eval_inplace)
static int eval_once(biogpt_hip_ctx *ctx, const int32_t *tokens, int32_t n, int32_t n_past, float *logits_out) {
    XpCallScope xp_scope(ctx);
    if (n == 1) {      // one token: a launch that stays on the device between the calls of the caller's loop
        clear_error();
        if (!check_eval_args(ctx, tokens, n, n_past)) return -1;
        if (!ctx->res_live) HIP_TRY(-2, hipSetDevice(ctx->device));      // a live resident launch needs no HIP call at all
        const int r = resident_eval(ctx, tokens[0], n_past);
        if (r < 0) return r;
        if (r == 1) { if (logits_out) std::memcpy(logits_out, ctx->row_cur, (size_t)ctx->hp.n_vocab * 4); return 0; }
    }
    bool in_graph = false;      // the replayed graph already wrote the pinned row
    const int rc = eval_device_impl(ctx, tokens, n, n_past, 1, &in_graph);
    if (rc) return rc;
    const size_t bytes = (size_t)ctx->hp.n_vocab * 4;
    if (!in_graph) {   // device -> pinned staging -> caller's (pageable) buffer: one DMA instead of the runtime's chunked staging
        if (!ctx->logits_host) HIP_TRY(-2, hipHostMalloc(reinterpret_cast<void **>(&ctx->logits_host), host_row_bytes(ctx), hipHostMallocDefault));
        HIP_TRY(-2, hipMemcpyAsync(ctx->logits_host, ctx->logits, bytes, hipMemcpyDeviceToHost, ctx->stream));
    }
    if (!wait_stream(ctx, Wait::Poll)) return -2;
    if (in_graph && ctx->stamp_expect != 0) {      // the pinned row of a replayed five-launch graph: its lineage lies behind it
        const uint32_t got = reinterpret_cast<const uint32_t *>(ctx->logits_host)[host_stamp_index(ctx)];
        const uint32_t want = ctx->stamp_expect;
        ctx->stamp_expect = 0;
        if (got != want) {
            const int fixed = repair_stale_row(ctx, tokens, n, n_past, got, want, false, Wait::Poll, [&]() -> bool {
                HIP_TRY(false, hipMemcpyAsync(ctx->logits_host, ctx->logits, bytes, hipMemcpyDeviceToHost, ctx->stream));
                return true;
            });
            if (fixed != 0) return fixed;
        }
    }
    ctx->row_cur = ctx->logits_host;
    if (logits_out) std::memcpy(logits_out, ctx->logits_host, bytes);
    return 0;
}

// logits_all holds at least `rows` rows; a new buffer drops the captured column steps (they hold the old pointer)
static bool ensure_logits_rows(biogpt_hip_ctx *c, size_t rows) {
    if (rows <= c->logits_all_rows) return true;
    if (c->logits_all) (void)hipFree(c->logits_all);
    c->logits_all = nullptr; c->logits_all_rows = 0;
    HIP_TRY(false, hipMalloc(&c->logits_all, rows * c->hp.n_vocab * 4));
    c->logits_all_rows = rows;
    drop_column_graphs(c);
    return true;
}

int biogpt_hip_eval_all(biogpt_hip_ctx *ctx, const int32_t *tokens, int32_t n, int32_t n_past, float *logits_out) {
    clear_error();
    if (!logits_out) BG_FAIL(-1, "null logits buffer");
    if (!check_eval_args(ctx, tokens, n, n_past)) return -1;
    HIP_TRY(-2, hipSetDevice(ctx->device));
    if (!resident_stop(ctx)) return -2; disarm_lineage(ctx);
    if (!ensure_logits_rows(ctx, (size_t)n)) return -2;
    if (!upload_state(ctx, tokens, n, n_past)) return -2;
    if (!enqueue_forward(ctx, ForwardPass::every_row(n, n_past + n))) return -2;
    HIP_TRY(-2, hipMemcpyAsync(logits_out, ctx->logits_all, (size_t)n * ctx->hp.n_vocab * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(-2, hipStreamSynchronize(ctx->stream));
    return 0;
}

// Prompt ingestion = consecutive evals of n_batch tokens (main.cpp:129-137), each attending to everything before
// it and to its own chunk (no mask inside an eval, F1).  Nothing else couples the chunks, so up to
// BIOGPT_HIP_PROMPT_COLS columns (several chunks) go through the layers in ONE pass -- every weight byte is
// streamed once for all of them (default 512 columns) -- with the attention of column i limited to the keys its own chunk would
// have seen (DevState::chunk).  Per-column arithmetic is unchanged: logits and KV rows are bit-identical to
// the chunk-by-chunk evaluation.  Leaves the last token's logits in ctx->logits.
bool enqueue_prompt(biogpt_hip_ctx *c, const int32_t *tokens, int n, int n_past, int n_batch, int *last_cols = nullptr) {
    const int max_cols = std::max(1, c->opt.prompt_cols);   // measured (Q4_0, -b 8, 512-token prompt): 16 -> 17.9k, 64 -> 36k, 128 -> 66k, 256 -> 87k, 512 -> 97k prompt tok/s
    const int group = n_batch >= max_cols ? n_batch : (max_cols / n_batch) * n_batch;   // whole chunks per pass
    if (std::min(group, n) >= MFMA_MIN_PASS_COLS && is_quantized(ftype_to_type(c->hp.ftype)) && !ensure_tile_images(c)) return false;
    for (int at = 0; at < n;) {
        const int m = std::min(group, n - at);
        if (!upload_state(c, tokens + at, m, n_past + at, m > n_batch ? n_batch : 0)) return false;
        if (!enqueue_forward(c, ForwardPass::last_row(m, n_past + at + m))) return false;
        if (last_cols) *last_cols = m;   // the device state now describes this pass (its n_past, its m tokens)
        at += m;
    }
    return true;
}

static int eval_prompt_once(biogpt_hip_ctx *ctx, const int32_t *tokens, int32_t n_tokens, int32_t n_past, int32_t n_batch, float *logits_out) {
    XpCallScope xp_scope(ctx);
    clear_error();
    if (n_batch < 1) BG_FAIL(-1, "n_batch must be >= 1");
    if (!check_eval_args(ctx, tokens, n_tokens, n_past)) return -1;
    HIP_TRY(-2, hipSetDevice(ctx->device));
    if (!resident_stop(ctx)) return -2; disarm_lineage(ctx);
    if (!enqueue_prompt(ctx, tokens, n_tokens, n_past, n_batch)) return -2;
    if (logits_out) {
        HIP_TRY(-2, hipMemcpyAsync(logits_out, ctx->logits, (size_t)ctx->hp.n_vocab * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (!wait_stream(ctx)) return -2;      // a prompt of up to 8 tokens is a pipelined launch (kernels_xcols.hip.h; one token: kernels_xpipe.hip.h)
    }
    return 0;
}

static int generate_greedy_once(biogpt_hip_ctx *ctx, const int32_t *prompt, int32_t n_prompt, int32_t n_batch,
                                int32_t n_predict, int32_t *out_ids, double *seconds_out) {
    XpCallScope xp_scope(ctx);
    clear_error();
    if (!ctx || !prompt || !out_ids) BG_FAIL(-1, "null argument");
    if (n_batch < 1) BG_FAIL(-1, "n_batch must be >= 1");
    if (n_prompt < 1) BG_FAIL(-1, "empty prompt");
    if (!check_eval_args(ctx, prompt, n_prompt, 0)) return -1;
    n_predict = std::min(n_predict, ctx->hp.n_positions - n_prompt);  // main.cpp:82
    if (n_predict <= 0) return 0;
    HIP_TRY(-2, hipSetDevice(ctx->device));
    if (!resident_stop(ctx)) return -2; disarm_lineage(ctx);
    bool use_graph = ctx->opt.no_graph == 0;
    if ((ctx->opt.dbg & 128) && !ctx->tstamp) {      // profiling builds: stage stamps of the pipelined launches (tools/tail_timeline.py)
        HIP_TRY(-2, hipMalloc(&ctx->tstamp, (size_t)4 << 20));
        HIP_TRY(-2, hipMemset(ctx->tstamp, 0, (size_t)4 << 20));
    }
    // the device's pipeline slot, if it is free, is this call's until its final synchronisation
    // Decided ONCE per bucket, here: xpipe_usable() can take the slot over from a holder that has gone idle in the meantime, so asking again at replay
    // time could name a graph that was never captured.  The graph replayed for a bucket is the one instantiated for it.
    int pl_bucket[6] = {0, 0, 0, 0, 0, 0};
    auto pl_of = [&](int b) { return pl_bucket[b]; };
    if (use_graph)  // instantiate every bucket this run will touch before the clock starts
        for (int b = graph_bucket(n_prompt + 1); b <= graph_bucket(n_prompt + n_predict - 1 > 0 ? n_prompt + n_predict - 1 : 1); b++) {
            pl_bucket[b] = pipeline_pl(ctx, bucket_tmax(ctx, b));
            if (!ensure_graph(ctx, 1, b, pl_bucket[b])) return -2;
        }
    if (use_graph) {   // captured five-launch steps are not replayed beside ANOTHER context's persistent launch (plain_graph_begin): such a run takes eager steps
        bool any_plain = false;
        for (int b = graph_bucket(n_prompt + 1); b <= graph_bucket(n_prompt + n_predict - 1 > 0 ? n_prompt + n_predict - 1 : 1); b++) any_plain = any_plain || pl_bucket[b] == 0;
        if (any_plain && !plain_graph_begin(ctx)) use_graph = false;
    }
    HIP_TRY(-2, hipStreamSynchronize(ctx->stream));

    const auto t0 = std::chrono::steady_clock::now();
    // prompt ingestion in chunks of n_batch (main.cpp:129-137), several chunks per pass; then the first sampled token.
    // Fused steps (graph replay, contexts up to 256 keys) sample the PREVIOUS token in their first kernel, so between
    // them no sampler kernel runs: `pending` = the last lm_head's arg-max has not been recorded yet.
    auto fused = [&](int T) { return use_graph && fused_decode_ok(ctx, bucket_tmax(ctx, graph_bucket(T))); };
    int last_cols = 0;
    if (!enqueue_prompt(ctx, prompt, n_prompt, 0, n_batch, &last_cols)) return -2;
    bool pending = n_predict > 1 && fused(n_prompt + 1);
    if (pending) {
        hipLaunchKernelGGL(bgk::advance_state_kernel, dim3(1), dim3(1), 0, ctx->stream, ctx->state, last_cols);
        HIP_TRY(-2, hipGetLastError());
    } else if (!enqueue_argmax(ctx, last_cols)) {
        return -2;
    }
    ctx->gen_launches = 0;
    for (int k = 1; k < n_predict; k++) {  // one eval + one sample per further token
        const int T = n_prompt + k;  // keys visible to this token: n_past + 1
        if (pending && !fused(T)) {  // leaving the fused range: record the token the unfused step will embed
            if (!enqueue_argmax(ctx, 0)) return -2;
            pending = false;
        }
        const int multi = pending ? std::min(xpipe_multi_tokens(ctx, T), n_predict - k) : 0;
        if (multi > 1) {   // the generation loop itself runs on the device: `multi` tokens in ONE launch (kernels_xpipe.hip.h)
            if (!enqueue_decode_fused(ctx, bucket_tmax(ctx, graph_bucket(T)), 2, 1, 0, -1, -1, multi)) return -2;
            if (ctx->gen_launches < 16) ctx->gen_launch_tokens[ctx->gen_launches++] = multi;
            k += multi - 1;
        } else if (use_graph) {
            HIP_TRY(-2, hipGraphLaunch(ctx->graph_step[pl_of(graph_bucket(T))][1][graph_bucket(T)], ctx->stream));
        } else {
            if (!enqueue_forward(ctx, ForwardPass::last_row(1, T)) || !enqueue_argmax(ctx, 1)) return -2;
        }
    }
    if (pending && !enqueue_argmax(ctx, 0)) return -2;   // the last token's sampler
    HIP_TRY(-2, hipStreamSynchronize(ctx->stream));
    if (!xpipe_check(ctx)) return -2;
    const auto t1 = std::chrono::steady_clock::now();
    if (seconds_out) *seconds_out = std::chrono::duration<double>(t1 - t0).count();
    HIP_TRY(-2, hipMemcpy(out_ids, reinterpret_cast<uint8_t *>(ctx->state) + sizeof(bgk::DevState) + (size_t)ctx->hp.n_positions * 4,
                          (size_t)n_predict * 4, hipMemcpyDeviceToHost));
    return n_predict;
}

// The XCD-pipelined decode step assumes that its 256 workgroups are spread 32 per XCD and become resident together; kernels of
// other streams or processes dispatched in between can break that (the launch then drains with an error word and garbage
// outputs).  These calls are idempotent for given arguments, so they are simply repeated once on the five-launch layer, which the
// context keeps from then on.
// n_past: the position the failed call evaluates.  Earlier asynchronous single-token evals (biogpt_hip_eval_device) that were still in flight went through the same
// tripped pipeline: their K / V rows are garbage and repeating only THIS call would return wrong logits with rc 0 -- then the caller is told where to resume instead.
static bool xpipe_retry(biogpt_hip_ctx *ctx, int n_past) {
    if (!ctx || !ctx->xp_tripped) return false;
    ctx->xp_tripped = false;
    const int from = ctx->unsynced_from;
    ctx->unsynced_from = -1;
    fprintf(stderr, "biogpt_hip: %s\n", last_error());
    if (from >= 0 && from < n_past) {
        bg::set_error("biogpt_hip_eval", "the pipelined decode step failed while evals from position %d on were still in flight: their K / V rows are invalid -- re-evaluate from n_past = %d (the context now uses the five-launch layer)", from, from);
        return false;
    }
    return true;
}
// once(): the call; a negative result after a tripped pipeline is repeated once
extern "C++" template <class Once>
int with_xpipe_retry(biogpt_hip_ctx *ctx, int n_past, Once once) {
    int rc = once();
    if (rc < 0 && xpipe_retry(ctx, n_past)) rc = once();
    return rc;
}
int biogpt_hip_eval_inplace(biogpt_hip_ctx *ctx, const int32_t *tokens, int32_t n, int32_t n_past, const float **row_out) {
    if (!row_out) BG_FAIL(-1, "null row pointer");
    const int rc = with_xpipe_retry(ctx, n_past, [&] { return eval_once(ctx, tokens, n, n_past, nullptr); });
    *row_out = rc == 0 ? ctx->row_cur : nullptr;
    return rc;
}
int64_t biogpt_hip_chunk_launches(const biogpt_hip_ctx *ctx) { return ctx ? ctx->xc_launches : -1; }
int64_t biogpt_hip_mfma_launches(const biogpt_hip_ctx *ctx) { return ctx ? ctx->mfma_launches : -1; }
int64_t biogpt_hip_wide_launches(const biogpt_hip_ctx *ctx) { return ctx ? ctx->wide_launches : -1; }
int64_t biogpt_hip_float_launches(const biogpt_hip_ctx *ctx) { return ctx ? ctx->float_launches : -1; }
int biogpt_hip_chain_kind(const biogpt_hip_ctx *ctx) {
    if (!ctx) BG_FAIL(-1, "null context");
    return chain_kind(ctx);
}
// The float chain's switch.  Off (the default), a float file is what it was: no call over column states.  The captured column steps bake the route: dropped.
int biogpt_hip_float_chain(biogpt_hip_ctx *ctx, int on) {
    clear_error();
    if (!ctx) BG_FAIL(-1, "null context");
    if (on != 0 && on != 1) BG_FAIL(-1, "on must be 0 or 1 (got %d)", on);
    if (session_refuses(ctx)) return -1;
    {
        std::lock_guard<std::mutex> lk(g_xp_mu);
        if (ctx->xp_in_call) BG_FAIL(-1, "the float fast chain cannot be switched while a call of this context is running");
    }
    if (on) {
        if (const char *why = float_chain_refusal(ctx->hp))
            BG_FAIL(-1, "the float fast chain cannot be switched on for this file: %s (it needs F32 / F16 weights, head size 64, d_model a multiple of 64, d_ff of 32; got ftype %d, d_model %d, d_ff %d, %d heads)", why, ctx->hp.ftype, ctx->hp.d_model, ctx->hp.d_ff, ctx->hp.n_head);
    }
    if (ctx->float_chain == (on == 1)) return 0;
    if (ctx->ready) {
        HIP_TRY(-2, hipSetDevice(ctx->device));
        HIP_TRY(-2, hipStreamSynchronize(ctx->stream));
    }
    drop_column_graphs(ctx);
    ctx->float_chain = on == 1;
    return 0;
}
// The association's switch.  Mode 0, the scalar association, is the context as it ever was; mode 1 is the SIMD association (kernels_assoc.hip.h): the five
// launches per layer on its kernels and nothing else.  Every captured graph bakes a route -- the column steps, the single-token steps and evals: dropped.
int biogpt_hip_assoc(biogpt_hip_ctx *ctx, int mode) {
    clear_error();
    if (!ctx) BG_FAIL(-1, "null context");
    if (mode != 0 && mode != 1) BG_FAIL(-1, "mode must be 0 (the scalar association) or 1 (the SIMD association) (got %d)", mode);
    if (session_refuses(ctx)) return -1;
    {
        std::lock_guard<std::mutex> lk(g_xp_mu);
        if (ctx->xp_in_call) BG_FAIL(-1, "the association cannot be switched while a call of this context is running");
    }
    if (mode == 1) {
        if (const char *why = assoc_refusal(ctx->hp))
            BG_FAIL(-1, "the SIMD association cannot be switched on for this file: it is %s (it needs Q4_0 / Q4_1 / Q5_0 / Q5_1 / Q8_0 weights, head size 64, d_model and d_ff multiples of 32; got ftype %d, d_model %d, d_ff %d, %d heads)", why, ctx->hp.ftype, ctx->hp.d_model, ctx->hp.d_ff, ctx->hp.n_head);
    }
    if (ctx->assoc == mode) return 0;
    if (ctx->ready) {
        HIP_TRY(-2, hipSetDevice(ctx->device));
        if (!resident_stop(ctx)) return -2;      // (a resident launch is a scalar-association launch; it synchronises the stream)
        HIP_TRY(-2, hipStreamSynchronize(ctx->stream));
        disarm_lineage(ctx);
    }
    for (auto &pl : ctx->graph_step) for (auto &row : pl) for (auto &g : row) if (g) { (void)hipGraphExecDestroy(g); g = nullptr; }
    for (auto &pl : ctx->graph_eval) for (auto &f : pl) for (auto &row : f) for (auto &g : row) if (g) { (void)hipGraphExecDestroy(g); g = nullptr; }
    drop_column_graphs(ctx);
    ctx->assoc = mode;
    return 0;
}
int biogpt_hip_get_assoc(const biogpt_hip_ctx *ctx) {
    if (!ctx) BG_FAIL(-1, "null context");
    return ctx->assoc;
}
// The SIMD chain's switch: a property of the context that takes effect only while it is in the SIMD association.  Off (the default), a context in mode 1 is what
// it was: no call over column states.  In mode 0 the switch is inert -- no launch, no check and no message looks at it.  The captured column steps bake the
// route: dropped.
int biogpt_hip_assoc_chain(biogpt_hip_ctx *ctx, int on) {
    clear_error();
    if (!ctx) BG_FAIL(-1, "null context");
    if (on != 0 && on != 1) BG_FAIL(-1, "on must be 0 or 1 (got %d)", on);
    if (session_refuses(ctx)) return -1;
    {
        std::lock_guard<std::mutex> lk(g_xp_mu);
        if (ctx->xp_in_call) BG_FAIL(-1, "the SIMD chain cannot be switched while a call of this context is running");
    }
    if (on) {
        if (const char *why = assoc_refusal(ctx->hp))
            BG_FAIL(-1, "the SIMD chain cannot be switched on for this file: it is %s (like the SIMD association it needs Q4_0 / Q4_1 / Q5_0 / Q5_1 / Q8_0 weights, head size 64, d_model and d_ff multiples of 32; got ftype %d, d_model %d, d_ff %d, %d heads)", why, ctx->hp.ftype, ctx->hp.d_model, ctx->hp.d_ff, ctx->hp.n_head);
    }
    if (ctx->assoc_chain == (on == 1)) return 0;
    if (ctx->ready) {
        HIP_TRY(-2, hipSetDevice(ctx->device));
        HIP_TRY(-2, hipStreamSynchronize(ctx->stream));
    }
    drop_column_graphs(ctx);
    ctx->assoc_chain = on == 1;
    return 0;
}
int biogpt_hip_get_assoc_chain(const biogpt_hip_ctx *ctx) {
    if (!ctx) BG_FAIL(-1, "null context");
    return ctx->assoc_chain ? 1 : 0;
}
int64_t biogpt_hip_simd_chain_launches(const biogpt_hip_ctx *ctx) { return ctx ? ctx->simd_chain_launches : -1; }
int biogpt_hip_fpipe_stamps(biogpt_hip_ctx *ctx, uint64_t *out, int n) {
    if (!ctx || !out || n < 0 || ctx->fp_state != 1 || !ctx->opt.fpipe_stamps) return -1;
    if (hipSetDevice(ctx->device) != hipSuccess) return -1;
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) return -1;
    const int m = n < 3 * 1024 ? n : 3 * 1024;
    return hipMemcpy(out, ctx->fp_ctl + 16, (size_t)m * 8, hipMemcpyDeviceToHost) == hipSuccess ? m : -1;
}
int64_t biogpt_hip_fpipe_launches(const biogpt_hip_ctx *ctx) { return ctx ? (ctx->fp_state == 1 ? ctx->fp_launches : -1) : -2; }
int biogpt_hip_generate_launches(const biogpt_hip_ctx *ctx, int32_t *tokens_out, int cap) {
    if (!ctx) return -1;
    for (int i = 0; i < ctx->gen_launches && i < cap && tokens_out; i++) tokens_out[i] = ctx->gen_launch_tokens[i];
    return ctx->gen_launches;
}
int biogpt_hip_resident_stats(const biogpt_hip_ctx *ctx, int64_t *out4) {
    if (!ctx || !out4) return -1;
    out4[0] = ctx->spec_hits; out4[1] = ctx->spec_misses; out4[2] = ctx->spec_streak; out4[3] = ctx->spec_need;
    return 0;
}
int biogpt_hip_eval_prompt(biogpt_hip_ctx *ctx, const int32_t *tokens, int32_t n_tokens, int32_t n_past, int32_t n_batch, float *logits_out) {
    return with_xpipe_retry(ctx, n_past, [&] { return eval_prompt_once(ctx, tokens, n_tokens, n_past, n_batch, logits_out); });
}
int biogpt_hip_eval(biogpt_hip_ctx *ctx, const int32_t *tokens, int32_t n, int32_t n_past, float *logits_out) {
    if (!logits_out) BG_FAIL(-1, "null logits buffer");
    return with_xpipe_retry(ctx, n_past, [&] { return eval_once(ctx, tokens, n, n_past, logits_out); });
}
int biogpt_hip_eval_topk(biogpt_hip_ctx *ctx, const int32_t *tokens, int32_t n, int32_t n_past, int32_t k, float *vals_out, int32_t *ids_out) {
    return with_xpipe_retry(ctx, n_past, [&] { return eval_topk_once(ctx, tokens, n, n_past, k, vals_out, ids_out); });
}
int biogpt_hip_generate_greedy(biogpt_hip_ctx *ctx, const int32_t *prompt, int32_t n_prompt, int32_t n_batch, int32_t n_predict, int32_t *out_ids,
                               double *seconds_out) {
    return with_xpipe_retry(ctx, 0, [&] { return generate_greedy_once(ctx, prompt, n_prompt, n_batch, n_predict, out_ids, seconds_out); });
}

static int hp_cols(const biogpt_hip_ctx *c) { return c->hp.n_positions; }   // scratch is sized [n_positions] columns

// per-sequence F32 K / V caches + state of n_seqs independent sequences (192 MiB per BioGPT-base sequence); new buffers drop the captured batched-decode graphs
static bool ensure_seq_caches(biogpt_hip_ctx *ctx, int n_seqs) {
    if (n_seqs <= ctx->batch_cap) return true;
    const size_t seq_stride = (size_t)ctx->hp.n_layer * ctx->hp.n_positions * ctx->hp.d_model;
    for (void *p : {(void *)ctx->bk, (void *)ctx->bv, (void *)ctx->seq, (void *)ctx->seq_gen}) if (p) (void)hipFree(p);
    ctx->bk = ctx->bv = nullptr; ctx->seq = nullptr; ctx->seq_gen = nullptr; ctx->batch_cap = 0;
    // every column owns a full F32 K / V cache (BioGPT-base: 201 MB; 48 layers at d_model 1600: 629 MB): a request that does not fit says how much it was
    if (hipMalloc(&ctx->bk, seq_stride * 4 * n_seqs) != hipSuccess || hipMalloc(&ctx->bv, seq_stride * 4 * n_seqs) != hipSuccess) {
        (void)hipGetLastError();
        if (ctx->bk) (void)hipFree(ctx->bk);
        ctx->bk = ctx->bv = nullptr;
        BG_FAIL(false, "no device memory for the K / V caches of %d columns: %.1f GB (%.0f MB per column = 2 x n_layer %d x n_positions %d x d_model %d x 4 bytes)", n_seqs,
                (double)seq_stride * 8.0 * n_seqs / 1e9, (double)seq_stride * 8.0 / 1e6, ctx->hp.n_layer, ctx->hp.n_positions, ctx->hp.d_model);
    }
    HIP_TRY(false, hipMalloc(&ctx->seq, sizeof(bgk::SeqState) * n_seqs));
    HIP_TRY(false, hipMalloc(&ctx->seq_gen, (size_t)n_seqs * ctx->hp.n_positions * 4));
    ctx->batch_cap = n_seqs;
    drop_column_graphs(ctx);
    return true;
}

// One pass of packed columns (pack_column_passes, pack_continuation_passes): the column states go up to ctx->cols (grown to the pass), then
// pass(n_cols, t_max, flat0) enqueues the pass; afterwards the host vector is empty and flat0 / pass_tmax stand at the next pass.
// tail (or null): words that go up behind the column states in the same copy, zero-padded to whole SeqStates -- at ctx->cols + n_cols while the pass runs
// (the run table of a pass, 16 bytes per run: pack_continuation_passes).
static bool flush_columns(biogpt_hip_ctx *ctx, std::vector<bgk::SeqState> &cols, int &pass_tmax, size_t &flat0,
                          const std::function<bool(int, int, size_t)> &pass, const std::vector<int32_t> *tail = nullptr) {
    if (cols.empty()) return true;
    const size_t n = cols.size();
    if (tail && !tail->empty()) {
        static_assert(sizeof(bgk::SeqState) == 32, "a column state holds two table rows");
        cols.resize(n + (tail->size() * 4 + sizeof(bgk::SeqState) - 1) / sizeof(bgk::SeqState));      // (new states are all zero)
        std::memcpy(static_cast<void *>(cols.data() + n), tail->data(), tail->size() * 4);
    }
    if (cols.size() > ctx->cols_cap) {
        if (ctx->cols) (void)hipFree(ctx->cols);
        ctx->cols = nullptr; ctx->cols_cap = 0;
        if (!tail) {
            HIP_TRY(false, hipMalloc(&ctx->cols, sizeof(bgk::SeqState) * cols.size()));
        } else if (hipMalloc(&ctx->cols, sizeof(bgk::SeqState) * cols.size()) != hipSuccess) {
            (void)hipGetLastError();
            ctx->cols = nullptr;
            BG_FAIL(false, "out of device memory: the %zu-byte column states of a pass could not be allocated", sizeof(bgk::SeqState) * cols.size());
        }
        ctx->cols_cap = cols.size();
    }
    HIP_TRY(false, hipMemcpyAsync(ctx->cols, cols.data(), sizeof(bgk::SeqState) * cols.size(), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(false, hipStreamSynchronize(ctx->stream));   // the host vector is reused for the next pass
    if (!pass((int)n, pass_tmax, flat0)) return false;
    flat0 += n;
    cols.clear();
    pass_tmax = 0;
    return true;
}

// Prompt columns of several sequences in common passes (generate_greedy_batch's prompt ingestion, score_batch): every token is a
// column that knows its sequence, its position and the end of its own n_batch-chunk (SeqState::seq_id / n_past / t_vis); whole
// chunks are packed into passes of up to BIOGPT_HIP_PROMPT_COLS columns (at most n_positions: the activation scratch).  The columns
// follow the flat order of `seqs`.  Per pass the column states go to ctx->cols, then pass(n_cols, t_max, flat0) enqueues the pass
// (flat0 = flat index of its first token).  Sequence s fills the K / V cache slot slot0 + s * slot_stride.  shared.n > 0: every sequence stands behind
// shared.n rows that lie in slot shared.slot (a multiple of n_batch, so the chunks are those of the whole sequence): its first token has position shared.n
// and its columns read those rows in place (SeqState::pad[0] / pad[1]; the pass is ForwardPass::packed_continuations).
// slots (or null): sequence s fills slot slots[s] instead (run_queue_call refills the units that have finished).
struct SharedRows { int n = 0, slot = 0; };
static bool pack_column_passes(biogpt_hip_ctx *ctx, const int32_t *seqs, const int32_t *lens, int n_seqs, int n_batch,
                               const std::function<bool(int, int, size_t)> &pass, int slot_stride = 1, int slot0 = 0, SharedRows shared = SharedRows{},
                               const int32_t *slots = nullptr) {
    const int max_cols = std::min(std::max(std::max(1, ctx->opt.prompt_cols), n_batch), hp_cols(ctx));   // the activation scratch holds n_positions columns
    std::vector<bgk::SeqState> cols;
    int pass_tmax = 0;
    size_t flat0 = 0;
    auto flush = [&]() -> bool { return flush_columns(ctx, cols, pass_tmax, flat0, pass); };
    size_t off = 0;
    for (int s = 0; s < n_seqs; s++) {
        const int len = lens[s];
        for (int at = 0; at < len; at += n_batch) {
            const int m = std::min(n_batch, len - at);
            if (!cols.empty() && (int)cols.size() + m > max_cols && !flush()) return false;
            for (int i = 0; i < m; i++) {
                bgk::SeqState cst{};
                cst.n_past = shared.n + at + i; cst.token = seqs[off + (size_t)(at + i)]; cst.seq_id = slots ? slots[s] : slot0 + s * slot_stride; cst.t_vis = shared.n + at + m;
                cst.pad[0] = shared.n; cst.pad[1] = shared.slot;
                cols.push_back(cst);
            }
            pass_tmax = std::max(pass_tmax, shared.n + at + m);
        }
        off += (size_t)len;
    }
    return flush();
}

// ---- byte buffers in parts --------------------------------------------------------------------------------------------------------------
// The parts of one buffer, one after another, each at a multiple of 16 bytes.  A layout function lays its parts out at a base pointer -- the device buffer, or a
// host image of its head -- and with no base gives the size alone, so a size cannot disagree with its offsets.
extern "C++" {
struct ByteLayout {
    size_t at = 0;
    size_t part(size_t bytes) { const size_t o = at; at = (at + bytes + 15) & ~(size_t)15; return o; }
    size_t bytes() const { return at; }
    template <class T> T *take(uint8_t *base, size_t n) { const size_t o = part(n * sizeof(T)); return base ? reinterpret_cast<T *>(base + o) : nullptr; }
};
// A zeroed host image of the head [first, end) of a device buffer laid out in parts: at(part) is the image's copy of the part; upload() puts it in place
struct HeadImage {
    uint8_t *d0;
    std::vector<uint8_t> h;
    HeadImage(void *first, void *end) : d0(static_cast<uint8_t *>(first)), h((size_t)(static_cast<uint8_t *>(end) - static_cast<uint8_t *>(first)), 0) {}
    template <class T> T *at(T *part) { return reinterpret_cast<T *>(h.data() + (reinterpret_cast<uint8_t *>(part) - d0)); }
    bool upload() { HIP_TRY(false, hipMemcpy(d0, h.data(), h.size(), hipMemcpyHostToDevice)); return true; }
};
// scratch device memory of one call
struct DeviceBytes {
    uint8_t *p = nullptr;
    DeviceBytes() = default;
    DeviceBytes(const DeviceBytes &) = delete;
    bool alloc(size_t bytes) { HIP_TRY(false, hipMalloc(&p, bytes)); return true; }
    template <class T> T *at(size_t off) const { return reinterpret_cast<T *>(p + off); }
    ~DeviceBytes() { if (p) (void)hipFree(p); }
};
}  // extern "C++"

// ---- column generation: the host side that greedy batch, sampling, beam search and contrastive search share ------------------------------
// Such a call generates with one column (and one K / V cache slot) per sequence: column p * per_prompt + j belongs to prompt p.  A mode checks its arguments,
// describes itself as a ColumnCall, hands it to run_column_call and reads its results back.
using ColumnStep = std::function<bool(int)>;

// ends the call's hold on the column-per-XCD launches (choose_column_path) when the call returns
struct XcBatchScope { biogpt_hip_ctx *c; ~XcBatchScope() { if (c) c->xc_batch = 0; } };

struct ColumnCall {
    // The call's hold on the device's pipeline slot and on the column-per-XCD launches ends with the description, when the mode returns.  A mode builds it after
    // its argument checks: XpCallScope's constructor does nothing and xc_batch is set by choose_column_path alone, so where the scopes begin cannot be observed.
    XpCallScope xp_scope;
    XcBatchScope xc_scope;
    explicit ColumnCall(biogpt_hip_ctx *c) : xp_scope(c), xc_scope{c} {}
    const int32_t *prompts = nullptr, *prompt_lens = nullptr;      // concatenated; `unit` names one in a message
    const char *unit = "prompt";
    int n_prompts = 0, per_prompt = 1, n_batch = 1;
    ColumnGraphs *graphs = nullptr;     // the mode's captured steps, valid for the call shape (key_a, key_b)
    int key_a = 0, key_b = 0;
    int extra_steps = 0;                // steps beyond one per token (contrastive: 1, the prompt's last token has a step of its own)
    StepForm form;                      // the mode names what it knows, its selection and whether that writes log-probabilities; run_column_call sets shared
                                        // and xcols
    int key_stride = 1;                 // positions a column can move on in one step, at most (prompt-lookup decoding: 1 + max_draft); > 1: the word behind
                                        // live_dev holds the furthest position of any column
    bool plain_steps = false;           // the step is no decode step of one column per sequence: never the column-per-XCD launches
    // A shared prefix (biogpt_hip_generate_*_prefix): sequence p is prefix ++ prompt p, and a prompt may be empty.  The first n_shared prefix rows are evaluated
    // once, into the slot behind the columns' (index n_prompts * per_prompt).  in_place: the steps read them there (the step is
    // ForwardPass::decode_step_shared); otherwise -- steps as column-per-XCD launches -- they are copied into every column's slot before the first step.
    const int32_t *prefix = nullptr;
    int n_prefix = 0;
    int n_shared = 0;                   // set by run_column_call, as in_place: the largest multiple of n_batch <= n_prefix - 1
    bool in_place = false;
    // set by run_column_call before any callable runs: the tokens to generate as clamped, the longest prompt, all prompt tokens
    int n_predict = 0, max_len = 0;
    long total = 0;
    // prepare() may set these two: they lie in buffers it grows
    const int32_t *live_dev = nullptr;  // device word that counts what still runs (null: every step is enqueued)
    float *hidden_store = nullptr;      // where the prompt pass leaves the hidden rows of its columns (null: nowhere)
    std::function<bool()> prepare;      // grows the mode's buffers, dropping its graphs where a pointer moves; runs before the graphs' key is looked at
    std::function<bool()> upload;       // the call's parameters, initial state and rules -> the device
    ColumnStep step;                    // step(t_max): the forward pass of all columns with t_max visible keys + the mode's selection, which leaves every column's
                                        // next token and position in ctx->seq
    std::function<bool()> after_ingest; // enqueued between the prompt pass and the first step
    std::function<bool()> before_sync;  // enqueued behind the last step, in front of the call's one synchronize (inside the timed span)
};

// n prompts, concatenated: none empty, every token valid; the longest and the sum of their lengths
static bool check_prompts(const biogpt_hip_ctx *c, const int32_t *prompts, const int32_t *lens, int n, const char *unit, int *max_len, long *total) {
    *max_len = 0; *total = 0;
    for (int p = 0; p < n; p++) {
        if (lens[p] < 1) BG_FAIL(false, "empty prompt (%s %d)", unit, p);
        if (!check_eval_args(c, prompts + *total, lens[p], 0)) return false;
        *max_len = std::max(*max_len, lens[p]);
        *total += lens[p];
    }
    return true;
}

// The gate of every call over column states.  wide_ok: the call is open to the wide chain (DESIGN.md 4.7 lists them); a wide file's row-tiled image is built
// here, before any capture -- it has no kernel to fall back to, so an image that does not fit is the call's error.
// A context in the SIMD association serves the single-sequence calls: every call over column states is refused by its name, before any launch
static bool assoc_refuses(const biogpt_hip_ctx *c, const char *what) {
    if (c->assoc && !c->assoc_chain) BG_FAIL(true, "%s runs over column states, which the SIMD association does not serve (biogpt_hip_assoc(ctx, 0) switches the context back to the scalar association)", what);
    return false;
}
static bool check_fast_chain(biogpt_hip_ctx *c, const char *what, bool wide_ok = false) {
    if (assoc_refuses(c, what)) return false;
    const int kind = chain_kind(c);
    if (kind == CHAIN_SIMD) {       // (nothing to build either)
        if (!wide_ok) BG_FAIL(false, "%s needs the BioGPT-base fast chain in the scalar association: the SIMD chain switched on for this context (biogpt_hip_assoc_chain) does not serve it (biogpt_hip_assoc(ctx, 0) switches the context back to the scalar association)", what);
        return true;
    }
    if (kind == CHAIN_FLOAT) {      // (nothing to build: the stage reads the arena's own rows)
        if (!wide_ok) BG_FAIL(false, "%s needs the BioGPT-base fast chain (block-quantized weights, d_model 1024, d_ff 4096): the float fast chain switched on for this %s file does not serve it", what, ftype_to_type(c->hp.ftype) == T_F16 ? "F16" : "F32");
        return true;
    }
    if (kind == CHAIN_NONE)
        BG_FAIL(false, "%s needs the BioGPT-base fast chain (block-quantized weights, d_model 1024, d_ff 4096, head size 64) or the wide one (block-quantized weights, head size 64, d_model a multiple of 64, d_ff of 32)", what);
    if (kind == CHAIN_BASE) return true;
    if (!wide_ok) BG_FAIL(false, "%s needs the BioGPT-base fast chain (d_model 1024, d_ff 4096): the wide fast chain of this file (d_model %d, d_ff %d) does not serve it", what, c->hp.d_model, c->hp.d_ff);
    HIP_TRY(false, hipSetDevice(c->device));
    if (!ensure_tile_images(c)) return false;
    if (c->tile_img == nullptr) BG_FAIL(false, "%s: no device memory for the row-tiled weight image the wide fast chain needs", what);
    return true;
}

// the device, the caches and the logits rows of n_seqs columns; `total` prompt tokens go through the prompt pass
// (n_slots: n_seqs, and one more for a shared prefix)
static bool begin_column_call(biogpt_hip_ctx *ctx, int n_slots, int n_seqs, long total) {
    HIP_TRY(false, hipSetDevice(ctx->device));
    if (!resident_stop(ctx)) return false;
    disarm_lineage(ctx);
    if (!ensure_seq_caches(ctx, n_slots)) return false;
    // matrix-core chain: decode steps have n_seqs columns, the prompt pass all prompt tokens; build the tiled weights before any graph capture
    // (a wide file has no other many-column kernel: always, and an image that does not fit is the call's error)
    // (a float file has no image at all: the float chain reads the arena's own rows; so does the SIMD chain)
    const bool wide = chain_kind_of(ctx->hp) == CHAIN_WIDE && chain_kind(ctx) != CHAIN_SIMD;
    const bool quant = is_quantized(ftype_to_type(ctx->hp.ftype)) && chain_kind(ctx) != CHAIN_SIMD;
    if (quant && (wide || std::max<long>(n_seqs, total) >= MFMA_MIN_DECODE_COLS) && !ensure_tile_images(ctx)) return false;
    if (wide && ctx->tile_img == nullptr) BG_FAIL(false, "no device memory for the row-tiled weight image the wide fast chain needs");
    return ensure_logits_rows(ctx, (size_t)n_seqs);
}

// the captured steps serve calls of one shape: another shape drops them
static void column_graphs_for(ColumnGraphs &gs, int a, int b) {
    if (gs.key_a == a && gs.key_b == b) return;
    drop_graphs(gs);
    gs.key_a = a; gs.key_b = b;
}

// Column p * per_prompt + j starts at prompt p's LAST token (the prompt pass leaves it to the first step), in the cache slot of its own index
static void fill_column_starts(bgk::SeqState *hs, int p, int per_prompt, int n_prompt, int32_t last_token) {
    for (int j = 0; j < per_prompt; j++) {
        bgk::SeqState &st = hs[(size_t)p * per_prompt + j];
        st = bgk::SeqState{};
        st.n_past = n_prompt - 1; st.token = last_token; st.seq_id = p * per_prompt + j;
    }
}
// pos0: the position of every prompt's first token (rows in front of it: a shared prefix); shared: the rows the steps read in another slot (none: {})
static bool upload_column_starts(biogpt_hip_ctx *ctx, const int32_t *prompts, const int32_t *lens, int n_prompts, int per_prompt, int pos0 = 0,
                                 SharedRows shared = SharedRows{}) {
    std::vector<bgk::SeqState> hs((size_t)n_prompts * per_prompt);
    size_t o = 0;
    for (int p = 0; p < n_prompts; p++) {
        o += (size_t)lens[p];
        fill_column_starts(hs.data(), p, per_prompt, pos0 + lens[p], prompts[o - 1]);
    }
    for (bgk::SeqState &st : hs) { st.pad[0] = shared.n; st.pad[1] = shared.n > 0 ? shared.slot : 0; }
    HIP_TRY(false, hipMemcpy(ctx->seq, hs.data(), sizeof(bgk::SeqState) * hs.size(), hipMemcpyHostToDevice));
    return true;
}

// 2 .. 8 columns: the steps as column-per-XCD launches while this call holds the device's pipeline slot.  Decided ONCE per call, before any capture: a
// graph is replayed only in the state it was captured for.  Returns the choice (0 | 1), which is also ctx->xc_batch until the call's XcBatchScope ends.
static int choose_column_path(biogpt_hip_ctx *ctx, int n_seqs, int max_len) {
    ctx->xc_batch = (chain_kind(ctx) != CHAIN_SIMD && n_seqs >= 2 && n_seqs <= 8 && max_len + 1 <= 256 && xcols_prepare(ctx, n_seqs, std::min(256, max_len + 1)) && xpipe_usable(ctx, 256)) ? 1 : 0;
    return ctx->xc_batch;
}

// The keys a step can see at most.  Step k (0: the prompt's last token) of a call whose columns move on by at most `stride` positions per step has columns up to
// position max_len - 1 + (k + 1) * stride - 1; with stride 1 that is the one key per step of every mode but prompt-lookup decoding.
struct ColumnKeys {
    int max_len, stride, P;
    // steps enqueued between two reads of the live word.  One group stays in flight behind the word the host waits for, so up to two groups run after the end:
    // little beside one step per token, half a call where a step is 8 tokens -- a stride > 1 polls every second step (a step of several columns per sequence
    // is long beside a graph launch)
    int group() const { return stride > 1 ? 2 : 8; }
    int worst(int k) const { return (int)std::min<long>(P, (long)max_len + (long)(k + 1) * stride - 1); }
    int first_replayed() const { return std::min(P, max_len + 1); }      // no replayed step is bounded lower
};

// Captures `step` for the context buckets of steps 2 .. n_steps (t_max = max_len + 1 .. keys.worst(n_steps - 1): the ones run_column_steps replays) into
// the slots of `form`, where they are not there yet.  *use_graph: whether the steps are replayed at all.
static bool capture_column_steps(biogpt_hip_ctx *ctx, ColumnGraphs &graphs, const StepForm &form, const ColumnKeys &keys, int n_steps, const ColumnStep &step, bool *use_graph) {
    *use_graph = ctx->opt.no_graph == 0 && (ctx->xc_batch != 0 || plain_graph_begin(ctx));      // (a captured five-launch step is not replayed beside another context's persistent launch)
    if (*use_graph && n_steps > 1) {
        for (int b = graph_bucket(keys.first_replayed()); b <= graph_bucket(keys.worst(n_steps - 1)); b++) {
            hipGraphExec_t &exec = graphs.exec[ColumnGraphs::slot(form, b)];
            if (exec) continue;
            hipGraph_t g = nullptr;
            HIP_TRY(false, hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal));
            const bool ok = step(bucket_tmax(ctx, b));
            hipError_t e = hipStreamEndCapture(ctx->stream, &g);
            if (!ok) { if (g) (void)hipGraphDestroy(g); return false; }
            HIP_TRY(false, e);
            HIP_TRY(false, hipGraphInstantiate(&exec, g, nullptr, nullptr, 0));
            (void)hipGraphDestroy(g);
        }
    }
    HIP_TRY(false, hipStreamSynchronize(ctx->stream));
    return true;
}

// Prompt ingestion for ALL prompts together (main.cpp:129-137 per prompt), packed into common passes (pack_column_passes): prompt p fills the cache slot of
// its first column, kv_share_kernel copies its rows to its other per_prompt - 1 slots.  The pass only has to fill the K / V caches: the first step
// re-evaluates each prompt's LAST token (same K / V row, same visible keys as its chunk gave it).
// A shared prefix (shared.n > 0 rows of `prefix`): those rows go once into slot shared.slot, as the prompt columns of one sequence; `prompts` are then the
// sequences' tokens from position shared.n on, packed columns that read the shared rows where they lie.  Steps that know one slot per column (!cc.in_place):
// kv_prefix_copy_kernel then copies the shared rows into every column's slot.  kv_share_kernel copies a prompt's own rows only, on either path.
// prompts / lens: the call's prompts, or behind a prefix what follows the shared rows.
static bool ingest_column_prompts(biogpt_hip_ctx *ctx, const ColumnCall &cc, const int32_t *prompts, const int32_t *lens, SharedRows shared) {
    const auto &hp = ctx->hp;
    const int n_prompts = cc.n_prompts, n_batch = cc.n_batch, per_prompt = cc.per_prompt;
    float *const hidden_store = cc.hidden_store;
    const int32_t *const prefix = cc.prefix;
    const bool copy_shared = !cc.in_place;
    const int64_t seq_stride = (int64_t)hp.n_layer * hp.n_positions * hp.d_model;
    if (shared.n > 0) {
        const int32_t n = shared.n;
        if (!pack_column_passes(ctx, prefix, &n, 1, n_batch, [&](int n_cols, int t_max, size_t) { return enqueue_forward(ctx, ForwardPass::packed_prompts(n_cols, t_max)); },
                                1, shared.slot))
            return false;
    }
    if (!pack_column_passes(ctx, prompts, lens, n_prompts, n_batch,
                            [&](int n_cols, int t_max, size_t) {
                                return enqueue_forward(ctx, shared.n > 0 ? ForwardPass::packed_continuations(n_cols, t_max, n_cols)
                                                                         : ForwardPass::packed_prompts_hidden(n_cols, t_max, hidden_store, per_prompt));
                            },
                            per_prompt, 0, shared))
        return false;
    if (per_prompt > 1) {
        hipLaunchKernelGGL(bgk::kv_share_kernel, dim3(hp.n_layer * hp.n_head, n_prompts * per_prompt, 2), dim3(256), 0, ctx->stream, ctx->seq, per_prompt, shared.n, ctx->bk, ctx->bv,
                           seq_stride, hp.n_positions, hp.d_model / hp.n_head);
        HIP_TRY(false, hipGetLastError());
    }
    if (shared.n > 0 && copy_shared) {
        hipLaunchKernelGGL(bgk::kv_prefix_copy_kernel, dim3(hp.n_layer * hp.n_head, n_prompts * per_prompt, 2), dim3(256), 0, ctx->stream, shared.n, shared.slot, ctx->bk, ctx->bv,
                           seq_stride, hp.n_positions, hp.d_model / hp.n_head);
        HIP_TRY(false, hipGetLastError());
    }
    return true;
}

// The prompts of a call behind a shared prefix, checked: the prefix is not empty, a suffix may be, every token is valid and every sequence fits the position
// table.  eff / eff_lens: every sequence's tokens from position n_shared on (prefix[n_shared:] ++ suffix, never empty).
static bool prefix_prompts(const biogpt_hip_ctx *c, ColumnCall &cc, std::vector<int32_t> &eff, std::vector<int32_t> &eff_lens) {
    const int P = c->hp.n_positions, V = c->hp.n_vocab;
    if (cc.n_prefix < 1) BG_FAIL(false, "n_prefix must be >= 1 (got %d)", cc.n_prefix);
    if (cc.n_prefix > P) BG_FAIL(false, "n_prefix (%d) exceeds n_positions (%d)", cc.n_prefix, P);
    for (int i = 0; i < cc.n_prefix; i++)
        if (cc.prefix[i] < 0 || cc.prefix[i] >= V) BG_FAIL(false, "token id %d (prefix, position %d) out of range [0, %d)", cc.prefix[i], i, V);
    cc.n_shared = (cc.n_prefix - 1) / cc.n_batch * cc.n_batch;
    const int own = cc.n_prefix - cc.n_shared;
    size_t off = 0;
    int max_suffix = 0;
    for (int p = 0; p < cc.n_prompts; p++) {
        const int len = cc.prompt_lens[p];
        if (len < 0) BG_FAIL(false, "suffix_lens[%d] (%d) is negative", p, len);
        if (len > P - cc.n_prefix) BG_FAIL(false, "n_prefix (%d) + suffix_lens[%d] (%d) exceeds n_positions (%d)", cc.n_prefix, p, len, P);
        for (int i = 0; i < len; i++) {
            const int32_t t = cc.prompts[off + (size_t)i];
            if (t < 0 || t >= V) BG_FAIL(false, "token id %d (%s %d, position %d) out of range [0, %d)", t, cc.unit, p, i, V);
        }
        eff.insert(eff.end(), cc.prefix + cc.n_shared, cc.prefix + cc.n_prefix);
        eff.insert(eff.end(), cc.prompts + off, cc.prompts + off + (size_t)len);
        eff_lens.push_back(own + len);
        max_suffix = std::max(max_suffix, len);
        off += (size_t)len;
    }
    cc.max_len = cc.n_prefix + max_suffix;
    cc.total = (long)cc.n_shared + (long)eff.size();
    return true;
}

// Step 1 eagerly (the last prompt token of every column, t_max = keys.worst(0)), then steps 2 .. n_steps replayed or eager, enqueued in groups of keys.group().
// live_dev (or null): a device word that holds how many sequences / searches still run.  It is copied to one of two pinned slots after each
// group, and once the group BEFORE the one just enqueued reports none, nothing more is enqueued (one group stays in flight; steps after the end change nothing).
// keys.stride > 1: the word behind live_dev (the furthest position of any column) travels with it, and a step k behind the last step e whose word has come back
// is bounded by that position + (k - e) * stride instead of keys.worst(k): attention follows the context the columns really have.
static bool run_column_steps(biogpt_hip_ctx *ctx, const ColumnGraphs &graphs, const StepForm &form, bool use_graph, const ColumnKeys &keys, int n_steps, const ColumnStep &step,
                             const int32_t *live_dev) {
    if (!step(keys.worst(0))) return false;
    const bool with_pos = live_dev && keys.stride > 1;
    int seen_step = -1, seen_pos = 0, grp_last[2] = {0, 0};
    for (int k = 1, grp = 0; k < n_steps; grp++) {
        for (const int end = std::min(n_steps - 1, k + keys.group() - 1); k <= end; k++) {
            int t_max = keys.worst(k);
            if (seen_step >= 0) t_max = std::min<long>(t_max, std::max<long>(keys.first_replayed(), (long)seen_pos + (long)(k - seen_step) * keys.stride));
            if (use_graph) HIP_TRY(false, hipGraphLaunch(graphs.exec[ColumnGraphs::slot(form, graph_bucket(t_max))], ctx->stream));
            else if (!step(t_max)) return false;
        }
        if (!live_dev) continue;
        HIP_TRY(false, hipMemcpyAsync(ctx->live_host + 2 * (grp & 1), live_dev, with_pos ? 8 : 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(false, hipEventRecord(ctx->live_ev[grp & 1], ctx->stream));
        grp_last[grp & 1] = k - 1;
        if (grp > 0) {
            const int o = (grp - 1) & 1;
            HIP_TRY(false, hipEventSynchronize(ctx->live_ev[o]));
            if (ctx->live_host[2 * o] <= 0) break;
            if (with_pos) { seen_step = grp_last[o]; seen_pos = ctx->live_host[2 * o + 1]; }
        }
    }
    return true;
}

// The one order of a column call.  Returns the tokens to generate as clamped (> 0) once every step has run and the stream has drained; 0: the longest prompt
// leaves no room (nothing was touched); -1: a bad prompt; -2: a failure.
static int run_column_call(biogpt_hip_ctx *ctx, ColumnCall &cc, int n_predict, double *seconds_out) {
    // behind a prefix the call's prompts are what follows the shared rows; max_len stays the longest whole sequence
    std::vector<int32_t> eff, eff_lens;
    const int32_t *prompts = cc.prompts, *lens = cc.prompt_lens;
    if (cc.prefix) {
        if (!prefix_prompts(ctx, cc, eff, eff_lens)) return -1;
        prompts = eff.data(); lens = eff_lens.data();
    } else if (!check_prompts(ctx, cc.prompts, cc.prompt_lens, cc.n_prompts, cc.unit, &cc.max_len, &cc.total)) {
        return -1;
    }
    cc.n_predict = std::min(n_predict, ctx->hp.n_positions - cc.max_len);  // main.cpp:82, for the longest prompt
    if (cc.n_predict <= 0) return 0;
    const int n_seqs = cc.n_prompts * cc.per_prompt, n_steps = cc.n_predict + cc.extra_steps;
    const SharedRows shared{cc.n_shared, n_seqs};       // (n_shared == 0: nothing is shared and every launch is that of the call without a prefix)
    if (!begin_column_call(ctx, n_seqs + (cc.prefix ? 1 : 0), n_seqs, cc.total)) return -2;
    if (cc.prepare && !cc.prepare()) return -2;      // buffers grow and graphs drop BEFORE the key is looked at: a captured step never holds a freed pointer
    column_graphs_for(*cc.graphs, cc.key_a, cc.key_b);
    const int xc = cc.plain_steps ? 0 : choose_column_path(ctx, n_seqs, cc.max_len);
    cc.in_place = cc.n_shared > 0 && xc == 0;
    if (!upload_column_starts(ctx, prompts, lens, cc.n_prompts, cc.per_prompt, cc.n_shared, cc.in_place ? shared : SharedRows{})) return -2;
    if (cc.upload && !cc.upload()) return -2;
    cc.form.shared = cc.in_place; cc.form.xcols = xc != 0;
    const ColumnKeys keys{cc.max_len, cc.key_stride, ctx->hp.n_positions};
    bool use_graph;
    if (!capture_column_steps(ctx, *cc.graphs, cc.form, keys, n_steps, cc.step, &use_graph)) return -2;

    const auto t0 = std::chrono::steady_clock::now();
    if (!ingest_column_prompts(ctx, cc, prompts, lens, shared)) return -2;
    if (cc.after_ingest && !cc.after_ingest()) return -2;
    if (!run_column_steps(ctx, *cc.graphs, cc.form, use_graph, keys, n_steps, cc.step, cc.live_dev)) return -2;
    if (cc.before_sync && !cc.before_sync()) return -2;
    HIP_TRY(-2, hipStreamSynchronize(ctx->stream));
    const auto t1 = std::chrono::steady_clock::now();
    if (!xpipe_check(ctx)) return -2;      // (steps as column-per-XCD launches: a disturbed one spoils the run -- the mode's caller repeats it on the launch chain)
    if (seconds_out) *seconds_out = std::chrono::duration<double>(t1 - t0).count();
    // (a call that failed, or whose n_predict clamped to 0, leaves the stats of the last call that generated)
    if (cc.prefix) { ctx->prefix_stats[0] = cc.n_shared; ctx->prefix_stats[1] = (int32_t)cc.total; ctx->prefix_stats[2] = xc; ctx->prefix_stats[3] = n_seqs; }
    return cc.n_predict;
}

// ---- log-probabilities of generated tokens: what greedy batch and sampled generation add when asked (kernels_genlp.hip.h) ----------------------
// The selection kernel of the step writes entry n_gen of every sequence into the context's block: GenLpCtl {n_top, stride = the call's n_predict as
// clamped}, then lp [seqs][stride], top_ids and top_lp [seqs][stride][n_top] -- the layout of the caller's arrays, so the read-out is one copy each.
// The block is allocated once, for GENLP_COLS sequences of n_positions entries with GENLP_MAX_TOP alternatives: a captured step keeps its pointers and,
// n_top and stride being device words, serves every K.
constexpr int GENLP_COLS = 512;     // columns of a call, at most
struct GenLpBufs {
    bgk::GenLpCtl *ctl;
    float *lp;
    int32_t *top_ids;
    float *top_lp;
    size_t bytes;
    bgk::GenLpOut out() const { return bgk::GenLpOut{ctl, lp, top_ids, top_lp}; }
};
static GenLpBufs genlp_bufs_at(uint8_t *base, size_t entries, size_t n_top = bgk::GENLP_MAX_TOP) {
    ByteLayout l;
    GenLpBufs b{};
    b.ctl = l.take<bgk::GenLpCtl>(base, 1); b.lp = l.take<float>(base, entries);
    b.top_ids = l.take<int32_t>(base, entries * n_top); b.top_lp = l.take<float>(base, entries * n_top);
    b.bytes = l.bytes();
    return b;
}
// the request of a call, before any HIP call; n_vocab < 0: not known yet
static bool check_gen_logprobs(const biogpt_hip_gen_logprobs *lp, int n_vocab) {
    if (!lp) BG_FAIL(false, "null argument: logprobs");
    if (!lp->lp) BG_FAIL(false, "null argument: logprobs.lp");
    if (lp->n_top < 0 || lp->n_top > bgk::GENLP_MAX_TOP) BG_FAIL(false, "logprobs.n_top must be in [0, %d] (got %d)", bgk::GENLP_MAX_TOP, lp->n_top);
    if (lp->n_top > 0 && !lp->top_ids) BG_FAIL(false, "null argument: logprobs.top_ids (n_top is %d)", lp->n_top);
    if (lp->n_top > 0 && !lp->top_lp) BG_FAIL(false, "null argument: logprobs.top_lp (n_top is %d)", lp->n_top);
    if (n_vocab >= 0 && lp->n_top > n_vocab) BG_FAIL(false, "logprobs.n_top (%d) exceeds n_vocab (%d)", lp->n_top, n_vocab);
    return true;
}
static bool genlp_prepare(biogpt_hip_ctx *ctx, GenLpBufs *b) {
    const size_t entries = (size_t)GENLP_COLS * ctx->hp.n_positions;
    if (!ctx->genlp_buf) HIP_TRY(false, hipMalloc(&ctx->genlp_buf, genlp_bufs_at(nullptr, entries).bytes));
    *b = genlp_bufs_at(ctx->genlp_buf, entries);
    return true;
}
static bool genlp_upload(const GenLpBufs &b, int n_top, int stride) {
    bgk::GenLpCtl h{};
    h.n_top = n_top; h.stride = stride;
    HIP_TRY(false, hipMemcpy(b.ctl, &h, sizeof(h), hipMemcpyHostToDevice));
    return true;
}
// The call's results -> the caller's arrays: [n_seqs][n_predict] and [n_seqs][n_predict][n_top].  lens (or null: every sequence has n_predict entries):
// entries at or past a sequence's length read 0 (lp, top_lp) and -1 (top_ids).
static bool genlp_read(const GenLpBufs &b, const biogpt_hip_gen_logprobs *lp, int n_seqs, int n_predict, const int32_t *lens) {
    const size_t n = (size_t)n_seqs * n_predict, K = (size_t)lp->n_top;
    HIP_TRY(false, hipMemcpy(lp->lp, b.lp, n * 4, hipMemcpyDeviceToHost));
    if (K > 0) {
        HIP_TRY(false, hipMemcpy(lp->top_ids, b.top_ids, n * K * 4, hipMemcpyDeviceToHost));
        HIP_TRY(false, hipMemcpy(lp->top_lp, b.top_lp, n * K * 4, hipMemcpyDeviceToHost));
    }
    for (int r = 0; lens && r < n_seqs; r++) {
        const size_t at = (size_t)r * n_predict + (size_t)lens[r], end = (size_t)(r + 1) * n_predict;
        std::fill(lp->lp + at, lp->lp + end, 0.0f);
        if (K > 0) {
            std::fill(lp->top_ids + at * K, lp->top_ids + end * K, -1);
            std::fill(lp->top_lp + at * K, lp->top_lp + end * K, 0.0f);
        }
    }
    return true;
}

// prefix != null (biogpt_hip_generate_greedy_prefix): sequence s is prefix ++ prompt s, the prompts are suffixes and may be empty;
// lp != null (biogpt_hip_generate_greedy_batch_lp): genlp_greedy_rows_kernel is the selection, and lp's arrays take the log-probabilities
static int generate_greedy_batch_once(biogpt_hip_ctx *ctx, const int32_t *prompts, const int32_t *prompt_lens, int32_t n_seqs,
                                      int32_t n_batch, int32_t n_predict, int32_t *out_ids, double *seconds_out, const int32_t *prefix = nullptr, int32_t n_prefix = 0,
                                      const biogpt_hip_gen_logprobs *lp = nullptr) {
    clear_error();
    if (!ctx || !prompts || !prompt_lens || !out_ids) BG_FAIL(-1, "null argument");
    if (lp && !check_gen_logprobs(lp, ctx->hp.n_vocab)) return -1;
    if (!ctx->ready) BG_FAIL(-1, "model has no tensors loaded (empty model): cannot evaluate");
    if (session_refuses(ctx)) return -1;
    if (prefix && (n_seqs < 1 || n_seqs > 511)) BG_FAIL(-1, "n_seqs must be in [1, 511] behind a prefix (got %d)", n_seqs);   // one slot holds the prefix
    // (the plain call meets the gate in enqueue_forward, as ever; the two variants are not open to the wide chain and say so by name)
    if ((prefix || lp) && !check_fast_chain(ctx, prefix ? "generation behind a shared prefix" : "generation with log-probabilities")) return -1;
    if (assoc_refuses(ctx, "batched greedy generation")) return -1;
    if (n_seqs < 1 || n_seqs > 512) BG_FAIL(-1, "n_seqs must be in [1, 512]");   // activation buffers hold n_positions >= 512 columns; each sequence owns a full F32 KV cache
    if (n_seqs > hp_cols(ctx)) BG_FAIL(-1, "n_seqs (%d) exceeds the %d activation columns of this model", n_seqs, hp_cols(ctx));
    if (n_batch < 1) BG_FAIL(-1, "n_batch must be >= 1");
    const int P = ctx->hp.n_positions, V = ctx->hp.n_vocab;
    ColumnCall cc(ctx);
    cc.prompts = prompts; cc.prompt_lens = prompt_lens; cc.unit = "sequence";
    cc.n_prompts = n_seqs; cc.n_batch = n_batch;
    cc.graphs = &ctx->graphs_greedy; cc.key_a = n_seqs;
    cc.prefix = prefix; cc.n_prefix = n_prefix;
    GenLpBufs lb{};
    if (lp) {
        cc.form.lp = true;
        cc.prepare = [&]() -> bool { return genlp_prepare(ctx, &lb); };
        cc.upload = [&]() -> bool { return genlp_upload(lb, lp->n_top, cc.n_predict); };
    }
    cc.step = [&](int t_max) -> bool {      // every step's arg-max is the next token
        if (!enqueue_forward(ctx, cc.in_place ? ForwardPass::decode_step_shared(n_seqs, t_max, cc.n_shared) : ForwardPass::decode_step(n_seqs, t_max))) return false;
        if (lp)
            hipLaunchKernelGGL(bgk::genlp_greedy_rows_kernel, dim3(n_seqs), dim3(bgk::LP_THREADS), 0, ctx->stream, ctx->logits_all, V, V, ctx->seq, ctx->seq_gen, P, 1, lb.out());
        else
            hipLaunchKernelGGL(bgk::argmax_rows_kernel, dim3(n_seqs), dim3(bgk::ARGMAX_ROWS_THREADS), 0, ctx->stream, ctx->logits_all, V, V, ctx->seq, 0, ctx->seq_gen, P, 1);
        HIP_TRY(false, hipGetLastError());
        return true;
    };
    n_predict = run_column_call(ctx, cc, n_predict, seconds_out);
    if (n_predict <= 0) return n_predict;
    std::vector<int32_t> gen((size_t)n_seqs * P);
    HIP_TRY(-2, hipMemcpy(gen.data(), ctx->seq_gen, gen.size() * 4, hipMemcpyDeviceToHost));
    for (int s = 0; s < n_seqs; s++) std::memcpy(out_ids + (size_t)s * n_predict, gen.data() + (size_t)s * P, (size_t)n_predict * 4);
    if (lp && !genlp_read(lb, lp, n_seqs, n_predict, nullptr)) return -2;
    return n_predict;
}
int biogpt_hip_generate_greedy_batch(biogpt_hip_ctx *ctx, const int32_t *prompts, const int32_t *prompt_lens, int32_t n_seqs,
                                     int32_t n_batch, int32_t n_predict, int32_t *out_ids, double *seconds_out) {
    return with_xpipe_retry(ctx, 0, [&] { return generate_greedy_batch_once(ctx, prompts, prompt_lens, n_seqs, n_batch, n_predict, out_ids, seconds_out); });
}

// ---- generation behind a shared prefix: the prefix's first n_shared rows evaluated once, read in place by every sequence (or copied, 2 .. 8 columns) ----
static bool check_prefix_pointers(const biogpt_hip_ctx *ctx, const int32_t *prefix, const int32_t *suffixes, const int32_t *suffix_lens) {
    clear_error();
    if (!ctx) BG_FAIL(false, "null context");
    if (!prefix) BG_FAIL(false, "null argument: prefix");
    if (!suffixes) BG_FAIL(false, "null argument: suffixes");
    if (!suffix_lens) BG_FAIL(false, "null argument: suffix_lens");
    return true;
}
int biogpt_hip_generate_greedy_prefix(biogpt_hip_ctx *ctx, const int32_t *prefix, int32_t n_prefix, const int32_t *suffixes, const int32_t *suffix_lens, int32_t n_seqs,
                                      int32_t n_batch, int32_t n_predict, int32_t *out_ids, double *seconds_out) {
    if (!check_prefix_pointers(ctx, prefix, suffixes, suffix_lens)) return -1;
    if (!out_ids) BG_FAIL(-1, "null argument: out_ids");
    return with_xpipe_retry(ctx, 0, [&] {
        return generate_greedy_batch_once(ctx, suffixes, suffix_lens, n_seqs, n_batch, n_predict, out_ids, seconds_out, prefix, n_prefix);
    });
}
// the pointers of a *_lp call: the request first (a caller's mistake there is named whatever else is wrong), then those of the form it takes
static bool check_lp_pointers(const biogpt_hip_ctx *ctx, const biogpt_hip_gen_logprobs *lp, const int32_t *prefix, int32_t n_prefix, const int32_t *suffixes,
                              const int32_t *suffix_lens) {
    clear_error();
    if (!check_gen_logprobs(lp, -1)) return false;
    if (!prefix && n_prefix != 0) BG_FAIL(false, "n_prefix must be 0 without a prefix (got %d)", n_prefix);
    if (prefix) return check_prefix_pointers(ctx, prefix, suffixes, suffix_lens);
    if (!ctx) BG_FAIL(false, "null context");
    return true;
}
// biogpt_hip_generate_greedy_batch (prefix == null) or biogpt_hip_generate_greedy_prefix with the log-probabilities of the generated tokens
int biogpt_hip_generate_greedy_batch_lp(biogpt_hip_ctx *ctx, const int32_t *prefix, int32_t n_prefix, const int32_t *suffixes, const int32_t *suffix_lens, int32_t n_seqs,
                                        int32_t n_batch, int32_t n_predict, int32_t *out_ids, double *seconds_out, const biogpt_hip_gen_logprobs *logprobs) {
    if (!check_lp_pointers(ctx, logprobs, prefix, n_prefix, suffixes, suffix_lens)) return -1;
    if (!out_ids) BG_FAIL(-1, "null argument: out_ids");
    return with_xpipe_retry(ctx, 0, [&] {
        return generate_greedy_batch_once(ctx, suffixes, suffix_lens, n_seqs, n_batch, n_predict, out_ids, seconds_out, prefix, prefix ? n_prefix : 0, logprobs);
    });
}
int biogpt_hip_prefix_stats(const biogpt_hip_ctx *ctx, int32_t out[4]) {
    clear_error();
    if (!ctx) BG_FAIL(-1, "null context");
    if (!out) BG_FAIL(-1, "null argument: out");
    std::memcpy(out, ctx->prefix_stats, sizeof(ctx->prefix_stats));
    return 0;
}

// ---- sequence scoring: teacher-forced causal passes, the log-softmax of every row on the device (kernels_score.hip.h) ----------------
// Row i of a scored sequence sees keys [0, n_past + i]: the prompt pass of biogpt_hip_eval_prompt with n_batch = 1 (DevState::chunk = 1;
// one column per sequence token, SeqState::t_vis = position + 1, for score_batch), whatever BIOGPT_HIP_CAUSAL says.  The lm_head runs over
// every column of a pass into logits_all (at most one pass of rows), logprob_rows_kernel reduces each row to {log-probability of the
// target, arg-max, target logit}; the call's targets go up once, its outputs come back in one copy.
static bool check_targets(const biogpt_hip_ctx *c, const int32_t *targets, int n, int seq) {
    if (!targets) return true;
    for (int i = 0; i < n; i++)
        if (targets[i] >= c->hp.n_vocab) BG_FAIL(false, "target id %d (sequence %d, row %d) out of range: must be < %d (negative: row not scored)", targets[i], seq, i, c->hp.n_vocab);
    return true;
}

// the targets of all `total` rows of the call (NULL: the next token of the same sequence, -1 for its last row) -> sc_tgt;
// sc_out laid out [3][total] for this call: log-probabilities, arg-max ids, target logits
static bool score_setup(biogpt_hip_ctx *c, const int32_t *seqs, const int32_t *lens, int n_seqs, const int32_t *targets, size_t total) {
    if (total > c->sc_cap) {
        for (void *p : {(void *)c->sc_tgt, (void *)c->sc_out}) if (p) (void)hipFree(p);
        c->sc_tgt = nullptr; c->sc_out = nullptr; c->sc_cap = 0;
        HIP_TRY(false, hipMalloc(&c->sc_tgt, total * 4));
        HIP_TRY(false, hipMalloc(&c->sc_out, 3 * total * 4));
        c->sc_cap = total;
    }
    std::vector<int32_t> tg(total);
    size_t off = 0;
    for (int s = 0; s < n_seqs; s++) {
        for (int i = 0; i < lens[s]; i++) tg[off + i] = targets ? targets[off + i] : (i + 1 < lens[s] ? seqs[off + i + 1] : -1);
        off += (size_t)lens[s];
    }
    HIP_TRY(false, hipMemcpy(c->sc_tgt, tg.data(), total * 4, hipMemcpyHostToDevice));
    return true;
}

// the log-softmax of the m rows logits_all holds for flat rows [flat0, flat0 + m) of the call
static bool enqueue_logprob(biogpt_hip_ctx *c, int m, size_t flat0, size_t total) {
    const int V = c->hp.n_vocab;
    float *const lp = reinterpret_cast<float *>(c->sc_out) + flat0;
    int32_t *const am = reinterpret_cast<int32_t *>(c->sc_out + total) + flat0;
    float *const lg = reinterpret_cast<float *>(c->sc_out + 2 * total) + flat0;
    hipLaunchKernelGGL(bgk::logprob_rows_kernel, dim3(m), dim3(bgk::LP_THREADS), 0, c->stream, c->logits_all, V, V, c->sc_tgt + flat0, lp, am, lg);
    HIP_TRY(false, hipGetLastError());
    return true;
}

// one copy of the outputs back, then into the caller's arrays (argmax_out / logit_out may be NULL)
static int score_finish(biogpt_hip_ctx *c, size_t total, float *logprob_out, int32_t *argmax_out, float *logit_out) {
    std::vector<uint32_t> h(3 * total);
    HIP_TRY(-2, hipMemcpyAsync(h.data(), c->sc_out, 3 * total * 4, hipMemcpyDeviceToHost, c->stream));
    if (!wait_stream(c)) return -2;
    std::memcpy(logprob_out, h.data(), total * 4);
    if (argmax_out) std::memcpy(argmax_out, h.data() + total, total * 4);
    if (logit_out) std::memcpy(logit_out, h.data() + 2 * total, total * 4);
    return 0;
}

// The causal passes of ONE sequence in the context's own cache (biogpt_hip_score, biogpt_hip_hidden): the passes of biogpt_hip_eval_prompt(tokens, n_past,
// n_batch = 1) -- same borders, same K / V rows.  causal_pass_cols: the columns of a pass at most (0: failure), with the tiled weights built if the first
// pass takes the matrix cores; causal_passes: per pass the state upload (a pass of several columns: chunks of one), then pass(at, m) for tokens [at, at + m).
static int causal_pass_cols(biogpt_hip_ctx *ctx, int n) {
    const int max_cols = std::min(std::max(1, ctx->opt.prompt_cols), hp_cols(ctx));
    if (std::min(max_cols, n) >= MFMA_MIN_PASS_COLS && is_quantized(ftype_to_type(ctx->hp.ftype)) && !ensure_tile_images(ctx)) return 0;
    return max_cols;
}
extern "C++" template <class Pass>
bool causal_passes(biogpt_hip_ctx *ctx, const int32_t *tokens, int n, int n_past, int max_cols, Pass pass) {
    for (int at = 0; at < n;) {
        const int m = std::min(max_cols, n - at);
        if (!upload_state(ctx, tokens + at, m, n_past + at, m > 1 ? 1 : 0) || !pass(at, m)) return false;
        at += m;
    }
    return true;
}

static int score_once(biogpt_hip_ctx *ctx, const int32_t *tokens, int32_t n, int32_t n_past, const int32_t *targets,
                      float *logprob_out, int32_t *argmax_out, float *logit_out) {
    XpCallScope xp_scope(ctx);
    clear_error();
    if (!check_eval_args(ctx, tokens, n, n_past)) return -1;
    if (!logprob_out) BG_FAIL(-1, "null logprob buffer");
    if (!check_targets(ctx, targets, n, 0)) return -1;
    HIP_TRY(-2, hipSetDevice(ctx->device));
    if (!resident_stop(ctx)) return -2; disarm_lineage(ctx);
    const int max_cols = causal_pass_cols(ctx, n);
    if (!max_cols) return -2;
    if (!ensure_logits_rows(ctx, (size_t)std::min(max_cols, (int)n)) || !score_setup(ctx, tokens, &n, 1, targets, (size_t)n)) return -2;
    const size_t V = (size_t)ctx->hp.n_vocab;
    const bool ok = causal_passes(ctx, tokens, n, n_past, max_cols, [&](int at, int m) -> bool {
        if (!enqueue_forward(ctx, ForwardPass::scored(m, n_past + at + m)) || !enqueue_logprob(ctx, m, (size_t)at, (size_t)n)) return false;
        if (at + m == n)   // the last row is what biogpt_hip_read_logits / biogpt_hip_logits_device return afterwards
            HIP_TRY(false, hipMemcpyAsync(ctx->logits, ctx->logits_all + (size_t)(m - 1) * V, V * 4, hipMemcpyDeviceToDevice, ctx->stream));
        return true;
    });
    if (!ok) return -2;
    return score_finish(ctx, (size_t)n, logprob_out, argmax_out, logit_out);
}

static int score_batch_once(biogpt_hip_ctx *ctx, const int32_t *seqs, const int32_t *lens, int32_t n_seqs, const int32_t *targets,
                            float *logprob_out, int32_t *argmax_out, float *logit_out) {
    XpCallScope xp_scope(ctx);
    clear_error();
    if (!ctx) BG_FAIL(-1, "null context");
    if (!seqs || !lens || !logprob_out) BG_FAIL(-1, "null argument");
    if (!ctx->ready) BG_FAIL(-1, "model has no tensors loaded (empty model): cannot evaluate");
    if (session_refuses(ctx)) return -1;
    if (n_seqs < 1 || n_seqs > 512) BG_FAIL(-1, "n_seqs must be in [1, 512]");   // each sequence owns a full F32 KV cache
    if (!check_fast_chain(ctx, "batched scoring", true)) return -1;
    size_t total = 0;
    for (int s = 0; s < n_seqs; s++) {
        if (lens[s] < 1) BG_FAIL(-1, "empty sequence (sequence %d)", s);
        if (!check_eval_args(ctx, seqs + total, lens[s], 0)) return -1;
        if (!check_targets(ctx, targets ? targets + total : nullptr, lens[s], s)) return -1;
        total += (size_t)lens[s];
    }
    HIP_TRY(-2, hipSetDevice(ctx->device));
    if (!resident_stop(ctx)) return -2; disarm_lineage(ctx);
    // every sequence from position 0 in its own K / V cache (bk / bv): the context's own cache and position stay as they are
    const size_t max_cols = (size_t)std::min(std::max(1, ctx->opt.prompt_cols), hp_cols(ctx));
    if (!ensure_seq_caches(ctx, n_seqs)) return -2;
    if ((long)std::min(max_cols, total) >= MFMA_MIN_PASS_COLS && !ensure_tile_images(ctx)) return -2;
    if (!ensure_logits_rows(ctx, std::min(max_cols, total)) || !score_setup(ctx, seqs, lens, n_seqs, targets, total)) return -2;
    if (!pack_column_passes(ctx, seqs, lens, n_seqs, 1, [&](int n_cols, int t_max, size_t flat0) {
            return enqueue_forward(ctx, ForwardPass::packed_scored(n_cols, t_max)) && enqueue_logprob(ctx, n_cols, flat0, total);
        }))
        return -2;
    return score_finish(ctx, total, logprob_out, argmax_out, logit_out);
}

int biogpt_hip_score(biogpt_hip_ctx *ctx, const int32_t *tokens, int32_t n_tokens, int32_t n_past, const int32_t *targets,
                     float *logprob_out, int32_t *argmax_out, float *logit_out) {
    return with_xpipe_retry(ctx, n_past, [&] { return score_once(ctx, tokens, n_tokens, n_past, targets, logprob_out, argmax_out, logit_out); });
}
int biogpt_hip_score_batch(biogpt_hip_ctx *ctx, const int32_t *seqs, const int32_t *lens, int32_t n_seqs, const int32_t *targets,
                           float *logprob_out, int32_t *argmax_out, float *logit_out) {
    return with_xpipe_retry(ctx, 0, [&] { return score_batch_once(ctx, seqs, lens, n_seqs, targets, logprob_out, argmax_out, logit_out); });
}

// ---- continuations of shared prefixes: each prefix once, read in place by the columns of its continuations -----------------------------------
// Group g is a prefix and n_conts[g] continuations of it; biogpt_hip_score_continuations is one group, biogpt_hip_score_continuations_batch several.  The
// prefix rows [0, n_prefix_g - 1) go into slot g of the per-sequence caches as the prompt columns of generate_greedy_batch do (t_vis = position + 1, no
// lm_head: none of their logits are wanted).  Continuation f (flat index over all groups) owns slot n_groups + f; its columns are the LAST token of its
// group's prefix at position n_prefix_g - 1 (every continuation re-evaluates it, as the samples of generate_sample do: one target per row) and then its
// own tokens but the last.  A column's attention reads rows [0, n_prefix_g - 1) from slot g and the rest from its own slot (SeqState::pad[0] / pad[1];
// attn_fast_kernel<.., SHARED>): no K / V row is copied.  The columns travel in ONE stream of passes of up to BIOGPT_HIP_PROMPT_COLS columns: every prefix
// column of every group first, then every continuation column in the flat order of `conts` -- so pure prefix passes, at most one mixed pass, then scored
// passes, each a ForwardPass::packed_continuations.  A short call is one pass, and a continuation column may share a pass with the prefix columns it reads
// (the q/k/v launch of a layer has written every column's row before its attention launch starts, as for the columns of one sequence).  The continuation
// columns of a pass have their log-probabilities taken behind it (enqueue_logprob): their flat row is the flat index of their TARGET, `total` rows in all.
// The packer builds the column states, uploads them (flush_columns) and enqueues each pass.  The caller supplies its checked arguments and, if it wants
// attn_runs_kernel in some passes, runs_of(cols, t_max, runs): it fills `runs` with the pass's run table (attn_runs_plan) and returns the number of runs,
// or 0 for the existing attention; the table then goes up behind the column states in the same copy.  Without runs_of no pass has a table.
using RunsOf = std::function<int(const std::vector<bgk::SeqState> &, int, std::vector<int32_t> &)>;
static bool pack_continuation_passes(biogpt_hip_ctx *ctx, const int32_t *prefixes, const int32_t *prefix_lens, int n_groups, const int32_t *conts,
                                     const int32_t *cont_lens, const int32_t *n_conts, size_t total, const RunsOf &runs_of = nullptr) {
    const size_t max_cols = (size_t)std::min(std::max(1, ctx->opt.prompt_cols), hp_cols(ctx));
    std::vector<bgk::SeqState> cols;
    std::vector<int32_t> runs;
    int pass_tmax = 0, n_pre = 0;
    size_t flat0 = 0;
    auto flush = [&]() -> bool {
        if (cols.empty()) return true;
        const int pre = n_pre, n_runs = runs_of ? runs_of(cols, pass_tmax, runs) : 0;
        runs.resize(4 * (size_t)n_runs);
        size_t at = flat0;
        if (!flush_columns(ctx, cols, pass_tmax, at, [&](int n_cols, int t_max, size_t f) {
                ForwardPass fp = ForwardPass::packed_continuations(n_cols, t_max, pre);
                if (n_runs) { fp.runs = reinterpret_cast<const int32_t *>(ctx->cols + n_cols); fp.n_runs = n_runs; }
                return enqueue_forward(ctx, fp) && (pre == n_cols || enqueue_logprob(ctx, n_cols - pre, f, total));
            }, runs_of ? &runs : nullptr))
            return false;
        flat0 = at - (size_t)pre;      // prefix columns have no flat row
        n_pre = 0;
        return true;
    };
    size_t pre_off = 0;
    for (int g = 0; g < n_groups; g++) {
        for (int i = 0; i + 1 < prefix_lens[g]; i++) {
            if (cols.size() == max_cols && !flush()) return false;
            bgk::SeqState cst{};
            cst.n_past = i; cst.token = prefixes[pre_off + (size_t)i]; cst.seq_id = g; cst.t_vis = i + 1;      // pad[0] = 0: every row its own
            cols.push_back(cst);
            n_pre++;
            pass_tmax = std::max(pass_tmax, i + 1);
        }
        pre_off += (size_t)prefix_lens[g];
    }
    pre_off = 0;
    size_t off = 0;
    for (int g = 0, f = 0; g < n_groups; g++) {
        const int n_prefix = prefix_lens[g];
        for (int c = 0; c < n_conts[g]; c++, f++) {
            for (int i = 0; i < cont_lens[f]; i++) {
                if (cols.size() == max_cols && !flush()) return false;
                bgk::SeqState cst{};
                cst.n_past = n_prefix - 1 + i; cst.token = i == 0 ? prefixes[pre_off + (size_t)(n_prefix - 1)] : conts[off + (size_t)(i - 1)];
                cst.seq_id = n_groups + f; cst.t_vis = n_prefix + i;
                cst.pad[0] = n_prefix - 1; cst.pad[1] = g;      // rows [0, n_prefix - 1) lie in the group's prefix slot
                cols.push_back(cst);
                pass_tmax = std::max(pass_tmax, n_prefix + i);
            }
            off += (size_t)cont_lens[f];
        }
        pre_off += (size_t)n_prefix;
    }
    return flush();
}

static int score_continuations_once(biogpt_hip_ctx *ctx, const int32_t *prefix, int32_t n_prefix, const int32_t *conts, const int32_t *cont_lens,
                                    int32_t n_conts, float *logprob_out, int32_t *argmax_out, float *logit_out, double *seconds_out) {
    XpCallScope xp_scope(ctx);
    clear_error();
    if (!ctx) BG_FAIL(-1, "null context");
    if (!prefix) BG_FAIL(-1, "null argument: prefix");
    if (!conts) BG_FAIL(-1, "null argument: conts");
    if (!cont_lens) BG_FAIL(-1, "null argument: cont_lens");
    if (!logprob_out) BG_FAIL(-1, "null argument: logprob_out");
    if (!ctx->ready) BG_FAIL(-1, "model has no tensors loaded (empty model): cannot evaluate");
    if (session_refuses(ctx)) return -1;
    if (n_prefix < 1) BG_FAIL(-1, "n_prefix must be >= 1 (got %d)", n_prefix);
    if (n_conts < 1 || n_conts > 511) BG_FAIL(-1, "n_conts must be in [1, 511] (got %d)", n_conts);   // slot 0 is the prefix; each continuation owns a full F32 KV cache
    const auto &hp = ctx->hp;
    if (!check_fast_chain(ctx, "shared-prefix scoring", true)) return -1;
    if (n_prefix > hp.n_positions) BG_FAIL(-1, "n_prefix (%d) exceeds n_positions (%d)", n_prefix, hp.n_positions);
    for (int i = 0; i < n_prefix; i++)
        if (prefix[i] < 0 || prefix[i] >= hp.n_vocab) BG_FAIL(-1, "token id %d (prefix, position %d) out of range [0, %d)", prefix[i], i, hp.n_vocab);
    size_t total = 0;
    for (int c = 0; c < n_conts; c++) {
        const int len = cont_lens[c];
        if (len < 1) BG_FAIL(-1, "empty continuation (continuation %d)", c);
        if (len > hp.n_positions - n_prefix)
            BG_FAIL(-1, "n_prefix (%d) + cont_lens[%d] (%d) exceeds n_positions (%d)", n_prefix, c, len, hp.n_positions);
        for (int i = 0; i < len; i++) {
            const int32_t t = conts[total + (size_t)i];
            if (t < 0 || t >= hp.n_vocab) BG_FAIL(-1, "token id %d (continuation %d, position %d) out of range [0, %d)", t, c, i, hp.n_vocab);
        }
        total += (size_t)len;
    }
    HIP_TRY(-2, hipSetDevice(ctx->device));
    if (!resident_stop(ctx)) return -2; disarm_lineage(ctx);
    // the prefix and every continuation in the per-sequence caches (bk / bv): the context's own cache, position and logits row stay as they are
    const size_t max_cols = (size_t)std::min(std::max(1, ctx->opt.prompt_cols), hp_cols(ctx));
    const int n_shared = n_prefix - 1;
    if (!ensure_seq_caches(ctx, n_conts + 1)) {
        (void)hipGetLastError();
        BG_FAIL(-2, "out of device memory: the %zu-byte K / V caches of %d continuations and their prefix could not be allocated",
                (size_t)2 * 4 * hp.n_layer * hp.n_positions * hp.d_model * (size_t)(n_conts + 1), n_conts);
    }
    if ((long)std::min(max_cols, total + (size_t)n_shared) >= MFMA_MIN_PASS_COLS && !ensure_tile_images(ctx)) return -2;
    if (!ensure_logits_rows(ctx, std::min(max_cols, total)) || !score_setup(ctx, conts, cont_lens, n_conts, conts, total)) return -2;
    HIP_TRY(-2, hipStreamSynchronize(ctx->stream));
    const auto t0 = std::chrono::steady_clock::now();
    if (!pack_continuation_passes(ctx, prefix, &n_prefix, 1, conts, cont_lens, &n_conts, total)) return -2;      // one group; never attn_runs_kernel
    const int rc = score_finish(ctx, total, logprob_out, argmax_out, logit_out);
    if (rc == 0 && seconds_out) *seconds_out = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return rc;
}

int biogpt_hip_score_continuations(biogpt_hip_ctx *ctx, const int32_t *prefix, int32_t n_prefix, const int32_t *conts, const int32_t *cont_lens,
                                   int32_t n_conts, float *logprob_out, int32_t *argmax_out, float *logit_out, double *seconds_out) {
    return with_xpipe_retry(ctx, 0, [&] {
        return score_continuations_once(ctx, prefix, n_prefix, conts, cont_lens, n_conts, logprob_out, argmax_out, logit_out, seconds_out);
    });
}

// ---- several (prefix, continuations) groups in one call ----------------------------------------------------------------------------------------
// Group g is score_continuations(prefix_g, conts_g): the columns and passes are pack_continuation_passes' for n_groups groups.  What this call adds per pass
// is its attention: attn_fast_kernel<.., SHARED> as in the single call, or attn_runs_kernel over the runs of attn_runs_plan (BIOGPT_HIP_RUN_ATTN;
// run_attn_table decides, the packer sends the table up behind the column states).
// attn_runs_kernel instead of attn_fast_kernel<.., SHARED> in a pass of this call (BIOGPT_HIP_RUN_ATTN=-1): a pass of RUN_ATTN_MIN_COLS columns or more whose longest
// shared range (the largest R of its runs) has RUN_ATTN_MIN_SHARED rows or more, and every pass of RUN_ATTN_ANY_SHARED_COLS columns or more.
// (2026-10-20, tools/prefix_batch_bench.py --ab: the call, 24 layers, the kernel never / always taken, runs / existing.  Passes of 512 columns: 0.63 - 0.64 x behind
// 384-token prefixes (16 / 64 / 128 groups of three one-token candidates, 8 groups of 32 x 8, one group of 64 x 8), 0.96 x behind 64-token prefixes (64 groups; ranges of
// at most 63 rows).  One pass of 386 columns (one example behind 384 tokens, longest range 383): 0.70 x.  One pass of 66 columns (behind 64 tokens): 1.04 x, of 18
// columns: 1.08 x -- it loses there.  Single passes in between: 258 columns behind 256 tokens (longest range 255) 0.97 x, 396 columns of 6 groups behind 64 tokens
// (ranges of at most 63 rows) 0.94 x; 130 columns behind 128 tokens 1.02 x and 132 columns of 2 groups behind 64 tokens 1.06 x lose.  The thresholds are the smallest
// measured wins.  Not measured: 133 .. 257 columns; 258 .. 395 columns with ranges shorter than 255 rows; other quantizations than Q4_0.  DESIGN.md 4.7 has the tables.)
constexpr int RUN_ATTN_MIN_COLS = 258, RUN_ATTN_MIN_SHARED = 255, RUN_ATTN_ANY_SHARED_COLS = 396;
constexpr int PFXB_MAX_SLOTS = 512;     // each slot is a full F32 KV cache
// the run table of a pass of `cols` with t_max visible keys -> runs; the number of runs, 0: the pass keeps the existing attention
static int run_attn_table(const biogpt_hip_ctx *ctx, const std::vector<bgk::SeqState> &cols, int t_max, std::vector<int32_t> &runs) {
    const int n = (int)cols.size();
    const int t_cap = attn_decode_t_cap(ctx->hp.n_positions, t_max);
    int n_runs = 0;
    if (t_cap <= bgk::RUNS_MAX_KEYS && ctx->opt.run_attn != 0 && (ctx->opt.run_attn == 1 || n >= RUN_ATTN_MIN_COLS)) {
        runs.resize(4 * (size_t)n);
        n_runs = attn_runs_plan(cols.data(), n, runs.data());
        int longest = 0;
        for (int r = 0; r < n_runs; r++) longest = std::max(longest, runs[4 * (size_t)r + 2]);
        if (ctx->opt.run_attn < 0 && n < RUN_ATTN_ANY_SHARED_COLS && longest < RUN_ATTN_MIN_SHARED) n_runs = 0;      // the existing attention
    }
    return n_runs;
}

static int score_continuations_batch_once(biogpt_hip_ctx *ctx, const int32_t *prefixes, const int32_t *prefix_lens, int32_t n_groups, const int32_t *conts,
                                          const int32_t *cont_lens, const int32_t *n_conts, float *logprob_out, int32_t *argmax_out, float *logit_out,
                                          double *seconds_out) {
    XpCallScope xp_scope(ctx);
    clear_error();
    if (!ctx) BG_FAIL(-1, "null context");
    if (!prefixes) BG_FAIL(-1, "null argument: prefixes");
    if (!prefix_lens) BG_FAIL(-1, "null argument: prefix_lens");
    if (!conts) BG_FAIL(-1, "null argument: conts");
    if (!cont_lens) BG_FAIL(-1, "null argument: cont_lens");
    if (!n_conts) BG_FAIL(-1, "null argument: n_conts");
    if (!logprob_out) BG_FAIL(-1, "null argument: logprob_out");
    if (!ctx->ready) BG_FAIL(-1, "model has no tensors loaded (empty model): cannot evaluate");
    if (session_refuses(ctx)) return -1;
    if (n_groups < 1) BG_FAIL(-1, "n_groups must be >= 1 (got %d)", n_groups);
    long slots = n_groups;
    for (int g = 0; g < n_groups; g++) {
        if (n_conts[g] < 1) BG_FAIL(-1, "n_conts[%d] must be >= 1 (got %d)", g, n_conts[g]);
        slots += n_conts[g];
    }
    if (slots > PFXB_MAX_SLOTS)
        BG_FAIL(-1, "%ld slots exceed the %d of one call: n_groups (%d) + the sum of n_conts (%ld), one slot per prefix and one per continuation", slots, PFXB_MAX_SLOTS, n_groups, slots - n_groups);
    const auto &hp = ctx->hp;
    if (!check_fast_chain(ctx, "shared-prefix scoring of many prompts")) return -1;
    size_t total = 0, pre_off = 0, pre_cols = 0;
    int cont_at = 0;
    for (int g = 0; g < n_groups; g++) {
        const int n_prefix = prefix_lens[g];
        if (n_prefix < 1) BG_FAIL(-1, "prefix_lens[%d] (n_prefix of group %d) must be >= 1 (got %d)", g, g, n_prefix);
        if (n_prefix > hp.n_positions) BG_FAIL(-1, "prefix_lens[%d] (n_prefix %d of group %d) exceeds n_positions (%d)", g, n_prefix, g, hp.n_positions);
        for (int i = 0; i < n_prefix; i++) {
            const int32_t t = prefixes[pre_off + (size_t)i];
            if (t < 0 || t >= hp.n_vocab) BG_FAIL(-1, "token id %d (group %d, prefix, position %d) out of range [0, %d)", t, g, i, hp.n_vocab);
        }
        for (int c = 0; c < n_conts[g]; c++, cont_at++) {
            const int len = cont_lens[cont_at];
            if (len < 1) BG_FAIL(-1, "empty continuation (group %d, continuation %d: cont_lens[%d])", g, c, cont_at);
            if (len > hp.n_positions - n_prefix)
                BG_FAIL(-1, "n_prefix (%d) + cont_lens[%d] (%d) of group %d, continuation %d exceeds n_positions (%d)", n_prefix, cont_at, len, g, c, hp.n_positions);
            for (int i = 0; i < len; i++) {
                const int32_t t = conts[total + (size_t)i];
                if (t < 0 || t >= hp.n_vocab) BG_FAIL(-1, "token id %d (group %d, continuation %d, position %d) out of range [0, %d)", t, g, c, i, hp.n_vocab);
            }
            total += (size_t)len;
        }
        pre_off += (size_t)n_prefix;
        pre_cols += (size_t)(n_prefix - 1);
    }
    const int n_all = cont_at;
    HIP_TRY(-2, hipSetDevice(ctx->device));
    if (!resident_stop(ctx)) return -2; disarm_lineage(ctx);
    // every prefix and every continuation in the per-sequence caches (bk / bv): the context's own cache, position and logits row stay as they are
    const size_t max_cols = (size_t)std::min(std::max(1, ctx->opt.prompt_cols), hp_cols(ctx));
    if (!ensure_seq_caches(ctx, (int)slots)) {
        (void)hipGetLastError();
        BG_FAIL(-2, "out of device memory: the %zu-byte K / V caches of %d prefixes and %d continuations could not be allocated",
                (size_t)2 * 4 * hp.n_layer * hp.n_positions * hp.d_model * (size_t)slots, n_groups, n_all);
    }
    if ((long)std::min(max_cols, total + pre_cols) >= MFMA_MIN_PASS_COLS && !ensure_tile_images(ctx)) return -2;
    if (!ensure_logits_rows(ctx, std::min(max_cols, total)) || !score_setup(ctx, conts, cont_lens, n_all, conts, total)) return -2;
    HIP_TRY(-2, hipStreamSynchronize(ctx->stream));
    const auto t0 = std::chrono::steady_clock::now();

    int n_passes = 0, n_run_passes = 0;
    if (!pack_continuation_passes(ctx, prefixes, prefix_lens, n_groups, conts, cont_lens, n_conts, total,
                                  [&](const std::vector<bgk::SeqState> &cols, int t_max, std::vector<int32_t> &runs) {
                                      const int n_runs = run_attn_table(ctx, cols, t_max, runs);
                                      n_passes++; n_run_passes += n_runs ? 1 : 0;
                                      return n_runs;
                                  }))
        return -2;
    const int rc = score_finish(ctx, total, logprob_out, argmax_out, logit_out);
    if (rc != 0) return rc;
    if (seconds_out) *seconds_out = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    const int32_t stats[4] = {(int32_t)pre_cols, (int32_t)total, n_passes, n_run_passes};
    std::memcpy(ctx->pfxb_stats, stats, sizeof(stats));
    return 0;
}

int biogpt_hip_score_continuations_batch(biogpt_hip_ctx *ctx, const int32_t *prefixes, const int32_t *prefix_lens, int32_t n_groups, const int32_t *conts,
                                         const int32_t *cont_lens, const int32_t *n_conts, float *logprob_out, int32_t *argmax_out, float *logit_out,
                                         double *seconds_out) {
    return with_xpipe_retry(ctx, 0, [&] {
        return score_continuations_batch_once(ctx, prefixes, prefix_lens, n_groups, conts, cont_lens, n_conts, logprob_out, argmax_out, logit_out, seconds_out);
    });
}
int biogpt_hip_prefix_batch_stats(const biogpt_hip_ctx *ctx, int32_t out[4]) {
    clear_error();
    if (!ctx) BG_FAIL(-1, "null context");
    if (!out) BG_FAIL(-1, "null argument: out");
    std::memcpy(out, ctx->pfxb_stats, sizeof(ctx->pfxb_stats));
    return 0;
}
int biogpt_hip_attn_runs_plan(const int32_t *seq_states, int32_t N, int32_t *runs_out) {
    clear_error();
    if (!seq_states || !runs_out) BG_FAIL(-1, "seq_states or runs_out is NULL");
    if (N < 1 || N > 1024) BG_FAIL(-1, "N must be in [1, 1024]");
    return attn_runs_plan(reinterpret_cast<const bgk::SeqState *>(seq_states), N, runs_out);
}

// ---- hidden states, pooled embeddings, classification heads: the same causal passes without the lm_head (kernels_embed.hip.h) ------------
// The passes are those of scoring (one column per token, row i sees keys [0, position of i]); their final stage is Rows::Hidden: the final
// LayerNorm of every column as f32 rows -- or, for a layer index k < n_layer, the residual stream after k layers as it lies in c->x.  Pooling
// and the caller's linear head run on the device per pass; the call's rows come back in one copy.
struct EmbedPlan {      // byte offsets into emb_buf (each a multiple of 16)
    size_t out = 0, pooled = 0, acc = 0, hid = 0, w = 0, b = 0, lens = 0, bytes = 0;
};
static bool ensure_embed_buf(biogpt_hip_ctx *c, size_t bytes) {
    if (bytes <= c->emb_cap) return true;
    if (c->emb_buf) (void)hipFree(c->emb_buf);
    c->emb_buf = nullptr; c->emb_cap = 0;
    if (hipMalloc(&c->emb_buf, bytes) != hipSuccess) {
        (void)hipGetLastError();
        c->emb_buf = nullptr;
        BG_FAIL(false, "out of device memory: the %zu-byte buffer of this call's output rows could not be allocated", bytes);
    }
    c->emb_cap = bytes;
    return true;
}

// the argument errors of biogpt_hip_embed_batch that need no model: before the context is looked at, before any HIP call
static bool check_embed_args(const int32_t *seqs, const int32_t *lens, int32_t n_seqs, const biogpt_hip_embed_opts &o, const float *out) {
    if (!seqs || !lens || !out) BG_FAIL(false, "null argument (seqs, lens and out must be given)");
    if (n_seqs < 1 || n_seqs > 512) BG_FAIL(false, "n_seqs must be in [1, 512]");   // each sequence owns a full F32 KV cache
    if (o.layer < -1) BG_FAIL(false, "layer (%d) must be in [-1, n_layer]", o.layer);
    if (o.pooling < 0 || o.pooling > 2) BG_FAIL(false, "unknown pooling (%d): 0 none, 1 last token, 2 mean", o.pooling);
    if (o.normalize != 0 && o.normalize != 1) BG_FAIL(false, "normalize (%d) must be 0 or 1", o.normalize);
    if (o.n_out < 0 || o.n_out > 256) BG_FAIL(false, "n_out (%d) must be in [0, 256]", o.n_out);
    if (o.n_out > 0 && !o.w) BG_FAIL(false, "w is NULL with n_out = %d", o.n_out);
    if (o.n_out == 0 && o.w) BG_FAIL(false, "w given with n_out = 0");
    if (o.n_out == 0 && o.b) BG_FAIL(false, "b given with n_out = 0");
    if (o.normalize && o.n_out > 0) BG_FAIL(false, "normalize cannot be combined with a head (n_out = %d)", o.n_out);
    for (int i = 0; o.b && i < o.n_out; i++)
        if (!std::isfinite(o.b[i])) BG_FAIL(false, "b[%d] is not finite", i);
    size_t off = 0;
    for (int s = 0; s < n_seqs; s++) {
        if (lens[s] < 1) BG_FAIL(false, "empty sequence (sequence %d)", s);
        for (int i = 0; i < lens[s]; i++)
            if (seqs[off + i] < 0) BG_FAIL(false, "token id %d out of range (sequence %d, token %d)", seqs[off + i], s, i);
        off += (size_t)lens[s];
    }
    return true;
}
// w [n_out][d_model] holds finite values only (its extent needs the model's width: after the model checks, still before any HIP call)
static bool check_head_values(const biogpt_hip_embed_opts &o, int D) {
    for (size_t i = 0; i < (size_t)o.n_out * D; i++)
        if (!std::isfinite(o.w[i])) BG_FAIL(false, "w[%zu][%zu] is not finite", i / D, i % D);
    return true;
}

static bool enqueue_head(biogpt_hip_ctx *c, const float *rows, int n_rows, const float *w, const float *b, int n_out, float *out) {
    HIP_TRY(false, launch_head_rows(c->stream, rows, n_rows, c->hp.d_model, w, b, n_out, out));
    return true;
}

static int hidden_once(biogpt_hip_ctx *ctx, const int32_t *tokens, int32_t n, int32_t n_past, float *hidden_out) {
    XpCallScope xp_scope(ctx);
    clear_error();
    if (!hidden_out) BG_FAIL(-1, "null hidden_out buffer");
    if (!check_eval_args(ctx, tokens, n, n_past)) return -1;
    HIP_TRY(-2, hipSetDevice(ctx->device));
    if (!resident_stop(ctx)) return -2; disarm_lineage(ctx);
    const size_t D = (size_t)ctx->hp.d_model;
    const int max_cols = causal_pass_cols(ctx, n);      // the passes of biogpt_hip_score
    if (!max_cols) return -2;
    if (!ensure_embed_buf(ctx, (size_t)n * D * 4)) return -2;
    float *const out = reinterpret_cast<float *>(ctx->emb_buf);
    if (!causal_passes(ctx, tokens, n, n_past, max_cols, [&](int at, int m) {
            return enqueue_forward(ctx, ForwardPass::hidden(m, n_past + at + m, HiddenStage{ctx->hp.n_layer, out + (size_t)at * D}));
        }))
        return -2;
    HIP_TRY(-2, hipMemcpyAsync(hidden_out, out, (size_t)n * D * 4, hipMemcpyDeviceToHost, ctx->stream));
    return wait_stream(ctx) ? 0 : -2;
}

static int embed_batch_once(biogpt_hip_ctx *ctx, const int32_t *seqs, const int32_t *lens, int32_t n_seqs, const biogpt_hip_embed_opts *opts,
                            float *out_host, double *seconds_out) {
    XpCallScope xp_scope(ctx);
    clear_error();
    biogpt_hip_embed_opts o{-1, 1, 0, 0, nullptr, nullptr};
    if (opts) o = *opts;
    if (!check_embed_args(seqs, lens, n_seqs, o, out_host)) return -1;
    if (!ctx) BG_FAIL(-1, "null context");
    if (!ctx->ready) BG_FAIL(-1, "model has no tensors loaded (empty model): cannot evaluate");
    if (session_refuses(ctx)) return -1;
    const auto &hp = ctx->hp;
    if (o.n_out > 0 && !check_head_width(hp.d_model)) return -1;      // (the wide and the float gates admit any d_model of 64 n_head)
    if (!check_fast_chain(ctx, "batched embedding", true)) return -1;
    if (o.layer > hp.n_layer) BG_FAIL(-1, "layer (%d) must be in [-1, n_layer = %d]", o.layer, hp.n_layer);
    size_t total = 0;
    for (int s = 0; s < n_seqs; s++) {
        if (!check_eval_args(ctx, seqs + total, lens[s], 0)) return -1;
        total += (size_t)lens[s];
    }
    if (o.n_out > 0 && !check_head_values(o, hp.d_model)) return -1;
    const int k = o.layer < 0 ? hp.n_layer : o.layer;
    const size_t D = (size_t)hp.d_model, W = o.n_out > 0 ? (size_t)o.n_out : D;
    const size_t n_rows = o.pooling != bgk::POOL_NONE ? (size_t)n_seqs : total;
    HIP_TRY(-2, hipSetDevice(ctx->device));
    if (!resident_stop(ctx)) return -2; disarm_lineage(ctx);
    // every sequence from position 0 in its own K / V cache (bk / bv): the context's own cache, position and logits row stay as they are
    const size_t max_cols = (size_t)std::min(std::max(1, ctx->opt.prompt_cols), hp_cols(ctx));
    if (!ensure_seq_caches(ctx, n_seqs)) return -2;
    if ((long)std::min(max_cols, total) >= MFMA_MIN_PASS_COLS && !ensure_tile_images(ctx)) return -2;
    const bool direct = o.pooling == bgk::POOL_NONE && o.n_out == 0;      // the rows of a pass are output rows as they are
    EmbedPlan pl;
    auto take = [&](size_t bytes) { const size_t at = pl.bytes; pl.bytes += (bytes + 15) & ~(size_t)15; return at; };
    pl.out = take(n_rows * W * 4);
    if (o.pooling != bgk::POOL_NONE && o.n_out > 0) pl.pooled = take((size_t)n_seqs * D * 4);
    if (o.pooling == bgk::POOL_MEAN) pl.acc = take((size_t)n_seqs * D * 8);
    if (!direct && k == hp.n_layer) pl.hid = take(std::min(max_cols, total) * D * 4);
    if (o.n_out > 0) { pl.w = take((size_t)o.n_out * D * 4); pl.b = take((size_t)o.n_out * 4); }
    pl.lens = take((size_t)n_seqs * 4);
    if (!ensure_embed_buf(ctx, pl.bytes)) return -2;
    uint8_t *const base = ctx->emb_buf;
    float *const d_out = reinterpret_cast<float *>(base + pl.out);
    float *const d_pool = o.pooling == bgk::POOL_NONE ? nullptr : (o.n_out > 0 ? reinterpret_cast<float *>(base + pl.pooled) : d_out);
    double *const d_acc = o.pooling == bgk::POOL_MEAN ? reinterpret_cast<double *>(base + pl.acc) : nullptr;
    float *const d_hid = reinterpret_cast<float *>(base + pl.hid);
    const float *const d_w = reinterpret_cast<const float *>(base + pl.w);
    const float *const d_b = o.b ? reinterpret_cast<const float *>(base + pl.b) : nullptr;
    const int32_t *const d_lens = reinterpret_cast<const int32_t *>(base + pl.lens);
    hipStream_t st = ctx->stream;
    // the call's inputs go up once (blocking copies: the host arrays are the caller's)
    HIP_TRY(-2, hipMemcpy(base + pl.lens, lens, (size_t)n_seqs * 4, hipMemcpyHostToDevice));
    if (o.n_out > 0) {
        HIP_TRY(-2, hipMemcpy(base + pl.w, o.w, (size_t)o.n_out * D * 4, hipMemcpyHostToDevice));
        if (o.b) HIP_TRY(-2, hipMemcpy(base + pl.b, o.b, (size_t)o.n_out * 4, hipMemcpyHostToDevice));
    }
    HIP_TRY(-2, hipStreamSynchronize(st));
    const auto t0 = std::chrono::steady_clock::now();
    if (d_acc) HIP_TRY(-2, hipMemsetAsync(d_acc, 0, (size_t)n_seqs * D * 8, st));
    if (!pack_column_passes(ctx, seqs, lens, n_seqs, 1, [&](int n_cols, int t_max, size_t flat0) {
            const HiddenStage hs{k, k < hp.n_layer ? nullptr : (direct ? d_out + flat0 * D : d_hid)};
            if (!enqueue_forward(ctx, ForwardPass::packed_hidden(n_cols, t_max, hs))) return false;
            const float *rows = hs.ln_out ? hs.ln_out : ctx->x;
            if (o.pooling == bgk::POOL_NONE) {
                if (o.n_out > 0) return enqueue_head(ctx, rows, n_cols, d_w, d_b, o.n_out, d_out + flat0 * W);
                if (!hs.ln_out) HIP_TRY(false, hipMemcpyAsync(d_out + flat0 * D, ctx->x, (size_t)n_cols * D * 4, hipMemcpyDeviceToDevice, st));
                return true;
            }
            HIP_TRY(false, launch_pool_rows(st, rows, n_cols, (int)D, ctx->cols, d_lens, o.pooling, d_pool, d_acc));
            return true;
        }))
        return -2;
    if (pool_needs_finish(d_acc, o.normalize))      // the mean of every accumulator row; the L2 normalisation of every output row
        HIP_TRY(-2, launch_pool_finish(st, d_pool ? d_pool : d_out, (int)n_rows, (int)D, d_acc, d_lens, o.normalize));
    if (d_pool && o.n_out > 0 && !enqueue_head(ctx, d_pool, n_seqs, d_w, d_b, o.n_out, d_out)) return -2;
    HIP_TRY(-2, hipMemcpyAsync(out_host, d_out, n_rows * W * 4, hipMemcpyDeviceToHost, st));
    if (!wait_stream(ctx)) return -2;
    const auto t1 = std::chrono::steady_clock::now();
    if (seconds_out) *seconds_out = std::chrono::duration<double>(t1 - t0).count();
    return 0;
}

int biogpt_hip_hidden(biogpt_hip_ctx *ctx, const int32_t *tokens, int32_t n_tokens, int32_t n_past, float *hidden_out) {
    return with_xpipe_retry(ctx, n_past, [&] { return hidden_once(ctx, tokens, n_tokens, n_past, hidden_out); });
}
int biogpt_hip_embed_batch(biogpt_hip_ctx *ctx, const int32_t *seqs, const int32_t *lens, int32_t n_seqs, const biogpt_hip_embed_opts *opts,
                           float *out, double *seconds_out) {
    return with_xpipe_retry(ctx, 0, [&] { return embed_batch_once(ctx, seqs, lens, n_seqs, opts, out, seconds_out); });
}

// ---- generation rules: transformers' logits processors on the device, between the forward pass and the selection (kernels_rules.hip.h) --------
// One check for the three entry points, before any HIP call.  n_positions < 0: no model (the kernel-alone entry).
constexpr int RULES_ROWS = 512;     // rows of a call: sequences of biogpt_hip_generate_sample (beams: BEAM_MAX)

static bool check_rules(const biogpt_hip_gen_rules *r, int n_vocab, int n_positions) {
    if (!r) return true;
    if (!std::isfinite(r->repetition_penalty) || !(r->repetition_penalty > 0.0f)) BG_FAIL(false, "repetition_penalty must be finite and > 0 (1.0: off)");
    if (r->no_repeat_ngram_size < 0) BG_FAIL(false, "no_repeat_ngram_size must be >= 0 (0: off)");
    if (n_positions >= 0 && r->no_repeat_ngram_size > n_positions)
        BG_FAIL(false, "no_repeat_ngram_size %d exceeds the model's %d positions", r->no_repeat_ngram_size, n_positions);
    if (r->min_new_tokens < 0) BG_FAIL(false, "min_new_tokens must be >= 0 (0: off)");
    if (r->n_suppress < 0 || r->n_suppress > bgk::RULES_MAX_SUPPRESS) BG_FAIL(false, "n_suppress must be in [0, %d]", bgk::RULES_MAX_SUPPRESS);
    if (r->n_suppress > 0 && !r->suppress) BG_FAIL(false, "suppress is NULL with n_suppress = %d", r->n_suppress);
    for (int i = 0; i < r->n_suppress; i++)
        if (r->suppress[i] < 0 || r->suppress[i] >= n_vocab) BG_FAIL(false, "suppress[%d] = %d out of range: must be in [0, %d)", i, r->suppress[i], n_vocab);
    if (n_vocab > bgk::RULES_MAX_VOCAB) BG_FAIL(false, "generation rules hold one bit per token in LDS: n_vocab must be at most %d", bgk::RULES_MAX_VOCAB);
    return true;
}

// a rule that writes -inf is active (min_new_tokens only with an EOS id, as transformers adds its processor)
static bool rules_ban(const biogpt_hip_gen_rules *r, int eos_id) {
    return r && (r->no_repeat_ngram_size > 0 || (r->min_new_tokens > 0 && eos_id >= 0) || r->n_suppress > 0);
}
static bool rules_active(const biogpt_hip_gen_rules *r, int eos_id) { return r && (r->repetition_penalty != 1.0f || rules_ban(r, eos_id)); }

static bgk::RulesCtl rules_ctl_of(const biogpt_hip_gen_rules *r, int mode, int eos_id) {
    bgk::RulesCtl h{};
    h.penalty = r->repetition_penalty; h.ngram = r->no_repeat_ngram_size; h.min_new = eos_id >= 0 ? r->min_new_tokens : 0;
    h.n_suppress = r->n_suppress; h.eos_id = eos_id; h.mode = mode;
    for (int i = 0; i < r->n_suppress; i++) h.suppress[i] = r->suppress[i];
    return h;
}

// The rules buffer: allocated once, at its largest (RULES_ROWS prompts of n_positions tokens), so that captured steps keep their pointers
struct RulesBufs {
    bgk::RulesCtl *ctl;
    bgk::RulesRow *rows;    // [RULES_ROWS]
    int32_t *toks;          // the call's prompts, one copy per prompt
    size_t bytes;
};
static RulesBufs rules_bufs_at(uint8_t *base, size_t n_toks) {
    ByteLayout l;
    RulesBufs b{};
    b.ctl = l.take<bgk::RulesCtl>(base, 1); b.rows = l.take<bgk::RulesRow>(base, RULES_ROWS); b.toks = l.take<int32_t>(base, n_toks);
    b.bytes = l.bytes();
    return b;
}

// the call's rules, its rows (row p * rows_per_prompt + j reads prompt p) and its prompts -> the device, once per call
static bool rules_upload(biogpt_hip_ctx *c, const biogpt_hip_gen_rules *r, int mode, int eos_id, const int32_t *prompts, const int32_t *prompt_lens,
                         int n_prompts, int rows_per_prompt) {
    if (!c->rules_buf) HIP_TRY(false, hipMalloc(&c->rules_buf, rules_bufs_at(nullptr, (size_t)RULES_ROWS * c->hp.n_positions).bytes));
    size_t total = 0;
    for (int p = 0; p < n_prompts; p++) total += (size_t)prompt_lens[p];
    std::vector<uint8_t> h(rules_bufs_at(nullptr, total).bytes, 0);
    const RulesBufs hb = rules_bufs_at(h.data(), total);
    *hb.ctl = rules_ctl_of(r, mode, eos_id);
    size_t o = 0;
    for (int p = 0; p < n_prompts; p++) {
        for (int j = 0; j < rows_per_prompt; j++) hb.rows[(size_t)p * rows_per_prompt + j] = bgk::RulesRow{(int32_t)o, prompt_lens[p]};
        o += (size_t)prompt_lens[p];
    }
    std::memcpy(hb.toks, prompts, total * 4);
    HIP_TRY(false, hipMemcpy(c->rules_buf, h.data(), h.size(), hipMemcpyHostToDevice));
    return true;
}

// skip: a device word per row (skip_stride words apart) that, set, leaves the row alone
static bool enqueue_rules(biogpt_hip_ctx *c, int n_rows, const int32_t *skip, int skip_stride) {
    const int V = c->hp.n_vocab;
    const RulesBufs b = rules_bufs_at(c->rules_buf, 0);
    hipLaunchKernelGGL(bgk::rules_rows_kernel, dim3(n_rows), dim3(bgk::LP_THREADS), (size_t)((V + 31) / 32) * 4, c->stream, c->logits_all, V, V, b.ctl, b.rows, b.toks, c->seq,
                       c->seq_gen, c->hp.n_positions, skip, skip_stride);
    HIP_TRY(false, hipGetLastError());
    return true;
}

// ---- trie-constrained generation: PrefixConstrainedLogitsProcessor over a closed set of sequences, between the forward pass and the selection (kernels_trie.hip.h) ----
// What can be judged without a model, before any HIP call: the two generation entries and the kernel-alone entry
static bool check_trie(const biogpt_hip_trie *trie, int eos_id) {
    if (!trie) BG_FAIL(false, "trie is NULL (the functions without a trie generate unconstrained)");
    if (eos_id < 0) BG_FAIL(false, "eos_id must be >= 0 with a trie: EOS is how an entry ends");
    if (eos_id >= trie->n_vocab) BG_FAIL(false, "eos_id %d out of range: must be in [0, %d)", eos_id, trie->n_vocab);
    if (trie->uses(eos_id)) BG_FAIL(false, "eos_id %d occurs in an entry of the trie", eos_id);
    if (trie->n_vocab > bgk::RULES_MAX_VOCAB) BG_FAIL(false, "a trie step holds one bit per token in LDS: n_vocab must be at most %d", bgk::RULES_MAX_VOCAB);
    return true;
}
static bool check_trie_vocab(const biogpt_hip_trie *trie, int n_vocab) {
    if (trie->n_vocab != n_vocab) BG_FAIL(false, "trie: built for n_vocab = %d, the model has %d", trie->n_vocab, n_vocab);
    return true;
}

// The trie's arrays on `device` -- [first | tok | child | term] in one block, uploaded at the first use there and freed with the handle -- as a TrieCtl
static bool trie_device(biogpt_hip_trie *trie, int device, bgk::TrieCtl *out) {
    ByteLayout l;
    const size_t o_f = l.part(trie->first.size() * 4), o_t = l.part(trie->tok.size() * 4), o_c = l.part(trie->child.size() * 4), o_m = l.part(trie->term.size());
    uint8_t *block = nullptr;
    for (const auto &c : trie->copies) if (c.device == device) block = static_cast<uint8_t *>(c.block);
    if (!block) {
        std::vector<uint8_t> h(l.bytes(), 0);
        std::memcpy(h.data() + o_f, trie->first.data(), trie->first.size() * 4);
        std::memcpy(h.data() + o_t, trie->tok.data(), trie->tok.size() * 4);
        std::memcpy(h.data() + o_c, trie->child.data(), trie->child.size() * 4);
        std::memcpy(h.data() + o_m, trie->term.data(), trie->term.size());
        HIP_TRY(false, hipMalloc(&block, h.size()));
        if (hipMemcpy(block, h.data(), h.size(), hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipFree(block);
            BG_FAIL(false, "the trie's upload failed: %s", hipGetErrorString(hipGetLastError()));
        }
        trie->copies.push_back({device, block});
        trie->free_copy = [](int, void *b) { (void)hipFree(b); };
    }
    *out = bgk::TrieCtl{};
    out->first = reinterpret_cast<const int32_t *>(block + o_f); out->tok = reinterpret_cast<const int32_t *>(block + o_t);
    out->child = reinterpret_cast<const int32_t *>(block + o_c); out->term = block + o_m;
    out->n_nodes = (int32_t)trie->n_nodes();
    return true;
}

// the call's trie, EOS id and mode -> the context's TrieCtl, once per call
static bool trie_upload(biogpt_hip_ctx *c, biogpt_hip_trie *trie, int mode, int eos_id) {
    bgk::TrieCtl h;
    if (!trie_device(trie, c->device, &h)) return false;
    h.eos_id = eos_id; h.mode = mode;
    if (!c->trie_ctl) HIP_TRY(false, hipMalloc(&c->trie_ctl, sizeof(bgk::TrieCtl)));
    HIP_TRY(false, hipMemcpy(c->trie_ctl, &h, sizeof(h), hipMemcpyHostToDevice));
    return true;
}

// skip: as enqueue_rules
static bool enqueue_trie(biogpt_hip_ctx *c, int n_rows, const int32_t *skip, int skip_stride) {
    const int V = c->hp.n_vocab;
    hipLaunchKernelGGL(bgk::trie_rows_kernel, dim3(n_rows), dim3(bgk::LP_THREADS), (size_t)((V + 31) / 32) * 4, c->stream, c->logits_all, V, V, c->trie_ctl, c->seq, c->seq_gen,
                       c->hp.n_positions, skip, skip_stride);
    HIP_TRY(false, hipGetLastError());
    return true;
}

// ---- sampled generation: n_prompts x n_samples columns of the batched decode step + the reference's sampler on the device (kernels_sample.hip.h) ----
// The column generation above with sample_rows_kernel as the selection.  A prompt with several samples is evaluated once, into the slot of its first
// sample.  With an EOS id the steps stop once every sequence has finished (SampleCtl::n_live).  The context's own K / V cache, position and logits row
// are left alone.
struct SampleBufs {
    bgk::SampleCtl *ctl;
    bgk::SampleSeq *seq;    // [n_seqs]
    bgk::SampleWide *wide;  // the sampler of a wide call (kernels_wide_sample.hip.h), behind everything the plain step knows
    size_t bytes;
};
static SampleBufs sample_bufs_at(uint8_t *base, size_t n_seqs) {
    ByteLayout l;
    SampleBufs b{};
    b.ctl = l.take<bgk::SampleCtl>(base, 1); b.seq = l.take<bgk::SampleSeq>(base, n_seqs); b.wide = l.take<bgk::SampleWide>(base, 1);
    b.bytes = l.bytes();
    return b;
}
// the parameters of a call as it starts: all n_seqs sequences run
static bgk::SampleCtl sample_ctl_of(int top_k, int eos_id, int n_seqs, double top_p, double temp) {
    bgk::SampleCtl hc{};
    hc.top_k = top_k; hc.eos_id = eos_id; hc.n_live = n_seqs; hc.top_p = top_p; hc.temp = temp;
    return hc;
}

// temp and top_p of any sampler; `who` begins the message: "", "sampler: " or "params[3]."
static bool check_temp_top_p(double temp, double top_p, const char *who = "") {
    if (!std::isfinite(temp) || !(temp > 0.0)) BG_FAIL(false, "%stemp must be finite and > 0", who);
    if (!std::isfinite(top_p)) BG_FAIL(false, "%stop_p must be finite (>= 1: no cut)", who);
    return true;
}
// The values of sample_rows_kernel's sampler and an EOS id (-1: none), for rows of V entries; V < 0: the width is not known yet, and the check with it follows.
// A message names the values with `pre` in front, a format of r: "" or "params[%d]."
static bool check_sample_values(int top_k, double top_p, double temp, int eos_id, int V, const char *pre = "", int r = 0) {
    char who[32];
    std::snprintf(who, sizeof who, pre, r);
    if (top_k < 1 || top_k > bgk::SAMPLE_MAX_K || (V >= 0 && top_k > V)) BG_FAIL(false, "%stop_k must be in [1, %d] and at most n_vocab", who, bgk::SAMPLE_MAX_K);
    if (!check_temp_top_p(temp, top_p, who)) return false;
    if (V < 0 && eos_id < -1) BG_FAIL(false, "%seos_id %d out of range: must be a token id, or -1 for none", who, eos_id);
    if (V >= 0 && (eos_id < -1 || eos_id >= V)) BG_FAIL(false, "%seos_id %d out of range: must be in [0, %d), or -1 for none", who, eos_id, V);
    return true;
}

// The generators of n rows as a caller holds them, 625 words each (the state words, then the index of the next output): checked, into SampleSeq[] and back
constexpr size_t MT_WORDS = bgk::MT_N + 1;
static_assert(sizeof(bgk::SampleSeq::mt) == MT_WORDS * 4, "a generator as SampleSeq holds it");
static bool check_mt_states(const uint32_t *mt, int n) {
    for (int r = 0; r < n; r++)
        if (mt[r * MT_WORDS + bgk::MT_N] > (uint32_t)bgk::MT_N) BG_FAIL(false, "generator index out of range (row %d)", r);
    return true;
}
static void mt_states_in(bgk::SampleSeq *seq, const uint32_t *mt, int n) { for (int r = 0; r < n; r++) std::memcpy(seq[r].mt, mt + r * MT_WORDS, MT_WORDS * 4); }
static void mt_states_out(uint32_t *mt, const bgk::SampleSeq *seq, int n) { for (int r = 0; r < n; r++) std::memcpy(mt + r * MT_WORDS, seq[r].mt, MT_WORDS * 4); }

static_assert(sizeof(bgk::SampleWide) == sizeof(biogpt_hip_sampler), "the sampler goes to the device as it is");
// the ranges of a sampler's values, for rows of V entries (V < 0: the width is not known yet)
static bool check_sampler(const biogpt_hip_sampler *sp, int V) {
    if (!sp) BG_FAIL(false, "null sampler");
    if (sp->top_k < 0) BG_FAIL(false, "sampler: top_k must be 0 (the whole vocabulary) or in [1, n_vocab] (got %d)", sp->top_k);
    if (V >= 0 && sp->top_k > V) BG_FAIL(false, "sampler: top_k must be 0 (the whole vocabulary) or in [1, n_vocab = %d] (got %d)", V, sp->top_k);
    if (!check_temp_top_p(sp->temp, sp->top_p, "sampler: ")) return false;
    if (!std::isfinite(sp->min_p) || !(sp->min_p >= 0.0 && sp->min_p < 1.0)) BG_FAIL(false, "sampler: min_p must be finite and in [0, 1) (0: off)");
    return true;
}
static bgk::SampleWide sample_wide_of(const biogpt_hip_sampler &sp) {
    bgk::SampleWide w{};
    w.top_k = sp.top_k; w.top_p = sp.top_p; w.min_p = sp.min_p; w.temp = sp.temp;
    return w;
}
// a sampler that sample_rows_kernel serves: the call is then the plain one
static bool sampler_is_plain(const biogpt_hip_sampler &sp) { return sp.top_k >= 1 && sp.top_k <= bgk::SAMPLE_MAX_K && sp.min_p == 0.0; }

static int generate_sample_once(biogpt_hip_ctx *ctx, const int32_t *prompts, const int32_t *prompt_lens, int32_t n_prompts, int32_t n_samples,
                                int32_t n_batch, int32_t n_predict, int32_t top_k, double top_p, double temp, const uint32_t *seeds, int32_t eos_id,
                                int32_t *out_ids, int32_t *out_lens, double *seconds_out, const biogpt_hip_gen_rules *rules, biogpt_hip_trie *trie = nullptr,
                                const int32_t *prefix = nullptr, int32_t n_prefix = 0, const biogpt_hip_gen_logprobs *lp = nullptr,
                                const biogpt_hip_sampler *wide = nullptr) {
    clear_error();
    if (!ctx) BG_FAIL(-1, "null context");
    // (wide != null, biogpt_hip_generate_sample_wide / _prefix: sample_wide_rows_kernel is the selection and top_k, top_p, temp are not looked at; no rules, no
    // trie, no log-probabilities)
    if (wide && (rules || trie || lp)) BG_FAIL(-1, "the wide sampler cannot be combined with generation rules, a trie or log-probabilities");
    if (wide && !check_sampler(wide, ctx->hp.n_vocab)) return -1;
    if (!prompts || !prompt_lens || !seeds || !out_ids || !out_lens) BG_FAIL(-1, "null argument");
    if (lp && !check_gen_logprobs(lp, ctx->hp.n_vocab)) return -1;
    if (lp && (rules || trie)) BG_FAIL(-1, "log-probabilities cannot be combined with generation rules or a trie");
    if (!ctx->ready) BG_FAIL(-1, "model has no tensors loaded (empty model): cannot evaluate");
    if (session_refuses(ctx)) return -1;
    if (prefix && (n_prompts < 1 || n_samples < 1 || (int64_t)n_prompts * n_samples > 511))
        BG_FAIL(-1, "n_prompts x n_samples must be in [1, 511] behind a prefix");   // one slot holds the prefix
    if (n_prompts < 1 || n_samples < 1 || (int64_t)n_prompts * n_samples > 512) BG_FAIL(-1, "n_prompts x n_samples must be in [1, 512]");   // each sequence owns a full F32 KV cache
    const int n_seqs = n_prompts * n_samples;
    if (n_seqs > hp_cols(ctx)) BG_FAIL(-1, "n_prompts x n_samples (%d) exceeds the %d activation columns of this model", n_seqs, hp_cols(ctx));
    if (n_batch < 1) BG_FAIL(-1, "n_batch must be >= 1");
    const int P = ctx->hp.n_positions, V = ctx->hp.n_vocab;
    if (!check_sample_values(top_k, top_p, temp, eos_id, V)) return -1;
    {   // the wide chain serves the plain call; each variant it does not serve is refused by its name
        const char *variant = wide ? "whole-vocabulary sampling" : trie ? "trie-constrained sampling" : prefix ? "sampled generation behind a shared prefix"
                              : lp ? "sampled generation with log-probabilities" : rules_active(rules, eos_id) ? "sampled generation under rules" : nullptr;
        if (!check_fast_chain(ctx, variant ? variant : "sampled generation", variant == nullptr)) return -1;
    }
    if (!check_rules(rules, V, P)) return -1;
    if (trie && !check_trie_vocab(trie, V)) return -1;
    const bool ru = rules_active(rules, eos_id);
    SampleBufs sb{};
    GenLpBufs lb{};
    ColumnCall cc(ctx);
    cc.prompts = prompts; cc.prompt_lens = prompt_lens;
    cc.n_prompts = n_prompts; cc.per_prompt = n_samples; cc.n_batch = n_batch;
    cc.graphs = &ctx->graphs_sample; cc.key_a = n_seqs;
    cc.form.sel = wide ? StepForm::Wide : trie ? StepForm::Trie : ru ? StepForm::Rules : StepForm::Plain;
    cc.prefix = prefix; cc.n_prefix = n_prefix;     // (prefix != null, biogpt_hip_generate_sample_prefix: the prompts are suffixes and may be empty; no rules, no trie)
    cc.form.lp = lp != nullptr;                     // (biogpt_hip_generate_sample_lp: sample_lp_rows_kernel is the selection; no rules, no trie)
    cc.prepare = [&]() -> bool {
        if (lp && !genlp_prepare(ctx, &lb)) return false;
        if (n_seqs > ctx->sample_cap) {
            if (ctx->sample_ctl) (void)hipFree(ctx->sample_ctl);
            ctx->sample_ctl = nullptr; ctx->sample_cap = 0;
            drop_graphs(ctx->graphs_sample);
            HIP_TRY(false, hipMalloc(&ctx->sample_ctl, sample_bufs_at(nullptr, (size_t)n_seqs).bytes));
            ctx->sample_cap = n_seqs;
        }
        sb = sample_bufs_at(reinterpret_cast<uint8_t *>(ctx->sample_ctl), (size_t)n_seqs);
        if (eos_id >= 0) cc.live_dev = &sb.ctl->n_live;
        return true;
    };
    cc.upload = [&]() -> bool {      // the call's parameters and the generators (std::mt19937(seeds[r]), their first block of outputs made here)
        std::vector<uint8_t> h(sb.bytes, 0);
        const SampleBufs hb = sample_bufs_at(h.data(), (size_t)n_seqs);
        *hb.ctl = sample_ctl_of(top_k, eos_id, n_seqs, top_p, temp);
        if (wide) *hb.wide = sample_wide_of(*wide);
        for (int r = 0; r < n_seqs; r++) { bgk::mt_seed(seeds[r], hb.seq[r].mt); bgk::mt_regenerate(hb.seq[r].mt); }
        HIP_TRY(false, hipMemcpy(sb.ctl, h.data(), h.size(), hipMemcpyHostToDevice));
        if (lp && !genlp_upload(lb, lp->n_top, cc.n_predict)) return false;
        if (trie && !trie_upload(ctx, trie, 0, eos_id)) return false;
        return !ru || rules_upload(ctx, rules, 0, eos_id, prompts, prompt_lens, n_prompts, n_samples);
    };
    cc.step = [&](int t_max) -> bool {
        if (!enqueue_forward(ctx, cc.in_place ? ForwardPass::decode_step_shared(n_seqs, t_max, cc.n_shared) : ForwardPass::decode_step(n_seqs, t_max))) return false;
        if (ru && !enqueue_rules(ctx, n_seqs, &sb.seq->finished, (int)(sizeof(bgk::SampleSeq) / 4))) return false;
        if (trie && !enqueue_trie(ctx, n_seqs, &sb.seq->finished, (int)(sizeof(bgk::SampleSeq) / 4))) return false;
        if (wide)
            hipLaunchKernelGGL(bgk::sample_wide_rows_kernel, dim3(n_seqs), dim3(bgk::WIDE_THREADS), 0, ctx->stream, ctx->logits_all, V, V, sb.wide, sb.ctl, sb.seq, ctx->seq,
                               ctx->seq_gen, P, (int32_t *)nullptr);
        else if (lp)
            hipLaunchKernelGGL(bgk::sample_lp_rows_kernel, dim3(n_seqs), dim3(bgk::SAMPLE_THREADS), 0, ctx->stream, ctx->logits_all, V, V, sb.ctl, sb.seq, ctx->seq, ctx->seq_gen, P,
                               lb.out());
        else
            hipLaunchKernelGGL(bgk::sample_rows_kernel, dim3(n_seqs), dim3(bgk::SAMPLE_THREADS), 0, ctx->stream, ctx->logits_all, V, V, sb.ctl, sb.seq, ctx->seq, ctx->seq_gen, P);
        HIP_TRY(false, hipGetLastError());
        return true;
    };
    n_predict = run_column_call(ctx, cc, n_predict, seconds_out);
    if (n_predict <= 0) return n_predict;
    std::vector<int32_t> gen((size_t)n_seqs * P);
    std::vector<bgk::SeqState> hs((size_t)n_seqs);
    HIP_TRY(-2, hipMemcpy(gen.data(), ctx->seq_gen, gen.size() * 4, hipMemcpyDeviceToHost));
    HIP_TRY(-2, hipMemcpy(hs.data(), ctx->seq, sizeof(bgk::SeqState) * n_seqs, hipMemcpyDeviceToHost));
    for (int r = 0; r < n_seqs; r++) {
        const int len = std::max(0, std::min(hs[(size_t)r].n_gen, n_predict));
        int32_t *o = out_ids + (size_t)r * n_predict;
        std::fill(o, o + n_predict, -1);
        std::memcpy(o, gen.data() + (size_t)r * P, (size_t)len * 4);
        out_lens[r] = len;
    }
    if (lp && !genlp_read(lb, lp, n_seqs, n_predict, out_lens)) return -2;
    return n_predict;
}

int biogpt_hip_generate_sample(biogpt_hip_ctx *ctx, const int32_t *prompts, const int32_t *prompt_lens, int32_t n_prompts, int32_t n_samples,
                               int32_t n_batch, int32_t n_predict, int32_t top_k, double top_p, double temp, const uint32_t *seeds, int32_t eos_id,
                               int32_t *out_ids, int32_t *out_lens, double *seconds_out) {
    return biogpt_hip_generate_sample_rules(ctx, prompts, prompt_lens, n_prompts, n_samples, n_batch, n_predict, top_k, top_p, temp, seeds, eos_id, out_ids, out_lens,
                                            seconds_out, nullptr);
}

int biogpt_hip_generate_sample_rules(biogpt_hip_ctx *ctx, const int32_t *prompts, const int32_t *prompt_lens, int32_t n_prompts, int32_t n_samples,
                                     int32_t n_batch, int32_t n_predict, int32_t top_k, double top_p, double temp, const uint32_t *seeds, int32_t eos_id,
                                     int32_t *out_ids, int32_t *out_lens, double *seconds_out, const biogpt_hip_gen_rules *rules) {
    return with_xpipe_retry(ctx, 0, [&] {
        return generate_sample_once(ctx, prompts, prompt_lens, n_prompts, n_samples, n_batch, n_predict, top_k, top_p, temp, seeds, eos_id, out_ids, out_lens, seconds_out, rules);
    });
}

// biogpt_hip_generate_sample of the sequences prefix ++ suffix_p behind the shared prefix rows; no rules, no trie
int biogpt_hip_generate_sample_prefix(biogpt_hip_ctx *ctx, const int32_t *prefix, int32_t n_prefix, const int32_t *suffixes, const int32_t *suffix_lens, int32_t n_prompts,
                                      int32_t n_samples, int32_t n_batch, int32_t n_predict, int32_t top_k, double top_p, double temp, const uint32_t *seeds, int32_t eos_id,
                                      int32_t *out_ids, int32_t *out_lens, double *seconds_out) {
    if (!check_prefix_pointers(ctx, prefix, suffixes, suffix_lens)) return -1;
    return with_xpipe_retry(ctx, 0, [&] {
        return generate_sample_once(ctx, suffixes, suffix_lens, n_prompts, n_samples, n_batch, n_predict, top_k, top_p, temp, seeds, eos_id, out_ids, out_lens, seconds_out, nullptr,
                                    nullptr, prefix, n_prefix);
    });
}

// biogpt_hip_generate_sample (prefix == null) or biogpt_hip_generate_sample_prefix with a sampler of any width.  One that sample_rows_kernel serves is handed
// to the plain call as its three values: the same launches, the same graphs
static int generate_sample_wide(biogpt_hip_ctx *ctx, const int32_t *prefix, int32_t n_prefix, const int32_t *prompts, const int32_t *prompt_lens, int32_t n_prompts,
                                int32_t n_samples, int32_t n_batch, int32_t n_predict, const biogpt_hip_sampler *sampler, const uint32_t *seeds, int32_t eos_id,
                                int32_t *out_ids, int32_t *out_lens, double *seconds_out) {
    clear_error();
    if (!check_sampler(sampler, ctx ? ctx->hp.n_vocab : -1)) return -1;
    const bool plain = sampler_is_plain(*sampler);
    return with_xpipe_retry(ctx, 0, [&] {
        return generate_sample_once(ctx, prompts, prompt_lens, n_prompts, n_samples, n_batch, n_predict, plain ? sampler->top_k : 1, plain ? sampler->top_p : 1.0,
                                    plain ? sampler->temp : 1.0, seeds, eos_id, out_ids, out_lens, seconds_out, nullptr, nullptr, prefix, prefix ? n_prefix : 0, nullptr,
                                    plain ? nullptr : sampler);
    });
}
int biogpt_hip_generate_sample_wide(biogpt_hip_ctx *ctx, const int32_t *prompts, const int32_t *prompt_lens, int32_t n_prompts, int32_t n_samples, int32_t n_batch,
                                    int32_t n_predict, const biogpt_hip_sampler *sampler, const uint32_t *seeds, int32_t eos_id, int32_t *out_ids, int32_t *out_lens,
                                    double *seconds_out) {
    return generate_sample_wide(ctx, nullptr, 0, prompts, prompt_lens, n_prompts, n_samples, n_batch, n_predict, sampler, seeds, eos_id, out_ids, out_lens, seconds_out);
}
int biogpt_hip_generate_sample_wide_prefix(biogpt_hip_ctx *ctx, const int32_t *prefix, int32_t n_prefix, const int32_t *suffixes, const int32_t *suffix_lens,
                                           int32_t n_prompts, int32_t n_samples, int32_t n_batch, int32_t n_predict, const biogpt_hip_sampler *sampler,
                                           const uint32_t *seeds, int32_t eos_id, int32_t *out_ids, int32_t *out_lens, double *seconds_out) {
    if (!check_prefix_pointers(ctx, prefix, suffixes, suffix_lens)) return -1;
    return generate_sample_wide(ctx, prefix, n_prefix, suffixes, suffix_lens, n_prompts, n_samples, n_batch, n_predict, sampler, seeds, eos_id, out_ids, out_lens, seconds_out);
}

// biogpt_hip_generate_sample (prefix == null) or biogpt_hip_generate_sample_prefix with the log-probabilities of the generated tokens; no rules, no trie
int biogpt_hip_generate_sample_lp(biogpt_hip_ctx *ctx, const int32_t *prefix, int32_t n_prefix, const int32_t *suffixes, const int32_t *suffix_lens, int32_t n_prompts,
                                  int32_t n_samples, int32_t n_batch, int32_t n_predict, int32_t top_k, double top_p, double temp, const uint32_t *seeds, int32_t eos_id,
                                  int32_t *out_ids, int32_t *out_lens, double *seconds_out, const biogpt_hip_gen_logprobs *logprobs) {
    if (!check_lp_pointers(ctx, logprobs, prefix, n_prefix, suffixes, suffix_lens)) return -1;
    return with_xpipe_retry(ctx, 0, [&] {
        return generate_sample_once(ctx, suffixes, suffix_lens, n_prompts, n_samples, n_batch, n_predict, top_k, top_p, temp, seeds, eos_id, out_ids, out_lens, seconds_out, nullptr,
                                    nullptr, prefix, prefix ? n_prefix : 0, logprobs);
    });
}

// biogpt_hip_generate_sample with trie_rows_kernel (mode 0) in front of the sampler; no rules
int biogpt_hip_generate_sample_trie(biogpt_hip_ctx *ctx, const int32_t *prompts, const int32_t *prompt_lens, int32_t n_prompts, int32_t n_samples,
                                    int32_t n_batch, int32_t n_predict, int32_t top_k, double top_p, double temp, const uint32_t *seeds, int32_t eos_id,
                                    biogpt_hip_trie *trie, int32_t *out_ids, int32_t *out_lens, double *seconds_out) {
    clear_error();
    if (!check_trie(trie, eos_id)) return -1;
    return with_xpipe_retry(ctx, 0, [&] {
        return generate_sample_once(ctx, prompts, prompt_lens, n_prompts, n_samples, n_batch, n_predict, top_k, top_p, temp, seeds, eos_id, out_ids, out_lens, seconds_out, nullptr,
                                    trie);
    });
}

// ---- beam search: G prompts x B beams as columns of the batched decode step, every prompt a search of its own (kernels_beam.hip.h) ----
// The column generation above with the three beam kernels as the selection: forward(G * B columns) + beam_group_rows + beam_group_select + kv_group_fork.
// Every prompt is evaluated once, into the slot of its group's first column; at a group's first step the device expands its first row alone (the other
// beams have no score yet).  The steps stop once every search has finished (BeamBatchHdr::n_live).  biogpt_hip_generate_beam is the call with G = 1.  The
// context's own K / V cache, position and logits row are left alone.
constexpr int BBATCH_COLS = 512;    // columns of a call, at most
// The buffers a beam step works on: the context's (beam_bufs_of) or a test entry's own (biogpt_hip_beam_rows_device, biogpt_hip_beam_table_device).
struct BeamBufs {
    hipStream_t stream;
    const float *logits;        // [G * B][n_vocab]
    int n_vocab;
    bgk::BeamBatchHdr *hdr;
    bgk::BeamFork *forks;       // room for G * (B - 1)
    int32_t *col_skip;          // [G * B]
    bgk::BeamCtl *ctl;          // [G]
    bgk::BeamCand *cand;        // [G * B][2 * B]
    int32_t *pool_ids;          // [G * B][ctl->ids_stride]
    bgk::SeqState *seq;         // [G * B]
    int32_t *seq_gen;           // [G * B][gen_stride]
    int gen_stride;
    float *bk, *bv;             // [G * B] cache slots of seq_stride floats: kv_runs (layer, head) runs of P * dk
    int64_t seq_stride;
    int kv_runs, P, dk;
};

// The state block of a beam step -- [hdr | forks | skip | ctl | cand | pool ids] -- for `cols` columns in `groups` groups, laid out at l's position in the buffer at
// base
static void beam_state_parts(ByteLayout &l, uint8_t *base, size_t cols, size_t groups, size_t cand_per_col, size_t ids_stride, BeamBufs *b) {
    b->hdr = l.take<bgk::BeamBatchHdr>(base, 1);
    b->forks = l.take<bgk::BeamFork>(base, cols);
    b->col_skip = l.take<int32_t>(base, cols);
    b->ctl = l.take<bgk::BeamCtl>(base, groups);
    b->cand = l.take<bgk::BeamCand>(base, cols * cand_per_col);
    b->pool_ids = l.take<int32_t>(base, cols * ids_stride);
}

// the context's: one block allocated once at its largest (captured steps keep their pointers); bbatch_buf null: the block's size alone
static BeamBufs beam_bufs_of(biogpt_hip_ctx *c, size_t *bytes = nullptr) {
    const auto &hp = c->hp;
    const int P = hp.n_positions;
    BeamBufs b{};
    ByteLayout l;
    beam_state_parts(l, c->bbatch_buf, BBATCH_COLS, BBATCH_COLS, 2 * bgk::BEAM_MAX, (size_t)P, &b);
    if (bytes) *bytes = l.bytes();
    b.stream = c->stream;
    b.logits = c->logits_all; b.n_vocab = hp.n_vocab;
    b.seq = c->seq; b.seq_gen = c->seq_gen; b.gen_stride = P;
    b.bk = c->bk; b.bv = c->bv;
    b.seq_stride = (int64_t)hp.n_layer * P * hp.d_model; b.kv_runs = hp.n_layer * hp.n_head; b.P = P; b.dk = hp.d_model / hp.n_head;
    return b;
}

// a group's search as a call starts it
static bgk::BeamCtl beam_ctl_of(int n_beams, int n_prompt, int n_predict, int eos_id, float length_penalty, int early_stopping, int ids_stride) {
    bgk::BeamCtl c{};
    c.n_beams = n_beams; c.n_prompt = n_prompt; c.n_predict = n_predict; c.eos_id = eos_id;
    c.length_penalty = length_penalty; c.early_stopping = early_stopping; c.ids_stride = ids_stride;
    c.heur_unsat = 1;
    return c;
}

// The head of a state block (hdr .. ctl of G groups) as a call starts it: all G searches run, no forks, and the rules kernel skips the columns whose row the first
// step does not expand.  ids_stride = b.P.
static bool upload_beam_start(const BeamBufs &b, int G, int B, const int32_t *prompt_lens, int n_predict, int eos_id, float length_penalty, int early_stopping) {
    HeadImage im(b.hdr, b.ctl + G);
    im.at(b.hdr)->n_live = G;
    for (int p = 0; p < G; p++) {
        im.at(b.ctl)[p] = beam_ctl_of(B, prompt_lens[p], n_predict, eos_id, length_penalty, early_stopping, b.P);
        for (int j = 1; j < B; j++) im.at(b.col_skip)[p * B + j] = 1;
    }
    return im.upload();
}

static void launch_beam_group_rows(const BeamBufs &b, int G, int B, bool given) {
    const int V = b.n_vocab, K = 2 * B;
    auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(G * B), dim3(bgk::LP_THREADS), 0, b.stream, b.logits, V, V, b.ctl, B, b.hdr, b.cand); };
    if (given) {
        if (K <= 8) go(bgk::beam_group_rows_kernel<8, true>);
        else if (K <= 16) go(bgk::beam_group_rows_kernel<16, true>);
        else go(bgk::beam_group_rows_kernel<32, true>);
    } else if (K <= 8) go(bgk::beam_group_rows_kernel<8, false>);
    else if (K <= 16) go(bgk::beam_group_rows_kernel<16, false>);
    else go(bgk::beam_group_rows_kernel<32, false>);
}

// rows -> select -> fork.  given: the rows hold log-probabilities already (the rules kernel has run over them)
static bool enqueue_beam_group_select(const BeamBufs &b, int G, int B, bool given) {
    launch_beam_group_rows(b, G, B, given);
    HIP_TRY(false, hipGetLastError());
    hipLaunchKernelGGL(bgk::beam_group_select_kernel, dim3(G), dim3(bgk::BEAM_SELECT_THREADS), 0, b.stream, b.cand, b.ctl, B, b.seq, b.seq_gen, b.gen_stride, b.pool_ids,
                       b.hdr, b.forks, b.col_skip);
    HIP_TRY(false, hipGetLastError());
    if (B > 1) {
        hipLaunchKernelGGL(bgk::kv_group_fork_kernel, dim3(b.kv_runs, bgk::BEAM_FORK_WGS, 2), dim3(256), 0, b.stream, b.hdr, b.forks, b.bk, b.bv, b.seq_stride, b.P, b.dk,
                           b.seq_gen, b.gen_stride);
        HIP_TRY(false, hipGetLastError());
    }
    return true;
}

// the pools of G finished searches (ctl: host copies; pool_ids: [G * B][ids_stride]) -> the output rows of biogpt_hip_generate_beam_batch
// unit, index0: what a failure names -- group p is `unit` index0 + p
static bool beam_read_pools(const bgk::BeamCtl *ctl, const int32_t *pool_ids, size_t ids_stride, int G, int B, int n_predict, int32_t *out_ids, int32_t *out_lens,
                            float *out_scores, int32_t *out_counts, const char *unit = "prompt", int index0 = 0) {
    for (int p = 0; p < G; p++) {
        const bgk::BeamCtl &st = ctl[p];
        if (!st.done || st.pool_n < 1 || st.pool_n > B) BG_FAIL(false, "internal: beam search of %s %d ended with %d hypotheses (done word %d)", unit, index0 + p, st.pool_n, st.done);
        out_counts[p] = st.pool_n;
        for (int r = 0; r < B; r++) {
            const size_t row = (size_t)p * B + r;
            int32_t *o = out_ids + row * n_predict;
            std::fill(o, o + n_predict, -1);
            out_lens[row] = 0; out_scores[row] = 0.0f;
            if (r >= st.pool_n) continue;
            const int slot = st.pool_order[r];
            out_lens[row] = std::min(st.pool_len[slot], n_predict);
            out_scores[row] = st.pool_score[slot];
            std::memcpy(o, pool_ids + ((size_t)p * B + slot) * ids_stride, (size_t)out_lens[row] * 4);
        }
    }
    return true;
}

static int generate_beam_batch_once(biogpt_hip_ctx *ctx, const int32_t *prompts, const int32_t *prompt_lens, int32_t n_prompts, int32_t n_batch, int32_t n_beams,
                                    int32_t n_predict, int32_t eos_id, float length_penalty, int32_t early_stopping, const biogpt_hip_gen_rules *rules,
                                    int32_t *out_ids, int32_t *out_lens, float *out_scores, int32_t *out_counts, double *seconds_out, biogpt_hip_trie *trie = nullptr) {
    clear_error();
    if (!ctx) BG_FAIL(-1, "null context");
    if (!prompts || !prompt_lens || !out_ids || !out_lens || !out_scores || !out_counts) BG_FAIL(-1, "null argument");
    if (!ctx->ready) BG_FAIL(-1, "model has no tensors loaded (empty model): cannot evaluate");
    if (session_refuses(ctx)) return -1;
    if (n_prompts < 1) BG_FAIL(-1, "n_prompts must be >= 1");
    if (n_beams < 1 || n_beams > bgk::BEAM_MAX) BG_FAIL(-1, "n_beams must be in [1, %d]", bgk::BEAM_MAX);
    if ((int64_t)n_prompts * n_beams > BBATCH_COLS) BG_FAIL(-1, "n_prompts x n_beams must be at most %d", BBATCH_COLS);   // each column owns a full F32 KV cache
    const int G = n_prompts, B = n_beams, n_seqs = G * B;
    if (n_seqs > hp_cols(ctx)) BG_FAIL(-1, "n_prompts x n_beams (%d) exceeds the %d activation columns of this model", n_seqs, hp_cols(ctx));
    if (n_batch < 1) BG_FAIL(-1, "n_batch must be >= 1");
    const auto &hp = ctx->hp;
    const int P = hp.n_positions;
    if (eos_id < -1 || eos_id >= hp.n_vocab) BG_FAIL(-1, "eos_id %d out of range: must be in [0, %d), or -1 for none", eos_id, hp.n_vocab);
    if (!std::isfinite(length_penalty)) BG_FAIL(-1, "length_penalty must be finite");
    if (early_stopping != 0 && early_stopping != 1) BG_FAIL(-1, "early_stopping must be 0 or 1");
    {
        const char *variant = trie ? "trie-constrained beam search" : rules_active(rules, eos_id) ? "beam search under rules" : nullptr;
        if (!check_fast_chain(ctx, variant ? variant : "beam search", variant == nullptr)) return -1;
    }
    if (hp.n_vocab < 2 * B) BG_FAIL(-1, "a vocabulary of %d tokens holds fewer than 2 x n_beams candidates", hp.n_vocab);
    if (!check_rules(rules, hp.n_vocab, P)) return -1;
    if (rules_ban(rules, eos_id) && hp.n_vocab - rules->n_suppress - 1 - P < 2 * B)
        BG_FAIL(-1, "the rules could leave a row fewer than 2 x n_beams candidates: n_vocab - n_suppress - 1 - n_positions = %d < %d", hp.n_vocab - rules->n_suppress - 1 - P, 2 * B);
    if (trie && !check_trie_vocab(trie, hp.n_vocab)) return -1;
    const bool ru = rules_active(rules, eos_id);
    const bool given = ru || trie;      // the row kernel takes processed log-probabilities as they are
    BeamBufs bufs{};
    std::vector<bgk::BeamCtl> hc;
    std::vector<int32_t> ids;
    ColumnCall cc(ctx);
    cc.prompts = prompts; cc.prompt_lens = prompt_lens;
    cc.n_prompts = G; cc.per_prompt = B; cc.n_batch = n_batch;
    cc.graphs = &ctx->graphs_beam; cc.key_a = G; cc.key_b = B;
    cc.form.sel = trie ? StepForm::Trie : ru ? StepForm::Rules : StepForm::Plain;
    cc.prepare = [&]() -> bool {
        if (!ctx->bbatch_buf) {
            size_t bytes;
            beam_bufs_of(ctx, &bytes);
            HIP_TRY(false, hipMalloc(&ctx->bbatch_buf, bytes));
        }
        bufs = beam_bufs_of(ctx);
        cc.live_dev = &bufs.hdr->n_live;
        return true;
    };
    cc.upload = [&]() -> bool {
        return upload_beam_start(bufs, G, B, prompt_lens, cc.n_predict, eos_id, length_penalty, early_stopping) &&
               (!ru || rules_upload(ctx, rules, 1, eos_id, prompts, prompt_lens, G, B)) && (!trie || trie_upload(ctx, trie, 1, eos_id));
    };
    cc.step = [&](int t_max) -> bool {
        return enqueue_forward(ctx, ForwardPass::decode_step(n_seqs, t_max)) && (!ru || enqueue_rules(ctx, n_seqs, bufs.col_skip, 1)) &&
               (!trie || enqueue_trie(ctx, n_seqs, bufs.col_skip, 1)) && enqueue_beam_group_select(bufs, G, B, given);
    };
    cc.before_sync = [&]() -> bool {      // every group's pool comes back behind the last step
        hc.resize((size_t)G); ids.resize((size_t)n_seqs * P);
        HIP_TRY(false, hipMemcpyAsync(hc.data(), bufs.ctl, sizeof(bgk::BeamCtl) * (size_t)G, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(false, hipMemcpyAsync(ids.data(), bufs.pool_ids, ids.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
        return true;
    };
    n_predict = run_column_call(ctx, cc, n_predict, seconds_out);
    if (n_predict <= 0) return n_predict;
    if (!beam_read_pools(hc.data(), ids.data(), (size_t)P, G, B, n_predict, out_ids, out_lens, out_scores, out_counts)) return -2;
    return n_predict;
}

int biogpt_hip_generate_beam_batch(biogpt_hip_ctx *ctx, const int32_t *prompts, const int32_t *prompt_lens, int32_t n_prompts, int32_t n_batch, int32_t n_beams,
                                   int32_t n_predict, int32_t eos_id, float length_penalty, int32_t early_stopping, const biogpt_hip_gen_rules *rules,
                                   int32_t *out_ids, int32_t *out_lens, float *out_scores, int32_t *out_counts, double *seconds_out) {
    return with_xpipe_retry(ctx, 0, [&] {
        return generate_beam_batch_once(ctx, prompts, prompt_lens, n_prompts, n_batch, n_beams, n_predict, eos_id, length_penalty, early_stopping, rules, out_ids, out_lens,
                                        out_scores, out_counts, seconds_out);
    });
}

// biogpt_hip_generate_beam_batch with trie_rows_kernel (mode 1) in front of the selection over given rows; no rules.  Candidates at -inf are legal here: a
// row holds as few finite values as the trie allows, and the search is beam_ref's over the masked rows ("Constrained decoding")
int biogpt_hip_generate_beam_trie(biogpt_hip_ctx *ctx, const int32_t *prompts, const int32_t *prompt_lens, int32_t n_prompts, int32_t n_batch, int32_t n_beams,
                                  int32_t n_predict, int32_t eos_id, float length_penalty, int32_t early_stopping, biogpt_hip_trie *trie, int32_t *out_ids,
                                  int32_t *out_lens, float *out_scores, int32_t *out_counts, double *seconds_out) {
    clear_error();
    if (!check_trie(trie, eos_id)) return -1;
    return with_xpipe_retry(ctx, 0, [&] {
        return generate_beam_batch_once(ctx, prompts, prompt_lens, n_prompts, n_batch, n_beams, n_predict, eos_id, length_penalty, early_stopping, nullptr, out_ids, out_lens,
                                        out_scores, out_counts, seconds_out, trie);
    });
}

// one prompt: the call above with a group of one; returns the number of hypotheses
int biogpt_hip_generate_beam_rules(biogpt_hip_ctx *ctx, const int32_t *prompt, int32_t n_prompt, int32_t n_batch, int32_t n_beams, int32_t n_predict,
                                   int32_t eos_id, float length_penalty, int32_t early_stopping, int32_t *out_ids, int32_t *out_lens, float *out_scores,
                                   double *seconds_out, const biogpt_hip_gen_rules *rules) {
    clear_error();
    if (!ctx) BG_FAIL(-1, "null context");
    if (!prompt || !out_ids || !out_lens || !out_scores) BG_FAIL(-1, "null argument");
    if (!ctx->ready) BG_FAIL(-1, "model has no tensors loaded (empty model): cannot evaluate");
    if (session_refuses(ctx)) return -1;
    if (n_beams < 1 || n_beams > bgk::BEAM_MAX) BG_FAIL(-1, "n_beams must be in [1, %d]", bgk::BEAM_MAX);
    if (n_batch < 1) BG_FAIL(-1, "n_batch must be >= 1");
    if (n_prompt < 1) BG_FAIL(-1, "empty prompt");      // (in this order: a call with several bad arguments reports the first of them)
    int32_t count[1] = {0};
    const int rc = biogpt_hip_generate_beam_batch(ctx, prompt, &n_prompt, 1, n_batch, n_beams, n_predict, eos_id, length_penalty, early_stopping, rules, out_ids, out_lens,
                                                  out_scores, count, seconds_out);
    return rc > 0 ? count[0] : rc;
}

int biogpt_hip_generate_beam(biogpt_hip_ctx *ctx, const int32_t *prompt, int32_t n_prompt, int32_t n_batch, int32_t n_beams, int32_t n_predict,
                             int32_t eos_id, float length_penalty, int32_t early_stopping, int32_t *out_ids, int32_t *out_lens, float *out_scores,
                             double *seconds_out) {
    return biogpt_hip_generate_beam_rules(ctx, prompt, n_prompt, n_batch, n_beams, n_predict, eos_id, length_penalty, early_stopping, out_ids, out_lens, out_scores,
                                          seconds_out, nullptr);
}

// ---- contrastive search: G prompts x k candidates as columns of the batched decode step (kernels_contrast.hip.h) ----
// The column generation above with contrast_rank + contrast_select + contrast_kv_row as the selection, and the hidden rows of the step's columns as a
// second epilogue of its forward pass.  Every prompt is evaluated once, into the slot of its group's first column, and the same pass leaves the hidden rows
// of its tokens in the group's context store; a group's first step carries the prompt's last token in all k columns (ContrastGroup::first), so
// n_predict tokens take n_predict + 1 steps of one captured form.  The steps stop once every group has finished (ContrastCtl::n_live).  The context's own
// K / V cache, position and logits row are left alone.
constexpr int CONTRAST_COLS = 512;    // columns of a call, at most (and so groups: top_k = 1)
static int contrast_slabs(const biogpt_hip_ctx *c) { return (c->hp.n_positions + bgk::CT_SLAB - 1) / bgk::CT_SLAB; }
// The step's device state, one block allocated at the first call at its largest (captured steps keep their pointers); contrast_buf null: the block's size alone
struct ContrastBufs {
    bgk::ContrastCtl *ctl;
    bgk::ContrastGroup *grp;    // [CONTRAST_COLS]
    float *cand;                // [CONTRAST_COLS][d_model]: the hidden rows of the step's columns
    float *slab_max;            // [CONTRAST_COLS][slabs][CT_MAX_K]
    float *scores;              // [CONTRAST_COLS][n_positions]: the winning score of every token
    size_t bytes;
};
static ContrastBufs contrast_bufs_at(uint8_t *base, const biogpt_hip_ctx *c) {
    ByteLayout l;
    ContrastBufs b{};
    b.ctl = l.take<bgk::ContrastCtl>(base, 1);
    b.grp = l.take<bgk::ContrastGroup>(base, CONTRAST_COLS);
    b.cand = l.take<float>(base, (size_t)CONTRAST_COLS * c->hp.d_model);
    b.slab_max = l.take<float>(base, (size_t)CONTRAST_COLS * contrast_slabs(c) * bgk::CT_MAX_K);
    b.scores = l.take<float>(base, (size_t)CONTRAST_COLS * c->hp.n_positions);
    b.bytes = l.bytes();
    return b;
}

// the rank kernel's dynamic LDS: the candidate rows, at least the room of its closing exchange; above 64 KB it has to be asked for
static bool contrast_rank_lds(std::set<const void *> *done, int k, int d, size_t *bytes) {
    *bytes = std::max((size_t)k * d * 4, (size_t)4 * bgk::CT_MAX_K * 4);
    const void *fn = reinterpret_cast<const void *>(bgk::contrast_rank_kernel);
    if (*bytes >= 64 * 1024 && !(done && done->count(fn))) {
        HIP_TRY(false, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bgk::CT_MAX_K * bgk::CT_MAX_D * 4));
        if (done) done->insert(fn);
    }
    return true;
}

static int generate_contrastive_once(biogpt_hip_ctx *ctx, const int32_t *prompts, const int32_t *prompt_lens, int32_t n_prompts, int32_t n_batch, int32_t top_k,
                                     float penalty_alpha, int32_t n_predict, int32_t eos_id, int32_t *out_ids, int32_t *out_lens, float *out_scores,
                                     double *seconds_out) {
    clear_error();
    // (what can be judged without the model comes first: these fail the same way with no context and no device)
    if (!prompts) BG_FAIL(-1, "null argument: prompts");
    if (!prompt_lens) BG_FAIL(-1, "null argument: prompt_lens");
    if (!out_ids) BG_FAIL(-1, "null argument: out_ids");
    if (!out_lens) BG_FAIL(-1, "null argument: out_lens");
    if (n_prompts < 1) BG_FAIL(-1, "n_prompts must be >= 1");
    if (top_k < 1 || top_k > bgk::CT_MAX_K) BG_FAIL(-1, "top_k must be in [1, %d]", bgk::CT_MAX_K);
    if ((int64_t)n_prompts * top_k > CONTRAST_COLS) BG_FAIL(-1, "n_prompts x top_k must be at most %d", CONTRAST_COLS);   // each column owns a full F32 KV cache
    if (n_batch < 1) BG_FAIL(-1, "n_batch must be >= 1");
    if (!(penalty_alpha >= 0.0f && penalty_alpha <= 1.0f)) BG_FAIL(-1, "penalty_alpha must be in [0, 1]");
    if (eos_id < -1) BG_FAIL(-1, "eos_id %d out of range: must be a token id, or -1 for none", eos_id);
    if (!ctx) BG_FAIL(-1, "null context");
    if (!ctx->ready) BG_FAIL(-1, "model has no tensors loaded (empty model): cannot evaluate");
    if (session_refuses(ctx)) return -1;
    const int G = n_prompts, K = top_k, n_seqs = G * K;
    if (n_seqs > hp_cols(ctx)) BG_FAIL(-1, "n_prompts x top_k (%d) exceeds the %d activation columns of this model", n_seqs, hp_cols(ctx));
    const auto &hp = ctx->hp;
    const int P = hp.n_positions, V = hp.n_vocab, D = hp.d_model;
    if (eos_id >= V) BG_FAIL(-1, "eos_id %d out of range: must be in [0, %d), or -1 for none", eos_id, V);
    if (!check_fast_chain(ctx, "contrastive search")) return -1;
    if (V < K) BG_FAIL(-1, "a vocabulary of %d tokens holds fewer than top_k candidates", V);
    ContrastBufs cb{};
    float *H = nullptr;         // the context store: [groups][n_positions][d_model] f32 rows, then their squared norms
    double *Hn = nullptr;
    size_t rank_lds = 0;
    const int n_slabs = contrast_slabs(ctx);
    const int64_t seq_stride = (int64_t)hp.n_layer * P * D;
    ColumnCall cc(ctx);
    cc.prompts = prompts; cc.prompt_lens = prompt_lens;
    cc.n_prompts = G; cc.per_prompt = K; cc.n_batch = n_batch;
    cc.graphs = &ctx->graphs_contrast; cc.key_a = G; cc.key_b = K;
    cc.extra_steps = 1;      // the prompt's last token, then one step per generated token
    cc.prepare = [&]() -> bool {
        if (!ctx->contrast_buf) HIP_TRY(false, hipMalloc(&ctx->contrast_buf, contrast_bufs_at(nullptr, ctx).bytes));
        if (G > ctx->contrast_groups) {      // the context store: new pointers, so the captured steps go
            if (ctx->contrast_h) (void)hipFree(ctx->contrast_h);
            ctx->contrast_h = nullptr; ctx->contrast_groups = 0;
            drop_graphs(ctx->graphs_contrast);
            const size_t bytes = (size_t)G * P * ((size_t)D * 4 + 8);
            if (hipMalloc(&ctx->contrast_h, bytes) != hipSuccess) {
                (void)hipGetLastError();
                BG_FAIL(false, "contrastive search: no room for the context store of %d prompts (%zu bytes: n_prompts x n_positions x (d_model f32 + one double))", G, bytes);
            }
            ctx->contrast_groups = G;
        }
        cb = contrast_bufs_at(ctx->contrast_buf, ctx);
        H = ctx->contrast_h;
        Hn = reinterpret_cast<double *>(H + (size_t)ctx->contrast_groups * P * D);
        cc.hidden_store = H;
        if (eos_id >= 0) cc.live_dev = &cb.ctl->n_live;
        return contrast_rank_lds(&ctx->lds_attr_done, K, D, &rank_lds);
    };
    cc.upload = [&]() -> bool {      // the call's parameters and every group's initial state: the prompt without its last token is the context, the first step appends that token's row
        HeadImage im(cb.ctl, cb.grp + G);
        bgk::ContrastCtl *hc = im.at(cb.ctl);
        hc->top_k = K; hc->eos_id = eos_id; hc->n_live = G; hc->alpha = penalty_alpha;
        bgk::ContrastGroup *hg = im.at(cb.grp);
        for (int p = 0; p < G; p++) { hg[p].len = prompt_lens[p] - 1; hg[p].first = 1; hg[p].copy_pos = -1; }
        return im.upload();
    };
    cc.step = [&](int t_max) -> bool {
        if (!enqueue_forward(ctx, ForwardPass::decode_step_hidden(n_seqs, t_max, cb.cand))) return false;
        hipLaunchKernelGGL(bgk::contrast_rank_kernel, dim3(n_slabs, G), dim3(bgk::CT_THREADS), rank_lds, ctx->stream, cb.cand, H, Hn, cb.grp, K, D, P, cb.slab_max);
        hipLaunchKernelGGL(bgk::contrast_select_kernel, dim3(G), dim3(bgk::CT_THREADS), 0, ctx->stream, cb.cand, ctx->logits_all, V, V, cb.ctl, cb.grp, cb.slab_max, n_slabs, H, Hn, D, P,
                           ctx->seq, ctx->seq_gen, P, cb.scores);
        if (K > 1)
            hipLaunchKernelGGL(bgk::contrast_kv_row_kernel, dim3(hp.n_layer * hp.n_head, G), dim3(256), 0, ctx->stream, cb.grp, K, ctx->bk, ctx->bv, seq_stride, P, D / hp.n_head);
        HIP_TRY(false, hipGetLastError());
        return true;
    };
    cc.after_ingest = [&]() -> bool {      // the squared norms of the rows the prompt pass left in the store
        hipLaunchKernelGGL(bgk::contrast_norms_kernel, dim3(n_slabs, G), dim3(bgk::CT_THREADS), 0, ctx->stream, H, Hn, cb.grp, D, P);
        HIP_TRY(false, hipGetLastError());
        return true;
    };
    n_predict = run_column_call(ctx, cc, n_predict, seconds_out);
    if (n_predict <= 0) return n_predict;
    std::vector<int32_t> gen((size_t)n_seqs * P);
    std::vector<float> sc((size_t)G * P);
    std::vector<bgk::SeqState> hs((size_t)n_seqs);
    HIP_TRY(-2, hipMemcpy(gen.data(), ctx->seq_gen, gen.size() * 4, hipMemcpyDeviceToHost));
    HIP_TRY(-2, hipMemcpy(sc.data(), cb.scores, sc.size() * 4, hipMemcpyDeviceToHost));
    HIP_TRY(-2, hipMemcpy(hs.data(), ctx->seq, sizeof(bgk::SeqState) * n_seqs, hipMemcpyDeviceToHost));
    for (int p = 0; p < G; p++) {      // a group's output is the history of its first column
        const int len = std::max(0, std::min(hs[(size_t)p * K].n_gen, n_predict));
        int32_t *o = out_ids + (size_t)p * n_predict;
        std::fill(o, o + n_predict, -1);
        std::memcpy(o, gen.data() + (size_t)p * K * P, (size_t)len * 4);
        out_lens[p] = len;
        if (out_scores) {
            std::fill(out_scores + (size_t)p * n_predict, out_scores + (size_t)(p + 1) * n_predict, 0.0f);
            std::memcpy(out_scores + (size_t)p * n_predict, sc.data() + (size_t)p * P, (size_t)len * 4);
        }
    }
    return n_predict;
}

int biogpt_hip_generate_contrastive(biogpt_hip_ctx *ctx, const int32_t *prompts, const int32_t *prompt_lens, int32_t n_prompts, int32_t n_batch, int32_t top_k,
                                    float penalty_alpha, int32_t n_predict, int32_t eos_id, int32_t *out_ids, int32_t *out_lens, float *out_scores,
                                    double *seconds_out) {
    return with_xpipe_retry(ctx, 0, [&] {
        return generate_contrastive_once(ctx, prompts, prompt_lens, n_prompts, n_batch, top_k, penalty_alpha, n_predict, eos_id, out_ids, out_lens, out_scores, seconds_out);
    });
}

// ---- prompt-lookup speculative decoding (kernels_lookup.hip.h) ------------------------------------------------------------------------------------
// One sequence and K / V cache slot per prompt (per_prompt = 1); a step is a packed pass of 1 + max_draft columns per sequence: the sequence's current token and
// the tokens lookup_draft_kernel copied from its text behind the earliest match of its longest matching tail n-gram, at consecutive positions with
// t_vis = position + 1 -- exactly what single-token steps would have shown each of them.  lookup_accept_kernel keeps the arg-max of every row up to the first
// draft that is not its row's arg-max, so the ids are those of biogpt_hip_generate_greedy_batch whatever was drafted.  A sequence moves on by 1 .. 1 + max_draft
// positions per step, a number only the device knows: the driver's key stride is 1 + max_draft and the steps' attention bound follows the furthest position the
// device reports (run_column_steps).  The steps stop through LookupCtl::n_live; the worst case is n_predict steps.
constexpr int LOOKUP_COLS = 512;                // columns of a step, at most (and so sequences: max_draft = 0)
constexpr size_t LOOKUP_TEXT_WORDS = (size_t)1 << 21;      // the texts of a call: every sequence has corpus_len + n_positions words
struct LookupBufs {
    bgk::LookupCtl *ctl;
    bgk::LookupSeq *seq;        // [LOOKUP_COLS]
    bgk::SeqState *cols;        // [LOOKUP_COLS]: the packed column states of the step
    int32_t *text;              // [LOOKUP_TEXT_WORDS]
    size_t bytes;
};
static LookupBufs lookup_bufs_at(uint8_t *base, size_t n_seqs = LOOKUP_COLS, size_t n_cols = LOOKUP_COLS, size_t text_words = LOOKUP_TEXT_WORDS) {
    ByteLayout l;
    LookupBufs b{};
    b.ctl = l.take<bgk::LookupCtl>(base, 1);
    b.seq = l.take<bgk::LookupSeq>(base, n_seqs);
    b.cols = l.take<bgk::SeqState>(base, n_cols);
    b.text = l.take<int32_t>(base, text_words);
    b.bytes = l.bytes();
    return b;
}

// what can be judged of a lookup call without the model
static bool check_lookup_shape(int64_t n_seqs, int max_draft, int max_ngram) {
    if (max_draft < 0 || max_draft > bgk::LK_MAX_DRAFT) BG_FAIL(false, "max_draft must be in [0, %d]", bgk::LK_MAX_DRAFT);
    if (max_ngram < 1 || max_ngram > bgk::LK_MAX_NGRAM) BG_FAIL(false, "max_ngram must be in [1, %d]", bgk::LK_MAX_NGRAM);
    if (n_seqs * (1 + max_draft) > LOOKUP_COLS) BG_FAIL(false, "n_prompts x (1 + max_draft) must be at most %d", LOOKUP_COLS);
    return true;
}

static int generate_lookup_once(biogpt_hip_ctx *ctx, const int32_t *prompts, const int32_t *prompt_lens, int32_t n_prompts, const int32_t *corpus,
                                const int32_t *corpus_lens, int32_t n_batch, int32_t n_predict, int32_t max_draft, int32_t max_ngram, int32_t eos_id,
                                int32_t *out_ids, int32_t *out_lens, int32_t *out_stats, double *seconds_out) {
    clear_error();
    // (what can be judged without the model comes first: these fail the same way with no context and no device)
    if (!prompts) BG_FAIL(-1, "null argument: prompts");
    if (!prompt_lens) BG_FAIL(-1, "null argument: prompt_lens");
    if (!out_ids) BG_FAIL(-1, "null argument: out_ids");
    if (!out_lens) BG_FAIL(-1, "null argument: out_lens");
    if ((corpus == nullptr) != (corpus_lens == nullptr)) BG_FAIL(-1, "corpus and corpus_lens must both be given, or both be NULL");
    if (n_prompts < 1) BG_FAIL(-1, "n_prompts must be >= 1");
    if (!check_lookup_shape(n_prompts, max_draft, max_ngram)) return -1;
    if (n_batch < 1) BG_FAIL(-1, "n_batch must be >= 1");
    if (eos_id < -1) BG_FAIL(-1, "eos_id %d out of range: must be a token id, or -1 for none", eos_id);
    size_t corpus_total = 0;
    for (int p = 0; corpus_lens && p < n_prompts; p++) {
        if (corpus_lens[p] < 0) BG_FAIL(-1, "corpus_lens[%d] = %d is negative", p, corpus_lens[p]);
        corpus_total += (size_t)corpus_lens[p];
    }
    if (!ctx) BG_FAIL(-1, "null context");
    if (!ctx->ready) BG_FAIL(-1, "model has no tensors loaded (empty model): cannot evaluate");
    if (session_refuses(ctx)) return -1;
    const int G = n_prompts, S = 1 + max_draft, n_cols = G * S;
    if (n_cols > hp_cols(ctx)) BG_FAIL(-1, "n_prompts x (1 + max_draft) (%d) exceeds the %d activation columns of this model", n_cols, hp_cols(ctx));
    const auto &hp = ctx->hp;
    const int P = hp.n_positions, V = hp.n_vocab;
    if (eos_id >= V) BG_FAIL(-1, "eos_id %d out of range: must be in [0, %d), or -1 for none", eos_id, V);
    for (size_t i = 0; i < corpus_total; i++)
        if (corpus[i] < 0 || corpus[i] >= V) BG_FAIL(-1, "corpus id %d out of range [0, %d)", corpus[i], V);
    if (corpus_total + (size_t)G * P > LOOKUP_TEXT_WORDS)
        BG_FAIL(-1, "corpus tokens (%zu) + n_prompts x n_positions (%d x %d) exceed the %zu words of the text buffer", corpus_total, G, P, LOOKUP_TEXT_WORDS);
    if (!check_fast_chain(ctx, "prompt-lookup decoding")) return -1;

    if (max_draft == 0) {      // nothing to draft: the batched greedy call itself, its ids cut behind the first EOS
        std::vector<int32_t> ids((size_t)G * std::max(n_predict, 1));
        const int n = generate_greedy_batch_once(ctx, prompts, prompt_lens, G, n_batch, n_predict, ids.data(), seconds_out);
        if (n <= 0) return n;
        for (int p = 0; p < G; p++) {
            const int32_t *row = ids.data() + (size_t)p * n;
            int len = n;
            for (int i = 0; i < n && eos_id >= 0; i++) if (row[i] == eos_id) { len = i + 1; break; }
            std::fill(out_ids + (size_t)p * n, out_ids + (size_t)(p + 1) * n, -1);
            std::memcpy(out_ids + (size_t)p * n, row, (size_t)len * 4);
            out_lens[p] = len;
            if (out_stats) { out_stats[3 * p] = len; out_stats[3 * p + 1] = 0; out_stats[3 * p + 2] = 0; }
        }
        return n;
    }

    LookupBufs lb{};
    ColumnCall cc(ctx);
    cc.prompts = prompts; cc.prompt_lens = prompt_lens;
    cc.n_prompts = G; cc.n_batch = n_batch;
    cc.graphs = &ctx->graphs_lookup; cc.key_a = G; cc.key_b = max_draft;
    cc.key_stride = S; cc.plain_steps = true;
    cc.prepare = [&]() -> bool {
        if (!ctx->lookup_buf) HIP_TRY(false, hipMalloc(&ctx->lookup_buf, lookup_bufs_at(nullptr).bytes));
        lb = lookup_bufs_at(ctx->lookup_buf);
        cc.live_dev = &lb.ctl->n_live;
        if (n_cols >= MFMA_MIN_PASS_COLS && !ensure_tile_images(ctx)) return false;
        return ensure_logits_rows(ctx, (size_t)n_cols);      // (a new buffer drops this mode's captured steps with the others')
    };
    cc.upload = [&]() -> bool {      // the call's parameters, every sequence's counters and its text: corpus ++ prompt, the generated tokens follow on the device
        HeadImage im(lb.ctl, lb.seq + G);
        bgk::LookupCtl *hc = im.at(lb.ctl);
        hc->max_draft = max_draft; hc->max_ngram = max_ngram; hc->eos_id = eos_id; hc->n_predict = cc.n_predict;
        hc->n_live = G; hc->max_pos = cc.max_len - 1;
        bgk::LookupSeq *hq = im.at(lb.seq);
        std::vector<int32_t> text(corpus_total + (size_t)G * P, 0);
        size_t at = 0, co = 0, po = 0;
        for (int p = 0; p < G; p++) {
            const int cl = corpus_lens ? corpus_lens[p] : 0;
            hq[p].text_off = (int32_t)at; hq[p].base_len = cl + prompt_lens[p];
            if (cl) std::memcpy(text.data() + at, corpus + co, (size_t)cl * 4);
            std::memcpy(text.data() + at + cl, prompts + po, (size_t)prompt_lens[p] * 4);
            at += (size_t)cl + P; co += (size_t)cl; po += (size_t)prompt_lens[p];
        }
        HIP_TRY(false, hipMemcpy(lb.text, text.data(), text.size() * 4, hipMemcpyHostToDevice));
        return im.upload();
    };
    cc.step = [&](int t_max) -> bool {
        hipLaunchKernelGGL(bgk::lookup_draft_kernel, dim3(G), dim3(bgk::LK_DRAFT_THREADS), 0, ctx->stream, lb.ctl, lb.seq, lb.text, ctx->seq, lb.cols);
        HIP_TRY(false, hipGetLastError());
        if (!enqueue_forward(ctx, ForwardPass::packed_verify(n_cols, t_max, lb.cols))) return false;
        hipLaunchKernelGGL(bgk::lookup_accept_kernel, dim3(G), dim3(bgk::LK_ACCEPT_THREADS), 0, ctx->stream, lb.ctl, lb.seq, lb.text, ctx->logits_all, V, V, ctx->seq,
                           ctx->seq_gen, P);
        HIP_TRY(false, hipGetLastError());
        return true;
    };
    n_predict = run_column_call(ctx, cc, n_predict, seconds_out);
    if (n_predict <= 0) return n_predict;
    std::vector<int32_t> gen((size_t)G * P);
    std::vector<bgk::SeqState> hs((size_t)G);
    std::vector<bgk::LookupSeq> hq((size_t)G);
    HIP_TRY(-2, hipMemcpy(gen.data(), ctx->seq_gen, gen.size() * 4, hipMemcpyDeviceToHost));
    HIP_TRY(-2, hipMemcpy(hs.data(), ctx->seq, sizeof(bgk::SeqState) * G, hipMemcpyDeviceToHost));
    HIP_TRY(-2, hipMemcpy(hq.data(), lb.seq, sizeof(bgk::LookupSeq) * G, hipMemcpyDeviceToHost));
    for (int p = 0; p < G; p++) {
        if (!hq[(size_t)p].finished) BG_FAIL(-2, "internal: prompt-lookup decoding left prompt %d unfinished after %d steps (%d of %d tokens)", p, n_predict, hs[(size_t)p].n_gen, n_predict);
        const int len = std::max(0, std::min(hs[(size_t)p].n_gen, n_predict));
        int32_t *o = out_ids + (size_t)p * n_predict;
        std::fill(o, o + n_predict, -1);
        std::memcpy(o, gen.data() + (size_t)p * P, (size_t)len * 4);
        out_lens[p] = len;
        if (out_stats) { out_stats[3 * p] = hq[(size_t)p].passes; out_stats[3 * p + 1] = hq[(size_t)p].drafted; out_stats[3 * p + 2] = hq[(size_t)p].accepted; }
    }
    return n_predict;
}

int biogpt_hip_generate_lookup(biogpt_hip_ctx *ctx, const int32_t *prompts, const int32_t *prompt_lens, int32_t n_prompts, const int32_t *corpus,
                               const int32_t *corpus_lens, int32_t n_batch, int32_t n_predict, int32_t max_draft, int32_t max_ngram, int32_t eos_id,
                               int32_t *out_ids, int32_t *out_lens, int32_t *out_stats, double *seconds_out) {
    return with_xpipe_retry(ctx, 0, [&] {
        return generate_lookup_once(ctx, prompts, prompt_lens, n_prompts, corpus, corpus_lens, n_batch, n_predict, max_draft, max_ngram, eos_id, out_ids, out_lens,
                                    out_stats, seconds_out);
    });
}

// ---- calls over a queue: finished units are refilled from a queue of requests ---------------------------------------------------------------------
// U = min(the most units the call may use, eligible requests) units serve any number of requests.  A unit is a column with its K / V slot
// (biogpt_hip_generate_queue, kernels_queue.hip.h) or a group slot of B columns (biogpt_hip_generate_beam_queue, kernels_beam_queue.hip.h): a request takes a
// unit when one is free, generates there at its own positions and under its own limit, and leaves the unit to the next request when it finishes.  The
// schedule counts steps, never time (QueueSchedule, whose "columns" are units; biogpt_hip_queue_plan is the same struct with given lengths), and
// run_queue_call is the one procedure of both modes:
//   1. eligible requests (those that may generate a token) are admitted in index order, the first U into units 0 .. U - 1;
//   2. steps are enqueued in groups of min(group, the most steps any running unit may still take);
//   3. behind each group the mode's header (finished flags, lengths) travels to pinned memory and the host waits for it;
//   4. every unit found finished has its results copied out by the mode (collect), in stream order, before the unit is reused;
//   5. finished units are refilled in ascending unit order with the pending requests in ascending request order: their prompts go through packed
//      prompt passes into exactly those units' (first) slots, the admit list goes up, the mode's launches behind it (enqueue_admit) set their state, and
//      they take part from the next group's first step;
//   6. the call ends when a header shows no running unit and nothing is pending.
// The host bounds every step's keys itself: a unit in use -- running, or finished and not refilled yet (it still attends at its frozen position) -- stands
// at position len - 1 + min(steps since admission, its limit) at most.  A refilled slot keeps its old rows beyond the new prompt: no decode-step attention
// kernel lets a column see a key at or beyond its own n_past + 1.  The steps are always the launch chain.
// A mode supplies (QueueCall): its units, its captured steps, the step itself, the admit record of a request and the launches behind the list, its header,
// and what happens to a finished unit's results.  Everything else -- the shared argument checks, the clamps, the schedule, capture, the loop, the waits,
// the timed span and the stats -- is stated once.
// Behind a shared prefix (QueueRequests::prefix, biogpt_hip_generate_queue_prefix) a request is prefix ++ its prompt: every length the driver reasons with is
// the whole sequence's (whole_len), the prefix's shared rows are evaluated once into one slot behind the units', inside the timed span and before the first
// refill, and a refill packs what follows them.
extern "C++" {
struct QueueSchedule {
    const std::vector<int32_t> &cap;        // tokens request r may generate at most; 0: it never takes a column.  A session appends to it (submit)
    int known = 0;                          // requests of cap the schedule has counted
    int C = 0, group, next = 0, pending = 0, running = 0;
    std::vector<int32_t> req, since;        // per column: its request (-1: none yet), steps since its admission
    std::vector<uint8_t> live;              // per column: its request still runs
    std::vector<uint8_t> dropped;           // per request: withdrawn while it was pending (a session's cancel)
    biogpt_hip_queue_stats st{};
    // A closed call: every request of cap_ is there, and the columns shrink to the eligible requests.  A session (fixed_columns): max_columns columns from
    // the start on, whatever has been submitted.
    QueueSchedule(const std::vector<int32_t> &cap_, int max_columns, int group_, bool fixed_columns = false) : cap(cap_), group(group_) {
        while (known < (int)cap.size()) submit();
        C = fixed_columns ? max_columns : std::min(max_columns, pending);
        req.assign((size_t)C, -1); since.assign((size_t)C, 0); live.assign((size_t)C, 0);
        st.columns = C;
    }
    // the request appended to cap becomes pending (or, without room for a token, never takes a column); its index
    int submit() { dropped.push_back(0); pending += cap[(size_t)known] > 0 ? 1 : 0; return known++; }
    bool done() const { return running == 0 && pending == 0; }
    bool is_pending(int r) const { return r >= next && r < known && cap[(size_t)r] > 0 && !dropped[(size_t)r]; }
    void drop(int r) { dropped[(size_t)r] = 1; pending--; }      // a pending request is withdrawn: it never takes a column
    int column_of(int r) const { for (int col = 0; col < C; col++) if (live[(size_t)col] && req[(size_t)col] == r) return col; return -1; }
    // free columns, ascending <- pending requests, ascending: admit(col, r) for each; the number admitted
    template <class Admit> int refill(Admit admit) {
        int n = 0;
        for (int col = 0; col < C && pending > 0; col++) {
            if (live[(size_t)col]) continue;
            while (cap[(size_t)next] <= 0 || dropped[(size_t)next]) next++;
            req[(size_t)col] = next; since[(size_t)col] = 0; live[(size_t)col] = 1;
            admit(col, next);
            next++; pending--; running++; n++;
        }
        st.admissions += n > 0 ? 1 : 0;
        return n;
    }
    int group_steps() const {
        int most = 0;
        for (int col = 0; col < C; col++) if (live[(size_t)col]) most = std::max(most, cap[(size_t)req[(size_t)col]] - since[(size_t)col]);
        return std::min(group, most);
    }
    // the position of column col's token at its next step, at most (len: its prompt's length); -1: the column was never used
    int position(int col, int len) const { return req[(size_t)col] < 0 ? -1 : len - 1 + std::min(since[(size_t)col], cap[(size_t)req[(size_t)col]]); }
    void step() { for (int col = 0; col < C; col++) if (req[(size_t)col] >= 0) since[(size_t)col]++; st.steps++; st.column_steps += C; }
    void end_group() { st.groups++; }
    void retire(int col, int len) { live[(size_t)col] = 0; running--; st.busy_column_steps += len; }
};

// The schedule of a queue session (biogpt_hip_queue_open): QueueSchedule with its columns fixed, fed while it runs.  A request is submitted, and may be
// cancelled, between two polls; what that does to the schedule happens at the next poll's start (begin_poll), in front of its first refill.  The session
// drives this struct and biogpt_hip_queue_plan_script runs it on a script with given lengths: one scheduler, with and without a device.
struct QueueSessionSchedule {
    enum State : uint8_t { PENDING, RUNNING, FINISHED, CANCELLED };
    std::vector<int32_t> cap;
    QueueSchedule q;
    std::vector<uint8_t> state, asked;      // per request: where it stands; a cancel has been asked for
    std::vector<int32_t> idle_new, cancels; // since the last poll: requests submitted without room for a token; cancels, in the order asked
    QueueSessionSchedule(int max_columns, int group) : q(cap, max_columns, group, true) {}
    int submit(int cap_r) {
        cap.push_back(std::max(cap_r, 0));
        state.push_back(cap_r > 0 ? PENDING : FINISHED); asked.push_back(0);
        const int r = q.submit();
        if (cap_r <= 0) idle_new.push_back(r);
        return r;
    }
    // 0: the request will be cancelled at the next poll's start; -1: no such request; -2: it has finished or was cancelled already
    int cancel(int r) {
        if (r < 0 || r >= q.known) return -1;
        if (state[(size_t)r] == FINISHED || state[(size_t)r] == CANCELLED || asked[(size_t)r]) return -2;
        asked[(size_t)r] = 1; cancels.push_back(r);
        return 0;
    }
    // A poll's start: idle(r) for a request that may not generate a token (it is finished with length 0); dropped(r) for a cancelled pending request;
    // stopped(col, r, len) for a cancelled running one, whose column is free for this poll's first refill -- a running request has taken one step per step
    // since its admission, so the host knows its length without a look.
    template <class Idle, class Dropped, class Stopped> void begin_poll(Idle idle, Dropped dropped, Stopped stopped) {
        for (int r : idle_new) idle(r);
        idle_new.clear();
        for (int r : cancels) {
            if (state[(size_t)r] == PENDING) { q.drop(r); state[(size_t)r] = CANCELLED; dropped(r); }
            else if (state[(size_t)r] == RUNNING) {
                const int col = q.column_of(r), len = q.since[(size_t)col];
                q.retire(col, len); state[(size_t)r] = CANCELLED;
                stopped(col, r, len);
            }
        }
        cancels.clear();
    }
    void admitted(int r) { state[(size_t)r] = RUNNING; }
    void finished(int col, int r, int len) { q.retire(col, len); state[(size_t)r] = FINISHED; }
};
}  // extern "C++"

// limits == gen_lens: biogpt_hip_queue_plan.  The host of a run sizes a group from the limits (it does not know where a request will end) and a look finds
// finished whoever has generated all its gen_lens[r] tokens.
static int queue_plan_of(const int32_t *gen_lens, const int32_t *limits, int32_t n_requests, int32_t max_columns, int32_t group, int32_t *admit_step, int32_t *column,
                         biogpt_hip_queue_stats *stats) {
    clear_error();
    if (!gen_lens) BG_FAIL(-1, "null argument: gen_lens");
    if (!limits) BG_FAIL(-1, "null argument: limits");
    if (!admit_step) BG_FAIL(-1, "null argument: admit_step");
    if (!column) BG_FAIL(-1, "null argument: column");
    if (n_requests < 1) BG_FAIL(-1, "n_requests must be >= 1");
    if (max_columns < 1 || max_columns > bgk::QUEUE_COLS) BG_FAIL(-1, "max_columns must be in [1, %d]", bgk::QUEUE_COLS);
    if (group < 1 || group > 64) BG_FAIL(-1, "group must be in [1, 64]");
    for (int r = 0; r < n_requests; r++) if (gen_lens[r] < 0) BG_FAIL(-1, "gen_lens[%d] (%d) is negative", r, gen_lens[r]);
    for (int r = 0; r < n_requests; r++) {
        if (limits[r] < gen_lens[r]) BG_FAIL(-1, "limits[%d] (%d) is below gen_lens[%d] (%d)", r, limits[r], r, gen_lens[r]);
        if (limits[r] > 0 && gen_lens[r] < 1) BG_FAIL(-1, "gen_lens[%d] is 0 under a limit of %d: a request that takes a column generates a token", r, limits[r]);
    }
    std::fill(admit_step, admit_step + n_requests, -1);
    std::fill(column, column + n_requests, -1);
    const std::vector<int32_t> cap(limits, limits + n_requests);
    QueueSchedule q(cap, max_columns, group);
    while (!q.done()) {
        q.refill([&](int col, int r) { admit_step[r] = q.st.steps; column[r] = col; });
        for (int g = q.group_steps(); g > 0; g--) q.step();
        q.end_group();
        for (int col = 0; col < q.C; col++)
            if (q.live[(size_t)col] && q.since[(size_t)col] >= gen_lens[q.req[(size_t)col]]) q.retire(col, gen_lens[q.req[(size_t)col]]);
    }
    if (stats) *stats = q.st;
    return 0;
}

int biogpt_hip_queue_plan(const int32_t *gen_lens, int32_t n_requests, int32_t max_columns, int32_t group, int32_t *admit_step, int32_t *column,
                          biogpt_hip_queue_stats *stats) {
    return queue_plan_of(gen_lens, gen_lens, n_requests, max_columns, group, admit_step, column, stats);
}

int biogpt_hip_queue_plan_limits(const int32_t *gen_lens, const int32_t *limits, int32_t n_requests, int32_t max_columns, int32_t group, int32_t *admit_step,
                                 int32_t *column, biogpt_hip_queue_stats *stats) {
    return queue_plan_of(gen_lens, limits, n_requests, max_columns, group, admit_step, column, stats);
}

// The session's scheduler on a script, with given lengths (biogpt_hip.h).  ops: [n_ops][2] = {kind, argument}: 0 SUBMIT (the next request: entry i of gen_lens /
// limits for the i-th submit), 1 POLL n (at most n groups), 2 CANCEL r.
int biogpt_hip_queue_plan_script(const int32_t *ops, int32_t n_ops, const int32_t *gen_lens, const int32_t *limits, int32_t max_columns, int32_t group, int32_t *admit_step,
                                 int32_t *column, int32_t *finish_group, int32_t *out_lens, biogpt_hip_queue_stats *stats) {
    clear_error();
    if (!ops) BG_FAIL(-1, "null argument: ops");
    if (n_ops < 0) BG_FAIL(-1, "n_ops must be >= 0");
    if (max_columns < 1 || max_columns > bgk::QUEUE_COLS) BG_FAIL(-1, "max_columns must be in [1, %d]", bgk::QUEUE_COLS);
    if (group < 1 || group > 64) BG_FAIL(-1, "group must be in [1, 64]");
    int R = 0;
    for (int i = 0; i < n_ops; i++) {
        const int kind = ops[2 * i], arg = ops[2 * i + 1];
        if (kind < 0 || kind > 2) BG_FAIL(-1, "ops[%d]: kind %d is none of 0 SUBMIT, 1 POLL, 2 CANCEL", i, kind);
        if (kind == 1 && arg < 0) BG_FAIL(-1, "ops[%d]: POLL %d: the groups of a poll must be >= 0", i, arg);
        R += kind == 0 ? 1 : 0;
    }
    if (R > 0) {
        if (!gen_lens) BG_FAIL(-1, "null argument: gen_lens");
        if (!limits) BG_FAIL(-1, "null argument: limits");
        if (!admit_step) BG_FAIL(-1, "null argument: admit_step");
        if (!column) BG_FAIL(-1, "null argument: column");
        if (!finish_group) BG_FAIL(-1, "null argument: finish_group");
    }
    for (int r = 0; r < R; r++) {
        if (gen_lens[r] < 0) BG_FAIL(-1, "gen_lens[%d] (%d) is negative", r, gen_lens[r]);
        if (limits[r] < gen_lens[r]) BG_FAIL(-1, "limits[%d] (%d) is below gen_lens[%d] (%d)", r, limits[r], r, gen_lens[r]);
        if (limits[r] > 0 && gen_lens[r] < 1) BG_FAIL(-1, "gen_lens[%d] is 0 under a limit of %d: a request that takes a column generates a token", r, limits[r]);
        admit_step[r] = column[r] = finish_group[r] = -1;
        if (out_lens) out_lens[r] = 0;
    }
    QueueSessionSchedule ss(max_columns, group);
    QueueSchedule &q = ss.q;
    for (int i = 0; i < n_ops; i++) {
        const int kind = ops[2 * i], arg = ops[2 * i + 1];
        if (kind == 0) { ss.submit(limits[q.known]); continue; }
        if (kind == 2) { (void)ss.cancel(arg); continue; }      // (what a session refuses -- an unknown or finished request -- changes nothing)
        ss.begin_poll([&](int r) { finish_group[r] = q.st.groups; }, [&](int r) { finish_group[r] = q.st.groups; },
                      [&](int, int r, int len) { finish_group[r] = q.st.groups; if (out_lens) out_lens[r] = len; });
        for (int n = 0; n < arg && !q.done(); n++) {
            q.refill([&](int col, int r) { admit_step[r] = q.st.steps; column[r] = col; ss.admitted(r); });
            for (int g = q.group_steps(); g > 0; g--) q.step();
            q.end_group();
            for (int col = 0; col < q.C; col++) {
                const int r = q.req[(size_t)col];
                if (!q.live[(size_t)col] || q.since[(size_t)col] < gen_lens[r]) continue;
                ss.finished(col, r, gen_lens[r]);
                finish_group[r] = q.st.groups;
                if (out_lens) out_lens[r] = gen_lens[r];
            }
        }
    }
    if (stats) *stats = q.st;
    return 0;
}

// A mode checks its own arguments between the shared checks (QueueRequests), describes itself as a QueueCall and hands both to run_queue_call.  The driver
// delivers every result as it goes, so the mode reads nothing back.
struct QueueRequests {
    const int32_t *prompts, *prompt_lens;       // concatenated
    int n_requests;
    const int32_t *n_predicts;                  // per request (or null: n_predict for every one)
    int n_predict, max_columns, group, n_batch;
    std::vector<size_t> off;                    // set by check_prompts: request r's prompt lies at prompts + off[r]
    std::vector<int32_t> cap;                   // set by run_queue_call: the tokens request r may generate (main.cpp:82 per request); 0: it never takes a unit
    // A shared prefix (biogpt_hip_generate_queue_prefix): request r is prefix ++ prompt r, the prompts are suffixes and may be empty.  pos0: the position of
    // every prompt's first token (the prefix's length; 0 without one).  n_shared, set by check_prompts: the prefix rows evaluated once and read in place, the
    // largest multiple of n_batch <= pos0 - 1 (0: nothing is shared and every launch is that of the call on the concatenations).
    const int32_t *prefix = nullptr;
    int pos0 = 0, n_shared = 0;
    int whole_len(int r) const { return pos0 + prompt_lens[r]; }
    // A session keeps every request's prompt on its own (own[r]; prompts is null and off unused) and lets prompt_lens, n_requests and cap grow
    const int32_t *const *own = nullptr;
    const int32_t *prompt(int r) const { return own ? own[r] : prompts + off[(size_t)r]; }

    // Tier one, what can be judged without the model (it fails the same way with no context and no device): check_count, the mode's column counts, check_sizes,
    // the mode's other parameters, then check_prompts, which ends the tier with the context itself.
    bool check_count() const { if (n_requests < 1) BG_FAIL(false, "n_requests must be >= 1"); return true; }
    bool check_sizes() const {
        if (group < 1 || group > 64) BG_FAIL(false, "group must be in [1, 64]");
        if (n_batch < 1) BG_FAIL(false, "n_batch must be >= 1");
        if (n_predict < 0) BG_FAIL(false, "n_predict must be >= 0");
        for (int r = 0; n_predicts && r < n_requests; r++)
            if (n_predicts[r] < 0 || n_predicts[r] > n_predict) BG_FAIL(false, "n_predicts[%d] (%d) must be in [0, n_predict = %d]", r, n_predicts[r], n_predict);
        return true;
    }
    bool check_prompts(const biogpt_hip_ctx *ctx) {
        off.assign((size_t)n_requests + 1, 0);
        for (int r = 0; r < n_requests; r++) {
            if (prefix && prompt_lens[r] < 0) BG_FAIL(false, "suffix_lens[%d] (%d) is negative", r, prompt_lens[r]);
            if (!prefix && prompt_lens[r] < 1) BG_FAIL(false, "empty prompt (request %d)", r);      // (behind a prefix no sequence is empty)
            off[(size_t)r + 1] = off[(size_t)r] + (size_t)prompt_lens[r];
        }
        for (int i = 0; i < pos0; i++)
            if (prefix[i] < 0) BG_FAIL(false, "token id %d (prefix, position %d) out of range", prefix[i], i);
        for (int r = 0; r < n_requests; r++)
            for (int i = 0; i < prompt_lens[r]; i++)
                if (prompts[off[(size_t)r] + (size_t)i] < 0) BG_FAIL(false, "token id %d (request %d, position %d) out of range", prompts[off[(size_t)r] + (size_t)i], r, i);
        n_shared = prefix ? (pos0 - 1) / n_batch * n_batch : 0;
        if (!ctx) BG_FAIL(false, "null context");
        if (!ctx->ready) BG_FAIL(false, "model has no tensors loaded (empty model): cannot evaluate");
        if (session_refuses(ctx)) return false;
        return true;
    }
    // Tier two, what needs the model's sizes: the mode's parameters, then the prompts.  Tier three, the fast chain, ends this check; what a mode still has to
    // hold against the model comes behind it.
    bool check_prompts_model(biogpt_hip_ctx *ctx, const char *what, bool wide_ok = false) const {
        const int P = ctx->hp.n_positions, V = ctx->hp.n_vocab;
        if (pos0 > P) BG_FAIL(false, "n_prefix (%d) exceeds n_positions (%d)", pos0, P);
        for (int i = 0; i < pos0; i++)
            if (prefix[i] >= V) BG_FAIL(false, "token id %d (prefix, position %d) out of range [0, %d)", prefix[i], i, V);
        for (int r = 0; r < n_requests; r++) {
            if (prefix && prompt_lens[r] > P - pos0) BG_FAIL(false, "n_prefix (%d) + suffix_lens[%d] (%d) exceeds n_positions (%d)", pos0, r, prompt_lens[r], P);
            if (prompt_lens[r] > P) BG_FAIL(false, "prompt_lens[%d] (%d) exceeds n_positions (%d)", r, prompt_lens[r], P);
            for (int i = 0; i < prompt_lens[r]; i++)
                if (prompts[off[(size_t)r] + (size_t)i] >= V) BG_FAIL(false, "token id %d (request %d, position %d) out of range [0, %d)", prompts[off[(size_t)r] + (size_t)i], r, i, V);
        }
        return check_fast_chain(ctx, what, wide_ok);
    }
};

struct QueueCall {
    int max_units = 0, per_unit = 1;                // units of the schedule, at most; columns of a unit
    const char *unit = "column", *step_name = "queue step";      // in messages
    ColumnGraphs *graphs = nullptr;                 // the mode's captured steps, valid for (units, key_b)
    int key_b = 0;
    StepForm form;                                  // the mode's selection, log-probabilities or not, shared rows or not (a queue's steps are never column-per-XCD launches)
    // what the driver writes as it goes (each may be null): the step count at which a request was admitted and its unit, the timed span, the schedule's counts
    int32_t *out_admit_step = nullptr, *out_unit = nullptr;
    double *seconds_out = nullptr;
    biogpt_hip_queue_stats *stats = nullptr;
    // prepare(units) sets these: they lie in buffers it allocates.  The admit list, on the device and pinned, with the size of a record; the header, on the
    // device and pinned, with fin[unit] != 0 in the pinned one where the unit's request has finished.
    void *admit_dev = nullptr, *admit_host = nullptr;
    size_t admit_bytes = 0;
    const void *hdr_dev = nullptr;
    void *hdr_host = nullptr;
    size_t hdr_bytes = 0;
    const int32_t *fin = nullptr;
    std::function<bool(int)> prepare;               // prepare(units): once the schedule has said how many units run -- the mode's buffers, the call's parameters and
                                                    // a start state in which no unit runs
    ColumnStep step;                                // step(t_max): the forward pass of all columns + the mode's selection and its report to the header
    std::function<void(int, int, int)> admit;       // admit(unit, r, i): entry i of the pinned admit list <- request r in `unit`
    std::function<bool(int)> enqueue_admit;         // enqueue_admit(n): the launches behind the copy of n admit records
    std::function<int(int, int)> collect;           // collect(unit, r): enqueues the copies of what request r left in `unit` (the unit is refilled behind them); the
                                                    // length the schedule retires it with, < 0: a failure
    std::function<bool()> landed;                   // (or none) behind every header wait and once behind the final synchronize: copies enqueued before the wait
                                                    // before have arrived
    // a session's (or none): after_group(g) enqueues what the look behind a group of g steps carries beside the header, in front of the header's copy;
    // looked() reads it, behind the wait and before any unit is collected
    std::function<bool(int)> after_group;
    std::function<bool()> looked;
};

// The one order of a queued call as an object that can stop between two groups: begin (the caches, the mode's buffers, the captured steps, the shared
// rows), turn (one refill, one group of steps, one look, the finished units collected), end (the stream drained, the pipeline's error word, the timed span).
// A closed call is begin, turn until the schedule is done, end (run_queue_call); a session (biogpt_hip_queue_open) runs begin at open, some turns per poll
// and end never -- its polls drain the stream themselves.  The schedule is the caller's: a session feeds it between turns.  The caller holds the call's
// scopes (XpCallScope, XcBatchScope) around whatever it runs of this.
struct QueueRun {
    biogpt_hip_ctx *ctx;
    QueueRequests &rq;
    QueueCall &qc;
    QueueSchedule &q;
    int U = 0, C = 0;
    SharedRows shared{};
    bool use_graph = false;
    std::chrono::steady_clock::time_point t0{};
    std::vector<int32_t> flat, lens, slots;

    // min_len / max_keys: the keys the first replayed step of any request sees at least / any step at most (the buckets to capture); total: the prompt
    // tokens the passes may see at once.  0; -1: the columns do not fit the model; -2: a failure
    int begin(int min_len, int max_keys, long total) {
        const int P = ctx->hp.n_positions;
        U = q.C; C = U * qc.per_unit;
        if (C > hp_cols(ctx)) BG_FAIL(-1, "max_columns (%d) exceeds the %d activation columns of this model", C, hp_cols(ctx));
        // (behind shared rows: they lie in one slot more, behind the units')
        shared = SharedRows{rq.n_shared, rq.n_shared > 0 ? C : 0};
        if (!begin_column_call(ctx, C + (shared.n > 0 ? 1 : 0), C, std::min<long>(total, P))) return -2;
        ctx->xc_batch = 0;      // the steps are always the launch chain
        if (!qc.prepare(U)) return -2;
        column_graphs_for(*qc.graphs, U, qc.key_b);
        // (ColumnKeys of a call whose first replayed step sees min_len keys and whose last one max_keys: every bucket a step here can be bounded by)
        if (!capture_column_steps(ctx, *qc.graphs, qc.form, ColumnKeys{min_len - 1, 1, P}, max_keys - min_len + 2, qc.step, &use_graph)) return -2;
        t0 = std::chrono::steady_clock::now();
        if (shared.n > 0) {      // the shared rows, once: the prompt columns of one sequence in the slot behind the units'
            const int32_t n = shared.n;
            if (!pack_column_passes(ctx, rq.prefix, &n, 1, rq.n_batch, [&](int n_cols, int t_max, size_t) { return enqueue_forward(ctx, ForwardPass::packed_prompts(n_cols, t_max)); },
                                    1, shared.slot))
                return -2;
            q.st.prompt_columns += n;
        }
        return 0;
    }

    // one refill, one group, one look.  0, or -2: a failure
    int turn() {
        const int P = ctx->hp.n_positions;
        const std::vector<int32_t> &cap = rq.cap;
        // ---- refill: the prompts of the admitted requests into the (first) slots of exactly their units, then the admit list and the mode's launches behind it ----
        flat.clear(); lens.clear(); slots.clear();
        const int n_admit = q.refill([&](int unit, int r) {
            const int32_t *p = rq.prompt(r);
            const int own = rq.pos0 - shared.n, len = own + rq.prompt_lens[r];      // behind a prefix: its rows that are not shared, then the suffix (never empty)
            qc.admit(unit, r, (int)slots.size());
            if (own > 0) flat.insert(flat.end(), rq.prefix + shared.n, rq.prefix + rq.pos0);
            flat.insert(flat.end(), p, p + rq.prompt_lens[r]); lens.push_back(len); slots.push_back(unit * qc.per_unit);
            if (qc.out_admit_step) qc.out_admit_step[r] = q.st.steps;
            if (qc.out_unit) qc.out_unit[r] = unit;
            q.st.prompt_columns += len;
        });
        if (n_admit > 0) {
            if (!pack_column_passes(ctx, flat.data(), lens.data(), n_admit, rq.n_batch,
                                    [&](int n_cols, int t_max, size_t) {
                                        return enqueue_forward(ctx, shared.n > 0 ? ForwardPass::packed_continuations(n_cols, t_max, n_cols) : ForwardPass::packed_prompts(n_cols, t_max));
                                    },
                                    1, 0, shared, slots.data()))
                return -2;
            HIP_TRY(-2, hipMemcpyAsync(qc.admit_dev, qc.admit_host, qc.admit_bytes * (size_t)n_admit, hipMemcpyHostToDevice, ctx->stream));
            if (!qc.enqueue_admit(n_admit)) return -2;
        }
        // ---- one group of steps ----
        const int n_steps = q.group_steps();
        for (int g = n_steps; g > 0; g--) {
            int t_max = 1;
            for (int unit = 0; unit < U; unit++)
                if (q.req[(size_t)unit] >= 0) t_max = std::max(t_max, q.position(unit, rq.whole_len(q.req[(size_t)unit])) + 1);
            t_max = std::min(t_max, P);
            if (use_graph) {
                hipGraphExec_t ge = qc.graphs->exec[ColumnGraphs::slot(qc.form, graph_bucket(t_max))];
                if (!ge) BG_FAIL(-2, "internal: no captured %s for %d keys", qc.step_name, t_max);
                HIP_TRY(-2, hipGraphLaunch(ge, ctx->stream));
            } else if (!qc.step(t_max)) {
                return -2;
            }
            q.step();
        }
        q.end_group();
        if (qc.after_group && !qc.after_group(n_steps)) return -2;
        // ---- the look at the units: the header behind the group (lag 0) ----
        HIP_TRY(-2, hipMemcpyAsync(qc.hdr_host, qc.hdr_dev, qc.hdr_bytes, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(-2, hipEventRecord(ctx->live_ev[0], ctx->stream));
        HIP_TRY(-2, hipEventSynchronize(ctx->live_ev[0]));
        // (the copies of the look before stand in front of this header in the stream: they have arrived)
        if (qc.landed && !qc.landed()) return -2;
        if (qc.looked && !qc.looked()) return -2;
        for (int unit = 0; unit < U; unit++) {
            if (!q.live[(size_t)unit]) continue;
            const int r = q.req[(size_t)unit];
            if (!qc.fin[unit]) {
                if (q.since[(size_t)unit] >= cap[(size_t)r])
                    BG_FAIL(-2, "internal: request %d (%s %d) is unfinished after %d steps, its limit is %d", r, qc.unit, unit, q.since[(size_t)unit], cap[(size_t)r]);
                continue;
            }
            const int len = qc.collect(unit, r);      // in stream order before the unit is reused; a session's collect retires the unit itself
            if (len < 0) return -2;
            if (q.live[(size_t)unit]) q.retire(unit, len);
        }
        return 0;
    }

    // the stream drained; what the caller asked for of the timed span and the counts
    int end() {
        HIP_TRY(-2, hipStreamSynchronize(ctx->stream));
        const auto t1 = std::chrono::steady_clock::now();
        if (qc.landed && !qc.landed()) return -2;
        if (!xpipe_check(ctx)) return -2;
        if (qc.seconds_out) *qc.seconds_out = std::chrono::duration<double>(t1 - t0).count();
        if (qc.stats) *qc.stats = q.st;
        return 0;
    }
};

// A closed call, for requests that passed their checks: the run driven to its end.  Returns 0 once every request has been served and the stream has drained,
// or at once where no request may generate a token (nothing was touched); -1: the columns do not fit the model; -2: a failure.
static int run_queue_call(biogpt_hip_ctx *ctx, QueueRequests &rq, QueueCall &qc) {
    const int P = ctx->hp.n_positions, R = rq.n_requests;
    // every request's own clamp; the buckets the steps can need
    rq.cap.assign((size_t)R, 0);
    int min_len = P, max_keys = 0;
    long total = 0;
    for (int r = 0; r < R; r++) {
        rq.cap[(size_t)r] = std::min(rq.n_predicts ? rq.n_predicts[r] : rq.n_predict, P - rq.whole_len(r));
        if (rq.cap[(size_t)r] <= 0) continue;
        min_len = std::min(min_len, rq.whole_len(r)); max_keys = std::max(max_keys, rq.whole_len(r) + rq.cap[(size_t)r]);
        total += rq.whole_len(r);
    }
    if (qc.out_admit_step) std::fill(qc.out_admit_step, qc.out_admit_step + R, -1);
    if (qc.out_unit) std::fill(qc.out_unit, qc.out_unit + R, -1);
    if (qc.seconds_out) *qc.seconds_out = 0.0;
    QueueSchedule q(rq.cap, qc.max_units, rq.group);
    if (qc.stats) *qc.stats = q.st;
    if (q.C == 0) return 0;      // nobody has room for a token: nothing was touched
    if (q.C * qc.per_unit > hp_cols(ctx)) BG_FAIL(-1, "max_columns (%d) exceeds the %d activation columns of this model", q.C * qc.per_unit, hp_cols(ctx));

    XpCallScope xp_scope(ctx);
    XcBatchScope xc_scope{ctx};
    QueueRun run{ctx, rq, qc, q};
    if (const int rc = run.begin(min_len, max_keys, total)) return rc;
    while (!q.done())
        if (const int rc = run.turn()) return rc;
    return run.end();
}

// ---- generation over a queue: a unit is a column; sampling with each request's own generator (kernels_queue.hip.h) ------------------------------------
struct QueueBufs {
    bgk::SampleCtl *ctl;
    bgk::SampleSeq *seq;        // [QUEUE_COLS]
    int32_t *limit;             // [QUEUE_COLS]
    bgk::QueueHdr *hdr;
    bgk::QueueAdmit *admit;     // [QUEUE_COLS]
    size_t bytes;
};
static QueueBufs queue_bufs_at(uint8_t *base) {
    ByteLayout l;
    QueueBufs b{};
    b.ctl = l.take<bgk::SampleCtl>(base, 1); b.seq = l.take<bgk::SampleSeq>(base, bgk::QUEUE_COLS); b.limit = l.take<int32_t>(base, bgk::QUEUE_COLS);
    b.hdr = l.take<bgk::QueueHdr>(base, 1); b.admit = l.take<bgk::QueueAdmit>(base, bgk::QUEUE_COLS);
    b.bytes = l.bytes();
    return b;
}
// the pinned twin: the header as the host reads it, the admit list as the host writes it
struct QueueHost { bgk::QueueHdr hdr; bgk::QueueAdmit admit[bgk::QUEUE_COLS]; };

// What request r left in column col, len tokens, to the caller's rows (in stream order before the column is reused): the ids straight from the column's seq_gen
// row, and with lp the column's rows of the log-probability block (lp_stride entries apart)
static bool queue_copy_out(biogpt_hip_ctx *ctx, int col, int r, int len, int n_predict, int32_t *out_ids, const biogpt_hip_gen_logprobs *lp, const GenLpBufs &lb,
                           int lp_stride) {
    if (len <= 0) return true;
    const size_t K = lp ? (size_t)lp->n_top : 0;
    HIP_TRY(false, hipMemcpyAsync(out_ids + (size_t)r * (size_t)n_predict, ctx->seq_gen + (size_t)col * ctx->hp.n_positions, (size_t)len * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (lp) {
        const size_t src = (size_t)col * (size_t)lp_stride, dst = (size_t)r * (size_t)n_predict;
        HIP_TRY(false, hipMemcpyAsync(lp->lp + dst, lb.lp + src, (size_t)len * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (K > 0) {
            HIP_TRY(false, hipMemcpyAsync(lp->top_ids + dst * K, lb.top_ids + src * K, (size_t)len * K * 4, hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(false, hipMemcpyAsync(lp->top_lp + dst * K, lb.top_lp + src * K, (size_t)len * K * 4, hipMemcpyDeviceToHost, ctx->stream));
        }
    }
    return true;
}

// ---- the column queue: what its two modes share ---------------------------------------------------------------------------------------------------------
// The arguments both entry points have.  prefix != null: request r is prefix ++ prompt r, the prompts are suffixes and may be empty; the first n_shared prefix
// rows are evaluated once, into the slot behind the columns', and read there by the refill passes and the steps (n_shared == 0: the call on the
// concatenations, launch for launch).  lp != null: the selection also writes log-probabilities, and a finished column's rows of the log-probability block go to
// its request's rows of lp's arrays, in stream order before the column is reused.
struct ColumnQueueArgs {
    const int32_t *prefix; int32_t n_prefix;
    const int32_t *prompts, *prompt_lens, *n_predicts;
    int32_t n_requests, n_predict, max_columns, group, n_batch;
    const uint32_t *seeds;
    int32_t *out_ids, *out_lens, *out_admit_step, *out_column;
    double *seconds_out; biogpt_hip_queue_stats *stats; const biogpt_hip_gen_logprobs *lp;
};
// What differs between the modes: the closed queue (one sampler for all requests) and the queue whose requests carry their own parameters
struct ColumnQueueMode {
    ColumnGraphs biogpt_hip_ctx::*graphs = nullptr;
    const char *what = nullptr;              // the mode by name, at the gate of the fast chain
    bool wide_ok = false;                    // the wide chain serves it
    const void *own_arg = nullptr;           // (or none, with its name) a pointer argument of the mode's own, named in a message between prompt_lens and seeds
    const char *own_arg_name = nullptr;
    int32_t *out_finish = nullptr;           // (or null) [n_requests]: -1 for a request that never ran, otherwise what `collected` writes
    std::function<bool(int, int)> check;     // check(V, P): the mode's parameters without the model (V < 0), then with its sizes
    std::function<bool(QueueCall &)> prepare;      // the mode's block on the device and its pinned twin: the QueueCall's admit list, with the size of an entry, and
                                                   // header, and `hdr` below; the call's parameters go up and nobody runs yet
    std::function<void()> select;            // the selection launch behind the forward pass
    std::function<void(int, int, const bgk::QueueAdmit &, const int32_t *)> admit;      // admit(i, r, a, own): entry i of the pinned admit list <- the record a and
                                                                                        // what the mode adds for request r, whose own tokens are `own`
    std::function<bool(int)> enqueue_admit;  // enqueue_admit(n): the admit kernel over n entries
    std::function<void(int, int)> collected; // (or none) collected(col, r): what the mode reads of finished column col beyond its length
    // what generate_column_queue has settled by the time one of these runs: the columns, the model's sizes, the shared rows, with lp the block the selection writes
    int C = 0, P = 0, V = 0, n_shared = 0;
    GenLpBufs lb{};
    const bgk::QueueHdr *hdr = nullptr;      // the pinned header, whose fin and len the driver reads
};

// Each of the four forms of a mode -- plain, shared rows, log-probabilities, both -- has its own captured steps (never column-per-XCD launches).
static int generate_column_queue(biogpt_hip_ctx *ctx, const ColumnQueueArgs &a, ColumnQueueMode &m) {
    clear_error();
    const biogpt_hip_gen_logprobs *const lp = a.lp;
    const int32_t *const prefix = a.prefix;
    const int32_t n_prefix = a.n_prefix, n_requests = a.n_requests, n_predict = a.n_predict, max_columns = a.max_columns;
    if (lp && !check_gen_logprobs(lp, -1)) return -1;
    if (!prefix && n_prefix != 0) BG_FAIL(-1, "n_prefix must be 0 without a prefix (got %d)", n_prefix);
    if (prefix && n_prefix < 1) BG_FAIL(-1, "n_prefix must be >= 1 (got %d)", n_prefix);
    if (!a.prompts) BG_FAIL(-1, prefix ? "null argument: suffixes" : "null argument: prompts");
    if (!a.prompt_lens) BG_FAIL(-1, prefix ? "null argument: suffix_lens" : "null argument: prompt_lens");
    if (m.own_arg_name && !m.own_arg) BG_FAIL(-1, "null argument: %s", m.own_arg_name);
    if (!a.seeds) BG_FAIL(-1, "null argument: seeds");
    if (!a.out_ids) BG_FAIL(-1, "null argument: out_ids");
    if (!a.out_lens) BG_FAIL(-1, "null argument: out_lens");
    QueueRequests rq{a.prompts, a.prompt_lens, n_requests, a.n_predicts, n_predict, max_columns, a.group, a.n_batch};
    rq.prefix = prefix; rq.pos0 = n_prefix;
    if (!rq.check_count()) return -1;
    if (prefix && (max_columns < 1 || max_columns > bgk::QUEUE_COLS - 1))
        BG_FAIL(-1, "max_columns must be in [1, %d] behind a prefix (got %d)", bgk::QUEUE_COLS - 1, max_columns);   // one slot holds the prefix
    if (max_columns < 1 || max_columns > bgk::QUEUE_COLS) BG_FAIL(-1, "max_columns must be in [1, %d]", bgk::QUEUE_COLS);
    if (!rq.check_sizes()) return -1;
    if (!m.check(-1, -1)) return -1;
    if (!rq.check_prompts(ctx)) return -1;
    const int P = m.P = ctx->hp.n_positions, V = m.V = ctx->hp.n_vocab;
    if (!m.check(V, P)) return -1;
    if (lp && lp->n_top > V) BG_FAIL(-1, "logprobs.n_top (%d) exceeds n_vocab (%d)", lp->n_top, V);
    if (!rq.check_prompts_model(ctx, m.what, m.wide_ok)) return -1;
    const size_t n_out = (size_t)n_requests * (size_t)n_predict, K = lp ? (size_t)lp->n_top : 0;
    std::fill(a.out_ids, a.out_ids + n_out, -1);
    std::fill(a.out_lens, a.out_lens + n_requests, 0);
    if (m.out_finish) std::fill(m.out_finish, m.out_finish + n_requests, -1);
    if (lp) {      // entries at or past a request's length, and those of a request that never takes a column, as genlp_read leaves them
        std::fill(lp->lp, lp->lp + n_out, 0.0f);
        if (K > 0) { std::fill(lp->top_ids, lp->top_ids + n_out * K, -1); std::fill(lp->top_lp, lp->top_lp + n_out * K, 0.0f); }
    }

    // a column's entries lie lp_stride apart in the block: no request generates n_positions tokens, so the block's rows hold any n_predict
    const int n_shared = m.n_shared = rq.n_shared, lp_stride = std::min(n_predict, P);
    biogpt_hip_queue_stats ran{};
    QueueCall qc;
    qc.max_units = max_columns;
    qc.graphs = &(ctx->*m.graphs); qc.form.lp = lp != nullptr; qc.form.shared = n_shared > 0;
    qc.out_admit_step = a.out_admit_step; qc.out_unit = a.out_column; qc.seconds_out = a.seconds_out; qc.stats = &ran;
    qc.prepare = [&](int units) -> bool {
        m.C = units;
        if (lp && (!genlp_prepare(ctx, &m.lb) || !genlp_upload(m.lb, lp->n_top, lp_stride))) return false;
        if (!m.prepare(qc)) return false;
        qc.fin = m.hdr->fin;
        return true;
    };
    qc.step = [&](int t_max) -> bool {      // (behind shared rows always in place: a queue never runs the column-per-XCD launches)
        if (!enqueue_forward(ctx, n_shared > 0 ? ForwardPass::decode_step_shared(m.C, t_max, n_shared) : ForwardPass::decode_step(m.C, t_max))) return false;
        m.select();
        HIP_TRY(false, hipGetLastError());
        return true;
    };
    qc.admit = [&](int col, int r, int i) {      // the state of the whole sequence at its last token: the suffix's, or the prefix's behind an empty one
        const int len = a.prompt_lens[r];
        const int32_t *const own = a.prompts + rq.off[(size_t)r];
        bgk::QueueAdmit rec{};
        rec.col = col; rec.last_token = len > 0 ? own[len - 1] : prefix[n_prefix - 1]; rec.len = rq.whole_len(r);
        rec.limit = rq.cap[(size_t)r]; rec.seed = a.seeds[r];
        rec.n_shared = n_shared; rec.shared_slot = n_shared > 0 ? m.C : 0;
        m.admit(i, r, rec, own);
    };
    qc.enqueue_admit = m.enqueue_admit;
    qc.collect = [&](int col, int r) -> int {      // the ids straight from the column's seq_gen row to the caller's row
        const int len = std::max(0, std::min(m.hdr->len[col], rq.cap[(size_t)r]));
        if (!queue_copy_out(ctx, col, r, len, n_predict, a.out_ids, lp, m.lb, lp_stride)) return -1;
        a.out_lens[r] = len;
        if (m.collected) m.collected(col, r);
        return len;
    };
    const int rc = run_queue_call(ctx, rq, qc);
    if (a.stats) *a.stats = ran;
    // (a call that failed, or in which no request had room for a token, leaves the stats of the last call that generated)
    if (rc == 0 && prefix && ran.columns > 0) {
        ctx->prefix_stats[0] = n_shared; ctx->prefix_stats[1] = ran.prompt_columns; ctx->prefix_stats[2] = 0; ctx->prefix_stats[3] = ran.columns;
    }
    return rc;
}

// The closed queue: top_k, top_p, temp and eos_id are the call's; queue_rows_kernel is the selection, with lp queue_rows_lp_kernel.  The plain form alone is
// open to the wide chain.
static int generate_queue_once(biogpt_hip_ctx *ctx, const ColumnQueueArgs &a, int32_t top_k, double top_p, double temp, int32_t eos_id) {
    QueueBufs qb{};
    QueueHost *qh = nullptr;
    ColumnQueueMode m;
    m.graphs = &biogpt_hip_ctx::graphs_queue;
    m.what = a.prefix ? "generation over a queue behind a shared prefix" : a.lp ? "generation over a queue with log-probabilities" : "generation over a queue";
    m.wide_ok = !a.prefix && !a.lp;
    m.check = [&](int V, int) -> bool { return check_sample_values(top_k, top_p, temp, eos_id, V); };
    m.prepare = [&](QueueCall &qc) -> bool {
        if (!ctx->queue_buf) HIP_TRY(false, hipMalloc(&ctx->queue_buf, queue_bufs_at(nullptr).bytes));
        if (!ctx->queue_host) HIP_TRY(false, hipHostMalloc(&ctx->queue_host, sizeof(QueueHost)));
        qb = queue_bufs_at(ctx->queue_buf);
        qh = reinterpret_cast<QueueHost *>(ctx->queue_host);
        qc.admit_dev = qb.admit; qc.admit_host = qh->admit; qc.admit_bytes = sizeof(bgk::QueueAdmit);
        qc.hdr_dev = qb.hdr; qc.hdr_host = &qh->hdr; qc.hdr_bytes = sizeof(bgk::QueueHdr); m.hdr = &qh->hdr;
        // the call's parameters; nobody runs yet
        const bgk::SampleCtl hc = sample_ctl_of(top_k, eos_id, 0, top_p, temp);
        HIP_TRY(false, hipMemcpy(qb.ctl, &hc, sizeof(hc), hipMemcpyHostToDevice));
        HIP_TRY(false, hipMemset(qb.hdr, 0, sizeof(bgk::QueueHdr)));
        return true;
    };
    m.select = [&] {
        if (a.lp)
            hipLaunchKernelGGL(bgk::queue_rows_lp_kernel, dim3(m.C), dim3(bgk::SAMPLE_THREADS), 0, ctx->stream, ctx->logits_all, m.V, m.V, qb.ctl, qb.seq, ctx->seq, ctx->seq_gen,
                               m.P, qb.limit, qb.hdr, m.lb.out());
        else
            hipLaunchKernelGGL(bgk::queue_rows_kernel, dim3(m.C), dim3(bgk::SAMPLE_THREADS), 0, ctx->stream, ctx->logits_all, m.V, m.V, qb.ctl, qb.seq, ctx->seq, ctx->seq_gen, m.P,
                               qb.limit, qb.hdr);
    };
    m.admit = [&](int i, int, const bgk::QueueAdmit &rec, const int32_t *) { qh->admit[i] = rec; };
    m.enqueue_admit = [&](int n_admit) -> bool {
        hipLaunchKernelGGL(bgk::queue_admit_kernel, dim3(n_admit), dim3(bgk::QUEUE_ADMIT_THREADS), 0, ctx->stream, qb.admit, qb.seq, ctx->seq, qb.limit, qb.hdr);
        HIP_TRY(false, hipGetLastError());
        return true;
    };
    return generate_column_queue(ctx, a, m);
}

int biogpt_hip_generate_queue(biogpt_hip_ctx *ctx, const int32_t *prompts, const int32_t *prompt_lens, int32_t n_requests, const int32_t *n_predicts,
                              int32_t n_predict, int32_t max_columns, int32_t group, int32_t n_batch, int32_t top_k, double top_p, double temp,
                              const uint32_t *seeds, int32_t eos_id, int32_t *out_ids, int32_t *out_lens, int32_t *out_admit_step, int32_t *out_column,
                              double *seconds_out, biogpt_hip_queue_stats *stats) {
    return biogpt_hip_generate_queue_prefix(ctx, nullptr, 0, prompts, prompt_lens, n_requests, n_predicts, n_predict, max_columns, group, n_batch, top_k, top_p, temp, seeds,
                                            eos_id, out_ids, out_lens, out_admit_step, out_column, seconds_out, stats, nullptr);
}

// biogpt_hip_generate_queue of the requests prefix ++ suffix r behind the shared prefix rows (prefix == null: of the suffixes themselves), with the
// log-probabilities of the generated tokens where asked
int biogpt_hip_generate_queue_prefix(biogpt_hip_ctx *ctx, const int32_t *prefix, int32_t n_prefix, const int32_t *suffixes, const int32_t *suffix_lens, int32_t n_requests,
                                     const int32_t *n_predicts, int32_t n_predict, int32_t max_columns, int32_t group, int32_t n_batch, int32_t top_k, double top_p,
                                     double temp, const uint32_t *seeds, int32_t eos_id, int32_t *out_ids, int32_t *out_lens, int32_t *out_admit_step,
                                     int32_t *out_column, double *seconds_out, biogpt_hip_queue_stats *stats, const biogpt_hip_gen_logprobs *logprobs) {
    const ColumnQueueArgs a{prefix, n_prefix, suffixes, suffix_lens, n_predicts, n_requests, n_predict, max_columns, group, n_batch, seeds,
                            out_ids, out_lens, out_admit_step, out_column, seconds_out, stats, logprobs};
    return with_xpipe_retry(ctx, 0, [&] { return generate_queue_once(ctx, a, top_k, top_p, temp, eos_id); });
}

// ---- generation over a queue whose requests carry their own parameters (biogpt_hip_generate_queue_requests) ---------------------------------------------
// The second mode of the column queue (generate_column_queue): the driver, the schedule and the admit state are the closed queue's; the step is the forward
// pass and ONE launch of queue_req_rows_kernel (the closed rules call has two), which reads a column's sampler, EOS id, rules and stop sequences from the column's record.
// An entry of the admit list is the admit record, the request's record and the request's own prompt tokens (the history its rules read), `stride` bytes apart:
// one upload per refill, as before, and a step causes no host traffic.  Behind a prefix the prefix's tokens go up once, in prepare.  The header carries the
// reason a column finished behind what the driver reads.  Its captured steps are graphs_queue_req, with the four forms of the closed queue.
struct QueueReqBufs {
    bgk::SampleSeq *seq;        // [QUEUE_COLS]
    int32_t *limit;             // [QUEUE_COLS]
    bgk::QueueReqHdr *hdr;
    uint8_t *stream;            // what queue_stream_kernel writes for a streaming session, at its largest (queue_stream_at): it lies right behind the header
                                // and travels with it in one copy
    bgk::QueueReqRec *rec;      // [QUEUE_COLS]
    int32_t *prefix;            // [n_positions]
    int32_t *hist;              // [QUEUE_COLS][n_positions]
    uint8_t *admit;             // QUEUE_COLS entries at their largest
    size_t bytes;
};
static_assert(sizeof(biogpt_hip_request_params) == 72 && offsetof(biogpt_hip_request_params, rules) == 24 && offsetof(biogpt_hip_request_params, stop) == 56,
              "biogpt_hip_request_params as the bindings lay it out (RequestParams, biogpt.cpp_amd/__init__.py)");
static size_t queue_req_stride(int n_own) { return (sizeof(bgk::QueueReqAdmit) + (size_t)n_own * 4 + 15) & ~(size_t)15; }
// The block of a streaming session for C columns, windows of g entries and K alternatives (K < 0: no log-probabilities), on the device or in the pinned look
struct QueueStreamBufs { bgk::QueueStreamOut out; size_t bytes; };
static QueueStreamBufs queue_stream_at(uint8_t *base, int C, int g, int K) {
    ByteLayout l;
    QueueStreamBufs b{};
    const size_t n = (size_t)C * (size_t)g;
    b.out.n_gen = l.take<int32_t>(base, (size_t)C); b.out.ids = l.take<int32_t>(base, n);
    if (K >= 0) { b.out.lp = l.take<float>(base, n); b.out.top_ids = l.take<int32_t>(base, n * (size_t)K); b.out.top_lp = l.take<float>(base, n * (size_t)K); }
    b.bytes = l.bytes();
    return b;
}
static_assert(sizeof(bgk::QueueReqHdr) % 16 == 0, "the stream block begins where the header ends");
static QueueReqBufs queue_req_bufs_at(uint8_t *base, int P) {
    ByteLayout l;
    QueueReqBufs b{};
    b.seq = l.take<bgk::SampleSeq>(base, bgk::QUEUE_COLS); b.limit = l.take<int32_t>(base, bgk::QUEUE_COLS); b.hdr = l.take<bgk::QueueReqHdr>(base, 1);
    b.stream = l.take<uint8_t>(base, queue_stream_at(nullptr, bgk::QUEUE_COLS, 64, bgk::GENLP_MAX_TOP).bytes);
    b.rec = l.take<bgk::QueueReqRec>(base, bgk::QUEUE_COLS); b.prefix = l.take<int32_t>(base, (size_t)P); b.hist = l.take<int32_t>(base, (size_t)bgk::QUEUE_COLS * P);
    b.admit = l.take<uint8_t>(base, (size_t)bgk::QUEUE_COLS * queue_req_stride(P));
    b.bytes = l.bytes();
    return b;
}

// What can be judged of request r's parameters without the model (V < 0), and with its sizes
static bool check_request_params(const biogpt_hip_request_params &p, int r, int V, int P) {
    if (!check_sample_values(p.top_k, p.top_p, p.temp, p.eos_id, V, "params[%d].", r)) return false;
    if (!check_rules(&p.rules, V >= 0 ? V : bgk::RULES_MAX_VOCAB, V >= 0 ? P : -1)) {
        const std::string why = last_error();
        BG_FAIL(false, "params[%d].rules: %s", r, why.c_str());
    }
    if (p.rules.n_suppress > bgk::QUEUE_REQ_SUPPRESS) BG_FAIL(false, "params[%d].rules.n_suppress (%d) must be in [0, %d] for a request of a queue", r, p.rules.n_suppress, bgk::QUEUE_REQ_SUPPRESS);
    if (p.n_stop < 0 || p.n_stop > bgk::QUEUE_REQ_STOPS) BG_FAIL(false, "params[%d].n_stop (%d) must be in [0, %d]", r, p.n_stop, bgk::QUEUE_REQ_STOPS);
    if (p.n_stop > 0 && !p.stop) BG_FAIL(false, "params[%d].stop is NULL with n_stop = %d", r, p.n_stop);
    if (p.n_stop > 0 && !p.stop_lens) BG_FAIL(false, "params[%d].stop_lens is NULL with n_stop = %d", r, p.n_stop);
    for (int i = 0, at = 0; i < p.n_stop; at += p.stop_lens[i], i++) {
        if (p.stop_lens[i] < 1 || p.stop_lens[i] > bgk::QUEUE_REQ_STOP_LEN)
            BG_FAIL(false, "params[%d].stop_lens[%d] (%d) must be in [1, %d]", r, i, p.stop_lens[i], bgk::QUEUE_REQ_STOP_LEN);
        for (int j = 0; j < p.stop_lens[i]; j++) {
            const int t = p.stop[at + j];
            if (t < 0 || (V >= 0 && t >= V)) BG_FAIL(false, "params[%d].stop: token id %d (sequence %d, position %d) out of range%s", r, t, i, j, V >= 0 ? " for this vocabulary" : "");
        }
    }
    return true;
}

static bgk::QueueReqRec request_rec_of(const biogpt_hip_request_params &p, int n_prefix, int n_own) {
    bgk::QueueReqRec rec{};
    rec.ctl = sample_ctl_of(p.top_k, p.eos_id, 0, p.top_p, p.temp);
    const bgk::RulesCtl rc = rules_ctl_of(&p.rules, 0, p.eos_id);
    rec.penalty = rc.penalty; rec.ngram = rc.ngram; rec.min_new = rc.min_new; rec.n_suppress = rc.n_suppress;
    rec.rules_on = rules_active(&p.rules, p.eos_id) ? 1 : 0;
    rec.n_prefix = n_prefix; rec.n_own = n_own; rec.n_stop = p.n_stop;
    for (int i = 0; i < rc.n_suppress; i++) rec.suppress[i] = rc.suppress[i];
    for (int i = 0, at = 0; i < p.n_stop; at += p.stop_lens[i], i++) {
        rec.stop_len[i] = p.stop_lens[i];
        for (int j = 0; j < p.stop_lens[i]; j++) rec.stop[i][j] = p.stop[at + j];
    }
    return rec;
}

static void enqueue_queue_req_rows(hipStream_t stream, int C, float *logits, int V, const QueueReqBufs &qb, bgk::SeqState *seq, int32_t *seq_gen,
                                   int gen_stride, int hist_stride, const GenLpBufs *lb) {
    const size_t lds = (size_t)((V + 31) / 32) * 4;
    if (lb)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(bgk::queue_req_rows_kernel<bgk::SampleGenLp>), dim3(C), dim3(bgk::SAMPLE_THREADS), lds, stream, logits, V, V, qb.rec, qb.seq, seq,
                           seq_gen, gen_stride, qb.limit, qb.hdr, qb.prefix, qb.hist, hist_stride, bgk::SampleGenLp{lb->out()});
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(bgk::queue_req_rows_kernel<bgk::SamplePlain>), dim3(C), dim3(bgk::SAMPLE_THREADS), lds, stream, logits, V, V, qb.rec, qb.seq, seq,
                           seq_gen, gen_stride, qb.limit, qb.hdr, qb.prefix, qb.hist, hist_stride, bgk::SamplePlain());
}

// every request's parameters, without the model (V < 0) and with its sizes; with_lp: no request may then have a rule switched on
static bool check_requests(const biogpt_hip_request_params *params, int n_requests, bool with_lp, int V, int P) {
    for (int r = 0; r < n_requests; r++) {
        if (!check_request_params(params[r], r, V, P)) return false;
        if (V < 0 && with_lp && rules_active(&params[r].rules, params[r].eos_id))
            BG_FAIL(false, "logprobs with generation rules (params[%d].rules has a rule switched on): no closed call returns log-probabilities under rules", r);
    }
    return true;
}

static int generate_queue_requests_once(biogpt_hip_ctx *ctx, const ColumnQueueArgs &a, const biogpt_hip_request_params *params, int32_t *out_finish) {
    QueueReqBufs qb{};
    bgk::QueueReqHdr *hh = nullptr;      // pinned: the header, then the admit list
    uint8_t *admit_host = nullptr;
    size_t stride = 0;
    ColumnQueueMode m;
    m.graphs = &biogpt_hip_ctx::graphs_queue_req;
    m.what = "generation over a queue with request parameters";
    m.own_arg = params; m.own_arg_name = "params";
    m.out_finish = out_finish;
    m.check = [&](int V, int P) -> bool { return check_requests(params, a.n_requests, a.lp != nullptr, V, P); };
    m.prepare = [&](QueueCall &qc) -> bool {
        const int P = m.P;
        int most_own = 0;
        for (int r = 0; r < a.n_requests; r++) most_own = std::max(most_own, a.prompt_lens[r]);
        stride = queue_req_stride(most_own);      // (most_own <= n_positions: check_prompts_model)
        if (!ctx->queue_req_buf) HIP_TRY(false, hipMalloc(&ctx->queue_req_buf, queue_req_bufs_at(nullptr, P).bytes));
        if (!ctx->queue_req_host) HIP_TRY(false, hipHostMalloc(&ctx->queue_req_host, sizeof(bgk::QueueReqHdr) + (size_t)bgk::QUEUE_COLS * queue_req_stride(P)));
        qb = queue_req_bufs_at(ctx->queue_req_buf, P);
        hh = reinterpret_cast<bgk::QueueReqHdr *>(ctx->queue_req_host);
        admit_host = ctx->queue_req_host + sizeof(bgk::QueueReqHdr);
        qc.admit_dev = qb.admit; qc.admit_host = admit_host; qc.admit_bytes = stride;
        qc.hdr_dev = qb.hdr; qc.hdr_host = hh; qc.hdr_bytes = sizeof(bgk::QueueReqHdr); m.hdr = &hh->q;
        // the prefix the rules read; nobody runs yet
        if (a.prefix) HIP_TRY(false, hipMemcpy(qb.prefix, a.prefix, (size_t)a.n_prefix * 4, hipMemcpyHostToDevice));
        HIP_TRY(false, hipMemset(qb.hdr, 0, sizeof(bgk::QueueReqHdr)));
        return true;
    };
    m.select = [&] { enqueue_queue_req_rows(ctx->stream, m.C, ctx->logits_all, m.V, qb, ctx->seq, ctx->seq_gen, m.P, m.P, a.lp ? &m.lb : nullptr); };
    m.admit = [&](int i, int r, const bgk::QueueAdmit &rec, const int32_t *own) {
        bgk::QueueReqAdmit *e = reinterpret_cast<bgk::QueueReqAdmit *>(admit_host + (size_t)i * stride);
        e->a = rec;
        e->rec = request_rec_of(params[r], a.n_prefix, a.prompt_lens[r]);
        std::memcpy(e + 1, own, (size_t)a.prompt_lens[r] * 4);
    };
    m.enqueue_admit = [&](int n_admit) -> bool {
        hipLaunchKernelGGL(bgk::queue_req_admit_kernel, dim3(n_admit), dim3(bgk::QUEUE_ADMIT_THREADS), 0, ctx->stream, qb.admit, (int)stride, qb.seq, ctx->seq, qb.limit, qb.hdr,
                           qb.rec, qb.hist, m.P);
        HIP_TRY(false, hipGetLastError());
        return true;
    };
    m.collected = [&](int col, int r) { if (out_finish) out_finish[r] = hh->reason[col]; };
    return generate_column_queue(ctx, a, m);
}

int biogpt_hip_generate_queue_requests(biogpt_hip_ctx *ctx, const int32_t *prefix, int32_t n_prefix, const int32_t *prompts, const int32_t *prompt_lens, int32_t n_requests,
                                       const int32_t *n_predicts, int32_t n_predict, int32_t max_columns, int32_t group, int32_t n_batch,
                                       const biogpt_hip_request_params *params, const uint32_t *seeds, int32_t *out_ids, int32_t *out_lens, int32_t *out_finish,
                                       int32_t *out_admit_step, int32_t *out_column, double *seconds_out, biogpt_hip_queue_stats *stats,
                                       const biogpt_hip_gen_logprobs *logprobs) {
    const ColumnQueueArgs a{prefix, n_prefix, prompts, prompt_lens, n_predicts, n_requests, n_predict, max_columns, group, n_batch, seeds,
                            out_ids, out_lens, out_admit_step, out_column, seconds_out, stats, logprobs};
    return with_xpipe_retry(ctx, 0, [&] { return generate_queue_requests_once(ctx, a, params, out_finish); });
}

// ---- queue sessions: submit, poll, stream and cancel while steps run (biogpt_hip_queue_open) -------------------------------------------------------------
// biogpt_hip_generate_queue_requests turned inside out: the run (QueueRun) is begun at open and its columns, K / V slots and captured steps persist; a poll is
// some turns of it; the schedule (QueueSessionSchedule) is fed between polls.  The steps, the admit kernel, the records and the device block are those of the
// closed call (graphs_queue_req, queue_req_bufs_at), so a session and closed calls of the same shape share their captured steps.  What a session adds:
//   the look    the pinned header of its own, with the stream block behind it where streaming is on: queue_stream_kernel runs behind every group and the block
//               travels in the header's copy.  The host keeps, per request, how many tokens it has delivered, and takes the part of the window beyond.
//   cancel      a running request: its column goes into a small pinned list, queue_cancel_kernel finishes it in front of the poll's first refill, and what it
//               had is copied out as for a finished one -- the host knows its length, one token per step since its admission.
//   events      what a poll delivers lies in blocks the session owns until the next poll: one per event, so a copy in flight never sees its target move.
// A request's prompt and record are copied at submit and dropped at its admission; a few words per request stay for the session's life.
struct QueueSessionEvent { int32_t id, kind, first, count, finish; size_t block; };
struct QueueSessionWaiting { std::vector<int32_t> prompt; bgk::QueueReqRec rec; };

struct biogpt_hip_queue_session {
    biogpt_hip_ctx *ctx;                    // null: the context was freed under the session
    biogpt_hip_queue_opts o{};
    std::vector<int32_t> prefix;
    int K = -1;                             // alternatives per token; -1: no log-probabilities
    int P = 0, V = 0, max_len = 0, lp_stride = 0;
    size_t stride = 0;                      // of an entry of the admit list
    QueueSessionSchedule ss;
    QueueRequests rq{};
    QueueCall qc;
    QueueRun run;
    // per request: what waits for its admission; then what stays
    std::vector<std::unique_ptr<QueueSessionWaiting>> waiting;
    std::vector<const int32_t *> own;
    std::vector<int32_t> lens, admit_step, column, sent;
    std::vector<uint32_t> seeds;
    // the device block and the pinned memory
    QueueReqBufs qb{};
    GenLpBufs lb{};
    uint8_t *look = nullptr;                // pinned: QueueReqHdr, then the stream block
    QueueStreamBufs sdev{}, shost{};
    int32_t *cancel_host = nullptr, *cancel_dev = nullptr;
    uint8_t *admit_host = nullptr;
    // the events of the last poll
    std::vector<QueueSessionEvent> evs;
    std::vector<std::vector<uint8_t>> blocks;
    std::vector<biogpt_hip_queue_event> out;
    double seconds = 0.0;
    bool failed = false;                    // a poll failed: the columns' state is unknown, only close is left

    biogpt_hip_queue_session(biogpt_hip_ctx *c, int max_columns, int group) : ctx(c), ss(max_columns, group), run{c, rq, qc, ss.q} {}
    const bgk::QueueReqHdr *hdr() const { return reinterpret_cast<const bgk::QueueReqHdr *>(look); }
    size_t block_bytes(int count) const { return (size_t)count * 4 * (K >= 0 ? 2 + 2 * (size_t)K : 1); }
    // an event with room for `count` tokens: ids, then lp, top_ids, top_lp
    uint8_t *event(int id, int kind, int first, int count, int finish) {
        blocks.emplace_back(std::max<size_t>(block_bytes(count), 4));
        evs.push_back(QueueSessionEvent{id, kind, first, count, finish, blocks.size() - 1});
        return blocks.back().data();
    }
    // what column col holds of its request, len tokens, into a block (in stream order before the column is reused)
    bool copy_out(int col, uint8_t *to, int len) {
        if (len <= 0) return true;
        const size_t n = (size_t)len, k = K > 0 ? (size_t)K : 0, src = (size_t)col * (size_t)lp_stride;
        HIP_TRY(false, hipMemcpyAsync(to, ctx->seq_gen + (size_t)col * P, n * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (K >= 0) {
            HIP_TRY(false, hipMemcpyAsync(to + n * 4, lb.lp + src, n * 4, hipMemcpyDeviceToHost, ctx->stream));
            if (k > 0) {
                HIP_TRY(false, hipMemcpyAsync(to + n * 8, lb.top_ids + src * k, n * k * 4, hipMemcpyDeviceToHost, ctx->stream));
                HIP_TRY(false, hipMemcpyAsync(to + n * 8 + n * k * 4, lb.top_lp + src * k, n * k * 4, hipMemcpyDeviceToHost, ctx->stream));
            }
        }
        return true;
    }
};

static void queue_session_orphan(biogpt_hip_ctx *c) {
    if (!c->session) return;
    (void)hipStreamSynchronize(c->stream);
    c->session->ctx = nullptr;
    c->session = nullptr;
}

static void queue_session_release(biogpt_hip_queue_session *s) {
    if (s->ctx) {
        (void)hipSetDevice(s->ctx->device);
        (void)hipStreamSynchronize(s->ctx->stream);
        s->ctx->session = nullptr;
    }
    if (s->look) (void)hipHostFree(s->look);
    if (s->cancel_host) (void)hipHostFree(s->cancel_host);
    if (s->cancel_dev) (void)hipFree(s->cancel_dev);
    delete s;
}

biogpt_hip_queue_session *biogpt_hip_queue_open(biogpt_hip_ctx *ctx, const biogpt_hip_queue_opts *opts) {
    clear_error();
    if (!opts) BG_FAIL(nullptr, "null argument: opts");
    const biogpt_hip_queue_opts &o = *opts;
    if (o.logprobs < -1 || o.logprobs > bgk::GENLP_MAX_TOP) BG_FAIL(nullptr, "logprobs must be -1 (none) or in [0, %d] (got %d)", bgk::GENLP_MAX_TOP, o.logprobs);
    if (!o.prefix && o.n_prefix != 0) BG_FAIL(nullptr, "n_prefix must be 0 without a prefix (got %d)", o.n_prefix);
    if (o.prefix && o.n_prefix < 1) BG_FAIL(nullptr, "n_prefix must be >= 1 (got %d)", o.n_prefix);
    if (o.prefix && (o.max_columns < 1 || o.max_columns > bgk::QUEUE_COLS - 1))
        BG_FAIL(nullptr, "max_columns must be in [1, %d] behind a prefix (got %d)", bgk::QUEUE_COLS - 1, o.max_columns);   // one slot holds the prefix
    if (o.max_columns < 1 || o.max_columns > bgk::QUEUE_COLS) BG_FAIL(nullptr, "max_columns must be in [1, %d]", bgk::QUEUE_COLS);
    if (o.group < 1 || o.group > 64) BG_FAIL(nullptr, "group must be in [1, 64]");
    if (o.n_batch < 1) BG_FAIL(nullptr, "n_batch must be >= 1");
    if (o.n_predict < 0) BG_FAIL(nullptr, "n_predict must be >= 0");
    if (o.max_len < 0) BG_FAIL(nullptr, "max_len must be >= 0 (0: n_positions)");
    if (!check_sample_values(o.top_k, o.top_p, o.temp, o.eos_id, -1)) return nullptr;
    for (int i = 0; i < o.n_prefix; i++)
        if (o.prefix[i] < 0) BG_FAIL(nullptr, "token id %d (prefix, position %d) out of range", o.prefix[i], i);
    if (!ctx) BG_FAIL(nullptr, "null context");
    if (!ctx->ready) BG_FAIL(nullptr, "model has no tensors loaded (empty model): cannot evaluate");
    if (session_refuses(ctx)) return nullptr;
    const int P = ctx->hp.n_positions, V = ctx->hp.n_vocab;
    if (!check_sample_values(o.top_k, o.top_p, o.temp, o.eos_id, V)) return nullptr;
    if (o.logprobs > V) BG_FAIL(nullptr, "logprobs (%d) exceeds n_vocab (%d)", o.logprobs, V);
    if (o.n_prefix > P) BG_FAIL(nullptr, "n_prefix (%d) exceeds n_positions (%d)", o.n_prefix, P);
    for (int i = 0; i < o.n_prefix; i++)
        if (o.prefix[i] >= V) BG_FAIL(nullptr, "token id %d (prefix, position %d) out of range [0, %d)", o.prefix[i], i, V);
    if (o.max_len > P) BG_FAIL(nullptr, "max_len (%d) exceeds n_positions (%d)", o.max_len, P);
    const int max_len = o.max_len > 0 ? o.max_len : P, first_len = std::max(1, (int)o.n_prefix);
    if (max_len < first_len + 1) BG_FAIL(nullptr, "max_len (%d) leaves no room for a token behind %d", max_len, first_len);
    if (!check_fast_chain(ctx, "a queue session")) return nullptr;

    biogpt_hip_queue_session *s = new biogpt_hip_queue_session(ctx, o.max_columns, o.group);
    s->o = o; s->o.prefix = nullptr;
    s->prefix.assign(o.prefix, o.prefix + o.n_prefix);
    s->K = o.logprobs; s->P = P; s->V = V; s->max_len = max_len; s->lp_stride = std::max(1, std::min((int)o.n_predict, P));
    QueueRequests &rq = s->rq;
    rq.prompts = nullptr; rq.prompt_lens = nullptr; rq.n_requests = 0; rq.n_predicts = nullptr;
    rq.n_predict = o.n_predict; rq.max_columns = o.max_columns; rq.group = o.group; rq.n_batch = o.n_batch;
    rq.prefix = s->prefix.empty() ? nullptr : s->prefix.data(); rq.pos0 = o.n_prefix;
    rq.n_shared = rq.prefix ? (rq.pos0 - 1) / o.n_batch * o.n_batch : 0;
    const int n_shared = rq.n_shared;
    QueueCall &qc = s->qc;
    qc.max_units = o.max_columns;
    qc.graphs = &ctx->graphs_queue_req; qc.form.lp = s->K >= 0; qc.form.shared = n_shared > 0;
    qc.prepare = [s, ctx](int units) -> bool {
        const int P = s->P;
        if (s->K >= 0 && (!genlp_prepare(ctx, &s->lb) || !genlp_upload(s->lb, s->K, s->lp_stride))) return false;
        s->stride = queue_req_stride(s->max_len);
        if (!ctx->queue_req_buf) HIP_TRY(false, hipMalloc(&ctx->queue_req_buf, queue_req_bufs_at(nullptr, P).bytes));
        if (!ctx->queue_req_host) HIP_TRY(false, hipHostMalloc(&ctx->queue_req_host, sizeof(bgk::QueueReqHdr) + (size_t)bgk::QUEUE_COLS * queue_req_stride(P)));
        s->qb = queue_req_bufs_at(ctx->queue_req_buf, P);
        s->admit_host = ctx->queue_req_host + sizeof(bgk::QueueReqHdr);
        const int g = s->o.stream ? s->o.group : 0;
        s->sdev = queue_stream_at(s->qb.stream, units, g, s->K);
        const size_t look_bytes = sizeof(bgk::QueueReqHdr) + (g > 0 ? s->sdev.bytes : 0);
        HIP_TRY(false, hipHostMalloc(&s->look, look_bytes));
        std::memset(s->look, 0, look_bytes);
        s->shost = queue_stream_at(s->look + sizeof(bgk::QueueReqHdr), units, g, s->K);
        HIP_TRY(false, hipHostMalloc(&s->cancel_host, sizeof(int32_t) * bgk::QUEUE_COLS));
        HIP_TRY(false, hipMalloc(&s->cancel_dev, sizeof(int32_t) * bgk::QUEUE_COLS));
        s->qc.admit_dev = s->qb.admit; s->qc.admit_host = s->admit_host; s->qc.admit_bytes = s->stride;
        s->qc.hdr_dev = s->qb.hdr; s->qc.hdr_host = s->look; s->qc.hdr_bytes = look_bytes; s->qc.fin = s->hdr()->q.fin;
        // the prefix the rules read; nobody runs yet
        if (!s->prefix.empty()) HIP_TRY(false, hipMemcpy(s->qb.prefix, s->prefix.data(), s->prefix.size() * 4, hipMemcpyHostToDevice));
        HIP_TRY(false, hipMemset(s->qb.hdr, 0, sizeof(bgk::QueueReqHdr)));
        return true;
    };
    qc.step = [s, ctx, n_shared](int t_max) -> bool {
        if (!enqueue_forward(ctx, n_shared > 0 ? ForwardPass::decode_step_shared(s->run.U, t_max, n_shared) : ForwardPass::decode_step(s->run.U, t_max))) return false;
        enqueue_queue_req_rows(ctx->stream, s->run.U, ctx->logits_all, s->V, s->qb, ctx->seq, ctx->seq_gen, s->P, s->P, s->K >= 0 ? &s->lb : nullptr);
        HIP_TRY(false, hipGetLastError());
        return true;
    };
    qc.admit = [s, n_shared](int col, int r, int i) {      // the state of the whole sequence at its last token: the suffix's, or the prefix's behind an empty one
        const QueueSessionWaiting &w = *s->waiting[(size_t)r];
        const int len = s->lens[(size_t)r];
        bgk::QueueReqAdmit *e = reinterpret_cast<bgk::QueueReqAdmit *>(s->admit_host + (size_t)i * s->stride);
        bgk::QueueAdmit rec{};
        rec.col = col; rec.last_token = len > 0 ? w.prompt[(size_t)len - 1] : s->prefix.back(); rec.len = s->rq.whole_len(r);
        rec.limit = s->rq.cap[(size_t)r]; rec.seed = s->seeds[(size_t)r];
        rec.n_shared = n_shared; rec.shared_slot = n_shared > 0 ? s->run.U : 0;
        e->a = rec;
        e->rec = w.rec;
        std::memcpy(e + 1, w.prompt.data(), (size_t)len * 4);
        s->admit_step[(size_t)r] = s->ss.q.st.steps; s->column[(size_t)r] = col;
        s->ss.admitted(r);
    };
    qc.enqueue_admit = [s, ctx](int n_admit) -> bool {
        hipLaunchKernelGGL(bgk::queue_req_admit_kernel, dim3(n_admit), dim3(bgk::QUEUE_ADMIT_THREADS), 0, ctx->stream, s->qb.admit, (int)s->stride, s->qb.seq, ctx->seq, s->qb.limit,
                           s->qb.hdr, s->qb.rec, s->qb.hist, s->P);
        HIP_TRY(false, hipGetLastError());
        // (the passes and the list's copy read the prompts of the admitted requests when they were enqueued: nothing waits for them any more)
        for (int col = 0; col < s->run.U; col++)
            if (s->ss.q.live[(size_t)col] && s->ss.q.since[(size_t)col] == 0) { const int r = s->ss.q.req[(size_t)col]; s->waiting[(size_t)r].reset(); s->own[(size_t)r] = nullptr; }
        return true;
    };
    if (o.stream) {
        qc.after_group = [s, ctx](int) -> bool {
            hipLaunchKernelGGL(bgk::queue_stream_kernel, dim3(s->run.U), dim3(bgk::QUEUE_STREAM_THREADS), 0, ctx->stream, ctx->seq, ctx->seq_gen, s->P, s->run.U, (int)s->o.group,
                               s->sdev.out, s->K >= 0 ? s->lb.lp : nullptr, s->K >= 0 ? s->lb.top_ids : nullptr, s->K >= 0 ? s->lb.top_lp : nullptr, s->lp_stride,
                               std::max(s->K, 0));
            HIP_TRY(false, hipGetLastError());
            return true;
        };
        qc.looked = [s]() -> bool {      // per running request, the tokens behind what it has been sent
            const QueueSchedule &q = s->ss.q;
            const int G = s->o.group;
            const size_t k = s->K > 0 ? (size_t)s->K : 0;
            for (int col = 0; col < s->run.U; col++) {
                if (!q.live[(size_t)col]) continue;
                const int r = q.req[(size_t)col];
                const int n = std::max(0, std::min(s->shost.out.n_gen[col], s->rq.cap[(size_t)r])), first = s->sent[(size_t)r], count = n - first, w = std::min(G, n);
                if (count <= 0) continue;
                const int at = first - (n - w);
                if (at < 0) BG_FAIL(false, "internal: request %d (column %d) appended %d tokens in one group of at most %d steps", r, col, count, G);
                uint8_t *to = s->event(r, 0, first, count, -1);
                const size_t c4 = (size_t)count * 4, from = (size_t)col * (size_t)G + (size_t)at;
                std::memcpy(to, s->shost.out.ids + from, c4);
                if (s->K >= 0) {
                    std::memcpy(to + c4, s->shost.out.lp + from, c4);
                    std::memcpy(to + 2 * c4, s->shost.out.top_ids + from * k, c4 * k);
                    std::memcpy(to + 2 * c4 + c4 * k, s->shost.out.top_lp + from * k, c4 * k);
                }
                s->sent[(size_t)r] = n;
            }
            return true;
        };
    }
    qc.collect = [s](int col, int r) -> int {
        const int len = std::max(0, std::min(s->hdr()->q.len[col], s->rq.cap[(size_t)r]));
        uint8_t *to = s->event(r, 1, 0, len, s->hdr()->reason[col]);
        if (!s->copy_out(col, to, len)) return -1;
        s->ss.finished(col, r, len);
        return len;
    };

    XpCallScope xp_scope(ctx);
    XcBatchScope xc_scope{ctx};
    const auto t0 = std::chrono::steady_clock::now();
    if (s->run.begin(first_len, max_len, P) != 0 || hipStreamSynchronize(ctx->stream) != hipSuccess || !xpipe_check(ctx)) {
        const std::string why = last_error();
        queue_session_release(s);
        BG_FAIL(nullptr, "%s", why.empty() ? "a queue session could not be opened" : why.c_str());
    }
    if (n_shared > 0) s->seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();      // (the shared rows belong to the timed span)
    ctx->session = s;
    return s;
}

static bool queue_session_usable(biogpt_hip_queue_session *s) {
    if (!s) BG_FAIL(false, "null queue session");
    if (!s->ctx) BG_FAIL(false, "the queue session's context has been freed: only biogpt_hip_queue_close is left");
    if (s->failed) BG_FAIL(false, "the queue session failed in an earlier poll: only biogpt_hip_queue_close is left");
    return true;
}

int biogpt_hip_queue_submit(biogpt_hip_queue_session *s, const int32_t *prompt, int32_t len, int32_t n_predict, uint32_t seed, const biogpt_hip_request_params *params) {
    clear_error();
    if (!queue_session_usable(s)) return -1;
    const int id = s->ss.q.known, pos0 = s->rq.pos0;
    if (len < 0) BG_FAIL(-1, "len (%d) is negative", len);
    if (len > 0 && !prompt) BG_FAIL(-1, "null argument: prompt");
    if (len < 1 && pos0 == 0) BG_FAIL(-1, "empty prompt (request %d)", id);      // (behind a prefix no sequence is empty)
    if (n_predict < 0 || n_predict > s->o.n_predict) BG_FAIL(-1, "n_predict (%d) must be in [0, the session's n_predict = %d]", n_predict, s->o.n_predict);
    biogpt_hip_request_params def{};
    def.top_k = s->o.top_k; def.eos_id = s->o.eos_id; def.top_p = s->o.top_p; def.temp = s->o.temp; def.rules.repetition_penalty = 1.0f;
    const biogpt_hip_request_params &p = params ? *params : def;
    if (!check_request_params(p, id, -1, -1) || !check_request_params(p, id, s->V, s->P)) return -1;
    if (s->K >= 0 && rules_active(&p.rules, p.eos_id))
        BG_FAIL(-1, "logprobs with generation rules (params of request %d have a rule switched on): no closed call returns log-probabilities under rules", id);
    if (len > s->P - pos0) BG_FAIL(-1, "n_prefix (%d) + len (%d) exceeds n_positions (%d)", pos0, len, s->P);
    for (int i = 0; i < len; i++)
        if (prompt[i] < 0 || prompt[i] >= s->V) BG_FAIL(-1, "token id %d (request %d, position %d) out of range [0, %d)", prompt[i], id, i, s->V);
    const int whole = pos0 + len, cap = std::min((int)n_predict, s->P - whole);
    if (cap > 0 && whole + cap > s->max_len)
        BG_FAIL(-1, "request %d needs %d keys (%d tokens and %d to generate): more than the session's max_len (%d), for which its steps were captured", id, whole + cap, whole, cap, s->max_len);
    std::unique_ptr<QueueSessionWaiting> w;
    if (cap > 0) {
        w.reset(new QueueSessionWaiting{std::vector<int32_t>(prompt, prompt + len), request_rec_of(p, pos0, len)});
    }
    s->own.push_back(w ? w->prompt.data() : nullptr);
    s->waiting.push_back(std::move(w));
    s->lens.push_back(len); s->admit_step.push_back(-1); s->column.push_back(-1); s->sent.push_back(0); s->seeds.push_back(seed);
    s->rq.cap.push_back(std::max(cap, 0));      // (the driver's copy of the clamp the schedule holds)
    const int r = s->ss.submit(cap);
    s->rq.n_requests = s->ss.q.known; s->rq.prompt_lens = s->lens.data(); s->rq.own = s->own.data();
    return r;
}

int biogpt_hip_queue_cancel(biogpt_hip_queue_session *s, int32_t id) {
    clear_error();
    if (!queue_session_usable(s)) return -1;
    const int rc = s->ss.cancel(id);
    if (rc == -1) BG_FAIL(-1, "no request %d in this queue session (%d submitted)", id, s->ss.q.known);
    if (rc == -2) BG_FAIL(-1, "request %d has finished or was cancelled already", id);
    return 0;
}

int biogpt_hip_queue_poll(biogpt_hip_queue_session *s, int32_t max_groups, const biogpt_hip_queue_event **events_out) {
    clear_error();
    if (!queue_session_usable(s)) return -1;
    if (max_groups < 0) BG_FAIL(-1, "max_groups must be >= 0");
    if (!events_out) BG_FAIL(-1, "null argument: events_out");
    biogpt_hip_ctx *ctx = s->ctx;
    QueueSchedule &q = s->ss.q;
    s->evs.clear(); s->blocks.clear(); s->out.clear();
    *events_out = nullptr;
    s->rq.prompt_lens = s->lens.data(); s->rq.own = s->own.data();
    bool ok = true, enqueued = false;
    int n_stop = 0;
    std::vector<std::pair<int, size_t>> stopped;      // the columns of the cancelled running requests, each with its event
    s->ss.begin_poll([&](int r) { s->event(r, 1, 0, 0, -1); },
                     [&](int r) { s->event(r, 2, 0, 0, -1); s->waiting[(size_t)r].reset(); s->own[(size_t)r] = nullptr; },
                     [&](int col, int r, int len) {
                         s->cancel_host[n_stop++] = col;
                         s->event(r, 2, 0, std::min(len, s->rq.cap[(size_t)r]), -1);
                         stopped.emplace_back(col, s->evs.size() - 1);
                     });
    if (!q.done() || n_stop > 0) {      // (nothing runs and nothing waits: no launch)
        HIP_TRY(-2, hipSetDevice(ctx->device));
        XpCallScope xp_scope(ctx);
        XcBatchScope xc_scope{ctx};
        const auto t0 = std::chrono::steady_clock::now();
        s->run.use_graph = s->run.use_graph && plain_graph_begin(ctx);      // (another context may have taken the pipeline slot since: eager launches from then on)
        if (n_stop > 0) {
            ok = hipMemcpyAsync(s->cancel_dev, s->cancel_host, (size_t)n_stop * 4, hipMemcpyHostToDevice, ctx->stream) == hipSuccess;
            if (ok) {
                hipLaunchKernelGGL(bgk::queue_cancel_kernel, dim3((n_stop + bgk::QUEUE_ADMIT_THREADS - 1) / bgk::QUEUE_ADMIT_THREADS), dim3(bgk::QUEUE_ADMIT_THREADS), 0, ctx->stream,
                                   s->cancel_dev, n_stop, s->qb.seq, ctx->seq, &s->qb.hdr->q);
                ok = hipGetLastError() == hipSuccess;
            }
            for (const auto &st : stopped)
                if (ok) ok = s->copy_out(st.first, s->blocks[s->evs[st.second].block].data(), s->evs[st.second].count);
            if (!ok && last_error()[0] == 0) bg::set_error("biogpt_hip_queue_poll", "a cancel could not be enqueued");
            enqueued = true;
        }
        for (int n = 0; ok && n < max_groups && !q.done(); n++) { ok = s->run.turn() == 0; enqueued = true; }
        if (enqueued && hipStreamSynchronize(ctx->stream) != hipSuccess && ok) { ok = false; bg::set_error("biogpt_hip_queue_poll", "the stream could not be drained"); }
        if (ok && enqueued && !xpipe_check(ctx)) ok = false;
        s->seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
    if (!ok) { s->failed = true; return -2; }
    const size_t k = s->K > 0 ? (size_t)s->K : 0;
    for (const QueueSessionEvent &e : s->evs) {
        biogpt_hip_queue_event ev{};
        const uint8_t *b = s->blocks[e.block].data();
        const size_t c4 = (size_t)e.count * 4;
        ev.id = e.id; ev.kind = e.kind; ev.first = e.first; ev.count = e.count; ev.finish = e.finish;
        ev.admit_step = s->admit_step[(size_t)e.id]; ev.column = s->column[(size_t)e.id];
        ev.n_top = s->K;
        ev.ids = reinterpret_cast<const int32_t *>(b);
        if (s->K >= 0) {
            ev.lp = reinterpret_cast<const float *>(b + c4);
            ev.top_ids = reinterpret_cast<const int32_t *>(b + 2 * c4);
            ev.top_lp = reinterpret_cast<const float *>(b + 2 * c4 + c4 * k);
        }
        s->out.push_back(ev);
    }
    *events_out = s->out.data();
    return (int)s->out.size();
}

int biogpt_hip_queue_session_stats(const biogpt_hip_queue_session *s, biogpt_hip_queue_stats *stats, double *seconds_out, int32_t *counts_out) {
    clear_error();
    if (!s) BG_FAIL(-1, "null queue session");
    if (!stats) BG_FAIL(-1, "null argument: stats");
    *stats = s->ss.q.st;
    if (seconds_out) *seconds_out = s->seconds;
    if (counts_out) { counts_out[0] = s->ss.q.known; counts_out[1] = s->ss.q.pending; counts_out[2] = s->ss.q.running; }
    return 0;
}

int biogpt_hip_queue_close(biogpt_hip_queue_session *s) {
    clear_error();
    if (!s) BG_FAIL(-1, "null queue session");
    biogpt_hip_ctx *ctx = s->ctx;
    queue_session_release(s);      // (requests still running are dropped with their columns' state: the next call's admit kernel or upload sets its own)
    if (ctx) (void)xpipe_check(ctx);
    return 0;
}

// ---- beam search over a queue: a unit is a group slot of B columns; finished searches hand their slot on (kernels_beam_queue.hip.h) ------------------
// S = min(max_columns / n_beams, eligible requests) group slots of B columns and K / V slots each serve any number of requests: a request's search runs in one
// slot -- group `slot` of biogpt_hip_generate_beam_batch's state, columns [slot * B, (slot + 1) * B) -- under its own clamp, and when it stops, by
// transformers' stopping rules or after its own n_predict steps, its pool is copied out and the slot goes to the next request.  What the mode supplies to
// run_queue_call: the step (the three beam kernels behind the forward pass, then beam_slot_report_kernel into the header, BeamQueueHdr); behind the admit list
// kv_share_slots_kernel -- the prompt pass has filled the first slot of each admitted group -- and beam_slot_admit_kernel; for a finished slot the copies of its
// BeamCtl and its B pool rows to the pinned twin, decoded into the caller's rows once a later wait has proved their arrival (landed).  A refilled slot keeps its
// old K / V rows beyond the new prompt and its old pool rows: no decode-step attention kernel lets a column see a key at or beyond its own n_past + 1, and
// pool_n = 0 hides the pool.
// The searches' state block is the context's bbatch_buf, the one biogpt_hip_generate_beam_batch uses (allocated once at its largest: the captured steps of
// both keep their pointers, and a closed call uploads its whole start state, so neither sees the other's leftovers); what the queue adds -- report header and
// admit list -- is a block of its own.  The steps are captured per bucket into graphs_bqueue, keyed by (S, B), trie or not, and always run the launch chain.
struct BeamQueueBufs {
    bgk::BeamQueueHdr *hdr;
    bgk::BeamQueueAdmit *admit;     // [BEAM_QUEUE_SLOTS]
    size_t bytes;
};
static BeamQueueBufs bqueue_bufs_at(uint8_t *base) {
    ByteLayout l;
    BeamQueueBufs b{};
    b.hdr = l.take<bgk::BeamQueueHdr>(base, 1); b.admit = l.take<bgk::BeamQueueAdmit>(base, bgk::BEAM_QUEUE_SLOTS);
    b.bytes = l.bytes();
    return b;
}
// the pinned twin: the header as the host reads it, the admit list as the host writes it, every slot's BeamCtl as it comes back; the slots' pool rows
// ([BBATCH_COLS][n_positions] words) lie behind it
struct BeamQueueHost {
    bgk::BeamQueueHdr hdr;
    bgk::BeamQueueAdmit admit[bgk::BEAM_QUEUE_SLOTS];
    bgk::BeamCtl ctl[bgk::BEAM_QUEUE_SLOTS];
};

static int generate_beam_queue_once(biogpt_hip_ctx *ctx, const int32_t *prompts, const int32_t *prompt_lens, int32_t n_requests, const int32_t *n_predicts,
                                    int32_t n_predict, int32_t n_beams, int32_t max_columns, int32_t group, int32_t n_batch, int32_t eos_id, float length_penalty,
                                    int32_t early_stopping, biogpt_hip_trie *trie, int32_t *out_ids, int32_t *out_lens, float *out_scores, int32_t *out_counts,
                                    int32_t *out_steps, int32_t *out_admit_step, int32_t *out_slot, double *seconds_out, biogpt_hip_queue_stats *stats) {
    clear_error();
    if (!prompts) BG_FAIL(-1, "null argument: prompts");
    if (!prompt_lens) BG_FAIL(-1, "null argument: prompt_lens");
    if (!out_ids) BG_FAIL(-1, "null argument: out_ids");
    if (!out_lens) BG_FAIL(-1, "null argument: out_lens");
    if (!out_scores) BG_FAIL(-1, "null argument: out_scores");
    if (!out_counts) BG_FAIL(-1, "null argument: out_counts");
    QueueRequests rq{prompts, prompt_lens, n_requests, n_predicts, n_predict, max_columns, group, n_batch};
    if (!rq.check_count()) return -1;
    if (n_beams < 1 || n_beams > bgk::BEAM_MAX) BG_FAIL(-1, "n_beams must be in [1, %d]", bgk::BEAM_MAX);
    if (max_columns < n_beams || max_columns > BBATCH_COLS) BG_FAIL(-1, "max_columns must be in [n_beams = %d, %d]", n_beams, BBATCH_COLS);
    if (!rq.check_sizes()) return -1;
    if (eos_id < -1) BG_FAIL(-1, "eos_id %d out of range: must be a token id, or -1 for none", eos_id);
    if (!std::isfinite(length_penalty)) BG_FAIL(-1, "length_penalty must be finite");
    if (early_stopping != 0 && early_stopping != 1) BG_FAIL(-1, "early_stopping must be 0 or 1");
    if (trie && !check_trie(trie, eos_id)) return -1;
    if (!rq.check_prompts(ctx)) return -1;
    const auto &hp = ctx->hp;
    const int P = hp.n_positions, V = hp.n_vocab, B = n_beams;
    if (eos_id >= V) BG_FAIL(-1, "eos_id %d out of range: must be in [0, %d), or -1 for none", eos_id, V);
    if (!rq.check_prompts_model(ctx, "beam search over a queue")) return -1;
    if (V < 2 * B) BG_FAIL(-1, "a vocabulary of %d tokens holds fewer than 2 x n_beams candidates", V);
    if (trie && !check_trie_vocab(trie, V)) return -1;
    const size_t row = (size_t)n_predict, rows = (size_t)n_requests * (size_t)B;
    std::fill(out_ids, out_ids + rows * row, -1);
    std::fill(out_lens, out_lens + rows, 0);
    std::fill(out_scores, out_scores + rows, 0.0f);
    std::fill(out_counts, out_counts + n_requests, 0);
    if (out_steps) std::fill(out_steps, out_steps + n_requests, 0);

    BeamBufs bufs{};
    BeamQueueBufs qb{};
    BeamQueueHost *qh = nullptr;
    int32_t *pool_host = nullptr;
    int S = 0, C = 0;
    const bool given = trie != nullptr;
    const int64_t seq_stride = (int64_t)hp.n_layer * P * hp.d_model;
    bgk::BeamQueueCall call{};
    call.n_beams = B; call.eos_id = eos_id; call.length_penalty = length_penalty; call.early_stopping = early_stopping; call.ids_stride = P;
    std::vector<std::pair<int, int>> landing;              // (slot, request): copies enqueued, not yet known to have arrived
    QueueCall qc;
    qc.max_units = max_columns / B; qc.per_unit = B;
    qc.unit = "slot"; qc.step_name = "beam queue step";
    qc.graphs = &ctx->graphs_bqueue; qc.key_b = B; qc.form.sel = trie ? StepForm::Trie : StepForm::Plain;
    qc.out_admit_step = out_admit_step; qc.out_unit = out_slot; qc.seconds_out = seconds_out; qc.stats = stats;
    qc.prepare = [&](int units) -> bool {
        S = units; C = S * B; call.n_slots = S;
        if (!ctx->bbatch_buf) {
            size_t bytes;
            beam_bufs_of(ctx, &bytes);
            HIP_TRY(false, hipMalloc(&ctx->bbatch_buf, bytes));
        }
        if (!ctx->bqueue_buf) HIP_TRY(false, hipMalloc(&ctx->bqueue_buf, bqueue_bufs_at(nullptr).bytes));
        if (!ctx->bqueue_host) HIP_TRY(false, hipHostMalloc(&ctx->bqueue_host, sizeof(BeamQueueHost) + (size_t)BBATCH_COLS * (size_t)P * 4));
        bufs = beam_bufs_of(ctx);
        qb = bqueue_bufs_at(ctx->bqueue_buf);
        qh = reinterpret_cast<BeamQueueHost *>(ctx->bqueue_host);
        pool_host = reinterpret_cast<int32_t *>(ctx->bqueue_host + sizeof(BeamQueueHost));
        qc.admit_dev = qb.admit; qc.admit_host = qh->admit; qc.admit_bytes = sizeof(bgk::BeamQueueAdmit);
        qc.hdr_dev = qb.hdr; qc.hdr_host = &qh->hdr; qc.hdr_bytes = sizeof(bgk::BeamQueueHdr); qc.fin = qh->hdr.fin;
        // nobody runs yet: every slot's search reads as stopped and reported, no forks
        HeadImage im(bufs.hdr, bufs.ctl + S);
        for (int s = 0; s < S; s++) {
            im.at(bufs.ctl)[s] = beam_ctl_of(B, 1, 0, eos_id, length_penalty, early_stopping, P);
            im.at(bufs.ctl)[s].done = 1;
        }
        for (int c = 0; c < C; c++) im.at(bufs.col_skip)[c] = 1;
        if (!im.upload()) return false;
        qh->hdr = bgk::BeamQueueHdr{};
        for (int s = 0; s < S; s++) qh->hdr.fin[s] = 1;
        HIP_TRY(false, hipMemcpy(qb.hdr, &qh->hdr, sizeof(bgk::BeamQueueHdr), hipMemcpyHostToDevice));
        return !trie || trie_upload(ctx, trie, 1, eos_id);
    };
    qc.step = [&](int t_max) -> bool {
        if (!enqueue_forward(ctx, ForwardPass::decode_step(C, t_max))) return false;
        if (trie && !enqueue_trie(ctx, C, bufs.col_skip, 1)) return false;
        if (!enqueue_beam_group_select(bufs, S, B, given)) return false;
        hipLaunchKernelGGL(bgk::beam_slot_report_kernel, dim3((S + bgk::BEAM_QUEUE_REPORT_THREADS - 1) / bgk::BEAM_QUEUE_REPORT_THREADS),
                           dim3(bgk::BEAM_QUEUE_REPORT_THREADS), 0, ctx->stream, bufs.ctl, S, qb.hdr);
        HIP_TRY(false, hipGetLastError());
        return true;
    };
    qc.admit = [&](int slot, int r, int i) {
        const int len = prompt_lens[r];
        qh->admit[i] = bgk::BeamQueueAdmit{slot, prompts[rq.off[(size_t)r] + (size_t)(len - 1)], len, rq.cap[(size_t)r]};
    };
    qc.enqueue_admit = [&](int n_admit) -> bool {
        if (B > 1) {
            hipLaunchKernelGGL(bgk::kv_share_slots_kernel, dim3(hp.n_layer * hp.n_head, n_admit * (B - 1), 2), dim3(256), 0, ctx->stream, qb.admit, B, S, ctx->bk, ctx->bv,
                               seq_stride, P, hp.d_model / hp.n_head);
            HIP_TRY(false, hipGetLastError());
        }
        hipLaunchKernelGGL(bgk::beam_slot_admit_kernel, dim3(n_admit), dim3(bgk::BEAM_QUEUE_ADMIT_THREADS), 0, ctx->stream, qb.admit, call, bufs.ctl, ctx->seq, bufs.col_skip,
                           bufs.hdr, qb.hdr);
        HIP_TRY(false, hipGetLastError());
        return true;
    };
    qc.collect = [&](int slot, int r) -> int {      // the search's state and its B pool rows (whole rows up to the last one's limit) -> the slot's pinned twin
        const int n_steps = std::max(0, std::min(qh->hdr.steps[slot], rq.cap[(size_t)r]));
        HIP_TRY(-1, hipMemcpyAsync(&qh->ctl[slot], bufs.ctl + slot, sizeof(bgk::BeamCtl), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(-1, hipMemcpyAsync(pool_host + (size_t)slot * B * P, bufs.pool_ids + (size_t)slot * B * P, ((size_t)(B - 1) * P + (size_t)rq.cap[(size_t)r]) * 4,
                                   hipMemcpyDeviceToHost, ctx->stream));
        landing.emplace_back(slot, r);
        if (out_steps) out_steps[r] = n_steps;
        return n_steps;
    };
    qc.landed = [&]() -> bool {      // the pools whose copies have arrived -> their requests' rows; the slots' twins are free again
        for (const auto &sr : landing) {
            const size_t o = (size_t)sr.second * (size_t)B;
            if (!beam_read_pools(&qh->ctl[sr.first], pool_host + (size_t)sr.first * B * P, (size_t)P, 1, B, n_predict, out_ids + o * row, out_lens + o, out_scores + o,
                                 out_counts + sr.second, "request", sr.second))
                return false;
        }
        landing.clear();
        return true;
    };
    return run_queue_call(ctx, rq, qc);
}

int biogpt_hip_generate_beam_queue(biogpt_hip_ctx *ctx, const int32_t *prompts, const int32_t *prompt_lens, int32_t n_requests, const int32_t *n_predicts,
                                   int32_t n_predict, int32_t n_beams, int32_t max_columns, int32_t group, int32_t n_batch, int32_t eos_id, float length_penalty,
                                   int32_t early_stopping, biogpt_hip_trie *trie, int32_t *out_ids, int32_t *out_lens, float *out_scores, int32_t *out_counts,
                                   int32_t *out_steps, int32_t *out_admit_step, int32_t *out_slot, double *seconds_out, biogpt_hip_queue_stats *stats) {
    return with_xpipe_retry(ctx, 0, [&] {
        return generate_beam_queue_once(ctx, prompts, prompt_lens, n_requests, n_predicts, n_predict, n_beams, max_columns, group, n_batch, eos_id, length_penalty,
                                        early_stopping, trie, out_ids, out_lens, out_scores, out_counts, out_steps, out_admit_step, out_slot, seconds_out, stats);
    });
}

// profiling builds (BIOGPT_HIP_PROFILE_HOOKS + BIOGPT_HIP_DBG=128): the raw 100 MHz stage stamps the pipelined launches left (kernels_xpipe.hip.h XP_WALL / XP_TAIL)
int biogpt_hip_debug_stamps(biogpt_hip_ctx *ctx, size_t offset, size_t count, unsigned long long *out) {
    clear_error();
    if (!ctx || !out) BG_FAIL(-1, "null argument");
    const size_t cap = ((size_t)4 << 20) / 8;                 // stamps in the buffer; checked without a sum that could wrap
    if (!ctx->tstamp || offset > cap || count > cap - offset) BG_FAIL(-1, "no stamps (profiling build with BIOGPT_HIP_DBG=128 only)");
    HIP_TRY(-2, hipSetDevice(ctx->device));
    if (!resident_stop(ctx)) return -2;
    HIP_TRY(-2, hipStreamSynchronize(ctx->stream));
    HIP_TRY(-2, hipMemcpy(out, ctx->tstamp + offset, count * 8, hipMemcpyDeviceToHost));
    return 0;
}

int biogpt_hip_read_kv(biogpt_hip_ctx *ctx, int which, size_t offset, size_t count, float *out) {
    if (!ctx || !out) BG_FAIL(-1, "null argument");
    const size_t L = (size_t)ctx->hp.n_layer, P = (size_t)ctx->hp.n_positions, D = (size_t)ctx->hp.d_model, H = (size_t)ctx->hp.n_head;
    const size_t dk = D / H, total = L * P * D;
    if (offset > total || count > total - offset) BG_FAIL(-1, "KV range out of bounds");      // (no sum that could wrap)
    if (count == 0) return 0;
    HIP_TRY(-2, hipSetDevice(ctx->device));
    if (!resident_stop(ctx)) return -2;
    // the device cache is head-major [layer][head][pos][dk]; the caller sees the reference's flat [layer][pos][d_model]
    // view (biogpt.cpp:331-335).  Only the requested range is gathered on the device and copied.
    DeviceBytes stage;
    if (!stage.alloc(count * 4)) return -2;
    const float *cache = which ? ctx->memory_v : ctx->memory_k;
    hipLaunchKernelGGL(bgk::kv_gather_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, ctx->stream, cache, stage.at<float>(0), (unsigned long long)offset,
                       (unsigned long long)count, (int)P, (int)D, (int)H, (int)dk);
    HIP_TRY(-2, hipGetLastError());
    HIP_TRY(-2, hipMemcpyAsync(out, stage.p, count * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(-2, hipStreamSynchronize(ctx->stream));
    return 0;
}

// What the last column call left in a column's K / V cache slot and beam pool row (tests of slot reuse): the K (which 0) or V (1) row of position pos in every
// layer, [n_layer][d_model] in the reference's channel order, and the first n_ids words of pool row `column` (either output may be NULL)
int biogpt_hip_read_column_state(biogpt_hip_ctx *ctx, int32_t column, int32_t which, int32_t pos, float *kv_out, int32_t n_ids, int32_t *pool_out) {
    clear_error();
    if (!ctx) BG_FAIL(-1, "null context");
    const int L = ctx->hp.n_layer, P = ctx->hp.n_positions, D = ctx->hp.d_model, H = ctx->hp.n_head, dk = D / H;
    if (column < 0 || column >= ctx->batch_cap) BG_FAIL(-1, "column %d out of range: this context holds %d column caches", column, ctx->batch_cap);
    if (kv_out && (pos < 0 || pos >= P)) BG_FAIL(-1, "pos %d out of range [0, %d)", pos, P);
    if (pool_out && (n_ids < 0 || n_ids > P || column >= BBATCH_COLS || !ctx->bbatch_buf)) BG_FAIL(-1, "no pool row %d of %d words (no beam search has run?)", column, n_ids);
    HIP_TRY(-2, hipSetDevice(ctx->device));
    HIP_TRY(-2, hipStreamSynchronize(ctx->stream));
    if (kv_out) {      // head-major [column][layer][head][pos][dk]
        const float *root = (which ? ctx->bv : ctx->bk) + (size_t)column * L * P * D;
        for (int l = 0; l < L; l++)
            for (int h = 0; h < H; h++)
                HIP_TRY(-2, hipMemcpy(kv_out + (size_t)l * D + (size_t)h * dk, root + (((size_t)l * H + h) * P + pos) * dk, (size_t)dk * 4, hipMemcpyDeviceToHost));
    }
    if (pool_out && n_ids > 0) HIP_TRY(-2, hipMemcpy(pool_out, beam_bufs_of(ctx).pool_ids + (size_t)column * P, (size_t)n_ids * 4, hipMemcpyDeviceToHost));
    return 0;
}

#include "engine_bench.inc"
#include "engine_probe.inc"
int biogpt_hip_quantize_file(const char *fname_in, const char *fname_out, int32_t ftype) {
    clear_error();
    if (!fname_in || !fname_out) BG_FAIL(-1, "null file name");
    return quantize_file(fname_in, fname_out, ftype) ? 0 : -1;
}

int biogpt_hip_write_synthetic(const char *fname, const biogpt_hip_hparams *hp, uint64_t seed) {
    clear_error();
    if (!fname || !hp) BG_FAIL(-1, "null argument");
    return write_synthetic(fname, *hp, seed) ? 0 : -1;
}

}  // extern "C"
