/*
 * include/biogpt_hip.h -- C-ABI of the MI355X-native BioGPT decoder engine.
 *
 * This is the drop-in boundary for the reference's model-library path:
 *
 *   reference (C++, biogpt.h)                         this library (extern "C")
 *   ------------------------------------------------  ---------------------------------------
 *   biogpt_model_load()      biogpt.h:128-132         biogpt_hip_load()
 *                            biogpt.cpp:27-453
 *   biogpt_eval()            biogpt.h:145-151         biogpt_hip_eval()
 *                            biogpt.cpp:812-847
 *   biogpt_graph()           biogpt.h:139-143         (internal: fixed launch sequence / hipGraph;
 *                            biogpt.cpp:624-810        nothing to size, see biogpt_compat.h)
 *   generation loop          main.cpp:91-151          biogpt_hip_generate_greedy()  (device-resident
 *   + top_k=1 sampler        biogpt.cpp:908-980        loop: argmax + token feedback stay in HBM)
 *   biogpt_model_quantize_internal + quantize CLI     biogpt_hip_quantize_file()
 *                            biogpt.cpp:459-621, quantize.cpp:8-135
 *   gpt_tokenize             biogpt.cpp:850-875       biogpt_hip_tokenize()         (host-only: Moses word
 *   gpt_decode               biogpt.cpp:877-906       biogpt_hip_decode()            splitting + byte BPE)
 *   teardown                 main.cpp:164-169         biogpt_hip_free()
 *
 * Plain pointers and sizes only: no C++/torch types cross this boundary.  The C++ wrappers with
 * the reference's exact signatures live in include/biogpt_compat.h and are implemented on top of
 * these entry points.  All functions are thread-compatible per context (one eval at a time per
 * context; different contexts -- e.g. one per GPU -- may run concurrently).
 *
 * Error convention: the reference returns false + fprintf(stderr).  Here: pointer
 * results are NULL on failure, int results are 0 on success and negative on failure; the message
 * is printed to stderr (prefixed like the reference's "%s: ...") and kept for
 * biogpt_hip_last_error().  There is NO CPU fallback: without a usable HIP device every compute
 * entry point fails loudly.
 */
#ifndef BIOGPT_HIP_H
#define BIOGPT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct biogpt_hip_ctx biogpt_hip_ctx;
typedef struct biogpt_hip_vocab biogpt_hip_vocab;   /* vocabulary + merge ranks of one model file (host memory) */

/* tokenizer status: the reference's moses_tokenize throws std::length_error for this input (see below) */
#define BIOGPT_HIP_E_LENGTH (-7)

/* header ints in file order (biogpt.cpp:54-60) + the merge count found in the file */
typedef struct biogpt_hip_hparams {
    int32_t n_vocab;
    int32_t n_layer;
    int32_t n_head;
    int32_t n_positions;
    int32_t d_ff;
    int32_t d_model;
    int32_t ftype;    /* ggml_ftype: 0 f32, 1 f16, 2 q4_0, 3 q4_1, 7 q8_0, 8 q5_0, 9 q5_1 */
    int32_t n_merges;
} biogpt_hip_hparams;

/* Last error message of the calling thread ("" if none). */
const char *biogpt_hip_last_error(void);

/* Library / build identification, e.g. "biogpt-hip gfx950 r1". */
const char *biogpt_hip_version(void);

/* ---- load / free --------------------------------------------------------------------------
 * biogpt_hip_load: parse `fname` (ggml-model.bin), repack every tensor into
 * the device arena on HIP device `device`, allocate the F32 KV cache (biogpt.cpp:324-358).
 * Replaces biogpt_model_load (biogpt.cpp:27-453); same validation and the same failure cases
 * (bad magic, bad vocab size, bad ftype, unknown tensor, wrong shape/size, missing tensors);
 * a file with zero tensors loads with a warning (biogpt.cpp:442-443) and cannot be evaluated.
 * Unlike the reference the merge count is taken from the file (F6) and embed_positions is sized
 * by the file (F5). */
biogpt_hip_ctx *biogpt_hip_load(const char *fname, int device, int verbosity);

/* Same, but the weight arena lives in caller-owned device memory (e.g. a torch uint8 tensor that
 * is then broadcast over RCCL); arena_bytes must be >= biogpt_hip_arena_bytes_for(). */
biogpt_hip_ctx *biogpt_hip_load_into(const char *fname, int device, int verbosity,
                                     void *device_arena, size_t arena_bytes);

/* Create a context around an arena that ALREADY holds repacked weights (received by broadcast from
 * a rank that loaded the file): no file access.  hp must equal the loading rank's hparams. */
biogpt_hip_ctx *biogpt_hip_attach(const biogpt_hip_hparams *hp, int device,
                                  void *device_arena, size_t arena_bytes);

/* Size in bytes of the device weight arena for these hparams (deterministic layout). */
size_t biogpt_hip_arena_bytes_for(const biogpt_hip_hparams *hp);

/* The context's arena (owned or external) -- what a multi-GPU launcher broadcasts. */
void  *biogpt_hip_arena_ptr(biogpt_hip_ctx *ctx);
size_t biogpt_hip_arena_bytes(const biogpt_hip_ctx *ctx);

void biogpt_hip_free(biogpt_hip_ctx *ctx);

/* An attached context (biogpt_hip_attach) has weights but no vocabulary: copy the token / merge tables of a context
 * that was loaded from the file, so that every replica can tokenize and decode (biogpt.cpp:850-906). */
int biogpt_hip_share_vocab(biogpt_hip_ctx *dst, const biogpt_hip_ctx *src);

/* ---- single-process multi-GPU replicas (replaces the ONE biogpt_model_load of examples/main/main.cpp:38) ----
 * The file is read once on devices[0]; the packed weight arena goes to the other devices with ONE RCCL broadcast
 * (ncclCommInitAll, in-process; librccl.so is resolved at run time); every device gets its own context.  Prompt g is
 * served by replica g mod n, one host thread per device, no collective on the data path.  NULL + message on failure. */
typedef struct biogpt_hip_replicas biogpt_hip_replicas;
biogpt_hip_replicas *biogpt_hip_replicas_load(const char *fname, const int *devices, int n_devices, int verbosity);
int biogpt_hip_replicas_count(const biogpt_hip_replicas *r);
biogpt_hip_ctx *biogpt_hip_replicas_ctx(biogpt_hip_replicas *r, int i);   /* borrowed: freed by biogpt_hip_replicas_free */
double biogpt_hip_replicas_broadcast_seconds(const biogpt_hip_replicas *r);
/* Greedy continuations (main.cpp:91-151 with --top_k 1) of n_prompts independent prompts (ids concatenated, lengths in
 * prompt_lens): out_ids[g][n_predict], out_counts[g] = ids produced for prompt g (n_predict clamped like main.cpp:82; may
 * be NULL); *seconds_out = wall time of the whole call.  Returns n_prompts or < 0. */
int biogpt_hip_replicas_generate_greedy(biogpt_hip_replicas *r, const int32_t *prompts, const int32_t *prompt_lens, int32_t n_prompts,
                                        int32_t n_batch, int32_t n_predict, int32_t *out_ids, int32_t *out_counts, double *seconds_out);
void biogpt_hip_replicas_free(biogpt_hip_replicas *r);

/* The BIOGPT_HIP_* tuning / debugging switches are read from the environment once, when a context is
 * created (no getenv on any launch path).  This re-reads them for an existing context and drops its
 * captured graphs (tests and sweep tools; the reference has no counterpart). */
int biogpt_hip_refresh_options(biogpt_hip_ctx *ctx);

/* The single-token decode step of BioGPT-base-shaped block-quantized models (Q4_0 .. Q8_0) with at most 256 keys runs as ONE
 * persistent launch pipelined over the 8 XCDs (csrc/kernels_xpipe.hip.h).  1: this context uses it; 0: switched off
 * (BIOGPT_HIP_XPIPE=0) or another context of the device holds the path; -1: not available (model shape / weight type /
 * device; another PROCESS holds the device's lock file) or abandoned after a disturbed launch (the
 * call was repeated on the five-launch layer). */
int biogpt_hip_xpipe_state(const biogpt_hip_ctx *ctx);

int biogpt_hip_get_hparams(const biogpt_hip_ctx *ctx, biogpt_hip_hparams *out);
int biogpt_hip_n_tensors(const biogpt_hip_ctx *ctx); /* tensors found in the file (389 for BioGPT) */

/* vocab / merges as read from the file (biogpt.cpp:72-156); pointers stay valid until free */
int biogpt_hip_vocab_token(const biogpt_hip_ctx *ctx, int32_t id, const char **bytes, int32_t *len);
int biogpt_hip_merge(const biogpt_hip_ctx *ctx, int32_t rank, const char **bytes, int32_t *len);

/* ---- eval ---------------------------------------------------------------------------------
 * One forward pass over n_tokens tokens at offset n_past; writes the LAST token's n_vocab logits
 * to host memory.  Replaces biogpt_eval (biogpt.cpp:812-847): same op order, no intra-chunk
 * causal mask (F1), K/V rows appended to the F32 cache at [n_past, n_past+n_tokens).
 * Requires 0 <= n_past, n_past + n_tokens <= n_positions, ids in [0, n_vocab).
 * n_threads of the reference has no meaning here and is not a parameter. */
int biogpt_hip_eval(biogpt_hip_ctx *ctx, const int32_t *tokens, int32_t n_tokens, int32_t n_past,
                    float *logits_out);

/* biogpt_eval (biogpt.cpp:812-847) without the final copy: *row_out points at the context's pinned host buffer that the launch
 * itself wrote the n_vocab logits of the last token into (valid until the next call on this context).  A loop of single-token calls
 * (main.cpp:91-151) -- through this entry or biogpt_hip_eval -- is served by ONE pipelined launch that stays on the device between
 * the calls and takes each next token from a pinned mailbox; it leaves the device after BIOGPT_HIP_RESIDENT_US
 * (default 1000) microseconds without a call, or as soon as the context is asked to do anything else. */
int biogpt_hip_eval_inplace(biogpt_hip_ctx *ctx, const int32_t *tokens, int32_t n_tokens, int32_t n_past,
                            const float **row_out);

/* The launch behind a loop of single-token evals may run AHEAD of a greedy caller: once four consecutive calls have named exactly the
 * arg-max of the row before (lowest id on ties -- what std::max_element over the logits returns, main.cpp:109-128 with top_k = 1), the
 * launch starts the next position from its own arg-max while the caller still reads the row, and the next call only confirms the token
 * (any other token / position ends that launch, costs one token's time, and doubles the number of matching calls needed before the
 * next attempt -- up to 64; BIOGPT_HIP_SPEC=0 switches it off).  Results are the same either way.  out4 = {calls served by a pass that was already
 * running, calls that named a different token than the running pass, current run of matching calls, matches needed}. */
int biogpt_hip_resident_stats(const biogpt_hip_ctx *ctx, int64_t *out4);

/* biogpt_eval with 2 .. 8 tokens -- the chunks of the reference's prompt loop (main.cpp:129-137, n_batch = 8) -- of a BioGPT-base-shaped block-quantized
 * (Q4_0 .. Q8_0) model at up to 256 keys runs as ONE persistent launch with one column per XCD (csrc/kernels_xcols.hip.h; BIOGPT_HIP_XCOLS=0: the launch chain of
 * kernels_fast.hip.h; same results bit for bit).  biogpt_hip_generate_greedy_batch with 2 .. 8 sequences runs its decode steps through the same kernel (one sequence per
 * XCD, its own K / V cache: no exchange between XCDs) while contexts stay within 256 keys.  Returns how many such launches this context has enqueued or captured (evals;
 * batched generation: one per captured context bucket + the first step) (-1: null context). */
int64_t biogpt_hip_chunk_launches(const biogpt_hip_ctx *ctx);
/* Launches of the many-column chain (q/k/v, out_proj, fc1, fc2, the all-rows lm_head) that went to the matrix-core kernels, counted as they are enqueued or
 * captured; -1: ctx is NULL.  A pass below the column threshold, a context without the row-tiled image and an lm_head whose rows are no multiple of 16 stay on
 * the 8-column kernels and do not count. */
int64_t biogpt_hip_mfma_launches(const biogpt_hip_ctx *ctx);
/* Which many-column layer chain the file has: 0 none (float weights, a head size other than 64, widths the tiles do not divide: the calls over column states
 * refuse it), 1 the BioGPT-base chain (block-quantized, d_model 1024, d_ff 4096), 2 the wide chain -- any other block-quantized file with head size 64, d_model a
 * multiple of 64 and d_ff of 32 (BioGPT-Large: 1600 / 6400): its passes over column states run their linear stages on the int8 matrix cores at every column
 * count, from a row-tiled weight image whose last lm_head tile is zero-padded; 3 the float chain -- an F32 / F16 file of the wide chain's widths, and only
 * while biogpt_hip_float_chain has switched it on for this context (a float file is 0 otherwise); 4 the SIMD chain -- a context in the SIMD association
 * (biogpt_hip_assoc, mode 1) while biogpt_hip_assoc_chain has switched it on (a context in mode 1 is 0 otherwise).  -1: ctx is NULL. */
int biogpt_hip_chain_kind(const biogpt_hip_ctx *ctx);
/* Linear-stage launches of the wide chain (q/k/v, out_proj, fc1, fc2, the all-rows lm_head), counted as they are enqueued or captured; 0 for ever on a
 * BioGPT-base file.  -1: ctx is NULL. */
int64_t biogpt_hip_wide_launches(const biogpt_hip_ctx *ctx);
/* The float chain's switch (off by default; BIOGPT_HIP_FLOAT_CHAIN=1 makes on the default of new contexts whose file can have it).  on 1: the calls over column
 * states the wide chain serves (score_batch, embed_batch, score_continuations, generate_greedy_batch, generate_sample, generate_beam / _beam_batch, the plain
 * generate_queue) serve this F32 / F16 file: its passes over column states run their linear stages on csrc/kernels_fchain.hip.h, which reads the file's own
 * row-major weights (no second image) with the oracle's arithmetic (f32-rounded products, a double sum, one rounding); biogpt_hip_chain_kind returns 3.  The
 * context's own passes (biogpt_hip_eval, score, hidden, generate_greedy, prompt chunks) are untouched, and every other call over column states refuses the
 * context by name.  on 0: the file is what it was without the switch, call by call and message by message.  Legal only for F32 / F16 weights with head size 64,
 * d_model a multiple of 64 and d_ff of 32, and not while a queue session is open or a call of the context is running.  Drops the captured column steps.
 * Returns 0, or -1 with a message (biogpt_hip_last_error) that names the reason. */
int biogpt_hip_float_chain(biogpt_hip_ctx *ctx, int on);
/* The association's switch: in which order the context sums.  mode 0 (the default) is ggml's SCALAR association, the context as it ever was.  mode 1 is the
 * SIMD association -- the logits, K / V rows and greedy ids of an AVX2 build of the reference, what the oracle computes with bo_opts.assoc = 3: activation
 * rows quantized with id = 127 / amax and nearest-even rounding, block dots in eight fma lanes, attention dots in 4 x 8 f32 fma lanes
 * (csrc/kernels_assoc.hip.h).  A context in mode 1 runs every pass as five launches per layer on those kernels: no fused, pipelined, chunk or resident launch,
 * no chain (biogpt_hip_chain_kind returns 0).  It serves the single-sequence calls -- biogpt_hip_eval and its _inplace / _device / _all / _topk / _prompt forms,
 * score, hidden, generate_greedy, biogpt_eval of the compat layer -- with contexts of up to 1024 tokens, and refuses every call over column states (the batched,
 * queue, beam, prefix, lookup, contrastive, trie and rules calls, embed_batch, score_batch) before any launch, with a message that names the call and the
 * association.  Mode 0 after mode 1 is bit for bit the context it was.  Legal for Q4_0 / Q4_1 / Q5_0 / Q5_1 / Q8_0 files with head size 64, d_model and d_ff
 * multiples of 32 (an F32 / F16 file is refused with a message that names the file type), and not while a queue session is open or a call of the context is
 * running.  Synchronises the stream, ends a resident launch, drops every captured graph.  BIOGPT_HIP_ASSOC=1 makes mode 1 the default of new contexts whose
 * file can have it.  Returns 0, -1 with a message (biogpt_hip_last_error), -2 on a HIP error. */
int biogpt_hip_assoc(biogpt_hip_ctx *ctx, int mode);
/* The context's association: 0 scalar, 1 SIMD.  -1: ctx is NULL. */
int biogpt_hip_get_assoc(const biogpt_hip_ctx *ctx);
/* The SIMD chain's switch (off by default; BIOGPT_HIP_ASSOC_CHAIN=1 makes on the default of new contexts whose file can have it).  It is a property of the
 * context that takes effect only while the context is in the SIMD association: in mode 0 a context with the switch set is bit for bit and launch for launch a
 * mode-0 context.  on 1, in mode 1: the calls over column states the wide and float chains serve (score_batch, embed_batch, score_continuations,
 * generate_greedy_batch, generate_sample, generate_beam / _beam_batch, the plain generate_queue) serve this context in the SIMD association -- every sequence's
 * logits, K / V rows and ids are those of the single-sequence calls of mode 1, i.e. of an AVX2 build of the reference.  Its passes over column states run on
 * csrc/kernels_schain.hip.h: one Q8 producer launch per linear stage, a many-column stage in which a thread owns whole (row, column) pairs, and the SIMD
 * attention over column states, with contexts of up to 1024 keys; biogpt_hip_chain_kind returns 4; a biogpt_hip_generate_greedy_batch of 2 .. 8 sequences takes no
 * column-per-XCD launch.  The context's own passes are untouched, and every other call over column states (prefix generation, log-probabilities, rules, trie,
 * contrastive, lookup, the wide sampler, score_continuations_batch, queue prefix / requests / sessions, the beam queue) refuses the context before any launch,
 * with a message that names the call and the SIMD chain.  on 0: a context in mode 1 is what it was without the switch, call by call and message by message.
 * Legal wherever biogpt_hip_assoc(ctx, 1) is (an F32 / F16 file is refused by file type), and not while a queue session is open or a call of the context is
 * running.  Drops the captured column steps.  Returns 0, -1 with a message (biogpt_hip_last_error), -2 on a HIP error. */
int biogpt_hip_assoc_chain(biogpt_hip_ctx *ctx, int on);
/* The SIMD chain's switch: 0 off, 1 on (whatever the association).  -1: ctx is NULL. */
int biogpt_hip_get_assoc_chain(const biogpt_hip_ctx *ctx);
/* Linear-stage launches of the SIMD chain (q/k/v, out_proj, fc1, fc2, the all-rows lm_head), counted as they are enqueued or captured; 0 for ever while the
 * switch is off.  -1: ctx is NULL. */
int64_t biogpt_hip_simd_chain_launches(const biogpt_hip_ctx *ctx);
/* Linear-stage launches of the float chain (q/k/v, out_proj, fc1, fc2, the all-rows lm_head), counted as they are enqueued or captured; 0 for ever while the
 * switch is off.  -1: ctx is NULL. */
int64_t biogpt_hip_float_launches(const biogpt_hip_ctx *ctx);
/* F32 / F16 files: single-token steps this context has enqueued (or captured into a replayed step) as ONE persistent launch for all layers (csrc/kernels_fpipe.hip.h);
 * -1: that launch is not available to this context (shape, device, BIOGPT_HIP_FPIPE=0, or abandoned after a failed launch) -- five launches per layer then */
int64_t biogpt_hip_fpipe_launches(const biogpt_hip_ctx *ctx);
/* Diagnostics of that launch (BIOGPT_HIP_FPIPE_STAMPS=1): stage-border times (s_memrealtime, 100 MHz) of workgroups 0, 128 and 255 of the LAST launch, [3][32 layers][32]:
 * entries 0..8 the first computing wave (A in, A out, B in, C in, C dot, D in, D out, E in, E dot), 16..21 the polling wave (inputs of A, B, C, D, E first / second half seen).
 * Returns the number of values copied, -1 when the launch or the option is not active. */
int biogpt_hip_fpipe_stamps(biogpt_hip_ctx *ctx, uint64_t *out, int n);
/* the last biogpt_hip_generate_greedy call (the loop main.cpp:91-151 with --top_k 1): how many multi-token pipelined launches it took and the tokens of each (up to cap);
 * 0 when every token was a launch / graph replay of its own.  Measurement aid: per-launch durations of a kernel trace divide by these. */
int biogpt_hip_generate_launches(const biogpt_hip_ctx *ctx, int32_t *tokens_out, int cap);

/* Same pass, logits stay in HBM (no PCIe); biogpt_hip_logits_device() returns the device pointer
 * to the n_vocab floats of the last evaluated token.  eval_device is asynchronous on the
 * context's stream; biogpt_hip_synchronize() waits for it. */
int          biogpt_hip_eval_device(biogpt_hip_ctx *ctx, const int32_t *tokens, int32_t n_tokens, int32_t n_past);
const float *biogpt_hip_logits_device(const biogpt_hip_ctx *ctx);
int          biogpt_hip_read_logits(biogpt_hip_ctx *ctx, float *out);   /* waits for the context's work, then copies that device row (n_vocab floats) to host memory */
int          biogpt_hip_synchronize(biogpt_hip_ctx *ctx);

/* biogpt_eval + the top-k selection of biogpt_sample_top_k_top_p (biogpt.cpp:929-936) on the device: evaluates like
 * biogpt_hip_eval and returns the k <= 64 largest logits of the last token (descending; equal logits: lower id first)
 * and their ids (main.cpp:98-128 only ever samples from the top_k = 40 candidates).  A prompt chunk: the selection runs on the device and
 * 512 bytes instead of the 170 KB row cross PCIe.  A single token -- the caller's loop: the resident launch of biogpt_hip_eval_inplace serves
 * the call and the same selection runs in one pass over the pinned row on the host (no launch per call).  Returns k (clamped to n_vocab) or < 0. */
int biogpt_hip_eval_topk(biogpt_hip_ctx *ctx, const int32_t *tokens, int32_t n_tokens, int32_t n_past, int32_t k,
                         float *vals_out, int32_t *ids_out);

/* All-rows variant used by parity tests: logits_out is [n_tokens][n_vocab] on the host
 * (the reference computes all rows and returns the last, biogpt.cpp:803,844; F8). */
int biogpt_hip_eval_all(biogpt_hip_ctx *ctx, const int32_t *tokens, int32_t n_tokens, int32_t n_past,
                        float *logits_out);

/* Prompt ingestion: the result of calling biogpt_hip_eval() on consecutive chunks of n_batch tokens
 * (main.cpp:129-137 with -b n_batch) -- same KV rows, same logits for the last token, bit for bit -- but several
 * chunks travel through the layers per pass (column i only attends to the keys its own chunk would have seen),
 * so the weights are streamed once per pass of up to 512 tokens (BIOGPT_HIP_PROMPT_COLS) instead of once per n_batch.  logits_out may be NULL: the call
 * is then asynchronous (biogpt_hip_logits_device() / biogpt_hip_synchronize()). */
int biogpt_hip_eval_prompt(biogpt_hip_ctx *ctx, const int32_t *tokens, int32_t n_tokens, int32_t n_past, int32_t n_batch,
                           float *logits_out);

/* Greedy generation harness = main.cpp:91-151 with --top_k 1: prompt fed in chunks of n_batch,
 * then n_predict (clamped to n_positions - n_prompt, main.cpp:82) tokens are sampled by arg-max
 * (lowest id wins ties) and fed back, all inside HBM (one captured hipGraph replay per token).
 * out_ids receives the sampled ids; *seconds_out (may be NULL) the wall time of the eval part
 * (main.cpp:96-103 equivalent: prompt evals + decode evals, the last sampled token is not
 * evaluated).  Returns the number of ids written, negative on error. */
int biogpt_hip_generate_greedy(biogpt_hip_ctx *ctx, const int32_t *prompt, int32_t n_prompt,
                               int32_t n_batch, int32_t n_predict, int32_t *out_ids,
                               double *seconds_out);

/* Batched greedy generation: n_seqs independent sequences decoded together on ONE device, one activation
 * column per sequence (own F32 KV cache, own position), so every weight byte is read once per step for all
 * sequences.  Each sequence's ids are identical to what biogpt_hip_generate_greedy() returns for it alone
 * (per-column arithmetic is unchanged).  No counterpart in the reference (it decodes one sequence); this is
 * the single-GPU form of "independent prompts" sharding.  prompts = the prompts concatenated,
 * prompt_lens[n_seqs] their lengths; n_predict is clamped to n_positions - max(prompt_lens); out_ids is
 * [n_seqs][returned n_predict].  Needs the BioGPT-base fast chain (block-quantized weights); n_seqs <= 512 (each
 * sequence owns a full F32 KV cache: 192 MiB at BioGPT-base); from 48 sequences the chain runs on the int8 matrix cores. */
int biogpt_hip_generate_greedy_batch(biogpt_hip_ctx *ctx, const int32_t *prompts, const int32_t *prompt_lens,
                                     int32_t n_seqs, int32_t n_batch, int32_t n_predict, int32_t *out_ids,
                                     double *seconds_out);

/* Beam search for one prompt: transformers' GenerationMixin._beam_search with do_sample = False, one EOS id (eos_id = -1: none), no logits
 * processors (biogpt_hip_generate_beam_rules below adds them), early_stopping 0 / 1 and any length_penalty ("Beam search").  The n_beams running beams decode together as the
 * columns of biogpt_hip_generate_greedy_batch, each in its own K / V cache; the log-softmax and top-2B of every beam row, the selection, the
 * pool of finished hypotheses and the K / V copies of forked beams run on the device inside the captured step (csrc/kernels_beam.hip.h).
 * The prompt is ingested in chunks of n_batch, as biogpt_hip_generate_greedy does; n_beams = 1 with eos_id = -1 returns its ids.
 * n_predict is clamped to n_positions - n_prompt (main.cpp:82).  Writes the finished hypotheses best first: out_ids [n_beams][n_predict]
 * (entries past a hypothesis's length are -1; an EOS that ended it is included), out_lens[n_beams] generated tokens, out_scores[n_beams]
 * normalized scores (sum of log-probabilities / length^length_penalty).  The context's own K / V cache and position are left alone.  Needs
 * the BioGPT-base fast chain (block-quantized weights), like biogpt_hip_generate_greedy_batch; anything else fails with -1.  Returns n_beams
 * (hypotheses written), 0 if n_predict clamps to 0, < 0 on error (argument errors, -1, come before any HIP call). */
int biogpt_hip_generate_beam(biogpt_hip_ctx *ctx, const int32_t *prompt, int32_t n_prompt, int32_t n_batch,
                             int32_t n_beams /* 1..16 */, int32_t n_predict, int32_t eos_id /* -1: none */,
                             float length_penalty, int32_t early_stopping /* 0/1 */,
                             int32_t *out_ids /* [n_beams][n_predict] */, int32_t *out_lens, float *out_scores,
                             double *seconds_out);

/* Sampled generation, batched: n_samples continuations of each of n_prompts prompts, drawn by the reference's sampler (biogpt_sample_top_k_top_p,
 * biogpt.cpp:908-980) on the device inside the captured decode step (csrc/kernels_sample.hip.h).  Sequence r = p * n_samples + j is sample j of
 * prompt p and is what main.cpp:91-151 produces for that prompt with --seed seeds[r] --top_k --top_p --temp -b n_batch (its own std::mt19937(seeds[r])),
 * stopped after the first eos_id if one is given ("Sampled generation": scale = 1 / temp and all probability arithmetic in double;
 * candidates by value descending, lower id first on equal values; top-p cut at the first cumsum >= top_p, then the renormalisation; libstdc++'s
 * discrete_distribution with one generate_canonical<double, 53>; no draw when fewer than two candidates are left).  The device's exp() is not glibc's:
 * the ids equal the reference loop's unless a draw lies within a few ulp of a partial-sum border or a cumulative sum within a few ulp of top_p.
 * prompts = the prompts concatenated, prompt_lens[n_prompts] their lengths (a prompt is evaluated once, its K / V rows copied to its other samples);
 * n_predict is clamped to n_positions - max(prompt_lens).  out_ids is [n_prompts * n_samples][returned n_predict] with -1 after a sequence's end,
 * out_lens its generated tokens (an EOS that ended it included).  n_prompts * n_samples in [1, 512]; top_k in [1, 64]; temp finite and > 0; top_p
 * finite (>= 1: no cut); eos_id in [-1, n_vocab).  The context's own K / V cache, position and logits row are left alone.  Needs the BioGPT-base fast
 * chain (block-quantized weights), like biogpt_hip_generate_greedy_batch; anything else fails with -1.  Returns the clamped n_predict, 0 if that is
 * <= 0, < 0 on error (argument errors, -1, come before any HIP call). */
int biogpt_hip_generate_sample(biogpt_hip_ctx *ctx, const int32_t *prompts, const int32_t *prompt_lens, int32_t n_prompts,
                               int32_t n_samples, int32_t n_batch, int32_t n_predict, int32_t top_k, double top_p, double temp,
                               const uint32_t *seeds /* [n_prompts * n_samples] */, int32_t eos_id /* -1: none */,
                               int32_t *out_ids, int32_t *out_lens, double *seconds_out);

/* The sampler's tail on the host (no device, no context; the function the kernel runs): state625 = the 624 words of std::mt19937(seed) + the index of
 * the next output (624 after seeding).  biogpt_hip_sample_candidates_host draws from k candidates already in selection order (vals: their f32
 * logits, best first; ids: their token ids), advancing the state in place.  Both return 0 or -1. */
int biogpt_hip_mt19937_seed(uint32_t seed, uint32_t *state625);
int biogpt_hip_sample_candidates_host(const float *vals, const int32_t *ids, int32_t k, double top_p, double temp,
                                      uint32_t *mt_state625, int32_t *id_out);

/* sample_rows_kernel over n_rows <= 4096 logits rows of n_vocab floats held in host memory: row r is drawn from with the state mt_states[r * 625 ..]
 * (advanced in place; a block of outputs regenerated on the device holds the words the host's form would).  For tests of the kernel itself. */
int biogpt_hip_sample_rows_device(int device, const float *logits, int32_t n_rows, int32_t n_vocab, int32_t top_k, double top_p, double temp,
                                  uint32_t *mt_states, int32_t *ids_out);

/* ---- generation rules: transformers' logits processors of the same names, on the device inside the captured step (csrc/kernels_rules.hip.h;
 * INTEGRATION.md, "Generation rules").  For a row whose sequence so far is h = prompt + generated tokens, L = len(h), values s:
 *   repetition_penalty p    every DISTINCT token t of h, once: s[t] = s[t] < 0 ? s[t] * p : s[t] / p (f32, IEEE division)
 *   no_repeat_ngram_size n  if L + 1 >= n: every i in [0, L - n] with h[i .. i+n-2] == h[L-n+1 .. L-1] bans h[i+n-1] (s = -inf); n = 1 bans every token seen
 *   min_new_tokens m        with an EOS id and fewer than m tokens generated: s[eos] = -inf (ignored without an EOS id)
 *   suppress                s[t] = -inf for each listed id, every step
 * The history includes the prompt.  The penalty is applied first.  biogpt_hip_generate_sample_rules applies the rules to the raw logits row, in
 * front of the reference's sampler (top_k = 1 never draws: greedy decoding with rules and an EOS); biogpt_hip_generate_beam_rules applies them to
 * the row's log-probabilities, after the log-softmax and before the top-2B, as transformers' _beam_search does (banned tokens stay in the
 * normalising sum; the penalty multiplies negative log-probabilities). */
typedef struct biogpt_hip_gen_rules {
    float repetition_penalty;      /* 1.0 off; finite, > 0 */
    int32_t no_repeat_ngram_size;  /* 0 off; <= n_positions */
    int32_t min_new_tokens;        /* 0 off */
    int32_t n_suppress;            /* 0 .. 256 */
    const int32_t *suppress;       /* ids in [0, n_vocab) */
} biogpt_hip_gen_rules;

/* biogpt_hip_generate_beam / biogpt_hip_generate_sample with rules.  rules == NULL, or a struct with every rule off: the result of the function
 * without rules, bit for bit, through the same launches and captured steps (a step with rules is a captured graph of its own; the values of the
 * rules live in device memory, not in the graph).  Argument errors (-1, the message names the field) come before any HIP call.  For beam search a
 * rule set that could leave a row with fewer than 2 x n_beams finite candidates (a banning rule active and
 * n_vocab - n_suppress - 1 - n_positions < 2 * n_beams) is an argument error. */
int biogpt_hip_generate_beam_rules(biogpt_hip_ctx *ctx, const int32_t *prompt, int32_t n_prompt, int32_t n_batch,
                                   int32_t n_beams, int32_t n_predict, int32_t eos_id, float length_penalty, int32_t early_stopping,
                                   int32_t *out_ids, int32_t *out_lens, float *out_scores, double *seconds_out,
                                   const biogpt_hip_gen_rules *rules);
int biogpt_hip_generate_sample_rules(biogpt_hip_ctx *ctx, const int32_t *prompts, const int32_t *prompt_lens, int32_t n_prompts,
                                     int32_t n_samples, int32_t n_batch, int32_t n_predict, int32_t top_k, double top_p, double temp,
                                     const uint32_t *seeds, int32_t eos_id, int32_t *out_ids, int32_t *out_lens, double *seconds_out,
                                     const biogpt_hip_gen_rules *rules);

/* Beam search over a batch of prompts in one call: n_prompts independent searches of n_beams beams each, as the n_prompts * n_beams columns of one
 * batched decode step (group g owns the columns and K / V cache slots [g * n_beams, (g + 1) * n_beams)).  The selection, the pool of finished
 * hypotheses, the stopping rules, the slot assignment and the K / V copies of forked beams run per group on the device inside the captured step
 * (csrc/kernels_beam.hip.h); a finished group leaves its state alone while the others go on.  prompts = the prompts concatenated,
 * prompt_lens[n_prompts] their lengths (a prompt is evaluated once, its K / V rows copied to its group's other slots); n_predict is clamped to
 * n' = n_positions - max(prompt_lens).  For prompt p the result is what
 *   biogpt_hip_generate_beam_rules(prompt p, n_batch, n_beams, n', eos_id, length_penalty, early_stopping, rules)
 * returns, hypothesis for hypothesis, ids and f32 scores bit for bit (n_prompts = 1 is biogpt_hip_generate_beam).  rules == NULL: none.
 * out_ids is [n_prompts][n_beams][returned n_predict] (-1 past a hypothesis's length and in rows past a prompt's count), out_lens and out_scores
 * [n_prompts][n_beams], out_counts[n_prompts] the hypotheses written per prompt.  n_beams in [1, 16]; n_prompts * n_beams in [1, 512] (each column
 * owns a full F32 KV cache); the other arguments as biogpt_hip_generate_beam_rules checks them.  The context's own K / V cache, position and logits
 * row are left alone.  Needs the BioGPT-base fast chain (block-quantized weights); anything else fails with -1.  Returns the clamped n_predict, 0 if
 * that is <= 0, < 0 on error (argument errors, -1, the message names the field, come before any HIP call). */
int biogpt_hip_generate_beam_batch(biogpt_hip_ctx *ctx, const int32_t *prompts /* concatenated */, const int32_t *prompt_lens, int32_t n_prompts,
                                   int32_t n_batch, int32_t n_beams, int32_t n_predict, int32_t eos_id, float length_penalty, int32_t early_stopping,
                                   const biogpt_hip_gen_rules *rules /* NULL: none */,
                                   int32_t *out_ids /* [n_prompts][n_beams][returned n_predict], -1 filled */, int32_t *out_lens /* [n_prompts][n_beams] */,
                                   float *out_scores /* [n_prompts][n_beams] */, int32_t *out_counts /* [n_prompts]: hypotheses returned */, double *seconds_out);

/* rules_rows_kernel over n_rows <= 4096 rows of n_vocab floats held in host memory.  mode 0: the rows are logits; mode 1: each row becomes its
 * log-probabilities first, (float)(((double)l - max) - log(sum exp(l - max))).  Row r's history is hist_lens[r] tokens of hist (the histories
 * concatenated), the first prompt_lens[r] of them its prompt.  rows_out: [n_rows][n_vocab].  For tests of the kernel itself. */
int biogpt_hip_rules_rows_device(int device, int32_t mode /* 0 logits, 1 log-probabilities */, const float *rows, int32_t n_rows, int32_t n_vocab,
                                 const int32_t *hist /* concatenated */, const int32_t *hist_lens, const int32_t *prompt_lens, int32_t eos_id,
                                 const biogpt_hip_gen_rules *rules, float *rows_out);

/* ---- trie-constrained generation: output restricted to a closed set of token sequences (entity names, labels of a schema), transformers'
 * prefix_allowed_tokens_fn / PrefixConstrainedLogitsProcessor over a trie, on the device inside the captured step (csrc/trie_host.cpp,
 * csrc/kernels_trie.hip.h; INTEGRATION.md, "Constrained decoding").
 *
 * The definition.  Let g be the tokens generated so far (the prompt excluded).  Walk g from the root:
 *   the walk ends at node u       A = {tokens of u's edges} + {eos_id if an entry ends at u}
 *   the walk leaves the trie      A = {eos_id}      (only a beam that took a candidate at -inf gets there)
 * A is never empty.  The masked row is s[t] for t in A and -inf elsewhere.
 *
 * biogpt_hip_trie_build: n_seqs >= 1 entries, concatenated in seqs, entry i of lens[i] >= 1 tokens in [0, n_vocab).  Duplicates merge; an entry may
 * be a prefix of another.  NULL (biogpt_hip_last_error() names the argument) for zero entries, an empty entry or an id out of range.  Host only: no
 * HIP call.  The layout is CSR: node u's edges are [first[u], first[u + 1]) of tok (ascending) and child, a terminal flag per node, and a bitmap of
 * the tokens that occur anywhere.  The device copy is made at the first use on a device and freed with the handle: free it after the contexts that
 * used it are idle.  A handle may serve any number of calls and contexts, one call at a time. */
typedef struct biogpt_hip_trie biogpt_hip_trie;
biogpt_hip_trie *biogpt_hip_trie_build(const int32_t *seqs /* concatenated */, const int32_t *lens, int32_t n_seqs, int32_t n_vocab);
void biogpt_hip_trie_free(biogpt_hip_trie *trie);
/* out: entries after merging, nodes, edges, the longest entry (max depth), the largest number of edges of a node (max fan-out) */
int biogpt_hip_trie_info(const biogpt_hip_trie *trie, int64_t out[5]);
/* The allowed set A after the generated tokens gen[0 .. n_gen), ascending, into out_ids (the first cap of them); returns its size, -1 on an argument
 * error.  eos_id in [0, n_vocab).  This function is the definition the kernel restates. */
int biogpt_hip_trie_allowed_host(const biogpt_hip_trie *trie, const int32_t *gen, int32_t n_gen, int32_t eos_id, int32_t *out_ids, int32_t cap);

/* biogpt_hip_generate_beam_batch with every beam row masked by the trie: the row becomes its log-probabilities (the normalising sum over the
 * UNMASKED row, as in transformers' _beam_search) and -inf outside A, then the selection runs.  Candidates at -inf are legal: they are ordered by the
 * existing rule (score, parent rank, token id), can become running beams or pool entries, and hypotheses with score -inf are returned as they are --
 * keep the ones with a finite score, and choose n_predict >= max depth + 1 so that entries can finish.  Every finite hypothesis that ends in eos_id is
 * an entry of the trie.  eos_id >= 0 is required and must occur in no entry; the trie's n_vocab must be the model's; trie == NULL is an argument
 * error (the functions without a trie exist); everything else as biogpt_hip_generate_beam_batch checks it.  No rules parameter: rules together with
 * a trie are not supported.  A step with a trie is a captured graph of its own that serves any trie (its arrays are named in device memory). */
int biogpt_hip_generate_beam_trie(biogpt_hip_ctx *ctx, const int32_t *prompts /* concatenated */, const int32_t *prompt_lens, int32_t n_prompts,
                                  int32_t n_batch, int32_t n_beams, int32_t n_predict, int32_t eos_id, float length_penalty, int32_t early_stopping,
                                  biogpt_hip_trie *trie, int32_t *out_ids, int32_t *out_lens, float *out_scores, int32_t *out_counts, double *seconds_out);
/* biogpt_hip_generate_sample with every unfinished sequence's logits row masked by the trie in front of the sampler; top_k = 1 is constrained greedy
 * decoding.  Candidates at -inf carry weight 0.  Arguments as above and as biogpt_hip_generate_sample checks them. */
int biogpt_hip_generate_sample_trie(biogpt_hip_ctx *ctx, const int32_t *prompts /* concatenated */, const int32_t *prompt_lens, int32_t n_prompts,
                                    int32_t n_samples, int32_t n_batch, int32_t n_predict, int32_t top_k, double top_p, double temp,
                                    const uint32_t *seeds, int32_t eos_id, biogpt_hip_trie *trie, int32_t *out_ids, int32_t *out_lens, double *seconds_out);
/* trie_rows_kernel over n_rows <= 4096 rows of n_vocab floats held in host memory.  mode 0: logits; mode 1: the members of A become log-probabilities.
 * Row r's generated tokens are hist_lens[r] tokens of hist.  rows_out: [n_rows][n_vocab].  For tests of the kernel itself and tools. */
int biogpt_hip_trie_rows_device(int device, biogpt_hip_trie *trie, int32_t mode, const float *rows, int32_t n_rows, int32_t n_vocab,
                                const int32_t *hist /* generated tokens, concatenated */, const int32_t *hist_lens, int32_t eos_id, float *rows_out);
/* biogpt_hip_trie_rows_device, then reps in [1, 10000] further launches over the same rows (restored on the device in front of each launch);
 * us_out[i]: microseconds between two device events around launch i alone.  For tools/trie_bench.py. */
int biogpt_hip_trie_rows_bench(int device, biogpt_hip_trie *trie, int32_t mode, const float *rows, int32_t n_rows, int32_t n_vocab, const int32_t *hist,
                               const int32_t *hist_lens, int32_t eos_id, float *rows_out, int32_t reps, float *us_out /* [reps] */);
/* One stand-alone attention launch over caller-supplied inputs, through the launch code of the engine's own passes (one layer).  route names the kernel the caller
 * expects: 0 .. 3 attn_fast_kernel<1, true>, <2, false>, <4, false> at 1024 threads and <4, false> as the slim launch, 4 .. 7 their SHARED instantiations,
 * 8 attn_prefix_kernel<8>, 9 the three attn_split_* launches, 10 attn_group_kernel<8>, 11 / 12 attn_tile_kernel<16, true> / <16, false>, 13 attn_kernel.  A
 * combination for which the engine would launch another kernel, or none, returns -1.  q [N][H * dk] (dk = 64 but for route 13); k_slots / v_slots
 * [n_slots][H][P][dk].  Exactly one of dev_state (4 words: n_past, n_gen, causal, chunk; one slot) and seq_states ([N][8] words as the engine's column states;
 * col_mode 0: column i reads slot i and n_past + 1 keys, 1: slot seq_id and t_vis keys; routes 4 .. 8: the first pad[0] rows from slot pad[1]).  t_max: the
 * furthest column's visible keys, from which the launch's load bound follows as in a pass.  The outputs come back whole, as allocated and preset to 0xff bytes:
 * rows = N rounded up to 16, plus 1 -- out [rows][H * dk]; q8 1 / 2: also the rows' Q8_0 / Q8_1 blocks, out_q [rows][H * dk], out_d / out_s [rows][H * dk / 32].
 * launched [8] (may be NULL): kernel (as route), threads, grid x, grid y, dynamic LDS bytes, t_cap, key ranges (route 9), 0.  For tests of the kernels themselves. */
int biogpt_hip_attn_device(int device, int32_t route, int32_t H, int32_t dk, int32_t N, int32_t P, int32_t t_max, int32_t n_slots, const float *q,
                           const float *k_slots, const float *v_slots, const int32_t *dev_state, const int32_t *seq_states, int32_t col_mode, int32_t q8, float *out,
                           int8_t *out_q, float *out_d, uint32_t *out_s, int32_t *launched);
/* One stand-alone launch of a linear stage of the many-column chain over caller-supplied inputs, through the launch code of the engine's own passes.  op: 0 LNQ
 * (LayerNorm + Q8 of N rows of 1024; q81 picks the Q8_1 form; route -1), 1 QKV, 2 OPROJ, 3 FC1_LN (one column, LayerNorm fused), 4 FC1_Q8, 5 FC2, 6 LMHEAD.  route
 * names the kernel the caller expects: 0 the 1-column VALU kernel, 1 the 8-column one, 2 / 3 the matrix-core kernel with one / two row tiles per wave.  A route the
 * engine would not take for (op, type, M, N, column states), a shape that is not the site's own (q/k/v 3072 x 1024, out_proj 1024 x 1024, fc1 4096 x 1024, fc2
 * 1024 x 4096; only lm_head's M is free) and two columns that write one (slot, position) return -1 before anything is allocated.  w_rows: M rows in the file's
 * block format (wtype 2, 3, 6, 7, 8).  (Only op 1 carries column states: there routes 2 / 3 need 64 columns for a pass and 48 for a decode step, col_mode 0; the other
 * ops accept them from 48 columns on, as in a decode step.)  Inputs by op: x [N][1024], ln_w, ln_b [1024] (ops 0, 3); aq_q [N][K] int8, aq_d [N][K / 32], aq_s [N][K / 32] in the
 * device layout of a producer's Q8 blocks (all others); bias [M] (not 0, 6); resid [N][M] (2, 5); op 1: exactly one of dev_state (4 words; one slot) and
 * seq_states ([N][8] words; col_mode 0: column i writes slot i, 1: slot seq_id) at position n_past, and one layer's k_slots / v_slots [n_slots][16][P][64],
 * updated in place.  The outputs come back whole, as allocated and preset to 0xff bytes: cols = N rounded up to 16, plus 1; ldo = M rounded up to 128, plus 16 --
 * out [cols][ldo] (op 1: the q rows, [cols][1024]); ops 0, 3, 4: out_q [cols][M'], out_d / out_s [cols][M' / 32] with M' = 1024 (op 0) or 4096.
 * launched [8] (may be NULL): kernel (as route), threads, grid x, grid y, dynamic LDS bytes, cols, ldo, 0.  For tests of the kernels themselves. */
int biogpt_hip_chain_device(int device, int32_t op, int32_t route, int32_t wtype, int32_t M, int32_t N, const void *w_rows, const float *x, const float *ln_w,
                            const float *ln_b, int32_t q81, const int8_t *aq_q, const float *aq_d, const uint32_t *aq_s, const float *bias, const float *resid,
                            const int32_t *dev_state, const int32_t *seq_states, int32_t col_mode, int32_t P, int32_t n_slots, float *k_slots, float *v_slots,
                            float *out, int8_t *out_q, float *out_d, uint32_t *out_s, int32_t *launched);
/* One stand-alone launch of the wide chain's linear stage over caller-supplied weights and Q8 columns, through the launch code of the engine's own passes: the
 * row-tiled image is built as for a wide file (ceil(M / 16) tiles, the last one zero-padded).  epi: 0 QKV (M == 3 K, 64 | K: K is d_model, heads of 64), 1 RESID,
 * 2 GELU (f32 rows through the fp16 table), 3 LOGITS; K a multiple of 32; 16 | M but for LOGITS.  w_rows: M rows of K / 32 blocks in the file's format (wtype 2, 3,
 * 6, 7, 8); aq_q [N][K] int8, aq_d [N][K / 32], aq_s [N][K / 32] in the device layout of a producer's Q8 blocks; bias [M] (not 3); resid [N][M] (1); epi 0: exactly
 * one of dev_state (4 words; one slot) and seq_states ([N][8] words; col_mode 0: column i writes slot i, 1: slot seq_id) at position n_past, and one layer's
 * k_slots / v_slots [n_slots][K / 64][P][64], updated in place.  out comes back whole, as allocated and preset to 0xff bytes: cols = N rounded up to 16, plus 1;
 * epi 0: [cols][K] (the q rows), otherwise [cols][ldo] with ldo = M rounded up to 128, plus 16.  launched [8] (may be NULL): threads, grid x, grid y, LDS bytes,
 * cols, ldo, row tiles, 0.  For tests of the kernel itself and tools. */
int biogpt_hip_wide_chain_device(int device, int32_t epi, int32_t wtype, int32_t M, int32_t K, int32_t N, const void *w_rows, const int8_t *aq_q, const float *aq_d,
                                 const uint32_t *aq_s, const float *bias, const float *resid, const int32_t *dev_state, const int32_t *seq_states, int32_t col_mode,
                                 int32_t P, int32_t n_slots, float *k_slots, float *v_slots, float *out, int32_t *launched);
/* A linear stage alone, timed: one untimed launch, then reps in [1, 10000] launches on device memory of arbitrary contents, us_out[i]: microseconds between two
 * device events around launch i alone.  which 0: the wide chain's kernel with the residual epilogue at M rows (16 | M) of K values (32 | K) and N <= 512 columns;
 * which 1: the BioGPT-base matrix-core kernel at out_proj (M 1024, K 1024) or fc2 (M 1024, K 4096).  For tools/wide_chain_bench.py. */
int biogpt_hip_wide_chain_bench(int device, int32_t which, int32_t wtype, int32_t M, int32_t K, int32_t N, int32_t reps, float *us_out);
/* One stand-alone launch of the float chain's linear stage over caller-supplied weights and f32 columns, through the launch code of the engine's own passes.
 * epi: 0 QKV (M == 3 K, 64 | K: K is d_model, heads of 64), 1 RESID, 2 GELU (f32 rows through the fp16 table), 3 LOGITS; K a multiple of 32; any M.  wtype 0:
 * w_rows is M rows of K f32, 1: of K f16 (bits); x [N][K] f32; ln_w / ln_b [K] (both or neither): the LayerNorm producer runs in front of the stage; cfg 0 .. 2: a
 * tile shape (4 rows x 8 columns, 32 x 8, 64 x 16 a workgroup), -1 the launch's own choice; bias [M] (not 3); resid [N][M] (1); epi 0: exactly one of dev_state (4
 * words; one slot) and seq_states ([N][8] words; col_mode 0: column i writes slot i, 1: slot seq_id) at position n_past, and one layer's k_slots / v_slots
 * [n_slots][K / 64][P][64], updated in place.  out comes back whole, as allocated and preset to 0xff bytes: cols = N rounded up to 16, plus 1; epi 0: [cols][K]
 * (the q rows), otherwise [cols][ldo] with ldo = M rounded up to 128, plus 16; ln_out (may be NULL) [cols][K]: the producer's rows, likewise.  launched [8] (may
 * be NULL): threads, grid x, grid y, LDS bytes, cols, ldo, cfg, 0.  For tests of the kernel itself and tools. */
int biogpt_hip_fchain_device(int device, int32_t epi, int32_t wtype, int32_t M, int32_t K, int32_t N, int32_t cfg, const void *w_rows, const float *x, const float *ln_w,
                             const float *ln_b, const float *bias, const float *resid, const int32_t *dev_state, const int32_t *seq_states, int32_t col_mode, int32_t P,
                             int32_t n_slots, float *k_slots, float *v_slots, float *out, float *ln_out, int32_t *launched);
/* One stand-alone launch of a kernel of the SIMD association (csrc/kernels_assoc.hip.h) over caller-supplied inputs, through the launch functions of a context
 * in mode 1 (biogpt_hip_assoc).  No model, no context.  wtype: a block format (2 / 3 / 6 / 7 / 8); K a multiple of 32.
 * stage 0 Q8: x [N][K], N in [1, 8]; ln_w / ln_b [K] (both or neither): the LayerNorm in front.  out_q [N + 1][K] the codes, out_d [N + 1][K / 32] the scale
 *   the dot reads (through f16 for Q4_0 / Q5_0 / Q8_0 weights; f32 for Q4_1 / Q5_1), out_s [N + 1][K / 32] words: the integer sum, or the bits of d * sum.
 * stage 1 MATVEC: matvec_simd_kernel on w_rows (M rows of K / 32 blocks in the file's format) and x [N][K], N in [1, 8]; (pro, epi) one of (1 LN, 0 QKV),
 *   (0 PLAIN, 1 RESID), (1, 2 GELU), (1, 3 LOGITS); ln_w / ln_b with pro 1; bias [M] (not 3); resid [N][M] (1).  epi 0: M == 3 K, 64 | K, dev_state (4 words)
 *   and one layer's k_slots / v_slots [K / 64][P][64], updated in place; out [N + 1][K] the q rows.  Otherwise out [N + 1][M + 16].  epi 3 with N == 1:
 *   pmax_val / pmax_idx [1025] (both or neither) the arg-max partial of every workgroup's rows.
 * stage 2 ATTN: attn_simd_kernel on q [N][H * 64], N in [1, 512], k_slots / v_slots [H][P][64] and dev_state {n_past, n_gen, causal, chunk}: column i sees
 *   the keys every attention kernel would show it, 1 .. 1024 and at most P.  out [N + 1][H * 64].
 * Outputs come back whole, as allocated and preset to 0xff bytes.  launched [8] (may be NULL): stage 0 / 1: threads, grid x, grid y, dynamic LDS bytes,
 * columns per workgroup, rows per workgroup; stage 2: 17, threads, grid x, grid y, static LDS bytes.  Every refusal comes before any HIP call.  For tests of
 * the kernels themselves and tools/assoc_bench.py. */
int biogpt_hip_assoc_device(int device, int32_t stage, int32_t wtype, int32_t pro, int32_t epi, int32_t M, int32_t K, int32_t N, int32_t H, int32_t P, const void *w_rows,
                            const float *x, const float *ln_w, const float *ln_b, const float *bias, const float *resid, const int32_t *dev_state, const float *q,
                            float *k_slots, float *v_slots, float *out, int8_t *out_q, float *out_d, uint32_t *out_s, float *pmax_val, int32_t *pmax_idx,
                            int32_t *launched);
/* A kernel of the SIMD association alone, timed: one untimed launch, then reps in [1, 10000] launches on device memory of arbitrary contents, us_out[i]:
 * microseconds between two device events around launch i alone.  which 0: matvec_simd_kernel with the residual epilogue at M rows of K values (32 | K) and
 * N <= 512 columns; which 1: the mat-vec a context in the scalar association launches at the same shape on its five-launch route -- the yardstick; which 2:
 * attn_simd_kernel with M heads, N query columns under the causal mask, the last of which sees K keys (N <= K <= 1024).  For tools/assoc_bench.py. */
int biogpt_hip_assoc_bench(int device, int32_t which, int32_t wtype, int32_t M, int32_t K, int32_t N, int32_t reps, float *us_out);
/* The kernels of the SIMD chain alone (csrc/kernels_schain.hip.h), through the launch functions a pass over column states of a context on the SIMD chain uses.  No
 * model, no context.  wtype: a block format (2 / 3 / 6 / 7 / 8); K a multiple of 32; N in [1, 512].
 *   stage 0 Q8: the producer over x [N][K], behind the LayerNorm when ln_w / ln_b are given: out_q [N + 1][K] codes, out_d [N + 1][K / 32] the scale the dot
 *     reads, out_s [N + 1][K / 32] words (Q8_0 form: the integer sum; Q8_1 form, for Q4_1 / Q5_1: bits of d * sum).
 *   stage 1 STAGE: the producer, then the many-column linear stage at tile shape cfg (0: 64 rows x 4 columns, 1: x 16, 2: x 32; -1: the launch's own choice).
 *     epi 0 QKV (M == 3 K, 64 | K; exactly one of dev_state {n_past, ..} and seq_states [N][8] (+ col_mode) names the column states; k_slots / v_slots
 *     [n_slots][K / 64][P][64] are updated in place; out = the q rows [cols][K]), 1 RESID (bias, resid [N][M]), 2 GELU (bias), 3 LOGITS; any M.  out but for QKV:
 *     [cols][ldo]; cols = N rounded up to 32, plus one guard column; ldo = M rounded up to 64, plus 16 guard rows.
 *   stage 2 ATTN: the SIMD attention over column states: q [N][H * 64], k_slots / v_slots [n_slots][H][P][64], seq_states [N][8]: column i reads slot i and
 *     n_past + 1 keys (col_mode 0) or slot seq_id and t_vis keys (col_mode 1), at most 1024 and at most P; shared 1: its rows j < pad[0] come from slot pad[1].
 *     out [N + 1][H * 64].
 * The outputs come back WHOLE as allocated and preset to 0xff bytes.  launched [8]: stage 0 / 2: threads, grid x, grid y, LDS bytes; stage 1: threads, grid x,
 * grid y, static LDS bytes, cols, ldo, cfg, columns of a tile.  Returns 0, -1 on a bad argument (before any HIP call), -2 on a HIP error. */
int biogpt_hip_schain_device(int device, int32_t stage, int32_t wtype, int32_t epi, int32_t M, int32_t K, int32_t N, int32_t cfg, int32_t H, int32_t P, int32_t n_slots,
                             int32_t col_mode, int32_t shared, const void *w_rows, const float *x, const float *ln_w, const float *ln_b, const float *bias,
                             const float *resid, const int32_t *dev_state, const int32_t *seq_states, const float *q, float *k_slots, float *v_slots, float *out,
                             int8_t *out_q, float *out_d, uint32_t *out_s, int32_t *launched);
/* A linear stage of the SIMD association alone, timed (microseconds of reps launches, each between two device events; one untimed launch in front).  which 0:
 * the SIMD chain's stage with the residual epilogue at tile shape cfg (-1: the launch's choice); 1: its Q8 producer; 2: the SIMD mat-vec a context's own pass in
 * mode 1 launches at N columns; 3: the wide chain's matrix-core stage of the scalar association (M a multiple of 16), for scale.  tools/simd_chain_bench.py. */
int biogpt_hip_schain_bench(int device, int32_t which, int32_t wtype, int32_t M, int32_t K, int32_t N, int32_t cfg, int32_t reps, float *us_out);
/* One stand-alone run of a stage of the embedding tail (ln_rows_kernel<1024> / <0>, pool_rows_kernel, pool_finish_kernel, head_rows_kernel) over caller-supplied
 * rows, through the launch code of biogpt_hip_hidden / biogpt_hip_embed_batch.  No model, no context; W a multiple of 4.  stage 0 LN: x [n_rows][W], ln_w / ln_b
 * [W]; W == 1024 takes the <1024> template, any other width <0>; seq_states (may be NULL) [n_rows][8] words with slot_div >= 1 and P: row i lands at row
 * (seq_id / slot_div) * P + n_past of n_out_rows (no two on one row); without them n_out_rows == n_rows.  out [n_out_rows + 1][W].  stage 1 POOL: mode 0 none,
 * 1 last, 2 mean; x: the rows of n_passes passes of pass_cols[p] columns one behind the other (n_rows in all), seq_states [n_rows][8] words (seq_id, n_past),
 * lens [n_seqs]: within a pass a sequence's columns are consecutive, at consecutive positions below its length, and end at its last position or with the pass.  pool_rows_kernel runs once per pass in stream
 * order (mean: on an accumulator zeroed first), then pool_finish_kernel when there is a mean or normalize; out [n_seqs + 1][W]; acc (mean) [n_seqs + 1][W]
 * doubles.  Mode 0 (with normalize): the rows themselves are normalised, out [n_rows + 1][W].  stage 2 HEAD: x [n_rows][W], w [n_out][W], b [n_out] or NULL,
 * n_out in [1, 256], 8 * W * 4 bytes within the 65536 of LDS a launch gets; out [n_rows + 1][n_out].  Outputs come back whole, as allocated and preset to 0xff
 * bytes: the last row is a guard row.  launched [8] (may be NULL): the kernel (ln_rows_kernel's template argument 1024 / 0, 1 pool_rows_kernel, 3
 * head_rows_kernel), threads, grid x, grid y, dynamic LDS bytes (POOL: the last pass's launch), pool_finish_kernel's grid (0: not launched), pool_rows_kernel
 * launches, 0.  For tests of the kernels themselves. */
int biogpt_hip_embed_device(int device, int32_t stage, int32_t W, int32_t n_rows, const float *x, const float *ln_w, const float *ln_b, const int32_t *seq_states,
                            int32_t slot_div, int32_t P, int32_t n_out_rows, int32_t mode, int32_t normalize, const int32_t *lens, int32_t n_seqs, int32_t n_passes,
                            const int32_t *pass_cols, const float *w, const float *b, int32_t n_out, float *out, double *acc, int32_t *launched);
/* One stand-alone run of a stage of the token tail -- the kernels every generated id of the single-stream path leaves through, and the host selections of
 * biogpt_hip_eval_topk -- over caller-supplied inputs, through the launch code of the engine's own calls.  No model, no context.  The tail's order: larger value
 * first; equal values, lower id first; a NaN is never before anything and nothing is before it.  n is M (stage 0), the number of partials (1) or V (2 .. 5).
 * stage 0 PARTIALS: the single-token lm_head launch (final LayerNorm + one column of K = 1024, whichever kernel the type and M get) on w_rows, n <= 131072 rows in
 * the file's format (wtype 0 F32, 2 / 3 / 6 / 7 / 8 the block formats), x / ln_w / ln_b [1024].  out_val [n + 16]: the logits row; part_val / part_idx [n + 16]:
 * the arg-max partial of each workgroup's rows.  launched: {kernel: 0 lm_stream_kernel, 1 matvec_fast_kernel, 2 matvec_kernel; partials written; rows per partial}.
 * stage 1 FINISH: argmax_kernel on part_in_val / part_in_idx [n], n in [1, 4096], and a state block of the probe's own: state [4] (n_past, n_gen >= 0, causal,
 * chunk), n_eval, n_positions in [1, 4096], n_vocab >= 1.  out_idx [4 + 2 n_positions + 16]: the block after the kernel -- the four words, tokens [n_positions]
 * (word 0: the next token), gen_ids [n_positions], 16 guard words; all but the four words preset to 0xff.  launched: {256, 1}.
 * stage 2 TOPK: topk_kernel on row [n], n <= 1048576, part_in_val [nparts] (nparts in [1, 4096]; any values: the answer never depends on them, only whether there
 * is one), k in [1, min(64, n)].  out_val / out_idx [80]: the pairs, part_idx [16]: word 0 is k, or -1 (more than 4096 logits reach the threshold, or fewer than k
 * values are comparable).  launched: {1024, 1}.
 * stage 3 HOST_TOPK, 4 HOST_BLOCKS, 5 HOST_FULL: the host selections on the same arguments and outputs, with NO HIP call (they run without a device) -- the one
 * pass over the row; the walk over the 64-row blocks whose maximum (part_in_val [nparts], nparts == ceil(n / 64), the TRUE maxima of the row's blocks as the
 * resident launch writes them behind the row) can hold a candidate; the partial sort of the whole row that answers when topk_kernel gives -1 (NaNs behind every
 * comparable value, by id).  part_idx word 0: the count found (3, 4: < k only when fewer than k values are comparable) or k (5).
 * Device outputs come back whole, as allocated and preset to 0xff bytes; the host stages preset theirs alike.  launched [8] may be NULL.  For tests of the tail itself. */
int biogpt_hip_tail_device(int device, int32_t stage, int32_t wtype, int32_t n, const void *w_rows, const float *x, const float *ln_w, const float *ln_b, const float *row,
                           const float *part_in_val, const int32_t *part_in_idx, int32_t nparts, int32_t k, const int32_t *state, int32_t n_eval, int32_t n_positions,
                           int32_t n_vocab, float *out_val, int32_t *out_idx, float *part_val, int32_t *part_idx, int32_t *launched);
/* A linear stage of a float file alone, timed: one untimed launch, then reps in [1, 10000] launches on device memory of ordinary values, us_out[i]: microseconds between
 * two device events around launch i alone.  which 0: the float chain's kernel with the residual epilogue at M rows of K values (32 | K), N <= 512 columns and
 * tile shape cfg (-1: the launch's choice); which 1: the generic mat-vec kernel, as a prompt pass of the context's own columns launches it.  For
 * tools/float_chain_bench.py. */
int biogpt_hip_fchain_bench(int device, int32_t which, int32_t wtype, int32_t M, int32_t K, int32_t N, int32_t cfg, int32_t reps, float *us_out);
/* One decode attention launch of N columns behind a shared prefix over caller-supplied inputs (head size 64, one layer): q [N][H * 64]; k_slots / v_slots
 * [N + 1][H][P][64], slot i column i's own and slot N the prefix's; seq_states [N][8] words as the engine's column states (n_past, ..., pad[0] = shared rows,
 * pad[1] = their slot).  which 0: the existing attn_fast_kernel<4, false, true>; 1: attn_prefix_kernel<8>, eight columns per workgroup (one shared range for
 * all columns); t_cap a multiple of 64, or P.  out [N][H * 64]; q8 1 / 2: also the rows' Q8_0 / Q8_1 blocks (out_q [N][H * 64], out_d / out_s [N][H * 2]), 0: none (the three may be NULL).
 * For tests of the kernel itself and tools. */
int biogpt_hip_attn_prefix_device(int device, int32_t H, int32_t N, int32_t P, int32_t t_cap, const float *q, const float *k_slots, const float *v_slots,
                                  const int32_t *seq_states, int32_t which, int32_t q8, float *out, int8_t *out_q, float *out_d, uint32_t *out_s);
/* biogpt_hip_attn_prefix_device, then reps in [1, 10000] further launches on the same inputs; us_out[i]: microseconds between two device events around
 * launch i alone (the K / V rows are in cache from the launch before).  For tools/prefix_gen_bench.py. */
int biogpt_hip_attn_prefix_bench(int device, int32_t H, int32_t N, int32_t P, int32_t t_cap, const float *q, const float *k_slots, const float *v_slots,
                                 const int32_t *seq_states, int32_t which, int32_t q8, float *out, int8_t *out_q, float *out_d, uint32_t *out_s, int32_t reps,
                                 float *us_out /* [reps] */);
/* The planner of attn_runs_kernel: the N packed column states of a pass (seq_states [N][8] words, col_mode 1) walked greedily into runs of up to eight
 * consecutive columns whose first R visible rows are the same rows of one slot S.  runs_out [N][4]: c0, n, R, S.  Returns the number of runs, or -1. */
int biogpt_hip_attn_runs_plan(const int32_t *seq_states, int32_t N, int32_t *runs_out /* [N][4]: c0, n, R, S */);
/* One attn_runs_kernel<8> launch over caller-supplied inputs through the engine's launch helper (head size 64, one layer, P <= 1024): q [N][H * 64];
 * k_slots / v_slots [n_slots][H][P][64]; seq_states [N][8] packed column states (slot seq_id, t_vis keys, the first pad[0] of them in slot pad[1]); t_max the
 * furthest visible key count.  runs [n_runs][4] or NULL (the planner's table): a caller's table is validated before anything is allocated -- every column in
 * exactly one run, n <= 8, the first R rows of every member really in S and its other rows in its own slot -- and refused with -1 otherwise.  The outputs are
 * returned whole as biogpt_hip_attn_device returns them (N rounded up to 16 rows plus a guard row, preset to 0xff; q8 1 / 2: the Q8_0 / Q8_1 blocks too).
 * launched [8] (may be NULL): kernel (16), threads, grid x, grid y, LDS bytes, t_cap, runs, 0.  For tests of the kernel itself. */
int biogpt_hip_attn_runs_device(int device, int32_t H, int32_t N, int32_t P, int32_t t_max, int32_t n_slots, const float *q, const float *k_slots,
                                const float *v_slots, const int32_t *seq_states, const int32_t *runs /* may be NULL */, int32_t n_runs, int32_t q8, float *out,
                                int8_t *out_q, float *out_d, uint32_t *out_s, int32_t *launched);
/* The same, then reps in [1, 10000] further launches on the same inputs; us_out[i]: microseconds around launch i alone.  For tools/prefix_batch_bench.py. */
int biogpt_hip_attn_runs_bench(int device, int32_t H, int32_t N, int32_t P, int32_t t_max, int32_t n_slots, const float *q, const float *k_slots,
                               const float *v_slots, const int32_t *seq_states, const int32_t *runs /* may be NULL */, int32_t n_runs, int32_t q8, float *out,
                               int8_t *out_q, float *out_d, uint32_t *out_s, int32_t *launched, int32_t reps, float *us_out /* [reps] */);
/* biogpt_hip_beam_rows_device with given = 1 over rows of which any number of values may be -inf, as a trie step leaves them (entries at -inf become
 * candidates, lower id first, where fewer than 2 * n_beams finite ones are left).  For tests of the kernel itself. */
int biogpt_hip_beam_rows_masked_device(int device, const float *rows, int32_t n_rows, int32_t n_vocab, int32_t n_beams, const float *run_score,
                                       int32_t first_step, float *cand_score, int32_t *cand_col, int32_t *cand_id);

/* logprob_rows_kernel (the log-softmax of biogpt_hip_score and of every beam score) over n_rows <= 4096 rows of n_vocab floats held in host memory,
 * row stride n_vocab: an odd n_vocab puts consecutive rows on the four 16-byte alignments.  targets[r] in [-1, n_vocab); for row r the outputs are
 * what biogpt_hip_score documents for a row: lp_out, argmax_out (lowest id on ties), logit_out; target -1 gives lp = logit = 0.  For tests of the
 * kernel itself. */
int biogpt_hip_logprob_rows_device(int device, const float *rows, int32_t n_rows, int32_t n_vocab, const int32_t *targets, float *lp_out,
                                   int32_t *argmax_out, float *logit_out);

/* beam_group_rows_kernel over n_rows <= 512 rows of n_vocab >= 2 * n_beams floats held in host memory, launched by the dispatch a call uses
 * (the 8 / 16 / 32-entry instantiation by n_beams; given = 1: the rows hold log-probabilities and are taken as they are, each with at least
 * 2 * n_beams finite values).  Row r is column r % n_beams of group r / n_beams and run_score[r] the score of the beam in it; n_rows is a multiple of
 * n_beams.  Outputs are [n_rows][2 * n_beams], best candidate first: cand_score = (float)(run_score + lp), cand_col = the column within the group,
 * cand_id the token.  Every entry is a sentinel (score NaN, col = id = -1) before the launch: with first_step = 1 only a group's row 0 is expanded
 * and the other rows keep it.  For tests of the kernel itself. */
int biogpt_hip_beam_rows_device(int device, const float *rows, int32_t n_rows, int32_t n_vocab, int32_t given, int32_t n_beams, const float *run_score,
                                int32_t first_step, float *cand_score, int32_t *cand_col, int32_t *cand_id);

/* A whole beam search over the beam kernels with the model replaced by a lookup: the row of a column whose token is t is table[t % n_table_rows]
 * (table: [n_table_rows][n_vocab], logits, or log-probabilities with given = 1), and the K / V row it leaves at its position p in its cache slot
 * (1 layer, 2 heads of 4 floats, P = max(prompt_lens) + n_predict positions) is the stamp {t, p, 2 * head + (0 K | 1 V),
 * (t + 7 p + 3 head + (0 | 1)) & 0xffff}.  Group g starts as a call with a prompt of prompt_lens[g] tokens ending in start_tokens[g] does.  Runs at
 * most max_steps steps (row, select and fork kernels through the step code of biogpt_hip_generate_beam_batch), fewer if every group finishes.
 * out_ids [n_groups][n_beams][n_predict], out_lens, out_scores, out_counts: as biogpt_hip_generate_beam_batch writes them, by the same read-out,
 * if every group has finished (returns n_predict); else they are emptied and the call returns 0.  The state after the last step, always:
 * col_token, col_n_gen, col_run_score, col_rank [n_groups * n_beams], col_hist [n_groups * n_beams][n_predict] (-1 where nothing was written),
 * grp_done, grp_step [n_groups], kv_out [2 K | V][n_groups * n_beams][2][P][4] (-1 where no step has written).  < 0 on error (argument errors, -1,
 * the message names the argument, come before any HIP call).  For tests of the kernels themselves. */
int biogpt_hip_beam_table_device(int device, const float *table, int32_t n_table_rows, int32_t n_vocab, int32_t given, const int32_t *start_tokens,
                                 const int32_t *prompt_lens, int32_t n_groups, int32_t n_beams, int32_t n_predict, int32_t eos_id, float length_penalty,
                                 int32_t early_stopping, int32_t max_steps, int32_t *out_ids, int32_t *out_lens, float *out_scores, int32_t *out_counts,
                                 int32_t *col_token, int32_t *col_n_gen, int32_t *col_hist, float *col_run_score, int32_t *col_rank, int32_t *grp_done,
                                 int32_t *grp_step, float *kv_out);

/* Contrastive search (Su et al. 2022; transformers' generate(penalty_alpha, top_k)): n_prompts deterministic searches in one call.  Group g owns the
 * top_k columns and K / V cache slots [g * top_k, (g + 1) * top_k) and a context store H_g: one f32 hidden row (biogpt_hip_hidden's row, after the
 * final LayerNorm) per context token and its squared norm as a double.  The prompt pass (chunks of n_batch) leaves the rows of prompt tokens
 * 0 .. L - 2 in H_g; the first step evaluates the last prompt token, appends its row, and its logits row l gives the first candidates: the top_k
 * largest values (value descending, lower id first on ties), p_j = (float)(exp((double)l_j - (double)m) / S) with the row maximum m and exponential
 * sum S of biogpt_hip_score's log-softmax.  Every later step feeds candidate j to column j at position len(H_g), which gives its hidden row h_j
 * and logits row; pen_j = max_i sim(h_j, H_g[i]), sim(a, b) = (float)(dot / sqrt(na * nb)) from double sums of exact f32 products (0 if a norm is 0);
 * score_j = (float)((1 - (double)alpha) * (double)p_j - (double)alpha * (double)pen_j); the winner is the highest score, the lowest j on ties.
 * Its id is the next token, its row joins H_g, its logits row gives the next candidates, its K / V row of that position is copied to the group's
 * other slots.  A winner equal to eos_id ends the group (the EOS is part of the output).  n generated tokens take n + 1 steps; n_predict is
 * clamped to n' = n_positions - max(prompt_lens).  A prompt's result does not depend on what else is in the call; top_k = 1 or penalty_alpha = 0
 * give the ids of biogpt_hip_generate_greedy_batch.  No rules or warpers.  out_ids is [n_prompts][returned n_predict] (-1 past a prompt's length),
 * out_lens [n_prompts], out_scores (may be NULL) [n_prompts][returned n_predict] the winning score of every token (0 past the length).
 * top_k in [1, 16], penalty_alpha in [0, 1], n_prompts * top_k in [1, 512] (each column owns a full F32 KV cache), eos_id in [-1, n_vocab).  The
 * context's own K / V cache, position and logits row are left alone.  Needs the BioGPT-base fast chain (block-quantized weights); anything else
 * fails with -1.  Returns the clamped n_predict, 0 if that is <= 0, < 0 on error (argument errors, -1, the message names the field, come before
 * any HIP call; -2 names the size of a context store that did not fit). */
int biogpt_hip_generate_contrastive(biogpt_hip_ctx *ctx, const int32_t *prompts /* concatenated */, const int32_t *prompt_lens, int32_t n_prompts,
                                    int32_t n_batch, int32_t top_k, float penalty_alpha, int32_t n_predict, int32_t eos_id /* -1: none */,
                                    int32_t *out_ids /* [n_prompts][returned n_predict], -1 filled */, int32_t *out_lens /* [n_prompts] */,
                                    float *out_scores /* [n_prompts][returned n_predict], may be NULL */, double *seconds_out);

/* The penalty and selection kernels of contrastive search over rows held in host memory, no model: k <= 16 candidate rows and T context rows of d
 * floats (4 | d, d <= 1024), probs[k] and alpha as above.  pen_out[k], score_out[k], *winner_out.  For tests of the kernels themselves. */
int biogpt_hip_contrast_rank_device(int device, const float *cand /* [k][d] */, const float *ctx_rows /* [T][d] */, int32_t k, int32_t T, int32_t d,
                                    const float *probs /* [k] */, float alpha, float *pen_out, float *score_out, int32_t *winner_out);

/* Prompt-lookup speculative decoding (transformers' generate(prompt_lookup_num_tokens = max_draft, max_matching_ngram_size = max_ngram); llama.cpp's
 * lookup): greedy decoding of n_prompts prompts whose ids are those of biogpt_hip_generate_greedy_batch, bit for bit, in fewer forward passes where the
 * output copies from text the sequence already holds.  Sequence p's text T is corpus_p ++ prompt_p ++ its generated tokens, of length L; corpus_p
 * (corpus_lens[p] ids of the concatenated `corpus`; both NULL: none) is material likely to be copied and is never evaluated.  Before every pass, for
 * n = max_ngram down to 1: the i in [0, L - n - 1] with T[i .. i + n) == T[L - n .. L); the largest n with a match wins, among its matches the smallest
 * i.  The draft is T[i + n .. i + n + d), d = min(max_draft, L - (i + n), n_predict - n_gen - 1); no match: d = 0.  The pass evaluates the current
 * token and the d drafted tokens at consecutive positions (each sees the keys up to its own position), a_j is the arg-max of row j (lowest id on
 * ties); the longest m with draft[j] == a_j for all j < m is accepted and a_0 .. a_m are appended, cut at n_predict and behind the first eos_id.
 * out_ids is [n_prompts][returned n_predict] (-1 past a prompt's length), out_lens [n_prompts], out_stats (may be NULL) [n_prompts][3]: passes,
 * drafted tokens, drafted tokens that reached the output (so a prompt's length is passes + accepted).  A prompt's ids and stats do not depend on what
 * else is in the call.  max_draft in [0, 15] (0: biogpt_hip_generate_greedy_batch itself), max_ngram in [1, 8], n_prompts * (1 + max_draft) in
 * [1, 512] and at most n_positions, eos_id in [-1, n_vocab), corpus ids in [0, n_vocab), sum(corpus_lens) + n_prompts * n_positions <= 2^21.  The
 * context's own K / V cache, position and logits row are left alone.  Needs the BioGPT-base fast chain (block-quantized weights); anything else
 * fails with -1.  Returns n_predict as clamped to n_positions - max(prompt_lens), 0 if that is <= 0, < 0 on error (argument errors, -1, the
 * message names the field, come before any HIP call). */
int biogpt_hip_generate_lookup(biogpt_hip_ctx *ctx, const int32_t *prompts /* concatenated */, const int32_t *prompt_lens, int32_t n_prompts,
                               const int32_t *corpus /* concatenated, may be NULL */, const int32_t *corpus_lens /* may be NULL */, int32_t n_batch,
                               int32_t n_predict, int32_t max_draft, int32_t max_ngram, int32_t eos_id /* -1: none */,
                               int32_t *out_ids /* [n_prompts][returned n_predict], -1 filled */, int32_t *out_lens /* [n_prompts] */,
                               int32_t *out_stats /* [n_prompts][3], may be NULL */, double *seconds_out);

/* ---- generation over a queue (continuous batching): finished columns are refilled from a queue of requests ----
 * n_requests requests (prompts concatenated, prompt_lens their lengths) share C = min(max_columns, eligible requests) columns and K / V cache slots: a
 * request takes a column when one is free and leaves it when it finishes, by EOS or at its own limit.  Request r's ids and length are those of
 * biogpt_hip_generate_sample(its prompt alone, n_samples 1, n_r, the same top_k / top_p / temp / eos_id / n_batch, seeds[r]), bit for bit, with
 * n_r = min(n_predicts[r], n_positions - prompt_lens[r]): the clamp is per request.  What else is in the queue, max_columns and group change nothing but the
 * time.  top_k = 1 never draws: greedy decoding with an EOS.  A request with n_r == 0 gets length 0 and never takes a column.  n_predicts == NULL: n_predict
 * for every request.  out_ids is [n_requests][n_predict] (n_predict is the row stride as GIVEN, not clamped) with -1 behind a request's length; out_lens
 * the generated tokens (an EOS that ended a request included).  out_admit_step[r] (may be NULL): the steps run before r's first step; out_column[r] (may be
 * NULL): its column; both -1 for a request that never ran.  The schedule is deterministic in steps (biogpt_hip_queue_plan computes it from the lengths
 * alone): requests are admitted in index order, steps run in groups of `group`, behind each group the host looks at the columns and refills the
 * finished ones, lowest column first.  stats (may be NULL): columns = C; steps; groups; admissions = refill rounds, the first included; prompt_columns =
 * prompt tokens evaluated; busy_column_steps = the sum of out_lens; column_steps = C * steps.  n_requests is limited by host memory alone: prompts stay on
 * the host until admitted.  max_columns in [1, 512], group in [1, 64], n_predicts[r] in [0, n_predict], top_k in [1, 64], temp finite and > 0, top_p finite,
 * eos_id in [-1, n_vocab), no empty prompt, prompt_lens[r] <= n_positions.  The context's own K / V cache, position and logits row are left alone.  Needs
 * the BioGPT-base fast chain (block-quantized weights); anything else fails with -1.  No rules, trie or several samples per request (a shared prefix and
 * log-probabilities: biogpt_hip_generate_queue_prefix; rules, stop sequences and a sampler per request: biogpt_hip_generate_queue_requests); the steps always run as the launch chain.  Returns 0, or < 0 on error (argument errors, -1, the message names the field, come before any HIP
 * call). */
typedef struct biogpt_hip_queue_stats {
    int32_t columns, steps, groups, admissions, prompt_columns;
    int64_t busy_column_steps, column_steps;
} biogpt_hip_queue_stats;

int biogpt_hip_generate_queue(biogpt_hip_ctx *ctx, const int32_t *prompts /* concatenated */, const int32_t *prompt_lens, int32_t n_requests,
                              const int32_t *n_predicts /* [n_requests], or NULL: n_predict for all */,
                              int32_t n_predict /* row stride of out_ids; every n_predicts[r] <= n_predict */, int32_t max_columns /* 1 .. 512 */,
                              int32_t group /* steps between two looks at the columns, 1 .. 64 */, int32_t n_batch, int32_t top_k, double top_p, double temp,
                              const uint32_t *seeds /* [n_requests] */, int32_t eos_id /* -1: none */,
                              int32_t *out_ids /* [n_requests][n_predict], -1 behind a request's length */, int32_t *out_lens,
                              int32_t *out_admit_step /* may be NULL */, int32_t *out_column /* may be NULL */, double *seconds_out,
                              biogpt_hip_queue_stats *stats /* may be NULL */);

/* The scheduler of biogpt_hip_generate_queue alone, on the host: no context, no HIP call.  gen_lens[r] = the tokens request r generates (0: it never takes a
 * column) -- the schedule of a call whose requests all run to their limits, and of a call with an EOS wherever no group was cut short by limits that
 * an EOS undercut.  admit_step / column [n_requests] and stats as above; prompt_columns stays 0 (the plan knows no prompts).  Returns 0 or -1. */
int biogpt_hip_queue_plan(const int32_t *gen_lens, int32_t n_requests, int32_t max_columns, int32_t group, int32_t *admit_step, int32_t *column,
                          biogpt_hip_queue_stats *stats /* may be NULL */);
/* The same scheduler for requests that may end before their limits, as a run drives it: limits[r] = the tokens request r may generate at most (n_r above; 0: it
 * never takes a column), gen_lens[r] <= limits[r] the tokens it generates (>= 1 where limits[r] > 0).  A group is min(group, the most tokens any running request
 * may STILL generate under its limit) -- the host of a run does not know where a request will end -- and a look finds finished whoever has generated its
 * gen_lens[r] tokens.  This is the schedule of every run of biogpt_hip_generate_queue and biogpt_hip_generate_beam_queue (there: steps and slots), with or
 * without an EOS; with limits == gen_lens it is biogpt_hip_queue_plan.  Returns 0 or -1. */
int biogpt_hip_queue_plan_limits(const int32_t *gen_lens, const int32_t *limits, int32_t n_requests, int32_t max_columns, int32_t group, int32_t *admit_step,
                                 int32_t *column, biogpt_hip_queue_stats *stats /* may be NULL */);

/* ---- beam search over a queue: finished searches hand their n_beams columns to the next request ----
 * n_requests requests share S = min(max_columns / n_beams, eligible requests) group slots of n_beams columns and K / V cache slots each: a request's search
 * takes a slot when one is free and leaves it when it stops, by transformers' stopping rules or after its own limit.  Request r's hypotheses, lengths, count
 * and scores are those of biogpt_hip_generate_beam(its prompt alone, n_r, the same n_beams / eos_id / length_penalty / early_stopping / n_batch) -- with a trie,
 * of biogpt_hip_generate_beam_trie of that prompt alone -- bit for bit, with n_r = min(n_predicts[r], n_positions - prompt_lens[r]): the clamp is per
 * request.  What else is in the queue, max_columns and group change nothing but the time.  A request with n_r == 0 gets count 0 and never takes a slot.
 * n_predicts == NULL: n_predict for every request.  out_ids is [n_requests][n_beams][n_predict] (n_predict is the row stride as GIVEN, not clamped), best
 * hypothesis first, -1 behind a hypothesis's length; out_lens / out_scores [n_requests][n_beams]; out_counts [n_requests] the hypotheses held (rows beyond:
 * length 0, score 0).  out_steps[r] (may be NULL): the steps r's search took; out_admit_step[r] (may be NULL): the steps run before its first one;
 * out_slot[r] (may be NULL): its slot; the last two -1 for a request that never ran.  The schedule is biogpt_hip_generate_queue's with slots for columns:
 * biogpt_hip_queue_plan_limits(out_steps, the limits n_r, n_requests, S, group) computes it for every run.  biogpt_hip_queue_plan(out_steps, ...) is the same
 * schedule only where no group was cut short by a limit that an early stop undercut -- always at group = 1 or when every search ran to its limit; after an early
 * stop with group > 1 a run may take more steps than that plan.  stats (may be NULL) count in slots: columns = S; steps; groups;
 * admissions; prompt_columns = prompt tokens evaluated (once per request); busy_column_steps = the sum of out_steps; column_steps = S * steps.
 * Needs 1 <= n_beams <= 16, n_beams <= max_columns <= 512, group in [1, 64], the BioGPT-base fast chain (block-quantized weights) and, with a trie, what
 * biogpt_hip_generate_beam_trie needs.  No generation rules (their history is built per call from the call's prompts), prefix or log-probabilities; the
 * steps always run as the launch chain.  The context's own K / V cache, position and logits row are left alone.  Returns 0, or < 0 on error (argument
 * errors, -1, the message names the field, come before any HIP call). */
int biogpt_hip_generate_beam_queue(biogpt_hip_ctx *ctx, const int32_t *prompts /* concatenated */, const int32_t *prompt_lens, int32_t n_requests,
                                   const int32_t *n_predicts /* [n_requests], or NULL: n_predict for all */,
                                   int32_t n_predict /* row stride of out_ids; every n_predicts[r] <= n_predict */, int32_t n_beams,
                                   int32_t max_columns /* n_beams .. 512 */, int32_t group /* steps between two looks at the slots, 1 .. 64 */, int32_t n_batch,
                                   int32_t eos_id /* -1: none */, float length_penalty, int32_t early_stopping, biogpt_hip_trie *trie /* may be NULL */,
                                   int32_t *out_ids /* [n_requests][n_beams][n_predict] */, int32_t *out_lens, float *out_scores, int32_t *out_counts,
                                   int32_t *out_steps /* may be NULL */, int32_t *out_admit_step /* may be NULL */, int32_t *out_slot /* may be NULL */,
                                   double *seconds_out, biogpt_hip_queue_stats *stats /* may be NULL */);

/* The draft kernel of prompt-lookup decoding over texts held in host memory, no model: sequence s has text_lens[s] tokens of the concatenated `texts`
 * (the last n_gen[s] of them generated, the last one its current token at position n_past[s]); finished (may be NULL): sequences that draft nothing.
 * draft_out [n_seqs][16] (-1 behind the draft), d_out [n_seqs], cols_out [n_seqs][1 + max_draft][4]: token, n_past, seq_id, t_vis of every packed
 * column state (the columns beyond 1 + d repeat column 0).  For tests of the kernel itself. */
int biogpt_hip_lookup_draft_device(int device, const int32_t *texts, const int32_t *text_lens, int32_t n_seqs, const int32_t *n_gen, const int32_t *n_past,
                                   const int32_t *finished, int32_t n_predict, int32_t max_draft, int32_t max_ngram, int32_t *draft_out, int32_t *d_out,
                                   int32_t *cols_out);

/* The accept kernel over logits rows held in host memory: rows [n_seqs * (1 + max_draft)][n_vocab], sequence s with n_gen[s] tokens at position
 * n_past[s] and the draft drafts[s][0 .. d[s]) (stride 16).  emit_out [n_seqs][16] the ids appended (-1 behind them), state_out [n_seqs][4]: the
 * column's token (-1: nothing appended), n_past, n_gen, finished; stats_out [n_seqs][3]: passes, drafted, accepted; live_out [2]: the count of
 * unfinished sequences and the furthest position.  For tests of the kernel itself. */
int biogpt_hip_lookup_accept_device(int device, const float *rows, int32_t n_seqs, int32_t n_vocab, int32_t max_draft, const int32_t *drafts, const int32_t *d,
                                    const int32_t *n_gen, const int32_t *n_past, const int32_t *finished, int32_t n_predict, int32_t eos_id, int32_t *emit_out,
                                    int32_t *state_out, int32_t *stats_out, int32_t *live_out);

/* ---- sequence scoring (no counterpart in the reference) ---------------------------------------
 * biogpt_hip_score: teacher-forced, causal log-probabilities of a sequence.  Row i sees the keys [0, n_past + i] -- what
 * biogpt_hip_eval_prompt(..., n_batch = 1) and a loop of single-token biogpt_hip_eval calls compute; NOT the unmasked chunk of
 * biogpt_hip_eval_all (F1), and independent of BIOGPT_HIP_CAUSAL.  For every row i with targets[i] >= 0, with l = the row's logits,
 * m = max(l), t = targets[i]:  logprob_out[i] = (l[t] - m) - log(sum_v exp(l[v] - m))  (natural log),  logit_out[i] = l[t]  (bit-identical
 * to the row eval_prompt(tokens[0..i], n_past, 1) returns); rows with targets[i] < 0 get 0 in both.  argmax_out[i] = the arg-max of row i
 * (lowest id on ties) for every row.  targets == NULL: next-token scoring, targets[i] = tokens[i + 1] and -1 for the last row.
 * argmax_out and logit_out may be NULL.  Arguments as for biogpt_hip_eval, plus targets[i] < n_vocab.  Afterwards the K / V rows
 * [n_past, n_past + n_tokens) and the device row (biogpt_hip_read_logits) are those biogpt_hip_eval_prompt(..., 1) leaves: a following
 * biogpt_hip_eval at n_past + n_tokens continues the sequence.  Passes of up to BIOGPT_HIP_PROMPT_COLS (512) columns; the log-softmax
 * runs on the device, n_tokens x 12 bytes cross PCIe.  Returns 0 or < 0. */
int biogpt_hip_score(biogpt_hip_ctx *ctx, const int32_t *tokens, int32_t n_tokens, int32_t n_past, const int32_t *targets,
                     float *logprob_out, int32_t *argmax_out, float *logit_out);

/* The same for n_seqs independent sequences, each scored from position 0 in its own K / V cache (the context's own cache and position
 * are left alone): seqs = the sequences concatenated, lens[n_seqs] their lengths (the layout of biogpt_hip_generate_greedy_batch);
 * targets (may be NULL: next-token scoring per sequence) and the outputs use the same flat layout as seqs.  The columns of all sequences
 * travel through common passes of up to BIOGPT_HIP_PROMPT_COLS columns; every sequence's results are bit-identical to
 * biogpt_hip_score(seq, n_past = 0).  Needs the BioGPT-base fast chain (block-quantized weights) and n_seqs <= 512, like
 * biogpt_hip_generate_greedy_batch; anything else fails with -1.  Returns 0 or < 0. */
int biogpt_hip_score_batch(biogpt_hip_ctx *ctx, const int32_t *seqs, const int32_t *lens, int32_t n_seqs, const int32_t *targets,
                           float *logprob_out, int32_t *argmax_out, float *logit_out);

/* Many continuations of ONE prefix (multiple choice, label ranking, reranking hypotheses of one prompt): conts = the n_conts continuations
 * concatenated, cont_lens[n_conts] their lengths; the outputs use the flat layout of conts.  For continuation c and i in [0, cont_lens[c]):
 * logprob_out = log P(cont_c[i] | prefix, cont_c[0..i)), logit_out = that token's logit, argmax_out = the row's arg-max -- rows
 * n_prefix - 1 + i of biogpt_hip_score(prefix + cont_c, 0), bit for bit.  The prefix rows [0, n_prefix - 1) are evaluated ONCE, without an
 * lm_head, into a K / V cache slot that every continuation's attention reads in place; no K / V row is copied.  Every continuation
 * re-evaluates the last prefix token in a slot of its own and its last token is never a column: n_prefix - 1 + sum(cont_lens) columns
 * instead of the sum(n_prefix + cont_lens[c]) of biogpt_hip_score_batch on the concatenations.  The context's own cache, position and
 * logits row are left alone.  Needs the BioGPT-base fast chain (block-quantized weights), like biogpt_hip_score_batch.  Argument errors
 * (null pointers, n_prefix < 1, n_conts outside [1, 511], an empty continuation, a token id out of range, n_prefix + cont_lens[c] >
 * n_positions, a model without the fast chain) return -1 before any HIP call and name the field; a failed allocation returns -2 and names
 * the size.  argmax_out and logit_out may be NULL.  seconds_out (may be NULL): the passes and the copy back.  Returns 0 or < 0. */
int biogpt_hip_score_continuations(biogpt_hip_ctx *ctx, const int32_t *prefix, int32_t n_prefix,
                                   const int32_t *conts /* concatenated */, const int32_t *cont_lens, int32_t n_conts,
                                   float *logprob_out, int32_t *argmax_out /* may be NULL */, float *logit_out /* may be NULL */,
                                   double *seconds_out /* may be NULL */);

/* Several (prefix, continuations) groups in ONE call (a dataset of multiple-choice / yes-no-maybe / reranking examples): prefixes = the n_groups prefixes
 * concatenated, prefix_lens[n_groups] their lengths; conts = all continuations concatenated group by group, n_conts[g] how many group g has, cont_lens
 * [sum n_conts] their lengths.  The outputs use the flat layout of conts; group g's are biogpt_hip_score_continuations(prefix_g, conts_g).  Each prefix's
 * rows [0, n_prefix_g - 1) are evaluated once, without an lm_head, into a K / V slot of their own; every continuation owns a slot, re-evaluates its group's
 * last prefix token and reads the prefix rows in place.  One call holds at most 512 slots: n_groups + sum(n_conts) <= 512.  All prefix columns of all
 * groups, then all continuation columns in flat order, travel in one stream of passes of up to BIOGPT_HIP_PROMPT_COLS columns.
 * BIOGPT_HIP_RUN_ATTN chooses the attention kernel of these passes (no other call looks at it): 0 the per-column kernel of biogpt_hip_score_continuations,
 * 1 attn_runs_kernel (up to eight neighbouring columns that see the same first rows load them once) in every pass of up to 1024 keys, -1 (default) the
 * latter where it was measured faster, by the size of the pass.  What is promised:
 *   RUN_ATTN=0  every group's numbers are those of biogpt_hip_score_continuations(prefix_g, conts_g), bit for bit;
 *   RUN_ATTN=1  a group's numbers do not depend on the other groups, their order or the pass size, bit for bit (they are the per-column kernel's wherever
 *               the double sums of the attention are not within a rounding of a float32 boundary);
 *   default     a pass's kernel depends on its size, so a group's company can move an output by one float32 ulp of one attention output on such a row.
 * Argument errors (null pointers, n_groups < 1, an n_conts[g] < 1, more than 512 slots, a prefix_lens[g] < 1, an empty continuation, a token id out of
 * range, n_prefix_g + cont_len > n_positions, a model without the fast chain) return -1 before any HIP call and name the group and the field; a failed
 * allocation returns -2 and names the size.  The context's own cache, position and logits row are left alone.  Returns 0 or < 0. */
int biogpt_hip_score_continuations_batch(biogpt_hip_ctx *ctx,
        const int32_t *prefixes /* concatenated */, const int32_t *prefix_lens, int32_t n_groups,
        const int32_t *conts /* concatenated, group-major */, const int32_t *cont_lens /* [sum n_conts] */,
        const int32_t *n_conts /* [n_groups] */,
        float *logprob_out, int32_t *argmax_out /* may be NULL */, float *logit_out /* may be NULL */,
        double *seconds_out /* may be NULL */);
/* The last successful biogpt_hip_score_continuations_batch of the context: {prefix columns, continuation columns, passes, passes whose attention ran on
 * attn_runs_kernel}.  Returns 0, or -1 for a null argument. */
int biogpt_hip_prefix_batch_stats(const biogpt_hip_ctx *ctx, int32_t out[4]);

/* ---- generation behind a shared prefix: one long few-shot or instruction block in front of many short inputs, or N samples of one long prompt ----
 * Sequence s is prefix ++ suffix_s (suffixes = the suffixes concatenated, suffix_lens their lengths; a suffix may be empty).  The ids -- for sampling
 * also the lengths -- are those of biogpt_hip_generate_greedy_batch / biogpt_hip_generate_sample on the concatenations with the same n_batch, seeds
 * and n_predict, bit for bit; n_predict is clamped to n_positions - (n_prefix + the longest suffix).  The prefix's first n_shared rows -- the largest
 * multiple of n_batch <= n_prefix - 1, so every n_batch chunk of a concatenation is either shared or a sequence's own -- are evaluated ONCE, without
 * an lm_head, into a K / V slot of their own; every sequence then evaluates prefix[n_shared:] ++ suffix_s only.  The decode steps read the shared
 * rows in place (path 0); where the steps of the plain call run as column-per-XCD launches (2 .. 8 columns, at most 255 prompt tokens) the shared rows
 * are copied into every column's slot instead and the steps are exactly those of the plain call (path 1).  n_shared == 0: the plain call.
 * Columns (n_seqs, n_prompts * n_samples) in [1, 511]: one slot holds the prefix.  Argument errors (null pointers, n_prefix < 1, a token id out of
 * range, n_prefix + suffix_lens[s] > n_positions, a model without the BioGPT-base fast chain, and those of the plain calls) return -1 before any HIP
 * call.  There is no form with generation rules or a trie.  The context's own K / V cache, position and logits row are left alone.  Returns as the
 * plain calls: the clamped n_predict, 0 if that is <= 0, < 0 on error. */
int biogpt_hip_generate_greedy_prefix(biogpt_hip_ctx *ctx, const int32_t *prefix, int32_t n_prefix, const int32_t *suffixes /* concatenated */,
                                      const int32_t *suffix_lens, int32_t n_seqs, int32_t n_batch, int32_t n_predict, int32_t *out_ids,
                                      double *seconds_out /* may be NULL */);
int biogpt_hip_generate_sample_prefix(biogpt_hip_ctx *ctx, const int32_t *prefix, int32_t n_prefix, const int32_t *suffixes /* concatenated */,
                                      const int32_t *suffix_lens, int32_t n_prompts, int32_t n_samples, int32_t n_batch, int32_t n_predict,
                                      int32_t top_k, double top_p, double temp, const uint32_t *seeds /* [n_prompts * n_samples] */,
                                      int32_t eos_id /* -1: none */, int32_t *out_ids, int32_t *out_lens, double *seconds_out /* may be NULL */);
/* Of the last of the two calls above that generated tokens on this context (a failed call, or one whose n_predict clamps to 0, changes nothing): {n_shared, prompt columns evaluated (n_shared + the sum over the prompts of
 * n_prefix - n_shared + suffix_lens[s]), path, columns}.  path names the route of the decode steps: 1 where they are column-per-XCD launches and shared
 * rows reach the columns' slots by a copy (also with n_shared == 0, when there was nothing to copy), 0 where they run on the launch chain and read shared rows in place.  Returns 0, or -1 for a null argument. */
int biogpt_hip_prefix_stats(const biogpt_hip_ctx *ctx, int32_t out[4]);

/* ---- whole-vocabulary sampling: any top_k up to n_vocab, top_p and min_p, drawn on the device inside the captured step (csrc/kernels_wide_sample.hip.h;
 * INTEGRATION.md, "Sampled generation") ----
 * A sampler is (top_k, top_p, min_p, temp).  top_k 0: the whole vocabulary (k = n_vocab), else k = top_k in [1, n_vocab]; temp finite and > 0; top_p
 * finite (>= 1: no cut); min_p finite and in [0, 1) (0: off).  A row's result is biogpt_sample_top_k_top_p's (biogpt.cpp:908-980) with that k, as
 * biogpt_hip_generate_sample states it, with one stage added between the top-p cut and the draw: of the n candidates left, the longest prefix with
 * probs[i] >= min_p * probs[0] stays (candidate 0 always; the draw normalises).  top_k = 0, top_p = 1, temp = 1 draws from the model's own distribution.
 * A row whose best value is -inf, or that holds NaNs only, gives id 0 and takes no generator output; rows hold no +inf.  The device sums integers
 * (weights rounded to 2^-62 of the best candidate's), in any order: the same row, sampler and generator state give the same id whatever else is in
 * the call, and the ids are the reference's wherever no decision -- a compared cumulative sum against top_p, u against a partial sum of the draw,
 * probs[i] / probs[0] against min_p -- lies within 1e-9 of its border (the sums differ from the reference's sequential ones by < 5e-12).
 * With top_k in [1, 64] and min_p = 0 the generate calls below ARE biogpt_hip_generate_sample / _prefix with the sampler's values, bit for bit; otherwise
 * the step's selection is sample_wide_rows_kernel, one launch as before, captured once for any sampler (the values live in device memory).  Everything else --
 * sequences, seeds, n_batch, EOS, outputs, limits, return values -- is as for biogpt_hip_generate_sample / biogpt_hip_generate_sample_prefix.  There is
 * no form with log-probabilities, generation rules, a trie or a queue.  Argument errors return -1 before any HIP call. */
typedef struct biogpt_hip_sampler {
    int32_t top_k, pad;
    double top_p, min_p, temp;
} biogpt_hip_sampler;
int biogpt_hip_generate_sample_wide(biogpt_hip_ctx *ctx, const int32_t *prompts, const int32_t *prompt_lens, int32_t n_prompts, int32_t n_samples,
                                    int32_t n_batch, int32_t n_predict, const biogpt_hip_sampler *sampler, const uint32_t *seeds, int32_t eos_id,
                                    int32_t *out_ids, int32_t *out_lens, double *seconds_out /* may be NULL */);
int biogpt_hip_generate_sample_wide_prefix(biogpt_hip_ctx *ctx, const int32_t *prefix, int32_t n_prefix, const int32_t *suffixes /* concatenated */,
                                           const int32_t *suffix_lens, int32_t n_prompts, int32_t n_samples, int32_t n_batch, int32_t n_predict,
                                           const biogpt_hip_sampler *sampler, const uint32_t *seeds, int32_t eos_id, int32_t *out_ids, int32_t *out_lens,
                                           double *seconds_out /* may be NULL */);
/* sample_wide_rows_kernel -- always, also for k <= 64 -- over n_rows <= 4096 logits rows of n_vocab floats held in host memory: row r is drawn from with
 * the state mt_states[r * 625 ..] (advanced in place); n_cand_out[r] (may be NULL): the candidates left after all cuts, 0 for a row without a finite
 * value.  For tests of the kernel itself. */
int biogpt_hip_sample_wide_rows_device(int device, const float *logits, int32_t n_rows, int32_t n_vocab, const biogpt_hip_sampler *sampler,
                                       uint32_t *mt_states, int32_t *ids_out, int32_t *n_cand_out);
/* One kernel alone on such rows, for measurement: which 0 sample_wide_rows_kernel, 1 sample_rows_kernel (then top_k in [1, 64], min_p 0).  After one
 * launch that is not timed, reps in [1, 10000] launches from the same generator states; seconds_out[i]: the time between two events around launch i. */
int biogpt_hip_sample_wide_rows_bench(int device, const float *logits, int32_t n_rows, int32_t n_vocab, const biogpt_hip_sampler *sampler,
                                      const uint32_t *mt_states, int32_t which, int32_t reps, double *seconds_out);

/* ---- log-probabilities of generated tokens: the model's confidence in what it generated, without a second pass (transformers' output_scores /
 * compute_transition_scores, the logprobs = k of OpenAI-style interfaces) ----
 * For sequence r and its generated token t < out_lens[r] (greedy: every t < the clamped n_predict), with l the f32 logits row the token was chosen
 * from -- the raw row: temperature 1, neither top_k nor top_p applied -- m = max l and S = sum_v exp(l[v] - m):
 *   lp[r][t] = (l[id] - m) - log(S), the arithmetic of biogpt_hip_score (f32 lane sums combined in double, rounded once): the model's log-probability
 *   of the emitted token, bit for bit what biogpt_hip_score_batch returns for the concatenation prompt_r ++ ids_r with n_batch = 1 -- NOT the
 *   probability under the truncated sampling distribution;
 *   top_ids[r][t][0 .. n_top) / top_lp[r][t][0 .. n_top): the row's first n_top entries, value descending and equal values lower id first, with their
 *   log-probabilities by the same formula.  top_ids[r][t][0] is the row's arg-max: in greedy generation the emitted id.
 * lp is [n][w] and top_ids / top_lp are [n][w][n_top], n the call's sequences and w the n_predict the call returns (as out_ids is [n][w]).  Entries at
 * or past a sequence's length are 0 (lp, top_lp) and -1 (top_ids); an EOS that ended a sampled sequence counts as generated and has its entry.
 * n_top in [0, 8]; with 0 top_ids and top_lp are not touched and may be NULL.  The selection kernel of the captured step writes the numbers
 * (csrc/kernels_genlp.hip.h), n_top travels in device memory: one set of captured steps serves every n_top. */
typedef struct biogpt_hip_gen_logprobs {
    int32_t  n_top;
    float   *lp;
    int32_t *top_ids;
    float   *top_lp;
} biogpt_hip_gen_logprobs;
/* biogpt_hip_generate_greedy_batch / biogpt_hip_generate_sample with log-probabilities.  The arguments are those of the _prefix forms: prefix == NULL
 * with n_prefix == 0 is the plain call on the prompts `suffixes` (none empty then), otherwise the call behind the shared prefix, on either of its
 * paths.  The ids, the lengths, the generator's stream and the return value are those of the call without log-probabilities, bit for bit.  Argument
 * errors return -1 before any HIP call, the message naming the field: logprobs NULL, logprobs.lp NULL, logprobs.n_top outside [0, 8], n_top > 0 with
 * logprobs.top_ids or logprobs.top_lp NULL, n_top > n_vocab, n_prefix != 0 without a prefix, and those of the calls without log-probabilities.  There
 * is no form with generation rules or a trie, and none for beam search, contrastive search, prompt-lookup decoding or biogpt_hip_generate_greedy. */
int biogpt_hip_generate_greedy_batch_lp(biogpt_hip_ctx *ctx, const int32_t *prefix /* or NULL */, int32_t n_prefix, const int32_t *suffixes /* concatenated */,
                                        const int32_t *suffix_lens, int32_t n_seqs, int32_t n_batch, int32_t n_predict, int32_t *out_ids,
                                        double *seconds_out /* may be NULL */, const biogpt_hip_gen_logprobs *logprobs);
int biogpt_hip_generate_sample_lp(biogpt_hip_ctx *ctx, const int32_t *prefix /* or NULL */, int32_t n_prefix, const int32_t *suffixes /* concatenated */,
                                  const int32_t *suffix_lens, int32_t n_prompts, int32_t n_samples, int32_t n_batch, int32_t n_predict,
                                  int32_t top_k, double top_p, double temp, const uint32_t *seeds /* [n_prompts * n_samples] */,
                                  int32_t eos_id /* -1: none */, int32_t *out_ids, int32_t *out_lens, double *seconds_out /* may be NULL */,
                                  const biogpt_hip_gen_logprobs *logprobs);
/* Test hook: the two selection kernels alone over rows held in host memory ([n_rows][n_vocab] f32, any width and alignment), one entry per row.  mode 0:
 * genlp_greedy_rows_kernel; mode 1: sample_lp_rows_kernel, drawing as biogpt_hip_sample_rows_device does (top_k, top_p, temp; mt_states: 625 words per
 * row, advanced in place) -- mode 0 ignores those four.  ids_out [n_rows]: the chosen ids; lp_out [n_rows]; top_ids_out / top_lp_out [n_rows][n_top]
 * (NULL with n_top 0).  Argument errors (those of logprobs above with n_vocab the argument, mode, NULL pointers, n_rows outside [1, 4096], and in mode 1
 * those of biogpt_hip_sample_rows_device) return -1 before any HIP call.  Returns 0, < 0 on error. */
int biogpt_hip_genlp_rows_device(int device, int32_t mode /* 0 greedy, 1 sampled */, const float *rows, int32_t n_rows, int32_t n_vocab, int32_t n_top,
                                 int32_t top_k, double top_p, double temp, uint32_t *mt_states, int32_t *ids_out, float *lp_out, int32_t *top_ids_out,
                                 float *top_lp_out);

/* ---- generation over a queue behind a shared prefix, with log-probabilities ----
 * biogpt_hip_generate_queue of the requests prefix ++ suffix r (suffixes concatenated, suffix_lens their lengths; behind a prefix a suffix may be empty):
 * the first n_shared prefix rows -- the largest multiple of n_batch <= n_prefix - 1 -- are evaluated ONCE, inside the timed span, into the slot behind
 * the columns', and the refill passes and the steps read them in place; a refill evaluates prefix[n_shared:] ++ suffix of the admitted requests alone.
 * Request r's clamp is n_r = min(n_predicts[r], n_positions - n_prefix - suffix_lens[r]).  Its ids and length -- and with logprobs its lp / top_ids / top_lp
 * rows -- are those of biogpt_hip_generate_sample_prefix / biogpt_hip_generate_sample_lp of the request alone (the same prefix, n_samples 1, n_r, the same
 * sampler, seeds[r], eos_id, n_batch), bit for bit, whatever else is in the queue and whatever max_columns and group are: the ids are those of
 * biogpt_hip_generate_queue on the concatenations, as are out_admit_step, out_column and stats but for stats.prompt_columns, the prompt columns evaluated:
 * n_shared + the sum over admitted requests of (n_prefix - n_shared + suffix_lens[r]).  n_shared == 0 (n_prefix <= n_batch): nothing is shared, no slot
 * is reserved and every launch is that of biogpt_hip_generate_queue on the concatenations.  prefix == NULL requires n_prefix == 0; with logprobs == NULL as
 * well the call IS biogpt_hip_generate_queue, with logprobs the plain queue with log-probabilities.  logprobs (or NULL): the struct above with
 * lp [n_requests][n_predict] and top_ids / top_lp [n_requests][n_predict][n_top] (n_predict the row stride as GIVEN); entries at or past a request's length,
 * and every entry of a request that never takes a column, read 0 / -1 / 0.  max_columns in [1, 511] behind a prefix (one K / V slot holds the shared rows);
 * n_prefix >= 1, n_prefix + suffix_lens[r] <= n_positions; everything else as biogpt_hip_generate_queue.  Afterwards biogpt_hip_prefix_stats reads
 * {n_shared, stats.prompt_columns, 0, columns}.  No rules (they are biogpt_hip_generate_queue_requests'), trie, wide sampler or several samples per request.  Returns 0, or < 0 on error (argument errors, -1,
 * come before any HIP call: first those of logprobs, then what needs no model, with no context and no device). */
int biogpt_hip_generate_queue_prefix(biogpt_hip_ctx *ctx, const int32_t *prefix /* or NULL */, int32_t n_prefix, const int32_t *suffixes /* concatenated */,
                                     const int32_t *suffix_lens, int32_t n_requests, const int32_t *n_predicts /* or NULL */, int32_t n_predict,
                                     int32_t max_columns, int32_t group, int32_t n_batch, int32_t top_k, double top_p, double temp, const uint32_t *seeds,
                                     int32_t eos_id, int32_t *out_ids, int32_t *out_lens, int32_t *out_admit_step /* may be NULL */,
                                     int32_t *out_column /* may be NULL */, double *seconds_out, biogpt_hip_queue_stats *stats /* may be NULL */,
                                     const biogpt_hip_gen_logprobs *logprobs /* or NULL */);
/* Test hook: one launch of the queue's step kernel alone -- queue_rows_lp_kernel, or with with_lp == 0 queue_rows_kernel -- over rows held in host memory
 * ([n_rows][n_vocab] f32; row r is column r, n_rows <= 512).  In and out: states [n_rows][8] (n_past, token, n_gen, seq_id, t_vis, 3 more words),
 * finished [n_rows], mt_states [n_rows][625], hdr [1 + 2 * n_rows] (n_live, fin[], len[]); limits [n_rows] is read.  ids_out [n_rows][stride],
 * lp_out [n_rows][stride], top_ids_out / top_lp_out [n_rows][stride][n_top] (NULL with n_top 0) are preset to 0xff bytes: what the launch does not write
 * stays so.  Argument errors return -1 before any HIP call.  Returns 0, < 0 on error. */
int biogpt_hip_queue_rows_device(int device, int32_t with_lp, const float *rows, int32_t n_rows, int32_t n_vocab, int32_t n_top, int32_t stride, int32_t top_k,
                                 double top_p, double temp, int32_t eos_id, uint32_t *mt_states, int32_t *states, const int32_t *limits, int32_t *finished,
                                 int32_t *hdr, int32_t *ids_out, float *lp_out, int32_t *top_ids_out, float *top_lp_out);

/* ---- generation over a queue whose requests carry their own parameters ----
 * biogpt_hip_generate_queue_prefix with one biogpt_hip_request_params per request instead of one top_k / top_p / temp / eos_id for the call: every request has its
 * own sampler, its own EOS id, its own generation rules and up to 4 stop sequences of up to 8 ids.  Request r's ids and length are those of
 *   biogpt_hip_generate_sample_rules(its prompt alone -- behind a prefix: prefix ++ suffix r --, n_samples 1, n_r, params[r]'s top_k / top_p / temp / eos_id / rules,
 *                                    seeds[r])
 * truncated just behind the first position at which one of its stop sequences is complete, bit for bit, whatever else is in the queue and whatever max_columns and
 * group are.  A stop sequence counts only where it lies entirely inside the generated tokens (a match never reaches back into the prompt); the check runs on the
 * token just appended, behind the EOS check, so the rules and the sampler see what they see in the closed call.  An EOS ends a request as before and is included.
 * out_finish[r] (may be NULL): 0 the request reached its limit; 1 it drew its EOS id; 2 + i stop sequence i completed (two at the same token: the lower index; a
 * stop sequence that completes on the limit's token is reported, not the limit); -1 it never took a column.  A call whose requests all carry the same sampler,
 * no rules and no stop sequence returns what biogpt_hip_generate_queue_prefix returns, item for item (ids, lens, admit_step, column, stats).
 * What composes: a prefix with everything; logprobs with samplers and stop sequences (the rows are those of biogpt_hip_generate_sample_lp of the request alone up
 * to the truncation, 0 / -1 / 0 behind it), but logprobs with a request that has a rule switched on is an argument error, as the closed calls have no such form.
 * No trie, wide sampler or several samples per request.  A step is the forward pass and ONE selection launch (queue_req_rows_kernel: rules, draw, stop check and
 * report; csrc/kernels_queue.hip.h).
 * Argument errors (-1, before any HIP call, in the order of biogpt_hip_generate_queue_prefix; those of a request name params[r] and the field): top_k outside
 * [1, 64] or above n_vocab, temp not finite or <= 0, top_p not finite, eos_id outside [-1, n_vocab), the rules as biogpt_hip_generate_sample_rules checks them,
 * rules.n_suppress > 64, n_stop outside [0, 4], a stop length outside [1, 8], a stop id outside [0, n_vocab).  Needs the BioGPT-base fast chain; a wide file is
 * refused (the rules were never checked at other vocabularies).  Returns 0, or < 0 on error. */
typedef struct biogpt_hip_request_params {
    int32_t top_k, eos_id;            /* top_k in [1, 64]; eos_id -1: none */
    double  top_p, temp;
    biogpt_hip_gen_rules rules;       /* as for biogpt_hip_generate_sample_rules; n_suppress <= 64 here */
    int32_t n_stop;                   /* 0 .. 4 stop sequences */
    const int32_t *stop;              /* concatenated ids */
    const int32_t *stop_lens;         /* each in [1, 8] */
} biogpt_hip_request_params;

int biogpt_hip_generate_queue_requests(biogpt_hip_ctx *ctx, const int32_t *prefix /* or NULL */, int32_t n_prefix, const int32_t *prompts /* concatenated; suffixes behind a prefix */,
                                       const int32_t *prompt_lens, int32_t n_requests, const int32_t *n_predicts /* or NULL */, int32_t n_predict, int32_t max_columns,
                                       int32_t group, int32_t n_batch, const biogpt_hip_request_params *params /* [n_requests] */, const uint32_t *seeds,
                                       int32_t *out_ids, int32_t *out_lens, int32_t *out_finish /* may be NULL */, int32_t *out_admit_step /* may be NULL */,
                                       int32_t *out_column /* may be NULL */, double *seconds_out, biogpt_hip_queue_stats *stats /* may be NULL */,
                                       const biogpt_hip_gen_logprobs *logprobs /* or NULL */);
/* Test hook: one launch of queue_req_rows_kernel alone (with_lp != 0: with log-probabilities) over rows held in host memory, as biogpt_hip_queue_rows_device: row r is
 * column r with the record of params[r].  Row r's history is hist_lens[r] tokens of hist (the histories concatenated): the first prompt_lens[r] its prompt, the
 * rest its generated tokens, states[r]'s n_gen of them.  hdr is [1 + 3 * n_rows]: n_live, fin[], len[], reason[].  ids_out [n_rows][stride] is preset to 0xff
 * bytes, then the first n_gen entries of row r to its generated tokens; lp_out / top_ids_out / top_lp_out are preset to 0xff bytes: what the launch does not
 * write stays so.  Argument errors return -1 before any HIP call.  Returns 0, < 0 on error. */
int biogpt_hip_queue_req_rows_device(int device, int32_t with_lp, const float *rows, int32_t n_rows, int32_t n_vocab, int32_t n_top, int32_t stride,
                                     const biogpt_hip_request_params *params /* [n_rows] */, const int32_t *hist /* concatenated */, const int32_t *hist_lens,
                                     const int32_t *prompt_lens, uint32_t *mt_states, int32_t *states, const int32_t *limits, int32_t *finished, int32_t *hdr,
                                     int32_t *ids_out, float *lp_out, int32_t *top_ids_out, float *top_lp_out);

/* ---- queue sessions: submit, poll, stream and cancel while steps run ----
 * biogpt_hip_generate_queue_requests turned inside out, for a caller whose requests arrive over time: the session's columns, K / V slots and captured steps
 * persist between calls, and the host submits a request, runs some groups of steps, reads what was produced and cancels a request, in any order.  One host
 * thread drives a session.
 *   Equality   Request r's ids, length, finish reason and log-probability rows are those of biogpt_hip_generate_queue_requests of r alone (so of
 *              biogpt_hip_generate_sample* of r alone with its sampler and rules, cut behind its first complete stop sequence), bit for bit, whenever it was
 *              submitted, whatever else is or was in the session and whatever max_columns and group are.
 *   Schedule   Deterministic in steps, given the script of calls.  The session has max_columns columns from open on.  biogpt_hip_queue_poll(max_groups) runs
 *              at most max_groups iterations of the closed call's loop: free columns are refilled in ascending order with the pending requests in submission
 *              order; one group of min(group, the most steps any running request may still take) steps runs; the host takes one look at the header and
 *              collects the finished columns.  Requests submitted between two polls are pending from the next poll's first refill on.  A poll with nothing
 *              running and nothing pending launches nothing.  Where all R >= max_columns requests are submitted before the first poll, the results, admit
 *              steps, columns and stats are those of biogpt_hip_generate_queue_requests with the same arguments.  biogpt_hip_queue_plan_script is the
 *              same scheduler on a script with given lengths, without a device.
 *   Events     A poll returns the events of its groups, in order, in memory the session owns until its next poll or its close.  kind 1 (finished): first 0,
 *              count the request's length, ids (and with log-probabilities lp [count], top_ids / top_lp [count][n_top]) all it generated, finish 0 limit /
 *              1 EOS / 2 + i stop sequence i.  A request that may not generate a token (n_predict 0, or no position left) is finished with count 0 at the
 *              next poll and never takes a column; its finish, admit_step and column read -1.  kind 2 (cancelled): the same with what the request had.
 *              kind 0 (delta), only with opts.stream: the tokens [first, first + count) a running request appended during one group; a request's deltas
 *              are contiguous, together they are its final ids and rows, and none follows its finished event.
 *   Cancel     A pending request is dropped at the next poll's start and never takes a column (cancelled, count 0).  A running request stops in front of
 *              that poll's first group: its event carries the tokens it had, a prefix of what it would have produced, and its column is refilled at that
 *              poll's first refill.  No other request's bits change.  An unknown id, or one that has finished or was cancelled, is an error (-1).
 *   Exclusive  While a session is open every other evaluating call on its context fails with -1 before any launch, its message naming the open session.
 *              biogpt_hip_queue_close with requests still running is legal and drops them; afterwards the context serves everything as before.
 * opts: max_columns in [1, 512] (511 behind a prefix), group in [1, 64], n_batch >= 1, n_predict >= 0 the most any request may ask for, max_len (0:
 * n_positions) the most keys any request may reach -- the steps are captured at open for every context bucket up to it, none inside a poll --, prefix /
 * n_prefix (or NULL / 0) the shared prefix, logprobs -1 (none) or n_top in [0, 8], stream 0 / 1, and top_k / eos_id / top_p / temp the sampler of a request
 * submitted without params.  biogpt_hip_queue_submit copies the prompt (the suffix behind a prefix, which may then be empty) and the parameters and returns the
 * request's id, 0, 1, 2, ... in submission order; n_predict in [0, opts.n_predict], params (or NULL) as for biogpt_hip_generate_queue_requests, a rule under
 * logprobs refused as there.  Argument errors return NULL / -1 before any HIP call, the message naming the field; those of opts that need no model come first,
 * with no context and no device.  Needs the BioGPT-base fast chain (block-quantized weights).  A poll that fails (-2) leaves only the close. */
typedef struct biogpt_hip_queue_session biogpt_hip_queue_session;
typedef struct biogpt_hip_queue_opts {
    int32_t max_columns, group, n_batch, n_predict;
    int32_t max_len;                  /* 0: n_positions */
    int32_t n_prefix;
    const int32_t *prefix;            /* or NULL */
    int32_t logprobs;                 /* -1: none; otherwise n_top */
    int32_t stream;
    int32_t top_k, eos_id;            /* the default sampler */
    double  top_p, temp;
} biogpt_hip_queue_opts;
typedef struct biogpt_hip_queue_event {
    int32_t id, kind;                 /* kind 0 delta, 1 finished, 2 cancelled */
    int32_t first, count;
    int32_t finish, admit_step, column, n_top;
    const int32_t *ids;               /* [count] */
    const float   *lp;                /* [count], or NULL without log-probabilities */
    const int32_t *top_ids;           /* [count][n_top] */
    const float   *top_lp;            /* [count][n_top] */
} biogpt_hip_queue_event;

biogpt_hip_queue_session *biogpt_hip_queue_open(biogpt_hip_ctx *ctx, const biogpt_hip_queue_opts *opts);
int biogpt_hip_queue_submit(biogpt_hip_queue_session *session, const int32_t *prompt, int32_t len, int32_t n_predict, uint32_t seed,
                            const biogpt_hip_request_params *params /* or NULL: the session's sampler */);
int biogpt_hip_queue_cancel(biogpt_hip_queue_session *session, int32_t id);
/* returns the number of events, *events_out the first; < 0 on error */
int biogpt_hip_queue_poll(biogpt_hip_queue_session *session, int32_t max_groups, const biogpt_hip_queue_event **events_out);
/* stats as biogpt_hip_generate_queue counts them, accumulated over the polls; seconds_out (may be NULL): the host time spent inside polls (and on the shared
 * rows at open); counts_out (may be NULL) [3]: requests submitted, pending, running */
int biogpt_hip_queue_session_stats(const biogpt_hip_queue_session *session, biogpt_hip_queue_stats *stats, double *seconds_out, int32_t *counts_out);
int biogpt_hip_queue_close(biogpt_hip_queue_session *session);
/* The session's scheduler alone, on the host, on a script: ops is [n_ops][2] = {kind, argument} with kind 0 SUBMIT (the i-th SUBMIT is request i: it
 * generates gen_lens[i] tokens under the limit limits[i], as for biogpt_hip_queue_plan_limits), 1 POLL n, 2 CANCEL r (what a session refuses changes nothing).
 * admit_step / column [requests]: as biogpt_hip_queue_plan, -1 where a request never took a column; finish_group [requests]: the groups run when the
 * request's finished or cancelled event was produced, -1 where the script ends before; lens (may be NULL) [requests]: the tokens it had then.  Returns 0 or -1. */
int biogpt_hip_queue_plan_script(const int32_t *ops, int32_t n_ops, const int32_t *gen_lens, const int32_t *limits, int32_t max_columns, int32_t group,
                                 int32_t *admit_step, int32_t *column, int32_t *finish_group, int32_t *lens /* may be NULL */,
                                 biogpt_hip_queue_stats *stats /* may be NULL */);
/* Test hooks: the two kernels of a session alone (csrc/kernels_queue.hip.h).  queue_stream_kernel over constructed columns: column c has n_gen[c] generated
 * tokens (any value: clamped to gen_stride), its token row is row c of gen_rows [C][gen_stride], with n_top >= 0 its log-probability rows are lp [C][lp_stride]
 * and top_ids / top_lp [C][lp_stride][n_top].  block_out [block_bytes], preset to 0xff bytes, is what lies behind a streaming session's header: n_gen [C],
 * ids [C][g], then lp [C][g], top_ids [C][g][n_top], top_lp [C][g][n_top], every part at a multiple of 16 bytes.  Returns the bytes of that layout, < 0 on error.
 * queue_cancel_kernel on the list cols [n] over 512 constructed columns: finished [512] and hdr [1 + 2 * 512] (n_live, fin[], len[]) in and out, n_gen [512]
 * read.  Returns 0, < 0 on error. */
int64_t biogpt_hip_queue_stream_device(int device, const int32_t *n_gen, const int32_t *gen_rows, int32_t C, int32_t gen_stride, int32_t g, int32_t n_top,
                                       int32_t lp_stride, const float *lp, const int32_t *top_ids, const float *top_lp, uint8_t *block_out, int64_t block_bytes);
int biogpt_hip_queue_cancel_device(int device, const int32_t *cols, int32_t n, int32_t *finished, const int32_t *n_gen, int32_t *hdr);

/* ---- hidden states, pooled embeddings, classification heads (no counterpart in the reference) ----
 * The activations in front of the lm_head, from the causal passes of biogpt_hip_score without the lm_head and the log-softmax.
 *
 * biogpt_hip_hidden: the final hidden state (after the last LayerNorm; transformers' last_hidden_state) of every token, f32
 * [n_tokens][d_model].  Causal whatever BIOGPT_HIP_CAUSAL says: row i sees the keys [0, n_past + i].  Serves every model
 * biogpt_hip_score serves (all seven file types, any shape).  Arguments as for biogpt_hip_eval.  Afterwards the K / V rows
 * [n_past, n_past + n_tokens) and the context's position are those biogpt_hip_eval_prompt(tokens, n_past, 1) leaves: a following
 * biogpt_hip_eval at n_past + n_tokens continues the sequence.  The context's logits row (biogpt_hip_read_logits /
 * biogpt_hip_logits_device) is UNDEFINED after the call: no logits are computed.  Returns 0 or < 0. */
/* final hidden state (after the last LayerNorm) of every token: [n_tokens][d_model]; causal: row i sees keys [0, n_past + i] */
int biogpt_hip_hidden(biogpt_hip_ctx *ctx, const int32_t *tokens, int32_t n_tokens, int32_t n_past, float *hidden_out);

typedef struct biogpt_hip_embed_opts {
    int32_t layer;      /* transformers' hidden_states index: 0 = embeddings ... k = input of layer k ... n_layer = after the final LayerNorm; -1 = n_layer */
    int32_t pooling;    /* 0 none (one row per token, flat order of seqs), 1 last token, 2 mean over the sequence's tokens */
    int32_t normalize;  /* 1: L2-normalise each output row; only without a head */
    int32_t n_out;      /* head: 0 = none, else rows of w, in [1, 256] */
    const float *w;     /* [n_out][d_model] f32, host memory */
    const float *b;     /* [n_out] or NULL */
} biogpt_hip_embed_opts;

/* Embeddings of n_seqs independent sequences (seqs / lens: the layout of biogpt_hip_score_batch), each from position 0 in a K / V
 * cache of its own; the context's own cache, position and logits row are left alone.  Without pooling and with layer = n_layer every
 * sequence's rows are bit-identical to biogpt_hip_hidden(seq, 0).  layer = k < n_layer stops after k layers (no final LayerNorm:
 * the residual stream, transformers' hidden_states[k]) and costs k / n_layer of the passes.  Pooling runs on the device: the row of the
 * last token, or the mean over the sequence's rows (double sums, rounded once); normalize divides each output row by its L2 norm
 * (a zero row stays zero).  A head is applied on the device to the pooled rows (sequence classification, BioGptForSequenceClassification.score)
 * or, without pooling, to every token's row (token classification): out[r][o] = (float)(b[o] + sum_d (double)w[o][d] * (double)x[r][d]).
 * Needs the BioGPT-base fast chain (block-quantized weights) and n_seqs in [1, 512], like biogpt_hip_score_batch; other files fail with
 * -1 (biogpt_hip_hidden serves them).  Argument errors (null pointers, an empty sequence, bad token ids, layer outside [-1, n_layer],
 * unknown pooling, normalize with a head, n_out outside [0, 256], n_out > 0 without w, w or b with n_out = 0, a non-finite value in
 * w or b) return -1 before any HIP call and name the field; a failed allocation returns -2 and names the size.  seconds_out (may be
 * NULL): the passes, pooling, head and the copy back.  Returns 0 or < 0. */
/* out: [rows][width]; rows = n_seqs with pooling, sum(lens) without; width = n_out with a head, else d_model */
int biogpt_hip_embed_batch(biogpt_hip_ctx *ctx, const int32_t *seqs, const int32_t *lens, int32_t n_seqs,
                           const biogpt_hip_embed_opts *opts /* NULL: {-1, 1, 0, 0, NULL, NULL} */, float *out, double *seconds_out);

/* ---- introspection for tests / profiling ---------------------------------------------------
 * Copy `count` floats of the F32 KV cache (which: 0 = K, 1 = V) starting at element `offset` of
 * the flat [n_layer][n_positions][d_model] array (biogpt.cpp:331-335) to host memory. */
int biogpt_hip_read_kv(biogpt_hip_ctx *ctx, int which, size_t offset, size_t count, float *out);
/* Tests of slot reuse: what the last column call (batched generation, beam search, a queue) left in column `column`'s own K / V cache slot and beam pool row.
 * kv_out (may be NULL): the K (which 0) or V (1) row of position pos in every layer, [n_layer][d_model]; pool_out (may be NULL): the first n_ids words of the
 * column's pool row.  Nothing is cleared between calls, so rows no call has written hold what the allocation held.  Returns 0, -1 (arguments) or -2. */
int biogpt_hip_read_column_state(biogpt_hip_ctx *ctx, int32_t column, int32_t which, int32_t pos, float *kv_out, int32_t n_ids, int32_t *pool_out);

/* Profiling builds only (-DBIOGPT_HIP_PROFILE_HOOKS, BIOGPT_HIP_DBG=128; no reference counterpart): the raw wall-clock stamps (100 MHz ticks) the
 * pipelined decode launches left in the context's stamp buffer, `count` words from word `offset` (tools/tail_timeline.py). */
int biogpt_hip_debug_stamps(biogpt_hip_ctx *ctx, size_t offset, size_t count, unsigned long long *out);

/* Stand-alone launch of the block-quantized mat-vec kernel on a weight matrix of the loaded
 * model, for kernel-level roofline timing: which = 0 fc1 of layer `layer`, 1 fc2,
 * 2 q/k/v fused, 3 out_proj, 4 lm_head (5-11: internal, see bench.py), 12 lm_head with the weights taken from a
 * different one of 14 device copies every launch (344 MB: not resident in the Infinity Cache), 13 (float files) all layers of one token at 104 keys as the
 * ONE persistent launch of kernels_fpipe.hip.h.  Runs `reps` back-to-back launches on the context's
 * stream bracketed by HIP events and returns the average seconds per launch in *seconds_out and
 * the algorithmic bytes of one launch in *bytes_out. */
int biogpt_hip_bench_matvec(biogpt_hip_ctx *ctx, int which, int layer, int reps,
                            double *seconds_out, double *bytes_out);

/* The decode mat-vec kernel (LayerNorm + Q4_0 W*A8 mat-vec, d_model = 1024 columns) on a synthetic weight
 * stream of `rows` rows -- far larger than the caches when rows >= 2^19 (302 MB): measures what the kernel
 * body sustains per byte when launch latency is amortised (SURVEY 8d roofline check).  `steps` = row steps per
 * wave.  HIP-event timed; *bytes_out = algorithmic bytes of one launch. */
int biogpt_hip_bench_stream(biogpt_hip_ctx *ctx, int32_t rows, int reps, int steps, double *seconds_out, double *bytes_out);

/* Timed replay of the captured single-token decode graph at a fixed n_past (no token feedback
 * side effects beyond the KV row at n_past): average seconds per token over `reps` replays,
 * HIP-event timed on the context's stream. */
int biogpt_hip_bench_decode(biogpt_hip_ctx *ctx, int32_t n_past, int reps, double *seconds_out);

/* The reference's greedy host loop (main.cpp:91-151: one eval call per token, sampler on the host) run in C++ on this
 * library and timed as a whole: mode 0 = biogpt_hip_eval + host arg-max (the logits row crosses PCIe every token),
 * mode 1 = biogpt_hip_eval_topk with k = 40.  out_ids (may be NULL) receives the n_predict ids.  Measurement aid. */
int biogpt_hip_bench_api_loop(biogpt_hip_ctx *ctx, const int32_t *prompt, int32_t n_prompt, int32_t n_predict, int32_t mode,
                              int32_t *out_ids, double *seconds_out);

/* ---- text <-> ids (host-only, no GPU needed) -------------------------------------
 * The reference's tokenizer stack -- moses_tokenize (mosestokenizer.cpp:290-358), bpe (bpe.cpp:20-91),
 * gpt_tokenize / gpt_decode (biogpt.cpp:850-906), moses_detokenize (mosestokenizer.cpp:360-466) --
 * re-implemented without std::regex, byte-for-byte equal in output including its quirks.
 *
 * Vocabulary handles: biogpt_hip_vocab_load() parses only the header, vocab and merges of a model file;
 * biogpt_hip_ctx_vocab() borrows the one a loaded context already holds (NULL for an attached context).
 * String results: the function returns the byte length of the result (without the terminating NUL) and
 * writes it only when cap >= length + 1 -- call again with a larger buffer otherwise.  Lists of words
 * travel as one '\n'-joined string.  Negative = error; BIOGPT_HIP_E_LENGTH where the reference throws
 * std::length_error (a period-final word that is neither an abbreviation nor a listed prefix, followed by
 * a word starting with a byte >= 0x80; mosestokenizer.cpp:264).
 *
 * Data files: nonbreaking_prefixes/nonbreaking_prefix.<lang> are read from the data directory
 * ($BIOGPT_DATA_DIR, else "../data" like mosestokenizer.cpp:11-12; a missing file = empty list, as in
 * the reference).  The five perluniprops byte classes are built in; <dir>/perluniprops/Is*.txt override
 * them when present.  lang: "" (what the reference CLI effectively passes), "en", "fr", ... */
biogpt_hip_vocab       *biogpt_hip_vocab_load(const char *fname);
/* from arrays: tokens[id] / merges[rank] ("left right" records as stored in the file), explicit byte lengths */
biogpt_hip_vocab       *biogpt_hip_vocab_create(const char *const *tokens, const int32_t *token_lens, int32_t n_tokens,
                                                const char *const *merges, const int32_t *merge_lens, int32_t n_merges);
void                    biogpt_hip_vocab_free(biogpt_hip_vocab *v);
const biogpt_hip_vocab *biogpt_hip_ctx_vocab(const biogpt_hip_ctx *ctx);
int biogpt_hip_tokenizer_set_data_dir(const char *dir);

/* gpt_tokenize: ids of `text`, always starting with 2 ("</s>"); pieces missing from the vocabulary are
 * dropped with a warning on stderr.  Returns the id count; writes min(count, cap) ids. */
int biogpt_hip_tokenize(const biogpt_hip_vocab *v, const char *text, const char *lang, int32_t *out_ids, int32_t cap);
/* gpt_decode of the vocabulary strings of `ids` (an id outside the table decodes as empty). */
int biogpt_hip_decode(const biogpt_hip_vocab *v, const int32_t *ids, int32_t n, const char *lang, char *out, int32_t cap);
/* gpt_decode on explicit token strings ('\n'-joined) */
int biogpt_hip_decode_strings(const char *tokens_nl, const char *lang, char *out, int32_t cap);

/* the stages, exposed for parity tests */
int biogpt_hip_moses_tokenize(const char *text, const char *lang, char *out, int32_t cap);        /* words, '\n'-joined */
int biogpt_hip_moses_detokenize(const char *tokens_nl, const char *lang, char *out, int32_t cap);
int biogpt_hip_bpe(const biogpt_hip_vocab *v, const char *word, char *out, int32_t cap);          /* pieces joined by ' ' */
/* membership table (256 x 0/1) of byte class `which`: 0 IsAlnum, 1 IsAlpha, 2 IsLower, 3 IsN, 4 IsSc */
int biogpt_hip_tokenizer_byte_class(int which, uint8_t *out256);

/* ---- host-side tools (no GPU needed) --------------------------------------------------------
 * File -> file quantizer, replaces examples/quantize (quantize.cpp:8-135 + biogpt.cpp:459-621):
 * ftype in {2,3,7,8,9}; every 2-D tensor whose name contains "weight" is quantized in rows of
 * ne[0]; header ftype rewritten; vocab/merges copied verbatim. */
int biogpt_hip_quantize_file(const char *fname_in, const char *fname_out, int32_t ftype);

/* The quantizer's inner loops on the device (biogpt.cpp:565-603 -> ggml_quantize_q4_0 .. q8_0): nrows rows of k
 * f32 values in host memory -> the FILE's block format of ggml type `type` (2 q4_0, 3 q4_1, 6 q5_0, 7 q5_1, 8 q8_0) in host
 * memory, byte-identical to biogpt_hip_quantize_file's host encoder. */
int biogpt_hip_quantize_rows_device(int device, int32_t type, const float *src, int64_t nrows, int64_t k, uint8_t *dst);

/* The LayerNorm + Q8 stage of the single-token decode launches, alone (tests of the stage itself; no model).
 * mode 0: n_rows rows of 1024 f32 values -> ggml_norm + gain / bias (ln_w, ln_b: 1024 values, or n_rows x 1024 with wb_per_row != 0), eps as given, then
 *   quantize_row_q8_0 (q81 = 0) or q8_1 (q81 = 1): q_out n_rows x 1024 codes, d_out n_rows x 32 block scales (q8_0: rounded through f16), s_out n_rows x 32
 *   (q8_1: the bits of the float d * sum; q8_0 with want_sum: the integer block sums; q8_0 without: not written, left 0xffffffff).
 * mode 1: the launches' activation quantizer on n_rows blocks of 32 values (ln_w, ln_b, eps unused): q_out n_rows x 32, d_out and s_out n_rows (q8_0 without
 *   want_sum: s = 0).
 * One workgroup of 512 threads per row (mode 0), thread t holding elements 4t .. 4t+3, as the pipelined launches run the stage. */
int biogpt_hip_ln_q8_device(int device, int32_t mode, const float *x, int32_t n_rows, const float *ln_w, const float *ln_b, int32_t wb_per_row, float eps,
                            int32_t q81, int32_t want_sum, int8_t *q_out, float *d_out, uint32_t *s_out);

/* The short arithmetic forms of that stage against the expressions they stand for, over all 2^32 float bit patterns in one launch.  out[18] = tested[6],
 * mismatches[6], lowest mismatching pattern[6] (~0: none) for the checks: 0 the short 1 / sqrtf(v) inside its guarded range, 1 the guarded function on every
 * pattern, 2 the Q8 rounding for |x| <= 2^22, 3 for every other pattern, 4 the short d = a / 127 and id = 1 / d inside their guarded range, 5 the guarded
 * function on every pattern. */
int biogpt_hip_q8_forms_device(int device, uint64_t *out);

/* Write a synthetic seeded BioGPT model: F32 (ftype 0) or F16 (ftype 1) file in the
 * reference's format, weights ~ N(0, 0.02^2), LayerNorm gains 1 + N(0, 0.02^2), biases N(0, 0.02^2),
 * embed_tokens row 1 zero; n_merges merge records are written (40000 keeps the reference's
 * loader happy, F6). */
int biogpt_hip_write_synthetic(const char *fname, const biogpt_hip_hparams *hp, uint64_t seed);

/* Measurement: the decode mat-vec over EVERY block-quantized matrix of the loaded model (24 x {q/k/v, out_proj, fc1, fc2} + lm_head = the W of SURVEY 8(d)) in one
 * launch, rows spread over the chip, each against a resident Q8 activation vector of its shape; launches alternate between two copies of the weights so that the
 * 256 MB Infinity Cache cannot serve them.  seconds_out per launch, bytes_out = SURVEY 8(d)'s algorithmic bytes per launch, check_out = max |device - host| over
 * sampled rows (0 = bit-identical to the reference's arithmetic; -1 = format not checked).  The figure north_star's ">= 70 % of the HBM roofline on the Q4_0
 * single-token decode mat-vec at d_model = 1024" asks for; replaces nothing of biogpt.cpp (its loop body is biogpt.cpp:705-803). */
int biogpt_hip_bench_sweep(biogpt_hip_ctx *ctx, int which /* 0: every matrix, two copies; 1: lm_head alone; 2: q/k/v + out_proj of every layer (the K = 1024, D x D shapes); 3: fc2 (K = 4096); 4: fc1 -- 1 .. 4 on as many copies in turn as exceed the Infinity Cache */, int reps, double *seconds_out, double *bytes_out, double *check_out);
/* the same, and (each may be NULL) the launch's output rows (matrix after matrix: per layer q/k/v, out_proj, fc1, fc2, then lm_head -- those `which` selects) and the two Q8
 * activation vectors (xq_out: 1024 + 4096 int8, xd_out: 32 + 128 block scales) they were computed with, so that a test can recompute rows with the oracle's vec_dot of
 * biogpt.cpp:705-716,767,803's mat-vecs */
int biogpt_hip_bench_sweep_ex(biogpt_hip_ctx *ctx, int which, int reps, double *seconds_out, double *bytes_out, double *check_out, float *rows_out, size_t rows_cap, int8_t *xq_out, float *xd_out);

/* Single-token evals of a context that does not hold the device's pipeline slot are replayed as a captured five-launch step.  The row of such a replay carries the
 * sequence number its first node fetched (forwarded by the last layer's last kernel and by the lm_head as they start); biogpt_hip_eval / biogpt_hip_eval_inplace /
 * biogpt_hip_read_logits compare it with the call's and, if it is another call's, repeat the call on eager launches.  out2 = {evals replayed that way, rows repeated}.
 * The contract behind it: the row biogpt_eval returns is the row of THIS eval (biogpt.cpp:840-844). */
int biogpt_hip_lineage_stats(biogpt_hip_ctx *ctx, int64_t *out2);

#ifdef __cplusplus
}
#endif
#endif /* BIOGPT_HIP_H */
