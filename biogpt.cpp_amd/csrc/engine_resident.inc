// Part of engine.hip (textually included there: same translation unit, same anonymous namespace / extern "C" block): single-token evals -- the resident launch behind biogpt_hip_eval's loop (mailbox, completion words, one position ahead of a greedy caller) and the graph-replayed / eager step of every other case.

// ---- resident single-token evals -------------------------------------------------------------------------------------------------------
// biogpt_eval() is called once per token (main.cpp:91-151).  As separate launches every call pays the pipelined launch's start-up (arrival
// tickets, first weight load exposed, GELU slice) + a graph launch + the completion poll: ~30 us of a ~300 us token.  With the device to itself
// the launch can simply STAY: after token tk it waits -- bounded by BIOGPT_HIP_RESIDENT_US -- for the next call to drop {n_past, token, seq} into a
// pinned mailbox, and every lm_head workgroup reports the rows it has written to the pinned logits row with a completion word.  A call then costs
// two PCIe hops and no HIP API call.  Anything else the context is asked to do first ends the resident launch (resident_stop).
static bool resident_stop(biogpt_hip_ctx *c) {
    if (!c || !c->res_live) return true;
    c->res_live = false;
    if (c->res_left > 0 && c->res_mbox) {      // it still waits for tokens: ask it to leave (a slot whose position is not the expected one)
        const uint32_t seq = ++c->res_seq;
        __atomic_store_n(reinterpret_cast<unsigned long long *>(c->res_mbox + (size_t)(seq & 63u) * 8), bgk::xp_post(seq, 0x1fff, 0xffffff, 0), __ATOMIC_RELEASE);
    }
    c->res_left = 0;
    c->spec_pending = false;
    HIP_TRY(false, hipSetDevice(c->device));
    HIP_TRY(false, hipStreamSynchronize(c->stream));      // a pass the launch started on its own account finishes first (at most one token's time)
    const bool ok = xpipe_check(c);
    if (c->res_acc & 1u) {      // the last pass the caller asked for wrote the alternate buffers: everything outside the resident launch reads the ordinary ones
        const size_t V = (size_t)c->hp.n_vocab;
        HIP_TRY(false, hipMemcpyAsync(c->logits, c->logits_alt, V * 4, hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(false, hipMemcpyAsync(c->pmax_val, c->pmax_val_alt, (size_t)c->pmax_cap * 4, hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(false, hipMemcpyAsync(c->pmax_idx, c->pmax_idx_alt, (size_t)c->pmax_cap * 4, hipMemcpyDeviceToDevice, c->stream));
        c->res_acc = 0;
    }
    return ok;
}

// Speculation policy: a launch runs ahead of the caller only after spec_need consecutive calls whose token WAS the device's arg-max of the row before (a greedy
// caller: always; a sampling caller: rarely for long), and every miss doubles spec_need (up to 64; 256 hits in a row halve it again) -- a miss costs the pass
// that was started in vain plus a fresh launch.
static bool spec_wanted(const biogpt_hip_ctx *c) { return c->opt.res_spec != 0 && c->spec_streak >= c->spec_need; }

// the pinned row buffers: the logits row + (resident launches) the maxima of its 64-row blocks behind it (kernels_xpipe.hip.h, xp_blockmax_offset)
static size_t host_row_bytes(const biogpt_hip_ctx *ctx) { return ((size_t)bgk::xp_blockmax_offset(ctx->hp.n_vocab) + 1024 + 4) * 4; }
static int host_stamp_index(const biogpt_hip_ctx *ctx) { return bgk::xp_blockmax_offset(ctx->hp.n_vocab) + 1024; }      // dword behind the row and its block maxima: the row's lineage
// one token through a resident launch; 1 = done (row in ctx->row_cur), 0 = not applicable here (caller takes the ordinary path), -2 = failure
static int resident_eval(biogpt_hip_ctx *ctx, int32_t token, int32_t n_past) {
    if (!ctx->opt.resident || ctx->opt.no_graph || !xpipe_lm_folds(ctx)) return 0;
    const int tmax = bucket_tmax(ctx, graph_bucket(n_past + 1));
    if (!fused_decode_ok(ctx, tmax) || !xpipe_bucket_ok(ctx, tmax)) return 0;      // up to 256 keys kernels_xpipe.hip.h, beyond (<= 1024) kernels_xlong.hip.h, each in its resident form
    if (ctx->hp.n_vocab >= 0xffffff || ctx->hp.n_positions >= 0x1fff) return 0;      // the mailbox word's fields (xp_post)
    const size_t V = (size_t)ctx->hp.n_vocab;
    const volatile uint32_t *const err = reinterpret_cast<const volatile uint32_t *>(ctx->xp_err_host);
    for (int attempt = 0; attempt < 4; attempt++) {
        if (ctx->res_live && (*err != 0u || ctx->res_left <= 0 || n_past != ctx->res_next)) {
            if (!resident_stop(ctx)) return -2;      // it has left (idle), is used up, or the caller moved elsewhere in the sequence
        }
        uint32_t seq;
        if (ctx->res_live) {      // hand the token to the launch that is waiting for it -- or that has already started this position with its own arg-max
            seq = ctx->res_seq + 1u;
            // the device's arg-max of the previous row, written when that row was complete (a few microseconds before the caller could have read it)
            bool have = false, gone = false;
            int32_t guess = -1;
            for (uint32_t spin = 0; spin < (ctx->spec_pending ? 0x40000000u : 1u); spin++) {
                const unsigned long long rec = __atomic_load_n(ctx->res_spec, __ATOMIC_ACQUIRE);
                if ((uint32_t)(rec >> 32) == seq) { have = true; guess = (int32_t)(uint32_t)rec; break; }
                if (*err != 0u) { gone = true; break; }
            }
            if (ctx->spec_pending && !have) {      // the launch left before it got here (idle time-out, failure): a fresh launch takes the token
                (void)gone;
                if (!resident_stop(ctx)) return -2;
                if (ctx->xp_state != 1) return 0;
                continue;
            }
            if (have) ctx->spec_streak = (guess == token) ? ctx->spec_streak + 1 : 0;
            if (ctx->spec_pending) {
                if (guess != token) {      // the pass in flight is not the one the caller wants: it ends the launch (the post below would not match), a fresh one follows
                    ctx->spec_misses++;
                    ctx->spec_need = std::min(ctx->spec_need * 2, 64);      // (0.6 ^ 64 ~ 6e-15: a sampling caller does not get there; a greedy one is back after 64 tokens)
                    ctx->spec_run = 0;
                    if (!resident_stop(ctx)) return -2;
                    if (ctx->xp_state != 1) return 0;
                    continue;
                }
                ctx->spec_hits++;
                if (++ctx->spec_run % 256 == 0) ctx->spec_need = std::max(4, ctx->spec_need / 2);      // a long run ahead of the caller earns the trust back
            }
            ctx->res_seq = seq;
            ctx->res_next++; ctx->res_left--;
            const bool spec_next = ctx->res_left > 0 && spec_wanted(ctx);
            __atomic_store_n(reinterpret_cast<unsigned long long *>(ctx->res_mbox + (size_t)(seq & 63u) * 8), bgk::xp_post(seq, n_past, token, spec_next ? 1 : 0), __ATOMIC_RELEASE);
            ctx->spec_pending = spec_next;
        } else {
            if (!xpipe_usable(ctx, tmax)) return 0;      // another context holds the device's pipeline slot
            if (!ctx->res_mbox) {
                HIP_TRY(-2, hipHostMalloc(reinterpret_cast<void **>(&ctx->res_mbox), 64 * 8 * 4, hipHostMallocDefault));
                HIP_TRY(-2, hipHostMalloc(reinterpret_cast<void **>(&ctx->res_done), 256 * 4, hipHostMallocDefault));
                std::memset(ctx->res_mbox, 0xff, 64 * 8 * 4);
                std::memset(ctx->res_done, 0, 256 * 4);
                ctx->res_seq = 0; ctx->res_acc = 0;      // fresh completion words: the sequence numbers start over with them (a zeroed word must never look "ahead" of a late number)
            }
            if (!ctx->res_spec) {
                HIP_TRY(-2, hipHostMalloc(reinterpret_cast<void **>(&ctx->res_spec), 64, hipHostMallocDefault));
                std::memset(ctx->res_spec, 0, 64);
                HIP_TRY(-2, hipHostMalloc(reinterpret_cast<void **>(&ctx->logits_host_alt), host_row_bytes(ctx), hipHostMallocDefault));
                HIP_TRY(-2, hipMalloc(&ctx->logits_alt, V * 4));
                HIP_TRY(-2, hipMalloc(&ctx->pmax_val_alt, (size_t)ctx->pmax_cap * 4));
                HIP_TRY(-2, hipMalloc(&ctx->pmax_idx_alt, (size_t)ctx->pmax_cap * 4));
            }
            if (!ctx->logits_host) HIP_TRY(-2, hipHostMalloc(reinterpret_cast<void **>(&ctx->logits_host), host_row_bytes(ctx), hipHostMallocDefault));
            if ((ctx->opt.res_dbg & 32) && !ctx->tstamp) {
                HIP_TRY(-2, hipMalloc(&ctx->tstamp, (size_t)4 << 20));
                HIP_TRY(-2, hipMemset(ctx->tstamp, 0, (size_t)4 << 20));
            }
            seq = ++ctx->res_seq;
            const int n_tok = tmax - n_past;          // up to the end of the context bucket
            const bool spec_next = n_tok > 1 && spec_wanted(ctx);
            const ResidentArgs ra{token, n_past, seq, spec_next ? 1 : 0};
            bool row_done = false;
            if (!enqueue_decode_fused(ctx, tmax, 1, 0, 0, -1, -1, n_tok, ctx->logits_host, &row_done, 1, &ra)) return -2;
            if (!row_done) BG_FAIL(-2, "internal: the resident launch does not write the host row");
            ctx->res_live = true; ctx->res_next = n_past + 1; ctx->res_left = n_tok - 1;
            ctx->res_nw = (ctx->lm_blocks + 3) / 4;
            ctx->mbox_synced = ctx->mbox_sent;
            ctx->spec_pending = spec_next;
        }
        // completion: one word per lm_head workgroup, written behind its rows (a launch that runs ahead may already have moved a word on to the next number)
        const volatile uint32_t *done = ctx->res_done;
        const int nw = ctx->res_nw;
        // no clock on the fast path (a clock read is a system call on some virtualised hosts: microseconds): the 5 s guard starts counting after ~10^6 polls
        std::chrono::steady_clock::time_point t0{};
        if (ctx->opt.res_dbg & 8) {      // time between the previous call's return and this post = the caller's own time + this function's overhead
            t0 = std::chrono::steady_clock::now();
            if (ctx->res_calls > 0) ctx->res_t_call += std::chrono::duration<double>(t0 - ctx->res_t_last).count();
            ctx->res_calls++;
        }
        bool ok = false, left = false, timing = false;
        std::chrono::steady_clock::time_point tg{};
        int k = 0;                       // completion words seen so far
        for (uint32_t spin = 0;; spin++) {
            while (k < nw && (int32_t)(done[k] - seq) >= 0) k++;
            if (k == nw) { ok = true; break; }
            if (*err != 0u) { left = true; break; }
            if ((spin & 0xfffffu) == 0xfffffu) {
                if (!timing) { tg = std::chrono::steady_clock::now(); timing = true; }
                else if (std::chrono::duration<double>(std::chrono::steady_clock::now() - tg).count() > 5.0) break;
            }
        }
        if (ok) {
            __atomic_thread_fence(__ATOMIC_ACQUIRE);
            ctx->res_acc = seq;
            ctx->row_cur = (seq & 1u) ? ctx->logits_host_alt : ctx->logits_host;
            if (ctx->opt.res_dbg & 8) { ctx->res_t_last = std::chrono::steady_clock::now(); ctx->res_t_wait += std::chrono::duration<double>(ctx->res_t_last - t0).count(); }
            return 1;
        }
        if (!left) { (void)resident_stop(ctx); BG_FAIL(-2, "a resident decode launch did not answer within 5 s"); }
        // the launch left (idle time-out racing with this call) or failed: wait for it, then this token goes into a fresh launch -- or, after a
        // failure, onto the five-launch layer through the ordinary path
        if (!resident_stop(ctx)) return -2;
        if (ctx->xp_state != 1) return 0;
    }
    return 0;
}

// form 0: the step; form 1: the step + a last node that writes the logits row into pinned host memory (biogpt_hip_eval)
static int eval_device_impl(biogpt_hip_ctx *ctx, const int32_t *tokens, int32_t n, int32_t n_past, int form, bool *row_in_host = nullptr) {
    XpCallScope xp_scope(ctx);
    clear_error();
    if (row_in_host) *row_in_host = false;
    ctx->dev_stamp_expect = 0; ctx->stamp_expect = 0;      // (set again below if this call is a replayed five-launch graph)
    if (!check_eval_args(ctx, tokens, n, n_past)) return -1;
    HIP_TRY(-2, hipSetDevice(ctx->device));
    if (!resident_stop(ctx)) return -2;
    // one token at a position of the five-launch decode step: replay its captured graph -- its first node pulls the
    // token and the position from a pinned mailbox slot -- instead of a copy command and 121 launches one by one
    if (n == 1 && !ctx->opt.no_graph && fused_decode_ok(ctx, bucket_tmax(ctx, graph_bucket(n_past + 1)))) {   // the captured step runs at the BUCKET's context bound
        if (ctx->mbox_host && ctx->mbox_sent - ctx->mbox_synced >= 64) {   // never overwrite a slot a queued replay has not read yet
            if (!wait_stream(ctx)) return -2;
        }
        const int b = graph_bucket(n_past + 1);
        const int pl = xpipe_usable(ctx, bucket_tmax(ctx, b)) ? 1 : 0;   // holds the slot until the stream is next synchronised (xpipe_check)
        // ANOTHER context of this process holds the device's pipeline slot right now -- typically with a resident launch that waits for its caller's next token:
        // this context's replayed five-launch graph then runs in the shadow of a persistent kernel that drains while the graph starts, and on this runtime the
        // graph's last nodes were observed to see the PREVIOUS replay's activations (tools/dbg_two_contexts.py, profiles/two_contexts_r4.txt: the returned row was
        // exactly the row of the call before, K / V rows correct; eager launches of the same kernels are not affected).  Such a call takes the eager launches.
        if (pl == 0 && !plain_graph_begin(ctx)) goto eager;      // (decided and recorded in one step under the slot's mutex)
        if (!ctx->mbox_host) {      // all three or none: a partial allocation would leave null pointers behind a non-null mbox_host on the next call
            int32_t *mh = nullptr; uint32_t *mc = nullptr, *sd = nullptr;
            const bool ok = hipHostMalloc(reinterpret_cast<void **>(&mh), 64 * 8 * 4 + 16, hipHostMallocDefault) == hipSuccess && hipMalloc(&mc, 16) == hipSuccess &&
                            hipMemset(mc, 0, 16) == hipSuccess && hipMalloc(&sd, 16) == hipSuccess && hipMemset(sd, 0, 16) == hipSuccess;
            if (!ok) {
                (void)hipGetLastError();
                if (mh) (void)hipHostFree(mh);
                if (mc) (void)hipFree(mc);
                if (sd) (void)hipFree(sd);
                BG_FAIL(-2, "could not allocate the mailbox of the replayed single-token evals");
            }
            ctx->mbox_host = mh; ctx->mbox_ctr = mc; ctx->seq_dev = sd;
        }
        if (!ctx->graph_eval[pl][form][b][0]) {
            const int L = ctx->hp.n_layer;
            const int nseg = 1;
            const int bounds[3] = {0, L, L};
            const size_t V = (size_t)ctx->hp.n_vocab;
            if (form == 1 && !ctx->logits_host) HIP_TRY(-2, hipHostMalloc(reinterpret_cast<void **>(&ctx->logits_host), host_row_bytes(ctx), hipHostMallocDefault));
            HIP_TRY(-2, hipStreamSynchronize(ctx->stream));
            for (int sgi = 0; sgi < nseg; sgi++) {
                hipGraph_t g = nullptr;
                HIP_TRY(-2, hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal));
                if (sgi == 0) hipLaunchKernelGGL(bgk::fetch_state_kernel, dim3(1), dim3(1), 0, ctx->stream, ctx->mbox_host, ctx->mbox_ctr, ctx->state, ctx->seq_dev);
                bool row_done = false;
                const bool ok = enqueue_decode_fused(ctx, bucket_tmax(ctx, b), 1, 0, bounds[sgi], bounds[sgi + 1], -1, 1, form == 1 ? ctx->logits_host : nullptr, &row_done, pl);
                if (ok && form == 1 && sgi == nseg - 1 && !row_done)
                    hipLaunchKernelGGL(bgk::logits_to_host_kernel, dim3((unsigned)((V + 1023) / 1024)), dim3(256), 0, ctx->stream, ctx->logits, ctx->logits_host, (int)V, pl == 0 ? ctx->seq_dev : nullptr, host_stamp_index(ctx));
                const hipError_t e = hipStreamEndCapture(ctx->stream, &g);
                if (!ok) { if (g) (void)hipGraphDestroy(g); return -2; }
                HIP_TRY(-2, e);
                HIP_TRY(-2, hipGraphInstantiate(&ctx->graph_eval[pl][form][b][sgi], g, nullptr, nullptr, 0));
                (void)hipGraphDestroy(g);
            }
            ctx->graph_eval_segs[form] = nseg;
        }
        int32_t *slot = ctx->mbox_host + (size_t)(ctx->mbox_sent & 63u) * 8;
        if (ctx->opt.verbose > 1) fprintf(stderr, "biogpt_hip[%p]: single-token eval as a graph replay: pl %d form %d bucket %d n_past %d token %d mailbox slot %u\n", (void *)ctx, pl, form, b, n_past, tokens[0], ctx->mbox_sent & 63u);
        if (++ctx->call_seq == 0) ctx->call_seq = 1;
        slot[0] = n_past; slot[1] = ctx->opt.causal; slot[2] = tokens[0]; slot[3] = (int32_t)ctx->call_seq;
        ctx->dev_stamp_expect = (pl == 0 && form == 0) ? ctx->call_seq : 0u; ctx->dev_stamp_tok = tokens[0]; ctx->dev_stamp_n_past = n_past;
        ctx->stamp_expect = (pl == 0 && form == 1) ? ctx->call_seq : 0u;      // the five-launch graph's row comes back with its lineage (kernels.hip.h, SEQ_*); eval_once checks it
        if (pl == 0) ctx->graph_evals++;
        if (pl == 0 && ctx->opt.fault_stale > 0 && ctx->graph_evals % ctx->opt.fault_stale == 0 && ctx->mbox_sent > 0) {
            // injected fault: this replay starts from the PREVIOUS slot -- it evaluates the previous call's token again and returns that call's row, the symptom of
            // profiles/two_contexts_r4.txt (the device's replay counter is set one back; the repair in eval_once puts it right)
            uint32_t *const back = reinterpret_cast<uint32_t *>(ctx->mbox_host + 64 * 8);
            *back = ctx->mbox_sent - 1u;
            HIP_TRY(-2, hipMemcpyAsync(ctx->mbox_ctr, back, 4, hipMemcpyHostToDevice, ctx->stream));
        }
        if (ctx->mbox_sent == ctx->mbox_synced && ctx->unsynced_from < 0) ctx->unsynced_from = n_past;      // (an asynchronous prompt chunk in front of it -- kernels_xcols.hip.h -- has already set the position)
        ctx->mbox_sent++;
        for (int sgi = 0; sgi < ctx->graph_eval_segs[form]; sgi++) HIP_TRY(-2, hipGraphLaunch(ctx->graph_eval[pl][form][b][sgi], ctx->stream));
        if (row_in_host) *row_in_host = form == 1;
        return 0;
    }
eager:
    if (!upload_state(ctx, tokens, n, n_past)) return -2;
    if (!enqueue_forward(ctx, ForwardPass::last_row(n, n_past + n))) return -2;
    return 0;
}

int biogpt_hip_eval_device(biogpt_hip_ctx *ctx, const int32_t *tokens, int32_t n, int32_t n_past) { return eval_device_impl(ctx, tokens, n, n_past, 0); }
