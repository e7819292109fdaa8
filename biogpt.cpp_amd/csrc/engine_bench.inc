// Part of engine.hip (textually included there: same translation unit, same anonymous namespace / extern "C" block): measurement entry points of the C-ABI (biogpt_hip_bench_matvec / _stream / _decode / _api_loop): HIP-event timed launches on the context's stream, profiling-build stage timelines.

int biogpt_hip_bench_matvec(biogpt_hip_ctx *ctx, int which, int layer, int reps, double *seconds_out, double *bytes_out) {
    XpCallScope xp_scope(ctx);
    clear_error();
    if (!ctx || !ctx->ready) BG_FAIL(-1, "no model");
    if (reps < 1 || (which < 4 && (layer < 0 || layer >= ctx->hp.n_layer)) || which > 13) BG_FAIL(-1, "bad argument");
    if (which == 13 && !fpipe_usable(ctx, 104)) BG_FAIL(-1, "the persistent float-weight launch is not available to this context");
    if (which >= 6 && which < 12 && !fused_decode_ok(ctx, 104)) BG_FAIL(-1, "the five-launch decode layer needs BioGPT-base shapes and block-quantized weights");
    HIP_TRY(-2, hipSetDevice(ctx->device));
    if (!resident_stop(ctx)) return -2; disarm_lineage(ctx);
    const auto &hp = ctx->hp;
    const int D = hp.d_model, F = hp.d_ff, V = hp.n_vocab, P = hp.n_positions;
    // cycling through the layers defeats L2 residency of one matrix (SURVEY 8d); the whole model still
    // fits the 256 MiB Infinity Cache -- stated in DESIGN.md
    const int32_t wt0 = ftype_to_type(hp.ftype);
    const bool chain = is_quantized(wt0) && D == 1024 && F == 4096 && D / hp.n_head == 64 && P <= 1024;
    // which == 12: the stand-alone lm_head with its weights NOT resident in the Infinity Cache: 14 copies of the matrix (Q4_0: 14 x 24.6 MB = 344 MB > 256 MB + the L2s),
    // a different one every launch -- the figure `north_star`'s "HBM roofline" means; which == 4 reads the one copy the model owns, which stays cache-resident between launches
    struct ColdCopies {
        std::vector<uint8_t *> v;
        ~ColdCopies() { for (uint8_t *q : v) if (q) (void)hipFree(q); }
    } cold;
    size_t cold_sc_off = 0, cold_qh_off = 0;
    if (which == 12) {
        const MatSlot &m = ctx->plan.lm_head;
        cold_sc_off = (m.qs_bytes + 255) & ~(size_t)255;
        cold_qh_off = cold_sc_off + ((m.sc_bytes + 255) & ~(size_t)255);
        const size_t total = cold_qh_off + m.qh_bytes + 256;
        const int ncopy = (int)std::max<size_t>(3, ((size_t)344 << 20) / std::max<size_t>(1, total) + 1);
        for (int i = 0; i < ncopy; i++) {
            uint8_t *q = nullptr;
            HIP_TRY(-2, hipMalloc(&q, total));
            cold.v.push_back(q);
            HIP_TRY(-2, hipMemcpyAsync(q, ctx->arena + m.qs, m.qs_bytes, hipMemcpyDeviceToDevice, ctx->stream));
            if (m.sc_bytes) HIP_TRY(-2, hipMemcpyAsync(q + cold_sc_off, ctx->arena + m.sc, m.sc_bytes, hipMemcpyDeviceToDevice, ctx->stream));
            if (m.qh_bytes) HIP_TRY(-2, hipMemcpyAsync(q + cold_qh_off, ctx->arena + m.qh, m.qh_bytes, hipMemcpyDeviceToDevice, ctx->stream));
        }
        HIP_TRY(-2, hipStreamSynchronize(ctx->stream));
    }
    auto launch = [&](int l) -> bool {
        ctx->launch_parity ^= 1;
        if (which == 13) return enqueue_fpipe(ctx);      // float files: all layers of one token at 104 keys as ONE persistent launch (kernels_fpipe.hip.h), no lm_head
        if (which == 11) return enqueue_decode_fused(ctx, 104, 1, 0, 0, -1, -2);   // the XCD-pipelined launch alone: all layers of one token at 104 keys, no lm_head
        if (which >= 6 && which <= 10) {   // one kernel of the five-launch decode layer (kernels_decode.hip.h), layer l mod L, `layer` = n_past for attention
            const int ll = l % hp.n_layer;
            return enqueue_decode_fused(ctx, 104, 0, 0, ll, ll + 1, which - 6);
        }
        if (which == 5) {  // attention of layer (l mod L) with `layer` keys in the cache
            bgk::AttnParams a{};
            const int ll = l % hp.n_layer, dk = D / hp.n_head;
            a.q = ctx->q; a.kcache = ctx->memory_k + (size_t)ll * P * D; a.vcache = ctx->memory_v + (size_t)ll * P * D;
            a.out = ctx->att; a.st = ctx->state;
            a.exp_tab = reinterpret_cast<const uint16_t *>(ctx->arena + ctx->plan.exp_tab);
            a.N = 1; a.D = D; a.dk = dk; a.P = P;
            a.dbg = ctx->opt.dbg; a.tstamp = ctx->tstamp;
            a.oq_q = ctx->aq_q[0]; a.oq_d = ctx->aq_d[0]; a.oq_s = ctx->aq_s[0];
            a.t_cap = std::min(P, (layer + 1 + 63) & ~63);
            if (a.t_cap <= 256) hipLaunchKernelGGL((bgk::attn_fast_kernel<1, true>), dim3(hp.n_head, 1), dim3(4 * ((a.t_cap + 63) & ~63)), 0, ctx->stream, a);
            else if (a.t_cap <= 512) hipLaunchKernelGGL((bgk::attn_fast_kernel<2, false>), dim3(hp.n_head, 1), dim3(1024), 0, ctx->stream, a);
            else hipLaunchKernelGGL((bgk::attn_fast_kernel<4, false>), dim3(hp.n_head, 1), dim3(1024), 0, ctx->stream, a);
            HIP_TRY(false, hipGetLastError());
            return true;
        }
        const LayerSlots &L = ctx->plan.layers[(size_t)(hp.n_layer ? l % hp.n_layer : 0)];
        if (which == 0) {
            const MvShape s = mv_shape(L.fc1.type, L.fc1.M, L.fc1.K);
            bgk::MatvecParams p = mv_base(ctx, L.fc1, s);
            p.x = ctx->x1; p.ldx = D; p.N = 1; p.ln_w = dev_vec(ctx, L.ln1_w); p.ln_b = dev_vec(ctx, L.ln1_b);
            p.bias = dev_vec(ctx, L.fc1_b); p.out = ctx->h; p.ldo = F;
            if (chain) { p.oq_q = ctx->aq_q[1]; p.oq_d = ctx->aq_d[1]; p.oq_s = ctx->aq_s[1]; HIP_TRY(false, launch_chain(CHAIN_FC1, p, ctx->stream)); }
            else HIP_TRY(false, (launch_mv<bgk::PRO_LN, bgk::EPI_GELU>(ctx->opt, p, s, ctx->stream)));
        } else if (which == 1) {
            const MvShape s = mv_shape(L.fc2.type, L.fc2.M, L.fc2.K);
            bgk::MatvecParams p = mv_base(ctx, L.fc2, s);
            p.x = ctx->h; p.ldx = F; p.N = 1; p.bias = dev_vec(ctx, L.fc2_b);
            p.resid = ctx->x1; p.ldr = D; p.out = ctx->x; p.ldo = D;
            if (chain) { p.aq_q = ctx->aq_q[1]; p.aq_d = ctx->aq_d[1]; p.aq_s = ctx->aq_s[1]; HIP_TRY(false, launch_chain(CHAIN_FC2, p, ctx->stream)); }
            else HIP_TRY(false, (launch_mv<bgk::PRO_PLAIN, bgk::EPI_RESID>(ctx->opt, p, s, ctx->stream)));
        } else if (which == 2) {
            const MvShape s = mv_shape(L.qkv.type, L.qkv.M, L.qkv.K);
            bgk::MatvecParams p = mv_base(ctx, L.qkv, s);
            p.x = ctx->x; p.ldx = D; p.N = 1; p.ln_w = dev_vec(ctx, L.ln0_w); p.ln_b = dev_vec(ctx, L.ln0_b);
            p.bias = dev_vec(ctx, L.qkv_b); p.q_out = ctx->q;
            p.kcache = ctx->memory_k + (size_t)(l % hp.n_layer) * P * D; p.vcache = ctx->memory_v + (size_t)(l % hp.n_layer) * P * D;
            p.q_scale = 0.125f;
            HIP_TRY(false, (launch_mv<bgk::PRO_LN, bgk::EPI_QKV>(ctx->opt, p, s, ctx->stream)));
        } else if (which == 3) {
            const MvShape s = mv_shape(L.o.type, L.o.M, L.o.K);
            bgk::MatvecParams p = mv_base(ctx, L.o, s);
            p.x = ctx->att; p.ldx = D; p.N = 1; p.bias = dev_vec(ctx, L.o_b);
            p.resid = ctx->x; p.ldr = D; p.out = ctx->x1; p.ldo = D;
            if (chain) { p.aq_q = ctx->aq_q[0]; p.aq_d = ctx->aq_d[0]; p.aq_s = ctx->aq_s[0]; HIP_TRY(false, launch_chain(CHAIN_OPROJ, p, ctx->stream)); }
            else HIP_TRY(false, (launch_mv<bgk::PRO_PLAIN, bgk::EPI_RESID>(ctx->opt, p, s, ctx->stream)));
        } else {
            const MatSlot &m = ctx->plan.lm_head;
            const MvShape s = mv_shape(m.type, m.M, m.K);
            bgk::MatvecParams p = mv_base(ctx, m, s);
            p.x = ctx->x; p.ldx = D; p.N = 1; p.ln_w = dev_vec(ctx, ctx->plan.ln_w); p.ln_b = dev_vec(ctx, ctx->plan.ln_b);
            p.out = ctx->logits; p.ldo = V; p.pmax_val = ctx->pmax_val; p.pmax_idx = ctx->pmax_idx;
            if (which == 12) {
                const uint8_t *q = cold.v[(size_t)l % cold.v.size()];
                p.W.qs = q; p.W.sc = q + cold_sc_off; p.W.qh = reinterpret_cast<const uint32_t *>(q + cold_qh_off);
            }
            HIP_TRY(false, (launch_mv<bgk::PRO_LN, bgk::EPI_LOGITS>(ctx->opt, p, s, ctx->stream)));
        }
        return true;
    };
    const int32_t tok0 = 0;
    if (!upload_state(ctx, &tok0, 1, which == 5 ? layer : (which >= 6 && which != 12 ? 103 : 0))) return -2;
    const bool stamps = (ctx->opt.dbg & 32) != 0 && which < 5;
    if (stamps) {
        if (!ctx->tstamp) HIP_TRY(-2, hipMalloc(&ctx->tstamp, 2 * 8192 * 8 * sizeof(unsigned long long)));
        HIP_TRY(-2, hipMemset(ctx->tstamp, 0, 2 * 8192 * 8 * sizeof(unsigned long long)));
    }
    float ms = 0.0f;
    if (which >= 6) {
        // the decode-layer kernels finish faster than the host can launch them one by one (~3.3 us per eager launch):
        // capture one sweep over the layers (which == 12: over the copies of the output projection) and time graph replays, as the decode step itself is replayed
        const int per = (which == 11 || which == 13) ? 4 : which == 12 ? (int)cold.v.size() : std::max(1, hp.n_layer);
        hipGraph_t g = nullptr;
        hipGraphExec_t ge = nullptr;
        HIP_TRY(-2, hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal));
        bool ok = true;
        for (int i = 0; i < per && ok; i++) ok = launch(layer + i);
        const hipError_t ce = hipStreamEndCapture(ctx->stream, &g);
        if (!ok || ce != hipSuccess) { if (g) (void)hipGraphDestroy(g); BG_FAIL(-2, "graph capture of the decode kernel failed"); }
        HIP_TRY(-2, hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
        (void)hipGraphDestroy(g);
        const int sweeps = std::max(1, reps / per);
        for (int i = 0; i < 2; i++) HIP_TRY(-2, hipGraphLaunch(ge, ctx->stream));
        HIP_TRY(-2, hipEventRecord(ctx->ev0, ctx->stream));
        for (int i = 0; i < sweeps; i++) HIP_TRY(-2, hipGraphLaunch(ge, ctx->stream));
        HIP_TRY(-2, hipEventRecord(ctx->ev1, ctx->stream));
        HIP_TRY(-2, hipEventSynchronize(ctx->ev1));
        HIP_TRY(-2, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
        (void)hipGraphExecDestroy(ge);
        reps = sweeps * per;
    } else {
        for (int i = 0; i < 3; i++) if (!launch(layer + i)) return -2;
        HIP_TRY(-2, hipEventRecord(ctx->ev0, ctx->stream));
        for (int i = 0; i < reps; i++) if (!launch(layer + i)) return -2;
        HIP_TRY(-2, hipEventRecord(ctx->ev1, ctx->stream));
        HIP_TRY(-2, hipEventSynchronize(ctx->ev1));
        HIP_TRY(-2, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    }
    if (seconds_out) *seconds_out = (double)ms * 1e-3 / reps;
    if (stamps) {  // timeline of the last two launches (A then B), shader-clock cycles
        const MatSlot *mm = which == 0 ? &ctx->plan.layers[0].fc1 : which == 1 ? &ctx->plan.layers[0].fc2
                          : which == 2 ? &ctx->plan.layers[0].qkv : which == 3 ? &ctx->plan.layers[0].o : &ctx->plan.lm_head;
        int grid = mv_shape(mm->type, mm->M, mm->K).grid;
        if (which == 4 && ctx->opt.lm_stream && mm->K == 1024 && is_quantized(mm->type)) grid = ((mm->M + 63) / 64 + 2) / 3;      // lm_stream_kernel's
        std::vector<unsigned long long> h(2 * (size_t)grid * 8);
        HIP_TRY(-2, hipMemcpy(h.data(), ctx->tstamp, h.size() * 8, hipMemcpyDeviceToHost));
        const int pb = ctx->launch_parity, pa = pb ^ 1;  // B = last launch, A = the one before
        auto at = [&](int par, int b, int k) { return h[((size_t)par * grid + b) * 8 + k]; };
        unsigned long long a_min0 = ~0ull, a_max6 = 0, b_min0 = ~0ull, a_max0 = 0;
        std::vector<double> seg[6];
        for (int b = 0; b < grid; b++) {
            a_min0 = std::min(a_min0, at(pa, b, 0)); a_max0 = std::max(a_max0, at(pa, b, 0));
            a_max6 = std::max(a_max6, at(pa, b, 6)); b_min0 = std::min(b_min0, at(pb, b, 0));
            for (int k = 0; k < 6; k++) seg[k].push_back((double)(at(pa, b, k + 1) - at(pa, b, k)));
        }
        fprintf(stderr, "timeline which=%d grid=%d: span(first entry -> last exit)=%llu cyc, entry spread=%llu, gap to next kernel's first entry=%lld\n",
                which, grid, a_max6 - a_min0, a_max0 - a_min0, (long long)(b_min0 - a_max6));
        const char *names[6] = {"entry->loads issued", "->x arrived", "->prologue done", "->barrier passed", "->main loop done", "->finish+epilogue"};
        for (int k = 0; k < 6; k++) {
            std::sort(seg[k].begin(), seg[k].end());
            fprintf(stderr, "   %-22s med %7.0f  max %7.0f cyc\n", names[k], seg[k][seg[k].size() / 2], seg[k].back());
        }
    }
    if (bytes_out) {
        if (which == 5) { *bytes_out = 2.0 * (layer + 1) * D * 4; return 0; }  // K and V rows of one layer
        if (which == 11 || which == 13) {   // every layer's four matrices + K / V rows at 104 keys + the new K / V rows + one x column in and out
            double b = 0.0;
            for (const auto &L : ctx->plan.layers)
                for (const MatSlot *m : {&L.qkv, &L.o, &L.fc1, &L.fc2}) b += (double)file_row_bytes(m->type, m->K) * (double)m->M;
            b += hp.n_layer * (2.0 * 104 * D * 4 + 2.0 * D * 4) + 8.0 * D;
            if (which == 11) b += (double)file_row_bytes(ctx->plan.lm_head.type, ctx->plan.lm_head.K) * (double)ctx->plan.lm_head.M + 4.0 * V;   // + the output projection and the logits row
            *bytes_out = b;
            return 0;
        }
        if (which == 7) { *bytes_out = 2.0 * 104 * D * 4 + 4.0 * D + 1.0 * D + 8.0 * (D / 32); return 0; }   // K, V rows at 104 keys + q + Q8 output
        if (which >= 6 && which < 12) {   // SURVEY 8d: rows*cols*(block_bytes/32) + 4*cols (activation) + 4*rows (out)
            const MatSlot *m6 = which == 6 ? &ctx->plan.layers[0].qkv : which == 8 ? &ctx->plan.layers[0].o : which == 9 ? &ctx->plan.layers[0].fc1 : &ctx->plan.layers[0].fc2;
            *bytes_out = (double)file_row_bytes(m6->type, m6->K) * (double)m6->M + 4.0 * (double)m6->K + 4.0 * (double)m6->M;
            return 0;
        }
        const MatSlot *m = which == 0 ? &ctx->plan.layers[0].fc1 : which == 1 ? &ctx->plan.layers[0].fc2
                         : which == 2 ? &ctx->plan.layers[0].qkv : which == 3 ? &ctx->plan.layers[0].o : &ctx->plan.lm_head;
        // SURVEY 8d: rows*cols*(block_bytes/32) + 4*cols (activation) + 4*rows (out)
        *bytes_out = (double)file_row_bytes(m->type, m->K) * (double)m->M + 4.0 * (double)m->K + 4.0 * (double)m->M;
    }
    return 0;
}

// The decode mat-vec over every block-quantized matrix of the model in ONE launch (kernels_sweep.hip.h), each launch on one of TWO copies of the weights in turn (Q4_0: 2 x
// 195 MB > the 256 MB Infinity Cache: the bytes come from HBM).  seconds_out: per launch (HIP events around `reps` launches); bytes_out: SURVEY 8(d)'s figure per launch
// (rows * cols * block_bytes / 32 + 4 * cols + 4 * rows over the 97 matrices); check_out: max |device - host| over ~200 sampled rows recomputed on the host with the
// reference's arithmetic (0 = bit-identical; -1 = not checked).
// which: 0 every matrix (two copies in turn); 1 lm_head alone; 2 the D x D shapes alone -- q/k/v + out_proj of every layer, K = 1024: north_star's "mat-vec at d_model = 1024" to
// the letter (Q4_0: 56.6 MB); 3 fc2 alone (K = 4096); 4 fc1 alone (K = 1024, 4096 rows).  1 .. 4: as many copies in turn as exceed the Infinity Cache.
// rows_out (rows_cap floats; may be null): the launch's output rows, matrix after matrix in the order of the list above (per layer q/k/v, out_proj, fc1, fc2; then lm_head);
// xq_out (1024 + 4096 int8) / xd_out (32 + 128 floats): the two Q8 activation vectors the rows were computed with -- what a test needs to recompute a row with the ORACLE's
// vec_dot (tests/test_gpu_decode_fused.py).
int biogpt_hip_bench_sweep_ex(biogpt_hip_ctx *ctx, int which, int reps, double *seconds_out, double *bytes_out, double *check_out, float *rows_out, size_t rows_cap,
                              int8_t *xq_out, float *xd_out) {
    XpCallScope xp_scope(ctx);
    clear_error();
    if (!ctx || !ctx->ready) BG_FAIL(-1, "no model");
    const auto &hp = ctx->hp;
    const int32_t wt = ftype_to_type(hp.ftype);
    if (reps < 1 || which < 0 || which > 4 || !is_quantized(wt) || hp.d_model != 1024 || hp.d_ff != 4096) BG_FAIL(-1, "the sweep needs block-quantized BioGPT-base shapes (K = 1024 / 4096)");
    HIP_TRY(-2, hipSetDevice(ctx->device));
    if (!resident_stop(ctx)) return -2; disarm_lineage(ctx);
    struct Bufs {
        std::vector<void *> v;
        ~Bufs() { for (void *q : v) if (q) (void)hipFree(q); }
        void *get(size_t n) { void *q = nullptr; if (hipMalloc(&q, n) != hipSuccess) return nullptr; v.push_back(q); return q; }
    } bufs;
    std::vector<const MatSlot *> mats;
    for (const auto &L : ctx->plan.layers) {
        if (which == 0 || which == 2) { mats.push_back(&L.qkv); mats.push_back(&L.o); }
        if (which == 0 || which == 4) mats.push_back(&L.fc1);
        if (which == 0 || which == 3) mats.push_back(&L.fc2);
    }
    if (which == 0 || which == 1) mats.push_back(&ctx->plan.lm_head);      // which == 1: the output projection alone (24.4 MB of Q4_0), on NCOPY copies in turn
    // the second copy of the weights: the span of the arena that holds the matrices
    size_t lo = ~(size_t)0, hi = 0;
    for (const MatSlot *m : mats) { lo = std::min({lo, m->qs, m->sc_bytes ? m->sc : lo, m->qh_bytes ? m->qh : lo}); hi = std::max({hi, m->qs + m->qs_bytes, m->sc + m->sc_bytes, m->qh + m->qh_bytes}); }
    const int NCOPY = which == 0 ? 2 : (int)std::max<size_t>(3, ((size_t)344 << 20) / std::max<size_t>(1, hi - lo) + 1);      // copy 0 = the arena itself
    std::vector<uint8_t *> copies((size_t)NCOPY, nullptr);
    for (int cpy = 1; cpy < NCOPY; cpy++) {
        copies[(size_t)cpy] = static_cast<uint8_t *>(bufs.get(hi - lo));
        if (!copies[(size_t)cpy]) BG_FAIL(-2, "no memory for a copy of the weights (%zu bytes)", hi - lo);
        HIP_TRY(-2, hipMemcpyAsync(copies[(size_t)cpy], ctx->arena + lo, hi - lo, hipMemcpyDeviceToDevice, ctx->stream));
    }
    // activations: one vector per input width, seeded; Q8_0 form (fp16-representable d, integer block sums) or Q8_1 (f32 d, s = d * sum)
    const bool q81 = wt == T_Q4_1 || wt == T_Q5_1;
    std::vector<int8_t> hxq[2]; std::vector<float> hxd[2]; std::vector<uint32_t> hxs[2];
    int8_t *dxq[2]; float *dxd[2]; uint32_t *dxs[2];
    uint64_t rs = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() { rs ^= rs << 13; rs ^= rs >> 7; rs ^= rs << 17; return rs; };
    for (int w = 0; w < 2; w++) {
        const int K = w == 0 ? 1024 : 4096;
        hxq[w].resize((size_t)K); hxd[w].resize((size_t)K / 32); hxs[w].resize((size_t)K / 32);
        for (int b = 0; b < K / 32; b++) {
            int sum = 0;
            for (int e = 0; e < 32; e++) { const int v = (int)(rnd() % 255) - 127; hxq[w][(size_t)b * 32 + e] = (int8_t)v; sum += v; }
            const float d = f16_to_f32(f32_to_f16(0.004f + 1e-5f * (float)(rnd() % 400)));
            hxd[w][(size_t)b] = d;
            float sf = (float)sum * d;
            uint32_t bits; std::memcpy(&bits, &sf, 4);
            hxs[w][(size_t)b] = q81 ? bits : (uint32_t)sum;
        }
        dxq[w] = static_cast<int8_t *>(bufs.get((size_t)K)); dxd[w] = static_cast<float *>(bufs.get((size_t)K / 32 * 4)); dxs[w] = static_cast<uint32_t *>(bufs.get((size_t)K / 32 * 4));
        if (!dxq[w] || !dxd[w] || !dxs[w]) BG_FAIL(-2, "no memory");
        HIP_TRY(-2, hipMemcpy(dxq[w], hxq[w].data(), (size_t)K, hipMemcpyHostToDevice));
        HIP_TRY(-2, hipMemcpy(dxd[w], hxd[w].data(), (size_t)K / 32 * 4, hipMemcpyHostToDevice));
        HIP_TRY(-2, hipMemcpy(dxs[w], hxs[w].data(), (size_t)K / 32 * 4, hipMemcpyHostToDevice));
    }
    size_t rows_total = 0;
    for (const MatSlot *m : mats) rows_total += (size_t)m->M;
    float *out = static_cast<float *>(bufs.get(rows_total * 4));
    if (!out) BG_FAIL(-2, "no memory");
    std::vector<std::vector<bgk::SweepJob>> jobs((size_t)NCOPY);
    std::vector<int32_t> unit_job;
    std::vector<size_t> out_off;
    double bytes = 0.0;
    size_t ro = 0;
    for (size_t jm = 0; jm < mats.size(); jm++) {
        const MatSlot &m = *mats[jm];
        if (m.K != 1024 && m.K != 4096) BG_FAIL(-1, "row length %lld", (long long)m.K);
        const int w = m.K == 1024 ? 0 : 1;
        const int64_t units = (m.M * (m.K / 32) + bgk::SWEEP_UNIT - 1) / bgk::SWEEP_UNIT;
        for (int cpy = 0; cpy < NCOPY; cpy++) {
            bgk::SweepJob j{};
            j.W = dev_matrix(ctx, m);
            if (cpy >= 1) { const uint8_t *copy = copies[(size_t)cpy]; j.W.qs = copy + (m.qs - lo); j.W.sc = copy + (m.sc - lo); j.W.qh = reinterpret_cast<const uint32_t *>(copy + (m.qh - lo)); }
            j.xq = dxq[w]; j.xd = dxd[w]; j.xs = dxs[w]; j.out = out + ro; j.unit0 = (int32_t)unit_job.size();
            jobs[cpy].push_back(j);
        }
        out_off.push_back(ro);
        for (int64_t u = 0; u < units; u++) unit_job.push_back((int32_t)jm);
        ro += (size_t)m.M;
        bytes += (double)file_row_bytes(m.type, m.K) * (double)m.M + 4.0 * (double)m.K + 4.0 * (double)m.M;
    }
    std::vector<bgk::SweepJob *> djobs((size_t)NCOPY, nullptr);
    for (int cpy = 0; cpy < NCOPY; cpy++) {
        djobs[cpy] = static_cast<bgk::SweepJob *>(bufs.get(jobs[cpy].size() * sizeof(bgk::SweepJob)));
        if (!djobs[cpy]) BG_FAIL(-2, "no memory");
        HIP_TRY(-2, hipMemcpy(djobs[cpy], jobs[cpy].data(), jobs[cpy].size() * sizeof(bgk::SweepJob), hipMemcpyHostToDevice));
    }
    int32_t *dunit = static_cast<int32_t *>(bufs.get(unit_job.size() * 4));
    if (!dunit) BG_FAIL(-2, "no memory");
    HIP_TRY(-2, hipMemcpy(dunit, unit_job.data(), unit_job.size() * 4, hipMemcpyHostToDevice));
    auto launch = [&](int cpy) {
        bgk::SweepParams sp{djobs[cpy], dunit};
        const dim3 grid((unsigned)unit_job.size());
        switch (wt) {
            case T_Q4_0: hipLaunchKernelGGL((bgk::matvec_sweep_kernel<bgk::W_Q4_0>), grid, dim3(512), 0, ctx->stream, sp); break;
            case T_Q4_1: hipLaunchKernelGGL((bgk::matvec_sweep_kernel<bgk::W_Q4_1>), grid, dim3(512), 0, ctx->stream, sp); break;
            case T_Q5_0: hipLaunchKernelGGL((bgk::matvec_sweep_kernel<bgk::W_Q5_0>), grid, dim3(512), 0, ctx->stream, sp); break;
            case T_Q5_1: hipLaunchKernelGGL((bgk::matvec_sweep_kernel<bgk::W_Q5_1>), grid, dim3(512), 0, ctx->stream, sp); break;
            default: hipLaunchKernelGGL((bgk::matvec_sweep_kernel<bgk::W_Q8_0>), grid, dim3(512), 0, ctx->stream, sp); break;
        }
    };
    for (int i = 0; i < 4; i++) launch(i % NCOPY);
    HIP_TRY(-2, hipGetLastError());
    HIP_TRY(-2, hipEventRecord(ctx->ev0, ctx->stream));
    for (int i = 0; i < reps; i++) launch(i % NCOPY);
    HIP_TRY(-2, hipEventRecord(ctx->ev1, ctx->stream));
    HIP_TRY(-2, hipEventSynchronize(ctx->ev1));
    float ms = 0.0f;
    HIP_TRY(-2, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    if (seconds_out) *seconds_out = (double)ms * 1e-3 / reps;
    if (bytes_out) *bytes_out = bytes;
    if (rows_out) HIP_TRY(-2, hipMemcpy(rows_out, out, std::min(rows_cap, rows_total) * 4, hipMemcpyDeviceToHost));
    if (xq_out) { std::memcpy(xq_out, hxq[0].data(), 1024); std::memcpy(xq_out + 1024, hxq[1].data(), 4096); }
    if (xd_out) { std::memcpy(xd_out, hxd[0].data(), 32 * 4); std::memcpy(xd_out + 32, hxd[1].data(), 128 * 4); }
    if (check_out) {
        // ~200 rows spread over the matrices, recomputed here from the arena's bytes with unit_dot_quant's expressions (Q4_0 and Q8_0; the other formats are not checked)
        *check_out = -1.0;
        if (wt == T_Q4_0 || wt == T_Q8_0) {
            double worst = 0.0;
            const size_t qb = wt == T_Q8_0 ? 32 : 16;
            for (size_t jm = 0; jm < mats.size(); jm++) {
                const MatSlot &m = *mats[jm];
                const int w = m.K == 1024 ? 0 : 1, BPR = (int)(m.K / 32);
                for (int pick = 0; pick < 2; pick++) {
                    const int64_t row = pick == 0 ? (int64_t)(rnd() % (uint64_t)m.M) : m.M - 1;
                    std::vector<uint8_t> q((size_t)BPR * qb); std::vector<uint16_t> sc((size_t)BPR);
                    HIP_TRY(-2, hipMemcpy(q.data(), ctx->arena + m.qs + (size_t)row * BPR * qb, q.size(), hipMemcpyDeviceToHost));
                    HIP_TRY(-2, hipMemcpy(sc.data(), ctx->arena + m.sc + (size_t)row * BPR * 2, sc.size() * 2, hipMemcpyDeviceToHost));
                    float dev = 0.0f;
                    HIP_TRY(-2, hipMemcpy(&dev, out + out_off[jm] + (size_t)row, 4, hipMemcpyDeviceToHost));
                    float sum = 0.0f;
                    for (int b = 0; b < BPR; b++) {
                        const int8_t *x = hxq[w].data() + (size_t)b * 32;
                        int si = 0;
                        if (wt == T_Q8_0) { for (int e = 0; e < 32; e++) si += (int)(int8_t)q[(size_t)b * 32 + e] * (int)x[e]; }
                        else { for (int e = 0; e < 16; e++) { const uint8_t v = q[(size_t)b * 16 + e]; si += ((int)(v & 15) - 8) * (int)x[e] + ((int)(v >> 4) - 8) * (int)x[e + 16]; } }
                        const float dw = f16_to_f32(sc[(size_t)b]), dx = hxd[w][(size_t)b];
                        const float term = wt == T_Q8_0 ? (float)si * (dw * dx) : ((float)si * dw) * dx;
                        sum = sum + term;
                    }
                    worst = std::max(worst, (double)std::fabs(sum - dev));
                }
            }
            *check_out = worst;
        }
    }
    return 0;
}

int biogpt_hip_bench_sweep(biogpt_hip_ctx *ctx, int which, int reps, double *seconds_out, double *bytes_out, double *check_out) {
    return biogpt_hip_bench_sweep_ex(ctx, which, reps, seconds_out, bytes_out, check_out, nullptr, 0, nullptr, nullptr);
}

int biogpt_hip_bench_stream(biogpt_hip_ctx *ctx, int32_t rows, int reps, int steps, double *seconds_out, double *bytes_out) {
    // The decode mat-vec kernel body on a weight stream far larger than the caches: rows x 1024 synthetic
    // Q4_0 blocks (random bytes), the model's final LayerNorm as prologue, logits epilogue without arg-max.
    clear_error();
    if (!ctx || !ctx->ready) BG_FAIL(-1, "no model");
    if (ctx->hp.d_model != 1024 || rows < 1024 || rows % 1024 || reps < 1 || steps < 2) BG_FAIL(-1, "bad argument");
    HIP_TRY(-2, hipSetDevice(ctx->device));
    if (!resident_stop(ctx)) return -2; disarm_lineage(ctx);
    const size_t nblk = (size_t)rows * 32;
    uint8_t *qs = nullptr, *sc = nullptr;
    float *out = nullptr;
    HIP_TRY(-2, hipMalloc(&qs, nblk * 16));
    HIP_TRY(-2, hipMalloc(&sc, nblk * 2));
    HIP_TRY(-2, hipMalloc(&out, (size_t)rows * 4));
    {
        std::vector<uint32_t> h(nblk * 4);
        uint64_t s = 0x9E3779B97F4A7C15ull;
        for (auto &v : h) { s = s * 6364136223846793005ull + 1442695040888963407ull; v = (uint32_t)(s >> 32); }
        HIP_TRY(-2, hipMemcpy(qs, h.data(), nblk * 16, hipMemcpyHostToDevice));
        std::vector<uint16_t> d(nblk, 0x2000);  // fp16 2^-7: finite, no NaN/inf scales
        HIP_TRY(-2, hipMemcpy(sc, d.data(), nblk * 2, hipMemcpyHostToDevice));
    }
    bgk::MatvecParams p{};
    p.W.qs = qs; p.W.sc = sc; p.W.qh = nullptr; p.W.type = T_Q4_0; p.W.M = rows; p.W.K = 1024;
    p.x = ctx->x; p.ldx = 1024; p.N = 1; p.eps = 1e-5f;
    p.ln_w = dev_vec(ctx, ctx->plan.ln_w); p.ln_b = dev_vec(ctx, ctx->plan.ln_b);
    p.out = out; p.ldo = rows; p.st = ctx->state; p.inv_k = 1.0 / 1024.0; p.k_pow2 = 1;
    p.rpw = 2 * steps;
    const int grid = (rows + 4 * p.rpw - 1) / (4 * p.rpw);
    const size_t sm = bgk::matvec_fast_smem_bytes(1024, p.rpw);
    auto launch = [&] { hipLaunchKernelGGL((bgk::matvec_fast_kernel<bgk::W_Q4_0, bgk::PRO_LN, bgk::EPI_LOGITS, 1024, 4, 1>), dim3(grid), dim3(256), sm, ctx->stream, p); };
    for (int i = 0; i < 2; i++) launch();
    HIP_TRY(-2, hipEventRecord(ctx->ev0, ctx->stream));
    for (int i = 0; i < reps; i++) launch();
    HIP_TRY(-2, hipEventRecord(ctx->ev1, ctx->stream));
    HIP_TRY(-2, hipEventSynchronize(ctx->ev1));
    float ms = 0.0f;
    HIP_TRY(-2, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    if (seconds_out) *seconds_out = (double)ms * 1e-3 / reps;
    if (bytes_out) *bytes_out = 18.0 * (double)nblk + 4.0 * 1024 + 4.0 * rows;   // file-density bytes (18 B / block) + x + out
    (void)hipFree(qs); (void)hipFree(sc); (void)hipFree(out);
    return 0;
}

int biogpt_hip_bench_decode(biogpt_hip_ctx *ctx, int32_t n_past, int reps, double *seconds_out) {
    XpCallScope xp_scope(ctx);
    clear_error();
    if (!ctx || !ctx->ready) BG_FAIL(-1, "no model");
    if (reps < 1 || n_past < 0 || n_past >= ctx->hp.n_positions) BG_FAIL(-1, "bad argument");
    HIP_TRY(-2, hipSetDevice(ctx->device));
    if (!resident_stop(ctx)) return -2; disarm_lineage(ctx);
    const int b = graph_bucket(n_past + 1);
    if ((ctx->opt.dbg & 224) && !ctx->tstamp) {
        HIP_TRY(-2, hipMalloc(&ctx->tstamp, (size_t)4 << 20));
        HIP_TRY(-2, hipMemset(ctx->tstamp, 0, (size_t)4 << 20));
    }
    const int pl = pipeline_pl(ctx, bucket_tmax(ctx, b));
    if (pl == 0 && !plain_graph_begin(ctx)) BG_FAIL(-2, "another context holds the device's pipeline slot: the captured five-launch step is not replayed beside its persistent launch");
    if (!ensure_graph(ctx, 0, b, pl)) return -2;
    const int32_t tok0 = 2;
    if (!upload_state(ctx, &tok0, 1, n_past)) return -2;
    for (int i = 0; i < 3; i++) HIP_TRY(-2, hipGraphLaunch(ctx->graph_step[pl][0][b], ctx->stream));
    HIP_TRY(-2, hipEventRecord(ctx->ev0, ctx->stream));
    for (int i = 0; i < reps; i++) HIP_TRY(-2, hipGraphLaunch(ctx->graph_step[pl][0][b], ctx->stream));
    HIP_TRY(-2, hipEventRecord(ctx->ev1, ctx->stream));
    HIP_TRY(-2, hipEventSynchronize(ctx->ev1));
    float ms = 0.0f;
    HIP_TRY(-2, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    if (seconds_out) *seconds_out = (double)ms * 1e-3 / reps;
    if (!xpipe_check(ctx)) return -2;
    if ((ctx->opt.dbg & 128) && ctx->tstamp && pl == 1 && bucket_tmax(ctx, b) > 256) {
        // long-context variant (kernels_xlong.hip.h): [n_layer][32] stamps of workgroup 0 of the layer's own XCDs (it is also the first helper -- and the combiner -- of head 2 xcd)
        const int nl = ctx->hp.n_layer;
        std::vector<unsigned long long> w((size_t)nl * 32);
        HIP_TRY(-2, hipMemcpy(w.data(), ctx->tstamp, w.size() * 8, hipMemcpyDeviceToHost));
        const int order[18] = {0, 6, 1, 16, 17, 18, 19, 20, 21, 22, 8, 3, 9, 10, 11, 4, 12, 5};
        const char *names[18] = {"x arrived", "LayerNorm + Q8 done", "q/k/v rows published", "helper: q row arrived", "helper: own scores published", "helper: head's scores arrived",
                                 "helper: max / exp / sum done", "helper: partial PV published", "combiner: partials arrived", "combiner: attention output published",
                                 "attention output arrived", "out_proj rows published", "x1 arrived", "LayerNorm + Q8 done", "fc1 rows + GELU done",
                                 "fc1 activations published", "fc1 activations arrived", "layer output published"};
        double seg[18] = {}, hop = 0.0;
        for (int l = 1; l < nl; l++) {
            for (int k = 1; k < 18; k++) seg[k] += (double)(long long)(w[(size_t)l * 32 + order[k]] - w[(size_t)l * 32 + order[k - 1]]) * 0.01;
            hop += (double)(long long)(w[(size_t)l * 32] - w[(size_t)(l - 1) * 32 + 5]) * 0.01;
        }
        const double n = nl > 1 ? nl - 1 : 1;
        fprintf(stderr, "XCD pipeline, long-context variant: wall clock of workgroup 0 of the layer's XCDs, mean over layers 1.. (us since the previous line)\n");
        fprintf(stderr, "   %-40s %6.2f   (previous layer's output published -> seen on the next XCD)\n", names[0], hop / n);
        for (int k = 1; k < 18; k++) fprintf(stderr, "   %-40s %6.2f\n", names[k], seg[k] / n);
        fprintf(stderr, "   one layer = %.2f us\n", nl > 1 ? (double)(long long)(w[(size_t)(nl - 1) * 32 + 5] - w[5]) * 0.01 / n : 0.0);
    } else if ((ctx->opt.dbg & 128) && ctx->tstamp && pl == 1) {
        // XCD pipeline (build with EXTRA=-DBIOGPT_HIP_PROFILE_HOOKS): wall clock (100 MHz) of workgroup 0 of each layer's XCD, last replay
        const int nl = ctx->hp.n_layer;
        std::vector<unsigned long long> w((size_t)nl * 16);
        HIP_TRY(-2, hipMemcpy(w.data(), ctx->tstamp, w.size() * 8, hipMemcpyDeviceToHost));
        // stamp order inside a layer
        const int order[16] = {0, 6, 1, 7, 13, 14, 15, 2, 8, 3, 9, 10, 11, 4, 12, 5};
        const char *names[16] = {"x arrived", "LayerNorm + Q8 done", "q/k/v rows stored / handed over", "q/k/v rows arrived", "scores + max", "exp + sum",
                                 "PV + slice sums in LDS", "attention output published", "attention output arrived", "out_proj rows published", "x1 arrived",
                                 "LayerNorm + Q8 done", "fc1 rows + GELU done", "fc1 activations published", "fc1 activations arrived", "layer output published"};
        double seg[16] = {}, hop = 0.0;
        for (int l = 1; l < nl; l++) {
            for (int k = 1; k < 16; k++) seg[k] += (double)(long long)(w[(size_t)l * 16 + order[k]] - w[(size_t)l * 16 + order[k - 1]]) * 0.01;
            hop += (double)(long long)(w[(size_t)l * 16] - w[(size_t)(l - 1) * 16 + 5]) * 0.01;
        }
        const double n = nl > 1 ? nl - 1 : 1;
        fprintf(stderr, "XCD pipeline: wall clock of workgroup 0 of the layer's XCD, mean over layers 1.. (us since the previous line)\n");
        fprintf(stderr, "   %-36s %6.2f   (previous layer's output published -> seen on the next XCD)\n", names[0], hop / n);
        for (int k = 1; k < 16; k++) fprintf(stderr, "   %-36s %6.2f\n", names[k], seg[k] / n);
        fprintf(stderr, "   one layer = %.2f us\n", nl > 1 ? (double)(long long)(w[(size_t)(nl - 1) * 16 + 5] - w[5]) * 0.01 / n : 0.0);
        {   // the two cross-XCD hops by the XCD they arrive on: x (layer l-1's MLP half on XCD 2l-1 -> layer l's attention half on XCD 2l mod 8), x1 (XCD 2l -> 2l+1)
            double hx[4] = {}, hx1[4] = {}; int cnt[4] = {};
            for (int l = 1; l < nl; l++) {
                hx[l & 3] += (double)(long long)(w[(size_t)l * 16] - w[(size_t)(l - 1) * 16 + 5]) * 0.01;
                hx1[l & 3] += (double)(long long)(w[(size_t)l * 16 + 9] - w[(size_t)l * 16 + 3]) * 0.01;
                cnt[l & 3]++;
            }
            for (int k = 0; k < 4; k++)
                if (cnt[k]) fprintf(stderr, "   hops onto XCD %d / %d: x %.2f us (from XCD %d), x1 %.2f us\n", 2 * k, 2 * k + 1, hx[k] / cnt[k], (2 * k + 7) & 7, hx1[k] / cnt[k]);
        }
        // the last layer, every workgroup of its XCD: us since workgroup 0 saw the layer input
        std::vector<unsigned long long> ws((size_t)32 * 16);
        HIP_TRY(-2, hipMemcpy(ws.data(), ctx->tstamp + (size_t)nl * 16, ws.size() * 8, hipMemcpyDeviceToHost));
        fprintf(stderr, "   last layer, per workgroup (columns: the 16 events above):\n");
        for (int sl = 0; sl < 32; sl++) {
            fprintf(stderr, "   wg %2d:", sl);
            for (int k = 0; k < 16; k++) {
                const unsigned long long t = ws[(size_t)sl * 16 + order[k]];
                if (t == 0) fprintf(stderr, "      -"); else fprintf(stderr, " %6.2f", (double)(long long)(t - ws[0]) * 0.01);
            }
            fprintf(stderr, "\n");
        }
    }
    if ((ctx->opt.dbg & 64) && ctx->tstamp && fused_decode_ok(ctx, bucket_tmax(ctx, b))) {
        // wall-clock (100 MHz) entry / exit of every workgroup of the last replay: per kernel, relative to the previous kernel's last exit
        const int nk = 5 * ctx->hp.n_layer;
        std::vector<unsigned long long> w((size_t)nk * 2048);
        HIP_TRY(-2, hipMemcpy(w.data(), ctx->tstamp + 128, w.size() * 8, hipMemcpyDeviceToHost));
        const int grids[5] = {192, 16, 64, 128, 128};      // launch_decode_layer's workgroups
        const char *kn[5] = {"dec_qkv  ", "dec_attn ", "dec_oproj", "dec_fc1  ", "dec_fc2  "};
        double acc[5][5] = {};
        unsigned long long prev_exit = 0;
        for (int k = 0; k < nk; k++) {
            unsigned long long e0 = ~0ull, e1 = 0, x0 = ~0ull, x1 = 0;
            for (int g = 0; g < grids[k % 5]; g++) {
                const unsigned long long en = w[((size_t)k * 1024 + g) * 2], ex = w[((size_t)k * 1024 + g) * 2 + 1];
                e0 = std::min(e0, en); e1 = std::max(e1, en); x0 = std::min(x0, ex); x1 = std::max(x1, ex);
            }
            if (k >= 5) {   // skip layer 0 (no previous stamp; embedding variant)
                acc[k % 5][0] += (double)(long long)(e0 - prev_exit); acc[k % 5][1] += (double)(e1 - e0);
                acc[k % 5][2] += (double)(x0 - e0); acc[k % 5][3] += (double)(x1 - e0); acc[k % 5][4] += 1.0;
            }
            prev_exit = x1;
        }
        fprintf(stderr, "wall-clock timeline per kernel (us, mean over layers 1..): previous kernel's last exit -> first entry | entry spread | first exit | last exit (from first entry)\n");
        double tot = 0.0;
        for (int j = 0; j < 5; j++) {
            fprintf(stderr, "   %s  gap %.2f | entries within %.2f | first exit %.2f | last exit %.2f\n", kn[j], acc[j][0] / acc[j][4] * 0.01,
                    acc[j][1] / acc[j][4] * 0.01, acc[j][2] / acc[j][4] * 0.01, acc[j][3] / acc[j][4] * 0.01);
            tot += (acc[j][0] + acc[j][3]) / acc[j][4] * 0.01;
        }
        fprintf(stderr, "   one layer = %.2f us\n", tot);
    }
    if ((ctx->opt.dbg & 32) && ctx->tstamp && fused_decode_ok(ctx, bucket_tmax(ctx, b))) {
        // per-segment shader-clock stamps, last layer, workgroup 0 / thread 0 (build with EXTRA=-DBIOGPT_HIP_PROFILE_HOOKS)
        unsigned long long h[80];
        HIP_TRY(-2, hipMemcpy(h, ctx->tstamp, sizeof h, hipMemcpyDeviceToHost));
        struct Seg { const char *kernel; int base, n; const char *names[5]; };
        const Seg segs[5] = {
            {"dec_qkv_kernel", 0, 3, {"entry -> loads issued / token embedded", "-> LayerNorm + Q8 in LDS", "-> rows finished, q / KV stored", "", ""}},
            {"dec_attn_kernel", 16, 4, {"entry -> loads issued", "-> scores + max", "-> exp table, sum", "-> PV, Q8, stored", ""}},
            {"dec_oproj_kernel", 32, 3, {"entry -> loads issued", "-> block terms in LDS", "-> in-order sum + store", "", ""}},
            {"dec_fc1_kernel", 48, 4, {"entry -> loads issued", "-> LayerNorm + Q8 in LDS", "-> rows finished, GELU", "-> Q8 block stored", ""}},
            {"dec_fc2_kernel", 64, 3, {"entry -> loads issued", "-> block terms in LDS", "-> in-order sum + store", "", ""}},
        };
        for (const Seg &sg : segs) {
            fprintf(stderr, "%s segments (shader cycles, workgroup 0 / wave 0):\n", sg.kernel);
            for (int k = 0; k < sg.n; k++) fprintf(stderr, "   %-42s %7lld\n", sg.names[k], (long long)(h[sg.base + k + 1] - h[sg.base + k]));
            if (sg.base == 0 || sg.base == 48) {   // inside the shared LayerNorm + Q8
                const char *ln[7] = {"loads issued -> column arrived", "-> wave sum 1 stored", "-> barrier 1", "-> mean, wave sum 2 stored", "-> barrier 2", "-> normalised value", "-> Q8 written"};
                const unsigned long long t0 = h[sg.base + 1];
                unsigned long long prev = t0;
                for (int k = 0; k < 7; k++) { fprintf(stderr, "      %-39s %7lld\n", ln[k], (long long)(h[sg.base + 8 + k] - prev)); prev = h[sg.base + 8 + k]; }
            }
        }
    } else if ((ctx->opt.dbg & 32) && ctx->tstamp) {
        unsigned long long h[16 * 8];
        HIP_TRY(-2, hipMemcpy(h, ctx->tstamp, sizeof h, hipMemcpyDeviceToHost));
        fprintf(stderr, "attention timeline (block 0, last layer; cycles since wave 0 entry):\n");
        for (int w = 0; w < 16; w += 5) {
            fprintf(stderr, "  wave %2d:", w);
            for (int k = 0; k < 8; k++) fprintf(stderr, " %7lld", (long long)(h[w * 8 + k] - h[0]));
            fprintf(stderr, "\n");
        }
    }
    return 0;
}

// arg-max with the lowest index winning ties (what std::max_element returns), eight independent running maxima so that the compiler can keep them in
// one vector register: ~4 us for 42 k logits against ~20 us for the scalar loop
static int32_t argmax_first(const float *v, size_t n) {
    float best[8]; int32_t at[8];
    for (int j = 0; j < 8; j++) { best[j] = -INFINITY; at[j] = 0x7fffffff; }
    size_t i = 0;
    for (; i + 8 <= n; i += 8)
        for (int j = 0; j < 8; j++)
            if (v[i + j] > best[j]) { best[j] = v[i + j]; at[j] = (int32_t)(i + j); }
    for (; i < n; i++)
        if (v[i] > best[i & 7] ) { best[i & 7] = v[i]; at[i & 7] = (int32_t)i; }
    float b = -INFINITY; int32_t a = 0x7fffffff;
    for (int j = 0; j < 8; j++)
        if (at[j] != 0x7fffffff && (best[j] > b || (best[j] == b && at[j] < a))) { b = best[j]; a = at[j]; }
    return a == 0x7fffffff ? 0 : a;
}

// The reference's host loop (main.cpp:91-151, greedy) as a C++ caller would run it on this library -- one eval call per
// token, the sampler on the host -- timed without any scripting-language overhead: mode 0 = biogpt_hip_eval (the whole
// logits row crosses PCIe, host arg-max), mode 1 = biogpt_hip_eval_topk with k = 40 (the CLI's top_k; 512 bytes cross).
int biogpt_hip_bench_api_loop(biogpt_hip_ctx *ctx, const int32_t *prompt, int32_t n_prompt, int32_t n_predict, int32_t mode, int32_t *out_ids,
                              double *seconds_out) {
    clear_error();
    if (!ctx || !prompt || n_prompt < 1 || n_predict < 1 || mode < 0 || mode > 4) BG_FAIL(-1, "bad argument");
    if (!check_eval_args(ctx, prompt, n_prompt, 0)) return -1;
    n_predict = std::min(n_predict, ctx->hp.n_positions - n_prompt);
    const size_t V = (size_t)ctx->hp.n_vocab;
    std::vector<float> logits(mode == 0 ? V : 64);
    int32_t ids[64];
    const auto t0 = std::chrono::steady_clock::now();
    int32_t tok = 0;
    int n_past = 0;
    for (int k = 0; k < n_predict; k++) {
        const int32_t *in = (k == 0) ? prompt : &tok;
        const int n_in = (k == 0) ? n_prompt : 1;
        if (mode == 0) {
            if (biogpt_hip_eval(ctx, in, n_in, n_past, logits.data()) != 0) return -2;
            tok = (int32_t)(std::max_element(logits.begin(), logits.end()) - logits.begin());
        } else if (mode == 3 || mode == 4) {   // the row read in place (pinned host memory the launch wrote), arg-max over 8 interleaved lanes; mode 4 (diagnostic): no arg-max, token fixed
            const float *row = nullptr;
            if (biogpt_hip_eval_inplace(ctx, in, n_in, n_past, &row) != 0) return -2;
            tok = mode == 3 ? argmax_first(row, V) : 2;
        } else if (mode == 1) {
            if (biogpt_hip_eval_topk(ctx, in, n_in, n_past, 40, logits.data(), ids) < 0) return -2;
            tok = ids[0];
        } else {   // mode 2 (diagnostic): the eval and a stream synchronise only -- no output leaves the device; token fixed
            if (biogpt_hip_eval_device(ctx, in, n_in, n_past) != 0) return -2;
            if (!wait_stream(ctx)) return -2;
            tok = 2;
        }
        n_past += n_in;
        if (out_ids) out_ids[k] = tok;
    }
    if (seconds_out) *seconds_out = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return n_predict;
}
