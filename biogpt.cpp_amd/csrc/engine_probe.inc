// Kernels reached without a model (tests of the kernels themselves, tools): rows held in host memory go to scratch device memory, the kernel runs as a call
// launches it, the results come back.  Part of engine.hip's translation unit.  Each entry reads: checks, layout, upload, launch, read back.

// ---- what the probes share --------------------------------------------------------------------------------------------------------------
// A probe's scratch image: the parts of one device buffer, each named once, in the order they lie in (ByteLayout: every part at a multiple of 16 bytes).
//   in(src, bytes)    the caller's rows; a null src or no bytes gives an empty part.  own(vector): a host image the probe built itself, kept until the upload
//   fill(bytes, b)    a part of bytes b (0: zeroed)
//   out(bytes, init)  an output: everything from the first output to the end of the buffer is preset to 0xff bytes -- guard rows, padding and whatever lies
//                     behind -- so what a kernel does not write reads as NaN / -1; init: what the launch finds there instead
// A part that is both (the K / V slots of a QKV stage) is an `in` that is read back.  upload() allocates, presets and copies, in that order; at() and read()
// serve afterwards.  A size is stated where the part is named and nowhere else.
extern "C++" {
struct ProbePart { size_t off = 0, bytes = 0; };
struct ProbeImage {
    ByteLayout l;
    DeviceBytes d;
    struct Fill { ProbePart p; const void *src; int byte; };
    std::vector<Fill> fills;
    std::vector<std::shared_ptr<void>> held;
    size_t first_out = ~(size_t)0;
    ProbePart part(size_t bytes, const void *src, int byte) {
        const ProbePart p{l.part(bytes), bytes};
        if (bytes) fills.push_back(Fill{p, src, byte});
        return p;
    }
    ProbePart in(const void *src, size_t bytes) { return part(src ? bytes : 0, src, 0); }
    template <class T> ProbePart own(std::vector<T> v) {
        auto h = std::make_shared<std::vector<T>>(std::move(v));
        held.push_back(h);
        return in(h->data(), h->size() * sizeof(T));
    }
    ProbePart fill(size_t bytes, int byte = 0) { return part(bytes, nullptr, byte); }
    ProbePart out(size_t bytes, const void *init = nullptr) {
        first_out = std::min(first_out, l.bytes());
        return init ? in(init, bytes) : ProbePart{l.part(bytes), bytes};
    }
    bool upload() {
        if (!d.alloc(l.bytes())) return false;
        if (first_out < l.bytes()) HIP_TRY(false, hipMemset(d.p + first_out, 0xff, l.bytes() - first_out));
        for (const Fill &f : fills) {
            if (f.src) HIP_TRY(false, hipMemcpy(d.p + f.p.off, f.src, f.p.bytes, hipMemcpyHostToDevice));
            else HIP_TRY(false, hipMemset(d.p + f.p.off, f.byte, f.p.bytes));
        }
        return true;
    }
    template <class T> T *at(ProbePart p) const { return d.at<T>(p.off); }
    bool read(ProbePart p, void *dst) const { return read(p, dst, p.bytes); }
    bool read(ProbePart p, void *dst, size_t bytes) const {      // (the first `bytes` of a part)
        if (bytes) HIP_TRY(false, hipMemcpy(dst, d.p + p.off, std::min(bytes, p.bytes), hipMemcpyDeviceToHost));
        return true;
    }
    // in stream order, for what a timed launch finds restored: dst = src; the first `bytes` of a part zeroed
    hipError_t restore(ProbePart dst, ProbePart src) const { return hipMemcpyAsync(d.p + dst.off, d.p + src.off, std::min(dst.bytes, src.bytes), hipMemcpyDeviceToDevice, 0); }
    hipError_t clear(ProbePart p, size_t bytes) const { return hipMemsetAsync(d.p + p.off, 0, std::min(bytes, p.bytes), 0); }
};

static const int32_t PROBE_NO_STATE[4] = {0, 0, 0, 0};      // the context state of a launch that reads column states, or none

// a refusal under the entry's own name from a check that several entries share
#define PROBE_FAIL(func, ret, ...) do { ::bg::set_error(func, __VA_ARGS__); return ret; } while (0)

// launched [8]: the words a probe reports of its launch, zeros behind them
static void report_launch(int32_t *launched, std::initializer_list<int32_t> words) {
    if (!launched) return;
    std::fill(launched, launched + 8, 0);
    std::copy(words.begin(), words.end(), launched);
}

// The column states of a linear stage's probe (chain, wide chain, float chain), refused under the entry's name `func`.  Only QKV reads them: exactly one of
// dev_state {n_past, ..} (the context's own columns: one slot, column i at n_past + i) and seq_states [N] SeqState words (col_mode 0: column i = slot i; 1:
// slot seq_id), every column's cache row inside its slot, no two columns on one row.  between (or none): what the entry checks between the arguments and the
// walk over the columns (the chain probe's route).
static bool probe_slot_ok(const char *func, int i, int slot, int n_slots) {
    if (slot < 0 || slot >= n_slots) PROBE_FAIL(func, false, "column %d: slot %d outside [0, n_slots)", i, slot);
    return true;
}
static bool probe_one_slot(const char *func, int n_slots) {
    if (n_slots != 1) PROBE_FAIL(func, false, "the context's own columns have one slot");
    return true;
}
static bool check_probe_columns(const char *func, bool qkv, int N, const int32_t *dev_state, const int32_t *seq_states, int col_mode, int P, int n_slots,
                                const void *k_slots, const void *v_slots, const std::function<bool()> &between = nullptr) {
    static_assert(sizeof(bgk::SeqState) == 32 && sizeof(bgk::DevState) == 16, "eight words per column state, four of context state");
    const bool batch = seq_states != nullptr;
    if (!qkv) {
        if (dev_state || batch) PROBE_FAIL(func, false, "only QKV reads column states");
        return !between || between();
    }
    if ((dev_state != nullptr) == batch) PROBE_FAIL(func, false, "exactly one of dev_state and seq_states names the column states");
    if (col_mode != 0 && col_mode != 1) PROBE_FAIL(func, false, "col_mode must be 0 or 1");
    if (!batch && col_mode) PROBE_FAIL(func, false, "col_mode 1 needs seq_states");
    if (!k_slots || !v_slots) PROBE_FAIL(func, false, "k_slots or v_slots is NULL");
    if (P < 1 || P > 8192) PROBE_FAIL(func, false, "P must be in [1, 8192]");
    if (n_slots < 1 || n_slots > 1024) PROBE_FAIL(func, false, "n_slots must be in [1, 1024]");
    if (!batch && !probe_one_slot(func, n_slots)) return false;
    if (between && !between()) return false;
    const bgk::SeqState *hs = reinterpret_cast<const bgk::SeqState *>(seq_states);
    std::set<std::pair<int, int>> seen;
    for (int i = 0; i < N; i++) {
        const int pos = batch ? hs[i].n_past : dev_state[0] + i, slot = batch ? (col_mode ? hs[i].seq_id : i) : 0;
        if (pos < 0 || pos >= P) PROBE_FAIL(func, false, "column %d: position %d outside [0, P)", i, pos);
        if (!probe_slot_ok(func, i, slot, n_slots)) return false;
        if (!seen.insert({slot, pos}).second) PROBE_FAIL(func, false, "column %d: a second column writes slot %d, position %d", i, slot, pos);
    }
    return true;
}

// The rows of a block-format (or float) matrix in a probe's image: w_rows (M rows in the file's format; null: none) repacked by repack_rows into the parts
// [qs | sc | qh], and with want_tile_image the row-tiled image of the matrix cores behind them, laid out by tile_image_place (image_fill: its bytes before
// retile() -- 0 for the rows the last tile has beyond the matrix).  sc_slack: bytes of zeros behind the scales (lm_stream_kernel stages a workgroup's scales
// 16 bytes at a time: the scale array rounded up, as in the arena).  After the upload: W() the matrix, image() its image, retile() builds the image from W().
struct BlockRows {
    int32_t type = 0, M = 0, K = 0;
    ProbePart qs, sc, qh, img;
    size_t xq = 0, xs = 0;
    bgk::DevMatrix W(const ProbeImage &im) const {
        bgk::DevMatrix w{};
        w.qs = im.d.p + qs.off; w.sc = sc.bytes ? im.d.p + sc.off : nullptr; w.qh = qh.bytes ? im.at<const uint32_t>(qh) : nullptr;
        w.type = type; w.M = M; w.K = K;
        return w;
    }
    bgk::DevMatrix image(const ProbeImage &im) const {
        bgk::DevMatrix w{};
        w.qs = im.d.p + img.off + xq; w.sc = im.d.p + img.off + xs; w.qh = nullptr; w.type = type; w.M = M; w.K = K;
        return w;
    }
    hipError_t retile(const ProbeImage &im) const {
        const bgk::DevMatrix w = W(im);
        return (hipError_t)bg_mfma_retile(type, &w, sizeof(w), im.d.p + img.off + xq, im.d.p + img.off + xs, 0);
    }
};
static BlockRows upload_block_rows(ProbeImage &im, int32_t wtype, const void *w_rows, int M, int K, bool want_tile_image, size_t sc_slack = 0, int image_fill = 0) {
    BlockRows r;
    r.type = wtype; r.M = M; r.K = K;
    if (w_rows && !is_quantized(wtype)) {
        r.qs = im.in(w_rows, file_row_bytes(wtype, K) * (size_t)M);
        r.sc = im.fill(sc_slack);
    } else if (w_rows) {
        const size_t nblk = (size_t)M * ((size_t)K / QK);
        const bool q81 = wtype == T_Q4_1 || wtype == T_Q5_1, q5 = wtype == T_Q5_0 || wtype == T_Q5_1;
        std::vector<uint8_t> qs(nblk * (wtype == T_Q8_0 ? 32 : 16)), sc(nblk * (q81 ? 4 : 2) + sc_slack, 0), qh(q5 ? nblk * 4 : 0);
        repack_rows(wtype, static_cast<const uint8_t *>(w_rows), M, K, qs.data(), sc.data(), qh.data());
        r.qs = im.own(std::move(qs)); r.sc = im.own(std::move(sc)); r.qh = im.own(std::move(qh));
    }
    if (want_tile_image) {
        size_t img_b = 0;
        tile_image_place(wtype, M, K, img_b, r.xq, r.xs);
        r.img = im.fill(img_b, image_fill);
    }
    return r;
}

// The parts of a linear stage's probe behind its inputs, in the order all three lay them out -- [bias | resid | context state | column states | GELU table |
// K slots | V slots] -- and the MatvecParams fields that follow from them: the common ones, then the QKV branch (q_out / kcache / vcache / q_scale, and with
// column states seq / col_mode / kv_seq_stride), the RESID branch (out / ldo / resid / ldr) or the plain one (out / ldo; none without an f32 output).  The
// caller names its output part(s) behind these and sets its input (aq_* or x / ldx).
struct StageParts { ProbePart bias, res, ds, st, tab, k, v; };
static StageParts stage_parts(ProbeImage &im, const float *bias, size_t bias_b, const float *resid, size_t res_b, const int32_t *dev_state, const int32_t *seq_states, int N,
                              const float *k_slots, const float *v_slots, size_t kv_b) {
    StageParts s;
    s.bias = im.in(bias, bias_b); s.res = im.in(resid, res_b);
    s.ds = im.in(dev_state ? dev_state : PROBE_NO_STATE, sizeof(bgk::DevState));
    s.st = im.in(seq_states, sizeof(bgk::SeqState) * (size_t)N);
    s.tab = im.own(gelu_table_f16());
    s.k = im.in(k_slots, kv_b); s.v = im.in(v_slots, kv_b);
    return s;
}
static bgk::MatvecParams stage_params(const ProbeImage &im, const bgk::DevMatrix &W, const StageParts &s, int D, int P, int N, bool qkv, int col_mode, ProbePart out, int ldo, int ldr) {
    bgk::MatvecParams p{};
    p.W = W;
    p.eps = 1e-5f; p.D = D; p.dk = 64; p.dk_log2 = 6; p.P = P;
    p.st = im.at<const bgk::DevState>(s.ds);
    p.gelu_tab = im.at<const uint16_t>(s.tab);
    p.N = N;
    if (s.bias.bytes) p.bias = im.at<const float>(s.bias);
    if (qkv) {
        p.q_out = im.at<float>(out); p.kcache = im.at<float>(s.k); p.vcache = im.at<float>(s.v);
        p.q_scale = 1.0f / sqrtf(64.0f);
        if (s.st.bytes) { p.seq = im.at<const bgk::SeqState>(s.st); p.col_mode = col_mode; p.kv_seq_stride = (int64_t)(D / 64) * P * 64; }
    } else if (out.bytes) {
        p.out = im.at<float>(out); p.ldo = ldo;
        if (s.res.bytes) { p.resid = im.at<const float>(s.res); p.ldr = ldr; }
    }
    return p;
}

// Two events and reps timed launches between them: before (or none) runs in front of the first event (the device-side restore of what the launch consumes),
// launch between the two, store(i, ms) takes launch i's milliseconds in the caller's unit.  Returns 0, or -2 with the HIP error of the step that failed.
struct EventPair {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    EventPair() = default;
    EventPair(const EventPair &) = delete;
    bool create() { HIP_TRY(false, hipEventCreate(&e0)); HIP_TRY(false, hipEventCreate(&e1)); return true; }
    ~EventPair() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
};
constexpr int PROBE_MAX_REPS = 10000;      // the timed entries take reps in [1, PROBE_MAX_REPS]; their untimed forms pass 0
static int time_launches(int reps, const std::function<hipError_t()> &before, const std::function<hipError_t()> &launch, const std::function<void(int, float)> &store) {
    EventPair ev;
    if (reps < 1) return 0;
    if (!ev.create()) return -2;
    for (int i = 0; i < reps; i++) {
        float ms = 0.0f;
        hipError_t e = before ? before() : hipSuccess;
        if (e == hipSuccess) e = hipEventRecord(ev.e0, 0);
        if (e == hipSuccess) e = launch();
        if (e == hipSuccess) e = hipEventRecord(ev.e1, 0);
        if (e == hipSuccess) e = hipEventSynchronize(ev.e1);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, ev.e0, ev.e1);
        store(i, ms);
        if (e != hipSuccess) BG_FAIL(-2, "a timed launch failed: %s", hipGetErrorString(e));
    }
    return 0;
}
}  // extern "C++"

// contrast_rank_kernel + contrast_pick over rows held in host memory (tests of the kernels themselves): k candidate rows against T context rows, no model
int biogpt_hip_contrast_rank_device(int device, const float *cand, const float *ctx_rows, int32_t k, int32_t T, int32_t d, const float *probs, float alpha,
                                    float *pen_out, float *score_out, int32_t *winner_out) {
    clear_error();
    if (!cand || !ctx_rows || !probs || !pen_out || !score_out || !winner_out) BG_FAIL(-1, "null argument");
    if (k < 1 || k > bgk::CT_MAX_K) BG_FAIL(-1, "k must be in [1, %d]", bgk::CT_MAX_K);
    if (T < 1 || T > (1 << 20)) BG_FAIL(-1, "T must be in [1, %d]", 1 << 20);
    if (d < 4 || d > bgk::CT_MAX_D || d % 4) BG_FAIL(-1, "d must be a multiple of 4 in [4, %d]", bgk::CT_MAX_D);
    if (!(alpha >= 0.0f && alpha <= 1.0f)) BG_FAIL(-1, "alpha must be in [0, 1]");
    HIP_TRY(-2, hipSetDevice(device));
    const int n_slabs = (T + bgk::CT_SLAB - 1) / bgk::CT_SLAB;
    bgk::ContrastGroup hg{};
    hg.len = T;
    ProbeImage im;      // [context rows | candidate rows | norms | slab maxima | probabilities | group | out]
    const ProbePart o_h = im.in(ctx_rows, (size_t)T * d * 4), o_c = im.in(cand, (size_t)k * d * 4), o_n = im.fill((size_t)T * 8), o_s = im.fill((size_t)n_slabs * bgk::CT_MAX_K * 4);
    const ProbePart o_p = im.in(probs, (size_t)k * 4), o_g = im.in(&hg, sizeof(hg)), o_o = im.out((2 * bgk::CT_MAX_K + 1) * 4);
    if (!im.upload()) return -2;
    const float *H = im.at<float>(o_h);
    double *Hn = im.at<double>(o_n);
    float *slab_max = im.at<float>(o_s);
    const bgk::ContrastGroup *grp = im.at<bgk::ContrastGroup>(o_g);
    size_t rank_lds;
    if (!contrast_rank_lds(nullptr, k, d, &rank_lds)) return -2;
    hipLaunchKernelGGL(bgk::contrast_norms_kernel, dim3(n_slabs, 1), dim3(bgk::CT_THREADS), 0, 0, H, Hn, grp, d, T);
    hipLaunchKernelGGL(bgk::contrast_rank_kernel, dim3(n_slabs, 1), dim3(bgk::CT_THREADS), rank_lds, 0, im.at<const float>(o_c), H, Hn, grp, k, d, T, slab_max);
    hipLaunchKernelGGL(bgk::contrast_pick_kernel, dim3(1), dim3(bgk::CT_THREADS), 0, 0, slab_max, grp, k, im.at<const float>(o_p), alpha, im.at<float>(o_o));
    HIP_TRY(-2, hipGetLastError());
    HIP_TRY(-2, hipDeviceSynchronize());
    float out[2 * bgk::CT_MAX_K + 1];
    if (!im.read(o_o, out, (size_t)(2 * k + 1) * 4)) return -2;
    std::memcpy(pen_out, out, (size_t)k * 4);
    std::memcpy(score_out, out + k, (size_t)k * 4);
    std::memcpy(winner_out, out + 2 * k, 4);
    return 0;
}

// rules_rows_kernel over rows held in host memory (tests of the kernel itself): row r's history is hist_lens[r] tokens of `hist` (the histories
// concatenated), the first prompt_lens[r] of them its prompt -- laid out for the kernel as a call lays them out (prompt words, generated words)
int biogpt_hip_rules_rows_device(int device, int32_t mode, const float *rows, int32_t n_rows, int32_t n_vocab, const int32_t *hist, const int32_t *hist_lens,
                                 const int32_t *prompt_lens, int32_t eos_id, const biogpt_hip_gen_rules *rules, float *rows_out) {
    clear_error();
    if (!rows || !hist || !hist_lens || !prompt_lens || !rules || !rows_out) BG_FAIL(-1, "null argument");
    if (mode != 0 && mode != 1) BG_FAIL(-1, "mode must be 0 (logits) or 1 (log-probabilities)");
    if (n_rows < 1 || n_rows > 4096 || n_vocab < 1) BG_FAIL(-1, "n_rows must be in [1, 4096], n_vocab >= 1");
    if (eos_id < -1 || eos_id >= n_vocab) BG_FAIL(-1, "eos_id %d out of range: must be in [0, %d), or -1 for none", eos_id, n_vocab);
    if (!check_rules(rules, n_vocab, -1)) return -1;
    size_t total = 0, n_pr = 0;
    int gs = 1;
    for (int r = 0; r < n_rows; r++) {
        if (hist_lens[r] < 0 || hist_lens[r] > (1 << 20) || prompt_lens[r] < 0 || prompt_lens[r] > hist_lens[r])
            BG_FAIL(-1, "hist_lens / prompt_lens of row %d: need 0 <= prompt_lens <= hist_lens <= %d", r, 1 << 20);
        for (int i = 0; i < hist_lens[r]; i++)
            if (hist[total + i] < 0 || hist[total + i] >= n_vocab) BG_FAIL(-1, "hist: token %d of row %d out of range", i, r);
        total += (size_t)hist_lens[r]; n_pr += (size_t)prompt_lens[r];
        gs = std::max(gs, hist_lens[r] - prompt_lens[r]);
    }
    HIP_TRY(-2, hipSetDevice(device));
    ByteLayout sl;      // the side image: [ctl | rows | prompt words | column states | generated words]
    const size_t o_ct = sl.part(sizeof(bgk::RulesCtl)), o_rr = sl.part(sizeof(bgk::RulesRow) * (size_t)n_rows), o_tk = sl.part(n_pr * 4);
    const size_t o_st = sl.part(sizeof(bgk::SeqState) * (size_t)n_rows), o_gn = sl.part((size_t)n_rows * gs * 4);
    std::vector<uint8_t> h(sl.bytes(), 0);
    *reinterpret_cast<bgk::RulesCtl *>(h.data() + o_ct) = rules_ctl_of(rules, mode, eos_id);
    bgk::RulesRow *rr = reinterpret_cast<bgk::RulesRow *>(h.data() + o_rr);
    int32_t *tk = reinterpret_cast<int32_t *>(h.data() + o_tk), *gn = reinterpret_cast<int32_t *>(h.data() + o_gn);
    bgk::SeqState *st = reinterpret_cast<bgk::SeqState *>(h.data() + o_st);
    size_t at = 0, po = 0;
    for (int r = 0; r < n_rows; r++) {
        const int np = prompt_lens[r], ng = hist_lens[r] - np;
        rr[r] = bgk::RulesRow{(int32_t)po, np};
        std::memcpy(tk + po, hist + at, (size_t)np * 4);
        std::memcpy(gn + (size_t)r * gs, hist + at + np, (size_t)ng * 4);
        st[r].n_gen = ng;
        at += (size_t)hist_lens[r]; po += (size_t)np;
    }
    ProbeImage im;      // [rows | side image]
    const ProbePart o_lg = im.in(rows, (size_t)n_rows * n_vocab * 4), o_side = im.in(h.data(), h.size());
    if (!im.upload()) return -2;
    const uint8_t *side = im.at<const uint8_t>(o_side);
    hipLaunchKernelGGL(bgk::rules_rows_kernel, dim3(n_rows), dim3(bgk::LP_THREADS), (size_t)((n_vocab + 31) / 32) * 4, 0, im.at<float>(o_lg), n_vocab, n_vocab,
                       reinterpret_cast<const bgk::RulesCtl *>(side + o_ct), reinterpret_cast<const bgk::RulesRow *>(side + o_rr), reinterpret_cast<const int32_t *>(side + o_tk),
                       reinterpret_cast<const bgk::SeqState *>(side + o_st), reinterpret_cast<const int32_t *>(side + o_gn), gs, nullptr, 0);
    HIP_TRY(-2, hipGetLastError());
    HIP_TRY(-2, hipDeviceSynchronize());
    return im.read(o_lg, rows_out) ? 0 : -2;
}

// trie_rows_kernel over rows held in host memory (tests of the kernel itself, tools): row r's generated tokens are hist_lens[r] tokens of `hist` (the
// histories concatenated), laid out for the kernel as a call lays them out.  reps > 0 (biogpt_hip_trie_rows_bench): the launch is then repeated on the
// same rows, restored by a device copy in front of each, and us_out[i] is the time between two events around launch i alone
static int trie_rows_device(int device, biogpt_hip_trie *trie, int32_t mode, const float *rows, int32_t n_rows, int32_t n_vocab, const int32_t *hist,
                            const int32_t *hist_lens, int32_t eos_id, float *rows_out, int32_t reps, float *us_out) {
    clear_error();
    if (!rows) BG_FAIL(-1, "rows is NULL");
    if (!hist || !hist_lens) BG_FAIL(-1, "hist or hist_lens is NULL");
    if (!rows_out) BG_FAIL(-1, "rows_out is NULL");
    if (mode != 0 && mode != 1) BG_FAIL(-1, "mode must be 0 (logits) or 1 (log-probabilities)");
    if (n_rows < 1 || n_rows > 4096) BG_FAIL(-1, "n_rows must be in [1, 4096]");
    if (reps < 0 || reps > PROBE_MAX_REPS || (reps > 0 && !us_out)) BG_FAIL(-1, "reps must be in [0, %d], with us_out", PROBE_MAX_REPS);
    if (!check_trie(trie, eos_id)) return -1;
    if (n_vocab != trie->n_vocab) BG_FAIL(-1, "n_vocab = %d, the trie was built for %d", n_vocab, trie->n_vocab);
    size_t total = 0;
    int gs = 1;
    for (int r = 0; r < n_rows; r++) {
        if (hist_lens[r] < 0 || hist_lens[r] > (1 << 20)) BG_FAIL(-1, "hist_lens[%d] = %d: must be in [0, %d]", r, hist_lens[r], 1 << 20);
        for (int i = 0; i < hist_lens[r]; i++)
            if (hist[total + i] < 0 || hist[total + i] >= n_vocab) BG_FAIL(-1, "hist: token %d of row %d out of range", i, r);
        total += (size_t)hist_lens[r];
        gs = std::max(gs, hist_lens[r]);
    }
    HIP_TRY(-2, hipSetDevice(device));
    const size_t lg_b = (size_t)n_rows * n_vocab * 4;
    ByteLayout sl;      // the side image: [ctl | column states | generated words]
    const size_t o_ct = sl.part(sizeof(bgk::TrieCtl)), o_st = sl.part(sizeof(bgk::SeqState) * (size_t)n_rows), o_gn = sl.part((size_t)n_rows * gs * 4);
    std::vector<uint8_t> h(sl.bytes(), 0);
    bgk::TrieCtl *hc = reinterpret_cast<bgk::TrieCtl *>(h.data() + o_ct);
    if (!trie_device(trie, device, hc)) return -2;
    hc->eos_id = eos_id; hc->mode = mode;
    bgk::SeqState *st = reinterpret_cast<bgk::SeqState *>(h.data() + o_st);
    int32_t *gn = reinterpret_cast<int32_t *>(h.data() + o_gn);
    size_t at = 0;
    for (int r = 0; r < n_rows; r++) {
        std::memcpy(gn + (size_t)r * gs, hist + at, (size_t)hist_lens[r] * 4);
        st[r].n_gen = hist_lens[r];
        at += (size_t)hist_lens[r];
    }
    ProbeImage im;      // [rows | side image | the rows again, with reps]
    const ProbePart o_lg = im.in(rows, lg_b), o_side = im.in(h.data(), h.size()), o_keep = im.in(reps > 0 ? rows : nullptr, lg_b);
    if (!im.upload()) return -2;
    const uint8_t *side = im.at<const uint8_t>(o_side);
    auto launch = [&]() -> hipError_t {
        hipLaunchKernelGGL(bgk::trie_rows_kernel, dim3(n_rows), dim3(bgk::LP_THREADS), (size_t)((n_vocab + 31) / 32) * 4, 0, im.at<float>(o_lg), n_vocab, n_vocab,
                           reinterpret_cast<const bgk::TrieCtl *>(side + o_ct), reinterpret_cast<const bgk::SeqState *>(side + o_st),
                           reinterpret_cast<const int32_t *>(side + o_gn), gs, nullptr, 0);
        return hipGetLastError();
    };
    HIP_TRY(-2, launch());
    HIP_TRY(-2, hipDeviceSynchronize());
    if (!im.read(o_lg, rows_out)) return -2;
    return time_launches(reps, [&] { return im.restore(o_lg, o_keep); }, launch, [&](int i, float ms) { us_out[i] = ms * 1e3f; });
}
int biogpt_hip_trie_rows_device(int device, biogpt_hip_trie *trie, int32_t mode, const float *rows, int32_t n_rows, int32_t n_vocab, const int32_t *hist,
                                const int32_t *hist_lens, int32_t eos_id, float *rows_out) {
    return trie_rows_device(device, trie, mode, rows, n_rows, n_vocab, hist, hist_lens, eos_id, rows_out, 0, nullptr);
}
int biogpt_hip_trie_rows_bench(int device, biogpt_hip_trie *trie, int32_t mode, const float *rows, int32_t n_rows, int32_t n_vocab, const int32_t *hist,
                               const int32_t *hist_lens, int32_t eos_id, float *rows_out, int32_t reps, float *us_out) {
    if (reps < 1) { clear_error(); BG_FAIL(-1, "reps must be in [1, %d]", PROBE_MAX_REPS); }
    return trie_rows_device(device, trie, mode, rows, n_rows, n_vocab, hist, hist_lens, eos_id, rows_out, reps, us_out);
}

// One stand-alone attention launch over caller-supplied inputs, through the launch helpers of enqueue_attention (one layer).  route: the AttnKernel the
// caller expects; a combination for which the engine would launch another kernel, or none, is refused before anything is allocated.  H heads of dk values
// (dk = 64 for every kernel but the generic one); q [N][H * dk]; k_slots / v_slots [n_slots][H][P][dk].  Column states: dev_state {n_past, n_gen, causal, chunk}
// (the context's own columns: one slot, visible_keys per column) or seq_states [N] SeqState words (col_mode 0: column i = slot i, T = n_past + 1; 1: slot
// seq_id, T = t_vis; the SHARED kernels and attn_prefix_kernel: the first pad[0] rows in slot pad[1]).  t_max: the pass's furthest visible key count, from
// which t_cap follows as in the engine.  q8 0: f32 rows only; 1 / 2: also their Q8_0 / Q8_1 blocks.  The outputs are returned WHOLE as they were allocated:
// rows = N rounded up to 16, plus one guard row, preset to 0xff -- out [rows][H * dk], out_q [rows][H * dk], out_d / out_s [rows][H * dk / 32] -- so a store
// beyond column N shows.  launched [8]: kernel, threads, grid x, grid y, dynamic LDS bytes, t_cap, key ranges (split), 0.
// reps > 0: the launch repeated, us_out[i] microseconds between two events around launch i alone -- a repeated stand-alone launch finds its K / V rows in cache.
// The image of an attention probe: [K slots | V slots | q | column states | the probe's own part (extra) | exp table | out | out_q | out_d | out_s], the outputs
// of rows = N rounded up to 16, plus one guard row; the AttnParams that follow from it (column states only where seq_states is given); the read-back.
struct AttnProbeParts { ProbePart k, v, q, st, extra, tab, out, oq, od, os; };
static AttnProbeParts attn_probe_parts(ProbeImage &im, int H, int dk, int N, int P, int n_slots, const float *q, const float *k_slots, const float *v_slots,
                                       const int32_t *seq_states, const void *extra, size_t extra_b) {
    const size_t D = (size_t)H * dk, rows = (size_t)((N + 15) & ~15) + 1, kv_b = (size_t)H * P * dk * 4 * (size_t)n_slots;
    AttnProbeParts o;
    o.k = im.in(k_slots, kv_b); o.v = im.in(v_slots, kv_b); o.q = im.in(q, (size_t)N * D * 4); o.st = im.in(seq_states, sizeof(bgk::SeqState) * (size_t)N);
    o.extra = im.in(extra, extra_b);
    o.tab = im.own(exp_table_f16());      // the table of the model loader
    o.out = im.out(rows * D * 4); o.oq = im.out(rows * D); o.od = im.out(rows * (D / 32) * 4); o.os = im.out(rows * (D / 32) * 4);
    return o;
}
static bgk::AttnParams attn_probe_params(const ProbeImage &im, const AttnProbeParts &o, int N, int D, int dk, int P, int t_cap, int col_mode, int64_t kv_seq_stride, int q8) {
    bgk::AttnParams a{};
    a.q = im.at<const float>(o.q); a.kcache = im.at<const float>(o.k); a.vcache = im.at<const float>(o.v); a.out = im.at<float>(o.out);
    a.exp_tab = im.at<const uint16_t>(o.tab);
    a.N = N; a.D = D; a.dk = dk; a.P = P; a.t_cap = t_cap;
    if (o.st.bytes) { a.seq = im.at<const bgk::SeqState>(o.st); a.col_mode = col_mode; a.kv_seq_stride = kv_seq_stride; }
    a.q81 = q8 == 2 ? 1 : 0;
    if (q8 > 0) { a.oq_q = im.at<int8_t>(o.oq); a.oq_d = im.at<float>(o.od); a.oq_s = im.at<uint32_t>(o.os); }
    return a;
}
static bool attn_probe_read(const ProbeImage &im, const AttnProbeParts &o, int q8, float *out, int8_t *out_q, float *out_d, uint32_t *out_s) {
    if (!im.read(o.out, out)) return false;
    return q8 <= 0 || (im.read(o.oq, out_q) && im.read(o.od, out_d) && im.read(o.os, out_s));
}
static int host_visible_keys(const int32_t *ds, int i, int N) {      // visible_keys (kernels.hip.h) on the host
    if (ds[2]) return ds[0] + i + 1;
    if (ds[3] <= 0) return ds[0] + N;
    const int end = (i / ds[3] + 1) * ds[3];
    return ds[0] + std::min(end, N);
}
static int attn_device(int device, int32_t route, int32_t H, int32_t dk, int32_t N, int32_t P, int32_t t_max, int32_t n_slots, const float *q, const float *k_slots,
                       const float *v_slots, const int32_t *dev_state, const int32_t *seq_states, int32_t col_mode, int32_t q8, float *out, int8_t *out_q, float *out_d,
                       uint32_t *out_s, int32_t *launched, int32_t reps, float *us_out) {
    if (!q || !k_slots || !v_slots || !out) BG_FAIL(-1, "q, k_slots, v_slots or out is NULL");
    const bool fast = route >= AK_FAST_1 && route < AK_PREFIX, shared = fast && route >= AK_FAST_SHARED;
    if (!fast && (route < AK_PREFIX || route > AK_GENERIC)) BG_FAIL(-1, "route %d is no attention kernel", route);
    if (H < 1 || H > 64) BG_FAIL(-1, "H must be in [1, 64]");
    if (N < 1 || N > 512) BG_FAIL(-1, "N must be in [1, 512]");
    if (P < 1 || P > 8192) BG_FAIL(-1, "P must be in [1, 8192]");
    if (n_slots < 1 || n_slots > 1024) BG_FAIL(-1, "n_slots must be in [1, 1024]");
    if (t_max < 1 || t_max > P) BG_FAIL(-1, "t_max must be in [1, P]: t_cap never exceeds the table");
    if (q8 < 0 || q8 > 2 || (q8 > 0 && (!out_q || !out_d || !out_s))) BG_FAIL(-1, "q8 must be 0, 1 or 2, with out_q, out_d and out_s");
    if (reps < 0 || reps > PROBE_MAX_REPS || (reps > 0 && !us_out)) BG_FAIL(-1, "reps must be in [0, %d], with us_out", PROBE_MAX_REPS);
    if (col_mode != 0 && col_mode != 1) BG_FAIL(-1, "col_mode must be 0 or 1");
    if ((dev_state != nullptr) == (seq_states != nullptr)) BG_FAIL(-1, "exactly one of dev_state and seq_states names the column states");
    static_assert(sizeof(bgk::SeqState) == 32, "eight words per column state");
    static_assert(sizeof(bgk::DevState) == 16, "four words of context state");
    const bool batch = seq_states != nullptr;
    // ---- what the engine would launch for this pass, and with which bounds ----
    int threads = 0;
    if (route == AK_GENERIC) {
        if (dk < 4 || dk > 256 || (dk & 3)) BG_FAIL(-1, "dk must be a multiple of 4 in [4, 256]");
        if (dk == 64 && t_max <= 1024) BG_FAIL(-1, "head size 64 up to 1024 keys never takes the generic kernel");
        if (batch) BG_FAIL(-1, "the generic kernel serves the context's own columns only (dev_state)");
        if (q8) BG_FAIL(-1, "the generic kernel writes no Q8 blocks");
        threads = attn_generic_threads(t_max);
        if (!attn_generic_ok(threads, dk, t_max)) BG_FAIL(-1, "context of %d tokens / head size %d not supported by the attention kernel (%d threads)", t_max, dk, threads);
        if (bgk::attn_smem_bytes(P, dk, threads) > 64 * 1024) BG_FAIL(-1, "a table of %d rows exceeds the generic kernel's LDS", P);
    } else {
        if (dk != 64) BG_FAIL(-1, "dk must be 64 for every kernel but the generic one");
        if (t_max > 1024) BG_FAIL(-1, "t_cap: beyond 1024 keys a pass takes the generic kernel (the reach of every other one)");
        if (P > 2048) BG_FAIL(-1, "P must be at most 2048 for every kernel but the generic one");
    }
    const bool pass_kernel = route == AK_GROUP || route == AK_TILE || route == AK_TILE_DMA;
    const int t_cap = route == AK_GENERIC ? P : pass_kernel ? attn_pass_t_cap(P, t_max) : attn_decode_t_cap(P, t_max);
    if (pass_kernel || route == AK_SPLIT) {
        if (batch) BG_FAIL(-1, "this kernel serves the context's own columns only (dev_state)");
        if (pass_kernel && (route == AK_GROUP) == attn_tile_table_ok(P)) BG_FAIL(-1, "a table of P = %d rows takes %s", P, attn_tile_table_ok(P) ? "the tile kernel (4 | P)" : "the grouped kernel (P not a multiple of 4)");
        if ((route == AK_TILE || route == AK_TILE_DMA) && (route == AK_TILE_DMA) != bgk::attn_tile_dma_ok(t_cap)) BG_FAIL(-1, "t_cap %d takes the %s form of the tile kernel", t_cap, bgk::attn_tile_dma_ok(t_cap) ? "DMA" : "plain");
    }
    if (route == AK_SPLIT) {
        if (N != 1) BG_FAIL(-1, "the split kernels serve N = 1 only");
        if (t_cap <= SPLIT_ATTN_ABOVE_KEYS) BG_FAIL(-1, "t_cap %d: the split kernels run above %d keys only", t_cap, SPLIT_ATTN_ABOVE_KEYS);
        if ((t_cap + bgk::SPLIT_KEYS - 1) / bgk::SPLIT_KEYS > bgk::SPLIT_MAX) BG_FAIL(-1, "t_cap %d: more than %d key ranges", t_cap, bgk::SPLIT_MAX);
    }
    if (route == AK_PREFIX) {
        if (!batch || col_mode != 0) BG_FAIL(-1, "attn_prefix_kernel serves decode steps only (seq_states, col_mode 0)");
        if (t_cap > bgk::PFX_MAX_KEYS || P > bgk::PFX_MAX_KEYS) BG_FAIL(-1, "P must be in [1, %d] for attn_prefix_kernel", bgk::PFX_MAX_KEYS);
    }
    if (fast) {
        if (shared && !batch) BG_FAIL(-1, "the SHARED kernels need seq_states");
        const bool slim = (route & 3) == AK_FAST_SLIM;
        if (slim && !batch) BG_FAIL(-1, "the slim launch serves decode steps of many sequences (seq_states)");
        const AttnLaunch g = attn_fast_geometry(t_cap, slim, shared, H, N);
        if (g.kernel != route) BG_FAIL(-1, "t_cap %d is outside the reach of route %d: the engine launches kernel %d there", t_cap, route, g.kernel);
    }
    // ---- every column's visible keys lie inside [1, t_cap], every slot inside the arrays ----
    const bgk::SeqState *hs = reinterpret_cast<const bgk::SeqState *>(seq_states);
    for (int i = 0; i < N; i++) {
        const int T = !batch ? host_visible_keys(dev_state, i, N) : col_mode ? hs[i].t_vis : hs[i].n_past + 1;
        if (!batch && dev_state[0] < 0) BG_FAIL(-1, "n_past %d is negative", dev_state[0]);
        if (batch && !col_mode && (hs[i].n_past < 0 || hs[i].n_past >= t_cap)) BG_FAIL(-1, "column %d: n_past %d outside [0, t_cap)", i, hs[i].n_past);
        if (T < 1 || T > t_cap || T > t_max) BG_FAIL(-1, "column %d: %d visible keys outside [1, t_cap = %d] (t_max %d)", i, T, t_cap, t_max);
        if (!batch) continue;
        const int slot = col_mode ? hs[i].seq_id : i;
        if (!probe_slot_ok(__func__, i, slot, n_slots)) return -1;
        if (shared || route == AK_PREFIX) {
            if (hs[i].pad[0] < 0 || hs[i].pad[0] > (col_mode ? T : hs[i].n_past)) BG_FAIL(-1, "column %d: %d shared rows outside [0, n_past]", i, hs[i].pad[0]);
            if (hs[i].pad[1] < 0 || hs[i].pad[1] >= n_slots) BG_FAIL(-1, "column %d: shared slot %d outside [0, n_slots)", i, hs[i].pad[1]);
            if (route == AK_PREFIX && (hs[i].pad[0] != hs[0].pad[0] || hs[i].pad[1] != hs[0].pad[1])) BG_FAIL(-1, "column %d: attn_prefix_kernel needs one shared range for all columns", i);
        }
    }
    if (!batch && !probe_one_slot(__func__, n_slots)) return -1;
    HIP_TRY(-2, hipSetDevice(device));
    const int D = H * dk;
    ProbeImage im;      // the outputs with their guard rows, and behind them the split scratch (a range past the context reads as NaN)
    const AttnProbeParts o = attn_probe_parts(im, H, dk, N, P, n_slots, q, k_slots, v_slots, seq_states, batch ? PROBE_NO_STATE : dev_state, sizeof(bgk::DevState));
    const ProbePart o_sps = im.out((size_t)H * P * 4), o_spm = im.out((size_t)H * bgk::SPLIT_MAX * 4), o_spv = im.out((size_t)H * bgk::SPLIT_MAX * 64 * 8);
    if (!im.upload()) return -2;
    bgk::AttnParams a = attn_probe_params(im, o, N, D, dk, P, t_cap, col_mode, (int64_t)H * P * dk, q8);
    a.st = im.at<const bgk::DevState>(o.extra);
    if (route == AK_SPLIT) { a.sp_scores = im.at<float>(o_sps); a.sp_max = im.at<float>(o_spm); a.sp_pv = im.at<double>(o_spv); }
    std::set<const void *> lds_done;
    AttnLaunch g{};
    auto launch = [&]() -> bool {
        if (route == AK_GENERIC) g = launch_attn_generic(a, H, N, threads, 0);
        else if (route == AK_GROUP) g = launch_attn_group(a, H, N, 0);
        else if (route == AK_TILE || route == AK_TILE_DMA) return launch_attn_tile(a, H, N, 0, lds_done, &g);
        else if (route == AK_SPLIT) return launch_attn_split(a, H, 0, &g);
        else if (route == AK_PREFIX) g = launch_attn_prefix(a, H, N, 0);
        else if (shared) g = launch_attn_fast<true>(a, (route & 3) == AK_FAST_SLIM, H, N, 0);
        else g = launch_attn_fast<false>(a, (route & 3) == AK_FAST_SLIM, H, N, 0);
        return true;
    };
    if (!launch()) return -2;
    HIP_TRY(-2, hipGetLastError());
    HIP_TRY(-2, hipDeviceSynchronize());
    report_launch(launched, {g.kernel, g.threads, g.grid_x, g.grid_y, (int32_t)g.lds, t_cap, a.n_split});
    if (!attn_probe_read(im, o, q8, out, out_q, out_d, out_s)) return -2;
    return time_launches(reps, nullptr, [&] { return launch() ? hipSuccess : hipErrorLaunchFailure; }, [&](int i, float ms) { us_out[i] = ms * 1000.0f; });
}
int biogpt_hip_attn_device(int device, int32_t route, int32_t H, int32_t dk, int32_t N, int32_t P, int32_t t_max, int32_t n_slots, const float *q, const float *k_slots,
                           const float *v_slots, const int32_t *dev_state, const int32_t *seq_states, int32_t col_mode, int32_t q8, float *out, int8_t *out_q, float *out_d,
                           uint32_t *out_s, int32_t *launched) {
    clear_error();
    return attn_device(device, route, H, dk, N, P, t_max, n_slots, q, k_slots, v_slots, dev_state, seq_states, col_mode, q8, out, out_q, out_d, out_s, launched, 0, nullptr);
}

// One decode attention launch of N columns behind a shared prefix (head size 64): k_slots / v_slots [N + 1][H][P][64], slot i column i's own, slot N the prefix's.
// which 0: attn_fast_kernel<4, false, true> as a slim launch; 1: attn_prefix_kernel<8>.  A caller of attn_device with the outputs cut to their N rows.
static int attn_prefix_device(int device, int32_t H, int32_t N, int32_t P, int32_t t_cap, const float *q, const float *k_slots, const float *v_slots,
                              const int32_t *seq_states, int32_t which, int32_t q8, float *out, int8_t *out_q, float *out_d, uint32_t *out_s, int32_t reps, float *us_out) {
    clear_error();
    if (!q || !k_slots || !v_slots || !seq_states || !out) BG_FAIL(-1, "q, k_slots, v_slots, seq_states or out is NULL");
    if (H < 1 || H > 64) BG_FAIL(-1, "H must be in [1, 64]");
    if (N < 1 || N > 512) BG_FAIL(-1, "N must be in [1, 512]");
    if (P < 1 || P > bgk::PFX_MAX_KEYS) BG_FAIL(-1, "P must be in [1, %d]", bgk::PFX_MAX_KEYS);
    if (t_cap < 1 || t_cap > P || attn_decode_t_cap(P, t_cap) != t_cap) BG_FAIL(-1, "t_cap must be in [1, P], and a multiple of 64 or P");
    if (which != 0 && which != 1) BG_FAIL(-1, "which must be 0 (attn_fast_kernel<4, false, true>) or 1 (attn_prefix_kernel<8>)");
    if (q8 < 0 || q8 > 2 || (q8 > 0 && (!out_q || !out_d || !out_s))) BG_FAIL(-1, "q8 must be 0, 1 or 2, with out_q, out_d and out_s");
    const int D = H * 64, rows = ((N + 15) & ~15) + 1;
    std::vector<float> o((size_t)rows * D), od((size_t)rows * (D / 32));
    std::vector<int8_t> oq((size_t)rows * D);
    std::vector<uint32_t> os((size_t)rows * (D / 32));
    const int rc = attn_device(device, which == 1 ? AK_PREFIX : AK_FAST_SLIM + AK_FAST_SHARED, H, 64, N, P, t_cap, N + 1, q, k_slots, v_slots, nullptr, seq_states, 0, q8, o.data(),
                               oq.data(), od.data(), os.data(), nullptr, reps, us_out);
    if (rc != 0) return rc;
    std::memcpy(out, o.data(), (size_t)N * D * 4);
    if (q8 > 0) {
        std::memcpy(out_q, oq.data(), (size_t)N * D);
        std::memcpy(out_d, od.data(), (size_t)N * (D / 32) * 4);
        std::memcpy(out_s, os.data(), (size_t)N * (D / 32) * 4);
    }
    return 0;
}
int biogpt_hip_attn_prefix_device(int device, int32_t H, int32_t N, int32_t P, int32_t t_cap, const float *q, const float *k_slots, const float *v_slots,
                                  const int32_t *seq_states, int32_t which, int32_t q8, float *out, int8_t *out_q, float *out_d, uint32_t *out_s) {
    return attn_prefix_device(device, H, N, P, t_cap, q, k_slots, v_slots, seq_states, which, q8, out, out_q, out_d, out_s, 0, nullptr);
}
int biogpt_hip_attn_prefix_bench(int device, int32_t H, int32_t N, int32_t P, int32_t t_cap, const float *q, const float *k_slots, const float *v_slots,
                                 const int32_t *seq_states, int32_t which, int32_t q8, float *out, int8_t *out_q, float *out_d, uint32_t *out_s, int32_t reps, float *us_out) {
    if (reps < 1 || reps > PROBE_MAX_REPS || !us_out) { clear_error(); BG_FAIL(-1, "reps must be in [1, %d], with us_out", PROBE_MAX_REPS); }
    return attn_prefix_device(device, H, N, P, t_cap, q, k_slots, v_slots, seq_states, which, q8, out, out_q, out_d, out_s, reps, us_out);
}

// One attn_runs_kernel<8> launch over caller-supplied inputs, through the engine's own launch helper (launch_attn_runs): N packed columns (seq_states,
// col_mode 1: slot seq_id, T = t_vis, the first pad[0] rows in slot pad[1]) in a table of P <= 1024 rows; q [N][H * 64]; k_slots / v_slots [n_slots][H][P][64];
// t_max the pass's furthest visible key count (t_cap follows as for the engine's packed passes).  runs [n_runs][4] {c0, n, R, S}, or NULL: the planner's
// (attn_runs_plan).  A caller's table is validated before anything is allocated: every column in exactly one run, runs of consecutive columns in order,
// n in [1, 8], and for every member the rows [0, R) really lie in slot S and the rows [R, T) in its own slot.  Outputs, guard rows and q8 as
// biogpt_hip_attn_device; launched [8]: kernel (16), threads, grid x, grid y, LDS bytes, t_cap, number of runs, 0.
static int attn_runs_device(int device, int32_t H, int32_t N, int32_t P, int32_t t_max, int32_t n_slots, const float *q, const float *k_slots, const float *v_slots,
                            const int32_t *seq_states, const int32_t *runs, int32_t n_runs, int32_t q8, float *out, int8_t *out_q, float *out_d, uint32_t *out_s,
                            int32_t *launched, int32_t reps, float *us_out) {
    clear_error();
    if (!q || !k_slots || !v_slots || !seq_states || !out) BG_FAIL(-1, "q, k_slots, v_slots, seq_states or out is NULL");
    if (H < 1 || H > 64) BG_FAIL(-1, "H must be in [1, 64]");
    if (N < 1 || N > 512) BG_FAIL(-1, "N must be in [1, 512]");
    if (P < 1 || P > bgk::RUNS_MAX_KEYS) BG_FAIL(-1, "P must be in [1, %d]", bgk::RUNS_MAX_KEYS);
    if (n_slots < 1 || n_slots > 1024) BG_FAIL(-1, "n_slots must be in [1, 1024]");
    if (t_max < 1 || t_max > P) BG_FAIL(-1, "t_max must be in [1, P]: t_cap never exceeds the table");
    if (q8 < 0 || q8 > 2 || (q8 > 0 && (!out_q || !out_d || !out_s))) BG_FAIL(-1, "q8 must be 0, 1 or 2, with out_q, out_d and out_s");
    if (reps < 0 || reps > PROBE_MAX_REPS || (reps > 0 && !us_out)) BG_FAIL(-1, "reps must be in [0, %d], with us_out", PROBE_MAX_REPS);
    const int t_cap = attn_decode_t_cap(P, t_max);
    const bgk::SeqState *hs = reinterpret_cast<const bgk::SeqState *>(seq_states);
    for (int i = 0; i < N; i++) {
        const int T = hs[i].t_vis;
        if (T < 1 || T > t_cap || T > t_max) BG_FAIL(-1, "column %d: %d visible keys outside [1, t_cap = %d] (t_max %d)", i, T, t_cap, t_max);
        if (!probe_slot_ok(__func__, i, hs[i].seq_id, n_slots)) return -1;
        if (hs[i].pad[0] < 0 || hs[i].pad[0] > T) BG_FAIL(-1, "column %d: %d shared rows outside [0, t_vis]", i, hs[i].pad[0]);
        if (hs[i].pad[1] < 0 || hs[i].pad[1] >= n_slots) BG_FAIL(-1, "column %d: shared slot %d outside [0, n_slots)", i, hs[i].pad[1]);
    }
    std::vector<int32_t> table(4 * (size_t)N);
    if (!runs) {
        n_runs = attn_runs_plan(hs, N, table.data());
    } else {
        if (n_runs < 1 || n_runs > N) BG_FAIL(-1, "n_runs must be in [1, N]");
        std::memcpy(table.data(), runs, 16 * (size_t)n_runs);
    }
    int next = 0;      // a caller's table and the planner's alike
    for (int r = 0; r < n_runs; r++) {
        const int c0 = table[4 * r], n = table[4 * r + 1], R = table[4 * r + 2], S = table[4 * r + 3];
        if (n < 1 || n > bgk::RUNS_MAX_COLS) BG_FAIL(-1, "run %d: n = %d outside [1, %d]", r, n, bgk::RUNS_MAX_COLS);
        if (c0 != next) BG_FAIL(-1, "run %d: starts at column %d, not at %d: every column lies in exactly one run, in order", r, c0, next);
        if (c0 + n > N) BG_FAIL(-1, "run %d: columns [%d, %d) beyond N = %d", r, c0, c0 + n, N);
        if (R < 0 || S < 0 || S >= n_slots) BG_FAIL(-1, "run %d: R = %d, S = %d outside the slots", r, R, S);
        for (int i = c0; i < c0 + n; i++) {
            const int ns = hs[i].pad[0], own = hs[i].seq_id, shr = hs[i].pad[1];
            const bool first_in_S = R <= hs[i].t_vis && (std::min(R, ns) == 0 || shr == S) && (R <= ns || own == S);
            const bool rest_own = R >= ns || shr == own || R >= hs[i].t_vis;
            if (!first_in_S || !rest_own) BG_FAIL(-1, "run %d: the first %d rows of column %d do not lie in slot %d with the others in its own", r, R, i, S);
        }
        next = c0 + n;
    }
    if (next != N) BG_FAIL(-1, "the runs cover columns [0, %d), not all %d", next, N);
    HIP_TRY(-2, hipSetDevice(device));
    const int D = H * 64;
    ProbeImage im;
    const AttnProbeParts o = attn_probe_parts(im, H, 64, N, P, n_slots, q, k_slots, v_slots, seq_states, table.data(), 16 * (size_t)n_runs);
    if (!im.upload()) return -2;
    const bgk::AttnParams a = attn_probe_params(im, o, N, D, 64, P, t_cap, 1, (int64_t)H * P * 64, q8);
    AttnLaunch g{};
    auto launch = [&]() -> hipError_t { g = launch_attn_runs(a, im.at<const int32_t>(o.extra), n_runs, H, 0); return hipSuccess; };
    (void)launch();
    HIP_TRY(-2, hipGetLastError());
    HIP_TRY(-2, hipDeviceSynchronize());
    report_launch(launched, {g.kernel, g.threads, g.grid_x, g.grid_y, (int32_t)g.lds, t_cap, n_runs});
    if (!attn_probe_read(im, o, q8, out, out_q, out_d, out_s)) return -2;
    return time_launches(reps, nullptr, launch, [&](int i, float ms) { us_out[i] = ms * 1000.0f; });
}
int biogpt_hip_attn_runs_device(int device, int32_t H, int32_t N, int32_t P, int32_t t_max, int32_t n_slots, const float *q, const float *k_slots, const float *v_slots,
                                const int32_t *seq_states, const int32_t *runs, int32_t n_runs, int32_t q8, float *out, int8_t *out_q, float *out_d, uint32_t *out_s,
                                int32_t *launched) {
    return attn_runs_device(device, H, N, P, t_max, n_slots, q, k_slots, v_slots, seq_states, runs, n_runs, q8, out, out_q, out_d, out_s, launched, 0, nullptr);
}
int biogpt_hip_attn_runs_bench(int device, int32_t H, int32_t N, int32_t P, int32_t t_max, int32_t n_slots, const float *q, const float *k_slots, const float *v_slots,
                               const int32_t *seq_states, const int32_t *runs, int32_t n_runs, int32_t q8, float *out, int8_t *out_q, float *out_d, uint32_t *out_s,
                               int32_t *launched, int32_t reps, float *us_out) {
    if (reps < 1 || reps > PROBE_MAX_REPS || !us_out) { clear_error(); BG_FAIL(-1, "reps must be in [1, %d], with us_out", PROBE_MAX_REPS); }
    return attn_runs_device(device, H, N, P, t_max, n_slots, q, k_slots, v_slots, seq_states, runs, n_runs, q8, out, out_q, out_d, out_s, launched, reps, us_out);
}

// logprob_rows_kernel over rows held in host memory (tests of the kernel itself): ldl = n_vocab, so an odd n_vocab puts rows 1, 2, 3 on the other
// 16-byte alignments
int biogpt_hip_logprob_rows_device(int device, const float *rows, int32_t n_rows, int32_t n_vocab, const int32_t *targets, float *lp_out, int32_t *argmax_out,
                                   float *logit_out) {
    clear_error();
    if (!rows) BG_FAIL(-1, "rows is NULL");
    if (!targets) BG_FAIL(-1, "targets is NULL");
    if (!lp_out || !argmax_out || !logit_out) BG_FAIL(-1, "lp_out, argmax_out or logit_out is NULL");
    if (n_rows < 1 || n_rows > 4096) BG_FAIL(-1, "n_rows must be in [1, 4096]");
    if (n_vocab < 1 || n_vocab > (1 << 20)) BG_FAIL(-1, "n_vocab must be in [1, %d]", 1 << 20);
    for (int r = 0; r < n_rows; r++)
        if (targets[r] < -1 || targets[r] >= n_vocab) BG_FAIL(-1, "targets[%d] = %d out of range: must be in [0, %d), or -1 for none", r, targets[r], n_vocab);
    HIP_TRY(-2, hipSetDevice(device));
    const size_t n = (size_t)n_rows;
    ProbeImage im;      // [rows | targets | lp, arg-max, logit: three arrays of n_rows words, one after another]
    const ProbePart o_lg = im.in(rows, n * n_vocab * 4), o_tg = im.in(targets, n * 4), o_lp = im.out(3 * n * 4);
    if (!im.upload()) return -2;
    hipLaunchKernelGGL(bgk::logprob_rows_kernel, dim3(n_rows), dim3(bgk::LP_THREADS), 0, 0, im.at<const float>(o_lg), n_vocab, n_vocab, im.at<const int32_t>(o_tg),
                       im.at<float>(o_lp), im.at<int32_t>(o_lp) + n, im.at<float>(o_lp) + 2 * n);
    HIP_TRY(-2, hipGetLastError());
    HIP_TRY(-2, hipDeviceSynchronize());
    std::vector<float> back(3 * n);
    if (!im.read(o_lp, back.data())) return -2;
    std::memcpy(lp_out, back.data(), n * 4); std::memcpy(argmax_out, back.data() + n, n * 4); std::memcpy(logit_out, back.data() + 2 * n, n * 4);
    return 0;
}

// what the beam entries below check of a row read as log-probabilities: the row kernel's precondition (the rules' argument check in a call)
static bool beam_given_rows_ok(const float *rows, size_t n_rows, int n_vocab, int K, const char *what) {
    for (size_t r = 0; r < n_rows; r++) {
        int finite = 0;
        for (int v = 0; v < n_vocab && finite < K; v++) finite += std::isfinite(rows[r * n_vocab + v]) ? 1 : 0;
        if (finite < K) BG_FAIL(false, "%s: row %zu holds fewer than 2 x n_beams = %d finite log-probabilities", what, r, K);
    }
    return true;
}

// beam_group_rows_kernel over rows held in host memory (tests of the kernel itself), through the dispatch of a call: row r is column r % n_beams of group
// r / n_beams, run_score[r] the score of the beam in it.  Every candidate is a sentinel (score NaN, col = id = -1) before the launch; with first_step a
// group's row 0 alone may write.  masked: given rows may hold fewer than 2 x n_beams finite values, as the rows of a trie step do.
static int beam_rows_device(int device, const float *rows, int32_t n_rows, int32_t n_vocab, int32_t given, int32_t n_beams, const float *run_score,
                            int32_t first_step, float *cand_score, int32_t *cand_col, int32_t *cand_id, bool masked) {
    clear_error();
    if (!rows) BG_FAIL(-1, "rows is NULL");
    if (!run_score) BG_FAIL(-1, "run_score is NULL");
    if (!cand_score || !cand_col || !cand_id) BG_FAIL(-1, "cand_score, cand_col or cand_id is NULL");
    if (given != 0 && given != 1) BG_FAIL(-1, "given must be 0 (logits) or 1 (log-probabilities)");
    if (first_step != 0 && first_step != 1) BG_FAIL(-1, "first_step must be 0 or 1");
    if (n_beams < 1 || n_beams > bgk::BEAM_MAX) BG_FAIL(-1, "n_beams must be in [1, %d]", bgk::BEAM_MAX);
    if (n_rows < 1 || n_rows > BBATCH_COLS || n_rows % n_beams) BG_FAIL(-1, "n_rows must be a multiple of n_beams in [1, %d]", BBATCH_COLS);
    if (n_vocab > (1 << 20)) BG_FAIL(-1, "n_vocab must be at most %d", 1 << 20);
    if (n_vocab < 2 * n_beams) BG_FAIL(-1, "n_vocab: a vocabulary of %d tokens holds fewer than 2 x n_beams candidates", n_vocab);
    const int B = n_beams, G = n_rows / B, K = 2 * B;
    if (given && !masked && !beam_given_rows_ok(rows, (size_t)n_rows, n_vocab, K, "rows")) return -1;
    HIP_TRY(-2, hipSetDevice(device));
    std::vector<bgk::BeamCtl> hc((size_t)G);
    for (int g = 0; g < G; g++) {
        bgk::BeamCtl &c = hc[(size_t)g];
        c = bgk::BeamCtl{};
        c.n_beams = B; c.step = first_step ? 0 : 1; c.heur_unsat = 1;
        for (int j = 0; j < B; j++) { c.run_score[j] = run_score[g * B + j]; c.col_rank[j] = j; }
    }
    ProbeImage im;      // [rows | hdr | ctl | cand]
    const ProbePart o_lg = im.in(rows, (size_t)n_rows * n_vocab * 4), o_hd = im.fill(sizeof(bgk::BeamBatchHdr)), o_ct = im.in(hc.data(), sizeof(bgk::BeamCtl) * (size_t)G),
                    o_cd = im.out(sizeof(bgk::BeamCand) * (size_t)n_rows * K);
    if (!im.upload()) return -2;
    BeamBufs b{};
    b.stream = 0;
    b.logits = im.at<const float>(o_lg); b.n_vocab = n_vocab;
    b.hdr = im.at<bgk::BeamBatchHdr>(o_hd); b.ctl = im.at<bgk::BeamCtl>(o_ct); b.cand = im.at<bgk::BeamCand>(o_cd);
    launch_beam_group_rows(b, G, B, given != 0);
    HIP_TRY(-2, hipGetLastError());
    HIP_TRY(-2, hipDeviceSynchronize());
    std::vector<bgk::BeamCand> out((size_t)n_rows * K);
    if (!im.read(o_cd, out.data())) return -2;
    for (size_t i = 0; i < out.size(); i++) { cand_score[i] = out[i].score; cand_col[i] = out[i].col; cand_id[i] = out[i].id; }
    return 0;
}

int biogpt_hip_beam_rows_device(int device, const float *rows, int32_t n_rows, int32_t n_vocab, int32_t given, int32_t n_beams, const float *run_score,
                                int32_t first_step, float *cand_score, int32_t *cand_col, int32_t *cand_id) {
    return beam_rows_device(device, rows, n_rows, n_vocab, given, n_beams, run_score, first_step, cand_score, cand_col, cand_id, false);
}
// the rows of a trie step: log-probabilities of which any number may be -inf
int biogpt_hip_beam_rows_masked_device(int device, const float *rows, int32_t n_rows, int32_t n_vocab, int32_t n_beams, const float *run_score, int32_t first_step,
                                       float *cand_score, int32_t *cand_col, int32_t *cand_id) {
    return beam_rows_device(device, rows, n_rows, n_vocab, 1, n_beams, run_score, first_step, cand_score, cand_col, cand_id, true);
}

// A whole beam search over the three beam kernels with the model replaced by a lookup (beam_table_feed_kernel, kernels_beam.hip.h), through the step
// and the read-out of biogpt_hip_generate_beam_batch: at most max_steps steps of feed + rows + select + fork, the live-group word read after each.
// Not capturable (it synchronizes every step).
int biogpt_hip_beam_table_device(int device, const float *table, int32_t n_table_rows, int32_t n_vocab, int32_t given, const int32_t *start_tokens,
                                 const int32_t *prompt_lens, int32_t n_groups, int32_t n_beams, int32_t n_predict, int32_t eos_id, float length_penalty,
                                 int32_t early_stopping, int32_t max_steps, int32_t *out_ids, int32_t *out_lens, float *out_scores, int32_t *out_counts,
                                 int32_t *col_token, int32_t *col_n_gen, int32_t *col_hist, float *col_run_score, int32_t *col_rank, int32_t *grp_done,
                                 int32_t *grp_step, float *kv_out) {
    clear_error();
    if (!table) BG_FAIL(-1, "table is NULL");
    if (!start_tokens || !prompt_lens) BG_FAIL(-1, "start_tokens or prompt_lens is NULL");
    if (!out_ids || !out_lens || !out_scores || !out_counts) BG_FAIL(-1, "out_ids, out_lens, out_scores or out_counts is NULL");
    if (!col_token || !col_n_gen || !col_hist || !col_run_score || !col_rank || !grp_done || !grp_step || !kv_out) BG_FAIL(-1, "a state output (col_*, grp_*, kv_out) is NULL");
    if (given != 0 && given != 1) BG_FAIL(-1, "given must be 0 (logits) or 1 (log-probabilities)");
    if (n_beams < 1 || n_beams > bgk::BEAM_MAX) BG_FAIL(-1, "n_beams must be in [1, %d]", bgk::BEAM_MAX);
    if (n_groups < 1 || (int64_t)n_groups * n_beams > BBATCH_COLS) BG_FAIL(-1, "n_groups x n_beams must be in [1, %d]", BBATCH_COLS);
    if (n_vocab > (1 << 20)) BG_FAIL(-1, "n_vocab must be at most %d", 1 << 20);
    if (n_vocab < 2 * n_beams) BG_FAIL(-1, "n_vocab: a vocabulary of %d tokens holds fewer than 2 x n_beams candidates", n_vocab);
    if (n_table_rows < 1 || n_table_rows > (1 << 16)) BG_FAIL(-1, "n_table_rows must be in [1, %d]", 1 << 16);
    if (n_predict < 1 || n_predict > 1024) BG_FAIL(-1, "n_predict must be in [1, 1024]");
    if (max_steps < 1) BG_FAIL(-1, "max_steps must be >= 1");
    if (eos_id < -1 || eos_id >= n_vocab) BG_FAIL(-1, "eos_id %d out of range: must be in [0, %d), or -1 for none", eos_id, n_vocab);
    if (!std::isfinite(length_penalty)) BG_FAIL(-1, "length_penalty must be finite");
    if (early_stopping != 0 && early_stopping != 1) BG_FAIL(-1, "early_stopping must be 0 or 1");
    const int G = n_groups, B = n_beams, n_cols = G * B;
    int max_len = 0;
    for (int g = 0; g < G; g++) {
        if (prompt_lens[g] < 1 || prompt_lens[g] > 1024) BG_FAIL(-1, "prompt_lens[%d] must be in [1, 1024]", g);
        if (start_tokens[g] < 0 || start_tokens[g] >= n_vocab) BG_FAIL(-1, "start_tokens[%d] = %d out of range: must be in [0, %d)", g, start_tokens[g], n_vocab);
        max_len = std::max(max_len, prompt_lens[g]);
    }
    if (given && !beam_given_rows_ok(table, (size_t)n_table_rows, n_vocab, 2 * B, "table")) return -1;
    HIP_TRY(-2, hipSetDevice(device));
    const int P = max_len + n_predict;
    constexpr int H = bgk::TABLE_HEADS, DK = bgk::TABLE_DK;
    const size_t lg_b = (size_t)n_cols * n_vocab * 4, kv_b = (size_t)n_cols * H * P * DK * 4, gen_b = (size_t)n_cols * P * 4;
    BeamBufs b{};
    auto state_at = [&](uint8_t *base, BeamBufs *bb) {      // the state block of a call at some base (null: its size alone)
        ByteLayout l;
        beam_state_parts(l, base, (size_t)n_cols, (size_t)G, (size_t)2 * B, (size_t)P, bb);
        return l.bytes();
    };
    std::vector<bgk::BeamCtl> hc((size_t)G);
    std::vector<bgk::SeqState> hs((size_t)n_cols);
    for (int g = 0; g < G; g++) fill_column_starts(hs.data(), g, B, prompt_lens[g], start_tokens[g]);
    const std::vector<float> kv_fill(kv_b / 4, -1.0f);      // a K / V row no step has written reads -1
    ProbeImage im;      // [table | logits | K | V | the state block of a call | column states | histories]
    const ProbePart o_tb = im.in(table, (size_t)n_table_rows * n_vocab * 4), o_lg = im.fill(lg_b), o_k = im.in(kv_fill.data(), kv_b), o_v = im.in(kv_fill.data(), kv_b), o_state = im.out(state_at(nullptr, &b)), o_seq = im.out(sizeof(bgk::SeqState) * (size_t)n_cols, hs.data()),
                    o_gen = im.out(gen_b);
    if (!im.upload()) return -2;
    state_at(im.at<uint8_t>(o_state), &b);
    const ProbePart o_hdr{(size_t)(reinterpret_cast<uint8_t *>(b.hdr) - im.d.p), sizeof(bgk::BeamBatchHdr)};      // the header, wherever the block keeps it
    float *table_d = im.at<float>(o_tb), *logits_d = im.at<float>(o_lg);
    b.bk = im.at<float>(o_k); b.bv = im.at<float>(o_v); b.seq = im.at<bgk::SeqState>(o_seq); b.seq_gen = im.at<int32_t>(o_gen);
    b.stream = 0;
    b.logits = logits_d; b.n_vocab = n_vocab; b.gen_stride = P;
    b.seq_stride = (int64_t)H * P * DK; b.kv_runs = H; b.P = P; b.dk = DK;
    if (!upload_beam_start(b, G, B, prompt_lens, n_predict, eos_id, length_penalty, early_stopping)) return -2;      // the initial state of a call, onto the block's head
    bgk::BeamBatchHdr hh{};
    int n_live = G;
    for (int s = 0; s < std::min(max_steps, n_predict) && n_live > 0; s++) {
        hipLaunchKernelGGL(bgk::beam_table_feed_kernel, dim3(n_cols), dim3(256), 0, 0, b.seq, table_d, n_table_rows, n_vocab, logits_d, b.bk, b.bv, P);
        HIP_TRY(-2, hipGetLastError());
        if (!enqueue_beam_group_select(b, G, B, given != 0)) return -2;
        if (!im.read(o_hdr, &hh)) return -2;      // (synchronizes)
        n_live = hh.n_live;
    }
    std::vector<int32_t> gen((size_t)n_cols * P);
    std::vector<uint8_t> hst(o_state.bytes);
    BeamBufs hb{};      // the state block on the host
    state_at(hst.data(), &hb);
    if (!im.read(o_state, hst.data()) || !im.read(o_seq, hs.data()) || !im.read(o_gen, gen.data()) || !im.read(o_k, kv_out) || !im.read(o_v, kv_out + kv_b / 4)) return -2;
    std::memcpy(hc.data(), hb.ctl, sizeof(bgk::BeamCtl) * (size_t)G);
    const int32_t *ids = hb.pool_ids;
    for (int g = 0; g < G; g++) {
        grp_done[g] = hc[(size_t)g].done; grp_step[g] = hc[(size_t)g].step;
        for (int j = 0; j < B; j++) {
            const size_t c = (size_t)g * B + j;
            col_token[c] = hs[c].token; col_n_gen[c] = hs[c].n_gen;
            col_run_score[c] = hc[(size_t)g].run_score[j]; col_rank[c] = hc[(size_t)g].col_rank[j];
            std::memcpy(col_hist + c * n_predict, gen.data() + c * P, (size_t)n_predict * 4);
        }
    }
    if (n_live > 0) {       // stopped by max_steps: no result yet
        std::fill(out_ids, out_ids + (size_t)n_cols * n_predict, -1);
        std::fill(out_lens, out_lens + n_cols, 0);
        std::fill(out_scores, out_scores + n_cols, 0.0f);
        std::fill(out_counts, out_counts + G, 0);
        return 0;
    }
    if (!beam_read_pools(hc.data(), ids, (size_t)P, G, B, n_predict, out_ids, out_lens, out_scores, out_counts)) return -2;
    return n_predict;
}

// the sampler's tail and its generator on the host: no device, no context
int biogpt_hip_mt19937_seed(uint32_t seed, uint32_t *state625) {
    clear_error();
    if (!state625) BG_FAIL(-1, "null argument");
    bgk::mt_seed(seed, state625);
    return 0;
}
int biogpt_hip_sample_candidates_host(const float *vals, const int32_t *ids, int32_t k, double top_p, double temp, uint32_t *mt_state625, int32_t *id_out) {
    clear_error();
    if (!vals || !ids || !mt_state625 || !id_out) BG_FAIL(-1, "null argument");
    if (k < 1 || k > (1 << 20)) BG_FAIL(-1, "k must be in [1, %d]", 1 << 20);
    if (!check_temp_top_p(temp, top_p)) return -1;
    if (mt_state625[bgk::MT_N] > (uint32_t)bgk::MT_N) BG_FAIL(-1, "generator index %u out of range", mt_state625[bgk::MT_N]);
    bgk::SampleWork w;
    std::vector<double> p((size_t)k);
    *id_out = ids[bgk::sample_tail(vals, k, top_p, temp, mt_state625, p.data(), w, 0, 1, bgk::SampleNoSync())];
    return 0;
}

// sample_wide_rows_kernel (which 0) or sample_rows_kernel (which 1) over rows held in host memory: row r draws from mt_in[r] (625 words; the words of a block
// regenerated on the device are those of the host's form).  mt_out (or null): the states after one launch; n_cand_out (or null): which 0 only.  reps > 0 (biogpt_hip_sample_wide_rows_bench): the launch is then repeated from the states it
// began with, restored by a device copy in front of each, and seconds_out[i] is the time between two events around launch i alone
static int sample_wide_rows_device(int device, const float *logits, int32_t n_rows, int32_t n_vocab, const biogpt_hip_sampler *sampler, const uint32_t *mt_in,
                                   uint32_t *mt_out, int32_t *ids_out, int32_t *n_cand_out, int32_t which, int32_t reps, double *seconds_out) {
    if (!logits || !mt_in) BG_FAIL(-1, "null argument");
    if (!check_sampler(sampler, n_vocab < 1 ? -1 : n_vocab)) return -1;
    if (n_rows < 1 || n_rows > 4096 || n_vocab < 1) BG_FAIL(-1, "n_rows must be in [1, 4096], n_vocab >= 1");
    if (which != 0 && which != 1) BG_FAIL(-1, "which must be 0 (sample_wide_rows_kernel) or 1 (sample_rows_kernel)");
    if (which == 1 && !sampler_is_plain(*sampler)) BG_FAIL(-1, "sample_rows_kernel serves top_k in [1, %d] with min_p 0", bgk::SAMPLE_MAX_K);
    if (reps < 0 || reps > PROBE_MAX_REPS || (reps > 0 && !seconds_out)) BG_FAIL(-1, "reps must be in [0, %d], with seconds_out", PROBE_MAX_REPS);
    if (!check_mt_states(mt_in, n_rows)) return -1;
    HIP_TRY(-2, hipSetDevice(device));
    const size_t sq_b = sample_bufs_at(nullptr, (size_t)n_rows).bytes;
    std::vector<uint8_t> h(sq_b, 0);
    const SampleBufs hb = sample_bufs_at(h.data(), (size_t)n_rows);
    *hb.ctl = sample_ctl_of(which == 1 ? sampler->top_k : 1, -1, n_rows, which == 1 ? sampler->top_p : 1.0, which == 1 ? sampler->temp : 1.0);
    *hb.wide = sample_wide_of(*sampler);
    mt_states_in(hb.seq, mt_in, n_rows);
    ProbeImage im;      // [logits | ctl + states + sampler | column states | ids | candidate counts | ctl + states + sampler again, with reps]
    const ProbePart o_lg = im.in(logits, (size_t)n_rows * n_vocab * 4), o_sq = im.in(h.data(), sq_b), o_st = im.fill(sizeof(bgk::SeqState) * (size_t)n_rows),
                    o_id = im.fill((size_t)n_rows * 4), o_nc = im.fill((size_t)n_rows * 4), o_keep = im.in(reps > 0 ? h.data() : nullptr, sq_b);
    if (!im.upload()) return -2;
    const SampleBufs sb = sample_bufs_at(im.at<uint8_t>(o_sq), (size_t)n_rows);
    auto launch = [&]() -> hipError_t {
        if (which == 0)
            hipLaunchKernelGGL(bgk::sample_wide_rows_kernel, dim3(n_rows), dim3(bgk::WIDE_THREADS), 0, 0, im.at<const float>(o_lg), n_vocab, n_vocab, sb.wide, sb.ctl, sb.seq,
                               im.at<bgk::SeqState>(o_st), im.at<int32_t>(o_id), 1, im.at<int32_t>(o_nc));
        else
            hipLaunchKernelGGL(bgk::sample_rows_kernel, dim3(n_rows), dim3(bgk::SAMPLE_THREADS), 0, 0, im.at<const float>(o_lg), n_vocab, n_vocab, sb.ctl, sb.seq,
                               im.at<bgk::SeqState>(o_st), im.at<int32_t>(o_id), 1);
        return hipGetLastError();
    };
    HIP_TRY(-2, launch());
    HIP_TRY(-2, hipDeviceSynchronize());
    if (mt_out) {
        std::vector<uint8_t> back(sq_b);
        if (!im.read(o_sq, back.data())) return -2;
        mt_states_out(mt_out, sample_bufs_at(back.data(), (size_t)n_rows).seq, n_rows);
    }
    if (ids_out && !im.read(o_id, ids_out)) return -2;
    if (n_cand_out && !im.read(o_nc, n_cand_out)) return -2;
    auto restore = [&] { const hipError_t e = im.restore(o_sq, o_keep); return e == hipSuccess ? im.clear(o_st, o_st.bytes) : e; };
    return time_launches(reps, restore, launch, [&](int i, float ms) { seconds_out[i] = (double)ms * 1e-3; });
}
// sample_rows_kernel over rows held in host memory (tests: ties, any row width and alignment, the selection's round form, a generator block running out):
// mt_states is advanced in place
int biogpt_hip_sample_rows_device(int device, const float *logits, int32_t n_rows, int32_t n_vocab, int32_t top_k, double top_p, double temp,
                                  uint32_t *mt_states, int32_t *ids_out) {
    clear_error();
    if (!logits || !mt_states || !ids_out) BG_FAIL(-1, "null argument");
    if (n_rows < 1 || n_rows > 4096 || n_vocab < 1) BG_FAIL(-1, "n_rows must be in [1, 4096], n_vocab >= 1");
    if (!check_sample_values(top_k, top_p, temp, -1, n_vocab)) return -1;
    biogpt_hip_sampler sp{};
    sp.top_k = top_k; sp.top_p = top_p; sp.temp = temp;
    return sample_wide_rows_device(device, logits, n_rows, n_vocab, &sp, mt_states, mt_states, ids_out, nullptr, 1, 0, nullptr);
}
int biogpt_hip_sample_wide_rows_device(int device, const float *logits, int32_t n_rows, int32_t n_vocab, const biogpt_hip_sampler *sampler, uint32_t *mt_states,
                                       int32_t *ids_out, int32_t *n_cand_out) {
    clear_error();
    if (!ids_out) BG_FAIL(-1, "null argument");
    return sample_wide_rows_device(device, logits, n_rows, n_vocab, sampler, mt_states, mt_states, ids_out, n_cand_out, 0, 0, nullptr);
}
int biogpt_hip_sample_wide_rows_bench(int device, const float *logits, int32_t n_rows, int32_t n_vocab, const biogpt_hip_sampler *sampler, const uint32_t *mt_states,
                                      int32_t which, int32_t reps, double *seconds_out) {
    clear_error();
    if (reps < 1) BG_FAIL(-1, "reps must be in [1, %d]", PROBE_MAX_REPS);
    return sample_wide_rows_device(device, logits, n_rows, n_vocab, sampler, mt_states, nullptr, nullptr, nullptr, which, reps, seconds_out);
}

// genlp_greedy_rows_kernel (mode 0) or sample_lp_rows_kernel (mode 1) over rows held in host memory (tests of the kernels themselves), one entry per row
// (stride 1): ids_out [n_rows] the chosen ids, lp_out [n_rows] their log-probabilities, top_ids_out / top_lp_out [n_rows][n_top] the rows' best entries
// (null with n_top 0).  Mode 1 draws as biogpt_hip_sample_rows_device does (top_k, top_p, temp, mt_states: 625 words per row, advanced in place); mode 0
// ignores those four.  The outputs are filled with 0xff bytes before the launch.
int biogpt_hip_genlp_rows_device(int device, int32_t mode, const float *rows, int32_t n_rows, int32_t n_vocab, int32_t n_top, int32_t top_k, double top_p, double temp,
                                 uint32_t *mt_states, int32_t *ids_out, float *lp_out, int32_t *top_ids_out, float *top_lp_out) {
    clear_error();
    if (mode != 0 && mode != 1) BG_FAIL(-1, "mode must be 0 (greedy) or 1 (sampled)");
    if (!rows) BG_FAIL(-1, "rows is NULL");
    if (!ids_out) BG_FAIL(-1, "ids_out is NULL");
    if (n_rows < 1 || n_rows > 4096) BG_FAIL(-1, "n_rows must be in [1, 4096]");
    if (n_vocab < 1 || n_vocab > (1 << 20)) BG_FAIL(-1, "n_vocab must be in [1, %d]", 1 << 20);
    const biogpt_hip_gen_logprobs req{n_top, lp_out, top_ids_out, top_lp_out};
    if (!check_gen_logprobs(&req, n_vocab)) return -1;
    if (mode == 1) {
        if (!mt_states) BG_FAIL(-1, "mt_states is NULL");
        if (!check_sample_values(top_k, top_p, temp, -1, n_vocab) || !check_mt_states(mt_states, n_rows)) return -1;
    }
    HIP_TRY(-2, hipSetDevice(device));
    std::vector<uint8_t> h(sample_bufs_at(nullptr, (size_t)n_rows).bytes, 0);
    const SampleBufs hb = sample_bufs_at(h.data(), (size_t)n_rows);
    *hb.ctl = sample_ctl_of(mode == 1 ? top_k : 1, -1, n_rows, top_p, temp);
    if (mode == 1) mt_states_in(hb.seq, mt_states, n_rows);
    ProbeImage im;      // [logits | ctl + states | column states | ids | the log-probability block]
    const ProbePart o_lg = im.in(rows, (size_t)n_rows * n_vocab * 4), o_sq = im.in(h.data(), h.size()), o_st = im.fill(sizeof(bgk::SeqState) * (size_t)n_rows),
                    o_id = im.out((size_t)n_rows * 4), o_lp = im.out(genlp_bufs_at(nullptr, (size_t)n_rows, (size_t)n_top).bytes);
    if (!im.upload()) return -2;
    const SampleBufs sb = sample_bufs_at(im.at<uint8_t>(o_sq), (size_t)n_rows);
    const GenLpBufs lb = genlp_bufs_at(im.at<uint8_t>(o_lp), (size_t)n_rows, (size_t)n_top);
    if (!genlp_upload(lb, n_top, 1)) return -2;
    if (mode == 0)
        hipLaunchKernelGGL(bgk::genlp_greedy_rows_kernel, dim3(n_rows), dim3(bgk::LP_THREADS), 0, 0, im.at<const float>(o_lg), n_vocab, n_vocab, im.at<bgk::SeqState>(o_st),
                           im.at<int32_t>(o_id), 1, 1, lb.out());
    else
        hipLaunchKernelGGL(bgk::sample_lp_rows_kernel, dim3(n_rows), dim3(bgk::SAMPLE_THREADS), 0, 0, im.at<const float>(o_lg), n_vocab, n_vocab, sb.ctl, sb.seq,
                           im.at<bgk::SeqState>(o_st), im.at<int32_t>(o_id), 1, lb.out());
    HIP_TRY(-2, hipGetLastError());
    HIP_TRY(-2, hipDeviceSynchronize());
    if (!im.read(o_id, ids_out) || !genlp_read(lb, &req, n_rows, 1, nullptr)) return -2;
    if (mode == 1) {
        if (!im.read(o_sq, h.data())) return -2;
        mt_states_out(mt_states, hb.seq, n_rows);
    }
    return 0;
}

// ---- the two queue probes: one launch of a column queue's selection over rows held in host memory (tests of the kernels themselves); row r is column r ----
// The caller builds what a running queue would hold and gets it back as the launch left it: states [n_rows][8] (the SeqState words), finished [n_rows]
// (SampleSeq::finished), mt_states [n_rows][625], hdr (n_live, then fin and len of the rows, then what a mode adds); limits [n_rows] is read only.  ids_out
// [n_rows][stride] the token histories, lp_out [n_rows][stride] and top_ids_out / top_lp_out [n_rows][stride][n_top] the rows of the log-probability block (null
// with n_top 0): filled with 0xff bytes before the launch, so what the kernel does not write stays so.
struct QueueProbeArgs {
    int device; int32_t with_lp; const float *rows; int32_t n_rows, n_vocab, n_top, stride;
    uint32_t *mt_states; int32_t *states; const int32_t *limits; int32_t *finished, *hdr, *ids_out;
    float *lp_out; int32_t *top_ids_out; float *top_lp_out;
    biogpt_hip_gen_logprobs req() const { return biogpt_hip_gen_logprobs{n_top, lp_out, top_ids_out, top_lp_out}; }
};
// a mode's block at some base (null: its size alone): what both modes keep of a column, and the driver's header
struct QueueProbeCols { bgk::SampleSeq *seq; int32_t *limit; bgk::QueueHdr *hdr; size_t bytes; };
struct QueueProbeMode {
    std::function<QueueProbeCols(uint8_t *)> cols;
    std::function<void(uint8_t *, int32_t *)> fill;      // fill(block, ids): what the host image of the block holds beyond `cols`; the ids rows as the launch finds
                                                         // them ([n_rows][stride], all -1 so far)
    std::function<void(uint8_t *, float *, bgk::SeqState *, int32_t *, const GenLpBufs *)> launch;      // launch(block, rows, states, ids, lb or null), all on the device
    std::function<void(const uint8_t *)> read;           // (or none) read(block): what the mode hands back beyond the header's fin and len
};

// the pointers and sizes both probes check, in the order of their arguments; own: a mode's own pointers, which stand between rows and mt_states
static bool queue_probe_args(const QueueProbeArgs &a, std::initializer_list<std::pair<const void *, const char *>> own) {
    if (!a.rows) BG_FAIL(false, "rows is NULL");
    for (const auto &p : own)
        if (!p.first) BG_FAIL(false, "%s is NULL", p.second);
    if (!a.mt_states) BG_FAIL(false, "mt_states is NULL");
    if (!a.states) BG_FAIL(false, "states is NULL");
    if (!a.limits) BG_FAIL(false, "limits is NULL");
    if (!a.finished) BG_FAIL(false, "finished is NULL");
    if (!a.hdr) BG_FAIL(false, "hdr is NULL");
    if (!a.ids_out) BG_FAIL(false, "ids_out is NULL");
    if (a.n_rows < 1 || a.n_rows > bgk::QUEUE_COLS) BG_FAIL(false, "n_rows must be in [1, %d]", bgk::QUEUE_COLS);
    if (a.n_vocab < 1 || a.n_vocab > (1 << 20)) BG_FAIL(false, "n_vocab must be in [1, %d]", 1 << 20);
    if (a.stride < 1 || a.stride > 1024) BG_FAIL(false, "stride must be in [1, 1024]");
    const biogpt_hip_gen_logprobs req = a.req();
    return check_gen_logprobs(&req, a.n_vocab);
}

// The launch and the round trip of what both modes hold, for arguments that passed queue_probe_args and the mode's own checks.  The device block is
// [rows | the mode's block | column states | ids | the log-probability block].
static int queue_probe_run(const QueueProbeArgs &a, const QueueProbeMode &m) {
    const int n_rows = a.n_rows, n_vocab = a.n_vocab, stride = a.stride, n_top = a.n_top;
    if (!check_mt_states(a.mt_states, n_rows)) return -1;
    HIP_TRY(-2, hipSetDevice(a.device));
    static_assert(sizeof(bgk::SeqState) == 32, "eight words per column state");
    const size_t entries = (size_t)n_rows * (size_t)stride;
    std::vector<uint8_t> h(m.cols(nullptr).bytes, 0);
    const QueueProbeCols hq = m.cols(h.data());
    std::vector<int32_t> ids(entries, -1);      // (0xff bytes)
    hq.hdr->n_live = a.hdr[0];
    mt_states_in(hq.seq, a.mt_states, n_rows);
    for (int r = 0; r < n_rows; r++) {
        hq.seq[r].finished = a.finished[r];
        hq.limit[r] = a.limits[r];
        hq.hdr->fin[r] = a.hdr[1 + r]; hq.hdr->len[r] = a.hdr[1 + n_rows + r];
    }
    m.fill(h.data(), ids.data());
    ProbeImage im;
    const ProbePart o_lg = im.in(a.rows, (size_t)n_rows * n_vocab * 4), o_q = im.in(h.data(), h.size()), o_st = im.in(a.states, sizeof(bgk::SeqState) * (size_t)n_rows),
                    o_id = im.out(entries * 4, ids.data()), o_lp = im.out(genlp_bufs_at(nullptr, entries, (size_t)n_top).bytes);
    if (!im.upload()) return -2;
    const GenLpBufs lb = genlp_bufs_at(im.at<uint8_t>(o_lp), entries, (size_t)n_top);
    const biogpt_hip_gen_logprobs req = a.req();
    if (!genlp_upload(lb, n_top, stride)) return -2;
    m.launch(im.at<uint8_t>(o_q), im.at<float>(o_lg), im.at<bgk::SeqState>(o_st), im.at<int32_t>(o_id), a.with_lp ? &lb : nullptr);
    HIP_TRY(-2, hipGetLastError());
    HIP_TRY(-2, hipDeviceSynchronize());
    if (!im.read(o_id, a.ids_out) || !im.read(o_st, a.states) || !im.read(o_q, h.data()) || !genlp_read(lb, &req, n_rows, stride, nullptr)) return -2;
    a.hdr[0] = hq.hdr->n_live;
    mt_states_out(a.mt_states, hq.seq, n_rows);
    for (int r = 0; r < n_rows; r++) {
        a.finished[r] = hq.seq[r].finished;
        a.hdr[1 + r] = hq.hdr->fin[r]; a.hdr[1 + n_rows + r] = hq.hdr->len[r];
    }
    if (m.read) m.read(h.data());
    return 0;
}

// queue_rows_lp_kernel (with_lp != 0) or queue_rows_kernel; hdr [1 + 2 * n_rows]
int biogpt_hip_queue_rows_device(int device, int32_t with_lp, const float *rows, int32_t n_rows, int32_t n_vocab, int32_t n_top, int32_t stride, int32_t top_k, double top_p,
                                 double temp, int32_t eos_id, uint32_t *mt_states, int32_t *states, const int32_t *limits, int32_t *finished, int32_t *hdr,
                                 int32_t *ids_out, float *lp_out, int32_t *top_ids_out, float *top_lp_out) {
    clear_error();
    const QueueProbeArgs a{device, with_lp, rows, n_rows, n_vocab, n_top, stride, mt_states, states, limits, finished, hdr, ids_out, lp_out, top_ids_out, top_lp_out};
    if (!queue_probe_args(a, {}) || !check_sample_values(top_k, top_p, temp, eos_id, n_vocab)) return -1;
    for (int r = 0; r < n_rows; r++)
        if (states[(size_t)r * 8 + 2] < 0) BG_FAIL(-1, "n_gen is negative (row %d)", r);
    QueueProbeMode m;
    m.cols = [](uint8_t *base) { const QueueBufs b = queue_bufs_at(base); return QueueProbeCols{b.seq, b.limit, b.hdr, b.bytes}; };
    m.fill = [&](uint8_t *block, int32_t *) { *queue_bufs_at(block).ctl = sample_ctl_of(top_k, eos_id, 0, top_p, temp); };
    m.launch = [&](uint8_t *block, float *lg, bgk::SeqState *st, int32_t *ids, const GenLpBufs *lb) {
        const QueueBufs qb = queue_bufs_at(block);
        if (lb)
            hipLaunchKernelGGL(bgk::queue_rows_lp_kernel, dim3(n_rows), dim3(bgk::SAMPLE_THREADS), 0, 0, lg, n_vocab, n_vocab, qb.ctl, qb.seq, st, ids, stride, qb.limit, qb.hdr,
                               lb->out());
        else
            hipLaunchKernelGGL(bgk::queue_rows_kernel, dim3(n_rows), dim3(bgk::SAMPLE_THREADS), 0, 0, lg, n_vocab, n_vocab, qb.ctl, qb.seq, st, ids, stride, qb.limit, qb.hdr);
    };
    return queue_probe_run(a, m);
}

// queue_req_rows_kernel<SampleGenLp> (with_lp != 0) or <SamplePlain>, row r with the record of params[r].  Row r's history is hist_lens[r] tokens of `hist` (the
// histories concatenated), the first prompt_lens[r] of them its prompt -- they go to the column's hist row, there is no prefix -- and the rest its generated
// tokens, states[r]'s n_gen of them, with which its row of ids_out begins.  hdr [1 + 3 * n_rows]: the reason of the rows behind fin and len.
int biogpt_hip_queue_req_rows_device(int device, int32_t with_lp, const float *rows, int32_t n_rows, int32_t n_vocab, int32_t n_top, int32_t stride,
                                     const biogpt_hip_request_params *params, const int32_t *hist, const int32_t *hist_lens, const int32_t *prompt_lens,
                                     uint32_t *mt_states, int32_t *states, const int32_t *limits, int32_t *finished, int32_t *hdr, int32_t *ids_out, float *lp_out,
                                     int32_t *top_ids_out, float *top_lp_out) {
    clear_error();
    const QueueProbeArgs a{device, with_lp, rows, n_rows, n_vocab, n_top, stride, mt_states, states, limits, finished, hdr, ids_out, lp_out, top_ids_out, top_lp_out};
    if (!queue_probe_args(a, {{params, "params"}, {hist, "hist"}, {hist_lens, "hist_lens"}, {prompt_lens, "prompt_lens"}})) return -1;
    int hist_stride = 1;
    for (int r = 0; r < n_rows; r++) {
        if (!check_request_params(params[r], r, n_vocab, -1)) return -1;
        const int n_gen = states[(size_t)r * 8 + 2];
        if (n_gen < 0 || n_gen >= stride) BG_FAIL(-1, "n_gen must be in [0, stride) (row %d)", r);
        if (prompt_lens[r] < 0 || prompt_lens[r] > 1024) BG_FAIL(-1, "prompt_lens[%d] must be in [0, 1024]", r);
        if (hist_lens[r] != prompt_lens[r] + n_gen) BG_FAIL(-1, "hist_lens[%d] (%d) must be prompt_lens[%d] (%d) + n_gen (%d)", r, hist_lens[r], r, prompt_lens[r], n_gen);
        hist_stride = std::max(hist_stride, prompt_lens[r]);
    }
    QueueProbeMode m;
    m.cols = [&](uint8_t *base) { const QueueReqBufs b = queue_req_bufs_at(base, hist_stride); return QueueProbeCols{b.seq, b.limit, &b.hdr->q, b.bytes}; };
    m.fill = [&](uint8_t *block, int32_t *ids) {
        const QueueReqBufs hq = queue_req_bufs_at(block, hist_stride);
        size_t at = 0;
        for (int r = 0; r < n_rows; r++) {
            hq.hdr->reason[r] = hdr[1 + 2 * n_rows + r];
            hq.rec[r] = request_rec_of(params[r], 0, prompt_lens[r]);
            std::memcpy(hq.hist + (size_t)r * hist_stride, hist + at, (size_t)prompt_lens[r] * 4);
            std::memcpy(ids + (size_t)r * stride, hist + at + prompt_lens[r], (size_t)(hist_lens[r] - prompt_lens[r]) * 4);
            at += (size_t)hist_lens[r];
        }
    };
    m.launch = [&](uint8_t *block, float *lg, bgk::SeqState *st, int32_t *ids, const GenLpBufs *lb) {
        enqueue_queue_req_rows(0, n_rows, lg, n_vocab, queue_req_bufs_at(block, hist_stride), st, ids, stride, hist_stride, lb);
    };
    m.read = [&](const uint8_t *block) {
        const QueueReqBufs hq = queue_req_bufs_at(const_cast<uint8_t *>(block), hist_stride);
        for (int r = 0; r < n_rows; r++) hdr[1 + 2 * n_rows + r] = hq.hdr->reason[r];
    };
    return queue_probe_run(a, m);
}

// ---- the two kernels of a queue session alone (kernels_queue.hip.h) ----
// queue_stream_kernel over constructed columns: column c has generated n_gen[c] tokens (any value: the kernel clamps it to gen_stride), its seq_gen row is row c
// of gen_rows [C][gen_stride], and with n_top >= 0 its rows of the log-probability block are lp [C][lp_stride], top_ids / top_lp [C][lp_stride][n_top].  block_out
// [block_bytes] is what lies behind a session's header -- queue_stream_at(C, g, n_top): n_gen [C], ids [C][g], then lp [C][g] and top_ids / top_lp [C][g][n_top],
// every part at a multiple of 16 bytes -- preset to 0xff bytes, so the padding between the parts and whatever lies behind the last one come back as they were.
// Returns the bytes of the layout, < 0 on error.
int64_t biogpt_hip_queue_stream_device(int device, const int32_t *n_gen, const int32_t *gen_rows, int32_t C, int32_t gen_stride, int32_t g, int32_t n_top, int32_t lp_stride,
                                       const float *lp, const int32_t *top_ids, const float *top_lp, uint8_t *block_out, int64_t block_bytes) {
    clear_error();
    if (!n_gen) BG_FAIL(-1, "n_gen is NULL");
    if (!gen_rows) BG_FAIL(-1, "gen_rows is NULL");
    if (!block_out) BG_FAIL(-1, "block_out is NULL");
    if (C < 1 || C > bgk::QUEUE_COLS) BG_FAIL(-1, "C must be in [1, %d]", bgk::QUEUE_COLS);
    if (gen_stride < 1 || gen_stride > 4096) BG_FAIL(-1, "gen_stride must be in [1, 4096]");
    if (g < 1 || g > 64) BG_FAIL(-1, "g must be in [1, 64]");
    if (n_top < -1 || n_top > bgk::GENLP_MAX_TOP) BG_FAIL(-1, "n_top must be -1 (no log-probabilities) or in [0, %d]", bgk::GENLP_MAX_TOP);
    if (n_top >= 0 && (lp_stride < 1 || lp_stride > gen_stride)) BG_FAIL(-1, "lp_stride must be in [1, gen_stride]");
    if (n_top >= 0 && !lp) BG_FAIL(-1, "lp is NULL");
    if (n_top > 0 && (!top_ids || !top_lp)) BG_FAIL(-1, "top_ids or top_lp is NULL with n_top = %d", n_top);
    const size_t need = queue_stream_at(nullptr, C, g, n_top).bytes;
    if (block_bytes < (int64_t)need) BG_FAIL(-1, "block_bytes (%lld) is below the %zu bytes of the layout", (long long)block_bytes, need);
    HIP_TRY(-2, hipSetDevice(device));
    const size_t rows = (size_t)C * (size_t)gen_stride, entries = n_top >= 0 ? (size_t)C * (size_t)lp_stride : 0, k = n_top > 0 ? (size_t)n_top : 0;
    std::vector<bgk::SeqState> st((size_t)C);
    for (int c = 0; c < C; c++) { st[(size_t)c] = bgk::SeqState{}; st[(size_t)c].n_gen = n_gen[c]; st[(size_t)c].seq_id = c; }
    ProbeImage im;
    const ProbePart o_st = im.in(st.data(), sizeof(bgk::SeqState) * (size_t)C), o_gen = im.in(gen_rows, rows * 4), o_lp = im.in(lp, entries * 4), o_ti = im.in(top_ids, entries * k * 4),
                    o_tl = im.in(top_lp, entries * k * 4), o_out = im.out((size_t)block_bytes);
    if (!im.upload()) return -2;
    const QueueStreamBufs sb = queue_stream_at(im.at<uint8_t>(o_out), C, g, n_top);
    hipLaunchKernelGGL(bgk::queue_stream_kernel, dim3(C), dim3(bgk::QUEUE_STREAM_THREADS), 0, 0, im.at<bgk::SeqState>(o_st), im.at<int32_t>(o_gen), gen_stride, C, g, sb.out,
                       n_top >= 0 ? im.at<float>(o_lp) : nullptr, n_top >= 0 ? im.at<int32_t>(o_ti) : nullptr, n_top >= 0 ? im.at<float>(o_tl) : nullptr, lp_stride, (int)k);
    HIP_TRY(-2, hipGetLastError());
    HIP_TRY(-2, hipDeviceSynchronize());
    return im.read(o_out, block_out) ? (int64_t)need : -2;
}

// queue_cancel_kernel on the list cols [n] over QUEUE_COLS constructed columns.  In and out: finished [512] (SampleSeq::finished) and hdr [1 + 2 * 512] (n_live,
// fin[], len[]); n_gen [512] is read.  Returns 0, < 0 on error.
int biogpt_hip_queue_cancel_device(int device, const int32_t *cols, int32_t n, int32_t *finished, const int32_t *n_gen, int32_t *hdr) {
    clear_error();
    if (!cols) BG_FAIL(-1, "cols is NULL");
    if (!finished) BG_FAIL(-1, "finished is NULL");
    if (!n_gen) BG_FAIL(-1, "n_gen is NULL");
    if (!hdr) BG_FAIL(-1, "hdr is NULL");
    if (n < 1 || n > bgk::QUEUE_COLS) BG_FAIL(-1, "n must be in [1, %d]", bgk::QUEUE_COLS);
    HIP_TRY(-2, hipSetDevice(device));
    constexpr int Q = bgk::QUEUE_COLS;
    std::vector<bgk::SampleSeq> sq((size_t)Q);
    std::vector<bgk::SeqState> st((size_t)Q);
    bgk::QueueHdr h{};
    h.n_live = hdr[0];
    for (int c = 0; c < Q; c++) {
        sq[(size_t)c] = bgk::SampleSeq{}; sq[(size_t)c].finished = finished[c];
        st[(size_t)c] = bgk::SeqState{}; st[(size_t)c].n_gen = n_gen[c];
        h.fin[c] = hdr[1 + c]; h.len[c] = hdr[1 + Q + c];
    }
    ProbeImage im;
    const ProbePart o_sq = im.in(sq.data(), sizeof(bgk::SampleSeq) * Q), o_st = im.in(st.data(), sizeof(bgk::SeqState) * Q), o_h = im.in(&h, sizeof(h)), o_c = im.in(cols, (size_t)n * 4);
    if (!im.upload()) return -2;
    hipLaunchKernelGGL(bgk::queue_cancel_kernel, dim3((n + bgk::QUEUE_ADMIT_THREADS - 1) / bgk::QUEUE_ADMIT_THREADS), dim3(bgk::QUEUE_ADMIT_THREADS), 0, 0, im.at<int32_t>(o_c), n,
                       im.at<bgk::SampleSeq>(o_sq), im.at<bgk::SeqState>(o_st), im.at<bgk::QueueHdr>(o_h));
    HIP_TRY(-2, hipGetLastError());
    HIP_TRY(-2, hipDeviceSynchronize());
    if (!im.read(o_sq, sq.data()) || !im.read(o_h, &h)) return -2;
    hdr[0] = h.n_live;
    for (int c = 0; c < Q; c++) { finished[c] = sq[(size_t)c].finished; hdr[1 + c] = h.fin[c]; hdr[1 + Q + c] = h.len[c]; }
    return 0;
}

// SURVEY 8 f1 on the device: `nrows` rows of `k` f32 values (host memory) -> the file's block format of `type`, byte-identical to
// the host quantizer (biogpt_hip_quantize_file uses the host one: it has to work without a GPU)
int biogpt_hip_quantize_rows_device(int device, int32_t type, const float *src, int64_t nrows, int64_t k, uint8_t *dst) {
    clear_error();
    if (!src || !dst || nrows < 1 || k < QK || k % QK) BG_FAIL(-1, "bad argument (row length must be a multiple of %d)", QK);
    if (!is_quantized(type)) BG_FAIL(-1, "type %d is not a block-quantized format", type);
    if (!select_device(device)) return -1;
    const long long nblocks = (long long)nrows * (k / QK);
    ProbeImage im;
    const ProbePart o_src = im.in(src, (size_t)nrows * (size_t)k * 4), o_dst = im.out((size_t)nblocks * file_block_bytes(type));
    if (!im.upload()) return -2;
    hipLaunchKernelGGL(bgk::quantize_blocks_kernel, dim3((unsigned)((nblocks + 255) / 256)), dim3(256), 0, 0, im.at<float>(o_src), im.at<uint8_t>(o_dst), nblocks, (int)type,
                       (int)file_block_bytes(type));
    HIP_TRY(-2, hipGetLastError());
    return im.read(o_dst, dst) ? 0 : -2;
}

// The decode launches' LayerNorm + Q8 stage (mode 0: ln4_q8_1024, one workgroup of 512 threads per row of 1024) or their activation quantizer (mode 1:
// q8_block32, n_rows blocks of 32 values) alone, on rows held in host memory.  Outputs are preset to 0xff bytes: what the stage does not write stays so.
int biogpt_hip_ln_q8_device(int device, int32_t mode, const float *x, int32_t n_rows, const float *ln_w, const float *ln_b, int32_t wb_per_row, float eps,
                            int32_t q81, int32_t want_sum, int8_t *q_out, float *d_out, uint32_t *s_out) {
    clear_error();
    if (!x || !q_out || !d_out || !s_out) BG_FAIL(-1, "null argument");
    if (mode != 0 && mode != 1) BG_FAIL(-1, "mode must be 0 (LayerNorm + Q8 of rows of 1024) or 1 (Q8 of blocks of 32)");
    if (n_rows < 1 || n_rows > (1 << 16)) BG_FAIL(-1, "n_rows must be in [1, %d]", 1 << 16);
    if (mode == 0 && (!ln_w || !ln_b)) BG_FAIL(-1, "mode 0 needs ln_w and ln_b");
    if (mode == 0 && q81 && !want_sum) BG_FAIL(-1, "the Q8_1 form always writes its block sums");
    if (!select_device(device)) return -1;
    const size_t k = mode == 0 ? 1024 : 32, nb = k / 32, n_wb = mode == 0 ? (wb_per_row ? (size_t)n_rows : 1) : 0;
    ProbeImage dv;      // [x | gain | bias | codes | scales | sums]
    const ProbePart o_x = dv.in(x, (size_t)n_rows * k * 4), o_w = dv.in(ln_w, n_wb * 1024 * 4), o_b = dv.in(ln_b, n_wb * 1024 * 4);
    const ProbePart o_q = dv.out((size_t)n_rows * k), o_d = dv.out((size_t)n_rows * nb * 4), o_s = dv.out((size_t)n_rows * nb * 4);
    if (!dv.upload()) return -2;
    if (mode == 0) {
        const int stride = wb_per_row ? 1024 : 0;
        auto kern = q81 ? bgk::ln_q8_probe_kernel<true, true> : (want_sum ? bgk::ln_q8_probe_kernel<false, true> : bgk::ln_q8_probe_kernel<false, false>);
        hipLaunchKernelGGL(kern, dim3(n_rows), dim3(512), 0, 0, dv.at<const float>(o_x), dv.at<const float>(o_w), dv.at<const float>(o_b), stride, eps,
                           dv.at<uint32_t>(o_q), dv.at<float>(o_d), dv.at<uint32_t>(o_s));
    } else {
        hipLaunchKernelGGL(bgk::q8_block32_probe_kernel, dim3((n_rows + 1) / 2), dim3(64), 0, 0, dv.at<const float>(o_x), (int)n_rows, (int)(q81 != 0), (int)(want_sum != 0),
                           dv.at<int8_t>(o_q), dv.at<float>(o_d), dv.at<uint32_t>(o_s));
    }
    HIP_TRY(-2, hipGetLastError());
    HIP_TRY(-2, hipDeviceSynchronize());
    return dv.read(o_q, q_out) && dv.read(o_d, d_out) && dv.read(o_s, s_out) ? 0 : -2;
}

// q8_round, ln_inv_std and q8_scales (kernels_decode.hip.h) against the expressions they stand for, over all 2^32 float bit patterns in one launch.
// out[18]: per check c of bgk::Q8F_CHECKS (kernels_q8probe.hip.h lists them) out[c] patterns tested, out[6 + c] mismatches, out[12 + c] the lowest
// mismatching pattern (~0: none).
int biogpt_hip_q8_forms_device(int device, uint64_t *out) {
    clear_error();
    if (!out) BG_FAIL(-1, "null argument");
    if (!select_device(device)) return -1;
    constexpr int N = bgk::Q8F_CHECKS;
    unsigned long long h[3 * N];
    for (int i = 0; i < 3 * N; i++) h[i] = i < 2 * N ? 0ull : ~0ull;
    ProbeImage dv;
    const ProbePart o_h = dv.in(h, sizeof(h));
    if (!dv.upload()) return -2;
    hipLaunchKernelGGL(bgk::q8_forms_kernel, dim3(bgk::Q8F_BLOCKS), dim3(bgk::Q8F_THREADS), 0, 0, dv.at<unsigned long long>(o_h));
    HIP_TRY(-2, hipGetLastError());
    HIP_TRY(-2, hipDeviceSynchronize());
    if (!dv.read(o_h, h)) return -2;
    for (int i = 0; i < 3 * N; i++) out[i] = (uint64_t)h[i];
    return 0;
}


// lookup_draft_kernel over texts held in host memory (tests of the kernel itself): sequence s has the text texts[..] of text_lens[s] tokens (corpus ++ prompt ++
// its n_gen[s] generated tokens, the last one its current token at position n_past[s]).  draft_out [n_seqs][16] (-1 behind the draft), d_out [n_seqs],
// cols_out [n_seqs][1 + max_draft][4]: token, n_past, seq_id, t_vis of every packed column state, the padding columns included.
int biogpt_hip_lookup_draft_device(int device, const int32_t *texts, const int32_t *text_lens, int32_t n_seqs, const int32_t *n_gen, const int32_t *n_past,
                                   const int32_t *finished, int32_t n_predict, int32_t max_draft, int32_t max_ngram, int32_t *draft_out, int32_t *d_out,
                                   int32_t *cols_out) {
    clear_error();
    if (!texts || !text_lens) BG_FAIL(-1, "texts or text_lens is NULL");
    if (!n_gen || !n_past) BG_FAIL(-1, "n_gen or n_past is NULL");
    if (!draft_out || !d_out || !cols_out) BG_FAIL(-1, "draft_out, d_out or cols_out is NULL");
    if (n_seqs < 1) BG_FAIL(-1, "n_seqs must be >= 1");
    if (!check_lookup_shape(n_seqs, max_draft, max_ngram)) return -1;
    if (n_predict < 1 || n_predict > (1 << 16)) BG_FAIL(-1, "n_predict must be in [1, %d]", 1 << 16);
    size_t total = 0;
    for (int s = 0; s < n_seqs; s++) {
        if (text_lens[s] < 1) BG_FAIL(-1, "text_lens[%d] must be >= 1", s);
        if (n_gen[s] < 0 || n_gen[s] >= text_lens[s]) BG_FAIL(-1, "n_gen[%d] = %d must be in [0, text_lens[%d])", s, n_gen[s], s);
        if (n_past[s] < 0) BG_FAIL(-1, "n_past[%d] is negative", s);
        total += (size_t)text_lens[s];
    }
    if (total > LOOKUP_TEXT_WORDS) BG_FAIL(-1, "the texts (%zu tokens) exceed the %zu words of the text buffer", total, LOOKUP_TEXT_WORDS);
    HIP_TRY(-2, hipSetDevice(device));
    const int S = 1 + max_draft;
    const size_t sz = lookup_bufs_at(nullptr, (size_t)n_seqs, (size_t)n_seqs * S, total).bytes;
    std::vector<uint8_t> h(sz, 0);
    const LookupBufs hb = lookup_bufs_at(h.data(), (size_t)n_seqs, (size_t)n_seqs * S, total);
    hb.ctl->max_draft = max_draft; hb.ctl->max_ngram = max_ngram; hb.ctl->eos_id = -1; hb.ctl->n_predict = n_predict; hb.ctl->n_live = n_seqs;
    std::memcpy(hb.text, texts, total * 4);
    std::vector<bgk::SeqState> hs((size_t)n_seqs);
    size_t at = 0;
    for (int s = 0; s < n_seqs; s++) {
        hb.seq[s].text_off = (int32_t)at; hb.seq[s].base_len = text_lens[s] - n_gen[s]; hb.seq[s].finished = finished && finished[s] ? 1 : 0;
        at += (size_t)text_lens[s];
        hs[(size_t)s] = bgk::SeqState{};
        hs[(size_t)s].n_past = n_past[s]; hs[(size_t)s].token = texts[at - 1]; hs[(size_t)s].n_gen = n_gen[s]; hs[(size_t)s].seq_id = s;
    }
    std::memset(hb.cols, 0xff, sizeof(bgk::SeqState) * (size_t)n_seqs * S);
    ProbeImage im;      // [the step's state, with the column states as 0xff | sequence states]
    const ProbePart o_lb = im.in(h.data(), sz), o_st = im.in(hs.data(), sizeof(bgk::SeqState) * (size_t)n_seqs);
    if (!im.upload()) return -2;
    const LookupBufs lb = lookup_bufs_at(im.at<uint8_t>(o_lb), (size_t)n_seqs, (size_t)n_seqs * S, total);
    hipLaunchKernelGGL(bgk::lookup_draft_kernel, dim3(n_seqs), dim3(bgk::LK_DRAFT_THREADS), 0, 0, lb.ctl, lb.seq, lb.text, im.at<const bgk::SeqState>(o_st), lb.cols);
    HIP_TRY(-2, hipGetLastError());
    HIP_TRY(-2, hipDeviceSynchronize());
    if (!im.read(o_lb, h.data())) return -2;
    for (int s = 0; s < n_seqs; s++) {
        std::memcpy(draft_out + (size_t)s * (bgk::LK_MAX_DRAFT + 1), hb.seq[s].draft, sizeof(hb.seq[s].draft));
        d_out[s] = hb.seq[s].d;
        for (int j = 0; j < S; j++) {
            const bgk::SeqState &c = hb.cols[(size_t)s * S + j];
            int32_t *o = cols_out + ((size_t)s * S + j) * 4;
            o[0] = c.token; o[1] = c.n_past; o[2] = c.seq_id; o[3] = c.t_vis;
        }
    }
    return 0;
}

// lookup_accept_kernel over logits rows held in host memory: rows [n_seqs * (1 + max_draft)][n_vocab], sequence s at n_gen[s] tokens and position n_past[s] with
// the draft drafts[s][0 .. d[s]) (stride 16).  emit_out [n_seqs][16] the ids appended (-1 behind them), state_out [n_seqs][4] the column's token (-1: none appended),
// n_past, n_gen, finished; stats_out [n_seqs][3] passes, drafted, accepted (from zero); live_out [2] the live word (from the unfinished sequences) and the
// furthest position.
int biogpt_hip_lookup_accept_device(int device, const float *rows, int32_t n_seqs, int32_t n_vocab, int32_t max_draft, const int32_t *drafts, const int32_t *d_in,
                                    const int32_t *n_gen, const int32_t *n_past, const int32_t *finished, int32_t n_predict, int32_t eos_id, int32_t *emit_out,
                                    int32_t *state_out, int32_t *stats_out, int32_t *live_out) {
    clear_error();
    if (!rows) BG_FAIL(-1, "rows is NULL");
    if (!drafts || !d_in) BG_FAIL(-1, "drafts or d is NULL");
    if (!n_gen || !n_past) BG_FAIL(-1, "n_gen or n_past is NULL");
    if (!emit_out || !state_out || !stats_out || !live_out) BG_FAIL(-1, "emit_out, state_out, stats_out or live_out is NULL");
    if (n_seqs < 1) BG_FAIL(-1, "n_seqs must be >= 1");
    if (!check_lookup_shape(n_seqs, max_draft, 1)) return -1;
    if (n_vocab < 1 || n_vocab > (1 << 20)) BG_FAIL(-1, "n_vocab must be in [1, %d]", 1 << 20);
    if (n_predict < 1 || n_predict > (1 << 16)) BG_FAIL(-1, "n_predict must be in [1, %d]", 1 << 16);
    if (eos_id < -1 || eos_id >= n_vocab) BG_FAIL(-1, "eos_id %d out of range: must be in [0, %d), or -1 for none", eos_id, n_vocab);
    int live = 0, far = 0;
    for (int s = 0; s < n_seqs; s++) {
        if (d_in[s] < 0 || d_in[s] > max_draft) BG_FAIL(-1, "d[%d] = %d must be in [0, max_draft]", s, d_in[s]);
        if (n_gen[s] < 0 || n_gen[s] > n_predict) BG_FAIL(-1, "n_gen[%d] = %d must be in [0, n_predict]", s, n_gen[s]);
        if (n_past[s] < 0) BG_FAIL(-1, "n_past[%d] is negative", s);
        live += finished && finished[s] ? 0 : 1;
        far = std::max(far, n_past[s]);
    }
    HIP_TRY(-2, hipSetDevice(device));
    const int S = 1 + max_draft;
    const size_t words = (size_t)n_seqs * n_predict;      // a sequence's text here is its generated tokens alone
    const size_t sz = lookup_bufs_at(nullptr, (size_t)n_seqs, 0, words).bytes;
    std::vector<uint8_t> h(sz, 0);
    const LookupBufs hb = lookup_bufs_at(h.data(), (size_t)n_seqs, 0, words);
    hb.ctl->max_draft = max_draft; hb.ctl->max_ngram = 1; hb.ctl->eos_id = eos_id; hb.ctl->n_predict = n_predict; hb.ctl->n_live = live; hb.ctl->max_pos = far;
    std::vector<bgk::SeqState> hs((size_t)n_seqs);
    for (int s = 0; s < n_seqs; s++) {
        bgk::LookupSeq &q = hb.seq[s];
        q.text_off = (int32_t)((size_t)s * n_predict); q.base_len = 0; q.finished = finished && finished[s] ? 1 : 0; q.d = d_in[s];
        std::memcpy(q.draft, drafts + (size_t)s * (bgk::LK_MAX_DRAFT + 1), sizeof(q.draft));
        hs[(size_t)s] = bgk::SeqState{};
        hs[(size_t)s].n_past = n_past[s]; hs[(size_t)s].token = -1; hs[(size_t)s].n_gen = n_gen[s]; hs[(size_t)s].seq_id = s;
    }
    ProbeImage im;      // [rows | the step's state | sequence states | generated ids, 0xff]
    const ProbePart o_lg = im.in(rows, (size_t)n_seqs * S * n_vocab * 4), o_lb = im.in(h.data(), sz), o_st = im.in(hs.data(), sizeof(bgk::SeqState) * (size_t)n_seqs),
                    o_gen = im.out(words * 4);
    if (!im.upload()) return -2;
    const LookupBufs lb = lookup_bufs_at(im.at<uint8_t>(o_lb), (size_t)n_seqs, 0, words);
    hipLaunchKernelGGL(bgk::lookup_accept_kernel, dim3(n_seqs), dim3(bgk::LK_ACCEPT_THREADS), 0, 0, lb.ctl, lb.seq, lb.text, im.at<const float>(o_lg), n_vocab, n_vocab,
                       im.at<bgk::SeqState>(o_st), im.at<int32_t>(o_gen), n_predict);
    HIP_TRY(-2, hipGetLastError());
    HIP_TRY(-2, hipDeviceSynchronize());
    std::vector<int32_t> gen(words);
    if (!im.read(o_lb, h.data()) || !im.read(o_st, hs.data()) || !im.read(o_gen, gen.data())) return -2;
    for (int s = 0; s < n_seqs; s++) {
        int32_t *e = emit_out + (size_t)s * (bgk::LK_MAX_DRAFT + 1);
        std::fill(e, e + bgk::LK_MAX_DRAFT + 1, -1);
        for (int i = n_gen[s]; i < hs[(size_t)s].n_gen && i - n_gen[s] <= bgk::LK_MAX_DRAFT && i < n_predict; i++) e[i - n_gen[s]] = gen[(size_t)s * n_predict + i];
        int32_t *o = state_out + (size_t)s * 4;
        o[0] = hs[(size_t)s].token; o[1] = hs[(size_t)s].n_past; o[2] = hs[(size_t)s].n_gen; o[3] = hb.seq[s].finished;
        stats_out[3 * s] = hb.seq[s].passes; stats_out[3 * s + 1] = hb.seq[s].drafted; stats_out[3 * s + 2] = hb.seq[s].accepted;
    }
    live_out[0] = hb.ctl->n_live; live_out[1] = hb.ctl->max_pos;
    return 0;
}

// One stand-alone launch of a linear stage of the many-column chain over caller-supplied inputs, through launch_lnq / launch_chain -- the helpers of enqueue_layer and
// enqueue_final -- so the probe's launch is the engine's.  op: 0 LNQ (lnq_kernel), 1 QKV, 2 OPROJ, 3 FC1_LN (the 1-column form with LayerNorm fused), 4 FC1_Q8, 5 FC2,
// 6 LMHEAD.  route: the ChainKernel the caller expects (0 the 1-column VALU kernel, 1 the 8-column one, 2 / 3 matmul_mfma_kernel with one / two row tiles per wave); a
// route the engine would not take for (op, type, M, N, column states) is refused before anything is allocated, as is a shape that is not the site's own.  Only QKV carries
// column states, so only there can the probe tell a pass (matrix cores from 64 columns) from a decode step of many sequences (from 48); for the other ops a matrix-core
// route is accepted from 48 columns on -- what the engine launches in a decode step, though never in a pass of 48 .. 63 columns.  w_rows: M rows
// in the file's block format, repacked by repack_rows; for a matrix-core route the row-tiled image is laid out by tile_image_place and built by bg_mfma_retile.
// Outputs come back WHOLE as allocated and preset to 0xff: cols = N rounded up to 16, plus one guard column; ldo = M rounded up to 128, plus 16 guard rows.
//   LNQ            x [N][1024], ln_w, ln_b; q81 picks the Q8_1 form              -> out_q [cols][1024], out_d / out_s [cols][32]
//   QKV            aq_*, bias [3072]; dev_state, or seq_states [N][8] + col_mode -> out [cols][1024] (q), k_slots / v_slots [n_slots][16][P][64] updated in place
//   OPROJ, FC2     aq_*, bias [1024], resid [N][1024]                            -> out [cols][ldo]
//   FC1_LN         x [1][1024], ln_w, ln_b, bias [4096]                          -> out_q [cols][4096], out_d / out_s [cols][128]
//   FC1_Q8         aq_*, bias [4096]                                             -> the same
//   LMHEAD         aq_*                                                          -> out [cols][ldo]
// aq_q [N][K] int8, aq_d [N][K / 32] f32, aq_s [N][K / 32] words, as a producer leaves them (Q8_0: d rounded through f16, the integer block sum; Q8_1: d, the bits of d * sum).
// launched [8]: kernel, threads, grid x, grid y, dynamic LDS bytes, cols, ldo, 0.
enum ChainProbeOp : int { CP_LNQ = 0, CP_QKV = 1, CP_OPROJ = 2, CP_FC1_LN = 3, CP_FC1_Q8 = 4, CP_FC2 = 5, CP_LMHEAD = 6 };
extern "C" int bg_mfma_tiles(int wt, int op, int M, int N);
int biogpt_hip_chain_device(int device, int32_t op, int32_t route, int32_t wtype, int32_t M, int32_t N, const void *w_rows, const float *x, const float *ln_w,
                            const float *ln_b, int32_t q81, const int8_t *aq_q, const float *aq_d, const uint32_t *aq_s, const float *bias, const float *resid,
                            const int32_t *dev_state, const int32_t *seq_states, int32_t col_mode, int32_t P, int32_t n_slots, float *k_slots, float *v_slots,
                            float *out, int8_t *out_q, float *out_d, uint32_t *out_s, int32_t *launched) {
    clear_error();
    static_assert(sizeof(bgk::SeqState) == 32 && sizeof(bgk::DevState) == 16, "eight words per column state, four of context state");
    if (op < CP_LNQ || op > CP_LMHEAD) BG_FAIL(-1, "op %d is no stage of the chain", op);
    if (N < 1 || N > 512) BG_FAIL(-1, "N must be in [1, 512]");
    const bool lnq = op == CP_LNQ, ln_in = lnq || op == CP_FC1_LN, q8_out = lnq || op == CP_FC1_LN || op == CP_FC1_Q8, f32_out = !q8_out;
    const int K = op == CP_FC2 ? 4096 : 1024;
    // ---- the site's own shape ----
    if (lnq) {
        if (q81 != 0 && q81 != 1) BG_FAIL(-1, "q81 must be 0 (Q8_0 blocks) or 1 (Q8_1)");
        if (route != -1) BG_FAIL(-1, "LNQ has one kernel: route must be -1");
    } else {
        if (wtype != T_Q4_0 && wtype != T_Q4_1 && wtype != T_Q5_0 && wtype != T_Q5_1 && wtype != T_Q8_0) BG_FAIL(-1, "type %d is no block format", wtype);
        if (!w_rows) BG_FAIL(-1, "w_rows is NULL");
        const int want = op == CP_QKV ? 3072 : (op == CP_FC1_LN || op == CP_FC1_Q8) ? 4096 : 1024;
        if (op != CP_LMHEAD && M != want) BG_FAIL(-1, "M = %d is not the site's own shape (%d x %d)", M, want, K);
        if (op == CP_LMHEAD && (M < 1 || M > (1 << 20))) BG_FAIL(-1, "M must be in [1, %d]", 1 << 20);
        q81 = (wtype == T_Q4_1 || wtype == T_Q5_1) ? 1 : 0;
    }
    if (ln_in ? (!x || !ln_w || !ln_b) : (!aq_q || !aq_d || !aq_s)) BG_FAIL(-1, "%s", ln_in ? "x, ln_w or ln_b is NULL" : "aq_q, aq_d or aq_s is NULL");
    if (!lnq && op != CP_LMHEAD && !bias) BG_FAIL(-1, "bias is NULL");
    if ((op == CP_OPROJ || op == CP_FC2) && !resid) BG_FAIL(-1, "resid is NULL");
    if (f32_out ? !out : (!out_q || !out_d || !out_s)) BG_FAIL(-1, "%s", f32_out ? "out is NULL" : "out_q, out_d or out_s is NULL");
    const bool batch = seq_states != nullptr;
    // ---- the route the engine takes: checked between the column states' arguments and the walk over the columns ----
    const ChainOp cop = op == CP_QKV ? CHAIN_QKV_Q8 : op == CP_OPROJ ? CHAIN_OPROJ : op == CP_FC1_LN ? CHAIN_FC1 : op == CP_FC1_Q8 ? CHAIN_FC1_Q8 : op == CP_FC2 ? CHAIN_FC2 : CHAIN_LMHEAD_Q8;
    const bool mfma = route == CK_MFMA_1 || route == CK_MFMA_2;
    auto route_ok = [&]() -> bool {
        if (lnq) return true;
        if (route < CK_VALU_1 || route > CK_MFMA_2) PROBE_FAIL("biogpt_hip_chain_device", false, "route %d is no kernel of the chain", route);
        if (op == CP_FC1_LN) {
            if (route != CK_VALU_1 || N != 1) PROBE_FAIL("biogpt_hip_chain_device", false, "FC1_LN is the 1-column kernel alone: one column, route 0");
        } else if (mfma) {
            const int min_cols = (op == CP_QKV && !(batch && col_mode == 0)) ? MFMA_MIN_PASS_COLS : MFMA_MIN_DECODE_COLS;
            if (N < min_cols) PROBE_FAIL("biogpt_hip_chain_device", false, "%d columns: the matrix-core kernels run from %d columns on", N, min_cols);
            if (M % 16 != 0) PROBE_FAIL("biogpt_hip_chain_device", false, "M = %d is no whole number of 16-row tiles: such a matrix has no image and stays on the 8-column kernel", M);
            static const int site_of[7] = {-1, 0, 1, -1, 2, 3, 4};
            const int tiles = bg_mfma_tiles(wtype, site_of[op], M, N);
            if (tiles != (route == CK_MFMA_2 ? 2 : 1)) PROBE_FAIL("biogpt_hip_chain_device", false, "the launch takes %d row tile(s) per wave for this type, M = %d and N = %d", tiles, M, N);
        } else {
            const bool one = chain_one_column(cop, N, batch);
            if (one != (route == CK_VALU_1)) PROBE_FAIL("biogpt_hip_chain_device", false, "%s", one ? "one column of the context's own takes the 1-column kernel here" : "the 1-column kernel serves N = 1 without column states, at out_proj, fc1 (LayerNorm fused) and fc2 only");
        }
        return true;
    };
    if (!check_probe_columns(__func__, op == CP_QKV, N, dev_state, seq_states, col_mode, P, n_slots, k_slots, v_slots, route_ok)) return -1;
    HIP_TRY(-2, hipSetDevice(device));
    const int cols = ((N + 15) & ~15) + 1, ldo = lnq ? 0 : ((M + 127) & ~127) + 16, MQ = lnq ? 1024 : M;      // MQ: Q8 values per output column
    const size_t bpr = (size_t)K / QK, kv_b = op == CP_QKV ? (size_t)16 * P * 64 * 4 * (size_t)n_slots : 0;
    const bool with_resid = f32_out && op != CP_QKV && op != CP_LMHEAD;
    ProbeImage im;      // [weights | image | x, gain, bias of the LayerNorm or the Q8 columns | the stage's parts | out | out_q | out_d | out_s], guard columns and rows in the outputs
    const BlockRows wr = upload_block_rows(im, wtype, lnq ? nullptr : w_rows, M, K, mfma);
    const ProbePart o_x = im.in(ln_in ? x : nullptr, (size_t)N * 1024 * 4), o_lw = im.in(ln_in ? ln_w : nullptr, 4096), o_lb = im.in(ln_in ? ln_b : nullptr, 4096);
    const ProbePart o_aq = im.in(ln_in ? nullptr : aq_q, (size_t)N * K), o_ad = im.in(ln_in ? nullptr : aq_d, (size_t)N * bpr * 4), o_as = im.in(ln_in ? nullptr : aq_s, (size_t)N * bpr * 4);
    const StageParts sp = stage_parts(im, lnq ? nullptr : bias, (size_t)MQ * 4, with_resid ? resid : nullptr, (size_t)N * M * 4, dev_state, seq_states, N, k_slots, v_slots, kv_b);
    const ProbePart o_out = im.out(f32_out ? (size_t)cols * (op == CP_QKV ? 1024 : ldo) * 4 : 0), o_oq = im.out(q8_out ? (size_t)cols * MQ : 0),
                    o_od = im.out(q8_out ? (size_t)cols * (MQ / 32) * 4 : 0), o_os = im.out(o_od.bytes);
    if (!im.upload()) return -2;
    ChainLaunch g{-1, 256, N, 1, 0};
    if (lnq) {
        HIP_TRY(-2, launch_lnq(im.at<const float>(o_x), N, im.at<const float>(o_lw), im.at<const float>(o_lb), q81, im.at<int8_t>(o_oq), im.at<float>(o_od), im.at<uint32_t>(o_os), 0));
    } else {
        bgk::MatvecParams p = stage_params(im, wr.W(im), sp, 1024, P, N, op == CP_QKV, col_mode, o_out, ldo, M);
        p.inv_k = 1.0 / (double)K; p.k_pow2 = 1;
        if (ln_in) { p.x = im.at<const float>(o_x); p.ldx = 1024; p.ln_w = im.at<const float>(o_lw); p.ln_b = im.at<const float>(o_lb); }
        else { p.aq_q = im.at<const int8_t>(o_aq); p.aq_d = im.at<const float>(o_ad); p.aq_s = im.at<const uint32_t>(o_as); }
        if (q8_out) { p.oq_q = im.at<int8_t>(o_oq); p.oq_d = im.at<float>(o_od); p.oq_s = im.at<uint32_t>(o_os); }
        const bgk::DevMatrix img = wr.image(im);
        if (mfma) HIP_TRY(-2, wr.retile(im));
        HIP_TRY(-2, launch_chain(cop, p, 0, mfma ? &img : nullptr, &g));
        if (g.kernel != route) BG_FAIL(-2, "internal: the launch took kernel %d, not route %d", g.kernel, route);
    }
    HIP_TRY(-2, hipGetLastError());
    HIP_TRY(-2, hipDeviceSynchronize());
    report_launch(launched, {g.kernel, g.threads, g.grid_x, g.grid_y, g.lds, cols, ldo});
    if (!im.read(o_out, out) || !im.read(o_oq, out_q) || !im.read(o_od, out_d) || !im.read(o_os, out_s)) return -2;
    if (!im.read(sp.k, k_slots) || !im.read(sp.v, v_slots)) return -2;
    return 0;
}

// One stand-alone launch of the wide chain's linear stage (matmul_wide_kernel, kernels_mfma_wide.hip.h) over caller-supplied weights and Q8 columns, through
// bg_wide_launch -- the entry of PassLaunch::wide_stage -- on an image laid out by tile_image_place and built as ensure_tile_images builds a wide file's (the
// last row tile zero-padded, then bg_mfma_retile).  epi: 0 QKV (M == 3 K, 64 | K: K is d_model, heads of 64), 1 RESID, 2 GELU, 3 LOGITS; 16 | M but for LOGITS.
// w_rows: M rows of K / 32 blocks in the file's format.  aq_q [N][K] int8, aq_d [N][K / 32] f32, aq_s [N][K / 32] words, as a producer leaves them.
// QKV: exactly one of dev_state and seq_states (+ col_mode) names the column states; k_slots / v_slots [n_slots][K / 64][P][64] are updated in place.
// out comes back WHOLE as allocated and preset to 0xff: cols = N rounded up to 16, plus one guard column; QKV: [cols][K] (the q rows), otherwise [cols][ldo]
// with ldo = M rounded up to 128, plus 16 guard rows.  launched [8]: threads, grid x, grid y, static LDS bytes, cols, ldo, row tiles, 0.
int biogpt_hip_wide_chain_device(int device, int32_t epi, int32_t wtype, int32_t M, int32_t K, int32_t N, const void *w_rows, const int8_t *aq_q, const float *aq_d,
                                 const uint32_t *aq_s, const float *bias, const float *resid, const int32_t *dev_state, const int32_t *seq_states, int32_t col_mode,
                                 int32_t P, int32_t n_slots, float *k_slots, float *v_slots, float *out, int32_t *launched) {
    clear_error();
    if (epi < bgk::EPI_QKV || epi > bgk::EPI_LOGITS) BG_FAIL(-1, "epi %d is no epilogue of the wide chain (0 QKV, 1 RESID, 2 GELU, 3 LOGITS)", epi);
    if (wtype != T_Q4_0 && wtype != T_Q4_1 && wtype != T_Q5_0 && wtype != T_Q5_1 && wtype != T_Q8_0) BG_FAIL(-1, "type %d is no block format", wtype);
    if (N < 1 || N > 512) BG_FAIL(-1, "N must be in [1, 512]");
    if (K < QK || K > (1 << 16) || K % QK != 0) BG_FAIL(-1, "K must be a multiple of %d in [%d, %d]", QK, QK, 1 << 16);
    if (M < 1 || M > (1 << 20)) BG_FAIL(-1, "M must be in [1, %d]", 1 << 20);
    if (epi != bgk::EPI_LOGITS && M % 16 != 0) BG_FAIL(-1, "M = %d is no whole number of 16-row tiles: only the lm_head has a partial last tile", M);
    if (epi == bgk::EPI_QKV && (K % 64 != 0 || M != 3 * K)) BG_FAIL(-1, "q/k/v is 3 K x K with heads of 64 (got %d x %d)", M, K);
    if (!w_rows || !aq_q || !aq_d || !aq_s || !out) BG_FAIL(-1, "w_rows, aq_q, aq_d, aq_s or out is NULL");
    if (epi != bgk::EPI_LOGITS && !bias) BG_FAIL(-1, "bias is NULL");
    if (epi == bgk::EPI_RESID && !resid) BG_FAIL(-1, "resid is NULL");
    const bool qkv = epi == bgk::EPI_QKV;
    if (!check_probe_columns(__func__, qkv, N, dev_state, seq_states, col_mode, P, n_slots, k_slots, v_slots)) return -1;
    HIP_TRY(-2, hipSetDevice(device));
    const int q81 = (wtype == T_Q4_1 || wtype == T_Q5_1) ? 1 : 0;
    const int cols = ((N + 15) & ~15) + 1, ldo = ((M + 127) & ~127) + 16;
    const size_t bpr = (size_t)K / QK, kv_b = qkv ? (size_t)(K / 64) * P * 64 * 4 * (size_t)n_slots : 0;
    ProbeImage im;      // [weights | image | the Q8 columns | the stage's parts | out], guard column and rows in the output
    const BlockRows wr = upload_block_rows(im, wtype, w_rows, M, K, true);
    const ProbePart o_aq = im.in(aq_q, (size_t)N * K), o_ad = im.in(aq_d, (size_t)N * bpr * 4), o_as = im.in(aq_s, (size_t)N * bpr * 4);
    const StageParts sp = stage_parts(im, bias, (size_t)M * 4, epi == bgk::EPI_RESID ? resid : nullptr, (size_t)N * M * 4, dev_state, seq_states, N, k_slots, v_slots, kv_b);
    const ProbePart o_out = im.out((size_t)cols * (qkv ? K : ldo) * 4);
    if (!im.upload()) return -2;
    bgk::MatvecParams p = stage_params(im, wr.W(im), sp, K, P, N, qkv, col_mode, o_out, ldo, M);
    p.aq_q = im.at<const int8_t>(o_aq); p.aq_d = im.at<const float>(o_ad); p.aq_s = im.at<const uint32_t>(o_as);
    const bgk::DevMatrix img = wr.image(im);
    HIP_TRY(-2, wr.retile(im));
    HIP_TRY(-2, (hipError_t)bg_wide_launch(wtype, epi, &p, sizeof(p), &img, sizeof(img), 0));
    HIP_TRY(-2, hipGetLastError());
    HIP_TRY(-2, hipDeviceSynchronize());
    const int tiles = (M + 15) / 16;
    report_launch(launched, {256, (tiles + 3) / 4, (N + 15) / 16, 16 * (1024 + 16) + 16 * 33 * 4 * (q81 ? 2 : 1) /* WideLds::BYTES */, cols, ldo, tiles});
    if (!im.read(o_out, out) || !im.read(sp.k, k_slots) || !im.read(sp.v, v_slots)) return -2;
    return 0;
}

// A linear stage alone, timed: reps launches on device memory of arbitrary contents (the kernels' time does not depend on the values), each between two
// device events; one untimed launch in front.  which 0: matmul_wide_kernel with the residual epilogue at any (M, K) the wide chain takes; which 1: the
// BioGPT-base matmul_mfma_kernel at its out_proj (K 1024) or fc2 (K 4096) site, M = 1024 -- the yardstick per block MAC.  For tools/wide_chain_bench.py.
int biogpt_hip_wide_chain_bench(int device, int32_t which, int32_t wtype, int32_t M, int32_t K, int32_t N, int32_t reps, float *us_out) {
    clear_error();
    if (which != 0 && which != 1) BG_FAIL(-1, "which must be 0 (the wide kernel) or 1 (the BioGPT-base kernel)");
    if (wtype != T_Q4_0 && wtype != T_Q4_1 && wtype != T_Q5_0 && wtype != T_Q5_1 && wtype != T_Q8_0) BG_FAIL(-1, "type %d is no block format", wtype);
    if (N < 1 || N > 512) BG_FAIL(-1, "N must be in [1, 512]");
    if (K < QK || K > (1 << 16) || K % QK != 0) BG_FAIL(-1, "K must be a multiple of %d in [%d, %d]", QK, QK, 1 << 16);
    if (M < 16 || M > (1 << 20) || M % 16 != 0) BG_FAIL(-1, "M must be a multiple of 16 in [16, %d]", 1 << 20);
    if (which == 1 && !((K == 1024 || K == 4096) && M == 1024)) BG_FAIL(-1, "the BioGPT-base kernel is timed at out_proj (1024 x 1024) or fc2 (1024 x 4096)");
    if (reps < 1 || reps > PROBE_MAX_REPS) BG_FAIL(-1, "reps must be in [1, %d]", PROBE_MAX_REPS);
    if (!us_out) BG_FAIL(-1, "us_out is NULL");
    HIP_TRY(-2, hipSetDevice(device));
    const size_t bpr = (size_t)K / QK;
    ProbeImage im;      // every part of 0x11 bytes
    const BlockRows wr = upload_block_rows(im, wtype, nullptr, M, K, true, 0, 0x11);
    const ProbePart o_aq = im.fill((size_t)N * K, 0x11), o_ad = im.fill((size_t)N * bpr * 4, 0x11), o_as = im.fill((size_t)N * bpr * 4, 0x11), o_bias = im.fill((size_t)M * 4, 0x11),
                    o_res = im.fill((size_t)N * M * 4, 0x11), o_out = im.fill((size_t)N * M * 4, 0x11);
    if (!im.upload()) return -2;
    bgk::MatvecParams p{};
    p.W.type = wtype; p.W.M = M; p.W.K = K;
    p.eps = 1e-5f; p.D = 1024; p.dk = 64; p.dk_log2 = 6; p.P = 1;
    p.N = N;
    p.aq_q = im.at<const int8_t>(o_aq); p.aq_d = im.at<const float>(o_ad); p.aq_s = im.at<const uint32_t>(o_as);
    p.bias = im.at<const float>(o_bias); p.resid = im.at<const float>(o_res); p.ldr = M; p.out = im.at<float>(o_out); p.ldo = M;
    const bgk::DevMatrix img = wr.image(im);
    auto launch = [&]() -> hipError_t {
        if (which == 0) return (hipError_t)bg_wide_launch(wtype, bgk::EPI_RESID, &p, sizeof(p), &img, sizeof(img), 0);
        return launch_chain(K == 1024 ? CHAIN_OPROJ : CHAIN_FC2, p, 0, &img, nullptr);
    };
    HIP_TRY(-2, launch());      // one untimed launch in front
    HIP_TRY(-2, hipDeviceSynchronize());
    return time_launches(reps, nullptr, launch, [&](int i, float ms) { us_out[i] = ms * 1e3f; });
}

// One stand-alone launch of the float chain's linear stage (fchain_kernel, kernels_fchain.hip.h) over caller-supplied weights and f32 columns, through
// bg_fchain_launch (and bg_fchain_ln in front of it when ln_w is given) -- the entries of PassLaunch::float_stage.  epi: 0 QKV (M == 3 K, 64 | K: K is d_model,
// heads of 64), 1 RESID, 2 GELU, 3 LOGITS; any M.  wtype 0: w_rows is M rows of K f32; 1: of K f16 (bits).  x [N][K] f32.  cfg: 0 .. 2 a tile shape, -1 the
// launch's own choice.  QKV: exactly one of dev_state and seq_states (+ col_mode) names the column states; k_slots / v_slots [n_slots][K / 64][P][64] are
// updated in place.  out comes back WHOLE as allocated and preset to 0xff: cols = N rounded up to 16, plus one guard column; QKV: [cols][K] (the q rows),
// otherwise [cols][ldo] with ldo = M rounded up to 128, plus 16 guard rows; ln_out (may be NULL; with ln_w only) [cols][K]: the producer's rows.
// launched [8]: threads, grid x, grid y, static LDS bytes, cols, ldo, cfg, 0.
int biogpt_hip_fchain_device(int device, int32_t epi, int32_t wtype, int32_t M, int32_t K, int32_t N, int32_t cfg, const void *w_rows, const float *x, const float *ln_w,
                             const float *ln_b, const float *bias, const float *resid, const int32_t *dev_state, const int32_t *seq_states, int32_t col_mode, int32_t P,
                             int32_t n_slots, float *k_slots, float *v_slots, float *out, float *ln_out, int32_t *launched) {
    clear_error();
    if (epi < bgk::EPI_QKV || epi > bgk::EPI_LOGITS) BG_FAIL(-1, "epi %d is no epilogue of the float chain (0 QKV, 1 RESID, 2 GELU, 3 LOGITS)", epi);
    if (wtype != T_F32 && wtype != T_F16) BG_FAIL(-1, "type %d is no float format (0 F32, 1 F16)", wtype);
    if (cfg < -1 || cfg > 2) BG_FAIL(-1, "cfg must be in [-1, 2]");
    if (N < 1 || N > 512) BG_FAIL(-1, "N must be in [1, 512]");
    if (K < QK || K > (1 << 16) || K % QK != 0) BG_FAIL(-1, "K must be a multiple of %d in [%d, %d]", QK, QK, 1 << 16);
    if (M < 1 || M > (1 << 20)) BG_FAIL(-1, "M must be in [1, %d]", 1 << 20);
    if (epi == bgk::EPI_QKV && (K % 64 != 0 || M != 3 * K)) BG_FAIL(-1, "q/k/v is 3 K x K with heads of 64 (got %d x %d)", M, K);
    if (!w_rows || !x || !out) BG_FAIL(-1, "w_rows, x or out is NULL");
    if ((ln_w != nullptr) != (ln_b != nullptr)) BG_FAIL(-1, "ln_w and ln_b come together");
    if (ln_out && !ln_w) BG_FAIL(-1, "ln_out needs ln_w and ln_b");
    if (epi != bgk::EPI_LOGITS && !bias) BG_FAIL(-1, "bias is NULL");
    if (epi == bgk::EPI_RESID && !resid) BG_FAIL(-1, "resid is NULL");
    const bool qkv = epi == bgk::EPI_QKV;
    if (!check_probe_columns(__func__, qkv, N, dev_state, seq_states, col_mode, P, n_slots, k_slots, v_slots)) return -1;
    HIP_TRY(-2, hipSetDevice(device));
    const int cols = ((N + 15) & ~15) + 1, ldo = ((M + 127) & ~127) + 16;
    const size_t kv_b = qkv ? (size_t)(K / 64) * P * 64 * 4 * (size_t)n_slots : 0;
    ProbeImage im;      // [weights | x | gain | bias of the LayerNorm | the stage's parts | the producer's rows | out], guard columns and rows in both outputs
    const BlockRows wr = upload_block_rows(im, wtype, w_rows, M, K, false);
    const ProbePart o_x = im.in(x, (size_t)N * K * 4), o_lw = im.in(ln_w, (size_t)K * 4), o_lb = im.in(ln_b, (size_t)K * 4);
    const StageParts sp = stage_parts(im, bias, (size_t)M * 4, epi == bgk::EPI_RESID ? resid : nullptr, (size_t)N * M * 4, dev_state, seq_states, N, k_slots, v_slots, kv_b);
    const ProbePart o_ln = im.out(ln_w ? (size_t)cols * K * 4 : 0), o_out = im.out((size_t)cols * (qkv ? K : ldo) * 4);
    if (!im.upload()) return -2;
    bgk::MatvecParams p = stage_params(im, wr.W(im), sp, K, P, N, qkv, col_mode, o_out, ldo, M);
    p.x = im.at<const float>(o_x); p.ldx = K;
    if (ln_w) {
        HIP_TRY(-2, (hipError_t)bg_fchain_ln(wtype, p.x, K, K, N, im.at<const float>(o_lw), im.at<const float>(o_lb), 1e-5f, im.at<float>(o_ln), 0));
        p.x = im.at<const float>(o_ln);
    }
    int32_t five[5] = {0, 0, 0, 0, 0};
    HIP_TRY(-2, (hipError_t)bg_fchain_launch(wtype, epi, &p, sizeof(p), cfg, 0, five));
    HIP_TRY(-2, hipGetLastError());
    HIP_TRY(-2, hipDeviceSynchronize());
    report_launch(launched, {five[0], five[1], five[2], five[3], cols, ldo, five[4]});
    if (!im.read(o_out, out) || (ln_out && !im.read(o_ln, ln_out)) || !im.read(sp.k, k_slots) || !im.read(sp.v, v_slots)) return -2;
    return 0;
}

// A linear stage of a float file alone, timed: reps launches on device memory filled with 0x3c bytes (ordinary normal values), each between two device
// events; one untimed launch in front.  which 0: fchain_kernel with the residual epilogue at tile shape cfg (-1: the launch's choice); which 1: the generic
// matvec_kernel<PRO_PLAIN, EPI_RESID> as a prompt pass of the context's own columns launches it (launch_mv) -- the yardstick.  For tools/float_chain_bench.py.
int biogpt_hip_fchain_bench(int device, int32_t which, int32_t wtype, int32_t M, int32_t K, int32_t N, int32_t cfg, int32_t reps, float *us_out) {
    clear_error();
    if (which != 0 && which != 1) BG_FAIL(-1, "which must be 0 (the float chain's kernel) or 1 (the generic mat-vec kernel)");
    if (wtype != T_F32 && wtype != T_F16) BG_FAIL(-1, "type %d is no float format (0 F32, 1 F16)", wtype);
    if (cfg < -1 || cfg > 2) BG_FAIL(-1, "cfg must be in [-1, 2]");
    if (N < 1 || N > 512) BG_FAIL(-1, "N must be in [1, 512]");
    if (K < QK || K > (1 << 16) || K % QK != 0) BG_FAIL(-1, "K must be a multiple of %d in [%d, %d]", QK, QK, 1 << 16);
    if (M < 1 || M > (1 << 20)) BG_FAIL(-1, "M must be in [1, %d]", 1 << 20);
    if (reps < 1 || reps > PROBE_MAX_REPS) BG_FAIL(-1, "reps must be in [1, %d]", PROBE_MAX_REPS);
    if (!us_out) BG_FAIL(-1, "us_out is NULL");
    HIP_TRY(-2, hipSetDevice(device));
    ProbeImage im;      // every part of 0x3c bytes (f32 0.0115, f16 1.06: ordinary products)
    const ProbePart o_w = im.fill((size_t)M * K * (wtype == T_F32 ? 4 : 2), 0x3c), o_x = im.fill((size_t)N * K * 4, 0x3c), o_bias = im.fill((size_t)M * 4, 0x3c),
                    o_res = im.fill((size_t)N * M * 4, 0x3c), o_out = im.fill((size_t)N * M * 4, 0x3c);
    if (!im.upload()) return -2;
    EngineOptions opt{};
    opt.load();
    MatSlot m{};
    m.type = wtype; m.M = M; m.K = K;
    const MvShape s = mv_shape(wtype, M, K);
    bgk::MatvecParams p{};
    p.W.qs = im.at<uint8_t>(o_w); p.W.type = wtype; p.W.M = M; p.W.K = K;
    p.upr = s.upr; p.lpr_log2 = s.lpr_log2; p.nit = s.nit; p.rpw = s.rpw;
    p.eps = 1e-5f; p.D = 1024; p.dk = 64; p.dk_log2 = 6; p.P = 1;
    p.inv_k = 1.0 / (double)K; p.k_pow2 = (K & (K - 1)) == 0;
    p.N = N; p.x = im.at<const float>(o_x); p.ldx = K;
    p.bias = im.at<const float>(o_bias); p.resid = im.at<const float>(o_res); p.ldr = M; p.out = im.at<float>(o_out); p.ldo = M;
    auto launch = [&]() -> hipError_t {
        if (which == 0) return (hipError_t)bg_fchain_launch(wtype, bgk::EPI_RESID, &p, sizeof(p), cfg, 0, nullptr);
        return launch_mv<bgk::PRO_PLAIN, bgk::EPI_RESID>(opt, p, s, 0);
    };
    HIP_TRY(-2, launch());      // one untimed launch in front
    HIP_TRY(-2, hipDeviceSynchronize());
    return time_launches(reps, nullptr, launch, [&](int i, float ms) { us_out[i] = ms * 1e3f; });
}

// The four kernels of the embedding tail (kernels_embed.hip.h) alone, over caller-supplied rows, through launch_ln_rows / launch_pool_rows / launch_pool_finish /
// launch_head_rows -- the helpers of enqueue_final, embed_batch_once and enqueue_head -- so the probe's launch is the engine's.  No model, no context.
// stage 0 LN: x [n_rows][W], ln_w / ln_b [W]; W == 1024 takes ln_rows_kernel<1024>, any other width <0>.  seq_states (may be NULL) [n_rows][8] words with slot_div
//   and P: row i lands at (seq_id / slot_div) * P + n_past of n_out_rows rows; without states n_out_rows == n_rows.  out [n_out_rows + 1][W].
// stage 1 POOL: mode 0 NONE, 1 LAST, 2 MEAN; x the rows of n_passes passes one behind the other, pass_cols [n_passes] columns each (n_rows in all), seq_states
//   [n_rows][8] words (seq_id, n_past), lens [n_seqs].  LAST / MEAN: pool_rows_kernel once per pass in stream order (MEAN: on an accumulator zeroed first), then
//   pool_finish_kernel if there is a mean or a normalisation; out [n_seqs + 1][W], acc (MEAN) [n_seqs + 1][W] doubles.  NONE (with normalize): the rows themselves
//   are normalised; out [n_rows + 1][W].
// stage 2 HEAD: x [n_rows][W], w [n_out][W], b [n_out] or NULL; out [n_rows + 1][n_out].
// Every output comes back WHOLE as allocated and preset to 0xff bytes: the last row is a guard row.  launched [8]: the kernel (ln_rows_kernel's template argument
// 1024 / 0, 1 pool_rows_kernel, 3 head_rows_kernel), threads, grid x, grid y, dynamic LDS bytes (POOL: of the last pass's launch), the grid of pool_finish_kernel
// (0: not launched), the number of pool_rows_kernel launches, 0.
int biogpt_hip_embed_device(int device, int32_t stage, int32_t W, int32_t n_rows, const float *x, const float *ln_w, const float *ln_b, const int32_t *seq_states,
                            int32_t slot_div, int32_t P, int32_t n_out_rows, int32_t mode, int32_t normalize, const int32_t *lens, int32_t n_seqs, int32_t n_passes,
                            const int32_t *pass_cols, const float *w, const float *b, int32_t n_out, float *out, double *acc, int32_t *launched) {
    clear_error();
    if (stage < 0 || stage > 2) BG_FAIL(-1, "stage %d is no stage (0 LN, 1 POOL, 2 HEAD)", stage);
    if (W < 4 || W > (1 << 16) || W % 4 != 0) BG_FAIL(-1, "W must be a multiple of 4 in [4, %d] (got %d)", 1 << 16, W);
    if (n_rows < 1 || n_rows > (stage == 1 ? 1 << 16 : 512)) BG_FAIL(-1, "n_rows must be in [1, %d] (the columns of a pass; POOL: of all passes)", stage == 1 ? 1 << 16 : 512);
    if (!x || !out) BG_FAIL(-1, "x or out is NULL");
    const bgk::SeqState *hs = reinterpret_cast<const bgk::SeqState *>(seq_states);
    size_t rows_out = 0, ld_out = (size_t)W;
    if (stage == 0) {
        if (!ln_w || !ln_b) BG_FAIL(-1, "ln_w or ln_b is NULL");
        if (!hs) {
            if (n_out_rows != n_rows) BG_FAIL(-1, "n_out_rows must be n_rows without seq_states");
        } else {
            if (slot_div < 1) BG_FAIL(-1, "slot_div must be at least 1");
            if (P < 1 || P > 8192) BG_FAIL(-1, "P must be in [1, 8192]");
            if (n_out_rows < 1 || n_out_rows > (1 << 16)) BG_FAIL(-1, "n_out_rows must be in [1, %d]", 1 << 16);
            std::set<long> seen;      // every row inside the output, no two columns on one row
            for (int i = 0; i < n_rows; i++) {
                if (hs[i].seq_id < 0) BG_FAIL(-1, "column %d: seq_id %d is negative", i, hs[i].seq_id);
                if (hs[i].n_past < 0 || hs[i].n_past >= P) BG_FAIL(-1, "column %d: position %d outside [0, P)", i, hs[i].n_past);
                const long r = (long)(hs[i].seq_id / slot_div) * P + hs[i].n_past;
                if (r >= n_out_rows) BG_FAIL(-1, "column %d: row %ld outside [0, n_out_rows)", i, r);
                if (!seen.insert(r).second) BG_FAIL(-1, "column %d: a second column writes row %ld", i, r);
            }
        }
        rows_out = (size_t)n_out_rows;
    } else if (stage == 1) {
        if (mode < bgk::POOL_NONE || mode > bgk::POOL_MEAN) BG_FAIL(-1, "unknown mode (%d): 0 none, 1 last token, 2 mean", mode);
        if (normalize != 0 && normalize != 1) BG_FAIL(-1, "normalize (%d) must be 0 or 1", normalize);
        if (mode == bgk::POOL_NONE && !normalize) BG_FAIL(-1, "mode 0 without normalize launches nothing");
        if (mode == bgk::POOL_MEAN && !acc) BG_FAIL(-1, "acc is NULL with mode 2");
        if (mode != bgk::POOL_NONE) {
            if (!lens || !hs || !pass_cols) BG_FAIL(-1, "lens, seq_states or pass_cols is NULL");
            if (n_seqs < 1 || n_seqs > 512) BG_FAIL(-1, "n_seqs must be in [1, 512]");
            if (n_passes < 1 || n_passes > n_rows) BG_FAIL(-1, "n_passes must be in [1, n_rows]");
            for (int s = 0; s < n_seqs; s++)
                if (lens[s] < 1) BG_FAIL(-1, "lens[%d] must be at least 1", s);
            long at = 0;
            for (int p = 0; p < n_passes; p++) {      // the layouts pack_column_passes produces: a sequence's columns consecutive, at consecutive positions below its length, up to its last position or the pass's end
                if (pass_cols[p] < 1 || pass_cols[p] > 512 || at + pass_cols[p] > n_rows) BG_FAIL(-1, "pass_cols[%d] = %d: a pass has 1 .. 512 columns, the passes n_rows in all", p, pass_cols[p]);
                std::set<int> done;
                for (long i = at; i < at + pass_cols[p]; i++) {
                    const int s = hs[i].seq_id, pos = hs[i].n_past;
                    if (s < 0 || s >= n_seqs) BG_FAIL(-1, "column %ld: seq_id %d outside [0, n_seqs)", i, s);
                    if (pos < 0 || pos >= lens[s]) BG_FAIL(-1, "column %ld: position %d at or past lens[%d] = %d", i, pos, s, lens[s]);
                    if (i > at && hs[i - 1].seq_id == s) {
                        if (pos != hs[i - 1].n_past + 1) BG_FAIL(-1, "column %ld: positions of sequence %d not consecutive (%d after %d)", i, s, pos, hs[i - 1].n_past);
                    } else if (!done.insert(s).second) BG_FAIL(-1, "column %ld: the columns of sequence %d are not consecutive in pass %d", i, s, p);
                }
                for (long i = at + 1; i < at + pass_cols[p]; i++) {      // a run ends with its sequence or with the pass (pool_rows_kernel would add the columns behind it to its sequence)
                    const int s = hs[i - 1].seq_id;
                    if (hs[i].seq_id != s && hs[i - 1].n_past != lens[s] - 1)
                        BG_FAIL(-1, "column %ld: sequence %d stops at position %d, short of lens[%d] - 1 = %d, inside pass %d", i - 1, s, hs[i - 1].n_past, s, lens[s] - 1, p);
                }
                at += pass_cols[p];
            }
            if (at != n_rows) BG_FAIL(-1, "pass_cols sum to %ld, not n_rows = %d", at, n_rows);
        }
        rows_out = mode == bgk::POOL_NONE ? (size_t)n_rows : (size_t)n_seqs;
    } else {
        if (n_out < 1 || n_out > 256) BG_FAIL(-1, "n_out (%d) must be in [1, 256]", n_out);
        if (!w) BG_FAIL(-1, "w is NULL");
        if (!check_head_width(W)) return -1;
        rows_out = (size_t)n_rows; ld_out = (size_t)n_out;
    }
    HIP_TRY(-2, hipSetDevice(device));
    const bool pool = stage == 1 && mode != bgk::POOL_NONE, mean = pool && mode == bgk::POOL_MEAN;
    ProbeImage im;      // [x | gain | bias | column states | lens | head matrix | head bias | accumulator | out]: the last two with their guard rows
    const ProbePart o_x = im.in(x, (size_t)n_rows * W * 4), o_lw = im.in(stage == 0 ? ln_w : nullptr, (size_t)W * 4), o_lb = im.in(stage == 0 ? ln_b : nullptr, (size_t)W * 4),
                    o_st = im.in(stage != 2 ? seq_states : nullptr, sizeof(bgk::SeqState) * (size_t)n_rows), o_lens = im.in(pool ? lens : nullptr, (size_t)n_seqs * 4),
                    o_w = im.in(stage == 2 ? w : nullptr, (size_t)n_out * W * 4), o_b = im.in(stage == 2 ? b : nullptr, (size_t)n_out * 4),
                    o_acc = im.out(mean ? (size_t)(n_seqs + 1) * W * 8 : 0), o_out = im.out((rows_out + 1) * ld_out * 4);
    if (!im.upload()) return -2;
    EmbedLaunch k{}, fin{};
    int32_t n_launches = 0;
    const bgk::SeqState *d_st = im.at<const bgk::SeqState>(o_st);
    float *d_out = im.at<float>(o_out);
    if (stage == 0) {
        HIP_TRY(-2, launch_ln_rows(0, im.at<const float>(o_x), W, W, n_rows, im.at<const float>(o_lw), im.at<const float>(o_lb), d_out, hs ? d_st : nullptr, hs ? slot_div : 0, P, &k));
    } else if (stage == 1) {
        double *d_acc = mean ? im.at<double>(o_acc) : nullptr;
        if (pool) {
            if (d_acc) HIP_TRY(-2, im.clear(o_acc, (size_t)n_seqs * W * 8));
            size_t at = 0;
            for (int p = 0; p < n_passes; p++) {
                HIP_TRY(-2, launch_pool_rows(0, im.at<const float>(o_x) + at * W, pass_cols[p], W, d_st + at, im.at<const int32_t>(o_lens), mode, d_out, d_acc, &k));
                at += (size_t)pass_cols[p];
                n_launches++;
            }
        } else {
            HIP_TRY(-2, im.restore(o_out, o_x));      // (a direct call's rows are written where they are normalised)
        }
        if (pool_needs_finish(d_acc, normalize))
            HIP_TRY(-2, launch_pool_finish(0, d_out, (int)rows_out, W, d_acc, im.at<const int32_t>(o_lens), normalize, &fin));
    } else {
        HIP_TRY(-2, launch_head_rows(0, im.at<const float>(o_x), n_rows, W, im.at<const float>(o_w), b ? im.at<const float>(o_b) : nullptr, n_out, d_out, &k));
    }
    HIP_TRY(-2, hipDeviceSynchronize());
    report_launch(launched, {k.kernel, k.threads, k.grid_x, k.grid_y, k.lds, fin.grid_x, n_launches});
    return im.read(o_out, out) && (!mean || im.read(o_acc, acc)) ? 0 : -2;
}

// The token tail alone (the lm_head's arg-max partials, argmax_kernel, topk_kernel and the host selections of biogpt_hip_eval_topk), over caller-supplied inputs,
// through launch_lm_head_row / launch_argmax / launch_topk -- the helpers of enqueue_decode_fused, enqueue_xcols and enqueue_final, of enqueue_argmax and of
// eval_topk_once -- so the probe's launch is the engine's.  No model, no context.  n: M (PARTIALS), nparts (FINISH), V (the selections).
// stage 0 PARTIALS: w_rows: n rows of 1024 weights in the file's format (wtype 0 F32, or a block format), x / ln_w / ln_b [1024].  out_val [n + 16] the logits row,
//   part_val / part_idx [n + 16] the partials.  launched: {kernel (0 lm_stream_kernel, 1 matvec_fast_kernel, 2 matvec_kernel), grid = partials, rows per partial}.
// stage 1 FINISH: part_in_val / part_in_idx [n] partials, n in [1, 4096]; state [4] (n_past, n_gen, causal, chunk), n_eval, n_positions in [1, 4096].  out_idx
//   [4 + 2 n_positions + 16]: the probe's state block after the kernel -- the four words, tokens [n_positions], gen_ids [n_positions], 16 guard words; everything
//   behind the four words preset to 0xff.  n_vocab: the clamp's bound.
// stage 2 TOPK: row [n], part_in_val [nparts] (1 .. 4096), k in [1, min(64, n)].  out_val / out_idx [64 + 16] the pairs, part_idx [16]: word 0 out_n.
// stage 3 HOST_TOPK, 4 HOST_BLOCKS (part_in_val: the maxima of the row's ceil(n / 64) 64-row blocks), 5 HOST_FULL (topk_full_row): the same outputs from the host
//   selections, word 0 of part_idx the count they return; no HIP call at all.
// Device outputs come back WHOLE as allocated and preset to 0xff bytes.  launched [8]: stage 0 as above; 1: {256, 1}; 2: {1024, 1}; host stages: zeros.
int biogpt_hip_tail_device(int device, int32_t stage, int32_t wtype, int32_t n, const void *w_rows, const float *x, const float *ln_w, const float *ln_b, const float *row,
                           const float *part_in_val, const int32_t *part_in_idx, int32_t nparts, int32_t k, const int32_t *state, int32_t n_eval, int32_t n_positions,
                           int32_t n_vocab, float *out_val, int32_t *out_idx, float *part_val, int32_t *part_idx, int32_t *launched) {
    clear_error();
    if (stage < 0 || stage > 5) BG_FAIL(-1, "stage %d is no stage (0 PARTIALS, 1 FINISH, 2 TOPK, 3 HOST_TOPK, 4 HOST_BLOCKS, 5 HOST_FULL)", stage);
    if (stage == 0) {
        const bool block = wtype == T_Q4_0 || wtype == T_Q4_1 || wtype == T_Q5_0 || wtype == T_Q5_1 || wtype == T_Q8_0;
        if (!block && wtype != T_F32) BG_FAIL(-1, "type %d is neither F32 nor a block format", wtype);
        if (n < 1 || n > (1 << 17)) BG_FAIL(-1, "M must be in [1, %d]", 1 << 17);
        if (!w_rows || !x || !ln_w || !ln_b) BG_FAIL(-1, "w_rows, x, ln_w or ln_b is NULL");
        if (!out_val || !part_val || !part_idx) BG_FAIL(-1, "out_val, part_val or part_idx is NULL");
        HIP_TRY(-2, hipSetDevice(device));
        const int M = n, K = 1024;
        const size_t cap_b = ((size_t)M + 16) * 4;
        const MvShape s = mv_shape(wtype, M, K);
        if (s.grid > M + 16) BG_FAIL(-2, "internal: %d partials for %d rows", s.grid, M);
        ProbeImage im;
        const BlockRows wr = upload_block_rows(im, wtype, w_rows, M, K, false, 16);
        const ProbePart o_x = im.in(x, K * 4), o_lw = im.in(ln_w, K * 4), o_lb = im.in(ln_b, K * 4), o_out = im.out(cap_b), o_pv = im.out(cap_b), o_pi = im.out(cap_b);
        if (!im.upload()) return -2;
        EngineOptions opt{};
        opt.load();
        bgk::MatvecParams p{};
        p.W = wr.W(im);
        p.upr = s.upr; p.lpr_log2 = s.lpr_log2; p.nit = s.nit; p.rpw = s.rpw;
        p.eps = 1e-5f; p.D = K; p.dk = 64; p.dk_log2 = 6; p.P = 1;
        p.inv_k = 1.0 / (double)K; p.k_pow2 = true;
        int grid = 0;
        MvLaunch took{-1, 0, 0};
        HIP_TRY(-2, launch_lm_head_row(opt, p, s, im.at<const float>(o_x), im.at<const float>(o_lw), im.at<const float>(o_lb), im.at<float>(o_out), im.at<float>(o_pv),
                                       im.at<int32_t>(o_pi), 0, &grid, &took));
        HIP_TRY(-2, hipDeviceSynchronize());
        report_launch(launched, {took.kernel, grid, took.rows_per_part});      // as the launch itself reports them
        return im.read(o_out, out_val) && im.read(o_pv, part_val) && im.read(o_pi, part_idx) ? 0 : -2;
    }
    if (stage == 1) {
        if (n < 1 || n > 4096) BG_FAIL(-1, "nparts must be in [1, 4096] (the partial buffers of a context)");
        if (!part_in_val || !part_in_idx || !state || !out_idx) BG_FAIL(-1, "part_in_val, part_in_idx, state or out_idx is NULL");
        if (n_positions < 1 || n_positions > 4096) BG_FAIL(-1, "n_positions must be in [1, 4096]");
        if (n_vocab < 1) BG_FAIL(-1, "n_vocab must be at least 1");
        if (state[1] < 0) BG_FAIL(-1, "n_gen %d is negative (gen_ids[n_gen] would be written in front of the block)", state[1]);
        HIP_TRY(-2, hipSetDevice(device));
        const size_t st_words = 4 + 2 * (size_t)n_positions + 16;
        std::vector<int32_t> st(st_words, -1);      // (0xff bytes behind the four words)
        std::memcpy(st.data(), state, sizeof(bgk::DevState));
        ProbeImage im;
        const ProbePart o_pv = im.in(part_in_val, (size_t)n * 4), o_pi = im.in(part_in_idx, (size_t)n * 4), o_st = im.out(st_words * 4, st.data());
        if (!im.upload()) return -2;
        HIP_TRY(-2, launch_argmax(im.at<const float>(o_pv), im.at<const int32_t>(o_pi), n, im.at<bgk::DevState>(o_st), n_eval, n_positions, n_vocab, 0));
        HIP_TRY(-2, hipDeviceSynchronize());
        report_launch(launched, {256, 1});
        return im.read(o_st, out_idx) ? 0 : -2;
    }
    // the selections
    if (n < 1 || n > (1 << 20)) BG_FAIL(-1, "V must be in [1, %d]", 1 << 20);
    if (k < 1 || k > 64 || k > n) BG_FAIL(-1, "k must be in [1, min(64, V)] (biogpt_hip_eval_topk clamps it to the vocabulary)");
    if (!row || !out_val || !out_idx || !part_idx) BG_FAIL(-1, "row, out_val, out_idx or part_idx is NULL");
    if (stage == 2 || stage == 4) {
        if (!part_in_val) BG_FAIL(-1, "part_in_val is NULL");
        if (nparts < 1 || nparts > 4096) BG_FAIL(-1, "nparts must be in [1, 4096] (the partial buffers of a context)");
        if (stage == 4 && nparts != (n + 63) / 64) BG_FAIL(-1, "HOST_BLOCKS walks the row's %d 64-row blocks (got nparts = %d)", (n + 63) / 64, nparts);
    }
    if (stage == 2) {
        HIP_TRY(-2, hipSetDevice(device));
        ProbeImage im;
        const ProbePart o_row = im.in(row, (size_t)n * 4), o_pv = im.in(part_in_val, (size_t)nparts * 4), o_ov = im.out(80 * 4), o_oi = im.out(80 * 4), o_on = im.out(16 * 4);
        if (!im.upload()) return -2;
        HIP_TRY(-2, launch_topk(im.at<const float>(o_row), n, k, im.at<const float>(o_pv), nparts, im.at<float>(o_ov), im.at<int32_t>(o_oi), im.at<int32_t>(o_on), 0));
        HIP_TRY(-2, hipDeviceSynchronize());
        report_launch(launched, {1024, 1});
        return im.read(o_ov, out_val) && im.read(o_oi, out_idx) && im.read(o_on, part_idx) ? 0 : -2;
    }
    std::memset(out_val, 0xff, 80 * 4); std::memset(out_idx, 0xff, 80 * 4); std::memset(part_idx, 0xff, 16 * 4);
    if (stage == 3) part_idx[0] = host_topk(row, n, k, out_val, out_idx);
    else if (stage == 4) part_idx[0] = host_topk_blocks(row, n, k, part_in_val, nparts, out_val, out_idx);
    else { topk_full_row(row, n, k, out_val, out_idx); part_idx[0] = k; }
    report_launch(launched, {});
    return 0;
}

// ---- the kernels of the SIMD association alone (kernels_assoc.hip.h), through the launch functions of a context in mode 1 ----
// stage 0 Q8: x [N][K] -> the rows as the mat-vec's prologue leaves them in LDS (behind the LayerNorm when ln_w / ln_b are given): out_q [N + 1][K] codes,
//   out_d [N + 1][K / 32] the scale the dot reads (through f16 for the Q8_0 form), out_s [N + 1][K / 32] words (Q8_0: the integer sum; Q8_1: bits of d * sum).
//   wtype names the weight format whose activation form it is (Q4_1 / Q5_1: Q8_1).
// stage 1 MATVEC: one launch of matvec_simd_kernel<wtype, pro, epi>: pro 0 PLAIN, 1 LN (ln_w, ln_b); epi 0 QKV (M == 3 K, 64 | K; dev_state, P and
//   k_slots / v_slots [1][K / 64][P][64], updated in place; out = the q rows [N + 1][K]), 1 RESID (bias, resid [N][M]), 2 GELU (bias), 3 LOGITS (N == 1: the
//   arg-max partial of every workgroup into pmax_val / pmax_idx [1025]; either NULL: none).  w_rows: M rows of K / 32 blocks in the file's format.
//   out but for QKV: [N + 1][M + 16].  N is what one workgroup row takes: 1 .. 8.
// stage 2 ATTN: attn_simd_kernel over q [N][H * 64], k_slots / v_slots [H][P][64] and dev_state {n_past, n_gen, causal, chunk}, from which column i's visible
//   keys follow as in every attention kernel (at most 1024, at most P); out [N + 1][H * 64].
// The outputs come back WHOLE as allocated and preset to 0xff bytes: what the launch does not write reads as NaN / -1.  launched [8]: stage 0 / 1: threads,
// grid x, grid y, dynamic LDS bytes, columns per workgroup, rows per workgroup; stage 2: AK_SIMD, threads, grid x, grid y, static LDS bytes.
int biogpt_hip_assoc_device(int device, int32_t stage, int32_t wtype, int32_t pro, int32_t epi, int32_t M, int32_t K, int32_t N, int32_t H, int32_t P, const void *w_rows,
                            const float *x, const float *ln_w, const float *ln_b, const float *bias, const float *resid, const int32_t *dev_state, const float *q,
                            float *k_slots, float *v_slots, float *out, int8_t *out_q, float *out_d, uint32_t *out_s, float *pmax_val, int32_t *pmax_idx,
                            int32_t *launched) {
    clear_error();
    if (stage < 0 || stage > 2) BG_FAIL(-1, "stage %d is no stage (0 Q8, 1 MATVEC, 2 ATTN)", stage);
    if (stage == 2) {
        if (H < 1 || H > 64) BG_FAIL(-1, "H must be in [1, 64]");
        if (N < 1 || N > 512) BG_FAIL(-1, "N must be in [1, 512]");
        if (P < 1 || P > 8192) BG_FAIL(-1, "P must be in [1, 8192]");
        if (!q || !k_slots || !v_slots || !dev_state || !out) BG_FAIL(-1, "q, k_slots, v_slots, dev_state or out is NULL");
        if (dev_state[0] < 0) BG_FAIL(-1, "n_past %d is negative", dev_state[0]);
        for (int i = 0; i < N; i++) {
            const int T = host_visible_keys(dev_state, i, N);
            if (T < 1 || T > bgk::SIMD_ATTN_MAXT) BG_FAIL(-1, "column %d sees T = %d keys: the kernel holds 1 .. %d", i, T, bgk::SIMD_ATTN_MAXT);
            if (T > P) BG_FAIL(-1, "column %d sees %d keys of a table of P = %d rows", i, T, P);
        }
        HIP_TRY(-2, hipSetDevice(device));
        const size_t D = (size_t)H * 64, kv_b = (size_t)H * P * 64 * 4;
        ProbeImage im;      // [K | V | q | context state | exp table | out], one guard row
        const ProbePart o_k = im.in(k_slots, kv_b), o_v = im.in(v_slots, kv_b), o_q = im.in(q, (size_t)N * D * 4), o_ds = im.in(dev_state, sizeof(bgk::DevState));
        const ProbePart o_tab = im.own(exp_table_f16()), o_out = im.out((size_t)(N + 1) * D * 4);
        if (!im.upload()) return -2;
        bgk::AttnParams a{};
        a.q = im.at<const float>(o_q); a.kcache = im.at<const float>(o_k); a.vcache = im.at<const float>(o_v); a.out = im.at<float>(o_out);
        a.st = im.at<const bgk::DevState>(o_ds); a.exp_tab = im.at<const uint16_t>(o_tab);
        a.N = N; a.D = (int32_t)D; a.dk = 64; a.P = P;
        const AttnLaunch g = launch_attn_simd(a, H, N, 0);
        HIP_TRY(-2, hipGetLastError());
        HIP_TRY(-2, hipDeviceSynchronize());
        report_launch(launched, {g.kernel, g.threads, g.grid_x, g.grid_y, (int32_t)g.lds});
        return im.read(o_out, out) ? 0 : -2;
    }
    if (wtype != T_Q4_0 && wtype != T_Q4_1 && wtype != T_Q5_0 && wtype != T_Q5_1 && wtype != T_Q8_0) BG_FAIL(-1, "type %d is no block format", wtype);
    if (K < QK || K > (1 << 16) || K % QK != 0) BG_FAIL(-1, "K must be a multiple of %d in [%d, %d]", QK, QK, 1 << 16);
    if (N < 1 || N > bgk::SIMD_MAX_COLS) BG_FAIL(-1, "N must be in [1, %d]: the columns of one workgroup row", bgk::SIMD_MAX_COLS);
    if (!x) BG_FAIL(-1, "x is NULL");
    if ((ln_w != nullptr) != (ln_b != nullptr)) BG_FAIL(-1, "ln_w and ln_b come together");
    const int q81 = (wtype == T_Q4_1 || wtype == T_Q5_1) ? 1 : 0;
    if (stage == 0) {
        if (!out_q || !out_d || !out_s) BG_FAIL(-1, "out_q, out_d or out_s is NULL");
        HIP_TRY(-2, hipSetDevice(device));
        const size_t bpr = (size_t)K / QK;
        ProbeImage im;      // [x | gain | bias of the LayerNorm | codes | d | s], one guard row each
        const ProbePart o_x = im.in(x, (size_t)N * K * 4), o_lw = im.in(ln_w, (size_t)K * 4), o_lb = im.in(ln_b, (size_t)K * 4);
        const ProbePart o_q = im.out((size_t)(N + 1) * K), o_d = im.out((size_t)(N + 1) * bpr * 4), o_s = im.out((size_t)(N + 1) * bpr * 4);
        if (!im.upload()) return -2;
        bgk::Q8SimdParams qp{};
        qp.x = im.at<const float>(o_x); qp.K = K; qp.N = N; qp.q81 = q81; qp.eps = 1e-5f;
        if (ln_w) { qp.ln_w = im.at<const float>(o_lw); qp.ln_b = im.at<const float>(o_lb); }
        qp.oq = im.at<int8_t>(o_q); qp.od = im.at<float>(o_d); qp.os = im.at<uint32_t>(o_s);
        SimdLaunch g{};
        HIP_TRY(-2, launch_q8_simd_rows(qp, 0, &g));
        HIP_TRY(-2, hipDeviceSynchronize());
        report_launch(launched, {g.threads, g.grid_x, g.grid_y, g.lds, g.nc, g.rows});
        return im.read(o_q, out_q) && im.read(o_d, out_d) && im.read(o_s, out_s) ? 0 : -2;
    }
    // stage 1
    if (pro != bgk::PRO_PLAIN && pro != bgk::PRO_LN) BG_FAIL(-1, "pro %d is no prologue of the SIMD mat-vec (0 PLAIN, 1 LN)", pro);
    if (epi < bgk::EPI_QKV || epi > bgk::EPI_LOGITS) BG_FAIL(-1, "epi %d is no epilogue of the SIMD mat-vec (0 QKV, 1 RESID, 2 GELU, 3 LOGITS)", epi);
    const bool forms_ok = (pro == bgk::PRO_LN && epi != bgk::EPI_RESID) || (pro == bgk::PRO_PLAIN && epi == bgk::EPI_RESID);
    if (!forms_ok) BG_FAIL(-1, "pro %d with epi %d is no site of the layer (LN -> QKV, PLAIN -> RESID, LN -> GELU, LN -> LOGITS)", pro, epi);
    if ((pro == bgk::PRO_LN) != (ln_w != nullptr)) BG_FAIL(-1, "ln_w and ln_b go with pro 1 (LN) and only with it");
    if (M < 1 || M > (1 << 20)) BG_FAIL(-1, "M must be in [1, %d]", 1 << 20);
    if (epi == bgk::EPI_QKV && (K % 64 != 0 || M != 3 * K)) BG_FAIL(-1, "q/k/v is 3 K x K with heads of 64 (got %d x %d)", M, K);
    if (!w_rows || !out) BG_FAIL(-1, "w_rows or out is NULL");
    if (epi != bgk::EPI_LOGITS && !bias) BG_FAIL(-1, "bias is NULL");
    if (epi == bgk::EPI_RESID && !resid) BG_FAIL(-1, "resid is NULL");
    if ((pmax_val != nullptr) != (pmax_idx != nullptr)) BG_FAIL(-1, "pmax_val and pmax_idx come together");
    if (pmax_val && (epi != bgk::EPI_LOGITS || N != 1)) BG_FAIL(-1, "the arg-max partials are the LOGITS epilogue's, of one column");
    const bool qkv = epi == bgk::EPI_QKV;
    if (!check_probe_columns(__func__, qkv, N, dev_state, nullptr, 0, P, 1, k_slots, v_slots)) return -1;
    if (bgk::matvec_simd_smem_bytes(K, 1) > 64 * 1024) BG_FAIL(-1, "a column of K = %d values exceeds the kernel's LDS", K);
    HIP_TRY(-2, hipSetDevice(device));
    const int cols = N + 1, ldo = M + 16;
    const size_t kv_b = qkv ? (size_t)(K / 64) * P * 64 * 4 : 0, part_b = (size_t)(MATVEC_MAX_GRID + 1) * 4;
    ProbeImage im;      // [weights | x | gain | bias of the LayerNorm | the stage's parts | out | partials], guard column and rows in the output
    const BlockRows wr = upload_block_rows(im, wtype, w_rows, M, K, false);
    const ProbePart o_x = im.in(x, (size_t)N * K * 4), o_lw = im.in(ln_w, (size_t)K * 4), o_lb = im.in(ln_b, (size_t)K * 4);
    const StageParts sp = stage_parts(im, bias, (size_t)M * 4, epi == bgk::EPI_RESID ? resid : nullptr, (size_t)N * M * 4, dev_state, nullptr, N, k_slots, v_slots, kv_b);
    const ProbePart o_out = im.out((size_t)cols * (qkv ? K : ldo) * 4), o_pv = im.out(pmax_val ? part_b : 0), o_pi = im.out(pmax_val ? part_b : 0);
    if (!im.upload()) return -2;
    bgk::MatvecParams p = stage_params(im, wr.W(im), sp, K, P, N, qkv, 0, o_out, ldo, M);
    p.x = im.at<const float>(o_x); p.ldx = K;
    if (ln_w) { p.ln_w = im.at<const float>(o_lw); p.ln_b = im.at<const float>(o_lb); }
    if (pmax_val) { p.pmax_val = im.at<float>(o_pv); p.pmax_idx = im.at<int32_t>(o_pi); }
    SimdLaunch g{};
    hipError_t e = hipErrorInvalidValue;
    if (epi == bgk::EPI_QKV) e = launch_mv_simd<bgk::PRO_LN, bgk::EPI_QKV>(p, 0, nullptr, &g);
    else if (epi == bgk::EPI_RESID) e = launch_mv_simd<bgk::PRO_PLAIN, bgk::EPI_RESID>(p, 0, nullptr, &g);
    else if (epi == bgk::EPI_GELU) e = launch_mv_simd<bgk::PRO_LN, bgk::EPI_GELU>(p, 0, nullptr, &g);
    else e = launch_mv_simd<bgk::PRO_LN, bgk::EPI_LOGITS>(p, 0, nullptr, &g);
    HIP_TRY(-2, e);
    HIP_TRY(-2, hipDeviceSynchronize());
    report_launch(launched, {g.threads, g.grid_x, g.grid_y, g.lds, g.nc, g.rows});
    if (!im.read(o_out, out) || !im.read(sp.k, k_slots) || !im.read(sp.v, v_slots)) return -2;
    if (pmax_val && (!im.read(o_pv, pmax_val) || !im.read(o_pi, pmax_idx))) return -2;
    return 0;
}

// A kernel of the SIMD association alone, timed: one untimed launch, then reps launches on device memory of 0x11 bytes (the kernels' time does not depend on the
// values), each between two device events.  which 0: matvec_simd_kernel<PLAIN, RESID> at M rows of K values and N columns (any N: the launch's own grid);
// which 1: the mat-vec a context in the scalar association launches at the same shape on its five-launch route (launch_mv<PLAIN, RESID>) -- the yardstick;
// which 2: attn_simd_kernel with M heads, K visible keys (1 .. 1024) and N query columns.  For tools/assoc_bench.py.
int biogpt_hip_assoc_bench(int device, int32_t which, int32_t wtype, int32_t M, int32_t K, int32_t N, int32_t reps, float *us_out) {
    clear_error();
    if (which < 0 || which > 2) BG_FAIL(-1, "which must be 0 (the SIMD mat-vec), 1 (the scalar association's mat-vec) or 2 (the SIMD attention)");
    if (N < 1 || N > 512) BG_FAIL(-1, "N must be in [1, 512]");
    if (reps < 1 || reps > PROBE_MAX_REPS) BG_FAIL(-1, "reps must be in [1, %d]", PROBE_MAX_REPS);
    if (!us_out) BG_FAIL(-1, "us_out is NULL");
    if (which == 2) {
        if (M < 1 || M > 64) BG_FAIL(-1, "M (heads) must be in [1, 64]");
        if (K < N || K > bgk::SIMD_ATTN_MAXT) BG_FAIL(-1, "K (visible keys of the last column) must be in [N, %d]", bgk::SIMD_ATTN_MAXT);
        HIP_TRY(-2, hipSetDevice(device));
        const size_t D = (size_t)M * 64, kv_b = (size_t)M * K * 64 * 4;
        const int32_t ds[4] = {K - N, 0, 1, 0};      // causal: column N - 1 sees K keys, the others fewer
        ProbeImage im;
        const ProbePart o_k = im.fill(kv_b, 0x11), o_v = im.fill(kv_b, 0x11), o_q = im.fill((size_t)N * D * 4, 0x11), o_ds = im.in(ds, sizeof(ds));
        const ProbePart o_tab = im.own(exp_table_f16()), o_out = im.fill((size_t)N * D * 4, 0x11);
        if (!im.upload()) return -2;
        bgk::AttnParams a{};
        a.q = im.at<const float>(o_q); a.kcache = im.at<const float>(o_k); a.vcache = im.at<const float>(o_v); a.out = im.at<float>(o_out);
        a.st = im.at<const bgk::DevState>(o_ds); a.exp_tab = im.at<const uint16_t>(o_tab);
        a.N = N; a.D = (int32_t)D; a.dk = 64; a.P = K;
        auto launch = [&]() -> hipError_t { launch_attn_simd(a, M, N, 0); return hipGetLastError(); };
        HIP_TRY(-2, launch());
        HIP_TRY(-2, hipDeviceSynchronize());
        return time_launches(reps, nullptr, launch, [&](int i, float ms) { us_out[i] = ms * 1e3f; });
    }
    if (wtype != T_Q4_0 && wtype != T_Q4_1 && wtype != T_Q5_0 && wtype != T_Q5_1 && wtype != T_Q8_0) BG_FAIL(-1, "type %d is no block format", wtype);
    if (K < QK || K > (1 << 16) || K % QK != 0) BG_FAIL(-1, "K must be a multiple of %d in [%d, %d]", QK, QK, 1 << 16);
    if (M < 1 || M > (1 << 20)) BG_FAIL(-1, "M must be in [1, %d]", 1 << 20);
    if (bgk::matvec_simd_smem_bytes(K, 1) > 64 * 1024) BG_FAIL(-1, "a column of K = %d values exceeds the kernel's LDS", K);
    HIP_TRY(-2, hipSetDevice(device));
    ProbeImage im;      // every part of 0x11 bytes: [qs | sc | qh | x | bias | resid | out]
    const size_t nblk = (size_t)M * (K / QK);
    const bool q81 = wtype == T_Q4_1 || wtype == T_Q5_1, q5 = wtype == T_Q5_0 || wtype == T_Q5_1;
    const ProbePart o_qs = im.fill(nblk * (wtype == T_Q8_0 ? 32 : 16), 0x11), o_sc = im.fill(nblk * (q81 ? 4 : 2) + 16, 0x11), o_qh = im.fill(q5 ? nblk * 4 : 0, 0x11);
    const ProbePart o_x = im.fill((size_t)N * K * 4, 0x11), o_bias = im.fill((size_t)M * 4, 0x11), o_res = im.fill((size_t)N * M * 4, 0x11), o_out = im.fill((size_t)N * M * 4, 0x11);
    if (!im.upload()) return -2;
    const MvShape s = mv_shape(wtype, M, K);
    bgk::MatvecParams p{};
    p.W.qs = im.d.p + o_qs.off; p.W.sc = im.d.p + o_sc.off; p.W.qh = q5 ? im.at<const uint32_t>(o_qh) : nullptr;
    p.W.type = wtype; p.W.M = M; p.W.K = K;
    p.upr = s.upr; p.lpr_log2 = s.lpr_log2; p.nit = s.nit; p.rpw = s.rpw;
    p.eps = 1e-5f; p.D = 1024; p.dk = 64; p.dk_log2 = 6; p.P = 1;
    p.inv_k = 1.0 / (double)K; p.k_pow2 = (K & (K - 1)) == 0;
    p.N = N; p.x = im.at<const float>(o_x); p.ldx = K;
    p.bias = im.at<const float>(o_bias); p.resid = im.at<const float>(o_res); p.ldr = M; p.out = im.at<float>(o_out); p.ldo = M;
    EngineOptions opt{};
    opt.load();
    auto launch = [&]() -> hipError_t {
        if (which == 0) return launch_mv_simd<bgk::PRO_PLAIN, bgk::EPI_RESID>(p, 0);
        return launch_mv<bgk::PRO_PLAIN, bgk::EPI_RESID>(opt, p, s, 0);
    };
    HIP_TRY(-2, launch());      // one untimed launch in front
    HIP_TRY(-2, hipDeviceSynchronize());
    return time_launches(reps, nullptr, launch, [&](int i, float ms) { us_out[i] = ms * 1e3f; });
}

// ---- the kernels of the SIMD chain alone (kernels_schain.hip.h), through the launch functions PassLaunch::simd_stage and enqueue_attention use ----
// stage 0 Q8: the producer (bg_schain_q8) over x [N][K], behind the LayerNorm when ln_w / ln_b are given: out_q [N + 1][K] codes, out_d [N + 1][K / 32] the
//   scale the dot reads (through f16 for the Q8_0 form), out_s [N + 1][K / 32] words.  wtype names the weight format whose activation form it is.
// stage 1 STAGE: the producer, then one launch of schain_kernel<wtype, epi> (bg_schain_launch) at tile shape cfg (0 .. 2; -1: the launch's own choice) -- a
//   linear stage as a pass enqueues it.  epi 0 QKV (M == 3 K, 64 | K; exactly one of dev_state and seq_states (+ col_mode) names the column states; k_slots /
//   v_slots [n_slots][K / 64][P][64], updated in place; out = the q rows [cols][K]), 1 RESID (bias, resid [N][M]), 2 GELU (bias), 3 LOGITS; any M.  out but for
//   QKV: [cols][ldo]; cols = N rounded up to 32, plus one guard column; ldo = M rounded up to 64, plus 16 guard rows.
// stage 2 ATTN: attn_simd_cols_kernel (bg_schain_attn) over q [N][H * 64], k_slots / v_slots [n_slots][H][P][64] and seq_states [N]: column i reads slot i
//   (col_mode 0, n_past + 1 keys) or slot seq_id (col_mode 1, t_vis keys); shared 1: its rows j < pad[0] come from slot pad[1].  out [N + 1][H * 64].
// The outputs come back WHOLE as allocated and preset to 0xff bytes.  launched [8]: stage 0 / 2: threads, grid x, grid y, LDS bytes; stage 1: threads, grid x,
// grid y, static LDS bytes, cols, ldo, cfg, columns of a tile.  Every refusal comes before any HIP call.
int biogpt_hip_schain_device(int device, int32_t stage, int32_t wtype, int32_t epi, int32_t M, int32_t K, int32_t N, int32_t cfg, int32_t H, int32_t P, int32_t n_slots,
                             int32_t col_mode, int32_t shared, const void *w_rows, const float *x, const float *ln_w, const float *ln_b, const float *bias,
                             const float *resid, const int32_t *dev_state, const int32_t *seq_states, const float *q, float *k_slots, float *v_slots, float *out,
                             int8_t *out_q, float *out_d, uint32_t *out_s, int32_t *launched) {
    clear_error();
    if (stage < 0 || stage > 2) BG_FAIL(-1, "stage %d is no stage (0 Q8, 1 STAGE, 2 ATTN)", stage);
    if (N < 1 || N > 512) BG_FAIL(-1, "N must be in [1, 512]");
    if (stage == 2) {
        if (H < 1 || H > 64) BG_FAIL(-1, "H must be in [1, 64]");
        if (P < 1 || P > 8192) BG_FAIL(-1, "P must be in [1, 8192]");
        if (n_slots < 1 || n_slots > 1024) BG_FAIL(-1, "n_slots must be in [1, 1024]");
        if (col_mode != 0 && col_mode != 1) BG_FAIL(-1, "col_mode must be 0 or 1");
        if (shared != 0 && shared != 1) BG_FAIL(-1, "shared must be 0 or 1");
        if (!q || !k_slots || !v_slots || !seq_states || !out) BG_FAIL(-1, "q, k_slots, v_slots, seq_states or out is NULL");
        const bgk::SeqState *hs = reinterpret_cast<const bgk::SeqState *>(seq_states);
        for (int i = 0; i < N; i++) {
            const int T = col_mode ? hs[i].t_vis : hs[i].n_past + 1;
            if (T < 1 || T > bgk::SIMD_ATTN_MAXT) BG_FAIL(-1, "column %d sees T = %d keys: the kernel holds 1 .. %d", i, T, bgk::SIMD_ATTN_MAXT);
            if (T > P) BG_FAIL(-1, "column %d sees %d keys of a table of P = %d rows", i, T, P);
            if (!probe_slot_ok(__func__, i, col_mode ? hs[i].seq_id : i, n_slots)) return -1;
            if (shared && (hs[i].pad[0] < 0 || hs[i].pad[0] > P)) BG_FAIL(-1, "column %d: %d shared rows outside [0, P]", i, hs[i].pad[0]);
            if (shared && (hs[i].pad[1] < 0 || hs[i].pad[1] >= n_slots)) BG_FAIL(-1, "column %d: shared slot %d outside [0, n_slots)", i, hs[i].pad[1]);
        }
        HIP_TRY(-2, hipSetDevice(device));
        const size_t D = (size_t)H * 64, kv_b = (size_t)n_slots * H * P * 64 * 4;
        ProbeImage im;      // [K | V | q | column states | exp table | out], one guard row
        const ProbePart o_k = im.in(k_slots, kv_b), o_v = im.in(v_slots, kv_b), o_q = im.in(q, (size_t)N * D * 4), o_st = im.in(seq_states, sizeof(bgk::SeqState) * (size_t)N);
        const ProbePart o_ds = im.in(PROBE_NO_STATE, sizeof(bgk::DevState)), o_tab = im.own(exp_table_f16()), o_out = im.out((size_t)(N + 1) * D * 4);
        if (!im.upload()) return -2;
        bgk::AttnParams a{};
        a.q = im.at<const float>(o_q); a.kcache = im.at<const float>(o_k); a.vcache = im.at<const float>(o_v); a.out = im.at<float>(o_out);
        a.st = im.at<const bgk::DevState>(o_ds); a.exp_tab = im.at<const uint16_t>(o_tab);
        a.seq = im.at<const bgk::SeqState>(o_st); a.col_mode = col_mode; a.kv_seq_stride = (int64_t)H * P * 64;
        a.N = N; a.D = (int32_t)D; a.dk = 64; a.P = P;
        int32_t four[4] = {0, 0, 0, 0};
        HIP_TRY(-2, (hipError_t)bg_schain_attn(&a, sizeof(a), shared, H, N, 0, four));
        HIP_TRY(-2, hipDeviceSynchronize());
        report_launch(launched, {four[0], four[1], four[2], four[3]});
        return im.read(o_out, out) ? 0 : -2;
    }
    if (wtype != T_Q4_0 && wtype != T_Q4_1 && wtype != T_Q5_0 && wtype != T_Q5_1 && wtype != T_Q8_0) BG_FAIL(-1, "type %d is no block format", wtype);
    if (K < QK || K > (1 << 16) || K % QK != 0) BG_FAIL(-1, "K must be a multiple of %d in [%d, %d]", QK, QK, 1 << 16);
    if (!x) BG_FAIL(-1, "x is NULL");
    if ((ln_w != nullptr) != (ln_b != nullptr)) BG_FAIL(-1, "ln_w and ln_b come together");
    const int q81 = (wtype == T_Q4_1 || wtype == T_Q5_1) ? 1 : 0;
    const size_t bpr = (size_t)K / QK;
    if (stage == 0) {
        if (!out_q || !out_d || !out_s) BG_FAIL(-1, "out_q, out_d or out_s is NULL");
        HIP_TRY(-2, hipSetDevice(device));
        ProbeImage im;      // [x | gain | bias of the LayerNorm | codes | d | s], one guard row each
        const ProbePart o_x = im.in(x, (size_t)N * K * 4), o_lw = im.in(ln_w, (size_t)K * 4), o_lb = im.in(ln_b, (size_t)K * 4);
        const ProbePart o_q = im.out((size_t)(N + 1) * K), o_d = im.out((size_t)(N + 1) * bpr * 4), o_s = im.out((size_t)(N + 1) * bpr * 4);
        if (!im.upload()) return -2;
        int32_t four[4] = {0, 0, 0, 0};
        HIP_TRY(-2, (hipError_t)bg_schain_q8(q81, im.at<const float>(o_x), K, K, N, ln_w ? im.at<const float>(o_lw) : nullptr, ln_w ? im.at<const float>(o_lb) : nullptr, 1e-5f,
                                             im.at<int8_t>(o_q), im.at<float>(o_d), im.at<uint32_t>(o_s), 0, four));
        HIP_TRY(-2, hipDeviceSynchronize());
        report_launch(launched, {four[0], four[1], four[2], four[3]});
        return im.read(o_q, out_q) && im.read(o_d, out_d) && im.read(o_s, out_s) ? 0 : -2;
    }
    // stage 1
    if (epi < bgk::EPI_QKV || epi > bgk::EPI_LOGITS) BG_FAIL(-1, "epi %d is no epilogue of the SIMD chain (0 QKV, 1 RESID, 2 GELU, 3 LOGITS)", epi);
    if (cfg < -1 || cfg > 2) BG_FAIL(-1, "cfg must be in [-1, 2]");
    if (M < 1 || M > (1 << 20)) BG_FAIL(-1, "M must be in [1, %d]", 1 << 20);
    if (epi == bgk::EPI_QKV && (K % 64 != 0 || M != 3 * K)) BG_FAIL(-1, "q/k/v is 3 K x K with heads of 64 (got %d x %d)", M, K);
    if (!w_rows || !out) BG_FAIL(-1, "w_rows or out is NULL");
    if (epi != bgk::EPI_LOGITS && !bias) BG_FAIL(-1, "bias is NULL");
    if (epi == bgk::EPI_RESID && !resid) BG_FAIL(-1, "resid is NULL");
    const bool qkv = epi == bgk::EPI_QKV;
    if (!check_probe_columns(__func__, qkv, N, dev_state, seq_states, col_mode, P, n_slots, k_slots, v_slots)) return -1;
    HIP_TRY(-2, hipSetDevice(device));
    const int cols = ((N + 31) & ~31) + 1, ldo = ((M + 63) & ~63) + 16;
    const size_t kv_b = qkv ? (size_t)(K / 64) * P * 64 * 4 * (size_t)n_slots : 0;
    ProbeImage im;      // [weights | x | gain | bias of the LayerNorm | the stage's parts | the producer's rows | out], guard column and rows in the output
    const BlockRows wr = upload_block_rows(im, wtype, w_rows, M, K, false);
    const ProbePart o_x = im.in(x, (size_t)N * K * 4), o_lw = im.in(ln_w, (size_t)K * 4), o_lb = im.in(ln_b, (size_t)K * 4);
    const StageParts sp = stage_parts(im, bias, (size_t)M * 4, epi == bgk::EPI_RESID ? resid : nullptr, (size_t)N * M * 4, dev_state, seq_states, N, k_slots, v_slots, kv_b);
    const ProbePart o_q = im.fill((size_t)N * K), o_d = im.fill((size_t)N * bpr * 4), o_s = im.fill((size_t)N * bpr * 4);
    const ProbePart o_out = im.out((size_t)cols * (qkv ? K : ldo) * 4);
    if (!im.upload()) return -2;
    bgk::MatvecParams p = stage_params(im, wr.W(im), sp, K, P, N, qkv, col_mode, o_out, ldo, M);
    HIP_TRY(-2, (hipError_t)bg_schain_q8(q81, im.at<const float>(o_x), K, K, N, ln_w ? im.at<const float>(o_lw) : nullptr, ln_w ? im.at<const float>(o_lb) : nullptr, 1e-5f,
                                         im.at<int8_t>(o_q), im.at<float>(o_d), im.at<uint32_t>(o_s), 0, nullptr));
    p.aq_q = im.at<const int8_t>(o_q); p.aq_d = im.at<const float>(o_d); p.aq_s = im.at<const uint32_t>(o_s);
    int32_t five[5] = {0, 0, 0, 0, 0};
    HIP_TRY(-2, (hipError_t)bg_schain_launch(wtype, epi, &p, sizeof(p), cfg, 0, five));
    HIP_TRY(-2, hipDeviceSynchronize());
    report_launch(launched, {five[0], five[1], five[2], five[3], cols, ldo, five[4], 4 << (five[4] == 0 ? 0 : five[4] + 1)});
    if (!im.read(o_out, out) || !im.read(sp.k, k_slots) || !im.read(sp.v, v_slots)) return -2;
    return 0;
}

// A linear stage of the SIMD association alone, timed: one untimed launch, then reps launches on device memory of 0x11 bytes (the kernels' time does not depend
// on the values), each between two device events.  which 0: schain_kernel with the residual epilogue at tile shape cfg (-1: the launch's choice) on rows a
// producer launch made in front of the timing; which 1: the producer alone; which 2: matvec_simd_kernel<PLAIN, RESID> as a context's own pass in mode 1
// launches it at N columns (its own grid) -- the yardstick at N = 8; which 3: the wide chain's matrix-core stage of the scalar association, for scale only.
// For tools/simd_chain_bench.py.
int biogpt_hip_schain_bench(int device, int32_t which, int32_t wtype, int32_t M, int32_t K, int32_t N, int32_t cfg, int32_t reps, float *us_out) {
    clear_error();
    if (which < 0 || which > 3) BG_FAIL(-1, "which must be 0 (the SIMD chain's stage), 1 (its producer), 2 (the SIMD mat-vec) or 3 (the wide chain's stage)");
    if (which == 3) return biogpt_hip_wide_chain_bench(device, 0, wtype, M, K, N, reps, us_out);
    if (wtype != T_Q4_0 && wtype != T_Q4_1 && wtype != T_Q5_0 && wtype != T_Q5_1 && wtype != T_Q8_0) BG_FAIL(-1, "type %d is no block format", wtype);
    if (cfg < -1 || cfg > 2) BG_FAIL(-1, "cfg must be in [-1, 2]");
    if (N < 1 || N > 512) BG_FAIL(-1, "N must be in [1, 512]");
    if (K < QK || K > (1 << 16) || K % QK != 0) BG_FAIL(-1, "K must be a multiple of %d in [%d, %d]", QK, QK, 1 << 16);
    if (M < 1 || M > (1 << 20)) BG_FAIL(-1, "M must be in [1, %d]", 1 << 20);
    if (reps < 1 || reps > PROBE_MAX_REPS) BG_FAIL(-1, "reps must be in [1, %d]", PROBE_MAX_REPS);
    if (!us_out) BG_FAIL(-1, "us_out is NULL");
    if (which == 2 && bgk::matvec_simd_smem_bytes(K, 1) > 64 * 1024) BG_FAIL(-1, "a column of K = %d values exceeds the SIMD mat-vec's LDS", K);
    HIP_TRY(-2, hipSetDevice(device));
    ProbeImage im;      // every part of 0x11 bytes: [qs | sc | qh | x | bias | resid | codes | d | s | out]
    const size_t nblk = (size_t)M * (K / QK), bpr = (size_t)K / QK;
    const bool q81 = wtype == T_Q4_1 || wtype == T_Q5_1, q5 = wtype == T_Q5_0 || wtype == T_Q5_1;
    const ProbePart o_qs = im.fill(nblk * (wtype == T_Q8_0 ? 32 : 16), 0x11), o_sc = im.fill(nblk * (q81 ? 4 : 2) + 16, 0x11), o_qh = im.fill(q5 ? nblk * 4 : 0, 0x11);
    const ProbePart o_x = im.fill((size_t)N * K * 4, 0x11), o_bias = im.fill((size_t)M * 4, 0x11), o_res = im.fill((size_t)N * M * 4, 0x11);
    const ProbePart o_q = im.fill((size_t)N * K, 0x11), o_d = im.fill((size_t)N * bpr * 4, 0x11), o_s = im.fill((size_t)N * bpr * 4, 0x11), o_out = im.fill((size_t)N * M * 4, 0x11);
    if (!im.upload()) return -2;
    const MvShape s = mv_shape(wtype, M, K);
    bgk::MatvecParams p{};
    p.W.qs = im.d.p + o_qs.off; p.W.sc = im.d.p + o_sc.off; p.W.qh = q5 ? im.at<const uint32_t>(o_qh) : nullptr;
    p.W.type = wtype; p.W.M = M; p.W.K = K;
    p.upr = s.upr; p.lpr_log2 = s.lpr_log2; p.nit = s.nit; p.rpw = s.rpw;
    p.eps = 1e-5f; p.D = 1024; p.dk = 64; p.dk_log2 = 6; p.P = 1;
    p.inv_k = 1.0 / (double)K; p.k_pow2 = (K & (K - 1)) == 0;
    p.N = N; p.x = im.at<const float>(o_x); p.ldx = K;
    p.bias = im.at<const float>(o_bias); p.resid = im.at<const float>(o_res); p.ldr = M; p.out = im.at<float>(o_out); p.ldo = M;
    p.aq_q = im.at<const int8_t>(o_q); p.aq_d = im.at<const float>(o_d); p.aq_s = im.at<const uint32_t>(o_s);
    auto produce = [&]() -> hipError_t {
        return (hipError_t)bg_schain_q8(q81 ? 1 : 0, p.x, K, K, N, nullptr, nullptr, 1e-5f, im.at<int8_t>(o_q), im.at<float>(o_d), im.at<uint32_t>(o_s), 0, nullptr);
    };
    auto launch = [&]() -> hipError_t {
        if (which == 0) return (hipError_t)bg_schain_launch(wtype, bgk::EPI_RESID, &p, sizeof(p), cfg, 0, nullptr);
        if (which == 1) return produce();
        return launch_mv_simd<bgk::PRO_PLAIN, bgk::EPI_RESID>(p, 0);
    };
    HIP_TRY(-2, produce());
    HIP_TRY(-2, launch());      // one untimed launch in front
    HIP_TRY(-2, hipDeviceSynchronize());
    return time_launches(reps, nullptr, launch, [&](int i, float ms) { us_out[i] = ms * 1e3f; });
}
