// Part of engine.hip (textually included there: same translation unit, same anonymous namespace / extern "C" block): the host side of the XCD-pipelined decode launches -- the per-device pipeline slot, device probe, layer table, hand-off regions and their calibration (xpipe_place_hops), tables kept in LDS, error check.

// ---- XCD-pipelined decode step (kernels_xpipe.hip.h): one persistent launch for all layers ------------------------
// Two such launches of different contexts on one device could each hold part of the compute units and wait for the rest
// (their workgroups only leave when their pipeline has run), so one context per device holds the path at a time: the slot is
// taken when a pipelined launch (or a graph holding one) is about to be enqueued and handed back whenever the holder's stream
// is known to be idle (every synchronising API call ends in xpipe_check).  A context that finds the slot taken runs that call on
// the five-launch layer.  The slot table is the ONE piece of process-global state of this library; it serialises contexts of
// this process only.  Two PROCESSES on one device are kept apart one level up: the contexts of a process may use the pipeline only while the process holds an advisory
// lock on a per-device file (xpipe_process_lock); a process that finds it taken runs the five-launch layer from the start (INTEGRATION.md section 4).
std::mutex g_xp_mu;
biogpt_hip_ctx *g_xp_owner[64] = {};
int g_xp_lock_fd[64] = {};         // per device: 0 not held, > 0 the lock file's descriptor + 1, -1 no lock file could be opened (no coordination: round 4's behaviour)
int g_xp_lock_refs[64] = {};       // contexts of this process that rely on it
pid_t g_xp_lock_pid[64] = {};      // the process that took it: a fork()ed child inherits the descriptor (and the table), not the right to the pipeline

// Persistent launches of two processes on one device would each hold part of the compute units and wait for the rest (0.3 s spin bounds, both contexts on the
// five-launch layer for good).  The first process that prepares a pipelined context on a device takes flock(LOCK_EX) on /dev/shm/biogpt_hip_<pci bus id>.lock (or /tmp)
// and keeps it while it has such contexts; the operating system drops it when the process ends, however it ends.  BIOGPT_HIP_PROC_LOCK=0: no lock.
bool xpipe_process_lock(biogpt_hip_ctx *c) {
    if (c->device < 0 || c->device >= 64 || !c->opt.proc_lock) return true;
    std::lock_guard<std::mutex> lk(g_xp_mu);
    int &fd1 = g_xp_lock_fd[c->device];
    if (fd1 != 0 && g_xp_lock_pid[c->device] != getpid()) {      // after fork(): the parent's lock (one open file description, shared) is not this process's -- ask again
        if (fd1 > 0) (void)close(fd1 - 1);                       // (closing the child's copy does not release the parent's lock)
        fd1 = 0; g_xp_lock_refs[c->device] = 0;
    }
    if (fd1 == 0) {
        g_xp_lock_pid[c->device] = getpid();
        char bus[64] = {0};
        if (hipDeviceGetPCIBusId(bus, (int)sizeof(bus) - 1, c->device) != hipSuccess) { (void)hipGetLastError(); snprintf(bus, sizeof(bus), "device%d", c->device); }
        for (char *q = bus; *q; q++) if (!((*q >= '0' && *q <= '9') || (*q >= 'a' && *q <= 'z') || (*q >= 'A' && *q <= 'Z'))) *q = '_';
        const std::string path = std::string(access("/dev/shm", W_OK) == 0 ? "/dev/shm" : "/tmp") + "/biogpt_hip_" + bus + ".lock";
        // (read-only is enough for flock: a file another user created under umask 022 still opens; O_NOFOLLOW: a symbolic link planted under the name is refused -- the
        //  lock is advisory and the directory world-writable: any local user can hold it and keep others on the five-launch layer, never worse; INTEGRATION.md section 4)
        const int fd = open(path.c_str(), O_CREAT | O_RDONLY | O_CLOEXEC | O_NOFOLLOW, 0666);
        if (fd < 0) fd1 = -1;
        else if (flock(fd, LOCK_EX | LOCK_NB) == 0) fd1 = fd + 1;
        else {
            (void)close(fd);
            c->xp_foreign = true;      // another PROCESS may have persistent launches on this device: this context's captured five-launch steps are not replayed beside them (plain_graph_begin)
            if (c->opt.verbose) fprintf(stderr, "biogpt_hip: another process drives the XCD-pipelined launches on this device (%s); this context uses the five-launch layer\n", path.c_str());
            return false;
        }
    }
    if (fd1 > 0) g_xp_lock_refs[c->device]++;
    c->xp_proc_ref = fd1 > 0;
    return true;
}
void xpipe_process_unlock(biogpt_hip_ctx *c) {
    if (!c->xp_proc_ref || c->device < 0 || c->device >= 64) return;
    std::lock_guard<std::mutex> lk(g_xp_mu);
    c->xp_proc_ref = false;
    if (--g_xp_lock_refs[c->device] <= 0 && g_xp_lock_fd[c->device] > 0) {      // the last pipelined context of this process on the device: another process may have the path
        (void)close(g_xp_lock_fd[c->device] - 1);
        g_xp_lock_fd[c->device] = 0; g_xp_lock_refs[c->device] = 0;
    }
}
std::vector<biogpt_hip_ctx *> g_xp_plain[64];      // per device: contexts whose captured five-launch steps may be in flight (plain_graph_begin)

void xpipe_release(biogpt_hip_ctx *c) {
    xpipe_process_unlock(c);
    {
        std::lock_guard<std::mutex> lk(g_xp_mu);
        if (c->device >= 0 && c->device < 64 && g_xp_owner[c->device] == c) g_xp_owner[c->device] = nullptr;
    }
    if (c->fp_layers) (void)hipFree(c->fp_layers);
    if (c->fp_gran) (void)hipFree(c->fp_gran);
    if (c->fp_ctl) (void)hipFree(c->fp_ctl);
    c->fp_layers = nullptr; c->fp_gran = nullptr; c->fp_ctl = nullptr; c->fp_state = -1;
    if (c->xp_layers) (void)hipFree(c->xp_layers);
    if (c->xp_gran) (void)hipFree(c->xp_gran);
    if (c->xp_gran_l) (void)hipFree(c->xp_gran_l);
    if (c->xc_gran) (void)hipFree(c->xc_gran);
    c->xc_gran = nullptr; c->xc_lds = 0;
    if (c->xp_hop) (void)hipFree(c->xp_hop);
    if (c->xp_ctl) (void)hipFree(c->xp_ctl);
    if (c->xp_samp) (void)hipFree(c->xp_samp);
    if (c->xp_err_host) (void)hipHostFree(c->xp_err_host);
    if (c->res_mbox) (void)hipHostFree(c->res_mbox);
    if (c->res_done) (void)hipHostFree(c->res_done);
    c->res_mbox = nullptr; c->res_done = nullptr;
    c->xp_layers = nullptr; c->xp_gran = nullptr; c->xp_gran_l = nullptr; c->xp_hop = nullptr; c->xp_ctl = nullptr; c->xp_samp = nullptr; c->xp_err_host = nullptr;
}

bool xpipe_model_ok(const biogpt_hip_ctx *c) {
    const auto &hp = c->hp;
    const int32_t wt = ftype_to_type(hp.ftype);
    return (wt == T_Q4_0 || wt == T_Q4_1 || wt == T_Q5_0 || wt == T_Q5_1 || wt == T_Q8_0) && hp.d_model == 1024 && hp.d_ff == 4096 && hp.n_head == 16 &&
           hp.n_positions >= 64 && hp.n_layer >= 1;
}

// the pipelined kernels live in their own translation unit (xpipe_tu.hip)
extern "C" int bg_xpipe_launch(int wt, int t_cap, size_t smem_bytes, hipStream_t st, const void *params, size_t params_bytes);
extern "C" int bg_xpipe_set_lds(int wt, size_t smem_bytes);

// pipeline units of the model: half layers (attention half on an even XCD, MLP half on the next, odd one); the XCD of the last one (and XCD 0)
// computes no lm_head rows
int xpipe_last_xcd(const biogpt_hip_ctx *c) {
    const int units = 2 * c->hp.n_layer;
    return (units - 1) & 7;
}
// > 64 KB of dynamic LDS needs the opt-in attribute (per device); set outside any stream capture
bool xpipe_set_lds(biogpt_hip_ctx *c) {
    const size_t sm = bgk::xpipe_smem_bytes(c->xp_gelu_p + c->xp_gelu_n);
    if (sm <= 64 * 1024) return true;
    return bg_xpipe_set_lds(ftype_to_type(c->hp.ftype), sm) == (int)hipSuccess;     // T_* values are the kernels' WType values
}

// Where the two cross-XCD hand-offs of every layer live (XpLayer::gx1, gx).  Device memory is interleaved over the two halves of the chip in 8 KB units
// (tools/microbench18.hip, profiles/microbench18_hop_by_address_r4.txt): a granule written on XCD a and polled on XCD b takes 0.40 us when its line is near both,
// 0.60 us when it is far from both, 0.50 us across the halves whatever the line.  Every region therefore has TWO 8 KB-aligned candidates (neighbours: one of each
// kind) and a calibration launch plays ping-pong over both between the XCDs of ITS hop (bgk::xp_hop_probe_kernel: the stores and polls of the real hand-off);
// the faster one is used.  mode (BIOGPT_HIP_HOP_PLACE): 1 calibrated (default), 0 always the first candidate, 2 the slower one (A/B).
bool xpipe_place_hops(biogpt_hip_ctx *c, std::vector<bgk::XpLayer> &tab) {
    const int nl = c->hp.n_layer, mode = c->opt.hop_place;
    const size_t region = 1024, bytes = (size_t)nl * 4 * region * 8 + 16384;      // [layer][x1, x][candidate][1024 granules], 16 KB-aligned
    if (hipMalloc(&c->xp_hop, bytes) != hipSuccess || hipMemset(c->xp_hop, 0, bytes) != hipSuccess) return false;
    bgk::xp_u64 *base = reinterpret_cast<bgk::xp_u64 *>((reinterpret_cast<uintptr_t>(c->xp_hop) + 16383) & ~(uintptr_t)16383);
    auto cand = [&](int l, int which, int k) { return base + ((size_t)(l * 2 + which) * 2 + k) * region; };
    std::vector<int> pick((size_t)nl * 2, 0);
    if (mode != 0) {
        std::vector<bgk::XpProbe> pr;
        for (int l = 0; l < nl; l++)
            for (int which = 0; which < 2; which++) {
                const int src = (2 * l + which) & 7;      // x1: unit 2 l -> 2 l + 1; x: unit 2 l + 1 -> 2 l + 2
                // the last layer's output goes to every XCD that computes lm_head rows: readers in BOTH halves of the chip -- near the producer's half costs the far readers
                // 0.5 us and the near ones 0.4, near the other half 0.5 and 0.6: judged by a hop that stays in the producer's half
                const int dst = (l == nl - 1 && which == 1) ? (src ^ 1) : ((src + 1) & 7);
                for (int k = 0; k < 2; k++)
                    for (int line = 0; line < 2; line++) pr.push_back({cand(l, which, k) + (line ? 512 + 130 : 2), src, dst});
            }
        bgk::XpProbe *d_pr = nullptr;
        uint32_t *d_ctl = nullptr;
        unsigned long long *d_ticks = nullptr;
        const int reps = 12;
        std::vector<unsigned long long> ticks(pr.size(), 0ull);
        uint32_t err = 1u;
        if (hipMalloc(&d_pr, pr.size() * sizeof(bgk::XpProbe)) == hipSuccess && hipMalloc(&d_ctl, 128) == hipSuccess && hipMalloc(&d_ticks, pr.size() * 8) == hipSuccess &&
            hipMemcpy(d_pr, pr.data(), pr.size() * sizeof(bgk::XpProbe), hipMemcpyHostToDevice) == hipSuccess && hipMemset(d_ctl, 0, 128) == hipSuccess &&
            hipMemset(d_ticks, 0, pr.size() * 8) == hipSuccess) {
            hipLaunchKernelGGL(bgk::xp_hop_probe_kernel, dim3(256), dim3(64), 0, c->stream, d_pr, (int)pr.size(), reps, d_ctl, d_ticks, d_ctl + 16);
            if (hipStreamSynchronize(c->stream) == hipSuccess && hipMemcpy(ticks.data(), d_ticks, pr.size() * 8, hipMemcpyDeviceToHost) == hipSuccess)
                (void)hipMemcpy(&err, d_ctl + 16, 4, hipMemcpyDeviceToHost);
        }
        (void)hipGetLastError();
        if (d_pr) (void)hipFree(d_pr);
        if (d_ctl) (void)hipFree(d_ctl);
        if (d_ticks) (void)hipFree(d_ticks);
        if (hipMemset(c->xp_hop, 0, bytes) != hipSuccess) return false;      // the probe values must not be mistaken for granules
        if (err == 0u) {
            double gain = 0.0;
            for (int r = 0; r < nl * 2; r++) {
                unsigned long long t[2];
                for (int k = 0; k < 2; k++) t[k] = std::max(ticks[(size_t)(r * 2 + k) * 2], ticks[(size_t)(r * 2 + k) * 2 + 1]);      // a region is as slow as its slower line
                const int fast = t[1] < t[0] ? 1 : 0;
                pick[(size_t)r] = mode == 2 ? 1 - fast : fast;
                gain += (double)(t[1 - fast] - t[fast]) * 10.0 / (2.0 * reps);
            }
            if (c->opt.verbose > 0) fprintf(stderr, "biogpt_hip: cross-XCD hand-off regions placed by measurement: the chosen 8 KB candidates are %.0f ns per hop faster than the others (mean over %d regions)\n", gain / (nl * 2), nl * 2);
        }   // a failed calibration keeps the first candidates: slower hops, same results
    }
    for (int l = 0; l < nl; l++) { tab[(size_t)l].gx1 = cand(l, 0, pick[(size_t)l * 2]); tab[(size_t)l].gx = cand(l, 1, pick[(size_t)l * 2 + 1]); }
    return true;
}

// once per context, outside any stream capture: is this an 8-XCD x 32-CU device that places workgroup b on XCD b % 8 ?
// then the layer table, the granules and the control words.  Leaves xp_state = 1 or -1; never fails the caller.
void xpipe_prepare(biogpt_hip_ctx *c) {
    if (c->xp_state != 0) return;
    c->xp_state = -1;
    if (!xpipe_model_ok(c)) return;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, c->device) != hipSuccess || prop.multiProcessorCount != 256) { (void)hipGetLastError(); return; }
    uint32_t *probe = nullptr;
    if (hipMalloc(&probe, 256 * 4) != hipSuccess) { (void)hipGetLastError(); return; }
    std::vector<uint32_t> where(256, 99u);
    hipLaunchKernelGGL(bgk::xp_probe_kernel, dim3(256), dim3(64), 0, c->stream, probe);
    bool ok = hipStreamSynchronize(c->stream) == hipSuccess && hipMemcpy(where.data(), probe, 256 * 4, hipMemcpyDeviceToHost) == hipSuccess;
    (void)hipFree(probe);
    int per_xcd[16] = {};
    for (int b = 0; ok && b < 256; b++) per_xcd[where[(size_t)b] & 15u]++;
    for (int x = 0; ok && x < 16; x++) ok = per_xcd[x] == (x < 8 ? 32 : 0);   // 8 XCDs, workgroups dealt evenly
    if (!ok) { (void)hipGetLastError(); return; }
    if (!xpipe_process_lock(c)) return;      // (in front of the calibration launch: it is a persistent launch itself)
    const auto &hp = c->hp;
    const size_t P = (size_t)hp.n_positions, D = (size_t)hp.d_model;
    std::vector<bgk::XpLayer> tab((size_t)hp.n_layer);
    for (int l = 0; l < hp.n_layer; l++) {
        const LayerSlots &L = c->plan.layers[(size_t)l];
        bgk::XpLayer &y = tab[(size_t)l];
        y.ln0_w = dev_vec(c, L.ln0_w); y.ln0_b = dev_vec(c, L.ln0_b); y.ln1_w = dev_vec(c, L.ln1_w); y.ln1_b = dev_vec(c, L.ln1_b);
        y.bqkv = dev_vec(c, L.qkv_b); y.bo = dev_vec(c, L.o_b); y.b1 = dev_vec(c, L.fc1_b); y.b2 = dev_vec(c, L.fc2_b);
        y.Wqkv = dev_matrix(c, L.qkv); y.Wo = dev_matrix(c, L.o); y.W1 = dev_matrix(c, L.fc1); y.W2 = dev_matrix(c, L.fc2);
        y.kcache = c->memory_k + (size_t)l * P * D; y.vcache = c->memory_v + (size_t)l * P * D;
    }
    const size_t gbytes = (size_t)hp.n_layer * bgk::XP_G_LAYER * 8;
    const uint32_t ctl0[3] = {1u, 0u, 1u};   // hand-off tag, error word, launch counter
    if (!xpipe_place_hops(c, tab)) { (void)hipGetLastError(); xpipe_release(c); return; }
    if (hipMalloc(&c->xp_layers, tab.size() * sizeof(bgk::XpLayer)) != hipSuccess || hipMalloc(&c->xp_gran, gbytes) != hipSuccess ||
        hipMalloc(&c->xp_ctl, 64) != hipSuccess || hipHostMalloc(reinterpret_cast<void **>(&c->xp_err_host), 64, hipHostMallocDefault) != hipSuccess ||
        hipMemcpy(c->xp_layers, tab.data(), tab.size() * sizeof(bgk::XpLayer), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(c->xp_gran, 0, gbytes) != hipSuccess || hipMemset(c->xp_ctl, 0, 64) != hipSuccess ||
        hipMemcpy(c->xp_ctl, ctl0, 12, hipMemcpyHostToDevice) != hipSuccess ||
        hipMalloc(&c->xp_samp, 2056 * 8) != hipSuccess || hipMemset(c->xp_samp, 0, 2056 * 8) != hipSuccess) {
        (void)hipGetLastError();
        xpipe_release(c);
        return;
    }
    if (hp.n_positions > 256) {   // contexts beyond 256 keys: the key-range helpers' granules (393 KB per layer); without them those contexts keep the five-launch layer
        const size_t lbytes = (size_t)hp.n_layer * bgk::XL_G_LAYER * 8;
        if (hipMalloc(&c->xp_gran_l, lbytes) != hipSuccess || hipMemset(c->xp_gran_l, 0, lbytes) != hipSuccess) {
            (void)hipGetLastError();
            if (c->xp_gran_l) (void)hipFree(c->xp_gran_l);
    if (c->xc_gran) (void)hipFree(c->xc_gran);
    c->xc_gran = nullptr; c->xc_lds = 0;
            c->xp_gran_l = nullptr;
        }
    }
    if (c->opt.xpipe_fault) {
        const uint32_t one = 1u;
        (void)hipMemcpy(c->xp_ctl + 8, &one, 4, hipMemcpyHostToDevice);
    }
    {
        // the GELU table, rebuilt exactly as upload_weights builds it: identity from some positive argument up to +inf, one constant from some negative
        // argument down to the most negative finite value; the MLP halves keep its non-trivial slices in LDS (70 KB)
        std::vector<uint16_t> tg(65536);
        for (uint32_t i = 0; i < 65536; i++) tg[i] = f32_to_f16(gelu_tanh_f32(f16_to_f32((uint16_t)i)));
        int P = 0x7C01;
        while (P > 0 && tg[(size_t)P - 1] == (uint16_t)(P - 1)) P--;
        const uint16_t Z = tg[0xFBFF];
        int N = 0x7C00;
        while (N > 0 && tg[0x8000 + (size_t)N - 1] == Z) N--;
        P = (P + 7) & ~7; N = (N + 7) & ~7;
        const size_t lds_max = 160 * 1024;
        if (P <= 0x7C00 && N <= 0x7C00 && bgk::xpipe_smem_bytes(P + N) <= lds_max) { c->xp_gelu_p = P; c->xp_gelu_n = N; c->xp_gelu_z = Z; }
    }
    if (c->xp_gelu_p + c->xp_gelu_n > 0) {
        // ggml_soft_max's table, rebuilt exactly as upload_weights builds it: arguments are <= 0; entry [0] must be 1.0 and the entries 0 from some negative argument
        // down to the most negative finite value; the slice in between shares the LDS region of the GELU slices (which only the MLP halves use)
        std::vector<uint16_t> te(0x7C00);
        for (uint32_t i = 0; i < 0x7C00; i++) te[i] = f32_to_f16(expf(f16_to_f32((uint16_t)(0x8000u + i))));
        int N = 0x7C00;
        while (N > 0 && te[(size_t)N - 1] == 0) N--;
        N = (N + 7) & ~7;
        if (f32_to_f16(expf(0.0f)) == 0x3C00 && N > 0 && N <= c->xp_gelu_p + c->xp_gelu_n) c->xp_exp_n = N;
    }
    if (!xpipe_set_lds(c)) { (void)hipGetLastError(); xpipe_release(c); return; }
    *c->xp_err_host = 0u;
    c->xp_state = 1;
}

// may a step of context bucket t_max go through the pipeline at all (model, device, options, bucket) ?
bool xpipe_bucket_ok(const biogpt_hip_ctx *c, int t_max) {
    return c->opt.xpipe && c->xp_state == 1 && c->assoc == 0 && (t_max <= 256 || (t_max <= 1024 && c->xp_gran_l != nullptr)) && c->device >= 0 && c->device < 64;
}
// ... and does this context hold the device's pipeline slot ?  Taken here if it is free -- or if its holder is outside every API call that took it and
// has nothing in flight (a resident launch that left after its idle time keeps the slot until its context is called again: such a holder is relieved here;
// it notices at its next call, like any context that finds the slot taken).
bool pipeline_slot_take(biogpt_hip_ctx *c);
bool xpipe_usable(biogpt_hip_ctx *c, int t_max) {
    if (!xpipe_bucket_ok(c, t_max)) return false;
    return pipeline_slot_take(c);
}
// the device's ONE slot for persistent 256-workgroup launches (the XCD pipeline, the chunk launch, the float-weight launch of kernels_fpipe.hip.h)
bool pipeline_slot_take(biogpt_hip_ctx *c) {
    if (c->device < 0 || c->device >= 64) return false;
    std::lock_guard<std::mutex> lk(g_xp_mu);
    biogpt_hip_ctx *&owner = g_xp_owner[c->device];
    if (owner != nullptr && owner != c && !owner->xp_in_call && hipStreamQuery(owner->stream) == hipSuccess) owner = nullptr;
    (void)hipGetLastError();      // hipErrorNotReady of the query is not an error of this call
    if (owner == nullptr) {
        // not while ANOTHER context may have five-launch graphs in flight (plain_graph_begin): a persistent launch would start beside them
        auto &pg = g_xp_plain[c->device];
        for (size_t i = 0; i < pg.size();) {
            if (pg[i] == c) { i++; continue; }
            if (hipStreamQuery(pg[i]->stream) == hipSuccess) { pg[i]->plain_inflight = false; pg.erase(pg.begin() + (long)i); }
            else { (void)hipGetLastError(); return false; }
        }
        (void)hipGetLastError();
    }
    if (owner == nullptr) owner = c;
    if (owner == c) c->xp_in_call = true;      // until the API call that asked returns (XpCallScope)
    return owner == c;
}
// A captured five-launch step (a "plain" graph: graph_eval / graph_step / a column step captured without the column-per-XCD launch) must not be replayed beside ANOTHER context's persistent launch: on
// this runtime its last nodes were observed to see the previous replay's activations (profiles/two_contexts_r4.txt; cause not found, profiles/stale_row_r5.txt).  The
// decision and its record are one step under g_xp_mu (ADVICE r4: a check followed by a launch let the slot change hands in between):
//   plain_graph_begin(c)  false: another context holds the slot -- the caller takes eager launches.  true: c is entered in the device's list of contexts with such
//                         graphs in flight, and xpipe_usable() gives no OTHER context the slot until c's stream has run dry.
//   plain_graph_end(c)    the context is destroyed (otherwise the entry is dropped by xpipe_usable() when it finds c's stream idle).
bool plain_graph_begin(biogpt_hip_ctx *c) {
    if (c->device < 0 || c->device >= 64) return true;
    if (c->xp_foreign && !c->opt.graph_contended) return false;      // the slot's owner may be a context of another process (it holds the device's lock file): eager launches
    std::lock_guard<std::mutex> lk(g_xp_mu);
    const biogpt_hip_ctx *owner = g_xp_owner[c->device];
    if (owner != nullptr && owner != c && !c->opt.graph_contended) return false;
    if (!c->plain_inflight) { c->plain_inflight = true; g_xp_plain[c->device].push_back(c); }
    return true;
}
void plain_graph_end(biogpt_hip_ctx *c) {
    if (c->device < 0 || c->device >= 64) return;
    std::lock_guard<std::mutex> lk(g_xp_mu);
    auto &pg = g_xp_plain[c->device];
    for (size_t i = 0; i < pg.size(); i++) if (pg[i] == c) { pg.erase(pg.begin() + (long)i); break; }
    c->plain_inflight = false;
}
// an API entry that may take the pipeline slot: while it runs, no other context may relieve this one of the slot (its launches are not enqueued yet)
struct XpCallScope {
    biogpt_hip_ctx *c;
    explicit XpCallScope(biogpt_hip_ctx *ctx) : c(ctx) {}
    ~XpCallScope() {
        if (!c) return;
        std::lock_guard<std::mutex> lk(g_xp_mu);
        c->xp_in_call = false;
    }
};
// the context's stream is idle (the caller just synchronised it): nothing pipelined is in flight, another context may have the slot
void xpipe_handback(biogpt_hip_ctx *c) {
    if (c->device < 0 || c->device >= 64) return;
    std::lock_guard<std::mutex> lk(g_xp_mu);
    if (g_xp_owner[c->device] == c) g_xp_owner[c->device] = nullptr;
}

// after a synchronisation: did a hand-off of the pipeline time out (or a workgroup land on an unexpected XCD) ?  Then the
// outputs of that call are garbage: report it, drop the captured graphs and never use the path again in this context.
bool xpipe_check(biogpt_hip_ctx *c) {
    xpipe_handback(c);
    if (!c->xp_err_host || *c->xp_err_host == 0u) { c->unsynced_from = -1; return true; }
    const uint32_t code = *c->xp_err_host;
    if (code == bgk::XP_QUIT) {     // a resident launch left on its own (idle) or on request: not a failure; the device-side word is cleared in stream order
        *c->xp_err_host = 0u;
        HIP_TRY(false, hipMemsetAsync(c->xp_ctl + 1, 0, 4, c->stream));
        return true;
    }
    *c->xp_err_host = 0u;
    c->xp_state = -1;
    if (c->fp_state == 1) c->fp_state = -1;
    c->xp_tripped = true;
    for (auto &pl : c->graph_step) for (auto &row : pl) for (auto &g : row) if (g) { (void)hipGraphExecDestroy(g); g = nullptr; }
    for (auto &pl : c->graph_eval) for (auto &f : pl) for (auto &row : f) for (auto &g : row) if (g) { (void)hipGraphExecDestroy(g); g = nullptr; }
    BG_FAIL(false, "the XCD-pipelined decode step failed (code %u: %s); this context now uses the five-launch layer", code,
            code == 2u ? "its workgroups were not dealt 32 per XCD -- another stream's kernels were dispatched in between" : code == 5u ? "hand-off tags used up" : "a hand-off timed out");
}

int graph_bucket(int T);
int bucket_tmax(const biogpt_hip_ctx *c, int b);
int fast_lm_grid(const biogpt_hip_ctx *c);
bool fused_decode_ok(const biogpt_hip_ctx *c, int t_max);
// tokens one pipelined launch may generate from context T = n_past + 1 on: up to the end of T's context bucket (0: not on the pipeline)
// does the final LayerNorm + lm_head run inside the pipelined launch (its 64-row blocks four per workgroup of the XCDs that are done) ?
bool xpipe_lm_folds(const biogpt_hip_ctx *c) {
    const auto &hp = c->hp;
    const MatSlot &m = c->plan.lm_head;
    // workgroups that take rows: the pipelined launch up to 256 keys (kernels_xpipe.hip.h, xp_lm_rank) and the long-context one (kernels_xlong.hip.h: every XCD but XCD 0 and the last unit's)
    const int lm_parts = fast_lm_grid(c), last_xcd = xpipe_last_xcd(c), lm_wgs = std::min(bgk::xp_lm_capacity(2 * hp.n_layer), 32 * (8 - 1 - (last_xcd != 0 ? 1 : 0)));
    return m.type == ftype_to_type(hp.ftype) && m.K == 1024 && m.M == hp.n_vocab && lm_parts == (hp.n_vocab + 63) / 64 && lm_parts <= 4 * lm_wgs && lm_parts <= 1024;
}
int xpipe_multi_tokens(biogpt_hip_ctx *c, int T) {
    if (!c->opt.xpipe_multi || !xpipe_lm_folds(c)) return 0;
    const int tmax = bucket_tmax(c, graph_bucket(T));
    if (!fused_decode_ok(c, tmax) || !xpipe_usable(c, tmax)) return 0;
    return tmax - T + 1;
}

