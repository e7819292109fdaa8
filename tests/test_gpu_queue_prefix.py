"""Queued generation behind a shared prefix, with log-probabilities (biogpt_hip_generate_queue_prefix, kernels_queue.hip.h) on the GPU.  The reference in
every test is the unchanged closed call of each request ALONE -- generate_sample(prefix=, logprobs=) -- and the unchanged generate_queue on the
concatenations: ids, lengths, log-probabilities (as float32 bit patterns), the schedule and the stats equal them, whatever else is in the queue, however many
columns there are and however often the host looks at them.  The step kernel alone (biogpt_hip_queue_rows_device) is held against sample_lp_rows_kernel
alone for the draw and the entries and against integer logic for the queue's own state.  No tolerance anywhere: every comparison is equality."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KW = dict(n_vocab=42384, n_layer=3, n_head=16, n_positions=1024, d_ff=4096, d_model=1024, n_merges=40000)
HOT = (40, 0.95, 6.0)
P = KW["n_positions"]


def prompt_of(n, seed):
    rng = np.random.default_rng(seed)
    return [2] + [int(v) for v in rng.integers(4, KW["n_vocab"], n - 1)]


def suffix_of(n, seed):
    return prompt_of(n + 1, seed)[1:]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@pytest.fixture(scope="module")
def files(pkg, tmp_path_factory):
    d = tmp_path_factory.mktemp("queue_prefix")
    f32 = str(d / "f32.bin")
    pkg.write_synthetic(f32, **KW)
    out = {"f32": f32}
    for name in ("q4_0", "q5_1", "q8_0"):
        out[name] = str(d / (name + ".bin"))
        pkg.quantize_file(f32, out[name], name)
    return out


@pytest.fixture(scope="module")
def q40(pkg, files):
    g = pkg.BiogptModel.load(files["q4_0"])
    yield g
    g.close()


def alone(g, prefix, suffix, n, seed, eos_id=-1, n_batch=8, logprobs=None):
    """The reference: the request by itself through the closed call.  logprobs=None: its ids; K: (ids, (lp, top_ids, top_lp))."""
    top_k, top_p, temp = HOT
    kw = dict(top_k=top_k, top_p=top_p, temp=temp, seeds=[seed], eos_id=eos_id, n_batch=n_batch)
    if prefix is not None:
        kw["prefix"] = prefix
    if logprobs is None:
        ids, _ = g.generate_sample([suffix], n, **kw)
        return [int(t) for t in ids[0]]
    ids, info, _ = g.generate_sample([suffix], n, logprobs=logprobs, **kw)
    return [int(t) for t in ids[0]], info[0]


def queue(g, prompts, n_predicts, seeds, max_columns, group, eos_id=-1, n_batch=8, **kw):
    top_k, top_p, temp = HOT
    ids, info, secs = g.generate_queue(prompts, max(n_predicts), max_columns=max_columns, group=group, top_k=top_k, top_p=top_p, temp=temp, seeds=seeds, eos_id=eos_id,
                                       n_batch=n_batch, n_predicts=n_predicts, **kw)
    return [[int(t) for t in s] for s in ids], info


def same_lp(got, want):
    """(lp, top_ids, top_lp) of one request, bit for bit."""
    return (got[0].shape == want[0].shape and got[1].shape == want[1].shape and np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(got[1], want[1])
            and np.array_equal(bits(got[2]), bits(want[2])))


def check_against_plain(g, info, plain_info, prefix, suffixes, n_batch):
    """admit_step, column and stats are the plain queue's on the concatenations, but for prompt_columns: the shared rows once, then what every admitted request
    adds to them; prefix_stats() reads the same."""
    n_shared = (len(prefix) - 1) // n_batch * n_batch
    ran = [r for r in range(len(suffixes)) if info["column"][r] >= 0]
    cols = n_shared + sum(len(prefix) - n_shared + len(suffixes[r]) for r in ran)
    assert info["admit_step"] == plain_info["admit_step"] and info["column"] == plain_info["column"]
    assert plain_info["stats"]["prompt_columns"] == sum(len(prefix) + len(suffixes[r]) for r in ran)
    assert info["stats"] == dict(plain_info["stats"], prompt_columns=cols)
    assert g.prefix_stats() == dict(n_shared=n_shared, prompt_columns=cols, path=0, columns=info["stats"]["columns"])


# ---- 1. equals the request alone ----

ONE_SUFFIX_LENS = (0, 3, 9, 14, 20, 25, 33)
ONE_PREDICTS = [1, 20, 7, 13, 4, 16, 10]
ONE_SEEDS = [301, 302, 303, 304, 305, 306, 307]
ONE_SUFFIXES = [suffix_of(n, 100 + n) for n in ONE_SUFFIX_LENS]
PREFIX17 = prompt_of(17, 41)      # n_batch 8: 16 shared rows, one own row
PREFIX16 = prompt_of(16, 42)      # n_batch 8: 8 shared rows, eight own rows
PREFIXES = {17: PREFIX17, 16: PREFIX16}


@pytest.fixture(scope="module")
def one_refs(pkg, files):
    """Per (weight format, prefix length): every request of the first test alone behind the prefix, computed once."""
    out = {}
    for name, lens in (("q4_0", (17, 16)), ("q5_1", (17,)), ("q8_0", (16,))):
        g = pkg.BiogptModel.load(files[name])
        for n_prefix in lens:
            w = [alone(g, PREFIXES[n_prefix], ONE_SUFFIXES[r], ONE_PREDICTS[r], ONE_SEEDS[r]) for r in range(7)]
            assert [len(s) for s in w] == ONE_PREDICTS
            assert len({t for s in w for t in s}) > 20, "fixture problem: the hot setting does not spread the samples"
            out[name, n_prefix] = w
        g.close()
    return out


@pytest.mark.parametrize("name, n_prefix, max_columns, group", [("q4_0", 17, 1, 1), ("q4_0", 17, 3, 4), ("q4_0", 17, 7, 1), ("q4_0", 16, 1, 1), ("q4_0", 16, 3, 4),
                                                                ("q4_0", 16, 7, 1), ("q5_1", 17, 3, 4), ("q8_0", 16, 7, 1)])
def test_equals_the_request_alone(pkg, files, one_refs, name, n_prefix, max_columns, group):
    g = pkg.BiogptModel.load(files[name])
    prefix = PREFIXES[n_prefix]
    got, info = queue(g, ONE_SUFFIXES, ONE_PREDICTS, ONE_SEEDS, max_columns, group, prefix=prefix)
    plain, plain_info = queue(g, [prefix + s for s in ONE_SUFFIXES], ONE_PREDICTS, ONE_SEEDS, max_columns, group)
    for r in range(7):
        assert got[r] == one_refs[name, n_prefix][r], (r, got[r], one_refs[name, n_prefix][r])
    assert got == plain
    assert g.prefix_stats()["n_shared"] == (16 if n_prefix == 17 else 8)
    check_against_plain(g, info, plain_info, prefix, ONE_SUFFIXES, 8)
    assert info["stats"]["columns"] == max_columns and info["stats"]["busy_column_steps"] == sum(ONE_PREDICTS)
    g.close()


# ---- 2. nothing to share ----

def test_nothing_to_share(q40):
    """5 prefix tokens at n_batch 8: no shared rows, no reserved slot -- the plain queue on the concatenations, its prompt columns included."""
    g = q40
    prefix = prompt_of(5, 43)
    got, info = queue(g, ONE_SUFFIXES, ONE_PREDICTS, ONE_SEEDS, 3, 4, prefix=prefix)
    assert g.prefix_stats()["n_shared"] == 0
    check_against_plain(g, info, info, prefix, ONE_SUFFIXES, 8)
    plain, plain_info = queue(g, [prefix + s for s in ONE_SUFFIXES], ONE_PREDICTS, ONE_SEEDS, 3, 4)
    assert got == plain and info == plain_info
    assert got[3] == alone(g, prefix, ONE_SUFFIXES[3], ONE_PREDICTS[3], ONE_SEEDS[3])


# ---- 3. log-probabilities ----

@pytest.fixture(scope="module")
def lp_refs(q40):
    """Every request of the first test alone with logprobs=K, behind the 17-token prefix and as the concatenation without one."""
    out = {}
    for K in (5, 0):
        out[True, K] = [alone(q40, PREFIX17, ONE_SUFFIXES[r], ONE_PREDICTS[r], ONE_SEEDS[r], logprobs=K) for r in range(7)]
        out[False, K] = [alone(q40, None, PREFIX17 + ONE_SUFFIXES[r], ONE_PREDICTS[r], ONE_SEEDS[r], logprobs=K) for r in range(7)]
    return out


@pytest.mark.parametrize("K", [5, 0])
@pytest.mark.parametrize("behind", [True, False])
def test_logprobs_equal_the_request_alone(q40, one_refs, lp_refs, behind, K):
    g = q40
    prompts = ONE_SUFFIXES if behind else [PREFIX17 + s for s in ONE_SUFFIXES]
    kw = dict(prefix=PREFIX17) if behind else {}
    got, info = queue(g, prompts, ONE_PREDICTS, ONE_SEEDS, 3, 4, logprobs=K, **kw)
    without, _ = queue(g, prompts, ONE_PREDICTS, ONE_SEEDS, 3, 4, **kw)
    assert got == without == one_refs["q4_0", 17]
    for r in range(7):
        want_ids, want = lp_refs[behind, K][r]
        assert got[r] == want_ids
        assert info["logprobs"][r][1].shape == (ONE_PREDICTS[r], K)
        assert same_lp(info["logprobs"][r], want), (behind, K, r, info["logprobs"][r][0].tolist(), want[0].tolist())
        if K > 0:
            assert (np.diff(info["logprobs"][r][2], axis=1) <= 0).all() and np.isfinite(info["logprobs"][r][0]).all()


def test_logprobs_equal_score_batch_at_n_batch_1(q40):
    """n_batch 1: every row of a prompt pass sees what a scored row sees, so the entries are score_batch's of prefix ++ suffix ++ ids on the generated
    positions, bit for bit -- the equality does not rest on the genlp path alone."""
    g = q40
    K = 5
    got, info = queue(g, ONE_SUFFIXES, ONE_PREDICTS, ONE_SEEDS, 3, 4, n_batch=1, prefix=PREFIX17, logprobs=K)
    assert g.prefix_stats()["n_shared"] == 16
    assert [len(s) for s in got] == ONE_PREDICTS
    full = [PREFIX17 + ONE_SUFFIXES[r] + got[r] for r in range(7)]
    first = [len(PREFIX17) + len(ONE_SUFFIXES[r]) - 1 for r in range(7)]      # the row that chose the first generated token

    def scored(targets):
        tg = [[-1] * first[r] + [int(v) for v in targets[r]] + [-1] for r in range(7)]
        out = g.score_batch(full, tg)
        return [out[r][0][first[r]:first[r] + len(got[r])] for r in range(7)]
    lp = scored(got)
    for r in range(7):
        assert np.array_equal(bits(info["logprobs"][r][0]), bits(lp[r])), (r, info["logprobs"][r][0].tolist(), lp[r].tolist())
    for j in range(K):
        top = scored([info["logprobs"][r][1][:, j] for r in range(7)])
        for r in range(7):
            assert np.array_equal(bits(info["logprobs"][r][2][:, j]), bits(top[r])), (r, j)


def raw_call(pkg, g, prefix, n_prefix, suffixes, n_predicts, seeds, max_columns, group, n_top, fill=7):
    """The C entry point itself, on arrays preset to `fill`: (rc, ids, lens, lp, top_ids, top_lp) with the arrays whole."""
    top_k, top_p, temp = HOT
    R, w = len(suffixes), max(n_predicts)
    flat = np.ascontiguousarray([t for s in suffixes for t in s] or [0], dtype=np.int32)
    lens = np.asarray([len(s) for s in suffixes], dtype=np.int32)
    pre = None if prefix is None else np.ascontiguousarray(prefix, dtype=np.int32)
    npr, sd = np.asarray(n_predicts, dtype=np.int32), np.asarray(seeds, dtype=np.uint32)
    out, ol = np.full((R, w), fill, np.int32), np.full(R, fill, np.int32)
    k = max(n_top, 1)
    lp, tid, tlp = np.full((R, w), fill, np.float32), np.full((R, w, k), fill, np.int32), np.full((R, w, k), fill, np.float32)
    req = pkg.GenLogprobs(n_top, lp.ctypes.data, tid.ctypes.data, tlp.ctypes.data)
    secs, st = ctypes.c_double(0.0), pkg.QueueStats()
    rc = pkg.lib().biogpt_hip_generate_queue_prefix(g._h, None if pre is None else pre.ctypes.data, n_prefix, flat.ctypes.data, lens.ctypes.data, R, npr.ctypes.data, w,
                                                    max_columns, group, 8, top_k, top_p, temp, sd.ctypes.data, -1, out.ctypes.data, ol.ctypes.data, None, None,
                                                    ctypes.byref(secs), ctypes.byref(st), ctypes.byref(req))
    return rc, out, ol, lp, tid, tlp


def test_logprob_tails_read_zero(pkg, q40, lp_refs):
    """The caller's arrays as the call leaves them: entries at or past a request's length, and every entry of a request that never takes a column, read
    0 / -1 / 0 whatever they held."""
    predicts = list(ONE_PREDICTS)
    predicts[4] = 0      # never takes a column
    rc, out, ol, lp, tid, tlp = raw_call(pkg, q40, PREFIX17, 17, ONE_SUFFIXES, predicts, ONE_SEEDS, 3, 4, 5)
    assert rc == 0, pkg._err()
    assert [int(v) for v in ol] == predicts
    for r in range(7):
        n = predicts[r]
        want_ids, want = lp_refs[True, 5][r]
        assert [int(t) for t in out[r, :n]] == want_ids[:n] and (out[r, n:] == -1).all()
        assert np.array_equal(bits(lp[r, :n]), bits(want[0][:n])) and np.array_equal(tid[r, :n], want[1][:n]) and np.array_equal(bits(tlp[r, :n]), bits(want[2][:n]))
        assert (bits(lp[r, n:]) == 0).all() and (tid[r, n:] == -1).all() and (bits(tlp[r, n:]) == 0).all()


# ---- 4. EOS and column reuse behind a prefix ----

def test_eos_ends_a_request_and_frees_its_column(q40):
    """12 requests on 3 columns behind the 17-token prefix.  Requests 0, 5 and 9 are one suffix, 0 and 5 with one seed: the EOS id is a token their free run
    draws early (taken from the free run, as tests/test_gpu_queue.py takes its), so they end by EOS before their limits while others run to theirs."""
    g = q40
    suffixes = [suffix_of(2 * r, 400 + r) for r in range(12)]
    suffixes[5] = suffixes[9] = suffixes[0]
    seeds = [500 + r for r in range(12)]
    seeds[5] = seeds[0]
    limits = [14, 9, 12, 20, 7, 16, 11, 18, 8, 15, 10, 13]
    free = [alone(g, PREFIX17, suffixes[r], limits[r], seeds[r]) for r in range(12)]
    assert free[0][:14] == free[5][:14]
    eos = next((t for i, t in enumerate(free[0]) if 1 <= i <= 6 and t not in free[0][:i]), None)
    assert eos is not None, "fixture problem: no early token of request 0's free run can serve as EOS: %s" % free[0]
    cut = [f[:f.index(eos) + 1] if eos in f else f for f in free]
    by_eos = [r for r in range(12) if len(cut[r]) < limits[r]]
    at_limit = [r for r in range(12) if eos not in free[r]]
    assert by_eos and at_limit and len({len(w) for w in cut}) >= 3, "fixture problem: the EOS id does not split the requests (%s)" % [len(w) for w in cut]
    want = [alone(g, PREFIX17, suffixes[r], limits[r], seeds[r], eos_id=eos, logprobs=3) for r in range(12)]
    assert [w[0] for w in want] == cut
    for group in (1, 4):
        got, info = queue(g, suffixes, limits, seeds, 3, group, eos_id=eos, prefix=PREFIX17, logprobs=3)
        for r in range(12):
            assert got[r] == want[r][0], (group, r, got[r], want[r][0])
            assert same_lp(info["logprobs"][r], want[r][1]), (group, r)
        st = info["stats"]
        assert st["columns"] == 3 and st["busy_column_steps"] == sum(len(w) for w in cut) <= st["column_steps"] == 3 * st["steps"]
        assert sorted(info["admit_step"]) == info["admit_step"] and info["column"][:3] == [0, 1, 2]


# ---- 5. a refilled column ----

def test_a_refilled_column_sees_neither_its_predecessor_nor_a_stale_lp_row(q40):
    """One column, group 1: a 40-token suffix with 12 new tokens, then an empty suffix with 20 -- every position of the second request lies on a K / V row the
    first one wrote and every entry of its log-probability row on one the first one wrote."""
    g = q40
    suffixes, limits, seeds = [suffix_of(40, 601), []], [12, 20], [611, 612]
    want = [alone(g, PREFIX17, suffixes[r], limits[r], seeds[r], logprobs=4) for r in range(2)]
    got, info = queue(g, suffixes, limits, seeds, 1, 1, prefix=PREFIX17, logprobs=4)
    assert got == [w[0] for w in want]
    assert same_lp(info["logprobs"][0], want[0][1]) and same_lp(info["logprobs"][1], want[1][1])
    assert info["column"] == [0, 0] and info["admit_step"] == [0, 12] and info["stats"]["admissions"] == 2 and info["stats"]["steps"] == 32


# ---- 6. bucket borders ----

def test_bucket_borders_and_a_request_clamped_by_its_own_length(q40):
    """A 60-token prefix, suffixes of 2 and 9 tokens with 12 new ones on 2 columns: their steps cross the 64-key bucket.  Then a request of 1000 tokens in all
    that asks for 64 and is clamped to 24, alone: the last bucket."""
    g = q40
    prefix = prompt_of(60, 44)
    suffixes, asked, seeds = [suffix_of(2, 701), suffix_of(9, 702), suffix_of(940, 703)], [12, 12, 64], [711, 712, 713]
    want = [alone(g, prefix, suffixes[r], asked[r], seeds[r]) for r in range(3)]
    assert [len(w) for w in want] == [12, 12, 24]
    got, info = queue(g, suffixes, asked, seeds, 2, 4, prefix=prefix)
    assert got == want
    plain, plain_info = queue(g, [prefix + s for s in suffixes], asked, seeds, 2, 4)
    assert plain == want
    got, info = queue(g, suffixes, asked, seeds, 2, 4, prefix=prefix)      # (prefix_stats: of the last call behind a prefix)
    check_against_plain(g, info, plain_info, prefix, suffixes, 8)


# ---- 7. the grouped attention kernel ----

def test_steps_on_the_grouped_attention_kernel(pkg, files, one_refs, monkeypatch):
    """BIOGPT_HIP_PREFIX_ATTN=1 (read when a model is loaded): every step behind shared rows takes attn_prefix_kernel<8>, here with a masked group of 3
    columns whose requests change under it."""
    monkeypatch.setenv("BIOGPT_HIP_PREFIX_ATTN", "1")
    g = pkg.BiogptModel.load(files["q4_0"])
    got, info = queue(g, ONE_SUFFIXES, ONE_PREDICTS, ONE_SEEDS, 3, 4, prefix=PREFIX17)
    g.close()
    assert got == one_refs["q4_0", 17]
    assert info["stats"]["columns"] == 3 and info["stats"]["busy_column_steps"] == sum(ONE_PREDICTS)


# ---- 8. forms do not share graphs ----

def test_forms_do_not_share_graphs_and_the_context_is_left_alone(pkg, files, one_refs, lp_refs):
    """One model, the same three columns throughout: plain queue, prefix queue, prefix + log-probabilities, plain again, a prefix of another length.  Each
    form has captured steps of its own; the context's own K / V cache and logits row are what they were."""
    g = pkg.BiogptModel.load(files["q4_0"])
    ctx_toks = prompt_of(9, 7)
    row = g.eval(ctx_toks, 0)
    D = KW["d_model"]
    k0, v0 = g.read_kv(0, 0, 3 * P * D), g.read_kv(1, 0, 3 * P * D)
    concat = [PREFIX17 + s for s in ONE_SUFFIXES]
    want = one_refs["q4_0", 17]
    assert queue(g, concat, ONE_PREDICTS, ONE_SEEDS, 3, 4)[0] == want
    assert queue(g, ONE_SUFFIXES, ONE_PREDICTS, ONE_SEEDS, 3, 4, prefix=PREFIX17)[0] == want
    got, info = queue(g, ONE_SUFFIXES, ONE_PREDICTS, ONE_SEEDS, 3, 4, prefix=PREFIX17, logprobs=5)
    assert got == want and all(same_lp(info["logprobs"][r], lp_refs[True, 5][r][1]) for r in range(7))
    assert queue(g, concat, ONE_PREDICTS, ONE_SEEDS, 3, 4)[0] == want
    assert queue(g, ONE_SUFFIXES, ONE_PREDICTS, ONE_SEEDS, 3, 4, prefix=PREFIX16)[0] == one_refs["q4_0", 16]
    got, info = queue(g, concat, ONE_PREDICTS, ONE_SEEDS, 3, 4, logprobs=5)
    assert got == want and all(same_lp(info["logprobs"][r], lp_refs[False, 5][r][1]) for r in range(7))
    assert np.array_equal(g.read_kv(0, 0, k0.size), k0) and np.array_equal(g.read_kv(1, 0, v0.size), v0)
    assert np.array_equal(g.read_logits(), row)
    g.close()


# ---- 9. the step kernel alone ----

def mt_seeded(seed):
    """std::mt19937(seed) before its first block of outputs: 624 words, then the index 624."""
    mt = np.zeros(625, dtype=np.uint64)
    mt[0] = seed
    for i in range(1, 624):
        mt[i] = (1812433253 * (int(mt[i - 1]) ^ (int(mt[i - 1]) >> 30)) + i) & 0xFFFFFFFF
    mt[624] = 624
    return mt.astype(np.uint32)


ROWS_STRIDE, ROWS_TOP = 6, 8
#            n_gen limit finished
ROWS_START = [(3, 5, 0),      # one token under its limit afterwards
              (4, 5, 0),      # reaches its limit in this launch
              (4, 5, 0),      # draws the EOS at its limit
              (1, 5, 0),      # draws the EOS under its limit
              (7, 9, 1),      # finished already: nothing may change
              (2, 5, 0)]      # fewer than 8 entries that are no NaN


@pytest.mark.parametrize("V", [42384, 1003])
def test_the_step_kernel_alone(pkg, V):
    top_k, top_p, temp = HOT
    rng = np.random.default_rng(900 + V)
    rows = (3.0 * rng.standard_normal((6, V))).astype(np.float32)
    rows[3] = rows[2]
    rows[5, :] = np.nan
    rows[5, rng.choice(V, 5, replace=False)] = (2.0 * rng.standard_normal(5)).astype(np.float32)
    mt0 = np.stack([mt_seeded(s) for s in (11, 12, 13, 13, 15, 16)])      # rows 2 and 3: one row, one generator, one draw
    # the draw and the entries: sample_lp_rows_kernel alone on the same rows
    mt_ref = mt0.copy()
    ref_ids, ref_lp, ref_tid, ref_tlp = pkg.genlp_rows(rows, ROWS_TOP, mode=1, top_k=top_k, top_p=top_p, temp=temp, states=mt_ref)
    eos = int(ref_ids[2])
    assert int(ref_ids[3]) == eos and all(int(ref_ids[r]) != eos for r in (0, 1, 5)), "fixture problem: the EOS id is not drawn by rows 2 and 3 alone: %s" % ref_ids
    assert (ref_tid[5, 5:] == -1).all() and (ref_tid[5, :5] >= 0).all() and (ref_tid[:5] >= 0).all()

    def start():
        states = np.zeros((6, 8), dtype=np.int32)
        for r, (n_gen, _, _) in enumerate(ROWS_START):
            states[r] = [20 + r, 1000 + r, n_gen, r, 0, 16, 6, 0]      # n_past, token, n_gen, seq_id, t_vis, shared rows and their slot
        hdr = np.zeros(13, dtype=np.int32)
        hdr[0] = 5                       # n_live
        hdr[1 + 4], hdr[7 + 4] = 1, 7    # the finished column's report, made when it finished
        return states, np.asarray([f for _, _, f in ROWS_START], dtype=np.int32), mt0.copy(), hdr
    limits = [lim for _, lim, _ in ROWS_START]

    # what integer logic says
    want_states, want_fin, _, want_hdr = start()
    for r, (n_gen, lim, fin) in enumerate(ROWS_START):
        if fin:
            continue
        want_states[r, 2] = n_gen + 1
        if int(ref_ids[r]) != eos:
            want_states[r, 0] += 1
            want_states[r, 1] = int(ref_ids[r])
        if int(ref_ids[r]) == eos or n_gen + 1 >= lim:
            want_fin[r] = 1
            want_hdr[0] -= 1
            want_hdr[1 + r], want_hdr[7 + r] = 1, n_gen + 1
    assert [int(v) for v in want_fin] == [0, 1, 1, 1, 1, 0] and int(want_hdr[0]) == 2 and [int(v) for v in want_hdr[7:]] == [0, 5, 5, 2, 7, 0]
    want_mt = mt_ref.copy()
    want_mt[4] = mt0[4]

    out = {}
    for with_lp in (True, False):
        states, fin, mt, hdr = start()
        ids, lp, tid, tlp = pkg.queue_rows(rows, states, limits, fin, mt, hdr, n_top=ROWS_TOP, stride=ROWS_STRIDE, top_k=top_k, top_p=top_p, temp=temp, eos_id=eos,
                                           with_lp=with_lp)
        assert np.array_equal(states, want_states), (with_lp, states.tolist(), want_states.tolist())
        assert np.array_equal(fin, want_fin) and np.array_equal(hdr, want_hdr), (with_lp, fin.tolist(), hdr.tolist(), want_hdr.tolist())
        assert np.array_equal(mt, want_mt)
        for r, (n_gen, _, done) in enumerate(ROWS_START):
            wrote = np.zeros(ROWS_STRIDE, dtype=bool)
            if not done:
                wrote[n_gen] = True
                assert int(ids[r, n_gen]) == int(ref_ids[r])
            assert (ids[r, ~wrote] == -1).all()
            if not with_lp:
                wrote[:] = False
            elif not done:
                assert bits(lp[r, n_gen]) == bits(ref_lp[r]), (r, float(lp[r, n_gen]), float(ref_lp[r]))
                assert np.array_equal(tid[r, n_gen], ref_tid[r]) and np.array_equal(bits(tlp[r, n_gen]), bits(ref_tlp[r])), r
            assert (bits(lp[r, ~wrote]) == -1).all() and (tid[r, ~wrote] == -1).all() and (bits(tlp[r, ~wrote]) == -1).all()      # 0xff bytes: never written
        out[with_lp] = ids
    assert np.array_equal(out[True], out[False])


# ---- 10. errors that need a model ----

def test_model_dependent_argument_errors(pkg, files, q40):
    g = pkg.BiogptModel.load(files["f32"])
    with pytest.raises(pkg.BiogptError, match="fast chain"):
        g.generate_queue([[5, 7]], 4, prefix=[2, 9, 11])
    g.close()
    g = q40
    with pytest.raises(pkg.BiogptError, match=r"n_prefix \(17\) \+ suffix_lens\[1\] \(1008\) exceeds n_positions"):
        g.generate_queue([[5], [5] * (P - 16)], 4, prefix=PREFIX17)
    with pytest.raises(pkg.BiogptError, match="n_prefix .* exceeds n_positions"):
        g.generate_queue([[5]], 4, prefix=[2] * (P + 1))
    with pytest.raises(pkg.BiogptError, match=r"max_columns must be in \[1, 511\] behind a prefix"):
        g.generate_queue([[5]], 4, prefix=PREFIX17, max_columns=512)
    with pytest.raises(pkg.BiogptError, match="out of range"):
        g.generate_queue([[5]], 4, prefix=[2, KW["n_vocab"]])
    rc = raw_call(pkg, g, PREFIX17, 17, [[5]], [4], [1], 3, 4, 9)[0]
    assert rc == -1 and "logprobs.n_top must be in [0, 8] (got 9)" in pkg._err()
    rc = raw_call(pkg, g, None, 3, [[2, 5]], [4], [1], 3, 4, 0)[0]
    assert rc == -1 and "n_prefix must be 0 without a prefix (got 3)" in pkg._err()
    want = alone(g, PREFIX17, [5, 7], 6, 21)      # still usable
    assert queue(g, [[5, 7]], [6], [21], 2, 4, prefix=PREFIX17)[0] == [want]
