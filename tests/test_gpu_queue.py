"""Generation over a queue (biogpt_hip_generate_queue, kernels_queue.hip.h) on the GPU.  The reference in every test is the unchanged generate_sample of each
request ALONE: the queue's ids and lengths equal it per request, whatever else is in the queue, however many columns there are and however often the
host looks at them; a refilled column does not see its predecessor's K / V rows; the schedule is the plan's; the context's own cache is left alone.
No tolerance anywhere: every comparison is equality of ids, lengths and integers."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KW = dict(n_vocab=42384, n_layer=3, n_head=16, n_positions=1024, d_ff=4096, d_model=1024, n_merges=40000)
HOT = (40, 0.95, 6.0)


def prompt_of(n, seed):
    rng = np.random.default_rng(seed)
    return [2] + [int(v) for v in rng.integers(4, KW["n_vocab"], n - 1)]


@pytest.fixture(scope="module")
def files(pkg, tmp_path_factory):
    d = tmp_path_factory.mktemp("queue")
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


def alone(g, prompt, n, seed, eos_id=-1, setting=HOT, n_batch=8):
    """The reference: the request by itself through the closed call."""
    top_k, top_p, temp = setting
    ids, _ = g.generate_sample([prompt], n, top_k=top_k, top_p=top_p, temp=temp, seeds=[seed], eos_id=eos_id, n_batch=n_batch)
    return [int(t) for t in ids[0]]


def queue(g, prompts, n_predicts, seeds, max_columns, group, eos_id=-1, setting=HOT, n_batch=8):
    top_k, top_p, temp = setting
    ids, info, secs = g.generate_queue(prompts, max(n_predicts), max_columns=max_columns, group=group, top_k=top_k, top_p=top_p, temp=temp, seeds=seeds, eos_id=eos_id,
                                       n_batch=n_batch, n_predicts=n_predicts)
    return [[int(t) for t in s] for s in ids], info


def check_plan(pkg, info, lens, prompts, max_columns, group):
    """admit_step / column / stats are the plan's for the lengths the run had (the plan knows no prompts: prompt_columns is the run's own)."""
    want = pkg.queue_plan(lens, max_columns, group)
    assert info["admit_step"] == want["admit_step"] and info["column"] == want["column"]
    ran = [r for r in range(len(lens)) if info["column"][r] >= 0]
    assert info["stats"] == dict(want["stats"], prompt_columns=sum(len(prompts[r]) for r in ran))


# ---- 1. equals the request alone ----

ONE_LENS = (5, 9, 14, 20, 25, 29, 33)
ONE_PREDICTS = [1, 20, 7, 13, 4, 16, 10]
ONE_SEEDS = [301, 302, 303, 304, 305, 306, 307]
ONE_PROMPTS = [prompt_of(n, 100 + n) for n in ONE_LENS]


@pytest.fixture(scope="module")
def one_refs(pkg, files):
    """Per weight format: every request of the first test alone, computed once."""
    out = {}
    for name in ("q4_0", "q5_1", "q8_0"):
        g = pkg.BiogptModel.load(files[name])
        out[name] = [alone(g, ONE_PROMPTS[r], ONE_PREDICTS[r], ONE_SEEDS[r]) for r in range(7)]
        g.close()
        assert [len(w) for w in out[name]] == ONE_PREDICTS
        assert len({t for w in out[name] for t in w}) > 20, "fixture problem: the hot setting does not spread the samples"
    return out


@pytest.mark.parametrize("name, max_columns, group", [("q4_0", 1, 1), ("q4_0", 1, 4), ("q4_0", 3, 1), ("q4_0", 3, 4), ("q4_0", 7, 1), ("q4_0", 7, 4),
                                                      ("q5_1", 3, 4), ("q8_0", 3, 1)])
def test_equals_the_request_alone(pkg, files, one_refs, name, max_columns, group):
    g = pkg.BiogptModel.load(files[name])
    got, info = queue(g, ONE_PROMPTS, ONE_PREDICTS, ONE_SEEDS, max_columns, group)
    g.close()
    for r in range(7):
        assert got[r] == one_refs[name][r], (r, got[r], one_refs[name][r])
    check_plan(pkg, info, [len(s) for s in got], ONE_PROMPTS, max_columns, group)
    assert info["stats"]["columns"] == max_columns and info["stats"]["busy_column_steps"] == sum(ONE_PREDICTS)


# ---- 2. EOS ----

def test_eos_ends_a_request_and_frees_its_column(pkg, q40):
    """12 requests on 3 columns.  Requests 0, 5 and 9 are one prompt, 0 and 5 with one seed: the EOS id is a token their free run draws early (taken from the
    free run, as test_gpu_sample.py takes its), so they end by EOS before their limits, each in its own column and step, while others run to theirs."""
    g = q40
    prompts = [prompt_of(6 + 2 * r, 400 + r) for r in range(12)]
    prompts[5] = prompts[9] = prompts[0]
    seeds = [500 + r for r in range(12)]
    seeds[5] = seeds[0]
    limits = [14, 9, 12, 20, 7, 16, 11, 18, 8, 15, 10, 13]
    free = [alone(g, prompts[r], limits[r], seeds[r]) for r in range(12)]
    assert free[0][:14] == free[5][:14]
    eos = next((t for i, t in enumerate(free[0]) if 1 <= i <= 6 and t not in free[0][:i]), None)
    assert eos is not None, "fixture problem: no early token of request 0's free run can serve as EOS: %s" % free[0]
    want = [f[:f.index(eos) + 1] if eos in f else f for f in free]
    by_eos = [r for r in range(12) if len(want[r]) < limits[r]]
    at_limit = [r for r in range(12) if eos not in free[r]]
    print("eos %d: ended by EOS before the limit %s, at the limit %s, lengths %s" % (eos, by_eos, at_limit, [len(w) for w in want]))
    assert by_eos and at_limit and len({len(w) for w in want}) >= 3, "fixture problem: the EOS id does not split the requests (%s)" % [len(w) for w in want]
    for r in (0, 3, 7):      # the reference itself, with the EOS: the closed call of the request alone
        assert alone(g, prompts[r], limits[r], seeds[r], eos_id=eos) == want[r], r
    for group in (1, 4):
        got, info = queue(g, prompts, limits, seeds, 3, group, eos_id=eos)
        for r in range(12):
            assert got[r] == want[r], (group, r, got[r], want[r])
        st = info["stats"]
        assert st["columns"] == 3 and st["busy_column_steps"] == sum(len(w) for w in want) <= st["column_steps"] == 3 * st["steps"]
        assert sorted(info["admit_step"]) == info["admit_step"] and info["column"][:3] == [0, 1, 2]
    check_plan(pkg, queue(g, prompts, limits, seeds, 3, 1, eos_id=eos)[1], [len(w) for w in want], prompts, 3, 1)      # group 1: no group is cut by a limit


# ---- 3. column reuse ----

def test_a_refilled_column_does_not_see_its_predecessor(q40):
    """One column, group 1: a 40-token prompt with 12 new tokens, then a 6-token prompt with 20: every position of the second request lies on a K / V row the
    first one wrote, and its ids are those of the request alone (in a context whose slot 0 holds that request's rows only up to its own position)."""
    g = q40
    prompts, limits, seeds = [prompt_of(40, 601), prompt_of(6, 602)], [12, 20], [611, 612]
    want = [alone(g, prompts[r], limits[r], seeds[r]) for r in range(2)]
    got, info = queue(g, prompts, limits, seeds, 1, 1)
    assert got == want
    assert info["column"] == [0, 0] and info["admit_step"] == [0, 12] and info["stats"]["admissions"] == 2 and info["stats"]["steps"] == 32


# ---- 4. bucket jumps ----

JUMP_LENS = (7, 12, 9, 70, 300, 1000)
JUMP_PREDICTS = [8, 8, 8, 10, 8, 64]


def test_long_requests_follow_short_ones_through_every_bucket(pkg, q40, monkeypatch):
    """3 columns of short requests; then the queue holds a 70-token prompt (its steps cross the 64-key bucket), a 300-token prompt (the 257 .. 512 kernels)
    and a 1000-token prompt that asks for 64 tokens and is clamped to 24 -- alone: its neighbours keep their own lengths.  Captured steps and eager ones."""
    g = q40
    prompts = [prompt_of(n, 700 + n) for n in JUMP_LENS]
    seeds = [720 + r for r in range(6)]
    monkeypatch.delenv("BIOGPT_HIP_NO_GRAPH", raising=False)
    g.refresh_options()
    want = [alone(g, prompts[r], JUMP_PREDICTS[r], seeds[r]) for r in range(6)]
    assert [len(w) for w in want] == [8, 8, 8, 10, 8, 24]
    try:
        for env in ({}, {"BIOGPT_HIP_NO_GRAPH": "1"}):
            monkeypatch.delenv("BIOGPT_HIP_NO_GRAPH", raising=False)
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            g.refresh_options()
            got, info = queue(g, prompts, JUMP_PREDICTS, seeds, 3, 4)
            for r in range(6):
                assert got[r] == want[r], (env, r, got[r], want[r])
            check_plan(pkg, info, [len(w) for w in want], prompts, 3, 4)
    finally:
        monkeypatch.delenv("BIOGPT_HIP_NO_GRAPH", raising=False)
        g.refresh_options()


# ---- 5. matrix-core steps ----

def test_48_columns_take_the_matrix_core_steps(q40):
    """max_columns = 48 (the decode steps' matrix-core threshold), 60 requests of 2 .. 6 tokens, top_k = 1: generate_greedy_batch's first tokens."""
    g = q40
    prompts = [prompt_of(5 + r % 11, 800 + r) for r in range(60)]
    limits = [2 + r % 5 for r in range(60)]
    greedy, _ = g.generate_greedy_batch(prompts, 6, n_batch=8)
    got, info = queue(g, prompts, limits, list(range(60)), 48, 4, setting=(1, 0.9, 0.9))
    for r in range(60):
        assert got[r] == [int(t) for t in greedy[r][:limits[r]]], r
    assert info["stats"]["columns"] == 48 and info["stats"]["admissions"] >= 2 and max(info["column"]) == 47


# ---- 6. degenerate queues ----

def test_degenerate_queues(pkg, q40):
    g = q40
    top_k, top_p, temp = HOT
    prompts, seeds = [prompt_of(8 + 3 * r, 900 + r) for r in range(4)], [910, 911, 912, 913]
    # fewer requests than columns
    want = [alone(g, prompts[r], 9, seeds[r]) for r in range(3)]
    got, info = queue(g, prompts[:3], [9, 9, 9], seeds[:3], 8, 4)
    assert got == want and info["stats"]["columns"] == 3 and info["column"] == [0, 1, 2] and info["stats"]["admissions"] == 1 and info["stats"]["steps"] == 9
    # as many requests as columns, equal limits: one admission, the ids of ONE closed call
    closed, _ = g.generate_sample(prompts, 10, top_k=top_k, top_p=top_p, temp=temp, seeds=seeds, n_batch=8)
    got, info = queue(g, prompts, [10] * 4, seeds, 4, 4)
    assert got == [[int(t) for t in s] for s in closed]
    assert info["stats"] == dict(columns=4, steps=10, groups=3, admissions=1, prompt_columns=sum(len(p) for p in prompts), busy_column_steps=40, column_steps=40)
    # a request whose prompt fills the position table: length 0, no column, the others unaffected
    full = [2] * KW["n_positions"]
    got, info = queue(g, [prompts[0], full, prompts[1], prompts[2]], [9, 9, 9, 9], [seeds[0], 1, seeds[1], seeds[2]], 2, 4)
    assert got == [want[0], [], want[1], want[2]]
    assert info["column"][1] == -1 and info["admit_step"][1] == -1 and info["column"][0] == 0 and info["column"][2] == 1 and info["stats"]["columns"] == 2
    # nobody eligible: nothing runs
    got, info = queue(g, [full, full], [4, 4], [1, 2], 4, 4)
    assert got == [[], []] and info["stats"]["steps"] == 0 and info["column"] == [-1, -1]
    # n_predicts = 0 for one request
    got, info = queue(g, prompts[:2], [0, 9], seeds[:2], 4, 4)
    assert got == [[], want[1]] and info["column"] == [-1, 0]


def test_model_dependent_argument_errors(pkg, files, tiny_models, q40):
    """What test_queue_capi.py cannot judge without a model: a float-weight file, ids beyond the vocabulary, a prompt beyond the position table."""
    for path in (files["f32"], tiny_models["f16"]):
        g = pkg.BiogptModel.load(path)
        with pytest.raises(pkg.BiogptError, match="fast chain"):
            g.generate_queue([[2, 5, 7]], 4)
        g.close()
    g = q40
    with pytest.raises(pkg.BiogptError, match="out of range"):
        g.generate_queue([[2, 5], [2, KW["n_vocab"]]], 4)
    with pytest.raises(pkg.BiogptError, match="eos_id"):
        g.generate_queue([[2, 5]], 4, eos_id=KW["n_vocab"])
    with pytest.raises(pkg.BiogptError, match="n_positions"):
        g.generate_queue([[2] * (KW["n_positions"] + 1)], 4)
    with pytest.raises(pkg.BiogptError, match="empty prompt"):
        g.generate_queue([[2, 5], []], 4)
    ids, info, _ = g.generate_queue([[2, 5, 7]], 4)      # still usable; the defaults: greedy
    greedy, _ = g.generate_greedy_batch([[2, 5, 7]], 4)
    assert [int(t) for t in ids[0]] == [int(t) for t in greedy[0]]


# ---- 7. repeatability ----

def test_same_call_same_result_other_seeds_other_ids(q40):
    g = q40
    prompts = [prompt_of(6 + r, 1000 + r) for r in range(9)]
    limits = [5 + (3 * r) % 7 for r in range(9)]
    seeds = [1100 + r for r in range(9)]
    a = queue(g, prompts, limits, seeds, 4, 2)
    b = queue(g, prompts, limits, seeds, 4, 2)
    assert a == b
    c, _ = queue(g, prompts, limits, [s + 100 for s in seeds], 4, 2)
    assert all(x != y for x, y in zip(c, a[0]))


# ---- 8. the context's own cache ----

def test_context_cache_untouched_and_eval_follows(pkg, files):
    g = pkg.BiogptModel.load(files["q4_0"])
    h = pkg.BiogptModel.load(files["q4_0"])
    ctx_toks = prompt_of(9, 7)
    row = g.eval(ctx_toks, 0)
    h.eval(ctx_toks, 0)
    D = KW["d_model"]
    k0, v0 = g.read_kv(0, 0, 3 * KW["n_positions"] * D), g.read_kv(1, 0, 3 * KW["n_positions"] * D)
    ids, info, _ = g.generate_queue([prompt_of(17, 8), prompt_of(5, 9), prompt_of(11, 10)], 12, max_columns=2, group=4, top_k=40, seed=3)
    assert [len(i) for i in ids] == [12, 12, 12] and info["stats"]["admissions"] == 2
    assert np.array_equal(g.read_kv(0, 0, k0.size), k0) and np.array_equal(g.read_kv(1, 0, v0.size), v0)
    assert np.array_equal(g.read_logits(), row)
    nxt = [123]
    assert np.array_equal(g.eval(nxt, len(ctx_toks)), h.eval(nxt, len(ctx_toks)))
    g.close()
    h.close()
