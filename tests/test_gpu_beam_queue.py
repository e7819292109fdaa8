"""Beam search over a queue (biogpt_hip_generate_beam_queue, kernels_beam_queue.hip.h) on the GPU.  The reference in every test is the unchanged generate_beam of
each request ALONE: the queue's hypotheses, lengths, counts and f32 scores equal it per request, whatever else is in the queue, however many slots there are
and however often the host looks at them; a refilled slot sees neither its predecessor's K / V rows nor its pool; the schedule is the plan's; the context's own
cache and a closed call that follows are left alone.  No tolerance anywhere: every comparison is equality."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KW = dict(n_vocab=42384, n_layer=3, n_head=16, n_positions=1024, d_ff=4096, d_model=1024, n_merges=40000)
V = KW["n_vocab"]


def prompt_of(n, seed):
    rng = np.random.default_rng(seed)
    return [2] + [int(v) for v in rng.integers(4, V, n - 1)]


@pytest.fixture(scope="module")
def files(pkg, tmp_path_factory):
    d = tmp_path_factory.mktemp("beam_queue")
    f32 = str(d / "f32.bin")
    pkg.write_synthetic(f32, **KW)
    out = {"f32": f32}
    for name in ("q4_0", "q5_1", "q8_0"):
        out[name] = str(d / (name + ".bin"))
        pkg.quantize_file(f32, out[name], name)
    return out


@pytest.fixture(scope="module")
def models(pkg, files):
    """One context per file for the whole module (a call leaves nothing behind that the next one reads: the last test checks that)."""
    ms = {name: pkg.BiogptModel.load(files[name]) for name in ("q4_0", "q5_1", "q8_0")}
    yield ms
    for m in ms.values():
        m.close()


def norm(hyps):
    """ids as int lists, scores as the f32 values they are (compared with ==)."""
    return [([int(t) for t in ids], float(np.float32(s))) for ids, s in hyps]


def alone(g, prompts, limits, **kw):
    """The reference: every request by itself through the closed call, under its own limit."""
    return [norm(g.generate_beam(p, n, **kw)[0]) for p, n in zip(prompts, limits)]


def queue(g, prompts, limits, slots, group, **kw):
    hyps, info, _ = g.generate_beam_queue(prompts, max(limits), max_columns=slots * kw["n_beams"], group=group, n_predicts=limits, **kw)
    return [norm(h) for h in hyps], info


def assert_equal(got, want, what):
    assert len(got) == len(want), what
    for r, (a, b) in enumerate(zip(got, want)):
        assert len(a) == len(b), (what, "request", r, "count", len(a), len(b))          # counts
        for i, ((ia, sa), (ib, sb)) in enumerate(zip(a, b)):
            assert ia == ib, (what, "request", r, "hypothesis", i, ia, ib)                # ids and lengths
            assert sa == sb, (what, "request", r, "hypothesis", i, sa, sb)                # f32 scores, ==


def check_plan(pkg, info, prompts, limits, slots, group):
    """admit_step / slot / stats are the plan's for the steps the searches took (the plan knows no prompts: prompt_columns is the run's own): the scheduler the
    call drives, given the steps and the limits as clamped (queue_plan(..., limits=): biogpt_hip_queue_plan_limits), in EVERY case.  queue_plan(steps) without
    the limits is the same schedule at group 1 and where every search ran to its limit, asserted; elsewhere a group may have been sized by a limit that an
    early stop undercut.  Returns whether the two plans agree."""
    steps = info["steps"]
    clamped = [max(0, min(n, KW["n_positions"] - len(p))) for n, p in zip(limits, prompts)]
    ran = [r for r in range(len(steps)) if info["slot"][r] >= 0]
    assert ran == [r for r, n in enumerate(clamped) if n > 0]
    want = pkg.queue_plan(steps, slots, group, limits=clamped)
    assert info["admit_step"] == want["admit_step"] and info["slot"] == want["column"]
    assert info["stats"] == dict(want["stats"], prompt_columns=sum(len(prompts[r]) for r in ran))
    plain = pkg.queue_plan(steps, slots, group)
    if group == 1 or all(steps[r] == clamped[r] for r in ran):
        assert plain == want
    return plain == want


def check_steps(want, steps, limits, what):
    """The steps a search took, against the reference's hypotheses: no hypothesis is longer than the search ran, and no search runs beyond its limit."""
    for r, hyps in enumerate(want):
        longest = max([len(ids) for ids, _ in hyps] or [0])
        assert longest <= steps[r] <= limits[r], (what, r, longest, steps[r], limits[r])


# ---- 1. equals the request alone; 2. the schedule is the plan's ----

ONE_LENS = (5, 9, 14, 20, 25, 29, 33)
ONE_LIMITS = [1, 20, 7, 13, 4, 16, 10]
ONE_PROMPTS = [prompt_of(n, 100 + n) for n in ONE_LENS]
SETTINGS = ((True, 1.0), (False, 0.8))      # (early_stopping, length_penalty)


def eos_from_free_run(g, prompt, B):
    """As test_gpu_beam_batch.py chooses it: the third token of the best hypothesis of an EOS-free run, so that EOS fires mid-run."""
    hyps, _ = g.generate_beam(prompt, 20, n_beams=B, eos_id=-1)
    return int(hyps[0][0][2])


@pytest.fixture(scope="module")
def one_refs(models):
    """Per (weight format, n_beams, early_stopping, length_penalty): the EOS id and every request of the first test alone, computed once and left unchanged."""
    cache = {}

    def get(name, B, es, lp):
        key = (name, B, es, lp)
        if key not in cache:
            g = models[name]
            eos = eos_from_free_run(g, ONE_PROMPTS[1], B)
            cache[key] = (eos, alone(g, ONE_PROMPTS, ONE_LIMITS, n_beams=B, eos_id=eos, length_penalty=lp, early_stopping=es, n_batch=8))
        return cache[key]
    return get


CASES = [("q4_0", B, S, group) for B in (1, 2, 5) for S in (1, 3, 7) for group in (1, 4)] + [("q5_1", 5, 3, 4), ("q8_0", 5, 3, 1)]


@pytest.mark.parametrize("name, B, slots, group", CASES)
def test_equals_the_request_alone(pkg, models, one_refs, name, B, slots, group):
    g = models[name]
    settings = SETTINGS + ((True, 0.8), (False, 1.0)) if (B, slots) == (5, 3) else SETTINGS
    for es, lp in settings:
        what = (name, B, slots, group, es, lp)
        eos, want = one_refs(name, B, es, lp)
        got, info = queue(g, ONE_PROMPTS, ONE_LIMITS, slots, group, n_beams=B, eos_id=eos, length_penalty=lp, early_stopping=es, n_batch=8)
        assert_equal(got, want, what)
        steps = info["steps"]
        check_steps(want, steps, ONE_LIMITS, what)
        print("%s: eos %d, steps %s of %s" % (what, eos, steps, ONE_LIMITS))
        # the fixture: searches of at least three different lengths, one that runs to its limit
        assert len(set(steps)) >= 3, ("fixture problem", what, steps)
        assert any(s == n for s, n in zip(steps, ONE_LIMITS)), ("fixture problem: no search runs to its limit", what, steps)
        # ... and one that stops before its limit.  A search stops early once n_beams hypotheses have ended with EOS.  This model's rows are close to uniform (a
        # generated token costs about 8.1 nats, log n_vocab is 10.7): an id taken from the free run ends ONE hypothesis, which later, better ones may push out
        # of the pool again, and the pool of a search with two or five beams never fills -- test_no_free_run_id_stops_a_search_with_several_beams_early asserts
        # that of every candidate id.  So here the one-beam searches stop early (at request 1's third token), and the same seven requests with two and five
        # beams stop early on the second file of section 1b, where all three conditions are asserted in every case.
        if B == 1:
            assert any(s < n for s, n in zip(steps, ONE_LIMITS)), ("fixture problem: no search stops before its limit", what, steps)
        check_plan(pkg, info, ONE_PROMPTS, ONE_LIMITS, slots, group)
        st = info["stats"]
        assert st["columns"] == slots and st["busy_column_steps"] == sum(steps) <= st["column_steps"] == slots * st["steps"]
        assert sorted(info["admit_step"]) == info["admit_step"] and info["slot"][:slots] == list(range(slots))


# ---- 1b. searches with several beams that stop before their limits ----
# On the model above no EOS id stops a search of two or five beams early (the test below searches for one and asserts that it finds none), so these cases
# run on a second file of the same shape, made from the same f32 file: the final LayerNorm's channel 0 is the constant 1 (gain 0, bias 1), column 0 of
# output_projection is 0 but for the EOS row, which holds EOS_BIAS -- every row's EOS logit is raised by EOS_BIAS and nothing else changes.  The other logits
# of a row are about N(0, 0.64^2), the largest of 42 384 near 2.7: at 2.5 EOS is among a row's leading candidates at every step without dominating it, so
# hypotheses end here and there and pools of two and five fill at different steps (at 3.0 and above nearly every search stops at step 2 or 3, at 2.0 the
# five-beam searches of the q8_0 file run to their limits).

EOS_BIAS = 2.5
BIASED_EOS = 2


@pytest.fixture(scope="module")
def biased(pkg, files, tmp_path_factory):
    from modelfile_py import read_model, write_model
    d = tmp_path_factory.mktemp("beam_queue_biased")
    hp, vocab, merges, tensors = read_model(files["f32"])
    out = []
    for t in tensors:
        a = np.frombuffer(t["raw"], dtype=np.float32).copy()
        if t["name"] == "biogpt.layer_norm.weight":
            a[0] = 0.0
        elif t["name"] == "biogpt.layer_norm.bias":
            a[0] = 1.0
        elif t["name"] == "output_projection.weight":
            a = a.reshape(t["ne"][1], t["ne"][0])
            a[:, 0] = 0.0
            a[BIASED_EOS, 0] = EOS_BIAS
        out.append(dict(t, raw=a.tobytes()))
    f32 = str(d / "f32.bin")
    write_model(f32, hp, vocab, merges, out)
    ms = {}
    for name in ("q4_0", "q8_0"):
        path = str(d / (name + ".bin"))
        pkg.quantize_file(f32, path, name)
        ms[name] = pkg.BiogptModel.load(path)
    yield ms
    for m in ms.values():
        m.close()


@pytest.fixture(scope="module")
def biased_refs(biased):
    cache = {}

    def get(name, B, es, lp):
        key = (name, B, es, lp)
        if key not in cache:
            cache[key] = alone(biased[name], ONE_PROMPTS, ONE_LIMITS, n_beams=B, eos_id=BIASED_EOS, length_penalty=lp, early_stopping=es, n_batch=8)
        return cache[key]
    return get


@pytest.mark.parametrize("name, B, slots, group", [("q4_0", B, S, group) for B in (2, 5) for S in (1, 3, 7) for group in (1, 4)] + [("q8_0", 5, 3, 4)])
def test_searches_with_several_beams_stop_early_and_hand_their_slots_on(pkg, biased, biased_refs, name, B, slots, group):
    """The seven requests of the first test where EOS is a leading candidate of every row: pools fill, searches stop before their limits at different steps,
    their pools are copied out while their neighbours run and their slots are refilled.  All three fixture conditions are asserted in every case."""
    g = biased[name]
    cut = 0
    for es, lp in SETTINGS:
        what = (name, B, slots, group, es, lp)
        want = biased_refs(name, B, es, lp)
        got, info = queue(g, ONE_PROMPTS, ONE_LIMITS, slots, group, n_beams=B, eos_id=BIASED_EOS, length_penalty=lp, early_stopping=es, n_batch=8)
        assert_equal(got, want, what)
        steps = info["steps"]
        check_steps(want, steps, ONE_LIMITS, what)
        print("%s: steps %s of %s" % (what, steps, ONE_LIMITS))
        assert len(set(steps)) >= 3, ("fixture problem", what, steps)
        assert any(s < n for s, n in zip(steps, ONE_LIMITS)), ("fixture problem: no search stops before its limit", what, steps)
        assert any(s == n for s, n in zip(steps, ONE_LIMITS)), ("fixture problem: no search runs to its limit", what, steps)
        assert all(len(w) == B for w, s, n in zip(want, steps, ONE_LIMITS) if s < n and es), what      # a search that stopped early under early_stopping had a full pool
        cut += 0 if check_plan(pkg, info, ONE_PROMPTS, ONE_LIMITS, slots, group) else 1
        assert info["stats"]["busy_column_steps"] == sum(steps)
    if (slots, group) == (1, 4):
        # one slot, group 4: the search that stops early leaves a group sized by its limit, so the run is NOT queue_plan(steps) -- it follows the plan with limits
        assert cut > 0, "fixture problem: no group was cut short by a limit that an early stop undercut"


def test_no_free_run_id_stops_a_search_with_several_beams_early(models):
    """Why the cases above need their own file.  Every id of every request's EOS-free hypotheses is tried as the EOS id on the first test's model: with two and
    with five beams each of them ends at most stray hypotheses and every search still runs to its limit.  (With one beam the first EOS fills the pool.)"""
    g = models["q4_0"]
    for B in (2, 5):
        cands = []
        for p in ONE_PROMPTS:
            hyps, _ = g.generate_beam(p, 20, n_beams=B, eos_id=-1)
            cands += [int(t) for ids, _ in hyps for t in ids]
        cands = list(dict.fromkeys(cands))
        assert len(cands) >= 100
        early = []
        for eos in cands:
            _, info = queue(g, ONE_PROMPTS, ONE_LIMITS, 7, 4, n_beams=B, eos_id=eos, length_penalty=1.0, early_stopping=True, n_batch=8)
            if info["steps"] != ONE_LIMITS:
                early.append((eos, info["steps"]))
        assert not early, (B, early)


# ---- 3. slot reuse ----

def test_a_refilled_slot_sees_neither_rows_nor_pool_of_its_predecessor(models):
    """One slot, group 1, no EOS: a 40-token prompt whose search runs 12 steps and ends with a full pool (at the limit every leading candidate is pooled), then
    a 6-token prompt with 20: every position of the second search (5 .. 25) lies on K / V rows the first one wrote (0 .. 51) in all four cache slots, its
    pool slots held the first request's 12-token ids, and its hypotheses, count and scores are those of the request alone.  Both premises are read back
    (read_column_state): after the first request alone the four columns hold its rows at position 20 (a prompt row, inside the second search's reach) and 45 (a
    generated row, beyond it) and its ids in their pool rows; after the call with both, row 20 has changed in every column, row 45 has not, and the pool rows
    hold the second request's ids."""
    g = models["q4_0"]
    B = 4
    prompts, limits = [prompt_of(40, 601), prompt_of(6, 602)], [12, 20]
    kw = dict(n_beams=B, eos_id=-1, length_penalty=1.0, early_stopping=True, n_batch=8)
    want = alone(g, prompts, limits, **kw)
    assert len(want[0]) == B and all(len(ids) == 12 for ids, _ in want[0]), "fixture problem: the first search does not fill its pool"
    assert len(want[1]) == B and all(len(ids) == 20 for ids, _ in want[1])
    got, _ = queue(g, prompts[:1], limits[:1], 1, 1, **kw)
    assert_equal(got, want[:1], "the first request in slot 0")
    first = [[g.read_column_state(c, pos, n_ids=12) for pos in (20, 45)] for c in range(B)]
    for c in range(B):
        assert np.abs(first[c][0][0]).max() > 0 and np.abs(first[c][1][0]).max() > 0, ("the first search left no row there", c)
    assert sorted([int(t) for t in first[c][0][1]] for c in range(B)) == sorted(ids for ids, _ in want[0])      # pool slots in the order they filled
    got, info = queue(g, prompts, limits, 1, 1, **kw)
    assert_equal(got, want, "reuse")
    for c in range(B):
        k20, pool = g.read_column_state(c, 20, n_ids=20)
        k45, _ = g.read_column_state(c, 45)
        assert not np.array_equal(k20, first[c][0][0]), ("the second search did not write row 20 of column", c)
        assert np.array_equal(k45, first[c][1][0]), ("row 45 is not the first search's", c)
        assert [int(t) for t in pool] in [ids for ids, _ in want[1]], ("pool row", c)
    assert info["slot"] == [0, 0] and info["admit_step"] == [0, 12] and info["steps"] == [12, 20]
    assert info["stats"]["admissions"] == 2 and info["stats"]["steps"] == 32 and info["stats"]["columns"] == 1


# ---- 4. matrix-core route and bucket jumps ----

def test_50_columns_take_the_matrix_core_steps(pkg, models):
    """Ten slots of five beams: 50 columns, at the decode steps' matrix-core threshold; 14 requests, so four slots are refilled."""
    g = models["q4_0"]
    prompts = [prompt_of(5 + r % 11, 800 + r) for r in range(14)]
    limits = [3 + (5 * r) % 9 for r in range(14)]
    kw = dict(n_beams=5, eos_id=-1, length_penalty=1.0, early_stopping=True, n_batch=8)
    want = alone(g, prompts, limits, **kw)
    got, info = queue(g, prompts, limits, 10, 4, **kw)
    assert_equal(got, want, "50 columns")
    assert info["steps"] == limits and info["stats"]["columns"] == 10 and info["stats"]["admissions"] >= 2 and max(info["slot"]) == 9
    assert check_plan(pkg, info, prompts, limits, 10, 4)


JUMP_LENS = (7, 12, 9, 70, 300, 1000)
JUMP_LIMITS = [8, 8, 8, 10, 8, 64]


def test_long_requests_follow_short_ones_through_every_bucket(pkg, models, monkeypatch):
    """Two slots of short requests; then the queue holds a 70-token prompt (its steps cross the 64-key bucket), a 300-token prompt (the 257 .. 512 kernels)
    and a 1000-token prompt that asks for 64 steps and is clamped to 24 -- alone: its neighbours keep their own limits.  Captured steps and eager ones."""
    g = models["q4_0"]
    prompts = [prompt_of(n, 700 + n) for n in JUMP_LENS]
    kw = dict(n_beams=3, eos_id=-1, length_penalty=1.0, early_stopping=True, n_batch=8)
    monkeypatch.delenv("BIOGPT_HIP_NO_GRAPH", raising=False)
    g.refresh_options()
    want = alone(g, prompts, JUMP_LIMITS, **kw)
    assert [max(len(ids) for ids, _ in w) for w in want] == [8, 8, 8, 10, 8, 24]
    try:
        for env in ({}, {"BIOGPT_HIP_NO_GRAPH": "1"}):
            monkeypatch.delenv("BIOGPT_HIP_NO_GRAPH", raising=False)
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            g.refresh_options()
            got, info = queue(g, prompts, JUMP_LIMITS, 2, 4, **kw)
            assert_equal(got, want, ("jumps", env))
            assert info["steps"] == [8, 8, 8, 10, 8, 24]
            assert check_plan(pkg, info, prompts, JUMP_LIMITS, 2, 4)
    finally:
        monkeypatch.delenv("BIOGPT_HIP_NO_GRAPH", raising=False)
        g.refresh_options()


# ---- 5. trie ----

EOS = 2
_rng = np.random.default_rng(77)
POOL = [int(t) for t in _rng.choice(np.arange(100, V), 12, replace=False)]
ENTRIES = [[int(t) for t in _rng.choice(POOL, int(_rng.integers(2, 6)))] for _ in range(36)]      # three dozen entries of 2 - 5 tokens over a 12-token pool


def test_trie_searches_equal_the_request_alone(pkg, models):
    """2 slots x 4 beams, 6 requests, limits below and above the entries' lengths: every request is generate_beam(prompt, trie=...) alone, hypotheses at -inf
    (beams that no entry continues) included."""
    g = models["q4_0"]
    trie = pkg.Trie.build(ENTRIES, V)
    prompts = [prompt_of(5 + 3 * r, 900 + r) for r in range(6)]
    limits = [8, 3, 8, 2, 6, 8]
    kw = dict(n_beams=4, eos_id=EOS, length_penalty=1.0, early_stopping=False, n_batch=8, trie=trie)
    want = alone(g, prompts, limits, **kw)
    finite = [[ids for ids, s in w if np.isfinite(s)] for w in want]
    for r, f in enumerate(finite):      # (the fixture: a finished finite hypothesis is an entry + EOS; one cut by the limit is a prefix of an entry)
        for ids in f:
            body = ids[:-1] if ids[-1] == EOS else ids
            assert any(e[:len(body)] == body for e in ENTRIES), (r, ids)
    for group in (1, 4):
        got, info = queue(g, prompts, limits, 2, group, **kw)
        assert_equal(got, want, ("trie", group))
        check_steps(want, info["steps"], limits, ("trie", group))
        print("trie, group %d: steps %s of %s" % (group, info["steps"], limits))
        assert any(s < n for s, n in zip(info["steps"], limits)), ("fixture problem: no constrained search stops before its limit", info["steps"])
        check_plan(pkg, info, prompts, limits, 2, group)
    free, _ = queue(g, prompts[:2], limits[:2], 2, 4, **dict(kw, trie=None))      # the same context without the trie: other graphs, other results
    assert free != want[:2]
    trie.close()


# ---- 6. captured and eager steps agree ----

def test_captured_and_eager_steps_agree(pkg, models, one_refs, monkeypatch):
    g = models["q4_0"]
    eos, want = one_refs("q4_0", 5, True, 1.0)
    kw = dict(n_beams=5, eos_id=eos, length_penalty=1.0, early_stopping=True, n_batch=8)
    runs = []
    try:
        for env in ({}, {"BIOGPT_HIP_NO_GRAPH": "1"}):
            monkeypatch.delenv("BIOGPT_HIP_NO_GRAPH", raising=False)
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            g.refresh_options()
            runs.append(queue(g, ONE_PROMPTS, ONE_LIMITS, 3, 4, **kw))
            assert_equal(runs[-1][0], want, ("paths", env))
    finally:
        monkeypatch.delenv("BIOGPT_HIP_NO_GRAPH", raising=False)
        g.refresh_options()
    assert runs[0] == runs[1]      # the infos too: steps, schedule, stats


# ---- degenerate queues and the errors that need a model ----

def test_degenerate_queues(models):
    g = models["q4_0"]
    kw = dict(n_beams=3, eos_id=-1, length_penalty=1.0, early_stopping=True, n_batch=8)
    prompts = [prompt_of(8 + 3 * r, 950 + r) for r in range(3)]
    want = alone(g, prompts, [9, 9, 9], **kw)
    got, info = queue(g, prompts, [9, 9, 9], 8, 4, **kw)      # fewer requests than slots; max_columns no multiple of n_beams below
    assert_equal(got, want, "few")
    assert info["stats"] == dict(columns=3, steps=9, groups=3, admissions=1, prompt_columns=sum(len(p) for p in prompts), busy_column_steps=27, column_steps=27)
    hyps, info, _ = g.generate_beam_queue(prompts, 9, max_columns=8, group=4, **kw)
    assert [norm(h) for h in hyps] == want and info["stats"]["columns"] == 2
    full = [2] * KW["n_positions"]      # a prompt that fills the position table: no slot, no hypotheses, the others unaffected
    got, info = queue(g, [prompts[0], full, prompts[1]], [9, 9, 0], 2, 4, **kw)
    assert got == [want[0], [], []] and info["slot"] == [0, -1, -1] and info["admit_step"] == [0, -1, -1] and info["steps"] == [9, 0, 0]
    got, info = queue(g, [full, full], [4, 4], 2, 4, **kw)
    assert got == [[], []] and info["stats"]["steps"] == 0 and info["slot"] == [-1, -1]


def test_model_dependent_argument_errors(pkg, files, models):
    f = pkg.BiogptModel.load(files["f32"])
    with pytest.raises(pkg.BiogptError, match="fast chain"):
        f.generate_beam_queue([[2, 5, 7]], 4)
    f.close()
    g = models["q4_0"]
    with pytest.raises(pkg.BiogptError, match="out of range"):
        g.generate_beam_queue([[2, 5], [2, V]], 4)
    with pytest.raises(pkg.BiogptError, match="eos_id"):
        g.generate_beam_queue([[2, 5]], 4, eos_id=V)
    with pytest.raises(pkg.BiogptError, match="n_positions"):
        g.generate_beam_queue([[2] * (KW["n_positions"] + 1)], 4)
    other = pkg.Trie.build([[3, 4], [5]], 100)
    with pytest.raises(pkg.BiogptError, match="n_vocab"):
        g.generate_beam_queue([[2, 5]], 4, trie=other)
    other.close()
    hyps, _, _ = g.generate_beam_queue([[2, 5, 7]], 4)      # still usable; the defaults
    assert norm(hyps[0]) == norm(g.generate_beam([2, 5, 7], 4)[0])


# ---- 7. neutrality ----

def test_context_cache_and_a_following_closed_call_are_untouched(pkg, files):
    g = pkg.BiogptModel.load(files["q4_0"])
    h = pkg.BiogptModel.load(files["q4_0"])
    ctx_toks = prompt_of(9, 7)
    row = g.eval(ctx_toks, 0)
    h.eval(ctx_toks, 0)
    D = KW["d_model"]
    k0, v0 = g.read_kv(0, 0, 3 * KW["n_positions"] * D), g.read_kv(1, 0, 3 * KW["n_positions"] * D)
    closed = [prompt_of(7, 31), prompt_of(13, 32), prompt_of(21, 33)]
    kw = dict(n_beams=4, eos_id=-1, n_batch=8)
    before = [norm(x) for x in g.generate_beam_batch(closed, 12, **kw)[0]]
    hyps, info, _ = g.generate_beam_queue([prompt_of(17, 8), prompt_of(5, 9), prompt_of(11, 10)], 12, max_columns=8, group=4, **kw)
    assert [len(x) for x in hyps] == [4, 4, 4] and info["stats"]["admissions"] == 2 and info["stats"]["columns"] == 2
    after = [norm(x) for x in g.generate_beam_batch(closed, 12, **kw)[0]]
    assert before == after
    assert np.array_equal(g.read_kv(0, 0, k0.size), k0) and np.array_equal(g.read_kv(1, 0, v0.size), v0)
    assert np.array_equal(g.read_logits(), row)
    nxt = [123]
    assert np.array_equal(g.eval(nxt, len(ctx_toks)), h.eval(nxt, len(ctx_toks)))      # the position too
    g.close()
    h.close()
