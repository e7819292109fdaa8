"""Queue sessions (biogpt_hip_queue_open ...: submit, poll, stream and cancel while steps run) on the GPU.  The reference of every request is the unchanged closed
call of the request ALONE -- generate_sample(<its sampler and rules>, prefix=, logprobs=), cut by the stop rule of tests/queue_requests_ref.py -- and, for a
script that submits everything up front, the unchanged generate_queue(params=); the schedule is held to biogpt_hip_queue_plan_script on the realised lengths.
The two kernels a session adds (queue_stream_kernel, queue_cancel_kernel) are held alone, through their probes, to integer logic on constructed columns, every
output word and every guard byte.  No tolerance anywhere: every comparison is equality of ids, integers and float32 bit patterns.

Fixture conditions (asserted where the fixtures are made): the stop sequence of the fourth parameter set fires before its request's limit, and the rules bite."""
import numpy as np
import pytest

import queue_requests_ref as qref

pytestmark = pytest.mark.gpu

KW = dict(n_vocab=42384, n_layer=3, n_head=16, n_positions=1024, d_ff=4096, d_model=1024, n_merges=40000)
HOT = dict(top_k=40, top_p=0.95, temp=6.0)      # the sampler of tests/test_gpu_queue_requests.py: decisions stay off their borders
GREEDY = dict(top_k=1)
RULE_KEYS = ("repetition_penalty", "no_repeat_ngram_size", "min_new_tokens", "suppress_tokens")
R = 12
LENS = [2, 13, 5, 9, 3, 12, 7, 4, 11, 6, 8, 10]
LIMITS = [10, 3, 7, 1, 9, 5, 2, 8, 4, 6, 10, 5]
SEEDS = [900 + r for r in range(R)]


def prompt_of(n, seed, V=KW["n_vocab"]):
    rng = np.random.default_rng(seed)
    return [2] + [int(v) for v in rng.integers(4, V, n - 1)]


PROMPTS = [prompt_of(n, 40 + n) for n in LENS]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@pytest.fixture(scope="module")
def files(pkg, tmp_path_factory):
    d = tmp_path_factory.mktemp("queue_session")
    f32 = str(d / "f32.bin")
    pkg.write_synthetic(f32, **KW)
    out = {}
    for name in ("q4_0", "q5_1"):
        out[name] = str(d / (name + ".bin"))
        pkg.quantize_file(f32, out[name], name)
    return out


@pytest.fixture(scope="module")
def q40(pkg, files):
    g = pkg.BiogptModel.load(files["q4_0"])
    yield g
    g.close()


def sampler_of(par):
    return dict(top_k=par.get("top_k", 1), top_p=par.get("top_p", 0.9), temp=par.get("temp", 0.9), eos_id=par.get("eos_id", -1))


def free_run(g, prompt, n, seed, par, logprobs=None, prefix=None):
    kw = dict(sampler_of(par), seeds=[seed], n_batch=8, **{k: par[k] for k in RULE_KEYS if k in par})
    if prefix is not None:
        kw["prefix"] = prefix
    if logprobs is None:
        ids, _ = g.generate_sample([prompt], n, **kw)
        return [int(t) for t in ids[0]], None
    ids, info, _ = g.generate_sample([prompt], n, logprobs=logprobs, **kw)
    return [int(t) for t in ids[0]], info[0]


def references(g, ruled, logprobs=None):
    """(pars, want): the twelve requests' parameters -- request r carries set r % 4 -- and each request alone as (ids, finish, logprobs rows or None).  ruled:
    four sets, two with rules and one with a stop sequence; otherwise four sets without rules (log-probabilities know none), one with a stop sequence.  The stop
    sequence is taken from the free run of request 7 (limit 8), where it fires; the suppressed ids are the first tokens of the greedy runs of the requests that
    carry them, so that rule bites in each."""
    sets = [HOT, dict(HOT, repetition_penalty=1.3), None, None] if ruled else [HOT, dict(top_k=10, top_p=0.8, temp=2.0), GREEDY, None]
    firsts = {}
    if ruled:
        firsts = {r: free_run(g, PROMPTS[r], LIMITS[r], SEEDS[r], GREEDY)[0][0] for r in (2, 6, 10)}
        sets[2] = dict(GREEDY, no_repeat_ngram_size=2, suppress_tokens=sorted(set(firsts.values())))
    free7, _ = free_run(g, PROMPTS[7], LIMITS[7], SEEDS[7], HOT)
    sets[3] = dict(HOT, stop=[[free7[2], free7[3]]])
    pars = [sets[r % 4] for r in range(R)]
    want = []
    for r in range(R):
        ids, rows = free_run(g, PROMPTS[r], LIMITS[r], SEEDS[r], pars[r], logprobs=logprobs)
        cut, reason = qref.stop_cut(ids, pars[r].get("stop", ()), -1)
        want.append((cut, reason, None if rows is None else tuple(a[:len(cut)] for a in rows)))
    assert want[7][1] == 2 and len(want[7][0]) <= 4 < LIMITS[7], "fixture problem: the stop sequence does not fire: %s" % (want[7],)
    for r, first in firsts.items():
        assert want[r][0][0] != first, "fixture problem: the suppressed id does not bite (request %d)" % r
    return pars, want


@pytest.fixture(scope="module")
def ruled(q40):
    return references(q40, True)


@pytest.fixture(scope="module")
def bare(q40):
    return references(q40, False, logprobs=3)


def run_script(pkg, g, script, pars, prompts=PROMPTS, limits=LIMITS, seeds=SEEDS, **session_kw):
    """Runs ("submit", r) / ("poll", n) / ("cancel", r) / ("drain",) on a fresh session.  Returns (events with "poll" added -- the index of the poll that delivered
    each --, the ids by request in submission order, the planner's ops as executed, the session's stats)."""
    events, order, ops, polls = [], [], [], [0]
    n_predict = session_kw.pop("n_predict", max(limits))
    with g.queue_session(n_predict=n_predict, **session_kw) as s:
        def poll(n):
            got = s.poll(n)
            ops.append((pkg.POLL, n))
            polls[0] += 1
            for e in got:
                events.append(dict(e, poll=polls[0]))
        for op in script:
            if op[0] == "submit":
                r = op[1]
                assert s.submit(prompts[r], limits[r], seeds[r], pkg.request_params(**pars[r])) == len(order)
                order.append(r)
                ops.append((pkg.SUBMIT,))
            elif op[0] == "cancel":
                s.cancel(op[1])
                ops.append((pkg.CANCEL, op[1]))
            elif op[0] == "poll":
                poll(op[1])
            else:
                while not s.idle():
                    poll(1)
        stats = s.stats()
    return events, order, ops, stats


def finals(events):
    return {e["id"]: e for e in events if e["kind"] != "delta"}


def check_alone(events, order, want, logprobs=False, skip=()):
    fin = finals(events)
    assert sorted(fin) == list(range(len(order)))
    for i, r in enumerate(order):
        if i in skip:
            continue
        e = fin[i]
        assert e["kind"] == "finished" and e["first"] == 0
        assert e["ids"].tolist() == want[r][0], (r, e["ids"].tolist(), want[r][0])
        assert e["finish"] == want[r][1], (r, e["finish"], want[r][1])
        if logprobs:
            lp, tid, tlp = e["logprobs"]
            assert np.array_equal(bits(lp), bits(want[r][2][0])) and np.array_equal(tid, want[r][2][1]) and np.array_equal(bits(tlp), bits(want[r][2][2])), r


def check_plan(pkg, events, order, ops, want, limits, max_columns, group, stats=None, prompt_columns=None):
    fin = finals(events)
    plan = pkg.queue_plan_script(ops, [len(want[r][0]) for r in order], [limits[r] for r in order], max_columns, group)
    assert [fin[i]["admit_step"] for i in range(len(order))] == plan["admit_step"] and [fin[i]["column"] for i in range(len(order))] == plan["column"]
    assert [len(fin[i]["ids"]) for i in range(len(order))] == plan["lens"]
    if stats is not None:
        assert stats["stats"] == dict(plan["stats"], prompt_columns=prompt_columns)
    return plan


ONE_PER_POLL = [op for r in range(R) for op in (("submit", r), ("poll", 1))] + [("drain",)]
BURSTS = ([("submit", r) for r in range(0, 5)] + [("drain",), ("poll", 1)] + [("submit", r) for r in range(5, 10)] + [("poll", 2), ("drain",), ("poll", 1), ("poll", 3)]
          + [("submit", r) for r in range(10, 12)] + [("drain",)])


# ---- 1. all up front: the closed call ----

@pytest.mark.parametrize("name, max_columns, group", [("q4_0", 3, 1), ("q4_0", 3, 4), ("q4_0", 8, 1), ("q4_0", 8, 4), ("q5_1", 3, 4)])
def test_all_up_front_is_the_closed_call(pkg, files, q40, ruled, name, max_columns, group):
    g = q40 if name == "q4_0" else pkg.BiogptModel.load(files[name])
    pars = ruled[0]
    events, order, ops, stats = run_script(pkg, g, [("submit", r) for r in range(R)] + [("drain",)], pars, max_columns=max_columns, group=group)
    ids, info, _ = g.generate_queue(PROMPTS, max(LIMITS), max_columns=max_columns, group=group, seeds=SEEDS, n_predicts=LIMITS, params=[pkg.request_params(**p) for p in pars])
    fin = finals(events)
    for r in range(R):
        e = fin[r]
        assert e["kind"] == "finished" and e["ids"].tolist() == ids[r].tolist(), r
        assert (e["finish"], e["admit_step"], e["column"]) == (info["finish"][r], info["admit_step"][r], info["column"][r]), r
    assert stats["stats"] == info["stats"] and (stats["submitted"], stats["pending"], stats["running"]) == (R, 0, 0)
    if name == "q4_0":
        check_alone(events, order, ruled[1])
    else:
        g.close()


# ---- 2. arrivals ----

@pytest.mark.parametrize("max_columns", [1, 3, 8])
@pytest.mark.parametrize("script", [ONE_PER_POLL, BURSTS], ids=["one_per_poll", "bursts"])
def test_arrivals_equal_the_request_alone(pkg, q40, ruled, script, max_columns):
    pars, want = ruled
    events, order, ops, stats = run_script(pkg, q40, script, pars, max_columns=max_columns, group=4)
    check_alone(events, order, want)
    check_plan(pkg, events, order, ops, want, LIMITS, max_columns, 4, stats, sum(LENS))
    if max_columns == 1:
        assert all(e["column"] == 0 for e in finals(events).values())


# ---- 3. streaming ----

@pytest.mark.parametrize("logprobs", [None, 3])
def test_streaming_deltas_are_the_final_rows(pkg, q40, ruled, bare, logprobs):
    pars, want = ruled if logprobs is None else bare
    kw = dict(max_columns=3, group=4) if logprobs is None else dict(max_columns=3, group=4, logprobs=3)
    events, order, ops, _ = run_script(pkg, q40, BURSTS, pars, stream=True, **kw)
    check_alone(events, order, want, logprobs=logprobs is not None)
    done, parts = set(), {}
    for e in events:
        if e["kind"] != "delta":
            done.add(e["id"])
            continue
        assert e["id"] not in done, "a delta behind the finished event of request %d" % e["id"]
        have = parts.setdefault(e["id"], [])
        assert e["first"] == sum(len(p["ids"]) for p in have) and 1 <= len(e["ids"]) <= 4, e
        have.append(e)
    fin = finals(events)
    for i in range(R):
        assert np.array_equal(np.concatenate([p["ids"] for p in parts[i]]), fin[i]["ids"]), i
        if logprobs is not None:
            for j in range(3):
                got = np.concatenate([p["logprobs"][j] for p in parts[i]])
                assert np.array_equal(got.view(np.int32), fin[i]["logprobs"][j].view(np.int32)), (i, j)
    # without stream: the same finished events, in the same polls
    plain, _, _, _ = run_script(pkg, q40, BURSTS, pars, **kw)
    assert all(e["kind"] == "finished" for e in plain)
    kept = [e for e in events if e["kind"] != "delta"]
    assert len(plain) == len(kept)
    for a, b in zip(plain, kept):
        assert {k: v for k, v in a.items() if k not in ("ids", "logprobs")} == {k: v for k, v in b.items() if k not in ("ids", "logprobs")}
        assert np.array_equal(a["ids"], b["ids"])
        if logprobs is not None:
            assert all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(a["logprobs"], b["logprobs"]))


# ---- 4. cancel ----

def test_cancel_pending_and_running(pkg, q40, bare):
    pars, want = bare
    script = [("submit", r) for r in range(R)] + [("poll", 1), ("cancel", 11), ("cancel", 0), ("poll", 1), ("drain",)]
    events, order, ops, stats = run_script(pkg, q40, script, pars, max_columns=3, group=4, logprobs=3)
    fin = finals(events)
    # request 0 (limit 10, no stop) had run one group of 4 steps: a prefix of itself alone, at the poll behind the cancel, and its column is refilled there
    e = fin[0]
    assert (e["kind"], e["poll"], e["finish"], e["column"], e["admit_step"]) == ("cancelled", 2, -1, 0, 0)
    assert e["ids"].tolist() == want[0][0][:4] and len(want[0][0]) == 10
    assert all(np.array_equal(a.view(np.int32), b[:4].view(np.int32)) for a, b in zip(e["logprobs"], want[0][2]))
    assert [i for i in range(R) if fin[i]["column"] == 0 and fin[i]["admit_step"] == 4] != [], "column 0 was not refilled at the cancel's poll"
    # request 11 was pending: never admitted
    e = fin[11]
    assert (e["kind"], e["poll"], len(e["ids"]), e["column"], e["admit_step"], e["finish"]) == ("cancelled", 2, 0, -1, -1, -1)
    # everybody else: the request alone, bit for bit
    check_alone(events, order, want, logprobs=True, skip=(0, 11))
    plan = check_plan(pkg, events, order, ops, want, LIMITS, 3, 4)
    assert plan["lens"][0] == 4 and plan["lens"][11] == 0
    assert stats["stats"]["busy_column_steps"] == sum(len(fin[i]["ids"]) for i in range(R))


def test_cancel_of_a_finished_or_unknown_request_is_an_error(pkg, q40, bare):
    pars, want = bare
    with q40.queue_session(max_columns=2, group=4, n_predict=10) as s:
        a = s.submit(PROMPTS[3], 1, SEEDS[3], pkg.request_params(**pars[3]))
        b = s.submit(PROMPTS[0], 10, SEEDS[0], pkg.request_params(**pars[0]))
        got = s.poll(1)
        assert [(e["id"], e["kind"]) for e in got] == [(a, "finished")]
        for bad, why in ((a, "has finished or was cancelled"), (7, "no request 7"), (-1, "no request -1")):
            with pytest.raises(pkg.BiogptError, match=why):
                s.cancel(bad)
        s.cancel(b)
        with pytest.raises(pkg.BiogptError, match="has finished or was cancelled"):
            s.cancel(b)
        got = s.poll(1)
        assert [(e["id"], e["kind"], e["ids"].tolist()) for e in got] == [(b, "cancelled", want[0][0][:4])]
        assert s.idle()
        # a request's own n_predict is held against the session's
        for n, why in ((-1, r"n_predict \(-1\) must be in \[0, the session's n_predict = 10\]"), (11, r"n_predict \(11\) must be in")):
            with pytest.raises(pkg.BiogptError, match=why):
                s.submit(PROMPTS[0], n)
        with pytest.raises(pkg.BiogptError, match="empty prompt"):
            s.submit([], 4)


# ---- 5. behind a prefix ----

def test_behind_a_prefix(pkg, q40):
    g = q40
    prefix = prompt_of(17, 41)
    suffixes = [prompt_of(n + 1, 700 + n)[1:] for n in (0, 5, 11, 3, 8)]
    limits, seeds = [6, 10, 4, 8, 5], [81, 82, 83, 84, 85]
    pars = [GREEDY, HOT, dict(top_k=10, top_p=0.8, temp=2.0), HOT, HOT]
    want = []
    for r in range(5):
        ids, rows = free_run(g, suffixes[r], limits[r], seeds[r], pars[r], logprobs=0, prefix=prefix)
        want.append((ids, 0, rows))
    script = [("submit", 0), ("submit", 1), ("poll", 1), ("submit", 2), ("submit", 3), ("submit", 4), ("drain",)]
    events, order, ops, stats = run_script(pkg, g, script, pars, prompts=suffixes, limits=limits, seeds=seeds, max_columns=2, group=4, prefix=prefix, logprobs=0, n_batch=8)
    check_alone(events, order, want, logprobs=True)
    check_plan(pkg, events, order, ops, want, limits, 2, 4, stats, 16 + sum(1 + len(s) for s in suffixes))


# ---- 6. idle and reuse ----

def test_idle_polls_and_reuse(pkg, q40, ruled):
    pars, want = ruled
    with q40.queue_session(max_columns=2, group=4, n_predict=10) as s:
        assert s.poll(3) == [] and s.stats()["stats"]["steps"] == 0 and s.idle()
        first = [s.submit(PROMPTS[r], LIMITS[r], SEEDS[r], pkg.request_params(**pars[r])) for r in (0, 1, 2)]
        got = [e for events in s.drain() for e in events]
        steps = s.stats()["stats"]["steps"]
        assert steps > 0 and s.poll(5) == [] and s.stats()["stats"]["steps"] == steps
        again = [s.submit(PROMPTS[r], LIMITS[r], SEEDS[r], pkg.request_params(**pars[r])) for r in (4, 5, 6, 0)]
        got += [e for events in s.drain(max_groups=2) for e in events]
        assert first + again == list(range(7))
    for i, r in enumerate((0, 1, 2, 4, 5, 6, 0)):
        e = next(e for e in got if e["id"] == i)
        assert e["kind"] == "finished" and e["ids"].tolist() == want[r][0] and e["finish"] == want[r][1] and e["column"] in (0, 1), (i, r)
    # a request without room for a token: finished with length 0 at the next poll, no column
    with q40.queue_session(max_columns=2, group=4, n_predict=10, top_k=40, top_p=0.95, temp=6.0) as s:
        s.submit(PROMPTS[0], 0)
        s.submit(PROMPTS[4], LIMITS[4], SEEDS[4])      # the session's default sampler: HOT
        got = s.poll(1)
        assert (got[0]["id"], got[0]["kind"], len(got[0]["ids"]), got[0]["column"], got[0]["finish"]) == (0, "finished", 0, -1, -1)
        got += [e for events in s.drain() for e in events]
        assert next(e for e in got if e["id"] == 1)["ids"].tolist() == want[4][0]      # (request 4's set is HOT alone)


# ---- 7. exclusivity and lifetime ----

def test_exclusive_use_and_lifetime(pkg, q40, ruled):
    g = q40
    pars, want = ruled
    s = g.queue_session(max_columns=2, group=2, n_predict=10)
    s.submit(PROMPTS[0], 10, SEEDS[0], pkg.request_params(**pars[0]))
    s.poll(1)
    assert s.stats()["running"] == 1
    for call in (lambda: g.score_batch([PROMPTS[1]]), lambda: g.generate_sample([PROMPTS[1]], 4, **HOT), lambda: g.eval(PROMPTS[1], 0),
                 lambda: g.generate_queue([PROMPTS[1]], 4), lambda: g.queue_session(max_columns=2)):
        with pytest.raises(pkg.BiogptError, match="a queue session is open on this context"):
            call()
    s.close()      # with request 0 still running: dropped
    for call in (lambda: s.poll(), lambda: s.submit(PROMPTS[1]), lambda: s.cancel(0)):
        with pytest.raises(pkg.BiogptError, match="the queue session is closed"):
            call()
    assert np.isfinite(g.eval(PROMPTS[1], 0)).all()
    g.score_batch([PROMPTS[1]])
    ids, _ = g.generate_sample([PROMPTS[0]], LIMITS[0], seeds=[SEEDS[0]], **HOT)
    assert ids[0].tolist() == want[0][0]
    ids, info, _ = g.generate_queue(PROMPTS, max(LIMITS), max_columns=2, group=2, seeds=SEEDS, n_predicts=LIMITS, params=[pkg.request_params(**p) for p in pars])
    assert [s_.tolist() for s_ in ids] == [w[0] for w in want] and info["finish"] == [w[1] for w in want]


def test_model_dependent_refusals(pkg, files, q40):
    f32 = files["q4_0"].replace("q4_0.bin", "f32.bin")
    g = pkg.BiogptModel.load(f32)
    with pytest.raises(pkg.BiogptError, match="a queue session needs the BioGPT-base fast chain"):
        g.queue_session(max_columns=2)
    g.close()
    V, P = KW["n_vocab"], KW["n_positions"]
    with pytest.raises(pkg.BiogptError, match="eos_id %d out of range" % V):
        q40.queue_session(eos_id=V)
    with pytest.raises(pkg.BiogptError, match=r"max_len \(%d\) exceeds n_positions" % (P + 1)):
        q40.queue_session(max_len=P + 1)
    with q40.queue_session(max_columns=2, n_predict=8, max_len=64, logprobs=1) as s:
        with pytest.raises(pkg.BiogptError, match="more than the session's max_len"):
            s.submit(prompt_of(60, 3), 8)
        with pytest.raises(pkg.BiogptError, match="logprobs with generation rules"):
            s.submit(PROMPTS[0], 4, params=pkg.request_params(no_repeat_ngram_size=2))
        with pytest.raises(pkg.BiogptError, match=r"token id %d \(request 0, position 1\) out of range" % V):
            s.submit([2, V], 4)
        assert s.stats()["submitted"] == 0


# ---- 8. the two kernels alone ----

def stream_expectation(n_gen, rows, g, guard, lp=None, tid=None, tlp=None):
    C, stride = rows.shape
    parts = [np.zeros(C, np.int32), np.full((C, g), -1, np.int32)]
    if lp is not None:
        K, lps = tid.shape[2], lp.shape[1]
        parts += [np.zeros((C, g), np.float32), np.full((C, g, K), -1, np.int32), np.zeros((C, g, K), np.float32)]
    for c in range(C):
        n = max(0, min(int(n_gen[c]), stride))
        w = min(g, n)
        parts[0][c] = n
        parts[1][c, :w] = rows[c, n - w:n]
        if lp is not None:
            for j in range(w):
                e = n - w + j
                if e < lps:
                    parts[2][c, j], parts[3][c, j], parts[4][c, j] = lp[c, e], tid[c, e], tlp[c, e]
    out = b""
    for p in parts:
        raw = p.tobytes()
        out += raw + b"\xff" * (-len(raw) % 16)
    return np.frombuffer(out + b"\xff" * guard, dtype=np.uint8)


@pytest.mark.parametrize("K", [None, 0, 1, 8])
def test_the_stream_kernel_alone(pkg, K):
    stride, lps, guard = 80, 70, 256
    rng = np.random.default_rng(5 if K is None else 50 + K)
    for g in (1, 4, 64):
        for C in (1, 63, 64, 65, 512):
            cases = [0, 1, g - 1, g, g + 1, stride, stride + 5, -3]
            n_gen = np.asarray([cases[(c + g) % len(cases)] for c in range(C)], dtype=np.int32)
            rows = rng.integers(0, 42384, (C, stride)).astype(np.int32)
            kw = {}
            if K is not None:
                kw = dict(lp=rng.standard_normal((C, lps)).astype(np.float32), top_ids=rng.integers(0, 42384, (C, lps, K)).astype(np.int32),
                          top_lp=rng.standard_normal((C, lps, K)).astype(np.float32))
            block, used = pkg.queue_stream_rows(n_gen, rows, g, guard=guard, **kw)
            want = stream_expectation(n_gen, rows, g, guard, kw.get("lp"), kw.get("top_ids"), kw.get("top_lp"))
            assert used + guard == block.size == want.size, (g, C, used, block.size, want.size)
            assert (block[used:] == 0xff).all(), "guard bytes behind the block were written (g %d, C %d)" % (g, C)
            assert np.array_equal(block, want), (g, C, np.flatnonzero(block != want)[:8].tolist())


def test_the_cancel_kernel_alone(pkg):
    Q = 512
    rng = np.random.default_rng(9)
    finished = np.zeros(Q, np.int32)
    finished[[9, 40, 511]] = 1
    n_gen = rng.integers(1, 30, Q).astype(np.int32)
    hdr = np.zeros(1 + 2 * Q, np.int32)
    hdr[0] = Q - 3
    for c in (9, 40, 511):
        hdr[1 + c], hdr[1 + Q + c] = 1, 77      # reported when they finished: their words stay
    want_fin, want_hdr = finished.copy(), hdr.copy()
    cols = [5, 9, 600, -1, 5, 510, 512]      # live, finished already, out of range twice, the live one again, another live one, one past the last column
    for c in (5, 510):
        want_fin[c], want_hdr[1 + c], want_hdr[1 + Q + c] = 1, 1, n_gen[c]
    want_hdr[0] = Q - 5
    pkg.queue_cancel_cols(cols, finished, n_gen, hdr)
    assert np.array_equal(finished, want_fin), np.flatnonzero(finished != want_fin).tolist()
    assert np.array_equal(hdr, want_hdr), np.flatnonzero(hdr != want_hdr).tolist()
