"""Queued generation whose requests carry their own parameters (biogpt_hip_generate_queue_requests, queue_req_rows_kernel) on the GPU.  The step kernel alone
(biogpt_hip_queue_req_rows_device) is held, column by column, to rules_ref.apply_rules on the row, the sampler restatement (oracle/sampler.py with
std::mt19937, as tests/sample_ref.py uses it) and integer logic for the states, the generators and the header.  The call is held to the unchanged closed call
of each request ALONE with the request's parameters -- generate_sample(<sampler>, <rules>) -- cut by the stop rule of tests/queue_requests_ref.py, to the plan
of the realised lengths, and, where every request carries the same sampler and nothing else, to the unchanged generate_queue.  No tolerance anywhere: every
comparison is equality of ids, lengths, integers and float32 bit patterns."""
import ctypes

import numpy as np
import pytest

import queue_requests_ref as qref
import rules_ref
import sample_ref
from oracle import sampler

pytestmark = pytest.mark.gpu

KW = dict(n_vocab=42384, n_layer=3, n_head=16, n_positions=1024, d_ff=4096, d_model=1024, n_merges=40000)
WIDE_B = dict(n_vocab=77, n_layer=1, n_head=3, n_positions=40, d_ff=96, d_model=192, n_merges=3)      # file B of tests/test_gpu_wide_chain.py
HOT = dict(top_k=40, top_p=0.95, temp=6.0)
GREEDY = dict(top_k=1)
MARGIN = 1e-9          # separates the device's exp() rounding from a wrong choice (tests/test_gpu_sample.py)
RULE_KEYS = ("repetition_penalty", "no_repeat_ngram_size", "min_new_tokens", "suppress_tokens")


def prompt_of(n, seed, V=KW["n_vocab"]):
    rng = np.random.default_rng(seed)
    return [2] + [int(v) for v in rng.integers(4, V, n - 1)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@pytest.fixture(scope="module")
def files(pkg, tmp_path_factory):
    d = tmp_path_factory.mktemp("queue_requests")
    f32 = str(d / "f32.bin")
    pkg.write_synthetic(f32, **KW)
    out = {"f32": f32}
    for name in ("q4_0", "q5_1"):
        out[name] = str(d / (name + ".bin"))
        pkg.quantize_file(f32, out[name], name)
    wide = str(d / "wide_f32.bin")
    pkg.write_synthetic(wide, **WIDE_B)
    out["wide"] = str(d / "wide_q4_0.bin")
    pkg.quantize_file(wide, out["wide"], "q4_0")
    return out


@pytest.fixture(scope="module")
def q40(pkg, files):
    g = pkg.BiogptModel.load(files["q4_0"])
    yield g
    g.close()


def sampler_of(par):
    return dict(top_k=par.get("top_k", 1), top_p=par.get("top_p", 0.9), temp=par.get("temp", 0.9), eos_id=par.get("eos_id", -1))


def free_run(g, prompt, n, seed, par, n_batch=8, logprobs=None):
    """The closed call of the request alone with its sampler and rules (it knows no stop sequences)."""
    kw = dict(sampler_of(par), seeds=[seed], n_batch=n_batch, **{k: par[k] for k in RULE_KEYS if k in par})
    if logprobs is None:
        ids, _ = g.generate_sample([prompt], n, **kw)
        return [int(t) for t in ids[0]]
    ids, info, _ = g.generate_sample([prompt], n, logprobs=logprobs, **kw)
    return [int(t) for t in ids[0]], info[0]


def alone(g, prompt, n, seed, par, n_batch=8):
    """The reference: (ids, finish) of the request by itself -- the closed call, cut by the stop rule."""
    return qref.stop_cut(free_run(g, prompt, n, seed, par, n_batch), par.get("stop", ()), par.get("eos_id", -1))


def queue(pkg, g, prompts, limits, seeds, pars, max_columns, group, **kw):
    ids, info, secs = g.generate_queue(prompts, max(limits), max_columns=max_columns, group=group, seeds=seeds, n_predicts=limits,
                                       params=[pkg.request_params(**p) for p in pars], **kw)
    return [[int(t) for t in s] for s in ids], info


def check_plan(pkg, info, lens, limits, prompt_columns, max_columns, group):
    """admit_step / column / stats are the plan's for the lengths the run had under its limits (the plan knows no prompts: prompt_columns is the run's own)."""
    want = pkg.queue_plan(lens, max_columns, group, limits=limits)
    assert info["admit_step"] == want["admit_step"] and info["column"] == want["column"]
    assert info["stats"] == dict(want["stats"], prompt_columns=prompt_columns)


# ---- 1. the step kernel alone ----

def mt_state(seed, draws=None):
    """The 625 words of std::mt19937(seed): as seeded (draws None: index 624, no block of outputs made yet), or behind the step of a live column, which makes
    the first block and takes `draws` outputs from it."""
    bg = np.random.MT19937()
    bg._legacy_seeding(int(seed))
    if draws is not None:
        bg.random_raw()
    key = np.asarray(bg.state["state"]["key"], dtype=np.uint32)
    return np.concatenate([key, np.asarray([624 if draws is None else draws], dtype=np.uint32)])


def kernel_columns(V):
    """The columns of the kernel-alone test for a vocabulary of V: dicts with the request's parameters, its prompt, its generated tokens so far, its limit, its
    finished flag, its seed and its logits row.  Tokens a, b, c ... are distinct ids; `top` is made the row's largest entry where a case needs the arg-max."""
    rng = np.random.default_rng(7000 + V)
    tok = [int(t) for t in rng.choice(np.arange(4, V), 24, replace=False)]
    a, b, c, d, e, x, y, z, w, q = tok[:10]
    eos = tok[10]
    cols = []

    def col(par, prompt, gen, limit=12, finished=0, top=None):
        row = (3.0 * rng.standard_normal(V)).astype(np.float32)
        if top is not None:
            row[top] = np.float32(20.0)
        cols.append(dict(par=par, prompt=list(prompt), gen=list(gen), limit=limit, finished=finished, seed=8000 + len(cols), row=row))
        return row

    col(GREEDY, tok[11:16], [x, y])                                                                   # 0 greedy: exact, no generator involved
    col(HOT, tok[11:17], [x])                                                                         # 1 sampled
    col(dict(HOT, repetition_penalty=1.3), [a, b, a, c], [d, a])                                      # 2 penalty alone; the repeated token in prompt and generated part
    row = col(dict(GREEDY, repetition_penalty=1.3), [a, b, a, c], [d, a])                             # 3 ... where it moves the arg-max off the penalised token
    row[a] = np.float32(1.2) * row.max()
    col(dict(GREEDY, no_repeat_ngram_size=2), [a, b, c], [a], top=b)                                  # 4 n-gram alone: a was followed by b
    col(dict(GREEDY, no_repeat_ngram_size=3), [a], [b], top=a)                                        # 5 L + 1 == n: no complete n-gram yet
    col(dict(GREEDY, no_repeat_ngram_size=4), [a], [a], top=a)                                        # 6 L + 1 == n - 1: the rule is off
    col(dict(GREEDY, min_new_tokens=3, eos_id=eos), [a, b], [c, d], top=eos)                          # 7 n_gen = m - 1: the EOS is banned
    col(dict(GREEDY, min_new_tokens=3, eos_id=eos), [a, b], [c, d, e], top=eos)                       # 8 n_gen = m: the EOS is drawn and ends the column
    row = col(HOT, [a, b], [c])                                                                       # 9 64 suppress ids: the row's best 64
    cols[-1]["par"] = dict(HOT, suppress_tokens=[int(t) for t in sample_ref.topk_order(row, 64)])
    col(dict(HOT, repetition_penalty=1.2, no_repeat_ngram_size=2, min_new_tokens=5, eos_id=eos, suppress_tokens=tok[16:24]), [a, b, c, a, d], [b, a])      # 10 all rules
    col(dict(GREEDY, stop=[[y, q], [y, z]]), [a, b], [x, y], top=z)                                   # 11 a stop sequence completes on this token
    col(dict(GREEDY, stop=[[z], [y, z]]), [a, b], [x, y], top=z)                                      # 12 two complete at once: the lower index
    col(dict(GREEDY, stop=[[z, w], [x, y, w]]), [a, b], [x, y], top=z)                                # 13 one token short
    col(dict(GREEDY, stop=[[b, y, z]]), [a, b], [y], top=z)                                           # 14 longer than n_gen: it would need the prompt's last token
    col(dict(HOT, repetition_penalty=1.3, stop=[[z]]), [a, b], [x, y], finished=1, top=z)             # 15 finished already: nothing may change
    col(GREEDY, [a, b], [x, y, c], limit=4, top=z)                                                    # 16 reaches its limit
    col(dict(HOT, eos_id=eos, stop=[[eos]]), [a, b], [x], top=eos)                                    # 17 a stop of one token that is the EOS id: the EOS wins
    cols[-1]["par"]["top_k"] = 1
    return cols


def processed_row(c):
    """The column's logits row as its rules leave it (rules_ref.apply_rules; a column without rules: the row itself)."""
    par = c["par"]
    rules = {k: par[k] for k in RULE_KEYS if k in par}
    return rules_ref.apply_rules(c["row"], c["prompt"] + c["gen"], len(c["prompt"]), rules, par.get("eos_id", -1)) if rules else c["row"]


def kernel_expectation(cols, V):
    """What the launch must leave: (states, finished, mt, hdr, ids rows, left-out columns), from the restatements alone."""
    n = len(cols)
    states = np.zeros((n, 8), dtype=np.int32)
    fin = np.zeros(n, dtype=np.int32)
    hdr = np.zeros(1 + 3 * n, dtype=np.int32)
    mt = np.zeros((n, 625), dtype=np.uint32)
    ids = []
    left_out = []
    hdr[0] = sum(1 for c in cols if not c["finished"])
    for r, c in enumerate(cols):
        par, gen = c["par"], c["gen"]
        n_gen, eos = len(gen), par.get("eos_id", -1)
        states[r] = [30 + r, 1000 + r, n_gen, r, 0, 0, 0, 0]
        if c["finished"]:      # reported when it finished, with a reason: all of it stays
            fin[r], hdr[1 + r], hdr[1 + n + r], hdr[1 + 2 * n + r] = 1, 1, n_gen, 5
            mt[r] = mt_state(c["seed"])
            ids.append(gen)
            continue
        row = processed_row(c)
        sp = sampler_of(par)
        rng = sample_ref.RecordingRng(sampler.Mt19937(c["seed"]))
        t = int(sampler.sample_top_k_top_p(row, sp["top_k"], sp["top_p"], sp["temp"], rng))
        if sample_ref.decision_margin(row, sp["top_k"], sp["top_p"], sp["temp"], rng.out) < MARGIN:
            left_out.append(r)
        mt[r] = mt_state(c["seed"], len(rng.out))
        now = gen + [t]
        cut, reason = qref.stop_cut(now, par.get("stop", ()), eos)
        assert cut == now, "fixture problem: column %d's history holds a stop sequence already" % r
        states[r, 2] = n_gen + 1
        if reason != 1:
            states[r, 0] += 1
            states[r, 1] = t
        if reason != 0 or n_gen + 1 >= c["limit"]:
            fin[r], hdr[1 + r], hdr[1 + n + r], hdr[1 + 2 * n + r] = 1, 1, n_gen + 1, reason
            hdr[0] -= 1
        ids.append(now)
    return states, fin, mt, hdr, ids, left_out


def kernel_start(cols):
    n = len(cols)
    states = np.zeros((n, 8), dtype=np.int32)
    hdr = np.zeros(1 + 3 * n, dtype=np.int32)
    hdr[0] = sum(1 for c in cols if not c["finished"])
    for r, c in enumerate(cols):
        states[r] = [30 + r, 1000 + r, len(c["gen"]), r, 0, 0, 0, 0]
        if c["finished"]:
            hdr[1 + r], hdr[1 + n + r], hdr[1 + 2 * n + r] = 1, len(c["gen"]), 5
    return states, np.asarray([c["finished"] for c in cols], dtype=np.int32), np.stack([mt_state(c["seed"]) for c in cols]), hdr


STRIDE, TOP = 6, 3


@pytest.mark.parametrize("V", [42384, 77])
def test_the_step_kernel_alone(pkg, V):
    cols = kernel_columns(V)
    n = len(cols)
    want_states, want_fin, want_mt, want_hdr, want_ids, left_out = kernel_expectation(cols, V)
    print("V %d: finished %s, reasons %s, left out %s" % (V, want_fin.tolist(), want_hdr[1 + 2 * n:].tolist(), left_out))
    assert len(left_out) <= 0, "fixture problem: a decision of columns %s lies within %g of a border" % (left_out, MARGIN)
    # the cases are what their comments say
    assert [int(want_hdr[1 + 2 * n + r]) for r in (8, 11, 12, 15, 16, 17)] == [1, 3, 2, 5, 0, 1] and [r for r in range(n) if want_fin[r]] == [8, 11, 12, 15, 16, 17]
    assert want_ids[3][-1] != cols[3]["prompt"][0] and want_ids[4][-1] != cols[4]["prompt"][1] and want_ids[5][-1] == cols[5]["prompt"][0]
    assert want_ids[6][-1] == cols[6]["prompt"][0] and want_ids[7][-1] != cols[7]["par"]["eos_id"] and want_ids[8][-1] == cols[8]["par"]["eos_id"]
    assert not set(want_ids[9][-1:]) & set(cols[9]["par"]["suppress_tokens"])
    rows = np.stack([c["row"] for c in cols])
    pars = [pkg.request_params(**c["par"]) for c in cols]
    hist = [c["prompt"] + c["gen"] for c in cols]
    # the entries of the log-probability block: sample_lp_rows_kernel alone on each live column's row as apply_rules leaves it, with the column's sampler and seed
    lp_ref = {}
    for r, c in enumerate(cols):
        if not c["finished"]:
            sp = sampler_of(c["par"])
            one = pkg.genlp_rows(processed_row(c)[None, :], TOP, mode=1, top_k=sp["top_k"], top_p=sp["top_p"], temp=sp["temp"], states=mt_state(c["seed"])[None, :].copy())
            assert int(one[0][0]) == want_ids[r][-1], (r, int(one[0][0]), want_ids[r][-1])
            lp_ref[r] = (one[1][0], one[2][0], one[3][0])
    out = {}
    for with_lp in (False, True):
        states, fin, mt, hdr = kernel_start(cols)
        ids, lp, tid, tlp = pkg.queue_req_rows(rows, pars, hist, [len(c["prompt"]) for c in cols], states, [c["limit"] for c in cols], fin, mt, hdr, n_top=TOP,
                                               stride=STRIDE, with_lp=with_lp)
        for r in range(n):
            assert [int(t) for t in ids[r, :len(want_ids[r])]] == want_ids[r], (with_lp, r, ids[r].tolist(), want_ids[r])
            assert (ids[r, len(want_ids[r]):] == -1).all(), (with_lp, r, ids[r].tolist())
            assert np.array_equal(states[r], want_states[r]), (with_lp, r, states[r].tolist(), want_states[r].tolist())
            assert np.array_equal(mt[r], want_mt[r]), (with_lp, r, int(mt[r, 624]), int(want_mt[r, 624]))
            wrote = np.zeros(STRIDE, dtype=bool)
            if with_lp and not cols[r]["finished"]:
                wrote[len(cols[r]["gen"])] = True
                at = len(cols[r]["gen"])
                assert bits(lp[r, at]) == bits(lp_ref[r][0]), (r, float(lp[r, at]), float(lp_ref[r][0]))
                assert np.array_equal(tid[r, at], lp_ref[r][1]) and np.array_equal(bits(tlp[r, at]), bits(lp_ref[r][2])), (r, tid[r, at].tolist(), lp_ref[r][1].tolist())
            assert (bits(lp[r, ~wrote]) == -1).all() and (tid[r, ~wrote] == -1).all() and (bits(tlp[r, ~wrote]) == -1).all(), (with_lp, r)      # 0xff bytes
        assert np.array_equal(fin, want_fin), (with_lp, fin.tolist(), want_fin.tolist())
        assert np.array_equal(hdr, want_hdr), (with_lp, hdr.tolist(), want_hdr.tolist())
        out[with_lp] = ids
    assert np.array_equal(out[True], out[False])


# ---- 2. equals the request alone ----

SEVEN_LENS = (5, 9, 14, 20, 25, 29, 33)
SEVEN_LIMITS = [1, 20, 7, 13, 12, 16, 10]
SEVEN_SEEDS = [301, 302, 303, 304, 305, 306, 307]
SEVEN_PROMPTS = [prompt_of(n, 100 + n) for n in SEVEN_LENS]


def seven_of(g):
    """The seven requests' parameters -- the EOS id, the suppressed ids and the stop sequence are taken from the free runs of their requests, so that each rule
    bites -- and each request alone."""
    free4 = free_run(g, SEVEN_PROMPTS[4], SEVEN_LIMITS[4], SEVEN_SEEDS[4], HOT)
    free5 = free_run(g, SEVEN_PROMPTS[5], SEVEN_LIMITS[5], SEVEN_SEEDS[5], GREEDY)
    free6 = free_run(g, SEVEN_PROMPTS[6], SEVEN_LIMITS[6], SEVEN_SEEDS[6], HOT)
    pars = [GREEDY, HOT, dict(HOT, repetition_penalty=1.3), dict(GREEDY, no_repeat_ngram_size=2), dict(HOT, min_new_tokens=4, eos_id=free4[1]),
            dict(GREEDY, suppress_tokens=sorted(set(free5[:3]))), dict(HOT, stop=[[free6[3], free6[4]]])]
    want = [alone(g, SEVEN_PROMPTS[r], SEVEN_LIMITS[r], SEVEN_SEEDS[r], pars[r]) for r in range(7)]
    assert want[4][0][1] != free4[1] and want[5][0][0] != free5[0], "fixture problem: a rule does not bite"
    assert want[6][1] == 2 and len(want[6][0]) <= 5, "fixture problem: the stop sequence does not fire: %s" % (want[6],)
    assert not rules_ref.ngram_repeats(SEVEN_PROMPTS[3] + want[3][0], 2)
    return pars, want


@pytest.fixture(scope="module")
def seven(pkg, files):
    out = {}
    for name in ("q4_0", "q5_1"):
        g = pkg.BiogptModel.load(files[name])
        out[name] = seven_of(g)
        g.close()
    return out


@pytest.mark.parametrize("name, max_columns, group", [("q4_0", 3, 1), ("q4_0", 3, 4), ("q4_0", 7, 4), ("q5_1", 3, 4)])
def test_equals_the_request_alone(pkg, files, seven, name, max_columns, group):
    pars, want = seven[name]
    g = pkg.BiogptModel.load(files[name])
    got, info = queue(pkg, g, SEVEN_PROMPTS, SEVEN_LIMITS, SEVEN_SEEDS, pars, max_columns, group)
    g.close()
    for r in range(7):
        assert got[r] == want[r][0], (r, got[r], want[r][0])
    assert info["finish"] == [w[1] for w in want]
    check_plan(pkg, info, [len(s) for s in got], SEVEN_LIMITS, sum(SEVEN_LENS), max_columns, group)


# ---- 3. the same parameters for all: the plain queue ----

def test_same_parameters_are_the_plain_queue(pkg, q40):
    g = q40
    prompts = [prompt_of(6 + 2 * r, 400 + r) for r in range(12)]
    seeds = [500 + r for r in range(12)]
    limits = [14, 9, 12, 20, 7, 16, 11, 18, 8, 15, 10, 13]
    free = free_run(g, prompts[0], limits[0], seeds[0], HOT)
    eos = free[3]
    plain_kw = dict(max_columns=3, group=4, seeds=seeds, n_predicts=limits)
    ids, info, _ = g.generate_queue(prompts, 20, eos_id=eos, **HOT, **plain_kw)
    got, got_info, _ = g.generate_queue(prompts, 20, params=pkg.request_params(eos_id=eos, **HOT), **plain_kw)
    assert [s.tolist() for s in got] == [s.tolist() for s in ids]
    finish = got_info.pop("finish")
    assert got_info == info
    assert finish == [1 if len(s) and int(s[-1]) == eos else 0 for s in ids] and 1 in finish and 0 in finish
    # behind a prefix
    prefix = prompt_of(17, 41)
    suffixes = [p[1:] for p in prompts]
    ids, info, _ = g.generate_queue(suffixes, 20, prefix=prefix, eos_id=eos, **HOT, **plain_kw)
    stats = g.prefix_stats()
    got, got_info, _ = g.generate_queue(suffixes, 20, prefix=prefix, params=[pkg.request_params(eos_id=eos, **HOT) for _ in range(12)], **plain_kw)
    assert [s.tolist() for s in got] == [s.tolist() for s in ids]
    got_info.pop("finish")
    assert got_info == info and g.prefix_stats() == stats and stats["n_shared"] == 16


# ---- 4. a refilled column inherits nothing ----

def test_refill_hygiene(pkg, q40):
    """One column.  A request with every rule on and a long history, then one with none, and the reverse order: each is its alone run."""
    g = q40
    long_prompt, short_prompt = prompt_of(33, 610), prompt_of(7, 611)
    free = free_run(g, long_prompt, 20, 71, HOT)
    ruled = dict(HOT, repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=6, eos_id=free[2], suppress_tokens=sorted(set(free[:2]) - {free[2]}),
                 stop=[[long_prompt[-1], free[0]]])
    reqs = [(long_prompt, 20, 71, ruled), (short_prompt, 20, 72, HOT)]
    want = [alone(g, *rq) for rq in reqs]
    assert want[0][0] != free[:len(want[0][0])]
    for order in ((0, 1), (1, 0)):
        got, info = queue(pkg, g, [reqs[i][0] for i in order], [reqs[i][1] for i in order], [reqs[i][2] for i in order], [reqs[i][3] for i in order], 1, 4)
        assert got == [want[i][0] for i in order], (order, got, want)
        assert info["finish"] == [want[i][1] for i in order] and info["column"] == [0, 0]


# ---- 5. behind a prefix ----

def test_rules_behind_a_prefix(pkg, q40):
    """prefix ++ suffix requests with rules and stop sequences against the closed rules call on the concatenations: the rules read the prefix's tokens too."""
    g = q40
    prefix = prompt_of(17, 41)
    suffixes = [prompt_of(n + 1, 700 + n)[1:] for n in (0, 5, 11, 18, 26)]
    suffixes[1] = [prefix[3], prefix[4]] + suffixes[1]      # (a bigram of the prefix stands again at the suffix's start)
    limits, seeds = [12, 20, 9, 15, 6], [81, 82, 83, 84, 85]
    pars = [dict(GREEDY, no_repeat_ngram_size=2), dict(HOT, repetition_penalty=1.3, no_repeat_ngram_size=3), HOT, dict(GREEDY, suppress_tokens=[5, 6, 7]),
            dict(HOT, repetition_penalty=1.2)]
    free2 = free_run(g, prefix + suffixes[2], limits[2], seeds[2], HOT)
    pars[2] = dict(HOT, stop=[[free2[4]]])
    want = [alone(g, prefix + suffixes[r], limits[r], seeds[r], pars[r]) for r in range(5)]
    assert want[2][1] == 2
    got, info = queue(pkg, g, suffixes, limits, seeds, pars, 3, 4, prefix=prefix)
    for r in range(5):
        assert got[r] == want[r][0], (r, got[r], want[r][0])
    assert info["finish"] == [w[1] for w in want]
    cols = 16 + sum(1 + len(s) for s in suffixes)
    check_plan(pkg, info, [len(s) for s in got], limits, cols, 3, 4)
    assert g.prefix_stats() == dict(n_shared=16, prompt_columns=cols, path=0, columns=3)


# ---- 6. log-probabilities ----

def test_logprobs_with_samplers_and_stop_sequences(pkg, q40):
    g = q40
    prompts = [prompt_of(n, 800 + n) for n in (6, 13, 21, 30)]
    limits, seeds = [10, 14, 8, 12], [91, 92, 93, 94]
    pars = [GREEDY, HOT, dict(top_k=10, top_p=0.8, temp=2.0), dict(HOT)]
    refs = [free_run(g, prompts[r], limits[r], seeds[r], pars[r], logprobs=2) for r in range(4)]
    pars[1] = dict(HOT, stop=[[refs[1][0][5]]])
    pars[3] = dict(HOT, stop=[[7, 8], [refs[3][0][2], refs[3][0][3]]])
    want = [qref.stop_cut(refs[r][0], pars[r].get("stop", ()), -1) for r in range(4)]
    assert [w[1] for w in want] == [0, 2, 0, 3] and len(want[1][0]) <= 6 and len(want[3][0]) <= 4
    for prefix in (None, prompts[0][:9]):
        ps = prompts if prefix is None else [p[1:] for p in prompts]
        if prefix is not None:      # the references behind the prefix, as the closed call gives them
            refs = [free_run(g, prefix + ps[r], limits[r], seeds[r], dict(sampler_of(pars[r])), logprobs=2) for r in range(4)]
            pars[1], pars[3] = dict(HOT, stop=[[refs[1][0][5]]]), dict(HOT, stop=[[7, 8], [refs[3][0][2], refs[3][0][3]]])
            want = [qref.stop_cut(refs[r][0], pars[r].get("stop", ()), -1) for r in range(4)]
        kw = {} if prefix is None else dict(prefix=prefix)
        got, info = queue(pkg, g, ps, limits, seeds, pars, 2, 4, logprobs=2, **kw)
        for r in range(4):
            n = len(want[r][0])
            assert got[r] == want[r][0], (r, got[r], want[r][0])
            lp, tid, tlp = info["logprobs"][r]
            assert lp.shape == (n,) and tid.shape == (n, 2) and tlp.shape == (n, 2)
            assert np.array_equal(bits(lp), bits(refs[r][1][0][:n])) and np.array_equal(tid, refs[r][1][1][:n]) and np.array_equal(bits(tlp), bits(refs[r][1][2][:n])), r
        assert info["finish"] == [w[1] for w in want]


def raw_call(pkg, g, prefix, prompts, n_predicts, seeds, pars, max_columns, group, n_top, fill=7):
    """The C entry point itself, on arrays preset to `fill`: (rc, ids, lens, finish, lp, top_ids, top_lp) with the arrays whole."""
    R, w = len(prompts), max(n_predicts)
    flat = np.ascontiguousarray([t for s in prompts for t in s] or [0], dtype=np.int32)
    lens = np.asarray([len(s) for s in prompts], dtype=np.int32)
    pre = None if prefix is None else np.ascontiguousarray(prefix, dtype=np.int32)
    npr, sd = np.asarray(n_predicts, dtype=np.int32), np.asarray(seeds, dtype=np.uint32)
    arr, keep = pkg._params_array([pkg.request_params(**p) for p in pars], R)
    out, ol, fin = np.full((R, w), fill, np.int32), np.full(R, fill, np.int32), np.full(R, fill, np.int32)
    k = max(n_top, 1)
    lp, tid, tlp = np.full((R, w), fill, np.float32), np.full((R, w, k), fill, np.int32), np.full((R, w, k), fill, np.float32)
    req = pkg.GenLogprobs(n_top, lp.ctypes.data, tid.ctypes.data, tlp.ctypes.data)
    secs, st = ctypes.c_double(0.0), pkg.QueueStats()
    rc = pkg.lib().biogpt_hip_generate_queue_requests(g._h, None if pre is None else pre.ctypes.data, 0 if pre is None else len(pre), flat.ctypes.data, lens.ctypes.data, R,
                                                      npr.ctypes.data, w, max_columns, group, 8, arr, sd.ctypes.data, out.ctypes.data, ol.ctypes.data, fin.ctypes.data, None,
                                                      None, ctypes.byref(secs), ctypes.byref(st), ctypes.byref(req))
    return rc, out, ol, fin, lp, tid, tlp


@pytest.mark.parametrize("behind", [False, True])
def test_logprob_tails_behind_a_stop_read_zero(pkg, q40, behind):
    """The caller's arrays as the call leaves them, whatever they held: entries at or past a request's length -- also the length a stop sequence cut on the
    device, before the request's limit -- and every entry of a request that never takes a column read 0 / -1 / 0, ids -1, and that request's finish -1."""
    g = q40
    prefix = prompt_of(17, 41) if behind else None
    prompts = [prompt_of(n, 900 + n)[1 if behind else 0:] for n in (6, 13, 21, 30, 9)]
    whole = [(prefix or []) + p for p in prompts]
    limits, seeds = [10, 14, 0, 12, 8], [95, 96, 97, 98, 99]      # request 2 never takes a column
    pars = [dict(GREEDY), dict(HOT), dict(HOT), dict(HOT), dict(top_k=10, top_p=0.8, temp=2.0)]
    refs = [free_run(g, whole[r], limits[r], seeds[r], pars[r], logprobs=3) if limits[r] else ([], None) for r in range(5)]
    pars[1] = dict(HOT, stop=[[refs[1][0][2]]])                          # fires within three tokens of 14
    pars[3] = dict(HOT, stop=[[5, 6, 7], [refs[3][0][3], refs[3][0][4]]])
    want = [qref.stop_cut(refs[r][0], pars[r].get("stop", ()), -1) for r in range(5)]
    assert len(want[1][0]) <= 3 and want[1][1] == 2 and len(want[3][0]) <= 5 and want[3][1] == 3
    rc, out, ol, fin, lp, tid, tlp = raw_call(pkg, g, prefix, prompts, limits, seeds, pars, 2, 4, 3)
    assert rc == 0, pkg._err()
    assert [int(v) for v in ol] == [len(w[0]) for w in want] and [int(v) for v in fin] == [0, 2, -1, 3, 0]
    for r in range(5):
        n = len(want[r][0])
        assert [int(t) for t in out[r, :n]] == want[r][0] and (out[r, n:] == -1).all(), (r, out[r].tolist())
        if n:
            ref = refs[r][1]
            assert np.array_equal(bits(lp[r, :n]), bits(ref[0][:n])) and np.array_equal(tid[r, :n], ref[1][:n]) and np.array_equal(bits(tlp[r, :n]), bits(ref[2][:n])), r
        assert (bits(lp[r, n:]) == 0).all() and (tid[r, n:] == -1).all() and (bits(tlp[r, n:]) == 0).all(), (r, lp[r].tolist(), tid[r].tolist())


# ---- 7. refusals that need a model ----

def test_model_dependent_refusals(pkg, files, q40):
    one = pkg.request_params(**HOT)
    for name in ("f32", "wide"):
        g = pkg.BiogptModel.load(files[name])
        with pytest.raises(pkg.BiogptError, match="generation over a queue with request parameters.*fast chain"):
            g.generate_queue([[2, 5, 7]], 4, params=one)
        g.close()
    g = q40
    V = KW["n_vocab"]
    with pytest.raises(pkg.BiogptError, match=r"params\[1\]\.stop: token id %d \(sequence 0, position 1\) out of range" % V):
        g.generate_queue([[2, 5], [2, 6]], 4, params=[one, pkg.request_params(stop=[[5, V]])])
    with pytest.raises(pkg.BiogptError, match=r"params\[0\]\.eos_id %d out of range" % V):
        g.generate_queue([[2, 5]], 4, params=pkg.request_params(eos_id=V))
    with pytest.raises(pkg.BiogptError, match=r"params\[0\]\.rules: .*suppress\[0\] = %d out of range" % V):
        g.generate_queue([[2, 5]], 4, params=pkg.request_params(suppress_tokens=[V]))
    with pytest.raises(pkg.BiogptError, match="logprobs with generation rules"):
        g.generate_queue([[2, 5]], 4, params=pkg.request_params(no_repeat_ngram_size=2), logprobs=1)
    prompt = prompt_of(9, 77)
    want = alone(g, prompt, 6, 21, HOT)      # still usable
    got, info = queue(pkg, g, [prompt], [6], [21], [HOT], 2, 4)
    assert got == [want[0]] and info["finish"] == [0]


# ---- 8. the forms of the two column queues share one context ----

def test_queue_forms_share_a_context(pkg, files):
    """Plain, prefix=, logprobs= and both, of generate_queue(params=...) and of the closed generate_queue, alternating on one context with one max_columns: each
    form has captured steps of its own, and every call returns what a fresh context returns."""
    def conv(v):
        if isinstance(v, np.ndarray):
            return (v.view(np.int32) if v.dtype == np.float32 else v).tolist()
        if isinstance(v, (list, tuple)):
            return [conv(x) for x in v]
        if isinstance(v, dict):
            return {k: conv(x) for k, x in v.items()}
        return v

    prefix = prompt_of(17, 41)
    prompts = [prompt_of(6 + 3 * r, 1000 + r) for r in range(6)]
    suffixes = [p[1:] for p in prompts]
    kw = dict(max_columns=3, group=4, seeds=[1100 + r for r in range(6)], n_predicts=[12, 7, 10, 12, 5, 9])
    ruled = [pkg.request_params(**p) for p in (GREEDY, HOT, dict(HOT, repetition_penalty=1.3), dict(GREEDY, no_repeat_ngram_size=2), HOT, dict(HOT, stop=[[5, 6]]))]
    bare = [pkg.request_params(**p) for p in (GREEDY, HOT, dict(top_k=10, top_p=0.8, temp=2.0), HOT, GREEDY, HOT)]      # (no log-probabilities under rules)
    calls = []
    for label, ps, more in (("plain", prompts, {}), ("prefix", suffixes, dict(prefix=prefix)), ("lp", prompts, dict(logprobs=2)),
                            ("lp prefix", suffixes, dict(prefix=prefix, logprobs=2))):
        calls.append(("requests " + label, lambda g, ps=ps, more=more: g.generate_queue(ps, 12, params=bare if "logprobs" in more else ruled, **more, **kw)))
        calls.append(("closed " + label, lambda g, ps=ps, more=more: g.generate_queue(ps, 12, **HOT, **more, **kw)))
    fresh = {}
    for label, call in calls:
        g = pkg.BiogptModel.load(files["q4_0"])
        fresh[label] = conv(call(g)[:2])
        g.close()
    g = pkg.BiogptModel.load(files["q4_0"])
    for at, (label, call) in enumerate(calls + calls[::-1]):
        assert conv(call(g)[:2]) == fresh[label], (at, label, "differs from a fresh context")
    g.close()
