"""Generation rules (kernels_rules.hip.h; biogpt_hip_generate_beam_rules / biogpt_hip_generate_sample_rules) on the GPU: the kernel alone equals
rules_ref.apply_rules (bit for bit on logits; to the score tolerance on log-probabilities); greedy and sampled generation with rules equal the
reference loop over the oracle with the rules in front of the sampler; beam search with rules equals beam_ref over the oracle's processed
log-probabilities; every rule changes an output and its invariant holds on the ids; neutral rules are today's path bit for bit; the captured,
eager and column-per-XCD paths agree; the context is left alone; argument errors name their field."""
import ctypes

import numpy as np
import pytest

import beam_ref
import rules_ref
from test_rules_capi import BAD_RULES

pytestmark = pytest.mark.gpu

KW = dict(n_vocab=42384, n_layer=3, n_head=16, n_positions=1024, d_ff=4096, d_model=1024, n_merges=40000)
V = KW["n_vocab"]
MARGIN = 1e-5             # beam selection (test_gpu_beam.py)
SAMPLE_MARGIN = 1e-9      # sampler decisions (test_gpu_sample.py)
NAMES = ["q4_0", "q5_1", "q8_0"]


def prompt_of(n, seed):
    rng = np.random.default_rng(seed)
    return [2] + [int(v) for v in rng.integers(4, V, n - 1)]


def looped(n, seed):
    """A prompt whose last two tokens occurred before (an n-gram ban of the first step comes from the prompt)."""
    p = prompt_of(n, seed)
    return p + p[1:3]


@pytest.fixture(scope="module")
def files(pkg, tmp_path_factory):
    d = tmp_path_factory.mktemp("rules")
    f32 = str(d / "f32.bin")
    pkg.write_synthetic(f32, **KW)
    out = {"f32": f32}
    for name in NAMES:
        out[name] = str(d / (name + ".bin"))
        pkg.quantize_file(f32, out[name], name)
    return out


# ---- 1 / 2. the kernel alone ----

def histories(n_vocab, n, rng):
    """(histories, prompt lengths): lengths 1, n - 1, n, 1023 and a few more, tokens from a small pool (duplicates), some of the tokens generated."""
    pool = rng.integers(0, n_vocab, 40)
    hs, pls = [], []
    for length in (1, max(1, n - 1), max(1, n), 1023, 7, 64, 300):
        h = [int(t) for t in rng.choice(pool, length)]
        hs.append(h)
        pls.append(int(rng.integers(0, length + 1)))
    pls[0], pls[3] = 1, 1000      # nothing generated / 23 tokens generated
    hs.append([int(t) for t in pool[:10]] * 3)      # periodic: the tail of every n <= 11 occurred before
    pls.append(12)
    return hs, pls


KERNEL_SETS = [dict(repetition_penalty=1.3), dict(repetition_penalty=0.7), dict(no_repeat_ngram_size=1), dict(no_repeat_ngram_size=2),
               dict(no_repeat_ngram_size=4), dict(min_new_tokens=5), dict(suppress_tokens=[0, 3, 95, 17]),
               dict(repetition_penalty=1.2, no_repeat_ngram_size=3, min_new_tokens=30, suppress_tokens=[1, 2, 3, 94])]


@pytest.mark.parametrize("n_vocab", [42384, 96, 1001])
@pytest.mark.parametrize("si", range(len(KERNEL_SETS)))
def test_kernel_on_logits_is_exact(pkg, n_vocab, si):
    rules = KERNEL_SETS[si]
    rng = np.random.default_rng(1000 * si + n_vocab)
    hs, pls = histories(n_vocab, rules.get("no_repeat_ngram_size", 3), rng)
    rows = (rng.standard_normal((len(hs), n_vocab)) * 3.0).astype(np.float32)
    eos = 5
    got = pkg.rules_rows(rows, hs, pls, mode=0, eos_id=eos, **rules)
    want = np.stack([rules_ref.apply_rules(rows[r], hs[r], pls[r], rules, eos) for r in range(len(hs))])
    assert (want != rows).any(), "fixture problem: the rule set changes nothing"
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:8]
    again = pkg.rules_rows(rows, hs, pls, mode=0, eos_id=-1, **rules)      # without an EOS id min_new_tokens does nothing
    want = np.stack([rules_ref.apply_rules(rows[r], hs[r], pls[r], rules, -1) for r in range(len(hs))])
    assert np.array_equal(again.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("n_vocab", [42384, 96, 1001])
@pytest.mark.parametrize("si", range(len(KERNEL_SETS)))
def test_kernel_on_logprobs(pkg, n_vocab, si):
    rules = KERNEL_SETS[si]
    p = float(rules.get("repetition_penalty", 1.0))
    rng = np.random.default_rng(2000 * si + n_vocab)
    hs, pls = histories(n_vocab, rules.get("no_repeat_ngram_size", 3), rng)
    rows = (rng.standard_normal((len(hs), n_vocab)) * 3.0).astype(np.float32)
    eos = 5
    got = pkg.rules_rows(rows, hs, pls, mode=1, eos_id=eos, **rules)
    lp = beam_ref.log_softmax_rows(rows)
    worst = 0.0
    for r in range(len(hs)):
        want = rules_ref.apply_rules(lp[r], hs[r], pls[r], rules, eos)
        banned = np.isneginf(want)
        assert np.array_equal(np.isneginf(got[r]), banned), r
        tol = np.full(n_vocab, 1e-4)
        if p != 1.0:
            tol[sorted(set(hs[r]))] = 1e-4 * p
        d = np.abs(got[r][~banned].astype(np.float64) - want[~banned].astype(np.float64))
        worst = max(worst, float(d.max()))
        assert (d <= tol[~banned]).all(), (r, float(d.max()))
    print("mode 1, n_vocab %d, %s: worst |difference| %.3g" % (n_vocab, rules, worst))


# ---- 3 / 4. greedy and sampled generation with rules against the oracle loop ----

SEQ_PROMPTS = [looped(6, 31), prompt_of(13, 32), looped(9, 33), prompt_of(5, 34), looped(17, 35), prompt_of(8, 36)]
N_PREDICT = 12
EOS = 7      # (a token of no prompt; min_new_tokens needs an EOS id to act)
# The synthetic model never repeats a token by itself.  A penalty below 1 favours the tokens seen (positive logits doubled, negative ones halved): the
# run then loops as a small model does, and the n-gram rule has loops to break (test_rules_do_something checks that both happen).
GEN_RULES = dict(repetition_penalty=0.5, no_repeat_ngram_size=3, min_new_tokens=6, suppress_tokens=[11, 12, 13])
_loop_cache = {}


def oracle_loop(oracle, files, name, nb, prompt_i, top_k, top_p, temp, seed, rules=GEN_RULES, eos=EOS):
    key = (name, nb, prompt_i, top_k, top_p, temp, seed, repr(sorted(rules.items())), eos)
    if key not in _loop_cache:
        o = oracle.OracleModel(files[name], n_threads=16)
        _loop_cache[key] = rules_ref.reference_loop_rules(o, SEQ_PROMPTS[prompt_i], nb, N_PREDICT, top_k, top_p, temp, seed, rules, eos)
    return _loop_cache[key]


@pytest.mark.parametrize("n_seqs", [2, 12])
@pytest.mark.parametrize("nb", [1, 8])
@pytest.mark.parametrize("name", NAMES)
def test_greedy_with_rules_against_oracle(pkg, oracle, files, name, nb, n_seqs):
    """top_k = 1 never draws: greedy decoding with rules.  2 sequences: two prompts; 12: six prompts x 2 samples (the samples share a prompt copy)."""
    n_prompts, n_samples = (2, 1) if n_seqs == 2 else (6, 2)
    want = [oracle_loop(oracle, files, name, nb, p, 1, 0.9, 0.9, 0)[0] for p in range(n_prompts) for _ in range(n_samples)]
    g = pkg.BiogptModel.load(files[name])
    got, _ = g.generate_sample(SEQ_PROMPTS[:n_prompts], N_PREDICT, n_samples=n_samples, top_k=1, seed=5, eos_id=EOS, n_batch=nb, **GEN_RULES)
    g.close()
    assert len(got) == n_seqs
    for r in range(n_seqs):
        assert list(got[r]) == want[r], (r, list(got[r]), want[r])


SAMPLE_SEEDS = [101, 202, 303, 404]     # sequence r = prompt r // 2, sample r % 2


@pytest.mark.parametrize("nb", [1, 8])
@pytest.mark.parametrize("name", NAMES)
def test_sampling_with_rules_against_oracle(pkg, oracle, files, name, nb):
    top_k, top_p, temp = 40, 0.9, 0.9
    want = []
    for r, seed in enumerate(SAMPLE_SEEDS):
        ids, margin = oracle_loop(oracle, files, name, nb, r // 2, top_k, top_p, temp, seed)
        print("%s n_batch=%d sequence %d: smallest margin %.3g, %d distinct ids" % (name, nb, r, margin, len(set(ids))))
        assert margin >= SAMPLE_MARGIN, "fixture problem: a decision of sequence %d lies %.3g from a border" % (r, margin)
        want.append(ids)
    g = pkg.BiogptModel.load(files[name])
    got, _ = g.generate_sample(SEQ_PROMPTS[:2], N_PREDICT, n_samples=2, top_k=top_k, top_p=top_p, temp=temp, seeds=SAMPLE_SEEDS, eos_id=EOS, n_batch=nb,
                               **GEN_RULES)
    g.close()
    for r in range(4):
        assert list(got[r]) == want[r], (r, list(got[r]), want[r])


# ---- 5. beam search with rules against the restatement ----

BEAM_PROMPT = looped(11, 3)
BEAM_PREDICT = 10
BEAM_RULES = dict(repetition_penalty=0.7, no_repeat_ngram_size=3, min_new_tokens=5, suppress_tokens=[11, 12, 13])      # (0.7: see GEN_RULES)


@pytest.fixture(scope="module")
def beam_rows(oracle, files):
    """One OracleLogprobs per file (rows cached per prefix) and its EOS id: the third token of the best EOS-free hypothesis of a run without
    rules (so that, without rules, EOS fires after 3 tokens)."""
    cache, eos = {}, {}

    def get(name):
        if name not in cache:
            cache[name] = beam_ref.OracleLogprobs(oracle.OracleModel(files[name], n_threads=16), BEAM_PROMPT, 8)
        return cache[name]

    def eos_of(name):
        if name not in eos:
            hyps, _ = beam_ref.beam_search(get(name), 4, BEAM_PREDICT, -1, 1.0, True)
            eos[name] = int(hyps[0][0][2])
        return eos[name]
    return get, eos_of


def check_beam(pkg, files, beam_rows, name, B, es, rules):
    get, eos_of = beam_rows
    eos = eos_of(name)
    want, margins = beam_ref.beam_search(rules_ref.rules_logprobs(get(name), BEAM_PROMPT, rules, eos), B, BEAM_PREDICT, eos, 1.0, es)
    small = [(k + 1, m) for k, m in enumerate(margins) if m < MARGIN]
    assert not small, "fixture problem: selection margins below %g at steps %s -- the case cannot tell the engine's rounding from a wrong choice" % (MARGIN, small)
    g = pkg.BiogptModel.load(files[name])
    got, _ = g.generate_beam(BEAM_PROMPT, BEAM_PREDICT, n_beams=B, eos_id=eos, length_penalty=1.0, early_stopping=es, n_batch=8, **rules)
    g.close()
    assert len(got) == len(want) == B
    for r, ((ids_w, s_w), (ids_g, s_g)) in enumerate(zip(want, got)):
        assert list(ids_g) == list(ids_w), (r, list(ids_g), list(ids_w))
        assert abs(float(s_g) - float(s_w)) <= 1e-4, (r, float(s_g), float(s_w))
    print("%s B=%d early_stopping=%s eos=%d %s: %d steps, lengths %s" % (name, B, es, eos, rules, len(margins), [len(h[0]) for h in got]))
    return want


@pytest.mark.parametrize("es", [True, False])
@pytest.mark.parametrize("B", [2, 5, 8])
@pytest.mark.parametrize("name", NAMES)
def test_beam_with_rules_against_restatement(pkg, files, beam_rows, name, B, es):
    check_beam(pkg, files, beam_rows, name, B, es, BEAM_RULES)


@pytest.mark.parametrize("name", NAMES)
def test_beam_model_card_shape(pkg, files, beam_rows, name):
    """generate(min_length, num_beams=5, early_stopping=True): min_new_tokens beyond the length at which the run without rules finishes its first hypothesis."""
    get, eos_of = beam_rows
    eos = eos_of(name)
    free, _ = beam_ref.beam_search(get(name), 5, BEAM_PREDICT, eos, 1.0, True)
    first = min(len(ids) for ids, _ in free if ids[-1] == eos)
    m = 7
    assert first < m, "fixture problem: the run without rules finishes no hypothesis before %d tokens" % m
    want = check_beam(pkg, files, beam_rows, name, 5, True, dict(min_new_tokens=m))
    assert all(eos not in ids[:m - 1] for ids, _ in want)


# ---- 6. every rule does something, and its invariant holds on the ids ----

def test_rules_do_something(pkg, files):
    g = pkg.BiogptModel.load(files["q4_0"])
    prompt = looped(9, 41)
    n_new = 48
    kw = dict(top_k=1, n_batch=8)
    free = list(g.generate_sample(prompt, n_new, eos_id=-1, **kw)[0][0])
    eos = free[3]
    cut = list(g.generate_sample(prompt, n_new, eos_id=eos, **kw)[0][0])
    assert cut == free[:free.index(eos) + 1] and len(cut) <= 4
    # min_new_tokens: no EOS among the first m - 1 tokens
    held = list(g.generate_sample(prompt, n_new, eos_id=eos, min_new_tokens=10, **kw)[0][0])
    assert held != cut and eos not in held[:9] and len(held) >= 10
    # suppress_tokens
    sup = sorted(set(free[:6]))
    out = list(g.generate_sample(prompt, n_new, eos_id=-1, suppress_tokens=sup, **kw)[0][0])
    assert out != free and not set(out) & set(sup)
    # repetition_penalty: below 1 the tokens seen are favoured, and the run repeats itself
    loop = list(g.generate_sample(prompt, n_new, eos_id=-1, repetition_penalty=0.5, **kw)[0][0])
    assert loop != free and len(set(free)) == len(free) and rules_ref.ngram_repeats(prompt + loop, 3)
    strict = list(g.generate_sample(prompt, n_new, eos_id=-1, repetition_penalty=1.5, **kw)[0][0])
    assert strict == free      # (above 1 nothing changes: the free run repeats no token)
    # no_repeat_ngram_size, on top of that penalty: no n-gram twice in prompt + output (the prompt holds a repeated bigram, no repeated trigram)
    assert rules_ref.ngram_repeats(prompt, 2) and not rules_ref.ngram_repeats(prompt, 3)
    for n in (1, 3):
        out = list(g.generate_sample(prompt, n_new, eos_id=-1, repetition_penalty=0.5, no_repeat_ngram_size=n, **kw)[0][0])
        assert out != loop, n
        if n == 1:
            assert len(set(out)) == len(out) and not set(out) & set(prompt)
        else:
            assert not rules_ref.ngram_repeats(prompt + out, n)
    # the same through beam search
    bfree, _ = g.generate_beam(prompt, 24, n_beams=4, eos_id=-1)
    bloop, _ = g.generate_beam(prompt, 24, n_beams=4, eos_id=-1, repetition_penalty=0.7)
    assert [list(i) for i, _ in bloop] != [list(i) for i, _ in bfree]
    assert any(rules_ref.ngram_repeats(prompt + [int(t) for t in i], 3) for i, _ in bloop)
    for rules in (dict(repetition_penalty=0.7, no_repeat_ngram_size=3), dict(suppress_tokens=[int(t) for t in bfree[0][0][:3]])):
        hyps, _ = g.generate_beam(prompt, 24, n_beams=4, eos_id=-1, **rules)
        if "no_repeat_ngram_size" in rules:
            assert [list(i) for i, _ in hyps] != [list(i) for i, _ in bloop]
            assert all(not rules_ref.ngram_repeats(prompt + [int(t) for t in i], 3) for i, _ in hyps)
        if "suppress_tokens" in rules:
            assert [list(i) for i, _ in hyps] != [list(i) for i, _ in bfree]
            assert all(not set(int(t) for t in i) & set(rules["suppress_tokens"]) for i, _ in hyps)
    beos = int(bfree[0][0][2])
    bcut, _ = g.generate_beam(prompt, 24, n_beams=4, eos_id=beos)
    bheld, _ = g.generate_beam(prompt, 24, n_beams=4, eos_id=beos, min_new_tokens=12)
    assert any(len(i) < 12 for i, _ in bcut) and all(len(i) >= 12 and beos not in list(i)[:11] for i, _ in bheld)
    g.close()


# ---- 7. neutral rules: today's path, bit for bit ----

def raw_beam(pkg, g, prompt, n_predict, B, eos, rules):
    L = pkg.lib()
    pr = np.ascontiguousarray(prompt, dtype=np.int32)
    ids, lens, sc = np.zeros((B, n_predict), np.int32), np.zeros(B, np.int32), np.zeros(B, np.float32)
    secs = ctypes.c_double(0.0)
    args = (g._h, pr.ctypes.data, pr.size, 8, B, n_predict, eos, 1.0, 1, ids.ctypes.data, lens.ctypes.data, sc.ctypes.data, ctypes.byref(secs))
    if rules == "old":
        rc = L.biogpt_hip_generate_beam(*args)
    else:
        rc = L.biogpt_hip_generate_beam_rules(*args, None if rules is None else ctypes.byref(rules))
    assert rc == B, pkg._err()
    return ids.tobytes(), lens.tobytes(), sc.tobytes()


def raw_sample(pkg, g, prompts, n_predict, n_samples, eos, rules):
    L = pkg.lib()
    lens = np.asarray([len(p) for p in prompts], dtype=np.int32)
    flat = np.ascontiguousarray(np.concatenate([np.asarray(p, dtype=np.int32) for p in prompts]))
    n = len(prompts) * n_samples
    sd = np.arange(1, n + 1, dtype=np.uint32)
    ids, ol = np.zeros((n, n_predict), np.int32), np.zeros(n, np.int32)
    secs = ctypes.c_double(0.0)
    args = (g._h, flat.ctypes.data, lens.ctypes.data, len(prompts), n_samples, 8, n_predict, 40, 0.9, 0.9, sd.ctypes.data, eos, ids.ctypes.data, ol.ctypes.data,
            ctypes.byref(secs))
    if rules == "old":
        rc = L.biogpt_hip_generate_sample(*args)
    else:
        rc = L.biogpt_hip_generate_sample_rules(*args, None if rules is None else ctypes.byref(rules))
    assert rc == n_predict, pkg._err()
    return ids.tobytes(), ol.tobytes()


def check_neutral(pkg, files, call):
    """call(g, rules) -> the raw result.  biogpt_hip_chunk_launches counts column-per-XCD launches as they are enqueued OR captured: a call that
    finds its graphs replays them and adds nothing, a call that has to capture a step adds one per graph.  So (a) on fresh contexts every variant
    advances the count as the existing entry point does, and (b) on one context, after the existing entry point has run, the variants advance it
    as a repeat of that call does (they find its graphs: no extra captured graph)."""
    neutral, keep = pkg.gen_rules()
    inert, keep2 = pkg.gen_rules(min_new_tokens=5)      # min_new_tokens without an EOS id: no rule is active
    variants = ("old", None, neutral, inert)
    base, first = None, []
    for rules in variants:
        g = pkg.BiogptModel.load(files["q4_0"])
        before = g.chunk_launches()
        out = call(g, rules)
        first.append(g.chunk_launches() - before)
        g.close()
        base = base or out
        assert out == base, rules
    assert len(set(first)) == 1, first
    g = pkg.BiogptModel.load(files["q4_0"])
    assert call(g, "old") == base
    later = []
    for rules in variants:
        before = g.chunk_launches()
        assert call(g, rules) == base, rules
        later.append(g.chunk_launches() - before)
    g.close()
    assert len(set(later)) == 1, later
    return first, later


def test_neutral_rules_change_nothing(pkg, files):
    prompt = prompt_of(21, 51)
    prompts = [prompt_of(9, 52), prompt_of(14, 53)]
    for B in (3, 12):
        print("beam B=%d: chunk launches %s" % (B, check_neutral(pkg, files, lambda g, rules: raw_beam(pkg, g, prompt, 20, B, -1, rules))))
    for n_samples in (2, 6):
        print("sample x%d: chunk launches %s" % (n_samples, check_neutral(pkg, files, lambda g, rules: raw_sample(pkg, g, prompts, 20, n_samples, -1, rules))))


# ---- 8. the paths agree; calls with and without rules alternate on one context ----

def test_paths_agree_with_rules(pkg, files, monkeypatch):
    prompt = looped(28, 6)
    prompts = [looped(10 + 3 * i, 60 + i) for i in range(6)]
    rules = dict(repetition_penalty=0.6, no_repeat_ngram_size=3, min_new_tokens=30, suppress_tokens=[11, 12, 13])
    g = pkg.BiogptModel.load(files["q4_0"])
    runs = {}
    for label, env in (("default", {}), ("repeat", {}), ("xcols off", {"BIOGPT_HIP_XCOLS": "0"}), ("no graph", {"BIOGPT_HIP_NO_GRAPH": "1"})):
        for k in ("BIOGPT_HIP_XCOLS", "BIOGPT_HIP_NO_GRAPH"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        g.refresh_options()
        for B in (2, 5, 12):
            hyps, _ = g.generate_beam(prompt, 40, n_beams=B, eos_id=EOS, length_penalty=1.0, early_stopping=False, n_batch=8, **rules)
            runs.setdefault(("beam", B), []).append((label, [(list(i), float(s)) for i, s in hyps]))
        for n_prompts, n_samples in ((2, 1), (5, 1), (6, 2)):
            ids, _ = g.generate_sample(prompts[:n_prompts], 40, n_samples=n_samples, top_k=40, top_p=0.9, temp=0.9, seed=7, eos_id=EOS, n_batch=8, **rules)
            runs.setdefault(("sample", n_prompts * n_samples), []).append((label, [list(i) for i in ids]))
    g.close()
    for key, rs in runs.items():
        for label, r in rs[1:]:
            assert r == rs[0][1], (key, label)


def test_calls_with_and_without_rules_alternate(pkg, files):
    prompt = looped(15, 71)
    prompts = [looped(8, 72), prompt_of(12, 73), looped(6, 74)]
    rules_a = dict(repetition_penalty=0.5, no_repeat_ngram_size=2)
    rules_b = dict(suppress_tokens=[11, 12], min_new_tokens=8)      # other values, the same captured steps
    fresh = {}
    for key, rules in (("free", {}), ("a", rules_a), ("b", rules_b)):
        g = pkg.BiogptModel.load(files["q4_0"])
        fresh[key] = ([(list(i), float(s)) for i, s in g.generate_beam(prompt, 24, n_beams=4, eos_id=EOS, **rules)[0]],
                      [list(i) for i in g.generate_sample(prompts, 24, n_samples=2, seed=3, eos_id=EOS, **rules)[0]])
        g.close()
    assert fresh["a"] != fresh["free"] and fresh["b"] != fresh["free"] and fresh["a"] != fresh["b"]
    g = pkg.BiogptModel.load(files["q4_0"])
    for key in ("a", "free", "b", "a", "free", "free", "b"):
        rules = {"free": {}, "a": rules_a, "b": rules_b}[key]
        got = ([(list(i), float(s)) for i, s in g.generate_beam(prompt, 24, n_beams=4, eos_id=EOS, **rules)[0]],
               [list(i) for i in g.generate_sample(prompts, 24, n_samples=2, seed=3, eos_id=EOS, **rules)[0]])
        assert got == fresh[key], key
    g.close()


# ---- 9. the context is left alone; arguments ----

def test_context_cache_untouched_and_eval_follows(pkg, files):
    g = pkg.BiogptModel.load(files["q4_0"])
    h = pkg.BiogptModel.load(files["q4_0"])
    ctx_toks = prompt_of(9, 7)
    g.eval(ctx_toks, 0)
    h.eval(ctx_toks, 0)
    D = KW["d_model"]
    k0, v0 = g.read_kv(0, 0, 3 * KW["n_positions"] * D), g.read_kv(1, 0, 3 * KW["n_positions"] * D)
    row0 = g.read_logits()
    hyps, _ = g.generate_beam(looped(17, 8), 12, n_beams=4, eos_id=EOS, n_batch=8, **GEN_RULES)
    ids, _ = g.generate_sample([looped(17, 8)], 12, n_samples=4, seed=3, eos_id=EOS, **GEN_RULES)
    assert len(hyps) == 4 and len(ids) == 4
    assert np.array_equal(g.read_kv(0, 0, k0.size), k0) and np.array_equal(g.read_kv(1, 0, v0.size), v0)
    assert np.array_equal(g.read_logits(), row0)
    nxt = [123]
    assert np.array_equal(g.eval(nxt, len(ctx_toks)), h.eval(nxt, len(ctx_toks)))
    g.close()
    h.close()


def test_float_files_and_bad_rules_fail(pkg, files, tiny_models, tmp_path):
    for path in (files["f32"], tiny_models["f16"]):
        g = pkg.BiogptModel.load(path)
        with pytest.raises(pkg.BiogptError, match="fast chain"):
            g.generate_beam([2, 5, 7], 4, n_beams=2, **GEN_RULES)
        with pytest.raises(pkg.BiogptError, match="fast chain"):
            g.generate_sample([2, 5, 7], 4, **GEN_RULES)
        g.close()
    g = pkg.BiogptModel.load(files["q4_0"])
    bad = [(kw, f) for kw, f in BAD_RULES if kw.get("suppress_tokens") != [3, 96]]
    bad += [(dict(suppress_tokens=[3, V]), "suppress"), (dict(no_repeat_ngram_size=KW["n_positions"] + 1), "no_repeat_ngram_size")]
    for kw, field in bad:
        with pytest.raises(pkg.BiogptError, match=field):
            g.generate_beam([2, 5, 7], 4, n_beams=2, **kw)
        with pytest.raises(pkg.BiogptError, match=field):
            g.generate_sample([2, 5, 7], 4, **kw)
    hyps, _ = g.generate_beam([2, 5, 7], 4, n_beams=3, eos_id=-1, **GEN_RULES)      # still usable
    assert len(hyps) == 3 and all(len(i) == 4 for i, _ in hyps)
    ids, _ = g.generate_sample([2, 5, 7], 4, n_samples=3, **GEN_RULES)
    assert len(ids) == 3 and all(len(i) == 4 for i in ids)
    g.close()
    # a rule set that could leave a beam row fewer than 2 x n_beams candidates: n_vocab - n_suppress - 1 - n_positions < 2 * n_beams
    f32, q = str(tmp_path / "small_f32.bin"), str(tmp_path / "small_q4_0.bin")
    pkg.write_synthetic(f32, **dict(KW, n_vocab=1045, n_layer=1, n_merges=16))      # 1045 - 1 - 1024 = 20
    pkg.quantize_file(f32, q, "q4_0")
    g = pkg.BiogptModel.load(q)
    with pytest.raises(pkg.BiogptError, match="n_beams"):
        g.generate_beam([2, 5, 7], 4, n_beams=11, eos_id=-1, no_repeat_ngram_size=2)
    with pytest.raises(pkg.BiogptError, match="n_beams"):
        g.generate_beam([2, 5, 7], 4, n_beams=8, eos_id=-1, suppress_tokens=[9, 10, 11, 12, 13])      # 15 < 16
    assert len(g.generate_beam([2, 5, 7], 4, n_beams=11, eos_id=-1, repetition_penalty=1.2)[0]) == 11      # (the penalty bans nothing)
    assert len(g.generate_beam([2, 5, 7], 4, n_beams=10, eos_id=-1, no_repeat_ngram_size=2)[0]) == 10
    assert len(g.generate_beam([2, 5, 7], 4, n_beams=11, eos_id=-1)[0]) == 11
    g.close()
