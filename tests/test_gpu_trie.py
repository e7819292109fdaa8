"""Trie-constrained generation (kernels_trie.hip.h; biogpt_hip_generate_beam_trie / biogpt_hip_generate_sample_trie) on the GPU: the kernel alone equals
trie_ref.mask bit for bit on logits, and on log-probabilities the allowed entries are those of rules_rows_kernel with neutral rules, bit for bit, inside the
float64 bound; the beam row kernel takes rows with fewer than 2 x n_beams finite values as beam_kernels_ref.row_candidates does; beam search, greedy and
sampled generation with a trie equal trie_ref + beam_ref / the reference loop over the oracle; finite hypotheses are entries; the captured and eager paths
agree; tries and calls alternate on one context; the context is left alone; argument errors name their field."""
import numpy as np
import pytest

import beam_kernels_ref as bkr
import beam_ref
import trie_ref

pytestmark = pytest.mark.gpu

KW = dict(n_vocab=42384, n_layer=3, n_head=16, n_positions=1024, d_ff=4096, d_model=1024, n_merges=40000)
V = KW["n_vocab"]
MARGIN = 1e-5             # beam selection (test_gpu_beam.py)
SAMPLE_MARGIN = 1e-9      # sampler decisions (test_gpu_sample.py)
NAMES = ["q4_0", "q8_0"]
EOS = 7                   # (a token of no prompt and no entry)
N_PREDICT = 8


# ---- the kernel alone ----

def kernel_cases(n_vocab):
    """[(name, entries, eos, histories)]: the shape tries of trie_ref, EOS = 0, = V - 1 and mid-word in turn ("dup_prefix" holds 0 and V - 1: mid-word)."""
    rng = np.random.default_rng([3, n_vocab])
    out = []
    for i, (name, entries) in enumerate(trie_ref.shape_tries(n_vocab).items()):
        which = "mid" if name == "dup_prefix" else ("first", "last", "mid")[i % 3]
        out.append((name, entries, trie_ref.unused_token(entries, n_vocab, which), trie_ref.probe_histories(entries, n_vocab, rng, n=4)))
    return out


@pytest.mark.parametrize("n_vocab", [42384, 42383, 1001, 96, 33])
def test_kernel_alone(pkg, n_vocab):
    cases = kernel_cases(n_vocab)
    assert {eos for _, _, eos, _ in cases} >= {0, n_vocab - 1}
    rng = np.random.default_rng(n_vocab)
    worst = 0.0
    for name, entries, eos, hs in cases:
        ref = trie_ref.RefTrie(entries)
        t = pkg.Trie.build(entries, n_vocab)
        rows = (rng.standard_normal((len(hs), n_vocab)) * 3.0).astype(np.float32)
        want = np.stack([ref.mask(rows[r], hs[r], eos) for r in range(len(hs))])
        kinds = {(ref.node(h) is None, bool(ref.node(h) and ref.node(h)["end"]), bool(ref.node(h) and ref.node(h)["next"])) for h in hs}
        assert {(True, False, False), (False, True, False), (False, False, True)} <= kinds, (name, kinds)      # off the trie, a leaf, inside
        # mode 0: the mask alone, bit for bit
        got = pkg.trie_rows(rows, t, hs, mode=0, eos_id=eos)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:8])
        # mode 1: the allowed entries are the log-probabilities rules_rows_kernel writes (neutral rules), within the bound of the float64 log-softmax
        got = pkg.trie_rows(rows, t, hs, mode=1, eos_id=eos)
        lp = pkg.rules_rows(rows, [[0]] * len(hs), mode=1, eos_id=-1)
        inside = ~np.isneginf(want)
        assert np.array_equal(np.isneginf(got), ~inside), name
        assert np.array_equal(got[inside].view(np.uint32), lp[inside].view(np.uint32)), name
        for r in range(len(hs)):
            ref64 = bkr.log_softmax64(rows[r])[0][inside[r]]
            d = np.abs(got[r][inside[r]].astype(np.float64) - ref64)
            assert (d <= bkr.lp_tolerance(n_vocab, ref64)).all(), (name, r, float(d.max()))
            worst = max(worst, float(d.max()))
        t.close()
    print("n_vocab %d: %d tries, mode 1 worst |lp - float64| %.3g" % (n_vocab, len(cases), worst))


@pytest.mark.parametrize("n_vocab", [42383, 70])
@pytest.mark.parametrize("B", [1, 4, 16])
def test_beam_rows_with_few_finite_values(pkg, B, n_vocab):
    """beam_group_rows_kernel<.., GIVEN> on rows of a trie step: group g's rows hold 0, 1, B and 2B - 1 finite log-probabilities (at the row's ends and
    anywhere); the candidates at -inf follow the finite ones, lower id first."""
    K = 2 * B
    rng = np.random.default_rng([B, n_vocab])
    counts = [0, 1, B, K - 1]
    rows = np.full((len(counts) * B, n_vocab), -np.inf, dtype=np.float32)
    for g, n in enumerate(counts):
        for j in range(B):
            at = rng.choice(n_vocab, n, replace=False)
            if n and j == 0:
                at[0] = n_vocab - 1
            if n > 1 and j == 0:
                at[1] = 0
            at = np.unique(at)
            rows[g * B + j, at] = -rng.integers(1, 200, at.size).astype(np.float32) / 8.0      # (ties among the finite values too)
    run = (-rng.integers(0, 80, rows.shape[0]) / 4.0).astype(np.float32)
    run[-1] = -np.inf      # a beam that took a candidate at -inf
    sc, col, ids = pkg.beam_rows(rows, B, run, given=True, masked=True)
    for r in range(rows.shape[0]):
        want_ids, want_sc = bkr.row_candidates(rows[r], K, run[r], True)
        assert np.array_equal(ids[r], want_ids), (r, ids[r], want_ids)
        assert np.array_equal(sc[r].view(np.uint32), want_sc.view(np.uint32)), (r, sc[r], want_sc)
        assert (col[r] == r % B).all()
    with pytest.raises(pkg.BiogptError, match="finite"):      # the entry of the rules keeps its precondition
        pkg.beam_rows(rows, B, run, given=True)


# ---- with a model ----

def prompt_of(n, seed):
    rng = np.random.default_rng(seed)
    return [2] + [int(v) for v in rng.integers(8, V, n - 1)]


PROMPTS = [prompt_of(5, 81), prompt_of(7, 82), prompt_of(9, 83)]
_rng = np.random.default_rng(77)
POOL = [int(t) for t in _rng.choice(np.arange(100, V), 50, replace=False)]
BIG = [[int(t) for t in _rng.choice(POOL, int(_rng.integers(1, 7)))] for _ in range(200)]      # ~200 entries of 1 - 6 tokens over a 50-token pool
SMALL = [POOL[:3], [POOL[0], POOL[3]], [POOL[4]]]                                              # 3 entries: junk beams occur at B = 5
TRIES = {"big": BIG, "small": SMALL}


@pytest.fixture(scope="module")
def files(pkg, tmp_path_factory):
    d = tmp_path_factory.mktemp("trie")
    f32 = str(d / "f32.bin")
    pkg.write_synthetic(f32, **KW)
    out = {"f32": f32}
    for name in NAMES:
        out[name] = str(d / (name + ".bin"))
        pkg.quantize_file(f32, out[name], name)
    return out


@pytest.fixture(scope="module")
def models(pkg, files):
    ms = {name: pkg.BiogptModel.load(files[name]) for name in NAMES}
    yield ms
    for m in ms.values():
        m.close()


@pytest.fixture(scope="module")
def tries(pkg):
    ts = {k: pkg.Trie.build(e, V) for k, e in TRIES.items()}
    yield ts
    for t in ts.values():
        t.close()


@pytest.fixture(scope="module")
def oracle_rows(oracle, files):
    """One beam_ref.OracleLogprobs per (file, prompt): rows cached per prefix, shared by every case."""
    cache = {}

    def get(name, p):
        if (name, p) not in cache:
            cache[(name, p)] = beam_ref.OracleLogprobs(oracle.OracleModel(files[name], n_threads=16), PROMPTS[p], 8)
        return cache[(name, p)]
    return get


_want = {}


def beam_reference(oracle_rows, name, p, which, B, es):
    key = (name, p, which, B, es)
    if key not in _want:
        _want[key] = trie_ref.beam_search_trie(oracle_rows(name, p), trie_ref.RefTrie(TRIES[which]), B, N_PREDICT, EOS, 1.0, es)
    return _want[key]


def check_hyps(got, want, entries, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for r, ((ids_w, s_w), (ids_g, s_g)) in enumerate(zip(want, got)):
        assert list(ids_g) == list(ids_w), (what, r, list(ids_g), list(ids_w))
        if np.isfinite(s_w):
            assert abs(float(s_g) - float(s_w)) <= 1e-4, (what, r, float(s_g), float(s_w))
            if ids_g[-1] == EOS:
                assert tuple(int(t) for t in ids_g[:-1]) in entries, (what, r, list(ids_g))
        else:
            assert s_g == -np.inf, (what, r, float(s_g))


@pytest.mark.parametrize("es", [True, False])
@pytest.mark.parametrize("B", [2, 5])
@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("which", ["big", "small"])
@pytest.mark.parametrize("name", NAMES)
def test_beam_with_trie_against_restatement(pkg, models, tries, oracle_rows, name, which, G, B, es):
    wants = []
    for p in range(G):
        want, margins = beam_reference(oracle_rows, name, p, which, B, es)
        small = [(k + 1, m) for k, m in enumerate(margins) if m < MARGIN]
        assert not small, "fixture problem: finite selection margins below %g at steps %s of prompt %d" % (MARGIN, small, p)
        wants.append(want)
    got, _ = models[name].generate_beam_batch(PROMPTS[:G], N_PREDICT, n_beams=B, eos_id=EOS, length_penalty=1.0, early_stopping=es, n_batch=8, trie=tries[which])
    entries = trie_ref.RefTrie(TRIES[which]).entries
    for p in range(G):
        check_hyps(got[p], wants[p], entries, (name, which, G, B, es, p))
    n_inf = sum(1 for p in range(G) for _, s in got[p] if not np.isfinite(s))
    print("%s %s G=%d B=%d es=%s: %s hypotheses, %d at -inf, lengths %s" % (name, which, G, B, es, [len(h) for h in got], n_inf, [[len(i) for i, _ in h] for h in got]))
    if which == "small" and B == 5:
        assert n_inf > 0, "fixture problem: no junk hypothesis with 3 entries and 5 beams"
    if G == 1:      # the one-prompt entry is the batch of one
        one, _ = models[name].generate_beam(PROMPTS[0], N_PREDICT, n_beams=B, eos_id=EOS, length_penalty=1.0, early_stopping=es, n_batch=8, trie=tries[which])
        assert [(list(i), s) for i, s in one] == [(list(i), s) for i, s in got[0]]


@pytest.mark.parametrize("which", ["big", "small"])
@pytest.mark.parametrize("name", NAMES)
def test_greedy_and_sampling_with_trie_against_oracle(pkg, oracle, files, models, tries, name, which):
    ref = trie_ref.RefTrie(TRIES[which])
    o = oracle.OracleModel(files[name], n_threads=16)
    want = [trie_ref.reference_loop_trie(o, p, 8, N_PREDICT, 1, 0.9, 0.9, 0, ref, EOS)[0] for p in PROMPTS]
    got, _ = models[name].generate_sample(PROMPTS, N_PREDICT, top_k=1, seed=5, eos_id=EOS, n_batch=8, trie=tries[which])
    for r in range(len(PROMPTS)):
        assert list(got[r]) == want[r], (r, list(got[r]), want[r])
        assert want[r][-1] == EOS and tuple(want[r][:-1]) in ref.entries      # (n_predict > max depth: every run finishes an entry)
    # top_k = 8, two samples per prompt: rows with fewer than 8 allowed tokens put candidates at -inf (weight 0) among the 8
    seeds = [101, 202, 303, 404, 505, 606]
    want = []
    for r, seed in enumerate(seeds):
        ids, margin = trie_ref.reference_loop_trie(o, PROMPTS[r // 2], 8, N_PREDICT, 8, 0.95, 1.3, seed, ref, EOS)
        assert margin >= SAMPLE_MARGIN, "fixture problem: a decision of sequence %d lies %.3g from a border" % (r, margin)
        want.append(ids)
    got, _ = models[name].generate_sample(PROMPTS, N_PREDICT, n_samples=2, top_k=8, top_p=0.95, temp=1.3, seeds=seeds, eos_id=EOS, n_batch=8, trie=tries[which])
    for r in range(len(seeds)):
        assert list(got[r]) == want[r], (r, list(got[r]), want[r])
    if which == "big":
        assert len({tuple(w) for w in want}) > 3, "fixture problem: the draws decide nothing"


def test_trie_of_the_greedy_continuations_reproduces_greedy(pkg, models):
    g = models["q4_0"]
    free, _ = g.generate_greedy_batch(PROMPTS, N_PREDICT)
    entries = [[int(t) for t in row] for row in free]
    assert all(EOS not in e for e in entries)
    t = pkg.Trie.build(entries + [e[:3] for e in entries], V)
    got, _ = g.generate_sample(PROMPTS, N_PREDICT, top_k=1, eos_id=EOS, trie=t)
    assert [list(i) for i in got] == entries
    hyps, _ = g.generate_beam_batch(PROMPTS, N_PREDICT, n_beams=1, eos_id=EOS, trie=t)
    assert [list(h[0][0]) for h in hyps] == entries      # one beam: greedy over log-probabilities
    t.close()


def test_a_prompts_result_does_not_depend_on_the_call(pkg, models, tries):
    g = models["q8_0"]
    kw = dict(n_beams=4, eos_id=EOS, early_stopping=False, trie=tries["big"])
    together, _ = g.generate_beam_batch(PROMPTS, N_PREDICT, **kw)
    for p in (1, 2):
        alone, _ = g.generate_beam_batch([PROMPTS[p]], N_PREDICT, **kw)
        assert [(list(i), s) for i, s in alone[0]] == [(list(i), s) for i, s in together[p]], p
    ids, _ = g.generate_sample(PROMPTS, N_PREDICT, top_k=8, seeds=[5, 6, 7], eos_id=EOS, trie=tries["big"])
    one, _ = g.generate_sample([PROMPTS[2]], N_PREDICT, top_k=8, seeds=[7], eos_id=EOS, trie=tries["big"])
    assert list(one[0]) == list(ids[2])


def run_both(g, trie, B=4):
    """(beam hypotheses of one prompt, sampled ids of three) with `trie` (None: unconstrained)."""
    kw = {} if trie is None else dict(trie=trie)
    hyps, _ = g.generate_beam(PROMPTS[1], N_PREDICT, n_beams=B, eos_id=EOS, **kw)
    ids, _ = g.generate_sample(PROMPTS, N_PREDICT, top_k=8, seed=3, eos_id=EOS, **kw)
    return [(list(i), float(s)) for i, s in hyps], [list(i) for i in ids]


def test_paths_agree_with_a_trie(pkg, files, tries, monkeypatch):
    g = pkg.BiogptModel.load(files["q4_0"])
    runs = []
    for label, env in (("default", {}), ("repeat", {}), ("xcols off", {"BIOGPT_HIP_XCOLS": "0"}), ("no graph", {"BIOGPT_HIP_NO_GRAPH": "1"})):
        for k in ("BIOGPT_HIP_XCOLS", "BIOGPT_HIP_NO_GRAPH"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        g.refresh_options()
        runs.append((label, [run_both(g, tries[w], B) for w in ("big", "small") for B in (2, 5)]))
    g.close()
    for label, r in runs[1:]:
        assert r == runs[0][1], label


def test_tries_and_free_calls_alternate_on_one_context(pkg, files, tries):
    """Each call equals its result on a fresh context; a second trie finds the captured steps of the first (biogpt_hip_chunk_launches counts column-per-XCD
    launches as they are enqueued or captured: a call that has to capture adds one per graph, so the other trie advances it as a repeat does)."""
    solo = {}
    for key in ("free", "big", "small"):
        g = pkg.BiogptModel.load(files["q4_0"])
        solo[key] = run_both(g, None if key == "free" else tries[key])
        g.close()
    assert solo["big"] != solo["free"] and solo["small"] != solo["free"] and solo["big"] != solo["small"]
    g = pkg.BiogptModel.load(files["q4_0"])
    steps = {}
    for key in ("big", "big", "small", "free", "small", "free", "big"):
        before = g.chunk_launches()
        assert run_both(g, None if key == "free" else tries[key]) == solo[key], key
        steps.setdefault(key, []).append(g.chunk_launches() - before)
    g.close()
    print("chunk launches per pair of calls: %s" % steps)
    assert steps["small"][0] == steps["big"][1] == steps["big"][2] == steps["small"][1], steps      # no capture after the first call with a trie


def test_context_cache_untouched_and_eval_follows(pkg, files, tries):
    g = pkg.BiogptModel.load(files["q4_0"])
    h = pkg.BiogptModel.load(files["q4_0"])
    ctx_toks = prompt_of(9, 7)
    g.eval(ctx_toks, 0)
    h.eval(ctx_toks, 0)
    D = KW["d_model"]
    k0, v0 = g.read_kv(0, 0, 3 * KW["n_positions"] * D), g.read_kv(1, 0, 3 * KW["n_positions"] * D)
    row0 = g.read_logits()
    hyps, ids = run_both(g, tries["big"])
    assert len(hyps) == 4 and len(ids) == 3
    assert np.array_equal(g.read_kv(0, 0, k0.size), k0) and np.array_equal(g.read_kv(1, 0, v0.size), v0)
    assert np.array_equal(g.read_logits(), row0)
    nxt = [123]
    assert np.array_equal(g.eval(nxt, len(ctx_toks)), h.eval(nxt, len(ctx_toks)))
    g.close()
    h.close()


def test_float_files_and_bad_arguments_fail(pkg, files, tiny_models, tries, models):
    for path in (files["f32"], tiny_models["f16"]):
        g = pkg.BiogptModel.load(path)
        t = pkg.Trie.build([[3, 4], [5]], g.hparams.n_vocab)
        with pytest.raises(pkg.BiogptError, match="fast chain"):
            g.generate_beam([2, 5, 7], 4, n_beams=2, eos_id=2, trie=t)
        with pytest.raises(pkg.BiogptError, match="fast chain"):
            g.generate_sample([2, 5, 7], 4, eos_id=2, trie=t)
        t.close()
        g.close()
    g = models["q4_0"]
    other = pkg.Trie.build([[3, 4], [5]], 100)
    bad = [(dict(eos_id=-1), "eos_id"), (dict(eos_id=V), "eos_id"), (dict(eos_id=POOL[0]), "eos_id"), (dict(trie=other), "n_vocab")]
    for kw, field in bad:
        args = dict(eos_id=EOS, trie=tries["small"])
        args.update(kw)
        with pytest.raises(pkg.BiogptError, match=field):
            g.generate_beam([2, 5, 7], 4, n_beams=2, **args)
        with pytest.raises(pkg.BiogptError, match=field):
            g.generate_beam_batch([[2, 5, 7]], 4, n_beams=2, **args)
        with pytest.raises(pkg.BiogptError, match=field):
            g.generate_sample([2, 5, 7], 4, **args)
    for kw, field in ((dict(n_beams=0), "n_beams"), (dict(n_beams=17), "n_beams"), (dict(length_penalty=float("nan")), "length_penalty"), (dict(n_batch=0), "n_batch")):
        with pytest.raises(pkg.BiogptError, match=field):
            g.generate_beam([2, 5, 7], 4, eos_id=EOS, trie=tries["small"], **kw)
    for kw, field in ((dict(top_k=0), "top_k"), (dict(temp=0.0), "temp"), (dict(n_samples=0), "n_samples")):
        with pytest.raises(pkg.BiogptError, match=field):
            g.generate_sample([2, 5, 7], 4, eos_id=EOS, trie=tries["small"], **kw)
    with pytest.raises(pkg.BiogptError, match="n_vocab"):
        pkg.trie_rows(np.zeros((1, V), np.float32), other, [[]], eos_id=EOS)
    other.close()
    hyps, _ = g.generate_beam([2, 5, 7], 4, n_beams=3, eos_id=EOS, trie=tries["small"])      # still usable
    assert 1 <= len(hyps) <= 3
