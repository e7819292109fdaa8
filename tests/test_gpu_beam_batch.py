"""Beam search over a batch of prompts (biogpt_hip_generate_beam_batch, kernels_beam.hip.h) on the GPU.  The searches of a call are independent:
for every prompt the batched call returns what the call with that prompt alone returns (biogpt_hip_generate_beam_rules, a group of one; n_predict
clamped for the longest prompt), hypothesis for hypothesis, ids and f32 scores bit for bit -- whatever the number of columns (chunk kernel,
8-column chain, matrix cores), with groups that finish at different steps, with rules, captured or eager.  What a search computes is held to
beam_ref (the restatement pinned to transformers) driven by the oracle, here for one batch per weight type and in test_gpu_beam.py for single
calls.  The context's own K / V cache and position are left alone."""
import ctypes

import numpy as np
import pytest

import beam_ref

pytestmark = pytest.mark.gpu

KW = dict(n_vocab=42384, n_layer=3, n_head=16, n_positions=1024, d_ff=4096, d_model=1024, n_merges=40000)
SEED = 0x42494F47
MARGIN = 1e-5
LENS = (7, 13, 21, 40)
N_PREDICT = 12


def prompt_of(n, seed):
    rng = np.random.default_rng(seed)
    return [2] + [int(v) for v in rng.integers(4, KW["n_vocab"], n - 1)]


PROMPTS = [prompt_of(n, 20 + i) for i, n in enumerate(LENS)]
MANY = [prompt_of(LENS[i % 4], 100 + i) for i in range(16)]


@pytest.fixture(scope="module")
def files(pkg, tmp_path_factory):
    d = tmp_path_factory.mktemp("beam_batch")
    f32 = str(d / "f32.bin")
    pkg.write_synthetic(f32, **KW)
    out = {"f32": f32}
    for name in ("q4_0", "q5_1", "q8_0"):
        out[name] = str(d / (name + ".bin"))
        pkg.quantize_file(f32, out[name], name)
    return out


@pytest.fixture(scope="module")
def models(pkg, files):
    """One context per file for the whole module (a call leaves nothing behind that the next one reads: test_neutral checks that)."""
    ms = {name: pkg.BiogptModel.load(files[name]) for name in ("q4_0", "q5_1", "q8_0")}
    yield ms
    for m in ms.values():
        m.close()


@pytest.fixture(scope="module")
def base24(pkg, tmp_path_factory):
    d = tmp_path_factory.mktemp("beam_batch24")
    f32, path = str(d / "f32.bin"), str(d / "q4_0.bin")
    pkg.write_synthetic(f32, seed=SEED, **dict(KW, n_layer=24))     # the seed of the bench
    pkg.quantize_file(f32, path, "q4_0")
    return path


def norm(hyps):
    """ids as int lists, scores as the f32 values they are (compared with ==)."""
    return [([int(t) for t in ids], float(np.float32(s))) for ids, s in hyps]


def singles(g, prompts, n_predict, **kw):
    """The definition's right-hand side: generate_beam of every prompt alone, n_predict clamped for the longest prompt."""
    n = min(n_predict, KW["n_positions"] - max(len(p) for p in prompts))
    return [norm(g.generate_beam(p, n, **kw)[0]) for p in prompts]


def batched(g, prompts, n_predict, **kw):
    return [norm(h) for h in g.generate_beam_batch(prompts, n_predict, **kw)[0]]


def eos_from_free_run(g, prompt, B=4):
    """As test_gpu_beam.py chooses it: the third token of the best hypothesis of an EOS-free run, so that EOS fires mid-run."""
    hyps, _ = g.generate_beam(prompt, N_PREDICT, n_beams=B, eos_id=-1)
    return int(hyps[0][0][2])


def assert_equal(got, want, what):
    assert len(got) == len(want), what
    for p, (a, b) in enumerate(zip(got, want)):
        assert len(a) == len(b), (what, "prompt", p, "count", len(a), len(b))          # counts
        for r, ((ia, sa), (ib, sb)) in enumerate(zip(a, b)):
            assert ia == ib, (what, "prompt", p, "hypothesis", r, ia, ib)                # ids and lengths
            assert sa == sb, (what, "prompt", p, "hypothesis", r, sa, sb)                # f32 scores, ==


# ---- 1. equals the single call, bit for bit ----

@pytest.mark.parametrize("es", [True, False])
@pytest.mark.parametrize("nb", [1, 8])
@pytest.mark.parametrize("B", [1, 2, 5, 8])
@pytest.mark.parametrize("name", ["q4_0", "q5_1", "q8_0"])
def test_equals_single_calls(models, name, B, nb, es):
    """4 prompts of 7 / 13 / 21 / 40 tokens: 4, 8, 20 and 32 columns (the chunk kernel, column-per-XCD launches, the 8-column chain)."""
    g = models[name]
    eos = eos_from_free_run(g, PROMPTS[1])
    kw = dict(n_beams=B, eos_id=eos, length_penalty=1.0, early_stopping=es, n_batch=nb)
    assert_equal(batched(g, PROMPTS, N_PREDICT, **kw), singles(g, PROMPTS, N_PREDICT, **kw), (name, B, nb, es))


@pytest.mark.parametrize("G,B", [(16, 5), (16, 8), (13, 3)])
@pytest.mark.parametrize("name", ["q4_0", "q5_1", "q8_0"])
def test_equals_single_calls_many_columns(models, name, G, B):
    """80 and 128 columns (the chain on the matrix cores), 39 columns (the 8-column chain with a ragged tail)."""
    g = models[name]
    eos = eos_from_free_run(g, MANY[0])
    kw = dict(n_beams=B, eos_id=eos, length_penalty=0.8, early_stopping=True, n_batch=8)
    assert_equal(batched(g, MANY[:G], N_PREDICT, **kw), singles(g, MANY[:G], N_PREDICT, **kw), (name, G, B))


def test_equals_single_calls_24_layers(pkg, base24):
    g = pkg.BiogptModel.load(base24)
    prompts = [prompt_of(n, 40 + i) for i, n in enumerate((40, 25, 40, 9, 33, 40, 17, 40, 40, 12, 40, 40, 28))]
    for B, n_predict in ((5, 32), (1, 16)):      # 65 columns (matrix cores), 13 columns
        kw = dict(n_beams=B, eos_id=-1, length_penalty=1.0, early_stopping=True, n_batch=8)
        assert_equal(batched(g, prompts, n_predict, **kw), singles(g, prompts, n_predict, **kw), ("24 layers", B))
    g.close()


def test_long_prompt_clamps_n_predict_for_all(models):
    """n_predict' = n_positions - max(prompt_lens) holds for every prompt of the batch, the short ones included."""
    g = models["q4_0"]
    prompts = [prompt_of(1018, 60), prompt_of(9, 61)]
    kw = dict(n_beams=3, eos_id=-1, n_batch=8)
    got = batched(g, prompts, 20, **kw)
    assert all(len(ids) == 6 for h in got for ids, _ in h)
    assert_equal(got, singles(g, prompts, 20, **kw), "clamped")
    assert g.generate_beam_batch([prompt_of(1024, 62), [2, 5]], 4)[0] == [[], []]


# ---- 2. groups finish at different steps ----

def test_groups_finish_at_different_steps(models):
    """With early_stopping a search stops at the step that fills its pool, so the longest hypothesis of a prompt is the step its group finished
    at.  The EOS id comes from EOS-free single calls: the first of their early tokens for which the single calls end at least 3 steps apart."""
    g = models["q4_0"]
    n_predict, chosen = 16, None
    free = [norm(g.generate_beam(p, n_predict, n_beams=4, eos_id=-1)[0]) for p in PROMPTS]
    cands = [t for h in free for ids, _ in h for t in ids[1:8]]
    for B in (2, 3, 4, 1):      # (one beam last: its pool is full with the first EOS, which always ends a group early)
        for eos in dict.fromkeys(cands):
            want = singles(g, PROMPTS, n_predict, n_beams=B, eos_id=eos, early_stopping=True)
            ends = [max(len(ids) for ids, _ in h) for h in want]
            if max(ends) - min(ends) >= 3:
                chosen = (B, eos, want, ends)
                break
        if chosen:
            break
    assert chosen, "fixture problem: no EOS id among the EOS-free hypotheses' early tokens makes the single searches end 3 steps apart"
    B, eos, want, ends = chosen
    got = batched(g, PROMPTS, n_predict, n_beams=B, eos_id=eos, early_stopping=True)
    got_ends = [max(len(ids) for ids, _ in h) for h in got]
    print("B=%d eos=%d: groups finished at steps %s" % (B, eos, got_ends))
    assert max(got_ends) - min(got_ends) >= 3, got_ends      # it happened in the batched call
    assert_equal(got, want, ("finish apart", B, eos))


# ---- 3. the restatement, driven by the oracle ----

@pytest.mark.parametrize("name", ["q4_0", "q5_1", "q8_0"])
def test_batch_against_restatement(models, oracle, files, name):
    g = models[name]
    B, nb, n_predict = 4, 8, 10
    prompts = [prompt_of(13, 3), prompt_of(9, 71), prompt_of(17, 72)]
    rows = [beam_ref.OracleLogprobs(oracle.OracleModel(files[name], n_threads=16), p, nb) for p in prompts]
    eos = int(beam_ref.beam_search(rows[0], B, n_predict, -1, 1.0, True)[0][0][0][2])
    want = []
    for p, r in enumerate(rows):
        hyps, margins = beam_ref.beam_search(r, B, n_predict, eos, 1.0, True)
        small = [(k + 1, m) for k, m in enumerate(margins) if m < MARGIN]
        assert not small, "fixture problem: prompt %d, selection margins below %g at steps %s -- the case cannot tell the engine's rounding from a wrong choice" % (p, MARGIN, small)
        want.append(hyps)
    got, _ = g.generate_beam_batch(prompts, n_predict, n_beams=B, eos_id=eos, length_penalty=1.0, early_stopping=True, n_batch=nb)
    assert len(got) == len(want)
    for p, (hw, hg) in enumerate(zip(want, got)):
        assert len(hg) == len(hw), (p, len(hg), len(hw))
        for r, ((ids_w, s_w), (ids_g, s_g)) in enumerate(zip(hw, hg)):
            assert list(ids_g) == list(ids_w), (p, r, list(ids_g), list(ids_w))
            assert abs(float(s_g) - float(s_w)) <= 1e-4, (p, r, float(s_g), float(s_w))


# ---- 4. rules ----

RULES = dict(repetition_penalty=0.7, no_repeat_ngram_size=3, min_new_tokens=5, suppress_tokens=[11, 12, 13])


def looped(n, seed):
    """A prompt that repeats itself, so that the n-gram rule and the penalty have something to act on."""
    p = prompt_of(max(4, n // 2), seed)
    return (p + p[1:] + p[1:])[:n]


@pytest.mark.parametrize("B", [2, 5])
@pytest.mark.parametrize("name", ["q4_0", "q8_0"])
def test_rules_equal_single_calls(models, name, B):
    g = models[name]
    prompts = [looped(n, 80 + i) for i, n in enumerate(LENS)]
    eos = eos_from_free_run(g, prompts[1])
    kw = dict(n_beams=B, eos_id=eos, early_stopping=True, n_batch=8)
    with_rules = batched(g, prompts, N_PREDICT, **kw, **RULES)
    assert_equal(with_rules, singles(g, prompts, N_PREDICT, **kw, **RULES), (name, B, "rules"))
    assert with_rules != batched(g, prompts, N_PREDICT, **kw), "the rules changed nothing: the case tests no rule"


def test_rules_off_is_rules_null(pkg, models):
    g = models["q4_0"]
    G, B, n = len(PROMPTS), 3, N_PREDICT
    flat = np.ascontiguousarray(np.concatenate([np.asarray(p, dtype=np.int32) for p in PROMPTS]))
    lens = np.asarray([len(p) for p in PROMPTS], dtype=np.int32)
    off, keep = pkg.gen_rules()
    outs = []
    for rules in (None, ctypes.byref(off)):
        ids, ol = np.zeros((G, B, n), dtype=np.int32), np.zeros((G, B), dtype=np.int32)
        sc, cnt = np.zeros((G, B), dtype=np.float32), np.zeros(G, dtype=np.int32)
        rc = pkg.lib().biogpt_hip_generate_beam_batch(g._h, flat.ctypes.data, lens.ctypes.data, G, 8, B, n, -1, 1.0, 1, rules, ids.ctypes.data, ol.ctypes.data,
                                                      sc.ctypes.data, cnt.ctypes.data, None)
        assert rc == n, pkg._err()
        outs.append((ids, ol, sc, cnt))
    for a, b in zip(*outs):
        assert np.array_equal(a, b)
    assert (outs[0][3] == B).all() and (outs[0][0][:, :, -1] >= 0).all()


# ---- 5. paths and neutrality ----

def test_paths_agree(pkg, files, monkeypatch):
    g = pkg.BiogptModel.load(files["q4_0"])
    runs = {}
    for label, env in (("default", {}), ("repeat", {}), ("xcols off", {"BIOGPT_HIP_XCOLS": "0"}), ("no graph", {"BIOGPT_HIP_NO_GRAPH": "1"})):
        for k in ("BIOGPT_HIP_XCOLS", "BIOGPT_HIP_NO_GRAPH"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        g.refresh_options()
        for G, B in ((4, 2), (4, 5), (16, 5)):
            for rules in ({}, RULES):
                runs.setdefault((G, B, bool(rules)), []).append((label, batched(g, MANY[:G], 24, n_beams=B, eos_id=-1, early_stopping=False, n_batch=8, **rules)))
    g.close()
    for key, rs in runs.items():
        for label, r in rs[1:]:
            assert r == rs[0][1], (key, label)


def test_one_prompt_is_generate_beam(models):
    g = models["q5_1"]
    for B in (1, 4, 16):
        kw = dict(n_beams=B, eos_id=-1, length_penalty=1.3, early_stopping=False, n_batch=8)
        assert batched(g, [PROMPTS[2]], 20, **kw) == [norm(g.generate_beam(PROMPTS[2], 20, **kw)[0])]
        assert batched(g, PROMPTS[2], 20, **kw) == batched(g, [PROMPTS[2]], 20, **kw)      # (one flat id list)


def test_neutral_for_single_calls_and_the_context(pkg, files):
    g = pkg.BiogptModel.load(files["q4_0"])
    h = pkg.BiogptModel.load(files["q4_0"])
    ctx_toks = prompt_of(9, 7)
    g.eval(ctx_toks, 0)
    h.eval(ctx_toks, 0)
    D = KW["d_model"]
    k0, v0 = g.read_kv(0, 0, 3 * KW["n_positions"] * D), g.read_kv(1, 0, 3 * KW["n_positions"] * D)
    kw = dict(n_beams=4, eos_id=-1, n_batch=8)
    before = norm(g.generate_beam(PROMPTS[1], 12, **kw)[0])
    got = batched(g, PROMPTS, 12, **kw)
    after = norm(g.generate_beam(PROMPTS[1], 12, **kw)[0])
    assert before == after == got[1]
    assert np.array_equal(g.read_kv(0, 0, k0.size), k0) and np.array_equal(g.read_kv(1, 0, v0.size), v0)
    nxt = [123]
    assert np.array_equal(g.eval(nxt, len(ctx_toks)), h.eval(nxt, len(ctx_toks)))      # the position too
    g.close()
    h.close()


# ---- 6. limits ----

def test_512_columns_run(models):
    """n_prompts * n_beams = 512: 32 prompts x 16 beams; a few of its prompts against the single call."""
    g = models["q4_0"]
    prompts = [prompt_of(5 + i % 9, 200 + i) for i in range(32)]
    kw = dict(n_beams=16, eos_id=-1, n_batch=8)
    got = batched(g, prompts, 6, **kw)
    assert len(got) == 32 and all(len(h) == 16 and all(len(ids) == 6 for ids, _ in h) for h in got)
    for p in (0, 13, 31):
        assert got[p] == norm(g.generate_beam(prompts[p], 6, **kw)[0]), p


def test_float_files_and_bad_arguments_fail(pkg, files, tiny_models):
    for path in (files["f32"], tiny_models["f16"]):
        g = pkg.BiogptModel.load(path)
        with pytest.raises(pkg.BiogptError, match="fast chain"):
            g.generate_beam_batch([[2, 5, 7]], 4, n_beams=2)
        g.close()
    g = pkg.BiogptModel.load(files["q4_0"])
    two = [[2, 5, 7], [2, 9]]
    for kw, msg in ((dict(n_beams=0), "n_beams"), (dict(n_beams=17), "n_beams"), (dict(n_batch=0), "n_batch"), (dict(eos_id=KW["n_vocab"]), "eos_id"),
                    (dict(eos_id=-2), "eos_id"), (dict(length_penalty=float("inf")), "length_penalty"), (dict(repetition_penalty=0.0), "repetition_penalty"),
                    (dict(no_repeat_ngram_size=-1), "no_repeat_ngram_size"), (dict(min_new_tokens=-1), "min_new_tokens"),
                    (dict(suppress_tokens=[KW["n_vocab"]]), "suppress")):
        with pytest.raises(pkg.BiogptError, match=msg):
            g.generate_beam_batch(two, 4, **kw)
    with pytest.raises(pkg.BiogptError, match="n_prompts x n_beams"):
        g.generate_beam_batch([[2, 5]] * 57, 4, n_beams=9)      # 513
    with pytest.raises(pkg.BiogptError, match="n_prompts"):
        g.generate_beam_batch([], 4)
    with pytest.raises(pkg.BiogptError, match="empty prompt"):
        g.generate_beam_batch([[2, 5], []], 4)
    with pytest.raises(pkg.BiogptError):
        g.generate_beam_batch([[2, 5], [2, 5, KW["n_vocab"]]], 4)      # a bad token
    L, a = pkg.lib(), np.zeros(64, dtype=np.int32)
    f = np.zeros(64, dtype=np.float32)
    args = [g._h, a.ctypes.data, a.ctypes.data, 1, 8, 2, 4, -1, 1.0, 2, None, a.ctypes.data, a.ctypes.data, f.ctypes.data, a.ctypes.data, None]
    assert L.biogpt_hip_generate_beam_batch(*args) == -1 and "early_stopping" in pkg._err()
    for i in (1, 2, 11, 12, 13, 14):      # each pointer in turn
        bad = list(args)
        bad[9], bad[i] = 1, None
        assert L.biogpt_hip_generate_beam_batch(*bad) == -1 and "null argument" in pkg._err(), i
    hyps, _ = g.generate_beam_batch(two, 4, n_beams=3, eos_id=-1)      # still usable
    assert [len(h) for h in hyps] == [3, 3] and all(len(i) == 4 for h in hyps for i, _ in h)
    g.close()
