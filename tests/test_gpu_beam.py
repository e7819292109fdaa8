"""Beam search (biogpt_hip_generate_beam: the batched search with one prompt, kernels_beam.hip.h) on the GPU: one beam is greedy decoding; the search equals beam_ref (the
restatement pinned to transformers by test_beam_restatement.py) driven by the oracle; its scores are the engine's own scoring of the
hypotheses; the captured, eager and column-per-XCD paths agree; the context's own K / V cache is left alone."""
import numpy as np
import pytest

import beam_ref

pytestmark = pytest.mark.gpu

KW = dict(n_vocab=42384, n_layer=3, n_head=16, n_positions=1024, d_ff=4096, d_model=1024, n_merges=40000)
SEED = 0x42494F47
MARGIN = 1e-5


def prompt_of(n, seed):
    rng = np.random.default_rng(seed)
    return [2] + [int(v) for v in rng.integers(4, KW["n_vocab"], n - 1)]


@pytest.fixture(scope="module")
def files(pkg, tmp_path_factory):
    d = tmp_path_factory.mktemp("beam")
    f32 = str(d / "f32.bin")
    pkg.write_synthetic(f32, **KW)
    out = {"f32": f32}
    for name in ("q4_0", "q5_1", "q8_0"):
        out[name] = str(d / (name + ".bin"))
        pkg.quantize_file(f32, out[name], name)
    return out


@pytest.fixture(scope="module")
def base24(pkg, tmp_path_factory):
    d = tmp_path_factory.mktemp("beam24")
    f32, path = str(d / "f32.bin"), str(d / "q4_0.bin")
    pkg.write_synthetic(f32, seed=SEED, **dict(KW, n_layer=24))     # the seed of the bench
    pkg.quantize_file(f32, path, "q4_0")
    return path


# ---- 1. one beam, no EOS: greedy decoding ----

def check_one_beam_is_greedy(pkg, path, prompt, n_predict):
    g = pkg.BiogptModel.load(path)
    for nb in (1, 8):
        want, _ = g.generate_greedy(prompt, n_predict, n_batch=nb)
        hyps, _ = g.generate_beam(prompt, n_predict, n_beams=1, eos_id=-1, n_batch=nb)
        assert len(hyps) == 1
        assert list(hyps[0][0]) == list(want), (nb, list(hyps[0][0]), list(want))
    g.close()


def test_one_beam_is_greedy_3_layers(pkg, files):
    check_one_beam_is_greedy(pkg, files["q4_0"], prompt_of(21, 1), 24)


def test_one_beam_is_greedy_24_layers(pkg, base24):
    check_one_beam_is_greedy(pkg, base24, prompt_of(40, 2), 32)


# ---- 2. the restatement, driven by the oracle ----

ORACLE_PROMPT = prompt_of(13, 3)
N_PREDICT = 10


@pytest.fixture(scope="module")
def oracle_rows(oracle, files):
    """One OracleLogprobs per (file, n_batch) shared by all cases (rows are cached per prefix), and the EOS id of each file: the
    third token of the best EOS-free hypothesis of a first restatement run (so that EOS fires mid-run)."""
    cache, eos = {}, {}

    def get(name, nb):
        if (name, nb) not in cache:
            o = oracle.OracleModel(files[name], n_threads=16)
            cache[(name, nb)] = beam_ref.OracleLogprobs(o, ORACLE_PROMPT, nb)
        return cache[(name, nb)]

    def eos_of(name):
        if name not in eos:
            hyps, _ = beam_ref.beam_search(get(name, 8), 4, N_PREDICT, -1, 1.0, True)
            eos[name] = int(hyps[0][0][2])
        return eos[name]
    return get, eos_of


def check_against_restatement(pkg, files, oracle_rows, name, B, nb, es):
    get, eos_of = oracle_rows
    eos = eos_of(name)
    want, margins = beam_ref.beam_search(get(name, nb), B, N_PREDICT, eos, 1.0, es)
    small = [(k + 1, m) for k, m in enumerate(margins) if m < MARGIN]
    assert not small, "fixture problem: selection margins below %g at steps %s -- the case cannot tell the engine's rounding from a wrong choice" % (MARGIN, small)
    g = pkg.BiogptModel.load(files[name])
    got, _ = g.generate_beam(ORACLE_PROMPT, N_PREDICT, n_beams=B, eos_id=eos, length_penalty=1.0, early_stopping=es, n_batch=nb)
    g.close()
    assert len(got) == len(want) == B
    for r, ((ids_w, s_w), (ids_g, s_g)) in enumerate(zip(want, got)):
        assert list(ids_g) == list(ids_w), (r, list(ids_g), list(ids_w))
        assert abs(float(s_g) - float(s_w)) <= 1e-4, (r, float(s_g), float(s_w))
    print("%s B=%d n_batch=%d early_stopping=%s eos=%d: %d steps, lengths %s" % (name, B, nb, es, eos, len(margins), [len(h[0]) for h in got]))


@pytest.mark.parametrize("es", [True, False])
@pytest.mark.parametrize("nb", [1, 8])
@pytest.mark.parametrize("B", [2, 4, 5, 8])
@pytest.mark.parametrize("name", ["q4_0", "q5_1", "q8_0"])
def test_beam_against_restatement(pkg, files, oracle_rows, name, B, nb, es):
    check_against_restatement(pkg, files, oracle_rows, name, B, nb, es)


@pytest.mark.parametrize("es", [True, False])
def test_twelve_beams_against_restatement(pkg, files, oracle_rows, es):
    """24 candidates per row (the 32-entry instantiation of the row kernel) and up to 11 forks in a step, more than the 8 copy workgroups a
    (layer, head) has: they stride over the fork list."""
    check_against_restatement(pkg, files, oracle_rows, "q4_0", 12, 8, es)


def test_eos_fires_in_the_restatement_cases(oracle_rows):
    """The fixture's EOS ends hypotheses mid-run (else the cases above test no finishing)."""
    get, eos_of = oracle_rows
    eos = eos_of("q4_0")
    hyps, _ = beam_ref.beam_search(get("q4_0", 8), 5, N_PREDICT, eos, 1.0, True)
    assert any(len(ids) < N_PREDICT and ids[-1] == eos for ids, _ in hyps)


# ---- 3. the scores are the engine's own scoring of the hypotheses ----

def check_self_consistent(pkg, path, prompt, n_predict, B=5):
    g = pkg.BiogptModel.load(path)
    hyps, _ = g.generate_beam(prompt, n_predict, n_beams=B, eos_id=-1, length_penalty=1.0, early_stopping=True, n_batch=1)
    assert len(hyps) == B
    n0, worst, exact = len(prompt), 0.0, 0
    for ids, s in hyps:
        toks = list(prompt) + [int(t) for t in ids]
        lp, _, _ = g.score(toks)
        acc = np.float32(0.0)
        for j in range(len(ids)):     # row n0 - 1 + j predicts generated token j
            acc = np.float32(acc + lp[n0 - 1 + j])
        want = beam_ref.normalize(acc, len(ids), 1.0)
        exact += int(want == np.float32(s))
        worst = max(worst, abs(float(want) - float(s)) / max(1.0, abs(float(want))))
    g.close()
    print("self-consistency %s: %d/%d scores bit-identical, worst relative difference %.3g" % (path, exact, B, worst))
    return exact, worst


def test_scores_are_the_engines_own_24_layers(pkg, base24):
    exact, worst = check_self_consistent(pkg, base24, prompt_of(40, 4), 64)
    assert exact == 5, worst      # the batched decode column is the single-sequence row bit for bit


def test_scores_are_the_engines_own_past_256_keys(pkg, base24):
    exact, worst = check_self_consistent(pkg, base24, prompt_of(240, 5), 32)
    assert exact == 5, worst


# ---- 4. the paths agree ----

def test_paths_agree(pkg, files, monkeypatch):
    prompt = prompt_of(30, 6)
    g = pkg.BiogptModel.load(files["q4_0"])
    runs = {}
    for label, env in (("default", {}), ("repeat", {}), ("xcols off", {"BIOGPT_HIP_XCOLS": "0"}), ("no graph", {"BIOGPT_HIP_NO_GRAPH": "1"})):
        for k in ("BIOGPT_HIP_XCOLS", "BIOGPT_HIP_NO_GRAPH"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        g.refresh_options()
        for B in (2, 5, 12):
            hyps, _ = g.generate_beam(prompt, 40, n_beams=B, eos_id=-1, length_penalty=1.0, early_stopping=False, n_batch=8)
            runs.setdefault(B, []).append((label, [(list(i), float(s)) for i, s in hyps]))
    g.close()
    for B, rs in runs.items():
        for label, r in rs[1:]:
            assert r == rs[0][1], (B, label)


# ---- 5. the context is left alone; arguments ----

def test_context_cache_untouched_and_eval_follows(pkg, files):
    g = pkg.BiogptModel.load(files["q4_0"])
    h = pkg.BiogptModel.load(files["q4_0"])
    ctx_toks = prompt_of(9, 7)
    g.eval(ctx_toks, 0)
    h.eval(ctx_toks, 0)
    D = KW["d_model"]
    k0, v0 = g.read_kv(0, 0, 3 * KW["n_positions"] * D), g.read_kv(1, 0, 3 * KW["n_positions"] * D)
    hyps, _ = g.generate_beam(prompt_of(17, 8), 12, n_beams=4, eos_id=-1, n_batch=8)
    assert len(hyps) == 4
    assert np.array_equal(g.read_kv(0, 0, k0.size), k0) and np.array_equal(g.read_kv(1, 0, v0.size), v0)
    nxt = [123]
    assert np.array_equal(g.eval(nxt, len(ctx_toks)), h.eval(nxt, len(ctx_toks)))
    g.close()
    h.close()


def test_float_files_and_bad_arguments_fail(pkg, files, tiny_models):
    for path in (files["f32"], tiny_models["f16"]):
        g = pkg.BiogptModel.load(path)
        with pytest.raises(pkg.BiogptError, match="fast chain"):
            g.generate_beam([2, 5, 7], 4, n_beams=2)
        g.close()
    g = pkg.BiogptModel.load(files["q4_0"])
    for kw, msg in ((dict(n_beams=0), "n_beams"), (dict(n_beams=17), "n_beams"), (dict(n_batch=0), "n_batch"),
                    (dict(eos_id=KW["n_vocab"]), "eos_id"), (dict(eos_id=-2), "eos_id")):
        with pytest.raises(pkg.BiogptError, match=msg):
            g.generate_beam([2, 5, 7], 4, **kw)
    with pytest.raises(pkg.BiogptError):
        g.generate_beam([2, 5, KW["n_vocab"]], 4)
    assert g.generate_beam([2] * KW["n_positions"], 4)[0] == []
    hyps, _ = g.generate_beam([2, 5, 7], 4, n_beams=3, eos_id=-1)      # still usable
    assert len(hyps) == 3 and all(len(i) == 4 for i, _ in hyps)
    g.close()
