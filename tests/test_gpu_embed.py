"""Hidden states, pooled embeddings and classification heads (biogpt_hip_hidden / biogpt_hip_embed_batch, kernels_embed.hip.h): the causal passes
of scoring with the final LayerNorm as their last stage.  Checked against the oracle's taps in causal mode, against the engine's own prompt pass
(K / V rows and the next row, bit for bit), batched against single, layer by layer, and -- pooling, normalisation, heads -- against embed_ref in
float64 on the engine's own rows, within bounds that follow from the arithmetic (embed_ref.*_bound)."""
import numpy as np
import pytest

import embed_ref

pytestmark = pytest.mark.gpu

ALL_TYPES = ["f32", "f16", "q4_0", "q4_1", "q5_0", "q5_1", "q8_0"]
KW = dict(n_vocab=42384, n_layer=3, n_head=16, n_positions=1024, d_ff=4096, d_model=1024, n_merges=40000)      # the KW of test_gpu_score.py
TINY_TOKS = [2] + [(53 * i + 29) % 316 + 4 for i in range(59)]      # 60 tokens (tiny n_positions = 64, n_vocab = 320)
LENS = [1, 2, 7, 13, 16, 17, 33, 40, 5]      # at 16 columns per pass: sequences that end on, start on and straddle pass borders


@pytest.fixture(scope="module")
def files(pkg, tmp_path_factory):
    d = tmp_path_factory.mktemp("embed_full")
    f32 = str(d / "f32.bin")
    pkg.write_synthetic(f32, **KW)
    out = {"f32": f32}
    for name in ("q4_0", "q8_0"):
        out[name] = str(d / (name + ".bin"))
        pkg.quantize_file(f32, out[name], name)
    return out


def causal_oracle(oracle, path, n_threads):
    o = oracle.OracleModel(path, n_threads=n_threads)
    o.set_mode("ggml", n_threads=n_threads, causal=1)
    return o


def make_seqs(lens, seed=11):
    rng = np.random.default_rng(seed)
    return [[2] + [int(v) for v in rng.integers(4, KW["n_vocab"], n - 1)] for n in lens]


def report(what, got, ref, tol=1e-3):
    d = float(np.abs(got.astype(np.float64) - ref.astype(np.float64)).max())
    print("%s: %s, max |diff| %.2e, %d/%d elements bit-identical" % (what, got.shape, d, int((got == ref).sum()), got.size))
    assert got.shape == ref.shape and np.isfinite(got).all(), what
    assert d <= tol, what


def within(what, got, ref, bound):
    err = np.abs(got.astype(np.float64) - ref)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print("%s: %s, max |diff| %.2e, at most %.3f of the bound" % (what, got.shape, float(err.max()), worst))
    assert got.dtype == np.float32 and got.shape == ref.shape, what
    assert (err <= bound).all(), what


# ---- 1. hidden states against the oracle's tap after the final LayerNorm ----

@pytest.mark.parametrize("cols", [16, 512])
@pytest.mark.parametrize("name", ALL_TYPES)
def test_hidden_tiny_models_against_causal_oracle(pkg, oracle, tiny_models, monkeypatch, name, cols):
    monkeypatch.setenv("BIOGPT_HIP_PROMPT_COLS", str(cols))
    g = pkg.BiogptModel.load(tiny_models[name])
    g.refresh_options()
    got = g.hidden(TINY_TOKS)
    o = causal_oracle(oracle, tiny_models[name], 4)
    o.eval(TINY_TOKS, 0, all_rows=True)
    report("tiny %s, %d columns per pass" % (name, cols), got, o.tap(g.hparams.n_layer))
    g.close()


@pytest.mark.parametrize("name", ["q4_0", "q8_0", "f32"])
def test_hidden_full_shape_600_tokens(pkg, oracle, files, name):
    toks = make_seqs([600], seed=600)[0]      # passes of 512 + 88 columns
    g = pkg.BiogptModel.load(files[name])
    got = g.hidden(toks)
    o = causal_oracle(oracle, files[name], 16)
    o.eval(toks, 0, all_rows=True)
    report("full shape %s" % name, got, o.tap(KW["n_layer"]))
    g.close()


# ---- 2. the context after hidden(): the K / V rows and the position of eval_prompt(tokens, n_past, 1) ----

def state_after_hidden(pkg, path, toks, n_past, cols, nxt, monkeypatch):
    monkeypatch.setenv("BIOGPT_HIP_PROMPT_COLS", str(cols))
    g = pkg.BiogptModel.load(path)
    h = pkg.BiogptModel.load(path)
    pre, rest = toks[:n_past], toks[n_past:]
    if n_past:
        g.eval_prompt(pre, 0, 1)
        h.eval_prompt(pre, 0, 1)
    hid = g.hidden(rest, n_past)
    h.eval_prompt(rest, n_past, 1)
    n = len(toks)
    hp = g.hparams
    cnt = hp.n_layer * hp.n_positions * hp.d_model
    for which in (0, 1):
        a = g.read_kv(which, 0, cnt).reshape(hp.n_layer, hp.n_positions, hp.d_model)[:, :n]
        b = h.read_kv(which, 0, cnt).reshape(hp.n_layer, hp.n_positions, hp.d_model)[:, :n]
        assert (a == b).all(), which
    ra, rb = g.eval([nxt], n), h.eval([nxt], n)
    assert (ra == rb).all() and np.isfinite(ra).all()
    # and the rows do not depend on where the call started: hidden(all tokens, 0) ends with the same rows
    if n_past:
        full = g.hidden(toks, 0)
        assert (full[n_past:] == hid).all()
    g.close()
    h.close()


@pytest.mark.parametrize("n_past", [0, 10])
@pytest.mark.parametrize("name", ["q4_0", "f32"])
def test_context_after_hidden_tiny(pkg, tiny_models, monkeypatch, name, n_past):
    state_after_hidden(pkg, tiny_models[name], TINY_TOKS, n_past, 16, 17, monkeypatch)


def test_context_after_hidden_full_shape(pkg, files, monkeypatch):
    toks = make_seqs([600], seed=7)[0]
    state_after_hidden(pkg, files["q4_0"], toks, 40, 512, 1234, monkeypatch)


# ---- 3. batch against single; the context's own state is left alone ----

@pytest.mark.parametrize("cols", [16, 512])
def test_embed_batch_rows_equal_hidden_rows(pkg, files, monkeypatch, cols):
    monkeypatch.setenv("BIOGPT_HIP_PROMPT_COLS", str(cols))
    g = pkg.BiogptModel.load(files["q4_0"])
    h = pkg.BiogptModel.load(files["q4_0"])
    seqs = make_seqs(LENS)
    own = make_seqs([48], seed=3)[0]
    g.eval_prompt(own, 0, 8)
    h.eval_prompt(own, 0, 8)
    hp = g.hparams
    cnt = hp.n_layer * hp.n_positions * hp.d_model
    kv0 = [g.read_kv(w, 0, cnt) for w in (0, 1)]
    row0 = g.read_logits()
    got = g.embed_batch(seqs, layer=-1, pooling="none")
    assert [r.shape for r in got] == [(n, 1024) for n in LENS]
    for w in (0, 1):
        assert (g.read_kv(w, 0, cnt) == kv0[w]).all(), "embed_batch wrote into the context's own K / V cache"
    assert (g.read_logits() == row0).all(), "embed_batch changed the context's logits row"
    assert (g.eval([77], len(own)) == h.eval([77], len(own))).all(), "embed_batch moved the context's position"
    for s, seq in enumerate(seqs):
        assert (got[s] == g.hidden(seq)).all(), (cols, s, len(seq))
    g.close()
    h.close()


# ---- 4. the layer index: transformers' hidden_states ----

def test_embed_batch_every_layer_against_oracle_taps(pkg, oracle, files, monkeypatch):
    monkeypatch.setenv("BIOGPT_HIP_PROMPT_COLS", "64")
    g = pkg.BiogptModel.load(files["q4_0"])
    seqs = make_seqs([40, 70, 9], seed=21)
    L = KW["n_layer"]
    taps = []
    o = causal_oracle(oracle, files["q4_0"], 16)
    for seq in seqs:
        o.eval(seq, 0, all_rows=True)
        taps.append([o.tap(k - 1) if k < L else o.tap(L) for k in range(L + 1)])
    for k in range(L + 1):
        got = g.embed_batch(seqs, layer=k, pooling="none")
        for s in range(len(seqs)):
            report("layer %d, sequence %d" % (k, s), got[s], taps[s][k])
    last = g.embed_batch(seqs, layer=-1, pooling="none")
    for s in range(len(seqs)):
        assert (last[s] == got[s]).all()      # -1 is n_layer
    g.close()


# ---- 5. pooling and normalisation ----

@pytest.mark.parametrize("cols", [16, 512])
def test_pooling_and_normalisation(pkg, files, monkeypatch, cols):
    monkeypatch.setenv("BIOGPT_HIP_PROMPT_COLS", str(cols))
    g = pkg.BiogptModel.load(files["q4_0"])
    seqs = make_seqs(LENS + [300], seed=5)
    for layer in (-1, 2):
        rows = g.embed_batch(seqs, layer=layer, pooling="none")
        last = g.embed_batch(seqs, layer=layer, pooling="last")
        mean = g.embed_batch(seqs, layer=layer, pooling="mean")
        assert last.shape == mean.shape == (len(seqs), 1024) and last.dtype == mean.dtype == np.float32
        for s, r in enumerate(rows):
            assert (last[s] == r[-1]).all(), (layer, s)
        within("mean, layer %d" % layer, mean, np.stack([embed_ref.pool(r, "mean") for r in rows]), np.stack([embed_ref.mean_bound(r) for r in rows]))
        assert float(np.abs(mean - last).max()) > 1e-3      # (two different things)
        ln = g.embed_batch(seqs, layer=layer, pooling="last", normalize=True)
        within("last + normalize, layer %d" % layer, ln, embed_ref.l2_normalize(last), embed_ref.normalize_bound(last))
        mn = g.embed_batch(seqs, layer=layer, pooling="mean", normalize=True)
        within("mean + normalize, layer %d" % layer, mn, embed_ref.l2_normalize(mean), embed_ref.normalize_bound(mean))
        nn = g.embed_batch(seqs, layer=layer, pooling="none", normalize=True)
        flat = np.concatenate(rows)
        within("rows + normalize, layer %d" % layer, np.concatenate(nn), embed_ref.l2_normalize(flat), embed_ref.normalize_bound(flat))
        assert float(np.abs(np.sqrt((ln.astype(np.float64) ** 2).sum(axis=1)) - 1.0).max()) <= 1e-6
    g.close()


# ---- 6. heads ----

@pytest.mark.parametrize("cols", [16, 512])
def test_heads(pkg, files, monkeypatch, cols):
    monkeypatch.setenv("BIOGPT_HIP_PROMPT_COLS", str(cols))
    g = pkg.BiogptModel.load(files["q4_0"])
    seqs = make_seqs(LENS, seed=8)
    rng = np.random.default_rng(17)
    W = rng.normal(0.0, 0.05, (7, 1024)).astype(np.float32)
    b = rng.normal(0.0, 0.5, 7).astype(np.float32)
    rows = g.embed_batch(seqs, pooling="none")
    last = np.stack([r[-1] for r in rows])
    flat = np.concatenate(rows)
    got = g.embed_batch(seqs, pooling="last", head=(W, b))
    within("head on the last token's row", got, embed_ref.head(last, W, b), embed_ref.head_bound(last, W, b))
    got = g.embed_batch(seqs, pooling="last", head=W)
    within("head without a bias", got, embed_ref.head(last, W), embed_ref.head_bound(last, W))
    got = g.embed_batch(seqs, pooling="none", head=(W, b))
    assert [r.shape for r in got] == [(n, 7) for n in LENS]
    within("head on every token's row", np.concatenate(got), embed_ref.head(flat, W, b), embed_ref.head_bound(flat, W, b))
    mean = g.embed_batch(seqs, pooling="mean")
    got = g.embed_batch(seqs, pooling="mean", head=(W, b))
    within("head on the mean row", got, embed_ref.head(mean, W, b), embed_ref.head_bound(mean, W, b))
    for n_out in (1, 256):
        Wn = rng.normal(0.0, 0.05, (n_out, 1024)).astype(np.float32)
        bn = rng.normal(0.0, 0.5, n_out).astype(np.float32)
        got = g.embed_batch(seqs, pooling="last", head=(Wn, bn))
        assert got.shape == (len(seqs), n_out)
        within("n_out = %d, pooled" % n_out, got, embed_ref.head(last, Wn, bn), embed_ref.head_bound(last, Wn, bn))
        got = np.concatenate(g.embed_batch(seqs, pooling="none", head=(Wn, bn)))
        within("n_out = %d, every token" % n_out, got, embed_ref.head(flat, Wn, bn), embed_ref.head_bound(flat, Wn, bn))
    g.close()


# ---- 7. repeatability; the captured graphs survive ----

def test_repeatable_and_generation_unchanged(pkg, files, monkeypatch):
    monkeypatch.setenv("BIOGPT_HIP_PROMPT_COLS", "16")
    g = pkg.BiogptModel.load(files["q4_0"])
    seqs = make_seqs(LENS, seed=2)
    prompt = make_seqs([12], seed=4)[0]
    prompts = make_seqs([9, 12, 5, 7], seed=6)
    ids0, _ = g.generate_greedy(prompt, 24)
    batch0, _ = g.generate_greedy_batch(prompts, 16)
    beam0, _ = g.generate_beam(prompt, 12, n_beams=4, eos_id=-1)
    rng = np.random.default_rng(1)
    W = rng.normal(0.0, 0.05, (3, 1024)).astype(np.float32)
    for kw in (dict(pooling="none"), dict(pooling="mean", normalize=True), dict(pooling="mean", head=W), dict(pooling="last", layer=1)):
        a = g.embed_batch(seqs, **kw)      # (9 sequences: more cache slots than the 4 of the batched generation above)
        b = g.embed_batch(seqs, **kw)
        a, b = (np.concatenate(a), np.concatenate(b)) if kw["pooling"] == "none" else (a, b)
        assert a.tobytes() == b.tobytes(), kw
    assert g.hidden(prompt).tobytes() == g.hidden(prompt).tobytes()
    ids1, _ = g.generate_greedy(prompt, 24)
    batch1, _ = g.generate_greedy_batch(prompts, 16)
    beam1, _ = g.generate_beam(prompt, 12, n_beams=4, eos_id=-1)
    assert list(ids0) == list(ids1) and len(ids0) == 24
    assert (batch0 == batch1).all()
    assert [list(i) for i, _ in beam0] == [list(i) for i, _ in beam1] and [s for _, s in beam0] == [s for _, s in beam1]
    g.close()


# ---- 8. the argument errors that need a model; files off the fast chain ----

def test_embed_argument_errors_that_need_the_model(pkg, files):
    g = pkg.BiogptModel.load(files["q4_0"])
    seqs = [[2, 5, 9], [2, 7]]
    with pytest.raises(pkg.BiogptError, match="layer"):
        g.embed_batch(seqs, layer=KW["n_layer"] + 1)
    with pytest.raises(pkg.BiogptError, match="layer"):
        g.embed_batch(seqs, layer=-2)
    with pytest.raises(pkg.BiogptError, match="token id"):
        g.embed_batch([[2, KW["n_vocab"]]])
    with pytest.raises(pkg.BiogptError, match="n_positions"):
        g.embed_batch([[2] * 1025])
    with pytest.raises(pkg.BiogptError, match="empty sequence"):
        g.embed_batch([[2, 5], []])
    with pytest.raises(pkg.BiogptError, match="n_seqs"):
        g.embed_batch([])
    W = np.ones((3, 1024), dtype=np.float32)
    W[2, 1000] = np.nan
    with pytest.raises(pkg.BiogptError, match=r"w\[2\]\[1000\]"):
        g.embed_batch(seqs, head=W)
    with pytest.raises(pkg.BiogptError, match="normalize"):
        g.embed_batch(seqs, head=np.ones((3, 1024), dtype=np.float32), normalize=True)
    with pytest.raises(pkg.BiogptError, match="d_model"):
        g.embed_batch(seqs, head=np.ones((3, 64), dtype=np.float32))
    with pytest.raises(pkg.BiogptError, match="no tokens"):
        g.hidden([])
    with pytest.raises(pkg.BiogptError, match="n_positions"):
        g.hidden([2, 5, 9], 1022)
    out = g.embed_batch(seqs)      # the context stays usable
    assert out.shape == (2, 1024) and np.isfinite(out).all()
    g.close()


@pytest.mark.parametrize("which", ["tiny_f16", "tiny_q4_0", "full_f32"])
def test_embed_batch_rejects_files_off_the_fast_chain(pkg, tiny_models, files, which):
    g = pkg.BiogptModel.load({"tiny_f16": tiny_models["f16"], "tiny_q4_0": tiny_models["q4_0"], "full_f32": files["f32"]}[which])
    with pytest.raises(pkg.BiogptError, match="fast chain"):
        g.embed_batch([[2, 5, 9], [2, 7]])
    assert np.isfinite(g.hidden([2, 5, 9])).all()      # biogpt_hip_hidden serves every file
    g.close()
