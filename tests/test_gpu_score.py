"""Sequence scoring (biogpt_hip_score / biogpt_hip_score_batch): teacher-forced causal log-probabilities, the lm_head over every column of
a pass and the log-softmax on the device (kernels_score.hip.h).  Checked against the oracle in causal mode (row i sees tokens 0 .. i), against
the engine's own prompt pass with n_batch = 1 (bit for bit), across pass borders, at full shapes and full depth, and batched."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ALL_TYPES = ["f32", "f16", "q4_0", "q4_1", "q5_0", "q5_1", "q8_0"]
KW = dict(n_vocab=42384, n_layer=3, n_head=16, n_positions=1024, d_ff=4096, d_model=1024, n_merges=40000)
TINY_TOKS = [2] + [(53 * i + 29) % 316 + 4 for i in range(59)]      # 60 tokens (tiny n_positions = 64, n_vocab = 320)


def log_softmax64(rows):
    r = np.asarray(rows, dtype=np.float64)
    m = r.max(axis=-1, keepdims=True)
    return r - m - np.log(np.exp(r - m).sum(axis=-1, keepdims=True))


def next_targets(toks):
    return list(toks[1:]) + [-1]


def check_against_oracle(what, toks, lp, am, lg, ref_rows):
    """logit_out within 1e-3 of the causal oracle's rows, arg-max equal, logprob within 2e-3 of the float64 log-softmax of the oracle rows."""
    tg = next_targets(toks)
    rows = np.arange(len(toks) - 1)
    ref_lg = ref_rows[rows, tg[:-1]]
    d_lg = float(np.abs(lg[:-1] - ref_lg).max())
    exact = int((lg[:-1] == ref_lg).sum())
    ref_lp = log_softmax64(ref_rows)[rows, tg[:-1]]
    d_lp = float(np.abs(lp[:-1].astype(np.float64) - ref_lp).max())
    print("%s: %d rows, target logits max |diff| %.2e (%d/%d bit-identical), logprob max |diff| %.2e"
          % (what, len(toks), d_lg, exact, len(toks) - 1, d_lp))
    assert d_lg <= 1e-3, what
    assert d_lp <= 2e-3, what
    assert (am == ref_rows.argmax(axis=1)).all(), what
    assert lp[-1] == 0.0 and lg[-1] == 0.0


@pytest.fixture(scope="module")
def files(pkg, tmp_path_factory):
    d = tmp_path_factory.mktemp("score_full")
    f32 = str(d / "f32.bin")
    pkg.write_synthetic(f32, **KW)
    out = {"f32": f32}
    for name in ("q4_0", "q5_1", "q8_0", "q4_1", "q5_0"):
        out[name] = str(d / (name + ".bin"))
        pkg.quantize_file(f32, out[name], name)
    return out


def causal_oracle(oracle, path, n_threads):
    o = oracle.OracleModel(path, n_threads=n_threads)
    o.set_mode("ggml", n_threads=n_threads, causal=1)
    return o


# ---- 1. tiny models, every file type, several passes and one pass ----

@pytest.mark.parametrize("cols", [16, 512])
@pytest.mark.parametrize("name", ALL_TYPES)
def test_score_tiny_models_against_causal_oracle(pkg, oracle, tiny_models, monkeypatch, name, cols):
    monkeypatch.setenv("BIOGPT_HIP_PROMPT_COLS", str(cols))
    g = pkg.BiogptModel.load(tiny_models[name])
    g.refresh_options()
    lp, am, lg = g.score(TINY_TOKS)
    ref = causal_oracle(oracle, tiny_models[name], 4).eval(TINY_TOKS, 0, all_rows=True)
    check_against_oracle("tiny %s, %d columns per pass" % (name, cols), TINY_TOKS, lp, am, lg, ref)
    g.close()


# ---- 2. the engine's own prompt pass with n_batch = 1, bit for bit ----

def self_consistency(pkg, path, toks, cols, rows, monkeypatch):
    monkeypatch.setenv("BIOGPT_HIP_PROMPT_COLS", str(cols))
    g = pkg.BiogptModel.load(path)
    h = pkg.BiogptModel.load(path)
    n = len(toks)
    lp, am, lg = g.score(toks)
    tg = next_targets(toks)
    for i in rows:
        row = h.eval_prompt(toks[:i + 1], 0, 1)
        if tg[i] >= 0:
            assert lg[i] == row[tg[i]], (path, i, lg[i], row[tg[i]])
            assert abs(float(lp[i]) - log_softmax64(row)[tg[i]]) <= 1e-4, (path, i)
        else:
            assert lg[i] == 0.0 and lp[i] == 0.0
        assert am[i] == int(np.argmax(row)), (path, i)
    # the K / V rows and the device row afterwards are those of eval_prompt(toks, 0, 1)
    last = h.eval_prompt(toks, 0, 1)
    assert (g.read_logits() == last).all()
    hp = g.hparams
    cnt = hp.n_layer * hp.n_positions * hp.d_model
    for which in (0, 1):
        a = g.read_kv(which, 0, cnt).reshape(hp.n_layer, hp.n_positions, hp.d_model)[:, :n]
        b = h.read_kv(which, 0, cnt).reshape(hp.n_layer, hp.n_positions, hp.d_model)[:, :n]
        assert (a == b).all(), which
    g.close()
    h.close()


@pytest.mark.parametrize("name", ["q4_0", "f32"])
def test_score_equals_prompt_pass_rows_tiny(pkg, tiny_models, monkeypatch, name):
    rows = [0, 15, 16, 31, 32, 47, 48, 59]      # 16 columns per pass: the first row, both sides of every border, the last
    self_consistency(pkg, tiny_models[name], TINY_TOKS, 16, rows, monkeypatch)


def test_score_equals_prompt_pass_rows_full_shape(pkg, files, monkeypatch):
    rng = np.random.default_rng(7)
    toks = [2] + [int(v) for v in rng.integers(4, KW["n_vocab"], 599)]
    rows = [0, 3, 7, 8, 63, 64, 511, 512, 599]    # 512 columns per pass; short prefixes take the chunk / single-token launches of eval_prompt
    self_consistency(pkg, files["q4_0"], toks, 512, rows, monkeypatch)


# ---- 3. causality: splitting a sequence changes nothing ----

@pytest.mark.parametrize("k", [10, 16])
def test_score_split_invariant(pkg, oracle, tiny_models, monkeypatch, k):
    monkeypatch.setenv("BIOGPT_HIP_PROMPT_COLS", "16")
    g = pkg.BiogptModel.load(tiny_models["q4_0"])
    tg = next_targets(TINY_TOKS)
    full = g.score(TINY_TOKS, 0, tg)
    a = g.score(TINY_TOKS[:k], 0, tg[:k])
    b = g.score(TINY_TOKS[k:], k, tg[k:])
    for x, y, z in zip(full, a, b):
        assert (x == np.concatenate([y, z])).all()
    # the next single-token eval continues the sequence
    n = len(TINY_TOKS)
    o = causal_oracle(oracle, tiny_models["q4_0"], 4)
    o.eval(TINY_TOKS, 0, all_rows=True)
    lg, lo = g.eval([17], n), o.eval([17], n)
    assert float(np.abs(lg - lo).max()) <= 1e-3 and int(lg.argmax()) == int(lo.argmax())
    g.close()


# ---- 4. full shapes: passes of 512 + 88 columns, every format; n_positions reached ----

@pytest.mark.parametrize("name", ["q4_0", "q4_1", "q5_0", "q5_1", "q8_0", "f32"])
def test_score_full_shape_600_tokens(pkg, oracle, files, name):
    rng = np.random.default_rng(600)
    toks = [2] + [int(v) for v in rng.integers(4, KW["n_vocab"], 599)]
    g = pkg.BiogptModel.load(files[name])
    lp, am, lg = g.score(toks)
    ref = causal_oracle(oracle, files[name], 16).eval(toks, 0, all_rows=True)
    check_against_oracle("full shape %s" % name, toks, lp, am, lg, ref)
    g.close()


def test_score_full_context_1024_tokens(pkg, oracle, files):
    rng = np.random.default_rng(1024)
    toks = [2] + [int(v) for v in rng.integers(4, KW["n_vocab"], 1023)]
    g = pkg.BiogptModel.load(files["q4_0"])
    lp, am, lg = g.score(toks)
    ref = causal_oracle(oracle, files["q4_0"], 16).eval(toks, 0, all_rows=True)
    check_against_oracle("full shape q4_0, 1024 tokens", toks, lp, am, lg, ref)
    with pytest.raises(pkg.BiogptError):
        g.score(toks + [5])
    g.close()


# ---- 5. full depth ----

def test_score_24_layers_q4_0(pkg, oracle, tmp_path):
    f32, path = str(tmp_path / "f32.bin"), str(tmp_path / "q4_0.bin")
    pkg.write_synthetic(f32, seed=0x42494F47, **dict(KW, n_layer=24))     # the seed of the base24_f32 fixture and the bench
    pkg.quantize_file(f32, path, "q4_0")
    rng = np.random.default_rng(256)
    toks = [2] + [int(v) for v in rng.integers(4, KW["n_vocab"], 255)]
    g = pkg.BiogptModel.load(path)
    lp, am, lg = g.score(toks)
    ref = causal_oracle(oracle, path, 16).eval(toks, 0, all_rows=True)
    check_against_oracle("24 layers q4_0", toks, lp, am, lg, ref)
    g.close()


# ---- 6. batched scoring ----

@pytest.mark.parametrize("cols", [64, 512])
@pytest.mark.parametrize("name", ["q4_0", "q5_1"])
def test_score_batch_equals_single_sequence_scores(pkg, files, monkeypatch, name, cols):
    monkeypatch.setenv("BIOGPT_HIP_PROMPT_COLS", str(cols))
    g = pkg.BiogptModel.load(files[name])
    rng = np.random.default_rng(9)
    lens = [1, 2, 7, 33, 64, 65, 100, 150, 200]
    seqs = [[2] + [int(v) for v in rng.integers(4, KW["n_vocab"], n - 1)] for n in lens]
    targets = []
    for s, seq in enumerate(seqs):
        if s % 3 == 0:
            targets.append(None)                                          # next-token scoring
        else:
            t = [int(v) for v in rng.integers(0, KW["n_vocab"], len(seq))]
            t[0] = -1                                                     # a prompt row that is not scored
            targets.append(t)
    # the context's own cache holds something of its own; batched scoring leaves it alone
    own = [2] + [int(v) for v in rng.integers(4, KW["n_vocab"], 47)]
    g.eval_prompt(own, 0, 8)
    hp = g.hparams
    cnt = hp.n_layer * hp.n_positions * hp.d_model
    kv0 = [g.read_kv(w, 0, cnt) for w in (0, 1)]
    got = g.score_batch(seqs, targets)
    for w in (0, 1):
        assert (g.read_kv(w, 0, cnt) == kv0[w]).all(), "score_batch wrote into the context's own K / V cache"
    got_null = g.score_batch(seqs)                                        # targets == NULL for every sequence
    for s, seq in enumerate(seqs):
        single = g.score(seq, 0, targets[s])
        for x, y in zip(got[s], single):
            assert (x == y).all(), (name, cols, s, len(seq))
        single_null = g.score(seq)
        for x, y in zip(got_null[s], single_null):
            assert (x == y).all(), (name, cols, s, len(seq))
    with pytest.raises(pkg.BiogptError, match="empty sequence"):
        g.score_batch([[2, 5], []])
    lp, _, _ = g.score_batch([[2, 5, 9]])[0]                               # still usable
    assert np.isfinite(lp).all()
    g.close()


@pytest.mark.parametrize("which", ["tiny_f16", "full_f32"])
def test_score_batch_rejects_float_files(pkg, tiny_models, files, which):
    g = pkg.BiogptModel.load(tiny_models["f16"] if which == "tiny_f16" else files["f32"])
    with pytest.raises(pkg.BiogptError, match="fast chain"):
        g.score_batch([[2, 5, 9], [2, 7]])
    lp, _, _ = g.score([2, 5, 9])                                          # single-sequence scoring works for every file type
    assert np.isfinite(lp).all()
    g.close()


# ---- 7. argument errors ----

def test_score_argument_errors(pkg, tiny_models):
    g = pkg.BiogptModel.load(tiny_models["q4_0"])
    with pytest.raises(pkg.BiogptError, match="target id"):
        g.score([2, 5, 9], 0, [5, 320, -1])                               # target >= n_vocab
    with pytest.raises(pkg.BiogptError, match="n_positions"):
        g.score([2, 5, 9], 62)                                            # n_past + n > n_positions
    with pytest.raises(pkg.BiogptError, match="token id"):
        g.score([2, 400], 0)
    with pytest.raises(pkg.BiogptError, match="no tokens"):
        g.score([], 0)
    with pytest.raises(pkg.BiogptError, match="n_seqs"):
        g.score_batch([])
    lp, am, lg = g.score([2, 5, 9])                                       # the context stays usable
    assert np.isfinite(lp).all() and lp[-1] == 0.0
    g.close()
