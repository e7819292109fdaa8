"""The SIMD association (biogpt_hip_assoc, mode 1; csrc/kernels_assoc.hip.h): whole calls of a context in mode 1 against the oracle with bo_opts.assoc = 3 --
the logits, K / V rows and greedy ids of an AVX2 build of the reference -- bit for bit.

Files: a tiny one (d_model 128, 2 heads, 1 layer, d_ff 256: rows of 4 and 8 blocks) in all five block formats, and the 3-layer BioGPT-base-width file of
tests/test_oracle_assoc.py in Q4_0 and Q5_1.  Every comparison is equality."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TINY = dict(n_vocab=256, n_layer=1, n_head=2, n_positions=384, d_ff=256, d_model=128, n_merges=16)
BASE = dict(n_vocab=42384, n_layer=3, n_head=16, n_positions=1024, d_ff=4096, d_model=1024, n_merges=40000)
KW = {"tiny": TINY, "base": BASE}
MODELS = [("tiny", "q4_0"), ("tiny", "q4_1"), ("tiny", "q5_0"), ("tiny", "q5_1"), ("tiny", "q8_0"), ("base", "q4_0"), ("base", "q5_1")]
IDS = ["%s-%s" % m for m in MODELS]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def seq_of(fam, n, seed):
    rng = np.random.default_rng(seed)
    return [2] + [int(v) for v in rng.integers(4, KW[fam]["n_vocab"], n - 1)]


@pytest.fixture(scope="module")
def files(pkg, tmp_path_factory):
    d = tmp_path_factory.mktemp("assoc")
    out = {}
    for fam in ("tiny", "base"):
        f32 = str(d / ("%s_f32.bin" % fam))
        pkg.write_synthetic(f32, **KW[fam])
        out[(fam, "f32")] = f32
        for f, name in MODELS:
            if f == fam:
                out[(fam, name)] = str(d / ("%s_%s.bin" % (fam, name)))
                pkg.quantize_file(f32, out[(fam, name)], name)
    return out


@pytest.fixture(scope="module")
def models(pkg, files):
    """One context in the SIMD association per file for the whole module, loaded when first asked for."""
    ms = {}

    def get(fam, name):
        if (fam, name) not in ms:
            ms[(fam, name)] = pkg.BiogptModel.load(files[(fam, name)], assoc="simd")
        return ms[(fam, name)]
    yield get
    for m in ms.values():
        m.close()


def simd_oracle(oracle, path, causal=None):
    o = oracle.OracleModel(path, n_threads=8, assoc=3)
    if causal is not None:
        o.set_mode("ggml", 8, causal=causal)
    return o


def kv_rows(g, hp, n):
    """Both caches of the first n positions of every layer: float32 [2][n_layer][n][d_model]."""
    L, P, D = hp["n_layer"], hp["n_positions"], hp["d_model"]
    return np.stack([np.stack([g.read_kv(w, (l * P) * D, n * D).reshape(n, D) for l in range(L)]) for w in (0, 1)])


@pytest.mark.parametrize("fam,name", MODELS, ids=IDS)
def test_decode_logits_and_caches(oracle, files, models, fam, name):
    """A chunk of 8, then 8 single-token evals: every logits row and both caches."""
    g, o = models(fam, name), simd_oracle(oracle, files[(fam, name)])
    assert g.assoc == "simd" and g.chain_kind() == 0 and g.xpipe_state() <= 0
    toks = seq_of(fam, 16, 1)
    assert (bits(g.eval(toks[:8], 0)) == bits(o.eval(toks[:8], 0))).all()
    for i in range(8, 16):
        assert (bits(g.eval([toks[i]], i)) == bits(o.eval([toks[i]], i))).all(), i
    hp = KW[fam]
    got = kv_rows(g, hp, 16)
    for w in (0, 1):
        assert (bits(got[w]) == bits(o.kv(w)[:, :16, :])).all(), w
    o.close()


@pytest.mark.parametrize("fam,name", MODELS, ids=IDS)
def test_eval_all_rows_and_hidden(oracle, files, models, fam, name):
    g, o = models(fam, name), simd_oracle(oracle, files[(fam, name)])
    toks = seq_of(fam, 11, 2)
    assert (bits(g.eval_all(toks, 0)) == bits(o.eval(toks, 0, all_rows=True))).all()
    oc = simd_oracle(oracle, files[(fam, name)], causal=1)
    oc.eval(toks, 0, all_rows=True)
    assert (bits(g.hidden(toks)) == bits(oc.tap(KW[fam]["n_layer"]))).all()
    o.close(); oc.close()


@pytest.mark.parametrize("fam,name", MODELS, ids=IDS)
def test_generate_greedy_ids(oracle, files, models, fam, name):
    g, o = models(fam, name), simd_oracle(oracle, files[(fam, name)])
    prompt = seq_of(fam, 11, 3)
    ids, _ = g.generate_greedy(prompt, 12)
    ref, _ = o.generate_greedy(prompt, 12)
    assert list(ids) == list(ref)
    o.close()


@pytest.mark.parametrize("fam,name", [("tiny", "q4_1"), ("tiny", "q8_0"), ("base", "q4_0")], ids=["tiny-q4_1", "tiny-q8_0", "base-q4_0"])
def test_score_is_the_contexts_own_loop_of_evals(models, fam, name):
    g = models(fam, name)
    toks = seq_of(fam, 10, 4)
    lp, am, tl = g.score(toks)
    rows = np.stack([g.eval([t], i) for i, t in enumerate(toks)])
    assert list(am) == [int(r.argmax()) for r in rows]
    want = np.array([rows[i][toks[i + 1]] for i in range(len(toks) - 1)], dtype=np.float32)
    assert (bits(tl[:len(toks) - 1]) == bits(want)).all()
    assert np.isfinite(lp[:len(toks) - 1]).all()


def test_eval_prompt_topk_device_and_inplace_forms(oracle, files, models):
    """The other single-sequence entries, on the tiny Q5_0 file: each returns the oracle's row."""
    g, o = models("tiny", "q5_0"), simd_oracle(oracle, files[("tiny", "q5_0")])
    toks = seq_of("tiny", 21, 5)
    want = None
    for at in range(0, 21, 8):
        want = o.eval(toks[at:at + 8], at)
    assert (bits(g.eval_prompt(toks, 0, 8)) == bits(want)).all()
    nxt = int(want.argmax())
    want = o.eval([nxt], 21)
    vals, ids = g.eval_topk([nxt], 21, 5)
    order = np.lexsort((np.arange(want.size), -want.astype(np.float64)))[:5]
    assert list(ids) == [int(i) for i in order] and (bits(vals) == bits(want[order])).all()
    g.eval_device([nxt], 21)
    assert (bits(g.read_logits()) == bits(want)).all()
    o.close()


def test_decode_across_256_keys(oracle, files, models):
    g, o = models("tiny", "q4_0"), simd_oracle(oracle, files[("tiny", "q4_0")])
    toks = seq_of("tiny", 302, 6)
    for at in range(0, 296, 8):
        g.eval_device(toks[at:at + 8], at); o.eval(toks[at:at + 8], at)
    assert (bits(g.eval(toks[296:300], 296)) == bits(o.eval(toks[296:300], 296))).all()
    for i in (300, 301):
        assert (bits(g.eval([toks[i]], i)) == bits(o.eval([toks[i]], i))).all()
    got = kv_rows(g, TINY, 302)
    for w in (0, 1):
        assert (bits(got[w]) == bits(o.kv(w)[:, :302, :])).all()
    o.close()


@pytest.mark.parametrize("fam,name", [("tiny", "q5_1"), ("base", "q4_0")], ids=["tiny-q5_1", "base-q4_0"])
def test_the_switch_changes_the_logits_and_mode_0_is_restored(pkg, files, fam, name):
    toks = seq_of(fam, 12, 7)
    def run(m):
        rows = [m.eval(toks[:8], 0)] + [m.eval([toks[i]], i) for i in range(8, 12)]
        ids, _ = m.generate_greedy(toks[:6], 6)
        return np.stack(rows), list(ids)
    fresh = pkg.BiogptModel.load(files[(fam, name)])      # a context that never switches
    assert fresh.assoc == "scalar"
    want_rows, want_ids = run(fresh)
    fresh.close()
    g = pkg.BiogptModel.load(files[(fam, name)])
    state0 = (g.xpipe_state(), g.chain_kind())
    rows0, ids0 = run(g)
    assert (bits(rows0) == bits(want_rows)).all() and ids0 == want_ids
    g.set_assoc("simd")
    assert g.assoc == "simd" and g.chain_kind() == 0
    rows1, _ = run(g)
    delta = float(np.abs(rows1.astype(np.float64) - rows0.astype(np.float64)).max())
    print("%s %s: max |logit(mode 1) - logit(mode 0)| = %.3e" % (fam, name, delta))
    assert delta > 0.0, "the switch is a no-op"
    g.set_assoc("scalar")
    assert g.assoc == "scalar" and (g.xpipe_state(), g.chain_kind()) == state0
    rows2, ids2 = run(g)
    assert (bits(rows2) == bits(want_rows)).all() and ids2 == want_ids
    g.close()


def test_two_contexts_in_different_modes(pkg, oracle, files):
    path = files[("tiny", "q4_0")]
    a, b = pkg.BiogptModel.load(path), pkg.BiogptModel.load(path, assoc="simd")
    oa, ob = oracle.OracleModel(path, n_threads=4), simd_oracle(oracle, path)
    toks = seq_of("tiny", 14, 8)
    assert (bits(a.eval(toks[:8], 0)) == bits(oa.eval(toks[:8], 0))).all()
    assert (bits(b.eval(toks[:8], 0)) == bits(ob.eval(toks[:8], 0))).all()
    for i in range(8, 14):      # interleaved
        ra, rb = a.eval([toks[i]], i), b.eval([toks[i]], i)
        assert (bits(ra) == bits(oa.eval([toks[i]], i))).all() and (bits(rb) == bits(ob.eval([toks[i]], i))).all(), i
    for m in (a, b):
        m.close()
    oa.close(); ob.close()


def test_column_calls_are_refused_by_name(models):
    g = models("tiny", "q4_0")
    p = [seq_of("tiny", 5, 9), seq_of("tiny", 6, 10)]
    calls = [lambda: g.generate_greedy_batch(p, 4), lambda: g.score_batch(p), lambda: g.embed_batch(p), lambda: g.generate_sample(p, 4),
             lambda: g.generate_beam(p[0], 4, n_beams=2), lambda: g.score_continuations(p[0], [p[1]]), lambda: g.queue_session(max_columns=2)]
    for call in calls:
        with pytest.raises(Exception, match="association"):
            call()
    assert (g.eval(p[0], 0) == g.eval(p[0], 0)).all()      # and the context goes on serving


def test_float_files_and_open_sessions_refuse_the_switch(pkg, files):
    f = pkg.BiogptModel.load(files[("tiny", "f32")])
    with pytest.raises(pkg.BiogptError, match="F32"):
        f.set_assoc("simd")
    assert f.assoc == "scalar"
    with pytest.raises(pkg.BiogptError, match="F32"):
        pkg.BiogptModel.load(files[("tiny", "f32")], assoc="simd")
    f.close()
    g = pkg.BiogptModel.load(files[("base", "q4_0")])      # (a queue session is the BioGPT-base chain's)
    with g.queue_session(max_columns=2, group=2, n_predict=4):
        with pytest.raises(pkg.BiogptError, match="queue session is open"):
            g.set_assoc("simd")
    g.set_assoc("simd")
    assert g.assoc == "simd"
    g.close()


def test_environment_default(pkg, files, monkeypatch):
    monkeypatch.setenv("BIOGPT_HIP_ASSOC", "1")
    g, f = pkg.BiogptModel.load(files[("tiny", "q8_0")]), pkg.BiogptModel.load(files[("tiny", "f32")])
    assert g.assoc == "simd" and f.assoc == "scalar"      # (the default holds where the file can have the mode)
    g.close(); f.close()
