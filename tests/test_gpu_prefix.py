"""Shared-prefix scoring (biogpt_hip_score_continuations): many continuations of one prefix, the prefix evaluated once and read in place by
every continuation's attention (attn_fast_kernel<.., SHARED>).  Checked bit for bit against score_batch of each concatenation (the route the
call replaces), against the causal oracle with the bounds of test_gpu_score.py, at the limits, for its argument errors and for what it must
leave alone."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KW = dict(n_vocab=42384, n_layer=3, n_head=16, n_positions=1024, d_ff=4096, d_model=1024, n_merges=40000)
LENS = [1, 2, 7, 40]


def log_softmax64(rows):
    r = np.asarray(rows, dtype=np.float64)
    m = r.max(axis=-1, keepdims=True)
    return r - m - np.log(np.exp(r - m).sum(axis=-1, keepdims=True))


@pytest.fixture(scope="module")
def files(pkg, tmp_path_factory):
    d = tmp_path_factory.mktemp("prefix_full")
    f32 = str(d / "f32.bin")
    pkg.write_synthetic(f32, **KW)
    out = {"f32": f32}
    for name in ("q4_0", "q5_1", "q8_0", "q4_1", "q5_0"):
        out[name] = str(d / (name + ".bin"))
        pkg.quantize_file(f32, out[name], name)
    return out


def make_case(seed, n_prefix, n_conts, lens=LENS):
    rng = np.random.default_rng(seed)
    prefix = [2] + [int(v) for v in rng.integers(4, KW["n_vocab"], n_prefix - 1)]
    conts = [[int(v) for v in rng.integers(4, KW["n_vocab"], lens[(c + seed) % len(lens)])] for c in range(n_conts)]
    return prefix, conts


# ---- 1. bit for bit against score_batch of the concatenation ----

@pytest.mark.parametrize("n_conts", [1, 3, 47, 48, 100])
@pytest.mark.parametrize("n_prefix", [1, 2, 64, 65, 257, 600])
@pytest.mark.parametrize("cols", [64, 512])
@pytest.mark.parametrize("name", ["q4_0", "q5_1"])
def test_continuations_equal_score_batch_rows(pkg, files, monkeypatch, name, cols, n_prefix, n_conts):
    """(logprob, argmax, logit) of every continuation == rows [n_prefix - 1, n_prefix - 1 + len) of score_batch([prefix + cont]) with the
    continuation's tokens as the targets of those rows.  cols: pass borders inside the prefix and inside a continuation; n_prefix: no shared
    rows at all (1), every t_cap class of the attention kernels; n_conts: both sides of the slim-kernel (48 columns) and matrix-core (64)
    cross-overs."""
    monkeypatch.setenv("BIOGPT_HIP_PROMPT_COLS", str(cols))
    g = pkg.BiogptModel.load(files[name])
    prefix, conts = make_case(n_prefix + n_conts, n_prefix, n_conts)
    got = g.score_continuations(prefix, conts)
    assert len(got) == n_conts
    bad = []
    for c, cont in enumerate(conts):
        n = len(cont)
        tg = [-1] * (n_prefix - 1) + list(cont) + [-1]
        lp, am, lg = g.score_batch([prefix + cont], [tg])[0]
        rows = slice(n_prefix - 1, n_prefix - 1 + n)
        for what, x, y in zip(("logprob", "argmax", "logit"), got[c], (lp[rows], am[rows], lg[rows])):
            assert x.shape == (n,)
            if not (x == y).all():
                bad.append((c, n, what, x[x != y][:4], y[x != y][:4]))
    assert not bad, (name, cols, n_prefix, n_conts, len(bad), bad[:6])
    g.close()


@pytest.mark.parametrize("n_prefix", [2, 300])
@pytest.mark.parametrize("name", ["q4_0", "q5_1"])
def test_slim_kernel_cross_over_in_one_pass(pkg, files, name, n_prefix):
    """47 and 48 single-token continuations: ONE scoring pass of exactly 47 columns (the per-t_cap instantiation) and of exactly 48 (the slim
    one), the same 47 continuations in both.  Both equal score_batch of the concatenations, hence each other."""
    g = pkg.BiogptModel.load(files[name])
    prefix, conts = make_case(48, n_prefix, 48, lens=[1])
    a = g.score_continuations(prefix, conts[:47])
    b = g.score_continuations(prefix, conts)
    tg = [-1] * (n_prefix - 1) + [0]
    for c, cont in enumerate(conts):
        tg[-1] = cont[0]
        lp, am, lg = g.score_batch([prefix], [tg])[0]
        for k, y in enumerate((lp[-1:], am[-1:], lg[-1:])):
            assert (b[c][k] == y).all(), (name, n_prefix, c, k)
            if c < 47:
                assert (a[c][k] == y).all(), (name, n_prefix, c, k)
    g.close()


# ---- 2. against the causal oracle, the bounds of test_gpu_score.check_against_oracle ----

def check_against_oracle(what, pkg, oracle, path, n_prefix, n_conts, seed, n_threads=16):
    """logits within 1e-3 of the causal oracle's rows, arg-max equal, log-probabilities within 2e-3 of the float64 log-softmax of the oracle's rows."""
    prefix, conts = make_case(seed, n_prefix, n_conts)
    g = pkg.BiogptModel.load(path)
    got = g.score_continuations(prefix, conts)
    g.close()
    o = oracle.OracleModel(path, n_threads=n_threads)
    o.set_mode("ggml", n_threads=n_threads, causal=1)
    first = np.asarray(o.eval(prefix, 0, all_rows=True))[-1:]            # the row of the last prefix token: every continuation's row 0
    d_lg = d_lp = 0.0
    for c, cont in enumerate(conts):
        # the oracle's cache holds the prefix rows; the continuation's columns but the last overwrite the rows behind them
        rest = np.asarray(o.eval(cont[:-1], n_prefix, all_rows=True)).reshape(len(cont) - 1, -1) if len(cont) > 1 else np.zeros((0, first.shape[1]))
        ref = np.concatenate([first, rest])
        idx = np.arange(len(cont))
        lp, am, lg = got[c]
        d_lg = max(d_lg, float(np.abs(lg - ref[idx, cont]).max()))
        d_lp = max(d_lp, float(np.abs(lp.astype(np.float64) - log_softmax64(ref)[idx, cont]).max()))
        assert (am == ref.argmax(axis=1)).all(), (what, c)
    print("%s: %d continuations behind %d tokens, target logits max |diff| %.2e, logprob max |diff| %.2e" % (what, n_conts, n_prefix, d_lg, d_lp))
    assert d_lg <= 1e-3, what
    assert d_lp <= 2e-3, what


@pytest.mark.parametrize("name,n_prefix,n_conts", [("q4_0", 300, 5), ("q4_1", 65, 4), ("q5_0", 2, 6), ("q5_1", 130, 50), ("q8_0", 520, 4)])
def test_continuations_against_causal_oracle(pkg, oracle, files, name, n_prefix, n_conts):
    check_against_oracle("full shape %s" % name, pkg, oracle, files[name], n_prefix, n_conts, 11)


def test_continuations_24_layers_q4_0(pkg, oracle, tmp_path):
    f32, path = str(tmp_path / "f32.bin"), str(tmp_path / "q4_0.bin")
    pkg.write_synthetic(f32, seed=0x42494F47, **dict(KW, n_layer=24))     # the seed of the base24_f32 fixture and the bench
    pkg.quantize_file(f32, path, "q4_0")
    check_against_oracle("24 layers q4_0", pkg, oracle, path, 200, 4, 24)


# ---- 3. limits ----

def test_continuations_reach_n_positions(pkg, files):
    g = pkg.BiogptModel.load(files["q4_0"])
    prefix, conts = make_case(5, 1000, 3, lens=[24, 3, 24])
    got = g.score_continuations(prefix, conts)                             # n_prefix + len == n_positions
    tg = [-1] * 999 + conts[0] + [-1]
    ref = g.score_batch([prefix + conts[0]], [tg])[0]
    for x, y in zip(got[0], ref):
        assert (x == y[999:1023]).all()
    with pytest.raises(pkg.BiogptError, match="n_positions"):
        g.score_continuations(prefix, [conts[1], conts[0] + [5]])           # one token more
    with pytest.raises(pkg.BiogptError, match="n_positions"):
        g.score_continuations(prefix + [7] * 24, [[5]])                    # the prefix alone fills the table
    lp, _, _ = g.score_continuations(prefix + [7] * 23, [[5]])[0]
    assert np.isfinite(lp).all()
    g.close()


@pytest.mark.parametrize("which", ["tiny_f16", "full_f32"])
def test_continuations_reject_float_files(pkg, tiny_models, files, which):
    g = pkg.BiogptModel.load(tiny_models["f16"] if which == "tiny_f16" else files["f32"])
    with pytest.raises(pkg.BiogptError, match="fast chain"):
        g.score_continuations([2, 5, 9], [[7], [11, 4]])
    lp, _, _ = g.score([2, 5, 9])                                          # single-sequence scoring works for every file type
    assert np.isfinite(lp).all()
    g.close()


def test_continuations_argument_errors(pkg, files):
    g = pkg.BiogptModel.load(files["q4_0"])
    V = KW["n_vocab"]
    good = g.score_continuations([2, 5, 9], [[7], [11, 4]])
    for field, prefix, conts in [
        ("n_prefix", [], [[7]]),
        ("n_conts", [2, 5], []),
        ("n_conts", [2, 5], [[7]] * 512),
        ("empty continuation (continuation 1)", [2, 5], [[7], [], [9]]),
        ("token id", [2, V], [[7]]),
        ("token id -3", [2, 5], [[7], [9, -3]]),
        ("token id", [2, 5], [[7, V + 1]]),
        ("cont_lens[1]", [2] * 1000, [[7], [9] * 25]),
        ("n_positions", [2] * 1025, [[7]]),
    ]:
        with pytest.raises(pkg.BiogptError, match=field.replace("(", r"\(").replace(")", r"\)").replace("[", r"\[").replace("]", r"\]")):
            g.score_continuations(prefix, conts)
    # null pointers: only the C-ABI can pass them
    pre = np.array([2, 5, 9], dtype=np.int32)
    flat = np.array([7, 11, 4], dtype=np.int32)
    lens = np.array([1, 2], dtype=np.int32)
    out = np.zeros(3, dtype=np.float32)
    f = pkg.lib().biogpt_hip_score_continuations
    for field, args in [("prefix", (None, 3, flat.ctypes.data, lens.ctypes.data, 2, out.ctypes.data)),
                        ("conts", (pre.ctypes.data, 3, None, lens.ctypes.data, 2, out.ctypes.data)),
                        ("cont_lens", (pre.ctypes.data, 3, flat.ctypes.data, None, 2, out.ctypes.data)),
                        ("logprob_out", (pre.ctypes.data, 3, flat.ctypes.data, lens.ctypes.data, 2, None))]:
        assert f(g._h, *args, None, None, None) == -1
        assert "null argument: " + field in pkg._err(), pkg._err()
    # argmax_out / logit_out / seconds_out may be NULL
    assert f(g._h, pre.ctypes.data, 3, flat.ctypes.data, lens.ctypes.data, 2, out.ctypes.data, None, None, None) == 0
    assert (out == np.concatenate([t[0] for t in good])).all()
    again = g.score_continuations([2, 5, 9], [[7], [11, 4]])               # the context stays usable
    for a, b in zip(good, again):
        for x, y in zip(a, b):
            assert (x == y).all()
    g.close()


# ---- 4. isolation: what a call leaves alone ----

def test_continuations_leave_the_context_alone(pkg, files):
    g = pkg.BiogptModel.load(files["q4_0"])
    rng = np.random.default_rng(3)
    own = [2] + [int(v) for v in rng.integers(4, KW["n_vocab"], 47)]
    prompt = [2] + [int(v) for v in rng.integers(4, KW["n_vocab"], 11)]
    seqs = [[2] + [int(v) for v in rng.integers(4, KW["n_vocab"], n - 1)] for n in (5, 70, 33)]
    prefix, conts = make_case(8, 90, 20)

    def others():
        beams, _ = g.generate_beam(prompt, 6, n_beams=3)
        samples, _ = g.generate_sample([prompt, prompt[:5]], 6, n_samples=3, seed=17)
        return beams, samples, g.score_batch(seqs)

    before = others()
    g.eval_prompt(own, 0, 8)
    hp = g.hparams
    cnt = hp.n_layer * hp.n_positions * hp.d_model
    kv0 = [g.read_kv(w, 0, cnt) for w in (0, 1)]
    row0 = g.read_logits()
    first = g.score_continuations(prefix, conts)
    for w in (0, 1):
        assert (g.read_kv(w, 0, cnt) == kv0[w]).all(), "score_continuations wrote into the context's own K / V cache"
    assert (g.read_logits() == row0).all(), "score_continuations changed the context's logits row"
    nxt = g.eval([own[5]], len(own))                                       # the context's own sequence continues where it stood
    h = pkg.BiogptModel.load(files["q4_0"])
    h.eval_prompt(own, 0, 8)
    assert (nxt == h.eval([own[5]], len(own))).all()
    h.close()
    after = others()
    for (ia, sa), (ib, sb) in zip(before[0], after[0]):
        assert (ia == ib).all() and sa == sb
    assert len(before[1]) == len(after[1]) and all((a == b).all() for a, b in zip(before[1], after[1]))
    for a, b in zip(before[2], after[2]):
        for x, y in zip(a, b):
            assert (x == y).all()
    second = g.score_continuations(prefix, conts)                          # and the other calls leave nothing behind that changes this one
    for a, b in zip(first, second):
        for x, y in zip(a, b):
            assert (x == y).all()
    g.close()


# ---- 5. ranking ----

def test_rank_continuations_orders_by_float64_sums(pkg, files):
    g = pkg.BiogptModel.load(files["q5_1"])
    prefix, conts = make_case(21, 40, 12)
    rows = g.score_continuations(prefix, conts)
    for normalize in (False, True):
        order, sums = g.rank_continuations(prefix, conts, normalize=normalize)
        want = np.asarray([lp.astype(np.float64).sum() / (len(lp) if normalize else 1) for lp, _, _ in rows])
        assert sums.dtype == np.float64 and (sums == want).all()
        assert sorted(order.tolist()) == list(range(len(conts)))
        assert (order == np.argsort(-want, kind="stable")).all()
        assert (np.diff(sums[order]) <= 0).all()
    g.close()
