"""Contrastive search (biogpt_hip_generate_contrastive, kernels_contrast.hip.h) on the GPU: the penalty and selection kernels alone against
contrast_ref (the restatement test_contrast_restatement.py checks on the CPU); the search against contrast_ref driven by the oracle's taps;
one candidate or no penalty is greedy decoding; a prompt's result does not depend on the rest of the call; past the 256-key bucket the
scores are reproduced from the engine's own rows; the captured, eager and column-per-XCD paths agree; the context and the other modes
are left alone.

The bound.  ULP = 2^-23, the spacing of f32 at 1.0.  p and sim lie in [-1, 1] and each is rounded once from double, the score is rounded once:
SCORE_TOL = 4 ULP = 4.8e-7 on pen and on score.  It is the one bound of this file: the kernels alone, the search against the restatement
driven by the oracle's taps (the oracle's rows are the engine's bit for bit at these shapes -- smoke() and test_gpu_parity.py report it -- so no
row term is added), and the scores reproduced from the engine's own rows.  In the model-driven cases the restatement forms the exponential sum S
of a logits row from the same f32 terms as lp_row_stats but adds them in double where the kernel adds up to 170 per lane in f32 first; that
difference is NOT given room here: a score that leaves the 4 ULP because of it fails, and the figures are printed.
Selections are compared where the restatement's margin exceeds MARGIN = 1e-5, and every case first asserts that ALL of its margins do."""
import numpy as np
import pytest

import contrast_ref

pytestmark = pytest.mark.gpu

KW = dict(n_vocab=42384, n_layer=3, n_head=16, n_positions=1024, d_ff=4096, d_model=1024, n_merges=40000)
SEED = 0x42494F47
MARGIN = 1e-5
ULP = 2.0 ** -23
SCORE_TOL = 4 * ULP
D = KW["d_model"]
FIXTURE = "fixture problem: selection margins below %g at steps %s -- the case cannot tell the engine's rounding from a wrong choice"


def prompt_of(n, seed):
    rng = np.random.default_rng(seed)
    return [2] + [int(v) for v in rng.integers(4, KW["n_vocab"], n - 1)]


@pytest.fixture(scope="module")
def files(pkg, tmp_path_factory):
    d = tmp_path_factory.mktemp("contrast")
    f32 = str(d / "f32.bin")
    pkg.write_synthetic(f32, **KW)
    out = {"f32": f32}
    for name in ("q4_0", "q5_1", "q8_0"):
        out[name] = str(d / (name + ".bin"))
        pkg.quantize_file(f32, out[name], name)
    return out


@pytest.fixture(scope="module")
def base24(pkg, tmp_path_factory):
    d = tmp_path_factory.mktemp("contrast24")
    f32, path = str(d / "f32.bin"), str(d / "q4_0.bin")
    pkg.write_synthetic(f32, seed=SEED, **dict(KW, n_layer=24))     # the seed of the bench
    pkg.quantize_file(f32, path, "q4_0")
    return path


# ---- 1. the kernels alone ----

def plant_row(T, where):
    """first row of the last slab / last row of the first slab (of the context, if that is shorter) / last row overall"""
    return {"slab_first": (T - 1) // 64 * 64, "slab_last": min(T, 64) - 1, "last": T - 1}[where]


@pytest.fixture(scope="module")
def kernel_rows():
    rng = np.random.default_rng(2022)
    return rng.standard_normal((1023, D)).astype(np.float32), rng.standard_normal((16, D)).astype(np.float32), rng.standard_normal(D).astype(np.float32)


@pytest.mark.parametrize("where", ["slab_first", "slab_last", "last"])
@pytest.mark.parametrize("k", [1, 2, 5, 16])
@pytest.mark.parametrize("T", [1, 63, 64, 65, 130, 1023])
def test_rank_kernels_against_restatement(pkg, kernel_rows, T, k, where):
    all_ctx, all_cand, noise = kernel_rows
    ctx, cand = all_ctx[:T].copy(), all_cand[:k].copy()
    t, j = plant_row(T, where), k - 1
    cand[j] = (2.0 * ctx[t] + 0.25 * noise).astype(np.float32)      # sim about 0.99 with row t alone, about 0.03 with the others
    probs = ((np.arange(k, dtype=np.float32) * 7 % k + 1) / np.float32(4 * k)).astype(np.float32)      # distinct, spaced by 1 / (4 k)
    alpha = 0.6
    pen_w, sc_w, win_w, margin = contrast_ref.rank(cand, ctx, probs, alpha)
    assert margin > MARGIN, FIXTURE % (MARGIN, [(1, margin)])
    assert pen_w[j] > 0.9
    pen, sc, win = pkg.contrast_rank(cand, ctx, probs, alpha)
    e_pen, e_sc = float(np.abs(pen.astype(np.float64) - pen_w).max()), float(np.abs(sc.astype(np.float64) - sc_w).max())
    print("T=%d k=%d %s: max |pen diff| %.3g, max |score diff| %.3g, winner %d (margin %.3g)" % (T, k, where, e_pen, e_sc, win, margin))
    assert e_pen <= SCORE_TOL and e_sc <= SCORE_TOL
    assert win == win_w


def test_rank_kernels_ties_and_zero_rows(pkg):
    ctx = np.zeros((70, D), dtype=np.float32)
    ctx[3, 5] = 1.0
    ctx[69, 9] = -2.0
    cand = np.zeros((4, D), dtype=np.float32)
    cand[0, 5] = 3.0          # the direction of row 3: exactly 1
    cand[1, 9] = 1.0          # against row 69: -1, against the zero rows: 0
    cand[3, 100] = 1.0        # orthogonal to everything: 0; candidate 2 is a zero row: 0
    pen, sc, win = pkg.contrast_rank(cand, ctx, [0.25, 0.25, 0.25, 0.25], 0.5)
    assert pen.tolist() == [1.0, 0.0, 0.0, 0.0]
    assert sc[1] == sc[2] == sc[3] == np.float32(0.125) and win == 1      # the lowest j of the tie


# ---- 2. the restatement, driven by the oracle's taps ----

ORACLE_PROMPT = prompt_of(13, 3)
N_PREDICT = 10


def oracle_tap(o, tokens, n_past):
    lg = o.eval(tokens, n_past)
    return o.tap(o.n_layer), lg


@pytest.fixture(scope="module")
def oracle_rows(oracle, files):
    cache = {}

    def get(name, nb):
        if (name, nb) not in cache:
            cache[(name, nb)] = contrast_ref.OracleRows(oracle.OracleModel(files[name], n_threads=16), ORACLE_PROMPT, nb, oracle_tap)
        return cache[(name, nb)]
    return get


@pytest.mark.parametrize("nb", [1, 8])
@pytest.mark.parametrize("alpha", [0.4, 0.6])
@pytest.mark.parametrize("k", [2, 4, 8])
@pytest.mark.parametrize("name", ["q4_0", "q5_1", "q8_0"])
def test_contrastive_against_restatement(pkg, files, oracle_rows, name, k, alpha, nb):
    rows = oracle_rows(name, nb)
    free, free_sc, margins = contrast_ref.search(rows, rows.prompt_hidden, N_PREDICT, k, alpha)
    eos = free[4]      # fires mid-run: at its first occurrence, the fifth token at the latest
    want, want_sc, m2 = contrast_ref.search(rows, rows.prompt_hidden, N_PREDICT, k, alpha, eos_id=eos)
    small = [(i + 1, m) for i, m in enumerate(margins) if m < MARGIN]
    assert not small, FIXTURE % (MARGIN, small)
    assert len(free) == N_PREDICT and 1 <= len(want) < N_PREDICT and want[-1] == eos
    tol = SCORE_TOL
    g = pkg.BiogptModel.load(files[name])
    worst = 0.0
    for eos_id, ids_w, sc_w in ((-1, free, free_sc), (eos, want, want_sc)):
        ids, sc = g.generate_contrastive([ORACLE_PROMPT], N_PREDICT, top_k=k, penalty_alpha=alpha, eos_id=eos_id, n_batch=nb)
        assert list(ids[0]) == list(ids_w), (eos_id, list(ids[0]), list(ids_w))
        diff = float(np.abs(sc[0].astype(np.float64) - sc_w).max())
        worst = max(worst, diff)
        assert diff <= tol, (eos_id, diff, tol)
    g.close()
    print("%s k=%d alpha=%g n_batch=%d eos=%d: smallest margin %.3g, max |score diff| %.3g (bound %.3g), EOS run %d tokens"
          % (name, k, alpha, nb, eos, min(margins), worst, tol, len(want)))


# ---- 3. one candidate, or no penalty: greedy decoding ----

def check_is_greedy(pkg, path, prompts, n_predict):
    g = pkg.BiogptModel.load(path)
    for nb in (1, 8):
        want, _ = g.generate_greedy_batch(prompts, n_predict, n_batch=nb)
        for k, alpha in ((1, 0.6), (4, 0.0), (1, 0.0)):
            ids, sc = g.generate_contrastive(prompts, n_predict, top_k=k, penalty_alpha=alpha, n_batch=nb)
            for p in range(len(prompts)):
                assert list(ids[p]) == [int(t) for t in want[p]], (nb, k, alpha, p)
                assert len(sc[p]) == n_predict
    g.close()


def test_one_candidate_or_no_penalty_is_greedy_3_layers(pkg, files):
    check_is_greedy(pkg, files["q4_0"], [prompt_of(21, 1), prompt_of(6, 11)], 24)


def test_one_candidate_or_no_penalty_is_greedy_24_layers(pkg, base24):
    check_is_greedy(pkg, base24, [prompt_of(40, 2)], 32)


# ---- 4. a prompt's result does not depend on what else is in the call ----

def test_batch_independence(pkg, files):
    prompts = [prompt_of(5, 21), prompt_of(13, 22), prompt_of(40, 23)]
    g = pkg.BiogptModel.load(files["q4_0"])
    ids, sc = g.generate_contrastive(prompts, 20, top_k=4, penalty_alpha=0.6, n_batch=8)
    for p, pr in enumerate(prompts):
        one_i, one_s = g.generate_contrastive([pr], 20, top_k=4, penalty_alpha=0.6, n_batch=8)
        assert list(ids[p]) == list(one_i[0]), p
        assert sc[p].tobytes() == one_s[0].tobytes(), p
    assert len({tuple(i) for i in ids}) == 3
    g.close()


def test_many_columns_equal_single_calls(pkg, files):
    """64 and 65 columns: the decode step on the matrix cores and the slim attention kernel (from 48 columns), the rank grid over 16 / 13 groups."""
    many = [prompt_of(n, 50 + i) for i, n in enumerate((40, 25, 7, 9, 33, 40, 17, 5, 40, 12, 21, 40, 28, 13, 6, 31))]
    g = pkg.BiogptModel.load(files["q4_0"])
    for G, k in ((16, 4), (13, 5)):
        eos = int(g.generate_contrastive([many[0]], 12, top_k=k, penalty_alpha=0.6)[0][0][5])      # ends prompt 0 mid-run, the others go on (or end elsewhere)
        ids, sc = g.generate_contrastive(many[:G], 12, top_k=k, penalty_alpha=0.6, eos_id=eos, n_batch=8)
        assert len(ids[0]) < 12 and max(len(i) for i in ids) == 12
        for p in range(G):
            one_i, one_s = g.generate_contrastive([many[p]], 12, top_k=k, penalty_alpha=0.6, eos_id=eos, n_batch=8)
            assert list(ids[p]) == list(one_i[0]), (G, k, p)
            assert sc[p].tobytes() == one_s[0].tobytes(), (G, k, p)
    g.close()


# ---- 5. the scores from the engine's own rows: one-column groups, and past the 256-key bucket ----

def check_scores_from_engine_rows(pkg, path, prompt, n, k, alpha, what):
    g = pkg.BiogptModel.load(path)
    ids, sc = g.generate_contrastive([prompt], n, top_k=k, penalty_alpha=alpha, n_batch=1)      # (n_batch 1: the prompt rows are hidden()'s causal rows)
    h = pkg.BiogptModel.load(path)
    cache = {}

    def rows(prefixes):
        for p in prefixes:
            if tuple(p) not in cache:
                toks = list(prompt) + list(p)
                hid = h.hidden(toks)
                cache[tuple(p)] = (hid, h.eval([toks[-1]], len(toks) - 1))
        return np.stack([cache[tuple(p)][0][-1] for p in prefixes]), np.stack([cache[tuple(p)][1] for p in prefixes])

    rows([[]])
    want, want_sc, margins = contrast_ref.search(rows, cache[()][0][:-1], n, k, alpha)
    g.close()
    h.close()
    small = [(i + 1, m) for i, m in enumerate(margins) if m < MARGIN]
    assert not small, FIXTURE % (MARGIN, small)
    diff = float(np.abs(sc[0].astype(np.float64) - want_sc).max())
    print("%s: max |score diff| %.3g (bound %.3g), %d/%d scores bit-identical, smallest margin %.3g"
          % (what, diff, SCORE_TOL, int((sc[0] == want_sc).sum()), n, min(margins)))
    assert list(ids[0]) == want
    assert diff <= SCORE_TOL
    return want_sc


def test_one_candidate_scores_carry_the_penalty(pkg, files):
    """top_k = 1: the id is the arg-max whatever the penalty, the score (1 - alpha) p - alpha pen still needs the hidden epilogue and the rank kernel of a one-column group."""
    want_sc = check_scores_from_engine_rows(pkg, files["q4_0"], prompt_of(70, 12), 10, 1, 0.6, "top_k 1, 70-token prompt + 10")
    assert (want_sc < 0).any()      # (a penalty that counts: p alone cannot make a score negative)


def test_scores_are_reproduced_from_the_engines_rows_past_256_keys(pkg, base24):
    check_scores_from_engine_rows(pkg, base24, prompt_of(250, 5), 12, 4, 0.6, "250-token prompt + 12")


# ---- 6. the paths agree ----

def test_paths_agree(pkg, files, monkeypatch):
    prompts = [prompt_of(30, 6)]
    g = pkg.BiogptModel.load(files["q4_0"])
    runs = {}
    for label, env in (("default", {}), ("repeat", {}), ("xcols off", {"BIOGPT_HIP_XCOLS": "0"}), ("no graph", {"BIOGPT_HIP_NO_GRAPH": "1"})):
        for key in ("BIOGPT_HIP_XCOLS", "BIOGPT_HIP_NO_GRAPH"):
            monkeypatch.delenv(key, raising=False)
        for key, v in env.items():
            monkeypatch.setenv(key, v)
        g.refresh_options()
        for k in (2, 5, 12):      # 2 and 5 columns: column-per-XCD launches by default; 12: the launch chain
            ids, sc = g.generate_contrastive(prompts, 40, top_k=k, penalty_alpha=0.6, n_batch=8)
            runs.setdefault(k, []).append((label, list(ids[0]), sc[0].tobytes()))
    g.close()
    for k, rs in runs.items():
        for label, ids, sc in rs[1:]:
            assert ids == rs[0][1] and sc == rs[0][2], (k, label)


# ---- 7. the context and the other modes are left alone; arguments ----

def test_context_cache_untouched_and_eval_follows(pkg, files):
    g = pkg.BiogptModel.load(files["q4_0"])
    h = pkg.BiogptModel.load(files["q4_0"])
    ctx_toks = prompt_of(9, 7)
    g.eval(ctx_toks, 0)
    h.eval(ctx_toks, 0)
    k0, v0 = g.read_kv(0, 0, 3 * KW["n_positions"] * D), g.read_kv(1, 0, 3 * KW["n_positions"] * D)
    ids, _ = g.generate_contrastive([prompt_of(17, 8)], 12, top_k=4, penalty_alpha=0.6, n_batch=8)
    assert len(ids[0]) == 12
    assert np.array_equal(g.read_kv(0, 0, k0.size), k0) and np.array_equal(g.read_kv(1, 0, v0.size), v0)
    nxt = [123]
    assert np.array_equal(g.eval(nxt, len(ctx_toks)), h.eval(nxt, len(ctx_toks)))
    g.close()
    h.close()


def test_existing_modes_are_unchanged_by_a_contrastive_call(pkg, files):
    prompts = [prompt_of(11, 31), prompt_of(19, 32)]
    g = pkg.BiogptModel.load(files["q4_0"])
    greedy0, _ = g.generate_greedy_batch(prompts, 16)
    sample0, _ = g.generate_sample(prompts, 16, n_samples=2, top_k=40, top_p=0.9, temp=0.9, seed=5)
    g.generate_contrastive(prompts, 16, top_k=4, penalty_alpha=0.6)
    greedy1, _ = g.generate_greedy_batch(prompts, 16)
    sample1, _ = g.generate_sample(prompts, 16, n_samples=2, top_k=40, top_p=0.9, temp=0.9, seed=5)
    assert np.array_equal(np.asarray(greedy0), np.asarray(greedy1))
    assert [list(s) for s in sample0] == [list(s) for s in sample1]
    g.close()


def test_float_files_and_bad_arguments_fail(pkg, files, tiny_models):
    for path in (files["f32"], tiny_models["f16"], tiny_models["q4_0"]):
        g = pkg.BiogptModel.load(path)
        with pytest.raises(pkg.BiogptError, match="fast chain"):
            g.generate_contrastive([[2, 5, 7]], 4, top_k=2)
        g.close()
    g = pkg.BiogptModel.load(files["q4_0"])
    for kw, msg in ((dict(top_k=0), "top_k"), (dict(top_k=17), "top_k"), (dict(n_batch=0), "n_batch"), (dict(penalty_alpha=1.5), "penalty_alpha"),
                    (dict(eos_id=KW["n_vocab"]), "eos_id"), (dict(eos_id=-2), "eos_id")):
        with pytest.raises(pkg.BiogptError, match=msg):
            g.generate_contrastive([[2, 5, 7]], 4, **kw)
    with pytest.raises(pkg.BiogptError):
        g.generate_contrastive([[2, 5, KW["n_vocab"]]], 4)
    with pytest.raises(pkg.BiogptError, match="empty prompt"):
        g.generate_contrastive([[2, 5], []], 4)
    assert [len(i) for i in g.generate_contrastive([[2] * KW["n_positions"]], 4)[0]] == [0]
    ids, sc = g.generate_contrastive([[2, 5, 7]], 4, top_k=3)      # still usable
    assert len(ids[0]) == 4 and len(sc[0]) == 4
    g.close()
