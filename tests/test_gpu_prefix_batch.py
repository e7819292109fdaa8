"""Shared-prefix scoring of many (prefix, continuations) groups in one call (biogpt_hip_score_continuations_batch): with BIOGPT_HIP_RUN_ATTN=0 every group is
score_continuations of that group, bit for bit; with =1 (attn_runs_kernel in every pass) a group's bits do not depend on its company, the order of the groups
or the pass size, and the numbers are the causal oracle's within the bounds of test_gpu_prefix.check_against_oracle; under the default the same bounds and the
columns and passes computed by hand.  Then the limits, every argument error, the float files, what the call leaves alone, and ranking."""
import numpy as np
import pytest

from test_gpu_prefix import KW, LENS, log_softmax64

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def files(pkg, tmp_path_factory):
    d = tmp_path_factory.mktemp("prefix_batch")
    f32 = str(d / "f32.bin")
    pkg.write_synthetic(f32, **KW)
    out = {"f32": f32}
    for name in ("q4_0", "q5_1"):
        out[name] = str(d / (name + ".bin"))
        pkg.quantize_file(f32, out[name], name)
    return out


def make_groups(seed, shapes):
    """shapes: [(n_prefix, n_conts)] -> (prefixes, continuations) with lengths cycling through LENS."""
    rng = np.random.default_rng(seed)
    prefixes, conts = [], []
    for g, (n_prefix, n_conts) in enumerate(shapes):
        prefixes.append([2] + [int(v) for v in rng.integers(4, KW["n_vocab"], n_prefix - 1)])
        conts.append([[int(v) for v in rng.integers(4, KW["n_vocab"], LENS[(c + g + seed) % len(LENS)])] for c in range(n_conts)])
    return prefixes, conts


MIXED = [(257, 3), (1, 9), (600, 1), (2, 3), (65, 9), (1, 1), (65, 1)]


def same(a, b):
    return len(a) == len(b) and all(len(x) == len(y) and all((p == q).all() and p.shape == q.shape for t, u in zip(x, y) for p, q in zip(t, u)) for x, y in zip(a, b))


def load(pkg, monkeypatch, path, run_attn=None, cols=None):
    if run_attn is None:
        monkeypatch.delenv("BIOGPT_HIP_RUN_ATTN", raising=False)
    else:
        monkeypatch.setenv("BIOGPT_HIP_RUN_ATTN", str(run_attn))
    if cols is not None:
        monkeypatch.setenv("BIOGPT_HIP_PROMPT_COLS", str(cols))
    return pkg.BiogptModel.load(path)


def expected_stats(prefixes, conts, cols):
    pre = sum(len(p) - 1 for p in prefixes)
    con = sum(len(c) for g in conts for c in g)
    return pre, con, -(-(pre + con) // cols)


# ---- 1. switch 0: the loop of score_continuations, bit for bit ----

@pytest.mark.parametrize("cols", [64, 512])
@pytest.mark.parametrize("name", ["q4_0", "q5_1"])
def test_switch_0_equals_the_loop_of_score_continuations(pkg, files, monkeypatch, name, cols):
    g = load(pkg, monkeypatch, files[name], 0, cols)
    prefixes, conts = make_groups(3, MIXED)
    got = g.score_continuations_batch(prefixes, conts)
    st = g.prefix_batch_stats()
    assert (st["prefix_columns"], st["continuation_columns"], st["passes"]) == expected_stats(prefixes, conts, cols) and st["run_passes"] == 0
    want = [g.score_continuations(p, c) for p, c in zip(prefixes, conts)]
    bad = [k for k, (a, b) in enumerate(zip(got, want)) if not same([a], [b])]
    assert not bad, (name, cols, bad)
    g.close()


# ---- 2. switch 1: a group's bits do not depend on its company ----

@pytest.mark.parametrize("name", ["q4_0", "q5_1"])
def test_switch_1_groups_do_not_depend_on_their_company(pkg, files, monkeypatch, name):
    prefixes, conts = make_groups(4, MIXED)
    g = load(pkg, monkeypatch, files[name], 1, 512)
    whole = g.score_continuations_batch(prefixes, conts)
    st = g.prefix_batch_stats()
    assert st["run_passes"] == st["passes"] == expected_stats(prefixes, conts, 512)[2]
    alone = [g.score_continuations_batch([p], [c])[0] for p, c in zip(prefixes, conts)]
    assert same(whole, alone), "a group alone differs from the group in company"
    rev = g.score_continuations_batch(prefixes[::-1], conts[::-1])[::-1]
    assert same(whole, rev), "the order of the groups changes a group's bits"
    g.close()
    h = load(pkg, monkeypatch, files[name], 1, 64)
    small = h.score_continuations_batch(prefixes, conts)
    st = h.prefix_batch_stats()
    assert st["run_passes"] == st["passes"] == expected_stats(prefixes, conts, 64)[2]
    h.close()
    assert same(whole, small), "the pass size changes a group's bits"


# ---- 3. against the causal oracle, the bounds of test_gpu_prefix.check_against_oracle ----

def check_against_oracle(what, pkg, oracle, g, path, prefixes, conts, n_threads=16):
    got = g.score_continuations_batch(prefixes, conts)
    o = oracle.OracleModel(path, n_threads=n_threads)
    o.set_mode("ggml", n_threads=n_threads, causal=1)
    d_lg = d_lp = 0.0
    for k, (prefix, cs) in enumerate(zip(prefixes, conts)):
        first = np.asarray(o.eval(prefix, 0, all_rows=True))[-1:]
        for c, cont in enumerate(cs):
            rest = np.asarray(o.eval(cont[:-1], len(prefix), all_rows=True)).reshape(len(cont) - 1, -1) if len(cont) > 1 else np.zeros((0, first.shape[1]))
            ref = np.concatenate([first, rest])
            idx = np.arange(len(cont))
            lp, am, lg = got[k][c]
            d_lg = max(d_lg, float(np.abs(lg - ref[idx, cont]).max()))
            d_lp = max(d_lp, float(np.abs(lp.astype(np.float64) - log_softmax64(ref)[idx, cont]).max()))
            assert (am == ref.argmax(axis=1)).all(), (what, k, c)
    print("%s: target logits max |diff| %.2e, logprob max |diff| %.2e" % (what, d_lg, d_lp))
    assert d_lg <= 1e-3, what
    assert d_lp <= 2e-3, what


@pytest.mark.parametrize("name", ["q4_0", "q5_1"])
def test_switch_1_against_the_causal_oracle(pkg, oracle, files, monkeypatch, name):
    prefixes, conts = make_groups(11, [(130, 5), (67, 4)])
    g = load(pkg, monkeypatch, files[name], 1, 512)
    check_against_oracle("switch 1 %s" % name, pkg, oracle, g, files[name], prefixes, conts)
    assert g.prefix_batch_stats()["run_passes"] == 1
    g.close()


def test_switch_1_24_layers_q4_0(pkg, oracle, tmp_path, monkeypatch):
    f32, path = str(tmp_path / "f32.bin"), str(tmp_path / "q4_0.bin")
    pkg.write_synthetic(f32, seed=0x42494F47, **dict(KW, n_layer=24))
    pkg.quantize_file(f32, path, "q4_0")
    prefixes, conts = make_groups(24, [(120, 3), (40, 2)])
    g = load(pkg, monkeypatch, path, 1, 512)
    check_against_oracle("switch 1, 24 layers q4_0", pkg, oracle, g, path, prefixes, conts)
    g.close()


@pytest.mark.parametrize("name", ["q4_0", "q5_1"])
def test_default_against_the_causal_oracle_with_the_stats_by_hand(pkg, oracle, files, monkeypatch, name):
    prefixes, conts = make_groups(12, [(90, 3), (45, 4)])
    g = load(pkg, monkeypatch, files[name], None, 64)
    check_against_oracle("default %s" % name, pkg, oracle, g, files[name], prefixes, conts)
    st = g.prefix_batch_stats()
    # 89 + 44 prefix columns; lengths LENS[(c + g + 12) % 4]: group 0 -> 1, 2, 7; group 1 -> 2, 7, 40, 1: 60 continuation columns; 193 columns in passes of 64
    assert (st["prefix_columns"], st["continuation_columns"], st["passes"]) == (133, 60, 4)
    assert st["run_passes"] == 0                                             # passes of 64 columns: below RUN_ATTN_MIN_COLS, the existing attention
    g.close()


def test_default_takes_the_run_kernel_in_a_full_pass(pkg, oracle, files, monkeypatch):
    prefixes, conts = make_groups(13, [(600, 2)])                             # lengths LENS[(c + 13) % 4]: 2, 7
    g = load(pkg, monkeypatch, files["q4_0"], None, 512)
    check_against_oracle("default, a full pass", pkg, oracle, g, files["q4_0"], prefixes, conts)
    # 599 prefix columns + 9: a pass of 512 columns (the run kernel), then one of 96 (below RUN_ATTN_MIN_COLS: the existing attention)
    assert g.prefix_batch_stats() == dict(prefix_columns=599, continuation_columns=9, passes=2, run_passes=1)
    g.close()


def test_the_single_call_never_takes_the_run_kernel(pkg, files, monkeypatch):
    """One group of 4 two-token continuations behind 300 tokens: one pass of 299 + 8 = 307 columns whose longest shared range has 299 rows, which the batch
    call gives to attn_runs_kernel by default.  score_continuations builds the same columns with the same packer and must not: its bits are the same under every
    BIOGPT_HIP_RUN_ATTN and are those of the batch call under =0; and it leaves the batch call's stats alone."""
    monkeypatch.delenv("BIOGPT_HIP_PROMPT_COLS", raising=False)
    rng = np.random.default_rng(21)
    prefix = [2] + [int(v) for v in rng.integers(4, KW["n_vocab"], 299)]
    conts = [[int(v) for v in rng.integers(4, KW["n_vocab"], 2)] for _ in range(4)]
    single = {}
    for switch in (None, 1, 0):
        g = load(pkg, monkeypatch, files["q4_0"], switch)
        single[switch] = g.score_continuations(prefix, conts)
        if switch == 0:
            batch_0 = g.score_continuations_batch([prefix], [conts])[0]
        g.close()
    assert same([single[None]], [single[1]]), "BIOGPT_HIP_RUN_ATTN=1 changes the bits of score_continuations"
    assert same([single[None]], [single[0]]), "BIOGPT_HIP_RUN_ATTN=0 changes the bits of score_continuations"
    assert same([single[0]], [batch_0]), "score_continuations differs from the batch call of its one group under BIOGPT_HIP_RUN_ATTN=0"
    g = load(pkg, monkeypatch, files["q4_0"], None)
    g.score_continuations_batch([prefix], [conts])
    st = g.prefix_batch_stats()
    assert st == dict(prefix_columns=299, continuation_columns=8, passes=1, run_passes=1)
    g.score_continuations(prefix[:40], conts[:2])
    assert g.prefix_batch_stats() == st, "a single call changed the stats of the last batch call"
    g.close()


# ---- 4. limits ----

def test_exactly_512_slots_run_and_513_are_refused(pkg, files, monkeypatch):
    g = load(pkg, monkeypatch, files["q4_0"], 0, 512)
    prefixes, conts = make_groups(5, [(3, 3)] * 128)                        # 128 * (1 + 3) = 512 slots
    for cs in conts:
        for c in cs:
            del c[1:]
    pre = np.concatenate([np.asarray(p, np.int32) for p in prefixes])
    plens = np.full(128, 3, np.int32)
    flat = np.asarray([c[0] for cs in conts for c in cs], np.int32)
    ncs = np.full(128, 3, np.int32)
    out = np.zeros(flat.size + 1, np.float32)
    f = pkg.lib().biogpt_hip_score_continuations_batch
    args = lambda clens, n_conts: (g._h, pre.ctypes.data, plens.ctypes.data, 128, flat.ctypes.data, clens.ctypes.data, n_conts.ctypes.data, out.ctypes.data, None, None, None)
    ones384, ones385 = np.ones(384, np.int32), np.ones(385, np.int32)
    assert f(*args(ones384, ncs)) == 0, pkg._err()
    assert g.prefix_batch_stats() == dict(prefix_columns=256, continuation_columns=384, passes=2, run_passes=0)
    want = g.score_continuations(prefixes[77], conts[77])
    assert (out[3 * 77:3 * 78] == np.concatenate([t[0] for t in want])).all()
    more = ncs.copy()
    more[127] = 4
    flat = np.append(flat, np.int32(9))
    assert f(*args(ones385, more)) == -1
    assert "513 slots" in pkg._err(), pkg._err()
    g.close()


def test_groups_reach_n_positions(pkg, files, monkeypatch):
    g = load(pkg, monkeypatch, files["q4_0"], 1, 512)
    prefixes, conts = make_groups(6, [(1000, 2), (5, 1)])
    conts[0] = [conts[0][0][:1] * 24, [7, 8, 9]]                              # n_prefix + len == n_positions
    got = g.score_continuations_batch(prefixes, conts)
    assert all(np.isfinite(lp).all() for grp in got for lp, _, _ in grp)
    with pytest.raises(pkg.BiogptError, match="n_positions"):
        g.score_continuations_batch(prefixes, [[conts[0][0] + [5], [7]], conts[1]])
    g.close()


# ---- 5. argument errors, float files ----

def test_argument_errors(pkg, files, monkeypatch):
    g = load(pkg, monkeypatch, files["q4_0"], None, 512)
    V = KW["n_vocab"]
    good = g.score_continuations_batch([[2, 5, 9], [2, 6]], [[[7], [11, 4]], [[8]]])
    esc = lambda s: s.replace("(", r"\(").replace(")", r"\)").replace("[", r"\[").replace("]", r"\]")
    for field, prefixes, conts in [
        ("prefix_lens[1]", [[2, 5], []], [[[7]], [[8]]]),
        ("n_conts[1]", [[2, 5], [2]], [[[7]], []]),
        ("empty continuation (group 1, continuation 2", [[2, 5], [2]], [[[7]], [[7], [8], []]]),
        ("token id %d (group 1, prefix, position 1)" % V, [[2, 5], [2, V]], [[[7]], [[8]]]),
        ("token id -3 (group 0, continuation 1, position 1)", [[2, 5], [2]], [[[7], [9, -3]], [[8]]]),
        ("token id %d (group 1, continuation 0, position 0)" % (V + 1), [[2, 5], [2]], [[[7]], [[V + 1]]]),
        ("of group 1, continuation 1 exceeds n_positions", [[2, 5], [2] * 1000], [[[7]], [[7], [9] * 25]]),
        ("exceeds n_positions", [[2, 5], [2] * 1025], [[[7]], [[7]]]),
    ]:
        with pytest.raises(pkg.BiogptError, match=esc(field)):
            g.score_continuations_batch(prefixes, conts)
    # what only the C-ABI can pass: null pointers, n_groups < 1
    pre = np.array([2, 5, 9], dtype=np.int32)
    plens = np.array([3], dtype=np.int32)
    flat = np.array([7, 11, 4], dtype=np.int32)
    lens = np.array([1, 2], dtype=np.int32)
    ncs = np.array([2], dtype=np.int32)
    out = np.zeros(3, dtype=np.float32)
    f = pkg.lib().biogpt_hip_score_continuations_batch
    ok = [pre.ctypes.data, plens.ctypes.data, 1, flat.ctypes.data, lens.ctypes.data, ncs.ctypes.data, out.ctypes.data]
    for at, field in ((0, "prefixes"), (1, "prefix_lens"), (3, "conts"), (4, "cont_lens"), (5, "n_conts"), (6, "logprob_out")):
        a = list(ok)
        a[at] = None
        assert f(g._h, *a, None, None, None) == -1
        assert "null argument: " + field in pkg._err(), pkg._err()
    for n in (0, -1):
        a = list(ok)
        a[2] = n
        assert f(g._h, *a, None, None, None) == -1 and "n_groups" in pkg._err()
    stats = np.zeros(4, dtype=np.int32)
    assert pkg.lib().biogpt_hip_prefix_batch_stats(g._h, None) == -1
    assert f(g._h, *ok, None, None, None) == 0                              # argmax_out / logit_out / seconds_out may be NULL
    assert (out == np.concatenate([t[0] for t in good[0]])).all()
    g.close()


@pytest.mark.parametrize("which", ["tiny_f16", "full_f32"])
def test_float_files_are_refused(pkg, tiny_models, files, which):
    g = pkg.BiogptModel.load(tiny_models["f16"] if which == "tiny_f16" else files["f32"])
    with pytest.raises(pkg.BiogptError, match="fast chain"):
        g.score_continuations_batch([[2, 5, 9]], [[[7], [11, 4]]])
    g.close()


# ---- 6. isolation, ranking ----

def test_the_call_leaves_the_context_alone(pkg, files, monkeypatch):
    g = load(pkg, monkeypatch, files["q4_0"], 1, 512)
    rng = np.random.default_rng(3)
    own = [2] + [int(v) for v in rng.integers(4, KW["n_vocab"], 47)]
    prefixes, conts = make_groups(8, [(90, 5), (30, 3)])
    g.eval_prompt(own, 0, 8)
    hp = g.hparams
    cnt = hp.n_layer * hp.n_positions * hp.d_model
    kv0 = [g.read_kv(w, 0, cnt) for w in (0, 1)]
    row0 = g.read_logits()
    first = g.score_continuations_batch(prefixes, conts)
    for w in (0, 1):
        assert (g.read_kv(w, 0, cnt) == kv0[w]).all(), "score_continuations_batch wrote into the context's own K / V cache"
    assert (g.read_logits() == row0).all(), "score_continuations_batch changed the context's logits row"
    nxt = g.eval([own[5]], len(own))                                       # the context's own sequence continues where it stood
    h = pkg.BiogptModel.load(files["q4_0"])
    h.eval_prompt(own, 0, 8)
    assert (nxt == h.eval([own[5]], len(own))).all()
    h.close()
    single = g.score_continuations(prefixes[0], conts[0])                  # another call over the same slots in between
    assert len(single) == 5
    assert same(first, g.score_continuations_batch(prefixes, conts))
    g.close()


def test_rank_continuations_batch_equals_the_per_group_ranking(pkg, files, monkeypatch):
    g = load(pkg, monkeypatch, files["q5_1"], 0, 512)
    prefixes, conts = make_groups(21, [(40, 12), (3, 2), (70, 5)])
    for normalize in (False, True):
        got = g.rank_continuations_batch(prefixes, conts, normalize=normalize)
        assert len(got) == 3
        for (order, sums), p, c in zip(got, prefixes, conts):
            o1, s1 = g.rank_continuations(p, c, normalize=normalize)
            assert sums.dtype == np.float64 and (sums == s1).all() and (order == o1).all()
    g.close()
