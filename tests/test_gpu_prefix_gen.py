"""Generation behind a shared prefix (generate_greedy_batch / generate_sample with prefix=): the prefix's shared rows are evaluated once and read in
place by every sequence's decode steps, or copied where the steps run as column-per-XCD launches.  Checked id for id against the same call on the
concatenations (the route it replaces), at the context buckets and the position table's end, across calls whose prefixes differ, for its argument
errors and for what it must leave alone."""
import numpy as np
import pytest

import prefix_gen_ref as ref

pytestmark = pytest.mark.gpu

KW = dict(n_vocab=42384, n_layer=3, n_head=16, n_positions=1024, d_ff=4096, d_model=1024, n_merges=40000)      # the files of test_gpu_prefix.py
LENS = [0, 1, 2, 7, 40]
N_PREDICT = 6


@pytest.fixture(scope="module")
def files(pkg, tmp_path_factory):
    d = tmp_path_factory.mktemp("prefix_gen")
    f32 = str(d / "f32.bin")
    pkg.write_synthetic(f32, **KW)
    out = {"f32": f32}
    for name in ("q4_0", "q5_1"):
        out[name] = str(d / (name + ".bin"))
        pkg.quantize_file(f32, out[name], name)
    return out


def make_case(seed, n_prefix, n_seqs, lens=LENS):
    rng = np.random.default_rng(seed)
    prefix = [2] + [int(v) for v in rng.integers(4, KW["n_vocab"], n_prefix - 1)]
    suffixes = [[int(v) for v in rng.integers(4, KW["n_vocab"], lens[s % len(lens)])] for s in range(n_seqs)]
    return prefix, suffixes


def check_greedy(g, prefix, suffixes, n_batch, path, n_predict=N_PREDICT):
    """ids == those of the call on the concatenations; the stats are those of the host restatement."""
    got, _ = g.generate_greedy_batch(suffixes, n_predict, n_batch=n_batch, prefix=prefix)
    st = g.prefix_stats()
    want, _ = g.generate_greedy_batch([prefix + s for s in suffixes], n_predict, n_batch=n_batch)
    assert got.shape == want.shape and got.shape[0] == len(suffixes)
    assert (got == want).all(), (len(prefix), n_batch, len(suffixes), np.argwhere(got != want)[:6])
    lay = ref.layout(len(prefix), n_batch, [len(s) for s in suffixes])
    assert st == dict(n_shared=lay["n_shared"], prompt_columns=lay["prompt_columns"], path=path, columns=len(suffixes)), st
    return got


# ---- 1. greedy == concatenation ----
# (n_prefix, n_batch, columns, path): path 1 where the plain call's steps are column-per-XCD launches (2 .. 8 columns, the longest sequence + 1 <= 256 keys)
GREEDY_CASES = [
    (1, 1, 3, 1), (1, 8, 3, 1), (2, 1, 3, 1), (2, 8, 3, 1),      # n_shared 0, 0, 1, 0
    (9, 8, 1, 0), (9, 8, 3, 1), (9, 8, 8, 1),                    # one column is never a column-per-XCD call; 3 and 8: copied
    (65, 8, 9, 0), (65, 8, 47, 0), (65, 8, 48, 0), (65, 8, 64, 0),      # in place, both sides of the slim (48) and matrix-core (48 / 64) cross-overs
    (300, 1, 3, 0),                                              # past 256 keys 3 columns stay on the launch chain: in place, n_shared 299
    (300, 8, 16, 0), (300, 8, 13, 0),
]


@pytest.mark.parametrize("n_prefix,n_batch,cols,path", GREEDY_CASES)
@pytest.mark.parametrize("name", ["q4_0", "q5_1"])
def test_greedy_prefix_equals_concatenation(pkg, files, name, n_prefix, n_batch, cols, path):
    g = pkg.BiogptModel.load(files[name])
    prefix, suffixes = make_case(n_prefix + cols, n_prefix, cols)
    check_greedy(g, prefix, suffixes, n_batch, path)
    g.close()


# ---- 2. bucket borders and the end of the position table ----

@pytest.mark.parametrize("n_prefix,cols,path", [(250, 3, 1), (250, 9, 0), (505, 3, 0), (505, 9, 0)])
def test_greedy_prefix_steps_cross_a_bucket(pkg, files, n_prefix, cols, path):
    """250 + 12 tokens cross 256 keys (3 columns: the copied path, whose steps leave the column-per-XCD launches there as the plain call's do),
    505 + 12 cross 512."""
    g = pkg.BiogptModel.load(files["q4_0"])
    prefix, suffixes = make_case(n_prefix, n_prefix, cols, lens=[0, 1, 2])
    got = check_greedy(g, prefix, suffixes, 8, path, n_predict=12)
    assert got.shape == (cols, 12)
    g.close()


def test_greedy_prefix_reaches_n_positions(pkg, files):
    g = pkg.BiogptModel.load(files["q4_0"])
    prefix, suffixes = make_case(5, 1000, 3, lens=[17, 0, 5])
    got = check_greedy(g, prefix, suffixes, 8, 0, n_predict=50)
    assert got.shape == (3, 7)                                             # clamped: 1024 - (1000 + 17)
    suffixes[1] = suffixes[0] + [9] * 7                                    # 1000 + 24: the table is full, as the plain call returns no token
    got, _ = g.generate_greedy_batch(suffixes, 1, prefix=prefix)
    want, _ = g.generate_greedy_batch([prefix + s for s in suffixes], 1)
    assert got.shape == want.shape == (3, 0)
    with pytest.raises(pkg.BiogptError, match="n_positions"):
        g.generate_greedy_batch([suffixes[1] + [9]], 1, prefix=prefix)      # one token more does not fit at all
    g.close()


# ---- 3. sampling == concatenation ----

def check_sample(g, prefix, suffixes, n_samples, eos_id, path, n_predict=N_PREDICT, seed=11):
    got, _ = g.generate_sample(suffixes, n_predict, n_samples=n_samples, seed=seed, eos_id=eos_id, prefix=prefix)
    st = g.prefix_stats()
    want, _ = g.generate_sample([prefix + s for s in suffixes], n_predict, n_samples=n_samples, seed=seed, eos_id=eos_id)
    assert len(got) == len(want) == len(suffixes) * n_samples
    assert [len(a) for a in got] == [len(b) for b in want]
    assert all((a == b).all() for a, b in zip(got, want)), [r for r, (a, b) in enumerate(zip(got, want)) if not (a == b).all()][:8]
    lay = ref.layout(len(prefix), 8, [len(s) for s in suffixes])
    assert st == dict(n_shared=lay["n_shared"], prompt_columns=lay["prompt_columns"], path=path, columns=len(suffixes) * n_samples), st
    return got


@pytest.mark.parametrize("cols,path", [(6, 1), (48, 0)])
@pytest.mark.parametrize("n_samples", [1, 3])
@pytest.mark.parametrize("name", ["q4_0", "q5_1"])
def test_sample_prefix_equals_concatenation(pkg, files, name, n_samples, cols, path):
    g = pkg.BiogptModel.load(files[name])
    prefix, suffixes = make_case(cols + n_samples, 65, cols // n_samples)
    free = check_sample(g, prefix, suffixes, n_samples, -1, path)
    assert all(len(a) == N_PREDICT for a in free)
    ids, counts = np.unique(np.concatenate([a[:-1] for a in free]), return_counts=True)
    eos = int(ids[np.argmax(counts)])                                       # the most frequent id in front of a last token as the EOS: a sequence that drew it ends early
    ended = check_sample(g, prefix, suffixes, n_samples, eos, path)
    assert any(len(a) < N_PREDICT for a in ended)
    g.close()


def test_samples_of_the_prefix_alone(pkg, files):
    """One prompt with an empty suffix x 16 samples: the prompt's own rows are the prefix's last chunk, shared among the samples by kv_share_kernel."""
    g = pkg.BiogptModel.load(files["q4_0"])
    prefix, _ = make_case(16, 70, 1)
    got = check_sample(g, prefix, [[]], 16, -1, 0)
    assert len({tuple(a) for a in got}) > 1                                 # different seeds: not sixteen copies of one sequence
    g.close()


# ---- 4. a captured step serves calls whose prefixes differ ----

def test_two_prefixes_of_different_length_back_to_back(pkg, files):
    """Same shape (9 columns), same context bucket, n_shared 64 and 88: a prefix baked into the captured step would give the second call the first's rows."""
    g = pkg.BiogptModel.load(files["q4_0"])
    for seed, n_prefix in ((1, 65), (2, 90), (3, 65)):
        prefix, suffixes = make_case(seed, n_prefix, 9)
        check_greedy(g, prefix, suffixes, 8, 0)
    for seed, n_prefix in ((4, 70), (5, 100)):
        prefix, suffixes = make_case(seed, n_prefix, 3)
        check_sample(g, prefix, suffixes, 3, -1, 0)
    g.close()


def test_ids_depend_on_the_shared_rows(pkg, files):
    """What makes the equalities above a check: two prefixes that differ in shared rows only (tokens 1 .. 63 of 70; every sequence's own columns are the
    same tokens at the same positions) give different ids, on the copied path and in place."""
    g = pkg.BiogptModel.load(files["q4_0"])
    prefix, suffixes = make_case(6, 70, 9)
    other = [prefix[0]] + [5 + (t % 1000) for t in prefix[1:64]] + prefix[64:]
    for cols in (4, 9):
        a = check_greedy(g, prefix, suffixes[:cols], 8, 1 if cols == 4 else 0)
        b = check_greedy(g, other, suffixes[:cols], 8, 1 if cols == 4 else 0)
        assert (a != b).any(axis=1).sum() >= cols // 2, (cols, a, b)
    g.close()


# ---- 4b. the in-place steps on attn_prefix_kernel<8> (BIOGPT_HIP_PREFIX_ATTN=1: the kernel for every shared-prefix step, whatever the thresholds) ----

@pytest.fixture
def grouped(monkeypatch):
    """The switch is read when a model is loaded: set before load."""
    monkeypatch.setenv("BIOGPT_HIP_PREFIX_ATTN", "1")


@pytest.mark.parametrize("n_prefix,cols,n_predict", [(65, 9, 6), (300, 13, 6), (300, 16, 6), (65, 48, 6), (250, 9, 12), (505, 13, 12)])
@pytest.mark.parametrize("name", ["q4_0", "q5_1"])
def test_greedy_prefix_on_the_grouped_kernel(pkg, files, grouped, name, n_prefix, cols, n_predict):
    """In a call the kernel works on per-layer cache offsets, a slot stride over n + 1 slots, the chain's Q8 hand-off and captured steps: a masked last group
    (9, 13 columns), whole groups (16, 48), steps across the 256- and 512-key buckets, suffixes of 0 .. 40 tokens (up to 52 own rows)."""
    g = pkg.BiogptModel.load(files[name])
    prefix, suffixes = make_case(n_prefix + cols + 1, n_prefix, cols)
    got = check_greedy(g, prefix, suffixes, 8, 0, n_predict=n_predict)
    assert got.shape == (cols, n_predict)
    g.close()
    plain = pkg.BiogptModel.load(files[name])       # (the switch does not reach the plain call; the yardstick again from a model of its own)
    want, _ = plain.generate_greedy_batch([prefix + s for s in suffixes], n_predict)
    assert (got == want).all()
    plain.close()


def test_greedy_prefix_default_dispatch_at_128_columns(pkg, files):
    """No switch: 128 columns behind 376 shared rows is where enqueue_attention takes the grouped kernel by itself (PREFIX_ATTN_MIN_COLS / _MIN_SHARED), on
    the matrix-core chain."""
    g = pkg.BiogptModel.load(files["q4_0"])
    prefix, suffixes = make_case(128, 384, 128, lens=[0, 1, 2, 7, 60])
    check_greedy(g, prefix, suffixes, 8, 0)
    g.close()


@pytest.mark.parametrize("n_samples,cols", [(1, 13), (3, 48)])
def test_sample_prefix_on_the_grouped_kernel(pkg, files, grouped, n_samples, cols):
    g = pkg.BiogptModel.load(files["q4_0"])
    prefix, suffixes = make_case(cols + n_samples + 2, 130, cols // n_samples)
    check_sample(g, prefix, suffixes, n_samples, -1, 0)
    prefix2, _ = make_case(77, 90, 1)                # another prefix length through the same captured step
    check_sample(g, prefix2, suffixes, n_samples, -1, 0)
    g.close()


# ---- 5. argument errors ----

def test_prefix_gen_argument_errors(pkg, files):
    g = pkg.BiogptModel.load(files["q4_0"])
    V = KW["n_vocab"]
    for field, prefix, suffixes in [
        ("n_prefix", [], [[7]]),
        ("token id", [2, V], [[7]]),
        ("token id -3", [2, 5], [[7], [9, -3]]),
        ("token id", [2, 5], [[7, V + 1]]),
        (r"suffix_lens\[1\].*n_positions", [2] * 1000, [[7], [9] * 25]),
        ("n_positions", [2] * 1025, [[7]]),
        (r"\[1, 511\]", [2, 5], []),
        (r"\[1, 511\]", [2, 5], [[7]] * 512),
    ]:
        with pytest.raises(pkg.BiogptError, match=field):
            g.generate_greedy_batch(suffixes, 4, prefix=prefix)
        with pytest.raises(pkg.BiogptError, match=field):
            g.generate_sample(suffixes, 4, prefix=prefix)
    with pytest.raises(pkg.BiogptError, match=r"\[1, 511\]"):
        g.generate_sample([[7]] * 128, 4, n_samples=4, prefix=[2, 5])
    with pytest.raises(pkg.BiogptError, match="n_batch"):
        g.generate_greedy_batch([[7]], 4, n_batch=0, prefix=[2, 5])
    with pytest.raises(ValueError, match="trie"):
        g.generate_sample([[7]], 4, eos_id=2, trie=object(), prefix=[2, 5])
    with pytest.raises(ValueError, match="rules"):
        g.generate_sample([[7]], 4, repetition_penalty=1.3, prefix=[2, 5])
    # null pointers: only the C-ABI can pass them
    pre = np.array([2, 5, 9], dtype=np.int32)
    flat = np.array([7, 11, 4], dtype=np.int32)
    lens = np.array([1, 2], dtype=np.int32)
    out = np.zeros((2, 4), dtype=np.int32)
    f = pkg.lib().biogpt_hip_generate_greedy_prefix
    for field, args in [("prefix", (None, 3, flat.ctypes.data, lens.ctypes.data, 2, 8, 4, out.ctypes.data)),
                        ("suffixes", (pre.ctypes.data, 3, None, lens.ctypes.data, 2, 8, 4, out.ctypes.data)),
                        ("suffix_lens", (pre.ctypes.data, 3, flat.ctypes.data, None, 2, 8, 4, out.ctypes.data)),
                        ("out_ids", (pre.ctypes.data, 3, flat.ctypes.data, lens.ctypes.data, 2, 8, 4, None))]:
        assert f(g._h, *args, None) == -1
        assert "null argument: " + field in pkg._err(), pkg._err()
    assert pkg.lib().biogpt_hip_prefix_stats(g._h, None) == -1
    assert f(g._h, pre.ctypes.data, 3, flat.ctypes.data, lens.ctypes.data, 2, 8, 4, out.ctypes.data, None) == 4      # seconds_out may be NULL
    want, _ = g.generate_greedy_batch([[2, 5, 9, 7], [2, 5, 9, 11, 4]], 4)
    assert (out == want).all()
    g.close()


@pytest.mark.parametrize("which", ["tiny_f16", "full_f32"])
def test_prefix_gen_rejects_float_files(pkg, tiny_models, files, which):
    g = pkg.BiogptModel.load(tiny_models["f16"] if which == "tiny_f16" else files["f32"])
    with pytest.raises(pkg.BiogptError, match="fast chain"):
        g.generate_greedy_batch([[7], [11, 4]], 4, prefix=[2, 5, 9])
    with pytest.raises(pkg.BiogptError, match="fast chain"):
        g.generate_sample([[7], [11, 4]], 4, prefix=[2, 5, 9])
    g.close()


# ---- 6. isolation: what a call leaves alone ----

def test_prefix_gen_leaves_the_context_alone(pkg, files):
    g = pkg.BiogptModel.load(files["q4_0"])
    rng = np.random.default_rng(3)
    own = [2] + [int(v) for v in rng.integers(4, KW["n_vocab"], 47)]
    prompt = [2] + [int(v) for v in rng.integers(4, KW["n_vocab"], 11)]
    seqs = [[2] + [int(v) for v in rng.integers(4, KW["n_vocab"], n - 1)] for n in (5, 70, 33)]
    prefix, suffixes = make_case(8, 90, 20)
    cpre, conts = prefix[:40], [s + [5] for s in suffixes[:6]]

    def others():
        beams, _ = g.generate_beam(prompt, 6, n_beams=3)
        samples, _ = g.generate_sample([prompt, prompt[:5]], 6, n_samples=3, seed=17)
        return beams, samples, g.score_batch(seqs), g.score_continuations(cpre, conts)

    def prefix_calls():
        a, _ = g.generate_greedy_batch(suffixes, N_PREDICT, prefix=prefix)                  # in place
        b, _ = g.generate_greedy_batch(suffixes[:4], N_PREDICT, prefix=prefix)              # copied
        c, _ = g.generate_sample(suffixes[:5], N_PREDICT, n_samples=3, seed=5, prefix=prefix)
        return [a, b] + c

    before = others()
    g.eval_prompt(own, 0, 8)
    hp = g.hparams
    cnt = hp.n_layer * hp.n_positions * hp.d_model
    kv0 = [g.read_kv(w, 0, cnt) for w in (0, 1)]
    row0 = g.read_logits()
    first = prefix_calls()
    for w in (0, 1):
        assert (g.read_kv(w, 0, cnt) == kv0[w]).all(), "a prefix call wrote into the context's own K / V cache"
    assert (g.read_logits() == row0).all(), "a prefix call changed the context's logits row"
    nxt = g.eval([own[5]], len(own))                                       # the context's own sequence continues where it stood
    h = pkg.BiogptModel.load(files["q4_0"])
    h.eval_prompt(own, 0, 8)
    assert (nxt == h.eval([own[5]], len(own))).all()
    h.close()
    after = others()
    for (ia, sa), (ib, sb) in zip(before[0], after[0]):
        assert (ia == ib).all() and sa == sb
    assert len(before[1]) == len(after[1]) and all((a == b).all() for a, b in zip(before[1], after[1]))
    for k in (2, 3):
        for a, b in zip(before[k], after[k]):
            for x, y in zip(a, b):
                assert (x == y).all()
    second = prefix_calls()                                                # and the other calls leave nothing behind that changes these
    assert len(first) == len(second) and all((a == b).all() for a, b in zip(first, second))
    g.close()
