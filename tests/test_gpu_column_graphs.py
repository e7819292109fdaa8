"""The captured steps of column generation (greedy batch, sampling, beam search) on one context: each mode keeps its own set, keyed by
the call's shape, and all of them hold the same cache, state and logits pointers.  Calls of the three modes with the same column count,
one after another on one context, must each return what a fresh context returns, and a repeated call what it returned the first time --
with the steps replayed from graphs and enqueued eagerly."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KW = dict(n_vocab=42384, n_layer=3, n_head=16, n_positions=1024, d_ff=4096, d_model=1024, n_merges=40000)
N_PREDICT = 12      # steps 2 .. 12 are two groups of enqueued steps: the count of running sequences / searches is read once between them


def prompt_of(n, seed):
    rng = np.random.default_rng(seed)
    return [2] + [int(v) for v in rng.integers(4, KW["n_vocab"], n - 1)]


PROMPTS = [prompt_of(17, 300 + i) for i in range(4)]


@pytest.fixture(scope="module")
def q40(pkg, tmp_path_factory):
    d = tmp_path_factory.mktemp("column_graphs")
    f32, path = str(d / "f32.bin"), str(d / "q4_0.bin")
    pkg.write_synthetic(f32, **KW)
    pkg.quantize_file(f32, path, "q4_0")
    return path


def greedy4(g):
    return g.generate_greedy_batch(PROMPTS, N_PREDICT)[0].tolist()


def sample4(g):      # 2 prompts x 2 samples; an EOS id that the poll reads for (it need not fire)
    return [list(map(int, ids)) for ids in g.generate_sample(PROMPTS[:2], N_PREDICT, n_samples=2, seed=11, eos_id=3)[0]]


def beam(g, B):
    return [(list(map(int, ids)), float(s)) for ids, s in g.generate_beam(PROMPTS[0], N_PREDICT, n_beams=B, eos_id=-1)[0]]


def beam_2x2(g):
    return [[(list(map(int, ids)), float(s)) for ids, s in h] for h in g.generate_beam_batch(PROMPTS[:2], N_PREDICT, n_beams=2, eos_id=-1)[0]]


CALLS = [("greedy_batch 4", greedy4), ("sample 2x2", sample4), ("beam B=4", lambda g: beam(g, 4)), ("beam_batch 2x2", beam_2x2),
         ("beam B=4", lambda g: beam(g, 4)), ("beam B=2", lambda g: beam(g, 2)), ("greedy_batch 4", greedy4)]


def test_modes_share_a_context(pkg, q40, monkeypatch):
    monkeypatch.delenv("BIOGPT_HIP_NO_GRAPH", raising=False)
    fresh = {}
    for label, call in CALLS:
        if label not in fresh:
            g = pkg.BiogptModel.load(q40)
            fresh[label] = call(g)
            g.close()
    g = pkg.BiogptModel.load(q40)
    for env in ({}, {"BIOGPT_HIP_NO_GRAPH": "1"}):
        monkeypatch.delenv("BIOGPT_HIP_NO_GRAPH", raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        g.refresh_options()
        first = {}
        for at, (label, call) in enumerate(CALLS):
            got = call(g)
            assert got == fresh[label], (env, at, label, "differs from a fresh context")
            assert got == first.setdefault(label, got), (env, at, label, "differs from its first occurrence")
    g.close()


# ---- every form of the closed calls, at one column count, on one context ----
# A mode's captured steps are filed by the form of the step: its selection (plain, rules, trie, the wide sampler), log-probabilities or not, a prefix read in
# place or not, column-per-XCD launches or the launch chain.  No form may replay another's step.

PREFIX = prompt_of(17, 77)                                   # 16 rows are shared at n_batch 8
TEN = [prompt_of(17, 300 + i) for i in range(10)]
TRIE_ENTRIES = [[5, 6, 7, 8] + prompt_of(11, 900 + i)[1:] for i in range(6)] + [[5, 9] + prompt_of(13, 950 + i)[1:] for i in range(4)]
WIDE = dict(top_k=0, min_p=0.05)
EOS = 3                                                      # in no prompt and no trie entry


def plain(out):
    """A call's result without its seconds, as nested lists: float32 arrays by their bit patterns."""
    def conv(v):
        if isinstance(v, np.ndarray):
            return (v.view(np.int32) if v.dtype == np.float32 else v).tolist()
        if isinstance(v, (list, tuple)):
            return [conv(x) for x in v]
        return v
    return conv(out[:-1])


def form_calls(pkg, n, trie):
    """The fifteen forms with n columns each: n greedy sequences, n / 2 prompts x 2 samples, n / 2 searches x 2 beams."""
    ps, half = TEN[:n], TEN[:n // 2]
    sfx, half_sfx = [p[1:9] for p in ps], [p[1:9] for p in half]
    skw = dict(n_samples=2, seed=11, eos_id=EOS)
    bkw = dict(n_beams=2)
    return [
        ("sample", lambda g: g.generate_sample(half, N_PREDICT, **skw)),
        ("sample rules", lambda g: g.generate_sample(half, N_PREDICT, repetition_penalty=1.3, **skw)),
        ("sample trie", lambda g: g.generate_sample(half, N_PREDICT, trie=trie, **skw)),
        ("sample prefix", lambda g: g.generate_sample(half_sfx, N_PREDICT, prefix=PREFIX, **skw)),
        ("sample lp", lambda g: g.generate_sample(half, N_PREDICT, logprobs=2, **skw)),
        ("sample lp prefix", lambda g: g.generate_sample(half_sfx, N_PREDICT, logprobs=2, prefix=PREFIX, **skw)),
        ("sample wide", lambda g: g.generate_sample(half, N_PREDICT, sampler=pkg.sampler(**WIDE), **skw)),
        ("sample wide prefix", lambda g: g.generate_sample(half_sfx, N_PREDICT, sampler=pkg.sampler(**WIDE), prefix=PREFIX, **skw)),
        ("greedy", lambda g: g.generate_greedy_batch(ps, N_PREDICT)),
        ("greedy prefix", lambda g: g.generate_greedy_batch(sfx, N_PREDICT, prefix=PREFIX)),
        ("greedy lp", lambda g: g.generate_greedy_batch(ps, N_PREDICT, logprobs=2)),
        ("greedy lp prefix", lambda g: g.generate_greedy_batch(sfx, N_PREDICT, logprobs=2, prefix=PREFIX)),
        ("beam", lambda g: g.generate_beam_batch(half, N_PREDICT, eos_id=-1, **bkw)),
        ("beam rules", lambda g: g.generate_beam_batch(half, N_PREDICT, eos_id=-1, no_repeat_ngram_size=2, repetition_penalty=1.3, **bkw)),
        ("beam trie", lambda g: g.generate_beam_batch(half, N_PREDICT, eos_id=EOS, trie=trie, **bkw)),
    ]


@pytest.mark.parametrize("n", [4, 10])      # 4: steps as column-per-XCD launches where the device serves them; 10: the launch chain, a prefix read in place
def test_forms_share_a_context(pkg, q40, monkeypatch, n):
    monkeypatch.delenv("BIOGPT_HIP_NO_GRAPH", raising=False)
    trie = pkg.Trie.build(TRIE_ENTRIES, KW["n_vocab"])
    calls = form_calls(pkg, n, trie)
    fresh = {}
    for label, call in calls:
        g = pkg.BiogptModel.load(q40)
        fresh[label] = plain(call(g))
        g.close()
    assert len({repr(v) for v in fresh.values()}) >= 8, "fixture problem: the forms hardly differ in what they return"
    g = pkg.BiogptModel.load(q40)
    for env in ({}, {"BIOGPT_HIP_NO_GRAPH": "1"}):
        monkeypatch.delenv("BIOGPT_HIP_NO_GRAPH", raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        g.refresh_options()
        first = {}
        for at, (label, call) in enumerate(calls + calls[::-1]):      # every form twice, all the others between its two occurrences
            got = plain(call(g))
            if n == 10 and "prefix" in label:
                assert g.prefix_stats()["path"] == 0 and g.prefix_stats()["n_shared"] == 16, (env, at, label, g.prefix_stats())
            assert got == fresh[label], (env, at, label, "differs from a fresh context")
            assert got == first.setdefault(label, got), (env, at, label, "differs from its first occurrence")
    g.close()
    trie.close()
