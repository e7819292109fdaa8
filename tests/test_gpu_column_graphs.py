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
