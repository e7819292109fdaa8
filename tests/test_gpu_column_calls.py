"""The four column-generation calls (sampling, beam search, contrastive search, greedy batch) through one context, one after another: calls that grow a
mode's buffers (and so drop its captured steps), a call with rules (another graph set), a call whose n_predict clamps to 0.  Every call must return, byte for
byte, what the same call returns alone on a fresh context -- with the steps replayed from graphs and enqueued eagerly.  No tolerance anywhere: the modes
themselves are held to their references by their own tests."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KW = dict(n_vocab=42384, n_layer=3, n_head=16, n_positions=1024, d_ff=4096, d_model=1024, n_merges=40000)      # the file of test_gpu_sample.py
N_PREDICT = 6


def prompt_of(n, seed):
    rng = np.random.default_rng(seed)
    return [2] + [int(v) for v in rng.integers(4, KW["n_vocab"], n - 1)]


PROMPTS = [prompt_of(5 + i, 700 + i) for i in range(5)]      # 5 .. 9 tokens
FULL = prompt_of(KW["n_positions"], 799)                     # leaves no room to generate: n_predict clamps to 0


def canon(x):
    """ids, lengths, scores and counts of a call's result as bytes and integers: equality of two of these is equality byte for byte"""
    if isinstance(x, np.ndarray):
        return (x.dtype.str, x.shape, x.tobytes())
    if isinstance(x, float):
        return np.float32(x).tobytes()
    if isinstance(x, (list, tuple)):
        return (len(x),) + tuple(canon(v) for v in x)
    return int(x)


def sample(g, prompts, seeds):
    return canon(g.generate_sample(prompts, N_PREDICT, seeds=seeds, eos_id=3)[0])


def beam(g, prompts, n_beams, **rules):
    return canon(g.generate_beam_batch(prompts, N_PREDICT, n_beams=n_beams, eos_id=-1, **rules)[0])


def contrastive(g, prompts):
    return canon(g.generate_contrastive(prompts, N_PREDICT, top_k=2, penalty_alpha=0.6, eos_id=3))


def greedy(g, prompts):
    return canon(g.generate_greedy_batch(prompts, N_PREDICT)[0])


CALLS = [
    ("sample 2", lambda g: sample(g, PROMPTS[:2], [11, 12])),
    ("sample 5", lambda g: sample(g, PROMPTS, [21, 22, 23, 24, 25])),                 # grows sample_ctl: the captured steps go
    ("beam 1x2", lambda g: beam(g, PROMPTS[:1], 2)),
    ("beam 2x3 rules", lambda g: beam(g, PROMPTS[1:3], 3, repetition_penalty=1.3)),   # the graph set of a call with rules
    ("contrastive 2x2", lambda g: contrastive(g, PROMPTS[:2])),
    ("contrastive 3x2", lambda g: contrastive(g, PROMPTS[2:5])),                      # grows the context store: the captured steps go
    ("sample 2", lambda g: sample(g, PROMPTS[:2], [11, 12])),
    ("greedy 2", lambda g: greedy(g, PROMPTS[3:5])),
]
CLAMPED = [      # (the call with no room to generate, what it returns, the ordinary call that follows it)
    (lambda g: g.generate_sample([FULL], N_PREDICT, seeds=[1])[0], [], "sample 2"),
    (lambda g: g.generate_beam_batch([FULL], N_PREDICT, n_beams=2, eos_id=-1)[0], [[]], "beam 1x2"),
    (lambda g: [a.tolist() for a in g.generate_contrastive([FULL], N_PREDICT, top_k=2)[0]], [[]], "contrastive 2x2"),
    (lambda g: g.generate_greedy_batch([FULL, FULL[:7]], N_PREDICT)[0].shape, (2, 0), "greedy 2"),
]


@pytest.fixture(scope="module")
def q40(pkg, tmp_path_factory):
    d = tmp_path_factory.mktemp("column_calls")
    f32, path = str(d / "f32.bin"), str(d / "q4_0.bin")
    pkg.write_synthetic(f32, **KW)
    pkg.quantize_file(f32, path, "q4_0")
    return path


@pytest.fixture(scope="module")
def fresh(pkg, q40):
    """every call alone on a context of its own (captured steps, the default)"""
    assert "BIOGPT_HIP_NO_GRAPH" not in os.environ
    out = {}
    for label, call in CALLS:
        if label not in out:
            g = pkg.BiogptModel.load(q40)
            out[label] = call(g)
            g.close()
    return out


def test_calls_share_a_context(pkg, q40, fresh, monkeypatch):
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


def test_a_clamped_call_leaves_nothing_behind(pkg, q40, fresh, monkeypatch):
    monkeypatch.delenv("BIOGPT_HIP_NO_GRAPH", raising=False)
    calls = dict(CALLS)
    g = pkg.BiogptModel.load(q40)
    for at, (clamped, nothing, label) in enumerate(CLAMPED):
        assert clamped(g) == nothing, (at, label, "a call with no room to generate returns 0")
        assert calls[label](g) == fresh[label], (at, label, "differs from a fresh context after a clamped call")
    g.close()
