"""beam_ref (the restatement biogpt_hip_generate_beam is held to) against transformers' own beam search, on the CPU: a tiny seeded
BioGptForCausalLM (nothing downloaded), generate(num_beams=B, do_sample=False, num_return_sequences=B) against beam_ref driven by the
same model's log-softmax rows.  Sequences identical, scores within 1e-5."""
import os

import numpy as np
import pytest

os.environ.setdefault("HF_HUB_OFFLINE", "1")
transformers = pytest.importorskip("transformers")
torch = pytest.importorskip("torch")

import beam_ref  # noqa: E402  (tests/ is on sys.path under pytest's rootdir-relative imports)

PROMPT = [2, 17, 40, 5, 33, 61, 8]
N_NEW = 12


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(1234)
    cfg = transformers.BioGptConfig(vocab_size=96, hidden_size=32, num_hidden_layers=2, num_attention_heads=2, intermediate_size=64,
                                    max_position_embeddings=64, initializer_range=0.5, pad_token_id=1, bos_token_id=0, eos_token_id=None)
    m = transformers.BioGptForCausalLM(cfg).eval()
    return m


def logprob_fn(m, prompt):
    cache = {}

    def fn(prefixes):
        out = []
        for p in prefixes:
            key = tuple(p)
            if key not in cache:
                with torch.no_grad():
                    lg = m(torch.tensor([list(prompt) + list(p)])).logits[0, -1].to(torch.float32)
                cache[key] = torch.log_softmax(lg, dim=-1).numpy()
            out.append(cache[key])
        return np.stack(out)
    return fn


def hf_beam(m, B, eos, lp, es):
    with torch.no_grad():
        r = m.generate(torch.tensor([PROMPT]), num_beams=B, max_new_tokens=N_NEW, early_stopping=es, length_penalty=lp,
                       eos_token_id=eos, pad_token_id=1, do_sample=False, num_return_sequences=B, output_scores=True,
                       return_dict_in_generate=True)
    if B == 1:   # num_beams=1 is transformers' greedy search: the score from its per-step rows
        ids = r.sequences[0, len(PROMPT):].tolist()
        s = torch.zeros((), dtype=torch.float32)
        for t, row in zip(ids, r.scores):
            s = s + torch.log_softmax(row[0].to(torch.float32), dim=-1)[t]
        return [(ids, float(beam_ref.normalize(float(s), len(ids), lp)))]
    n_gen = (r.beam_indices + 1).bool().sum(dim=1)
    return [(r.sequences[i, len(PROMPT):len(PROMPT) + int(n_gen[i])].tolist(), float(r.sequences_scores[i])) for i in range(B)]


def eos_coverage(fn, eos):
    """(hypotheses that EOS ended before N_NEW tokens, runs that stopped before N_NEW steps) over B = 2, 4, 5 and both early_stopping."""
    short = early = 0
    for B in (2, 4, 5):
        for es in (True, False):
            hyps, margins = beam_ref.beam_search(fn, B, N_NEW, eos, 1.0, es)
            short += sum(1 for ids, _ in hyps if len(ids) < N_NEW and ids[-1] == eos)
            early += len(margins) < N_NEW
    return short, early


@pytest.fixture(scope="module")
def eos_id(model):
    """The first token that, as EOS, finishes hypotheses mid-run and lets some run stop before N_NEW steps."""
    fn = logprob_fn(model, PROMPT)
    for e in range(model.config.vocab_size):
        short, early = eos_coverage(fn, e)
        if short and early:
            return e
    pytest.fail("no token of the seeded model ends hypotheses mid-run as EOS: the fixture exercises nothing")


@pytest.mark.parametrize("es", [True, False])
@pytest.mark.parametrize("lp", [0.0, 1.0, 2.0])
@pytest.mark.parametrize("B", [1, 2, 4, 5])
@pytest.mark.parametrize("use_eos", [False, True])
def test_restatement_matches_transformers(model, eos_id, B, lp, es, use_eos):
    eos = eos_id if use_eos else None
    want = hf_beam(model, B, eos, lp, es)
    got, margins = beam_ref.beam_search(logprob_fn(model, PROMPT), B, N_NEW, eos if eos is not None else -1, lp, es)
    assert len(got) == B
    for (ids_w, s_w), (ids_g, s_g) in zip(want, got):
        assert ids_w == list(ids_g), (ids_w, ids_g)
        assert abs(s_w - float(s_g)) <= 1e-5, (s_w, float(s_g))


def test_eos_finishes_hypotheses_mid_run_and_can_stop_early(model, eos_id):
    """The fixture exercises what it should: EOS ends hypotheses before N_NEW tokens, and some run stops before N_NEW steps."""
    short, early = eos_coverage(logprob_fn(model, PROMPT), eos_id)
    assert short > 0 and early > 0
