"""rules_ref (the restatement the engine's generation rules are held to) against transformers' own logits processors, on the CPU: the tiny seeded
BioGptForCausalLM of test_beam_restatement.py (nothing downloaded), generate(repetition_penalty, no_repeat_ngram_size, min_new_tokens,
suppress_tokens) greedy and with beams, against a greedy loop / beam_ref.beam_search over rules_ref.apply_rules.  Ids identical, beam scores
within 1e-5.  The fixture's strength is asserted: every rule changes some output, min_new_tokens overrides an EOS that would have come earlier,
and an n-gram ban comes from the prompt."""
import os

import numpy as np
import pytest

os.environ.setdefault("HF_HUB_OFFLINE", "1")
transformers = pytest.importorskip("transformers")
torch = pytest.importorskip("torch")

import beam_ref  # noqa: E402
import rules_ref  # noqa: E402

PROMPT = [2, 17, 40, 5, 33, 17, 40]      # the last two tokens occur before: with n = 3 the first step's ban (token 5) comes from the prompt
N_NEW = 12
M_MIN = 8
MODES = [1, 2, 4, 5]                     # 1: greedy search


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(1234)
    cfg = transformers.BioGptConfig(vocab_size=96, hidden_size=32, num_hidden_layers=2, num_attention_heads=2, intermediate_size=64,
                                    max_position_embeddings=64, initializer_range=0.5, pad_token_id=1, bos_token_id=0, eos_token_id=None)
    return transformers.BioGptForCausalLM(cfg).eval()


def logits_fn(m):
    cache = {}

    def fn(prefix):
        key = tuple(prefix)
        if key not in cache:
            with torch.no_grad():
                cache[key] = m(torch.tensor([list(PROMPT) + list(prefix)])).logits[0, -1].to(torch.float32)
        return cache[key]
    return fn


def logprob_fn(m):
    lf = logits_fn(m)
    return lambda prefixes: np.stack([torch.log_softmax(lf(p), dim=-1).numpy() for p in prefixes])


def ref_greedy(m, rules, eos):
    lf, ids = logits_fn(m), []
    for _ in range(N_NEW):
        row = rules_ref.apply_rules(lf(ids).numpy(), PROMPT + ids, len(PROMPT), rules, eos)
        ids.append(int(np.argmax(row)))
        if eos >= 0 and ids[-1] == eos:
            break
    return ids


def ref_run(m, B, rules, eos, es=True):
    """[(ids, score or None), ...] of the restatement."""
    if B == 1:
        return [(ref_greedy(m, rules, eos), None)]
    hyps, _ = beam_ref.beam_search(rules_ref.rules_logprobs(logprob_fn(m), PROMPT, rules, eos), B, N_NEW, eos, 1.0, es)
    return [(list(i), float(s)) for i, s in hyps]


def hf_run(m, B, rules, eos, es=True):
    r = rules_ref.full(rules)
    kw = dict(max_new_tokens=N_NEW, eos_token_id=eos if eos >= 0 else None, pad_token_id=1, do_sample=False, return_dict_in_generate=True,
              repetition_penalty=float(r["repetition_penalty"]), no_repeat_ngram_size=int(r["no_repeat_ngram_size"]),
              min_new_tokens=int(r["min_new_tokens"]) if r["min_new_tokens"] else None,
              suppress_tokens=list(r["suppress_tokens"]) if len(r["suppress_tokens"]) else None)
    with torch.no_grad():
        if B == 1:
            out = m.generate(torch.tensor([PROMPT]), num_beams=1, **kw)
            ids = out.sequences[0, len(PROMPT):].tolist()
            if eos >= 0 and eos in ids:
                ids = ids[:ids.index(eos) + 1]
            return [(ids, None)]
        out = m.generate(torch.tensor([PROMPT]), num_beams=B, num_return_sequences=B, early_stopping=es, length_penalty=1.0, output_scores=True, **kw)
    n_gen = (out.beam_indices + 1).bool().sum(dim=1)
    return [(out.sequences[i, len(PROMPT):len(PROMPT) + int(n_gen[i])].tolist(), float(out.sequences_scores[i])) for i in range(B)]


@pytest.fixture(scope="module")
def fixture(model):
    """The EOS id (the third token of the free greedy run: that run ends after 3 < M_MIN tokens) and the rule sets (the suppressed ids are the
    first two distinct tokens of the free greedy run)."""
    free = ref_greedy(model, None, -1)
    eos = free[2]
    assert eos not in free[:2]
    sup = [int(t) for t in dict.fromkeys(free) if t != eos][:2]
    assert len(sup) == 2
    sets = {
        "penalty": dict(repetition_penalty=1.3),
        "penalty_below_1": dict(repetition_penalty=0.8),
        "ngram_3": dict(no_repeat_ngram_size=3),
        "ngram_1": dict(no_repeat_ngram_size=1),
        "min_new": dict(min_new_tokens=M_MIN),
        "suppress": dict(suppress_tokens=sup),
    }
    sets["all"] = dict(repetition_penalty=1.3, no_repeat_ngram_size=3, min_new_tokens=M_MIN, suppress_tokens=sets["suppress"]["suppress_tokens"])
    return eos, sets


SET_NAMES = ["penalty", "penalty_below_1", "ngram_3", "ngram_1", "min_new", "suppress", "all"]


@pytest.mark.parametrize("es", [True, False])
@pytest.mark.parametrize("use_eos", [False, True])
@pytest.mark.parametrize("B", MODES)
@pytest.mark.parametrize("name", SET_NAMES)
def test_rules_match_transformers(model, fixture, name, B, use_eos, es):
    if B == 1 and not es:
        es = True      # (greedy search has no early_stopping: the same case twice)
    eos_id, sets = fixture
    eos = eos_id if use_eos else -1
    want = hf_run(model, B, sets[name], eos, es)
    got = ref_run(model, B, sets[name], eos, es)
    assert len(got) == len(want) == B
    for (ids_w, s_w), (ids_g, s_g) in zip(want, got):
        assert ids_w == ids_g, (ids_w, ids_g)
        if s_w is not None:
            assert abs(s_w - s_g) <= 1e-5, (s_w, s_g)


@pytest.mark.parametrize("name", SET_NAMES)
def test_every_rule_set_changes_some_output(model, fixture, name):
    eos_id, sets = fixture
    changed = 0
    for B in MODES:
        for eos in (-1, eos_id):
            changed += [i for i, _ in ref_run(model, B, sets[name], eos)] != [i for i, _ in ref_run(model, B, None, eos)]
    print("%s: %d of %d runs differ from the run without rules" % (name, changed, 2 * len(MODES)))
    assert changed >= 1


def test_min_new_tokens_overrides_an_earlier_eos(model, fixture):
    eos_id, sets = fixture
    for B in MODES:
        free = ref_run(model, B, None, eos_id)
        assert any(len(i) < M_MIN and i[-1] == eos_id for i, _ in free), (B, free)
        held = ref_run(model, B, sets["min_new"], eos_id)
        assert all(eos_id not in i[:M_MIN - 1] for i, _ in held), (B, held)
        assert ref_run(model, B, sets["min_new"], -1) == ref_run(model, B, None, -1)      # ignored without an EOS id


def test_an_ngram_ban_comes_from_the_prompt(model):
    row = np.zeros(96, dtype=np.float32)
    out = rules_ref.apply_rules(row, PROMPT, len(PROMPT), dict(no_repeat_ngram_size=3))
    assert np.flatnonzero(np.isneginf(out)).tolist() == [5]
    for B in MODES:      # token 5 is out of every first step, and no 3-gram of prompt + output occurs twice
        for ids, _ in ref_run(model, B, dict(no_repeat_ngram_size=3), -1):
            assert ids[0] != 5 and not rules_ref.ngram_repeats(PROMPT + ids, 3), ids


def test_apply_rules_arithmetic():
    row = np.array([2.0, -3.0, 0.0, 1.5, -0.5, 7.0], dtype=np.float32)
    p = np.float32(1.3)
    out = rules_ref.apply_rules(row, [0, 1, 1, 0, 4], 2, dict(repetition_penalty=1.3, suppress_tokens=[5]), eos=3)
    assert out[0] == np.float32(2.0) / p and out[1] == np.float32(-3.0) * p and out[4] == np.float32(-0.5) * p
    assert out[2] == 0.0 and out[3] == np.float32(1.5) and np.isneginf(out[5])
    out = rules_ref.apply_rules(row, [0, 1, 1], 2, dict(min_new_tokens=2), eos=3)
    assert np.isneginf(out[3]) and np.isfinite(np.delete(out, 3)).all()
    out = rules_ref.apply_rules(row, [0, 1, 1, 4], 2, dict(min_new_tokens=2), eos=3)
    assert np.isfinite(out).all()
    out = rules_ref.apply_rules(row, [0, 1, 2, 0, 1], 5, dict(no_repeat_ngram_size=3))      # tail (0, 1) occurred at 0: ban 2
    assert np.flatnonzero(np.isneginf(out)).tolist() == [2]
    out = rules_ref.apply_rules(row, [0, 1], 2, dict(no_repeat_ngram_size=3))                # L + 1 >= n, no position to match
    assert np.isfinite(out).all()
    out = rules_ref.apply_rules(row, [4], 1, dict(no_repeat_ngram_size=3))                   # L + 1 < n
    assert np.isfinite(out).all()
