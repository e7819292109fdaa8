"""trie_ref (the restatement trie-constrained generation is held to) against transformers' own prefix_allowed_tokens_fn /
PrefixConstrainedLogitsProcessor, on the CPU: the tiny seeded BioGptForCausalLM of test_rules_restatement.py (nothing downloaded),
generate(prefix_allowed_tokens_fn=...) greedy and with 2 / 4 beams and both early_stopping values, against a greedy loop / beam_ref's search over
trie_ref's masked rows.  The hypotheses with a finite score are compared, ids identical and scores within 1e-4: which candidate at -inf torch's top-k
takes is its unspecified tie order.  The fixture's strength is asserted: finite margins of at least 1e-5, the constraint changes the output, rows with
fewer allowed tokens than 2 x num_beams occur, and every finite hypothesis is an entry.

Where the comparison ends: transformers keeps a finished candidate among the step's 2 x num_beams as a running beam at score - 1e9, which beats a
candidate at -inf.  So once a step has fewer than num_beams finite candidates that do not stop, it goes on decoding behind an EOS, and the hypotheses that
come of it (scores near -1e9 / length, counted as not finite below) fill its pool, which under early_stopping ends its search early.  beam_ref's search
has no such stand-in: there the places go to candidates at -inf, which die out.  The fixture (150 entries over 12 tokens) stays clear of that regime on
the beams it follows; INTEGRATION.md, "Constrained decoding", names the difference."""
import os

import numpy as np
import pytest

os.environ.setdefault("HF_HUB_OFFLINE", "1")
transformers = pytest.importorskip("transformers")
torch = pytest.importorskip("torch")

import beam_ref  # noqa: E402
import trie_ref  # noqa: E402

PROMPT = [2, 17, 40, 5, 33, 17, 40]
N_NEW = 8
EOS = 9
VOCAB = 96
_rng = np.random.default_rng(21)
POOL = [int(t) for t in _rng.choice(np.arange(10, VOCAB), 12, replace=False)]
ENTRIES = [[int(t) for t in _rng.choice(POOL, int(_rng.integers(1, 6)))] for _ in range(150)]      # depth <= 5 < N_NEW: every entry can finish
TRIE = trie_ref.RefTrie(ENTRIES)


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(1234)
    cfg = transformers.BioGptConfig(vocab_size=VOCAB, hidden_size=32, num_hidden_layers=2, num_attention_heads=2, intermediate_size=64,
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


def allowed_fn(batch_id, input_ids):
    return TRIE.allowed(input_ids.tolist()[len(PROMPT):], EOS)


def ref_greedy(m, trie):
    lf, ids = logits_fn(m), []
    for _ in range(N_NEW):
        row = lf(ids).numpy()
        ids.append(int(np.argmax(trie.mask(row, ids, EOS) if trie else row)))
        if ids[-1] == EOS:
            break
    return ids


def hf_run(m, B, es=True, constrained=True):
    kw = dict(max_new_tokens=N_NEW, eos_token_id=EOS, pad_token_id=1, do_sample=False, return_dict_in_generate=True,
              prefix_allowed_tokens_fn=allowed_fn if constrained else None)
    with torch.no_grad():
        if B == 1:
            ids = m.generate(torch.tensor([PROMPT]), num_beams=1, **kw).sequences[0, len(PROMPT):].tolist()
            return [(ids[:ids.index(EOS) + 1] if EOS in ids else ids, None)]
        out = m.generate(torch.tensor([PROMPT]), num_beams=B, num_return_sequences=B, early_stopping=es, length_penalty=1.0, output_scores=True, **kw)
    n_gen = (out.beam_indices + 1).bool().sum(dim=1)
    return [(out.sequences[i, len(PROMPT):len(PROMPT) + int(n_gen[i])].tolist(), float(out.sequences_scores[i])) for i in range(B)]


def test_greedy_matches_transformers(model):
    want = hf_run(model, 1)[0][0]
    got = ref_greedy(model, TRIE)
    assert got == want, (got, want)
    assert got[-1] == EOS and tuple(got[:-1]) in TRIE.entries
    assert got != ref_greedy(model, None)[:len(got)]      # the constraint changes the run
    assert hf_run(model, 1, constrained=False)[0][0] == ref_greedy(model, None)


@pytest.mark.parametrize("es", [True, False])
@pytest.mark.parametrize("B", [2, 4])
def test_beams_match_transformers_on_the_finite_hypotheses(model, B, es):
    hyps, margins = trie_ref.beam_search_trie(logprob_fn(model), TRIE, B, N_NEW, EOS, 1.0, es)
    small = [(k + 1, m) for k, m in enumerate(margins) if m < 1e-5]
    assert not small, "fixture problem: finite selection margins below 1e-5 at steps %s" % small
    got = [(ids, float(s)) for ids, s in trie_ref.finite(hyps)]
    want = [(ids, s) for ids, s in hf_run(model, B, es) if s > -1e8]      # (-1e9 / length: transformers' stand-in, see above)
    assert len(got) == len(want) >= 1, (got, want)
    for (ids_w, s_w), (ids_g, s_g) in zip(want, got):
        assert ids_w == ids_g, (ids_w, ids_g)
        assert abs(s_w - s_g) <= 1e-4, (s_w, s_g)
        assert ids_g[-1] == EOS and tuple(ids_g[:-1]) in TRIE.entries
    free, _ = beam_ref.beam_search(logprob_fn(model), B, N_NEW, EOS, 1.0, es)
    assert [list(i) for i, _ in free] != [i for i, _ in got]


def test_fixture_has_narrow_rows_and_the_mask_is_the_processor(model):
    """Rows with fewer allowed tokens than 2 x 4 occur along the entries (candidates at -inf enter the step's 2B), and trie_ref.mask is
    PrefixConstrainedLogitsProcessor's scores + mask on a row."""
    sizes = [len(TRIE.allowed(list(e[:k]), EOS)) for e in TRIE.entries for k in range(len(e) + 1)]
    assert min(sizes) < 8 and max(sizes) >= 8, (min(sizes), max(sizes))
    proc = transformers.PrefixConstrainedLogitsProcessor(allowed_fn, 1)
    row = torch.randn(1, VOCAB)
    for gen in ([], list(ENTRIES[0][:1]), list(ENTRIES[0]), [POOL[0], 3], [3]):
        want = proc(torch.tensor([PROMPT + gen]), row.clone())[0].numpy()
        assert np.array_equal(TRIE.mask(row[0].numpy(), gen, EOS), want), gen
