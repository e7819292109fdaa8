"""contrast_ref (the restatement biogpt_hip_generate_contrastive is held to) on the CPU: hand-made rows where the answer is known, and
transformers' own contrastive search on a tiny seeded BioGptForCausalLM (nothing downloaded) where this transformers still has it."""
import os

import numpy as np
import pytest

os.environ.setdefault("HF_HUB_OFFLINE", "1")      # (read when transformers / huggingface_hub are first imported, by whichever module does that)

import contrast_ref  # noqa: E402

D = 1024


def unit(i, d=D):
    v = np.zeros(d, dtype=np.float32)
    v[i] = 1.0
    return v


def test_wave_sum_and_dot_are_sums():
    rng = np.random.default_rng(0)
    v = rng.standard_normal(64)
    assert abs(contrast_ref.wave_sum(v) - v.sum()) < 1e-12
    a, b = rng.standard_normal(D).astype(np.float32), rng.standard_normal((5, D)).astype(np.float32)
    want = b.astype(np.float64) @ a.astype(np.float64)
    assert np.allclose(contrast_ref.dots(a, b), want, rtol=0, atol=1e-11)
    small = rng.standard_normal((3, 12)).astype(np.float32)      # a width that is no multiple of 256
    assert np.allclose(contrast_ref.dots(small[0], small), small.astype(np.float64) @ small[0].astype(np.float64), rtol=0, atol=1e-13)


def test_candidate_equal_to_a_context_row_is_penalised_by_exactly_one():
    rng = np.random.default_rng(1)
    ctx = rng.standard_normal((70, D)).astype(np.float32)
    cand = np.stack([ctx[37], (3.0 * ctx[5]).astype(np.float32)])      # (a power-of-two-free multiple: still the same direction up to f32 rounding)
    pen = contrast_ref.penalties(cand, ctx)
    assert pen[0] == np.float32(1.0)
    assert abs(float(pen[1]) - 1.0) <= 2 ** -23


def test_orthogonal_candidate_is_penalised_by_zero():
    ctx = np.stack([unit(0), unit(1), (2.0 * unit(2)).astype(np.float32)])
    pen = contrast_ref.penalties(np.stack([unit(7), unit(1)]), ctx)
    assert pen[0] == np.float32(0.0) and pen[1] == np.float32(1.0)


def test_negative_similarity_is_kept():
    pen = contrast_ref.penalties(np.stack([-unit(3)]), np.stack([unit(3)]))
    assert pen[0] == np.float32(-1.0)


def test_zero_norm_rows_have_similarity_zero():
    ctx = np.stack([np.zeros(D, np.float32), -unit(4)])
    pen = contrast_ref.penalties(np.stack([unit(4), np.zeros(D, np.float32)]), ctx)
    assert pen[0] == np.float32(0.0)      # max(sim with the zero row = 0, sim with -e4 = -1)
    assert pen[1] == np.float32(0.0)      # a zero candidate: every sim is 0


def test_ties_go_to_the_lower_candidate():
    ctx = np.stack([unit(0)])
    cand = np.stack([unit(5), unit(6), unit(7)])
    pen, sc, w, margin = contrast_ref.rank(cand, ctx, [0.25, 0.25, 0.25], 0.6)
    assert w == 0 and margin == 0.0 and sc[0] == sc[1] == sc[2]
    _, _, w, _ = contrast_ref.rank(cand, ctx, [0.1, 0.25, 0.25], 0.6)
    assert w == 1


def test_score_arithmetic():
    pen, sc, w, margin = contrast_ref.rank(np.stack([unit(0), unit(1)]), np.stack([unit(0)]), [0.9, 0.2], 0.6)
    a = float(np.float32(0.6))
    assert sc[0] == np.float32((1.0 - a) * float(np.float32(0.9)) - a * 1.0)
    assert sc[1] == np.float32((1.0 - a) * float(np.float32(0.2)))
    assert w == 1 and abs(margin - (float(sc[1]) - float(sc[0]))) == 0.0


def test_candidates_order_and_probabilities():
    row = np.array([0.5, 3.0, -1.0, 3.0, 2.0, 0.5], dtype=np.float32)
    ids, p = contrast_ref.candidates(row, 4)
    assert ids == [1, 3, 4, 0]
    full = np.exp(row.astype(np.float64) - 3.0)
    assert np.allclose(p, (full / full.sum())[ids], rtol=1e-6)


def toy_rows(n_vocab=40, d=32, seed=3):
    """A deterministic 'model': the rows of a prefix depend on the whole prefix."""
    def rows(prefixes):
        hid, lg = [], []
        for p in prefixes:
            rng = np.random.default_rng([seed, len(p)] + [int(t) for t in p])
            hid.append(rng.standard_normal(d).astype(np.float32))
            lg.append((3.0 * rng.standard_normal(n_vocab)).astype(np.float32))
        return np.stack(hid), np.stack(lg)
    return rows


@pytest.mark.parametrize("k, alpha", [(1, 0.6), (4, 0.0), (1, 0.0)])
def test_one_candidate_or_no_penalty_is_argmax(k, alpha):
    rows = toy_rows()
    prompt_hidden = np.random.default_rng(9).standard_normal((6, 32)).astype(np.float32)
    ids, scores, margins = contrast_ref.search(rows, prompt_hidden, 9, k, alpha)
    want, pre = [], []
    for _ in range(9):
        pre.append(int(np.argmax(rows([pre])[1][0])))
        want = list(pre)
    assert ids == want
    assert len(scores) == len(margins) == 9


def test_search_stops_at_eos_and_includes_it():
    rows = toy_rows()
    prompt_hidden = np.random.default_rng(9).standard_normal((6, 32)).astype(np.float32)
    free, _, _ = contrast_ref.search(rows, prompt_hidden, 9, 4, 0.6)
    ids, scores, margins = contrast_ref.search(rows, prompt_hidden, 9, 4, 0.6, eos_id=free[3])
    cut = free.index(free[3]) + 1
    assert ids == free[:cut] and len(scores) == len(margins) == cut


def test_empty_prompt_context_is_allowed():
    ids, _, _ = contrast_ref.search(toy_rows(), np.zeros((0, 32), np.float32), 4, 3, 0.5)
    assert len(ids) == 4


# ---- transformers' own contrastive search (releases that still carry it in the library; newer ones fetch it from the hub: never attempted) ----

def test_against_transformers(monkeypatch):
    transformers = pytest.importorskip("transformers")
    torch = pytest.importorskip("torch")
    if not hasattr(transformers.GenerationMixin, "_contrastive_search"):
        pytest.skip("this transformers loads contrastive search from the hub")
    monkeypatch.setenv("HF_HUB_OFFLINE", "1")      # (for whatever reads it at call time; the guard above is what rules a hub access out)
    torch.manual_seed(1234)
    cfg = transformers.BioGptConfig(vocab_size=96, hidden_size=32, num_hidden_layers=2, num_attention_heads=2, intermediate_size=64,
                                    max_position_embeddings=64, initializer_range=0.5, pad_token_id=1, bos_token_id=0, eos_token_id=None)
    m = transformers.BioGptForCausalLM(cfg).eval()
    prompt = [2, 17, 40, 5, 33, 61, 8]
    cache = {}

    def both(tokens):
        key = tuple(tokens)
        if key not in cache:
            with torch.no_grad():
                o = m(torch.tensor([list(tokens)]), output_hidden_states=True)
            cache[key] = (o.hidden_states[-1][0].to(torch.float32).numpy(), o.logits[0, -1].to(torch.float32).numpy())
        return cache[key]

    def rows(prefixes):
        got = [both(list(prompt) + list(p)) for p in prefixes]
        return np.stack([g[0][-1] for g in got]), np.stack([g[1] for g in got])

    prompt_hidden = both(prompt)[0][:-1]
    for k, alpha in ((2, 0.4), (4, 0.6), (8, 0.6)):
        want, _, margins = contrast_ref.search(rows, prompt_hidden, 12, k, alpha)
        with torch.no_grad():
            r = m.generate(torch.tensor([prompt]), penalty_alpha=alpha, top_k=k, max_new_tokens=12, do_sample=False, pad_token_id=1)
        got = r[0, len(prompt):].tolist()
        # transformers computes the same quantities in f32 torch arithmetic: a decision is comparable where its margin exceeds what f32 sums
        # over 32 and 96 terms can move a score by (1e-5, the bound the GPU tests use).  The seeded model keeps every margin above it.
        small = [(i + 1, g) for i, g in enumerate(margins) if g <= 1e-5]
        assert not small, "fixture problem: selection margins below 1e-5 at steps %s" % small
        assert len(want) == 12 and got == want, (k, alpha, got, want, margins)
