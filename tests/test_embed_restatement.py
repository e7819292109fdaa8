"""embed_ref (the restatement the engine's pooling, normalisation and heads are held to) against transformers, on the CPU: a small random
BioGptConfig (nothing downloaded), a right-padded batch of three sequences of unequal length.

  LAST pooling + the `score` weight            == BioGptForSequenceClassification(...).logits
  no pooling + the `classifier` weight, bias   == BioGptForTokenClassification(...).logits
  MEAN over last_hidden_state                  == the masked mean

embed_ref works in float64 on transformers' own f32 hidden rows; transformers works in f32.  The tolerance is the classical bound of an f32
sum of n terms in any order, gamma_n * sum |terms| with gamma_n = n u / (1 - n u), u = 2^-24: n = hidden_size products + the bias for
the heads (the products themselves round too: one more), n = the sequence's rows + the division for the mean."""
import os

import numpy as np
import pytest

os.environ.setdefault("HF_HUB_OFFLINE", "1")
transformers = pytest.importorskip("transformers")
torch = pytest.importorskip("torch")

import embed_ref  # noqa: E402

HIDDEN = 32
PAD = 1
SEQS = [[2, 17, 40, 5, 33, 17, 40, 61, 9], [2, 8, 77, 30], [2, 55, 12, 90, 41, 6]]
U = 2.0 ** -24


def gamma(n):
    return n * U / (1.0 - n * U)


def config(**kw):
    return transformers.BioGptConfig(vocab_size=96, hidden_size=HIDDEN, num_hidden_layers=2, num_attention_heads=2, intermediate_size=64,
                                     max_position_embeddings=64, initializer_range=0.5, pad_token_id=PAD, bos_token_id=0, eos_token_id=2, **kw)


def batch():
    n = max(len(s) for s in SEQS)
    ids = torch.tensor([s + [PAD] * (n - len(s)) for s in SEQS])
    mask = torch.tensor([[1] * len(s) + [0] * (n - len(s)) for s in SEQS])
    return ids, mask


def run(model):
    ids, mask = batch()
    with torch.no_grad():
        out = model(input_ids=ids, attention_mask=mask, output_hidden_states=True)
    return out, [out.hidden_states[-1][s, :len(seq)].to(torch.float64).numpy() for s, seq in enumerate(SEQS)]


def test_last_pooling_and_score_weight_are_sequence_classification():
    torch.manual_seed(4321)
    m = transformers.BioGptForSequenceClassification(config(num_labels=5)).eval()
    assert m.score.bias is None
    w = m.score.weight.detach().to(torch.float64).numpy()
    out, rows = run(m)
    for s, r in enumerate(rows):
        got = embed_ref.embed(r, pooling="last", w=w)
        want = out.logits[s].to(torch.float64).numpy()
        tol = gamma(HIDDEN + 1) * (np.abs(r[-1]) @ np.abs(w).T)
        print("sequence %d: max |diff| %.3g, bound %.3g" % (s, np.abs(got - want).max(), tol.min()))
        assert got.shape == (5,) and (np.abs(got - want) <= tol).all(), (s, got, want, tol)
    assert np.abs(out.logits.numpy()).max() > 0.1      # not a comparison of zeros


def test_no_pooling_and_classifier_are_token_classification():
    torch.manual_seed(4322)
    m = transformers.BioGptForTokenClassification(config(num_labels=7)).eval()
    with torch.no_grad():
        m.classifier.bias.normal_(0.0, 0.5)      # (initialised to zero: make the bias count)
    w = m.classifier.weight.detach().to(torch.float64).numpy()
    b = m.classifier.bias.detach().to(torch.float64).numpy()
    out, rows = run(m)
    for s, r in enumerate(rows):
        got = embed_ref.embed(r, pooling="none", w=w, b=b)
        want = out.logits[s, :len(SEQS[s])].to(torch.float64).numpy()
        tol = gamma(HIDDEN + 2) * (np.abs(r) @ np.abs(w).T + np.abs(b))
        print("sequence %d: max |diff| %.3g, bound %.3g" % (s, np.abs(got - want).max(), tol.min()))
        assert got.shape == (len(SEQS[s]), 7) and (np.abs(got - want) <= tol).all(), s
    assert np.abs(embed_ref.head(rows[0], w, b) - embed_ref.head(rows[0], w)).max() > 0.05      # the bias was in it


def test_mean_pooling_is_the_masked_mean():
    torch.manual_seed(4323)
    m = transformers.BioGptModel(config()).eval()
    ids, mask = batch()
    with torch.no_grad():
        h = m(input_ids=ids, attention_mask=mask).last_hidden_state
        mf = mask.to(h.dtype).unsqueeze(-1)
        want = ((h * mf).sum(dim=1) / mf.sum(dim=1)).to(torch.float64).numpy()
    for s, seq in enumerate(SEQS):
        r = h[s, :len(seq)].to(torch.float64).numpy()
        got = embed_ref.embed(r, pooling="mean")
        tol = gamma(len(seq) + 1) * np.abs(r).sum(axis=0) / len(seq)
        print("sequence %d: max |diff| %.3g, bound %.3g" % (s, np.abs(got - want[s]).max(), tol.min()))
        assert (np.abs(got - want[s]) <= tol).all(), s
        # padded positions are not in it: the mean over ALL rows of a padded sequence differs
        if len(seq) < ids.shape[1]:
            assert np.abs(h[s].to(torch.float64).numpy().mean(axis=0) - got).max() > 1e-3


def test_hidden_states_index_is_the_layer_index():
    """hidden_states[0] = the embeddings, [k] = the input of layer k, [n_layer] = after the final LayerNorm = last_hidden_state: what
    biogpt_hip_embed_opts::layer counts."""
    torch.manual_seed(4324)
    m = transformers.BioGptModel(config()).eval()
    ids, mask = batch()
    with torch.no_grad():
        out = m(input_ids=ids, attention_mask=mask, output_hidden_states=True)
    assert len(out.hidden_states) == m.config.num_hidden_layers + 1
    assert torch.equal(out.hidden_states[-1], out.last_hidden_state)
    assert not torch.equal(out.hidden_states[0], out.hidden_states[1])
    # entry 0 does not depend on the tokens in front of a position (embeddings), entry 1 does (one layer of attention)
    ids2 = ids.clone()
    ids2[:, 1] = 44
    with torch.no_grad():
        out2 = m(input_ids=ids2, attention_mask=mask, output_hidden_states=True)
    assert torch.equal(out.hidden_states[0][:, 2:], out2.hidden_states[0][:, 2:])
    assert not torch.equal(out.hidden_states[1][:, 2:], out2.hidden_states[1][:, 2:])


def test_restatement_pieces():
    r = np.array([[3.0, 4.0], [0.0, 0.0], [1.0, -1.0]])
    assert (embed_ref.pool(r, "last") == r[-1]).all() and (embed_ref.pool(r, "none") == r).all()
    assert np.allclose(embed_ref.pool(r, "mean"), [4.0 / 3.0, 1.0])
    n = embed_ref.l2_normalize(r)
    assert np.allclose(n[0], [0.6, 0.8]) and (n[1] == 0.0).all() and np.allclose(n[2], [2 ** -0.5, -2 ** -0.5])
    w = np.array([[1.0, 2.0], [0.5, -1.0], [0.0, 0.0]])
    assert np.allclose(embed_ref.head(r[0], w, [1.0, 0.0, -2.0]), [12.0, -2.5, -2.0])
    with pytest.raises(ValueError):
        embed_ref.pool(r, "max")
