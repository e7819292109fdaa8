"""Scoring statistics and the comparison of two files as whole calls (BiogptModel.score / score_batch with top, rank, entropy; BiogptModel.compare) on
the tiny files of conftest.py (no chain: score only), on a small wide file (not BioGPT-base widths, an odd vocabulary of 77: the rows of a pass lie on all
four 16-byte alignments; the full-width files of wide_models.py take minutes to write) and on a one-layer file at BioGPT-base widths with an odd vocabulary
(the chain that has score_batch and logprobs=).  Rank, entropy and KL are held to the float64 restatement (score_stats_ref.py) on the rows
eval_prompt(.., n_batch = 1) returns, which are score()'s rows bit for bit (test_gpu_score.py); everything else is equality."""
import numpy as np
import pytest

import score_stats_ref as R

pytestmark = pytest.mark.gpu

WIDE = dict(n_vocab=77, n_layer=1, n_head=3, n_positions=40, d_ff=96, d_model=192, n_merges=3)
BASE = dict(n_vocab=1031, n_layer=1, n_head=16, n_positions=64, d_ff=4096, d_model=1024, n_merges=3)
N_VOCAB = dict(q4_0=320, q5_1=320, f16=320, f32=320, wide=77, base_q4_0=1031, base_q5_1=1031)
ROWS = [0, 15, 16, 17, 31, 32]      # 16 columns per pass: the first row and both sides of two borders


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def held(got, ref):
    return (np.abs(np.asarray(got, dtype=np.float64) - ref) <= R.tolerance(ref)).all()


@pytest.fixture(scope="module")
def paths(pkg, tiny_models, tmp_path_factory):
    d = tmp_path_factory.mktemp("score_stats")
    out = dict(tiny_models)
    for fam, kw, types in (("wide", WIDE, ("q4_0",)), ("base", BASE, ("q4_0", "q5_1"))):
        f32 = str(d / (fam + "_f32.bin"))
        pkg.write_synthetic(f32, **kw)
        for t in types:
            out[fam if fam == "wide" else fam + "_" + t] = str(d / ("%s_%s.bin" % (fam, t)))
            pkg.quantize_file(f32, out[fam if fam == "wide" else fam + "_" + t], t)
    return out


def tokens_of(name, n=36):
    return [2] + [(53 * i + 29) % (N_VOCAB[name] - 4) + 4 for i in range(n - 1)]


def rows_of(pkg, path, toks):
    """The logits rows score() reduces, from a second load: row i = eval_prompt(toks[:i + 1], 0, 1)."""
    h = pkg.BiogptModel.load(path)
    out = {i: h.eval_prompt(toks[:i + 1], 0, 1).copy() for i in ROWS}
    h.close()
    return out


@pytest.mark.parametrize("K", [0, 8])
@pytest.mark.parametrize("name", ["q4_0", "q5_1", "f16", "wide", "base_q4_0"])
def test_score_stats_equals_score_and_the_restatement(pkg, paths, monkeypatch, name, K):
    monkeypatch.setenv("BIOGPT_HIP_PROMPT_COLS", "16")
    toks = tokens_of(name)
    g = pkg.BiogptModel.load(paths[name])
    lp, am, lg = g.score(toks)
    last = g.read_logits().copy()
    got = g.score(toks, top=K, rank=True, entropy=True)
    assert np.array_equal(bits(got["lp"]), bits(lp)) and np.array_equal(got["argmax"], am) and np.array_equal(bits(got["logit"]), bits(lg))
    assert np.array_equal(bits(g.read_logits()), bits(last)) and got["top_ids"].shape == (len(toks), K) and got["rank"][-1] == -1
    for i, row in rows_of(pkg, paths[name], toks).items():
        ref = R.row_stats(row, toks[i + 1], K)
        print("%s K=%d row %d: rank %d (ref %d), entropy %.9g (ref %.12g)" % (name, K, i, got["rank"][i], ref["rank"], got["entropy"][i], ref["entropy"]))
        assert got["rank"][i] == ref["rank"] and held(got["entropy"][i], ref["entropy"]) and np.array_equal(got["top_ids"][i], ref["top_ids"]), (name, i)
    if g.chain_kind() != 0:      # the chains score_batch is open to
        seqs = [toks[:n] for n in (1, 7, 19)]
        for seq, b in zip(seqs, g.score_batch(seqs, top=K, rank=True, entropy=True)):
            one = g.score(seq, top=K, rank=True, entropy=True)
            assert all(np.array_equal(bits(b[key]), bits(one[key])) for key in one), (name, len(seq))
    g.close()


@pytest.mark.parametrize("name", ["base_q4_0", "base_q5_1"])
def test_top_rows_equal_generation_logprobs(pkg, paths, name):
    g = pkg.BiogptModel.load(paths[name])
    prompts = [[2, 17, 40, 9], [2, 301, 5, 77, 12, 200, 31]]
    ids, info, _ = g.generate_greedy_batch(prompts, 12, 1, logprobs=5)
    scored = g.score_batch([p + [int(v) for v in s] for p, s in zip(prompts, ids)], top=5)
    for p, s, (lp, top_ids, top_lp), sc in zip(prompts, ids, info, scored):
        at = slice(len(p) - 1, len(p) - 1 + len(s))
        assert len(s) > 0 and np.array_equal(sc["top_ids"][at], top_ids) and np.array_equal(bits(sc["top_lp"][at]), bits(top_lp)), name
        assert np.array_equal(bits(sc["lp"][at]), bits(lp)), name
    g.close()


@pytest.mark.parametrize("name_p, name_q", [("wide", "wide"), ("q4_0", "f32")])
def test_compare(pkg, paths, monkeypatch, name_p, name_q):
    monkeypatch.setenv("BIOGPT_HIP_PROMPT_COLS", "16")
    toks = tokens_of(name_p)
    p, q = pkg.BiogptModel.load(paths[name_p]), pkg.BiogptModel.load(paths[name_q])
    c = p.compare(q, toks)
    with pytest.raises(pkg.BiogptError, match="same context"):
        p.compare(p, toks)
    if name_p == name_q:      # a file against a second load of itself
        assert (c["kl"] == 0.0).all() and (c["kl_rev"] == 0.0).all() and np.array_equal(c["argmax"], c["argmax_other"])
    rp, rq = rows_of(pkg, paths[name_p], toks), rows_of(pkg, paths[name_q], toks)
    for i in ROWS:
        ref = R.row_kl(rp[i], rq[i])
        print("row %d: kl %.9g (ref %.12g), kl_rev %.9g (ref %.12g)" % (i, c["kl"][i], ref[0], c["kl_rev"][i], ref[1]))
        assert held(c["kl"][i], ref[0]) and held(c["kl_rev"][i], ref[1]) and (name_p == name_q or ref[0] > 0.0), i
    # each context is left as score() leaves it: the same outputs, and the next eval continues the sequence
    for m, lp_name, am_name, name in ((p, "lp", "argmax", name_p), (q, "lp_other", "argmax_other", name_q)):
        fresh = pkg.BiogptModel.load(paths[name])
        lp, am, _ = fresh.score(toks)
        assert np.array_equal(bits(c[lp_name]), bits(lp)) and np.array_equal(c[am_name], am), lp_name
        assert np.array_equal(bits(m.read_logits()), bits(fresh.read_logits()))
        assert np.array_equal(bits(m.eval([17], len(toks))), bits(fresh.eval([17], len(toks)))), lp_name
        fresh.close()
        m.close()
