"""A vocabulary that is no multiple of 16 through the many-column passes: one-layer files at BioGPT-base widths with n_vocab = 1045 (a fine-tune with a few added
tokens).  The row-tiled weight image of the matrix-core kernels is addressed by whole 16-row tiles, so such an lm_head has none and stays on the 8-column kernel,
while the layers of the same pass run on the matrix cores.  score_batch over 70 and 130 tokens and a decode step of 50 sequences: the target logits equal the
causal oracle's bit for bit -- with targets in the last, partial tile too --, the arg-max rows are equal, and the rows equal score() of the same tokens in passes
below 64 columns (the 8-column kernels throughout); the log-probabilities lie within the derived bound of the float64 log-softmax of the oracle's rows.
logprob_rows_kernel alone gives the same bits for a row on any of the four 16-byte alignments."""
import numpy as np
import pytest

import beam_kernels_ref as bk

pytestmark = pytest.mark.gpu

V = 1045
KW = dict(n_vocab=V, n_layer=1, n_head=16, n_positions=1024, d_ff=4096, d_model=1024, n_merges=16)


@pytest.fixture(scope="module")
def files(pkg, tmp_path_factory):
    d = tmp_path_factory.mktemp("odd_vocab")
    f32 = str(d / "f32.bin")
    pkg.write_synthetic(f32, **KW)
    even = str(d / "f32_1040.bin")
    pkg.write_synthetic(even, **dict(KW, n_vocab=1040))
    out = {}
    for name in ("q4_0", "q5_1"):
        out[name], out[name + ".1040"] = str(d / (name + ".bin")), str(d / (name + "_1040.bin"))
        pkg.quantize_file(f32, out[name], name)
        pkg.quantize_file(even, out[name + ".1040"], name)
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _tokens(seed, n):
    return [2] + [int(v) for v in np.random.default_rng(seed).integers(4, V, n - 1)]


@pytest.mark.parametrize("name", ["q4_0", "q5_1"])
def test_score_batch_with_a_vocabulary_that_is_no_multiple_of_16(pkg, oracle, files, monkeypatch, name):
    seqs = [_tokens(70, 70), _tokens(130, 130)]
    o = oracle.OracleModel(files[name], n_threads=16)
    o.set_mode("ggml", n_threads=16, causal=1)
    refs = [o.eval(s, 0, all_rows=True) for s in seqs]
    g = pkg.BiogptModel.load(files[name])
    monkeypatch.setenv("BIOGPT_HIP_PROMPT_COLS", "32")      # options are read when the context is created
    small = pkg.BiogptModel.load(files[name])
    monkeypatch.delenv("BIOGPT_HIP_PROMPT_COLS")
    try:
        tails = [[V - 1 - (i % 5) for i in range(len(s))] for s in seqs]      # 1044 .. 1040: the rows of the last, partial tile
        for targets in (None, tails):
            before = g.mfma_launches()
            got = g.score_batch(seqs, targets)
            assert g.mfma_launches() - before == 4, "the layer's four stages of the one pass run on the matrix cores, the lm_head does not"
            for i, (s, ref) in enumerate(zip(seqs, refs)):
                lp, am, lg = got[i]
                tg = np.asarray((list(s[1:]) + [-1]) if targets is None else targets[i])
                rows = np.flatnonzero(tg >= 0)
                want = ref[rows, tg[rows]]
                assert (lg[rows].view(np.uint32) == want.view(np.uint32)).all(), (name, i, "target logits differ from the oracle's", np.flatnonzero(lg[rows] != want)[:6])
                assert (am == ref.argmax(axis=1)).all(), (name, i)
                ls = np.stack([bk.log_softmax64(row)[0] for row in ref[rows]])[np.arange(rows.size), tg[rows]]
                assert (np.abs(lp[rows].astype(np.float64) - ls) <= bk.lp_tolerance(V, ls)).all(), (name, i, "log-probabilities off the float64 log-softmax of the oracle's rows")
                assert np.isfinite(lp).all()
                one = small.score(s, 0, list(tg))
                for a, b, what in zip((lp, am, lg), one, ("logprobs", "arg-max", "target logits")):
                    assert (a == b).all(), (name, i, what, "score_batch differs from score in passes of 32 columns")
        assert small.mfma_launches() == 0
    finally:
        g.close(); small.close()


K_TOP = 4


def _order(row, k):
    """The row's k best ids: value descending, equal values lower id first."""
    return np.lexsort((np.arange(row.size), -row.astype(np.float64)))[:k]


@pytest.mark.parametrize("name", ["q4_0", "q5_1"])
def test_decode_step_of_50_sequences_with_a_vocabulary_that_is_no_multiple_of_16(pkg, oracle, files, monkeypatch, name):
    """Three decode steps of 50 columns (n_batch = 1: causal, as score).  Every step's chosen log-probability and its K best ids and log-probabilities equal, as
    bit patterns, score() of prompt ++ ids in passes of 32 columns; the K best ids are those of the causal oracle's row, and every log-probability lies within
    the derived bound (beam_kernels_ref.lp_tolerance) of the float64 log-softmax of that row.  Few of the best ids lie in the last, partial tile (rows 1040 ..
    1044), but every log-probability holds the sum over the whole row: a wrong logit there moves its bits off score's."""
    prompts = [_tokens(1000 + i, 2 + i % 3) for i in range(50)]
    n_predict = 3
    o = oracle.OracleModel(files[name], n_threads=16)
    o.set_mode("ggml", n_threads=16, causal=1)
    g = pkg.BiogptModel.load(files[name])
    monkeypatch.setenv("BIOGPT_HIP_PROMPT_COLS", "32")
    small = pkg.BiogptModel.load(files[name])
    monkeypatch.delenv("BIOGPT_HIP_PROMPT_COLS")
    try:
        ids, info, _ = g.generate_greedy_batch(prompts, n_predict, n_batch=1, logprobs=K_TOP)
        tail_hits = 0
        for r, p in enumerate(prompts):
            gen = [int(t) for t in ids[r]]
            lp, top_ids, top_lp = info[r]
            assert len(gen) == n_predict and lp.shape == (n_predict,) and top_ids.shape == top_lp.shape == (n_predict, K_TOP)
            full = p + gen
            rows = np.arange(len(p) - 1, len(p) - 1 + n_predict)
            ref = o.eval(full, 0, all_rows=True)[rows]

            def scored(targets):
                tg = [-1] * len(full)
                for i, t in zip(rows, targets):
                    tg[i] = int(t)
                return small.score(full, 0, tg)[0][rows]

            assert (bits(lp) == bits(scored(gen))).all(), (name, r, "the chosen tokens' log-probabilities differ from score's", lp.tolist())
            for j in range(K_TOP):
                assert (bits(top_lp[:, j]) == bits(scored(top_ids[:, j]))).all(), (name, r, j, "a top log-probability differs from score's")
            for i in range(n_predict):
                want = _order(ref[i], K_TOP)
                assert (top_ids[i] == want).all() and gen[i] == int(want[0]), (name, r, i, top_ids[i].tolist(), want.tolist())
                ls = bk.log_softmax64(ref[i])[0]
                for got, where in ((lp[i:i + 1], [gen[i]]), (top_lp[i], want)):
                    assert (np.abs(got.astype(np.float64) - ls[where]) <= bk.lp_tolerance(V, ls[where])).all(), (name, r, i)
            tail_hits += int((top_ids >= 1040).sum())
        print("%s: %d of the %d top entries lie in the last, partial tile" % (name, tail_hits, 50 * n_predict * K_TOP))
    finally:
        g.close(); small.close()


@pytest.mark.parametrize("name", ["q4_0", "q5_1"])
def test_decode_steps_keep_the_lm_head_off_the_matrix_cores(pkg, files, name):
    """The same call on the same model cut to 1040 tokens (whole tiles) and with 1045: every pass of either launches the layer's four stages on the matrix cores;
    with 1040 tokens the passes that end in the lm_head launch a fifth there, with 1045 none does."""
    prompts = [[min(t, 1039) for t in _tokens(1000 + i, 2 + i % 3)] for i in range(50)]      # ids both vocabularies have
    delta = {}
    for which in (name, name + ".1040"):
        g = pkg.BiogptModel.load(files[which])
        try:
            g.generate_greedy_batch(prompts, 3, n_batch=1)
            delta[which] = g.mfma_launches()
        finally:
            g.close()
    odd, even = delta[name], delta[name + ".1040"]
    print("%s: %d matrix-core launches with 1045 tokens, %d with 1040" % (name, odd, even))
    assert odd > 0 and odd % 4 == 0, "four stages of the one layer per pass, nothing else"
    assert 0 < even - odd <= odd // 4, "with whole tiles at most one more launch per pass, and at least one: the decode steps' lm_head"


@pytest.mark.parametrize("n_vocab", [1045, 1043, 1046, 42383])
def test_log_probabilities_do_not_depend_on_the_rows_alignment(pkg, n_vocab):
    """logprob_rows_kernel alone on one row repeated eight times: with a row stride that is no multiple of 4 floats the copies lie on all four 16-byte
    alignments (twice each), and all eight log-probabilities, arg-maxes and logits are the same bits -- and within the derived bound of float64."""
    rng = np.random.default_rng(n_vocab)
    row = (rng.standard_normal(n_vocab) * 3.0).astype(np.float32)
    row[-3:] += np.float32(4.0)                                      # mass in the tail behind the last whole quad
    rows = np.ascontiguousarray(np.tile(row, (8, 1)))
    for target in (0, 3, n_vocab // 2, n_vocab - 1):
        lp, am, lg = pkg.logprob_rows(rows, [target] * 8)
        assert (bits(lp) == bits(lp[:1])).all(), (n_vocab, target, lp.tolist())
        assert (am == int(_order(row, 1)[0])).all() and (lg == row[target]).all()
        ls = bk.log_softmax64(row)[0][target]
        assert abs(float(lp[0]) - ls) <= bk.lp_tolerance(n_vocab, ls), (n_vocab, target, float(lp[0]), ls)
