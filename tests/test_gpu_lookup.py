"""Prompt-lookup speculative decoding (biogpt_hip_generate_lookup, kernels_lookup.hip.h): the draft and the accept kernel alone against the host restatement
(tests/lookup_ref.py), the call's ids against generate_greedy_batch / generate_greedy (exactly: no tolerance anywhere), its counters against the simulator.

The tiny fixtures (d_model 64) are served by neither generate_greedy_batch nor this mode -- both need the BioGPT-base fast chain and say so; the identity
tests run on 3-layer full-width files of every block-quantized type."""
import numpy as np
import pytest

import lookup_ref

pytestmark = pytest.mark.gpu

KW = dict(n_vocab=42384, n_layer=3, n_head=16, n_positions=1024, d_ff=4096, d_model=1024, n_merges=40000)      # the file of test_gpu_score.py
QUANT = ["q4_0", "q4_1", "q5_0", "q5_1", "q8_0"]
N_PREDICT = 16


def prompt_of(n, seed):
    rng = np.random.default_rng(seed)
    return [2] + [int(v) for v in rng.integers(4, KW["n_vocab"], n - 1)]


SETS = {
    1: [prompt_of(12, 1)],
    3: [prompt_of(60, 31), prompt_of(250, 32), prompt_of(7, 33)],      # the verify columns straddle 64 keys, and 256 (where single-token attention changes kernels)
    9: [prompt_of(n, 90 + i) for i, n in enumerate((5, 40, 9, 62, 17, 6, 33, 21, 11))],
}


@pytest.fixture(scope="module")
def files(pkg, tmp_path_factory):
    d = tmp_path_factory.mktemp("lookup_full")
    f32 = str(d / "f32.bin")
    pkg.write_synthetic(f32, **KW)
    out = {}
    for name in QUANT:
        out[name] = str(d / (name + ".bin"))
        pkg.quantize_file(f32, out[name], name)
    return out


@pytest.fixture(scope="module")
def q40(pkg, files):
    g = pkg.BiogptModel.load(files["q4_0"])
    yield g
    g.close()


@pytest.fixture(scope="module")
def greedy(q40):
    """generate_greedy_batch of every prompt set, once"""
    return {n: [[int(t) for t in row] for row in q40.generate_greedy_batch(ps, N_PREDICT)[0]] for n, ps in SETS.items()}


def corpus_for(prompts, want):
    """even prompts: their own continuation (every draft right); odd prompts: the continuation with every fifth token wrong (drafts made and cut short)"""
    return [list(want[p]) if p % 2 == 0 else [t if i % 5 != 3 else (t + 1) % KW["n_vocab"] for i, t in enumerate(want[p])] for p in range(len(prompts))]


def check_stats(prompts, corpus, want, stats, max_draft, max_ngram, eos_id=-1):
    for p, pr in enumerate(prompts):
        sim, _ = lookup_ref.simulate(pr, corpus[p] if corpus else [], want[p], max_draft, max_ngram, eos_id)
        assert stats[p] == sim, (p, stats[p], sim)


# ---- 1. the draft kernel alone ----

def draft_texts():
    rng = np.random.default_rng(7)
    texts = [[int(v) for v in rng.integers(0, 3, n)] for n in (1, 2, 63, 64, 65)]
    long = [int(v) for v in rng.integers(4, 9, 1100)]      # "corpus" and "prompt" both long, a 5-symbol alphabet: matches at every n, many i
    texts.append(long)
    texts.append([int(v) for v in rng.integers(10, 4000, 300)] + [5000, 5001, 5002])      # no match at all
    texts.append([7, 8, 9, 1, 2, 3, 9] + [int(v) for v in range(100, 400)] + [5, 9])          # a match only at n = 1
    texts.append([int(v) for v in range(600, 900)] + [600, 601, 602])                       # one match, at i = 0, of every n up to 3
    texts.append(texts[2] + [1, 1])                                                         # finished: drafts nothing
    texts.append(long[:700])                                                                # room 0
    texts.append(long[:701])                                                                # room 2
    return texts


@pytest.mark.parametrize("max_draft", [1, 7, 15])
@pytest.mark.parametrize("max_ngram", [1, 3, 8])
def test_draft_kernel_alone(pkg, max_ngram, max_draft):
    texts = draft_texts()
    n = len(texts)
    n_predict = 40
    n_gen = [0, 1, 5, 0, 20, 30, 3, 0, 1, 4, 39, 37]
    n_past = [len(t) - 1 + (3 if i % 2 else 0) for i, t in enumerate(texts)]      # (the position is not the text length: a corpus, another chunking)
    finished = [0] * n
    finished[9] = 1
    drafts, d, cols = pkg.lookup_draft(texts, n_gen, n_past, n_predict, max_draft=max_draft, max_ngram=max_ngram, finished=finished)
    kinds = set()
    for s, t in enumerate(texts):
        room = n_predict - n_gen[s] - 1
        want, wn, wi = lookup_ref.draft(t, max_ngram, 0 if finished[s] else max_draft, room)
        assert drafts[s] == want and int(d[s]) == len(want), (s, len(t), drafts[s], want)
        assert cols[s].tolist() == lookup_ref.column_states(t[-1], n_past[s], s, want, max_draft).tolist(), s
        kinds.add((wn, len(want) == max_draft))
    assert drafts[6] == [] and drafts[9] == [] and drafts[10] == [] and len(drafts[11]) == min(2, max_draft)
    assert drafts[7][:1] == [1] and drafts[8] == list(range(603, 603 + max_draft))
    assert len({k[0] for k in kinds}) >= 2


# ---- 2. the accept kernel alone ----

def rows_with(rng, n_vocab, am):
    """rows of N(0, 1) logits whose arg-max is am[r] (am[r] < 0: left random)"""
    rows = rng.standard_normal((len(am), n_vocab)).astype(np.float32)
    for r, a in enumerate(am):
        if a >= 0:
            rows[r, a] = 9.0
    return rows


@pytest.mark.parametrize("n_vocab", [320, 1021, 42383, 42384])      # (odd widths: the stacked rows start on all four 16-byte alignments)
def test_accept_kernel_alone(pkg, n_vocab):
    rng = np.random.default_rng(n_vocab)
    md, n_predict, eos = 7, 20, 77
    hi = n_vocab - 1
    cases = [      # (draft, arg-max of rows 0 .. (-1: random), n_gen)
        ([4, 5, 6, 7, 8, 9, 10], [4, 5, 6, 7, 8, 9, 10, hi], 2),       # all drafts right
        ([4, 5, 6], [9, 5, 6, 7, -1, -1, -1, -1], 2),                  # first draft wrong
        ([4, 0, 6, 8, 9], [4, 0, hi, 8, 9, 3, -1, -1], 0),             # wrong in the middle; row 1 (row 17 of the stack: with an odd width 1 or 3 floats off
        #                                                                a 16-byte boundary) has its maximum at id 0, in the scalar head, row 2 in the tail
        ([], [11, -1, -1, -1, -1, -1, -1, -1], 5),                     # d = 0
        ([4, 5, 6], [4, 5, 6, 7, -1, -1, -1, -1], 1),                  # row 1 holds an exact tie (below): the lower id wins
        ([4, eos, 6, 7], [4, eos, 6, 7, 8, -1, -1, -1], 3),            # EOS inside the accepted run
        ([4, 5, 6, 7], [4, 5, 6, 7, 8, -1, -1, -1], 17),               # n_predict reached inside the run
        ([4, 5], [4, 5, 6, -1, -1, -1, -1, -1], 17),                   # ... exactly at its end
        ([4, 5], [4, 5, 6, -1, -1, -1, -1, -1], 20),                   # finished before: untouched
        ([], [-1, -1, -1, -1, -1, -1, -1, -1], 4),                     # d = 0, row 0 all -inf (below): id 0
        ([], [-1, -1, -1, -1, -1, -1, -1, -1], 6),                     # d = 0, row 0 all NaN (below): id 0
    ]
    n = len(cases) if n_vocab == 320 else 5      # (the wide rows: the first five cases)
    cases = cases[:n]
    rows = np.concatenate([rows_with(rng, n_vocab, am) for _, am, _ in cases])
    rows[4 * (md + 1) + 1, [5, 200]] = 9.0      # case 4, row 1: ids 5 and 200 tie; 5 is drafted and wins
    rows[4 * (md + 1) + 2, [6, 3]] = 9.0        # ... row 2: ids 3 and 6 tie; 6 is drafted and loses
    if n_vocab == 320:
        rows[9 * (md + 1)] = -np.inf
        rows[10 * (md + 1)] = np.nan
        assert lookup_ref.argmax_low(rows[9 * (md + 1)]) == 0 and lookup_ref.argmax_low(rows[10 * (md + 1)]) == 0
    n_gen = [c[2] for c in cases]
    n_past = [30 + 3 * s + g for s, g in enumerate(n_gen)]
    finished = [1 if g >= n_predict else 0 for g in n_gen]
    emitted, state, stats, (live, far) = pkg.lookup_accept(rows, [c[0] for c in cases], n_gen, n_past, n_predict, md, eos_id=eos, finished=finished)
    want_live, want_far = n - sum(finished), max(n_past)
    for s, (dr, _, g) in enumerate(cases):
        am = [lookup_ref.argmax_low(rows[s * (md + 1) + j]) for j in range(md + 1)]
        if finished[s]:
            assert emitted[s] == [] and state[s].tolist() == [-1, n_past[s], g, 1] and stats[s].tolist() == [0, 0, 0]
            continue
        out, tok, npast, ng, fin, acc = lookup_ref.accept(am, dr, g, n_past[s], n_predict, eos)
        assert emitted[s] == out, (s, emitted[s], out)
        assert state[s].tolist() == [tok, npast, ng, int(fin)], s
        assert stats[s].tolist() == [1, len(dr), acc], s
        want_live -= int(fin)
        want_far = max(want_far, npast)
    assert (live, far) == (want_live, want_far)
    assert emitted[0] == [4, 5, 6, 7, 8, 9, 10, hi] and emitted[1] == [9] and emitted[2] == [4, 0, hi] and emitted[3] == [11] and emitted[4] == [4, 5, 3]
    if n_vocab == 320:
        assert emitted[5] == [4, eos] and emitted[6] == [4, 5, 6] and emitted[7] == [4, 5, 6] and state[5][3] == 1 and state[6][3] == 1 and state[7][3] == 1
        assert emitted[9] == [0] and emitted[10] == [0] and state[9][0] == 0 and state[10][0] == 0      # (never the empty pair's id 0x7fffffff)


# ---- 3. identity with greedy decoding ----

@pytest.mark.parametrize("with_corpus", [False, True])
@pytest.mark.parametrize("max_draft", [0, 1, 7, 15])
@pytest.mark.parametrize("n_prompts", [1, 3, 9])
def test_ids_are_greedy_ids(q40, greedy, n_prompts, max_draft, with_corpus):
    prompts, want = SETS[n_prompts], greedy[n_prompts]
    corpus = corpus_for(prompts, want) if with_corpus else None
    ids, stats, _ = q40.generate_lookup(prompts, N_PREDICT, max_draft=max_draft, max_ngram=3, corpus=corpus)
    for p in range(n_prompts):
        assert list(ids[p]) == want[p], (p, list(ids[p]), want[p])
    check_stats(prompts, corpus, want, stats, max_draft, 3)
    if with_corpus and max_draft >= 7:
        assert stats[0]["accepted"] >= 8, stats[0]


def test_single_prompt_is_generate_greedy(q40):
    for pr in (SETS[1][0], SETS[3][0], SETS[3][1]):
        want = [int(t) for t in q40.generate_greedy(pr, N_PREDICT)[0]]
        for corpus in (None, [want]):
            ids, stats, _ = q40.generate_lookup([pr], N_PREDICT, max_draft=7, max_ngram=3, corpus=corpus)
            assert list(ids[0]) == want, (len(pr), corpus is not None)


@pytest.mark.parametrize("name", QUANT[1:])
def test_every_quantized_type(pkg, files, name):
    g = pkg.BiogptModel.load(files[name])
    prompts = SETS[3]
    want = [[int(t) for t in row] for row in g.generate_greedy_batch(prompts, N_PREDICT)[0]]
    for max_draft, corpus in ((7, None), (15, corpus_for(prompts, want))):
        ids, stats, _ = g.generate_lookup(prompts, N_PREDICT, max_draft=max_draft, corpus=corpus)
        assert [list(i) for i in ids] == want, (name, max_draft)
        check_stats(prompts, corpus, want, stats, max_draft, 3)
    g.close()


def test_tiny_models_fail_as_greedy_batch_does(pkg, tiny_models):
    for name, path in tiny_models.items():
        g = pkg.BiogptModel.load(path)
        with pytest.raises(pkg.BiogptError, match="needs the BioGPT-base fast chain"):
            g.generate_greedy_batch([[2, 5, 7], [2, 9]], 4)
        with pytest.raises(pkg.BiogptError, match="prompt-lookup decoding needs the BioGPT-base fast chain"):
            g.generate_lookup([[2, 5, 7], [2, 9]], 4)
        g.close()


def test_clamped_by_a_long_prompt(q40):
    """n_predict clamps to 10 for the longest prompt; the drafts of both sequences are cut at the end of the cache"""
    prompts = [prompt_of(KW["n_positions"] - 10, 41), prompt_of(30, 42)]
    want = [[int(t) for t in row] for row in q40.generate_greedy_batch(prompts, N_PREDICT)[0]]
    assert len(want[0]) == 10
    for corpus in (None, [list(w) for w in want]):
        ids, stats, _ = q40.generate_lookup(prompts, N_PREDICT, max_draft=15, max_ngram=3, corpus=corpus)
        assert [list(i) for i in ids] == want
        check_stats(prompts, corpus, want, stats, 15, 3)
    assert stats[0]["passes"] <= 3, stats      # the first pass drafts nothing (no match), the second is cut at n_predict - n_gen - 1 = 8
    ids, stats, _ = q40.generate_lookup([prompt_of(KW["n_positions"], 43)], N_PREDICT)
    assert len(ids[0]) == 0 and stats[0]["passes"] == 0


def test_eos_cuts_the_greedy_ids(q40, greedy):
    prompts, want = SETS[3], greedy[3]
    eos = want[0][5]
    cut = [w[:w.index(eos) + 1] if eos in w else w for w in want]
    assert len(cut[0]) <= 6 and max(len(c) for c in cut) == N_PREDICT
    for max_draft in (0, 7):
        for corpus in (None, corpus_for(prompts, want)):
            ids, stats, _ = q40.generate_lookup(prompts, N_PREDICT, max_draft=max_draft, corpus=corpus, eos_id=eos)
            assert [list(i) for i in ids] == cut, (max_draft, corpus is not None)
            check_stats(prompts, corpus, want, stats, max_draft, 3, eos_id=eos)


def test_batch_independence(q40, greedy):
    prompts, want = SETS[9], greedy[9]
    corpus = corpus_for(prompts, want)
    ids, stats, _ = q40.generate_lookup(prompts, N_PREDICT, max_draft=7, corpus=corpus)
    for p in (0, 3, 4):
        one_i, one_s, _ = q40.generate_lookup([prompts[p]], N_PREDICT, max_draft=7, corpus=[corpus[p]])
        assert list(one_i[0]) == list(ids[p]) and one_s[0] == stats[p], p
    two_i, two_s, _ = q40.generate_lookup([prompts[3], prompts[0]], N_PREDICT, max_draft=7, corpus=[corpus[3], corpus[0]])
    assert list(two_i[0]) == list(ids[3]) and two_s[0] == stats[3]


def test_argument_errors_that_need_the_model(pkg, tiny_models, q40):
    g = pkg.BiogptModel.load(tiny_models["q4_0"])      # n_positions 64, n_vocab 320
    for kw, field in ((dict(prompts=[[2, 5]] * 9, max_draft=7), "exceeds the 64 activation columns"),
                      (dict(prompts=[[2, 5]], corpus=[[4, 320]]), "corpus id 320 out of range"),
                      (dict(prompts=[[2, 5]], corpus=[[4, -1]]), "corpus id -1 out of range"),
                      (dict(prompts=[[2, 5]], eos_id=320), "eos_id"),
                      (dict(prompts=[[2, 5]], corpus=[[4] * (1 << 21)]), "words of the text buffer")):
        with pytest.raises(pkg.BiogptError, match=field):
            g.generate_lookup(n_predict=4, **kw)
    g.close()
    with pytest.raises(pkg.BiogptError, match="empty prompt"):
        q40.generate_lookup([[2, 5], []], 4)
    with pytest.raises(pkg.BiogptError, match="token id 42384 out of range"):
        q40.generate_lookup([[2, 5], [2, KW["n_vocab"]]], 4)


# ---- 4. the speculation really happens ----

def test_own_continuation_as_corpus(q40):
    """corpus = the sequence's own greedy continuation: the counters are the simulator's, and the input is one for which that means at most half the passes"""
    prompts = [prompt_of(12, 1), prompt_of(21, 2)]
    n_predict = 48
    want = [[int(t) for t in row] for row in q40.generate_greedy_batch(prompts, n_predict)[0]]
    for p, pr in enumerate(prompts):      # a condition on the input, not a measurement
        assert lookup_ref.simulate(pr, want[p], want[p], 7, 3)[0]["passes"] <= n_predict // 2, p
    first = None
    for _ in range(2):      # the second call replays the captured steps
        ids, stats, _ = q40.generate_lookup(prompts, n_predict, max_draft=7, max_ngram=3, corpus=want)
        assert [list(i) for i in ids] == want
        check_stats(prompts, want, want, stats, 7, 3)
        assert all(s["passes"] <= n_predict // 2 and s["passes"] + s["accepted"] == n_predict for s in stats), stats
        first = first or (ids, stats)
        assert [list(i) for i in ids] == [list(i) for i in first[0]] and stats == first[1]


def test_no_corpus_random_prompt(q40):
    """the low-acceptance end: nothing to copy but what the model itself repeats"""
    prompts = [prompt_of(12, 1)]
    n_predict = 48
    want = [[int(t) for t in row] for row in q40.generate_greedy_batch(prompts, n_predict)[0]]
    first = None
    for _ in range(2):
        ids, stats, _ = q40.generate_lookup(prompts, n_predict, max_draft=7, max_ngram=3)
        assert [list(i) for i in ids] == want
        check_stats(prompts, None, want, stats, 7, 3)
        first = first or stats
        assert stats == first
