"""The SIMD chain: the calls over column states of a context in the SIMD association, switched on per context (biogpt_hip_assoc_chain; csrc/kernels_schain.hip.h;
DESIGN.md 4.7).

Three synthetic files, quantized with quantize_file.  "tiny" is the tiny file of tests/test_gpu_assoc.py (d_model 128, d_ff 256, 2 heads, 1 layer: rows of 4 and
8 blocks) in all five block formats.  "base" has BioGPT-base's widths (1024 / 4096 / 16 heads; 2 layers) with a vocabulary of 2053 (odd: the lm_head's last row
tile is partial), as Q4_0 and Q5_1.  "large" has BioGPT-Large's widths (1600 / 6400 / 25 heads; 1 layer: K = 1600 is one K phase of the stage and a partial
one, K = 6400 seven), as Q8_0.

Every comparison is equality.  Loaded with assoc="simd", assoc_chain=True the batched calls equal the unchanged single-sequence calls of the same context in
mode 1 (score, generate_greedy, hidden: matvec_simd_kernel / attn_simd_kernel), which holds the new kernels to the old ones; and they equal the oracle with
assoc = 3 -- target logits bit for bit, arg-max rows, greedy ids, and the ids (beam: and scores) that tests/sample_ref.py / tests/beam_ref.py compute from the
SIMD oracle's rows.  Without the chain's switch the same context refuses with the SIMD association's text; in mode 0 the switch changes nothing."""
import numpy as np
import pytest

import beam_ref
import embed_ref
import sample_ref

pytestmark = pytest.mark.gpu

TINY = dict(n_vocab=256, n_layer=1, n_head=2, n_positions=384, d_ff=256, d_model=128, n_merges=16)      # (tests/test_gpu_assoc.py's)
BASE = dict(n_vocab=2053, n_layer=2, n_head=16, n_positions=96, d_ff=4096, d_model=1024, n_merges=3)
LARGE = dict(n_vocab=2053, n_layer=1, n_head=25, n_positions=96, d_ff=6400, d_model=1600, n_merges=3)
KW = {"tiny": TINY, "base": BASE, "large": LARGE}
MODELS = [("tiny", "q4_0"), ("tiny", "q4_1"), ("tiny", "q5_0"), ("tiny", "q5_1"), ("tiny", "q8_0"), ("base", "q4_0"), ("base", "q5_1"), ("large", "q8_0")]
IDS = ["%s-%s" % m for m in MODELS]
SPLITS = {1: (1,), 7: (2, 5), 8: (3, 5), 9: (1, 8), 15: (2, 5, 8), 16: (3, 5, 8), 17: (1, 7, 9), 33: (4, 12, 17)}      # packed columns -> sequence lengths
MARGIN = 1e-9          # sampling: separates the device's exp() rounding from a wrong choice (tests/test_gpu_sample.py)
BEAM_MARGIN = 1e-5     # beam selection (tests/test_gpu_beam.py)
HOT = (40, 0.95, 6.0)
SIMD_TEXT = "which the SIMD association does not serve"      # the refusal of a context in mode 1 without the chain, as tests/test_gpu_assoc.py pins it


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def seq_of(fam, n, seed):
    rng = np.random.default_rng(seed)
    return [2] + [int(v) for v in rng.integers(4, KW[fam]["n_vocab"], n - 1)]


@pytest.fixture(scope="module")
def files(pkg, tmp_path_factory):
    d = tmp_path_factory.mktemp("schain")
    out = {}
    for fam in KW:
        f32 = str(d / ("%s_f32.bin" % fam))
        pkg.write_synthetic(f32, **KW[fam])
        out[(fam, "f32")] = f32
        for f, name in MODELS:
            if f == fam:
                out[(fam, name)] = str(d / ("%s_%s.bin" % (fam, name)))
                pkg.quantize_file(f32, out[(fam, name)], name)
    return out


@pytest.fixture(scope="module")
def models(pkg, files):
    """One context per file for the whole module, in the SIMD association with the SIMD chain switched on, loaded when first asked for."""
    ms = {}

    def get(fam, name):
        if (fam, name) not in ms:
            ms[(fam, name)] = pkg.BiogptModel.load(files[(fam, name)], assoc="simd", assoc_chain=True)
        return ms[(fam, name)]
    yield get
    for m in ms.values():
        m.close()


def simd_oracle(oracle, path, causal=None):
    o = oracle.OracleModel(path, n_threads=16, assoc=3)
    if causal is not None:
        o.set_mode("ggml", 16, causal=causal)
    return o


class Grew:
    """chain_kind() is 4 and the stage counter grew inside the block."""

    def __init__(self, g):
        self.g = g

    def __enter__(self):
        self.before = self.g.simd_chain_launches()
        return self

    def __exit__(self, *exc):
        if exc[0] is None:
            assert self.g.chain_kind() == 4 and self.g.assoc == "simd" and self.g.assoc_chain
            assert self.g.simd_chain_launches() > self.before
        return False


# ---- 1. score_batch: the context's own score(), and the causal SIMD oracle ----

@pytest.mark.parametrize("fam,name", MODELS, ids=IDS)
def test_score_batch_equals_score_and_the_oracle(oracle, files, models, fam, name):
    g = models(fam, name)
    o = simd_oracle(oracle, files[(fam, name)], causal=1)
    with Grew(g):
        for total, lens in SPLITS.items():
            seqs = [seq_of(fam, n, 100 * total + i) for i, n in enumerate(lens)]
            got = g.score_batch(seqs)
            assert len(got) == len(seqs)
            for s, seq in enumerate(seqs):
                lp, am, lg = got[s]
                lp1, am1, lg1 = g.score(seq)
                what = (fam, name, total, s)
                assert (bits(lp) == bits(lp1)).all() and (am == am1).all() and (bits(lg) == bits(lg1)).all(), what
                ref = o.eval(seq, 0, all_rows=True)
                assert (am == ref.argmax(axis=1)).all(), what
                if len(seq) > 1:
                    rows = np.arange(len(seq) - 1)
                    want = np.ascontiguousarray(ref[rows, seq[1:]], dtype=np.float32)
                    print(what, "target logits: max |diff| %.3g" % float(np.abs(lg[:-1] - want).max()))
                    assert (bits(lg[:-1]) == bits(want)).all(), what
    o.close()


# ---- 2. greedy decoding of 1, 3 and 17 prompts ----

@pytest.mark.parametrize("fam,name", MODELS, ids=IDS)
def test_greedy_batch_equals_greedy_and_the_oracle(oracle, files, models, fam, name):
    g = models(fam, name)
    n_predict = 6
    lens = (5, 9, 3, 12, 7, 4, 10, 6, 8, 11, 2, 13, 5, 9, 3, 7, 12)
    prompts = [seq_of(fam, n, 300 + i) for i, n in enumerate(lens)]
    if fam == "tiny":
        prompts.append(seq_of(fam, 30, 399))      # 30 tokens + 6 new ones: the steps cross 32 keys
    o = simd_oracle(oracle, files[(fam, name)])
    alone = []
    before = g.simd_chain_launches()
    for p in prompts:
        ids, _ = g.generate_greedy(p, n_predict)
        ref, _ = o.generate_greedy(p, n_predict)
        assert list(ids) == list(ref), (fam, name, p)
        alone.append([int(t) for t in ids])
    o.close()
    assert g.simd_chain_launches() == before      # (the context's own passes are not the chain's)
    with Grew(g):
        for n in (1, 3, 17):
            got, _ = g.generate_greedy_batch(prompts[:n], n_predict)
            assert [[int(t) for t in s] for s in got] == alone[:n], (fam, name, n)
        if fam == "tiny":
            got, _ = g.generate_greedy_batch(prompts[16:], n_predict)
            assert [[int(t) for t in s] for s in got] == alone[16:], (fam, name, "across 32 keys")


# ---- 3. sampled generation against the reference loop on the SIMD oracle's rows ----

@pytest.mark.parametrize("fam,name", MODELS, ids=IDS)
def test_sample_against_the_oracle_loop(oracle, files, models, fam, name):
    top_k, top_p, temp = HOT
    prompts = [seq_of(fam, 5, 11), seq_of(fam, 13, 12)]
    seeds = [101, 202, 303, 404]          # sequence r = prompt r // 2, sample r % 2
    n_predict = 10
    want = []
    for r, seed in enumerate(seeds):
        o = simd_oracle(oracle, files[(fam, name)])
        ids, margin = sample_ref.reference_loop(o, prompts[r // 2], 8, n_predict, top_k, top_p, temp, seed)
        o.close()
        print("%s %s sequence %d: smallest margin %.3g, %d distinct ids" % (fam, name, r, margin, len(set(ids))))
        assert margin >= MARGIN, "fixture problem: a decision of sequence %d lies %.3g from a border" % (r, margin)
        want.append(ids)
    g = models(fam, name)
    with Grew(g):
        got, _ = g.generate_sample(prompts, n_predict, n_samples=2, top_k=top_k, top_p=top_p, temp=temp, seeds=seeds, eos_id=-1, n_batch=8)
    assert [[int(t) for t in s] for s in got] == want, (fam, name)


# ---- 4. beam search, alone and over a batch, against the restatement on the SIMD oracle's rows ----

@pytest.mark.parametrize("fam,name", MODELS, ids=IDS)
def test_beam_batch_against_the_restatement(oracle, files, models, fam, name):
    n_beams, n_predict = 3, 6
    prompts = [seq_of(fam, 7, 21), seq_of(fam, 12, 22), seq_of(fam, 4, 23)]
    g = models(fam, name)
    with Grew(g):
        got, _ = g.generate_beam_batch(prompts, n_predict, n_beams=n_beams, eos_id=-1, length_penalty=1.0, early_stopping=True, n_batch=8)
    assert len(got) == len(prompts)
    for p, prompt in enumerate(prompts):
        o = simd_oracle(oracle, files[(fam, name)])
        want, margins = beam_ref.beam_search(beam_ref.OracleLogprobs(o, prompt, 8), n_beams, n_predict, -1, 1.0, True)
        o.close()
        small = [(k + 1, m) for k, m in enumerate(margins) if m < BEAM_MARGIN]
        assert not small, "fixture problem: selection margins below %g at steps %s of prompt %d" % (BEAM_MARGIN, small, p)
        assert len(got[p]) == len(want) == n_beams
        for r, ((ids_w, s_w), (ids_g, s_g)) in enumerate(zip(want, got[p])):
            assert [int(t) for t in ids_g] == [int(t) for t in ids_w], (fam, name, p, r)
            # the restatement's score is a float64 sum of float64 log-softmax rows; the engine's an f32 sum of its f32 rows: n_predict roundings of values below 2^4
            assert abs(float(s_g) - float(s_w)) <= 1e-4, (fam, name, p, r, float(s_g), float(s_w))
        # and the f32 scores are those of the single call, bit for bit
        with Grew(g):
            one, _ = g.generate_beam(prompt, n_predict, n_beams=n_beams, eos_id=-1, length_penalty=1.0, early_stopping=True, n_batch=8)
        assert [([int(t) for t in i], float(np.float32(s))) for i, s in one] == [([int(t) for t in i], float(np.float32(s))) for i, s in got[p]], (fam, name, p)


# ---- 5. the plain queue equals generate_sample(top_k = 1) of each request alone ----

@pytest.mark.parametrize("fam,name", MODELS, ids=IDS)
def test_queue_equals_each_request_alone(models, fam, name):
    g = models(fam, name)
    lens, predicts, seeds = (5, 9, 14, 3, 11), [1, 9, 4, 7, 2], [301, 302, 303, 304, 305]
    prompts = [seq_of(fam, n, 400 + n) for n in lens]
    want = []
    for r in range(len(prompts)):
        ids, _ = g.generate_sample([prompts[r]], predicts[r], top_k=1, top_p=1.0, temp=1.0, seeds=[seeds[r]], eos_id=-1, n_batch=8)
        want.append([int(t) for t in ids[0]])
    assert [len(w) for w in want] == predicts
    with Grew(g):
        ids, info, _ = g.generate_queue(prompts, max(predicts), max_columns=2, group=2, top_k=1, top_p=1.0, temp=1.0, seeds=seeds, eos_id=-1, n_batch=8,
                                        n_predicts=predicts)
    assert [[int(t) for t in s] for s in ids] == want, (fam, name)


# ---- 6. embed_batch equals hidden of each sequence ----

@pytest.mark.parametrize("fam,name", MODELS, ids=IDS)
def test_embed_batch_equals_hidden(models, fam, name):
    g = models(fam, name)
    seqs = [seq_of(fam, n, 500 + n) for n in (1, 7, 9, 16)]       # 33 packed columns
    with Grew(g):
        got = g.embed_batch(seqs, layer=-1, pooling="none")
    for s, seq in enumerate(seqs):
        assert got[s].shape == (len(seq), KW[fam]["d_model"])
        assert (bits(got[s]) == bits(g.hidden(seq))).all(), (fam, name, s)
    with Grew(g):
        last, mean = g.embed_batch(seqs, layer=-1, pooling="last"), g.embed_batch(seqs, layer=-1, pooling="mean")
    for s, seq in enumerate(seqs):      # hidden() pooled on the host: the last row as it is; the mean within embed_ref's bound for a double sum rounded once
        rows = g.hidden(seq)
        assert (bits(last[s]) == bits(rows[-1])).all(), (fam, name, s)
        assert (np.abs(np.asarray(mean[s], dtype=np.float64) - embed_ref.pool(rows, "mean")) <= embed_ref.mean_bound(rows)).all(), (fam, name, s)


# ---- 7. score_continuations equals score_batch of the concatenations ----

@pytest.mark.parametrize("fam,name", MODELS, ids=IDS)
def test_continuations_equal_score_batch_of_the_concatenations(models, fam, name):
    g = models(fam, name)
    prefix = seq_of(fam, 17, 600)
    conts = [seq_of(fam, n, 610 + n)[1:] for n in (2, 6, 9)]       # 1, 5 and 8 tokens
    with Grew(g):
        got = g.score_continuations(prefix, conts)
    n = len(prefix)
    for c, cont in enumerate(conts):
        tg = [-1] * (n - 1) + list(cont) + [-1]
        lp, am, lg = g.score_batch([prefix + cont], [tg])[0]
        sl = slice(n - 1, n - 1 + len(cont))
        assert (bits(got[c][0]) == bits(lp[sl])).all() and (got[c][1] == am[sl]).all() and (bits(got[c][2]) == bits(lg[sl])).all(), (fam, name, c)


# ---- 8. the switch ----

def test_without_the_chain_mode_1_refuses_as_before(pkg, files):
    """The same context with and without the chain's switch; switching it drops nothing the context's own passes need."""
    seqs = [seq_of("tiny", 5, 1), seq_of("tiny", 9, 2)]
    g = pkg.BiogptModel.load(files[("tiny", "q4_1")], assoc="simd")
    assert g.chain_kind() == 0 and not g.assoc_chain and g.simd_chain_launches() == 0
    own = g.score(seqs[1])
    for call in (lambda: g.score_batch(seqs), lambda: g.generate_greedy_batch(seqs, 4), lambda: g.embed_batch(seqs), lambda: g.generate_sample(seqs, 4),
                 lambda: g.generate_beam(seqs[0], 4, n_beams=2), lambda: g.score_continuations(seqs[0], [seqs[1]]), lambda: g.generate_queue(seqs, 4)):
        with pytest.raises(pkg.BiogptError, match=SIMD_TEXT):
            call()
    assert g.simd_chain_launches() == 0
    g.set_assoc_chain(True)
    assert g.chain_kind() == 4 and g.assoc_chain
    got = g.score_batch(seqs)
    assert all((bits(x) == bits(y)).all() for x, y in zip(got[1], own))
    assert all((bits(x) == bits(y)).all() for x, y in zip(g.score(seqs[1]), own))
    g.set_assoc_chain(False)
    assert g.chain_kind() == 0
    with pytest.raises(pkg.BiogptError, match=SIMD_TEXT):
        g.score_batch(seqs)
    g.close()


def test_calls_the_simd_chain_does_not_serve_say_so_by_name(pkg, models):
    g = models("tiny", "q4_0")
    seqs = [seq_of("tiny", 5, 1), seq_of("tiny", 9, 2)]
    trie = pkg.Trie.build([[5, 6, 7], [5, 8]], TINY["n_vocab"])
    before = g.simd_chain_launches()
    for call, text in ((lambda: g.generate_contrastive(seqs, 4), "contrastive search needs the BioGPT-base fast chain"),
                       (lambda: g.generate_lookup(seqs, 4), "prompt-lookup decoding needs the BioGPT-base fast chain"),
                       (lambda: g.generate_sample(seqs, 4, repetition_penalty=1.3), "sampled generation under rules needs the BioGPT-base fast chain"),
                       (lambda: g.generate_beam_batch(seqs, 4, n_beams=2, no_repeat_ngram_size=2), "beam search under rules needs the BioGPT-base fast chain"),
                       (lambda: g.generate_sample(seqs, 4, trie=trie, eos_id=2), "trie-constrained sampling needs the BioGPT-base fast chain"),
                       (lambda: g.generate_beam_batch(seqs, 4, n_beams=2, trie=trie), "trie-constrained beam search needs the BioGPT-base fast chain"),
                       (lambda: g.generate_sample(seqs, 4, sampler=pkg.sampler(top_k=0)), "whole-vocabulary sampling needs the BioGPT-base fast chain"),
                       (lambda: g.generate_greedy_batch(seqs, 4, prefix=[2, 7, 9]), "generation behind a shared prefix needs the BioGPT-base fast chain"),
                       (lambda: g.generate_sample(seqs, 4, prefix=[2, 7, 9]), "sampled generation behind a shared prefix needs the BioGPT-base fast chain"),
                       (lambda: g.generate_greedy_batch(seqs, 4, logprobs=2), "generation with log-probabilities needs the BioGPT-base fast chain"),
                       (lambda: g.generate_sample(seqs, 4, logprobs=2), "sampled generation with log-probabilities needs the BioGPT-base fast chain"),
                       (lambda: g.generate_queue(seqs, 4, prefix=[2, 7, 9]), "generation over a queue behind a shared prefix needs the BioGPT-base fast chain"),
                       (lambda: g.generate_queue(seqs, 4, logprobs=2), "generation over a queue with log-probabilities needs the BioGPT-base fast chain"),
                       (lambda: g.generate_queue(seqs, 4, params=[pkg.request_params(), pkg.request_params()]), "needs the BioGPT-base fast chain"),
                       (lambda: g.queue_session(max_columns=4), "a queue session needs the BioGPT-base fast chain"),
                       (lambda: g.generate_beam_queue(seqs, 4, n_beams=2, max_columns=4), "beam search over a queue needs the BioGPT-base fast chain"),
                       (lambda: g.score_continuations_batch([seqs[0]], [[[5, 6], [7]]]), "shared-prefix scoring of many prompts needs the BioGPT-base fast chain")):
        with pytest.raises(pkg.BiogptError, match=text) as e:
            call()
        assert "SIMD chain" in str(e.value), str(e.value)
    trie.close()
    assert g.chain_kind() == 4 and g.simd_chain_launches() == before      # refused before any launch


@pytest.mark.parametrize("fam,name", [("tiny", "q5_1"), ("base", "q4_0")], ids=["tiny-q5_1", "base-q4_0"])
def test_in_mode_0_the_switch_changes_nothing(pkg, files, fam, name):
    seqs = [seq_of(fam, 5, 1), seq_of(fam, 9, 2), seq_of(fam, 17, 3)]
    fresh = pkg.BiogptModel.load(files[(fam, name)])      # a context that never switches
    kind0 = fresh.chain_kind()
    want0 = fresh.score_batch(seqs)
    ids0, _ = fresh.generate_greedy_batch(seqs, 5)
    assert fresh.simd_chain_launches() == 0 and not fresh.assoc_chain
    fresh.close()
    g = pkg.BiogptModel.load(files[(fam, name)], assoc="simd", assoc_chain=True)
    want1 = g.score_batch(seqs)
    assert any((bits(x) != bits(y)).any() for s in range(len(seqs)) for x, y in zip(want1[s], want0[s])), "the two associations give the same rows"
    g.set_assoc("scalar")
    assert g.assoc == "scalar" and g.assoc_chain and g.chain_kind() == kind0
    n = g.simd_chain_launches()
    got0 = g.score_batch(seqs)
    assert all((bits(x) == bits(y)).all() for s in range(len(seqs)) for x, y in zip(got0[s], want0[s]))
    ids, _ = g.generate_greedy_batch(seqs, 5)
    assert [[int(t) for t in s] for s in ids] == [[int(t) for t in s] for s in ids0]
    assert g.simd_chain_launches() == n
    g.set_assoc("simd")
    assert g.chain_kind() == 4
    got1 = g.score_batch(seqs)
    assert all((bits(x) == bits(y)).all() for s in range(len(seqs)) for x, y in zip(got1[s], want1[s]))
    assert g.simd_chain_launches() > n
    g.close()


def test_float_files_and_open_sessions_refuse_the_switch(pkg, files):
    f = pkg.BiogptModel.load(files[("tiny", "f32")])
    with pytest.raises(pkg.BiogptError, match="F32"):
        f.set_assoc_chain(True)
    assert not f.assoc_chain and f.chain_kind() == 0
    f.set_assoc_chain(False)      # (off is what every file is)
    with pytest.raises(pkg.BiogptError, match="F32"):
        pkg.BiogptModel.load(files[("tiny", "f32")], assoc_chain=True)
    f.close()
    g = pkg.BiogptModel.load(files[("base", "q4_0")])      # (a queue session is the BioGPT-base chain's)
    with g.queue_session(max_columns=2, group=2, n_predict=4):
        with pytest.raises(pkg.BiogptError, match="queue session is open"):
            g.set_assoc_chain(True)
    g.set_assoc_chain(True)
    assert g.assoc_chain and g.assoc == "scalar" and g.chain_kind() == 1
    g.close()


def test_environment_default(pkg, files, monkeypatch):
    monkeypatch.setenv("BIOGPT_HIP_ASSOC_CHAIN", "1")
    g, f = pkg.BiogptModel.load(files[("tiny", "q8_0")]), pkg.BiogptModel.load(files[("tiny", "f32")])
    assert g.assoc_chain and g.assoc == "scalar" and not f.assoc_chain      # (the default holds where the file can have it; the association is its own switch)
    g.set_assoc("simd")
    assert g.chain_kind() == 4
    g.close(); f.close()
