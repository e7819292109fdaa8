"""The float chain: the calls over column states on F32 / F16 files, switched on per context (csrc/kernels_fchain.hip.h).

Three synthetic files.  A has BioGPT-base's widths (1024 / 4096 / 16 heads; 2 layers) with a vocabulary of 2053, as F32 and F16.  B is the smallest file that
takes every path: d_model 192, d_ff 96 (rows of 3 and 6 blocks of 32: one partial staging phase, lanes without a chunk), 3 heads, n_vocab 77, as F32 and F16.
C has BioGPT-Large's widths (1600 / 6400 / 25 heads; 1 layer), as F16.  The F16 files are made as tests/test_gpu_fpipe.py makes its own: the 2-D weights as
float16, ftype 1.

Every comparison is equality.  With float_chain=True the batched calls equal the unchanged single-sequence calls of the same context (score, generate_greedy,
hidden: fdec_kernel / matvec_kernel), which holds the new kernel to the old ones; and they equal the CPU oracle -- target logits bit for bit, arg-max rows,
greedy ids, and the ids (beam: and scores) that tests/sample_ref.py / tests/beam_ref.py compute from the oracle's rows.  The packed column counts 1, 15, 16, 17
and 33 are the issue's; 7, 8 and 9 the borders of the kernel's 8-column tile.  Without the switch the same files are what they were: chain_kind 0 and the
gate's text ("fast chain")."""
import numpy as np
import pytest

import beam_ref
import sample_ref

pytestmark = pytest.mark.gpu

A = dict(n_vocab=2053, n_layer=2, n_head=16, n_positions=96, d_ff=4096, d_model=1024, n_merges=3)
B = dict(n_vocab=77, n_layer=1, n_head=3, n_positions=40, d_ff=96, d_model=192, n_merges=3)
Cc = dict(n_vocab=2053, n_layer=1, n_head=25, n_positions=96, d_ff=6400, d_model=1600, n_merges=3)
KW = {"A": A, "B": B, "C": Cc}
MODELS = [("A", "f32"), ("A", "f16"), ("B", "f32"), ("B", "f16"), ("C", "f16")]
IDS = ["%s-%s" % m for m in MODELS]
SPLITS = {1: (1,), 7: (2, 5), 8: (3, 5), 9: (1, 8), 15: (2, 5, 8), 16: (3, 5, 8), 17: (1, 7, 9), 33: (4, 12, 17)}      # packed columns -> sequence lengths
MARGIN = 1e-9          # sampling: separates the device's exp() rounding from a wrong choice (tests/test_gpu_sample.py)
BEAM_MARGIN = 1e-5     # beam selection (tests/test_gpu_beam.py)
HOT = (40, 0.95, 6.0)


def seq_of(fam, n, seed):
    rng = np.random.default_rng(seed)
    return [2] + [int(v) for v in rng.integers(4, KW[fam]["n_vocab"], n - 1)]


@pytest.fixture(scope="module")
def files(pkg, tmp_path_factory):
    from modelfile_py import read_model, write_model
    d = tmp_path_factory.mktemp("fchain")
    out = {}
    for fam in ("A", "B", "C"):
        f32, f16 = str(d / ("%s_f32.bin" % fam)), str(d / ("%s_f16.bin" % fam))
        pkg.write_synthetic(f32, **KW[fam])
        hp, vocab, merges, tensors = read_model(f32)           # convert.py --use-f16: the 2-D "*.weight" tensors as float16, ftype 1
        for t in tensors:
            if len(t["ne"]) == 2 and t["name"].endswith(".weight") and t["type"] == 0:
                t["raw"] = np.frombuffer(t["raw"], dtype=np.float32).astype(np.float16).tobytes()
                t["type"] = 1
        write_model(f16, dict(hp, ftype=1), vocab, merges, tensors)
        out[(fam, "f32")], out[(fam, "f16")] = f32, f16
    return out


@pytest.fixture(scope="module")
def models(pkg, files):
    """One context per file for the whole module, the float chain switched on, loaded when first asked for."""
    ms = {}

    def get(fam, name):
        if (fam, name) not in ms:
            ms[(fam, name)] = pkg.BiogptModel.load(files[(fam, name)], float_chain=True)
        return ms[(fam, name)]
    yield get
    for m in ms.values():
        m.close()


def causal_oracle(oracle, path):
    o = oracle.OracleModel(path, n_threads=16)
    o.set_mode("ggml", n_threads=16, causal=1)
    return o


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- 1. score_batch: the context's own score(), and the causal oracle ----

@pytest.mark.parametrize("fam,name", MODELS, ids=IDS)
def test_score_batch_equals_score_and_the_oracle(oracle, files, models, fam, name):
    g = models(fam, name)
    o = causal_oracle(oracle, files[(fam, name)])
    before = g.float_launches()
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
    assert g.chain_kind() == 3 and g.float_launches() > before
    o.close()


# ---- 2. greedy decoding of 1, 3 and 17 prompts ----

@pytest.mark.parametrize("fam,name", MODELS, ids=IDS)
def test_greedy_batch_equals_greedy_and_the_oracle(oracle, files, models, fam, name):
    g = models(fam, name)
    n_predict = 6
    lens = (5, 9, 3, 12, 7, 4, 10, 6, 8, 11, 2, 13, 5, 9, 3, 7, 12)
    prompts = [seq_of(fam, n, 300 + i) for i, n in enumerate(lens)]
    o = oracle.OracleModel(files[(fam, name)], n_threads=16)
    alone = []
    for p in prompts:
        ids, _ = g.generate_greedy(p, n_predict)
        ref, _ = o.generate_greedy(p, n_predict)
        assert list(ids) == list(ref), (fam, name, p)
        alone.append([int(t) for t in ids])
    o.close()
    before = g.float_launches()
    for n in (1, 3, 17):
        got, _ = g.generate_greedy_batch(prompts[:n], n_predict)
        assert [[int(t) for t in s] for s in got] == alone[:n], (fam, name, n)
    assert g.float_launches() > before


# ---- 3. sampled generation against the reference loop on the oracle's rows ----

@pytest.mark.parametrize("fam,name", MODELS, ids=IDS)
def test_sample_against_the_oracle_loop(oracle, files, models, fam, name):
    top_k, top_p, temp = HOT
    prompts = [seq_of(fam, 5, 11), seq_of(fam, 13, 12)]
    seeds = [101, 202, 303, 404]          # sequence r = prompt r // 2, sample r % 2
    n_predict = 10
    want = []
    for r, seed in enumerate(seeds):
        o = oracle.OracleModel(files[(fam, name)], n_threads=16)
        ids, margin = sample_ref.reference_loop(o, prompts[r // 2], 8, n_predict, top_k, top_p, temp, seed)
        o.close()
        print("%s %s sequence %d: smallest margin %.3g, %d distinct ids" % (fam, name, r, margin, len(set(ids))))
        assert margin >= MARGIN, "fixture problem: a decision of sequence %d lies %.3g from a border" % (r, margin)
        want.append(ids)
    g = models(fam, name)
    got, _ = g.generate_sample(prompts, n_predict, n_samples=2, top_k=top_k, top_p=top_p, temp=temp, seeds=seeds, eos_id=-1, n_batch=8)
    assert [[int(t) for t in s] for s in got] == want, (fam, name)


# ---- 4. beam search over a batch against the restatement on the oracle's rows ----

@pytest.mark.parametrize("fam,name", MODELS, ids=IDS)
def test_beam_batch_against_the_restatement(oracle, files, models, fam, name):
    n_beams, n_predict = 3, 6
    prompts = [seq_of(fam, 7, 21), seq_of(fam, 12, 22), seq_of(fam, 4, 23)]
    g = models(fam, name)
    got, _ = g.generate_beam_batch(prompts, n_predict, n_beams=n_beams, eos_id=-1, length_penalty=1.0, early_stopping=True, n_batch=8)
    assert len(got) == len(prompts)
    for p, prompt in enumerate(prompts):
        o = oracle.OracleModel(files[(fam, name)], n_threads=16)
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
        one, _ = g.generate_beam(prompt, n_predict, n_beams=n_beams, eos_id=-1, length_penalty=1.0, early_stopping=True, n_batch=8)
        assert [([int(t) for t in i], float(np.float32(s))) for i, s in one] == [([int(t) for t in i], float(np.float32(s))) for i, s in got[p]], (fam, name, p)


# ---- 5. the queue equals generate_sample of each request alone ----

@pytest.mark.parametrize("fam,name", MODELS, ids=IDS)
def test_queue_equals_each_request_alone(models, fam, name):
    top_k, top_p, temp = HOT
    g = models(fam, name)
    lens, predicts, seeds = (5, 9, 14, 3, 11, 7), [1, 9, 4, 7, 2, 6], [301, 302, 303, 304, 305, 306]
    prompts = [seq_of(fam, n, 400 + n) for n in lens]
    want = []
    for r in range(len(prompts)):
        ids, _ = g.generate_sample([prompts[r]], predicts[r], top_k=top_k, top_p=top_p, temp=temp, seeds=[seeds[r]], eos_id=-1, n_batch=8)
        want.append([int(t) for t in ids[0]])
    assert [len(w) for w in want] == predicts
    for max_columns in (2, 4):
        ids, info, _ = g.generate_queue(prompts, max(predicts), max_columns=max_columns, group=2, top_k=top_k, top_p=top_p, temp=temp, seeds=seeds, eos_id=-1,
                                        n_batch=8, n_predicts=predicts)
        assert [[int(t) for t in s] for s in ids] == want, (fam, name, max_columns)


# ---- 6. embed_batch equals hidden of each sequence ----

@pytest.mark.parametrize("fam,name", MODELS, ids=IDS)
def test_embed_batch_equals_hidden(models, fam, name):
    g = models(fam, name)
    seqs = [seq_of(fam, n, 500 + n) for n in (1, 7, 9, 16)]       # 33 packed columns
    got = g.embed_batch(seqs, layer=-1, pooling="none")
    for s, seq in enumerate(seqs):
        assert got[s].shape == (len(seq), KW[fam]["d_model"])
        assert (bits(got[s]) == bits(g.hidden(seq))).all(), (fam, name, s)


# ---- 7. score_continuations equals score_batch of the concatenations ----

@pytest.mark.parametrize("fam,name", MODELS, ids=IDS)
def test_continuations_equal_score_batch_of_the_concatenations(models, fam, name):
    g = models(fam, name)
    prefix = seq_of(fam, 11, 600)
    conts = [seq_of(fam, n, 610 + n)[1:] for n in (2, 6, 4, 9)]       # 1, 5, 3 and 8 tokens
    got = g.score_continuations(prefix, conts)
    n = len(prefix)
    for c, cont in enumerate(conts):
        tg = [-1] * (n - 1) + list(cont) + [-1]
        lp, am, lg = g.score_batch([prefix + cont], [tg])[0]
        sl = slice(n - 1, n - 1 + len(cont))
        assert (bits(got[c][0]) == bits(lp[sl])).all() and (got[c][1] == am[sl]).all() and (bits(got[c][2]) == bits(lg[sl])).all(), (fam, name, c)


# ---- 8. the switch ----

@pytest.mark.parametrize("name", ("f32", "f16"))
def test_without_the_switch_the_file_is_what_it_was(pkg, files, name):
    """chain_kind 0 and the gate's text; switched on and off again, the same; and the context's own passes are untouched by the switch."""
    seqs = [seq_of("A", 5, 1), seq_of("A", 9, 2)]
    off = pkg.BiogptModel.load(files[("A", name)])
    on = pkg.BiogptModel.load(files[("A", name)], float_chain=True)
    assert off.chain_kind() == 0 and off.float_launches() == 0 and on.chain_kind() == 3
    for call in (lambda: off.score_batch(seqs), lambda: off.generate_greedy_batch(seqs, 4), lambda: off.embed_batch(seqs), lambda: off.generate_sample(seqs, 4)):
        with pytest.raises(pkg.BiogptError, match="fast chain"):
            call()
    for seq in seqs:      # two contexts of one file, the switch on and off: equal score rows
        a, b = on.score(seq), off.score(seq)
        assert all((bits(x) == bits(y)).all() for x, y in zip(a, b))
    assert on.float_launches() == 0 and off.float_launches() == 0
    want = on.score_batch(seqs)
    off.float_chain(True)
    assert off.chain_kind() == 3
    got = off.score_batch(seqs)
    assert all((bits(x) == bits(y)).all() for s in range(len(seqs)) for x, y in zip(got[s], want[s]))
    off.float_chain(False)
    assert off.chain_kind() == 0
    with pytest.raises(pkg.BiogptError, match="fast chain"):
        off.score_batch(seqs)
    off.close()
    on.close()


def test_switching_on_fails_with_its_reason(pkg, tiny_models, files, tmp_path_factory):
    g = pkg.BiogptModel.load(tiny_models["f16"])
    with pytest.raises(pkg.BiogptError, match="head size is not 64"):
        g.float_chain(True)
    assert g.chain_kind() == 0
    g.close()
    with pytest.raises(pkg.BiogptError, match="head size is not 64"):
        pkg.BiogptModel.load(tiny_models["f16"], float_chain=True)
    q40 = str(tmp_path_factory.mktemp("fchain_q") / "q4_0.bin")
    pkg.quantize_file(files[("A", "f32")], q40, "q4_0")
    g = pkg.BiogptModel.load(q40)
    with pytest.raises(pkg.BiogptError, match="block-quantized"):
        g.float_chain(True)
    assert g.chain_kind() == 1 and g.float_launches() == 0
    g.float_chain(False)      # (off is what every file is)
    g.close()


def test_calls_the_float_chain_does_not_serve_say_so_by_name(pkg, models):
    """these stay with BioGPT-base block-quantized files; each refusal names its call."""
    g = models("B", "f16")
    seqs = [seq_of("B", 5, 1), seq_of("B", 9, 2)]
    trie = pkg.Trie.build([[5, 6, 7], [5, 8]], B["n_vocab"])
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
        assert "float fast chain" in str(e.value), str(e.value)
    trie.close()
    assert g.chain_kind() == 3
