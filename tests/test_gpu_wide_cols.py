"""The wide column layer in the engine (biogpt_hip_wide_cols; csrc/kernels_wcols.hip.h): the batched calls of a wide file at 1 .. 16 columns with
the switch on against the same build with it off, against the single-sequence calls and against the CPU oracle -- every comparison is equality -- and the launch
counter that says which kernels ran.  The files are tests/test_gpu_wide_chain.py's: B (d_model 192 = 3 blocks, d_ff 96, n_vocab 77) in all five formats, and A
(BioGPT-Large's widths, n_vocab 2053: a partial last round and a zero-padded lm_head tile) in one."""
import numpy as np
import pytest

from test_gpu_long_context import TOKS, W
from test_gpu_wide_chain import A, B, B_TYPES, HOT, KW, seq_of

pytestmark = pytest.mark.gpu

MODELS = [("B", t) for t in B_TYPES] + [("A", "q5_1")]
LENS = (5, 9, 3, 12, 7, 4, 10, 6, 8, 11, 2, 13, 5, 9, 3, 7)


@pytest.fixture(scope="module")
def files(pkg, tmp_path_factory):
    d = tmp_path_factory.mktemp("wide_cols")
    out = {}
    for fam, kw in (("A", A), ("B", B), ("W", W)):
        f32 = str(d / ("%s_f32.bin" % fam))
        pkg.write_synthetic(f32, **kw)
        for name in sorted({t for f, t in MODELS if f == fam} | ({"q4_0"} if fam == "W" else set())):
            out[(fam, name)] = str(d / ("%s_%s.bin" % (fam, name)))
            pkg.quantize_file(f32, out[(fam, name)], name)
    return out


@pytest.fixture
def pair(pkg, files, request):
    """(switch on, switch off) contexts of the test's file"""
    fam, name = request.param
    on, off = pkg.BiogptModel.load(files[(fam, name)], wide_cols=True), pkg.BiogptModel.load(files[(fam, name)], wide_cols=False)
    assert on.wide_cols is True and off.wide_cols is False and on.wide_cols_launches() == 0
    yield fam, name, on, off
    assert off.wide_cols_launches() == 0
    on.close(); off.close()


def rows(ids):
    return [[int(t) for t in s] for s in ids]


@pytest.mark.parametrize("pair", MODELS, indirect=True, ids=["%s-%s" % m for m in MODELS])
def test_greedy_batch_equals_greedy_and_the_oracle(oracle, files, pair):
    fam, name, on, off = pair
    prompts = [seq_of(fam, n, 300 + i) for i, n in enumerate(LENS)]
    o = oracle.OracleModel(files[(fam, name)], n_threads=16)
    alone = []
    for p in prompts:
        alone.append(rows([on.generate_greedy(p, 6)[0]])[0])
        assert alone[-1] == [int(t) for t in o.generate_greedy(p, 6)[0]], (fam, name, p)
    o.close()
    assert on.wide_cols_launches() == 0      # (the context's own columns are not the layer's)
    for n in (3, 16):
        before = on.wide_cols_launches()
        assert rows(on.generate_greedy_batch(prompts[:n], 6)[0]) == alone[:n], (fam, name, n)
        assert on.wide_cols_launches() > before and rows(off.generate_greedy_batch(prompts[:n], 6)[0]) == alone[:n]
    # 17 sequences of two tokens: one packed prompt pass of 34 columns and steps of 17 -- none of them the layer's
    before, wide = on.wide_cols_launches(), on.wide_launches()
    many = [seq_of(fam, 2, 700 + i) for i in range(17)]
    assert rows(on.generate_greedy_batch(many, 4)[0]) == rows(off.generate_greedy_batch(many, 4)[0])
    assert on.wide_cols_launches() == before and on.wide_launches() > wide


@pytest.mark.parametrize("pair", MODELS, indirect=True, ids=["%s-%s" % m for m in MODELS])
def test_beam_and_sample_do_not_depend_on_the_switch(pair):
    fam, name, on, off = pair
    prompts = [seq_of(fam, 7, 21), seq_of(fam, 12, 22), seq_of(fam, 4, 23)]
    beams = [g.generate_beam_batch(prompts, 6, n_beams=5, eos_id=-1, length_penalty=1.0, early_stopping=True, n_batch=8)[0] for g in (on, off)]
    flat = [[([int(t) for t in i], int(np.float32(s).view(np.uint32))) for i, s in hyp] for hyp in beams[0]]
    assert flat == [[([int(t) for t in i], int(np.float32(s).view(np.uint32))) for i, s in hyp] for hyp in beams[1]] and all(len(h) == 5 for h in flat)
    one = on.generate_beam(prompts[0], 6, n_beams=5, eos_id=-1, length_penalty=1.0, early_stopping=True, n_batch=8)[0]      # five columns
    assert [([int(t) for t in i], int(np.float32(s).view(np.uint32))) for i, s in one] == flat[0]
    top_k, top_p, temp = HOT
    kw = dict(n_samples=2, top_k=top_k, top_p=top_p, temp=temp, seeds=[101, 202, 303, 404], eos_id=-1, n_batch=8)
    before = on.wide_cols_launches()
    a, b = on.generate_sample(prompts[:2], 10, **kw)[0], off.generate_sample(prompts[:2], 10, **kw)[0]
    assert rows(a) == rows(b) and [len(s) for s in a] == [10] * 4 and on.wide_cols_launches() > before


def test_two_column_steps_beyond_1024_keys(pkg, files):
    on, off = pkg.BiogptModel.load(files[("W", "q4_0")], wide_cols=True), pkg.BiogptModel.load(files[("W", "q4_0")], wide_cols=False)
    try:
        prompts = [TOKS[:1015], TOKS[50:650]]
        a, b = on.generate_greedy_batch(prompts, 24)[0], off.generate_greedy_batch(prompts, 24)[0]
        assert rows(a) == rows(b) and on.wide_cols_launches() > 0 and off.wide_cols_launches() == 0
        assert on.long_cols_launches() == off.long_cols_launches() > 0      # (the attention beyond 1024 keys is the wide chain's, switch or no switch)
    finally:
        on.close(); off.close()


def test_files_the_wide_chain_does_not_serve_are_refused_by_name(pkg, tmp_path):
    f32, q = str(tmp_path / "f32.bin"), str(tmp_path / "q4_0.bin")
    pkg.write_synthetic(f32, n_vocab=2048, n_layer=1, n_head=16, n_positions=96, d_ff=4096, d_model=1024, n_merges=3)
    pkg.quantize_file(f32, q, "q4_0")
    for path, why in ((f32, "not block-quantized"), (q, "BioGPT-base shapes")):
        g = pkg.BiogptModel.load(path)
        assert g.set_wide_cols(True) is False and "not served" in pkg._err() and why in pkg._err() and g.wide_cols is False
        g.close()
