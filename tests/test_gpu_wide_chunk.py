"""The wide chunk layer (csrc/kernels_wchunk.hip.h): evals of 2 .. 8 tokens of block-quantized files that are not BioGPT-base, whole calls, bit
for bit against the CPU oracle (scalar association): logits rows and K / V rows as uint32.  Files A and B are tests/test_gpu_wide_decode.py's (A: rows of 6
and 5 blocks, 1100 positions; B: BioGPT-Large's widths in one layer).  `wide_chunk_launches` says which evals ran the new kernels: seven launches per layer."""
import numpy as np
import pytest

from test_gpu_wide_decode import A, IDS, KW, MODELS, bits, files, same_kv, toks_of, walk      # noqa: F401 (files: the fixture)

pytestmark = pytest.mark.gpu

PLANS = {"mixed": (2, 1, 3, 4, 11, 5, 1, 6, 7, 8), "loop": (8, 8, 8, 6)}      # tokens per eval, one behind another; loop: the reference's, 30 tokens in chunks of 8


def plan_of(toks, sizes, n_past=0):
    plan = []
    for n in sizes:
        plan.append((toks[n_past:n_past + n], n_past))
        n_past += n
    return plan


def chunks_in(plan):
    return sum(1 for toks, n_past in plan if 2 <= len(toks) <= 8 and n_past + len(toks) <= 1024)


def load_pair(pkg, oracle, files, fam, name, **kw):
    return pkg.BiogptModel.load(files[(fam, name)], **kw), oracle.OracleModel(files[(fam, name)], n_threads=16)


@pytest.mark.parametrize("sizes", PLANS.values(), ids=PLANS.keys())
@pytest.mark.parametrize("fam,name", MODELS, ids=IDS)
def test_chunks_equal_the_oracle_on_and_off(pkg, oracle, files, fam, name, sizes):
    plan = plan_of(toks_of(fam, sum(sizes), 23), sizes)
    L = KW[fam]["n_layer"]
    for on in (True, False):
        g, o = load_pair(pkg, oracle, files, fam, name, wide_decode=True, wide_chunk=on)
        try:
            assert g.wide_chunk is on and g.wide_chunk_launches() == 0
            singles = walk(g, o, plan, (fam, name, on))
            same_kv(g, o, fam, sum(sizes), (fam, name, on))
            assert g.wide_chunk_launches() == (7 * L * chunks_in(plan) if on else 0)
            assert g.wide_decode_launches() == 5 * L * singles
        finally:
            g.close(); o.close()


@pytest.mark.parametrize("name", ("q4_1", "q8_0"))
def test_key_borders(pkg, oracle, files, name):
    """A chunk of 8 whose last key is on either side of every key count at which the attention launch changes form, the last that still has 1024 keys, and one
    beyond: that one keeps the generic route and leaves the counter still."""
    t = toks_of("A", 1040, 29)
    g, o = load_pair(pkg, oracle, files, "A", name, wide_chunk=True)
    try:
        at = 0
        for last in (64, 65, 128, 129, 256, 257, 1024, 1032):
            plan = ([(t[at:last - 8], at)] if at < last - 8 else []) + [(t[last - 8:last], last - 8)]
            before = g.wide_chunk_launches()
            walk(g, o, plan, ("A", name, "keys", last))
            assert g.wide_chunk_launches() == before + 7 * A["n_layer"] * chunks_in(plan), last
            at = last
        assert chunks_in(plan) == 0
        same_kv(g, o, "A", 1032, ("A", name, "keys"))
    finally:
        g.close(); o.close()


@pytest.mark.parametrize("name", ("q4_0", "q5_1"))
def test_generate_greedy(pkg, oracle, files, name):
    """A 20-token prompt travels as one pass of 20 columns (generic); a 7-token prompt is one chunk.  The ids are the oracle's either way."""
    g, o = load_pair(pkg, oracle, files, "A", name, wide_chunk=True)
    try:
        for n_prompt, chunks in ((20, 0), (7, 1)):
            prompt = toks_of("A", n_prompt, 31)
            before = g.wide_chunk_launches()
            ids, _ = g.generate_greedy(prompt, 12)
            ref, _ = o.generate_greedy(prompt, 12)
            assert list(ids) == list(ref), n_prompt
            assert g.wide_chunk_launches() == before + 7 * A["n_layer"] * chunks, n_prompt
    finally:
        g.close(); o.close()


def test_untouched_contexts(pkg, files, tmp_path):
    # a BioGPT-base file: not served, the counter stays 0
    f32, q40 = str(tmp_path / "base_f32.bin"), str(tmp_path / "base_q4_0.bin")
    pkg.write_synthetic(f32, n_vocab=512, n_layer=1, n_head=16, n_positions=32, d_ff=4096, d_model=1024, n_merges=3)
    pkg.quantize_file(f32, q40, "q4_0")
    g = pkg.BiogptModel.load(q40)
    try:
        assert g.set_wide_chunk(True) is False and g.wide_chunk is False
        g.eval([2, 5, 9], 0); g.eval([7, 8], 3)
        assert g.wide_chunk_launches() == 0
    finally:
        g.close()
    # a float file: "not served"
    g = pkg.BiogptModel.load(files[("A", "f32")])
    try:
        assert g.set_wide_chunk(True) is False and "not served" in pkg._err() and g.wide_chunk is False
    finally:
        g.close()
    # the SIMD association keeps its launches and its bits
    t = toks_of("A", 16, 19)
    rows = []
    for on in (False, True):
        g = pkg.BiogptModel.load(files[("A", "q4_0")], assoc="simd", wide_chunk=on)
        try:
            rows.append([g.eval(t[:5], 0), g.eval(t[5:13], 5), g.eval(t[13:15], 13)])
            assert g.wide_chunk_launches() == 0
        finally:
            g.close()
    assert all((bits(a) == bits(b)).all() for a, b in zip(*rows))
