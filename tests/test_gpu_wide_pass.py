"""The wide pass layer (csrc/kernels_wpass.hip.h): evals of 9 or more tokens of block-quantized files that are not BioGPT-base, whole calls, bit
for bit against the CPU oracle (scalar association): logits rows and K / V rows as uint32.  Files A and B are tests/test_gpu_wide_decode.py's (A: rows of 6
and 5 blocks, 1100 positions; B: BioGPT-Large's widths in one layer, 64 positions).  `wide_pass_launches` says which evals ran the new kernels: seven launches
per layer, two more for a pass that wants every row."""
import numpy as np
import pytest

from test_gpu_wide_chunk import load_pair, plan_of
from test_gpu_wide_decode import A, IDS, KW, MODELS, bits, files, same_kv, toks_of, walk      # noqa: F401 (files: the fixture)

pytestmark = pytest.mark.gpu

# tokens per eval, one behind another.  A: the smallest pass, a full tile, one column over a tile, one over a two-tile wave, the column count at which the
# attention launch changes form, with single tokens and a chunk between them; B: 9, 17 and 33 within its 64 positions
PLANS = {"A": (9, 1, 16, 5, 17, 33, 1, 80), "B": (9, 1, 17, 4, 33)}


def passes_in(plan):
    return sum(1 for toks, n_past in plan if len(toks) >= 9 and n_past + len(toks) <= 1024)


@pytest.mark.parametrize("fam,name", MODELS, ids=IDS)
def test_passes_equal_the_oracle_on_and_off(pkg, oracle, files, fam, name):
    sizes = PLANS[fam]
    plan = plan_of(toks_of(fam, sum(sizes), 37), sizes)
    L = KW[fam]["n_layer"]
    for on in (True, False):
        g, o = load_pair(pkg, oracle, files, fam, name, wide_decode=True, wide_chunk=True, wide_pass=on)
        try:
            assert g.wide_pass is on and g.wide_pass_launches() == 0
            singles = walk(g, o, plan, (fam, name, on))
            same_kv(g, o, fam, sum(sizes), (fam, name, on))
            assert g.wide_pass_launches() == (7 * L * passes_in(plan) if on else 0)
            assert g.wide_decode_launches() == 5 * L * singles
            assert g.wide_chunk_launches() == 7 * L * sum(1 for toks, _ in plan if 2 <= len(toks) <= 8)
        finally:
            g.close(); o.close()


@pytest.mark.parametrize("name", ("q4_1", "q8_0"))
def test_key_border(pkg, oracle, files, name):
    """A pass of 16 whose last key is 1024 runs the layer; one that ends at 1032 keeps the generic route and leaves the counter still."""
    t = toks_of("A", 1040, 41)
    g, o = load_pair(pkg, oracle, files, "A", name, wide_pass=True)
    try:
        walk(g, o, [(t[:1008], 0)], ("A", name, "prefix"))      # (1008 columns: one pass of the layer itself)
        before = g.wide_pass_launches()
        assert before == 7 * A["n_layer"]
        walk(g, o, [(t[1008:1024], 1008)], ("A", name, "keys", 1024))
        assert g.wide_pass_launches() == before + 7 * A["n_layer"]
        walk(g, o, [(t[1016:1032], 1016)], ("A", name, "keys", 1032))
        assert g.wide_pass_launches() == before + 7 * A["n_layer"]
        same_kv(g, o, "A", 1032, ("A", name, "keys"))
    finally:
        g.close(); o.close()


@pytest.mark.parametrize("name", ("q4_0", "q5_1"))
def test_every_row_calls(pkg, oracle, files, name):
    """eval_all of 33 tokens (no mask inside the eval) against the oracle's rows of the same eval.  score and hidden of 33 tokens (row i sees tokens 0 .. i)
    against the oracle's per-token rows: the target's logit bit for bit, the arg-max, every K / V row the pass wrote, and the log-probability against the
    float64 log-softmax of the oracle's row (1e-4: an f32 log-sum-exp over 613 logits of magnitude below 100 is good to a few units of 1e-5).  The oracle has no
    score and no bit-exact final LayerNorm row: the log-probabilities and hidden rows are also the switch-off route's, bit for bit.  Two stage launches more per
    pass that wants every row, none for hidden."""
    t = toks_of("A", 34, 43)
    tgt = np.asarray(t[1:34])
    L = A["n_layer"]
    g, o = load_pair(pkg, oracle, files, "A", name, wide_pass=True)
    off = pkg.BiogptModel.load(files[("A", name)], wide_pass=False)
    try:
        rows = g.eval_all(t[:33], 0)
        assert (bits(rows) == bits(o.eval(t[:33], 0, all_rows=True))).all()
        assert g.wide_pass_launches() == 7 * L + 2
        ref = np.stack([o.eval([t[i]], i) for i in range(33)])
        lp, am, tl = g.score(t[:33], 0, targets=tgt)
        assert g.wide_pass_launches() == 2 * (7 * L + 2)
        same_kv(g, o, "A", 33, ("A", name, "score"))
        assert (bits(tl) == bits(ref[np.arange(33), tgt])).all() and list(am) == [int(np.lexsort((np.arange(r.size), -r))[0]) for r in ref]
        r64 = ref.astype(np.float64)
        lse = np.log(np.exp(r64 - r64.max(axis=1, keepdims=True)).sum(axis=1)) + r64.max(axis=1)
        assert np.abs(lp - (r64[np.arange(33), tgt] - lse)).max() < 1e-4
        assert (bits(lp) == bits(off.score(t[:33], 0, targets=tgt)[0])).all()
        hid = g.hidden(t[1:34], 0)
        assert g.wide_pass_launches() == 2 * (7 * L + 2) + 7 * L
        for i in range(33):
            o.eval([t[1 + i]], i)
        same_kv(g, o, "A", 33, ("A", name, "hidden"))
        assert (bits(hid) == bits(off.hidden(t[1:34], 0))).all() and off.wide_pass_launches() == 0
    finally:
        g.close(); o.close(); off.close()


@pytest.mark.parametrize("name", ("q4_0", "q5_1"))
def test_generate_greedy(pkg, oracle, files, name):
    """A 20-token prompt travels as one pass of 20 columns: the ids are the oracle's, the pass counter moves by seven launches per layer, the chunk counter stays."""
    g, o = load_pair(pkg, oracle, files, "A", name, wide_pass=True)
    try:
        prompt = toks_of("A", 20, 31)
        ids, _ = g.generate_greedy(prompt, 12)
        ref, _ = o.generate_greedy(prompt, 12)
        assert list(ids) == list(ref)
        assert g.wide_pass_launches() == 7 * A["n_layer"] and g.wide_chunk_launches() == 0
    finally:
        g.close(); o.close()


def test_untouched_contexts(pkg, files, tmp_path):
    # a BioGPT-base file: not served, the counter stays 0
    f32, q40 = str(tmp_path / "base_f32.bin"), str(tmp_path / "base_q4_0.bin")
    pkg.write_synthetic(f32, n_vocab=512, n_layer=1, n_head=16, n_positions=32, d_ff=4096, d_model=1024, n_merges=3)
    pkg.quantize_file(f32, q40, "q4_0")
    g = pkg.BiogptModel.load(q40)
    try:
        assert g.set_wide_pass(True) is False and g.wide_pass is False
        g.eval(list(range(2, 14)), 0); g.eval_all(list(range(2, 12)), 12)
        assert g.wide_pass_launches() == 0
    finally:
        g.close()
    # a float file: "not served"
    g = pkg.BiogptModel.load(files[("A", "f32")])
    try:
        assert g.set_wide_pass(True) is False and "not served" in pkg._err() and g.wide_pass is False
    finally:
        g.close()
    # the SIMD association keeps its launches and its bits
    t = toks_of("A", 40, 19)
    rows = []
    for on in (False, True):
        g = pkg.BiogptModel.load(files[("A", "q4_0")], assoc="simd", wide_pass=on)
        try:
            rows.append([g.eval(t[:9], 0), g.eval(t[9:26], 9), g.eval_all(t[26:40], 26)])
            assert g.wide_pass_launches() == 0
        finally:
            g.close()
    assert all((bits(a) == bits(b)).all() for a, b in zip(*rows))
