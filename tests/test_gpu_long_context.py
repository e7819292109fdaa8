"""The long-context attention behind its switch (biogpt_hip_long_context; csrc/kernels_attn_long.hip.h): whole calls on a tiny wide file with a
2048-row position table, bit for bit against the CPU oracle (scalar association) -- logits rows and the K / V rows written, as uint32 -- with the switch on
and off, and the launch counters that say which route an eval took.  Beyond 1024 keys: on, the wide pass / chunk / decode layers serve the eval and its
attention is one launch of the new kernels per layer; off, today's route (the generic kernels for passes and chunks, attn_kernel + a quantize launch inside
the wide decode layer) and the new counter stays 0."""
import numpy as np
import pytest

from test_gpu_wide_decode import bits

pytestmark = pytest.mark.gpu

W = dict(n_vocab=613, n_layer=2, n_head=3, n_positions=2048, d_ff=160, d_model=192, n_merges=3)
L = W["n_layer"]
TYPES = ("q4_0", "q5_1", "q8_0")
# tokens per eval, one behind another: the fill to 1016 keys; a pass of 16 ending at 1032, a chunk of 8 ending at 1040, the tokens at keys 1041 and 1042; a
# pass of 972 (the tile kernel: 80 columns or more) ending at 2014; a pass of 33 ending at 2047; the token at key 2048
SIZES = (1016, 16, 8, 1, 1, 972, 33, 1)
TOKS = [2] + [int(v) for v in np.random.default_rng(51).integers(4, W["n_vocab"], 2047)]


def plan():
    out, n_past = [], 0
    for n in SIZES:
        out.append((TOKS[n_past:n_past + n], n_past))
        n_past += n
    return out


@pytest.fixture(scope="module")
def files(pkg, tmp_path_factory):
    d = tmp_path_factory.mktemp("long_context")
    out = {"f32": str(d / "w_f32.bin"), "base_f32": str(d / "base_f32.bin"), "base": str(d / "base_q4_0.bin")}
    pkg.write_synthetic(out["f32"], **W)
    for name in TYPES:
        out[name] = str(d / ("w_%s.bin" % name))
        pkg.quantize_file(out["f32"], out[name], name)
    pkg.write_synthetic(out["base_f32"], n_vocab=512, n_layer=1, n_head=16, n_positions=1040, d_ff=4096, d_model=1024, n_merges=3)
    pkg.quantize_file(out["base_f32"], out["base"], "q4_0")
    return out


_ref = {}


def reference(oracle, files, name):
    """The oracle's row of every eval of the plan and its K / V rows, once per file (shared by the switch-on and the switch-off walk; never modified)."""
    if name not in _ref:
        o = oracle.OracleModel(files[name], n_threads=16)
        try:
            rows = [o.eval(toks, n_past).copy() for toks, n_past in plan()]
            _ref[name] = (rows, [o.kv(0).copy(), o.kv(1).copy()])
        finally:
            o.close()
    return _ref[name]


@pytest.mark.parametrize("on", (True, False), ids=("on", "off"))
@pytest.mark.parametrize("name", TYPES)
def test_walk_equals_the_oracle(pkg, oracle, files, name, on):
    rows, kv = reference(oracle, files, name)
    g = pkg.BiogptModel.load(files[name], wide_decode=True, wide_chunk=True, wide_pass=True, long_context=on)
    try:
        assert g.long_context is on and g.long_attn_launches() == 0
        for (toks, n_past), ref in zip(plan(), rows):
            got = g.eval(toks, n_past)
            assert (bits(got) == bits(ref)).all(), (name, on, n_past, len(toks), "max |diff| %.3g" % float(np.abs(got - ref).max()))
        P, D = W["n_positions"], W["d_model"]
        for which in (0, 1):
            for l in range(L):
                got = g.read_kv(which, l * P * D, P * D).reshape(P, D)
                assert (bits(got) == bits(kv[which][l, :P])).all(), (name, on, "KV"[which], l)
        beyond = [n for n, (toks, n_past) in zip(SIZES, plan()) if n_past + n > 1024]
        assert g.long_attn_launches() == (L * len(beyond) if on else 0)
        assert g.wide_pass_launches() == 7 * L * (1 + (sum(1 for n in beyond if n >= 9) if on else 0))
        assert g.wide_chunk_launches() == (7 * L * sum(1 for n in beyond if 2 <= n <= 8) if on else 0)
        assert g.wide_decode_launches() == 5 * L * sum(1 for n in SIZES if n == 1)      # (the layer serves single tokens at every key count; off, with attn_kernel inside)
    finally:
        g.close()


@pytest.mark.parametrize("which", ("base", "f32"))
def test_files_that_are_not_served_ignore_the_switch(pkg, files, which):
    """A BioGPT-base-width file and an F32 file: the switch stays off ("not served"), the counter 0, and a pass that crosses 1024 keys has the bits it had."""
    toks = TOKS[:1032] if which == "base" else TOKS[:1040]
    toks = [2] + [4 + t % 500 for t in toks[1:]]
    g, off = pkg.BiogptModel.load(files[which]), pkg.BiogptModel.load(files[which])
    try:
        assert g.set_long_context(True) is False and "not served" in pkg._err() and g.long_context is False
        for m in (g, off):
            m.eval(toks[:1016], 0)
        assert (bits(g.eval(toks[1016:1032], 1016)) == bits(off.eval(toks[1016:1032], 1016))).all()
        assert g.long_attn_launches() == 0
    finally:
        g.close(); off.close()


def test_score_and_generate_cross_1024_keys(pkg, files):
    on, off = pkg.BiogptModel.load(files["q5_1"], long_context=True), pkg.BiogptModel.load(files["q5_1"], long_context=False)
    try:
        a, b = on.score(TOKS[:1100]), off.score(TOKS[:1100])
        assert (bits(a) == bits(b)).all()
        assert on.long_attn_launches() == L and off.long_attn_launches() == 0
        ia, ib = on.generate_greedy(TOKS[:1015], 24)[0], off.generate_greedy(TOKS[:1015], 24)[0]
        assert list(ia) == list(ib) and len(ia) == 24
        assert on.long_attn_launches() > L and off.long_attn_launches() == 0
    finally:
        on.close(); off.close()
