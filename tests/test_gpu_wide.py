"""The fast chain at BioGPT-base widths on model files OFF the operating point of write_synthetic (tests/wide_models.py: peaked attention, pre-GELU values
over the table's whole range, LayerNorm outlier / zero / constant blocks, dead and degenerate weight blocks, and a Q8_0 file with codes and scales no
quantizer emits).  tests/test_wide_models.py proves on the CPU that the files are what they claim, that the oracle is finite on them and that every row
compared here has a top-two gap of at least twice the 1e-3 bar.  Every comparison: finite, max |diff| <= 1e-3, arg-max equal, and -- for block-quantized
files, on the paths DESIGN 4.1 / 4.3 / 4.4 state to be bit-identical to the oracle -- equal bit for bit (asserted here; the synthetic-file tests report it).

Which attention kernel a test reaches: single tokens up to 256 keys run the attention stage of dec_xpipe_kernel (persistent launch) or dec_attn_kernel (five-launch
layer); single tokens at 257 .. 512 keys run dec_xpipe_kernel with two workgroups per head by default and the key-range helpers of kernels_xlong.hip.h with
BIOGPT_HIP_XPIPE_DUAL=0 (both are run here); chunks of 2 .. 8 tokens run the attention of kernels_xcols.hip.h; passes of fewer than 80 columns (the 96-token
prompt in passes of 64 + 32, the 19-token eval) run the per-column pass attention, and only the 700-token pass (512 + 188 columns) runs attn_tile_kernel.
Every test that names a path asserts that the path was taken (the prompt passes: biogpt_hip_mfma_launches counts the four linear stages of every layer)."""
import numpy as np
import pytest

import wide_models as wm
from wide_models import KW

pytestmark = pytest.mark.gpu

ATOL = 1e-3          # the contract's bar on logits
KV_ATOL = 1e-4       # K / V rows, as test_gpu_parity
COMBINED = ["combined." + t for t in wm.QUANT] + ["rawq8"]
SINGLE = [w + ".q4_0" for w in wm.INGREDIENTS]
L, P, D = KW["n_layer"], KW["n_positions"], KW["d_model"]


@pytest.fixture(scope="module")
def files(pkg, tmp_path_factory):
    return wm.build(pkg, tmp_path_factory.mktemp("wide"), wm.FILES)


def _load(pkg, path, monkeypatch, **env):
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))      # options are read when the context is created
    g = pkg.BiogptModel.load(path)
    for k in env:
        monkeypatch.delenv(k)
    return g


class Tally:
    def __init__(self, what, exact):
        self.what, self.exact, self.worst, self.rows, self.same = what, exact, 0.0, 0, 0

    def row(self, got, ref, at):
        d = float(np.abs(got - ref).max())
        self.worst, self.rows, self.same = max(self.worst, d), self.rows + 1, self.same + int((got == ref).all())
        assert np.isfinite(got).all(), "%s at %s: output not finite" % (self.what, at)
        assert d <= ATOL, "%s at %s: max |diff| %.3e" % (self.what, at, d)
        assert int(got.argmax()) == int(ref.argmax()), "%s at %s: arg-max %d, oracle %d" % (self.what, at, got.argmax(), ref.argmax())
        if self.exact:
            assert (got == ref).all(), "%s at %s: not bit-identical to the oracle, max |diff| %.3e in %d elements" % (self.what, at, d, int((got != ref).sum()))

    def done(self):
        print("%s: %d rows, worst |diff| %.2e, %d bit-identical" % (self.what, self.rows, self.worst, self.same))


def _kv_rows(g, o, n_keys, what):
    for which in (0, 1):
        ref = o.kv(which)
        for l in range(L):
            got = g.read_kv(which, l * P * D, n_keys * D).reshape(n_keys, D)
            d = float(np.abs(got - ref[l, :n_keys]).max())
            assert np.isfinite(got).all() and d <= KV_ATOL, "%s: %s rows of layer %d differ by %.3e" % (what, "KV"[which], l, d)


# ---- 1. single-token decode, 0 .. 70 keys, through the persistent launch and through the five-launch layer ----

@pytest.mark.parametrize("name", COMBINED + SINGLE)
def test_single_token_decode(pkg, oracle, files, monkeypatch, name):
    gp = pkg.BiogptModel.load(files[name])
    gf = _load(pkg, files[name], monkeypatch, BIOGPT_HIP_XPIPE=0, BIOGPT_HIP_RESIDENT=0)
    try:
        assert gp.xpipe_state() == 1 and gf.xpipe_state() != 1
        o = oracle.OracleModel(files[name], n_threads=16)
        tp, tf = Tally(name + " persistent launch", True), Tally(name + " five-launch layer", True)
        for tok, n_past, lo in wm.decode_rows(o, wm.seed_of(name, "decode")):
            tp.row(gp.eval([tok], n_past), lo, n_past)
            tf.row(gf.eval([tok], n_past), lo, n_past)
        tp.done(); tf.done()
        _kv_rows(gp, o, 71, name + " persistent launch")
        _kv_rows(gf, o, 71, name + " five-launch layer")
        assert gp.xpipe_state() == 1, "the persistent launch was abandoned on the way"
    finally:
        gp.close(); gf.close()


# ---- 2. + 4. chunks of 8 on both sides of 256 keys, one eval of 19 tokens, single tokens beyond 300 keys ----

def _walk(g, o, plan, t):
    for toks, n_past, compared in plan:
        lo = o.eval(toks, n_past)
        if compared:
            t.row(g.eval(toks, n_past), lo, (n_past, len(toks)))
        else:
            g.eval_device(toks, n_past)
    t.done()


@pytest.mark.parametrize("name", COMBINED)
def test_chunks_and_long_context_decode(pkg, oracle, files, name):
    g = pkg.BiogptModel.load(files[name])
    try:
        assert g.xpipe_state() == 1
        o = oracle.OracleModel(files[name], n_threads=16)
        plan = wm.chunk_plan(wm.seed_of(name, "chunks"))
        _walk(g, o, plan, Tally(name + " chunks", True))
        _kv_rows(g, o, 327, name + " chunks")
        assert g.chunk_launches() == sum(1 for toks, _, _ in plan if 2 <= len(toks) <= 8), "a chunk left the column-per-XCD launch"
        assert g.xpipe_state() == 1
    finally:
        g.close()


@pytest.mark.parametrize("name", COMBINED)
def test_long_context_decode_with_key_range_helpers(pkg, oracle, files, monkeypatch, name):
    """Single tokens at 301 .. 304 keys through kernels_xlong.hip.h (BIOGPT_HIP_XPIPE_DUAL=0, resident launch and all)."""
    g = _load(pkg, files[name], monkeypatch, BIOGPT_HIP_XPIPE_DUAL=0)
    try:
        assert g.xpipe_state() == 1
        o = oracle.OracleModel(files[name], n_threads=16)
        _walk(g, o, wm.long_plan(wm.seed_of(name, "long")), Tally(name + " key-range helpers", True))
        _kv_rows(g, o, 304, name + " key-range helpers")
        assert g.xpipe_state() == 1
    finally:
        g.close()


# ---- 3. the prompt pass on the matrix cores ----

@pytest.mark.parametrize("name", COMBINED + SINGLE)
def test_prompt_pass_on_the_matrix_cores(pkg, oracle, files, monkeypatch, name):
    g = _load(pkg, files[name], monkeypatch, BIOGPT_HIP_PROMPT_COLS=64)      # passes of 64 + 32 columns
    try:
        o = oracle.OracleModel(files[name], n_threads=16)
        toks = wm.tokens(wm.seed_of(name, "prompt"), 96)
        lo = wm.prompt_row(o, toks)
        t = Tally(name + " prompt pass", True)
        t.row(g.eval_prompt(toks, 0, 8), lo, 96)
        t.done()
        _kv_rows(g, o, 96, name + " prompt pass")
        assert g.mfma_launches() == 4 * L, "the 64-column pass left the matrix cores (or the 32-column pass reached them): %d launches there" % g.mfma_launches()
    finally:
        g.close()


def test_prompt_pass_beyond_the_attention_ring(pkg, oracle, files):
    """700 tokens in passes of 512 + 188 columns: attn_tile_kernel, past the 640 keys that its ring holds."""
    name = "combined.q4_0"
    g = pkg.BiogptModel.load(files[name])
    try:
        o = oracle.OracleModel(files[name], n_threads=16)
        toks = wm.tokens(wm.seed_of(name, "prompt700"), 700)
        lo = wm.prompt_row(o, toks)
        t = Tally(name + " 700-token prompt pass", True)
        t.row(g.eval_prompt(toks, 0, 8), lo, 700)
        t.done()
        _kv_rows(g, o, 700, name + " 700-token prompt pass")
        assert g.mfma_launches() == 2 * 4 * L, "a pass left the matrix cores: %d launches there" % g.mfma_launches()
    finally:
        g.close()


# ---- 5. float files: the streaming launch below 224 keys, the five-launch float layer beyond, an 8-token chunk ----

@pytest.mark.parametrize("name", wm.FLOAT_FILES)
def test_float_files(pkg, oracle, files, name):
    """Bit-identity is reported, not asserted, on float files (the bar is 1e-3 there)."""
    g = pkg.BiogptModel.load(files[name])
    try:
        o = oracle.OracleModel(files[name], n_threads=16)
        plan = wm.float_plan(wm.seed_of(name, "floats"))
        _walk(g, o, plan, Tally(name + " float paths", False))
        _kv_rows(g, o, 233, name + " float paths")
        below = sum(1 for toks, n_past, _ in plan if len(toks) == 1 and n_past < 224)
        assert g.fpipe_launches() == below, "single tokens below 224 keys: %d, through the streaming launch: %d" % (below, g.fpipe_launches())
    finally:
        g.close()


# ---- 6. hidden(): the final LayerNorm over rows (ln_rows_kernel<1024>) meets the outlier, zero and constant blocks ----

@pytest.mark.parametrize("name", COMBINED + wm.FLOAT_FILES + ["outlier.q4_0"])
def test_final_layernorm_rows(pkg, oracle, files, name):
    toks = wm.tokens(106, 40)
    g = pkg.BiogptModel.load(files[name])
    try:
        got = g.hidden(toks)
    finally:
        g.close()
    o = oracle.OracleModel(files[name], n_threads=16)
    o.set_mode("ggml", n_threads=16, causal=1)
    o.eval(toks, 0)
    ref = o.tap(L)
    d = float(np.abs(got.astype(np.float64) - ref).max())
    print("%s hidden(): max |diff| %.2e, largest |value| %.1f, %d/%d elements bit-identical" % (name, d, float(np.abs(ref).max()), int((got == ref).sum()), got.size))
    assert got.shape == ref.shape and np.isfinite(got).all() and d <= ATOL
    z = slice(32 * wm.OUT_ZERO_BLOCK, 32 * wm.OUT_ZERO_BLOCK + 32)
    c = slice(32 * wm.OUT_CONST_BLOCK, 32 * wm.OUT_CONST_BLOCK + 32)
    assert (got[:, z] == 0.0).all() and (got[:, c] == np.float32(0.3)).all()      # gain 0: the bias itself, whatever the row
