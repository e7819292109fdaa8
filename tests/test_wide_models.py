"""CPU proof that the files of tests/wide_models.py are what they claim and that the oracle can be trusted on them; without it tests/test_gpu_wide.py
could pass on a fixture that had quietly become benign.  The conditions are conditions on the test's INPUT (wide_ref.layer_stats, a float64 restatement of
one layer's input side, itself checked against the oracle's taps), for the prompts the GPU test uses.

Each ingredient's conditions are asserted, unchanged, on that ingredient's own file and on the combined file -- for the 96-token prompt of the prompt pass (chunks
of 8: the visibility of every random-token plan of the GPU test) and for the token sequence of the teacher-forced single-token decode (causal, 0 .. 70 keys)."""
import numpy as np
import pytest

import wide_models as wm
import wide_ref as wr
from modelfile_py import read_model

L = wm.L
F16_TINY = 2.0 ** -24            # the smallest f16 subnormal: the fp16 exp table returns 0 below half of it

# max |logits(ggml mode) - logits(hf mode)| of the oracle over ORACLE_SELF_TOKENS single-token evals, measured on the build machine (deterministic there):
#   plain synthetic f32 file   1.070e-03
#   combined wide f32 file     5.737e-02
# asserted with a margin of 2 x (a different libm on another host; nothing random enters)
ORACLE_SELF_TOKENS = 12
ORACLE_SELF_PLAIN = 1.070e-3
ORACLE_SELF_WIDE = 5.737e-2


@pytest.fixture(scope="module")
def built(pkg, tmp_path_factory):
    d = tmp_path_factory.mktemp("wide_cpu")
    files = wm.build(pkg, d, wm.FILES + ["plain.f32", "peaked.f32"])
    hp, vocab, merges, order, W = wm.load_arrays(files["plain.f32"])
    return dict(files=files, W=W)


@pytest.fixture(scope="module")
def stats(built, oracle):
    """layer_stats of every layer (and the final LayerNorm): which = a file's transformation, for the 96-token prompt of the GPU test's prompt pass fed in chunks
    of 8; which + "/decode": for the 71 tokens of the GPU test's teacher-forced single-token decode of that file in q4_0, each seeing the keys up to itself."""
    memo = {}

    def get(key):
        if key not in memo:
            which, _, run = key.partition("/")
            T = wm.transformed(built["W"], which)
            name = "combined.q4_0" if which in ("combined", "plain") else which + ".q4_0"
            if run == "decode":
                o = oracle.OracleModel(built["files"][name], n_threads=8)
                toks, n_batch = [tok for tok, _, _ in wm.decode_rows(o, wm.seed_of(name, "decode"))], None
            else:
                toks, n_batch = wm.tokens(wm.seed_of(name, "prompt"), 96), 8
            memo[key] = [wr.layer_stats(T, toks, l, n_batch=n_batch) for l in range(L + 1)]
        return memo[key]
    return get


# ---- the conditions, as functions of layer_stats results, so that the plain file can be shown to fail them ----

def peaked_figures(st):
    out = {}
    for l in (0, 1):
        pmax = st[l]["probs"].max(axis=2)
        out[l] = dict(one_hot=float((pmax > 0.999).mean()), mid=float(((pmax > 0.5) & (pmax < 0.99)).mean()),
                      pmin=float(np.where(st[l]["visible"][None], st[l]["probs"], 1.0).min()))
    return out


def peaked_ok(fig):
    return fig[1]["one_hot"] >= 0.5 and fig[0]["mid"] >= 0.05 and fig[0]["pmin"] < F16_TINY and fig[1]["pmin"] < F16_TINY


def gelu_figures(st):
    pre = np.concatenate([st[l]["pre_gelu"].ravel() for l in (0, 1)])
    return dict(lo=float(pre.min()), hi=float(pre.max()), near=float((np.abs(pre) <= 1.0).mean()), finite=bool(np.isfinite(pre.astype(np.float16)).all()),
                patterns=int(wr.f16_patterns(pre).size))


def gelu_ok(fig):
    return fig["lo"] < -8.0 and fig["hi"] > 8.0 and fig["near"] >= 0.10 and fig["finite"] and fig["patterns"] >= 2000


def outlier_figures(st):
    out = []
    for l in range(L + 1):                    # the first LayerNorm of every layer and the final one
        amax, codes = wr.q8_blocks(st[l]["ln0"])
        x = st[l]["ln0"].astype(np.float32).reshape(amax.shape + (32,))
        out.append(dict(zero=int((amax == 0).sum()), lone=int(((codes != 0).sum(axis=2) == 1).sum()),
                        const=int(((x == x[:, :, :1]).all(axis=2) & (x[:, :, 0] != 0)).sum())))
    return out


def outlier_ok(fig):
    return all(f["zero"] >= 1 and f["lone"] >= 1 and f["const"] >= 1 for f in fig)


def test_peaked(stats):
    for key in ("peaked", "combined", "peaked/decode", "combined/decode"):
        fig = peaked_figures(stats(key))
        print(key, "file:", fig)
        assert peaked_ok(fig), key


def test_gelu(stats):
    print("plain synthetic file:", gelu_figures(stats("plain")))
    for key in ("gelu", "combined", "gelu/decode", "combined/decode"):
        fig = gelu_figures(stats(key))
        print(key, "file:", fig)
        assert gelu_ok(fig), key


def test_outlier(stats):
    for which in ("outlier", "combined", "outlier/decode", "combined/decode"):
        fig = outlier_figures(stats(which))
        print(which, "file, Q8 blocks with amax == 0 / one non-zero code / 32 equal non-zero values per LayerNorm:", fig)
        assert outlier_ok(fig)
        h1 = stats(which)[1]["ln1"]
        assert (np.abs(h1[:, wm.OUT_BIAS_CH] - wm.OUT_BIAS) < 10.0).all()      # the bias-50 channel of layer 1's second LayerNorm


def test_plain_synthetic_file_fails_the_conditions(stats):
    """The sanity check of the conditions themselves: on write_synthetic's own output none of them holds."""
    st = stats("plain")
    assert not peaked_ok(peaked_figures(st))
    assert not gelu_ok(gelu_figures(st))
    assert not outlier_ok(outlier_figures(st))
    assert not any(f["zero"] or f["lone"] or f["const"] for f in outlier_figures(st))
    assert peaked_figures(st)[1]["one_hot"] == 0.0 and gelu_figures(st)["hi"] < 8.0


BLOCK_LAYOUT = {2: (18, False), 3: (20, True), 6: (22, False), 7: (24, True), 8: (34, False)}      # type: (bytes, has m)
DEAD = [wm.lname(l, p) for l in range(L) for p in ("self_attn.q_proj.weight", "self_attn.v_proj.weight", "fc1.weight", "fc2.weight")] + ["output_projection.weight"]


@pytest.mark.parametrize("typ", wm.QUANT)
def test_dead_weight_blocks_and_finite_scales(built, typ):
    hp, _, _, tensors = read_model(built["files"]["combined." + typ])
    zero = sub = zero_m = 0
    for t in tensors:
        if t["type"] in (0, 1):
            assert np.isfinite(np.frombuffer(t["raw"], dtype=np.float32 if t["type"] == 0 else np.float16)).all(), t["name"]
            continue
        nbytes, has_m = BLOCK_LAYOUT[t["type"]]
        blk = np.frombuffer(t["raw"], dtype=np.uint8).reshape(-1, nbytes)
        d = blk[:, 0:2].copy().view(np.float16)[:, 0]
        assert np.isfinite(d).all(), t["name"]
        if has_m:
            m = blk[:, 2:4].copy().view(np.float16)[:, 0]
            assert np.isfinite(m).all(), t["name"]
        if t["name"] in DEAD:
            zero += int((d == 0).sum())
            sub += int(((d != 0) & (np.abs(d.astype(np.float32)) < 2.0 ** -14)).sum())
            if has_m:
                zero_m += int(((d == 0) & (m != 0)).sum())
    print("%s: %d blocks with d == 0, %d with an f16-subnormal d, %d with d == 0 and m != 0" % (typ, zero, sub, zero_m))
    assert zero >= 100 and sub >= 8
    if typ in ("q4_1", "q5_1"):
        assert zero_m >= 8


def test_float_and_raw_files_hold_no_nan_or_infinity(built):
    for name in ("combined.f32", "combined.f16", "rawq8", "peaked.q4_0", "gelu.q4_0", "outlier.q4_0", "dead.q4_0"):
        _, _, _, tensors = read_model(built["files"][name])
        for t in tensors:
            if t["type"] in (0, 1):
                assert np.isfinite(np.frombuffer(t["raw"], dtype=np.float32 if t["type"] == 0 else np.float16)).all(), (name, t["name"])
            else:
                blk = np.frombuffer(t["raw"], dtype=np.uint8).reshape(-1, BLOCK_LAYOUT[t["type"]][0])
                assert np.isfinite(blk[:, 0:2].copy().view(np.float16)).all(), (name, t["name"])
    _, _, _, tensors = read_model(built["files"]["rawq8"])
    edited = [t for t in tensors if ".q_proj.weight" in t["name"] or ".fc2.weight" in t["name"]]
    blk = np.concatenate([np.frombuffer(t["raw"], dtype=np.uint8).reshape(-1, 34) for t in edited])
    assert int((blk[:, 2:] == 0x80).all(axis=1).sum()) >= 64 and int((blk[:, 2:] == 0x7F).all(axis=1).sum()) >= 64
    assert int((blk[:, 0:2].copy().view(np.float16)[:, 0] < 0).sum()) >= 64


def test_layer_stats_against_the_oracles_taps(built, oracle):
    """The restatement against OracleModel.tap in "hf" mode (plain float arithmetic, causal) on the wide and the peaked f32 file.  Bound: 1e-4 of the largest
    value of the tap.  float32 carries 6e-8 per operation, a row is a few thousand of them deep (sums of 4096 terms, three layers), which gives 1e-5 at the
    outside; a mistake in the restatement (a scale, a bias, the position offset, the mask) moves values by a sizeable fraction of themselves."""
    for which in ("combined", "peaked"):
        toks = wm.tokens(3, 24)
        st = wr.layer_stats(wm.transformed(built["W"], which), toks, L, hf=True)
        o = oracle.OracleModel(built["files"][which + ".f32"], n_threads=8, mode="hf")
        o.eval(toks, 0)
        for k in range(L + 2):
            ref = o.tap(k - 1).astype(np.float64)
            got = st["taps"][k] if k <= L else st["ln0"]
            d, scale = float(np.abs(got - ref).max()), float(np.abs(ref).max())
            print("%s tap %d: max |diff| %.2e of %.1f" % (which, k - 1, d, scale))
            assert d <= 1e-4 * scale, (which, k)


def test_layer_stats_in_the_mode_the_conditions_use(built, oracle):
    """The branches that produce the asserted conditions -- tanh GELU, eps 1e-5, and both visibility masks -- against the oracle's taps in ggml mode on the wide f32
    file: 24 tokens as three chunks of 8 (no mask inside a chunk; the taps hold the last chunk's rows) and as one causal eval.  Bound: 5e-3 of the tap's largest
    value.  The oracle's two fp16 tables round argument and result to f16 (2^-11 = 4.9e-4 relative each) once per layer and table; ten such steps are allowed
    over three layers, while a wrong mask or GELU moves the rows by a sizeable fraction of themselves.  (eps 1e-5 against 1e-12 is below this bound: it is
    restated from the source, not shown here.)"""
    toks = wm.tokens(3, 24)
    T = wm.transformed(built["W"], "combined")
    for n_batch in (8, None):
        st = wr.layer_stats(T, toks, L, n_batch=n_batch)
        o = oracle.OracleModel(built["files"]["combined.f32"], n_threads=8)
        if n_batch:
            for at in range(0, 24, 8):
                o.eval(toks[at:at + 8], at)
            rows = slice(16, 24)
        else:
            o.set_mode("ggml", n_threads=8, causal=1)
            o.eval(toks, 0)
            rows = slice(0, 24)
        for k in range(L + 2):
            ref = o.tap(k - 1).astype(np.float64)
            got = (st["taps"][k] if k <= L else st["ln0"])[rows]
            d, scale = float(np.abs(got - ref).max()), float(np.abs(ref).max())
            print("ggml mode, n_batch %s, tap %d: max |diff| %.2e of %.1f" % (n_batch, k - 1, d, scale))
            assert d <= 5e-3 * scale, (n_batch, k)


@pytest.mark.parametrize("name", wm.FILES)
def test_oracle_rows_are_finite_with_a_top_two_gap(built, oracle, name):
    """Every row on which the GPU test compares an arg-max: finite, and the two largest logits at least 2e-3 apart -- twice the 1e-3 bar, so two rows within
    the bar of each other cannot disagree about the arg-max."""
    worst, n = np.inf, 0
    for scenario, n_past, row in wm.compared_rows(oracle, name, built["files"][name]):
        assert np.isfinite(row).all(), (name, scenario, n_past)
        gap = wm.top_two_gap(row)
        assert gap >= 2e-3, (name, scenario, n_past, gap)
        worst, n = min(worst, gap), n + 1
    print("%s: %d rows, smallest top-two gap %.4f" % (name, n, worst))
    assert n > 0


def _self_diff(oracle, path):
    a, b = oracle.OracleModel(path, n_threads=8), oracle.OracleModel(path, n_threads=8, mode="hf")
    worst, tok = 0.0, 2
    for n_past in range(ORACLE_SELF_TOKENS):         # single tokens: the causal mask of "hf" mode has nothing to mask
        la, lb = a.eval([tok], n_past), b.eval([tok], n_past)
        assert np.isfinite(la).all() and np.isfinite(lb).all()
        worst = max(worst, float(np.abs(la - lb).max()))
        tok = int(lb.argmax())
    return worst


def test_oracle_against_itself(built, oracle):
    """ggml mode (fp16 GELU / exp tables, tanh GELU, eps 1e-5) against "hf" mode (plain float arithmetic) far from the band: the restatement of the
    reference's tables is not itself wrong there."""
    plain, wide = _self_diff(oracle, built["files"]["plain.f32"]), _self_diff(oracle, built["files"]["combined.f32"])
    print("oracle ggml vs hf, max |diff| over the logits: plain synthetic %.3e, combined wide %.3e" % (plain, wide))
    assert plain <= 2 * ORACLE_SELF_PLAIN and wide <= 2 * ORACLE_SELF_WIDE
