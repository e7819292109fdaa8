"""The wide decode layer (csrc/kernels_wdecode.hip.h): single-token steps of block-quantized files that are not BioGPT-base, whole calls, bit
for bit against the CPU oracle (scalar association).  File A (d_model 192, d_ff 160, 3 heads, n_vocab 613, 2 layers) has rows of 6 and 5 blocks, an odd
vocabulary and row counts no workgroup share divides; file B has BioGPT-Large's widths (1600 / 6400 / 25 heads) in one layer.  Neither is a base shape, so
with the switch on every single token runs the new kernels, and `wide_decode_launches` says so.  File A has 1100 positions, so that the key borders
reach beyond the 1024 keys up to which the generic attention launch writes out_proj's Q8 blocks itself.  Logits rows and K / V rows are compared as uint32."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

A = dict(n_vocab=613, n_layer=2, n_head=3, n_positions=1100, d_ff=160, d_model=192, n_merges=3)
B = dict(n_vocab=1029, n_layer=1, n_head=25, n_positions=64, d_ff=6400, d_model=1600, n_merges=3)
KW = {"A": A, "B": B}
TYPES = {"A": ("q4_0", "q4_1", "q5_0", "q5_1", "q8_0"), "B": ("q4_0", "q5_1", "q8_0")}
MODELS = [(f, t) for f in ("A", "B") for t in TYPES[f]]
IDS = ["%s-%s" % m for m in MODELS]


def toks_of(fam, n, seed):
    return [2] + [int(v) for v in np.random.default_rng(seed).integers(4, KW[fam]["n_vocab"], n - 1)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def files(pkg, tmp_path_factory):
    d = tmp_path_factory.mktemp("wide_decode")
    out = {}
    for fam in KW:
        f32 = str(d / ("%s_f32.bin" % fam))
        pkg.write_synthetic(f32, **KW[fam])
        out[(fam, "f32")] = f32
        for name in TYPES[fam]:
            out[(fam, name)] = str(d / ("%s_%s.bin" % (fam, name)))
            pkg.quantize_file(f32, out[(fam, name)], name)
    return out


def same_kv(g, o, fam, n_keys, what):
    L, P, D = KW[fam]["n_layer"], KW[fam]["n_positions"], KW[fam]["d_model"]
    for which in (0, 1):
        ref = o.kv(which)
        for l in range(L):
            got = g.read_kv(which, l * P * D, n_keys * D).reshape(n_keys, D)
            assert (bits(got) == bits(ref[l, :n_keys])).all(), (what, "KV"[which], l)


def walk(g, o, plan, what):
    """plan: (tokens, n_past) evals; every row equals the oracle's.  Returns the number of single-token evals."""
    for toks, n_past in plan:
        got, ref = g.eval(toks, n_past), o.eval(toks, n_past)
        assert (bits(got) == bits(ref)).all(), (what, n_past, len(toks), "max |diff| %.3g" % float(np.abs(got - ref).max()))
    return sum(1 for toks, _ in plan if len(toks) == 1)


@pytest.mark.parametrize("fam,name", MODELS, ids=IDS)
def test_decode_equals_the_oracle_on_and_off(pkg, oracle, files, fam, name):
    """An 11-token prompt in one eval, then 6 single tokens: every row and every K / V row written equals the oracle's; 5 launches per layer and token with
    the switch on, none with it off, the same bits either way."""
    t = toks_of(fam, 17, 7)
    plan = [(t[:11], 0)] + [([t[11 + i]], 11 + i) for i in range(6)]
    for on in (True, False):
        g = pkg.BiogptModel.load(files[(fam, name)], wide_decode=on)
        o = oracle.OracleModel(files[(fam, name)], n_threads=16)
        try:
            assert g.wide_decode is on and g.wide_decode_launches() == 0
            singles = walk(g, o, plan, (fam, name, on))
            same_kv(g, o, fam, 17, (fam, name, on))
            assert g.wide_decode_launches() == (5 * KW[fam]["n_layer"] * singles if on else 0)
        finally:
            g.close(); o.close()


@pytest.mark.parametrize("name", ("q4_1", "q8_0"))
def test_single_tokens_and_chunks_share_the_cache(pkg, oracle, files, name):
    t = toks_of("A", 24, 11)
    plan = [(t[:5], 0), ([t[5]], 5), (t[6:14], 6), ([t[14]], 14), ([t[15]], 15), (t[16:19], 16), ([t[19]], 19)]
    g = pkg.BiogptModel.load(files[("A", name)], wide_decode=True)
    o = oracle.OracleModel(files[("A", name)], n_threads=16)
    try:
        singles = walk(g, o, plan, ("A", name, "mixed"))
        same_kv(g, o, "A", 20, ("A", name, "mixed"))
        assert g.wide_decode_launches() == 5 * A["n_layer"] * singles
    finally:
        g.close(); o.close()


@pytest.mark.parametrize("name", ("q4_0", "q5_1"))
def test_generate_greedy_and_topk(pkg, oracle, files, name):
    prompt = toks_of("A", 9, 13)
    g = pkg.BiogptModel.load(files[("A", name)], wide_decode=True)
    o = oracle.OracleModel(files[("A", name)], n_threads=16)
    try:
        ids, _ = g.generate_greedy(prompt, 40)
        ref, _ = o.generate_greedy(prompt, 40)
        assert list(ids) == list(ref)
        assert g.wide_decode_launches() > 0      # (the captured steps count once, when they are captured)
        g.eval(prompt, 0)
        row = g.eval([int(ids[0])], len(prompt))
        vals, top = g.eval_topk([int(ids[0])], len(prompt), 5)
        order = np.lexsort((np.arange(row.size), -row))[:5]
        assert list(top) == list(order) and (bits(vals) == bits(row[order])).all()
    finally:
        g.close(); o.close()


@pytest.mark.parametrize("name", ("q4_1", "q8_0"))
def test_key_borders(pkg, oracle, files, name):
    """One token just below and just above every key count at which the attention launch changes form (the gate's own list), and at the last position."""
    borders = pkg.wide_decode_key_borders()
    assert borders and borders[-1] < A["n_positions"] - 1
    t = toks_of("A", A["n_positions"], 17)
    g = pkg.BiogptModel.load(files[("A", name)], wide_decode=True)
    o = oracle.OracleModel(files[("A", name)], n_threads=16)
    try:
        for n_past in sorted({b - 1 for b in borders} | set(borders) | {A["n_positions"] - 1}):      # n_past + 1 keys: b and b + 1
            before = g.wide_decode_launches()
            walk(g, o, [(t[:n_past], 0), ([t[n_past]], n_past)], ("A", name, "keys", n_past + 1))
            same_kv(g, o, "A", n_past + 1, ("A", name, "keys", n_past + 1))
            assert g.wide_decode_launches() == before + 5 * A["n_layer"]
    finally:
        g.close(); o.close()


def test_untouched_contexts(pkg, oracle, files, tmp_path):
    # a BioGPT-base file: not served, the counter stays 0
    f32, q40 = str(tmp_path / "base_f32.bin"), str(tmp_path / "base_q4_0.bin")
    pkg.write_synthetic(f32, n_vocab=512, n_layer=1, n_head=16, n_positions=32, d_ff=4096, d_model=1024, n_merges=3)
    pkg.quantize_file(f32, q40, "q4_0")
    g = pkg.BiogptModel.load(q40)
    try:
        assert g.set_wide_decode(True) is False and g.wide_decode is False
        g.eval([2, 5, 9], 0); g.eval([7], 3)
        assert g.wide_decode_launches() == 0
    finally:
        g.close()
    # a float file: "not served"
    g = pkg.BiogptModel.load(files[("A", "f32")])
    try:
        assert g.set_wide_decode(True) is False and "not served" in pkg._err() and g.wide_decode is False
    finally:
        g.close()
    # the SIMD association keeps its launches and its bits
    t = toks_of("A", 8, 19)
    rows = []
    for on in (False, True):
        g = pkg.BiogptModel.load(files[("A", "q4_0")], assoc="simd", wide_decode=on)
        try:
            g.eval(t[:5], 0)
            rows.append([g.eval([t[5 + i]], 5 + i) for i in range(3)])
            assert g.wide_decode_launches() == 0
        finally:
            g.close()
    assert all((bits(a) == bits(b)).all() for a, b in zip(*rows))
