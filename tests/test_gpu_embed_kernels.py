"""The four kernels of the embedding tail, each alone (ln_rows_kernel<1024> / <0>, pool_rows_kernel, pool_finish_kernel, head_rows_kernel), through
biogpt_hip_embed_device, which launches through the helpers of the engine's own calls.  Every case of tests/embed_cases.py: rows whose double sums are exact in
any order are held to tests/embed_ref.py bit for bit, hostile full-mantissa rows to its bounds against an exact sum; every guard byte and every unwritten row
keeps its preset; the launch is the one the shape should get.  No model files."""
import pytest

import embed_cases as C
import embed_ref as E

pytestmark = pytest.mark.gpu


# ---- LayerNorm ----

@pytest.mark.parametrize("W", C.LN_WIDTHS)
def test_layer_norm_rows(pkg, W):
    ran = 0
    for name, kw in C.ln_cases():
        if kw["x"].shape[1] != W:
            continue
        want = E.layer_norm_rows(**kw)
        got = pkg.embed_device("LN", kw["x"], ln_w=kw["w"], ln_b=kw["b"], seq_states=kw.get("states"), slot_div=kw.get("slot_div", 0), P=kw.get("P", 0),
                               n_out_rows=kw.get("n_out_rows"))
        C.assert_bits(got["out"], want, name)      # the rows, and the 0xff preset of every unwritten row and of the guard row
        assert got["launched"].tolist() == [1024 if W == 1024 else 0, 256, len(kw["x"]), 1, 0, 0, 0, 0], (name, got["launched"])
        ran += 1
    assert ran >= 2


# ---- pooling ----

def run_pool(pkg, c):
    got = pkg.embed_device("POOL", c["x"], seq_states=c["states"], lens=c["lens"], pass_cols=c["pass_cols"], pooling=c["pooling"], normalize=c["normalize"])
    W, none = c["W"], c["pooling"] == "none"
    rows_out = len(c["x"]) if none else len(c["lens"])
    finish = rows_out if (c["pooling"] == "mean" or c["normalize"]) else 0
    want = [0, 0, 0, 0, 0, finish, 0, 0] if none else [1, 256, -(-W // 64), c["pass_cols"][-1], 0, finish, len(c["pass_cols"]), 0]
    assert got["launched"].tolist() == want, (c["name"], got["launched"], want)
    return got


def check_pool(c, got):
    C.check_pool(c, got["out"], got.get("acc"))


@pytest.mark.parametrize("W", C.POOL_WIDTHS)
def test_pooling(pkg, W):
    means = {}
    for c in C.pool_cases(W):
        got = run_pool(pkg, c)
        check_pool(c, got)
        if c["pooling"] == "mean" and not c["normalize"] and c["lens"] == list(C.POOL_LENS):
            means.setdefault(c["kind"], []).append((c["name"], got))
    # the same sequences in passes of 16 columns, in one pass and in passes of one column: the same bits on exact rows (accumulator and mean)
    for kind, runs in means.items():
        assert len(runs) == len(C.PACKINGS), kind
        if kind in C.EXACT_KINDS:
            for name, got in runs[1:]:
                C.assert_bits(got["out"], runs[0][1]["out"], name + " against " + runs[0][0])
                C.assert_bits(got["acc"], runs[0][1]["acc"], name + " against " + runs[0][0] + " (acc)")


def test_normalising_a_rounded_mean(pkg):
    """Means of 4/3 and 5/3: the float32 mean is normalised, not the double quotient (exact in any order, and the two differ)."""
    c = C.thirds_case()
    check_pool(c, run_pool(pkg, c))


# ---- the head ----

@pytest.mark.parametrize("shape", C.HEAD_SHAPES, ids=["%dx%dx%d" % s for s in C.HEAD_SHAPES])
def test_head(pkg, shape):
    n_rows, n_out, W = shape
    ran = 0
    for c in C.head_cases():
        if (c["x"].shape[0], c["w"].shape[0], c["x"].shape[1]) != shape:
            continue
        got = pkg.embed_device("HEAD", c["x"], w=c["w"], b=c["b"])
        assert got["launched"].tolist() == [3, 256, -(-n_rows // 8), 1, 8 * W * 4, 0, 0, 0], (c["name"], got["launched"])
        C.assert_guard(got["out"], [-1], c["name"])
        if c["expect"] == "bits":
            C.assert_bits(got["out"], C.head_expected(c), c["name"])
        else:
            ref, bound = C.head_bound(c)
            C.assert_within(got["out"][:-1], ref, bound, c["name"])
        ran += 1
    assert ran >= 6


def test_head_at_the_widest_row_a_launch_admits(pkg):
    """W = 2048: 8 rows are exactly the 65,536 bytes of dynamic LDS that check_head_width admits."""
    c = C.head_border_case()
    got = pkg.embed_device("HEAD", c["x"], w=c["w"], b=c["b"])
    assert got["launched"].tolist() == [3, 256, 2, 1, 65536, 0, 0, 0], got["launched"]
    C.assert_bits(got["out"], C.head_expected(c), c["name"])
