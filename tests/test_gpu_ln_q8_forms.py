"""The LayerNorm + Q8 stage of the single-token decode launches, alone.

1. The short arithmetic forms of csrc/kernels_decode.hip.h (q8_round, ln_inv_std, q8_scales) against the expressions they stand for over ALL 2^32 float bit
   patterns, in one launch (biogpt_hip_q8_forms_device): no mismatch, and the number of patterns each check saw is the size of the range its guard states.
2. ln4_q8_1024 (one workgroup of 512 threads per row, as the pipelined launches run it) and q8_block32 through biogpt_hip_ln_q8_device, bit for bit against the
   LayerNorm + Q8 restatement of tests/chain_ref.py (held to bo_layer_norm / bo_quantize by tests/test_chain_restatement.py): the LayerNorm rows of
   tests/chain_cases.py and rows whose blocks are set through the bias (gain 0), so that a quotient lands exactly on k + 0.5 and one ulp to either side, the
   block maximum is 127 * 2^j, or lies outside the range of the short scales, where the general expressions run.  No tolerance."""
import numpy as np
import pytest

import chain_cases as C
import chain_ref as R

F32 = np.float32
FORMS = ((False, False), (False, True), (True, True))      # (q81, want_sum): Q8_0 without and with integer block sums, Q8_1


@pytest.mark.gpu
def test_short_forms_equal_the_expressions_on_every_bit_pattern(pkg):
    res = pkg.q8_forms_device()
    print(res)
    n_round = 2 * (0x4A800000 + 1)                          # |x| <= 2^22
    want = {"ln_inv_std_short in range": 0x71800000 - 0x35800000,       # 2^-20 <= v < 2^100
            "ln_inv_std every pattern": 1 << 32,
            "q8_round |x| <= 2^22": n_round,
            "q8_round every other pattern": (1 << 32) - n_round,
            "q8_scales_short in range": 0x71800000 - 0x0D800000,        # 2^-100 <= a < 2^100
            "q8_scales every pattern": 1 << 32}
    assert set(res) == set(want)
    for name, n in want.items():
        assert res[name]["tested"] == n, (name, res[name], n)
    for name in want:
        first = res[name]["first"]
        assert res[name]["mismatches"] == 0 and first is None, (name, res[name], None if first is None else hex(first))


# ---- rows --------------------------------------------------------------------------------------------------------------------------------------------------

def _tie_triples(g, d, idv, amax, n):
    """n triples (x, its neighbour below, its neighbour above) with float32(x * idv) exactly k + 0.5, |x| < amax."""
    out = []
    for k in g.permutation(np.arange(0, 126)):
        target = F32(k + 0.5)
        x0 = F32(target * d)
        for step in range(-3, 4):
            x = x0
            for _ in range(abs(step)):
                x = np.nextafter(x, F32(np.inf) if step > 0 else F32(0))
            if F32(x * idv) == target and abs(x) < amax:
                sgn = F32(-1.0) if g.integers(0, 2) else F32(1.0)
                out.append([sgn * x, sgn * np.nextafter(x, F32(0)), sgn * np.nextafter(x, F32(np.inf))])
                break
        if len(out) == n:
            break
    assert len(out) == n, "no %d exact ties for this scale" % n
    return np.array(out, dtype=F32).reshape(-1)


def designed_blocks():
    """[4 * 32, 32]: four rows' worth of blocks.  Row 0: amax = 127 * 2^j, j = -16 .. 15 (d = 2^j, id = 2^-j: every quotient exact), ties k + 0.5 and their
    neighbours.  Row 1: a general scale per block, x searched so that float32(x * id) is exactly k + 0.5, and its neighbours.  Row 2: amax = 127 * 2^j for
    j = -24 .. 15 cycled (the scales an f16 holds exactly, subnormals included) with random values.  Row 3: block maxima around and outside [2^-100, 2^100)
    beside ordinary blocks of the same wave, a zero block, and waves wholly inside the range."""
    g = np.random.default_rng(0x7181)
    blocks = np.zeros((128, 32), dtype=F32)
    for j in range(32):                                               # row 0
        e = j - 16
        ks = g.integers(0, 126, 10)
        sg = np.where(g.integers(0, 2, 10) == 1, -1.0, 1.0)
        t = ((ks + 0.5) * sg).astype(F32)
        vals = np.concatenate([[127.0], t, np.nextafter(t, F32(0)), np.nextafter(t, (F32(np.inf) * sg).astype(F32)), [0.0]]).astype(F32)
        blocks[j] = np.ldexp(vals, e).astype(F32)
    for j in range(32):                                               # row 1
        amax = F32(g.uniform(0.5, 4.0))
        d = F32(amax / F32(127.0))
        idv = F32(F32(1.0) / d)
        tri = _tie_triples(g, d, idv, amax, 10)
        blocks[32 + j] = np.concatenate([[amax if j % 2 else -amax], tri, [F32(g.uniform(-1, 1)) * amax]]).astype(F32)
    for j in range(32):                                               # row 2
        e = -24 + (j * 40) // 32 + (j % 2)
        e = min(e, 15)
        v = g.uniform(-127.0, 127.0, 32).astype(F32)
        v[g.integers(0, 32)] = 127.0 if j % 3 else -127.0
        blocks[64 + j] = np.ldexp(v, e).astype(F32)
    lo, hi = F32(2.0 ** -100), F32(2.0 ** 100)
    maxima = {0: np.nextafter(lo, F32(0)), 1: lo, 2: F32(1e-33), 3: F32(1.0), 5: F32(3e-36), 8: hi, 9: np.nextafter(hi, F32(0)), 10: F32(1e31), 11: F32(2.5),
              13: F32(1e33), 16: F32(0.0), 17: F32(7.0), 27: F32(1e-32)}
    for j in range(32):                                               # row 3 (blocks 0 - 7, 8 - 15, 16 - 23, 24 - 31: the four waves of the LayerNorm stage)
        amax = maxima.get(j, F32(g.uniform(0.01, 100.0)))
        v = (g.uniform(-1.0, 1.0, 32).astype(F32) * amax).astype(F32)
        v[g.integers(0, 32)] = amax if j % 2 else -amax
        blocks[96 + j] = v if amax > 0 else F32(0.0)
    return blocks


@pytest.fixture(scope="module")
def stage_rows():
    """x [n, 1024], ln_w, ln_b [n, 1024], and the rows' LayerNorm outputs by the restatement.  Rows 0 .. 8: tests/chain_cases.py's LayerNorm rows under its gain /
    bias (outlier channels, a zero and a constant block, variance 0, magnitude 1e18: variance + eps beyond ln_inv_std's range); then the designed rows: gain 0,
    so that LayerNorm's output IS the bias (0 * finite + b = b exactly), over an ordinary input row."""
    x0 = C.ln_rows()
    w0, b0 = C.ln_gain_bias()
    des = designed_blocks().reshape(-1, 1024)
    n = x0.shape[0] + des.shape[0]
    g = np.random.default_rng(0x7182)
    x = np.concatenate([x0, g.standard_normal(des.shape, dtype=F32)])
    w = np.concatenate([np.broadcast_to(w0, x0.shape), np.zeros_like(des)]).astype(F32)
    b = np.concatenate([np.broadcast_to(b0, x0.shape), des]).astype(F32)
    assert n <= 64
    with np.errstate(over="ignore", invalid="ignore"):
        y = np.stack([R.layer_norm(x[i], w[i], b[i]) for i in range(n)])
    assert (y[x0.shape[0]:].view(np.uint32) == des.view(np.uint32)).all(), "a designed row's LayerNorm output is its bias"
    return x, w, b, y


def _want(y, q81):
    with np.errstate(over="ignore", invalid="ignore"):
        return R.quantize_q8(y, q81)


def _same(got, want, what):
    bad = np.argwhere(got.view(np.uint8).reshape(got.shape[0], -1) != want.view(np.uint8).reshape(want.shape[0], -1))
    assert bad.size == 0, (what, "%d bytes differ" % len(bad), "first (row, byte)", tuple(int(v) for v in bad[0]))


def test_designed_rows_hold_what_they_claim(stage_rows):      # (no GPU needed)
    """Exact ties and their neighbours among the quotients; block maxima on both sides of the short scales' range."""
    des = designed_blocks()
    amax = np.abs(des).max(axis=1)
    d = (amax / F32(127.0)).astype(F32)
    with np.errstate(divide="ignore", over="ignore"):
        idv = np.where(d != 0, F32(1.0) / d, F32(0.0)).astype(F32)
    t = (des[:64] * idv[:64, None]).astype(F32)
    frac = np.abs(t) - np.floor(np.abs(t))
    assert ((frac == 0.5).sum(axis=1) >= 10).all(), "every block of the two tie rows has 10 quotients exactly on k + 0.5"
    assert (d[:32] == np.ldexp(F32(1.0), np.arange(-16, 16))).all()
    rng = (amax[96:] >= F32(2.0 ** -100)) & (amax[96:] < F32(2.0 ** 100))
    assert (~rng).sum() >= 8 and rng[24:27].all() and rng[28:].all() and not rng[0] and rng[1] and not rng[8] and rng[9]
    assert np.isfinite(des * idv[:, None]).all(), "every quotient is finite: the restatement's integer conversion is defined"
    for q81 in (False, True):           # a rounding that is not half away from zero shows on these rows
        right, wrong = R.quantize_q8(des[:96], q81), R.quantize_q8(des[:96], q81, mistake="nearest_even")
        assert ((right[0] != wrong[0]).sum(axis=1) >= 1)[:64].all(), "every block of the two tie rows has a code that nearest-even rounding moves"


@pytest.mark.gpu
@pytest.mark.parametrize("q81,want_sum", FORMS, ids=["q8_0", "q8_0_sums", "q8_1"])
def test_stage_equals_the_restatement(pkg, stage_rows, q81, want_sum):
    x, w, b, y = stage_rows
    wq, wd, ws = _want(y, q81)
    n0 = C.ln_rows().shape[0]
    for what, sl, per_row in (("chain_cases rows, one gain / bias", slice(0, n0), False), ("every row, a gain / bias per row", slice(0, x.shape[0]), True)):
        q, d, s = pkg.ln_q8_device(x[sl], w[sl] if per_row else w[0], b[sl] if per_row else b[0], q81=q81, want_sum=want_sum)
        _same(q, wq[sl], (what, "codes"))
        _same(d, wd[sl], (what, "scales"))
        if q81 or want_sum:
            _same(s, ws[sl], (what, "sums"))
        else:
            assert (s == 0xFFFFFFFF).all(), (what, "block sums written by the form that has none")


@pytest.mark.gpu
@pytest.mark.parametrize("q81,want_sum", FORMS, ids=["q8_0", "q8_0_sums", "q8_1"])
def test_block_quantizer_equals_the_restatement(pkg, stage_rows, q81, want_sum):
    """q8_block32 on every block of the stage's LayerNorm outputs (an odd number of them: the last wave holds one block)."""
    y = stage_rows[3]
    blocks = np.ascontiguousarray(y.reshape(-1, 32)[:-1])
    assert blocks.shape[0] % 2 == 1
    wq, wd, ws = _want(blocks, q81)
    q, d, s = pkg.ln_q8_device(blocks, q81=q81, want_sum=want_sum, blocks=True)
    _same(q, wq, "codes")
    _same(d, wd, "scales")
    if q81 or want_sum:
        _same(s, ws, "sums")
    else:
        assert (s == 0).all()
