"""Each kernel of the wide decode layer (csrc/kernels_wdecode.hip.h) alone, through biogpt_hip_wdecode_device, bit for bit against tests/chain_ref.py's
restatement of the oracle's arithmetic (lnq, block_sums, epi_resid, epi_gelu_q8, quantize_q8) on tests/chain_cases.py's hostile weights, activation columns
and LayerNorm rows, resized to the width at hand; the attention against tests/attn_ref.py.  Shapes (K, M): rows of 6, 5, 50 and 200 blocks, M no multiple of
any workgroup's share.  Every stage that applies to a shape runs on it: both residual kernels everywhere, fc1 where 32 | M, q/k/v where M == 3 K.  Guard
words behind every output stay 0xff, and at BioGPT-Large's shapes the reported launch is the row DESIGN.md 4.4 states for the engine's launch."""
import numpy as np
import pytest

import attn_ref
import chain_cases as C
import chain_ref as R
from chain_ref import F32

pytestmark = pytest.mark.gpu

SHAPES = [(192, 576), (160, 192), (1600, 1600), (6400, 1600)]
LN_ROWS = {192: range(len(C.LN_FAMILIES)), 160: range(len(C.LN_FAMILIES)), 1600: (0, 2, 4, 5, 7), 6400: (0, 2, 6)}      # 1600: normal, outlier, constant, huge, offset; 6400 (two chunks a thread, 25 chunk rows): normal, outlier, tiny
# (threads, grid, LDS bytes, most rows of a workgroup) of the launches at BioGPT-Large's shapes, as DESIGN.md 4.4 lists them
LAUNCH = {("OPROJ", 1600, 1600): (384, 256, 1568, 7), ("FC2", 6400, 1600): (704, 256, 5712, 7)}


def check_launch(got, stage, K, M):
    threads, grid, lds, rows = (int(v) for v in got["launched"][:4])
    assert threads % 64 == 0 and 64 <= threads <= 1024 and grid * rows >= M and lds <= 65536, (stage, K, M, threads, grid, lds, rows)
    assert (threads, grid, lds, rows) == LAUNCH.get((stage, K, M), (threads, grid, lds, rows)), (stage, K, M)


def guarded(row, n, dtype):
    out = np.full(n, 0xff, np.uint8).repeat(np.dtype(dtype).itemsize).view(dtype)
    out[:len(row)] = row
    return out


def same(got, want, what):
    for k, w in want.items():
        g = got[k]
        assert g.shape == w.shape and (g.view(np.uint8) == w.view(np.uint8)).all(), (what, k, np.argwhere(g.view(np.uint8) != w.view(np.uint8))[:4].tolist())


def ln_case(K, row, fc1):
    x = np.resize(C.ln_rows()[row], K).astype(F32)
    w, b = (np.resize(a, K).astype(F32) for a in C.ln_gain_bias())
    if fc1:      # the blocks that meet the fc1 family's +-65504 scales come out tiny
        blk = np.arange(K) // 32
        w[blk % 8 == 4], b[blk % 8 == 4] = 1e-6, 0.0
    return x, w, b


@pytest.mark.parametrize("wtype", R.TYPES, ids=[R.NAMES[t] for t in R.TYPES])
@pytest.mark.parametrize("shape", SHAPES, ids=["K%d_M%d" % s for s in SHAPES])
def test_linear_stages_equal_the_restatement(pkg, oracle, shape, wtype):
    K, M = shape
    q81, seed = R.Q81[wtype], K + M + R.TYPES.index(wtype)
    # out_proj and fc2: the producer's blocks in, bias and residual
    W = C.weights(oracle, "OPROJ", wtype, M, K)
    aq = C.columns("OPROJ", q81, K, 6)
    acc = R.block_sums(wtype, W, M, K, *aq)
    for col in (0, 3, 5):      # plain; scales of 1e+-30 / 65504; large codes
        bias, resid = C.bias_resid("OPROJ", wtype, acc[col:col + 1], seed + col)
        want = {"out": guarded(R.epi_resid(acc[col:col + 1], bias, resid)[0], M + 16, F32)}
        for stage in ("OPROJ", "FC2"):
            got = pkg.wdecode_device(stage, wtype, M, K, w_rows=W, aq=tuple(a[col] for a in aq), bias=bias, resid=resid[0])
            same(got, want, (stage, shape, col))
            check_launch(got, stage, K, M)
    # fc1: LayerNorm in front, GELU table and the Q8 hand-off behind
    if M % 32 == 0:
        W = C.weights(oracle, "FC1_Q8", wtype, M, K)
        bias = (C._rng(10, seed).standard_normal(M, dtype=F32) * F32(0.5)).astype(F32)
        for row in LN_ROWS[K]:
            x, w, b = ln_case(K, row, True)
            pre = R.block_sums(wtype, W, M, K, *R.lnq(x[None], w, b, q81))
            assert np.abs((bias[None] + pre).astype(F32)).max() < 65504.0, "the case stays inside the f16 range"
            (q, d, s), _ = R.epi_gelu_q8(pre, bias, q81)
            want = {"q": guarded(q[0], M + 32, np.int8), "d": guarded(d[0], M // 32 + 1, F32), "s": guarded(s[0], M // 32 + 1, np.uint32)}
            got = pkg.wdecode_device("FC1", wtype, M, K, w_rows=W, x=x, ln_w=w, ln_b=b, bias=bias)
            same(got, want, ("FC1", shape, C.LN_FAMILIES[row]))
            check_launch(got, "FC1", K, M)
    # q/k/v: LayerNorm in front, the Q scale and the cache rows behind
    if M == 3 * K and K % 64 == 0:
        H, P, n_past = K // 64, 7, 4
        W = C.weights(oracle, "QKV", wtype, M, K)
        bias = (C._rng(8, seed).standard_normal(M, dtype=F32) * F32(0.1)).astype(F32)
        for row in LN_ROWS[K]:
            x, w, b = ln_case(K, row, False)
            v = (bias[None] + R.block_sums(wtype, W, M, K, *R.lnq(x[None], w, b, q81))).astype(F32)[0]
            cache = np.full((H, P, 64), 0xff, np.uint8).repeat(4, axis=2).view(F32)
            want = {"out": guarded((v[:K] * R.Q_SCALE).astype(F32), K + 16, F32)}
            for name, rows in (("k", v[K:2 * K]), ("v", v[2 * K:])):
                want[name] = cache.copy()
                want[name][:, n_past, :] = rows.reshape(H, 64)
            got = pkg.wdecode_device("QKV", wtype, M, K, w_rows=W, x=x, ln_w=w, ln_b=b, bias=bias, k_cache=cache, v_cache=cache, P=P, n_past=n_past)
            same(got, want, ("QKV", shape, C.LN_FAMILIES[row]))
            check_launch(got, "QKV", K, M)


@pytest.mark.parametrize("q81", (False, True), ids=["q8_0", "q8_1"])
def test_attention_equals_the_restatement(pkg, q81):
    """Three heads at every form of the launch: 1 key, both sides of each border, the last key the kernel holds."""
    H, P = 3, 300
    g = np.random.default_rng(5)
    q = g.standard_normal(H * 64, dtype=F32)
    K, V = (g.standard_normal((H, P, 64), dtype=F32) for _ in range(2))
    borders = pkg.wide_decode_key_borders()
    own = borders[:-1]      # (the last border is the generic launch's own, which the layer keeps beyond these: tests/test_gpu_wide_decode.py)
    for T in sorted({1} | set(own) | {b + 1 for b in own[:-1]}):
        got = pkg.wdecode_device("ATTN", R.Q4_1 if q81 else R.Q4_0, H=H, P=P, n_past=T - 1, q=q, k_cache=K, v_cache=V)
        ref = [attn_ref.head(q[h * 64:h * 64 + 64], K[h], V[h], T) for h in range(H)]
        out, firm = np.concatenate([r["out"] for r in ref]), ~np.concatenate([r["fragile"] for r in ref])
        assert firm.mean() > 0.9 and (got["out"][:H * 64].view(np.uint32)[firm] == out.view(np.uint32)[firm]).all(), T
        assert (got["out"][H * 64:].view(np.uint32) == 0xffffffff).all(), T
        cq, cd, cs = R.quantize_q8(got["out"][:H * 64], q81)      # the blocks are those of the row the kernel wrote
        same(got, {"q": guarded(cq, H * 64 + 32, np.int8), "d": guarded(cd, 2 * H + 1, F32), "s": guarded(cs, 2 * H + 1, np.uint32)}, ("ATTN", T))
        assert tuple(got["launched"][:3]) == (1024, H, 16 if T <= own[0] else 8 if T <= own[1] else 4), T
