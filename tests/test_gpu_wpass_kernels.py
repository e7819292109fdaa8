"""Each site of the wide pass layer's linear stage (csrc/kernels_wpass.hip.h) alone, through biogpt_hip_wpass_device, bit for bit (as bytes, guard row included)
against tests/chain_ref.py's restatement of the oracle's arithmetic -- the restatement tests/test_chain_ref.py holds to the oracle on the CPU -- on
tests/chain_cases.py's hostile weights, activation columns and LayerNorm rows, used as tests/test_gpu_wchunk_kernels.py uses them.  (K, M, N): rows of 6 and 5
blocks (one partial phase) and of 50 and 200 (32 + 18, 6 x 32 + 8); 9 columns (the smallest pass), 16 (a full tile), 17 (a second column tile with one live
column) and 33 (a second column group); M = 613 at the logits site is 38 row tiles and 5 rows; M = 160 is five fc1 units (and 10 row tiles), M = 1600 at fc1
50: neither divides by a four-wave workgroup, whose last waves have no unit.  Every shape runs under the launch rule (cfg -1: the reported shape is the rule's
for the device's compute units) and under each of the four forced shapes (10 CT + WPB), so every instantiation -- four waves sharing the two-buffer phase loop
at K = 1600 and 6400 among them -- is held to the restatement."""
import functools

import numpy as np
import pytest

import chain_cases as C
import chain_ref as R
from chain_ref import F32
from test_gpu_wchunk_kernels import POOL, ln_blocks
from test_gpu_wdecode_kernels import same

pytestmark = pytest.mark.gpu

SHAPES = [(192, 576, 9), (160, 192, 17), (1600, 1600, 33), (6400, 1600, 16), (192, 613, 17), (1600, 160, 17)]
CFGS = (-1, 11, 14, 21, 24)
CASES = [(s, t) for s in SHAPES for t in R.TYPES]
N_PAST = 3


@functools.lru_cache(maxsize=2)
def reference(oracle, K, M, wtype):
    """(weights, the pool's eight columns, their block sums) per site the shape has: a column's sums do not depend on its neighbours."""
    q81 = R.Q81[wtype]
    ref = {}
    W = C.weights(oracle, "OPROJ", wtype, M, K)
    aq = tuple(a[list(POOL)] for a in C.columns("OPROJ", q81, K, 8))
    ref["RESID"] = (W, aq, R.block_sums(wtype, W, M, K, *aq))
    if M % 32 == 0:
        W = C.weights(oracle, "FC1_Q8", wtype, M, K)
        aq = ln_blocks(K, True, q81) if K <= 1600 else tuple(a[list(POOL)] for a in C.columns("FC1_Q8", q81, K, 8))
        ref["FC1"] = (W, aq, R.block_sums(wtype, W, M, K, *aq))
    if M == 3 * K and K % 64 == 0:
        W = C.weights(oracle, "QKV", wtype, M, K)
        aq = ln_blocks(K, False, q81)
        ref["QKV"] = (W, aq, R.block_sums(wtype, W, M, K, *aq))
    return ref


def check_launch(got, site, K, M, N, cfg):
    ct, wpb, gx, gy, lds, cus = (int(v) for v in got["launched"][:6])
    units = (M + 15) // 16 // (2 if site == "FC1" else 1)
    want_ct = cfg // 10 if cfg > 0 else 2 if N > 16 else 1
    want_wpb = cfg % 10 if cfg > 0 else 4 if units * -(-N // (16 * want_ct)) >= 4 * cus else 1      # the rule of DESIGN.md 4.4
    assert cus >= 1 and (ct, wpb) == (want_ct, want_wpb) and gx == -(-units // wpb) and gy == -(-N // (16 * ct)), (site, K, M, N, cfg, ct, wpb, gx, gy, cus)
    assert lds == (2 if K > 1024 else 1) * 16 * ct * (1040 + 132 * (2 if got["q81"] else 1)), (site, K, lds)


@pytest.mark.parametrize("cfg", CFGS, ids=["rule" if c < 0 else "ct%d_wpb%d" % divmod(c, 10) for c in CFGS])      # (varies fastest: the reference is shared)
@pytest.mark.parametrize("shape,wtype", CASES, ids=["K%d_M%d_N%d-%s" % (s + (R.NAMES[t],)) for s, t in CASES])
def test_sites_equal_the_restatement(pkg, oracle, shape, wtype, cfg):
    K, M, N = shape
    q81, seed = R.Q81[wtype], K + M + R.TYPES.index(wtype)
    ref = reference(oracle, K, M, wtype)
    pick = np.arange(N) % 8      # column c of the call is column c mod 8 of the pool: every tile holds every family
    cols = lambda aq: tuple(np.ascontiguousarray(a[pick]) for a in aq)

    def run(site, want, **kw):
        got = pkg.wpass_device(site, wtype, M, K, N, cfg=cfg, **kw)
        same(got, want, (site, shape, cfg))
        check_launch(dict(got, q81=q81), site, K, M, N, cfg)

    # the logits site: the raw sums, any M; out_proj and fc2: bias and residual (16 | M)
    W, aq, acc = ref["RESID"]
    acc = acc[pick]
    run("LOGITS", {"out": C.whole(acc, N + 1, M, F32)}, w_rows=W, aq=cols(aq))
    if M % 16 == 0:
        bias, resid = C.bias_resid("OPROJ", wtype, acc, seed + N)
        run("RESID", {"out": C.whole(R.epi_resid(acc, bias, resid), N + 1, M, F32)}, w_rows=W, aq=cols(aq), bias=bias, resid=resid)
    # fc1: the GELU table and each column's Q8 hand-off at column stride M, compared as integers and uint32
    if "FC1" in ref:
        W, aq, acc = ref["FC1"]
        acc = acc[pick]
        bias = (C._rng(10, seed).standard_normal(M, dtype=F32) * F32(0.5)).astype(F32)
        assert np.abs((bias[None] + acc).astype(F32)).max() < 65504.0, "the case stays inside the f16 range"
        (q, d, s), _ = R.epi_gelu_q8(acc, bias, q81)
        run("FC1", {"q": C.whole(q, N + 1, M, np.int8), "d": C.whole(d, N + 1, M // 32, F32), "s": C.whole(s, N + 1, M // 32, np.uint32)}, w_rows=W, aq=cols(aq), bias=bias)
    # q/k/v: the Q scale behind the bias, column c's cache rows at n_past + c and no other
    if "QKV" in ref:
        W, aq, acc = ref["QKV"]
        acc = acc[pick]
        H, P = K // 64, N_PAST + N + 1
        bias = (C._rng(8, seed).standard_normal(M, dtype=F32) * F32(0.1)).astype(F32)
        v = (bias[None] + acc).astype(F32)
        cache = np.full((H, P, 64), 0xff, np.uint8).repeat(4, axis=2).view(F32)
        want = {"out": C.whole((v[:, :K] * R.Q_SCALE).astype(F32), N + 1, K, F32)}
        for name, rows in (("k", v[:, K:2 * K]), ("v", v[:, 2 * K:])):
            want[name] = cache.copy()
            want[name][:, N_PAST:N_PAST + N, :] = rows.reshape(N, H, 64).transpose(1, 0, 2)
        run("QKV", want, w_rows=W, aq=cols(aq), bias=bias, k_cache=cache, v_cache=cache, P=P, n_past=N_PAST)
