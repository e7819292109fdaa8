"""Each linear stage of the wide chunk layer (csrc/kernels_wchunk.hip.h) alone, through biogpt_hip_wchunk_device, bit for bit (as bytes, guard row included)
against tests/chain_ref.py's restatement of the oracle's arithmetic on tests/chain_cases.py's hostile weights, activation columns and LayerNorm rows, used as
tests/test_gpu_wdecode_kernels.py uses them for one column.  Shapes (K, M): rows of 6, 5, 50 and 200 blocks, M no multiple of any workgroup's share; N = 2, 3
and 8 columns, every column of a call from another family.  (6400, 1600) at 8 columns is the launch above 64 KB of LDS."""
import functools

import numpy as np
import pytest

import chain_cases as C
import chain_ref as R
from chain_ref import F32
from test_gpu_wdecode_kernels import LN_ROWS, SHAPES, ln_case, same

pytestmark = pytest.mark.gpu

LARGE_TYPES = (R.Q4_0, R.Q5_1, R.Q8_0)
CASES = [(s, t) for s in SHAPES for t in (R.TYPES if s[0] < 1000 else LARGE_TYPES)]
POOL = (0, 3, 5, 1, 4, 2, 6, 7)      # the order a call takes the site's pool in: plain, scales of 1e+-30 / 65504, large codes first
N_PAST = 2


def ln_blocks(K, fc1, q81):
    """Eight columns of LayerNorm + Q8 blocks, as the producer launch leaves them: LayerNorm families in turn, a family's second use rotated by whole blocks."""
    fams = list(LN_ROWS[K])
    rows = []
    for i in range(8):
        x, w, b = ln_case(K, fams[i % len(fams)], fc1)
        rows.append(np.roll(x, 32 * (i // len(fams))))
    return R.lnq(np.stack(rows), w, b, q81)


@functools.lru_cache(maxsize=2)
def reference(oracle, K, M, wtype):
    """The block sums of all eight columns of every site the shape has, once per (shape, format): a column's sums do not depend on its neighbours."""
    q81 = R.Q81[wtype]
    ref = {}
    W = C.weights(oracle, "OPROJ", wtype, M, K)
    aq = tuple(a[list(POOL)] for a in C.columns("OPROJ", q81, K, 8))
    ref["RESID"] = (W, aq, R.block_sums(wtype, W, M, K, *aq))
    if M % 32 == 0 and K <= 1600:      # (fc1 reads d_model-wide rows; 32 rows of 200 blocks for 8 columns are 274 KB of LDS: fc2's K is not an fc1 shape)
        W = C.weights(oracle, "FC1_Q8", wtype, M, K)
        aq = ln_blocks(K, True, q81)
        ref["FC1"] = (W, aq, R.block_sums(wtype, W, M, K, *aq))
    if M == 3 * K and K % 64 == 0:
        W = C.weights(oracle, "QKV", wtype, M, K)
        aq = ln_blocks(K, False, q81)
        ref["QKV"] = (W, aq, R.block_sums(wtype, W, M, K, *aq))
    return ref


def check_launch(got, stage, K, M, N):
    threads, grid, lds, rows = (int(v) for v in got["launched"][:4])
    assert threads % 64 == 0 and 64 <= threads <= 1024 and grid * rows >= M and rows * N <= threads, (stage, K, M, N, threads, grid, lds, rows)
    if (K, N) == (6400, 8):
        assert lds > 65536, lds


@pytest.mark.parametrize("N", (2, 3, 8))
@pytest.mark.parametrize("shape,wtype", CASES, ids=["K%d_M%d-%s" % (s + (R.NAMES[t],)) for s, t in CASES])
def test_stages_equal_the_restatement(pkg, oracle, shape, wtype, N):
    K, M = shape
    q81, seed = R.Q81[wtype], K + M + R.TYPES.index(wtype)
    ref = reference(oracle, K, M, wtype)
    cols = lambda aq: tuple(a[:N] for a in aq)
    # out_proj and fc2: bias and residual, [N][M]
    W, aq, acc = ref["RESID"]
    bias, resid = C.bias_resid("OPROJ", wtype, acc[:N], seed + N)
    want = {"out": C.whole(R.epi_resid(acc[:N], bias, resid), N + 1, M, F32)}
    for stage in ("OPROJ", "FC2"):
        got = pkg.wchunk_device(stage, wtype, M, K, N, w_rows=W, aq=cols(aq), bias=bias, resid=resid)
        same(got, want, (stage, shape, N))
        check_launch(got, stage, K, M, N)
    # fc1: the GELU table and each column's Q8 hand-off at column stride M
    if "FC1" in ref:
        W, aq, acc = ref["FC1"]
        bias = (C._rng(10, seed).standard_normal(M, dtype=F32) * F32(0.5)).astype(F32)
        assert np.abs((bias[None] + acc[:N]).astype(F32)).max() < 65504.0, "the case stays inside the f16 range"
        (q, d, s), _ = R.epi_gelu_q8(acc[:N], bias, q81)
        want = {"q": C.whole(q, N + 1, M, np.int8), "d": C.whole(d, N + 1, M // 32, F32), "s": C.whole(s, N + 1, M // 32, np.uint32)}
        got = pkg.wchunk_device("FC1", wtype, M, K, N, w_rows=W, aq=cols(aq), bias=bias)
        same(got, want, ("FC1", shape, N))
        check_launch(got, "FC1", K, M, N)
    # q/k/v: the Q scale behind the bias, column c's cache rows at n_past + c and no other
    if "QKV" in ref:
        W, aq, acc = ref["QKV"]
        H, P = K // 64, N_PAST + N + 1
        bias = (C._rng(8, seed).standard_normal(M, dtype=F32) * F32(0.1)).astype(F32)
        v = (bias[None] + acc[:N]).astype(F32)
        cache = np.full((H, P, 64), 0xff, np.uint8).repeat(4, axis=2).view(F32)
        want = {"out": C.whole((v[:, :K] * R.Q_SCALE).astype(F32), N + 1, K, F32)}
        for name, rows in (("k", v[:, K:2 * K]), ("v", v[:, 2 * K:])):
            want[name] = cache.copy()
            want[name][:, N_PAST:N_PAST + N, :] = rows.reshape(N, H, 64).transpose(1, 0, 2)
        got = pkg.wchunk_device("QKV", wtype, M, K, N, w_rows=W, aq=cols(aq), bias=bias, k_cache=cache, v_cache=cache, P=P, n_past=N_PAST)
        same(got, want, ("QKV", shape, N))
        check_launch(got, "QKV", K, M, N)


@pytest.mark.parametrize("N", (1, 9))
def test_column_counts_outside_the_chunk_are_refused_by_name(pkg, N):
    z = np.zeros((N, 192), np.int8), np.zeros((N, 6), F32), np.zeros((N, 6), np.uint32)
    with pytest.raises(pkg.BiogptError, match="N = %d columns" % N):
        pkg.wchunk_device("OPROJ", R.Q4_0, 192, 192, N, w_rows=np.zeros(192 * 6 * 18, np.uint8), aq=z, bias=np.zeros(192, F32), resid=np.zeros((N, 192), F32))
