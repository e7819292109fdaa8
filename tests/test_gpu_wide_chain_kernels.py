"""The wide chain's linear stage (matmul_wide_kernel, csrc/kernels_mfma_wide.hip.h), alone, against the oracle's arithmetic: the 20 instantiations (5 block
formats x QKV / RESID / GELU / LOGITS) through biogpt_hip_wide_chain_device, which builds the row-tiled image as a wide file's is built (the last row tile
zero-padded) and launches through the entry of the engine's own passes.

Shapes (K, M, N): BioGPT-Large's q/k/v (1600 = 32 + 18 blocks: a partial last phase; 17 columns: one live column in the second tile), its fc2 (6400 = 6 x 32 + 8
blocks; 16 columns: exactly one tile), a three-block row (one partial phase) with M = 192 at ONE column, and an lm_head of 2053 rows
(128 tiles + 5 rows: the zero-padded tile) at 33 columns.  Every epilogue that applies to a shape runs on it: q/k/v where M == 3 K, the residual and GELU
epilogues where 16 | M, the logits epilogue everywhere.

The inputs are tests/chain_cases.py's hostile weights and columns (extreme codes, scales 0 / subnormal / +-65504, zero blocks, +-127 activations, scales of
1e+-30), generated at these shapes; the expected outputs are tests/chain_ref.py's restatement (block_sums and the epilogues), which
tests/test_chain_restatement.py holds to the oracle on the CPU.  The comparison is exact: every f32 row and K / V row bit for bit, and every guard byte -- the
columns from N on, the rows from M on, every cache row no column writes -- still 0xff."""
import functools

import numpy as np
import pytest

import chain_cases as C
import chain_ref as R
from chain_ref import F32

pytestmark = pytest.mark.gpu

SHAPES = [(1600, 4800, 17), (6400, 1600, 16), (96, 192, 1), (1600, 2053, 33)]
LDS = {False: 16 * 1040 + 16 * 33 * 4, True: 16 * 1040 + 2 * 16 * 33 * 4}


def epilogues(K, M):
    e = []
    if M == 3 * K and K % 64 == 0:
        e.append("QKV")
    if M % 16 == 0:
        e += ["RESID", "GELU"]
    return e + ["LOGITS"]


@functools.lru_cache(maxsize=2)
def inputs(oracle, fc1, wtype, K, M, N):
    """(weights, columns, block sums) of a shape: the fc1 family (every pre-activation inside the f16 range) for the GELU epilogue, the general one otherwise."""
    op = "FC1_Q8" if fc1 else "OPROJ"
    W = C.weights(oracle, op, wtype, M, K)
    aq = C.columns(op, R.Q81[wtype], K, N)
    acc = R.block_sums(wtype, W, M, K, *aq)
    acc.setflags(write=False)
    return W, aq, acc


def qkv_want(acc, bias, D):
    """chain_ref.epi_qkv at d_model D: q = (b + acc) * (1 / sqrt(64)), k and v = b + acc."""
    q = ((bias[None, :D] + acc[:, :D]).astype(F32) * R.Q_SCALE).astype(F32)
    kv = (bias[None, D:] + acc[:, D:]).astype(F32)
    return q, kv[:, :D], kv[:, D:]


def check_launch(got, wtype, M, N, what):
    tiles = (M + 15) // 16
    exp = (256, (tiles + 3) // 4, (N + 15) // 16, LDS[R.Q81[wtype]]) + C.geometry(M, N) + (tiles,)
    assert tuple(got["launched"][:7]) == exp, (what, list(got["launched"]), exp)


@pytest.mark.parametrize("wtype", R.TYPES, ids=[R.NAMES[t] for t in R.TYPES])
@pytest.mark.parametrize("shape", SHAPES, ids=["K%d_M%d_N%d" % s for s in SHAPES])
def test_stage_equals_the_restatement(pkg, oracle, shape, wtype):
    K, M, N = shape
    cols, ldo = C.geometry(M, N)
    seed = N + 1000 * R.TYPES.index(wtype) + K
    for epi in epilogues(K, M):
        W, aq, acc = inputs(oracle, epi == "GELU", wtype, K, M, N)
        args = dict(epi=epi, wtype=wtype, M=M, K=K, N=N, w_rows=W, aq_q=aq[0], aq_d=aq[1], aq_s=aq[2])
        want = {}
        if epi == "LOGITS":
            want["out"] = C.whole(acc, cols, ldo, F32)
        elif epi == "RESID":
            args["bias"], args["resid"] = C.bias_resid("OPROJ", wtype, acc, seed)
            want["out"] = C.whole(R.epi_resid(acc, args["bias"], args["resid"]), cols, ldo, F32)
        elif epi == "GELU":
            args["bias"] = (C._rng(10, seed).standard_normal(M, dtype=F32) * F32(0.5)).astype(F32)
            pre = (args["bias"][None, :] + acc).astype(F32)
            assert np.isfinite(pre).all() and np.abs(pre).max() < 65504.0, "the case stays inside the f16 range"
            want["out"] = C.whole(R.gelu_table()[R._f16_index(pre)], cols, ldo, F32)
        else:
            H = K // 64
            for form in (1, 2) if N > 1 else (1, 0):      # one column per sequence; packed columns of three slots (one column: the context's own)
                st = C.qkv_states(form, N, seed)
                a = dict(args, bias=(C._rng(8, seed).standard_normal(M, dtype=F32) * F32(0.1)).astype(F32))
                q, k, v = qkv_want(acc, a["bias"], K)
                w = {"out": C.whole(q, cols, K, F32)}
                for name, rows in (("k", k), ("v", v)):
                    slots = np.full((st["n_slots"], H, st["P"], 64), 0xff, dtype=np.uint8).repeat(4, axis=3).view(F32)
                    slots[st["slot"], :, st["pos"], :] = rows.reshape(N, H, 64)
                    w[name] = slots
                a.update(dev_state=st["dev_state"], seq_states=st["seq_states"], col_mode=st["col_mode"], P=st["P"])
                a["k_slots"] = a["v_slots"] = np.full((st["n_slots"], H, st["P"], 64), 0xff, dtype=np.uint8).repeat(4, axis=3).view(F32)
                what = ("QKV", R.NAMES[wtype], shape, "states %d" % form)
                got = pkg.wide_chain_device(**a)
                check_launch(got, wtype, M, N, what)
                C.compare(got, w, what)
            continue
        what = (epi, R.NAMES[wtype], shape)
        got = pkg.wide_chain_device(**args)
        check_launch(got, wtype, M, N, what)
        C.compare(got, want, what)
        assert np.isfinite(got["out"][:N, :M]).all(), what


def test_refusals_come_before_any_launch(pkg, oracle):
    K, M, N = 96, 192, 1
    z = dict(wtype=R.Q4_0, M=M, K=K, N=N, w_rows=np.zeros(M * (K // 32) * 18, np.uint8), aq_q=np.zeros((N, K), np.int8), aq_d=np.zeros((N, K // 32), F32),
             aq_s=np.zeros((N, K // 32), np.uint32), bias=np.zeros(M, F32))
    with pytest.raises(pkg.BiogptError, match="whole number of 16-row tiles"):
        pkg.wide_chain_device(epi="GELU", **dict(z, M=200))
    with pytest.raises(pkg.BiogptError, match="multiple of 32"):
        pkg.wide_chain_device(epi="GELU", **dict(z, K=100))
    with pytest.raises(pkg.BiogptError, match="3 K x K"):
        pkg.wide_chain_device(epi="QKV", dev_state=np.zeros(4, np.int32), P=1, k_slots=np.zeros((1, 1, 1, 64), F32), v_slots=np.zeros((1, 1, 1, 64), F32), **z)
    with pytest.raises(pkg.BiogptError, match="resid is NULL"):
        pkg.wide_chain_device(epi="RESID", **z)
