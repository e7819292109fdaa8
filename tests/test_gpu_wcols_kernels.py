"""The wide column layer's linear stage (wcols_kernel, csrc/kernels_wcols.hip.h), alone, against the oracle's arithmetic: through biogpt_hip_wcols_device, which
builds the row-tiled image as a wide file's is built and launches through the entry of the engine's own passes.

Shapes (M, K): (48, 96) -- 3 blocks, fewer than one round of either wave count; (77, 1600) -- 50 blocks, a partial last round (32 + 18 at 8 waves, 3 x 16 + 2 at
4), and a zero-padded fifth row tile; (48, 6400) -- 200 blocks, full rounds and a partial one (6 x 32 + 8; 12 x 16 + 8); and (192, 64), the smallest q/k/v (none of
the other three is 3 K x K).  Every epilogue that applies to a shape runs on it, at 1, 2, 5, 15 and 16 columns, at 4 and at 8 waves.

The inputs are tests/chain_cases.py's hostile weights and columns; the expected outputs are tests/chain_ref.py's restatement (block_sums and the epilogues).
The comparison is exact: every f32 row and K / V row bit for bit, and every guard byte -- the columns from N on, the rows from M on, every cache row no column
writes -- still 0xff; so both wave counts give the same bytes."""
import numpy as np
import pytest

import chain_cases as C
import chain_ref as R
from chain_ref import F32
from test_gpu_wide_chain_kernels import epilogues, qkv_want

pytestmark = pytest.mark.gpu

SHAPES = [(48, 96), (77, 1600), (48, 6400), (192, 64)]
COLS = (1, 2, 5, 15, 16)


def cases(oracle, wtype, M, K, N, seed):
    """(epilogue, probe arguments, whole expected outputs) of one shape and column count"""
    cols, ldo = C.geometry(M, N)
    for epi in epilogues(K, M):
        op = "FC1_Q8" if epi == "GELU" else "OPROJ"
        W, aq = C.weights(oracle, op, wtype, M, K), C.columns(op, R.Q81[wtype], K, N)
        acc = R.block_sums(wtype, W, M, K, *aq)
        a = dict(epi=epi, wtype=wtype, M=M, K=K, N=N, w_rows=W, aq_q=aq[0], aq_d=aq[1], aq_s=aq[2])
        if epi == "LOGITS":
            yield epi, a, {"out": C.whole(acc, cols, ldo, F32)}
        elif epi == "RESID":
            a["bias"], a["resid"] = C.bias_resid("OPROJ", wtype, acc, seed)
            yield epi, a, {"out": C.whole(R.epi_resid(acc, a["bias"], a["resid"]), cols, ldo, F32)}
        elif epi == "GELU":
            a["bias"] = (C._rng(10, seed).standard_normal(M, dtype=F32) * F32(0.5)).astype(F32)
            pre = (a["bias"][None, :] + acc).astype(F32)
            assert np.isfinite(pre).all() and np.abs(pre).max() < 65504.0, "the case stays inside the f16 range"
            yield epi, a, {"out": C.whole(R.gelu_table()[R._f16_index(pre)], cols, ldo, F32)}
        else:
            H = K // 64
            a["bias"] = (C._rng(8, seed).standard_normal(M, dtype=F32) * F32(0.1)).astype(F32)
            q, k, v = qkv_want(acc, a["bias"], K)
            for form in (1, 2) if N > 1 else (1, 0):      # one column per sequence; packed columns of three slots (one column: the context's own)
                st = C.qkv_states(form, N, seed)
                empty = np.full((st["n_slots"], H, st["P"], 64), 0xff, dtype=np.uint8).repeat(4, axis=3).view(F32)
                want = {"out": C.whole(q, cols, K, F32)}
                for name, rows in (("k", k), ("v", v)):
                    want[name] = empty.copy()
                    want[name][st["slot"], :, st["pos"], :] = rows.reshape(N, H, 64)
                yield "QKV states %d" % form, dict(a, dev_state=st["dev_state"], seq_states=st["seq_states"], col_mode=st["col_mode"], P=st["P"], k_slots=empty,
                                                   v_slots=empty), want


@pytest.mark.parametrize("wtype", R.TYPES, ids=[R.NAMES[t] for t in R.TYPES])
@pytest.mark.parametrize("shape", SHAPES, ids=["M%d_K%d" % s for s in SHAPES])
def test_stage_equals_the_restatement(pkg, oracle, shape, wtype):
    M, K = shape
    for N in COLS:
        for epi, args, want in cases(oracle, wtype, M, K, N, N + 1000 * R.TYPES.index(wtype) + K):
            for nw in (4, 8):
                what = (epi, R.NAMES[wtype], shape, N, nw)
                got = pkg.wcols_device(nw=nw, **args)
                rounds = -(-(K // 32) // (4 * nw))
                assert tuple(got["launched"][:5]) == (nw, 64 * nw, (M + 15) // 16, 2 * 4 * nw * 1024, rounds), (what, list(got["launched"]))
                C.compare(got, want, what)
