"""The float chain's linear stage (fchain_kernel, csrc/kernels_fchain.hip.h), alone, against the oracle's arithmetic: every fchain_kernel<WT, EPI> (F32 / F16 x
QKV / RESID / GELU / LOGITS) at each of its three tile shapes, through biogpt_hip_fchain_device, which launches through the entry of the engine's own passes.

Shapes (K, M, N): BioGPT-base's q/k/v at 17 columns (both column-state forms; the K / V slots whole), its fc2 at 16, 1600 x 1600 at 9 (K is no multiple of 64
sixteen-byte chunks: a partial last staging phase, lanes without a chunk), a three-block row at ONE column, an lm_head of 2053 rows at 33 columns; and the
borders of the kernel's own 8- and 16-column tiles the five do not cover: 7, 8 and 15 columns at the small shape.  Every epilogue that applies runs on a shape.

The inputs are tests/fchain_ref.py's rows, whose double sums are exact in ANY order (the kernel's association is its own), the expected outputs its
restatement, which tests/test_fchain_restatement.py holds to the oracle on the CPU.  The comparison is exact: every f32 row and K / V row bit for bit, and
every guard byte -- the columns from N on, the rows from M on, every cache row no column writes -- still 0xff.  The LayerNorm producer runs on
chain_cases.ln_rows() (no row is chain_ref.ln_fragile), for both types."""
import functools

import numpy as np
import pytest

import chain_cases as C
import fchain_ref as FR
from fchain_ref import F32

pytestmark = pytest.mark.gpu

SHAPES = FR.SHAPES + [(96, 192, 7), (96, 192, 8), (96, 192, 15)]
TILES = {0: (4, 8), 1: (32, 8), 2: (64, 16)}      # cfg -> rows, columns of a workgroup


@functools.lru_cache(maxsize=4)
def sums(wtype, K, M, N, kind="mirror"):
    W, X = FR.case(wtype, K, M, N, kind)
    acc = FR.dots(wtype, W, X)
    acc.setflags(write=False)
    return W, X, acc


def ff(shape):
    return np.full(shape, 0xff, dtype=np.uint8).repeat(4, axis=-1).view(F32)


def check_launch(got, cfg, M, N, what):
    tm, tn = TILES[cfg]
    exp = (256, (M + tm - 1) // tm, (N + tn - 1) // tn, tn * (8192 // tn + 4) * 4) + C.geometry(M, N) + (cfg,)
    assert tuple(got["launched"][:7]) == exp, (what, list(got["launched"]), exp)


def run_stage(pkg, wtype, K, M, N, W, X, acc, cfg):
    cols, ldo = C.geometry(M, N)
    seed = N + 1000 * wtype + K
    for epi in FR.epilogues(K, M):
        args = dict(epi=epi, wtype=wtype, M=M, K=K, N=N, w_rows=W, x=X, cfg=cfg)
        what = (epi, FR.NAMES[wtype], (K, M, N), "cfg %d" % cfg)
        if epi == "QKV":
            H = K // 64
            bias = FR.bias_of(M, seed)
            q, k, v = FR.epi_qkv(acc, bias, K)
            for form in (1, 2) if N > 1 else (1, 0):      # one column per sequence; packed columns of three slots (one column: the context's own)
                st = C.qkv_states(form, N, seed)
                w = {"out": C.whole(q, cols, K, F32)}
                for name, rows in (("k", k), ("v", v)):
                    slots = ff((st["n_slots"], H, st["P"], 64))
                    slots[st["slot"], :, st["pos"], :] = rows.reshape(N, H, 64)
                    w[name] = slots
                a = dict(args, bias=bias, dev_state=st["dev_state"], seq_states=st["seq_states"], col_mode=st["col_mode"], P=st["P"])
                a["k_slots"] = a["v_slots"] = ff((st["n_slots"], H, st["P"], 64))
                got = pkg.fchain_device(**a)
                check_launch(got, cfg, M, N, what + ("states %d" % form,))
                C.compare(got, w, what + ("states %d" % form,))
            continue
        if epi == "LOGITS":
            want = acc
        elif epi == "RESID":
            args["bias"], args["resid"] = FR.bias_of(M, seed), FR.resid_of(N, M, seed)
            want = FR.epi_resid(acc, args["bias"], args["resid"])
        else:
            args["bias"] = FR.bias_of(M, seed, 0.5)
            want = FR.epi_gelu(acc, args["bias"])
        got = pkg.fchain_device(**args)
        check_launch(got, cfg, M, N, what)
        C.compare(got, {"out": C.whole(want, cols, ldo, F32)}, what)
        assert np.isfinite(got["out"][:N, :M]).all(), what


@pytest.mark.parametrize("wtype", FR.TYPES, ids=[FR.NAMES[t] for t in FR.TYPES])
@pytest.mark.parametrize("shape", SHAPES, ids=["K%d_M%d_N%d" % s for s in SHAPES])
def test_stage_equals_the_restatement(pkg, shape, wtype):
    K, M, N = shape
    W, X, acc = sums(wtype, K, M, N)
    for cfg in (0, 1, 2):
        run_stage(pkg, wtype, K, M, N, W, X, acc, cfg)


def test_subnormal_f16_weights(pkg):
    K, M, N = FR.SUB_SHAPE
    W, X, acc = sums(FR.W_F16, K, M, N, "sub")
    assert (np.abs(W.astype(F32)) < 2.0 ** -14).all() and (acc != 0).all()
    for cfg in (0, 1, 2):
        run_stage(pkg, FR.W_F16, K, M, N, W, X, acc, cfg)


def test_the_launch_chooses_its_tile_by_the_grid(pkg):
    """cfg -1: the largest tile that still gives 512 workgroups, else the next smaller one; the same rows whichever it is."""
    for (K, M, N), cfg in (((1024, 3072, 17), 0), ((96, 192, 1), 0), ((1024, 2053, 33), 0)):
        W, X, acc = sums(FR.W_F32, K, M, N)
        got = pkg.fchain_device(epi="LOGITS", wtype=FR.W_F32, M=M, K=K, N=N, w_rows=W, x=X)
        tm, tn = TILES[int(got["launched"][6])]
        grids = {c: -(-M // TILES[c][0]) * -(-N // TILES[c][1]) for c in TILES}
        want = 2 if grids[2] >= 512 else 1 if grids[1] >= 512 else 0
        assert int(got["launched"][6]) == want, ((K, M, N), list(got["launched"]), grids)
        C.compare(got, {"out": C.whole(acc, *C.geometry(M, N), F32)}, ("auto", K, M, N))


@pytest.mark.parametrize("wtype", FR.TYPES, ids=[FR.NAMES[t] for t in FR.TYPES])
def test_layer_norm_producer(pkg, wtype):
    """fchain_ln_kernel on the hostile LayerNorm rows, then the stage on its output: the producer's rows whole (guard column 0xff), and the logits of a small
    matrix of exact rows against the restatement on the restated rows."""
    x = C.ln_rows()
    w, b = C.ln_gain_bias()
    N, K, M = x.shape[0], 1024, 40
    with np.errstate(all="ignore"):
        y = FR.layer_norm(wtype, x, w, b)
    W = np.zeros((M, K), F32 if wtype == FR.W_F32 else np.float16)
    W[np.arange(M), np.arange(M) * 25 % K] = 1.0      # one weight a row: the sum is one product, exact in any order
    with np.errstate(all="ignore"):
        acc = FR.dots(wtype, W, y)
    finite = np.isfinite(y).all(axis=1)
    assert finite.sum() >= N - 1, "at most the 1e18 row leaves the f16 range"
    got = pkg.fchain_device(epi="LOGITS", wtype=wtype, M=M, K=K, N=N, w_rows=W, x=x, ln_w=w, ln_b=b, cfg=0)
    cols, ldo = C.geometry(M, N)
    want_ln = C.whole(y, cols, K, F32)
    assert (got["ln"].view(np.uint32) == want_ln.view(np.uint32)).all(), (FR.NAMES[wtype], np.argwhere(got["ln"].view(np.uint32) != want_ln.view(np.uint32))[:5])
    want = C.whole(acc, cols, ldo, F32)
    rows = np.flatnonzero(finite)
    assert (got["out"][rows].view(np.uint32) == want[rows].view(np.uint32)).all()
    assert (got["out"][N:].view(np.uint32) == 0xffffffff).all() and (got["out"][:, M:].view(np.uint32) == 0xffffffff).all()


def test_refusals_come_before_any_launch(pkg):
    K, M, N = 96, 192, 1
    z = dict(wtype=FR.W_F32, M=M, K=K, N=N, w_rows=np.zeros((M, K), F32), x=np.zeros((N, K), F32), bias=np.zeros(M, F32))
    with pytest.raises(pkg.BiogptError, match="multiple of 32"):
        pkg.fchain_device(epi="GELU", **dict(z, K=100))
    with pytest.raises(pkg.BiogptError, match="no float format"):
        pkg.fchain_device(epi="GELU", **dict(z, wtype=2))
    with pytest.raises(pkg.BiogptError, match="3 K x K"):
        pkg.fchain_device(epi="QKV", dev_state=np.zeros(4, np.int32), P=1, k_slots=np.zeros((1, 1, 1, 64), F32), v_slots=np.zeros((1, 1, 1, 64), F32), **z)
    with pytest.raises(pkg.BiogptError, match="resid is NULL"):
        pkg.fchain_device(epi="RESID", **z)
    with pytest.raises(pkg.BiogptError, match="ln_w and ln_b come together"):
        pkg.fchain_device(epi="GELU", ln_w=np.ones(K, F32), **z)
    with pytest.raises(pkg.BiogptError, match=r"cfg must be in \[-1, 2\]"):
        pkg.fchain_device(epi="GELU", cfg=3, **z)
