"""The SIMD association, restated in numpy float32 as oracle/biogpt_oracle.c computes it with bo_opts.assoc = 3 (the shape of ggml's AVX2 kernels): the Q8
activation rows (quantize_block_q8_avx2), the block dot of the five formats (vec_dot_simd) and the f32 dot of the attention (vec_dot_f32_simd, bo_attn_head with
assoc & 1).  tests/test_assoc_restatement.py holds this file to the oracle on the CPU; tests/test_gpu_assoc_kernels.py holds the kernels of
csrc/kernels_assoc.hip.h to it bit for bit.  Layouts are those of tests/chain_ref.py.

numpy has no float32 fma.  fma32 builds one: the product of two float32 is exact in float64 (48 bits), TwoSum gives the error of adding the third operand,
and a float64 sum rounded to odd rounds to float32 exactly as the infinitely precise a * b + c does (53 >= 2 * 24 + 2)."""
import numpy as np

import chain_ref as R

F32 = np.float32


def fma32(a, b, c):
    """float32 fma(a, b, c) = fl32(a * b + c) with ONE rounding, elementwise."""
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=F32), np.asarray(b, dtype=F32), np.asarray(c, dtype=F32))
    p = a.astype(np.float64) * b.astype(np.float64)
    c64 = c.astype(np.float64)
    s = p + c64
    bb = s - p
    e = (p - (s - bb)) + (c64 - bb)                       # s + e = p + c exactly
    bits = s.view(np.int64).copy()
    fix = (e != 0) & ((bits & 1) == 0)                    # inexact and even: the odd neighbour on the error's side
    step = np.where((e > 0) == (s > 0), 1, -1)
    bits = np.where(fix, bits + step, bits)
    return bits.view(np.float64).astype(F32)


# ---- activation rows ------------------------------------------------------------------------------------------------------------------------------------

def quantize_q8(x, q81):
    """Rows of float32 [..., 32 n] -> (codes int8, d float32, s uint32) in the device layout: d = amax / 127, id = 127 / amax (each one correctly rounded
    division), codes = nearest-even of fl(x * id); Q8_0 keeps d through f16 and the integer sum, Q8_1 the f32 d and the bits of fl(d * sum)."""
    x = np.asarray(x, dtype=F32)
    v = x.reshape(x.shape[:-1] + (x.shape[-1] // 32, 32))
    amax = np.abs(v).max(axis=-1)
    d = (amax / F32(127.0)).astype(F32)
    with np.errstate(divide="ignore"):
        idv = np.where(amax != 0, F32(127.0) / amax, F32(0.0)).astype(F32)
    q = np.rint((v * idv[..., None]).astype(F32)).astype(np.int32)
    isum = q.sum(axis=-1)
    if q81:
        dd, s = d, (d * isum.astype(F32)).astype(F32).view(np.uint32)
    else:
        dd, s = d.astype(np.float16).astype(F32), isum.astype(np.int32).view(np.uint32)
    return q.astype(np.int8).reshape(x.shape), dd, s


def lnq(x, w, b, q81):
    """LayerNorm (tests/chain_ref.py: bo_layer_norm) in front of quantize_q8, row by row."""
    return quantize_q8(np.stack([R.layer_norm(r, w, b) for r in np.asarray(x, dtype=F32)]), q81)


# ---- the block dot -----------------------------------------------------------------------------------------------------------------------------------------

def hsum8(a):
    """[..., 8] -> ((a0+a4)+(a2+a6)) + ((a1+a5)+(a3+a7)), every + a float32 add."""
    r = (a[..., :4] + a[..., 4:]).astype(F32)
    return ((r[..., 0] + r[..., 2]).astype(F32) + (r[..., 1] + r[..., 3]).astype(F32)).astype(F32)


def block_sums(wtype, raw, M, K, aq_q, aq_d, aq_s, rows=None):
    """acc float32 [N, len(rows)]: vec_dot_simd of every chosen weight row (all by default) against every activation column."""
    codes, dw, mw = R.decode_weights(wtype, raw, M, K)
    if rows is not None:
        rows = np.asarray(rows)
        codes, dw, mw = codes[rows], dw[rows], (None if mw is None else mw[rows])
    Rn, nb, N = codes.shape[0], K // 32, aq_q.shape[0]
    xq = np.asarray(aq_q).reshape(N, nb, 32).astype(np.int32)
    xs = aq_s.view(F32) if R.Q81[wtype] else None
    acc = np.zeros((N, Rn, 8), dtype=F32)
    summs = np.zeros((N, Rn), dtype=F32)
    for b in range(nb):
        prod = codes[:, b, :].astype(np.int32)[None, :, :] * xq[:, b, :][:, None, :]                 # [N, R, 32]
        lanes = prod.reshape(N, Rn, 8, 4).sum(axis=-1).astype(F32)                                      # exact integers below 2^17
        d = (dw[:, b][None, :] * aq_d[:, b][:, None]).astype(F32)                                      # F16(d_w) * F16(d_y) / F16(d_w) * d_y
        acc = fma32(d[:, :, None], lanes, acc)
        if mw is not None:
            summs = (summs + (mw[:, b][None, :] * xs[:, b][:, None]).astype(F32)).astype(F32)
    return (hsum8(acc) + summs).astype(F32)


# ---- the f32 dot and the attention ---------------------------------------------------------------------------------------------------------------------------

def reduce32(a):
    """[..., 32] accumulators a[i mod 32] -> 0 += 2, 1 += 3 (vectors of 8), 0 += 1, low + high half, two hadds."""
    a = (a[..., :16] + a[..., 16:]).astype(F32)
    a = (a[..., :8] + a[..., 8:]).astype(F32)
    t = (a[..., :4] + a[..., 4:]).astype(F32)
    return ((t[..., 0] + t[..., 1]).astype(F32) + (t[..., 2] + t[..., 3]).astype(F32)).astype(F32)


def dot_rows(X, y):
    """vec_dot_f32_simd of every row of X [R, n] with y [n]: float32 [R]."""
    X, y = np.asarray(X, dtype=F32), np.asarray(y, dtype=F32)
    n = y.size
    full = n & ~31
    acc = np.zeros((X.shape[0], 32), dtype=F32)
    for i in range(0, full, 32):
        acc = fma32(X[:, i:i + 32], y[None, i:i + 32], acc)
    s = reduce32(acc)
    for i in range(full, n):
        s = (s + (X[:, i] * y[i]).astype(F32)).astype(F32)
    return s


def attn_head(q, K, V, T):
    """bo_attn_head with assoc & 1: q [dk] (already scaled), K / V [rows >= T, dk] -> float32 [dk]."""
    import attn_ref
    q, K, V = np.asarray(q, dtype=F32), np.asarray(K, dtype=F32)[:T], np.asarray(V, dtype=F32)[:T]
    S = dot_rows(K, q)
    mx = S.max()
    with np.errstate(over="ignore"):
        val = attn_ref.exp_table()[(S - mx).astype(F32).astype(np.float16).view(np.uint16)]
    total = 0.0
    for v in val:                                          # (f16 values: the double sum is exact in any order)
        total += float(v)
    p = (val * F32(1.0 / total)).astype(F32)
    return dot_rows(np.ascontiguousarray(V.T), p)
