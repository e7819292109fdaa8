"""The linear stages of the many-column chain, restated in numpy float32 as oracle/biogpt_oracle.c computes them: the integer dot of every 32-element block, the
per-type block term in the order mfma_block_term / unit_dot_quant state, the f32 sum over the blocks in block order, and each epilogue as bo_eval writes it.
tests/test_chain_restatement.py proves on the CPU that this file equals bo_vec_dot_q, bo_layer_norm, bo_quantize and bo_gelu_table; tests/test_gpu_chain_kernels.py
holds the kernels to it bit for bit.  Every function takes `mistake`, the name of one kernel mistake to commit (MISTAKES): the CPU test shows that each is seen.

Layouts.  Weights: M rows of K / 32 blocks in the file's format (Q4_0 18 bytes: d f16, 16 nibble bytes; Q4_1 20: d, m; Q5_0 22: d, qh; Q5_1 24: d, m, qh; Q8_0 34:
d, 32 int8).  Activations, as a producer kernel leaves them: q int8 [N, K], d float32 [N, K / 32], s uint32 [N, K / 32] -- for the Q8_0 consumers (Q4_0, Q5_0, Q8_0
weights) d is the scale rounded through f16 and s the integer block sum; for the Q8_1 consumers d is the f32 scale and s the bits of the float d * sum."""
import numpy as np

Q4_0, Q4_1, Q5_0, Q5_1, Q8_0 = 2, 3, 6, 7, 8
TYPES = (Q4_0, Q4_1, Q5_0, Q5_1, Q8_0)
NAMES = {Q4_0: "q4_0", Q4_1: "q4_1", Q5_0: "q5_0", Q5_1: "q5_1", Q8_0: "q8_0"}
BLOCK_BYTES = {Q4_0: 18, Q4_1: 20, Q5_0: 22, Q5_1: 24, Q8_0: 34}
Q81 = {Q4_0: False, Q4_1: True, Q5_0: False, Q5_1: True, Q8_0: False}
F32 = np.float32
EPS = F32(1e-5)
Q_SCALE = F32(0.125)        # 1 / sqrt(64)

MISTAKES = {
    "dropped_last_block": "the sum stops one block short of the row",
    "previous_tile_scale": "a 16-row tile is scaled by the weight scales of the tile before it",
    "dx_before_dw": "Q4_0: (dot * d_x) * d_w instead of (dot * d_w) * d_x",
    "product_first": "Q8_0: (dot * d_w) * d_x instead of dot * (d_w * d_x)",
    "fused_min_term": "Q4_1 / Q5_1: the min term added with one rounding (fma) instead of a product and a sum",
    "pairwise_sum": "the block terms summed as two halves instead of in block order",
    "nearest_even": "Q8 codes rounded to nearest-even instead of half away from zero",
    "sum_before_f16": "Q8_1: s = sum * d taken from a d rounded through f16; Q8_0: d stored unrounded",
    "clamped_column_stored": "a column clamped to N - 1 is stored: column N - 1's value lands in column N",
    "bias_after_scale": "q rows: acc * q_scale + b instead of (b + acc) * q_scale",
    "resid_first": "(acc + resid) + b instead of (acc + b) + resid",
    "gelu_without_f16": "fc1: the table looked up at a truncated instead of a rounded f16 index",
    "ln_float_sums": "LayerNorm: mean and variance summed in float32 instead of double",
    "ln_scale_first": "LayerNorm: gain * scale first, then the centred value",
}


# ---- formats ------------------------------------------------------------------------------------------------------------------------------------------

def decode_weights(wtype, raw, M, K):
    """File-format rows -> (codes int8/int16 [M, K / 32, 32] as the dot uses them, d float32 [M, K / 32], m float32 [M, K / 32] or None)."""
    bb, nb = BLOCK_BYTES[wtype], K // 32
    b = np.ascontiguousarray(raw, dtype=np.uint8).reshape(M, nb, bb)
    d = b[:, :, 0:2].copy().view(np.float16).astype(F32).reshape(M, nb)
    m = None
    at = 2
    if Q81[wtype]:
        m = b[:, :, 2:4].copy().view(np.float16).astype(F32).reshape(M, nb)
        at = 4
    if wtype == Q8_0:
        return b[:, :, 2:34].copy().view(np.int8).astype(np.int16), d, None
    qh = None
    if wtype in (Q5_0, Q5_1):
        qh = b[:, :, at:at + 4].copy().view("<u4").reshape(M, nb)
        at += 4
    qs = b[:, :, at:at + 16]
    lo, hi = (qs & 0x0F).astype(np.int16), (qs >> 4).astype(np.int16)
    if qh is not None:
        j = np.arange(16, dtype=np.uint32)
        lo |= (((qh[:, :, None] >> j) & 1) << 4).astype(np.int16)
        hi |= (((qh[:, :, None] >> (j + 16)) & 1) << 4).astype(np.int16)
    codes = np.concatenate([lo, hi], axis=2)
    if wtype == Q4_0:
        codes -= 8
    if wtype == Q5_0:
        codes -= 16
    return codes, d, m


def oracle_blocks(q81, q, d, s):
    """One activation row in the device layout -> the bytes of the oracle's blk_q8_0 / blk_q8_1 row."""
    nb = d.size
    if q81:
        b = np.zeros(nb, dtype=np.dtype([("d", "<f4"), ("s", "<f4"), ("q", "i1", 32)]))
        b["d"], b["s"], b["q"] = d, s.view(F32), q.reshape(nb, 32)
    else:
        b = np.zeros(nb, dtype=np.dtype([("d", "<u2"), ("q", "i1", 32)]))
        h = d.astype(np.float16)
        assert (h.astype(F32).view(np.uint32) == d.view(np.uint32)).all(), "a Q8_0 scale is an f16 value"
        b["d"], b["q"] = h.view(np.uint16), q.reshape(nb, 32)
    return b.tobytes()


# ---- the block sums ----------------------------------------------------------------------------------------------------------------------------------

def block_sums(wtype, raw, M, K, aq_q, aq_d, aq_s, rows=None, mistake=None, chunk=64):
    """acc float32 [N, len(rows)]: the reference's vec_dot of every chosen weight row (all by default) against every activation column."""
    codes, dw, mw = decode_weights(wtype, raw, M, K)
    if mistake == "previous_tile_scale":
        t = np.maximum(np.arange(M) // 16 - 1, 0) * 16 + np.arange(M) % 16
        dw = dw[t]
        mw = None if mw is None else mw[t]
    if rows is not None:
        rows = np.asarray(rows)
        codes, dw, mw = codes[rows], dw[rows], (None if mw is None else mw[rows])
    R, nb, N = codes.shape[0], K // 32, aq_q.shape[0]
    wf = np.ascontiguousarray(codes.transpose(1, 0, 2), dtype=F32)               # [nb, R, 32]
    dwT = np.ascontiguousarray(dw.T)                                             # [nb, R]
    mwT = None if mw is None else np.ascontiguousarray(mw.T)
    xs = aq_s.view(F32) if Q81[wtype] else None
    out = np.zeros((N, R), dtype=F32)
    last = nb - 1 if mistake == "dropped_last_block" else nb
    for c0 in range(0, N, chunk):
        c1 = min(N, c0 + chunk)
        xf = np.ascontiguousarray(aq_q[c0:c1].reshape(c1 - c0, nb, 32).transpose(1, 2, 0), dtype=F32)       # [nb, 32, n]
        dots = np.matmul(wf, xf)            # [nb, R, n]: integers below 2^24, exact in float32 whatever the order
        terms = []
        for b in range(last):
            dot, d_w, d_x = dots[b], dwT[b][:, None], aq_d[c0:c1, b][None, :]
            if wtype == Q8_0:
                t = (dot * d_w) * d_x if mistake == "product_first" else dot * (d_w * d_x)
            elif wtype == Q4_0:
                t = (dot * d_x) * d_w if mistake == "dx_before_dw" else (dot * d_w) * d_x
            elif wtype == Q5_0:
                t = (d_w * d_x) * dot
            else:
                if mistake == "fused_min_term":
                    t = ((d_w * d_x).astype(np.float64) * dot + mwT[b][:, None].astype(np.float64) * xs[c0:c1, b][None, :]).astype(F32)
                else:
                    t = (d_w * d_x) * dot + mwT[b][:, None] * xs[c0:c1, b][None, :]
            terms.append(t.astype(F32))
        if mistake == "pairwise_sum":
            h = [np.zeros((R, c1 - c0), dtype=F32), np.zeros((R, c1 - c0), dtype=F32)]
            for b, t in enumerate(terms):
                h[b >= len(terms) // 2] = h[b >= len(terms) // 2] + t
            acc = h[0] + h[1]
        else:
            acc = np.zeros((R, c1 - c0), dtype=F32)
            for t in terms:
                acc = acc + t
        out[c0:c1] = acc.T
    return out


# ---- quantize_row_q8_0 / _q8_1 and LayerNorm -----------------------------------------------------------------------------------------------------------

def quantize_q8(x, q81, mistake=None):
    """Rows of float32 [..., 32 n] -> (codes int8, d float32, s uint32) in the device layout."""
    x = np.asarray(x, dtype=F32)
    v = x.reshape(x.shape[:-1] + (x.shape[-1] // 32, 32))
    amax = np.abs(v).max(axis=-1)
    d = (amax / F32(127.0)).astype(F32)
    with np.errstate(divide="ignore"):
        idv = np.where(d != 0, F32(1.0) / d, F32(0.0)).astype(F32)
    with np.errstate(invalid="ignore"):      # (a committed mistake may leave the f16 range; no committed case does)
        t = (v * idv[..., None]).astype(F32).astype(np.float64)
        r = np.rint(t) if mistake == "nearest_even" else np.trunc(t + np.copysign(0.5, t))
        q = r.astype(np.int32)
    isum = q.sum(axis=-1)
    dh = d.astype(np.float16).astype(F32)
    if q81:
        s = (isum.astype(F32) * (dh if mistake == "sum_before_f16" else d)).astype(F32).view(np.uint32)
        dd = d
    else:
        s, dd = isum.astype(np.int32).view(np.uint32), (d if mistake == "sum_before_f16" else dh)
    return q.astype(np.int8).reshape(x.shape), dd, s


def _seq_sum(a, dtype):
    with np.errstate(over="ignore"):
        return np.add.accumulate(a.astype(dtype), dtype=dtype)[-1]      # one element after another, as the reference's loop


def layer_norm(x, w, b, mistake=None):
    """One row, as bo_layer_norm: double sums, (x - mean) * scale, * w, + b."""
    x, w, b = (np.asarray(a, dtype=F32) for a in (x, w, b))
    acc_t = F32 if mistake == "ln_float_sums" else np.float64
    n = x.size
    mean = F32(_seq_sum(x, acc_t) / acc_t(n))
    v = (x - mean).astype(F32)
    var = F32(_seq_sum((v * v).astype(F32), acc_t) / acc_t(n))
    scale = F32(1.0) / np.sqrt(F32(var + EPS), dtype=F32)
    if mistake == "ln_scale_first":
        return ((w * scale).astype(F32) * v + b).astype(F32)
    return ((w * (v * scale).astype(F32)).astype(F32) + b).astype(F32)


def ln_fragile(x):
    """True when the association of the double sums could decide a float32 of the row's mean or variance: the exact sums (Python integers over the floats'
    binary expansions) rounded once differ from the sequential double sums' float32, or a float32 rounding border lies within the double sums' error bound."""
    from fractions import Fraction
    x = np.asarray(x, dtype=F32)
    n = x.size
    fx = [Fraction(float(t)) for t in x]
    s_exact = sum(fx)
    s_seq = float(_seq_sum(x, np.float64))
    mean = F32(s_seq / n)
    if F32(float(s_exact / n)) != mean or _near_border(s_exact / n, sum(abs(t) for t in fx) / n, n):
        return True
    v = (x - mean).astype(F32)
    sq = (v * v).astype(F32)
    fq = [Fraction(float(t)) for t in sq]
    q_exact = sum(fq)
    var = F32(float(_seq_sum(sq, np.float64)) / n)
    return bool(F32(float(q_exact / n)) != var or _near_border(q_exact / n, q_exact / n, n))


def _near_border(value, magnitude, n):
    """A float32 rounding border within n * 2^-53 * magnitude of value (the worst error of n double additions in any order)."""
    from fractions import Fraction
    err = Fraction(n, 2 ** 53) * magnitude
    lo, hi = F32(float(value - err)), F32(float(value + err))
    return bool(lo != hi)


def lnq(x, w, b, q81, mistake=None):
    """lnq_kernel: rows [N, 1024] -> (codes, d, s) [N, ...]."""
    y = np.stack([layer_norm(r, w, b, mistake) for r in np.asarray(x, dtype=F32)])
    return quantize_q8(y, q81, mistake)


# ---- the GELU table and the epilogues -------------------------------------------------------------------------------------------------------------------

_TABLE = None


def gelu_table():
    """float32 [65536]: table[h] = f16(gelu(f16 value h)) as ggml_init builds it -- the tanh form in float32 arithmetic, with the C library's tanhf (numpy's
    float32 tanh differs from it in the last bit often enough to move 235 entries)."""
    global _TABLE
    if _TABLE is None:
        import ctypes
        import ctypes.util
        tanhf = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6").tanhf
        tanhf.restype, tanhf.argtypes = ctypes.c_float, [ctypes.c_float]
        x = np.arange(65536, dtype=np.uint16).view(np.float16).astype(F32)
        with np.errstate(all="ignore"):
            inner = ((F32(0.79788456080286535587989211986876) * x).astype(F32) * (F32(1.0) + (F32(0.044715) * x).astype(F32) * x).astype(F32)).astype(F32)
            th = np.array([tanhf(float(v)) for v in inner], dtype=F32)
            g = ((F32(0.5) * x).astype(F32) * (F32(1.0) + th).astype(F32)).astype(F32)
            _TABLE = g.astype(np.float16).astype(F32)
    return _TABLE


def _f16_index(v, mistake=None):
    with np.errstate(over="ignore"):
        if mistake == "gelu_without_f16":       # round toward zero: drop the bits below f16's
            h = v.astype(np.float16)
            up = np.abs(h.astype(F32)) > np.abs(v)
            h = np.where(up, np.nextafter(h, np.float16(0)), h).astype(np.float16)
            return h.view(np.uint16)
        return v.astype(np.float16).view(np.uint16)


def epi_qkv(acc, bias, mistake=None):
    """[N, 3072] -> (q [N, 1024], k [N, 1024], v [N, 1024])."""
    if mistake == "bias_after_scale":
        q = ((acc[:, :1024] * Q_SCALE).astype(F32) + bias[None, :1024]).astype(F32)
    else:
        q = ((bias[None, :1024] + acc[:, :1024]).astype(F32) * Q_SCALE).astype(F32)
    kv = (bias[None, 1024:] + acc[:, 1024:]).astype(F32)
    return q, kv[:, :1024], kv[:, 1024:]


def epi_resid(acc, bias, resid, mistake=None):
    if mistake == "resid_first":
        return ((acc + resid).astype(F32) + bias[None, :]).astype(F32)
    return ((acc + bias[None, :]).astype(F32) + resid).astype(F32)


def epi_gelu_q8(acc, bias, q81, mistake=None):
    """[N, 4096] -> fc2's activation blocks (codes [N, 4096], d, s [N, 128])."""
    g = gelu_table()[_f16_index((bias[None, :] + acc).astype(F32), mistake)]
    return quantize_q8(g, q81, mistake), g
