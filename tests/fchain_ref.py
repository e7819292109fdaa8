"""The float chain's linear stage (csrc/kernels_fchain.hip.h), restated in numpy as oracle/biogpt_oracle.c computes a float mat-vec (vec_dot_f32 / vec_dot_f16):
every product rounded to float32, the running sum in double one element after another, one rounding to float32 at the end; with F16 weights the activation row
is first rounded through float16.  The LayerNorm producer is chain_ref.layer_norm (and the float16 rounding for F16 files), the epilogues are chain_ref's.
tests/test_fchain_restatement.py holds this file to oracle.vec_dot on the CPU; tests/test_gpu_fchain_kernels.py holds the kernels to it bit for bit.

The kernel's association of the double sum is its own (a K-split over lanes and a butterfly), so a bit-for-bit comparison needs rows whose double sum is EXACT in
any order.  case() builds them:
  * every weight and activation is sign * (1.f) * 2^e with a random 24-bit significand (11-bit for F16 weights) and e in [-4, 4): a float32 product lies in
    [2^-8, 2^8) with its last bit at 2^-31 or above, a sum of at most 4096 of them stays below 2^20 -- 51 bits, inside a double's 53, whatever the order;
  * the second half of every activation column repeats the first, the second half of every weight row is the first with the sign flipped, except for three
    terms: the products cancel pair by pair and the result is a small remainder of large terms (an f32 accumulator loses it);
  * row groups with +-0.0 weights (whole rows, and pairs inside mirrored rows), and a column with +-0.0 activations: zeros add nothing to the span;
  * kind "sub" (F16): every weight a subnormal float16 (k * 2^-24, 1 <= k < 1024) against activations in [1, 2): a product has at most 21 significant bits at
    2^-34 or above and stays below 2^-13, the sum below 2^-1 -- 33 bits.
span_bits() checks the argument on the actual products of every output."""
import functools

import numpy as np

import chain_ref as R

F32, F64 = np.float32, np.float64
W_F32, W_F16 = 0, 1
TYPES = (W_F32, W_F16)
NAMES = {W_F32: "f32", W_F16: "f16"}
SHAPES = [(1024, 3072, 17), (4096, 1024, 16), (1600, 1600, 9), (96, 192, 1), (1024, 2053, 33)]      # (K, M, N): the issue's
SUB_SHAPE = (1024, 64, 9)                                                                            # the subnormal-weight group (F16)

MISTAKES = {
    "f32_accumulator": "the running sum kept in float32 instead of double",
    "fused_product": "the product not rounded to float32 (an fma into the double sum)",
    "no_f16_rounding": "F16 weights: the activation row not rounded through float16",
    "resid_grouping": "the residual epilogue as v + (bias + resid) instead of (v + bias) + resid",
}


def _rng(*key):
    return np.random.default_rng([0x46434841] + [int(k) for k in key])


def _values(g, shape, bits):
    """sign * (1 + m / 2^(bits - 1)) * 2^e: a random `bits`-bit significand, e in [-4, 4)."""
    m = g.integers(0, 1 << (bits - 1), shape).astype(F64) / F64(1 << (bits - 1))
    e = g.integers(-4, 4, shape).astype(F64)
    s = g.integers(0, 2, shape).astype(F64) * 2.0 - 1.0
    return (s * (1.0 + m) * np.exp2(e)).astype(F32)


def _zeros(g, shape):
    return np.where(g.integers(0, 2, shape) == 1, F32(0.0), F32(-0.0)).astype(F32)


@functools.lru_cache(maxsize=None)
def case(wtype, K, M, N, kind="mirror"):
    """-> (W [M, K] float32 or float16, X [N, K] float32), read-only."""
    g = _rng(wtype, K, M, N, 0 if kind == "mirror" else 1)
    h = K // 2
    if kind == "sub":
        assert wtype == W_F16
        k = g.integers(1, 1024, (M, K)).astype(np.uint16) | (g.integers(0, 2, (M, K)).astype(np.uint16) << 15)
        W = k.view(np.float16)
        X = (1.0 + g.integers(0, 1 << 23, (N, K)).astype(F64) / F64(1 << 23)).astype(F32)
    else:
        bits = 24 if wtype == W_F32 else 11
        X = np.empty((N, K), F32)
        X[:, :h] = _values(g, (N, h), 24)
        X[:, h:] = X[:, :h]
        Wf = np.empty((M, K), F32)
        Wf[:, :h] = _values(g, (M, h), bits)
        Wf[:, h:] = -Wf[:, :h]
        for r in range(M):      # three terms of the second half are their own
            at = h + g.choice(h, 3, replace=False)
            Wf[r, at] = _values(g, 3, bits)
        for r in range(5, M, 16):      # +-0.0 inside a mirrored row: both members of a pair
            at = g.choice(h, max(1, h // 4), replace=False)
            Wf[r, at] = _zeros(g, at.size)
            Wf[r, at + h] = _zeros(g, at.size)
        if M > 9:
            Wf[7], Wf[9] = F32(-0.0), F32(0.0)
        if N > 1:      # a column with +-0.0 activations, pair by pair
            at = g.choice(h, max(1, h // 4), replace=False)
            X[1, at] = _zeros(g, at.size)
            X[1, at + h] = X[1, at]
        W = Wf if wtype == W_F32 else Wf.astype(np.float16)
        assert (W.astype(F32) == Wf).all()
    W.setflags(write=False)
    X.setflags(write=False)
    return W, X


def activation(wtype, X, mistake=None):
    """The row the dot reads: rounded through float16 for F16 weights (ggml's fp32_to_fp16_row)."""
    X = np.asarray(X, dtype=F32)
    if wtype == W_F16 and mistake != "no_f16_rounding":
        return X.astype(np.float16).astype(F32)
    return X


def products(wtype, W, x, mistake=None):
    """[rows, K]: the terms of the sums of weight rows W against ONE activation row x (already through activation()), as doubles."""
    Wf = np.asarray(W).astype(F32)
    if mistake == "fused_product":
        return Wf.astype(F64) * x.astype(F64)[None, :]      # exact in double
    return (Wf * x[None, :]).astype(F32).astype(F64)


def dots(wtype, W, X, rows=None, mistake=None):
    """[N, rows] float32: vec_dot of every weight row (or of `rows`) against every column."""
    W = np.asarray(W)
    if rows is not None:
        W = W[rows]
    xs = activation(wtype, X, mistake)
    out = np.empty((xs.shape[0], W.shape[0]), F32)
    acc_t = F32 if mistake == "f32_accumulator" else F64
    for c in range(xs.shape[0]):
        p = products(wtype, W, xs[c], mistake)
        p = np.concatenate([np.zeros((p.shape[0], 1), acc_t), p.astype(acc_t)], axis=1)            # sumf = 0.0; then one element after another
        out[c] = np.add.accumulate(p, axis=1, dtype=acc_t)[:, -1].astype(F32)
    return out


def span_bits(wtype, W, X):
    """The widest window, over all outputs, that the partial sums of an output's products can occupy in ANY order: from the last bit of the smallest product's
    float32 to the top bit of the sum of the magnitudes.  <= 53: every order gives the same double."""
    xs = activation(wtype, X)
    worst = 0
    for c in range(xs.shape[0]):
        p = np.abs(products(wtype, W, xs[c]))
        _, e = np.frexp(p)                                   # p = m * 2^e, 0.5 <= m < 1: the float32's last bit is 2^(e - 24)
        lo = np.where(p > 0, e - 24, 1 << 20).min(axis=1)
        _, hi = np.frexp(p.sum(axis=1))                      # the sum of the magnitudes lies below 2^hi
        live = lo < (1 << 20)
        if live.any():
            worst = max(worst, int((hi[live] + 1 - lo[live]).max()))
    return worst


def layer_norm(wtype, x, w, b, mistake=None):
    """fchain_ln_kernel: rows [N, K] -> rows [N, K]; chain_ref.layer_norm, and the float16 rounding for F16 files."""
    y = np.stack([R.layer_norm(r, w, b, mistake) for r in np.asarray(x, dtype=F32)])
    return activation(wtype, y)


def epi_qkv(acc, bias, D):
    """chain_ref.epi_qkv at d_model D: q = (b + acc) * (1 / sqrt(64)), k and v = b + acc."""
    q = ((bias[None, :D] + acc[:, :D]).astype(F32) * R.Q_SCALE).astype(F32)
    kv = (bias[None, D:] + acc[:, D:]).astype(F32)
    return q, kv[:, :D], kv[:, D:]


def epi_resid(acc, bias, resid, mistake=None):
    if mistake == "resid_grouping":
        return (acc + (bias[None, :] + resid).astype(F32)).astype(F32)
    return R.epi_resid(acc, bias, resid)


def epi_gelu(acc, bias):
    pre = (bias[None, :] + acc).astype(F32)
    assert np.isfinite(pre).all() and np.abs(pre).max() < 65504.0, "the case stays inside the f16 range"
    return R.gelu_table()[R._f16_index(pre)]


def bias_of(M, seed, scale=0.1):
    return (_rng(8, seed, M).standard_normal(M, dtype=F32) * F32(scale)).astype(F32)


def resid_of(N, M, seed):
    return _rng(9, seed, M).standard_normal((N, M), dtype=F32)


def epilogues(K, M):
    e = []
    if M == 3 * K and K % 64 == 0:
        e.append("QKV")
    return e + ["RESID", "GELU", "LOGITS"]
