"""Pooling, L2 normalisation and the linear head of biogpt_hip_embed_batch, restated in numpy float64 on given hidden rows (what the engine's
pool_rows_kernel / pool_finish_kernel / head_rows_kernel are held to), and the error bounds that follow from the engine's arithmetic:
double sums of f32 terms (or of exact f32 x f32 products), rounded to f32 once.

Pinned to transformers (BioGptForSequenceClassification, BioGptForTokenClassification, the masked mean of last_hidden_state) by
test_embed_restatement.py."""
import numpy as np

EPS32 = 2.0 ** -23      # spacing of f32 relative to the value: covers one rounding to f32 (half of it, rounded to nearest)
EPS64 = 2.0 ** -50      # per-term allowance of a double sum (8 x the unit roundoff 2^-53: any order, with the division / square root beside it)


def pool(rows, pooling):
    """rows: [len, width] hidden rows of ONE sequence.  pooling 'none' -> the rows, 'last' -> row len - 1, 'mean' -> the mean over the rows; float64."""
    r = np.asarray(rows, dtype=np.float64)
    if pooling == "none":
        return r
    if pooling == "last":
        return r[-1]
    if pooling == "mean":
        return r.sum(axis=0) / r.shape[0]
    raise ValueError(pooling)


def l2_normalize(x):
    """x / ||x||_2 along the last axis in float64; a zero row stays zero."""
    x = np.asarray(x, dtype=np.float64)
    n = np.sqrt((x * x).sum(axis=-1, keepdims=True))
    return np.where(n == 0.0, x, x / np.where(n == 0.0, 1.0, n))


def head(x, w, b=None):
    """out[..., o] = b[o] + sum_d w[o, d] * x[..., d] in float64."""
    out = np.asarray(x, dtype=np.float64) @ np.asarray(w, dtype=np.float64).T
    return out if b is None else out + np.asarray(b, dtype=np.float64)


def embed(rows, pooling="last", normalize=False, w=None, b=None):
    """The whole of embed_batch for one sequence's hidden rows, in float64 throughout.  (The engine rounds the pooled row to f32 before it
    normalises it or applies the head -- the pooled row is an output of its own -- so test_gpu_embed.py checks stage by stage: each stage's
    restatement on the engine's own f32 input of that stage.)"""
    x = pool(rows, pooling)
    if normalize:
        x = l2_normalize(x)
    if w is not None:
        x = head(x, w, b)
    return x


# ---- bounds: |engine - restatement| of each stage, from the arithmetic alone ----

def mean_bound(rows):
    """(float)(double sum of n f32 terms / n) against the float64 mean: one f32 rounding of the result (EPS32 * |ref|) + the error of the
    double sum, n * EPS64 * sum |terms|, divided by n with it."""
    r = np.abs(np.asarray(rows, dtype=np.float64))
    n = r.shape[0]
    return EPS32 * np.abs(pool(rows, "mean")) + n * EPS64 * r.sum(axis=0) / n


def normalize_bound(x):
    """(float)(x / sqrt(double sum of squares)) against float64: one f32 rounding of the result + the sum's error carried through the quotient
    (relative error of the sum of width non-negative terms <= width * EPS64; of its square root, and of the quotient, no more)."""
    x = np.asarray(x, dtype=np.float64)
    ref = np.abs(l2_normalize(x))
    return EPS32 * ref + x.shape[-1] * EPS64 * ref


def head_bound(x, w, b=None):
    """(float)(b + double sum of d_model exact products) against float64: one f32 rounding of the result + d_model * EPS64 * (sum_d |w x| + |b|),
    per output."""
    mag = np.abs(np.asarray(x, dtype=np.float64)) @ np.abs(np.asarray(w, dtype=np.float64)).T
    if b is not None:
        mag = mag + np.abs(np.asarray(b, dtype=np.float64))
    return EPS32 * np.abs(head(x, w, b)) + np.shape(x)[-1] * EPS64 * mag
