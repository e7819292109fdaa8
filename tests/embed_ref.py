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


def subnormal_allowance():
    """Half the spacing of float32 below its normal range, 2^-150: there the spacing is 2^-149 whatever the value, so the bounds' relative term EPS32 * |ref| does
    not cover the one rounding to float32.  Added ONLY where a float32 result of the subnormal row kind is compared with float64 (tests/test_embed_kernels_capi.py)."""
    return 2.0 ** -150


# ---- the four kernels restated exactly: float32 bits out --------------------------------------------------------------------------------------------------
# ln_rows_kernel, pool_rows_kernel + pool_finish_kernel and head_rows_kernel compute double sums of f32 terms (or of exact f32 x f32 products) and round once.
# On terms whose double sum is exact in any order (exact_in_any_order) the result is known bit for bit; elsewhere the sum is taken exactly (math.fsum) and the
# kernel is held to the *_bound functions above.  Every function takes `mistake`, the name of one kernel mistake to commit (MISTAKES):
# tests/test_embed_kernels_capi.py shows that each is seen by a case of tests/embed_cases.py.
import math  # noqa: E402

import chain_ref  # noqa: E402

F32 = np.float32
GUARD = np.frombuffer(b"\xff" * 4, dtype=np.float32)[0]      # what the probe presets its outputs to

MISTAKES = {
    "mean_f32_sum": "the mean's sum accumulated in float32 instead of double",
    "mean_pass_count": "the mean divided by the column count of the sequence's last pass instead of its length",
    "mean_drop_16th": "every 16th row of a sequence (positions 15, 31, ...) missing from the mean",
    "mean_drop_pass_head": "the first row of a sequence in its second and later passes missing from the mean",
    "last_minus_2": "LAST taken from position len - 2",
    "norm_sqrtf": "the norm's square root taken in float32",
    "norm_unrounded_mean": "the unrounded double mean normalised instead of the float32 mean",
    "head_f32_products": "the head's products rounded to float32 before the double sum",
    "head_pad_last_row": "the padded rows of the head's last row group take row n_rows - 1 and are stored: row n_rows - 1 lands in the row behind the output",
    "head_drop_chunk": "the head's 16-byte chunks 64 .. W / 4 - 1 (elements from 256) missing from the sum",
    "head_bias_f32": "the head's bias added in float32 after the sum was rounded",
    "ln_var_e2": "LayerNorm: the variance as E[x^2] - mean^2",
    "ln_fused": "LayerNorm: gain and bias applied as one fused multiply-add",
    "ln_no_slot_div": "the scattered LayerNorm row computed from seq_id, not seq_id / slot_div",
}


def exact_in_any_order(terms):
    """terms: [n_terms, ...] float64, summed along axis 0.  True where all terms of a sum are multiples of one 2^q and sum |terms| < 2^(q + 53): every partial
    sum, in any order and any grouping, is then a multiple of 2^q below 2^(q + 53), that is, a double: the double sum is exact.  Returns a bool array over the
    remaining axes (a bool for one sum)."""
    t = np.abs(np.asarray(terms, dtype=np.float64))
    t = t.reshape(t.shape[0], -1)
    if not np.isfinite(t).all():
        return np.zeros(np.shape(terms)[1:], bool)
    m, e = np.frexp(t)
    M = np.ldexp(m, 53).astype(np.int64)                                   # |term| = M * 2^(e - 53), exactly
    low = (M & -M).astype(np.float64)                                      # the lowest set bit of M
    q_term = np.where(t == 0.0, 1 << 20, e - 53 + np.frexp(low)[1] - 1)    # a term is a multiple of 2^q_term, of no higher power
    q = q_term.min(axis=0)
    scaled = np.ldexp(t, -np.where(q == 1 << 20, 0, q))                    # integers: |term| / 2^q (exact: a power of two)
    ok = (scaled < 2.0 ** 53).all(axis=0) & (scaled.sum(axis=0) < 2.0 ** 53)      # (non-negative integers: a true sum below 2^53 is summed exactly)
    return ok.reshape(np.shape(terms)[1:])


def exact_sum(terms):
    """The sum along axis 0 of float64 terms, exactly, rounded to double once (math.fsum); +0.0 for a sum of zeros of either sign, as a sum that starts at +0.0."""
    t = np.asarray(terms, dtype=np.float64)
    flat = t.reshape(t.shape[0], -1)
    if bool(np.all(exact_in_any_order(flat))):
        return flat.sum(axis=0).reshape(t.shape[1:]) + 0.0
    return np.array([math.fsum(col) for col in flat.T.tolist()], dtype=np.float64).reshape(t.shape[1:]) + 0.0


def _f32_seq_sum(terms):
    return np.add.accumulate(np.asarray(terms, dtype=F32), axis=0, dtype=F32)[-1]


def layer_norm_rows(x, w, b, states=None, slot_div=1, P=1, n_out_rows=None, mistake=None):
    """ln_rows_kernel over x [N, W]: chain_ref.layer_norm of every row (any width), row i at (seq_id / slot_div) * P + n_past of the output when states [N, 8]
    (n_past in word 0, seq_id in word 3) are given.  Returns float32 [n_out_rows + 1, W]: unwritten rows and the guard row keep the 0xff preset."""
    x = np.asarray(x, dtype=F32)
    N, W = x.shape
    rows = []
    for r in x:
        if mistake in ("ln_var_e2", "ln_fused"):
            rows.append(_layer_norm_mistaken(r, w, b, mistake))
        else:
            rows.append(chain_ref.layer_norm(r, w, b))
    if states is None:
        at = list(range(N))
        n_out_rows = N
    else:
        st = np.asarray(states, dtype=np.int64)
        at = [int((s[3] if mistake == "ln_no_slot_div" else s[3] // slot_div) * P + s[0]) for s in st]
    out = np.full((max(n_out_rows, max(at) + 1) + 1, W), GUARD, dtype=F32)
    for i, r in zip(at, rows):
        out[i] = r
    return out


def _layer_norm_mistaken(x, w, b, mistake):
    x, w, b = (np.asarray(a, dtype=F32) for a in (x, w, b))
    n = x.size
    mean = F32(float(np.add.accumulate(x.astype(np.float64))[-1]) / n)
    v = (x - mean).astype(F32)
    if mistake == "ln_var_e2":
        ex2 = F32(float(np.add.accumulate((x * x).astype(F32).astype(np.float64))[-1]) / n)
        var = F32(ex2 - F32(mean * mean))
    else:
        var = F32(float(np.add.accumulate((v * v).astype(F32).astype(np.float64))[-1]) / n)
    with np.errstate(invalid="ignore", divide="ignore"):
        scale = F32(1.0) / np.sqrt(F32(var + chain_ref.EPS), dtype=F32)
    t = (v * scale).astype(F32)
    if mistake == "ln_fused":
        return (w.astype(np.float64) * t.astype(np.float64) + b.astype(np.float64)).astype(F32)      # (the product is exact in double: one rounding of w t + b)
    return ((w * t).astype(F32) + b).astype(F32)


def normalize_rows(x, mistake=None, unrounded=None):
    """pool_finish_kernel's normalisation of float32 rows [n, W]: (float)(x / sqrt(double sum of squares)); a zero row stays as it is, signs of zero included."""
    x = np.asarray(x, dtype=F32)
    src = x.astype(np.float64) if unrounded is None else np.asarray(unrounded, dtype=np.float64)
    ss = exact_sum((src * src).T)
    out = x.copy()
    for r in range(x.shape[0]):
        if ss[r] == 0.0:
            continue
        with np.errstate(all="ignore"):
            nrm = float(np.sqrt(F32(ss[r]))) if mistake == "norm_sqrtf" else math.sqrt(ss[r])
            out[r] = (src[r] / nrm).astype(F32)
    return out


def pool_stage(x, states, pass_cols, lens, pooling, normalize=False, mistake=None):
    """The POOL stage over the passes' rows x [n_rows, W] (pass p: pass_cols[p] rows), states [n_rows, 8] (n_past in word 0, seq_id in word 3), lens [n_seqs].
    'last': the row at position len - 1; 'mean': acc = the double sum of a sequence's rows over all passes, out = (float)(acc / len); 'none': the rows.  normalize:
    normalize_rows of the result.  Returns (out float32 [rows + 1, W], acc float64 [n_seqs + 1, W] or None), guard rows and unwritten rows 0xff."""
    x = np.asarray(x, dtype=F32)
    n_rows, W = x.shape
    if pooling == "none":
        out = np.full((n_rows + 1, W), GUARD, dtype=F32)
        out[:n_rows] = normalize_rows(x, mistake) if normalize else x
        return out, None
    st = np.asarray(states, dtype=np.int64)
    seq, pos = st[:, 3], st[:, 0]
    n_seqs = len(lens)
    out = np.full((n_seqs + 1, W), GUARD, dtype=F32)
    written = np.zeros(n_seqs, bool)
    if pooling == "last":
        for i in range(n_rows):
            want = lens[seq[i]] - (2 if mistake == "last_minus_2" and lens[seq[i]] > 1 else 1)
            if pos[i] == want:
                out[seq[i]], written[seq[i]] = x[i], True
        acc = None
        unrounded = None
    elif pooling == "mean":
        pass_of = np.repeat(np.arange(len(pass_cols)), pass_cols)
        acc = np.frombuffer(b"\xff" * (8 * (n_seqs + 1) * W), dtype=np.float64).reshape(n_seqs + 1, W).copy()
        unrounded = np.zeros((n_seqs, W), np.float64)
        for s in range(n_seqs):
            mine = np.flatnonzero(seq == s)
            keep = list(mine)
            if mistake == "mean_drop_16th":
                keep = [i for i in mine if pos[i] % 16 != 15]
            elif mistake == "mean_drop_pass_head" and len(mine):
                first = pass_of[mine[0]]
                keep = [i for i in mine if pass_of[i] == first or (i > 0 and seq[i - 1] == s and pass_of[i - 1] == pass_of[i])]
            if mistake == "mean_f32_sum":
                a = _f32_seq_sum(x[keep]).astype(np.float64) if len(keep) else np.zeros(W)
            else:
                a = exact_sum(x[keep].astype(np.float64)) if len(keep) else np.zeros(W)
            acc[s] = a
            div = float(pass_cols[pass_of[mine[-1]]]) if mistake == "mean_pass_count" and len(mine) else float(lens[s])
            unrounded[s] = a / div
            out[s], written[s] = unrounded[s].astype(F32), True
    else:
        raise ValueError(pooling)
    if normalize:
        w = np.flatnonzero(written)
        out[w] = normalize_rows(out[w], mistake, unrounded[w] if mistake == "norm_unrounded_mean" and unrounded is not None else None)
    return out, acc


def head_stage(x, w, b=None, mistake=None):
    """head_rows_kernel: out[r][o] = (float)(b[o] + the double sum over d of the exact products w[o][d] x[r][d]); float32 [n_rows + 1, n_out] with the guard row."""
    x, w = np.asarray(x, dtype=F32), np.asarray(w, dtype=F32)
    n_rows, W = x.shape
    n_out = w.shape[0]
    if mistake == "head_drop_chunk":
        x, w = x[:, :256], w[:, :256]
    if mistake == "head_f32_products":
        with np.errstate(over="ignore", under="ignore"):
            terms = (w.T[:, None, :] * x.T[:, :, None]).astype(F32).astype(np.float64)      # [d, r, o]
    else:
        terms = w.T.astype(np.float64)[:, None, :] * x.T.astype(np.float64)[:, :, None]
    t = exact_sum(terms)
    bo = np.zeros(n_out, np.float64) if b is None else np.asarray(b, dtype=F32).astype(np.float64)
    out = np.full((n_rows + 1, n_out), GUARD, dtype=F32)
    if mistake == "head_bias_f32":
        out[:n_rows] = (t.astype(F32) + bo.astype(F32)).astype(F32)
    else:
        out[:n_rows] = (bo + t).astype(F32)
    if mistake == "head_pad_last_row" and n_rows % 8 != 0:
        out[n_rows] = out[n_rows - 1]
    return out
