"""A float64 numpy restatement of one row of score_stats_rows_kernel / score_compare_rows_kernel (kernels_score_stats.hip.h), and the bound the tests
hold entropy and KL to.  Not a test module: a helper the tests import."""
import numpy as np


def tolerance(ref):
    """A double sum of up to 57717 terms in any order is within n * 2^-53 = 6.4e-12 of the sum of the terms' magnitudes; one f32 rounding follows."""
    return 2.0 ** -23 * np.abs(ref) + 1e-9


def shifted(row, order=None):
    """(d = l - max, e = exp(d), S) of an f32 row in float64; order: a permutation the sum is taken in."""
    r = np.asarray(row, dtype=np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        d = r - (np.nanmax(r) if not np.isnan(r).all() else -np.inf)
        e = np.exp(d)
    o = np.arange(r.size) if order is None else order
    return d, e, float(np.add.reduce(e[o]))


def weighted(e, x, order=None):
    """sum_v e_v x_v without the terms of weight 0."""
    o = np.arange(e.size) if order is None else order
    with np.errstate(invalid="ignore"):
        t = np.where(e[o] != 0.0, e[o] * x[o], 0.0)
    return float(np.add.reduce(t))


def row_stats(row, target, K, order=None):
    """dict(top_ids [K], top_lp [K] float64, rank, entropy float64) of one row; (-1, 0) for entries the row does not have."""
    r = np.asarray(row, dtype=np.float32)
    d, e, S = shifted(r, order)
    with np.errstate(divide="ignore", invalid="ignore"):
        H = np.log(S) - weighted(e, d, order) / S
        lp = d - np.log(S)
    ids = [int(i) for i in np.argsort(-r.astype(np.float64), kind="stable") if r[i] == r[i]][:K]      # value descending, lower id first, NaN never
    top_ids = np.array(ids + [-1] * (K - len(ids)), dtype=np.int64)
    top_lp = np.array([lp[i] for i in ids] + [0.0] * (K - len(ids)))
    rank = -1
    if target >= 0 and r[target] == r[target]:
        rank = int((r > r[target]).sum() + (r[:target] == r[target]).sum())
    return dict(top_ids=top_ids, top_lp=top_lp, rank=rank, entropy=H)


def row_kl(p, q, order=None):
    """(KL(P || Q), KL(Q || P)) of two rows' softmax distributions in float64, the kernel's expression."""
    dp, ep, Sp = shifted(p, order)
    dq, eq, Sq = shifted(q, order)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (weighted(ep, dp - dq, order) / Sp - np.log(Sp) + np.log(Sq), weighted(eq, dq - dp, order) / Sq - np.log(Sq) + np.log(Sp))
