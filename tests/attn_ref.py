"""A numpy restatement of the attention of one (head, query) as the oracle computes it (oracle/biogpt_oracle.c, bo_attn_head).  It is NOT the reference of any
test: the reference is bo_attn_head.  It exists because a test that asks a kernel for bit equality with the oracle has to know where bit equality is owed.  The
kernels and the oracle perform the same roundings on the same quantities --

    score_j = fl32( sum_d double(fl32(k_jd * q_d)) )              a double sum of 64 products rounded to f32
    e_j     = table[ fp16(fl32(score_j - max)) ]                   the fp16 exponent table (built from bo_exp_table over all 65,536 patterns, never np.exp)
    inv     = fl32( 1.0 / sum_j double(e_j) )
    p_j     = fl32( e_j * inv )
    out_d   = fl32( sum_j double(fl32(v_jd * p_j)) )

-- and differ only in the ORDER in which they add the terms of the three double sums.  So every double sum is computed here exactly (math.fsum) and classified:

  * order-independent: every non-zero term is a multiple of 2^g and sum |term| < 2^(g + 53).  Then every partial sum of every association is a multiple of 2^g
    below 2^(g + 53), hence a double: no association rounds at all, and all of them give the exact sum.  (Sums of f32 products often are: that is why a score may
    sit exactly on a float32 tie without being in doubt.)
  * otherwise an association's result lies within  margin = n * 2^-53 * sum |term|  (n terms) of the exact sum, and the sum is FRAGILE if a float32 rounding
    boundary lies within that margin of it: two associations may then round to different floats.  For the probability sum the quantity rounded is 1 / sum.

A row -- the 64 outputs of one (head, query) -- is fragile in output d if one of its scores, its inv, or the sum of output d is fragile.
The module also holds a plain float64 softmax attention (plain_head) for the sanity bound of tests/test_attn_restatement.py."""
import math

import numpy as np

_TABLE = None


def exp_table():
    """float32 [65536]: the oracle's fp16-table exponent by fp16 bit pattern of the argument."""
    global _TABLE
    if _TABLE is None:
        from oracle import oracle as O
        L = O.lib()
        _TABLE = np.array([L.bo_exp_table(L.bo_fp16_to_fp32(h)) for h in range(1 << 16)], dtype=np.float32)
    return _TABLE


def sum_info(terms):
    """terms float64 [n_sums][n_terms].  Returns (exact float64 [n_sums]: the correctly rounded exact sums; oi bool: order-independent; margin float64: 0 where oi)."""
    terms = np.ascontiguousarray(terms, dtype=np.float64)
    assert np.isfinite(terms).all()
    n = terms.shape[1]
    exact = np.array([math.fsum(r) for r in terms.tolist()], dtype=np.float64)
    absum = np.abs(terms).sum(axis=1)                        # within n * 2^-53 (relative) of the true value: far inside the slack taken below
    m, e = np.frexp(terms)                                   # term = m * 2^e, 0.5 <= |m| < 1
    M = np.abs(np.ldexp(m, 53)).astype(np.int64)             # the 53-bit significand as an integer
    low = (M & -M).astype(np.float64)                        # its lowest set bit
    _, le = np.frexp(np.where(low > 0, low, 1.0))            # low = 2^(le - 1)
    g_each = np.where(terms != 0.0, e.astype(np.int64) - 53 + (le.astype(np.int64) - 1), np.int64(1 << 20))
    g = g_each.min(axis=1)
    all_zero = g == (1 << 20)
    g = np.where(all_zero, 0, g)
    oi = all_zero | (absum * (1.0 + 1e-9) < np.ldexp(1.0, (g + 53).astype(np.int32)))
    margin = np.where(oi, 0.0, n * 2.0 ** -53 * absum)
    return exact, oi, margin


def f32_boundary_distance(x):
    """Distance (float64) of each x to the nearer float32 rounding boundary around it (the midpoints between fl32(x) and its two neighbours)."""
    x = np.asarray(x, dtype=np.float64)
    f = x.astype(np.float32)
    up = np.nextafter(f, np.float32(np.inf)).astype(np.float64)
    dn = np.nextafter(f, np.float32(-np.inf)).astype(np.float64)
    f64 = f.astype(np.float64)
    return np.minimum(np.abs(x - (f64 + up) / 2), np.abs(x - (f64 + dn) / 2))


def head(q, K, V, T):
    """q float32 [dk]; K, V float32 [>= T][dk]; T visible keys.  Returns a dict: out float32 [dk] and the intermediate values per key (scores, x = score - max, e,
    p) and inv, so that the first wrong key of a kernel can be found from one run; and the classification: score_oi / score_fragile [T], inv_fragile,
    inv_near_tie (1 / sum within two ulps of double of a float32 boundary: where a reciprocal that is not the IEEE quotient may round elsewhere), out_oi /
    out_fragile [dk], fragile [dk] (the row's verdict per output)."""
    q = np.asarray(q, dtype=np.float32)
    K = np.asarray(K[:T], dtype=np.float32)
    V = np.asarray(V[:T], dtype=np.float32)
    tab = exp_table()
    s_exact, s_oi, s_margin = sum_info((K * q[None, :]).astype(np.float64))      # float32 * float32 in numpy: the product rounded to f32
    scores = s_exact.astype(np.float32)
    score_fragile = ~s_oi & (f32_boundary_distance(s_exact) <= s_margin)
    mx = scores.max()
    x = scores - mx                                                              # float32 subtraction
    with np.errstate(over="ignore"):
        e = tab[x.astype(np.float16).view(np.uint16)]
    sum_exact, sum_oi, sum_margin = sum_info(e.astype(np.float64)[None, :])
    ssum = float(sum_exact[0])
    inv64 = 1.0 / ssum
    inv = np.float32(inv64)
    inv_margin = 0.0 if sum_oi[0] else float(sum_margin[0]) / (ssum * ssum)      # d(1 / s) = ds / s^2
    d_inv = float(f32_boundary_distance(np.array([inv64]))[0])
    inv_fragile = (not sum_oi[0]) and d_inv <= inv_margin
    inv_near_tie = d_inv <= 2.0 * np.spacing(inv64)
    p = e * inv                                                                  # float32
    o_exact, o_oi, o_margin = sum_info((V * p[:, None]).astype(np.float64).T)
    out = o_exact.astype(np.float32)
    out_fragile = ~o_oi & (f32_boundary_distance(o_exact) <= o_margin)
    return {"out": out, "scores": scores, "x": x, "e": e, "sum": ssum, "inv": inv, "p": p, "score_oi": s_oi, "score_fragile": score_fragile, "inv_fragile": bool(inv_fragile),
            "inv_near_tie": bool(inv_near_tie), "out_oi": o_oi, "out_fragile": out_fragile, "fragile": out_fragile | bool(inv_fragile) | bool(score_fragile.any())}


def plain_head(scores, V, T):
    """Softmax attention in float64 over given scores: exp, one division, one matrix product.  No table, no float32 rounding."""
    s = np.asarray(scores[:T], dtype=np.float64)
    w = np.exp(s - s.max())
    return (w / w.sum()) @ np.asarray(V[:T], dtype=np.float64)
