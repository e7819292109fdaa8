"""score_stats_rows_kernel and score_compare_rows_kernel (kernels_score_stats.hip.h) alone, through biogpt_hip_score_stats_device, against the float64
restatement of score_stats_ref.py: widths with only a tail, one quad per thread plus a tail, and the two real vocabularies; rows on every 16-byte
alignment; random, tied, constant, nearly empty and NaN rows.  Ids and ranks are exact, the plain outputs are logprob_rows_kernel's bits, entropy and
KL are held to 2^-23 |ref| + 1e-9 (score_stats_ref.tolerance), which the restatement itself keeps when it sums in the opposite order."""
import numpy as np
import pytest

import score_stats_ref as R
from beam_kernels_ref import lp_tolerance

pytestmark = pytest.mark.gpu

K = 5
WIDTHS = [3, 4 * 256 + 3, 42384, 57717]
KINDS = ["random", "tied", "constant", "sparse", "nan", "untargeted"]


def bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


def held(got, ref):
    """got (f32) against ref (f64): the tolerance where ref is finite, the same infinity or NaN where it is not."""
    got, ref = np.atleast_1d(np.asarray(got, dtype=np.float64)), np.atleast_1d(np.asarray(ref, dtype=np.float64))
    fin = np.isfinite(ref)
    return (np.abs(got[fin] - ref[fin]) <= R.tolerance(ref[fin])).all() and np.array_equal(got[~fin], ref[~fin], equal_nan=True)


def make_rows(V, seed):
    """One row of each kind and its target."""
    rng = np.random.default_rng(seed)
    rows = (rng.standard_normal((len(KINDS), V)) * 3.0).astype(np.float32)
    tg = rng.integers(0, V, len(KINDS)).astype(np.int32)
    ties = sorted(rng.choice(V, 3, replace=False))
    rows[1, ties] = rows[1].max() + 1.0
    tg[1] = ties[1]      # one tied entry comes before it
    rows[2] = 0.75
    keep = rng.choice(V, K - 2, replace=False)
    rows[3, np.setdiff1d(np.arange(V), keep)] = -np.inf
    tg[3] = keep[0]
    rows[4, tg[4]] = np.nan
    tg[5] = -1
    return rows, tg


@pytest.mark.parametrize("start", [0, 1, 2, 3])
@pytest.mark.parametrize("V", WIDTHS)
def test_stats_kernel_against_float64(pkg, V, start):
    rows, tg = make_rows(V, 100 + V)
    n, rev = len(rows), np.arange(V)[::-1]
    got = pkg.score_stats_device(rows, tg, n_top=K, start=start)
    lp, am, lg = pkg.logprob_rows(rows, tg)
    assert np.array_equal(bits(got["lp"][:n]), bits(lp)) and np.array_equal(bits(got["logit"][:n]), bits(lg)) and np.array_equal(got["argmax"][:n], am)
    for name in got:      # the guard entry behind every output
        assert (np.ascontiguousarray(got[name][n:]).view(np.uint8) == 0xff).all(), name
    for r, kind in enumerate(KINDS):
        ref = R.row_stats(rows[r], int(tg[r]), K)
        print("%s V=%d start=%d: rank %d (ref %d), entropy %.9g (ref %.12g)" % (kind, V, start, got["rank"][r], ref["rank"], got["entropy"][r], ref["entropy"]))
        assert held(np.float32(R.row_stats(rows[r], int(tg[r]), K, order=rev)["entropy"]), ref["entropy"]), kind
        assert np.array_equal(got["top_ids"][r], ref["top_ids"]) and got["rank"][r] == ref["rank"] and held(got["entropy"][r], ref["entropy"]), kind
        fin = np.isfinite(ref["top_lp"])      # (the NaN row: every lp NaN, as its S; the sparse row: entries at -inf)
        assert (np.abs(got["top_lp"][r][fin] - ref["top_lp"][fin]) <= lp_tolerance(V, ref["top_lp"][fin])).all(), kind
        assert np.array_equal(got["top_lp"][r][~fin], ref["top_lp"][~fin], equal_nan=True), kind
        for j in np.flatnonzero(got["top_ids"][r] == tg[r]):
            assert bits(got["top_lp"][r, j]) == bits(got["lp"][r]), kind
    assert got["rank"][1] == 1 and got["rank"][4] == -1 and got["rank"][5] == -1 and np.isnan(got["entropy"][4])
    if V == 3:      # entries the row does not have
        assert (got["top_ids"][:4, 3:] == -1).all() and (got["top_lp"][:4, 3:] == 0.0).all()


@pytest.mark.parametrize("start", [0, 1, 2, 3])
@pytest.mark.parametrize("V", WIDTHS)
def test_compare_kernel_against_float64(pkg, V, start):
    p, tg = make_rows(V, 200 + V)
    n, rev = len(p), np.arange(V)[::-1]
    q = (np.random.default_rng(300 + V).standard_normal(p.shape) * 3.0).astype(np.float32)
    q[1], q[2] = p[1], p[2] + np.float32(1.5)      # the same bits; a constant apart
    q[0, V - 1] = -np.inf                          # -inf where p is finite
    tg[5] = tg[0]
    got = pkg.score_stats_device(p, tg, rows_q=q, start=start)
    for rows, lp_name, am_name in ((p, "lp", "argmax"), (q, "lp_other", "argmax_other")):
        lp, am, _ = pkg.logprob_rows(rows, tg)
        assert np.array_equal(bits(got[lp_name][:n]), bits(lp)) and np.array_equal(got[am_name][:n], am), lp_name
    for name in got:
        assert (np.ascontiguousarray(got[name][n:]).view(np.uint8) == 0xff).all(), name
    for r, kind in enumerate(KINDS):
        ref = R.row_kl(p[r], q[r])
        print("%s V=%d start=%d: kl %.9g (ref %.12g), kl_rev %.9g (ref %.12g)" % (kind, V, start, got["kl"][r], ref[0], got["kl_rev"][r], ref[1]))
        assert held(np.float32(R.row_kl(p[r], q[r], order=rev)), ref) and held([got["kl"][r], got["kl_rev"][r]], ref), kind
    assert got["kl"][1] == 0.0 and got["kl_rev"][1] == 0.0 and abs(got["kl"][2]) <= 1e-9 and abs(got["kl_rev"][2]) <= 1e-9
    assert got["kl"][0] == np.inf and np.isfinite(got["kl_rev"][0]) and np.isnan(got["kl"][4]) and np.isnan(got["kl_rev"][4])
