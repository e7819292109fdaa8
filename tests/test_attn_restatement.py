"""The cases of tests/test_gpu_attn_kernels.py on the CPU (tests/attn_cases.py): what the oracle (bo_attn_head) and the numpy restatement (tests/attn_ref.py)
say about them, so that the GPU test's claim -- bit equality with the oracle on every row -- is owed on every row it makes it for.

The bound of test_restatement_is_within_two_fp16_roundings_of_plain_attention, derived and not measured.  Given the float32 scores, plain attention is
p_j = e_j / sum e with e_j = exp(x_j), x_j = s_j - max <= 0, in float64.  The oracle's e'_j differs from e_j by two fp16 roundings:
  * the argument x_j is rounded to fp16 (11 significant bits): |x'_j - x_j| <= |x_j| 2^-11.  Only |x_j| <= 17.4 matters (beyond, e_j < 2^-25 and e'_j = 0, an
    absolute error below eta = 2^-25), so exp(x'_j) = e_j (1 + a) with |a| <= exp(17.4 * 2^-11) - 1;
  * the table value is rounded to fp16: relative 2^-11 where the result is a normal fp16, absolute at most eta = 2^-25 (half the subnormal spacing 2^-24) where
    it is subnormal or zero.
So |e'_j - e_j| <= delta e_j + eta with delta = exp(17.4 * 2^-11) (1 + 2^-11) - 1 = 0.00902.  The key at the maximum has x = 0 and e' = e = 1 exactly, so both
sums are at least 1, and for non-negative weights |p' - p|_1 <= 2 |e' - e|_1 / sum e' <= 2 (delta / (1 - delta) + T eta).  The float32 roundings of the
restatement (x, inv, p, the products, the output: each 2^-24 relative, x at most 2^-20 absolute) add less than 2^-18.  An output is a p-weighted sum of V:
    |out' - out| <= max|V| * (2 delta / (1 - delta) + T 2^-24 + 2^-18)."""
import math

import numpy as np
import pytest

import attn_cases as A
import attn_ref


@pytest.fixture(scope="module")
def cases(oracle):
    return A.all_cases()


def test_restatement_equals_the_oracle_and_no_row_is_fragile(cases):
    fragile, near, bad, rows = [], [], [], 0
    for c in cases:
        ref, orc = A.ref_rows(c), A.oracle_rows(c)
        for i in range(c.N):
            for h in range(A.H):
                r, o = ref[i][h], orc[i, h * c.dk:(h + 1) * c.dk]
                rows += 1
                if r["fragile"].any():
                    fragile.append((c.name, i, h))
                if r["inv_near_tie"]:         # the documented difference of inv_sum_f32 from (float)(1.0 / sum) could show here: no committed case goes near it
                    near.append((c.name, i, h, r["sum"]))
                ne = (r["out"].view(np.uint32) != o.view(np.uint32)) & ~r["fragile"]
                if ne.any():
                    d = int(np.argmax(ne))
                    bad.append((c.name, i, h, d, float(r["out"][d]), float(o[d]), int(c.T[i])))
    assert not bad, (len(bad), bad[:6])
    assert not fragile, ("a seed gives a fragile row: choose another seed", fragile[:6])
    assert not near, near[:6]
    assert rows > 10000


def rows_by_the_kernels_addressing(c, k, v, dev, st, i, h):
    """Column i's visible rows of head h read from the slot arrays as the kernels address them (not through Case.gather)."""
    if dev is not None:
        T = A.visible_keys((int(dev[0]), int(dev[2]), int(dev[3])), i, c.N)
        return k[0, h, :T], v[0, h, :T]
    T = int(st[i, 4]) if c.col_mode else int(st[i, 0]) + 1
    slot = int(st[i, 3]) if c.col_mode else i
    ns, sh = (int(st[i, 5]), int(st[i, 6])) if 4 <= c.route <= 8 else (0, 0)      # the SHARED instantiations and attn_prefix_kernel
    return np.concatenate([k[sh, h, :ns], k[slot, h, ns:T]]), np.concatenate([v[sh, h, :ns], v[slot, h, ns:T]])


def test_the_sentinel_never_reaches_the_oracles_output(cases):
    for c in cases:
        k, v = c.slots()
        dev, st = c.states()
        orc = A.oracle_rows(c)
        assert np.isfinite(orc).all(), c.name
        seen = np.zeros(k.shape[:3], dtype=bool)
        for i in range(c.N):
            for h in range(A.H):
                K, V = rows_by_the_kernels_addressing(c, k, v, dev, st, i, h)
                Kl, Vl = c.gather(i, h)
                assert K.shape == Kl.shape and (K == Kl).all() and (V == Vl).all(), (c.name, i, h, "the layout does not hold the case's rows")
                assert (K != A.SENTINEL).any(axis=1).all() and (np.abs(V) < 1e29).all(), (c.name, i, h)
                assert np.abs(orc[i, h * c.dk:(h + 1) * c.dk]).max() <= np.abs(V).max(), (c.name, i, h, "an output outside the hull of its V rows")
                if dev is not None:
                    seen[0, h, :K.shape[0]] = True
                else:
                    ns = int(st[i, 5]) if 4 <= c.route <= 8 else 0
                    seen[int(st[i, 3]) if c.col_mode else i, h, ns:K.shape[0]] = True
                    seen[int(st[i, 6]), h, :ns] = True
        assert (k[~seen] == A.SENTINEL).all() and (v[~seen] == A.SENTINEL).all(), (c.name, "a row no column sees holds something else than the sentinel")
        assert (~seen).any() or c.P == c.t_max, c.name


def test_every_family_has_what_it_claims(cases, oracle):
    """Counted on column 0 (the column the keys were built for) of every head, from the restatement's s - max, table values and sums."""
    seen = set()
    for c in cases:
        if c.family is None or c.family == "q8" or (c.family, c.t_max, c.dk) in seen:
            continue
        seen.add((c.family, c.t_max, c.dk))
        T = int(c.T[0])
        for h in range(A.H):
            r = A.ref_rows(c)[0][h]
            x, e, what = r["x"].astype(np.float64), r["e"], (c.name, h)
            with np.errstate(over="ignore"):
                arg16 = r["x"].astype(np.float16)
            top = np.flatnonzero(x == 0.0)
            if c.family in ("equal", "v_alt"):
                assert (e == 1.0).all() and r["sum"] == float(T), what
                assert T != 1024 or r["inv"] == np.float32(2.0 ** -10), what
            if c.family == "tie2":
                assert len(top) == 2 and top[0] // 16 != top[1] // 16, (what, top)      # 16 keys per wave of attn_fast_kernel
            if c.family == "tie64":
                assert len(top) == 64 and len(set(top // 64)) == (T + 63) // 64, (what, len(top))
            if c.family.startswith("peak"):
                at = {"peak_last": T - 1, "peak_first": 0, "peak_shared": T // 4}[c.family]
                assert list(top) == [at] and np.delete(x, at).max() <= -28.0, (what, top)
                assert c.family != "peak_shared" or at < T // 2, what       # inside the shared range of the layouts with one
            if c.family == "ranges":
                sub = (x >= A.SUBNORMAL_X[0]) & (x <= A.SUBNORMAL_X[1])
                zero = (x < A.ZERO_X) & np.isfinite(arg16)
                inf = x < A.INF_X
                assert sub.sum() >= 1 and ((e[sub] > 0) & (e[sub] < 2.0 ** -14)).all(), (what, "the table's subnormal results")
                assert zero.sum() >= 1 and (e[zero] == 0).all(), (what, "below -17.4: zero")
                assert inf.sum() >= 1 and np.isneginf(arg16[inf]).all() and (e[inf] == 0).all(), (what, "below -65504: the fp16 argument is -inf")
                assert ((x > A.SUBNORMAL_X[1]) & (x < 0)).sum() >= 1, what
            if c.family == "small_quarter":
                small = float(e[x < 0].astype(np.float64).sum()) / r["sum"]
                assert len(top) == 1 and (x[x < 0] < -7.9).all() and (x[x < 0] > -8.1).all(), what
                assert T != 1024 or 0.24 < small < 0.27, (what, small)
            if c.family == "wide":
                assert x.min() < -20.0 and (e == 0).any() and (e > 0).sum() > 1, what
            V = c.gather(0, h)[1]
            if c.family == "v_alt":
                assert (np.abs(V) > 9.9e3).all() and (np.sign(V[::2]) > 0).all() and (np.sign(V[1::2]) < 0).all(), what
                assert np.abs(r["out"]).max() <= 1e4 / T + 1.0, (what, "the rows cancel")
            if c.family == "v_mixed":
                big = np.abs(V).max(axis=1) > 10.0
                assert big.any() and (~big).any() and (np.abs(V[~big]) < 1e-2).all(), what
            if c.family == "v_zero":
                assert (r["out"].view(np.uint32) == 0).all(), what
    assert {f for f, _, _ in seen} == set(A.FAMILIES[1:]) and {t for _, t, _ in seen} == {65, 257, 1024}


def test_the_q8_row_has_what_it_claims(oracle):
    """T = 1: the oracle's output IS the chosen V row; its blocks through the oracle's quantizer."""
    q, K, V = A.q8_content()
    row = np.concatenate([oracle.attn_head(q[0, h * 64:(h + 1) * 64], K[h], V[h], 1) for h in range(A.H)])
    assert (row.view(np.uint32) == V.reshape(-1).view(np.uint32)).all()
    b0 = np.frombuffer(oracle.quantize(oracle.TYPE_Q8_0, row, row.size).tobytes(), dtype=np.dtype([("d", "<u2"), ("q", "i1", 32)]))
    assert oracle.fp16_to_fp32(b0["d"][0]) == 1.0 and list(b0["q"][0][:10]) == [127, 1, -1, 2, -2, 3, -3, 127, -127, 4]      # roundf: halves away from zero
    assert (np.abs(row[10:32] * 2) % 2 == 1).all()                                                                               # every element of the block is a half
    assert b0["d"][1] == 0 and (b0["q"][1] == 0).all()
    assert b0["q"][2][6] == 127 and np.delete(b0["q"][2], 6).max() == 0 and b0["q"][3][4] == -127
    b1 = np.frombuffer(oracle.quantize(oracle.TYPE_Q8_1, row, row.size).tobytes(), dtype=np.dtype([("d", "<f4"), ("s", "<f4"), ("q", "i1", 32)]))
    assert (b1["q"] == b0["q"]).all() and b1["d"][1] == 0 and b1["s"][1] == 0 and b1["s"][0] == np.float32(b1["q"][0].astype(np.int32).sum())


def test_restatement_is_within_two_fp16_roundings_of_plain_attention(cases):
    delta = math.exp(17.4 * 2.0 ** -11) * (1 + 2.0 ** -11) - 1
    worst = 0.0
    for c in cases:
        ref = A.ref_rows(c)
        for i in range(c.N):
            for h in range(A.H):
                V = c.gather(i, h)[1]
                T = int(c.T[i])
                plain = attn_ref.plain_head(ref[i][h]["scores"], V, T)
                bound = float(np.abs(V).max()) * (2 * delta / (1 - delta) + T * 2.0 ** -24 + 2.0 ** -18)
                err = float(np.abs(ref[i][h]["out"].astype(np.float64) - plain).max())
                assert err <= bound, (c.name, i, h, err, bound)
                worst = max(worst, err / bound if bound > 0 else 0.0)
    print("largest error / bound: %.3g" % worst)
