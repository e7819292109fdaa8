"""tests/fchain_ref.py against the oracle, on the CPU: the restatement of the float chain's linear stage that tests/test_gpu_fchain_kernels.py holds the kernels
to.  For every case (the five shapes x F32 / F16, and the subnormal-weight group):
  (a) the sums are exact in any order -- span_bits() bounds the window of every output's partial sums by a double's 53 bits, and on a sample of outputs the
      sequential sum, a permuted sum and math.fsum give the same double;
  (b) the reference equals oracle.vec_dot (bo_vec_dot: vec_dot_f32 / vec_dot_f16 behind the activation row's conversion), row by row, on the sampled rows of
      every column;
  (c) each of the four named mistakes (fchain_ref.MISTAKES) changes the expected output.
The LayerNorm rows are chain_cases.ln_rows(): none of them is chain_ref.ln_fragile, so the producer's own association of the double sums cannot show."""
import math

import numpy as np
import pytest

import chain_cases as C
import chain_ref as R
import fchain_ref as FR
from fchain_ref import F32, F64

CASES = [(t, K, M, N, "mirror") for (K, M, N) in FR.SHAPES for t in FR.TYPES] + [(FR.W_F16,) + FR.SUB_SHAPE + ("sub",)]
IDS = ["%s_K%d_M%d_N%d_%s" % ((FR.NAMES[c[0]],) + c[1:]) for c in CASES]


def sample_rows(M):
    """The special rows (zeros, +-0.0 pairs, the last row) and every 29th."""
    return np.unique(np.concatenate([np.arange(0, M, 29), np.array([r for r in (5, 7, 9, 21, M - 1) if r < M])]))


def row_bytes(wtype, w):
    return np.ascontiguousarray(w).view(np.uint8)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_sums_are_exact_in_any_order(case):
    wtype, K, M, N, kind = case
    W, X = FR.case(wtype, K, M, N, kind)
    span = FR.span_bits(wtype, W, X)
    print(IDS[CASES.index(case)], "widest window of partial sums: %d bits" % span)
    assert span <= 53
    g = np.random.default_rng(K + M)
    rows = sample_rows(M)[:12]
    xs = FR.activation(wtype, X)
    for c in range(N):
        p = FR.products(wtype, W[rows], xs[c])
        seq = np.add.accumulate(p, axis=1)[:, -1]
        perm = np.add.accumulate(p[:, g.permutation(K)], axis=1)[:, -1]
        fs = np.array([math.fsum(r) for r in p.tolist()], dtype=F64)
        assert (seq == perm).all() and (seq == fs).all(), (case, c)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_reference_equals_the_oracle_row_by_row(oracle, case):
    wtype, K, M, N, kind = case
    W, X = FR.case(wtype, K, M, N, kind)
    rows = sample_rows(M)
    got = FR.dots(wtype, W, X, rows=rows)
    for c in range(N):
        want = np.array([oracle.vec_dot(wtype, row_bytes(wtype, W[r]), X[c]) for r in rows], dtype=F32)
        assert (got[c].view(np.uint32) == want.view(np.uint32)).all(), (case, c)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_each_mistake_changes_the_expected_output(case):
    wtype, K, M, N, kind = case
    W, X = FR.case(wtype, K, M, N, kind)
    rows = sample_rows(M)
    clean = FR.dots(wtype, W, X, rows=rows)
    for mistake in ("f32_accumulator", "fused_product", "no_f16_rounding"):
        if mistake == "no_f16_rounding" and wtype != FR.W_F16:
            continue
        if wtype == FR.W_F16 and mistake == "fused_product":
            continue      # (an 11-bit weight times an 11-bit activation is exact in float32: the rounding of the product has nothing to do)
        bad = FR.dots(wtype, W, X, rows=rows, mistake=mistake)
        share = float((bad.view(np.uint32) != clean.view(np.uint32)).mean())
        print(IDS[CASES.index(case)], mistake, "changes %.1f %% of the sampled outputs" % (100 * share))
        assert share > 0, (case, mistake)
    bias, resid = FR.bias_of(rows.size, K), FR.resid_of(N, rows.size, K)
    good, bad = FR.epi_resid(clean, bias, resid), FR.epi_resid(clean, bias, resid, mistake="resid_grouping")
    share = float((bad.view(np.uint32) != good.view(np.uint32)).mean())
    print(IDS[CASES.index(case)], "resid_grouping changes %.1f %% of the sampled outputs" % (100 * share))
    assert share > 0, case
    assert set(FR.MISTAKES) == {"f32_accumulator", "fused_product", "no_f16_rounding", "resid_grouping"}


def test_epilogues_are_chain_refs():
    g = np.random.default_rng(3)
    acc = g.standard_normal((3, 3072), dtype=F32)
    bias = g.standard_normal(3072, dtype=F32)
    for a, b in zip(FR.epi_qkv(acc, bias, 1024), R.epi_qkv(acc, bias)):
        assert (a.view(np.uint32) == b.view(np.uint32)).all()
    resid = g.standard_normal((3, 3072), dtype=F32)
    assert (FR.epi_resid(acc, bias, resid) == R.epi_resid(acc, bias, resid)).all()
    assert (FR.epi_gelu(acc, bias) == R.gelu_table()[R._f16_index((bias[None, :] + acc).astype(F32))]).all()


def test_layer_norm_rows_are_the_oracles_and_not_fragile(oracle):
    x = C.ln_rows()
    w, b = C.ln_gain_bias()
    for i, row in enumerate(x):
        assert not R.ln_fragile(row), C.LN_FAMILIES[i]
    with np.errstate(all="ignore"):
        for wtype in FR.TYPES:
            y = FR.layer_norm(wtype, x, w, b)
            for i, row in enumerate(x):
                want = oracle.layer_norm(row, w, b)
                if wtype == FR.W_F16:
                    want = want.astype(np.float16).astype(F32)
                assert (y[i].view(np.uint32) == want.view(np.uint32)).all(), (FR.NAMES[wtype], C.LN_FAMILIES[i])
            assert (FR.layer_norm(wtype, x, w, b, mistake="ln_float_sums").view(np.uint32) != y.view(np.uint32)).any()
