"""tests/chain_ref.py is the oracle's arithmetic, and tests/chain_cases.py holds what it says -- shown here without a GPU, so that tests/test_gpu_chain_kernels.py may
hold the kernels to the restatement bit for bit.

  * the block sums equal bo_vec_dot_q: on every row of the small matrices; on the large ones on the hostile rows (the first and last rows of tiles, workgroups
    and the matrix), on the first and last row of every 16-row tile of a seeded sample of tiles, against the hostile columns and the columns on the tile tails;
  * LayerNorm equals bo_layer_norm, the Q8 blocks equal bo_quantize, the GELU table equals bo_gelu_table at every finite f16;
  * each family holds what its description claims, and every expected output is finite;
  * no LayerNorm row is fragile: its mean and variance come out the same float32 from the sequential double sums and from the exact sums rounded once, with no
    float32 border within the error bound of 1024 double additions -- so the kernels' own association of those sums owes the same bits;
  * each named kernel mistake (chain_ref.MISTAKES), committed in the restatement, changes an expected output of a committed case."""
import numpy as np
import pytest

import chain_cases as C
import chain_ref as R
from chain_ref import F32, Q81

IDS = [R.NAMES[t] for t in R.TYPES]
HOSTILE_COLS = [0, 1, 2, 3, 4, 5]


def _dots(oracle, wtype, W, K, aq, rows, cols):
    out = np.zeros((len(cols), len(rows)), dtype=F32)
    for i, c in enumerate(cols):
        yb = R.oracle_blocks(Q81[wtype], aq[0][c], aq[1][c], aq[2][c])
        for j, r in enumerate(rows):
            out[i, j] = oracle.vec_dot_q(wtype, K, W[r].tobytes(), yb)
    return out


def _sample_rows(M, seed, n_tiles=12):
    tiles = C._rng(10, seed, M).integers(0, M // 16, n_tiles)
    return sorted(set(C.hostile_rows(M)) | {int(t) * 16 for t in tiles} | {int(t) * 16 + 15 for t in tiles})


@pytest.mark.parametrize("wtype", R.TYPES, ids=IDS)
@pytest.mark.parametrize("op", ["QKV", "OPROJ", "FC1_Q8", "FC2", "LMHEAD"])
def test_block_sums_equal_the_oracles_vec_dot(oracle, op, wtype):
    M, K = C.shape_of(op, C.LM_SWEEP_M)
    n = max(C.column_counts(op, wtype))
    W, aq = C.weights(oracle, op, wtype, M, K), C.columns(op, Q81[wtype], K, n)
    acc = C.sums(oracle, op, wtype, M, n)
    assert np.isfinite(acc).all()
    rows = _sample_rows(M, wtype)
    cols = sorted(set(HOSTILE_COLS + [7, 47, 48, 63, 64, 80, n - 1]))
    ref = _dots(oracle, wtype, W, K, aq, rows, cols)
    got = acc[np.ix_(cols, rows)]
    assert (got.view(np.uint32) == ref.view(np.uint32)).all(), np.argwhere(got.view(np.uint32) != ref.view(np.uint32))[:6]


@pytest.mark.parametrize("wtype", R.TYPES, ids=IDS)
def test_small_lm_heads_equal_the_oracle_on_every_row(oracle, wtype):
    for M in C.LM_ROWS[:-1] + C.LM_ODD:
        W, aq = C.weights(oracle, "LMHEAD", wtype, M, 1024), C.columns("LMHEAD", Q81[wtype], 1024, 65)
        rows = range(M) if M <= 112 else _sample_rows(M, wtype) + [M - 1, M - 2, 1040, 1041]
        acc = C.sums(oracle, "LMHEAD", wtype, M, 65)
        ref = _dots(oracle, wtype, W, 1024, aq, list(rows), HOSTILE_COLS + [64])
        got = acc[np.ix_(HOSTILE_COLS + [64], list(rows))]
        assert np.isfinite(acc).all() and (got.view(np.uint32) == ref.view(np.uint32)).all(), M


def test_gelu_table_equals_the_oracles(oracle):
    tab = R.gelu_table()
    x = np.arange(65536, dtype=np.uint16).view(np.float16).astype(F32)
    fin = np.flatnonzero(np.isfinite(x))
    ref = np.array([oracle.gelu_table(float(x[i])) for i in fin], dtype=F32)
    assert (tab[fin].view(np.uint32) == ref.view(np.uint32)).all()
    big = x[fin][x[fin] >= 8]
    assert (tab[fin][x[fin] >= 8] == big).all(), "from 8 on the table returns its argument"


def _oracle_q8(oracle, row, q81):
    return oracle.quantize(oracle.TYPE_Q8_1 if q81 else oracle.TYPE_Q8_0, row, row.size).tobytes()


def test_layernorm_rows_equal_the_oracle_and_none_is_fragile(oracle):
    x = C.ln_rows()
    for fc1 in (False, True):
        w, b = C.ln_gain_bias(fc1)
        for i, row in enumerate(x):
            y, yo = R.layer_norm(row, w, b), oracle.layer_norm(row, w, b)
            assert np.isfinite(y).all() and (y.view(np.uint32) == yo.view(np.uint32)).all(), C.LN_FAMILIES[i]
            for q81 in (False, True):
                q, d, s = R.quantize_q8(y, q81)
                assert R.oracle_blocks(q81, q, d, s) == _oracle_q8(oracle, yo, q81), (C.LN_FAMILIES[i], q81)
    for i, row in enumerate(x):
        assert not R.ln_fragile(row), C.LN_FAMILIES[i]
    # the families
    w, b = C.ln_gain_bias()
    fam = {f: x[C.LN_FAMILIES.index(f)] for f in set(C.LN_FAMILIES)}
    assert np.ptp(fam["constant"]) == 0 and (R.layer_norm(fam["constant"], w, b) == b).all()
    assert 1e18 < np.abs(fam["huge"]).max() < 1e19 and np.abs(fam["outlier"]).max() > 500 and abs(float(fam["offset"].mean()) - 300) < 1
    q, d, s = R.lnq(x, w, b, True)
    assert (d[:, C.OUT_ZERO_BLOCK] == 0).all() and (q.reshape(-1, 32, 32)[:, C.OUT_ZERO_BLOCK] == 0).all()
    assert (q.reshape(-1, 32, 32)[:, C.OUT_CONST_BLOCK] == 127).all() and (s.view(F32)[:, C.OUT_CONST_BLOCK] == F32(4064) * d[:, C.OUT_CONST_BLOCK]).all()


@pytest.mark.parametrize("wtype", R.TYPES, ids=IDS)
def test_fc1_epilogue_equals_the_oracles_table_and_quantizer(oracle, wtype):
    q81 = Q81[wtype]
    args, want = C.build(oracle, "FC1_Q8", wtype, 17)
    g = want["gelu"]
    pre = (args["bias"][None, :] + C.sums(oracle, "FC1_Q8", wtype, 4096, 17)).astype(F32)
    assert np.isfinite(g).all() and np.abs(pre.astype(np.float16).astype(F32)).max() == 65504.0, "pre-activations reach the last finite f16 and stay finite"
    for c in (0, 1, 2, 3, 4, 16):
        for r in list(range(32 * 127, 32 * 128)) + C.hostile_rows(4096) + [32, 40, 2112, 3104]:
            assert g[c, r] == F32(oracle.gelu_table(float(pre[c, r]))), (c, r)
        blk = R.oracle_blocks(q81, want["out_q"][c], want["out_d"][c], want["out_s"][c])
        assert blk == _oracle_q8(oracle, g[c], q81), c
    # the zero-weight groups: bias alone, on roundf ties and on amax = 127 * 2^j
    for grp, j in C.TIE_GROUPS.items():
        v = g[0, 32 * grp:32 * grp + 32]
        assert (v == args["bias"][32 * grp:32 * grp + 32]).all() and v.max() == 127 * 2.0 ** j
        t = v.astype(np.float64) / 2.0 ** j
        ties = np.flatnonzero(t - np.floor(t) == 0.5)
        assert len(ties) >= 20, (grp, len(ties))
        assert want["out_d"][0, grp] == F32(2.0 ** j)
        assert (want["out_q"][0, 32 * grp + ties] == np.floor(t[ties]) + 1).all(), "half away from zero"
        assert (np.floor(t[ties]) % 2 == 0).any(), "a tie that nearest-even would round down"
    W = R.decode_weights(wtype, args["w_rows"], 4096, 1024)
    assert (W[1][:, 3::8] == 0).all() and all((W[0][32 * grp:32 * grp + 32] == (-8 if wtype == R.Q4_0 else -16 if wtype == R.Q5_0 else 0)).all() for grp in C.ZERO_GROUPS)


@pytest.mark.parametrize("wtype", R.TYPES, ids=IDS)
def test_families_hold_what_they_claim(oracle, wtype):
    M, K = 3072, 1024
    raw = C.weights(oracle, "QKV", wtype, M, K)
    codes, d, m = R.decode_weights(wtype, raw, M, K)
    hostile = C.hostile_rows(M)
    A, B = hostile[0::2], hostile[1::2]
    off = {R.Q4_0: 8, R.Q5_0: 16}.get(wtype, 0)
    lo, hi = (-128, 127) if wtype == R.Q8_0 else (0 - off, (31 if wtype in (R.Q5_0, R.Q5_1) else 15) - off)
    assert (codes[A][:, 0::2] == lo).all() and (codes[A][:, 1::2] == hi).all(), "all-minimum and all-maximum codes"
    if wtype in (R.Q5_0, R.Q5_1):
        at = 4 if wtype == R.Q5_1 else 2
        qh = raw[A][:, :, at:at + 4].copy().view("<u4")[..., 0]
        assert (qh[:, 0::2] == 0).all() and (qh[:, 1::2] == 0xFFFFFFFF).all(), "every qh bit"
    sub = np.float16(0).view(np.uint16) + 1
    for r, val in ((0, 0.0), (1, float(np.uint16(sub).view(np.float16))), (4, 65504.0), (5, -65504.0), (7, -float(np.uint16(sub).view(np.float16)))):
        assert (d[B][:, r::8] == F32(val)).all(), (r, val)
    assert (d[B][:, 2::8] < 0).all() and (d[B][:, 3::8] == 0).all() and (raw[B][:, 3::8] == 0).all(), "negative scales; zero blocks"
    if m is not None:
        assert (m[B][:, 0::8] != 0).all() and (d[B][:, 0::8] == 0).all(), "d = 0 with m != 0"
    q, dx, s = C.columns("QKV", Q81[wtype], K, 81)
    qb = q.reshape(81, 32, 32)
    assert (dx[1][[0, 1, 8, 9]] == 0).all() and (qb[1][[0, 1, 8, 9]] == 0).all() and (s[1][[0, 1]] == 0).all(), "all-zero blocks"
    assert (np.abs(qb[2]) == 127).all() and (qb[4][0::2] == 127).all() and (qb[4][1::2] == -127).all() and (qb[5] >= 64).all()
    big, tiny = (F32(1e30), F32(1e-30)) if Q81[wtype] else (F32(65504.0), F32(2.0 ** -24))
    assert (dx[3][3::8] == big).all() and (dx[3][4::8] == tiny).all()
    if Q81[wtype]:
        assert (s.view(F32)[4][0::2] == F32(4064) * dx[4][0::2]).all() and (s.view(F32)[4][1::2] == F32(-4064) * dx[4][1::2]).all(), "Q8_1 sums at their ends"
    else:
        assert (s.view(np.int32)[4][0::2] == 4064).all() and (s.view(np.int32)[4][1::2] == -4064).all()
    # bias and residual that cancel the sum; positions 0 and P - 1; packed columns of three slots in scrambled order
    args, want = C.build(oracle, "OPROJ", wtype, 9)
    out = want["out"][:9, :1024]
    assert np.isfinite(out).all() and (out[1] == 0).all() and ((C.sums(oracle, "OPROJ", wtype, 1024, 9)[0] + args["bias"])[3::37] == 0).all()
    ends = {}
    for N in C.column_counts("QKV", wtype):
        st = C.qkv_states(C.qkv_form(N), N, N + 1000 * R.TYPES.index(wtype))
        assert len(set(zip(st["slot"], st["pos"]))) == N and st["pos"].min() >= 0 and st["pos"].max() < st["P"], N
        ends.setdefault(C.qkv_form(N), set()).update({"first"} if st["pos"].min() == 0 else set(), {"last"} if st["pos"].max() == st["P"] - 1 else set())
    assert ends == {0: {"first", "last"}, 1: {"first", "last"}, 2: {"first", "last"}}, "positions 0 and P - 1 in every form of the column states"
    st = C.qkv_states(2, 65, 1)
    assert set(st["slot"]) == {0, 1, 2} and (np.diff(st["slot"]) != 0).any() and (st["seq_states"][:, 3] == st["slot"]).all()
    assert {C.qkv_form(N) for N in C.column_counts("QKV", wtype)} == {0, 1, 2}


@pytest.mark.parametrize("wtype", R.TYPES, ids=IDS)
def test_every_expected_output_is_finite(oracle, wtype):
    for op in ("QKV", "OPROJ", "FC1_Q8", "FC2", "LMHEAD"):
        N = max(C.column_counts(op, wtype))
        args, want = C.build(oracle, op, wtype, N, M=C.LM_SWEEP_M if op == "LMHEAD" else None)
        M = args["M"]
        if "out" in want:
            assert np.isfinite(want["out"][:N, :(1024 if op == "QKV" else M)]).all(), op
        if op == "QKV":
            st = C.qkv_states(C.qkv_form(N), N, N + 1000 * R.TYPES.index(wtype))
            assert np.isfinite(want["k"][st["slot"], :, st["pos"]]).all() and np.isfinite(want["v"][st["slot"], :, st["pos"]]).all()
        if "out_d" in want:
            assert np.isfinite(want["out_d"][:N]).all() and np.isfinite(want["gelu"]).all()
    for row in C.FC1_LN_ROWS:
        _, want = C.build_fc1_ln(oracle, wtype, row)
        assert np.isfinite(want["gelu"]).all() and np.isfinite(want["out_d"][:1]).all()


def test_one_column_fc1_equals_the_oracle(oracle):
    for wtype in (R.Q4_0, R.Q5_1):
        args, want = C.build_fc1_ln(oracle, wtype, 2)
        y = oracle.layer_norm(args["x"][0], args["ln_w"], args["ln_b"])
        assert R.oracle_blocks(Q81[wtype], *(a[0] for a in want["aq"])) == _oracle_q8(oracle, y, Q81[wtype])
        rows = _sample_rows(4096, wtype)
        acc = R.block_sums(wtype, args["w_rows"], 4096, 1024, *want["aq"], rows=rows)
        assert (acc.view(np.uint32) == _dots(oracle, wtype, args["w_rows"], 1024, want["aq"], rows, [0]).view(np.uint32)).all()


# ---- the mistakes ------------------------------------------------------------------------------------------------------------------------------------

def _differs(a, b):
    return any((a[k].view(np.uint8) != b[k].view(np.uint8)).any() for k in ("out", "out_q", "out_d", "out_s", "k", "v") if k in a)


def _caught(oracle, op, wtype, N, mistake):
    M = C.LM_SWEEP_M if op == "LMHEAD" else None
    _, want = C.build(oracle, op, wtype, N, M=M)
    _, wrong = C.build(oracle, op, wtype, N, M=M, mistake=mistake)
    if not _differs(want, wrong):
        return False
    with pytest.raises(AssertionError):
        C.compare(wrong, want, mistake)
    return True


SEEN_BY = {      # mistake -> the (op, type) cases that must see it
    "dropped_last_block": [(op, t) for op in ("QKV", "OPROJ", "FC1_Q8", "FC2", "LMHEAD") for t in R.TYPES],
    "previous_tile_scale": [(op, t) for op in ("QKV", "OPROJ", "FC1_Q8", "FC2", "LMHEAD") for t in R.TYPES],
    "pairwise_sum": [(op, t) for op in ("QKV", "OPROJ", "FC2", "LMHEAD") for t in R.TYPES],
    "dx_before_dw": [(op, R.Q4_0) for op in ("QKV", "OPROJ", "FC2", "LMHEAD")],
    "product_first": [(op, R.Q8_0) for op in ("QKV", "OPROJ", "FC2", "LMHEAD")],
    "fused_min_term": [(op, t) for op in ("QKV", "OPROJ", "FC2", "LMHEAD") for t in (R.Q4_1, R.Q5_1)],
    "clamped_column_stored": [(op, t) for op in ("QKV", "OPROJ", "FC1_Q8", "FC2", "LMHEAD") for t in (R.Q4_0, R.Q5_1)],
    "bias_after_scale": [("QKV", t) for t in R.TYPES],
    "resid_first": [(op, t) for op in ("OPROJ", "FC2") for t in R.TYPES],
    "nearest_even": [("FC1_Q8", t) for t in R.TYPES],
    "sum_before_f16": [("FC1_Q8", t) for t in R.TYPES],
    "gelu_without_f16": [("FC1_Q8", t) for t in R.TYPES],
}


@pytest.mark.parametrize("mistake", sorted(SEEN_BY))
def test_each_mistake_changes_an_expected_output(oracle, mistake):
    for op, wtype in SEEN_BY[mistake]:
        assert _caught(oracle, op, wtype, 49, mistake), (mistake, op, R.NAMES[wtype])


def test_layernorm_mistakes_change_the_blocks():
    """ln_scale_first moves single float32 rows by an ulp: the Q8_1 blocks show it in their f32 scale, the Q8_0 blocks (f16 scale) only where a code moves -- on
    these rows they do not, so for that form it is a mistake these outputs cannot show."""
    for mistake, forms in (("ln_float_sums", (False, True)), ("ln_scale_first", (True,)), ("nearest_even", (False, True)), ("sum_before_f16", (False, True))):
        for q81 in forms:
            _, want = C.build_lnq(q81)
            _, wrong = C.build_lnq(q81, mistake=mistake)
            assert _differs(want, wrong), (mistake, q81)
    assert set(SEEN_BY) | {"ln_float_sums", "ln_scale_first"} == set(R.MISTAKES)


def test_mistakes_these_outputs_cannot_show(oracle):
    """The claims of HISTORY.md's list, on the committed cases.  Q4_0's order of the two scales: on the ordinary rows against the ordinary columns every output keeps
    its bits (the integer dots are short enough for dot * d_w and dot * d_x to be exact, so both orders round once, alike); it shows against column 5.  LayerNorm's
    gain * scale first: invisible through the Q8_0 blocks of these rows."""
    for op in ("LMHEAD", "OPROJ", "QKV"):
        M, K = C.shape_of(op, C.LM_SWEEP_M)
        W, aq = C.weights(oracle, op, R.Q4_0, M, K), C.columns(op, False, K, 49)
        right = C.sums(oracle, op, R.Q4_0, M, 49)
        wrong = R.block_sums(R.Q4_0, W, M, K, *aq, mistake="dx_before_dw")
        rows = np.setdiff1d(np.arange(M), C.hostile_rows(M))
        cols = np.setdiff1d(np.arange(49), [2, 4, 5])
        assert (right[np.ix_(cols, rows)].view(np.uint32) == wrong[np.ix_(cols, rows)].view(np.uint32)).all(), op
        assert (right[5].view(np.uint32) != wrong[5].view(np.uint32)).any(), op
    _, want = C.build_lnq(False)
    _, wrong = C.build_lnq(False, mistake="ln_scale_first")
    assert not _differs(want, wrong)
