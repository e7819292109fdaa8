"""Every linear stage of the many-column chain, alone, against the oracle's arithmetic: lnq_kernel; the 8-column and 1-column matvec_fast_kernel forms behind
launch_chain; the 25 matmul_mfma_kernel instantiations (with retile_kernel in front of them).  biogpt_hip_chain_device launches them through the launch helpers
of the engine's own passes and reports the kernel family and geometry it launched.  The cases are those of tests/chain_cases.py, their expected outputs the
restatement tests/chain_ref.py, which tests/test_chain_restatement.py holds to the oracle on the CPU.

Per case: the f32 rows, the Q8 codes, scales and sums, and the K / V rows equal the restatement bit for bit ("many columns": no tolerance enters); every
guard byte -- the columns from N on, the rows from M on, every cache row no column writes -- still holds 0xff; the launch is the kernel family and geometry the
route names; and wherever both the 8-column and the matrix-core kernel are legal for a case, their outputs are equal (the promise of score_continuations in
enqueue_final rests on this)."""
import numpy as np
import pytest

import chain_cases as C
import chain_ref as R

pytestmark = pytest.mark.gpu

KEYS = ("out", "out_q", "out_d", "out_s", "k", "v")


def run(pkg, oracle, args, want, route, what):
    got = pkg.chain_device(route=route, **args)
    if args["op"] != "LNQ":
        M, N = args["M"], args["N"]
        K = C.shape_of(args["op"], M)[1]
        exp = C.expected_launch(args["op"], route, args["wtype"], M, K, N) + C.geometry(M, N)
        assert tuple(got["launched"][:7]) == exp, (what, route, "launched", list(got["launched"]), "expected", exp)
    C.compare(got, want, (what, route))
    return got


def sweep(pkg, oracle, op, wtype, counts, M=None, n_pool=None):
    for N in counts:
        args, want = C.build(oracle, op, wtype, N, M=M, n_pool=n_pool)
        form = C.qkv_form(N) if op == "QKV" else None
        what = "%s %s M %d N %d%s" % (op, R.NAMES[wtype], args["M"], N, "" if form is None else " states %d" % form)
        outs = [run(pkg, oracle, args, want, route, what) for route in C.legal_routes(op, wtype, args["M"], N, form)]
        if len(outs) == 2:      # (implied by the two comparisons above; stated for itself)
            for key in KEYS:
                if key in outs[0]:
                    assert (outs[0][key].view(np.uint8) == outs[1][key].view(np.uint8)).all(), (what, key, "the 8-column and the matrix-core kernel differ")


@pytest.mark.parametrize("wtype", R.TYPES, ids=[R.NAMES[t] for t in R.TYPES])
@pytest.mark.parametrize("op", ["QKV", "OPROJ", "FC1_Q8", "FC2"])
def test_site_equals_the_restatement(pkg, oracle, op, wtype):
    counts = C.column_counts(op, wtype)
    sweep(pkg, oracle, op, wtype, counts, n_pool=max(counts))


@pytest.mark.parametrize("wtype", R.TYPES, ids=[R.NAMES[t] for t in R.TYPES])
def test_lm_head_equals_the_restatement(pkg, oracle, wtype):
    """The column sweep at 1040 rows; 64 .. 112 rows (the last workgroup with 1 to 4 live waves); 1045 and 1043 rows, which have no whole tiles and stay on
    the 8-column kernel."""
    counts = C.column_counts("LMHEAD", wtype)
    sweep(pkg, oracle, "LMHEAD", wtype, counts, M=C.LM_SWEEP_M, n_pool=max(counts))
    for M in C.LM_ROWS[:-1] + C.LM_ODD:
        sweep(pkg, oracle, "LMHEAD", wtype, (64, 65), M=M, n_pool=65)


@pytest.mark.parametrize("wtype", R.TYPES, ids=[R.NAMES[t] for t in R.TYPES])
def test_lm_head_at_the_full_vocabulary(pkg, oracle, wtype):
    """42384 rows at 65 columns: the matrix-core kernel against the 8-column kernel whole, and both against the restatement on sampled rows."""
    M, K, N = C.LM_FULL, 1024, 65
    W = C.weights(oracle, "LMHEAD", wtype, M, K)
    aq = C.columns("LMHEAD", R.Q81[wtype], K, N)
    rows = np.unique(np.concatenate([C.hostile_rows(M), C._rng(9, wtype).integers(0, M, 256)]))
    ref = R.block_sums(wtype, W, M, K, *aq, rows=rows)
    args = dict(op="LMHEAD", wtype=wtype, M=M, N=N, w_rows=W, aq_q=aq[0], aq_d=aq[1], aq_s=aq[2])
    outs = {}
    for route in ("VALU_8", "MFMA_1"):
        got = pkg.chain_device(route=route, **args)
        exp = C.expected_launch("LMHEAD", route, wtype, M, K, N) + C.geometry(M, N)
        assert tuple(got["launched"][:7]) == exp, (route, list(got["launched"]), exp)
        out = got["out"]
        assert (out[:N, rows].view(np.uint32) == ref.view(np.uint32)).all(), (route, R.NAMES[wtype], np.argwhere(out[:N, rows].view(np.uint32) != ref.view(np.uint32))[:6])
        assert (out[N:].view(np.uint8) == 0xff).all() and (out[:, M:].view(np.uint8) == 0xff).all(), (route, "a store beyond column N or row M")
        assert np.isfinite(out[:N, :M]).all()
        outs[route] = out
    assert (outs["VALU_8"].view(np.uint32) == outs["MFMA_1"].view(np.uint32)).all()


@pytest.mark.parametrize("q81", [False, True], ids=["q8_0", "q8_1"])
def test_lnq_equals_the_restatement(pkg, oracle, q81):
    args, want = C.build_lnq(q81)
    C.compare(pkg.chain_device(**args), want, ("LNQ", q81))


@pytest.mark.parametrize("wtype", R.TYPES, ids=[R.NAMES[t] for t in R.TYPES])
def test_one_column_fc1_with_layernorm_equals_the_restatement(pkg, oracle, wtype):
    for row in C.FC1_LN_ROWS:
        args, want = C.build_fc1_ln(oracle, wtype, row)
        run(pkg, oracle, args, want, "VALU_1", "FC1_LN %s row %d" % (R.NAMES[wtype], row))


def test_matrix_cores_refused_for_rows_that_are_no_whole_tiles(pkg, oracle):
    args, _ = C.build(oracle, "LMHEAD", R.Q4_0, 64, M=1045)
    with pytest.raises(pkg.BiogptError, match="whole number of 16-row tiles"):
        pkg.chain_device(route="MFMA_1", **args)
