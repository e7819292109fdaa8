"""The kernels of the token tail, each alone, through biogpt_hip_tail_device, which launches through the helpers of the engine's own calls: the lm_head's arg-max
partials (lm_stream_kernel, matvec_fast_kernel, matvec_kernel), argmax_kernel and topk_kernel on every case of tests/tail_cases.py -- tied, infinite and NaN rows
no whole call produces.  Everything is held to tests/tail_ref.py exactly: the partials to partials() of the row the kernel itself returned (a pure selection
check), that row's bits to tests/chain_ref.py for the block formats, the finisher's token to finish(), topk_kernel to its outcome -- the k pairs of topk(), or -1
where the restatement says so.  Every guard entry keeps its 0xff preset.  No model files."""
import numpy as np
import pytest

import chain_ref as R
import tail_cases as C
import tail_ref as T

pytestmark = pytest.mark.gpu
F32 = np.float32


def _preset(a, what):
    assert (np.asarray(a).view(np.uint32) == 0xFFFFFFFF).all(), what


def run_partials(pkg, wtype, M, edits=False, lm_stream=True):
    c = C.partials_case(wtype, M, edits, lm_stream)
    x, w, b = C.column()
    got = pkg.tail_device("PARTIALS", wtype=wtype, w_rows=c["raw"], M=M, x=x, ln_w=w, ln_b=b)
    what = (R.NAMES.get(wtype, "f32"), M, edits, lm_stream)
    assert (got["kernel"], got["rows_per_part"]) == (C.expected_kernel(wtype, M, lm_stream), c["rpp"]), (what, got["launched"])
    nparts = -(-M // c["rpp"])
    assert got["grid"] == nparts, (what, got["launched"])
    row = got["row"][:M]
    _preset(got["row"][M:], what)
    _preset(got["pmax_val"][nparts:], what)
    _preset(got["pmax_idx"][nparts:], what)
    pv, pi = T.partials(row, c["rpp"])
    bad = np.flatnonzero((got["pmax_val"][:nparts].view(np.uint32) != pv.view(np.uint32)) | (got["pmax_idx"][:nparts] != pi))
    print("%s: %d partials, %d differ" % (what, nparts, bad.size))
    assert bad.size == 0, (what, [(int(p), float(got["pmax_val"][p]), int(got["pmax_idx"][p]), float(pv[p]), int(pi[p])) for p in bad[:6]])
    if wtype != C.F32_TYPE:
        assert C.same_row(row, c["want"]), what
    else:
        np.testing.assert_allclose(row, c["want"], rtol=0, atol=1e-4)      # (the float kernel's row is not this test's subject: only that the right weights were read)
    return got


@pytest.mark.parametrize("wtype", (C.F32_TYPE,) + R.TYPES, ids=("f32",) + tuple(R.NAMES[t] for t in R.TYPES))
def test_partials_on_tied_rows(pkg, wtype):
    for M in C.PARTIAL_M:
        run_partials(pkg, wtype, M)


def test_partials_on_nan_and_inf_rows_small(pkg):
    run_partials(pkg, R.Q8_0, 1045, edits=True)


def test_partials_full_grid_stream_kernel(pkg):
    got = run_partials(pkg, R.Q8_0, C.FULL_M, edits=True)
    assert got["grid"] == 663 and got["kernel"] == 0


def test_partials_full_grid_block_kernel(pkg, monkeypatch):
    monkeypatch.setenv("BIOGPT_HIP_LM_STREAM", "0")
    got = run_partials(pkg, R.Q8_0, C.FULL_M, edits=True, lm_stream=False)
    assert got["grid"] == 663 and got["kernel"] == 1


def test_partials_f32_nan_and_inf_rows(pkg):
    """The generic kernel's epilogue on NaN / inf logits: float weights of NaN and inf."""
    M = 1045
    raw = C.base_weights(C.F32_TYPE, M).copy()
    x, w, b = C.column()
    raw[[0, 5, 300, 1044]] = np.nan
    raw[[7, 301], 0] = np.inf
    raw[[2, 640], 0] = -np.inf
    got = pkg.tail_device("PARTIALS", wtype=0, w_rows=raw, M=M, x=x, ln_w=w, ln_b=b)
    rpp, row = got["rows_per_part"], got["row"][:M]
    assert rpp == C.rows_per_part(C.F32_TYPE, M) and np.isnan(row[[0, 5, 300, 1044]]).all() and np.isinf(row[[7, 301, 2, 640]]).all()
    pv, pi = T.partials(row, rpp)
    n = len(pv)
    assert got["pmax_val"][:n].tobytes() == pv.tobytes() and got["pmax_idx"][:n].tolist() == pi.tolist()
    _preset(got["pmax_val"][n:], "f32")


def test_finish(pkg):
    P = 8
    for name, v, i in C.finish_cases():
        for state, n_eval in (((5, 2, 0, 0), 1), ((0, P, 0, 0), 3)):      # a free gen_ids slot; none (n_gen == n_positions: the id is not recorded)
            got = pkg.tail_device("FINISH", pmax_val=v, pmax_idx=i, state=state, n_eval=n_eval, n_positions=P, n_vocab=C.N_VOCAB)
            want = T.finish(v, i, C.N_VOCAB)
            print("%s: token %d, want %d" % (name, got["token"], want))
            assert got["token"] == want, (name, got["token"], want)
            assert (got["n_past"], got["n_gen"]) == (state[0] + n_eval, state[1] + 1) and got["block"][2:4].tolist() == [0, 0], name
            assert got["recorded"] == (want if state[1] < P else None), name
            blk = got["block"].copy()
            blk[4] = -1
            if state[1] < P:
                blk[4 + P + state[1]] = -1
            assert (blk[4:] == -1).all(), name      # nothing else written: tokens, gen_ids, guard


def test_topk(pkg):
    refused = 0
    for c in C.topk_cases():
        row, k, pm, name = c["row"], c["k"], c["pmax"], c["name"]
        n, v, i = T.topk_kernel(row, pm, pm.size, k)
        got = pkg.tail_device("TOPK", row=row, pmax_val=pm, k=k)
        assert got["n"] == n, (name, got["n"], n)
        assert (got["count"][1:] == -1).all(), name
        if n == k:
            assert got["vals"][:k].tobytes() == v.tobytes() and got["ids"][:k].tolist() == i.tolist(), name
            _preset(got["vals"][k:], name)
            _preset(got["ids"][k:], name)
        else:
            refused += 1
            _preset(got["vals"], name)      # a refusal writes no pair
            _preset(got["ids"], name)
    assert refused >= 12
