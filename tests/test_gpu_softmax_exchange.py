"""The softmax of the pipelined decode launch's attention stage (csrc/kernels_xpipe.hip.h, stage B of xp_run) at the contexts where its two forms can go wrong:
one exchange up to 128 keys (two numerator registers per lane, one unsigned sum of numerator * 2^24, the PV loop's weights by register and lane), two exchanges
beyond, and the stage's tail (eight slice sums read together, added from s0 and s1 on).  tests/softmax_exchange_rows.py states the files and rows -- peaked attention (numerators
exactly 0 and 1.0) and uniform attention (every numerator 1.0: the largest sum); tests/test_softmax_exchange_rows.py holds them, on the CPU, to the cap on rows
without an arg-max assertion.

Every row: finite, max |diff| <= 1e-3 and bit-identical to the oracle (the contract of test_gpu_wide.Tally); the arg-max where the oracle row's top-two gap
is at least 2e-3 (computed here from the oracle row), which at most 1 row in 20 may miss."""
import numpy as np
import pytest

import softmax_exchange_rows as sx

pytestmark = pytest.mark.gpu

ATOL = 1e-3          # the contract's bar on logits


@pytest.fixture(scope="module")
def files(pkg, tmp_path_factory):
    return sx.build(pkg, tmp_path_factory.mktemp("sx"))


@pytest.fixture(scope="module")
def rows_of(oracle, files):
    """The oracle's compared rows of a file, computed once and shared by the two launch forms."""
    memo = {}

    def get(name):
        if name not in memo:
            memo[name] = sx.oracle_rows(oracle, files[name], name, n_threads=16)
        return memo[name]
    return get


@pytest.mark.parametrize("resident", [True, False], ids=["resident", "per-call"])
@pytest.mark.parametrize("name", sx.FILES)
def test_single_tokens_at_the_contexts_of_both_softmax_forms(pkg, files, rows_of, monkeypatch, name, resident):
    rows = rows_of(name)
    close = set(sx.close_rows(rows))
    assert len(close) <= sx.CAP * len(rows), "%d compared rows have a top-two gap below %g: another seed" % (len(close), sx.GAP)
    if not resident:
        monkeypatch.setenv("BIOGPT_HIP_RESIDENT", "0")      # options are read when the context is created
    g = pkg.BiogptModel.load(files[name])
    if not resident:
        monkeypatch.delenv("BIOGPT_HIP_RESIDENT")
    try:
        assert g.xpipe_state() == 1
        what = "%s, %s" % (name, "resident launch" if resident else "one launch per call")
        worst, same = 0.0, 0
        for toks, n_past, compared in sx.plan(name):
            got = g.eval(toks, n_past)
            if not compared:
                continue
            ref = rows[n_past]
            d = float(np.abs(got - ref).max())
            worst, same = max(worst, d), same + int((got == ref).all())
            print("%s at %d: max |diff| %.3e, %d elements differ" % (what, n_past, d, int((got != ref).sum())))
            assert np.isfinite(got).all(), "%s at %d: output not finite" % (what, n_past)
            assert d <= ATOL, "%s at %d: max |diff| %.3e" % (what, n_past, d)
            if n_past not in close:
                assert int(got.argmax()) == int(ref.argmax()), "%s at %d: arg-max %d, oracle %d" % (what, n_past, got.argmax(), ref.argmax())
            assert (got == ref).all(), "%s at %d: not bit-identical to the oracle, max |diff| %.3e in %d elements" % (what, n_past, d, int((got != ref).sum()))
        print("%s: %d rows, worst |diff| %.2e, %d bit-identical, %d without an arg-max assertion" % (what, len(rows), worst, same, len(close)))
        assert g.xpipe_state() == 1, "the persistent launch was abandoned on the way"
    finally:
        g.close()


@pytest.mark.parametrize("name", sx.GEN_FILES)
def test_multi_token_launches_across_the_variants(pkg, oracle, files, name):
    """generate_greedy (several tokens per launch) from 60 keys to 199: the 64-, 128-, 192- and 256-key variants in one call, ids equal to the oracle's."""
    g = pkg.BiogptModel.load(files[name])
    try:
        assert g.xpipe_state() == 1
        prompt = sx.prompt_tokens(name)
        ids, _ = g.generate_greedy(prompt, sx.N_GEN)
        o = oracle.OracleModel(files[name], n_threads=16)
        ref, _ = o.generate_greedy(prompt, sx.N_GEN)
        o.close()
        first = next((k for k in range(min(len(ids), len(ref))) if ids[k] != ref[k]), min(len(ids), len(ref)))
        assert list(ids) == list(ref), "%s: %d ids, the oracle %d; they differ from token %d on" % (name, len(ids), len(ref), first)
        assert g.xpipe_state() == 1, "the persistent launch was abandoned on the way"
    finally:
        g.close()
