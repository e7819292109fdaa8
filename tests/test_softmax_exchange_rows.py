"""CPU check of the inputs of tests/test_gpu_softmax_exchange.py (tests/softmax_exchange_rows.py): on every file the oracle's compared rows are finite and at
most 1 in 20 has a top-two gap below 2e-3 -- the rows on which the GPU test does not ask for the arg-max -- and the files are what they claim: in layers 0
and 1 of a uniform file every q row is exactly 0.  A seed that misses the cap is replaced in softmax_exchange_rows.SEEDS."""
import numpy as np
import pytest

import softmax_exchange_rows as sx
import wide_models as wm


@pytest.fixture(scope="module")
def files(pkg, tmp_path_factory):
    return sx.build(pkg, tmp_path_factory.mktemp("sx_cpu"))


def test_the_plan_meets_every_context_once_and_in_order():
    for name in sx.FILES:
        steps = sx.plan(name)
        assert [n_past for _, n_past, compared in steps if compared] == list(sx.CONTEXTS)
        at = 0
        for toks, n_past, compared in steps:
            assert n_past == at and 1 <= len(toks) <= 8 and (len(toks) == 1 or not compared)
            at += len(toks)
        assert at == sx.CONTEXTS[-1] + 1
    assert {c & 7 for c in sx.CONTEXTS if 64 <= c < 128} == set(range(8)), "the token's own key in every wave of the 128-key variant"


def test_uniform_zeroes_the_q_rows_of_two_layers():
    W = {wm.lname(l, "self_attn.q_proj.%s" % part): np.ones(4, np.float32) for l in range(wm.L) for part in ("weight", "bias")}
    sx.uniform(W)
    for l in range(wm.L):
        for part in ("weight", "bias"):
            assert (W[wm.lname(l, "self_attn.q_proj.%s" % part)] == (0.0 if l < 2 else 1.0)).all()


@pytest.mark.parametrize("name", sx.FILES)
def test_compared_rows_are_finite_and_few_are_close(oracle, files, name):
    rows = sx.oracle_rows(oracle, files[name], name, n_threads=8)
    assert sorted(rows) == sorted(sx.CONTEXTS)
    assert all(r.shape == (wm.V,) and np.isfinite(r).all() for r in rows.values())
    close = sx.close_rows(rows)
    print("%s: %d of %d rows with a top-two gap below %g: n_past %s" % (name, len(close), len(rows), sx.GAP, close))
    assert len(close) <= sx.CAP * len(rows)
