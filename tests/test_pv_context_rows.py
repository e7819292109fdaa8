"""CPU check of the inputs of tests/test_gpu_pv_context.py (tests/pv_context_rows.py): on every file of the walk the oracle is finite and at most 1 row in 20
has a top-two gap below 2e-3 -- the rows on which the GPU test does not ask for the arg-max.  A seed that misses the cap is replaced in pv_context_rows.SEEDS."""
import numpy as np
import pytest

import pv_context_rows as pc
import wide_models as wm


@pytest.fixture(scope="module")
def files(pkg, tmp_path_factory):
    return wm.build(pkg, tmp_path_factory.mktemp("pv_cpu"), pc.FILES)


@pytest.mark.parametrize("name", pc.FILES)
def test_walk_rows_are_finite_and_few_are_close(oracle, files, name):
    toks, rows = pc.oracle_walk(oracle, files[name], name, n_threads=8)
    assert rows.shape == (pc.N_ROWS, wm.V) and np.isfinite(rows).all()
    close = pc.close_rows(rows)
    print("%s: %d of %d rows with a top-two gap below %g: n_past %s" % (name, len(close), pc.N_ROWS, pc.GAP, close))
    assert len(close) <= pc.CAP * pc.N_ROWS
