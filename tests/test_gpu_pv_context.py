"""The PV loop of the pipelined decode launch's attention stage (csrc/kernels_xpipe.hip.h, stage B of xp_run) at every context length up to 272 keys: every
count of old keys per wave in the 64- / 128- / 192- / 256-key variants and with two workgroups per head, the token's own key in every wave and in slots of
both parities, on files with peaked attention (many softmax weights exactly 0).  tests/pv_context_rows.py states the rows; tests/test_pv_context_rows.py
holds them, on the CPU, to the cap on rows without an arg-max assertion.

Every row: finite, max |diff| <= 1e-3 and bit-identical to the oracle (the contract of test_gpu_wide.Tally); the arg-max where the oracle row's top-two gap
is at least 2e-3 (computed here from the oracle row), which at most 1 row in 20 may miss."""
import numpy as np
import pytest

import pv_context_rows as pc
import wide_models as wm

pytestmark = pytest.mark.gpu

ATOL = 1e-3          # the contract's bar on logits


@pytest.fixture(scope="module")
def files(pkg, tmp_path_factory):
    return wm.build(pkg, tmp_path_factory.mktemp("pv"), pc.FILES)


@pytest.fixture(scope="module")
def walks(oracle, files):
    """The oracle's rows of a file's walk, computed once and shared by the two launch forms."""
    memo = {}

    def get(name):
        if name not in memo:
            toks, rows = pc.oracle_walk(oracle, files[name], name, n_threads=16)
            rows.setflags(write=False)
            memo[name] = (toks, rows)
        return memo[name]
    return get


@pytest.mark.parametrize("resident", [True, False], ids=["resident", "per-call"])
@pytest.mark.parametrize("name", pc.FILES)
def test_single_tokens_at_every_context_length(pkg, files, walks, monkeypatch, name, resident):
    toks, rows = walks(name)
    close = set(pc.close_rows(rows))
    assert len(close) <= pc.CAP * pc.N_ROWS, "%d rows of the walk have a top-two gap below %g: another seed" % (len(close), pc.GAP)
    if not resident:
        monkeypatch.setenv("BIOGPT_HIP_RESIDENT", "0")      # options are read when the context is created
    g = pkg.BiogptModel.load(files[name])
    if not resident:
        monkeypatch.delenv("BIOGPT_HIP_RESIDENT")
    try:
        assert g.xpipe_state() == 1
        what = "%s, %s" % (name, "resident launch" if resident else "one launch per call")
        worst, same = 0.0, 0
        for n_past in range(pc.N_ROWS):
            got, ref = g.eval([toks[n_past]], n_past), rows[n_past]
            d = float(np.abs(got - ref).max())
            worst, same = max(worst, d), same + int((got == ref).all())
            assert np.isfinite(got).all(), "%s at %d: output not finite" % (what, n_past)
            assert d <= ATOL, "%s at %d: max |diff| %.3e" % (what, n_past, d)
            if n_past not in close:
                assert int(got.argmax()) == int(ref.argmax()), "%s at %d: arg-max %d, oracle %d" % (what, n_past, got.argmax(), ref.argmax())
            assert (got == ref).all(), "%s at %d: not bit-identical to the oracle, max |diff| %.3e in %d elements" % (what, n_past, d, int((got != ref).sum()))
        print("%s: %d rows, worst |diff| %.2e, %d bit-identical, %d without an arg-max assertion" % (what, pc.N_ROWS, worst, same, len(close)))
        assert g.xpipe_state() == 1, "the persistent launch was abandoned on the way"
    finally:
        g.close()


@pytest.mark.parametrize("name", pc.FILES)
def test_multi_token_launches_in_every_variant(pkg, oracle, files, name):
    """generate_greedy (several tokens per launch) from one prompt per variant: 58 ids equal to the oracle's."""
    g = pkg.BiogptModel.load(files[name])
    try:
        assert g.xpipe_state() == 1
        for n_prompt in pc.PROMPTS:
            prompt = pc.prompt_tokens(name, n_prompt)
            ids, _ = g.generate_greedy(prompt, pc.N_GEN)
            o = oracle.OracleModel(files[name], n_threads=16)
            ref, _ = o.generate_greedy(prompt, pc.N_GEN)
            o.close()
            first = next((k for k in range(min(len(ids), len(ref))) if ids[k] != ref[k]), min(len(ids), len(ref)))
            assert list(ids) == list(ref), "%s, prompt of %d: %d ids, the oracle %d; they differ from token %d on" % (name, n_prompt, len(ids), len(ref), first)
        assert g.xpipe_state() == 1, "the persistent launch was abandoned on the way"
    finally:
        g.close()
