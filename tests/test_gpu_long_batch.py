"""The batched calls of a wide file at 1025 .. 2048 keys (csrc/kernels_attn_long_cols.hip.h): whole calls over column states on the tiny wide
file of tests/test_gpu_long_context.py (2 layers, 3 heads of 64, d_ff 160, 2048 positions), bit for bit against the same build's single-context calls, and the
launch counters that say which kernels attended.  Before these kernels every call here was refused."""
import numpy as np
import pytest

from test_gpu_long_context import L, TOKS, TYPES, W, files  # noqa: F401  (files: the module's fixture)
from test_gpu_wide_decode import bits

pytestmark = pytest.mark.gpu

SEQS = [TOKS[:2048], TOKS[100:1200], TOKS[300:340]]
PROMPTS = [TOKS[:1015], TOKS[50:650], TOKS[700:720]]
PREFIX, CONTS = TOKS[:1500], [TOKS[1500:1505], TOKS[40:43], TOKS[900:909]]


@pytest.mark.parametrize("name", TYPES)
def test_batched_calls_equal_the_single_calls(pkg, files, name):
    g, one = pkg.BiogptModel.load(files[name]), pkg.BiogptModel.load(files[name], long_context=True)
    try:
        got = g.score_batch(SEQS)
        for s, triple in zip(SEQS, got):
            for a, b in zip(triple, one.score(s)):
                assert (bits(a) == bits(b)).all(), (name, "score_batch", len(s))
        # passes of 512 columns: [1024, 1536) and [1536, 2048) of the first sequence, and the last 76 + 40 columns, see beyond 1024 keys
        assert g.long_cols_launches() == 3 * L and g.long_attn_launches() == 0
        n0 = g.long_cols_launches()
        ids = g.generate_greedy_batch(PROMPTS, 24)[0]
        for p, row in zip(PROMPTS, ids):
            assert list(row) == list(one.generate_greedy(p, 24)[0]), (name, "generate_greedy_batch", len(p))
        assert g.long_cols_launches() > n0 and (g.long_cols_launches() - n0) % L == 0      # (steps at 1025 .. 1038 keys, enqueued or captured once)
        n0 = g.long_cols_launches()
        for c, triple in zip(CONTS, g.score_continuations(PREFIX, CONTS)):
            for a, b in zip(triple, one.score(PREFIX + c)):
                assert (bits(a) == bits(b[len(PREFIX) - 1:-1])).all(), (name, "score_continuations", len(c))
        assert g.long_cols_launches() == n0 + L and g.long_attn_launches() == 0      # (the third pass: 475 prefix columns and the 17 scored ones)
    finally:
        g.close(); one.close()


def test_sampling_does_not_depend_on_the_form(pkg, files, monkeypatch):
    """generate_sample with a seed: the run form where the rule takes it against a context that takes the column form everywhere."""
    rule = pkg.BiogptModel.load(files["q5_1"])
    monkeypatch.setenv("BIOGPT_HIP_LONG_RUNS", "0")
    cols = pkg.BiogptModel.load(files["q5_1"])
    try:
        a = rule.generate_sample([TOKS[:1100], TOKS[200:230]], 12, n_samples=2, seed=7)[0]
        b = cols.generate_sample([TOKS[:1100], TOKS[200:230]], 12, n_samples=2, seed=7)[0]
        assert [list(x) for x in a] == [list(x) for x in b] and all(len(x) == 12 for x in a)
        assert rule.long_cols_launches() > 0 and cols.long_cols_launches() > 0 and rule.long_attn_launches() == 0
    finally:
        rule.close(); cols.close()


def test_short_tables_never_launch_the_long_kernels(pkg, tmp_path):
    f32, q = str(tmp_path / "w96_f32.bin"), str(tmp_path / "w96_q4_0.bin")
    pkg.write_synthetic(f32, **dict(W, n_positions=96))
    pkg.quantize_file(f32, q, "q4_0")
    g = pkg.BiogptModel.load(q)
    try:
        g.score_batch([TOKS[:96], TOKS[5:40]])
        g.generate_greedy_batch([TOKS[:30], TOKS[40:50]], 8)
        assert g.long_cols_launches() == 0 and g.long_attn_launches() == 0
    finally:
        g.close()
