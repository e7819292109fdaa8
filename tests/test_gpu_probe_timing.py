"""The timed entries of the kernel probes (biogpt_hip_*_bench) at the smallest shapes each accepts: every one of them returns reps finite, positive times.
The two whose launch consumes its input -- the trie rows (rewritten in place) and the sampler (generator states advanced) -- are also held to what the
untimed entry gives on the same input: the rows the timed entry hands back, the caller's states it leaves alone, and a second untimed run afterwards.
This does NOT show that the device copy is restored in front of each timed launch: the rows are read back before the timed launches, the timed sampler
entry returns no states, and no entry returns what the device holds after the last timed launch.  The restore step is covered by reading the code alone."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPS = 3


def timed(t):
    t = np.asarray(t, dtype=np.float64)
    assert t.shape == (REPS,) and np.isfinite(t).all() and (t > 0).all(), t


def test_trie_rows_bench(pkg):
    V = 33
    rows = np.random.default_rng(1).standard_normal((2, V)).astype(np.float32)
    trie = pkg.Trie.build([[5, 7, 9], [5, 8], [11]], V)
    hist = [[5], []]
    for mode in (0, 1):
        want = pkg.trie_rows(rows, trie, hist, mode=mode)
        got, us = pkg.trie_rows(rows, trie, hist, mode=mode, reps=REPS)
        timed(us)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), mode
        assert np.array_equal(pkg.trie_rows(rows, trie, hist, mode=mode).view(np.uint32), want.view(np.uint32)), mode
    trie.close()


@pytest.mark.parametrize("which", [0, 1])
def test_sampler_rows_bench(pkg, which):
    V = 33
    rows = np.random.default_rng(2).standard_normal((2, V)).astype(np.float32)
    sampler = (8, 0.9, 0.0, 0.8)
    seeded = np.zeros((2, 625), np.uint32)
    for r in range(2):
        assert pkg.lib().biogpt_hip_mt19937_seed(40 + r, seeded[r].ctypes.data) == 0

    def draw(states):
        if which == 0:
            return pkg.sample_wide_rows(rows, sampler, states)[0]
        ids = np.zeros(2, np.int32)
        assert pkg.lib().biogpt_hip_sample_rows_device(0, rows.ctypes.data, 2, V, 8, 0.9, 0.8, states.ctypes.data, ids.ctypes.data) == 0, pkg._err()
        return ids

    first = seeded.copy()
    want = draw(first)                       # first: the states after one launch
    states = seeded.copy()
    timed(pkg.sample_wide_rows_bench(rows, sampler, states, which=which, reps=REPS))
    assert np.array_equal(states, seeded)    # every timed launch began from the states as given
    assert np.array_equal(draw(states), want) and np.array_equal(states, first)


def test_linear_stage_benches(pkg):
    timed(pkg.wide_chain_bench("wide", 2, 16, 32, 1, reps=REPS))      # Q4_0
    timed(pkg.fchain_bench("float", 0, 1, 32, 1, reps=REPS))
    timed(pkg.fchain_bench("generic", 0, 1, 32, 1, reps=REPS))


def test_attention_benches(pkg):
    """One head, two columns behind a shared row in a table of four: the runs kernel (packed columns) and both kernels of the prefix entry."""
    H, N, P = 1, 2, 4
    rng = np.random.default_rng(3)
    q = rng.standard_normal((N, 64)).astype(np.float32)
    k, v = (rng.standard_normal((N + 1, H, P, 64)).astype(np.float32) for _ in range(2))
    st = np.zeros((N, 8), np.int32)
    st[:, 0] = [1, 2]          # n_past
    st[:, 3] = [0, 1]          # seq_id: the column's own slot
    st[:, 4] = [2, 3]          # t_vis
    st[:, 5] = 1               # one shared row ...
    st[:, 6] = N               # ... in the last slot
    res = pkg.attn_runs_device(H, P, 3, N + 1, q, k, v, st, reps=REPS)
    assert res[0] == 0, pkg._err()
    timed(res[6])
    same = st.copy()
    same[:, 0] = 1             # a decode step: both columns at position 1
    out, us = np.zeros_like(q), np.zeros(REPS, np.float32)
    for which in (0, 1):
        rc = pkg.lib().biogpt_hip_attn_prefix_bench(0, H, N, P, P, q.ctypes.data, k.ctypes.data, v.ctypes.data, same.ctypes.data, which, 0, out.ctypes.data, None, None, None,
                                                    REPS, us.ctypes.data)
        assert rc == 0, pkg._err()
        timed(us)
