"""attn_prefix_kernel<8> (decode attention of eight columns behind one shared prefix per workgroup) through biogpt_hip_attn_prefix_device: bit for bit the
f32 rows and the Q8 blocks of the existing attn_fast_kernel<4, false, true> on the same inputs.  The existing kernel is the reference here; both kernels are
held to the oracle's attention, alone and bit for bit, by tests/test_gpu_attn_kernels.py.  A mismatch here is a finding to report with its rows, not a
tolerance to add."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

H = 2
SENTINEL = np.float32(3.0e30)      # large and finite: a row that must not be read as a key or value shows up as inf / nan or a wrong row


def make_inputs(seed, N, P, n_shared, peak=None, max_own=8):
    """Column i sees n_shared shared rows and 1 + (i * 3 + seed) % max_own own rows (mixed within a group of eight).  Returns q, k, v, states, t_cap."""
    rng = np.random.default_rng(seed)
    own = np.array([1 + (i * 3 + seed) % max_own for i in range(N)])
    T = n_shared + own
    t_cap = int(min(P, (int(T.max()) + 63) // 64 * 64))
    assert T.max() <= t_cap
    q = rng.standard_normal((N, H, 64)).astype(np.float32)
    k = np.full((N + 1, H, P, 64), SENTINEL, dtype=np.float32)
    v = np.full((N + 1, H, P, 64), SENTINEL, dtype=np.float32)
    for a in (k, v):
        a[N, :, :n_shared] = rng.standard_normal((H, n_shared, 64)).astype(np.float32)
        for i in range(N):
            a[i, :, n_shared:T[i]] = rng.standard_normal((H, int(own[i]), 64)).astype(np.float32)
    if peak == "shared":        # one shared key 30 above the rest for column 0 (and wherever else q points that way)
        k[N, :, n_shared // 2] = q[0] * (30.0 / (q[0] ** 2).sum(axis=-1, keepdims=True))
    if peak == "own":           # every column's last own key 30 above the rest
        for i in range(N):
            k[i, :, T[i] - 1] = q[i] * (30.0 / (q[i] ** 2).sum(axis=-1, keepdims=True))
    st = np.zeros((N, 8), dtype=np.int32)
    st[:, 0] = T - 1            # n_past: the column's own token is its last key
    st[:, 3] = np.arange(N)     # seq_id
    st[:, 5] = n_shared         # pad[0]
    st[:, 6] = N                # pad[1]: the prefix slot
    return q.reshape(N, H * 64), k, v, st, t_cap


def run(pkg, which, q8, q, k, v, st, P, t_cap):
    N, D = q.shape
    out = np.zeros((N, D), dtype=np.float32)
    oq = np.zeros((N, D), dtype=np.int8)
    od = np.zeros((N, D // 32), dtype=np.float32)
    os_ = np.zeros((N, D // 32), dtype=np.uint32)
    rc = pkg.lib().biogpt_hip_attn_prefix_device(0, H, N, P, t_cap, q.ctypes.data, k.ctypes.data, v.ctypes.data, st.ctypes.data, which, q8, out.ctypes.data,
                                                 oq.ctypes.data, od.ctypes.data, os_.ctypes.data)
    assert rc == 0, pkg._err()
    return out, oq, od, os_


def check(pkg, what, N, P, n_shared, peak=None, seed=1, max_own=8):
    q, k, v, st, t_cap = make_inputs(seed + N + n_shared, N, P, n_shared, peak, max_own)
    for q8 in (1, 2):
        ref = run(pkg, 0, q8, q, k, v, st, P, t_cap)
        assert np.isfinite(ref[0]).all() and np.abs(ref[0]).max() < 1e3, (what, "the existing kernel read a sentinel row")
        assert np.isfinite(ref[2]).all()
        got = run(pkg, 1, q8, q, k, v, st, P, t_cap)
        bad = np.argwhere(got[0].view(np.uint32) != ref[0].view(np.uint32))
        assert bad.size == 0, (what, q8, len(bad), [(int(i), int(j), float(got[0][i, j]), float(ref[0][i, j])) for i, j in bad[:6]])
        for name, x, y in zip(("q", "d", "s"), got[1:], ref[1:]):
            assert (x.view(np.uint8) == y.view(np.uint8)).all(), (what, q8, name, np.argwhere(x != y)[:6])


@pytest.mark.parametrize("n_shared", [0, 1, 3, 64, 65, 120])
@pytest.mark.parametrize("N", [1, 8, 9, 19])
@pytest.mark.parametrize("P", [128, 1024])
def test_prefix_attention_equals_the_existing_kernel(pkg, P, N, n_shared):
    check(pkg, "P %d N %d shared %d" % (P, N, n_shared), N, P, n_shared)


@pytest.mark.parametrize("peak", ["shared", "own"])
@pytest.mark.parametrize("N,n_shared", [(9, 65), (19, 120)])
def test_prefix_attention_peaked_rows(pkg, N, n_shared, peak):
    check(pkg, "peak %s N %d shared %d" % (peak, N, n_shared), N, 1024, n_shared, peak=peak, seed=7)


@pytest.mark.parametrize("N,n_shared", [(9, 0), (19, 65), (19, 300)])
def test_prefix_attention_many_own_rows(pkg, N, n_shared):
    """1 .. 41 own rows, mixed within a group: the own-row score sweep (16 keys) and the own-row PV loop (stride 8) run several rounds with tails, as in a
    generation call (suffix + generated tokens)."""
    check(pkg, "own rows to 41, N %d shared %d" % (N, n_shared), N, 1024, n_shared, seed=3, max_own=41)


def test_prefix_attention_probe_argument_errors(pkg):
    q, k, v, st, t_cap = make_inputs(3, 9, 128, 3)
    out = np.zeros_like(q)
    f = pkg.lib().biogpt_hip_attn_prefix_device
    args = lambda **kw: [kw.get("H", H), kw.get("N", 9), kw.get("P", 128), kw.get("t_cap", t_cap), q.ctypes.data, k.ctypes.data, v.ctypes.data,
                         kw.get("st", st).ctypes.data, kw.get("which", 1), kw.get("q8", 0), out.ctypes.data, None, None, None]
    assert f(0, *args()) == 0
    mixed = st.copy(); mixed[4, 5] = 2
    past = st.copy(); past[2, 0] = t_cap
    for field, kw in [("which", dict(which=2)), ("t_cap", dict(t_cap=129)), ("P must", dict(P=2048)), ("q8", dict(q8=1)), ("one shared range", dict(st=mixed)),
                      ("n_past", dict(st=past))]:
        assert f(0, *args(**kw)) == -1
        assert field in pkg._err(), (field, pkg._err())
    us = np.zeros(3, dtype=np.float32)
    assert pkg.lib().biogpt_hip_attn_prefix_bench(0, *args(), 3, us.ctypes.data) == 0 and (us > 0).all()
    assert pkg.lib().biogpt_hip_attn_prefix_bench(0, *args(), 0, us.ctypes.data) == -1
