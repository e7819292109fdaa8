"""Every stand-alone attention kernel, alone, against the oracle's attention (oracle/biogpt_oracle.c, bo_attn_head): attn_fast_kernel<1, true>, <2, false>,
<4, false> at 1024 threads and as the slim launch, each plain and SHARED; attn_prefix_kernel<8>; the three attn_split_* launches; attn_group_kernel<8>;
attn_tile_kernel<16, true> and <16, false>; the generic attn_kernel.  biogpt_hip_attn_device launches them through the launch code of the engine's own
passes and reports the kernel and geometry it launched; the cases are those of tests/attn_cases.py, whose oracle rows tests/test_attn_restatement.py examines
on the CPU (no committed case has a fragile row, so bit equality is owed everywhere).

Every visible column's outputs equal the oracle's bit for bit; the Q8 codes, d and s equal the oracle's quantizer on the oracle's row; columns from N on and
the guard row still hold 0xff.  The kernels differ from the oracle only in how they associate the double sums: a row the restatement (tests/attn_ref.py) finds
fragile there would be held to one float32 ulp instead -- looked up only when a row differs."""
import numpy as np
import pytest

import attn_cases as A

pytestmark = pytest.mark.gpu


def launch(pkg, c, **over):
    """The case through the probe: (rc, out, out_q, out_d, out_s, launched).  over: arguments replaced (the argument-error test)."""
    k, v = over.pop("kv", None) or c.slots()
    dev, st = c.states()
    D, rows = A.H * c.dk, (c.N + 15) // 16 * 16 + 1
    out = np.zeros((rows, D), dtype=np.float32)
    oq, od, os_ = np.zeros((rows, D), dtype=np.int8), np.zeros((rows, D // 32), dtype=np.float32), np.zeros((rows, D // 32), dtype=np.uint32)
    launched = np.full(8, -1, dtype=np.int32)
    a = dict(route=c.route, H=A.H, dk=c.dk, N=c.N, P=c.P, t_max=c.t_max, n_slots=c.n_slots, dev=dev, st=st, col_mode=c.col_mode, q8=c.q8)
    a.update(over)
    ptr = lambda x: None if x is None else x.ctypes.data
    q8 = a["q8"]
    rc = pkg.lib().biogpt_hip_attn_device(0, a["route"], a["H"], a["dk"], a["N"], a["P"], a["t_max"], a["n_slots"], c.q.ctypes.data, k.ctypes.data, v.ctypes.data, ptr(a["dev"]),
                                          ptr(a["st"]), a["col_mode"], q8, out.ctypes.data, ptr(oq) if q8 else None, ptr(od) if q8 else None, ptr(os_) if q8 else None,
                                          launched.ctypes.data)
    return rc, out, oq, od, os_, launched


def oracle_q8(oracle, row, form):
    """The oracle's quantizer on a row: codes int8 [D], d as the float the kernels store (Q8_0: the fp16 value), s as 32 bits (Q8_0: the code sum, Q8_1: the float)."""
    nb = row.size // 32
    if form == 1:
        b = np.frombuffer(oracle.quantize(oracle.TYPE_Q8_0, row, row.size).tobytes(), dtype=np.dtype([("d", "<u2"), ("q", "i1", 32)]))
        return b["q"].reshape(-1), b["d"].view(np.float16).astype(np.float32), b["q"].astype(np.int32).sum(axis=1).astype(np.uint32)
    b = np.frombuffer(oracle.quantize(oracle.TYPE_Q8_1, row, row.size).tobytes(), dtype=np.dtype([("d", "<f4"), ("s", "<f4"), ("q", "i1", 32)]))
    assert b.size == nb
    return b["q"].reshape(-1), b["d"].copy(), b["s"].copy().view(np.uint32)


def check(pkg, oracle, c):
    what = "%s [route %s, N %d, P %d, t_max %d]" % (c.name, A.ROUTE_NAMES[c.route], c.N, c.P, c.t_max)
    rc, out, oq, od, os_, launched = launch(pkg, c)
    assert rc == 0, (what, pkg._err())
    assert tuple(launched[:4]) == c.expected_launch() and launched[5] == c.t_cap, (what, "launched", list(launched), "expected", c.expected_launch(), c.t_cap)
    ref = A.oracle_rows(c)
    got, N = out[:c.N], c.N
    bad = np.argwhere(got.view(np.uint32) != ref.view(np.uint32))
    if bad.size:
        import attn_ref
        rr = A.ref_rows(c)
        msgs = []
        for i, j in bad:
            h, d = int(j) // c.dk, int(j) % c.dk
            r = rr[i][h]
            if r["fragile"][d] and abs(float(got[i, j]) - float(ref[i, j])) <= float(np.spacing(np.abs(ref[i, j]))):
                continue        # the association decides this float32: one ulp is owed, no more
            msgs.append("route %s column %d head %d dim %d: kernel %r oracle %r (T %d, fragile %s)" % (A.ROUTE_NAMES[c.route], i, h, d, float(got[i, j]), float(ref[i, j]),
                                                                                                      int(c.T[i]), bool(r["fragile"][d])))
        assert not msgs, (what, len(msgs), msgs[:6])
    assert (out[N:].view(np.uint8) == 0xff).all(), (what, "a store beyond column N", np.argwhere(out[N:].view(np.uint32) != 0xffffffff)[:4])
    if not c.q8:
        return
    for i in range(N):
        q_ref, d_ref, s_ref = oracle_q8(oracle, ref[i], c.q8)
        assert (oq[i] == q_ref).all(), (what, "Q8 codes", i, np.flatnonzero(oq[i] != q_ref)[:6], oq[i][oq[i] != q_ref][:6], q_ref[oq[i] != q_ref][:6])
        assert (od[i].view(np.uint32) == d_ref.view(np.uint32)).all(), (what, "Q8 d", i, od[i], d_ref)
        assert (os_[i] == s_ref).all(), (what, "Q8 s", i, os_[i], s_ref)
    for name, x in (("codes", oq), ("d", od), ("s", os_)):
        assert (x[N:].view(np.uint8) == 0xff).all(), (what, "a Q8 store beyond column N", name)


@pytest.mark.parametrize("group", sorted(A.groups()))
def test_kernel_equals_the_oracle(pkg, oracle, group):
    for c in A.groups()[group]:
        check(pkg, oracle, c)


def test_every_route_runs_at_every_border_of_its_classes():
    """The case list itself: each route at each key count of T_BORDERS the engine gives it, the split trio and the generic kernel at theirs."""
    by_route = {}
    for c in A.all_cases():
        by_route.setdefault(c.route, set()).add((c.t_max, c.P, c.dk))
    have = lambda r, P: {t for t, p, dk in by_route[r] if p == P}
    for shared in (0, A.SHARED):
        assert have(A.FAST_1 + shared, 1024) >= {1, 2, 63, 64, 65, 255, 256} and have(A.FAST_2 + shared, 1024) >= {257, 511, 512}
        assert have(A.FAST_4 + shared, 1024) >= {513, 640, 641, 1023, 1024} and have(A.FAST_SLIM + shared, 1024) >= set(A.T_BORDERS)
        assert have(A.FAST_4 + shared, 600) >= {577, 600} and have(A.FAST_1 + shared, 100) >= {65, 100}
    assert have(A.PREFIX, 1024) >= set(A.T_BORDERS) and have(A.GROUP, 1026) >= set(A.T_BORDERS)
    assert have(A.SPLIT, 1024) >= {257, 511, 512, 513, 640, 641, 1023, 1024} and have(A.SPLIT, 600) >= {513, 577, 600}
    assert have(A.TILE_DMA, 1024) >= {1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 640} and have(A.TILE, 1024) >= {641, 1023, 1024}
    assert {p for _, p, _ in by_route[A.GROUP]} >= {102, 7, 3} and {p for _, p, _ in by_route[A.TILE_DMA]} >= {4, 100, 600, 1024}
    for dk in (16, 32, 64, 128):
        ts = {t for t, p, k in by_route[A.GENERIC] if k == dk}
        assert ts >= {1025, 2047, 2048} and (dk == 64 or ts >= set(A.T_BORDERS)), dk
    assert max(t for t, p, k in by_route[A.GENERIC]) == A.ATTN_MAXK * 1024
    assert set(by_route) == set(A.ROUTE_NAMES)


def test_probe_refuses_what_the_engine_never_launches(pkg):
    """Every refusal is made before anything is allocated or read, so the arrays of the valid case serve."""
    q, K, V = A.content("plain", 100)
    tile = A.dev_case("tile", A.TILE_DMA, 4, 100, q, K, V, (96, 0, 0))
    group = A.dev_case("group", A.GROUP, 4, 102, q, K, V, (96, 0, 0))
    q3, K3, V3 = A.content("plain", 300)
    split = A.dev_case("split", A.SPLIT, 1, 1024, q3, K3, V3, (299, 0, 0))
    fast = A.seq_case("fast", A.FAST_2, 2, 1024, q3, K3, V3, 300)
    shared = A.seq_case("shared", A.FAST_SLIM + A.SHARED, 2, 1024, q3, K3, V3, 300, n_shared=[5, 7])
    prefix = A.seq_case("prefix", A.PREFIX, 2, 1024, q3, K3, V3, 300, n_shared=[5, 5])
    q32, K32, V32 = A.content("plain", 1100, dk=32)
    generic = A.dev_case("generic", A.GENERIC, 1, 2048, q32, K32, V32, (1099, 0, 0), dk=32)
    for c in (tile, group, split, fast, shared, prefix, generic):
        assert launch(pkg, c)[0] == 0, (c.name, pkg._err())

    def refused(c, field, **over):
        kv = c.slots()
        rc, out = launch(pkg, c, kv=kv, **over)[:2]
        assert rc == -1 and field in pkg._err(), (c.name, over, rc, pkg._err())
        assert (out == 0).all()

    state = lambda n_past, causal=0, chunk=0: np.array([n_past, 0, causal, chunk], dtype=np.int32)
    seq = lambda c, **kw: _edit(c.states()[1], **kw)
    refused(tile, "grouped kernel", P=102)                                   # tile with P no multiple of 4
    refused(tile, "grouped kernel", P=3, t_max=3, N=1, dev=state(2))
    refused(group, "tile kernel", P=104)                                     # the grouped kernel where the engine takes the tile kernel
    refused(tile, "form of the tile kernel", route=A.TILE)                   # up to 640 keys the DMA form
    refused(prefix, "P must be", P=1028)                                     # prefix beyond PFX_MAX_KEYS
    refused(prefix, "one shared range", st=seq(prefix, row=1, n_shared=4))
    refused(prefix, "col_mode 0", col_mode=1)
    refused(split, "N = 1", N=2, dev=state(298))                             # split with N != 1
    refused(split, "above 256 keys", t_max=200, dev=state(199))
    refused(split, "1024", P=2048, t_max=1100, dev=state(1099))              # more than SPLIT_MAX ranges: beyond 1024 keys no kernel but the generic one
    refused(fast, "outside the reach", route=A.FAST_1)                       # fast with t_cap over the instantiation's reach
    refused(fast, "outside the reach", route=A.FAST_4)
    refused(fast, "outside the reach", route=A.FAST_2, t_max=513, st=seq(fast, n_past=512))
    refused(fast, "1024", P=2048, t_max=1025, st=seq(fast, n_past=1024))
    refused(fast, "seq_states", route=A.FAST_SLIM, st=None, dev=state(298))  # the slim and the SHARED launches are decode steps
    refused(shared, "seq_states", st=None, dev=state(298))
    refused(generic, "not supported", dk=48)                                 # attn_threads % dk != 0
    refused(generic, "not supported", P=8192, t_max=4097, dev=state(4096))   # T > ATTN_MAXK * threads
    refused(generic, "never takes the generic kernel", dk=64, t_max=1024, dev=state(1023))
    refused(generic, "no Q8", q8=1)
    refused(tile, "visible keys", dev=state(97))                             # T outside [1, t_cap]
    refused(tile, "negative", dev=state(-4))
    refused(tile, "negative", dev=state(-1, causal=1))
    refused(fast, "n_past", st=seq(fast, n_past=320))
    refused(fast, "n_past", st=seq(fast, n_past=-1))
    refused(fast, "visible keys", col_mode=1, st=seq(fast, t_vis=0))
    refused(fast, "visible keys", col_mode=1, st=seq(fast, t_vis=301))
    refused(tile, "t_max must be", t_max=101)                                # t_cap > P
    refused(fast, "t_max must be", t_max=1025)
    refused(fast, "slot", col_mode=1, st=seq(fast, t_vis=300, seq_id=2))     # a slot outside the arrays
    refused(shared, "shared slot", st=seq(shared, row=1, slot=3))
    refused(shared, "shared rows", st=seq(shared, row=0, n_shared=300))
    refused(tile, "exactly one", st=fast.states()[1])
    refused(tile, "exactly one", dev=None)
    refused(tile, "one slot", n_slots=2)
    refused(tile, "route", route=14)
    refused(tile, "dk must be 64", dk=32)
    refused(tile, "q8", q8=3)


def _edit(st, row=None, n_past=None, t_vis=None, seq_id=None, n_shared=None, slot=None):
    st = st.copy()
    rows = slice(None) if row is None else row
    for col, val in ((0, n_past), (4, t_vis), (3, seq_id), (5, n_shared), (6, slot)):
        if val is not None:
            st[rows, col] = val
    return st
