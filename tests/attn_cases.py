"""The cases of tests/test_gpu_attn_kernels.py (every stand-alone attention kernel against the oracle's bo_attn_head) and of tests/test_attn_restatement.py
(the same cases on the CPU: what the oracle and the restatement say about them).  A case is the LOGICAL content -- per column and head the visible key / value
rows, in order -- and a layout: the route (kernel), the table size P, the column states and which cache slot holds which rows.  Every row of every slot that no
column may see holds SENTINEL.  Cases are seeded; the content of a (family, T) is the same for every route, so the oracle's rows are computed once (memo by
content)."""
import hashlib

import numpy as np

H = 3                                   # D = 192: six Q8 blocks per row, not a power of two
SENTINEL = np.float32(3.0e30)           # large and finite: a NaN would be ignored by fmaxf and hide a missing mask
FAST_1, FAST_2, FAST_4, FAST_SLIM, SHARED, PREFIX, SPLIT, GROUP, TILE_DMA, TILE, GENERIC = 0, 1, 2, 3, 4, 8, 9, 10, 11, 12, 13
ROUTE_NAMES = {0: "fast<1,true>", 1: "fast<2,false>", 2: "fast<4,false>@1024", 3: "fast<4,false> slim", 4: "fast<1,true,SHARED>", 5: "fast<2,false,SHARED>",
               6: "fast<4,false,SHARED>@1024", 7: "fast<4,false,SHARED> slim", 8: "prefix<8>", 9: "split trio", 10: "group<8>", 11: "tile<16,true>",
               12: "tile<16,false>", 13: "generic"}
T_BORDERS = [1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 640, 641, 1023, 1024]
ATTN_MAXK, SPLIT_KEYS, SPLIT_ABOVE = 4, 64, 256


def visible_keys(dev, i, N):
    """kernels.hip.h visible_keys: dev = (n_past, causal, chunk)."""
    n_past, causal, chunk = dev
    if causal:
        return n_past + i + 1
    if chunk <= 0:
        return n_past + N
    return n_past + min((i // chunk + 1) * chunk, N)


def decode_t_cap(P, t_max):
    return min(P, (t_max + 63) // 64 * 64)


def fast_route(P, t_max, slim=False, shared=False):
    """The attn_fast_kernel instantiation a decode pass of t_max keys takes in a table of P rows."""
    t_cap = decode_t_cap(P, t_max)
    return (FAST_SLIM if slim else FAST_1 if t_cap <= 256 else FAST_2 if t_cap <= 512 else FAST_4) + (SHARED if shared else 0)


def tile_route(P, t_max):
    return TILE_DMA if min(P, t_max) * 64 + 3 * 8 * 1024 <= 8 * 16 * 64 * 8 else TILE      # attn_tile_dma_ok: up to 640 keys


def generic_threads(t_max):
    nt = 256
    while nt < 1024 and t_max > nt:
        nt *= 2
    return nt


class Case:
    """mode "dev": the context's own columns -- one table, dev = (n_past, causal, chunk), column i sees its first visible_keys rows.
    mode "seq": one slot per column -- tables[i] = (K_i, V_i) [H][T_i][dk]; col_mode 1: column i's slot is perm[i] and T_i travels as t_vis; n_shared[i] > 0
    (SHARED routes, prefix): the column's first n_shared[i] rows lie in the extra last slot (they are the same rows for every column that has them)."""

    def __init__(self, name, route, N, P, q, tables, mode, dev=None, T=None, col_mode=0, perm=None, n_shared=None, dk=64, q8=0, family=None):
        self.name, self.route, self.N, self.P, self.dk, self.q8, self.family = name, route, N, P, dk, q8, family
        self.q = np.ascontiguousarray(q[:N], dtype=np.float32)
        assert self.q.shape == (N, H * dk)
        self.mode, self.dev, self.col_mode = mode, dev, col_mode
        if mode == "dev":
            self.T = np.array([visible_keys(dev, i, N) for i in range(N)])
            self.tables = tables
            assert tables[0].shape[1] >= self.T.max() and tables[0].shape == tables[1].shape
            self.n_slots = 1
        else:
            self.T = np.asarray(T)
            self.tables = tables
            self.perm = np.arange(N) if perm is None else np.asarray(perm)
            assert col_mode == 1 or perm is None
            self.n_shared = None if n_shared is None else np.asarray(n_shared)
            self.n_slots = N + (1 if n_shared is not None else 0)
            for i in range(N):
                assert tables[i][0].shape == (H, self.T[i], dk) == tables[i][1].shape
        self.t_max = int(self.T.max())
        assert 1 <= self.T.min() and self.t_max <= P
        pass_kernel = route in (GROUP, TILE, TILE_DMA)
        self.t_cap = P if route == GENERIC else min(P, self.t_max) if pass_kernel else decode_t_cap(P, self.t_max)

    def gather(self, i, h):
        """Column i's visible K and V rows of head h, contiguous [T_i][dk]."""
        T = int(self.T[i])
        if self.mode == "dev":
            return self.tables[0][h, :T], self.tables[1][h, :T]
        return self.tables[i][0][h], self.tables[i][1][h]

    def slots(self):
        """k_slots, v_slots [n_slots][H][P][dk] with SENTINEL in every row no column may see."""
        k = np.full((self.n_slots, H, self.P, self.dk), SENTINEL, dtype=np.float32)
        v = np.full((self.n_slots, H, self.P, self.dk), SENTINEL, dtype=np.float32)
        if self.mode == "dev":
            k[0, :, :self.t_max] = self.tables[0][:, :self.t_max]
            v[0, :, :self.t_max] = self.tables[1][:, :self.t_max]
            return k, v
        for i in range(self.N):
            ns = 0 if self.n_shared is None else int(self.n_shared[i])
            for a, t in ((k, self.tables[i][0]), (v, self.tables[i][1])):
                a[self.perm[i], :, ns:self.T[i]] = t[:, ns:]
                if ns:
                    assert ((a[self.N, :, :ns] == SENTINEL) | (a[self.N, :, :ns] == t[:, :ns])).all(), "the shared rows are the same for every column"
                    a[self.N, :, :ns] = t[:, :ns]
        return k, v

    def states(self):
        """(dev_state int32 [4] or None, seq_states int32 [N][8] or None)"""
        if self.mode == "dev":
            return np.array([self.dev[0], 0, self.dev[1], self.dev[2]], dtype=np.int32), None
        st = np.zeros((self.N, 8), dtype=np.int32)
        st[:, 0] = self.T - 1                       # n_past: the column's own token is its last key
        st[:, 3] = self.perm if self.col_mode else np.arange(self.N)
        if self.col_mode:
            st[:, 4] = self.T                       # t_vis
            st[:, 0] = self.T + 5                   # a position that is NOT t_vis - 1: packed columns take their keys from t_vis alone
        if self.n_shared is not None:
            st[:, 5] = self.n_shared
            st[:, 6] = self.N
        return None, st

    def expected_launch(self):
        """(kernel, threads, grid x, grid y) as the engine launches this route."""
        r, N, t64 = self.route, self.N, (self.t_cap + 63) // 64 * 64
        if r < PREFIX:
            return (r, max(256, t64) if r & 3 == FAST_SLIM else 4 * t64 if r & 3 == FAST_1 else 1024, H, N)
        if r in (PREFIX, GROUP):
            return (r, 512, H, (N + 7) // 8)
        if r == SPLIT:
            return (r, 256, H, (self.t_cap + SPLIT_KEYS - 1) // SPLIT_KEYS)
        if r in (TILE, TILE_DMA):
            return (r, 512, H, (N + 15) // 16)
        return (r, generic_threads(self.t_max), H, N)


# ---- the oracle's rows, once per content --------------------------------------------------------------------------------------------------
_memo = {}


def _key(tag, q, K, V):
    hsh = hashlib.blake2b(digest_size=16)
    for a in (q, K, V):
        hsh.update(np.ascontiguousarray(a).tobytes())
    return (tag, hsh.digest())


def oracle_rows(case):
    """float32 [N][H * dk]: bo_attn_head of every (column, head) of the case.  Shared among the tests that need it; never modified."""
    from oracle import oracle as O
    out = np.zeros((case.N, H * case.dk), dtype=np.float32)
    for i in range(case.N):
        for h in range(H):
            K, V = case.gather(i, h)
            qv = case.q[i, h * case.dk:(h + 1) * case.dk]
            key = _key("oracle", qv, K, V)
            if key not in _memo:
                _memo[key] = O.attn_head(qv, np.ascontiguousarray(K), np.ascontiguousarray(V), int(case.T[i]))
            out[i, h * case.dk:(h + 1) * case.dk] = _memo[key]
    out.setflags(write=False)
    return out


def ref_rows(case):
    """attn_ref.head of every (column, head): a list [N][H] of its dicts (memo by content)."""
    import attn_ref
    rows = []
    for i in range(case.N):
        rows.append([])
        for h in range(H):
            K, V = case.gather(i, h)
            qv = case.q[i, h * case.dk:(h + 1) * case.dk]
            key = _key("ref", qv, K, V)
            if key not in _memo:
                _memo[key] = attn_ref.head(qv, K, V, int(case.T[i]))
            rows[-1].append(_memo[key])
    return rows


# ---- content ----------------------------------------------------------------------------------------------------------------------------
def _toward(q, targets):
    """Key rows [H][T][dk] whose score with q [H][dk] is (about) targets [T]: multiples of q."""
    q64 = q.astype(np.float64)
    return (q64[:, None, :] * (np.asarray(targets, dtype=np.float64)[None, :, None] / (q64 ** 2).sum(axis=-1)[:, None, None])).astype(np.float32)


FAMILIES = ["plain", "equal", "tie2", "tie64", "peak_last", "peak_first", "peak_shared", "ranges", "small_quarter", "wide", "v_alt", "v_mixed", "v_zero"]
SUBNORMAL_X = (-17.3, -9.7)            # s - max with a subnormal fp16 table value
ZERO_X, INF_X = -17.4, -65504.0        # below: the table gives zero; below: the fp16 argument is -inf


def content(family, T, dk=64, seed=0):
    """(q [17][H * dk], K, V [H][T][dk]) of a family at T keys.  Column 1's query is column 0's halved (a power of two: ties stay ties), the others are random."""
    rng = np.random.default_rng([FAMILIES.index(family), T, dk, seed])
    q = rng.standard_normal((17, H, dk)).astype(np.float32) * np.float32(0.125)      # as the engine's q rows: already scaled (scores of N(0,1) keys: sigma about 1)
    q[1] = q[0] * np.float32(0.5)
    K = rng.standard_normal((H, T, dk)).astype(np.float32)
    V = rng.standard_normal((H, T, dk)).astype(np.float32)
    if family in ("equal", "v_alt"):                 # all keys equal: the sum is exactly T
        K[:] = K[:, :1]
    elif family == "tie2":                           # two keys tied at the maximum, in different waves
        K[:, [1, T - 2]] = _toward(q[0], [8.0])
    elif family == "tie64":                          # 64 keys tied at the maximum, spread over the context
        K[:, np.unique(np.linspace(0, T - 1, 64).astype(int))] = _toward(q[0], [8.0])
    elif family in ("peak_last", "peak_first", "peak_shared"):      # one key 30 above the rest
        K = _toward(q[0], rng.uniform(-1.0, 1.0, T))
        at = {"peak_last": T - 1, "peak_first": 0, "peak_shared": T // 4}[family]
        K[:, at] = _toward(q[0], [30.0])[:, 0]
    elif family == "ranges":                         # s - max in the table's subnormal, zero and -inf ranges, and ordinary keys
        groups = [np.linspace(-17.2, -9.8, 9), [-17.6, -18.0, -30.0, -100.0, -1000.0], [-65600.0, -70000.0, -1.0e5], [-0.5, -1.0, -2.0, -4.0, -8.0]]
        pool = np.concatenate([np.asarray(g, dtype=np.float64) for g in groups])
        x = pool[rng.permutation(T) % len(pool)] if T > len(pool) else pool[:T].copy()
        x[T // 2] = 0.0
        K = _toward(q[0], 5.0 + x)
    elif family == "small_quarter":                  # T - 1 keys at -8 below one key: at 1024 keys the small terms carry a quarter of the sum
        x = np.full(T, -8.0)
        x[T // 3] = 0.0
        K = _toward(q[0], 3.0 + x)
    elif family == "wide":                           # q scaled by 8: a wide random range
        q *= np.float32(8.0)
    if family == "v_alt":                            # rows alternating +-1e4 + N(0,1) under uniform probabilities: an f32 accumulator fails, the double one does not
        V += (np.float32(1e4) * (1 - 2 * (np.arange(T) % 2))).astype(np.float32)[None, :, None]
    elif family == "v_mixed":                        # magnitudes 1e3 and 1e-3 mixed by row
        V *= np.where(rng.integers(0, 2, T) == 1, np.float32(1e3), np.float32(1e-3)).astype(np.float32)[None, :, None]
    elif family == "v_zero":
        V[:] = 0.0
    return q.reshape(17, H * dk), K, V


def q8_content():
    """T = 1: the output is the V row itself, so the test chooses the row the Q8 stage sees.  Six blocks of 32 (H = 3): halves that roundf takes away from
    zero under amax = 127; zeros (d = 0, codes 0); one 1e6 among 1e-3s; amax at a negative element; two random blocks."""
    rng = np.random.default_rng(88)
    row = rng.standard_normal(H * 64).astype(np.float32)
    b = np.zeros(32, dtype=np.float32)
    b[:10] = [127.0, 0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 126.5, -126.5, 3.5]
    b[10:] = rng.integers(-120, 120, 22).astype(np.float32) + np.float32(0.5)
    row[0:32] = b
    row[32:64] = 0.0
    row[64:96] = 1e-3
    row[70] = 1e6
    row[96:128] = rng.uniform(-1.0, 1.0, 32).astype(np.float32)
    row[100] = -127.0
    q, K, V = content("plain", 1, seed=5)
    V = np.repeat(row.reshape(H, 1, 64), 1, axis=1).copy()
    return q, K, V


# ---- layouts ------------------------------------------------------------------------------------------------------------------------------
def dev_case(name, route, N, P, q, K, V, dev, **kw):
    return Case(name, route, N, P, q, (K, V), "dev", dev=dev, **kw)


def seq_case(name, route, N, P, q, K, V, T, n_shared=None, col_mode=0, perm=None, **kw):
    """Every column's table is the first T[i] rows of (K, V)."""
    T = np.broadcast_to(np.asarray(T), (N,))
    return Case(name, route, N, P, q, [(K[:, :t], V[:, :t]) for t in T], "seq", T=T, n_shared=n_shared, col_mode=col_mode, perm=perm, **kw)


def distinct_seq_case(name, route, N, P, T, n_shared, seed, col_mode=0, **kw):
    """Columns with tables of their own behind common shared rows: reading the wrong slot, or a row on the wrong side of n_shared, gives another result."""
    rng = np.random.default_rng([seed, N, P])
    T = np.asarray(T)
    S = 0 if n_shared is None else int(np.max(n_shared))
    common = rng.standard_normal((2, H, S, 64)).astype(np.float32)
    tables = []
    for i in range(N):
        own = rng.standard_normal((2, H, int(T[i]), 64)).astype(np.float32)
        ns = 0 if n_shared is None else int(n_shared[i])
        own[:, :, :ns] = common[:, :, :ns]
        tables.append((own[0], own[1]))
    q = rng.standard_normal((N, H * 64)).astype(np.float32) * np.float32(0.125)
    perm = rng.permutation(N) if col_mode else None
    return Case(name, route, N, P, q, tables, "seq", T=T, n_shared=n_shared, col_mode=col_mode, perm=perm, **kw)


def route_layouts(T, P=1024):
    """For T keys seen by every column: (tag, maker(name, q, K, V, **kw)) for each route the engine can give such a pass in a table of P rows (dk = 64)."""
    out = []
    N2 = min(2, T)

    def dev_n(n):       # n columns that all see T keys
        return (T - n, 0, 0)
    out.append(("fast", lambda name, q, K, V, **kw: seq_case(name, fast_route(P, T), 2, P, q, K, V, T, **kw)))
    out.append(("fast_dev", lambda name, q, K, V, **kw: dev_case(name, fast_route(P, T), N2, P, q, K, V, dev_n(N2), **kw)))
    out.append(("fast_shared", lambda name, q, K, V, **kw: seq_case(name, fast_route(P, T, shared=True), 2, P, q, K, V, T, n_shared=[T // 2, T // 2], **kw)))
    out.append(("slim", lambda name, q, K, V, **kw: seq_case(name, fast_route(P, T, slim=True), 2, P, q, K, V, T, **kw)))
    out.append(("slim_shared", lambda name, q, K, V, **kw: seq_case(name, fast_route(P, T, slim=True, shared=True), 2, P, q, K, V, T, n_shared=[T // 2, T // 2], **kw)))
    out.append(("prefix", lambda name, q, K, V, **kw: seq_case(name, PREFIX, 2, P, q, K, V, T, n_shared=[T // 2, T // 2], **kw)))
    if decode_t_cap(P, T) > SPLIT_ABOVE:
        out.append(("split", lambda name, q, K, V, **kw: dev_case(name, SPLIT, 1, P, q, K, V, (T - 1, 0, 0), **kw)))
    if P % 4 == 0:
        out.append(("tile", lambda name, q, K, V, **kw: dev_case(name, tile_route(P, T), N2, P, q, K, V, dev_n(N2), **kw)))
    else:
        out.append(("group", lambda name, q, K, V, **kw: dev_case(name, GROUP, N2, P, q, K, V, dev_n(N2), **kw)))
    return out


def _q8_of(n):
    return 1 + n % 2


def border_cases():
    """Every route at both sides of every class border of its geometry: all columns see T keys."""
    cases = []
    for T in T_BORDERS:
        q, K, V = content("plain", T)
        for P in (1024, 1026):                        # 1026 is no multiple of 4: a pass takes attn_group_kernel
            for tag, make in route_layouts(T, P):
                if P == 1026 and tag != "group":
                    continue
                cases.append(make("border %s T %d P %d" % (tag, T, P), q, K, V, q8=_q8_of(len(cases))))
        # more columns than a group: 9 for the kernels of 8 columns per workgroup, 17 for the tile kernel at the borders of its own classes
        n9, n17 = min(9, T), min(17, T)
        cases.append(seq_case("border prefix9 T %d" % T, PREFIX, 9, 1024, q, K, V, T, n_shared=[T // 2] * 9, q8=_q8_of(T)))
        cases.append(dev_case("border group9 T %d" % T, GROUP, n9, 1026, q, K, V, (T - n9, 0, 0), q8=_q8_of(T + 1)))
        if T in (64, 65, 640, 641, 1024):
            cases.append(dev_case("border tile17 T %d" % T, tile_route(1024, T), n17, 1024, q, K, V, (T - n17, 0, 0), q8=_q8_of(T)))
    for P, Ts in ((600, (513, 577, 600)), (100, (65, 100))):      # t_cap = P, no multiple of 64: the last ranges / waves are cut at the table's end
        for T in Ts:
            q, K, V = content("plain", T, seed=P)
            for tag, make in route_layouts(T, P):
                cases.append(make("border %s T %d P %d" % (tag, T, P), q, K, V, q8=_q8_of(len(cases))))
    return cases


def generic_cases():
    """attn_kernel: every head size at both sides of its thread-count borders, up to ATTN_MAXK keys per thread (1024 threads: beyond 3072 keys)."""
    cases = []
    for dk in (16, 32, 64, 128):
        for P, Ts in ((2048, T_BORDERS + [1025, 2047, 2048]), (4096, [3072, 3073, 4096])):
            for T in Ts:
                if (dk == 64 and T <= 1024) or (P == 4096 and dk not in (16, 64)):
                    continue
                q, K, V = content("plain", T, dk=dk)
                n = min(2, T)
                cases.append(dev_case("generic dk %d T %d P %d" % (dk, T, P), GENERIC, n, P, q, K, V, (T - n, 0, 0), dk=dk))
    q, K, V = content("plain", 1500, dk=32)
    cases.append(dev_case("generic dk 32 causal", GENERIC, 5, 2048, q, K, V, (1495, 1, 0), dk=32))
    cases.append(dev_case("generic dk 32 chunk", GENERIC, 5, 2048, q, K, V, (1495, 0, 2), dk=32))
    return cases


def family_cases():
    """The score and V families at T in {65, 257, 1024} on every route."""
    cases = []
    for T in (65, 257, 1024):
        for fam in FAMILIES[1:]:
            q, K, V = content(fam, T)
            for P in (1024, 1026):
                for tag, make in route_layouts(T, P):
                    if P == 1026 and tag != "group":
                        continue
                    cases.append(make("family %s %s T %d" % (fam, tag, T), q, K, V, q8=_q8_of(len(cases)), family=fam))
            q32, K32, V32 = content(fam, T, dk=32)
            cases.append(dev_case("family %s generic T %d" % (fam, T), GENERIC, 2, 2048, q32, K32, V32, (T - 2, 0, 0), dk=32, family=fam))
    return cases


COLUMN_COUNTS = [1, 7, 8, 9, 15, 16, 17, 33, 81]
DEV_STATES = [("chunk0", lambda N, room: (room, 0, 0)), ("chunk8", lambda N, room: (room, 0, 8)), ("causal", lambda N, room: (room, 1, 0)),
              ("from0", lambda N, room: (0, 0, 8))]


def column_cases():
    """Column structure: tails of the 8- and 16-column groups, 1 / 2 / 3 / 6 tiles, the forms of the context state, packed columns, shared ranges."""
    cases = []
    for N in COLUMN_COUNTS:
        for tag, dev in DEV_STATES:
            for P, route in ((100, None), (102, GROUP), (7, GROUP), (3, GROUP), (4, None)):
                if N > P:
                    continue
                d = dev(N, P - N)
                q, K, V = content("plain", P, seed=1000 + N)
                r = route if route is not None else tile_route(P, max(visible_keys(d, i, N) for i in range(N)))
                cases.append(dev_case("columns %s N %d P %d %s" % (ROUTE_NAMES[r], N, P, tag), r, N, P, np.tile(q, (5, 1)), K, V, d, q8=_q8_of(len(cases))))
        if N <= 17:                                   # a pass of a few columns on the per-column kernel, each with its own visible keys
            q, K, V = content("plain", 100, seed=2000 + N)
            for tag, dev in DEV_STATES[1:3]:
                d = dev(N, 100 - N)
                cases.append(dev_case("columns fast N %d %s" % (N, tag), fast_route(100, 100), N, 100, q, K, V, d, q8=_q8_of(len(cases))))
        # one slot per column, contents of their own, 1 .. 41 own rows mixed within a group
        own = np.array([1 + (i * 3 + N) % 41 for i in range(N)])
        for S in (0, 1, 55):
            T = S + own
            ns = [S] * N
            cases.append(distinct_seq_case("columns prefix N %d shared %d" % (N, S), PREFIX, N, 128, T, ns, 31, q8=_q8_of(len(cases))))
            for slim in (False, True):
                cases.append(distinct_seq_case("columns %s N %d shared %d" % ("slim" if slim else "fast", N, S), fast_route(128, int(T.max()), slim, True), N, 128, T, ns, 32,
                                               q8=_q8_of(len(cases))))
        # packed columns: a permuted seq_id and a t_vis per column; per column pad[0] in {0, 1, T - 1}
        T = np.array([2 + (i * 7 + N) % 90 for i in range(N)])
        mixed = np.array([(0, 1, t - 1)[i % 3] for i, t in enumerate(T)])
        for slim in (False, True):
            cases.append(distinct_seq_case("columns packed %s N %d" % ("slim" if slim else "fast", N), fast_route(100, int(T.max()), slim, False), N, 100, T, None, 33, col_mode=1,
                                           q8=_q8_of(len(cases))))
            cases.append(distinct_seq_case("columns packed shared %s N %d" % ("slim" if slim else "fast", N), fast_route(100, int(T.max()), slim, True), N, 100, T, mixed, 34,
                                           col_mode=1, q8=_q8_of(len(cases))))
    for N, P in ((2, 3), (3, 3), (4, 4), (2, 4)):      # the smallest tables filled by their columns
        q, K, V = content("plain", P, seed=2500 + N)
        for tag, dev in DEV_STATES[:3]:
            cases.append(dev_case("columns tiny N %d P %d %s" % (N, P, tag), tile_route(P, P) if P == 4 else GROUP, N, P, q, K, V, dev(N, P - N), q8=_q8_of(len(cases))))
    # larger tables: P = 1024 with t_cap < P, 6 tiles in both forms of the tile kernel; P = 600 = t_cap
    for name, N, P, d in (("dma", 81, 1024, (500, 0, 8)), ("plain", 33, 1024, (700, 0, 8)), ("plain causal", 81, 1024, (900, 1, 0)), ("P600", 81, 600, (519, 0, 8))):
        q, K, V = content("plain", d[0] + N, seed=3000 + N)
        t_max = max(visible_keys(d, i, N) for i in range(N))
        cases.append(dev_case("columns tile %s N %d P %d" % (name, N, P), tile_route(P, t_max), N, P, np.tile(q, (5, 1)), K, V, d, q8=_q8_of(len(cases))))
    q, K, V = content("plain", 1000, seed=3100)
    cases.append(dev_case("columns group N 33 P 1022", GROUP, 33, 1022, np.tile(q, (2, 1)), K, V, (967, 0, 8), q8=1))
    return cases


def q8_cases():
    """The Q8 stage through T = 1, both forms, on every route that can run one key."""
    q, K, V = q8_content()
    cases = []
    for q8 in (1, 2):
        for P in (1024, 7, 4):
            for tag, make in route_layouts(1, P):
                cases.append(make("q8 form %d %s P %d" % (q8, tag, P), q, K, V, q8=q8, family="q8"))
    return cases


_groups = None


def groups():
    """{group name: [Case]}: one GPU test per group."""
    global _groups
    if _groups is None:
        g = {}
        for kind, cases in (("border", border_cases()), ("generic", generic_cases()), ("family", family_cases()), ("columns", column_cases()), ("q8", q8_cases())):
            for c in cases:
                g.setdefault("%s %s" % (kind, ROUTE_NAMES[c.route]), []).append(c)
        _groups = g
    return _groups


def all_cases():
    return [c for cs in groups().values() for c in cs]
