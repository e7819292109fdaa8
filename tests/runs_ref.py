"""attn_runs_kernel<8> on the CPU side of its tests: a Python restatement of its planner (attn_runs_plan in engine.hip), the invariants a run table owes, and the
cases of tests/test_gpu_runs_attn.py -- packed passes (col_mode 1) of prefix columns and continuation columns with the slot layout of
biogpt_hip_score_continuations_batch.  A case is the logical content (per column and head the visible key / value rows, in order) and a layout (which slot
holds which rows); every row of every slot that no column may see holds attn_cases.SENTINEL.  tests/test_runs_restatement.py examines the cases on the CPU
(no committed case has a fragile row, so the GPU test owes bit equality with the oracle everywhere)."""
import numpy as np

import attn_cases as A

H, DK, MAX_RUN = A.H, 64, 8
OWN = [0, 1, 7, 8, 15, 16, 17, 40]
FAMILIES = ["tie64", "peak_shared", "peak_last", "ranges", "v_alt", "v_zero"]


# ---- the planner, restated ------------------------------------------------------------------------------------------------------------------
def plan(st):
    """st int32 [N][8] packed column states (3: seq_id, 4: t_vis, 5: pad[0], 6: pad[1]) -> [(c0, n, R, S)], greedily: a run is cut at 8 columns or at the first
    column that does not fit.  Columns without shared rows of one seq_id form prefix runs (S = seq_id, R = the smallest t_vis); columns with equal
    (pad[0], pad[1]), pad[0] > 0, continuation runs (S = pad[1], R = pad[0]); a column that sees fewer rows than pad[0] stands alone with R = t_vis."""
    st = np.asarray(st).reshape(-1, 8)
    runs, i, N = [], 0, len(st)
    while i < N:
        sid, tv, p0, p1 = (int(x) for x in st[i, 3:7])
        pre = p0 <= 0
        n, R = 1, tv if pre else min(p0, tv)
        if pre or tv >= p0:
            while n < MAX_RUN and i + n < N:
                s2, t2, q0, q1 = (int(x) for x in st[i + n, 3:7])
                if pre and not (q0 <= 0 and s2 == sid):
                    break
                if not pre and not (q0 == p0 and q1 == p1 and t2 >= q0):
                    break
                if pre:
                    R = min(R, t2)
                n += 1
        runs.append((i, n, R, sid if pre else p1))
        i += n
    return runs


def row_slot(st, i, j):
    """The slot that holds visible row j of column i."""
    return int(st[i, 6]) if j < int(st[i, 5]) else int(st[i, 3])


def check_invariants(st, runs):
    """A partition of the columns into runs of consecutive columns in order, n in [1, 8]; for every member the rows [0, R) lie in S and are visible, and
    the rows [R, T) lie in its own slot."""
    st = np.asarray(st).reshape(-1, 8)
    nxt = 0
    for c0, n, R, S in runs:
        assert c0 == nxt and 1 <= n <= MAX_RUN, (c0, n, nxt)
        for i in range(c0, c0 + n):
            T = int(st[i, 4])
            assert 0 <= R <= T, (i, R, T)
            assert all(row_slot(st, i, j) == S for j in range(R)), (i, R, S)
            assert all(row_slot(st, i, j) == int(st[i, 3]) for j in range(R, T)), (i, R)
        nxt = c0 + n
    assert nxt == len(st)


def column_states(groups):
    """groups: [("pre", t0, n)] n consecutive tokens of one prompt seeing t0 .. t0 + n - 1 rows, or ("cont", R, [own...]) candidates behind R shared rows, each
    with `own` rows of its own.  Slots are numbered as the engine numbers them: prefix slots first (one per group, in order), then one per continuation.
    Returns (st int32 [N][8], n_slots)."""
    n_groups = len(groups)
    rows, cont = [], 0
    for g, grp in enumerate(groups):
        if grp[0] == "pre":
            for k in range(grp[2]):
                rows.append([grp[1] + k - 1, 0, 0, g, grp[1] + k, 0, 0, 0])
        else:
            for own in grp[2]:
                rows.append([grp[1] + own - 1, 0, 0, n_groups + cont, grp[1] + own, grp[1], g, 0])
                cont += 1
    return np.asarray(rows, dtype=np.int32).reshape(-1, 8), n_groups + cont


# ---- kernel cases -----------------------------------------------------------------------------------------------------------------------------
class RunCase:
    """A packed pass for the probe.  Column i of a group sees the first T_i rows of the group's content table; in a "plain" case the own rows of a continuation
    are rows of its own instead (reading the wrong slot, or a row on the wrong side of R, gives another result)."""

    def __init__(self, name, P, groups, family="plain", seed=0, q8=0):
        self.name, self.P, self.groups, self.family, self.q8 = name, P, groups, family, q8
        self.st, self.n_slots = column_states(groups)
        self.N, self.dk = len(self.st), DK
        self.T = self.st[:, 4].copy()
        self.t_max = int(self.T.max())
        assert 1 <= self.T.min() and self.t_max <= P <= 1024
        rng = np.random.default_rng([seed, self.N, P])
        self.q = np.zeros((self.N, H * DK), dtype=np.float32)
        self.tables = []                                            # per column (K, V) [H][T_i][dk]
        self.k = np.full((self.n_slots, H, P, DK), A.SENTINEL, dtype=np.float32)
        self.v = np.full((self.n_slots, H, P, DK), A.SENTINEL, dtype=np.float32)
        col = 0
        for g, grp in enumerate(groups):
            Ts = [grp[1] + k for k in range(grp[2])] if grp[0] == "pre" else [grp[1] + own for own in grp[2]]
            tg = max(Ts)
            if family == "plain":
                qt = rng.standard_normal((17, H * DK)).astype(np.float32) * np.float32(0.125)
                K, V = rng.standard_normal((2, H, tg, DK)).astype(np.float32)
            else:
                qt, K, V = A.content(family, tg, seed=seed + g)
            shared = tg if grp[0] == "pre" else grp[1]
            self.k[g, :, :shared], self.v[g, :, :shared] = K[:, :shared], V[:, :shared]
            for n, T in enumerate(Ts):
                self.q[col] = qt[n % 17]
                Kc, Vc = K[:, :T].copy(), V[:, :T].copy()
                if grp[0] == "cont":
                    if family == "plain":
                        Kc[:, shared:], Vc[:, shared:] = rng.standard_normal((2, H, T - shared, DK)).astype(np.float32)
                    s = int(self.st[col, 3])
                    self.k[s, :, shared:T], self.v[s, :, shared:T] = Kc[:, shared:], Vc[:, shared:]
                self.tables.append((Kc, Vc))
                col += 1
        assert col == self.N

    def gather(self, i, h):
        return self.tables[i][0][h], self.tables[i][1][h]

    def slots(self):
        return self.k, self.v


def _own(n, room, at=0):
    """n own-row counts cycling through OWN from `at`, those that fit the table."""
    fit = [o for o in OWN if o <= room]
    return [fit[(at + k) % len(fit)] for k in range(n)]


_cases = None


def kernel_cases():
    """The cases of tests/test_gpu_runs_attn.py: H = 3, dk = 64, P in {100, 1024}; N in {1, 7, 8, 9, 17, 33}; R in {1, 2, 63, 64, 65, 127, 128, 129, 1016,
    1023}; own rows in OWN, inside P; prefix runs, continuation runs, mixed passes; the content families that stress the sums and the masks."""
    global _cases
    if _cases is not None:
        return _cases
    cs = []
    q8 = lambda: len(cs) % 3
    for N in (1, 7, 8, 9, 17, 33):                                  # P = 100: column counts around the run size, both kinds
        cs.append(RunCase("pre N %d from 1" % N, 100, [("pre", 1, N)], seed=1, q8=q8()))
        cs.append(RunCase("pre N %d from 63" % N, 100, [("pre", 63, N)], seed=2, q8=q8()))
        for R in ((1, 63) if N not in (9, 17) else (1, 2, 63, 64, 65)):
            cs.append(RunCase("cont N %d R %d" % (N, R), 100, [("cont", R, _own(N, 100 - R, N))], seed=3, q8=q8()))
    for R in (63, 64, 65, 127, 128, 129, 1016, 1023):               # P = 1024: every R, a run of 8 and a lone column
        cs.append(RunCase("cont P 1024 R %d" % R, 1024, [("cont", R, _own(9, 1024 - R, R))], seed=4, q8=q8()))
    for t0 in (57, 121, 125, 1009, 1017):                           # prefix runs across the 64 / 128 borders of the sweeps and up to the table's end
        cs.append(RunCase("pre P 1024 from %d" % t0, 1024, [("pre", t0, 8)], seed=5, q8=q8()))
    # mixed passes: the end of one prompt, a whole short prompt, two groups adjacent (9 candidates, then 3), a group without shared rows (n_prefix = 1)
    cs.append(RunCase("mixed P 100", 100, [("pre", 30, 11), ("pre", 1, 4), ("cont", 41, _own(9, 50)), ("cont", 5, [1, 2, 40]), ("cont", 0, [1, 3])], seed=6, q8=1))
    cs.append(RunCase("mixed P 1024", 1024, [("pre", 250, 9), ("pre", 1, 1), ("cont", 259, [1, 40, 7]), ("cont", 2, [1] * 9), ("cont", 0, [2])], seed=7, q8=2))
    for fam in FAMILIES:
        for P, R in ((100, 58), (1024, 217)):
            cs.append(RunCase("family %s P %d" % (fam, P), P, [("pre", R + 33, 8), ("cont", R, [1, 40, 8, 17, 40, 0, 16, 7, 15])], family=fam, seed=8, q8=q8()))
    _cases = cs
    return cs


def oracle_rows(case):
    return A.oracle_rows(case)


def ref_rows(case):
    return A.ref_rows(case)
