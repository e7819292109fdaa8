"""Log-probabilities of generated tokens (logprobs=K of generate_greedy_batch / generate_sample; kernels_genlp.hip.h) on the GPU.

Calls, on the 3-layer base-width Q4_0 model of test_gpu_sample.py (prompts of at most 24 tokens, 12 new tokens):
  - the ids (sampling: and the lengths) are those of the call without logprobs, at 1, 3, 9 and 50 sequences -- one column, column-per-XCD launches, the
    launch chain, the matrix-core chain -- greedy and sampled with an EOS id;
  - n_batch = 1: lp and top_lp equal score_batch of prompt ++ ids, as int32 bit patterns (K in 1, 5, 8);
  - n_batch = 8: they equal logprob_rows_kernel over the rows of a host loop of biogpt_hip_eval (chunks of 8, then token by token), and numpy's stable
    order on (-logit, id) gives top_ids;
  - behind a prefix of 20 tokens (n_batch 8: 16 shared rows), copied (3 columns) and in place (9 columns): everything equals the call on the concatenations;
  - entries past a sampled sequence's EOS are 0 / -1, and calls with another K on the same context (the same captured steps and buffers) are right.
The kernels alone (biogpt_hip_genlp_rows_device) on the hostile rows of beam_kernels_ref.py: ids and top ids exact against the (value descending, lower id
first) order, log-probabilities within beam_kernels_ref.lp_tolerance of a float64 log-softmax (every case prints its worst |diff| / tol), and in mode 1
the draw, the ids and the generator states of biogpt_hip_sample_candidates_host and of the plain sample_rows_kernel."""
import ctypes

import numpy as np
import pytest

import beam_kernels_ref as bk

pytestmark = pytest.mark.gpu

KW = dict(n_vocab=42384, n_layer=3, n_head=16, n_positions=1024, d_ff=4096, d_model=1024, n_merges=40000)
N_PREDICT = 12
HOT = dict(top_k=40, top_p=0.95, temp=6.0)
SEED0 = 500
PREFIX_LEN = 20


def prompt_of(n, seed):
    rng = np.random.default_rng(seed)
    return [2] + [int(v) for v in rng.integers(4, KW["n_vocab"], n - 1)]


def prompts_for(n):
    return [prompt_of(5 + (7 * i) % 20, 1000 + i) for i in range(n)]      # 5 .. 24 tokens


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@pytest.fixture(scope="module")
def model(pkg, tmp_path_factory):
    d = tmp_path_factory.mktemp("genlp")
    f32, q40 = str(d / "f32.bin"), str(d / "q4_0.bin")
    pkg.write_synthetic(f32, **KW)
    pkg.quantize_file(f32, q40, "q4_0")
    g = pkg.BiogptModel.load(q40)
    yield g
    g.close()


class Runs:
    """The calls of this module on one context, each made once: (mode, sequences, n_batch, K or None, prefix?) -> (ids, info or None, prompts)."""

    def __init__(self, g):
        self.g, self.cache, self.eos = g, {}, {}

    def layout(self, n, mode="sample"):
        """(prompts, samples per prompt): 50 sampled sequences are 25 prompts x 2 samples (the prompt's K / V rows shared between slots)."""
        return (prompts_for(25), 2) if n == 50 and mode == "sample" else (prompts_for(n), 1)

    def eos_for(self, n, nb):
        """An id the free run of this shape draws at a place >= 2 of some sequence and not before it there: with it as EOS that sequence ends early."""
        if (n, nb) not in self.eos:
            prompts, ns = self.layout(n)
            free, _ = self.g.generate_sample(prompts, N_PREDICT, n_samples=ns, seed=SEED0, eos_id=-1, n_batch=nb, **HOT)
            pick = [(t, int(s[t])) for s in free for t in range(2, N_PREDICT - 2) if int(s[t]) not in [int(v) for v in s[:t]]]
            assert pick, "fixture problem: no sequence of the free run offers an EOS id"
            self.eos[(n, nb)] = min(pick)[1]
        return self.eos[(n, nb)]

    def get(self, mode, n, nb, K, prefix=False):
        key = (mode, n, nb, K, prefix)
        if key in self.cache:
            return self.cache[key]
        prompts, ns = self.layout(n, mode)
        kw = dict(n_batch=nb)
        if K is not None:
            kw["logprobs"] = K
        given = prompts
        if prefix:
            assert ns == 1
            pre = prompt_of(PREFIX_LEN, 77)
            kw["prefix"] = pre
            prompts = [pre + p[1:] for p in prompts]      # the sequences as the model sees them
            given = [p[PREFIX_LEN:] for p in prompts]
        if mode == "greedy":
            out = self.g.generate_greedy_batch(given, N_PREDICT, **kw)
        else:
            out = self.g.generate_sample(given, N_PREDICT, n_samples=ns, seed=SEED0, eos_id=self.eos_for(n, nb), **HOT, **kw)
        ids, info = ([list(map(int, s)) for s in out[0]], out[1] if K is not None else None)
        assert len(out) == (3 if K is not None else 2)
        self.cache[key] = (ids, info, [prompts[r // ns] for r in range(len(ids))])
        return self.cache[key]


@pytest.fixture(scope="module")
def runs(model):
    return Runs(model)


# ---- 1. the ids are the plain call's ----

@pytest.mark.parametrize("n", [1, 3, 9, 50])
@pytest.mark.parametrize("mode", ["greedy", "sample"])
def test_ids_are_those_of_the_plain_call(runs, mode, n):
    want, _, _ = runs.get(mode, n, 1, None)
    for K in (5, 0):
        got, info, _ = runs.get(mode, n, 1, K)
        assert got == want, (mode, n, K)      # (lists of different lengths differ: the lengths are compared too)
        assert len(info) == len(got) == n
        for r in range(n):
            lp, ti, tl = info[r]
            assert lp.dtype == np.float32 and ti.dtype == np.int32 and tl.dtype == np.float32
            assert lp.shape == (len(got[r]),) and ti.shape == tl.shape == (len(got[r]), K), (mode, n, K, r)
            assert np.isfinite(lp).all() and (lp <= 0).all() and np.isfinite(tl).all()
            if K:
                assert (tl[:, 0] >= lp).all() and (np.diff(tl, axis=1) <= 0).all()
                if mode == "greedy":
                    assert ti[:, 0].tolist() == got[r] and np.array_equal(bits(tl[:, 0]), bits(lp))
    if mode == "greedy":
        assert all(len(s) == N_PREDICT for s in want)
    else:
        assert any(len(s) < N_PREDICT for s in want), "fixture problem: no sequence ended at the EOS id"
        eos = runs.eos_for(n, 1)
        assert all(s[-1] == eos for s in want if len(s) < N_PREDICT) and all(eos not in s[:-1] for s in want)
    assert np.array_equal(np.concatenate([bits(i[0]) for i in runs.get(mode, n, 1, 5)[1]]), np.concatenate([bits(i[0]) for i in runs.get(mode, n, 1, 0)[1]]))


# ---- 2. n_batch = 1: against scoring, bit for bit ----

def score_targets(g, seqs, prompts, targets):
    """score_batch of prompt ++ ids with `targets` behind the prompt's last row (and -1 elsewhere): the rows that chose the generated tokens."""
    full = [p + s for p, s in zip(prompts, seqs)]
    tg = [[-1] * (len(p) - 1) + [int(v) for v in t] + [-1] for p, t in zip(prompts, targets)]
    out = g.score_batch(full, tg)
    return [out[r][0][len(prompts[r]) - 1:len(prompts[r]) - 1 + len(seqs[r])] for r in range(len(seqs))]


@pytest.mark.parametrize("n", [1, 3, 9, 50])
@pytest.mark.parametrize("mode", ["greedy", "sample"])
def test_lp_equals_score_batch(model, runs, mode, n):
    ids, info, prompts = runs.get(mode, n, 1, 5)
    want = score_targets(model, ids, prompts, ids)
    for r in range(n):
        assert np.array_equal(bits(info[r][0]), bits(want[r])), (mode, n, r, info[r][0].tolist(), want[r].tolist())


@pytest.mark.parametrize("K", [1, 5, 8])
@pytest.mark.parametrize("mode", ["greedy", "sample"])
def test_top_lp_equals_score_batch(model, runs, mode, K):
    n = 3
    ids, info, prompts = runs.get(mode, n, 1, K)
    assert ids == runs.get(mode, n, 1, None)[0]
    want = score_targets(model, ids * K, prompts * K, [info[r][1][:, j] for j in range(K) for r in range(n)])
    lp_want = score_targets(model, ids, prompts, ids)
    for r in range(n):
        assert np.array_equal(bits(info[r][0]), bits(lp_want[r])), (mode, K, r)
        for j in range(K):
            assert np.array_equal(bits(info[r][2][:, j]), bits(want[j * n + r])), (mode, K, r, j)
        if K > 1:      # the order: value descending -- equal log-probabilities are not told apart here, the kernel tests do that
            assert (np.diff(info[r][2], axis=1) <= 0).all()
        assert all(len(set(row)) == K for row in info[r][1].tolist())


# ---- 3. n_batch = 8: against the rows of a host loop of biogpt_hip_eval ----

def eval_rows(g, prompt, ids, nb):
    """The logits rows that chose ids[0], ids[1], ...: the prompt in chunks of nb, then one token at a time."""
    row = None
    for at in range(0, len(prompt), nb):
        row = g.eval(prompt[at:at + nb], at)
    rows = [row.copy()]
    for t, tok in enumerate(ids[:-1]):
        rows.append(g.eval([tok], len(prompt) + t).copy())
    return np.stack(rows)


@pytest.mark.parametrize("mode", ["greedy", "sample"])
def test_n_batch_8_equals_the_eval_loop(pkg, model, runs, mode):
    n, K = 3, 5
    ids, info, prompts = runs.get(mode, n, 8, K)
    assert ids == runs.get(mode, n, 8, None)[0]
    for r in range(n):
        rows = eval_rows(model, prompts[r], ids[r], 8)
        lp, ti, tl = info[r]
        want, am, _ = pkg.logprob_rows(rows, np.asarray(ids[r]))
        assert np.array_equal(bits(lp), bits(want)), (mode, r, lp.tolist(), want.tolist())
        order = np.stack([np.lexsort((np.arange(row.size), -row.astype(np.float64)))[:K] for row in rows])
        assert np.array_equal(ti, order), (mode, r)
        assert np.array_equal(ti[:, 0], am)
        for j in range(K):
            assert np.array_equal(bits(tl[:, j]), bits(pkg.logprob_rows(rows, ti[:, j])[0])), (mode, r, j)


# ---- 4. behind a shared prefix ----

@pytest.mark.parametrize("n,path", [(3, 1), (9, 0)])
@pytest.mark.parametrize("mode", ["greedy", "sample"])
def test_prefix_forms_equal_the_call_on_the_concatenations(model, runs, mode, n, path):
    K = 5
    ids, info, seqs = runs.get(mode, n, 8, K, prefix=True)
    st = model.prefix_stats()
    assert st["n_shared"] == 16 and st["path"] == path and st["columns"] == n, st
    plain, _, _ = runs.get(mode, n, 8, None, prefix=True)
    assert ids == plain
    if mode == "greedy":
        w_ids, w_info, _ = model.generate_greedy_batch(seqs, N_PREDICT, n_batch=8, logprobs=K)
    else:
        w_ids, w_info, _ = model.generate_sample(seqs, N_PREDICT, seed=SEED0, eos_id=runs.eos_for(n, 8), n_batch=8, logprobs=K, **HOT)
    assert ids == [list(map(int, s)) for s in w_ids]
    for r in range(n):
        assert np.array_equal(bits(info[r][0]), bits(w_info[r][0])), (mode, n, r)
        assert np.array_equal(info[r][1], w_info[r][1]), (mode, n, r)
        assert np.array_equal(bits(info[r][2]), bits(w_info[r][2])), (mode, n, r)


# ---- 5. the tail; other K on the same context ----

def test_tail_entries_and_other_k_on_the_same_context(pkg, model, runs):
    n, nb = 3, 1
    prompts, _ = runs.layout(n)
    eos = runs.eos_for(n, nb)
    want, w_info, _ = runs.get("sample", n, nb, 8)
    flat = np.ascontiguousarray(np.concatenate([np.asarray(p, dtype=np.int32) for p in prompts]))
    lens = np.asarray([len(p) for p in prompts], dtype=np.int32)
    sd = np.asarray([SEED0 + r for r in range(n)], dtype=np.uint32)
    for K in (8, 2, 0, 5):      # the captured steps and the device block of K = 8 serve the others
        out, ol, secs = np.full((n, N_PREDICT), 12345, dtype=np.int32), np.zeros(n, dtype=np.int32), ctypes.c_double(0.0)
        lp = np.full((n, N_PREDICT), np.float32(7.0))
        ti, tl = np.full((n, N_PREDICT, max(K, 1)), 12345, dtype=np.int32), np.full((n, N_PREDICT, max(K, 1)), np.float32(7.0))
        req = pkg.GenLogprobs(K, lp.ctypes.data, ti.ctypes.data, tl.ctypes.data)
        assert pkg.lib().biogpt_hip_generate_sample_lp(model._h, None, 0, flat.ctypes.data, lens.ctypes.data, n, 1, nb, N_PREDICT, HOT["top_k"], HOT["top_p"], HOT["temp"],
                                                       sd.ctypes.data, eos, out.ctypes.data, ol.ctypes.data, ctypes.byref(secs), ctypes.byref(req)) == N_PREDICT, pkg._err()
        assert any(int(v) < N_PREDICT for v in ol)
        for r in range(n):
            m = int(ol[r])
            assert out[r, :m].tolist() == want[r] and (out[r, m:] == -1).all()
            assert np.array_equal(bits(lp[r, :m]), bits(w_info[r][0])) and not lp[r, m:].any(), (K, r)
            if K:
                assert np.array_equal(ti[r, :m], w_info[r][1][:, :K]) and (ti[r, m:] == -1).all(), (K, r)
                assert np.array_equal(bits(tl[r, :m]), bits(w_info[r][2][:, :K])) and not tl[r, m:].any(), (K, r)
            else:
                assert (ti == 12345).all() and (tl == 7.0).all()      # n_top = 0: not touched
    # greedy on the same context, K = 8 then 3
    g8, i8, _ = runs.get("greedy", n, nb, 8)
    g3, i3, _ = runs.get("greedy", n, nb, 3)
    assert g8 == g3
    for r in range(n):
        assert np.array_equal(bits(i8[r][0]), bits(i3[r][0])) and np.array_equal(i8[r][1][:, :3], i3[r][1]) and np.array_equal(bits(i8[r][2][:, :3]), bits(i3[r][2]))


def test_n_top_beyond_a_call_s_reach_and_plain_errors_still_fail(pkg, model):
    with pytest.raises(pkg.BiogptError, match="n_top"):
        req = pkg.GenLogprobs(9, 1, 1, 1)
        out, secs = np.zeros((1, 4), np.int32), ctypes.c_double(0.0)
        p, pl = np.asarray([2, 5], np.int32), np.asarray([2], np.int32)
        if pkg.lib().biogpt_hip_generate_greedy_batch_lp(model._h, None, 0, p.ctypes.data, pl.ctypes.data, 1, 8, 4, out.ctypes.data, ctypes.byref(secs), ctypes.byref(req)) < 0:
            raise pkg.BiogptError(pkg._err())
    with pytest.raises(pkg.BiogptError, match="empty prompt"):
        model.generate_greedy_batch([[2, 5], []], 4, logprobs=2)
    with pytest.raises(pkg.BiogptError, match="top_k"):
        model.generate_sample([[2, 5]], 4, top_k=0, logprobs=2)
    ids, info, _ = model.generate_greedy_batch([[2] * KW["n_positions"]], 4, logprobs=2)      # no room: nothing generated
    assert ids.shape == (1, 0) and [a.shape for a in info[0]] == [(0,), (0, 2), (0, 2)]


# ---- 6. the kernels alone, on hostile rows ----

KERNEL_WIDTHS = (42384, 42383, 1021, 70, 33)
SEED = 7


def hostile_rows(V):
    """Logits rows (given = False) and rows of log-probabilities with -inf entries (given = True: never fewer than 8 finite values), every kind at
    least four times: with an odd V on every 16-byte alignment."""
    names, rows = [], []
    for given in (False, True):
        kinds = bk.row_kinds(V, 4, given, SEED)
        for k in kinds:
            names += ["%s%s" % (k, "/lp" if given else "")] * len(kinds[k])
            rows.append(kinds[k])
    return names, np.ascontiguousarray(np.concatenate(rows), dtype=np.float32)


def order_of(row, K):
    return np.lexsort((np.arange(row.size), -row.astype(np.float64)))[:K]


def check_lps(V, names, rows, ids, lp, ti, tl, what):
    """ids' and the top entries' log-probabilities against the float64 log-softmax; returns the worst |diff| / tol."""
    worst, at = 0.0, ""
    for r in range(rows.shape[0]):
        ref = bk.log_softmax64(rows[r])[0]
        for got, where in ((lp[r:r + 1], ids[r:r + 1]), (tl[r], ti[r])):
            want = ref[where]
            assert np.isfinite(want).all(), (what, names[r], r)
            ratio = np.abs(got.astype(np.float64) - want) / bk.lp_tolerance(V, want)
            assert (ratio <= 1.0).all(), (what, V, names[r], r, got.tolist(), want.tolist(), ratio.tolist())
            if ratio.size and float(ratio.max()) > worst:
                worst, at = float(ratio.max()), names[r]
    return worst, at


@pytest.mark.parametrize("V", KERNEL_WIDTHS)
def test_greedy_kernel_on_hostile_rows(pkg, V):
    names, rows = hostile_rows(V)
    n = rows.shape[0]
    want8 = np.stack([order_of(row, 8) for row in rows])
    base = None
    for K in (8, 5, 1, 0):
        ids, lp, ti, tl = pkg.genlp_rows(rows, K, mode=0)
        bad = np.nonzero(ids != want8[:, 0])[0]
        assert bad.size == 0, (V, K, [(names[r], int(ids[r]), int(want8[r, 0])) for r in bad])
        assert np.array_equal(ti, want8[:, :K]), (V, K, [(names[r], ti[r].tolist(), want8[r, :K].tolist()) for r in range(n) if not np.array_equal(ti[r], want8[r, :K])])
        worst, at = check_lps(V, names, rows, ids, lp, ti, tl, "greedy K=%d" % K)
        print("genlp greedy V=%d K=%d: worst |diff| / tol = %.3f (%s)" % (V, K, worst, at))
        if base is None:
            base = (lp, tl)
        else:      # the numbers do not depend on K
            assert np.array_equal(bits(lp), bits(base[0])) and np.array_equal(bits(tl), bits(base[1][:, :K])), (V, K)
    # the arithmetic of logprob_rows_kernel, bit for bit
    s_lp, s_am, _ = pkg.logprob_rows(rows, want8[:, 0])
    assert np.array_equal(bits(base[0]), bits(s_lp)) and np.array_equal(s_am, want8[:, 0])
    for j in range(8):
        assert np.array_equal(bits(base[1][:, j]), bits(pkg.logprob_rows(rows, want8[:, j])[0])), (V, j)


def fresh_states(pkg, n, seed0):
    st = np.zeros((n, 625), dtype=np.uint32)
    for r in range(n):
        assert pkg.lib().biogpt_hip_mt19937_seed(seed0 + r, st[r].ctypes.data) == 0
    return st


def host_draws(pkg, rows, top_k, top_p, temp, states):
    """(index among the candidates, id) per row: the selection by the stable order + biogpt_hip_sample_candidates_host, states advanced in place."""
    out = []
    for r, row in enumerate(rows):
        order = order_of(row, top_k).astype(np.int32)
        vals = np.ascontiguousarray(row[order], dtype=np.float32)
        got = ctypes.c_int32(-1)
        assert pkg.lib().biogpt_hip_sample_candidates_host(vals.ctypes.data, order.ctypes.data, vals.size, top_p, temp, states[r].ctypes.data, ctypes.byref(got)) == 0, pkg._err()
        out.append((int(np.nonzero(order == got.value)[0][0]), int(got.value)))
    return out


@pytest.mark.parametrize("V", KERNEL_WIDTHS)
@pytest.mark.parametrize("top_k,top_p,temp,K", [(40, 0.9, 0.9, 8), (5, 0.5, 0.7, 8), (1, 0.9, 0.9, 5), (16, 1.0, 3.0, 0)])
def test_sampling_kernel_on_hostile_rows(pkg, V, top_k, top_p, temp, K):
    names, rows = hostile_rows(V)
    n = rows.shape[0]
    top_k = min(top_k, V)
    want8 = np.stack([order_of(row, 8) for row in rows])
    hs, ds, ps = fresh_states(pkg, n, 900), fresh_states(pkg, n, 900), fresh_states(pkg, n, 900)
    for step in range(2):
        ids, lp, ti, tl = pkg.genlp_rows(rows, K, mode=1, top_k=top_k, top_p=top_p, temp=temp, states=ds)
        want = host_draws(pkg, rows, top_k, top_p, temp, hs)
        bad = [(names[r], int(ids[r]), want[r]) for r in range(n) if int(ids[r]) != want[r][1]]
        assert not bad, (V, step, bad)
        plain = np.zeros(n, dtype=np.int32)
        assert pkg.lib().biogpt_hip_sample_rows_device(0, rows.ctypes.data, n, V, top_k, top_p, temp, ps.ctypes.data, plain.ctypes.data) == 0, pkg._err()
        assert np.array_equal(plain, ids) and np.array_equal(ps, ds), (V, step)      # the plain kernel: same ids, same states
        assert np.array_equal(ti, want8[:, :K]), (V, step, [(names[r], ti[r].tolist(), want8[r, :K].tolist()) for r in range(n) if not np.array_equal(ti[r], want8[r, :K])])
        finite = np.isfinite(rows[np.arange(n), ids])      # (a candidate of probability 0 is never drawn: the drawn id's logit is finite)
        assert finite.all(), [names[r] for r in np.nonzero(~finite)[0]]
        worst, at = check_lps(V, names, rows, ids, lp, ti, tl, "sampled")
        print("genlp sampled V=%d top_k=%d K=%d step %d: worst |diff| / tol = %.3f (%s)" % (V, top_k, K, step, worst, at))
        s_lp = pkg.logprob_rows(rows, ids)[0]
        assert np.array_equal(bits(lp), bits(s_lp)), (V, step)      # the arithmetic of logprob_rows_kernel, bit for bit
    # The generator's stream is the host's.  (The kernel regenerates an exhausted block on entry, the host at its first draw: a row that never drew holds
    # two forms of one state.  One more draw, on the host, from both brings them to the same form.)
    two, two_ids, got = np.zeros(2, dtype=np.float32), np.arange(2, dtype=np.int32), ctypes.c_int32(-1)
    for st in (ds, hs):
        for r in range(n):
            assert pkg.lib().biogpt_hip_sample_candidates_host(two.ctypes.data, two_ids.ctypes.data, 2, 1.0, 1.0, st[r].ctypes.data, ctypes.byref(got)) == 0, pkg._err()
    assert np.array_equal(ds, hs), V
