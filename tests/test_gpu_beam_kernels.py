"""The scoring and beam-step kernels on their own, on rows and tables the test constructs (no model file anywhere in this module):

  (a) logprob_rows_kernel / lp_row_stats against a float64 log-softmax, on rows of every awkward kind at widths that put the scalar head and tail,
      the float4 body and the four alignments to work;
  (b) beam_group_rows_kernel<8 | 16 | 32, given> against a stable arg-sort, ids exact where values tie;
  (c) whole searches through rows -> select -> fork with a table for a model (biogpt_hip_beam_table_device): tables whose scores tie exactly
      against beam_ref bit for bit, Gaussian logits tables under the margin rule of test_gpu_beam.py, and the fork bookkeeping column by column
      and K / V row by K / V row.

The bound of (a) is beam_kernels_ref.lp_tolerance (derived there); every case prints its worst |diff| / tol."""
import numpy as np
import pytest

import beam_kernels_ref as bk
import beam_ref

pytestmark = pytest.mark.gpu

SEED = 7
MARGIN = 1e-5
RUN_SCORES = (-3.25, 0.0, -1e3)


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64)


# ---- (a) the log-softmax ----

@pytest.mark.parametrize("V", bk.WIDTHS)
def test_logprob_rows_against_float64(pkg, V):
    kinds = bk.row_kinds(V, 16, False, SEED)
    names = [k for k in kinds for _ in range(len(kinds[k]))]
    rows = np.concatenate([kinds[k] for k in kinds])
    n = rows.shape[0]
    ref = [bk.log_softmax64(r) for r in rows]
    rng = np.random.default_rng([SEED, V])
    am_want = np.array([am for _, am in ref])
    worst = {}
    for what, tg in (("arg-max", am_want), ("first", np.zeros(n, int)), ("last", np.full(n, V - 1)), ("second", np.ones(n, int)), ("last but one", np.full(n, V - 2)),
                     ("random", rng.integers(0, V, n)), ("none", np.full(n, -1))):
        lp, am, lg = pkg.logprob_rows(rows, tg)
        assert np.array_equal(am, am_want), (what, [(names[r], int(am[r]), int(am_want[r])) for r in np.nonzero(am != am_want)[0]])
        if what == "none":
            assert not lp.any() and not lg.any()
            continue
        assert np.array_equal(lg.view(np.int32), rows[np.arange(n), tg].view(np.int32)), what
        want = np.array([ref[r][0][tg[r]] for r in range(n)])
        ratio = np.abs(lp.astype(np.float64) - want) / bk.lp_tolerance(V, want)
        for r in range(n):
            worst[names[r]] = max(worst.get(names[r], 0.0), float(ratio[r]))
        bad = np.nonzero(~(ratio <= 1.0))[0]
        print("logprob_rows V=%d target %s: worst |diff| / tol = %.3f (%s)" % (V, what, ratio.max(), names[int(ratio.argmax())]))
        assert bad.size == 0, (V, what, [(names[r], r, int(tg[r]), float(lp[r]), float(want[r]), float(ratio[r])) for r in bad])
    print("logprob_rows V=%d: worst |diff| / tol over all targets = %.3f; per kind %s" % (V, max(worst.values()), {k: round(v, 3) for k, v in worst.items()}))


# ---- (b) the row kernel of a beam step ----

def check_beam_rows(pkg, V, B, given):
    kinds = bk.row_kinds(V, B, given, SEED)
    names = [k for k in kinds for _ in range(len(kinds[k]))]
    rows = np.concatenate([kinds[k] for k in kinds])
    pad = (-rows.shape[0]) % B        # whole groups: the first rows again
    rows = np.concatenate([rows, rows[:pad]])
    names += names[:pad]
    n, K = rows.shape[0], 2 * B
    rs = np.array([RUN_SCORES[r % 3] for r in range(n)], dtype=np.float32)
    want = [bk.row_candidates(rows[r], K, rs[r], given) for r in range(n)]
    worst = 0.0
    for first in (False, True):
        sc, col, ids = pkg.beam_rows(rows, B, rs, given=given, first_step=first)
        for r in range(n):
            if first and r % B:
                assert np.isnan(sc[r]).all() and (col[r] == -1).all() and (ids[r] == -1).all(), (names[r], r, "a row the first step must not expand was written")
                continue
            w_ids, w_sc = want[r]
            assert np.array_equal(ids[r], w_ids), (names[r], r, float(rs[r]), ids[r].tolist(), w_ids.tolist())
            assert (col[r] == r % B).all(), (names[r], r, col[r].tolist())
            if given:
                assert np.array_equal(sc[r].view(np.int32), w_sc.view(np.int32)), (names[r], r, sc[r].tolist(), w_sc.tolist())
            else:
                lp64 = bk.log_softmax64(rows[r])[0][w_ids]
                tol = bk.lp_tolerance(V, lp64) + ulp32(w_sc)
                ratio = np.abs(sc[r].astype(np.float64) - w_sc.astype(np.float64)) / tol
                worst = max(worst, float(ratio.max()))
                assert (ratio <= 1.0).all(), (names[r], r, float(rs[r]), sc[r].tolist(), w_sc.tolist(), ratio.tolist())
    return worst


@pytest.mark.parametrize("B", bk.BEAMS)
@pytest.mark.parametrize("V", bk.WIDTHS)
def test_beam_rows_against_stable_sort(pkg, V, B):
    check_beam_rows(pkg, V, B, True)
    worst = check_beam_rows(pkg, V, B, False)
    print("beam_rows V=%d B=%d: ids and parents exact in both modes, given scores bit-exact; logits mode worst |diff| / tol = %.3f" % (V, B, worst))


# ---- (c) whole searches over a table ----

def as_lists(hyps):
    return [([int(t) for t in ids], np.float32(s)) for ids, s in hyps]


@pytest.mark.parametrize("V,R,B", list(bk.tied_cases()))
def test_tied_searches_equal_the_restatement_bit_for_bit(pkg, V, R, B):
    table = bk.tied_table(V, R, bk.TIED_SEED)
    starts, plens = [g[0] for g in bk.GROUPS], [g[1] for g in bk.GROUPS]
    eos = bk.eos_of(V)
    lengths = []
    for es in (True, False):
        for lpen in bk.TIED_PENALTIES:
            want = [as_lists(bk.tied_reference(V, R, B, s, es, lpen)[0]) for s in starts]
            got3, _ = pkg.beam_table(table, starts, plens, B, bk.N_PREDICT, eos_id=eos, length_penalty=lpen, early_stopping=es)
            got1, _ = pkg.beam_table(table, starts[:1], plens[:1], B, bk.N_PREDICT, eos_id=eos, length_penalty=lpen, early_stopping=es)
            assert got3 is not None and got1 is not None
            for g in range(3):
                assert len(got3[g]) == len(want[g]), (es, lpen, g, len(got3[g]), len(want[g]))
                for r, ((ids_g, s_g), (ids_w, s_w)) in enumerate(zip(got3[g], want[g])):
                    assert ids_g == ids_w, (es, lpen, g, r, ids_g, ids_w)
                    assert s_g.view(np.int32) == s_w.view(np.int32), (es, lpen, g, r, float(s_g), float(s_w))
            assert [(i, float(s)) for i, s in got1[0]] == [(i, float(s)) for i, s in got3[0]], (es, lpen)
            lengths.append([len(i) for i, _ in got3[0]])
    print("tied V=%d B=%d: hypothesis lengths of group 0 %s" % (V, B, lengths))


@pytest.mark.parametrize("V,B", [(33, 2), (33, 16), (96, 5), (1001, 8), (1001, 12)])
def test_logits_searches_equal_the_restatement(pkg, V, B):
    """The non-GIVEN path through the shared step at small widths: Gaussian logits tables, the margin rule and the 1e-4 of test_gpu_beam.py."""
    rng = np.random.default_rng([SEED, V, B, 1])
    table = (rng.standard_normal((V, V)) * 2.5).astype(np.float32)
    starts, plens = [g[0] for g in bk.GROUPS], [g[1] for g in bk.GROUPS]
    first = beam_ref.beam_search(bk.table_logprobs(table, starts[0], given=False), B, bk.N_PREDICT, -1, 1.0, True)[0]
    eos = int(first[0][0][2])        # fires mid-run
    for es in (True, False):
        want = []
        for s in starts:
            hyps, margins = beam_ref.beam_search(bk.table_logprobs(table, s, given=False), B, bk.N_PREDICT, eos, 1.0, es)
            small = [(k + 1, m) for k, m in enumerate(margins) if m < MARGIN]
            assert not small, "fixture problem: selection margins below %g at steps %s" % (MARGIN, small)
            want.append(as_lists(hyps))
        got, _ = pkg.beam_table(table, starts, plens, B, bk.N_PREDICT, eos_id=eos, length_penalty=1.0, early_stopping=es, given=False)
        assert got is not None
        for g in range(3):
            assert len(got[g]) == len(want[g])
            for r, ((ids_g, s_g), (ids_w, s_w)) in enumerate(zip(got[g], want[g])):
                assert ids_g == ids_w, (es, g, r, ids_g, ids_w)
                assert abs(float(s_g) - float(s_w)) <= 1e-4, (es, g, r, float(s_g), float(s_w))


@pytest.mark.parametrize("max_steps", [1, 2, 7])
@pytest.mark.parametrize("V,R,B", [(33, 33, 2), (33, 33, 16), (96, 96, 5), (1001, 1001, 12), (1001, 1001, 16), (42384, 64, 8)])
def test_forks_column_by_column(pkg, V, R, B, max_steps):
    """No EOS, max_steps steps, every group still live: each column holds the running beam of its rank -- token, length, history, score -- and its
    K / V rows of the generated positions are the stamps of that history, both heads (a fork that copied a row too few leaves the stamp of the
    beam that had the column before)."""
    table = bk.tied_table(V, R, bk.TIED_SEED)
    starts, plens = [g[0] for g in bk.GROUPS], [g[1] for g in bk.GROUPS]
    res, st = pkg.beam_table(table, starts, plens, B, bk.N_PREDICT, eos_id=-1, length_penalty=1.0, early_stopping=False, max_steps=max_steps)
    assert res is None and not st["done"].any() and (st["step"] == max_steps).all()
    forked = 0
    for g, (start, n_prompt) in enumerate(bk.GROUPS):
        trace = []
        running = beam_ref.running_beams(bk.table_logprobs(table, start), B, bk.N_PREDICT, max_steps, -1, 1.0, False, trace)
        assert len(running) == B
        assert sorted(st["rank"][g].tolist()) == list(range(B)), (g, st["rank"][g].tolist())
        forked += sum(len(t["parents"]) - len(set(t["parents"])) for t in trace[1:])
        for c in range(B):
            hist, score = running[int(st["rank"][g, c])]
            assert st["n_gen"][g, c] == max_steps == len(hist)
            assert st["token"][g, c] == hist[-1], (g, c)
            assert st["hist"][g, c, :max_steps].tolist() == hist, (g, c, st["hist"][g, c, :max_steps].tolist(), hist)
            assert (st["hist"][g, c, max_steps:] == -1).all()
            assert st["run_score"][g, c].view(np.int32) == np.float32(score).view(np.int32), (g, c)
            for kv, cache in ((0, st["k"]), (1, st["v"])):
                for head in range(2):
                    assert np.array_equal(cache[g, c, head, n_prompt - 1], bk.stamp(start, n_prompt - 1, head, kv)), (g, c, kv, head)
                    for j in range(max_steps - 1):
                        assert np.array_equal(cache[g, c, head, n_prompt + j], bk.stamp(hist[j], n_prompt + j, head, kv)), (g, c, kv, head, j, cache[g, c, head, n_prompt + j])
                    assert (cache[g, c, head, n_prompt + max_steps - 1:] == -1.0).all(), (g, c, kv, head)
    print("forks V=%d B=%d after %d steps: %d forked children over the three groups" % (V, B, max_steps, forked))
