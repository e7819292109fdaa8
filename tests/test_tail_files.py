"""The tied model files of tests/wide_models.py (build_tail) are what they claim, proved with the oracle over exactly the rows tests/test_gpu_tail_calls.py
compares (wide_models.tail_plan): the lm_head is made of copies of a few base rows; (a) at some step the winning value's copies lie in different partials and its
lowest copy is not in the first of them; (b) at some step the winner's lowest copy is in rows 42368 .. 42383; (c) at some step a tie straddles place k; (d) the
row layout "b" hands topk_kernel has more than 4096 candidates at its threshold; every row's winning value stands 2e-3 above the next value (the F32 file's rows
are not bit-identical to the oracle's); the raw-edited Q8_0 file keeps at least k comparable logits in every compared row, and NaN, +inf and -inf each occur."""
import numpy as np
import pytest

import tail_ref as T
import wide_models as wm

K, V = wm.TIED_K, wm.V


@pytest.fixture(scope="module")
def compared(pkg, oracle, tmp_path_factory):
    files = wm.build_tail(pkg, tmp_path_factory.mktemp("tail"), wm.TAIL_FILES)
    out = {}
    for name in wm.TAIL_FILES:
        for what, prompt, steps in wm.tail_plan(name):
            o = oracle.OracleModel(files[name], n_threads=16)
            out[(name, what)] = list(wm.tail_rows(o, prompt, steps))
    return out


def test_layouts():
    for layout, copies in (("a", 1322), ("b", 5288)):
        c = wm.tied_classes(layout)
        n = 4 + wm.TIED_CYC[layout] + 4
        count = np.bincount(c, minlength=n)
        assert count[:4].tolist() == [16] * 4 and count[-4:].tolist() == [4] * 4 and count[4:-4].min() >= copies - 1 and count[4:-4].max() <= copies
        assert set(c[:64]) == {0, 1, 2, 3} and set(c[V - 16:]) == set(range(n - 4, n)) and set(c[64:128]) == set(range(4, 4 + min(64, wm.TIED_CYC[layout])))
    assert V - 16 == 662 * 64 == 42368 and wm.TIED_CYC["b"] * 4096 < V - 80 < wm.TIED_CYC["a"] * 4096
    a = wm.tied_classes("a")
    assert a[wm.TAIL_PINF_ROWS[0]] == a[wm.TAIL_PINF_ROWS[1]] and wm.TAIL_PINF_ROWS[0] // 64 == 2 != wm.TAIL_PINF_ROWS[1] // 64
    assert all(r // 64 in (1, 2, 3, 662) for r in wm.TAIL_NAN_ROWS) and wm.TAIL_NINF_ROWS[0] >= V - 16


def test_conditions_on_the_compared_rows(compared):
    a = b = c = 0
    for (name, what), rows in compared.items():
        layout = "b" if name.startswith("tied_b") else "a"
        cls = wm.tied_classes(layout)
        for n_past, row, tok in rows:
            assert row.shape == (V,) and tok == T.argmax(row)
            vals = np.unique(row[~np.isnan(row)])
            assert len(vals) >= 2 and (np.isinf(vals[-1]) or vals[-1] - vals[-2] >= 2e-3), (name, what, n_past, vals[-3:])
            if name == "tail_q8":
                continue
            assert len(vals) == cls.max() + 1 and np.isfinite(row).all(), (name, what, n_past)
            copies = np.flatnonzero(row == row[tok])
            assert copies[0] == tok and (cls[copies] == cls[tok]).all() and len(copies) == (cls == cls[tok]).sum()
            a += len({int(r) // 64 for r in copies}) > 1 and tok >= 64
            b += tok >= V - 16
            v, i = T.topk(row, K + 1)
            c += v[K - 1] == v[K]
    assert a >= 3 and b >= 2 and c >= 3, (a, b, c)


def test_layout_b_overflows_the_candidate_slots(compared):
    n_past, row, tok = compared[("tied_b.q4_0", "short")][0]          # the row eval_topk's prompt chunk leaves: topk_kernel's
    t0, raced = T.topk_threshold(T.block_maxima(row), 663, K)
    assert not raced and int((row >= t0).sum()) > T.TOPK_CAP and T.topk_kernel(row, T.block_maxima(row), 663, K)[0] == -1
    n_past, row, tok = compared[("tied_a.q4_0", "short")][0]          # layout "a": answered
    assert T.topk_kernel(row, T.block_maxima(row), 663, K)[0] == K


def test_edited_file_keeps_k_comparable_logits(compared):
    nan = pinf = ninf = 0
    for what in ("short", "second column", "long"):
        for n_past, row, tok in compared[("tail_q8", what)]:
            assert (~np.isnan(row)).sum() >= V - 8 >= K and np.isnan(row[list(wm.TAIL_NAN_ROWS)]).all()
            nan, pinf, ninf = nan + int(np.isnan(row).any()), pinf + int((row == np.inf).any()), ninf + int((row == -np.inf).any())
            edited = list(wm.TAIL_PINF_ROWS + wm.TAIL_NINF_ROWS)
            assert not np.isfinite(row[edited]).any() and np.isfinite(np.delete(row, edited + list(wm.TAIL_NAN_ROWS))).all()
    assert nan >= 10 and pinf >= 3 and ninf >= 3, (nan, pinf, ninf)
    # the lower +inf copy stands behind block 2's NaN: where +inf wins, a held NaN would hand the id to the copy 20 blocks later
    wins = [tok for what in ("short", "second column", "long") for _, row, tok in compared[("tail_q8", what)]]
    assert wm.TAIL_PINF_ROWS[0] in wins or any(64 < t < 128 for t in wins), wins
