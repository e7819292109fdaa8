"""The probe of the embedding tail's four kernels (biogpt_hip_embed_device) and its case list, without a GPU: the symbol is declared, exported and bound; its
refusals come before any HIP call and name the field; every exact case of tests/embed_cases.py is exact in any order and no LayerNorm row is fragile; the float32
restatements of embed_ref agree with its float64 ones within the *_bound functions; and each named kernel mistake (embed_ref.MISTAKES), committed in the
restatement, changes an expected output of a case -- in bits on an exact case, beyond the bound on a bounded one."""
import ctypes
import os
import re

import numpy as np
import pytest

import chain_ref
import embed_cases as C
import embed_ref as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def test_symbol_exported_and_bound(pkg):
    hdr = open(os.path.join(ROOT, "include", "biogpt_hip.h")).read()
    name = "biogpt_hip_embed_device"
    assert re.search(r"\b%s\s*\(" % name, hdr)
    assert name in {n for n, _, _ in pkg.SYMBOLS}
    assert getattr(ctypes.CDLL(pkg.LIB_PATH), name) is not None
    assert getattr(pkg.lib(), name).restype is ctypes.c_int
    assert callable(pkg.embed_device)


# ---- refusals: -1 with the field named, before any HIP call (there is no device here: a HIP call would make it -2) ----

def _st(seq, pos):
    return C.states(np.asarray(seq), np.asarray(pos))


REFUSALS = [
    ("W no multiple of 4 (LN)", dict(stage="LN", x=np.zeros((1, 6), F32), ln_w=np.zeros(6, F32), ln_b=np.zeros(6, F32)), "W must be a multiple of 4"),
    ("W no multiple of 4 (POOL)", dict(stage="POOL", x=np.zeros((1, 62), F32), seq_states=_st([0], [0]), lens=[1], pass_cols=[1], pooling="last"), "W must be a multiple of 4"),
    ("W no multiple of 4 (HEAD)", dict(stage="HEAD", x=np.zeros((1, 10), F32), w=np.zeros((1, 10), F32)), "W must be a multiple of 4"),
    ("n_out 0", dict(stage="HEAD", x=np.zeros((1, 8), F32), w=np.zeros((1, 8), F32), n_out=0), r"n_out \(0\) must be in \[1, 256\]"),
    ("n_out 257", dict(stage="HEAD", x=np.zeros((1, 8), F32), w=np.zeros((257, 8), F32)), r"n_out \(257\) must be in \[1, 256\]"),
    ("w missing", dict(stage="HEAD", x=np.zeros((1, 8), F32), n_out=1), "w is NULL"),
    ("head width over the LDS of a launch", dict(stage="HEAD", x=np.zeros((1, 2052), F32), w=np.zeros((1, 2052), F32)), "width 2052 needs 65664 bytes of LDS"),
    ("columns of a sequence not consecutive", dict(stage="POOL", x=np.zeros((3, 8), F32), seq_states=_st([0, 1, 0], [0, 0, 1]), lens=[2, 1], pass_cols=[3], pooling="mean"),
     "columns of sequence 0 are not consecutive"),
    ("positions not consecutive", dict(stage="POOL", x=np.zeros((2, 8), F32), seq_states=_st([0, 0], [0, 2]), lens=[3], pass_cols=[2], pooling="mean"),
     "positions of sequence 0 not consecutive"),
    ("position at lens[seq]", dict(stage="POOL", x=np.zeros((2, 8), F32), seq_states=_st([0, 0], [0, 1]), lens=[1], pass_cols=[2], pooling="last"),
     r"position 1 at or past lens\[0\] = 1"),
    ("a run that stops short of its sequence inside a pass", dict(stage="POOL", x=np.zeros((4, 8), F32), seq_states=_st([0, 0, 0, 1], [0, 1, 2, 0]), lens=[8, 1], pass_cols=[4],
                                                                  pooling="mean"), r"sequence 0 stops at position 2, short of lens\[0\] - 1 = 7, inside pass 0"),
    ("seq_id past n_seqs", dict(stage="POOL", x=np.zeros((1, 8), F32), seq_states=_st([1], [0]), lens=[1], pass_cols=[1], pooling="last"), "seq_id 1 outside"),
    ("pass_cols short of n_rows", dict(stage="POOL", x=np.zeros((2, 8), F32), seq_states=_st([0, 0], [0, 1]), lens=[2], pass_cols=[1], pooling="last"), "pass_cols sum to 1"),
    ("none without normalize", dict(stage="POOL", x=np.zeros((1, 8), F32), pooling="none"), "launches nothing"),
    ("ln_b missing", dict(stage="LN", x=np.zeros((1, 8), F32), ln_w=np.zeros(8, F32)), "ln_w or ln_b is NULL"),
    ("scatter row outside the output", dict(stage="LN", x=np.zeros((1, 8), F32), ln_w=np.zeros(8, F32), ln_b=np.zeros(8, F32), seq_states=_st([4], [1]), slot_div=2, P=8,
                                            n_out_rows=16), "row 17 outside"),
    ("two columns on one scatter row", dict(stage="LN", x=np.zeros((2, 8), F32), ln_w=np.zeros(8, F32), ln_b=np.zeros(8, F32), seq_states=_st([0, 1], [3, 3]), slot_div=2,
                                            P=8, n_out_rows=8), "a second column writes row 3"),
    ("slot_div 0", dict(stage="LN", x=np.zeros((1, 8), F32), ln_w=np.zeros(8, F32), ln_b=np.zeros(8, F32), seq_states=_st([0], [0]), slot_div=0, P=8, n_out_rows=8),
     "slot_div must be at least 1"),
]


@pytest.mark.parametrize("what,kw,text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_probe_refuses_before_any_hip_call(pkg, what, kw, text):
    with pytest.raises(pkg.BiogptError, match=text):
        pkg.embed_device(**kw)


def test_refusal_returns_minus_one(pkg):
    x = np.zeros((1, 6), F32)
    out = np.zeros((2, 6), F32)
    rc = pkg.lib().biogpt_hip_embed_device(0, 0, 6, 1, x.ctypes.data, x.ctypes.data, x.ctypes.data, None, 0, 0, 1, 0, 0, None, 0, 0, None, None, None, 0, out.ctypes.data, None, None)
    assert rc == -1 and b"W must be a multiple of 4" in pkg.lib().biogpt_hip_last_error()
    rc = pkg.lib().biogpt_hip_embed_device(0, 3, 8, 1, x.ctypes.data, None, None, None, 0, 0, 1, 0, 0, None, 0, 0, None, None, None, 0, out.ctypes.data, None, None)
    assert rc == -1 and b"no stage" in pkg.lib().biogpt_hip_last_error()


# ---- the predicate ----

def test_exact_in_any_order():
    assert E.exact_in_any_order(np.array([1.0, 2.0 ** -52, -0.5]))
    assert not E.exact_in_any_order(np.array([1.0, 2.0 ** -53, 1.0]))             # 2 + 2^-53 needs 55 bits
    assert E.exact_in_any_order(np.array([2.0 ** 52, 2.0 ** 52 - 1.0]))
    assert E.exact_in_any_order(np.array([2.0 ** 52, 2.0 ** 52]))                 # multiples of 2^52
    assert not E.exact_in_any_order(np.array([2.0 ** 52, 2.0 ** 52, 1.0]))        # multiples of 1 with sum |terms| = 2^53 + 1
    assert E.exact_in_any_order(np.array([0.0, -0.0])) and E.exact_in_any_order(np.array([5e-324, -5e-324, 1e-310]))
    assert not E.exact_in_any_order(np.array([1.0, np.inf]))
    both = E.exact_in_any_order(np.array([[1.0, 1.0], [2.0 ** -30, 2.0 ** -60]]))
    assert both.tolist() == [True, False]
    third = F32(1.0) / F32(3.0)
    assert not E.exact_in_any_order(np.full(1600, float(third) ** 2))              # 48-bit squares, 1600 of them: no common grid below 2^53
    assert E.exact_sum(np.array([[-0.0], [-0.0]])).tobytes() == np.array([0.0]).tobytes()
    assert E.exact_sum(np.array([1e18, 1.0, -1e18, 1e-6]))[()] == 1.0 + 1e-6


# ---- the case list is what it says ----

def test_no_layernorm_row_is_fragile():
    assert C.LN_WIDTHS[0] == 1024 and set(C.LN_WIDTHS[1:]) == {4, 8, 252, 256, 260, 1028, 1280, 1600}
    for W in C.LN_WIDTHS:
        rows = C.ln_rows(W)
        assert rows.shape == (len(C.LN_FAMILIES), W) and rows.dtype == F32
        for f, r in zip(C.LN_FAMILIES, rows):
            assert not chain_ref.ln_fragile(r), (W, f)
    for name, kw in C.ln_cases():
        want = E.layer_norm_rows(**kw)
        live = np.ones(len(want), bool)
        live[-1] = False
        if "states" in kw:
            live[:] = False
            live[[(s[3] // kw["slot_div"]) * kw["P"] + s[0] for s in kw["states"]]] = True
            assert live.sum() == 6 and len(want) == 3 * C.LN_P + 1
        assert np.isfinite(want[live]).all(), name
        assert (want[~live].view(np.uint8) == 0xFF).all(), name


def _exact(sums):
    return all(bool(np.all(E.exact_in_any_order(t))) for t in sums)


@pytest.mark.parametrize("W", C.POOL_WIDTHS)
def test_pool_cases_are_exact_where_they_say_and_within_bounds_everywhere(W):
    cases = C.pool_cases(W) + ([C.thirds_case()] if W == C.POOL_WIDTHS[0] else [])
    seen = set()
    for c in cases:
        out, acc = C.pool_expected(c)
        seen.add((c["kind"], c["pooling"], c["normalize"], c["expect"]))
        if c["expect"] == "bits":
            assert _exact(C.pool_sums(c)), c["name"]
        elif c["expect"] == "acc":
            assert c["kind"] in C.EXACT_KINDS and _exact(C.pool_sums(dict(c, normalize=False))), c["name"]
        else:
            assert c["kind"] in C.BOUNDED_KINDS or (c["kind"] == "constant" and c["normalize"]), c["name"]
        # the float32 restatement against the float64 one of embed_ref (numpy's sums), within the stage's bound
        seq = c["states"][:, 3]
        if c["pooling"] == "mean" and not c["normalize"] and len(set(seq)) == len(c["lens"]) and all((seq == s).sum() == n for s, n in enumerate(c["lens"])):
            for s in range(len(c["lens"])):
                r = c["x"][seq == s]
                extra = E.subnormal_allowance() if c["kind"] == "subnormal" else 0.0
                assert (np.abs(out[s].astype(np.float64) - E.pool(r, "mean")) <= E.mean_bound(r) + extra).all(), (c["name"], s)
        if c["normalize"]:
            rows = C.pool_expected(dict(c, normalize=False))[0][:-1]
            assert (np.abs(out[:-1].astype(np.float64) - E.l2_normalize(rows)) <= E.normalize_bound(rows)).all(), c["name"]
        if c["pooling"] == "last" and not c["normalize"]:
            for s, n in enumerate(c["lens"]):
                src = c["x"][(seq == s) & (c["states"][:, 0] == n - 1)]
                assert len(src) == 1 and out[s].tobytes() == src[0].tobytes(), (c["name"], s)
        C.check_pool(c, out, acc)      # the check the GPU test applies to the probe's result accepts the restatement itself
    if W in (68, 1600):
        assert {k for k, _, _, _ in seen} == set(C.KINDS)
    assert {(p, n) for _, p, n, _ in seen} >= {("last", False), ("mean", False), ("last", True), ("mean", True), ("none", True)}


def test_pool_layouts_are_what_the_text_says():
    assert sorted(C.POOL_LENS) == [1, 2, 15, 16, 17, 33, 40]
    seq, pos, cols = C.pool_layout(C.POOL_LENS, "p16")
    starts = np.concatenate([[0], np.cumsum(C.POOL_LENS)])
    assert any(s % 16 == 0 and s > 0 for s in starts[:-1]) and any(e % 16 == 0 for e in starts[1:-1])
    assert any(s // 16 != (e - 1) // 16 for s, e in zip(starts[:-1], starts[1:]))      # a sequence straddles a border
    assert cols == [16] * 7 + [12] and C.pool_layout(C.POOL_LENS, "one")[2] == [124] and C.pool_layout(C.POOL_LENS, "p1")[2] == [1] * 124
    # constant: the mean of n equal floats is that float; stamp: a pooled element names its place
    c = next(c for c in C.pool_cases(68) if c["name"] == "pool W=68 constant p16 mean")
    out, _ = C.pool_expected(c)
    for s in range(len(C.POOL_LENS)):
        assert out[s].tobytes() == c["x"][seq == s][0].tobytes()
    c = next(c for c in C.pool_cases(68) if c["name"] == "pool W=68 stamp p16 last")
    out, _ = C.pool_expected(c)
    for s, n in enumerate(C.POOL_LENS):
        assert (out[s] == (s * 64 + n - 1) * 2048 + np.arange(68)).all()
    c = next(c for c in C.pool_cases(68) if c["name"] == "pool W=68 one_hot p16 last+normalize")
    out, _ = C.pool_expected(c)
    assert (np.abs(out[:-1]).sum(axis=1) == 1.0).all() and (np.abs(out[:-1]).max(axis=1) == 1.0).all()
    c = next(c for c in C.pool_cases(68) if c["name"] == "pool W=68 subnormal p16 none+normalize")
    zero = np.flatnonzero((c["x"] == 0).all(axis=1))
    assert len(zero) and np.signbit(c["x"][zero]).any() and (np.abs(c["x"][c["x"] != 0]) < 2.0 ** -126).all()
    assert C.pool_expected(c)[0][zero].tobytes() == c["x"][zero].tobytes()      # a zero row stays as it is, signs included


def test_head_cases_are_exact_where_they_say_and_within_bounds_everywhere():
    cases = C.head_cases()
    shapes = {(c["x"].shape[0], c["w"].shape[0], c["x"].shape[1]) for c in cases}
    assert (17, 5, 260) in shapes and (9, 256, 1600) in shapes
    assert {s[0] for s in shapes} == {1, 7, 8, 9, 17} and {s[1] for s in shapes} == {1, 3, 4, 5, 256} and {s[2] for s in shapes} == {4, 252, 256, 260, 1024, 1600}
    assert {c["kind"] for c in cases} == set(C.KINDS) and {c["b"] is None for c in cases} == {True, False}
    for c in cases:
        out = C.head_expected(c)
        if c["expect"] == "bits":
            assert c["kind"] in C.EXACT_KINDS and _exact(C.head_sums(c)), c["name"]
        else:
            assert c["kind"] in C.BOUNDED_KINDS
        assert np.isfinite(out[:-1]).all() and (out[-1].view(np.uint8) == 0xFF).all(), c["name"]
        extra = E.subnormal_allowance() if c["kind"] == "subnormal" else 0.0
        assert (np.abs(out[:-1].astype(np.float64) - E.head(c["x"], c["w"], c["b"])) <= E.head_bound(c["x"], c["w"], c["b"]) + extra).all(), c["name"]
    assert _exact(C.head_sums(C.head_border_case()))
    c = next(c for c in cases if c["name"] == "head rows=17 out=5 W=260 stamp")
    out = C.head_expected(c)
    for r in range(17):
        for o in range(5):
            assert out[r, o] == (r + 1) * (2048 * o + (37 * r) % 260 + 1) + (2048 * o + 260)


# ---- every named mistake is seen ----

def _head_seen(c, mistake):
    """Does the mistaken expectation differ in a way the GPU test notices: in bits where the case is held bit for bit, beyond head_bound elsewhere."""
    want, wrong = C.head_expected(c), C.head_expected(c, mistake)
    if c["expect"] == "bits":
        return C.differs_in_bits(want, wrong)
    ref, bound = C.head_bound(c)
    return bool((np.abs(wrong[:-1].astype(np.float64) - ref) > bound).any()) or C.differs_in_bits(want[-1], wrong[-1])


def _pool_seen(c, mistake):
    """Does C.check_pool, the GPU test's own check, refuse the mistaken restatement's result."""
    try:
        C.check_pool(c, *C.pool_expected(c, mistake))
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("mistake", sorted(E.MISTAKES))
def test_each_mistake_changes_an_expected_output(mistake):
    seen = []
    if mistake.startswith("ln_"):
        for name, kw in C.ln_cases():
            if C.differs_in_bits(E.layer_norm_rows(**kw), E.layer_norm_rows(mistake=mistake, **kw)):
                seen.append(name)
    elif mistake.startswith("head_"):
        for c in C.head_cases():
            if c["x"].shape[1] > 1024 and c["w"].shape[0] > 5:
                continue      # (the largest shape adds no kind)
            if _head_seen(c, mistake):
                seen.append(c["name"])
    else:
        for c in [c for W in (68, 16) for c in (C.pool_cases(W) if W == 68 else [C.thirds_case()])]:
            if _pool_seen(c, mistake):
                seen.append(c["name"])
    print(mistake, "-- seen by %d cases, e.g." % len(seen), seen[:4])
    assert seen, "no case sees '%s' (%s): the case list is incomplete" % (mistake, E.MISTAKES[mistake])


def test_mistakes_are_seen_by_the_cases_meant_for_them():
    """The hostile cases do their own work: rows that are alike see the dropped row, the thirds see the unrounded mean, cancellation sees float32 sums."""
    by_name = {c["name"]: c for c in C.pool_cases(68)}
    c = by_name["pool W=68 constant p16 mean"]
    assert C.differs_in_bits(C.pool_expected(c)[0], C.pool_expected(c, "mean_drop_16th")[0])
    c = by_name["pool W=68 cancel p16 mean"]
    assert _pool_seen(c, "mean_f32_sum")
    # normalize_bound alone, on the kernel's own mean, is tight enough for a float32 square root to show where 124 rows give it the chance (its error and the
    # result's rounding are half a unit each: a single row need not show it; the exact kinds see it in bits)
    assert _pool_seen(by_name["pool W=68 gauss p16 mean+normalize"], "norm_sqrtf")
    for kind in C.BOUNDED_KINDS:
        assert _pool_seen(by_name["pool W=68 %s p16 none+normalize" % kind], "norm_sqrtf"), kind
    assert _pool_seen(by_name["pool W=68 gauss p1 mean"], "mean_pass_count")      # out against (float)(acc / len) of the returned accumulator
    c = C.thirds_case()
    assert _exact(C.pool_sums(c)) and C.differs_in_bits(C.pool_expected(c)[0], C.pool_expected(c, "norm_unrounded_mean")[0])
    h = {c["name"]: c for c in C.head_cases()}
    c = h["head rows=17 out=5 W=260 constant +b"]
    assert C.differs_in_bits(C.head_expected(c), C.head_expected(c, "head_bias_f32"))
    c = h["head rows=17 out=5 W=260 grid"]
    assert C.differs_in_bits(C.head_expected(c), C.head_expected(c, "head_pad_last_row")) and C.differs_in_bits(C.head_expected(c), C.head_expected(c, "head_drop_chunk"))
