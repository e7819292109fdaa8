"""Pooling, normalisation and heads of biogpt_hip_embed_batch at the widths other than 1024, through whole calls: the wide chain's files of
tests/test_gpu_wide_chain.py (A: d_model 1600, B: d_model 192) and one F32 file of B's shape with the float chain switched on.  As tests/test_gpu_embed.py
sections 5 - 7 do at 1024: every stage against embed_ref in float64 on the engine's own rows, within the bounds that follow from the arithmetic
(embed_ref.*_bound); LAST against the rows bit for bit; repeat calls byte for byte.  16 columns per pass, so that sequences end on, start on and straddle passes."""
import numpy as np
import pytest

import embed_ref
from embed_cases import assert_within

pytestmark = pytest.mark.gpu

A = dict(n_vocab=2053, n_layer=2, n_head=25, n_positions=96, d_ff=6400, d_model=1600, n_merges=3)      # tests/test_gpu_wide_chain.py
B = dict(n_vocab=77, n_layer=1, n_head=3, n_positions=40, d_ff=96, d_model=192, n_merges=3)
KW = {"A": A, "B": B}
MODELS = [("A", "q4_0"), ("B", "q4_0"), ("B", "q5_1"), ("B", "f32")]      # (B, f32): the float chain
IDS = ["%s-%s" % m for m in MODELS]
LENS = [15, 1, 16, 2, 17, 33, 40, 7]      # flat starts 0, 15, 16, 32, 34, 51, 84, 124: on, off and across the borders of 16-column passes


def within(what, got, ref, bound):
    assert_within(got, ref, bound, what)


def make_seqs(fam, seed):
    rng = np.random.default_rng(seed)
    return [[2] + [int(v) for v in rng.integers(4, KW[fam]["n_vocab"], n - 1)] for n in LENS]


@pytest.fixture(scope="module")
def models(pkg, tmp_path_factory):
    d = tmp_path_factory.mktemp("embed_wide")
    ms = {}
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("BIOGPT_HIP_PROMPT_COLS", "16")
        f32 = {}
        for fam in KW:
            f32[fam] = str(d / ("%s_f32.bin" % fam))
            pkg.write_synthetic(f32[fam], **KW[fam])

        def get(fam, name):
            if (fam, name) not in ms:
                if name == "f32":
                    ms[(fam, name)] = pkg.BiogptModel.load(f32[fam], float_chain=True)
                else:
                    path = str(d / ("%s_%s.bin" % (fam, name)))
                    pkg.quantize_file(f32[fam], path, name)
                    ms[(fam, name)] = pkg.BiogptModel.load(path)
            return ms[(fam, name)]
        yield get
        for m in ms.values():
            m.close()


@pytest.mark.parametrize("fam,name", MODELS, ids=IDS)
def test_pooling_and_normalisation(models, fam, name):
    g, D = models(fam, name), KW[fam]["d_model"]
    seqs = make_seqs(fam, 5)
    served = g.float_launches if name == "f32" else g.wide_launches      # the chain that serves the passes: the float chain on the F32 file, the wide one elsewhere
    before = served()
    rows = g.embed_batch(seqs, pooling="none")
    assert served() > before, (fam, name)
    assert [r.shape for r in rows] == [(n, D) for n in LENS] and all(np.isfinite(r).all() for r in rows)
    last = g.embed_batch(seqs, pooling="last")
    mean = g.embed_batch(seqs, pooling="mean")
    assert last.shape == mean.shape == (len(seqs), D) and last.dtype == mean.dtype == np.float32
    for s, r in enumerate(rows):
        assert last[s].tobytes() == r[-1].tobytes(), (fam, name, s)
    within("mean", mean, np.stack([embed_ref.pool(r, "mean") for r in rows]), np.stack([embed_ref.mean_bound(r) for r in rows]))
    assert float(np.abs(mean - last).max()) > 1e-3      # (two different things)
    ln = g.embed_batch(seqs, pooling="last", normalize=True)
    within("last + normalize", ln, embed_ref.l2_normalize(last), embed_ref.normalize_bound(last))
    mn = g.embed_batch(seqs, pooling="mean", normalize=True)
    within("mean + normalize", mn, embed_ref.l2_normalize(mean), embed_ref.normalize_bound(mean))
    nn = g.embed_batch(seqs, pooling="none", normalize=True)
    flat = np.concatenate(rows)
    within("rows + normalize", np.concatenate(nn), embed_ref.l2_normalize(flat), embed_ref.normalize_bound(flat))
    assert float(np.abs(np.sqrt((ln.astype(np.float64) ** 2).sum(axis=1)) - 1.0).max()) <= 1e-6


@pytest.mark.parametrize("fam,name", MODELS, ids=IDS)
def test_heads(models, fam, name):
    g, D = models(fam, name), KW[fam]["d_model"]
    seqs = make_seqs(fam, 8)
    rng = np.random.default_rng(17)
    rows = g.embed_batch(seqs, pooling="none")
    last, flat = np.stack([r[-1] for r in rows]), np.concatenate(rows)
    mean = g.embed_batch(seqs, pooling="mean")
    for n_out in (1, 7, 256):
        W = rng.normal(0.0, 0.05, (n_out, D)).astype(np.float32)
        b = rng.normal(0.0, 0.5, n_out).astype(np.float32)
        got = g.embed_batch(seqs, pooling="last", head=(W, b))
        assert got.shape == (len(seqs), n_out)
        within("n_out = %d, last" % n_out, got, embed_ref.head(last, W, b), embed_ref.head_bound(last, W, b))
        got = g.embed_batch(seqs, pooling="mean", head=(W, b))
        within("n_out = %d, mean" % n_out, got, embed_ref.head(mean, W, b), embed_ref.head_bound(mean, W, b))
        got = g.embed_batch(seqs, pooling="none", head=(W, b))
        assert [r.shape for r in got] == [(n, n_out) for n in LENS]
        within("n_out = %d, every token" % n_out, np.concatenate(got), embed_ref.head(flat, W, b), embed_ref.head_bound(flat, W, b))
    W = rng.normal(0.0, 0.05, (7, D)).astype(np.float32)
    got = g.embed_batch(seqs, pooling="last", head=W)
    within("head without a bias", got, embed_ref.head(last, W), embed_ref.head_bound(last, W))


@pytest.mark.parametrize("fam,name", MODELS, ids=IDS)
def test_repeat_calls_are_byte_identical(models, fam, name):
    g, D = models(fam, name), KW[fam]["d_model"]
    seqs = make_seqs(fam, 2)
    W = np.random.default_rng(1).normal(0.0, 0.05, (3, D)).astype(np.float32)
    for kw in (dict(pooling="none", normalize=True), dict(pooling="mean", normalize=True), dict(pooling="mean", head=W), dict(pooling="last"), dict(pooling="none", head=W)):
        a = g.embed_batch(seqs, **kw)
        b = g.embed_batch(seqs, **kw)
        a, b = (np.concatenate(a), np.concatenate(b)) if kw["pooling"] == "none" else (a, b)
        assert a.tobytes() == b.tobytes(), (fam, name, kw)


def test_a_head_wider_than_the_lds_of_a_launch_is_refused_by_name(pkg, tmp_path):
    """d_model 2112 = 33 heads of 64 passes the loader and the wide chain's gate; head_rows_kernel's 8 rows of it are 67,584 bytes of LDS, over the 65,536 a
    launch gets: an argument error before any HIP call, not a launch failure."""
    f32, q40 = str(tmp_path / "w2112_f32.bin"), str(tmp_path / "w2112_q4_0.bin")
    pkg.write_synthetic(f32, **dict(B, n_head=33, d_model=2112))
    pkg.quantize_file(f32, q40, "q4_0")
    g = pkg.BiogptModel.load(q40)
    try:
        for pooling in ("last", "none"):
            with pytest.raises(pkg.BiogptError, match="width 2112 needs 67584 bytes of LDS"):
                g.embed_batch([[2, 5, 9], [2, 7]], pooling=pooling, head=np.ones((3, 2112), np.float32))
    finally:
        g.close()
