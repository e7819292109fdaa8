"""tests/assoc_ref.py -- the numpy restatement the GPU tests hold the SIMD association's kernels to -- held to the oracle (bo_opts.assoc = 3, bo_attn_head with
assoc = 1) on the CPU, bit for bit; and the inputs of tests/assoc_cases.py shown, on the references alone, to tell the two associations apart."""
import ctypes
import ctypes.util

import numpy as np
import pytest

import assoc_cases as AC
import assoc_ref as A
import chain_ref as R
import modelfile_py

F32 = np.float32
TINY = dict(n_vocab=256, n_layer=1, n_head=2, n_positions=64, d_ff=256, d_model=128, n_merges=16)
FTYPE_NAMES = {R.Q4_0: "q4_0", R.Q4_1: "q4_1", R.Q5_0: "q5_0", R.Q5_1: "q5_1", R.Q8_0: "q8_0"}


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def test_fma32_is_the_c_library_fmaf():
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.fmaf.restype, libm.fmaf.argtypes = ctypes.c_float, [ctypes.c_float] * 3
    rng = np.random.default_rng(3)
    n = 20000
    a = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 6, n)).astype(F32)
    b = np.where(rng.random(n) < 0.5, rng.integers(-64516, 64517, n).astype(F32), rng.standard_normal(n).astype(F32))
    c = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 6, n)).astype(F32)
    c[: n // 4] = -(a[: n // 4] * b[: n // 4]).astype(F32)      # cancellation: the product's low bits decide
    want = np.array([libm.fmaf(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], dtype=F32)
    assert (bits(A.fma32(a, b, c)) == bits(want)).all()


@pytest.mark.parametrize("T", [1, 31, 32, 33, 64, 65, 101])
def test_attention_is_the_oracles(oracle, T):
    q, K, V = AC.attn_inputs(2, 1, 128, seed=T)
    for h in range(2):
        qv = q[0, h * 64:(h + 1) * 64]
        want = oracle.attn_head(qv, K[h], V[h], T, assoc=1)
        got = A.attn_head(qv, K[h], V[h], T)
        assert (bits(got) == bits(want)).all()
        scalar = oracle.attn_head(qv, K[h], V[h], T, assoc=0)
        print("T = %d, head %d: %d of 64 outputs differ between the associations" % (T, h, int((bits(want) != bits(scalar)).sum())))


@pytest.fixture(scope="module")
def tiny_files(pkg, tmp_path_factory):
    d = tmp_path_factory.mktemp("assoc_tiny")
    f32 = str(d / "f32.bin")
    pkg.write_synthetic(f32, **TINY)
    out = {}
    for wtype, name in FTYPE_NAMES.items():
        out[wtype] = str(d / (name + ".bin"))
        pkg.quantize_file(f32, out[wtype], name)
    return out


@pytest.mark.parametrize("wtype", R.TYPES, ids=[R.NAMES[t] for t in R.TYPES])
def test_quantization_and_dot_give_the_oracles_k_rows(oracle, tiny_files, wtype):
    """Layer 0's K rows: embeddings -> the oracle's LayerNorm -> the restatement's Q8 rows and block dot on the file's k_proj rows, + bias == the oracle's cache."""
    path = tiny_files[wtype]
    o = oracle.OracleModel(path, assoc=3)
    tokens = [2, 17, 99, 200, 5, 63, 128, 31, 7]
    o.eval(tokens, 0)
    x = o.tap(-1)
    assert x.shape == (len(tokens), TINY["d_model"])
    _, _, _, tensors = modelfile_py.read_model(path)
    t = {e["name"]: e for e in tensors}
    f32 = lambda name: np.frombuffer(t[name]["raw"], dtype=F32)
    lw, lb = f32("biogpt.layers.0.self_attn_layer_norm.weight"), f32("biogpt.layers.0.self_attn_layer_norm.bias")
    kw, kb = t["biogpt.layers.0.self_attn.k_proj.weight"], f32("biogpt.layers.0.self_attn.k_proj.bias")
    assert kw["type"] == wtype
    D = TINY["d_model"]
    raw = np.frombuffer(kw["raw"], dtype=np.uint8)
    y = np.stack([oracle.layer_norm(r, lw, lb) for r in x])
    acc = A.block_sums(wtype, raw, D, D, *A.quantize_q8(y, R.Q81[wtype]))
    got = (kb[None, :] + acc).astype(F32)
    want = o.kv(0)[0, :len(tokens), :]
    assert (bits(got) == bits(want)).all()
    # the same rows in the scalar association: the fixture tells the modes apart
    scalar = R.block_sums(wtype, raw, D, D, *R.quantize_q8(y, R.Q81[wtype]))
    share = float((bits(acc) != bits(scalar)).mean())
    print("%s: K rows of the tiny file, %.0f %% differ between the associations" % (R.NAMES[wtype], 100 * share))
    assert share >= 1 / 3
    o.close()


@pytest.mark.parametrize("K", [32, 64, 1024])
@pytest.mark.parametrize("q81", [False, True])
def test_q8_rows_hold_the_hostile_blocks(K, q81):
    """The rows of tests/assoc_cases.py hold the blocks that part the two quantizations, and the restatement's codes are, element by element, the
    nearest-even of fl(x * fl(127 / amax)).  (The oracle exposes its SIMD rows through a model's mat-vec only: the K-row test above holds quantization and
    dot together to it.)"""
    x = AC.q8_rows(K)
    q, d, s = A.quantize_q8(x, q81)
    qs, ds, ss = R.quantize_q8(x, q81)
    # the hostile blocks do what they are there for
    assert (q[0, :32] != qs[0, :32]).sum() >= 15, "the tie block separates nearest-even from roundf"
    a = AC.recip_amax()
    assert F32(F32(127.0) / a) != F32(F32(1.0) / F32(a / F32(127.0)))
    assert (q[2, :32] == 0).all() and d[2, 0] == 0 and s[2, 0] == 0
    assert (q[0, :32] == np.rint(AC.tie_block()).astype(np.int8)).all() and d[0, 0] == 1.0
    # every block from first principles, one element at a time
    v = x.reshape(8, K // 32, 32)
    amax = np.abs(v).max(axis=-1)
    for r in range(8):
        for b in range(K // 32):
            am = float(amax[r, b])
            idv = float(F32(F32(127.0) / F32(am))) if am != 0 else 0.0
            want = [int(np.rint(F32(F32(e) * F32(idv)))) for e in v[r, b]]
            assert list(q[r, b * 32:(b + 1) * 32]) == want


@pytest.mark.parametrize("wtype", R.TYPES, ids=[R.NAMES[t] for t in R.TYPES])
def test_mat_vec_cases_tell_the_associations_apart(wtype):
    """On the references alone: in every case the GPU test launches, the SIMD restatement differs from the scalar one (tests/chain_ref.py) in at least a
    third of the output rows -- a kernel that computed the scalar association would not pass one of them."""
    for case in AC.matvec_cases(wtype) + ([AC.lm_head_case()] if wtype == R.Q4_0 else []):
        share = AC.share_differing(case)
        print("%s: %.0f %% of the rows differ between the associations" % (case.name, 100 * share))
        assert share >= 1 / 3, case.name
