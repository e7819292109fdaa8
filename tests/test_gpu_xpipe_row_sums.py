"""The in-order row sums of the pipelined decode launch (csrc/kernels_xpipe.hip.h, xp_run): the q / k / v rows of stage A, the fc1 rows of stage D (thread t < 128
sums row t behind the stage's barrier and hands the GELU value to the Q8 step in its register) and the fc2 rows of stage E.  Whichever lanes sum a row, the row
keeps the oracle's additions in the oracle's order: block 0, 1, 2, ... of the row.

Files: d_model 1024, one layer (the fewest the pipeline takes), a vocabulary of 2048.  "plain" as Q4_0, Q5_1 and Q8_0 -- the settled-signed, the {d, m} and the
plain unit forms -- and "ranged.q4_0", whose q / k / v, fc1 and fc2 weights carry a factor 2^e per (row, block), e in -7 .. 7 with both ends in every row, so
that the block terms of a row span thousands and a re-associated sum changes bits.  The set-up shows that on the CPU before any row is compared: on the file's
own quantized weights, a pairwise-tree sum of the block terms (tests/chain_ref.py's arithmetic, held to its block_sums) differs from the in-order sum in at
least HALF of the rows of each of the three matrices.

Every compared row: finite and bit-identical to the oracle."""
import os

import numpy as np
import pytest

import chain_ref as R
from modelfile_py import read_model
import wide_models as wm

pytestmark = pytest.mark.gpu

F32 = np.float32
KW = dict(n_vocab=2048, n_layer=1, n_head=16, n_positions=256, d_ff=4096, d_model=1024, n_merges=3)
FILES = ["plain.q4_0", "plain.q5_1", "plain.q8_0", "ranged.q4_0"]
CONTEXTS = (0, 1, 31, 63, 64, 127, 128, 191)      # the 64-, 128- and 192-key variants, both q / k / v forms (the head's own rows up to 128 keys, handed over beyond)
RESIDENT_CONTEXTS = (1, 63, 64, 127)
E_MAX = 7                                          # block factors 2^-7 .. 2^7
MIN_SPAN = 2.0 ** 12                               # ... which must leave the quantized block scales of every row at least this far apart
MIN_SHARE = 0.5                                    # share of a matrix's rows whose pairwise-tree sum must differ from the in-order sum
N_PROMPT, N_GEN = 60, 40                           # generate_greedy over 60 .. 99 keys: the 64-key launch, then the 128-key one
MATRICES = {"q/k/v": ["self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj"], "fc1": ["fc1"], "fc2": ["fc2"]}


def tokens(seed, n):
    rng = np.random.default_rng(seed)
    return [2] + [int(v) for v in rng.integers(4, KW["n_vocab"], n - 1)]


def ranged(W):
    """x 2^e per (row, block) of the q / k / v, fc1 and fc2 weights, e in -E_MAX .. E_MAX, both ends in every row; their biases x 8 (the rows grow about as much)."""
    rng = np.random.default_rng(0x524F5753)
    for l in range(KW["n_layer"]):
        for group in MATRICES.values():
            for name in group:
                a = wm._own(W, wm.lname(l, name + ".weight"))
                M, nb = a.shape[0], a.shape[1] // 32
                e = rng.integers(-E_MAX, E_MAX + 1, (M, nb))
                ends = np.argsort(rng.random((M, nb)), axis=1)[:, :2]
                e[np.arange(M), ends[:, 0]], e[np.arange(M), ends[:, 1]] = -E_MAX, E_MAX
                a.reshape(M, nb, 32)[...] *= np.ldexp(F32(1.0), e)[:, :, None].astype(F32)
                wm._own(W, wm.lname(l, name + ".bias"))[...] *= F32(8.0)


def block_terms(wtype, raw, M, K, x):
    """float32 [M, K / 32]: the block terms of every weight row against ONE activation row x, as tests/chain_ref.py's block_sums forms them (Q4_0)."""
    assert wtype == R.Q4_0
    codes, dw, _ = R.decode_weights(wtype, raw, M, K)
    q, d, s = R.quantize_q8(x[None, :], False)
    dots = np.einsum("mbk,bk->mb", codes.astype(np.int32), q.reshape(K // 32, 32).astype(np.int32)).astype(F32)      # exact integers
    terms = ((dots * dw).astype(F32) * d[0][None, :]).astype(F32)
    in_order = np.add.accumulate(terms, axis=1, dtype=F32)[:, -1]                                                   # one term after another
    assert (in_order == R.block_sums(wtype, raw, M, K, q, d, s)[0]).all(), "the terms are not chain_ref's"
    return terms, dw, in_order


def tree_sum(terms):
    t = terms
    while t.shape[1] > 1:
        t = (t[:, 0::2] + t[:, 1::2]).astype(F32)
    return t[:, 0]


def order_sensitive_shares(path):
    """{matrix: share of its rows whose pairwise-tree sum differs from the in-order sum}, and the least span of a row's block scales."""
    _, _, _, tensors = read_model(path)
    T = {t["name"]: t for t in tensors}
    rng = np.random.default_rng(7)
    shares, span = {}, np.inf
    for what, group in MATRICES.items():
        differ = rows = 0
        for name in group:
            t = T[wm.lname(0, name + ".weight")]
            K, M = t["ne"]
            # a LayerNorm output (q / k / v, fc1), a GELU output (fc2): what the stage's Q8 step sees
            x = rng.normal(0.0, 1.0, K).astype(F32) if what != "fc2" else (np.maximum(rng.normal(0.0, 1.0, K), -0.17) * 0.5).astype(F32)
            terms, dw, in_order = block_terms(t["type"], np.frombuffer(t["raw"], dtype=np.uint8), M, K, x)
            differ += int((tree_sum(terms) != in_order).sum())
            rows += M
            span = min(span, float((np.abs(dw).max(axis=1) / np.abs(dw).min(axis=1)).min()))
        shares[what] = differ / rows
    return shares, span


@pytest.fixture(scope="module")
def files(pkg, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("row_sums"))
    out = {}
    plain = os.path.join(d, "plain.f32.bin")
    pkg.write_synthetic(plain, **KW)
    hp, vocab, merges, order, W = wm.load_arrays(plain)
    T = dict(W)
    ranged(T)
    wide = os.path.join(d, "ranged.f32.bin")
    wm.save_arrays(wide, hp, vocab, merges, order, T)
    for name in FILES:
        which, typ = name.split(".")
        out[name] = os.path.join(d, name + ".bin")
        pkg.quantize_file(plain if which == "plain" else wide, out[name], typ)
    os.remove(plain); os.remove(wide)
    # the order must matter, or the comparisons below show nothing about it
    shares, span = order_sensitive_shares(out["ranged.q4_0"])
    print("ranged.q4_0: least span of a row's block scales 2^%.1f; rows whose pairwise-tree sum differs from the in-order sum: %s"
          % (np.log2(span), ", ".join("%s %.1f %%" % (k, 100 * v) for k, v in shares.items())))
    assert span >= MIN_SPAN, "block scales of a row span only 2^%.1f" % np.log2(span)
    for what, share in shares.items():
        assert share >= MIN_SHARE, "%s: a re-associated sum changes only %.1f %% of the rows" % (what, 100 * share)
    return out


def plan():
    """[(tokens, n_past, compared)]: single tokens at CONTEXTS, chunks of up to 8 tokens between them."""
    t = tokens(1, CONTEXTS[-1] + 1)
    steps, at = [], 0
    for c in CONTEXTS:
        while at < c:
            n = min(8, c - at)
            steps.append((t[at:at + n], at, False))
            at += n
        steps.append((t[c:c + 1], c, True))
        at = c + 1
    return steps


@pytest.fixture(scope="module")
def rows_of(oracle, files):
    """The oracle's compared rows of a file, computed once and shared by the two launch forms."""
    memo = {}

    def get(name):
        if name not in memo:
            o = oracle.OracleModel(files[name], n_threads=16)
            rows = {}
            for toks, n_past, compared in plan():
                lo = o.eval(toks, n_past)
                if compared:
                    rows[n_past] = np.array(lo, dtype=np.float32)
                    rows[n_past].setflags(write=False)
            o.close()
            memo[name] = rows
        return memo[name]
    return get


@pytest.mark.parametrize("resident", [False, True], ids=["per-call", "resident"])
@pytest.mark.parametrize("name", FILES)
def test_single_tokens_are_bit_identical_to_the_oracle(pkg, files, rows_of, monkeypatch, name, resident):
    rows = rows_of(name)
    if not resident:
        monkeypatch.setenv("BIOGPT_HIP_RESIDENT", "0")      # options are read when the context is created
    g = pkg.BiogptModel.load(files[name])
    if not resident:
        monkeypatch.delenv("BIOGPT_HIP_RESIDENT")
    try:
        assert g.xpipe_state() == 1
        what = "%s, %s" % (name, "resident launch" if resident else "one launch per call")
        wanted = RESIDENT_CONTEXTS if resident else CONTEXTS
        seen = 0
        for toks, n_past, compared in plan():
            if n_past > wanted[-1]:
                break
            got = g.eval(toks, n_past)
            if not compared or n_past not in wanted:
                continue
            ref = rows[n_past]
            seen += 1
            print("%s at %d: max |diff| %.3e, %d elements differ" % (what, n_past, float(np.abs(got - ref).max()), int((got != ref).sum())))
            assert np.isfinite(got).all() and np.isfinite(ref).all(), "%s at %d: output not finite" % (what, n_past)
            assert (got == ref).all(), "%s at %d: not bit-identical to the oracle, max |diff| %.3e in %d elements" % (
                what, n_past, float(np.abs(got - ref).max()), int((got != ref).sum()))
        assert seen == len(wanted)
        assert g.xpipe_state() == 1, "the persistent launch was abandoned on the way"
    finally:
        g.close()


def test_greedy_continuation_across_a_launch_boundary(pkg, oracle, files):
    """generate_greedy (several tokens per launch) from 60 keys to 99 on the order-sensitive file: the 64-key launch, then the 128-key one; ids equal to the oracle's."""
    name = "ranged.q4_0"
    g = pkg.BiogptModel.load(files[name])
    try:
        assert g.xpipe_state() == 1
        prompt = tokens(1001, N_PROMPT)
        ids, _ = g.generate_greedy(prompt, N_GEN)
        o = oracle.OracleModel(files[name], n_threads=16)
        ref, _ = o.generate_greedy(prompt, N_GEN)
        o.close()
        first = next((k for k in range(min(len(ids), len(ref))) if ids[k] != ref[k]), min(len(ids), len(ref)))
        assert len(ref) == N_GEN and list(ids) == list(ref), "%s: %d ids, the oracle %d; they differ from token %d on" % (name, len(ids), len(ref), first)
        assert g.xpipe_state() == 1, "the persistent launch was abandoned on the way"
    finally:
        g.close()
