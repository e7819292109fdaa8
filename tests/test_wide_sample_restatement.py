"""The wide sampler without a GPU: its Python restatement (wide_sample_ref.sample_wide) equals oracle/sampler.py where the reference has a say (min_p = 0),
does what the contract says where it has none (min-p on rows with known probabilities, rows without a finite value), the generator in its 625-word form is
std::mt19937, and the new entry points are exported, bound and refuse bad arguments before any HIP call."""
import ctypes
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import sample_ref
import wide_sample_ref as ref
from oracle import sampler as oracle_sampler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("biogpt_hip_generate_sample_wide", "biogpt_hip_generate_sample_wide_prefix", "biogpt_hip_sample_wide_rows_device", "biogpt_hip_sample_wide_rows_bench")
NV = 42384


@pytest.mark.parametrize("k", [1, 40, 65, 1000, NV])
@pytest.mark.parametrize("top_p,temp", [(0.9, 0.9), (1.0, 1.0)])
def test_restatement_equals_the_oracle_without_min_p(k, top_p, temp):
    """Random rows, ONE generator carried across them on either side: the ids are the oracle's, and so is what the generators give next (a draw taken with
    one candidate left, or not taken with two, would shift it)."""
    rng = np.random.default_rng(k * 17 + int(temp * 10))
    rows = (rng.standard_normal((3, NV)) * 2.5).astype(np.float32)
    rows[2] = np.round(rows[2] * 2.0) / 2.0
    a, b = oracle_sampler.Mt19937(5), oracle_sampler.Mt19937(5)
    for row in rows:
        want = oracle_sampler.sample_top_k_top_p(row, k, top_p, temp, a)
        got, n, margin = ref.sample_wide(row, (k, top_p, 0.0, temp), b)
        assert got == want
        assert 1 <= n <= k and margin > 0.0
    assert [a() for _ in range(4)] == [b() for _ in range(4)]
    # top_k = 0 is the whole row
    a, b = oracle_sampler.Mt19937(6), oracle_sampler.Mt19937(6)
    assert ref.sample_wide(rows[0], (0, top_p, 0.0, temp), a)[0] == ref.sample_wide(rows[0], (NV, top_p, 0.0, temp), b)[0]


@pytest.mark.parametrize("k,top_p,temp", [(40, 0.9, 0.9), (1000, 0.95, 1.3), (5000, 1.0, 1.0)])
def test_margin_without_min_p_is_sample_ref_s(k, top_p, temp):
    """The margin extends sample_ref.decision_margin: without min-p it is that function's value (the same doubles, summed in the same order)."""
    rng = np.random.default_rng(k)
    rows = (rng.standard_normal((4, 5000)) * 2.5).astype(np.float32)
    gen = sample_ref.RecordingRng(oracle_sampler.Mt19937(9))
    for row in rows:
        before = len(gen.out)
        _, _, margin = ref.sample_wide(row, (k, top_p, 0.0, temp), gen)
        assert margin == sample_ref.decision_margin(row, k, top_p, temp, gen.out[before:])


def logits_of(probs):
    return np.log(np.asarray(probs, dtype=np.float64)).astype(np.float32)


class FixedRng:
    """Two outputs that make generate_canonical_53 return u (to 2^-32)."""

    def __init__(self, u):
        self.out = [0, int(u * 4294967296.0)]
        self.taken = 0

    def __call__(self):
        self.taken += 1
        return self.out.pop(0)


def test_min_p_on_rows_with_known_probabilities():
    probs = [0.4, 0.3, 0.15, 0.1, 0.05]      # ratios to the best: 1, 0.75, 0.375, 0.25, 0.125
    row = logits_of(probs)[[3, 0, 4, 2, 1]]  # ids: 1 -> 0.4, 4 -> 0.3, 3 -> 0.15, 0 -> 0.1, 2 -> 0.05
    by_rank = [1, 4, 3, 0, 2]
    for min_p, n_want in ((0.0, 5), (0.1, 5), (0.2, 4), (0.3, 3), (0.5, 2), (0.8, 1)):
        r = FixedRng(0.999)                  # the last candidate left
        got, n, margin = ref.sample_wide(row, (0, 1.0, min_p, 1.0), r)
        assert (n, got) == (n_want, by_rank[n_want - 1]), min_p
        assert r.taken == (2 if n_want > 1 else 0)
        if min_p > 0.0:
            want_margin = min(abs(p / 0.4 - min_p) for p in probs[:min(n_want + 1, 5)])
            assert margin <= want_margin + 1e-7 and margin > 0.01
    # the kept candidates are drawn in proportion: 0.4 / 0.7 and 0.3 / 0.7 with min_p = 0.5
    assert ref.sample_wide(row, (0, 1.0, 0.5, 1.0), FixedRng(0.57))[0] == 1
    assert ref.sample_wide(row, (0, 1.0, 0.5, 1.0), FixedRng(0.58))[0] == 4
    # behind the top-p cut: 0.4 + 0.3 + 0.15 >= 0.8 leaves three, of which min_p = 0.5 keeps two; top_k in front of both
    assert ref.sample_wide(row, (0, 0.8, 0.0, 1.0), FixedRng(0.999))[:2] == (3, 3)
    assert ref.sample_wide(row, (0, 0.8, 0.5, 1.0), FixedRng(0.999))[:2] == (4, 2)
    assert ref.sample_wide(row, (1, 0.8, 0.5, 1.0), FixedRng(0.999))[:2] == (1, 1)
    # the temperature acts before min-p: at temp 2 the ratios are their square roots (0.866, 0.612, 0.5, 0.354)
    assert ref.sample_wide(row, (0, 1.0, 0.55, 2.0), FixedRng(0.999))[1] == 3


def test_min_p_with_a_tie_across_the_cut():
    """Equal values have equal probabilities: min-p keeps all of them or none, and among them the lower id comes first."""
    row = logits_of([0.3, 0.1, 0.1, 0.3, 0.1, 0.1])      # ranks: ids 0, 3 (0.3), then 1, 2, 4, 5 (ratio 1 / 3)
    assert ref.sample_wide(row, (0, 1.0, 0.3, 1.0), FixedRng(0.999))[:2] == (5, 6)
    assert ref.sample_wide(row, (0, 1.0, 0.4, 1.0), FixedRng(0.999))[:2] == (3, 2)
    assert ref.sample_wide(row, (0, 1.0, 0.4, 1.0), FixedRng(0.25))[0] == 0
    # a top-p cut inside the tie (0.3 + 0.3 + 0.1 + 0.1 >= 0.75) ends at the tie's second id; top_k = 3 ends at its first
    assert ref.sample_wide(row, (0, 0.75, 0.0, 1.0), FixedRng(0.999))[:2] == (2, 4)
    assert ref.sample_wide(row, (3, 1.0, 0.0, 1.0), FixedRng(0.999))[:2] == (1, 3)
    assert ref.sample_wide(row, (0, 0.75, 0.3, 1.0), FixedRng(0.999))[:2] == (2, 4)


def test_rows_without_a_finite_value_give_id_0_and_no_draw():
    for fill in (-np.inf, np.nan):
        r = FixedRng(0.5)
        assert ref.sample_wide(np.full(9, fill, dtype=np.float32), (0, 0.9, 0.1, 1.0), r) == (0, 0, math.inf)
        assert r.taken == 0
    # NaNs are never candidates; -inf entries are, with probability 0
    row = np.array([np.nan, 1.0, -np.inf, np.nan, 1.0], dtype=np.float32)
    assert ref.sample_wide(row, (0, 1.0, 0.0, 1.0), FixedRng(0.75))[:2] == (4, 3)
    assert ref.sample_wide(row, (0, 1.0, 0.01, 1.0), FixedRng(0.25))[:2] == (1, 2)
    one = np.array([np.nan, -np.inf, 3.0], dtype=np.float32)
    r = FixedRng(0.5)
    assert ref.sample_wide(one, (0, 0.9, 0.0, 1.0), r)[:2] == (2, 1) and r.taken == 0


def test_state_generator_is_mt19937():
    st = ref.mt_seed(5489)
    a, b = ref.StateRng(st), oracle_sampler.Mt19937(5489)
    assert [a() for _ in range(1300)] == [b() for _ in range(1300)]
    last = [a() for _ in range(8700)][-1]
    assert last == 4123659995      # the 10000th output of std::mt19937 (ISO C++ [rand.predef])
    run_out = ref.mt_seed(3)
    assert int(ref.canonical_state(run_out)[624]) == 0 and int(run_out[624]) == 624


def test_wide_symbols_exported_and_bound(pkg):
    hdr = open(os.path.join(ROOT, "include", "biogpt_hip.h")).read()
    bound = {name for name, _, _ in pkg.SYMBOLS}
    raw = ctypes.CDLL(pkg.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in bound, name
        assert getattr(raw, name) is not None
    assert "biogpt_hip_sampler" in hdr
    sp = pkg.sampler()
    assert (sp.top_k, sp.top_p, sp.min_p, sp.temp) == (0, 1.0, 0.0, 1.0) and ctypes.sizeof(sp) == 32
    assert callable(pkg.sample_wide_rows)


BAD_SAMPLERS = [(dict(top_k=-1), "top_k"), (dict(min_p=1.0), "min_p"), (dict(min_p=-0.1), "min_p"), (dict(min_p=float("nan")), "min_p"),
                (dict(temp=0.0), "temp"), (dict(temp=float("nan")), "temp"), (dict(temp=float("inf")), "temp"), (dict(top_p=float("inf")), "top_p"),
                (dict(top_p=float("nan")), "top_p")]


def test_generate_wide_refuses_before_any_hip_call(pkg):
    L = pkg.lib()
    prompt, lens = np.array([2, 5, 7], dtype=np.int32), np.array([3], dtype=np.int32)
    seeds = np.array([1, 2], dtype=np.uint32)
    ids, ol, secs = np.zeros((2, 8), dtype=np.int32), np.zeros(2, dtype=np.int32), ctypes.c_double(0.0)

    def plain(sp):
        return L.biogpt_hip_generate_sample_wide(None, prompt.ctypes.data, lens.ctypes.data, 1, 2, 8, 8, sp, seeds.ctypes.data, -1, ids.ctypes.data, ol.ctypes.data,
                                                 ctypes.byref(secs))

    def prefixed(sp, pre=prompt.ctypes.data):
        return L.biogpt_hip_generate_sample_wide_prefix(None, pre, 3, prompt.ctypes.data, lens.ctypes.data, 1, 2, 8, 8, sp, seeds.ctypes.data, -1, ids.ctypes.data,
                                                        ol.ctypes.data, ctypes.byref(secs))

    good = pkg.sampler(top_p=0.9)
    assert plain(ctypes.byref(good)) == -1 and "null context" in pkg._err()
    assert prefixed(ctypes.byref(good)) == -1 and "null context" in pkg._err()
    assert plain(None) == -1 and "sampler" in pkg._err()
    for kw, word in BAD_SAMPLERS:
        sp = pkg.sampler(**kw)
        assert plain(ctypes.byref(sp)) == -1 and word in pkg._err(), kw


def test_rows_entries_refuse_before_any_hip_call(pkg):
    L = pkg.lib()
    rows = np.zeros((2, 70), dtype=np.float32)
    st = np.stack([ref.mt_seed(1), ref.mt_seed(2)])
    ids, nc, secs = np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.int32), np.zeros(4, dtype=np.float64)

    def device(sp, n_rows=2, nv=70, rows_p=rows.ctypes.data, st_p=st.ctypes.data, ids_p=ids.ctypes.data):
        return L.biogpt_hip_sample_wide_rows_device(0, rows_p, n_rows, nv, ctypes.byref(sp), st_p, ids_p, nc.ctypes.data)

    def bench(sp, which=0, reps=2, secs_p=secs.ctypes.data):
        return L.biogpt_hip_sample_wide_rows_bench(0, rows.ctypes.data, 2, 70, ctypes.byref(sp), st.ctypes.data, which, reps, secs_p)

    for kw, word in BAD_SAMPLERS + [(dict(top_k=71), "top_k")]:
        assert device(pkg.sampler(**kw)) == -1 and word in pkg._err(), kw
        assert bench(pkg.sampler(**kw)) == -1 and word in pkg._err(), kw
    good = pkg.sampler(top_p=0.9)
    assert device(good, n_rows=0) == -1 and device(good, n_rows=4097) == -1 and "n_rows" in pkg._err()
    assert device(good, rows_p=None) == -1 and device(good, st_p=None) == -1 and device(good, ids_p=None) == -1
    assert L.biogpt_hip_sample_wide_rows_device(0, rows.ctypes.data, 2, 70, None, st.ctypes.data, ids.ctypes.data, nc.ctypes.data) == -1
    bad = st.copy()
    bad[1, 624] = 625
    assert device(good, st_p=bad.ctypes.data) == -1 and "generator index" in pkg._err()
    assert bench(good, reps=0) == -1 and bench(good, reps=10001) == -1 and "reps" in pkg._err()
    assert bench(good, which=2) == -1 and "which" in pkg._err()
    assert bench(good, which=1) == -1 and "sample_rows_kernel" in pkg._err()      # top_k 0 is not the narrow kernel's
    assert bench(pkg.sampler(top_k=40, min_p=0.1), which=1) == -1
    assert bench(good, secs_p=None) == -1


def test_sampler_keyword_routes_and_refuses(pkg, monkeypatch):
    """sampler= goes to the wide entry points (behind a prefix: the prefix form), carries top_k / top_p / temp itself and combines with neither logprobs nor
    rules nor a trie; without it the call is what it was."""
    called = []

    class Lib:
        def __getattr__(self, name):
            def fn(*args):
                called.append(name)
                return 0
            return fn

    monkeypatch.setattr(pkg, "lib", lambda: Lib())
    m = pkg.BiogptModel.__new__(pkg.BiogptModel)
    m._h = None
    sp = pkg.sampler(top_p=0.9)
    assert m.generate_sample([[2, 5]], 4, sampler=sp)[0] == [] and called == ["biogpt_hip_generate_sample_wide"]
    assert m.generate_sample([[2, 5]], 4, sampler=(0, 0.9, 0.0, 1.0), n_samples=2, seed=3, eos_id=2, n_batch=1)[0] == [] and called[-1] == "biogpt_hip_generate_sample_wide"
    assert m.generate_sample([[2, 5]], 4, sampler=sp, prefix=[2, 3])[0] == [] and called[-1] == "biogpt_hip_generate_sample_wide_prefix"
    assert m.generate_sample([[2, 5]], 4, sampler=None)[0] == [] and called[-1] == "biogpt_hip_generate_sample_rules"
    n = len(called)
    for kw in (dict(top_k=50), dict(top_p=0.8), dict(temp=1.0)):
        with pytest.raises(pkg.BiogptError, match="defaults"):
            m.generate_sample([[2, 5]], 4, sampler=sp, **kw)
    for kw, word in ((dict(logprobs=2), "logprobs"), (dict(trie=object()), "trie"), (dict(repetition_penalty=1.2), "rules"), (dict(no_repeat_ngram_size=2), "rules"),
                     (dict(min_new_tokens=1), "rules"), (dict(suppress_tokens=[5]), "rules")):
        with pytest.raises(ValueError, match="sampler= cannot be combined with .*" + word):
            m.generate_sample([[2, 5]], 4, sampler=sp, **kw)
    assert len(called) == n


def test_wide_kernel_uses_no_scratch(pkg, tmp_path):
    """sample_wide_rows_kernel: the kernel descriptor in obj/engine.o, read as test_sample_capi.py reads the sampler's."""
    llvm = "/opt/rocm/lib/llvm/bin"
    if not (os.path.exists(llvm + "/clang-offload-bundler") and shutil.which("objcopy")):
        pytest.skip("no clang-offload-bundler / objcopy in this image")
    pkg.build()
    path = os.path.join(ROOT, "biogpt.cpp_amd", "csrc", "obj", "engine.o")
    assert os.path.exists(path), path
    fat, co = str(tmp_path / "engine.fatbin"), str(tmp_path / "engine.co")
    subprocess.check_call(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", path, fat])
    subprocess.check_call([llvm + "/clang-offload-bundler", "--unbundle", "--type=o", "--input=" + fat, "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co])
    notes = subprocess.check_output([llvm + "/llvm-readelf", "--notes", co], text=True)
    name, seen = None, set()
    for line in notes.splitlines():
        m = re.match(r"\s+\.name:\s+(\S+)", line)
        if m:
            name = m.group(1)
        m = re.match(r"\s+\.private_segment_fixed_size:\s+(\d+)", line)
        if m and name and "sample_wide_rows_kernel" in name:
            assert int(m.group(1)) == 0, "%s uses %s bytes of scratch per lane" % (name, m.group(1))
            seen.add(name)
    assert len(seen) == 1, seen
