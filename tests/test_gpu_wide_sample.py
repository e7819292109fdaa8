"""Whole-vocabulary sampling (biogpt_hip_generate_sample_wide, kernels_wide_sample.hip.h) on the GPU: the kernel against its restatement
(wide_sample_ref.sample_wide: ids, candidate counts and generator states) on rows of every awkward kind and width, wherever no decision lies within MARGIN
of a border -- the rule and the constant of test_gpu_sample.py; generation against the oracle loop; samplers that sample_rows_kernel serves give the plain
call's result bit for bit; a sequence depends on nothing but its row, sampler and generator; the eager, captured, column-per-XCD and prefix paths agree;
an EOS ends its sequence alone; the context is left alone; bad arguments are refused."""
import ctypes

import numpy as np
import pytest

import wide_sample_ref as ref
from wide_sample_ref import S

pytestmark = pytest.mark.gpu

KW = dict(n_vocab=42384, n_layer=3, n_head=16, n_positions=1024, d_ff=4096, d_model=1024, n_merges=40000)
MARGIN = 1e-9          # two summation orders of <= 42 384 doubles summing to <= 1 differ by <= 4.7e-12, exp() by ~1e-15: this separates rounding from a wrong choice
NUCLEUS = S(0, 0.9, 0.9)
ANCESTRAL = S(0, 1.0, 1.0)
MIN_P = S(0, 1.0, 1.5, 0.05)


def prompt_of(n, seed):
    rng = np.random.default_rng(seed)
    return [2] + [int(v) for v in rng.integers(4, KW["n_vocab"], n - 1)]


def lists(ids):
    return [[int(t) for t in s] for s in ids]


@pytest.fixture(scope="module")
def files(pkg, tmp_path_factory):
    d = tmp_path_factory.mktemp("wide")
    f32 = str(d / "f32.bin")
    pkg.write_synthetic(f32, **KW)
    out = {"f32": f32}
    for name in ("q4_0", "q8_0"):
        out[name] = str(d / (name + ".bin"))
        pkg.quantize_file(f32, out[name], name)
    return out


@pytest.fixture(scope="module")
def model(pkg, files):
    g = pkg.BiogptModel.load(files["q4_0"])
    yield g
    g.close()


# ---- 1. the kernel against the restatement ----

WIDTHS = [42384, 42383, 1021, 257, 70]
SAMPLERS = [S(0, 0.9, 1.0), S(0, 1.0, 1.0), S(0, 1.0, 1.5, 0.05), S(1000, 0.95, 0.9), S(65, 1.0, 2.0), S(0, 0.5, 0.7, 0.3)]
STEPS = 3


def clamp(sampler, nv):
    return (min(sampler[0], nv),) + sampler[1:]


def kernel_case(nv, si):
    """The rows, the sampler and the first generator seed of case (width, sampler)."""
    return ref.row_kinds(nv, nv * 31 + si), clamp(SAMPLERS[si], nv), 900 + 50 * si


def restated_steps(rows, sampler, seed0, steps=STEPS):
    """steps draws from every row, row r from its own std::mt19937(seed0 + r).  Returns ([step][row] ids, [step][row] n_cand, final states, smallest margin)."""
    states = np.stack([ref.mt_seed(seed0 + r) for r in range(rows.shape[0])])
    ids, cand, margin = [], [], np.inf
    for _ in range(steps):
        out = [ref.sample_wide(rows[r], sampler, ref.StateRng(states[r])) for r in range(rows.shape[0])]
        ids.append([o[0] for o in out])
        cand.append([o[1] for o in out])
        margin = min([margin] + [o[2] for o in out])
    return ids, cand, states, margin


@pytest.mark.parametrize("si", range(len(SAMPLERS)), ids=["k%d_p%g_m%g_t%g" % s for s in SAMPLERS])
@pytest.mark.parametrize("nv", WIDTHS)
def test_kernel_equals_restatement(pkg, nv, si):
    rows, sampler, seed0 = kernel_case(nv, si)
    want_ids, want_cand, want_states, margin = restated_steps(rows, sampler, seed0)
    print("width %d sampler %s: smallest margin %.3g" % (nv, sampler, margin))
    assert margin >= MARGIN, "fixture problem: a decision lies %.3g from a border -- the case cannot tell the device's sums from a wrong choice" % margin
    states = np.stack([ref.mt_seed(seed0 + r) for r in range(rows.shape[0])])
    for step in range(STEPS):
        ids, cand = pkg.sample_wide_rows(rows, sampler, states)
        assert [int(t) for t in ids] == want_ids[step], step
        assert [int(c) for c in cand] == want_cand[step], step
    for r in range(rows.shape[0]):
        assert np.array_equal(ref.canonical_state(states[r]), ref.canonical_state(want_states[r])), r
    # what the rows are there for: a row without a finite value draws nothing, a dominant entry under a cut neither, the others do
    drew = [int(want_states[r][624]) != 624 for r in range(rows.shape[0])]
    assert not drew[20] and not drew[21] and any(drew[:14]) and drew[14]
    assert want_cand[0][20] == want_cand[0][21] == 0
    if sampler[1] < 1.0:
        assert want_cand[0][15] == 1 and not drew[15]


# ---- 2. the generator's block runs out on the way ----

def test_kernel_regenerates_the_generator_block(pkg):
    rng = np.random.default_rng(5)
    rows = (rng.standard_normal((1, 2048)) * 2.5).astype(np.float32)
    sampler = S(0, 1.0, 2.0)
    want_ids, _, want_states, margin = restated_steps(rows, sampler, 77, steps=330)
    assert margin >= MARGIN, "fixture problem: a draw lies %.3g from a border" % margin
    states = np.stack([ref.mt_seed(77)])
    got = [int(pkg.sample_wide_rows(rows, sampler, states)[0][0]) for _ in range(330)]
    assert got == [w[0] for w in want_ids]
    assert len(set(got)) > 100
    assert np.array_equal(ref.canonical_state(states[0]), ref.canonical_state(want_states[0]))


# ---- 3. against the oracle loop ----

ORACLE_PROMPTS = [prompt_of(5, 11), prompt_of(13, 12)]
ORACLE_SEEDS = [1101, 1202, 1303, 1404]     # sequence r = prompt r // 2, sample r % 2; chosen on the CPU: every margin below is >= 1.2e-8
N_PREDICT = 8


@pytest.mark.parametrize("sampler", [NUCLEUS, MIN_P], ids=["nucleus", "min_p"])
@pytest.mark.parametrize("nb", [1, 8])
@pytest.mark.parametrize("name", ["q4_0", "q8_0"])
def test_wide_sample_against_oracle_loop(pkg, oracle, files, name, nb, sampler):
    want = []
    for r, seed in enumerate(ORACLE_SEEDS):
        o = oracle.OracleModel(files[name], n_threads=16)
        ids, margin = ref.reference_loop(o, ORACLE_PROMPTS[r // 2], nb, N_PREDICT, sampler, seed)
        print("%s n_batch=%d %s sequence %d: smallest margin %.3g" % (name, nb, sampler, r, margin))
        assert margin >= MARGIN, "fixture problem: a decision of sequence %d lies %.3g from a border" % (r, margin)
        want.append(ids)
    assert len(set(t for ids in want for t in ids)) > 24, "fixture problem: the samples do not spread"
    g = pkg.BiogptModel.load(files[name])
    got, _ = g.generate_sample(ORACLE_PROMPTS, N_PREDICT, n_samples=2, seeds=ORACLE_SEEDS, eos_id=-1, n_batch=nb, sampler=sampler)
    g.close()
    assert lists(got) == want


# ---- 4. a sampler that sample_rows_kernel serves is the plain call ----

@pytest.mark.parametrize("top_k,top_p,temp", [(40, 0.9, 0.9), (64, 1.0, 1.0)])
def test_narrow_samplers_are_the_plain_call(pkg, model, top_k, top_p, temp):
    prompts = [prompt_of(11, 60), prompt_of(6, 61), prompt_of(19, 62)]
    kw = dict(n_samples=2, seed=70, n_batch=8)
    plain, _ = model.generate_sample(prompts, 24, top_k=top_k, top_p=top_p, temp=temp, **kw)
    wide, _ = model.generate_sample(prompts, 24, sampler=pkg.sampler(top_k=top_k, top_p=top_p, min_p=0.0, temp=temp), **kw)
    assert lists(wide) == lists(plain)
    eos = int(plain[0][2])
    plain_e, _ = model.generate_sample(prompts, 24, top_k=top_k, top_p=top_p, temp=temp, eos_id=eos, **kw)
    wide_e, _ = model.generate_sample(prompts, 24, sampler=(top_k, top_p, 0.0, temp), eos_id=eos, **kw)
    assert lists(wide_e) == lists(plain_e) and len(plain_e[0]) <= 3
    # and the wide kernel is another route: with min-p, or one candidate more, the ids part from the plain call's
    other, _ = model.generate_sample(prompts, 24, sampler=(0, top_p, 0.0, temp), **kw)
    assert lists(other) != lists(plain)


# ---- 5. determinism and independence ----

def test_a_sequence_depends_on_its_row_sampler_and_generator_alone(pkg, model):
    prompts = [prompt_of(n, 20 + n) for n in (7, 19, 12, 33, 5)]
    seeds = [5, 6, 7, 8, 9]
    for sampler in (NUCLEUS, MIN_P):
        batch, _ = model.generate_sample(prompts, 16, seeds=seeds, sampler=sampler)
        again, _ = model.generate_sample(prompts, 16, seeds=seeds, sampler=sampler)
        assert lists(again) == lists(batch)
        for r in (0, 3):
            alone, _ = model.generate_sample(prompts[r], 16, seeds=[seeds[r]], sampler=sampler)
            assert lists(alone)[0] == lists(batch)[r], r
        other, _ = model.generate_sample(prompts, 16, seeds=[s + 100 for s in seeds], sampler=sampler)
        assert all(a != b for a, b in zip(lists(other), lists(batch)))
    prompt = prompt_of(13, 53)
    shared, _ = model.generate_sample([prompt], 16, n_samples=4, seeds=[31, 32, 33, 34], sampler=ANCESTRAL)
    repeated, _ = model.generate_sample([prompt] * 4, 16, n_samples=1, seeds=[31, 32, 33, 34], sampler=ANCESTRAL)
    assert lists(shared) == lists(repeated) and len(set(tuple(s) for s in lists(shared))) == 4


# ---- 6. the paths agree ----

def test_paths_agree(pkg, files, monkeypatch):
    g = pkg.BiogptModel.load(files["q4_0"])
    cases = {n: [prompt_of(8 + 2 * i, 90 + n + i) for i in range(n)] for n in (1, 3, 8, 12)}
    runs = {}
    for label, env in (("default", {}), ("repeat", {}), ("xcols off", {"BIOGPT_HIP_XCOLS": "0"}), ("no graph", {"BIOGPT_HIP_NO_GRAPH": "1"})):
        for k in ("BIOGPT_HIP_XCOLS", "BIOGPT_HIP_NO_GRAPH"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        g.refresh_options()
        for n, prompts in cases.items():
            ids, _ = g.generate_sample(prompts, 24, seed=7, n_batch=8, sampler=NUCLEUS)
            runs.setdefault(n, []).append((label, lists(ids)))
    for k in ("BIOGPT_HIP_XCOLS", "BIOGPT_HIP_NO_GRAPH"):
        monkeypatch.delenv(k, raising=False)
    g.refresh_options()
    for n, rs in runs.items():
        for label, r in rs[1:]:
            assert r == rs[0][1], (n, label)
    # behind a prefix: the shared rows copied into the columns' slots (6 columns: column-per-XCD launches) and read in place (12 columns)
    prefix = prompt_of(21, 300)
    for cols, n_samples, path in ((6, 2, 1), (12, 3, 0)):
        suffixes = [prompt_of(3 + i, 310 + i)[1:] for i in range(cols // n_samples)]
        for sampler in (NUCLEUS, MIN_P):
            got, _ = g.generate_sample(suffixes, 20, n_samples=n_samples, seed=11, prefix=prefix, sampler=sampler)
            st = g.prefix_stats()
            want, _ = g.generate_sample([prefix + s for s in suffixes], 20, n_samples=n_samples, seed=11, sampler=sampler)
            assert lists(got) == lists(want), (cols, sampler)
            assert st["path"] == path and st["n_shared"] == 16 and st["columns"] == cols, st
    g.close()


# ---- 7. EOS; the context is left alone ----

def test_eos_ends_its_sequence_alone(pkg, model):
    prompts = [prompt_of(11, 60), prompt_of(6, 61)]
    seeds = [71, 72, 73, 74]
    free, _ = model.generate_sample(prompts, 40, n_samples=2, seeds=seeds, sampler=MIN_P)
    eos = int(free[0][2])
    assert eos not in [int(t) for t in free[0][:2]]
    flat = np.ascontiguousarray(np.concatenate([np.asarray(p, dtype=np.int32) for p in prompts]))
    lens = np.asarray([len(p) for p in prompts], dtype=np.int32)
    sd = np.asarray(seeds, dtype=np.uint32)
    sp = pkg.sampler(*MIN_P)
    out, ol, secs = np.zeros((4, 40), dtype=np.int32), np.zeros(4, dtype=np.int32), ctypes.c_double(0.0)
    assert pkg.lib().biogpt_hip_generate_sample_wide(model._h, flat.ctypes.data, lens.ctypes.data, 2, 2, 8, 40, ctypes.byref(sp), sd.ctypes.data, eos, out.ctypes.data,
                                                     ol.ctypes.data, ctypes.byref(secs)) == 40, pkg._err()
    assert int(ol[0]) == 3 and list(out[0][:3]) == [int(t) for t in free[0][:3]] and (out[0][3:] == -1).all()
    for r in range(1, 4):
        f = [int(t) for t in free[r]]
        want = f[:f.index(eos) + 1] if eos in f else f
        assert list(out[r][:ol[r]]) == want and (out[r][ol[r]:] == -1).all(), r
    assert any(int(ol[r]) == 40 for r in range(1, 4))      # a sequence that never draws it runs its full length
    one, _ = model.generate_sample(prompts[0], 40, seeds=[71], eos_id=eos, sampler=MIN_P)      # every sequence ends early: the host stops enqueueing
    assert lists(one)[0] == [int(t) for t in free[0][:3]]


def test_context_cache_untouched_and_eval_follows(pkg, files):
    g = pkg.BiogptModel.load(files["q4_0"])
    h = pkg.BiogptModel.load(files["q4_0"])
    ctx_toks = prompt_of(9, 7)
    row = g.eval(ctx_toks, 0)
    h.eval(ctx_toks, 0)
    D = KW["d_model"]
    k0, v0 = g.read_kv(0, 0, 3 * KW["n_positions"] * D), g.read_kv(1, 0, 3 * KW["n_positions"] * D)
    ids, _ = g.generate_sample([prompt_of(17, 8)], 12, n_samples=4, seed=3, sampler=NUCLEUS)
    assert len(ids) == 4 and all(len(s) == 12 for s in ids)
    assert np.array_equal(g.read_kv(0, 0, k0.size), k0) and np.array_equal(g.read_kv(1, 0, v0.size), v0)
    assert np.array_equal(g.read_logits(), row)
    assert np.array_equal(g.eval([123], len(ctx_toks)), h.eval([123], len(ctx_toks)))
    g.close()
    h.close()


# ---- 8. refusals ----

def test_float_files_and_bad_arguments_fail(pkg, files, tiny_models, model):
    for path in (files["f32"], tiny_models["f16"]):
        g = pkg.BiogptModel.load(path)
        with pytest.raises(pkg.BiogptError, match="fast chain"):
            g.generate_sample([2, 5, 7], 4, sampler=NUCLEUS)
        g.close()
    V = KW["n_vocab"]
    for kw, msg in ((dict(top_k=-1), "top_k"), (dict(top_k=V + 1), "top_k"), (dict(min_p=1.0), "min_p"), (dict(min_p=-0.5), "min_p"), (dict(min_p=float("nan")), "min_p"),
                    (dict(temp=0.0), "temp"), (dict(temp=float("nan")), "temp"), (dict(top_p=float("inf")), "top_p")):
        with pytest.raises(pkg.BiogptError, match=msg):
            model.generate_sample([2, 5, 7], 4, sampler=pkg.sampler(**kw))
    for kw, msg in ((dict(eos_id=V), "eos_id"), (dict(n_batch=0), "n_batch"), (dict(n_samples=0), "n_samples"), (dict(n_samples=513), "n_samples")):
        with pytest.raises(pkg.BiogptError, match=msg):
            model.generate_sample([2, 5, 7], 4, sampler=NUCLEUS, **kw)
    for kw in (dict(top_k=50), dict(top_p=0.5), dict(temp=1.0)):
        with pytest.raises(pkg.BiogptError, match="defaults"):
            model.generate_sample([2, 5, 7], 4, sampler=NUCLEUS, **kw)
    trie = pkg.Trie.build([[5, 7]], V)
    for kw, word in ((dict(logprobs=2), "logprobs"), (dict(trie=trie, eos_id=2), "trie"), (dict(repetition_penalty=1.3), "rules"), (dict(suppress_tokens=[9]), "rules")):
        with pytest.raises(ValueError, match="sampler= cannot be combined with .*" + word):
            model.generate_sample([2, 5, 7], 4, sampler=NUCLEUS, **kw)
    trie.close()
    with pytest.raises(pkg.BiogptError, match="empty prompt"):
        model.generate_sample([[2, 5], []], 4, sampler=NUCLEUS)
    assert model.generate_sample([2] * KW["n_positions"], 4, sampler=NUCLEUS)[0] == []
    ids, _ = model.generate_sample([2, 5, 7], 4, n_samples=3, sampler=pkg.sampler(top_k=V, top_p=1.5))      # still usable; top_k = n_vocab, top_p >= 1: no cut
    assert len(ids) == 3 and all(len(i) == 4 for i in ids)
