"""Sampled generation (biogpt_hip_generate_sample, kernels_sample.hip.h) on the GPU: the ids are the reference loop's (sample_ref: the oracle's logits
through oracle/sampler.py with std::mt19937(seed)) wherever no decision lies within MARGIN of a border; top_k = 1 is greedy decoding; a sequence
does not depend on its neighbours nor on how its prompt's K / V rows reached its slot; an EOS ends its sequence alone; the captured, eager and
column-per-XCD paths agree; the context's own K / V cache is left alone; the kernel itself against its host twin on rows of every awkward kind."""
import ctypes

import numpy as np
import pytest

import sample_ref

pytestmark = pytest.mark.gpu

KW = dict(n_vocab=42384, n_layer=3, n_head=16, n_positions=1024, d_ff=4096, d_model=1024, n_merges=40000)
SEED = 0x42494F47
MARGIN = 1e-9          # device exp() is good to ~1e-15 relative: this separates rounding from a wrong choice
DEFAULT = (40, 0.9, 0.9)
HOT = (40, 0.95, 6.0)


def prompt_of(n, seed):
    rng = np.random.default_rng(seed)
    return [2] + [int(v) for v in rng.integers(4, KW["n_vocab"], n - 1)]


@pytest.fixture(scope="module")
def files(pkg, tmp_path_factory):
    d = tmp_path_factory.mktemp("sample")
    f32 = str(d / "f32.bin")
    pkg.write_synthetic(f32, **KW)
    out = {"f32": f32}
    for name in ("q4_0", "q5_1", "q8_0"):
        out[name] = str(d / (name + ".bin"))
        pkg.quantize_file(f32, out[name], name)
    return out


@pytest.fixture(scope="module")
def base24(pkg, tmp_path_factory):
    d = tmp_path_factory.mktemp("sample24")
    f32, path = str(d / "f32.bin"), str(d / "q4_0.bin")
    pkg.write_synthetic(f32, seed=SEED, **dict(KW, n_layer=24))     # the seed of the bench
    pkg.quantize_file(f32, path, "q4_0")
    return path


# ---- 1. against the oracle loop ----

ORACLE_PROMPTS = [prompt_of(5, 11), prompt_of(13, 12)]
ORACLE_SEEDS = [101, 202, 303, 404]     # sequence r = prompt r // 2, sample r % 2
N_PREDICT = 16


@pytest.mark.parametrize("setting", [DEFAULT, HOT], ids=["default", "hot"])
@pytest.mark.parametrize("nb", [1, 8])
@pytest.mark.parametrize("name", ["q4_0", "q5_1", "q8_0"])
def test_sample_against_oracle_loop(pkg, oracle, files, name, nb, setting):
    top_k, top_p, temp = setting
    want = []
    for r, seed in enumerate(ORACLE_SEEDS):
        o = oracle.OracleModel(files[name], n_threads=16)
        ids, margin = sample_ref.reference_loop(o, ORACLE_PROMPTS[r // 2], nb, N_PREDICT, top_k, top_p, temp, seed)
        print("%s n_batch=%d %s sequence %d: smallest margin %.3g, %d distinct ids" % (name, nb, setting, r, margin, len(set(ids))))
        assert margin >= MARGIN, "fixture problem: a decision of sequence %d lies %.3g from a border -- the case cannot tell the device's exp() from a wrong choice" % (r, margin)
        if setting == HOT:
            assert len(set(ids)) > 3, "fixture problem: the hot setting does not spread the oracle's samples (sequence %d: %s)" % (r, ids)
        want.append(ids)
    g = pkg.BiogptModel.load(files[name])
    got, _ = g.generate_sample(ORACLE_PROMPTS, N_PREDICT, n_samples=2, top_k=top_k, top_p=top_p, temp=temp, seeds=ORACLE_SEEDS, eos_id=-1, n_batch=nb)
    g.close()
    assert len(got) == 4
    for r in range(4):
        assert list(got[r]) == want[r], (r, list(got[r]), want[r])


# ---- 2. top_k = 1: greedy decoding ----

def check_greedy_limit(pkg, path, prompts, n_predict):
    g = pkg.BiogptModel.load(path)
    want, _ = g.generate_greedy_batch(prompts, n_predict, n_batch=8)
    for seed in (0, 977):
        got, _ = g.generate_sample(prompts, n_predict, top_k=1, top_p=0.9, temp=0.9, seed=seed, n_batch=8)
        assert [list(s) for s in got] == [list(w) for w in want], seed
    g.close()


def test_top_k_1_is_greedy_3_layers(pkg, files):
    check_greedy_limit(pkg, files["q4_0"], [prompt_of(21, 1), prompt_of(9, 2), prompt_of(30, 3)], 24)


def test_top_k_1_is_greedy_24_layers(pkg, base24):
    check_greedy_limit(pkg, base24, [prompt_of(40, 2), prompt_of(17, 4)], 32)


# ---- 3. independence ----

def test_a_sequence_does_not_depend_on_its_batch(pkg, files):
    top_k, top_p, temp = HOT
    prompts = [prompt_of(n, 20 + n) for n in (7, 19, 12, 33, 5)]
    seeds = [5, 6, 7, 8, 9]
    g = pkg.BiogptModel.load(files["q4_0"])
    kw = dict(top_k=top_k, top_p=top_p, temp=temp, n_batch=8)
    batch, _ = g.generate_sample(prompts, 24, seeds=seeds, **kw)
    again, _ = g.generate_sample(prompts, 24, seeds=seeds, **kw)
    assert [list(s) for s in again] == [list(s) for s in batch]
    for r in range(5):
        alone, _ = g.generate_sample(prompts[r], 24, seeds=[seeds[r]], **kw)
        assert list(alone[0]) == list(batch[r]), r
    other, _ = g.generate_sample(prompts, 24, seeds=[s + 100 for s in seeds], **kw)
    assert all(list(a) != list(b) for a, b in zip(other, batch))
    g.close()


def test_shared_prompt_equals_the_prompt_repeated(pkg, files):
    top_k, top_p, temp = HOT
    g = pkg.BiogptModel.load(files["q5_1"])
    for n_prompt, nb in ((13, 8), (40, 8), (9, 1)):
        prompt = prompt_of(n_prompt, 40 + n_prompt)
        kw = dict(top_k=top_k, top_p=top_p, temp=temp, seeds=[31, 32, 33, 34], n_batch=nb)
        shared, _ = g.generate_sample([prompt], 20, n_samples=4, **kw)
        repeated, _ = g.generate_sample([prompt] * 4, 20, n_samples=1, **kw)
        assert [list(s) for s in shared] == [list(s) for s in repeated], (n_prompt, nb)
        assert len(set(tuple(s) for s in shared)) == 4
    # default seeds: seed + sequence index
    a, _ = g.generate_sample([prompt], 8, n_samples=3, seed=50)
    b, _ = g.generate_sample([prompt], 8, n_samples=3, seeds=[50, 51, 52])
    assert [list(s) for s in a] == [list(s) for s in b]
    g.close()


# ---- 4. EOS ----

def test_eos_ends_its_sequence_alone(pkg, files):
    top_k, top_p, temp = HOT
    prompts = [prompt_of(11, 60), prompt_of(6, 61)]
    kw = dict(n_samples=2, top_k=top_k, top_p=top_p, temp=temp, seeds=[71, 72, 73, 74], n_batch=8)
    g = pkg.BiogptModel.load(files["q4_0"])
    free, _ = g.generate_sample(prompts, 40, eos_id=-1, **kw)
    eos = int(free[0][2])
    assert eos not in [int(t) for t in free[0][:2]]
    L = pkg.lib()
    flat = np.ascontiguousarray(np.concatenate([np.asarray(p, dtype=np.int32) for p in prompts]))
    lens = np.asarray([len(p) for p in prompts], dtype=np.int32)
    sd = np.asarray(kw["seeds"], dtype=np.uint32)
    out, ol, secs = np.zeros((4, 40), dtype=np.int32), np.zeros(4, dtype=np.int32), ctypes.c_double(0.0)
    assert L.biogpt_hip_generate_sample(g._h, flat.ctypes.data, lens.ctypes.data, 2, 2, 8, 40, top_k, top_p, temp, sd.ctypes.data, eos, out.ctypes.data,
                                        ol.ctypes.data, ctypes.byref(secs)) == 40, pkg._err()
    assert int(ol[0]) == 3 and list(out[0][:3]) == [int(t) for t in free[0][:3]] and int(out[0][2]) == eos
    assert (out[0][3:] == -1).all()
    for r in range(1, 4):
        f = [int(t) for t in free[r]]
        want = f[:f.index(eos) + 1] if eos in f else f
        assert list(out[r][:ol[r]]) == want and (out[r][ol[r]:] == -1).all(), r
    assert any(int(ol[r]) == 40 for r in range(1, 4))      # a sequence that never draws it runs its full length
    # every sequence ends early: the host stops enqueueing (the result is the same either way)
    one, _ = g.generate_sample(prompts[0], 40, n_samples=1, top_k=top_k, top_p=top_p, temp=temp, seeds=[71], eos_id=eos, n_batch=8)
    assert [int(t) for t in one[0]] == [int(t) for t in free[0][:3]]
    g.close()


# ---- 5. the paths agree ----

def test_paths_agree(pkg, files, monkeypatch):
    top_k, top_p, temp = HOT
    g = pkg.BiogptModel.load(files["q4_0"])
    cases = {2: [prompt_of(30, 80), prompt_of(12, 81)], 5: [prompt_of(10 + 3 * i, 82 + i) for i in range(5)], 12: [prompt_of(8 + 2 * i, 90 + i) for i in range(12)]}
    runs = {}
    for label, env in (("default", {}), ("repeat", {}), ("xcols off", {"BIOGPT_HIP_XCOLS": "0"}), ("no graph", {"BIOGPT_HIP_NO_GRAPH": "1"})):
        for k in ("BIOGPT_HIP_XCOLS", "BIOGPT_HIP_NO_GRAPH"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        g.refresh_options()
        for n, prompts in cases.items():
            ids, _ = g.generate_sample(prompts, 40, top_k=top_k, top_p=top_p, temp=temp, seed=7, n_batch=8)
            runs.setdefault(n, []).append((label, [list(s) for s in ids]))
        # prompt + generation crossing 256 keys (3 samples of one prompt)
        ids, _ = g.generate_sample([prompt_of(240, 99)], 32, n_samples=3, top_k=top_k, top_p=top_p, temp=temp, seed=9, n_batch=8)
        runs.setdefault("256", []).append((label, [list(s) for s in ids]))
    g.close()
    for n, rs in runs.items():
        for label, r in rs[1:]:
            assert r == rs[0][1], (n, label)


# ---- 6. the context is left alone; arguments ----

def test_context_cache_untouched_and_eval_follows(pkg, files):
    g = pkg.BiogptModel.load(files["q4_0"])
    h = pkg.BiogptModel.load(files["q4_0"])
    ctx_toks = prompt_of(9, 7)
    row = g.eval(ctx_toks, 0)
    h.eval(ctx_toks, 0)
    D = KW["d_model"]
    k0, v0 = g.read_kv(0, 0, 3 * KW["n_positions"] * D), g.read_kv(1, 0, 3 * KW["n_positions"] * D)
    ids, _ = g.generate_sample([prompt_of(17, 8)], 12, n_samples=4, seed=3)
    assert len(ids) == 4
    assert np.array_equal(g.read_kv(0, 0, k0.size), k0) and np.array_equal(g.read_kv(1, 0, v0.size), v0)
    assert np.array_equal(g.read_logits(), row)
    nxt = [123]
    assert np.array_equal(g.eval(nxt, len(ctx_toks)), h.eval(nxt, len(ctx_toks)))
    g.close()
    h.close()


def test_float_files_and_bad_arguments_fail(pkg, files, tiny_models):
    for path in (files["f32"], tiny_models["f16"]):
        g = pkg.BiogptModel.load(path)
        with pytest.raises(pkg.BiogptError, match="fast chain"):
            g.generate_sample([2, 5, 7], 4)
        g.close()
    g = pkg.BiogptModel.load(files["q4_0"])
    for kw, msg in ((dict(top_k=0), "top_k"), (dict(top_k=65), "top_k"), (dict(temp=0.0), "temp"), (dict(temp=float("nan")), "temp"),
                    (dict(top_p=float("inf")), "top_p"), (dict(eos_id=KW["n_vocab"]), "eos_id"), (dict(eos_id=-2), "eos_id"), (dict(n_batch=0), "n_batch"),
                    (dict(n_samples=0), "n_samples"), (dict(n_samples=513), "n_samples")):
        with pytest.raises(pkg.BiogptError, match=msg):
            g.generate_sample([2, 5, 7], 4, **kw)
    with pytest.raises(pkg.BiogptError, match="empty prompt"):
        g.generate_sample([[2, 5], []], 4)
    with pytest.raises(pkg.BiogptError):
        g.generate_sample([2, 5, KW["n_vocab"]], 4)
    assert g.generate_sample([2] * KW["n_positions"], 4)[0] == []
    ids, _ = g.generate_sample([2, 5, 7], 4, n_samples=3, top_p=1.5)      # still usable; top_p >= 1: no cut
    assert len(ids) == 3 and all(len(i) == 4 for i in ids)
    g.close()


# ---- 7. the kernel on rows of every awkward kind, against its host twin ----

def host_rows(pkg, rows, top_k, top_p, temp, states):
    """The selection by stable arg-sort + biogpt_hip_sample_candidates_host, row r with states[r] (advanced in place)."""
    out = []
    for r, row in enumerate(rows):
        order = np.argsort(-row.astype(np.float64), kind="stable")[:top_k].astype(np.int32)
        vals = np.ascontiguousarray(row[order], dtype=np.float32)
        got = ctypes.c_int32(-1)
        assert pkg.lib().biogpt_hip_sample_candidates_host(vals.ctypes.data, order.ctypes.data, vals.size, top_p, temp, states[r].ctypes.data,
                                                           ctypes.byref(got)) == 0, pkg._err()
        out.append(int(got.value))
    return out


def device_rows(pkg, rows, top_k, top_p, temp, states):
    lg = np.ascontiguousarray(rows, dtype=np.float32)
    ids = np.zeros(lg.shape[0], dtype=np.int32)
    assert pkg.lib().biogpt_hip_sample_rows_device(0, lg.ctypes.data, lg.shape[0], lg.shape[1], top_k, top_p, temp, states.ctypes.data, ids.ctypes.data) == 0, pkg._err()
    return [int(t) for t in ids]


def fresh_states(pkg, n, seed0):
    st = np.zeros((n, 625), dtype=np.uint32)
    for r in range(n):
        assert pkg.lib().biogpt_hip_mt19937_seed(seed0 + r, st[r].ctypes.data) == 0
    return st


@pytest.mark.parametrize("nv", [42384, 42383, 1021, 320, 70])
@pytest.mark.parametrize("top_k,top_p,temp", [(40, 0.9, 0.9), (64, 1.0, 1.0), (5, 0.5, 0.7), (1, 0.9, 0.9), (2, 0.9999, 3.0)])
def test_kernel_equals_host_twin(pkg, nv, top_k, top_p, temp):
    """Random rows (odd widths leave every row but the first off the 16-byte grid), rows quantized to few distinct values (ties everywhere, at
    the k-th place too), and rows whose best elements all sit in a few threads' strides (the selection's round form).  Candidates with equal
    values have equal probabilities, and the draws are not near a border, so the ids must be the host's."""
    rng = np.random.default_rng(nv * 7 + top_k)
    n = 24
    rows = (rng.standard_normal((n, nv)) * 2.5).astype(np.float32)
    rows[8:16] = np.round(rows[8:16] * 2.0) / 2.0
    if nv >= 42383:
        idx = np.arange(nv)
        rows[16:] -= np.where((idx // 4) % 256 < 30, 0.0, 50.0).astype(np.float32)      # ~30 threads hold the best ~5000 elements: with top_k >= 40 the bound
        #                                                                                  comes from the other threads and more than 1024 elements pass it
    hs, ds = fresh_states(pkg, n, 900), fresh_states(pkg, n, 900)
    for step in range(3):
        assert device_rows(pkg, rows, top_k, top_p, temp, ds) == host_rows(pkg, rows, top_k, top_p, temp, hs), step


def test_kernel_regenerates_the_generator_block(pkg):
    """One state drawn from 330 times on the device (its 624 outputs run out once on the way): the ids and the final state are the host's."""
    rng = np.random.default_rng(5)
    rows = (rng.standard_normal((1, 2048)) * 2.5).astype(np.float32)
    hs, ds = fresh_states(pkg, 1, 77), fresh_states(pkg, 1, 77)
    got, want = [], []
    for _ in range(330):
        got += device_rows(pkg, rows, 40, 1.0, 2.0, ds)
        want += host_rows(pkg, rows, 40, 1.0, 2.0, hs)
    assert got == want
    assert np.array_equal(ds, hs)
