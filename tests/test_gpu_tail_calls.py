"""Whole calls on model files whose logits tie (tests/wide_models.py, build_tail): an lm_head of copies of a few base rows in all five block formats and F32, and
a Q8_0 copy with NaN / +-inf lm_head scales.  Every generated id and every top-k pair equals tests/tail_ref.py applied to the oracle's rows, exactly, through
each path an id leaves by: the in-launch loop of generate_greedy, the five-launch layer, contexts past 256 keys with the key-range helpers and with the dual
form, eager launches, the F32 file, the resident loop of eval + eval_topk with and without the block walk, eval_topk on a prompt chunk (topk_kernel, and behind
its refusal the full-row fallback) and two batched columns.  tests/test_tail_files.py proves on the CPU what these rows hold.  The edits touch lm_head rows only:
no NaN reaches K / V or the next token, and no row is all NaN."""
import numpy as np
import pytest

import tail_cases
import tail_ref as T
import wide_models as wm

pytestmark = pytest.mark.gpu
K = wm.TIED_K
QUANT_FILES = ["tied_a." + t for t in wm.QUANT] + ["tail_q8"]
BOTH = ["tied_a.q4_0", "tail_q8"]


@pytest.fixture(scope="module")
def files(pkg, tmp_path_factory):
    return wm.build_tail(pkg, tmp_path_factory.mktemp("tail"), wm.TAIL_FILES)


@pytest.fixture(scope="module")
def want(oracle, files):
    """{(name, what): [(n_past, oracle row, id)]}, computed once."""
    out = {}
    for name in wm.TAIL_FILES:
        for what, prompt, steps in wm.tail_plan(name):
            out[(name, what)] = list(wm.tail_rows(oracle.OracleModel(files[name], n_threads=16), prompt, steps))
    return out


def _load(pkg, path, monkeypatch, **env):
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))      # options are read when the context is created
    g = pkg.BiogptModel.load(path)
    for k in env:
        monkeypatch.delenv(k)
    return g


def _greedy(pkg, files, want, monkeypatch, name, what, **env):
    plan = {w: (p, s) for w, p, s in wm.tail_plan(name)}
    prompt, steps = plan[what]
    g = _load(pkg, files[name], monkeypatch, **env)
    try:
        ids, _ = g.generate_greedy(prompt, steps)
        ref = [tok for _, _, tok in want[(name, what)]]
        print("%s %s %s: ids %s, want %s" % (name, what, env, list(ids), ref))
        assert list(ids) == ref, (name, what, env)
        return g.xpipe_state()
    finally:
        g.close()


@pytest.mark.parametrize("name", QUANT_FILES + ["tied_b.q4_0"])
def test_in_launch_loop(pkg, files, want, monkeypatch, name):
    assert _greedy(pkg, files, want, monkeypatch, name, "short") == 1


@pytest.mark.parametrize("name", QUANT_FILES)
def test_five_launch_layer(pkg, files, want, monkeypatch, name):
    assert _greedy(pkg, files, want, monkeypatch, name, "short", BIOGPT_HIP_XPIPE=0) != 1


@pytest.mark.parametrize("dual", (1, 0))
@pytest.mark.parametrize("name", BOTH)
def test_past_256_keys(pkg, files, want, monkeypatch, name, dual):
    assert _greedy(pkg, files, want, monkeypatch, name, "long", BIOGPT_HIP_XPIPE_DUAL=dual) == 1


@pytest.mark.parametrize("name", BOTH)
def test_eager_launches(pkg, files, want, monkeypatch, name):
    _greedy(pkg, files, want, monkeypatch, name, "short", BIOGPT_HIP_NO_GRAPH=1)


def test_f32_file(pkg, files, want, monkeypatch):
    _greedy(pkg, files, want, monkeypatch, "tied_a.f32", "short")


def _pairs(got, row, what):
    v, i = T.topk(row, K)
    assert len(i) == K
    assert got[1].tolist() == i.tolist() and got[0].tobytes() == v.tobytes(), (what, got[1][:8], i[:8])


@pytest.mark.parametrize("blocks", (1, 0))
@pytest.mark.parametrize("name", BOTH + ["tied_a.q8_0", "tied_b.q4_0"])
def test_resident_loop_of_eval_and_eval_topk(pkg, files, want, monkeypatch, name, blocks):
    rows = want[(name, "short")]
    prompt = wm.tail_prompt(name, 0)
    g = _load(pkg, files[name], monkeypatch, BIOGPT_HIP_TOPK_BLOCKS=blocks)
    try:
        lg = g.eval(prompt, 0)
        assert tail_cases.same_row(lg, rows[0][1]), name
        for (n_past, _, tok), (_, nxt, _) in zip(rows[:-1], rows[1:]):
            _pairs(g.eval_topk([tok], n_past, K), nxt, (name, blocks, n_past))
            lg = g.eval([tok], n_past)                      # the same position again: the same row
            assert tail_cases.same_row(lg, nxt) and T.argmax(lg) == T.argmax(nxt), (name, blocks, n_past)
    finally:
        g.close()


@pytest.mark.parametrize("name", BOTH + ["tied_b.q4_0"])
def test_eval_topk_on_a_prompt_chunk(pkg, files, want, name):
    row = want[(name, "short")][0][1]
    g = pkg.BiogptModel.load(files[name])
    try:
        _pairs(g.eval_topk(wm.tail_prompt(name, 0), 0, K), row, name)      # tied_b: topk_kernel refuses (more than 4096 candidates), the full-row fallback answers
        for k in (1, 7):
            v, i = T.topk(row, k)
            got = g.eval_topk(wm.tail_prompt(name, 0), 0, k)
            assert got[1].tolist() == i.tolist() and got[0].tobytes() == v.tobytes(), (name, k)
    finally:
        g.close()


@pytest.mark.parametrize("name", BOTH)
def test_two_batched_columns(pkg, files, want, name):
    g = pkg.BiogptModel.load(files[name])
    try:
        ids, _ = g.generate_greedy_batch([wm.tail_prompt(name, 0), wm.tail_prompt(name, 1)], wm.TAIL_STEPS)
        ref = [[tok for _, _, tok in want[(name, w)]] for w in ("short", "second column")]
        print("%s batched: %s, want %s" % (name, np.asarray(ids).tolist(), ref))
        assert np.asarray(ids).tolist() == ref, name
    finally:
        g.close()
