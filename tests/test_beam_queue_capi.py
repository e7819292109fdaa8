"""Beam search over a queue (biogpt_hip_generate_beam_queue) without a GPU: the C-ABI is exported and bound with the declared signature, every argument
error that can be judged without a model returns -1 and names its field before any HIP call (the ones that need the model's sizes are checked where a
model can be loaded, tests/test_gpu_beam_queue.py), the Python wrapper passes what it documents, and the three kernels hold everything in registers."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_P = ctypes.c_void_p
NAME = "biogpt_hip_generate_beam_queue"


def test_beam_queue_symbol_exported_and_bound(pkg):
    hdr = open(os.path.join(ROOT, "include", "biogpt_hip.h")).read()
    bound = {name: (res, args) for name, res, args in pkg.SYMBOLS}
    raw = ctypes.CDLL(pkg.LIB_PATH)
    assert re.search(r"\b%s\s*\(" % NAME, hdr)
    assert NAME in bound
    assert getattr(raw, NAME) is not None
    assert getattr(pkg.lib(), NAME).restype is ctypes.c_int
    i32, f32, f64 = ctypes.c_int32, ctypes.c_float, ctypes.c_double
    assert bound[NAME][1] == [_P, _P, _P, i32, _P, i32, i32, i32, i32, i32, i32, f32, i32, _P, _P, _P, _P, _P, _P, _P, _P, ctypes.POINTER(f64),
                              ctypes.POINTER(pkg.QueueStats)]
    decl = re.search(r"int %s\((.*?)\);" % NAME, hdr, re.S).group(1)
    decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
    assert [a.split()[-1].lstrip("*") for a in decl.split(",")] == ["ctx", "prompts", "prompt_lens", "n_requests", "n_predicts", "n_predict", "n_beams", "max_columns",
                                                                     "group", "n_batch", "eos_id", "length_penalty", "early_stopping", "trie", "out_ids", "out_lens",
                                                                     "out_scores", "out_counts", "out_steps", "out_admit_step", "out_slot", "seconds_out", "stats"]
    assert hasattr(pkg.BiogptModel, "generate_beam_queue")


def call(pkg, ctx=None, prompts=True, lens=(3, 2), tokens=(2, 5, 7, 2, 9), n_requests=2, n_predicts=None, n_predict=8, n_beams=2, max_columns=4, group=4, n_batch=8,
         eos_id=2, length_penalty=1.0, early_stopping=1, ids=True, ol=True, scores=True, counts=True, prompt_lens=True):
    pr = np.array(tokens, dtype=np.int32)
    ln = np.array(lens, dtype=np.int32)
    npr = None if n_predicts is None else np.array(n_predicts, dtype=np.int32)
    B = max(1, min(n_beams, 64))
    out = np.zeros((2 * B, 8), dtype=np.int32)
    lens_out, sc, cnt = np.zeros(2 * B, dtype=np.int32), np.zeros(2 * B, dtype=np.float32), np.zeros(2, dtype=np.int32)
    steps, adm, slot = np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.int32)
    secs = ctypes.c_double(0.0)
    st = pkg.QueueStats()
    rc = pkg.lib().biogpt_hip_generate_beam_queue(ctx, pr.ctypes.data if prompts else None, ln.ctypes.data if prompt_lens else None, n_requests,
                                                  None if npr is None else npr.ctypes.data, n_predict, n_beams, max_columns, group, n_batch, eos_id, length_penalty,
                                                  early_stopping, None, out.ctypes.data if ids else None, lens_out.ctypes.data if ol else None,
                                                  sc.ctypes.data if scores else None, cnt.ctypes.data if counts else None, steps.ctypes.data, adm.ctypes.data,
                                                  slot.ctypes.data, ctypes.byref(secs), ctypes.byref(st))
    return rc, pkg._err()


@pytest.mark.parametrize("kw, field", [
    (dict(), "null context"),
    (dict(n_predicts=(8, 0)), "null context"),
    (dict(n_beams=1, max_columns=1), "null context"), (dict(n_beams=16, max_columns=512), "null context"), (dict(eos_id=-1), "null context"),
    (dict(prompts=False), "prompts"), (dict(prompt_lens=False), "prompt_lens"), (dict(ids=False), "out_ids"), (dict(ol=False), "out_lens"),
    (dict(scores=False), "out_scores"), (dict(counts=False), "out_counts"),
    (dict(n_requests=0), "n_requests"), (dict(n_requests=-3), "n_requests"),
    (dict(n_beams=0), "n_beams must be in [1, 16]"), (dict(n_beams=17, max_columns=64), "n_beams must be in [1, 16]"), (dict(n_beams=-2), "n_beams must be in [1, 16]"),
    (dict(n_beams=5, max_columns=4), "max_columns must be in [n_beams = 5, 512]"), (dict(max_columns=513), "max_columns must be in [n_beams = 2, 512]"),
    (dict(max_columns=0), "max_columns"),
    (dict(group=0), "group must be in [1, 64]"), (dict(group=65), "group must be in [1, 64]"),
    (dict(n_batch=0), "n_batch"), (dict(n_predict=-1), "n_predict"),
    (dict(n_predicts=(3, 9)), "n_predicts[1]"), (dict(n_predicts=(-1, 4)), "n_predicts[0]"),
    (dict(lens=(3, 0), tokens=(2, 5, 7)), "empty prompt (request 1)"), (dict(lens=(-1, 2)), "empty prompt (request 0)"),
    (dict(tokens=(2, 5, 7, -4, 9)), "token id -4 (request 1, position 0)"),
    (dict(eos_id=-2), "eos_id"), (dict(length_penalty=float("nan")), "length_penalty"), (dict(length_penalty=float("inf")), "length_penalty"),
    (dict(early_stopping=2), "early_stopping"),
])
def test_beam_queue_argument_errors_come_before_any_device_call(pkg, kw, field):
    """No device on this machine: a call that reached HIP would return -2, not -1."""
    rc, msg = call(pkg, **kw)
    assert rc == -1, (rc, msg)
    assert field in msg, msg


def test_trie_is_judged_before_the_context(pkg):
    """With a trie, EOS is how an entry ends: no EOS id, or one that an entry uses, fails without a context as biogpt_hip_generate_beam_trie's check does."""
    trie = pkg.Trie.build([[5, 6], [5, 7, 8]], 64)
    model = pkg.BiogptModel.__new__(pkg.BiogptModel)
    model._h = None
    with pytest.raises(pkg.BiogptError, match="eos_id must be >= 0 with a trie"):
        model.generate_beam_queue([[2, 5]], 4, n_beams=2, max_columns=4, eos_id=-1, trie=trie)
    with pytest.raises(pkg.BiogptError, match="occurs in an entry"):
        model.generate_beam_queue([[2, 5]], 4, n_beams=2, max_columns=4, eos_id=7, trie=trie)
    with pytest.raises(pkg.BiogptError, match="null context"):
        model.generate_beam_queue([[2, 5]], 4, n_beams=2, max_columns=4, eos_id=2, trie=trie)


# ---- the scheduler with limits (biogpt_hip_queue_plan_limits): the struct a run drives, given where the requests ended ----

def plan_under_limits(steps, limits, slots, group):
    """DESIGN.md 4.7 restated for requests that may end before their limits: a group is min(group, the most steps any running request may STILL take under its
    limit), and a look finds finished whoever has taken all its steps."""
    waiting = [r for r, n in enumerate(limits) if n > 0]
    S = min(slots, len(waiting))
    admit_step, slot = [-1] * len(limits), [-1] * len(limits)
    holder, since = [None] * S, {}
    n_steps = groups = admissions = 0
    while waiting or since:
        took = False
        for s in range(S):
            if holder[s] is None and waiting:
                r = waiting.pop(0)
                holder[s], since[r] = r, 0
                admit_step[r], slot[r] = n_steps, s
                took = True
        admissions += 1 if took else 0
        g = min(group, max(limits[r] - since[r] for r in since))
        n_steps += g
        groups += 1
        for s in range(S):
            r = holder[s]
            if r is not None:
                since[r] += g
                if since[r] >= steps[r]:
                    del since[r]
                    holder[s] = None
    stats = dict(columns=S, steps=n_steps, groups=groups, admissions=admissions, prompt_columns=0, busy_column_steps=sum(steps), column_steps=S * n_steps)
    return dict(stats=stats, admit_step=admit_step, column=slot)


def test_plan_with_limits_is_the_plan_where_nothing_ends_early_and_differs_where_it_must(pkg):
    hdr = open(os.path.join(ROOT, "include", "biogpt_hip.h")).read()
    assert re.search(r"\bbiogpt_hip_queue_plan_limits\s*\(", hdr) and "biogpt_hip_queue_plan_limits" in {n for n, _, _ in pkg.SYMBOLS}
    # one column, group 4: request 0 ends after 2 of its 10 steps.  The host had sized the group by the limit: 4 steps run before request 1 is admitted,
    # where the plan that takes the steps for the limits says 2
    assert pkg.queue_plan([2, 3], 1, 4, limits=[10, 3]) == dict(
        stats=dict(columns=1, steps=7, groups=2, admissions=2, prompt_columns=0, busy_column_steps=5, column_steps=7), admit_step=[0, 4], column=[0, 0])
    assert pkg.queue_plan([2, 3], 1, 4)["admit_step"] == [0, 2] and pkg.queue_plan([2, 3], 1, 4)["stats"]["steps"] == 5
    assert pkg.queue_plan([2, 3], 1, 1, limits=[10, 3]) == pkg.queue_plan([2, 3], 1, 1)      # group 1: nothing to cut short
    rng = np.random.default_rng(5)
    differ = 0
    for _ in range(200):
        n = int(rng.integers(1, 14))
        limits = [int(v) for v in rng.integers(0, 12, n)]
        steps = [int(rng.integers(1, m + 1)) if m > 0 else 0 for m in limits]
        slots, group = int(rng.integers(1, 6)), int(rng.integers(1, 7))
        assert pkg.queue_plan(steps, slots, group, limits=limits) == plan_under_limits(steps, limits, slots, group), (steps, limits, slots, group)
        assert pkg.queue_plan(steps, slots, group, limits=steps) == pkg.queue_plan(steps, slots, group)
        differ += pkg.queue_plan(steps, slots, group, limits=limits) != pkg.queue_plan(steps, slots, group)
    assert differ > 20


@pytest.mark.parametrize("args, field", [
    (dict(steps=[3, 2], limits=[2, 2]), "limits[0] (2) is below gen_lens[0] (3)"), (dict(steps=[0, 2], limits=[4, 2]), "gen_lens[0] is 0 under a limit of 4"),
    (dict(steps=[-1, 2], limits=[4, 2]), "gen_lens[0]"), (dict(steps=[1, 2], limits=[4, 2], slots=0), "max_columns"), (dict(steps=[1, 2], limits=[4, 2], group=65), "group"),
])
def test_plan_with_limits_argument_errors(pkg, args, field):
    with pytest.raises(pkg.BiogptError, match=re.escape(field)):
        pkg.queue_plan(args["steps"], args.get("slots", 2), args.get("group", 4), limits=args["limits"])
    with pytest.raises(pkg.BiogptError, match="one entry per request"):
        pkg.queue_plan([1, 2], 2, 4, limits=[1])


def _words(addr, n, ctype):
    return [int(v) for v in np.ctypeslib.as_array(ctypes.cast(addr, ctypes.POINTER(ctype)), (n,))]


class FakeLib:
    """Stands where the library is: keeps the arguments of biogpt_hip_generate_beam_queue (the arrays copied while they live) and answers as a run of no
    eligible request would."""
    def __init__(self):
        self.args = self.lens = self.tokens = self.n_predicts = None

    def biogpt_hip_generate_beam_queue(self, *args):
        self.args = args
        R = args[3]
        self.lens = _words(args[2], R, ctypes.c_int32)
        self.tokens = _words(args[1], sum(self.lens), ctypes.c_int32)
        self.n_predicts = None if args[4] is None else _words(args[4], R, ctypes.c_int32)
        return 0


def test_python_wrapper_passes_what_it_documents(pkg, monkeypatch):
    sig = inspect.signature(pkg.BiogptModel.generate_beam_queue)
    assert list(sig.parameters)[1:] == ["prompts", "n_predict", "n_beams", "max_columns", "group", "eos_id", "length_penalty", "early_stopping", "n_batch", "n_predicts",
                                        "trie"]
    want = dict(n_beams=5, group=4, eos_id=2, length_penalty=1.0, early_stopping=True, n_batch=8, n_predicts=None, trie=None)
    assert {k: sig.parameters[k].default for k in want} == want
    mc = sig.parameters["max_columns"].default
    assert 5 <= mc <= 512 and mc % 5 == 0      # whole groups of the default five beams
    fake = FakeLib()
    monkeypatch.setattr(pkg, "lib", lambda: fake)
    model = pkg.BiogptModel.__new__(pkg.BiogptModel)
    model._h = None

    hyps, info, secs = model.generate_beam_queue([[2, 5, 7], [2, 9], [2]], 6)
    a = fake.args
    assert fake.tokens == [2, 5, 7, 2, 9, 2] and fake.lens == [3, 2, 1] and a[3] == 3
    assert fake.n_predicts is None and a[5:13] == (6, 5, mc, 4, 8, 2, 1.0, 1) and a[13] is None
    assert hyps == [[], [], []] and info["admit_step"] == [0, 0, 0] and info["slot"] == [0, 0, 0] and info["steps"] == [0, 0, 0]
    assert set(info["stats"]) == {n for n, _ in pkg.QueueStats._fields_}
    model.generate_beam_queue([[2, 5, 7], [2, 9]], 6, n_predicts=[6, 2], n_beams=3, max_columns=9, group=2, eos_id=-1, length_penalty=0.8, early_stopping=False, n_batch=4)
    assert fake.n_predicts == [6, 2] and fake.args[5:11] == (6, 3, 9, 2, 4, -1) and abs(fake.args[11] - 0.8) < 1e-12 and fake.args[12] == 0
    model.generate_beam_queue([2, 5, 7], 6)      # one flat id list: one request
    assert fake.args[3] == 1 and fake.lens == [3]
    with pytest.raises(pkg.BiogptError, match="n_predicts"):
        model.generate_beam_queue([[2], [3]], 4, n_predicts=[1, 2, 3])


def test_beam_queue_kernels_use_no_scratch(pkg, tmp_path):
    """beam_slot_admit_kernel, kv_share_slots_kernel and beam_slot_report_kernel: the kernel descriptors in obj/engine.o, read as test_queue_capi.py reads
    the sampling queue's."""
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
        if m and name and re.search(r"beam_slot_admit_kernel|kv_share_slots_kernel|beam_slot_report_kernel", name):
            assert int(m.group(1)) == 0, "%s uses %s bytes of scratch per lane" % (name, m.group(1))
            seen.add(name)
    assert len(seen) == 3, seen
