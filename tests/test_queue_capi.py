"""Generation over a queue (biogpt_hip_generate_queue, biogpt_hip_queue_plan) without a GPU: the C-ABI is exported and bound with the declared signature,
every argument error that can be judged without a model returns -1 and names its field before any HIP call (the ones that need the model's sizes -- a
token or eos_id >= n_vocab, a float-weight file -- are checked where a model can be loaded, tests/test_gpu_queue.py), the Python wrapper's defaults are
the documented ones, and the two kernels hold everything in registers and LDS."""
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
NAMES = ("biogpt_hip_generate_queue", "biogpt_hip_queue_plan")


def test_queue_symbols_exported_and_bound(pkg):
    hdr = open(os.path.join(ROOT, "include", "biogpt_hip.h")).read()
    bound = {name: (res, args) for name, res, args in pkg.SYMBOLS}
    raw = ctypes.CDLL(pkg.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr)
        assert name in bound
        assert getattr(raw, name) is not None
        assert getattr(pkg.lib(), name).restype is ctypes.c_int
    i32, f64 = ctypes.c_int32, ctypes.c_double
    assert bound["biogpt_hip_generate_queue"][1] == [_P, _P, _P, i32, _P, i32, i32, i32, i32, i32, f64, f64, _P, i32, _P, _P, _P, _P, ctypes.POINTER(f64),
                                                     ctypes.POINTER(pkg.QueueStats)]
    decl = re.search(r"int biogpt_hip_generate_queue\((.*?)\);", hdr, re.S).group(1)
    decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
    assert [a.split()[-1].lstrip("*") for a in decl.split(",")] == ["ctx", "prompts", "prompt_lens", "n_requests", "n_predicts", "n_predict", "max_columns", "group",
                                                                     "n_batch", "top_k", "top_p", "temp", "seeds", "eos_id", "out_ids", "out_lens", "out_admit_step",
                                                                     "out_column", "seconds_out", "stats"]
    decl = re.search(r"int biogpt_hip_queue_plan\((.*?)\);", hdr, re.S).group(1)
    assert len(re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")) == 7 == len(bound["biogpt_hip_queue_plan"][1])
    # the struct as the header lays it out: five int32, then two int64 at offset 24
    assert [n for n, _ in pkg.QueueStats._fields_] == ["columns", "steps", "groups", "admissions", "prompt_columns", "busy_column_steps", "column_steps"]
    assert ctypes.sizeof(pkg.QueueStats) == 40 and pkg.QueueStats.busy_column_steps.offset == 24
    assert hasattr(pkg.BiogptModel, "generate_queue") and callable(pkg.queue_plan)


def call(pkg, ctx=None, prompts=True, lens=(3, 2), tokens=(2, 5, 7, 2, 9), n_requests=2, n_predicts=None, n_predict=8, max_columns=4, group=4, n_batch=8, top_k=40,
         top_p=0.9, temp=0.9, seeds=True, eos_id=-1, ids=True, ol=True, prompt_lens=True):
    pr = np.array(tokens, dtype=np.int32)
    ln = np.array(lens, dtype=np.int32)
    sd = np.array([1, 2], dtype=np.uint32)
    npr = None if n_predicts is None else np.array(n_predicts, dtype=np.int32)
    out = np.zeros((2, 8), dtype=np.int32)
    lens_out, adm, col = np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.int32)
    secs = ctypes.c_double(0.0)
    st = pkg.QueueStats()
    rc = pkg.lib().biogpt_hip_generate_queue(ctx, pr.ctypes.data if prompts else None, ln.ctypes.data if prompt_lens else None, n_requests,
                                             None if npr is None else npr.ctypes.data, n_predict, max_columns, group, n_batch, top_k, top_p, temp,
                                             sd.ctypes.data if seeds else None, eos_id, out.ctypes.data if ids else None, lens_out.ctypes.data if ol else None,
                                             adm.ctypes.data, col.ctypes.data, ctypes.byref(secs), ctypes.byref(st))
    return rc, pkg._err()


@pytest.mark.parametrize("kw, field", [
    (dict(), "null context"),
    (dict(n_predicts=(8, 0)), "null context"),
    (dict(prompts=False), "prompts"), (dict(prompt_lens=False), "prompt_lens"), (dict(seeds=False), "seeds"), (dict(ids=False), "out_ids"), (dict(ol=False), "out_lens"),
    (dict(n_requests=0), "n_requests"), (dict(n_requests=-3), "n_requests"),
    (dict(max_columns=0), "max_columns must be in [1, 512]"), (dict(max_columns=513), "max_columns must be in [1, 512]"),
    (dict(group=0), "group must be in [1, 64]"), (dict(group=65), "group must be in [1, 64]"),
    (dict(n_batch=0), "n_batch"), (dict(n_predict=-1), "n_predict"),
    (dict(n_predicts=(3, 9)), "n_predicts[1]"), (dict(n_predicts=(-1, 4)), "n_predicts[0]"),
    (dict(lens=(3, 0), tokens=(2, 5, 7)), "empty prompt (request 1)"), (dict(lens=(-1, 2)), "empty prompt (request 0)"),
    (dict(tokens=(2, 5, 7, -4, 9)), "token id -4 (request 1, position 0)"),
    (dict(top_k=0), "top_k"), (dict(top_k=65), "top_k"), (dict(temp=0.0), "temp"), (dict(temp=float("nan")), "temp"), (dict(temp=-1.0), "temp"),
    (dict(top_p=float("inf")), "top_p"), (dict(top_p=float("nan")), "top_p"), (dict(eos_id=-2), "eos_id"),
])
def test_queue_argument_errors_come_before_any_device_call(pkg, kw, field):
    """No device on this machine: a call that reached HIP would return -2, not -1."""
    rc, msg = call(pkg, **kw)
    assert rc == -1, (rc, msg)
    assert field in msg, msg


def _words(addr, n, ctype):
    return [int(v) for v in np.ctypeslib.as_array(ctypes.cast(addr, ctypes.POINTER(ctype)), (n,))]


class FakeLib:
    """Stands where the library is: keeps the arguments of biogpt_hip_generate_queue (the arrays copied while they live) and answers as a run of no
    eligible request would."""
    def __init__(self):
        self.args = self.lens = self.tokens = self.seeds = self.n_predicts = None

    def biogpt_hip_generate_queue(self, *args):
        self.args = args
        R = args[3]
        self.lens = _words(args[2], R, ctypes.c_int32)
        self.tokens = _words(args[1], sum(self.lens), ctypes.c_int32)
        self.seeds = _words(args[12], R, ctypes.c_uint32)
        self.n_predicts = None if args[4] is None else _words(args[4], R, ctypes.c_int32)
        return 0


def test_python_wrapper_defaults(pkg, monkeypatch):
    sig = inspect.signature(pkg.BiogptModel.generate_queue)
    assert list(sig.parameters)[1:] == ["prompts", "n_predict", "max_columns", "group", "top_k", "top_p", "temp", "seed", "seeds", "eos_id", "n_batch", "n_predicts"]
    want = dict(max_columns=64, group=4, top_k=1, top_p=0.9, temp=0.9, seed=0, seeds=None, eos_id=-1, n_batch=8, n_predicts=None)
    assert {k: sig.parameters[k].default for k in want} == want
    fake = FakeLib()
    monkeypatch.setattr(pkg, "lib", lambda: fake)
    model = pkg.BiogptModel.__new__(pkg.BiogptModel)
    model._h = None

    ids, info, secs = model.generate_queue([[2, 5, 7], [2, 9], [2]], 6, seed=0xFFFFFFFE)
    a = fake.args
    assert fake.tokens == [2, 5, 7, 2, 9, 2] and fake.lens == [3, 2, 1] and a[3] == 3
    assert fake.n_predicts is None and a[5:12] == (6, 64, 4, 8, 1, 0.9, 0.9) and a[13] == -1
    assert fake.seeds == [0xFFFFFFFE, 0xFFFFFFFF, 0]      # seeds=None: seed + r, modulo 2^32
    assert [len(i) for i in ids] == [0, 0, 0] and info["admit_step"] == [0, 0, 0] and set(info["stats"]) == {n for n, _ in pkg.QueueStats._fields_}
    model.generate_queue([[2, 5, 7], [2, 9]], 6, seeds=[11, 12], n_predicts=[6, 2], max_columns=3, group=2, top_k=40, eos_id=2, n_batch=4)
    assert fake.seeds == [11, 12] and fake.n_predicts == [6, 2] and fake.args[5:10] == (6, 3, 2, 4, 40) and fake.args[13] == 2
    model.generate_queue([2, 5, 7], 6)      # one flat id list: one request
    assert fake.args[3] == 1 and fake.lens == [3]
    with pytest.raises(pkg.BiogptError, match="seeds"):
        model.generate_queue([[2], [3]], 4, seeds=[1])
    with pytest.raises(pkg.BiogptError, match="n_predicts"):
        model.generate_queue([[2], [3]], 4, n_predicts=[1, 2, 3])


def test_queue_kernels_use_no_scratch(pkg, tmp_path):
    """queue_rows_kernel and queue_admit_kernel: the kernel descriptors in obj/engine.o, read as test_sample_capi.py reads the sampler's."""
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
        if m and name and re.search(r"queue_rows_kernel|queue_admit_kernel", name):
            assert int(m.group(1)) == 0, "%s uses %s bytes of scratch per lane" % (name, m.group(1))
            seen.add(name)
    assert len(seen) == 2, seen
