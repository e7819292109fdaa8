"""Hidden states and embeddings (biogpt_hip_hidden / biogpt_hip_embed_batch) without a GPU: the C-ABI is exported and bound, the struct has the
documented layout, argument errors come before any HIP call and name the field, and the new kernels hold everything in registers and LDS
(no scratch).

There is no context without a device, so the errors checked here are those that need no model -- biogpt_hip_embed_batch looks at them before
it looks at the context.  The three that need the model's shape (layer > n_layer, a token id >= n_vocab, a non-finite value in w, whose extent
is n_out x d_model) are checked after the model and still before any HIP call; test_gpu_embed.py covers them."""
import ctypes
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("biogpt_hip_hidden", "biogpt_hip_embed_batch")


def test_embed_symbols_exported_and_bound(pkg):
    hdr = open(os.path.join(ROOT, "include", "biogpt_hip.h")).read()
    bound = {name for name, _, _ in pkg.SYMBOLS}
    raw = ctypes.CDLL(pkg.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in bound, name
        assert getattr(raw, name) is not None
        assert getattr(pkg.lib(), name).restype is ctypes.c_int
    import inspect
    p = inspect.signature(pkg.BiogptModel.embed_batch).parameters
    assert (p["layer"].default, p["pooling"].default, p["normalize"].default, p["head"].default) == (-1, "last", False, None)
    assert inspect.signature(pkg.BiogptModel.hidden).parameters["n_past"].default == 0


def test_embed_struct_layout(pkg):
    """typedef struct { int32_t layer, pooling, normalize, n_out; const float *w, *b; } biogpt_hip_embed_opts -- as the header spells it."""
    hdr = open(os.path.join(ROOT, "include", "biogpt_hip.h")).read()
    m = re.search(r"typedef struct(?: biogpt_hip_embed_opts)? \{(.*?)\} biogpt_hip_embed_opts;", hdr, re.S)
    assert m
    fields = re.findall(r"^\s*((?:const\s+)?\w+\s*\*?)\s*(\w+);", m.group(1), re.M)
    assert [(t.replace(" ", ""), n) for t, n in fields] == [("int32_t", "layer"), ("int32_t", "pooling"), ("int32_t", "normalize"), ("int32_t", "n_out"),
                                                            ("constfloat*", "w"), ("constfloat*", "b")]
    E = pkg.EmbedOpts
    assert [n for n, _ in E._fields_] == [n for _, n in fields]
    assert (E.layer.offset, E.pooling.offset, E.normalize.offset, E.n_out.offset, E.w.offset, E.b.offset) == (0, 4, 8, 12, 16, 24)
    assert ctypes.sizeof(E) == 32
    o, keep = pkg.embed_opts()
    assert (o.layer, o.pooling, o.normalize, o.n_out) == (-1, 1, 0, 0) and not o.w and not o.b
    w = np.arange(6, dtype=np.float32).reshape(2, 3)
    o, keep = pkg.embed_opts(3, "mean", False, (w, [0.5, -1.0]))
    assert (o.layer, o.pooling, o.normalize, o.n_out, o.w[5], o.b[1]) == (3, 2, 0, 2, 5.0, -1.0)
    o, keep = pkg.embed_opts(pooling="none", normalize=True, head=None)
    assert (o.pooling, o.normalize) == (0, 1)
    with pytest.raises(pkg.BiogptError, match="pooling"):
        pkg.embed_opts(pooling="max")


TOKS = np.array([2, 5, 7, 2, 9], dtype=np.int32)
LENS = np.array([3, 2], dtype=np.int32)


def call(pkg, opts, seqs=TOKS, lens=LENS, n_seqs=2, out=True):
    buf = np.zeros((8, 1024), dtype=np.float32)
    return pkg.lib().biogpt_hip_embed_batch(None, None if seqs is None else seqs.ctypes.data, None if lens is None else lens.ctypes.data, n_seqs,
                                            ctypes.byref(opts) if opts is not None else None, buf.ctypes.data if out else None, None)


def test_embed_null_context_fails_without_a_device(pkg):
    out = np.zeros((3, 64), dtype=np.float32)
    assert pkg.lib().biogpt_hip_hidden(None, TOKS.ctypes.data, 3, 0, out.ctypes.data) == -1
    assert "null context" in pkg._err()
    assert pkg.lib().biogpt_hip_hidden(None, TOKS.ctypes.data, 3, 0, None) == -1
    assert "hidden_out" in pkg._err()
    o, keep = pkg.embed_opts()
    assert call(pkg, o) == -1 and "null context" in pkg._err()      # sound arguments: the context is the first thing wrong
    assert call(pkg, None) == -1 and "null context" in pkg._err()   # opts == NULL: the defaults


W = np.ones((2, 1024), dtype=np.float32)
# (keyword arguments of embed_opts, the field the message must name)
BAD_OPTS = [
    (dict(layer=-2), "layer"),
    (dict(head=(W, [0.0, math.nan])), "b[1]"),
    (dict(head=(W, [math.inf, 0.0])), "b[0]"),
    (dict(normalize=True, head=W), "normalize"),
    (dict(normalize=True, head=(W, [0.0, 1.0]), pooling="none"), "normalize"),
    (dict(head=np.ones((257, 4), dtype=np.float32)), "n_out"),
]


@pytest.mark.parametrize("kw,field", BAD_OPTS, ids=["%s_%d" % (re.sub(r"\W", "", f), i) for i, (_, f) in enumerate(BAD_OPTS)])
def test_embed_argument_errors_come_before_any_hip_call(pkg, kw, field):
    """No device on this machine and no context: a call that reached HIP (or the context) would not return -1 with this message."""
    o, keep = pkg.embed_opts(**kw)
    assert call(pkg, o) == -1
    assert field in pkg._err() and "null context" not in pkg._err(), pkg._err()


def test_embed_struct_errors_the_python_helper_cannot_build(pkg):
    o, keep = pkg.embed_opts()
    for v in (-1, 3):
        o.pooling = v
        assert call(pkg, o) == -1 and "pooling" in pkg._err()
    o, keep = pkg.embed_opts()
    o.normalize = 2
    assert call(pkg, o) == -1 and "normalize" in pkg._err()
    o, keep = pkg.embed_opts()
    o.n_out = -1
    assert call(pkg, o) == -1 and "n_out" in pkg._err()
    o.n_out = 3      # NULL w with n_out > 0
    assert call(pkg, o) == -1 and "w is NULL" in pkg._err()
    o, keep = pkg.embed_opts(head=(W, [0.0, 1.0]))
    o.n_out = 0      # w, then b alone, given with n_out == 0
    assert call(pkg, o) == -1 and "w given" in pkg._err()
    o.w = None
    assert call(pkg, o) == -1 and "b given" in pkg._err()


def test_embed_sequence_errors_come_before_any_hip_call(pkg):
    o, keep = pkg.embed_opts()
    assert call(pkg, o, seqs=None) == -1 and "null argument" in pkg._err()
    assert call(pkg, o, lens=None) == -1 and "null argument" in pkg._err()
    assert call(pkg, o, out=False) == -1 and "null argument" in pkg._err()
    for n in (0, -1, 513):
        assert call(pkg, o, n_seqs=n) == -1 and "n_seqs" in pkg._err()
    assert call(pkg, o, lens=np.array([5, 0], dtype=np.int32)) == -1 and "empty sequence (sequence 1)" in pkg._err()
    assert call(pkg, o, seqs=np.array([2, 5, 7, -4, 9], dtype=np.int32)) == -1 and "token id -4" in pkg._err()


def test_embed_kernels_use_no_scratch(pkg, tmp_path):
    """ln_rows_kernel<1024> / <0>, pool_rows_kernel, pool_finish_kernel, head_rows_kernel: the kernel descriptors in obj/engine.o, read as
    test_score_capi.py reads the log-softmax kernel's."""
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
        if m and name and re.search(r"ln_rows_kernel|pool_rows_kernel|pool_finish_kernel|head_rows_kernel", name):
            assert int(m.group(1)) == 0, "%s uses %s bytes of scratch per lane" % (name, m.group(1))
            seen.add(name)
    assert len(seen) == 5, seen
