"""Contrastive search (biogpt_hip_generate_contrastive, biogpt_hip_contrast_rank_device) without a GPU: the C-ABI is exported and bound with the
declared signature, every argument error returns -1 and names its field before any HIP call, and the new kernels hold everything in
registers and LDS (no scratch)."""
import ctypes
import os
import re

import numpy as np
import pytest

from test_beam_batch_capi import kernel_scratch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_P = ctypes.c_void_p


def test_contrast_symbols_exported_and_bound(pkg):
    hdr = open(os.path.join(ROOT, "include", "biogpt_hip.h")).read()
    bound = {name: (res, args) for name, res, args in pkg.SYMBOLS}
    raw = ctypes.CDLL(pkg.LIB_PATH)
    for name in ("biogpt_hip_generate_contrastive", "biogpt_hip_contrast_rank_device"):
        assert re.search(r"\b%s\s*\(" % name, hdr)
        assert name in bound
        assert getattr(raw, name) is not None
        assert getattr(pkg.lib(), name).restype is ctypes.c_int
    # (ctx, prompts, prompt_lens, n_prompts, n_batch, top_k, penalty_alpha, n_predict, eos_id, out_ids, out_lens, out_scores, seconds_out)
    assert bound["biogpt_hip_generate_contrastive"][1] == [_P, _P, _P, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_float, ctypes.c_int32,
                                                           ctypes.c_int32, _P, _P, _P, ctypes.POINTER(ctypes.c_double)]
    # (device, cand, ctx_rows, k, T, d, probs, alpha, pen_out, score_out, winner_out)
    assert bound["biogpt_hip_contrast_rank_device"][1] == [ctypes.c_int, _P, _P, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _P, ctypes.c_float, _P, _P, _P]
    decl = re.search(r"int biogpt_hip_generate_contrastive\((.*?)\);", hdr, re.S).group(1)
    decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
    assert [a.split()[-1].lstrip("*") for a in decl.split(",")] == ["ctx", "prompts", "prompt_lens", "n_prompts", "n_batch", "top_k", "penalty_alpha", "n_predict",
                                                                     "eos_id", "out_ids", "out_lens", "out_scores", "seconds_out"]
    assert hasattr(pkg.BiogptModel, "generate_contrastive") and callable(pkg.contrast_rank)


def call(pkg, ctx=None, prompts=True, lens=True, n_prompts=2, n_batch=8, top_k=4, alpha=0.6, n_predict=8, eos_id=-1, ids=True, ol=True):
    pr = np.array([2, 5, 7, 2, 9], dtype=np.int32)
    ln = np.array([3, 2], dtype=np.int32)
    out = np.zeros((max(n_prompts, 1), 8), dtype=np.int32)
    lens_out = np.zeros(max(n_prompts, 1), dtype=np.int32)
    secs = ctypes.c_double(0.0)
    rc = pkg.lib().biogpt_hip_generate_contrastive(ctx, pr.ctypes.data if prompts else None, ln.ctypes.data if lens else None, n_prompts, n_batch, top_k, alpha,
                                                   n_predict, eos_id, out.ctypes.data if ids else None, lens_out.ctypes.data if ol else None, None,
                                                   ctypes.byref(secs))
    return rc, pkg._err()


@pytest.mark.parametrize("kw, field", [
    (dict(), "null context"),
    (dict(prompts=False), "prompts"), (dict(lens=False), "prompt_lens"), (dict(ids=False), "out_ids"), (dict(ol=False), "out_lens"),
    (dict(n_prompts=0), "n_prompts"), (dict(n_prompts=-3), "n_prompts"),
    (dict(top_k=0), "top_k"), (dict(top_k=17), "top_k"),
    (dict(n_prompts=129, top_k=4), "n_prompts x top_k"), (dict(n_prompts=513, top_k=1), "n_prompts x top_k"),
    (dict(n_batch=0), "n_batch"),
    (dict(alpha=-0.1), "penalty_alpha"), (dict(alpha=1.5), "penalty_alpha"), (dict(alpha=float("nan")), "penalty_alpha"),
    (dict(eos_id=-2), "eos_id"),
])
def test_contrastive_argument_errors_come_before_any_device_call(pkg, kw, field):
    """No device on this machine: a call that reached HIP would return -2, not -1."""
    rc, msg = call(pkg, **kw)
    assert rc == -1, (rc, msg)
    assert field in msg, msg


@pytest.mark.parametrize("kw, field", [
    (dict(cand=False), "null"), (dict(k=0), "k must"), (dict(k=17), "k must"), (dict(T=0), "T must"), (dict(d=6), "d must"), (dict(d=2048), "d must"),
    (dict(alpha=2.0), "alpha"),
])
def test_rank_entry_argument_errors(pkg, kw, field):
    a = dict(cand=True, k=2, T=3, d=8, alpha=0.5)
    a.update(kw)
    buf = np.zeros(4096 * 4, dtype=np.float32)
    pen, sc, win = np.zeros(16, np.float32), np.zeros(16, np.float32), ctypes.c_int32(0)
    rc = pkg.lib().biogpt_hip_contrast_rank_device(0, buf.ctypes.data if a["cand"] else None, buf.ctypes.data, a["k"], a["T"], a["d"], buf.ctypes.data, a["alpha"],
                                                   pen.ctypes.data, sc.ctypes.data, ctypes.addressof(win))
    assert rc == -1 and field in pkg._err(), (rc, pkg._err())


def test_contrast_kernels_use_no_scratch(pkg, tmp_path):
    ks = {n: v for n, v in kernel_scratch(pkg, tmp_path).items() if re.search(r"contrast_\w+_kernel", n)}
    for n, v in ks.items():
        assert v == 0, "%s uses %d bytes of scratch per lane" % (n, v)
    assert len(ks) == 5, sorted(ks)      # rank, select, kv_row, norms, pick
