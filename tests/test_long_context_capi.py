"""The long-context attention's C interface without a GPU: the symbols of include/biogpt_hip.h exist with their signatures, a null context is refused, and the
probe's refusals come back before any HIP call, with their messages."""
import ctypes as C
import os
import re

import numpy as np


def test_symbols_and_signatures(pkg):
    L = pkg.lib()
    for name, res, n_args in (("biogpt_hip_long_context", C.c_int, 2), ("biogpt_hip_get_long_context", C.c_int, 1), ("biogpt_hip_long_attn_launches", C.c_int64, 1),
                              ("biogpt_hip_attn_long_device", C.c_int, 16), ("biogpt_hip_attn_long_bench", C.c_int, 17), ("biogpt_hip_attn_device_bench", C.c_int, 21)):
        f = getattr(L, name)
        assert f.restype is res and len(f.argtypes) == n_args, name
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "biogpt_hip.h")).read()
    for decl in ("int biogpt_hip_long_context(biogpt_hip_ctx *ctx, int on);", "int biogpt_hip_get_long_context(const biogpt_hip_ctx *ctx);",
                 "int64_t biogpt_hip_long_attn_launches(const biogpt_hip_ctx *ctx);"):
        assert decl in header, decl
    for name, n_args in (("biogpt_hip_attn_long_device", 16), ("biogpt_hip_attn_long_bench", 17), ("biogpt_hip_attn_device_bench", 21)):
        probe = re.search(r"int %s\(([^;]*)\);" % name, header)
        assert probe and probe.group(1).count(",") + 1 == n_args, name      # the declaration has the arguments the binding passes


def test_null_context(pkg):
    L = pkg.lib()
    assert L.biogpt_hip_long_context(None, 1) == -1 and "null context" in pkg._err()
    assert L.biogpt_hip_get_long_context(None) == -1 and "null context" in pkg._err()
    assert L.biogpt_hip_long_attn_launches(None) == -1


def test_probe_refusals_come_before_any_hip_call(pkg):
    H, P = 3, 2048
    q, kv = np.zeros((16, H * 64), np.float32), np.zeros((H, P, 64), np.float32)
    state = lambda n_past, causal=0: np.array([n_past, 0, causal, 0], dtype=np.int32)
    for kw, msg in ((dict(form=0, N=1, t_max=1024, dev_state=state(1023)), "t_max must be in"), (dict(form=1, N=16, t_max=2049, dev_state=state(2033)), "t_max must be in"),
                    (dict(form=1, N=8, t_max=1100, dev_state=state(1092)), "tile form"), (dict(form=0, N=9, t_max=1100, dev_state=state(1091)), "column form"),
                    (dict(form=0, N=2, t_max=1100, dev_state=state(1200)), "visible keys"), (dict(form=0, N=1, t_max=1100, dev_state=state(-1, 1)), "negative"),
                    (dict(form=3, N=1, t_max=1100, dev_state=state(1099)), "form must be"), (dict(form=0, N=1, t_max=1100, dev_state=None), "NULL"),
                    (dict(form=0, N=1, t_max=1100, dev_state=state(1099), q8=3), "q8 must be"), (dict(form=0, N=1, t_max=1100, dev_state=state(1099), reps=100000), "reps must be")):
        rc = pkg.attn_long_device(H=H, P=P, q=q, k_slot=kv, v_slot=kv, **kw)[0]
        assert rc == -1 and msg in pkg._err(), (kw, rc, pkg._err())
