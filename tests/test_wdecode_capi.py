"""The wide decode layer's C interface without a GPU: the symbols of include/biogpt_hip.h exist with their signatures, and the refusals come back before
any launch, with their messages."""
import ctypes as C
import os
import re

import numpy as np
import pytest


def test_symbols_and_signatures(pkg):
    L = pkg.lib()
    for name, res, n_args in (("biogpt_hip_wide_decode", C.c_int, 2), ("biogpt_hip_get_wide_decode", C.c_int, 1), ("biogpt_hip_wide_decode_launches", C.c_int64, 1),
                              ("biogpt_hip_wide_decode_key_borders", C.c_int, 2), ("biogpt_hip_wdecode_device", C.c_int, 27)):
        f = getattr(L, name)
        assert f.restype is res and len(f.argtypes) == n_args, name
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "biogpt_hip.h")).read()
    for decl, n_args in (("int biogpt_hip_wide_decode(biogpt_hip_ctx *ctx, int on);", 2), ("int biogpt_hip_get_wide_decode(const biogpt_hip_ctx *ctx);", 1),
                         ("int64_t biogpt_hip_wide_decode_launches(const biogpt_hip_ctx *ctx);", 1), ("int biogpt_hip_wide_decode_key_borders(int32_t *out, int cap);", 2)):
        assert decl in header and decl.count(",") + 1 == n_args, decl
    probe = re.search(r"int biogpt_hip_wdecode_device\(([^;]*)\);", header)
    assert probe and probe.group(1).count(",") + 1 == 27      # the declaration has the arguments the binding passes
    borders = pkg.wide_decode_key_borders()
    assert borders == sorted(borders) and len(borders) >= 1 and borders[0] >= 1


def test_null_context(pkg):
    L = pkg.lib()
    assert L.biogpt_hip_wide_decode(None, 1) == -1 and "null context" in pkg._err()
    assert L.biogpt_hip_get_wide_decode(None) == -1 and "null context" in pkg._err()
    assert L.biogpt_hip_wide_decode_launches(None) == -1


def test_probe_refusals_come_before_any_launch(pkg):
    z = dict(wtype=2, M=192, K=160, w_rows=np.zeros(192 * 5 * 18, np.uint8), bias=np.zeros(192, np.float32))
    aq = (np.zeros(160, np.int8), np.zeros(5, np.float32), np.zeros(5, np.uint32))
    for kw, msg in ((dict(z, stage=7), "no stage"), (dict(z, stage="OPROJ", wtype=0, aq=aq), "no block format"), (dict(z, stage="OPROJ", K=100, aq=aq), "multiple of 32"),
                    (dict(z, stage="OPROJ", aq=aq), "resid is NULL"), (dict(z, stage="OPROJ"), "aq_q, aq_d or aq_s is NULL"), (dict(z, stage="FC1", M=200), "does not hold"),
                    (dict(z, stage="FC1"), "x, ln_w or ln_b is NULL"), (dict(z, stage="QKV", x=aq[1], ln_w=aq[1], ln_b=aq[1]), "3 K x K"),
                    (dict(stage="ATTN", H=3, P=300, n_past=256), "the kernel holds"), (dict(z, stage="FC2", aq=aq, resid=z["bias"], reps=-1), "reps must be")):
        with pytest.raises(pkg.BiogptError, match=msg):
            pkg.wdecode_device(**kw)
