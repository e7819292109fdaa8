"""The wide pass layer's C interface without a GPU: the symbols of include/biogpt_hip.h exist with their signatures, a null context is refused, and the
probe's refusals come back before any launch, with their messages."""
import ctypes as C
import os
import re

import numpy as np
import pytest


def test_symbols_and_signatures(pkg):
    L = pkg.lib()
    for name, res, n_args in (("biogpt_hip_wide_pass", C.c_int, 2), ("biogpt_hip_get_wide_pass", C.c_int, 1), ("biogpt_hip_wide_pass_launches", C.c_int64, 1),
                              ("biogpt_hip_wpass_device", C.c_int, 25)):
        f = getattr(L, name)
        assert f.restype is res and len(f.argtypes) == n_args, name
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "biogpt_hip.h")).read()
    for decl, n_args in (("int biogpt_hip_wide_pass(biogpt_hip_ctx *ctx, int on);", 2), ("int biogpt_hip_get_wide_pass(const biogpt_hip_ctx *ctx);", 1),
                         ("int64_t biogpt_hip_wide_pass_launches(const biogpt_hip_ctx *ctx);", 1)):
        assert decl in header and decl.count(",") + 1 == n_args, decl
    probe = re.search(r"int biogpt_hip_wpass_device\(([^;]*)\);", header)
    assert probe and probe.group(1).count(",") + 1 == 25      # the declaration has the arguments the binding passes


def test_null_context(pkg):
    L = pkg.lib()
    assert L.biogpt_hip_wide_pass(None, 1) == -1 and "null context" in pkg._err()
    assert L.biogpt_hip_get_wide_pass(None) == -1 and "null context" in pkg._err()
    assert L.biogpt_hip_wide_pass_launches(None) == -1


def test_probe_refusals_come_before_any_launch(pkg):
    N = 9
    aq = (np.zeros((N, 160), np.int8), np.zeros((N, 5), np.float32), np.zeros((N, 5), np.uint32))
    z = dict(wtype=2, M=192, K=160, N=N, w_rows=np.zeros(192 * 5 * 18, np.uint8), bias=np.zeros(192, np.float32), aq=aq)
    for kw, msg in ((dict(z, site=2), "no site"), (dict(z, site="RESID", wtype=0), "no block format"), (dict(z, site="RESID", K=100), "multiple of 32"),
                    (dict(z, site="RESID", N=8), "N = 8 columns"), (dict(z, site="RESID"), "resid is NULL"), (dict(z, site="RESID", aq=None), "aq_q, aq_d or aq_s is NULL"),
                    (dict(z, site="FC1", M=208), "does not hold"), (dict(z, site="QKV"), "does not hold"), (dict(z, site="LOGITS", reps=-1), "reps must be"),
                    (dict(z, site="LOGITS", which=1), "which must be"), (dict(z, site="LOGITS", cfg=12), "no launch shape")):
        with pytest.raises(pkg.BiogptError, match=msg):
            pkg.wpass_device(**kw)
