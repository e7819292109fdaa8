"""The wide chain's public symbols without a GPU: biogpt_hip_chain_kind and biogpt_hip_wide_launches (and the probe of the kernel alone,
biogpt_hip_wide_chain_device) are declared, exported and bound; the first two reject a null context; the probe's refusals come before any HIP call."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_exported_and_bound(pkg):
    hdr = open(os.path.join(ROOT, "include", "biogpt_hip.h")).read()
    bound = {name for name, _, _ in pkg.SYMBOLS}
    raw = ctypes.CDLL(pkg.LIB_PATH)
    for name in ("biogpt_hip_chain_kind", "biogpt_hip_wide_launches", "biogpt_hip_wide_chain_device"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in bound, name
        assert getattr(raw, name) is not None
    for name in ("bg_wide_launch", "bg_wide_quantize"):      # the wide chain's own translation unit is linked in
        assert getattr(raw, name) is not None
    assert hasattr(pkg.BiogptModel, "chain_kind") and hasattr(pkg.BiogptModel, "wide_launches")


def test_null_context_is_rejected(pkg):
    assert pkg.lib().biogpt_hip_wide_launches(None) == -1
    assert pkg.lib().biogpt_hip_chain_kind(None) == -1
    assert b"null context" in pkg.lib().biogpt_hip_last_error()


def test_probe_refuses_before_any_launch(pkg):
    K, M, N = 96, 192, 1
    z = dict(wtype=2, M=M, K=K, N=N, w_rows=np.zeros(M * (K // 32) * 18, np.uint8), aq_q=np.zeros((N, K), np.int8), aq_d=np.zeros((N, K // 32), np.float32),
             aq_s=np.zeros((N, K // 32), np.uint32), bias=np.zeros(M, np.float32))
    for epi, kw, text in (("GELU", dict(M=200), "whole number of 16-row tiles"), ("GELU", dict(K=100), "multiple of 32"), ("GELU", dict(wtype=0), "no block format"),
                          ("LOGITS", dict(N=0), r"N must be in \[1, 512\]"), ("RESID", {}, "resid is NULL"), ("GELU", dict(bias=None), "bias is NULL"),
                          ("GELU", dict(dev_state=np.zeros(4, np.int32)), "only QKV reads column states")):
        with pytest.raises(pkg.BiogptError, match=text):
            pkg.wide_chain_device(epi=epi, **dict(z, **kw))
    kv = np.zeros((1, 1, 1, 64), np.float32)
    with pytest.raises(pkg.BiogptError, match="3 K x K"):
        pkg.wide_chain_device(epi="QKV", dev_state=np.zeros(4, np.int32), P=1, k_slots=kv, v_slots=kv, **z)
    q = dict(z, K=64, M=192, w_rows=np.zeros(192 * 2 * 18, np.uint8), aq_q=np.zeros((1, 64), np.int8), aq_d=np.zeros((1, 2), np.float32), aq_s=np.zeros((1, 2), np.uint32))
    with pytest.raises(pkg.BiogptError, match="exactly one of dev_state and seq_states"):
        pkg.wide_chain_device(epi="QKV", P=1, k_slots=kv, v_slots=kv, **q)
    with pytest.raises(pkg.BiogptError, match=r"position 1 outside \[0, P\)"):
        pkg.wide_chain_device(epi="QKV", dev_state=np.array([1, 0, 0, 0], np.int32), P=1, k_slots=kv, v_slots=kv, **q)
