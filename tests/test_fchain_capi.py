"""The float chain's public symbols without a GPU: biogpt_hip_float_chain and biogpt_hip_float_launches (and the probe of the kernel alone,
biogpt_hip_fchain_device, with its timing twin) are declared, exported and bound; the first two reject a null context; the probe's refusals come before any
HIP call."""
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
    for name in ("biogpt_hip_float_chain", "biogpt_hip_float_launches", "biogpt_hip_fchain_device", "biogpt_hip_fchain_bench"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in bound, name
        assert getattr(raw, name) is not None
    for name in ("bg_fchain_launch", "bg_fchain_ln", "bg_fchain_cfg"):      # the float chain's own translation unit is linked in
        assert getattr(raw, name) is not None
    assert hasattr(pkg.BiogptModel, "float_chain") and hasattr(pkg.BiogptModel, "float_launches")
    assert "float_chain" in pkg.BiogptModel.load.__func__.__code__.co_varnames


def test_null_context_is_rejected(pkg):
    assert pkg.lib().biogpt_hip_float_launches(None) == -1
    assert pkg.lib().biogpt_hip_float_chain(None, 1) == -1
    assert b"null context" in pkg.lib().biogpt_hip_last_error()
    assert pkg.lib().biogpt_hip_float_chain(None, 0) == -1


def test_the_launch_picks_the_largest_tile_that_fills_the_chip(pkg):
    """bg_fchain_cfg: 64 x 16 tiles from 512 workgroups of them, else 32 x 8 from 512, else 4 x 8."""
    raw = ctypes.CDLL(pkg.LIB_PATH)
    seen = set()
    for M, N in ((1024, 8), (1024, 64), (1024, 128), (1024, 512), (4096, 64), (4096, 128), (3072, 160), (3072, 176), (42384, 8), (42384, 1), (192, 1), (2053, 33)):
        grids = [-(-M // 4) * -(-N // 8), -(-M // 32) * -(-N // 8), -(-M // 64) * -(-N // 16)]
        want = 2 if grids[2] >= 512 else 1 if grids[1] >= 512 else 0
        assert raw.bg_fchain_cfg(M, N) == want, (M, N, grids)
        seen.add(want)
    assert seen == {0, 1, 2}


def test_probe_refuses_before_any_launch(pkg):
    K, M, N = 96, 192, 1
    z = dict(wtype=0, M=M, K=K, N=N, w_rows=np.zeros((M, K), np.float32), x=np.zeros((N, K), np.float32), bias=np.zeros(M, np.float32))
    for epi, kw, text in (("GELU", dict(K=100), "multiple of 32"), ("GELU", dict(wtype=2), "no float format"), ("LOGITS", dict(N=0), r"N must be in \[1, 512\]"),
                          ("RESID", {}, "resid is NULL"), ("GELU", dict(bias=None), "bias is NULL"), ("GELU", dict(cfg=3), r"cfg must be in \[-1, 2\]"),
                          ("GELU", dict(ln_w=np.ones(K, np.float32)), "ln_w and ln_b come together"),
                          ("GELU", dict(dev_state=np.zeros(4, np.int32)), "only QKV reads column states")):
        with pytest.raises(pkg.BiogptError, match=text):
            pkg.fchain_device(epi=epi, **dict(z, **kw))
    kv = np.zeros((1, 1, 1, 64), np.float32)
    with pytest.raises(pkg.BiogptError, match="3 K x K"):
        pkg.fchain_device(epi="QKV", dev_state=np.zeros(4, np.int32), P=1, k_slots=kv, v_slots=kv, **z)
    q = dict(z, K=64, M=192, w_rows=np.zeros((192, 64), np.float32), x=np.zeros((1, 64), np.float32))
    with pytest.raises(pkg.BiogptError, match="exactly one of dev_state and seq_states"):
        pkg.fchain_device(epi="QKV", P=1, k_slots=kv, v_slots=kv, **q)
    with pytest.raises(pkg.BiogptError, match=r"position 1 outside \[0, P\)"):
        pkg.fchain_device(epi="QKV", dev_state=np.array([1, 0, 0, 0], np.int32), P=1, k_slots=kv, v_slots=kv, **q)
