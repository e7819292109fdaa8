"""The SIMD association's C ABI without a GPU: the switch (biogpt_hip_assoc / biogpt_hip_get_assoc) and the probe of its kernels (biogpt_hip_assoc_device) are
declared, exported and bound; a null context and a mode outside {0, 1} are refused; every refusal of the probe comes before any HIP call and names the field
(there is no device here: a HIP call would make the result -2)."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
Q4_0 = 2


@pytest.mark.parametrize("name", ["biogpt_hip_assoc", "biogpt_hip_get_assoc", "biogpt_hip_assoc_device"])
def test_symbols_exported_and_bound(pkg, name):
    hdr = open(os.path.join(ROOT, "include", "biogpt_hip.h")).read()
    assert re.search(r"\b%s\s*\(" % name, hdr)
    assert name in {n for n, _, _ in pkg.SYMBOLS}
    assert getattr(ctypes.CDLL(pkg.LIB_PATH), name) is not None
    assert getattr(pkg.lib(), name).restype is ctypes.c_int


def test_python_surface(pkg):
    assert callable(pkg.assoc_device) and callable(pkg.BiogptModel.set_assoc) and isinstance(pkg.BiogptModel.assoc, property)
    assert pkg.ASSOC_MODES == {"scalar": 0, "simd": 1}


def test_null_context_is_refused(pkg):
    for mode in (0, 1):
        assert pkg.lib().biogpt_hip_assoc(None, mode) == -1
        assert b"null context" in pkg.lib().biogpt_hip_last_error()
    assert pkg.lib().biogpt_hip_get_assoc(None) == -1


def test_mode_outside_0_1_is_refused_with_a_message(pkg):
    # (no device, so no context: the arguments are checked in front of everything a context holds, and a block of zeros stands in for the handle)
    buf = ctypes.create_string_buffer(1 << 16)
    for mode in (-1, 2, 7):
        assert pkg.lib().biogpt_hip_assoc(ctypes.cast(buf, ctypes.c_void_p), mode) == -1
        msg = pkg.lib().biogpt_hip_last_error()
        assert b"mode must be 0" in msg and str(mode).encode() in msg


x32 = np.zeros((1, 32), F32)
w1 = np.zeros(18, np.uint8)
REFUSALS = [
    ("unknown stage", dict(stage=3, wtype=Q4_0, K=32, x=x32), "stage 3 is no stage"),
    ("negative stage", dict(stage=-1, wtype=Q4_0, K=32, x=x32), "stage -1 is no stage"),
    ("float type (Q8)", dict(stage="Q8", wtype=0, K=32, x=x32), "type 0 is no block format"),
    ("float type (MATVEC)", dict(stage="MATVEC", wtype=1, M=1, K=32, x=x32, w_rows=w1, epi="RESID"), "type 1 is no block format"),
    ("unknown type", dict(stage="MATVEC", wtype=5, M=1, K=32, x=x32, w_rows=w1, epi="RESID"), "type 5 is no block format"),
    ("K no multiple of 32 (Q8)", dict(stage="Q8", wtype=Q4_0, K=48, x=np.zeros((1, 48), F32)), "K must be a multiple of 32"),
    ("K no multiple of 32 (MATVEC)", dict(stage="MATVEC", wtype=Q4_0, M=1, K=40, x=np.zeros((1, 40), F32), w_rows=w1, epi="RESID"), "K must be a multiple of 32"),
    ("K zero", dict(stage="Q8", wtype=Q4_0, K=0, N=1, x=x32), "K must be a multiple of 32"),
    ("N zero", dict(stage="Q8", wtype=Q4_0, K=32, N=0, x=x32), r"N must be in \[1, 8\]"),
    ("N nine (Q8)", dict(stage="Q8", wtype=Q4_0, K=32, x=np.zeros((9, 32), F32)), r"N must be in \[1, 8\]"),
    ("N nine (MATVEC)", dict(stage="MATVEC", wtype=Q4_0, M=1, K=32, x=np.zeros((9, 32), F32), w_rows=w1, epi="RESID", bias=np.zeros(1, F32),
                             resid=np.zeros((9, 1), F32)), r"N must be in \[1, 8\]"),
    ("x missing", dict(stage="Q8", wtype=Q4_0, K=32, N=1), "x is NULL"),
    ("ln_b missing", dict(stage="Q8", wtype=Q4_0, K=32, x=x32, ln_w=np.zeros(32, F32)), "ln_w and ln_b come together"),
    ("LN with the residual epilogue", dict(stage="MATVEC", wtype=Q4_0, M=1, K=32, x=x32, w_rows=w1, epi="RESID", ln_w=np.zeros(32, F32), ln_b=np.zeros(32, F32),
                                           bias=np.zeros(1, F32), resid=np.zeros((1, 1), F32)), "no site of the layer"),
    ("PLAIN with GELU", dict(stage="MATVEC", wtype=Q4_0, M=1, K=32, x=x32, w_rows=w1, epi="GELU", bias=np.zeros(1, F32)), "no site of the layer"),
    ("unknown epilogue", dict(stage="MATVEC", wtype=Q4_0, M=1, K=32, x=x32, w_rows=w1, epi=4), "epi 4 is no epilogue"),
    ("M zero", dict(stage="MATVEC", wtype=Q4_0, M=0, K=32, x=x32, w_rows=w1, epi="RESID", bias=np.zeros(1, F32), resid=np.zeros((1, 1), F32)), "M must be in"),
    ("bias missing", dict(stage="MATVEC", wtype=Q4_0, M=1, K=32, x=x32, w_rows=w1, epi="RESID", resid=np.zeros((1, 1), F32)), "bias is NULL"),
    ("resid missing", dict(stage="MATVEC", wtype=Q4_0, M=1, K=32, x=x32, w_rows=w1, epi="RESID", bias=np.zeros(1, F32)), "resid is NULL"),
    ("weights missing", dict(stage="MATVEC", wtype=Q4_0, M=1, K=32, x=x32, epi="RESID", bias=np.zeros(1, F32), resid=np.zeros((1, 1), F32)), "w_rows or out is NULL"),
    ("q/k/v of another shape", dict(stage="MATVEC", wtype=Q4_0, M=64, K=64, x=np.zeros((1, 64), F32), w_rows=np.zeros(64 * 2 * 18, np.uint8), epi="QKV",
                                    ln_w=np.zeros(64, F32), ln_b=np.zeros(64, F32), bias=np.zeros(64, F32), dev_state=[0, 0, 0, 0], P=4,
                                    k_slots=np.zeros((1, 4, 64), F32), v_slots=np.zeros((1, 4, 64), F32)), "q/k/v is 3 K x K"),
    ("q/k/v position outside the table", dict(stage="MATVEC", wtype=Q4_0, M=192, K=64, x=np.zeros((2, 64), F32), w_rows=np.zeros(192 * 2 * 18, np.uint8), epi="QKV",
                                              ln_w=np.zeros(64, F32), ln_b=np.zeros(64, F32), bias=np.zeros(192, F32), dev_state=[3, 0, 0, 0], P=4,
                                              k_slots=np.zeros((1, 4, 64), F32), v_slots=np.zeros((1, 4, 64), F32)), r"position 4 outside \[0, P\)"),
    ("column states without q/k/v", dict(stage="MATVEC", wtype=Q4_0, M=1, K=32, x=x32, w_rows=w1, epi="RESID", bias=np.zeros(1, F32), resid=np.zeros((1, 1), F32),
                                         dev_state=[0, 0, 0, 0]), "only QKV reads column states"),
    ("partials of two columns", dict(stage="MATVEC", wtype=Q4_0, M=1, K=32, x=np.zeros((2, 32), F32), w_rows=w1, epi="LOGITS", ln_w=np.zeros(32, F32),
                                     ln_b=np.zeros(32, F32), partials=True), "of one column"),
    ("T beyond 1024", dict(stage="ATTN", H=1, P=2048, q=np.zeros((1, 64), F32), k_slots=np.zeros((1, 2048, 64), F32), v_slots=np.zeros((1, 2048, 64), F32),
                           dev_state=[1024, 0, 0, 0]), r"sees T = 1025 keys: the kernel holds 1 \.\. 1024"),
    ("T beyond the table", dict(stage="ATTN", H=1, P=8, q=np.zeros((2, 64), F32), k_slots=np.zeros((1, 8, 64), F32), v_slots=np.zeros((1, 8, 64), F32),
                                dev_state=[7, 0, 0, 0]), "sees 9 keys of a table of P = 8 rows"),
    ("no heads", dict(stage="ATTN", H=0, P=8, q=np.zeros((1, 64), F32), k_slots=np.zeros((1, 8, 64), F32), v_slots=np.zeros((1, 8, 64), F32), dev_state=[0, 0, 0, 0]),
     r"H must be in \[1, 64\]"),
    ("state missing", dict(stage="ATTN", H=1, P=8, q=np.zeros((1, 64), F32), k_slots=np.zeros((1, 8, 64), F32), v_slots=np.zeros((1, 8, 64), F32)), "dev_state or out is NULL"),
]


@pytest.mark.parametrize("what,kw,text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_probe_refuses_before_any_hip_call(pkg, what, kw, text):
    with pytest.raises(pkg.BiogptError, match=text):
        pkg.assoc_device(**kw)


def test_probe_refusal_returns_minus_one(pkg):
    rc = pkg.lib().biogpt_hip_assoc_device(0, 9, Q4_0, 0, 0, 1, 32, 1, 0, 0, *([None] * 17))
    assert rc == -1 and b"no stage" in pkg.lib().biogpt_hip_last_error()
    rc = pkg.lib().biogpt_hip_assoc_device(0, 0, Q4_0, 0, 0, 1, 33, 1, 0, 0, *([None] * 17))
    assert rc == -1 and b"K must be a multiple of 32" in pkg.lib().biogpt_hip_last_error()
