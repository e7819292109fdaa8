"""The probe of the chain's linear stages (biogpt_hip_chain_device) and the matrix-core launch counter without a GPU: the C-ABI is exported and bound, and
every refusal -- a shape that is not the site's own, a route the engine would not take, two columns on one cache row -- comes before any HIP call."""
import ctypes
import os
import re

import numpy as np
import pytest

import chain_cases as C
import chain_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_exported_and_bound(pkg):
    hdr = open(os.path.join(ROOT, "include", "biogpt_hip.h")).read()
    bound = {name for name, _, _ in pkg.SYMBOLS}
    raw = ctypes.CDLL(pkg.LIB_PATH)
    for name in ("biogpt_hip_chain_device", "biogpt_hip_mfma_launches"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in bound, name
        assert getattr(raw, name) is not None
    assert pkg.lib().biogpt_hip_mfma_launches(None) == -1
    assert raw.bg_mfma_tiles is not None


def test_the_two_tile_rule_is_the_one_the_cases_state(pkg):
    """bg_mfma_tiles (mfma_tu.hip) against chain_cases.two_tiles on both sides of every border, for every format and site."""
    raw = ctypes.CDLL(pkg.LIB_PATH)
    site = {"QKV": 0, "OPROJ": 1, "FC1_Q8": 2, "FC2": 3, "LMHEAD": 4}
    for op, s in site.items():
        M = C.shape_of(op, 1040)[0]
        for wt in R.TYPES:
            for N in (48, 64, 240, 241, 257, 336, 337, 353, 512):
                assert raw.bg_mfma_tiles(wt, s, M, N) == (2 if C.two_tiles(op, wt, M, N) else 1), (op, wt, N)
    assert C.two_tiles("FC1_Q8", R.Q4_0, 4096, 241) and not C.two_tiles("FC1_Q8", R.Q4_0, 4096, 240)
    assert C.two_tiles("QKV", R.Q8_0, 3072, 337) and not C.two_tiles("QKV", R.Q8_0, 3072, 336)
    assert not C.two_tiles("FC1_Q8", R.Q5_1, 4096, 512) and raw.bg_mfma_tiles(99, 0, 3072, 512) == 0


@pytest.fixture(scope="module")
def base():
    """Arguments of valid launches, small enough to build at once (the weights are zero bytes: nothing reads them before a refusal)."""
    def args(op, N, wtype=R.Q4_0, M=None, **kw):
        M, K = C.shape_of(op, M or 1040)
        a = dict(op=op, wtype=wtype, M=M, N=N, w_rows=np.zeros(M * (K // 32) * R.BLOCK_BYTES[wtype], np.uint8), aq_q=np.zeros((N, K), np.int8),
                 aq_d=np.zeros((N, K // 32), np.float32), aq_s=np.zeros((N, K // 32), np.uint32))
        if op != "LMHEAD":
            a["bias"] = np.zeros(M, np.float32)
        if op in ("OPROJ", "FC2"):
            a["resid"] = np.zeros((N, M), np.float32)
        if op == "QKV":
            a.update(dev_state=np.array([0, 0, 0, 0], np.int32), P=N, k_slots=np.zeros((1, 16, N, 64), np.float32), v_slots=np.zeros((1, 16, N, 64), np.float32))
        a.update(kw)
        return a
    return args


def refused(pkg, field, **a):
    with pytest.raises(pkg.BiogptError) as e:
        pkg.chain_device(**a)
    assert field in str(e.value), (field, str(e.value))


def test_shapes_that_are_not_the_sites_own(pkg, base):
    for op, M in (("QKV", 1024), ("OPROJ", 1040), ("FC1_Q8", 1024), ("FC2", 4096)):
        a = base(op, 8)
        a["M"] = M
        refused(pkg, "not the site's own shape", route="VALU_8", **a)
    a = base("LMHEAD", 8)
    a["M"] = 0
    refused(pkg, "M must be", route="VALU_8", **a)
    for field, key, val in (("no block format", "wtype", 1), ("N must be", "N", 513), ("N must be", "N", 0)):
        a = base("OPROJ", 8)
        a[key] = val
        refused(pkg, field, route="VALU_8", **a)
    refused(pkg, "bias is NULL", route="VALU_8", **base("OPROJ", 8, bias=None))
    refused(pkg, "resid is NULL", route="VALU_8", **base("FC2", 8, resid=None))
    refused(pkg, "aq_q", route="VALU_8", **base("LMHEAD", 8, aq_d=None))


def test_routes_the_engine_would_not_take(pkg, base):
    refused(pkg, "from 48 columns on", route="MFMA_1", **base("OPROJ", 47))
    refused(pkg, "from 48 columns on", route="MFMA_1", **base("LMHEAD", 47))
    refused(pkg, "from 64 columns on", route="MFMA_1", **base("QKV", 63))                       # the context's own columns: a pass, not a decode step
    st = np.zeros((63, 8), np.int32)
    st[:, 3] = st[:, 0] = np.arange(63)
    packed = dict(dev_state=None, seq_states=st, col_mode=1, P=63, k_slots=np.zeros((63, 16, 63, 64), np.float32), v_slots=np.zeros((63, 16, 63, 64), np.float32))
    refused(pkg, "from 64 columns on", route="MFMA_1", **base("QKV", 63, **packed))
    refused(pkg, "whole number of 16-row tiles", route="MFMA_1", **base("LMHEAD", 64, M=1045))
    refused(pkg, "whole number of 16-row tiles", route="MFMA_1", **base("LMHEAD", 64, M=1043))
    refused(pkg, "1 row tile(s)", route="MFMA_2", **base("FC1_Q8", 240))                          # one tile short of the switch
    refused(pkg, "2 row tile(s)", route="MFMA_1", **base("FC1_Q8", 241))
    refused(pkg, "1 row tile(s)", route="MFMA_2", **base("FC1_Q8", 512, wtype=R.Q4_1))            # no two-tile form with a min term
    refused(pkg, "1 row tile(s)", route="MFMA_2", **base("QKV", 336))
    refused(pkg, "2 row tile(s)", route="MFMA_1", **base("QKV", 337))
    refused(pkg, "1 row tile(s)", route="MFMA_2", **base("OPROJ", 512))
    refused(pkg, "1-column kernel serves", route="VALU_1", **base("OPROJ", 2))
    refused(pkg, "1-column kernel serves", route="VALU_1", **base("QKV", 1))
    refused(pkg, "1-column kernel serves", route="VALU_1", **base("LMHEAD", 1))
    refused(pkg, "1-column kernel serves", route="VALU_1", **base("FC1_Q8", 1))
    refused(pkg, "takes the 1-column kernel", route="VALU_8", **base("FC2", 1))
    x = np.zeros((2, 1024), np.float32)
    ln = dict(op="FC1_LN", wtype=R.Q4_0, M=4096, w_rows=np.zeros(4096 * 32 * 18, np.uint8), x=x, ln_w=x[0], ln_b=x[0], bias=np.zeros(4096, np.float32))
    refused(pkg, "1-column kernel alone", route="VALU_1", N=2, **ln)
    refused(pkg, "1-column kernel alone", route="VALU_8", N=1, **ln)
    refused(pkg, "only QKV reads column states", route="VALU_8", **base("OPROJ", 8, dev_state=np.zeros(4, np.int32)))
    refused(pkg, "q81 must be", op="LNQ", N=2, x=x, ln_w=x[0], ln_b=x[0], q81=2)
    refused(pkg, "x, ln_w or ln_b", op="LNQ", N=2, x=x, ln_w=None, ln_b=x[0])


def test_column_states_of_qkv(pkg, base):
    refused(pkg, "exactly one", route="VALU_8", **base("QKV", 8, dev_state=None))
    refused(pkg, "position 8 outside", route="VALU_8", **base("QKV", 8, dev_state=np.array([1, 0, 0, 0], np.int32)))
    refused(pkg, "position -1 outside", route="VALU_8", **base("QKV", 8, dev_state=np.array([-1, 0, 0, 0], np.int32)))
    refused(pkg, "one slot", route="VALU_8", **base("QKV", 8, k_slots=np.zeros((2, 16, 8, 64), np.float32), v_slots=np.zeros((2, 16, 8, 64), np.float32)))
    st = np.zeros((8, 8), np.int32)
    st[:, 0] = [0, 1, 2, 3, 0, 1, 2, 3]
    st[:, 3] = [0, 0, 0, 0, 1, 1, 1, 1]
    kv = dict(k_slots=np.zeros((2, 16, 4, 64), np.float32), v_slots=np.zeros((2, 16, 4, 64), np.float32))
    ok = dict(dev_state=None, seq_states=st, col_mode=1, P=4, **kv)
    two = st.copy()
    two[5, 0] = 0                                                                                 # columns 4 and 5 both write slot 1, position 0
    refused(pkg, "a second column writes slot 1, position 0", route="VALU_8", **base("QKV", 8, **dict(ok, seq_states=two)))
    far = st.copy()
    far[7, 3] = 2
    refused(pkg, "slot 2 outside", route="VALU_8", **base("QKV", 8, **dict(ok, seq_states=far)))
    refused(pkg, "slot 2 outside", route="VALU_8", **base("QKV", 8, **dict(ok, col_mode=0)))     # col_mode 0: column i writes slot i
    refused(pkg, "col_mode 1 needs seq_states", route="VALU_8", **base("QKV", 8, col_mode=1))


def test_expected_geometry_of_the_cases():
    """The launch geometry the GPU test expects, at the values read off the launch code: workgroups of 256 threads (320 with the staging wave of K = 4096),
    64 * J rows x 16 columns per matrix-core workgroup, 4 * rpw rows x 8 columns per VALU workgroup."""
    assert C.expected_launch("FC1_Q8", "MFMA_2", R.Q4_0, 4096, 1024, 241)[:4] == (3, 256, 32, 16)
    assert C.expected_launch("FC1_Q8", "MFMA_1", R.Q4_1, 4096, 1024, 241)[:4] == (2, 256, 64, 16)
    assert C.expected_launch("FC2", "MFMA_1", R.Q8_0, 1024, 4096, 512)[:4] == (2, 320, 16, 32)
    assert C.expected_launch("LMHEAD", "MFMA_1", R.Q5_0, 1040, 1024, 49)[:4] == (2, 256, 17, 4)
    assert C.expected_launch("LMHEAD", "VALU_8", R.Q5_0, 1045, 1024, 9)[:4] == (1, 256, 33, 2)
    assert C.expected_launch("QKV", "VALU_8", R.Q5_0, 3072, 1024, 17)[:4] == (1, 256, 384, 3)
    assert C.expected_launch("OPROJ", "VALU_1", R.Q5_0, 1024, 1024, 1)[:4] == (0, 256, 128, 1)
    assert C.expected_launch("FC2", "VALU_8", R.Q5_0, 1024, 4096, 8)[:4] == (1, 256, 256, 1)
    assert C.expected_launch("FC1_LN", "VALU_1", R.Q5_0, 4096, 1024, 1)[:4] == (0, 256, 128, 1)


def _qkv_probes(pkg, N, **states):
    """One QKV launch of each linear-stage probe on the same column states (zero weights: nothing reads them before a refusal)."""
    n_slots = states.pop("n_slots", 1)
    P = states["P"]
    z = lambda *s: np.zeros(s, np.float32)
    big = dict(k_slots=z(n_slots, 16, P, 64), v_slots=z(n_slots, 16, P, 64), **states)
    small = dict(k_slots=z(n_slots, 1, P, 64), v_slots=z(n_slots, 1, P, 64), **states)
    aq = lambda K: dict(aq_q=np.zeros((N, K), np.int8), aq_d=z(N, K // 32), aq_s=np.zeros((N, K // 32), np.uint32))
    return (
        lambda: pkg.chain_device(op="QKV", route="VALU_8", wtype=R.Q4_0, M=3072, N=N, w_rows=np.zeros(3072 * 32 * R.BLOCK_BYTES[R.Q4_0], np.uint8), bias=z(3072), **aq(1024), **big),
        lambda: pkg.wide_chain_device("QKV", R.Q4_0, 192, 64, N, np.zeros(192 * 2 * R.BLOCK_BYTES[R.Q4_0], np.uint8), bias=z(192), **aq(64), **small),
        lambda: pkg.fchain_device("QKV", 0, 192, 64, N, z(192, 64), z(N, 64), bias=z(192), **small),
    )


def _packed(N=8, P=4):
    st = np.zeros((N, 8), np.int32)
    st[:, 0] = np.arange(N) % P        # n_past
    st[:, 3] = np.arange(N) // P       # seq_id
    return st


def _with(st, row, word, val):
    st = st.copy()
    st[row, word] = val
    return st


COLUMN_REFUSALS = {
    "neither": ("exactly one of dev_state and seq_states names the column states", dict(dev_state=None, seq_states=None, P=8)),
    "both": ("exactly one of dev_state and seq_states names the column states", dict(dev_state=np.zeros(4, np.int32), seq_states=_packed(), col_mode=1, P=4, n_slots=2)),
    "col_mode 2": ("col_mode must be 0 or 1", dict(seq_states=_packed(), col_mode=2, P=4, n_slots=2)),
    "slot": ("column 7: slot 2 outside [0, n_slots)", dict(seq_states=_with(_packed(), 7, 3, 2), col_mode=1, P=4, n_slots=2)),
    "position": ("column 6: position 4 outside [0, P)", dict(seq_states=_with(_packed(), 6, 0, 4), col_mode=1, P=4, n_slots=2)),
    "one row": ("column 5: a second column writes slot 1, position 0", dict(seq_states=_with(_packed(), 5, 0, 0), col_mode=1, P=4, n_slots=2)),
}


@pytest.mark.parametrize("case", sorted(COLUMN_REFUSALS))
def test_the_three_linear_stage_probes_refuse_column_states_alike(pkg, case):
    """The chain, wide-chain and float-chain probes check a QKV launch's column states by one rule: the same refusal, word for word, from all three, each
    under its own entry's name."""
    text, states = COLUMN_REFUSALS[case]
    said = []
    for call in _qkv_probes(pkg, 8, **states):
        with pytest.raises(pkg.BiogptError) as e:
            call()
        said.append(str(e.value).split(": ", 1))
    assert [s[0] for s in said] == ["biogpt_hip_chain_device", "biogpt_hip_wide_chain_device", "biogpt_hip_fchain_device"], said
    assert said[0][1] == said[1][1] == said[2][1], said
    assert text in said[0][1], (text, said[0][1])
