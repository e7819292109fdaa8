"""The C interface of the wide column layer without a GPU: the new symbols of include/biogpt_hip.h exist with their signatures, a null context is refused, and
the launch geometry (bg_wcols_geometry, through the probe's report without any rows: no HIP call) is the one csrc/kernels_wcols.hip.h describes."""
import ctypes as C
import os
import re

import pytest


def test_symbols_and_signatures(pkg):
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "biogpt_hip.h")).read()
    for name, res, n_args in (("biogpt_hip_wide_cols", C.c_int, 2), ("biogpt_hip_get_wide_cols", C.c_int, 1), ("biogpt_hip_wide_cols_launches", C.c_int64, 1),
                              ("biogpt_hip_wcols_device", C.c_int, 25)):
        f = getattr(pkg.lib(), name)
        assert f.restype is res and len(f.argtypes) == n_args, name
        decl = re.search(r"%s(\(([^;]*)\));" % name, header)
        assert decl and decl.group(2).count(",") + 1 == n_args, name      # the declaration has the arguments the binding passes
    assert pkg.lib().biogpt_hip_wide_cols_launches(None) == -1
    assert pkg.lib().biogpt_hip_wide_cols(None, 1) == -1 and pkg.lib().biogpt_hip_get_wide_cols(None) == -1
    assert callable(pkg.wcols_device) and callable(pkg.BiogptModel.set_wide_cols) and callable(pkg.BiogptModel.wide_cols_launches)


# (epi, M, K, N, nw forced) -> waves, threads, grid (row tiles), LDS bytes (a ring of 2 x 4 nw blocks x 256 f32), rounds of 4 nw blocks
@pytest.mark.parametrize("epi,M,K,N,nw,want", [
    ("RESID", 48, 96, 1, 0, (4, 256, 3, 32768, 1)),           # 3 blocks: fewer than a round
    ("LOGITS", 77, 1600, 5, 0, (8, 512, 5, 65536, 2)),        # 50 blocks: 32 + 18; a zero-padded fifth tile
    ("LOGITS", 77, 1600, 5, 4, (4, 256, 5, 32768, 4)),        # 16 + 16 + 16 + 2
    ("RESID", 48, 6400, 16, 0, (8, 512, 3, 65536, 7)),        # 200 blocks: 6 x 32 + 8
    ("RESID", 48, 6400, 16, 4, (4, 256, 3, 32768, 13)),
    ("QKV", 4800, 1600, 8, 0, (8, 512, 300, 65536, 2)),
])
def test_geometry(pkg, epi, M, K, N, nw, want):
    got = pkg.wcols_device(epi, 2, M, K, N, nw=nw)["launched"]
    assert tuple(got[:5]) == want and tuple(got[5:7]) == (17, ((M + 127) & ~127) + 16)


@pytest.mark.parametrize("kw,text", [(dict(N=17), "holds 1 .. 16"), (dict(N=0), "holds 1 .. 16"), (dict(K=100), "multiple of 32"), (dict(M=77), "does not hold"),
                                     (dict(nw=2), "nw must be"), (dict(epi="QKV"), "does not hold")])
def test_refusals_come_before_any_hip_call(pkg, kw, text):
    a = dict(dict(epi="RESID", wtype=2, M=48, K=96, N=1), **kw)
    with pytest.raises(pkg.BiogptError, match=text):
        pkg.wcols_device(**a)
