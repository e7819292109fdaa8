"""Shared-prefix scoring of many groups in one call, without a device: the symbols of biogpt_hip_score_continuations_batch and its companions are exported
and bound, the Python wrappers exist, a null context fails before any device is touched, and the cutting of a dataset into calls of at most 512 slots."""
import ctypes as C

import numpy as np
import pytest

SYMBOLS = ["biogpt_hip_score_continuations_batch", "biogpt_hip_prefix_batch_stats", "biogpt_hip_attn_runs_plan", "biogpt_hip_attn_runs_device",
           "biogpt_hip_attn_runs_bench"]


def test_symbols_are_exported_and_bound(pkg):
    lib = pkg.lib()
    for name in SYMBOLS:
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and fn.argtypes, name
    assert len(lib.biogpt_hip_score_continuations_batch.argtypes) == 11
    assert len(lib.biogpt_hip_attn_runs_device.argtypes) == 18 and len(lib.biogpt_hip_attn_runs_bench.argtypes) == 20


def test_python_wrappers_exist(pkg):
    for name in ("score_continuations_batch", "rank_continuations_batch", "prefix_batch_stats"):
        assert callable(getattr(pkg.BiogptModel, name)), name
    for name in ("attn_runs_plan", "attn_runs_device", "prefix_batch_chunks"):
        assert callable(getattr(pkg, name)), name


def test_null_context_fails_without_a_device(pkg):
    a = np.array([2, 5, 9], dtype=np.int32)
    one = np.array([1], dtype=np.int32)
    out = np.zeros(4, dtype=np.float32)
    rc = pkg.lib().biogpt_hip_score_continuations_batch(None, a.ctypes.data, np.array([3], dtype=np.int32).ctypes.data, 1, a.ctypes.data, one.ctypes.data,
                                                        one.ctypes.data, out.ctypes.data, None, None, None)
    assert rc == -1 and "null context" in pkg._err()
    stats = np.zeros(4, dtype=np.int32)
    assert pkg.lib().biogpt_hip_prefix_batch_stats(None, stats.ctypes.data) == -1 and "null context" in pkg._err()


def test_chunking_of_a_dataset(pkg):
    chunks = pkg.prefix_batch_chunks
    assert chunks([]) == []
    assert chunks([3] * 128) == [(0, 128)]                                  # 128 * (1 + 3) = 512 slots: one call
    assert chunks([3] * 127 + [4]) == [(0, 127), (127, 128)]                # 513 slots: two calls, order kept
    assert chunks([511]) == [(0, 1)]
    assert chunks([255, 255, 255]) == [(0, 2), (2, 3)]
    assert chunks([1] * 600) == [(0, 256), (256, 512), (512, 600)]
    assert chunks([510, 1, 1]) == [(0, 1), (1, 3)]
    with pytest.raises(pkg.BiogptError, match="group 2 alone needs 513 slots"):
        chunks([3, 3, 512, 3])
    assert chunks([2, 5], max_slots=6) == [(0, 1), (1, 2)]


class _Stub:
    """score_continuations_batch over a stub of the library call: records each call's groups and returns each target's flat index in the dataset."""

    def __init__(self, pkg, calls):
        self._h, self.calls, self.at = None, calls, 0
        self.pkg = pkg

    def call(self, h, prefixes, prefix_lens, n_groups, conts, cont_lens, n_conts, lp, am, lg, secs):
        ncs = np.ctypeslib.as_array(C.cast(C.c_void_p(n_conts), C.POINTER(C.c_int32)), (n_groups,)).copy()
        lens = np.ctypeslib.as_array(C.cast(C.c_void_p(cont_lens), C.POINTER(C.c_int32)), (int(ncs.sum()),)).copy()
        total = int(lens.sum())
        self.calls.append((n_groups, ncs.tolist(), lens.tolist()))
        np.ctypeslib.as_array(C.cast(C.c_void_p(lp), C.POINTER(C.c_float)), (total,))[:] = np.arange(self.at, self.at + total)
        self.at += total
        return 0


def test_score_continuations_batch_cuts_513_slots_into_two_calls(pkg, monkeypatch):
    calls = []
    stub = _Stub(pkg, calls)

    class Lib:
        biogpt_hip_score_continuations_batch = staticmethod(stub.call)

    monkeypatch.setattr(pkg, "lib", lambda: Lib)
    prefixes = [[2, 4 + g] for g in range(128)]
    conts = [[[5], [6, 7], [8]] for _ in range(127)] + [[[5], [6], [7], [8, 9, 10]]]
    m = pkg.BiogptModel.__new__(pkg.BiogptModel)
    m._h = None
    got = pkg.BiogptModel.score_continuations_batch(m, prefixes, conts)
    assert [c[0] for c in calls] == [127, 1] and calls[1][1] == [4] and calls[1][2] == [1, 1, 1, 3]
    assert m.prefix_batch_calls == 2
    assert [len(g) for g in got] == [3] * 127 + [4]
    flat = np.concatenate([lp for g in got for lp, _, _ in g])
    assert (flat == np.arange(flat.size)).all()                            # order kept across the calls
    assert [len(lp) for lp, _, _ in got[-1]] == [1, 1, 1, 3]
    with pytest.raises(pkg.BiogptError, match="alone needs 513 slots"):
        pkg.BiogptModel.score_continuations_batch(m, [[2]], [[[5]] * 512])
    with pytest.raises(pkg.BiogptError, match="one entry per prefix"):
        pkg.BiogptModel.score_continuations_batch(m, [[2], [3]], [[[5]]])
