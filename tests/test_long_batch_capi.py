"""The C interface of the batched calls beyond 1024 keys without a GPU: the new symbols of include/biogpt_hip.h exist with their signatures, the run planner of
attn_long_runs_kernel gives the expected runs on hand-written column states, and the column steps' bucket function equals graph_bucket on short tables."""
import ctypes as C
import os
import re

import numpy as np
import pytest


def test_symbols_and_signatures(pkg):
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "biogpt_hip.h")).read()
    for name, res, n_args in (("biogpt_hip_long_cols_launches", C.c_int64, 1), ("biogpt_hip_long_runs_plan", C.c_int, 3), ("biogpt_hip_column_bucket", C.c_int, 3),
                              ("biogpt_hip_attn_long_cols_device", C.c_int, 23)):
        f = getattr(pkg.lib(), name)
        assert f.restype is res and len(f.argtypes) == n_args, name
        decl = re.search(r"%s(\(([^;]*)\));" % name, header)
        assert decl and decl.group(2).count(",") + 1 == n_args, name      # the declaration has the arguments the binding passes
    assert pkg.lib().biogpt_hip_long_cols_launches(None) == -1
    assert callable(pkg.attn_long_cols_device) and callable(pkg.BiogptModel.long_cols_launches)


def state(slot, t_vis, ns=0, shr=0):
    return [t_vis + 5, 0, 0, slot, t_vis, ns, shr, 0]


@pytest.mark.parametrize("states,runs", [
    ([state(3, 1000 + i) for i in range(35)], [(0, 16), (16, 16), (32, 3)]),                                                  # a cut at 16 columns
    ([state(0, 9)] * 5 + [state(1, 9)] * 2 + [state(1, 9, 4, 7)] * 3 + [state(1, 9, 5, 7)] + [state(1, 9, 5, 6)], [(0, 5), (5, 2), (7, 3), (10, 1), (11, 1)]),  # slot, shared rows, their slot
    ([state(i, 1200) for i in range(4)], [(i, 1) for i in range(4)]),                                                        # single columns: a decode step's
])
def test_run_plan(pkg, states, runs):
    assert [tuple(r) for r in pkg.long_runs_plan(states)] == runs


@pytest.mark.parametrize("P", (64, 1024))
def test_column_buckets_of_short_tables_are_graph_buckets(pkg, P):
    assert all(pkg.column_bucket(P, T) == pkg.column_bucket(P, T, own=True) for T in range(1, P + 1))


def test_column_buckets_of_a_long_table(pkg):
    got = [pkg.column_bucket(2048, T) for T in (1, 64, 65, 256, 257, 512, 513, 1024, 1025, 2048)]
    assert got == [0, 0, 1, 3, 4, 4, 5, 5, 6, 6] and pkg.column_bucket(2048, 1025, own=True) == 5
