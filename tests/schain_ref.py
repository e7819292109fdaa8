"""The SIMD chain's attention over column states, restated on tests/assoc_ref.py: a column's visible rows gathered from its slots, then assoc_ref.attn_head on
them -- where a key's row lies changes what is gathered, never the order of the sums.  tests/test_schain_capi.py holds this file to assoc_ref.py and the oracle
where the gathering is the identity; tests/test_gpu_schain_kernels.py holds attn_simd_cols_kernel (csrc/kernels_schain.hip.h) to it bit for bit."""
import numpy as np

import assoc_ref as A

F32 = np.float32


def column_view(st, i, col_mode, shared):
    """(own slot, visible keys, shared rows, shared slot) of column i from its eight state words {n_past, token, n_gen, seq_id, t_vis, pad[0], pad[1], pad[2]}."""
    n_past, _, _, seq_id, t_vis, n_shared, shr_slot, _ = (int(v) for v in st[i])
    return (seq_id if col_mode else i), (t_vis if col_mode else n_past + 1), (n_shared if shared else 0), shr_slot


def gather_rows(slots, h, own, T, n_shared, shr_slot):
    """Rows 0 .. T - 1 of head h as column sees them: the first n_shared from the shared slot, the rest from its own.  slots [n_slots, H, P, 64]."""
    rows = np.array(slots[own, h, :T], dtype=F32, copy=True)
    n = min(n_shared, T)
    if n > 0:
        rows[:n] = slots[shr_slot, h, :n]
    return rows


def attn_columns(q, k_slots, v_slots, st, col_mode, shared):
    """float32 [N, H * 64]: every (column, head) through assoc_ref.attn_head on its gathered rows.  q [N, H * 64], k_slots / v_slots [n_slots, H, P, 64]."""
    q = np.asarray(q, dtype=F32)
    N, H = q.shape[0], k_slots.shape[1]
    out = np.zeros((N, H * 64), F32)
    for i in range(N):
        own, T, n_shared, shr_slot = column_view(st, i, col_mode, shared)
        for h in range(H):
            K, V = gather_rows(k_slots, h, own, T, n_shared, shr_slot), gather_rows(v_slots, h, own, T, n_shared, shr_slot)
            out[i, h * 64:(h + 1) * 64] = A.attn_head(q[i, h * 64:(h + 1) * 64], K, V, T)
    return out
