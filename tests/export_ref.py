"""The export of pool slots (sfa_ring_export_slots, include/sfa.h), restated in torch on CPU copies of a pool.

Written from what a state row {sink_len, window_len, write_pos, seen} MEANS, not from the kernel: a slot holds its first
sink_len tokens in the sink rows; the ring holds the window_len NEWEST tokens, the newest one in the slot just behind
write_pos (a commit stores at write_pos and moves it on), the one before it one slot further back, wrapping at slot 0.
The newest token has position seen - 1.  So the twin walks the ring BACKWARDS from write_pos - 1 and reverses the walk;
the brute-force model of tests/test_export_host.py checks that reading against a simulated cache.

A paged ring is first gathered into its contiguous twin (tests/paged_ref.py: unmapped pages read as zeros, which is what
the export writes for them); FP8 buffers are first read by the reading rule (tests/fp8_ref.py)."""
import torch

import fp8_ref
import paged_ref


def clamp_cu(cu, T):
    """the offsets as every packed call clamps them: into [0, T], each end at least its start"""
    out = []
    for a, b in zip(cu[:-1], cu[1:]):
        c0 = min(max(int(a), 0), T)
        out.append((c0, max(c0, min(max(int(b), 0), T))))
    return out


def token_order(state_row, num_sink, Wc):
    """[(is_sink, row or ring slot, position)] of the live tokens of one state row, oldest first"""
    sl = min(max(int(state_row[0]), 0), num_sink)
    wl = min(max(int(state_row[1]), 0), Wc)
    wp = min(max(int(state_row[2]), 0), Wc - 1)
    seen = int(state_row[3])
    toks = [(True, j, j) for j in range(sl)]
    back, slot, pos = [], wp, seen
    for _ in range(wl):                      # the newest token first: one slot back and one position down at a time
        slot = slot - 1 if slot > 0 else Wc - 1
        pos -= 1
        back.append((False, slot, pos))
    return toks + back[::-1]


def export_twin(sink_k, sink_v, ring_k, ring_v, state, slots, cu, T, num_sink, Wc, table=None, kv_scale=None, dtype=None):
    """The expected (k, v, pos) of an export: k / v [1, H_kv, T, D] in `dtype` (default: the buffers' own), pos int32 [T].
    sink_* [S, H_kv, num_sink, D]; ring_* [S, H_kv, Wc, D], or the pages [n_pages, H_kv, P, D] with `table` [S, Wc / P];
    FP8 buffers are read with kv_scale ([2, H_kv] or None = ones) into `dtype`.  All tensors on the CPU."""
    if table is not None:                    # FP8 pages are gathered as bytes (a zero byte is the code of +0)
        as_bytes = ring_k.dtype == fp8_ref.FP8
        ring_k, ring_v = (paged_ref.gather(r.view(torch.uint8) if as_bytes else r, table) for r in (ring_k, ring_v))
        if as_bytes:
            ring_k, ring_v = ring_k.view(fp8_ref.FP8), ring_v.view(fp8_ref.FP8)
    if sink_k.dtype == fp8_ref.FP8:
        ks, vs = (None, None) if kv_scale is None else (kv_scale[0], kv_scale[1])
        sink_k, ring_k = fp8_ref.dequant(sink_k, ks, dtype), fp8_ref.dequant(ring_k, ks, dtype)
        sink_v, ring_v = fp8_ref.dequant(sink_v, vs, dtype), fp8_ref.dequant(ring_v, vs, dtype)
    S, H, _, D = sink_k.shape
    k = torch.zeros(1, H, T, D, dtype=sink_k.dtype)
    v = torch.zeros_like(k)
    pos = torch.full((T,), -1, dtype=torch.int32)
    for (c0, c1), c in zip(clamp_cu(cu, T), [int(x) for x in slots]):
        if not 0 <= c < S:
            continue
        for j, (is_sink, row, p) in enumerate(token_order(state[c].tolist(), num_sink, Wc)[:c1 - c0]):
            k[0, :, c0 + j] = (sink_k if is_sink else ring_k)[c, :, row]
            v[0, :, c0 + j] = (sink_v if is_sink else ring_v)[c, :, row]
            pos[c0 + j] = p
    return k, v, pos


def same_bits(a, b):
    """bitwise equality (NaN patterns and the sign of zero included)"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    view = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[a.element_size()]
    return torch.equal(a.contiguous().view(view), b.contiguous().view(view))
