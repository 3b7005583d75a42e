"""The far-offset twin of the export (sfa_ring_export_slots): the pool's last slot lies past 4 GiB (far_slot) and the
output pack sits behind a head stride of 4 GiB and more (far_head_skew), both in one arena of tests/far_views.py.  The
same calls on ordinary tensors are the reference: far == near bitwise, near == the torch twin, and every word of the arena
outside the operands still holds the sentinel."""
import pytest
import torch

import export_ref as X
import far_views as F
from util import rand

pytestmark = pytest.mark.gpu
DEV = "cuda"
ARENA_I16 = (1 << 31) + (1 << 26)          # int16 elements: 4 GiB + 128 MiB, as tests/test_gpu_far_offsets.py
S, HKV, NS, WC, D = 9, 2, 4, 48, 128
NAMED = [8, 3, 1]                          # the prefilled slots; 8 is the far one and is wrapped by a commit
PACK_OFF = 1 << 22                         # the pack starts 4 Mi elements into the arena: clear of every pool slot


def _layer(bufs):
    from sink_attention import SinkCacheLayer
    L = SinkCacheLayer(NS, WC)
    L.sink_k, L.sink_v, L.window_k, L.window_v = bufs
    L._dev_state = torch.zeros(S, 4, dtype=torch.int32, device=DEV)
    L.is_initialized = L.prefilled = L._per_seq = L._pool = True
    return L


def _fill(L, g_seed):
    g = torch.Generator().manual_seed(g_seed)
    lens = [NS + WC + 20, 9, 2]
    T = sum(lens)
    k, v = rand((1, HKV, T, D), g, torch.bfloat16).to(DEV), rand((1, HKV, T, D), g, torch.bfloat16).to(DEV)
    L.prefill_slots(k, v, [0, lens[0], lens[0] + lens[1], T], NAMED)
    kc, vc = rand((1, HKV, 5, D), g, torch.bfloat16).to(DEV), rand((1, HKV, 5, D), g, torch.bfloat16).to(DEV)
    L.commit_packed_dyn(kc, vc, [0, 5], [8], [5])
    assert L._dev_state[8].tolist() == [NS, WC, 5, NS + WC + 25]


def test_export_of_a_slot_past_4_gib_into_a_pack_behind_a_4_gib_head_stride():
    need = ARENA_I16 * 2
    free, total = torch.cuda.mem_get_info()
    if free < need + (2 << 30):
        pytest.skip(f"far-offset arena needs {need / 2**30:.2f} + 2 GiB free, the device reports {free / 2**30:.2f} "
                    f"of {total / 2**30:.2f} GiB")
    dt = torch.bfloat16
    slots, cu = [8, 3, -1, 1, 8], [0, 52, 63, 66, 68, 80]       # the far slot in full and cut short; a zero tail; padding
    T = cu[-1] + 4
    shapes = [(S, HKV, NS, D), (S, HKV, NS, D), (S, HKV, WC, D), (S, HKV, WC, D)]
    # near
    Ln = _layer([torch.zeros(s, dtype=dt, device=DEV) for s in shapes])
    _fill(Ln, 4242)
    near = [torch.full((1, HKV, T, D), float("nan"), dtype=dt, device=DEV) for _ in range(2)] + \
           [torch.full((T,), -7, dtype=torch.int32, device=DEV)]
    Ln.export_slots(slots, cu=cu, out=tuple(near))
    want = X.export_twin(*(t.cpu() for t in (Ln.sink_k, Ln.sink_v, Ln.window_k, Ln.window_v)), Ln._dev_state.cpu(), slots, cu,
                         T, NS, WC)
    assert all(X.same_bits(a.cpu(), b) for a, b in zip(near, want))
    # far
    arena = torch.empty(ARENA_I16, dtype=torch.int16, device=DEV).view(dt)
    try:
        F.fill_sentinel(arena)
        farb = F.views(arena, F.far_slot, shapes)
        for t in farb:
            t.view(torch.int16)[NAMED] = 0
            assert t[8].data_ptr() - arena.data_ptr() >= F.TWO32 and t[3, -1, -1].data_ptr() - arena.data_ptr() < F.TWO31
        pack = F.views(arena[PACK_OFF:], F.far_head_skew, [(1, HKV, T, D)] * 2)
        for t in pack:
            assert t.stride(1) * 2 >= F.TWO32 and t[0, 1].data_ptr() - arena.data_ptr() >= F.TWO32
            assert F.is_sentinel(t)                                     # clear of the pool's slots: nothing was zeroed here
        Lf = _layer(farb)
        _fill(Lf, 4242)
        for a, b in zip(farb, (Ln.sink_k, Ln.sink_v, Ln.window_k, Ln.window_v)):
            assert X.same_bits(a[NAMED], b[NAMED])
        pos = torch.full((T,), -7, dtype=torch.int32, device=DEV)
        before = [t[NAMED].clone() for t in farb]
        Lf.export_slots(slots, cu=cu, out=(pack[0], pack[1], pos))
        assert X.same_bits(pack[0], near[0]) and X.same_bits(pack[1], near[1]) and torch.equal(pos, near[2])
        assert torch.equal(Lf._dev_state, Ln._dev_state)
        for t, b in zip(farb, before):                                  # read only: the named slots keep their bytes,
            assert X.same_bits(t[NAMED], b)
            rest = [c for c in range(S) if c not in NAMED]
            assert F.is_sentinel(t.view(torch.int16)[rest])             # the others the sentinel
        F.assert_untouched(arena, list(farb) + list(pack), "export far")
    finally:
        del arena
        torch.cuda.empty_cache()
