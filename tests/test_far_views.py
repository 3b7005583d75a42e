"""CPU: the far-offset placements of tests/far_views.py are what they claim (index arithmetic on ``meta`` arenas, so
nothing is allocated): right shapes, inside the arena, pairwise disjoint, and really across the thresholds."""
import pytest
import torch

import far_views as F
from far_views import TWO31, TWO32


def _dense_shapes(B, Hq, Hkv, Nq, Nk, D):
    q, k = (B, Hq, Nq, D), (B, Hkv, Nk, D)
    return [q, k, k, q, q, q, k, k]              # q k v o dO dq dk dv


def _pool_shapes(S, Hkv, ns, W, D):
    return [(S, Hkv, ns, D)] * 2 + [(S, Hkv, W, D)] * 2


CASES = [
    ("far_batch-2B", F.far_batch, _dense_shapes(2, 4, 2, 512, 512, 128), 2),
    ("far_batch-2B-d256-NqNk", F.far_batch, _dense_shapes(2, 4, 2, 256, 768, 256), 2),
    ("far_batch-fp32", F.far_batch, _dense_shapes(2, 4, 2, 512, 512, 48), 4),
    ("far_batch-rows-cache", F.far_batch, _pool_shapes(2, 2, 4, 64, 128), 2),
    ("far_head-2B", F.far_head, _dense_shapes(2, 2, 1, 512, 512, 128), 2),
    ("band_head-2B", F.band_head, _dense_shapes(2, 2, 1, 640, 640, 128), 2),
    ("far_head-packed", F.far_head, _dense_shapes(1, 2, 1, 517, 517, 80), 2),
    ("wide_rows-fwd", F.wide_rows(2048, F.FWD_MARGIN), _dense_shapes(2, 2, 1, 2048, 2048, 128)[:4], 2),
    ("wide_rows-bwd", F.wide_rows(4096, F.BWD_MARGIN), _dense_shapes(2, 2, 1, 4096, 4096, 128), 2),
    ("over_rows-fwd", F.over_rows(2048, F.FWD_MARGIN), _dense_shapes(2, 2, 1, 2048, 2048, 128)[:4], 2),
    ("over_rows-bwd", F.over_rows(4096, F.BWD_MARGIN), _dense_shapes(2, 2, 1, 4096, 4096, 128), 2),
    ("wide_rows-packed", F.wide_rows(517, F.FWD_MARGIN), _dense_shapes(1, 2, 1, 517, 517, 128)[:4], 2),
    ("far_slot-2B", F.far_slot, _pool_shapes(9, 1, 4, 64, 64), 2),
    ("far_slot-fp32", F.far_slot, _pool_shapes(9, 2, 4, 64, 48), 4),
]
DT = {2: torch.bfloat16, 4: torch.float32}


@pytest.mark.parametrize("name,geom,shapes,itemsize", CASES, ids=[c[0] for c in CASES])
def test_views_have_the_right_shape_lie_inside_the_arena_and_do_not_overlap(name, geom, shapes, itemsize):
    specs = geom.place(shapes, itemsize)
    n = F.arena_numel(specs)
    assert n * itemsize <= F.ARENA_LIMIT_BYTES, f"{name}: arena of {n * itemsize / 2**30:.2f} GiB"
    assert n % 8 == 0
    arena = torch.empty(n, dtype=DT[itemsize], device="meta")
    vs = F.views(arena, geom, shapes)
    for v, s, shape in zip(vs, specs, shapes):
        assert tuple(v.shape) == shape and v.stride() == s.strides and v.storage_offset() == s.offset
        assert v.stride(3) == 1 and 0 <= s.offset and s.last < n
        assert all((st * itemsize) % 16 == 0 for st in s.strides[:3]) and (s.offset * itemsize) % 16 == 0
    assert F.disjoint(specs)
    with pytest.raises(AssertionError):              # one element short: the last view no longer fits
        F.views(torch.empty(n - 8, dtype=DT[itemsize], device="meta"), geom, shapes)


def test_disjoint_sees_an_overlap():
    a = F.Spec((1, 1, 4, 8), 0, (64, 64, 16, 1))
    assert F.disjoint([a, F.Spec((1, 1, 4, 8), 8, (64, 64, 16, 1))])
    assert not F.disjoint([a, F.Spec((1, 1, 4, 8), 7, (64, 64, 16, 1))])
    assert not F.disjoint([a, F.Spec((1, 1, 2, 8), 16, (64, 64, 16, 1))])


@pytest.mark.parametrize("itemsize", [2, 4])
def test_far_batch_crosses_4_gib_at_batch_1_and_keeps_batch_0_near(itemsize):
    for s in F.far_batch.place(_dense_shapes(2, 4, 2, 512, 768, 128), itemsize):
        assert s.at(1, 0, 0) * itemsize >= TWO32
        assert s.at(0, s.shape[1] - 1, s.shape[2] - 1, s.shape[3] - 1) * itemsize < TWO31
        assert s.strides[0] >= TWO31 if itemsize == 2 else s.strides[0] == 1 << 30
        assert s.strides[0] > 0x7FFFFFFF or itemsize == 4          # no int32 holds the 2-byte batch stride


def test_far_head_crosses_4_gib_at_head_1_and_keeps_rows_and_batches_near():
    for s in F.far_head.place(_dense_shapes(2, 2, 1, 1024, 1024, 128), 2):
        B, H, N, D = s.shape
        assert s.strides[1] * 2 >= TWO32 and not F.head_stride_ok(s.strides[1])
        assert F.head_stride_ok(s.strides[1] - 8)
        assert s.at(B - 1, 0, N - 1, D - 1) * 2 < TWO31
        assert F.row_reach_ok(N, s.strides[2], F.BWD_MARGIN)       # only the head stride is out of range
        if H > 1:
            assert s.at(0, 1, 0) >= TWO31


def test_band_head_is_the_largest_accepted_head_stride_and_lies_in_the_signed_band():
    for s in F.band_head.place(_dense_shapes(2, 2, 1, 640, 640, 128), 2):
        B, H, N, D = s.shape
        sh = s.strides[1]
        assert F.head_stride_ok(sh) and not F.head_stride_ok(sh + 8) and TWO31 <= sh * 2 < TWO32
        assert s.at(B - 1, 0, N - 1, D - 1) * 2 < TWO31 and F.row_reach_ok(N, s.strides[2], F.BWD_MARGIN)
    with pytest.raises(AssertionError):
        F.band_head.place(_dense_shapes(2, 2, 1, 64, 64, 48), 4)


@pytest.mark.parametrize("N,margin,sn,ratio", [(4096, 1280, 399448, 1.52), (2048, 320, 906856, 1.73)])
def test_wide_and_over_rows_straddle_the_rule_by_one_step(N, margin, sn, ratio):
    w, o = F.wide_rows(N, margin), F.over_rows(N, margin)
    assert w.sn == sn and o.sn == sn + 8 and sn % 8 == 0
    assert F.row_reach_ok(N, w.sn, margin) and not F.row_reach_ok(N, o.sn, margin)
    last = (N - 1) * w.sn * 2                                       # the signed / unsigned band
    assert TWO31 <= last < TWO32 and abs(last / TWO31 - ratio) < 0.005
    for s in w.place(_dense_shapes(2, 2, 1, N, N, 128), 2):
        assert s.strides[2] == sn and s.strides[1] * 2 < 65536 and s.strides[0] * 2 < 65536
        assert TWO31 <= s.at(0, 0, N - 1) * 2 < TWO32


def test_wide_rows_for_a_pack():
    w = F.wide_rows(517, F.FWD_MARGIN)
    assert F.row_reach_ok(517, w.sn, F.FWD_MARGIN) and not F.row_reach_ok(517, w.sn + 8, F.FWD_MARGIN)
    assert TWO31 <= 516 * w.sn * 2 < TWO32


@pytest.mark.parametrize("itemsize", [2, 4])
def test_far_slot_last_slot_far_first_slots_near(itemsize):
    S = 9
    for s in F.far_slot.place(_pool_shapes(S, 2, 4, 64, 64), itemsize):
        assert s.at(S - 1, 0, 0) * itemsize >= TWO32 and s.strides[0] * (S - 1) * itemsize >= TWO32
        if itemsize == 2:
            assert s.strides[0] * (S - 1) >= TWO31
        assert s.at(1, s.shape[1] - 1, s.shape[2] - 1, s.shape[3] - 1) * itemsize < TWO31
        assert s.at(S - 2, 0, 0) * itemsize < TWO32                # exactly one slot lies past 4 GiB


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_far_view_holds_the_values_and_assert_untouched_sees_a_stray_store(dtype):
    g = torch.Generator().manual_seed(5)
    t = torch.randn(2, 2, 5, 16, generator=g).to(dtype)
    arena = torch.empty(4096, dtype=dtype)
    F.fill_sentinel(arena)
    assert F.is_sentinel(arena)
    v = F.far_view(arena, t, (2048, 512, 40), 24)
    assert torch.equal(v, t) and v.data_ptr() == arena.data_ptr() + 24 * arena.element_size()
    assert not F.is_sentinel(v)
    out = F.far_view(arena, (2, 2, 5, 16), (2048, 512, 40), 1024)
    assert F.is_sentinel(out) and bool(torch.isnan(out.float()).all())
    F.assert_untouched(arena, [v, out], "clean", inputs=[(v, t)])
    v.copy_(t)
    v[1, 1, 4, 15] += 1                                              # a store inside an input operand's view
    with pytest.raises(AssertionError, match="input operand 0"):
        F.assert_untouched(arena, [v, out], "inside", inputs=[(v, t)])
    F.fill_sentinel(arena)
    arena[3000] = 1.0                                                # a store outside every view
    with pytest.raises(AssertionError, match="element 3000"):
        F.assert_untouched(arena, [v, out], "stray")
    assert F.is_sentinel(arena)                                      # left ready for the next case
