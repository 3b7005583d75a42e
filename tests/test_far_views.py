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


# ------------------------------------------------------------------------------------------- the serving pool's cases
# The placements of the serving-pool cases of tests/test_gpu_far_offsets.py (its constants are read from the module), and
# the proof that those cases can fail: no mutant of a kernel runs on the GPU - a kernel that truncates an address reads or
# writes outside its allocation - so for every row a far case reads or stores, the address under each of three errors is
# computed here and must, for at least one row of every operand, differ from the true one and lie outside the arena or on
# sentinel words that no operand of the case covers.  Such a kernel then fails far == near or the arena check.
import test_gpu_far_offsets as G  # noqa: E402

FP8 = torch.float8_e4m3fn
DT[1] = FP8
ARENA_BYTES = G.ARENA_I16 * 2
ERRORS = ("elem_i32", "byte_u32", "byte_i32")
NEW_PLACEMENTS = [
    ("far_slot-fp8", F.far_slot, _pool_shapes(9, 2, 4, 64, 128), 1),
    ("far_slot-fp8-d80", F.far_slot, _pool_shapes(9, 2, 4, 64, 80), 1),
    ("far_slot2-2B", F.far_slot2, _pool_shapes(35, 1, 4, 64, 128), 2),
    ("far_slot2-fp32", F.far_slot2, _pool_shapes(35, 2, 4, 64, 128), 4),
    ("far_head_skew-pack", F.far_head_skew, [(1, 2, 4 + 64 + 7 + 53, 128)] * 4, 2),
    ("far_head_skew-pack-fp32", F.far_head_skew, [(1, 2, 4 + 64 + 7 + 53, 64)] * 4, 4),
    ("far_slot-pages", F.far_slot, [(9, 2, 32, 128)] * 2, 2),
]


@pytest.mark.parametrize("name,geom,shapes,itemsize", NEW_PLACEMENTS, ids=[c[0] for c in NEW_PLACEMENTS])
def test_serving_placements_lie_inside_the_gpu_arena_and_do_not_overlap(name, geom, shapes, itemsize):
    test_views_have_the_right_shape_lie_inside_the_arena_and_do_not_overlap(name, geom, shapes, itemsize)
    assert F.arena_numel(geom.place(shapes, itemsize)) * itemsize <= ARENA_BYTES


def test_far_slot_with_one_byte_elements_puts_slot_8_at_2_32_and_slots_4_to_7_in_the_band():
    for s in F.far_slot.place(_pool_shapes(9, 2, 4, 64, 96), 1):
        assert s.strides[0] == 1 << 29 and s.at(8, 0, 0) >= TWO32 and s.at(8, 0, 0) - s.offset == TWO32
        for c in (4, 5, 6, 7):
            assert TWO31 <= s.at(c, 0, 0) and s.at(c, s.shape[1] - 1, s.shape[2] - 1, s.shape[3] - 1) < TWO32
        assert s.at(3, s.shape[1] - 1, s.shape[2] - 1, s.shape[3] - 1) < TWO31
        assert all(st % 16 == 0 for st in s.strides[:3]) and s.offset % 16 == 0


def test_far_slot2_puts_two_slots_past_4_gib_and_far_head_skew_moves_head_1_past_the_rows_of_head_0():
    for itemsize in (2, 4):
        for s in F.far_slot2.place(_pool_shapes(35, 2, 4, 64, 128), itemsize):
            assert s.at(33, 0, 0) * itemsize >= TWO32 and s.at(32, 1, 63, 127) * itemsize < TWO32
            assert s.at(34, 1, 63, 127) * itemsize < ARENA_BYTES
        for s in F.far_head_skew.place([(1, 2, 128, 128)] * 4, itemsize):
            assert s.at(0, 1, 0) * itemsize >= TWO32 and s.at(0, 0, 127, 127) * itemsize < TWO31
            low = (s.at(0, 1, 0) * itemsize) % TWO32               # where a 32-bit byte offset puts head 1
            assert low >= (s.at(0, 0, 127, 127) - s.offset + 1) * itemsize


@pytest.mark.parametrize("D", [128, 80, 64])
def test_page_pool_picks_pages_on_both_sides_of_every_line(D):
    Hkv, P = 2, G.PG
    n = G.ARENA_I16
    pp = F.page_pool(n, Hkv * P * D, 2)
    k, v = pp.specs(Hkv, P, D)
    assert F.disjoint([F.Spec((len(pp.picks), Hkv, P, D), 0, k.strides), F.Spec((len(pp.picks), Hkv, P, D), pp.page_numel, v.strides)])
    assert v.last < n and (pp.n_pages + 1) * pp.stride > n - pp.stride           # the largest addressed byte is inside
    byte = lambda p: k.at(p, 0, 0) * 2
    assert byte(pp.p31 - 1) < TWO31 <= byte(pp.p31) and byte(pp.p32 - 1) < TWO32 <= byte(pp.p32)
    assert k.at(pp.e31 - 1, 0, 0) < TWO31 <= k.at(pp.e31, 0, 0)
    picks = pp.picks
    for line in (pp.p31, pp.e31, pp.p32):
        assert line - 1 in picks and line in picks
    assert 0 in picks and pp.n_pages - 1 in picks and picks == sorted(set(picks))
    if D == 128:
        assert (pp.p31, pp.p32, pp.n_pages) == (65536, 131072, 135168)
    tab = F.deal_pages(picks, 3, G.WP // P, pp.p31, pp.p32)
    flat = [e for r in tab for e in r]
    assert len(set(flat)) == 9 and all(e in picks for e in flat)
    for r in tab:
        assert r[0] >= pp.p32 and r[1] < pp.p31 and pp.p31 <= r[2] < pp.p32 and r != sorted(r)
    assert 0 in flat and pp.n_pages - 1 in flat and pp.p31 - 1 in flat and pp.p31 in flat and pp.p32 - 1 in flat and pp.p32 in flat


def _assert_exposed(operands, itemsize, what):
    ex = F.exposed(operands, itemsize, ARENA_BYTES // itemsize)
    for (name, err), n in ex.items():
        if err == "elem_i32" and itemsize == 4:
            assert n == 0          # fp32: the arena holds fewer than 2^31 elements, no element offset leaves an int
        else:
            assert n > 0, (what, name, err, "no row of this operand would show the error")
    assert {e for _, e in ex} == set(ERRORS) and {o for o, _ in ex} == set(operands)


def _pool_operands(geom, S, Hkv, W, D, itemsize, named):
    specs = geom.place(_pool_shapes(S, Hkv, 4, W, D), itemsize)
    return {n: F.slot_rows(s, named) for n, s in zip(("sink_k", "sink_v", "window_k", "window_v"), specs)}


def test_truncated_addresses_expose_the_far_slot_cases():
    es = {"bf16": 2, "fp16": 2, "fp32": 4}
    for dt, D, _g, Hkv in G.PACKED:
        _assert_exposed(_pool_operands(F.far_slot, G.SLOT_S, Hkv, G.WC, D, es[dt], G.SLOT_NAMED), es[dt], ("packed", dt, D))
    for dt, D, _g, Hkv in G.FORK:
        for named in ([1, 3, 8, 5, 2], [1, 3, 8, 5, 2, 7]):
            _assert_exposed(_pool_operands(F.far_slot, G.SLOT_S, Hkv, G.WC, D, es[dt], named), es[dt], ("fork", dt, D))
        _assert_exposed(_pool_operands(F.far_slot2, 35, Hkv, G.WC, D, es[dt], [33, 1, 34, 2]), es[dt], ("far to far", dt, D))
    for dt, D, _g, Hkv in G.FP8_CASES:
        _assert_exposed(_pool_operands(F.far_slot, G.SLOT_S, Hkv, G.WC, D, 1, G.FP8_NAMED), 1, ("fp8", dt, D))


@pytest.mark.parametrize("dt,D", [("bf16", 128), ("fp16", 80), ("fp32", 64)])
def test_truncated_addresses_expose_the_far_head_pack(dt, D):
    itemsize = 4 if dt == "fp32" else 2
    ops = {}
    for n, T in enumerate((3 + 40 + 2 + G.NS + G.WC + 7 + 8, 7 + 16 + 1 + 3 + 5)):       # the two packs of the script
        for name, s in zip(("q", "k", "v", "o"), F.far_head_skew.place([(1, 2, T, D)] * 4, itemsize)):
            rows = s.row_starts() + (n << 22)
            assert int(rows.max()) + D <= ARENA_BYTES // itemsize
            ops[f"{name}{n}"] = (rows, D)
    _assert_exposed(ops, itemsize, ("far-head pack", dt, D))


def test_truncated_addresses_expose_the_paged_cases():
    n = G.ARENA_I16
    for dt, D, _g, Hkv in G.PAGED:
        pp = F.page_pool(n, Hkv * G.PG * D, 2)
        specs = pp.specs(Hkv, G.PG, D)
        lo, mid, hi = ([p for p in pp.picks if a <= p < b] for a, b in ((0, pp.p31), (pp.p31, pp.p32), (pp.p32, pp.n_pages)))
        tables = {"serving": [e for r in F.deal_pages(pp.picks, 3, G.WP // G.PG, pp.p31, pp.p32) for e in r],
                  "fork": lo[:3] + mid[:3] + hi[:3], "unmapped": F.deal_pages(pp.picks, 3, 3, pp.p31, pp.p32)[0]}
        for what, pages in tables.items():
            _assert_exposed({nm: F.slot_rows(s, pages) for nm, s in zip(("page_k", "page_v"), specs)}, 2, ("paged", what, dt, D))
    specs = F.far_slot.place([(9, 2, G.PG, 128)] * 2, 2)
    _assert_exposed({nm: F.slot_rows(s, [8, 1, 3, 7, 5, 2]) for nm, s in zip(("page_k", "page_v"), specs)}, 2, "paged far_slot")


def test_exposed_reports_nothing_for_a_near_case_and_a_landing_on_another_operand():
    near = {"a": (torch.arange(4, dtype=torch.int64) * 64, 16)}
    assert set(F.exposed(near, 2, 1 << 20).values()) == {0}
    # a far_head operand: the byte truncations of head 1 land exactly on head 0 of the same operand - not exposed
    s = F.far_head.place([(1, 2, 8, 64)], 2)[0]
    ex = F.exposed({"q": (s.row_starts(), 64)}, 2, ARENA_BYTES // 2)
    assert ex[("q", "byte_u32")] == 0 and ex[("q", "byte_i32")] == 0 and ex[("q", "elem_i32")] == 8
    t = F.truncations(torch.tensor([TWO31, TWO31 + 5, 3 << 30]), 2)
    assert t["elem_i32"].tolist() == [-TWO32, -TWO32 + 10, (3 << 31) - (1 << 33)] and t["byte_u32"].tolist() == [0, 10, TWO31]
    assert t["byte_i32"].tolist() == [0, 10, -TWO31]


@pytest.mark.parametrize("dtype,sentinel", [(FP8, F.SENTINEL8), (torch.bfloat16, F.SENTINEL16), (torch.float32, F.SENTINEL16)])
def test_the_sentinel_parameter_and_one_byte_elements(dtype, sentinel):
    arena = torch.empty(4096, dtype=torch.uint8).view(dtype)
    F.fill_sentinel(arena, sentinel)
    assert F.is_sentinel(arena, sentinel) and bool(torch.isnan(arena.float()).all())
    if dtype == FP8:
        assert bool((arena.view(torch.uint8) == 0x7F).all())
        with pytest.raises(AssertionError):
            F.fill_sentinel(arena)                   # 0x7FC1: one NaN byte and a finite one
    v = F.far_view(arena, (1, 2, 3, 16), (0, 128, 32), 16)
    v.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[v.element_size()]).zero_()
    assert not F.is_sentinel(v, sentinel)
    assert torch.equal(F.sentinel_full((2, 3), dtype, "cpu", sentinel).view(torch.uint8), arena[:6].view(torch.uint8).reshape(2, -1))
    F.assert_untouched(arena, [v], "clean", sentinel=sentinel)
    arena.view(torch.uint8)[1000] = 3
    with pytest.raises(AssertionError, match="8-byte words outside"):
        F.assert_untouched(arena, [v], "stray", sentinel=sentinel)
    assert F.is_sentinel(arena, sentinel)
