"""CPU companion of tests/test_gpu_paged_fp8_far.py, in the manner of tests/test_far_views.py: the page pool of that case
at one byte per element has pages on both sides of 2^31 and of 2^32 bytes, the case's table holds some of each, and for
the K and the V page buffer at least one row the case touches would, under a signed or an unsigned 32-bit byte offset (or
a 32-bit element offset: the same number here), land outside the arena or on sentinel bytes that no operand owns - so a
kernel with that error cannot pass the GPU case."""
import far_views as F
import test_gpu_far_offsets as G
import test_gpu_paged_fp8_far as T

ARENA_BYTES = G.ARENA_I16 * 2
TWO31, TWO32 = F.TWO31, F.TWO32


def _pool():
    _dt, D, _g, Hkv = T.CASE
    return F.page_pool(ARENA_BYTES, Hkv * G.PG * D, 1), Hkv, D


def test_the_page_pool_at_one_byte_per_element_has_pages_on_both_sides_of_every_line():
    pp, Hkv, D = _pool()
    k, v = pp.specs(Hkv, G.PG, D)
    assert v.last < ARENA_BYTES and pp.p31 == pp.e31                 # bytes are elements
    byte = lambda p: k.at(p, 0, 0)
    assert byte(pp.p31 - 1) < TWO31 <= byte(pp.p31) and byte(pp.p32 - 1) < TWO32 <= byte(pp.p32) < ARENA_BYTES
    assert (pp.p31, pp.p32, pp.n_pages) == (TWO31 // pp.stride, TWO32 // pp.stride, ARENA_BYTES // pp.stride)
    tab = F.deal_pages(pp.picks, 3, G.WP // G.PG, pp.p31, pp.p32)
    flat = [e for r in tab for e in r]
    assert len(set(flat)) == 9 and 0 in flat and pp.n_pages - 1 in flat
    for r in tab:
        assert r[0] >= pp.p32 and r[1] < pp.p31 and pp.p31 <= r[2] < pp.p32 and r != sorted(r)


def test_a_32_bit_byte_offset_would_leave_the_operands_of_the_case():
    pp, Hkv, D = _pool()
    specs = pp.specs(Hkv, G.PG, D)
    pages = [e for r in F.deal_pages(pp.picks, 3, G.WP // G.PG, pp.p31, pp.p32) for e in r]
    ops = {nm: F.slot_rows(s, pages) for nm, s in zip(("page_k", "page_v"), specs)}
    ex = F.exposed(ops, 1, ARENA_BYTES)
    assert {e for _, e in ex} == {"elem_i32", "byte_u32", "byte_i32"} and {o for o, _ in ex} == set(ops)
    for (name, err), n in ex.items():
        assert n > 0, (name, err, "no row of this operand would show the error")
    # an offset that keeps 64 bits moves nothing: the same rows against themselves
    rows, n = ops["page_k"]
    assert bool((rows >= 0).all()) and int(rows.max()) + n <= ARENA_BYTES
