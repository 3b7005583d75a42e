"""Far-offset views: small [B, H, N, D] operands placed at large strides inside one arena.

A kernel's address arithmetic goes wrong where an operand LIES, not in what it holds: a 32-bit product of a row or head
index and a stride, a batch or slot offset kept in an int, a byte offset past 2^31 read as negative.  None of that
needs a large problem - it needs a small tensor whose strides push its far rows past 2^31 elements, 2^31 bytes or
2^32 bytes.  This module computes such placements (pure index arithmetic, so the CPU tests run them on ``meta``
arenas) and builds the ``as_strided`` views.

Several operands share one arena: every geometry interleaves them in the columns of the same rows (operand i at
column offset c_i of a row of ``sn`` elements), so a whole forward + backward lives in one allocation.

Geometries (each states the offsets it produces; ``tests/test_far_views.py`` checks the statements):

* ``far_batch``   ``sb * itemsize >= 2^32``: batch 1 starts at or past 2^32 bytes, which for the 2-byte types is at or
  past element 2^31.  fp32 gets its own arithmetic: ``sb = 2^30`` elements (2^31 fp32 elements would be 8 GiB).  Batch
  0 - rows and heads - stays below 2^31 bytes.
* ``far_head``    ``sh * itemsize >= 2^32`` with rows and batches near (all of head 0 below 2^31 bytes).  A second
  head costs 4 GiB, so this geometry takes operands of at most two heads.
* ``band_head``   the largest head stride the MFMA paths accept: ``sh * 2 = 2^32 - 16`` bytes, inside [2^31, 2^32), the
  band where a 32-bit head stride read as signed would be negative.  2-byte types only; otherwise as ``far_head``.
* ``wide_rows(N, margin)``  the largest row stride ``sn`` (a multiple of 8) that passes the library's row-reach rule
  for ``N`` rows; every (batch, head) slice is a column block of the same rows.  ``over_rows`` is the next multiple of
  8, the smallest that fails.  The rule, restated from ``slice_ok()`` of csrc/sfa_fwd_mfma.hip (margin 320) and
  csrc/sfa_bwd_mfma.hip (margin 1280): ``(N + margin) * sn * 2 + 512 < 2^32 - 65536``.
  N = 4096, margin 1280: sn = 399448, last row at 1.52 x 2^31 bytes; N = 2048, margin 320: sn = 906856, 1.73 x 2^31.
* ``far_slot``    a pool ``[S, H, W, D]`` whose ``stride[0]`` times the last slot index reaches 2^32 bytes (2^31
  elements for the 2-byte types; fp32 as for ``far_batch``), the first slots near.  With one-byte elements (the FP8
  pool, item size 1) and 9 slots the stride is 2^29: slot 8 starts at byte and element 2^32, slots 4 to 7 lie in
  [2^31, 2^32) - the band where a signed 32-bit offset is negative - and column blocks are multiples of 16 elements.
  ``far_slot2`` puts the last TWO slots past 2^32 bytes (35 slots fit the arena): a copy from far to far.
* ``far_head_skew``  ``far_head`` with head 1 a further head-0's-worth of rows on: ``sh * itemsize`` is 2^32 plus the
  bytes of head 0, so that a byte offset cut to 32 bits puts head 1 on sentinel words behind head 0, not on head 0.

The page picker (``page_pool``, ``PagePool``) lays a paged ring out as a production server does, as ONE buffer: page p of
K is ``page_numel`` elements at element ``p * stride``, page p of V the ``page_numel`` after them, ``stride = 2 *
page_numel``; ``n_pages = arena elements // stride``.  It states ``p31`` / ``e31`` / ``p32``, the first page at or past
2^31 bytes / 2^31 elements / 2^32 bytes (H_kv 2, P 32, D 128, 2-byte types in the 4.1 GiB arena: stride 16384 elements,
p31 = 65536, e31 = p32 = 131072, n_pages = 135168), and ``picks``: the page on each side of every line, the first and
the last page and one neighbour each.  ``deal_pages`` deals them into table rows that are not monotone and hold one
page past 2^32 bytes, one below 2^31 bytes and one of the band.  A page under a line may straddle it.

Sentinels: ``fill_sentinel`` / ``is_sentinel`` / ``assert_untouched`` take the 16-bit pattern the arena is filled with.
The default ``SENTINEL16`` is a NaN as bf16, fp16 and fp32, but as two e4m3fn bytes it is one NaN (0x7F) and one finite
code (0xC1); one-byte cases pass ``SENTINEL8`` (0x7F in every byte).

``truncations`` / ``exposed`` stand in for device mutants: for the rows of a far case they form the address a kernel
would form with the element offset in a signed 32-bit int, or the byte offset in an unsigned or a signed one, and count
the rows whose wrong address leaves the arena or falls on sentinel words outside the case's operands.
"""
from dataclasses import dataclass
from typing import List, Sequence, Tuple

import torch

TWO31 = 1 << 31
TWO32 = 1 << 32
ARENA_LIMIT_BYTES = int(4.5 * (1 << 30))
FWD_MARGIN = 320          # slice_ok() of csrc/sfa_fwd_mfma.hip
BWD_MARGIN = 1280         # slice_ok() of csrc/sfa_bwd_mfma.hip
SENTINEL16 = 0x7FC1       # as bf16, fp16 and (twice) fp32 a NaN: a load from a wrong address poisons the result
SENTINEL64 = int.from_bytes(SENTINEL16.to_bytes(2, "little") * 4, "little")
SENTINEL8 = 0x7F7F        # one-byte elements (e4m3fn): NaN in every byte; SENTINEL16 there is one NaN (0x7F) and a finite 0xC1


def row_reach_ok(N: int, sn: int, margin: int) -> bool:
    """The row-reach rule of the MFMA paths for a slice of N rows at row stride sn (elements, 2-byte types)."""
    return (N + margin) * sn * 2 + 512 < TWO32 - 65536


def head_stride_ok(sh: int) -> bool:
    """The head-stride rule of the MFMA paths (2-byte types): the hand-placed kernels carry it as 32-bit bytes."""
    return 0 <= sh * 2 < TWO32


def _up(x: int, m: int) -> int:
    return -(-x // m) * m


@dataclass(frozen=True)
class Spec:
    """Where one operand lies: storage offset and element strides of a [B, H, N, D] view."""
    shape: Tuple[int, int, int, int]
    offset: int
    strides: Tuple[int, int, int, int]

    def at(self, b: int, h: int, n: int, d: int = 0) -> int:
        return self.offset + b * self.strides[0] + h * self.strides[1] + n * self.strides[2] + d

    @property
    def last(self) -> int:
        """Largest element offset the view holds."""
        B, H, N, D = self.shape
        return self.at(B - 1, H - 1, N - 1, D - 1)

    def row_starts(self) -> torch.Tensor:
        """Element offset of every row (b, h, n), int64 [B * H * N]."""
        B, H, N, _ = self.shape
        ar = lambda n, s: torch.arange(n, dtype=torch.int64) * s
        return (self.offset + ar(B, self.strides[0])[:, None, None] + ar(H, self.strides[1])[None, :, None] +
                ar(N, self.strides[2])[None, None, :]).reshape(-1)


@dataclass(frozen=True)
class Geometry:
    name: str
    kind: str                 # "batch" | "head" | "band" | "rows" | "slot"
    sn: int = 0               # rows: the row stride
    N: int = 0                # rows: the row count the stride was sized for
    margin: int = 0
    n_far: int = 1            # slot: how many of the last slots lie at or past 2^32 bytes
    skew: bool = False        # head: head 1 lies a further head-0's-worth of rows on (far_head_skew)

    def place(self, shapes: Sequence[Tuple[int, int, int, int]], itemsize: int) -> List[Spec]:
        """Non-overlapping placements for operands of the given shapes, all in one arena."""
        shapes = [tuple(int(x) for x in s) for s in shapes]
        cols = [_up(s[3], 16 if itemsize == 1 else 8) for s in shapes]      # 16-byte aligned column blocks
        Bm, Hm, Nm = (max(s[i] for s in shapes) for i in range(3))
        if self.kind == "rows":
            sn, specs, c = self.sn, [], 0
            for s, col in zip(shapes, cols):                  # slice (b, h) of an operand: its own column block
                specs.append(Spec(s, c, (s[1] * col, col, sn, 1)))
                c += s[0] * s[1] * col
            assert c <= sn, f"{self.name}: {c} columns do not fit a row of {sn} elements"
            return specs
        sn = sum(cols)
        far = TWO32 // itemsize
        if self.kind in ("head", "band"):
            assert Hm <= 2, "far_head: a third head would lie past 8 GiB"
            assert self.kind == "head" or itemsize == 2, "band_head: the rule it sits under is that of the 2-byte MFMA paths"
            sb, sh = Nm * sn, far if self.kind == "head" else far - 8
            if self.skew:
                sh += _up(Bm * sb, 16)
            assert Bm * sb * itemsize < TWO31, "far_head: batches and rows must stay near"
        elif self.kind == "batch":
            sh = Nm * sn
            assert Hm * sh * itemsize < TWO31, "far_batch: heads and rows must stay near"
            sb = far
        else:                                                 # slot: the last slot far, S - 1 equal steps
            sh = Nm * sn
            assert Bm > self.n_far >= 1
            sb = _up(-(-far // (Bm - self.n_far)), 16 if itemsize == 1 else 8)
            assert Hm * sh <= sb, "far_slot: a slot does not fit the slot stride"
        specs, c = [], 0
        for s, col in zip(shapes, cols):
            specs.append(Spec(s, c, (sb, sh, sn, 1)))
            c += col
        return specs


far_batch = Geometry("far_batch", "batch")
far_head = Geometry("far_head", "head")
band_head = Geometry("band_head", "band")
far_head_skew = Geometry("far_head_skew", "head", skew=True)
far_slot = Geometry("far_slot", "slot")
far_slot2 = Geometry("far_slot2", "slot", n_far=2)


def wide_rows(N: int, margin: int) -> Geometry:
    sn = ((TWO32 - 65536 - 512 - 1) // (2 * (N + margin))) // 8 * 8
    while not row_reach_ok(N, sn, margin):
        sn -= 8
    while row_reach_ok(N, sn + 8, margin):
        sn += 8
    return Geometry(f"wide_rows({N},{margin})", "rows", sn, N, margin)


def over_rows(N: int, margin: int) -> Geometry:
    return Geometry(f"over_rows({N},{margin})", "rows", wide_rows(N, margin).sn + 8, N, margin)


def arena_numel(specs: Sequence[Spec]) -> int:
    """Elements an arena needs to hold the placements (a multiple of 8)."""
    return _up(max(s.last for s in specs) + 1, 8)


def far_view(arena: torch.Tensor, t, strides, offset: int) -> torch.Tensor:
    """An ``as_strided`` view of ``arena`` with element strides (sb, sh, sn[, 1]) at ``offset``; ``t`` is a small
    contiguous [B, H, N, D] tensor, whose values the view then holds, or just a shape."""
    shape = tuple(t.shape) if isinstance(t, torch.Tensor) else tuple(t)
    strides = tuple(strides)[:3] + (1,)
    last = offset + sum((n - 1) * s for n, s in zip(shape, strides))
    assert arena.dim() == 1 and 0 <= offset and last < arena.numel(), "view outside the arena"
    v = arena.as_strided(shape, strides, arena.storage_offset() + offset)     # (as_strided counts from the storage)
    if isinstance(t, torch.Tensor):
        assert t.dtype == arena.dtype
        v.copy_(t)
    return v


def views(arena: torch.Tensor, geometry: Geometry, operands) -> List[torch.Tensor]:
    """One view per operand (tensor: copied in; shape: left as the arena has it), placed by ``geometry``."""
    shapes = [tuple(o.shape) if isinstance(o, torch.Tensor) else tuple(o) for o in operands]
    specs = geometry.place(shapes, arena.element_size())
    return [far_view(arena, o, s.strides, s.offset) for o, s in zip(operands, specs)]


def disjoint(specs: Sequence[Spec]) -> bool:
    """True when no two rows of any of the placements share an element (index arithmetic only)."""
    starts = torch.cat([s.row_starts() for s in specs])
    ends = torch.cat([s.row_starts() + s.shape[3] for s in specs])
    order = torch.argsort(starts)
    starts, ends = starts[order], ends[order]
    return bool((ends[:-1] <= starts[1:]).all())


def _sentinel64(sentinel: int) -> int:
    assert 0 <= sentinel < 1 << 16
    w = int.from_bytes(sentinel.to_bytes(2, "little") * 4, "little")
    return w - (1 << 64) if w >> 63 else w


def fill_sentinel(arena: torch.Tensor, sentinel: int = SENTINEL16) -> None:
    assert arena.element_size() > 1 or sentinel >> 8 == sentinel & 0xFF, "one-byte elements: a sentinel of two equal bytes"
    arena.view(torch.int64).fill_(_sentinel64(sentinel))


def _sentinel_scalar(dtype, device, sentinel: int = SENTINEL16) -> torch.Tensor:
    es = torch.empty((), dtype=dtype).element_size()
    if es == 1:
        assert sentinel >> 8 == sentinel & 0xFF
        return torch.full((1,), sentinel & 0xFF, dtype=torch.uint8, device=device).view(dtype).reshape(())
    s16 = sentinel - (1 << 16) if sentinel >> 15 else sentinel
    return torch.full((es // 2,), s16, dtype=torch.int16, device=device).view(dtype).reshape(())


def is_sentinel(t: torch.Tensor, sentinel: int = SENTINEL16) -> bool:
    """Every element of a (strided) tensor still holds the sentinel."""
    bits = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()]
    want = _sentinel_scalar(t.dtype, t.device, sentinel).view(bits)
    return bool((t.view(bits) == want).all())


def assert_untouched(arena: torch.Tensor, touched: Sequence[torch.Tensor], what: str = "", inputs=(),
                     sentinel: int = SENTINEL16) -> None:
    """The arena was filled with the sentinel before the operands were placed: write it back over the views, then the
    whole arena must be the sentinel again - a store at a truncated address shows as a foreign word.  (One reduction
    over the arena; it leaves the arena ready for the next case.)  ``inputs``: (view, source) pairs of operands the call
    only reads - they must still hold the source's values, or a stray store landed inside another operand's view."""
    for i, (v, src) in enumerate(inputs):
        assert torch.equal(v, src), f"{what}: input operand {i} changed under the call"
    for v in touched:
        if v.element_size() == 1:
            v.view(torch.uint8).fill_(sentinel & 0xFF)
        else:
            v.copy_(_sentinel_scalar(v.dtype, v.device, sentinel).expand(v.shape))
    bad = arena.view(torch.int64) != _sentinel64(sentinel)
    n_bad = int(bad.sum())
    if n_bad:
        first = int(bad.to(torch.uint8).argmax()) * (8 // arena.element_size())
        fill_sentinel(arena, sentinel)
        raise AssertionError(f"{what}: {n_bad} 8-byte words outside the operands were written, the first at element "
                             f"{first} (byte {first * arena.element_size()})")


# ------------------------------------------------------------------------------------------- a large page pool
@dataclass(frozen=True)
class PagePool:
    """The production layout of a paged ring inside the arena: page p of K is the ``page_numel`` elements from element
    ``p * stride`` on, page p of V the ``page_numel`` after them (``stride = 2 * page_numel``), so both buffers are plain
    views ``[n_pages, H_kv, P, D]`` with ``stride[0] = stride``.  ``p31`` / ``e31`` / ``p32``: the first page whose K
    part starts at or past 2^31 bytes / 2^31 elements / 2^32 bytes (``e31`` and ``p32`` coincide at item size 2)."""
    page_numel: int
    stride: int
    n_pages: int
    p31: int
    e31: int
    p32: int

    @property
    def picks(self) -> List[int]:
        """Pages on both sides of each line, the first and the last one, and a neighbour of each so that three table
        rows of three entries can be dealt (duplicates dropped, ascending)."""
        ps = {0, 1, self.p31 - 1, self.p31, self.p31 + 1, self.e31 - 1, self.e31, self.p32 - 1, self.p32, self.p32 + 1,
              self.n_pages - 1}
        return sorted(p for p in ps if 0 <= p < self.n_pages)

    def specs(self, Hkv: int, P: int, D: int) -> List[Spec]:
        """K and V page buffers as placements (for the CPU checks and the views)."""
        assert Hkv * P * D == self.page_numel
        return [Spec((self.n_pages, Hkv, P, D), off, (self.stride, P * D, D, 1)) for off in (0, self.page_numel)]


def page_pool(arena_numel: int, page_numel: int, itemsize: int) -> PagePool:
    stride = 2 * page_numel
    first = lambda x: -(-x // stride)                          # first page that starts at or past element x
    pp = PagePool(page_numel, stride, arena_numel // stride, first(TWO31 // itemsize), first(TWO31), first(TWO32 // itemsize))
    assert pp.p32 < pp.n_pages, "the arena holds no page past 2^32 bytes"
    return pp


def deal_pages(picks: Sequence[int], n_slots: int, per: int, p31: int, p32: int) -> List[List[int]]:
    """A table [n_slots][per] over the picked pages, -1 elsewhere: every row gets one page past 2^32 bytes and one
    below 2^31 bytes, no row is monotone (the far page comes first), no page is dealt twice."""
    lo = [p for p in picks if p < p31]
    mid = [p for p in picks if p31 <= p < p32]
    hi = [p for p in picks if p >= p32]
    assert len(lo) >= n_slots and len(hi) >= n_slots and per >= 2, (lo, mid, hi)
    tab = []
    for s in range(n_slots):
        row = ([hi[s], lo[-1 - s]] + ([mid[s]] if s < len(mid) else []))[:per]
        tab.append(row + [-1] * (per - len(row)))
    return tab


# ------------------------------------------------------------------------------------------- truncated addresses
def _wrap32(x: torch.Tensor) -> torch.Tensor:
    return ((x + TWO31) % TWO32) - TWO31


def truncations(elem: torch.Tensor, itemsize: int) -> dict:
    """Byte addresses a kernel forms for rows at element offsets ``elem`` (int64) under the three errors this module is
    built to show: the element offset kept in a signed 32-bit int, the byte offset in an unsigned, in a signed one."""
    byte = elem * itemsize
    return {"elem_i32": _wrap32(elem) * itemsize, "byte_u32": byte % TWO32, "byte_i32": _wrap32(byte)}


def exposed(operands: dict, itemsize: int, arena_numel: int) -> dict:
    """``operands``: name -> (row starts in elements, int64 tensor; row length in elements): every row of the arena a
    far case reads or stores.  Returns {(operand, error): rows} - the rows of that operand whose address under that error
    differs from the true one and lies outside the arena or on a run of sentinel words that no operand's row touches.  A
    kernel with the error then moves wrong bytes (far != near: the sentinel is NaN) or leaves a foreign word (the arena
    check).  A case is proven able to fail when no entry is 0."""
    starts = torch.cat([r for r, _ in operands.values()]) * itemsize
    ends = torch.cat([r + n for r, n in operands.values()]) * itemsize
    order = torch.argsort(starts)
    starts, ends = starts[order], ends[order]
    assert bool((ends[:-1] <= starts[1:]).all()), "the operands' rows overlap"
    out = {}
    for name, (rows, n) in operands.items():
        for err, addr in truncations(rows, itemsize).items():
            differs = addr != rows * itemsize
            outside = (addr < 0) | (addr + n * itemsize > arena_numel * itemsize)
            i = torch.searchsorted(starts, addr + n * itemsize)          # rows that start before this one's end ...
            prev_end = torch.where(i > 0, ends[(i - 1).clamp(min=0)], torch.zeros_like(addr))
            free = prev_end <= addr                                       # ... and the last of them ends before it starts
            out[(name, err)] = int((differs & (outside | free)).sum())
    return out


def slot_rows(spec: Spec, slots: Sequence[int]):
    """(row starts, row length) of the named slots (dim 0) of a placement."""
    B, H, N, D = spec.shape
    ar = lambda n, st: torch.arange(n, dtype=torch.int64) * st
    b = torch.tensor(list(slots), dtype=torch.int64) * spec.strides[0]
    assert all(0 <= x < B for x in slots)
    return (spec.offset + b[:, None, None] + ar(H, spec.strides[1])[None, :, None] + ar(N, spec.strides[2])[None, None, :]).reshape(-1), D


def sentinel_full(shape, dtype, device, sentinel: int = SENTINEL16) -> torch.Tensor:
    """An ordinary tensor that holds what a view of a freshly filled arena holds."""
    return _sentinel_scalar(dtype, device, sentinel).expand(tuple(shape)).clone() if torch.empty((), dtype=dtype).element_size() > 1 \
        else torch.full(tuple(shape), sentinel & 0xFF, dtype=torch.uint8, device=device).view(dtype)
