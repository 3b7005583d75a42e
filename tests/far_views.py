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
  elements for the 2-byte types; fp32 as for ``far_batch``), the first slots near.
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

    def place(self, shapes: Sequence[Tuple[int, int, int, int]], itemsize: int) -> List[Spec]:
        """Non-overlapping placements for operands of the given shapes, all in one arena."""
        shapes = [tuple(int(x) for x in s) for s in shapes]
        cols = [_up(s[3], 8) for s in shapes]                 # 16-byte aligned column blocks
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
            assert Bm * sb * itemsize < TWO31, "far_head: batches and rows must stay near"
        elif self.kind == "batch":
            sh = Nm * sn
            assert Hm * sh * itemsize < TWO31, "far_batch: heads and rows must stay near"
            sb = far
        else:                                                 # slot: the last slot far, S - 1 equal steps
            sh = Nm * sn
            sb = _up(-(-far // (Bm - 1)), 8)
            assert Hm * sh <= sb, "far_slot: a slot does not fit the slot stride"
        specs, c = [], 0
        for s, col in zip(shapes, cols):
            specs.append(Spec(s, c, (sb, sh, sn, 1)))
            c += col
        return specs


far_batch = Geometry("far_batch", "batch")
far_head = Geometry("far_head", "head")
band_head = Geometry("band_head", "band")
far_slot = Geometry("far_slot", "slot")


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


def fill_sentinel(arena: torch.Tensor) -> None:
    arena.view(torch.int64).fill_(SENTINEL64)


def _sentinel_scalar(dtype, device) -> torch.Tensor:
    n = torch.empty((), dtype=dtype).element_size() // 2
    return torch.full((n,), SENTINEL16, dtype=torch.int16, device=device).view(dtype).reshape(())


def is_sentinel(t: torch.Tensor) -> bool:
    """Every element of a (strided) tensor still holds the sentinel."""
    bits = {2: torch.int16, 4: torch.int32}[t.element_size()]
    want = _sentinel_scalar(t.dtype, t.device).view(bits)
    return bool((t.view(bits) == want).all())


def assert_untouched(arena: torch.Tensor, touched: Sequence[torch.Tensor], what: str = "", inputs=()) -> None:
    """The arena was filled with the sentinel before the operands were placed: write it back over the views, then the
    whole arena must be the sentinel again - a store at a truncated address shows as a foreign word.  (One reduction
    over the arena; it leaves the arena ready for the next case.)  ``inputs``: (view, source) pairs of operands the call
    only reads - they must still hold the source's values, or a stray store landed inside another operand's view."""
    for i, (v, src) in enumerate(inputs):
        assert torch.equal(v, src), f"{what}: input operand {i} changed under the call"
    for v in touched:
        v.copy_(_sentinel_scalar(v.dtype, v.device).expand(v.shape))
    bad = arena.view(torch.int64) != SENTINEL64
    n_bad = int(bad.sum())
    if n_bad:
        first = int(bad.to(torch.uint8).argmax()) * (8 // arena.element_size())
        fill_sentinel(arena)
        raise AssertionError(f"{what}: {n_bad} 8-byte words outside the operands were written, the first at element "
                             f"{first} (byte {first * arena.element_size()})")
