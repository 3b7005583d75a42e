"""Sink + sliding-window KV cache for decode, with a copy-free attention path.

Same observable behaviour as the reference's ``sink_attention/cache.py`` (``SinkCacheLayer`` :29-238,
``SinkAttentionCache`` :241-330): a fixed sink buffer ``[B, H_kv, num_sink, D]`` plus a circular window buffer
``[B, H_kv, window_size, D]``; prefill stores the state and hands the full K/V back (the prefill kernel masks),
a decode step overwrites one ring slot.  ``update()`` / ``get_kv()`` still return the linearised ``[sink, window]``
tensors for callers that want them, but attention itself no longer needs them:

    layer.append(k_new, v_new)                       # one slot written, no torch.cat
    out = layer.decode_attention(q, s_aux=sinks)     # sfa_decode_ring reads sink buffer + ring in place

The reference rebuilds ``[B, H_kv, ns+W, D]`` with up to three ``torch.cat`` per step and measures that copy as
costly as the attention itself (its README, "cache update + decode").  Bookkeeping is host-side Python on torch
tensors and works on any device; ``decode_attention`` needs the HIP library.
"""
from abc import ABC
from typing import List, Optional, Tuple

import torch

from .decode_kernel import rows16

try:  # the HF base classes are optional, exactly as in the reference (cache.py:20-26)
    from transformers.cache_utils import Cache as _HFCache, CacheLayerMixin as _HFLayer
    _HAS_HF = True
except ImportError:  # pragma: no cover
    _HAS_HF = False
    _HFCache = object
    _HFLayer = ABC


def pages_needed(tokens: int, window_size: int, page_size: int) -> int:
    """Table entries a slot touches once its ring has held at most ``tokens`` tokens: the prefix
    ``0 .. ceil(min(tokens, Wc) / P) - 1``.  The ring fills from slot 0 upwards until it is full (the prefill placement
    and the commit both do), so reads and stores stay inside that prefix (include/sfa.h, the paged pool)."""
    return -(-min(max(int(tokens), 0), window_size) // page_size)


class PageAllocator:
    """Host-side bookkeeping of a paged pool's table: a free list of pages and, per slot, the pages mapped so far.  Pure
    Python: it launches no kernel and never reads the device; the changed entries are written into ``table`` (device
    int32 ``[S, Wc / P]``) with torch ops.  It assumes that it alone writes the table it was given (a fresh table is
    all -1).

    Shared pages (``share``, behind ``fork_slots(share=True)``): ``refcount[p]`` is the number of table entries that name
    page p, and a page is on the free list iff its count is 0.  A page with a count above 1 is never stored into:
    ``reserve`` gives a slot that is about to write into such a page one of its own and returns the ``(src_page,
    dst_page)`` copies that every layer on this table must run (``sfa_pages_copy``) before the step.  What a step may
    write is decided on the host from token counts alone: while ``tokens_after <= Wc`` the ring has not wrapped, ring
    position equals token index, and the pages that intersect ``[lo, tokens_after)`` are the candidates (``lo[s]``: a
    lower bound of the tokens slot s's ring held when it last took part in a share); beyond ``Wc`` the host cannot know
    ``write_pos`` (a prompt longer than the ring is placed with ``write_pos = 0`` whatever its length modulo ``Wc``), so
    every shared entry of the slot is made private.  ``shared[s]`` says whether slot s ever took part in a share: a pool
    that never shares pays one flag test per slot in ``reserve``.  ``layers`` are the cache layers whose pools read this
    table."""

    def __init__(self, table: torch.Tensor, num_pages: int, page_size: int, window_size: int):
        self.table, self.num_pages, self.page_size, self.window_size = table, int(num_pages), int(page_size), int(window_size)
        self.free_list = list(range(self.num_pages - 1, -1, -1))        # pop() hands out page 0 first
        self.rows = [[] for _ in range(table.shape[0])]                 # slot -> its pages, entry j = table[slot][j]
        self.refcount = [0] * self.num_pages                            # page -> table entries that name it
        self.lo = [0] * table.shape[0]                                  # slot -> ring tokens at its last share
        self.shared = [False] * table.shape[0]                          # slot -> it may hold a page with a count above 1
        self.layers = []                                                # the layers attached to this table

    def attach(self, layer) -> None:
        """Register a layer whose pool reads this table: ``reserve_pages`` runs the page copies on every one."""
        if not any(l is layer for l in self.layers):
            self.layers.append(layer)

    def _slots(self, slots):
        lst = slots.tolist() if isinstance(slots, torch.Tensor) else [int(x) for x in slots]
        bad = [x for x in lst if not 0 <= x < len(self.rows)]
        if bad or len(set(lst)) != len(lst):
            raise ValueError(f"slots {lst}: each must name one slot of the pool of {len(self.rows)}, once")
        return lst

    def _write(self, rows, cols, vals):
        if rows:
            dev = self.table.device
            self.table[torch.tensor(rows, device=dev), torch.tensor(cols, device=dev)] = \
                torch.tensor(vals, dtype=torch.int32, device=dev)

    @staticmethod
    def _per_slot(x, n, what):
        lst = [x] * n if isinstance(x, int) else (x.tolist() if isinstance(x, torch.Tensor) else [int(v) for v in x])
        if len(lst) != n:
            raise ValueError(f"{what} must be one number or one per slot ({n}), got {len(lst)}")
        return lst

    def reserve(self, slots, tokens_after, tokens_before=None):
        """Map the prefix of pages ``tokens_after`` needs and make private every shared page the step may store into
        (the class docstring has the rule).  Returns the ``(src_page, dst_page)`` copies decided, in table order; empty
        for slots that share nothing.  ``tokens_before`` (ring tokens, one number or one per slot) lowers ``lo`` of a slot
        first, for a caller that re-admitted it below the count of its last share.  Raises ``RuntimeError("out of pages:
        need X, free Y")``, copies and growth counted together, before anything changes."""
        lst = self._slots(slots)
        tok = self._per_slot(tokens_after, len(lst), "tokens_after")
        lo = [self.lo[s] for s in lst] if tokens_before is None else \
            [min(self.lo[s], max(b, 0)) for s, b in zip(lst, self._per_slot(tokens_before, len(lst), "tokens_before"))]
        P = self.page_size
        more = [max(pages_needed(t, self.window_size, P) - len(self.rows[s]), 0) for s, t in zip(lst, tok)]
        # an entry is copied if, after the copies decided before it in this call, its page still has another owner: of a
        # source and its last fork reserving together only the first one copies
        cow, taken, private = [], {}, []
        for s, t, l in zip(lst, tok, lo):
            if not self.shared[s]:          # never took part in a share: nothing to look at, whatever its length
                continue
            row = self.rows[s]
            if t > self.window_size:        # every entry; afterwards the slot holds no shared page
                js = range(len(row))
                private.append(s)
            else:                           # the entries j with j P < t and (j + 1) P > lo
                js = range(min(l // P, len(row)), min(-(-t // P), len(row)))
            for j in js:
                if self.refcount[row[j]] - taken.get(row[j], 0) > 1:
                    cow.append((s, j))
                    taken[row[j]] = taken.get(row[j], 0) + 1
        if len(cow) + sum(more) > len(self.free_list):
            raise RuntimeError(f"out of pages: need {len(cow) + sum(more)}, free {len(self.free_list)}")
        for s, l in zip(lst, lo):
            self.lo[s] = l
        for s in private:
            self.shared[s] = False
        rows, cols, vals, copies = [], [], [], []
        for s, j in cow:
            old, page = self.rows[s][j], self.free_list.pop()
            self.refcount[old] -= 1
            self.refcount[page] = 1
            self.rows[s][j] = page
            rows.append(s), cols.append(j), vals.append(page)
            copies.append((old, page))
        for s, m in zip(lst, more):
            for _ in range(m):
                page = self.free_list.pop()
                self.refcount[page] = 1
                rows.append(s), cols.append(len(self.rows[s])), vals.append(page)
                self.rows[s].append(page)
        self._write(rows, cols, vals)
        return copies

    def share(self, src, dst, ring_tokens) -> None:
        """Alias table rows (host lists only, nothing is popped from the free list): the row of ``dst[i]`` becomes the row
        of ``src[i]`` and every aliased page gains a reference.  ``ring_tokens[i]`` (one number or one per pair) is the
        exact number of tokens the ring of ``src[i]`` holds; it becomes ``lo`` of both slots.  One source may feed many
        destinations.  A destination must map no page (``free`` comes first) and differ from its source."""
        src, dst = [int(x) for x in src], self._slots(dst)
        if len(src) != len(dst):
            raise ValueError(f"share: src and dst must pair up, got {len(src)} and {len(dst)} entries")
        lo = self._per_slot(ring_tokens, len(dst), "ring_tokens")
        bad = [s for s in src if not 0 <= s < len(self.rows)]
        if bad or any(s == d for s, d in zip(src, dst)) or set(src) & set(dst):
            raise ValueError(f"share: src {src} / dst {dst}: each source must be a slot of the pool of {len(self.rows)} "
                             f"that is no destination of the call")
        for d in dst:
            if self.rows[d]:
                raise ValueError(f"share: slot {d} still maps {len(self.rows[d])} pages: free_pages({d}) comes first")
        for s, d, l in zip(src, dst, lo):
            self.rows[d] = list(self.rows[s])
            self.lo[s] = self.lo[d] = max(int(l), 0)
            self.shared[s] = self.shared[d] = True
        for s in set(src):                  # one pass over a source's pages, however many destinations it feeds
            n = src.count(s)
            for page in self.rows[s]:
                self.refcount[page] += n
        if dst:                             # whole rows, copied where the table lives (a destination's row was all -1)
            dev = self.table.device
            self.table[torch.tensor(dst, device=dev)] = self.table[torch.tensor(src, device=dev)]

    def free(self, slots) -> None:
        rows, cols = [], []
        for s in self._slots(slots):
            for j, page in enumerate(self.rows[s]):
                rows.append(s), cols.append(j)
                self.refcount[page] -= 1
                if self.refcount[page] == 0:
                    self.free_list.append(page)
            self.rows[s] = []
            self.lo[s], self.shared[s] = 0, False
        self._write(rows, cols, [-1] * len(rows))

    def pool_bytes(self, H_kv: int, D: int, elem_bytes: int) -> int:
        """Bytes of ring memory (K and V) the mapped pages hold, a page that several slots share counted once."""
        return 2 * len({p for r in self.rows for p in r}) * H_kv * self.page_size * D * elem_bytes


def _copy_pages(pages: PageAllocator, copies) -> None:
    """Run the page copies ``reserve`` decided: one upload of the pairs, then ``sfa_pages_copy`` on every layer attached to
    the table, on the current stream.  A layer left out would go on reading the page of another sequence."""
    if not copies:
        return
    pairs = torch.tensor([[s for s, _ in copies], [d for _, d in copies]], dtype=torch.int32, device=pages.table.device)
    for layer in pages.layers:
        if layer._pages is pages:       # a layer whose pool was set up anew has left this table
            layer._pages_copy(pairs[0], pairs[1])


class SinkCacheLayer(_HFLayer if _HAS_HF else object):
    """One layer's cache: ``num_sink`` pinned leading tokens + a ring of the last ``window_size`` others."""

    def __init__(self, num_sink: int, window_size: int):
        if _HAS_HF:
            super().__init__()
        self.num_sink = int(num_sink)
        self.window_size = int(window_size)
        self.sink_k = self.sink_v = self.window_k = self.window_v = None
        self.sink_len = 0        # valid rows of the sink buffer
        self.window_len = 0      # valid slots of the ring
        self.write_pos = 0       # ring slot the next decoded token goes to
        self.prefilled = False
        self.seen_tokens = 0
        self.is_initialized = False

    # ------------------------------------------------------------------ state
    def lazy_initialization(self, key_states: torch.Tensor, *_, **__):
        B, H_kv, _n, D = key_states.shape
        mk = lambda n: torch.zeros(B, H_kv, n, D, dtype=key_states.dtype, device=key_states.device)
        self.sink_k, self.sink_v = mk(self.num_sink), mk(self.num_sink)
        self.window_k, self.window_v = mk(self.window_size), mk(self.window_size)
        self.is_initialized = True

    def _prefill(self, k, v):
        N = k.shape[2]
        self.seen_tokens = N
        ns = min(N, self.num_sink)
        self.sink_k[:, :, :ns] = k[:, :, :ns]
        self.sink_v[:, :, :ns] = v[:, :, :ns]
        self.sink_len = ns
        rest = N - ns
        if rest <= 0:
            self.window_len, self.write_pos = 0, 0
        elif rest <= self.window_size:
            self.window_k[:, :, :rest] = k[:, :, ns:]
            self.window_v[:, :, :rest] = v[:, :, ns:]
            self.window_len = rest
            self.write_pos = rest % self.window_size
        else:   # keep only the newest window_size tokens; the ring is full and wraps at slot 0
            self.window_k.copy_(k[:, :, N - self.window_size:])
            self.window_v.copy_(v[:, :, N - self.window_size:])
            self.window_len, self.write_pos = self.window_size, 0
        self.prefilled = True
        return k, v

    def append(self, k: torch.Tensor, v: torch.Tensor) -> None:
        """Write decoded token(s) ``[B, H_kv, n, D]`` into the ring (oldest evicted).  No linearisation."""
        self._refuse_per_seq("append")
        if not self.is_initialized:
            self.lazy_initialization(k)
        if not self.prefilled:      # first tokens ever: same placement as a prefill (sinks first)
            self._prefill(k, v)
            return
        for i in range(k.shape[2]):
            self.seen_tokens += 1
            if self.window_size > 0:
                self.window_k[:, :, self.write_pos] = k[:, :, i]
                self.window_v[:, :, self.write_pos] = v[:, :, i]
                self.write_pos = (self.write_pos + 1) % self.window_size
                self.window_len = min(self.window_len + 1, self.window_size)
        self.prefilled = True

    def update(self, key_states, value_states, cache_kwargs: Optional[dict] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """Reference-compatible update: prefill returns the full input K/V, decode returns linearised [sink, window]."""
        self._refuse_per_seq("update")
        if not self.is_initialized:
            self.lazy_initialization(key_states)
        if not self.prefilled:
            return self._prefill(key_states, value_states)
        self.append(key_states, value_states)
        return self.get_kv()

    def get_kv(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """Chronological ``[B, H_kv, sink_len + window_len, D]`` copy (oldest first) - only for callers that need it."""
        self._refuse_per_seq("get_kv")
        ks, vs = [self.sink_k[:, :, :self.sink_len]], [self.sink_v[:, :, :self.sink_len]]
        if self.window_len > 0:
            if self.window_len < self.window_size or self.write_pos == 0:
                ks.append(self.window_k[:, :, :self.window_len])
                vs.append(self.window_v[:, :, :self.window_len])
            else:
                ks += [self.window_k[:, :, self.write_pos:], self.window_k[:, :, :self.write_pos]]
                vs += [self.window_v[:, :, self.write_pos:], self.window_v[:, :, :self.write_pos]]
        return torch.cat(ks, dim=2), torch.cat(vs, dim=2)

    # -------------------------------------------------------------- attention
    def decode_attention(self, q: torch.Tensor, s_aux: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Single-query attention of ``q [B, H_q, 1, D]`` over the cached keys, reading both buffers in place."""
        self._refuse_per_seq("decode_attention")
        from .decode_kernel import sink_decode_attention_ring
        return sink_decode_attention_ring(q, self.sink_k, self.sink_v, self.sink_len, self.window_k, self.window_v,
                                          self.window_len, s_aux=s_aux)

    def decode_step(self, q: torch.Tensor, k_new: torch.Tensor, v_new: torch.Tensor,
                    s_aux: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One generation step = ``append(k_new, v_new)`` + ``decode_attention(q)``, as ONE kernel pass once the cache
        is in steady state (``sfa_decode_ring_step``: the kernel stores the token into its ring slot and attends over
        the updated cache; no ``torch.cat``, no separate slot-write launches)."""
        self._refuse_per_seq("decode_step")
        steady = (self.prefilled and self.window_size > 0 and k_new.shape[2] == 1 and self.window_k is not None
                  and self.window_k.is_cuda)
        if not steady:
            self.append(k_new, v_new)
            return self.decode_attention(q, s_aux=s_aux)
        pos = self.write_pos
        new_len = min(self.window_len + 1, self.window_size)
        out = self._ring_step(q, k_new, v_new, new_len, pos, s_aux)
        self.seen_tokens += 1
        self.write_pos = (pos + 1) % self.window_size
        self.window_len = new_len
        return out

    def _ring_step(self, q, k_new, v_new, new_len, pos, s_aux):
        """sfa_decode_ring_step with the per-layer constants (buffer descriptors, workspace) built once: at B=1 the
        step is host-bound, so the Python work per token is kept to the four per-call descriptors."""
        from . import _native as N
        st = getattr(self, "_step_state", None)
        key = (self.sink_k.data_ptr(), self.window_k.data_ptr(), q.shape, q.dtype)
        if st is None or st["key"] != key:
            B, H_q, _one, D = q.shape
            H_kv = self.sink_k.shape[1]
            if q.dtype != self.window_k.dtype or q.dtype not in N.SFA_DTYPE:
                raise TypeError("q and the cache buffers must share one dtype")
            assert _one == 1 and H_q % H_kv == 0 and (D * q.element_size()) % 16 == 0
            st = self._step_consts(key, q)
        N.require_gpu(q, k_new, v_new, s_aux)
        if k_new.dtype != q.dtype or v_new.dtype != q.dtype or k_new.shape != v_new.shape:
            raise TypeError("k_new / v_new must be [B, H_kv, 1, D] tensors of q's dtype")
        q, k_new, v_new = N.unit_inner(q.detach()), N.unit_inner(k_new.detach()), N.unit_inner(v_new.detach())
        s_aux_f, aux = self._aux(s_aux)
        out = torch.empty(q.shape, device=q.device, dtype=q.dtype)
        sk, sv, wk, wv = st["descs"]
        with torch.cuda.device(q.device):
            rc = st["lib"].sfa_decode_ring_step(N.desc(q), sk, sv, self.sink_len, wk, wv, new_len, pos, N.desc(k_new),
                                                N.desc(v_new), N.desc(out), aux,
                                                st["ws"].data_ptr(), st["ws"].numel(), st["scale"],
                                                self._decode_flags(N), N.stream_ptr(q.device))
        N.check(rc, "sfa_decode_ring_step")
        return out

    # ------------------------------------------- several new tokens (speculative verify, chunked continuation)
    def extend_attention(self, q: torch.Tensor, k_new: torch.Tensor, v_new: torch.Tensor,
                         s_aux: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Attention of n new queries ``q [B, H_q, n, D]`` over the cache plus the chunk's own ``k_new`` / ``v_new``
        ``[B, H_kv, n, D]``, exactly as n successive ``decode_step`` calls would see it, WITHOUT modifying the cache
        (``sfa_decode_ring_multi``, commit off).  Speculative verify: ``out = extend_attention(q, k, v)``, then
        ``append(k[:, :, :a], v[:, :, :a])`` for the ``a`` accepted drafts - rejected ones never enter the ring."""
        self._refuse_per_seq("extend_attention")
        return self._ring_multi(q, k_new, v_new, s_aux, commit=False)

    def extend_step(self, q: torch.Tensor, k_new: torch.Tensor, v_new: torch.Tensor,
                    s_aux: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``extend_attention`` followed by the commit of all n tokens: afterwards the cache is bitwise the state that
        ``append(k_new, v_new)`` leaves (the kernels store the chunk after every read of the slots it overwrites)."""
        self._refuse_per_seq("extend_step")
        n = q.shape[2]
        out = self._ring_multi(q, k_new, v_new, s_aux, commit=True)
        self.seen_tokens += n
        self.write_pos = (self.write_pos + n) % self.window_size
        self.window_len = min(self.window_len + n, self.window_size)
        return out

    def _ring_multi(self, q, k_new, v_new, s_aux, commit, tree=None):
        """sfa_decode_ring_multi with the per-layer constants (buffer descriptors, workspace for the full cache) built once
        per chunk shape, as _ring_step does."""
        from . import _native as N
        if not (self.is_initialized and self.prefilled):
            raise ValueError("extend_attention / extend_step need a prefilled cache: the first chunk is a prefill "
                             "(sink_flash_attention)")
        N.require_gpu(q, k_new, v_new, s_aux)
        if self.window_size < 1:
            raise ValueError("extend_attention / extend_step need a ring of at least one slot (window_size >= 1)")
        if not self.window_k.is_cuda:
            raise RuntimeError("sink_attention runs only on MI355X (HIP) tensors; got a CPU cache and there is no CPU "
                               "fallback")
        B, H_q, n, D = q.shape
        H_kv = self.sink_k.shape[1]
        self._check_chunk(N, q, k_new, v_new, None, "[B, H_kv, n, D]")
        st = getattr(self, "_multi_state", None)
        key = (self.sink_k.data_ptr(), self.window_k.data_ptr(), q.shape, q.dtype)
        if st is None or st["key"] != key:
            ws_bytes = N.lib().sfa_decode_multi_workspace_bytes(B, H_q, H_kv, n, self.num_sink + self.window_size + n, D,
                                                                N.SFA_DTYPE[q.dtype])
            if ws_bytes == 0:
                raise ValueError(f"D={D}: a K/V row must be a multiple of 16 bytes, <= 1 KiB")
            st = self._call_consts("_multi_state", key, ws_bytes, False, q)
        q, k_new, v_new = rows16(q), rows16(k_new), rows16(v_new)
        s_aux_f, aux = self._aux(s_aux)
        out = torch.empty((B, H_q, n, D), device=q.device, dtype=q.dtype)
        sk, sv, wk, wv = st["descs"]
        with torch.cuda.device(q.device):
            if tree is not None:
                rc = st["lib"].sfa_decode_ring_tree(N.desc(q), sk, sv, self.sink_len, wk, wv, self.window_len,
                                                    self.write_pos, N.desc(k_new), N.desc(v_new), N.desc(out), aux,
                                                    tree[0].data_ptr(), tree[1], st["ws"].data_ptr(), st["ws"].numel(),
                                                    st["scale"], 0, N.stream_ptr(q.device))
            else:
                rc = st["lib"].sfa_decode_ring_multi(N.desc(q), sk, sv, self.sink_len, wk, wv, self.window_len,
                                                     self.write_pos, N.desc(k_new), N.desc(v_new), N.desc(out), aux,
                                                     1 if commit else 0, st["ws"].data_ptr(), st["ws"].numel(),
                                                     st["scale"], 0, N.stream_ptr(q.device))
        N.check(rc, "sfa_decode_ring_tree" if tree is not None else "sfa_decode_ring_multi")
        return out

    def _call_consts(self, attr, key, ws_bytes, zeroed, q):
        """The per-layer constants of one family of calls, built once per ``key`` and kept in ``self.<attr>``: the
        library handle, the softmax scale, the descriptors of the four cache buffers and a workspace of ``ws_bytes``
        (zero-filled if ``zeroed``) on q's device."""
        import math
        from . import _native as N
        st = dict(key=key, lib=N.lib(), scale=1.0 / math.sqrt(q.shape[3]),
                  descs=[N.desc(t) for t in (self.sink_k, self.sink_v, self.window_k, self.window_v)],
                  ws=(torch.zeros if zeroed else torch.empty)((max(int(ws_bytes), 256),), device=q.device,
                                                              dtype=torch.uint8))
        setattr(self, attr, st)
        return st

    def _step_consts(self, key, q):
        """``_step_state``, shared by ``decode_step`` and ``decode_step_dyn``: the workspace is owned across calls and
        zeroed once, the one-pass decode keeps its arrival counters there."""
        from . import _native as N
        B, H_q, _one, D = q.shape
        ws_bytes = N.lib().sfa_decode_workspace_bytes(B, H_q, self.sink_k.shape[1], self.num_sink + self.window_size, D,
                                                      N.SFA_DTYPE[q.dtype])
        return self._call_consts("_step_state", key, ws_bytes, True, q)

    def _check_chunk(self, N, q, k_new, v_new, out, layout):
        """Shape of ``k_new`` / ``v_new`` against q and the cache (``layout``: how the message spells it), one dtype
        for all of them, and ``out`` where the caller brings one."""
        shape = (q.shape[0], self.sink_k.shape[1], q.shape[2], q.shape[3])
        if k_new.shape != shape or v_new.shape != k_new.shape:
            raise ValueError(f"k_new / v_new must be {layout} = {shape}, got {tuple(k_new.shape)}")
        if self._kv8:
            self._act16("q, k_new and v_new", q, k_new, v_new)
        elif q.dtype != self.window_k.dtype or k_new.dtype != q.dtype or v_new.dtype != q.dtype or q.dtype not in N.SFA_DTYPE:
            raise TypeError("q, k_new, v_new and the cache buffers must share one dtype")
        if out is not None and (out.shape != q.shape or out.dtype != q.dtype):
            raise ValueError(f"out must be a {tuple(q.shape)} tensor of q's dtype")

    @staticmethod
    def _aux(s_aux):
        """``s_aux`` as the fp32 tensor the kernels read (the caller holds it across the call) and its pointer."""
        if s_aux is None:
            return None, None
        f = s_aux.detach().contiguous().float()
        return f, f.data_ptr()

    one_pass = False     # opt-in: SFA_FLAG_DECODE_ONE_PASS (last-arriver fold inside the split kernel, one launch)

    def _decode_flags(self, N) -> int:
        # Measured on MI355X (round 3, fence-free fold: write-through partial stores, sc1 loads; profiles/r03_kbench_decode_1pass.log):
        # B=1, 4100 keys 21.2 vs 19.2 us with two launches (the fold's loads are round trips to the memory side, dearer than
        # a back-to-back launch), 132 keys (one split) 15.8 vs 19.2 us - so two launches stay the default.
        return N.FLAG_DECODE_ONE_PASS if self.one_pass else 0

    # ------------------------------------------------ device-resident state (hipGraph capture)
    def enable_device_state(self, per_sequence: bool = False) -> torch.Tensor:
        """Move the ring bookkeeping {sink_len, window_len, write_pos} to a device int32 tensor so that
        ``decode_step_dyn``, ``extend_attention_dyn``, ``extend_step_dyn`` and ``commit_dyn`` need no host-side integers:
        a whole generation or speculative step can then be captured with ``torch.cuda.graph`` and replayed (the kernels
        read and advance the state themselves; the calls may be mixed on one state).  Call after prefill.  The host-state
        calls (``append``, ``decode_step``, ``extend_step``) do not update the device state, nor the dyn calls the host
        counters: switch with ``enable_device_state()`` / ``pull_state()``.

        ``per_sequence=True``: one state row ``{sink_len, window_len, write_pos, seen}`` per batch row, an int32 ``[B, 4]``
        tensor, every row starting from the host counters (``seen = seen_tokens``).  The cache then enters per-sequence
        mode, as after ``prefill_varlen``: the dyn calls advance each row on its own (``commit_dyn`` takes B counts) and
        the host-state methods raise."""
        if self._per_seq:
            if per_sequence:
                return self._dev_state
            raise RuntimeError("this cache is in per-sequence mode: its state is the [B, 4] tensor of "
                               "enable_device_state(per_sequence=True) / prefill_varlen")
        assert self.is_initialized and self.prefilled and self.window_size > 0, "prefill the cache first"
        if per_sequence:
            row = [self.sink_len, self.window_len, self.write_pos, self.seen_tokens]
            self._dev_state = torch.tensor([row] * self.window_k.shape[0], dtype=torch.int32, device=self.window_k.device)
            self._per_seq = True
            return self._dev_state
        self._dev_state = torch.tensor([self.sink_len, self.window_len, self.write_pos], dtype=torch.int32,
                                       device=self.window_k.device)
        return self._dev_state

    def pull_state(self) -> None:
        """Refresh the host-side counters from the device state (one small device-to-host copy).  ``seen_tokens`` is
        exact only while fewer than ``window_size`` tokens were committed since the last pull (the state holds no token
        count: a full ring's ``write_pos`` is taken modulo ``window_size``).  Per-sequence mode: ``sink_len``,
        ``window_len``, ``write_pos`` and ``seen_tokens`` become host lists with one exact value per sequence."""
        st = getattr(self, "_dev_state", None)
        if st is not None and self._per_seq:
            rows = st.tolist()
            self.sink_len, self.window_len, self.write_pos, self.seen_tokens = ([r[i] for r in rows] for i in range(4))
        elif st is not None:
            sl, wl, wp = st.tolist()
            W = self.window_size
            if wl < W:                       # still filling: one slot per step
                steps = wl - self.window_len
            elif self.window_len < W:        # filled up since the last pull: the step that took the last slot wrapped
                steps = (W - self.window_len) + wp          # write_pos to 0, every later step advanced it by one
            else:                            # full before and after (steps counted modulo the ring size)
                steps = (wp - self.write_pos) % W
            self.seen_tokens += steps
            self.sink_len, self.window_len, self.write_pos = sl, wl, wp

    def decode_step_dyn(self, q: torch.Tensor, k_new: torch.Tensor, v_new: torch.Tensor,
                        s_aux: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                        slots=None) -> torch.Tensor:
        """``decode_step`` with the state on the device (``sfa_decode_ring_step_dyn``): capturable into a hipGraph.
        ``out`` (optional, [B,H_q,1,D]) lets the caller keep a static output buffer across replays.  Per-sequence mode
        (``sfa_decode_ring_step_rows``): every row stores its token at its own slot and attends over its own keys.
        ``slots`` (``sfa_decode_ring_step_slots``, see ``init_pool``): batch row b works on cache row ``slots[b]``; a row
        with ``slots[b] = -1`` is inactive (zeros in ``out``, nothing stored, no state moves)."""
        from . import _native as N
        self._refuse_fp8("decode_step_dyn")
        slots = self._slots_arg(slots, q.shape[0], writes=True)
        st = getattr(self, "_dev_state", None)
        assert st is not None, "call enable_device_state() first"
        ss = getattr(self, "_step_state", None)
        key = (self.sink_k.data_ptr(), self.window_k.data_ptr(), q.shape, q.dtype)
        if ss is None or ss["key"] != key:
            ss = self._step_consts(key, q)
        N.require_gpu(q, k_new, v_new, s_aux)
        if k_new.dtype != q.dtype or v_new.dtype != q.dtype or q.dtype != self.window_k.dtype:
            raise TypeError("q, k_new, v_new and the cache buffers must share one dtype")
        q, k_new, v_new = N.unit_inner(q.detach()), N.unit_inner(k_new.detach()), N.unit_inner(v_new.detach())
        s_aux_f, aux = self._aux(s_aux)
        if out is None:
            out = torch.empty(q.shape, device=q.device, dtype=q.dtype)
        sk, sv, wk, wv = ss["descs"]
        lib = ss["lib"]
        if slots is not None:
            N.require_gpu(slots)
            fn, name, tail = lib.sfa_decode_ring_step_slots, "sfa_decode_ring_step_slots", (slots.data_ptr(),)
        elif self._per_seq:
            fn, name, tail = lib.sfa_decode_ring_step_rows, "sfa_decode_ring_step_rows", ()
        else:
            fn, name, tail = lib.sfa_decode_ring_step_dyn, "sfa_decode_ring_step_dyn", ()
        with torch.cuda.device(q.device):
            rc = fn(N.desc(q), sk, sv, wk, wv, N.desc(k_new), N.desc(v_new), N.desc(out), aux, st.data_ptr(), *tail,
                    ss["ws"].data_ptr(), ss["ws"].numel(), ss["scale"], self._decode_flags(N), N.stream_ptr(q.device))
        N.check(rc, name)
        return out

    # ---------------------------- several new tokens with the state on the device (capturable speculative step)
    def extend_attention_dyn(self, q: torch.Tensor, k_new: torch.Tensor, v_new: torch.Tensor,
                             s_aux: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                             slots=None) -> torch.Tensor:
        """``extend_attention`` with the state on the device (``sfa_decode_ring_multi_dyn``, commit off): capturable into a
        hipGraph, no host sync.  Neither the cache nor the device state changes.  The output is bitwise what
        ``extend_attention`` gives at the same state.  ``out`` (optional, [B, H_q, n, D]) is a static output buffer.
        Per-sequence mode (``sfa_decode_ring_multi_rows``): each row attends with its own state; ``extend_step_dyn``
        then advances every row by n.  ``slots`` (``sfa_decode_ring_multi_slots``): row b attends over cache row
        ``slots[b]`` of the pool; the same slot may be named twice here (nothing is written)."""
        return self._ring_multi_dyn(q, k_new, v_new, s_aux, out, commit=False, slots=slots)

    def extend_step_dyn(self, q: torch.Tensor, k_new: torch.Tensor, v_new: torch.Tensor,
                        s_aux: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                        slots=None) -> torch.Tensor:
        """``extend_step`` with the state on the device: attend, commit all n tokens, advance the device state.  The host
        counters are refreshed by ``pull_state()``.  ``slots``: as for ``decode_step_dyn`` (each slot at most once)."""
        return self._ring_multi_dyn(q, k_new, v_new, s_aux, out, commit=True, slots=slots)

    def commit_dyn(self, k_new: torch.Tensor, v_new: torch.Tensor, count: torch.Tensor, slots=None) -> None:
        """Store the first ``a = clamp(count, 0, n)`` tokens of a chunk ``[B, H_kv, n, D]`` into the ring and advance the
        device state (``sfa_ring_commit_dyn``): afterwards buffers and state are what ``append(k_new[:, :, :a], ...)``
        leaves.  ``count`` is a 0-d or 1-element integer tensor on the GPU (the acceptance count of a speculative step,
        computed by torch ops); it is never read on the host.  Per-sequence mode (``sfa_ring_commit_rows``): ``count``
        holds B values, row b commits its first ``clamp(count[b], 0, n)`` tokens.  ``slots``
        (``sfa_ring_commit_slots``): row b commits into cache row ``slots[b]`` (each slot at most once; an inactive row
        commits nothing)."""
        return self._commit_dyn(k_new, v_new, count, None, slots)

    def _commit_dyn(self, k_new, v_new, count, path, slots=None):
        """sfa_ring_commit[_path]_{dyn,rows,slots}: one count for the shared state, B of them for per-sequence rows."""
        from . import _native as N
        self._refuse_fp8("commit_path_dyn" if path is not None else "commit_dyn")
        slots = self._slots_arg(slots, k_new.shape[0], writes=True)
        st = self._require_dyn("commit_path_dyn" if path is not None else "commit_dyn")
        if not isinstance(count, torch.Tensor) or count.dtype.is_floating_point or count.dtype.is_complex \
                or count.dtype == torch.bool:
            raise TypeError("count must be an integer tensor")
        B, H_kv, _w, D = self.window_k.shape
        if slots is not None:           # the buffers are the pool: B is the chunk's
            B = slots.numel()
        if self._per_seq and count.numel() != B:
            raise ValueError(f"count must hold B = {B} values in per-sequence mode (one per sequence), "
                             f"got shape {tuple(count.shape)}")
        if not self._per_seq and count.numel() != 1:
            raise ValueError(f"count must hold one value, got shape {tuple(count.shape)}")
        N.require_gpu(k_new, v_new, count, self.window_k, slots)
        if k_new.dim() != 4 or k_new.shape[:2] != (B, H_kv) or k_new.shape[3] != D or v_new.shape != k_new.shape \
                or k_new.shape[2] < 1:
            raise ValueError(f"k_new / v_new must be [B, H_kv, n, D] = [{B}, {H_kv}, n, {D}], got {tuple(k_new.shape)}")
        if k_new.dtype != self.window_k.dtype or v_new.dtype != k_new.dtype:
            raise TypeError("k_new / v_new must have the cache buffers' dtype")
        k_new, v_new = self._rows16(k_new), self._rows16(v_new)
        cnt = count.reshape(B if self._per_seq else 1)
        if cnt.dtype != torch.int32:
            cnt = cnt.to(torch.int32)      # a cast kernel: capturable
        if self._per_seq:
            cnt = cnt.contiguous()
        wk, wv = self._ring_descs()
        mode = "slots" if slots is not None else "rows" if self._per_seq else "dyn"
        name, mid = "sfa_ring_commit_" + mode, ()
        if path is not None:
            from .decode_kernel import tree_path_dev
            pt, pstride = tree_path_dev(path, B, k_new.shape[2], k_new.device)
            name, mid = "sfa_ring_commit_path_" + mode, (pt.data_ptr(), pstride)
        with torch.cuda.device(k_new.device):
            rc = getattr(N.lib(), name)(wk, wv, N.desc(k_new), N.desc(v_new), cnt.data_ptr(), *mid, st.data_ptr(),
                                        *(() if slots is None else (slots.data_ptr(),)), N.stream_ptr(k_new.device))
        N.check(rc, name)

    # ------------------------------- tree-structured speculative verify (Medusa / EAGLE / SpecInfer draft trees)
    def extend_attention_tree(self, q: torch.Tensor, k_new: torch.Tensor, v_new: torch.Tensor, parent,
                              s_aux: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Verify a draft TREE of n <= 64 nodes in one pass (``sfa_decode_ring_tree``), host state, cache untouched.
        ``parent`` ([n] shared or [B, n]; list or integer tensor): ``parent[u]`` in [-1, u), -1 = a root hanging off the
        cache; checked on the host (a device tensor is synced).  Row u of ``q`` / ``k_new`` / ``v_new`` is node u; it
        attends to what the last of ``depth[u] + 1`` ``decode_step`` calls appending its root-to-u path would see
        (RoPE position of node u: ``seen_tokens + depth[u]``, see ``spec_tree.tree_depth``).  A chain
        (``parent = [-1, 0, ..., n - 2]``) gives ``extend_attention`` bitwise.  Commit the accepted path with
        ``commit_path``."""
        self._refuse_per_seq("extend_attention_tree")
        from .decode_kernel import tree_parent_host
        tree = tree_parent_host(parent, q.shape[0], q.shape[2], q.device)
        return self._ring_multi(q, k_new, v_new, s_aux, commit=False, tree=tree)

    def extend_attention_tree_dyn(self, q: torch.Tensor, k_new: torch.Tensor, v_new: torch.Tensor,
                                  parent: torch.Tensor, s_aux: Optional[torch.Tensor] = None,
                                  out: Optional[torch.Tensor] = None, slots=None) -> torch.Tensor:
        """``extend_attention_tree`` with the state on the device (``sfa_decode_ring_tree_dyn``; per-sequence mode
        ``sfa_decode_ring_tree_rows``, row b with its own state and tree): capturable, no host sync, neither the cache
        nor the state changes.  ``parent`` is an integer tensor ([n] or [B, n]) that is never read on the host: an entry
        outside [-1, u) reads as -1 (a root).  ``slots`` (``sfa_decode_ring_tree_slots``): row b verifies its tree
        against cache row ``slots[b]`` (the same slot may be named twice: nothing is written)."""
        from .decode_kernel import tree_parent_dev
        self._refuse_fp8("extend_attention_tree_dyn")
        if q.shape[2] > 64:
            raise ValueError(f"a tree chunk holds at most 64 nodes, got n = {q.shape[2]}")
        tree = tree_parent_dev(parent, q.shape[0], q.shape[2], q.device)
        return self._ring_multi_dyn(q, k_new, v_new, s_aux, out, commit=False, tree=tree, slots=slots)

    def commit_path_dyn(self, k_new: torch.Tensor, v_new: torch.Tensor, path: torch.Tensor,
                        count: torch.Tensor, slots=None) -> None:
        """Store an accepted tree path (``sfa_ring_commit_path_dyn`` / ``_rows``): with ``a = clamp(count, 0, n)`` the
        chunk rows ``path[:a]`` (``path`` [n] or [B, n], entries clamped into [0, n)) enter the ring in that order and
        the device state advances by a - buffers and state are then what ``append(k_new[:, :, path[:a]], ...)`` leaves.
        ``count`` follows the rules of ``commit_dyn`` (one value, or B values in per-sequence mode).  No host sync.
        ``slots`` (``sfa_ring_commit_path_slots``): as for ``commit_dyn``."""
        if not isinstance(path, torch.Tensor):
            raise TypeError("path must be an integer tensor")
        return self._commit_dyn(k_new, v_new, count, path, slots)

    def commit_path(self, k_new: torch.Tensor, v_new: torch.Tensor, path) -> None:
        """Host-state commit of a tree path: ``append`` of the chunk rows ``path`` ([a] shared or [B, a]; list or
        integer tensor, entries in [0, n), checked on the host) in that order."""
        self._refuse_per_seq("commit_path")
        n = k_new.shape[2]
        p = path if isinstance(path, torch.Tensor) else torch.tensor(path, dtype=torch.long)
        if p.dtype.is_floating_point or p.dtype.is_complex or p.dtype == torch.bool or p.dim() not in (1, 2) or \
                (p.dim() == 2 and p.shape[0] != k_new.shape[0]):
            raise ValueError(f"path must be an integer [a] or [B, a] index, got {tuple(p.shape)} {p.dtype}")
        h = p.detach().cpu().long()
        if h.numel() and bool(((h < 0) | (h >= n)).any()):
            raise ValueError(f"path entries must lie in [0, {n}): got {h.tolist()}")
        if h.shape[-1] == 0:
            return
        idx = h.to(k_new.device)
        if idx.dim() == 1:
            kk, vv = k_new.index_select(2, idx), v_new.index_select(2, idx)
        else:
            g = idx[:, None, :, None].expand(k_new.shape[0], k_new.shape[1], idx.shape[1], k_new.shape[3])
            kk, vv = k_new.gather(2, g), v_new.gather(2, g)
        self.append(kk, vv)

    # ------------------------------------------------ per-sequence state (ragged batches)
    _per_seq = False     # set by prefill_varlen / enable_device_state(per_sequence=True)

    def _refuse_per_seq(self, what):
        self._refuse_fp8(what)
        if self._per_seq:
            raise RuntimeError(f"{what}() works on the host-side state, which a cache in per-sequence mode "
                               "(prefill_varlen / enable_device_state(per_sequence=True)) does not keep: use "
                               "decode_step_dyn / extend_attention_dyn / extend_step_dyn / commit_dyn")

    def prefill_varlen(self, k: torch.Tensor, v: torch.Tensor, cu_seqlens) -> torch.Tensor:
        """Prefill a ragged batch: ``k`` / ``v`` ``[1, H_kv, T, D]`` hold n_seq packed sequences (sequence b = rows
        ``cu_seqlens[b] : cu_seqlens[b + 1]``, the layout ``sink_flash_attention_varlen`` takes).  Allocates
        ``[n_seq, H_kv, num_sink / window_size, D]`` buffers, stores every sequence with the placement a prefill of it
        alone gives (``sfa_ring_fill_varlen``, one launch) and enters per-sequence mode; returns the ``[n_seq, 4]``
        device state ``{sink_len, window_len, write_pos, seen}``.  ``cu_seqlens``: a device int32 tensor (not validated,
        no sync) or a host list / CPU tensor (checked here).  The prompt attention itself is the caller's
        ``sink_flash_attention_varlen`` call on the same pack."""
        from . import _native as N
        self._refuse_fp8("prefill_varlen")
        N.require_gpu(k, v)
        if self.window_size < 1:
            raise ValueError("prefill_varlen needs a ring of at least one slot (window_size >= 1)")
        if k.dim() != 4 or k.shape[0] != 1 or v.shape != k.shape:
            raise ValueError(f"k / v must be packed [1, H_kv, T, D] tensors of one shape, got {tuple(k.shape)} / "
                             f"{tuple(v.shape)}")
        if k.dtype not in N.SFA_DTYPE or v.dtype != k.dtype:
            raise TypeError("k / v must share one of the dtypes float32 / float16 / bfloat16")
        _one, H_kv, T, D = k.shape
        cu = self._cu_arg(cu_seqlens, T, k.device)
        n_seq = cu.numel() - 1
        mk = lambda n: torch.zeros(n_seq, H_kv, n, D, dtype=k.dtype, device=k.device)
        self.sink_k, self.sink_v = mk(self.num_sink), mk(self.num_sink)
        self.window_k, self.window_v = mk(self.window_size), mk(self.window_size)
        state = torch.empty(n_seq, 4, dtype=torch.int32, device=k.device)
        k, v = self._rows16(k), self._rows16(v)
        with torch.cuda.device(k.device):
            rc = N.lib().sfa_ring_fill_varlen(*(N.desc(t) for t in (self.sink_k, self.sink_v, self.window_k,
                                                                     self.window_v, k, v)),
                                              cu.data_ptr(), n_seq, state.data_ptr(), N.stream_ptr(k.device))
        N.check(rc, "sfa_ring_fill_varlen")
        self.sink_len = self.window_len = self.write_pos = self.seen_tokens = 0   # not kept in this mode
        self.is_initialized = self.prefilled = True
        self._per_seq = True
        self._dev_state = state
        return state

    @staticmethod
    def _cu_arg(cu_seqlens, T, device):
        """cu_seqlens as a device int32 tensor: a device tensor is taken as it is (no sync), a host list / CPU tensor is
        checked against the pack length T."""
        if isinstance(cu_seqlens, torch.Tensor) and cu_seqlens.is_cuda:
            if cu_seqlens.dtype.is_floating_point or cu_seqlens.dtype == torch.bool or cu_seqlens.dim() != 1:
                raise TypeError("cu_seqlens must be a 1-D integer tensor")
            cu = cu_seqlens.to(device=device, dtype=torch.int32).contiguous()
        else:
            lst = cu_seqlens.tolist() if isinstance(cu_seqlens, torch.Tensor) else [int(x) for x in cu_seqlens]
            if len(lst) < 2 or lst[0] != 0 or lst[-1] > T or any(b < a for a, b in zip(lst[:-1], lst[1:])):
                raise ValueError(f"bad cu_seqlens {lst} for T={T}: need 0 = c_0 <= c_1 <= ... <= T")
            cu = torch.tensor(lst, dtype=torch.int32, device=device)
        if cu.numel() < 2:
            raise ValueError("cu_seqlens needs at least two offsets")
        return cu

    def positions(self, slots=None) -> torch.Tensor:
        """Per-sequence mode: the ``seen`` column of the device state, ``[B]`` int32 (a view that follows the state, no
        sync): the position the next token of each sequence takes, for per-row RoPE positions built in torch ops.
        ``slots`` (list or integer tensor ``[B]``): ``seen`` of the named slots of a pool, gathered by torch indexing (no
        sync); inactive rows (-1) read 0."""
        st = self._require_dyn("positions")
        if not self._per_seq:
            raise RuntimeError("positions() needs per-sequence mode (prefill_varlen / enable_device_state(per_sequence="
                               "True)): the shared state holds no token count")
        if slots is None:
            return st[:, 3]
        idx = self._slots_arg(slots, None, writes=False).to(st.device).long()
        S = st.shape[0]
        ok = (idx >= 0) & (idx < S)
        return torch.where(ok, st[idx.clamp(0, S - 1), 3], torch.zeros_like(st[:1, 3]))

    # ------------------------------------------------ slot pool (continuous batching)
    _pool = False        # set by init_pool
    kv_scale = None      # FP8 pool: f32 [2, H_kv] on the device (row 0 K, row 1 V), allocated by init_pool

    @property
    def _kv8(self) -> bool:
        return self.window_k is not None and self.window_k.dtype == torch.float8_e4m3fn

    def _refuse_fp8(self, what):
        if self._kv8:
            raise TypeError(f"{what}() does not serve an FP8 (float8_e4m3fn) pool: use the packed calls prefill_slots / "
                            "ragged_step_dyn / commit_packed_dyn (and fork_slots, release_slots, positions, "
                            "packed_positions)")
        if self.page_size:       # a paged pool is served by the same calls as an FP8 pool
            raise TypeError(f"{what}() does not serve a paged pool (init_pool(page_size=...)): use the packed calls "
                            "prefill_slots / ragged_step_dyn / commit_packed_dyn (and fork_slots, release_slots, "
                            "positions, packed_positions)")

    # paged pool (init_pool(page_size=...)): window_k / window_v are the ring PAGES [num_pages, H_kv, P, D], page_table
    # the device int32 [S, Wc / P] map (entry [s][j]: the page of ring slots [j P, (j + 1) P) of slot s, -1 unmapped)
    page_size = None
    page_table = None
    _pages = None        # the host-side allocator behind reserve_pages / free_pages (shared by the layers of a cache)

    def _page_args(self):
        return (self.page_table.data_ptr(), self.page_table.stride(0))

    def _pool_entry(self, base, fp8, paged):
        """The entry point of a packed call on this pool: ``base`` on a 16-bit contiguous pool, else the form for an FP8
        pool, a paged pool, or - both - a paged FP8 pool (``init_pool(page_size=P, kv_dtype=torch.float8_e4m3fn)``)."""
        return fp8 + "_slots" if self._kv8 and not self.page_size else \
            paged + "_fp8_slots" if self._kv8 else paged + "_slots" if self.page_size else base

    def _pool_tail(self, n_slots=False):
        """What those forms take in front of the tail: (page_table, table_stride[, n_slots]) of a paged pool, then
        kv_scale of an FP8 pool."""
        pg = (*self._page_args(), *((self.num_slots,) if n_slots else ())) if self.page_size else ()
        return (*pg, *((self._kv_scale_ptr(),) if self._kv8 else ()))

    def reserve_pages(self, slots, tokens_after) -> None:
        """Map the ring pages the coming step needs (paged pool; pure host bookkeeping, no kernel, no device read):
        for each host slot the first ``ceil(min(tokens_after, window_size) / page_size)`` table entries are mapped from
        the free list; entries already mapped stay.  ``tokens_after`` (one number or one per slot) is an upper bound
        of the slot's ``seen`` after the step; ``seen`` counts the sink tokens too, so at most one page more than the ring
        reaches is reserved (``num_sink <= page_size``).  The changed
        entries are written into ``page_table`` with torch ops on the current stream.  Raises ``RuntimeError("out of
        pages: need X, free Y")`` before anything changes.

        A slot that shares pages (``fork_slots(share=True)``) first gets a page of its own for every shared page the step
        may store into (``PageAllocator``): the pairs are uploaded once and ``sfa_pages_copy`` runs on EVERY layer
        attached to the table, on the current stream, behind the table write and in front of the caller's step."""
        pages = self._require_paged("reserve_pages")
        _copy_pages(pages, pages.reserve(slots, tokens_after))

    def free_pages(self, slots) -> None:
        """Return the pages of the host ``slots`` to the free list and write -1 into their table rows (a retired
        sequence).  ``release_slots`` zeroes state rows and frees no pages; call both at retirement."""
        self._require_paged("free_pages").free(slots)

    def _require_paged(self, what):
        if self._pages is None:
            raise TypeError(f"{what} needs a paged pool: init_pool(..., page_size=P)")
        return self._pages

    def _act16(self, what, *tensors):
        """An FP8 pool takes bfloat16 / float16 activations of one dtype."""
        dt = tensors[0].dtype
        if dt not in (torch.bfloat16, torch.float16) or any(t.dtype != dt for t in tensors):
            raise TypeError(f"{what} of an FP8 pool must be bfloat16 or float16 tensors of one dtype, got "
                            f"{[str(t.dtype) for t in tensors]}")

    def _kv_scale_ptr(self):
        return None if self.kv_scale is None else self.kv_scale.data_ptr()

    def set_kv_scale(self, k_scale, v_scale) -> None:
        """Set the static per-KV-head scales of an FP8 pool: ``k_scale`` / ``v_scale`` hold H_kv values each (tensor, list
        or one number for every head) and are copied IN PLACE into ``kv_scale`` (f32 ``[2, H_kv]``, row 0 K, row 1 V; ones
        after ``init_pool``).  The kernels read the tensor when they run, never the host: with device tensors as sources
        the copy is capturable, and a captured step keeps the pointer, so a later in-place update is seen by the next
        replay.  Codes already in the pool are not rescaled: set the scales of a calibrated checkpoint before the first
        ``prefill_slots``, and keep equal scales on pools that exchange slots (``fork_slots`` copies bytes)."""
        if not (self._pool and self._kv8):
            raise TypeError("set_kv_scale needs an FP8 pool: init_pool(..., dtype=torch.float8_e4m3fn) or, paged, "
                            "init_pool(..., page_size=P, kv_dtype=torch.float8_e4m3fn)")
        for row, x in ((0, k_scale), (1, v_scale)):
            t = x if isinstance(x, torch.Tensor) else torch.tensor(x, dtype=torch.float32)
            if t.dim() > 1 or (t.dim() == 1 and t.numel() != self.kv_scale.shape[1]) or t.dtype.is_complex:
                raise ValueError(f"a scale must hold H_kv = {self.kv_scale.shape[1]} values (or one), got shape "
                                 f"{tuple(t.shape)}")
            self.kv_scale[row].copy_(t.to(torch.float32) if t.dim() else t.to(torch.float32).expand(self.kv_scale.shape[1]))

    def init_pool(self, num_slots: int, H_kv: int, D: int, dtype=torch.bfloat16, device="cuda", page_size=None,
                  num_pages=None, page_table=None, kv_dtype=None) -> torch.Tensor:
        """Allocate a pool of ``num_slots`` cache rows that lives as long as the server: ``[S, H_kv, num_sink /
        window_size, D]`` buffers and a zeroed int32 ``[S, 4]`` device state ``{sink_len, window_len, write_pos, seen}``
        (returned).  The layer enters per-sequence mode (the host-state methods refuse, as after ``prefill_varlen``).  A
        step then names the slots it works on with the ``slots=`` keyword of the dyn methods: a device int32 ``[B]``
        tensor (never read on the host, so a captured step replays at any occupancy by rewriting it in place), or a host
        list, which is checked for range and duplicates and uploaded.  Batch row b works on slot ``slots[b]``; -1 marks
        an inactive row.  A slot must be prefilled (``prefill_slots``) before it is used, or admitted by
        ``ragged_step_dyn(admit=True)``: to every other call an all-zero state row is not a prefilled cache.

        ``dtype=torch.float8_e4m3fn``: an FP8 pool - half the bytes per slot and per step.  The buffers hold OCP e4m3fn
        codes, ``kv_scale`` (f32 ``[2, H_kv]``, ones; ``set_kv_scale``) the static per-KV-head scales.  It is served by
        ``prefill_slots``, ``ragged_step_dyn``, ``commit_packed_dyn``, ``fork_slots``, ``release_slots``, ``positions``
        and ``packed_positions`` with bfloat16 / float16 activations; every other method raises ``TypeError``.  A stored
        element is ``e4m3fn(clamp(x / scale, -448, 448))`` and reads back as ``code * scale`` in the activations' dtype:
        the tokens of a step are attended at 16-bit precision inside that step and at FP8 precision afterwards, so a
        prompt admitted in chunks is not bitwise the prompt admitted in one call.

        ``page_size=P``: a PAGED pool - the ring memory follows the sequence lengths.  ``window_k`` / ``window_v`` are
        then ``[num_pages, H_kv, P, D]`` page buffers (default ``num_pages``: the full capacity ``S * Wc / P``; a server
        passes less) and ``page_table`` a device int32 ``[S, Wc / P]`` map, the given tensor or a new one filled with
        -1 (unmapped).  P is a power of two >= 32 that divides ``window_size`` (which need not be a power of two).  The
        kernels read the table when they run, so an in-place update is seen by the next replay of a captured graph.
        ``reserve_pages`` before a step and ``free_pages`` at retirement keep the table; a store to an unmapped page is
        dropped and a read of one is in bounds but unspecified.  Served by the calls of an FP8 pool, at bfloat16 /
        float16 and head dims 64 / 80 / 96 / 128; every other method raises ``TypeError``.  Sinks and state rows are not
        paged.  The defaults (``page_size=None``) give the contiguous pool.

        ``kv_dtype=torch.float8_e4m3fn`` (default None: the buffers have ``dtype``): the cache buffers hold FP8 codes and
        ``dtype`` (bfloat16 / float16) only names the activations the pool is meant for.  With ``page_size`` this is the
        PAGED FP8 pool - FP8 sinks ``[S, H_kv, num_sink, D]``, FP8 pages ``[num_pages, H_kv, P, D]``, ``kv_scale`` and
        ``page_table`` as above, every rule of the two pools unchanged, served by the same calls.  Without ``page_size``
        it is the contiguous FP8 pool of ``dtype=torch.float8_e4m3fn``.  (``dtype=torch.float8_e4m3fn`` together with
        ``page_size`` stays refused: the paged FP8 pool is spelled with ``kv_dtype``.)"""
        if kv_dtype is not None:
            if kv_dtype != torch.float8_e4m3fn:
                raise TypeError(f"kv_dtype must be None (the buffers have dtype) or torch.float8_e4m3fn, got {kv_dtype}")
            if dtype not in (torch.float16, torch.bfloat16):
                raise TypeError(f"with kv_dtype=float8_e4m3fn, dtype names the activations and must be bfloat16 or float16, "
                                f"got {dtype}")
        if page_size is None and (num_pages is not None or page_table is not None):
            raise ValueError("num_pages / page_table need page_size")
        if page_size is not None:
            P = int(page_size)
            if dtype == torch.float8_e4m3fn:
                raise TypeError("a paged FP8 pool is not served: init_pool takes dtype=float8_e4m3fn or page_size, not both "
                                "(the paged FP8 pool is dtype=bfloat16 / float16, page_size=P, kv_dtype=float8_e4m3fn)")
            if dtype not in (torch.float16, torch.bfloat16) or D not in (64, 80, 96, 128):
                raise ValueError(f"a paged pool serves bfloat16 / float16 at head dims 64 / 80 / 96 / 128, got {dtype}, D = {D}")
            if P < 32 or P & (P - 1):
                raise ValueError(f"page_size must be a power of two and at least 32, got {page_size}")
            if self.window_size < 1 or self.window_size % P:
                raise ValueError(f"window_size ({self.window_size}) must be a multiple of page_size ({P})")
            per_slot = self.window_size // P
            num_pages = int(num_slots) * per_slot if num_pages is None else int(num_pages)
            if num_pages < 1:
                raise ValueError(f"a paged pool needs at least one page, got num_pages = {num_pages}")
            if page_table is not None and (not isinstance(page_table, torch.Tensor) or page_table.dtype != torch.int32 or
                                           tuple(page_table.shape) != (int(num_slots), per_slot) or
                                           not page_table.is_contiguous()):
                raise ValueError(f"page_table must be a contiguous int32 [S, Wc / P] = [{int(num_slots)}, {per_slot}] tensor")
        # what export_slots gives back: the activations' dtype (an FP8 pool spelled dtype=float8_e4m3fn names none: bfloat16)
        self._act_dtype = torch.bfloat16 if dtype == torch.float8_e4m3fn else dtype
        if kv_dtype is not None:     # from here on `dtype` is what the buffers hold
            dtype = kv_dtype
        if self.window_size < 1:
            raise ValueError("init_pool needs a ring of at least one slot (window_size >= 1)")
        if int(num_slots) < 1:
            raise ValueError(f"init_pool needs at least one slot, got num_slots = {num_slots}")
        if dtype not in (torch.float32, torch.float16, torch.bfloat16, torch.float8_e4m3fn):
            raise TypeError("the pool's dtype must be float32 / float16 / bfloat16 / float8_e4m3fn")
        if dtype == torch.float8_e4m3fn and D not in (64, 80, 96, 128):
            raise ValueError(f"an FP8 pool serves head dims 64 / 80 / 96 / 128, got D = {D}")
        mk = lambda n: torch.zeros(int(num_slots), H_kv, n, D, dtype=dtype, device=device)
        self.sink_k, self.sink_v = mk(self.num_sink), mk(self.num_sink)
        self.page_size = self.page_table = self._pages = None
        if page_size is None:
            self.window_k, self.window_v = mk(self.window_size), mk(self.window_size)
        else:
            pg = lambda: torch.zeros(num_pages, H_kv, P, D, dtype=dtype, device=device)
            self.window_k, self.window_v = pg(), pg()
            self.page_size = P
            self.page_table = page_table if page_table is not None else \
                torch.full((int(num_slots), per_slot), -1, dtype=torch.int32, device=device)
            self._pages = PageAllocator(self.page_table, num_pages, P, self.window_size)
            self._pages.attach(self)
        # FP8 (OCP e4m3fn, one byte per element): the pool holds codes, the activations of the packed calls stay 16-bit;
        # the caller-owned static scales start at one (set_kv_scale)
        self.kv_scale = torch.ones(2, H_kv, dtype=torch.float32, device=device) if dtype == torch.float8_e4m3fn else None
        self._dev_state = torch.zeros(int(num_slots), 4, dtype=torch.int32, device=device)
        self.sink_len = self.window_len = self.write_pos = self.seen_tokens = 0   # not kept in this mode
        self.is_initialized = self.prefilled = True
        self._per_seq = self._pool = True
        return self._dev_state

    @property
    def num_slots(self) -> int:
        """Rows of the cache buffers (the S of a pool)."""
        return 0 if self.sink_k is None else self.sink_k.shape[0]

    def _slots_arg(self, slots, B, writes):
        """``slots=`` of a dyn call as a contiguous int32 tensor on the cache's device (None stays None).  A device tensor
        is passed through unread.  A host list / CPU tensor is checked: B entries, each -1 or in [0, S), and - for a call
        that stores or advances (``writes``) - no slot twice."""
        if slots is None:
            return None
        if not self._per_seq:
            raise RuntimeError("slots= needs per-sequence state rows: init_pool (or prefill_varlen / "
                               "enable_device_state(per_sequence=True))")
        S = self.num_slots
        if isinstance(slots, torch.Tensor) and slots.is_cuda:
            if slots.dtype.is_floating_point or slots.dtype == torch.bool or slots.dim() != 1:
                raise TypeError("slots must be a 1-D integer tensor")
            if B is not None and slots.numel() != B:
                raise ValueError(f"slots must hold B = {B} entries (one per batch row), got {slots.numel()}")
            return slots.to(dtype=torch.int32).contiguous()     # an int32 contiguous tensor is passed as it is
        lst = slots.tolist() if isinstance(slots, torch.Tensor) else [int(x) for x in slots]
        if B is not None and len(lst) != B:
            raise ValueError(f"slots must hold B = {B} entries (one per batch row), got {len(lst)}")
        bad = [x for x in lst if x != -1 and not 0 <= x < S]
        if bad:
            raise ValueError(f"slots {bad} outside the pool of {S} slots (use -1 for an inactive row)")
        live = [x for x in lst if x >= 0]
        if writes and len(set(live)) != len(live):
            raise ValueError(f"slots {lst}: a slot is named twice in a call that stores or advances")
        return torch.tensor(lst, dtype=torch.int32, device=self.window_k.device)

    def prefill_slots(self, k: torch.Tensor, v: torch.Tensor, cu_seqlens, slots) -> torch.Tensor:
        """Admit requests into a pool: ``k`` / ``v`` ``[1, H_kv, T, D]`` hold packed sequences as for ``prefill_varlen``;
        sequence i is stored into slot ``slots[i]`` with the placement a prefill of it alone gives and writes that state
        row (``sfa_ring_fill_varlen_slots``, one launch, no allocation).  Every other slot keeps buffers and state, so
        this runs while the other sequences keep decoding, and it is how a released slot is reused.  Returns the pool's
        state."""
        from . import _native as N
        if not (self._per_seq and self.is_initialized):
            raise RuntimeError("prefill_slots needs a pool: call init_pool first")
        if k.dim() != 4 or k.shape[0] != 1 or v.shape != k.shape:
            raise ValueError(f"k / v must be packed [1, H_kv, T, D] tensors of one shape, got {tuple(k.shape)} / "
                             f"{tuple(v.shape)}")
        n_seq = (cu_seqlens.numel() if isinstance(cu_seqlens, torch.Tensor) else len(cu_seqlens)) - 1
        slots = self._slots_arg(slots, n_seq, writes=True)
        N.require_gpu(k, v, self.window_k, slots)
        if self._kv8:
            self._act16("k / v", k, v)
        elif k.dtype != self.window_k.dtype or v.dtype != k.dtype:
            raise TypeError("k / v must have the pool's dtype")
        if k.shape[1] != self.window_k.shape[1] or k.shape[3] != self.window_k.shape[3]:
            raise ValueError(f"k / v must be [1, H_kv, T, D] = [1, {self.window_k.shape[1]}, T, {self.window_k.shape[3]}], "
                             f"got {tuple(k.shape)}")
        cu = self._cu_arg(cu_seqlens, k.shape[2], k.device)
        k, v = self._rows16(k), self._rows16(v)
        name = self._pool_entry("sfa_ring_fill_varlen_slots", "sfa_ring_fill_varlen_fp8", "sfa_ring_fill_varlen_paged")
        with torch.cuda.device(k.device):
            rc = getattr(N.lib(), name)(*(N.desc(t) for t in (self.sink_k, self.sink_v, self.window_k, self.window_v, k, v)),
                                        cu.data_ptr(), n_seq, self._dev_state.data_ptr(), slots.data_ptr(),
                                        *self._pool_tail(), N.stream_ptr(k.device))
        N.check(rc, name)
        return self._dev_state

    def release_slots(self, slots) -> None:
        """Retire sequences: zero the state rows of ``slots`` (list or integer tensor; -1 entries name nothing) with torch
        ops on the current stream (no sync, capturable).  The buffers keep their stale content, which no kernel reads
        beyond a row's ``sink_len`` / ``window_len``.  A released slot must be prefilled again (``prefill_slots``), or
        admitted by ``ragged_step_dyn(admit=True)``, before it is used: an all-zero state is not a prefilled cache."""
        st = self._require_dyn("release_slots")
        idx = self._slots_arg(slots, None, writes=False).to(st.device)
        hit = (torch.arange(st.shape[0], device=st.device, dtype=torch.int32)[:, None] == idx[None, :]).any(dim=1)
        st.mul_((~hit).to(torch.int32)[:, None])

    def fork_slots(self, src, dst, source: Optional["SinkCacheLayer"] = None, share: bool = False, tokens=None) -> None:
        """``share=True`` (paged pool, within one pool): the fork SHARES the source's ring pages instead of copying them.
        ``PageAllocator.share`` writes the source's table row into the destination's row (every page gains a reference),
        ``sfa_ring_share_paged_slots`` copies the live sink rows and the state row, and no ring byte moves: time and
        memory of the fork do not grow with the prompt.  Every later call on ``dst[i]`` still gives bitwise what it gives
        after a copying fork, because ``reserve_pages`` hands a slot a private copy of a shared page before a step stores
        into it (copy on first write).  ``tokens`` is required: the exact ``seen`` of each source (one int or one per
        pair), from which the ring's fill ``max(tokens - num_sink, 0)`` is passed on.  ``src`` / ``dst`` must be host
        lists or CPU tensors, every pair two distinct slots of the pool (no -1), and ``dst[i]`` must map no page
        (``free_pages`` first): the table is host bookkeeping, so the call is not capturable.  ``source`` must be None or
        this layer.  A slot that is re-admitted after ``release_slots`` needs ``free_pages`` in between, or the allocator
        keeps the count of its last share.  On a layer whose table serves several layers use
        ``SinkAttentionCache.fork_slots(share=True)``: the table is aliased once, not once per layer.

        ``share=False`` (the default), every pool: copy slots on the device (``sfa_ring_copy_slots``, one launch, no allocation, capturable): pair i copies slot
        ``src[i]`` of ``source``'s pool (another pooled layer of equal geometry, dtype and device; default: this layer,
        a fork) into slot ``dst[i]`` of this layer's pool.  The live sink rows, the live ring slots (each at its
        position) and the state row are copied, so any later call on ``dst[i]`` gives bitwise what the same call on
        ``src[i]`` gives; rows the source does not reach keep what the destination held.  One source may feed many
        destinations: parallel sampling is ``fork_slots([p] * (n - 1), free[:n - 1])``.  A pair with a -1 (or any value
        outside its pool) on either side, or with ``src[i] == dst[i]`` in one pool, moves nothing, so a captured call
        replays with any number of live pairs.  Undefined: a destination named twice, and in one pool a destination that
        is also a live source - a beam step forks into free slots and releases dead ones (``beam_fork_plan``) instead
        of permuting in place.  ``src`` / ``dst``: device int32 ``[n]`` tensors, passed through unread, or host lists /
        CPU tensors, which are checked (equal lengths, range, the two undefined cases) and uploaded."""
        from . import _native as N
        if share:
            pages = self._require_paged("fork_slots(share=True)")
            if len(pages.layers) > 1:
                raise ValueError(f"fork_slots(share=True): this layer's page table serves {len(pages.layers)} layers and is "
                                 f"aliased once, not once per layer: call SinkAttentionCache.fork_slots(share=True)")
            src_l, dst_l, ring, src_t, dst_t = self._share_args(src, dst, source, tokens)
            N.require_gpu(self.sink_k)
            pages.share(src_l, dst_l, ring)
            return self._share_call(src_t, dst_t)
        if tokens is not None:
            raise ValueError("fork_slots: tokens belongs to share=True")
        source = self if source is None else source
        if not isinstance(source, SinkCacheLayer):
            raise TypeError("fork_slots: source must be a SinkCacheLayer")
        dst_state, src_state = self._require_pool("fork_slots"), source._require_pool("fork_slots")
        if source is not self:
            if source.window_k.dtype != self.window_k.dtype:
                raise TypeError(f"fork_slots: the pools differ in dtype ({source.window_k.dtype} / {self.window_k.dtype})")
            if source.window_k.shape[1:] != self.window_k.shape[1:] or source.sink_k.shape[1:] != self.sink_k.shape[1:]:
                raise ValueError(f"fork_slots: the pools differ in geometry: source [S, H_kv, num_sink / Wc, D] = "
                                 f"{tuple(source.sink_k.shape)} / {tuple(source.window_k.shape)}, this layer "
                                 f"{tuple(self.sink_k.shape)} / {tuple(self.window_k.shape)}")
            if source.page_size != self.page_size or source.window_size != self.window_size:
                raise ValueError(f"fork_slots: the pools differ in paging: source page_size {source.page_size} of a ring "
                                 f"of {source.window_size}, this layer {self.page_size} of {self.window_size}")
            if source.window_k.device != self.window_k.device:
                raise ValueError("fork_slots: the pools must live on one device")
        src, dst = self._fork_args(src, dst, source)
        N.require_gpu(self.window_k, source.window_k, src, dst)
        if src.numel() == 0:
            return
        name = "sfa_ring_copy_paged_slots" if self.page_size else "sfa_ring_copy_slots"
        with torch.cuda.device(self.window_k.device):
            rc = getattr(N.lib(), name)(
                *(N.desc(t) for t in (source.sink_k, source.sink_v, source.window_k, source.window_v)),
                src_state.data_ptr(),
                *(N.desc(t) for t in (self.sink_k, self.sink_v, self.window_k, self.window_v)), dst_state.data_ptr(),
                src.data_ptr(), dst.data_ptr(), src.numel(),
                *((*source._page_args(), *self._page_args()) if self.page_size else ()), N.stream_ptr(self.window_k.device))
        N.check(rc, name)

    def _fork_args(self, src, dst, source):
        """``src`` / ``dst`` of ``fork_slots`` as int32 tensors on the pool's device: ``_slots_arg`` for each (``src``
        against ``source``'s pool, ``dst`` against this one), equal lengths, and - where both are host lists - the two
        cases the kernel leaves undefined.  A pair is live when both entries name a slot and it is not ``s == d`` in one
        pool."""
        host = [None if isinstance(x, torch.Tensor) and x.is_cuda else
                (x.tolist() if isinstance(x, torch.Tensor) else [int(v) for v in x]) for x in (src, dst)]
        n = [x.numel() if h is None else len(h) for x, h in ((src, host[0]), (dst, host[1]))]
        if n[0] != n[1]:
            raise ValueError(f"fork_slots: src and dst must pair up, got {n[0]} and {n[1]} entries")
        src_t, dst_t = source._slots_arg(src, None, writes=False), self._slots_arg(dst, None, writes=False)
        if host[0] is not None and host[1] is not None:
            live = [(s, d) for s, d in zip(*host) if s >= 0 and d >= 0 and not (source is self and s == d)]
            dsts = [d for _, d in live]
            if len(set(dsts)) != len(dsts):
                raise ValueError(f"fork_slots: dst {host[1]} names a destination twice")
            if source is self:
                both = sorted(set(dsts) & {s for s, _ in live})
                if both:
                    raise ValueError(f"fork_slots: slots {both} are a destination and the source of another pair in one "
                                     f"call; fork into free slots (beam_fork_plan)")
        return src_t.to(self.window_k.device), dst_t.to(self.window_k.device)

    def _share_args(self, src, dst, source, tokens):
        """The arguments of ``fork_slots(share=True)`` checked on the host: (src list, dst list, the ring fill of each
        source, src / dst as device int32 tensors)."""
        self._require_pool("fork_slots")
        self._require_paged("fork_slots(share=True)")
        if source is not None and source is not self:
            raise ValueError("fork_slots(share=True): pages are shared within one page buffer: source must be None or the "
                             "object itself (between two pools use share=False)")
        if any(isinstance(x, torch.Tensor) and x.is_cuda for x in (src, dst)):
            raise TypeError("fork_slots(share=True): src / dst must be host lists or CPU tensors: the page table is host "
                            "bookkeeping, so the call is not capturable")
        src_l, dst_l = ([int(v) for v in (x.tolist() if isinstance(x, torch.Tensor) else x)] for x in (src, dst))
        if len(src_l) != len(dst_l):
            raise ValueError(f"fork_slots: src and dst must pair up, got {len(src_l)} and {len(dst_l)} entries")
        S = self.num_slots
        bad = [(s, d) for s, d in zip(src_l, dst_l) if not (0 <= s < S and 0 <= d < S) or s == d]
        if bad:
            raise ValueError(f"fork_slots(share=True): pairs {bad}: each must name two distinct slots of the pool of {S} "
                             f"(no -1: a shared fork is not replayed)")
        if tokens is None:
            raise ValueError("fork_slots(share=True) needs tokens=: the exact seen of each source (one int or one per "
                             "pair), which bounds the pages a later step may store into")
        tok = [tokens] * len(src_l) if isinstance(tokens, int) else \
            [int(t) for t in (tokens.tolist() if isinstance(tokens, torch.Tensor) else tokens)]
        if len(tok) != len(src_l):
            raise ValueError(f"fork_slots(share=True): tokens must be one number or one per pair ({len(src_l)}), got "
                             f"{len(tok)}")
        src_t, dst_t = self._fork_args(src_l, dst_l, self)      # a destination twice, a destination that is a source
        return src_l, dst_l, [max(t - self.num_sink, 0) for t in tok], src_t, dst_t

    def _share_call(self, src_t, dst_t) -> None:
        """``sfa_ring_share_paged_slots`` on this layer: sinks and state rows of the pairs, no ring memory."""
        from . import _native as N
        N.require_gpu(self.sink_k, src_t, dst_t)
        if src_t.numel() == 0:
            return
        st = self._dev_state
        with torch.cuda.device(self.sink_k.device):
            rc = N.lib().sfa_ring_share_paged_slots(N.desc(self.sink_k), N.desc(self.sink_v), st.data_ptr(),
                                                    N.desc(self.sink_k), N.desc(self.sink_v), st.data_ptr(),
                                                    src_t.data_ptr(), dst_t.data_ptr(), src_t.numel(),
                                                    N.stream_ptr(self.sink_k.device))
        N.check(rc, "sfa_ring_share_paged_slots")

    def _pages_copy(self, src_pages, dst_pages) -> None:
        """``sfa_pages_copy`` on this layer's page buffers (device int32 page ids, pair i: src -> dst)."""
        from . import _native as N
        N.require_gpu(self.window_k, src_pages, dst_pages)
        wk, wv = self._ring_descs()
        with torch.cuda.device(self.window_k.device):
            rc = N.lib().sfa_pages_copy(wk, wv, src_pages.data_ptr(), dst_pages.data_ptr(), src_pages.numel(),
                                        N.stream_ptr(self.window_k.device))
        N.check(rc, "sfa_pages_copy")

    # ------------------------------------------------ export / import (the way out of a pool, and back in)
    _act_dtype = None    # set by init_pool: the dtype of the packs an FP8 pool exports

    def live_lengths(self, slots) -> torch.Tensor:
        """Tokens each named slot of a pool holds: ``clamp(sink_len) + clamp(window_len)`` of its state row, ``[n]`` int32;
        0 for a -1 entry and for a fresh (released) slot.  Torch ops on the device state (no sync, capturable), in the
        manner of ``positions``: what ``export_slots`` writes per sequence, and the lengths its offsets are built from."""
        st = self._require_pool("live_lengths")
        if slots is None:
            raise TypeError("live_lengths: slots must name the slots (list or integer tensor)")
        idx = self._slots_arg(slots, None, writes=False).to(st.device).long()
        S = st.shape[0]
        ok = (idx >= 0) & (idx < S)
        row = st[idx.clamp(0, S - 1)]
        live = row[:, 0].clamp(0, self.num_sink) + row[:, 1].clamp(0, self.window_size)
        return torch.where(ok, live, torch.zeros_like(live))

    def export_slots(self, slots, cu=None, T=None, out=None, return_positions: bool = False):
        """Read slots of a pool out as packed K/V in TOKEN order - the inverse of ``prefill_slots``
        (``sfa_ring_export_slots``, one launch, nothing of the pool is written).  Sequence i is slot ``slots[i]`` and owns
        rows ``cu[i] : cu[i + 1]`` of ``k`` / ``v`` ``[1, H_kv, T, D]``: its sink rows, then its ring from the oldest
        token to the newest, whatever ``write_pos`` is, through the page table of a paged pool and dequantised
        (``code * kv_scale``, the packed step's own read) into the ``dtype`` given to ``init_pool`` on an FP8 pool.  A
        sequence with fewer rows than live tokens is truncated (its FIRST rows are written); every other row of the pack
        - behind a sequence's live tokens, of a -1 slot, behind ``cu[-1]`` - is zero.  A ring slot whose page is unmapped
        exports zeros.  Returns ``(k, v, cu)`` with ``cu`` the device int32 offsets, or ``(k, v, cu, pos)`` with
        ``return_positions=True``: ``pos`` ``[T]`` int32, the position of each token (what RoPE took; -1 on zeroed rows).

        ``cu=None`` is the convenient form: the offsets are the cumulative sum of ``live_lengths(slots)`` (on the
        device), and unless ``T`` or ``out`` gives it the total is read back ONCE to size the pack - not capturable.
        With ``cu`` (a device int32 tensor, unread; or a host list, checked) and ``T`` or ``out``, nothing is read on the
        host and the call is capturable.  ``out = (k, v)`` or ``(k, v, pos)``: the pack to write into (``T`` is its row
        count; any strides with 16-byte aligned rows, e.g. a ``[1, T, H_kv, D]``-stored view).  ``slots`` as for the dyn
        calls (a device tensor is passed through unread, a host list is checked); a slot may be named twice."""
        from . import _native as N
        st = self._require_pool("export_slots")
        if slots is None:
            raise TypeError("export_slots: slots must name the slots (list or integer tensor)")
        slots = self._slots_arg(slots, None, writes=False)
        n_seq = slots.numel()
        if n_seq < 1:
            raise ValueError("export_slots needs at least one slot")
        dev = self.sink_k.device
        _S, H_kv, _ns, D = self.sink_k.shape
        dt = self._act_dtype if self._kv8 else self.window_k.dtype
        pos = None
        if out is not None:
            if not isinstance(out, (tuple, list)) or len(out) not in (2, 3) or not all(isinstance(t, torch.Tensor) for t in out):
                raise TypeError("export_slots: out must be (k, v) or (k, v, pos) tensors")
            k, v = out[0], out[1]
            pos = out[2] if len(out) == 3 else None
            if self._kv8:
                self._act16("out of export_slots", k, v)
            elif k.dtype != dt or v.dtype != dt:
                raise TypeError(f"export_slots: out must have the pool's dtype {dt}, got {k.dtype} / {v.dtype}")
            if k.dim() != 4 or k.shape[0] != 1 or k.shape[1] != H_kv or k.shape[3] != D or v.shape != k.shape:
                raise ValueError(f"export_slots: out must be packed [1, H_kv, T, D] = [1, {H_kv}, T, {D}] tensors of one "
                                 f"shape, got {tuple(k.shape)} / {tuple(v.shape)}")
            if T is not None and int(T) != k.shape[2]:
                raise ValueError(f"export_slots: T = {T} but out holds {k.shape[2]} rows")
            T = k.shape[2]
            for t in (k, v):     # an output cannot be copied into shape as _rows16 does for an input
                if t.numel() and (t.stride(3) != 1 or t.data_ptr() % 16 or
                                  any((t.stride(i) * t.element_size()) % 16 for i in range(3))):
                    raise ValueError("export_slots: the rows of out must be 16-byte aligned with a unit last stride")
            if pos is not None and (pos.dtype != torch.int32 or pos.dim() != 1 or pos.numel() != T or not pos.is_contiguous()):
                raise ValueError(f"export_slots: pos of out must be a contiguous int32 [T] = [{T}] tensor")
        if cu is None:
            live = self.live_lengths(slots)
            cu_t = torch.zeros(n_seq + 1, dtype=torch.int32, device=live.device)
            cu_t[1:] = torch.cumsum(live, 0)
            if T is None:
                T = int(cu_t[-1].item())         # the one read-back of the convenient form
        else:
            if isinstance(cu, torch.Tensor) and cu.is_cuda:
                if T is None:
                    raise ValueError("export_slots: a device cu needs T or out: the size of the pack is not read back from "
                                     "the device")
            elif T is None:
                T = int(cu[-1])
            cu_t = self._cu_arg(cu, int(T), dev)
            if cu_t.numel() != n_seq + 1:
                raise ValueError(f"export_slots: cu must hold n + 1 = {n_seq + 1} offsets for {n_seq} slots, got "
                                 f"{cu_t.numel()}")
        T = int(T)
        if T < 0:
            raise ValueError(f"export_slots: T must be >= 0, got {T}")
        N.require_gpu(self.window_k, slots, cu_t)
        if out is None:
            k = torch.empty(1, H_kv, T, D, dtype=dt, device=dev)      # every row is written by the kernel
            v = torch.empty_like(k)
        N.require_gpu(k, v, pos)
        if pos is None and return_positions:
            pos = torch.empty(T, dtype=torch.int32, device=dev)
        if T > 0:
            name = self._pool_entry("sfa_ring_export_slots", "sfa_ring_export_fp8", "sfa_ring_export_paged")
            with torch.cuda.device(dev):
                rc = getattr(N.lib(), name)(*(N.desc(t) for t in (self.sink_k, self.sink_v, self.window_k, self.window_v,
                                                                  k, v)),
                                            cu_t.data_ptr(), n_seq, st.data_ptr(), slots.data_ptr(),
                                            None if pos is None else pos.data_ptr(), *self._pool_tail(),
                                            N.stream_ptr(dev))
            N.check(rc, name)
        return (k, v, cu_t, pos) if return_positions else (k, v, cu_t)

    def import_slots(self, k: torch.Tensor, v: torch.Tensor, cu, slots, seen=None) -> torch.Tensor:
        """Admit exported sequences: ``prefill_slots(k, v, cu, slots)``, then - with ``seen`` (device int32 ``[n]`` or a
        host list: the source's ``positions(slots)``) - column 3 of the named state rows is overwritten by a torch
        scatter on the current stream (-1 slots are skipped; no sync).  That is what lets a sequence that has already
        evicted tokens (``seen > num_sink + Wc``) resume at the right RoPE position: the mask depends on ``sink_len``,
        ``window_len`` and ``write_pos`` only, ``seen`` is the position counter.  Returns the pool's state.

        - The imported ring is rotated to ``write_pos = 0`` when it is full (the prefill placement), so later steps read
          the same tokens in another physical order: their outputs are within tolerance of the source's, not bitwise
          equal to them.  A second export is bitwise the first.
        - Importing into a smaller ``Wc`` keeps the sinks and the newest ``Wc`` tokens - the cache policy itself.
        - Importing an evicted sequence into a larger ``Wc`` cannot bring back what was evicted: the ring holds what the
          pack held and grows from there.
        A pack exported with zero tails (``m_i > live``) must be imported with the offsets of the live tokens
        (``export_slots`` with ``cu=None`` gives exactly those), or the zero rows are admitted as tokens.  A slot that was
        admitted by a first chunk shorter than ``num_sink`` (``sink_len < num_sink`` under a non-empty ring) arrives with
        its first ``num_sink`` tokens as sinks.  On a paged pool ``reserve_pages(slots, seen)`` comes first, as before
        ``prefill_slots``."""
        st = self._require_pool("import_slots")
        if not isinstance(k, torch.Tensor) or not isinstance(v, torch.Tensor):
            raise TypeError("import_slots: k / v must be tensors")
        if self._kv8:
            self._act16("k / v", k, v)
        elif k.dtype != self.window_k.dtype or v.dtype != k.dtype:
            raise TypeError("k / v must have the pool's dtype")
        n_seq = (cu.numel() if isinstance(cu, torch.Tensor) else len(cu)) - 1
        seen_t = self._packed_i32(seen, n_seq, "seen", "n", st.device)
        idx = self._slots_arg(slots, n_seq, writes=True)
        self.prefill_slots(k, v, cu, idx)
        if seen_t is not None:
            S = st.shape[0]
            idx = idx.to(st.device).long()
            ok = (idx >= 0) & (idx < S)
            # rows of skipped entries go to a scratch row S behind the state, so that the scatter stays branch-free
            col = torch.cat([st[:, 3], st.new_zeros(1)])
            col.scatter_(0, torch.where(ok, idx, torch.full_like(idx, S)), seen_t)
            st[:, 3] = col[:S]
        return st

    def _require_dyn(self, what):
        if not (self.is_initialized and self.prefilled):
            raise ValueError(f"{what} needs a prefilled cache: the first chunk is a prefill (sink_flash_attention)")
        st = getattr(self, "_dev_state", None)
        if st is None:
            raise RuntimeError(f"{what} needs the state on the device: call enable_device_state() first")
        return st

    _rows16 = staticmethod(rows16)

    def _ring_descs(self):
        key = (self.window_k.data_ptr(), self.window_v.data_ptr())
        rd = getattr(self, "_ring_desc", None)
        if rd is None or rd[0] != key:
            from . import _native as N
            rd = (key, (N.desc(self.window_k), N.desc(self.window_v)))
            self._ring_desc = rd
        return rd[1]

    def _ring_multi_dyn(self, q, k_new, v_new, s_aux, out, commit, tree=None, slots=None):
        """sfa_decode_ring_multi_dyn with the per-layer constants (buffer descriptors, a workspace for the full cache plus
        the chunk) built once per chunk shape, as _ring_multi does."""
        from . import _native as N
        self._refuse_fp8("extend_attention_tree_dyn" if tree is not None else
                         "extend_step_dyn" if commit else "extend_attention_dyn")
        slots = self._slots_arg(slots, q.shape[0], writes=bool(commit))
        dev_state = self._require_dyn("extend_attention_tree_dyn" if tree is not None else
                                      "extend_step_dyn" if commit else "extend_attention_dyn")
        N.require_gpu(q, k_new, v_new, s_aux, out, self.window_k, slots)
        B, H_q, n, D = q.shape
        H_kv = self.sink_k.shape[1]
        self._check_chunk(N, q, k_new, v_new, out, "[B, H_kv, n, D]")
        st = getattr(self, "_multi_dyn_state", None)
        key = (self.sink_k.data_ptr(), self.window_k.data_ptr(), q.shape, q.dtype)
        if st is None or st["key"] != key:
            ws_bytes = N.lib().sfa_decode_multi_workspace_bytes(B, H_q, H_kv, n, self.num_sink + self.window_size + n, D,
                                                                N.SFA_DTYPE[q.dtype])
            if ws_bytes == 0:
                raise ValueError(f"D={D}: a K/V row must be a multiple of 16 bytes, <= 1 KiB")
            st = self._call_consts("_multi_dyn_state", key, ws_bytes, False, q)
        q, k_new, v_new = self._rows16(q), self._rows16(k_new), self._rows16(v_new)
        s_aux_f, aux = self._aux(s_aux)
        if out is None:
            out = torch.empty((B, H_q, n, D), device=q.device, dtype=q.dtype)
        sk, sv, wk, wv = st["descs"]
        mode = "_slots" if slots is not None else "_rows" if self._per_seq else "_dyn"
        if tree is not None:
            name, mid = "sfa_decode_ring_tree" + mode, (tree[0].data_ptr(), tree[1])
        else:
            name, mid = "sfa_decode_ring_multi" + mode, (1 if commit else 0,)
        with torch.cuda.device(q.device):
            rc = getattr(st["lib"], name)(N.desc(q), sk, sv, wk, wv, N.desc(k_new), N.desc(v_new), N.desc(out), aux,
                                          *mid, dev_state.data_ptr(), *(() if slots is None else (slots.data_ptr(),)),
                                          st["ws"].data_ptr(), st["ws"].numel(), st["scale"], 0, N.stream_ptr(q.device))
        N.check(rc, name)
        return out

    # ------------------------------------------------ packed ragged step (chunked prefill + decode in one call)
    def _require_pool(self, what):
        if not (self._pool and self.is_initialized):
            raise RuntimeError(f"{what} needs a pool: call init_pool first")
        return self._dev_state

    def ragged_step_dyn(self, q: torch.Tensor, k_new: torch.Tensor, v_new: torch.Tensor, cu_q, slots,
                        s_aux: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                        commit: bool = True, admit: bool = False, parent=None, commit_seq=None,
                        groups=None) -> torch.Tensor:
        """One step over the pool in which every sequence brings its own number of new tokens
        (``sfa_decode_ring_ragged_slots``): ``q`` ``[1, H_q, T, D]`` and ``k_new`` / ``v_new`` ``[1, H_kv, T, D]`` hold
        the new tokens of n_seq sequences back to back (the layout ``prefill_slots`` takes); sequence i is rows
        ``cu_q[i] : cu_q[i + 1]`` and works on slot ``slots[i]``.  Decode rows (1 token), draft rows (k tokens) and the
        next chunk of a long prompt (hundreds) run in one call whose cost follows T.  Each sequence is attended as
        ``extend_attention_dyn`` of its own chunk at its slot's state; with ``commit`` its tokens are stored and its
        state row advances by its length (``extend_step_dyn``).  Rows of an inactive sequence (slot -1), and rows behind
        ``cu_q[-1]`` (padding of a step captured at a fixed T) come back as zeros and change nothing.  ``cu_q`` and
        ``slots``: device int32 tensors (never read on the host: the call is graph-capturable and a captured step replays
        at any mix of lengths by rewriting them in place) or host lists, which are checked.

        ``admit=False``: the call continues sequences that ``prefill_slots`` has admitted (``sink_len`` never changes).
        ``admit=True`` (``SFA_FLAG_RAGGED_ADMIT``): a sequence whose slot is fresh - its state row has ``seen == 0``, as
        after ``init_pool`` or ``release_slots``, read on the device - is admitted by this call: it attends to its own
        chunk alone with the mask of a prefill (the first ``min(n_i, num_sink)`` tokens stay visible behind the window;
        ``n_i > window_size + num_sink`` is fine), and with ``commit`` its tokens and state row end bitwise as
        ``prefill_slots`` of the chunk leaves them.  Every other sequence of the pack is bit for bit what it is with
        ``admit=False``, so one captured step serves admission, chunked prefill, decode and draft rows:
        ``release_slots``, ``packed_positions``, then this call.  A first chunk shorter than ``num_sink`` pins only its
        own tokens as sinks (later tokens go to the ring, as ``append`` after a short prompt does): a scheduler should
        give an admitting chunk at least ``min(prompt, num_sink)`` tokens.

        ``parent`` / ``commit_seq`` (``sfa_decode_ring_ragged_tree_slots``; both None: the call above, unchanged).
        ``parent`` ``[T]``, packed like ``q``: ``parent[cu_q[i] + u]`` is the parent of node u of sequence i as a local
        index in [-1, u), anything else reads as -1.  A sequence of at most 64 tokens that is not admitting is then a draft
        tree, attended as ``extend_attention_tree_dyn(slots=)`` of its chunk; longer and admitting sequences ignore their
        entries.  Write ``u - 1`` for chains (decode rows, short chunks, chain drafts).  ``commit_seq`` ``[n_seq]``:
        with ``commit``, sequence i is stored and advanced iff ``commit_seq[i] != 0`` - 1 for decode rows and prompt
        chunks, 0 for draft rows, whose accepted prefix ``commit_packed_dyn`` stores afterwards.  Device int32 tensors are
        taken as they are and never read on the host; host lists are checked for their length (T, n_seq).

        ``groups`` (``sfa_decode_ring_ragged_group_paged_slots``; None: the call above, unchanged; paged pools only):
        offsets ``cu_g`` ``[n_grp + 1]`` over the SEQUENCES of the pack (``group_offsets`` builds them from group ids) -
        group g is the consecutive sequences ``cu_g[g] : cu_g[g + 1]``, forks of one prompt made with
        ``fork_slots(share=True)``.  The ring slots that the members of a group share (the same pages in their table rows,
        unwrapped, decided on the device) are read once per group instead of once per member; the output is that of the
        ungrouped call within its tolerance, pool and state rows end bitwise as it leaves them, and a group that shares
        nothing is computed exactly as without ``groups``.  The caller promises nothing: any grouping is safe.  A device
        int32 tensor is never read on the host (a captured step replays at any grouping by rewriting it in place), a host
        list is checked and uploaded once.  ``parent`` together with ``groups`` is refused."""
        from . import _native as N
        dev_state = self._require_pool("ragged_step_dyn")
        if groups is not None:
            if not self.page_size:
                raise TypeError("ragged_step_dyn(groups=) needs a paged pool: init_pool(..., page_size=P)")
            if parent is not None:
                raise ValueError("ragged_step_dyn(groups=) takes no parent=: draft trees inside a group are not served")
        N.require_gpu(q, k_new, v_new, s_aux, out, self.window_k)
        if q.dim() != 4 or q.shape[0] != 1:
            raise ValueError(f"q must be a packed [1, H_q, T, D] tensor, got {tuple(q.shape)}")
        _one, H_q, T, D = q.shape
        H_kv = self.sink_k.shape[1]
        self._check_chunk(N, q, k_new, v_new, out, "[1, H_kv, T, D]")
        cu = self._cu_arg(cu_q, T, q.device)
        n_seq = cu.numel() - 1
        slots = self._slots_arg(slots, n_seq, writes=bool(commit))
        N.require_gpu(slots)
        parent = self._packed_i32(parent, T, "parent", "T", q.device)
        commit_seq = self._packed_i32(commit_seq, n_seq, "commit_seq", "n_seq", q.device)
        cu_g = None if groups is None else self._group_arg(groups, n_seq, q.device)
        n_grp = 0 if cu_g is None else cu_g.numel() - 1
        # the grouped call keeps constants and workspace of its own, so that grouped and ungrouped steps (and graphs
        # captured of either) can alternate on one layer without replacing each other's workspace
        attr = "_ragged_group_state" if n_grp else "_ragged_state"
        st = getattr(self, attr, None)
        key = (self.sink_k.data_ptr(), self.window_k.data_ptr(), q.shape, n_seq, q.dtype) + ((n_grp,) if n_grp else ())
        if st is None or st["key"] != key:
            ws_bytes = 0
            if n_grp:
                ws_bytes = N.lib().sfa_decode_ragged_group_workspace_bytes(
                    n_seq, n_grp, H_q, H_kv, T, self.num_sink + self.window_size, D, N.SFA_DTYPE[q.dtype])
            if ws_bytes == 0:        # no groups; or a shape no grouped instance serves, which the library refuses itself
                ws_bytes = N.lib().sfa_decode_ragged_workspace_bytes(
                    n_seq, H_q, H_kv, T, self.num_sink + self.window_size, D, N.SFA_DTYPE[q.dtype])
            if ws_bytes == 0:
                raise ValueError(f"D={D}: a K/V row must be a multiple of 16 bytes, <= 1 KiB (H_q = {H_q} a multiple "
                                 f"of H_kv = {H_kv}, T >= 1)")
            st = self._call_consts(attr, key, ws_bytes, False, q)
        q, k_new, v_new = self._rows16(q), self._rows16(k_new), self._rows16(v_new)
        s_aux_f, aux = self._aux(s_aux)
        if out is None:
            out = torch.empty((1, H_q, T, D), device=q.device, dtype=q.dtype)
        sk, sv, wk, wv = st["descs"]
        name, mid, kvs = "sfa_decode_ring_ragged_slots", (), ()
        if parent is not None or commit_seq is not None or self._kv8 or self.page_size:
            name = self._pool_entry("sfa_decode_ring_ragged_tree_slots", "sfa_decode_ring_ragged_fp8",
                                    "sfa_decode_ring_ragged_paged")
            mid = (None if parent is None else parent.data_ptr(), None if commit_seq is None else commit_seq.data_ptr())
            kvs = self._pool_tail()
        grp = ()
        if cu_g is not None:     # the grouped forms of the two paged entry points: no parent, (cu_g, n_grp) behind n_seq
            name = "sfa_decode_ring_ragged_group_paged_fp8_slots" if self._kv8 else "sfa_decode_ring_ragged_group_paged_slots"
            mid, grp = mid[1:], (cu_g.data_ptr(), n_grp)
        with torch.cuda.device(q.device):
            rc = getattr(st["lib"], name)(N.desc(q), sk, sv, wk, wv, N.desc(k_new), N.desc(v_new), N.desc(out), aux, *mid,
                                          1 if commit else 0, dev_state.data_ptr(), slots.data_ptr(),
                                          cu.data_ptr(), n_seq, *grp, *kvs, st["ws"].data_ptr(), st["ws"].numel(),
                                          st["scale"], N.FLAG_RAGGED_ADMIT if admit else 0,
                                          N.stream_ptr(q.device))
        N.check(rc, name)
        return out

    @staticmethod
    def _group_arg(groups, n_seq, device):
        """``groups`` of ``ragged_step_dyn`` as a device int32 tensor ``[n_grp + 1]``: a device tensor is taken as it is
        (no sync), a host list / CPU tensor is checked against n_seq and uploaded."""
        if isinstance(groups, torch.Tensor) and groups.is_cuda:
            if groups.dtype.is_floating_point or groups.dtype == torch.bool or groups.dim() != 1:
                raise TypeError("groups must be a 1-D integer tensor")
            cu_g = groups.to(device=device, dtype=torch.int32).contiguous()
        else:
            lst = groups.tolist() if isinstance(groups, torch.Tensor) else [int(x) for x in groups]
            if len(lst) < 2 or lst[0] < 0 or lst[-1] > n_seq or any(b < a for a, b in zip(lst[:-1], lst[1:])):
                raise ValueError(f"bad groups {lst} for n_seq={n_seq}: need 0 <= g_0 <= g_1 <= ... <= n_seq")
            cu_g = torch.tensor(lst, dtype=torch.int32, device=device)
        if cu_g.numel() < 2:
            raise ValueError("groups needs at least two offsets")
        return cu_g

    @staticmethod
    def _packed_i32(x, n, what, nname, device):
        """A per-row / per-sequence int32 array of a packed call (None stays None): a device tensor is passed through
        unread (a cast / copy kernel at most), a host list / CPU tensor is checked for its length and uploaded."""
        if x is None:
            return None
        if isinstance(x, torch.Tensor):
            if x.dtype.is_floating_point or x.dtype.is_complex or x.dtype == torch.bool or x.dim() != 1:
                raise TypeError(f"{what} must be a 1-D integer tensor")
            lst = None if x.is_cuda else x.tolist()
        else:
            lst = [int(v) for v in x]
        if (len(lst) if lst is not None else x.numel()) != n:
            raise ValueError(f"{what} must hold {nname} = {n} entries, got {len(lst) if lst is not None else x.numel()}")
        if lst is not None:
            return torch.tensor(lst, dtype=torch.int32, device=device)
        return x.to(device=device, dtype=torch.int32).contiguous()

    def commit_packed_dyn(self, k_new: torch.Tensor, v_new: torch.Tensor, cu_q, slots, count, path=None) -> None:
        """Store the accepted prefixes / tree paths of a packed step (``sfa_ring_commit_path_ragged_slots``): ``k_new`` /
        ``v_new`` ``[1, H_kv, T, D]`` are the pack of the step, ``count`` ``[n_seq]`` the accepted tokens per sequence,
        ``path`` ``[T]`` (packed like ``k_new``, sequence-local entries; None: the identity) the order.  For sequence i
        with ``a = clamp(count[i], 0, n_i)`` the packed rows ``cu_q[i] + path[cu_q[i] : cu_q[i] + a]`` (entries clamped
        into [0, n_i)) enter the ring of slot ``slots[i]`` in that order and its state row advances by a: buffers and
        state are what ``commit_path_dyn(slots=)`` (``commit_dyn(slots=)`` without a path) leaves for the sequence's
        slice.  Inactive and empty sequences, ``a == 0`` and rows behind ``cu_q[-1]`` change nothing; never an admission.
        No host sync (``spec_tree.greedy_accept_packed`` gives ``path`` and ``count``); device tensors are not read on
        the host, host lists are checked for their length."""
        from . import _native as N
        dev_state = self._require_pool("commit_packed_dyn")
        N.require_gpu(k_new, v_new, self.window_k)
        _S, H_kv, _w, D = self.window_k.shape
        if k_new.dim() != 4 or k_new.shape[0] != 1 or k_new.shape[1] != H_kv or k_new.shape[3] != D or \
                v_new.shape != k_new.shape or k_new.shape[2] < 1:
            raise ValueError(f"k_new / v_new must be packed [1, H_kv, T, D] = [1, {H_kv}, T, {D}], got {tuple(k_new.shape)}")
        if self._kv8:
            self._act16("k_new / v_new", k_new, v_new)
        elif k_new.dtype != self.window_k.dtype or v_new.dtype != k_new.dtype:
            raise TypeError("k_new / v_new must have the cache buffers' dtype")
        T = k_new.shape[2]
        cu = self._cu_arg(cu_q, T, k_new.device)
        n_seq = cu.numel() - 1
        slots = self._slots_arg(slots, n_seq, writes=True)
        count = self._packed_i32(count, n_seq, "count", "n_seq", k_new.device)
        if count is None:
            raise TypeError("count must be an integer tensor or list of n_seq entries")
        path = self._packed_i32(path, T, "path", "T", k_new.device)
        N.require_gpu(slots)
        k_new, v_new = self._rows16(k_new), self._rows16(v_new)
        wk, wv = self._ring_descs()
        name = self._pool_entry("sfa_ring_commit_path_ragged_slots", "sfa_ring_commit_path_ragged_fp8",
                                "sfa_ring_commit_path_ragged_paged")
        with torch.cuda.device(k_new.device):
            rc = getattr(N.lib(), name)(wk, wv, N.desc(k_new), N.desc(v_new), count.data_ptr(),
                                        None if path is None else path.data_ptr(), cu.data_ptr(), n_seq,
                                        dev_state.data_ptr(), slots.data_ptr(),
                                        *self._pool_tail(n_slots=True), N.stream_ptr(k_new.device))
        N.check(rc, name)

    def packed_positions(self, cu_q, slots, T: int) -> torch.Tensor:
        """RoPE positions of a packed step: for packed row ``cu_q[i] + t`` of sequence i, ``seen[slots[i]] + t``; -1 for
        rows behind ``cu_q[-1]`` (padding) and for rows of inactive sequences.  ``[T]`` int64, built from torch ops on
        the tensors' device (``bucketize`` over ``arange(T)``: no sync, capturable); call it before the committing
        ``ragged_step_dyn`` of the step, which moves ``seen``.  With draft trees in the pack (``parent=``) node u sits
        at ``seen + depth[u]``: ``pos - spec_tree.packed_local(cu_q, T) + spec_tree.packed_tree_depth(parent, cu_q, T)``
        for the rows with ``pos >= 0``."""
        dev_state = self._require_pool("packed_positions")
        cu = cu_q if isinstance(cu_q, torch.Tensor) else torch.tensor([int(x) for x in cu_q], device=dev_state.device)
        sl = slots if isinstance(slots, torch.Tensor) else torch.tensor([int(x) for x in slots], device=dev_state.device)
        if cu.dim() != 1 or cu.numel() < 2 or sl.dim() != 1 or sl.numel() != cu.numel() - 1:
            raise ValueError("cu_q must hold n_seq + 1 >= 2 offsets and slots n_seq entries")
        cu, sl = cu.to(dev_state.device).long(), sl.to(dev_state.device).long()
        n_seq, S = sl.numel(), dev_state.shape[0]
        rows = torch.arange(int(T), device=cu.device)
        # the last sequence that starts at or before the row (empty sequences share a start with their successor)
        seq = (torch.bucketize(rows, cu[:n_seq], right=True) - 1).clamp(0, n_seq - 1)
        slot = sl[seq]
        ok = (rows >= cu[seq]) & (rows < cu[seq + 1]) & (slot >= 0) & (slot < S)
        pos = dev_state[slot.clamp(0, S - 1), 3].long() + rows - cu[seq]
        return torch.where(ok, pos, torch.full_like(pos, -1))

    # ------------------------------------------------------- HF layer surface
    def get_seq_length(self, *_, **__) -> int:
        self._refuse_per_seq("get_seq_length")
        return self.sink_len + self.window_len

    def get_mask_sizes(self, cache_position, *_, **__) -> Tuple[int, int]:
        return self.get_seq_length(), 0

    def get_max_cache_shape(self) -> int:
        return self.num_sink + self.window_size

    def get_max_length(self) -> int:   # abstract in transformers >= 5 (the reference predates it)
        return self.num_sink + self.window_size

    def reorder_cache(self, beam_idx: torch.LongTensor):
        if self.sink_k is None:
            return
        idx = beam_idx.to(self.sink_k.device)
        self.sink_k, self.sink_v = self.sink_k.index_select(0, idx), self.sink_v.index_select(0, idx)
        self.window_k, self.window_v = self.window_k.index_select(0, idx), self.window_v.index_select(0, idx)
        if self._per_seq:       # the state rows follow their sequences
            self._dev_state = self._dev_state.index_select(0, idx.to(self._dev_state.device))


class SinkAttentionCache(_HFCache if _HAS_HF else object):
    """Per-layer ``SinkCacheLayer``s behind the transformers ``Cache`` interface (layers created on first use)."""

    def __init__(self, num_sink: int = 4, window_size: int = 4096):
        self.num_sink, self.window_size = num_sink, window_size
        self._seen_tokens = 0
        if _HAS_HF:
            super().__init__(layer_class_to_replicate=None, layers=[])
        else:  # pragma: no cover
            self.layers: List[SinkCacheLayer] = []

    def __len__(self):
        return len(self.layers)

    def __getitem__(self, idx):
        return self.layers[idx]

    def __repr__(self):
        return (f"SinkAttentionCache(num_sink={self.num_sink}, window_size={self.window_size}, "
                f"layers={len(self.layers)}, seen_tokens={self._seen_tokens})")

    def _layer(self, layer_idx: int) -> SinkCacheLayer:
        while len(self.layers) <= layer_idx:
            self.layers.append(SinkCacheLayer(self.num_sink, self.window_size))
        return self.layers[layer_idx]

    def update(self, key_states, value_states, layer_idx: int, cache_kwargs: Optional[dict] = None):
        out = self._layer(layer_idx).update(key_states, value_states, cache_kwargs)
        if layer_idx == 0:
            self._seen_tokens = self.layers[0].seen_tokens
        return out

    def append(self, key_states, value_states, layer_idx: int) -> None:
        """Copy-free decode update of one layer (pair with ``self[layer_idx].decode_attention``)."""
        self._layer(layer_idx).append(key_states, value_states)
        if layer_idx == 0:
            self._seen_tokens = self.layers[0].seen_tokens

    def decode_step(self, q, key_states, value_states, layer_idx: int, s_aux=None):
        """Fused cache update + attention of one layer for one new token (``SinkCacheLayer.decode_step``)."""
        out = self._layer(layer_idx).decode_step(q, key_states, value_states, s_aux=s_aux)
        if layer_idx == 0:
            self._seen_tokens = self.layers[0].seen_tokens
        return out

    def extend_attention(self, q, key_states, value_states, layer_idx: int, s_aux=None):
        """n new tokens of one layer attended over its cache WITHOUT committing them (``SinkCacheLayer.extend_attention``)."""
        return self._layer(layer_idx).extend_attention(q, key_states, value_states, s_aux=s_aux)

    def extend_step(self, q, key_states, value_states, layer_idx: int, s_aux=None):
        """n new tokens of one layer: attention + commit (``SinkCacheLayer.extend_step``)."""
        out = self._layer(layer_idx).extend_step(q, key_states, value_states, s_aux=s_aux)
        if layer_idx == 0:
            self._seen_tokens = self.layers[0].seen_tokens
        return out

    def decode_step_dyn(self, q, key_states, value_states, layer_idx: int, s_aux=None, out=None, slots=None):
        """``SinkCacheLayer.decode_step_dyn`` of one layer: the fused single-token step with the state on the device."""
        return self._layer(layer_idx).decode_step_dyn(q, key_states, value_states, s_aux=s_aux, out=out, slots=slots)

    def extend_attention_dyn(self, q, key_states, value_states, layer_idx: int, s_aux=None, out=None, slots=None):
        """``SinkCacheLayer.extend_attention_dyn`` of one layer: verify with the state on the device (capturable)."""
        return self._layer(layer_idx).extend_attention_dyn(q, key_states, value_states, s_aux=s_aux, out=out,
                                                           slots=slots)

    def extend_step_dyn(self, q, key_states, value_states, layer_idx: int, s_aux=None, out=None, slots=None):
        """``SinkCacheLayer.extend_step_dyn`` of one layer: attention + commit of all n tokens, state on the device.
        ``seen_tokens`` follows after ``pull_state()`` of layer 0."""
        return self._layer(layer_idx).extend_step_dyn(q, key_states, value_states, s_aux=s_aux, out=out, slots=slots)

    def commit_dyn(self, key_states, value_states, count, layer_idx: int, slots=None) -> None:
        """``SinkCacheLayer.commit_dyn`` of one layer: store the first ``count`` (device tensor) tokens of the chunk."""
        self._layer(layer_idx).commit_dyn(key_states, value_states, count, slots=slots)

    def extend_attention_tree(self, q, key_states, value_states, parent, layer_idx: int, s_aux=None):
        """``SinkCacheLayer.extend_attention_tree`` of one layer: verify a draft tree, host state, nothing committed."""
        return self._layer(layer_idx).extend_attention_tree(q, key_states, value_states, parent, s_aux=s_aux)

    def extend_attention_tree_dyn(self, q, key_states, value_states, parent, layer_idx: int, s_aux=None, out=None,
                                  slots=None):
        """``SinkCacheLayer.extend_attention_tree_dyn`` of one layer: verify a draft tree, state on the device."""
        return self._layer(layer_idx).extend_attention_tree_dyn(q, key_states, value_states, parent, s_aux=s_aux,
                                                                out=out, slots=slots)

    def commit_path(self, key_states, value_states, path, layer_idx: int) -> None:
        """``SinkCacheLayer.commit_path`` of one layer: append the chunk rows of an accepted path (host state)."""
        self._layer(layer_idx).commit_path(key_states, value_states, path)
        if layer_idx == 0:
            self._seen_tokens = self.layers[0].seen_tokens

    def commit_path_dyn(self, key_states, value_states, path, count, layer_idx: int, slots=None) -> None:
        """``SinkCacheLayer.commit_path_dyn`` of one layer: store the first ``count`` (device) rows of ``path``."""
        self._layer(layer_idx).commit_path_dyn(key_states, value_states, path, count, slots=slots)

    def prefill_varlen(self, key_states, value_states, cu_seqlens, layer_idx: int) -> torch.Tensor:
        """``SinkCacheLayer.prefill_varlen`` of one layer: a packed ragged batch into per-sequence buffers and state."""
        return self._layer(layer_idx).prefill_varlen(key_states, value_states, cu_seqlens)

    page_table = None    # paged pools: the one table every layer's pool shares (init_pool(page_size=...))
    _pages = None

    def init_pool(self, num_slots: int, H_kv: int, D: int, dtype=torch.bfloat16, device="cuda",
                  layer_idx: int = 0, page_size=None, num_pages=None, page_table=None, kv_dtype=None) -> torch.Tensor:
        """``SinkCacheLayer.init_pool`` of one layer: a pool of ``num_slots`` cache rows and its ``[S, 4]`` state.  With
        ``page_size`` the layers' pools are paged and share ONE table tensor (``cache.page_table``: that of the first
        paged layer, or the given one) and one allocator, so one mapping serves every layer: the layers must agree in
        ``num_slots``, ``page_size`` and ``num_pages``."""
        layer = self._layer(layer_idx)
        if page_size is None:
            return layer.init_pool(num_slots, H_kv, D, dtype, device, kv_dtype=kv_dtype)
        shared = self.page_table if page_table is None else page_table
        state = layer.init_pool(num_slots, H_kv, D, dtype, device, page_size=page_size, num_pages=num_pages,
                                page_table=shared, kv_dtype=kv_dtype)
        if self._pages is not None and shared is self.page_table:
            if (self._pages.num_pages, self._pages.page_size) != (layer._pages.num_pages, layer._pages.page_size):
                raise ValueError("init_pool: the paged layers of a cache share one table and must agree in page_size "
                                 "and num_pages")
            layer._pages = self._pages
            self._pages.attach(layer)      # reserve_pages copies pages on every layer of the table
        else:
            self.page_table, self._pages = layer.page_table, layer._pages
        return state

    def reserve_pages(self, slots, tokens_after) -> None:
        """``SinkCacheLayer.reserve_pages`` on the table the layers share: one mapping serves every layer."""
        if self._pages is None:
            raise TypeError("reserve_pages needs a paged pool: init_pool(..., page_size=P)")
        _copy_pages(self._pages, self._pages.reserve(slots, tokens_after))

    def free_pages(self, slots) -> None:
        """``SinkCacheLayer.free_pages`` on the table the layers share."""
        if self._pages is None:
            raise TypeError("free_pages needs a paged pool: init_pool(..., page_size=P)")
        self._pages.free(slots)

    def set_kv_scale(self, k_scale, v_scale, layer_idx: int) -> None:
        """``SinkCacheLayer.set_kv_scale`` of one layer: the static per-KV-head scales of its FP8 pool, copied in place."""
        self._layer(layer_idx).set_kv_scale(k_scale, v_scale)

    def prefill_slots(self, key_states, value_states, cu_seqlens, slots, layer_idx: int) -> torch.Tensor:
        """``SinkCacheLayer.prefill_slots`` of one layer: packed sequences into the named slots of its pool."""
        return self._layer(layer_idx).prefill_slots(key_states, value_states, cu_seqlens, slots)

    def ragged_step_dyn(self, q, key_states, value_states, cu_q, slots, layer_idx: int, s_aux=None, out=None,
                        commit=True, admit: bool = False, parent=None, commit_seq=None, groups=None):
        """``SinkCacheLayer.ragged_step_dyn`` of one layer: a packed step, every sequence with its own token count;
        ``admit=True`` takes sequences on fresh slots from position 0 in the same call; ``parent`` / ``commit_seq``:
        draft trees in the pack and per-sequence commit; ``groups``: fork groups whose shared prompt prefix is read once
        (paged pools)."""
        return self._layer(layer_idx).ragged_step_dyn(q, key_states, value_states, cu_q, slots, s_aux=s_aux, out=out,
                                                      commit=commit, admit=admit, parent=parent, commit_seq=commit_seq,
                                                      groups=groups)

    def commit_packed_dyn(self, key_states, value_states, cu_q, slots, count, layer_idx: int, path=None) -> None:
        """``SinkCacheLayer.commit_packed_dyn`` of one layer: store the accepted prefixes / paths of a packed step."""
        self._layer(layer_idx).commit_packed_dyn(key_states, value_states, cu_q, slots, count, path=path)

    def packed_positions(self, cu_q, slots, T: int, layer_idx: int = 0) -> torch.Tensor:
        """``SinkCacheLayer.packed_positions`` of one layer: the RoPE position of every packed row (-1: no row)."""
        return self._layer(layer_idx).packed_positions(cu_q, slots, T)

    def live_lengths(self, slots, layer_idx: int = 0) -> torch.Tensor:
        """``SinkCacheLayer.live_lengths`` of one layer: the tokens each named slot holds (sinks + ring)."""
        return self._layer(layer_idx).live_lengths(slots)

    def export_slots(self, slots, layer_idx: int, cu=None, T=None, out=None, return_positions: bool = False):
        """``SinkCacheLayer.export_slots`` of one layer: the named slots as packed K/V in token order."""
        return self._layer(layer_idx).export_slots(slots, cu=cu, T=T, out=out, return_positions=return_positions)

    def import_slots(self, key_states, value_states, cu, slots, layer_idx: int, seen=None) -> torch.Tensor:
        """``SinkCacheLayer.import_slots`` of one layer: admit an exported pack; ``seen`` restores the positions."""
        return self._layer(layer_idx).import_slots(key_states, value_states, cu, slots, seen=seen)

    def release_slots(self, slots) -> None:
        """``SinkCacheLayer.release_slots`` of every layer that holds a pool (layers without one are skipped)."""
        for layer in self.layers:
            if layer._pool:
                layer.release_slots(slots)

    def fork_slots(self, src, dst, source: Optional["SinkAttentionCache"] = None, share: bool = False,
                   tokens=None) -> None:
        """``SinkCacheLayer.fork_slots`` of every layer that holds a pool: slot ``src[i]`` of ``source`` (another
        ``SinkAttentionCache`` whose layer l holds the pool that layer l here is paired with; default: this cache) into
        slot ``dst[i]`` of this cache.  ``share=True`` (paged pools on the cache's one table; ``tokens``: the exact
        ``seen`` of each source): the table rows are aliased ONCE (``PageAllocator.share``), then every pooled layer
        copies its sinks and state rows (``sfa_ring_share_paged_slots``); rules and refusals as in
        ``SinkCacheLayer.fork_slots``.  Host bookkeeping: not capturable."""
        if share:
            if self._pages is None:
                raise TypeError("fork_slots(share=True) needs a paged pool: init_pool(..., page_size=P)")
            if source is not None and source is not self:
                raise ValueError("fork_slots(share=True): pages are shared within one page buffer: source must be None or "
                                 "the object itself (between two pools use share=False)")
            pooled = [layer for layer in self.layers if layer._pool]
            if any(layer._pages is not self._pages for layer in pooled):
                raise ValueError("fork_slots(share=True): every pooled layer of the cache must be paged on the cache's table")
            args = [layer._share_args(src, dst, None, tokens) for layer in pooled]
            if not args:
                return
            from . import _native as N
            N.require_gpu(*(layer.sink_k for layer in pooled))
            self._pages.share(*args[0][:3])
            for layer, a in zip(pooled, args):
                layer._share_call(a[3], a[4])
            return
        if tokens is not None:
            raise ValueError("fork_slots: tokens belongs to share=True")
        if source is not None and not isinstance(source, SinkAttentionCache):
            raise TypeError("fork_slots: source must be a SinkAttentionCache")
        for l, layer in enumerate(self.layers):
            if not layer._pool:
                continue
            if source is not None and l >= len(source.layers):
                raise ValueError(f"fork_slots: source has no layer {l}")
            layer.fork_slots(src, dst, None if source is None else source.layers[l])

    def get_seq_length(self, layer_idx: int = 0, *_, **__) -> int:
        return self.layers[layer_idx].get_seq_length() if layer_idx < len(self.layers) else 0

    def get_max_cache_length(self) -> int:
        return self.num_sink + self.window_size

    def reorder_cache(self, beam_idx):
        for layer in self.layers:
            layer.reorder_cache(beam_idx)

    @property
    def seen_tokens(self) -> int:
        return self._seen_tokens


def group_offsets(group_ids) -> list:
    """``groups`` of ``ragged_step_dyn`` from one group id per sequence of the pack: sequences with the same id must be
    consecutive (a run is one group), ``None`` or a negative id leaves a sequence ungrouped.  Returns the host list of
    offsets ``[n_grp + 1]``.  Offsets are consecutive, so every sequence lies in some run: an ungrouped sequence becomes
    a group of one, which the step computes exactly as an ungrouped one."""
    ids = [None if (g is None or (isinstance(g, int) and g < 0)) else g for g in group_ids]
    cu, seen, prev = [0], set(), object()
    for i, g in enumerate(ids):
        if i and (g is None or g != prev):
            cu.append(i)
        if g is not None and g != prev:
            if g in seen:
                raise ValueError(f"group id {g} is not consecutive in {list(group_ids)}")
            seen.add(g)
        prev = g if g is not None else object()
    cu.append(len(ids))
    return cu


def beam_fork_plan(beam_idx, slots, free_slots):
    """Slot bookkeeping of one beam-search step over a pool, on host lists (no GPU).  Row b of the next step continues
    the sequence that row ``beam_idx[b]`` held in slot ``slots[beam_idx[b]]``.  Returns ``(new_slots, src, dst,
    freed)``: the first row that continues a beam keeps that beam's slot; every further row that continues it takes a
    slot from ``free_slots`` (in order) and contributes a pair ``(src[i], dst[i])``; the slots of beams that nobody
    continues are ``freed``.  Raises ``ValueError`` when ``free_slots`` runs out.  A beam step is then
    ``fork_slots(src, dst)``, ``release_slots(freed)`` and an in-place rewrite of the step's ``slots`` tensor with
    ``new_slots``: no destination is a source, so nothing is permuted in place.  A freed slot is free from the next
    step on (it may still be a source of this one only if somebody continues it, and then it is not freed)."""
    beam_idx, slots, free = [int(x) for x in beam_idx], [int(x) for x in slots], [int(x) for x in free_slots]
    B = len(slots)
    if len(beam_idx) != B:
        raise ValueError(f"beam_idx must hold one entry per row: {len(beam_idx)} entries for {B} slots")
    bad = [p for p in beam_idx if not 0 <= p < B]
    if bad:
        raise ValueError(f"beam_idx entries {bad} outside [0, {B})")
    new_slots, src, dst, kept = [], [], [], set()
    for p in beam_idx:
        if p not in kept:
            kept.add(p)
            new_slots.append(slots[p])
            continue
        if not free:
            raise ValueError(f"beam_fork_plan: free_slots ran out ({len(dst)} forks placed, more needed)")
        d = free.pop(0)
        src.append(slots[p])
        dst.append(d)
        new_slots.append(d)
    freed = [slots[p] for p in range(B) if p not in kept]
    return new_slots, src, dst, freed
