"""CPU-only tests of page sharing on a fork (copy on first write): the reference counts of PageAllocator against its
rule on a CPU int32 table - P = 32, Wc = 128, 12 pages -, the refusals of fork_slots(share=True), the
two new symbols in the header, and the host checks of sfa_pages_copy / sfa_ring_share_paged_slots (status and exact
sfa_last_error() text; host tensors stand in for device memory as in tests/test_paged_pool_host.py - every call returns
before a launch).  The last test restates the address check of tests/test_far_views.py for the far case of
tests/test_gpu_page_share.py."""
import copy
import ctypes
import os
import subprocess
import tempfile

import pytest
import torch

import far_views as F
from sink_attention import PageAllocator, SinkAttentionCache, SinkCacheLayer, pages_needed
from sink_attention import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, W, NP, S = 32, 128, 12, 6
PER = W // P
HKV, D, NS = 2, 64, 4
PTR = ctypes.c_void_p(0x1000)      # stands in for a device array: never read
_KEEP = []


def _alloc(n_pages=NP):
    return PageAllocator(torch.full((S, PER), -1, dtype=torch.int32), n_pages, P, W)


def _state(a):
    return copy.deepcopy((a.table.tolist(), a.rows, a.refcount, a.free_list, a.lo, a.shared))


def _consistent(a):
    """refcount[p] = table entries that name p; on the free list iff 0; the table mirrors rows"""
    flat = [p for r in a.rows for p in r]
    assert a.refcount == [flat.count(p) for p in range(a.num_pages)]
    assert sorted(a.free_list) == [p for p in range(a.num_pages) if a.refcount[p] == 0]
    assert a.table.tolist() == [r + [-1] * (PER - len(r)) for r in a.rows]


class _Parent:
    """the allocator before reference counts, restated: a free list popped from the end, growth slot by slot"""

    def __init__(self, n_pages):
        self.free_list, self.rows = list(range(n_pages - 1, -1, -1)), [[] for _ in range(S)]

    def reserve(self, slots, tokens):
        tok = [tokens] * len(slots) if isinstance(tokens, int) else tokens
        more = [max(pages_needed(t, W, P) - len(self.rows[s]), 0) for s, t in zip(slots, tok)]
        if sum(more) > len(self.free_list):
            raise RuntimeError(f"out of pages: need {sum(more)}, free {len(self.free_list)}")
        for s, m in zip(slots, more):
            for _ in range(m):
                self.rows[s].append(self.free_list.pop())

    def free(self, slots):
        for s in slots:
            self.free_list += self.rows[s]
            self.rows[s] = []


# ------------------------------------------------------------------------------------------------ unshared: unchanged
def test_unshared_use_hands_out_the_page_ids_of_the_parent():
    """the calls of tests/test_paged_pool_host.py (reserve, grow, cap at Wc / P, exhaustion, free, reuse), step by step"""
    a, ref = _alloc(), _Parent(NP)
    script = [("reserve", [3, 1], [40, 1]), ("reserve", [3, 1], [64, 33]), ("reserve", [0], 10 ** 6),
              ("reserve", [2, 4], [128, 1]), ("reserve", [5, 3], [33, 128]), ("reserve", [3], 64), ("free", [1]),
              ("reserve", [5], 70), ("free", [0, 3]), ("reserve", [1, 3], [96, 20]), ("free", [5, 2, 1, 3, 4])]
    raised = 0
    for op, slots, *tok in script:
        before = _state(a)
        try:
            got = getattr(a, op)(slots, *tok)
            getattr(ref, op)(slots, *tok)
            assert got == ([] if op == "reserve" else None)          # nothing to copy without a share
        except RuntimeError as e:
            with pytest.raises(RuntimeError) as e2:
                getattr(ref, op)(slots, *tok)
            assert str(e) == str(e2.value) == "out of pages: need 5, free 4" and _state(a) == before
            raised += 1
        assert a.rows == ref.rows and a.free_list == ref.free_list, (op, slots)
        _consistent(a)
    assert raised == 1 and len(a.free_list) == NP and a.refcount == [0] * NP


# ------------------------------------------------------------------------------------------------ share and the rule
def _forked(lo, n_forks=2, mapped=None):
    """slot 0 holds `mapped` (default: lo) ring tokens, forked into slots 1 .. n_forks at lo"""
    a = _alloc()
    a.reserve([0], lo if mapped is None else mapped)
    free = list(a.free_list)
    a.share([0] * n_forks, list(range(1, n_forks + 1)), lo)
    assert a.free_list == free                                     # nothing is popped
    return a


def test_share_aliases_the_rows_and_counts_the_references():
    a = _forked(70, n_forks=3)
    assert a.rows[0] == [0, 1, 2] and a.rows[1] == a.rows[2] == a.rows[3] == a.rows[0]
    assert a.rows[1] is not a.rows[0] and a.table[:4].tolist() == [[0, 1, 2, -1]] * 4
    assert a.refcount[:3] == [4, 4, 4] and a.lo[:4] == [70] * 4 and len(a.free_list) == NP - 3
    _consistent(a)
    with pytest.raises(ValueError, match=r"slot 2 still maps 3 pages: free_pages\(2\) comes first"):
        a.share([0], [2], 70)
    for src, dst in (([0], [0]), ([9], [4]), ([4], [9]), ([0, 4], [4, 5]), ([0], [4, 5])):
        before = _state(a)
        with pytest.raises(ValueError):
            a.share(src, dst, 70)
        assert _state(a) == before


@pytest.mark.parametrize("lo,copied", [(40, [1]), (5, [0]), (31, [0]), (64, []), (0, [])])
def test_the_first_reserve_copies_exactly_the_pages_the_rule_names(lo, copied):
    """lo inside page 1, inside page 0, on the last row of page 0, on a page boundary (no copy, only growth), empty ring"""
    a = _forked(lo)
    own = list(a.rows[0])
    got = a.reserve([1], lo + 1)                                   # a decode row: positions [lo, lo + 1)
    grown = pages_needed(lo + 1, W, P) - len(own)
    assert [s for s, _ in got] == [own[j] for j in copied]
    fresh = [d for _, d in got]
    assert a.rows[1] == [fresh[copied.index(j)] if j in copied else own[j] for j in range(len(own))] + \
        a.rows[1][len(own):] and len(a.rows[1]) == len(own) + grown
    assert all(a.refcount[p] == 1 for p in fresh + a.rows[1][len(own):]) and a.rows[0] == a.rows[2] == own
    assert [a.refcount[p] for p in own] == [2 if j in copied else 3 for j in range(len(own))]
    _consistent(a)
    assert a.reserve([1], lo + 2) == [] and a.reserve([1], min(lo + 20, P * len(a.rows[1]))) == []     # later: nothing
    # a chunk that crosses into the next shared page copies both (the source mapped one page more than it holds)
    b = _forked(40, mapped=96)
    assert [s for s, _ in b.reserve([2], 70)] == [b.rows[0][1], b.rows[0][2]] and b.rows[2][0] == b.rows[0][0]


def test_past_the_ring_every_shared_entry_is_made_private():
    a = _forked(W, n_forks=1)
    own = list(a.rows[0])
    got = a.reserve([1], W + 1)            # the host cannot know write_pos: a long prompt is placed with write_pos = 0
    assert [s for s, _ in got] == own and not set(a.rows[1]) & set(own) and all(a.refcount[p] == 1 for p in own + a.rows[1])
    assert a.reserve([0], W + 1) == [] and a.reserve([1], 3 * W) == []           # what is left is each slot's own
    _consistent(a)
    b = _forked(W - 1, n_forks=1)
    assert [s for s, _ in b.reserve([1], W)] == [b.rows[0][3]]                    # not wrapped yet: the last page alone


def test_source_and_last_fork_in_one_call_copy_once_and_tokens_before_lowers_lo():
    a = _forked(40, n_forks=1)
    own = list(a.rows[0])
    got = a.reserve([0, 1], [41, 41])
    assert len(got) == 1 and got[0][0] == own[1] and a.rows[0][1] == got[0][1] and a.rows[1] == own     # the first copies
    assert a.reserve([1, 0], 45) == []
    _consistent(a)
    b = _forked(40, n_forks=1)
    assert [s for s, _ in b.reserve([1], 41, tokens_before=10)] == [b.rows[0][0], b.rows[0][1]] and b.lo[1] == 10
    with pytest.raises(ValueError, match="one per slot"):
        b.reserve([0, 1], 41, tokens_before=[1])


def test_free_keeps_shared_pages_alive_and_freeing_everything_restores_the_pool():
    a = _forked(70)
    own = list(a.rows[0])
    a.reserve([1], 71)
    a.free([0])                                                    # the source first: its pages live on in the forks
    assert a.rows[0] == [] and a.table[0].tolist() == [-1] * PER and a.lo[0] == 0
    assert [a.refcount[p] for p in own] == [2, 2, 1] and not set(own) & set(a.free_list)
    assert a.rows[2] == own and a.rows[1][:2] == own[:2]
    _consistent(a)
    a.free([2])
    assert a.free_list[-1] == own[2] and a.refcount[own[0]] == 1              # entry by entry, as before
    a.free([1])
    assert len(a.free_list) == NP and a.refcount == [0] * NP and bool((a.table == -1).all()) and a.lo == [0] * S


def test_an_out_of_pages_copy_on_write_raises_and_changes_nothing():
    a = _alloc(5)
    a.reserve([0], 96)
    a.share([0, 0], [1, 2], 70)
    a.reserve([3], 33)                                             # the pool is full: 3 shared + 2
    before = _state(a)
    with pytest.raises(RuntimeError, match=r"^out of pages: need 1, free 0$"):
        a.reserve([1], 71)                                         # one copy, no growth
    assert _state(a) == before
    a.free([3])
    before = _state(a)
    assert before[2:4] == ([3, 3, 3, 0, 0], [3, 4])
    with pytest.raises(RuntimeError, match=r"^out of pages: need 3, free 2$"):
        a.reserve([1, 4], [71, 40])                                # copy and growth are counted together
    assert _state(a) == before
    assert len(a.reserve([1, 4], [71, 20])) == 1
    _consistent(a)


def test_pool_bytes_counts_distinct_pages():
    a = _forked(70, n_forks=3)
    page = 2 * HKV * P * D * 2
    assert a.pool_bytes(HKV, D, 2) == 3 * page
    a.reserve([1, 2], 71)
    assert a.pool_bytes(HKV, D, 2) == 5 * page and sum(len(r) for r in a.rows) == 12


# ------------------------------------------------------------------------------------------------ Python surface
def _cpu_pool(paged=True, cls=SinkCacheLayer, layers=1):
    obj = cls(NS, W)
    for l in range(layers):
        kw = dict(layer_idx=l) if cls is SinkAttentionCache else {}
        obj.init_pool(S, HKV, D, torch.bfloat16, "cpu", **kw, **(dict(page_size=P, num_pages=NP) if paged else {}))
    return obj


def test_every_layer_of_a_table_is_registered_with_its_allocator():
    layer = _cpu_pool()
    assert layer._pages.layers == [layer] and layer._pages.refcount == [0] * NP
    cache = _cpu_pool(cls=SinkAttentionCache, layers=3)
    assert [id(l) for l in cache._pages.layers] == [id(cache[l]) for l in range(3)]
    assert all(cache[l]._pages is cache._pages for l in range(3))
    assert cache.reserve_pages([0], 5) is None and layer.reserve_pages([0], 5) is None        # the signatures stay


@pytest.mark.parametrize("cls", [SinkCacheLayer, SinkAttentionCache])
def test_refusals_of_a_shared_fork(cls):
    with pytest.raises(TypeError, match=r"fork_slots\(share=True\) needs a paged pool: init_pool\(\.\.\., page_size=P\)"):
        _cpu_pool(paged=False, cls=cls).fork_slots([0], [1], share=True, tokens=9)
    pool, other = _cpu_pool(cls=cls), _cpu_pool(cls=cls)
    pool.reserve_pages([0], 44)
    alloc = pool._pages
    before = _state(alloc)
    with pytest.raises(ValueError, match="source must be None or the object itself"):
        pool.fork_slots([0], [1], source=other, share=True, tokens=44)
    with pytest.raises(TypeError, match="host lists or CPU tensors.*not capturable"):
        pool.fork_slots(_FakeCuda([0]), [1], share=True, tokens=44)
    for src, dst in (([0], [-1]), ([-1], [1]), ([0], [0]), ([0], [S]), ([S], [1])):
        with pytest.raises(ValueError, match="two distinct slots of the pool"):
            pool.fork_slots(src, dst, share=True, tokens=44)
    with pytest.raises(ValueError, match="pair up"):
        pool.fork_slots([0, 0], [1], share=True, tokens=44)
    with pytest.raises(ValueError, match=r"needs tokens=: the exact seen"):
        pool.fork_slots([0], [1], share=True)
    with pytest.raises(ValueError, match="one number or one per pair"):
        pool.fork_slots([0, 0], [1, 2], share=True, tokens=[44])
    with pytest.raises(ValueError, match="names a destination twice"):
        pool.fork_slots([0, 0], [1, 1], share=True, tokens=44)
    with pytest.raises(ValueError, match="a destination and the source of another pair"):
        pool.fork_slots([0, 1], [1, 2], share=True, tokens=44)
    with pytest.raises(ValueError, match="tokens belongs to share=True"):
        pool.fork_slots([0], [1], tokens=44)
    assert _state(alloc) == before                                  # no refusal moved the table
    with pytest.raises(RuntimeError, match="MI355X"):               # every check passed: only the device is missing
        pool.fork_slots(torch.tensor([0, 0]), [1, 2], share=True, tokens=[44, 44])
    assert _state(alloc) == before


class _FakeCuda(torch.Tensor):
    """a CPU tensor that says it lives on the GPU: the refusal reads is_cuda and nothing else"""

    @staticmethod
    def __new__(cls, data):
        return torch.Tensor._make_subclass(cls, torch.tensor(data, dtype=torch.int32))

    @property
    def is_cuda(self):
        return True


def test_a_layer_of_a_shared_table_points_to_the_cache_level_call():
    cache = _cpu_pool(cls=SinkAttentionCache, layers=2)
    cache.reserve_pages([0], 44)
    with pytest.raises(ValueError, match=r"serves 2 layers .* call SinkAttentionCache.fork_slots\(share=True\)"):
        cache[1].fork_slots([0], [1], share=True, tokens=44)
    assert cache._pages.rows[1] == []


# ------------------------------------------------------------------------------------------------ exports, header
def test_the_two_symbols_are_exported_and_declared():
    lib = N.lib()
    assert len(lib.sfa_pages_copy.argtypes) == 6 and len(lib.sfa_ring_share_paged_slots.argtypes) == 10
    assert lib.sfa_abi_version() == 2 and N.ABI_VERSION == 2
    TT, I = "const sfa_tensor*", "const int32_t*"
    src = ('#include "sfa.h"\n'
           'int main(void) {\n'
           f'  int (*a)({TT}, {TT}, {I}, {I}, int, void*) = sfa_pages_copy;\n'
           f'  int (*b)({TT}, {TT}, {I}, {TT}, {TT}, int32_t*, {I}, {I}, int, void*) = sfa_ring_share_paged_slots;\n'
           '  return a == 0 || b == 0 || SFA_ABI_VERSION != 2;\n'
           '}\n')
    with tempfile.NamedTemporaryFile("w", suffix=".c", delete=False) as f:
        f.write(src)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                        "-fsyntax-only", f.name], capture_output=True, text=True)
    os.unlink(f.name)
    assert r.returncode == 0, r.stderr


# ------------------------------------------------------------------------------------------------ C ABI refusals
def _d(*shape, dtype=torch.bfloat16, view=None):
    t = torch.zeros(*shape, dtype=dtype)
    _KEEP.append(t)
    return N.desc(t if view is None else view(t))


def _pc(wk, wv, src=PTR, dst=PTR, n=2):
    lib = N.lib()
    rc = lib.sfa_pages_copy(wk, wv, src, dst, n, None)
    return rc, lib.sfa_last_error().decode()


def test_refusals_of_pages_copy():
    pg = lambda n=NP, d=D, dt=torch.bfloat16, p=P: _d(n, HKV, p, d, dtype=dt)
    assert _pc(None, pg()) == (-1, "window_k: null tensor descriptor")
    assert _pc(pg(), None) == (-1, "window_v: null tensor descriptor")
    assert _pc(pg(), pg(), n=-1) == (-1, "n_pairs must be >= 0 (got -1)")
    assert _pc(pg(), pg(NP + 1)) == (-1, f"window_k and window_v differ in shape[0]: {NP} vs {NP + 1}")
    assert _pc(pg(), pg(p=64)) == (-1, "window_k and window_v differ in shape[2]: 32 vs 64")
    assert _pc(pg(), pg(dt=torch.float16)) == (-1, "window_k and window_v differ in dtype")
    assert _pc(pg(dt=torch.float32), pg(dt=torch.float32)) == (-1, "pages_copy: the page buffers hold bf16, f16 or FP8 (e4m3) "
                                                                   "(got dtype 0)")
    assert _pc(pg(0), pg(0)) == (-1, "pages_copy: the page buffers need shape[0] = n_pages in [1, 2^30) (got 0)")
    assert _pc(pg(), pg(), None, None, n=0) == (0, "")                       # nothing to do, nothing launched
    assert _pc(pg(), pg(), None) == (-1, "src_pages: null device pointer")
    assert _pc(pg(), pg(), PTR, None) == (-1, "dst_pages: null device pointer")
    assert _pc(pg(d=20), pg(d=20)) == (-1, "pages_copy: K/V rows must be a multiple of 16 bytes (head dim 20)")
    odd = _d(NP, HKV, P, D + 4, view=lambda t: t[..., :D])                   # rows 136 bytes apart
    assert _pc(odd, odd) == (-1, "pages_copy: rows of every tensor must be 16-byte aligned")
    f8 = pg(dt=torch.float8_e4m3fn, d=40)
    assert _pc(f8, f8) == (-1, "pages_copy: K/V rows must be a multiple of 16 bytes (head dim 40)")


def _sh(sk, sv, dk, dv, sstate=PTR, dstate=PTR, ss=PTR, ds=PTR, n=1):
    lib = N.lib()
    rc = lib.sfa_ring_share_paged_slots(sk, sv, sstate, dk, dv, dstate, ss, ds, n, None)
    return rc, lib.sfa_last_error().decode()


def test_refusals_of_ring_share_paged_slots():
    sk = lambda s=S, h=HKV, ns=NS, d=D, dt=torch.bfloat16: _d(s, h, ns, d, dtype=dt)
    ok = (sk(), sk(), sk(), sk())
    names = ("src_sink_k", "src_sink_v", "dst_sink_k", "dst_sink_v")
    for i, name in enumerate(names):
        assert _sh(*(None if j == i else t for j, t in enumerate(ok))) == (-1, f"{name}: null tensor descriptor")
    for kw, name in ((dict(sstate=None), "src_state"), (dict(dstate=None), "dst_state"), (dict(ss=None), "src_slots"),
                     (dict(ds=None), "dst_slots")):
        assert _sh(*ok, **kw) == (-1, f"{name}: null device pointer")
    assert _sh(*ok, n=-2) == (-1, "n_pairs must be >= 0 (got -2)")
    assert _sh(sk(), sk(), sk(d=128), sk(), n=0) == (0, "")
    assert _sh(sk(), sk(), sk(), sk(dt=torch.float16)) == (-1, "ring_share_slots: dst_sink_v and src_sink_k differ in dtype "
                                                               "(the four buffers must share one)")
    rc, err = _sh(sk(), sk(), sk(d=128), sk(d=128))
    assert rc == -1 and err == (f"ring_share_slots: dst_sink_k must be [S, H_kv, num_sink, D] = [S, {HKV}, {NS}, {D}] in both "
                                f"pools (got [{S}, {HKV}, {NS}, 128])")
    assert _sh(sk(), sk(S + 1), sk(), sk()) == (-1, f"pool: the src sink buffers must share shape[0] = S >= 1 (sink {S} / "
                                                    f"{S + 1})")
    assert _sh(sk(d=20), sk(d=20), sk(d=20), sk(d=20)) == (-1, "ring_share_slots: K/V rows must be a multiple of 16 bytes "
                                                               "(head dim 20)")
    odd = lambda: _d(S, HKV, NS, D + 4, view=lambda t: t[..., :D])
    assert _sh(odd(), odd(), odd(), odd()) == (-1, "ring_share_slots: rows of every tensor must be 16-byte aligned")


# ------------------------------------------------------------------------------------------------ the far case
def test_truncated_addresses_expose_the_far_pages_copy():
    """tests/test_gpu_page_share.py copies pages across 2^32 bytes of one arena: for its geometry every one of the three
    truncation errors of far_views puts some row of every copied page outside the arena or onto sentinel words."""
    import test_gpu_page_share as G
    n = G.ARENA_I16
    pp = F.page_pool(n, G.HKV * G.P * G.D_FAR, 2)
    pairs = G.far_pairs(pp)
    assert any(s < pp.p31 and d >= pp.p32 for s, d in pairs) and any(s >= pp.p32 and d < pp.p31 for s, d in pairs)
    pages = sorted({p for pr in pairs for p in pr})
    ops = {nm: F.slot_rows(s, pages) for nm, s in zip(("page_k", "page_v"), pp.specs(G.HKV, G.P, G.D_FAR))}
    ex = F.exposed(ops, 2, n)
    assert set(e for _, e in ex) == {"elem_i32", "byte_u32", "byte_i32"}
    for key, rows in ex.items():
        assert rows > 0, (key, "no row of this operand would show the error")
