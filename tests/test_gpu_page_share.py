"""Paged pool: a fork that SHARES the source's ring pages (fork_slots(share=True): PageAllocator.share +
sfa_ring_share_paged_slots) and copies a page only before the first store into it (reserve_pages: sfa_pages_copy on every
layer of the table).  The yardstick is a TWIN pool: the same geometry and the same calls, but forked with share=False, the
copying fork.  Everything a reader of a slot can see must be equal bit for bit - o of every step, every state row, the
sinks, and the live rows of tests/paged_ref.py::gather of every slot's ring through its own table (rows beyond a slot's
fill are not compared: a copying fork leaves there what the destination held, a shared page what the source held).
Nothing here is a tolerance.

H_kv = 2, H_q = 4, num_sink = 4, P = 32, 6 slots, 24 pages; prompts of 3 tokens (empty ring), 9 (inside page 0), 44 (row 8
of page 1) and 68 (the ring ends on a page boundary) on Wc = 128, and 150 on Wc = 64 (wrapped: write_pos = 0).  The last
two tests call sfa_pages_copy through the C ABI: a strided view with sentinels around every page, and pages on both sides
of 2^32 bytes of one arena (tests/far_views.py)."""
from types import SimpleNamespace

import pytest
import torch

import far_views as F
import paged_ref as PR
from sink_attention import PageAllocator, SinkAttentionCache, SinkCacheLayer
from sink_attention import _native as N
from util import rand

pytestmark = pytest.mark.gpu
DEV = "cuda"
HKV, HQ, NS, P, S, NPG = 2, 4, 4, 32, 6, 24
FP8 = torch.float8_e4m3fn
TREE, PATH = [-1, 0, 0, 1, 2], [0, 2, 4]      # a draft tree of 5 nodes whose accepted path is root -> 2 -> 4
ARENA_I16 = (1 << 31) + (1 << 26)             # int16 elements: 4 GiB + 128 MiB, as tests/test_gpu_far_offsets.py
D_FAR = 128


def _bits(t):
    return t.view(torch.uint8) if t.element_size() == 1 else t.view(torch.int16)


# ------------------------------------------------------------------ a pool and the calls of a serving loop on it
def _mk(dtype, D, W=128, kv_dtype=None, layers=1, n_pages=NPG):
    """owner: what reserve_pages / fork_slots / free_pages are called on (the layer, or the cache of `layers` layers)"""
    if layers == 1:
        owner = SinkCacheLayer(NS, W)
        owner.init_pool(S, HKV, D, dtype, DEV, page_size=P, num_pages=n_pages, kv_dtype=kv_dtype)
        ls = [owner]
    else:
        owner = SinkAttentionCache(NS, W)
        for l in range(layers):
            owner.init_pool(S, HKV, D, dtype, DEV, layer_idx=l, page_size=P, num_pages=n_pages, kv_dtype=kv_dtype)
        ls = list(owner.layers)
    if kv_dtype is not None:
        for layer in ls:
            layer.set_kv_scale([0.5, 2.0], [4.0, 0.25])
    return SimpleNamespace(owner=owner, layers=ls, seen=[0] * S, dtype=dtype, D=D)


_DATA = {}


def _data(seed, n, D, dtype):
    """q [1, H_q, n, D], k / v [1, H_kv, n, D] and s_aux of one (seed, layer): made once, shared by a pool and its twin"""
    key = (seed, n, D, dtype)
    if key not in _DATA:
        g = torch.Generator().manual_seed(seed)
        _DATA[key] = tuple(t.to(DEV) for t in (rand((1, HQ, n, D), g, dtype), rand((1, HKV, n, D), g, dtype),
                                               rand((1, HKV, n, D), g, dtype), torch.randn(HQ, generator=g) * 0.5))
    return _DATA[key]


def _prefill(pool, slot, n, seed):
    pool.owner.reserve_pages([slot], n)
    for l, layer in enumerate(pool.layers):
        _q, k, v, _sa = _data(seed + 1000 * l, n, pool.D, pool.dtype)
        layer.prefill_slots(k, v, [0, n], [slot])
    pool.seen[slot] = n


def _fork(pool, src, dsts, share):
    if share:
        pool.owner.fork_slots([src] * len(dsts), dsts, share=True, tokens=pool.seen[src])
    else:
        pool.owner.reserve_pages(dsts, pool.seen[src])
        pool.owner.fork_slots([src] * len(dsts), dsts)
    for d in dsts:
        pool.seen[d] = pool.seen[src]


def _step(pool, seqs, seed, reserve_on=None):
    """one packed step: seqs = [(slot, n, kind)], kind "c": n tokens attended and committed (a decode row, a chunk), "t": a
    draft tree of n = 5 nodes verified with commit_seq 0, whose path PATH commit_packed_dyn stores afterwards.
    reserve_pages comes first (on `reserve_on`, default the owner).  Returns o of every layer."""
    slots, lens = [s for s, _, _ in seqs], [n for _, n, _ in seqs]
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    (reserve_on or pool.owner).reserve_pages(slots, [pool.seen[s] + n for s, n in zip(slots, lens)])
    parent, path = [], []
    for _, n, kind in seqs:
        assert kind == "c" or n == len(TREE)
        parent += TREE if kind == "t" else list(range(-1, n - 1))
        path += PATH + [0] * (n - len(PATH)) if kind == "t" else list(range(n))
    trees = [kind == "t" for _, _, kind in seqs]
    outs = []
    for l, layer in enumerate(pool.layers):
        q, k, v, sa = _data(seed + 1000 * l, cu[-1], pool.D, pool.dtype)
        outs.append(layer.ragged_step_dyn(q, k, v, cu, slots, s_aux=sa, parent=parent, commit_seq=[0 if t else 1 for t in trees]))
        if any(trees):
            layer.commit_packed_dyn(k, v, cu, slots, [len(PATH) if t else 0 for t in trees], path=path)
    for (s, n, kind) in seqs:
        pool.seen[s] += len(PATH) if kind == "t" else n
    return outs


def _same(a, b, what, outs=None):
    """everything a reader of pool a can see against pool b"""
    if outs is not None:
        for l, (oa, ob) in enumerate(zip(*outs)):
            assert not torch.isnan(oa.float()).any() and torch.equal(_bits(oa), _bits(ob)), (what, "o", "layer", l)
    for l, (la, lb) in enumerate(zip(a.layers, b.layers)):
        assert torch.equal(la._dev_state, lb._dev_state), (what, "state", l, la._dev_state.tolist(), lb._dev_state.tolist())
        assert la._dev_state[:, 3].tolist() == a.seen, (what, "the host's seen", a.seen)
        live = la._dev_state[:, 1].tolist()
        for name in ("sink_k", "sink_v"):
            assert torch.equal(_bits(getattr(la, name)), _bits(getattr(lb, name))), (what, name, l)
        for name in ("window_k", "window_v"):
            ra, rb = (PR.gather(_bits(getattr(x, name)), x.page_table.cpu()) for x in (la, lb))
            for s in range(S):
                assert torch.equal(ra[s, :, :live[s]], rb[s, :, :live[s]]), (what, name, "layer", l, "slot", s)


def _pair(dtype, D, **kw):
    return _mk(dtype, D, **kw), _mk(dtype, D, **kw)


def _script(sh, tw, prompt, seed, forks=(1, 2, 3)):
    """case 1: fork one prompt into three slots, then four packed steps that mix decode rows, a 40-token chunk and a draft
    tree; source and forks get different tokens; compared after every call"""
    for p, share in ((sh, True), (tw, False)):
        _prefill(p, 0, prompt, seed)
        _fork(p, 0, list(forks), share)
    _same(sh, tw, "after the fork")
    a, b, c = forks
    steps = [[(0, 1, "c"), (a, 1, "c"), (b, 1, "c"), (c, 1, "c")],
             [(a, 40, "c"), (0, 1, "c"), (b, 5, "t")],
             [(c, 40, "c"), (b, 1, "c"), (a, 5, "t"), (0, 5, "t")],
             [(0, 1, "c"), (c, 1, "c"), (a, 1, "c"), (b, 1, "c")]]
    for i, seqs in enumerate(steps):
        outs = _step(sh, seqs, seed + 1 + i), _step(tw, seqs, seed + 1 + i)
        _same(sh, tw, f"prompt {prompt}, step {i}", outs)


# ------------------------------------------------------------------ 1. the serving loop against the copying twin
@pytest.mark.parametrize("dtype,D,prompt", [(torch.bfloat16, 64, 3), (torch.bfloat16, 80, 9), (torch.bfloat16, 64, 44),
                                            (torch.float16, 80, 44), (torch.bfloat16, 80, 68)])
def test_a_shared_fork_is_bitwise_the_copying_fork_over_a_serving_loop(dtype, D, prompt):
    sh, tw = _pair(dtype, D)
    _script(sh, tw, prompt, seed=100 + prompt)
    assert N.last_path().startswith("decode_") and "paged" in N.last_path()


# ------------------------------------------------------------------ 2. sharing is real
@pytest.mark.parametrize("prompt", [44, 68, 100])
def test_the_fork_aliases_pages_and_the_first_step_copies_what_the_host_rule_names(prompt):
    sh = _mk(torch.bfloat16, 64)
    _prefill(sh, 0, prompt, seed=200)
    al = sh.owner._pages
    free, row = list(al.free_list), sh.owner.page_table[0].tolist()
    ring_before = {n: _bits(getattr(sh.owner, n)).clone() for n in ("window_k", "window_v")}
    _fork(sh, 0, [1, 2, 3], share=True)
    assert N.last_path() == "ring_share_slots_paged"
    assert sh.owner.page_table[:4].tolist() == [row] * 4 and al.free_list == free        # rows alias, nothing was popped
    for n, old in ring_before.items():
        assert torch.equal(_bits(getattr(sh.owner, n)), old), "the fork moved ring bytes"
    # the host rule, replayed on a CPU table: the same calls must give the same table
    host = PageAllocator(torch.full((S, 128 // P), -1, dtype=torch.int32), NPG, P, 128)
    host.reserve([0], prompt)
    host.share([0] * 3, [1, 2, 3], max(prompt - NS, 0))
    want = host.reserve([0, 1, 2, 3], prompt + 1)
    _step(sh, [(s, 1, "c") for s in range(4)], seed=201)
    assert N.last_path().startswith("decode_")
    assert sh.owner.page_table.cpu().tolist() == host.table.tolist() and al.rows == host.rows and al.refcount == host.refcount
    first_written = (prompt - NS) // P                     # the page ring position prompt - num_sink lies in
    full = row[:first_written]
    assert len(want) == 3 * sum(1 for j, e in enumerate(row) if e >= 0 and j >= first_written)
    tab = sh.owner.page_table.tolist()
    for j, e in enumerate(full):                          # the untouched full pages: one page id in all four rows
        assert [tab[s][j] for s in range(4)] == [e] * 4 and al.refcount[e] == 4
    for j in range(first_written, len([e for e in row if e >= 0])):
        assert len({tab[s][j] for s in range(4)}) == 4     # what a step stores into is each slot's own
    assert al.pool_bytes(HKV, 64, 2) == 2 * len({e for r in tab for e in r if e >= 0}) * HKV * P * 64 * 2


# ------------------------------------------------------------------ 3. a wrapped ring
def test_a_wrapped_ring_makes_every_entry_private_and_equals_the_twin():
    """Wc = 64, a prompt of 150 tokens: write_pos = 0 with a token count that is 18 modulo Wc; the first reserve makes every
    entry private, and three steps that wrap again equal the twin"""
    sh, tw = _pair(torch.bfloat16, 64, W=64)
    for p, share in ((sh, True), (tw, False)):
        _prefill(p, 0, 150, seed=300)
        _fork(p, 0, [1, 2], share)
    assert sh.owner._dev_state[0].tolist() == [NS, 64, 0, 150]
    _same(sh, tw, "after the fork")
    al = sh.owner._pages
    assert al.rows[0] == al.rows[1] == al.rows[2] and len(al.rows[0]) == 2
    steps = [[(0, 1, "c"), (1, 1, "c"), (2, 1, "c")], [(1, 40, "c"), (2, 5, "t"), (0, 1, "c")],
             [(2, 40, "c"), (1, 40, "c"), (0, 40, "c")]]
    for i, seqs in enumerate(steps):
        outs = _step(sh, seqs, 301 + i), _step(tw, seqs, 301 + i)
        if i == 0:
            assert len({e for s in range(3) for e in al.rows[s]}) == 6 and max(al.refcount) == 1
        _same(sh, tw, f"wrapped, step {i}", outs)
    assert sh.owner._dev_state[1].tolist() == [NS, 64, 81 % 64, 231]


# ------------------------------------------------------------------ 4. FP8 pages
def test_a_shared_fork_of_a_paged_fp8_pool_is_its_copy_forked_twin():
    sh, tw = _pair(torch.bfloat16, 64, kv_dtype=FP8)
    assert sh.owner.window_k.dtype == FP8 and sh.owner.kv_scale.tolist() == [[0.5, 2.0], [4.0, 0.25]]
    _script(sh, tw, 44, seed=400)
    assert N.last_path().endswith("_paged_kvfp8")


# ------------------------------------------------------------------ 5. forks of forks, the first source retired
def test_forks_of_forks_survive_the_first_source():
    sh, tw = _pair(torch.bfloat16, 64)
    p, a, b = 2, 4, 1
    for pool, share in ((sh, True), (tw, False)):
        _prefill(pool, p, 44, seed=500)
        _fork(pool, p, [a], share)
        _step(pool, [(a, 1, "c"), (p, 1, "c")], 501)
        _fork(pool, a, [b], share)
    _same(sh, tw, "a from p, b from a")
    al = sh.owner._pages
    assert al.refcount[al.rows[p][0]] == 3 and al.rows[a] == al.rows[b]
    for pool in (sh, tw):
        pool.owner.release_slots([p])
        pool.owner.free_pages([p])
        pool.seen[p] = 0
    assert al.refcount[al.rows[a][0]] == 2 and al.rows[p] == []
    for i, seqs in enumerate([[(a, 1, "c"), (b, 1, "c")], [(b, 40, "c"), (a, 5, "t")], [(a, 1, "c"), (b, 1, "c")]]):
        outs = _step(sh, seqs, 502 + i), _step(tw, seqs, 502 + i)
        _same(sh, tw, f"p freed, step {i}", outs)


# ------------------------------------------------------------------ 6. every layer of the table
@pytest.mark.parametrize("on_layer0", [False, True], ids=["cache.reserve_pages", "layer0.reserve_pages"])
def test_the_copies_run_on_every_layer_of_the_table(on_layer0):
    sh, tw = _pair(torch.bfloat16, 64, layers=2)
    for pool, share in ((sh, True), (tw, False)):
        _prefill(pool, 0, 44, seed=600)
        _fork(pool, 0, [1, 2], share)
    assert not torch.equal(sh.layers[0].window_k, sh.layers[1].window_k)          # different K / V per layer
    assert sh.layers[0].page_table is sh.layers[1].page_table and len(sh.owner._pages.layers) == 2
    _same(sh, tw, "after the fork")
    for i, seqs in enumerate([[(0, 1, "c"), (1, 1, "c"), (2, 1, "c")], [(1, 40, "c"), (2, 5, "t"), (0, 1, "c")]]):
        outs = _step(sh, seqs, 601 + i, reserve_on=sh.layers[0] if on_layer0 else None), _step(tw, seqs, 601 + i)
        _same(sh, tw, f"two layers, step {i}", outs)


# ------------------------------------------------------------------ 7. a captured step around a copying reserve
def test_one_captured_step_replays_before_and_after_a_reserve_that_copied():
    dtype, D = torch.bfloat16, 64
    sh, tw = _pair(dtype, D)
    for pool in (sh, tw):
        _prefill(pool, 0, 44, seed=700)
    L = sh.owner
    q, k, v, sa = (t.clone() for t in _data(701, 2, D, dtype))
    cu, slots = torch.tensor([0, 1, 2], dtype=torch.int32, device=DEV), torch.tensor([0, -1], dtype=torch.int32, device=DEV)
    out = torch.zeros_like(q)
    step = lambda: L.ragged_step_dyn(q, k, v, cu, slots, s_aux=sa, out=out)

    def feed(seed, live):
        for dst, src in zip((q, k, v), _data(seed, 2, D, dtype)):
            dst.copy_(src)
        slots.copy_(torch.tensor(live, dtype=torch.int32))

    def twin(seed, live):
        tq, tk, tv, _ = _data(seed, 2, D, dtype)
        tw.owner.reserve_pages([s for s in live if s >= 0], [tw.seen[s] + 1 for s in live if s >= 0])
        o = tw.owner.ragged_step_dyn(tq, tk, tv, [0, 1, 2], live, s_aux=sa)
        for s in live:
            if s >= 0:
                tw.seen[s] += 1
        return o

    def mine(seed, live, run):
        feed(seed, live)
        L.reserve_pages([s for s in live if s >= 0], [sh.seen[s] + 1 for s in live if s >= 0])
        run()
        for s in live:
            if s >= 0:
                sh.seen[s] += 1
        return out.clone()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):             # the warm-up is a step of its own: it commits a token of slot 0
        feed(701, [0, -1])
        L.reserve_pages([0], 45)
        step()
        sh.seen[0] += 1
    torch.cuda.current_stream().wait_stream(side)
    _same(sh, tw, "warm-up", ([out.clone()], [twin(701, [0, -1])]))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    _same(sh, tw, "replay before the fork", ([mine(702, [0, -1], graph.replay)], [twin(702, [0, -1])]))
    _fork(sh, 0, [1], share=True)
    _fork(tw, 0, [1], share=False)
    al = L._pages
    shared = list(al.rows[0])
    o = mine(703, [0, 1], graph.replay)       # its reserve_pages copies page 1 for the first writer
    assert al.rows[0][1] != al.rows[1][1] and al.rows[0][0] == al.rows[1][0] == shared[0]
    _same(sh, tw, "replay after a reserve that copied", ([o], [twin(703, [0, 1])]))
    _same(sh, tw, "and once more", ([mine(704, [0, 1], graph.replay)], [twin(704, [0, 1])]))


# ------------------------------------------------------------------ 8. sfa_pages_copy through the C ABI
def _pages_copy(wk, wv, src, dst):
    s, d = (torch.tensor(x, dtype=torch.int32, device=DEV) for x in (src, dst))
    rc = N.lib().sfa_pages_copy(N.desc(wk), N.desc(wv), s.data_ptr(), d.data_ptr(), len(src), N.stream_ptr(wk.device))
    N.check(rc, "sfa_pages_copy")
    torch.cuda.synchronize()
    assert N.last_path() == "pages_copy"


@pytest.mark.parametrize("dtype", [torch.bfloat16, FP8], ids=["bf16", "fp8"])
def test_pages_copy_moves_whole_pages_and_nothing_else(dtype):
    """D = 80 (rows of 160 / 80 bytes), Hkv = 3 and a page buffer that is a strided view: 5 spare rows behind every head
    (head stride (P + 5) D > P D) and a spare head behind every page, all holding a sentinel.  Five pairs: three live,
    one with a -1, one with src == dst (and an entry == n_pages behaves as the -1)."""
    D, Hkv, n = 80, 3, 9
    g = torch.Generator().manual_seed(800)
    es = 1 if dtype == FP8 else 2
    base = [torch.full((n, Hkv + 1, P + 5, D * es), 0x5A, dtype=torch.uint8, device=DEV) for _ in range(2)]
    views = [b.view(dtype)[:, :Hkv, :P] for b in base]
    assert views[0].shape == (n, Hkv, P, D) and views[0].stride(1) == (P + 5) * D > P * D
    for vw in views:
        vw.view(torch.uint8).copy_(torch.randint(0, 256, (n, Hkv, P, D * es), generator=g, dtype=torch.uint8))
    want = [b.clone() for b in base]
    src, dst = [0, 1, -1, 3, 2], [5, 6, 7, 3, 8]
    for w in want:
        for s, d in ((0, 5), (1, 6), (2, 8)):
            w[d, :Hkv, :P] = w[s, :Hkv, :P]
    _pages_copy(views[0], views[1], src, dst)
    for b, w, name in zip(base, want, "KV"):
        assert torch.equal(b, w), (name, (b != w).nonzero()[:4].tolist())
    assert not torch.equal(base[0], base[1])
    before = [b.clone() for b in base]
    _pages_copy(views[0], views[1], [n, 4, -1], [4, n, 2 ** 31 - 1])          # nothing is live
    assert torch.equal(base[0], before[0]) and torch.equal(base[1], before[1])


# ------------------------------------------------------------------ 9. pages on both sides of 2^32 bytes
def far_pairs(pp):
    """(src, dst) over the picks of a far_views.PagePool: near to far, far to near, the band in between on either side;
    no destination twice, no destination that is a source"""
    lo, mid, hi = ([p for p in pp.picks if a <= p < b] for a, b in ((0, pp.p31), (pp.p31, pp.p32), (pp.p32, pp.n_pages)))
    return [(lo[0], hi[0]), (hi[1], lo[1]), (mid[0], hi[2]), (lo[2], mid[2])]


def test_pages_copy_across_four_gib_of_one_arena():
    need = ARENA_I16 * 2
    free, total = torch.cuda.mem_get_info()
    if free < need + (2 << 30):
        pytest.skip(f"far-offset arena needs {need / 2**30:.2f} + 2 GiB free, the device reports {free / 2**30:.2f} of "
                    f"{total / 2**30:.2f} GiB")
    arena = torch.empty(ARENA_I16, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    F.fill_sentinel(arena)
    pp = F.page_pool(arena.numel(), HKV * P * D_FAR, 2)
    pages = [F.far_view(arena, sp.shape, sp.strides, sp.offset) for sp in pp.specs(HKV, P, D_FAR)]
    pairs = far_pairs(pp)
    used = sorted({p for pr in pairs for p in pr})
    rank = {p: i for i, p in enumerate(used)}
    assert pages[0][pairs[0][1]].data_ptr() - arena.data_ptr() >= F.TWO32 > pages[1][pairs[0][0]].data_ptr() - arena.data_ptr()
    g = torch.Generator().manual_seed(900)
    near = [rand((len(used), HKV, P, D_FAR), g, torch.bfloat16).to(DEV) for _ in range(2)]      # the contiguous twin
    for buf, nr in zip(pages, near):
        for p in used:
            buf[p].copy_(nr[rank[p]])
    _pages_copy(near[0], near[1], [rank[s] for s, _ in pairs], [rank[d] for _, d in pairs])
    _pages_copy(pages[0], pages[1], [s for s, _ in pairs], [d for _, d in pairs])
    for buf, nr, name in zip(pages, near, "KV"):
        for s, d in pairs:
            assert torch.equal(_bits(buf[d]), _bits(nr[rank[d]])) and torch.equal(_bits(buf[d]), _bits(buf[s])), (name, s, d)
        for p in used:
            assert torch.equal(_bits(buf[p]), _bits(nr[rank[p]])), (name, p)
    F.assert_untouched(arena, [buf[p] for buf in pages for p in used], "pages_copy far")
    del arena, pages
    torch.cuda.empty_cache()
