"""Paged slot pool: prefill_slots, ragged_step_dyn, commit_packed_dyn and fork_slots on a pool whose ring lives in pages
[n_pages, H_kv, P, D] behind a device table (sfa_ring_fill_varlen_paged_slots, sfa_decode_ring_ragged_paged_slots,
sfa_ring_commit_path_ragged_paged_slots, sfa_ring_copy_paged_slots).  The contract is two bitwise equalities against the
TWIN, the contiguous pool tests/paged_ref.py::gather builds (include/sfa.h), so no test here has a tolerance of its own:

  read     o of a paged step is bit for bit o of the same call on the twin;
  storage  after a storing call on both pools every mapped page row equals the twin's ring slot, every row the contiguous
           call leaves alone keeps its bytes, pages mapped to no slot keep their bytes, sinks and state rows are equal.

Geometry of tests/test_gpu_ragged_tree.py: a pool of 8 slots, H_kv = 2, num_sink = 4, the slot fills of its _pool() (sink
not full, ring partly filled, filled exactly, wrapped) and 30 more tokens into the wrapped slots, so that write_pos = 37
lies inside the second page; (Wc, P) in (64, 32), (96, 32): a tile is a page.  Lengths [1, 7, 0, 16, 33, 64, 110] padded to
T = 240 with an inactive and an empty sequence; 110 > Wc + num_sink is the long admission.  The `walk` pack of
tests/packed_regime.py (H_kv 8, G 8, T 1024, Wc 320) runs at P = 64: two tiles per page, five pages, waves that walk
several tiles.  Tables are a seeded shuffle of the page pool, interleaved across the slots, and map only the prefix each
slot needs.  No test can pass empty: every page row that holds no live ring slot - pages no slot owns and the unused
rows of mapped pages - is NaN before every call, so a tile read from the wrong page puts NaN into o; every pool asserts
at least two table rows that are neither the identity nor monotone and a wrapped ring whose write_pos is no multiple of
P; every storing call asserts that it wrote rows."""
import pytest
import torch

import packed_regime as R
import paged_ref as PR
import test_gpu_packed_long as PL
import test_gpu_ragged_tree as RT
from sink_attention import SinkCacheLayer
from test_gpu_fp8_pool import CASES, _zero_rows
from test_gpu_ragged_tree import HKV, NS, S, _check_rows, _cu, _i32, _oracle, _pack, _parents, _run
from test_gpu_slots import _dev_slots, _path
from test_ragged_tree_host import binary, chain, comb, rand_tree, star
from util import DECODE_TOL, rand

pytestmark = pytest.mark.gpu
DEV = "cuda"
GEO = [(64, 32), (96, 32)]
GRID = [(dt, D, G, W, P) for dt, D, G in CASES for W, P in GEO]
LENGTHS = [1, 7, 0, 16, 33, 64, 110]
T_PAD = 240
FRESH = (6, 7)
PLAIN = [3, -1, 5, 2, 1, 0, 4]          # every named slot is prefilled; the 7-token sequence is inactive
ADMIT = [3, -1, 5, 2, 7, 4, 6]          # the sequences of 33 and 110 tokens on the fresh slots 7 and 6
MASK = [1, 1, 1, 0, 1, 0, 1]
SINKS = ("sink_k", "sink_v")
RING = ("window_k", "window_v")
INT_MAX = 2 ** 31 - 1


def _trees():
    return [chain(1), star(7), [], binary(16), rand_tree(33, 3), comb(64), star(110)]     # the last one is ignored: n > 64


def _bits(t):
    return t.view(torch.int16)


# ------------------------------------------------------------------ pools
def _base(dtype, D, W, seed, fresh=FRESH):
    """the contiguous pool of test_gpu_ragged_tree._pool, with 30 more tokens in the wrapped slots: write_pos = 37"""
    layer, hist = RT._pool(dtype, D, W, seed, fresh)
    wrapped = [s for s in range(S) if s % 4 == 3 and s not in fresh]
    g = torch.Generator().manual_seed(seed + 1000)
    kc, vc = rand((1, HKV, 30 * len(wrapped), D), g, dtype), rand((1, HKV, 30 * len(wrapped), D), g, dtype)
    layer.commit_packed_dyn(kc.to(DEV), vc.to(DEV), _i32(_cu([30] * len(wrapped))), _dev_slots(wrapped),
                            _i32([30] * len(wrapped)))
    for j, s in enumerate(wrapped):
        hist[s]["com"] = tuple(torch.cat([old, new[:, :, 30 * j:30 * j + 30]], dim=2) for old, new in zip(hist[s]["com"], (kc, vc)))
        assert layer._dev_state[s].tolist() == [NS, W, 37, NS + W + 4 + 7 + 30]
    return layer, hist


def _empty(dtype, D, W, S_=S, Hkv=HKV, ns=NS):
    layer = SinkCacheLayer(ns, W)
    layer.init_pool(S_, Hkv, D, dtype, DEV)
    return layer


def _contig(base):
    """a contiguous pooled copy of `base` (buffers and state)"""
    c = SinkCacheLayer(base.num_sink, base.window_size)
    for name in SINKS + RING:
        setattr(c, name, getattr(base, name).clone())
    c._dev_state = base._dev_state.clone()
    c.is_initialized = c.prefilled = c._per_seq = c._pool = True
    return c


def _ring_after(base, call):
    """window_len of every slot after `call` on a copy of the contiguous pool: what the prefix rule maps"""
    dry = _contig(base)
    call(dry)
    return dry._dev_state[:, 1].tolist()


def _table(S_, per, need, n_pages, seed, identity):
    """identity: slot s owns pages s * per + j.  Else a seeded shuffle of the page pool dealt out entry by entry across the
    slots (interleaved); the first seed from `seed` on that leaves two rows neither identity nor monotone."""
    if identity:
        return [[s * per + j if j < need[s] else -1 for j in range(per)] for s in range(S_)]
    for sd in range(seed, seed + 64):
        perm = torch.randperm(n_pages, generator=torch.Generator().manual_seed(sd)).tolist()
        tab = [[-1] * per for _ in range(S_)]
        it = iter(perm)
        for j in range(per):
            for s in range(S_):
                if j < need[s]:
                    tab[s][j] = next(it)
        if _scrambled(tab, per) >= 2:
            return tab
    raise AssertionError("no shuffle with two scrambled rows")


def _scrambled(tab, per):
    """rows that are neither the identity nor monotone"""
    n = 0
    for s, row in enumerate(tab):
        m = [e for e in row if e >= 0]
        n += len(m) >= 2 and m != sorted(m) and m != [s * per + j for j in range(len(m))]
    return n


def _paged(base, P, seed, after=None, extra=4, identity=False, wrap_check=True):
    """(paged pool, twin) holding what the contiguous pool `base` holds.  after[s]: the window_len slot s reaches in the
    coming call (default: what it holds); the first ceil(max(window_len, after) / P) entries of its row are mapped.  Every
    page row that holds no live ring slot is NaN; the twin's ring is gather(pages, table), so it holds the same NaN rows
    beyond each fill and zeros where no page is mapped."""
    W, dtype = base.window_size, base.sink_k.dtype
    S_, Hkv, _, D = base.sink_k.shape
    per = W // P
    st = base._dev_state.tolist()
    need = [PR.pages_needed(max(st[s][1], 0 if after is None else after[s]), W, P) for s in range(S_)]
    n_pages = S_ * per + extra
    tab = _table(S_, per, need, n_pages, seed, identity)
    assert identity or _scrambled(tab, per) >= 2, tab
    if wrap_check:
        wraps = [st[s][2] for s in range(S_) if st[s][1] == W and st[s][2] != 0]
        assert wraps and all(wp % P for wp in wraps), wraps
    pg = SinkCacheLayer(base.num_sink, W)
    pg.init_pool(S_, Hkv, D, dtype, DEV, page_size=P, num_pages=n_pages)
    assert pg.window_k.shape == (n_pages, Hkv, P, D) and bool((pg.page_table == -1).all())
    pg.page_table.copy_(torch.tensor(tab, dtype=torch.int32))
    pg._dev_state.copy_(base._dev_state)
    for name in SINKS:
        getattr(pg, name).copy_(getattr(base, name))
    for name in RING:
        pages = getattr(pg, name)
        pages.fill_(float("nan"))
        for s in range(S_):
            for j in range(need[s]):
                n = min(max(st[s][1] - j * P, 0), P)          # live rows of this page
                pages[tab[s][j], :, :n] = getattr(base, name)[s, :, j * P:j * P + n]
    tw = _contig(base)
    for name in RING:
        setattr(tw, name, PR.gather(getattr(pg, name), pg.page_table.cpu()))
    return pg, tw


def _snap(layer):
    d = {name: _bits(getattr(layer, name)).clone() for name in SINKS + RING}
    d["state"] = layer._dev_state.clone()
    return d


def _unmoved(layer, snap, what):
    for name in SINKS + RING:
        assert torch.equal(_bits(getattr(layer, name)), snap[name]), (what, name)
    assert torch.equal(layer._dev_state, snap["state"]), (what, "state")


def _stored(pg, tw, s_pg, s_tw, what):
    """the storage equality after one storing call on both pools; returns the number of rows the call wrote"""
    tab = pg.page_table.tolist()
    n_pages, P = pg.window_k.shape[0], pg.page_size
    rows = 0
    for name in RING:
        new, old = _bits(getattr(tw, name)), s_tw[name]
        exp = s_pg[name].clone()
        for s, row in enumerate(tab):
            for j, e in enumerate(row):
                if PR.mapped(e, n_pages):
                    sl = slice(j * P, (j + 1) * P)
                    changed = (new[s, :, sl] != old[s, :, sl]).any(dim=-1, keepdim=True)
                    exp[e] = torch.where(changed, new[s, :, sl], exp[e])
                    rows += int(changed.sum())
                    # a mapped page is the twin's ring, written rows and others alike
                    assert torch.equal(_bits(getattr(pg, name))[e], new[s, :, sl]), (what, name, "slot", s, "entry", j)
        got = _bits(getattr(pg, name))
        bad = (got != exp).any(dim=-1).nonzero()
        assert torch.equal(got, exp), (what, name, "rows (page, head, row)", bad[:4].tolist(), "of", len(bad))
    for name in SINKS:
        assert torch.equal(_bits(getattr(pg, name)), _bits(getattr(tw, name))), (what, name)
        rows += int((_bits(getattr(tw, name)) != s_tw[name]).any(dim=-1).sum())
    assert torch.equal(pg._dev_state, tw._dev_state), (what, pg._dev_state.tolist(), tw._dev_state.tolist())
    return rows


def _both(pg, tw, call, what, stores):
    """`call` on the paged pool and on its twin: the outputs, bitwise equal; the storage equality if it stores"""
    s_pg, s_tw = _snap(pg), _snap(tw)
    o_p = call(pg)
    path = _path()
    assert path.endswith("_paged"), (what, path)
    o_t = call(tw)
    assert _path() == path[:-len("_paged")], (what, _path(), path)
    if o_p is not None:
        assert not torch.isnan(o_p).any(), (what, "a tile came from a page that is not the slot's")
        diff = (o_p != o_t).any(dim=(0, 1, 3)).nonzero().flatten().tolist()
        assert torch.equal(o_p, o_t), (what, "packed rows", diff[:8])
    if stores:
        rows = _stored(pg, tw, s_pg, s_tw, what)
        print(what, "rows written", rows)
        assert rows > 0, what
    else:
        _unmoved(pg, s_pg, (what, "the pool must not move"))
    return o_p


# ------------------------------------------------------------------ 1. the step: read equality, and storage when it commits
@pytest.mark.parametrize("dtype,D,G,W,P", GRID)
def test_the_step_is_bitwise_the_step_on_the_twin(dtype, D, G, W, P):
    base, _ = _base(dtype, D, W, seed=201)
    q, k, v, sa = _pack(dtype, D, G, T_PAD, seed=202)
    cu, par = _cu(LENGTHS), _parents(LENGTHS, _trees(), T_PAD)
    # (slots, parent, commit_seq, admit, commit): plain, trees, per-sequence commit of a tree pack, the admitting form, commit
    forms = [(PLAIN, None, None, False, False), (PLAIN, par, None, False, False), (PLAIN, par, MASK, False, True),
             (ADMIT, None, None, True, True), (ADMIT, par, MASK, True, False), (PLAIN, None, None, False, True)]
    for n, (slots, parent, mask, admit, commit) in enumerate(forms):
        call = lambda p: _run(p, q, k, v, cu, slots, parent, commit_seq=mask, sa=sa, commit=commit, admit=admit)
        pg, tw = _paged(base, P, seed=210 + n, after=_ring_after(base, call))
        o = _both(pg, tw, call, ("form", n, dtype, D, W, P), stores=commit)
        path = _path()
        assert ("decode_tree_mfma_" if parent is not None else "decode_multi_mfma_") in path and \
            ("_admit" in path) == admit and ("_commit" in path) == commit, path
        _zero_rows(o, LENGTHS, slots)
        assert o[:, :, :cu[-1]].any()
        if admit and commit:        # the long admission: 110 tokens into slot 6, the ring full and wrapped at slot 0
            assert pg._dev_state[6].tolist() == [NS, W, 0, 110] and pg._dev_state[7].tolist() == [NS, 29, 29, 33]


# ------------------------------------------------------------------ 2. the storing calls
@pytest.mark.parametrize("dtype,D,G,W,P", GRID)
def test_prefill_and_packed_commit_store_what_the_twin_stores(dtype, D, G, W, P):
    g = torch.Generator().manual_seed(221)
    fills = [[2, 9, NS + W, NS + W + 40][s % 4] for s in range(S)]
    live = [s for s in range(S) if s not in FRESH]
    kp, vp = (rand((1, HKV, sum(fills[s] for s in live), D), g, dtype).to(DEV) for _ in range(2))
    def prefill(p):
        p.prefill_slots(kp, vp, _cu([fills[s] for s in live]), live)
    cur = _empty(dtype, D, W)
    pg, tw = _paged(cur, P, seed=222, after=_ring_after(cur, prefill), wrap_check=False)
    assert bool(torch.isnan(pg.window_k).all())                    # nothing is live yet: every page row is NaN
    _both(pg, tw, prefill, ("prefill_slots", dtype, D, W, P), stores=True)
    assert pg._dev_state[3].tolist() == [NS, W, 0, NS + W + 40]
    # the packed commit, with and without a path: counts beyond n_i, zero, negative; an inactive and an empty sequence
    lengths, slots, counts = [7, 7, 0, 7, 7, 7, 7], [3, -1, 5, 2, 1, 0, 4], [9, 7, 3, 7, 5, -2, 0]
    k2, v2 = (rand((1, HKV, 60, D), g, dtype).to(DEV) for _ in range(2))
    path = []
    for n in lengths:
        p_ = torch.randint(0, max(n, 1), (n,), generator=g).tolist()
        if n:
            p_[1], p_[2] = n + 3, -2                               # entries outside [0, n): clamped on the device
        path += p_
    path += [9] * (60 - len(path))
    for use_path in (True, False):
        commit = lambda p: p.commit_packed_dyn(k2, v2, _i32(_cu(lengths)), _dev_slots(slots), _i32(counts),
                                               path=_i32(path) if use_path else None)
        pg, tw = _paged(tw, P, seed=223 + use_path, after=_ring_after(tw, commit), wrap_check=use_path is False)
        _both(pg, tw, commit, ("commit_packed_dyn", "path", use_path, dtype, D, W, P), stores=True)
        assert _path() == "ring_commit_path_ragged_slots"          # the twin's call; _both has seen the paged name
    assert pg._dev_state[3].tolist() == [NS, W, 14, NS + W + 54]    # wrapped, write_pos inside the first page


@pytest.mark.parametrize("dtype,D,G,W,P", [(torch.bfloat16, 64, 8, 64, 32), (torch.float16, 80, 1, 96, 32),
                                           (torch.bfloat16, 96, 1, 96, 32), (torch.float16, 128, 8, 64, 32)])
def test_fork_slots_copies_through_both_tables_within_a_pool_and_between_two(dtype, D, G, W, P):
    base, _ = _base(dtype, D, W, seed=231)
    wl = base._dev_state[:, 1].tolist()
    fork = lambda p: p.fork_slots([3, 1], [6, 7])                  # a wrapped ring and a partly filled one
    after = list(wl)
    after[6], after[7] = wl[3], wl[1]                              # the caller maps the destination's pages first
    pg, tw = _paged(base, P, seed=232, after=after)
    _both(pg, tw, fork, ("fork in one pool", dtype, D, W, P), stores=True)
    assert pg._dev_state[6].tolist() == pg._dev_state[3].tolist() and pg._dev_state[7].tolist() == pg._dev_state[1].tolist()
    # into a second paged pool of another size and another shuffle
    after2 = [0] * S
    after2[0], after2[5], after2[2], after2[3] = wl[3], wl[1], W, W      # slots 2 and 3: mapped and empty
    other_pg, other_tw = _paged(_empty(dtype, D, W), P, seed=233, after=after2, extra=9, wrap_check=False)
    assert other_pg.window_k.shape[0] != pg.window_k.shape[0]
    s_pg, s_tw = _snap(other_pg), _snap(other_tw)
    other_pg.fork_slots([3, 7], [0, 5], source=pg)
    assert _path() == "ring_copy_slots_paged", _path()
    other_tw.fork_slots([3, 7], [0, 5], source=tw)
    assert _path() == "ring_copy_slots", _path()
    assert _stored(other_pg, other_tw, s_pg, s_tw, "fork between two pools") > 0
    with pytest.raises(ValueError, match="differ in (geometry|paging)"):
        pg.fork_slots([0], [1], source=base)
    # a step on the forks is bitwise the step on the sources
    lengths = [1, 7]
    q, k, v, sa = _pack(dtype, D, G, 8, seed=234)
    o_src = _run(pg, q, k, v, _cu(lengths), [3, 1], sa=sa).clone()
    assert not torch.isnan(o_src).any() and o_src.any()
    for pool, slots in ((pg, [6, 7]), (other_pg, [0, 5])):
        o = _run(pool, q, k, v, _cu(lengths), slots, sa=sa)
        assert _path().endswith("_paged") and torch.equal(o, o_src), slots


# ------------------------------------------------------------------ 3. the fp64 oracle (a sanity check: the contract is above)
@pytest.mark.parametrize("dtype,D,G,W,P", [(dt, D, G) + GEO[n % 2] for n, (dt, D, G) in enumerate(CASES)])
def test_the_oracle_over_the_history(dtype, D, G, W, P):
    base, hist = _base(dtype, D, W, seed=241)
    pg, _ = _paged(base, P, seed=242)
    q, k, v, sa = _pack(dtype, D, G, T_PAD, seed=243)
    trees = _trees()
    o = _run(pg, q, k, v, _cu(LENGTHS), PLAIN, _parents(LENGTHS, trees, T_PAD), sa=sa)
    assert _path().startswith("decode_tree_mfma_") and _path().endswith("_ragged_paged"), _path()
    ref = _oracle(q, k, v, sa, hist, W, LENGTHS, PLAIN, trees)
    assert len(ref) == sum(1 for n, s in zip(LENGTHS, PLAIN) if n and s >= 0)
    _check_rows(o, ref, LENGTHS, DECODE_TOL[dtype], ("paged pool", dtype, D, G, W, P))


# ------------------------------------------------------------------ 4. the table is only a map
@pytest.mark.parametrize("dtype,D,G,W,P", GRID[::3])
def test_a_shuffled_and_an_identity_table_give_the_same_bits(dtype, D, G, W, P):
    base, _ = _base(dtype, D, W, seed=251)
    q, k, v, sa = _pack(dtype, D, G, T_PAD, seed=252)
    par = _parents(LENGTHS, _trees(), T_PAD)
    shuf, _ = _paged(base, P, seed=253)
    ident, _ = _paged(base, P, seed=253, identity=True)
    assert shuf.page_table.tolist() != ident.page_table.tolist()
    for parent in (None, par):
        a = _run(shuf, q, k, v, _cu(LENGTHS), PLAIN, parent, sa=sa)
        b = _run(ident, q, k, v, _cu(LENGTHS), PLAIN, parent, sa=sa)
        assert not torch.isnan(a).any() and torch.equal(a, b)


def _move(pg, s, free):
    """move the pages of slot s to the pages `free` with torch copies, NaN what they leave, rewrite the row in place;
    returns the pages that are free now"""
    row = [e for e in pg.page_table[s].tolist() if e >= 0]
    ptr = pg.page_table.data_ptr()
    for old, new in zip(row, free):
        for name in RING:
            getattr(pg, name)[new].copy_(getattr(pg, name)[old])
            getattr(pg, name)[old].fill_(float("nan"))
    pg.page_table[s, :len(row)] = torch.tensor(free[:len(row)], dtype=torch.int32, device=DEV)
    assert pg.page_table.data_ptr() == ptr
    return row


@pytest.mark.parametrize("dtype,D,G,W,P", [(torch.bfloat16, 64, 8, 96, 32), (torch.float16, 128, 8, 64, 32)])
def test_moving_a_slot_to_other_pages_changes_no_bit_eagerly_and_from_one_captured_graph(dtype, D, G, W, P):
    base, _ = _base(dtype, D, W, seed=261)
    pg, _ = _paged(base, P, seed=262, extra=4)
    q, k, v, sa = _pack(dtype, D, G, T_PAD, seed=263)
    owned = {e for row in pg.page_table.tolist() for e in row if e >= 0}
    free = [e for e in range(pg.window_k.shape[0]) if e not in owned]
    assert len(free) >= W // P
    sq, sk, sv, sad = q.to(DEV), k.to(DEV), v.to(DEV), sa.to(DEV)
    scu, ssl = _i32(_cu(LENGTHS)), _dev_slots(PLAIN)
    so = torch.zeros_like(sq)
    step = lambda out: pg.ragged_step_dyn(sq, sk, sv, scu, ssl, s_aux=sad, out=out, commit=False)
    o1 = step(None).clone()
    assert not torch.isnan(o1).any()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):         # warm-up outside the capture (the workspace exists already)
        step(so)
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(so)
    so.zero_()
    graph.replay()
    assert torch.equal(so, o1)
    free = _move(pg, 3, free)               # slot 3: the wrapped ring, every page of its row
    assert torch.equal(step(None), o1), "eager, after the move"
    so.zero_()
    graph.replay()                          # the graph reads the table when it runs
    assert torch.equal(so, o1), "the captured graph, after the move"
    _move(pg, 3, free)                      # and back
    so.zero_()
    graph.replay()
    assert torch.equal(so, o1)


# ------------------------------------------------------------------ 5. unmapped entries: defined behaviour, exercised once each
@pytest.mark.parametrize("entry", [-1, "n_pages", INT_MAX])
def test_a_store_to_an_unmapped_page_is_dropped_and_the_state_row_still_advances(entry):
    dtype, D, W, P = torch.bfloat16, 64, 64, 32
    base, _ = _base(dtype, D, W, seed=271)
    pg, tw = _paged(base, P, seed=272)
    e = pg.window_k.shape[0] if entry == "n_pages" else entry
    assert pg._dev_state[2].tolist() == [NS, W, 0, NS + W]         # a full ring at write_pos 0: 7 tokens go to page entry 0
    pg.page_table[2, 0] = e
    g = torch.Generator().manual_seed(273)
    k, v = (rand((1, HKV, 7, D), g, dtype).to(DEV) for _ in range(2))
    before = _snap(pg)
    for p in (pg, tw):
        p.commit_packed_dyn(k, v, _i32([0, 7]), _dev_slots([2]), _i32([7]))
    assert _path() == "ring_commit_path_ragged_slots"
    for name in SINKS + RING:
        assert torch.equal(_bits(getattr(pg, name)), before[name]), (entry, name, "every page keeps its bytes")
    assert torch.equal(pg._dev_state, tw._dev_state) and pg._dev_state[2].tolist() == [NS, W, 7, NS + W + 7]
    assert not torch.equal(_bits(tw.window_k)[2], _bits(base.window_k)[2])         # the twin did store


# ------------------------------------------------------------------ 6. determinism
def test_two_runs_give_the_same_bits():
    dtype, D, G, W, P = torch.float16, 80, 1, 96, 32
    base, _ = _base(dtype, D, W, seed=281)
    q, k, v, sa = _pack(dtype, D, G, T_PAD, seed=282)
    par = _parents(LENGTHS, _trees(), T_PAD)
    call = lambda p: _run(p, q, k, v, _cu(LENGTHS), PLAIN, par, sa=sa, commit=True)
    after = _ring_after(base, call)
    a, _ = _paged(base, P, seed=283, after=after)
    b, _ = _paged(base, P, seed=283, after=after)
    o1 = _run(a, q, k, v, _cu(LENGTHS), PLAIN, par, sa=sa).clone()
    o2 = _run(a, q, k, v, _cu(LENGTHS), PLAIN, par, sa=sa)
    assert torch.equal(o1, o2)
    call(a), call(b)
    _unmoved(a, _snap(b), "two committing runs leave the same bytes")


# ------------------------------------------------------------------ 7. the walk pack: two tiles per page, multi-tile wave walks
@pytest.mark.parametrize("dt,D", [("bf16", 64), ("fp16", 128), ("bf16", 80), ("fp16", 96)])
def test_the_walk_pack_at_two_tiles_per_page(dt, D):
    P = 64
    inp = R.pack_inputs("walk", "randn", dt, D)
    case = inp["case"]
    assert (case["Hkv"], case["G"], case["T_PAD"], case["Wc"]) == (8, 8, 1024, 320)
    base = PL._pool(inp)
    for commit in (False, True):
        call = lambda p: PL._run(p, inp, commit=commit)
        pg, tw = _paged(base, P, seed=291 + commit, after=_ring_after(base, call))
        assert pg.page_table.shape[1] == 5
        PL._reaches(case, pg, case["T_PAD"])                    # the regime, from the paged pool's own state rows
        o = _both(pg, tw, call, ("walk", dt, D, "commit", commit), stores=commit)
        assert o.any()
