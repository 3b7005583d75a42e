"""Paged FP8 (e4m3) slot pool: prefill_slots, ragged_step_dyn, commit_packed_dyn and fork_slots on a pool whose ring lives
in FP8 pages [n_pages, H_kv, P, D] behind a device table (sfa_ring_fill_varlen_paged_fp8_slots,
sfa_decode_ring_ragged_paged_fp8_slots, sfa_ring_commit_path_ragged_paged_fp8_slots, sfa_ring_copy_paged_slots on FP8
buffers).  The pool composes the FP8 pool and the paged pool, and the contract (include/sfa.h) is four bitwise
equalities, so no test here has a tolerance of its own (the oracle test uses the existing DECODE_TOL):

  read 1   o equals o of the same step on the contiguous FP8 twin gather(pages8, table): same sinks, state, scales;
  read 2   o equals o of the same step on a 16-bit paged pool with the same table holding dequant(codes, scale, T);
  storage  every mapped page row holds quant(the row the same call writes into that 16-bit paged pool); every other
           byte of the page buffers keeps its value, pages mapped to no slot included; stores to unmapped pages are
           dropped; the sinks hold the FP8 twin's bytes; the state rows of the three pools are equal;
  copy     after fork_slots every later call on the destination is bitwise the call on the source.

Geometry of tests/test_gpu_paged_pool.py: 8 slots, H_kv 2, num_sink 4, the fills of its _base (sink not full, ring partly
filled, filled exactly, wrapped with write_pos = 37 inside the second page), (Wc, P) in (64, 32) and (96, 32), the four
(dtype, D, G) of test_gpu_fp8_pool.CASES, lengths [1, 7, 0, 16, 33, 64, 110]; the `walk` pack of tests/packed_regime.py at
P = 64.  Scales differ per head and between K and V (a power of two and a non-power each), so a K / V swap or another
head's scale fails.

No test can pass empty, and a wrong address fails instead of faulting: every page row that holds no live ring slot is
0x7F (NaN in e4m3fn) before every call, and every page buffer is the FIRST HALF of an allocation twice its size whose
second half is 0x7F and is asserted untouched after every call - a page offset taken at two bytes per element lands
there, in bytes this file owns, and shows as NaN in o or as a changed guard byte.  Every storing call asserts that it
wrote rows."""
import pytest
import torch

import packed_regime as R
import paged_ref as PR
import test_gpu_packed_long as PL
import test_gpu_paged_pool as PP
from fp8_ref import FP8, dequant, quant
from sink_attention import SinkCacheLayer
from test_gpu_fp8_pool import CASES, SCALES, _clone, _row, _zero_rows
from test_gpu_paged_pool import ADMIT, FRESH, GEO, INT_MAX, LENGTHS, MASK, PLAIN, RING, SINKS, T_PAD, _trees
from test_gpu_ragged_tree import HKV, NS, S, _check_rows, _cu, _i32, _oracle, _pack, _parents, _run
from test_gpu_slots import BUFS, _dev_slots, _path
from util import DECODE_TOL, rand

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN8 = 0x7F
GRID = [(dt, D, G, W, P, SCALES) for dt, D, G in CASES for W, P in GEO] + [(torch.bfloat16, 64, 8, 96, 32, None)]
TAIL = "_paged_kvfp8"


def _u8(t):
    return t.view(torch.uint8)


def _ints(t):
    return t.view(torch.uint8) if t.dtype == FP8 else t.view(torch.int16)


def _put(dst, codes):
    """FP8 codes into an FP8 buffer of the same shape, as bytes"""
    _u8(dst).copy_(_u8(codes.contiguous()).to(dst.device))


# ------------------------------------------------------------------ pools
def _fp8_layer(S_, Hkv, D, W, ns, act, scales):
    """an empty contiguous FP8 pool, spelled with the keyword"""
    b8 = SinkCacheLayer(ns, W)
    b8.init_pool(S_, Hkv, D, act, DEV, kv_dtype=FP8)
    assert b8.window_k.dtype == FP8 and b8.window_k.shape == (S_, Hkv, W, D) and b8.page_size is None
    if scales is not None:
        b8.set_kv_scale(*scales)
    return b8


def _base8(dtype, D, W, seed, scales, fresh=FRESH):
    """The contiguous FP8 pool holding quant(the 16-bit pool of test_gpu_paged_pool._base) - what the FP8 storing calls
    leave for that history (tests/test_gpu_fp8_pool.py) - and the history as it reads back."""
    base16, hist = PP._base(dtype, D, W, seed, fresh)
    b8 = _fp8_layer(S, HKV, D, W, NS, dtype, scales)
    for name in BUFS:
        _put(getattr(b8, name), quant(getattr(base16, name).cpu(), _row(scales, name)))
    b8._dev_state.copy_(base16._dev_state)
    dq = lambda kv: tuple(dequant(quant(x, _row(scales, n)), _row(scales, n), dtype) for x, n in zip(kv, ("_k", "_v")))
    return b8, {s: dict(pre=dq(h["pre"]), com=dq(h["com"])) for s, h in hist.items()}


def _ring_after(base8, call):
    dry = _clone(base8)
    call(dry)
    return dry._dev_state[:, 1].tolist()


def _twin(pg):
    """the contiguous FP8 twin of a paged FP8 pool as it stands: gather(pages8, table), the same sinks, state and scales"""
    tw = SinkCacheLayer(pg.num_sink, pg.window_size)
    for name in SINKS:
        setattr(tw, name, getattr(pg, name).clone())
    for name in RING:
        setattr(tw, name, PR.gather(_u8(getattr(pg, name)), pg.page_table.cpu()).view(FP8))
    tw._dev_state = pg._dev_state.clone()
    tw.kv_scale = pg.kv_scale.clone()
    tw.is_initialized = tw.prefilled = tw._per_seq = tw._pool = True
    return tw


def _paged8(base8, act, P, seed, after=None, extra=4, wrap_check=True):
    """(paged FP8 pool, its contiguous FP8 twin) holding what the contiguous FP8 pool `base8` holds.  after[s]: the
    window_len slot s reaches in the coming call; that prefix of its table row is mapped (a seeded shuffle).  Every page
    row without a live ring slot is 0x7F, and each page buffer is the first half of a guard allocation of 0x7F."""
    W = base8.window_size
    S_, Hkv, ns, D = base8.sink_k.shape
    per = W // P
    st = base8._dev_state.tolist()
    need = [PR.pages_needed(max(st[s][1], 0 if after is None else after[s]), W, P) for s in range(S_)]
    n_pages = S_ * per + extra
    tab = PP._table(S_, per, need, n_pages, seed, False)
    assert PP._scrambled(tab, per) >= 2, tab                       # two rows neither identity nor monotone
    if wrap_check:
        wraps = [st[s][2] for s in range(S_) if st[s][1] == W and st[s][2] != 0]
        assert wraps and all(wp % P for wp in wraps), wraps         # a wrapped ring, write_pos no multiple of P
    pg = SinkCacheLayer(ns, W)
    pg.init_pool(S_, Hkv, D, act, DEV, page_size=P, num_pages=n_pages, kv_dtype=FP8)
    assert pg.window_k.shape == (n_pages, Hkv, P, D) and pg.window_k.dtype == pg.sink_k.dtype == FP8
    assert pg.kv_scale.shape == (2, Hkv) and bool((pg.page_table == -1).all())
    pg.kv_scale.copy_(base8.kv_scale)
    pg.page_table.copy_(torch.tensor(tab, dtype=torch.int32))
    pg._dev_state.copy_(base8._dev_state)
    pg._guard = {}
    for name in SINKS:
        _put(getattr(pg, name), getattr(base8, name))
    for name in RING:
        big = torch.full((2 * n_pages, Hkv, P, D), NAN8, dtype=torch.uint8, device=DEV)
        pg._guard[name] = big
        setattr(pg, name, big[:n_pages].view(FP8))
        pages, src = big[:n_pages], _u8(getattr(base8, name))
        for s in range(S_):
            for j in range(need[s]):
                n = min(max(st[s][1] - j * P, 0), P)               # live rows of this page
                pages[tab[s][j], :, :n] = src[s, :, j * P:j * P + n]
        assert getattr(pg, name).data_ptr() == big.data_ptr() and getattr(pg, name).is_contiguous()
    return pg, _twin(pg)


def _deq_paged(pg, act, scales):
    """the 16-bit paged pool of read 2 and of the storage equality: the same table and state, pages and sinks holding
    dequant(codes, scale, act) (0x7F reads as NaN there too)"""
    n_pages, Hkv, P, D = pg.window_k.shape
    p = SinkCacheLayer(pg.num_sink, pg.window_size)
    p.init_pool(pg.num_slots, Hkv, D, act, DEV, page_size=P, num_pages=n_pages)
    p.page_table.copy_(pg.page_table)
    p._dev_state.copy_(pg._dev_state)
    for name in BUFS:
        getattr(p, name).copy_(dequant(getattr(pg, name).cpu(), _row(scales, name), act).to(DEV))
    return p


def _guard_ok(pg, what):
    for name, big in pg._guard.items():
        n = big.shape[0] // 2
        assert getattr(pg, name).data_ptr() == big.data_ptr(), (what, name)
        assert bool((big[n:] == NAN8).all()), (what, name, "bytes behind the page buffer changed: a page offset at 2 bytes "
                                               "per element?")


def _snap(layer):
    d = {name: _ints(getattr(layer, name)).clone() for name in BUFS}
    d["state"] = layer._dev_state.clone()
    return d


def _unmoved(layer, snap, what):
    for name in BUFS:
        assert torch.equal(_ints(getattr(layer, name)), snap[name]), (what, name)
    assert torch.equal(layer._dev_state, snap["state"]), (what, "state")


def _stored_vs_twin(pg, tw, s_pg, s_tw, what):
    """after one storing call on the paged FP8 pool and on its contiguous FP8 twin: every mapped page is the twin's ring
    slot, every page row the twin's call left alone keeps its bytes (pages mapped to no slot too), sinks and state rows are
    equal.  Returns the number of rows written."""
    tab = pg.page_table.tolist()
    n_pages, P = pg.window_k.shape[0], pg.page_size
    rows = 0
    for name in RING:
        new, old, got = _u8(getattr(tw, name)), s_tw[name], _u8(getattr(pg, name))
        exp = s_pg[name].clone()
        for s, row in enumerate(tab):
            for j, e in enumerate(row):
                if PR.mapped(e, n_pages):
                    sl = slice(j * P, (j + 1) * P)
                    changed = (new[s, :, sl] != old[s, :, sl]).any(dim=-1, keepdim=True)
                    exp[e] = torch.where(changed, new[s, :, sl], exp[e])
                    rows += int(changed.sum())
                    assert torch.equal(got[e], new[s, :, sl]), (what, name, "slot", s, "entry", j)
        bad = (got != exp).any(dim=-1).nonzero()
        assert torch.equal(got, exp), (what, name, "rows (page, head, row)", bad[:4].tolist(), "of", len(bad))
    for name in SINKS:
        assert torch.equal(_u8(getattr(pg, name)), _u8(getattr(tw, name))), (what, name)
        rows += int((_u8(getattr(tw, name)) != s_tw[name]).any(dim=-1).sum())
    assert torch.equal(pg._dev_state, tw._dev_state), (what, pg._dev_state.tolist(), tw._dev_state.tolist())
    return rows


def _stored_vs_16(pg, p16, s_pg, s_16, scales, what):
    """... and on the 16-bit paged pool: every row that call wrote there is, in the FP8 pool, its quant; every other byte
    of the FP8 buffers is the snapshot's"""
    rows = 0
    for name in BUFS:
        new16 = getattr(p16, name)
        changed = (_ints(new16) != s_16[name]).any(dim=-1, keepdim=True)
        want = _u8(quant(new16.cpu(), _row(scales, name))).to(DEV)
        exp = torch.where(changed, want, s_pg[name])
        got = _u8(getattr(pg, name))
        bad = (got != exp).any(dim=-1).nonzero()
        assert torch.equal(got, exp), (what, name, "vs quant(16-bit paged), rows", bad[:4].tolist(), "of", len(bad))
        rows += int(changed.sum())
    assert torch.equal(pg._dev_state, p16._dev_state), (what, pg._dev_state.tolist(), p16._dev_state.tolist())
    return rows


def _three(pg, tw, act, scales, call, what, stores):
    """`call` on the paged FP8 pool, on its contiguous FP8 twin and on the 16-bit paged pool of its dequantised codes: the
    three outputs bitwise equal, the three names, the guard, and the storage equalities if it stores"""
    p16 = _deq_paged(pg, act, scales)
    s_pg, s_tw, s_16 = _snap(pg), _snap(tw), _snap(p16)
    o = call(pg)
    path = _path()
    assert path.endswith(TAIL), (what, path)
    stem = path[:-len(TAIL)]
    o_t = call(tw)
    assert _path() == stem + "_kvfp8", (what, _path(), path)
    o_16 = call(p16)
    assert _path() == stem + "_paged", (what, _path(), path)
    _guard_ok(pg, what)
    if o is not None:
        assert not torch.isnan(o).any(), (what, "a tile came from bytes that are no live row of the slot")
        for other, name in ((o_t, "the contiguous FP8 twin"), (o_16, "the 16-bit paged pool")):
            diff = (o != other).any(dim=(0, 1, 3)).nonzero().flatten().tolist()
            assert torch.equal(o, other), (what, name, "packed rows", diff[:8])
    if stores:
        rows = _stored_vs_twin(pg, tw, s_pg, s_tw, what)
        rows16 = _stored_vs_16(pg, p16, s_pg, s_16, scales, what)
        print(what, "rows written", rows, rows16)
        assert rows > 0 and rows16 == rows, (what, rows, rows16)
    else:
        _unmoved(pg, s_pg, (what, "the pool must not move"))
    return o


# ------------------------------------------------------------------ 1. the step: both read equalities, storage when it commits
@pytest.mark.parametrize("dtype,D,G,W,P,scales", GRID)
def test_the_step_is_bitwise_the_step_on_both_twins(dtype, D, G, W, P, scales):
    base8, _ = _base8(dtype, D, W, 301, scales)
    q, k, v, sa = _pack(dtype, D, G, T_PAD, seed=302)
    cu, par = _cu(LENGTHS), _parents(LENGTHS, _trees(), T_PAD)
    # (slots, parent, commit_seq, admit, commit): plain, trees, per-sequence commit of a tree pack, the admitting form
    # (the 110-token admission included), trees + admission, commit
    forms = [(PLAIN, None, None, False, False), (PLAIN, par, None, False, False), (PLAIN, par, MASK, False, True),
             (ADMIT, None, None, True, True), (ADMIT, par, MASK, True, False), (PLAIN, None, None, False, True)]
    for n, (slots, parent, mask, admit, commit) in enumerate(forms):
        call = lambda p: _run(p, q, k, v, cu, slots, parent, commit_seq=mask, sa=sa, commit=commit, admit=admit)
        pg, tw = _paged8(base8, dtype, P, seed=310 + n, after=_ring_after(base8, call))
        o = _three(pg, tw, dtype, scales, call, ("form", n, dtype, D, W, P), stores=commit)
        assert o[:, :, :cu[-1]].any()
        _zero_rows(o, LENGTHS, slots)
        if admit and commit:        # the long admission: 110 tokens into slot 6, the ring full and wrapped at slot 0
            assert pg._dev_state[6].tolist() == [NS, W, 0, 110] and pg._dev_state[7].tolist() == [NS, 29, 29, 33]


# ------------------------------------------------------------------ 2. the storing calls
@pytest.mark.parametrize("dtype,D,G,W,P,scales", GRID)
def test_prefill_and_packed_commit_store_quant_of_what_the_16_bit_paged_pool_gets(dtype, D, G, W, P, scales):
    g = torch.Generator().manual_seed(321)
    fills = [[2, 9, NS + W, NS + W + 40][s % 4] for s in range(S)]
    live = [s for s in range(S) if s not in FRESH]
    kp, vp = (rand((1, HKV, sum(fills[s] for s in live), D), g, dtype).to(DEV) for _ in range(2))
    def prefill(p):
        p.prefill_slots(kp, vp, _cu([fills[s] for s in live]), live)
    cur = _fp8_layer(S, HKV, D, W, NS, dtype, scales)
    pg, tw = _paged8(cur, dtype, P, seed=322, after=_ring_after(cur, prefill), wrap_check=False)
    assert bool((_u8(pg.window_k) == NAN8).all())                  # nothing is live yet: every page row is NaN
    _three(pg, tw, dtype, scales, prefill, ("prefill_slots", dtype, D, W, P), stores=True)
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
        pg, tw = _paged8(tw, dtype, P, seed=323 + use_path, after=_ring_after(tw, commit), wrap_check=use_path is False)
        _three(pg, tw, dtype, scales, commit, ("commit_packed_dyn", "path", use_path, dtype, D, W, P), stores=True)
    assert pg._dev_state[3].tolist() == [NS, W, 14, NS + W + 54]    # wrapped, write_pos inside the first page


def test_the_names_of_the_storing_calls():
    dtype, D, W, P = torch.bfloat16, 64, 64, 32
    base8, _ = _base8(dtype, D, W, 331, SCALES)
    pg, _ = _paged8(base8, dtype, P, seed=332, after=[W] * S)
    g = torch.Generator().manual_seed(333)
    k, v = (rand((1, HKV, 7, D), g, dtype).to(DEV) for _ in range(2))
    pg.commit_packed_dyn(k, v, _i32([0, 7]), _dev_slots([1]), _i32([7]))
    assert _path() == "ring_commit_path_ragged_slots_paged_kvfp8", _path()
    pg.prefill_slots(k, v, [0, 7], [6])
    assert _path() == "ring_fill_varlen_slots_paged_kvfp8", _path()
    q, k1, v1, _ = _pack(dtype, D, 8, 8, seed=334)
    _run(pg, q, k1, v1, _cu([1, 7]), [3, 1], commit=True)
    assert _path().startswith("decode_multi_mfma_bf16_d64_rb") and _path().endswith("_ragged_commit_paged_kvfp8"), _path()
    _guard_ok(pg, "names")
    with pytest.raises(TypeError, match="bfloat16 or float16 tensors of one dtype"):
        pg.prefill_slots(k.float(), v.float(), [0, 7], [6])
    with pytest.raises(TypeError, match="packed calls"):
        pg.extend_step_dyn(q.to(DEV), k1.to(DEV), v1.to(DEV), slots=[0])


# ------------------------------------------------------------------ 3. fork: the copy equality
@pytest.mark.parametrize("dtype,D,G,W,P", [(torch.bfloat16, 64, 8, 64, 32), (torch.float16, 80, 1, 96, 32),
                                           (torch.bfloat16, 96, 1, 96, 32), (torch.float16, 128, 8, 64, 32)])
def test_fork_slots_copies_codes_through_both_tables_within_a_pool_and_between_two(dtype, D, G, W, P):
    base8, _ = _base8(dtype, D, W, 341, SCALES)
    wl = base8._dev_state[:, 1].tolist()
    after = list(wl)
    after[6], after[7] = wl[3], wl[1]                              # the caller maps the destination's pages first
    pg, tw = _paged8(base8, dtype, P, seed=342, after=after)
    s_pg, s_tw = _snap(pg), _snap(tw)
    pg.fork_slots([3, 1], [6, 7])                                  # a wrapped ring and a partly filled one
    assert _path() == "ring_copy_slots_paged", _path()
    tw.fork_slots([3, 1], [6, 7])
    assert _path() == "ring_copy_slots", _path()
    assert _stored_vs_twin(pg, tw, s_pg, s_tw, ("fork in one pool", dtype, D, W, P)) > 0
    _guard_ok(pg, "fork in one pool")
    assert pg._dev_state[6].tolist() == pg._dev_state[3].tolist() and pg._dev_state[7].tolist() == pg._dev_state[1].tolist()
    # into a second paged FP8 pool of another size and another shuffle, equal scales
    after2 = [0] * S
    after2[0], after2[5], after2[2], after2[3] = wl[3], wl[1], W, W      # slots 2 and 3: mapped and empty
    other_pg, other_tw = _paged8(_fp8_layer(S, HKV, D, W, NS, dtype, SCALES), dtype, P, seed=343, after=after2, extra=9,
                                 wrap_check=False)
    assert other_pg.window_k.shape[0] != pg.window_k.shape[0]
    s_pg, s_tw = _snap(other_pg), _snap(other_tw)
    other_pg.fork_slots([3, 7], [0, 5], source=pg)
    assert _path() == "ring_copy_slots_paged", _path()
    other_tw.fork_slots([3, 7], [0, 5], source=tw)
    assert _stored_vs_twin(other_pg, other_tw, s_pg, s_tw, "fork between two pools") > 0
    _guard_ok(other_pg, "fork between two pools"), _guard_ok(pg, "the source of the fork")
    with pytest.raises(ValueError, match="differ in (geometry|paging)"):
        pg.fork_slots([0], [1], source=base8)                      # a contiguous FP8 pool
    with pytest.raises(TypeError, match="differ in dtype"):
        pg.fork_slots([0], [1], source=_deq_paged(pg, dtype, SCALES))      # a 16-bit paged pool: another kv_dtype
    # every later call on the forks is bitwise the call on the sources: a committing step, its output and what it leaves
    lengths = [1, 7]
    q, k, v, sa = _pack(dtype, D, G, 8, seed=344)
    src = _twin(pg)
    o_src = _run(src, q, k, v, _cu(lengths), [3, 1], sa=sa, commit=True).clone()
    assert not torch.isnan(o_src).any() and o_src.any()
    for pool, slots in ((pg, [6, 7]), (other_pg, [0, 5])):
        o = _run(pool, q, k, v, _cu(lengths), slots, sa=sa, commit=True)
        assert _path().endswith(TAIL) and torch.equal(o, o_src), slots
        after_ = _twin(pool)
        for d, s in zip(slots, [3, 1]):
            st = src._dev_state[s].tolist()
            assert after_._dev_state[d].tolist() == st
            for name, n in (("sink_k", st[0]), ("sink_v", st[0]), ("window_k", st[1]), ("window_v", st[1])):
                assert torch.equal(_u8(getattr(after_, name))[d, :, :n], _u8(getattr(src, name))[s, :, :n]), (slots, name)
        _guard_ok(pool, "the step on the forks")


# ------------------------------------------------------------------ 4. the fp64 oracle over the dequantised history
@pytest.mark.parametrize("dtype,D,G,W,P", [(dt, D, G) + GEO[n % 2] for n, (dt, D, G) in enumerate(CASES)])
def test_the_oracle_over_the_dequantised_history(dtype, D, G, W, P):
    base8, hist8 = _base8(dtype, D, W, 351, SCALES)
    pg, _ = _paged8(base8, dtype, P, seed=352)
    q, k, v, sa = _pack(dtype, D, G, T_PAD, seed=353)
    trees = _trees()
    o = _run(pg, q, k, v, _cu(LENGTHS), PLAIN, _parents(LENGTHS, trees, T_PAD), sa=sa)
    assert _path().startswith("decode_tree_mfma_") and _path().endswith("_ragged" + TAIL), _path()
    ref = _oracle(q, k, v, sa, hist8, W, LENGTHS, PLAIN, trees)
    assert len(ref) == sum(1 for n, s in zip(LENGTHS, PLAIN) if n and s >= 0)
    _check_rows(o, ref, LENGTHS, DECODE_TOL[dtype], ("paged fp8 pool", dtype, D, G, W, P))


# ------------------------------------------------------------------ 5. unmapped entries
@pytest.mark.parametrize("entry", [-1, "n_pages", INT_MAX])
def test_a_store_to_an_unmapped_page_is_dropped_and_the_state_row_still_advances(entry):
    dtype, D, W, P = torch.bfloat16, 64, 64, 32
    base8, _ = _base8(dtype, D, W, 361, SCALES)
    pg, tw = _paged8(base8, dtype, P, seed=362)
    e = pg.window_k.shape[0] if entry == "n_pages" else entry
    assert pg._dev_state[2].tolist() == [NS, W, 0, NS + W]         # a full ring at write_pos 0: 7 tokens go to page entry 0
    pg.page_table[2, 0] = e
    g = torch.Generator().manual_seed(363)
    k, v = (rand((1, HKV, 7, D), g, dtype).to(DEV) for _ in range(2))
    before, tw_before = _snap(pg), _snap(tw)
    for p in (pg, tw):
        p.commit_packed_dyn(k, v, _i32([0, 7]), _dev_slots([2]), _i32([7]))
    moved = [name for name in BUFS if not torch.equal(_ints(getattr(pg, name)), before[name])]
    assert not moved, (entry, moved, "every page keeps its bytes")
    _guard_ok(pg, ("unmapped", entry))
    assert torch.equal(pg._dev_state, tw._dev_state) and pg._dev_state[2].tolist() == [NS, W, 7, NS + W + 7]
    assert not torch.equal(_u8(tw.window_k)[2], tw_before["window_k"][2])          # the twin did store


# ------------------------------------------------------------------ 6. determinism
def test_two_runs_give_the_same_bits():
    dtype, D, G, W, P = torch.float16, 80, 1, 96, 32
    base8, _ = _base8(dtype, D, W, 371, SCALES)
    q, k, v, sa = _pack(dtype, D, G, T_PAD, seed=372)
    par = _parents(LENGTHS, _trees(), T_PAD)
    call = lambda p: _run(p, q, k, v, _cu(LENGTHS), PLAIN, par, sa=sa, commit=True)
    after = _ring_after(base8, call)
    a, _ = _paged8(base8, dtype, P, seed=373, after=after)
    b, _ = _paged8(base8, dtype, P, seed=373, after=after)
    o1 = _run(a, q, k, v, _cu(LENGTHS), PLAIN, par, sa=sa).clone()
    o2 = _run(a, q, k, v, _cu(LENGTHS), PLAIN, par, sa=sa)
    assert torch.equal(o1, o2) and not torch.isnan(o1).any()
    before = _snap(a)
    call(a), call(b)
    _unmoved(a, _snap(b), "two committing runs leave the same bytes")
    assert not torch.equal(_u8(a.window_k), before["window_k"]), "the committing run wrote rows"
    _guard_ok(a, "run a"), _guard_ok(b, "run b")


# ------------------------------------------------------------------ 7. one captured graph, replayed after in-place changes
def _move(pg, s, free):
    """move the pages of slot s to the pages `free` with torch copies, 0x7F what they leave, rewrite the row in place;
    returns the pages that are free now"""
    row = [e for e in pg.page_table[s].tolist() if e >= 0]
    ptr = pg.page_table.data_ptr()
    for old, new in zip(row, free):
        for name in RING:
            pages = _u8(getattr(pg, name))
            pages[new].copy_(pages[old])
            pages[old].fill_(NAN8)
    pg.page_table[s, :len(row)] = torch.tensor(free[:len(row)], dtype=torch.int32, device=DEV)
    assert pg.page_table.data_ptr() == ptr
    return row


def test_one_captured_graph_replays_after_in_place_changes_of_lengths_slots_table_and_scales():
    dtype, D, G, W, P, T, n_seq = torch.bfloat16, 64, 8, 96, 32, 112, 6
    base8, _ = _base8(dtype, D, W, 381, SCALES)
    pg, _ = _paged8(base8, dtype, P, seed=382, after=[W] * S, extra=4)        # every slot mapped: any mix of lengths fits
    sq = torch.zeros(1, HKV * G, T, D, dtype=dtype, device=DEV)
    sk, sv = (torch.zeros(1, HKV, T, D, dtype=dtype, device=DEV) for _ in range(2))
    scu, ssl = torch.zeros(n_seq + 1, dtype=torch.int32, device=DEV), torch.full((n_seq,), -1, dtype=torch.int32, device=DEV)
    so = torch.zeros_like(sq)
    sad = rand((HKV * G,), torch.Generator().manual_seed(380), torch.float32, 0.8).to(DEV)
    step = lambda p, out: p.ragged_step_dyn(sq, sk, sv, scu, ssl, s_aux=sad, out=out, commit=True, admit=True)
    start = _snap(pg)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):         # warm-up outside the capture (allocates the workspace); all rows inactive
        step(pg, so)
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(pg, so)
    _unmoved(pg, start, "warm-up and capture with every sequence inactive")
    owned = {e for row in pg.page_table.tolist() for e in row if e >= 0}
    free = [e for e in range(pg.window_k.shape[0]) if e not in owned]
    assert len(free) >= W // P
    # (lengths, slots, move the pages of slot 3, new scales): decode rows; chunks and an admission of 70 tokens on the
    # fresh slot 6 after slot 3 (the wrapped ring) moved to other pages; partly inactive, after an in-place set_kv_scale
    steps = [([1, 1, 1, 1, 1, 1], [0, 1, 2, 3, 4, 5], False, None),
             ([16, 70, 7, 9, 1, 5], [1, 6, 3, 2, 4, 0], True, None),
             ([33, 4, 0, 12, 1, 40], [5, -1, 2, 7, -1, 3], True, ([1.5, 0.5], [0.25, 3.0]))]
    for r, (lengths, slots, move, scales) in enumerate(steps):
        q, k, v, _ = _pack(dtype, D, G, T, seed=383 + r)
        sq.copy_(q), sk.copy_(k), sv.copy_(v)
        scu.copy_(torch.tensor(_cu(lengths), dtype=torch.int32)), ssl.copy_(torch.tensor(slots, dtype=torch.int32))
        if move:
            free = _move(pg, 3, free)
        if scales is not None:
            ptr = pg.kv_scale.data_ptr()
            pg.set_kv_scale(torch.tensor(scales[0], device=DEV), torch.tensor(scales[1], device=DEV))
            assert pg.kv_scale.data_ptr() == ptr                    # in place: the graph keeps the pointer
        tw = _twin(pg)                                              # the twin of the pool as it stands: table, scales, state
        s_pg, s_tw = _snap(pg), _snap(tw)
        so.zero_()
        graph.replay()
        o = step(tw, None)                                          # the eager run of the same inputs on the twin
        assert _path().endswith("_ragged_admit_commit_kvfp8"), _path()
        assert not torch.isnan(so).any() and torch.equal(so, o), ("replay", r)
        assert _stored_vs_twin(pg, tw, s_pg, s_tw, ("replay", r)) > 0
        _guard_ok(pg, ("replay", r))
        _zero_rows(so, lengths, slots)
        assert so[:, :, :_cu(lengths)[-1]].any()
    assert pg._dev_state[6, 3].item() == 70 and pg._dev_state[7, 3].item() == 12


# ------------------------------------------------------------------ 8. the walk pack: two tiles per page, multi-tile wave walks
@pytest.mark.parametrize("dt,D", [("bf16", 64), ("fp16", 128), ("bf16", 80), ("fp16", 96)])
def test_the_walk_pack_at_two_tiles_per_page(dt, D):
    P = 64
    inp = R.pack_inputs("walk", "randn", dt, D)
    case, act = inp["case"], inp["dtype"]
    assert (case["Hkv"], case["G"], case["T_PAD"], case["Wc"]) == (8, 8, 1024, 320)
    scales = PL._scales(case["Hkv"])
    base8 = PL._pool(inp, fp8=True)
    assert base8.kv_scale.tolist() == torch.tensor(scales, dtype=torch.float32).tolist()
    for commit in (False, True):
        call = lambda p: PL._run(p, inp, commit=commit)
        pg, tw = _paged8(base8, act, P, seed=391 + commit, after=_ring_after(base8, call))
        assert pg.page_table.shape[1] == 5
        PL._reaches(case, pg, case["T_PAD"])                    # the regime, from the paged pool's own state rows
        o = _three(pg, tw, act, scales, call, ("walk", dt, D, "commit", commit), stores=commit)
        assert o.any()
