"""GPU tests of the export of pool slots (sfa_ring_export_slots and its FP8 / paged / paged FP8 forms;
SinkCacheLayer.export_slots / import_slots / live_lengths).

The contract of include/sfa.h: the live tokens of each named slot arrive in TOKEN order - sink rows, then the ring from
its oldest token - bitwise (a 16-bit / fp32 pool: the bytes; an FP8 pool: T(float(code) * scale)), every other row of the
pack is exactly zero, pos holds each token's position, and nothing of the pool is written.  The expected pack is the torch
twin of tests/export_ref.py, which tests/test_export_host.py holds to a brute-force model of the cache.

One pool per (kind, dtype, D, Wc) holds ten slots in ten fill states (_STATES), reached the way a server reaches them:
prefill_slots, then committing ragged_step_dyn calls of 1 to 7 tokens.  Every token row carries its slot and its number
in its first 16 elements (one bit per element), so that a wrong row cannot match.

Paged pools use the smallest page the library serves, P = 32, with rings of one and of three pages (Wc 32 and 96) where
the contiguous pools use Wc 16 and 48."""
import functools

import pytest
import torch

import export_ref as X
from oracle import sink_oracle as O
from sink_attention import SinkCacheLayer, _native
from util import DECODE_TOL, maxdiff, rand

pytestmark = pytest.mark.gpu
DEV = "cuda"
HKV, G, NS, S, P = 2, 2, 4, 11, 32
BF, FP, F32, FP8 = torch.bfloat16, torch.float16, torch.float32, torch.float8_e4m3fn
KINDS = ("c16", "fp8", "paged", "paged_fp8")
TAIL = {"c16": "", "fp8": "_kvfp8", "paged": "_paged", "paged_fp8": "_paged_kvfp8"}
SCALES = ([0.37, 1.9], [2.3, 0.011])          # K and V, per head: no power of two, no two alike
BUFS = ("sink_k", "sink_v", "window_k", "window_v")
CASES = [(kind, dt, D, w) for kind in KINDS for dt, D in ((BF, 64), (FP, 80), (BF, 128)) for w in (0, 1)] + \
        [("c16", F32, 20, 0)]


def _wc(kind, w):
    return ((32, 96) if "paged" in kind else (16, 48))[w]


def _states(Wc):
    """slot -> (prefill length, tokens committed afterwards); slot 0 stays fresh, slot 10 is never named"""
    return {1: (NS - 1, 0),             # fewer tokens than num_sink
            2: (NS, 0),                 # exactly num_sink, an empty ring
            3: (NS + 2, 5),             # a ring partly filled, by a prefill and by commits
            4: (NS + Wc, 0),            # a ring exactly full, prefilled: write_pos 0
            5: (NS + Wc, 1),            # wrapped, write_pos 1
            6: (NS + Wc, Wc // 2),      # wrapped, write_pos Wc / 2
            7: (NS + Wc, Wc - 1),       # wrapped, write_pos Wc - 1
            8: (NS + Wc + 9, 0),        # a prompt longer than the cache: evicted by the prefill itself
            9: (NS + Wc - 1, 3)}        # commits that fill the ring and wrap it


def _coded(s, n, D, dtype, g):
    """n token rows [1, HKV, n, D] of slot s: random, with bit b of the token number in element b and bit b of 8 s + head
    in element 8 + b (1.0 / 0.5: exact in every dtype and under every scale's quantisation distinct)"""
    x = rand((1, HKV, n, D), g, dtype)
    t = torch.arange(n)
    for b in range(8):
        x[0, :, :, b] = torch.where((t >> b) & 1 == 1, 1.0, 0.5).to(dtype)[None, :]
        for h in range(HKV):
            x[0, h, :, 8 + b] = 1.0 if ((8 * s + h) >> b) & 1 else 0.5
    return x


def _new(kind, dtype, D, Wc, slots_=S):
    layer = SinkCacheLayer(NS, Wc)
    kw = dict(page_size=P) if "paged" in kind else {}
    if "fp8" in kind:
        kw["kv_dtype"] = FP8
    layer.init_pool(slots_, HKV, D, dtype, DEV, **kw)
    if "fp8" in kind:
        layer.set_kv_scale(*SCALES)
    return layer


def _reserve(layer, slots, seed=5):
    """map the whole ring of every slot, one slot at a time in a shuffled order: the table is no identity"""
    if layer.page_size:
        order = [slots[i] for i in torch.randperm(len(slots), generator=torch.Generator().manual_seed(seed)).tolist()]
        for s in order:
            layer.reserve_pages([s], layer.num_sink + layer.window_size)


@functools.lru_cache(maxsize=None)
def _pool(kind, dtype, D, Wc):
    """(layer, state rows on the host) - shared by the tests of a case, which leave it as it is"""
    g = torch.Generator().manual_seed(1000 + 7 * D + Wc)
    layer = _new(kind, dtype, D, Wc)
    for name in BUFS:                                   # stale content everywhere: bytes of 0x3c / 0x3c3c are finite
        getattr(layer, name).view(torch.uint8).fill_(0x3C)
    st = _states(Wc)
    used = sorted(st)
    _reserve(layer, used)
    toks = {s: (_coded(s, a + b, D, dtype, g), -_coded(s, a + b, D, dtype, g)) for s, (a, b) in st.items()}
    cu = [0]
    for s in used:
        cu.append(cu[-1] + st[s][0])
    layer.prefill_slots(torch.cat([toks[s][0][:, :, :st[s][0]] for s in used], 2).to(DEV),
                        torch.cat([toks[s][1][:, :, :st[s][0]] for s in used], 2).to(DEV), cu, used)
    done = {s: 0 for s in used}
    rnd = 0
    while any(done[s] < st[s][1] for s in used):        # committing steps of 1 to 7 tokens per sequence
        take = {s: min(st[s][1] - done[s], 1 + (rnd + s) % 7) for s in used if done[s] < st[s][1]}
        seqs = sorted(take)
        cq = [0]
        for s in seqs:
            cq.append(cq[-1] + take[s])
        sl = lambda s, i: toks[s][i][:, :, st[s][0] + done[s]:st[s][0] + done[s] + take[s]]
        kn, vn = (torch.cat([sl(s, i) for s in seqs], 2).to(DEV) for i in (0, 1))
        q = rand((1, HKV * G, cq[-1], D), g, dtype).to(DEV)
        layer.ragged_step_dyn(q, kn, vn, cq, seqs, commit=True)
        for s in seqs:
            done[s] += take[s]
        rnd += 1
    state = layer._dev_state.tolist()
    for s, (a, b) in st.items():
        rem = a + b - NS
        assert state[s] == [min(a, NS), min(max(rem, 0), Wc), (rem % Wc if b else (rem if 0 < rem < Wc else 0)), a + b], (s, state[s])
    assert state[0] == [0, 0, 0, 0] and [state[s][2] for s in (5, 6, 7)] == [1, Wc // 2, Wc - 1]
    return layer, state


def _twin(layer, slots, cu, T):
    cpu = lambda t: None if t is None else t.detach().cpu()
    return X.export_twin(*(cpu(getattr(layer, n)) for n in BUFS), cpu(layer._dev_state), slots, cu, T, NS,
                         layer.window_size, table=cpu(layer.page_table), kv_scale=cpu(layer.kv_scale),
                         dtype=layer._act_dtype)


def _snapshot(layer):
    return [getattr(layer, n).clone() for n in BUFS] + [layer._dev_state.clone()] + \
        ([layer.page_table.clone()] if layer.page_size else []) + ([layer.kv_scale.clone()] if layer.kv_scale is not None else [])


def _same_snapshot(a, b):
    return all(X.same_bits(x.view(torch.uint8) if x.dtype == FP8 else x, y.view(torch.uint8) if y.dtype == FP8 else y)
               for x, y in zip(a, b))


def _nan_out(layer, T, pos=True):
    dt = layer._act_dtype
    k = torch.full((1, HKV, T, layer.sink_k.shape[3]), float("nan"), dtype=dt, device=DEV)
    return (k, k.clone(), torch.full((T,), -7, dtype=torch.int32, device=DEV)) if pos else (k, k.clone())


def _assert_pack(got, want, what):
    k, v, pos = got
    wk, wv, wpos = want
    assert pos.cpu().tolist() == wpos.tolist(), (what, "pos", pos.cpu().tolist(), wpos.tolist())
    for name, a, b in (("k", k, wk), ("v", v, wv)):
        a = a.cpu()
        if not X.same_bits(a, b):
            rows = [r for r in range(a.shape[2]) if not X.same_bits(a[:, :, r], b[:, :, r])]
            r = rows[0]
            bits = lambda t: t[:, :, r].contiguous().view(torch.uint8).flatten()
            at = (bits(a) != bits(b)).nonzero().flatten().tolist()[:8]
            raise AssertionError((what, name, "rows that differ", rows, "first bytes", at, bits(a)[at].tolist(),
                                  bits(b)[at].tolist()))


NAMED = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, -1, 6]            # every state, an inactive entry, the same slot twice


# ------------------------------------------------------------------------------------------------ 1. the pack
@pytest.mark.parametrize("kind,dtype,D,w", CASES)
def test_the_pack_is_bitwise_the_twin_and_the_pool_is_not_written(kind, dtype, D, w):
    Wc = _wc(kind, w)
    layer, state = _pool(kind, dtype, D, Wc)
    before = _snapshot(layer)
    # the convenient form: offsets from live_lengths, one read-back for T
    live = layer.live_lengths(NAMED).tolist()
    assert live == [0 if s < 0 else state[s][0] + state[s][1] for s in NAMED]
    k, v, cu, pos = layer.export_slots(NAMED, return_positions=True)
    assert _native.last_path() == "ring_export_slots" + TAIL[kind], _native.last_path()
    cu_l = cu.tolist()
    assert cu_l == [sum(live[:i]) for i in range(len(live) + 1)] and k.shape == (1, HKV, cu_l[-1], D)
    assert k.dtype == v.dtype == layer._act_dtype and pos.dtype == torch.int32
    _assert_pack((k, v, pos), _twin(layer, NAMED, cu_l, cu_l[-1]), (kind, "convenient"))
    assert not (pos < 0).any()
    # explicit offsets over outputs full of NaN: sequences cut short, sequences with a zero tail, rows behind cu[-1]
    # (the last sequence is cut short in front of the padding: rows behind it belong to no sequence)
    room = [n - 2 if (i % 3 == 0 or i == len(live) - 1) and n > 2 else n + 3 if i % 3 == 1 else n for i, n in enumerate(live)]
    cu2 = [sum(room[:i]) for i in range(len(room) + 1)]
    T = cu2[-1] + 5
    for cu_arg in (cu2, torch.tensor(cu2, dtype=torch.int32, device=DEV)):
        out = _nan_out(layer, T)
        got = layer.export_slots(torch.tensor(NAMED, dtype=torch.int32, device=DEV), cu=cu_arg, out=out)
        assert got[0] is out[0] and got[1] is out[1] and len(got) == 3
        want = _twin(layer, NAMED, cu2, T)
        _assert_pack(out, want, (kind, "explicit"))
        assert any(m < n for m, n in zip(room, live)) and int((want[2] < 0).sum()) >= 5 + 3 * 4
        zero = (want[2] < 0).nonzero().flatten().tolist()
        assert not out[0][:, :, zero].any() and not out[1][:, :, zero].any()          # exactly zero, not NaN
    again = _nan_out(layer, T)
    layer.export_slots(NAMED, cu=cu2, out=again)
    assert all(X.same_bits(a, b) for a, b in zip(again, out)), "a repeated call is bitwise identical"
    assert _same_snapshot(_snapshot(layer), before), "export wrote into the pool"


@pytest.mark.parametrize("kind,dtype,D,w", [c for c in CASES if "paged" in c[0] and c[3] == 1])
def test_an_unmapped_page_exports_zero_rows_with_their_positions(kind, dtype, D, w):
    Wc = _wc(kind, w)
    layer, state = _pool(kind, dtype, D, Wc)
    table = layer.page_table.clone()
    try:
        layer.page_table[6, 1] = -1                      # ring slots 32 .. 63 of slot 6 (write_pos 48: both sides of it)
        layer.page_table[7, 0] = 10 ** 6                 # beyond n_pages: unmapped as well
        named = [6, 7, 4]
        k, v, cu, pos = layer.export_slots(named, return_positions=True)
        want = _twin(layer, named, cu.tolist(), k.shape[2])
        _assert_pack((k, v, pos), want, (kind, "unmapped"))
        full = _twin_with(layer, table, named, cu.tolist(), k.shape[2])
        assert pos.cpu().tolist() == full[2].tolist() and not (pos < 0).any()
        holes = [r for r in range(k.shape[2]) if bool(full[0][:, :, r].any()) and not bool(want[0][:, :, r].any())]
        assert len(holes) == 2 * P and not k[:, :, holes].any() and not v[:, :, holes].any()
    finally:
        layer.page_table.copy_(table)


def _twin_with(layer, table, slots, cu, T):
    now = layer.page_table.clone()
    layer.page_table.copy_(table)
    try:
        return _twin(layer, slots, cu, T)
    finally:
        layer.page_table.copy_(now)


# ------------------------------------------------------------------------------------------------ 2. round trips
MOVED = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9]
DEST = [3, 9, 0, 7, 1, 8, 2, 10, 5, 4]


def _move(src, dst, moved=MOVED, dest=DEST):
    k, v, cu, pos = src.export_slots(moved, return_positions=True)
    _reserve(dst, dest, seed=9)
    dst.import_slots(k, v, cu, dest, seen=src.positions(moved))
    return k, v, cu, pos


@pytest.mark.parametrize("kind,dtype,D,w", [c for c in CASES if c[3] == 0])
def test_export_import_export_is_bitwise_in_a_pool_of_the_same_geometry(kind, dtype, D, w):
    Wc = _wc(kind, w)
    src, _ = _pool(kind, dtype, D, Wc)
    dst = _new(kind, dtype, D, Wc)
    k, v, cu, pos = _move(src, dst)
    k2, v2, cu2, pos2 = dst.export_slots(DEST, return_positions=True)
    assert torch.equal(cu2, cu) and torch.equal(pos2, pos)
    assert X.same_bits(k2, k) and X.same_bits(v2, v)
    assert torch.equal(dst.live_lengths(DEST), src.live_lengths(MOVED))
    assert torch.equal(dst.positions(DEST), src.positions(MOVED))
    ring_full = dst._dev_state[DEST, 1] == Wc
    assert bool((dst._dev_state[DEST, 2][ring_full] == 0).all())         # a full ring arrives rotated to write_pos 0


def _decode_rows(layer, slots, q, kn, vn, sa):
    n = len(slots)
    return layer.ragged_step_dyn(q, kn, vn, list(range(n + 1)), slots, s_aux=sa, commit=False).cpu()


def _oracle_rows(k, v, cu, state_rows, Wc, q, kn, vn, sa):
    """fp64 rows of one decode token per sequence over the exported tokens: the sinks, the ring - less its oldest token
    when it is full, which the new token pushes out of the window - and the token itself"""
    rows = []
    for i, (sl, wl, _wp, _seen) in enumerate(state_rows):
        a, b = cu[i], cu[i + 1]
        keep = [j for j in range(b - a) if not (wl == Wc and j == sl)]
        kk = torch.cat([k[:, :, a:b][:, :, keep], kn[:, :, i:i + 1]], 2)
        vv = torch.cat([v[:, :, a:b][:, :, keep], vn[:, :, i:i + 1]], 2)
        rows.append(O.decode_dense(q[:, :, i:i + 1], kk, vv, sa))
    return torch.cat(rows, 2)


@pytest.mark.parametrize("move", ["bf16_to_paged", "wc16_to_wc48", "fp8_to_bf16"])
def test_a_move_into_another_geometry_decodes_like_the_source(move):
    dt, D = BF, 64
    src_kind, src_wc, dst_kind, dst_wc = {"bf16_to_paged": ("c16", 32, "paged", 32),"wc16_to_wc48": ("c16", 16, "c16", 48),
                                          "fp8_to_bf16": ("fp8", 16, "c16", 16)}[move]
    src, _ = _pool(src_kind, dt, D, src_wc)
    dst = _new(dst_kind, dt, D, dst_wc)
    moved, dest = MOVED[1:], DEST[1:]                      # a fresh slot decodes nothing
    k, v, cu, pos = _move(src, dst, moved, dest)
    k, v, cu = k.cpu(), v.cpu(), cu.tolist()
    assert torch.equal(dst.positions(dest), src.positions(moved))
    live = src.live_lengths(moved).tolist()
    assert dst.live_lengths(dest).tolist() == [min(n, NS + dst_wc) for n in live] == live
    k2, v2, _cu2, pos2 = dst.export_slots(dest, return_positions=True)
    assert X.same_bits(k2.cpu(), k) and X.same_bits(v2.cpu(), v) and torch.equal(pos2, pos)
    g = torch.Generator().manual_seed(77)
    n = len(moved)
    q, kn, vn = (rand((1, h, n, D), g, dt) for h in (HKV * G, HKV, HKV))
    sa = rand((HKV * G,), g, F32, 0.8)
    for layer, slots, Wc in ((src, moved, src_wc), (dst, dest, dst_wc)):
        o = _decode_rows(layer, slots, q.to(DEV), kn.to(DEV), vn.to(DEV), sa.to(DEV))
        ref = _oracle_rows(k, v, cu, layer._dev_state[slots].tolist(), Wc, q, kn, vn, sa)
        err = (o.double() - ref).abs().amax(dim=(0, 1, 3))
        print(move, "Wc", Wc, "max error per sequence", [f"{e:.2e}" for e in err.tolist()])
        assert err.max().item() <= DECODE_TOL[dt], (move, Wc, err.tolist())


# ------------------------------------------------------------------------------------------------ 3. capture, strides
def test_a_captured_export_replays_after_states_and_offsets_are_rewritten():
    kind, dt, D, Wc = "paged_fp8", BF, 64, 96
    shared, _ = _pool(kind, dt, D, Wc)
    layer = _new(kind, dt, D, Wc)
    _move(shared, layer, MOVED, MOVED)                    # a pool of this test's own: its states are rewritten below
    T, n = 256, 6
    slots = torch.tensor([7, 6, -1, 3, 8, 6], dtype=torch.int32, device=DEV)
    cu = torch.tensor([0, 100, 150, 150, 161, 250, 256], dtype=torch.int32, device=DEV)
    out = _nan_out(layer, T)
    call = lambda o: layer.export_slots(slots, cu=cu, out=o)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(out)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call(out)
    rounds = [([7, 6, -1, 3, 8, 6], [0, 100, 150, 150, 161, 250, 256], None),
              ([1, 2, 9, 5, 4, 0], [0, 3, 7, 110, 200, 240, 240], None),
              ([6, 6, 6, -1, -1, 7], [0, 60, 160, 170, 170, 170, 256], {6: [4, 50, 17, 900], 7: [2, 96, 95, 5000]})]
    for sl, c, states in rounds:
        slots.copy_(torch.tensor(sl, dtype=torch.int32))
        cu.copy_(torch.tensor(c, dtype=torch.int32))
        for s, row in (states or {}).items():
            layer._dev_state[s] = torch.tensor(row, dtype=torch.int32, device=DEV)
        eager = _nan_out(layer, T)
        call(eager)
        for t in out:
            t.fill_(-7) if t.dtype == torch.int32 else t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert all(X.same_bits(a, b) for a, b in zip(out, eager)), (sl, c)
        _assert_pack(out, _twin(layer, sl, c, T), ("replay", sl))


def test_the_pack_may_be_a_strided_view():
    kind, dt, D, Wc = "c16", FP, 80, 48
    layer, _ = _pool(kind, dt, D, Wc)
    named = [7, 3, 9]
    k, v, cu, pos = layer.export_slots(named, return_positions=True)
    T = k.shape[2] + 3
    store = [torch.full((1, T, HKV, D), float("nan"), dtype=dt, device=DEV) for _ in range(2)]       # [1, T, H_kv, D]
    views = tuple(s.permute(0, 2, 1, 3) for s in store)
    assert views[0].stride(1) == D and views[0].stride(2) == HKV * D
    layer.export_slots(named, cu=cu, out=views)
    for got, ref in zip(store, (k, v)):
        assert X.same_bits(got[:, :T - 3], ref.permute(0, 2, 1, 3).contiguous()) and not got[:, T - 3:].any()
