"""ragged_step_dyn(decode_kernel="draft") (SFA_FLAG_RAGGED_DECODE_DRAFT): the six contracts of
include/sfa.h on variants of `walk` / `capped` whose draft sequences (n_i >= 2, G n_i <= 32) fill the 32-row block
exactly, with padding rows and at its smallest, over rings wrapped off a tile edge, exactly full (token t loses t + 1
slots), filling up inside the chunk, nearly empty, with the sinks not full, and on fresh slots admitted with fewer and more
tokens than num_sink.  `_pad` variants add inactive sequences until H_kv n_seq = 2048 (one split, 3 / 9 tiles per wave:
the LDS ring wraps at either depth), the others plan S >= 3."""
import pytest
import torch

import packed_regime as R
import test_gpu_packed_long as PL
import test_gpu_paged_fp8_pool as PF
import test_gpu_paged_pool as PP
from test_gpu_decode_multi import TOL
from test_gpu_fp8_pool import _snap as _snap8, _unmoved as _unmoved8
from test_gpu_ragged_chunk import _ref8
from test_gpu_ragged_decode import _pad
from test_gpu_ragged_tree import _check_rows, _i32, _oracle_tree, _parents
from test_gpu_slots import _clone, _dev_slots, _path
from test_ragged_tree_host import binary, chain, comb
from util import DECODE_TOL, maxdiff

pytestmark = pytest.mark.gpu


def _pack(name, G, n, base="walk", Hkv=8, Wc=None):
    """draft sequences of n tokens over the ring states of the docstring, two admitted ones (min(n, 3) and n tokens), an
    inactive one, a decode row, a 3-token sequence, an empty one LAST (test_a_draft_sequence... adds a chunk there) and a
    160-token chunk"""
    Wc = R.PACKS[base]["Wc"] if Wc is None else Wc
    F = R.NS + Wc
    c = R.variant(R.PACKS[base], name=name, G=G, Hkv=Hkv, Wc=Wc, T_PAD=256, S=13,
                  lengths=[n, n, n, n, n, min(n, 3), n, 2, 1, 3, 160 if n < 32 else 33, 0],       # n = 32: 234 rows of T_PAD
                  hist=[F + 37, F, F - 3, 9, 2, 0, 0, 50, 50, F + 101, F + 5, 0], slots=[3, 0, 5, 2, 9, 8, 10, -1, 4, 1, 7, 11],
                  admit=[False] * 5 + [True, True] + [False] * 4 + [True])
    R.PACKS[name] = c
    return c


FILL = [_pack("draft_g4", 4, 8), _pack("draft_g16", 16, 2, Hkv=2), _pack("draft_g5", 5, 6, Hkv=2), _pack("draft_g1n2", 1, 2),
        _pack("draft_g1n32", 1, 32), _pack("draft_g4n9", 4, 9), _pack("draft_clip", 1, 32, Hkv=2, Wc=16),
        _pack("draft_capped", 4, 8, base="capped", Hkv=8)]
for c in (_pad(FILL[0], "draft_g4_pad"), _pad(_pack("draft_capped2", 8, 4, base="capped", Hkv=2), "draft_capped_pad")):
    R.PACKS[c["name"]] = c
TYPES = PL.TYPES
CASES = [(c["name"], k, *TYPES[(i + j) % 4]) for i, c in enumerate(FILL[:7]) for j, k in enumerate(("randn", "probe"))] + \
        [("draft_g4", "randn", "fp16", 128), ("draft_g4", "probe", "bf16", 80), ("draft_g4", "randn", "fp16", 96),
         ("draft_g4_pad", "randn", "fp16", 128), ("draft_g4_pad", "probe", "bf16", 80), ("draft_capped_pad", "randn", "bf16", 64),
         ("draft_capped", "probe", "bf16", 64)]


def _run(layer, inp, dec, chunk=False, commit=False, parent=None, slots=None, lengths=None, qkv=None, out=None, **kw):
    case = inp["case"]
    q, k, v = PL._dev(inp) if qkv is None else qkv
    o = layer.ragged_step_dyn(q, k, v, _i32(R.cu_of(case["lengths"] if lengths is None else lengths)),
                              _dev_slots(case["slots"] if slots is None else slots), s_aux=inp["s_aux"].to(PL.DEV), out=out,
                              commit=commit, admit=True, parent=None if parent is None else _i32(parent), chunk_kernel=chunk,
                              decode_kernel=dec, **kw)
    tag = "_dec1raw" if kw.get("raw_fp8") else "_dec1"
    assert ((tag + "_draft_") in _path()) == (dec == "draft") and (tag in _path()) == bool(dec) and "_mfma_" in _path(), _path()
    return o


def _draft_rows(case):
    """the rows of the draft sequences; asserts the regime with the plan of packed_regime - one split and >= 3 tiles per
    wave on a padded pack, S >= 3 on the long rings of the others - so that no case passes empty"""
    cu, m = R.cu_of(case["lengths"]), torch.zeros(case["T_PAD"], dtype=torch.bool)
    S, tiles = [], []
    for i in R.live(case):
        n = case["lengths"][i]
        if n >= 2 and case["G"] * n <= 32:
            m[cu[i]:cu[i + 1]] = True
            st = [0, 0, 0, 0] if case["admit"][i] else R.state_after(case["hist"][i], case["ns"], case["Wc"])
            p = R.multi_plan(st[0], st[1], n, R.want_splits(1, case["Hkv"], len(case["lengths"])))
            S.append(p["S"]), tiles.append(p["T"])
    assert m.any() and not m[:cu[-1]].all()
    if case["name"].endswith("_pad"):
        assert max(S) == 1 and max(tiles) // R.WAVES >= 3, (S, tiles)
    elif case["Wc"] >= 320:
        assert max(S) >= 3, S
    return m.to(PL.DEV)


@pytest.mark.parametrize("name,kind,dt,D", CASES)
def test_draft_rows_meet_the_oracle_and_the_rest_is_the_call_with_true(name, kind, dt, D):
    """contracts 1 to 3; `draft_g4n9`: 36 rows stay on the split kernel with its bits (its 3-token sequences are drafts)"""
    inp = R.pack_inputs(name, kind, dt, D)
    case, what = inp["case"], (name, kind, dt, D)
    layer, m = PL._pool(inp), _draft_rows(inp["case"])
    base = _run(layer, inp, True).clone()
    _run(layer, inp, "draft")                                # allocates the call's own workspace
    layer._ragged_draft_state["ws"].fill_(0xFF)
    o = _run(layer, inp, "draft", out=torch.full_like(base, float("nan"))).clone()
    _check_rows(o, PL._ref(name, kind, dt, D), case["lengths"], TOL[inp["dtype"]], what)
    assert torch.equal(o[:, :, ~m], base[:, :, ~m]) and not torch.isnan(o).any(), what
    oc, cb = _run(layer, inp, "draft", chunk=True), _run(layer, inp, True, chunk=True)     # the serving configuration
    assert torch.equal(oc[:, :, ~m], cb[:, :, ~m]) and torch.equal(oc[:, :, m], o[:, :, m]), what
    a, b = _clone(layer), _clone(layer)
    a._pool = b._pool = True
    assert torch.equal(_run(a, inp, "draft", commit=True), o)
    _run(b, inp, False, commit=True)
    PL._same_pool(a, b, what)
    assert not torch.equal(a._dev_state, layer._dev_state)


@pytest.mark.parametrize("pool,dt,D", [("fp8", "bf16", 80), ("paged", "fp16", 128), ("paged_fp8", "bf16", 64)])
def test_the_other_three_pool_kinds(pool, dt, D):
    """`draft_g4`: the oracle each kind is held to today, the paged pools bitwise their twins (contract 6), the commit of the
    default call; FP8: raw_fp8=True moves the single-token rows alone"""
    inp = R.pack_inputs("draft_g4", "randn", dt, D)
    case, dtype, what = inp["case"], inp["dtype"], (pool, dt, D)
    fp8, M, m = pool != "paged", PF if pool == "paged_fp8" else PP, _draft_rows(inp["case"])
    ref, tol = (_ref8(inp), DECODE_TOL[dtype]) if fp8 else (PL._ref("draft_g4", "randn", dt, D), TOL[dtype])
    base = PL._pool(inp, fp8=fp8)
    for commit in (False, True):
        call = lambda p, flag="draft", **kw: _run(p, inp, flag, commit=commit, **kw)
        if pool == "fp8":
            pg, plain = PL._clone8(base), PL._clone8(base)
            raw, raw_true = call(PL._clone8(base), raw_fp8=True), call(PL._clone8(base), True, raw_fp8=True)
            o = call(pg)
            assert torch.equal(raw[:, :, ~m], raw_true[:, :, ~m]) and torch.equal(raw[:, :, m], o[:, :, m]), what
        elif fp8:
            make = lambda: PF._paged8(base, dtype, 64, seed=491 + commit, after=PF._ring_after(base, call))
            (pg, tw), (plain, _) = make(), make()            # the same seed: the same table, the same pages
            o = PF._three(pg, tw, dtype, PL._scales(case["Hkv"]), call, what, stores=commit)
        else:
            make = lambda: PP._paged(base, 64, seed=591 + commit, after=PP._ring_after(base, call))
            (pg, tw), (plain, _) = make(), make()
            o = PP._both(pg, tw, call, what, stores=commit)
        _check_rows(o, ref, case["lengths"], tol, what)
        assert torch.equal(o[:, :, ~m], call(plain, True)[:, :, ~m]) and not torch.isnan(o).any(), what
        _unmoved8(plain, _snap8(pg), what) if pool == "fp8" else M._unmoved(plain, M._snap(pg), what)


@pytest.mark.parametrize("dt,D", [("bf16", 64), ("fp16", 128)])
def test_a_draft_sequence_gives_the_same_bits_alone_permuted_and_beside_an_added_chunk(dt, D):
    """contract 4 on `draft_capped` (H_kv 8, Wc 1024): at T = 256 the split kernel's cap is want = 6, with 160 more rows 4, so
    its plan of a full ring (34 tiles) follows T; the draft plan follows (n_seq, H_kv) alone"""
    inp = R.pack_inputs("draft_capped", "randn", dt, D)
    case, layer, m = inp["case"], PL._pool(inp), _draft_rows(inp["case"])
    lengths, slots, cu = case["lengths"], case["slots"], R.cu_of(case["lengths"])
    drafts = [i for i in R.live(case) if m[cu[i]]]
    o = _run(layer, inp, "draft").clone()
    i = drafts[1]                                            # the exactly full ring
    alone = _run(layer, inp, "draft", slots=[s if j == i else -1 for j, s in enumerate(slots)])
    assert torch.equal(alone[:, :, cu[i]:cu[i + 1]], o[:, :, cu[i]:cu[i + 1]]) and not alone[:, :, cu[i + 1]:].any(), "alone"
    order = list(range(len(lengths)))[::-1]
    l2, s2 = [lengths[j] for j in order], [slots[j] for j in order]
    gather = torch.cat([torch.arange(cu[j], cu[j + 1]) for j in order] + [torch.arange(cu[-1], case["T_PAD"])]).to(PL.DEV)
    o2 = _run(layer, inp, "draft", slots=s2, lengths=l2, qkv=tuple(t[:, :, gather].contiguous() for t in PL._dev(inp)))
    g = torch.Generator().manual_seed(5)
    more = lambda t: torch.cat([t, torch.randn(1, t.shape[1], 160, D, generator=g).to(t)], dim=2)
    o3 = _run(layer, inp, "draft", lengths=lengths[:-1] + [160 + case["T_PAD"] - cu[-1]], qkv=tuple(more(t) for t in PL._dev(inp)))
    for i in drafts:
        a, j = o[:, :, cu[i]:cu[i + 1]], order.index(i)
        assert torch.equal(a, o2[:, :, R.cu_of(l2)[j]:R.cu_of(l2)[j + 1]]), ("sequence", i, "moved to", j)
        assert torch.equal(a, o3[:, :, cu[i]:cu[i + 1]]), ("sequence", i, "beside an added chunk", maxdiff(a, o3[:, :, cu[i]:cu[i + 1]]))


@pytest.mark.parametrize("name,dt,D", [("draft_g4", "bf16", 64), ("draft_g1n32", "fp16", 128), ("draft_clip", "bf16", 80),
                                       ("draft_g4_pad", "fp16", 96)])
def test_trees_against_the_tree_oracle_chains_bitwise_and_the_packed_commit(name, dt, D):
    """contract 5; comb and binary trees on the draft sequences (`draft_clip`: Wc 16 clips the ancestors of a comb of 32)
    against the per-node oracle; contract 3 through commit_seq and commit_packed_dyn with a path"""
    inp = R.pack_inputs(name, "randn", dt, D)
    case, layer, m = inp["case"], PL._pool(inp), _draft_rows(inp["case"])
    lengths, cu = case["lengths"], R.cu_of(case["lengths"])
    par = lambda shape: _parents(lengths, [shape[i % 2](n) if 1 < n <= 64 else chain(n) for i, n in enumerate(lengths)], case["T_PAD"])
    o = _run(layer, inp, "draft").clone()
    assert torch.equal(_run(layer, inp, "draft", parent=par((chain, chain))), o), "a chain-shaped parent"
    parent = par((comb, binary))
    ot = _run(layer, inp, "draft", parent=parent).clone()
    assert _path().startswith("decode_tree_")
    assert torch.equal(ot[:, :, ~m], _run(layer, inp, True, parent=parent)[:, :, ~m])
    ref, keep = {}, torch.zeros_like(m)
    for i in R.live(case):
        L = case["hist"][i]
        if m[cu[i]] and not case["admit"][i]:               # an admitting sequence ignores its tree
            fq, fk, fv = inp["full"][i]
            ref[i] = _oracle_tree(fq[:, :, L:], fk, fv, inp["s_aux"], L, min(L, case["ns"]), case["Wc"], parent[cu[i]:cu[i + 1]])
            keep[cu[i]:cu[i + 1]] = True
    assert len(ref) >= 5
    _check_rows(ot * keep[:, None], ref, lengths, TOL[inp["dtype"]], (name, dt, D, "trees"))
    a, b = _clone(layer), _clone(layer)
    a._pool = b._pool = True
    cs = [0 if m[cu[i]] else 1 for i in range(len(lengths))]
    path = torch.cat([torch.arange(n).flip(0) % max(n, 1) for n in lengths] + [torch.zeros(case["T_PAD"] - cu[-1], dtype=torch.long)])
    for p, flag in ((a, "draft"), (b, False)):
        _run(p, inp, flag, commit=True, parent=parent, commit_seq=_i32(cs))
        k, v = PL._dev(inp)[1:]
        p.commit_packed_dyn(k, v, _i32(cu), _dev_slots(case["slots"]), _i32([2 * (1 - x) for x in cs]), path=_i32(path.tolist()))
    PL._same_pool(a, b, (name, "commit_seq and the packed commit"))


def test_one_captured_graph_while_a_sequence_goes_from_1_to_4_to_9_tokens():
    """decode row -> draft sequence -> split kernel by rewriting cu_q; each replay is bitwise the eager call at that mix"""
    inp = R.pack_inputs("draft_g4", "randn", "bf16", 64)
    case, layer = inp["case"], PL._pool(inp)
    q, k, v = PL._dev(inp)
    sad, so = inp["s_aux"].to(PL.DEV), torch.zeros_like(q)
    mixes = [[n0] + case["lengths"][1:] for n0 in (1, 4, 9)]
    eager = [_run(layer, inp, "draft", lengths=ln).clone() for ln in mixes]
    scu, ssl = _i32(R.cu_of(mixes[0])), _dev_slots(case["slots"])
    graph = torch.cuda.CUDAGraph()                          # the eager calls above have allocated the workspace
    with torch.cuda.graph(graph):
        layer.ragged_step_dyn(q, k, v, scu, ssl, s_aux=sad, out=so, commit=False, admit=True, decode_kernel="draft")
    for ln, want in list(zip(mixes, eager)) * 2:
        scu.copy_(_i32(R.cu_of(ln)))
        graph.replay()
        assert torch.equal(so, want), (ln[0], maxdiff(so, want))
    assert not torch.equal(eager[0], eager[1]) and not torch.equal(eager[1], eager[2])
