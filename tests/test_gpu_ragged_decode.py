"""ragged_step_dyn(decode_kernel=True) (SFA_FLAG_RAGGED_DECODE1), the three contracts of include/sfa.h on
the packs of tests/packed_regime.py and on decode-heavy variants of `walk`: rings wrapped off a tile edge, exactly full (the
evicted slot masked), one short of full, nearly empty, sinks not full, a fresh slot admitted with one token.  The `_pad`
variants add inactive sequences until H_kv n_seq = 2048: want_d = 1, one split, every wave walks 3 to 9 tiles and the LDS
ring wraps."""
import pytest
import torch

import packed_regime as R
import test_gpu_packed_long as PL
import test_gpu_paged_fp8_pool as PF
import test_gpu_paged_pool as PP
from test_gpu_decode_multi import TOL
from test_gpu_fp8_pool import _snap as _snap8, _unmoved as _unmoved8
from test_gpu_ragged_chunk import _ref8
from test_gpu_ragged_tree import _check_rows, _i32, _parents
from test_gpu_slots import _clone, _dev_slots, _path
from test_ragged_tree_host import chain, comb
from util import DECODE_TOL, maxdiff

pytestmark = pytest.mark.gpu
_W, _F = R.PACKS["walk"], R.NS + R.PACKS["walk"]["Wc"]
DEC = R.variant(_W, name="dec_walk", T_PAD=256, S=12, lengths=[1, 1, 1, 1, 1, 1, 1, 0, 3, 160],
                hist=[_F + 37, _F, _F - 1, 9, 2, 0, 50, 20, 100, _F + 5], slots=[3, 0, 5, 2, 9, 8, -1, 6, 1, 7],
                admit=[False] * 5 + [True] + [False] * 4)


def _pad(case, name):
    k = 2048 // case["Hkv"] - len(case["lengths"])
    return R.variant(case, name=name, lengths=case["lengths"] + [0] * k, hist=case["hist"] + [0] * k,
                     slots=case["slots"] + [-1] * k, admit=case["admit"] + [False] * k)


for c in (DEC, _pad(DEC, "dec_walk_pad"), _pad(R.PACKS["capped"], "capped_pad"),
          R.variant(DEC, name="dec_g32", Hkv=2, G=32), R.variant(DEC, name="dec_g5", Hkv=2, G=5)):
    R.PACKS[c["name"]] = c
NAMES = ["walk", "capped", "wide_g1", "admission", "dec_walk", "dec_walk_pad", "capped_pad"]
CASES = [(n, k, dt, D) for n in NAMES for k in ("randn", "probe") for dt, D in PL.TYPES] + \
        [("dec_g32", "randn", "bf16", 64), ("dec_g5", "probe", "fp16", 128)]


def _run(layer, inp, dec, chunk=False, commit=False, parent=None, slots=None, lengths=None, qkv=None, out=None):
    case = inp["case"]
    q, k, v = PL._dev(inp) if qkv is None else qkv
    o = layer.ragged_step_dyn(q, k, v, _i32(R.cu_of(case["lengths"] if lengths is None else lengths)),
                              _dev_slots(case["slots"] if slots is None else slots), s_aux=inp["s_aux"].to(PL.DEV), out=out,
                              commit=commit, admit=any(case["admit"]), parent=None if parent is None else _i32(parent),
                              chunk_kernel=chunk, decode_kernel=dec)
    assert ("_dec1" in _path()) == dec and ("_chunk128" in _path()) == chunk and "_mfma_" in _path(), _path()
    return o


def _dec_rows(case):
    """the rows of the decode sequences; asserts the regime with the plan of packed_regime: S = 1 and >= 3 tiles per wave
    on a padded pack, S >= 3 for the full rings of the others - no case passes empty"""
    cu, m = R.cu_of(case["lengths"]), torch.zeros(case["T_PAD"], dtype=torch.bool)
    S, tiles = [], []
    for i in R.live(case):
        if case["lengths"][i] == 1:
            m[cu[i]] = True
            st = [0, 0, 0, 0] if case["admit"][i] else R.state_after(case["hist"][i], case["ns"], case["Wc"])
            p = R.multi_plan(st[0], st[1], 1, R.want_splits(1, case["Hkv"], len(case["lengths"])))
            S.append(p["S"]), tiles.append(p["T"])
    assert m.any() and not m[:cu[-1]].all()
    if case["name"].endswith("_pad"):
        assert max(S) == 1 and max(tiles) // R.WAVES >= 3, (S, tiles)
    else:
        assert max(S) >= 3, S
    return m.to(PL.DEV)


@pytest.mark.parametrize("name,kind,dt,D", CASES)
def test_oracle_parity_the_other_rows_and_the_storage_of_the_call_without_the_keyword(name, kind, dt, D):
    inp = R.pack_inputs(name, kind, dt, D)
    case, what = inp["case"], (name, kind, dt, D)
    layer, m = PL._pool(inp), _dec_rows(inp["case"])
    base = _run(layer, inp, False).clone()
    _run(layer, inp, True)                                   # allocates the call's own workspace
    layer._ragged_decode_state["ws"].fill_(0xFF)
    o = _run(layer, inp, True, out=torch.full_like(base, float("nan"))).clone()
    _check_rows(o, PL._ref(name, kind, dt, D), case["lengths"], TOL[inp["dtype"]], what)
    assert torch.equal(o[:, :, ~m], base[:, :, ~m]) and not torch.isnan(o).any(), what
    oc, cb = _run(layer, inp, True, chunk=True), _run(layer, inp, False, chunk=True)     # the serving configuration
    assert torch.equal(oc[:, :, ~m], cb[:, :, ~m]) and torch.equal(oc[:, :, m], o[:, :, m]), what
    a, b = _clone(layer), _clone(layer)
    a._pool = b._pool = True
    assert torch.equal(_run(a, inp, True, commit=True), o)
    _run(b, inp, False, commit=True)
    PL._same_pool(a, b, what)
    assert not torch.equal(a._dev_state, layer._dev_state)


@pytest.mark.parametrize("pool,dt,D", [("fp8", "bf16", 80), ("paged", "fp16", 128), ("paged_fp8", "bf16", 64)])
def test_the_other_three_pool_kinds(pool, dt, D):
    """`dec_walk`: the oracle each kind is held to today, the paged pools bitwise their twins, the commit of the default call"""
    inp = R.pack_inputs("dec_walk", "randn", dt, D)
    case, dtype, what = inp["case"], inp["dtype"], (pool, dt, D)
    fp8, M, m = pool != "paged", PF if pool == "paged_fp8" else PP, _dec_rows(inp["case"])
    ref, tol = (_ref8(inp), DECODE_TOL[dtype]) if fp8 else (PL._ref("dec_walk", "randn", dt, D), TOL[dtype])
    base = PL._pool(inp, fp8=fp8)
    for commit in (False, True):
        call = lambda p, flag=True: _run(p, inp, flag, commit=commit)
        if pool == "fp8":
            pg, plain = PL._clone8(base), PL._clone8(base)
            o = call(pg)
        elif fp8:
            make = lambda: PF._paged8(base, dtype, 64, seed=391 + commit, after=PF._ring_after(base, call))
            (pg, tw), (plain, _) = make(), make()            # the same seed: the same table, the same pages
            o = PF._three(pg, tw, dtype, PL._scales(case["Hkv"]), call, what, stores=commit)
        else:
            make = lambda: PP._paged(base, 64, seed=291 + commit, after=PP._ring_after(base, call))
            (pg, tw), (plain, _) = make(), make()
            o = PP._both(pg, tw, call, what, stores=commit)
        _check_rows(o, ref, case["lengths"], tol, what)
        assert torch.equal(o[:, :, ~m], call(plain, False)[:, :, ~m]) and not torch.isnan(o).any(), what
        _unmoved8(plain, _snap8(pg), what) if pool == "fp8" else M._unmoved(plain, M._snap(pg), what)


@pytest.mark.parametrize("name,dt,D", [("dec_walk", "bf16", 64), ("dec_walk_pad", "fp16", 128), ("walk", "bf16", 80)])
def test_a_decode_sequence_gives_the_same_bits_alone_permuted_repeated_and_replayed(name, dt, D):
    """contract 3; the graph: captured with every sequence inactive, replayed at two mixes by rewriting cu_q and slots"""
    inp = R.pack_inputs(name, "randn", dt, D)
    case, layer = inp["case"], PL._pool(inp)
    lengths, slots, cu = case["lengths"], case["slots"], R.cu_of(case["lengths"])
    o = _run(layer, inp, True).clone()
    assert torch.equal(_run(layer, inp, True), o), "repeated"
    for i in [i for i in R.live(case) if lengths[i] == 1]:
        alone = _run(layer, inp, True, slots=[s if j == i else -1 for j, s in enumerate(slots)])
        assert torch.equal(alone[:, :, cu[i]], o[:, :, cu[i]]), ("alone", i, maxdiff(alone[:, :, cu[i]], o[:, :, cu[i]]))
        assert not alone[:, :, :cu[i]].any() and not alone[:, :, cu[i + 1]:].any(), ("alone", i, "other rows must be zero")
    order = [(7 * j + 3) % len(lengths) for j in range(len(lengths))] if len(lengths) % 7 else list(range(len(lengths)))[::-1]
    l2, s2 = [lengths[i] for i in order], [slots[i] for i in order]
    gather = torch.cat([torch.arange(cu[i], cu[i + 1]) for i in order] + [torch.arange(cu[-1], case["T_PAD"])]).to(PL.DEV)
    qkv2 = tuple(t[:, :, gather].contiguous() for t in PL._dev(inp))
    o2 = _run(layer, inp, True, slots=s2, lengths=l2, qkv=qkv2).clone()
    for j, i in enumerate(order):
        a, b = o[:, :, cu[i]:cu[i + 1]], o2[:, :, R.cu_of(l2)[j]:R.cu_of(l2)[j + 1]]
        assert slots[i] < 0 or lengths[i] != 1 or torch.equal(a, b), ("sequence", i, "moved to", j, maxdiff(a, b))
    sq, sk, sv = (torch.zeros_like(t) for t in qkv2)
    scu, ssl = _i32([0] * (len(lengths) + 1)), _dev_slots([-1] * len(lengths))
    so, sad = torch.zeros_like(sq), inp["s_aux"].to(PL.DEV)
    step = lambda: layer.ragged_step_dyn(sq, sk, sv, scu, ssl, s_aux=sad, out=so, commit=False, admit=any(case["admit"]),
                                         decode_kernel=True)
    graph = torch.cuda.CUDAGraph()                          # the eager calls above have allocated the workspace
    with torch.cuda.graph(graph):
        step()
    for qkv, ln, sl, eager in ((PL._dev(inp), lengths, slots, o), (qkv2, l2, s2, o2)):
        for dst, src in zip((sq, sk, sv), qkv):
            dst.copy_(src)
        scu.copy_(_i32(R.cu_of(ln))), ssl.copy_(_dev_slots(sl))
        for _ in range(2):
            graph.replay()
            assert torch.equal(so, eager), maxdiff(so, eager)


def test_with_parent_trees_stay_trees_and_one_token_sequences_stay_decode_sequences_and_groups_are_refused():
    inp = R.pack_inputs("walk", "randn", "bf16", 64)
    case, layer, m = inp["case"], PL._pool(inp), _dec_rows(inp["case"])
    parent = _parents(case["lengths"], [comb(n) if 1 < n <= 64 else chain(n) for n in case["lengths"]], case["T_PAD"])
    o = _run(layer, inp, True, parent=parent).clone()
    assert _path().startswith("decode_tree_")
    assert torch.equal(o[:, :, ~m], _run(layer, inp, False, parent=parent)[:, :, ~m])
    assert torch.equal(o[:, :, m], _run(layer, inp, True)[:, :, m])
    with pytest.raises(ValueError, match="decode_kernel"):
        layer.ragged_step_dyn(*PL._dev(inp), R.cu_of(case["lengths"]), case["slots"], groups=[0, 2], decode_kernel=True)
    with pytest.raises(ValueError, match="decode_kernel"):
        layer.ragged_step_dyn(*PL._dev(inp), R.cu_of(case["lengths"]), case["slots"], force_generic=True, decode_kernel=True)
