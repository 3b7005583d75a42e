"""ragged_step_dyn(chunk_kernel=True) (SFA_FLAG_RAGGED_CHUNK128), the three contracts of include/sfa.h on
the packs of tests/packed_regime.py: `walk` (four rounds per split, both LDS sets, last blocks with 4 / 2 / 2 / 1 live
waves), `capped` (partial last rounds), `wide_g1` (G = 1; EDGE: lengths 128 and 127) and the admission of 700 tokens."""
import pytest
import torch

import packed_regime as R
import test_gpu_packed_long as PL
import test_gpu_paged_fp8_pool as PF
import test_gpu_paged_pool as PP
from fp8_ref import dequant, quant
from test_gpu_decode_multi import TOL
from test_gpu_fp8_pool import _snap as _snap8, _unmoved as _unmoved8
from test_gpu_ragged_tree import _check_rows, _i32, _parents
from test_gpu_slots import _clone, _dev_slots, _path
from sink_attention import _native as N
from test_ragged_chunk_host import wblk_rule
from test_ragged_tree_host import chain, comb
from util import DECODE_TOL, maxdiff

pytestmark = pytest.mark.gpu
EDGE = "wide_g1_edge"
R.PACKS[EDGE] = R.variant(R.PACKS["wide_g1"], name=EDGE, lengths=[1, 3, 8, 127, 2, 1, 128, 0, 33])
NAMES = ["walk", "capped", "wide_g1", EDGE, "admission"]


def _run(layer, inp, chunk, commit=False, parent=None, slots=None, lengths=None, qkv=None, out=None):
    case = inp["case"]
    q, k, v = PL._dev(inp) if qkv is None else qkv
    o = layer.ragged_step_dyn(q, k, v, _i32(R.cu_of(case["lengths"] if lengths is None else lengths)),
                              _dev_slots(case["slots"] if slots is None else slots), s_aux=inp["s_aux"].to(PL.DEV), out=out,
                              commit=commit, admit=any(case["admit"]), parent=None if parent is None else _i32(parent),
                              chunk_kernel=chunk)
    assert ("_ragged_chunk128" in _path()) == chunk and "_mfma_" in _path(), _path()
    return o


def _chunk_rows(case, tree=False):
    cu, m = R.cu_of(case["lengths"]), torch.zeros(case["T_PAD"], dtype=torch.bool)
    for i, n in enumerate(case["lengths"]):
        m[cu[i]:cu[i + 1]] = case["G"] * n >= 128 and (not tree or n > 64)
    assert m.any() and not m[:cu[-1]].all()
    return m.to(PL.DEV)


def _others_unmoved(case, o, base, what, tree=False):
    m = _chunk_rows(case, tree)
    assert torch.equal(o[:, :, ~m], base[:, :, ~m]) and not torch.isnan(o).any(), what


@pytest.mark.parametrize("name,kind,dt,D", [(n, k, dt, D) for n in NAMES for k in ("randn", "probe") for dt, D in PL.TYPES] +
                         [("walk", f, dt, D) for f in ("up", "down") for dt, D in (("bf16", 64), ("fp16", 128))])
def test_oracle_parity_and_the_storage_of_the_call_without_the_keyword(name, kind, dt, D):
    inp = R.pack_inputs(name, kind, dt, D)
    case, what = inp["case"], (name, kind, dt, D)
    layer = PL._pool(inp)
    base = _run(layer, inp, False).clone()
    _run(layer, inp, True)                                   # allocates the call's own workspace
    layer._ragged_chunk_state["ws"].fill_(0xFF)
    o = _run(layer, inp, True, out=torch.full_like(base, float("nan")))
    _check_rows(o, PL._ref(name, kind, dt, D), case["lengths"], TOL[inp["dtype"]], what)
    _others_unmoved(case, o, base, what)
    G, T = case["G"], case["T_PAD"]        # the device's block table, behind the ungrouped workspace, against the rule
    off = N.lib().sfa_decode_ragged_workspace_bytes(len(case["lengths"]), case["Hkv"] * G, case["Hkv"], T,
                                                    case["ns"] + case["Wc"], D, N.SFA_DTYPE[inp["dtype"]])
    rule = wblk_rule(G, case["lengths"], T)
    assert layer._ragged_chunk_state["ws"][off:off + 8 * len(rule)].view(torch.int32).view(-1, 2).tolist() == rule
    a, b = _clone(layer), _clone(layer)
    a._pool = b._pool = True
    assert torch.equal(_run(a, inp, True, commit=True), o)
    _run(b, inp, False, commit=True)
    PL._same_pool(a, b, what)
    assert not torch.equal(a._dev_state, layer._dev_state)


def _ref8(inp):
    case, sc = inp["case"], PL._scales(inp["case"]["Hkv"])
    deq = lambda t, i, x: torch.cat([dequant(quant(t[:, :, :case["hist"][i]], sc[x]), sc[x], inp["dtype"]), t[:, :, case["hist"][i]:]], dim=2)
    inp8 = dict(inp, full={i: (fq, deq(fk, i, 0), deq(fv, i, 1)) for i, (fq, fk, fv) in inp["full"].items()})
    return {i: R.oracle_rows(inp8, i) for i in R.live(case)}


@pytest.mark.parametrize("pool,dt,D", [("fp8", "bf16", 80), ("paged", "fp16", 128), ("paged_fp8", "bf16", 64)])
def test_the_other_three_pool_kinds(pool, dt, D):
    """`walk`: the oracle each kind is held to today, the paged pools bitwise their twins, the commit of the default call"""
    inp = R.pack_inputs("walk", "randn", dt, D)
    case, dtype, what = inp["case"], inp["dtype"], (pool, dt, D)
    fp8, M = pool != "paged", PF if pool == "paged_fp8" else PP
    ref, tol = (_ref8(inp), DECODE_TOL[dtype]) if fp8 else (PL._ref("walk", "randn", dt, D), TOL[dtype])
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
        _others_unmoved(case, o, call(plain, False), what)
        _unmoved8(plain, _snap8(pg), what) if pool == "fp8" else M._unmoved(plain, M._snap(pg), what)


@pytest.mark.parametrize("name,dt,D", [("walk", "bf16", 64), ("capped", "fp16", 128), ("wide_g1", "bf16", 80)])
def test_a_chunk_sequence_gives_the_same_bits_alone_permuted_repeated_and_replayed(name, dt, D):
    """contract 3; the graph: captured with every sequence inactive, replayed at two mixes by rewriting cu_q and slots"""
    inp = R.pack_inputs(name, "randn", dt, D)
    case, layer = inp["case"], PL._pool(inp)
    lengths, slots, cu = case["lengths"], case["slots"], R.cu_of(case["lengths"])
    o = _run(layer, inp, True).clone()
    assert torch.equal(_run(layer, inp, True), o), "repeated"
    for i in [i for i, n in enumerate(lengths) if case["G"] * n >= 128]:
        alone = _run(layer, inp, True, slots=[s if j == i else -1 for j, s in enumerate(slots)])
        rows = slice(cu[i], cu[i + 1])
        assert torch.equal(alone[:, :, rows], o[:, :, rows]), ("alone", i, maxdiff(alone[:, :, rows], o[:, :, rows]))
        assert not alone[:, :, :cu[i]].any() and not alone[:, :, cu[i + 1]:].any(), ("alone", i, "other rows must be zero")
    order = [6, 2, 0, 8, 3, 7, 1, 5, 4]
    l2, s2 = [lengths[i] for i in order], [slots[i] for i in order]
    gather = torch.cat([torch.arange(cu[i], cu[i + 1]) for i in order] + [torch.arange(cu[-1], case["T_PAD"])]).to(PL.DEV)
    qkv2 = tuple(t[:, :, gather].contiguous() for t in PL._dev(inp))
    o2 = _run(layer, inp, True, slots=s2, lengths=l2, qkv=qkv2).clone()
    for j, i in enumerate(order):
        a, b = o[:, :, cu[i]:cu[i + 1]], o2[:, :, R.cu_of(l2)[j]:R.cu_of(l2)[j + 1]]
        assert slots[i] < 0 or torch.equal(a, b), ("sequence", i, "moved to", j, maxdiff(a, b))
    sq, sk, sv = (torch.zeros_like(t) for t in qkv2)
    scu, ssl = _i32([0] * (len(lengths) + 1)), _dev_slots([-1] * len(lengths))
    so, sad = torch.zeros_like(sq), inp["s_aux"].to(PL.DEV)
    step = lambda: layer.ragged_step_dyn(sq, sk, sv, scu, ssl, s_aux=sad, out=so, commit=False, chunk_kernel=True)
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


def test_with_parent_a_long_sequence_is_a_chunk_and_a_possible_tree_is_not_and_groups_are_refused():
    """the 70- / 160-token sequences ignore `parent` (bitwise the chunk call without it); the 40-token comb tree stays a tree"""
    inp = R.pack_inputs("walk", "randn", "bf16", 64)
    case, layer = inp["case"], PL._pool(inp)
    parent = _parents(case["lengths"], [comb(n) if 1 < n <= 64 else chain(n) for n in case["lengths"]], case["T_PAD"])
    m = _chunk_rows(case, tree=True)
    assert int(m.sum()) == 70 + 160 and 40 in case["lengths"]
    o = _run(layer, inp, True, parent=parent).clone()
    assert _path().startswith("decode_tree_")
    _others_unmoved(case, o, _run(layer, inp, False, parent=parent), "parent", tree=True)
    assert torch.equal(o[:, :, m], _run(layer, inp, True)[:, :, m])
    with pytest.raises(ValueError, match="chunk_kernel"):
        layer.ragged_step_dyn(*PL._dev(inp), R.cu_of(case["lengths"]), case["slots"], groups=[0, 2], chunk_kernel=True)
