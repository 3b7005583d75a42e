"""The packed serving step (ragged_step_dyn with its admit=, parent= and FP8-pool forms) at long caches: waves that walk
several tiles, split counts capped by the call-wide workgroup target, many splits beside few.

Every other packed GPU test runs at Wc in {16, 48}, where a split holds at most 4 tiles, so each of the 4 waves of a
workgroup runs the body of its software-pipelined tile loop once and no sequence plans more than 2 splits
(tests/test_packed_regime.py::test_no_existing_packed_test_gives_a_wave_a_second_tile).  The three packs of
tests/packed_regime.py reach the rest: `walk` (Wc 320, H_kv 8: one split of up to 16 tiles, a wave walks up to 4),
`capped` (Wc 1024, the cap of 4 splits binds: 9 - 10 tiles per split, a shorter last split) and `wide` (Wc 1024, small
T: 9 - 10 splits beside sequences with 1 or 2, 12 launched).  tests/test_packed_regime.py proves on the CPU what the
packs reach and that the probe and softmax-range inputs used here cannot pass on a kernel with a one-key mask error or a
broken rescale; every test below asks packed_regime.regime() again with the device's own state rows and the shapes it
launches before it asserts anything.  Tolerances: TOL of tests/test_gpu_decode_multi.py, DECODE_TOL for the FP8 oracle."""
import math

import pytest
import torch

import packed_regime as R
from fp8_ref import FP8, dequant
from fp8_ref import quant as quant8
from test_gpu_decode_multi import TOL
from test_gpu_fp8_pool import K_SCALE, V_SCALE, _snap, _stored, _unmoved
from test_gpu_fp8_pool import _clone as _clone8
from test_gpu_ragged_admit import _twin_commit
from test_gpu_ragged_tree import _check_rows, _i32, _oracle_tree, _parents
from test_gpu_slots import BUFS, _clone, _dev_slots, _new_pool, _path
from test_ragged_tree_host import chain, comb
from util import DECODE_TOL, maxdiff

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = ["walk", "capped", "wide", "wide_g1"]
MULTI = ["walk", "capped"]
TYPES = [("bf16", 64), ("fp16", 128), ("bf16", 80), ("fp16", 96)]
_REFS = {}


def _ref(name, kind, dt, D, aux=True):
    """the fp64 oracle of every live sequence, computed once per input set"""
    key = (name, kind, dt, D, aux)
    if key not in _REFS:
        inp = R.pack_inputs(name, kind, dt, D)
        _REFS[key] = {i: R.oracle_rows(inp, i, sa=inp["s_aux"] if aux else None) for i in R.live(inp["case"])}
    return _REFS[key]


def _scales(Hkv):
    """the scales of tests/test_gpu_fp8_pool.py, repeated over the KV heads"""
    return [K_SCALE[h % 2] for h in range(Hkv)], [V_SCALE[h % 2] for h in range(Hkv)]


def _pool(inp, fp8=False):
    """A pool in which slot case["slots"][i] holds the history of sequence i: the first num_sink + Wc tokens through
    prefill_slots, the others through one commit_packed_dyn, so that a longer history leaves a wrapped ring with
    write_pos != 0.  Slots of admitting, empty and inactive sequences stay fresh.  The state rows are checked against
    packed_regime.state_after."""
    from sink_attention import SinkCacheLayer
    case, dtype = inp["case"], inp["dtype"]
    ns, wc, Hkv, D = case["ns"], case["Wc"], case["Hkv"], inp["q"].shape[3]
    if fp8:
        layer = SinkCacheLayer(ns, wc)
        layer.init_pool(case["S"], Hkv, D, FP8, DEV)
        layer.set_kv_scale(*_scales(Hkv))
    else:
        layer = _new_pool(ns, wc, case["S"], Hkv, D, dtype)
    seqs = [i for i in R.live(case) if not case["admit"][i]]
    slots = [case["slots"][i] for i in seqs]
    fill = [min(case["hist"][i], ns + wc) for i in seqs]
    cat = lambda x, lo, hi: torch.cat([inp["hist"][i][x][:, :, lo(j):hi(j)] for j, i in enumerate(seqs)], dim=2).to(DEV)
    layer.prefill_slots(cat(0, lambda j: 0, lambda j: fill[j]), cat(1, lambda j: 0, lambda j: fill[j]), R.cu_of(fill), slots)
    extra = [case["hist"][i] - f for i, f in zip(seqs, fill)]
    if any(extra):
        layer.commit_packed_dyn(cat(0, lambda j: fill[j], lambda j: None), cat(1, lambda j: fill[j], lambda j: None),
                                _i32(R.cu_of(extra)), _dev_slots(slots), _i32(extra))
    st = layer._dev_state.tolist()
    for i, s in zip(seqs, slots):
        assert st[s] == R.state_after(case["hist"][i], ns, wc), (i, s, st[s])
    return layer


def _dev(inp):
    if "dev" not in inp:
        inp["dev"] = tuple(inp[x].to(DEV) for x in ("q", "k", "v"))
    return inp["dev"]


def _run(layer, inp, sa="call", commit=False, admit=False, parent=None, slots=None, lengths=None, qkv=None, out=None):
    case = inp["case"]
    q, k, v = _dev(inp) if qkv is None else qkv
    sa = inp["s_aux"] if isinstance(sa, str) else sa
    o = layer.ragged_step_dyn(q, k, v, _i32(R.cu_of(case["lengths"] if lengths is None else lengths)),
                              _dev_slots(case["slots"] if slots is None else slots), s_aux=None if sa is None else sa.to(DEV),
                              out=out, commit=commit, admit=admit, parent=None if parent is None else _i32(parent))
    path = _path()
    assert path.startswith("decode_tree_" if parent is not None else "decode_multi_") and "_ragged" in path, path
    assert ("_admit" in path) == admit and ("_commit" in path) == commit, path
    return o


def _reaches(case, layer, T, slots=None, lengths=None, admit=None):
    """regime() over the state rows the DEVICE holds and the shapes of the launch; asserts what the pack is there for and
    returns the regime.  No test can pass empty: a pool or a pack that misses its regime fails here."""
    st = layer._dev_state.tolist()
    slots = case["slots"] if slots is None else slots
    real = R.variant(case, T_PAD=T, Hkv=layer.window_k.shape[1], Wc=layer.window_size, slots=slots,
                     lengths=case["lengths"] if lengths is None else lengths, admit=case["admit"] if admit is None else admit,
                     states=[st[s] if s >= 0 else [0] * 4 for s in slots])
    rg = R.regime(real)
    assert rg
    walked = max(len(w) for r in rg for w in r["walks"].values())
    if case["name"] in ("walk", "admission"):
        assert rg[0]["want"] == 1 and walked == 4 and max(r["tps"] for r in rg) >= 16, (walked, rg[0]["want"])
    elif case["name"] == "capped":
        assert rg[0]["want"] == 4 and walked == 3 and {r["S"] for r in rg} >= {4} and max(r["tps"] for r in rg) == 10
    else:
        assert rg[0]["Sw"] == 12 and {9, 10, 1, 2} <= {r["S"] for r in rg} and walked == 1
    return rg


def _same_pool(a, b, what):
    for name in BUFS:
        assert torch.equal(getattr(a, name), getattr(b, name)), (what, name)
    assert torch.equal(a._dev_state, b._dev_state), (what, a._dev_state.tolist(), b._dev_state.tolist())


def _mfma(dt, D):
    return dt != "fp32" and D in (64, 80, 96, 128)


# ------------------------------------------------------------------ 1. oracle parity, randn; commit off and on
@pytest.mark.parametrize("name,dt,D", [(n, dt, D) for n in NAMES for dt, D in TYPES] + [("walk", "fp32", 48)])
def test_every_live_row_is_the_oracle_and_a_commit_leaves_what_commit_dyn_leaves(name, dt, D):
    inp = R.pack_inputs(name, "randn", dt, D)
    case, dtype = inp["case"], inp["dtype"]
    layer = _pool(inp)
    rg = _reaches(case, layer, case["T_PAD"])
    before = _clone(layer)
    outs = {}
    for aux in (True, False):
        o = _run(layer, inp, sa=inp["s_aux"] if aux else None)
        assert ("_mfma_" in _path()) == _mfma(dt, D) and (not _mfma(dt, D) or f"_rb{rg[0]['nrb']}_" in _path()), _path()
        _check_rows(o, _ref(name, "randn", dt, D, aux), case["lengths"], TOL[dtype], (name, dt, D, "s_aux", aux))
        _same_pool(layer, before, "commit off: the pool must not move")
        outs[aux] = o
    twin = _clone(layer)
    twin._pool = True
    o2 = _run(layer, inp, commit=True)
    assert torch.equal(o2, outs[True]), maxdiff(o2, outs[True])
    cu = R.cu_of(case["lengths"])
    k, v = _dev(inp)[1:]
    for i in R.live(case):
        n = case["lengths"][i]
        twin.commit_dyn(k[:, :, cu[i]:cu[i] + n], v[:, :, cu[i]:cu[i] + n], torch.full((1,), n, device=DEV), slots=[case["slots"][i]])
    _same_pool(layer, twin, (name, dt, D, "the committed pool is commit_dyn(slots=) per sequence"))


# ------------------------------------------------------------------ 2. mask-edge probes: plain, trees, the admitting form
def _trees(case, shape):
    """per sequence of the pack: `shape` for the sequences a packed tree call reads as trees (n <= 64), a chain elsewhere"""
    return [shape(n) if 1 < n <= 64 else chain(n) for n in case["lengths"]]


@pytest.mark.parametrize("form", ["plain", "chain", "comb", "admit"])
@pytest.mark.parametrize("name", MULTI)
@pytest.mark.parametrize("dt,D", TYPES)
def test_mask_edge_probes(dt, D, name, form):
    """inputs and reference: packed_regime.pack_inputs(kind="probe"), whose CPU proof
    (tests/test_packed_regime.py::test_a_one_key_mask_error_moves_a_probe_row_tenfold) shows that a one-key error at
    the diagonal, the window start, the sink end or the pack edge moves a row by more than 170 tolerances.  chain: the
    (Tree, Ragged) instance on chain-shaped trees, the same reference; comb: comb trees on the sequences of at most 64
    tokens, referenced per node over its root-to-node path; admit: the admitting instance with no fresh slot."""
    inp = R.pack_inputs(name, "probe", dt, D)
    case, dtype = inp["case"], inp["dtype"]
    layer = _pool(inp)
    _reaches(case, layer, case["T_PAD"])
    ref = dict(_ref(name, "probe", dt, D))
    parent = None
    if form in ("chain", "comb"):
        trees = _trees(case, chain if form == "chain" else comb)
        parent = _parents(case["lengths"], trees, case["T_PAD"])
    if form == "comb":
        key = (name, "probe-comb", dt, D)
        if key not in _REFS:
            _REFS[key] = {}
            for i in R.live(case):
                n, L = case["lengths"][i], case["hist"][i]
                if 1 < n <= 64:
                    fq, fk, fv = inp["full"][i]
                    _REFS[key][i] = _oracle_tree(fq[:, :, L:], fk, fv, inp["s_aux"], L, min(L, case["ns"]), case["Wc"], trees[i])
        assert len(_REFS[key]) >= 3
        ref.update(_REFS[key])
    o = _run(layer, inp, parent=parent, admit=form == "admit")
    _check_rows(o, ref, case["lengths"], TOL[dtype], ("probe", name, dt, D, form))


# ------------------------------------------------------------------ 3. softmax-range inputs
@pytest.mark.parametrize("family", ["up", "down", "hill", "offset", "aux_sweep"])
@pytest.mark.parametrize("name", MULTI)
@pytest.mark.parametrize("dt,D", [("bf16", 64), ("fp16", 128)])
def test_softmax_range_inputs(dt, D, name, family):
    """staircases along the chronological key order, a 60 nat offset and s_aux at +-40: every wave that walks two live
    tiles rescales by alpha < 2^-8 in one of the staircases, and rows leave their first tile at m = -inf
    (tests/test_packed_regime.py::test_the_kernel_model_rescales_in_every_walk_and_its_mutants_fail)"""
    inp = R.pack_inputs(name, family, dt, D)
    case = inp["case"]
    layer = _pool(inp)
    _reaches(case, layer, case["T_PAD"])
    o = _run(layer, inp)
    assert "_mfma_" in _path(), _path()
    _check_rows(o, _ref(name, family, dt, D), case["lengths"], TOL[inp["dtype"]], ("range", name, dt, D, family))


# ------------------------------------------------------------------ 4. the plan, read back from the device
@pytest.mark.parametrize("name", NAMES)
def test_the_plan_read_back_from_a_poisoned_workspace(name):
    """One raw C-ABI call: the workspace is exactly sfa_decode_ragged_workspace_bytes bytes inside an allocation filled
    with 0xFF (o too).  Both guard regions keep 0xFF; in the leading partial array ([rows][Sw] f32, rowid = (hk * T +
    packed row) * G + g) entry `split` of a live row is written exactly when split < S of the model, and no entry of any
    other row is; o is bitwise the ordinary call's.  Pins packed_regime's plan to the kernels and fails a split or
    reduce kernel that touches a partial it does not own."""
    from sink_attention import _native as N
    dt, D = "bf16", 64
    inp = R.pack_inputs(name, "randn", dt, D)
    case, dtype = inp["case"], inp["dtype"]
    layer = _pool(inp)
    Hkv, G, T, n_seq = case["Hkv"], case["G"], case["T_PAD"], len(case["lengths"])
    rg = _reaches(case, layer, T)
    geom = R.ragged_geom(n_seq, Hkv * G, Hkv, T, case["ns"] + case["Wc"])
    lib = N.lib()
    need = lib.sfa_decode_ragged_workspace_bytes(n_seq, Hkv * G, Hkv, T, case["ns"] + case["Wc"], D, N.SFA_DTYPE[dtype])
    assert need >= (2 + D) * 4 * geom["rows"] * 1 and need % 256 == 0
    GUARD = 1 << 16
    big = torch.full((GUARD + need + GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
    assert (big.data_ptr() + GUARD) % 256 == 0
    q, k, v = _dev(inp)
    o = torch.empty_like(q)
    o.view(torch.int16).fill_(-1)
    sa = inp["s_aux"].to(DEV)
    cu, slots = _i32(R.cu_of(case["lengths"])), _dev_slots(case["slots"])
    with torch.cuda.device(q.device):
        rc = lib.sfa_decode_ring_ragged_slots(N.desc(q), N.desc(layer.sink_k), N.desc(layer.sink_v), N.desc(layer.window_k),
                                              N.desc(layer.window_v), N.desc(k), N.desc(v), N.desc(o), sa.data_ptr(), 0,
                                              layer._dev_state.data_ptr(), slots.data_ptr(), cu.data_ptr(), n_seq,
                                              big.data_ptr() + GUARD, need, 1.0 / math.sqrt(D), 0, N.stream_ptr(q.device))
    N.check(rc, "sfa_decode_ring_ragged_slots")
    torch.cuda.synchronize()
    assert f"_rb{geom['nrb']}_ragged" in _path() and geom["nrb"] == rg[0]["nrb"], (_path(), geom)
    assert bool((big[:GUARD] == 0xFF).all()) and bool((big[GUARD + need:] == 0xFF).all()), "a guard region was written"
    Sw = geom["Sw"]
    assert geom["rows"] * Sw <= geom["P"]
    written = (big[GUARD:GUARD + geom["rows"] * Sw * 4].view(torch.int32) != -1).view(Hkv, T, G, Sw).cpu()
    cuq = R.cu_of(case["lengths"])
    expect = torch.zeros(T, Sw, dtype=torch.bool)
    S_of = {r["seq"]: r["S"] for r in rg}
    for i, S in S_of.items():
        expect[cuq[i]:cuq[i] + case["lengths"][i]] = torch.arange(Sw) < S
    assert len(S_of) == 7 and max(S_of.values()) == (1 if name == "walk" else 4 if name == "capped" else 10)
    bad = (written != expect.view(1, T, 1, Sw)).nonzero()
    assert not len(bad), ("partials (hk, packed row, g, split) written against the plan", bad[:8].tolist(), S_of)
    assert torch.equal(o, _run(layer, inp)), "the raw call and the ordinary call differ"


# ------------------------------------------------------------------ 5. neighbours do not matter
@pytest.mark.parametrize("name,dt,D", [("walk", "bf16", 64), ("capped", "fp16", 128), ("wide", "bf16", 80), ("wide_g1", "fp16", 96)])
def test_a_sequence_gives_the_same_bits_alone_and_wherever_it_lies(name, dt, D):
    inp = R.pack_inputs(name, "randn", dt, D)
    case = inp["case"]
    layer = _pool(inp)
    _reaches(case, layer, case["T_PAD"])
    lengths, slots, cu = case["lengths"], case["slots"], R.cu_of(case["lengths"])
    o = _run(layer, inp).clone()
    for i in (0, 3, 6):                   # decode on a wrapped ring, a chunk with the wrap inside a tile, the long chunk
        alone = _run(layer, inp, slots=[s if j == i else -1 for j, s in enumerate(slots)])
        rows = slice(cu[i], cu[i] + lengths[i])
        assert torch.equal(alone[:, :, rows], o[:, :, rows]), ("alone", i, maxdiff(alone[:, :, rows], o[:, :, rows]))
        alone[:, :, rows] = 0
        assert not alone.any(), ("alone", i, "every other row must be zero")
    order = [6, 2, 0, 8, 3, 7, 1, 5, 4]
    l2 = [lengths[i] for i in order]
    cu2 = R.cu_of(l2)
    gather = torch.cat([torch.arange(cu[i], cu[i] + lengths[i]) for i in order] + [torch.arange(cu[-1], case["T_PAD"])]).to(DEV)
    o2 = _run(layer, inp, slots=[slots[i] for i in order], lengths=l2, qkv=tuple(t[:, :, gather] for t in _dev(inp)))
    for j, i in enumerate(order):
        a, b = o[:, :, cu[i]:cu[i] + lengths[i]], o2[:, :, cu2[j]:cu2[j] + l2[j]]
        if slots[i] >= 0:
            assert torch.equal(a, b), ("sequence", i, "moved to", j, maxdiff(a, b))


# ------------------------------------------------------------------ 6. the FP8 pool
def _dequant_pool(p8, inp):
    """the 16-bit pool of the read equality: (codes.float() * scale).to(dtype) in every buffer, the same state"""
    case = inp["case"]
    sc = _scales(case["Hkv"])
    pd = _new_pool(case["ns"], case["Wc"], case["S"], case["Hkv"], inp["q"].shape[3], inp["dtype"])
    for name in BUFS:
        getattr(pd, name).copy_(dequant(getattr(p8, name).cpu(), sc[0 if name.endswith("_k") else 1], inp["dtype"]).to(DEV))
    pd._dev_state.copy_(p8._dev_state)
    return pd


@pytest.mark.parametrize("name,dt,D", [("walk", "bf16", 64), ("walk", "fp16", 128), ("capped", "bf16", 80), ("capped", "fp16", 96),
                                       ("wide", "bf16", 64), ("wide_g1", "fp16", 128)])
def test_fp8_pool_read_equality_oracle_and_storage_equality(name, dt, D):
    inp = R.pack_inputs(name, "randn", dt, D)
    case, dtype = inp["case"], inp["dtype"]
    sc = _scales(case["Hkv"])
    p8, p16 = _pool(inp, fp8=True), _pool(inp)
    _reaches(case, p8, case["T_PAD"])
    pd = _dequant_pool(p8, inp)
    comb_par = _parents(case["lengths"], _trees(case, comb), case["T_PAD"])
    # read equality: o over the codes is bitwise o over a 16-bit pool of the dequantised codes, in every form
    plain = None
    for parent, admit in ((None, False), (comb_par, False), (None, True), (comb_par, True)):
        before = _snap(p8)
        o8 = _run(p8, inp, parent=parent, admit=admit)
        path = _path()
        assert "_mfma_" in path and path.endswith("_kvfp8"), path
        od = _run(pd, inp, parent=parent, admit=admit)
        assert _path() == path[:-len("_kvfp8")], (_path(), path)
        diff = (o8 != od).any(dim=(0, 1, 3)).nonzero().flatten().tolist()
        assert torch.equal(o8, od), (name, "tree", parent is not None, "admit", admit, "packed rows", diff[:8])
        _unmoved(p8, before, "commit off: the pool must not move")
        plain = o8.clone() if plain is None else plain
    # the oracle over the dequantised history
    deq = lambda t, x: dequant(quant8(t, sc[x]), sc[x], dtype)
    inp8 = dict(inp, full={i: (fq, torch.cat([deq(fk[:, :, :case["hist"][i]], 0), fk[:, :, case["hist"][i]:]], dim=2),
                               torch.cat([deq(fv[:, :, :case["hist"][i]], 1), fv[:, :, case["hist"][i]:]], dim=2))
                           for i, (fq, fk, fv) in inp["full"].items()})
    ref8 = {i: R.oracle_rows(inp8, i) for i in R.live(case)}
    _check_rows(plain, ref8, case["lengths"], DECODE_TOL[dtype], ("fp8 pool", name, dt, D))
    # storage equality of a committing step: every row the 16-bit pool gets is stored as its quantised codes
    s8, s16 = _snap(p8), _snap(p16)
    oc = _run(p8, inp, commit=True)
    assert _path().endswith("_commit_kvfp8") and torch.equal(oc, plain), _path()
    _run(p16, inp, commit=True)
    rows = _stored(p8, p16, s8, s16, sc, ("committing step", name, dt, D))
    assert rows >= 2 * case["Hkv"] * 300, rows


# ------------------------------------------------------------------ 7. admission at depth
@pytest.mark.parametrize("dt,D", [("bf16", 64), ("fp16", 128), ("fp32", 48)])
def test_a_fresh_slot_admitted_with_700_tokens(dt, D):
    """22 chunk tiles in one split: tile 0 holds the sinks, the late row blocks step over the chunk tiles behind their
    window.  Every row against the oracle (the admitted sequence: a prefill of its own tokens); state rows and pool
    bitwise prefill_slots of the admitted tokens and commit_dyn of the others."""
    inp = R.pack_inputs("admission", "randn", dt, D)
    case, dtype = inp["case"], inp["dtype"]
    layer = _pool(inp)
    rg = _reaches(case, layer, case["T_PAD"])
    adm = [r for r in rg if r["seq"] == 0]
    assert adm[0]["plan"]["T"] == 22 and adm[0]["nsk"] == 4 and any(r["skipped"][(0, 0)] for r in adm)
    twin = _clone(layer)
    twin._pool = True
    before = _clone(layer)
    o = _run(layer, inp, admit=True)
    _check_rows(o, _ref("admission", "randn", dt, D), case["lengths"], TOL[dtype], ("admission", dt, D))
    _same_pool(layer, before, "commit off: the pool must not move")
    o2 = _run(layer, inp, admit=True, commit=True)
    assert torch.equal(o, o2)
    _twin_commit(twin, inp["k"], inp["v"], list(zip(case["lengths"], case["slots"], case["admit"])))
    _same_pool(layer, twin, ("admission", dt, D))
    assert layer._dev_state[6].tolist() == [4, 320, 0, 700]


# ------------------------------------------------------------------ 8. one captured graph, three mixes
def test_one_captured_graph_replays_at_three_mixes():
    """the capped geometry captured once (release, then an admitting and committing step) and replayed at: decode rows on
    low fills (S = 1 everywhere), the pack of the table (S = 4, waves walk 3 tiles), a mix with a slot released and
    readmitted in the same iteration.  Each replay is bitwise the eager run: o, pool and state."""
    name, dt, D = "capped", "bf16", 64
    inp = R.pack_inputs(name, "randn", dt, D)
    case, dtype = inp["case"], inp["dtype"]
    layer = _pool(inp)
    T, n_seq, Hq, Hkv = case["T_PAD"], len(case["lengths"]), case["Hkv"] * case["G"], case["Hkv"]
    sq = torch.zeros(1, Hq, T, D, dtype=dtype, device=DEV)
    sk, sv = (torch.zeros(1, Hkv, T, D, dtype=dtype, device=DEV) for _ in range(2))
    scu = torch.zeros(n_seq + 1, dtype=torch.int32, device=DEV)
    ssl = torch.full((n_seq,), -1, dtype=torch.int32, device=DEV)
    srel = torch.full((2,), -1, dtype=torch.int32, device=DEV)
    so = torch.zeros_like(sq)
    sad = inp["s_aux"].to(DEV)

    def step(p, out):
        p.release_slots(srel)
        return p.ragged_step_dyn(sq, sk, sv, scu, ssl, s_aux=sad, out=out, commit=True, admit=True)

    start = _clone(layer)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):         # warm-up outside the capture (allocates the workspace); all rows inactive
        step(layer, so)
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(layer, so)
    _same_pool(layer, start, "warm-up and capture with every sequence inactive")
    pad = lambda x, fill: x + [fill] * (n_seq - len(x))
    # (lengths, slots, released, admitting): slots 7 and 4 hold 9 and 2 tokens; slot 5 is released and readmitted with 40
    mixes = [(pad([1, 1], 0), pad([7, 4], -1), [-1, -1], None),
             (case["lengths"], case["slots"], [-1, -1], None),
             (pad([40, 1, 70], 0), pad([5, 3, 2], -1), [5, -1], 0)]
    g = torch.Generator().manual_seed(808)
    for r, (lengths, slots, rel, adm) in enumerate(mixes):
        if r == 1:
            q, k, v = inp["q"], inp["k"], inp["v"]
        else:
            q, k, v = (R.RI._rand(tuple(inp[x].shape), g, dtype) for x in ("q", "k", "v"))
        sq.copy_(q), sk.copy_(k), sv.copy_(v), srel.copy_(torch.tensor(rel, dtype=torch.int32))
        scu.copy_(torch.tensor(R.cu_of(lengths), dtype=torch.int32)), ssl.copy_(torch.tensor(slots, dtype=torch.int32))
        if adm is not None:      # the regime as the step will see it: the released slot reads as fresh
            layer_after = _clone(layer)
            layer_after._pool = True
            layer_after.release_slots(srel)
        admit = [j == adm for j in range(n_seq)]
        real = R.variant(case, lengths=lengths, slots=slots, admit=admit,
                         states=[(layer_after if adm is not None else layer)._dev_state[s].tolist() if s >= 0 else [0] * 4 for s in slots])
        rg = R.regime(real)
        if r == 0:
            assert len(rg) == 2 and all(x["S"] == 1 for x in rg)
        else:
            assert max(x["S"] for x in rg) == 4 and max(len(w) for x in rg for w in x["walks"].values()) == 3
        twin = _clone(layer)
        twin._pool = True
        before = layer._dev_state.clone()
        graph.replay()
        oe = step(twin, None)
        assert torch.equal(so, oe), ("replay", r, maxdiff(so, oe))
        _same_pool(layer, twin, ("replay", r))
        assert not torch.equal(layer._dev_state, before), ("replay", r, "the step moved the pool")
        assert so[:, :, :R.cu_of(lengths)[-1]].any()
    assert layer._dev_state[5].tolist() == [4, 36, 36, 40]            # released, then admitted with 40 tokens


# ------------------------------------------------------------------ 9. determinism
def test_two_runs_and_two_committing_runs_give_the_same_bits():
    inp = R.pack_inputs("capped", "randn", "bf16", 64)
    case = inp["case"]
    p8 = _pool(inp, fp8=True)
    _reaches(case, p8, case["T_PAD"])
    o1 = _run(p8, inp).clone()
    o2 = _run(p8, inp)
    assert torch.equal(o1, o2)
    a, b = _clone8(p8), _clone8(p8)
    oa, ob = _run(a, inp, commit=True), _run(b, inp, commit=True)
    assert torch.equal(oa, ob) and torch.equal(oa, o1)
    _unmoved(a, _snap(b), "two committing runs leave the same bytes")
    assert not torch.equal(a._dev_state, p8._dev_state)
