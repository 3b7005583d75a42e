"""ragged_step_dyn(decode_kernel=True, raw_fp8=True) (SFA_FLAG_RAGGED_DECODE1_RAW8) on the decode packs of
tests/test_gpu_ragged_decode.py, FP8 and paged FP8 pools.  Every call under test runs on a 0xFF workspace into a NaN `out`
and asserts the `_dec1raw` path.  The sharp test is the second: at power-of-two scales the folded scales round exactly as
T(code * s) does, so the decode rows must be the bits of decode_kernel=True alone."""
import pytest
import torch

import packed_regime as R
import test_gpu_packed_long as PL
import test_gpu_paged_fp8_pool as PF
import test_gpu_ragged_decode as RD
from test_gpu_ragged_chunk import _ref8
from test_gpu_ragged_tree import _check_rows, _i32, _parents
from test_gpu_slots import _dev_slots, _path
from test_ragged_tree_host import chain, comb
from util import DECODE_TOL, maxdiff

pytestmark = pytest.mark.gpu
POW2 = lambda Hkv: ([(0.25, 2.0, 1.0, 0.5)[h % 4] for h in range(Hkv)], [(1.0, 0.5, 2.0, 0.25)[h % 4] for h in range(Hkv)])


def _run(layer, inp, raw=True, dec=True, chunk=False, commit=False, parent=None, slots=None, lengths=None, qkv=None):
    case = inp["case"]
    q, k, v = PL._dev(inp) if qkv is None else qkv
    call = lambda out, commit: layer.ragged_step_dyn(
        q, k, v, _i32(R.cu_of(case["lengths"] if lengths is None else lengths)), _dev_slots(case["slots"] if slots is None else slots),
        s_aux=inp["s_aux"].to(PL.DEV), out=out, commit=commit, admit=any(case["admit"]), parent=None if parent is None else _i32(parent),
        chunk_kernel=chunk, decode_kernel=dec, raw_fp8=raw)
    out = None
    if raw:
        out = torch.full_like(call(None, False), float("nan"))          # allocates the keyword's own workspace
        getattr(layer, "_ragged_raw8_chunk_state" if chunk else "_ragged_raw8_state")["ws"].fill_(0xFF)
    o = call(out, commit)
    p = _path()
    assert ("_dec1raw" in p) == raw and ("_dec1" in p) == dec and ("_chunk128" in p) == chunk and "_mfma_" in p, p
    return o.clone()


def _fresh(base, pool, inp, call, seed):
    """a pool holding base's codes: a contiguous FP8 clone, or (paged FP8 pool, contiguous twin) with the ring `call` reaches mapped"""
    if pool == "fp8":
        return PL._clone8(base), None
    return PF._paged8(base, inp["dtype"], 64, seed=seed, after=PF._ring_after(base, call))


ORACLE = [("fp8", "dec_walk", "randn", "bf16", 64), ("paged_fp8", "dec_walk", "probe", "fp16", 128),
          ("fp8", "dec_walk_pad", "probe", "bf16", 80), ("paged_fp8", "dec_walk_pad", "randn", "fp16", 96),
          ("fp8", "capped_pad", "randn", "fp16", 128), ("fp8", "capped_pad", "probe", "bf16", 64),
          ("paged_fp8", "dec_g32", "randn", "fp16", 80), ("paged_fp8", "dec_g5", "probe", "bf16", 96),
          ("fp8", "dec_walk", "probe", "fp16", 64), ("paged_fp8", "dec_walk", "randn", "bf16", 128)]


@pytest.mark.parametrize("pool,name,kind,dt,D", ORACLE)
def test_the_fp64_oracle_over_the_dequantised_codes_at_scales_that_are_no_powers_of_two(pool, name, kind, dt, D):
    inp = R.pack_inputs(name, kind, dt, D)
    case, what, m = inp["case"], (pool, name, kind, dt, D), RD._dec_rows(inp["case"])
    pg, tw = _fresh(PL._pool(inp, fp8=True), pool, inp, lambda p: _run(p, inp), 491)
    o = _run(pg, inp)
    _check_rows(o, _ref8(inp), case["lengths"], DECODE_TOL[inp["dtype"]], what)
    assert torch.equal(o[:, :, ~m], _run(pg, inp, raw=False)[:, :, ~m]) and not torch.isnan(o).any(), what
    assert tw is None or torch.equal(o, _run(tw, inp)), (what, "the paged FP8 pool against its contiguous twin")


@pytest.mark.parametrize("pool,name,dt,D", [(p, n, dt, D) for p, (n, dt, D) in zip(
    ["fp8", "paged_fp8"] * 3, [("dec_walk", "bf16", 128), ("dec_walk", "fp16", 80), ("dec_walk_pad", "fp16", 64),
                               ("dec_walk_pad", "bf16", 96), ("dec_g32", "fp16", 128), ("dec_g32", "bf16", 64)])])
def test_bitwise_the_register_path_at_power_of_two_scales(pool, name, dt, D):
    inp = R.pack_inputs(name, "randn", dt, D)
    what, m, base = (pool, name, dt, D), RD._dec_rows(inp["case"]), PL._pool(inp, fp8=True)
    base.set_kv_scale(*POW2(inp["case"]["Hkv"]))
    pg, tw = _fresh(base, pool, inp, lambda p: _run(p, inp), 492)
    o, ref = _run(pg, inp), _run(pg, inp, raw=False)
    assert tw is None or torch.equal(o, _run(tw, inp)), (what, "the paged FP8 pool against its contiguous twin")
    bad = (o != ref).any(dim=(0, 1, 3)).nonzero().flatten().tolist()
    assert torch.equal(o, ref) and m.any(), (what, "packed rows", bad[:8], maxdiff(o, ref))


@pytest.mark.parametrize("pool,dt,D", [("fp8", "fp16", 96), ("paged_fp8", "bf16", 128)])
def test_the_rest_of_the_call_chunk_kernel_admit_parent_and_the_commit_of_the_default_call(pool, dt, D):
    inp = R.pack_inputs("dec_walk", "randn", dt, D)               # admits a fresh slot with one token
    case, what, m = inp["case"], (pool, dt, D), RD._dec_rows(inp["case"])
    base = PL._pool(inp, fp8=True)
    commit = lambda p, raw=True: _run(p, inp, raw=raw, dec=raw, commit=True)
    (pg, _), (a, _), (b, _) = (_fresh(base, pool, inp, commit, 493) for _ in range(3))
    o = _run(pg, inp)
    oc, cb = _run(pg, inp, chunk=True), _run(pg, inp, raw=False, dec=False, chunk=True)
    assert torch.equal(oc[:, :, ~m], cb[:, :, ~m]) and torch.equal(oc[:, :, m], o[:, :, m]), what
    parent = _parents(case["lengths"], [comb(n) if 1 < n <= 64 else chain(n) for n in case["lengths"]], case["T_PAD"])
    op = _run(pg, inp, parent=parent)
    assert _path().startswith("decode_tree_") and torch.equal(op[:, :, m], o[:, :, m]), what
    assert torch.equal(op[:, :, ~m], _run(pg, inp, raw=False, dec=False, parent=parent)[:, :, ~m]), what
    assert torch.equal(commit(a), o)
    commit(b, False)
    for x in PF.BUFS:
        assert torch.equal(PF._u8(getattr(a, x)), PF._u8(getattr(b, x))), (what, x)
    assert torch.equal(a._dev_state, b._dev_state) and not torch.equal(a._dev_state, pg._dev_state), what


@pytest.mark.parametrize("pool,name,dt,D", [("fp8", "dec_walk", "bf16", 80), ("paged_fp8", "dec_walk_pad", "fp16", 128)])
def test_a_decode_sequence_gives_the_same_bits_alone_permuted_repeated_and_replayed(pool, name, dt, D):
    inp = R.pack_inputs(name, "randn", dt, D)
    case = inp["case"]
    layer, _ = _fresh(PL._pool(inp, fp8=True), pool, inp, lambda p: _run(p, inp), 494)
    lengths, slots, cu = case["lengths"], case["slots"], R.cu_of(case["lengths"])
    o = _run(layer, inp)
    assert torch.equal(_run(layer, inp), o), "repeated"
    for i in [i for i in R.live(case) if lengths[i] == 1]:
        alone = _run(layer, inp, slots=[s if j == i else -1 for j, s in enumerate(slots)])
        assert torch.equal(alone[:, :, cu[i]], o[:, :, cu[i]]), ("alone", i, maxdiff(alone[:, :, cu[i]], o[:, :, cu[i]]))
    order = [(7 * j + 3) % len(lengths) for j in range(len(lengths))] if len(lengths) % 7 else list(range(len(lengths)))[::-1]
    l2, s2 = [lengths[i] for i in order], [slots[i] for i in order]
    gather = torch.cat([torch.arange(cu[i], cu[i + 1]) for i in order] + [torch.arange(cu[-1], case["T_PAD"])]).to(PL.DEV)
    qkv2 = tuple(t[:, :, gather].contiguous() for t in PL._dev(inp))
    o2 = _run(layer, inp, slots=s2, lengths=l2, qkv=qkv2)
    for j, i in enumerate(order):
        a, b = o[:, :, cu[i]:cu[i + 1]], o2[:, :, R.cu_of(l2)[j]:R.cu_of(l2)[j + 1]]
        assert slots[i] < 0 or lengths[i] != 1 or torch.equal(a, b), ("sequence", i, "moved to", j, maxdiff(a, b))
    sq, sk, sv = (torch.zeros_like(t) for t in qkv2)
    scu, ssl = _i32([0] * (len(lengths) + 1)), _dev_slots([-1] * len(lengths))
    so, sad = torch.zeros_like(sq), inp["s_aux"].to(PL.DEV)
    step = lambda: layer.ragged_step_dyn(sq, sk, sv, scu, ssl, s_aux=sad, out=so, commit=False, admit=any(case["admit"]),
                                         decode_kernel=True, raw_fp8=True)
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


def test_the_refusals():
    inp = R.pack_inputs("dec_walk", "randn", "bf16", 64)
    args = lambda: (*PL._dev(inp), R.cu_of(inp["case"]["lengths"]), inp["case"]["slots"])
    p8, p16 = PL._pool(inp, fp8=True), PL._pool(inp)
    with pytest.raises(ValueError, match="raw_fp8"):
        p8.ragged_step_dyn(*args(), raw_fp8=True)
    with pytest.raises(TypeError, match="raw_fp8"):
        p16.ragged_step_dyn(*args(), decode_kernel=True, raw_fp8=True)
    for kw in (dict(groups=[0, 2]), dict(force_generic=True)):
        with pytest.raises(ValueError, match="decode_kernel"):
            p8.ragged_step_dyn(*args(), decode_kernel=True, raw_fp8=True, **kw)
