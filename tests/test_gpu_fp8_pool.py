"""FP8 (OCP e4m3fn) slot pool: prefill_slots, ragged_step_dyn, commit_packed_dyn and fork_slots on a pool whose buffers
hold one byte per element (sfa_ring_fill_varlen_fp8_slots, sfa_decode_ring_ragged_fp8_slots,
sfa_ring_commit_path_ragged_fp8_slots, sfa_ring_copy_slots).  The contract is two bitwise equalities (include/sfa.h,
restated in tests/fp8_ref.py), so no test here has a tolerance of its own:

  storage  every row a storing call writes holds quant(the 16-bit row the same call writes into a 16-bit twin pool), every
           other row keeps its bytes, the state rows are equal;
  read     o on the FP8 pool is bit for bit o of the same step on a 16-bit pool holding dequant(codes).

The oracle test runs the fp64 oracle of tests/test_gpu_ragged_tree.py over dequant(quant(history)) at the existing
DECODE_TOL: quantisation is part of the input.  Geometry of tests/test_gpu_ragged_tree.py: a pool of 8 slots, H_kv = 2,
num_sink = 4, Wc in {16, 48}, lengths [1, 7, 0, 16, 33, 64, 70] padded to T = 200, the slot fills of its _pool(), an
inactive sequence.  Scales K = [0.37, 2.0], V = [1.0, 0.25]: different per head and between K and V, so a wrong index or
a K / V swap fails; within [2^-3, 2^2], so no f16 subnormal enters."""
import pytest
import torch

from fp8_ref import FP8, dequant, quant
from sink_attention import SinkCacheLayer, spec_tree
from test_gpu_ragged_tree import (HKV, NS, PERM_HOLE, S, T_PAD, _check_rows, _cu, _i32, _mix_a, _oracle, _pack, _parents,
                                  _run)
from test_gpu_slots import BUFS, _dev_slots, _path
from test_ragged_tree_host import LENGTHS, binary, chain, comb, rand_tree, star
from util import DECODE_TOL, rand

pytestmark = pytest.mark.gpu
DEV = "cuda"
K_SCALE, V_SCALE = [0.37, 2.0], [1.0, 0.25]
SCALES = (K_SCALE, V_SCALE)
# every row-chunk count (D / 16 = 4, 5, 6, 8) once
CASES = [(torch.bfloat16, 64, 8), (torch.float16, 80, 1), (torch.bfloat16, 96, 1), (torch.float16, 128, 8)]
GRID = [(dt, D, G, W, SCALES) for dt, D, G in CASES for W in (16, 48)] + [(torch.bfloat16, 64, 8, 16, None)]
ORACLE = [(torch.bfloat16, 64, 8, 16), (torch.float16, 80, 1, 48), (torch.bfloat16, 96, 1, 16), (torch.float16, 128, 8, 48)]
BIG = 2000.0            # |BIG| / scale > 448 for every scale here; exact in bf16 and f16


def _row(scales, name):
    return None if scales is None else scales[0 if name.endswith("_k") else 1]


def _new(W, D, dtype, scales=None):
    layer = SinkCacheLayer(NS, W)
    st = layer.init_pool(S, HKV, D, dtype, DEV)
    assert st.shape == (S, 4) and not st.any()
    if dtype == FP8:
        assert layer.kv_scale.shape == (2, HKV) and layer.kv_scale.dtype == torch.float32 and layer.kv_scale.is_cuda
        if scales is not None:
            layer.set_kv_scale(*scales)
            assert layer.kv_scale.tolist() == torch.tensor(scales, dtype=torch.float32).tolist()
    return layer


def _bytes(t):
    return t.view(torch.uint8) if t.dtype == FP8 else t.view(torch.int16)


def _snap(layer):
    """buffers (as integers: codes / 16-bit patterns) and state, cloned"""
    d = {name: _bytes(getattr(layer, name)).clone() for name in BUFS}
    d["state"] = layer._dev_state.clone()
    return d


def _clone(layer):
    c = SinkCacheLayer(layer.num_sink, layer.window_size)
    for name in BUFS:
        setattr(c, name, getattr(layer, name).clone())
    c._dev_state = layer._dev_state.clone()
    c.kv_scale = None if layer.kv_scale is None else layer.kv_scale.clone()
    c.is_initialized = c.prefilled = c._per_seq = c._pool = True
    return c


def _unmoved(layer, snap, what, slots=None):
    sel = slice(None) if slots is None else torch.tensor(sorted(slots), device=DEV)
    for name in BUFS:
        assert torch.equal(_bytes(getattr(layer, name))[sel], snap[name][sel]), (what, name)
    assert torch.equal(layer._dev_state[sel], snap["state"][sel]), (what, "state")


def _stored(p8, p16, s8, s16, scales, what):
    """the storage equality after one storing call on both pools; returns the number of rows the call wrote"""
    rows = 0
    for name in BUFS:
        new16 = getattr(p16, name)
        changed = (_bytes(new16) != s16[name]).any(dim=-1, keepdim=True)          # [S, H_kv, rows, 1]
        want = quant(new16.cpu(), _row(scales, name)).view(torch.uint8).to(DEV)
        exp = torch.where(changed, want, s8[name])
        got = _bytes(getattr(p8, name))
        bad = (got != exp).any(dim=-1).nonzero()
        assert torch.equal(got, exp), (what, name, "rows (slot, head, row)", bad[:4].tolist(), "of", len(bad))
        rows += int(changed.sum())
    assert torch.equal(p8._dev_state, p16._dev_state), (what, p8._dev_state.tolist(), p16._dev_state.tolist())
    return rows


def _fill_calls(dtype, D, W, seed, fresh=()):
    """the calls that bring a pool to the fills of test_gpu_ragged_tree._pool (per slot s % 4: a sink that is not full
    under an empty ring, a ring partly filled, filled exactly, full and wrapped to write_pos != 0; `fresh` slots stay as
    init_pool leaves them): a prefill_slots and a commit_packed_dyn of a 7-token chunk per slot.  Returns (calls, hist)
    with hist as _pool gives it: the 16-bit tokens every slot holds, on the CPU."""
    g = torch.Generator().manual_seed(seed)
    fills = [[(2, 0), (9, 0), (NS + W, 0), (NS + W + 4, 7)][s % 4] for s in range(S)]
    live = [s for s in range(S) if s not in fresh]
    pre = {s: (rand((1, HKV, fills[s][0], D), g, dtype), rand((1, HKV, fills[s][0], D), g, dtype)) for s in live}
    kp, vp = torch.cat([pre[s][0] for s in live], dim=2).to(DEV), torch.cat([pre[s][1] for s in live], dim=2).to(DEV)
    kc, vc = rand((1, HKV, 7 * len(live), D), g, dtype), rand((1, HKV, 7 * len(live), D), g, dtype)
    counts = [fills[s][1] for s in live]
    calls = [("prefill_slots", lambda p: p.prefill_slots(kp, vp, _cu([fills[s][0] for s in live]), live)),
             ("commit_packed_dyn", lambda p: p.commit_packed_dyn(kc.to(DEV), vc.to(DEV), _i32(_cu([7] * len(live))),
                                                                 _dev_slots(live), _i32(counts)))]
    hist = {}
    for j, s in enumerate(live):
        c = fills[s][1]
        hist[s] = dict(pre=pre[s], com=(kc[:, :, 7 * j:7 * j + c], vc[:, :, 7 * j:7 * j + c]))
    for s in fresh:
        z = torch.zeros(1, HKV, 0, D, dtype=dtype)
        hist[s] = dict(pre=(z, z), com=(z, z))
    return calls, hist


def _fp8_pool(dtype, D, W, seed, scales=SCALES, fresh=()):
    p8 = _new(W, D, FP8, scales)
    calls, hist = _fill_calls(dtype, D, W, seed, fresh)
    for _, f in calls:
        f(p8)
    return p8, hist


def _dequant_pool(p8, dtype, scales):
    """the 16-bit pool of the read equality: (codes.float() * scale).to(dtype) in every buffer, the same state"""
    pd = _new(p8.window_size, p8.window_k.shape[3], dtype)
    for name in BUFS:
        getattr(pd, name).copy_(dequant(getattr(p8, name).cpu(), _row(scales, name), dtype).to(DEV))
    pd._dev_state.copy_(p8._dev_state)
    return pd


def _zero_rows(o, lengths, slots):
    cu = _cu(lengths)
    live = torch.zeros(o.shape[2], dtype=torch.bool)
    for i, (n, s) in enumerate(zip(lengths, slots)):
        if s >= 0:
            live[cu[i]:cu[i] + n] = True
    assert not o[:, :, ~live.to(o.device)].any(), "padded rows and the rows of an inactive sequence must be zero"


# ------------------------------------------------------------------ 1. storage equality
@pytest.mark.parametrize("dtype,D,G,W,scales", GRID)
def test_every_stored_row_is_quant_of_the_row_a_16_bit_pool_gets(dtype, D, G, W, scales):
    p8, p16 = _new(W, D, FP8, scales), _new(W, D, dtype)
    calls, _ = _fill_calls(dtype, D, W, seed=101, fresh=(6, 7))
    q, k, v, sa = _pack(dtype, D, G, T_PAD, seed=102)
    cu = _cu(LENGTHS)
    # slots 7 and 6 are fresh: the sequences of 33 and 64 tokens are admitted by the step; the 7-token one is inactive and
    # the 16-token one is not committed
    slots, mask = [3, -1, 5, 2, 7, 6, 4], [1, 1, 1, 0, 1, 1, 1]
    # one token per kind of placement with |x| / scale > 448: a decode row (ring), token 2 of an admitted sequence (sink)
    # and its last token (ring)
    for t, sign in ((0, 1.0), (cu[4] + 2, -1.0), (cu[5] - 1, 1.0)):
        k[:, :, t], v[:, :, t] = sign * BIG, -sign * BIG
    par = _parents(LENGTHS, _mix_a(), T_PAD)
    step = lambda p: p.ragged_step_dyn(q.to(DEV), k.to(DEV), v.to(DEV), _i32(cu), _dev_slots(slots), s_aux=sa.to(DEV),
                                       commit=True, admit=True, parent=_i32(par), commit_seq=_i32(mask))
    counts = [1, 3, 2, 20, -3, 40, 70]
    g = torch.Generator().manual_seed(103)
    path = []
    for n in LENGTHS:
        p = torch.randint(0, max(n, 1), (n,), generator=g).tolist()
        if n >= 7:
            p[1], p[2] = n + 3, -2                   # entries outside [0, n): clamped on the device
        path += p
    path += [9] * (T_PAD - len(path))
    _, k2, v2, _ = _pack(dtype, D, 1, T_PAD, seed=104)
    commit = lambda p, pt: p.commit_packed_dyn(k2.to(DEV), v2.to(DEV), _i32(cu), _dev_slots(PERM_HOLE), _i32(counts), path=pt)
    calls += [("ragged_step_dyn(commit, admit, commit_seq)", step), ("commit_packed_dyn(path)", lambda p: commit(p, _i32(path))),
              ("commit_packed_dyn()", lambda p: commit(p, None))]
    for what, f in calls:
        s8, s16 = _snap(p8), _snap(p16)
        f(p8)
        assert _path().endswith("_kvfp8"), (what, _path())
        f(p16)
        assert not _path().endswith("_kvfp8"), (what, _path())
        rows = _stored(p8, p16, s8, s16, scales, (what, dtype, D, W))
        print(what, "rows written", rows)
        assert rows > 0, what
        if what.startswith("ragged_step_dyn"):
            # the saturated tokens: every element of their rows is +-448 (0x7e / 0xfe), in the ring and in the sinks
            n_big = 0
            for name in BUFS:
                x16, c8 = getattr(p16, name), _bytes(getattr(p8, name))
                big = x16.abs() == BIG
                assert bool(((c8[big] & 0x7f) == 0x7e).all()) and bool((((c8[big] >> 7) == 1) == (x16[big] < 0)).all()), name
                n_big += int(big.all(dim=-1).sum())
            assert n_big == 2 * HKV * 3, n_big                  # K and V rows of three tokens, both heads
            assert p8._dev_state[7].tolist() == [NS, min(33 - NS, W), (33 - NS) % W if 33 - NS < W else 0, 33]


def test_activations_must_be_16_bit_and_of_one_dtype():
    p8 = _new(16, 64, FP8)
    q, k, v, _ = _pack(torch.float32, 64, 8, 8, seed=1)
    with pytest.raises(TypeError, match="bfloat16 or float16 tensors of one dtype"):
        p8.ragged_step_dyn(q.to(DEV), k.to(DEV), v.to(DEV), [0, 8], [0])
    with pytest.raises(TypeError, match="bfloat16 or float16 tensors of one dtype"):
        p8.prefill_slots(k.to(DEV).bfloat16(), v.to(DEV).half(), [0, 8], [0])
    with pytest.raises(TypeError, match="bfloat16 or float16 tensors of one dtype"):
        p8.commit_packed_dyn(k.to(DEV), v.to(DEV), [0, 8], [0], [1])
    with pytest.raises(TypeError, match="packed calls"):
        p8.extend_step_dyn(q.to(DEV).bfloat16(), k.to(DEV).bfloat16(), v.to(DEV).bfloat16(), slots=[0])
    assert not p8._dev_state.any()


# ------------------------------------------------------------------ 2. read equality
@pytest.mark.parametrize("dtype,D,G,W,scales", GRID)
def test_o_is_bitwise_o_over_a_16_bit_pool_of_the_dequantised_codes(dtype, D, G, W, scales):
    p8, _ = _fp8_pool(dtype, D, W, seed=111, scales=scales, fresh=(6, 7))
    q, k, v, sa = _pack(dtype, D, G, T_PAD, seed=112)
    cu = _cu(LENGTHS)
    par = _parents(LENGTHS, _mix_a(), T_PAD)
    fresh = [3, -1, 5, 2, 7, 6, 4]                 # the sequences of 33 and 64 tokens on the fresh slots
    # (slots, parent, admit, commit): the plain mask; trees; admission; each with commit off, then on
    for slots, parent, admit in ((PERM_HOLE, None, False), (PERM_HOLE, par, False), (fresh, None, True), (fresh, par, True)):
        for commit in (False, True):
            a, b = _clone(p8), _dequant_pool(p8, dtype, scales)
            before = _snap(a)
            o8 = _run(a, q, k, v, cu, slots, parent, sa=sa, commit=commit, admit=admit)
            path = _path()
            assert path.startswith("decode_tree_mfma_" if parent is not None else "decode_multi_mfma_") and \
                path.endswith("_kvfp8") and ("_admit" in path) == admit and ("_commit" in path) == commit, path
            od = _run(b, q, k, v, cu, slots, parent, sa=sa, commit=commit, admit=admit)
            assert _path() == path[:-len("_kvfp8")], (_path(), path)
            diff = (o8 != od).any(dim=(0, 1, 3)).nonzero().flatten().tolist()
            assert torch.equal(o8, od), ("parent", parent is not None, "admit", admit, "commit", commit, "packed rows", diff[:8])
            _zero_rows(o8, LENGTHS, slots)
            assert o8[:, :, :cu[-1]].any()
            assert torch.equal(a._dev_state, b._dev_state)
            if not commit:
                _unmoved(a, before, "commit off: the pool must not move")
            else:
                assert not torch.equal(a._dev_state, before["state"])


# ------------------------------------------------------------------ 3. the fp64 oracle over the dequantised history
@pytest.mark.parametrize("dtype,D,G,W", ORACLE)
def test_the_oracle_over_the_dequantised_history(dtype, D, G, W):
    p8, hist = _fp8_pool(dtype, D, W, seed=121)
    dq = lambda kv: (dequant(quant(kv[0], K_SCALE), K_SCALE, dtype), dequant(quant(kv[1], V_SCALE), V_SCALE, dtype))
    hist8 = {s: dict(pre=dq(h["pre"]), com=dq(h["com"])) for s, h in hist.items()}
    q, k, v, sa = _pack(dtype, D, G, T_PAD, seed=122)
    trees = _mix_a()
    o = _run(p8, q, k, v, _cu(LENGTHS), PERM_HOLE, _parents(LENGTHS, trees, T_PAD), sa=sa)
    assert _path().startswith("decode_tree_mfma_") and _path().endswith("_ragged_kvfp8"), _path()
    ref = _oracle(q, k, v, sa, hist8, W, LENGTHS, PERM_HOLE, trees)
    assert len(ref) == sum(1 for n, s in zip(LENGTHS, PERM_HOLE) if n and s >= 0)
    _check_rows(o, ref, LENGTHS, DECODE_TOL[dtype], ("fp8 pool", dtype, D, G, W))


# ------------------------------------------------------------------ 4. fork
def _live_equal(a, sa_, b, sb, what):
    """slot sa_ of pool a against slot sb of pool b: the state row and the live rows, as bytes"""
    st = a._dev_state[sa_].tolist()
    assert st == b._dev_state[sb].tolist() and st[3] > 0, (what, st, b._dev_state[sb].tolist())
    for name, n in (("sink_k", st[0]), ("sink_v", st[0]), ("window_k", st[1]), ("window_v", st[1])):
        assert torch.equal(_bytes(getattr(a, name))[sa_, :, :n], _bytes(getattr(b, name))[sb, :, :n]), (what, name)


@pytest.mark.parametrize("dtype,D,G,W", [(torch.bfloat16, 64, 8, 16), (torch.float16, 80, 1, 48)])
def test_fork_slots_copies_codes_within_a_pool_and_between_two(dtype, D, G, W):
    p8, _ = _fp8_pool(dtype, D, W, seed=131, fresh=(6, 7))
    other = _new(W, D, FP8, SCALES)                       # equal scales on pools that exchange slots
    ref = _clone(p8)
    before = _snap(p8)
    p8.fork_slots([3, 1], [6, 7])                          # a wrapped ring and a partly filled one
    assert _path() == "ring_copy_slots", _path()
    _live_equal(p8, 6, ref, 3, "fork 3 -> 6"), _live_equal(p8, 7, ref, 1, "fork 1 -> 7")
    _unmoved(p8, before, "a fork moves its destinations only", [s for s in range(S) if s not in (6, 7)])
    n1 = ref._dev_state[1, 1].item()                       # rows the source does not reach keep what the destination held
    assert torch.equal(_bytes(p8.window_k)[7, :, n1:], before["window_k"][7, :, n1:])
    other.fork_slots([3, 7], [0, 5], source=p8)            # into a second FP8 pool ...
    _live_equal(other, 0, ref, 3, "park 3"), _live_equal(other, 5, ref, 1, "park 7")
    assert not other._dev_state[[1, 2, 3, 4, 6, 7]].any()
    mid = _snap(p8)
    p8.fork_slots([0], [2], source=other)                  # ... and back out of it
    _live_equal(p8, 2, ref, 3, "back 0 -> 2")
    _unmoved(p8, mid, "the way back moves slot 2 only", [s for s in range(S) if s != 2])
    with pytest.raises(TypeError, match="differ in dtype"):
        p8.fork_slots([0], [1], source=_new(W, D, dtype))
    # a step on the forks is bitwise the step on the sources
    lengths = [1, 7]
    q, k, v, sa = _pack(dtype, D, G, 8, seed=132)
    o_src = _run(ref, q, k, v, _cu(lengths), [3, 1], sa=sa).clone()
    for pool, slots in ((p8, [6, 7]), (p8, [2, 7]), (other, [0, 5])):
        o = _run(pool, q, k, v, _cu(lengths), slots, sa=sa)
        assert _path().endswith("_kvfp8") and torch.equal(o, o_src), slots


# ------------------------------------------------------------------ 5. determinism, one captured graph
def test_two_runs_give_the_same_bits():
    p8, _ = _fp8_pool(torch.float16, 80, 48, seed=141)
    q, k, v, sa = _pack(torch.float16, 80, 1, T_PAD, seed=142)
    par = _parents(LENGTHS, _mix_a(), T_PAD)
    o1 = _run(p8, q, k, v, _cu(LENGTHS), PERM_HOLE, par, sa=sa).clone()
    o2 = _run(p8, q, k, v, _cu(LENGTHS), PERM_HOLE, par, sa=sa)
    assert torch.equal(o1, o2)
    a, b = _clone(p8), _clone(p8)
    for p in (a, b):
        _run(p, q, k, v, _cu(LENGTHS), PERM_HOLE, par, sa=sa, commit=True)
    _unmoved(a, _snap(b), "two committing runs leave the same bytes")


def test_one_captured_graph_replays_at_new_lengths_slots_and_scales():
    dtype, D, G, W, T, n_seq = torch.bfloat16, 64, 8, 16, 112, 6
    layer, _ = _fp8_pool(dtype, D, W, seed=151, fresh=(6, 7))
    sq = torch.zeros(1, HKV * G, T, D, dtype=dtype, device=DEV)
    sk, sv = (torch.zeros(1, HKV, T, D, dtype=dtype, device=DEV) for _ in range(2))
    scu, ssl = torch.zeros(n_seq + 1, dtype=torch.int32, device=DEV), torch.full((n_seq,), -1, dtype=torch.int32, device=DEV)
    srel = torch.full((2,), -1, dtype=torch.int32, device=DEV)
    spar, scs = torch.full((T,), -1, dtype=torch.int32, device=DEV), torch.zeros(n_seq, dtype=torch.int32, device=DEV)
    sdr, stg = (torch.zeros(T, dtype=torch.int64, device=DEV) for _ in range(2))
    so = torch.zeros_like(sq)
    sad = rand((HKV * G,), torch.Generator().manual_seed(150), torch.float32, 0.8).to(DEV)

    def step(p, out):
        """one iteration of the serving loop; returns (positions, o)"""
        p.release_slots(srel)
        pos = p.packed_positions(scu, ssl, T)
        o = p.ragged_step_dyn(sq, sk, sv, scu, ssl, s_aux=sad, out=out, commit=True, admit=True, parent=spar, commit_seq=scs)
        path, count = spec_tree.greedy_accept_packed(spar, sdr, stg, scu, n_seq)
        p.commit_packed_dyn(sk, sv, scu, ssl, count * (1 - scs), path=path)
        return pos, o

    start = _snap(layer)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):         # warm-up outside the capture (allocates the workspace); all rows inactive
        step(layer, so)
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        spos, _ = step(layer, so)
    _unmoved(layer, start, "warm-up and capture with every sequence inactive")
    # (lengths, slots, trees, commit_seq, released, new scales): all decode; trees + a chunk + an admission; after an
    # in-place set_kv_scale, partly inactive, with a slot released and readmitted in the same iteration
    steps = [([1, 1, 1, 1, 1, 1], [0, 1, 2, 3, 4, 5], [chain(1)] * 6, [1] * 6, [-1, -1], None),
             ([16, 70, 7, 9, 1, 5], [1, 2, 3, 6, 4, 0], [rand_tree(16, 30, False), star(70), binary(7), chain(9), chain(1),
                                                         comb(5)], [0, 1, 0, 1, 1, 0], [-1, -1], None),
             ([33, 4, 0, 12, 1, 40], [5, -1, 2, 7, -1, 3], [comb(33), star(4), [], chain(12), chain(1), chain(40)],
              [0, 0, 1, 1, 1, 1], [3, -1], ([1.5, 0.5], [0.25, 3.0]))]
    for r, (lengths, slots, trees, mask, rel, scales) in enumerate(steps):
        q, k, v, _ = _pack(dtype, D, G, T, seed=152 + r)
        g = torch.Generator().manual_seed(160 + r)
        draft, target = torch.randint(0, 2, (T,), generator=g), torch.randint(0, 2, (T,), generator=g)
        sq.copy_(q), sk.copy_(k), sv.copy_(v), sdr.copy_(draft), stg.copy_(target)
        scu.copy_(torch.tensor(_cu(lengths), dtype=torch.int32)), ssl.copy_(torch.tensor(slots, dtype=torch.int32))
        spar.copy_(torch.tensor(_parents(lengths, trees, T), dtype=torch.int32))
        scs.copy_(torch.tensor(mask, dtype=torch.int32)), srel.copy_(torch.tensor(rel, dtype=torch.int32))
        if scales is not None:
            ptr = layer.kv_scale.data_ptr()
            layer.set_kv_scale(torch.tensor(scales[0], device=DEV), torch.tensor(scales[1], device=DEV))
            assert layer.kv_scale.data_ptr() == ptr                 # in place: the graph keeps the pointer
        twin = _clone(layer)
        before = _snap(layer)
        graph.replay()
        pos, o = step(twin, None)                                   # the eager run of the same inputs
        assert _path() == "ring_commit_path_ragged_slots_kvfp8", _path()
        assert torch.equal(spos, pos) and torch.equal(so, o), ("replay", r)
        _unmoved(layer, _snap(twin), ("replay", r, "the pool is the eager run's"))
        assert not torch.equal(layer._dev_state, before["state"]), ("replay", r, "the step moved the pool")
        _zero_rows(so, lengths, slots)
        assert so[:, :, :_cu(lengths)[-1]].any()
    assert layer._dev_state[3, 3].item() == 40                       # released, then admitted with 40 tokens
