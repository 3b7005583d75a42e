"""Packed ragged step over the slot pool (sfa_decode_ring_ragged_slots / SinkCacheLayer.ragged_step_dyn): sequences with
their own token counts - decode rows, draft rows, prompt chunks, an empty one - in one call.

Every sequence must come out as sfa_decode_ring_multi of its own chunk at its slot's state: checked against the f64
oracle over tests/test_decode_multi_host.py::history_keys, against extend_attention_dyn(slots=) where the lengths agree,
bitwise against itself under a reordering of the pack, and bitwise against commit_dyn(slots=) for what a commit leaves.
Shapes: H_kv = 2, G in {1, 8}, num_sink = 4, Wc in {16, 48}, S = 7 slots, T <= 160 packed rows."""
import pytest
import torch

import probe_inputs as P
from test_gpu_decode_multi import TOL, _oracle_rows
from test_ragged_step_host import PROBE_TYPES, probe_pack
from test_gpu_slots import BUFS, SENTINEL, TYPES, _clone, _dev_slots, _new_pool, _path, _prefill
from util import maxdiff, rand

pytestmark = pytest.mark.gpu
DEV = "cuda"
HKV, NS, S = 2, 4, 7
LENGTHS = [1, 3, 0, 8, 5, 33, 70]      # 1 token; G * n = 24 / 40 / 64 around the 32-row block; empty; > 1 tile; n > Wc
T_PAD = 128                            # 120 rows of sequences and a padded tail of 8
PERM = [3, 0, 5, 2, 6, 1, 4]           # sequence i -> slot PERM[i]
PERM_HOLE = [3, -1, 5, 2, 6, 1, 4]     # ... with the 3-token sequence inactive


def _cu(lengths):
    cu = [0]
    for n in lengths:
        cu.append(cu[-1] + n)
    return cu


def _fills(W):
    """per slot s (s % 4): (prefill length, tokens then committed) - a sink that is not full under an empty ring, a ring
    partly filled, a ring filled exactly, a full ring wrapped to write_pos != 0 (the mix of test_gpu_ragged_cache.py)"""
    return [(2, 0), (9, 0), (NS + W, 0), (NS + W + 4, 7)]


def _pool(dtype, D, W, seed, sentinel=None):
    """A pool of S slots at mixed fills; returns (layer, hist) with hist[s] = (k, v, sink_len) of slot s's whole history
    on the CPU.  A slot that is never prefilled keeps its sentinel buffers."""
    g = torch.Generator().manual_seed(seed)
    layer = _new_pool(NS, W, S, HKV, D, dtype, sentinel)
    fills = [_fills(W)[s % 4] for s in range(S)]
    hist = _prefill(layer, [f[0] for f in fills], list(range(S)), HKV, D, dtype, g)
    kc, vc = rand((S, HKV, 7, D), g, dtype), rand((S, HKV, 7, D), g, dtype)
    layer.commit_dyn(kc.to(DEV), vc.to(DEV), torch.tensor([f[1] for f in fills], device=DEV), slots=list(range(S)))
    out = []
    for s, (k, v) in enumerate(hist):
        c = fills[s][1]
        out.append((torch.cat([k, kc[s:s + 1, :, :c]], dim=2), torch.cat([v, vc[s:s + 1, :, :c]], dim=2),
                    min(fills[s][0], NS)))
    return layer, out


def _pack(dtype, D, G, lengths, T, seed):
    g = torch.Generator().manual_seed(seed)
    q = rand((1, HKV * G, T, D), g, dtype)
    k, v = rand((1, HKV, T, D), g, dtype), rand((1, HKV, T, D), g, dtype)
    sa = rand((HKV * G,), g, torch.float32, 0.8)
    return q, k, v, sa


def _oracle(q, k, v, sa, hist, W, lengths, slots):
    """f64 rows of every active sequence: {i: [1, Hq, n_i, D]}"""
    cu, out = _cu(lengths), {}
    for i, (n, s) in enumerate(zip(lengths, slots)):
        if n == 0 or s < 0:
            continue
        hk, hv, sl = hist[s]
        L = hk.shape[2]
        sel = slice(cu[i], cu[i] + n)
        qf = torch.cat([torch.zeros(1, q.shape[1], L, q.shape[3], dtype=q.dtype), q[:, :, sel]], dim=2)
        out[i] = _oracle_rows(qf, torch.cat([hk, k[:, :, sel]], dim=2), torch.cat([hv, v[:, :, sel]], dim=2), sa, L, sl, W,
                              n, slice(0, 1))
    return out


def _run(layer, q, k, v, cu, slots, sa=None, commit=False, out=None):
    o = layer.ragged_step_dyn(q.to(DEV), k.to(DEV), v.to(DEV), torch.tensor(cu, dtype=torch.int32, device=DEV),
                              _dev_slots(slots), s_aux=None if sa is None else sa.to(DEV), out=out, commit=commit)
    assert "_ragged" in _path(), _path()
    return o


def _check_rows(o, ref, lengths, slots, tol, what):
    """active rows within tol of the oracle, every other row exactly zero"""
    cu = _cu(lengths)
    live = torch.zeros(o.shape[2], dtype=torch.bool)
    for i, r in ref.items():
        got = o[:, :, cu[i]:cu[i] + lengths[i]].double().cpu()
        err = (got - r).abs().amax(dim=(0, 1, 3))
        assert err.max().item() <= tol, (what, "sequence", i, "slot", slots[i], "row errors", err.tolist())
        live[cu[i]:cu[i] + lengths[i]] = True
    assert not o[:, :, ~live.to(o.device)].any(), (what, "inactive / empty / padded rows must be zero")


# ------------------------------------------------------------------ 1. parity against the oracle
@pytest.mark.parametrize("W", [16, 48])
@pytest.mark.parametrize("G", [1, 8])
@pytest.mark.parametrize("dtype,D", TYPES)
def test_parity_with_the_oracle_over_mixed_fills_and_lengths(dtype, D, G, W):
    layer, hist = _pool(dtype, D, W, seed=11)
    q, k, v, sa = _pack(dtype, D, G, LENGTHS, T_PAD, seed=12)
    cu = _cu(LENGTHS)
    for slots, aux in ((PERM_HOLE, sa), (PERM, None)):
        before = _clone(layer)
        o = _run(layer, q, k, v, cu, slots, aux)
        mfma = dtype != torch.float32 and D in (64, 80, 96, 128)
        assert ("_mfma_" in _path()) == mfma and _path().endswith("_ragged"), _path()
        ref = _oracle(q, k, v, aux, hist, W, LENGTHS, slots)
        assert len(ref) == sum(1 for n, s in zip(LENGTHS, slots) if n and s >= 0)
        _check_rows(o, ref, LENGTHS, slots, TOL[dtype], (dtype, D, G, W, slots))
        for name in BUFS:       # commit off: nothing moves
            assert torch.equal(getattr(layer, name), getattr(before, name)), name
        assert torch.equal(layer._dev_state, before._dev_state)


# ------------------------------------------------------------------ 2. zeros and untouched pool rows
@pytest.mark.parametrize("dtype,D,G", [(torch.bfloat16, 64, 8), (torch.float32, 48, 1)])
def test_inactive_rows_are_zero_and_unnamed_slots_keep_their_bits(dtype, D, G):
    W = 16
    layer, _ = _pool(dtype, D, W, seed=21, sentinel=SENTINEL)
    # slots 0, 1 and 5 are named by no sequence, slot 2 only by the empty one; the 4-token sequence is inactive
    lengths, slots = [5, 0, 33, 4, 1], [3, 2, 6, -1, 4]
    q, k, v, sa = _pack(dtype, D, G, lengths, 64, seed=22)
    before = _clone(layer)
    o = torch.full((1, HKV * G, 64, D), 3.0, dtype=dtype, device=DEV)
    _run(layer, q, k, v, _cu(lengths), slots, sa, commit=True, out=o)
    live = torch.zeros(64, dtype=torch.bool)
    for i, (n, s) in enumerate(zip(lengths, slots)):
        if s >= 0:
            live[_cu(lengths)[i]:_cu(lengths)[i] + n] = True
    assert not o[:, :, ~live.to(DEV)].any() and o[:, :, live.to(DEV)].abs().sum() > 0
    for s in (0, 1, 2, 5):
        for name in BUFS:
            assert torch.equal(getattr(layer, name)[s], getattr(before, name)[s]), ("untouched slot", s, name)
        assert torch.equal(layer._dev_state[s], before._dev_state[s]), ("untouched state", s)
    for i, s in ((0, 3), (2, 6), (4, 4)):
        assert layer._dev_state[s, 3].item() == before._dev_state[s, 3].item() + lengths[i]
        assert torch.equal(layer.sink_k[s], before.sink_k[s]) and layer._dev_state[s, 0] == before._dev_state[s, 0]


# ------------------------------------------------------------------ 3. order independence, bitwise
@pytest.mark.parametrize("dtype,D,G,W", [(torch.bfloat16, 64, 8, 16), (torch.float16, 128, 1, 48),
                                         (torch.bfloat16, 80, 8, 48), (torch.float32, 64, 8, 16)])
def test_a_sequence_gives_the_same_bits_wherever_it_lies_in_the_pack(dtype, D, G, W):
    layer, _ = _pool(dtype, D, W, seed=31)
    q, k, v, sa = _pack(dtype, D, G, LENGTHS, T_PAD, seed=32)
    cu = _cu(LENGTHS)
    o1 = _run(layer, q, k, v, cu, PERM, sa)
    order = [5, 2, 0, 6, 3, 1, 4]
    l2 = [LENGTHS[i] for i in order]
    cu2 = _cu(l2)
    gather = torch.cat([torch.arange(cu[i], cu[i] + LENGTHS[i]) for i in order] + [torch.arange(cu[-1], T_PAD)])
    o2 = _run(layer, q[:, :, gather], k[:, :, gather], v[:, :, gather], cu2, [PERM[i] for i in order], sa)
    for j, i in enumerate(order):
        a, b = o1[:, :, cu[i]:cu[i] + LENGTHS[i]], o2[:, :, cu2[j]:cu2[j] + l2[j]]
        assert torch.equal(a, b), ("sequence", i, "moved to", j, maxdiff(a, b))


# ------------------------------------------------------------------ 4. commit, bitwise
@pytest.mark.parametrize("dtype,D,G,W", [(torch.bfloat16, 64, 8, 16), (torch.float16, 80, 1, 48),
                                         (torch.float32, 128, 8, 16), (torch.bfloat16, 48, 1, 48)])
def test_commit_leaves_what_commit_dyn_leaves_and_the_same_output(dtype, D, G, W):
    layer, _ = _pool(dtype, D, W, seed=41, sentinel=SENTINEL)
    q, k, v, sa = _pack(dtype, D, G, LENGTHS, T_PAD, seed=42)
    cu = _cu(LENGTHS)
    twin, dry = _clone(layer), _clone(layer)
    twin._pool = dry._pool = True
    o = _run(layer, q, k, v, cu, PERM_HOLE, sa, commit=True)
    assert _path().endswith("_ragged_commit"), _path()
    assert torch.equal(o, _run(dry, q, k, v, cu, PERM_HOLE, sa, commit=False))
    for n in sorted(set(LENGTHS) - {0}):      # the same tokens through commit_dyn(slots=), one group per length
        idx = [i for i in range(len(LENGTHS)) if LENGTHS[i] == n and PERM_HOLE[i] >= 0]
        if not idx:
            continue
        kc = torch.cat([k[:, :, cu[i]:cu[i] + n] for i in idx]).to(DEV)
        vc = torch.cat([v[:, :, cu[i]:cu[i] + n] for i in idx]).to(DEV)
        twin.commit_dyn(kc, vc, torch.full((len(idx),), n, device=DEV), slots=[PERM_HOLE[i] for i in idx])
    for name in BUFS:
        assert torch.equal(getattr(layer, name), getattr(twin, name)), name
    assert torch.equal(layer._dev_state, twin._dev_state), (layer._dev_state, twin._dev_state)


# ------------------------------------------------------------------ 5. agreement with the existing call
@pytest.mark.parametrize("n", [1, 4, 8])
@pytest.mark.parametrize("dtype,D,G", [(torch.bfloat16, 64, 8), (torch.float16, 128, 1), (torch.float32, 80, 8)])
def test_equal_lengths_agree_with_extend_attention_dyn(dtype, D, G, n):
    W = 16
    layer, _ = _pool(dtype, D, W, seed=51)
    slots = [4, 2, 6, 0, 3]
    B = len(slots)
    q, k, v, sa = _pack(dtype, D, G, [n] * B, n * B, seed=52)
    o = _run(layer, q, k, v, _cu([n] * B), slots, sa)
    unpack = lambda t: t.reshape(t.shape[1], B, n, D).transpose(0, 1).contiguous().to(DEV)
    ref = layer.extend_attention_dyn(unpack(q), unpack(k), unpack(v), s_aux=sa.to(DEV), slots=slots)
    got = o.reshape(HKV * G, B, n, D).transpose(0, 1)
    assert maxdiff(got, ref) <= TOL[dtype], maxdiff(got, ref)


# ------------------------------------------------------------------ 6. mask-edge probes
# inputs and reference: tests/test_ragged_step_host.py::probe_pack, whose CPU proof shows that a one-key mask error at
# the diagonal, the oldest window key, the key behind it or the pack edge cannot stay within TOL
@pytest.mark.parametrize("W", [16, 48])
@pytest.mark.parametrize("dt,D,G", PROBE_TYPES)
def test_mask_edge_probes(dt, D, G, W):
    dtype = P._DT[dt]
    q, k, v, sa, hist, lengths, ref, _ = probe_pack(dt, D, G, W)
    layer = _new_pool(NS, W, S, HKV, D, dtype)
    slots = [5, 1, 3, 0, 6]
    kp, vp = torch.cat([h[0] for h in hist], dim=2), torch.cat([h[1] for h in hist], dim=2)
    layer.prefill_slots(kp.to(DEV), vp.to(DEV), _cu([h[0].shape[2] for h in hist]), slots)
    o = _run(layer, q, k, v, _cu(lengths), slots, sa)
    _check_rows(o, ref, lengths, slots, TOL[dtype], ("probe", dt, D, G, W))


# ------------------------------------------------------------------ 7. determinism
def test_two_runs_give_the_same_bits():
    layer, _ = _pool(torch.bfloat16, 64, 48, seed=71)
    q, k, v, sa = _pack(torch.bfloat16, 64, 8, LENGTHS, T_PAD, seed=72)
    o1 = _run(layer, q, k, v, _cu(LENGTHS), PERM, sa).clone()
    o2 = _run(layer, q, k, v, _cu(LENGTHS), PERM, sa)
    assert torch.equal(o1, o2)


# ------------------------------------------------------------------ 8. capture
def test_a_captured_step_replays_at_any_mix_of_lengths():
    dtype, D, G, W, T = torch.bfloat16, 64, 8, 16, 96
    layer, _ = _pool(dtype, D, W, seed=81)
    n_seq = 5
    sq = torch.zeros(1, HKV * G, T, D, dtype=dtype, device=DEV)
    sk, sv = (torch.zeros(1, HKV, T, D, dtype=dtype, device=DEV) for _ in range(2))
    scu = torch.zeros(n_seq + 1, dtype=torch.int32, device=DEV)
    ssl = torch.full((n_seq,), -1, dtype=torch.int32, device=DEV)
    so = torch.zeros_like(sq)
    sa = rand((HKV * G,), torch.Generator().manual_seed(80), torch.float32, 0.8).to(DEV)
    start = _clone(layer)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):         # warm-up outside the capture (allocates the workspace); all rows inactive
        layer.ragged_step_dyn(sq, sk, sv, scu, ssl, s_aux=sa, out=so, commit=True)
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        layer.ragged_step_dyn(sq, sk, sv, scu, ssl, s_aux=sa, out=so, commit=True)
    for name in BUFS:
        assert torch.equal(getattr(layer, name), getattr(start, name)), name
    assert torch.equal(layer._dev_state, start._dev_state)
    steps = [([1, 40, 3, 8, 1], [0, 5, 2, 6, 3]), ([70, 1, 0, 1, 8], [4, -1, 1, 2, 0]), ([1, 1, 1, 1, 92], [6, 5, 4, 3, 2])]
    for r, (lengths, slots) in enumerate(steps):
        q, k, v, _ = _pack(dtype, D, G, lengths, T, seed=82 + r)
        eager = _clone(layer)
        eager._pool = True
        sq.copy_(q), sk.copy_(k), sv.copy_(v)
        scu.copy_(torch.tensor(_cu(lengths), dtype=torch.int32)), ssl.copy_(torch.tensor(slots, dtype=torch.int32))
        graph.replay()
        oe = _run(eager, q, k, v, _cu(lengths), slots, sa.cpu(), commit=True)
        assert torch.equal(so, oe), ("replay", r, maxdiff(so, oe))
        for name in BUFS:
            assert torch.equal(getattr(layer, name), getattr(eager, name)), ("replay", r, name)
        assert torch.equal(layer._dev_state, eager._dev_state), ("replay", r)
