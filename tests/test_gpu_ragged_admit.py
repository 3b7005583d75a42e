"""Admission in the packed ragged step (SFA_FLAG_RAGGED_ADMIT, SinkCacheLayer.ragged_step_dyn(admit=True)): a sequence
whose slot is fresh (state row seen == 0) is taken from position 0 in the same call that continues the others.

An admitting sequence must come out as a prefill of its own tokens (oracle.sink_oracle.sink_attention_dense of the
sequence alone) and leave what prefill_slots leaves, bitwise; every continuing sequence of the pack stays what
tests/test_gpu_ragged_step.py checks.  Shapes: H_kv = 2, G in {1, 8}, num_sink in {4, 40} (40: the sinks span one full
32-key tile and part of the next), Wc in {16, 48}, S = 7 slots, T <= 192 packed rows, admitting lengths
{0, 1, 3, 4, 5, 33, 70, 100} over two packs, each with continuing sequences at two of the four fills (_fills_ns: those of
test_gpu_ragged_step._fills(W), restated over the test's own num_sink), an inactive sequence and a padded tail."""
import pytest
import torch

import probe_inputs as P
from oracle import sink_oracle as O
from test_gpu_decode_multi import TOL, _oracle_rows
from test_gpu_ragged_step import LENGTHS, PERM_HOLE, _check_rows, _cu, _fills, _oracle, _pack
from test_gpu_slots import BUFS, SENTINEL, _clone, _dev_slots, _new_pool, _path, _prefill
from test_ragged_admit_host import PROBE_LENGTHS, PROBE_TYPES, admit_probe
from util import maxdiff, rand

pytestmark = pytest.mark.gpu
DEV = "cuda"
HKV, S = 2, 7
# (length, slot, admitting) per sequence; a continuing sequence on slot s starts at fill _fills_ns(ns, W)[s % 4]
PACKS = {
    "a": (128, [(100, 4, True), (5, 0, False), (4, 6, True), (0, 2, True), (3, -1, False), (8, 1, False), (1, 5, True)]),
    "b": (160, [(1, 2, False), (70, 0, True), (33, 5, True), (2, -1, False), (33, 3, False), (5, 6, True), (3, 1, True)]),
}
TYPES = [(torch.bfloat16, 64), (torch.float16, 64), (torch.bfloat16, 128), (torch.float16, 128), (torch.float16, 96),
         (torch.float32, 64), (torch.bfloat16, 48)]
SMALL = [(torch.bfloat16, 64, 8, 16, 40), (torch.float16, 128, 1, 48, 4), (torch.bfloat16, 96, 8, 48, 40),
         (torch.float32, 64, 8, 16, 4), (torch.bfloat16, 48, 1, 48, 40)]


def _fills_ns(ns, W):
    """(prefill length, tokens then committed): a sink that is not full under an empty ring, a ring partly filled, a ring
    filled exactly, a full ring wrapped to write_pos != 0 - at this num_sink (at 4: test_gpu_ragged_step._fills(W))"""
    return [(2, 0), (ns + 5, 0), (ns + W, 0), (ns + W + 4, 7)]


assert all(_fills_ns(4, W) == _fills(W) for W in (16, 48))


def _mixed_pool(dtype, D, W, ns, seqs, seed, sentinel=None):
    """A pool whose continuing slots are prefilled (and advanced) as test_gpu_ragged_step._pool does and whose other slots
    are fresh; returns (layer, hist) with hist[slot] = (k, v, sink_len) of the slot's history on the CPU."""
    g = torch.Generator().manual_seed(seed)
    layer = _new_pool(ns, W, S, HKV, D, dtype, sentinel)
    cont = [s for _, s, adm in seqs if not adm and s >= 0]
    fills = [_fills_ns(ns, W)[s % 4] for s in cont]
    hist = _prefill(layer, [f[0] for f in fills], cont, HKV, D, dtype, g)
    kc, vc = rand((len(cont), HKV, 7, D), g, dtype), rand((len(cont), HKV, 7, D), g, dtype)
    layer.commit_dyn(kc.to(DEV), vc.to(DEV), torch.tensor([f[1] for f in fills], device=DEV), slots=cont)
    out = {}
    for j, s in enumerate(cont):
        c = fills[j][1]
        out[s] = (torch.cat([hist[j][0], kc[j:j + 1, :, :c]], dim=2), torch.cat([hist[j][1], vc[j:j + 1, :, :c]], dim=2),
                  min(fills[j][0], ns))
    return layer, out


def _run(layer, q, k, v, cu, slots, sa=None, commit=False, admit=True, out=None):
    o = layer.ragged_step_dyn(q.to(DEV), k.to(DEV), v.to(DEV), torch.tensor(cu, dtype=torch.int32, device=DEV),
                              _dev_slots(slots), s_aux=None if sa is None else sa.to(DEV), out=out, commit=commit,
                              admit=admit)
    want = "_ragged" + ("_admit" if admit else "") + ("_commit" if commit else "")
    assert _path().endswith(want), _path()
    return o


def _reference(q, k, v, sa, hist, W, ns, seqs):
    """f64 rows {i: [1, Hq, n_i, D]}: an admitting sequence alone through the dense oracle, a continuing one through the
    chunk oracle of tests/test_gpu_ragged_step.py"""
    lengths, slots = [n for n, _, _ in seqs], [s for _, s, _ in seqs]
    cu = _cu(lengths)
    hist_list = {s: h for s, h in hist.items()}
    ref = _oracle(q, k, v, sa, hist_list, W, lengths, [s if not adm else -1 for _, s, adm in seqs])
    for i, (n, s, adm) in enumerate(seqs):
        if adm and n and s >= 0:
            sel = slice(cu[i], cu[i] + n)
            ref[i], _ = O.sink_attention_dense(q[:, :, sel], k[:, :, sel], v[:, :, sel], ns, W, sa)
    return ref


def _twin_commit(twin, k, v, seqs):
    """what the committed step must leave: prefill_slots of the admitting sequences, commit_dyn(slots=) of the others"""
    lengths = [n for n, _, _ in seqs]
    cu = _cu(lengths)
    adm = [i for i, (n, s, a) in enumerate(seqs) if a and n and s >= 0]
    if adm:
        kp = torch.cat([k[:, :, cu[i]:cu[i] + lengths[i]] for i in adm], dim=2).to(DEV)
        vp = torch.cat([v[:, :, cu[i]:cu[i] + lengths[i]] for i in adm], dim=2).to(DEV)
        twin.prefill_slots(kp, vp, _cu([lengths[i] for i in adm]), [seqs[i][1] for i in adm])
    for i, (n, s, a) in enumerate(seqs):
        if not a and n and s >= 0:
            twin.commit_dyn(k[:, :, cu[i]:cu[i] + n].to(DEV), v[:, :, cu[i]:cu[i] + n].to(DEV),
                            torch.full((1,), n, device=DEV), slots=[s])


def _same_pool(a, b, what):
    for name in BUFS:
        assert torch.equal(getattr(a, name), getattr(b, name)), (what, name)
    assert torch.equal(a._dev_state, b._dev_state), (what, a._dev_state.tolist(), b._dev_state.tolist())


# ------------------------------------------------------------------ 1. parity against the oracle, commit off
@pytest.mark.parametrize("W", [16, 48])
@pytest.mark.parametrize("ns", [4, 40])
@pytest.mark.parametrize("G", [1, 8])
@pytest.mark.parametrize("dtype,D", TYPES)
def test_admitting_rows_are_a_prefill_and_continuing_rows_keep_their_oracle(dtype, D, G, ns, W):
    mfma = dtype != torch.float32 and D in (64, 80, 96, 128)
    for name, (T, seqs) in PACKS.items():
        lengths, slots = [n for n, _, _ in seqs], [s for _, s, _ in seqs]
        layer, hist = _mixed_pool(dtype, D, W, ns, seqs, seed=110)
        q, k, v, sa = _pack(dtype, D, G, lengths, T, seed=120)
        before = _clone(layer)
        for aux in (sa, None):
            o = _run(layer, q, k, v, _cu(lengths), slots, aux)
            assert ("_mfma_" in _path()) == mfma, _path()
            ref = _reference(q, k, v, aux, hist, W, ns, seqs)
            assert len(ref) == sum(1 for n, s in zip(lengths, slots) if n and s >= 0)
            _check_rows(o, ref, lengths, slots, TOL[dtype], (name, dtype, D, G, ns, W, aux is not None))
            _same_pool(layer, before, "commit off: nothing moves")


# ------------------------------------------------------------------ 2. commit, bitwise
@pytest.mark.parametrize("pack", ["a", "b"])
@pytest.mark.parametrize("dtype,D,G,W,ns", SMALL)
def test_commit_leaves_what_prefill_slots_and_commit_dyn_leave(dtype, D, G, W, ns, pack):
    T, seqs = PACKS[pack]
    lengths, slots = [n for n, _, _ in seqs], [s for _, s, _ in seqs]
    layer, _ = _mixed_pool(dtype, D, W, ns, seqs, seed=210, sentinel=SENTINEL)
    q, k, v, sa = _pack(dtype, D, G, lengths, T, seed=220)
    twin, dry = _clone(layer), _clone(layer)
    twin._pool = dry._pool = True
    o = _run(layer, q, k, v, _cu(lengths), slots, sa, commit=True)
    assert torch.equal(o, _run(dry, q, k, v, _cu(lengths), slots, sa, commit=False))
    _twin_commit(twin, k, v, seqs)
    _same_pool(layer, twin, (pack, dtype, D, G, W, ns))
    for i, (n, s, adm) in enumerate(seqs):
        if adm and s >= 0:
            nsk, rem = min(n, ns), n - min(n, ns)
            assert layer._dev_state[s].tolist() == [nsk, min(rem, W), rem if rem < W else 0, n], (i, s)
    named = {s for n, s, _ in seqs if s >= 0 and n}
    for s in set(range(S)) - named:           # slots that no sequence names, or only an empty one: sentinel, zero state
        for name in BUFS:
            assert (getattr(layer, name)[s] == SENTINEL).all(), ("unnamed slot", s, name)
        assert not layer._dev_state[s].any(), ("unnamed slot", s)


# ------------------------------------------------------------------ 3. without a fresh slot the flag changes nothing
@pytest.mark.parametrize("ns", [4, 40])
@pytest.mark.parametrize("dtype,D,G,W", [(torch.bfloat16, 64, 8, 16), (torch.float16, 128, 1, 48), (torch.float32, 48, 8, 16)])
def test_the_flag_changes_nothing_for_continuing_sequences(dtype, D, G, W, ns):
    # every slot prefilled at the four fills (seen > 0), the pack of tests/test_gpu_ragged_step.py
    layer, _ = _mixed_pool(dtype, D, W, ns, [(1, s, False) for s in range(S)], seed=310, sentinel=SENTINEL)
    assert (layer._dev_state[:, 3] > 0).all()
    q, k, v, sa = _pack(dtype, D, G, LENGTHS, 128, seed=320)
    off, on = _clone(layer), _clone(layer)
    off._pool = on._pool = True
    cu = _cu(LENGTHS)
    for commit in (False, True):
        o_off = _run(off, q, k, v, cu, PERM_HOLE, sa, commit=commit, admit=False)
        o_on = _run(on, q, k, v, cu, PERM_HOLE, sa, commit=commit, admit=True)
        assert torch.equal(o_off, o_on), (commit, maxdiff(o_off, o_on))
        _same_pool(off, on, ("admit on / off", commit))


# ------------------------------------------------------------------ 4. position independence, bitwise
@pytest.mark.parametrize("dtype,D,G,W,ns", SMALL)
def test_an_admitting_sequence_gives_the_same_bits_wherever_it_lies(dtype, D, G, W, ns):
    T, seqs = PACKS["b"]
    lengths, slots = [n for n, _, _ in seqs], [s for _, s, _ in seqs]
    layer, _ = _mixed_pool(dtype, D, W, ns, seqs, seed=410)
    q, k, v, sa = _pack(dtype, D, G, lengths, T, seed=420)
    cu = _cu(lengths)
    o1 = _run(layer, q, k, v, cu, slots, sa)
    order = [5, 2, 0, 6, 3, 1, 4]
    l2 = [lengths[i] for i in order]
    cu2 = _cu(l2)
    gather = torch.cat([torch.arange(cu[i], cu[i] + lengths[i]) for i in order] + [torch.arange(cu[-1], T)])
    o2 = _run(layer, q[:, :, gather], k[:, :, gather], v[:, :, gather], cu2, [slots[i] for i in order], sa)
    for j, i in enumerate(order):
        a, b = o1[:, :, cu[i]:cu[i] + lengths[i]], o2[:, :, cu2[j]:cu2[j] + l2[j]]
        assert torch.equal(a, b), ("sequence", i, "moved to", j, maxdiff(a, b))


# ------------------------------------------------------------------ 5. a chunked prompt, end to end
def _schedule(prompts, first, budget, decode):
    """rows per step and sequence: every prompt takes an equal share of what is left of the budget (the earlier prompts
    the remainder), the first chunk of prompt i is first[i] tokens where given; then `decode` one-token steps"""
    left, steps, begun = list(prompts), [], [False] * len(prompts)
    while any(left):
        room, take = budget, [0] * len(prompts)
        for i in range(len(prompts)):
            if left[i] and not begun[i] and first[i]:
                take[i] = min(first[i], left[i], room)
                room -= take[i]
        live = [i for i in range(len(prompts)) if left[i] and not take[i]]
        for j, i in enumerate(live):
            take[i] = min(left[i], room // (len(live) - j))
            room -= take[i]
        for i in range(len(prompts)):
            left[i] -= take[i]
            begun[i] = begun[i] or take[i] > 0
        steps.append(take)
    return steps + [[1] * len(prompts)] * decode


# num_sink = 4: every admitting chunk of the schedule but the 2-token one holds at least min(prompt, num_sink) tokens.
# num_sink = 40: the first chunks (10, 10, 5, 2 tokens) are all shorter than the sink buffer, so every prompt pins only its
# first chunk and continues behind a short admission with a large sink buffer.
@pytest.mark.parametrize("dtype,D,G,W,ns", [(torch.bfloat16, 64, 8, 16, 4), (torch.float16, 128, 1, 48, 4),
                                            (torch.float32, 48, 1, 16, 4), (torch.bfloat16, 64, 8, 16, 40),
                                            (torch.float16, 128, 1, 48, 40)])
def test_chunked_prompts_through_admitting_steps_only(dtype, D, G, W, ns):
    prompts, first, budget = [100, 37, 5, 20], [0, 0, 0, 2], 32      # the last prompt's first chunk: 2 tokens < num_sink
    slots = [5, 0, 3, 6]
    steps = _schedule(prompts, first, budget, decode=3)
    assert steps[0] == [10, 10, 5, 2] and all(sum(s) <= budget for s in steps) and len(steps) > 5
    total = [p + 3 for p in prompts]
    g = torch.Generator().manual_seed(510)
    seq = [(rand((1, HKV * G, n, D), g, dtype), rand((1, HKV, n, D), g, dtype), rand((1, HKV, n, D), g, dtype)) for n in total]
    sa = rand((HKV * G,), g, torch.float32, 0.8)
    layer = _new_pool(ns, W, S, HKV, D, dtype)
    done = [0] * len(prompts)
    got = [torch.zeros(1, HKV * G, n, D, dtype=torch.float64) for n in total]
    for take in steps:
        cu = _cu(take)
        pad = lambda parts, H: torch.cat(parts + [torch.zeros(1, H, budget - cu[-1], D, dtype=dtype)], dim=2)
        q = pad([seq[i][0][:, :, done[i]:done[i] + take[i]] for i in range(4)], HKV * G)
        k = pad([seq[i][1][:, :, done[i]:done[i] + take[i]] for i in range(4)], HKV)
        v = pad([seq[i][2][:, :, done[i]:done[i] + take[i]] for i in range(4)], HKV)
        pos = layer.packed_positions(cu, slots, budget)
        o = _run(layer, q, k, v, cu, slots, sa, commit=True)
        for i in range(4):
            assert pos[cu[i]:cu[i + 1]].tolist() == list(range(done[i], done[i] + take[i]))
            got[i][:, :, done[i]:done[i] + take[i]] = o[:, :, cu[i]:cu[i + 1]].double().cpu()
            done[i] += take[i]
    assert done == total and layer.positions(slots).tolist() == total
    for i in range(4):
        qi, ki, vi = seq[i]
        f = steps[0][i]
        if f < min(prompts[i], ns):
            # the first chunk pinned only its own tokens as sinks: history_keys(prefill = first chunk, ...) from then on
            head, _ = O.sink_attention_dense(qi[:, :, :f], ki[:, :, :f], vi[:, :, :f], ns, W, sa)
            ref = torch.cat([head, _oracle_rows(qi, ki, vi, sa, f, ns, W, total[i] - f, slice(0, 1))], dim=2)
            assert layer._dev_state[slots[i], 0].item() == f
        else:
            ref, _ = O.sink_attention_dense(qi, ki, vi, ns, W, sa)
            assert layer._dev_state[slots[i], 0].item() == min(ns, prompts[i])
        err = (got[i] - ref).abs().amax(dim=(0, 1, 3))
        assert err.max().item() <= TOL[dtype], ("prompt", i, "row errors", err.tolist())


# ------------------------------------------------------------------ 6. mask-edge probes
# inputs: tests/test_ragged_admit_host.py::admit_probe, whose CPU proof shows that a sink edge wrong by one key, sinks
# clipped by the window or a sink tile classed dead cannot stay within TOL
@pytest.mark.parametrize("W", [16, 48])
@pytest.mark.parametrize("ns", [4, 40])
@pytest.mark.parametrize("dt,D,G", PROBE_TYPES)
def test_mask_edge_probes(dt, D, G, ns, W):
    dtype = P._DT[dt]
    prs = admit_probe(dt, D, G, W, ns)
    sa = prs[0]["s_aux"]
    seqs = [(PROBE_LENGTHS[0], 4, True), (8, 1, False), (PROBE_LENGTHS[1], 2, True), (3, -1, False)]
    lengths, slots = [n for n, _, _ in seqs], [s for _, s, _ in seqs]
    T = 192
    layer, hist = _mixed_pool(dtype, D, W, ns, seqs, seed=610)
    q, k, v, _ = _pack(dtype, D, G, lengths, T, seed=620)
    cu = _cu(lengths)
    for i, pr in ((0, prs[0]), (2, prs[1])):
        sel = slice(cu[i], cu[i] + lengths[i])
        q[:, :, sel], k[:, :, sel], v[:, :, sel] = pr["q"], pr["k"], pr["v"]
    kinds = {P.KINDS[x] for x in prs[0]["kind"].unique().tolist()}
    assert kinds == {"diag", "future", "win_oldest", "win_behind", "sink_last", "sink_next"}, kinds
    o = _run(layer, q, k, v, cu, slots, sa)
    ref = _reference(q, k, v, sa, hist, W, ns, seqs)
    _check_rows(o, ref, lengths, slots, TOL[dtype], ("probe", dt, D, G, ns, W))


# ------------------------------------------------------------------ 7. capture
def test_a_captured_step_admits_continues_and_readmits():
    dtype, D, G, W, ns, T, n_seq = torch.bfloat16, 64, 8, 16, 4, 96, 3
    layer = _new_pool(ns, W, S, HKV, D, dtype, SENTINEL)
    A, B = 2, 5
    sq = torch.zeros(1, HKV * G, T, D, dtype=dtype, device=DEV)
    sk, sv = (torch.zeros(1, HKV, T, D, dtype=dtype, device=DEV) for _ in range(2))
    scu = torch.zeros(n_seq + 1, dtype=torch.int32, device=DEV)
    ssl = torch.full((n_seq,), -1, dtype=torch.int32, device=DEV)
    so = torch.zeros_like(sq)
    sa = rand((HKV * G,), torch.Generator().manual_seed(700), torch.float32, 0.8).to(DEV)
    start = _clone(layer)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):         # warm-up outside the capture (allocates the workspace); all rows inactive
        layer.ragged_step_dyn(sq, sk, sv, scu, ssl, s_aux=sa, out=so, commit=True, admit=True)
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        layer.ragged_step_dyn(sq, sk, sv, scu, ssl, s_aux=sa, out=so, commit=True, admit=True)
    _same_pool(layer, start, "capture runs nothing")
    # (lengths, slots, slots released before the step): A admits; A continues while B admits; A is released and admits a
    # shorter prompt while B decodes
    steps = [([70, 0, 1], [A, -1, -1], []), ([8, 40, 0], [A, B, -1], []), ([1, 0, 9], [B, -1, A], [A])]
    for r, (lengths, slots, free) in enumerate(steps):
        q, k, v, _ = _pack(dtype, D, G, lengths, T, seed=710 + r)
        if free:
            layer.release_slots(free)
        eager = _clone(layer)
        eager._pool = True
        sq.copy_(q), sk.copy_(k), sv.copy_(v)
        scu.copy_(torch.tensor(_cu(lengths), dtype=torch.int32)), ssl.copy_(torch.tensor(slots, dtype=torch.int32))
        graph.replay()
        oe = _run(eager, q, k, v, _cu(lengths), slots, sa.cpu(), commit=True)
        assert torch.equal(so, oe), ("replay", r, maxdiff(so, oe))
        _same_pool(layer, eager, ("replay", r))
    assert layer._dev_state[A].tolist() == [4, 5, 5, 9] and layer._dev_state[B, 3].item() == 41


# ------------------------------------------------------------------ 8. determinism
def test_two_runs_give_the_same_bits():
    T, seqs = PACKS["a"]
    lengths, slots = [n for n, _, _ in seqs], [s for _, s, _ in seqs]
    layer, _ = _mixed_pool(torch.bfloat16, 64, 48, 40, seqs, seed=810)
    q, k, v, sa = _pack(torch.bfloat16, 64, 8, lengths, T, seed=820)
    o1 = _run(layer, q, k, v, _cu(lengths), slots, sa).clone()
    o2 = _run(layer, q, k, v, _cu(lengths), slots, sa)
    assert torch.equal(o1, o2)
