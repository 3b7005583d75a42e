"""GPU tests of the slot-indexed calls (continuous batching): SinkCacheLayer.init_pool / prefill_slots / release_slots and
the slots= keyword of the *_dyn methods (sfa_decode_ring_step_slots, sfa_decode_ring_multi_slots,
sfa_decode_ring_tree_slots, sfa_ring_commit_slots, sfa_ring_commit_path_slots, sfa_ring_fill_varlen_slots).

The oracle is the equivalence rule of include/sfa.h: with P = the pool gathered by index_select(0, slots), X_slots(pool,
slots) gives for every active batch row bitwise the output of X_rows(P) at the same B and leaves pool[slots[b]] bitwise
what X_rows leaves in row b; slots nobody names are untouched; inactive rows (-1) get zeros.  On top of it: B = 1
host-state twins (placement, churn), the fp64 oracle through the stale-content probe (tests/slots_probe.py, proved on the
CPU in tests/test_slots_host.py), and a captured step replayed at changing occupancy."""
import random

import pytest
import torch

from oracle import sink_oracle as O
from slots_probe import stale_probe, true_keys
from test_gpu_decode_multi import TOL
from util import maxdiff, rand

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 7.0
BUFS = ("sink_k", "sink_v", "window_k", "window_v")
TYPES = [(dt, D) for dt in (torch.bfloat16, torch.float16, torch.float32) for D in (64, 80, 128, 48)]

# the fill mix of tests/test_gpu_ragged_cache.py::RAGGED, re-stated: (num_sink, ring capacity, prefill length per row,
# then per-row commits of a 7-token chunk): sink not full, ring partly filled, the chunk fills the ring (None: ns + W -
# n), a wrapped ring with write_pos != 0, and a ring smaller than the chunk
RAGGED = [
    (4, 16, [2, 9, None, 20], [0, 0, 0, 7]),
    (4, 3, [1, 5, 12, 3], [0, 2, 2, 1]),
]


def _path():
    from sink_attention import _native
    return _native.last_path()


def _dev_slots(slots):
    return torch.tensor(slots, dtype=torch.int32, device=DEV)


def _new_pool(ns, W, S, Hkv, D, dtype, sentinel=None):
    from sink_attention import SinkCacheLayer
    layer = SinkCacheLayer(ns, W)
    st = layer.init_pool(S, Hkv, D, dtype, DEV)
    assert st.shape == (S, 4) and not st.any()
    if sentinel is not None:
        for name in BUFS:
            getattr(layer, name).fill_(sentinel)
    return layer


def _prefill(layer, lengths, slots, Hkv, D, dtype, g):
    """prefill_slots of len(lengths) packed sequences into `slots`; returns the per-sequence (k, v) on the CPU"""
    hist = [(rand((1, Hkv, L, D), g, dtype), rand((1, Hkv, L, D), g, dtype)) for L in lengths]
    cu = [0]
    for L in lengths:
        cu.append(cu[-1] + L)
    k = torch.cat([h[0] for h in hist], dim=2).to(DEV)
    v = torch.cat([h[1] for h in hist], dim=2).to(DEV)
    layer.prefill_slots(k, v, cu, slots)
    assert _path() == "ring_fill_varlen_slots", _path()
    return hist


def _mixed_pool(dtype, Hkv, D, ns, W, pres, commits, n, S, g):
    """A pool of S slots, every slot prefilled: slot s gets fill kind s % 4 of the RAGGED row (prefill, then a per-row
    commit of a 7-token chunk through commit_dyn(slots=))."""
    layer = _new_pool(ns, W, S, Hkv, D, dtype)
    lengths = [ns + W - n if pres[s % 4] is None else pres[s % 4] for s in range(S)]
    _prefill(layer, lengths, list(range(S)), Hkv, D, dtype, g)
    kc, vc = rand((S, Hkv, 7, D), g, dtype).to(DEV), rand((S, Hkv, 7, D), g, dtype).to(DEV)
    layer.commit_dyn(kc, vc, torch.tensor([commits[s % 4] for s in range(S)], device=DEV), slots=list(range(S)))
    assert _path() == "ring_commit_slots", _path()
    return layer


def _clone(layer):
    from sink_attention import SinkCacheLayer
    c = SinkCacheLayer(layer.num_sink, layer.window_size)
    for name in BUFS:
        setattr(c, name, getattr(layer, name).clone())
    c._dev_state = layer._dev_state.clone()
    c.is_initialized = c.prefilled = c._per_seq = True
    c.one_pass = layer.one_pass
    return c


def _gathered(layer, slots):
    """P[slots]: a per-sequence layer of B rows, row b = a copy of pool slot slots[b] (inactive rows: the first active
    row's slot - any valid prefilled row)"""
    from sink_attention import SinkCacheLayer
    live = [s for s in slots if s >= 0]
    idx = torch.tensor([s if s >= 0 else live[0] for s in slots], device=DEV)
    r = SinkCacheLayer(layer.num_sink, layer.window_size)
    for name in BUFS:
        setattr(r, name, getattr(layer, name).index_select(0, idx))
    r._dev_state = layer._dev_state.index_select(0, idx)
    r.is_initialized = r.prefilled = r._per_seq = True
    r.one_pass = layer.one_pass
    return r


def _check_rule(pool, slots, call, what, has_out=True):
    """Run `call(layer, slots_or_None)` on the pool with slots and on the gathered rows without, and assert the
    equivalence rule."""
    rows = _gathered(pool, slots)
    before = _clone(pool)
    o_s = call(pool, _dev_slots(slots))
    path = _path()
    assert "_slots" in path, (what, path)
    o_r = call(rows, None)
    assert "_rows" in _path(), (what, _path())
    named = set()
    for b, s in enumerate(slots):
        if s < 0:
            if has_out:
                assert not o_s[b].any(), (what, "inactive row", b)
            continue
        named.add(s)
        if has_out:
            assert torch.equal(o_s[b], o_r[b]), (what, b, s, maxdiff(o_s[b], o_r[b]))
        for name in BUFS:
            assert torch.equal(getattr(pool, name)[s], getattr(rows, name)[b]), (what, name, b, s)
        assert torch.equal(pool._dev_state[s], rows._dev_state[b]), (what, b, s, pool._dev_state[s], rows._dev_state[b])
    for s in range(pool.num_slots):
        if s not in named:
            for name in BUFS:
                assert torch.equal(getattr(pool, name)[s], getattr(before, name)[s]), (what, "unnamed slot", name, s)
            assert torch.equal(pool._dev_state[s], before._dev_state[s]), (what, "unnamed slot state", s)
    return path


# ---------------------------------------------------------------------------------------------- 1. prefill placement
@pytest.mark.parametrize("dtype,D", TYPES)
def test_prefill_slots_places_each_sequence_as_a_b1_prefill(dtype, D):
    from sink_attention import SinkCacheLayer
    ns, W, Hkv, S = 4, 16, 2, 9
    lengths = [1, ns - 1, ns + 1, ns + W, ns + W + 5, 3 * (ns + W)]
    slots = [7, 2, 8, 0, 5, 3]
    g = torch.Generator().manual_seed(5)
    layer = _new_pool(ns, W, S, Hkv, D, dtype, sentinel=SENTINEL)
    layer._dev_state.copy_(torch.arange(4 * S, dtype=torch.int32).view(S, 4) + 100)      # sentinel state rows
    hist = _prefill(layer, lengths, slots, Hkv, D, dtype, g)
    for (k, v), s, L in zip(hist, slots, lengths):
        twin = SinkCacheLayer(ns, W)
        twin.lazy_initialization(k.to(DEV))
        for name in BUFS:
            getattr(twin, name).fill_(SENTINEL)          # rows a prefill does not reach keep their content
        twin.append(k.to(DEV), v.to(DEV))
        assert layer._dev_state[s].tolist() == [twin.sink_len, twin.window_len, twin.write_pos, twin.seen_tokens], (s, L)
        for name in BUFS:
            assert torch.equal(getattr(layer, name)[s:s + 1], getattr(twin, name)), (name, s, L)
    for s in set(range(S)) - set(slots):
        for name in BUFS:
            assert bool((getattr(layer, name)[s] == SENTINEL).all()), (name, s)
        assert layer._dev_state[s].tolist() == [100 + 4 * s + i for i in range(4)], s
    assert layer.positions(slots).tolist() == lengths
    # a device slot tensor with a skipped sequence (-1): nothing of it is stored
    before = _clone(layer)
    k = rand((1, Hkv, 12, D), g, dtype).to(DEV)
    layer.prefill_slots(k, k, torch.tensor([0, 5, 12], dtype=torch.int32, device=DEV), _dev_slots([-1, 1]))
    assert layer._dev_state[1].tolist() == [4, 3, 3, 7]
    for s in set(range(S)) - {1}:
        for name in BUFS:
            assert torch.equal(getattr(layer, name)[s], getattr(before, name)[s]), (name, s)
        assert torch.equal(layer._dev_state[s], before._dev_state[s])


# ------------------------------------------------------------------ 2 + 3. the equivalence rule, inactive rows included
# (S, slots): identity, a permutation, a strict subset of a larger pool, and the subset with an inactive row
SLOT_CASES = [(4, [0, 1, 2, 3]), (4, [2, 0, 3, 1]), (7, [5, 0, 3, 6]), (7, [4, -1, 1, 2]), (7, [-1, 6, -1, 3])]


@pytest.mark.parametrize("G", [1, 8])
@pytest.mark.parametrize("dtype,D", TYPES)
def test_slots_calls_are_bitwise_the_rows_calls_on_the_gathered_pool(dtype, D, G):
    Hkv, n = 2, 3
    Hq, B = G * Hkv, 4
    for c, (ns, W, pres, commits) in enumerate(RAGGED):
        for S, slots in SLOT_CASES:
            g = torch.Generator().manual_seed(200 + 10 * c + S)
            pool = _mixed_pool(dtype, Hkv, D, ns, W, pres, commits, n, S, g)
            sa = rand((Hq,), g, torch.float32, 0.8).to(DEV)
            q1, k1, v1 = (rand((B, h, 1, D), g, dtype).to(DEV) for h in (Hq, Hkv, Hkv))
            q, k, v = (rand((B, h, n, D), g, dtype).to(DEV) for h in (Hq, Hkv, Hkv))
            what = f"case {c} S={S} slots={slots}"

            def step(one_pass):
                def call(layer, s):
                    layer.one_pass = one_pass
                    o = layer.decode_step_dyn(q1, k1, v1, s_aux=sa, slots=s)
                    layer.one_pass = False
                    return o
                return call

            p = _check_rule(pool, slots, step(False), what + " step")
            assert "_ringstep_slots" in p and "_1pass" not in p, p
            p = _check_rule(pool, slots, step(True), what + " step one-pass")
            assert "_ringstep_slots_1pass" in p, p
            p = _check_rule(pool, slots, lambda l, s: l.extend_attention_dyn(q, k, v, s_aux=sa, slots=s),
                            what + " extend_attention")
            assert p.startswith("decode_multi") and p.endswith("_slots"), p
            chain = torch.tensor([-1, 0, 1], dtype=torch.int32, device=DEV)
            o_chain = pool.extend_attention_tree_dyn(q, k, v, chain, s_aux=sa, slots=_dev_slots(slots))
            o_multi = pool.extend_attention_dyn(q, k, v, s_aux=sa, slots=_dev_slots(slots))
            assert torch.equal(o_chain, o_multi), what                 # a chain is the multi call, bit for bit
            p = _check_rule(pool, slots, lambda l, s: l.extend_attention_tree_dyn(q, k, v, chain, s_aux=sa, slots=s),
                            what + " tree (chain)")
            assert p.startswith("decode_tree") and p.endswith("_slots"), p
            tree = torch.tensor([[-1, 0, 0], [-1, -1, 1], [-1, 0, 1], [-1, 0, 0]], dtype=torch.int32, device=DEV)
            _check_rule(pool, slots, lambda l, s: l.extend_attention_tree_dyn(q, k, v, tree, s_aux=sa, slots=s),
                        what + " tree (branching)")
            p = _check_rule(pool, slots, lambda l, s: l.extend_step_dyn(q, k, v, s_aux=sa, slots=s), what + " extend_step")
            assert p.endswith("_slots_commit"), p
            cnt = torch.tensor([0, n, 1, 2], dtype=torch.int32, device=DEV)
            p = _check_rule(pool, slots, lambda l, s: l.commit_dyn(k, v, cnt, slots=s), what + " commit", has_out=False)
            assert p == "ring_commit_slots", p
            path = torch.tensor([[0, 2, 1], [0, 1, 2], [1, 2, 0], [0, 2, 2]], dtype=torch.int32, device=DEV)
            cnt2 = torch.tensor([n, 0, 2, 1], dtype=torch.int32, device=DEV)
            p = _check_rule(pool, slots, lambda l, s: l.commit_path_dyn(k, v, path, cnt2, slots=s),
                            what + " commit_path", has_out=False)
            assert p == "ring_commit_path_slots", p
            # and once more after all those advances (rings wrapped further)
            _check_rule(pool, slots, lambda l, s: l.extend_attention_dyn(q, k, v, s_aux=sa, slots=s), what + " again")


# ---------------------------------------------------------------------------------------------- 4. a slot named twice
@pytest.mark.parametrize("dtype,D", [(torch.bfloat16, 64), (torch.float16, 128), (torch.float32, 48)])
def test_the_same_slot_twice_in_a_reading_call_gives_the_same_bits(dtype, D):
    Hq, Hkv, n, S = 16, 2, 3, 6
    ns, W, pres, commits = RAGGED[0]
    g = torch.Generator().manual_seed(301)
    pool = _mixed_pool(dtype, Hkv, D, ns, W, pres, commits, n, S, g)
    sa = rand((Hq,), g, torch.float32, 0.8).to(DEV)
    q, k, v = (rand((1, h, n, D), g, dtype).to(DEV).expand(4, h, n, D).contiguous() for h in (Hq, Hkv, Hkv))
    slots = _dev_slots([3, 3, 5, 3])
    before = _clone(pool)
    tree = torch.tensor([-1, 0, 0], dtype=torch.int32, device=DEV)
    for out in (pool.extend_attention_dyn(q, k, v, s_aux=sa, slots=slots),
                pool.extend_attention_tree_dyn(q, k, v, tree, s_aux=sa, slots=slots)):
        assert "_slots" in _path(), _path()
        assert torch.equal(out[0], out[1]) and torch.equal(out[0], out[3])
        assert not torch.equal(out[0], out[2])
    for name in BUFS:
        assert torch.equal(getattr(pool, name), getattr(before, name))
    assert torch.equal(pool._dev_state, before._dev_state)


# ---------------------------------------------------------------------------------------------- 5. stale-content probe
@pytest.mark.parametrize("L", [2, 9])
def test_a_reused_slot_does_not_leak_its_previous_tenant(L):
    """The slot's sink rows and whole ring hold keys that are 2 x the codes of the queries to come (tests/slots_probe.py);
    it is released and a short prompt (L = 2: sink not full; L = 9: ring partly filled) is prefilled into it.  Verify and
    step must equal a B = 1 twin that never saw the stale keys and the fp64 oracle.  One leaked stale key moves a row by
    at least 164 x the bf16 tolerance (tests/test_slots_host.py::test_one_leaked_stale_key_exceeds_the_tolerance_tenfold:
    smallest factor 180.9 at L = 2, 164.9 at L = 9; ten are required)."""
    from sink_attention import SinkCacheLayer
    dt, Hq, Hkv, D, ns, W, n, S, slot = torch.bfloat16, 4, 2, 64, 4, 16, 3, 3, 1
    pr = stale_probe(Hq, Hkv, D, ns, W, n, L, dt, seed=3)
    pool = _new_pool(ns, W, S, Hkv, D, dt)
    # the previous tenant: a full sink and a full ring of stale keys
    pool.sink_k[slot], pool.sink_v[slot] = pr["stale_k"][0, :, :ns].to(DEV), pr["stale_v"][0, :, :ns].to(DEV)
    pool.window_k[slot], pool.window_v[slot] = pr["stale_k"][0, :, ns:].to(DEV), pr["stale_v"][0, :, ns:].to(DEV)
    pool._dev_state[slot] = torch.tensor([ns, W, 5, ns + W + 5], dtype=torch.int32, device=DEV)
    pool.release_slots([slot])
    assert pool._dev_state[slot].tolist() == [0, 0, 0, 0]
    assert bool((pool.window_k[slot] == pr["stale_k"][0, :, ns:].to(DEV)).all())        # the content is still there
    pool.prefill_slots(pr["kp"].to(DEV), pr["vp"].to(DEV), [0, L], [slot])
    twin = SinkCacheLayer(ns, W)
    twin.append(pr["kp"].to(DEV), pr["vp"].to(DEV))
    sa = pr["s_aux"].to(DEV)
    q, kc, vc = pr["q"].to(DEV), pr["kc"].to(DEV), pr["vc"].to(DEV)
    slots = _dev_slots([slot])
    out = pool.extend_attention_dyn(q[:, :, :n], kc[:, :, :n], vc[:, :, :n], s_aux=sa, slots=slots)
    ref = twin.extend_attention(q[:, :, :n], kc[:, :, :n], vc[:, :, :n], s_aux=sa)
    print(f"L={L} verify vs twin {maxdiff(out, ref):.3e}")
    assert maxdiff(out, ref) < TOL[dt], maxdiff(out, ref)
    for t in range(n):
        k, v = true_keys(pr, t)
        o64 = O.decode_dense(pr["q"][:, :, t:t + 1], k, v, pr["s_aux"])
        print(f"L={L} verify t={t} vs oracle {maxdiff(out[:, :, t:t + 1], o64):.3e}")
        assert maxdiff(out[:, :, t:t + 1], o64) < TOL[dt], (t, maxdiff(out[:, :, t:t + 1], o64))
    pool.commit_dyn(kc[:, :, :n], vc[:, :, :n], torch.tensor([n], device=DEV), slots=slots)
    twin.append(kc[:, :, :n], vc[:, :, :n])
    for one_pass in (False, True):          # the step (token n), then one more step with the same query
        pool.one_pass = twin.one_pass = one_pass
        o1 = pool.decode_step_dyn(q[:, :, n:], kc[:, :, n:], vc[:, :, n:], s_aux=sa, slots=slots)
        r1 = twin.decode_step(q[:, :, n:], kc[:, :, n:], vc[:, :, n:], s_aux=sa)
        print(f"L={L} step one_pass={one_pass} vs twin {maxdiff(o1, r1):.3e}")
        assert maxdiff(o1, r1) < TOL[dt], (one_pass, maxdiff(o1, r1))
        if not one_pass:
            k, v = true_keys(pr, n)
            o64 = O.decode_dense(pr["q"][:, :, n:], k, v, pr["s_aux"])
            assert maxdiff(o1, o64) < TOL[dt], maxdiff(o1, o64)
    assert pool._dev_state[slot].tolist() == [twin.sink_len, twin.window_len, twin.write_pos, twin.seen_tokens]


# ---------------------------------------------------------------------------------------------- 6. churn
def _assert_slot_is_twin(pool, s, twin, what):
    """Slot s against a B = 1 host-state twin: the state row, and bitwise every row the state makes readable (the sink
    rows below sink_len, the ring slots below window_len).  Rows beyond those belong to whoever had the slot before: a
    reused slot keeps them, the twin (fresh buffers) has zeros there."""
    row = pool._dev_state[s].tolist()
    assert row == [twin.sink_len, twin.window_len, twin.write_pos, twin.seen_tokens], (what, row)
    sl, wl = twin.sink_len, twin.window_len
    assert torch.equal(pool.sink_k[s:s + 1, :, :sl], twin.sink_k[:, :, :sl]), what
    assert torch.equal(pool.sink_v[s:s + 1, :, :sl], twin.sink_v[:, :, :sl]), what
    assert torch.equal(pool.window_k[s:s + 1, :, :wl], twin.window_k[:, :, :wl]), what
    assert torch.equal(pool.window_v[s:s + 1, :, :wl], twin.window_v[:, :, :wl]), what


@pytest.mark.parametrize("dtype,D,G", [(torch.bfloat16, 64, 8), (torch.float16, 80, 1), (torch.float32, 128, 8)])
def test_churn_admit_step_retire_reuse_matches_b1_twins(dtype, D, G):
    from sink_attention import SinkCacheLayer
    ns, W, n, Hkv, S, STEPS = 4, 16, 4, 2, 6, 36
    Hq = G * Hkv
    g = torch.Generator().manual_seed(61)
    rng = random.Random(61)
    pool = _new_pool(ns, W, S, Hkv, D, dtype)
    sa = rand((Hq,), g, torch.float32, 0.8).to(DEV)
    live = {}                # slot -> (twin, steps left)
    admitted = reused = retired = spec = single = 0
    used = set()
    for step in range(STEPS):
        # admit: up to two requests per step into free slots, while the others keep their state
        free = [s for s in range(S) if s not in live]
        rng.shuffle(free)
        n_admit = rng.choice([0, 1, 1, 2]) if step else 3
        for s in free[:max(n_admit, 0 if live else 1)]:
            L = rng.choice([1, 2, 3, 5, 9, 18, 25, 45])
            k, v = rand((1, Hkv, L, D), g, dtype).to(DEV), rand((1, Hkv, L, D), g, dtype).to(DEV)
            pool.prefill_slots(k, v, [0, L], [s])
            twin = SinkCacheLayer(ns, W)
            twin.append(k, v)
            live[s] = [twin, rng.randint(3, 14)]
            admitted += 1
            reused += s in used
            used.add(s)
        slots = list(live)
        rng.shuffle(slots)
        if step % 5 == 4:
            slots.insert(rng.randrange(len(slots) + 1), -1)           # an inactive row in the batch
        B = len(slots)
        act = [(b, s) for b, s in enumerate(slots) if s >= 0]
        if step % 2:                                                  # a single-token step
            pool.one_pass = step % 4 == 3
            q, k, v = (rand((B, h, 1, D), g, dtype).to(DEV) for h in (Hq, Hkv, Hkv))
            out = pool.decode_step_dyn(q, k, v, s_aux=sa, slots=slots)
            assert "_ringstep_slots" in _path() and ("_1pass" in _path()) == pool.one_pass, _path()
            for b, s in act:
                ref = live[s][0].decode_step(q[b:b + 1], k[b:b + 1], v[b:b + 1], s_aux=sa)
                assert maxdiff(out[b:b + 1], ref) < TOL[dtype], (step, b, s, maxdiff(out[b:b + 1], ref))
            single += 1
        else:                                                         # a speculative step with per-row acceptance
            q, k, v = (rand((B, h, n, D), g, dtype).to(DEV) for h in (Hq, Hkv, Hkv))
            out = pool.extend_attention_dyn(q, k, v, s_aux=sa, slots=slots)
            acc = [rng.randint(0, n) for _ in range(B)]
            pool.commit_dyn(k, v, torch.tensor(acc, device=DEV), slots=slots)
            assert _path() == "ring_commit_slots", _path()
            for b, s in act:
                ref = live[s][0].extend_attention(q[b:b + 1], k[b:b + 1], v[b:b + 1], s_aux=sa)
                assert maxdiff(out[b:b + 1], ref) < TOL[dtype], (step, b, s, maxdiff(out[b:b + 1], ref))
                live[s][0].append(k[b:b + 1, :, :acc[b]], v[b:b + 1, :, :acc[b]])
            spec += 1
        for b, s in enumerate(slots):
            if s < 0:
                assert not out[b].any(), (step, b)
        for s, (twin, _left) in live.items():
            _assert_slot_is_twin(pool, s, twin, f"step {step} slot {s}")
        assert pool.positions(slots).tolist() == [live[s][0].seen_tokens if s >= 0 else 0 for s in slots]
        # retire: sequences that are done release their slot
        done = []
        for s in live:
            live[s][1] -= 1
            if live[s][1] <= 0:
                done.append(s)
        if done:
            pool.release_slots(done)
            for s in done:
                assert pool._dev_state[s].tolist() == [0, 0, 0, 0]
                del live[s]
            retired += len(done)
    assert STEPS >= 30 and admitted >= 8 and reused >= 3 and retired >= 4 and spec >= 10 and single >= 10, \
        (admitted, reused, retired, spec, single)


# ---------------------------------------------------------------------------------------------- 7. hipGraph
def test_a_captured_step_replays_at_any_occupancy():
    """One step (verify, acceptance in torch ops, commit_dyn) captured once at B = 4 with a persistent slots tensor.
    Between replays the tensor is rewritten in place (other slots, a -1) and a slot is re-prefilled outside the graph;
    every replay equals the eager call on a cloned pool, bitwise."""
    dt, Hq, Hkv, D, n, S, B = torch.bfloat16, 16, 2, 64, 4, 6, 4
    ns, W, pres, commits = RAGGED[0]
    g = torch.Generator().manual_seed(71)
    pool = _mixed_pool(dt, Hkv, D, ns, W, pres, commits, n, S, g)
    sa = rand((Hq,), g, torch.float32, 0.8).to(DEV)
    q = torch.zeros(B, Hq, n, D, device=DEV, dtype=dt)
    k = torch.zeros(B, Hkv, n, D, device=DEV, dtype=dt)
    v = torch.zeros(B, Hkv, n, D, device=DEV, dtype=dt)
    out = torch.zeros(B, Hq, n, D, device=DEV, dtype=dt)
    match = torch.zeros(B, n, dtype=torch.bool, device=DEV)
    slots = _dev_slots([0, 1, 2, 3])

    def step(layer, o):
        layer.extend_attention_dyn(q, k, v, s_aux=sa, out=o, slots=slots)
        acc = match.int().cumprod(-1).sum(-1)
        layer.commit_dyn(k, v, acc, slots=slots)

    def fill():
        for t in (q, k, v):
            t.copy_(rand(tuple(t.shape), g, dt))
        match.copy_(torch.rand(B, n, generator=g) < 0.8)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    fill()
    with torch.cuda.stream(side):           # warm-up outside the graph: builds the per-layer constants
        step(pool, out)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(pool, out)
    occupancy = [[0, 1, 2, 3], [5, 4, 3, 2], [1, -1, 5, 0], [-1, -1, 4, -1], [2, 3, 0, 1], [4, 0, -1, 5], [3, 5, 1, 2]]
    for rnd in range(14):
        slots.copy_(_dev_slots(occupancy[rnd % len(occupancy)]))      # rewritten in place
        if rnd % 3 == 2:                                              # a slot is retired and reused outside the graph
            s = rnd % S
            pool.release_slots([s])
            L = [3, 11, 30, 50][rnd % 4]
            kk = rand((1, Hkv, L, D), g, dt).to(DEV)
            pool.prefill_slots(kk, kk, [0, L], [s])
        fill()
        torch.cuda.synchronize()
        eager = _clone(pool)
        o_ref = torch.full_like(out, 3.0)
        step(eager, o_ref)
        out.fill_(5.0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, o_ref), (rnd, maxdiff(out, o_ref))
        for name in BUFS:
            assert torch.equal(getattr(pool, name), getattr(eager, name)), (rnd, name)
        assert torch.equal(pool._dev_state, eager._dev_state), (rnd, pool._dev_state, eager._dev_state)
        for b, s in enumerate(occupancy[rnd % len(occupancy)]):
            if s < 0:
                assert not out[b].any(), (rnd, b)
    assert int(pool._dev_state[:, 3].min()) > 0
