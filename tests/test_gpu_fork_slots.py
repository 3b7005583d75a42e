"""GPU tests of the slot copy (sfa_ring_copy_slots, SinkCacheLayer.fork_slots / SinkAttentionCache.fork_slots): the fork
of parallel sampling and beam search, and parking a sequence in a second pool.

The contract of include/sfa.h: the rows the readers of the source's state would read and the state row arrive bitwise
and in place, so every later call on the destination is bitwise the same call on the source; rows the source does not
reach keep what the destination held; pairs with a -1, an out-of-range value or src == dst move nothing; nothing else
in either pool is touched.  On top of it: the fp64 oracle over every fork's own history after the rings have wrapped
past the fork point, the stale-content probe of tests/slots_probe.py, and a captured fork + step replayed with the index
tensors rewritten in place."""
import pytest
import torch

from oracle import sink_oracle as O
from slots_probe import stale_probe, true_keys
from test_decode_multi_host import history_keys
from test_gpu_decode_multi import TOL
from test_gpu_slots import BUFS, DEV, SENTINEL, TYPES, _clone, _dev_slots, _new_pool, _path, _prefill
from util import maxdiff, rand

pytestmark = pytest.mark.gpu
S, HKV, G = 8, 2, 2
GEOMS = [(4, 16), (4, 3), (40, 48)]
SOURCES = [0, 1, 2, 3, 4, 5]          # the slots _source_pool fills, one per state the copy can meet
FREE = [6, 7]


def _fclone(layer):
    c = _clone(layer)
    c._pool = True
    return c


def _source_pool(dtype, D, ns, W, g, tenant=False):
    """A pool of S = 8 slots over sentinel buffers.  Slot 0: fresh; 1: a prompt shorter than num_sink; 2: a partly filled
    ring; 3: a ring filled exactly; 4: a wrapped ring with write_pos != 0 (prefill, then commit_dyn(slots=)); 5: a ring
    smaller than the last chunk (a commit of W + 2 tokens).  Slots 6 and 7 are free: sentinel rows and a zero state, or
    (`tenant`) previous tenants of other lengths, one longer than every source and one shorter than most."""
    layer = _new_pool(ns, W, S, HKV, D, dtype, sentinel=SENTINEL)
    half = max(1, W // 2)
    _prefill(layer, [ns - 1, ns + half, ns + W, ns + W - 1, ns + 2], [1, 2, 3, 4, 5], HKV, D, dtype, g)
    for slot, n in ((4, 3), (5, W + 2)):
        kc, vc = rand((1, HKV, n, D), g, dtype).to(DEV), rand((1, HKV, n, D), g, dtype).to(DEV)
        layer.commit_dyn(kc, vc, torch.tensor([n], device=DEV), slots=[slot])
    assert layer._dev_state[:6].tolist() == [
        [0, 0, 0, 0], [ns - 1, 0, 0, ns - 1], [ns, half, half, ns + half], [ns, W, 0, ns + W],
        [ns, W, 2, ns + W + 2], [ns, W, (W + 4) % W, ns + W + 4]], layer._dev_state
    assert (W + 4) % W != 0
    if tenant:
        _prefill(layer, [2 * (ns + W) + 5, ns + 1], FREE, HKV, D, dtype, g)
    return layer


def _live(layer, s):
    sl, wl = layer._dev_state[s, 0].item(), layer._dev_state[s, 1].item()
    return {"sink_k": sl, "sink_v": sl, "window_k": wl, "window_v": wl}


def _assert_copied(dst_pool, before, src_pool, pairs, what):
    """Every pair (s, d): the state row and the live rows of d equal those of s, the other rows of d hold what they held
    in `before`; every slot of dst_pool that is no destination is bitwise `before`."""
    for s, d in pairs:
        assert torch.equal(dst_pool._dev_state[d], src_pool._dev_state[s]), (what, s, d, dst_pool._dev_state[d])
        for name, n in _live(src_pool, s).items():
            got, src, old = getattr(dst_pool, name)[d], getattr(src_pool, name)[s], getattr(before, name)[d]
            assert torch.equal(got[:, :n], src[:, :n]), (what, name, s, d, "live rows")
            assert torch.equal(got[:, n:], old[:, n:]), (what, name, s, d, "rows the source does not reach")
    named = {d for _, d in pairs}
    for c in range(dst_pool.num_slots):
        if c not in named:
            for name in BUFS:
                assert torch.equal(getattr(dst_pool, name)[c], getattr(before, name)[c]), (what, "unnamed slot", name, c)
            assert torch.equal(dst_pool._dev_state[c], before._dev_state[c]), (what, "unnamed slot state", c)


def _assert_pools_equal(a, b, what):
    for name in BUFS:
        assert torch.equal(getattr(a, name), getattr(b, name)), (what, name)
    assert torch.equal(a._dev_state, b._dev_state), (what, a._dev_state, b._dev_state)


# ---------------------------------------------------------------------------------------------------- 1. bitwise copy
@pytest.mark.parametrize("dtype,D", TYPES)
def test_fork_copies_live_rows_and_state_bitwise_and_nothing_else(dtype, D):
    for gi, (ns, W) in enumerate(GEOMS):
        for tenant in (False, True):
            g = torch.Generator().manual_seed(900 + 2 * gi + tenant)
            pool = _source_pool(dtype, D, ns, W, g, tenant)
            # after the first call the destinations hold the previous call's forks: tenants of yet other lengths
            for k, src in enumerate(([0, 1], [2, 3], [4, 5], [5, 2])):
                before = _fclone(pool)
                pool.fork_slots(src if k % 2 else _dev_slots(src), FREE if k % 2 else _dev_slots(FREE))
                assert _path() == "ring_copy_slots", _path()
                _assert_copied(pool, before, before, list(zip(src, FREE)), f"ns={ns} W={W} tenant={tenant} src={src}")


# ---------------------------------------------------------------------------------------------------- 2. twin behaviour
@pytest.mark.parametrize("dtype,D", TYPES)
def test_a_fork_behaves_bitwise_as_its_source(dtype, D):
    Hq, n = G * HKV, 3
    for gi, (ns, W) in enumerate(GEOMS):
        g = torch.Generator().manual_seed(920 + gi)
        pool = _source_pool(dtype, D, ns, W, g, tenant=True)
        sa = rand((Hq,), g, torch.float32, 0.8).to(DEV)
        for src in ([0, 1], [2, 3], [4, 5]):
            what = f"ns={ns} W={W} src={src}"
            pool.fork_slots(src, FREE)
            q, k, v = (rand((2, h, n, D), g, dtype).to(DEV) for h in (Hq, HKV, HKV))
            q1, k1, v1 = (rand((2, h, 1, D), g, dtype).to(DEV) for h in (Hq, HKV, HKV))
            qr, kr, vr = (rand((1, h, 7, D), g, dtype).to(DEV) for h in (Hq, HKV, HKV))
            calls = {      # the packed step first: it admits the fork of the fresh slot, as it admits the fresh slot
                "ragged_step_dyn": lambda sl: pool.ragged_step_dyn(qr, kr, vr, [0, 2, 7], sl, s_aux=sa, commit=True,
                                                                   admit=True),
                "extend_step_dyn": lambda sl: pool.extend_step_dyn(q, k, v, s_aux=sa, slots=sl),
                "decode_step_dyn": lambda sl: pool.decode_step_dyn(q1, k1, v1, s_aux=sa, slots=sl),
            }
            for name, call in calls.items():
                o_src, o_dst = call(src), call(FREE)
                assert torch.equal(o_src, o_dst), (what, name, maxdiff(o_src, o_dst))
                before = _fclone(pool)
                _assert_copied(pool, before, pool, list(zip(src, FREE)), what + " after " + name)    # live rows, state


@pytest.mark.parametrize("L", [2, 9])
def test_a_fork_over_a_longer_previous_tenant_does_not_leak_it(L):
    """tests/test_gpu_slots.py::test_a_reused_slot_does_not_leak_its_previous_tenant with the fork in the place of the
    prefill: the destination's sink rows and whole ring hold keys that are 2 x the codes of the queries to come, the
    source holds a short prompt.  One leaked stale key moves a row by at least 164 x the bf16 tolerance
    (tests/test_slots_host.py::test_one_leaked_stale_key_exceeds_the_tolerance_tenfold)."""
    from sink_attention import SinkCacheLayer
    dt, Hq, Hkv, D, ns, W, n, slot, src = torch.bfloat16, 4, 2, 64, 4, 16, 3, 1, 2
    pr = stale_probe(Hq, Hkv, D, ns, W, n, L, dt, seed=3)
    pool = _new_pool(ns, W, 3, Hkv, D, dt)
    pool.sink_k[slot], pool.sink_v[slot] = pr["stale_k"][0, :, :ns].to(DEV), pr["stale_v"][0, :, :ns].to(DEV)
    pool.window_k[slot], pool.window_v[slot] = pr["stale_k"][0, :, ns:].to(DEV), pr["stale_v"][0, :, ns:].to(DEV)
    pool._dev_state[slot] = torch.tensor([ns, W, 5, ns + W + 5], dtype=torch.int32, device=DEV)
    pool.prefill_slots(pr["kp"].to(DEV), pr["vp"].to(DEV), [0, L], [src])
    pool.fork_slots([src], [slot])                 # no release in between: the copy alone makes the slot the source's
    assert bool((pool.window_k[slot, :, W - 1] == pr["stale_k"][0, :, ns + W - 1].to(DEV)).all())     # still there
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
    o1 = pool.decode_step_dyn(q[:, :, n:], kc[:, :, n:], vc[:, :, n:], s_aux=sa, slots=slots)
    k, v = true_keys(pr, n)
    o64 = O.decode_dense(pr["q"][:, :, n:], k, v, pr["s_aux"])
    print(f"L={L} step vs oracle {maxdiff(o1, o64):.3e}")
    assert maxdiff(o1, o64) < TOL[dt], maxdiff(o1, o64)
    assert pool._dev_state[slot].tolist() == [min(L, ns), L - min(L, ns) + n + 1, L - min(L, ns) + n + 1, L + n + 1]


# ------------------------------------------------------------------------------------ 3. independence, oracle parity
@pytest.mark.parametrize("dtype,D,ns,W", [(torch.bfloat16, 64, 4, 16), (torch.float16, 80, 4, 3),
                                          (torch.float32, 128, 40, 48), (torch.bfloat16, 48, 4, 16)])
def test_forks_diverge_independently_and_match_the_oracle_on_their_own_history(dtype, D, ns, W):
    Hq, L, src, dsts = G * HKV, ns + 5, 2, [5, 0, 7]
    g = torch.Generator().manual_seed(940)
    pool = _new_pool(ns, W, S, HKV, D, dtype, sentinel=SENTINEL)
    (kp, vp), = _prefill(pool, [L], [src], HKV, D, dtype, g)
    never = _fclone(pool)
    pool.fork_slots([src] * 3, dsts)
    sa = rand((Hq,), g, torch.float32, 0.8)
    rows = [src] + dsts
    hist = [[kp, vp] for _ in rows]
    alone = _dev_slots([src, -1, -1, -1])          # the same B: the split plan of a step follows the call's shape
    worst = 0.0
    for i in range(W + 5):                         # every ring wraps past the fork point
        q, k, v = (rand((4, h, 1, D), g, dtype) for h in (Hq, HKV, HKV))
        out = pool.decode_step_dyn(q.to(DEV), k.to(DEV), v.to(DEV), s_aux=sa.to(DEV), slots=rows)
        ref = never.decode_step_dyn(q.to(DEV), k.to(DEV), v.to(DEV), s_aux=sa.to(DEV), slots=alone)
        assert torch.equal(out[0], ref[0]), (i, maxdiff(out[0], ref[0]))
        keep = torch.tensor(history_keys(L + i, ns, W, 0))
        for r in range(4):
            hist[r] = [torch.cat([hist[r][0], k[r:r + 1]], dim=2), torch.cat([hist[r][1], v[r:r + 1]], dim=2)]
            o64 = O.decode_dense(q[r:r + 1], hist[r][0][:, :, keep], hist[r][1][:, :, keep], sa)
            err = maxdiff(out[r:r + 1], o64)
            worst = max(worst, err)
            assert err < TOL[dtype], (i, r, err)
    print(f"{dtype} D={D} ns={ns} W={W}: worst error against the oracle {worst:.3e} (tolerance {TOL[dtype]:.1e})")
    for name in BUFS:
        assert torch.equal(getattr(pool, name)[src], getattr(never, name)[src]), name
    assert torch.equal(pool._dev_state[src], never._dev_state[src])
    assert pool.positions(rows).tolist() == [L + W + 5] * 4


# ---------------------------------------------------------------------------------------------------- 4. skips
@pytest.mark.parametrize("dtype,D,ns,W", [(torch.bfloat16, 64, 4, 16), (torch.float32, 48, 4, 3),
                                          (torch.float16, 128, 40, 48)])
def test_pairs_with_an_inactive_or_identical_end_move_nothing(dtype, D, ns, W):
    g = torch.Generator().manual_seed(960)
    pool = _source_pool(dtype, D, ns, W, g, tenant=True)
    before = _fclone(pool)
    # src = -1, dst = -1, a source and a destination outside the pool (device tensors are not validated), src == dst;
    # the two live pairs among them are still copied
    src = _dev_slots([-1, 2, 9, 4, 3, 1, 5])
    dst = _dev_slots([0, -1, 2, 4, S, 7, 6])
    pool.fork_slots(src, dst)
    assert _path() == "ring_copy_slots", _path()
    _assert_copied(pool, before, before, [(1, 7), (5, 6)], "skips")
    pool.fork_slots(_dev_slots([-1, 3, S]), _dev_slots([0, -1, 2]))           # no live pair at all
    pool.fork_slots([-1, 3, 2], [0, -1, 2])                                    # ... and as host lists
    pool.fork_slots([], [])
    after = _fclone(pool)
    _assert_copied(pool, before, before, [(1, 7), (5, 6)], "skips, then nothing")
    _assert_pools_equal(pool, after, "no live pair")


# ---------------------------------------------------------------------------------------------------- 5. two pools
@pytest.mark.parametrize("dtype,D,ns,W", [(torch.bfloat16, 64, 4, 16), (torch.float16, 48, 4, 3),
                                          (torch.float32, 80, 40, 48)])
def test_park_in_a_second_pool_and_unpark_into_other_slots(dtype, D, ns, W):
    Hq, n = G * HKV, 3
    g = torch.Generator().manual_seed(970)
    a = _source_pool(dtype, D, ns, W, g)
    never = _fclone(a)                                        # slots 2 and 4 stay where they are
    b = _new_pool(ns, W, 3, HKV, D, dtype, sentinel=SENTINEL)
    b._dev_state.copy_(torch.arange(12, dtype=torch.int32).view(3, 4) + 50)
    b0 = _fclone(b)
    b.fork_slots([2, 4], [2, 0], source=a)                    # park
    assert _path() == "ring_copy_slots", _path()
    _assert_copied(b, b0, a, [(2, 2), (4, 0)], "park")
    _assert_pools_equal(a, never, "the source pool after parking")
    parked = _fclone(b)
    a.release_slots([2, 4])
    _prefill(a, [ns + W + 3, 2], [4, 2], HKV, D, dtype, g)    # other sequences take the slots
    a0 = _fclone(a)
    a.fork_slots(_dev_slots([2, 0]), _dev_slots([6, 7]), source=b)     # unpark somewhere else
    _assert_copied(a, a0, b, [(2, 6), (0, 7)], "unpark")
    _assert_pools_equal(b, parked, "the side pool after unparking")    # slot 1 of it was never named
    assert b._dev_state[1].tolist() == [54, 55, 56, 57] and bool((b.window_k[1] == SENTINEL).all())
    sa = rand((Hq,), g, torch.float32, 0.8).to(DEV)
    for step in range(3):
        q, k, v = (rand((2, h, n, D), g, dtype).to(DEV) for h in (Hq, HKV, HKV))
        q1, k1, v1 = (rand((2, h, 1, D), g, dtype).to(DEV) for h in (Hq, HKV, HKV))
        for name, call in {"extend_step_dyn": lambda p, sl: p.extend_step_dyn(q, k, v, s_aux=sa, slots=sl),
                           "decode_step_dyn": lambda p, sl: p.decode_step_dyn(q1, k1, v1, s_aux=sa, slots=sl)}.items():
            got, ref = call(a, [6, 7]), call(never, [2, 4])
            assert torch.equal(got, ref), (step, name, maxdiff(got, ref))
            assert torch.equal(a._dev_state[[6, 7]], never._dev_state[[2, 4]]), (step, name)
            for (s, d) in ((2, 6), (4, 7)):
                for buf, live in _live(never, s).items():
                    assert torch.equal(getattr(a, buf)[d][:, :live], getattr(never, buf)[s][:, :live]), (step, name, buf)


# ---------------------------------------------------------------------------------------------------- 6. all layers
def test_the_cache_forks_every_layer():
    from sink_attention import SinkAttentionCache
    dt, D, ns, W = torch.bfloat16, 64, 4, 16
    g = torch.Generator().manual_seed(980)
    cache = SinkAttentionCache(ns, W)
    for l in range(2):
        cache.init_pool(S, HKV, D, dt, DEV, layer_idx=l)
        k, v = rand((1, HKV, 30, D), g, dt).to(DEV), rand((1, HKV, 30, D), g, dt).to(DEV)
        cache.prefill_slots(k, v, [0, 7, 30], [1, 3], layer_idx=l)
    befores = [_fclone(layer) for layer in cache.layers]
    cache.fork_slots([1, 3, 1], [0, 6, 2])
    for l, layer in enumerate(cache.layers):
        _assert_copied(layer, befores[l], befores[l], [(1, 0), (3, 6), (1, 2)], f"layer {l}")
    assert not torch.equal(cache[0].window_k[0], cache[1].window_k[0])         # each layer got its own rows
    side = SinkAttentionCache(ns, W)
    for l in range(2):
        side.init_pool(2, HKV, D, dt, DEV, layer_idx=l)
    side0 = [_fclone(layer) for layer in side.layers]
    side.fork_slots([3], [1], source=cache)
    for l, layer in enumerate(side.layers):
        _assert_copied(layer, side0[l], cache[l], [(3, 1)], f"side layer {l}")


# ---------------------------------------------------------------------------------------------------- 7. hipGraph
def test_a_captured_fork_and_step_replay_with_rewritten_indices():
    """fork_slots with device src / dst of length 4, then one packed step on the destinations, captured once.  Between
    replays the two index tensors are rewritten in place: three live pairs, none, one source into four destinations.
    Every replay equals the eager calls on a cloned pool, bitwise."""
    dt, D, ns, W, Hq, T = torch.bfloat16, 64, 4, 16, G * HKV, 10
    g = torch.Generator().manual_seed(990)
    pool = _source_pool(dt, D, ns, W, g, tenant=True)
    sa = rand((Hq,), g, torch.float32, 0.8).to(DEV)
    q = torch.zeros(1, Hq, T, D, device=DEV, dtype=dt)
    k = torch.zeros(1, HKV, T, D, device=DEV, dtype=dt)
    v = torch.zeros(1, HKV, T, D, device=DEV, dtype=dt)
    out = torch.zeros(1, Hq, T, D, device=DEV, dtype=dt)
    cu = torch.tensor([0, 1, 3, 6, 10], dtype=torch.int32, device=DEV)
    src, dst = _dev_slots([-1] * 4), _dev_slots([-1] * 4)

    def step(layer, o):
        layer.fork_slots(src, dst)
        layer.ragged_step_dyn(q, k, v, cu, dst, s_aux=sa, out=o, commit=True, admit=True)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):           # warm-up outside the graph (allocates the workspace): nothing is live
        step(pool, out)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(pool, out)
    rounds = [([3, 1, -1, 2], [6, 7, -1, 0]),       # three live pairs; the step runs on slots 6, 7, 0
              ([3, -1, S, 5], [3, 6, 7, -1]),       # none: src == dst, src = -1, src outside the pool, dst = -1
              ([4, 4, 4, 4], [1, 2, 6, 7])]         # one source into four destinations
    for rnd, (s_, d_) in enumerate(rounds):
        src.copy_(_dev_slots(s_))
        dst.copy_(_dev_slots(d_))
        for t in (q, k, v):
            t.copy_(rand(tuple(t.shape), g, dt))
        torch.cuda.synchronize()
        eager = _fclone(pool)
        o_ref = torch.full_like(out, 3.0)
        step(eager, o_ref)
        out.fill_(5.0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, o_ref), (rnd, maxdiff(out, o_ref))
        _assert_pools_equal(pool, eager, f"replay {rnd}")
    assert pool._dev_state[[1, 2, 6, 7], 3].tolist() == [pool._dev_state[4, 3].item() + n for n in (1, 2, 3, 4)]


# ---------------------------------------------------------------------------------------------------- 8. determinism
def test_the_same_fork_twice_from_the_same_start_leaves_the_same_bits():
    dt, D, ns, W = torch.float16, 80, 40, 48
    g = torch.Generator().manual_seed(995)
    pool = _source_pool(dt, D, ns, W, g, tenant=True)
    one, two = _fclone(pool), _fclone(pool)
    for p in (one, two):
        p.fork_slots(_dev_slots([4, 4, 1]), _dev_slots([6, 7, 0]))
    _assert_pools_equal(one, two, "two runs")
    assert not torch.equal(one.window_k, pool.window_k)
