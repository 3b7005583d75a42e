"""GPU tests of tree-structured speculative verification over the sink + ring cache (sfa_decode_ring_tree*,
sfa_ring_commit_path_*): (1) a chain-shaped tree is bitwise the multi-token call, (2) random trees / forests against the
fp64 oracle over each node's visible keys, (3) node u against extend_attention of its root-to-u path, (4) per-sequence
trees in a ragged batch against the shared-state call, (5) path commits against append(), (6) a captured 3-layer tree
step (verify, greedy_accept, commit_path_dyn) against an eager twin and the oracle."""
import random

import pytest
import torch

from oracle import sink_oracle as O
from test_gpu_decode_multi import TOL, _assert_same_state, _state, _tokens
from test_gpu_decode_multi_dyn import FILLS, _assert_same_cache, _twins
from test_gpu_ragged_cache import _ragged, _shared_twin
from test_tree_host import depths, path_to, random_tree
from util import maxdiff, rand

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPE_D = [(dt, D) for dt in (torch.bfloat16, torch.float16, torch.float32) for D in (64, 80, 128, 48)]


def _path():
    from sink_attention import _native
    return _native.last_path()


def _tree_path_name(dtype, D):
    if dtype != torch.float32 and D in (64, 80, 96, 128):
        return "decode_tree_mfma_" + {torch.bfloat16: "bf16", torch.float16: "f16"}[dtype] + f"_d{D}"
    return "decode_tree_f32_"


def _chain(n):
    return [-1] + list(range(n - 1))


def _tree_keys(total, sink_len, W, parent, u):
    """Indices into cat(history[0:total], chunk) that node u sees (the contract of include/sfa.h)."""
    d = depths(parent)
    ring = range(max(sink_len, total + d[u] - W + 1), total)
    chunk = [total + v for v in path_to(parent, u) if d[u] - d[v] <= W - 1]
    return torch.tensor(sorted(set(range(sink_len)) | set(ring) | set(chunk)))


def _oracle_tree(q, k, v, sa, total, sink_len, W, parent):
    """fp64 decode_dense per node over the keys it sees; q / k / v hold the history then the chunk on dim 2."""
    rows = []
    for u in range(len(parent)):
        keep = _tree_keys(total, sink_len, W, parent, u)
        rows.append(O.decode_dense(q[:, :, total + u:total + u + 1], k[:, :, keep], v[:, :, keep], sa))
    return torch.cat(rows, dim=2)


# ------------------------------------------------------------------------------------------ 1. chain identity
@pytest.mark.parametrize("n", [3, 8])
@pytest.mark.parametrize("G", [1, 8])
@pytest.mark.parametrize("dtype,D", DTYPE_D)
def test_chain_tree_is_bitwise_the_multi_token_call(dtype, D, G, n):
    Hkv = 2
    for seed, (name, ns, W, prefill, appends) in enumerate(FILLS):
        if prefill is None:
            prefill = ns + W - n
        dyn, host, (qc, kc, vc), sa = _twins(dtype, 1, G * Hkv, Hkv, D, ns, W, prefill, appends, n, 301 + seed)
        chain = _chain(n)
        before, st0 = _state(host), dyn._dev_state.clone()
        out = host.extend_attention_tree(qc, kc, vc, chain, s_aux=sa)
        assert _path().startswith(_tree_path_name(dtype, D)) and "_dyn" not in _path(), _path()
        ref = host.extend_attention(qc, kc, vc, s_aux=sa)
        assert torch.equal(out, ref), (name, maxdiff(out, ref))
        _assert_same_state(_state(host), before, f"{name}: extend_attention_tree modified the cache")
        outd = dyn.extend_attention_tree_dyn(qc, kc, vc, torch.tensor(chain, device=DEV), s_aux=sa)
        assert _path().startswith(_tree_path_name(dtype, D)) and _path().endswith("_dyn"), _path()
        assert torch.equal(outd, dyn.extend_attention_dyn(qc, kc, vc, s_aux=sa)), name
        assert torch.equal(outd, ref), name
        assert torch.equal(dyn._dev_state, st0), name


# ------------------------------------------------------------------------------------------ 2. random trees vs oracle
# (num_sink, ring capacity, prefill, single appends, n, tree shape, forest)
TREES = [
    (4, 16, 9, 0, 12, "random", False),
    (4, 16, 20, 7, 24, "deep", True),        # wrapped ring; depth > Wc: the window clips ring and chunk keys
    (4, 3, 12, 2, 10, "random", True),       # Wc = 3 < most depths
    (0, 32, 50, 0, 20, "star", False),       # depth-1 star
    (4, 64, 100, 5, 64, "random", True),     # 64 nodes: two chunk tiles
    (2, 8, 3, 0, 64, "deep", False),         # a deep tree much longer than the ring
]


@pytest.mark.parametrize("dtype,D", DTYPE_D)
def test_random_trees_match_the_fp64_oracle(dtype, D):
    Hq, Hkv = 8, 2
    for i, (ns, W, prefill, appends, n, shape, forest) in enumerate(TREES):
        parent = random_tree(random.Random(400 + i), n, forest, shape)
        dyn, host, (qc, kc, vc), sa = _twins(dtype, 2, Hq, Hkv, D, ns, W, prefill, appends, n, 410 + i)
        q, k, v, _ = _tokens(2, Hq, Hkv, D, prefill + appends + n, dtype, 410 + i, True)
        out = host.extend_attention_tree(qc, kc, vc, parent, s_aux=sa)
        assert _path().startswith(_tree_path_name(dtype, D)), _path()
        o64 = _oracle_tree(q, k, v, sa.cpu(), prefill + appends, host.sink_len, W, parent)
        assert maxdiff(out, o64) < TOL[dtype], (i, maxdiff(out, o64))
        outd = dyn.extend_attention_tree_dyn(qc, kc, vc, torch.tensor(parent, device=DEV), s_aux=sa)
        assert torch.equal(outd, out), (i, maxdiff(outd, out))
        outb = host.extend_attention_tree(qc, kc, vc, [parent, parent], s_aux=sa)   # [B, n]: the same bits
        assert torch.equal(outb, out), i


# ------------------------------------------------------------------------------------------ 3. path property
@pytest.mark.parametrize("dtype,D", [(torch.bfloat16, 64), (torch.float16, 128), (torch.float32, 48)])
def test_node_u_is_the_last_row_of_its_root_to_u_path(dtype, D):
    ns, W, prefill, n = 4, 8, 30, 20
    parent = random_tree(random.Random(7), n, True, "deep")
    _dyn, host, (qc, kc, vc), sa = _twins(dtype, 1, 16, 2, D, ns, W, prefill, 0, n, 501)
    out = host.extend_attention_tree(qc, kc, vc, parent, s_aux=sa)
    d = depths(parent)
    for u in range(n):
        idx = torch.tensor(path_to(parent, u), device=DEV)
        ref = host.extend_attention(qc[:, :, idx], kc[:, :, idx], vc[:, :, idx], s_aux=sa)
        assert maxdiff(out[:, :, u], ref[:, :, d[u]]) < TOL[dtype], (u, maxdiff(out[:, :, u], ref[:, :, d[u]]))


# ------------------------------------------------------------------------------------------ 4. per-sequence trees
@pytest.mark.parametrize("dtype,D", [(torch.bfloat16, 64), (torch.float16, 80), (torch.float32, 128),
                                     (torch.bfloat16, 48)])
@pytest.mark.parametrize("G", [1, 8])
def test_ragged_trees_are_rowwise_the_shared_call(dtype, D, G):
    ns, W, n, Hkv, B = 4, 16, 10, 2, 4
    g = torch.Generator().manual_seed(600 + G)
    layer, _hist = _ragged(ns, W, [2, 9, ns + W - n, 45], Hkv, D, dtype, g)
    rng = random.Random(601)
    trees = [random_tree(rng, n, b % 2 == 1, ("random", "deep", "star", "random")[b]) for b in range(B)]
    q, k, v = (rand((B, h, n, D), g, dtype).to(DEV) for h in (G * Hkv, Hkv, Hkv))
    sa = rand((G * Hkv,), g, torch.float32, 0.8).to(DEV)
    st0 = layer._dev_state.clone()
    out = layer.extend_attention_tree_dyn(q, k, v, torch.tensor(trees, device=DEV), s_aux=sa)
    assert _path().startswith(_tree_path_name(dtype, D)) and _path().endswith("_rows"), _path()
    assert torch.equal(layer._dev_state, st0)
    for b in range(B):
        ref = _shared_twin(layer, b).extend_attention_tree_dyn(q, k, v, torch.tensor(trees[b], device=DEV), s_aux=sa)
        assert torch.equal(out[b], ref[b]), (b, maxdiff(out[b], ref[b]))
    chain = torch.tensor(_chain(n), device=DEV)
    assert torch.equal(layer.extend_attention_tree_dyn(q, k, v, chain, s_aux=sa),
                       layer.extend_attention_dyn(q, k, v, s_aux=sa))


# ------------------------------------------------------------------------------------------ 5. path commit
@pytest.mark.parametrize("ns,W,prefill,appends,n", [(4, 16, 9, 0, 6), (4, 16, 20, 13, 6), (2, 3, 6, 1, 8)])
def test_commit_path_dyn_matches_append_of_the_path(ns, W, prefill, appends, n):
    raw = [0, 2, 3, -4, n + 5, 5, 1, 4][:n]          # out-of-range entries clamp into [0, n)
    clamped = [min(max(x, 0), n - 1) for x in raw]
    for count in (-1, 0, 2, 4, n, n + 3):
        a = min(max(count, 0), n)
        dyn, host, (_q, kc, vc), _ = _twins(torch.bfloat16, 2, 4, 2, 64, ns, W, prefill, appends, n, 701, aux=False)
        dyn.commit_path_dyn(kc, vc, torch.tensor(raw, device=DEV), torch.tensor(count, device=DEV))
        assert _path() == "ring_commit_path_dyn", _path()
        if a:
            idx = torch.tensor(clamped[:a], dtype=torch.long, device=DEV)
            host.append(kc[:, :, idx], vc[:, :, idx])
        _assert_same_cache(dyn, host, a, f"count {count}")


def test_commit_path_rows_matches_per_row_append():
    from sink_attention import SinkCacheLayer
    ns, W, n, B, dtype = 4, 16, 6, 3, torch.float16
    g = torch.Generator().manual_seed(702)
    k0, v0 = rand((B, 2, 25, 64), g, dtype).to(DEV), rand((B, 2, 25, 64), g, dtype).to(DEV)
    layer = SinkCacheLayer(ns, W)
    layer.append(k0, v0)
    layer.enable_device_state(per_sequence=True)
    kc, vc = rand((B, 2, n, 64), g, dtype).to(DEV), rand((B, 2, n, 64), g, dtype).to(DEV)
    paths = [[0, 1, 3, 5, 2, 4], [0, 2, 9, 1, 1, 1], [0, -3, 4, 5, 2, 3]]
    counts = [3, n + 2, -1]
    layer.commit_path_dyn(kc, vc, torch.tensor(paths, device=DEV), torch.tensor(counts, device=DEV))
    assert _path() == "ring_commit_path_rows", _path()
    for b in range(B):
        a = min(max(counts[b], 0), n)
        twin = SinkCacheLayer(ns, W)
        twin.append(k0[b:b + 1], v0[b:b + 1])
        if a:
            idx = torch.tensor([min(max(x, 0), n - 1) for x in paths[b][:a]], dtype=torch.long, device=DEV)
            twin.append(kc[b:b + 1, :, idx], vc[b:b + 1, :, idx])
        assert layer._dev_state[b].tolist() == [twin.sink_len, twin.window_len, twin.write_pos, twin.seen_tokens], b
        assert torch.equal(layer.window_k[b:b + 1], twin.window_k) and torch.equal(layer.window_v[b:b + 1], twin.window_v)


def test_invalid_parent_entries_read_as_roots_on_the_device():
    n = 12
    dyn, _host, (qc, kc, vc), sa = _twins(torch.bfloat16, 1, 16, 2, 64, 4, 16, 30, 0, n, 703)
    good = random_tree(random.Random(3), n, False, "random")
    bad, clean = list(good), list(good)
    for u, x in ((3, 3), (5, 9), (7, -2), (11, 64)):
        bad[u], clean[u] = x, -1
    o_bad = dyn.extend_attention_tree_dyn(qc, kc, vc, torch.tensor(bad, device=DEV), s_aux=sa)
    o_clean = dyn.extend_attention_tree_dyn(qc, kc, vc, torch.tensor(clean, device=DEV), s_aux=sa)
    assert torch.equal(o_bad, o_clean)


# ------------------------------------------------------------------------------------------ 6. captured tree step
def test_tree_speculative_loop_captured_in_a_hip_graph():
    """L=3 layers, B=4 per-sequence (ragged prefill).  One captured step = extend_attention_tree_dyn of every layer ->
    greedy_accept on device tensors -> commit_path_dyn of every layer.  Each replay is bitwise an eager twin (the same
    calls, not captured) and within TOL of B=1 host-state twins (extend_attention_tree, then commit_path of the path read
    on the host); one replay is checked against the fp64 oracle.  The rounds cross ring fill and wrap.  Two replays
    from the same state are bitwise equal."""
    from sink_attention import SinkCacheLayer, greedy_accept
    g = torch.Generator().manual_seed(801)
    dt, B, Hq, Hkv, D, ns, W, n, L = torch.bfloat16, 4, 16, 2, 64, 4, 16, 7, 3
    parent_l = [[-1, 0, 0, 1, 1, 3, 5], [-1, 0, 1, 2, 3, 4, 5], [-1, 0, 0, 0, 0, 0, 0], [-1, 0, 1, 1, 2, 4, 4]]
    parent = torch.tensor(parent_l, device=DEV)
    pc = torch.tensor(parent_l).clamp(min=0)
    sa = rand((Hq,), g, torch.float32, 0.8).to(DEV)
    pre = [ns + 2, ns + 9, ns + 14, ns + 30]
    cu = [0]
    for p in pre:
        cu.append(cu[-1] + p)
    graph_layers, eager_layers, twins, hist = [], [], [], []
    for _ in range(L):
        kp, vp = rand((B, Hkv, max(pre), D), g, dt), rand((B, Hkv, max(pre), D), g, dt)
        pk = torch.cat([kp[b:b + 1, :, :pre[b]] for b in range(B)], dim=2).to(DEV)
        pv = torch.cat([vp[b:b + 1, :, :pre[b]] for b in range(B)], dim=2).to(DEV)
        a, e = SinkCacheLayer(ns, W), SinkCacheLayer(ns, W)
        a.prefill_varlen(pk, pv, cu)
        e.prefill_varlen(pk, pv, cu)
        graph_layers.append(a)
        eager_layers.append(e)
        rows = []
        for b in range(B):
            t = SinkCacheLayer(ns, W)
            t.append(kp[b:b + 1, :, :pre[b]].to(DEV), vp[b:b + 1, :, :pre[b]].to(DEV))
            rows.append(t)
        twins.append(rows)
        hist.append([[kp[b:b + 1, :, :pre[b]], vp[b:b + 1, :, :pre[b]]] for b in range(B)])
    qs = [torch.zeros(B, Hq, n, D, device=DEV, dtype=dt) for _ in range(L)]
    ks = [torch.zeros(B, Hkv, n, D, device=DEV, dtype=dt) for _ in range(L)]
    vs = [torch.zeros(B, Hkv, n, D, device=DEV, dtype=dt) for _ in range(L)]
    outs = [torch.zeros(B, Hq, n, D, device=DEV, dtype=dt) for _ in range(L)]
    draft = torch.zeros(B, n, dtype=torch.long, device=DEV)
    target = torch.zeros(B, n, dtype=torch.long, device=DEV)
    counts = []

    def step(layers, o):
        for i, layer in enumerate(layers):
            layer.extend_attention_tree_dyn(qs[i], ks[i], vs[i], parent, s_aux=sa, out=o[i])
        path, count = greedy_accept(parent, draft, target)
        for i, layer in enumerate(layers):
            layer.commit_path_dyn(ks[i], vs[i], path, count)
        return path, count

    def fill(rnd):
        for i in range(L):
            qs[i].copy_(rand((B, Hq, n, D), g, dt))
            ks[i].copy_(rand((B, Hkv, n, D), g, dt))
            vs[i].copy_(rand((B, Hkv, n, D), g, dt))
        tg = torch.randint(0, 3, (B, n), generator=g)
        dr = torch.where(torch.rand(B, n, generator=g) < 0.6, tg.gather(1, pc), torch.randint(0, 3, (B, n), generator=g))
        if rnd % 3 == 0:
            dr[:, 1:] = 7                                     # every draft rejected: count = 1
        target.copy_(tg)
        draft.copy_(dr)

    def check(rnd, oracle):
        e_outs = [torch.empty_like(o) for o in outs]
        path, count = step(eager_layers, e_outs)
        for i in range(L):
            assert torch.equal(outs[i], e_outs[i]), (rnd, i, maxdiff(outs[i], e_outs[i]))
            assert torch.equal(graph_layers[i]._dev_state, eager_layers[i]._dev_state), (rnd, i)
            assert torch.equal(graph_layers[i].window_k, eager_layers[i].window_k), (rnd, i)
        pl, cl = path.tolist(), count.tolist()
        counts.extend(cl)
        for i in range(L):
            for b in range(B):
                tw = twins[i][b]
                ref = tw.extend_attention_tree(qs[i][b:b + 1], ks[i][b:b + 1], vs[i][b:b + 1], parent_l[b], s_aux=sa)
                assert maxdiff(outs[i][b:b + 1], ref) < TOL[dt], (rnd, i, b)
                if oracle:
                    hk, hv = hist[i][b]
                    total = hk.shape[2]
                    kk = torch.cat([hk, ks[i][b:b + 1].cpu()], dim=2)
                    vv = torch.cat([hv, vs[i][b:b + 1].cpu()], dim=2)
                    qq = torch.cat([torch.zeros(1, Hq, total, D, dtype=dt), qs[i][b:b + 1].cpu()], dim=2)
                    o64 = _oracle_tree(qq, kk, vv, sa.cpu(), total, tw.sink_len, W, parent_l[b])
                    assert maxdiff(outs[i][b:b + 1], o64) < TOL[dt], (rnd, i, b, maxdiff(outs[i][b:b + 1], o64))
                sel = pl[b][:cl[b]]
                tw.commit_path(ks[i][b:b + 1], vs[i][b:b + 1], sel)
                hist[i][b][0] = torch.cat([hist[i][b][0], ks[i][b:b + 1, :, sel].cpu()], dim=2)
                hist[i][b][1] = torch.cat([hist[i][b][1], vs[i][b:b + 1, :, sel].cpu()], dim=2)
                assert torch.equal(graph_layers[i].window_k[b:b + 1], tw.window_k), (rnd, i, b)
                assert graph_layers[i]._dev_state[b].tolist() == [tw.sink_len, tw.window_len, tw.write_pos,
                                                                  tw.seen_tokens], (rnd, i, b)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    fill(1)
    with torch.cuda.stream(side):              # warm-up outside the graph: builds the per-layer constants
        step(graph_layers, outs)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    check(-1, False)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(graph_layers, outs)
    for rnd in range(6):
        fill(rnd)
        graph.replay()
        torch.cuda.synchronize()
        check(rnd, oracle=rnd == 4)
    assert 1 in counts and max(counts) > 2, counts
    assert all(t.window_len == W for t in twins[0][2:])
    # determinism: two replays from the same state
    fill(5)
    saved = [(x._dev_state.clone(), x.window_k.clone(), x.window_v.clone()) for x in graph_layers]

    def replay():
        graph.replay()
        torch.cuda.synchronize()
        return [o.clone() for o in outs] + [x.window_k.clone() for x in graph_layers] + \
            [x._dev_state.clone() for x in graph_layers]

    first = replay()
    for x, (s, wk, wv) in zip(graph_layers, saved):
        x._dev_state.copy_(s)
        x.window_k.copy_(wk)
        x.window_v.copy_(wv)
    second = replay()
    assert all(torch.equal(x, y) for x, y in zip(first, second))
