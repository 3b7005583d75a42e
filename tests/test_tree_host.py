"""CPU-only tests of tree-structured speculative verification (sfa_decode_ring_tree*, sfa_ring_commit_path_*,
SinkCacheLayer.extend_attention_tree* / commit_path*, sink_attention.spec_tree): exports, workspace, argument checks that
return before any launch, the tree visibility contract (against a replay of append() along each node's root-to-node
path) and the draft-tree helpers against brute force.  No GPU compute."""
import copy
import random

import pytest
import torch

from sink_attention import SinkCacheLayer, greedy_accept, tree_ancestor_mask, tree_depth
from test_decode_multi_host import _abi_args, visible_keys


# ------------------------------------------------------------------ tree model (pure Python)
def depths(parent):
    d = []
    for u, p in enumerate(parent):
        d.append(0 if p < 0 else d[p] + 1)
    return d


def path_to(parent, u):
    """Root-to-u node list."""
    out = [u]
    while parent[out[-1]] >= 0:
        out.append(parent[out[-1]])
    return out[::-1]


def tree_visible_keys(sink_len, window_len, write_pos, Wc, parent, u):
    """Keys node u of a tree chunk may attend to, given the cache state BEFORE the chunk: (sink rows, ring slots, chunk
    nodes).  The contract of include/sfa.h (sfa_decode_ring_tree)."""
    d = depths(parent)
    sinks = list(range(sink_len))
    slots = []
    for s in range(window_len):
        c = (s - write_pos + window_len) % Wc - window_len          # chronological position, -1 = newest
        if c >= d[u] - Wc + 1:
            slots.append(s)
    chunk = [v for v in path_to(parent, u) if d[u] - d[v] <= Wc - 1]
    return sinks, slots, sorted(chunk)


def random_tree(rng, n, forest=False, shape="random"):
    par = []
    for u in range(n):
        if u == 0 or (forest and rng.random() < 0.15):
            par.append(-1)
        elif shape == "star":
            par.append(0)
        elif shape == "deep":
            par.append(u - 1 if rng.random() < 0.85 else rng.randrange(u))
        else:
            par.append(rng.randrange(max(0, u - 4), u))
    return par


def _ids_layer(num_sink, W, prefill):
    ids = torch.arange(prefill, dtype=torch.float32).view(1, 1, -1, 1)
    layer = SinkCacheLayer(num_sink, W)
    layer.append(ids, ids)
    return layer


TREES = [(ns, W, pre, n, forest, shape, seed)
         for seed, (ns, W, pre, n, forest, shape) in enumerate([
             (4, 16, 9, 12, False, "random"), (4, 16, 40, 20, True, "random"), (2, 3, 12, 10, False, "deep"),
             (0, 8, 20, 9, True, "star"), (4, 5, 30, 30, False, "deep"), (4, 64, 100, 64, True, "random"),
             (1, 1, 5, 6, False, "deep"), (4, 16, 2, 16, True, "deep")])]


@pytest.mark.parametrize("ns,W,prefill,n,forest,shape,seed", TREES)
def test_tree_visibility_matches_a_replay_of_append_along_the_path(ns, W, prefill, n, forest, shape, seed):
    rng = random.Random(seed)
    parent = random_tree(rng, n, forest, shape)
    layer = _ids_layer(ns, W, prefill)
    sl, wl, wp = layer.sink_len, layer.window_len, layer.write_pos
    sink_ids = layer.sink_k[0, 0, :, 0].tolist()
    ring_ids = layer.window_k[0, 0, :, 0].tolist()
    node_id = lambda v: 1000 + v
    for u in range(n):
        twin = copy.deepcopy(layer)
        for v in path_to(parent, u):       # depth[u] + 1 single-token steps appending the root-to-u path
            x = torch.full((1, 1, 1, 1), float(node_id(v)))
            twin.append(x, x)
        kk, _ = twin.get_kv()
        replay = sorted(int(x) for x in kk[0, 0, :, 0].tolist())
        sinks, slots, chunk = tree_visible_keys(sl, wl, wp, W, parent, u)
        mine = sorted([int(sink_ids[j]) for j in sinks] + [int(ring_ids[s]) for s in slots] + [node_id(v) for v in chunk])
        assert mine == replay, (u, parent, mine, replay)


@pytest.mark.parametrize("ns,W,prefill,n", [(4, 16, 9, 12), (2, 3, 12, 10), (0, 8, 20, 9), (4, 5, 30, 30)])
def test_tree_visibility_of_a_chain_is_the_multi_token_mask(ns, W, prefill, n):
    layer = _ids_layer(ns, W, prefill)
    chain = [-1] + list(range(n - 1))
    for t in range(n):
        assert tree_visible_keys(layer.sink_len, layer.window_len, layer.write_pos, W, chain, t) == \
            visible_keys(layer.sink_len, layer.window_len, layer.write_pos, W, n, t)


# ------------------------------------------------------------------ spec_tree helpers against brute force
def _brute_accept(parent, draft, target):
    n = len(parent)
    acc = [False] * n
    acc[0] = True
    for u in range(1, n):
        p = parent[u]
        if p < 0 or not acc[p] or draft[u] != target[p]:
            continue
        if any(parent[v] == p and acc[v] for v in range(u)):
            continue
        acc[u] = True
    d = depths(parent)
    path = sorted((u for u in range(n) if acc[u]), key=lambda u: d[u])
    return path, len(path)


def _bad_entries(rng, parent):
    """Entries outside [-1, u) read as -1: corrupt a copy, return it with the cleaned tree it must equal."""
    bad, clean = list(parent), list(parent)
    for u in range(1, len(parent)):
        if rng.random() < 0.1:
            bad[u] = rng.choice([u, u + 3, -2, -7, 99])
            clean[u] = -1
    return bad, clean


@pytest.mark.parametrize("seed", range(12))
def test_tree_depth_and_ancestor_mask_match_brute_force(seed):
    rng = random.Random(100 + seed)
    n = rng.choice([1, 2, 7, 33, 64])
    rows = [random_tree(rng, n, forest=seed % 2 == 1, shape=("random", "deep", "star")[seed % 3]) for _ in range(3)]
    bad, clean = zip(*(_bad_entries(rng, r) for r in rows))
    d = tree_depth(torch.tensor(bad))
    m = tree_ancestor_mask(torch.tensor(bad, dtype=torch.int32))
    assert m.shape == (3, n, n) and m.dtype == torch.bool
    for b, par in enumerate(clean):
        assert d[b].tolist() == depths(par)
        for u in range(n):
            anc = set(path_to(par, u))
            assert [v for v in range(n) if m[b, u, v]] == sorted(anc), (b, u)
    assert tree_depth(torch.tensor(bad[0])).tolist() == depths(clean[0])      # a shared [n] tree


@pytest.mark.parametrize("seed", range(16))
def test_greedy_accept_matches_brute_force(seed):
    rng = random.Random(200 + seed)
    B, n = 4, rng.choice([2, 5, 16, 40, 64])
    shared = seed % 2 == 0
    trees = [random_tree(rng, n, forest=seed % 3 == 0, shape=("random", "deep", "star")[seed % 3])] * B if shared else \
        [random_tree(rng, n, forest=seed % 3 == 0, shape=("random", "deep", "star")[seed % 3]) for _ in range(B)]
    vocab = 3 if seed % 4 == 1 else 6                    # a small vocabulary: many sibling ties
    draft = [[rng.randrange(vocab) for _ in range(n)] for _ in range(B)]
    target = [[rng.randrange(vocab) for _ in range(n)] for _ in range(B)]
    for b in range(B):                                   # make a real accepted path likely
        for u in range(1, n):
            if trees[b][u] >= 0 and rng.random() < 0.5:
                draft[b][u] = target[b][trees[b][u]]
    par = torch.tensor(trees[0]) if shared else torch.tensor(trees)
    path, count = greedy_accept(par, torch.tensor(draft), torch.tensor(target))
    assert path.shape == (B, n) and count.shape == (B,)
    assert int(path.min()) >= 0 and int(path.max()) < n
    for b in range(B):
        ref, c = _brute_accept(trees[b], draft[b], target[b])
        assert int(count[b]) == c and path[b, :c].tolist() == ref, (b, trees[b], draft[b], target[b])


def test_greedy_accept_ties_and_all_rejected():
    parent = torch.tensor([-1, 0, 0, 0, 1, 2, 3])
    target = torch.tensor([[5, 8, 9, 9, 0, 0, 0], [5, 8, 9, 9, 0, 0, 0]])
    draft = torch.tensor([[0, 7, 7, 7, 8, 9, 9],          # nodes 1..3 all match target[0] = 5? no: 7 != 5 -> rejected
                          [0, 5, 5, 4, 8, 9, 9]])         # 1 and 2 carry the accepted token: the lowest index wins
    path, count = greedy_accept(parent, draft, target)
    assert count.tolist() == [1, 3]
    assert path[0, :1].tolist() == [0]
    assert path[1, :3].tolist() == [0, 1, 4]
    p1, c1 = greedy_accept(parent, draft[1], target[1])   # unbatched
    assert int(c1) == 3 and p1[:3].tolist() == [0, 1, 4]


# ------------------------------------------------------------------ library surface
def test_library_exports_the_tree_calls():
    from sink_attention import _native
    lib = _native.lib()
    for name in ("sfa_decode_ring_tree", "sfa_decode_ring_tree_dyn", "sfa_decode_ring_tree_rows",
                 "sfa_ring_commit_path_dyn", "sfa_ring_commit_path_rows"):
        assert hasattr(lib, name), name
    assert lib.sfa_abi_version() == 2
    import sink_attention
    for name in ("sink_decode_attention_ring_tree", "tree_depth", "tree_ancestor_mask", "greedy_accept"):
        assert name in sink_attention.__all__ and hasattr(sink_attention, name)


@pytest.mark.parametrize("B,Hq,Hkv,n,D,dt", [(1, 64, 8, 16, 64, 2), (8, 64, 8, 60, 64, 2), (2, 4, 1, 64, 48, 0)])
def test_tree_workspace_needs_no_gpu_and_is_monotonic(B, Hq, Hkv, n, D, dt):
    """The tree calls size their workspace with sfa_decode_multi_workspace_bytes (same plan, same partials)."""
    from sink_attention import _native
    lib = _native.lib()
    cap = 4 + 4096 + n
    full = lib.sfa_decode_multi_workspace_bytes(B, Hq, Hkv, n, cap, D, dt)
    assert full >= B * Hq * n * (D + 2) * 4
    prev = 0
    for nkv in list(range(n, 400)) + list(range(400, cap + 1, 97)) + [cap]:
        ws = lib.sfa_decode_multi_workspace_bytes(B, Hq, Hkv, n, nkv, D, dt)
        assert 0 < ws <= full and ws >= prev, (nkv, ws, prev, full)
        prev = ws


def _tree_call(N, d, parent_ptr, bstride, which="host", state_ptr=1, **over):
    d = dict(d, **over)
    lib = N.lib()
    if which == "host":
        return lib.sfa_decode_ring_tree(d["q"], d["sk"], d["sv"], 4, d["wk"], d["wv"], 16, 3, d["kn"], d["vn"], d["o"],
                                        None, parent_ptr, bstride, None, 0, 0.125, 0, None)
    fn = lib.sfa_decode_ring_tree_dyn if which == "dyn" else lib.sfa_decode_ring_tree_rows
    return fn(d["q"], d["sk"], d["sv"], d["wk"], d["wv"], d["kn"], d["vn"], d["o"], None, parent_ptr, bstride,
              state_ptr, None, 0, 0.125, 0, None)


@pytest.mark.parametrize("which", ["host", "dyn", "rows"])
def test_tree_c_abi_rejects_bad_arguments_before_any_launch(which):
    N, t, d = _abi_args(B=2, n=3)
    lib = N.lib()
    par = torch.tensor([-1, 0, 0], dtype=torch.int32)        # a host tensor: every call below fails its checks first
    pp = par.data_ptr()
    assert _tree_call(N, d, None, 0, which) == -1 and b"parent" in lib.sfa_last_error()           # null parent
    for bs in (-1, 1, 2):                                                                          # bad batch stride
        assert _tree_call(N, d, pp, bs, which) == -1 and b"parent_bstride" in lib.sfa_last_error(), bs
    for n in (0, 65):
        _, _, dn = _abi_args(B=2, n=n)
        assert _tree_call(N, dn, pp, 0, which) == -1, n
    assert b"64" in lib.sfa_last_error()
    t_bad = torch.zeros(2 * 8 * 3 * 68, dtype=torch.bfloat16).as_strided((2, 8, 3, 64), (8 * 3 * 68, 3 * 68, 68, 1))
    assert _tree_call(N, d, pp, 0, which, q=N.desc(t_bad)) == -1 and b"aligned" in lib.sfa_last_error()   # 136-byte rows
    if which != "host":
        assert _tree_call(N, d, pp, 0, which, state_ptr=None) == -1 and b"state" in lib.sfa_last_error()
    # every argument valid, no workspace: the last check before the launch
    assert _tree_call(N, d, pp, 0, which) == -3 and b"workspace" in lib.sfa_last_error()
    assert _tree_call(N, d, pp, 3, which) == -3


@pytest.mark.parametrize("rows", [False, True])
def test_commit_path_c_abi_rejects_bad_arguments(rows):
    N, t, d = _abi_args(B=2, n=3)
    lib = N.lib()
    fn = lib.sfa_ring_commit_path_rows if rows else lib.sfa_ring_commit_path_dyn
    cnt = torch.zeros(2, dtype=torch.int32)
    path = torch.zeros(2, 3, dtype=torch.int32)
    call = lambda cp, pp, bs, sp=1: fn(d["wk"], d["wv"], d["kn"], d["vn"], cp, pp, bs, sp, None)
    assert call(cnt.data_ptr(), None, 0) == -1 and b"path" in lib.sfa_last_error()
    assert call(None, path.data_ptr(), 0) == -1 and b"count" in lib.sfa_last_error()
    assert call(cnt.data_ptr(), path.data_ptr(), 0, None) == -1 and b"state" in lib.sfa_last_error()
    for bs in (-3, 1, 2):
        assert call(cnt.data_ptr(), path.data_ptr(), bs) == -1 and b"path_bstride" in lib.sfa_last_error(), bs


# ------------------------------------------------------------------ Python surface (host-side checks)
def test_host_tree_calls_validate_parent_before_touching_the_device():
    _, t, _ = _abi_args(n=4)
    layer = SinkCacheLayer(4, 16)
    layer.append(torch.zeros(1, 2, 30, 64, dtype=torch.bfloat16), torch.zeros(1, 2, 30, 64, dtype=torch.bfloat16))
    for bad in ([-1, 0, 2, 1], [-1, 0, -2, 1], [-1, 0, 1], [[-1, 0, 1, 2]] * 2, [0, 0, 1, 2]):
        with pytest.raises(ValueError):
            layer.extend_attention_tree(t["q"], t["kn"], t["vn"], bad)
    with pytest.raises(TypeError):
        layer.extend_attention_tree(t["q"], t["kn"], t["vn"], torch.tensor([-1.0, 0.0, 1.0, 2.0]))
    _, t65, _ = _abi_args(n=65)
    with pytest.raises(ValueError, match="64"):
        layer.extend_attention_tree(t65["q"], t65["kn"], t65["vn"], [-1] + list(range(64)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):         # a valid tree reaches the device check
        layer.extend_attention_tree(t["q"], t["kn"], t["vn"], [-1, 0, 0, 1])
    assert layer.window_len == 16 and layer.seen_tokens == 30


@pytest.mark.parametrize("B", [1, 3])
def test_commit_path_is_append_of_the_gathered_rows(B):
    """Host-state commit_path on CPU tensors (pure bookkeeping): the same buffers and counters as append()."""
    g = torch.Generator().manual_seed(5)
    for ns, W, pre in ((4, 16, 9), (4, 16, 40), (2, 3, 12)):
        k0, v0 = torch.randn(B, 2, pre, 8, generator=g), torch.randn(B, 2, pre, 8, generator=g)
        kn, vn = torch.randn(B, 2, 10, 8, generator=g), torch.randn(B, 2, 10, 8, generator=g)
        paths = [[0, 3, 4, 9], [1, 2, 5, 6], [0, 7, 8, 9]][:B]
        a, b = SinkCacheLayer(ns, W), SinkCacheLayer(ns, W)
        for c in (a, b):
            c.append(k0, v0)
        a.commit_path(kn, vn, torch.tensor(paths) if B > 1 else paths[0])
        for r in range(B):
            ref = SinkCacheLayer(ns, W)
            ref.append(k0[r:r + 1], v0[r:r + 1])
            ref.append(kn[r:r + 1, :, paths[r]], vn[r:r + 1, :, paths[r]])
            assert torch.equal(a.window_k[r:r + 1], ref.window_k) and torch.equal(a.window_v[r:r + 1], ref.window_v)
            assert (a.window_len, a.write_pos, a.seen_tokens) == (ref.window_len, ref.write_pos, ref.seen_tokens)
        with pytest.raises(ValueError):
            b.commit_path(kn, vn, [0, 10])
