"""Packed ragged step with draft trees and per-sequence commit (sfa_decode_ring_ragged_tree_slots /
SinkCacheLayer.ragged_step_dyn(parent=, commit_seq=)) and the packed commit (sfa_ring_commit_path_ragged_slots /
commit_packed_dyn).

A sequence of at most 64 tokens that is not admitting is a draft tree: every node must come out as decode_dense over the
keys of its root-to-node path (the construction of tests/test_gpu_tree_verify.py::_oracle_tree, re-stated here); every
other sequence keeps the ragged mask.  A chain-shaped parent is bitwise the plain ragged call; a sequence gives the same
bits alone and in the pack; commit_seq stores what the existing call stores, for the named sequences only; the packed
commit is bitwise commit_path_dyn(slots=) per sequence.  Pool of 8 slots, H_kv = 2, num_sink = 4, Wc in {16, 48},
lengths [1, 7, 0, 16, 33, 64, 70] (64: the last tree length, 70 ignores parent), T padded to 200."""
import pytest
import torch

import probe_inputs as P
from oracle import sink_oracle as O
from sink_attention import SinkCacheLayer, spec_tree
from test_gpu_slots import BUFS, SENTINEL, _clone, _dev_slots, _new_pool, _path
from test_ragged_tree_host import (LENGTHS, PROBE_TREES, PROBE_TYPES, binary, chain, comb, corrupt, rand_tree, read_as, star,
                                   tree_probe_pack)
from test_tree_host import depths, path_to
from util import DECODE_TOL, maxdiff, rand

pytestmark = pytest.mark.gpu
DEV = "cuda"
HKV, NS, S = 2, 4, 8
T_PAD = 200                             # 191 rows of sequences and a padded tail of 9
PERM = [3, 0, 5, 2, 7, 1, 4]            # sequence i -> slot PERM[i] (slot 6 is named by none)
PERM_HOLE = [3, -1, 5, 2, 7, 1, 4]      # ... with the 7-token sequence inactive
# bf16 / f16 at 64, 80, 96, 128 and fp32 at 48, 80, G in {1, 8}, paired
CASES = [(torch.bfloat16, 64, 8), (torch.float16, 80, 1), (torch.bfloat16, 96, 1), (torch.float16, 128, 8),
         (torch.bfloat16, 128, 1), (torch.float16, 64, 1), (torch.float32, 48, 8), (torch.float32, 80, 1)]
SMALL = [(torch.bfloat16, 64, 8, 16), (torch.float16, 128, 1, 48), (torch.bfloat16, 80, 8, 48), (torch.float32, 48, 8, 16)]


def _cu(lengths):
    cu = [0]
    for n in lengths:
        cu.append(cu[-1] + n)
    return cu


def _i32(x):
    return torch.tensor(x, dtype=torch.int32, device=DEV)


def _pool(dtype, D, W, seed, fresh=(), sentinel=None):
    """A pool of S slots at the fills of tests/test_gpu_ragged_step.py (per slot s % 4: a sink that is not full under an
    empty ring, a ring partly filled, filled exactly, full and wrapped to write_pos != 0); the slots in `fresh` stay as
    init_pool leaves them.  Returns (layer, hist): hist[s] = the prefill and the committed tokens of slot s, on the CPU."""
    g = torch.Generator().manual_seed(seed)
    layer = _new_pool(NS, W, S, HKV, D, dtype, sentinel)
    fills = [[(2, 0), (9, 0), (NS + W, 0), (NS + W + 4, 7)][s % 4] for s in range(S)]
    live = [s for s in range(S) if s not in fresh]
    pre = {s: (rand((1, HKV, fills[s][0], D), g, dtype), rand((1, HKV, fills[s][0], D), g, dtype)) for s in live}
    layer.prefill_slots(torch.cat([pre[s][0] for s in live], dim=2).to(DEV), torch.cat([pre[s][1] for s in live], dim=2).to(DEV),
                        _cu([fills[s][0] for s in live]), live)
    kc, vc = rand((len(live), HKV, 7, D), g, dtype), rand((len(live), HKV, 7, D), g, dtype)
    layer.commit_dyn(kc.to(DEV), vc.to(DEV), torch.tensor([fills[s][1] for s in live], device=DEV), slots=live)
    hist = {}
    for j, s in enumerate(live):
        c = fills[s][1]
        hist[s] = dict(pre=pre[s], com=(kc[j:j + 1, :, :c], vc[j:j + 1, :, :c]))
    for s in fresh:
        z = torch.zeros(1, HKV, 0, D, dtype=dtype)
        hist[s] = dict(pre=(z, z), com=(z, z))
    return layer, hist


def _hist_kv(h):
    return torch.cat([h["pre"][0], h["com"][0]], dim=2), torch.cat([h["pre"][1], h["com"][1]], dim=2)


def _pack(dtype, D, G, T, seed):
    g = torch.Generator().manual_seed(seed)
    q = rand((1, HKV * G, T, D), g, dtype)
    k, v = rand((1, HKV, T, D), g, dtype), rand((1, HKV, T, D), g, dtype)
    sa = rand((HKV * G,), g, torch.float32, 0.8)
    return q, k, v, sa


def _parents(lengths, trees, T, stale=5):
    """the packed parent array: per sequence its tree (local entries), `stale` behind the pack"""
    out = []
    for n, t in zip(lengths, trees):
        assert len(t) == n
        out += t
    return out + [stale] * (T - len(out))


# two assignments of tree shapes to LENGTHS = [1, 7, 0, 16, 33, 64, 70]; the 70-token sequence gets a star / a random tree,
# which the kernels must ignore (read_as: its chain)
def _mix_a():
    return [chain(1), star(7), [], binary(16), rand_tree(33, 3), comb(64), star(70)]


def _mix_b():
    return [[7], rand_tree(7, 4), [], corrupt(rand_tree(16, 5), 1)[0], comb(33), rand_tree(64, 6), rand_tree(70, 7)]


def _tree_keys(total, sink_len, W, parent, u):
    """Indices into cat(history[0:total], chunk) that node u sees (the contract of include/sfa.h)."""
    d = depths(parent)
    ring = range(max(sink_len, total + d[u] - W + 1), total)
    chunk = [total + v for v in path_to(parent, u) if d[u] - d[v] <= W - 1]
    return torch.tensor(sorted(set(range(sink_len)) | set(ring) | set(chunk)))


def _oracle_tree(q, k, v, sa, total, sink_len, W, parent):
    """fp64 decode_dense per node over the keys it sees; k / v hold the history then the chunk on dim 2, q the chunk."""
    rows = []
    for u in range(len(parent)):
        keep = _tree_keys(total, sink_len, W, parent, u)
        rows.append(O.decode_dense(q[:, :, u:u + 1], k[:, :, keep], v[:, :, keep], sa))
    return torch.cat(rows, dim=2)


def _oracle(q, k, v, sa, hist, W, lengths, slots, trees):
    """f64 rows of every active sequence {i: [1, Hq, n_i, D]}: per node over its root-to-node path, with the tree the
    device reads (read_as: bad entries as roots, a chain beyond 64 tokens)"""
    cu, out = _cu(lengths), {}
    for i, (n, s) in enumerate(zip(lengths, slots)):
        if n == 0 or s < 0:
            continue
        hk, hv = _hist_kv(hist[s])
        L = hk.shape[2]
        sel = slice(cu[i], cu[i] + n)
        out[i] = _oracle_tree(q[:, :, sel], torch.cat([hk, k[:, :, sel]], dim=2), torch.cat([hv, v[:, :, sel]], dim=2), sa, L,
                              min(hist[s]["pre"][0].shape[2], NS), W, read_as(trees[i], n))
    return out


def _run(layer, q, k, v, cu, slots, parent=None, commit_seq=None, sa=None, commit=False, admit=False, out=None):
    o = layer.ragged_step_dyn(q.to(DEV), k.to(DEV), v.to(DEV), _i32(cu), _dev_slots(slots),
                              s_aux=None if sa is None else sa.to(DEV), out=out, commit=commit, admit=admit,
                              parent=None if parent is None else _i32(parent),
                              commit_seq=None if commit_seq is None else _i32(commit_seq))
    want = "decode_tree_" if parent is not None else "decode_multi_"
    assert _path().startswith(want) and "_ragged" in _path(), _path()
    return o


def _check_rows(o, ref, lengths, tol, what):
    """active rows within tol of the oracle (each figure printed first), every other row exactly zero"""
    cu = _cu(lengths)
    live = torch.zeros(o.shape[2], dtype=torch.bool)
    for i, r in ref.items():
        got = o[:, :, cu[i]:cu[i] + lengths[i]].double().cpu()
        err = (got - r).abs().amax(dim=(0, 1, 3))
        print(what, "sequence", i, "n", lengths[i], "max error", err.max().item(), "tol", tol)
        assert err.max().item() <= tol, (what, "sequence", i, "row errors", err.tolist())
        live[cu[i]:cu[i] + lengths[i]] = True
    assert not o[:, :, ~live.to(o.device)].any(), (what, "inactive / empty / padded rows must be zero")


def _same_pool(a, b, what, slots=None):
    for s in (range(S) if slots is None else slots):
        for name in BUFS:
            assert torch.equal(getattr(a, name)[s], getattr(b, name)[s]), (what, "slot", s, name)
        assert torch.equal(a._dev_state[s], b._dev_state[s]), (what, "state row", s, a._dev_state[s], b._dev_state[s])


# ------------------------------------------------------------------ 1. parity against the oracle
@pytest.mark.parametrize("W", [16, 48])
@pytest.mark.parametrize("dtype,D,G", CASES)
def test_every_node_is_decode_dense_over_its_root_to_node_path(dtype, D, G, W):
    layer, hist = _pool(dtype, D, W, seed=11)
    q, k, v, sa = _pack(dtype, D, G, T_PAD, seed=12)
    cu = _cu(LENGTHS)
    for slots, aux, trees in ((PERM_HOLE, sa, _mix_a()), (PERM, None, _mix_b())):
        before = _clone(layer)
        o = _run(layer, q, k, v, cu, slots, _parents(LENGTHS, trees, T_PAD), sa=aux)
        mfma = dtype != torch.float32 and D in (64, 80, 96, 128)
        assert _path().startswith("decode_tree_mfma_" if mfma else "decode_tree_f32_") and _path().endswith("_ragged"), _path()
        ref = _oracle(q, k, v, aux, hist, W, LENGTHS, slots, trees)
        assert len(ref) == sum(1 for n, s in zip(LENGTHS, slots) if n and s >= 0)
        _check_rows(o, ref, LENGTHS, DECODE_TOL[dtype], (dtype, D, G, W))
        _same_pool(layer, before, "commit off: nothing moves")


# ------------------------------------------------------------------ 2. rule (a): a chain is the plain ragged call, bitwise
@pytest.mark.parametrize("W", [16, 48])
@pytest.mark.parametrize("dtype,D,G", CASES)
def test_a_chain_shaped_parent_is_bitwise_the_plain_ragged_call(dtype, D, G, W):
    # slot 7 (the 33-token sequence) is fresh: with admit=True it is admitted in the call
    layer, _ = _pool(dtype, D, W, seed=21, fresh=(7,))
    q, k, v, sa = _pack(dtype, D, G, T_PAD, seed=22)
    cu = _cu(LENGTHS)
    chains = [chain(n) for n in LENGTHS]
    # ... and where the kernels must not read it: the admitting sequence and the one of 70 tokens hold other trees
    stale = chains[:4] + [star(33), chain(64), rand_tree(70, 8)]
    for admit, trees in ((False, chains), (True, chains), (True, stale)):
        par = _parents(LENGTHS, trees, T_PAD, stale=-7)
        plain, tree = _clone(layer), _clone(layer)
        plain._pool = tree._pool = True
        o1 = _run(plain, q, k, v, cu, PERM_HOLE, None, sa=sa, commit=True, admit=admit)
        o2 = _run(tree, q, k, v, cu, PERM_HOLE, par, sa=sa, commit=True, admit=admit)
        assert _path().endswith("_ragged_admit_commit" if admit else "_ragged_commit"), _path()
        for i, n in enumerate(LENGTHS):
            a, b = o1[:, :, cu[i]:cu[i] + n], o2[:, :, cu[i]:cu[i] + n]
            assert torch.equal(a, b), ("admit", admit, "sequence", i, "n", n, maxdiff(a, b))
        assert torch.equal(o1, o2)
        _same_pool(plain, tree, ("admit", admit))


# ------------------------------------------------------------------ 3. rule (b): alone or in the pack, the same bits
@pytest.mark.parametrize("dtype,D,G,W", SMALL)
def test_a_sequence_gives_the_same_bits_alone_and_next_to_its_neighbours(dtype, D, G, W):
    layer, _ = _pool(dtype, D, W, seed=31, fresh=(7,))          # the 33-token sequence is admitting
    q, k, v, sa = _pack(dtype, D, G, T_PAD, seed=32)
    cu = _cu(LENGTHS)
    trees = _mix_a()
    full = _run(layer, q, k, v, cu, PERM_HOLE, _parents(LENGTHS, trees, T_PAD), sa=sa, admit=True)
    for i, n in enumerate(LENGTHS):
        if n == 0 or PERM_HOLE[i] < 0:
            continue
        # sequence i alone at the head of a pack of the same (T, n_seq): its neighbours are empty
        lengths = [n if j == i else 0 for j in range(len(LENGTHS))]
        sel = torch.arange(cu[i], cu[i] + n)
        q1, k1, v1 = (torch.zeros_like(t) for t in (q, k, v))
        q1[:, :, :n], k1[:, :, :n], v1[:, :, :n] = q[:, :, sel], k[:, :, sel], v[:, :, sel]
        alone = _run(layer, q1, k1, v1, _cu(lengths), PERM_HOLE, trees[i] + [3] * (T_PAD - n), sa=sa, admit=True)
        a, b = full[:, :, cu[i]:cu[i] + n], alone[:, :, :n]
        assert torch.equal(a, b), ("sequence", i, "n", n, maxdiff(a, b))
        assert not alone[:, :, n:].any()


# ------------------------------------------------------------------ 4. agreement with the per-batch tree call
@pytest.mark.parametrize("dtype,D,G,W", SMALL)
def test_equal_lengths_agree_with_extend_attention_tree_dyn(dtype, D, G, W):
    layer, _ = _pool(dtype, D, W, seed=41)
    slots, n = [4, 2, 7, 0, 3], 16
    B = len(slots)
    q, k, v, sa = _pack(dtype, D, G, n * B, seed=42)
    trees = [rand_tree(n, 10 + b) for b in range(B - 1)] + [comb(n)]
    o = _run(layer, q, k, v, _cu([n] * B), slots, _parents([n] * B, trees, n * B), sa=sa)
    unpack = lambda t: t.reshape(t.shape[1], B, n, D).transpose(0, 1).contiguous().to(DEV)
    ref = layer.extend_attention_tree_dyn(unpack(q), unpack(k), unpack(v), _i32(trees), s_aux=sa.to(DEV), slots=slots)
    got = o.reshape(HKV * G, B, n, D).transpose(0, 1)
    print("max difference", maxdiff(got, ref), "tol", DECODE_TOL[dtype])
    assert maxdiff(got, ref) <= DECODE_TOL[dtype], maxdiff(got, ref)


# ------------------------------------------------------------------ 5. per-sequence commit
@pytest.mark.parametrize("dtype,D,G,W", SMALL)
def test_commit_seq_stores_the_named_sequences_and_nothing_else(dtype, D, G, W):
    # decode row, masked decode row, chunk (70), tree (16, masked), chain draft (7), admitting (33, fresh slot 7), masked
    # admitting (5, fresh slot 6), inactive (12); slot 3 is fresh and named by none
    lengths = [1, 1, 70, 16, 7, 33, 5, 12]
    slots = [0, 1, 2, 4, 5, 7, 6, -1]
    mask = [1, 0, 1, 0, 1, 1, 0, 1]
    T = 160
    layer, _ = _pool(dtype, D, W, seed=51, fresh=(3, 6, 7), sentinel=SENTINEL)
    q, k, v, sa = _pack(dtype, D, G, T, seed=52)
    cu = _cu(lengths)
    trees = [chain(1), chain(1), star(70), rand_tree(16, 20), chain(7), chain(33), chain(5), star(12)]
    par = _parents(lengths, trees, T)
    before, twin, dry = _clone(layer), _clone(layer), _clone(layer)
    twin._pool = dry._pool = True
    o = _run(layer, q, k, v, cu, slots, par, commit_seq=mask, sa=sa, commit=True, admit=True)
    assert _path().endswith("_ragged_admit_commit"), _path()
    assert torch.equal(o, _run(dry, q, k, v, cu, slots, par, sa=sa, commit=False, admit=True))
    _run(twin, q, k, v, cu, slots, None, sa=sa, commit=True, admit=True)          # the existing call stores every sequence
    for i, s in enumerate(slots):
        if s < 0:
            continue
        _same_pool(layer, twin if mask[i] else before, ("sequence", i, "commit_seq", mask[i]), [s])
        assert mask[i] == 0 or layer._dev_state[s, 3].item() == before._dev_state[s, 3].item() + lengths[i]
    _same_pool(layer, before, "a slot no sequence names keeps its sentinel", [3])
    assert all((getattr(layer, name)[3] == SENTINEL).all() for name in BUFS) and not layer._dev_state[3].any()
    # commit == 0 wins over the mask; a null mask with a parent stores everything
    _run(dry, q, k, v, cu, slots, par, commit_seq=mask, sa=sa, commit=False, admit=True)
    _same_pool(dry, before, "commit = 0")
    _run(dry, q, k, v, cu, slots, par, sa=sa, commit=True, admit=True)
    _same_pool(dry, twin, "parent without a mask commits every sequence")


# ------------------------------------------------------------------ 6. the packed commit
def _append_twin(h, k_path, v_path, W):
    """the host-state cache of one slot on the CPU: its prefill, its committed tokens, then append() of the path tokens"""
    tw = SinkCacheLayer(NS, W)
    tw.append(h["pre"][0].clone(), h["pre"][1].clone())
    if h["com"][0].shape[2]:
        tw.append(h["com"][0], h["com"][1])
    if k_path.shape[2]:
        tw.append(k_path, v_path)
    return tw


@pytest.mark.parametrize("use_path", [True, False])
@pytest.mark.parametrize("dtype,D,W", [(torch.bfloat16, 64, 16), (torch.float16, 80, 48), (torch.float32, 48, 16),
                                       (torch.bfloat16, 128, 48)])
def test_commit_packed_dyn_is_bitwise_the_per_sequence_path_commit(dtype, D, W, use_path):
    layer, hist = _pool(dtype, D, W, seed=61, sentinel=SENTINEL)
    _, k, v, _ = _pack(dtype, D, 1, T_PAD, seed=62)
    cu = _cu(LENGTHS)
    # counts: all of one token; an inactive sequence; an empty one; more than n_i; negative; a > Wc at Wc = 16; n_i
    counts = [1, 3, 2, 20, -3, 40, 70]
    g = torch.Generator().manual_seed(63)
    path = []
    for n in LENGTHS:
        p = torch.randint(0, max(n, 1), (n,), generator=g).tolist()
        if n >= 7:
            p[1], p[2] = n + 3, -2                   # entries outside [0, n): clamped on the device
        path += p
    path += [9] * (T_PAD - len(path))
    twin, before = _clone(layer), _clone(layer)
    layer.commit_packed_dyn(k.to(DEV), v.to(DEV), _i32(cu), _dev_slots(PERM_HOLE), _i32(counts),
                            path=_i32(path) if use_path else None)
    assert _path() == "ring_commit_path_ragged_slots", _path()
    for i, (n, s) in enumerate(zip(LENGTHS, PERM_HOLE)):
        if n == 0 or s < 0:
            continue
        sel = slice(cu[i], cu[i] + n)
        kc, vc, cnt = k[:, :, sel].to(DEV), v[:, :, sel].to(DEV), _i32([counts[i]])
        if use_path:
            twin.commit_path_dyn(kc, vc, _i32(path[sel]), cnt, slots=[s])
        else:
            twin.commit_dyn(kc, vc, cnt, slots=[s])
        # ... and the ring is what append() of the path tokens leaves
        a = min(max(counts[i], 0), n)
        idx = [min(max(x, 0), n - 1) for x in path[sel][:a]] if use_path else list(range(a))
        tw = _append_twin(hist[s], k[:, :, sel][:, :, idx], v[:, :, sel][:, :, idx], W)
        assert layer._dev_state[s].tolist() == [tw.sink_len, tw.window_len, tw.write_pos, tw.seen_tokens], (i, s)
        assert torch.equal(layer.window_k[s, :, :tw.window_len].cpu(), tw.window_k[0, :, :tw.window_len]), (i, s)
        assert torch.equal(layer.window_v[s, :, :tw.window_len].cpu(), tw.window_v[0, :, :tw.window_len]), (i, s)
    _same_pool(layer, twin, "packed commit against the per-sequence commits")
    named = [s for n, s in zip(LENGTHS, PERM_HOLE) if n and s >= 0]
    _same_pool(layer, before, "inactive, empty and unnamed slots", [s for s in range(S) if s not in named])
    _same_pool(layer, before, "count <= 0 changes nothing", [PERM_HOLE[4]])


# ------------------------------------------------------------------ 7. mask-edge probes
# inputs and reference: tests/test_ragged_tree_host.py::tree_probe_pack, whose CPU proof shows that a sibling shown or the
# oldest window key dropped in a tree sequence of this pack cannot stay within DECODE_TOL
@pytest.mark.parametrize("W", [16, 48])
@pytest.mark.parametrize("dt,D,G", PROBE_TYPES)
def test_mask_edge_probes(dt, D, G, W):
    dtype = P._DT[dt]
    q, k, v, sa, hist, lengths, parent, ref, _ = tree_probe_pack(dt, D, G, W)
    layer = _new_pool(NS, W, S, HKV, D, dtype)
    slots = [5, 1, 3, 0, 6, 2]
    kp, vp = torch.cat([h[0] for h in hist], dim=2), torch.cat([h[1] for h in hist], dim=2)
    layer.prefill_slots(kp.to(DEV), vp.to(DEV), _cu([h[0].shape[2] for h in hist]), slots)
    o = _run(layer, q, k, v, _cu(lengths), slots, parent, sa=sa)
    assert len(PROBE_TREES[W]) == len(lengths)
    _check_rows(o, ref, lengths, DECODE_TOL[dtype], ("probe", dt, D, G, W))


# ------------------------------------------------------------------ 8. determinism
def test_two_runs_give_the_same_bits():
    layer, _ = _pool(torch.bfloat16, 64, 16, seed=71)
    q, k, v, sa = _pack(torch.bfloat16, 64, 8, T_PAD, seed=72)
    par = _parents(LENGTHS, _mix_b(), T_PAD)
    o1 = _run(layer, q, k, v, _cu(LENGTHS), PERM, par, sa=sa).clone()
    o2 = _run(layer, q, k, v, _cu(LENGTHS), PERM, par, sa=sa)
    assert torch.equal(o1, o2)


# ------------------------------------------------------------------ 9. one captured graph for the whole step
def _twin_step(twin, q, k, v, sa, lengths, slots, trees, mask, draft, target, W):
    """the step through the existing B = 1 calls, sequence by sequence: returns {i: output rows}; `twin` ends as the pool
    must.  Admitting: prefill_slots; stored in the step: extend_step_dyn; a draft tree: extend_attention_tree_dyn,
    greedy_accept and commit_path_dyn."""
    cu, out = _cu(lengths), {}
    for i, (n, s) in enumerate(zip(lengths, slots)):
        if n == 0 or s < 0:
            continue
        sel = slice(cu[i], cu[i] + n)
        qi, ki, vi = q[:, :, sel].to(DEV), k[:, :, sel].to(DEV), v[:, :, sel].to(DEV)
        if twin._dev_state[s, 3].item() == 0:          # admitting (always stored here)
            assert mask[i] == 1
            twin.prefill_slots(ki, vi, [0, n], [s])
            out[i] = None
        elif mask[i]:
            out[i] = twin.extend_step_dyn(qi, ki, vi, s_aux=sa.to(DEV), slots=[s])
        else:
            par = _i32(trees[i])
            out[i] = twin.extend_attention_tree_dyn(qi, ki, vi, par, s_aux=sa.to(DEV), slots=[s])
            path, count = spec_tree.greedy_accept(par, draft[sel].to(DEV), target[sel].to(DEV))
            twin.commit_path_dyn(ki, vi, path, count.reshape(1), slots=[s])
    return out


def test_one_captured_graph_serves_decode_trees_chunks_and_admission():
    dtype, D, G, W, T, n_seq = torch.bfloat16, 64, 8, 16, 112, 6
    layer, _ = _pool(dtype, D, W, seed=81, fresh=(6, 7))
    sq = torch.zeros(1, HKV * G, T, D, dtype=dtype, device=DEV)
    sk, sv = (torch.zeros(1, HKV, T, D, dtype=dtype, device=DEV) for _ in range(2))
    scu, ssl = torch.zeros(n_seq + 1, dtype=torch.int32, device=DEV), torch.full((n_seq,), -1, dtype=torch.int32, device=DEV)
    spar, scs = torch.full((T,), -1, dtype=torch.int32, device=DEV), torch.zeros(n_seq, dtype=torch.int32, device=DEV)
    sdr, stg = (torch.zeros(T, dtype=torch.int64, device=DEV) for _ in range(2))
    so = torch.zeros_like(sq)
    sa = rand((HKV * G,), torch.Generator().manual_seed(80), torch.float32, 0.8)
    sad = sa.to(DEV)

    def step():
        layer.ragged_step_dyn(sq, sk, sv, scu, ssl, s_aux=sad, out=so, commit=True, admit=True, parent=spar, commit_seq=scs)
        path, count = spec_tree.greedy_accept_packed(spar, sdr, stg, scu, n_seq)
        layer.commit_packed_dyn(sk, sv, scu, ssl, count * (1 - scs), path=path)

    start = _clone(layer)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):         # warm-up outside the capture (allocates the workspace); all rows inactive
        step()
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    _same_pool(layer, start, "warm-up and capture with every sequence inactive")
    # (lengths, slots, trees, commit_seq): all decode; trees + a chunk + an admission; partly inactive with a readmission
    steps = [([1, 1, 1, 1, 1, 1], [0, 1, 2, 3, 4, 5], [chain(1)] * 6, [1] * 6),
             ([16, 70, 7, 9, 1, 5], [1, 2, 3, 6, 4, 0], [rand_tree(16, 30, False), star(70), binary(7), chain(9), chain(1),
                                                         comb(5)], [0, 1, 0, 1, 1, 0]),
             ([33, 4, 0, 12, 1, 40], [5, -1, 2, 7, -1, 3], [comb(33), star(4), [], chain(12), chain(1), chain(40)],
              [0, 0, 1, 1, 1, 1])]
    for r, (lengths, slots, trees, mask) in enumerate(steps):
        q, k, v, _ = _pack(dtype, D, G, T, seed=82 + r)
        g = torch.Generator().manual_seed(90 + r)
        draft, target = torch.randint(0, 2, (T,), generator=g), torch.randint(0, 2, (T,), generator=g)
        twin = _clone(layer)
        twin._pool = True
        sq.copy_(q), sk.copy_(k), sv.copy_(v), sdr.copy_(draft), stg.copy_(target)
        scu.copy_(torch.tensor(_cu(lengths), dtype=torch.int32)), ssl.copy_(torch.tensor(slots, dtype=torch.int32))
        spar.copy_(torch.tensor(_parents(lengths, trees, T), dtype=torch.int32))
        scs.copy_(torch.tensor(mask, dtype=torch.int32))
        graph.replay()
        ref = _twin_step(twin, q, k, v, sa, lengths, slots, trees, mask, draft, target, W)
        cu = _cu(lengths)
        live = torch.zeros(T, dtype=torch.bool)
        for i, o in ref.items():
            live[cu[i]:cu[i] + lengths[i]] = True
            if o is not None:
                d = maxdiff(so[:, :, cu[i]:cu[i] + lengths[i]], o)
                print("replay", r, "sequence", i, "n", lengths[i], "max difference", d)
                assert d <= DECODE_TOL[dtype], ("replay", r, "sequence", i, d)
        assert not so[:, :, ~live.to(DEV)].any()
        _same_pool(layer, twin, ("replay", r))
