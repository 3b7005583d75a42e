"""GPU tests of the per-sequence device state (ragged batches): SinkCacheLayer.prefill_varlen and the *_dyn methods in
per-sequence mode (sfa_ring_fill_varlen, sfa_decode_ring_step_rows, sfa_decode_ring_multi_rows, sfa_ring_commit_rows).

Anchors: (1) every row of a ragged cache holds bitwise what a B=1 twin driven by append() / decode_step() holds;
(2) with a uniform state the rows calls are bitwise the shared dyn calls; (3) row b of a rows call is bitwise row b of a
shared dyn call on the same B-row buffers at row b's state (the plan depends only on (B, H_kv, row blocks) and the
state); (4) the fp64 oracle over each row's own history."""
import pytest
import torch

from oracle import sink_oracle as O
from test_gpu_decode_multi import TOL
from util import maxdiff, rand

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _path():
    from sink_attention import _native
    return _native.last_path()


def _twin(ns, W, k, v):
    """A B=1 layer prefilled by append() (the reference placement); None for an empty history."""
    from sink_attention import SinkCacheLayer
    t = SinkCacheLayer(ns, W)
    if k.shape[2] > 0:
        t.append(k.to(DEV), v.to(DEV))
    return t


def _assert_row_is_twin(layer, b, twin, what):
    """Row b of a per-sequence layer: buffers bitwise and state row == the twin's host counters (seen included)."""
    row = layer._dev_state[b].tolist()
    if twin.sink_k is None:                    # empty history: untouched buffers, zero state
        assert row == [0, 0, 0, 0], (what, row)
        for buf in (layer.sink_k, layer.sink_v, layer.window_k, layer.window_v):
            assert not buf[b].any(), what
        return
    assert row == [twin.sink_len, twin.window_len, twin.write_pos, twin.seen_tokens], (what, row)
    for x, y in zip((layer.sink_k, layer.sink_v, layer.window_k, layer.window_v),
                    (twin.sink_k, twin.sink_v, twin.window_k, twin.window_v)):
        assert torch.equal(x[b:b + 1], y), what


def _ragged(ns, W, lengths, Hkv, D, dtype, g):
    """A per-sequence layer prefilled by prefill_varlen from one pack, and the per-row histories (CPU)."""
    from sink_attention import SinkCacheLayer
    hist = [(rand((1, Hkv, L, D), g, dtype), rand((1, Hkv, L, D), g, dtype)) for L in lengths]
    cu = [0]
    for L in lengths:
        cu.append(cu[-1] + L)
    k = torch.cat([h[0] for h in hist], dim=2).to(DEV)
    v = torch.cat([h[1] for h in hist], dim=2).to(DEV)
    layer = SinkCacheLayer(ns, W)
    layer.prefill_varlen(k, v, torch.tensor(cu, dtype=torch.int32, device=DEV))
    assert _path() == "ring_fill_varlen", _path()
    return layer, [list(h) for h in hist]


def _keys(sink_len, L, W, t):
    """Positions chunk query t of a row with L tokens of history sees: its sink_len sink tokens (a row prefilled with
    fewer than num_sink tokens keeps only those) and the newest W positions up to L + t."""
    pos = L + t
    return torch.tensor(sorted(set(range(sink_len)) | set(range(max(sink_len, pos - W + 1), pos + 1))))


def _shared_twin(layer, b):
    """A shared-state layer on clones of the per-sequence layer's B-row buffers, its state = row b's first 3 fields."""
    from sink_attention import SinkCacheLayer
    s = SinkCacheLayer(layer.num_sink, layer.window_size)
    s.sink_k, s.sink_v, s.window_k, s.window_v = (t.clone() for t in (layer.sink_k, layer.sink_v, layer.window_k,
                                                                       layer.window_v))
    s.is_initialized = s.prefilled = True
    s._dev_state = layer._dev_state[b, :3].clone()
    return s


# ---------------------------------------------------------------------------------------------- 1. prefill placement
@pytest.mark.parametrize("dtype,D", [(dt, D) for dt in (torch.bfloat16, torch.float16, torch.float32)
                                     for D in (64, 80, 128, 48)])
def test_prefill_varlen_places_every_row_as_a_b1_prefill(dtype, D):
    ns, W, Hkv = 4, 16, 2
    lengths = [0, 1, ns - 1, ns, ns + 1, ns + W, ns + W + 5, 3 * (ns + W)]
    g = torch.Generator().manual_seed(5)
    layer, hist = _ragged(ns, W, lengths, Hkv, D, dtype, g)
    assert layer._dev_state.shape == (len(lengths), 4) and layer._dev_state.dtype == torch.int32
    for b, (k, v) in enumerate(hist):
        _assert_row_is_twin(layer, b, _twin(ns, W, k, v), f"row {b} (L = {lengths[b]})")
    assert layer.positions().tolist() == lengths


def test_prefill_varlen_takes_a_host_list_and_the_cache_form():
    from sink_attention import SinkAttentionCache
    g = torch.Generator().manual_seed(6)
    lengths = [7, 30, 2]
    k = rand((1, 2, sum(lengths), 64), g, torch.bfloat16).to(DEV)
    v = rand((1, 2, sum(lengths), 64), g, torch.bfloat16).to(DEV)
    cache = SinkAttentionCache(num_sink=4, window_size=16)
    st = cache.prefill_varlen(k, v, [0, 7, 37, 39], layer_idx=1)
    assert st.tolist() == [[4, 3, 3, 7], [4, 16, 0, 30], [2, 0, 0, 2]]
    assert cache[1].positions().tolist() == lengths


# ---------------------------------------------------------------------------------------------- 2. uniform state
def _uniform_pair(dtype, B, Hq, Hkv, D, ns, W, pre, g):
    from sink_attention import SinkCacheLayer
    kp, vp = rand((B, Hkv, pre, D), g, dtype).to(DEV), rand((B, Hkv, pre, D), g, dtype).to(DEV)
    shared, rows = SinkCacheLayer(ns, W), SinkCacheLayer(ns, W)
    for c in (shared, rows):
        c.append(kp, vp)
    shared.enable_device_state()
    st = rows.enable_device_state(per_sequence=True)
    assert st.tolist() == [[min(pre, ns), min(pre - min(pre, ns), W), shared.write_pos, pre]] * B
    return shared, rows


def _same_buffers(a, b):
    return all(torch.equal(x, y) for x, y in zip((a.sink_k, a.sink_v, a.window_k, a.window_v),
                                                 (b.sink_k, b.sink_v, b.window_k, b.window_v)))


@pytest.mark.parametrize("dtype,D", [(torch.bfloat16, 64), (torch.float16, 128), (torch.float32, 64),
                                     (torch.bfloat16, 48)])
@pytest.mark.parametrize("pre", [3, 13, 45])
def test_uniform_state_rows_calls_are_bitwise_the_shared_calls(dtype, D, pre):
    g = torch.Generator().manual_seed(11 + pre)
    B, Hq, Hkv, ns, W, n = 3, 8, 2, 4, 16, 3
    shared, rows = _uniform_pair(dtype, B, Hq, Hkv, D, ns, W, pre, g)
    sa = rand((Hq,), g, torch.float32, 0.5).to(DEV)
    seen = pre

    def check(what):
        s, r = shared._dev_state.tolist(), rows._dev_state.tolist()
        assert all(row == s + [seen] for row in r), (what, s, r)
        assert _same_buffers(shared, rows), what

    for one_pass in (False, True):
        shared.one_pass = rows.one_pass = one_pass
        q, k, v = (rand((B, h, 1, D), g, dtype).to(DEV) for h in (Hq, Hkv, Hkv))
        o1 = shared.decode_step_dyn(q, k, v, s_aux=sa)
        o2 = rows.decode_step_dyn(q, k, v, s_aux=sa)
        assert "_ringstep_rows" in _path(), _path()
        seen += 1
        assert torch.equal(o1, o2), ("decode_step", one_pass, maxdiff(o1, o2))
        check(f"decode_step one_pass={one_pass}")
    q, k, v = (rand((B, h, n, D), g, dtype).to(DEV) for h in (Hq, Hkv, Hkv))
    o1 = shared.extend_attention_dyn(q, k, v, s_aux=sa)
    o2 = rows.extend_attention_dyn(q, k, v, s_aux=sa)
    assert "_rows" in _path() and not _path().endswith("_commit"), _path()
    assert torch.equal(o1, o2), maxdiff(o1, o2)
    check("extend_attention")
    o1 = shared.extend_step_dyn(q, k, v, s_aux=sa)
    o2 = rows.extend_step_dyn(q, k, v, s_aux=sa)
    assert _path().endswith("_rows_commit"), _path()
    seen += n
    assert torch.equal(o1, o2), maxdiff(o1, o2)
    check("extend_step")
    k, v = rand((B, Hkv, n, D), g, dtype).to(DEV), rand((B, Hkv, n, D), g, dtype).to(DEV)
    shared.commit_dyn(k, v, torch.tensor(2, device=DEV))
    rows.commit_dyn(k, v, torch.full((B,), 2, dtype=torch.int32, device=DEV))
    assert _path() == "ring_commit_rows", _path()
    seen += 2
    check("commit")


# ------------------------------------------------------------------------- 3 + 4. ragged fills: bitwise anchor, oracle
# (num_sink, ring capacity, prefill length per row, then per-row commits of a 7-token chunk): the rows mix the FILLS of
# test_gpu_decode_multi_dyn.py - sink not full, ring partly filled, the chunk fills the ring (None: ns + W - n), a
# wrapped ring with write_pos != 0, and a ring smaller than the chunk
RAGGED = [
    (4, 16, [2, 9, None, 20], [0, 0, 0, 7]),
    (4, 3, [1, 5, 12, 3], [0, 2, 2, 1]),
]


def _ragged_layer(dtype, Hq, Hkv, D, ns, W, pres, commits, n, g):
    layer, hist = _ragged(ns, W, [ns + W - n if p is None else p for p in pres], Hkv, D, dtype, g)
    kc, vc = rand((len(pres), Hkv, 7, D), g, dtype), rand((len(pres), Hkv, 7, D), g, dtype)
    layer.commit_dyn(kc.to(DEV), vc.to(DEV), torch.tensor(commits, device=DEV))
    for b, a in enumerate(commits):
        hist[b][0] = torch.cat([hist[b][0], kc[b:b + 1, :, :a]], dim=2)
        hist[b][1] = torch.cat([hist[b][1], vc[b:b + 1, :, :a]], dim=2)
    return layer, hist


@pytest.mark.parametrize("n", [1, 3, 8])
@pytest.mark.parametrize("G", [1, 8])
@pytest.mark.parametrize("dtype,D", [(dt, D) for dt in (torch.bfloat16, torch.float16, torch.float32)
                                     for D in (64, 80, 128, 48)])
def test_ragged_extend_attention_is_rowwise_the_shared_call_and_the_oracle(dtype, D, G, n):
    Hkv = 2
    Hq = G * Hkv
    for c, (ns, W, pres, commits) in enumerate(RAGGED):
        g = torch.Generator().manual_seed(100 + 10 * c + n)
        layer, hist = _ragged_layer(dtype, Hq, Hkv, D, ns, W, pres, commits, n, g)
        B = len(pres)
        q, k, v = (rand((B, h, n, D), g, dtype) for h in (Hq, Hkv, Hkv))
        sa = rand((Hq,), g, torch.float32, 0.8)
        st0 = layer._dev_state.clone()
        out = layer.extend_attention_dyn(q.to(DEV), k.to(DEV), v.to(DEV), s_aux=sa.to(DEV))
        assert "_rows" in _path(), _path()
        assert torch.equal(layer._dev_state, st0)
        for b in range(B):
            ref = _shared_twin(layer, b).extend_attention_dyn(q.to(DEV), k.to(DEV), v.to(DEV), s_aux=sa.to(DEV))
            assert torch.equal(out[b], ref[b]), (c, b, maxdiff(out[b], ref[b]))
            L = hist[b][0].shape[2]
            k_all, v_all = torch.cat([hist[b][0], k[b:b + 1]], dim=2), torch.cat([hist[b][1], v[b:b + 1]], dim=2)
            for t in range(n):
                keep = _keys(int(st0[b, 0]), L, W, t)
                o64 = O.decode_dense(q[b:b + 1, :, t:t + 1], k_all[:, :, keep], v_all[:, :, keep], sa)
                assert maxdiff(out[b:b + 1, :, t:t + 1], o64) < TOL[dtype], (c, b, t, maxdiff(out[b:b + 1, :, t:t + 1], o64))


@pytest.mark.parametrize("dtype,D", [(torch.bfloat16, 64), (torch.float16, 80), (torch.float32, 128)])
def test_ragged_extend_step_matches_b1_twins(dtype, D):
    ns, W, n, Hq, Hkv = 4, 16, 3, 8, 2
    g = torch.Generator().manual_seed(21)
    pres, commits = RAGGED[0][2:]
    layer, hist = _ragged_layer(dtype, Hq, Hkv, D, ns, W, pres, commits, n, g)
    twins = []
    for (hk, hv), a in zip(hist, commits):      # the same prefill / commit split as the ragged rows
        P = hk.shape[2] - a
        t = _twin(ns, W, hk[:, :, :P], hv[:, :, :P])
        t.append(hk[:, :, P:].to(DEV), hv[:, :, P:].to(DEV))
        twins.append(t)
    B = len(twins)
    q, k, v = (rand((B, h, n, D), g, dtype).to(DEV) for h in (Hq, Hkv, Hkv))
    out = layer.extend_step_dyn(q, k, v)
    for b, t in enumerate(twins):
        ref = t.extend_step(q[b:b + 1], k[b:b + 1], v[b:b + 1])
        assert maxdiff(out[b:b + 1], ref) < TOL[dtype], (b, maxdiff(out[b:b + 1], ref))
        _assert_row_is_twin(layer, b, t, f"row {b}")


# ---------------------------------------------------------------------------------------------- 5. single-token steps
@pytest.mark.parametrize("one_pass", [False, True])
@pytest.mark.parametrize("dtype,D", [(torch.bfloat16, 64), (torch.float16, 128), (torch.float32, 80)])
def test_decode_step_rows_matches_b1_twins_across_fill(dtype, D, one_pass):
    ns, W, Hq, Hkv = 4, 16, 8, 2
    lengths = [2, 10, 19, 30]                 # rows reach a full ring at different steps
    g = torch.Generator().manual_seed(31)
    layer, hist = _ragged(ns, W, lengths, Hkv, D, dtype, g)
    layer.one_pass = one_pass
    twins = [_twin(ns, W, *h) for h in hist]
    B = len(lengths)
    sa = rand((Hq,), g, torch.float32, 0.5).to(DEV)
    for step in range(20):
        q, k, v = (rand((B, h, 1, D), g, dtype).to(DEV) for h in (Hq, Hkv, Hkv))
        out = layer.decode_step_dyn(q, k, v, s_aux=sa)
        assert "_ringstep_rows" in _path() and ("_1pass" in _path()) == one_pass, _path()
        for b, t in enumerate(twins):
            ref = t.decode_step(q[b:b + 1], k[b:b + 1], v[b:b + 1], s_aux=sa)
            assert maxdiff(out[b:b + 1], ref) < TOL[dtype], (step, b, maxdiff(out[b:b + 1], ref))
            _assert_row_is_twin(layer, b, t, f"step {step} row {b}")
    assert layer.positions().tolist() == [L + 20 for L in lengths]


# ---------------------------------------------------------------------------------------------- 6. per-row commit
@pytest.mark.parametrize("idt", [torch.int32, torch.int64])
def test_commit_rows_matches_per_row_append(idt):
    ns, W, n, Hkv, D, dtype = 4, 8, 5, 2, 64, torch.bfloat16
    lengths = [3, 9, 14, 40, 6]
    counts = [0, n, -2, n + 3, 2]
    g = torch.Generator().manual_seed(41)
    layer, hist = _ragged(ns, W, lengths, Hkv, D, dtype, g)
    twins = [_twin(ns, W, *h) for h in hist]
    for rnd in range(3):
        k, v = rand((len(lengths), Hkv, n, D), g, dtype).to(DEV), rand((len(lengths), Hkv, n, D), g, dtype).to(DEV)
        layer.commit_dyn(k, v, torch.tensor(counts, dtype=idt, device=DEV))
        assert _path() == "ring_commit_rows", _path()
        for b, t in enumerate(twins):
            a = max(0, min(counts[b], n))
            t.append(k[b:b + 1, :, :a], v[b:b + 1, :, :a])
            _assert_row_is_twin(layer, b, t, f"round {rnd} row {b} count {counts[b]}")
        counts = counts[1:] + counts[:1]
    layer.pull_state()
    assert layer.seen_tokens == [t.seen_tokens for t in twins]
    assert layer.window_len == [t.window_len for t in twins]


# ---------------------------------------------------------------------------------- 7. captured speculative loop, B=4
def test_ragged_speculative_loop_captured_in_a_hip_graph():
    """L=3 layers, rows prefilled by prefill_varlen at different lengths.  One captured step = decode_step_dyn of every
    layer (one token per row), extend_attention_dyn of every layer (n drafts per row), per-row acceptance
    a_b = leading matches in torch ops, commit_dyn of every layer.  Every replay matches B=1 eager twins per row and
    layer (decode_step, extend_attention, append of a_b tokens): cache bitwise, outputs within TOL; one replay (ring
    full and wrapped on every row) is checked against the fp64 oracle over layer 0's histories."""
    from sink_attention import SinkCacheLayer
    g = torch.Generator().manual_seed(71)
    dt, Hq, Hkv, D, ns, W, n, L = torch.bfloat16, 16, 2, 64, 4, 16, 4, 3
    lengths = [3, 8, 15, 25]
    B = len(lengths)
    sa = rand((Hq,), g, torch.float32, 0.8).to(DEV)
    layers, twins, hist0 = [], [], None
    for i in range(L):
        layer, hist = _ragged(ns, W, lengths, Hkv, D, dt, g)
        layers.append(layer)
        twins.append([_twin(ns, W, *h) for h in hist])
        if i == 0:
            hist0 = hist
    q1s = [torch.zeros(B, Hq, 1, D, device=DEV, dtype=dt) for _ in range(L)]
    k1s = [torch.zeros(B, Hkv, 1, D, device=DEV, dtype=dt) for _ in range(L)]
    v1s = [torch.zeros(B, Hkv, 1, D, device=DEV, dtype=dt) for _ in range(L)]
    o1s = [torch.zeros(B, Hq, 1, D, device=DEV, dtype=dt) for _ in range(L)]
    qs = [torch.zeros(B, Hq, n, D, device=DEV, dtype=dt) for _ in range(L)]
    ks = [torch.zeros(B, Hkv, n, D, device=DEV, dtype=dt) for _ in range(L)]
    vs = [torch.zeros(B, Hkv, n, D, device=DEV, dtype=dt) for _ in range(L)]
    outs = [torch.zeros(B, Hq, n, D, device=DEV, dtype=dt) for _ in range(L)]
    match = torch.zeros(B, n, dtype=torch.bool, device=DEV)

    def step():
        for i, layer in enumerate(layers):
            layer.decode_step_dyn(q1s[i], k1s[i], v1s[i], s_aux=sa, out=o1s[i])
        for i, layer in enumerate(layers):
            layer.extend_attention_dyn(qs[i], ks[i], vs[i], s_aux=sa, out=outs[i])
        acc = match.int().cumprod(-1).sum(-1)
        for i, layer in enumerate(layers):
            layer.commit_dyn(ks[i], vs[i], acc)

    def fill():
        for bufs in (q1s, k1s, v1s, qs, ks, vs):
            for t in bufs:
                t.copy_(rand(tuple(t.shape), g, dt))
        pat = torch.rand(B, n, generator=g) < 0.8
        match.copy_(pat)
        return [int(x) for x in pat.int().cumprod(-1).sum(-1)]

    def eager(acc, rnd, oracle):
        for i in range(L):
            for b, t in enumerate(twins[i]):
                r1 = t.decode_step(q1s[i][b:b + 1], k1s[i][b:b + 1], v1s[i][b:b + 1], s_aux=sa)
                assert maxdiff(o1s[i][b:b + 1], r1) < TOL[dt], (rnd, i, b, maxdiff(o1s[i][b:b + 1], r1))
                rn = t.extend_attention(qs[i][b:b + 1], ks[i][b:b + 1], vs[i][b:b + 1], s_aux=sa)
                assert maxdiff(outs[i][b:b + 1], rn) < TOL[dt], (rnd, i, b, maxdiff(outs[i][b:b + 1], rn))
                if i == 0:
                    h = hist0[b]
                    h[0] = torch.cat([h[0], k1s[0][b:b + 1].cpu()], dim=2)
                    h[1] = torch.cat([h[1], v1s[0][b:b + 1].cpu()], dim=2)
                    if oracle:
                        Lh = h[0].shape[2]
                        k_all = torch.cat([h[0], ks[0][b:b + 1].cpu()], dim=2)
                        v_all = torch.cat([h[1], vs[0][b:b + 1].cpu()], dim=2)
                        for tq in range(n):
                            keep = _keys(t.sink_len, Lh, W, tq)
                            o64 = O.decode_dense(qs[0][b:b + 1, :, tq:tq + 1].cpu(), k_all[:, :, keep],
                                                 v_all[:, :, keep], sa.cpu())
                            assert maxdiff(outs[0][b:b + 1, :, tq:tq + 1], o64) < TOL[dt], (rnd, b, tq)
                    h[0] = torch.cat([h[0], ks[0][b:b + 1, :, :acc[b]].cpu()], dim=2)
                    h[1] = torch.cat([h[1], vs[0][b:b + 1, :, :acc[b]].cpu()], dim=2)
                t.append(ks[i][b:b + 1, :, :acc[b]], vs[i][b:b + 1, :, :acc[b]])
                _assert_row_is_twin(layers[i], b, t, f"replay {rnd} layer {i} row {b}")

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    acc = fill()
    with torch.cuda.stream(side):           # warm-up outside the graph: builds the per-layer constants
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager(acc, -1, False)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    oracle_done = False
    for rnd in range(16):
        full = all(t.window_len == W for t in twins[0])      # every row's ring full before this replay
        acc = fill()
        graph.replay()
        torch.cuda.synchronize()
        eager(acc, rnd, full and not oracle_done)
        oracle_done = oracle_done or full
    assert oracle_done
    assert min(h[0].shape[2] for h in hist0) - ns > W     # every row filled its ring and wrapped
    assert layers[0].positions().tolist() == [h[0].shape[2] for h in hist0]


# ---------------------------------------------------------------------------------------------- 8. determinism
def test_rows_replays_from_the_same_state_are_bitwise_equal():
    g = torch.Generator().manual_seed(91)
    dt, Hq, Hkv, D, ns, W, n = torch.bfloat16, 64, 8, 64, 4, 512, 8
    layer, _ = _ragged(ns, W, [700, 3, 260, 515], Hkv, D, dt, g)
    B = 4
    q, k, v = (rand((B, h, n, D), g, dt).to(DEV) for h in (Hq, Hkv, Hkv))
    sa = rand((Hq,), g, torch.float32, 0.5).to(DEV)
    out = torch.zeros(B, Hq, n, D, device=DEV, dtype=dt)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        layer.extend_attention_dyn(q, k, v, s_aux=sa, out=out)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        layer.extend_attention_dyn(q, k, v, s_aux=sa, out=out)
    graph.replay()
    torch.cuda.synchronize()
    first = out.clone()
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, first)


# ---------------------------------------------------------------------------------------------- 9. end to end
def test_varlen_prompt_then_prefill_varlen_then_one_batched_verify():
    """sink_flash_attention_varlen on a packed prompt, prefill_varlen of the same pack, then ONE extend_attention_dyn for
    the whole ragged batch: prompt and chunk outputs against the oracle over each full sequence."""
    from sink_attention import SinkCacheLayer, sink_flash_attention_varlen
    g = torch.Generator().manual_seed(97)
    dt, Hq, Hkv, D, ns, W, n = torch.bfloat16, 8, 2, 64, 4, 16, 4
    lengths = [5, 17, 40, 64]
    T = sum(lengths)
    cu = [0]
    for L in lengths:
        cu.append(cu[-1] + L)
    q, k, v = (rand((1, h, T, D), g, dt) for h in (Hq, Hkv, Hkv))
    sa = rand((Hq,), g, torch.float32, 0.8)
    o = sink_flash_attention_varlen(q.to(DEV), k.to(DEV), v.to(DEV), cu, num_sink=ns, window_size=W, s_aux=sa.to(DEV))
    layer = SinkCacheLayer(ns, W)
    layer.prefill_varlen(k.to(DEV), v.to(DEV), torch.tensor(cu, dtype=torch.int32, device=DEV))
    B = len(lengths)
    qc, kc, vc = (rand((B, h, n, D), g, dt) for h in (Hq, Hkv, Hkv))
    out = layer.extend_attention_dyn(qc.to(DEV), kc.to(DEV), vc.to(DEV), s_aux=sa.to(DEV))
    for b, L in enumerate(lengths):
        sl = slice(cu[b], cu[b + 1])
        o_ref, _ = O.sink_attention_dense(q[:, :, sl], k[:, :, sl], v[:, :, sl], ns, W, sa)
        assert maxdiff(o[:, :, sl], o_ref) < TOL[dt], (b, maxdiff(o[:, :, sl], o_ref))
        k_all, v_all = torch.cat([k[:, :, sl], kc[b:b + 1]], dim=2), torch.cat([v[:, :, sl], vc[b:b + 1]], dim=2)
        q_all = torch.cat([q[:, :, sl], qc[b:b + 1]], dim=2)
        o_full, _ = O.sink_attention_dense(q_all, k_all, v_all, ns, W, sa)
        assert maxdiff(out[b:b + 1], o_full[:, :, L:]) < TOL[dt], (b, maxdiff(out[b:b + 1], o_full[:, :, L:]))
