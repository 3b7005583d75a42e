"""GPU parity of the device-state multi-token decode (sfa_decode_ring_multi_dyn / sfa_ring_commit_dyn):
SinkCacheLayer.extend_attention_dyn / extend_step_dyn / commit_dyn against twin layers driven by the host-state calls
(extend_attention / extend_step / append), BITWISE: the dyn kernels replan from the device state with the host formulas,
so the same state runs the same tile-to-split assignment and fold order.  Then a speculative loop of several layers
captured once into a hipGraph (verify, acceptance count in torch ops, commit) and replayed across ring fill and wrap."""
import pytest
import torch

from oracle import sink_oracle as O
from test_decode_multi_host import history_keys
from test_gpu_decode_multi import TOL, _assert_same_state, _state, _tokens
from util import maxdiff, rand

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _path():
    from sink_attention import _native
    return _native.last_path()


def _expected_path(dtype, D):
    if dtype != torch.float32 and D in (64, 80, 96, 128):
        return "decode_multi_mfma_" + {torch.bfloat16: "bf16", torch.float16: "f16"}[dtype] + f"_d{D}"
    return "decode_multi_f32_"


# (name, num_sink, ring capacity, prefill tokens, single appends after the prefill); the chunk fill level is from n
FILLS = [
    ("sink_not_full", 4, 16, 2, 0),
    ("ring_partly_filled", 4, 16, 9, 0),
    ("chunk_fills_ring", 4, 16, None, 0),      # prefill = 4 + 16 - n: the chunk takes the ring's last free slots
    ("wrapped_ring", 4, 16, 20, 7),            # full ring, write_pos = 7
    ("n_over_capacity", 4, 3, 12, 2),          # Wc = 3 < n for n = 8
]


def _twins(dtype, B, Hq, Hkv, D, ns, W, prefill, appends, n, seed, aux=True):
    """Two layers holding the same history: `dyn` (state on the device) and `host`; plus the chunk."""
    from sink_attention import SinkCacheLayer
    total = prefill + appends
    q, k, v, sa = _tokens(B, Hq, Hkv, D, total + n, dtype, seed, aux)
    dyn, host = SinkCacheLayer(ns, W), SinkCacheLayer(ns, W)
    for c in (dyn, host):
        c.append(k[:, :, :prefill].to(DEV), v[:, :, :prefill].to(DEV))
        for i in range(prefill, total):
            c.append(k[:, :, i:i + 1].to(DEV), v[:, :, i:i + 1].to(DEV))
    dyn.enable_device_state()
    chunk = tuple(x[:, :, total:].to(DEV) for x in (q, k, v))
    return dyn, host, chunk, (sa.to(DEV) if sa is not None else None)


def _dev_state(layer):
    return layer._dev_state.clone()


def _assert_same_cache(dyn, host, committed, what):
    """Buffers bitwise and counters equal after dyn.pull_state(); seen_tokens only where pull_state() can count it
    (fewer than window_size tokens committed since the last pull)."""
    dyn.pull_state()
    a, b = _state(dyn), _state(host)
    if committed >= dyn.window_size:
        a = a[:3] + (b[3],) + a[4:]
    _assert_same_state(a, b, what)


@pytest.mark.parametrize("n", [1, 3, 8])
@pytest.mark.parametrize("G", [1, 8])
@pytest.mark.parametrize("dtype,D", [(dt, D) for dt in (torch.bfloat16, torch.float16, torch.float32)
                                     for D in (64, 80, 96, 128, 48)])
def test_extend_attention_dyn_is_bitwise_the_host_state_call(dtype, D, G, n):
    Hkv = 2
    for seed, (name, ns, W, prefill, appends) in enumerate(FILLS):
        if prefill is None:
            prefill = ns + W - n
        dyn, host, (qc, kc, vc), sa = _twins(dtype, 1, G * Hkv, Hkv, D, ns, W, prefill, appends, n, 31 + seed)
        before, st0 = _state(dyn), _dev_state(dyn)
        out = dyn.extend_attention_dyn(qc, kc, vc, s_aux=sa)
        path = _path()
        assert path.startswith(_expected_path(dtype, D)) and "_dyn" in path and not path.endswith("_commit"), path
        ref = host.extend_attention(qc, kc, vc, s_aux=sa)
        assert torch.equal(out, ref), (name, maxdiff(out, ref))
        _assert_same_state(_state(dyn), before, f"{name}: extend_attention_dyn modified the cache")
        assert torch.equal(dyn._dev_state, st0), name


@pytest.mark.parametrize("fill", [0, 100, 2000, 4096 + 37])
def test_extend_attention_dyn_gpt_oss_geometry_at_every_fill(fill):
    """B=1, H_q=64 / H_kv=8, D=64, W=4096, n=8, s_aux: the full-cache grid has many surplus splits at a low fill."""
    ns, W, n = 4, 4096, 8
    dyn, host, (qc, kc, vc), sa = _twins(torch.bfloat16, 1, 64, 8, 64, ns, W, ns + fill, 0, n, 41)
    out = dyn.extend_attention_dyn(qc, kc, vc, s_aux=sa)
    assert _path().startswith("decode_multi_mfma_bf16_d64") and "_dyn" in _path(), _path()
    assert torch.equal(out, host.extend_attention(qc, kc, vc, s_aux=sa))


def test_large_batch_caps_the_split_count():
    """B * H_kv * row blocks large enough that the workgroup target caps the split count below the tile bound."""
    dyn, host, (qc, kc, vc), sa = _twins(torch.bfloat16, 16, 32, 8, 128, 4, 2048, 900, 0, 8, 43)
    out = dyn.extend_attention_dyn(qc, kc, vc, s_aux=sa)
    assert torch.equal(out, host.extend_attention(qc, kc, vc, s_aux=sa))


@pytest.mark.parametrize("n", [1, 3, 8])
@pytest.mark.parametrize("dtype,D", [(torch.bfloat16, 64), (torch.float16, 128), (torch.bfloat16, 80),
                                     (torch.float32, 64), (torch.bfloat16, 48)])
def test_extend_step_dyn_matches_extend_step(dtype, D, n):
    for seed, (name, ns, W, prefill, appends) in enumerate(FILLS):
        if prefill is None:
            prefill = ns + W - n
        dyn, host, (qc, kc, vc), sa = _twins(dtype, 2, 8, 2, D, ns, W, prefill, appends, n, 51 + seed)
        out = dyn.extend_step_dyn(qc, kc, vc, s_aux=sa)
        assert "_dyn" in _path() and _path().endswith("_commit"), _path()
        ref = host.extend_step(qc, kc, vc, s_aux=sa)
        assert torch.equal(out, ref), (name, maxdiff(out, ref))
        _assert_same_cache(dyn, host, n, f"{name}: extend_step_dyn != extend_step")


@pytest.mark.parametrize("ns,W,prefill,appends,n", [(4, 16, 9, 0, 5), (4, 16, 20, 13, 5), (2, 3, 6, 1, 8)])
def test_commit_dyn_matches_append(ns, W, prefill, appends, n):
    dtype = torch.bfloat16
    for count, a in ((0, 0), (1, 1), (n - 1, n - 1), (n, n), (-1, 0), (n + 3, n)):
        for idt in (torch.int32, torch.int64):
            dyn, host, (_q, kc, vc), _ = _twins(dtype, 2, 4, 2, 64, ns, W, prefill, appends, n, 61, aux=False)
            cnt = torch.tensor(count, dtype=idt, device=DEV)
            if idt == torch.int64:
                cnt = cnt.reshape(1)
            dyn.commit_dyn(kc, vc, cnt)
            assert _path() == "ring_commit_dyn", _path()
            host.append(kc[:, :, :a], vc[:, :, :a])
            _assert_same_cache(dyn, host, a, f"count {count} ({idt})")


def _accept(match):
    """The acceptance rule in torch ops: the number of leading drafts that match (int64, on the device)."""
    return torch.cumprod(match.to(torch.int32), 0).sum()


def test_speculative_loop_captured_in_a_hip_graph():
    """L=3 layers; one captured step = extend_attention_dyn of every layer -> a = leading matches (torch ops on a device
    tensor the test sets before each replay) -> commit_dyn of every layer.  Every replay is bitwise the eager loop
    (extend_attention + a host-side count + append) on twin layers, across ring fill and wrap; one replay is also
    checked against the fp64 oracle over the layer's whole history."""
    from sink_attention import SinkCacheLayer
    g = torch.Generator().manual_seed(71)
    dt, B, Hq, Hkv, D, ns, W, n, L = torch.bfloat16, 1, 16, 2, 64, 4, 16, 4, 3
    pre = ns + 5
    sa = rand((Hq,), g, torch.float32, 0.8).to(DEV)
    graph_layers = [SinkCacheLayer(ns, W) for _ in range(L)]
    eager_layers = [SinkCacheLayer(ns, W) for _ in range(L)]
    hist_k, hist_v = [], []
    for a, b in zip(graph_layers, eager_layers):
        kp, vp = rand((B, Hkv, pre, D), g, dt), rand((B, Hkv, pre, D), g, dt)
        hist_k.append(kp)
        hist_v.append(vp)
        for c in (a, b):
            c.append(kp.to(DEV), vp.to(DEV))
        a.enable_device_state()
    qs = [torch.zeros(B, Hq, n, D, device=DEV, dtype=dt) for _ in range(L)]
    ks = [torch.zeros(B, Hkv, n, D, device=DEV, dtype=dt) for _ in range(L)]
    vs = [torch.zeros(B, Hkv, n, D, device=DEV, dtype=dt) for _ in range(L)]
    outs = [torch.zeros(B, Hq, n, D, device=DEV, dtype=dt) for _ in range(L)]
    match = torch.zeros(n, dtype=torch.bool, device=DEV)

    def step():
        for i, layer in enumerate(graph_layers):
            layer.extend_attention_dyn(qs[i], ks[i], vs[i], s_aux=sa, out=outs[i])
        acc = _accept(match)
        for i, layer in enumerate(graph_layers):
            layer.commit_dyn(ks[i], vs[i], acc)

    def fill(pattern):
        for i in range(L):
            qs[i].copy_(rand((B, Hq, n, D), g, dt))
            ks[i].copy_(rand((B, Hkv, n, D), g, dt))
            vs[i].copy_(rand((B, Hkv, n, D), g, dt))
        match.copy_(torch.tensor(pattern, dtype=torch.bool))
        a = 0
        while a < n and pattern[a]:            # leading matches, counted on the host for the eager twin
            a += 1
        return a

    def eager(a, check):
        for i, b in enumerate(eager_layers):
            ref = b.extend_attention(qs[i], ks[i], vs[i], s_aux=sa)
            if check:
                assert torch.equal(outs[i], ref), (rnd, i, maxdiff(outs[i], ref))
            b.append(ks[i][:, :, :a], vs[i][:, :, :a])
            hist_k[i] = torch.cat([hist_k[i], ks[i][:, :, :a].cpu()], dim=2)
            hist_v[i] = torch.cat([hist_v[i], vs[i][:, :, :a].cpu()], dim=2)

    rnd = -1
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    a0 = fill([True, True, False, True])
    with torch.cuda.stream(side):           # warm-up outside the graph: builds the per-layer constants, commits a0
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager(a0, check=True)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    patterns = [[True] * n, [False] * n, [True, False, True, True], [True] * n, [True, True, True, False],
                [True] * n, [False, True, True, True], [True] * n, [True, True, False, False], [True] * n,
                [True, False, False, False], [True] * n, [True] * n, [False] * n, [True, True, True, False]]
    oracle_round = 9                          # ring full and wrapped by then
    for rnd, pat in enumerate(patterns):
        a = fill(pat)
        hist_len = hist_k[0].shape[2]
        graph.replay()
        torch.cuda.synchronize()
        if rnd == oracle_round:
            assert graph_layers[0]._dev_state.tolist()[1] == W
            k_all = torch.cat([hist_k[0], ks[0].cpu()], dim=2)
            v_all = torch.cat([hist_v[0], vs[0].cpu()], dim=2)
            for t in range(n):
                keep = torch.tensor(history_keys(hist_len, ns, W, t))
                o64 = O.decode_dense(qs[0][:, :, t:t + 1].cpu(), k_all[:, :, keep], v_all[:, :, keep], sa.cpu())
                assert maxdiff(outs[0][:, :, t:t + 1], o64) < TOL[dt], (t, maxdiff(outs[0][:, :, t:t + 1], o64))
        eager(a, check=True)
        for x, y in zip(graph_layers, eager_layers):
            _assert_same_cache(x, y, a, f"replay {rnd}")
    assert hist_k[0].shape[2] - ns > 2 * W       # the ring filled and wrapped more than once


def test_decode_step_dyn_and_extend_step_dyn_share_one_state_in_a_graph():
    """decode_step_dyn then extend_step_dyn on the same layer (one device state) inside one graph: every replay equals
    decode_step + extend_step on an eager twin, bitwise."""
    from sink_attention import SinkCacheLayer
    g = torch.Generator().manual_seed(81)
    dt, B, Hq, Hkv, D, ns, W, n = torch.float16, 2, 8, 2, 128, 4, 24, 3
    a, b = SinkCacheLayer(ns, W), SinkCacheLayer(ns, W)
    kp, vp = rand((B, Hkv, 10, D), g, dt).to(DEV), rand((B, Hkv, 10, D), g, dt).to(DEV)
    for c in (a, b):
        c.append(kp, vp)
    a.enable_device_state()
    sa = rand((Hq,), g, torch.float32, 0.5).to(DEV)
    q1, k1, v1 = (torch.zeros(B, h, 1, D, device=DEV, dtype=dt) for h in (Hq, Hkv, Hkv))
    qn, kn, vn = (torch.zeros(B, h, n, D, device=DEV, dtype=dt) for h in (Hq, Hkv, Hkv))
    o1, on = torch.zeros(B, Hq, 1, D, device=DEV, dtype=dt), torch.zeros(B, Hq, n, D, device=DEV, dtype=dt)

    def step():
        a.decode_step_dyn(q1, k1, v1, s_aux=sa, out=o1)
        a.extend_step_dyn(qn, kn, vn, s_aux=sa, out=on)

    def fill():
        for t in (q1, k1, v1, qn, kn, vn):
            t.copy_(rand(tuple(t.shape), g, dt))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    fill()
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(o1, b.decode_step(q1, k1, v1, s_aux=sa)) and torch.equal(on, b.extend_step(qn, kn, vn, s_aux=sa))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for rnd in range(10):                     # 4 tokens per replay: fills the ring (24) and wraps
        fill()
        graph.replay()
        torch.cuda.synchronize()
        r1 = b.decode_step(q1, k1, v1, s_aux=sa)
        rn = b.extend_step(qn, kn, vn, s_aux=sa)
        assert torch.equal(o1, r1) and torch.equal(on, rn), rnd
        _assert_same_cache(a, b, 1 + n, f"replay {rnd}")


def test_replays_from_the_same_state_are_bitwise_equal():
    from sink_attention import SinkCacheLayer
    g = torch.Generator().manual_seed(91)
    dt, B, Hq, Hkv, D, ns, W, n = torch.bfloat16, 1, 64, 8, 64, 4, 512, 8
    layer = SinkCacheLayer(ns, W)
    kp = rand((B, Hkv, 700, D), g, dt).to(DEV)
    layer.append(kp, kp.flip(2))
    layer.enable_device_state()
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
