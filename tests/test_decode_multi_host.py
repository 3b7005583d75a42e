"""CPU-only tests of the multi-token decode (sfa_decode_ring_multi, SinkCacheLayer.extend_attention / extend_step):
exports, workspace query, argument checks that return before any launch, and the key-visibility contract itself
(checked against a brute-force replay of append() on host tensors).  No GPU compute."""
import copy
import itertools

import pytest
import torch

from sink_attention import SinkAttentionCache, SinkCacheLayer, sink_decode_attention_ring_multi


def visible_keys(sink_len, window_len, write_pos, Wc, n, t):
    """Keys query t (0 <= t < n) of a chunk of n new tokens may attend to, given the cache state BEFORE the chunk:
    (sink rows, ring slots, chunk tokens).  The contract of include/sfa.h (sfa_decode_ring_multi)."""
    sinks = list(range(sink_len))
    slots = []
    for s in range(window_len):
        r = (s - write_pos + window_len) % Wc          # chronological index, 0 = oldest
        if window_len - r + t <= Wc - 1:
            slots.append(s)
    chunk = [u for u in range(n) if u <= t and t - u <= Wc - 1]
    return sinks, slots, chunk


def history_keys(prefill, num_sink, Wc, t):
    """The same set in absolute token positions of the whole history (prefill tokens 0 .. prefill - 1, then the chunk):
    the sink rows hold the first min(prefill, num_sink) tokens, every later token is a window token."""
    sl = min(prefill, num_sink)
    pos = prefill + t
    return sorted(set(range(sl)) | set(range(max(sl, pos - Wc + 1), pos + 1)))


def _ids_layer(num_sink, W, prefill, n):
    """A host cache whose K rows carry their token's absolute position (D = 1)."""
    ids = torch.arange(prefill + n, dtype=torch.float32).view(1, 1, -1, 1)
    layer = SinkCacheLayer(num_sink, W)
    layer.append(ids[:, :, :prefill], ids[:, :, :prefill])
    return layer, ids


STATES = [(ns, W, p, n) for ns, W in itertools.product((0, 2, 4), (1, 3, 8))
          for p, n in ((1, 1), (2, 5), (3, 17), (5, 2), (9, 8), (12, 3), (20, 9), (20, 17))]


@pytest.mark.parametrize("ns,W,prefill,n", STATES)
def test_visibility_helper_matches_a_replay_of_append(ns, W, prefill, n):
    layer, ids = _ids_layer(ns, W, prefill, n)
    sl, wl, wp = layer.sink_len, layer.window_len, layer.write_pos
    sink_ids = layer.sink_k[0, 0, :, 0].tolist()
    ring_ids = layer.window_k[0, 0, :, 0].tolist()
    for t in range(n):
        twin = copy.deepcopy(layer)
        twin.append(ids[:, :, prefill:prefill + t + 1], ids[:, :, prefill:prefill + t + 1])
        kk, _ = twin.get_kv()            # what a single-query decode at step t attends to
        replay = sorted(int(x) for x in kk[0, 0, :, 0].tolist())
        sinks, slots, chunk = visible_keys(sl, wl, wp, W, n, t)
        mine = sorted([int(sink_ids[j]) for j in sinks] + [int(ring_ids[s]) for s in slots] + [prefill + u for u in chunk])
        assert mine == replay, (t, mine, replay)
        assert history_keys(prefill, ns, W, t) == replay, t


@pytest.mark.parametrize("ns,W,prefill,n", STATES[::3])
def test_commit_placement_matches_append(ns, W, prefill, n):
    """extend_step's commit contract: token t >= n - Wc lands in slot (write_pos + t) mod Wc, the counters advance as
    n appends advance them."""
    layer, ids = _ids_layer(ns, W, prefill, n)
    wl, wp, seen = layer.window_len, layer.write_pos, layer.seen_tokens
    ring = layer.window_k[0, 0, :, 0].clone()
    for t in range(max(0, n - W), n):
        ring[(wp + t) % W] = prefill + t
    layer.append(ids[:, :, prefill:], ids[:, :, prefill:])
    assert torch.equal(layer.window_k[0, 0, :, 0], ring)
    assert layer.write_pos == (wp + n) % W and layer.window_len == min(wl + n, W) and layer.seen_tokens == seen + n


def test_library_exports_the_multi_decode():
    from sink_attention import _native
    lib = _native.lib()
    assert hasattr(lib, "sfa_decode_ring_multi") and hasattr(lib, "sfa_decode_multi_workspace_bytes")
    assert lib.sfa_abi_version() == 2


@pytest.mark.parametrize("B,Hq,Hkv,n,D,dt", [(1, 64, 8, 8, 64, 2), (32, 32, 32, 4, 128, 2), (2, 4, 1, 5, 64, 0),
                                             (1, 16, 2, 50, 80, 2), (4, 8, 2, 1, 40, 1)])
def test_multi_workspace_needs_no_gpu_and_is_monotonic(B, Hq, Hkv, n, D, dt):
    from sink_attention import _native
    lib = _native.lib()
    cap = 4 + 4096 + n
    full = lib.sfa_decode_multi_workspace_bytes(B, Hq, Hkv, n, cap, D, dt)
    assert full >= B * Hq * n * (D + 2) * 4          # at least one partial per row
    prev = 0
    for nkv in list(range(n, 700)) + list(range(700, cap + 1, 53)) + [cap]:
        ws = lib.sfa_decode_multi_workspace_bytes(B, Hq, Hkv, n, nkv, D, dt)
        assert 0 < ws <= full and ws >= prev, (nkv, ws, prev, full)
        prev = ws


def test_multi_workspace_rejects_unsupported_head_dims():
    from sink_attention import _native
    lib = _native.lib()
    assert lib.sfa_decode_multi_workspace_bytes(1, 4, 4, 3, 100, 20, 2) == 0      # 40-byte rows
    assert lib.sfa_decode_multi_workspace_bytes(1, 4, 4, 3, 100, 512, 0) == 0     # 2 KiB rows
    assert lib.sfa_decode_multi_workspace_bytes(1, 6, 4, 3, 100, 64, 2) == 0      # H_q % H_kv != 0


def _abi_args(B=1, Hq=8, Hkv=2, n=3, D=64, ns=4, W=16):
    """Host tensors: the C entry point validates them without touching the device and returns before any launch."""
    from sink_attention import _native as N
    mk = lambda *s: torch.zeros(*s, dtype=torch.bfloat16)
    t = dict(q=mk(B, Hq, n, D), sk=mk(B, Hkv, ns, D), sv=mk(B, Hkv, ns, D), wk=mk(B, Hkv, W, D), wv=mk(B, Hkv, W, D),
             kn=mk(B, Hkv, n, D), vn=mk(B, Hkv, n, D), o=mk(B, Hq, n, D))
    return N, t, {k: N.desc(v) for k, v in t.items()}


def _call(N, d, sink_len, wl, wp, ws=None, ws_bytes=0, **over):
    d = dict(d, **over)
    return N.lib().sfa_decode_ring_multi(d["q"], d["sk"], d["sv"], sink_len, d["wk"], d["wv"], wl, wp, d["kn"], d["vn"],
                                         d["o"], None, 0, ws, ws_bytes, 0.125, 0, None)


def test_c_abi_rejects_bad_arguments_before_any_launch():
    N, t, d = _abi_args()
    lib = N.lib()
    assert _call(N, d, 4, 10, 3) == -1 and b"write_pos" in lib.sfa_last_error()     # ring not full: write_pos != window_len
    assert _call(N, d, 4, 16, 16) == -1                                             # write_pos outside the ring
    assert _call(N, d, 5, 16, 3) == -1                                              # sink_len > num_sink
    assert _call(N, d, 4, 17, 3) == -1                                              # window_len > capacity
    _, _, d2 = _abi_args(n=4)
    assert _call(N, d, 4, 16, 3, kn=d2["kn"], vn=d2["vn"]) == -1 and b"k_new" in lib.sfa_last_error()   # k_new rows != n
    _, _, d3 = _abi_args(Hq=6, Hkv=4)
    assert _call(N, d3, 4, 16, 3) == -1 and b"divisible" in lib.sfa_last_error()
    # every argument valid, no workspace: SFA_ERR_WORKSPACE (the check that comes last before the launch)
    assert _call(N, d, 4, 16, 3) == -3 and b"workspace" in lib.sfa_last_error()
    assert _call(N, d, 4, 10, 10) == -3
    assert _call(N, d, 4, 0, 0) == -3


def test_python_entry_points_refuse_cpu_tensors():
    _, t, _ = _abi_args()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sink_decode_attention_ring_multi(t["q"], t["sk"], t["sv"], 4, t["wk"], t["wv"], 16, 3, t["kn"], t["vn"])
    layer = SinkCacheLayer(4, 16)
    layer.append(torch.zeros(1, 2, 30, 64, dtype=torch.bfloat16), torch.zeros(1, 2, 30, 64, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        layer.extend_attention(t["q"], t["kn"], t["vn"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        layer.extend_step(t["q"], t["kn"], t["vn"])
    assert layer.window_len == 16 and layer.seen_tokens == 30     # nothing was committed


def test_python_entry_points_refuse_an_unprefilled_cache():
    _, t, _ = _abi_args()
    with pytest.raises(ValueError, match="prefilled"):
        SinkCacheLayer(4, 16).extend_attention(t["q"], t["kn"], t["vn"])
    cache = SinkAttentionCache(num_sink=4, window_size=16)
    with pytest.raises(ValueError, match="prefilled"):
        cache.extend_step(t["q"], t["kn"], t["vn"], layer_idx=0)
    with pytest.raises(ValueError, match="prefilled"):
        cache.extend_attention(t["q"], t["kn"], t["vn"], layer_idx=2)
    assert cache.seen_tokens == 0
