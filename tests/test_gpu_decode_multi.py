"""GPU parity of the multi-token decode over the sink + ring cache (sfa_decode_ring_multi):
SinkCacheLayer.extend_attention / extend_step against (1) a twin cache that runs n successive decode_step calls,
(2) the fp64 oracle on the keys each row may see in the full chronological history, (3) the cache contract (untouched by
extend_attention, bitwise the twin's after extend_step) and (4) the kernel path that ran."""
import copy

import pytest
import torch

from oracle import sink_oracle as O
from test_decode_multi_host import history_keys
from util import DECODE_TOL, maxdiff, rand
from util import chunk_oracle_rows as _oracle_rows

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = DECODE_TOL


def _path():
    from sink_attention import _native
    return _native.last_path()


def _expected_path(dtype, D):
    if dtype != torch.float32 and D in (64, 80, 96, 128):
        return "decode_multi_mfma_" + {torch.bfloat16: "bf16", torch.float16: "f16"}[dtype] + f"_d{D}"
    return "decode_multi_f32_"


def _tokens(B, Hq, Hkv, D, total, dtype, seed, aux):
    g = torch.Generator().manual_seed(seed)
    q = rand((B, Hq, total, D), g, dtype)
    k, v = rand((B, Hkv, total, D), g, dtype), rand((B, Hkv, total, D), g, dtype)
    sa = rand((Hq,), g, torch.float32, 0.8) if aux else None
    return q, k, v, sa


def _state(layer):
    return (layer.sink_len, layer.window_len, layer.write_pos, layer.seen_tokens,
            [t.clone() for t in (layer.sink_k, layer.sink_v, layer.window_k, layer.window_v)])


def _assert_same_state(a, b, what):
    assert a[:4] == b[:4], (what, a[:4], b[:4])
    for x, y in zip(a[4], b[4]):
        assert torch.equal(x, y), what


def _check_case(dtype, B, Hq, Hkv, D, ns, W, prefill, n, aux, seed=7):
    from sink_attention import SinkCacheLayer
    q, k, v, sa = _tokens(B, Hq, Hkv, D, prefill + n, dtype, seed, aux)
    sad = sa.to(DEV) if sa is not None else None
    layer, twin = SinkCacheLayer(ns, W), SinkCacheLayer(ns, W)
    for c in (layer, twin):
        c.append(k[:, :, :prefill].to(DEV), v[:, :, :prefill].to(DEV))
    qc, kc, vc = (x[:, :, prefill:].to(DEV) for x in (q, k, v))
    before = _state(layer)

    out = layer.extend_attention(qc, kc, vc, s_aux=sad)
    assert _path().startswith(_expected_path(dtype, D)), _path()
    _assert_same_state(_state(layer), before, "extend_attention modified the cache")   # (3a)

    ref = torch.cat([twin.decode_step(qc[:, :, t:t + 1], kc[:, :, t:t + 1], vc[:, :, t:t + 1], s_aux=sad)
                     for t in range(n)], dim=2)
    tol = TOL[dtype]
    assert out.shape == (B, Hq, n, D) and out.dtype == dtype
    assert maxdiff(out, ref) < tol, ("twin", maxdiff(out, ref))                         # (1)
    o64 = _oracle_rows(q, k, v, sa, prefill, ns, W, n, slice(None))
    assert maxdiff(out, o64) < tol, ("oracle", maxdiff(out, o64))                       # (2)

    out2 = layer.extend_step(qc, kc, vc, s_aux=sad)
    assert _path().startswith(_expected_path(dtype, D)) and _path().endswith("_commit"), _path()
    assert torch.equal(out2, out)
    _assert_same_state(_state(layer), _state(twin), "extend_step != n decode_step")   # (3b)


@pytest.mark.parametrize("n", [1, 3, 8])
def test_full_ring_bf16(n):
    _check_case(torch.bfloat16, 2, 8, 2, 128, 4, 64, 100, n, aux=False)


@pytest.mark.parametrize("dtype,B,Hq,Hkv,D,ns,W,prefill,n,aux", [
    (torch.float16, 1, 32, 8, 128, 4, 300, 5, 16, False),     # ring never fills
    (torch.bfloat16, 1, 64, 8, 64, 0, 128, 200, 40, True),    # s_aux, gpt-oss sliding-layer shape, chunk wraps the ring
    (torch.bfloat16, 1, 16, 2, 80, 4, 16, 30, 50, False),     # n > W: 400 rows, several row blocks
    (torch.float16, 1, 8, 2, 128, 4, 32, 2, 12, False),       # sink buffer partly filled
    (torch.bfloat16, 1, 8, 8, 96, 4, 48, 70, 32, False),      # MHA
    (torch.float32, 2, 4, 1, 64, 2, 8, 3, 5, False),          # MQA, f32-accumulate path
    (torch.bfloat16, 1, 8, 2, 40, 4, 16, 20, 6, True),        # head dim without an MFMA kernel: f32-accumulate path
])
def test_cases(dtype, B, Hq, Hkv, D, ns, W, prefill, n, aux):
    _check_case(dtype, B, Hq, Hkv, D, ns, W, prefill, n, aux)


def test_wrapped_ring_mid_chunk():
    """Ring full with write_pos in the middle (the chunk's commit wraps past slot 0)."""
    from sink_attention import SinkCacheLayer
    dtype, B, Hq, Hkv, D, ns, W, n = torch.bfloat16, 1, 64, 8, 64, 4, 128, 40
    q, k, v, sa = _tokens(B, Hq, Hkv, D, 300 + 100 + n, dtype, 3, True)
    layer, twin = SinkCacheLayer(ns, W), SinkCacheLayer(ns, W)
    for c in (layer, twin):
        c.append(k[:, :, :300].to(DEV), v[:, :, :300].to(DEV))
        for i in range(300, 400):
            c.append(k[:, :, i:i + 1].to(DEV), v[:, :, i:i + 1].to(DEV))
    assert layer.write_pos == 100 and layer.window_len == W
    qc, kc, vc = (x[:, :, 400:].to(DEV) for x in (q, k, v))
    out = layer.extend_step(qc, kc, vc, s_aux=sa.to(DEV))
    ref = torch.cat([twin.decode_step(qc[:, :, t:t + 1], kc[:, :, t:t + 1], vc[:, :, t:t + 1], s_aux=sa.to(DEV))
                     for t in range(n)], dim=2)
    assert maxdiff(out, ref) < TOL[dtype]
    assert maxdiff(out, _oracle_rows(q, k, v, sa, 400, ns, W, n, slice(None))) < TOL[dtype]
    _assert_same_state(_state(layer), _state(twin), "wrapped commit")


def test_speculative_loop():
    """Six rounds of 5 drafts: verify all with extend_attention, accept a seeded prefix of 0..5 and append only those.
    The accepted rows match a twin that only ever sees the accepted tokens through decode_step."""
    from sink_attention import SinkCacheLayer
    dtype, B, Hq, Hkv, D, ns, W = torch.bfloat16, 1, 16, 2, 128, 4, 24
    q, k, v, sa = _tokens(B, Hq, Hkv, D, 40 + 30, dtype, 11, True)
    sad = sa.to(DEV)
    layer, twin = SinkCacheLayer(ns, W), SinkCacheLayer(ns, W)
    for c in (layer, twin):
        c.append(k[:, :, :40].to(DEV), v[:, :, :40].to(DEV))
    rng = torch.Generator().manual_seed(5)
    for rnd in range(6):
        sl = slice(40 + 5 * rnd, 45 + 5 * rnd)
        qd, kd, vd = q[:, :, sl].to(DEV), k[:, :, sl].to(DEV), v[:, :, sl].to(DEV)
        out = layer.extend_attention(qd, kd, vd, s_aux=sad)
        a = int(torch.randint(0, 6, (1,), generator=rng))
        layer.append(kd[:, :, :a], vd[:, :, :a])
        for i in range(a):
            ref = twin.decode_step(qd[:, :, i:i + 1], kd[:, :, i:i + 1], vd[:, :, i:i + 1], s_aux=sad)
            assert maxdiff(out[:, :, i:i + 1], ref) < TOL[dtype], (rnd, i)
        _assert_same_state(_state(layer), _state(twin), f"round {rnd}")


def test_large_wrapped_ring_with_s_aux():
    """B=4, H_q=64 / H_kv=8, D=64, num_sink=4, W=4096, ring full and wrapped, n=8, s_aux; batches 0-1 vs the oracle."""
    from sink_attention import SinkCacheLayer
    dtype, B, Hq, Hkv, D, ns, W, n = torch.bfloat16, 4, 64, 8, 64, 4, 4096, 8
    pre = ns + W + 37
    q, k, v, sa = _tokens(B, Hq, Hkv, D, pre + n, dtype, 13, True)
    layer = SinkCacheLayer(ns, W)
    layer.append(k[:, :, :ns + W].to(DEV), v[:, :, :ns + W].to(DEV))
    layer.append(k[:, :, ns + W:pre].to(DEV), v[:, :, ns + W:pre].to(DEV))
    assert layer.write_pos == 37 and layer.window_len == W
    out = layer.extend_attention(q[:, :, pre:].to(DEV), k[:, :, pre:].to(DEV), v[:, :, pre:].to(DEV), s_aux=sa.to(DEV))
    assert _path().startswith("decode_multi_mfma_bf16_d64"), _path()
    ref = _oracle_rows(q, k, v, sa, pre, ns, W, n, slice(0, 2))
    assert maxdiff(out[:2], ref) < TOL[dtype]


def test_transposed_views_give_bitwise_the_contiguous_result():
    from sink_attention import SinkCacheLayer, sink_decode_attention_ring_multi
    dtype, B, Hq, Hkv, D, ns, W, n = torch.bfloat16, 2, 16, 4, 128, 4, 64, 9
    q, k, v, sa = _tokens(B, Hq, Hkv, D, 100 + n, dtype, 17, True)
    layer = SinkCacheLayer(ns, W)
    layer.append(k[:, :, :100].to(DEV), v[:, :, :100].to(DEV))
    qc, kc, vc = (x[:, :, 100:].contiguous().to(DEV) for x in (q, k, v))
    qt, kt, vt = (x.transpose(1, 2).contiguous().transpose(1, 2) for x in (qc, kc, vc))   # [B, n, H, D] storage
    assert not qt.is_contiguous()
    args = (layer.sink_k, layer.sink_v, layer.sink_len, layer.window_k, layer.window_v, layer.window_len, layer.write_pos)
    a = sink_decode_attention_ring_multi(qc, *args[:7], kc, vc, s_aux=sa.to(DEV))
    b = sink_decode_attention_ring_multi(qt, *args[:7], kt, vt, s_aux=sa.to(DEV))
    assert torch.equal(a, b)
    assert torch.equal(layer.extend_attention(qt, kt, vt, s_aux=sa.to(DEV)), a)


def test_deterministic():
    from sink_attention import SinkCacheLayer
    dtype, B, Hq, Hkv, D, ns, W, n = torch.bfloat16, 1, 64, 8, 64, 4, 512, 16
    q, k, v, sa = _tokens(B, Hq, Hkv, D, 700 + n, dtype, 19, True)
    layer = SinkCacheLayer(ns, W)
    layer.append(k[:, :, :700].to(DEV), v[:, :, :700].to(DEV))
    args = [x[:, :, 700:].to(DEV) for x in (q, k, v)]
    a = layer.extend_attention(*args, s_aux=sa.to(DEV))
    b = layer.extend_attention(*args, s_aux=sa.to(DEV))
    assert torch.equal(a, b)


def test_c_abi_errors_launch_nothing():
    from sink_attention import SinkCacheLayer, _native as N
    dtype, B, Hq, Hkv, D, ns, W, n = torch.bfloat16, 1, 8, 2, 64, 4, 16, 3
    q, k, v, _ = _tokens(B, Hq, Hkv, D, 30 + n, dtype, 23, False)
    layer = SinkCacheLayer(ns, W)
    layer.append(k[:, :, :30].to(DEV), v[:, :, :30].to(DEV))
    before = _state(layer)
    qd, kd, vd = (x[:, :, 30:].contiguous().to(DEV) for x in (q, k, v))
    out = torch.full((B, Hq, n, D), 7.0, dtype=dtype, device=DEV)
    lib = N.lib()
    need = lib.sfa_decode_multi_workspace_bytes(B, Hq, Hkv, n, layer.sink_len + layer.window_len + n, D, 2)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    d = [N.desc(t) for t in (qd, layer.sink_k, layer.sink_v, layer.window_k, layer.window_v, kd, vd, out)]

    def call(wl, wp, ws_ptr, ws_bytes, kn=d[5], commit=1):
        return lib.sfa_decode_ring_multi(d[0], d[1], d[2], layer.sink_len, d[3], d[4], wl, wp, kn, d[6], d[7], None,
                                         commit, ws_ptr, ws_bytes, 0.125, 0, N.stream_ptr(qd.device))

    assert call(10, 3, ws.data_ptr(), need) == -1                       # ring not full, write_pos != window_len
    assert call(16, 16, ws.data_ptr(), need) == -1                      # write_pos outside the ring
    assert call(16, 0, ws.data_ptr(), need, kn=N.desc(kd[:, :, :2])) == -1   # k_new rows != n
    assert call(16, 0, ws.data_ptr(), need - 256) == -3                 # workspace too small
    assert call(16, 0, ws.data_ptr() + 16, need) == -3                  # misaligned workspace
    assert call(16, 0, None, 0) == -3
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    _assert_same_state(_state(layer), before, "a refused call changed the cache")
