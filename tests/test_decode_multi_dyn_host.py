"""CPU-only tests of the device-state multi-token decode (sfa_decode_ring_multi_dyn, sfa_ring_commit_dyn and the
SinkCacheLayer / SinkAttentionCache *_dyn methods): exports, the header, argument checks that return before any launch
and the Python-side refusals.  No GPU compute: every C call here fails its checks before a launch."""
import os
import subprocess
import tempfile

import pytest
import torch

from sink_attention import SinkAttentionCache, SinkCacheLayer


def test_library_exports_the_dyn_entry_points():
    from sink_attention import _native
    lib = _native.lib()
    assert hasattr(lib, "sfa_decode_ring_multi_dyn") and hasattr(lib, "sfa_ring_commit_dyn")
    assert lib.sfa_abi_version() == 2


def test_header_declares_them_and_compiles_as_c99():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = ('#include "sfa.h"\n'
           'int main(void) {\n'
           '  int (*a)(const sfa_tensor*, const sfa_tensor*, const sfa_tensor*, const sfa_tensor*, const sfa_tensor*,\n'
           '           const sfa_tensor*, const sfa_tensor*, const sfa_tensor*, const float*, int, int32_t*, void*,\n'
           '           size_t, float, unsigned, void*) = sfa_decode_ring_multi_dyn;\n'
           '  int (*b)(const sfa_tensor*, const sfa_tensor*, const sfa_tensor*, const sfa_tensor*, const int32_t*,\n'
           '           int32_t*, void*) = sfa_ring_commit_dyn;\n'
           '  return a == 0 || b == 0;\n'
           '}\n')
    with tempfile.NamedTemporaryFile("w", suffix=".c", delete=False) as f:
        f.write(src)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(root, "include"),
                        "-fsyntax-only", f.name], capture_output=True, text=True)
    os.unlink(f.name)
    assert r.returncode == 0, r.stderr


def _abi_args(B=1, Hq=8, Hkv=2, n=3, D=64, ns=4, W=16, dtype=torch.bfloat16):
    """Host tensors: the C entry points validate them without touching the device and return before any launch."""
    from sink_attention import _native as N
    mk = lambda *s: torch.zeros(*s, dtype=dtype)
    t = dict(q=mk(B, Hq, n, D), sk=mk(B, Hkv, ns, D), sv=mk(B, Hkv, ns, D), wk=mk(B, Hkv, W, D), wv=mk(B, Hkv, W, D),
             kn=mk(B, Hkv, n, D), vn=mk(B, Hkv, n, D), o=mk(B, Hq, n, D))
    return N, t, {k: N.desc(v) for k, v in t.items()}


# a host int32 buffer standing in for the device state / count: never dereferenced, every call below fails its checks
_HOST_STATE = torch.zeros(4, dtype=torch.int32)


def _multi(N, d, state=_HOST_STATE.data_ptr(), ws=None, ws_bytes=0, commit=1, **over):
    d = dict(d, **over)
    return N.lib().sfa_decode_ring_multi_dyn(d["q"], d["sk"], d["sv"], d["wk"], d["wv"], d["kn"], d["vn"], d["o"], None,
                                             commit, state, ws, ws_bytes, 0.125, 0, None)


def test_multi_dyn_rejects_bad_arguments_before_any_launch():
    N, t, d = _abi_args()
    lib = N.lib()
    assert _multi(N, d, state=None) == -1 and b"state" in lib.sfa_last_error()
    _, _, d2 = _abi_args(n=4)
    assert _multi(N, d, kn=d2["kn"], vn=d2["vn"]) == -1 and b"k_new" in lib.sfa_last_error()     # k_new rows != n
    _, _, d3 = _abi_args(Hq=6, Hkv=4)
    assert _multi(N, d3) == -1 and b"divisible" in lib.sfa_last_error()
    _, _, d4 = _abi_args(dtype=torch.float16)
    assert _multi(N, d, kn=d4["kn"], vn=d4["vn"]) == -1 and b"dtype" in lib.sfa_last_error()
    _, _, d5 = _abi_args(Hkv=4, Hq=8)
    assert _multi(N, d, wk=d5["wk"], wv=d5["wv"]) == -1 and b"window" in lib.sfa_last_error()   # ring H_kv != k_new's
    _, _, d6 = _abi_args(D=20)                                                                     # 40-byte rows
    assert _multi(N, d6) == -2
    # every argument valid: the workspace check comes last, and it is sized for the FULL cache plus the chunk
    assert _multi(N, d) == -3 and b"workspace" in lib.sfa_last_error()
    need = lib.sfa_decode_multi_workspace_bytes(1, 8, 2, 3, 4 + 16 + 3, 64, 2)
    partial = lib.sfa_decode_multi_workspace_bytes(1, 8, 2, 3, 3, 64, 2)
    assert need > 0
    fake_ws = 1 << 20          # 256-byte aligned, never dereferenced (the size check fails first)
    assert _multi(N, d, ws=fake_ws, ws_bytes=need - 1) == -3
    if partial < need:
        assert _multi(N, d, ws=fake_ws, ws_bytes=partial) == -3


def _commit(N, d, count=_HOST_STATE.data_ptr(), state=_HOST_STATE.data_ptr(), **over):
    d = dict(d, **over)
    return N.lib().sfa_ring_commit_dyn(d["wk"], d["wv"], d["kn"], d["vn"], count, state, None)


def test_commit_dyn_rejects_bad_arguments_before_any_launch():
    N, t, d = _abi_args()
    lib = N.lib()
    assert _commit(N, d, count=None) == -1 and b"count" in lib.sfa_last_error()
    assert _commit(N, d, state=None) == -1 and b"state" in lib.sfa_last_error()
    _, _, d2 = _abi_args(dtype=torch.float16)
    assert _commit(N, d, kn=d2["kn"], vn=d2["vn"]) == -1 and b"dtype" in lib.sfa_last_error()
    _, _, d3 = _abi_args(Hkv=4, Hq=8)
    assert _commit(N, d, kn=d3["kn"], vn=d3["vn"]) == -1 and b"[B, H_kv, n, D]" in lib.sfa_last_error()
    _, _, d4 = _abi_args(D=4)                                                                     # 8-byte rows
    assert _commit(N, d4) == -1 and b"16 bytes" in lib.sfa_last_error()
    _, _, d5 = _abi_args(n=2)
    assert _commit(N, d, kn=d5["kn"], vn=d["vn"]) == -1                                          # k_new / v_new differ
    assert _commit(N, d, wk=d["kn"]) == -1                                                        # window_k / window_v differ


def _prefilled_cpu_layer(ns=4, W=16, prefill=30, D=64):
    layer = SinkCacheLayer(ns, W)
    kv = torch.zeros(1, 2, prefill, D, dtype=torch.bfloat16)
    layer.append(kv, kv)
    return layer


def test_python_methods_need_enable_device_state():
    _, t, _ = _abi_args()
    layer = _prefilled_cpu_layer()
    count = torch.tensor(1, dtype=torch.int32)
    for call in (lambda: layer.extend_attention_dyn(t["q"], t["kn"], t["vn"]),
                 lambda: layer.extend_step_dyn(t["q"], t["kn"], t["vn"]),
                 lambda: layer.commit_dyn(t["kn"], t["vn"], count)):
        with pytest.raises(RuntimeError, match="enable_device_state"):
            call()


def test_python_methods_refuse_cpu_tensors():
    _, t, _ = _abi_args()
    layer = _prefilled_cpu_layer()
    state = layer.enable_device_state()
    before = state.clone()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        layer.extend_attention_dyn(t["q"], t["kn"], t["vn"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        layer.extend_step_dyn(t["q"], t["kn"], t["vn"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        layer.commit_dyn(t["kn"], t["vn"], torch.tensor(2, dtype=torch.int32))
    assert torch.equal(state, before) and layer.window_len == 16 and layer.seen_tokens == 30


def test_commit_dyn_refuses_a_float_or_multi_element_count():
    _, t, _ = _abi_args()
    layer = _prefilled_cpu_layer()
    layer.enable_device_state()
    with pytest.raises(TypeError, match="integer"):
        layer.commit_dyn(t["kn"], t["vn"], torch.tensor(2.0))
    with pytest.raises(TypeError, match="integer"):
        layer.commit_dyn(t["kn"], t["vn"], torch.tensor(True))
    with pytest.raises(TypeError, match="integer"):
        layer.commit_dyn(t["kn"], t["vn"], 2)
    with pytest.raises(ValueError, match="one value"):
        layer.commit_dyn(t["kn"], t["vn"], torch.tensor([1, 2], dtype=torch.int32))
    with pytest.raises(ValueError, match="one value"):
        layer.commit_dyn(t["kn"], t["vn"], torch.zeros(0, dtype=torch.int64))


def test_python_methods_refuse_an_unprefilled_cache():
    _, t, _ = _abi_args()
    count = torch.tensor(1, dtype=torch.int32)
    layer = SinkCacheLayer(4, 16)
    with pytest.raises(ValueError, match="prefilled"):
        layer.extend_attention_dyn(t["q"], t["kn"], t["vn"])
    with pytest.raises(ValueError, match="prefilled"):
        layer.commit_dyn(t["kn"], t["vn"], count)
    cache = SinkAttentionCache(num_sink=4, window_size=16)
    with pytest.raises(ValueError, match="prefilled"):
        cache.extend_step_dyn(t["q"], t["kn"], t["vn"], layer_idx=0)
    with pytest.raises(ValueError, match="prefilled"):
        cache.extend_attention_dyn(t["q"], t["kn"], t["vn"], layer_idx=1)
    with pytest.raises(ValueError, match="prefilled"):
        cache.commit_dyn(t["kn"], t["vn"], count, layer_idx=2)
    assert cache.seen_tokens == 0
