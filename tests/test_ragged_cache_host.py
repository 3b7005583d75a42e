"""CPU-only tests of the per-sequence device state (sfa_decode_ring_step_rows, sfa_decode_ring_multi_rows,
sfa_ring_commit_rows, sfa_ring_fill_varlen and SinkCacheLayer's per-sequence mode): exports, the header, argument checks
that return before any launch, the Python-side refusals, and the fill kernel's placement formula against a replay of
_prefill + append.  No GPU compute: every C call here fails its checks before a launch."""
import os
import subprocess
import tempfile

import pytest
import torch

from sink_attention import SinkAttentionCache, SinkCacheLayer

ROWS = ("sfa_decode_ring_step_rows", "sfa_decode_ring_multi_rows", "sfa_ring_commit_rows", "sfa_ring_fill_varlen")


def test_library_exports_the_rows_entry_points():
    from sink_attention import _native
    lib = _native.lib()
    for name in ROWS:
        assert hasattr(lib, name), name
    assert lib.sfa_abi_version() == 2


def test_header_declares_them_and_compiles_as_c99():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = ('#include "sfa.h"\n'
           'int main(void) {\n'
           '  int (*a)(const sfa_tensor*, const sfa_tensor*, const sfa_tensor*, const sfa_tensor*, const sfa_tensor*,\n'
           '           const sfa_tensor*, const sfa_tensor*, const sfa_tensor*, const float*, int32_t*, void*, size_t,\n'
           '           float, unsigned, void*) = sfa_decode_ring_step_rows;\n'
           '  int (*b)(const sfa_tensor*, const sfa_tensor*, const sfa_tensor*, const sfa_tensor*, const sfa_tensor*,\n'
           '           const sfa_tensor*, const sfa_tensor*, const sfa_tensor*, const float*, int, int32_t*, void*,\n'
           '           size_t, float, unsigned, void*) = sfa_decode_ring_multi_rows;\n'
           '  int (*c)(const sfa_tensor*, const sfa_tensor*, const sfa_tensor*, const sfa_tensor*, const int32_t*,\n'
           '           int32_t*, void*) = sfa_ring_commit_rows;\n'
           '  int (*d)(const sfa_tensor*, const sfa_tensor*, const sfa_tensor*, const sfa_tensor*, const sfa_tensor*,\n'
           '           const sfa_tensor*, const int32_t*, int, int32_t*, void*) = sfa_ring_fill_varlen;\n'
           '  return a == 0 || b == 0 || c == 0 || d == 0;\n'
           '}\n')
    with tempfile.NamedTemporaryFile("w", suffix=".c", delete=False) as f:
        f.write(src)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(root, "include"),
                        "-fsyntax-only", f.name], capture_output=True, text=True)
    os.unlink(f.name)
    assert r.returncode == 0, r.stderr


def _abi_args(B=2, Hq=8, Hkv=2, n=3, D=64, ns=4, W=16, T=40, dtype=torch.bfloat16):
    """Host tensors: the C entry points validate them without touching the device and return before any launch."""
    from sink_attention import _native as N
    mk = lambda *s: torch.zeros(*s, dtype=dtype)
    t = dict(q=mk(B, Hq, n, D), sk=mk(B, Hkv, ns, D), sv=mk(B, Hkv, ns, D), wk=mk(B, Hkv, W, D), wv=mk(B, Hkv, W, D),
             kn=mk(B, Hkv, n, D), vn=mk(B, Hkv, n, D), o=mk(B, Hq, n, D), q1=mk(B, Hq, 1, D), k1=mk(B, Hkv, 1, D),
             o1=mk(B, Hq, 1, D), kp=mk(1, Hkv, T, D), vp=mk(1, Hkv, T, D))
    return N, t, {k: N.desc(v) for k, v in t.items()}


# host int32 buffers standing in for the device state / counts / offsets: never dereferenced, every call below fails
# its checks first
_HOST = torch.zeros(64, dtype=torch.int32)
P = _HOST.data_ptr()


def _step(N, d, state=P, ws=None, ws_bytes=0, **over):
    d = dict(d, **over)
    return N.lib().sfa_decode_ring_step_rows(d["q1"], d["sk"], d["sv"], d["wk"], d["wv"], d["k1"], d["k1"], d["o1"], None,
                                             state, ws, ws_bytes, 0.125, 0, None)


def _multi(N, d, state=P, ws=None, ws_bytes=0, commit=1, **over):
    d = dict(d, **over)
    return N.lib().sfa_decode_ring_multi_rows(d["q"], d["sk"], d["sv"], d["wk"], d["wv"], d["kn"], d["vn"], d["o"], None,
                                              commit, state, ws, ws_bytes, 0.125, 0, None)


def _commit(N, d, count=P, state=P, **over):
    d = dict(d, **over)
    return N.lib().sfa_ring_commit_rows(d["wk"], d["wv"], d["kn"], d["vn"], count, state, None)


def _fill(N, d, cu=P, n_seq=2, state=P, **over):
    d = dict(d, **over)
    return N.lib().sfa_ring_fill_varlen(d["sk"], d["sv"], d["wk"], d["wv"], d["kp"], d["vp"], cu, n_seq, state, None)


def test_step_rows_rejects_bad_arguments_before_any_launch():
    N, _, d = _abi_args()
    lib = N.lib()
    assert _step(N, d, state=None) == -1 and b"state" in lib.sfa_last_error()
    _, _, d2 = _abi_args(B=3)
    assert _step(N, d, q1=d2["q1"], o1=d2["o1"]) == -1                                      # q batch != the buffers'
    _, _, d3 = _abi_args(dtype=torch.float16)
    assert _step(N, d, k1=d3["k1"]) == -1 and b"dtype" in lib.sfa_last_error()
    assert _step(N, d, k1=d["kn"]) == -1 and b"k_new" in lib.sfa_last_error()                # k_new with n = 3 rows
    assert _step(N, d) == -3 and b"workspace" in lib.sfa_last_error()                        # all valid but the workspace


def test_multi_rows_rejects_bad_arguments_before_any_launch():
    N, _, d = _abi_args()
    lib = N.lib()
    assert _multi(N, d, state=None) == -1 and b"state" in lib.sfa_last_error()
    _, _, d2 = _abi_args(n=4)
    assert _multi(N, d, kn=d2["kn"], vn=d2["vn"]) == -1 and b"k_new" in lib.sfa_last_error()
    _, _, d3 = _abi_args(B=3)
    assert _multi(N, d, sk=d3["sk"], sv=d3["sv"]) == -1 and b"sink" in lib.sfa_last_error()  # buffers' B != q's
    _, _, d4 = _abi_args(dtype=torch.float32)
    assert _multi(N, d, kn=d4["kn"], vn=d4["vn"]) == -1 and b"dtype" in lib.sfa_last_error()
    _, _, d5 = _abi_args(D=20)                                                                  # 40-byte rows
    assert _multi(N, d5) == -2
    assert _multi(N, d) == -3 and b"workspace" in lib.sfa_last_error()
    need = lib.sfa_decode_multi_workspace_bytes(2, 8, 2, 3, 4 + 16 + 3, 64, 2)
    assert need > 0 and _multi(N, d, ws=1 << 20, ws_bytes=need - 1) == -3


def test_commit_rows_rejects_bad_arguments_before_any_launch():
    N, _, d = _abi_args()
    lib = N.lib()
    assert _commit(N, d, count=None) == -1 and b"count" in lib.sfa_last_error()
    assert _commit(N, d, state=None) == -1 and b"state" in lib.sfa_last_error()
    _, _, d2 = _abi_args(dtype=torch.float16)
    assert _commit(N, d, kn=d2["kn"], vn=d2["vn"]) == -1 and b"dtype" in lib.sfa_last_error()
    _, _, d3 = _abi_args(B=3)
    assert _commit(N, d, kn=d3["kn"], vn=d3["vn"]) == -1 and b"[B, H_kv, n, D]" in lib.sfa_last_error()
    _, _, d4 = _abi_args(D=4)                                                                   # 8-byte rows
    assert _commit(N, d4) == -1 and b"16 bytes" in lib.sfa_last_error()
    assert _commit(N, d, wk=d["kn"]) == -1                                                      # window_k / _v differ


def test_fill_varlen_rejects_bad_arguments_before_any_launch():
    N, _, d = _abi_args()
    lib = N.lib()
    assert _fill(N, d, cu=None) == -1 and b"cu_seqlens" in lib.sfa_last_error()
    assert _fill(N, d, state=None) == -1 and b"state" in lib.sfa_last_error()
    assert _fill(N, d, n_seq=3) == -1 and b"n_seq" in lib.sfa_last_error()                     # n_seq != buffers' B
    assert _fill(N, d, n_seq=0) == -1 and b"n_seq" in lib.sfa_last_error()
    assert _fill(N, d, kp=d["kn"], vp=d["vn"]) == -1 and b"packed" in lib.sfa_last_error()     # batch dim 2
    _, _, d2 = _abi_args(dtype=torch.float16)
    assert _fill(N, d, kp=d2["kp"], vp=d2["vp"]) == -1 and b"dtype" in lib.sfa_last_error()
    _, _, d3 = _abi_args(Hkv=4)
    assert _fill(N, d, kp=d3["kp"], vp=d3["vp"]) == -1 and b"H_kv" in lib.sfa_last_error()
    _, _, d4 = _abi_args(W=0)
    assert _fill(N, d4) == -1 and b"capacity" in lib.sfa_last_error()
    _, _, d5 = _abi_args(D=4)
    assert _fill(N, d5) == -1 and b"16 bytes" in lib.sfa_last_error()
    assert _fill(N, d, vp=d["kn"]) == -1                                                        # k / v differ


# ------------------------------------------------------------------------------------------------ Python surface
def _prefilled_cpu_layer(ns=4, W=16, prefill=30, D=64, B=2):
    layer = SinkCacheLayer(ns, W)
    kv = torch.zeros(B, 2, prefill, D, dtype=torch.bfloat16)
    layer.append(kv, kv)
    return layer


def test_per_sequence_state_starts_from_the_host_counters():
    layer = _prefilled_cpu_layer(prefill=9, B=3)
    st = layer.enable_device_state(per_sequence=True)
    assert st.dtype == torch.int32 and st.tolist() == [[4, 5, 5, 9]] * 3
    assert layer.enable_device_state(per_sequence=True) is st
    assert layer.positions().tolist() == [9, 9, 9]
    with pytest.raises(RuntimeError, match="per-sequence"):
        layer.enable_device_state()
    layer.pull_state()
    assert layer.seen_tokens == [9, 9, 9] and layer.write_pos == [5, 5, 5]


def test_shared_mode_is_unchanged_and_has_no_positions():
    layer = _prefilled_cpu_layer(prefill=9)
    st = layer.enable_device_state()
    assert st.tolist() == [4, 5, 5]
    with pytest.raises(RuntimeError, match="per-sequence"):
        layer.positions()
    assert layer.get_seq_length() == 9


def test_per_sequence_layer_refuses_the_host_state_methods():
    _, t, _ = _abi_args()
    layer = _prefilled_cpu_layer()
    layer.enable_device_state(per_sequence=True)
    calls = {
        "append": lambda: layer.append(t["kn"], t["vn"]),
        "update": lambda: layer.update(t["kn"], t["vn"]),
        "get_kv": lambda: layer.get_kv(),
        "decode_attention": lambda: layer.decode_attention(t["q1"]),
        "decode_step": lambda: layer.decode_step(t["q1"], t["k1"], t["k1"]),
        "extend_attention": lambda: layer.extend_attention(t["q"], t["kn"], t["vn"]),
        "extend_step": lambda: layer.extend_step(t["q"], t["kn"], t["vn"]),
        "get_seq_length": lambda: layer.get_seq_length(),
    }
    for name, call in calls.items():
        with pytest.raises(RuntimeError, match=f"{name}.*per-sequence mode"):
            call()
    assert layer.seen_tokens == 30 and layer.window_len == 16


def test_per_sequence_python_methods_refuse_cpu_tensors():
    _, t, _ = _abi_args()
    layer = _prefilled_cpu_layer()
    state = layer.enable_device_state(per_sequence=True)
    before = state.clone()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        layer.decode_step_dyn(t["q1"], t["k1"], t["k1"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        layer.extend_attention_dyn(t["q"], t["kn"], t["vn"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        layer.extend_step_dyn(t["q"], t["kn"], t["vn"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        layer.commit_dyn(t["kn"], t["vn"], torch.tensor([1, 2], dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SinkCacheLayer(4, 16).prefill_varlen(t["kp"], t["vp"], [0, 10, 40])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SinkAttentionCache(4, 16).prefill_varlen(t["kp"], t["vp"], [0, 10, 40], layer_idx=0)
    assert torch.equal(state, before)


def test_commit_dyn_in_per_sequence_mode_wants_b_counts():
    _, t, _ = _abi_args()
    layer = _prefilled_cpu_layer(B=2)
    layer.enable_device_state(per_sequence=True)
    with pytest.raises(ValueError, match="B = 2 values"):
        layer.commit_dyn(t["kn"], t["vn"], torch.tensor(1, dtype=torch.int32))
    with pytest.raises(ValueError, match="B = 2 values"):
        layer.commit_dyn(t["kn"], t["vn"], torch.tensor([1, 2, 3], dtype=torch.int32))
    with pytest.raises(TypeError, match="integer"):
        layer.commit_dyn(t["kn"], t["vn"], torch.tensor([1.0, 2.0]))
    # the shared mode keeps refusing a multi-element count
    shared = _prefilled_cpu_layer(B=2)
    shared.enable_device_state()
    with pytest.raises(ValueError, match="one value"):
        shared.commit_dyn(t["kn"], t["vn"], torch.tensor([1, 2], dtype=torch.int32))


# ------------------------------------------------------------------------------------ the fill kernel's placement
def fill_formula(L, ns, Wc):
    """The placement sfa_ring_fill_varlen documents (include/sfa.h) for a sequence of L tokens: (sink rows -> token,
    ring slots -> token, state row)."""
    sl = min(L, ns)
    r = L - sl
    sink = {j: j for j in range(sl)}
    ring = {s: sl + s for s in range(r)} if r <= Wc else {s: L - Wc + s for s in range(Wc)}
    return sink, ring, [sl, min(r, Wc), r if r < Wc else 0, L]


def _replay(L, ns, Wc, split):
    """_prefill of the first `split` tokens (append() of a fresh layer) then one append() per further token; D = 1 rows
    that carry their token index (+1, so that an unwritten zero row is told apart)."""
    ids = torch.arange(1, L + 1, dtype=torch.float32).view(1, 1, -1, 1)
    layer = SinkCacheLayer(ns, Wc)
    if split > 0:
        layer.append(ids[:, :, :split], ids[:, :, :split])
        for i in range(split, L):
            layer.append(ids[:, :, i:i + 1], ids[:, :, i:i + 1])
    return layer


@pytest.mark.parametrize("ns", [0, 2, 4])
@pytest.mark.parametrize("Wc", [1, 3, 8])
def test_fill_formula_is_the_placement_of_prefill_and_of_appends(ns, Wc):
    for L in range(0, 3 * (ns + Wc) + 2):
        sink, ring, state = fill_formula(L, ns, Wc)
        layer = _replay(L, ns, Wc, L)            # one prefill of the whole sequence
        if L == 0:
            assert state == [0, 0, 0, 0]
            continue
        assert [layer.sink_len, layer.window_len, layer.write_pos, layer.seen_tokens] == state, (L, state)
        sk = layer.sink_k.flatten().tolist()
        wk = layer.window_k.flatten().tolist()
        assert all(sk[j] == (sink[j] + 1 if j in sink else 0) for j in range(ns)), (L, sk, sink)
        assert all(wk[s] == (ring[s] + 1 if s in ring else 0) for s in range(Wc)), (L, wk, ring)
        # the same sequence decoded token by token after a short prefill gives the same keys in every slot it
        # reached, with the same chronology (the kernels need only the key set and write_pos)
        step = _replay(L, ns, Wc, min(L, ns + 1))
        assert step.sink_len == state[0] and step.window_len == state[1] and step.seen_tokens == L
        assert sorted(step.window_k.flatten().tolist()[:state[1]]) == sorted(wk[:state[1]])
