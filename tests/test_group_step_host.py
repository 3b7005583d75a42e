"""CPU-only tests of the fork-group calls: the three symbols in the library and the header, a workspace size of 0 on the
shapes no grouped instance serves, every refusal of the two entry points (status and exact sfa_last_error() text; host
tensors stand in for device memory - every call returns before a launch) in the order of their paged siblings, and the
Python refusals of ragged_step_dyn(groups=)."""
import ctypes
import os
import subprocess
import tempfile

import pytest
import torch

from sink_attention import SinkAttentionCache, SinkCacheLayer, group_offsets
from sink_attention import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HQ, HKV, D, NS, S, T = 8, 2, 64, 4, 5, 6
P, PER, NP = 32, 3, 7
_KEEP = []
PTR = ctypes.c_void_p(0x1000)      # stands in for a device array: never read
FP8 = torch.float8_e4m3fn


def _d(*shape, dtype=torch.bfloat16):
    t = torch.zeros(*shape, dtype=dtype)
    _KEEP.append(t)
    return N.desc(t)


def _args(act=torch.bfloat16, d=D, p=P, kv=None):
    kv = act if kv is None else kv
    return dict(q=_d(1, HQ, T, d, dtype=act), kn=_d(1, HKV, T, d, dtype=act), vn=_d(1, HKV, T, d, dtype=act),
                o=_d(1, HQ, T, d, dtype=act), sk=_d(S, HKV, NS, d, dtype=kv), sv=_d(S, HKV, NS, d, dtype=kv),
                wk=_d(NP, HKV, p, d, dtype=kv), wv=_d(NP, HKV, p, d, dtype=kv))


def _step(a, fp8=False, state=PTR, slots=PTR, cu=PTR, n_seq=2, cu_g=PTR, n_grp=1, table=PTR, stride=PER, flags=0, ws=None,
          ws_bytes=0):
    lib = N.lib()
    fn = lib.sfa_decode_ring_ragged_group_paged_fp8_slots if fp8 else lib.sfa_decode_ring_ragged_group_paged_slots
    tail = (table, stride) + ((None,) if fp8 else ())
    rc = fn(a["q"], a["sk"], a["sv"], a["wk"], a["wv"], a["kn"], a["vn"], a["o"], None, None, 1, state, slots, cu, n_seq,
            cu_g, n_grp, *tail, ws, ws_bytes, 0.125, flags, None)
    return rc, lib.sfa_last_error().decode()


def test_the_symbols_are_exported_and_the_header_compiles_as_c():
    lib = N.lib()
    assert len(lib.sfa_decode_ring_ragged_group_paged_slots.argtypes) == 24
    assert len(lib.sfa_decode_ring_ragged_group_paged_fp8_slots.argtypes) == 25
    assert len(lib.sfa_decode_ragged_group_workspace_bytes.argtypes) == 8
    assert lib.sfa_abi_version() == 2 and N.ABI_VERSION == 2
    TT, I = "const sfa_tensor*", "const int32_t*"
    src = ('#include "sfa.h"\n'
           'int main(void) {\n'
           f'  int (*a)({TT}, {TT}, {TT}, {TT}, {TT}, {TT}, {TT}, {TT}, const float*, {I}, int, int32_t*, {I}, {I}, int,\n'
           f'           {I}, int, {I}, int, void*, size_t, float, unsigned, void*) = sfa_decode_ring_ragged_group_paged_slots;\n'
           f'  int (*b)({TT}, {TT}, {TT}, {TT}, {TT}, {TT}, {TT}, {TT}, const float*, {I}, int, int32_t*, {I}, {I}, int,\n'
           f'           {I}, int, {I}, int, const float*, void*, size_t, float, unsigned, void*) =\n'
           '      sfa_decode_ring_ragged_group_paged_fp8_slots;\n'
           '  size_t (*c)(int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int) =\n'
           '      sfa_decode_ragged_group_workspace_bytes;\n'
           '  return a == 0 || b == 0 || c == 0 || SFA_ABI_VERSION != 2;\n'
           '}\n')
    with tempfile.NamedTemporaryFile("w", suffix=".c", delete=False) as f:
        f.write(src)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                        "-fsyntax-only", f.name], capture_output=True, text=True)
    os.unlink(f.name)
    assert r.returncode == 0, r.stderr


def test_the_workspace_is_zero_where_no_grouped_instance_exists():
    ws = N.lib().sfa_decode_ragged_group_workspace_bytes
    bf, f16, f32 = N.SFA_DTYPE[torch.bfloat16], N.SFA_DTYPE[torch.float16], N.SFA_DTYPE[torch.float32]
    base = N.lib().sfa_decode_ragged_workspace_bytes(2, HQ, HKV, T, NS + P * PER, D, bf)
    assert ws(2, 1, HQ, HKV, T, NS + P * PER, D, bf) > base > 0
    assert ws(2, 1, HQ, HKV, T, NS + P * PER, D, f16) == ws(2, 1, HQ, HKV, T, NS + P * PER, D, bf)
    for d in (64, 80, 96, 128):
        assert ws(2, 1, HQ, HKV, T, NS + P * PER, d, bf) > 0
    assert ws(2, 1, HQ, HKV, T, NS + P * PER, D, f32) == 0                 # no f32 instance
    for d in (32, 48, 72, 256):
        assert ws(2, 1, HQ, HKV, T, NS + P * PER, d, bf) == 0              # other head dims
    assert ws(2, 0, HQ, HKV, T, NS + P * PER, D, bf) == 0 and ws(2, -1, HQ, HKV, T, NS + P * PER, D, bf) == 0
    assert ws(0, 1, HQ, HKV, T, NS + P * PER, D, bf) == 0 and ws(2, 1, HQ, 3, T, NS + P * PER, D, bf) == 0
    assert ws(2, 3, HQ, HKV, T, NS + P * PER, D, bf) >= ws(2, 1, HQ, HKV, T, NS + P * PER, D, bf)


@pytest.mark.parametrize("fp8", [False, True])
def test_refusals_in_the_order_of_the_paged_sibling(fp8):
    who = "decode_ragged_paged_fp8" if fp8 else "decode_ragged_paged"
    mk = lambda **kw: _args(kv=FP8 if fp8 else None, **kw)
    call = lambda a, **kw: _step(a, fp8=fp8, **kw)
    ok = mk()
    # the checks of the paged pool
    assert call(dict(ok, wk=None)) == (-1, "window_k: null tensor descriptor")
    assert call(ok, table=None) == (-1, "page_table: null device pointer")
    assert call(mk(p=48)) == (-1, f"{who}: the page size (window_k shape[2] = 48) must be a power of two and at least 32")
    assert call(ok, stride=0) == (-1, f"{who}: table_stride (0) must be at least 1 (Wc = table_stride * P)")
    # the null device arrays and n_seq of the sibling, then cu_g and n_grp
    assert call(ok, state=None) == (-1, "state: null device pointer")
    assert call(ok, slots=None) == (-1, "slots: null device pointer")
    assert call(ok, cu=None) == (-1, "cu_q: null device pointer")
    assert call(ok, n_seq=0) == (-1, "decode_ragged: n_seq (0) must be at least 1")
    assert call(ok, cu_g=None) == (-1, "cu_g: null device pointer")
    assert call(ok, n_grp=0) == (-1, "decode_ragged: n_grp (0) must be at least 1")
    assert call(ok, n_grp=-3) == (-1, "decode_ragged: n_grp (-3) must be at least 1")
    assert call(ok, n_seq=0, cu_g=None)[1] == "decode_ragged: n_seq (0) must be at least 1"      # n_seq before cu_g
    assert call(ok, cu_g=None, n_grp=0)[1] == "cu_g: null device pointer"                        # cu_g before n_grp
    # then the sibling's own: what the pool serves, in the text of the existing form
    kind = "a paged FP8 pool serves bf16 / f16 activations" if fp8 else "a paged pool serves bf16 / f16"
    rc, msg = call(mk(d=48))
    assert rc == -2 and msg == f"{who}: {kind} at head dims 64 / 80 / 96 / 128 (got dtype 2, head dim 48)", msg
    rc, msg = call(ok, flags=N.FLAG_FORCE_GENERIC)
    assert rc == -2 and msg == f"{who}: {kind} at head dims 64 / 80 / 96 / 128 (got dtype 2, head dim 64, SFA_FLAG_FORCE_GENERIC)", msg
    if not fp8:
        rc, msg = call(_args(act=torch.float32))
        assert rc == -2 and msg == f"{who}: {kind} at head dims 64 / 80 / 96 / 128 (got dtype 0, head dim 64)", msg
    # a good call stops at the workspace: the size is the grouped one
    need = N.lib().sfa_decode_ragged_group_workspace_bytes(2, 1, HQ, HKV, T, NS + P * PER, D, N.SFA_DTYPE[torch.bfloat16])
    rc, msg = call(ok)
    assert rc == -3 and str(need) in msg, msg
    plain = N.lib().sfa_decode_ragged_workspace_bytes(2, HQ, HKV, T, NS + P * PER, D, N.SFA_DTYPE[torch.bfloat16])
    rc, msg = call(ok, ws=PTR, ws_bytes=plain)               # the ungrouped size is too small
    assert rc == -3 and str(need) in msg, msg


def test_python_refusals():
    k = torch.zeros(1, HKV, 2, D, dtype=torch.bfloat16)
    q = torch.zeros(1, HQ, 2, D, dtype=torch.bfloat16)
    plain = SinkCacheLayer(NS, P * PER)
    plain.init_pool(S, HKV, D, torch.bfloat16, "cpu")
    with pytest.raises(TypeError, match=r"needs a paged pool: init_pool\(\.\.\., page_size=P\)"):
        plain.ragged_step_dyn(q, k, k, [0, 1, 2], [0, 1], groups=[0, 2])
    paged = SinkCacheLayer(NS, P * PER)
    paged.init_pool(S, HKV, D, torch.bfloat16, "cpu", page_size=P)
    with pytest.raises(ValueError, match="takes no parent="):
        paged.ragged_step_dyn(q, k, k, [0, 1, 2], [0, 1], parent=[-1, -1], groups=[0, 2])
    cache = SinkAttentionCache(NS, P * PER)
    cache.init_pool(S, HKV, D, torch.bfloat16, "cpu", layer_idx=0)
    with pytest.raises(TypeError, match="needs a paged pool"):
        cache.ragged_step_dyn(q, k, k, [0, 1, 2], [0, 1], 0, groups=[0, 2])
    # groups=None is today's call: on a CPU pool it gets as far as the device check of every packed call
    with pytest.raises(RuntimeError, match="MI355X"):
        paged.ragged_step_dyn(q, k, k, [0, 1, 2], [0, 1])
    # host lists are checked against n_seq before anything is uploaded
    for bad in ([0, 3], [2, 1], [-1, 2], [0]):
        with pytest.raises(ValueError, match="groups"):
            SinkCacheLayer._group_arg(bad, 2, "cpu")
    assert SinkCacheLayer._group_arg(group_offsets([5, 5]), 2, "cpu").tolist() == [0, 2]
