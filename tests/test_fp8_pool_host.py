"""CPU-only tests of the FP8 (e4m3) slot pool: the three *_fp8_slots symbols and SFA_DTYPE_FP8_E4M3 in the header, the
table of their refusals (status and exact sfa_last_error() text; host tensors stand in for device memory as in
tests/test_ring_entry_matrix_host.py - every call returns before a launch), every older entry point still answering an FP8
buffer with "unknown dtype 3", the Python refusals of the non-packed methods, and the properties of the storing rule as
tests/fp8_ref.py restates it."""
import ctypes
import inspect
import os
import subprocess
import tempfile

import pytest
import torch

import test_ring_entry_matrix_host as M
from fp8_ref import FP8, dequant, quant, quant_by_division, same_codes
from sink_attention import SinkAttentionCache, SinkCacheLayer
from sink_attention import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HQ, HKV, D, NS, W, S, T = 8, 2, 64, 4, 16, 5, 6
# the scales of tests/test_gpu_fp8_pool.py
K_SCALE, V_SCALE = [0.37, 2.0], [1.0, 0.25]
_KEEP = []


def _d(*shape, dtype=torch.bfloat16, odd=False):
    """a descriptor of a host tensor; odd: D columns of a (D + 8)-column buffer (rows no multiple of 16 bytes for FP8,
    16-byte multiples that start 16-byte aligned for 16-bit types)"""
    t = torch.zeros(*shape[:3], shape[3] + 8, dtype=dtype)[..., :shape[3]] if odd else torch.zeros(*shape, dtype=dtype)
    _KEEP.append(t)
    return N.desc(t)


def _args(act=torch.bfloat16, cache=FP8, d=D, **odd):
    o = lambda k: bool(odd.get(k))
    return dict(q=_d(1, HQ, T, d, dtype=act), kn=_d(1, HKV, T, d, dtype=act, odd=o("kn")), vn=_d(1, HKV, T, d, dtype=act),
                o=_d(1, HQ, T, d, dtype=act), sk=_d(S, HKV, NS, d, dtype=cache), sv=_d(S, HKV, NS, d, dtype=cache),
                wk=_d(S, HKV, W, d, dtype=cache, odd=o("wk")), wv=_d(S, HKV, W, d, dtype=cache, odd=o("wk")))


PTR = ctypes.c_void_p(0x1000)      # stands in for a device array: never read


def _step(a, state=PTR, slots=PTR, cu=PTR, n_seq=2, flags=0):
    lib = N.lib()
    rc = lib.sfa_decode_ring_ragged_fp8_slots(a["q"], a["sk"], a["sv"], a["wk"], a["wv"], a["kn"], a["vn"], a["o"], None,
                                              PTR, PTR, 1, state, slots, cu, n_seq, PTR, None, 0, 0.125, flags, None)
    return rc, lib.sfa_last_error().decode()


def _commit(a, state=PTR, slots=PTR, cu=PTR, n_seq=2, flags=0):
    lib = N.lib()
    rc = lib.sfa_ring_commit_path_ragged_fp8_slots(a["wk"], a["wv"], a["kn"], a["vn"], PTR, PTR, cu, n_seq, state, slots,
                                                   PTR, None)
    return rc, lib.sfa_last_error().decode()


def _fill(a, state=PTR, slots=PTR, cu=PTR, n_seq=2, flags=0):
    lib = N.lib()
    rc = lib.sfa_ring_fill_varlen_fp8_slots(a["sk"], a["sv"], a["wk"], a["wv"], a["kn"], a["vn"], cu, n_seq, state, slots,
                                            PTR, None)
    return rc, lib.sfa_last_error().decode()


CALLS = {"decode_ragged_fp8": _step, "ring_commit_ragged_fp8": _commit, "ring_fill_varlen_fp8": _fill}
ALIGNED = {"decode_ragged_fp8": "decode_multi", "ring_commit_ragged_fp8": "ring_commit", "ring_fill_varlen_fp8": "ring_fill_varlen"}


# ------------------------------------------------------------------------------------------------ exports, header
def test_the_symbols_are_exported_and_the_header_compiles_as_c():
    lib = N.lib()
    assert len(lib.sfa_decode_ring_ragged_fp8_slots.argtypes) == 22
    assert len(lib.sfa_ring_commit_path_ragged_fp8_slots.argtypes) == 12
    assert len(lib.sfa_ring_fill_varlen_fp8_slots.argtypes) == 12
    assert lib.sfa_abi_version() == 2 and N.ABI_VERSION == 2 and N.SFA_DTYPE_FP8_E4M3 == 3
    assert torch.float8_e4m3fn not in N.SFA_DTYPE                  # the activation dtypes are what they were
    TT = "const sfa_tensor*"
    src = ('#include "sfa.h"\n'
           'int main(void) {\n'
           f'  int (*a)({TT}, {TT}, {TT}, {TT}, {TT}, {TT}, {TT}, {TT}, const float*, const int32_t*, const int32_t*, int,\n'
           '           int32_t*, const int32_t*, const int32_t*, int, const float*, void*, size_t, float, unsigned, void*) =\n'
           '      sfa_decode_ring_ragged_fp8_slots;\n'
           f'  int (*b)({TT}, {TT}, {TT}, {TT}, const int32_t*, const int32_t*, const int32_t*, int, int32_t*, const int32_t*,\n'
           '           const float*, void*) = sfa_ring_commit_path_ragged_fp8_slots;\n'
           f'  int (*c)({TT}, {TT}, {TT}, {TT}, {TT}, {TT}, const int32_t*, int, int32_t*, const int32_t*, const float*,\n'
           '           void*) = sfa_ring_fill_varlen_fp8_slots;\n'
           '  return a == 0 || b == 0 || c == 0 || SFA_ABI_VERSION != 2 || SFA_DTYPE_FP8_E4M3 != 3;\n'
           '}\n')
    with tempfile.NamedTemporaryFile("w", suffix=".c", delete=False) as f:
        f.write(src)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                        "-fsyntax-only", f.name], capture_output=True, text=True)
    os.unlink(f.name)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("cls", [SinkCacheLayer, SinkAttentionCache])
def test_python_surface(cls):
    assert "k_scale" in inspect.signature(cls.set_kv_scale).parameters
    if cls is SinkAttentionCache:
        assert "layer_idx" in inspect.signature(cls.set_kv_scale).parameters


# ------------------------------------------------------------------------------------------------ C ABI refusals
@pytest.mark.parametrize("who", list(CALLS))
def test_refusals_of_the_fp8_calls(who):
    call = CALLS[who]
    step = who == "decode_ragged_fp8"
    # a 16-bit pool handed to an _fp8 call
    assert call(_args(cache=torch.bfloat16)) == (-1, f"{who}: the cache buffers must be FP8 (e4m3)")
    # fp32 activations; a head dim no MFMA instance serves
    assert call(_args(act=torch.float32)) == (-2, f"{who}: an FP8 pool serves bf16 / f16 activations at head dims 64 / 80 / "
                                                  "96 / 128 (got dtype 0, head dim 64)")
    assert call(_args(d=48)) == (-2, f"{who}: an FP8 pool serves bf16 / f16 activations at head dims 64 / 80 / 96 / 128 "
                                     "(got dtype 2, head dim 48)")
    # FP8 rows of 72 bytes; 16-bit rows are checked at 2 bytes per element (144-byte rows pass, the FP8 ones do not)
    assert call(_args(wk=True)) == (-1, f"{ALIGNED[who]}: rows of every tensor must be 16-byte aligned")
    bad16 = _args()
    t = torch.zeros(1, HKV, T, D + 1, dtype=torch.bfloat16)[..., :D]
    _KEEP.append(t)
    bad16["kn"] = bad16["vn"] = N.desc(t)
    assert call(bad16) == (-1, f"{ALIGNED[who]}: rows of every tensor must be 16-byte aligned")
    # null device arrays
    ok = _args()
    assert call(ok, state=None) == (-1, "state: null device pointer")
    assert call(ok, slots=None) == (-1, "slots: null device pointer")
    null_cu = "cu_seqlens: null device pointer" if who == "ring_fill_varlen_fp8" else "cu_q: null device pointer"
    assert call(ok, cu=None) == (-1, null_cu)
    # the activations share one dtype; FP8 is no activation dtype
    mixed = dict(ok, kn=_d(1, HKV, T, D, dtype=torch.float16), vn=_d(1, HKV, T, D, dtype=torch.float16))
    if step:
        assert call(mixed) == (-1, "decode_ragged_fp8: q and k_new / v_new must share one dtype")
        assert call(ok, flags=N.FLAG_FORCE_GENERIC)[0] == -2
        # what is left is the workspace: every other check has passed
        rc, err = call(ok)
        assert rc == -3 and err.startswith("decode_ragged workspace: need "), (rc, err)
    act8 = dict(ok, kn=_d(1, HKV, T, D, dtype=FP8), vn=_d(1, HKV, T, D, dtype=FP8))
    rc, err = call(act8)
    assert rc == -1 and err.endswith(": unknown dtype 3"), (rc, err)


def test_every_older_entry_point_still_answers_unknown_dtype_3():
    fp8 = M._descs(dtype=FP8)
    assert len(M.ENTRY) == 23
    for name, (act, cache, _sig) in M.ENTRY.items():
        st, err = M.call(name, descs={c: fp8[c] for c in cache})
        assert st == -1 and err.endswith(": unknown dtype 3"), (name, st, err)
        st, err = M.call(name, descs={c: fp8[c] for c in act + cache})
        assert st == -1 and err.endswith(": unknown dtype 3"), (name, st, err)


def test_copy_slots_takes_fp8_pools_and_refuses_a_mix():
    lib = N.lib()
    a, b = _args(), _args(cache=torch.bfloat16)
    pool = lambda x: (x["sk"], x["sv"], x["wk"], x["wv"])
    rc = lib.sfa_ring_copy_slots(*pool(a), PTR, *pool(a), PTR, PTR, PTR, 0, None)
    assert rc == 0, lib.sfa_last_error()
    rc = lib.sfa_ring_copy_slots(*pool(a), PTR, *pool(b), PTR, PTR, PTR, 1, None)
    assert rc == -1 and b"differ in dtype" in lib.sfa_last_error()
    odd = _args(wk=True)
    rc = lib.sfa_ring_copy_slots(*pool(odd), PTR, *pool(odd), PTR, PTR, PTR, 1, None)
    assert rc == -1 and lib.sfa_last_error() == b"ring_copy_slots: rows of every tensor must be 16-byte aligned"


# ------------------------------------------------------------------------------------------------ Python refusals
def _cpu_pool():
    layer = SinkCacheLayer(NS, W)
    st = layer.init_pool(S, HKV, D, FP8, "cpu")
    assert st.shape == (S, 4) and layer.sink_k.dtype == FP8 and layer.window_v.dtype == FP8
    assert layer.sink_k.element_size() == 1 and layer.window_k.shape == (S, HKV, W, D)
    assert layer.kv_scale.dtype == torch.float32 and layer.kv_scale.shape == (2, HKV) and bool((layer.kv_scale == 1).all())
    return layer


def test_the_non_packed_methods_refuse_an_fp8_pool():
    layer = _cpu_pool()
    q, k = torch.zeros(1, HQ, 1, D, dtype=torch.bfloat16), torch.zeros(1, HKV, 1, D, dtype=torch.bfloat16)
    cnt, par = torch.zeros(1, dtype=torch.int32), torch.tensor([-1], dtype=torch.int32)
    calls = dict(append=(k, k), update=(k, k), get_kv=(), decode_attention=(q,), decode_step=(q, k, k),
                 extend_attention=(q, k, k), extend_step=(q, k, k), decode_step_dyn=(q, k, k),
                 extend_attention_dyn=(q, k, k), extend_step_dyn=(q, k, k), commit_dyn=(k, k, cnt),
                 extend_attention_tree=(q, k, k, [-1]), extend_attention_tree_dyn=(q, k, k, par),
                 commit_path_dyn=(k, k, par, cnt), commit_path=(k, k, [0]), prefill_varlen=(k, k, [0, 1]),
                 get_seq_length=())
    for name, args in calls.items():
        with pytest.raises(TypeError, match=r"FP8 .* pool: use the packed calls prefill_slots / ragged_step_dyn / "
                                            r"commit_packed_dyn") as e:
            getattr(layer, name)(*args)
        assert name in str(e.value), (name, str(e.value))
    assert layer.sink_k.dtype == FP8 and not layer._dev_state.any()            # nothing was replaced or moved


def test_set_kv_scale_copies_in_place_and_init_pool_checks_the_head_dim():
    layer = _cpu_pool()
    ptr = layer.kv_scale.data_ptr()
    layer.set_kv_scale(K_SCALE, torch.tensor(V_SCALE, dtype=torch.float64))
    assert layer.kv_scale.data_ptr() == ptr and layer.kv_scale.dtype == torch.float32
    assert torch.equal(layer.kv_scale, torch.tensor([K_SCALE, V_SCALE], dtype=torch.float32))
    layer.set_kv_scale(0.5, 2)
    assert layer.kv_scale.tolist() == [[0.5, 0.5], [2.0, 2.0]] and layer.kv_scale.data_ptr() == ptr
    with pytest.raises(ValueError, match="H_kv = 2"):
        layer.set_kv_scale([1.0, 2.0, 3.0], V_SCALE)
    cache = SinkAttentionCache(NS, W)
    cache.init_pool(S, HKV, D, FP8, "cpu", layer_idx=1)
    cache.set_kv_scale(K_SCALE, V_SCALE, layer_idx=1)
    assert torch.equal(cache[1].kv_scale, torch.tensor([K_SCALE, V_SCALE], dtype=torch.float32))
    with pytest.raises(ValueError, match="64 / 80 / 96 / 128"):
        SinkCacheLayer(NS, W).init_pool(S, HKV, 48, FP8, "cpu")
    bf = SinkCacheLayer(NS, W)
    bf.init_pool(S, HKV, D, torch.bfloat16, "cpu")
    assert bf.kv_scale is None
    with pytest.raises(TypeError, match="FP8 pool"):
        bf.set_kv_scale(K_SCALE, V_SCALE)


# ------------------------------------------------------------------------------------------------ the storing rule
def _all16(dtype):
    """every finite value of a 16-bit dtype, as [1, H_kv, n, 8] (the same values under each head's scale)"""
    x = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(dtype)
    x = x[torch.isfinite(x.float())]
    x = x[:x.numel() // 8 * 8].reshape(1, 1, -1, 8)
    return x.expand(1, HKV, -1, 8).contiguous()


def test_overflow_saturates_to_448_and_never_becomes_nan():
    x = torch.tensor([448.0, -448.0, 449.0, -1e4, 3e38, -3e38, 464.0, 480.0], dtype=torch.bfloat16).reshape(1, 1, 1, 8)
    codes = quant(x.expand(1, HKV, 1, 8), [1.0, 1.0]).view(torch.uint8)[0, 0, 0].tolist()
    assert codes == [0x7e, 0xfe, 0x7e, 0xfe, 0x7e, 0xfe, 0x7e, 0x7e], [hex(c) for c in codes]
    for dtype in (torch.bfloat16, torch.float16):
        x = _all16(dtype)
        for row in (K_SCALE, V_SCALE, None, [2.0 ** -3, 2.0 ** 2]):
            c = quant(x, row).view(torch.uint8)
            assert not ((c & 0x7f) == 0x7f).any(), (dtype, row, "a NaN code from finite input")
            big = (x.float().abs() / torch.tensor(row or [1.0, 1.0])[:, None, None]) > 448
            assert ((c[big] & 0x7f) == 0x7e).all(), (dtype, row, "|x| / scale > 448 must give +-448")
            assert (((c >> 7) == 1) == (x.view(torch.int16) < 0)).all(), (dtype, row, "the sign survives")


def test_the_reciprocal_and_the_division_give_the_same_codes_at_the_tests_scales():
    for dtype in (torch.bfloat16, torch.float16):
        x = _all16(dtype)
        for row in (K_SCALE, V_SCALE, None):
            a, b = quant(x, row), quant_by_division(x, row)
            bad = (a.view(torch.uint8) != b.view(torch.uint8)).nonzero()
            assert same_codes(a, b), (dtype, row, bad[:4].tolist(), x[tuple(bad[0])].item() if len(bad) else None)


def test_dequant_is_one_multiply_and_exact_at_power_of_two_scales():
    codes = torch.arange(256, dtype=torch.uint8).view(FP8)
    keep = torch.isfinite(codes.float())
    codes = codes[keep][:248].reshape(1, 1, 31, 8).expand(1, HKV, 31, 8).contiguous()
    for dtype in (torch.bfloat16, torch.float16):
        y = dequant(codes, V_SCALE, dtype)                   # 1.0 and 0.25: exact in both 16-bit types
        assert y.dtype == dtype and torch.equal(y.float(), codes.float() * torch.tensor(V_SCALE)[:, None, None])
        assert same_codes(quant(y, V_SCALE), codes)          # and a round trip gives the codes back
        z = dequant(codes, K_SCALE, dtype)                   # 0.37: rounded once into the 16-bit type
        assert torch.equal(z, (codes.float() * torch.tensor(K_SCALE, dtype=torch.float32)[:, None, None]).to(dtype))
