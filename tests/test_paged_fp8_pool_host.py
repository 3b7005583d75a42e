"""CPU-only tests of the paged FP8 slot pool: the three *_paged_fp8_slots symbols in the header, the table of their
refusals (status and exact sfa_last_error() text, in the documented order; host tensors stand in for device memory as in
tests/test_paged_pool_host.py - every call returns before a launch), sfa_ring_copy_paged_slots on FP8 descriptors, and the
Python surface of init_pool(..., page_size=P, kv_dtype=torch.float8_e4m3fn)."""
import ctypes
import os
import subprocess
import tempfile

import pytest
import torch

from sink_attention import PageAllocator, SinkAttentionCache, SinkCacheLayer
from sink_attention import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP8 = torch.float8_e4m3fn
HQ, HKV, D, NS, S, T = 8, 2, 64, 4, 5, 6
P, PER, NP = 32, 3, 7              # Wc = 96: three pages per slot, a pool of seven
W = P * PER
_KEEP = []
PTR = ctypes.c_void_p(0x1000)      # stands in for a device array: never read


def _d(*shape, dtype=torch.bfloat16):
    t = torch.zeros(*shape, dtype=dtype)
    _KEEP.append(t)
    return N.desc(t)


def _args(act=torch.bfloat16, d=D, p=P, npk=NP, npv=None, cache=FP8, sinks=None):
    sinks = cache if sinks is None else sinks
    return dict(q=_d(1, HQ, T, d, dtype=act), kn=_d(1, HKV, T, d, dtype=act), vn=_d(1, HKV, T, d, dtype=act),
                o=_d(1, HQ, T, d, dtype=act), sk=_d(S, HKV, NS, d, dtype=sinks), sv=_d(S, HKV, NS, d, dtype=sinks),
                wk=_d(npk, HKV, p, d, dtype=cache), wv=_d(npk if npv is None else npv, HKV, p, d, dtype=cache))


def _step(a, state=PTR, slots=PTR, cu=PTR, table=PTR, stride=PER, flags=0):
    lib = N.lib()
    rc = lib.sfa_decode_ring_ragged_paged_fp8_slots(a["q"], a["sk"], a["sv"], a["wk"], a["wv"], a["kn"], a["vn"], a["o"],
                                                    None, PTR, PTR, 1, state, slots, cu, 2, table, stride, PTR, None, 0,
                                                    0.125, flags, None)
    return rc, lib.sfa_last_error().decode()


def _commit(a, state=PTR, slots=PTR, cu=PTR, table=PTR, stride=PER, flags=0):
    lib = N.lib()
    rc = lib.sfa_ring_commit_path_ragged_paged_fp8_slots(a["wk"], a["wv"], a["kn"], a["vn"], PTR, PTR, cu, 2, state, slots,
                                                         table, stride, S, PTR, None)
    return rc, lib.sfa_last_error().decode()


def _fill(a, state=PTR, slots=PTR, cu=PTR, table=PTR, stride=PER, flags=0):
    lib = N.lib()
    rc = lib.sfa_ring_fill_varlen_paged_fp8_slots(a["sk"], a["sv"], a["wk"], a["wv"], a["kn"], a["vn"], cu, 2, state, slots,
                                                  table, stride, PTR, None)
    return rc, lib.sfa_last_error().decode()


CALLS = {"decode_ragged_paged_fp8": _step, "ring_commit_ragged_paged_fp8": _commit, "ring_fill_varlen_paged_fp8": _fill}


# ------------------------------------------------------------------------------------------------ exports, header
def test_the_symbols_are_exported_and_the_header_compiles_as_c():
    lib = N.lib()
    assert len(lib.sfa_decode_ring_ragged_paged_fp8_slots.argtypes) == 24
    assert len(lib.sfa_ring_commit_path_ragged_paged_fp8_slots.argtypes) == 15
    assert len(lib.sfa_ring_fill_varlen_paged_fp8_slots.argtypes) == 14
    assert lib.sfa_abi_version() == 2 and N.ABI_VERSION == 2
    TT, I = "const sfa_tensor*", "const int32_t*"
    src = ('#include "sfa.h"\n'
           'int main(void) {\n'
           f'  int (*a)({TT}, {TT}, {TT}, {TT}, {TT}, {TT}, {TT}, {TT}, const float*, {I}, {I}, int,\n'
           f'           int32_t*, {I}, {I}, int, {I}, int, const float*, void*, size_t, float, unsigned, void*) =\n'
           '      sfa_decode_ring_ragged_paged_fp8_slots;\n'
           f'  int (*b)({TT}, {TT}, {TT}, {TT}, {I}, {I}, {I}, int, int32_t*, {I}, {I}, int, int, const float*, void*) =\n'
           '      sfa_ring_commit_path_ragged_paged_fp8_slots;\n'
           f'  int (*c)({TT}, {TT}, {TT}, {TT}, {TT}, {TT}, {I}, int, int32_t*, {I}, {I}, int, const float*, void*) =\n'
           '      sfa_ring_fill_varlen_paged_fp8_slots;\n'
           '  return a == 0 || b == 0 || c == 0 || SFA_ABI_VERSION != 2;\n'
           '}\n')
    with tempfile.NamedTemporaryFile("w", suffix=".c", delete=False) as f:
        f.write(src)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                        "-fsyntax-only", f.name], capture_output=True, text=True)
    os.unlink(f.name)
    assert r.returncode == 0, r.stderr


# ------------------------------------------------------------------------------------------------ C ABI refusals
@pytest.mark.parametrize("who", list(CALLS))
def test_refusals_of_the_paged_fp8_calls_in_their_order(who):
    call = CALLS[who]
    ok = _args()
    # 1. the checks a paged call adds, with the existing texts under the new names
    assert call(dict(ok, wk=None)) == (-1, "window_k: null tensor descriptor")
    assert call(ok, table=None) == (-1, "page_table: null device pointer")
    for p in (48, 16, 1):
        assert call(_args(p=p)) == (-1, f"{who}: the page size (window_k shape[2] = {p}) must be a power of two and at "
                                        "least 32")
    assert call(ok, stride=0) == (-1, f"{who}: table_stride (0) must be at least 1 (Wc = table_stride * P)")
    assert call(_args(npv=NP + 1)) == (-1, f"window_k and window_v differ in shape[0]: {NP} vs {NP + 1}")
    assert call(_args(npk=0)) == (-1, f"{who}: the page buffers need shape[0] = n_pages in [1, 2^30) (got 0)")
    assert call(_args(p=48), table=None)[1] == "page_table: null device pointer"
    assert call(_args(p=48), stride=0)[1].startswith(f"{who}: the page size")
    # a bad page size of 16-bit pages is a page-size error too: the paged checks come before the dtypes are compared
    assert call(_args(p=48, cache=torch.bfloat16))[1].startswith(f"{who}: the page size")
    # 2. the FP8 sibling's checks in their order: null device arrays ...
    assert call(ok, state=None) == (-1, "state: null device pointer")
    assert call(ok, slots=None) == (-1, "slots: null device pointer")
    null_cu = "cu_seqlens: null device pointer" if who == "ring_fill_varlen_paged_fp8" else "cu_q: null device pointer"
    assert call(ok, cu=None) == (-1, null_cu)
    # ... the cache buffers are FP8 (a 16-bit page buffer ends here), the activations share one dtype ...
    for bad in (torch.bfloat16, torch.float16):
        assert call(_args(cache=bad)) == (-1, f"{who}: the cache buffers must be FP8 (e4m3)")
    if who != "ring_commit_ragged_paged_fp8":                     # the commit takes no sinks
        assert call(_args(sinks=torch.bfloat16)) == (-1, f"{who}: the cache buffers must be FP8 (e4m3)")
    mixed = dict(ok, kn=_d(1, HKV, T, D, dtype=torch.float16), vn=_d(1, HKV, T, D, dtype=torch.float16))
    if who == "decode_ragged_paged_fp8":
        assert call(mixed) == (-1, f"{who}: q and k_new / v_new must share one dtype")
    # 3. what a paged FP8 pool serves: no fp32 activations, no other head dim, no generic kernels
    served = f"{who}: a paged FP8 pool serves bf16 / f16 activations at head dims 64 / 80 / 96 / 128 "
    assert call(_args(act=torch.float32)) == (-2, served + "(got dtype 0, head dim 64)")
    assert call(_args(d=48)) == (-2, served + "(got dtype 2, head dim 48)")
    assert call(_args(act=torch.float16, d=48)) == (-2, served + "(got dtype 1, head dim 48)")
    if who == "decode_ragged_paged_fp8":
        assert call(ok, flags=N.FLAG_FORCE_GENERIC) == (-2, served + "(got dtype 2, head dim 64, SFA_FLAG_FORCE_GENERIC)")
        # what is left is the workspace, sized with q's dtype for Wc = table_stride * P: every other check has passed
        for act in (torch.bfloat16, torch.float16):
            rc, err = call(_args(act=act))
            need = N.lib().sfa_decode_ragged_workspace_bytes(2, HQ, HKV, T, NS + W, D, N.SFA_DTYPE[act])
            assert need > 0 and rc == -3 and err.startswith(f"decode_ragged workspace: need {need} bytes"), (rc, err)
        rc, err = call(ok, stride=PER + 2)
        need = N.lib().sfa_decode_ragged_workspace_bytes(2, HQ, HKV, T, NS + (PER + 2) * P, D, N.SFA_DTYPE[torch.bfloat16])
        assert rc == -3 and err.startswith(f"decode_ragged workspace: need {need} bytes"), (rc, err)


def test_the_commit_takes_the_pool_size_as_an_argument():
    lib = N.lib()
    a = _args()
    rc = lib.sfa_ring_commit_path_ragged_paged_fp8_slots(a["wk"], a["wv"], a["kn"], a["vn"], PTR, PTR, PTR, 2, PTR, PTR, PTR,
                                                         PER, 0, PTR, None)
    assert rc == -1 and lib.sfa_last_error() == b"pool: the ring needs shape[0] = S >= 1 slots (got 0)"


def test_the_existing_paged_and_fp8_calls_keep_their_refusals():
    lib = N.lib()
    a = _args()                                                     # FP8 pages and sinks
    rc = lib.sfa_decode_ring_ragged_paged_slots(a["q"], a["sk"], a["sv"], a["wk"], a["wv"], a["kn"], a["vn"], a["o"], None,
                                                PTR, PTR, 1, PTR, PTR, PTR, 2, PTR, PER, None, 0, 0.125, 0, None)
    assert (rc, lib.sfa_last_error()) == (-1, b"window_k: unknown dtype 3")
    rc = lib.sfa_ring_fill_varlen_paged_slots(a["sk"], a["sv"], a["wk"], a["wv"], a["kn"], a["vn"], PTR, 2, PTR, PTR, PTR, PER,
                                              None)
    assert (rc, lib.sfa_last_error()) == (-1, b"window_k: unknown dtype 3")
    rc = lib.sfa_ring_commit_path_ragged_paged_slots(a["wk"], a["wv"], a["kn"], a["vn"], PTR, PTR, PTR, 2, PTR, PTR, PTR, PER,
                                                     S, None)
    assert (rc, lib.sfa_last_error()) == (-1, b"window_k: unknown dtype 3")
    # the contiguous FP8 calls: their names and texts, on a contiguous ring [S, H_kv, Wc, D]
    def fp8(act=torch.bfloat16, cache=FP8):
        c = dict(_args(act=act, cache=cache), wk=_d(S, HKV, W, D, dtype=cache), wv=_d(S, HKV, W, D, dtype=cache))
        step = lib.sfa_decode_ring_ragged_fp8_slots(c["q"], c["sk"], c["sv"], c["wk"], c["wv"], c["kn"], c["vn"], c["o"], None,
                                                    PTR, PTR, 1, PTR, PTR, PTR, 2, PTR, None, 0, 0.125, 0, None)
        e_step = lib.sfa_last_error().decode()
        com = lib.sfa_ring_commit_path_ragged_fp8_slots(c["wk"], c["wv"], c["kn"], c["vn"], PTR, PTR, PTR, 2, PTR, PTR, PTR, None)
        e_com = lib.sfa_last_error().decode()
        fill = lib.sfa_ring_fill_varlen_fp8_slots(c["sk"], c["sv"], c["wk"], c["wv"], c["kn"], c["vn"], PTR, 2, PTR, PTR, PTR, None)
        return [(step, e_step), (com, e_com), (fill, lib.sfa_last_error().decode())]
    names = ("decode_ragged_fp8", "ring_commit_ragged_fp8", "ring_fill_varlen_fp8")
    assert fp8(cache=torch.bfloat16) == [(-1, f"{n}: the cache buffers must be FP8 (e4m3)") for n in names]
    assert fp8(act=torch.float32) == [(-2, f"{n}: an FP8 pool serves bf16 / f16 activations at head dims 64 / 80 / 96 / 128 "
                                           "(got dtype 0, head dim 64)") for n in names]
    rc, err = fp8()[0]
    assert rc == -3 and err.startswith("decode_ragged workspace: need"), (rc, err)


def _copy(a, b=None, n_pairs=1):
    lib = N.lib()
    b = a if b is None else b
    pool = lambda x: (x["sk"], x["sv"], x["wk"], x["wv"])
    rc = lib.sfa_ring_copy_paged_slots(*pool(a), PTR, *pool(b), PTR, PTR, PTR, n_pairs, PTR, PER, PTR, PER, None)
    return rc, lib.sfa_last_error().decode()


def test_the_paged_copy_takes_fp8_pools_and_still_refuses_mixed_ones():
    ok = _args()
    assert _copy(ok, n_pairs=0) == (0, "")                          # all eight FP8: the dtype checks pass, nothing to do
    assert _copy(ok, b=_args(npk=3), n_pairs=0) == (0, "")
    one = "(the eight buffers must share one)"
    assert _copy(_args(sinks=torch.bfloat16)) == (-1, f"ring_copy_slots: src_window_k and src_sink_k differ in dtype {one}")
    assert _copy(ok, b=_args(cache=torch.bfloat16)) == (-1, f"ring_copy_slots: dst_sink_k and src_sink_k differ in dtype {one}")
    assert _copy(_args(cache=torch.bfloat16), b=ok) == (-1, f"ring_copy_slots: dst_sink_k and src_sink_k differ in dtype {one}")
    assert _copy(ok, b=_args(p=64)) == (-1, "ring_copy_paged: the pools differ in page size (src 32, dst 64)")
    rc, err = _copy(ok, b=_args(d=128))
    assert rc == -1 and err.startswith("ring_copy_slots: dst_sink_k must be [S, H_kv, num_sink, D]"), (rc, err)
    # one byte per element: rows of D = 72 codes are no multiple of 16 bytes; other head dims stay unsupported
    assert _copy(_args(d=72)) == (-1, "ring_copy_slots: K/V rows must be a multiple of 16 bytes (head dim 72)")
    assert _copy(_args(d=48)) == (-2, "ring_copy_paged: a paged pool serves bf16 / f16 at head dims 64 / 80 / 96 / 128 "
                                      "(got dtype 3, head dim 48)")


# ------------------------------------------------------------------------------------------------ Python surface
def _cpu_pool(act=torch.bfloat16, **kw):
    layer = SinkCacheLayer(NS, W)
    st = layer.init_pool(S, HKV, D, act, "cpu", page_size=P, kv_dtype=FP8, **kw)
    assert st.shape == (S, 4) and not st.any() and layer.page_size == P and layer.window_size == W
    return layer


def test_init_pool_with_kv_dtype_allocates_fp8_pages_sinks_scales_and_a_table():
    for act in (torch.bfloat16, torch.float16):
        layer = _cpu_pool(act, num_pages=NP)
        assert layer.window_k.shape == layer.window_v.shape == (NP, HKV, P, D)
        assert layer.sink_k.shape == layer.sink_v.shape == (S, HKV, NS, D)
        assert {t.dtype for t in (layer.sink_k, layer.sink_v, layer.window_k, layer.window_v)} == {FP8}
        assert layer.kv_scale.shape == (2, HKV) and layer.kv_scale.dtype == torch.float32 and bool((layer.kv_scale == 1).all())
        assert layer.page_table.dtype == torch.int32 and layer.page_table.shape == (S, PER)
        assert bool((layer.page_table == -1).all()) and layer.num_slots == S and layer._kv8
    assert _cpu_pool().window_k.shape == (S * PER, HKV, P, D)              # the default: the full capacity
    given = torch.full((S, PER), -1, dtype=torch.int32)
    assert _cpu_pool(page_table=given).page_table is given
    # without page_size the keyword gives the contiguous FP8 pool of dtype=float8_e4m3fn
    a, b = SinkCacheLayer(NS, W), SinkCacheLayer(NS, W)
    a.init_pool(S, HKV, D, torch.bfloat16, "cpu", kv_dtype=FP8)
    b.init_pool(S, HKV, D, FP8, "cpu")
    for name in ("sink_k", "sink_v", "window_k", "window_v", "kv_scale", "_dev_state"):
        x, y = getattr(a, name), getattr(b, name)
        assert x.shape == y.shape and x.dtype == y.dtype, name
    assert a.window_k.shape == (S, HKV, W, D) and a.page_size is None and a.page_table is None and a._pages is None


def test_kv_dtype_none_is_the_pool_of_today():
    for kw in (dict(), dict(page_size=P, num_pages=NP)):
        a, b = SinkCacheLayer(NS, W), SinkCacheLayer(NS, W)
        a.init_pool(S, HKV, D, torch.float16, "cpu", **kw)
        b.init_pool(S, HKV, D, torch.float16, "cpu", kv_dtype=None, **kw)
        for name in ("sink_k", "sink_v", "window_k", "window_v", "_dev_state"):
            x, y = getattr(a, name), getattr(b, name)
            assert x.shape == y.shape and x.dtype == y.dtype == (torch.int32 if name == "_dev_state" else torch.float16)
        assert b.kv_scale is None and a.page_size == b.page_size and not b._kv8
        assert (a.page_table is None) == (b.page_table is None)
    f = SinkCacheLayer(NS, W)
    f.init_pool(S, HKV, D, torch.float32, "cpu")                          # fp32 pools stay as they are
    assert f.window_k.dtype == torch.float32


def test_the_refusals_of_init_pool():
    mk = lambda w=W: SinkCacheLayer(NS, w)
    with pytest.raises(TypeError, match="paged FP8 pool is not served"):    # the legacy spelling keeps its refusal
        mk().init_pool(S, HKV, D, FP8, "cpu", page_size=P)
    for bad in (torch.float16, torch.float32, torch.float8_e5m2, torch.int8, "fp8"):
        with pytest.raises(TypeError, match="kv_dtype must be None"):
            mk().init_pool(S, HKV, D, torch.bfloat16, "cpu", page_size=P, kv_dtype=bad)
        with pytest.raises(TypeError, match="kv_dtype must be None"):
            mk().init_pool(S, HKV, D, torch.bfloat16, "cpu", kv_dtype=bad)
    for kw in (dict(page_size=P), dict()):
        with pytest.raises(TypeError, match="dtype names the activations and must be bfloat16 or float16"):
            mk().init_pool(S, HKV, D, torch.float32, "cpu", kv_dtype=FP8, **kw)
    with pytest.raises(ValueError, match="head dims 64 / 80 / 96 / 128"):
        mk().init_pool(S, HKV, 48, torch.bfloat16, "cpu", page_size=P, kv_dtype=FP8)
    with pytest.raises(ValueError, match="head dims 64 / 80 / 96 / 128"):
        mk().init_pool(S, HKV, 48, torch.bfloat16, "cpu", kv_dtype=FP8)
    with pytest.raises(ValueError, match="power of two and at least 32"):
        mk().init_pool(S, HKV, D, torch.bfloat16, "cpu", page_size=48, kv_dtype=FP8)
    with pytest.raises(ValueError, match=r"window_size \(80\) must be a multiple of page_size \(32\)"):
        mk(80).init_pool(S, HKV, D, torch.bfloat16, "cpu", page_size=32, kv_dtype=FP8)


def test_the_non_packed_methods_refuse_a_paged_fp8_pool():
    layer = _cpu_pool(num_pages=NP)
    q, k = torch.zeros(1, HQ, 1, D, dtype=torch.bfloat16), torch.zeros(1, HKV, 1, D, dtype=torch.bfloat16)
    cnt, par = torch.zeros(1, dtype=torch.int32), torch.tensor([-1], dtype=torch.int32)
    calls = dict(append=(k, k), update=(k, k), get_kv=(), decode_attention=(q,), decode_step=(q, k, k),
                 extend_attention=(q, k, k), extend_step=(q, k, k), decode_step_dyn=(q, k, k),
                 extend_attention_dyn=(q, k, k), extend_step_dyn=(q, k, k), commit_dyn=(k, k, cnt),
                 extend_attention_tree=(q, k, k, [-1]), extend_attention_tree_dyn=(q, k, k, par),
                 commit_path_dyn=(k, k, par, cnt), commit_path=(k, k, [0]), prefill_varlen=(k, k, [0, 1]),
                 get_seq_length=())
    for name, args in calls.items():
        with pytest.raises(TypeError, match=r"(FP8 \(float8_e4m3fn\)|paged) pool.*: use the packed calls prefill_slots / "
                                            r"ragged_step_dyn / commit_packed_dyn") as e:
            getattr(layer, name)(*args)
        assert name in str(e.value), (name, str(e.value))
    assert layer.window_k.shape == (NP, HKV, P, D) and layer.window_k.dtype == FP8 and not layer._dev_state.any()
    with pytest.raises(RuntimeError, match="MI355X"):              # a packed call: only the device is missing
        layer.prefill_slots(k, k, [0, 1], [0])


def test_scales_and_pages_of_a_paged_fp8_pool():
    layer = _cpu_pool(num_pages=NP)
    ptr = layer.kv_scale.data_ptr()
    layer.set_kv_scale([0.37, 2.0], 0.25)
    assert layer.kv_scale.data_ptr() == ptr
    assert layer.kv_scale.tolist() == torch.tensor([[0.37, 2.0], [0.25, 0.25]], dtype=torch.float32).tolist()
    with pytest.raises(ValueError, match="H_kv = 2 values"):
        layer.set_kv_scale([1.0, 2.0, 3.0], 1.0)
    layer.reserve_pages([3, 1], [40, 1])
    assert layer.page_table.tolist() == [[-1] * 3, [2, -1, -1], [-1] * 3, [0, 1, -1], [-1] * 3]
    layer.free_pages([3])
    assert layer.page_table[3].tolist() == [-1] * 3 and len(layer._pages.free_list) == NP - 1
    with pytest.raises(RuntimeError, match=r"^out of pages: need 9, free 6$"):
        layer.reserve_pages([0, 2, 3], [96, 96, 96])
    plain = SinkCacheLayer(NS, W)
    plain.init_pool(S, HKV, D, torch.bfloat16, "cpu", page_size=P)
    with pytest.raises(TypeError, match="set_kv_scale needs an FP8 pool"):
        plain.set_kv_scale(1.0, 1.0)


def test_the_layers_of_a_cache_share_one_table_and_keep_their_own_scales():
    cache = SinkAttentionCache(NS, W)
    for l in range(2):
        cache.init_pool(S, HKV, D, torch.bfloat16, "cpu", layer_idx=l, page_size=P, num_pages=NP, kv_dtype=FP8)
    assert all(cache[l].page_table is cache.page_table and cache[l].window_k.dtype == FP8 for l in range(2))
    assert cache[0].window_k.data_ptr() != cache[1].window_k.data_ptr() and cache[1]._pages is cache[0]._pages
    cache.reserve_pages([2, 4], [33, 1])
    assert cache.page_table.tolist() == [[-1] * 3, [-1] * 3, [0, 1, -1], [-1] * 3, [2, -1, -1]]
    cache.set_kv_scale([0.5, 1.5], [2.0, 0.75], layer_idx=1)
    assert cache[1].kv_scale.tolist() == [[0.5, 1.5], [2.0, 0.75]] and bool((cache[0].kv_scale == 1).all())
    plain = SinkAttentionCache(NS, W)
    plain.init_pool(S, HKV, D, torch.float16, "cpu", kv_dtype=FP8)        # passed through without paging too
    assert plain[0].window_k.dtype == FP8 and plain[0].window_k.shape == (S, HKV, W, D) and plain.page_table is None


def test_fork_slots_refuses_pools_that_differ_in_kv_dtype_paging_or_ring():
    a, b = _cpu_pool(num_pages=NP), _cpu_pool(num_pages=2 * NP)
    p16 = SinkCacheLayer(NS, W)
    p16.init_pool(S, HKV, D, torch.bfloat16, "cpu", page_size=P, num_pages=NP)
    c8 = SinkCacheLayer(NS, W)
    c8.init_pool(S, HKV, D, torch.bfloat16, "cpu", kv_dtype=FP8)
    p64 = SinkCacheLayer(NS, 2 * W)
    p64.init_pool(S, HKV, D, torch.bfloat16, "cpu", page_size=2 * P, kv_dtype=FP8)
    wide = SinkCacheLayer(NS, 2 * W)
    wide.init_pool(S, HKV, D, torch.bfloat16, "cpu", page_size=P, kv_dtype=FP8)
    with pytest.raises(TypeError, match="differ in dtype"):
        a.fork_slots([0], [1], source=p16)
    for other in (c8, p64, wide):
        with pytest.raises(ValueError, match="differ in (geometry|paging)"):
            a.fork_slots([0], [1], source=other)
    with pytest.raises(RuntimeError, match="MI355X"):              # equal kv_dtype, P and Wc, another n_pages: only the device is missing
        a.fork_slots([0], [1], source=b)


def test_pool_bytes_at_one_byte_per_element_is_half_the_16_bit_figure():
    """the allocator example of DESIGN.md 3.3.10: 64 slots, Wc 4096, P 64, H_kv 8, D 128, holding 32 x 200, 16 x 1000,
    12 x 4000 and 4 x 30000 tokens: 1396 of 4096 pages, 349 MiB per layer at 16 bits, 174.5 MiB in FP8"""
    S_, Wc, P_, Hkv, D_ = 64, 4096, 64, 8, 128
    alloc = PageAllocator(torch.full((S_, Wc // P_), -1, dtype=torch.int32), S_ * Wc // P_, P_, Wc)
    alloc.reserve(list(range(S_)), [200] * 32 + [1000] * 16 + [4000] * 12 + [30000] * 4)
    assert sum(len(r) for r in alloc.rows) == 1396
    b2, b1 = alloc.pool_bytes(Hkv, D_, 2), alloc.pool_bytes(Hkv, D_, 1)
    assert b2 == 2 * b1 == 349 * 2 ** 20 and b1 == 2 * 1396 * Hkv * P_ * D_
    print("paged 16-bit", b2 / 2 ** 20, "MiB; paged FP8", b1 / 2 ** 20, "MiB; contiguous 16-bit",
          2 * S_ * Hkv * Wc * D_ * 2 / 2 ** 20, "MiB")
