"""CPU-only tests of the paged slot pool: the four *_paged_slots symbols in the header, the table of their refusals (status
and exact sfa_last_error() text; host tensors stand in for device memory as in tests/test_fp8_pool_host.py - every call
returns before a launch), the Python refusals of the non-packed methods and of FP8 plus paging, the host-side page
allocator (the prefix rule against a brute-force walk of the placements, exhaustion, reuse, one table for every layer)
and the properties of tests/paged_ref.py::gather."""
import ctypes
import os
import subprocess
import tempfile

import pytest
import torch

import paged_ref as PR
from sink_attention import PageAllocator, SinkAttentionCache, SinkCacheLayer, pages_needed
from sink_attention import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HQ, HKV, D, NS, S, T = 8, 2, 64, 4, 5, 6
P, PER, NP = 32, 3, 7              # Wc = 96: three pages per slot, a pool of seven
W = P * PER
_KEEP = []
PTR = ctypes.c_void_p(0x1000)      # stands in for a device array: never read


def _d(*shape, dtype=torch.bfloat16):
    t = torch.zeros(*shape, dtype=dtype)
    _KEEP.append(t)
    return N.desc(t)


def _args(act=torch.bfloat16, d=D, p=P, npk=NP, npv=None):
    return dict(q=_d(1, HQ, T, d, dtype=act), kn=_d(1, HKV, T, d, dtype=act), vn=_d(1, HKV, T, d, dtype=act),
                o=_d(1, HQ, T, d, dtype=act), sk=_d(S, HKV, NS, d, dtype=act), sv=_d(S, HKV, NS, d, dtype=act),
                wk=_d(npk, HKV, p, d, dtype=act), wv=_d(npk if npv is None else npv, HKV, p, d, dtype=act))


def _step(a, state=PTR, slots=PTR, cu=PTR, table=PTR, stride=PER, flags=0):
    lib = N.lib()
    rc = lib.sfa_decode_ring_ragged_paged_slots(a["q"], a["sk"], a["sv"], a["wk"], a["wv"], a["kn"], a["vn"], a["o"], None,
                                                PTR, PTR, 1, state, slots, cu, 2, table, stride, None, 0, 0.125, flags, None)
    return rc, lib.sfa_last_error().decode()


def _commit(a, state=PTR, slots=PTR, cu=PTR, table=PTR, stride=PER, flags=0):
    lib = N.lib()
    rc = lib.sfa_ring_commit_path_ragged_paged_slots(a["wk"], a["wv"], a["kn"], a["vn"], PTR, PTR, cu, 2, state, slots,
                                                     table, stride, S, None)
    return rc, lib.sfa_last_error().decode()


def _fill(a, state=PTR, slots=PTR, cu=PTR, table=PTR, stride=PER, flags=0):
    lib = N.lib()
    rc = lib.sfa_ring_fill_varlen_paged_slots(a["sk"], a["sv"], a["wk"], a["wv"], a["kn"], a["vn"], cu, 2, state, slots,
                                              table, stride, None)
    return rc, lib.sfa_last_error().decode()


def _copy(a, state=PTR, slots=PTR, cu=PTR, table=PTR, stride=PER, flags=0, b=None, n_pairs=1):
    lib = N.lib()
    b = a if b is None else b
    pool = lambda x: (x["sk"], x["sv"], x["wk"], x["wv"])
    rc = lib.sfa_ring_copy_paged_slots(*pool(a), state, *pool(b), state, slots, slots, n_pairs, table, stride, table, stride,
                                       None)
    return rc, lib.sfa_last_error().decode()


CALLS = {"decode_ragged_paged": _step, "ring_commit_ragged_paged": _commit, "ring_fill_varlen_paged": _fill,
         "ring_copy_paged": _copy}


# ------------------------------------------------------------------------------------------------ exports, header
def test_the_symbols_are_exported_and_the_header_compiles_as_c():
    lib = N.lib()
    assert len(lib.sfa_decode_ring_ragged_paged_slots.argtypes) == 23
    assert len(lib.sfa_ring_commit_path_ragged_paged_slots.argtypes) == 14
    assert len(lib.sfa_ring_fill_varlen_paged_slots.argtypes) == 13
    assert len(lib.sfa_ring_copy_paged_slots.argtypes) == 18
    assert lib.sfa_abi_version() == 2 and N.ABI_VERSION == 2
    TT, I = "const sfa_tensor*", "const int32_t*"
    src = ('#include "sfa.h"\n'
           'int main(void) {\n'
           f'  int (*a)({TT}, {TT}, {TT}, {TT}, {TT}, {TT}, {TT}, {TT}, const float*, {I}, {I}, int,\n'
           f'           int32_t*, {I}, {I}, int, {I}, int, void*, size_t, float, unsigned, void*) =\n'
           '      sfa_decode_ring_ragged_paged_slots;\n'
           f'  int (*b)({TT}, {TT}, {TT}, {TT}, {I}, {I}, {I}, int, int32_t*, {I}, {I}, int, int, void*) =\n'
           '      sfa_ring_commit_path_ragged_paged_slots;\n'
           f'  int (*c)({TT}, {TT}, {TT}, {TT}, {TT}, {TT}, {I}, int, int32_t*, {I}, {I}, int, void*) =\n'
           '      sfa_ring_fill_varlen_paged_slots;\n'
           f'  int (*d)({TT}, {TT}, {TT}, {TT}, {I}, {TT}, {TT}, {TT}, {TT}, int32_t*, {I}, {I}, int, {I}, int, {I}, int,\n'
           '           void*) = sfa_ring_copy_paged_slots;\n'
           '  return a == 0 || b == 0 || c == 0 || d == 0 || SFA_ABI_VERSION != 2;\n'
           '}\n')
    with tempfile.NamedTemporaryFile("w", suffix=".c", delete=False) as f:
        f.write(src)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                        "-fsyntax-only", f.name], capture_output=True, text=True)
    os.unlink(f.name)
    assert r.returncode == 0, r.stderr


# ------------------------------------------------------------------------------------------------ C ABI refusals
@pytest.mark.parametrize("who", list(CALLS))
def test_refusals_of_the_paged_calls(who):
    call = CALLS[who]
    ok = _args()
    # the checks a paged call adds, in their order, before those of its contiguous sibling
    null = dict(ok, wk=None)
    assert call(null) == (-1, "window_k: null tensor descriptor")
    assert call(ok, table=None) == (-1, "page_table: null device pointer")
    for p in (48, 16, 1):
        assert call(_args(p=p)) == (-1, f"{who}: the page size (window_k shape[2] = {p}) must be a power of two and at "
                                        "least 32")
    assert call(ok, stride=0) == (-1, f"{who}: table_stride (0) must be at least 1 (Wc = table_stride * P)")
    assert call(_args(npv=NP + 1)) == (-1, f"window_k and window_v differ in shape[0]: {NP} vs {NP + 1}")
    assert call(_args(npk=0)) == (-1, f"{who}: the page buffers need shape[0] = n_pages in [1, 2^30) (got 0)")
    # a null table is reported before a bad page size, a bad page size before a bad stride
    assert call(_args(p=48), table=None)[1] == "page_table: null device pointer"
    assert call(_args(p=48), stride=0)[1].startswith(f"{who}: the page size")
    # then the sibling's checks, in its order: null device arrays ...
    if who != "ring_copy_paged":
        assert call(ok, state=None) == (-1, "state: null device pointer")
        assert call(ok, slots=None) == (-1, "slots: null device pointer")
        null_cu = "cu_seqlens: null device pointer" if who == "ring_fill_varlen_paged" else "cu_q: null device pointer"
        assert call(ok, cu=None) == (-1, null_cu)
    else:
        assert call(ok, state=None) == (-1, "src_state: null device pointer")
        assert call(ok, slots=None) == (-1, "src_slots: null device pointer")
    # ... one dtype ...
    mixed = dict(ok, kn=_d(1, HKV, T, D, dtype=torch.float16), vn=_d(1, HKV, T, D, dtype=torch.float16))
    if who == "decode_ragged_paged":
        assert call(mixed) == (-1, "q, the cache buffers and k_new / v_new must share one dtype")
    elif who == "ring_commit_ragged_paged":
        assert call(mixed) == (-1, "k_new / v_new and the ring must share one dtype")
    elif who == "ring_fill_varlen_paged":
        assert call(mixed) == (-1, "k / v and the cache buffers must share one dtype")
    # ... and after them what a paged pool serves: no fp32, no other head dim, no generic kernels
    assert call(_args(act=torch.float32)) == (-2, f"{who}: a paged pool serves bf16 / f16 at head dims 64 / 80 / 96 / 128 "
                                                  "(got dtype 0, head dim 64)")
    assert call(_args(d=48)) == (-2, f"{who}: a paged pool serves bf16 / f16 at head dims 64 / 80 / 96 / 128 (got dtype 2, "
                                     "head dim 48)")
    if who == "decode_ragged_paged":
        assert call(ok, flags=N.FLAG_FORCE_GENERIC) == (-2, f"{who}: a paged pool serves bf16 / f16 at head dims 64 / 80 / "
                                                            "96 / 128 (got dtype 2, head dim 64, SFA_FLAG_FORCE_GENERIC)")
        # what is left is the workspace, sized for Wc = table_stride * P: every other check has passed
        rc, err = call(ok)
        need = N.lib().sfa_decode_ragged_workspace_bytes(2, HQ, HKV, T, NS + W, D, N.SFA_DTYPE[torch.bfloat16])
        assert rc == -3 and err.startswith(f"decode_ragged workspace: need {need} bytes"), (rc, err)
    if who == "ring_copy_paged":
        # two pools: equal geometry, P included; n_pages of each is free; no pairs: nothing to do
        assert call(ok, b=_args(p=64)) == (-1, "ring_copy_paged: the pools differ in page size (src 32, dst 64)")
        assert call(ok, b=_args(npk=3), n_pairs=0) == (0, "")
        rc, err = call(ok, b=_args(d=128))
        assert rc == -1 and err.startswith("ring_copy_slots: dst_sink_k must be [S, H_kv, num_sink, D]"), (rc, err)


def test_the_commit_takes_the_pool_size_as_an_argument():
    lib = N.lib()
    a = _args()
    rc = lib.sfa_ring_commit_path_ragged_paged_slots(a["wk"], a["wv"], a["kn"], a["vn"], PTR, PTR, PTR, 2, PTR, PTR, PTR, PER,
                                                     0, None)
    assert rc == -1 and lib.sfa_last_error() == b"pool: the ring needs shape[0] = S >= 1 slots (got 0)"


# ------------------------------------------------------------------------------------------------ Python surface
def _cpu_pool(**kw):
    layer = SinkCacheLayer(NS, W)
    st = layer.init_pool(S, HKV, D, torch.bfloat16, "cpu", page_size=P, **kw)
    assert st.shape == (S, 4) and layer.page_size == P and layer.window_size == W
    assert layer.sink_k.shape == (S, HKV, NS, D)
    assert layer.page_table.dtype == torch.int32 and layer.page_table.shape == (S, PER)
    return layer


def test_init_pool_allocates_pages_and_a_table_of_minus_one():
    layer = _cpu_pool(num_pages=NP)
    assert layer.window_k.shape == layer.window_v.shape == (NP, HKV, P, D) and layer.window_k.dtype == torch.bfloat16
    assert bool((layer.page_table == -1).all()) and layer.num_slots == S
    assert _cpu_pool().window_k.shape == (S * PER, HKV, P, D)              # the default: the full capacity
    given = torch.full((S, PER), -1, dtype=torch.int32)
    assert _cpu_pool(page_table=given).page_table is given
    # the defaults give the contiguous pool
    plain = SinkCacheLayer(NS, W)
    plain.init_pool(S, HKV, D, torch.bfloat16, "cpu")
    assert plain.window_k.shape == (S, HKV, W, D) and plain.page_size is None and plain.page_table is None
    odd = SinkCacheLayer(NS, 320)                                           # Wc itself need not be a power of two
    odd.init_pool(2, HKV, D, torch.float16, "cpu", page_size=64)
    assert odd.page_table.shape == (2, 5) and odd.window_k.shape == (10, HKV, 64, D)
    mk = lambda w=W: SinkCacheLayer(NS, w)
    with pytest.raises(TypeError, match="paged FP8 pool is not served"):
        mk().init_pool(S, HKV, D, torch.float8_e4m3fn, "cpu", page_size=P)
    for bad in (16, 48, 0):
        with pytest.raises(ValueError, match="power of two and at least 32"):
            mk().init_pool(S, HKV, D, torch.bfloat16, "cpu", page_size=bad)
    with pytest.raises(ValueError, match=r"window_size \(80\) must be a multiple of page_size \(32\)"):
        mk(80).init_pool(S, HKV, D, torch.bfloat16, "cpu", page_size=32)
    with pytest.raises(ValueError, match="bfloat16 / float16 at head dims 64 / 80 / 96 / 128"):
        mk().init_pool(S, HKV, D, torch.float32, "cpu", page_size=P)
    with pytest.raises(ValueError, match="bfloat16 / float16 at head dims 64 / 80 / 96 / 128"):
        mk().init_pool(S, HKV, 48, torch.bfloat16, "cpu", page_size=P)
    with pytest.raises(ValueError, match="need page_size"):
        mk().init_pool(S, HKV, D, torch.bfloat16, "cpu", num_pages=4)
    with pytest.raises(ValueError, match=r"int32 \[S, Wc / P\] = \[5, 3\]"):
        mk().init_pool(S, HKV, D, torch.bfloat16, "cpu", page_size=P, page_table=torch.zeros(S, PER + 1, dtype=torch.int32))


def test_the_non_packed_methods_refuse_a_paged_pool():
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
        with pytest.raises(TypeError, match=r"paged pool .*: use the packed calls prefill_slots / ragged_step_dyn / "
                                            r"commit_packed_dyn") as e:
            getattr(layer, name)(*args)
        assert name in str(e.value), (name, str(e.value))
    assert layer.window_k.shape == (NP, HKV, P, D) and not layer._dev_state.any()      # nothing was replaced or moved
    plain = SinkCacheLayer(NS, W)
    plain.init_pool(S, HKV, D, torch.bfloat16, "cpu")
    for f in (lambda: plain.reserve_pages([0], 5), lambda: plain.free_pages([0])):
        with pytest.raises(TypeError, match="needs a paged pool"):
            f()


# ------------------------------------------------------------------------------------------------ the allocator
@pytest.mark.parametrize("wc,p,ns", [(64, 32, 4), (96, 32, 4), (320, 64, 4), (64, 64, 0), (128, 32, 40)])
def test_the_prefix_rule_against_a_walk_of_the_placements(wc, p, ns):
    """every ring slot a prefill, an admission or a token-by-token commit writes, and every slot a read touches, for every
    `seen` in 0 .. 3 Wc, lies in the first pages_needed(ring tokens) <= pages_needed(seen) table entries"""
    assert pages_needed(0, wc, p) == 0 and pages_needed(1, wc, p) == 1 and pages_needed(p + 1, wc, p) == min(2, wc // p)
    assert pages_needed(10 ** 9, wc, p) == wc // p == PR.pages_needed(3 * wc, wc, p)
    for L in range(3 * wc + 1):
        # a prefill / admission of L tokens in one call
        st = PR.prefill_state(L, ns, wc)
        held = L - st[0]
        need = PR.pages_needed(held, wc, p)
        over = -(-ns // p)          # the sinks count in `seen` and not in the ring: one page at most while num_sink <= P
        assert need <= pages_needed(L, wc, p) <= need + over, (L, "tokens_after over-reserves by at most one page")
        touched = set(PR.prefill_ring_slots(L, ns, wc)) | set(PR.read_ring_slots(st))
        assert {s // p for s in touched} == set(range(need)), (L, sorted(touched)[-3:], need)
    for L0 in (0, 1, ns, ns + 1, ns + p - 1, ns + wc - 1, ns + wc, ns + wc + 5):
        # ... and grown from L0 by commits of 1, 7 and Wc + 3 tokens
        for step in (1, 7, wc + 3):
            st, seen = PR.prefill_state(L0, ns, wc), L0
            while seen <= 3 * wc:
                slots, after = PR.commit_ring_slots(st, step, wc)
                held = after[3] - after[0]
                need = PR.pages_needed(held, wc, p)
                assert need <= pages_needed(after[3], wc, p) <= need + over
                touched = set(slots) | set(PR.read_ring_slots(st)) | set(PR.read_ring_slots(after))
                assert {s // p for s in touched} <= set(range(need)), (L0, step, seen, need)
                assert after[1] == min(held, wc) and (after[1] == wc or after[2] == after[1]), after
                st, seen = after, after[3]


def test_reserve_maps_a_prefix_and_exhaustion_changes_nothing():
    layer = _cpu_pool(num_pages=NP)
    tab = layer.page_table
    layer.reserve_pages([3, 1], [40, 1])                       # 40 tokens: two pages; 1 token: one
    assert tab.tolist() == [[-1] * 3, [2, -1, -1], [-1] * 3, [0, 1, -1], [-1] * 3]
    layer.reserve_pages([3, 1], [64, 33])                      # entries already mapped stay; slot 1 grows by one
    assert tab[3].tolist() == [0, 1, -1] and tab[1].tolist() == [2, 3, -1]
    layer.reserve_pages([0], 10 ** 6)                          # capped at Wc / P
    assert tab[0].tolist() == [4, 5, 6] and layer._pages.free_list == []
    before = tab.clone()
    rows = [list(r) for r in layer._pages.rows]
    with pytest.raises(RuntimeError, match=r"^out of pages: need 3, free 0$"):
        layer.reserve_pages([2, 3], [33, 96])                  # 2 for slot 2 and 1 more for slot 3
    assert torch.equal(tab, before) and layer._pages.rows == rows and layer._pages.free_list == []
    layer.reserve_pages([3], 64)                               # still served: nothing new is needed
    with pytest.raises(ValueError, match="once"):
        layer.reserve_pages([1, 1], 5)
    with pytest.raises(ValueError, match="one per slot"):
        layer.reserve_pages([1, 2], [5])


def test_free_and_reserve_again_reuse_the_pages():
    layer = _cpu_pool(num_pages=NP)
    layer.reserve_pages([0, 1, 2], [96, 96, 20])
    assert sorted(layer.page_table[:3].flatten().tolist()) == [-1, -1, 0, 1, 2, 3, 4, 5, 6]
    st = layer._dev_state.clone()
    layer.free_pages([1])
    assert layer.page_table[1].tolist() == [-1, -1, -1] and len(layer._pages.free_list) == 3
    assert torch.equal(layer._dev_state, st)                   # pages and state rows are retired by different calls
    owned = set(layer.page_table[0].tolist()) | {layer.page_table[2, 0].item()}
    layer.reserve_pages([4], 70)
    got = layer.page_table[4].tolist()
    assert len(set(got)) == 3 and not set(got) & owned and set(got) | owned == set(range(NP))
    layer.release_slots([0])                                   # keeps its meaning: state rows only, no page is freed
    assert layer.page_table[0].tolist() != [-1] * 3 and len(layer._pages.free_list) == 0
    assert layer._pages.pool_bytes(HKV, D, 2) == 2 * 7 * HKV * P * D * 2


def test_the_layers_of_a_cache_share_one_table_and_one_allocator():
    cache = SinkAttentionCache(NS, W)
    for l in range(3):
        cache.init_pool(S, HKV, D, torch.bfloat16, "cpu", layer_idx=l, page_size=P, num_pages=NP)
    assert all(cache[l].page_table is cache.page_table for l in range(3))
    assert cache[0].window_k.data_ptr() != cache[1].window_k.data_ptr()      # the pages are each layer's own
    cache.reserve_pages([2, 4], [33, 1])
    assert cache.page_table.tolist() == [[-1] * 3, [-1] * 3, [0, 1, -1], [-1] * 3, [2, -1, -1]]
    cache[1].reserve_pages([0], 1)                                            # through a layer: the same allocator
    assert cache.page_table[0].tolist() == [3, -1, -1] and cache[2]._pages is cache[0]._pages
    cache.free_pages([2])
    assert cache.page_table[2].tolist() == [-1] * 3
    with pytest.raises(ValueError, match="must agree in page_size and num_pages"):
        cache.init_pool(S, HKV, D, torch.bfloat16, "cpu", layer_idx=3, page_size=P, num_pages=NP + 1)
    with pytest.raises(TypeError, match="needs a paged pool"):
        SinkAttentionCache(NS, W).reserve_pages([0], 1)


def test_fork_slots_refuses_pools_that_differ_in_paging():
    a, b = _cpu_pool(num_pages=NP), SinkCacheLayer(NS, W)
    b.init_pool(S, HKV, D, torch.bfloat16, "cpu", page_size=P, num_pages=2 * NP)
    c = SinkCacheLayer(NS, W)
    c.init_pool(S, HKV, D, torch.bfloat16, "cpu")
    with pytest.raises(ValueError, match="differ in (geometry|paging)"):
        a.fork_slots([0], [1], source=c)
    with pytest.raises(RuntimeError, match="MI355X"):          # equal paging, another n_pages: only the device is missing
        a.fork_slots([0], [1], source=b)


# ------------------------------------------------------------------------------------------------ gather
def test_gather_and_scatter_are_inverse_on_the_mapped_pages():
    g = torch.Generator().manual_seed(5)
    pages = torch.randn(NP, HKV, P, 8, generator=g).bfloat16()
    table = torch.tensor([[4, -1, -1], [6, 0, 2], [-1, -1, -1], [5, NP, -1], [1, 3, 2 ** 31 - 1]], dtype=torch.int32)
    win = PR.gather(pages, table)
    assert win.shape == (5, HKV, W, 8) and win.dtype == pages.dtype
    assert torch.equal(win[1, :, P:2 * P], pages[0]) and torch.equal(win[4, :, :P], pages[1])
    for s, j in ((0, 1), (2, 0), (3, 1), (3, 2), (4, 2)):                  # -1, n_pages and INT_MAX read as zeros
        assert not win[s, :, j * P:(j + 1) * P].any(), (s, j)
    back = PR.scatter(win, table, torch.full_like(pages, 7.0))
    assert torch.equal(back, pages)                                         # every page is mapped once here
    ident = torch.arange(6, dtype=torch.int32).reshape(2, 3)
    assert torch.equal(PR.gather(pages, ident), pages[:6].reshape(2, 3, HKV, P, 8).permute(0, 2, 1, 3, 4).reshape(2, HKV, W, 8))
    assert isinstance(PageAllocator(table.clone(), NP, P, W).rows, list)
