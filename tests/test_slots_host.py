"""CPU-only tests of the slot-indexed calls (sfa_decode_ring_step_slots, sfa_decode_ring_multi_slots,
sfa_decode_ring_tree_slots, sfa_ring_commit_slots, sfa_ring_commit_path_slots, sfa_ring_fill_varlen_slots and
SinkCacheLayer's pool: init_pool / prefill_slots / slots= / positions / release_slots): exports, the header, argument checks
that return before any launch, the Python-side checks of a host slot list, the pool's bookkeeping, and the CPU proof that
the stale-content probe of tests/slots_probe.py tells one leaked stale key from a correct read.  No GPU compute: every C
call here fails its checks before a launch."""
import os
import subprocess
import tempfile

import pytest
import torch

from oracle import sink_oracle as O
from sink_attention import SinkAttentionCache, SinkCacheLayer
from slots_probe import stale_probe, stale_rows, true_keys
from test_gpu_decode_multi import TOL

# entry point -> number of arguments include/sfa.h declares
SLOTS = {"sfa_decode_ring_step_slots": 16, "sfa_decode_ring_multi_slots": 17, "sfa_decode_ring_tree_slots": 18,
         "sfa_ring_commit_slots": 8, "sfa_ring_commit_path_slots": 10, "sfa_ring_fill_varlen_slots": 11}


def test_library_exports_the_slots_entry_points_with_the_declared_argument_counts():
    from sink_attention import _native
    lib = _native.lib()
    for name, nargs in SLOTS.items():
        assert hasattr(lib, name), name
        assert len(getattr(lib, name).argtypes) == nargs, name
    assert lib.sfa_abi_version() == 2


def test_header_declares_them_and_compiles_as_c99():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    T = "const sfa_tensor*"
    src = ('#include "sfa.h"\n'
           'int main(void) {\n'
           f'  int (*a)({T}, {T}, {T}, {T}, {T}, {T}, {T}, {T}, const float*, int32_t*, const int32_t*, void*, size_t,\n'
           '           float, unsigned, void*) = sfa_decode_ring_step_slots;\n'
           f'  int (*b)({T}, {T}, {T}, {T}, {T}, {T}, {T}, {T}, const float*, int, int32_t*, const int32_t*, void*,\n'
           '           size_t, float, unsigned, void*) = sfa_decode_ring_multi_slots;\n'
           f'  int (*c)({T}, {T}, {T}, {T}, {T}, {T}, {T}, {T}, const float*, const int32_t*, int64_t, int32_t*,\n'
           '           const int32_t*, void*, size_t, float, unsigned, void*) = sfa_decode_ring_tree_slots;\n'
           f'  int (*d)({T}, {T}, {T}, {T}, const int32_t*, int32_t*, const int32_t*, void*) = sfa_ring_commit_slots;\n'
           f'  int (*e)({T}, {T}, {T}, {T}, const int32_t*, const int32_t*, int64_t, int32_t*, const int32_t*,\n'
           '           void*) = sfa_ring_commit_path_slots;\n'
           f'  int (*f)({T}, {T}, {T}, {T}, {T}, {T}, const int32_t*, int, int32_t*, const int32_t*,\n'
           '           void*) = sfa_ring_fill_varlen_slots;\n'
           '  return a == 0 || b == 0 || c == 0 || d == 0 || e == 0 || f == 0 || SFA_ABI_VERSION != 2;\n'
           '}\n')
    with tempfile.NamedTemporaryFile("w", suffix=".c", delete=False) as f:
        f.write(src)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(root, "include"),
                        "-fsyntax-only", f.name], capture_output=True, text=True)
    os.unlink(f.name)
    assert r.returncode == 0, r.stderr


def _abi_args(S=5, B=2, Hq=8, Hkv=2, n=3, D=64, ns=4, W=16, T=40, dtype=torch.bfloat16):
    """Host tensors: a pool of S slots and the activations of B batch rows.  The C entry points validate them without
    touching the device and return before any launch."""
    from sink_attention import _native as N
    mk = lambda *s: torch.zeros(*s, dtype=dtype)
    t = dict(q=mk(B, Hq, n, D), sk=mk(S, Hkv, ns, D), sv=mk(S, Hkv, ns, D), wk=mk(S, Hkv, W, D), wv=mk(S, Hkv, W, D),
             kn=mk(B, Hkv, n, D), vn=mk(B, Hkv, n, D), o=mk(B, Hq, n, D), q1=mk(B, Hq, 1, D), k1=mk(B, Hkv, 1, D),
             o1=mk(B, Hq, 1, D), kp=mk(1, Hkv, T, D), vp=mk(1, Hkv, T, D))
    return N, t, {k: N.desc(v) for k, v in t.items()}


# host int32 buffers standing in for the device state / counts / offsets / slots: never dereferenced, every call below
# fails its checks first
_HOST = torch.zeros(64, dtype=torch.int32)
P = _HOST.data_ptr()


def _step(N, d, state=P, slots=P, ws=None, ws_bytes=0, **over):
    d = dict(d, **over)
    return N.lib().sfa_decode_ring_step_slots(d["q1"], d["sk"], d["sv"], d["wk"], d["wv"], d["k1"], d["k1"], d["o1"],
                                              None, state, slots, ws, ws_bytes, 0.125, 0, None)


def _multi(N, d, state=P, slots=P, ws=None, ws_bytes=0, commit=1, **over):
    d = dict(d, **over)
    return N.lib().sfa_decode_ring_multi_slots(d["q"], d["sk"], d["sv"], d["wk"], d["wv"], d["kn"], d["vn"], d["o"],
                                               None, commit, state, slots, ws, ws_bytes, 0.125, 0, None)


def _tree(N, d, parent=P, stride=0, state=P, slots=P, ws=None, ws_bytes=0, **over):
    d = dict(d, **over)
    return N.lib().sfa_decode_ring_tree_slots(d["q"], d["sk"], d["sv"], d["wk"], d["wv"], d["kn"], d["vn"], d["o"], None,
                                              parent, stride, state, slots, ws, ws_bytes, 0.125, 0, None)


def _commit(N, d, count=P, state=P, slots=P, **over):
    d = dict(d, **over)
    return N.lib().sfa_ring_commit_slots(d["wk"], d["wv"], d["kn"], d["vn"], count, state, slots, None)


def _commit_path(N, d, count=P, path=P, stride=0, state=P, slots=P, **over):
    d = dict(d, **over)
    return N.lib().sfa_ring_commit_path_slots(d["wk"], d["wv"], d["kn"], d["vn"], count, path, stride, state, slots, None)


def _fill(N, d, cu=P, n_seq=2, state=P, slots=P, **over):
    d = dict(d, **over)
    return N.lib().sfa_ring_fill_varlen_slots(d["sk"], d["sv"], d["wk"], d["wv"], d["kp"], d["vp"], cu, n_seq, state,
                                              slots, None)


CALLS = {"step": _step, "multi": _multi, "tree": _tree, "commit": _commit, "commit_path": _commit_path, "fill": _fill}


@pytest.mark.parametrize("name", list(CALLS))
def test_null_slots_fail_before_any_launch(name):
    N, _, d = _abi_args()
    assert CALLS[name](N, d, slots=None) == -1
    assert b"slots: null device pointer" in N.lib().sfa_last_error()


@pytest.mark.parametrize("name", ["step", "multi", "tree", "fill"])
def test_mismatched_pool_size_between_the_buffers_fails(name):
    N, _, d = _abi_args()
    _, _, d7 = _abi_args(S=7)
    assert CALLS[name](N, d, wk=d7["wk"], wv=d7["wv"]) == -1                 # sink S = 5, ring S = 7
    assert b"pool: sink and window buffers must share shape[0]" in N.lib().sfa_last_error()
    assert CALLS[name](N, d, sv=d7["sv"]) == -1                              # sink_k / sink_v differ
    assert b"differ in shape[0]" in N.lib().sfa_last_error()


@pytest.mark.parametrize("name", ["commit", "commit_path"])
def test_mismatched_ring_buffers_fail(name):
    N, _, d = _abi_args()
    _, _, d7 = _abi_args(S=7)
    assert CALLS[name](N, d, wv=d7["wv"]) == -1 and b"window_k" in N.lib().sfa_last_error()


def test_mismatched_batch_between_the_activations_fails():
    N, _, d = _abi_args()
    lib = N.lib()
    _, _, d3 = _abi_args(B=3)
    assert _step(N, d, k1=d3["k1"]) == -1 and b"share shape[0] = B" in lib.sfa_last_error()
    assert _step(N, d, o1=d3["o1"]) == -1 and b"q and o" in lib.sfa_last_error()
    assert _multi(N, d, kn=d3["kn"], vn=d3["vn"]) == -1 and b"k_new" in lib.sfa_last_error()
    assert _multi(N, d, o=d3["o"]) == -1 and b"q and o" in lib.sfa_last_error()
    assert _tree(N, d, kn=d3["kn"], vn=d3["vn"]) == -1 and b"k_new" in lib.sfa_last_error()
    assert _commit(N, d, vn=d3["vn"]) == -1 and b"k_new" in lib.sfa_last_error()
    assert _commit_path(N, d, vn=d3["vn"]) == -1 and b"k_new" in lib.sfa_last_error()


def test_everything_the_rows_calls_check_is_still_checked_and_b_differs_from_s():
    """B = 2 batch rows on a pool of S = 5: shapes the rows calls refuse are accepted up to the workspace check (the last
    one before a launch); the siblings' own checks still fire."""
    N, _, d = _abi_args()
    lib = N.lib()
    assert _step(N, d) == -3 and b"workspace" in lib.sfa_last_error()
    assert _multi(N, d) == -3 and b"workspace" in lib.sfa_last_error()
    assert _tree(N, d) == -3 and b"workspace" in lib.sfa_last_error()
    need = lib.sfa_decode_multi_workspace_bytes(2, 8, 2, 3, 4 + 16 + 3, 64, 2)      # sized by B = 2, not by S
    assert need > 0 and _multi(N, d, ws=1 << 20, ws_bytes=need - 1) == -3
    assert lib.sfa_decode_ring_multi_rows(d["q"], d["sk"], d["sv"], d["wk"], d["wv"], d["kn"], d["vn"], d["o"], None, 0,
                                          P, None, 0, 0.125, 0, None) == -1             # the rows call wants B == S
    assert _step(N, d, state=None) == -1 and b"state" in lib.sfa_last_error()
    assert _multi(N, d, state=None) == -1 and b"state" in lib.sfa_last_error()
    assert _tree(N, d, parent=None) == -1 and b"parent" in lib.sfa_last_error()
    assert _tree(N, d, stride=2) == -1 and b"parent_bstride" in lib.sfa_last_error()
    assert _commit(N, d, count=None) == -1 and b"count" in lib.sfa_last_error()
    assert _commit_path(N, d, path=None) == -1 and b"path" in lib.sfa_last_error()
    assert _commit_path(N, d, stride=1) == -1 and b"path_bstride" in lib.sfa_last_error()
    _, _, dh = _abi_args(dtype=torch.float16)
    assert _step(N, d, k1=dh["k1"]) == -1 and b"dtype" in lib.sfa_last_error()
    assert _multi(N, d, kn=dh["kn"], vn=dh["vn"]) == -1 and b"dtype" in lib.sfa_last_error()
    assert _commit(N, d, kn=dh["kn"], vn=dh["vn"]) == -1 and b"dtype" in lib.sfa_last_error()
    _, _, d20 = _abi_args(D=20)                                                       # 40-byte rows
    assert _multi(N, d20) == -2
    assert _fill(N, d, cu=None) == -1 and b"cu_seqlens" in lib.sfa_last_error()
    assert _fill(N, d, n_seq=0) == -1 and b"n_seq" in lib.sfa_last_error()
    assert _fill(N, d, kp=d["kn"], vp=d["vn"]) == -1 and b"packed" in lib.sfa_last_error()
    _, _, d0 = _abi_args(S=0)
    assert _multi(N, d0) == -1 and b"pool" in lib.sfa_last_error()
    assert _commit(N, d0) == -1 and b"pool" in lib.sfa_last_error()
    assert _fill(N, d0) == -1 and b"pool" in lib.sfa_last_error()
    assert _step(N, d0) == -1 and b"pool" in lib.sfa_last_error()


# ------------------------------------------------------------------------------------------------ Python surface
def _cpu_pool(S=5, ns=4, W=16, Hkv=2, D=64):
    layer = SinkCacheLayer(ns, W)
    state = layer.init_pool(S, Hkv, D, torch.bfloat16, "cpu")
    return layer, state


def test_init_pool_allocates_the_pool_and_enters_per_sequence_mode():
    layer, state = _cpu_pool()
    assert state.dtype == torch.int32 and state.shape == (5, 4) and not state.any()
    assert layer.sink_k.shape == (5, 2, 4, 64) and layer.window_v.shape == (5, 2, 16, 64)
    assert layer.sink_k.dtype == torch.bfloat16 and layer.num_slots == 5
    assert layer.enable_device_state(per_sequence=True) is state
    _, t, _ = _abi_args()
    for name, call in {"append": lambda: layer.append(t["kn"], t["vn"]), "get_kv": lambda: layer.get_kv(),
                       "decode_step": lambda: layer.decode_step(t["q1"], t["k1"], t["k1"]),
                       "extend_step": lambda: layer.extend_step(t["q"], t["kn"], t["vn"])}.items():
        with pytest.raises(RuntimeError, match=f"{name}.*per-sequence mode"):
            call()
    with pytest.raises(ValueError, match="at least one slot"):
        SinkCacheLayer(4, 16).init_pool(0, 2, 64, torch.bfloat16, "cpu")
    cache = SinkAttentionCache(4, 16)
    st = cache.init_pool(3, 2, 64, torch.float16, "cpu", layer_idx=1)
    assert st.shape == (3, 4) and cache[1].window_k.shape == (3, 2, 16, 64)


def test_positions_and_release_slots_bookkeeping():
    layer, state = _cpu_pool()
    state.copy_(torch.tensor([[4, 3, 3, 7], [4, 16, 0, 30], [2, 0, 0, 2], [4, 16, 5, 100], [1, 0, 0, 1]]))
    assert layer.positions().tolist() == [7, 30, 2, 100, 1]
    assert layer.positions([3, -1, 0]).tolist() == [100, 0, 7]
    assert layer.positions(torch.tensor([4, 4, -1, 1])).tolist() == [1, 1, 0, 30]     # a read may name a slot twice
    layer.release_slots([1, -1, 4])
    assert state.tolist() == [[4, 3, 3, 7], [0, 0, 0, 0], [2, 0, 0, 2], [4, 16, 5, 100], [0, 0, 0, 0]]
    layer.release_slots(torch.tensor([0], dtype=torch.int32))
    assert state[0].tolist() == [0, 0, 0, 0] and layer.positions([0, 3]).tolist() == [0, 100]
    with pytest.raises(ValueError, match="outside the pool of 5 slots"):
        layer.positions([5])
    with pytest.raises(ValueError, match="outside the pool of 5 slots"):
        layer.release_slots([-2])
    cache = SinkAttentionCache(4, 16)
    st1 = cache.init_pool(3, 2, 64, torch.bfloat16, "cpu", layer_idx=1)      # layer 0 exists but holds no pool
    st1.fill_(9)
    cache.release_slots([2])
    assert st1.tolist() == [[9] * 4, [9] * 4, [0] * 4]


def test_a_host_slot_list_is_checked_before_any_gpu_work():
    """Every call below gets CPU tensors: the slot list is refused first; only a valid list reaches the no-CPU-fallback
    refusal."""
    _, t, _ = _abi_args()
    layer, state = _cpu_pool()
    before = state.clone()
    cnt = torch.tensor([1, 2], dtype=torch.int32)
    path = torch.tensor([0, 1, 2], dtype=torch.int32)
    parent = torch.tensor([-1, 0, 0], dtype=torch.int32)
    calls = {
        "decode_step_dyn": lambda s: layer.decode_step_dyn(t["q1"], t["k1"], t["k1"], slots=s),
        "extend_attention_dyn": lambda s: layer.extend_attention_dyn(t["q"], t["kn"], t["vn"], slots=s),
        "extend_step_dyn": lambda s: layer.extend_step_dyn(t["q"], t["kn"], t["vn"], slots=s),
        "extend_attention_tree_dyn": lambda s: layer.extend_attention_tree_dyn(t["q"], t["kn"], t["vn"], parent, slots=s),
        "commit_dyn": lambda s: layer.commit_dyn(t["kn"], t["vn"], cnt, slots=s),
        "commit_path_dyn": lambda s: layer.commit_path_dyn(t["kn"], t["vn"], path, cnt, slots=s),
        "prefill_slots": lambda s: layer.prefill_slots(t["kp"], t["vp"], [0, 10, 40], s),
    }
    writes = ("decode_step_dyn", "extend_step_dyn", "commit_dyn", "commit_path_dyn", "prefill_slots")
    for name, call in calls.items():
        with pytest.raises(ValueError, match="outside the pool of 5 slots"):
            call([0, 5])                                        # the pool is smaller than the slot
        with pytest.raises(ValueError, match="B = 2 entries"):
            call([0, 1, 2])
        if name in writes:
            with pytest.raises(ValueError, match="named twice"):
                call([3, 3])
        else:                                                   # a call that writes nothing may name a slot twice
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                call([3, 3])
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call([4, -1])
    assert torch.equal(state, before)
    shared = SinkCacheLayer(4, 16)
    kv = torch.zeros(2, 2, 9, 64, dtype=torch.bfloat16)
    shared.append(kv, kv)
    shared.enable_device_state()
    with pytest.raises(RuntimeError, match="per-sequence"):
        shared.extend_attention_dyn(t["q"], t["kn"], t["vn"], slots=[0, 1])
    with pytest.raises(RuntimeError, match="init_pool"):
        SinkCacheLayer(4, 16).prefill_slots(t["kp"], t["vp"], [0, 10, 40], [0, 1])
    cache = SinkAttentionCache(4, 16)
    cache.init_pool(3, 2, 64, torch.bfloat16, "cpu")
    with pytest.raises(ValueError, match="outside the pool of 3 slots"):
        cache.prefill_slots(t["kp"], t["vp"], [0, 10, 40], [0, 3], layer_idx=0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cache.prefill_slots(t["kp"], t["vp"], [0, 10, 40], [0, 1], layer_idx=0)


# --------------------------------------------------------------------------- the stale-content probe, proved on the CPU
TOL_CACHE = max(TOL.values())   # the table of tests/test_gpu_decode_multi.py; its largest entry is bf16's
PROBE = dict(Hq=4, Hkv=2, D=64, ns=4, W=16, n=3)     # the geometry tests/test_gpu_slots.py runs
PROBE_PROMPTS = (2, 9)        # sink not full (ring empty); sink full, ring partly filled


@pytest.mark.parametrize("L", PROBE_PROMPTS)
def test_one_leaked_stale_key_exceeds_the_tolerance_tenfold(L):
    """fp64 oracle over the keys a reused slot really holds against the same oracle that also sees ONE stale key, for
    every stale row the new state leaves behind: the worst row over the n verify queries and the step moves by at least
    10 x the bf16 tolerance (measured: the smallest factor is printed; it is in the hundreds)."""
    pr = stale_probe(L=L, dtype=torch.bfloat16, seed=3, **PROBE)
    n, ns, W = PROBE["n"], PROBE["ns"], PROBE["W"]
    rows = stale_rows(ns, W, L)
    assert TOL_CACHE == TOL[torch.bfloat16]
    assert len(rows) == ns + W - L and L + n + 1 <= W
    smallest = float("inf")
    for j in rows:
        worst = 0.0
        for t in range(n + 1):
            k, v = true_keys(pr, t)
            ref = O.decode_dense(pr["q"][:, :, t:t + 1], k, v, pr["s_aux"])
            leak = O.decode_dense(pr["q"][:, :, t:t + 1], torch.cat([k, pr["stale_k"][:, :, j:j + 1]], dim=2),
                                  torch.cat([v, pr["stale_v"][:, :, j:j + 1]], dim=2), pr["s_aux"])
            worst = max(worst, (ref - leak).abs().max().item())
        smallest = min(smallest, worst / TOL_CACHE)
    print(f"L = {L}: smallest factor over {len(rows)} stale rows = {smallest:.1f}")
    assert smallest >= 10, smallest

