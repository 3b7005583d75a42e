"""CPU-only tests of the slot copy (sfa_ring_copy_slots, SinkCacheLayer.fork_slots / SinkAttentionCache.fork_slots and
sink_attention.beam_fork_plan): the export, the header, every refusal of the C entry point - each returns before any
launch, host tensors stand in for device memory as in tests/test_slots_host.py -, the order of the checks, the
Python-side checks of host slot lists, and the beam bookkeeping simulated on lists.  No GPU compute."""
import os
import random
import subprocess
import tempfile

import pytest
import torch

from sink_attention import SinkAttentionCache, SinkCacheLayer, beam_fork_plan

NAMES = ("ssk", "ssv", "swk", "swv", "dsk", "dsv", "dwk", "dwv")
ARG = dict(zip(NAMES, ("src_sink_k", "src_sink_v", "src_window_k", "src_window_v",
                       "dst_sink_k", "dst_sink_v", "dst_window_k", "dst_window_v")))


def test_library_exports_the_copy_with_the_declared_argument_count():
    from sink_attention import _native
    lib = _native.lib()
    assert hasattr(lib, "sfa_ring_copy_slots")
    assert len(lib.sfa_ring_copy_slots.argtypes) == 14
    assert lib.sfa_abi_version() == 2


def test_header_declares_it_and_compiles_as_c99():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    T = "const sfa_tensor*"
    src = ('#include "sfa.h"\n'
           'int main(void) {\n'
           f'  int (*a)({T}, {T}, {T}, {T}, const int32_t*, {T}, {T}, {T}, {T}, int32_t*, const int32_t*,\n'
           '           const int32_t*, int, void*) = sfa_ring_copy_slots;\n'
           '  return a == 0 || SFA_ABI_VERSION != 2;\n'
           '}\n')
    with tempfile.NamedTemporaryFile("w", suffix=".c", delete=False) as f:
        f.write(src)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(root, "include"),
                        "-fsyntax-only", f.name], capture_output=True, text=True)
    os.unlink(f.name)
    assert r.returncode == 0, r.stderr


def _pools(S_src=5, S_dst=3, Hkv=2, D=64, ns=4, W=16, dtype=torch.bfloat16):
    """Host tensors of a source pool and a destination pool; the C entry point validates the descriptors without
    touching the memory and every call below returns before a launch."""
    from sink_attention import _native as N
    mk = lambda S, n: torch.zeros(S, Hkv, n, D, dtype=dtype)
    t = dict(ssk=mk(S_src, ns), ssv=mk(S_src, ns), swk=mk(S_src, W), swv=mk(S_src, W),
             dsk=mk(S_dst, ns), dsv=mk(S_dst, ns), dwk=mk(S_dst, W), dwv=mk(S_dst, W))
    return N, t, {k: N.desc(v) for k, v in t.items()}


# host int32 memory standing in for the device state rows and slot arrays: never dereferenced
_HOST = torch.zeros(64, dtype=torch.int32)
P = _HOST.data_ptr()


def _copy(N, d, src_state=P, dst_state=P, src_slots=P, dst_slots=P, n_pairs=2, **over):
    d = dict(d, **over)
    rc = N.lib().sfa_ring_copy_slots(d["ssk"], d["ssv"], d["swk"], d["swv"], src_state, d["dsk"], d["dsv"], d["dwk"],
                                     d["dwv"], dst_state, src_slots, dst_slots, n_pairs, None)
    return rc, N.lib().sfa_last_error().decode()


def test_zero_pairs_return_ok_without_a_launch():
    N, _, d = _pools()
    assert _copy(N, d, n_pairs=0) == (0, "")
    assert _copy(N, d, n_pairs=0, dsk=d["ssk"], dsv=d["ssv"], dwk=d["swk"], dwv=d["swv"]) == (0, "")     # one pool


@pytest.mark.parametrize("name", NAMES)
def test_a_null_descriptor_is_refused_by_name(name):
    N, _, d = _pools()
    assert _copy(N, d, **{name: None}) == (-1, f"{ARG[name]}: null tensor descriptor")


@pytest.mark.parametrize("name", ["src_state", "dst_state", "src_slots", "dst_slots"])
def test_a_null_device_array_is_refused_by_name(name):
    N, _, d = _pools()
    assert _copy(N, d, **{name: None}) == (-1, f"{name}: null device pointer")


def test_a_negative_pair_count_is_refused():
    N, _, d = _pools()
    assert _copy(N, d, n_pairs=-1) == (-1, "n_pairs must be >= 0 (got -1)")


@pytest.mark.parametrize("name", NAMES[1:])
def test_one_dtype_across_the_eight_buffers(name):
    N, _, d = _pools()
    _, _, dh = _pools(dtype=torch.float16)
    rc, msg = _copy(N, d, **{name: dh[name]})
    assert rc == -1 and msg.startswith(f"ring_copy_slots: {ARG[name]} and src_sink_k differ in dtype"), msg
    rc, msg = _copy(N, dh, ssk=d["ssk"])                       # the first buffer is the odd one: the second reports
    assert rc == -1 and "src_sink_v and src_sink_k differ in dtype" in msg, msg


@pytest.mark.parametrize("what,other", [("H_kv", dict(Hkv=4)), ("num_sink", dict(ns=8)), ("Wc", dict(W=32)),
                                        ("D", dict(D=128))])
def test_the_two_pools_must_share_their_geometry(what, other):
    N, _, d = _pools()
    _, _, o = _pools(**other)
    dst = {k: o[k] for k in ("dsk", "dsv", "dwk", "dwv")}
    rc, msg = _copy(N, d, **dst)
    first = "dst_window_k" if what == "Wc" else "dst_sink_k"   # the first buffer, in argument order, that differs
    assert rc == -1 and msg.startswith(f"ring_copy_slots: {first} must be [S, H_kv, "), msg
    # ... and within one pool (a single buffer of another geometry)
    rc, msg = _copy(N, d, swv=N.desc(torch.zeros(5, 2, 16, 32, dtype=torch.bfloat16)))
    assert rc == -1 and msg.startswith("ring_copy_slots: src_window_v must be [S, H_kv, Wc, D]"), msg


def test_the_four_buffers_of_a_pool_share_s_and_s_is_free_between_the_pools():
    N, _, d = _pools(S_src=5, S_dst=3)
    _, _, d7 = _pools(S_src=7, S_dst=7)
    rc, msg = _copy(N, d, swk=d7["swk"], swv=d7["swv"])
    assert rc == -1 and msg.startswith("pool: the src sink and window buffers must share shape[0]"), msg
    rc, msg = _copy(N, d, dsv=d7["dsv"])
    assert rc == -1 and msg.startswith("pool: the dst sink and window buffers must share shape[0]"), msg
    _, _, d0 = _pools(S_dst=0)
    rc, msg = _copy(N, d0)
    assert rc == -1 and msg.startswith("pool: the dst"), msg
    # S_src = 5 and S_dst = 3 pass every shape check: the next refusal is the alignment one
    off = torch.zeros(3 * 2 * 16 * 64 + 1, dtype=torch.bfloat16)[1:].view(3, 2, 16, 64)
    assert _copy(N, d, dwk=N.desc(off)) == (-1, "ring_copy_slots: rows of every tensor must be 16-byte aligned")


def test_rows_are_16_byte_multiples_with_unit_last_stride():
    N, _, d = _pools()
    _, _, d20 = _pools(D=20)                                   # 40-byte rows
    rc, msg = _copy(N, d20)
    assert rc == -1 and msg == "ring_copy_slots: K/V rows must be a multiple of 16 bytes (head dim 20)", msg
    strided = torch.zeros(5, 2, 16, 128, dtype=torch.bfloat16)[..., ::2]
    rc, msg = _copy(N, d, swk=N.desc(strided))
    assert rc == -1 and msg == "src_window_k: last-dim stride must be 1 (got 2)", msg
    padded = torch.zeros(3, 2, 4, 68, dtype=torch.bfloat16)[..., :64]          # row stride 136 bytes
    rc, msg = _copy(N, d, dsk=N.desc(padded))
    assert rc == -1 and msg == "ring_copy_slots: rows of every tensor must be 16-byte aligned", msg


def test_of_two_defects_the_earlier_check_reports():
    N, _, d = _pools()
    _, _, dh = _pools(dtype=torch.float16)
    _, _, dw = _pools(W=32)
    padded = N.desc(torch.zeros(3, 2, 4, 68, dtype=torch.bfloat16)[..., :64])
    order = [
        (dict(dwv=None, src_state=None), "dst_window_v: null tensor descriptor"),
        (dict(ssk=None, dwv=None), "src_sink_k: null tensor descriptor"),
        (dict(src_slots=None, dst_state=None), "dst_state: null device pointer"),
        (dict(dst_slots=None, n_pairs=-3), "dst_slots: null device pointer"),
        (dict(n_pairs=-3, ssv=dh["ssv"]), "n_pairs must be >= 0 (got -3)"),
        (dict(ssv=dh["ssv"], dwk=dw["dwk"], dwv=dw["dwv"]), "ring_copy_slots: src_sink_v and src_sink_k differ in dtype"),
        (dict(dwk=dw["dwk"], dwv=dw["dwv"], dsk=padded), "ring_copy_slots: dst_window_k must be [S, H_kv, Wc, D]"),
    ]
    for over, msg in order:
        rc, got = _copy(N, d, **over)
        assert rc == -1 and got.startswith(msg), (over.keys(), got)
    _, _, d7 = _pools(S_dst=7)
    rc, got = _copy(N, d, dsv=d7["dsv"], dsk=padded)
    assert rc == -1 and got.startswith("pool: the dst"), got


# ------------------------------------------------------------------------------------------------ Python surface
def _cpu_pool(S=5, ns=4, W=16, Hkv=2, D=64, dtype=torch.bfloat16):
    layer = SinkCacheLayer(ns, W)
    layer.init_pool(S, Hkv, D, dtype, "cpu")
    return layer


def test_host_lists_are_checked_before_any_gpu_work():
    """CPU pools: a bad list is refused first; only a valid call reaches the no-CPU-fallback refusal."""
    a, b = _cpu_pool(S=5), _cpu_pool(S=3)
    a._dev_state.fill_(3)
    before = a._dev_state.clone()
    with pytest.raises(ValueError, match="must pair up, got 2 and 3"):
        a.fork_slots([0, 1], [2, 3, 4])
    with pytest.raises(ValueError, match="must pair up"):
        a.fork_slots(torch.tensor([0]), [2, 3])
    with pytest.raises(ValueError, match=r"slots \[5\] outside the pool of 5 slots"):
        a.fork_slots([0, 5], [1, 2])
    with pytest.raises(ValueError, match=r"slots \[-2\] outside the pool of 5 slots"):
        a.fork_slots([0, 1], [-2, 2])
    with pytest.raises(ValueError, match=r"slots \[3\] outside the pool of 3 slots"):
        a.fork_slots([3], [0], source=b)                       # src is checked against the source's pool ...
    with pytest.raises(ValueError, match=r"slots \[4\] outside the pool of 3 slots"):
        b.fork_slots([4], [4], source=a)                       # ... and dst against this one
    with pytest.raises(ValueError, match="names a destination twice"):
        a.fork_slots([0, 1], [2, 2])
    with pytest.raises(ValueError, match="names a destination twice"):
        a.fork_slots([0, 0, 1], [2, 3, 2], source=_cpu_pool(S=5))
    with pytest.raises(ValueError, match=r"slots \[1\] are a destination and the source of another pair"):
        a.fork_slots([0, 1], [1, 2])
    # what the kernel skips is not a live pair: -1 on either side, s == d in one pool
    for src, dst in (([0, 0, 0], [1, 2, 3]), ([0, -1, 0], [1, 1, -1]), ([2, 2], [2, 3]), ([0, 1], [1, -1]), ([], [])):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            a.fork_slots(src, dst)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        a.fork_slots([0, 1], [1, 2], source=_cpu_pool(S=5))    # two pools: a destination may carry a source's number
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        a.fork_slots(torch.tensor([0, 1]), torch.tensor([3, 4], dtype=torch.int32))
    assert torch.equal(a._dev_state, before)


def test_fork_slots_needs_two_pools_of_one_geometry_dtype_and_kind():
    a = _cpu_pool()
    with pytest.raises(RuntimeError, match="fork_slots needs a pool: call init_pool first"):
        SinkCacheLayer(4, 16).fork_slots([0], [1])
    with pytest.raises(RuntimeError, match="fork_slots needs a pool: call init_pool first"):
        a.fork_slots([0], [1], source=SinkCacheLayer(4, 16))
    with pytest.raises(TypeError, match="differ in dtype"):
        a.fork_slots([0], [1], source=_cpu_pool(dtype=torch.float16))
    for other in (dict(W=32), dict(ns=8), dict(Hkv=4), dict(D=128)):
        with pytest.raises(ValueError, match="differ in geometry"):
            a.fork_slots([0], [1], source=_cpu_pool(**other))
    with pytest.raises(TypeError, match="source must be a SinkCacheLayer"):
        a.fork_slots([0], [1], source=SinkAttentionCache(4, 16))
    cache, other = SinkAttentionCache(4, 16), SinkAttentionCache(4, 16)
    cache.init_pool(5, 2, 64, torch.bfloat16, "cpu", layer_idx=1)          # layer 0 exists and holds no pool: skipped
    with pytest.raises(ValueError, match="outside the pool of 5 slots"):
        cache.fork_slots([0], [7])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cache.fork_slots([0], [1])
    with pytest.raises(TypeError, match="source must be a SinkAttentionCache"):
        cache.fork_slots([0], [1], source=a)
    with pytest.raises(ValueError, match="source has no layer 1"):
        cache.fork_slots([0], [1], source=other)
    other.init_pool(3, 2, 64, torch.float16, "cpu", layer_idx=1)
    with pytest.raises(TypeError, match="differ in dtype"):
        cache.fork_slots([0], [1], source=other)


# ------------------------------------------------------------------------------------------------ beam_fork_plan
def test_identity_beams_fork_nothing_and_free_nothing():
    assert beam_fork_plan([0, 1, 2, 3], [5, 2, 7, 0], [1, 3]) == ([5, 2, 7, 0], [], [], [])
    assert beam_fork_plan([2, 0, 3, 1], [5, 2, 7, 0], []) == ([7, 5, 0, 2], [], [], [])          # a permutation too


def test_one_beam_taken_by_all_rows_forks_b_minus_1_times_from_one_source():
    new, src, dst, freed = beam_fork_plan([2, 2, 2, 2], [5, 2, 7, 0], [1, 3, 4, 6])
    assert new == [7, 1, 3, 4] and src == [7, 7, 7] and dst == [1, 3, 4] and freed == [5, 2, 0]


def test_dead_beams_are_freed_and_an_exhausted_free_list_raises():
    new, src, dst, freed = beam_fork_plan(torch.tensor([0, 0, 3, 3]), (4, 5, 6, 7), [0, 1])
    assert (new, src, dst, freed) == ([4, 0, 7, 1], [4, 7], [0, 1], [5, 6])
    with pytest.raises(ValueError, match="free_slots ran out"):
        beam_fork_plan([0, 0, 3, 3], [4, 5, 6, 7], [0])
    with pytest.raises(ValueError, match="one entry per row"):
        beam_fork_plan([0, 0, 3], [4, 5, 6, 7], [0])
    with pytest.raises(ValueError, match=r"outside \[0, 4\)"):
        beam_fork_plan([0, 4, 3, 3], [4, 5, 6, 7], [0])


def test_random_beam_steps_simulated_on_lists_keep_every_rows_history():
    """A pool as a list of histories: fork = copy, release = clear.  After every step the slot of row b holds the
    history of its parent; no pair's destination is a live slot, a source or named twice (what fork_slots leaves
    undefined); the slot accounting closes."""
    rng = random.Random(11)
    S, B = 12, 5
    for trial in range(50):
        order = list(range(S))
        rng.shuffle(order)
        slots, free = order[:B], order[B:]
        pool = [None] * S
        for b, s in enumerate(slots):
            pool[s] = [("prompt", b)]
        for step in range(8):
            beam_idx = [rng.randrange(B) for _ in range(B)] if rng.random() < 0.8 else list(range(B))
            want = [list(pool[slots[p]]) for p in beam_idx]
            new, src, dst, freed = beam_fork_plan(beam_idx, slots, free)
            assert len(set(dst)) == len(dst) and not set(dst) & set(src) and not set(dst) & set(slots)
            assert all(d in free for d in dst) and set(src) <= set(slots)
            for s, d in zip(src, dst):                         # fork_slots(src, dst): any order, no pair reads a dst
                pool[d] = list(pool[s])
            for s in freed:                                    # release_slots(freed)
                pool[s] = None
            free = [s for s in free if s not in dst] + freed
            slots = new
            assert len(set(slots)) == B and not set(slots) & set(free) and len(free) == S - B
            for b in range(B):
                assert pool[slots[b]] == want[b], (trial, step, b)
                pool[slots[b]].append((step, b))               # the row's next token
            assert sum(p is not None for p in pool) == B
