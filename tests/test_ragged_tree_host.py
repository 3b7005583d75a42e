"""Host-side checks of the packed tree step and the packed commit (sfa_decode_ring_ragged_tree_slots,
sfa_ring_commit_path_ragged_slots; SinkCacheLayer.ragged_step_dyn(parent=, commit_seq=) / commit_packed_dyn;
spec_tree.packed_tree_depth / greedy_accept_packed): exports and declarations, the refusals of both entry points, the
unchanged workspace query, the Python surface through a stub library, the packed torch helpers against the per-tree
ones, and a CPU mask model of the packed tree step - checked against a replay of append() along every path, and shown to
move a probe row of tests/test_gpu_ragged_tree.py::test_mask_edge_probes tenfold under a one-key error."""
import contextlib
import copy
import ctypes
import functools
import inspect
import os
import random
import subprocess
import tempfile

import pytest
import torch

import probe_inputs as P
from sink_attention import SinkAttentionCache, SinkCacheLayer, spec_tree
from test_probe_inputs import factors, masked_attention
from test_ragged_step_host import _abi_args
from test_tree_host import depths, path_to, random_tree
from util import DECODE_TOL

HKV, NS = 2, 4
MAX_TREE = 64
LENGTHS = [1, 7, 0, 16, 33, 64, 70]      # 64: the last tree length; 70 ignores `parent`; an empty sequence


# ------------------------------------------------------------------------------------------------ trees of a pack
def chain(n):
    return list(range(-1, n - 1))


def star(n):
    return [-1] * n


def binary(n):
    return [(u - 1) // 2 if u else -1 for u in range(n)]


def comb(n):
    """a spine 0, 2, 4, ... with one leaf per spine node: depth n / 2 (32 at n = 64), so that a ring of 16 clips the
    ancestors inside the chunk"""
    return [-1 if u == 0 else (u - 2 if u % 2 == 0 else u - 1) for u in range(n)]


def rand_tree(n, i, forest=True):
    return random_tree(random.Random(P.TREE_RNG_SEED + i), n, forest=forest)


def corrupt(parent, seed):
    """(array with some entries outside [-1, u), the tree the device reads: those entries as roots)"""
    rng = random.Random(seed)
    raw, seen = list(parent), list(parent)
    for u in range(len(parent)):
        if rng.random() < 0.3:
            raw[u] = rng.choice([u, u + 1, u + 7, -2, -100, 1 << 20])
            seen[u] = -1
    return raw, seen


def read_as(parent, n):
    """the tree a sequence of n tokens is attended with: its entries with the kernels' rule, a chain beyond 64 tokens"""
    if n > MAX_TREE:
        return chain(n)
    return [p if -1 <= p < u else -1 for u, p in enumerate(parent)]


def packed_valid(L, sl, W, parent, n):
    """The CPU mask model of one sequence of the packed tree step: bool [n, L + n] over cat(history, chunk) for a slot
    whose history holds L tokens (the first sl of them in the sink rows).  Node u at depth d sees the sinks, history
    position j iff j >= L + d - W + 1, and chunk node v iff v is u or an ancestor and d[u] - d[v] <= W - 1."""
    par = read_as(parent, n)
    d = depths(par)
    m = torch.zeros(n, L + n, dtype=torch.bool)
    for u in range(n):
        m[u, :sl] = True
        m[u, max(sl, L + d[u] - W + 1):L] = True
        for v in path_to(par, u):
            if d[u] - d[v] <= W - 1:
                m[u, L + v] = True
    return m


# ------------------------------------------------------------------------------------------------ exports, header
def test_library_exports_and_header_declare_both_calls():
    from sink_attention import _native
    lib = _native.lib()
    assert len(lib.sfa_decode_ring_ragged_tree_slots.argtypes) == 21
    assert len(lib.sfa_ring_commit_path_ragged_slots.argtypes) == 11
    assert lib.sfa_abi_version() == 2 and _native.ABI_VERSION == 2
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    T = "const sfa_tensor*"
    src = ('#include "sfa.h"\n'
           'int main(void) {\n'
           f'  int (*a)({T}, {T}, {T}, {T}, {T}, {T}, {T}, {T}, const float*, const int32_t*, const int32_t*, int, int32_t*,\n'
           '           const int32_t*, const int32_t*, int, void*, size_t, float, unsigned, void*) =\n'
           '      sfa_decode_ring_ragged_tree_slots;\n'
           f'  int (*b)({T}, {T}, {T}, {T}, const int32_t*, const int32_t*, const int32_t*, int, int32_t*, const int32_t*,\n'
           '           void*) = sfa_ring_commit_path_ragged_slots;\n'
           '  return a == 0 || b == 0 || SFA_ABI_VERSION != 2;\n'
           '}\n')
    with tempfile.NamedTemporaryFile("w", suffix=".c", delete=False) as f:
        f.write(src)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(root, "include"),
                        "-fsyntax-only", f.name], capture_output=True, text=True)
    os.unlink(f.name)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("cls", [SinkCacheLayer, SinkAttentionCache])
def test_python_surface_has_the_keywords_and_the_packed_commit(cls):
    p = inspect.signature(cls.ragged_step_dyn).parameters
    assert p["parent"].default is None and p["commit_seq"].default is None
    assert p["admit"].default is False and p["commit"].default is True
    p = inspect.signature(cls.commit_packed_dyn).parameters
    assert p["path"].default is None and "count" in p and "cu_q" in p and "slots" in p


# ------------------------------------------------------------------------------------------------ C ABI refusals
def _ptr(x):
    return ctypes.c_void_p(0x1000) if x else None


def _step(N, d, n_seq=3, state=1, slots=1, cu=1, parent=1, commit_seq=1, ws=None, ws_bytes=0, scale=0.125, flags=0, **over):
    """non-null values stand for device pointers: every call here returns before a launch, so none is read"""
    d = dict(d, **over)
    lib = N.lib()
    rc = lib.sfa_decode_ring_ragged_tree_slots(d["q"], d["sk"], d["sv"], d["wk"], d["wv"], d["kn"], d["vn"], d["o"], None,
                                               _ptr(parent), _ptr(commit_seq), 1, _ptr(state), _ptr(slots), _ptr(cu), n_seq,
                                               ws, ws_bytes, scale, flags, None)
    return rc, lib.sfa_last_error()


def _old_step(N, d, n_seq=3, state=1, slots=1, cu=1, ws=None, ws_bytes=0, scale=0.125, flags=0, **over):
    d = dict(d, **over)
    lib = N.lib()
    rc = lib.sfa_decode_ring_ragged_slots(d["q"], d["sk"], d["sv"], d["wk"], d["wv"], d["kn"], d["vn"], d["o"], None, 1,
                                          _ptr(state), _ptr(slots), _ptr(cu), n_seq, ws, ws_bytes, scale, flags, None)
    return rc, lib.sfa_last_error()


def test_the_tree_step_refuses_what_the_ragged_step_refuses_with_the_same_text():
    N, t, d = _abi_args()
    _, _, d2 = _abi_args(B=2)
    _, _, d3 = _abi_args(T=13)
    _, _, d4 = _abi_args(S=4)
    _, _, d5 = _abi_args(Hq=6, Hkv=4)
    _, _, d6 = _abi_args(D=20)
    _, t7, _ = _abi_args(D=72)
    half = lambda *s: N.desc(torch.zeros(*s, dtype=torch.float16))
    need = N.lib().sfa_decode_ragged_workspace_bytes(3, 8, 2, 12, 20, 64, 2)
    cases = [(-1, b"state: null device pointer", dict(state=0)), (-1, b"slots: null device pointer", dict(slots=0)),
             (-1, b"cu_q: null device pointer", dict(cu=0)), (-1, b"n_seq (0) must be at least 1", dict(n_seq=0)),
             (-1, b"[1, H, T, D]", dict(d2)), (-1, b"k_new", dict(kn=d3["kn"], vn=d3["vn"])), (-1, b"", dict(o=d3["o"])),
             (-1, b"pool", dict(wk=d4["wk"], wv=d4["wv"])), (-1, b"divisible", dict(d5)), (-2, b"head dim", dict(d6)),
             (-1, b"aligned", dict(q=N.desc(t7["q"][..., 4:68]))),
             (-1, b"dtype", dict(kn=half(1, 2, 12, 64), vn=half(1, 2, 12, 64))), (-1, b"scale", dict(scale=float("nan"))),
             (-3, b"workspace", dict()), (-3, b"workspace", dict(ws=ctypes.c_void_p(0x10000), ws_bytes=need - 1)),
             (-3, b"workspace", dict(ws=ctypes.c_void_p(0x10010), ws_bytes=need))]
    for want, word, kw in cases:
        for flags in (0, N.FLAG_RAGGED_ADMIT):
            for extra in (dict(), dict(parent=0), dict(commit_seq=0), dict(parent=0, commit_seq=0)):   # both may be null
                got = _step(N, d, flags=flags, **kw, **extra)
                assert got[0] == want and word in got[1], (kw.keys(), extra, got)
                assert got == _old_step(N, d, flags=flags, **kw), (kw.keys(), extra, got)


def _commit(N, d, count=1, path=1, cu=1, n_seq=3, state=1, slots=1, **over):
    d = dict(d, **over)
    lib = N.lib()
    rc = lib.sfa_ring_commit_path_ragged_slots(d["wk"], d["wv"], d["kn"], d["vn"], _ptr(count), _ptr(path), _ptr(cu), n_seq,
                                               _ptr(state), _ptr(slots), None)
    return rc, lib.sfa_last_error()


def test_the_packed_commit_refuses_bad_arguments_before_any_launch():
    N, t, d = _abi_args()
    for kw, word in [(dict(count=0), b"count: null device pointer"), (dict(cu=0), b"cu_q: null device pointer"),
                     (dict(state=0), b"state: null device pointer"), (dict(slots=0), b"slots: null device pointer"),
                     (dict(n_seq=0), b"n_seq (0) must be at least 1"), (dict(n_seq=-3), b"n_seq (-3) must be at least 1")]:
        for path in (0, 1):             # a null path is the identity, never an error
            rc, err = _commit(N, d, path=path, **kw)
            assert rc == -1 and word in err, (kw, rc, err)
    _, _, d2 = _abi_args(B=2)
    rc, err = _commit(N, d, kn=d2["kn"], vn=d2["vn"])
    assert rc == -1 and b"packed [1, H_kv, T, D] (got shape[0] = 2)" in err, err
    _, _, d3 = _abi_args(T=13)
    rc, err = _commit(N, d, vn=d3["vn"])
    assert rc == -1 and err == b"k_new and v_new differ in shape[2]: 12 vs 13", err                       # shared T
    half = N.desc(torch.zeros(1, 2, 12, 64, dtype=torch.float16))
    rc, err = _commit(N, d, kn=half, vn=half)
    assert rc == -1 and b"k_new / v_new and the ring must share one dtype" in err, err
    _, _, d5 = _abi_args(Hkv=4, Hq=8)
    rc, err = _commit(N, d, kn=d5["kn"], vn=d5["vn"])
    assert rc == -1 and b"like the ring" in err, err
    _, t7, _ = _abi_args(D=72)
    off = N.desc(t7["kn"][..., 4:68])
    rc, err = _commit(N, d, kn=off, vn=off)
    assert rc == -1 and b"ring_commit: rows of every tensor must be 16-byte aligned" in err, err
    rc, err = _commit(N, d, wk=None)
    assert rc == -1 and err == b"window_k: null tensor descriptor", err
    # the same defects through the existing slots commit give the same text (the shared checks)
    lib = N.lib()
    rc2 = lib.sfa_ring_commit_slots(d["wk"], d["wv"], half, half, _ptr(1), _ptr(1), _ptr(1), None)
    assert rc2 == -1 and b"k_new / v_new and the ring must share one dtype" in lib.sfa_last_error()


def test_the_workspace_query_is_unchanged():
    """decode_ragged_workspace restated (csrc/sfa_decode_multi.hip): the tree instances take the plan, the grid and the
    partials of the ragged ones"""
    from sink_attention import _native
    ws = _native.lib().sfa_decode_ragged_workspace_bytes
    al, cd = (lambda x: (x + 255) & ~255), (lambda a, b: -(-a // b))
    for n_seq, Hq, Hkv, T, nkv, D in [(7, 16, 2, 200, 20, 64), (7, 2, 2, 200, 52, 128), (3, 8, 2, 12, 20, 64),
                                      (64, 64, 8, 2048, 4100, 128), (1, 4, 4, 1, 5, 48)]:
        G = Hq // Hkv
        rows = Hkv * T * G
        nrb = cd(G * T, 32) + n_seq
        P_ = min(rows * max(cd(cd(nkv + T, 32) + 2, 4), 1), rows + 2048 * 32)
        want = 2 * al(P_ * 4) + al(P_ * D * 4) + al(nrb * 8) + al(T * 4)
        assert ws(n_seq, Hq, Hkv, T, nkv, D, 2) == want, (n_seq, Hq, Hkv, T, nkv, D)


# ------------------------------------------------------------------------------------------------ Python surface
class _StubLib:
    """stands in for libsfa.so: records the entry point a method reaches and its arguments, launches nothing"""

    def __init__(self):
        self.calls = []

    def sfa_decode_ragged_workspace_bytes(self, *a):
        return 256

    def __getattr__(self, name):
        if not name.startswith("sfa_"):
            raise AttributeError(name)

        def f(*args):
            self.calls.append((name, args))
            return 0
        return f


@pytest.fixture
def stub(monkeypatch):
    from sink_attention import _native
    lib = _StubLib()
    monkeypatch.setattr(_native, "lib", lambda: lib)
    monkeypatch.setattr(_native, "require_gpu", lambda *t: None)
    monkeypatch.setattr(_native, "stream_ptr", lambda device: 0)
    monkeypatch.setattr(torch.cuda, "device", lambda device: contextlib.nullcontext())
    return lib


def _cpu_pool(S=5, W=16, cls=SinkCacheLayer):
    if cls is SinkCacheLayer:
        layer = SinkCacheLayer(NS, W)
        layer.init_pool(S, HKV, 64, torch.bfloat16, "cpu")
        return layer
    cache = SinkAttentionCache(num_sink=NS, window_size=W)
    cache.init_pool(S, HKV, 64, torch.bfloat16, "cpu")
    return cache


def _mk(h, T=6):
    return torch.zeros(1, h, T, 64, dtype=torch.bfloat16)


@pytest.mark.parametrize("cls", [SinkCacheLayer, SinkAttentionCache])
def test_without_the_keywords_the_step_reaches_the_old_symbol(stub, cls):
    pool = _cpu_pool(cls=cls)
    kw = dict(layer_idx=0) if cls is SinkAttentionCache else {}
    pool.ragged_step_dyn(_mk(8), _mk(2), _mk(2), [0, 2, 6], [0, 1], **kw)
    pool.ragged_step_dyn(_mk(8), _mk(2), _mk(2), [0, 2, 6], [0, 1], commit=False, admit=True, **kw)
    assert [c[0] for c in stub.calls] == ["sfa_decode_ring_ragged_slots"] * 2
    assert len(stub.calls[0][1]) == 19 and stub.calls[0][1][9] == 1 and stub.calls[1][1][9] == 0
    assert stub.calls[1][1][17] == 0x40
    stub.calls.clear()
    par, cs = torch.tensor([-1, 0, -1, 0, 0, 2], dtype=torch.int32), torch.tensor([1, 0], dtype=torch.int32)
    pool.ragged_step_dyn(_mk(8), _mk(2), _mk(2), [0, 2, 6], [0, 1], parent=par, commit_seq=cs, admit=True, **kw)
    pool.ragged_step_dyn(_mk(8), _mk(2), _mk(2), [0, 2, 6], [0, 1], parent=[-1, 0, -1, 0, 0, 2], **kw)
    pool.ragged_step_dyn(_mk(8), _mk(2), _mk(2), [0, 2, 6], [0, 1], commit_seq=[1, 0], **kw)
    assert [c[0] for c in stub.calls] == ["sfa_decode_ring_ragged_tree_slots"] * 3
    a = stub.calls[0][1]
    assert len(a) == 21 and a[9] is not None and a[10] is not None and a[11] == 1 and a[19] == 0x40
    assert stub.calls[1][1][9] is not None and stub.calls[1][1][10] is None
    assert stub.calls[2][1][9] is None and stub.calls[2][1][10] is not None
    stub.calls.clear()
    cnt, path = torch.tensor([2, 1], dtype=torch.int32), torch.tensor([0, 1, 0, 2, 1, 3], dtype=torch.int32)
    pool.commit_packed_dyn(_mk(2), _mk(2), [0, 2, 6], [0, 1], cnt, path=path, **kw)
    pool.commit_packed_dyn(_mk(2), _mk(2), [0, 2, 6], [0, 1], [2, 1], **kw)
    assert [c[0] for c in stub.calls] == ["sfa_ring_commit_path_ragged_slots"] * 2
    a = stub.calls[0][1]
    assert len(a) == 11 and a[4] is not None and a[5] is not None and a[7] == 2
    assert stub.calls[1][1][5] is None


def test_host_lists_are_checked_and_nothing_is_called(stub):
    layer = _cpu_pool()
    step = lambda **kw: layer.ragged_step_dyn(_mk(8), _mk(2), _mk(2), [0, 2, 6], [0, 1], **kw)
    with pytest.raises(ValueError, match="parent must hold T = 6 entries, got 5"):
        step(parent=[-1, 0, -1, 0, 0])
    with pytest.raises(ValueError, match="commit_seq must hold n_seq = 2 entries, got 3"):
        step(commit_seq=[1, 0, 1])
    with pytest.raises(ValueError, match="parent must hold T = 6"):
        step(parent=torch.zeros(7, dtype=torch.int32))
    with pytest.raises(TypeError, match="parent must be a 1-D integer tensor"):
        step(parent=torch.zeros(6))
    with pytest.raises(TypeError, match="commit_seq must be a 1-D integer tensor"):
        step(commit_seq=torch.zeros(1, 2, dtype=torch.int32))
    commit = lambda count, **kw: layer.commit_packed_dyn(_mk(2), _mk(2), [0, 2, 6], [0, 1], count, **kw)
    with pytest.raises(ValueError, match="count must hold n_seq = 2 entries, got 1"):
        commit([2])
    with pytest.raises(ValueError, match="path must hold T = 6 entries, got 4"):
        commit([2, 1], path=[0, 1, 0, 1])
    with pytest.raises(TypeError, match="count must be"):
        commit(None)
    with pytest.raises(ValueError, match=r"packed \[1, H_kv, T, D\]"):
        layer.commit_packed_dyn(torch.zeros(2, 2, 6, 64, dtype=torch.bfloat16), torch.zeros(2, 2, 6, 64, dtype=torch.bfloat16),
                                [0, 2, 6], [0, 1], [1, 1])
    with pytest.raises(ValueError, match="named twice"):
        layer.commit_packed_dyn(_mk(2), _mk(2), [0, 2, 6], [1, 1], [1, 1])
    with pytest.raises(RuntimeError, match="needs a pool"):
        SinkCacheLayer(NS, 16).commit_packed_dyn(_mk(2), _mk(2), [0, 2, 6], [0, 1], [1, 1])
    assert stub.calls == []


def test_the_packed_commit_refuses_cpu_tensors():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _cpu_pool().commit_packed_dyn(_mk(2), _mk(2), [0, 2, 6], [0, 1], [1, 1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _cpu_pool().ragged_step_dyn(_mk(8), _mk(2), _mk(2), [0, 2, 6], [0, 1], parent=[-1] * 6)


# ------------------------------------------------------------------------------------------------ spec_tree, packed
def _random_pack(rng, n_seq, T_extra):
    lengths = [rng.choice([0, 1, 2, 5, 16, 33, 64, 65, 70]) for _ in range(n_seq)]
    cu = [0]
    for n in lengths:
        cu.append(cu[-1] + n)
    T = cu[-1] + T_extra
    parent = []
    for i, n in enumerate(lengths):
        par = random_tree(rng, n, forest=rng.random() < 0.5, shape=rng.choice(["random", "deep", "star"])) if n else []
        parent += corrupt(par, rng.randrange(1 << 30))[0] if rng.random() < 0.3 else par
    parent += [rng.randrange(-3, 80) for _ in range(T - cu[-1])]           # stale entries behind the pack
    return lengths, cu, T, parent


@pytest.mark.parametrize("seed", range(6))
def test_packed_tree_depth_is_tree_depth_row_by_row(seed):
    rng = random.Random(seed)
    lengths, cu, T, parent = _random_pack(rng, n_seq=rng.randrange(1, 9), T_extra=rng.randrange(0, 9))
    T = max(T, 1)
    parent = (parent + [0])[:T]
    got = spec_tree.packed_tree_depth(torch.tensor(parent, dtype=torch.int32), torch.tensor(cu, dtype=torch.int32), T)
    local = spec_tree.packed_local(torch.tensor(cu), T)
    assert got.shape == (T,) and got.dtype == torch.long
    want, wl = [0] * T, [0] * T
    for i, n in enumerate(lengths):
        sl = slice(cu[i], cu[i] + n)
        wl[sl] = range(n)
        if n > MAX_TREE:
            want[sl] = range(n)
        elif n:
            want[sl] = spec_tree.tree_depth(torch.tensor(parent[sl])).tolist()
            assert want[sl] == depths(read_as(parent[sl], n))
    assert got.tolist() == want and local.tolist() == wl


@pytest.mark.parametrize("seed", range(6))
def test_greedy_accept_packed_is_greedy_accept_row_by_row(seed):
    rng = random.Random(100 + seed)
    lengths, cu, T, parent = _random_pack(rng, n_seq=rng.randrange(1, 9), T_extra=rng.randrange(0, 9))
    T = max(T, 1)
    parent = (parent + [0])[:T]
    g = torch.Generator().manual_seed(seed)
    draft, target = torch.randint(0, 3, (T,), generator=g), torch.randint(0, 3, (T,), generator=g)
    path, count = spec_tree.greedy_accept_packed(torch.tensor(parent, dtype=torch.int32), draft, target,
                                                 torch.tensor(cu, dtype=torch.int32), len(lengths))
    assert path.shape == (T,) and count.shape == (len(lengths),)
    for i, n in enumerate(lengths):
        sl = slice(cu[i], cu[i] + n)
        if n == 0:
            assert count[i] == 0
        elif n > MAX_TREE:
            assert count[i] == n and path[sl].tolist() == list(range(n))
        else:
            p, c = spec_tree.greedy_accept(torch.tensor(parent[sl]), draft[sl], target[sl])
            assert count[i] == c and path[sl][:c].tolist() == p[:c].tolist(), (i, n)
            assert ((path[sl] >= 0) & (path[sl] < n)).all()
    with pytest.raises(ValueError, match="n_seq"):
        spec_tree.greedy_accept_packed(torch.tensor(parent), draft, target, torch.tensor(cu), len(lengths) + 1)


# ------------------------------------------------------------------------------------------------ the mask model
PACK_SHAPES = {1: chain, 7: star, 16: binary, 33: comb, 64: comb, 70: star}


@pytest.mark.parametrize("W", [16, 48])
@pytest.mark.parametrize("prefill", [2, 9, NS + 16, NS + 48 + 5])
def test_the_mask_model_matches_a_replay_of_append_along_every_path(prefill, W):
    """for every length of the pack: the keys packed_valid shows to node u are those the cache holds after appending u's
    root-to-u path to a cache of `prefill` tokens, one token at a time (a sequence of 70 tokens: its chain)"""
    ids = torch.arange(prefill, dtype=torch.float32).view(1, 1, -1, 1)
    base = SinkCacheLayer(NS, W)
    base.append(ids, ids)
    for n in LENGTHS:
        for parent in ([PACK_SHAPES[n](n), rand_tree(n, n), corrupt(rand_tree(n, n + 1), n)[0]] if n else []):
            m = packed_valid(prefill, min(prefill, NS), W, parent, n)
            par = read_as(parent, n)
            for u in range(n):
                twin = copy.deepcopy(base)
                for v in path_to(par, u):
                    x = torch.full((1, 1, 1, 1), float(prefill + v))
                    twin.append(x, x)
                replay = sorted(int(x) for x in twin.get_kv()[0][0, 0, :, 0].tolist())
                assert torch.nonzero(m[u]).flatten().tolist() == replay, (n, u, parent)


# (history length, tree or chunk length) per sequence: trees next to chunk_probe sequences.  The ring wrapped (NS + W + 5),
# full and not wrapped (NS + W), partly filled (9) and nearly empty (5)
PROBE_TREES = {16: [("tree", 25, "comb64"), ("chunk", 25, 33), ("tree", 20, "rand16"), ("chunk", 52, 1), ("tree", 9, "bin7"),
                    ("tree", 20, "rand33")],
               48: [("tree", 57, "comb64"), ("chunk", 57, 33), ("tree", 52, "rand16"), ("chunk", 20, 5), ("tree", 5, "bin7"),
                    ("tree", 52, "rand33")]}
PROBE_TYPES = [("bf16", 64, 8), ("fp16", 128, 1), ("bf16", 96, 1), ("fp32", 48, 8), ("fp32", 80, 1)]
_PROBE_TREE = {"comb64": lambda: comb(64), "rand16": lambda: rand_tree(16, 1), "bin7": lambda: binary(7),
               "rand33": lambda: rand_tree(33, 2)}


@functools.lru_cache(maxsize=None)
def tree_probe_pack(dt, D, G, W):
    """tree_probe inputs (TREE_KINDS) as sequences of a pack next to chunk_probe sequences: (q, k, v [1, H, T, D], s_aux,
    [(k, v) history per sequence], lengths, packed parent, {i: f64 reference rows [1, Hq, n, D]}, per-sequence
    (probe dict, history length, parent))"""
    dtype = P._DT[dt]
    prs = []
    for i, (kind, L, what) in enumerate(PROBE_TREES[W]):
        if kind == "tree":
            par = _PROBE_TREE[what]()
            prs.append((P.tree_probe(1, HKV * G, HKV, D, NS, W, L, par, dtype, seed=700 + i), L, par))
        else:
            prs.append((P.chunk_probe(1, HKV * G, HKV, D, NS, W, L, what, dtype, seed=700 + i), L, chain(what)))
    sa = prs[0][0]["s_aux"]                    # one s_aux per call: the first sequence's
    qs, ks, vs, hist, ref, parent = [], [], [], [], {}, []
    for i, (pr, L, par) in enumerate(prs):
        n = len(par)
        qs.append(pr["q"][:, :, L:]), ks.append(pr["k"][:, :, L:]), vs.append(pr["v"][:, :, L:])
        hist.append((pr["k"][:, :, :L], pr["v"][:, :, :L]))
        parent += par
        ref[i] = masked_attention(pr["q"][:, :, L:], pr["k"], pr["v"], None, packed_valid(L, min(L, NS), W, par, n), sa)[0]
    cat = lambda ts: torch.cat(ts, dim=2)
    return cat(qs), cat(ks), cat(vs), sa, hist, [len(p[2]) for p in prs], parent, ref, prs


def _mutants(L, W, par):
    """one-key errors of a tree sequence: a sibling shown, the oldest visible window key dropped"""
    n = len(par)
    true = packed_valid(L, min(L, NS), W, par, n)
    d = depths(par)
    sib, old = true.clone(), true.clone()
    for u in range(n):
        s = [x for x in range(n) if x != u and par[x] == par[u]]
        if s:
            sib[u, L + s[0]] = True
        first = L + d[u] - W + 1
        if NS <= first < L:
            old[u, first] = False
    return true, {"a sibling shown": sib, "oldest window key lost": old}


@pytest.mark.parametrize("W", [16, 48])
@pytest.mark.parametrize("dt,D,G", PROBE_TYPES)
def test_a_one_key_error_in_a_packed_tree_moves_a_probe_row_tenfold(dt, D, G, W):
    """Model against mutated model on the inputs of test_gpu_ragged_tree.py::test_mask_edge_probes: each mutant moves some
    row of some tree sequence of the pack by at least ten times DECODE_TOL; the unmutated model is the reference of the GPU
    test (factor 0 against itself)."""
    q, k, v, sa, hist, lengths, parent, ref, prs = tree_probe_pack(dt, D, G, W)
    tol = (DECODE_TOL[P._DT[dt]], 0.0)
    best = {}
    for i, (pr, L, par) in enumerate(prs):
        if PROBE_TREES[W][i][0] != "tree":
            continue
        inp = dict(q=pr["q"][:, :, L:], k=pr["k"], v=pr["v"], s_aux=sa)
        true, muts = _mutants(L, W, par)
        assert factors(inp, true, true, torch.arange(len(par)), tol_o=tol)[0] == 0.0
        for what, mut in muts.items():
            hit = torch.nonzero((true != mut).any(1)).flatten()
            if hit.numel() == 0:
                continue
            fo = factors(inp, true, mut, hit, tol_o=tol)[0]
            print(f"{dt} D={D} G={G} Wc={W} sequence {i} (history {L}, n {len(par)}), {what}: {fo:.1f} tolerances")
            best[what] = max(best.get(what, 0.0), fo)
    assert set(best) == {"a sibling shown", "oldest window key lost"}
    for what, fo in best.items():
        assert fo >= 10, (what, fo)
