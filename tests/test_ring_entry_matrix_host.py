"""CPU-only characterisation of the argument checks of all 23 sink + ring cache entry points of libsfa.so: a table of
entry point x defect, each cell the status code and the exact sfa_last_error() text; a second table of combined defects
that pins which message wins (the order of the checks); and the empty-shape calls that return SFA_OK without a launch.
Host tensors stand in for device memory as in tests/test_slots_host.py: every call here returns before any launch, so
nothing is dereferenced."""
import pytest
import torch

from sink_attention import _native as N

B, S, HQ, HKV, NN, D, NS, W, T = 2, 5, 8, 2, 3, 64, 4, 16, 6
BF, FP = torch.bfloat16, torch.float16


def _z(*shape, dtype=BF):
    return torch.zeros(*shape, dtype=dtype)


def _odd(*shape, dtype=BF):
    """130-byte rows: shape[3] = 64 columns of a 65-column buffer (unit last stride, row stride not a 16-byte multiple)"""
    return torch.zeros(*shape[:3], shape[3] + 1, dtype=dtype)[..., :shape[3]]


def _tensors(mk=_z, dtype=BF, b=B, s=S, hq=HQ, n=NN, t=T):
    """q / kn / vn / o: a chunk of n tokens for b batch rows; q1 / k1 / v1 / o1: one token; qp / kp / vp / op: a pack of
    t rows; sk .. wv: the cache of b rows; psk .. pwv: a pool of s slots"""
    return dict(q=mk(b, hq, n, D, dtype=dtype), kn=mk(b, HKV, n, D, dtype=dtype), vn=mk(b, HKV, n, D, dtype=dtype),
                o=mk(b, hq, n, D, dtype=dtype), q1=mk(b, hq, 1, D, dtype=dtype), k1=mk(b, HKV, 1, D, dtype=dtype),
                v1=mk(b, HKV, 1, D, dtype=dtype), o1=mk(b, hq, 1, D, dtype=dtype), qp=mk(1, hq, t, D, dtype=dtype),
                kp=mk(1, HKV, t, D, dtype=dtype), vp=mk(1, HKV, t, D, dtype=dtype), op=mk(1, hq, t, D, dtype=dtype),
                sk=mk(b, HKV, NS, D, dtype=dtype), sv=mk(b, HKV, NS, D, dtype=dtype), wk=mk(b, HKV, W, D, dtype=dtype),
                wv=mk(b, HKV, W, D, dtype=dtype), psk=mk(s, HKV, NS, D, dtype=dtype), psv=mk(s, HKV, NS, D, dtype=dtype),
                pwk=mk(s, HKV, W, D, dtype=dtype), pwv=mk(s, HKV, W, D, dtype=dtype))


_KEEP = []      # the tensors behind every descriptor stay alive for the module


def _descs(**kw):
    t = _tensors(**kw)
    _KEEP.append(t)
    return {k: N.desc(v) for k, v in t.items()}


BASE = _descs()
_HOST = torch.zeros(64, dtype=torch.int32)      # stands in for state / slots / parent / path / count / cu: never read
P = _HOST.data_ptr()
WS = 1 << 20                                     # a 256-byte aligned address, never dereferenced
SCALARS = dict(aux=None, ws=None, wsb=0, scale=0.125, flags=0, stream=None, state=P, slots=P, parent=P, pstride=0,
               count=P, path=P, pathstride=0, cu=P, nseq=2, commit=1, sl=NS, wl=W, wp=0)

# the argument list of every entry point in the names of BASE / SCALARS.  act: the activations an entry point takes
# (chunk, one token, pack or none); cache: the buffers of B rows, the pool, or a single key segment
CHUNK, ONE, PACK = ("q", "kn", "vn", "o"), ("q1", "k1", "v1", "o1"), ("qp", "kp", "vp", "op")
ROWS, POOL = ("sk", "sv", "wk", "wv"), ("psk", "psv", "pwk", "pwv")


def _sig(act, cache, mid, tail="ws wsb scale flags stream"):
    q, kn, vn, o = act
    sk, sv, wk, wv = cache
    return mid.format(q=q, kn=kn, vn=vn, o=o, sk=sk, sv=sv, wk=wk, wv=wv).split() + tail.split()


_DYN = "{q} {sk} {sv} {wk} {wv} {kn} {vn} {o} aux"
_HOSTST = "{q} {sk} {sv} sl {wk} {wv} wl wp {kn} {vn} {o} aux"
_CM = "{wk} {wv} {kn} {vn} count"
ENTRY = {
    "sfa_decode": (ONE, ROWS, _sig(ONE, ROWS, "{q} {sk} {sv} {o} aux")),
    "sfa_decode_ring": (ONE, ROWS, _sig(ONE, ROWS, "{q} {sk} {sv} sl {wk} {wv} wl {o} aux")),
    "sfa_decode_ring_step": (ONE, ROWS, _sig(ONE, ROWS, _HOSTST)),
    "sfa_decode_ring_step_dyn": (ONE, ROWS, _sig(ONE, ROWS, _DYN + " state")),
    "sfa_decode_ring_step_rows": (ONE, ROWS, _sig(ONE, ROWS, _DYN + " state")),
    "sfa_decode_ring_step_slots": (ONE, POOL, _sig(ONE, POOL, _DYN + " state slots")),
    "sfa_decode_ring_multi": (CHUNK, ROWS, _sig(CHUNK, ROWS, _HOSTST + " commit")),
    "sfa_decode_ring_multi_dyn": (CHUNK, ROWS, _sig(CHUNK, ROWS, _DYN + " commit state")),
    "sfa_decode_ring_multi_rows": (CHUNK, ROWS, _sig(CHUNK, ROWS, _DYN + " commit state")),
    "sfa_decode_ring_multi_slots": (CHUNK, POOL, _sig(CHUNK, POOL, _DYN + " commit state slots")),
    "sfa_decode_ring_ragged_slots": (PACK, POOL, _sig(PACK, POOL, _DYN + " commit state slots cu nseq")),
    "sfa_decode_ring_tree": (CHUNK, ROWS, _sig(CHUNK, ROWS, _HOSTST + " parent pstride")),
    "sfa_decode_ring_tree_dyn": (CHUNK, ROWS, _sig(CHUNK, ROWS, _DYN + " parent pstride state")),
    "sfa_decode_ring_tree_rows": (CHUNK, ROWS, _sig(CHUNK, ROWS, _DYN + " parent pstride state")),
    "sfa_decode_ring_tree_slots": (CHUNK, POOL, _sig(CHUNK, POOL, _DYN + " parent pstride state slots")),
    "sfa_ring_commit_dyn": (CHUNK, ROWS, _sig(CHUNK, ROWS, _CM + " state", "stream")),
    "sfa_ring_commit_rows": (CHUNK, ROWS, _sig(CHUNK, ROWS, _CM + " state", "stream")),
    "sfa_ring_commit_slots": (CHUNK, POOL, _sig(CHUNK, POOL, _CM + " state slots", "stream")),
    "sfa_ring_commit_path_dyn": (CHUNK, ROWS, _sig(CHUNK, ROWS, _CM + " path pathstride state", "stream")),
    "sfa_ring_commit_path_rows": (CHUNK, ROWS, _sig(CHUNK, ROWS, _CM + " path pathstride state", "stream")),
    "sfa_ring_commit_path_slots": (CHUNK, POOL, _sig(CHUNK, POOL, _CM + " path pathstride state slots", "stream")),
    "sfa_ring_fill_varlen": (PACK, ROWS, _sig(PACK, ROWS, "{sk} {sv} {wk} {wv} {kn} {vn} cu nseq state", "stream")),
    "sfa_ring_fill_varlen_slots": (PACK, POOL, _sig(PACK, POOL, "{sk} {sv} {wk} {wv} {kn} {vn} cu nseq state slots",
                                                    "stream")),
}
assert len(ENTRY) == 23


def call(name, descs=None, **scalars):
    """Run entry point `name` on BASE with `descs` (name -> descriptor or None) and `scalars` replaced; returns
    (status, error text)."""
    d = dict(BASE, **(descs or {}))
    s = dict(SCALARS, **scalars)
    lib = N.lib()
    st = getattr(lib, name)(*[d[a] if a in d else s[a] for a in ENTRY[name][2]])
    return st, lib.sfa_last_error().decode()


def _swap(name, other, *roles):
    """the entry point's tensors of the given roles (q, kn, vn, o, sk, sv, wk, wv) taken from the descriptor set `other`"""
    act, cache, _ = ENTRY[name]
    names = dict(zip(("q", "kn", "vn", "o", "sk", "sv", "wk", "wv"), act + cache))
    return {names[r]: (other[names[r]] if other is not None else None) for r in roles}


HALF, HQ7, N0, N65, ODD, S7 = (_descs(dtype=FP), _descs(hq=7), _descs(n=0, t=0), _descs(n=65), _descs(mk=_odd),
                               _descs(s=7))
B2PACK = {"qp": BASE["q"], "kp": BASE["kn"], "vp": BASE["vn"], "op": BASE["o"]}    # [2, H, 3, D] where a pack belongs


def _has(name, arg):
    return arg in ENTRY[name][2]


def _need(name):
    """the workspace size the entry point asks for at BASE"""
    lib = N.lib()
    act = ENTRY[name][0]
    if act is ONE:
        nkv = NS if name == "sfa_decode" else NS + W
        return lib.sfa_decode_workspace_bytes(B, HQ, HKV, nkv, D, 2)
    if act is PACK:
        return lib.sfa_decode_ragged_workspace_bytes(2, HQ, HKV, T, NS + W, D, 2)
    return lib.sfa_decode_multi_workspace_bytes(B, HQ, HKV, NN, NS + W + NN, D, 2)


def defect(name, which):
    """keyword arguments of call() that plant defect `which` in entry point `name`, or None where it does not apply"""
    commit, fill = name.startswith("sfa_ring_commit"), name.startswith("sfa_ring_fill")
    chunkless = name in ("sfa_decode", "sfa_decode_ring")
    if which == "null_state":
        return dict(state=None) if _has(name, "state") else None
    if which == "null_slots":
        return dict(slots=None) if _has(name, "slots") else None
    if which == "null_cache":
        return dict(descs=_swap(name, None, "wk" if commit else "sk"))
    if which == "null_k_new":
        return None if chunkless else dict(descs=_swap(name, None, "kn"))
    if which == "dtype":
        return dict(descs=_swap(name, HALF, "q", "o") if chunkless else _swap(name, HALF, "kn", "vn"))
    if which == "heads":
        return None if commit or fill else dict(descs=_swap(name, HQ7, "q", "o"))
    if which == "n0":
        if fill or ENTRY[name][0] is ONE:
            return None
        return dict(descs=_swap(name, N0, "kn", "vn") if commit else _swap(name, N0, "q", "o", "kn", "vn"))
    if which == "n65":
        return dict(descs=_swap(name, N65, "q", "o", "kn", "vn")) if "_tree" in name else None
    if which == "bstride":
        if _has(name, "pstride"):
            return dict(pstride=2)
        return dict(pathstride=1) if _has(name, "pathstride") else None
    if which == "misaligned":
        return dict(descs=_swap(name, ODD, "q") if chunkless else _swap(name, ODD, "kn"))
    if which == "pool_s":
        return dict(descs=_swap(name, S7, "wk", "wv")) if ENTRY[name][1] is POOL and not commit else None
    if which == "null_ws":
        return dict(ws=None, wsb=0) if _has(name, "ws") else None
    if which == "short_ws":
        return dict(ws=WS, wsb=_need(name) - 1) if _has(name, "ws") else None
    if which == "unaligned_ws":
        return dict(ws=WS + 16, wsb=1 << 30) if _has(name, "ws") else None
    if which == "not_packed":
        return dict(descs=B2PACK) if name == "sfa_decode_ring_ragged_slots" else None
    if which == "n_seq0":
        return dict(nseq=0) if _has(name, "nseq") else None
    if which in ("null_parent", "null_count", "null_path", "null_cu"):      # only used in COMBINED
        arg = which[5:]
        return {arg: None} if _has(name, arg) else None
    raise KeyError(which)


DEFECTS = ("null_state", "null_slots", "null_cache", "null_k_new", "dtype", "heads", "n0", "n65", "bstride",
           "misaligned", "pool_s", "null_ws", "short_ws", "unaligned_ws", "not_packed", "n_seq0")

# entry point -> defect -> (status, sfa_last_error()); a defect that an entry point cannot have is absent
EXPECT = {
    "sfa_decode": {
        "null_cache": (-1, 'k: null tensor descriptor'),
        "dtype": (-1, 'q and k differ in dtype'),
        "heads": (-1, 'H_q (7) must be divisible by H_kv (2)'),
        "misaligned": (-1, 'decode: q/k/v rows must be 16-byte aligned'),
        "null_ws": (-3, 'decode workspace: need 4608 bytes, 256-byte aligned (got 0 at (nil))'),
        "short_ws": (-3, 'decode workspace: need 4608 bytes, 256-byte aligned (got 4607 at 0x100000)'),
        "unaligned_ws": (-3, 'decode workspace: need 4608 bytes, 256-byte aligned (got 1073741824 at 0x100010)'),
    },
    "sfa_decode_ring": {
        "null_cache": (-1, 'k: null tensor descriptor'),
        "dtype": (-1, 'q and k differ in dtype'),
        "heads": (-1, 'H_q (7) must be divisible by H_kv (2)'),
        "misaligned": (-1, 'decode: q/k/v rows must be 16-byte aligned'),
        "null_ws": (-3, 'decode workspace: need 4608 bytes, 256-byte aligned (got 0 at (nil))'),
        "short_ws": (-3, 'decode workspace: need 4608 bytes, 256-byte aligned (got 4607 at 0x100000)'),
        "unaligned_ws": (-3, 'decode workspace: need 4608 bytes, 256-byte aligned (got 1073741824 at 0x100010)'),
    },
    "sfa_decode_ring_step": {
        "null_cache": (-1, 'k: null tensor descriptor'),
        "null_k_new": (-1, 'k_new / v_new: null tensor descriptor'),
        "dtype": (-1, "k_new / v_new must be [B, H_kv, 1, D] in the ring's dtype"),
        "heads": (-1, 'H_q (7) must be divisible by H_kv (2)'),
        "misaligned": (-1, 'decode: q/k/v rows must be 16-byte aligned'),
        "null_ws": (-3, 'decode workspace: need 4608 bytes, 256-byte aligned (got 0 at (nil))'),
        "short_ws": (-3, 'decode workspace: need 4608 bytes, 256-byte aligned (got 4607 at 0x100000)'),
        "unaligned_ws": (-3, 'decode workspace: need 4608 bytes, 256-byte aligned (got 1073741824 at 0x100010)'),
    },
    "sfa_decode_ring_step_dyn": {
        "null_state": (-1, 'state: null device pointer'),
        "null_cache": (-1, 'cache buffers: null tensor descriptor'),
        "null_k_new": (-1, 'k_new / v_new: null tensor descriptor'),
        "dtype": (-1, "k_new / v_new must be [B, H_kv, 1, D] in the ring's dtype"),
        "heads": (-1, 'H_q (7) must be divisible by H_kv (2)'),
        "misaligned": (-1, 'decode: q/k/v rows must be 16-byte aligned'),
        "null_ws": (-3, 'decode workspace: need 4608 bytes, 256-byte aligned (got 0 at (nil))'),
        "short_ws": (-3, 'decode workspace: need 4608 bytes, 256-byte aligned (got 4607 at 0x100000)'),
        "unaligned_ws": (-3, 'decode workspace: need 4608 bytes, 256-byte aligned (got 1073741824 at 0x100010)'),
    },
    "sfa_decode_ring_step_rows": {
        "null_state": (-1, 'state: null device pointer'),
        "null_cache": (-1, 'cache buffers: null tensor descriptor'),
        "null_k_new": (-1, 'k_new / v_new: null tensor descriptor'),
        "dtype": (-1, "k_new / v_new must be [B, H_kv, 1, D] in the ring's dtype"),
        "heads": (-1, 'H_q (7) must be divisible by H_kv (2)'),
        "misaligned": (-1, 'decode: q/k/v rows must be 16-byte aligned'),
        "null_ws": (-3, 'decode workspace: need 4608 bytes, 256-byte aligned (got 0 at (nil))'),
        "short_ws": (-3, 'decode workspace: need 4608 bytes, 256-byte aligned (got 4607 at 0x100000)'),
        "unaligned_ws": (-3, 'decode workspace: need 4608 bytes, 256-byte aligned (got 1073741824 at 0x100010)'),
    },
    "sfa_decode_ring_step_slots": {
        "null_state": (-1, 'state: null device pointer'),
        "null_slots": (-1, 'slots: null device pointer'),
        "null_cache": (-1, 'cache buffers: null tensor descriptor'),
        "null_k_new": (-1, 'k_new / v_new: null tensor descriptor'),
        "dtype": (-1, "k_new / v_new must be [B, H_kv, 1, D] in the ring's dtype"),
        "heads": (-1, 'H_q (7) must be divisible by H_kv (2)'),
        "misaligned": (-1, 'decode: q/k/v rows must be 16-byte aligned'),
        "pool_s": (-1, 'pool: sink and window buffers must share shape[0] = S (sink 5, window 7)'),
        "null_ws": (-3, 'decode workspace: need 4608 bytes, 256-byte aligned (got 0 at (nil))'),
        "short_ws": (-3, 'decode workspace: need 4608 bytes, 256-byte aligned (got 4607 at 0x100000)'),
        "unaligned_ws": (-3, 'decode workspace: need 4608 bytes, 256-byte aligned (got 1073741824 at 0x100010)'),
    },
    "sfa_decode_ring_multi": {
        "null_cache": (-1, 'sink_k: null tensor descriptor'),
        "null_k_new": (-1, 'k_new: null tensor descriptor'),
        "dtype": (-1, 'q, the cache buffers and k_new / v_new must share one dtype'),
        "heads": (-1, 'H_q (7) must be divisible by H_kv (2)'),
        "n0": (-1, 'decode_multi: the chunk needs at least one token'),
        "misaligned": (-1, 'decode_multi: rows of every tensor must be 16-byte aligned'),
        "null_ws": (-3, 'decode_multi workspace: need 12800 bytes, 256-byte aligned (got 0 at (nil))'),
        "short_ws": (-3, 'decode_multi workspace: need 12800 bytes, 256-byte aligned (got 12799 at 0x100000)'),
        "unaligned_ws": (-3, 'decode_multi workspace: need 12800 bytes, 256-byte aligned (got 1073741824 at 0x100010)'),
    },
    "sfa_decode_ring_multi_dyn": {
        "null_state": (-1, 'state: null device pointer'),
        "null_cache": (-1, 'cache buffers: null tensor descriptor'),
        "null_k_new": (-1, 'k_new: null tensor descriptor'),
        "dtype": (-1, 'q, the cache buffers and k_new / v_new must share one dtype'),
        "heads": (-1, 'H_q (7) must be divisible by H_kv (2)'),
        "n0": (-1, 'decode_multi: the chunk needs at least one token'),
        "misaligned": (-1, 'decode_multi: rows of every tensor must be 16-byte aligned'),
        "null_ws": (-3, 'decode_multi workspace: need 12800 bytes, 256-byte aligned (got 0 at (nil))'),
        "short_ws": (-3, 'decode_multi workspace: need 12800 bytes, 256-byte aligned (got 12799 at 0x100000)'),
        "unaligned_ws": (-3, 'decode_multi workspace: need 12800 bytes, 256-byte aligned (got 1073741824 at 0x100010)'),
    },
    "sfa_decode_ring_multi_rows": {
        "null_state": (-1, 'state: null device pointer'),
        "null_cache": (-1, 'cache buffers: null tensor descriptor'),
        "null_k_new": (-1, 'k_new: null tensor descriptor'),
        "dtype": (-1, 'q, the cache buffers and k_new / v_new must share one dtype'),
        "heads": (-1, 'H_q (7) must be divisible by H_kv (2)'),
        "n0": (-1, 'decode_multi: the chunk needs at least one token'),
        "misaligned": (-1, 'decode_multi: rows of every tensor must be 16-byte aligned'),
        "null_ws": (-3, 'decode_multi workspace: need 12800 bytes, 256-byte aligned (got 0 at (nil))'),
        "short_ws": (-3, 'decode_multi workspace: need 12800 bytes, 256-byte aligned (got 12799 at 0x100000)'),
        "unaligned_ws": (-3, 'decode_multi workspace: need 12800 bytes, 256-byte aligned (got 1073741824 at 0x100010)'),
    },
    "sfa_decode_ring_multi_slots": {
        "null_state": (-1, 'state: null device pointer'),
        "null_slots": (-1, 'slots: null device pointer'),
        "null_cache": (-1, 'cache buffers: null tensor descriptor'),
        "null_k_new": (-1, 'k_new: null tensor descriptor'),
        "dtype": (-1, 'q, the cache buffers and k_new / v_new must share one dtype'),
        "heads": (-1, 'H_q (7) must be divisible by H_kv (2)'),
        "n0": (-1, 'decode_multi: the chunk needs at least one token'),
        "misaligned": (-1, 'decode_multi: rows of every tensor must be 16-byte aligned'),
        "pool_s": (-1, 'pool: sink and window buffers must share shape[0] = S >= 1 (sink 5, window 7)'),
        "null_ws": (-3, 'decode_multi workspace: need 12800 bytes, 256-byte aligned (got 0 at (nil))'),
        "short_ws": (-3, 'decode_multi workspace: need 12800 bytes, 256-byte aligned (got 12799 at 0x100000)'),
        "unaligned_ws": (-3, 'decode_multi workspace: need 12800 bytes, 256-byte aligned (got 1073741824 at 0x100010)'),
    },
    "sfa_decode_ring_ragged_slots": {
        "null_state": (-1, 'state: null device pointer'),
        "null_slots": (-1, 'slots: null device pointer'),
        "null_cache": (-1, 'cache buffers: null tensor descriptor'),
        "null_k_new": (-1, 'k_new: null tensor descriptor'),
        "dtype": (-1, 'q, the cache buffers and k_new / v_new must share one dtype'),
        "heads": (-1, 'H_q (7) must be divisible by H_kv (2)'),
        "n0": (-1, 'decode_multi: the chunk needs at least one token'),
        "misaligned": (-1, 'decode_multi: rows of every tensor must be 16-byte aligned'),
        "pool_s": (-1, 'pool: sink and window buffers must share shape[0] = S >= 1 (sink 5, window 7)'),
        "null_ws": (-3, 'decode_ragged workspace: need 13312 bytes, 256-byte aligned (got 0 at (nil))'),
        "short_ws": (-3, 'decode_ragged workspace: need 13312 bytes, 256-byte aligned (got 13311 at 0x100000)'),
        "unaligned_ws": (-3, 'decode_ragged workspace: need 13312 bytes, 256-byte aligned (got 1073741824 at 0x100010)'),
        "not_packed": (-1, 'decode_ragged: q / k_new / v_new / o must be packed [1, H, T, D] (got shape[0] = 2)'),
        "n_seq0": (-1, 'decode_ragged: n_seq (0) must be at least 1'),
    },
    "sfa_decode_ring_tree": {
        "null_cache": (-1, 'sink_k: null tensor descriptor'),
        "null_k_new": (-1, 'k_new: null tensor descriptor'),
        "dtype": (-1, 'q, the cache buffers and k_new / v_new must share one dtype'),
        "heads": (-1, 'H_q (7) must be divisible by H_kv (2)'),
        "n0": (-1, 'decode_multi: the chunk needs at least one token'),
        "n65": (-1, 'decode_tree: a tree chunk holds at most 64 nodes (got n = 65)'),
        "bstride": (-1, 'parent_bstride 2: 0 (one tree shared by the batch) or >= n = 3 (one row per sequence)'),
        "misaligned": (-1, 'decode_multi: rows of every tensor must be 16-byte aligned'),
        "null_ws": (-3, 'decode_multi workspace: need 12800 bytes, 256-byte aligned (got 0 at (nil))'),
        "short_ws": (-3, 'decode_multi workspace: need 12800 bytes, 256-byte aligned (got 12799 at 0x100000)'),
        "unaligned_ws": (-3, 'decode_multi workspace: need 12800 bytes, 256-byte aligned (got 1073741824 at 0x100010)'),
    },
    "sfa_decode_ring_tree_dyn": {
        "null_state": (-1, 'state: null device pointer'),
        "null_cache": (-1, 'cache buffers: null tensor descriptor'),
        "null_k_new": (-1, 'k_new: null tensor descriptor'),
        "dtype": (-1, 'q, the cache buffers and k_new / v_new must share one dtype'),
        "heads": (-1, 'H_q (7) must be divisible by H_kv (2)'),
        "n0": (-1, 'decode_multi: the chunk needs at least one token'),
        "n65": (-1, 'decode_tree: a tree chunk holds at most 64 nodes (got n = 65)'),
        "bstride": (-1, 'parent_bstride 2: 0 (one tree shared by the batch) or >= n = 3 (one row per sequence)'),
        "misaligned": (-1, 'decode_multi: rows of every tensor must be 16-byte aligned'),
        "null_ws": (-3, 'decode_multi workspace: need 12800 bytes, 256-byte aligned (got 0 at (nil))'),
        "short_ws": (-3, 'decode_multi workspace: need 12800 bytes, 256-byte aligned (got 12799 at 0x100000)'),
        "unaligned_ws": (-3, 'decode_multi workspace: need 12800 bytes, 256-byte aligned (got 1073741824 at 0x100010)'),
    },
    "sfa_decode_ring_tree_rows": {
        "null_state": (-1, 'state: null device pointer'),
        "null_cache": (-1, 'cache buffers: null tensor descriptor'),
        "null_k_new": (-1, 'k_new: null tensor descriptor'),
        "dtype": (-1, 'q, the cache buffers and k_new / v_new must share one dtype'),
        "heads": (-1, 'H_q (7) must be divisible by H_kv (2)'),
        "n0": (-1, 'decode_multi: the chunk needs at least one token'),
        "n65": (-1, 'decode_tree: a tree chunk holds at most 64 nodes (got n = 65)'),
        "bstride": (-1, 'parent_bstride 2: 0 (one tree shared by the batch) or >= n = 3 (one row per sequence)'),
        "misaligned": (-1, 'decode_multi: rows of every tensor must be 16-byte aligned'),
        "null_ws": (-3, 'decode_multi workspace: need 12800 bytes, 256-byte aligned (got 0 at (nil))'),
        "short_ws": (-3, 'decode_multi workspace: need 12800 bytes, 256-byte aligned (got 12799 at 0x100000)'),
        "unaligned_ws": (-3, 'decode_multi workspace: need 12800 bytes, 256-byte aligned (got 1073741824 at 0x100010)'),
    },
    "sfa_decode_ring_tree_slots": {
        "null_state": (-1, 'state: null device pointer'),
        "null_slots": (-1, 'slots: null device pointer'),
        "null_cache": (-1, 'cache buffers: null tensor descriptor'),
        "null_k_new": (-1, 'k_new: null tensor descriptor'),
        "dtype": (-1, 'q, the cache buffers and k_new / v_new must share one dtype'),
        "heads": (-1, 'H_q (7) must be divisible by H_kv (2)'),
        "n0": (-1, 'decode_multi: the chunk needs at least one token'),
        "n65": (-1, 'decode_tree: a tree chunk holds at most 64 nodes (got n = 65)'),
        "bstride": (-1, 'parent_bstride 2: 0 (one tree shared by the batch) or >= n = 3 (one row per sequence)'),
        "misaligned": (-1, 'decode_multi: rows of every tensor must be 16-byte aligned'),
        "pool_s": (-1, 'pool: sink and window buffers must share shape[0] = S >= 1 (sink 5, window 7)'),
        "null_ws": (-3, 'decode_multi workspace: need 12800 bytes, 256-byte aligned (got 0 at (nil))'),
        "short_ws": (-3, 'decode_multi workspace: need 12800 bytes, 256-byte aligned (got 12799 at 0x100000)'),
        "unaligned_ws": (-3, 'decode_multi workspace: need 12800 bytes, 256-byte aligned (got 1073741824 at 0x100010)'),
    },
    "sfa_ring_commit_dyn": {
        "null_state": (-1, 'state: null device pointer'),
        "null_cache": (-1, 'window_k: null tensor descriptor'),
        "null_k_new": (-1, 'k_new: null tensor descriptor'),
        "dtype": (-1, 'k_new / v_new and the ring must share one dtype'),
        "n0": (-1, 'ring_commit: the chunk needs at least one token'),
        "misaligned": (-1, 'ring_commit: rows of every tensor must be 16-byte aligned'),
    },
    "sfa_ring_commit_rows": {
        "null_state": (-1, 'state: null device pointer'),
        "null_cache": (-1, 'window_k: null tensor descriptor'),
        "null_k_new": (-1, 'k_new: null tensor descriptor'),
        "dtype": (-1, 'k_new / v_new and the ring must share one dtype'),
        "n0": (-1, 'ring_commit: the chunk needs at least one token'),
        "misaligned": (-1, 'ring_commit: rows of every tensor must be 16-byte aligned'),
    },
    "sfa_ring_commit_slots": {
        "null_state": (-1, 'state: null device pointer'),
        "null_slots": (-1, 'slots: null device pointer'),
        "null_cache": (-1, 'window_k: null tensor descriptor'),
        "null_k_new": (-1, 'k_new: null tensor descriptor'),
        "dtype": (-1, 'k_new / v_new and the ring must share one dtype'),
        "n0": (-1, 'ring_commit: the chunk needs at least one token'),
        "misaligned": (-1, 'ring_commit: rows of every tensor must be 16-byte aligned'),
    },
    "sfa_ring_commit_path_dyn": {
        "null_state": (-1, 'state: null device pointer'),
        "null_cache": (-1, 'window_k: null tensor descriptor'),
        "null_k_new": (-1, 'k_new: null tensor descriptor'),
        "dtype": (-1, 'k_new / v_new and the ring must share one dtype'),
        "n0": (-1, 'ring_commit: the chunk needs at least one token'),
        "bstride": (-1, 'path_bstride 1: 0 (one path shared by the batch) or >= n = 3 (one row per sequence)'),
        "misaligned": (-1, 'ring_commit: rows of every tensor must be 16-byte aligned'),
    },
    "sfa_ring_commit_path_rows": {
        "null_state": (-1, 'state: null device pointer'),
        "null_cache": (-1, 'window_k: null tensor descriptor'),
        "null_k_new": (-1, 'k_new: null tensor descriptor'),
        "dtype": (-1, 'k_new / v_new and the ring must share one dtype'),
        "n0": (-1, 'ring_commit: the chunk needs at least one token'),
        "bstride": (-1, 'path_bstride 1: 0 (one path shared by the batch) or >= n = 3 (one row per sequence)'),
        "misaligned": (-1, 'ring_commit: rows of every tensor must be 16-byte aligned'),
    },
    "sfa_ring_commit_path_slots": {
        "null_state": (-1, 'state: null device pointer'),
        "null_slots": (-1, 'slots: null device pointer'),
        "null_cache": (-1, 'window_k: null tensor descriptor'),
        "null_k_new": (-1, 'k_new: null tensor descriptor'),
        "dtype": (-1, 'k_new / v_new and the ring must share one dtype'),
        "n0": (-1, 'ring_commit: the chunk needs at least one token'),
        "bstride": (-1, 'path_bstride 1: 0 (one path shared by the batch) or >= n = 3 (one row per sequence)'),
        "misaligned": (-1, 'ring_commit: rows of every tensor must be 16-byte aligned'),
    },
    "sfa_ring_fill_varlen": {
        "null_state": (-1, 'state: null device pointer'),
        "null_cache": (-1, 'sink_k: null tensor descriptor'),
        "null_k_new": (-1, 'k: null tensor descriptor'),
        "dtype": (-1, 'k / v and the cache buffers must share one dtype'),
        "misaligned": (-1, 'ring_fill_varlen: rows of every tensor must be 16-byte aligned'),
        "n_seq0": (-1, 'n_seq must be >= 1 (got 0)'),
    },
    "sfa_ring_fill_varlen_slots": {
        "null_state": (-1, 'state: null device pointer'),
        "null_slots": (-1, 'slots: null device pointer'),
        "null_cache": (-1, 'sink_k: null tensor descriptor'),
        "null_k_new": (-1, 'k: null tensor descriptor'),
        "dtype": (-1, 'k / v and the cache buffers must share one dtype'),
        "misaligned": (-1, 'ring_fill_varlen: rows of every tensor must be 16-byte aligned'),
        "pool_s": (-1, 'pool: sink and window buffers must share shape[0] = S >= 1 (sink 5, window 7)'),
        "n_seq0": (-1, 'n_seq must be >= 1 (got 0)'),
    },
}

CELLS = [(name, which) for name in ENTRY for which in DEFECTS if defect(name, which) is not None]


def test_the_table_covers_every_applicable_cell():
    assert {(n, w) for n, cells in EXPECT.items() for w in cells} == set(CELLS)
    for which in DEFECTS:                      # every defect has an entry point that can have it
        assert any(w == which for _, w in CELLS), which


@pytest.mark.parametrize("name", list(ENTRY))
def test_every_defect_fails_with_its_status_and_text_before_any_launch(name):
    for which, want in EXPECT[name].items():
        assert call(name, **defect(name, which)) == want, which


def _both(name, *whiches):
    kw = {}
    for which in whiches:
        one = dict(defect(name, which))
        kw.setdefault("descs", {}).update(one.pop("descs", {}))
        kw.update(one)
    return kw


# two defects at once: the message of the check that runs first wins
COMBINED = [
    ("sfa_decode_ring_step_slots", ("null_k_new", "null_state"), "k_new / v_new: null tensor descriptor"),
    ("sfa_decode_ring_step_slots", ("null_state", "null_slots"), "state: null device pointer"),
    ("sfa_decode_ring_step_slots", ("null_slots", "null_cache"), "slots: null device pointer"),
    ("sfa_decode_ring_step_slots", ("null_cache", "heads"), "cache buffers: null tensor descriptor"),
    ("sfa_decode_ring_step_slots", ("pool_s", "null_ws"),
     "pool: sink and window buffers must share shape[0] = S (sink 5, window 7)"),
    ("sfa_decode_ring_step_rows", ("misaligned", "null_ws"), "decode: q/k/v rows must be 16-byte aligned"),
    ("sfa_decode_ring_multi_dyn", ("null_state", "null_k_new"), "state: null device pointer"),
    ("sfa_decode_ring_multi_slots", ("null_state", "null_slots"), "state: null device pointer"),
    ("sfa_decode_ring_multi_slots", ("null_slots", "null_cache"), "slots: null device pointer"),
    ("sfa_decode_ring_multi_slots", ("null_cache", "n0"), "cache buffers: null tensor descriptor"),
    ("sfa_decode_ring_multi_slots", ("n0", "dtype"), "q, the cache buffers and k_new / v_new must share one dtype"),
    ("sfa_decode_ring_multi_slots", ("n0", "pool_s"), "decode_multi: the chunk needs at least one token"),
    ("sfa_decode_ring_multi_slots", ("heads", "pool_s"), "H_q (7) must be divisible by H_kv (2)"),
    ("sfa_decode_ring_multi_slots", ("pool_s", "null_ws"),
     "pool: sink and window buffers must share shape[0] = S >= 1 (sink 5, window 7)"),
    ("sfa_decode_ring_multi_rows", ("misaligned", "null_ws"), "decode_multi: rows of every tensor must be 16-byte aligned"),
    ("sfa_decode_ring_tree", ("n65", "null_ws"), "decode_tree: a tree chunk holds at most 64 nodes (got n = 65)"),
    ("sfa_decode_ring_tree_slots", ("null_state", "null_slots"), "state: null device pointer"),
    ("sfa_decode_ring_tree_slots", ("null_slots", "null_cache"), "slots: null device pointer"),
    ("sfa_decode_ring_tree_slots", ("n65", "dtype"), "q, the cache buffers and k_new / v_new must share one dtype"),
    ("sfa_decode_ring_tree_slots", ("pool_s", "n65"),
     "pool: sink and window buffers must share shape[0] = S >= 1 (sink 5, window 7)"),
    ("sfa_decode_ring_tree_dyn", ("n65", "null_parent"), "decode_tree: a tree chunk holds at most 64 nodes (got n = 65)"),
    ("sfa_decode_ring_tree_rows", ("null_parent", "bstride"), "parent: null device pointer"),
    ("sfa_decode_ring_tree_rows", ("bstride", "null_ws"),
     "parent_bstride 2: 0 (one tree shared by the batch) or >= n = 3 (one row per sequence)"),
    ("sfa_decode_ring_ragged_slots", ("null_state", "null_slots"), "state: null device pointer"),
    ("sfa_decode_ring_ragged_slots", ("null_slots", "null_cu"), "slots: null device pointer"),
    ("sfa_decode_ring_ragged_slots", ("null_cu", "n_seq0"), "cu_q: null device pointer"),
    ("sfa_decode_ring_ragged_slots", ("n_seq0", "null_cache"), "decode_ragged: n_seq (0) must be at least 1"),
    ("sfa_decode_ring_ragged_slots", ("null_cache", "dtype"), "cache buffers: null tensor descriptor"),
    ("sfa_decode_ring_ragged_slots", ("pool_s", "not_packed"),
     "pool: sink and window buffers must share shape[0] = S >= 1 (sink 5, window 7)"),
    ("sfa_decode_ring_ragged_slots", ("not_packed", "short_ws"),
     "decode_ragged: q / k_new / v_new / o must be packed [1, H, T, D] (got shape[0] = 2)"),
    ("sfa_ring_commit_dyn", ("null_k_new", "null_count"), "k_new: null tensor descriptor"),
    ("sfa_ring_commit_rows", ("null_count", "null_state"), "count: null device pointer"),
    ("sfa_ring_commit_rows", ("null_state", "dtype"), "state: null device pointer"),
    ("sfa_ring_commit_slots", ("null_slots", "null_cache"), "slots: null device pointer"),
    ("sfa_ring_commit_slots", ("null_slots", "null_count"), "slots: null device pointer"),
    ("sfa_ring_commit_path_slots", ("null_slots", "null_state"), "slots: null device pointer"),
    ("sfa_ring_commit_path_slots", ("null_count", "bstride"), "count: null device pointer"),
    ("sfa_ring_commit_path_slots", ("n0", "null_path"), "ring_commit: the chunk needs at least one token"),
    ("sfa_ring_commit_path_rows", ("misaligned", "null_path"), "ring_commit: rows of every tensor must be 16-byte aligned"),
    ("sfa_ring_commit_path_dyn", ("null_path", "bstride"), "path: null device pointer"),
    ("sfa_ring_fill_varlen_slots", ("null_cache", "null_cu"), "sink_k: null tensor descriptor"),
    ("sfa_ring_fill_varlen_slots", ("null_cu", "null_state"), "cu_seqlens: null device pointer"),
    ("sfa_ring_fill_varlen_slots", ("null_state", "null_slots"), "state: null device pointer"),
    ("sfa_ring_fill_varlen_slots", ("null_slots", "n_seq0"), "slots: null device pointer"),
    ("sfa_ring_fill_varlen_slots", ("n_seq0", "dtype"), "n_seq must be >= 1 (got 0)"),
    ("sfa_ring_fill_varlen_slots", ("dtype", "pool_s"), "k / v and the cache buffers must share one dtype"),
    ("sfa_ring_fill_varlen_slots", ("pool_s", "misaligned"),
     "pool: sink and window buffers must share shape[0] = S >= 1 (sink 5, window 7)"),
]


@pytest.mark.parametrize("name,whiches,text", COMBINED, ids=[f"{n[4:]}-{'+'.join(w)}" for n, w, _ in COMBINED])
def test_of_two_defects_the_earlier_check_reports(name, whiches, text):
    assert call(name, **_both(name, *whiches)) == (-1, text)


def test_other_refusals_keep_their_status_and_text():
    assert call("sfa_ring_fill_varlen", nseq=3) == (-1, "n_seq (3) must match the cache buffers' batch (sink 2, window 2)")
    assert call("sfa_ring_fill_varlen", descs={"kp": BASE["kn"], "vp": BASE["vn"]}) == \
        (-1, "packed layout: k / v must be [1, H_kv, T, D] (batch dim 2)")
    assert call("sfa_decode_ring_step", wp=W) == (-1, "write slot 16 outside the 16 valid ring slots")
    assert call("sfa_decode_ring_multi", wl=3, wp=5) == (-1, "write_pos (5) must equal window_len (3) until the ring is full")
    assert call("sfa_decode_ring_multi", sl=NS + 1) == (-1, "sink_len 5 outside [0, 4]")
    assert call("sfa_decode_ring_multi_rows", descs=_swap("sfa_decode_ring_multi_slots", BASE, "sk", "sv", "wk", "wv") and
                {"sk": BASE["psk"], "sv": BASE["psv"], "wk": BASE["pwk"], "wv": BASE["pwv"]}) == \
        (-1, "sink / window buffers must be [B, H_kv, *, D] like k_new")            # the rows call wants B == S
    d20 = _descs(n=NN)
    d20 = {k: N.desc(t[..., :20]) for k, t in _KEEP[-1].items()}                     # head dim 20: 40-byte rows
    assert call("sfa_decode_ring_multi", descs=d20) == \
        (-2, "decode_multi: head dim 20 (40 bytes/row) must be a multiple of 16 bytes and <= 1024 bytes")
    assert call("sfa_ring_commit_dyn", descs=d20) == (-1, "ring_commit: K/V rows must be a multiple of 16 bytes (head dim 20)")
    s0 = _descs(s=0)
    pool0 = {k: s0[k] for k in POOL}
    assert call("sfa_decode_ring_step_slots", descs=pool0) == \
        (-1, "pool: the cache buffers need shape[0] = S slots, 1 <= S < 2^30 (got 0)")
    assert call("sfa_decode_ring_multi_slots", descs=pool0) == \
        (-1, "pool: sink and window buffers must share shape[0] = S >= 1 (sink 0, window 0)")
    assert call("sfa_ring_commit_slots", descs=pool0) == (-1, "pool: the ring needs shape[0] = S >= 1 slots (got 0)")
    assert call("sfa_ring_fill_varlen_slots", descs=pool0) == \
        (-1, "pool: sink and window buffers must share shape[0] = S >= 1 (sink 0, window 0)")


# calls on an empty shape that return SFA_OK without a launch (the ones that still launch a commit are GPU business):
# B = 0 everywhere but sfa_ring_commit_dyn / sfa_ring_commit_path_dyn; H_q = 0 where nothing is to be committed
B0, HQ0 = _descs(b=0), _descs(hq=0)
EMPTY_B = [n for n in ENTRY if n.startswith("sfa_decode") and n not in ("sfa_decode_ring_multi_dyn",
                                                                         "sfa_decode_ring_ragged_slots")] + \
    ["sfa_ring_commit_rows", "sfa_ring_commit_slots", "sfa_ring_commit_path_rows", "sfa_ring_commit_path_slots"]
EMPTY_H = [n for n in ENTRY if "_tree" in n or "_step" in n or n in ("sfa_decode", "sfa_decode_ring")]
EMPTY_H_NO_COMMIT = ["sfa_decode_ring_multi", "sfa_decode_ring_multi_dyn", "sfa_decode_ring_multi_rows",
                     "sfa_decode_ring_multi_slots"]


def test_empty_shapes_return_ok_without_a_launch():
    for name in EMPTY_B:
        pool = ENTRY[name][1] is POOL
        descs = {k: v for k, v in B0.items() if not (pool and k in POOL)}     # a pool keeps its S slots
        assert call(name, descs=descs) == (0, ""), name
    assert call("sfa_decode_ring_multi_dyn", descs=B0, commit=0) == (0, "")
    for name in EMPTY_H:
        assert call(name, descs=_swap(name, HQ0, "q", "o")) == (0, ""), name
    for name in EMPTY_H_NO_COMMIT:
        assert call(name, descs=_swap(name, HQ0, "q", "o"), commit=0) == (0, ""), name
