"""CPU-only characterisation of the argument checks of 33 sink + ring cache entry points of libsfa.so (the 23 calls on
16-bit contiguous caches and the ten calls on an FP8, a paged or a paged FP8 slot pool): a table of
entry point x defect, each cell the status code and the exact sfa_last_error() text; a second table of combined defects
that pins which message wins (the order of the checks); and the empty-shape calls that return SFA_OK without a launch.
Host tensors stand in for device memory as in tests/test_slots_host.py: every call here returns before any launch, so
nothing is dereferenced."""
import pytest
import torch

from sink_attention import _native as N

B, S, HQ, HKV, NN, D, NS, W, T = 2, 5, 8, 2, 3, 64, 4, 16, 6
PG, PER, NPG = 32, 2, 7                          # paged pools: page size, pages per slot (Wc = 64), pages of the pool
BF, FP, F32, FP8 = torch.bfloat16, torch.float16, torch.float32, torch.float8_e4m3fn


def _z(*shape, dtype=BF):
    return torch.zeros(*shape, dtype=dtype)


def _odd(*shape, dtype=BF):
    """130-byte rows: shape[3] = 64 columns of a 65-column buffer (unit last stride, row stride not a 16-byte multiple)"""
    return torch.zeros(*shape[:3], shape[3] + 1, dtype=dtype)[..., :shape[3]]


def _tensors(mk=_z, dtype=BF, b=B, s=S, hq=HQ, n=NN, t=T, pg=PG):
    """q / kn / vn / o: a chunk of n tokens for b batch rows; q1 / k1 / v1 / o1: one token; qp / kp / vp / op: a pack of
    t rows; sk .. wv: the cache of b rows; psk .. pwv: a pool of s slots; fsk .. fwv: that pool in FP8; gk / gv: the
    pages of a paged pool (its sinks are psk / psv), hk / hv: FP8 pages (sinks fsk / fsv)"""
    return dict(fsk=mk(s, HKV, NS, D, dtype=FP8), fsv=mk(s, HKV, NS, D, dtype=FP8), fwk=mk(s, HKV, W, D, dtype=FP8),
                fwv=mk(s, HKV, W, D, dtype=FP8), gk=mk(NPG, HKV, pg, D, dtype=dtype), gv=mk(NPG, HKV, pg, D, dtype=dtype),
                hk=mk(NPG, HKV, pg, D, dtype=FP8), hv=mk(NPG, HKV, pg, D, dtype=FP8),
                q=mk(b, hq, n, D, dtype=dtype), kn=mk(b, HKV, n, D, dtype=dtype), vn=mk(b, HKV, n, D, dtype=dtype),
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
BASE.update(dsk=BASE["psk"], dsv=BASE["psv"], dgk=BASE["gk"], dgv=BASE["gv"])    # the destination pool of the paged copy
_HOST = torch.zeros(64, dtype=torch.int32)      # stands in for state / slots / parent / path / count / cu: never read
P = _HOST.data_ptr()
WS = 1 << 20                                     # a 256-byte aligned address, never dereferenced
SCALARS = dict(aux=None, ws=None, wsb=0, scale=0.125, flags=0, stream=None, state=P, slots=P, parent=P, pstride=0,
               count=P, path=P, pathstride=0, cu=P, nseq=2, commit=1, sl=NS, wl=W, wp=0, cseq=P, kvs=P, table=P,
               tstride=PER, nslots=S, dstate=P, dslots=P, npairs=1, dtable=P, dtstride=PER)

# the argument list of every entry point in the names of BASE / SCALARS.  act: the activations an entry point takes
# (chunk, one token, pack or none); cache: the buffers of B rows, the pool, or a single key segment
CHUNK, ONE, PACK = ("q", "kn", "vn", "o"), ("q1", "k1", "v1", "o1"), ("qp", "kp", "vp", "op")
ROWS, POOL = ("sk", "sv", "wk", "wv"), ("psk", "psv", "pwk", "pwv")
POOL8, PAGED, PAGED8 = ("fsk", "fsv", "fwk", "fwv"), ("psk", "psv", "gk", "gv"), ("fsk", "fsv", "hk", "hv")


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

# the ten calls on an FP8, a paged and a paged FP8 pool: the packed step, the packed commit, the slot prefill (and the
# paged copy, which takes two pools and no activations).  ENTRY stays the 23 calls on 16-bit contiguous caches
POOL_ENTRY = {}
_STEP = _DYN + " parent cseq commit state slots cu nseq"
_CMP = _CM + " path cu nseq state slots"
_FILL = "{sk} {sv} {wk} {wv} {kn} {vn} cu nseq state slots"
COPY = "sfa_ring_copy_paged_slots"
for _kind, _cache, _tail in (("fp8", POOL8, " kvs"), ("paged", PAGED, " table tstride{n}"),
                             ("paged_fp8", PAGED8, " table tstride{n} kvs")):
    POOL_ENTRY[f"sfa_decode_ring_ragged_{_kind}_slots"] = (PACK, _cache, _sig(PACK, _cache, _STEP + _tail.format(n="")))
    POOL_ENTRY[f"sfa_ring_commit_path_ragged_{_kind}_slots"] = (PACK, _cache, _sig(PACK, _cache,
                                                                                    _CMP + _tail.format(n=" nslots"), "stream"))
    POOL_ENTRY[f"sfa_ring_fill_varlen_{_kind}_slots"] = (PACK, _cache, _sig(PACK, _cache, _FILL + _tail.format(n=""), "stream"))
POOL_ENTRY[COPY] = ((), PAGED, "psk psv gk gv state dsk dsv dgk dgv dstate slots dslots npairs table tstride dtable dtstride "
                    "stream".split())
NEW = list(POOL_ENTRY)
ALL = {**ENTRY, **POOL_ENTRY}
assert len(NEW) == 10 and len(ALL) == 33


def call(name, descs=None, **scalars):
    """Run entry point `name` on BASE with `descs` (name -> descriptor or None) and `scalars` replaced; returns
    (status, error text)."""
    d = dict(BASE, **(descs or {}))
    s = dict(SCALARS, **scalars)
    lib = N.lib()
    st = getattr(lib, name)(*[d[a] if a in d else s[a] for a in ALL[name][2]])
    return st, lib.sfa_last_error().decode()


def _swap(name, other, *roles):
    """the entry point's tensors of the given roles (q, kn, vn, o, sk, sv, wk, wv) taken from the descriptor set `other`"""
    act, cache, _ = ALL[name]
    names = dict(zip(("q", "kn", "vn", "o", "sk", "sv", "wk", "wv"), act + cache))
    return {names[r]: (other[names[r]] if other is not None else None) for r in roles}


HALF, HQ7, N0, N65, ODD, S7 = (_descs(dtype=FP), _descs(hq=7), _descs(n=0, t=0), _descs(n=65), _descs(mk=_odd),
                               _descs(s=7))
B2PACK = {"qp": BASE["q"], "kp": BASE["kn"], "vp": BASE["vn"], "op": BASE["o"]}    # [2, H, 3, D] where a pack belongs
# the pools' own: fp32 everywhere, pages of 48 / 16 / 64 rows, head dim 48 (the first 48 columns of every tensor)
FLOAT, PG48, PG16, PG64 = _descs(dtype=F32), _descs(pg=48), _descs(pg=16), _descs(pg=64)
D48 = {k: N.desc(t[..., :48]) for k, t in _tensors().items()}
_KEEP.append(D48)
ALL8 = ("q", "kn", "vn", "o", "sk", "sv", "wk", "wv")


def _has(name, arg):
    return arg in ALL[name][2]


def _kind(name):
    """(FP8?, paged?) of one of the ten pool entry points; (False, False) for the 23 others"""
    return name in NEW and "fp8_slots" in name, name in NEW and "_paged_" in name


def _need(name):
    """the workspace size the entry point asks for at BASE"""
    lib = N.lib()
    act = ALL[name][0]
    if act is ONE:
        nkv = NS if name == "sfa_decode" else NS + W
        return lib.sfa_decode_workspace_bytes(B, HQ, HKV, nkv, D, 2)
    if act is PACK:
        return lib.sfa_decode_ragged_workspace_bytes(2, HQ, HKV, T, NS + (PER * PG if _kind(name)[1] else W), D, 2)
    return lib.sfa_decode_multi_workspace_bytes(B, HQ, HKV, NN, NS + W + NN, D, 2)


def _copy_defect(which):
    """defect() of sfa_ring_copy_paged_slots: two pools (psk psv gk gv -> dsk dsv dgk dgv), no activations"""
    pool = ("psk", "psv", "gk", "gv", "dsk", "dsv", "dgk", "dgv")
    both = lambda other: {k: other[k[1:] if k[0] == "d" else k] for k in pool}
    return {"null_state": dict(state=None), "null_slots": dict(slots=None), "null_cache": dict(descs={"psk": None}),
            "null_table": dict(table=None), "table_stride0": dict(tstride=0),
            "page_npo2": dict(descs={"gk": PG48["gk"], "gv": PG48["gv"]}),
            "page_small": dict(descs={"gk": PG16["gk"], "gv": PG16["gv"]}),
            "cache_dtype": dict(descs={"gk": BASE["hk"], "gv": BASE["hv"]}),      # FP8 pages beside 16-bit sinks
            "head_dim": dict(descs=both(D48)), "fp32": dict(descs=both(FLOAT)),
            "copy_page_sizes": dict(descs={"dgk": PG64["gk"], "dgv": PG64["gv"]})}.get(which)


def _pool_defect(name, which):
    """the defects that only the ten pool entry points can have"""
    fp8, paged = _kind(name)
    if which in ("page_npo2", "page_small"):
        return dict(descs=_swap(name, PG48 if which == "page_npo2" else PG16, "wk", "wv")) if paged else None
    if which == "table_stride0":
        return dict(tstride=0) if paged else None
    if which == "null_table":
        return dict(table=None) if paged else None
    if which == "cache_dtype":      # 16-bit buffers where FP8 ones belong, and the other way round
        other = {POOL8: POOL, PAGED8: PAGED, PAGED: PAGED8}[ALL[name][1]]
        return dict(descs={c: BASE[o] for c, o in zip(ALL[name][1], other)})
    if which == "act_dtype":        # k_new in f16 beside bf16 q / v_new
        return dict(descs=_swap(name, HALF, "kn")) if fp8 else None
    if which == "head_dim":
        return dict(descs=_swap(name, D48, *ALL8))
    if which == "fp32":             # fp32 activations; a 16-bit paged pool shares their dtype
        return dict(descs=_swap(name, FLOAT, "q", "kn", "vn", "o") if fp8 else _swap(name, FLOAT, *ALL8))
    if which == "force_generic":
        return dict(flags=N.FLAG_FORCE_GENERIC) if _has(name, "flags") else None
    return None                     # copy_page_sizes: the copy alone


POOL_DEFECTS = ("page_npo2", "page_small", "table_stride0", "null_table", "cache_dtype", "act_dtype", "head_dim", "fp32",
                "force_generic", "copy_page_sizes")


def defect(name, which):
    """keyword arguments of call() that plant defect `which` in entry point `name`, or None where it does not apply"""
    commit, fill = name.startswith("sfa_ring_commit"), name.startswith("sfa_ring_fill")
    chunkless = name in ("sfa_decode", "sfa_decode_ring")
    if name == COPY:
        return _copy_defect(which)
    if which in POOL_DEFECTS:
        return _pool_defect(name, which) if name in NEW else None
    if which == "dtype" and _kind(name)[0] and (commit or fill):
        return None                 # k / v of one 16-bit dtype are what an FP8 commit or prefill takes: see act_dtype
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
        if fill or ALL[name][0] is ONE:
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
        return dict(descs=_swap(name, S7, "wk", "wv")) if ALL[name][1] in (POOL, POOL8) and not commit else None
    if which == "null_ws":
        return dict(ws=None, wsb=0) if _has(name, "ws") else None
    if which == "short_ws":
        return dict(ws=WS, wsb=_need(name) - 1) if _has(name, "ws") else None
    if which == "unaligned_ws":
        return dict(ws=WS + 16, wsb=1 << 30) if _has(name, "ws") else None
    if which == "not_packed":
        return dict(descs=B2PACK) if name == "sfa_decode_ring_ragged_slots" or name in NEW else None
    if which == "n_seq0":
        return dict(nseq=0) if _has(name, "nseq") else None
    if which in ("null_parent", "null_count", "null_path", "null_cu"):      # only used in COMBINED
        arg = which[5:]
        return {arg: None} if _has(name, arg) else None
    raise KeyError(which)


DEFECTS = ("null_state", "null_slots", "null_cache", "null_k_new", "dtype", "heads", "n0", "n65", "bstride",
           "misaligned", "pool_s", "null_ws", "short_ws", "unaligned_ws", "not_packed", "n_seq0") + POOL_DEFECTS

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

# the ten pool entry points.  Three texts recur under the call's own name `who`
_FP8_ONLY = '{who}: the cache buffers must be FP8 (e4m3)'
_PAGE = '{who}: the page size (window_k shape[2] = {p}) must be a power of two and at least 32'
_STRIDE = '{who}: table_stride (0) must be at least 1 (Wc = table_stride * P)'
_SERVES = {(True, False): '{who}: an FP8 pool serves bf16 / f16 activations at head dims 64 / 80 / 96 / 128 ',
           (False, True): '{who}: a paged pool serves bf16 / f16 at head dims 64 / 80 / 96 / 128 ',
           (True, True): '{who}: a paged FP8 pool serves bf16 / f16 activations at head dims 64 / 80 / 96 / 128 '}


def _pool_rows(who, fp8, paged, rows):
    """the cells every call of one pool kind shares, under its name in the messages, joined to its own `rows`"""
    serves = _SERVES[fp8, paged].format(who=who)
    out = dict(rows, head_dim=(-2, serves + '(got dtype 2, head dim 48)'), fp32=(-2, serves + '(got dtype 0, head dim 64)'))
    out["cache_dtype"] = (-1, _FP8_ONLY.format(who=who) if fp8 else 'window_k: unknown dtype 3')
    if paged:
        out.update(page_npo2=(-1, _PAGE.format(who=who, p=48)), page_small=(-1, _PAGE.format(who=who, p=16)),
                   table_stride0=(-1, _STRIDE.format(who=who)), null_table=(-1, 'page_table: null device pointer'))
    if "null_ws" in rows:
        out["force_generic"] = (-2, serves + '(got dtype 2, head dim 64, SFA_FLAG_FORCE_GENERIC)')
    return out


def _step_rows(need, fp8, who):
    ws = f'decode_ragged workspace: need {need} bytes, 256-byte aligned '
    rows = {
        "null_state": (-1, 'state: null device pointer'),
        "null_slots": (-1, 'slots: null device pointer'),
        "null_cache": (-1, 'cache buffers: null tensor descriptor'),
        "null_k_new": (-1, 'k_new: null tensor descriptor'),
        "dtype": (-1, f'{who}: q and k_new / v_new must share one dtype' if fp8 else
                  'q, the cache buffers and k_new / v_new must share one dtype'),
        "heads": (-1, 'H_q (7) must be divisible by H_kv (2)'),
        "n0": (-1, 'decode_multi: the chunk needs at least one token'),
        "misaligned": (-1, 'decode_multi: rows of every tensor must be 16-byte aligned'),
        "null_ws": (-3, ws + '(got 0 at (nil))'),
        "short_ws": (-3, ws + f'(got {need - 1} at 0x100000)'),
        "unaligned_ws": (-3, ws + '(got 1073741824 at 0x100010)'),
        "not_packed": (-1, 'decode_ragged: q / k_new / v_new / o must be packed [1, H, T, D] (got shape[0] = 2)'),
        "n_seq0": (-1, 'decode_ragged: n_seq (0) must be at least 1'),
    }
    if fp8:
        rows["act_dtype"] = (-1, 'k_new and v_new differ in dtype')
    return rows


def _commit_rows(fp8):
    rows = {
        "null_state": (-1, 'state: null device pointer'),
        "null_slots": (-1, 'slots: null device pointer'),
        "null_cache": (-1, 'window_k: null tensor descriptor'),
        "null_k_new": (-1, 'k_new: null tensor descriptor'),
        "n0": (-1, 'ring_commit: the chunk needs at least one token'),
        "misaligned": (-1, 'ring_commit: rows of every tensor must be 16-byte aligned'),
        "not_packed": (-1, 'ring_commit_ragged: k_new / v_new must be packed [1, H_kv, T, D] (got shape[0] = 2)'),
        "n_seq0": (-1, 'ring_commit_ragged: n_seq (0) must be at least 1'),
    }
    rows.update({"act_dtype": (-1, 'k_new and v_new differ in dtype')} if fp8 else
                {"dtype": (-1, 'k_new / v_new and the ring must share one dtype')})
    return rows


def _fill_rows(fp8):
    rows = {
        "null_state": (-1, 'state: null device pointer'),
        "null_slots": (-1, 'slots: null device pointer'),
        "null_cache": (-1, 'sink_k: null tensor descriptor'),
        "null_k_new": (-1, 'k: null tensor descriptor'),
        "misaligned": (-1, 'ring_fill_varlen: rows of every tensor must be 16-byte aligned'),
        "not_packed": (-1, 'packed layout: k / v must be [1, H_kv, T, D] (batch dim 2)'),
        "n_seq0": (-1, 'n_seq must be >= 1 (got 0)'),
    }
    rows.update({"act_dtype": (-1, 'k and v differ in dtype')} if fp8 else
                {"dtype": (-1, 'k / v and the cache buffers must share one dtype')})
    return rows


_POOL_S = (-1, 'pool: sink and window buffers must share shape[0] = S >= 1 (sink 5, window 7)')
for _sfx, _fp8, _paged in (("fp8", True, False), ("paged", False, True), ("paged_fp8", True, True)):
    _own = {} if _paged else {"pool_s": _POOL_S}          # a paged ring takes S from the sinks
    EXPECT[f"sfa_decode_ring_ragged_{_sfx}_slots"] = _pool_rows(
        f"decode_ragged_{_sfx}", _fp8, _paged, dict(_step_rows(26112 if _paged else 13312, _fp8, f"decode_ragged_{_sfx}"), **_own))
    EXPECT[f"sfa_ring_commit_path_ragged_{_sfx}_slots"] = _pool_rows(f"ring_commit_ragged_{_sfx}", _fp8, _paged,
                                                                     _commit_rows(_fp8))
    EXPECT[f"sfa_ring_fill_varlen_{_sfx}_slots"] = _pool_rows(f"ring_fill_varlen_{_sfx}", _fp8, _paged,
                                                              dict(_fill_rows(_fp8), **_own))
EXPECT[COPY] = dict(_pool_rows("ring_copy_paged", False, True, {
    "null_state": (-1, 'src_state: null device pointer'),
    "null_slots": (-1, 'src_slots: null device pointer'),
    "null_cache": (-1, 'src_sink_k: null tensor descriptor'),
    "copy_page_sizes": (-1, 'ring_copy_paged: the pools differ in page size (src 32, dst 64)'),
}), cache_dtype=(-1, 'ring_copy_slots: src_window_k and src_sink_k differ in dtype (the eight buffers must share one)'))

CELLS = [(name, which) for name in ALL for which in DEFECTS if defect(name, which) is not None]


def test_the_table_covers_every_applicable_cell():
    assert {(n, w) for n, cells in EXPECT.items() for w in cells} == set(CELLS)
    for which in DEFECTS:                      # every defect has an entry point that can have it
        assert any(w == which for _, w in CELLS), which


@pytest.mark.parametrize("name", list(ALL))
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


# the same for the ten pool entry points, with the status: a paged call checks its pages and table first (paged_ring),
# then the null device arrays, then n_seq, then what its contiguous sibling checks; an FP8 call says what it serves where
# its sibling checks the head dim, a 16-bit paged call after every check of its sibling
_RAG, _CMT, _FIL = "sfa_decode_ring_ragged_%s_slots", "sfa_ring_commit_path_ragged_%s_slots", "sfa_ring_fill_varlen_%s_slots"
COMBINED_POOL = [
    (_RAG % "paged", ("cache_dtype", "null_table"), -1, "window_k: unknown dtype 3"),
    (_RAG % "paged", ("null_table", "page_npo2"), -1, "page_table: null device pointer"),
    (_RAG % "paged", ("page_small", "table_stride0"), -1, _PAGE.format(who="decode_ragged_paged", p=16)),
    (_RAG % "paged", ("table_stride0", "null_state"), -1, _STRIDE.format(who="decode_ragged_paged")),
    (_RAG % "paged", ("null_state", "null_slots"), -1, "state: null device pointer"),
    (_RAG % "paged", ("null_slots", "null_cu"), -1, "slots: null device pointer"),
    (_RAG % "paged", ("null_cu", "n_seq0"), -1, "cu_q: null device pointer"),
    (_RAG % "paged", ("n_seq0", "null_cache"), -1, "decode_ragged: n_seq (0) must be at least 1"),
    (_RAG % "paged", ("not_packed", "force_generic"), -1,
     "decode_ragged: q / k_new / v_new / o must be packed [1, H, T, D] (got shape[0] = 2)"),
    (_RAG % "paged", ("force_generic", "null_ws"), -2,
     _SERVES[False, True].format(who="decode_ragged_paged") + "(got dtype 2, head dim 64, SFA_FLAG_FORCE_GENERIC)"),
    (_RAG % "paged_fp8", ("null_table", "null_state"), -1, "page_table: null device pointer"),
    (_RAG % "paged_fp8", ("page_npo2", "act_dtype"), -1, _PAGE.format(who="decode_ragged_paged_fp8", p=48)),
    (_RAG % "paged_fp8", ("cache_dtype", "dtype"), -1, _FP8_ONLY.format(who="decode_ragged_paged_fp8")),
    (_RAG % "paged_fp8", ("dtype", "heads"), -1, "decode_ragged_paged_fp8: q and k_new / v_new must share one dtype"),
    (_RAG % "paged_fp8", ("not_packed", "force_generic"), -2,
     _SERVES[True, True].format(who="decode_ragged_paged_fp8") + "(got dtype 2, head dim 64, SFA_FLAG_FORCE_GENERIC)"),
    (_RAG % "fp8", ("null_state", "null_slots"), -1, "state: null device pointer"),
    (_RAG % "fp8", ("n_seq0", "cache_dtype"), -1, "decode_ragged: n_seq (0) must be at least 1"),
    (_RAG % "fp8", ("cache_dtype", "n0"), -1, _FP8_ONLY.format(who="decode_ragged_fp8")),
    (_RAG % "fp8", ("pool_s", "not_packed"), -1, _POOL_S[1]),
    (_RAG % "fp8", ("pool_s", "force_generic"), -1, _POOL_S[1]),
    (_RAG % "fp8", ("not_packed", "force_generic"), -2,
     _SERVES[True, False].format(who="decode_ragged_fp8") + "(got dtype 2, head dim 64, SFA_FLAG_FORCE_GENERIC)"),
    (_RAG % "fp8", ("head_dim", "null_ws"), -2,
     _SERVES[True, False].format(who="decode_ragged_fp8") + "(got dtype 2, head dim 48)"),
    (_CMT % "paged", ("page_npo2", "null_slots"), -1, _PAGE.format(who="ring_commit_ragged_paged", p=48)),
    (_CMT % "paged", ("null_slots", "null_cu"), -1, "slots: null device pointer"),
    (_CMT % "paged", ("n_seq0", "null_count"), -1, "ring_commit_ragged: n_seq (0) must be at least 1"),
    (_CMT % "paged", ("null_count", "null_state"), -1, "count: null device pointer"),
    (_CMT % "paged_fp8", ("table_stride0", "cache_dtype"), -1, _STRIDE.format(who="ring_commit_ragged_paged_fp8")),
    (_CMT % "paged_fp8", ("cache_dtype", "n0"), -1, _FP8_ONLY.format(who="ring_commit_ragged_paged_fp8")),
    (_CMT % "fp8", ("null_slots", "null_cu"), -1, "slots: null device pointer"),
    (_CMT % "fp8", ("null_state", "cache_dtype"), -1, "state: null device pointer"),
    (_CMT % "fp8", ("fp32", "null_state"), -1, "state: null device pointer"),
    (_FIL % "paged", ("table_stride0", "null_cu"), -1, _STRIDE.format(who="ring_fill_varlen_paged")),
    (_FIL % "paged", ("null_cu", "n_seq0"), -1, "cu_seqlens: null device pointer"),
    (_FIL % "paged_fp8", ("page_npo2", "act_dtype"), -1, _PAGE.format(who="ring_fill_varlen_paged_fp8", p=48)),
    (_FIL % "paged_fp8", ("n_seq0", "cache_dtype"), -1, "n_seq must be >= 1 (got 0)"),
    (_FIL % "fp8", ("cache_dtype", "pool_s"), -1, _FP8_ONLY.format(who="ring_fill_varlen_fp8")),
    (_FIL % "fp8", ("pool_s", "fp32"), -1, _POOL_S[1]),
    (COPY, ("null_table", "page_npo2"), -1, "page_table: null device pointer"),
    (COPY, ("page_npo2", "copy_page_sizes"), -1, _PAGE.format(who="ring_copy_paged", p=48)),
    (COPY, ("copy_page_sizes", "null_state"), -1, "ring_copy_paged: the pools differ in page size (src 32, dst 64)"),
    (COPY, ("fp32", "null_state"), -1, "src_state: null device pointer"),
]


@pytest.mark.parametrize("name,whiches,status,text", COMBINED_POOL,
                         ids=[f"{n[4:]}-{'+'.join(w)}" for n, w, _, _ in COMBINED_POOL])
def test_of_two_pool_defects_the_earlier_check_reports(name, whiches, status, text):
    assert call(name, **_both(name, *whiches)) == (status, text)


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
