"""Host-side checks of the packed ragged step (sfa_decode_ring_ragged_slots, SinkCacheLayer.ragged_step_dyn /
packed_positions): exports, workspace sizing, argument checks that launch nothing, the torch-op position map, and the CPU
proof that the probe inputs of tests/test_gpu_ragged_step.py::test_mask_edge_probes cannot pass with a one-key mask
error (oracle against mutated oracle, as tests/test_probe_inputs.py does for the other calls)."""
import ctypes
import functools

import pytest
import torch

import probe_inputs as P
from sink_attention import SinkAttentionCache, SinkCacheLayer
from test_gpu_decode_multi import TOL, _oracle_rows
from test_probe_inputs import factors, masked_attention

HKV, NS = 2, 4
# (history length, chunk length) per sequence at Wc = 16 and 48: diagonals on a tile edge (n = 32, 33) and on a row-block
# edge (G n = 32: n = 4 at G = 8, n = 32 at G = 1); the oldest visible ring key and the evicted one at ring slots 0 and
# Wc - 1 (history ns + Wc: a full ring that has not wrapped; ns + Wc + 5: wrapped); a ring shorter than the chunk; a ring
# that is partly filled
PROBE_SEQS = {16: [(20, 4), (25, 33), (20, 32), (9, 17), (52, 1)], 48: [(52, 4), (57, 33), (52, 32), (30, 49), (20, 5)]}
PROBE_TYPES = [("bf16", 64, 8), ("bf16", 128, 1), ("fp16", 80, 8), ("fp32", 48, 1), ("fp32", 64, 8)]
@functools.lru_cache(maxsize=None)
def probe_pack(dt, D, G, W):
    """chunk_probe inputs per sequence of PROBE_SEQS[W], packed: (q, k, v [1, H, T, D], s_aux, [(k, v) history per
    sequence], chunk lengths, {i: f64 reference rows}, per-sequence probe dicts with the call's s_aux)"""
    dtype = P._DT[dt]
    qs, ks, vs, hist, ref, prs = [], [], [], [], {}, []
    for i, (L, n) in enumerate(PROBE_SEQS[W]):
        prs.append(P.chunk_probe(1, HKV * G, HKV, D, NS, W, L, n, dtype, seed=600 + i, aux=True))
    sa = prs[0]["s_aux"]                            # one s_aux per call: the first sequence's
    for i, (L, n) in enumerate(PROBE_SEQS[W]):
        pr = prs[i]
        pr["s_aux"] = sa
        if i + 1 < len(prs):
            # the pack edge: in the last q head of every KV group the LAST row of sequence i aims at the FIRST chunk key of
            # sequence i + 1 (q = a * its code), which it must not see
            L2 = PROBE_SEQS[W][i + 1][0]
            pr["q"][0, G - 1::G, L + n - 1] = (pr["a"] * prs[i + 1]["k"][0, :, L2].float()).to(dtype)
        qs.append(pr["q"][:, :, L:]), ks.append(pr["k"][:, :, L:]), vs.append(pr["v"][:, :, L:])
        hist.append((pr["k"][:, :, :L], pr["v"][:, :, :L]))
        ref[i] = _oracle_rows(pr["q"], pr["k"], pr["v"], sa, L, NS, W, n, slice(0, 1))
    cat = lambda ts: torch.cat(ts, dim=2)
    return cat(qs), cat(ks), cat(vs), sa, hist, [n for _, n in PROBE_SEQS[W]], ref, prs


# ------------------------------------------------------------------------------------------------ exports, workspace
def test_library_exports_the_ragged_step():
    from sink_attention import _native
    lib = _native.lib()
    assert hasattr(lib, "sfa_decode_ring_ragged_slots") and hasattr(lib, "sfa_decode_ragged_workspace_bytes")
    assert lib.sfa_abi_version() == 2
    assert hasattr(SinkCacheLayer, "ragged_step_dyn") and hasattr(SinkAttentionCache, "ragged_step_dyn")
    assert hasattr(SinkCacheLayer, "packed_positions") and hasattr(SinkAttentionCache, "packed_positions")


def test_workspace_needs_no_gpu_and_rejects_unsupported_shapes():
    from sink_attention import _native
    ws = _native.lib().sfa_decode_ragged_workspace_bytes
    assert ws(8, 64, 8, 519, 4 + 4096, 64, 2) >= 64 * 519 * (64 + 2) * 4     # at least one partial per packed row
    assert ws(1, 4, 4, 3, 100, 20, 2) == 0        # 40-byte rows
    assert ws(1, 4, 4, 3, 100, 512, 0) == 0       # 2 KiB rows
    assert ws(1, 6, 4, 3, 100, 64, 2) == 0        # H_q % H_kv != 0
    assert ws(0, 4, 4, 3, 100, 64, 2) == 0 and ws(1, 4, 4, 0, 100, 64, 2) == 0
    assert ws(2048, 8, 2, 4096, 4100, 64, 2) > 0  # no cap on n_seq below 1024


@pytest.mark.parametrize("n_seq,Hq,Hkv,D,dt", [(8, 64, 8, 64, 2), (1, 4, 4, 128, 1), (300, 16, 2, 80, 2), (5, 8, 1, 48, 0)])
def test_workspace_is_monotonic_in_T_and_in_the_cache_size(n_seq, Hq, Hkv, D, dt):
    from sink_attention import _native
    ws = _native.lib().sfa_decode_ragged_workspace_bytes
    prev = 0
    for T in list(range(1, 300)) + list(range(300, 9000, 37)):
        w = ws(n_seq, Hq, Hkv, T, 4 + 4096, D, dt)
        assert w > 0 and w >= prev, ("T", T, w, prev)
        prev = w
    prev = 0
    for nkv in list(range(1, 700)) + list(range(700, 20000, 53)):
        w = ws(n_seq, Hq, Hkv, 160, nkv, D, dt)
        assert w > 0 and w >= prev, ("Nkv_cache", nkv, w, prev)
        prev = w


# ------------------------------------------------------------------------------------------------ C ABI checks
def _abi_args(T=12, Hq=8, Hkv=2, D=64, ns=4, W=16, S=3, B=1):
    """Host tensors: the C entry point validates them without touching the device and returns before any launch."""
    from sink_attention import _native as N
    mk = lambda *s: torch.zeros(*s, dtype=torch.bfloat16)
    t = dict(q=mk(B, Hq, T, D), sk=mk(S, Hkv, ns, D), sv=mk(S, Hkv, ns, D), wk=mk(S, Hkv, W, D), wv=mk(S, Hkv, W, D),
             kn=mk(B, Hkv, T, D), vn=mk(B, Hkv, T, D), o=mk(B, Hq, T, D))
    return N, t, {k: N.desc(v) for k, v in t.items()}


def _call(N, d, n_seq=3, state=1, slots=1, cu=1, ws=None, ws_bytes=0, scale=0.125, **over):
    """state / slots / cu: any non-null value stands for a device pointer (nothing is launched, so it is never read)"""
    d = dict(d, **over)
    p = lambda x: ctypes.c_void_p(0x1000) if x else None
    return N.lib().sfa_decode_ring_ragged_slots(d["q"], d["sk"], d["sv"], d["wk"], d["wv"], d["kn"], d["vn"], d["o"], None,
                                                0, p(state), p(slots), p(cu), n_seq, ws, ws_bytes, scale, 0, None)


def test_c_abi_rejects_bad_arguments_before_any_launch():
    N, t, d = _abi_args()
    lib = N.lib()
    err = lib.sfa_last_error
    assert _call(N, d, state=0) == -1 and b"state" in err()
    assert _call(N, d, slots=0) == -1 and b"slots" in err()
    assert _call(N, d, cu=0) == -1 and b"cu_q" in err()
    assert _call(N, d, n_seq=0) == -1 and b"n_seq" in err()
    _, _, d2 = _abi_args(B=2)
    assert _call(N, d2) == -1 and b"[1, H, T, D]" in err()                                  # not a pack
    _, _, d3 = _abi_args(T=13)
    assert _call(N, d, kn=d3["kn"], vn=d3["vn"]) == -1 and b"k_new" in err()                # k_new does not share T
    assert _call(N, d, o=d3["o"]) == -1                                                     # o does not share T
    _, _, d4 = _abi_args(S=4)
    assert _call(N, d, wk=d4["wk"], wv=d4["wv"]) == -1 and b"pool" in err()                 # pool buffers do not share S
    _, _, d5 = _abi_args(Hq=6, Hkv=4)
    assert _call(N, d5) == -1 and b"divisible" in err()
    _, _, d6 = _abi_args(D=20)
    assert _call(N, d6) == -2                                                               # 40-byte rows
    _, t7, _ = _abi_args(D=72)
    assert _call(N, d, q=N.desc(t7["q"][..., 4:68])) == -1 and b"aligned" in err()          # data pointer off by 8 bytes
    mk = lambda *s: torch.zeros(*s, dtype=torch.float16)
    assert _call(N, d, kn=N.desc(mk(1, 2, 12, 64)), vn=N.desc(mk(1, 2, 12, 64))) == -1 and b"dtype" in err()
    assert _call(N, d, scale=float("nan")) == -1
    # every argument valid, no workspace / a short one / a misaligned one: SFA_ERR_WORKSPACE, the last check before the launch
    need = lib.sfa_decode_ragged_workspace_bytes(3, 8, 2, 12, 20, 64, 2)
    assert need > 0
    assert _call(N, d) == -3 and b"workspace" in err()
    assert _call(N, d, ws=ctypes.c_void_p(0x10000), ws_bytes=need - 1) == -3
    assert _call(N, d, ws=ctypes.c_void_p(0x10010), ws_bytes=need) == -3


# ------------------------------------------------------------------------------------------------ Python entry points
def _cpu_pool(S=5, W=16):
    layer = SinkCacheLayer(NS, W)
    layer.init_pool(S, HKV, 64, torch.bfloat16, "cpu")
    return layer


def test_python_entry_points_refuse_cpu_tensors_and_a_cache_without_a_pool():
    mk = lambda h, T=6: torch.zeros(1, h, T, 64, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _cpu_pool().ragged_step_dyn(mk(8), mk(2), mk(2), [0, 2, 6], [0, 1])
    with pytest.raises(RuntimeError, match="needs a pool"):
        SinkCacheLayer(NS, 16).ragged_step_dyn(mk(8), mk(2), mk(2), [0, 2, 6], [0, 1])
    with pytest.raises(RuntimeError, match="needs a pool"):
        SinkCacheLayer(NS, 16).packed_positions([0, 2, 6], [0, 1], 6)
    cache = SinkAttentionCache(num_sink=NS, window_size=16)
    with pytest.raises(RuntimeError, match="needs a pool"):
        cache.ragged_step_dyn(mk(8), mk(2), mk(2), [0, 2, 6], [0, 1], layer_idx=0)
    layer = SinkCacheLayer(NS, 16)      # per-sequence rows without a pool (prefill_varlen's mode) are not a pool either
    layer.is_initialized = layer.prefilled = layer._per_seq = True
    with pytest.raises(RuntimeError, match="needs a pool"):
        layer.ragged_step_dyn(mk(8), mk(2), mk(2), [0, 2, 6], [0, 1])


def test_packed_positions_against_a_python_loop():
    layer = _cpu_pool(S=5)
    layer._dev_state[:, 3] = torch.tensor([100, 7, 0, 33, 2500], dtype=torch.int32)
    cu, slots, T = [0, 1, 4, 4, 12, 17], [3, -1, 1, 4, 0], 24      # an inactive sequence, an empty one, a padded tail
    want = [-1] * T
    for i, s in enumerate(slots):
        for t in range(cu[i + 1] - cu[i]):
            want[cu[i] + t] = int(layer._dev_state[s, 3]) + t if s >= 0 else -1
    assert layer.packed_positions(cu, slots, T).tolist() == want
    got = layer.packed_positions(torch.tensor(cu, dtype=torch.int32), torch.tensor(slots, dtype=torch.int32), T)
    assert got.tolist() == want and want[0] == 33 and want[1:4] == [-1] * 3 and want[4] == 2500 and want[17:] == [-1] * 7
    cache = SinkAttentionCache(num_sink=NS, window_size=16)
    cache.init_pool(5, HKV, 64, torch.bfloat16, "cpu")
    assert cache.packed_positions([0, 3], [9], 4).tolist() == [-1] * 4      # a slot outside the pool is inactive
    assert cache.packed_positions([0, 3], [2], 4).tolist() == [0, 1, 2, -1]


# ------------------------------------------------------------------------------------------------ the CPU proof
def _mutants(W):
    """per sequence i of the probe pack: the true mask [n, L + n + 1] over (history, chunk, the first chunk token of the
    next sequence in the pack) and the one-key mutants at each edge"""
    seqs = PROBE_SEQS[W]
    out = []
    for i, (L, n) in enumerate(seqs):
        pos, j = torch.arange(n) + L, torch.arange(L + n + 1)
        true = (j[None, :] <= pos[:, None]) & ((j[None, :] < NS) | (j[None, :] >= pos[:, None] - W + 1))
        r = torch.arange(n)
        mut = {}
        m = true.clone(); m[r, pos] = False; mut["diagonal lost"] = m
        if n > 1:
            m = true.clone(); m[r[:-1], pos[:-1] + 1] = True; mut["later chunk token"] = m
        old = pos - W + 1                   # the oldest window key of each row, where it is not a sink row
        ok = old >= NS
        if ok.any():
            m = true.clone(); m[r[ok], old[ok]] = False; mut["oldest window key lost"] = m
        ok = old - 1 >= NS
        if ok.any():
            m = true.clone(); m[r[ok], old[ok] - 1] = True; mut["key behind the window"] = m
        if i + 1 < len(seqs):
            m = true.clone(); m[n - 1, L + n] = True; mut["first row of the next sequence"] = m
        out.append((true, mut))
    return out


@pytest.mark.parametrize("W", [16, 48])
@pytest.mark.parametrize("dt,D,G", PROBE_TYPES)
def test_a_one_key_mask_error_moves_a_probe_row_tenfold(dt, D, G, W):
    """Oracle against mutated oracle on the inputs of test_gpu_ragged_step.py::test_mask_edge_probes: a one-key error at
    each edge moves some row of the pack by at least ten times TOL, and the unmutated oracle passes (factor 0 against
    itself; it is also the reference of the GPU test).  probe_inputs.amplitude(D) = 2.0 is enough at these shapes."""
    q, k, v, sa, hist, lengths, ref, prs = probe_pack(dt, D, G, W)
    tol = (TOL[P._DT[dt]], 0.0)
    cu = [0]
    for n in lengths:
        cu.append(cu[-1] + n)
    best = {}
    for i, (true, muts) in enumerate(_mutants(W)):
        L, n = PROBE_SEQS[W][i]
        nxt = k[:, :, cu[i + 1]:cu[i + 1] + 1] if i + 1 < len(lengths) else torch.zeros_like(k[:, :, :1])
        nxv = v[:, :, cu[i + 1]:cu[i + 1] + 1] if i + 1 < len(lengths) else torch.zeros_like(v[:, :, :1])
        inp = dict(q=prs[i]["q"][:, :, L:], k=torch.cat([prs[i]["k"], nxt], dim=2), v=torch.cat([prs[i]["v"], nxv], dim=2),
                   s_aux=sa)
        rows = torch.arange(n)
        assert factors(inp, true, true, rows, tol_o=tol)[0] == 0.0
        o_true = masked_attention(inp["q"], inp["k"], inp["v"], None, true, sa)[0]
        assert (o_true - ref[i]).abs().max().item() < 1e-9        # the masked form IS the oracle of the GPU test
        for what, mut in muts.items():
            hit = torch.nonzero((true != mut).any(1)).flatten()
            fo = factors(inp, true, mut, hit, tol_o=tol)[0]
            print(f"{dt} D={D} G={G} Wc={W} sequence {i} (history {L}, n {n}), {what}: {fo:.1f} tolerances")
            best[what] = max(best.get(what, 0.0), fo)
    # "some row": the pack as a whole catches each edge (with G = 1 a short sequence has too few rows to draw every kind)
    assert set(best) == {"diagonal lost", "later chunk token", "oldest window key lost", "key behind the window",
                         "first row of the next sequence"}
    for what, fo in best.items():
        assert fo >= 10, (what, fo)
