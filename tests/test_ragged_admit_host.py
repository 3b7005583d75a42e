"""Host-side checks of admission in the packed ragged step (SFA_FLAG_RAGGED_ADMIT, ragged_step_dyn(admit=True)): the
flag and the keyword, argument checks and workspace that the flag leaves alone, the index-set model of an admitting
sequence's mask and of its placement, and the CPU proof (oracle against mutated oracle, as tests/test_probe_inputs.py)
that the probe inputs of tests/test_gpu_ragged_admit.py::test_mask_edge_probes cannot pass with a wrong sink edge."""
import functools
import inspect
import os
import re

import pytest
import torch

import probe_inputs as P
from oracle import sink_oracle as O
from sink_attention import SinkAttentionCache, SinkCacheLayer
from test_decode_multi_host import history_keys
from test_probe_inputs import factors, masked_attention
from test_ragged_step_host import _abi_args, _call
from util import DECODE_TOL as TOL
from util import rand

HKV = 2
ADMIT_LENGTHS = [0, 1, 3, 4, 5, 33, 70, 100]
SINKS = [4, 40]
WINDOWS = [16, 48]
KTILE = 32                             # keys per tile of the split kernels
# the admitting probe sequences of a pack: both longer than num_sink + Wc at (4, 16), (4, 48) and (40, 16); at (40, 48)
# the longer one is (100 > 88) and the shorter one has its sink edge inside the second key tile without a row beyond it
PROBE_LENGTHS = [100, 70]
PROBE_TYPES = [("bf16", 64, 8), ("fp16", 128, 1), ("bf16", 96, 8), ("fp32", 48, 1), ("fp32", 64, 8)]


def admit_keys(n, num_sink, Wc, t):
    """The chunk tokens query t of an admitting sequence of n tokens sees (include/sfa.h, SFA_FLAG_RAGGED_ADMIT)."""
    nsk = min(n, num_sink)
    return [u for u in range(t + 1) if u < nsk or t - u <= Wc - 1]


def admit_placement(n, num_sink, Wc):
    """(sink row -> token, ring slot -> token, state row) that a committing admission of n tokens leaves"""
    nsk = min(n, num_sink)
    rem = n - nsk
    sink = {j: j for j in range(nsk)}
    ring = {s: nsk + s for s in range(rem)} if rem <= Wc else {s: n - Wc + s for s in range(Wc)}
    return sink, ring, [nsk, min(rem, Wc), rem if rem < Wc else 0, n]


@functools.lru_cache(maxsize=None)
def admit_probe(dt, D, G, W, ns):
    """probe inputs of the admitting sequences of PROBE_LENGTHS, each a self-attention of its own tokens (kinds diag /
    future / win_oldest / win_behind / sink_last / sink_next of probe_inputs at amplitude 2), and one s_aux for the call"""
    prs = [P.dense_probe(1, HKV * G, HKV, n, n, D, ns, W, P._DT[dt], 900 + i, aux=True, pairs=False, a=2.0)
           for i, n in enumerate(PROBE_LENGTHS)]
    for pr in prs:
        pr["s_aux"] = prs[0]["s_aux"]
    return prs


# ------------------------------------------------------------------------------------------------ flag and keyword
def test_header_and_bindings_define_the_flag():
    from sink_attention import _native
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "sfa.h")).read()
    assert re.search(r"^#define\s+SFA_FLAG_RAGGED_ADMIT\s+0x40u\s*$", header, re.M)
    assert re.search(r"^#define\s+SFA_ABI_VERSION\s+2\s*$", header, re.M)
    assert _native.FLAG_RAGGED_ADMIT == 0x40
    assert _native.lib().sfa_abi_version() == 2


@pytest.mark.parametrize("cls", [SinkCacheLayer, SinkAttentionCache])
def test_ragged_step_dyn_has_the_admit_keyword(cls):
    p = inspect.signature(cls.ragged_step_dyn).parameters
    assert "admit" in p and p["admit"].default is False
    assert p["commit"].default is True


def test_argument_checks_and_workspace_are_those_of_a_call_without_the_flag():
    """the cases of tests/test_ragged_step_host.py::test_c_abi_rejects_bad_arguments_before_any_launch, each with the flag
    off and on: same status, same message"""
    import ctypes
    N, t, d = _abi_args()
    lib = N.lib()

    def both(want, word=None, **kw):
        got = []
        for flags in (0, N.FLAG_RAGGED_ADMIT):
            dd = dict(d, **{k: v for k, v in kw.items() if k in d})
            rest = {k: v for k, v in kw.items() if k not in d}
            p = lambda x: ctypes.c_void_p(0x1000) if x else None
            a = dict(n_seq=3, state=1, slots=1, cu=1, ws=None, ws_bytes=0, scale=0.125)
            a.update(rest)
            rc = lib.sfa_decode_ring_ragged_slots(dd["q"], dd["sk"], dd["sv"], dd["wk"], dd["wv"], dd["kn"], dd["vn"],
                                                  dd["o"], None, 0, p(a["state"]), p(a["slots"]), p(a["cu"]), a["n_seq"],
                                                  a["ws"], a["ws_bytes"], a["scale"], flags, None)
            got.append((rc, lib.sfa_last_error()))
        assert got[0] == got[1] and got[0][0] == want, got
        assert word is None or word in got[0][1], got
    assert _call(N, d, state=0) == -1                     # the helper of the existing file still sees the same library
    both(-1, b"state", state=0)
    both(-1, b"slots", slots=0)
    both(-1, b"cu_q", cu=0)
    both(-1, b"n_seq", n_seq=0)
    _, _, d3 = _abi_args(T=13)
    both(-1, b"k_new", kn=d3["kn"], vn=d3["vn"])
    _, _, d4 = _abi_args(S=4)
    both(-1, b"pool", wk=d4["wk"], wv=d4["wv"])
    both(-1, None, scale=float("nan"))
    need = lib.sfa_decode_ragged_workspace_bytes(3, 8, 2, 12, 20, 64, 2)
    both(-3, b"workspace")
    both(-3, None, ws=ctypes.c_void_p(0x10000), ws_bytes=need - 1)


def test_workspace_bytes_are_unchanged():
    """the formula of decode_ragged_workspace (csrc/sfa_decode_multi.hip), restated: an admitting sequence plans over its
    chunk tiles only, which the bound of every fill level covers"""
    from sink_attention import _native
    ws = _native.lib().sfa_decode_ragged_workspace_bytes
    al, cd = (lambda x: (x + 255) & ~255), (lambda a, b: -(-a // b))
    for n_seq, Hq, Hkv, T, nkv, D in [(7, 16, 2, 192, 64, 64), (7, 2, 2, 128, 20, 128), (3, 8, 2, 12, 20, 64),
                                      (64, 64, 8, 2048, 4100, 128), (1, 4, 4, 1, 5, 48)]:
        G = Hq // Hkv
        rows = Hkv * T * G
        nrb = cd(G * T, 32) + n_seq
        P_ = min(rows * max(cd(cd(nkv + T, 32) + 2, 4), 1), rows + 2048 * 32)
        want = 2 * al(P_ * 4) + al(P_ * D * 4) + al(nrb * 8) + al(T * 4)
        assert ws(n_seq, Hq, Hkv, T, nkv, D, 2) == want, (n_seq, Hq, Hkv, T, nkv, D)


# ------------------------------------------------------------------------------------------------ mask and placement
@pytest.mark.parametrize("W", WINDOWS)
@pytest.mark.parametrize("ns", SINKS)
def test_the_admitting_mask_is_the_prefill_mask_of_the_sequence(ns, W):
    for n in ADMIT_LENGTHS:
        nsk = min(n, ns)
        full = O.valid_mask(torch.arange(n), torch.arange(n), ns, W)
        for t in range(n):
            keys = admit_keys(n, ns, W, t)
            assert keys == torch.nonzero(full[t]).flatten().tolist(), (n, t)
            if t >= nsk:    # the same set seen as a chunk behind a prefill of the sink tokens alone
                assert keys == history_keys(nsk, ns, W, t - nsk), (n, t)


@pytest.mark.parametrize("W", WINDOWS)
@pytest.mark.parametrize("ns", SINKS)
def test_the_placement_model_is_that_of_a_prefill(ns, W):
    for n in ADMIT_LENGTHS[1:]:
        ids = torch.arange(n, dtype=torch.float32).view(1, 1, n, 1)
        layer = SinkCacheLayer(ns, W)
        layer.append(ids, ids)            # first tokens ever: SinkCacheLayer._prefill
        sink, ring, state = admit_placement(n, ns, W)
        assert state == [layer.sink_len, layer.window_len, layer.write_pos, layer.seen_tokens], (n, state)
        assert {j: int(layer.sink_k[0, 0, j, 0]) for j in range(layer.sink_len)} == sink, n
        assert {s: int(layer.window_k[0, 0, s, 0]) for s in range(layer.window_len)} == ring, n
    assert admit_placement(0, ns, W) == ({}, {}, [0, 0, 0, 0])


# ------------------------------------------------------------------------------------------------ the CPU proof
def _mutants(n, ns, W):
    """the true mask [n, n] of an admitting sequence and the masks of a kernel that gets its sink edge wrong"""
    t, u = torch.arange(n).view(-1, 1), torch.arange(n).view(1, -1)
    nsk = min(n, ns)
    causal, win = u <= t, t - u <= W - 1
    true = causal & ((u < nsk) | win)
    assert torch.equal(true, O.valid_mask(torch.arange(n), torch.arange(n), ns, W))
    tile_start, tile_last = (u // KTILE) * KTILE, (u // KTILE) * KTILE + KTILE - 1
    dead = (tile_start < nsk) & (tile_last < t - W + 1)      # a tile that holds sinks, classed by the window alone
    return true, {
        "nsk - 1": causal & ((u < nsk - 1) | win),
        "nsk + 1": causal & ((u < nsk + 1) | win),
        "sinks clipped by the window": causal & win,
        "sink tile classed dead": true & ~dead,
    }


@pytest.mark.parametrize("W", WINDOWS)
@pytest.mark.parametrize("ns", SINKS)
@pytest.mark.parametrize("dt,D,G", PROBE_TYPES)
def test_a_wrong_sink_edge_moves_a_probe_row_tenfold(dt, D, G, ns, W):
    """Oracle against mutated oracle on the inputs of test_gpu_ragged_admit.py::test_mask_edge_probes: each mutant moves
    some row of the admitting probe sequences by at least ten times DECODE_TOL; the unmutated model is the oracle."""
    prs = admit_probe(dt, D, G, W, ns)
    tol = (TOL[P._DT[dt]], 0.0)
    best = {}
    for pr, n in zip(prs, PROBE_LENGTHS):
        true, muts = _mutants(n, ns, W)
        o_true = masked_attention(pr["q"], pr["k"], pr["v"], None, true, pr["s_aux"])[0]
        ref, _ = O.sink_attention_dense(pr["q"], pr["k"], pr["v"], ns, W, pr["s_aux"])
        assert (o_true - ref).abs().max().item() < 1e-9
        for what, mut in muts.items():
            hit = torch.nonzero((true != mut).any(1)).flatten()
            if hit.numel() == 0:
                continue
            fo = factors(dict(q=pr["q"], k=pr["k"], v=pr["v"], s_aux=pr["s_aux"]), true, mut, hit, tol_o=tol)[0]
            print(f"{dt} D={D} G={G} ns={ns} Wc={W} n={n}, {what}: {fo:.1f} tolerances over {hit.numel()} rows")
            best[what] = max(best.get(what, 0.0), fo)
    assert set(best) == {"nsk - 1", "nsk + 1", "sinks clipped by the window", "sink tile classed dead"}, best
    for what, fo in best.items():
        assert fo >= 10, (what, fo)


@pytest.mark.parametrize("W", WINDOWS)
@pytest.mark.parametrize("ns", SINKS)
def test_the_model_is_the_oracle_on_randn_inputs(ns, W):
    """masked attention under the index-set model against sink_attention_dense of the sequence alone, randn inputs of the
    GPU test's shapes: within half of DECODE_TOL (the two are the same mask, so the distance is rounding of f64)"""
    g = torch.Generator().manual_seed(5)
    for dtype, D, G in ((torch.bfloat16, 64, 8), (torch.float32, 48, 1)):
        sa = rand((HKV * G,), g, torch.float32, 0.8)
        for n in ADMIT_LENGTHS[1:]:
            q = rand((1, HKV * G, n, D), g, dtype)
            k, v = rand((1, HKV, n, D), g, dtype), rand((1, HKV, n, D), g, dtype)
            mask = torch.zeros(n, n, dtype=torch.bool)
            for t in range(n):
                mask[t, admit_keys(n, ns, W, t)] = True
            o = masked_attention(q, k, v, None, mask, sa)[0]
            ref, _ = O.sink_attention_dense(q, k, v, ns, W, sa)
            assert (o - ref).abs().max().item() <= 0.5 * TOL[dtype], (dtype, n)
