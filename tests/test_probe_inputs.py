"""CPU proof that the mask-edge probe inputs (tests/probe_inputs.py) discriminate and that randn inputs do not.

No kernel is involved: the fp64 oracle under the TRUE mask against the same fp64 attention under a MUTATED mask (one key
too many or too few at one edge), measured with the tolerances tests/test_gpu_mask_edges.py asserts with
(bf16: O 2e-2 + 2e-2 |ref|, dQ 5e-2 + 5e-2 |ref|; cache calls: TOL of tests/test_gpu_decode_multi.py).

  (2a) randn inputs at N = 8192, W = 4096, D = 128: every mutant restricted to the last row of each 256-row block (on the
       rows with a full window, p >= W), or to one 32-key column range (num_sink +- 1 excepted, see RANDN_BLIND), stays
       WITHIN the tolerance: the existing randn parity tests cannot see it.
  (2b) probe inputs: every mutant exceeds the O tolerance AND the dQ tolerance at least tenfold on some element
       (forward-only cache / tree calls: the O tolerance).  Smallest factors measured at a = 2 (printed by the tests, -s):
       on the inputs the GPU file runs: c3slice (D = 128, W = 4096) O 60, dQ 12.9;  d64 (W = 700) O 48, dQ 12.7;  nq_lt_nk
       (D = 128, W = 600, six block-edge probes in all) O 41, dQ 12.3;  pack: O 126, dQ 52;  ring chunk (bf16 TOL 1.6e-2): 237;
       tree sibling: 205.  At a = 1 the D = 64 case drops to 9.0.  (A dropped "must be seen" key can exceed the dQ tolerance
       5e-2 + 5e-2 |ref| at most 20 x, since the difference IS |ref|; the pair rows' partner is chosen for a large |dP| gap
       to get past 10, from a wider list on block-edge rows.)
  (2c) every case of the GPU file has at least MIN_ROWS rows per q head of every kind it can have, the "must" of every
       drawn kind agrees with valid_mask, and every block edge is probed by every kind in turn (the sink_cap cases hold
       SINK_CAP sink_last rows per (batch, KV head) by construction).
  (2d) ONE backward kernel mutated, the forward and the other one right (masked_attention_per_kernel; LSE and Delta come
       from the true forward, as the kernels read them).  Against the tolerance dK / dV had alone, 5e-2 max(1, max |ref|) +
       5e-2 |ref|, a dK/dV kernel that drops the diagonal key or the oldest window key on the last row of every 256-row
       block, or inside one 32-key column range, PASSES (d64: 0.53 - 0.98 of the tolerance, one at 1.27; pinned below).
       Against the per-element sum bound of util.assert_within_sum_bound, 4 u A + u |ref|, every mutant of the dK/dV kernel
       alone exceeds the dV or the dK bound at least tenfold, on all rows, block-edge rows, one column range, the first /
       last key of the 32-key blocks only ("keyedge") and the first / last 64-row step of each 32-key block's sweep only
       ("sweepend"); every mutant of the dQ kernel alone exceeds the dQ tolerance tenfold.  Smallest factors measured
       (dQ-only / dK/dV-only): c3slice 18.4 / 31.1, d64 17.6 / 46.3, nq_lt_nk 16.1 / 30.2, rowsplit 19.4 / 35.3, strip80_aux
       22.2 / 32.5, skew96_w512 20.7 / 38.6, sinkcap_d128 16.4 / 25.6, sinkcap_rowsplit 20.5 / 25.7; pack mutants > 1e6.
       Blind by construction, and covered by the other group of cases (_blind): num_sink - 1 in dK/dV where hundreds of rows
       per KV head aim at key num_sink - 1 (dV 5.5 - 15.5 x on all rows, 0.2 - 0.7 x on block edges; the sink_cap cases, whose
       SINK_CAP kept rows are single block-edge rows, reach 25.6 x and each kept row alone 10.4 x or more), and num_sink - 1
       in dQ on the sink_cap cases (single rows: 4.5 x; the other cases: 16 x or more).
       Single pairs: dropping one probed "must be seen" pair from dK / dV exceeds the bound tenfold for all but 0 - 0.8 % of
       the pairs (strip80_aux, W = 128 at D = 80: 9.9 %).
       The 4 of the bound is derived (util.assert_within_sum_bound), not fitted: a CPU model of the documented arithmetic
       (util.rounded_model_bwd) stays within half of it on every bf16 / fp16 case of the GPU file.  Largest ratio of the
       model, dK / dV: c3slice 0.19 / 0.27, ragged_fp16 0.17 / 0.26, d64 0.21 / 0.29, d80 0.20 / 0.32, d96 0.22 / 0.47, sinks300
       0.18 / 0.32, n20000_w32 0.15 / 0.35, rowsplit 0.13 / 0.23, rowsplit_fallback 0.14 / 0.20, nq_lt_nk 0.15 / 0.26, strip80_aux
       0.09 / 0.20, strip64_bnhd 0.12 / 0.22, strip64_dq 0.16 / 0.23, strip80_dq_aux 0.38 / 0.23, skew96_w512 0.16 / 0.36, d32 0.20 /
       0.31, d256 0.23 / 0.31, d64_generic 0.20 / 0.32, w0 0.00 / 0.04, w1 0.10 / 0.37, w_ge_n 0.21 / 0.29, ns_ge_n 0.16 / 0.22, ns0
       0.12 / 0.35, sinkcap_d128 0.18 / 0.33, sinkcap_rowsplit 0.18 / 0.36; packs 0 - 8: at most 0.23 / 0.38.  (The kernels on
       an MI355X: at most 0.38 / 0.42, tests/test_gpu_mask_edges.py prints them.)  fp16 only: below 2^-14 a packed value keeps a
       fixed spacing instead of a relative precision, so A counts every visible pair at 2^-14 at least (oracle: tiny); without
       that the model itself is 400 x over the bound on keys nobody aims at, whose dV is about 3e-8.
"""
import functools
import math
import random

import pytest
import torch

import probe_inputs as P
from oracle import sink_oracle as O
from test_decode_multi_host import history_keys
from test_tree_host import depths, path_to, random_tree
from util import UNIT_ROUNDOFF, assert_within_sum_bound, probe_reference, rounded_model_bwd, sum_bound_ratio, sum_bound_tolerance

DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
TOL_O = (2e-2, 2e-2)          # bf16 forward, tests/test_gpu_prefill.py
TOL_G = (5e-2, 5e-2)          # dQ
TOL_CACHE = 1.6e-2            # tests/test_gpu_decode_multi.py::TOL[bf16]


# ------------------------------------------------------------------------------------------------ fp64 masked attention
def masked_attention(q, k, v, do, mask, s_aux=None, rows=None):
    """fp64 softmax attention under an arbitrary boolean mask [R, Nk] (or broadcastable to [B, Hq, R, Nk]) for the rows
    `rows` of q (default: all), forward and the explicit backward formulas of oracle/sink_oracle.py.  Returns o, lse, dq
    (those rows), dk, dv (the contribution of those rows, summed over the GQA group) and ds_aux (or None)."""
    B, Hq, _, D = q.shape
    Hkv, Nk = k.shape[1], k.shape[2]
    g = Hq // Hkv
    if rows is not None:
        q, do = q[:, :, rows], (do[:, :, rows] if do is not None else None)
    qf = q.double()
    kf, vf = (x.double().repeat_interleave(g, dim=1) for x in (k, v))
    scale = 1.0 / math.sqrt(D)
    s = (qf @ kf.transpose(-1, -2)) * scale
    s = s.masked_fill(~mask, float("-inf"))
    s_all = s if s_aux is None else torch.cat([s, s_aux.double().view(1, Hq, 1, 1).expand(B, Hq, s.shape[2], 1)], -1)
    lse = torch.logsumexp(s_all, -1)
    p = torch.nan_to_num(torch.exp(s - lse.unsqueeze(-1)), nan=0.0)
    o = p @ vf
    if do is None:
        return o, lse, None, None, None, None
    dof = do.double()
    delta = (dof * o).sum(-1)
    dv = p.transpose(-1, -2) @ dof
    ds = p * (dof @ vf.transpose(-1, -2) - delta.unsqueeze(-1))
    dq = (ds @ kf) * scale
    dk = (ds.transpose(-1, -2) @ qf) * scale
    dk, dv = (x.view(B, Hkv, g, Nk, D).sum(2) for x in (dk, dv))
    dsa = None if s_aux is None else -(torch.exp(s_aux.double().view(1, Hq, 1) - lse) * delta).sum((0, 2))
    return o, lse, dq, dk, dv, dsa


def edge_mask(p, j, ns, W, dW=0, dns=0, dc=0):
    """valid_mask with the window / the sink count / the causal edge moved by one key."""
    i, jj = p.view(-1, 1), j.view(1, -1)
    return (jj <= i + dc) & ((jj < ns + dns) | (jj >= i - (W + dW) + 1))


MUTANTS = {"W+1": dict(dW=1), "W-1": dict(dW=-1), "ns+1": dict(dns=1), "ns-1": dict(dns=-1),
           "causal+1": dict(dc=1), "causal-1": dict(dc=-1)}
RESTRICT = ("all", "blockedge", "cols")


def mutant_mask(name, restrict, Nq, Nk, ns, W):
    """(true mask, mutated mask) of a dense call; "blockedge": only the last row of every 256-row block is mutated;
    "cols": only one 32-key aligned column range (one that holds the moved edge for some rows)."""
    rows, j = torch.arange(Nq), torch.arange(Nk)
    p = rows + (Nk - Nq)
    true = edge_mask(p, j, ns, W)
    assert torch.equal(true, O.valid_mask(p, j, ns, W))
    mut = edge_mask(p, j, ns, W, **MUTANTS[name])
    if restrict == "blockedge":
        mut = torch.where((rows % 256 == 255).view(-1, 1), mut, true)
    elif restrict == "cols":
        # W: the rows that see / lose a key of [c0, c0 + 32) at their window edge; causal: rows with a full window
        c0 = {"ns+1": ns, "ns-1": ns - 1, "causal+1": (Nk + W) // 2, "causal-1": (Nk + W) // 2}.get(name, max(Nk - W, 64) // 2) // 32 * 32
        mut = torch.where(((j >= c0) & (j < c0 + 32)).view(1, -1), mut, true)
    return true, mut


def factors(inp, true, mut, rows, tol_o=TOL_O, tol_g=TOL_G):
    """max over elements of |mutated - true| / (atol + rtol |true|) for O and dQ on `rows`."""
    sa = inp.get("s_aux")
    a = masked_attention(inp["q"], inp["k"], inp["v"], inp.get("do"), true[rows], sa, rows)
    b = masked_attention(inp["q"], inp["k"], inp["v"], inp.get("do"), mut[rows], sa, rows)
    fo = ((a[0] - b[0]).abs() / (tol_o[0] + tol_o[1] * a[0].abs())).max().item()
    if a[2] is None:
        return fo, None, None
    fq = ((a[2] - b[2]).abs() / (tol_g[0] + tol_g[1] * a[2].abs())).max().item()
    # dK / dV: the exact change of the whole gradient (rows outside `rows` do not change); their tolerance is at least 5e-2
    fkv = max((a[3] - b[3]).abs().max().item(), (a[4] - b[4]).abs().max().item()) / 5e-2
    return fo, fq, fkv


def affected(true, mut, cap=768):
    r = torch.nonzero((true != mut).any(1)).flatten()
    if r.numel() > cap:        # a row slice is enough: the first, the middle and the last of the affected rows
        r = torch.cat([r[:cap // 3], r[r.numel() // 2 - cap // 6:r.numel() // 2 + cap // 6], r[-cap // 3:]])
    return r


# ------------------------------------------------------------------------------------------------ 1. the harness itself
@pytest.mark.parametrize("B,Hq,Hkv,Nq,Nk,D,ns,W,aux", [(2, 4, 2, 150, 150, 32, 3, 20, True), (1, 4, 1, 90, 140, 64, 5, 33, False),
                                                       (1, 2, 2, 70, 70, 32, 0, 0, True), (1, 2, 1, 64, 64, 32, 100, 7, False)])
def test_masked_attention_equals_the_oracle_under_the_true_mask(B, Hq, Hkv, Nq, Nk, D, ns, W, aux):
    pr = P.dense_probe(B, Hq, Hkv, Nq, Nk, D, ns, W, torch.bfloat16, 1, aux=aux)
    for inp in (pr, P.randn_like_probe(pr, 2)):
        true = O.valid_mask(torch.arange(Nq) + Nk - Nq, torch.arange(Nk), ns, W)
        got = masked_attention(inp["q"], inp["k"], inp["v"], inp["do"], true, inp["s_aux"])
        o, lse = O.sink_attention_dense(inp["q"], inp["k"], inp["v"], ns, W, inp["s_aux"])
        ref = (o, lse) + tuple(O.sink_attention_bwd_dense(inp["q"], inp["k"], inp["v"], inp["do"], ns, W, inp["s_aux"]))
        for x, y in zip(got, ref):
            assert (x is None) == (y is None)
            if x is not None:
                assert torch.allclose(x, y, rtol=1e-12, atol=1e-12, equal_nan=True)


def test_masked_attention_equals_decode_dense_per_row_for_the_cache_forms():
    ns, W, total, n = 3, 10, 40, 7
    pr = P.chunk_probe(1, 4, 2, 32, ns, W, total, n, torch.bfloat16, 3)
    pos, j = torch.arange(n) + total, torch.arange(total + n)
    o = masked_attention(pr["q"], pr["k"], pr["v"], None, O.valid_mask(pos, j, ns, W), pr["s_aux"], rows=pos)[0]
    for t in range(n):
        keep = torch.tensor(history_keys(total, ns, W, t))
        ref = O.decode_dense(pr["q"][:, :, total + t:total + t + 1], pr["k"][:, :, keep], pr["v"][:, :, keep], pr["s_aux"])
        assert torch.allclose(o[:, :, t:t + 1], ref, rtol=1e-12, atol=1e-12)
    parent = random_tree(random.Random(1), 12, True, "random")
    tp = P.tree_probe(1, 4, 2, 32, ns, W, total, parent, torch.bfloat16, 4)
    m = tree_mask(total, ns, W, parent)
    o = masked_attention(tp["q"], tp["k"], tp["v"], None, m, tp["s_aux"], rows=torch.arange(len(parent)) + total)[0]
    for u in range(len(parent)):
        keep = torch.nonzero(m[u]).flatten()
        ref = O.decode_dense(tp["q"][:, :, total + u:total + u + 1], tp["k"][:, :, keep], tp["v"][:, :, keep], tp["s_aux"])
        assert torch.allclose(o[:, :, u:u + 1], ref, rtol=1e-12, atol=1e-12)


def tree_mask(total, sl, W, parent):
    """[n, total + n]: the keys node u sees (the contract of include/sfa.h, as tests/test_gpu_tree_verify.py::_tree_keys)."""
    d = depths(parent)
    m = torch.zeros(len(parent), total + len(parent), dtype=torch.bool)
    for u in range(len(parent)):
        m[u, :sl] = True
        m[u, max(sl, total + d[u] - W + 1):total] = True
        for v in path_to(parent, u):
            if d[u] - d[v] <= W - 1:
                m[u, total + v] = True
    return m


# ------------------------------------------------------------------------------------------------ 2a. randn is blind
BIG = (1, 4, 1, 8192, 8192, 128, 4, 4096)


# ns+1 / ns-1 restricted to one column range are NOT in this list: the range that holds key num_sink (num_sink - 1) is read
# by EVERY row beyond the window, and over thousands of rows the largest single randn weight (about e^4 / (W e^0.5)) times
# |v| reaches the O tolerance (measured 1.3 x); they stay in (2b)
RANDN_BLIND = [(n, r) for n in MUTANTS for r in ("blockedge", "cols") if not (n.startswith("ns") and r == "cols")]


@pytest.mark.parametrize("name,restrict", RANDN_BLIND)
def test_randn_inputs_do_not_see_a_restricted_mutant(name, restrict):
    B, Hq, Hkv, Nq, Nk, D, ns, W = BIG
    inp = P.randn_like_probe(P.dense_probe(B, Hq, Hkv, Nq, Nk, D, ns, W, torch.bfloat16, 5), 6)
    true, mut = mutant_mask(name, restrict, Nq, Nk, ns, W)
    rows = affected(true, mut)
    if restrict == "blockedge":
        # the first rows see few keys, so one key more or less IS visible to randn there (row 255 under j < i loses one key of
        # 256); the statement is about the windows the kernels are built for: rows with a full window
        rows = rows[rows >= W]
    assert rows.numel() > 0
    fo, fq, fkv = factors(inp, true, mut, rows)
    print(f"randn {name}/{restrict}: {rows.numel()} rows, O {fo:.3f} dQ {fq:.3f} dK/dV {fkv:.3f} of the tolerance")
    assert fo < 1 and fq < 1 and fkv < 1, (fo, fq, fkv)


# ------------------------------------------------------------------------------------------------ 2b. the probes see it
def _smallest_factors(shape, a=None, seed=5, names=MUTANTS, restricts=RESTRICT, pr=None):
    B, Hq, Hkv, Nq, Nk, D, ns, W = shape
    pr = P.dense_probe(B, Hq, Hkv, Nq, Nk, D, ns, W, torch.bfloat16, seed, a=a) if pr is None else pr
    res = {}
    for name in names:
        for restrict in restricts:
            true, mut = mutant_mask(name, restrict, Nq, Nk, ns, W)
            fo, fq, _ = factors(pr, true, mut, affected(true, mut))
            res[name, restrict] = (fo, fq)
    return res


@pytest.mark.parametrize("case_id", ["c3slice", "d64", "nq_lt_nk"])
def test_probes_catch_every_mutant(case_id):
    """on the very inputs tests/test_gpu_mask_edges.py runs for these three cases (bf16)"""
    case = next(c for c in P.DENSE_CASES if c["id"] == case_id)
    shape = case["shape"]
    res = _smallest_factors(shape, pr=P.dense_case_probe(case))
    for key, (fo, fq) in res.items():
        print(f"probe {shape} {key}: O {fo:.1f} dQ {fq:.1f} tolerances")
    print("smallest:", min(x[0] for x in res.values()), min(x[1] for x in res.values()))
    bad = {k: x for k, x in res.items() if not (x[0] >= 10 and x[1] >= 10)}
    assert not bad, bad


def test_amplitude_is_the_smallest_power_of_two():
    """a = 1 misses the factor 10 at head dim 64 (the noise of W keys outweighs a logit of 8), a = 2 holds it."""
    shape = (1, 4, 2, 3000, 3000, 64, 70, 700)
    lo = _smallest_factors(shape, a=1.0)
    hi = _smallest_factors(shape, a=2.0)
    print("a = 1:", min(min(x) for x in lo.values()), " a = 2:", min(min(x) for x in hi.values()))
    assert min(min(x) for x in lo.values()) < 10 <= min(min(x) for x in hi.values())
    assert all(P.amplitude(D) == 2.0 for D in (32, 64, 80, 96, 128, 256))
    # the peak: share of the softmax mass on the target of a single "diag" row with a full window of 4096 keys
    for D, least in ((64, 0.99), (128, 0.99)):
        pr = P.dense_probe(1, 1, 1, 8, 4200, D, 4, 4096, torch.bfloat16, 9, pairs=False)
        rows = torch.nonzero((pr["kind"][0, 0] == 0)).flatten()
        pos = rows + 4200 - 8
        s = (pr["q"][0, 0, rows].double() @ pr["k"][0, 0].double().T) / math.sqrt(D)
        s = s.masked_fill(~O.valid_mask(pos, torch.arange(4200), 4, 4096), float("-inf"))
        share = torch.softmax(s, -1)[torch.arange(rows.numel()), pos]
        assert share.min().item() > least, (D, share)
        assert abs(s.max().item() - 2.0 * math.sqrt(D)) < 1e-9          # the largest scaled logit of a single row


def _pack_masks(cu, ns, W):
    T = cu[-1]
    seq = torch.zeros(T, dtype=torch.long)
    start = torch.zeros(T, dtype=torch.long)
    for s, (a, b) in enumerate(zip(cu[:-1], cu[1:])):
        seq[a:b], start[a:b] = s, a
    pos = torch.arange(T) - start
    same = seq.view(-1, 1) == seq.view(1, -1)
    pj, pi = pos.view(1, -1), pos.view(-1, 1)
    true = same & (pj <= pi) & ((pj < ns) | (pj >= pi - W + 1))
    j = torch.arange(T).view(1, -1)
    prev = true | ((j == start.view(-1, 1) - 1) & (start.view(-1, 1) > 0))
    sinks = true | ((j < ns) & (seq.view(-1, 1) > 0))
    return true, {"previous sequence's last key": prev, "the pack's first num_sink keys": sinks}


def test_probes_catch_the_pack_mutants_and_equal_the_per_sequence_oracle():
    Hq, Hkv, D, ns, W, cu = 4, 2, 64, 4, 100, [0, 300, 301, 700, 1000]
    pr = P.dense_probe(1, Hq, Hkv, cu[-1], cu[-1], D, ns, W, torch.bfloat16, 7, aux=True, cu=cu)
    true, muts = _pack_masks(cu, ns, W)
    got = masked_attention(pr["q"], pr["k"], pr["v"], pr["do"], true, pr["s_aux"])
    for a, b in zip(cu[:-1], cu[1:]):
        sl = (slice(None), slice(None), slice(a, b))
        o, _ = O.sink_attention_dense(pr["q"][sl], pr["k"][sl], pr["v"][sl], ns, W, pr["s_aux"])
        g = O.sink_attention_bwd_dense(pr["q"][sl], pr["k"][sl], pr["v"][sl], pr["do"][sl], ns, W, pr["s_aux"])
        assert torch.allclose(got[0][sl], o, atol=1e-12) and torch.allclose(got[2][sl], g[0], atol=1e-12)
        assert torch.allclose(got[3][sl], g[1], atol=1e-12) and torch.allclose(got[4][sl], g[2], atol=1e-12)
    for what, mut in muts.items():
        rows = affected(true, mut)
        fo, fq, _ = factors(pr, true, mut, rows)
        print(f"pack, {what}: O {fo:.1f} dQ {fq:.1f} tolerances")
        assert fo >= 10 and fq >= 10, (what, fo, fq)


def test_probes_catch_the_ring_and_tree_mutants():
    tol = (TOL_CACHE, 0.0)
    ns, W, extra, n = 4, 1024, 1004, 40
    total = ns + W + extra
    pr = P.chunk_probe(1, 16, 2, 64, ns, W, total, n, torch.bfloat16, 11)
    pos, j = torch.arange(n) + total, torch.arange(total + n)
    true = torch.zeros(total + n, total + n, dtype=torch.bool)
    true[pos] = O.valid_mask(pos, j, ns, W)
    evicted, later = true.clone(), true.clone()
    evicted[pos, pos - W] = True                                    # the slot the row's own token evicts is still read
    later[pos[:-1], pos[:-1] + 1] = True                            # chunk row t sees chunk token t + 1
    for what, mut in (("evicted slot", evicted), ("later chunk token", later)):
        fo, _, _ = factors(pr, true, mut, affected(true, mut), tol_o=tol)
        print(f"ring, {what}: O {fo:.1f} tolerances")
        assert fo >= 10, (what, fo)
    parent = random_tree(random.Random(2), 24, True, "random")
    total = 4 + 1024 + 13
    tp = P.tree_probe(1, 8, 2, 64, 4, 1024, total, parent, torch.bfloat16, 13)
    m = tree_mask(total, 4, 1024, parent)
    true = torch.zeros(total + len(parent), total + len(parent), dtype=torch.bool)
    true[total:] = m
    sib = true.clone()
    for u in range(len(parent)):
        for x in range(len(parent)):
            if x != u and parent[x] == parent[u]:
                sib[total + u, total + x] = True
    fo, _, _ = factors(tp, true, sib, affected(true, sib), tol_o=tol)
    print(f"tree, a node sees its sibling: O {fo:.1f} tolerances")
    assert fo >= 10, fo


# ------------------------------------------------------------------------------------------------ 2c. coverage
def _check_musts(pr, Nq, Nk, ns, W, cu=None):
    """the 'must' of every drawn kind agrees with the true mask, and pair partners are visible"""
    if cu is None:
        start, pos = torch.zeros(Nq, dtype=torch.long), torch.arange(Nq) + Nk - Nq
    else:
        start = torch.zeros(Nq, dtype=torch.long)
        for a, b in zip(cu[:-1], cu[1:]):
            start[a:b] = a
        pos = torch.arange(Nq) - start
    tgt, kind = pr["target"], pr["kind"]
    tp = tgt - start                                  # target position within the row's own sequence
    seen = (tp >= 0) & (tp <= pos) & ((tp < ns) | (tp >= pos - max(W, 0) + 1))
    must = torch.tensor([P.MUST_SEE[k] for k in P.KINDS])[kind]
    assert torch.equal(seen, must)
    assert bool(((tgt >= 0) & (tgt < Nk)).all())
    if "pair" in pr and bool(pr["pair"].any()):
        pp = pr["partner"] - start                   # partners: inside the window of every one-key mutant, never the target
        ok = (pp >= 0) & (pp <= pos - 2) & (pp >= pos - max(W, 0) + 3) & (pr["partner"] != tgt) & (pp >= pos - 1 - P.PAIR_OFFSETS_EDGE)
        assert bool(ok[pr["pair"]].all()) and bool((pr["partner"][~pr["pair"]] == -1).all())


@pytest.mark.parametrize("case", P.DENSE_CASES, ids=[c["id"] for c in P.DENSE_CASES])
def test_every_dense_case_covers_its_kinds(case):
    B, Hq, Hkv, Nq, Nk, D, ns, W = case["shape"]
    pr = P.dense_case_probe(case)                     # the inputs the GPU test runs
    _check_musts(pr, Nq, Nk, ns, W)
    counts = P.kind_counts(pr)
    missing = set(case.get("missing", ())) | {"prev_last", "pack_sink"}
    capped = pr["kind"] == P.KINDS.index("sink_last") if case.get("sink_cap") else torch.zeros_like(pr["pair"])
    if case.get("sink_cap"):
        # few sink_last rows BY CONSTRUCTION: sink_cap per (batch, KV head), all of them single rows (checked in part 2d)
        assert capped.view(B, Hkv, -1).sum(-1).tolist() == [[case["sink_cap"]] * Hkv] * B
        missing.add("sink_last")
    short = {k: c for k, c in counts.items() if k not in missing and c < P.MIN_ROWS}
    assert not short, (case["id"], short, counts)
    # GQA: the heads of one group probe one row with different kinds wherever the row has at least that many
    exist, _, _ = P.row_targets(Nq, Nk, ns, W)
    g = Hq // Hkv
    kd = pr["kind"].view(B, Hkv, g, Nq)
    distinct = torch.tensor([[len(set(kd[b, h, :, r].tolist())) for r in range(0, Nq, 37)] for b in range(B) for h in range(Hkv)])
    assert torch.equal(distinct, torch.minimum(exist.sum(0)[::37], torch.tensor(g)).expand_as(distinct))
    # block edges: the last row of every 256-row block is a probed (pair) row, and over the block edges every kind that exists
    # on one of them is drawn (as long as there are at least as many (block, head) slots as kinds)
    edges = torch.arange(255, Nq, 256)
    if edges.numel():
        if W >= P.PAIR_MIN_WINDOW:
            assert bool((pr["pair"] | capped)[:, :, edges].all())
        have = set(pr["kind"][:, :, edges].flatten().tolist())
        can = set(torch.nonzero(exist[:, edges].all(1)).flatten().tolist())
        if edges.numel() * Hq >= 6:
            assert can <= have, (case["id"], can, have)


@pytest.mark.parametrize("i", range(len(P.VARLEN_CASES)))
def test_every_pack_covers_its_kinds(i):
    c = P.VARLEN_CASES[i]
    T = c["cu"][-1]
    pr = P.pack_case_probe(i)                         # the inputs the GPU test runs
    _check_musts(pr, T, T, c["ns"], c["W"], c["cu"])
    counts = P.kind_counts(pr)
    short = {k: n for k, n in counts.items() if k not in set(c.get("missing", ())) and n < P.MIN_ROWS}
    assert not short, (i, short, counts)


def _chunk_counts(pr):
    return {name: int((pr["kind"] == i).sum()) for i, name in enumerate(P.KINDS[:6])}


def test_cache_cases_cover_their_kinds():
    """a chunk has n rows only, so the count is over (row, head): every kind has at least MIN_ROWS probes over the case,
    except the kinds the case names as missing; every 'must' agrees with the mask.  The inputs are those of the GPU test."""
    for row in P.CHUNK_CASES:
        dt, B, Hq, Hkv, D, ns, W, extra, n = row
        total = ns + W + extra
        pr = P.chunk_case_probe(row)
        _check_musts(pr, n, total + n, ns, W)
        missing = set(P._NO_SINK) if ns == 0 else set()
        if n == 1:
            missing.add("future")                      # a chunk of one token has no later token
        short = {k: c for k, c in _chunk_counts(pr).items() if k not in missing and c < P.MIN_ROWS}
        assert not short, (row, short)
    c = P.RAGGED_CASE
    for pr, L, missing in zip(P.ragged_case_probes(), c["lengths"], c["missing"]):
        _check_musts(pr, c["n"], L + c["n"], c["ns"], c["W"])
        short = {k: x for k, x in _chunk_counts(pr).items() if k not in missing and x < P.MIN_ROWS}
        assert not short, (L, short)


def test_tree_cases_cover_their_kinds():
    """every row of the GPU test's tree table, with its trees, seeds, head counts and head dims: the 'must' of every drawn
    kind agrees with the tree mask and every kind has at least MIN_ROWS (node, head) probes, except those TREE_MISSING names"""
    from test_gpu_tree_verify import TREES
    for i, row in enumerate(TREES + P.TREE_CASES_EXTRA):
        ns, W, prefill, appends, n, shape, forest = row
        parent = random_tree(random.Random(P.TREE_RNG_SEED + i), n, forest, shape)
        total = prefill + appends
        m = tree_mask(total, min(ns, total), W, parent)
        for dt, D in P.TREE_DTYPE_D:
            tp = P.tree_case_probe(i, row, parent, dt, D)
            seen = m[torch.arange(n).view(1, 1, n), tp["target"]]
            must = torch.tensor([P.TREE_MUST_SEE[k] for k in P.TREE_KINDS])[tp["kind"]]
            assert torch.equal(seen, must)
            counts = {name: int((tp["kind"] == j).sum()) for j, name in enumerate(P.TREE_KINDS)}
            short = {k: c for k, c in counts.items() if k not in P.TREE_MISSING.get(i, ()) and c < P.MIN_ROWS}
            assert not short, (i, row, D, short)


# ------------------------------------------------------------------------------------------------ 2d. one kernel at a time
# The product has three kernels with their own mask code (forward, dQ, dK/dV); a mutant of ONE of them leaves the other
# two right.  The backward kernels read LSE and Delta from the forward / preprocess pass and apply their own mask to
# P = exp(S - LSE).
def masked_attention_per_kernel(q, k, v, do, m_fwd, m_dq, m_dkdv, s_aux=None, rows=None):
    """masked_attention with one mask per kernel: m_fwd decides O, LSE and Delta, m_dq the P of dQ, m_dkdv the P of dK / dV.
    Returns o, lse, dq, dk, dv, ds_aux like masked_attention (equal to it to 1e-12 when the three masks are equal) and the
    bound terms A_K, A_V of util.assert_within_sum_bound (fp64, summed over the GQA group like dK / dV, under m_dkdv)."""
    B, Hq, _, D = q.shape
    Hkv, Nk = k.shape[1], k.shape[2]
    g = Hq // Hkv
    if rows is not None:
        q, do = q[:, :, rows], do[:, :, rows]
    qf, dof = q.double(), do.double()
    kf, vf = (x.double().repeat_interleave(g, dim=1) for x in (k, v))
    scale = 1.0 / math.sqrt(D)
    s = (qf @ kf.transpose(-1, -2)) * scale
    sm = s.masked_fill(~m_fwd, float("-inf"))
    s_all = sm if s_aux is None else torch.cat([sm, s_aux.double().view(1, Hq, 1, 1).expand(B, Hq, s.shape[2], 1)], -1)
    lse = torch.logsumexp(s_all, -1)
    e = torch.exp(s - lse.unsqueeze(-1))          # (a key the forward did not see can weigh more than 1)
    e = torch.where(torch.isinf(lse).unsqueeze(-1), torch.zeros_like(e), e)
    o = e.masked_fill(~m_fwd, 0.0) @ vf
    delta = (dof * o).sum(-1)
    dp = dof @ vf.transpose(-1, -2)
    pq, pkv = e.masked_fill(~m_dq, 0.0), e.masked_fill(~m_dkdv, 0.0)
    dq = ((pq * (dp - delta.unsqueeze(-1))) @ kf) * scale
    dk = ((pkv * (dp - delta.unsqueeze(-1))).transpose(-1, -2) @ qf) * scale
    dv = pkv.transpose(-1, -2) @ dof
    a_k = ((pkv * (dp.abs() + (dof * o).abs().sum(-1, keepdim=True))).transpose(-1, -2) @ qf.abs()) * scale
    a_v = pkv.transpose(-1, -2) @ dof.abs()
    dk, dv, a_k, a_v = (x.view(B, Hkv, g, Nk, D).sum(2) for x in (dk, dv, a_k, a_v))
    dsa = None if s_aux is None else -(torch.exp(s_aux.double().view(1, Hq, 1) - lse) * delta).sum((0, 2))
    return o, lse, dq, dk, dv, dsa, a_k, a_v


RESTRICT_DKDV = RESTRICT + ("keyedge", "sweepend")


def restricted(true, mut, restrict, name, Nq, Nk, ns, W):
    """mutant_mask's restrictions and two more for the dK/dV walk (32-key blocks, swept in 64-row steps): "keyedge": only
    the first and the last key of a 32-key block are mutated; "sweepend": only the first and the last 64-row step in which a
    32-key block is visible (under either mask)."""
    if restrict in RESTRICT:
        return mutant_mask(name, restrict, Nq, Nk, ns, W)[1]
    j = torch.arange(Nk)
    if restrict == "keyedge":
        return torch.where(((j % 32 == 0) | (j % 32 == 31)).view(1, -1), mut, true)
    nr, nc = -(-Nq // 64), -(-Nk // 32)
    vis = torch.zeros(nr * 64, nc * 32, dtype=torch.bool)
    vis[:Nq, :Nk] = true | mut
    vis = vis.view(nr, 64, nc, 32).any(3).any(1)                                   # [64-row step, 32-key block]
    step = torch.arange(nr).view(-1, 1)
    first = torch.where(vis, step, torch.full_like(step, nr)).min(0).values
    last = torch.where(vis, step, torch.full_like(step, -1)).max(0).values
    ends = (step == first.view(1, -1)) | (step == last.view(1, -1))                # [nr, nc]
    ends = ends.repeat_interleave(64, 0)[:Nq].repeat_interleave(32, 1)[:, :Nk]
    return torch.where(ends, mut, true)


def pair_terms(inp, ref, r, t):
    """For the (row r[n], key t[n]) pairs, per (batch, q head): P = exp(s - LSE), dS = P (dP - Delta) with LSE / O of the
    case's reference (forward under the true mask), and the gathered q, k, dO rows.  r, t: [n] or [B, Hq, n]."""
    q, k, v, do = (inp[x].double() for x in ("q", "k", "v", "do"))
    B, Hq, _, D = q.shape
    g = Hq // k.shape[1]
    if r.dim() == 1:
        r, t = r.view(1, 1, -1).expand(B, Hq, -1), t.view(1, 1, -1).expand(B, Hq, -1)
    take = lambda x, idx: torch.gather(x, 2, idx.unsqueeze(-1).expand(B, Hq, idx.shape[-1], D))
    qr, dor, orow = take(q, r), take(do, r), take(ref["o"], r)
    kt, vt = take(k.repeat_interleave(g, dim=1), t), take(v.repeat_interleave(g, dim=1), t)
    p = torch.exp((qr * kt).sum(-1) / math.sqrt(D) - torch.gather(ref["lse"], 2, r))
    ds = p * ((dor * vt).sum(-1) - (dor * orow).sum(-1))
    return p, ds, qr, kt, dor


def sparse_diffs(inp, ref, true, mut):
    """mutated minus true dQ [B,Hq,Nq,D] and dK, dV [B,Hkv,Nk,D] when ONE backward kernel runs under `mut`: only the pairs on
    which the masks differ contribute, with P taken from the true forward's LSE (equal to masked_attention_per_kernel
    minus the reference, checked below)."""
    r, t = torch.nonzero(true != mut, as_tuple=True)
    sign = torch.where(mut[r, t], 1.0, -1.0).double().view(1, 1, -1, 1)
    p, ds, qr, kt, dor = pair_terms(inp, ref, r, t)
    B, Hq, Nq, D = inp["q"].shape
    Hkv, Nk = inp["k"].shape[1], inp["k"].shape[2]
    scale = 1.0 / math.sqrt(D)
    ddq = torch.zeros(B, Hq, Nq, D, dtype=torch.float64).index_add_(2, r, sign * scale * ds.unsqueeze(-1) * kt)
    ddk = torch.zeros(B, Hq, Nk, D, dtype=torch.float64).index_add_(2, t, sign * scale * ds.unsqueeze(-1) * qr)
    ddv = torch.zeros(B, Hq, Nk, D, dtype=torch.float64).index_add_(2, t, sign * p.unsqueeze(-1) * dor)
    return ddq, ddk.view(B, Hkv, Hq // Hkv, Nk, D).sum(2), ddv.view(B, Hkv, Hq // Hkv, Nk, D).sum(2)


def sum_bound(ref, which, u):
    """the tolerance of util.assert_within_sum_bound, per element"""
    return sum_bound_tolerance(ref["d" + which], ref["a_" + which], u, {v: k for k, v in UNIT_ROUNDOFF.items()}[u])


def old_tolerance(ref, which):
    """the dK / dV tolerance tests/test_gpu_mask_edges.py had alone before the sum bound (and keeps beside it)"""
    x = ref["d" + which].abs()
    return 5e-2 * max(1.0, x.max().item()) + 5e-2 * x


def per_kernel_factors(inp, ref, true, mut, u, tol=None):
    """(dQ-only mutant: largest |change of dQ| / dQ tolerance;  dK/dV-only mutant: the same for dK and for dV against the sum
    bound, or against tol(ref, "k" / "v"))"""
    ddq, ddk, ddv = sparse_diffs(inp, ref, true, mut)
    tk, tv = ((sum_bound(ref, w, u) if tol is None else tol(ref, w)) for w in "kv")
    fq = (ddq.abs() / (TOL_G[0] + TOL_G[1] * ref["dq"].abs())).max().item()
    return fq, (ddk.abs() / tk).max().item(), (ddv.abs() / tv).max().item()


@functools.lru_cache(maxsize=None)
def _case(case_id):
    """probe inputs and reference of one dense case of the GPU file (what tests/test_gpu_mask_edges.py::_dense caches)"""
    case = next(c for c in P.DENSE_CASES if c["id"] == case_id)
    ns, W = case["shape"][6:]
    pr = P.dense_case_probe(case)
    o, lse, (dq, dk, dv, _, a_k, a_v) = probe_reference(pr, ns, W)
    return case, pr, dict(o=o, lse=lse, dq=dq, dk=dk, dv=dv, a_k=a_k, a_v=a_v)


def test_per_kernel_attention_equals_masked_attention_and_the_sparse_form():
    B, Hq, Hkv, Nq, Nk, D, ns, W = 2, 4, 2, 150, 190, 32, 3, 20
    pr = P.dense_probe(B, Hq, Hkv, Nq, Nk, D, ns, W, torch.bfloat16, 1, aux=True)
    p, j = torch.arange(Nq) + Nk - Nq, torch.arange(Nk)
    true = edge_mask(p, j, ns, W)
    for m in (true, edge_mask(p, j, ns, W, dW=1), edge_mask(p, j, ns, W, dc=-1)):        # three equal masks: today's function
        a = masked_attention(pr["q"], pr["k"], pr["v"], pr["do"], m, pr["s_aux"])
        b = masked_attention_per_kernel(pr["q"], pr["k"], pr["v"], pr["do"], m, m, m, pr["s_aux"])
        for x, y in zip(a, b[:6]):
            assert torch.allclose(x, y, rtol=1e-12, atol=1e-12)
    # ... and the bound terms are those of the oracles, dense and banded
    full = masked_attention_per_kernel(pr["q"], pr["k"], pr["v"], pr["do"], true, true, true, pr["s_aux"])
    dense = O.sink_attention_bwd_dense(pr["q"], pr["k"], pr["v"], pr["do"], ns, W, pr["s_aux"], bounds=True)
    assert torch.allclose(full[6], dense[4], rtol=1e-12, atol=1e-12) and torch.allclose(full[7], dense[5], rtol=1e-12, atol=1e-12)
    assert bool((dense[1].abs() <= dense[4] * (1 + 1e-12)).all()) and bool((dense[2].abs() <= dense[5] * (1 + 1e-12)).all())
    sq = P.dense_probe(1, 4, 2, 700, 700, 32, 3, 40, torch.bfloat16, 2, aux=True)
    d2 = O.sink_attention_bwd_dense(sq["q"], sq["k"], sq["v"], sq["do"], 3, 40, sq["s_aux"], bounds=True)
    b2 = O.sink_attention_bwd_banded(sq["q"], sq["k"], sq["v"], sq["do"], 3, 40, sq["s_aux"], bounds=True)
    for x, y in zip(d2, b2):
        assert torch.allclose(x, y, rtol=1e-11, atol=1e-11)
    assert len(O.sink_attention_bwd_banded(sq["q"], sq["k"], sq["v"], sq["do"], 3, 40, sq["s_aux"])) == 4
    # one kernel mutated: the other kernels' outputs do not move, and sparse_diffs is the exact change
    ref = dict(o=full[0], lse=full[1], dq=full[2], dk=full[3], dv=full[4])
    for name in MUTANTS:
        mut = edge_mask(p, j, ns, W, **MUTANTS[name])
        ddq, ddk, ddv = sparse_diffs(pr, ref, true, mut)
        kv = masked_attention_per_kernel(pr["q"], pr["k"], pr["v"], pr["do"], true, true, mut, pr["s_aux"])
        dq = masked_attention_per_kernel(pr["q"], pr["k"], pr["v"], pr["do"], true, mut, true, pr["s_aux"])
        for i in (0, 1, 2, 5):
            assert torch.equal(kv[i], full[i])
        for i in (0, 1, 3, 4, 5):
            assert torch.equal(dq[i], full[i])
        assert torch.allclose(kv[3] - full[3], ddk, atol=1e-10) and torch.allclose(kv[4] - full[4], ddv, atol=1e-10)
        assert torch.allclose(dq[2] - full[2], ddq, atol=1e-10)
        assert ddv.abs().max() > 0 and ddq.abs().max() > 0


def single_pair_factors(pr, ref, u):
    """[B, Hq, Nq]: the factor by which dropping the ONE pair (row, its target) from dK / dV exceeds the sum bound at the
    target key - max over d of P_it |dO_id| against the dV bound, of scale |dS_it| |q_id| against the dK bound; the larger."""
    B, Hq, Nq, D = pr["q"].shape
    Hkv = pr["k"].shape[1]
    r = torch.arange(Nq).view(1, 1, Nq).expand(B, Hq, Nq)
    p, ds, qr, _, dor = pair_terms(pr, ref, r, pr["target"])
    at = lambda x: torch.gather(x.repeat_interleave(Hq // Hkv, dim=1), 2, pr["target"].unsqueeze(-1).expand(B, Hq, Nq, D))
    fv = (p.unsqueeze(-1) * dor.abs() / at(sum_bound(ref, "v", u))).max(-1).values
    fk = (ds.abs().unsqueeze(-1) * qr.abs() / math.sqrt(D) / at(sum_bound(ref, "k", u))).max(-1).values
    return torch.maximum(fv, fk)


# the dense cases the per-kernel proofs run on, with the very inputs of the GPU file: hand-placed lists + sink tail at three
# shapes, N_q < N_kv, the row split, a strip and a skew case, and the two sink-edge cases
PROOF_CASES = ("c3slice", "d64", "nq_lt_nk", "rowsplit", "strip80_aux", "skew96_w512", "sinkcap_d128", "sinkcap_rowsplit")
FACTOR = 10.0


def _blind(case, name, kernel):
    """The (mutant, kernel) combinations a case cannot see BY CONSTRUCTION (another case does):
    ns - 1 in dK/dV without sink_cap: hundreds of rows per KV head aim at key num_sink - 1, and one contribution missing
      among n equal ones is below a relative precision of 4 u (measured: dV 5.5 - 15.5 x on all rows, 0.2 - 0.7 x on block
      edges); the sink_cap cases exist for this edge.
    ns - 1 in dQ with sink_cap: the kept sink_last rows are single rows, whose dS is near 0 (measured 4.5 x); every other case
      has pair rows there."""
    return name == "ns-1" and (kernel == "dkdv") != bool(case.get("sink_cap"))


def _mutants_of(case):
    ns = case["shape"][6]
    return [n for n in MUTANTS if ns > 0 or not n.startswith("ns")]       # (num_sink = 0: no sink edge, no kind aims at one)


@pytest.mark.parametrize("case_id", PROOF_CASES)
def test_probes_catch_a_mutant_of_one_backward_kernel(case_id):
    """A mask mutant of the dK/dV kernel ALONE exceeds the sum bound of dV or of dK tenfold, under every restriction
    (mutants that change no pair - a key edge that is not on the mutated edge - are skipped); one of the dQ kernel alone
    exceeds the dQ tolerance tenfold."""
    case, pr, ref = _case(case_id)
    B, Hq, Hkv, Nq, Nk, D, ns, W = case["shape"]
    u = UNIT_ROUNDOFF[pr["q"].dtype]
    bad, low = {}, {"dq": 1e30, "dk/dv": 1e30}
    for name in _mutants_of(case):
        true, full = mutant_mask(name, "all", Nq, Nk, ns, W)
        for restrict in RESTRICT_DKDV:
            mut = restricted(true, full, restrict, name, Nq, Nk, ns, W)
            if not bool((true != mut).any()):
                continue
            fq, fk, fv = per_kernel_factors(pr, ref, true, mut, u)
            print(f"{case_id} {name}/{restrict}: dQ-only {fq:.1f} x dQ tolerance; dK/dV-only {fk:.1f} x dK bound, {fv:.1f} x dV bound"
                  + (" (blind by construction: dK/dV)" if _blind(case, name, "dkdv") else "")
                  + (" (blind by construction: dQ)" if _blind(case, name, "dq") else ""))
            if not _blind(case, name, "dkdv"):
                low["dk/dv"] = min(low["dk/dv"], max(fk, fv))
                if max(fk, fv) < FACTOR:
                    bad[name, restrict, "dkdv"] = (fk, fv)
            if restrict in RESTRICT and not _blind(case, name, "dq"):
                low["dq"] = min(low["dq"], fq)
                if fq < FACTOR:
                    bad[name, restrict, "dq"] = fq
    print(f"{case_id} smallest: {low}")
    assert not bad, bad


def test_probes_catch_the_pack_mutants_of_one_backward_kernel():
    Hq, Hkv, D, ns, W, cu = 4, 2, 64, 4, 100, [0, 300, 301, 700, 1000]        # the pack of the test above
    pr = P.dense_probe(1, Hq, Hkv, cu[-1], cu[-1], D, ns, W, torch.bfloat16, 7, aux=True, cu=cu)
    true, muts = _pack_masks(cu, ns, W)
    f = masked_attention_per_kernel(pr["q"], pr["k"], pr["v"], pr["do"], true, true, true, pr["s_aux"])
    ref = dict(o=f[0], lse=f[1], dq=f[2], dk=f[3], dv=f[4], a_k=f[6], a_v=f[7])
    for what, mut in muts.items():
        fq, fk, fv = per_kernel_factors(pr, ref, true, mut, UNIT_ROUNDOFF[torch.bfloat16])
        print(f"pack, {what}: dQ-only {fq:.1f} x; dK/dV-only {fk:.1f} x dK bound, {fv:.1f} x dV bound")
        assert fq >= FACTOR and max(fk, fv) >= FACTOR, (what, fq, fk, fv)


def test_the_old_dkdv_tolerance_is_blind_to_restricted_dkdv_mutants():
    """Why the sum bound exists: against 5e-2 max(1, max |ref|) + 5e-2 |ref| (max |dV| = 57.5 on this case) a dK/dV kernel that
    drops the diagonal key or the oldest window key on the last row of every 256-row block, or inside one 32-key column range,
    stays within the tolerance (one exception, measured 1.27: dV of causal-1 in a column range; still far from a reliable
    factor), and the same mutants exceed the sum bound more than twenty times."""
    case, pr, ref = _case("d64")
    B, Hq, Hkv, Nq, Nk, D, ns, W = case["shape"]
    for name in ("causal-1", "W-1"):
        true, full = mutant_mask(name, "all", Nq, Nk, ns, W)
        for restrict in ("blockedge", "cols"):
            mut = restricted(true, full, restrict, name, Nq, Nk, ns, W)
            _, ok, ov = per_kernel_factors(pr, ref, true, mut, None, tol=old_tolerance)
            _, fk, fv = per_kernel_factors(pr, ref, true, mut, UNIT_ROUNDOFF[torch.bfloat16])
            print(f"d64 {name}/{restrict}: old tolerance dK {ok:.2f} dV {ov:.2f}; sum bound dK {fk:.1f} dV {fv:.1f}")
            assert ok < 1 and (ov < 1 or (name, restrict) == ("causal-1", "cols") and ov < 1.5), (name, restrict, ok, ov)
            assert max(fk, fv) >= 2 * FACTOR


# ---- single pairs
@pytest.mark.parametrize("case_id", PROOF_CASES)
def test_single_must_be_seen_pairs_exceed_the_sum_bound(case_id):
    """Dropping ONE probed "must be seen" (row, target) pair from dK / dV: the share of pairs whose factor is below 10 is at
    most a quarter, and every kind the case has, the block-edge rows and both key-edge classes (target % 32 = 0 / 31) keep at
    least MIN_ROWS pairs at 10 or above (a class of n < 4/3 MIN_ROWS pairs: three quarters of them, the same share).  A single
    block edge holds one or two such pairs only (H_q rows, half of them "must not" kinds), so the edges count as one class;
    how many of them keep a pair is printed.  sink_last pairs count only in the sink_cap cases (_blind)."""
    case, pr, ref = _case(case_id)
    Nq = case["shape"][3]
    f = single_pair_factors(pr, ref, UNIT_ROUNDOFF[pr["q"].dtype])
    kind = pr["kind"]
    must = torch.tensor([P.MUST_SEE[k] for k in P.KINDS])[kind]
    if not case.get("sink_cap"):
        sl = kind == P.KINDS.index("sink_last")
        if bool(sl.any()):
            print(f"{case_id} sink_last (blind by construction): {int((f[sl] >= FACTOR).sum())} of {int(sl.sum())} pairs at {FACTOR:.0f} x")
        must = must & ~sl
    good = must & (f >= FACTOR)
    rows = torch.arange(Nq).view(1, 1, Nq).expand_as(must)
    classes = {name: kind == i for i, name in enumerate(P.KINDS) if P.MUST_SEE[name]}
    classes.update({"block edge": rows % P.BLOCK == P.BLOCK - 1, "key % 32 = 0": pr["target"] % 32 == 0,
                    "key % 32 = 31": pr["target"] % 32 == 31})
    share = 1.0 - good.sum().item() / must.sum().item()
    print(f"{case_id}: {int(must.sum())} pairs, share below {FACTOR:.0f} x: {share:.4f}, smallest factor {f[must].min().item():.2f}")
    assert share <= 0.25
    for name, sel in classes.items():
        n, ok = int((must & sel).sum()), int((good & sel).sum())
        if n:
            print(f"   {name}: {ok} of {n} at {FACTOR:.0f} x or above, smallest {f[must & sel].min().item():.2f}")
            assert ok >= min(P.MIN_ROWS, math.ceil(0.75 * n)), (case_id, name, ok, n)
    edges = [e for e in range(P.BLOCK - 1, Nq, P.BLOCK) if bool(must[:, :, e].any())]
    print(f"   block edges with such a pair: {len(edges)}, of which {sum(bool(good[:, :, e].any()) for e in edges)} keep one at {FACTOR:.0f} x")


# ---- the sink edge
BEFORE_SINK_CAP = {"d64": "04bcee4f6225b0cfecff7db7398cf70f565c41e7a127cbc0f02ca82763263698",
                   "strip80_aux": "15c4330aa4f2c4a2a7228bc13f69dfad8156f5007110ec852d8a4697cfcbd950"}

def _digest(pr):
    import hashlib
    h = hashlib.sha256()
    for name in ("k", "kind", "target", "pair"):          # integers and +-1 codes only: exact whatever the CPU
        x = pr[name]
        h.update((x.to(torch.int8) if x.dtype != torch.long else x).numpy().tobytes())
    return h.hexdigest()


def test_sink_cap_is_off_by_default_and_keeps_single_edge_rows():
    """sink_cap = None leaves dense_probe as it was (digests of k, kind, target, pair taken before the keyword existed: they
    cover every draw from the generator but the randn values themselves); with it, k / v / dO and the rows that are not
    re-aimed do not change, every (batch, KV head) holds exactly SINK_CAP sink_last rows, all single, every block edge beyond the
    window is kept by some group, and every kept row exceeds the dV / dK sum bound tenfold ON ITS OWN."""
    for cid, want in BEFORE_SINK_CAP.items():
        assert _digest(P.dense_case_probe(next(c for c in P.DENSE_CASES if c["id"] == cid))) == want, cid
    SL = P.KINDS.index("sink_last")
    for cid in ("sinkcap_d128", "sinkcap_rowsplit"):
        case, pr, ref = _case(cid)
        B, Hq, Hkv, Nq, Nk, D, ns, W = case["shape"]
        off = P.dense_probe(B, Hq, Hkv, Nq, Nk, D, ns, W, pr["q"].dtype, 1000 + [c["id"] for c in P.DENSE_CASES].index(cid))
        assert all(torch.equal(pr[x], off[x]) for x in ("k", "v", "do"))
        same = (pr["kind"] == off["kind"]) & (pr["pair"] == off["pair"])
        assert torch.equal(pr["q"][same], off["q"][same]) and bool((pr["kind"][~same & (pr["kind"] != SL)] == 0).all())
        sl = pr["kind"] == SL
        assert sl.view(B, Hkv, -1).sum(-1).tolist() == [[P.SINK_CAP] * Hkv] * B and not bool((sl & pr["pair"]).any())
        assert int((off["kind"] == SL).view(B, Hkv, -1).sum(-1).min()) > 20 * P.SINK_CAP      # (what the cap removes)
        beyond = [e for e in range(P.BLOCK - 1, Nq, P.BLOCK) if e - W + 1 > ns - 1]
        assert len(beyond) >= 4 and all(bool(sl[:, :, e].any()) for e in beyond), (cid, beyond)
        f = single_pair_factors(pr, ref, UNIT_ROUNDOFF[pr["q"].dtype])[sl]
        print(f"{cid}: factors of the {f.numel()} kept sink_last rows, each alone: {f.min().item():.1f} .. {f.max().item():.1f}")
        assert f.min().item() >= FACTOR


# ---- the rounding model
def _model_ratios(pr, ns, W, ref):
    u = UNIT_ROUNDOFF[pr["q"].dtype]
    _, dq, dk, dv = rounded_model_bwd(pr["q"], pr["k"], pr["v"], pr["do"], ns, W, pr["s_aux"])
    rq = ((dq.double() - ref["dq"]).abs() / (TOL_G[0] + TOL_G[1] * ref["dq"].abs())).max().item()
    return sum_bound_ratio(dk, ref["dk"], ref["a_k"], u), sum_bound_ratio(dv, ref["dv"], ref["a_v"], u), rq


@pytest.mark.parametrize("case", [c for c in P.DENSE_CASES if c["dtype"] != "fp32"], ids=lambda c: c["id"])
def test_the_rounding_model_stays_within_half_of_the_sum_bound(case):
    """util.rounded_model_bwd (p and dS packed to the dtype, Delta from the rounded O, f32 LSE, results rounded) against the
    fp64 oracle on the inputs of every bf16 / fp16 dense case of the GPU file: the 4 of the bound is not fitted to a kernel"""
    ns, W = case["shape"][6:]
    if case["id"] in PROOF_CASES:
        _, pr, ref = _case(case["id"])
    else:
        pr = P.dense_case_probe(case)
        o, lse, (dq, dk, dv, _, a_k, a_v) = probe_reference(pr, ns, W)
        ref = dict(dq=dq, dk=dk, dv=dv, a_k=a_k, a_v=a_v)
    rk, rv, rq = _model_ratios(pr, ns, W, ref)
    print(f"model {case['id']}: dK {rk:.3f} dV {rv:.3f} of the sum bound, dQ {rq:.3f} of its tolerance")
    assert rk <= 0.5 and rv <= 0.5 and rq <= 0.5, (rk, rv, rq)
    assert_within_sum_bound(ref["dk"].to(pr["q"].dtype), ref["dk"], ref["a_k"], UNIT_ROUNDOFF[pr["q"].dtype], "rounded reference")


@pytest.mark.parametrize("i", range(len(P.VARLEN_CASES)))
def test_the_rounding_model_stays_within_half_of_the_sum_bound_on_the_packs(i):
    c = P.VARLEN_CASES[i]
    pr = P.pack_case_probe(i)
    worst = [0.0, 0.0, 0.0]
    for a, b in zip(c["cu"][:-1], c["cu"][1:]):
        if b > a:
            sq = {x: (pr[x][:, :, a:b] if x != "s_aux" else pr[x]) for x in ("q", "k", "v", "do", "s_aux")}
            _, _, (dq, dk, dv, _, a_k, a_v) = probe_reference(sq, c["ns"], c["W"])
            worst = [max(x, y) for x, y in zip(worst, _model_ratios(sq, c["ns"], c["W"], dict(dq=dq, dk=dk, dv=dv, a_k=a_k, a_v=a_v)))]
    print(f"model pack {i}: dK {worst[0]:.3f} dV {worst[1]:.3f} of the sum bound, dQ {worst[2]:.3f} of 5e-2 + 5e-2 |ref|")
    assert max(worst[:2]) <= 0.5, worst
