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
       drawn kind agrees with valid_mask, and every block edge is probed by every kind in turn.
"""
import math
import random

import pytest
import torch

import probe_inputs as P
from oracle import sink_oracle as O
from test_decode_multi_host import history_keys
from test_tree_host import depths, path_to, random_tree

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
            assert bool(pr["pair"][:, :, edges].all())
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
