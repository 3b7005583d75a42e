"""Mask-edge probe inputs: q / k / v whose softmax puts (almost) all of a row's mass on ONE chosen key that sits on an
edge of the attention mask, so that a mask wrong by one key at that edge moves the row by O(1) instead of O(1 / W).
Plain torch on the CPU; imports neither the product nor a GPU.  tests/test_probe_inputs.py proves on the CPU (fp64
oracle against mutated oracle) that these inputs tell a one-key mask error from a correct mask and that randn does not.

Construction
  * every key position j gets a random code c_j in {-1, +1}^D (exact in bf16 / fp16): k[j] = c_j;
  * row i aims at a target key t(i): q[i] = a * c_t.  The scaled logit is a * sqrt(D) on the target and about
    a * N(0, 1) on every other key;
  * PAIR rows aim at the target and at one interior key u as well (one of positions p - 2 .. p - 33, up to p - 257 on block-edge rows, visible whatever a
    one-key mutant does; the one whose dP = dO . v differs most from the target's, because dQ of the row is proportional
    to that difference): q[i] = a * (c_t + c_u), entries in {-2a, 0, +2a}.  Both logits are EQUAL (a * (D + c_t . c_u) / sqrt(D)), so
    if both keys are seen P is 1/2, 1/2 and dQ of the row is O(1); if only one is seen P is 1, 0 and dQ is about 0.  Single
    rows cannot move dQ by ten tolerances (a peaked row and a diffuse row both have dS near 0); pair rows are what makes
    condition (2b) hold on dQ.  dK / dV have a tolerance that scales with max |ref| and sees no single key; they are judged
    element by element against the bound of their own sum as well (tests/util.py::assert_within_sum_bound), which a single
    row moves by up to 1 / (4 u) (condition (2d));
  * sink_cap (the sinkcap_* cases): hundreds of rows per KV head aim at key num_sink - 1, and one contribution missing
    among n equal ones is invisible at a relative precision of 4 u; with sink_cap only that many rows per (batch, KV head)
    keep sink_last, as single rows on block edges, and the others aim at diag;
  * v and dO stay randn rounded to the dtype; s_aux is the usual 0.5 * randn.

Kinds (the edges of oracle.sink_oracle.valid_mask; p = position of the row in its sequence, ns = num_sink, W = window):
  diag          t = p              must be seen           future        t = p + 1        must not
  win_oldest    t = p - W + 1      must be seen           win_behind    t = p - W        must not (a sink key is left out)
  sink_last     t = ns - 1         must be seen from      sink_next     t = ns           must not, for rows beyond the
                                   rows beyond the window                                window
  prev_last     the last key of the previous sequence of a pack                          must not
  pack_sink     key ns - 1 of the PACK (sequence 0's last sink), from later sequences    must not
A kind exists for a row when its target exists and valid_mask agrees with the kind's "must" (checked by the CPU test);
the kind of a row is drawn from the kinds that exist for it.  The q heads of one KV group take DIFFERENT kinds for the same
row (consecutive entries of the row's list), and the last row of every 256-row block walks the list with
(block * H_q + head), so that every block edge is probed by every kind in turn; block-edge rows are pair rows.
The ring / tree calls are the same picture over the chronological history: a chunk of n tokens after `total` history
tokens is attention with N_q = n < N_kv = total + n (kinds: the oldest key a row still sees, the key it has just lost -
still physically in the ring -, the chunk's own later token, the sink edge); a tree node adds `sibling` and `lower`
(a non-ancestor of lower depth), both "must not", and `parent`.

Amplitude (tests/test_probe_inputs.py::test_amplitude_is_the_smallest_power_of_two): a = 2 for every head dim, the smallest
power of two for which every mask mutant exceeds the O and dQ tolerances tenfold (smallest factor measured at a = 2: dQ 12.3,
O 41; at a = 1 and D = 64: 9.0).  Largest scaled logit: a * sqrt(D) = 11.3 / 16 / 17.9 / 19.6 / 22.6 / 32 on a single row at
D = 32 / 64 / 80 / 96 / 128 / 256, and a * (D + c . c') / sqrt(D), about a * (sqrt(D) + 4) at most, on a pair row.

The single-token decode probes (decode_probe, DECODE_KINDS, at the end of the file) are the same idea over the sink buffer
and the ring as the fused step reads them: one query per (batch, q head), the edges of the step's key set and of its split
plan (tests/decode_regime.py), s_aux at the target's logit; tests/test_decode_probes.py holds their CPU proofs.
"""
import torch

KINDS = ("diag", "future", "win_oldest", "win_behind", "sink_last", "sink_next", "prev_last", "pack_sink")
MUST_SEE = {"diag": True, "future": False, "win_oldest": True, "win_behind": False, "sink_last": True,
            "sink_next": False, "prev_last": False, "pack_sink": False}
TREE_KINDS = ("self", "parent", "sibling", "lower", "ring_oldest", "ring_lost", "sink_last")
TREE_MUST_SEE = {"self": True, "parent": True, "sibling": False, "lower": False, "ring_oldest": True,
                 "ring_lost": False, "sink_last": True}
BLOCK = 256            # row block of the forward / dQ / dK/dV kernels
PAIR_MIN_WINDOW = 5    # p - 2 stays inside the window of every one-key mutant
PAIR_OFFSETS = 32      # partner candidates p - 2 .. p - 33
PAIR_OFFSETS_EDGE = 256  # ... and p - 2 .. p - 257 for the last row of a 256-row block: a mutant restricted to block edges
                         # is caught by a handful of rows, each of which has to clear the factor on its own

# head dim -> amplitude (power of two, exact in every dtype)
AMPLITUDE = {32: 2.0, 40: 2.0, 48: 2.0, 64: 2.0, 80: 2.0, 96: 2.0, 128: 2.0, 256: 2.0,
             16: 4.0}   # D = 16 (the decode probes only): a sqrt(D) = 16 as at D = 64; a = 2 leaves the target below the other keys' sum


def amplitude(D):
    return AMPLITUDE[D]


def _rand(shape, g, dtype, scale=1.0):
    return (torch.randn(*shape, generator=g, dtype=torch.float32) * scale).to(dtype)


def codes(shape, g, dtype, device="cpu"):
    """random +-1 key codes (exact in every dtype); g: a torch.Generator of that device, or None for the global one"""
    return (torch.randint(0, 2, shape, generator=g, device=device).float() * 2 - 1).to(dtype)


def row_targets(Nq, Nk, ns, W, cu=None):
    """Per row of a dense call (cu None; rows are the LAST Nq positions of Nk keys) or of a pack (cu: sequence
    boundaries, Nq == Nk == cu[-1]): exist [K, Nq] bool and target [K, Nq] (absolute key index, -1 where the kind does
    not exist), and the pair partner candidates [PAIR_OFFSETS_EDGE, Nq] (absolute key index of positions p - 2 .. p - 33, -1 where
    the position does not exist or is not safely inside the window)."""
    rows = torch.arange(Nq)
    if cu is None:
        start = torch.zeros(Nq, dtype=torch.long)
        length = torch.full((Nq,), Nk, dtype=torch.long)
        p = rows + (Nk - Nq)
    else:
        assert Nq == Nk == cu[-1]
        start = torch.zeros(Nq, dtype=torch.long)
        length = torch.zeros(Nq, dtype=torch.long)
        for a, b in zip(cu[:-1], cu[1:]):
            start[a:b], length[a:b] = a, b - a
        p = rows - start
    W = max(W, 0)
    far = p - W + 1                      # first position of the window
    t = {"diag": p, "future": p + 1, "win_oldest": p - W + 1, "win_behind": p - W,
         "sink_last": torch.full_like(p, ns - 1), "sink_next": torch.full_like(p, ns)}
    ex = {"diag": (W >= 1) | (p < ns),
          "future": p + 1 < length,
          "win_oldest": (W >= 1) & (p - W + 1 >= ns),
          "win_behind": p - W >= ns,
          "sink_last": (ns >= 1) & (far > ns - 1),
          "sink_next": (ns >= 1) & (far > ns)}
    exist = torch.zeros(len(KINDS), Nq, dtype=torch.bool)
    target = torch.full((len(KINDS), Nq), -1, dtype=torch.long)
    for i, kind in enumerate(KINDS[:6]):
        e = ex[kind] if torch.is_tensor(ex[kind]) else torch.full((Nq,), bool(ex[kind]))
        exist[i] = e
        target[i] = torch.where(e, t[kind] + start, torch.full_like(p, -1))
    later = start > 0
    exist[6], target[6] = later, torch.where(later, start - 1, torch.full_like(p, -1))
    ps = later & (ns >= 1) & (start > ns - 1)
    exist[7], target[7] = ps, torch.where(ps, torch.full_like(p, ns - 1), torch.full_like(p, -1))
    # pair partners: positions p - 2 .. p - 33 of the row's own sequence that stay inside the window of every one-key
    # mutant (p - off >= p - W + 3); [PAIR_OFFSETS_EDGE, Nq] absolute key index or -1
    off = torch.arange(2, 2 + PAIR_OFFSETS_EDGE).view(-1, 1)
    ok = (p.view(1, -1) - off >= 0) & (off <= W - 3)
    partner = torch.where(ok, p.view(1, -1) - off + start.view(1, -1), torch.full_like(ok, -1, dtype=torch.long))
    return exist, target, partner


def _draw(exist, Hq, Hkv, g, edge_rows):
    """kind index [Hq, R]: consecutive entries of each row's list of existing kinds for the heads of one KV group;
    rows flagged in edge_rows (value = block index, -1 elsewhere) walk the list with block * Hq + head."""
    K, R = exist.shape
    n_exist = exist.sum(0)
    assert bool((n_exist >= 1).all()), "a row without any probe kind"
    grp = Hq // Hkv
    base = torch.randint(0, 1 << 20, (Hkv, R), generator=g)
    h = torch.arange(Hq).view(Hq, 1)
    c = base.repeat_interleave(grp, dim=0) + (h % grp)
    c = torch.where(edge_rows.view(1, R) >= 0, edge_rows.view(1, R) * Hq + h, c)
    want = c % n_exist.view(1, R)                                # [Hq, R]
    order = torch.cumsum(exist.long(), 0) - 1                    # [K, R]
    hit = exist.view(1, K, R) & (order.view(1, K, R) == want.view(Hq, 1, R))
    return hit.long().argmax(1)


def _cap_sink_rows(kind, exist, edge, Hkv, cap):
    """Keep at most `cap` rows per (batch, KV head) aimed at sink_last and re-aim the others at diag (in place, no random
    draw).  Block-edge rows come first: group s = batch * H_kv + KV head takes the block edges s * cap, s * cap + 1, ... (mod
    their number) of those on which sink_last exists, on the head that drew sink_last there, else on head (block mod group
    size), whose kind is overwritten - so that over the groups every block edge beyond the window is kept somewhere; where
    there are fewer such edges than `cap`, the first other sink_last rows fill up.  Returns keep [B,Hq,R]."""
    B, Hq, R = kind.shape
    grp = Hq // Hkv
    SL, DIAG = KINDS.index("sink_last"), KINDS.index("diag")
    keep = torch.zeros(B, Hq, R, dtype=torch.bool)
    edges = torch.nonzero((edge >= 0) & exist[SL]).flatten().tolist()
    for b in range(B):
        for hk in range(Hkv):
            s, h0 = b * Hkv + hk, hk * grp
            mine = [edges[(s * cap + x) % len(edges)] for x in range(min(cap, len(edges)))]
            for r in mine:
                drew = torch.nonzero(kind[b, h0:h0 + grp, r] == SL).flatten()
                h = h0 + (int(drew[0]) if drew.numel() else int(edge[r]) % grp)
                kind[b, h, r], keep[b, h, r] = SL, True
            h, r = torch.nonzero((kind[b, h0:h0 + grp] == SL) & ~keep[b, h0:h0 + grp], as_tuple=True)
            order = sorted(range(h.numel()), key=lambda x: (int(r[x]), int(h[x])))
            for x in order[:cap - len(mine)]:
                keep[b, h0 + int(h[x]), r[x]] = True
    drop = (kind == SL) & ~keep
    assert bool(exist[DIAG].view(1, 1, R).expand_as(drop)[drop].all()), "a capped sink_last row without a diagonal key"
    kind[drop] = DIAG
    return keep


def dense_probe(B, Hq, Hkv, Nq, Nk, D, ns, W, dtype, seed, aux=False, cu=None, a=None, pairs=True, sink_cap=None):
    """Probe inputs of one dense call (or one pack, B = 1 and cu given).  Returns a dict: q [B,Hq,Nq,D], k / v
    [B,Hkv,Nk,D], do, s_aux (or None), kind [B,Hq,Nq] (index into KINDS), target [B,Hq,Nq] (absolute key index),
    pair [B,Hq,Nq] bool, partner [B,Hq,Nq] (absolute key index, -1 on single rows).
    sink_cap (default None: off, every output as before): at most that many rows per (batch, KV head) aim at sink_last, as
    SINGLE rows; the others are re-aimed at diag.  Hundreds of rows per KV head aim at key num_sink - 1 otherwise, and one
    contribution missing among n equal ones cannot be seen in dK / dV of that key at a relative precision of a few u."""
    a = amplitude(D) if a is None else a
    g = torch.Generator().manual_seed(seed)
    k = codes((B, Hkv, Nk, D), g, dtype)
    v = _rand((B, Hkv, Nk, D), g, dtype)
    do = _rand((B, Hq, Nq, D), g, dtype)
    sa = _rand((Hq,), g, torch.float32, 0.5) if aux else None
    exist, target, partner = row_targets(Nq, Nk, ns, W, cu)
    rows = torch.arange(Nq)
    edge = torch.where(rows % BLOCK == BLOCK - 1, rows // BLOCK, torch.full_like(rows, -1))
    grp = Hq // Hkv
    kind = torch.stack([_draw(exist, Hq, Hkv, g, edge) for _ in range(B)])              # [B, Hq, Nq]
    single = _cap_sink_rows(kind, exist, edge, Hkv, sink_cap) if sink_cap is not None else None
    tgt = target.t()[rows.view(1, 1, Nq), kind]                                          # [B, Hq, Nq]
    kq = k.float().repeat_interleave(grp, dim=1)                                         # [B, Hq, Nk, D]
    vq = v.float().repeat_interleave(grp, dim=1)
    take = lambda x, idx: torch.gather(x, 2, idx.clamp(min=0).unsqueeze(-1).expand(B, Hq, Nq, D))
    # the partner of a pair row: the candidate whose dP = dO . v differs most from the target's (dQ of the row is
    # proportional to that difference)
    dp_t = (do.float() * take(vq, tgt)).sum(-1)
    best, best_gap = torch.full((B, Hq, Nq), -1, dtype=torch.long), torch.full((B, Hq, Nq), -1.0)
    er = torch.nonzero(edge >= 0).flatten()                      # block-edge rows: the wider candidate list
    for c in range(partner.shape[0]):
        r = slice(None) if c < PAIR_OFFSETS else er
        if c >= PAIR_OFFSETS and er.numel() == 0:
            break
        n_r = Nq if c < PAIR_OFFSETS else er.numel()
        cand = partner[c][r].view(1, 1, n_r).expand(B, Hq, n_r)
        vc = torch.gather(vq, 2, cand.clamp(min=0).unsqueeze(-1).expand(B, Hq, n_r, D))
        gap = ((do.float()[:, :, r] * vc).sum(-1) - dp_t[:, :, r]).abs()
        gap = torch.where(cand >= 0, gap, torch.full_like(gap, -1.0))
        better = gap > best_gap[:, :, r]
        best[:, :, r] = torch.where(better, cand, best[:, :, r])
        best_gap[:, :, r] = torch.where(better, gap, best_gap[:, :, r])
    pair = (torch.rand(B, Hq, Nq, generator=g) < 0.5) | (edge >= 0).view(1, 1, Nq)
    pair &= (best >= 0) & bool(pairs)
    if single is not None:
        pair &= ~single
    q = a * (take(kq, tgt) + take(kq, best) * pair.unsqueeze(-1))
    partner = torch.where(pair, best, torch.full_like(best, -1))
    return dict(q=q.to(dtype), k=k, v=v, do=do, s_aux=sa, kind=kind, target=tgt, pair=pair, partner=partner, a=a)


def randn_like_probe(pr, seed):
    """The randn inputs of the same shapes (tests/util.py::rand), for the comparison of part (2a)."""
    g = torch.Generator().manual_seed(seed)
    out = dict(pr)
    for name in ("q", "k", "v", "do"):
        if pr[name] is None:
            continue
        out[name] = _rand(tuple(pr[name].shape), g, pr[name].dtype)
    return out


def chunk_probe(B, Hq, Hkv, D, ns, W, total, n, dtype, seed, aux=True, a=None):
    """Multi-token call over the ring: `total` history tokens then a chunk of n.  q / k / v hold the WHOLE history on dim 2
    ([.., total + n, D]; q rows of the history are zero), as tests/test_gpu_decode_multi.py::_tokens does; kind / target
    are per chunk row, target an index into the history (tests/test_decode_multi_host.py::history_keys).  The sink rows
    hold the first min(total, ns) tokens.  s_aux at 0.8 * randn as the neighbouring tests."""
    sl = min(total, ns)
    pr = dense_probe(B, Hq, Hkv, n, total + n, D, sl, W, dtype, seed, aux=False, a=a, pairs=False)
    g = torch.Generator().manual_seed(seed + 1)
    pr["s_aux"] = _rand((Hq,), g, torch.float32, 0.8) if aux else None
    pr["q"] = torch.cat([torch.zeros(B, Hq, total, D, dtype=dtype), pr["q"]], dim=2)
    pr["do"] = None
    return pr


def _depths(parent):
    d = []
    for u, p in enumerate(parent):
        d.append(0 if p < 0 else d[p] + 1)
    return d


def _ancestors(parent, u):
    out = []
    while u >= 0:
        out.append(u)
        u = parent[u]
    return out


def tree_probe(B, Hq, Hkv, D, ns, W, total, parent, dtype, seed, aux=True, a=None):
    """Tree call over the ring: node u sits at position total + depth(u) and sees the sinks, ring keys
    [max(sl, total + d - W + 1), total) and its ancestors (itself included) within W - 1 levels.  Key index of node v in
    cat(history, chunk) is total + v.  Kinds per (q head, node): TREE_KINDS."""
    a = amplitude(D) if a is None else a
    n = len(parent)
    sl = min(total, ns)
    d = _depths(parent)
    g = torch.Generator().manual_seed(seed)
    k = codes((B, Hkv, total + n, D), g, dtype)
    v = _rand((B, Hkv, total + n, D), g, dtype)
    sa = _rand((Hq,), g, torch.float32, 0.8) if aux else None
    K = len(TREE_KINDS)
    exist = torch.zeros(K, n, dtype=torch.bool)
    target = torch.full((K, n), -1, dtype=torch.long)
    for u in range(n):
        anc = set(_ancestors(parent, u))
        cand = {}
        if W >= 1:
            cand["self"] = total + u
        if parent[u] >= 0 and W >= 2:
            cand["parent"] = total + parent[u]
        sib = [x for x in range(n) if x != u and parent[x] == parent[u]]
        if sib:
            cand["sibling"] = total + sib[0]
        low = [x for x in range(n) if d[x] < d[u] and x not in anc]
        if low:
            cand["lower"] = total + low[-1]
        first = total + d[u] - W + 1
        if sl <= first < total:
            cand["ring_oldest"] = first
        if sl <= first - 1 < total:
            cand["ring_lost"] = first - 1
        if sl >= 1 and first > sl - 1:
            cand["sink_last"] = sl - 1
        for name, t in cand.items():
            exist[TREE_KINDS.index(name), u], target[TREE_KINDS.index(name), u] = True, t
    none = torch.full((n,), -1, dtype=torch.long)
    kind = torch.stack([_draw(exist, Hq, Hkv, g, none) for _ in range(B)])
    tgt = target.t()[torch.arange(n).view(1, 1, n), kind]
    kq = k.float().repeat_interleave(Hq // Hkv, dim=1)
    qc = a * torch.gather(kq, 2, tgt.unsqueeze(-1).expand(B, Hq, n, D))
    q = torch.cat([torch.zeros(B, Hq, total, D), qc], dim=2).to(dtype)
    return dict(q=q, k=k, v=v, s_aux=sa, kind=kind, target=tgt, exist=exist, a=a)


def kind_counts(pr, kinds=KINDS):
    """{kind name: smallest number of rows over (batch, q head)} of one probe."""
    kd = pr["kind"]
    return {name: int((kd == i).sum(-1).min()) for i, name in enumerate(kinds)}


# ------------------------------------------------------------------------------------------------ case tables
# The cases of tests/test_gpu_mask_edges.py; tests/test_probe_inputs.py checks the kind coverage of every one on the CPU.
# shape = (B, Hq, Hkv, Nq, Nk, D, ns, W).  fwd / dq: substrings sfa_last_path() must show after the forward / the backward.
# missing: the kinds the case lacks BY CONSTRUCTION (every other kind of KINDS[:6] must have >= MIN_ROWS rows per q head).
MIN_ROWS = 8
SINK_CAP = 4           # rows per (batch, KV head) aimed at sink_last in the sink-edge cases (tests/test_probe_inputs.py: every
                       # kept row clears ten sum bounds of dV on its own)
_NO_WINDOW_EDGE = ("win_oldest", "win_behind", "sink_last", "sink_next")     # W >= N: no row is beyond the window
_NO_SINK = ("sink_last", "sink_next")                                        # num_sink = 0
DENSE_CASES = [
    # hand-placed forward / dQ work lists, dK/dV with the sink tail
    dict(id="c3slice", shape=(1, 4, 1, 8192, 8192, 128, 4, 4096), dtype="bf16", fwd="asm4x64pk", dq="dqasm4x64"),
    dict(id="ragged_fp16", shape=(2, 8, 2, 2100, 2100, 128, 4, 1024), dtype="fp16", fwd="asm4x64pk", dq="dqasm4x64"),
    dict(id="d64", shape=(1, 4, 2, 3000, 3000, 64, 70, 700), dtype="bf16", fwd="asm4x64pk", dq="dqasm4x64"),
    dict(id="d80", shape=(1, 4, 2, 3000, 3000, 80, 70, 700), dtype="bf16", fwd="asm4x64pk", dq="dqasm4x64"),
    dict(id="d96", shape=(1, 4, 2, 3000, 3000, 96, 70, 700), dtype="fp16", fwd="asm4x64pk", dq="dqasm4x64"),
    # sink split of block 0's sweep, sinks over more than one block
    dict(id="sinks300", shape=(1, 2, 1, 3000, 3000, 96, 300, 512), dtype="bf16", fwd="asm4x64pk", dq="dqasm4x64"),
    dict(id="n20000_w32", shape=(1, 2, 1, 20000, 20000, 128, 4, 32), dtype="bf16", fwd="asm4x64pk", dq="dqasm4x64"),
    # row split on a small grid, and its compiled fallback (N_q < N_kv; W >= N_kv)
    dict(id="rowsplit", shape=(1, 4, 1, 2048, 2048, 128, 4, 512), dtype="bf16", fwd="asm4x64pk", dq="dqasm4x64",
         rule_dkdv="dkdvasm4x64rs"),
    dict(id="rowsplit_fallback", shape=(1, 8, 2, 1024, 1200, 128, 4, 4096), dtype="bf16", fwd="asm4x64pk", dq="dqasm4x64",
         rule_dkdv="dkdvws8", missing=_NO_WINDOW_EDGE),
    dict(id="nq_lt_nk", shape=(1, 2, 1, 1000, 1300, 128, 4, 600), dtype="bf16", fwd="asm4x64pk", dq="dqasm4x64"),
    # sliding layers: strip forward / dQ, skewed dK/dV sweep
    dict(id="strip80_aux", shape=(1, 8, 1, 2048, 2048, 80, 0, 128), dtype="bf16", aux=True, fwd="stripasm", dq="dq4w",
         missing=_NO_SINK),
    dict(id="strip64_bnhd", shape=(2, 16, 2, 2048, 2048, 64, 0, 128), dtype="bf16", layout="bnhd", fwd="stripasm",
         dq="dq4w", missing=_NO_SINK),
    # ... on a grid that fills the chip twice (cdiv(N, 64) * (group / 4) * H_kv * B >= 2 * CUs): the hand-placed strip dQ body;
    # the two cases above are its small-grid fallback, the compiled 4-wave dQ kernel
    dict(id="strip64_dq", shape=(4, 16, 2, 2048, 2048, 64, 0, 128), dtype="bf16", layout="bnhd", fwd="stripasm",
         dq="dqstripasm", missing=_NO_SINK),
    dict(id="strip80_dq_aux", shape=(2, 16, 2, 4096, 4096, 80, 0, 128), dtype="fp16", aux=True, fwd="stripasm",
         dq="dqstripasm", missing=_NO_SINK),
    dict(id="skew96_w512", shape=(1, 6, 2, 1500, 1500, 96, 0, 512), dtype="bf16", fwd="asm4x64pk", dq="dqasm4x64pk",
         missing=_NO_SINK),
    # compiled MFMA kernels
    dict(id="d32", shape=(2, 4, 2, 1500, 1500, 32, 4, 600), dtype="bf16", fwd="fwd_mfma_bf16_d32", dq="bwd_mfma_bf16_d32"),
    dict(id="d256", shape=(2, 4, 2, 1500, 1500, 256, 4, 600), dtype="fp16", fwd="fwd_mfma_f16_d256", dq="bwd_mfma_f16_d256"),
    # exact-f32 kernels
    dict(id="fp32", shape=(1, 4, 2, 700, 700, 64, 4, 300), dtype="fp32", fwd="fwd_generic", dq="bwd_generic"),
    dict(id="d64_generic", shape=(1, 4, 2, 3000, 3000, 64, 70, 700), dtype="bf16", generic=True, fwd="fwd_generic",
         dq="bwd_generic"),
    # degenerate windows
    dict(id="w0", shape=(1, 4, 2, 777, 777, 128, 4, 0), dtype="bf16", fwd="fwd_mfma", dq="bwd_mfma",
         missing=("win_oldest", "diag")),               # W = 0: the diagonal itself is the first key behind the window
    dict(id="w1", shape=(1, 4, 2, 777, 777, 128, 4, 1), dtype="bf16", fwd="fwd_mfma", dq="bwd_mfma"),
    dict(id="w_ge_n", shape=(1, 4, 2, 777, 777, 128, 4, 1000), dtype="bf16", fwd="fwd_mfma", dq="bwd_mfma",
         missing=_NO_WINDOW_EDGE),
    dict(id="ns_ge_n", shape=(1, 4, 2, 777, 777, 128, 1000, 16), dtype="bf16", fwd="fwd_mfma", dq="bwd_mfma",
         missing=_NO_WINDOW_EDGE),                      # every key is a sink key
    dict(id="ns0", shape=(1, 4, 2, 777, 777, 128, 0, 100), dtype="bf16", fwd="fwd_mfma", dq="bwd_mfma", missing=_NO_SINK),
    # the sink edge in dK / dV: SINK_CAP single rows per (batch, KV head) aim at key num_sink - 1 (dense_probe(sink_cap=)), so
    # that one dropped contribution to that key exceeds the per-element sum bound of tests/util.py; B * H_kv = 4 groups, row
    # head dim 128, with and without the row split of a small grid
    dict(id="sinkcap_d128", shape=(1, 4, 4, 2048, 2048, 128, 4, 512), dtype="bf16", fwd="asm4x64pk", dq="dqasm4x64",
         sink_cap=SINK_CAP),                            # group size 1: too few trips per chunk for the row split, sink tail
    dict(id="sinkcap_rowsplit", shape=(2, 4, 2, 2048, 2048, 128, 4, 512), dtype="bf16", fwd="asm4x64pk", dq="dqasm4x64",
         rule_dkdv="dkdvasm4x64rs", sink_cap=SINK_CAP),
]
# packed batches: the nine cu lists of tests/test_gpu_varlen.py::test_varlen_native_kernels_one_launch; W is the window of
# that table where it is shorter than the pack's sequences, else cut so that the longer sequences have a window edge
VARLEN_CASES = [
    dict(Hq=8, Hkv=2, D=128, ns=4, W=300, cu=[0, 1000, 1001, 1900, 4000, 4127]),
    dict(Hq=4, Hkv=4, D=64, ns=0, W=64, cu=[0, 63, 64, 200, 200, 455], missing=_NO_SINK + ("pack_sink",)),
    dict(Hq=8, Hkv=1, D=80, ns=130, W=50, cu=[0, 129, 700], missing=("pack_sink",)),     # sequence 0 has 129 < ns keys
    dict(Hq=4, Hkv=2, D=96, ns=2, W=200, cu=[0, 257, 640]),
    dict(Hq=4, Hkv=1, D=96, ns=0, W=4096, cu=[0, 200, 264, 265], missing=_NO_WINDOW_EDGE + ("pack_sink",)),
    dict(Hq=1, Hkv=1, D=80, ns=130, W=300, cu=[0, 200, 400], missing=_NO_WINDOW_EDGE),
    dict(Hq=8, Hkv=2, D=128, ns=4, W=300, cu=[0, 1100, 1101, 2300, 4400]),
    dict(Hq=16, Hkv=16, D=128, ns=4, W=600, cu=[0, 4500, 9000]),
    dict(Hq=16, Hkv=2, D=80, ns=0, W=128, cu=[0, 300, 301, 1500, 2100], missing=_NO_SINK + ("pack_sink",)),
]
# multi-token calls over a FULL ring: (dtype, B, Hq, Hkv, D, ns, W, extra, n): the cache holds ns + W + extra tokens
# (write_pos = extra mod W); extra = W - n / 2 makes the chunk's commit wrap past slot 0 mid-chunk
CHUNK_CASES = [
    ("bf16", 1, 16, 2, 64, 4, 1024, 37, 8),
    ("bf16", 1, 16, 2, 64, 4, 1024, 1004, 40),
    ("fp16", 2, 8, 2, 128, 4, 4096, 4092, 8),
    ("bf16", 1, 16, 2, 128, 4, 4096, 4076, 40),
    ("fp16", 1, 32, 4, 64, 0, 1024, 1, 1),           # the one-token ring decode as n = 1 (no sinks: three kinds on 32 heads)
    ("fp32", 1, 16, 2, 64, 2, 1024, 1020, 8),        # f32-accumulate path
]
# trees: the table of tests/test_gpu_tree_verify.py (num_sink, ring capacity, prefill, single appends, n, shape, forest)
# and two rows at ring capacity 1024 (ring full and wrapped)
TREE_CASES_EXTRA = [
    (4, 1024, 1028, 13, 24, "random", True),
    (0, 1024, 1500, 3, 64, "deep", False),
]
# row of TREES + TREE_CASES_EXTRA -> the tree kinds it lacks BY CONSTRUCTION (every other kind of TREE_KINDS must have
# >= MIN_ROWS (node, head) probes over the case)
_NO_RING_EDGE = ("ring_oldest", "ring_lost", "sink_last")
TREE_MISSING = {
    0: _NO_RING_EDGE,                           # 9 tokens in a ring of 16: no node is deep enough to lose a ring key
    3: ("lower", "sink_last"),                  # a star has no non-ancestor of lower depth; num_sink = 0
    5: ("ring_oldest", "ring_lost"),            # 3 tokens of history, 2 of them sinks: one ring key, seen by 2 nodes
    7: ("sink_last",),                          # num_sink = 0
}
# per-sequence device state: one ragged batch of three fill levels (tokens held per sequence) at ring capacity 1024
# (ring partly filled; filled by the chunk's 4th token; full and wrapped).  missing: per sequence
RAGGED_CASE = dict(ns=4, W=1024, lengths=[300, 4 + 1024 - 4, 2500], n=8, Hq=16, Hkv=2, D=64, dtype="bf16",
                   missing=[_NO_WINDOW_EDGE, (), ()])


# ------------------------------------------------------------------------------------------------ the inputs of each case
# (one builder per table, used by the GPU test AND by the coverage test: the inputs whose coverage is asserted are the
# inputs that run)
_DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
TREE_RNG_SEED = 400        # random_tree(random.Random(TREE_RNG_SEED + i), ...) for row i of TREES + TREE_CASES_EXTRA
TREE_SHAPE = (2, 8, 2)     # B, Hq, Hkv of the tree cases
TREE_DTYPE_D = [("bf16", 64), ("fp16", 128), ("fp32", 48)]


def dense_case_probe(case):
    i = [c["id"] for c in DENSE_CASES].index(case["id"])
    B, Hq, Hkv, Nq, Nk, D, ns, W = case["shape"]
    return dense_probe(B, Hq, Hkv, Nq, Nk, D, ns, W, _DT[case["dtype"]], 1000 + i, aux=case.get("aux", False),
                       sink_cap=case.get("sink_cap"))


def pack_case_probe(i):
    c = VARLEN_CASES[i]
    T = c["cu"][-1]
    return dense_probe(1, c["Hq"], c["Hkv"], T, T, c["D"], c["ns"], c["W"], torch.bfloat16, 2000 + i, aux=True, cu=c["cu"])


def chunk_case_probe(row):
    dt, B, Hq, Hkv, D, ns, W, extra, n = row
    return chunk_probe(B, Hq, Hkv, D, ns, W, ns + W + extra, n, _DT[dt], 3000 + CHUNK_CASES.index(row))


def tree_case_probe(i, row, parent, dt, D):
    ns, W, prefill, appends = row[:4]
    B, Hq, Hkv = TREE_SHAPE
    return tree_probe(B, Hq, Hkv, D, ns, W, prefill + appends, parent, _DT[dt], 4000 + i)


def ragged_case_probes():
    c = RAGGED_CASE
    return [chunk_probe(1, c["Hq"], c["Hkv"], c["D"], c["ns"], c["W"], L, c["n"], _DT[c["dtype"]], 5000 + b)
            for b, L in enumerate(c["lengths"])]


# ------------------------------------------------------------------------------------------------ single-token decode
# One query per (batch, q head) over the sink buffer + ring, aimed at ONE key on an edge of what the step may read
# (tests/decode_regime.py names the splits; tests/test_decode_probes.py proves on the CPU that every mutant of the key set
# moves these inputs by ten tolerances).  EVERY row of the four cache buffers holds a +-1 code and a randn value, live or
# not, so the rows beyond the fill and beyond sink_len are planted by construction, and so is the evicted token (the old
# bytes of the slot the step overwrites).  s_aux[h] sits at the target's logit a sqrt(D) (+ 0.25 randn): the target of a
# must-see row holds about half of the softmax mass, so counting it twice moves the row by about |v| / 6, dropping it by
# |v| / 2; a must-not-see row is about zero and moves by |v| / 2 when its target is read.
#   kind          target (key index in the kernel's order: sink rows, then ring slots)           must
#   newest        the token being decoded, N1 + write_pos, read from k_new in the fused step     see
#   evicted       the OLD content of slot write_pos of a full ring                               not
#   ring_oldest   slot write_pos + 1 of a full ring                                              see
#   sink_last     sink row sink_len - 1                                                          see
#   beyond_fill   ring row window_len + 1 (one past the live rows after the step), ring not full not
#   beyond_sink   sink row sink_len < num_sink                                                   not
#   split_first   key k_beg of a split s >= 1                                                    see
#   split_last    key k_end - 1 of a split s >= 1                                                see
#   last_key      key N_kv - 1, the one the clamped tail loads repeat                            see, once
DECODE_KINDS = ("newest", "evicted", "ring_oldest", "sink_last", "beyond_fill", "beyond_sink", "split_first", "split_last",
                "last_key")
DECODE_MUST_SEE = {"newest": True, "evicted": False, "ring_oldest": True, "sink_last": True, "beyond_fill": False,
                   "beyond_sink": False, "split_first": True, "split_last": True, "last_key": True}
DECODE_AUX_JITTER = 0.25


def decode_cache(B, Hkv, D, ns, Wc, dtype, seed):
    """the four cache buffers, every row written: K rows are codes, V rows randn"""
    g = torch.Generator().manual_seed(seed)
    return dict(sink_k=codes((B, Hkv, ns, D), g, dtype), sink_v=_rand((B, Hkv, ns, D), g, dtype),
                window_k=codes((B, Hkv, Wc, D), g, dtype), window_v=_rand((B, Hkv, Wc, D), g, dtype))


def _key_loc(j, N1, slot):
    return ("sink", j) if j < N1 else ("new", 0) if j - N1 == slot else ("ring", j - N1)


def probe_splits(row):
    """the splits s >= 1 of one regime row that hold keys, in the order the probes take them: the last one (index >= 64 on
    the many-split grids), one in [32, 64), split 1, then the others"""
    live = [s for s in range(1, len(row["n_keys"])) if row["n_keys"][s] > 0]
    mid = [s for s in live if 32 <= s < 64]
    pref = live[-1:] + ([40] if 40 in mid else mid[:1]) + live[:1]
    return list(dict.fromkeys(pref + live))


def decode_kinds(state, ns, Wc, row):
    """{kind: [locations]} of one batch row: state = (sink_len, window_len, write_pos) BEFORE the step, row = its entry of
    decode_regime.regime(step=True).  A location is ("sink", r), ("ring", slot) - the bytes in the buffer before the step -
    or ("new", 0): k_new / v_new."""
    sl, wl, wp = state
    N1, Nkv = row["N1"], row["Nkv"]
    out = {k: [] for k in DECODE_KINDS}
    out["newest"] = [("new", 0)]
    if wl == Wc:
        out["evicted"] = [("ring", wp)]
        if Wc >= 2:
            out["ring_oldest"] = [("ring", (wp + 1) % Wc)]
    if sl >= 1:
        out["sink_last"] = [("sink", sl - 1)]
    if wl + 1 < Wc:
        out["beyond_fill"] = [("ring", wl + 1)]
    if sl < ns:
        out["beyond_sink"] = [("sink", sl)]
    pref = probe_splits(row)
    for s, s2 in zip(pref, pref[1:] + pref[:1]):          # (split_last starts one further: the last split may hold one key)
        out["split_first"].append(_key_loc(row["k_beg"][s], N1, wp))
        out["split_last"].append(_key_loc(row["k_beg"][s2] + row["n_keys"][s2] - 1, N1, wp))
    out["last_key"] = [_key_loc(Nkv - 1, N1, wp)]
    return out


def decode_probe(cache, states, Hq, rows, seed, rot=0, a=None):
    """q / k_new / v_new / s_aux of one fused step over `cache` (decode_cache, or a twin that earlier steps advanced) at the
    per-row `states`; rows: decode_regime.regime(...)[1].  The heads of a GQA group take consecutive kinds of the row's
    list (which the (batch, q head) pairs walk on from `rot`), so every head of a group aims at another key as long as the row has as
    many kinds as the group has heads; further heads take split_first / split_last of further splits where the row has
    them.  Returns q [B,Hq,1,D], k_new / v_new [B,Hkv,1,D], s_aux [Hq] f32, kind [B,Hq] (index into DECODE_KINDS),
    loc[b][h] (the target's location), a."""
    B, Hkv, ns, D = cache["sink_k"].shape
    Wc = cache["window_k"].shape[2]
    dtype = cache["sink_k"].dtype
    a = amplitude(D) if a is None else a
    g = torch.Generator().manual_seed(seed)
    k_new, v_new = codes((B, Hkv, 1, D), g, dtype), _rand((B, Hkv, 1, D), g, dtype)
    s_aux = a * D ** 0.5 + DECODE_AUX_JITTER * torch.randn(Hq, generator=g, dtype=torch.float32)
    grp = Hq // Hkv
    q = torch.zeros(B, Hq, 1, D)
    kind = torch.zeros(B, Hq, dtype=torch.long)
    loc = [[None] * Hq for _ in range(B)]
    for b in range(B):
        cand = decode_kinds(states[b], ns, Wc, rows[b])
        names = [k for k in DECODE_KINDS if cand[k]]
        split_kinds = [k for k in ("split_first", "split_last") if cand[k]]
        used = {k: 0 for k in names}
        for hk in range(Hkv):
            r0 = (hk * grp + b * Hq + rot) % len(names)
            seq = names[r0:] + names[:r0]
            for i in range(grp):
                name = seq[i] if i < len(seq) else (split_kinds[i % 2] if split_kinds else seq[i % len(seq)])
                where = cand[name][used[name] % len(cand[name])]
                used[name] += 1
                h = hk * grp + i
                src = {"sink": cache["sink_k"], "ring": cache["window_k"], "new": k_new}[where[0]]
                q[b, h, 0] = a * src[b, hk, where[1]].float()
                kind[b, h], loc[b][h] = DECODE_KINDS.index(name), where
    return dict(q=q.to(dtype), k_new=k_new, v_new=v_new, s_aux=s_aux, kind=kind, loc=loc, a=a)


def decode_kept(cache, state, b, k_new=None, v_new=None):
    """K, V [Hkv, N_kv, D] of batch row b in the kernel's key order - sink rows [0, sink_len), then ring slots [0,
    window_len after the step) with slot write_pos taken from k_new / v_new - and the rows a step must NOT read:
    extras = {"evicted" / "beyond_fill" / "beyond_sink": (K, V) [Hkv, 1, D]} where they exist.  k_new None: no step, the
    keys of the state as it is."""
    sl, wl, wp = state
    Wc = cache["window_k"].shape[2]
    ns = cache["sink_k"].shape[2]
    step = k_new is not None
    wl1 = min(wl + 1, Wc) if step else wl
    rk, rv = cache["window_k"][b, :, :wl1].clone(), cache["window_v"][b, :, :wl1].clone()
    extras = {}
    if step:
        if wl == Wc:
            extras["evicted"] = (rk[:, wp:wp + 1].clone(), rv[:, wp:wp + 1].clone())
        rk[:, wp], rv[:, wp] = k_new[b, :, 0], v_new[b, :, 0]
        if wl + 1 < Wc:
            extras["beyond_fill"] = (cache["window_k"][b, :, wl + 1:wl + 2], cache["window_v"][b, :, wl + 1:wl + 2])
    if sl < ns:
        extras["beyond_sink"] = (cache["sink_k"][b, :, sl:sl + 1], cache["sink_v"][b, :, sl:sl + 1])
    return torch.cat([cache["sink_k"][b, :, :sl], rk], 1), torch.cat([cache["sink_v"][b, :, :sl], rv], 1), extras


def decode_apply(cache, states, k_new, v_new, active=None):
    """the CPU twin of a storing step: slot write_pos of every active row takes k_new / v_new IN PLACE, no other byte
    moves; returns the advanced states"""
    Wc = cache["window_k"].shape[2]
    out = []
    for b, (sl, wl, wp) in enumerate(states):
        if active is not None and not active[b]:
            out.append((sl, wl, wp))
            continue
        cache["window_k"][b, :, wp] = k_new[b, :, 0]
        cache["window_v"][b, :, wp] = v_new[b, :, 0]
        out.append((sl, min(wl + 1, Wc), 0 if wp + 1 == Wc else wp + 1))
    return out


def decode_oracle(cache, states, pr, step=True):
    """fp64 oracle (oracle.sink_oracle.decode_dense) of every batch row over the tokens the cache keeps"""
    from oracle import sink_oracle as O
    rows = []
    for b, st in enumerate(states):
        K, V, _ = decode_kept(cache, st, b, pr["k_new"] if step else None, pr["v_new"] if step else None)
        rows.append(O.decode_dense(pr["q"][b:b + 1], K[None], V[None], pr["s_aux"]))
    return torch.cat(rows, 0)


class DecodeRun:
    """One sequence of fused steps over a CPU twin of the cache: the probe of every step, its regime and its fp64
    reference, and the twin's update.  case: a row of decode_regime.MANY / GROUPS / FILLS; states: one (sink_len,
    window_len, write_pos) per batch row; device_state: the launch is planned for the full cache (decode_step_dyn);
    active: rows of a slots= call that are not -1 (an inactive row gets zeros and nothing of it moves)."""

    def __init__(self, case, states, device_state, seed, rot=0, active=None):
        import decode_regime as R
        self.R, self.case, self.device_state = R, dict(case, B=len(states)), device_state
        self.states, self.seed, self.rot = list(states), seed, rot
        self.active = [True] * len(states) if active is None else list(active)
        self.cache = decode_cache(len(states), case["Hkv"], case["D"], case["ns"], case["Wc"], R.DT[case["dtype"]], seed)

    def probe(self):
        """dict(pl, rows, pr, ref, states) of the next step; the twin does not move"""
        pl, rows = self.R.regime(self.case, self.states, step=True, device_state=self.device_state)
        self.seed, self.rot = self.seed + 1, self.rot + 1
        pr = decode_probe(self.cache, self.states, self.case["Hq"], rows, self.seed, rot=self.rot)
        ref = decode_oracle(self.cache, self.states, pr)
        for b, on in enumerate(self.active):
            if not on:
                ref[b] = 0
        return dict(pl=pl, rows=rows, pr=pr, ref=ref, states=list(self.states), active=self.active)

    def apply(self, pr):
        self.states = decode_apply(self.cache, self.states, pr["k_new"], pr["v_new"], self.active)


FILLS_INACTIVE = 3         # batch row of the slots= form that is inactive (a copy of state 0 nobody stores)


def decode_runs(case):
    """[(name, DecodeRun, steps)] of one case: the launches tests/test_gpu_decode_edges.py makes and
    tests/test_decode_probes.py proves.  many / groups: one host-state step per state of the case (`step<i>`), many also
    `dyn` (shared device state at the second state).  fills: `rows` (one batch row per state), `slots` (the same with an
    inactive row) and `shared<i>` (state i alone, B = 2), three steps each."""
    import decode_regime as R
    tables = R.MANY + R.GROUPS + R.FILLS
    base = 7000 + 100 * [c["id"] for c in tables].index(case["id"])
    B, st = case["B"], case["states"]
    if case in R.FILLS:
        with_off = st[:FILLS_INACTIVE] + [st[0]] + st[FILLS_INACTIVE:]
        act = [b != FILLS_INACTIVE for b in range(len(with_off))]
        runs = [("rows", DecodeRun(case, st, True, base, 0), R.FILLS_STEPS),
                ("slots", DecodeRun(case, with_off, True, base + 10, 3, active=act), R.FILLS_STEPS)]
        runs += [(f"shared{i}", DecodeRun(case, [s, s], True, base + 20 + 4 * i, 6 + i), R.FILLS_STEPS)
                 for i, s in enumerate(st)]
        return runs
    runs = [(f"step{i}", DecodeRun(case, [s] * B, False, base + 10 * i, i * B * case["Hq"]), 1) for i, s in enumerate(st)]
    if case in R.MANY:
        runs.append(("dyn", DecodeRun(case, [st[1]] * B, True, base + 50, 5), 1))
    return runs
