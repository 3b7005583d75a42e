"""Which tiles every wave of the packed serving step walks: a pure-Python restatement of the launch arithmetic of
sfa_decode_ring_ragged_slots, the way tests/grid_regime.py restates the work lists.  Sources
(csrc/sfa_decode_multi.hip): want_splits, max_splits, ragged_geom, multi_plan, fill_state / advance_row (the state row
after a fill and a commit), tile_info (segment and chronological range), tile_class with its admitting `nsk` branch,
key_visible / key_visible_admit, and the tile loop of multi_split_mfma_kernel: split s owns tiles [s tps, (s + 1) tps),
wave w of a split takes tiles s tps + w, + 4, + 8 ..., and next_live steps over the tiles that are dead for the row block.

regime(case) gives, per sequence and 32-row block, S, tps, the last split's length, the tiles per wave, the ordered
(tile, segment, class) walk of every (split, wave) and the (split, wave, iteration) in which each mask-edge key lies.
Tree sequences are not modelled: their chunk tiles are classified from the ancestor bitmask; their sink and ring tiles
follow this model with the depth in place of the row index (a chain tree is the plain sequence).

Three packs at num_sink = 4 (PACKS): the seven sequences of SEQS as (chunk length, history length) and two more
entries, an inactive sequence of 2 tokens (slot -1) and an empty one.  tests/test_packed_regime.py proves on the CPU
what each reaches; tests/test_gpu_packed_long.py runs them.
  walk    H_kv 8, G 8, T_PAD 1024, Wc 320   want = 1: one split per sequence, tps up to 16, a wave walks up to 4 tiles
  capped  H_kv 2, G 8, T_PAD 1024, Wc 1024  want = 4 binds: S = 4, tps = 9 .. 10, waves walk 2 .. 3 tiles
  wide    H_kv 2, G 1 / 8, T_PAD 320, Wc 1024   want = 12 / 54: S = 9 .. 10 beside S in {1, 2}, Sw = 12

Inputs (pack_inputs): randn, the mask-edge probes of tests/probe_inputs.py (chunk_probe per sequence at the long Wc, the
pack-edge row of tests/test_ragged_step_host.py::probe_pack) and softmax-range families built from the pieces of
tests/range_inputs.py along the chronological key order.  Probe amplitude: probe_inputs.amplitude(D) = 2.0, unchanged
at Wc = 320 and 1024: the smallest one-key mutant factor over (pack, type, mutant), printed by
tests/test_packed_regime.py::test_a_one_key_mask_error_moves_a_probe_row_tenfold, is 178 tolerances (capped, bf16 D = 64,
the pack neighbour's first key; fp16: 1489), against the tenfold margin asked for.

kernel_model: the fp64 walk in the kernel's order of operations (per-wave online softmax over its live tiles, the
four-wave merge, the split reduce with s_aux) and three mutants of it."""
import functools
import math

import torch

import probe_inputs as P
import range_inputs as RI

TILE, WAVES, MIN_TILES, TARGET_WGS = 32, 4, 4, 2048
NS = 4
SEG = ("sink", "ring", "chunk")
CLS = ("dead", "full", "edge")
LOG2E = 1.4426950408889634


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ launch arithmetic
def want_splits(B, Hkv, nrb):
    return max(cdiv(TARGET_WGS, max(B * Hkv * nrb, 1)), 1)


def max_splits(B, Hkv, nrb, Nkv):
    return max(min(cdiv(cdiv(Nkv, TILE) + 2, MIN_TILES), want_splits(B, Hkv, nrb)), 1)


def ragged_geom(n_seq, Hq, Hkv, T, Nkv_cache):
    G = Hq // Hkv
    nrb = cdiv(G * T, 32) + n_seq
    rows = Hkv * T * G
    by_keys = max(cdiv(cdiv(Nkv_cache + T, TILE) + 2, MIN_TILES), 1)
    return dict(G=G, nrb=nrb, rows=rows, Sw=max_splits(1, Hkv, nrb, Nkv_cache + T), P=min(rows * by_keys, rows + TARGET_WGS * 32),
                want=want_splits(1, Hkv, nrb))


def multi_plan(sl, wl, n, want):
    T0 = cdiv(sl, TILE)
    T1 = T0 + cdiv(wl, TILE)
    T = T1 + cdiv(n, TILE)
    s = max(min(cdiv(cdiv(sl + wl + n, TILE) + 2, MIN_TILES), want), 1)
    s = min(s, cdiv(T, MIN_TILES))
    tps = cdiv(T, s)
    return dict(T0=T0, T1=T1, T=T, tps=tps, S=cdiv(T, tps))


def state_after(L, ns, wc, fill=None):
    """the state row {sink_len, window_len, write_pos, seen} of a slot that was prefilled with the first `fill` tokens
    (default min(L, ns + wc)) of a history of L and then advanced by commits of the others"""
    fill = min(L, ns + wc) if fill is None else fill
    sl = min(fill, ns)
    rem = fill - sl
    wl, wp = (rem, rem) if rem < wc else (wc, 0)
    acc = L - fill
    return [sl, min(wl + acc, wc), (wp + acc) % wc, L]


def ring_chron(st, wc, s):
    sl, wl, wp, _ = st
    x = s - wp + wl
    x = x - wc if x >= wc else (x + wc if x < 0 else x)
    return x - wl


def ring_slot(st, wc, c):
    """the inverse: the ring slot of chronological key c in [-wl, -1]"""
    sl, wl, wp, _ = st
    return (c + wl + wp - wl) % wc if wl == wc else c + wl


def tile_info(st, wc, n, plan, i):
    """(segment, start, count, cmin, cmax) of tile i"""
    sl, wl, wp, _ = st
    if i < plan["T0"]:
        seg, start, ln = 0, TILE * i, sl
    elif i < plan["T1"]:
        seg, start, ln = 1, TILE * (i - plan["T0"]), wl
    else:
        seg, start, ln = 2, TILE * (i - plan["T1"]), n
    count = min(ln - start, TILE)
    if seg == 2:
        cmin, cmax = start, start + count - 1
    elif seg == 1:
        s1 = start + count - 1
        if wl == wc and start < wp <= s1:
            cmin, cmax = -wc, -1
        else:
            cmin, cmax = ring_chron(st, wc, start), ring_chron(st, wc, s1)
    else:
        cmin = cmax = 0
    return seg, start, count, cmin, cmax


def tile_class(ti, wc, tmin, tmax, nsk=0):
    seg, start, count, cmin, cmax = ti
    if seg == 0:
        return 1 if count == TILE else 2
    if nsk > 0 and seg == 2 and start < nsk:
        if cmin > tmax:
            return 0
        return 1 if (count == TILE and cmax <= tmin and (cmax < nsk or nsk >= tmax - wc + 1)) else 2
    if cmax < tmin - wc + 1 or cmin > tmax:
        return 0
    return 1 if (count == TILE and cmin >= tmax - wc + 1 and cmax <= tmin) else 2


def holds_wrap(st, wc, ti):
    """a ring tile with the wrap inside: the newest keys in its first slots, the oldest behind them"""
    return ti[0] == 1 and st[1] == wc and ti[1] < st[2] <= ti[1] + ti[2] - 1


def tile_keys(st, wc, ti):
    """chronological index of every key of a tile (sink keys: None)"""
    seg, start, count = ti[:3]
    if seg == 0:
        return [None] * count
    if seg == 2:
        return list(range(start, start + count))
    return [ring_chron(st, wc, start + kk) for kk in range(count)]


def visible(seg, c, t, wc, nsk=0):
    return seg == 0 or (c <= t and (c >= t - wc + 1 or (seg == 2 and c < nsk)))


# ------------------------------------------------------------------------------------------------ the packs
# (chunk length, history length): decode on a wrapped ring; a partly filled ring; a ring filled exactly; wrapped, the wrap
# point not on a tile edge; nearly empty; a prompt chunk longer than a tile walk; sink not yet full
def SEQS(wc):
    return [(1, NS + wc + 37), (3, 100), (40, NS + wc), (70, NS + wc + 461), (1, 9), (160, NS + wc + 5), (33, 2)]


def _pack(name, Hkv, G, T_PAD, Wc):
    seqs = SEQS(Wc)
    lengths = [n for n, _ in seqs[:4]] + [2] + [n for n, _ in seqs[4:6]] + [0] + [seqs[6][0]]
    hist = [L for _, L in seqs[:4]] + [50] + [L for _, L in seqs[4:6]] + [20] + [seqs[6][1]]
    slots = [3, 0, 5, 2, -1, 7, 1, 6, 4]            # sequence 4 is inactive, sequence 7 is empty
    return dict(name=name, Hkv=Hkv, G=G, T_PAD=T_PAD, Wc=Wc, ns=NS, lengths=lengths, hist=hist, slots=slots, S=8,
                admit=[False] * len(lengths))


PACKS = {"walk": _pack("walk", 8, 8, 1024, 320), "capped": _pack("capped", 2, 8, 1024, 1024),
         "wide": _pack("wide", 2, 8, 320, 1024), "wide_g1": _pack("wide_g1", 2, 1, 320, 1024)}


def admission_case():
    """the walk geometry with a fresh slot admitted with 700 tokens in one call (22 chunk tiles) beside three continuing
    sequences and an inactive one"""
    c = PACKS["walk"]
    wc = c["Wc"]
    return variant(c, name="admission", lengths=[700, 1, 3, 40, 2], hist=[0, NS + wc + 37, 100, NS + wc, 50],
                   slots=[6, 3, 0, 5, -1], admit=[True, False, False, False, False])


def case_of(name):
    return admission_case() if name == "admission" else PACKS[name]


def variant(case, **kw):
    out = dict(case)
    out.update(kw)
    return out


def cu_of(lengths):
    cu = [0]
    for n in lengths:
        cu.append(cu[-1] + n)
    return cu


def live(case):
    """indices of the sequences that have work"""
    return [i for i, (n, s) in enumerate(zip(case["lengths"], case["slots"])) if n > 0 and s >= 0]


# ------------------------------------------------------------------------------------------------ the regime
def seq_plan(case, i):
    """state row, nsk and plan of sequence i as the kernels see them"""
    wc, ns, n = case["Wc"], case["ns"], case["lengths"][i]
    geom = ragged_geom(len(case["lengths"]), case["Hkv"] * case["G"], case["Hkv"], case["T_PAD"], ns + wc)
    st = case["states"][i] if "states" in case else state_after(case["hist"][i], ns, wc)
    nsk = 0
    if case["admit"][i]:
        st, nsk = [0, 0, 0, 0], min(n, ns)
    return st, nsk, multi_plan(st[0], st[1], n, geom["want"]), geom


def regime(case):
    """[dict] per (live sequence, row block): seq, rb, tmin, tmax, S, tps, last (tiles of the last split), per_wave
    (tiles assigned to a wave: min, max over the waves that get any), walks {(split, wave): [(tile, seg, class)] of the
    live tiles in order}, skipped {(split, wave): [tiles stepped over]}, edges {name: [(row t, tile, split, wave,
    iteration or None when the tile is dead for the block)] over the block's rows}; "wrap" is ring slot write_pos of a full
    ring, the oldest key, which follows the newest physically."""
    out = []
    G, wc = case["G"], case["Wc"]
    for i in live(case):
        n = case["lengths"][i]
        st, nsk, plan, geom = seq_plan(case, i)
        R = G * n
        for rb in range(cdiv(R, 32)):
            tmin, tmax = 32 * rb // G, min(32 * rb + 31, R - 1) // G
            walks, skipped, where = {}, {}, {}
            for split in range(plan["S"]):
                tbeg, tend = split * plan["tps"], min((split + 1) * plan["tps"], plan["T"])
                for wave in range(WAVES):
                    w, sk = [], []
                    for t in range(tbeg + wave, tend, WAVES):
                        ti = tile_info(st, wc, n, plan, t)
                        cls = tile_class(ti, wc, tmin, tmax, nsk)
                        if cls:
                            where[t] = (split, wave, len(w))
                            w.append((t, ti[0], cls))
                        else:
                            sk.append(t)
                            where[t] = (split, wave, None)
                    walks[(split, wave)], skipped[(split, wave)] = w, sk
            sl, wl, wp, _ = st
            edges = {}
            for t in range(tmin, tmax + 1):
                keys = {"diagonal": plan["T1"] + t // TILE}
                old = t - wc + 1
                if -wl <= old <= -1:
                    keys["oldest ring key"] = plan["T0"] + ring_slot(st, wc, old) // TILE
                if -wl <= old - 1 <= -1:
                    keys["key behind the window"] = plan["T0"] + ring_slot(st, wc, old - 1) // TILE
                if sl > 0:
                    keys["last sink key"] = (sl - 1) // TILE
                if wl == wc and wp > 0:
                    keys["wrap"] = plan["T0"] + wp // TILE
                for k, tile in keys.items():
                    edges.setdefault(k, []).append((t, tile) + where[tile])
            last = plan["T"] - (plan["S"] - 1) * plan["tps"]
            pw = [len(range(w, min(plan["tps"], plan["T"]), WAVES)) for w in range(WAVES)]
            out.append(dict(seq=i, rb=rb, tmin=tmin, tmax=tmax, n=n, state=st, nsk=nsk, plan=plan, S=plan["S"], tps=plan["tps"],
                            last=last, per_wave=(min(x for x in pw if x), max(pw)), walks=walks, skipped=skipped,
                            edges=edges, Sw=geom["Sw"], nrb=geom["nrb"],
                            want=geom["want"]))
    return out


def first_tile_masks_a_row(case, r):
    """(split, wave) of block r whose first live tile shows some row of the block no key while a later tile of the walk
    shows that row one: the row leaves its first tile with m = -inf"""
    G, wc, n = case["G"], case["Wc"], r["n"]
    hits = []
    for key, w in r["walks"].items():
        if len(w) < 2:
            continue
        sees = []
        for t, seg, _ in w:
            ti = tile_info(r["state"], wc, n, r["plan"], t)
            ks = tile_keys(r["state"], wc, ti)
            sees.append([any(visible(seg, c, row, wc, r["nsk"]) for c in ks) for row in range(r["tmin"], r["tmax"] + 1)])
        if any(not sees[0][x] and any(s[x] for s in sees[1:]) for x in range(len(sees[0]))):
            hits.append(key)
    return hits


# ------------------------------------------------------------------------------------------------ inputs
DT = P._DT


@functools.lru_cache(maxsize=None)
def pack_inputs(name, kind, dt, D, aux=True, seed=900):
    """One pack's tensors on the CPU: q [1, Hq, T_PAD, D], k / v [1, Hkv, T_PAD, D], s_aux (or None), hist {i: (k, v)
    [1, Hkv, L_i, D]} per live sequence, full {i: (q, k, v) over history + chunk}, probes {i: the chunk_probe dict}.
    kind: randn | probe | up | down | hill | offset | aux_sweep."""
    case = case_of(name)
    dtype = DT[dt]
    Hkv, G, T, wc = case["Hkv"], case["G"], case["T_PAD"], case["Wc"]
    Hq = Hkv * G
    g = torch.Generator().manual_seed(seed)
    q = RI._rand((1, Hq, T, D), g, dtype)
    k, v = RI._rand((1, Hkv, T, D), g, dtype), RI._rand((1, Hkv, T, D), g, dtype)
    sa = RI._rand((Hq,), g, torch.float32, 0.8) if aux else None
    if kind == "aux_sweep":
        sa = torch.tensor([RI.AUX_SWEEP[h % len(RI.AUX_SWEEP)] for h in range(Hq)], dtype=torch.float32)
    cu = cu_of(case["lengths"])
    hist, full, probes = {}, {}, {}
    order = live(case)
    for i in order:
        n, L = case["lengths"][i], case["hist"][i]
        if kind == "probe":
            pr = P.chunk_probe(1, Hq, Hkv, D, case["ns"], wc, L, n, dtype, seed=seed + 10 * i, aux=False)
            probes[i] = pr
            fq, fk, fv = pr["q"], pr["k"], pr["v"]
        elif kind in ("randn", "aux_sweep"):
            fk = torch.cat([RI._rand((1, Hkv, L, D), g, dtype), k[:, :, cu[i]:cu[i] + n]], dim=2)
            fv = torch.cat([RI._rand((1, Hkv, L, D), g, dtype), v[:, :, cu[i]:cu[i] + n]], dim=2)
            fq = torch.cat([torch.zeros(1, Hq, L, D, dtype=dtype), q[:, :, cu[i]:cu[i] + n]], dim=2)
        else:
            fq, fk, fv = _range_seq(kind, case, i, dtype, D, g)
        full[i] = (fq, fk, fv)
    if kind == "probe":
        # the pack edge (tests/test_ragged_step_host.py::probe_pack): in the last q head of every KV group the LAST row of
        # a sequence aims at the FIRST chunk key of the next live sequence, which it must not see
        for a, b in zip(order[:-1], order[1:]):
            La, na, Lb = case["hist"][a], case["lengths"][a], case["hist"][b]
            full[a][0][0, G - 1::G, La + na - 1] = (probes[a]["a"] * full[b][1][0, :, Lb].float()).to(dtype)
    for i in order:
        n, L = case["lengths"][i], case["hist"][i]
        fq, fk, fv = full[i]
        q[:, :, cu[i]:cu[i] + n], k[:, :, cu[i]:cu[i] + n], v[:, :, cu[i]:cu[i] + n] = fq[:, :, L:], fk[:, :, L:], fv[:, :, L:]
        hist[i] = (fk[:, :, :L], fv[:, :, :L])
    return dict(q=q, k=k, v=v, s_aux=sa, hist=hist, full=full, probes=probes, case=case, dtype=dtype)


def range_heights(kind, case, i):
    """H [L + n] in nat over the chronological positions of sequence i (history, then the chunk).  up / down: a level per
    64 keys of the chronological ring order, the steps at ring slots 0, 36 and 63 of every other tile (a tile edge, inside
    a tile, the last key of a tile), centred for `down`; hill: up to the middle of the ring's span, then down twice as fast (the tile
    with the ring's wrap inside holds the newest keys beside the oldest: the row's maximum in `up` and in `down`, its
    minimum here); offset: RI.OFFSET everywhere."""
    n, L, wc, ns = case["lengths"][i], case["hist"][i], case["Wc"], case["ns"]
    H = torch.zeros(L + n, dtype=torch.float64)
    if kind == "offset":
        return H + RI.OFFSET
    st = state_after(L, ns, wc)
    first = L - st[1]                       # position of the oldest ring key
    shift = st[2] % TILE if st[1] == wc else 0
    for t in range((L + n - first) // 64 + 2):
        x = first + 64 * t + (0, 36, 63)[t % 3] - shift
        if 0 < x < L + n:
            H[x:] += RI.STEPS[t % 3]
    if kind == "down":
        H = -H
        H = H - (H.max() + H.min()) / 2
    if kind == "hill":
        mid = (first + L + n) // 2
        H[mid:] = 3 * H[mid] - 2 * H[mid:]
    return H


def _range_seq(kind, case, i, dtype, D, g):
    """q / k / v over history + chunk of sequence i for a softmax-range family (the construction of range_inputs.dense_range:
    a common shift a_row H_key along one +-1 code per KV head)"""
    Hkv, G = case["Hkv"], case["G"]
    Hq, n, L = Hkv * G, case["lengths"][i], case["hist"][i]
    u = torch.randint(0, 2, (1, Hkv, 1, D), generator=g).double() * 2 - 1
    nq = torch.randn(1, Hq, n, D, generator=g, dtype=torch.float32).double()
    nk = torch.randn(1, Hkv, L + n, D, generator=g, dtype=torch.float32).double()
    fv = RI._rand((1, Hkv, L + n, D), g, dtype)
    H = range_heights(kind, case, i)
    t, h = torch.arange(n).view(1, n), torch.arange(Hq).view(Hq, 1)
    a = torch.tensor(RI.OFFSET_GAINS if kind == "offset" else RI.GAINS, dtype=torch.float64)[(t + h + 1) % 4]
    uq = u.repeat_interleave(G, dim=1)
    fq = RI._perp(nq, uq) + a.view(1, Hq, n, 1) * uq
    fk = RI._perp(nk, u) + (H / math.sqrt(D)).view(1, 1, L + n, 1) * u
    fq = torch.cat([torch.zeros(1, Hq, L, D, dtype=torch.float64), fq], dim=2)
    return fq.to(dtype), fk.to(dtype), fv


def oracle_rows(inp, i, sa="call"):
    """fp64 reference of sequence i: tests/util.py::chunk_oracle_rows over its whole history"""
    from util import chunk_oracle_rows
    case = inp["case"]
    fq, fk, fv = inp["full"][i]
    L = case["hist"][i]
    sa = inp["s_aux"] if isinstance(sa, str) else sa
    if case["admit"][i]:                    # an admitted sequence is a prefill of its own tokens
        from oracle import sink_oracle as O
        return O.sink_attention_dense(fq, fk, fv, case["ns"], case["Wc"], sa)[0]
    return chunk_oracle_rows(fq, fk, fv, sa, L, min(L, case["ns"]), case["Wc"],
                             case["lengths"][i], slice(0, 1))


# ------------------------------------------------------------------------------------------------ the kernel's walk, fp64
MODEL_MUTANTS = ("no_rescale", "m_safe", "reduce_inf_weight")


def kernel_model(inp, i, mutant=None, heads=None):
    """Sequence i in the kernel's order: per (KV head, row block, split, wave) the online softmax over the wave's live tiles
    (log2 domain, m_safe guard), the four-wave merge, the reduce over the S partials and s_aux.  Returns o [1, Hq, n, D]
    (fp64) and ev: a list of (kv head, rb, split, wave, iteration, min alpha over the block's rows that had a finite m) and
    the number of (wave, row) pairs that left their first tile with m = -inf and met a visible key later.
    Mutants: no_rescale (o and l keep their value after a wave's first tile), m_safe (the -inf guard dropped),
    reduce_inf_weight (a partial with m = -inf enters the reduce with weight 1)."""
    assert mutant is None or mutant in MODEL_MUTANTS
    case = inp["case"]
    G, wc, Hkv = case["G"], case["Wc"], case["Hkv"]
    n, L = case["lengths"][i], case["hist"][i]
    fq, fk, fv = (x.double() for x in inp["full"][i])
    D = fq.shape[3]
    c2 = LOG2E / math.sqrt(D)
    st, nsk, plan, _ = seq_plan(case, i)
    sa = inp["s_aux"]
    o = torch.zeros(1, Hkv * G, n, D, dtype=torch.float64)
    ev, started_inf = [], 0
    ninf = float("-inf")
    blocks = [r for r in regime(case) if r["seq"] == i]
    for hk in (range(Hkv) if heads is None else heads):
        for r in blocks:
            rows = torch.arange(32 * r["rb"], min(32 * r["rb"] + 32, G * n))
            tq, head = rows // G, hk * G + rows % G
            qb = fq[0, head, L + tq]                                            # [rows, D]
            parts = []
            for split in range(r["S"]):
                wm, wl_, wo = [], [], []
                for wave in range(WAVES):
                    m = torch.full((len(rows),), ninf, dtype=torch.float64)
                    l = torch.zeros(len(rows), dtype=torch.float64)
                    acc = torch.zeros(len(rows), D, dtype=torch.float64)
                    for it, (t, seg, cls) in enumerate(r["walks"][(split, wave)]):
                        ti = tile_info(st, wc, n, plan, t)
                        ks = tile_keys(st, wc, ti)
                        pos = torch.tensor([ti[1] + kk if seg == 0 else L + c for kk, c in enumerate(ks)])
                        cc = torch.tensor([0 if c is None else c for c in ks])
                        vis = torch.ones(len(rows), len(ks), dtype=torch.bool) if seg == 0 else \
                            (cc[None, :] <= tq[:, None]) & ((cc[None, :] >= tq[:, None] - wc + 1) | ((seg == 2) & (cc[None, :] < nsk)))
                        s = (qb @ fk[0, hk, pos].t() * c2).masked_fill(~vis, ninf)
                        m_new = torch.maximum(m, s.max(dim=1).values)
                        m_safe = m_new if mutant == "m_safe" else torch.where(m_new == ninf, torch.zeros_like(m_new), m_new)
                        alpha = torch.exp2(m - m_safe)
                        p = torch.exp2(s - m_safe[:, None])
                        if it >= 1:
                            fin = m > ninf
                            started_inf += int((~fin & (m_new > ninf)).sum())
                            if fin.any():
                                ev.append((hk, r["rb"], split, wave, it, float(alpha[fin].min())))
                        if mutant == "no_rescale" and it >= 1:
                            alpha = torch.where(torch.isnan(alpha), alpha, torch.ones_like(alpha))
                        l = l * alpha + p.sum(dim=1)
                        acc = acc * alpha[:, None] + p @ fv[0, hk, pos]
                        m = m_new
                    wm.append(m), wl_.append(l), wo.append(acc)
                wm, wl_, wo = torch.stack(wm), torch.stack(wl_), torch.stack(wo)
                ms = wm.max(dim=0).values
                wgt = torch.where(wm == ninf, torch.zeros_like(wm), torch.exp2(wm - ms))
                parts.append((ms, (wl_ * wgt).sum(0), (wo * wgt[:, :, None]).sum(0)))
            pm = torch.stack([x[0] for x in parts])
            sal = torch.full((len(rows),), ninf, dtype=torch.float64) if sa is None else sa.double()[head] * LOG2E
            mstar = torch.maximum(pm.max(dim=0).values, sal)
            w = torch.exp2(pm - mstar)
            if mutant == "reduce_inf_weight":
                w = torch.where(pm == ninf, torch.ones_like(w), w)
            else:
                w = torch.where(pm == ninf, torch.zeros_like(w), w)
            Lsum = (torch.stack([x[1] for x in parts]) * w).sum(0) + torch.exp2(sal - mstar)
            O = (torch.stack([x[2] for x in parts]) * w[:, :, None]).sum(0)
            o[0, head, tq] = O / Lsum[:, None]
    return o, ev, started_inf
