"""CPU: the short-window cases of tests/sliding_regime.py reach, at 256 CUs, the kernels and walks their rows claim (the GPU
tests of tests/test_gpu_sliding.py ask the same again for the device they run on); between them they cover every
hand-placed strip body, every trip count of the skewed sweep and both sides of every dispatch edge; strip_asm_nt and the
skew's T are what a brute-force count over oracle.valid_mask gives; every case's probe inputs hold enough rows of every
kind; and the probes tell the mutants a short-window kernel can have from the correct walk, fp64 oracle against mutated
fp64 oracle (no kernel involved), where randn inputs of the same shape do not.

The mutants (part 5), on one case per table (sliding_regime.PROOF_CASES; the first batch element and two KV heads of it):
  W+1, W-1        the window edge moved by a key, in the forward (O), in the dQ kernel alone, in the dK/dV kernel alone
  oldest_tile     an item drops the oldest tile of its walk (a ring that slid one tile too far)        forward, dQ
  tile_first/last the first / the last key of every 64-key tile is dropped                              forward, dQ
  stale           an item reads the oldest tile of its walk from the slot's previous lap: the keys and values of tile
                  t - R in place of tile t (R = NT + 1 slots of the hand-placed bodies, the ring of the compiled kernel)
                  forward
  slice_row       the first row of every 32-row slice is dropped from dK / dV                           dK/dV
  trips-1         one trip fewer: a wave's 64 keys lose the last 32-row slice they can see              dK/dV
A forward mutant is measured on O, a dQ mutant on dQ (tolerances of tests/test_gpu_mask_edges.py, the bf16 ones for both
dtypes: the looser), a dK/dV mutant on the larger of the dK and dV factors against the sum bound of
util.assert_within_sum_bound; each must reach FACTOR = 10, the criterion of tests/test_probe_inputs.py.  Smallest factors
measured (printed with -s): SMALLEST below, 14.3 at least.  randn inputs of the same shapes do see these unrestricted
mutants - at N of a few hundred a key is 1 / W of a row - but not with the margin: W - 1 in the dQ kernel alone moves
randn by 2.8 tolerances on edges_d80_bf16_w129, in the dK/dV kernel by 3.5 bounds, one trip fewer on the pack by 4.8.
W = 1 and W = 2: a row has one or two keys and s_aux holds the rest.  Without s_aux the one key holds p = 1, dS = p (1 - p) dP
is 0 and dQ, dK are identically 0, so these rows always carry s_aux; with the usual 0.5 randn s_aux p is still 1 to nine
digits.  sliding_regime.case_probe puts s_aux at the target's logit for them (p about 1/2) and scales dO by 4: a dropped key
moves dQ of the row by |dQ| itself, 20 |dQ| / (1 + |dQ|) tolerances, which passes 10 only where |dQ| > 1.  Measured smallest
factor over the six W = 1 cases and W = 2: 11.6 (dO x 1: 5.1 .. 9.0 on the dQ mutants; usual s_aux: 0.0).  No case is marked
path-only.
"""
import functools

import pytest
import torch

import probe_inputs as P
import sliding_regime as S
from grid_regime import regime as grid_regime, strip_asm_nt
from oracle import sink_oracle as O
from test_probe_inputs import (FACTOR, TOL_O, _check_musts, masked_attention, masked_attention_per_kernel,
                               per_kernel_factors)
from util import UNIT_ROUNDOFF

ALL = sorted(S.CASES)


# ------------------------------------------------------------------------------------------------ 1. claims
@pytest.mark.parametrize("cid", ALL)
def test_case_reaches_its_regime_at_256_cus(cid):
    r, missed = S.case_regime(cid, 256)
    assert not missed, missed
    c = S.CASES[cid]
    if c["Nq"] == c["Nk"] and c["D"] in (64, 80, 96):           # the dQ rule is grid_regime's where that one applies
        g = grid_regime(c["B"], c["Hq"], c["Hkv"], c["Nq"], c["D"], c["ns"], c["W"], 256, lens=c["lens"])
        assert r["dq"] == g["dq"].replace("compiled", "dq4w") and r["dq_side_stream"] == g["dq_side_stream"], (r["dq"], g["dq"])
        assert r["fwd"].split("_hpw")[0] in g["fwd"] or (g["fwd"] == "strip" and r["fwd"] in ("strip", "nw4")), (r["fwd"], g["fwd"])


# ------------------------------------------------------------------------------------------------ 2. coverage
def _rs():
    return {cid: S.case_regime(cid, 256)[0] for cid in ALL}


def test_the_tables_cover_every_body_trip_count_and_dispatch_edge():
    rs = _rs()
    C = S.CASES
    fwd = {(C[i]["D"], C[i]["dtype"], r["NT"]) for i, r in rs.items() if r["fwd"].startswith("stripasm")}
    assert fwd == {(D, dt, nt) for D in (64, 80, 96) for dt in S.DTYPES for nt in (2, 3, 4)}, "the 18 strip forward bodies"
    dq = {(C[i]["D"], C[i]["dtype"], r["NT"]) for i, r in rs.items() if r["dq"].startswith("dqstripasm")}
    assert dq == {(D, dt, nt) for D in (64, 80) for dt in S.DTYPES for nt in (2, 3, 4)}, "the 12 strip dQ bodies"
    # each forward body at the smallest and the largest window of its class, each class edge from both sides
    for D in (64, 80, 96):
        for dt in S.DTYPES:
            ws = {C[i]["W"] for i, r in rs.items() if r["fwd"].startswith("stripasm") and (C[i]["D"], C[i]["dtype"]) == (D, dt)}
            assert {1, 65, 66, 129, 130, 193} <= ws, (D, dt, ws)
        assert any(C[i]["W"] == 194 and C[i]["D"] == D and r["fwd"] in ("strip", "nw4") for i, r in rs.items()), D
    # strips: every item a cold start, one strip per sequence, a ragged last strip, a pack whose short sequences exit
    sa = [r for r in rs.values() if r["fwd"].startswith("stripasm")]
    assert any(r["L"] == 1 for r in sa) and any(r["n_strips"] == 1 and r["L"] > 1 for r in sa)
    assert any(1 < r["L"] and r["last_strip_items"] < r["L"] for r in sa) and any(r["exited_blocks"] > 0 for r in sa)
    assert {r["NT"] for r in sa if r["steady_items"] > 0} == {2, 3, 4} and any(not r["steady_w"] and r["L"] > 1 for r in sa)
    # the skewed sweep: every T from 6 to 18, both sides of the steps the issue names, and the window behind the last one
    sk = {r["T"] for r in rs.values() if r["skew"]}
    assert set(range(6, 19)) <= sk, sorted(set(range(6, 19)) - sk)
    w_t = {C[i]["W"]: r["T"] for i, r in rs.items() if r["skew"] and C[i]["Nq"] == S.N_SKEW and not C[i]["lens"]}
    for lo in (129, 161, 257, 481):
        assert w_t[lo + 1] == w_t[lo] + 1, (lo, w_t)
    assert any(C[i]["W"] == 512 and r["skew"] for i, r in rs.items()) and any(C[i]["W"] == 513 and not r["skew"] for i, r in rs.items())
    for D in (64, 80, 96):
        assert len({r["T"] for i, r in rs.items() if r["skew"] and C[i]["D"] == D and C[i]["Hq"] == 6}) >= 3, D
    assert any(r["skew"] and r["g"] == 1 for r in rs.values()) and any(r["skew"] and C[i]["W"] > C[i]["Nq"] for i, r in rs.items())
    # the compiled strip kernel
    ring = {i: r for i, r in rs.items() if r["fwd"] == "strip" and i in S.RING}
    assert {r["hpw"] for r in ring.values()} == {1, 2, 4, 8} and {r["TS"] for r in ring.values()} == {0, 1, 2, 3}
    assert any(r["hgroups"] == 2 for r in ring.values())
    assert {C[i]["ns"] for i in ring} >= {0, 1, 64, 65, 130} and {C[i]["W"] for i in ring} >= {1, 63, 64, 65, 194, 255, 256}
    assert {C[i]["D"] for i in S.RING} >= {32, 64, 80, 96}
    assert all(r["overwrites"] >= 2 and r["resident_ok"] for r in ring.values())
    assert any(r["shortest_strip"] < S.STRIP_MIN for r in ring.values()) and any(r["multi_load"] for r in ring.values())
    assert any(r["whole_sequence"] and C[i]["D"] == 32 and C[i]["B"] * C[i]["Hkv"] * r["hgroups"] >= 256 for i, r in ring.items())
    assert any(r["P"] > 0 for r in ring.values()) and any(r["shorter_than_bm"] for r in ring.values())
    assert any(r["sink_tile_holds_window_keys"] for r in ring.values())
    assert any(r["max_resident"] == r["R"] for r in ring.values()), "no q tile reads as many tiles as the ring has slots"
    # both sides of 256 | 257 and of the LDS cap (the same shape, one window key apart)
    assert any(C[i]["W"] == 256 and r["fwd"] == "strip" for i, r in rs.items())
    assert any(C[i]["W"] == 257 and C[i]["D"] == 64 and r["fwd"] == "asm4x64pk" for i, r in rs.items())
    a, b = (C[i] for i in S.LDS_CAP_PAIR)
    assert {k: v for k, v in a.items() if k not in ("id", "W", "claims")} == {k: v for k, v in b.items() if k not in ("id", "W", "claims")}
    assert b["W"] - a["W"] == 1 and rs[a["id"]]["fwd"] == "strip" and rs[b["id"]]["fwd"] == "nw4"
    assert rs[a["id"]]["lds"] == S.STRIP_LDS_CAP < rs[b["id"]]["lds"]


def test_regime_on_hand_worked_shapes():
    # the gpt-oss sliding layer (C4): one (batch, KV head) of 8192 rows at group 8: 256 items of two head sets, L = 1
    r = S.regime(1, 64, 8, 8192, 8192, 64, 0, 128, 256)
    assert (r["fwd"], r["L"], r["n_strips"], r["steady_w"], r["dq"], r["T"]) == ("stripasm_nt3", 8, 16, True, "dqstripasm_nt3", 6)
    # sink keys: the compiled strip kernel, 3 + 1 slots at BM = 32
    r = S.regime(1, 64, 8, 8192, 8192, 64, 4, 128, 256)
    assert (r["fwd"], r["hpw"], r["BM"], r["R"], r["TS"], r["skew"]) == ("strip", 8, 32, 4, 1, False)
    # a device with more CUs shortens the strips
    assert S.regime(16, 64, 16, 461, 461, 64, 0, 129, 304)["L"] == 6
    # the walk of one strip of two 64-row q tiles, W = 100, no sinks, ring of 4: tiles 0..1, then tile 2 prefetched
    w = S.strip_walk(128, 0, 100, 64, 4, 0, 4)
    assert w[0]["tiles"] == [(0, 1), (0, 2)] and w[0]["loads"] == [0, 1] and w[0]["overwrites"] == 0


# ------------------------------------------------------------------------------------------------ 3. brute force
def test_tile_and_trip_counts_against_the_oracle_mask():
    """strip_asm_nt(W): the 64-key tiles a 64-row tile can see (at least 2: the body has no one-tile form); the skew's T: the
    32-row slices the 64 keys of a wave can see (at least 6: the skew of four waves needs them).  Counted with valid_mask on
    a tile / a wave far from the start of the sequence, for every window from 1 to 600."""
    q0 = 1024
    rows, keys = torch.arange(q0, q0 + 64), torch.arange(0, q0 + 64)
    krows, kkeys = torch.arange(q0, q0 + 64 + 640), torch.arange(q0, q0 + 64)
    for W in range(1, 601):
        m = O.valid_mask(rows, keys, 0, W)
        tiles = int(m.view(64, -1, 64).any(2).any(0).sum())
        assert strip_asm_nt(W) == (max(tiles, 2) if W <= 193 else 0), (W, tiles)
        mk = O.valid_mask(krows, kkeys, 0, W)                    # [rows from the wave's first key on, the wave's 64 keys]
        slices = int(mk.view(-1, 32, 64).any(2).any(1).sum())
        assert slices == (62 + W) // 32 + 1 and S.skew_trips(W, 10 ** 6) == max(slices, S.SKEW_MIN_TRIPS), (W, slices)


# ------------------------------------------------------------------------------------------------ 4. probe kinds
@functools.lru_cache(maxsize=None)
def _probe(cid):
    return S.case_probe(S.CASES[cid])


@pytest.mark.parametrize("cid", ALL)
def test_every_case_covers_its_kinds(cid):
    c = S.CASES[cid]
    pr = _probe(cid)
    _check_musts(pr, pr["q"].shape[2], pr["k"].shape[2], c["ns"], c["W"], S.case_cu(c))
    counts = P.kind_counts(pr)
    missing = set(c["missing"]) | (set() if c["lens"] else {"prev_last", "pack_sink"})
    short = {k: n for k, n in counts.items() if k not in missing and n < P.MIN_ROWS}
    assert not short, (cid, short, counts)
    # a case may miss only what its shape excludes: the sink kinds at ns = 0, the window kinds when W >= N
    allowed = set()
    if c["ns"] == 0:
        allowed |= {"sink_last", "sink_next", "pack_sink"}
    if c["W"] >= max(c["lens"] or [c["Nq"]]):
        allowed |= {"win_oldest", "win_behind", "sink_last", "sink_next"}
    assert set(c["missing"]) <= allowed, (cid, c["missing"])
    if c["W"] < max(c["lens"] or [c["Nq"]]):
        assert counts["win_oldest"] >= P.MIN_ROWS or counts["win_behind"] >= P.MIN_ROWS, counts


# ------------------------------------------------------------------------------------------------ 5. the mutants
def _coords(c):
    """per row: position in its sequence (N_q < N_kv: the last rows) and row index in it; per key: position; same[i, j]"""
    Nq, Nk = (sum(c["lens"]),) * 2 if c["lens"] else (c["Nq"], c["Nk"])
    rs, ks = torch.zeros(Nq, dtype=torch.long), torch.zeros(Nk, dtype=torch.long)
    rl = torch.full((Nq,), Nq, dtype=torch.long)
    for a, b in zip(S.case_cu(c) or [0], (S.case_cu(c) or [0, 0])[1:]):
        rs[a:b], ks[a:b], rl[a:b] = a, a, b - a
    row = torch.arange(Nq) - rs
    return row, row + (Nk - Nq), torch.arange(Nk) - ks, rs.view(-1, 1) == ks.view(1, -1), rl


def _item_rows(c, r):
    """rows per item of the forward / dQ walk of the case: 64 for the hand-placed bodies, BM of the compiled strip kernel"""
    return r["BM"] if r["fwd"] == "strip" else 64


def _ring_slots(c, r):
    return r["R"] if r["fwd"] == "strip" else (r["NT"] + 1 if r["NT"] else 4)


def mutant_masks(c, r):
    """{name: (kernels it is a mutant of, mask)} and the true mask [Nq, Nk]"""
    ns, W = c["ns"], c["W"]
    row, p, kp, same, rl = _coords(c)
    i, j = p.view(-1, 1), kp.view(1, -1)
    win = lambda w: same & (j <= i) & ((j < ns) | (j >= i - w + 1))
    true = win(W)
    out = {"W+1": ("fwd", "dq", "dkdv", win(W + 1)), "W-1": ("fwd", "dq", "dkdv", win(W - 1))}
    BM = _item_rows(c, r)
    q0 = (row // BM * BM + (p - row)).view(-1, 1)                         # position of the item's first row
    t_old = (q0 - min(W, 10 ** 9) + 1).clamp(min=0) // 64
    out["oldest_tile"] = ("fwd", "dq", true & ~((j // 64 == t_old) & (j >= ns) & (t_old * 64 + 63 < q0)))
    out["tile_first"] = ("fwd", "dq", true & ~((j % 64 == 0) & (j >= ns)))
    out["tile_last"] = ("fwd", "dq", true & ~((j % 64 == 63) & (j >= ns)))
    out["slice_row"] = ("dkdv", true & ~(row.view(-1, 1) % 32 == 0))
    T = torch.tensor([S.skew_trips(W, int(n)) for n in rl]).view(-1, 1)
    out["trips-1"] = ("dkdv", true & ~(row.view(-1, 1) >= (j // 64) * 64 + 32 * (T - 1)))
    return true, {k: v for k, v in out.items() if bool((v[-1] != true).any())}


def _stale_factor(c, r, inp, true, o_true):
    """largest |O' - O| / tolerance when an item reads its oldest tile from the slot's previous lap"""
    row, p, kp, same, rl = _coords(c)
    BM, R, W = _item_rows(c, r), _ring_slots(c, r), c["W"]
    worst = 0.0
    for q0 in range(0, true.shape[0], BM):
        if c["lens"] and int(row[q0]) % BM:                          # (items are counted per sequence; the proof pack is walked whole)
            continue
        rows = torch.arange(q0, min(q0 + BM, true.shape[0]))
        rows = rows[row[rows] // BM == row[q0] // BM]
        first = int(p[q0]) - int(row[q0]) % BM
        t = max(first - W + 1, 0) // 64
        if t - R < 0 or t < -(-c["ns"] // 64):
            continue
        base = q0 - int(row[q0])                                     # first key of the sequence in the pack
        k2, v2 = inp["k"].clone(), inp["v"].clone()
        n = min(64, true.shape[1] - base - 64 * t)
        k2[:, :, base + 64 * t:base + 64 * t + n] = inp["k"][:, :, base + 64 * (t - R):base + 64 * (t - R) + n]
        v2[:, :, base + 64 * t:base + 64 * t + n] = inp["v"][:, :, base + 64 * (t - R):base + 64 * (t - R) + n]
        o2 = masked_attention(inp["q"], k2, v2, None, true[rows], inp["s_aux"], rows)[0]
        worst = max(worst, ((o2 - o_true[:, :, rows]).abs() / (TOL_O[0] + TOL_O[1] * o_true[:, :, rows].abs())).max().item())
    return worst


def _small(pr, c):
    """the first batch element and the first two KV heads of a probe (the mutants act on every head alike)"""
    g = c["Hq"] // c["Hkv"]
    hk = min(2, c["Hkv"])
    cut = lambda x, h: None if x is None else x[:1, :h]
    out = dict(pr, q=cut(pr["q"], g * hk), do=cut(pr["do"], g * hk), k=cut(pr["k"], hk), v=cut(pr["v"], hk))
    out["s_aux"] = None if pr["s_aux"] is None else pr["s_aux"][:g * hk]
    return out


def mutant_factors(c, inp):
    """{(mutant, kernel): factor} on the inputs inp"""
    r = S.case_regime(c["id"], 256)[0]
    true, muts = mutant_masks(c, r)
    u = UNIT_ROUNDOFF[inp["q"].dtype]
    f = masked_attention_per_kernel(inp["q"], inp["k"], inp["v"], inp["do"], true, true, true, inp["s_aux"])
    ref = dict(o=f[0], lse=f[1], dq=f[2], dk=f[3], dv=f[4], a_k=f[6], a_v=f[7])
    res = {}
    for name, spec in muts.items():
        kernels, mut = spec[:-1], spec[-1]
        fq, fk, fv = per_kernel_factors(inp, ref, true, mut, u)
        if "fwd" in kernels:
            rows = torch.nonzero((true != mut).any(1)).flatten()
            o2 = masked_attention(inp["q"], inp["k"], inp["v"], None, mut[rows], inp["s_aux"], rows)[0]
            res[name, "fwd"] = ((o2 - ref["o"][:, :, rows]).abs() / (TOL_O[0] + TOL_O[1] * ref["o"][:, :, rows].abs())).max().item()
        if "dq" in kernels:
            res[name, "dq"] = fq
        if "dkdv" in kernels:
            res[name, "dkdv"] = max(fk, fv)
    stale = _stale_factor(c, r, inp, true, ref["o"])
    if stale > 0:
        res["stale", "fwd"] = stale
    return res


# smallest factor per proof case over every (mutant, kernel), as printed by the test below
SMALLEST = {"edges_d80_bf16_w129": 14.3, "whole_d64_bf16_w65": 21.8, "ragged_d64_fp16_w130": 21.3, "pack_d64_bf16_w193": 23.6,
            "skew_d64_fp16_w162": 26.2, "ring_hpw4_g4_ns1_w63": 21.2}


@pytest.mark.parametrize("cid", S.PROOF_CASES)
def test_probes_catch_the_short_window_mutants_and_randn_hides_one(cid):
    c = S.CASES[cid]
    pr = _small(_probe(cid), c)
    got = mutant_factors(c, pr)
    blind = mutant_factors(c, P.randn_like_probe(pr, 77))
    for k in sorted(got):
        print(f"{cid} {k[0]}/{k[1]}: probe {got[k]:.1f} x, randn {blind[k]:.2f} x")
    print(f"{cid} smallest: {min(got.values()):.1f}")
    assert {k[0] for k in got} >= {"W+1", "W-1", "oldest_tile", "tile_first", "tile_last", "slice_row"}, sorted(got)
    bad = {k: v for k, v in got.items() if v < FACTOR}
    assert not bad, bad
    assert min(got.values()) >= 0.9 * SMALLEST[cid], "the docstring's figure is stale"
    assert min(blind.values()) < FACTOR, "randn inputs of the same shape reach the tenfold margin on every mutant too"


def test_the_proof_subset_runs_the_ring_and_trip_mutants():
    """`stale` needs an item whose oldest tile has a previous lap, `trips-1` a window whose last slice is not padding of the
    minimum of 6: both exist on the proof subset, on a hand-placed body, on the compiled ring and on the skew"""
    have = {cid: set(k[0] for k in mutant_factors(S.CASES[cid], _small(_probe(cid), S.CASES[cid]))) for cid in
            ("whole_d64_bf16_w65", "ring_hpw4_g4_ns1_w63", "skew_d64_fp16_w162")}
    assert "stale" in have["whole_d64_bf16_w65"] and "stale" in have["ring_hpw4_g4_ns1_w63"], have
    assert "trips-1" in have["skew_d64_fp16_w162"], have


@pytest.mark.parametrize("cid", [i for i in sorted(S.EDGES) if S.CASES[i]["W"] <= S.AUX_AT_LOGIT_MAX_W])
def test_tiny_windows_reach_the_margin(cid):
    """W = 1 (every head dim and dtype) and W = 2: every mutant that changes a pair reaches the margin, the dQ ones included"""
    c = S.CASES[cid]
    assert c["aux"] and not S.PATH_ONLY
    got = mutant_factors(c, _small(_probe(cid), c))
    print(cid, {k: round(v, 1) for k, v in got.items()})
    assert {k[1] for k in got} == {"fwd", "dq", "dkdv"}
    low = {k: v for k, v in got.items() if v < FACTOR}
    assert not low, low


def test_s_aux_is_not_tied_to_the_window():
    """each window of the edges table runs with and without s_aux (W = 1, 2: always with it), each class edge on both sides"""
    for W in (65, 66, 129, 130, 193):
        assert {c["aux"] for c in S.EDGES.values() if c["W"] == W} == {True, False}, W
    assert all(c["aux"] for c in S.EDGES.values() if c["W"] <= 2)
