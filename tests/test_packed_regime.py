"""CPU proofs for tests/test_gpu_packed_long.py (model and inputs: tests/packed_regime.py).

1. Regime: each pack reaches what its table line claims - waves that walk several tiles (walk, capped), the capped
   split count with a shorter last split (capped), many splits beside few and surplus launched splits (wide) - and the
   walks hold the transitions the tile loop of multi_split_mfma_kernel has never run in a packed call: sink -> ring,
   ring -> chunk (the FP8 -> 16-bit flip of st8), a dead tile stepped over between two live ones, full -> edge, a first
   tile that shows a row no key.
2. The gap: over every geometry of the existing packed GPU files and every fill a slot can have, tps <= 4 and S <= 2 -
   no wave of those tests runs the loop body twice.
3. Probes: on the probe inputs at the long Wc every one-key mask mutant moves some row by ten tolerances, and the edge
   keys lie in a later iteration of a wave and in a later split.
4. Range: the fp64 model of the kernel's order of operations equals the oracle; every wave that walks two live tiles
   rescales by alpha < 2^-8 in the rising staircase, the falling one or the hill; some row leaves its first tile at m = -inf; the
   mutants of the model miss the tolerance tenfold."""
import pytest
import torch

import packed_regime as R
from test_gpu_decode_multi import TOL
from test_probe_inputs import MUTANTS, edge_mask, factors, masked_attention

MULTI = ("walk", "capped")


def _long(case, r):
    return case["hist"][r["seq"]] >= case["ns"] + case["Wc"]


def _steps(rg):
    """every (earlier, later) pair of consecutive live tiles over the walks of a regime"""
    for r in rg:
        for w in r["walks"].values():
            for a, b in zip(w[:-1], w[1:]):
                yield r, a, b


# ------------------------------------------------------------------------------------------------ 1. regime proofs
@pytest.mark.parametrize("name", ["walk", "capped", "wide", "wide_g1"])
def test_the_pack_reaches_what_its_table_line_claims(name):
    case = R.PACKS[name]
    rg = R.regime(case)
    assert len(R.live(case)) == 7 and sum(case["lengths"][i] for i in R.live(case)) == 308
    assert case["Wc"] <= 1024 and case["T_PAD"] <= 1024 and case["ns"] == 4
    pool_bytes = case["S"] * case["Hkv"] * (case["ns"] + case["Wc"]) * 128 * 4 * 2      # K and V, fp32 at D = 128 at most
    assert pool_bytes < 64 << 20
    long_ = [r for r in rg if _long(case, r)]
    short = [r for r in rg if not _long(case, r)]
    assert {r["seq"] for r in long_} == {0, 2, 3, 6} and {r["seq"] for r in short} == {1, 5, 8}
    if name == "walk":
        assert rg[0]["want"] == 1 and rg[0]["Sw"] == 1 and all(r["S"] == 1 for r in rg)
        assert {r["tps"] for r in long_} <= set(range(12, 17)) and {12, 16} <= {r["tps"] for r in long_}
        assert all(r["per_wave"][0] >= 3 and r["per_wave"][1] <= 4 for r in long_)
    elif name == "capped":
        assert rg[0]["want"] == 4 and rg[0]["Sw"] == 4
        assert all(r["S"] == 4 and r["tps"] in (9, 10) and 7 <= r["last"] <= 9 for r in long_)
        assert any(r["last"] < r["tps"] for r in long_)
        assert all(r["per_wave"] == (2, 3) for r in long_)
        # the planned count ceil((ceil(Nkv / 32) + 2) / 4) would be 9 or 10: the cap binds
        assert all(R.cdiv(R.cdiv(sum(r["state"][:2]) + r["n"], 32) + 2, 4) > 4 for r in long_)
    else:
        assert rg[0]["want"] == (12 if name == "wide" else 54) and rg[0]["Sw"] == 12
        assert {r["S"] for r in long_} == {9, 10} and {r["S"] for r in short} == {1, 2}
        assert all(r["S"] < r["Sw"] for r in rg)                 # surplus workgroups exit in every sequence
        assert all(r["tps"] <= 4 and r["per_wave"] == (1, 1) for r in rg)
        assert any(r["last"] < r["tps"] for r in long_)
        # S = ceil(T / tps) below the planned s: T = 34 plans s = 9 at tps = 4 and 9 splits; T = 38 plans 10
        ring_only = [k for r in long_ for k in range(r["S"])
                     if all(seg == 1 for w in range(4) for _, seg, _ in r["walks"][(k, w)]) and
                     sum(len(r["walks"][(k, w)]) + len(r["skipped"][(k, w)]) for w in range(4)) == 4]
        assert ring_only, "no split wholly inside the ring"
        wrap = {r["seq"]: r["edges"]["wrap"][0][2] for r in long_ if "wrap" in r["edges"]}
        assert wrap and max(wrap.values()) > 0, wrap


@pytest.mark.parametrize("name", MULTI)
def test_the_walks_hold_the_transitions_the_tile_loop_has_never_run(name):
    case = R.PACKS[name]
    rg = R.regime(case)
    steps = list(_steps(rg))
    seg_steps = {(R.SEG[a[1]], R.SEG[b[1]]) for _, a, b in steps}
    assert ("sink", "ring") in seg_steps and ("ring", "chunk") in seg_steps, seg_steps
    assert any(b[0] - a[0] > R.WAVES for _, a, b in steps), "no dead tile between two live ones"
    assert any(a[2] == 1 and b[2] == 2 for _, a, b in steps), "no full -> edge step"
    assert any(a[2] == 2 and b[2] == 1 for _, a, b in steps), "no edge -> full step"
    masked = [(r["seq"], r["rb"], k) for r in rg for k in R.first_tile_masks_a_row(case, r)]
    print(name, "walks whose first tile shows a row no key:", masked)
    assert masked
    # a wave that crosses the ring's wrap: chronologically newer keys first, older ones after
    assert any(a[1] == b[1] == 1 and R.tile_info(r["state"], case["Wc"], r["n"], r["plan"], a[0])[4] >
               R.tile_info(r["state"], case["Wc"], r["n"], r["plan"], b[0])[4] for r, a, b in steps)


def test_an_admission_at_depth_walks_dead_chunk_tiles():
    """a fresh slot admitted with 700 tokens in the walk geometry: 22 chunk tiles in one split, the first holds the
    sinks; the late row blocks step over the chunk tiles behind their window"""
    case = R.admission_case()
    rg = [r for r in R.regime(case) if r["seq"] == 0]
    assert rg[0]["plan"]["T"] == 22 and rg[0]["S"] == 1 and rg[0]["nsk"] == 4 and rg[0]["state"] == [0, 0, 0, 0]
    late = rg[-1]
    w0 = late["walks"][(0, 0)]
    assert w0[0][0] == 0 and w0[1][0] - w0[0][0] > R.WAVES, w0       # tile 0 (the sinks), then a jump over dead tiles
    assert any(len(r["walks"][(0, w)]) >= 3 for r in rg for w in range(4))


# ------------------------------------------------------------------------------------------------ 2. the gap, recorded
def _existing_geometries():
    """(file, H_kv, G, T_PAD, n_seq, num_sink, Wc, lengths) of every packed call of the existing GPU files"""
    import test_gpu_ragged_admit as A
    import test_gpu_ragged_step as ST
    import test_gpu_ragged_tree as TR
    out = []
    for W in (16, 48):
        for G in (1, 8):
            out.append(("ragged_step", ST.HKV, G, ST.T_PAD, len(ST.LENGTHS), ST.NS, W, ST.LENGTHS))
            out.append(("ragged_step zeros", ST.HKV, G, 64, 5, ST.NS, W, [5, 0, 33, 4, 1]))
            out.append(("ragged_step capture", ST.HKV, G, 96, 5, ST.NS, W, [1, 40, 3, 8, 70, 92]))
            for ns in (4, 40):
                for T, seqs in A.PACKS.values():
                    out.append(("ragged_admit", A.HKV, G, T, len(seqs), ns, W, [n for n, _, _ in seqs]))
            # tests/test_gpu_fp8_pool.py imports this geometry; its captured step runs T = 112 over 6 sequences
            out.append(("ragged_tree / fp8_pool", TR.HKV, G, TR.T_PAD, len(TR.LENGTHS), TR.NS, W, TR.LENGTHS))
            out.append(("fp8_pool capture", TR.HKV, G, 112, 6, TR.NS, W, list(range(1, 113))))
    # tests/test_gpu_far_offsets.py::test_pool_and_rows_calls_far (its numbers are local to the test): Wc = 64
    for G, Hkv in ((8, 1), (1, 2), (2, 2)):
        out.append(("far_offsets", Hkv, G, 46, 4, 4, 64, [1, 3, 40, 2]))
    return out


def test_no_existing_packed_test_gives_a_wave_a_second_tile():
    """THE GAP: this is why tests/test_gpu_packed_long.py exists.  Over every fill a slot can have (sink_len <= num_sink,
    window_len <= Wc; an admitting sequence is the empty fill) no sequence of the existing packed GPU tests plans more
    than 4 tiles per split - one tile per wave, the loop body of multi_split_mfma_kernel runs once - or more than 2
    splits."""
    worst_tps, worst_S = 0, 0
    for what, Hkv, G, T, n_seq, ns, W, lengths in _existing_geometries():
        geom = R.ragged_geom(n_seq, Hkv * G, Hkv, T, ns + W)
        for n in set(lengths) - {0}:
            for sl in range(ns + 1):
                for wl in range(W + 1):
                    p = R.multi_plan(sl, wl, n, geom["want"])
                    worst_tps, worst_S = max(worst_tps, p["tps"]), max(worst_S, p["S"])
                    assert p["tps"] <= 4 and p["S"] <= 2, (what, G, T, ns, W, n, sl, wl, p)
    print("existing packed tests: max tiles per split", worst_tps, "max splits", worst_S)
    assert (worst_tps, worst_S) == (4, 2)


# ------------------------------------------------------------------------------------------------ 3. probes
PROBE_TYPES = [("bf16", 64), ("fp16", 128), ("bf16", 80), ("fp16", 96)]
EDGE_KEYS = ("diagonal", "oldest ring key", "key behind the window", "wrap")


def _probe_masks(case, i, nxt):
    """the true mask [n, L + n + 1] of sequence i over (history, chunk, the first chunk key of the next live sequence)
    and its one-key mutants: the six of tests/test_probe_inputs.py::MUTANTS and the pack neighbour's first key"""
    n, L, W = case["lengths"][i], case["hist"][i], case["Wc"]
    sl = min(L, case["ns"])
    pos, j = torch.arange(n) + L, torch.arange(L + n + 1)
    own = (j <= L + n - 1).view(1, -1)
    true = edge_mask(pos, j, sl, W) & own
    muts = {}
    for what, kw in MUTANTS.items():
        if what.startswith("ns") and sl + kw["dns"] < 0:
            continue
        m = edge_mask(pos, j, sl, W, **kw) & own
        if not torch.equal(m, true):
            muts[what] = m
    if nxt:
        m = true.clone()
        m[n - 1, L + n] = True
        muts["neighbour's first key"] = m
    return true, muts


@pytest.mark.parametrize("name", MULTI)
@pytest.mark.parametrize("dt,D", PROBE_TYPES)
def test_a_one_key_mask_error_moves_a_probe_row_tenfold(dt, D, name):
    """Oracle against mutated oracle on the inputs of test_gpu_packed_long.py::test_mask_edge_probes.  The amplitude is
    probe_inputs.amplitude(D) = 2.0, unchanged: the smallest factor over (pack, type, mutant) is 178 tolerances (every
    figure is printed)."""
    inp = R.pack_inputs(name, "probe", dt, D)
    case = inp["case"]
    tol = (TOL[inp["dtype"]], 0.0)
    order = R.live(case)
    best = {}
    for x, i in enumerate(order):
        n, L = case["lengths"][i], case["hist"][i]
        fq, fk, fv = inp["full"][i]
        nxt = order[x + 1] if x + 1 < len(order) else None
        zk = torch.zeros_like(fk[:, :, :1])
        nk, nv = (inp["full"][nxt][1][:, :, case["hist"][nxt]:case["hist"][nxt] + 1],
                  inp["full"][nxt][2][:, :, case["hist"][nxt]:case["hist"][nxt] + 1]) if nxt is not None else (zk, zk)
        d = dict(q=fq[:, :, L:], k=torch.cat([fk, nk], dim=2), v=torch.cat([fv, nv], dim=2), s_aux=inp["s_aux"])
        true, muts = _probe_masks(case, i, nxt is not None)
        o_true = masked_attention(d["q"], d["k"], d["v"], None, true, inp["s_aux"])[0]
        assert (o_true - R.oracle_rows(inp, i)).abs().max().item() < 1e-9      # the masked form IS the GPU test's oracle
        for what, mut in muts.items():
            hit = torch.nonzero((true != mut).any(1)).flatten()
            fo = factors(d, true, mut, hit, tol_o=tol)[0]
            best[what] = max(best.get(what, 0.0), fo)
    print(name, dt, D, {k: round(v, 1) for k, v in best.items()})
    assert set(best) == set(MUTANTS) | {"neighbour's first key"}, set(best)
    for what, fo in best.items():
        assert fo >= 10, (what, fo)


def test_the_edge_keys_lie_in_a_later_iteration_and_in_a_later_split():
    """regime() of the probe packs: the diagonal, the oldest visible ring key, the key behind it and the wrap point are
    met in iteration >= 1 of a wave's walk (both packs) and in a split > 0 (capped).  The last sink key cannot be: with
    num_sink = 4 it lies in tile 0, the first tile of wave 0 of split 0, in every plan."""
    for name in MULTI:
        rg = R.regime(R.PACKS[name])
        for key in EDGE_KEYS:
            hits = [e for r in rg for e in r["edges"].get(key, [])]
            assert any(e[4] is not None and e[4] >= 1 for e in hits), (name, key, "never in a later iteration")
            if name == "capped":
                assert any(e[2] > 0 and e[4] is not None for e in hits), (name, key, "never in a later split")
        sink = [e for r in rg for e in r["edges"].get("last sink key", [])]
        assert sink and all(e[1:] == (0, 0, 0, 0) for e in sink)


# ------------------------------------------------------------------------------------------------ 4. range
RANGE_TYPE = ("bf16", 64)
FAMILIES = ("up", "down", "hill", "offset", "aux_sweep")


def _model_error(inp, i, mutant=None):
    o, ev, inf0 = R.kernel_model(inp, i, mutant, heads=[0])
    G = inp["case"]["G"]
    err = (o[:, :G] - R.oracle_rows(inp, i)[:, :G]).abs()
    return torch.nan_to_num(err, nan=float("inf")).max().item(), ev, inf0, o


@pytest.mark.parametrize("name", MULTI)
def test_the_staircases_step_on_tile_edges_and_inside_tiles(name):
    case = R.PACKS[name]
    i = 6                                                    # the 160-token chunk on a wrapped ring
    H = R.range_heights("up", case, i)
    L, st = case["hist"][i], R.state_after(case["hist"][i], case["ns"], case["Wc"])
    steps = torch.nonzero(H[1:] != H[:-1]).flatten() + 1
    slots = {R.ring_slot(st, case["Wc"], int(x) - L) % R.TILE for x in steps if -st[1] <= int(x) - L <= -1}
    assert {0, 31} <= slots and slots - {0, 31}, slots
    assert len(steps) >= (st[1] + case["lengths"][i]) // 64
    D = R.range_heights("down", case, i)
    assert D[0] > D[-1] and abs(float(D.max() + D.min())) < 1e-9
    assert float(R.range_heights("offset", case, i).min()) == 60.0


@pytest.mark.parametrize("name", MULTI)
def test_the_kernel_model_rescales_in_every_walk_and_its_mutants_fail(name):
    dt, D = RANGE_TYPE
    case = R.PACKS[name]
    tol = TOL[R.DT[dt]]
    rescaled, walks2, inf_starts = set(), set(), 0
    worst = {m: 0.0 for m in R.MODEL_MUTANTS}
    for fam in FAMILIES:
        inp = R.pack_inputs(name, fam, dt, D)
        if fam == "aux_sweep":
            assert inp["s_aux"].min().item() == -40.0 and inp["s_aux"].max().item() == 40.0
        for i in R.live(case):
            err, ev, inf0, o_model = _model_error(inp, i)
            assert err <= tol / 2, (fam, i, err)                 # the correct model: the oracle, to rounding
            inf_starts += inf0
            for hk, rb, split, wave, it, alpha in ev:
                walks2.add((i, rb, split, wave))
                if alpha < 2.0 ** -8 and fam in ("up", "down", "hill"):
                    rescaled.add((i, rb, split, wave))
            if fam == "up" or (fam == "down" and case["lengths"][i] in (1, 70)):
                for m in R.MODEL_MUTANTS:
                    e, _, _, o_mut = _model_error(inp, i, m)
                    if m == "reduce_inf_weight":                 # against the correct model: bitwise the same
                        e = torch.nan_to_num((o_mut - o_model).abs(), nan=float("inf")).max().item()
                    worst[m] = max(worst[m], e)
    # every wave that walks at least two live tiles (in which some row has seen a key before the second)
    model = {(r["seq"], r["rb"], k[0], k[1]) for r in R.regime(case) for k, w in r["walks"].items() if len(w) >= 2}
    assert walks2 <= model and len(walks2) > 100
    print(name, "waves with two live tiles", len(walks2), "of them rescaling by alpha < 2^-8:", len(rescaled),
          "rows starting at m = -inf:", inf_starts, "mutant errors / tol:", {m: e / tol for m, e in worst.items()})
    assert rescaled == walks2, sorted(walks2 - rescaled)[:8]
    assert inf_starts > 0
    assert worst["no_rescale"] >= 10 * tol and worst["m_safe"] >= 10 * tol, worst
    # A partial with m = -inf carries l = 0 and O = 0 exactly (every p of it is exp2(-inf - 0), and the wave merge gives a
    # wave with m = -inf the weight 0), so any finite weight in the reduce leaves the sum unchanged: this mutant is
    # equivalent on every input.  What the kernel's `ms != -inf` test guards against is exp2(-inf - mstar) on a partial
    # that was never WRITTEN (split >= S), which tests/test_gpu_packed_long.py::test_the_plan_read_back pins with a
    # poisoned workspace.
    assert worst["reduce_inf_weight"] == 0.0
