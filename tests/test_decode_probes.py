"""CPU proofs for the single-token decode edge tests (tests/test_gpu_decode_edges.py): no GPU.

  1. tests/decode_regime.py restates decode_plan and the workspace layout: pinned against sfa_decode_workspace_bytes
     over a sweep of shapes (max_splits and the counter region), and every case reaches the regime it is listed for.
  2. The decode probes of tests/probe_inputs.py tell a kernel that is wrong by one key, by one split, by one fold round
     or by one head from a correct one: for every launch of every case, the fp64 oracle against a MUTATED oracle moves
     the output by at least ten DECODE_TOL, while the unmutated oracle rounded to the dtype stays within half of it.
  3. randn does not: at the shape and seed of tests/test_gpu_decode.py::test_long_kv, dropping a whole split of 256 keys
     or miscounting one key stays inside that test's tolerance.  That is why this family exists.
Every launch is enumerated by probe_inputs.decode_runs, the function the GPU file walks."""
import math

import pytest
import torch

import decode_regime as R
import probe_inputs as P
from oracle import sink_oracle as O
from util import DECODE_TOL, rand

FACTOR = 10.0
CASES = R.MANY + R.GROUPS + R.FILLS
# mutant -> the kind whose probes catch it (None: several)
MUTANTS = {"drop_newest": "newest", "see_evicted": "evicted", "drop_ring_oldest": "ring_oldest",
           "see_beyond_fill": "beyond_fill", "see_beyond_sink": "beyond_sink", "drop_split_first": "split_first",
           "drop_split_last": "split_last", "double_last_key": "last_key", "drop_split_0": "sink_last",
           "drop_split_tail": "last_key", "drop_split_ge64": None, "drop_split_32_63": None, "fold_w64": None,
           "fold_w32": None, "swap_heads": None}


# ------------------------------------------------------------------------------------------------ 1. the plan
def test_plan_matches_the_workspace_query_over_a_sweep():
    from sink_attention import _native
    lib = _native.lib()
    n = 0
    for dt, Ds in ((torch.bfloat16, (16, 64, 80, 128, 256, 512)), (torch.float16, (8, 48, 96, 128)),
                   (torch.float32, (4, 32, 64, 80, 256))):
        for D in Ds:
            for B, Hq, Hkv in ((1, 8, 1), (2, 4, 1), (1, 12, 2), (10, 16, 2), (11, 2, 2), (8, 32, 8), (32, 32, 32), (3, 3, 1)):
                for Nkv in (1, 3, 255, 256, 257, 504, 1024, 1025, 2404, 4100, 6657, 16384, 16385, 131072):
                    got = lib.sfa_decode_workspace_bytes(B, Hq, Hkv, Nkv, D, R.SFA_DTYPE[dt])
                    assert got == R.workspace_bytes(B, Hq, Hkv, Nkv, D, dt), (dt, D, B, Hq, Hkv, Nkv)
                    pl = R.plan(B, Hq, Hkv, Nkv, D, dt)
                    assert 1 <= pl["splits"] <= pl["max_splits"] and pl["kps"] % pl["iter_keys"] == 0
                    assert (pl["splits"] - 1) * pl["kps"] < max(Nkv, 1) <= pl["splits"] * pl["kps"]
                    lay = R.layout(B, Hq, Hkv, pl["splits"], D)
                    assert lay["cnt"][1] == R.counter_bytes(B, Hkv) >= (B * Hkv + 1) * 4 and lay["end"] <= got
                    n += 1
    assert n > 1000


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["id"])
def test_case_reaches_its_regime(case):
    runs = P.decode_runs(case)
    seen_fresh, seen_empty = set(), set()
    for name, run, steps in runs:
        for step in range(steps):
            L = run.probe()
            pl, rows = L["pl"], L["rows"]
            for k, v in case["reach"].items():
                assert pl[k] == v, (case["id"], name, k, pl[k], v)
            for b, r in enumerate(rows):
                if not L["active"][b]:
                    continue
                if r["fresh_split"] > 0:
                    seen_fresh.add((name, b, step))
                if r["empty"]:
                    seen_empty.add((name, b, step))
            run.apply(L["pr"])
        print(case["id"], name, R.describe(pl, rows))
    pl, rows = R.regime(case, [case["states"][0]] * case["B"], device_state=case in R.FILLS)
    if case in R.MANY:
        assert rows[0]["n_keys"][-1] == 1 and pl["splits"] > R.REDUCE_W and pl["o_rounds"] == 9
        assert {n for n, _, _ in seen_fresh} >= {"step1", "step2", "dyn"}            # splits 40, 64 and 40
    if case in R.GROUPS:
        r = rows[0]
        assert 2 <= pl["splits"] <= 5 and r["cls"][-1] == "partial" and r["Nkv"] % pl["kps"] and r["Nkv"] % pl["iter_keys"]
        assert r["clamped"][-1] > 0 and seen_fresh
    if case in R.FILLS:
        assert pl["splits"] >= 4
        assert len({b for n, b, _ in seen_fresh if n == "rows"}) >= 2 and len({b for n, b, _ in seen_empty if n == "rows"}) >= 2
        # a row whose key count ends exactly on a split edge, and its two neighbours
        assert {R.regime(case, case["states"], device_state=True)[1][b]["Nkv"] for b in (2, 3, 4)} == \
            {pl["kps"] - 1, pl["kps"], pl["kps"] + 1}


# ------------------------------------------------------------------------------------------------ 2. mutants
def _weighted(s, Vq, sa, mult, numer=None):
    """softmax over logits s [Hq, n] + log(mult) with the s_aux column in the denominator; numer: a 0 / 1 factor on the
    numerator alone (a fold that loses a split's O row but not its statistics)"""
    sm = s + torch.log(mult).view(1, -1)
    lse = torch.logsumexp(torch.cat([sa.view(-1, 1), sm], 1), 1, keepdim=True)
    p = torch.exp(sm - lse)
    if numer is not None:
        p = p * numer.view(1, -1)
    return torch.einsum("hn,hnd->hd", p, Vq)


def _row_mutants(state, Wc, row, n, extras, S, kps):
    """{mutant: (mult, numer)} of one batch row; keys [0, n) are the kept ones, then the extras in `extras` order"""
    sl, wl, wp = state
    N1, Nkv = row["N1"], row["Nkv"]
    base = torch.cat([torch.ones(n, dtype=torch.float64), torch.zeros(len(extras), dtype=torch.float64)])
    out = {}

    def edit(name, idx, val, numer=False):
        m = base.clone() if not numer else torch.ones_like(base)
        m[idx] = val
        out[name] = (base, m) if numer else (m, None)

    out["none"] = (base, None)
    edit("drop_newest", N1 + wp, 0.0)
    for i, k in enumerate(extras):
        edit("see_" + k, n + i, 1.0)
    if wl == Wc and Wc >= 2:
        edit("drop_ring_oldest", N1 + (wp + 1) % Wc, 0.0)
    live = [s for s in range(S) if row["n_keys"][s] > 0]
    if len(live) >= 2:
        edit("drop_split_first", [row["k_beg"][s] for s in live[1:]], 0.0)
        edit("drop_split_last", [row["k_beg"][s] + row["n_keys"][s] - 1 for s in live[1:]], 0.0)
        edit("drop_split_tail", slice(row["k_beg"][live[-1]], Nkv), 0.0)
    edit("double_last_key", Nkv - 1, 2.0)
    edit("drop_split_0", slice(0, min(kps, Nkv)), 0.0)
    if len(live) > 64:
        edit("drop_split_ge64", slice(64 * kps, Nkv), 0.0)
        edit("fold_w64", slice(64 * kps, Nkv), 0.0, numer=True)
    if len(live) > 40:
        edit("drop_split_32_63", slice(40 * kps, 41 * kps), 0.0)
        edit("fold_w32", slice(32 * kps, Nkv), 0.0, numer=True)
    return out


def launch_ratios(run, L):
    """{mutant: max |mutated oracle - oracle| / DECODE_TOL} over the active rows of one launch, and the largest
    |round(oracle) - oracle| / DECODE_TOL"""
    pr, ref = L["pr"], L["ref"]
    dt = pr["q"].dtype
    tol = DECODE_TOL[dt]
    Hq, D = pr["q"].shape[1], pr["q"].shape[3]
    Wc = run.cache["window_k"].shape[2]
    g = Hq // run.cache["sink_k"].shape[1]
    worst = {}
    for b, st in enumerate(L["states"]):
        if not L["active"][b]:
            continue
        K, V, ex = P.decode_kept(run.cache, st, b, pr["k_new"], pr["v_new"])
        n = K.shape[1]
        names = list(ex)
        Ka = torch.cat([K] + [ex[k][0] for k in names], 1).double().repeat_interleave(g, 0)
        Va = torch.cat([V] + [ex[k][1] for k in names], 1).double().repeat_interleave(g, 0)
        s = torch.einsum("hd,hnd->hn", pr["q"][b, :, 0].double(), Ka) / math.sqrt(D)
        sa = pr["s_aux"].double()
        muts = _row_mutants(st, Wc, L["rows"][b], n, names, L["pl"]["splits"], L["pl"]["kps"])
        o0 = _weighted(s, Va, sa, muts.pop("none")[0])
        assert (o0 - ref[b, :, 0]).abs().max() < 1e-9            # the weighted form IS the oracle when nothing is mutated
        for name, (mult, numer) in muts.items():
            d = (_weighted(s, Va, sa, mult, numer) - o0).abs().max().item() / tol
            worst[name] = max(worst.get(name, 0.0), d)
        if g >= 2:
            sw = o0.view(-1, g, D).roll(1, 1).reshape(-1, D)        # every head takes its neighbour's row
            worst["swap_heads"] = max(worst.get("swap_heads", 0.0), (sw - o0).abs().max().item() / tol)
    rounding = (ref.to(dt).double() - ref).abs().max().item() / tol
    return worst, rounding


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["id"])
def test_every_mutant_misses_the_tolerance_tenfold(case):
    """per LAUNCH, not only per case: a GPU test of one launch catches a mutant only if that launch's probe does"""
    low = {}
    kinds = {}
    for name, run, steps in P.decode_runs(case):
        for step in range(steps):
            L = run.probe()
            worst, rounding = launch_ratios(run, L)
            assert rounding <= 0.5, (case["id"], name, step, rounding)
            have = {P.DECODE_KINDS[int(k)] for b in range(len(L["states"])) if L["active"][b] for k in L["pr"]["kind"][b]}
            for m, r in worst.items():
                # a mutant that one kind catches is judged in the launches that aim at that kind; the others in all
                if MUTANTS[m] is None or MUTANTS[m] in have:
                    assert r >= FACTOR, (case["id"], name, step, m, r)
                    low[m] = min(low.get(m, float("inf")), r)
            Hkv = run.cache["sink_k"].shape[1]
            g = L["pr"]["q"].shape[1] // Hkv
            for b in range(len(L["states"])):
                if L["active"][b]:
                    for h in range(L["pr"]["q"].shape[1]):
                        kinds.setdefault(P.DECODE_KINDS[int(L["pr"]["kind"][b, h])], []).append((name, step, b, h // g))
                    # the heads of a group do not all aim at one key (how far they differ is what swap_heads measures)
                    for hk in range(Hkv):
                        locs = L["pr"]["loc"][b][hk * g:(hk + 1) * g]
                        cand = P.decode_kinds(L["states"][b], case["ns"], case["Wc"], L["rows"][b])
                        n_keys = len({v[0] for v in cand.values() if v})       # (kinds may share a key: a one-key split)
                        assert len(set(locs)) >= min(g, n_keys, 2), (case["id"], name, b, hk, locs)
            run.apply(L["pr"])
    print(case["id"], "smallest factor per mutant:", {m: round(r, 1) for m, r in sorted(low.items())})
    # every mutant the case's regime has was judged, and every kind is aimed at by two (batch, head) pairs on two KV heads
    want = {"drop_newest", "double_last_key", "drop_split_0", "drop_split_first", "drop_split_last", "drop_split_tail"}
    if case["Hq"] // case["Hkv"] >= 2:
        want |= {"swap_heads"}
    if case in R.MANY:
        want |= {"see_evicted", "drop_ring_oldest", "drop_split_ge64", "drop_split_32_63", "fold_w64", "fold_w32"}
    if case in R.GROUPS:
        want |= {"see_evicted", "drop_ring_oldest"}
    if case in R.FILLS:
        want |= {"see_evicted", "drop_ring_oldest", "see_beyond_fill", "see_beyond_sink"}
    assert want <= set(low), (case["id"], want - set(low))
    for kind in {MUTANTS[m] for m in low if MUTANTS[m]}:
        pairs = set(kinds.get(kind, []))
        assert len(pairs) >= 2 and (case["Hkv"] < 2 or len({p[3] for p in pairs}) >= 2), (case["id"], kind, pairs)


# ------------------------------------------------------------------------------------------------ 3. randn does not
def test_randn_at_the_long_kv_shape_hides_a_dropped_split_and_a_miscounted_key():
    """the inputs of tests/test_gpu_decode.py::test_long_kv[16384] (its _case at seed 42) and its tolerance (atol = rtol =
    2e-2): a decode that loses the first or the last 256 keys, loses one key or counts one twice still passes"""
    B, Hq, Hkv, Nkv, D = 1, 32, 8, 16384, 128
    g = torch.Generator().manual_seed(42)
    q, k, v = (rand(s, g, torch.bfloat16) for s in ((B, Hq, 1, D), (B, Hkv, Nkv, D), (B, Hkv, Nkv, D)))
    sa = rand((Hq,), g, torch.float32, 2.0).to(torch.bfloat16)
    ref = O.decode_dense(q, k, v, sa)
    twice = torch.cat([torch.arange(Nkv), torch.tensor([Nkv - 1])])
    for what, keep in (("first split", slice(256, None)), ("last split", slice(0, Nkv - 256)), ("one key", slice(0, Nkv - 1)),
                       ("one key twice", twice)):
        d = (O.decode_dense(q, k[:, :, keep], v[:, :, keep], sa) - ref).abs()
        print(f"randn, {what}: moves the output by {d.max().item():.2e} (max |ref| {ref.abs().max().item():.3f}, allowed 2e-2)")
        assert bool((d <= 2e-2 + 2e-2 * ref.abs()).all()) and d.max().item() < 2e-2, what
        assert d.max().item() > 1e-4, what          # (the mutants are real: they do move the output)
