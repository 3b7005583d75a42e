"""CPU proofs for the softmax-range inputs (tests/range_inputs.py) at every shape, head dim and dtype
tests/test_gpu_softmax_range.py runs.  No kernel is involved: the fp64 tile-walk model of the forward kernels' deferred
rescale against oracle.sink_oracle, against its own mutants and against its reduced-precision twin.  Every test prints
what it measured (-s).

  model      the unmutated walk equals the oracle to 1e-9 (O and LSE), packs included.
  coverage   every staircase_up case: at least 64 events with 2^-16 <= alpha < 2^-8 after a row's first visible tile, at least
             one in every 64-row wave (per batch and head) that has a visible later tile, each of those waves with a moving
             row and a still row in the same tile, rises of 2 .. 8 log2 units that do not move the reference beside moves.
             Measured: 416 - 1748 events per case (strip shapes 416 - 857), every wave covered.
  mutants    every switch of range_inputs.MUTANTS moves O by at least 10 x the forward tolerance of the dtype on every
             staircase_up case (smallest measured: bf16 20.0 on asm_nq_lt_nk, fp16 110, fp32 2.5e4; never_fp16 overflows: inf).
             The other families never take the rescale after the first tile (they test range, not alpha) and are not asked to.
  the gap    make_qkv-style randn inputs at the same shapes: at most 8 events after a row's first visible tile per shape (zero at
             two shapes in three), all with a rise under 10 log2 units, with s_aux = 0.5 randn and without.  The real mask-edge
             probes (tests/probe_inputs.py) were expected to take the branch only with an alpha too small to matter; measured
             on dense_probe at (1, 4, 1, 777, 777, 128, 4, 400) they have 2805 moves, 1001 of them mid-range, and alpha := 0 moves
             O by 106 tolerances.  So the probes do see that one mutant; the test prints every mutant's factor on them and
             asserts only what holds (the walk equals the oracle, the branch is taken).
  precision  the precision model (S in f32, P rounded to the dtype before the PV and row-sum products, O rounded; backward:
             delta from the rounded O, P and dS rounded) is within HALF of every tolerance the GPU file applies: O, LSE,
             dQ, dK, dV, ds_aux.  Largest margins measured (fraction of the tolerance): bf16 O 0.475, LSE 0.450; fp16 O 0.333;
             fp32 O 0.463 (fp32_down), gradients at most 0.11.

Final amplitudes (range_inputs): STEPS = (0.6, 0.75, 0.9) sqrt(128) = 6.8 / 8.5 / 10.2 nat at gain 1 (9.8 / 12.2 / 14.7 log2 units;
at gain 0.5 4.9 / 6.1 / 7.3, under the rule singly and over it in pairs); SINK_TOP = 48 nat; OFFSET = 60 nat; fp32 inputs: staircase_down
and offset at a quarter of that (FP32_SCALE: at full height the f32 dot products alone cost 1.3 x the fp32 O tolerance),
staircase_up as a sawtooth of three full steps (FP32_PERIOD); GUARD = 4 control rows behind each step."""
import math

import pytest
import torch

import probe_inputs as P
import range_inputs as R
from oracle import sink_oracle as O

IDS = [c["id"] for c in R.DENSE_CASES]
UP = [c for c in R.DENSE_CASES if c["family"] == "staircase_up"]


def _inf_abs(x):
    d = x.abs()
    return torch.where(torch.isfinite(d), d, torch.full_like(d, float("inf"))).max().item()


def _check_coverage(cov, what):
    print(what, cov)
    assert cov["mid"] >= 64, (what, cov)
    assert cov["waves"] > 0 and cov["waves_mid"] == cov["waves"], (what, cov)
    assert cov["waves_mixed"] == cov["waves"], (what, cov)
    assert cov["under"] > 0 and cov["moves"] > 0, (what, cov)


# ------------------------------------------------------------------------------------------------ the model itself
@pytest.mark.parametrize("case", R.DENSE_CASES, ids=IDS)
def test_walk_equals_oracle_and_covers(case):
    B, Hq, Hkv, Nq, Nk, D, ns, W = case["shape"]
    inp = R.case_inputs(case)
    o_r, lse_r = O.sink_attention_dense(inp["q"], inp["k"], inp["v"], ns, W, inp["s_aux"])
    o, lse, ev = R.tile_walk(inp["q"], inp["k"], inp["v"], ns, W, inp["s_aux"])
    eo, el = (o - o_r).abs().max().item(), (lse - lse_r).abs().max().item()
    cov = R.coverage(ev)
    print(case["id"], "walk - oracle: O %.1e LSE %.1e" % (eo, el), cov)
    assert eo < 1e-9 and el < 1e-9
    if case["family"] == "staircase_up":
        _check_coverage(cov, case["id"])
    if case["family"] == "staircase_down":
        # the reference never moves once the top level has been seen; p underflows behind it
        assert cov["later"] <= 8, cov
        if case["dtype"] != "fp32":
            s = R._scores(inp["q"], inp["k"], ns, W, False)
            depth = (s.max(-1).values.unsqueeze(-1) - s)[torch.isfinite(s)].max().item()
            print(case["id"], "deepest visible p: 2^-%.0f" % depth)
            assert depth > 126.0


def test_walk_of_a_tile_order_detail_and_the_event_list():
    """events() lists (batch, head, row, tile, alpha); a row without any visible key keeps O = 0, LSE = -inf; N_q < N_kv"""
    inp = R.dense_range("staircase_up", 1, 2, 1, 70, 200, 32, 3, 40, torch.bfloat16, 5)
    o, lse, ev = R.tile_walk(inp["q"], inp["k"], inp["v"], 3, 40, None)
    o_r, lse_r = O.sink_attention_dense(inp["q"], inp["k"], inp["v"], 3, 40, None)
    assert (o - o_r).abs().max().item() < 1e-9 and (lse - lse_r).abs().max().item() < 1e-9
    lst = R.events(ev)
    assert len(lst) == int(ev["asked"].sum()) and all(0 < a < 1 for *_, a in lst)
    q0 = torch.zeros(1, 1, 4, 32, dtype=torch.bfloat16)
    o, lse, _ = R.tile_walk(q0, inp["k"][:, :, :4], inp["v"][:, :, :4], 0, 0, None)
    assert (o == 0).all() and (lse == float("-inf")).all()


def test_pack_walk_equals_the_per_sequence_oracle_and_covers():
    c = R.PACK_CASE
    inp = R.pack_inputs()
    o, lse = R.walk_pack(R.tile_walk, inp, c["cu"], c["ns"], c["W"])
    for a, b in zip(c["cu"][:-1], c["cu"][1:]):
        sl = (slice(None), slice(None), slice(a, b))
        o_r, lse_r = O.sink_attention_dense(inp["q"][sl], inp["k"][sl], inp["v"][sl], c["ns"], c["W"], inp["s_aux"])
        assert (o[sl] - o_r).abs().max().item() < 1e-9 and (lse[:, :, a:b] - lse_r).abs().max().item() < 1e-9
    for s, (a, b) in enumerate(zip(c["cu"][:-1], c["cu"][1:])):
        ev = R.tile_walk(inp["q"][:, :, a:b], inp["k"][:, :, a:b], inp["v"][:, :, a:b], c["ns"], c["W"], inp["s_aux"])[2]
        if s == 0:
            assert int(ev["later"].sum()) == 0          # the randn sequence
        else:
            _check_coverage(R.coverage(ev), f"pack sequence {s}")


# ------------------------------------------------------------------------------------------------ mutants
@pytest.mark.parametrize("case", UP, ids=[c["id"] for c in UP])
def test_every_mutant_moves_o_by_ten_tolerances(case):
    B, Hq, Hkv, Nq, Nk, D, ns, W = case["shape"]
    tol = R.TOL_O[R.DT[case["dtype"]]]
    inp = R.case_inputs(case)
    o_r, _ = O.sink_attention_dense(inp["q"], inp["k"], inp["v"], ns, W, inp["s_aux"])
    fac = {mu: _inf_abs(R.tile_walk(inp["q"], inp["k"], inp["v"], ns, W, inp["s_aux"], mutant=mu)[0] - o_r) / tol
           for mu in R.MUTANTS}
    print(case["id"], "mutant factors:", {k: round(v, 1) for k, v in fac.items()})
    assert min(fac.values()) >= 10, fac


# ------------------------------------------------------------------------------------------------ the gap, pinned
SHAPES = sorted(set((c["shape"], c["dtype"]) for c in R.DENSE_CASES), key=str)


@pytest.mark.parametrize("shape,dtn", SHAPES, ids=["x".join(map(str, s)) + "_" + d for s, d in SHAPES])
def test_randn_inputs_never_move_the_reference(shape, dtn):
    B, Hq, Hkv, Nq, Nk, D, ns, W = shape
    dt = R.DT[dtn]
    g = torch.Generator().manual_seed(42)                        # tests/util.py::make_qkv
    q = R._rand((B, Hq, Nq, D), g, dt)
    k, v = R._rand((B, Hkv, Nk, D), g, dt), R._rand((B, Hkv, Nk, D), g, dt)
    sa = R._rand((Hq,), g, torch.float32, 0.5)
    for aux in (sa, None):
        ev = R.tile_walk(q, k, v, ns, W, aux)[2]
        n = int(ev["later"].sum())
        print(shape, dtn, "s_aux" if aux is not None else "no s_aux", "events after the first visible tile:", n,
              "largest rise %.1f log2 units" % ev["rise"][ev["vis"] & torch.isfinite(ev["rise"])].max().item())
        # measured: zero at 21 of the 31 (shape, dtype) pairs, 1 - 3 at nine, 8 at (1, 4, 2, 750, 750, 64, 4, 128) (rows whose
        # sink tile shows 4 keys before a 128-key window); every rise below 10 log2 units.  The staircase: 416 or more.
        assert n <= 8


def test_probe_inputs_take_the_branch():
    shape = (1, 4, 1, 777, 777, 128, 4, 400)
    B, Hq, Hkv, Nq, Nk, D, ns, W = shape
    pr = P.dense_probe(B, Hq, Hkv, Nq, Nk, D, ns, W, torch.bfloat16, 1000, aux=True)
    o_r, _ = O.sink_attention_dense(pr["q"], pr["k"], pr["v"], ns, W, pr["s_aux"])
    o, _, ev = R.tile_walk(pr["q"], pr["k"], pr["v"], ns, W, pr["s_aux"])
    assert (o - o_r).abs().max().item() < 1e-9
    fac = {mu: _inf_abs(R.tile_walk(pr["q"], pr["k"], pr["v"], ns, W, pr["s_aux"], mutant=mu)[0] - o_r) / R.TOL_O[torch.bfloat16]
           for mu in R.MUTANTS}
    print("probes:", int(ev["later"].sum()), "moves,", int(R.mid(ev).sum()), "mid-range; mutant factors", {k: round(v, 1) for k, v in fac.items()})
    assert int(ev["later"].sum()) > 0


# ------------------------------------------------------------------------------------------------ kernel precision
def _margins(dt, inp, ns, W, cu=None):
    q, k, v, do, sa = (inp[x] for x in ("q", "k", "v", "do", "s_aux"))
    mar = {}
    worst = lambda name, x: mar.__setitem__(name, max(mar.get(name, 0.0), x))
    dsa_p, dsa_r = 0.0, 0.0
    g_all = []
    for a, b in zip(*(([0], [q.shape[2]]) if cu is None else (cu[:-1], cu[1:]))):
        sq = (slice(None), slice(None), slice(a, b))
        sk = sq if cu is not None else (slice(None),) * 3
        o_r, lse_r = O.sink_attention_dense(q[sq], k[sk], v[sk], ns, W, sa)
        g_r = O.sink_attention_bwd_dense(q[sq], k[sk], v[sk], do[sq], ns, W, sa)
        o_p, lse_p = R.precision_fwd(q[sq], k[sk], v[sk], ns, W, sa)
        g_p = R.precision_bwd(q[sq], k[sk], v[sk], do[sq], o_p, lse_p, ns, W, sa)
        worst("o", (o_p.double() - o_r).abs().max().item() / R.TOL_O[dt])
        fin = torch.isfinite(lse_r)
        worst("lse", (lse_p.double()[fin] - lse_r[fin]).abs().max().item() / R.TOL_LSE)
        g_all.append((g_p, g_r))
        dsa_p, dsa_r = dsa_p + g_p[3].double(), dsa_r + g_r[3]
    for i, name in enumerate(("dq", "dk", "dv")):
        ref = torch.cat([g_r[i] for _, g_r in g_all], 2)
        got = torch.cat([g_p[i].double() for g_p, _ in g_all], 2)
        mar[name] = (got - ref).abs().max().item() / R.grad_tol(dt, ref)
    mar["ds_aux"] = (dsa_p - dsa_r).abs().max().item() / R.grad_tol(dt, dsa_r, aux=True)
    return mar


@pytest.mark.parametrize("case", R.DENSE_CASES, ids=IDS)
def test_precision_model_is_within_half_of_every_tolerance(case):
    B, Hq, Hkv, Nq, Nk, D, ns, W = case["shape"]
    mar = _margins(R.DT[case["dtype"]], R.case_inputs(case), ns, W)
    print(case["id"], "precision model / tolerance:", {k: round(v, 3) for k, v in mar.items()})
    assert max(mar.values()) <= 0.5, mar


def test_precision_model_on_the_pack():
    c = R.PACK_CASE
    mar = _margins(R.DT[c["dtype"]], R.pack_inputs(), c["ns"], c["W"], cu=c["cu"])
    print("pack precision model / tolerance:", {k: round(v, 3) for k, v in mar.items()})
    assert max(mar.values()) <= 0.5, mar


# ------------------------------------------------------------------------------------------------ the cache calls
def test_decode_inputs_span_the_range():
    """staircase_down over DECODE_NKV keys: the level of the last 256 keys lies more than 100 log2 units below the first 256
    for a head of gain 1 (above it for the heads of gain -1); aux_sweep carries -40 .. +40 nat"""
    for cid, dtn, Hq, Hkv, D, family in R.DECODE_CASES:
        inp = R.history_range(family, 2, Hq, Hkv, D, R.DECODE_NKV, 1, R.DT[dtn], 7600 + len(cid))
        if family == "aux_sweep":
            assert sorted(set(inp["s_aux"].tolist())) == sorted(set(R.AUX_SWEEP[h % 5] for h in range(Hq)))
            continue
        span = (inp["H"][:256].mean() - inp["H"][-256:].mean()).item() * R.LOG2E
        print(cid, "first 256 keys above the last 256 by %.0f log2 units at gain 1; gains" % span, sorted(set(inp["a"].flatten().tolist())))
        assert (span > 100) == (dtn != "fp32") and span > 25
        assert {1.0, 0.5, 0.0} <= set(inp["a"].flatten().tolist()) and (Hq < 5 or -1.0 in inp["a"].flatten().tolist())
        o = O.decode_dense(inp["q"], inp["k"], inp["v"], inp["s_aux"])
        assert torch.isfinite(o).all() and o.abs().max().item() > 10 * 1.6e-2


def test_precision_model_on_the_cache_calls():
    """decode over every key and the n = 5 chunk over sinks + ring are rows of dense attention (the last position(s) of the
    history): the precision model stays within half of tests/util.py::DECODE_TOL on the inputs the GPU file runs.
    Measured: chunk 0.36 (bf16 staircase_down, max |O| 2.3), everything else below 0.15."""
    from util import DECODE_TOL
    ns, W, extra, n = R.CHUNK_RING
    total = ns + W + extra
    runs = [("chunk " + c[0], c, R.history_range(c[5], 2, c[2], c[3], c[4], total + n, n, R.DT[c[1]], 7700 + len(c[0]), step=128), ns, W)
            for c in R.CHUNK_CASES]
    runs += [("decode " + c[0], c, R.history_range(c[5], 2, c[2], c[3], c[4], R.DECODE_NKV, 1, R.DT[c[1]], 7600 + len(c[0])), 0, R.DECODE_NKV)
             for c in R.DECODE_CASES]
    for what, c, inp, ns_, W_ in runs:
        o_r, _ = O.sink_attention_dense(inp["q"], inp["k"], inp["v"], ns_, W_, inp["s_aux"])
        o_p, _ = R.precision_fwd(inp["q"], inp["k"], inp["v"], ns_, W_, inp["s_aux"])
        mar = (o_p.double() - o_r).abs().max().item() / DECODE_TOL[R.DT[c[1]]]
        print(what, "precision model / tolerance: %.3f, max |O| %.2f" % (mar, o_r.abs().max().item()))
        assert mar <= 0.5, (what, mar)
