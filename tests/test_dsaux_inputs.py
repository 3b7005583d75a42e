"""CPU proofs for the Delta / ds_aux tests of the backward preprocess pass (tests/test_gpu_dsaux.py): no GPU.

  1. tests/dsaux_inputs.py restates the workspace layout and the kernel rule: pinned against sfa_bwd_workspace_bytes on the
     cross-compiled library, and every case of the table reaches the kernel it is listed under.
  2. A Python model of the pass (rows -> waves of 16 -> blocks of 64 -> partials [B, Hq, nblk] -> the reducer's walk over
     t in range(B * nblk)), fp64 arithmetic on an O rounded to the dtype and an f32 LSE, stays within HALF of the Delta and
     ds_aux bounds on every row class of every case.
  3. Twelve mutants of that model - each one a slip the real kernels could make - exceed a bound at least TEN times on at
     least one class of every case they apply to (MUTANTS says which), and each applies to at least one case.
  4. randn does not see them: on the inputs of test_gpu_varlen.py::test_varlen_fwd_bwd_matches_per_sequence_oracle the model
     without its tail block moves ds_aux by far less than the 1.5 that test allows."""
import pytest
import torch

import dsaux_inputs as X
from util import rand

HALF, TEN = 0.5, 10.0


# ------------------------------------------------------------------------------------------------ the model of the pass
def model(pr, mask, mut=None, do=None):
    """Delta [B,Hq,N] as it lands in the workspace and ds_aux [Hq], computed the way the pass is organised.  mut: a mutant."""
    B, Hq, _, N, Nk, D = pr["shape"]
    dt = pr["dtype"]
    nblk = X.cdiv(N, X.PRE_ROWS)
    P = nblk * X.PRE_ROWS
    o = pr["o"].to(dt).double()                                   # O as the forward stores it
    if mut == "o_read_contiguous":                                # O lives in [B, N, H, D] memory, read with contiguous strides
        o = o.transpose(1, 2).contiguous().view(B, Hq, N, D)
    dof = (X.make_do(pr, mask) if do is None else do).double()
    delta = (o * dof).sum(-1).float().double().view(B * Hq, N)    # f32 in the workspace
    lse = pr["lse"].float().double().reshape(-1)
    sa = pr["s_aux"].double()
    if mut == "saux_of_neighbour":
        sa = sa[torch.arange(Hq) ^ 1]
    rb = Nk if mut == "rowbase_nkv" else N                        # rowbase = (b Hq + h) * N_q
    rowbase = torch.arange(B * Hq).view(-1, 1) * rb
    i = torch.arange(P).view(1, -1)
    valid = (i < N).expand(B * Hq, P).clone()
    ic = i.clamp(max=N - 1)                                       # the clamped loads
    if mut == "padded_rows_counted":                              # the clamp without the `i < p.N` guard
        valid[:] = True
    if mut == "tail_block_dropped":
        valid &= i < (nblk - 1) * X.PRE_ROWS
    if mut == "pack_last_sequence_dropped":
        valid &= i < [a for a, b in zip(pr["cu"][:-1], pr["cu"][1:]) if b > a][-1]
    # Delta as written: rows the pass skips keep what the caller left there (the tests poison it; here 0)
    buf = torch.zeros(B * Hq * max(N, rb) + P, dtype=torch.float64)
    rows = valid[:, :N]
    buf[(rowbase + i[:, :N])[rows]] = delta[rows]
    got_delta = buf[:B * Hq * N].view(B, Hq, N)
    li = rowbase + ic - (1 if mut == "lse_of_previous_row" else 0)
    ls = lse[li.clamp(0, lse.numel() - 1)]
    h_of = (torch.arange(B * Hq) % Hq).view(-1, 1)
    term = -torch.exp(sa[h_of] - ls) * delta.gather(1, ic.expand(B * Hq, P)) * valid
    if mut == "every_chunk_lane_counts":                          # the vec kernel without `chunk == 0`: once per lane of the row
        term = term * X.lanes_per_row(D)
    waves = term.view(B, Hq, nblk, 4, X.WAVE_ROWS).sum(-1)
    if mut == "wave_partial_lost":
        waves[..., 1] = 0
    part = waves.sum(-1).float().double()                         # [B, Hq, nblk], f32
    slot_h = torch.arange(Hq) ^ 1 if mut == "partial_in_neighbour_slot" else torch.arange(Hq)
    flat = torch.zeros(B * Hq * nblk, dtype=torch.float64)
    b_i, h_i, k_i = torch.meshgrid(torch.arange(B), torch.arange(Hq), torch.arange(nblk), indexing="ij")
    flat[((b_i * Hq + slot_h[h_i]) * nblk + k_i).reshape(-1)] = part.reshape(-1)
    nb = nblk - 1 if mut == "reducer_nblk_minus_1" else nblk
    t = torch.arange((1 if mut == "reducer_stops_after_batch_0" else B) * nb)
    ds = torch.stack([flat[((t // nb) * Hq + h) * nb + t % nb].sum() for h in range(Hq)]) if nb else torch.zeros(Hq, dtype=torch.float64)
    return got_delta, ds.double()


# mutant -> the cases it applies to
MUTANTS = {
    "tail_block_dropped": lambda c: True,
    "padded_rows_counted": lambda c: c["N"] % X.PRE_ROWS != 0,
    "wave_partial_lost": lambda c: c["N"] > X.WAVE_ROWS,
    "every_chunk_lane_counts": lambda c: c["kernel"].startswith("vec"),
    "lse_of_previous_row": lambda c: c["B"] * c["Hq"] > 1,
    "rowbase_nkv": lambda c: c["Nk"] > c["N"],
    "saux_of_neighbour": lambda c: c["Hq"] >= 2,
    "partial_in_neighbour_slot": lambda c: c["Hq"] >= 2,
    "reducer_nblk_minus_1": lambda c: c["N"] > X.PRE_ROWS,
    "reducer_stops_after_batch_0": lambda c: c["B"] >= 2,
    "o_read_contiguous": lambda c: c["layout"] in ("o_bnhd", "both_bnhd"),
    "pack_last_sequence_dropped": lambda c: c["cu"] is not None,
}


def worst(pr, mask, mut=None):
    d, s = model(pr, mask, mut)
    return max(X.ratios(pr, d, s, mask))


# ------------------------------------------------------------------------------------------------ 1. layout and rule
def test_layout_is_what_the_workspace_query_covers():
    from sink_attention import _native
    lib = _native.lib()
    for name, c in X.CASES.items():
        lay = X.layout(c["B"], c["Hq"], c["N"])
        assert lay["delta"] == 0 and lay["part"] % 256 == 0 and lay["part"] >= 4 * c["B"] * c["Hq"] * c["N"]
        assert lay["end"] == X.align256(4 * c["B"] * c["Hq"] * c["N"]) + X.align256(4 * c["B"] * c["Hq"] * X.cdiv(c["N"], 64))
        for flags in (0, _native.FLAG_FORCE_GENERIC, _native.FLAG_BWD_OVERLAP):
            got = lib.sfa_bwd_workspace_bytes(c["B"], c["Hq"], c["Hkv"], c["N"], c["D"], X.SFA_DTYPE[c["dtype"]], c["ns"],
                                              c["W"], flags)
            assert got >= lay["end"], (name, flags, got, lay)
            if flags == _native.FLAG_FORCE_GENERIC or c["dtype"] == torch.float32 or c["D"] not in X.MFMA_DIMS:
                assert got == lay["end"], (name, flags, got, lay)       # nothing else in a generic backward's workspace


def test_every_case_reaches_the_kernel_it_is_listed_under():
    for name, c in X.CASES.items():
        assert X.expected_kernel(c) == c["kernel"], name
        assert X.expected_bwd(c) == c["bwd"], name
        assert 16 <= c["W"] <= 40 and c["B"] <= 3 and c["Hq"] <= 8, name
        if c["Nk"] != c["N"] or c["cu"] is not None:
            assert c["bwd"] == "mfma", name                             # served by the MFMA family only
    cs = X.CASES.values()
    assert {c["kernel"] for c in cs} == {"vec16", "vec8", "vec4", "scalar"}
    assert {1, 15, 16, 17, 63, 64, 65, 69, 133, 517, 2050} <= {c["N"] for c in cs}
    assert {c["B"] for c in cs} == {1, 2, 3} and {1, 2, 4, 8} <= {c["Hq"] // c["Hkv"] for c in cs}
    assert {128, 80, 96, 72, 64, 40, 56, 32, 24, 16, 8, 20, 256, 100} <= {c["D"] for c in cs}
    assert {"o_bnhd", "do_bnhd", "both_bnhd", "o_off8", "do_off8"} <= {c["layout"] for c in cs}
    assert X.cdiv(X.CASES["d128_bf16_n2050"]["N"], X.PRE_ROWS) > 32


def test_head_offsets_are_distinct_and_pairs_are_far_apart():
    for Hq in (2, 3, 4, 8):
        off = X.head_offsets(Hq)
        assert off.unique().numel() == Hq and off.abs().max() <= 2.0
        for h in range(Hq):
            if h ^ 1 < Hq:
                assert abs(off[h] - off[h ^ 1]) >= 2.0
            if h + 1 < Hq:
                assert abs(off[h] - off[h + 1]) >= 1.0


def test_inputs_are_what_the_bound_assumes():
    pr = X.problem("d64_bf16_n69")
    assert set(pr["sign"].unique().tolist()) == {-1.0, 1.0}
    for name, m in pr["classes"].items():
        do = X.make_do(pr, m)
        assert (do[~m] == 0).all() and (do[m].abs() == 1).all(), name
        ref = X.reference(pr, m)
        assert (ref["delta"][m] > 0).all() and (ref["delta"][~m] == 0).all() and (ref["ds"] <= 0).all()     # one sign
        assert (ref["a"] >= ref["delta"] * (1 - 1e-12)).all()
        gen = X.reference(pr, do=do)                                   # the general form agrees with the class form
        assert torch.allclose(gen["delta"], ref["delta"]) and torch.allclose(gen["A"], ref["A"])
    p = pr["p_aux"]
    assert 0.02 < p.min() and p.max() < 0.999 and 0.2 < p.median() < 0.8


# ------------------------------------------------------------------------------------------------ 2. and 3.
@pytest.mark.parametrize("name", list(X.CASES))
def test_model_within_half_and_every_mutant_ten_times_over(name):
    c, pr = X.CASES[name], X.problem(name)
    for cls, m in pr["classes"].items():
        r = worst(pr, m)
        assert r <= HALF, f"{name}/{cls}: the unmutated model reaches {r:.3f} of a bound"
    for mut, applies in MUTANTS.items():
        if not applies(c):
            continue
        best = max(((worst(pr, m, mut), cls) for cls, m in pr["classes"].items()))
        assert best[0] >= TEN, f"{name}: mutant {mut} reaches only {best[0]:.2f} bounds (class {best[1]})"


def test_every_mutant_applies_to_some_case():
    for mut, applies in MUTANTS.items():
        assert any(applies(c) for c in X.CASES.values()), mut


# ------------------------------------------------------------------------------------------------ 4. the motivation
def test_randn_at_the_old_tolerance_does_not_see_a_lost_block():
    """inputs of test_gpu_varlen.py::test_varlen_fwd_bwd_matches_per_sequence_oracle (bf16), the model against the oracle"""
    g = torch.Generator().manual_seed(31)
    Hq, Hkv, D, ns, W, cu, dt = 8, 2, 128, 2, 40, [0, 70, 71, 300, 517], torch.bfloat16
    T = cu[-1]
    q, k, v = rand((1, Hq, T, D), g, dt), rand((1, Hkv, T, D), g, dt), rand((1, Hkv, T, D), g, dt)
    do = rand((1, Hq, T, D), g, dt)
    sa = rand((Hq,), g, torch.float32, 0.5)
    o, lse = X._forward(q, k, v, ns, W, sa, cu)
    pr = dict(shape=(1, Hq, Hkv, T, T, D), dtype=dt, o=o.double(), lse=lse.double(), s_aux=sa, cu=cu)
    ref = -(torch.exp(sa.double().view(1, Hq, 1) - lse.double()) * (o.double() * do.double()).sum(-1)).sum((0, 2))
    mask = torch.ones(1, Hq, T, dtype=torch.bool)
    _, ok = model(pr, mask, do=do)
    _, bad = model(pr, mask, "tail_block_dropped", do=do)
    moved = (bad - ref).abs().max().item()
    assert (ok - ref).abs().max().item() < 0.1
    assert 0.0 < moved < 1.5, moved                                    # a lost block passes `maxdiff < tg * 10`
    assert moved < 0.5                                                 # ... with room to spare
