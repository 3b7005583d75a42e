"""Delta and ds_aux of the backward preprocess pass (csrc/sfa_generic.hip: bwd_preprocess_vec_kernel, bwd_preprocess_kernel,
dsaux_reduce_kernel) against the fp64 oracle, row class by row class, under the per-sum bounds of tests/dsaux_inputs.py:

    Delta, row by row   |got - ref| <= 4 u a_i + u |ref_i|          ds_aux[h]   |got - ref| <= 4 u A_h + u |ref_h|

Raw C-ABI calls: O, LSE, dQ, dK, dV and ds_aux are NaN-filled and every workspace byte is 0xFF before the call; Delta is read
back from the start of the workspace.  tests/test_dsaux_inputs.py proves on the CPU that a model of the correct pass stays
within half of these bounds on the very cases and classes run here, and that twelve wrong passes each leave them tenfold.
Every case prints its largest ratios (pytest -s shows them; profiles/dsaux_ratios.log keeps one run)."""
import pytest
import torch

import dsaux_inputs as X

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def forwards():
    """raw_fwd of a case, once per module (the forward does not depend on the class)"""
    cache = {}

    def get(name):
        if name not in cache:
            c, pr = X.CASES[name], X.problem(name)
            cache[name] = X.raw_fwd(c, pr["q"].to(DEV), pr["k"].to(DEV), pr["v"].to(DEV), pr["s_aux"].to(DEV))
        return cache[name]
    return get


def run_class(name, st, mask=None, do=None):
    """one backward on the case's layout; returns the result and its (Delta, ds_aux) ratios"""
    c, pr = X.CASES[name], X.problem(name)
    d = X.make_do(pr, mask) if do is None else do
    r = X.raw_bwd(st, X.place_do(c, d.to(DEV)))
    assert not torch.isnan(r["ds_aux"]).any(), f"{name}: NaN in ds_aux"
    assert not torch.isnan(r["delta"]).any(), f"{name}: NaN in the Delta region (a row the pass did not write)"
    assert not torch.isnan(r["part"]).any(), f"{name}: NaN among the ds_aux partials"
    return r, X.ratios(pr, r["delta"], r["ds_aux"], mask, do if mask is None else None)


@pytest.mark.parametrize("name", list(X.CASES))
def test_delta_and_ds_aux_within_their_sum_bounds(name, forwards):
    c, pr = X.CASES[name], X.problem(name)
    st = forwards(name)
    # the kernels the case is listed under: the preprocess rule on the tensors actually handed over, the family from the path
    o_al, do_al = X.rows16(st["o"]), X.rows16(X.place_do(c, X.make_do(pr, pr["classes"]["all"]).to(DEV)))
    assert X.preprocess_vectorised(c["dtype"], c["D"], o_al and do_al) == c["kernel"].startswith("vec"), name
    if c["kernel"].startswith("vec"):
        assert X.lanes_per_row(c["D"]) == int(c["kernel"][3:])
    if c["layout"] == "o_off8":
        assert not o_al and st["fwd_path"] == "fwd_generic_f32math", st["fwd_path"]
    worst = [0.0, 0.0, "", ""]
    for cls, m in pr["classes"].items():
        r, (rd, rs) = run_class(name, st, m)
        want = "bwd_mfma_" if c["bwd"] == "mfma" else "bwd_generic_f32math"
        assert r["bwd_path"].startswith(want), (name, r["bwd_path"])
        if rd > worst[0]:
            worst[0], worst[2] = rd, cls
        if rs > worst[1]:
            worst[1], worst[3] = rs, cls
        assert rd <= 1.0, f"{name}/{cls}: Delta reaches {rd:.3f} of its row bound 4 u a + u |ref|"
        assert rs <= 1.0, f"{name}/{cls}: ds_aux reaches {rs:.3f} of its bound 4 u A + u |ref|"
        outside = ~m.any(2).any(0)                                   # heads with no row in the class: exactly 0
        assert (r["ds_aux"].cpu()[outside] == 0).all() and (r["delta"].cpu()[~m] == 0).all(), f"{name}/{cls}"
    print(f"\ndsaux_ratio {name:22s} {c['kernel']:6s} {c['bwd']:7s} Delta {worst[0]:.4f} ({worst[2]})  ds_aux {worst[1]:.4f} ({worst[3]})")


def test_ds_aux_of_all_rows_is_the_sum_over_the_block_classes(forwards):
    name = "d128_bf16_n517"
    pr, st = X.problem(name), forwards(name)
    B, Hq, _, N, _, _ = pr["shape"]
    whole, _ = run_class(name, st, pr["classes"]["all"])
    parts = sum(run_class(name, st, m)[0]["ds_aux"].double() for m in X.block_classes(B, Hq, N))
    tol = X.reference(pr, pr["classes"]["all"])["tol_ds"]
    assert ((parts - whole["ds_aux"].double()).abs().cpu() <= tol).all(), (parts, whole["ds_aux"], tol)


def test_ds_aux_of_a_batch_is_the_sum_of_its_elements_run_alone(forwards):
    name = "d64_bf16_n69"
    c, pr, st = X.CASES[name], X.problem(name), forwards(name)
    assert c["B"] == 3
    m = pr["classes"]["all"]
    whole, _ = run_class(name, st, m)
    do = X.make_do(pr, m).to(DEV)
    alone = torch.zeros(c["Hq"], dtype=torch.float64, device=DEV)
    for b in range(c["B"]):
        sb = X.raw_fwd(c, *(pr[x][b:b + 1].to(DEV) for x in ("q", "k", "v")), pr["s_aux"].to(DEV))
        rb = X.raw_bwd(sb, do[b:b + 1])
        assert torch.equal(rb["delta"], whole["delta"][b:b + 1])      # a row's Delta does not depend on its batch
        alone += rb["ds_aux"].double()
    tol = X.reference(pr, m)["tol_ds"]
    assert ((alone - whole["ds_aux"].double()).abs().cpu() <= tol).all(), (alone, whole["ds_aux"], tol)


@pytest.mark.parametrize("name", ["d128_bf16_n517", "f32_d64_n133", "pack_d80_fp16"])
def test_two_calls_are_bitwise_equal(name, forwards):
    pr, st = X.problem(name), forwards(name)
    a, _ = run_class(name, st, pr["classes"]["all"])
    b, _ = run_class(name, st, pr["classes"]["all"])
    assert torch.equal(a["ds_aux"], b["ds_aux"]) and torch.equal(a["delta"], b["delta"]) and torch.equal(a["part"], b["part"])


def test_unaligned_do_with_more_keys_than_queries_is_refused_before_the_pass(forwards):
    """bwd_mfma_refused: N_q != N_kv has no generic form, so rows off 16-byte alignment are SFA_ERR_UNSUPPORTED, asked before
    the preprocess: ds_aux and every workspace byte stay as the caller left them"""
    name = "d128_bf16_nq37_nk101"
    c, pr, st = X.CASES[name], X.problem(name), forwards(name)
    do = X.place_do(dict(c, layout="do_off8"), X.make_do(pr, pr["classes"]["all"]).to(DEV))
    assert not X.rows16(do)
    r = X.raw_bwd(st, do, refused=True)
    assert torch.isnan(r["ds_aux"]).all() and (r["ws"] == 0xFF).all() and torch.isnan(r["dq"]).all()


# ------------------------------------------------------------------------------------------------ through autograd
def _autograd(pr, c, s_aux, grad=None):
    """sink_flash_attention forward + backward; grad: a dO, or None for out.sum().backward()"""
    from sink_attention import sink_flash_attention
    q, k, v = (pr[x].to(DEV).requires_grad_(True) for x in ("q", "k", "v"))
    sa = s_aux.to(DEV).requires_grad_(True)
    out = sink_flash_attention(q, k, v, num_sink=c["ns"], window_size=c["W"], s_aux=sa)
    if grad is None:
        out.sum().backward()
    else:
        out.backward(grad)
    return sa.grad


def test_bf16_s_aux_gets_the_cast_of_the_raw_ds_aux():
    name = "d64_bf16_n69"
    c, pr = X.CASES[name], X.problem(name)
    sa16 = pr["s_aux"].bfloat16()
    do = X.make_do(pr, pr["classes"]["all"]).to(DEV)
    got = _autograd(pr, c, sa16, do)
    st = X.raw_fwd(c, pr["q"].to(DEV), pr["k"].to(DEV), pr["v"].to(DEV), sa16.float().to(DEV))
    raw = X.raw_bwd(st, do)["ds_aux"]
    assert got.dtype == torch.bfloat16 and torch.equal(got, raw.bfloat16())
    # and the f32 result is the right one for THIS s_aux (the rounded parameter): the bound, with the reference rebuilt
    lse = torch.log(torch.exp(pr["lse"]) - torch.exp(pr["s_aux"].double()).view(1, -1, 1) + torch.exp(sa16.double()).view(1, -1, 1))
    p = torch.exp(sa16.double().view(1, -1, 1) - lse)
    scale = (1 - p) / (1 - pr["p_aux"])                            # o = (1 - p_aux) * (softmax over the keys) v
    ref = -(p * scale * pr["delta_all"]).sum((0, 2))
    A = (p * scale * pr["a_all"]).sum((0, 2))
    assert ((raw.double().cpu() - ref).abs() <= X.FACTOR * pr["u"] * A + pr["u"] * ref.abs()).all()


def test_sum_backward_is_an_explicit_ones_grad(forwards):
    name = "d128_bf16_o_bnhd"
    c, pr, st = X.CASES[name], X.problem(name), forwards(name)
    ones = torch.ones(pr["q"].shape, dtype=pr["dtype"])
    got = _autograd(pr, c, pr["s_aux"])                              # a stride-0 grad, materialised by the op
    r, (rd, rs) = run_class(name, st, do=ones)
    assert torch.equal(got, r["ds_aux"])
    assert rd <= 1.0 and rs <= 1.0, (rd, rs)                         # terms of both signs: the same form of bound holds


def test_fp32_grad_on_bf16_inputs_is_the_bf16_grad(forwards):
    name = "d32_bf16_n65"
    c, pr, st = X.CASES[name], X.problem(name), forwards(name)
    m = pr["classes"]["tail"]
    got = _autograd(pr, c, pr["s_aux"], X.make_do(pr, m).float().to(DEV))       # +-1 and 0: the cast is exact
    r, _ = run_class(name, st, m)
    assert torch.equal(got, r["ds_aux"])
