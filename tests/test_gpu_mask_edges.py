"""GPU parity on mask-edge probe inputs (tests/probe_inputs.py): the product ops through the C ABI against the fp64 oracle
of the same inputs, one group of cases per code path that decides which (row, key) pairs exist, at windows where randn
inputs cannot tell a mask that is off by one key from a correct one (tests/test_probe_inputs.py proves both on the CPU).
Tolerances are those of the neighbouring randn test of the same kernel; every case asserts the kernel path it ran.
dK and dV of the dense and the packed calls are ALSO judged element by element against the bound of their own sum
(util.assert_within_sum_bound: |got - ref| <= 4 u A + u |ref|), because their other tolerance scales with max |ref| and
lets a mask error confined to the dK/dV kernel pass (tests/test_probe_inputs.py, part 2d, proves both).
A row aimed at its diagonal key meets its maximum in the LAST tile of its walk, a row aimed at a sink key in the FIRST:
the online-softmax rescale branch is forced both ways."""
import functools
import random

import pytest
import torch

import probe_inputs as P
from oracle import sink_oracle as O
from test_gpu_decode_multi import TOL, _expected_path, _oracle_rows
from test_gpu_tree_verify import TREES, _oracle_tree, _tree_path_name
from test_tree_host import random_tree
from util import (PROBE_TOL_DKDV, PROBE_TOL_DQ, PROBE_TOL_DS_AUX, PROBE_TOL_O, UNIT_ROUNDOFF, assert_close,
                  assert_within_sum_bound, dkdv_kernel_name, maxdiff, oracle_bwd, oracle_fwd, probe_reference,
                  sum_bound_ratio)

pytestmark = pytest.mark.gpu
DEV = "cuda"
DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}


def _path():
    from sink_attention import _native
    return _native.last_path()


def _ex():
    from sink_attention.sink_flash_attention import _sink_flash_attention_ex
    return _sink_flash_attention_ex


# ------------------------------------------------------------------------------------------------ dense calls
@functools.lru_cache(maxsize=1)
def _dense(case_id):
    """probe inputs and fp64 oracle of one case (shared by the two dK/dV modes)"""
    case = next(c for c in P.DENSE_CASES if c["id"] == case_id)
    B, Hq, Hkv, Nq, Nk, D, ns, W = case["shape"]
    pr = P.dense_case_probe(case)
    o_r, _, grads = probe_reference(pr, ns, W)       # (dq, dk, dv, ds_aux and the bound terms A_K, A_V)
    return pr, o_r, grads


@pytest.mark.parametrize("dkdv", ["rule", "asm"], indirect=True)     # the fixture's two modes, run back to back per case
@pytest.mark.parametrize("case", P.DENSE_CASES, ids=[c["id"] for c in P.DENSE_CASES])
def test_dense_mask_edges(case, dkdv):
    B, Hq, Hkv, Nq, Nk, D, ns, W = case["shape"]
    dt = DT[case["dtype"]]
    pr, o_r, (dq_r, dk_r, dv_r, dsa_r, ak_r, av_r) = _dense(case["id"])
    if case.get("layout") == "bnhd":           # [B, N, H, D] storage, passed as transposed views
        qd, kd, vd = (pr[x].transpose(1, 2).contiguous().to(DEV).transpose(1, 2).requires_grad_(True) for x in "qkv")
        dod = pr["do"].transpose(1, 2).contiguous().to(DEV).transpose(1, 2)
    else:
        qd, kd, vd = (pr[x].to(DEV).requires_grad_(True) for x in "qkv")
        dod = pr["do"].to(DEV)
    sad = pr["s_aux"].to(DEV).requires_grad_(True) if pr["s_aux"] is not None else None
    generic = case.get("generic", False)
    out = _ex()(qd, kd, vd, ns, W, s_aux=sad, force_generic=generic)
    fwd_path = _path()
    assert case["fwd"] in fwd_path, fwd_path
    out.backward(dod)
    bwd_path = _path()
    print(case["id"], dkdv, fwd_path, bwd_path)
    assert case["dq"] in bwd_path, bwd_path
    want = None if generic else dkdv_kernel_name(dkdv, B, Hkv, Nq, Nk, D, W, dtype=dt, ns=ns)
    if dkdv == "rule" and "rule_dkdv" in case:
        want = case["rule_dkdv"]
    assert want is None or want in bwd_path, (want, bwd_path)
    if dt == torch.float32:
        assert_close(out, o_r, 2e-5, 0.0, "fwd")
        for got, ref, what in ((qd.grad, dq_r, "dq"), (kd.grad, dk_r, "dk"), (vd.grad, dv_r, "dv")):
            assert_close(got, ref, 2e-4, 0.0, what)
        return
    to = PROBE_TOL_O[dt]                     # (2e-2 bf16, 1e-2 fp16; dQ 5e-2; dK / dV 5e-2 max(1, max |ref|) + 5e-2 |ref|)
    assert_close(out, o_r, to, to, "fwd")
    assert_close(qd.grad, dq_r, PROBE_TOL_DQ, PROBE_TOL_DQ, "dq")
    assert_close(kd.grad, dk_r, PROBE_TOL_DKDV * max(1.0, dk_r.abs().max().item()), PROBE_TOL_DKDV, "dk")
    assert_close(vd.grad, dv_r, PROBE_TOL_DKDV * max(1.0, dv_r.abs().max().item()), PROBE_TOL_DKDV, "dv")
    u = UNIT_ROUNDOFF[dt]
    print(f"sum bound {case['id']} {dkdv}: dK {sum_bound_ratio(kd.grad, dk_r, ak_r, u):.3f} dV {sum_bound_ratio(vd.grad, dv_r, av_r, u):.3f}")
    assert_within_sum_bound(kd.grad, dk_r, ak_r, u, "dk")
    assert_within_sum_bound(vd.grad, dv_r, av_r, u, "dv")
    if sad is not None:
        assert maxdiff(sad.grad, dsa_r) < PROBE_TOL_DS_AUX * max(1.0, dsa_r.abs().max().item())


# ------------------------------------------------------------------------------------------------ packed batches
@functools.lru_cache(maxsize=1)
def _pack(i):
    c = P.VARLEN_CASES[i]
    cu, ns, W = c["cu"], c["ns"], c["W"]
    T = cu[-1]
    pr = P.pack_case_probe(i)
    o = torch.zeros(pr["q"].shape, dtype=torch.float64)
    dq, dk, dv = (torch.zeros(pr[x].shape, dtype=torch.float64) for x in "qkv")
    ak, av = torch.zeros_like(dk), torch.zeros_like(dv)
    dsa = torch.zeros(c["Hq"], dtype=torch.float64)
    for a, b in zip(cu[:-1], cu[1:]):
        if b == a:
            continue
        sl = (slice(None), slice(None), slice(a, b))
        args = (pr["q"][sl], pr["k"][sl], pr["v"][sl])
        o[sl], _ = oracle_fwd(*args, ns, W, pr["s_aux"])
        g = oracle_bwd(*args, pr["do"][sl], ns, W, pr["s_aux"], bounds=True)
        dq[sl], dk[sl], dv[sl], ak[sl], av[sl] = g[0], g[1], g[2], g[4], g[5]
        dsa += g[3]
    return pr, o, dq, dk, dv, dsa, ak, av


@pytest.mark.parametrize("dkdv", ["rule", "asm"], indirect=True)     # (so that one cached oracle serves both)
@pytest.mark.parametrize("i", range(len(P.VARLEN_CASES)))
def test_packed_mask_edges(i, dkdv):
    """cu_seqlens inside the grid: besides the edges of each sequence's own mask, rows of later sequences aim at the last
    key of the PREVIOUS sequence and at the pack's first num_sink keys (one index away / the sink tiles every block reads)"""
    from sink_attention.varlen import sink_flash_attention_varlen
    c = P.VARLEN_CASES[i]
    cu = c["cu"]
    pr, o_r, dq_r, dk_r, dv_r, dsa_r, ak_r, av_r = _pack(i)
    qd, kd, vd = (pr[x].to(DEV).requires_grad_(True) for x in "qkv")
    sad = pr["s_aux"].to(DEV).requires_grad_(True)
    out = sink_flash_attention_varlen(qd, kd, vd, cu, num_sink=c["ns"], window_size=c["W"], s_aux=sad)
    assert _path().startswith("fwd_mfma"), _path()
    out.backward(pr["do"].to(DEV))
    longest = max(b - a for a, b in zip(cu[:-1], cu[1:]))
    want = dkdv_kernel_name(dkdv, len(cu) - 1, c["Hkv"], longest, longest, c["D"], c["W"], packed=True, ns=c["ns"])
    assert want in _path(), (want, _path())
    # O, dQ, ds_aux: the tolerances of tests/test_gpu_varlen.py::test_varlen_native_kernels_one_launch.  dK / dV: that test's
    # absolute 1.5e-1 is sized for randn gradients of a few units; here the keys many rows aim at (the sinks) collect max |dK|
    # of 86 - 152 on packs 0, 2, 6, 7, where one bf16 rounding of the RESULT is 0.25 - 0.5.  Where 1.5e-1 is below that, the
    # bound is the exact-f32 kernel's own error on the same pack (force_generic, sequence by sequence, bf16 result) plus one
    # rounding of the reference, 2^-8 max |ref|; never the MFMA kernel's error.  Measured max |dK - ref| (MFMA / exact-f32 /
    # bound; max |dK ref|): pack 0 0.44 / 0.29 / 0.71 (107), pack 2 0.23 / 0.23 / 0.57 (87), pack 6 0.34 / 0.30 / 0.80 (127),
    # pack 7 0.44 / 0.44 / 1.01 (145); dV: at most 0.20 / 0.20 / 0.51.  The other packs stay at 1.5e-1 or within 0.05 of it.
    e32 = _pack_f32_error(i, pr, dk_r, dv_r)
    errs = {x: maxdiff(a, b) for x, a, b in (("o", out, o_r), ("dq", qd.grad, dq_r), ("dk", kd.grad, dk_r), ("dv", vd.grad, dv_r))}
    tol = {x: max(1.5e-1, e32[x] + 2.0 ** -8 * r.abs().max().item()) for x, r in (("dk", dk_r), ("dv", dv_r))}
    print("pack", i, dkdv, _path(), "mfma", errs, "f32", e32, "tol", tol, "max|dk|", dk_r.abs().max().item(), "max|dv|",
          dv_r.abs().max().item())
    assert errs["o"] < 2e-2 and errs["dq"] < 1.5e-1, errs
    assert errs["dk"] < tol["dk"] and errs["dv"] < tol["dv"], (errs, tol)
    u = UNIT_ROUNDOFF[torch.bfloat16]
    print(f"sum bound pack {i} {dkdv}: dK {sum_bound_ratio(kd.grad, dk_r, ak_r, u):.3f} dV {sum_bound_ratio(vd.grad, dv_r, av_r, u):.3f}")
    assert_within_sum_bound(kd.grad, dk_r, ak_r, u, "dk")
    assert_within_sum_bound(vd.grad, dv_r, av_r, u, "dv")
    assert maxdiff(sad.grad, dsa_r) < 1.5


_F32_ERR = {}


def _pack_f32_error(i, pr, dk_r, dv_r):
    """max |dK - ref|, max |dV - ref| of the exact-f32 kernels (bf16 in, f32 math, bf16 out) on pack i, each sequence alone"""
    if i not in _F32_ERR:
        c = P.VARLEN_CASES[i]
        dk, dv = torch.zeros_like(dk_r), torch.zeros_like(dv_r)
        for a, b in zip(c["cu"][:-1], c["cu"][1:]):
            if b == a:
                continue
            q, k, v = (pr[x][:, :, a:b].to(DEV).requires_grad_(True) for x in "qkv")
            sa = pr["s_aux"].to(DEV).requires_grad_(True)
            _ex()(q, k, v, c["ns"], c["W"], s_aux=sa, force_generic=True).backward(pr["do"][:, :, a:b].to(DEV))
            assert "generic" in _path(), _path()
            dk[:, :, a:b], dv[:, :, a:b] = k.grad.double().cpu(), v.grad.double().cpu()
        _F32_ERR[i] = {"dk": maxdiff(dk, dk_r), "dv": maxdiff(dv, dv_r)}
    return _F32_ERR[i]


# ------------------------------------------------------------------------------------------------ ring: multi-token calls
def _full_ring(k, v, ns, W, total):
    from sink_attention import SinkCacheLayer
    layer = SinkCacheLayer(ns, W)
    layer.append(k[:, :, :ns + W].to(DEV), v[:, :, :ns + W].to(DEV))
    layer.append(k[:, :, ns + W:total].to(DEV), v[:, :, ns + W:total].to(DEV))
    assert layer.window_len == W and layer.write_pos == (total - ns - W) % W
    return layer


@pytest.mark.parametrize("dt,B,Hq,Hkv,D,ns,W,extra,n", P.CHUNK_CASES)
def test_ring_chunk_mask_edges(dt, B, Hq, Hkv, D, ns, W, extra, n):
    """ring full and wrapped (the chunk's commit wraps past slot 0 where extra + n > W): chunk rows aim at the oldest key they
    still see, at the key they have just lost (still in the ring: extend_attention commits nothing), at the chunk's later
    token and at the sink edge"""
    dtype, total = DT[dt], ns + W + extra
    pr = P.chunk_case_probe((dt, B, Hq, Hkv, D, ns, W, extra, n))
    layer = _full_ring(pr["k"], pr["v"], ns, W, total)
    qc, kc, vc = (pr[x][:, :, total:].to(DEV) for x in "qkv")
    sad = pr["s_aux"].to(DEV)
    out = layer.extend_attention(qc, kc, vc, s_aux=sad)
    assert _path().startswith(_expected_path(dtype, D)), _path()
    o64 = _oracle_rows(pr["q"], pr["k"], pr["v"], pr["s_aux"], total, ns, W, n, slice(None))
    assert maxdiff(out, o64) < TOL[dtype], ("oracle", maxdiff(out, o64))
    out2 = layer.extend_step(qc, kc, vc, s_aux=sad)
    assert _path().startswith(_expected_path(dtype, D)) and _path().endswith("_commit"), _path()
    assert torch.equal(out2, out)
    assert layer.write_pos == (extra + n) % W and layer.window_len == W


# ------------------------------------------------------------------------------------------------ trees
@pytest.mark.parametrize("dt,D", P.TREE_DTYPE_D)
def test_tree_mask_edges(dt, D):
    """nodes aim at themselves, their parent, a SIBLING, a non-ancestor of lower depth, the oldest ring key their depth still
    sees and the one it has lost"""
    from sink_attention import SinkCacheLayer
    dtype, (B, Hq, Hkv) = DT[dt], P.TREE_SHAPE
    for i, (ns, W, prefill, appends, n, shape, forest) in enumerate(TREES + P.TREE_CASES_EXTRA):
        parent = random_tree(random.Random(P.TREE_RNG_SEED + i), n, forest, shape)
        total = prefill + appends
        tp = P.tree_case_probe(i, (ns, W, prefill, appends, n, shape, forest), parent, dt, D)
        host, dyn = SinkCacheLayer(ns, W), SinkCacheLayer(ns, W)
        for c in (host, dyn):
            c.append(tp["k"][:, :, :prefill].to(DEV), tp["v"][:, :, :prefill].to(DEV))
            for t in range(prefill, total):
                c.append(tp["k"][:, :, t:t + 1].to(DEV), tp["v"][:, :, t:t + 1].to(DEV))
        dyn.enable_device_state()
        qc, kc, vc = (tp[x][:, :, total:].to(DEV) for x in "qkv")
        sad = tp["s_aux"].to(DEV)
        out = host.extend_attention_tree(qc, kc, vc, parent, s_aux=sad)
        assert _path().startswith(_tree_path_name(dtype, D)) and "_dyn" not in _path(), _path()
        o64 = _oracle_tree(tp["q"], tp["k"], tp["v"], tp["s_aux"], total, host.sink_len, W, parent)
        assert maxdiff(out, o64) < TOL[dtype], (i, maxdiff(out, o64))
        outd = dyn.extend_attention_tree_dyn(qc, kc, vc, torch.tensor(parent, device=DEV), s_aux=sad)
        assert _path().startswith(_tree_path_name(dtype, D)) and _path().endswith("_dyn"), _path()
        assert torch.equal(outd, out), i


# ------------------------------------------------------------------------------------------------ per-sequence state
def test_ragged_rows_mask_edges():
    """one ragged batch of three fill levels (ring partly filled, filled by the chunk's 4th token, full and wrapped), kinds drawn per
    sequence: the _rows kernels read every sequence's own window_len / write_pos"""
    from sink_attention import SinkCacheLayer
    c = P.RAGGED_CASE
    ns, W, n, Hq, Hkv, D, dtype = c["ns"], c["W"], c["n"], c["Hq"], c["Hkv"], c["D"], DT[c["dtype"]]
    prs = P.ragged_case_probes()
    sa = prs[0]["s_aux"]
    cu = [0]
    for L in c["lengths"]:
        cu.append(cu[-1] + L)
    layer = SinkCacheLayer(ns, W)
    layer.prefill_varlen(torch.cat([p["k"][:, :, :L] for p, L in zip(prs, c["lengths"])], dim=2).to(DEV),
                         torch.cat([p["v"][:, :, :L] for p, L in zip(prs, c["lengths"])], dim=2).to(DEV),
                         torch.tensor(cu, dtype=torch.int32, device=DEV))
    q, k, v = (torch.cat([p[x][:, :, L:] for p, L in zip(prs, c["lengths"])], dim=0).to(DEV) for x in "qkv")
    out = layer.extend_attention_dyn(q, k, v, s_aux=sa.to(DEV))
    assert _path().startswith(_expected_path(dtype, D)) and "_rows" in _path(), _path()
    for b, (p, L) in enumerate(zip(prs, c["lengths"])):
        o64 = _oracle_rows(p["q"], p["k"], p["v"], sa, L, ns, W, n, slice(None))
        assert maxdiff(out[b:b + 1], o64) < TOL[dtype], (b, maxdiff(out[b:b + 1], o64))
