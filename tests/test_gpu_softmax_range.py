"""GPU parity on softmax-range inputs (tests/range_inputs.py): the product ops against the fp64 oracle of the same rounded
inputs, on logits that climb, fall or sit far from zero along the key index.  The randn parity tests run every MFMA forward
with alpha == 1 from the first tile to the last (the deferred-rescale rule never fires on them); here the out-of-line
rescale of the hand-placed bodies, the between-blocks rescale of the strip bodies and the inline one of the compiled
kernels run with 2^-16 <= alpha < 2^-8 in every 64-row wave, beside rows of the same wave that keep alpha = 1.
tests/test_range_inputs.py proves on the CPU that these inputs do that, that a kernel with a wrong alpha misses the O
tolerance tenfold, and that a correct kernel of the dtype stays within half of every tolerance used here:
  O        tests/test_gpu_prefill.py::test_shapes_fwd_bwd per dtype: max |error| < 2e-2 (bf16) / 4e-3 (fp16) / 2e-5 (fp32)
  dQ/dK/dV that test's 1.5e-1 / 3e-2 / 2e-4, scaled by max(1, max |reference|) as the neighbouring tests scale theirs;
           ds_aux: ten times that (as there)
  LSE      5e-3 (tests/test_asm_emu.py), read from the autograd node's saved tensors, natural-log units
  decode   tests/util.py::DECODE_TOL
Every case asserts the kernel it ran and that two forwards agree bit for bit."""
import functools
import re

import pytest
import torch

import range_inputs as R
from oracle import sink_oracle as O
from util import DECODE_TOL, chunk_oracle_rows, dkdv_kernel_name, maxdiff, per_seq_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _path():
    from sink_attention import _native
    return _native.last_path()


def _ex():
    from sink_attention.sink_flash_attention import _sink_flash_attention_ex
    return _sink_flash_attention_ex


def _check(dt, out, lse, grads, sa_grad, o_r, lse_r, g_r, what):
    """print every figure, then assert"""
    dq_r, dk_r, dv_r, dsa_r = g_r
    fig = {"o": (maxdiff(out, o_r), R.TOL_O[dt])}
    fin = torch.isfinite(lse_r)
    fig["lse"] = (maxdiff(lse.cpu()[fin], lse_r[fin]), R.TOL_LSE)
    for name, got, ref in zip(("dq", "dk", "dv"), grads, (dq_r, dk_r, dv_r)):
        fig[name] = (maxdiff(got, ref), R.grad_tol(dt, ref))
    fig["ds_aux"] = (maxdiff(sa_grad, dsa_r), R.grad_tol(dt, dsa_r, aux=True))
    print(what, {k: "%.3g / %.3g" % v for k, v in fig.items()})
    bad = {k: v for k, v in fig.items() if not v[0] < v[1]}
    assert not bad, (what, bad)


# ------------------------------------------------------------------------------------------------ dense calls
@functools.lru_cache(maxsize=1)
def _dense(case_id):
    """inputs and fp64 oracle of one case (shared by the two dK/dV modes)"""
    case = next(c for c in R.DENSE_CASES if c["id"] == case_id)
    B, Hq, Hkv, Nq, Nk, D, ns, W = case["shape"]
    inp = R.case_inputs(case)
    o_r, lse_r = O.sink_attention_dense(inp["q"], inp["k"], inp["v"], ns, W, inp["s_aux"])
    g_r = O.sink_attention_bwd_dense(inp["q"], inp["k"], inp["v"], inp["do"], ns, W, inp["s_aux"])
    return inp, o_r, lse_r, g_r


@pytest.mark.parametrize("dkdv", ["rule", "asm"], indirect=True)     # the fixture's two modes, run back to back per case
@pytest.mark.parametrize("case", R.DENSE_CASES, ids=[c["id"] for c in R.DENSE_CASES])
def test_dense_softmax_range(case, dkdv):
    B, Hq, Hkv, Nq, Nk, D, ns, W = case["shape"]
    dt = R.DT[case["dtype"]]
    inp, o_r, lse_r, g_r = _dense(case["id"])
    generic = case.get("generic", False)
    qd, kd, vd = (inp[x].to(DEV).requires_grad_(True) for x in "qkv")
    sad = inp["s_aux"].to(DEV).requires_grad_(True)
    out = _ex()(qd, kd, vd, ns, W, s_aux=sad, force_generic=generic)
    fwd_path = _path()
    assert case["fwd"] in fwd_path, fwd_path
    lse = out.grad_fn.saved_tensors[4]
    assert lse.shape == (B, Hq, Nq) and lse.dtype == torch.float32
    with torch.no_grad():
        again = _ex()(qd, kd, vd, ns, W, s_aux=sad, force_generic=generic)
    assert _path() == fwd_path
    assert torch.equal(again, out.detach()), "two forwards differ"
    out.backward(inp["do"].to(DEV))
    bwd_path = _path()
    assert case["dq"] in bwd_path, bwd_path
    want = None if generic else dkdv_kernel_name(dkdv, B, Hkv, Nq, Nk, D, W, dtype=dt, ns=ns)
    assert want is None or want in bwd_path, (want, bwd_path)
    _check(dt, out, lse, (qd.grad, kd.grad, vd.grad), sad.grad, o_r, lse_r, g_r, f"{case['id']} {dkdv} {fwd_path} | {bwd_path}")


# ------------------------------------------------------------------------------------------------ one packed batch
@functools.lru_cache(maxsize=1)
def _pack():
    c = R.PACK_CASE
    inp = R.pack_inputs()
    o_r, dq_r, dk_r, dv_r, dsa_r = per_seq_oracle(inp["q"], inp["k"], inp["v"], inp["do"], c["cu"], c["ns"], c["W"], inp["s_aux"])
    lse_r = torch.cat([O.sink_attention_dense(inp["q"][:, :, a:b], inp["k"][:, :, a:b], inp["v"][:, :, a:b], c["ns"], c["W"],
                                              inp["s_aux"])[1] for a, b in zip(c["cu"][:-1], c["cu"][1:])], dim=2)
    return inp, o_r, lse_r, (dq_r, dk_r, dv_r, dsa_r)


def test_packed_softmax_range(dkdv):
    """cu_seqlens inside the grid: the second and third sequence carry the staircase (tiles count from each sequence's own
    first key), the first is randn; against the per-sequence oracle"""
    from sink_attention.varlen import sink_flash_attention_varlen
    c = R.PACK_CASE
    dt = R.DT[c["dtype"]]
    inp, o_r, lse_r, g_r = _pack()
    qd, kd, vd = (inp[x].to(DEV).requires_grad_(True) for x in "qkv")
    sad = inp["s_aux"].to(DEV).requires_grad_(True)
    out = sink_flash_attention_varlen(qd, kd, vd, c["cu"], num_sink=c["ns"], window_size=c["W"], s_aux=sad)
    fwd_path = _path()
    assert "asm4x64pk" in fwd_path, fwd_path
    lse = out.grad_fn.saved_tensors[4]                       # [H_q, T]
    assert lse.shape == (c["Hq"], c["cu"][-1])
    with torch.no_grad():
        again = sink_flash_attention_varlen(qd, kd, vd, c["cu"], num_sink=c["ns"], window_size=c["W"], s_aux=sad)
    assert torch.equal(again, out.detach())
    out.backward(inp["do"].to(DEV))
    longest = max(b - a for a, b in zip(c["cu"][:-1], c["cu"][1:]))
    want = dkdv_kernel_name(dkdv, len(c["cu"]) - 1, c["Hkv"], longest, longest, c["D"], c["W"], packed=True, ns=c["ns"])
    assert want in _path(), (want, _path())
    _check(dt, out, lse.unsqueeze(0), (qd.grad, kd.grad, vd.grad), sad.grad, o_r, lse_r, g_r, f"pack {dkdv} {fwd_path} | {_path()}")


# ------------------------------------------------------------------------------------------------ decode, multi-token
@pytest.mark.parametrize("cid,dtn,Hq,Hkv,D,family", R.DECODE_CASES, ids=[c[0] for c in R.DECODE_CASES])
def test_decode_softmax_range(cid, dtn, Hq, Hkv, D, family):
    """one query over DECODE_NKV keys in several splits: a level per 256 keys, so that the maximum of a late split lies more
    than 100 log2 units below the first split's (and, on the heads of gain -1, above it); s_aux from -40 to +40 nat"""
    from sink_attention import sink_decode_attention
    dt = R.DT[dtn]
    inp = R.history_range(family, 2, Hq, Hkv, D, R.DECODE_NKV, 1, dt, 7600 + len(cid))
    q, k, v, sa = inp["q"], inp["k"], inp["v"], inp["s_aux"]
    out = sink_decode_attention(q.to(DEV), k.to(DEV), v.to(DEV), s_aux=sa.to(DEV))
    path = _path()
    splits = int(re.search(r"_s(\d+)$", path).group(1))
    assert path.startswith("decode_splitkv") and splits > 1, path
    assert torch.equal(sink_decode_attention(q.to(DEV), k.to(DEV), v.to(DEV), s_aux=sa.to(DEV)), out)
    err = maxdiff(out, O.decode_dense(q, k, v, sa))
    print(cid, path, "max |error| %.3g / %.3g" % (err, DECODE_TOL[dt]))
    assert err < DECODE_TOL[dt], (path, err)


@pytest.mark.parametrize("cid,dtn,Hq,Hkv,D,family", R.CHUNK_CASES, ids=[c[0] for c in R.CHUNK_CASES])
def test_ring_multi_softmax_range(cid, dtn, Hq, Hkv, D, family):
    """sink_decode_attention_ring_multi (through the cache layer) with n = 5 over a full, wrapped ring: the sinks hold the
    staircase's top level, the ring the levels far below; MFMA path and exact-f32 path"""
    from sink_attention import SinkCacheLayer
    dt = R.DT[dtn]
    ns, W, extra, n = R.CHUNK_RING
    total = ns + W + extra
    inp = R.history_range(family, 2, Hq, Hkv, D, total + n, n, dt, 7700 + len(cid), step=128)
    k, v, sa = inp["k"], inp["v"], inp["s_aux"]
    q = torch.cat([torch.zeros(2, Hq, total, D, dtype=dt), inp["q"]], dim=2)
    layer = SinkCacheLayer(ns, W)
    layer.append(k[:, :, :ns + W].to(DEV), v[:, :, :ns + W].to(DEV))
    layer.append(k[:, :, ns + W:total].to(DEV), v[:, :, ns + W:total].to(DEV))
    assert layer.window_len == W and layer.write_pos == extra % W
    qc, kc, vc = (x[:, :, total:].to(DEV) for x in (q, k, v))
    out = layer.extend_attention(qc, kc, vc, s_aux=sa.to(DEV))
    path = _path()
    want = "decode_multi_f32_" if dt == torch.float32 else "decode_multi_mfma_" + {"bf16": "bf16", "fp16": "f16"}[dtn] + f"_d{D}"
    assert path.startswith(want), path
    assert torch.equal(layer.extend_attention(qc, kc, vc, s_aux=sa.to(DEV)), out)
    err = maxdiff(out, chunk_oracle_rows(q, k, v, sa, total, ns, W, n, slice(None)))
    print(cid, path, "max |error| %.3g / %.3g" % (err, DECODE_TOL[dt]))
    assert err < DECODE_TOL[dt], (path, err)
