"""GPU: the same call twice - on ordinary contiguous tensors ("near") and on views of one large arena whose strides put
the operands past 2^31 elements, 2^31 bytes or 2^32 bytes ("far", tests/far_views.py).  Every case asserts

  (a) the near result against the fp64 oracle at the suite's tolerances (bf16 / fp16: O 2e-2, gradients 1.5e-1; fp32:
      2e-5 / 2e-4; decode: TOL of tests/test_gpu_decode_multi.py),
  (b) far == near bitwise, for every output,
  (c) the same sfa_last_path() in both runs - or, where the library documents another kernel for the far layout (the
      generic path behind slice_ok(), or SFA_ERR_UNSUPPORTED with nothing written), exactly that,
  (d) the rest of the arena still holds its sentinel: no store landed at a truncated address.

The problems are small; only their addresses are large.  One arena per module (4.1 GiB), every case re-fills it.
The last section runs the serving pool (packed step forms, packed commit, fork; the FP8 pool; the paged pool)."""
import functools
import math

import pytest
import torch

import far_views as F
import probe_inputs as P
from oracle import sink_oracle as O
from util import DECODE_TOL as TOL
from util import assert_close, chunk_oracle_rows, dkdv_kernel_name, maxdiff, oracle_bwd, oracle_fwd, per_seq_oracle, rand

pytestmark = pytest.mark.gpu
DEV = "cuda"
ARENA_I16 = (1 << 31) + (1 << 26)          # int16 elements: 4 GiB + 128 MiB, viewed in each case's dtype
UNSUPPORTED = -2                           # SFA_ERR_UNSUPPORTED of include/sfa.h


@pytest.fixture(scope="module")
def arena16():
    need = ARENA_I16 * 2
    free, total = torch.cuda.mem_get_info()
    if free < need + (2 << 30):
        pytest.skip(f"far-offset arena needs {need / 2**30:.2f} + 2 GiB free, the device reports {free / 2**30:.2f} "
                    f"of {total / 2**30:.2f} GiB")
    assert need <= F.ARENA_LIMIT_BYTES
    a = torch.empty(ARENA_I16, dtype=torch.int16, device=DEV)
    yield a
    del a
    torch.cuda.empty_cache()


def _arena(arena16, dtype, sentinel=F.SENTINEL16):
    a = arena16.view(dtype)
    F.fill_sentinel(a, sentinel)
    return a


def _nat():
    from sink_attention import _native
    return _native


def _stream():
    return _nat().stream_ptr(torch.device(DEV))


# ------------------------------------------------------------------------------------------- dense / packed prefill
def _run_prefill(t, ns, W, sa, cu=None, flags=0):
    """sfa_fwd + sfa_bwd (or the packed pair) through the C ABI on the operands of dict t (q k v o do dq dk dv); lse, the
    workspace and ds_aux are ordinary allocations (raw pointers of the ABI).  Returns status, paths and ds_aux."""
    N = _nat()
    lib = N.lib()
    B, Hq, Nq, D = t["q"].shape
    Hkv = t["k"].shape[1]
    scale = 1.0 / math.sqrt(D)
    lse = torch.zeros(B, Hq, Nq, dtype=torch.float32, device=DEV)
    sap = sa.data_ptr() if sa is not None else None
    d = {x: N.desc(t[x]) for x in t}
    r = dict(lse=lse, fwd_path=None, bwd_path=None, dsa=None, rc_bwd=None)
    if cu is not None:
        cud = torch.tensor(cu, dtype=torch.int32, device=DEV)
        longest = max(b - a for a, b in zip(cu[:-1], cu[1:]))
        r["rc_fwd"] = lib.sfa_fwd_varlen(d["q"], d["k"], d["v"], d["o"], lse.data_ptr(), sap, cud.data_ptr(), len(cu) - 1,
                                         longest, ns, W, scale, flags, _stream())
    else:
        r["rc_fwd"] = lib.sfa_fwd(d["q"], d["k"], d["v"], d["o"], lse.data_ptr(), sap, ns, W, scale, flags, _stream())
    r["err_fwd"] = lib.sfa_last_error().decode()
    if r["rc_fwd"] != 0 or "do" not in t:
        if r["rc_fwd"] == 0:
            r["fwd_path"] = N.last_path()
        return r
    r["fwd_path"] = N.last_path()
    bflags = N.bwd_flags(flags)
    ws = torch.empty(max(int(lib.sfa_bwd_workspace_bytes(B, Hq, Hkv, Nq, D, N.SFA_DTYPE[t["q"].dtype], ns, W, bflags)), 256),
                     dtype=torch.uint8, device=DEV)
    dsa = torch.zeros(Hq, dtype=torch.float32, device=DEV) if sa is not None else None
    dsap = dsa.data_ptr() if sa is not None else None
    if cu is not None:
        r["rc_bwd"] = lib.sfa_bwd_varlen(d["q"], d["k"], d["v"], d["o"], d["do"], lse.data_ptr(), sap, d["dq"], d["dk"],
                                         d["dv"], dsap, cud.data_ptr(), len(cu) - 1, longest, ws.data_ptr(), ws.numel(),
                                         ns, W, scale, bflags, _stream())
    else:
        r["rc_bwd"] = lib.sfa_bwd(d["q"], d["k"], d["v"], d["o"], d["do"], lse.data_ptr(), sap, d["dq"], d["dk"], d["dv"],
                                  dsap, ws.data_ptr(), ws.numel(), ns, W, scale, bflags, _stream())
    r["err_bwd"] = lib.sfa_last_error().decode()
    if r["rc_bwd"] == 0:
        r["bwd_path"] = N.last_path()
    r["dsa"] = dsa
    torch.cuda.synchronize()
    return r


OUTS = ("o", "dq", "dk", "dv")


def _near_operands(inp, bwd=True):
    t = {x: inp[x].to(DEV) for x in (("q", "k", "v", "do") if bwd else ("q", "k", "v"))}
    t["o"] = torch.empty_like(t["q"])
    if bwd:
        t["dq"], t["dk"], t["dv"] = torch.empty_like(t["q"]), torch.empty_like(t["k"]), torch.empty_like(t["v"])
    return t


def _far_operands(arena, geom, inp, bwd=True):
    names = ("q", "k", "v", "o", "do", "dq", "dk", "dv") if bwd else ("q", "k", "v", "o")
    src = dict(q=inp["q"], k=inp["k"], v=inp["v"], do=inp.get("do"))
    shape_of = dict(o="q", dq="q", dk="k", dv="v")
    ops = [src[x].to(DEV) if x in src else tuple(inp[shape_of[x]].shape) for x in names]
    return dict(zip(names, F.views(arena, geom, ops)))


@functools.lru_cache(maxsize=2)
def _inputs(dt, B, Hq, Hkv, Nq, Nk, D, ns, W, aux, probe=False, cu=None):
    """CPU inputs and fp64 oracle of one case, shared by its dK/dV modes and geometries."""
    dtype = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[dt]
    if probe:
        pr = P.dense_probe(B, Hq, Hkv, Nq, Nk, D, ns, W, dtype, 7100, aux=aux)
        inp = {x: pr[x] for x in ("q", "k", "v", "do")}
        sa = pr["s_aux"]
    else:
        g = torch.Generator().manual_seed(7000 + D + Nq)
        inp = dict(q=rand((B, Hq, Nq, D), g, dtype), k=rand((B, Hkv, Nk, D), g, dtype), v=rand((B, Hkv, Nk, D), g, dtype),
                   do=rand((B, Hq, Nq, D), g, dtype))
        sa = rand((Hq,), g, torch.float32, 0.5) if aux else None
    if cu is not None:
        o_r, dq_r, dk_r, dv_r, _ = per_seq_oracle(inp["q"], inp["k"], inp["v"], inp["do"], list(cu), ns, W, sa)
        return inp, sa, dict(o=o_r, dq=dq_r, dk=dk_r, dv=dv_r)
    banded = Nq == Nk and Nq > 1024
    o_r, _ = oracle_fwd(inp["q"], inp["k"], inp["v"], ns, W, sa, banded=banded)
    dq_r, dk_r, dv_r, _ = oracle_bwd(inp["q"], inp["k"], inp["v"], inp["do"], ns, W, sa, banded=banded)
    return inp, sa, dict(o=o_r, dq=dq_r, dk=dk_r, dv=dv_r)


def _check_oracle(t, ref, dtype, what, probe=False, outs=OUTS):
    if probe:            # the tolerances of tests/test_gpu_mask_edges.py::test_dense_mask_edges (bf16)
        assert_close(t["o"], ref["o"], 2e-2, 2e-2, what + " o")
        assert_close(t["dq"], ref["dq"], 5e-2, 5e-2, what + " dq")
        for x in ("dk", "dv"):
            assert_close(t[x], ref[x], 5e-2 * max(1.0, ref[x].abs().max().item()), 5e-2, what + " " + x)
        return
    to, tg = (2e-5, 2e-4) if dtype == torch.float32 else (2e-2, 1.5e-1)
    errs = {x: maxdiff(t[x], ref[x]) for x in outs}
    print(what, "errors against the oracle", errs)
    for x in outs:
        assert errs[x] < (to if x == "o" else tg), (what, x, errs)


def _twin(arena16, geom, case, mode="same", bwd=True, cu=None, far_fwd=None, far_bwd=None, dkdv=None, probe=False):
    """mode "same": far must run the near kernels and match bitwise.  "generic": the far layout is outside the MFMA
    paths' strides, the library takes fwd_generic / bwd_generic (named in far_fwd / far_bwd) and must match the oracle.
    (Calls that have no generic form: _refusal.)"""
    dt, B, Hq, Hkv, Nq, Nk, D, ns, W, aux = case
    inp, sa, ref = _inputs(dt, B, Hq, Hkv, Nq, Nk, D, ns, W, aux, probe, None if cu is None else tuple(cu))
    dtype = inp["q"].dtype
    outs = OUTS if bwd else ("o",)
    sad = sa.to(DEV) if sa is not None else None
    near = _near_operands(inp, bwd)
    rn = _run_prefill(near, ns, W, sad, cu)
    assert rn["rc_fwd"] == 0 and (not bwd or rn["rc_bwd"] == 0), rn
    if dkdv is not None and bwd:
        nb = len(cu) - 1 if cu is not None else B
        longest = max(b - a for a, b in zip(cu[:-1], cu[1:])) if cu is not None else None
        want = dkdv_kernel_name(dkdv, nb, Hkv, longest or Nq, longest or Nk, D, W, packed=cu is not None, dtype=dtype, ns=ns)
        assert want is None or want in rn["bwd_path"], (want, rn["bwd_path"])
    _check_oracle(near, ref, dtype, "near", probe, outs)                                        # (a)
    arena = _arena(arena16, dtype)
    far = _far_operands(arena, geom, inp, bwd)
    rf = _run_prefill(far, ns, W, sad, cu)
    print(geom.name, case, "near", rn["fwd_path"], "|", rn["bwd_path"], "far", rf["rc_fwd"], rf["fwd_path"], "|",
          rf["rc_bwd"], rf["bwd_path"])
    assert rf["rc_fwd"] == 0 and (not bwd or rf["rc_bwd"] == 0), rf
    if mode == "same":
        assert rf["fwd_path"] == rn["fwd_path"] and rf["bwd_path"] == rn["bwd_path"], (rn, rf)   # (c)
        for x in outs:
            assert torch.equal(far[x], near[x]), f"far {x} differs from near: max {maxdiff(far[x], near[x]):.3e}"   # (b)
        assert torch.equal(rf["lse"], rn["lse"])
    else:
        assert rn["fwd_path"].startswith("fwd_mfma") and rf["fwd_path"] == far_fwd, (rn["fwd_path"], rf["fwd_path"])
        assert not bwd or ("generic" not in rn["bwd_path"] and rf["bwd_path"] == far_bwd), (rn["bwd_path"], rf["bwd_path"])
        _check_oracle(far, ref, dtype, "far", probe, outs)
    if sad is not None and bwd and mode == "same":
        assert torch.equal(rf["dsa"], rn["dsa"])
    F.assert_untouched(arena, list(far.values()), f"{geom.name} {case}",                    # (d)
                       inputs=[(far[x], near[x]) for x in (("q", "k", "v", "do") if bwd else ("q", "k", "v"))])


def _refusal(arena16, geom, B, Hq, Hkv, Nq, Nk, D, cu, aux, fwd_refused, msg):
    """A layout outside the MFMA paths' strides on a call that has no generic form (packed, or N_q != N_kv): the
    forward (where fwd_refused - a stride over the backward's rule only still serves the forward) and the backward
    return SFA_ERR_UNSUPPORTED with a message that names the limit, and have written NOTHING when they return: o, lse,
    dq, dk, dv, ds_aux, the workspace, the inputs and the rest of the arena are as they were."""
    N = _nat()
    lib = N.lib()
    dtype = torch.bfloat16
    g = torch.Generator().manual_seed(7600 + D + Nk)
    src = dict(q=rand((B, Hq, Nq, D), g, dtype), k=rand((B, Hkv, Nk, D), g, dtype), v=rand((B, Hkv, Nk, D), g, dtype),
               do=rand((B, Hq, Nq, D), g, dtype))
    src = {x: t.to(DEV) for x, t in src.items()}
    sad = rand((Hq,), g, torch.float32, 0.5).to(DEV) if aux else None
    arena = _arena(arena16, dtype)
    far = _far_operands(arena, geom, src)
    ns, W, scale = 2, 128, 1.0 / math.sqrt(D)
    lse = torch.full((B, Hq, Nq), 7.0, dtype=torch.float32, device=DEV)
    cud = torch.tensor(cu, dtype=torch.int32, device=DEV) if cu is not None else None
    longest = max(b - a for a, b in zip(cu[:-1], cu[1:])) if cu is not None else None
    d = {x: N.desc(far[x]) for x in far}
    sap = sad.data_ptr() if aux else None
    if cu is not None:
        rc = lib.sfa_fwd_varlen(d["q"], d["k"], d["v"], d["o"], lse.data_ptr(), sap, cud.data_ptr(), len(cu) - 1, longest,
                                ns, W, scale, 0, _stream())
    else:
        rc = lib.sfa_fwd(d["q"], d["k"], d["v"], d["o"], lse.data_ptr(), sap, ns, W, scale, 0, _stream())
    torch.cuda.synchronize()
    if fwd_refused:
        assert rc == UNSUPPORTED and msg in lib.sfa_last_error().decode(), (rc, lib.sfa_last_error())
        for x in OUTS:                               # straight after the refused forward, before anything is put into o
            assert F.is_sentinel(far[x]), f"{x} was written by a forward that returned SFA_ERR_UNSUPPORTED"
        assert bool((lse == 7.0).all()), "lse was written by a refused forward"
        far["o"].copy_(src["q"])                     # the backward reads an O: any values will do for a call that must refuse
    else:
        assert rc == 0 and N.last_path().startswith("fwd_mfma"), (rc, lib.sfa_last_error(), N.last_path())
    o_in = far["o"].clone()
    bflags = N.bwd_flags()
    ws = torch.full((max(int(lib.sfa_bwd_workspace_bytes(1 if cu is not None else B, Hq, Hkv, Nq, D, N.SFA_DTYPE[dtype], ns, W,
                                                          bflags)), 256),), 0xA5, dtype=torch.uint8, device=DEV)
    dsa = torch.full((Hq,), 123.0, dtype=torch.float32, device=DEV) if aux else None
    args = (d["q"], d["k"], d["v"], d["o"], d["do"], lse.data_ptr(), sap, d["dq"], d["dk"], d["dv"], dsa.data_ptr() if aux else None)
    if cu is not None:
        rc = lib.sfa_bwd_varlen(*args, cud.data_ptr(), len(cu) - 1, longest, ws.data_ptr(), ws.numel(), ns, W, scale, bflags,
                                _stream())
    else:
        rc = lib.sfa_bwd(*args, ws.data_ptr(), ws.numel(), ns, W, scale, bflags, _stream())
    torch.cuda.synchronize()
    assert rc == UNSUPPORTED and msg in lib.sfa_last_error().decode(), (rc, lib.sfa_last_error())
    for x in ("dq", "dk", "dv"):
        assert F.is_sentinel(far[x]), f"{x} was written by a backward that returned SFA_ERR_UNSUPPORTED"
    assert torch.equal(far["o"], o_in)
    assert bool((ws == 0xA5).all()), "the workspace was written by a refused backward"
    assert dsa is None or bool((dsa == 123.0).all()), "ds_aux was written by a refused backward"
    F.assert_untouched(arena, list(far.values()), f"{geom.name} refusal", inputs=[(far[x], src[x]) for x in src])


#              dtype  B Hq Hkv  Nq   Nk    D  ns   W  s_aux
DENSE = [("bf16", 2, 4, 2, 512, 512, 128, 4, 200, True),        # hand-placed work-list kernels
         ("fp16", 2, 4, 2, 640, 640, 64, 0, 128, False),        # strip kernels + the skewed dK/dV sweep
         ("bf16", 2, 4, 2, 520, 520, 80, 2, 300, False),
         ("bf16", 2, 4, 2, 512, 512, 256, 0, 300, False),       # compiled kernels
         ("fp32", 2, 4, 2, 512, 512, 48, 2, 100, True),         # generic
         ("bf16", 2, 4, 2, 256, 768, 128, 4, 200, False)]       # N_q < N_kv


@pytest.mark.parametrize("case", DENSE, ids=[f"{c[0]}-d{c[6]}-nq{c[4]}-nk{c[5]}" for c in DENSE])
def test_dense_far_batch(arena16, case, dkdv):
    """All eight operands behind a batch stride of 4 GiB: batch 1 starts at element 2^31 (fp32: 2^30)."""
    _twin(arena16, F.far_batch, case, dkdv=dkdv)


def test_dense_far_batch_probe_inputs(arena16, dkdv):
    """... on mask-edge probe inputs: a base address that lands on other plausible data cannot pass."""
    _twin(arena16, F.far_batch, ("bf16", 2, 4, 2, 512, 512, 128, 4, 200, True), dkdv=dkdv, probe=True)


HEAD = [("bf16", 2, 2, 1, 512, 512, 128, 4, 200, True), ("fp16", 2, 2, 1, 640, 640, 64, 0, 128, False)]


@pytest.mark.parametrize("case", HEAD, ids=["bf16-d128", "fp16-d64"])
def test_dense_far_head(arena16, case, dkdv):
    """Head stride of 4 GiB (q head 1 at element 2^31).  The hand-placed kernels carry head strides as 32-bit bytes, so
    slice_ok() sends such operands to the generic kernels: near runs fwd_mfma / the MFMA backward, far runs
    fwd_generic_f32math / bwd_generic_f32math and matches the oracle.  (Before the guard the far run took the MFMA path
    with the stride cut to 0 and returned head 0's result for head 1.)"""
    _twin(arena16, F.far_head, case, mode="generic", far_fwd="fwd_generic_f32math", far_bwd="bwd_generic_f32math", dkdv=dkdv)


@pytest.mark.parametrize("case", HEAD, ids=["bf16-d128", "fp16-d64"])
def test_dense_head_stride_just_under_4_gib(arena16, case, dkdv):
    """The largest head stride slice_ok() accepts, 2^32 - 16 bytes: as a signed 32-bit number it is negative.  The MFMA
    kernels of the near run serve it and give the same bits."""
    _twin(arena16, F.band_head, case, dkdv=dkdv)


CU = [0, 70, 71, 300, 517]


def test_far_head_n_q_below_n_kv_is_refused_and_writes_nothing(arena16):
    _refusal(arena16, F.far_head, 2, 2, 1, 256, 768, 128, None, True, True, "head stride")


@pytest.mark.parametrize("D,aux", [(128, True), (80, False)])
def test_packed_far_head_is_refused_and_writes_nothing(arena16, D, aux):
    _refusal(arena16, F.far_head, 1, 2, 1, 517, 517, D, CU, aux, True, "head stride")


# ------------------------------------------------------------------------------------------- row reach
ROWS_FWD = ("bf16", 2, 2, 1, 2048, 2048, 128, 4, 128, False)
ROWS_BWD = ("bf16", 2, 2, 1, 4096, 4096, 128, 4, 128, False)


def test_forward_at_the_widest_row_stride(arena16):
    """sn = 906856: the last row of every slice lies 1.73 x 2^31 bytes behind its first, still on the MFMA path."""
    _twin(arena16, F.wide_rows(2048, F.FWD_MARGIN), ROWS_FWD, bwd=False)


def test_backward_at_the_widest_row_stride(arena16, dkdv):
    _twin(arena16, F.wide_rows(4096, F.BWD_MARGIN), ROWS_BWD, dkdv=dkdv)


def test_forward_one_step_over_the_row_rule_takes_the_generic_kernel(arena16):
    _twin(arena16, F.over_rows(2048, F.FWD_MARGIN), ROWS_FWD, bwd=False, mode="generic", far_fwd="fwd_generic_f32math")


def test_backward_one_step_over_the_row_rule_takes_the_generic_kernel(arena16):
    # (the forward's rule still holds at this stride: it stays on the MFMA path, as in the near run)
    g = F.over_rows(4096, F.BWD_MARGIN)
    assert F.row_reach_ok(4096, g.sn, F.FWD_MARGIN)
    case = ROWS_BWD
    inp, sa, ref = _inputs(*case)
    near = _near_operands(inp)
    rn = _run_prefill(near, case[7], case[8], None)
    arena = _arena(arena16, torch.bfloat16)
    far = _far_operands(arena, g, inp)
    rf = _run_prefill(far, case[7], case[8], None)
    assert rn["rc_fwd"] == rn["rc_bwd"] == rf["rc_fwd"] == rf["rc_bwd"] == 0, (rn, rf)
    assert rf["fwd_path"] == rn["fwd_path"] and torch.equal(far["o"], near["o"])
    assert "generic" not in rn["bwd_path"] and rf["bwd_path"] == "bwd_generic_f32math", (rn["bwd_path"], rf["bwd_path"])
    _check_oracle(far, ref, torch.bfloat16, "far")
    F.assert_untouched(arena, list(far.values()), g.name)


@pytest.mark.parametrize("margin", [F.FWD_MARGIN, F.BWD_MARGIN])
@pytest.mark.parametrize("cu,Nq,Nk", [(CU, 517, 517), (None, 256, 768)], ids=["packed", "nq256-nk768"])
def test_over_the_row_rule_packed_and_n_q_below_n_kv_are_refused(arena16, margin, cu, Nq, Nk):
    """One step of 8 over the forward's rule: forward and backward refuse.  One step over the backward's: the forward
    still runs on the MFMA path, the backward refuses."""
    g = F.over_rows(Nk, margin)
    fwd_refused = not F.row_reach_ok(Nk, g.sn, F.FWD_MARGIN)
    assert fwd_refused == (margin == F.FWD_MARGIN)
    _refusal(arena16, g, 1 if cu else 2, 2, 1, Nq, Nk, 128, cu, True, fwd_refused, "4 GiB head slices")


@pytest.mark.parametrize("D", [128, 80])
def test_packed_at_the_widest_row_stride(arena16, D, dkdv):
    """cu = [0, 70, 71, 300, 517]; the stride is sized for the pack's T = 517 rows and the backward's margin (the forward
    alone, at its own wider stride, reaches the [2^31, 2^32) band)."""
    cu = CU
    case = ("bf16", 1, 2, 1, 517, 517, D, 0, 128, False)
    _twin(arena16, F.wide_rows(517, F.FWD_MARGIN), case, bwd=False, cu=cu)
    _twin(arena16, F.wide_rows(517, F.BWD_MARGIN), case, cu=cu, dkdv=dkdv)


# ------------------------------------------------------------------------------------------- decode
def _abi_decode(q, k, v, out, sa, ring=None, new=None):
    """sfa_decode (ring None), sfa_decode_ring (ring = (window_k, window_v, sink_len, window_len); k / v are then the
    sink buffers) or sfa_decode_ring_step (new = (k_new, v_new, write_pos)) through the C ABI: every tensor operand,
    the output included, is the caller's.  Returns the kernel path."""
    N = _nat()
    lib = N.lib()
    B, Hq, _one, D = q.shape
    n1 = k.shape[2] if ring is None else ring[2]
    n2 = 0 if ring is None else ring[3]
    ws = torch.zeros(max(int(lib.sfa_decode_workspace_bytes(B, Hq, k.shape[1], n1 + n2, D, N.SFA_DTYPE[q.dtype])), 256),
                     dtype=torch.uint8, device=DEV)
    tail = (sa.data_ptr(), ws.data_ptr(), ws.numel(), 1.0 / math.sqrt(D), 0, _stream())
    if ring is None:
        rc = lib.sfa_decode(N.desc(q), N.desc(k), N.desc(v), N.desc(out), *tail)
    elif new is None:
        rc = lib.sfa_decode_ring(N.desc(q), N.desc(k), N.desc(v), n1, N.desc(ring[0]), N.desc(ring[1]), n2, N.desc(out), *tail)
    else:
        rc = lib.sfa_decode_ring_step(N.desc(q), N.desc(k), N.desc(v), n1, N.desc(ring[0]), N.desc(ring[1]), n2, new[2],
                                      N.desc(new[0]), N.desc(new[1]), N.desc(out), *tail)
    N.check(rc, "decode")
    torch.cuda.synchronize()
    return N.last_path()


@pytest.mark.parametrize("dt,D,Nkv", [("bf16", 128, 300), ("bf16", 128, 4100), ("fp32", 64, 300)])
def test_decode_far_batch(arena16, dt, D, Nkv):
    dtype = {"bf16": torch.bfloat16, "fp32": torch.float32}[dt]
    g = torch.Generator().manual_seed(7200 + Nkv)
    B, Hq, Hkv = 2, 8, 2
    q, k, v = rand((B, Hq, 1, D), g, dtype), rand((B, Hkv, Nkv, D), g, dtype), rand((B, Hkv, Nkv, D), g, dtype)
    sa = rand((Hq,), g, torch.float32, 0.5)
    nq, nk, nv = q.to(DEV), k.to(DEV), v.to(DEV)
    near = torch.empty_like(nq)
    pn = _abi_decode(nq, nk, nv, near, sa.to(DEV))
    assert maxdiff(near, O.decode_dense(q, k, v, sa)) < TOL[dtype]
    arena = _arena(arena16, dtype)
    fq, fk, fv, far = F.views(arena, F.far_batch, [nq, nk, nv, tuple(q.shape)])
    pf = _abi_decode(fq, fk, fv, far, sa.to(DEV))
    assert pf == pn and torch.equal(far, near), (pn, pf, maxdiff(far, near))
    F.assert_untouched(arena, [fq, fk, fv, far], "decode", inputs=[(fq, nq), (fk, nk), (fv, nv)])


def _layer(ns, W, bufs, state, per_seq, pool):
    from sink_attention.cache import SinkCacheLayer
    L = SinkCacheLayer(ns, W)
    L.sink_k, L.sink_v, L.window_k, L.window_v = bufs
    L._dev_state = state
    L.is_initialized = L.prefilled = True
    L._per_seq, L._pool = per_seq, pool
    return L


@pytest.mark.parametrize("dt,D", [("bf16", 128), ("fp32", 64)])
def test_ring_decode_and_steps_far_batch(arena16, dt, D):
    """sfa_decode_ring, _step and _step_dyn with the sink and window buffers, q, k_new, v_new and the outputs behind a
    4 GiB batch stride."""
    dtype = {"bf16": torch.bfloat16, "fp32": torch.float32}[dt]
    g = torch.Generator().manual_seed(7300 + D)
    B, Hq, Hkv, ns, W, wl = 2, 8, 2, 4, 96, 40
    shapes = [(B, Hkv, ns, D)] * 2 + [(B, Hkv, W, D)] * 2
    cpu = [rand(s, g, dtype) for s in shapes]
    q, kn, vn = rand((B, Hq, 1, D), g, dtype), rand((B, Hkv, 1, D), g, dtype), rand((B, Hkv, 1, D), g, dtype)
    sa = rand((Hq,), g, torch.float32, 0.5)
    arena = _arena(arena16, dtype)
    nearb = [t.to(DEV) for t in cpu]
    farb = F.views(arena, F.far_batch, [t.to(DEV) for t in cpu])
    fq, fkn, fvn, fo1, fo2, fout = F.views(arena[1 << 22:], F.far_batch,
                                           [q.to(DEV), kn.to(DEV), vn.to(DEV)] + [tuple(q.shape)] * 3)
    mk = lambda: torch.empty(q.shape, dtype=dtype, device=DEV)
    res = []
    for bufs, (qq, kk, vv), (o1, o2, out) in ((nearb, (q.to(DEV), kn.to(DEV), vn.to(DEV)), (mk(), mk(), None)),
                                              (farb, (fq, fkn, fvn), (fo1, fo2, fout))):
        p1 = _abi_decode(qq, bufs[0], bufs[1], o1, sa.to(DEV), ring=(bufs[2], bufs[3], ns, wl))
        p2 = _abi_decode(qq, bufs[0], bufs[1], o2, sa.to(DEV), ring=(bufs[2], bufs[3], ns, wl + 1), new=(kk, vv, wl))
        st = torch.tensor([ns, wl + 1, wl + 1], dtype=torch.int32, device=DEV)
        L = _layer(ns, W, bufs, st, False, False)
        o3 = L.decode_step_dyn(qq, kk, vv, s_aux=sa.to(DEV), out=out)
        p3 = _nat().last_path()
        res.append(((o1, o2, o3.clone()), (p1, p2, p3), st.tolist()))
    (on, pn, sn_), (of, pf, sf_) = res
    kc = torch.cat([cpu[0], cpu[2][:, :, :wl]], dim=2)
    vc = torch.cat([cpu[1], cpu[3][:, :, :wl]], dim=2)
    assert maxdiff(on[0], O.decode_dense(q, kc, vc, sa)) < TOL[dtype]
    assert maxdiff(on[1], O.decode_dense(q, torch.cat([kc, kn], 2), torch.cat([vc, vn], 2), sa)) < TOL[dtype]
    assert maxdiff(on[2], O.decode_dense(q, torch.cat([kc, kn, kn], 2), torch.cat([vc, vn, vn], 2), sa)) < TOL[dtype]
    assert pn == pf and sn_ == sf_ == [ns, wl + 2, wl + 2], (pn, pf, sn_, sf_)
    for a, b in zip(on, of):
        assert torch.equal(a, b)
    for a, b in zip(nearb, farb):
        assert torch.equal(a, b)
    F.assert_untouched(arena, list(farb) + [fq, fkn, fvn, fo1, fo2, fout], "ring",
                       inputs=[(fq, q.to(DEV)), (fkn, kn.to(DEV)), (fvn, vn.to(DEV))])


# ------------------------------------------------------------------------------------------- slot pool / state rows
TREE = [-1, 0, 0, 1, 1, 2, 4, 4]
POOL = [("bf16", 64, 8, 1), ("fp16", 128, 1, 2), ("fp32", 48, 2, 2)]       # dtype, D, G = Hq / Hkv, Hkv


def _pool_script(L, inp, slots_a, slots_b, sa, outs, pool):
    """Every slot-indexed (pool) or per-row (rows) call once, on layer L; returns outputs, paths and states."""
    dev = lambda x: x.to(DEV) if isinstance(x, torch.Tensor) else x
    N = _nat()
    rec = []

    def note(name, out=None):
        rec.append((name, N.last_path(), None if out is None else out.clone(), L._dev_state.clone()))

    kw = lambda s: dict(slots=torch.tensor(s, dtype=torch.int32, device=DEV)) if pool else {}
    o = L.decode_step_dyn(inp["q1"], inp["k1"], inp["v1"], s_aux=sa, out=outs["o1"], **kw(slots_a))
    note("step", o)
    for n in (1, 3, 8):
        o = L.extend_attention_dyn(inp["q8"][:, :, :n], inp["k8"][:, :, :n], inp["v8"][:, :, :n], s_aux=sa,
                                   out=outs["o8"][:, :, :n], **kw(slots_b))
        note(f"multi{n}", o)
    o = L.extend_step_dyn(inp["q8"][:, :, :3], inp["k8"][:, :, :3], inp["v8"][:, :, :3], s_aux=sa, out=outs["o8"][:, :, :3],
                          **kw(slots_a))
    note("multi3_commit", o)
    o = L.extend_attention_tree_dyn(inp["q8"], inp["k8"], inp["v8"], torch.tensor(TREE, device=DEV), s_aux=sa,
                                    out=outs["o8"], **kw(slots_b))
    note("tree", o)
    cnt = torch.tensor([2, 5], dtype=torch.int32, device=DEV)
    L.commit_dyn(inp["k8"], inp["v8"], cnt, **kw(slots_a))
    note("commit")
    L.commit_path_dyn(inp["k8"], inp["v8"], torch.tensor([0, 1, 4, 6, 0, 0, 0, 0], device=DEV), cnt, **kw(slots_b))
    note("commit_path")
    return rec


@pytest.mark.parametrize("dt,D,G,Hkv", POOL, ids=[f"{p[0]}-d{p[1]}-g{p[2]}" for p in POOL])
@pytest.mark.parametrize("form", ["slots", "rows"])
def test_pool_and_rows_calls_far(arena16, form, dt, D, G, Hkv):
    """slots: a pool of 9 slots whose stride[0] puts slot 8 at 4 GiB (element 2^31 for the 2-byte types); every call
    names slot 1 (near) and slot 8 (far), the ragged step also slot 3 and an inactive row.  rows: the same calls in
    their per-row form on a cache of two rows behind a 4 GiB batch stride.  Outputs, paths, states and the content of
    every named slot equal the near twin's; the unnamed slots and the rest of the arena keep the sentinel."""
    dtype = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[dt]
    pool = form == "slots"
    g = torch.Generator().manual_seed(7400 + D)
    Hq, ns, W = G * Hkv, 4, 64
    S, named = (9, [8, 1, 3]) if pool else (2, [1, 0])
    geom = F.far_slot if pool else F.far_batch
    lens = [ns + W + 9, 10, 30][:len(named)]                  # slot 8 / row 1: a ring that has already wrapped
    cu = [0] + [sum(lens[:i + 1]) for i in range(len(lens))]
    T = cu[-1]
    kp, vp = rand((1, Hkv, T, D), g, dtype), rand((1, Hkv, T, D), g, dtype)
    B = 2
    cpu = dict(q1=rand((B, Hq, 1, D), g, dtype), k1=rand((B, Hkv, 1, D), g, dtype), v1=rand((B, Hkv, 1, D), g, dtype),
               q8=rand((B, Hq, 8, D), g, dtype), k8=rand((B, Hkv, 8, D), g, dtype), v8=rand((B, Hkv, 8, D), g, dtype))
    rl = [1, 3, 40, 2]                                        # ragged step: the last sequence inactive
    rcu = [0, 1, 4, 44, 46]
    rq, rk, rv = rand((1, Hq, 46, D), g, dtype), rand((1, Hkv, 46, D), g, dtype), rand((1, Hkv, 46, D), g, dtype)
    sa = rand((Hq,), g, torch.float32, 0.5).to(DEV)
    shapes = [(S, Hkv, ns, D)] * 2 + [(S, Hkv, W, D)] * 2
    arena = _arena(arena16, dtype)
    farb = F.views(arena, geom, shapes)
    for t in farb:
        t[named] = 0                                          # the named slots start as the near pool's: zeros
    nearb = [torch.zeros(s, dtype=dtype, device=DEV) for s in shapes]
    act = arena[1 << 22:]                                     # activations and outputs: far views too
    names = ["q1", "k1", "v1", "q8", "k8", "v8"]
    fv = F.views(act, F.far_batch, [cpu[x].to(DEV) for x in names] + [tuple(cpu["q1"].shape), tuple(cpu["q8"].shape)])
    far_in, far_out = dict(zip(names, fv[:6])), dict(o1=fv[6], o8=fv[7])
    near_in = {x: cpu[x].to(DEV) for x in names}
    near_out = dict(o1=torch.empty_like(near_in["q1"]), o8=torch.empty_like(near_in["q8"]))
    slots_a, slots_b = ([1, 8], [8, 1]) if pool else (None, None)
    runs = []
    for bufs, inp, outs in ((nearb, near_in, near_out), (farb, far_in, far_out)):
        st = torch.zeros(S, 4, dtype=torch.int32, device=DEV)
        L = _layer(ns, W, bufs, st, True, True)
        L.prefill_slots(kp.to(DEV), vp.to(DEV), cu, named)    # sfa_ring_fill_varlen_slots
        rec = [("fill", _nat().last_path(), None, st.clone())]
        L._pool = pool
        rec += _pool_script(L, inp, slots_a, slots_b, sa, outs, pool)
        if pool:
            o = L.ragged_step_dyn(rq.to(DEV), rk.to(DEV), rv.to(DEV), rcu, [8, 1, 3, -1], s_aux=sa)
            rec.append(("ragged", _nat().last_path(), o.clone(), st.clone()))
        runs.append(rec)
    # (a) the near run's first step against the oracle: row b attends its prompt's surviving keys plus the new token
    o_step = runs[0][1][2]
    order = slots_a if pool else [0, 1]
    for b, c in enumerate(order):
        i = named.index(c)
        keys = torch.arange(cu[i], cu[i + 1])
        keep = torch.cat([keys[:ns], keys[ns:][-W:]]) if lens[i] > ns else keys
        if lens[i] - ns >= W:                                  # a full ring: the step evicts the oldest window key
            keep = torch.cat([keep[:ns], keep[ns + 1:]])
        kk = torch.cat([kp[:, :, keep], cpu["k1"][b:b + 1]], dim=2)
        vv = torch.cat([vp[:, :, keep], cpu["v1"][b:b + 1]], dim=2)
        ref = O.decode_dense(cpu["q1"][b:b + 1], kk, vv, sa.cpu())
        assert maxdiff(o_step[b:b + 1], ref) < TOL[dtype], (b, c, maxdiff(o_step[b:b + 1], ref))
    for (name, pn, on, sn_), (_, pf, of, sf_) in zip(*runs):
        assert pn == pf, (name, pn, pf)
        assert torch.equal(sn_, sf_), (name, sn_.tolist(), sf_.tolist())
        assert on is None or torch.equal(on, of), (name, maxdiff(on, of))
    assert "ragged" in runs[0][-1][1] or not pool
    rest = [c for c in range(S) if c not in named]
    for a, b in zip(nearb, farb):
        assert torch.equal(a[named], b[named])
        assert not rest or (F.is_sentinel(b[rest]) and not bool(a[rest].any()))
    F.assert_untouched(arena, list(farb) + list(fv), f"{form} {dt}")


def test_pool_probe_inputs_far_slot(arena16):
    """A verify chunk over far slots on mask-edge probe inputs (tests/probe_inputs.py::chunk_probe): one wrong base
    address moves a row's whole softmax mass, so it cannot pass on plausible data."""
    dtype, Hq, Hkv, D, ns, W, n = torch.bfloat16, 8, 1, 64, 4, 64, 8
    named, S = [8, 1], 9
    prs = [P.chunk_probe(1, Hq, Hkv, D, ns, W, L, n, dtype, 7500 + i, aux=False) for i, L in enumerate((ns + W + 9, 40))]
    lens = [ns + W + 9, 40]
    cu = [0, lens[0], lens[0] + lens[1]]
    kp = torch.cat([pr["k"][:, :, :L] for pr, L in zip(prs, lens)], dim=2)
    vp = torch.cat([pr["v"][:, :, :L] for pr, L in zip(prs, lens)], dim=2)
    q = torch.cat([pr["q"][:, :, L:] for pr, L in zip(prs, lens)], dim=0)
    kn = torch.cat([pr["k"][:, :, L:] for pr, L in zip(prs, lens)], dim=0)
    vn = torch.cat([pr["v"][:, :, L:] for pr, L in zip(prs, lens)], dim=0)
    sa = None
    shapes = [(S, Hkv, ns, D)] * 2 + [(S, Hkv, W, D)] * 2
    arena = _arena(arena16, dtype)
    farb = F.views(arena, F.far_slot, shapes)
    for t in farb:
        t[named] = 0
    nearb = [torch.zeros(s, dtype=dtype, device=DEV) for s in shapes]
    outs = []
    for bufs in (nearb, farb):
        st = torch.zeros(S, 4, dtype=torch.int32, device=DEV)
        L = _layer(ns, W, bufs, st, True, True)
        L.prefill_slots(kp.to(DEV), vp.to(DEV), cu, named)
        o = L.extend_step_dyn(q.to(DEV), kn.to(DEV), vn.to(DEV), s_aux=sa, slots=named)
        outs.append((o, _nat().last_path(), st.clone()))
    (on, pn, sn_), (of, pf, sf_) = outs
    for b, (pr, L) in enumerate(zip(prs, lens)):
        ref = chunk_oracle_rows(pr["q"], pr["k"], pr["v"], None, L, ns, W, n, slice(0, 1))
        assert maxdiff(on[b:b + 1], ref) < TOL[dtype], (b, maxdiff(on[b:b + 1], ref))
    assert pn == pf and torch.equal(sn_, sf_) and torch.equal(on, of), (pn, pf, maxdiff(on, of))
    for a, b in zip(nearb, farb):
        assert torch.equal(a[named], b[named]) and F.is_sentinel(b[[0, 2, 3, 4, 5, 6, 7]])
    F.assert_untouched(arena, list(farb), "pool probe")


# ------------------------------------------------------------------------------------------- the serving pool, far
# The packed serving calls (ragged_step_dyn with admit / parent / commit_seq, commit_packed_dyn, fork_slots) on the
# contiguous 16-bit and fp32 pool, the FP8 pool and the paged pool.  One script of calls runs on a near pool and on a far
# one; after EVERY call the output, the path, the state rows and the bytes of every named slot (paged: of every mapped
# page) are recorded, and the two records must be equal.  Every case asserts from data_ptr() that what it calls far lies
# at or past its line, and that every storing call changed bytes of every slot it names.  No mutant of a kernel runs
# here: tests/test_far_views.py proves on the CPU, per case and per operand, that a 32-bit element offset, an unsigned or
# a signed 32-bit byte offset would move one of these rows onto the sentinel or out of the arena.
from test_gpu_ragged_tree import _check_rows, _cu, _i32, _oracle_tree          # noqa: E402
from test_ragged_tree_host import binary, chain, read_as, star                 # noqa: E402
import paged_ref as PR                                                         # noqa: E402
from fp8_ref import FP8, dequant                                               # noqa: E402

DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
NS, WC, PG = 4, 64, 32
RING = ("window_k", "window_v")
BUFS = ("sink_k", "sink_v") + RING


def _ints(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _offset(arena, t):
    """bytes from the arena's first byte to the first byte of t (data_ptr arithmetic on the device tensors)"""
    return t.data_ptr() - arena.data_ptr()


def _pool_layer(W, bufs, S, table=None, scales=None):
    L = _layer(NS, W, list(bufs), torch.zeros(S, 4, dtype=torch.int32, device=DEV), True, True)
    if table is not None:
        L.page_size, L.page_table = bufs[2].shape[2], torch.tensor(table, dtype=torch.int32, device=DEV)
    if scales is not None:
        L.kv_scale = torch.ones(2, bufs[0].shape[1], dtype=torch.float32, device=DEV)
        L.set_kv_scale(*scales)
    return L


def _content(L, named):
    """bytes of every named slot, cloned: sinks per slot; the ring per slot, or per mapped table entry of a paged pool"""
    c = {}
    for name in BUFS:
        buf = _ints(getattr(L, name))
        for s in named:
            if L.page_size and name in RING:
                for j, e in enumerate(L.page_table[s].tolist()):
                    if 0 <= e < buf.shape[0]:
                        c[(name, s, j)] = buf[e].clone()
            else:
                c[(name, s)] = buf[s].clone()
    return c


def _play(L, steps, named):
    rec = [dict(name="start", path=None, o=None, st=L._dev_state.clone(), c=_content(L, named), writes=())]
    for name, fn, writes in steps:
        o = fn(L)
        torch.cuda.synchronize()
        rec.append(dict(name=name, path=_nat().last_path(), o=None if o is None else o.clone(), st=L._dev_state.clone(),
                        c=_content(L, named), writes=writes))
    return rec


def _changed(rec, i, s):
    """did call i of a record change bytes of slot s?"""
    a, b = rec[i - 1]["c"], rec[i]["c"]
    return any(k not in a or not torch.equal(a[k], b[k]) for k in b if k[1] == s)


def _same_records(near, far, what):
    assert len(near) == len(far)
    for i, (a, b) in enumerate(zip(near, far)):
        w = (what, a["name"])
        assert a["path"] == b["path"], (w, a["path"], b["path"])                                    # (c)
        assert torch.equal(a["st"], b["st"]), (w, a["st"].tolist(), b["st"].tolist())               # (b)
        assert (a["o"] is None) == (b["o"] is None) and (a["o"] is None or torch.equal(a["o"], b["o"])), \
            (w, "o", None if a["o"] is None else maxdiff(a["o"].float(), b["o"].float()))
        assert a["c"].keys() == b["c"].keys(), w
        for k in a["c"]:
            assert torch.equal(a["c"][k], b["c"][k]), (w, "content of", k)
        for s in a["writes"]:                       # a storing call moved bytes of every slot it names, in both runs
            assert _changed(near, i, s) and _changed(far, i, s), (w, "stored nothing into slot", s)


def _rows(g, dtype, H, T, D):
    return rand((1, H, T, D), g, dtype)


class _Serving:
    """The script of the serving sequence over the slots (far, a, b): b is prefilled with 30 tokens (a partly filled
    ring) and decodes; far is fresh and is admitted with num_sink + Wc + 7 tokens (the ring full, wrapped at slot 0, then
    moved on by the tree step: write_pos 7); a is fresh and is admitted with 2 < num_sink tokens (a short one).  One
    sequence of every pack is inactive (-1), every pack has a padded tail.  `hist` replays on the CPU what every slot
    holds, for the fp64 oracle of every attending call."""

    def __init__(self, dt, D, G, Hkv, W, slots, seed, short=False, place=None):
        self.dtype, self.D, self.G, self.Hkv, self.W = DT[dt], D, G, Hkv, W
        self.far, self.a, self.b = slots
        far, a, b = slots
        dtype, Hq = self.dtype, G * Hkv
        g = torch.Generator().manual_seed(seed)
        self.sa = rand((Hq,), g, torch.float32, 0.5)
        sad = self.sa.to(DEV)
        kp, vp = _rows(g, dtype, Hkv, 30, D), _rows(g, dtype, Hkv, 30, D)
        self.long = NS + W + 7
        L1, S1 = [3, 40, 2, self.long], [b, -1, a, far]
        T1 = sum(L1) + 8
        assert T1 <= 260
        p1 = [_rows(g, dtype, h, T1, D) for h in (Hq, Hkv, Hkv)]
        L2, S2 = [7, 16, 1, 3], [far, b, a, -1]
        T2 = sum(L2) + 5
        trees = [star(7), binary(16), chain(1), chain(3)]
        par = sum(trees, []) + [5] * (T2 - sum(L2))
        seq = [1, 0, 1, 1]                                        # the 16-node tree on b is held back
        p2 = [_rows(g, dtype, h, T2, D) for h in (Hq, Hkv, Hkv)]
        path = [6, 9, -2, 3, 0, 1, 2] + [15, 3, 3, 20, 0, -1, 7, 8, 9, 1, 2, 4, 5, 6, 10, 11] + [0] + [2, 1, 0] + [9] * 5
        cnt_a, cnt_b = [9, -2, 0, 2], [3, 5, 1, 2]                # beyond n_i, negative, zero, an inactive sequence
        d1, d2 = [t.to(DEV) for t in p1] + [None], [t.to(DEV) for t in p2] + [None]
        self.views, self.inputs = [], []
        if place is not None:               # the packs themselves (and their outputs) on views: place(operands, n-th pack)
            for n, d in enumerate((d1, d2)):
                vs = place(d[:3] + [tuple(d[0].shape)], n)
                self.inputs += list(zip(vs[:3], d[:3]))
                self.views += vs
                d[:] = vs
        kpd, vpd = kp.to(DEV), vp.to(DEV)

        def step(L, d, lens, sl, **kw):
            return L.ragged_step_dyn(d[0], d[1], d[2], _i32(_cu(lens)), _i32(sl), s_aux=sad, out=d[3], **kw)

        def prefill(L):
            L.prefill_slots(kpd, vpd, [0, 30], [b])

        def commit(L, cnt, pt):
            L.commit_packed_dyn(d2[1], d2[2], _i32(_cu(L2)), _i32(S2), _i32(cnt), path=None if pt is None else _i32(pt))

        self.steps = [("prefill_slots", prefill, (b,)),
                      ("admit", lambda L: step(L, d1, L1, S1, admit=True, commit=True), (far, a, b))]
        self.events = [("store", b, kp, vp), ("attend", "admit", p1, L1, S1, None, True)]
        self.events += [("store", s, p1[1][:, :, c:c + n], p1[2][:, :, c:c + n])
                        for s, c, n in zip(S1, _cu(L1), L1) if s >= 0]
        if not short:
            self.steps += [("tree", lambda L: step(L, d2, L2, S2, parent=_i32(par), commit_seq=_i32(seq), commit=True), (far, a)),
                           ("commit_path", lambda L: commit(L, cnt_a, path), (far,)),
                           ("commit", lambda L: commit(L, cnt_b, None), (far, a, b))]
            self.events += [("attend", "tree", p2, L2, S2, trees, False)]
            cu2 = _cu(L2)
            self.events += [("store", s, p2[1][:, :, c:c + n], p2[2][:, :, c:c + n])
                            for s, c, n, m in zip(S2, cu2, L2, seq) if s >= 0 and m]
            for cnt, pt in ((cnt_a, path), (cnt_b, None)):
                for i, (s, c, n) in enumerate(zip(S2, cu2, L2)):
                    acc = min(max(cnt[i], 0), n)
                    if s < 0 or acc == 0:
                        continue
                    src = [c + (j if pt is None else min(max(pt[c + j], 0), n - 1)) for j in range(acc)]
                    self.events.append(("store", s, p2[1][:, :, src], p2[2][:, :, src]))
        self.plain = lambda L, sl: step(L, d2, L2, sl, commit=False)
        self.steps.append(("plain", lambda L: self.plain(L, S2), ()))
        self.events.append(("attend", "plain", p2, L2, S2, None, False))
        self.short = short

    def check_states(self, rec, what):
        """the far slot's first committed state, outright: the ring full and wrapped; then write_pos != 0"""
        by = {r["name"]: r for r in rec}
        assert by["admit"]["st"][self.far].tolist() == [NS, self.W, 0, self.long], (what, by["admit"]["st"].tolist())
        assert by["admit"]["st"][self.a].tolist() == [2, 0, 0, 2] and by["admit"]["st"][self.b].tolist() == [NS, 29, 29, 33]
        if not self.short:
            assert by["tree"]["st"][self.far].tolist() == [NS, self.W, 7, self.long + 7], (what, by["tree"]["st"].tolist())
            assert by["commit"]["st"][self.far].tolist() == [NS, self.W, 17, self.long + 17]
            assert by["commit"]["st"][self.b].tolist() == [NS, 34, 34, 38]

    def check_oracle(self, rec, what):
        """(a): every attending call of a record against fp64 decode_dense per node over the replayed history"""
        by = {r["name"]: r for r in rec}
        hist = {}
        for ev in self.events:
            if ev[0] == "store":
                _, s, k, v = ev
                if s not in hist:
                    hist[s] = [k[:, :, :0], v[:, :, :0], min(k.shape[2], NS)]
                hist[s][0], hist[s][1] = torch.cat([hist[s][0], k], dim=2), torch.cat([hist[s][1], v], dim=2)
                continue
            _, name, (q, k, v), lens, sl, trees, admit = ev
            ref = {}
            for i, (s, c, n) in enumerate(zip(sl, _cu(lens), lens)):
                if s < 0 or n == 0:
                    continue
                sel = slice(c, c + n)
                if s not in hist:     # an admission: the mask of a prefill of the chunk alone, its first tokens the sinks
                    assert admit
                    rows = []
                    for u in range(n):
                        keep = [c + w for w in range(u + 1) if w < min(n, NS) or u - w <= self.W - 1]
                        rows.append(O.decode_dense(q[:, :, c + u:c + u + 1], k[:, :, keep], v[:, :, keep], self.sa))
                    ref[i] = torch.cat(rows, dim=2)
                    continue
                hk, hv, nsink = hist[s]
                par = read_as(trees[i], n) if trees is not None else chain(n)
                ref[i] = _oracle_tree(q[:, :, sel], torch.cat([hk, k[:, :, sel]], dim=2), torch.cat([hv, v[:, :, sel]], dim=2),
                                      self.sa, hk.shape[2], nsink, self.W, par)
            assert len(ref) == 3
            _check_rows(by[name]["o"], ref, lens, TOL[self.dtype], (what, name))


# ---- 1. the packed serving forms on far slots of the contiguous pool
PACKED = [("bf16", 64, 8, 1), ("fp16", 128, 1, 2), ("bf16", 96, 1, 2), ("fp32", 48, 2, 2)]      # dtype, D, G, Hkv
SLOT_S, SLOT_NAMED = 9, [8, 1, 3]                     # far (fresh, admitted long), a (fresh, short), b (prefilled)


def _pool_shapes(S, Hkv, W, D):
    return [(S, Hkv, NS, D)] * 2 + [(S, Hkv, W, D)] * 2


def _far_pool(arena, geom, S, Hkv, W, D, named, sentinel=F.SENTINEL16):
    bufs = F.views(arena, geom, _pool_shapes(S, Hkv, W, D))
    for t in bufs:
        _ints(t)[named] = 0                           # the named slots start as the near pool's: zeros
    return bufs


def _near_pool(S, Hkv, W, D, dtype):
    return [torch.zeros(s, dtype=torch.uint8 if dtype == FP8 else dtype, device=DEV).view(dtype) for s in _pool_shapes(S, Hkv, W, D)]


def _unnamed_keep_the_sentinel(nearb, farb, S, named, sentinel=F.SENTINEL16):
    rest = [c for c in range(S) if c not in named]
    for a, b in zip(nearb, farb):
        assert F.is_sentinel(_ints(b)[rest], sentinel) and not bool(_ints(a)[rest].any())


@pytest.mark.parametrize("dt,D,G,Hkv", PACKED, ids=[f"{p[0]}-d{p[1]}-g{p[2]}" for p in PACKED])
def test_packed_serving_calls_far_slot(arena16, dt, D, G, Hkv):
    """prefill, an admitting committing step, a tree step with commit_seq, commit_packed_dyn with count and path and
    without a path, a plain step - on a pool whose slot 8 lies at 4 GiB and receives the long admission."""
    dtype = DT[dt]
    sv = _Serving(dt, D, G, Hkv, WC, SLOT_NAMED, seed=7700 + D)
    near = _play(_pool_layer(WC, _near_pool(SLOT_S, Hkv, WC, D, dtype), SLOT_S), sv.steps, SLOT_NAMED)
    sv.check_states(near, "near")
    sv.check_oracle(near, (dt, D, G))                                                               # (a)
    arena = _arena(arena16, dtype)
    farb = _far_pool(arena, F.far_slot, SLOT_S, Hkv, WC, D, SLOT_NAMED)
    for t in farb:
        assert _offset(arena, t[8]) >= F.TWO32 and _offset(arena, t[3, -1, -1]) < F.TWO31
        assert dtype == torch.float32 or (_offset(arena, t[8]) // t.element_size()) >= F.TWO31
    far = _play(_pool_layer(WC, farb, SLOT_S), sv.steps, SLOT_NAMED)
    _same_records(near, far, ("far_slot", dt, D))                                                   # (b), (c)
    _unnamed_keep_the_sentinel(_near_pool(SLOT_S, Hkv, WC, D, dtype), farb, SLOT_S, SLOT_NAMED)
    assert "_admit_commit" in far[2]["path"] and "decode_tree_" in far[3]["path"] and \
        far[4]["path"] == far[5]["path"] == "ring_commit_path_ragged_slots", [r["path"] for r in far]
    F.assert_untouched(arena, farb, f"packed serving {dt} {D}")                                     # (d)


@pytest.mark.parametrize("dt,D", [("bf16", 128), ("fp16", 80), ("fp32", 64)])
def test_packed_serving_calls_with_the_pack_behind_a_far_head(arena16, dt, D):
    """q, k_new, v_new and out of every step of the serving script on far_head_skew views (G 1, H_kv 2): head 1 of each
    lies past 4 GiB, over a near pool.  The library serves the layout (it forms these addresses in 64 bits and documents
    no limit for them): far == near bitwise, the pool included."""
    dtype, Hkv, S, named = DT[dt], 2, 4, [2, 1, 3]
    arena = _arena(arena16, dtype)
    place = lambda ops, n: F.views(arena[n << 22:], F.far_head_skew, ops)
    sn_, sf_ = (_Serving(dt, D, 1, Hkv, WC, named, seed=7800 + D, place=pl) for pl in (None, place))
    for t in sf_.views:
        assert _offset(arena, t[0, 1]) >= F.TWO32 and _offset(arena, t[0, 0, -1]) < F.TWO31
        assert dtype == torch.float32 or _offset(arena, t[0, 1]) // 2 >= F.TWO31
    near = _play(_pool_layer(WC, _near_pool(S, Hkv, WC, D, dtype), S), sn_.steps, named)
    sn_.check_states(near, "near")
    sn_.check_oracle(near, ("far-head pack", dt, D))                                                # (a)
    far = _play(_pool_layer(WC, _near_pool(S, Hkv, WC, D, dtype), S), sf_.steps, named)
    _same_records(near, far, ("far_head_skew pack", dt, D))                                         # (b), (c)
    assert far[2]["o"][:, 1].any() and not torch.isnan(far[2]["o"].float()).any()
    F.assert_untouched(arena, sf_.views, f"far-head pack {dt}", inputs=sf_.inputs)                  # (d)


# ---- 2. fork_slots across the 4 GiB line
FORK = [("bf16", 128, 8, 1), ("fp32", 128, 1, 2)]      # 16 and 32 pieces per row: a full ring spans more than one copy block


def _copy_block():
    """pieces one workgroup of ring_copy_slots_kernel copies: 256 * SFA_COPY_PIECES (csrc/sfa_decode_multi.hip)"""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "sink-flash-attention-kernel_amd", "csrc", "sfa_decode_multi.hip")).read()
    return 256 * int(re.search(r"#define SFA_COPY_PIECES (\d+)", src).group(1))


class _Forks:
    """prefill_slots of a wrapped ring (slot `w`) and a short one (slot `s`), then forks; `step(L, slots)` is a plain step
    of a [1, 7] pack over two slots, which must give on every pair of forks the bits it gives on the sources."""

    def __init__(self, dt, D, G, Hkv, w, s, seed, W=WC, both_bodies=True):
        self.dtype, self.w, self.s, self.W = DT[dt], w, s, W
        dtype, Hq = self.dtype, G * Hkv
        g = torch.Generator().manual_seed(seed)
        self.lens = [NS + W + 9, 10]
        T = sum(self.lens)
        self.kp, self.vp = _rows(g, dtype, Hkv, T, D), _rows(g, dtype, Hkv, T, D)
        self.kc, self.vc = _rows(g, dtype, Hkv, 5, D), _rows(g, dtype, Hkv, 5, D)      # 5 more tokens: write_pos 5
        self.pack = [_rows(g, dtype, h, 8, D) for h in (Hq, Hkv, Hkv)]
        self.sa = rand((Hq,), g, torch.float32, 0.5)
        kpd, vpd, sad = self.kp.to(DEV), self.vp.to(DEV), self.sa.to(DEV)
        d = [t.to(DEV) for t in self.pack]
        cpr = D * torch.empty((), dtype=dtype).element_size() // 16
        block = _copy_block()
        live_w, live_s = (NS + W) * cpr, 10 * cpr
        # the wrapped source: at least one block whose pieces are all live (the unpredicated body) and a last, partial
        # one (the predicated body); the short source: less than one block
        assert not both_bodies or (live_w // block >= 1 and live_w % block and live_s < block), (live_w, live_s, block)

        def prefill(L):
            L.prefill_slots(kpd, vpd, _cu(self.lens), [w, s])
            L.commit_packed_dyn(self.kc.to(DEV), self.vc.to(DEV), [0, 5], [w], [5])
        self.prefill = ("prefill_slots", prefill, (w, s))
        self.step = lambda L, slots: L.ragged_step_dyn(d[0], d[1], d[2], [0, 1, 8], slots, s_aux=sad, commit=False)

    def fork(self, src, dst, writes, partner=False):
        return (f"fork {src} -> {dst}", lambda L: L.fork_slots(src, dst, source=L.partner if partner else None), writes)

    def over(self, slots):
        return (f"step {slots}", lambda L: self.step(L, slots), ())

    def check_oracle(self, o, what):
        ref, cu = {}, _cu(self.lens)
        q, k, v = self.pack
        for i, (c, n) in enumerate(((0, 1), (1, 7))):
            hk, hv = self.kp[:, :, cu[i]:cu[i + 1]], self.vp[:, :, cu[i]:cu[i + 1]]
            if i == 0:
                hk, hv = torch.cat([hk, self.kc], 2), torch.cat([hv, self.vc], 2)
            ref[i] = _oracle_tree(q[:, :, c:c + n], torch.cat([hk, k[:, :, c:c + n]], 2), torch.cat([hv, v[:, :, c:c + n]], 2),
                                  self.sa, hk.shape[2], NS, self.W, chain(n))
        _check_rows(o, ref, [1, 7], TOL[self.dtype], what)


def _steps_equal(rec, names, what):
    outs = [r["o"] for r in rec if r["name"] in names]
    assert len(outs) == len(names) and all(torch.equal(outs[0], o) for o in outs[1:]), (what, names)


@pytest.mark.parametrize("dt,D,G,Hkv", FORK, ids=[f"{p[0]}-d{p[1]}" for p in FORK])
def test_fork_slots_across_the_4_gib_line(arena16, dt, D, G, Hkv):
    """near -> far (1 -> 8), far -> near (8 -> 2), a short ring (3 -> 5), a self pair and an inactive pair in one call;
    then source= between a pool of near tensors and the pool of arena views, in both directions."""
    dtype, S, named = DT[dt], SLOT_S, [1, 3, 8, 5, 2]
    fk = _Forks(dt, D, G, Hkv, 1, 3, seed=7900 + D)
    steps = [fk.prefill, fk.fork([1, 3, 4, -1], [8, 5, 4, 6], (8, 5)), fk.fork([8], [2], (2,)),
             fk.over([1, 3]), fk.over([8, 5]), fk.over([2, 5])]
    nearb = _near_pool(S, Hkv, WC, D, dtype)
    Ln = _pool_layer(WC, nearb, S)
    near = _play(Ln, steps, named)
    fk.check_oracle(near[4]["o"], ("fork sources", dt, D))                                          # (a)
    _steps_equal(near, ["step [1, 3]", "step [8, 5]", "step [2, 5]"], "near")
    arena = _arena(arena16, dtype)
    farb = _far_pool(arena, F.far_slot, S, Hkv, WC, D, named)
    for t in farb:
        assert _offset(arena, t[8]) >= F.TWO32 and _offset(arena, t[5, -1, -1]) < F.TWO32 and _offset(arena, t[3, -1, -1]) < F.TWO31
    Lf = _pool_layer(WC, farb, S)
    far = _play(Lf, steps, named)
    _same_records(near, far, ("fork", dt, D))                                                       # (b), (c)
    _steps_equal(far, ["step [1, 3]", "step [8, 5]", "step [2, 5]"], "far")
    assert far[2]["path"] == "ring_copy_slots" and far[2]["st"][8].tolist() == [NS, WC, 5, NS + WC + 14]
    assert not far[3]["st"][[0, 4, 6, 7]].any()                      # the self pair and the inactive pair moved nothing
    _unnamed_keep_the_sentinel(nearb, farb, S, named)
    # source=: out of each pool into a fresh pool of near tensors, and from there back into slots 7 and 8
    named2 = named + [7]
    for t in farb:
        _ints(t)[7] = 0
    recs = []
    for L in (Ln, Lf):
        Z = _pool_layer(WC, _near_pool(S, Hkv, WC, D, dtype), S)
        Z.partner, L.partner = L, Z
        rz = _play(Z, [fk.fork([8, 3], [0, 6], (0, 6), partner=True), fk.over([0, 6])], [0, 6])
        rl = _play(L, [fk.fork([6, 0], [8, 7], (8, 7), partner=True), fk.over([7, 8]), fk.over([1, 3])], named2)
        recs.append((rz, rl))
    (rzn, rln), (rzf, rlf) = recs
    _same_records(rzn, rzf, ("fork out of the pool", dt, D))
    _same_records(rln, rlf, ("fork into the pool", dt, D))
    assert torch.equal(rzf[2]["o"], far[4]["o"]) and torch.equal(rlf[2]["o"], rlf[3]["o"]) and torch.equal(rlf[3]["o"], far[4]["o"])
    assert rlf[1]["st"][8].tolist() == [NS, 6, 6, 10] and rlf[1]["st"][7].tolist() == [NS, WC, 5, NS + WC + 14]
    _unnamed_keep_the_sentinel(nearb, farb, S, named2)
    F.assert_untouched(arena, farb, f"fork {dt}")                                                   # (d)


@pytest.mark.parametrize("dt,D,G,Hkv", FORK, ids=[f"{p[0]}-d{p[1]}" for p in FORK])
def test_fork_slots_far_to_far(arena16, dt, D, G, Hkv):
    """far_slot2: 35 slots of which 33 and 34 both lie past 4 GiB; the wrapped ring of 33 is forked into 34."""
    dtype, S, named = DT[dt], 35, [33, 1, 34, 2]
    fk = _Forks(dt, D, G, Hkv, 33, 1, seed=7950 + D)
    steps = [fk.prefill, fk.fork([33, 1], [34, 2], (34, 2)), fk.over([33, 1]), fk.over([34, 2])]
    nearb = _near_pool(S, Hkv, WC, D, dtype)
    near = _play(_pool_layer(WC, nearb, S), steps, named)
    fk.check_oracle(near[3]["o"], ("far to far, sources", dt, D))
    arena = _arena(arena16, dtype)
    farb = _far_pool(arena, F.far_slot2, S, Hkv, WC, D, named)
    for t in farb:
        assert _offset(arena, t[33]) >= F.TWO32 and _offset(arena, t[34]) >= F.TWO32 and _offset(arena, t[2, -1, -1]) < F.TWO31
    far = _play(_pool_layer(WC, farb, S), steps, named)
    _same_records(near, far, ("far to far", dt, D))
    _steps_equal(far, ["step [33, 1]", "step [34, 2]"], "far")
    _unnamed_keep_the_sentinel(nearb, farb, S, named)
    F.assert_untouched(arena, farb, f"fork far to far {dt}")


# ---- 3. the FP8 pool: one byte per element, slot 8 at element and byte 2^32, slots 4 .. 7 in [2^31, 2^32)
from test_gpu_fp8_pool import _row, _snap as _snap8, _stored as _stored8       # noqa: E402

FP8_CASES = [("bf16", 64, 8, 1), ("fp16", 128, 1, 2), ("fp16", 80, 1, 2)]
FP8_NAMED = [8, 1, 5, 2, 6]           # far (2^32), a (near), b (the band); the forks' destinations: near, the band


def _play_fp8(p8, p16, steps, named, scales, dtype):
    """The near run of an FP8 script with its two contracts (tests/fp8_ref.py) checked at every call: a 16-bit twin pool
    p16 takes the same calls - every row a call stores is quant(the twin's row), the state rows are equal; and o is bit
    for bit o of the same call on a 16-bit pool that holds dequant(codes)."""
    rec = [dict(name="start", path=None, o=None, st=p8._dev_state.clone(), c=_content(p8, named), writes=())]
    S, W = p8._dev_state.shape[0], p8.window_size
    for name, fn, writes in steps:
        s8, s16 = _snap8(p8), _snap8(p16)
        pd = _pool_layer(W, [dequant(getattr(p8, n).cpu(), _row(scales, n), dtype).to(DEV) for n in BUFS], S)
        pd._dev_state.copy_(p8._dev_state)
        o8 = fn(p8)
        path = _nat().last_path()
        fn(p16)
        od = fn(pd)
        if o8 is not None:
            assert path.endswith("_kvfp8") and _nat().last_path() == path[:-len("_kvfp8")], (name, path, _nat().last_path())
            assert torch.equal(o8, od), (name, "o differs from the 16-bit step over the dequantised codes", maxdiff(o8, od))
            assert not torch.isnan(o8.float()).any() and o8.any()
        if writes:
            assert _stored8(p8, p16, s8, s16, scales, name) > 0, name
        rec.append(dict(name=name, path=path, o=None if o8 is None else o8.clone(), st=p8._dev_state.clone(),
                        c=_content(p8, named), writes=writes))
    return rec


@pytest.mark.parametrize("dt,D,G,Hkv", FP8_CASES, ids=[f"{p[0]}-d{p[1]}-g{p[2]}" for p in FP8_CASES])
def test_fp8_pool_serving_calls_far_slot(arena16, dt, D, G, Hkv):
    dtype, S = DT[dt], SLOT_S
    scales = ([0.37, 2.0][:Hkv], [0.25, 1.0][:Hkv])
    sv = _Serving(dt, D, G, Hkv, WC, FP8_NAMED[:3], seed=8000 + D)
    steps = sv.steps[:-1] + [("fork", lambda L: L.fork_slots([8, 1], [2, 6]), (2, 6)), sv.steps[-1]]
    p8 = _pool_layer(WC, _near_pool(S, Hkv, WC, D, FP8), S, scales=scales)
    p16 = _pool_layer(WC, _near_pool(S, Hkv, WC, D, dtype), S)
    near = _play_fp8(p8, p16, steps, FP8_NAMED, scales, dtype)                                      # (a): both contracts
    sv.check_states(near, "near")
    arena = _arena(arena16, FP8, F.SENTINEL8)
    assert bool((arena.view(torch.uint8)[:: 1 << 20] == 0x7F).all())
    farb = _far_pool(arena, F.far_slot, S, Hkv, WC, D, FP8_NAMED)
    for t in farb:
        assert _offset(arena, t[8]) >= F.TWO32 and _offset(arena, t[2, -1, -1]) < F.TWO31
        assert all(F.TWO31 <= _offset(arena, t[s]) and _offset(arena, t[s, -1, -1]) < F.TWO32 for s in (5, 6))
    far = _play(_pool_layer(WC, farb, S, scales=scales), steps, FP8_NAMED)
    _same_records(near, far, ("fp8 far_slot", dt, D))                                               # (b), (c)
    assert far[2]["path"].endswith("_ragged_admit_commit_kvfp8") and far[4]["path"] == "ring_commit_path_ragged_slots_kvfp8", \
        [r["path"] for r in far]
    # a step over the forks (2 <- 8, 6 <- 1) is the plain step over their sources, in the far pool
    Lf = _pool_layer(WC, farb, S, scales=scales)
    Lf._dev_state.copy_(far[-1]["st"])
    o_forks = sv.plain(Lf, [2, 5, 6, -1])
    assert torch.equal(o_forks, far[-1]["o"])
    _unnamed_keep_the_sentinel(_near_pool(S, Hkv, WC, D, FP8), farb, S, FP8_NAMED, F.SENTINEL8)
    F.assert_untouched(arena, farb, f"fp8 {dt} {D}", sentinel=F.SENTINEL8)                          # (d)


# ---- 4. the paged pool: far pages behind the table
PAGED = [("bf16", 128, 1, 2), ("fp16", 80, 8, 2)]
WP = 96                               # three table entries per slot: one page of every class (deal_pages)


def _near_paged(S, Hkv, W, D, dtype, table, n_pages):
    """init_pool(page_size=32, num_pages=n_pages) with `table`; every page row holds the sentinel (NaN), as the arena's do"""
    from sink_attention.cache import SinkCacheLayer
    L = SinkCacheLayer(NS, W)
    L.init_pool(S, Hkv, D, dtype, DEV, page_size=PG, num_pages=n_pages)
    L.page_table.copy_(torch.tensor(table, dtype=torch.int32))
    for name in RING:
        getattr(L, name).copy_(F.sentinel_full(getattr(L, name).shape, dtype, DEV))
    return L


def _far_paged(S, Hkv, W, D, dtype, table, pages):
    sinks = [torch.zeros(S, Hkv, NS, D, dtype=dtype, device=DEV) for _ in range(2)]
    return _pool_layer(W, sinks + list(pages), S, table=table)


def _rank_table(tab):
    """the table with every page index replaced by its rank among the mapped ones, and their number"""
    pages = sorted(e for r in tab for e in r if e >= 0)
    return [[pages.index(e) if e >= 0 else e for e in r] for r in tab], len(pages)


def _contig_twin(L):
    """the contiguous twin of a paged pool (tests/paged_ref.py::gather), built before any call"""
    S, Hkv, _, D = L.sink_k.shape
    ring = [PR.gather(getattr(L, name), L.page_table.cpu()) for name in RING]
    tw = _pool_layer(L.window_size, [L.sink_k.clone(), L.sink_v.clone()] + ring, S)
    tw._dev_state.copy_(L._dev_state)
    return tw


def _paged_is_the_twin(rp, rt, what):
    """record of a paged run against the record of the same script on its contiguous twin: bitwise"""
    for a, b in zip(rp, rt):
        w = (what, a["name"])
        if a["path"] is not None:
            assert a["path"].endswith("_paged") and b["path"] == a["path"][:-len("_paged")], (w, a["path"], b["path"])
        assert torch.equal(a["st"], b["st"]), w
        assert a["o"] is None or torch.equal(a["o"], b["o"]), (w, "o")
        for k, x in a["c"].items():
            y = b["c"][k[:2]]
            assert torch.equal(x, y if len(k) == 2 else y[:, k[2] * PG:(k[2] + 1) * PG]), (w, k)


def _mapped_views(pages, tab):
    return [buf[e] for buf in pages for r in tab for e in r if 0 <= e < buf.shape[0]]


def _page_views(arena, pp, Hkv, D):
    return [F.far_view(arena, sp.shape, sp.strides, sp.offset) for sp in pp.specs(Hkv, PG, D)]


@pytest.mark.parametrize("dt,D,G,Hkv", PAGED, ids=[f"{p[0]}-d{p[1]}-g{p[2]}" for p in PAGED])
def test_paged_pool_on_one_large_page_buffer(arena16, dt, D, G, Hkv):
    """The production layout: the whole arena is one K / V page buffer (far_views.page_pool), the table of the three
    named slots holds pages on both sides of 2^31 bytes, of 2^31 elements and of 2^32 bytes, every other page keeps the
    sentinel.  The far run equals the near twin (init_pool, ranks in the table) and the contiguous twin of gather()."""
    dtype, S, named = DT[dt], 4, [3, 1, 2]
    arena = _arena(arena16, dtype)
    pp = F.page_pool(arena.numel(), Hkv * PG * D, arena.element_size())
    tab = [[-1] * (WP // PG) for _ in range(S)]
    for s, row in zip(named, F.deal_pages(pp.picks, 3, WP // PG, pp.p31, pp.p32)):
        tab[s] = row
    sv = _Serving(dt, D, G, Hkv, WP, named, seed=8100 + D)
    rtab, n_map = _rank_table(tab)
    Ln = _near_paged(S, Hkv, WP, D, dtype, rtab, n_map + 2)
    tw = _contig_twin(Ln)
    near = _play(Ln, sv.steps, named)
    sv.check_states(near, "near")
    sv.check_oracle(near, ("paged", dt, D))                                                         # (a)
    twin = _play(tw, sv.steps, named)
    pages = _page_views(arena, pp, Hkv, D)
    for s in named:
        hi, lo, mid = tab[s]
        for buf in pages:
            assert _offset(arena, buf[hi]) >= F.TWO32 and _offset(arena, buf[hi]) // arena.element_size() >= F.TWO31
        assert _offset(arena, pages[0][lo]) < F.TWO31 <= _offset(arena, pages[0][mid]) < F.TWO32    # (a page may straddle its line)
    assert pp.n_pages - 1 in tab[2] and 0 in tab[2]
    for v in _mapped_views(pages, tab):           # every row of a mapped page is NaN until a call stores into it
        assert bool(torch.isnan(v.float()).all())
    far = _play(_far_paged(S, Hkv, WP, D, dtype, tab, pages), sv.steps, named)
    _same_records(near, far, ("paged far pages", dt, D))                                            # (b), (c)
    _paged_is_the_twin(far, twin, ("paged far pages", dt, D))
    for k in far[-1]["c"]:            # every page of the long admission's slot and the first page of every slot was stored into
        if k[0] in RING and (k[1] == named[0] or k[2] == 0):
            assert not torch.equal(far[0]["c"][k], far[-1]["c"][k]), ("never written", k)
    F.assert_untouched(arena, _mapped_views(pages, tab), f"paged {dt} {D}")                         # (d)


@pytest.mark.parametrize("dt,D,G,Hkv", PAGED[:1], ids=["bf16-d128"])
def test_paged_pool_small_entries_times_a_huge_page_stride(arena16, dt, D, G, Hkv):
    """The other factor large: 9 pages on the far_slot geometry, page 8 at 4 GiB."""
    dtype, S, named = DT[dt], 3, [0, 1, 2]
    tab = [[8, 1], [3, 7], [5, 2]]
    sv = _Serving(dt, D, G, Hkv, WC, named, seed=8200 + D, short=True)
    Ln = _near_paged(S, Hkv, WC, D, dtype, tab, 9)
    tw = _contig_twin(Ln)
    near = _play(Ln, sv.steps, named)
    sv.check_states(near, "near")
    sv.check_oracle(near, ("paged far_slot", dt, D))
    twin = _play(tw, sv.steps, named)
    arena = _arena(arena16, dtype)
    pages = F.views(arena, F.far_slot, [(9, Hkv, PG, D)] * 2)
    for buf in pages:
        assert _offset(arena, buf[8]) >= F.TWO32 and _offset(arena, buf[7]) < F.TWO32 and buf.stride(0) * 2 >= 1 << 29
    far = _play(_far_paged(S, Hkv, WC, D, dtype, tab, pages), sv.steps, named)
    _same_records(near, far, ("paged far_slot", dt, D))
    _paged_is_the_twin(far, twin, ("paged far_slot", dt, D))
    assert not torch.equal(far[0]["c"][("window_k", 0, 0)], far[-1]["c"][("window_k", 0, 0)])      # page 8
    assert F.is_sentinel(pages[0][[0, 4, 6]]) and F.is_sentinel(pages[1][[0, 4, 6]])
    F.assert_untouched(arena, _mapped_views(pages, tab), f"paged far_slot {dt}")


@pytest.mark.parametrize("dt,D,G,Hkv", PAGED, ids=[f"{p[0]}-d{p[1]}-g{p[2]}" for p in PAGED])
def test_fork_slots_between_paged_pools_and_across_the_lines(arena16, dt, D, G, Hkv):
    """Inside the large pool from a slot whose pages all lie below 2^31 bytes to one whose pages all lie past 2^32; out
    of it into an ordinary paged pool and from there back into pages of the band.  The destinations are mapped first."""
    dtype, S = DT[dt], 4
    arena = _arena(arena16, dtype)
    pp = F.page_pool(arena.numel(), Hkv * PG * D, arena.element_size())
    lo, mid, hi = ([p for p in pp.picks if a <= p < b] for a, b in ((0, pp.p31), (pp.p31, pp.p32), (pp.p32, pp.n_pages)))
    tab = [[lo[1], lo[2], lo[0]], [hi[2], hi[0], hi[1]], [mid[2], mid[0], mid[1]], [-1, -1, -1]]
    tab_n = [[-1, -1, -1], [5, 0, 3], [2, 4, 1], [-1, -1, -1]]
    fk = _Forks(dt, D, G, Hkv, 0, 2, seed=8300 + D, W=WP, both_bodies=False)
    steps = [fk.prefill, fk.fork([0], [1], (1,)), fk.over([0, 2]), fk.over([1, 2])]
    steps_n = [fk.fork([1, 2], [1, 2], (1, 2), partner=True), fk.over([1, 2])]
    steps_back = [fk.fork([1], [2], (2,), partner=True), fk.over([2, -1]), fk.over([0, -1])]
    pages = _page_views(arena, pp, Hkv, D)
    assert all(_offset(arena, pages[0][e]) < F.TWO31 for e in tab[0])        # (the page under a line may straddle it)
    assert all(_offset(arena, buf[e]) >= F.TWO32 for e in tab[1] for buf in pages)
    assert all(F.TWO31 <= _offset(arena, pages[0][e]) < F.TWO32 for e in tab[2])
    rtab, n_map = _rank_table(tab)
    recs = []
    for A in (_near_paged(S, Hkv, WP, D, dtype, rtab, n_map + 2), _far_paged(S, Hkv, WP, D, dtype, tab, pages)):
        N = _near_paged(S, Hkv, WP, D, dtype, tab_n, 6)
        A.partner, N.partner = N, A
        recs.append((_play(A, steps, [0, 1, 2]), _play(N, steps_n, [1, 2]), _play(A, steps_back, [0, 1, 2])))
    (a1, n1, b1), (a2, n2, b2) = recs
    fk.check_oracle(a1[3]["o"], ("paged fork sources", dt, D))
    for x, y, what in ((a1, a2, "inside the pool"), (n1, n2, "out of the pool"), (b1, b2, "back into the pool")):
        _same_records(x, y, ("paged fork", what, dt, D))
    assert a2[2]["path"] == "ring_copy_slots_paged" and a2[2]["st"][1].tolist() == [NS, WP, 5, NS + WP + 14]
    assert torch.equal(a2[3]["o"], a2[4]["o"]) and torch.equal(n2[2]["o"], a2[3]["o"])             # forks step as their sources
    assert torch.equal(b2[2]["o"], b2[3]["o"])
    F.assert_untouched(arena, _mapped_views(pages, tab), f"paged fork {dt} {D}")


def test_a_store_to_an_unmapped_entry_of_the_far_pool_is_dropped(arena16):
    """Entries -1 and n_pages in the row of a slot of the large pool: 40 tokens whose ring slots lie on them are dropped,
    the state row advances, no word of the arena changes (n_pages times the page stride is an address inside the arena's
    last pages' neighbourhood, so only the arena check tells a dropped store from a misplaced one); the next tokens reach
    the third, mapped entry."""
    dt, D, G, Hkv, S = "bf16", 128, 1, 2, 2
    dtype = DT[dt]
    arena = _arena(arena16, dtype)
    pp = F.page_pool(arena.numel(), Hkv * PG * D, 2)
    row = F.deal_pages(pp.picks, 3, WP // PG, pp.p31, pp.p32)[0]
    tab = [row, [-1, -1, -1]]
    g = torch.Generator().manual_seed(8400)
    kp, vp = (_rows(g, dtype, Hkv, NS + WP, D).to(DEV) for _ in range(2))
    kc, vc = (_rows(g, dtype, Hkv, 40, D).to(DEV) for _ in range(2))

    def prefill(L):
        L.prefill_slots(kp, vp, [0, NS + WP], [0])

    def unmap(L):
        L.page_table[0, 0], L.page_table[0, 1] = -1, L.window_k.shape[0]

    commit = lambda n: lambda L: L.commit_packed_dyn(kc[:, :, :n], vc[:, :, :n], [0, n], [0], [n])
    steps = [("prefill_slots", prefill, (0,)), ("unmap", unmap, ()), ("commit 40", commit(40), ()), ("commit 30", commit(30), (0,))]
    rtab, n_map = _rank_table(tab)
    near = _play(_near_paged(S, Hkv, WP, D, dtype, rtab, n_map + 2), steps, [0])
    pages = _page_views(arena, pp, Hkv, D)
    assert _offset(arena, pages[0][row[0]]) >= F.TWO32
    Lf = _far_paged(S, Hkv, WP, D, dtype, tab, pages)
    far = _play(Lf, steps[:2], [0])
    kept = [(buf, e, buf[e].clone()) for buf in pages for e in row[:2]]
    far += _play(Lf, steps[2:], [0])[1:]
    _same_records(near, far, "unmapped entries")
    assert Lf.page_table[0].tolist() == [-1, pp.n_pages, row[2]]
    assert far[3]["st"][0].tolist() == [NS, WP, 40, NS + WP + 40] and far[4]["st"][0].tolist() == [NS, WP, 70, NS + WP + 70]
    assert far[3]["path"] == "ring_commit_path_ragged_slots_paged"
    for buf, e, t in kept:
        assert torch.equal(t, buf[e]), ("a dropped store reached page", e)
    changed = (far[4]["c"][("window_k", 0, 2)] != far[2]["c"][("window_k", 0, 2)]).any(dim=-1)
    assert changed[:, :6].all() and not changed[:, 6:].any()          # ring slots 64 .. 69: rows 0 .. 5 of the third page
    F.assert_untouched(arena, _mapped_views(pages, tab), "unmapped entries")
