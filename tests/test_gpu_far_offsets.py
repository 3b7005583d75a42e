"""GPU: the same call twice - on ordinary contiguous tensors ("near") and on views of one large arena whose strides put
the operands past 2^31 elements, 2^31 bytes or 2^32 bytes ("far", tests/far_views.py).  Every case asserts

  (a) the near result against the fp64 oracle at the suite's tolerances (bf16 / fp16: O 2e-2, gradients 1.5e-1; fp32:
      2e-5 / 2e-4; decode: TOL of tests/test_gpu_decode_multi.py),
  (b) far == near bitwise, for every output,
  (c) the same sfa_last_path() in both runs - or, where the library documents another kernel for the far layout (the
      generic path behind slice_ok(), or SFA_ERR_UNSUPPORTED with nothing written), exactly that,
  (d) the rest of the arena still holds its sentinel: no store landed at a truncated address.

The problems are small; only their addresses are large.  One arena per module (4.1 GiB), every case re-fills it."""
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


def _arena(arena16, dtype):
    a = arena16.view(dtype)
    F.fill_sentinel(a)
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
