"""Inputs, reference and case table for the backward preprocess pass: Delta[b,h,i] = sum_e dO O and the gradient of the
learnable sink logit, ds_aux[h] = - sum_{b,i} exp(s_aux[h] - lse[b,h,i]) Delta[b,h,i] (csrc/sfa_generic.hip:
bwd_preprocess_vec_kernel<T, LPR>, bwd_preprocess_kernel<T>, dsaux_reduce_kernel; launched by bwd_preprocess).

Why randn cannot judge ds_aux: its terms have random signs, so |ds_aux| is a small remainder of a large sum and the honest
bound of that sum (u sum |terms|) is wider than what a lost 64-row block moves.  Here every term of one ROW CLASS has the
same sign and every other row contributes exactly nothing:

  q, k, v     randn rounded to the dtype, a short window (16 to 40 keys) so that the per-row bound stays tight
  s_aux[h]    the median over (b, i) of the LSE of the same problem WITHOUT s_aux (p_aux = exp(s_aux - lse) about 1/2) plus a
              per-head offset within +-2 nat, distinct for every head, the two heads of a pair (h, h ^ 1) at least 2 nat apart:
              a kernel that takes a neighbour's s_aux or partial is off by a factor, not by noise
  dO          sign(o_ref) (+-1, exact in every dtype) on the rows of the class and exactly 0 elsewhere: Delta_i = sum_e |o_ie|
              on the class; elsewhere Delta and the row's ds_aux term are exactly 0 in the kernel too (delta == 0)

Row classes come from the launch arithmetic (PRE_ROWS = 64 rows per workgroup, 16 per wave): all, tail (the last 64-row
block, partial unless 64 | N), last (row N - 1, the row the clamped loads re-read), row0, wave1 / wave3 (rows 16 w .. 16 w + 15
of block 0 and of the last full block), block (one block in the middle), batch, head, and seq<s> for packs.

Reference (fp64, oracle/sink_oracle.py on the exact inputs upcast): Delta_ref, the terms t = -p_aux Delta_ref, and the
bound terms a[b,h,i] = sum_e |dO_ie| sum_j p_ij |v_je| (the oracle forward run with |v| in place of v).  Bounds, with u the
unit roundoff of the dtype (tests/util.py::UNIT_ROUNDOFF; fp32: 2^-22):

  Delta, row by row   |got - ref| <= 4 u a_i + u |ref_i|
  ds_aux[h]           |got - ref| <= 4 u A_h + u |ref_h|,   A_h = sum_{b, i in class} p_aux a

The 4 is the argument of util.assert_within_sum_bound, not fitted to a kernel: the forward packs P to the dtype once (o_e
moves by at most u sum_j p |v|) and rounds O once (u |o_e|, no more than the same sum): 2 u a at worst, and a twofold
margin.  f32 accumulation, expf and the f32 LSE are negligible beside it for the 16-bit types.  fp32: the LSE is stored in
f32, which moves p_aux by |lse| 2^-24 (lse is 3 to 6 here: up to 2^-22 relative), expf and O's own rounding add 2^-23
each; under 2^-21 together, against a bound of at least 5 * 2^-22 |ref|.

Where Delta is read: bwd_layout (csrc/sfa_api.hip) puts Delta at byte 0 of the backward workspace, f32 [B, Hq, N_q], and the
ds_aux partials f32 [B, Hq, ceil(N_q / 64)] at the next 256-byte boundary.  sfa_bwd_varlen carves with the same function
for B = 1, N = total rows of the pack.  layout() restates it; tests/test_dsaux_inputs.py pins the sizes on the library.

No GPU and no product import at module level; the raw calls at the end import sink_attention when called."""
import functools

import torch

from util import UNIT_ROUNDOFF, oracle_fwd, rand

PRE_ROWS = 64               # kPreRows: rows of one workgroup of the pass
WAVE_ROWS = 16              # rows of one of its four waves
U = {**UNIT_ROUNDOFF, torch.float32: 2.0 ** -22}
DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
SFA_DTYPE = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}      # include/sfa.h
MFMA_DIMS = (32, 64, 80, 96, 128, 256)                                   # bwd_mfma_supported (16-bit dtypes)
FACTOR = 4.0


def cdiv(a, b):
    return -(-a // b)


def align256(x):
    return (x + 255) & ~255


# ------------------------------------------------------------------------------------------------ launch arithmetic
def preprocess_vectorised(dtype, D, rows16=True):
    """bwd_preprocess_vectorised: 16-bit, D % 8 == 0, D <= 128, O and dO with 16-byte aligned base and strides"""
    return dtype != torch.float32 and D % 8 == 0 and D <= 128 and rows16


def lanes_per_row(D):
    """LPR of the vec kernel (bwd_preprocess): lanes x 16 bytes that hold one row"""
    return 4 if D <= 32 else (8 if D <= 64 else 16)


def rows16(t):
    """rows16() of csrc/sfa_generic.hip on a 16-bit [B, H, N, D] tensor"""
    return t.data_ptr() % 16 == 0 and all((t.stride(i) * 2) % 16 == 0 for i in range(3))


def layout(B, Hq, N):
    """bwd_layout: byte offsets of Delta and of the ds_aux partials, and the end of the two regions"""
    delta_off = 0
    part_off = delta_off + align256(4 * B * Hq * N)
    return dict(delta=delta_off, part=part_off, nblk=cdiv(N, PRE_ROWS),
                end=part_off + align256(4 * B * Hq * cdiv(N, PRE_ROWS)))


# ------------------------------------------------------------------------------------------------ the cases
# kernel: which preprocess kernel the rule picks (vec16 / vec8 / vec4 = the vec kernel at that LPR; scalar); bwd: the family the
# rest of the backward runs in ("mfma" / "generic").  layout: contig; o_bnhd / do_bnhd / both_bnhd ([B, N, H, D] memory); o_off8 /
# do_off8 (a [..., 4:4+D] slice of a wider buffer: rows 8 bytes off a 16-byte boundary).  W stays at 16 to 40 keys.
def _c(B, Hq, Hkv, N, D, dt, ns, W, kernel, bwd, layout="contig", Nk=None, cu=None):
    return dict(B=B, Hq=Hq, Hkv=Hkv, N=N, D=D, dtype=DT[dt], ns=ns, W=W, kernel=kernel, bwd=bwd, layout=layout,
                Nk=N if Nk is None else Nk, cu=cu)


PACK_CU = (0, 70, 71, 71, 200, 261)        # a one-row and an empty sequence
CASES = {
    # vec kernel, 16 lanes per row
    "d128_bf16_n517": _c(2, 8, 2, 517, 128, "bf16", 2, 40, "vec16", "mfma"),
    "d80_fp16_n133": _c(3, 4, 1, 133, 80, "fp16", 0, 24, "vec16", "mfma"),
    "d96_bf16_n65": _c(1, 8, 1, 65, 96, "bf16", 1, 16, "vec16", "mfma"),
    "d72_fp16_n63": _c(2, 2, 2, 63, 72, "fp16", 2, 16, "vec16", "generic"),
    "d128_fp16_n64": _c(1, 2, 1, 64, 128, "fp16", 0, 16, "vec16", "mfma"),
    "d128_bf16_n1": _c(3, 4, 2, 1, 128, "bf16", 1, 16, "vec16", "mfma"),
    "d128_bf16_n2050": _c(2, 2, 1, 2050, 128, "bf16", 4, 32, "vec16", "mfma"),     # 33 partials per (b, h)
    # 8 lanes per row; D = 40, 56: inactive chunks
    "d64_bf16_n69": _c(3, 4, 2, 69, 64, "bf16", 2, 16, "vec8", "mfma"),
    "d64_fp16_n17": _c(2, 8, 8, 17, 64, "fp16", 0, 16, "vec8", "mfma"),
    "d40_bf16_n133": _c(1, 4, 2, 133, 40, "bf16", 1, 24, "vec8", "generic"),
    "d56_fp16_n15": _c(2, 2, 1, 15, 56, "fp16", 0, 16, "vec8", "generic"),
    # 4 lanes per row
    "d32_bf16_n65": _c(2, 4, 1, 65, 32, "bf16", 2, 16, "vec4", "mfma"),
    "d24_fp16_n16": _c(1, 2, 2, 16, 24, "fp16", 0, 16, "vec4", "generic"),
    "d16_bf16_n63": _c(3, 2, 1, 63, 16, "bf16", 1, 16, "vec4", "generic"),
    "d8_fp16_n69": _c(1, 8, 4, 69, 8, "fp16", 0, 24, "vec4", "generic"),
    # scalar kernel
    "f32_d16_n69": _c(1, 4, 2, 69, 16, "fp32", 2, 16, "scalar", "generic"),
    "f32_d64_n133": _c(2, 2, 1, 133, 64, "fp32", 0, 24, "scalar", "generic"),
    "f32_d100_n17": _c(3, 2, 2, 17, 100, "fp32", 1, 16, "scalar", "generic"),
    "d20_bf16_n65": _c(2, 4, 4, 65, 20, "bf16", 0, 16, "scalar", "generic"),
    "d256_bf16_n133": _c(1, 4, 1, 133, 256, "bf16", 2, 32, "scalar", "mfma"),
    # unaligned 16-bit rows.  An unaligned O: the forward takes the exact-f32 kernels (fwd_mfma: slice_ok(o) fails), the
    # backward stays with the MFMA kernels (slices_ok does not look at O) but its preprocess is the scalar one, and the row
    # constants are then made by the MFMA family's own pass.  An unaligned dO: slices_ok fails, the whole backward is generic.
    "d64_bf16_o_off8": _c(2, 4, 2, 69, 64, "bf16", 2, 16, "scalar", "mfma", layout="o_off8"),
    "d64_fp16_do_off8": _c(2, 4, 2, 69, 64, "fp16", 0, 16, "scalar", "generic", layout="do_off8"),
    # N_q < N_kv (MFMA path only): Delta and LSE are indexed by N_q
    "d128_bf16_nq37_nk101": _c(2, 4, 2, 37, 128, "bf16", 2, 24, "vec16", "mfma", Nk=101),
    # strided O and dO
    "d128_bf16_o_bnhd": _c(2, 4, 2, 133, 128, "bf16", 2, 24, "vec16", "mfma", layout="o_bnhd"),
    "d64_fp16_do_bnhd": _c(2, 4, 1, 69, 64, "fp16", 0, 16, "vec8", "mfma", layout="do_bnhd"),
    "d80_bf16_both_bnhd": _c(3, 2, 2, 65, 80, "bf16", 1, 16, "vec16", "mfma", layout="both_bnhd"),
    # the packed call: the pass runs row-wise over the pack (B = 1, N = T)
    "pack_d128_bf16": _c(1, 4, 2, PACK_CU[-1], 128, "bf16", 2, 24, "vec16", "mfma", cu=PACK_CU),
    "pack_d80_fp16": _c(1, 4, 1, PACK_CU[-1], 80, "fp16", 0, 16, "vec16", "mfma", cu=PACK_CU),
}


def expected_kernel(c):
    """the preprocess kernel bwd_preprocess picks for the case, from the rule alone"""
    aligned = c["layout"] not in ("o_off8", "do_off8")
    if not preprocess_vectorised(c["dtype"], c["D"], aligned):
        return "scalar"
    return "vec%d" % lanes_per_row(c["D"])


def expected_bwd(c):
    """family of the rest of the backward: bwd_mfma_supported, and bwd_mfma's own fall-back for an unaligned dO"""
    mfma = c["dtype"] != torch.float32 and c["D"] in MFMA_DIMS and c["layout"] != "do_off8"
    return "mfma" if mfma else "generic"


# ------------------------------------------------------------------------------------------------ inputs and reference
def head_offsets(Hq):
    """distinct offsets within +-2 nat; even heads take the lower half, odd heads the upper: h and h ^ 1 differ by > 2 nat"""
    if Hq == 1:
        return torch.zeros(1, dtype=torch.float64)
    base = torch.linspace(-2.0, 2.0, Hq, dtype=torch.float64)
    rank = [h // 2 if h % 2 == 0 else (Hq + 1) // 2 + h // 2 for h in range(Hq)]
    return base[torch.tensor(rank)]


def _forward(q, k, v, ns, W, sa, cu):
    """fp64 oracle forward; packs: sequence by sequence"""
    if cu is None:
        Nq, Nk = q.shape[2], k.shape[2]
        return oracle_fwd(q, k, v, ns, W, sa, banded=(Nq == Nk and Nq > 256))
    o = torch.zeros(q.shape, dtype=torch.float64)
    lse = torch.zeros(q.shape[:3], dtype=torch.float64)
    for a, b in zip(cu[:-1], cu[1:]):
        if b > a:
            o[:, :, a:b], lse[:, :, a:b] = oracle_fwd(q[:, :, a:b], k[:, :, a:b], v[:, :, a:b], ns, W, sa, banded=False)
    return o, lse


def row_classes(B, Hq, N, cu=None):
    """name -> bool mask [B, Hq, N]; empty classes are left out"""
    nblk = cdiv(N, PRE_ROWS)
    i = torch.arange(N)
    rows = {"all": i >= 0, "tail": i >= (nblk - 1) * PRE_ROWS, "last": i == N - 1, "row0": i == 0}
    full = N // PRE_ROWS                                    # full blocks
    for w in (1, 3):
        m = (i >= w * WAVE_ROWS) & (i < (w + 1) * WAVE_ROWS)
        if full >= 1:
            r0 = (full - 1) * PRE_ROWS + w * WAVE_ROWS
            m = m | ((i >= r0) & (i < r0 + WAVE_ROWS))
        rows["wave%d" % w] = m
    if nblk >= 2:
        j = nblk // 2
        rows["block"] = (i >= j * PRE_ROWS) & (i < (j + 1) * PRE_ROWS)
    out = {n: m.view(1, 1, N).expand(B, Hq, N).clone() for n, m in rows.items()}
    if B >= 2:
        out["batch"] = torch.zeros(B, Hq, N, dtype=torch.bool)
        out["batch"][B - 1] = True
    if Hq >= 2:
        out["head"] = torch.zeros(B, Hq, N, dtype=torch.bool)
        out["head"][:, 1] = True
    if cu is not None:
        for s, (a, b) in enumerate(zip(cu[:-1], cu[1:])):
            out["seq%d" % s] = ((i >= a) & (i < b)).view(1, 1, N).expand(B, Hq, N).clone()
    return {n: m for n, m in out.items() if m.any()}


def block_classes(B, Hq, N):
    """one class per 64-row block (the additivity test)"""
    i = torch.arange(N)
    return [((i >= j * PRE_ROWS) & (i < (j + 1) * PRE_ROWS)).view(1, 1, N).expand(B, Hq, N).clone()
            for j in range(cdiv(N, PRE_ROWS))]


def build(B, Hq, Hkv, N, D, dtype, ns, W, Nk=None, cu=None, seed=7):
    """The problem of one case: inputs in the dtype and everything of the fp64 reference that does not depend on the class."""
    Nk = N if Nk is None else Nk
    g = torch.Generator().manual_seed(seed)
    q, k, v = rand((B, Hq, N, D), g, dtype), rand((B, Hkv, Nk, D), g, dtype), rand((B, Hkv, Nk, D), g, dtype)
    _, lse0 = _forward(q, k, v, ns, W, None, cu)
    med = lse0.double().permute(1, 0, 2).reshape(Hq, -1).median(-1).values
    s_aux = (med + head_offsets(Hq)).float()                       # what the kernels are given: f32
    o, lse = _forward(q, k, v, ns, W, s_aux, cu)
    pv, _ = _forward(q, k, v.abs(), ns, W, s_aux, cu)              # sum_j p_ij |v_je|
    sign = torch.sign(o).to(dtype)
    p_aux = torch.exp(s_aux.double().view(1, Hq, 1) - lse.double())
    return dict(q=q, k=k, v=v, s_aux=s_aux, o=o.double(), lse=lse.double(), sign=sign, p_aux=p_aux,
                delta_all=(o.double() * sign.double()).sum(-1),                    # sum_e |o_ie|
                a_all=(sign.double().abs() * pv.double()).sum(-1),
                pv=pv.double(), classes=row_classes(B, Hq, N, cu), dtype=dtype, u=U[dtype], cu=cu,
                shape=(B, Hq, Hkv, N, Nk, D), ns=ns, W=W)


@functools.lru_cache(maxsize=None)
def problem(name):
    """build() of a case of the table, computed once per process and shared (treat it as read-only)"""
    c = CASES[name]
    return build(c["B"], c["Hq"], c["Hkv"], c["N"], c["D"], c["dtype"], c["ns"], c["W"], Nk=c["Nk"],
                 cu=None if c["cu"] is None else list(c["cu"]))


def make_do(pr, mask):
    """dO of a class: sign(o_ref) on its rows, exactly 0 elsewhere"""
    return pr["sign"] * mask.unsqueeze(-1).to(pr["dtype"])


def reference(pr, mask=None, do=None):
    """fp64 Delta [B,Hq,N] and ds_aux [Hq] with their tolerances (tol_delta row by row, tol_ds per head).  mask: a row class
    (dO = make_do); do: any other dO of the dtype (then the terms may cancel; the bound has the same form)."""
    u = pr["u"]
    if do is None:
        m = mask.double()
        delta, a = pr["delta_all"] * m, pr["a_all"] * m
    else:
        delta = (pr["o"] * do.double()).sum(-1)
        a = (do.double().abs() * pr["pv"]).sum(-1)
    ds = -(pr["p_aux"] * delta).sum((0, 2))
    A = (pr["p_aux"] * a).sum((0, 2))
    return dict(delta=delta, a=a, ds=ds, A=A, tol_delta=FACTOR * u * a + u * delta.abs(), tol_ds=FACTOR * u * A + u * ds.abs())


def ratio(got, ref, tol):
    """largest |got - ref| / tol; an error where the tolerance is 0 (a row or head outside the class) is inf, NaN is inf"""
    err = (got.detach().double().cpu() - ref).abs()
    r = torch.where(err > 0, err / tol, torch.zeros_like(err))
    r = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), r)
    return r.max().item() if r.numel() else 0.0


def ratios(pr, got_delta, got_ds, mask=None, do=None):
    """(Delta ratio, ds_aux ratio) of a result against reference()"""
    ref = reference(pr, mask, do)
    return ratio(got_delta, ref["delta"], ref["tol_delta"]), ratio(got_ds, ref["ds"], ref["tol_ds"])


# ------------------------------------------------------------------------------------------------ raw calls (GPU)
def _nan(shape, dt, dev):
    return torch.full(shape, float("nan"), device=dev, dtype=dt)


def _alloc_o(c, shape, dt, dev):
    """NaN-filled O in the case's memory layout, as a [B, H, N, D] view"""
    B, H, N, D = shape
    if c["layout"] in ("o_bnhd", "both_bnhd"):
        return _nan((B, N, H, D), dt, dev).transpose(1, 2)
    if c["layout"] == "o_off8":
        return _nan((B, H, N, D + 8), dt, dev)[..., 4:4 + D]
    return _nan(shape, dt, dev)


def place_do(c, do):
    """dO (device, contiguous) moved into the case's memory layout"""
    if c["layout"] in ("do_bnhd", "both_bnhd"):
        return do.transpose(1, 2).contiguous().transpose(1, 2)
    if c["layout"] == "do_off8":
        buf = torch.zeros(do.shape[:3] + (do.shape[3] + 8,), device=do.device, dtype=do.dtype)
        buf[..., 4:4 + do.shape[3]] = do
        return buf[..., 4:4 + do.shape[3]]
    return do


def raw_fwd(c, q, k, v, s_aux):
    """sfa_fwd / sfa_fwd_varlen through the C ABI into a NaN-filled O (the case's layout) and LSE.  Returns a state dict."""
    from sink_attention import _native as N
    lib = N.lib()
    B, Hq, Nq, D = q.shape
    st = dict(c=c, q=q, k=k, v=v, s_aux=s_aux, o=_alloc_o(c, q.shape, q.dtype, q.device),
              lse=_nan((B, Hq, Nq), torch.float32, q.device), scale=D ** -0.5, cu=None)
    stream = N.stream_ptr(q.device)
    if c["cu"] is None:
        N.check(lib.sfa_fwd(N.desc(q), N.desc(k), N.desc(v), N.desc(st["o"]), st["lse"].data_ptr(), s_aux.data_ptr(),
                            c["ns"], c["W"], st["scale"], 0, stream), "sfa_fwd")
    else:
        cu = torch.tensor(c["cu"], dtype=torch.int32, device=q.device)
        st.update(cu=cu, max_seqlen=max(b - a for a, b in zip(c["cu"][:-1], c["cu"][1:])))
        N.check(lib.sfa_fwd_varlen(N.desc(q), N.desc(k), N.desc(v), N.desc(st["o"]), st["lse"].data_ptr(), s_aux.data_ptr(),
                                   cu.data_ptr(), cu.numel() - 1, st["max_seqlen"], c["ns"], c["W"], st["scale"], 0, stream),
                "sfa_fwd_varlen")
    st["fwd_path"] = N.last_path()
    return st


def raw_bwd(st, do, refused=False):
    """sfa_bwd / sfa_bwd_varlen on the state of raw_fwd with dQ, dK, dV and ds_aux NaN-filled and every byte of a fresh
    workspace 0xFF.  Returns ds_aux [Hq] and Delta [B, Hq, N_q] as read from the start of the workspace (layout()), the
    partials region, and sfa_last_path().  refused: the call must return SFA_ERR_UNSUPPORTED (status and workspace come back too)."""
    from sink_attention import _native as N
    lib = N.lib()
    c, q, k, v = st["c"], st["q"], st["k"], st["v"]
    B, Hq, Nq, D = q.shape
    Hkv = k.shape[1]
    dev = q.device
    dq, dk, dv = _nan(q.shape, q.dtype, dev), _nan(k.shape, k.dtype, dev), _nan(v.shape, v.dtype, dev)
    ds = _nan((Hq,), torch.float32, dev)
    flags = N.bwd_flags()
    n_ws = int(lib.sfa_bwd_workspace_bytes(B, Hq, Hkv, Nq, D, N.SFA_DTYPE[q.dtype], c["ns"], c["W"], flags))
    lay = layout(B, Hq, Nq)
    assert n_ws >= lay["end"], (n_ws, lay)
    ws = torch.full((max(n_ws, 256),), 0xFF, dtype=torch.uint8, device=dev)
    stream = N.stream_ptr(dev)
    if st["cu"] is None:
        status = lib.sfa_bwd(N.desc(q), N.desc(k), N.desc(v), N.desc(st["o"]), N.desc(do), st["lse"].data_ptr(),
                             st["s_aux"].data_ptr(), N.desc(dq), N.desc(dk), N.desc(dv), ds.data_ptr(), ws.data_ptr(),
                             ws.numel(), c["ns"], c["W"], st["scale"], flags, stream)
    else:
        cu = st["cu"]
        status = lib.sfa_bwd_varlen(N.desc(q), N.desc(k), N.desc(v), N.desc(st["o"]), N.desc(do), st["lse"].data_ptr(),
                                    st["s_aux"].data_ptr(), N.desc(dq), N.desc(dk), N.desc(dv), ds.data_ptr(), cu.data_ptr(),
                                    cu.numel() - 1, st["max_seqlen"], ws.data_ptr(), ws.numel(), c["ns"], c["W"], st["scale"],
                                    flags, stream)
    if refused:
        assert status == -2, status                                  # SFA_ERR_UNSUPPORTED
    else:
        N.check(status, "sfa_bwd")
    path = N.last_path()
    torch.cuda.synchronize(dev)
    n = B * Hq * Nq
    delta = ws[lay["delta"]:lay["delta"] + 4 * n].view(torch.float32).view(B, Hq, Nq).clone()
    part = ws[lay["part"]:lay["part"] + 4 * B * Hq * lay["nblk"]].view(torch.float32).view(B, Hq, lay["nblk"]).clone()
    return dict(ds_aux=ds, delta=delta, part=part, bwd_path=path, dq=dq, dk=dk, dv=dv, ws=ws, status=status)
