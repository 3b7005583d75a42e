"""Shared helpers for the GPU parity tests."""
import math

import torch

from oracle import sink_oracle as O


def rand(shape, seed_gen, dtype, scale=1.0):
    """CPU-generator randn (reproducible everywhere), rounded to ``dtype``."""
    return (torch.randn(*shape, generator=seed_gen, dtype=torch.float32) * scale).to(dtype)


def make_qkv(B, Hq, Hkv, N, D, dtype, seed=42):
    g = torch.Generator().manual_seed(seed)
    q = rand((B, Hq, N, D), g, dtype)
    k = rand((B, Hkv, N, D), g, dtype)
    v = rand((B, Hkv, N, D), g, dtype)
    return q, k, v, g


def oracle_fwd(q, k, v, ns, W, s_aux=None, banded=None):
    """fp64 oracle on the exact low-precision inputs (upcast)."""
    N = q.shape[2]
    if banded is None:
        banded = N > 1024
    fn = O.sink_attention_banded if banded else O.sink_attention_dense
    o, lse = fn(q.cpu(), k.cpu(), v.cpu(), ns, W, None if s_aux is None else s_aux.cpu().float())
    return o, lse


def oracle_bwd(q, k, v, do, ns, W, s_aux=None, banded=None, bounds=False):
    """dQ, dK, dV, ds_aux in fp64; bounds=True: also A_K, A_V, the per-element sums assert_within_sum_bound takes, every
    visible pair counted at least at the smallest normal number of q.dtype (fp16: 2^-14; bf16: 2^-126, nothing)"""
    N = q.shape[2]
    if banded is None:
        banded = N > 1024
    fn = O.sink_attention_bwd_banded if banded else O.sink_attention_bwd_dense
    sa = None if s_aux is None else s_aux.cpu().float()
    if not bounds:
        return fn(q.cpu(), k.cpu(), v.cpu(), do.cpu(), ns, W, sa)
    return fn(q.cpu(), k.cpu(), v.cpu(), do.cpu(), ns, W, sa, bounds=True, tiny=torch.finfo(q.dtype).tiny)


def device_oracle(q, k, v, do, ns, W, s_aux, cu=None):
    """fp64 oracle over the WHOLE tensor on q.device: O, LSE, dQ, dK, dV, ds_aux and the sum-bound terms A_K, A_V
    (bounds=True, tiny of q.dtype), one (sequence, batch, KV head) unit at a time so that the intermediates stay small.  The
    same functions as oracle_fwd / oracle_bwd, banded above 1024 rows.  cu: cu_seqlens of a packed batch [1, H, T, D]
    (LSE comes back as [1, Hq, T]); s_aux [Hq] or None."""
    dev, f64 = q.device, torch.float64
    B, Hq, _, D = q.shape
    Hkv = k.shape[1]
    g = Hq // Hkv
    tiny = torch.finfo(q.dtype).tiny
    o, dq = (torch.zeros(q.shape, dtype=f64, device=dev) for _ in range(2))
    dk, dv, a_k, a_v = (torch.zeros(k.shape, dtype=f64, device=dev) for _ in range(4))
    lse = torch.full(q.shape[:3], float("-inf"), dtype=f64, device=dev)
    dsa = None if s_aux is None else torch.zeros(Hq, dtype=f64, device=dev)
    seqs = [(0, q.shape[2])] if cu is None else [(int(a), int(b)) for a, b in zip(cu[:-1], cu[1:]) if b > a]
    for r0, r1 in seqs:
        banded = r1 - r0 > 1024
        fwd = O.sink_attention_banded if banded else O.sink_attention_dense
        bwd = O.sink_attention_bwd_banded if banded else O.sink_attention_bwd_dense
        for b in range(B):
            for hk in range(Hkv):
                hq = slice(hk * g, (hk + 1) * g)
                uq = (slice(b, b + 1), hq, slice(r0, r1))
                uk = (slice(b, b + 1), slice(hk, hk + 1), slice(r0, r1))
                sa = None if s_aux is None else s_aux[hq].float()
                o[uq], lse[uq] = fwd(q[uq], k[uk], v[uk], ns, W, sa)
                r = bwd(q[uq], k[uk], v[uk], do[uq], ns, W, sa, bounds=True, tiny=tiny)
                dq[uq], dk[uk], dv[uk], a_k[uk], a_v[uk] = r[0], r[1], r[2], r[4], r[5]
                if dsa is not None:
                    dsa[hq] += r[3]
    return o, lse, dq, dk, dv, dsa, a_k, a_v


def probe_reference(pr, ns, W):
    """fp64 oracle of one dense probe (tests/probe_inputs.py::dense_probe): o, lse, (dq, dk, dv, ds_aux, A_K, A_V).  Shared
    by tests/test_gpu_mask_edges.py and the CPU proofs of tests/test_probe_inputs.py, so that the bound terms the GPU
    assertion uses are the ones whose discrimination is proved."""
    Nq, Nk = pr["q"].shape[2], pr["k"].shape[2]
    banded = Nq == Nk and Nq > 1024            # (the banded oracle walks N_q = N_kv only)
    o, lse = oracle_fwd(pr["q"], pr["k"], pr["v"], ns, W, pr["s_aux"], banded=banded)
    return o, lse, oracle_bwd(pr["q"], pr["k"], pr["v"], pr["do"], ns, W, pr["s_aux"], banded=banded, bounds=True)


def maxdiff(a, b):
    if a.numel() == 0:
        return 0.0
    return (a.detach().double().cpu() - b.detach().double().cpu()).abs().max().item()


def assert_close(actual, expected, atol, rtol, what=""):
    e = expected.detach().double()                  # compared where the reference lives (device_oracle: on the GPU)
    a = actual.detach().to(e.device).double()
    err = (a - e).abs()
    tol = atol + rtol * e.abs()
    bad = err > tol
    assert not bad.any(), (f"{what}: {int(bad.sum())}/{bad.numel()} elements out of tolerance "
                           f"(atol={atol}, rtol={rtol}); max abs err {err.max().item():.3e}")


# tolerances of the dense mask-edge probe tests (tests/test_gpu_mask_edges.py::test_dense_mask_edges and, imported from
# here, tests/test_gpu_sliding.py): O and dQ atol = rtol; dK / dV and ds_aux scale with max(1, max |ref|); LSE as
# tests/test_gpu_softmax_range.py
PROBE_TOL_O = {torch.bfloat16: 2e-2, torch.float16: 1e-2}
PROBE_TOL_DQ = 5e-2
PROBE_TOL_DKDV = 5e-2
PROBE_TOL_DS_AUX = 5e-2
PROBE_TOL_LSE = 5e-3


# unit roundoff of the storage dtype: round-to-nearest moves a value by at most u |value|
UNIT_ROUNDOFF = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
SUM_BOUND_FACTOR = 4.0


def sum_bound_tolerance(ref, A, u, dtype):
    """4 u A + u max(|ref|, smallest normal number of dtype), per element"""
    return SUM_BOUND_FACTOR * u * A + u * ref.abs().clamp(min=torch.finfo(dtype).tiny)     # (+ the result's own rounding)


def sum_bound_ratio(got, ref, A, u):
    """largest |got - ref| / sum_bound_tolerance over the elements (the result's dtype: got.dtype)"""
    g, r, a = (x.detach().to(ref.device).double() for x in (got, ref, A))      # (where the reference lives)
    tol = sum_bound_tolerance(r, a, u, got.dtype)
    err = (g - r).abs()
    ratio = torch.where(err > 0, err / tol, torch.zeros_like(err))         # (err > 0 = tol: inf, and it fails)
    return ratio.max().item() if ratio.numel() else 0.0


def assert_within_sum_bound(got, ref, A, u, what=""):
    """dK / dV element by element against the bound of their OWN sum: |got - ref| <= 4 u A + u |ref|, where A is the sum of
    the magnitudes of the element's terms (oracle_bwd(bounds=True): A_V = P^T |dO|, A_K = scale sum_i P_ij (|dP_ij| +
    sum_e |dO_ie O_ie|) |q_id|, over the GQA group) and u the unit roundoff of the dtype (UNIT_ROUNDOFF).
    Where the 4 comes from (the documented arithmetic, DESIGN.md 3.x: f32 accumulation, P and dS packed to the dtype once,
    the result rounded once): the packing moves each term by at most u |term|, i.e. the sum by at most u A; Delta is
    rowsum(dO O) of an O that the forward already rounded, at most u sum_e |dO_e O_e| per row, which enters dS through
    P - the second part of A_K -, so both parts together stay below u A_K; the result's own rounding is the u |ref| term
    and |ref| <= A; f32 accumulation (2^-24 per add) is negligible.  fp16 keeps that relative precision down to 2^-14 only
    (subnormal below, fixed spacing 2^-24): a packed term is moved by at most u max(|term|, 2^-14), which is why A counts
    every visible pair at 2^-14 at least, and the result's rounding is u max(|ref|, 2^-14).  Worst case below 2 u A + u |ref|; the factor 4 is a
    twofold margin over that sum and is not fitted to any kernel's output (tests/test_probe_inputs.py keeps a CPU model
    of this arithmetic within half of the bound).  Returns the largest ratio."""
    ratio = sum_bound_ratio(got, ref, A, u)
    assert ratio <= 1.0, (f"{what}: |got - ref| reaches {ratio:.3f} of the sum bound 4 u A + u |ref| (u = 2^{int(math.log2(u))})")
    return ratio


def _rt(x, dtype):
    """x (fp64) rounded to dtype and back"""
    return x.to(dtype).double()


def rounded_model_bwd(q, k, v, do, ns, W, s_aux=None, block=256):
    """CPU model of the documented arithmetic of the MFMA kernels on inputs of dtype q.dtype: the forward
    packs p to the dtype for P V, O is stored in the dtype, LSE in f32; Delta = rowsum(dO O) of that O, f32; the backward
    takes p = exp2(c s - LSE log2e) in f32, packs p (for dV) and dS = p (dP - Delta) (for dQ / dK) to the dtype,
    accumulates in f32 and rounds dQ / dK / dV to the dtype.  fp64 stands in for f32 accumulation (its 2^-24 is not
    modelled).  N_q <= N_kv (rows are the last N_q positions), row blocks over the sink + window key ranges like the
    banded oracle.  Returns o, dq, dk, dv in the dtype."""
    dt = q.dtype
    B, Hq, Nq, D = q.shape
    Hkv, Nk = k.shape[1], k.shape[2]
    g = Hq // Hkv
    scale = 1.0 / math.sqrt(D)
    o = torch.zeros(B, Hq, Nq, D, dtype=torch.float64)
    dq = torch.zeros(B, Hq, Nq, D, dtype=torch.float64)
    dk, dv = (torch.zeros(B, Hkv, Nk, D, dtype=torch.float64) for _ in range(2))
    dof = do.double()
    for r0 in range(0, Nq, block):
        r1 = min(Nq, r0 + block)
        pos = torch.arange(r0, r1) + (Nk - Nq)
        p1 = int(pos[-1]) + 1
        nsb = min(ns, p1)
        w0 = max(int(pos[0]) - W + 1, nsb, 0)
        cols = torch.cat([torch.arange(0, nsb), torch.arange(w0, p1) if p1 > w0 else torch.arange(0)])
        qb, dob = q[:, :, r0:r1].double(), dof[:, :, r0:r1]
        kb, vb = (x[:, :, cols].double().repeat_interleave(g, dim=1) for x in (k, v))
        s = (torch.matmul(qb, kb.transpose(-2, -1)) * scale).float().double()
        s = s.masked_fill(~O.valid_mask(pos, cols, ns, W), float("-inf"))
        s_all = s if s_aux is None else torch.cat([s, s_aux.double().view(1, Hq, 1, 1).expand(B, Hq, r1 - r0, 1)], -1)
        m = s_all.max(-1, keepdim=True).values
        m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
        e = torch.exp(s - m)
        l = torch.exp(s_all - m).sum(-1, keepdim=True)
        lse = (m + torch.log(l)).float().double()
        ob = _rt(torch.nan_to_num(torch.matmul(_rt(e, dt), vb) / l, nan=0.0), dt)      # packed p, f32 row sum, O stored
        o[:, :, r0:r1] = ob
        delta = (dob * ob).sum(-1, keepdim=True).float().double()
        p = torch.nan_to_num(torch.exp(s - lse), nan=0.0).float().double()
        dp = torch.matmul(dob, vb.transpose(-2, -1))
        ds = _rt(p * (dp - delta), dt)
        C = cols.numel()
        dq[:, :, r0:r1] = torch.matmul(ds, kb) * scale
        dk.index_add_(2, cols, (torch.matmul(ds.transpose(-2, -1), qb) * scale).view(B, Hkv, g, C, D).sum(2))
        dv.index_add_(2, cols, torch.matmul(_rt(p, dt).transpose(-2, -1), dob).view(B, Hkv, g, C, D).sum(2))
    return o.to(dt), dq.to(dt), dk.to(dt), dv.to(dt)


def dkdv_kernel_name(mode, B, Hkv, Nq, Nk, D, window, packed=False, dtype=torch.bfloat16, ns=1):
    """Name of the dK/dV kernel sfa_bwd must dispatch to, as it appears in sfa_last_path(): restates dkdv_asm() of
    csrc/sfa_bwd_mfma.hip.  mode: "rule" (the library's rule) / "asm" / "ws" (the per-call overrides).  None where the
    choice does not exist (fp32, head dims without a hand-placed body).  ns = num_sink of the call.  Packed batches: B = sequences, Nq = Nk = the
    longest one (the launch problem of sfa_bwd_varlen)."""
    if dtype == torch.float32 or D not in (64, 80, 96, 128):
        return None
    W = min(max(window, 0), Nk)
    # short windows without sink keys, self-attention, head dims below 128: the skewed sweep (dkdv_skew() of the library),
    # unless the call names one of the other kernels
    if mode == "rule" and D in (64, 80, 96) and ns <= 0 and (packed or Nq == Nk) and 1 <= W <= 512:
        return "dkdvasmskew"
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    wgs = -(-Nk // 256) * Hkv * B
    if not (D == 128 or W > 256 or wgs >= 2 * n_cu):   # short windows below head dim 128 on a grid that does not fill the chip twice: compiled kernels only
        return "dkdvws8"
    if mode == "asm":
        return "dkdvasm4x64"
    if mode == "ws":
        return "dkdvws8"
    dense = (not packed) and Nq == Nk      # row split available: the hand-placed kernel fills the chip whatever the grid
    fills = -(-Nk // 256) * Hkv * B >= n_cu
    return "dkdvasm4x64" if (dense or fills) else "dkdvws8"


# max |error| of the decode kernels against the fp64 oracle, per dtype (shared by the decode test modules)
DECODE_TOL = {torch.float32: 2e-5, torch.float16: 2e-3, torch.bfloat16: 1.6e-2}


def per_seq_oracle(q, k, v, do, cu, ns, W, sa):
    """fp64 oracle of a packed batch [1, H, T, D]: the dense oracle applied to every sequence cu[i] : cu[i + 1]."""
    o = torch.zeros(q.shape, dtype=torch.float64)
    dq, dk, dv = torch.zeros(q.shape, dtype=torch.float64), torch.zeros(k.shape, dtype=torch.float64), torch.zeros(
        v.shape, dtype=torch.float64)
    dsa = torch.zeros(q.shape[1], dtype=torch.float64)
    for a, b in zip(cu[:-1], cu[1:]):
        sl = (slice(None), slice(None), slice(a, b))
        o[sl], _ = O.sink_attention_dense(q[sl], k[sl], v[sl], ns, W, sa)
        g = O.sink_attention_bwd_dense(q[sl], k[sl], v[sl], do[sl], ns, W, sa)
        dq[sl], dk[sl], dv[sl] = g[0], g[1], g[2]
        if sa is not None:
            dsa += g[3]
    return o, dq, dk, dv, dsa


def chunk_oracle_rows(q, k, v, sa, prefill, ns, W, n, batches):
    """fp64 decode_dense per chunk row over the keys of the chronological history it may see."""
    from test_decode_multi_host import history_keys
    rows = []
    for t in range(n):
        keep = torch.tensor(history_keys(prefill, ns, W, t))
        pos = prefill + t
        rows.append(O.decode_dense(q[batches, :, pos:pos + 1], k[batches][:, :, keep], v[batches][:, :, keep], sa))
    return torch.cat(rows, dim=2)
