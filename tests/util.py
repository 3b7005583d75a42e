"""Shared helpers for the GPU parity tests."""
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


def oracle_bwd(q, k, v, do, ns, W, s_aux=None, banded=None):
    N = q.shape[2]
    if banded is None:
        banded = N > 1024
    fn = O.sink_attention_bwd_banded if banded else O.sink_attention_bwd_dense
    return fn(q.cpu(), k.cpu(), v.cpu(), do.cpu(), ns, W, None if s_aux is None else s_aux.cpu().float())


def maxdiff(a, b):
    if a.numel() == 0:
        return 0.0
    return (a.detach().double().cpu() - b.detach().double().cpu()).abs().max().item()


def assert_close(actual, expected, atol, rtol, what=""):
    a = actual.detach().double().cpu()
    e = expected.detach().double().cpu()
    err = (a - e).abs()
    tol = atol + rtol * e.abs()
    bad = err > tol
    assert not bad.any(), (f"{what}: {int(bad.sum())}/{bad.numel()} elements out of tolerance "
                           f"(atol={atol}, rtol={rtol}); max abs err {err.max().item():.3e}")


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
