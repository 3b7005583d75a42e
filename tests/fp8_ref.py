"""The two rules of the FP8 (OCP e4m3fn) slot pool (include/sfa.h), restated in torch.

Storing a 16-bit element x of KV head h:  code = e4m3fn_rne(clamp(float(x) * (1.0f / scale[h]), -448, 448)).
Reading a code of KV head h as dtype T:   T(float(code) * scale[h]), one f32 multiply, round-to-nearest-even to T.

`scale_row` is one row of kv_scale ([H_kv] f32: row 0 for K, row 1 for V) or None for all ones; the tensors are
[..., H_kv, rows, D] with the KV head on dim -3.  Codes are compared as bytes: `codes.view(torch.uint8)`."""
import torch

FP8 = torch.float8_e4m3fn
FP8_MAX = 448.0


def _per_head(scale_row, like):
    if scale_row is None:
        return torch.ones(like.shape[-3], dtype=torch.float32, device=like.device)
    s = torch.as_tensor(scale_row, dtype=torch.float32).to(like.device)
    assert s.shape == (like.shape[-3],), (s.shape, like.shape)
    return s


def quant(x, scale_row=None):
    """16-bit rows [..., H_kv, n, D] -> e4m3fn codes of the same shape: f32 multiply by the per-head reciprocal, explicit
    clamp to +-448, round-to-nearest-even."""
    r = 1.0 / _per_head(scale_row, x)                       # IEEE f32 division, one reciprocal per head
    return (x.float() * r[:, None, None]).clamp(-FP8_MAX, FP8_MAX).to(FP8)


def quant_by_division(x, scale_row=None):
    """The same with a division per element in place of the reciprocal (tests/test_fp8_pool_host.py compares the two)."""
    s = _per_head(scale_row, x)
    return (x.float() / s[:, None, None]).clamp(-FP8_MAX, FP8_MAX).to(FP8)


def dequant(codes, scale_row, dtype):
    """e4m3fn codes [..., H_kv, n, D] -> what a kernel reads as `dtype`: one f32 multiply, then round-to-nearest-even."""
    s = _per_head(scale_row, codes)
    return (codes.float() * s[:, None, None]).to(dtype)


def same_codes(a, b):
    return a.dtype == b.dtype == FP8 and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))
