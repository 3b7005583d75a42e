"""CPU: tests/util.py::device_oracle (the whole-tensor fp64 reference the GPU work-list tests compute on the device, unit by
unit) against oracle_fwd / oracle_bwd(bounds=True) on CPU tensors.  The same fp64 functions on slices of the same inputs:
measured bitwise equal on every output (dense and banded, bf16 and fp16 inputs), so equality is what is asserted."""
import pytest
import torch

from util import device_oracle, oracle_bwd, oracle_fwd, rand

NAMES = ("o", "lse", "dq", "dk", "dv", "ds_aux", "a_k", "a_v")


def _inputs(shape_q, shape_k, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    q, k, v, do = (rand(s, g, dtype) for s in (shape_q, shape_k, shape_k, shape_q))
    return q, k, v, do, rand((shape_q[1],), g, torch.float32, 0.5)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_device_oracle_is_the_oracle_gqa(dtype):
    B, Hq, Hkv, N, D, ns, W = 2, 4, 2, 1100, 32, 4, 300              # above 1024 rows: the banded functions
    q, k, v, do, sa = _inputs((B, Hq, N, D), (B, Hkv, N, D), dtype, 5)
    got = device_oracle(q, k, v, do, ns, W, sa)
    ref = (*oracle_fwd(q, k, v, ns, W, sa), *oracle_bwd(q, k, v, do, ns, W, sa, bounds=True))
    for name, a, b in zip(NAMES, got, ref):
        assert torch.equal(a, b), name


def test_device_oracle_is_the_oracle_packed():
    lens, Hq, Hkv, D, ns, W = [1100, 0, 1, 300], 4, 2, 32, 4, 300    # banded, empty, one row, dense
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    T = cu[-1]
    q, k, v, do, sa = _inputs((1, Hq, T, D), (1, Hkv, T, D), torch.bfloat16, 6)
    got = device_oracle(q, k, v, do, ns, W, sa, cu=cu)
    ref = [torch.zeros_like(x) for x in got]
    ref[1].fill_(float("-inf"))
    for a, b in zip(cu[:-1], cu[1:]):
        if b > a:
            sl = (slice(None), slice(None), slice(a, b))
            r = (*oracle_fwd(q[sl], k[sl], v[sl], ns, W, sa), *oracle_bwd(q[sl], k[sl], v[sl], do[sl], ns, W, sa, bounds=True))
            for i in (0, 1, 2, 3, 4, 6, 7):
                ref[i][sl] = r[i]
            ref[5] += r[5]
    for name, a, b in zip(NAMES, got, ref):
        assert torch.equal(a, b), name
