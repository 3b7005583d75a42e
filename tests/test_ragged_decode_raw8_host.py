"""CPU-only tests of SFA_FLAG_RAGGED_DECODE1_RAW8: the flag in the header and the binding, the workspace query (the bit
adds no bytes) and the refusals of ragged_step_dyn(raw_fp8=True) that need no GPU."""
import os
import re

import pytest
import torch

from sink_attention import SinkCacheLayer, _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEC, CHUNK, RAW = 0x100, 0x80, 0x200


def test_the_flag_is_in_the_header_and_the_binding():
    hdr = open(os.path.join(ROOT, "include", "sfa.h")).read()
    assert re.search(r"#define SFA_FLAG_RAGGED_DECODE1_RAW8 0x200u\b", hdr) and N.FLAG_RAGGED_DECODE1_RAW8 == RAW


@pytest.mark.parametrize("G,T,n_seq,D", [(8, 1024, 9, 64), (1, 320, 9, 128), (3, 130, 1, 80), (32, 7, 300, 96)])
def test_the_bit_adds_no_bytes_to_the_workspace(G, T, n_seq, D):
    step = N.lib().sfa_decode_ragged_step_workspace_bytes
    for dt in (N.SFA_DTYPE[torch.bfloat16], N.SFA_DTYPE[torch.float16]):
        a = (n_seq, 2 * G, 2, T, 100, D, dt)
        assert step(*a, DEC | RAW) == step(*a, DEC) > step(*a, RAW) == step(*a, 0) > 0
        assert step(*a, DEC | CHUNK | RAW) == step(*a, DEC | CHUNK)


@pytest.mark.parametrize("fp8,kw,err", [(True, {}, ValueError), (False, dict(decode_kernel=True), TypeError),
                                        (True, dict(decode_kernel=True, groups=[0, 1]), ValueError),
                                        (True, dict(decode_kernel=True, force_generic=True), ValueError)])
def test_the_keyword_is_refused_before_anything_else(fp8, kw, err):
    """without decode_kernel=True; on a pool that holds no FP8 codes; with groups=; with force_generic=True"""
    q, k = torch.zeros(1, 4, 3, 64, dtype=torch.bfloat16), torch.zeros(1, 2, 3, 64, dtype=torch.bfloat16)
    layer = SinkCacheLayer(4, 32)
    layer.window_k = torch.zeros(1, 2, 32, 64, dtype=torch.float8_e4m3fn if fp8 else torch.bfloat16)
    with pytest.raises(err, match="raw_fp8" if len(kw) < 2 else "decode_kernel"):
        layer.ragged_step_dyn(q, k, k, [0, 1, 3], [0, 1], raw_fp8=True, **kw)
