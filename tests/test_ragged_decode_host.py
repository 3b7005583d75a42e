"""CPU-only tests of SFA_FLAG_RAGGED_DECODE1: the flag and the workspace query in the header, the library and _native.py,
the size rule of the query, and the refusals of ragged_step_dyn(decode_kernel=True) that need no GPU."""
import os
import re

import pytest
import torch

import packed_regime as R
from sink_attention import SinkCacheLayer, _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HKV, NKV = 2, 100
DEC, CHUNK = 0x100, 0x80


def al256(x):
    return -(-x // 256) * 256


def test_the_flag_and_the_symbol_are_in_the_header_the_library_and_the_binding():
    hdr = open(os.path.join(ROOT, "include", "sfa.h")).read()
    assert re.search(r"#define SFA_FLAG_RAGGED_DECODE1 0x100u\b", hdr) and N.FLAG_RAGGED_DECODE1 == DEC
    assert re.search(r"size_t sfa_decode_ragged_step_workspace_bytes\(int64_t n_seq,", hdr)
    assert len(N.lib().sfa_decode_ragged_step_workspace_bytes.argtypes) == 8 and N.lib().sfa_abi_version() == 2


@pytest.mark.parametrize("G,T,n_seq,D", [(8, 1024, 9, 64), (1, 320, 9, 128), (3, 130, 1, 80), (32, 7, 300, 96)])
def test_the_workspace_is_the_ungrouped_one_then_the_table_then_the_decode_partials(G, T, n_seq, D):
    step, plain, chunk = (getattr(N.lib(), f"sfa_decode_ragged_{x}workspace_bytes") for x in ("step_", "", "chunk_"))
    bf, f16, f32 = (N.SFA_DTYPE[t] for t in (torch.bfloat16, torch.float16, torch.float32))
    P = HKV * G * n_seq * R.max_splits(1, HKV, n_seq, NKV + 1)
    dec = 2 * al256(4 * P) + al256(4 * P * D)
    for dt in (bf, f16):
        a = (n_seq, G * HKV, HKV, T, NKV, D, dt)
        assert step(*a, 0) == plain(*a) > 0 and step(*a, CHUNK) == chunk(*a) and step(*a, 0x40) == plain(*a)
        assert step(*a, DEC) == plain(*a) + dec and step(*a, DEC | CHUNK) == chunk(*a) + dec
        bigger = [(n_seq + 1, G * HKV, HKV, T, NKV, D, dt), (n_seq, G * HKV, HKV, T, NKV + 500, D, dt)]
        assert all(step(*b, DEC) >= step(*a, DEC) for b in bigger)
    for a in [(n_seq, G * HKV, HKV, T, NKV, D, f32), (n_seq, G * HKV, HKV, T, NKV, 48, bf), (n_seq, G * HKV, HKV, T, NKV, 256, bf),
              (n_seq, 64 * HKV, HKV, T, NKV, D, bf)]:
        assert plain(*a) > 0 and step(*a, DEC) == 0 and step(*a, DEC | CHUNK) == 0


@pytest.mark.parametrize("Hq,D,dtype,kw", [(4, 64, torch.bfloat16, dict(groups=[0, 1])), (4, 256, torch.bfloat16, {}),
                                           (4, 64, torch.float32, {}), (4, 64, torch.float16, dict(force_generic=True)),
                                           (128, 64, torch.bfloat16, {})])
def test_the_keyword_is_refused_by_name_before_anything_else(Hq, D, dtype, kw):
    q, k = torch.zeros(1, Hq, 3, D, dtype=dtype), torch.zeros(1, 2, 3, D, dtype=dtype)
    with pytest.raises(ValueError, match="decode_kernel"):
        SinkCacheLayer(4, 32).ragged_step_dyn(q, k, k, [0, 1, 3], [0, 1], decode_kernel=True, **kw)
