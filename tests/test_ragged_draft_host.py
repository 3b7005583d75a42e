"""CPU-only tests of SFA_FLAG_RAGGED_DECODE_DRAFT: the flag in the header and the binding, the size rule
of sfa_decode_ragged_step_workspace_bytes(..., flags), the three values of ragged_step_dyn(decode_kernel=) and the
refusals that need no GPU."""
import os
import re

import pytest
import torch

import packed_regime as R
from sink_attention import SinkCacheLayer, _native as N
from test_ragged_decode_host import CHUNK, DEC, HKV, NKV, ROOT, al256
from test_ragged_tree_host import _cpu_pool, _mk, stub  # noqa: F401  (stub: a fixture)

DRAFT = 0x400


def test_the_flag_is_in_the_header_and_the_binding():
    hdr = open(os.path.join(ROOT, "include", "sfa.h")).read()
    assert re.search(r"#define SFA_FLAG_RAGGED_DECODE_DRAFT 0x400u\b", hdr) and N.FLAG_RAGGED_DECODE_DRAFT == DRAFT
    assert len(N.lib().sfa_decode_ragged_step_workspace_bytes.argtypes) == 8 and N.lib().sfa_abi_version() == 2


@pytest.mark.parametrize("G,T,n_seq,D", [(8, 1024, 9, 64), (1, 320, 9, 128), (3, 130, 1, 80), (16, 7, 300, 96), (5, 64, 2048, 64)])
def test_the_draft_partials_lie_behind_the_decode_partials(G, T, n_seq, D):
    step = N.lib().sfa_decode_ragged_step_workspace_bytes
    bf, f16, f32 = (N.SFA_DTYPE[t] for t in (torch.bfloat16, torch.float16, torch.float32))
    Pd = HKV * n_seq * 32 * R.max_splits(1, HKV, n_seq, NKV + 32 // G)
    draft = 2 * al256(4 * Pd) + al256(4 * Pd * D)
    for dt in (bf, f16):
        a = (n_seq, G * HKV, HKV, T, NKV, D, dt)
        assert step(*a, DEC) > 0 and step(*a, DEC | DRAFT) == step(*a, DEC) + draft
        assert step(*a, DEC | CHUNK | DRAFT) == step(*a, DEC | CHUNK) + draft and step(*a, DEC | 0x200 | DRAFT) == step(*a, DEC | DRAFT)
        assert step(*a, DRAFT) == step(*a, 0) and step(*a, CHUNK | DRAFT) == step(*a, CHUNK)    # ignored without 0x100
    for a in [(n_seq, G * HKV, HKV, T, NKV, D, f32), (n_seq, G * HKV, HKV, T, NKV, 256, bf), (n_seq, 17 * HKV, HKV, T, NKV, D, bf),
              (n_seq, 32 * HKV, HKV, T, NKV, D, f16)]:
        assert step(*a, 0) > 0 and step(*a, DEC | DRAFT) == 0 and step(*a, DEC | CHUNK | DRAFT) == 0
    assert step(n_seq, 32 * HKV, HKV, T, NKV, D, bf, DEC) > 0        # G = 32 keeps its decode rows


@pytest.mark.parametrize("value,flags", [(False, 0), (True, DEC), ("draft", DEC | DRAFT)])
def test_the_three_values_reach_the_library_with_their_flags(stub, value, flags):
    layer = _cpu_pool()
    layer.ragged_step_dyn(_mk(8), _mk(2), _mk(2), [0, 2, 6], [0, 1], decode_kernel=value, chunk_kernel=True)
    name, args = stub.calls[-1]          # behind the workspace queries
    assert name == "sfa_decode_ring_ragged_slots" and args[-2] == flags | CHUNK


@pytest.mark.parametrize("Hq,D,dtype,kw", [(4, 64, torch.bfloat16, dict(decode_kernel="foo")), (4, 64, torch.bfloat16, dict(decode_kernel=1)),
                                           (4, 64, torch.bfloat16, dict(groups=[0, 1])), (4, 256, torch.bfloat16, {}),
                                           (4, 64, torch.float32, {}), (4, 64, torch.float16, dict(force_generic=True)),
                                           (64, 64, torch.bfloat16, {})])
def test_the_keyword_is_refused_by_name_before_anything_else(Hq, D, dtype, kw):
    q, k = torch.zeros(1, Hq, 3, D, dtype=dtype), torch.zeros(1, 2, 3, D, dtype=dtype)
    with pytest.raises(ValueError, match="decode_kernel"):
        SinkCacheLayer(4, 32).ragged_step_dyn(q, k, k, [0, 1, 3], [0, 1], **{"decode_kernel": "draft", **kw})
