"""Head dim 256 on the slot pool, host side: init_pool admits it for the paged, FP8 and paged FP8 forms, and the three
workspace sizes say what exists there - the packed step (unchanged), no grouped and no chunk instance."""
import pytest
import torch

import group_regime as GR
from sink_attention import SinkCacheLayer, _native as N

FP8 = torch.float8_e4m3fn
FORMS = [dict(page_size=32), dict(dtype=FP8), dict(page_size=32, kv_dtype=FP8)]


@pytest.mark.parametrize("form", FORMS)
def test_init_pool_admits_256_and_still_refuses_48(form):
    kw = dict(dtype=torch.bfloat16, device="cpu")
    kw.update(form)
    layer = SinkCacheLayer(4, 64)
    layer.init_pool(8, 2, 256, **kw)
    assert layer.window_k.shape[-1] == 256 and layer.window_k.dtype == (FP8 if FP8 in form.values() else torch.bfloat16)
    with pytest.raises(ValueError, match="head dims 64 / 80 / 96 / 128"):
        SinkCacheLayer(4, 64).init_pool(8, 2, 48, **kw)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_the_workspace_sizes_at_256(dt):
    lib, d = N.lib(), N.SFA_DTYPE[dt]
    shape = (9, 64, 8, 520, 4 + 4096)           # n_seq, H_q, H_kv, T, num_sink + Wc
    assert lib.sfa_decode_ragged_chunk_workspace_bytes(*shape, 256, d) == 0
    assert lib.sfa_decode_ragged_group_workspace_bytes(shape[0], 2, *shape[1:], 256, d) == 0
    assert lib.sfa_decode_ragged_chunk_workspace_bytes(*shape, 128, d) > 0       # the predicate was split, not dropped
    assert lib.sfa_decode_ragged_workspace_bytes(*shape, 256, d) == GR.ragged_workspace_bytes(*shape, 256)
