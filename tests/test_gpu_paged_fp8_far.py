"""Far-offset twin of the paged FP8 pool, in the manner of the paged case of tests/test_gpu_far_offsets.py: the 4.1 GiB
arena, filled with 0x7F (NaN in e4m3fn), is ONE FP8 K page buffer and one V page buffer (far_views.page_pool at one byte
per element), and the table of the three named slots mixes pages from both sides of 2^31 and of 2^32 bytes - which are
element offsets too, an element being a byte.  The serving script of that module (prefill, an admitting step with the
long admission, a tree step with per-sequence commit, the packed commit with and without a path, a plain step) runs on a
near pool (init_pool(page_size=32, kv_dtype=float8_e4m3fn), the pages' ranks in the table) and on the far one: outputs,
paths, state rows and the bytes of every mapped page are equal after every call, the near run equals its contiguous FP8
twin, and the rest of the arena keeps its sentinel.  tests/test_paged_fp8_far_views.py proves on the CPU that a signed or
unsigned 32-bit byte offset would leave this case's operands."""
import pytest
import torch

import far_views as F
import test_gpu_far_offsets as G
from fp8_ref import FP8
from sink_attention import SinkCacheLayer
from test_gpu_far_offsets import arena16          # noqa: F401  (the module-scoped arena and its skip rule)

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASE = ("bf16", 128, 1, 2)             # activations, D, G, H_kv
SCALES = ([0.37, 2.0], [0.25, 1.0])
TAIL = "_paged_kvfp8"


def _u8(t):
    return t.view(torch.uint8)


def _near(S, Hkv, W, D, act, table, n_pages):
    """the near pool: the keyword spelling, `table`, every page row 0x7F as the arena's are"""
    L = SinkCacheLayer(G.NS, W)
    L.init_pool(S, Hkv, D, act, DEV, page_size=G.PG, num_pages=n_pages, kv_dtype=FP8)
    L.page_table.copy_(torch.tensor(table, dtype=torch.int32))
    L.set_kv_scale(*SCALES)
    for name in G.RING:
        _u8(getattr(L, name)).fill_(F.SENTINEL8 & 0xFF)
    return L


def _contig_twin(L):
    """the contiguous FP8 twin (tests/paged_ref.py::gather over the bytes), built before any call"""
    S = L.sink_k.shape[0]
    ring = [G.PR.gather(_u8(getattr(L, name)), L.page_table.cpu()).view(FP8) for name in G.RING]
    tw = G._pool_layer(L.window_size, [L.sink_k.clone(), L.sink_v.clone()] + ring, S, scales=SCALES)
    tw._dev_state.copy_(L._dev_state)
    return tw


def _is_the_twin(rp, rt, what):
    """record of the paged FP8 run against the record of the script on its contiguous FP8 twin: bitwise"""
    for a, b in zip(rp, rt):
        w = (what, a["name"])
        if a["path"] is not None:
            assert a["path"].endswith(TAIL) and b["path"] == a["path"][:-len(TAIL)] + "_kvfp8", (w, a["path"], b["path"])
        assert torch.equal(a["st"], b["st"]), w
        assert a["o"] is None or (torch.equal(a["o"], b["o"]) and not torch.isnan(a["o"].float()).any() and a["o"].any()), (w, "o")
        for k, x in a["c"].items():
            y = b["c"][k[:2]]
            assert torch.equal(x, y if len(k) == 2 else y[:, k[2] * G.PG:(k[2] + 1) * G.PG]), (w, k)


def test_paged_fp8_pool_on_one_large_page_buffer(arena16):
    dt, D, Gq, Hkv = CASE
    act, S, named, W = G.DT[dt], 4, [3, 1, 2], G.WP
    arena = G._arena(arena16, FP8, F.SENTINEL8)
    assert arena.element_size() == 1 and bool((_u8(arena)[:: 1 << 20] == 0x7F).all())
    pp = F.page_pool(arena.numel(), Hkv * G.PG * D, 1)
    assert pp.p31 == pp.e31 < pp.p32                                # one byte per element: the lines of bytes are those of elements
    tab = [[-1] * (W // G.PG) for _ in range(S)]
    for s, row in zip(named, F.deal_pages(pp.picks, 3, W // G.PG, pp.p31, pp.p32)):
        tab[s] = row
    sv = G._Serving(dt, D, Gq, Hkv, W, named, seed=8300 + D)
    rtab, n_map = G._rank_table(tab)
    Ln = _near(S, Hkv, W, D, act, rtab, n_map + 2)
    tw = _contig_twin(Ln)
    near = G._play(Ln, sv.steps, named)
    sv.check_states(near, "near")
    _is_the_twin(near, G._play(tw, sv.steps, named), ("paged fp8, near", dt, D))
    pages = G._page_views(arena, pp, Hkv, D)
    assert all(p.dtype == FP8 and p.shape == (pp.n_pages, Hkv, G.PG, D) for p in pages)
    for s in named:
        hi, lo, mid = tab[s]
        for buf in pages:
            assert G._offset(arena, buf[hi]) >= F.TWO32
        assert G._offset(arena, pages[0][lo]) < F.TWO31 <= G._offset(arena, pages[0][mid]) < F.TWO32
    assert pp.n_pages - 1 in tab[2] and 0 in tab[2]
    for v in G._mapped_views(pages, tab):          # every row of a mapped page is 0x7F until a call stores into it
        assert bool((_u8(v) == 0x7F).all())
    sinks = [torch.zeros(S, Hkv, G.NS, D, dtype=torch.uint8, device=DEV).view(FP8) for _ in range(2)]
    far = G._play(G._pool_layer(W, sinks + list(pages), S, table=tab, scales=SCALES), sv.steps, named)
    G._same_records(near, far, ("paged fp8 far pages", dt, D))
    assert far[2]["path"].endswith("_ragged_admit_commit" + TAIL) and far[3]["path"].startswith("decode_tree_mfma_") and \
        far[4]["path"] == "ring_commit_path_ragged_slots" + TAIL and far[1]["path"] == "ring_fill_varlen_slots" + TAIL, \
        [r["path"] for r in far]
    for k in far[-1]["c"]:            # every page of the long admission's slot and the first page of every slot was stored into
        if k[0] in G.RING and (k[1] == named[0] or k[2] == 0):
            assert not torch.equal(far[0]["c"][k], far[-1]["c"][k]), ("never written", k)
    F.assert_untouched(arena, G._mapped_views(pages, tab), f"paged fp8 {dt} {D}", sentinel=F.SENTINEL8)
