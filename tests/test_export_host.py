"""CPU-only tests of the export of pool slots (sfa_ring_export_slots and its three pool forms; SinkCacheLayer.export_slots
/ import_slots / live_lengths): the symbols and their prototypes, the torch twin of tests/export_ref.py against a
brute-force model of the sink + ring cache, and the argument errors that are raised before anything touches a GPU."""
import random
from unittest import mock

import pytest
import torch

import export_ref as X
import paged_ref

BF, FP, F32, FP8 = torch.bfloat16, torch.float16, torch.float32, torch.float8_e4m3fn
ENTRIES = {"sfa_ring_export_slots": 12, "sfa_ring_export_fp8_slots": 13, "sfa_ring_export_paged_slots": 14,
           "sfa_ring_export_paged_fp8_slots": 15}


# ------------------------------------------------------------------------------------------------ 1. the library
@pytest.mark.parametrize("name", list(ENTRIES))
def test_library_exports_the_call_with_the_declared_argument_count(name):
    from sink_attention import _native
    lib = _native.lib()
    assert hasattr(lib, name)
    assert len(getattr(lib, name).argtypes) == ENTRIES[name]
    # the siblings they are named and ordered after: the fill of the same pool takes the same count less pos_out
    fill = name.replace("ring_export", "ring_fill_varlen")
    assert len(getattr(lib, fill).argtypes) == ENTRIES[name] - 1


def _host_call(name, dtype=BF, cache=BF, D=64, T=6, nseq=2, batch=1, **null):
    """the entry point on host tensors: every call here returns before any launch, nothing is dereferenced"""
    from sink_attention import _native as N
    S, H, ns, W, P = 3, 2, 4, 64, 32
    paged, fp8 = "_paged" in name, "_fp8" in name
    z = lambda *s, dt: torch.zeros(*s, dtype=dt)
    t = dict(sk=z(S, H, ns, D, dt=cache), sv=z(S, H, ns, D, dt=cache),
             wk=z(*((5, H, P, D) if paged else (S, H, W, D)), dt=cache), wv=z(*((5, H, P, D) if paged else (S, H, W, D)), dt=cache),
             ko=z(batch, H, T, D, dt=dtype), vo=z(batch, H, T, D, dt=dtype))
    i32 = torch.zeros(16, dtype=torch.int32)
    p = {k: (None if null.get(k) else i32.data_ptr()) for k in ("cu", "state", "slots")}
    tail = ([i32.data_ptr(), 2] if paged else []) + ([None] if fp8 else [])
    rc = getattr(N.lib(), name)(*(N.desc(t[k]) for k in ("sk", "sv", "wk", "wv", "ko", "vo")), p["cu"], nseq, p["state"],
                                p["slots"], None, *tail, None)
    return rc, N.lib().sfa_last_error().decode()


def test_host_checks_run_before_any_launch():
    base = "sfa_ring_export_slots"
    assert _host_call(base, cu=True) == (-1, "cu_seqlens: null device pointer")
    assert _host_call(base, state=True) == (-1, "state: null device pointer")
    assert _host_call(base, slots=True) == (-1, "slots: null device pointer")
    assert _host_call(base, nseq=0) == (-1, "n_seq must be >= 1 (got 0)")
    assert _host_call(base, batch=2) == (-1, "packed layout: k_out / v_out must be [1, H_kv, T, D] (batch dim 2)")
    assert _host_call(base, dtype=FP) == (-1, "k_out / v_out and the cache buffers must share one dtype")
    assert _host_call(base, dtype=BF, cache=BF, D=20)[1] == "ring_export: K/V rows must be a multiple of 16 bytes (head dim 20)"
    assert _host_call("sfa_ring_export_fp8_slots", cache=BF) == (-1, "ring_export_fp8: the cache buffers must be FP8 (e4m3)")
    assert _host_call("sfa_ring_export_paged_fp8_slots", cache=BF) == (
        -1, "ring_export_paged_fp8: the cache buffers must be FP8 (e4m3)")
    rc, msg = _host_call("sfa_ring_export_fp8_slots", cache=FP8, dtype=F32)
    assert rc == -2 and msg.startswith("ring_export_fp8: an FP8 pool serves bf16 / f16 activations"), msg
    rc, msg = _host_call("sfa_ring_export_paged_slots", cache=F32, dtype=F32)
    assert rc == -2 and msg.startswith("ring_export_paged: a paged pool serves bf16 / f16"), msg
    assert _host_call(base, T=0) == (0, "")          # an empty pack: SFA_OK without a launch


# ------------------------------------------------------------------------------------------------ 2. the twin
class _Model:
    """A sink + ring cache over token NUMBERS, fed the way the library feeds one: the first chunk by the prefill
    placement, every later chunk by the commit rule (token t of n goes to slot (write_pos + t) mod Wc if t >= n - Wc)."""

    def __init__(self, ns, Wc):
        self.ns, self.Wc = ns, Wc
        self.sink, self.ring, self.state = [None] * ns, [None] * Wc, [0, 0, 0, 0]

    def prefill(self, toks):
        L = len(toks)
        sl = min(L, self.ns)
        rem = L - sl
        self.sink[:sl] = toks[:sl]
        for s in (range(rem) if rem <= self.Wc else range(self.Wc)):
            self.ring[s] = toks[sl + s] if rem <= self.Wc else toks[L - self.Wc + s]
        self.state = paged_ref.prefill_state(L, self.ns, self.Wc)

    def commit(self, toks):
        n = len(toks)
        slots, after = paged_ref.commit_ring_slots(self.state, n, self.Wc)
        for t, s in zip(range(max(0, n - self.Wc), n), slots):
            self.ring[s] = toks[t]
        self.state = after


def _fed(n, ns, Wc, rng):
    """a model that has been fed tokens 0 .. n - 1 in random chunks (the first at least min(n, ns), as a scheduler
    admits: see SFA_FLAG_RAGGED_ADMIT in include/sfa.h)"""
    m = _Model(ns, Wc)
    first = rng.randint(min(n, ns), n) if n else 0
    m.prefill(list(range(first)))
    t = first
    while t < n:
        c = min(n - t, rng.randint(1, Wc + 3))
        m.commit(list(range(t, t + c)))
        t += c
    return m


def _as_pool(models, ns, Wc, H=2, D=4):
    """the models as pool buffers: token number t is the value t + 1 (K) / -(t + 1) (V) in every element, empty rows 0"""
    S = len(models)
    sk, wk = torch.zeros(S, H, ns, D), torch.zeros(S, H, Wc, D)
    for c, m in enumerate(models):
        for j, t in enumerate(m.sink):
            sk[c, :, j] = 0 if t is None else t + 1
        for j, t in enumerate(m.ring):
            wk[c, :, j] = 0 if t is None else t + 1
    return sk, -sk, wk, -wk, torch.tensor([m.state for m in models], dtype=torch.int32)


@pytest.mark.parametrize("ns,Wc", [(4, 16), (4, 3), (0, 5), (3, 1)])
def test_the_twin_gives_first_sinks_then_newest_window_for_every_fill(ns, Wc):
    rng = random.Random(100 * ns + Wc)
    edges = sorted({0, 1, max(ns - 1, 0), ns, ns + 1, ns + Wc - 1, ns + Wc, ns + Wc + 1, ns + 2 * Wc, ns + 3 * Wc + 2})
    wps = set()
    for rep in range(6):
        lengths = edges + [rng.randint(ns + Wc, ns + 4 * Wc) for _ in range(6)]
        models = [_fed(n, ns, Wc, rng) for n in lengths]
        sk, sv, wk, wv, state = _as_pool(models, ns, Wc)
        want = []
        for n, m in zip(lengths, models):
            sl, wl, wp, seen = m.state
            assert seen == n and sl == min(n, ns) and wl == min(n - sl, Wc)
            wps.add(wp)
            want.append(list(range(sl)) + list(range(n - wl, n)))       # tokens[:sl] + tokens[n - wl:]
        cu = [0]
        for w in want:
            cu.append(cu[-1] + len(w))
        k, v, pos = X.export_twin(sk, sv, wk, wv, state, list(range(len(models))), cu, cu[-1] + 2, ns, Wc)
        flat = [t for w in want for t in w]
        assert pos.tolist() == flat + [-1, -1]                          # a token's position is its number
        assert k[0, 0, :, 0].tolist() == [t + 1 for t in flat] + [0, 0]
        assert torch.equal(v, -k) and bool((k == k[:, :1, :, :1]).all())
    assert len(wps) >= min(Wc, 4), wps                                  # write_pos landed all over the ring


def test_the_twin_truncates_pads_skips_and_reads_pages():
    ns, Wc, P = 2, 64, 32
    rng = random.Random(7)
    models = [_fed(n, ns, Wc, rng) for n in (ns + Wc + 9, 5, 0)]
    sk, sv, wk, wv, state = _as_pool(models, ns, Wc)
    full = list(range(ns)) + list(range(ns + 9, ns + Wc + 9))
    #          truncated   zero tail    inactive  the same slot again, fresh slot
    slots, cu = [0, 1, -1, 0, 2], [0, 10, 20, 23, 89, 89]
    k, v, pos = X.export_twin(sk, sv, wk, wv, state, slots, cu, 92, ns, Wc)
    assert pos.tolist() == full[:10] + list(range(5)) + [-1] * 5 + [-1] * 3 + full + [-1] * 3
    assert k[0, 1, :, 2].tolist() == [p + 1 for p in pos.tolist()]      # zero rows: -1 + 1
    # the same pool paged: slot 0 on pages 3 and 1, slot 1 on page 0 with its second page unmapped, slot 2 unmapped
    table = torch.tensor([[3, 1], [0, -1], [-1, 7]], dtype=torch.int32)
    pk = paged_ref.scatter(wk, table, torch.zeros(4, 2, P, 4))
    kp, vp, pp = X.export_twin(sk, sv, pk, paged_ref.scatter(wv, table, torch.zeros(4, 2, P, 4)), state, slots, cu, 92, ns,
                               Wc, table=table)
    assert torch.equal(kp, k) and torch.equal(vp, v) and torch.equal(pp, pos)
    table[0, 1] = -1                         # now unmap the page that holds slot 0's ring slots 32 .. 63
    ku, _, pu = X.export_twin(sk, sv, pk, pk, state, slots, cu, 92, ns, Wc, table=table)
    assert torch.equal(pu, pos)              # the positions stay, the rows of that page read as zeros
    gone = [i for i, (is_sink, slot, _) in enumerate(X.token_order(state[0].tolist(), ns, Wc)) if not is_sink and slot >= 32]
    assert len(gone) == 32 and not ku[0, :, [23 + i for i in gone]].any()
    keep = [r for r in range(92) if r not in {23 + i for i in gone} | {i for i in gone if i < 10}]
    assert torch.equal(ku[0, :, keep], k[0, :, keep])


def test_the_twin_dequantises_by_the_reading_rule():
    import fp8_ref
    g = torch.Generator().manual_seed(3)
    S, H, ns, Wc, D = 2, 2, 2, 4, 8
    codes = lambda n: (torch.randn(S, H, n, D, generator=g) * 3).to(FP8)
    sk, sv, wk, wv = codes(ns), codes(ns), codes(Wc), codes(Wc)
    scale = torch.tensor([[0.37, 1.9], [2.3, 0.011]])
    state = torch.tensor([[2, 4, 1, 11], [1, 0, 0, 1]], dtype=torch.int32)
    k, v, pos = X.export_twin(sk, sv, wk, wv, state, [0, 1], [0, 6, 7], 7, ns, Wc, kv_scale=scale, dtype=FP)
    assert k.dtype == FP and pos.tolist() == [0, 1, 7, 8, 9, 10, 0]
    ring = [1, 2, 3, 0]                      # write_pos 1 on a full ring: the oldest token sits at slot 1
    assert torch.equal(k[0, :, 2:6], fp8_ref.dequant(wk[0], scale[0], FP)[:, ring])
    assert torch.equal(v[0, :, 2:6], fp8_ref.dequant(wv[0], scale[1], FP)[:, ring])
    assert torch.equal(v[0, :, 6], (sv[1, :, 0].float() * scale[1][:, None]).to(FP))


# ------------------------------------------------------------------------------------------------ 3. Python arguments
def _cpu_pool(dtype=BF, **kw):
    from sink_attention import SinkCacheLayer
    layer = SinkCacheLayer(4, 16)
    layer.init_pool(3, 2, 64, dtype, "cpu", **kw)
    return layer


def test_live_lengths_reads_the_state_rows():
    layer = _cpu_pool()
    layer._dev_state.copy_(torch.tensor([[4, 16, 3, 90], [2, 0, 0, 2], [0, 0, 0, 0]], dtype=torch.int32))
    got = layer.live_lengths([1, -1, 0, 2, 0])
    assert got.dtype == torch.int32 and got.tolist() == [2, 0, 20, 0, 20]


def test_export_slots_refuses_bad_arguments_before_any_gpu_work():
    layer = _cpu_pool()
    pack = lambda dt, T=8: torch.zeros(1, 2, T, 64, dtype=dt)
    with pytest.raises(TypeError, match="out must have the pool's dtype"):
        layer.export_slots([0, 1], cu=[0, 4, 8], out=(pack(FP), pack(FP)))
    with pytest.raises(ValueError, match=r"bad cu_seqlens \[0, 4, 9\] for T=8"):
        layer.export_slots([0, 1], cu=[0, 4, 9], T=8)
    dev_cu = mock.MagicMock(spec=torch.Tensor)
    dev_cu.is_cuda = True
    with pytest.raises(ValueError, match="a device cu needs T or out"):
        layer.export_slots([0, 1], cu=dev_cu)
    with pytest.raises(ValueError, match="cu must hold n \\+ 1 = 3 offsets"):
        layer.export_slots([0, 1], cu=[0, 4], T=8)
    with pytest.raises(ValueError, match="outside the pool of 3 slots"):
        layer.export_slots([0, 3], cu=[0, 4, 8], T=8)
    with pytest.raises(ValueError, match="T = 9 but out holds 8 rows"):
        layer.export_slots([0, 1], cu=[0, 4, 8], T=9, out=(pack(BF), pack(BF)))
    with pytest.raises(ValueError, match="16-byte aligned"):
        layer.export_slots([0, 1], cu=[0, 4, 8], out=(torch.zeros(1, 2, 8, 65, dtype=BF)[..., :64], pack(BF)))
    fp8 = _cpu_pool(BF, kv_dtype=FP8)
    assert fp8._act_dtype == BF and _cpu_pool(FP, kv_dtype=FP8)._act_dtype == FP
    with pytest.raises(TypeError, match="must be bfloat16 or float16"):
        fp8.export_slots([0], cu=[0, 8], out=(pack(F32), pack(F32)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):      # past the argument checks: the kernel is the only path
        layer.export_slots([0, 1], cu=[0, 4, 8], T=8)


def test_import_slots_refuses_bad_arguments_before_any_gpu_work():
    layer = _cpu_pool()
    k = torch.zeros(1, 2, 8, 64, dtype=FP)
    with pytest.raises(TypeError, match="k / v must have the pool's dtype"):
        layer.import_slots(k, k, [0, 4, 8], [0, 1])
    k = k.to(BF)
    with pytest.raises(ValueError, match="seen must hold n = 2 entries, got 3"):
        layer.import_slots(k, k, [0, 4, 8], [0, 1], seen=[4, 4, 4])
    with pytest.raises(ValueError, match="a slot is named twice"):
        layer.import_slots(k, k, [0, 4, 8], [1, 1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        layer.import_slots(k, k, [0, 4, 8], [0, 1], seen=[40, 4])


def test_the_cache_forms_forward_to_the_layer():
    from sink_attention import SinkAttentionCache
    for name in ("export_slots", "import_slots", "live_lengths"):
        assert callable(getattr(SinkAttentionCache, name))
