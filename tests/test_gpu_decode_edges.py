"""GPU tests of the single-token decode kernels (csrc/sfa_decode.hip) where randn at a trivial split plan says little:
more than 64 splits (the later statistics rounds of reduce_head, nine O rounds), head loops of 2 / 3 / 6 trips, padded lane
groups, and the device-state forms on a grid of four splits with rows at every fill level.

Inputs are the decode probes of tests/probe_inputs.py: every (batch, q head) aims at one key on an edge of what the step
may read, with about half of the softmax mass on it.  tests/test_decode_probes.py proves on the CPU, for every launch made
here (probe_inputs.decode_runs enumerates them for both files), that a decode wrong by one key, one split, one fold round
or one head misses DECODE_TOL at least tenfold.  The launch arithmetic is restated in tests/decode_regime.py and pinned
here against the lpk{}_gt{}_s{} suffix of sfa_last_path().

What every launch asserts: the whole output against the fp64 oracle over the kept tokens at DECODE_TOL; last_path() against
regime(); a second run from the same state gives the same bits; outputs the caller owns are NaN-filled before the call; the
partials region of the cache's workspace is filled with 0xFF bytes before every call (the counters are left alone, and must
read zero after every one-pass call); after a storing step the four cache buffers and the state equal, bitwise, a twin
updated on the CPU.  The small-ring equalities of tests/test_gpu_decode.py are asserted at the same strength: decode_step
against append + decode_attention, decode_step_dyn against the host-state step (where both launches walk a row's keys in
the same order: equal keys per split, or every key in split 0)."""
import math

import pytest
import torch

import decode_regime as R
import probe_inputs as P
from util import DECODE_TOL, maxdiff

pytestmark = pytest.mark.gpu
DEV = "cuda"
BUFS = ("sink_k", "sink_v", "window_k", "window_v")
ONE_PASS = [False, True]
POOL_SLOTS = 13
# batch row -> pool slot of the slots= form (row probe_inputs.FILLS_INACTIVE is inactive); slots 3, 6 and 10 are nobody's
SLOT_OF = [7, 2, 11, -1, 0, 9, 4, 12, 5, 1, 8]
IDLE_STATE = (4, 7, 7, 11)


def _native():
    from sink_attention import _native
    return _native


# ------------------------------------------------------------------------------------------------ layers from a twin
def _layer(run, mode, one_pass):
    """a SinkCacheLayer that holds the twin's bytes and state: mode host / dyn (one shared device state) / rows"""
    from sink_attention import SinkCacheLayer
    layer = SinkCacheLayer(run.case["ns"], run.case["Wc"])
    for name in BUFS:
        setattr(layer, name, run.cache[name].to(DEV))
    layer.is_initialized = layer.prefilled = True
    layer.one_pass = one_pass
    if mode == "rows":
        layer._dev_state = torch.tensor([[sl, wl, wp, sl + wl] for sl, wl, wp in run.states], dtype=torch.int32, device=DEV)
        layer._per_seq = True
        return layer
    assert len(set(run.states)) == 1
    layer.sink_len, layer.window_len, layer.write_pos = run.states[0]
    layer.seen_tokens = layer.sink_len + layer.window_len
    if mode == "dyn":
        layer.enable_device_state()
    return layer


def _pool(run, one_pass):
    """a pool of POOL_SLOTS slots: batch row b of the twin lives in slot SLOT_OF[b]; the other slots hold other codes and
    a state nobody moves"""
    from sink_attention import SinkCacheLayer
    c = run.case
    layer = SinkCacheLayer(c["ns"], c["Wc"])
    layer.init_pool(POOL_SLOTS, c["Hkv"], c["D"], R.DT[c["dtype"]], DEV)
    junk = P.decode_cache(POOL_SLOTS, c["Hkv"], c["D"], c["ns"], c["Wc"], R.DT[c["dtype"]], 99)
    state = [IDLE_STATE] * POOL_SLOTS
    for b, s in enumerate(SLOT_OF):
        if s >= 0:
            for name in BUFS:
                junk[name][s] = run.cache[name][b]
            sl, wl, wp = run.states[b]
            state[s] = (sl, wl, wp, sl + wl)
    for name in BUFS:
        getattr(layer, name).copy_(junk[name])
    layer._dev_state.copy_(torch.tensor(state, dtype=torch.int32))
    layer.one_pass = one_pass
    return layer, junk, state


def _ws(layer, q):
    """the cache's step workspace (made before the first call, so that it can be poisoned for it too): the partials region
    filled with 0xFF bytes - a NaN in every float -, the counters left alone"""
    st = getattr(layer, "_step_state", None)
    key = (layer.sink_k.data_ptr(), layer.window_k.data_ptr(), q.shape, q.dtype)
    if st is None or st["key"] != key:
        st = layer._step_consts(key, q)
    B, Hq = q.shape[0], q.shape[1]
    Hkv, D = layer.sink_k.shape[1], q.shape[3]
    assert st["ws"].numel() == R.workspace_bytes(B, Hq, Hkv, layer.num_sink + layer.window_size, D, q.dtype)
    cnt = R.counter_bytes(B, Hkv)
    st["ws"][cnt:] = 0xFF
    return st["ws"], cnt


def _dev(pr):
    return tuple(pr[x].to(DEV) for x in ("q", "k_new", "v_new", "s_aux"))


def _step(layer, mode, inp, one_pass, slots=None, out=None):
    """one fused step with a poisoned workspace; returns (out, path)"""
    q, kn, vn, sa = inp
    ws, cnt = _ws(layer, q)
    if mode == "host":
        out = layer.decode_step(q, kn, vn, s_aux=sa)
    else:
        out = torch.full_like(q, float("nan")) if out is None else out.fill_(float("nan"))
        layer.decode_step_dyn(q, kn, vn, s_aux=sa, out=out, slots=slots)
    path = _native().last_path()
    assert ("1pass" in path) == one_pass, path
    if one_pass:
        assert not ws[:cnt].any(), "one-pass arrival counters must read zero after the call"
    return out, path


KIND = {"host": "_ringstep_", "dyn": "_ringstep_dyn_", "rows": "_ringstep_rows_", "slots": "_ringstep_slots_"}


def _judge(out, L, path, what, kind):
    pl = L["pl"]
    dt = L["pr"]["q"].dtype
    err = maxdiff(out, L["ref"])
    print(f"{what}: {path} | {R.describe(pl, L['rows'])} | max err {err:.2e} (tol {DECODE_TOL[dt]:.1e})")
    assert path.endswith("_" + pl["suffix"]) and kind in path, (what, path, pl["suffix"])
    assert not torch.isnan(out).any(), what
    assert err < DECODE_TOL[dt], (what, err)


def _same_as_twin(layer, run, what):
    """the four buffers bitwise, every byte: the written slot holds k_new / v_new, the planted rows beyond the fill and
    beyond sink_len are untouched"""
    for name in BUFS:
        assert torch.equal(getattr(layer, name).cpu(), run.cache[name]), (what, name)


def _raw_decode(q, sa, one_pass, k=None, v=None, layer=None):
    """sfa_decode (k, v: one contiguous segment) or sfa_decode_ring (layer: its buffers and host state) with a workspace
    of our own - counters zero, partials 0xFF - and a NaN-filled output; the one-pass flag is not reachable through the
    Python wrappers of these two"""
    N = _native()
    lib = N.lib()
    B, Hq, _, D = q.shape
    Hkv = (k if layer is None else layer.sink_k).shape[1]
    n = k.shape[2] if layer is None else layer.sink_len + layer.window_len
    need = lib.sfa_decode_workspace_bytes(B, Hq, Hkv, n, D, N.SFA_DTYPE[q.dtype])
    assert need == R.workspace_bytes(B, Hq, Hkv, n, D, q.dtype)
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    cnt = R.counter_bytes(B, Hkv)
    ws[cnt:] = 0xFF
    out = torch.full_like(q, float("nan"))
    flags = N.FLAG_DECODE_ONE_PASS if one_pass else 0
    tail = (sa.data_ptr(), ws.data_ptr(), ws.numel(), 1.0 / math.sqrt(D), flags, N.stream_ptr(q.device))
    with torch.cuda.device(q.device):
        if layer is None:
            rc, name = lib.sfa_decode(N.desc(q), N.desc(k), N.desc(v), N.desc(out), *tail), "sfa_decode"
        else:
            rc = lib.sfa_decode_ring(N.desc(q), N.desc(layer.sink_k), N.desc(layer.sink_v), layer.sink_len,
                                     N.desc(layer.window_k), N.desc(layer.window_v), layer.window_len, N.desc(out), *tail)
            name = "sfa_decode_ring"
    N.check(rc, name)
    path = N.last_path()
    assert ("1pass" in path) == one_pass, path
    torch.cuda.synchronize()
    if one_pass:
        assert not ws[:cnt].any()
    return out, path


# ------------------------------------------------------------------------------------------------ many, groups
def _host_case(case, one_pass):
    for name, run, _ in P.decode_runs(case):
        mode = "dyn" if name == "dyn" else "host"
        what = f"{case['id']}/{name}/{'1pass' if one_pass else '2launch'}"
        L = run.probe()
        inp = _dev(L["pr"])
        q, kn, vn, sa = inp
        a, b = _layer(run, mode, one_pass), _layer(run, mode, one_pass)
        c = _layer(run, "host", one_pass)                          # the twin that appends, then attends
        out, path = _step(a, mode, inp, one_pass)
        _judge(out, L, path, what, KIND[mode])
        out_b, _ = _step(b, mode, inp, one_pass)
        assert torch.equal(out, out_b), (what, "two runs differ")
        run.apply(L["pr"])
        _same_as_twin(a, run, what)
        if mode == "dyn":
            assert tuple(a._dev_state.tolist()) == run.states[0], what
            ref_out, _ = _step(c, "host", inp, one_pass)           # decode_step_dyn against the host-state step
            assert torch.equal(out, ref_out), (what, "dyn against host state", maxdiff(out, ref_out))
            continue
        assert (a.sink_len, a.window_len, a.write_pos) == run.states[0], what
        # decode_step against append + decode_attention, bitwise
        c.append(kn, vn)
        _same_as_twin(c, run, what + " append")
        ring, rpath = _raw_decode(q, sa, one_pass, layer=c)
        _judge(ring, L, rpath, what + " decode_attention", "_ring_")
        assert torch.equal(out, ring), (what, "decode_step against append + decode_attention", maxdiff(out, ring))
        assert torch.equal(ring, _raw_decode(q, sa, one_pass, layer=c)[0]), (what, "two runs differ")
        if not one_pass:
            assert torch.equal(ring, c.decode_attention(q, s_aux=sa)), what
        if name != "step0":
            continue
        # the same keys linearised: sink_decode_attention
        from sink_attention import sink_decode_attention
        kl, vl = c.get_kv()
        lin, lpath = _raw_decode(q, sa, one_pass, k=kl, v=vl)
        _judge(lin, L, lpath, what + " sink_decode_attention", "decode_splitkv_")
        assert "ring" not in lpath
        assert torch.equal(lin, _raw_decode(q, sa, one_pass, k=kl, v=vl)[0]), (what, "two runs differ")
        if not one_pass:
            assert torch.equal(lin, sink_decode_attention(q, kl, vl, s_aux=sa)), what


@pytest.mark.parametrize("one_pass", ONE_PASS, ids=["2launch", "1pass"])
@pytest.mark.parametrize("case", R.MANY, ids=lambda c: c["id"])
def test_many_splits(case, one_pass):
    """S = 65: two statistics rounds in the reduce kernel, three (W = 32) or two (W = 64) in the one-pass fold, nine O
    rounds, a last split of one key; the fresh slot in split 0, 40 and 64"""
    _host_case(case, one_pass)


@pytest.mark.parametrize("one_pass", ONE_PASS, ids=["2launch", "1pass"])
@pytest.mark.parametrize("case", R.GROUPS, ids=lambda c: c["id"])
def test_head_groups_and_lane_padding(case, one_pass):
    """2 to 5 splits with a partial last one; head loops of 2, 3 and 6 trips; lane groups of 2, 16 and 32 lanes; D = 80
    with six padded lanes"""
    _host_case(case, one_pass)


# ------------------------------------------------------------------------------------------------ fills
def _state_rows(layer, idx):
    return [tuple(r[:3]) for r in layer._dev_state[idx].tolist()]


@pytest.mark.parametrize("one_pass", ONE_PASS, ids=["2launch", "1pass"])
@pytest.mark.parametrize("case", R.FILLS, ids=lambda c: c["id"])
def test_fill_levels_rows_and_slots(case, one_pass):
    """per-sequence rows and slots= on a grid of four splits: empty splits for the short rows, the fresh slot in splits 0 to
    3, a key count that ends on a split edge, rows that fill and wrap within the three steps; an inactive row of the slots
    form gets zeros and nothing of it moves, nor does a slot nobody names"""
    runs = {name: run for name, run, _ in P.decode_runs(case)}
    tag = f"{case['id']}/{'1pass' if one_pass else '2launch'}"
    run = runs["rows"]
    a, b = _layer(run, "rows", one_pass), _layer(run, "rows", one_pass)
    for step in range(R.FILLS_STEPS):
        L = run.probe()
        inp = _dev(L["pr"])
        out, path = _step(a, "rows", inp, one_pass)
        _judge(out, L, path, f"{tag}/rows/{step}", KIND["rows"])
        assert torch.equal(out, _step(b, "rows", inp, one_pass)[0]), (tag, step, "two runs differ")
        run.apply(L["pr"])
        _same_as_twin(a, run, f"{tag}/rows/{step}")
        assert _state_rows(a, slice(None)) == run.states and a._dev_state[:, 3].tolist() == [
            sl + wl + step + 1 for sl, wl, _ in case["states"]], (tag, step)
    run = runs["slots"]
    (a, junk, idle), (b, _, _) = _pool(run, one_pass), _pool(run, one_pass)
    slots = torch.tensor(SLOT_OF, dtype=torch.int32, device=DEV)
    live = [s for s in SLOT_OF if s >= 0]
    off = SLOT_OF.index(-1)
    assert off == P.FILLS_INACTIVE
    for step in range(R.FILLS_STEPS):
        L = run.probe()
        inp = _dev(L["pr"])
        out, path = _step(a, "slots", inp, one_pass, slots=slots)
        _judge(out, L, path, f"{tag}/slots/{step}", KIND["slots"])
        assert not out[off].any(), (tag, step, "inactive row")
        assert torch.equal(out, _step(b, "slots", inp, one_pass, slots=slots)[0]), (tag, step, "two runs differ")
        run.apply(L["pr"])
        for name in BUFS:
            got = getattr(a, name).cpu()
            for bb, s in enumerate(SLOT_OF):
                if s >= 0:
                    assert torch.equal(got[s], run.cache[name][bb]), (tag, step, name, bb, s)
            for s in set(range(POOL_SLOTS)) - set(live):
                assert torch.equal(got[s], junk[name][s]), (tag, step, name, "a slot nobody names", s)
        st = a._dev_state.tolist()
        for bb, s in enumerate(SLOT_OF):
            if s >= 0:
                assert tuple(st[s][:3]) == run.states[bb], (tag, step, bb, s)
        assert all(tuple(st[s]) == IDLE_STATE for s in set(range(POOL_SLOTS)) - set(live)), (tag, step)


@pytest.mark.parametrize("one_pass", ONE_PASS, ids=["2launch", "1pass"])
@pytest.mark.parametrize("case", R.FILLS, ids=lambda c: c["id"])
def test_fill_levels_shared_state(case, one_pass):
    """every fill state alone through the shared-state decode_step_dyn (B = 2), three steps, against the oracle and
    against the host-state decode_step on a twin"""
    tag = f"{case['id']}/{'1pass' if one_pass else '2launch'}"
    for name, run, steps in P.decode_runs(case):
        if not name.startswith("shared"):
            continue
        a, b, h = _layer(run, "dyn", one_pass), _layer(run, "dyn", one_pass), _layer(run, "host", one_pass)
        for step in range(steps):
            L = run.probe()
            inp = _dev(L["pr"])
            out, path = _step(a, "dyn", inp, one_pass)
            _judge(out, L, path, f"{tag}/{name}/{step}", KIND["dyn"])
            assert torch.equal(out, _step(b, "dyn", inp, one_pass)[0]), (tag, name, step, "two runs differ")
            host, hpath = _step(h, "host", inp, one_pass)
            hpl, _ = R.regime(run.case, L["states"], device_state=False)
            assert hpath.endswith("_" + hpl["suffix"]), (hpath, hpl["suffix"])
            nkv = L["rows"][0]["Nkv"]
            if hpl["kps"] == L["pl"]["kps"] or nkv <= min(hpl["kps"], L["pl"]["kps"]):     # the same walk over the keys
                assert torch.equal(out, host), (tag, name, step, "dyn against host state", maxdiff(out, host))
            assert maxdiff(host, L["ref"]) < DECODE_TOL[out.dtype], (tag, name, step)
            run.apply(L["pr"])
            _same_as_twin(a, run, f"{tag}/{name}/{step}")
            _same_as_twin(h, run, f"{tag}/{name}/{step} host")
            assert tuple(a._dev_state.tolist()) == run.states[0] == (h.sink_len, h.window_len, h.write_pos), (tag, name, step)


@pytest.mark.parametrize("one_pass", ONE_PASS, ids=["2launch", "1pass"])
def test_fill_levels_from_a_captured_graph(one_pass):
    """the three steps of the rows form eagerly and from ONE captured graph replayed three times: the same bits in the
    outputs, the buffers and the state"""
    case = R.FILLS[1]
    run = {name: r for name, r, _ in P.decode_runs(case)}["rows"]
    eager, graphed = _layer(run, "rows", one_pass), _layer(run, "rows", one_pass)
    scratch = _layer(run, "rows", one_pass)
    probes = []
    for _ in range(R.FILLS_STEPS):
        probes.append(run.probe())
        run.apply(probes[-1]["pr"])
    static = [t.clone() for t in _dev(probes[0]["pr"])]
    out = torch.full_like(static[0], float("nan"))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                    # warm-up on a layer of its own: the graphed one keeps its state
        scratch.decode_step_dyn(static[0], static[1], static[2], s_aux=static[3])
    torch.cuda.current_stream().wait_stream(side)
    _ws(graphed, static[0])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        graphed.decode_step_dyn(static[0], static[1], static[2], s_aux=static[3], out=out)
    for step, L in enumerate(probes):
        inp = _dev(L["pr"])
        ref, path = _step(eager, "rows", inp, one_pass)
        _judge(ref, L, path, f"graph/{step}", KIND["rows"])
        for s, t in zip(static, inp):
            s.copy_(t)
        _ws(graphed, static[0])
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, ref), (step, maxdiff(out, ref))
    for name in BUFS:
        assert torch.equal(getattr(eager, name), getattr(graphed, name)), name
    _same_as_twin(graphed, run, "graph")
    assert torch.equal(eager._dev_state, graphed._dev_state) and _state_rows(graphed, slice(None)) == run.states
