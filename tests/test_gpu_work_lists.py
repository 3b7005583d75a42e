"""GPU: the work-list (forward, dQ) and ticketed (dK/dV) kernels on grids of several rounds, every item checked.

Almost every other shape of the suite has at most one item per CU: one round, no dynamic tail, no tickets.  The cases of
tests/grid_regime.py reach the rest - partial last rounds, the three heads-per-workgroup forms, the dQ tail claimed from a
workspace counter, ticket queues with remainders and both block orders, sink-split extras ahead of ticketed workgroups, the
row split, packed lists with holes, the strip kernels - and each test first asserts, with the device's own CU count, that
its case does reach the regime it is there for.  A list error skips an item or computes the wrong one, so
  * every output and the whole workspace are poisoned before the call (NaN / 0xFF bytes: grid_regime.raw_fwd_bwd; through
    the packed op only best effort, see _poison_allocator) and no NaN may be left;
  * O, LSE, dQ, dK, dV and ds_aux are compared over the WHOLE tensor with the fp64 oracle computed on the device
    (util.device_oracle): O 2e-2 + 2e-2 |ref| (fp16: 5e-3, as tools/fuzz.py), dQ 5e-2 + 5e-2 |ref|, LSE 5e-3
    (tests/test_gpu_softmax_range.py), ds_aux 1.5 (tests/test_gpu_varlen.py), dK / dV element by element within the
    derived sum bound (util.assert_within_sum_bound; the largest ratio is printed);
  * O, LSE and dQ of the full call equal, bit for bit, those of every batch element / sequence run alone (a shorter list):
    an item's result does not depend on where in a list it ran or whether it was claimed from the tail.  dK / dV are left
    out of that: their split plan changes with the grid.
The stale-counter tests reuse one workspace across calls and replay a captured graph: the counters must be zeroed by every
call, not by whoever allocated the workspace."""
import functools

import pytest
import torch

import grid_regime as R
from util import UNIT_ROUNDOFF, assert_close, assert_within_sum_bound, device_oracle, dkdv_kernel_name, maxdiff, rand

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL_O = {torch.bfloat16: 2e-2, torch.float16: 5e-3}
TOL_DQ, TOL_LSE, TOL_DS_AUX = 5e-2, 5e-3, 1.5
DENSE = [(n, D) for n, c in R.DENSE_CASES.items() for D in c["Ds"]]
PACKED = [(n, D) for n, c in R.PACKED_CASES.items() for D in c["Ds"]]


def _n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _reaches(name, D):
    r, missed = R.case_regime(name, D, _n_cu())
    assert not missed, missed
    return r


def _flags():
    from sink_attention import _native
    return _native.bwd_flags()


@pytest.fixture(scope="module", autouse=True)
def _drop_references():
    """the inputs and fp64 references are computed once per case and shared by every test of the module (about 6 GB on the
    device between them); they go when the module is done"""
    yield
    _dense.cache_clear()
    _packed.cache_clear()
    torch.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def _dense(name, D):
    """device inputs and the whole-tensor fp64 reference of a dense case (shared by the dK/dV modes and the counter tests)"""
    c = R.DENSE_CASES[name]
    B, Hq, Hkv, N, ns, W = c["shape"]
    dt = getattr(torch, c["dtype"])
    g = torch.Generator().manual_seed(101 + D)
    q, k, v, do = (rand(s, g, dt).to(DEV) for s in ((B, Hq, N, D), (B, Hkv, N, D), (B, Hkv, N, D), (B, Hq, N, D)))
    sa = rand((Hq,), g, torch.float32, 0.5).to(DEV)
    return (q, k, v, do, sa), device_oracle(q, k, v, do, ns, W, sa)


@functools.lru_cache(maxsize=None)
def _packed(name, D):
    c = R.PACKED_CASES[name]
    cu = [0]
    for n in c["lens"]:
        cu.append(cu[-1] + n)
    T, dt = cu[-1], getattr(torch, c["dtype"])
    g = torch.Generator().manual_seed(211 + D)
    q, k, v, do = (rand(s, g, dt).to(DEV) for s in ((1, c["Hq"], T, D), (1, c["Hkv"], T, D), (1, c["Hkv"], T, D), (1, c["Hq"], T, D)))
    sa = rand((c["Hq"],), g, torch.float32, 0.5).to(DEV)
    return (q, k, v, do, sa), cu, device_oracle(q, k, v, do, c["ns"], c["W"], sa, cu=cu)


def _check(got, ref, dt, what):
    """got: o, lse, dq, dk, dv, ds_aux of the kernels; ref: device_oracle's tuple.  No NaN first (the poison), then parity."""
    o_r, lse_r, dq_r, dk_r, dv_r, dsa_r, a_k, a_v = ref
    for name, t in zip(("o", "lse", "dq", "dk", "dv", "ds_aux"), got):
        n_nan = int(torch.isnan(t).sum())
        assert n_nan == 0, f"{what}: {n_nan} of {t.numel()} elements of {name} were never written (still NaN)"
    o, lse, dq, dk, dv, dsa = got
    assert_close(o, o_r, TOL_O[dt], TOL_O[dt], what + " o")
    fin = torch.isfinite(lse_r)
    e_lse = maxdiff(lse[fin], lse_r[fin])
    assert_close(dq, dq_r, TOL_DQ, TOL_DQ, what + " dq")
    u = UNIT_ROUNDOFF[dt]
    e_dsa = maxdiff(dsa, dsa_r)
    print(f"{what}: lse {e_lse:.3g} / {TOL_LSE}, ds_aux {e_dsa:.3g} / {TOL_DS_AUX}", end="")
    assert e_lse < TOL_LSE and e_dsa < TOL_DS_AUX, (what, e_lse, e_dsa)
    r_k = assert_within_sum_bound(dk, dk_r, a_k, u, what + " dk")
    r_v = assert_within_sum_bound(dv, dv_r, a_v, u, what + " dv")
    print(f", sum-bound ratio dk {r_k:.3f} dv {r_v:.3f}")


OUT = ("o", "lse", "dq", "dk", "dv", "ds_aux")


@pytest.mark.parametrize("name,D", DENSE)
def test_dense_lists_every_item(name, D, dkdv):
    r = _reaches(name, D)
    c = R.DENSE_CASES[name]
    B, Hq, Hkv, N, ns, W = c["shape"]
    (q, k, v, do, sa), ref = _dense(name, D)
    dt, flags = q.dtype, _flags()
    out = R.raw_fwd_bwd(q, k, v, do, sa, ns, W, flags)
    what = f"{name} d{D} {dkdv} [{out['fwd_path']} | {out['bwd_path']}]"
    assert r["fwd"] in out["fwd_path"] and r["dq"] in out["bwd_path"], what
    want = dkdv_kernel_name(dkdv, B, Hkv, N, N, D, W, dtype=dt, ns=ns)
    assert want in out["bwd_path"], (want, what)
    assert out["bwd_path"].endswith("_overlap") == r["dq_side_stream"], what
    _check([out[x] for x in OUT], ref, dt, what)
    # position independence: every batch element alone, a shorter list (one round where the case has three)
    assert R.regime(1, Hq, Hkv, N, D, ns, W, _n_cu())["rounds"] < r["rounds"]
    for b in range(B):
        sl = slice(b, b + 1)
        alone = R.raw_fwd_bwd(q[sl], k[sl], v[sl], do[sl], sa, ns, W, flags)
        for x in ("o", "lse", "dq"):
            assert not torch.isnan(alone[x]).any(), (what, b, x)
            assert torch.equal(alone[x], out[x][sl]), f"{what}: {x} of batch element {b} depends on its place in the list"


def _poison_allocator(*tensors):
    """Best effort only: the op allocates its outputs with torch.empty, and the caching allocator tends to hand back the block
    freed last of a fitting size - here blocks of the outputs' sizes that were just filled with NaN.  Nothing guarantees
    that it does; the raw-ABI tests above poison for certain."""
    junk = [torch.full_like(t, float("nan")) for t in tensors]
    torch.cuda.synchronize()
    del junk


@pytest.mark.parametrize("name,D", PACKED)
def test_packed_lists_with_holes_and_strips(name, D, dkdv):
    from sink_attention import _native
    from sink_attention.sink_flash_attention import _sink_flash_attention_ex
    from sink_attention.varlen import sink_flash_attention_varlen
    r = _reaches(name, D)
    c = R.PACKED_CASES[name]
    Hq, Hkv, ns, W = c["Hq"], c["Hkv"], c["ns"], c["W"]
    (q, k, v, do, sa), cu, ref = _packed(name, D)
    dt = q.dtype
    qd, kd, vd, sad = (t.clone().requires_grad_(True) for t in (q, k, v, sa))
    _poison_allocator(q, torch.empty(Hq, cu[-1], device=DEV))
    out = sink_flash_attention_varlen(qd, kd, vd, cu, num_sink=ns, window_size=W, s_aux=sad)
    fwd_path = _native.last_path()
    lse = out.grad_fn.saved_tensors[4]
    assert lse.shape == (Hq, cu[-1])
    _poison_allocator(q, k, v)
    out.backward(do)
    what = f"{name} d{D} {dkdv} [{fwd_path} | {_native.last_path()}]"
    assert r["fwd"] in fwd_path and r["dq"] in _native.last_path(), what
    longest = max(c["lens"])
    want = dkdv_kernel_name(dkdv, len(c["lens"]), Hkv, longest, longest, D, W, packed=True, dtype=dt, ns=ns)
    assert want in _native.last_path(), (want, what)
    _check([out.detach(), lse.unsqueeze(0), qd.grad, kd.grad, vd.grad, sad.grad], ref, dt, what)
    for a, b in zip(cu[:-1], cu[1:]):
        if b > a:
            alone = _sink_flash_attention_ex(q[:, :, a:b], k[:, :, a:b], v[:, :, a:b], ns, W, s_aux=sa)
            assert torch.equal(alone, out.detach()[:, :, a:b]), f"{what}: O of sequence {a}:{b} depends on the pack"


def _same(a, b, what):
    for x in OUT:
        assert not torch.isnan(a[x]).any(), (what, x)
        assert torch.equal(a[x], b[x]), f"{what}: {x} differs"


@pytest.mark.parametrize("name,D", [("mha", 128), ("tail", 64)])
def test_stale_counters_in_a_reused_workspace(name, D, dkdv):
    """The ticket heads (mha, tail) and the dQ tail counter (tail) are zeroed by the call that uses them: two backward
    calls on one workspace, the second on the counters the first left, each equal to a call on a fresh poisoned workspace.
    (The 0xFF poison alone does not show a missing memset: a counter of 0xFFFFFFFF wraps to 0 at its first claim, which
    costs one claim and no item.  The counters a finished call leaves behind are past the end of their queues, and a call
    that starts from those claims nothing - profiles/worklist_mutants.log.)"""
    r = _reaches(name, D)
    assert r["tickets"] and (name != "tail" or r["dq_tail"])
    ns, W = R.DENSE_CASES[name]["shape"][4:]
    (q, k, v, do, sa), _ = _dense(name, D)
    flags = _flags()
    fresh = [R.raw_fwd_bwd(q, k, v, do, sa, ns, W, flags, do_scale=s) for s in (None, 0.5)]
    first = R.raw_fwd_bwd(q, k, v, do, sa, ns, W, flags)
    second = R.raw_fwd_bwd(q, k, v, do, sa, ns, W, flags, ws=first["ws"], do_scale=0.5)
    assert second["ws"] is first["ws"]
    _same(first, fresh[0], f"{name} d{D} {dkdv} first call")
    _same(second, fresh[1], f"{name} d{D} {dkdv} second call on the first one's workspace")
    assert not torch.equal(first["dq"], second["dq"])


def test_stale_counters_under_graph_replay(dkdv):
    """forward + backward of `mha` captured in one graph (memset nodes, the ticketed kernel, the side-stream fork) and
    replayed twice on the same workspace with q changed in between: each replay equals the eager call"""
    name, D = "mha", 128
    r = _reaches(name, D)
    assert r["tickets"]
    ns, W = R.DENSE_CASES[name]["shape"][4:]
    (q, k, v, do, sa), _ = _dense(name, D)
    flags = _flags()
    q2 = q * 0.5
    eager = [R.raw_fwd_bwd(x, k, v, do, sa, ns, W, flags) for x in (q, q2)]
    qs = q.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        bufs = R.raw_fwd_bwd(qs, k, v, do, sa, ns, W, flags)            # warm-up on a side stream, as capture asks
    torch.cuda.current_stream().wait_stream(side)

    def poison(ws):
        for x in OUT:
            bufs[x].fill_(float("nan"))
        if ws:
            bufs["ws"].fill_(0xFF)

    poison(True)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        R.raw_fwd_bwd(qs, k, v, do, sa, ns, W, flags, out=bufs)
    poison(True)
    graph.replay()
    torch.cuda.synchronize()
    _same(bufs, eager[0], f"mha {dkdv} first replay")
    poison(False)                                                       # the workspace stays as the first replay left it
    qs.copy_(q2)
    graph.replay()
    torch.cuda.synchronize()
    _same(bufs, eager[1], f"mha {dkdv} second replay")
