"""GPU: the short-window kernels at every tile count, window-class edge and strip length (tests/sliding_regime.py).

The hand-placed strip forward (18 bodies) and strip dQ (12 bodies) are picked by strip_asm_nt(W), the skewed dK/dV sweep
takes T(W) trips and the compiled strip kernel sizes its ring from W, the GQA group and num_sink; the rest of the suite
meets almost all of them at W = 128.  Here every case first asks sliding_regime.regime() again with the device's own CU
count and fails if a claim of its row is not met, then
  * calls sfa_fwd + sfa_bwd (sfa_*_varlen for a pack) through the C ABI with O, LSE, dQ, dK, dV and ds_aux NaN-filled and the
    workspace 0xFF-filled (sliding_regime.raw_fwd_bwd) - no NaN may be left;
  * asserts the forward, dQ and dK/dV kernels in sfa_last_path(), the strip length and the ring size included;
  * compares O, LSE, dQ and ds_aux over the whole tensor with the fp64 oracle computed on the device (util.device_oracle) and
    dK / dV element by element with util.assert_within_sum_bound, at the tolerances of
    tests/test_gpu_mask_edges.py::test_dense_mask_edges (util.PROBE_TOL_*: O 2e-2 / 1e-2 abs + rel, dQ 5e-2, dK / dV and
    ds_aux 5e-2 max(1, max |ref|), LSE 5e-3) on mask-edge probe inputs (tests/probe_inputs.py), whose discrimination of the
    short-window mutants tests/test_sliding_regime.py proves on the CPU.  The sum-bound ratios are printed.
The large shapes (`whole`, `ragged_strips`, three `ring` cases) build inputs and reference for probe_B = 2 different batch
elements and repeat them along the batch.

Strip position.  A row's tiles are accumulated in the same order whatever item of a strip it is: tools/asmgen/fwd_strip.py
and dq_strip.py unroll an item's NT tiles oldest first in every block set - the strip's first item and every item whose
tiles do not all exist take the general blocks (one compare per tile against W, or 0 for a tile index below 0), later items
the steady blocks when W = 64 (NT - 1) or one more - and the two sets differ only in sub-blocks that are dead (left out:
their P would be 0, and x + 0 = x) or full (no mask instructions); the MFMA order, the key halves and the deferred rescale
test are shared (tile_sub / emit_M_at / emit_C_at).  So O, LSE and dQ of a row are asserted BITWISE equal between a call
whose strips hold 8 items, one whose strips hold 2 and (forward) one whose every item is a cold start."""
import functools

import pytest
import torch

import range_inputs as RI
import sliding_regime as S
from oracle import sink_oracle as O
from util import (PROBE_TOL_DKDV, PROBE_TOL_DQ, PROBE_TOL_DS_AUX, PROBE_TOL_LSE, PROBE_TOL_O, UNIT_ROUNDOFF, assert_close,
                  assert_within_sum_bound, device_oracle, dkdv_kernel_name, maxdiff)

pytestmark = pytest.mark.gpu
DEV = "cuda"
DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
OUT = ("o", "lse", "dq", "dk", "dv", "ds_aux")


def _n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _reaches(cid):
    r, missed = S.case_regime(cid, _n_cu())
    assert not missed, missed
    return r


def _flags():
    from sink_attention import _native
    return _native.bwd_flags()


@pytest.fixture(scope="module", autouse=True)
def _drop_inputs():
    yield
    _inputs.cache_clear()
    torch.cuda.empty_cache()


def _oracle(q, k, v, do, ns, W, sa, cu=None):
    """util.device_oracle, and for N_q < N_kv (which it does not slice) the same dense oracle unit by unit"""
    if q.shape[2] == k.shape[2]:
        return device_oracle(q, k, v, do, ns, W, sa, cu=cu)
    B, Hq, Hkv = q.shape[0], q.shape[1], k.shape[1]
    g, f64 = Hq // Hkv, torch.float64
    o, dq = (torch.zeros(q.shape, dtype=f64, device=q.device) for _ in range(2))
    dk, dv, a_k, a_v = (torch.zeros(k.shape, dtype=f64, device=q.device) for _ in range(4))
    lse = torch.zeros(q.shape[:3], dtype=f64, device=q.device)
    dsa = None if sa is None else torch.zeros(Hq, dtype=f64, device=q.device)
    for b in range(B):
        for hk in range(Hkv):
            uq, uk = (slice(b, b + 1), slice(hk * g, (hk + 1) * g)), (slice(b, b + 1), slice(hk, hk + 1))
            s = None if sa is None else sa[uq[1]].float()
            o[uq], lse[uq] = O.sink_attention_dense(q[uq], k[uk], v[uk], ns, W, s)
            r = O.sink_attention_bwd_dense(q[uq], k[uk], v[uk], do[uq], ns, W, s, bounds=True, tiny=torch.finfo(q.dtype).tiny)
            dq[uq], dk[uk], dv[uk], a_k[uk], a_v[uk] = r[0], r[1], r[2], r[4], r[5]
            if dsa is not None:
                dsa[uq[1]] += r[3]
    return o, lse, dq, dk, dv, dsa, a_k, a_v


def _spread(x, rep, layout):
    """the base batch repeated rep times; "bnhd": stored [B, N, H, D], passed as the transposed view"""
    x = x.repeat(rep, 1, 1, 1) if rep > 1 else x
    return x.transpose(1, 2).contiguous().transpose(1, 2) if layout == "bnhd" else x


@functools.lru_cache(maxsize=None)
def _inputs(cid, family="probe"):
    """device inputs of a case and the fp64 reference of its base batch, built once and shared by every test of the module.
    The cache has no limit: the inputs and references of all cases (about 3 GB) stay on the device until the module ends
    (_drop_inputs), which spares the determinism and strip-length tests a second oracle run."""
    c = S.CASES[cid]
    if family == "probe":
        src = S.case_probe(c)
    else:
        src = RI.dense_range(family, c["probe_B"], c["Hq"], c["Hkv"], c["Nq"], c["Nk"], c["D"], c["ns"], c["W"], DT[c["dtype"]], 17)
        cov = RI.coverage(RI.tile_walk(src["q"][:1, :4], src["k"][:1, :1], src["v"][:1, :1], c["ns"], c["W"], src["s_aux"][:4])[2])
        # the inputs do rescale between blocks: mid-range alpha in most 64-row waves (a wave sees two steps of the staircase
        # at most when W = 65, so not in all of them)
        assert cov["mid"] >= 64 and 2 * cov["waves_mid"] >= cov["waves"] > 0, cov
    base = {x: src[x].to(DEV) for x in ("q", "k", "v", "do")}
    sa = None if src["s_aux"] is None else src["s_aux"].to(DEV)
    cu = S.case_cu(c)
    ref = _oracle(base["q"], base["k"], base["v"], base["do"], c["ns"], c["W"], sa, cu)
    rep = c["B"] // c["probe_B"]
    assert rep * c["probe_B"] == c["B"]
    full = {x: _spread(t, rep, c["layout"]) for x, t in base.items()}
    return dict(full, s_aux=sa, ref=ref, rep=rep, cu=cu)


def _call(c, inp, W=None, sel=None):
    """the raw call of a case (sel: a (batch slice, q head slice, KV head slice) of it, passed as views)"""
    q, k, v, do = (inp[x] for x in ("q", "k", "v", "do"))
    sa = inp["s_aux"]
    if sel is not None:
        b, hq, hk = sel
        q, do, k, v = q[b, hq], do[b, hq], k[b, hk], v[b, hk]
        sa = None if sa is None else sa[hq].contiguous()
    return S.raw_fwd_bwd(q, k, v, do, sa, c["ns"], c["W"] if W is None else W, _flags(), cu=inp["cu"])


def _want_paths(c, r, dt):
    if r["fwd"].startswith("stripasm"):
        fwd = "%s_len%d" % (r["fwd"], r["L"])
    elif r["fwd"] == "strip":
        fwd = "_strip%d_ring%d_hpw%d" % (r["strip"], r["R"], r["hpw"])
    else:
        fwd = "_%s_hpw" % r["fwd"]
    packed = bool(c["lens"])
    B, N, Nk = (len(c["lens"]), max(c["lens"]), max(c["lens"])) if packed else (c["B"], c["Nq"], c["Nk"])
    dkdv = "dkdvasmskew" if r["skew"] else dkdv_kernel_name("rule", B, c["Hkv"], N, Nk, c["D"], c["W"], packed=packed, dtype=dt, ns=c["ns"])
    return fwd, r["dq"], dkdv


def _assert_paths(c, r, out, what):
    fwd, dq, dkdv = _want_paths(c, r, DT[c["dtype"]])
    assert fwd in out["fwd_path"], (what, fwd)
    assert dq in out["bwd_path"] and (dkdv is None or dkdv in out["bwd_path"]), (what, dq, dkdv)
    assert ("dkdvasmskew" in out["bwd_path"]) == r["skew"], what


def _check(out, inp, dt, what, tol=None):
    """no NaN left (the poison), then parity with the base batch's reference, one repetition of it at a time"""
    o_r, lse_r, dq_r, dk_r, dv_r, dsa_r, a_k, a_v = inp["ref"]
    for name in OUT:
        if out[name] is not None:
            n_nan = int(torch.isnan(out[name]).sum())
            assert n_nan == 0, f"{what}: {n_nan} of {out[name].numel()} elements of {name} were never written (still NaN)"
    u, Bp = UNIT_ROUNDOFF[dt], o_r.shape[0]
    to, tq, tkv, tl, ta = tol or (PROBE_TOL_O[dt], PROBE_TOL_DQ, PROBE_TOL_DKDV, PROBE_TOL_LSE, PROBE_TOL_DS_AUX)
    fin = torch.isfinite(lse_r)
    fig = dict(lse=0.0, dk=0.0, dv=0.0)
    for i in range(inp["rep"]):
        sl = slice(i * Bp, (i + 1) * Bp)
        assert_close(out["o"][sl], o_r, to, to, what + " o")
        assert_close(out["dq"][sl], dq_r, tq, tq, what + " dq")
        assert_close(out["dk"][sl], dk_r, tkv * max(1.0, dk_r.abs().max().item()), tkv, what + " dk")
        assert_close(out["dv"][sl], dv_r, tkv * max(1.0, dv_r.abs().max().item()), tkv, what + " dv")
        fig["lse"] = max(fig["lse"], maxdiff(out["lse"][sl][fin], lse_r[fin]))
        fig["dk"] = max(fig["dk"], assert_within_sum_bound(out["dk"][sl], dk_r, a_k, u, what + " dk"))
        fig["dv"] = max(fig["dv"], assert_within_sum_bound(out["dv"][sl], dv_r, a_v, u, what + " dv"))
    e_dsa, t_dsa = 0.0, 0.0
    if dsa_r is not None:
        e_dsa, t_dsa = maxdiff(out["ds_aux"], dsa_r * inp["rep"]), ta * max(1.0, (dsa_r * inp["rep"]).abs().max().item())
    print(f"{what}: lse {fig['lse']:.3g} / {tl}, ds_aux {e_dsa:.3g} / {t_dsa:.3g}, sum-bound ratio dk {fig['dk']:.3f} dv {fig['dv']:.3f}")
    assert fig["lse"] < tl and (dsa_r is None or e_dsa < t_dsa), (what, fig, e_dsa, t_dsa)


def _run(cid):
    r = _reaches(cid)
    c = S.CASES[cid]
    inp = _inputs(cid)
    out = _call(c, inp)
    what = f"{cid} [{out['fwd_path']} | {out['bwd_path']}]"
    _assert_paths(c, r, out, what)
    _check(out, inp, DT[c["dtype"]], what)
    return r, c, inp, out, what


def _same(a, b, names, what, sl=None):
    for x in names:
        got = b[x] if sl is None else b[x][sl]
        assert not torch.isnan(a[x]).any(), (what, x)
        assert torch.equal(a[x], got), f"{what}: {x} differs ({int((a[x] != got).sum())} of {got.numel()} elements)"


# ------------------------------------------------------------------------------------------------ the tables
@pytest.mark.parametrize("cid", sorted(S.EDGES))
def test_edges_every_body_at_both_ends_of_its_window_class(cid):
    """L = 1: every item is a cold start.  W = 194 runs what takes over from the hand-placed bodies."""
    _run(cid)


@pytest.mark.parametrize("cid", sorted(S.WHOLE))
def test_whole_sequence_strips_are_independent_of_the_strip_length(cid):
    """one strip per sequence (L = 8: seven items on a sliding ring, steady blocks from item NT - 1 on), then four batch
    elements of it alone (L = 2, the dQ strip body still) and one (batch, KV head) alone (L = 1, forward strip body only: the
    grid is too small for the dQ one): bitwise, see the module docstring"""
    r, c, inp, out, what = _run(cid)
    g, n_cu = c["Hq"] // c["Hkv"], _n_cu()
    sub = S.regime(4, c["Hq"], c["Hkv"], c["Nq"], c["Nk"], c["D"], c["ns"], c["W"], n_cu)
    strip_dq = r["dq"].startswith("dqstripasm")            # (D = 96 has no strip dQ body: its dQ kernel changes with the grid)
    assert sub["fwd"] == r["fwd"] and (sub["dq"] == r["dq"] or not strip_dq) and 1 < sub["L"] < r["L"], (sub["L"], sub["dq"])
    b = slice(5, 9)
    part = _call(c, inp, sel=(b, slice(None), slice(None)))
    assert "%s_len%d" % (sub["fwd"], sub["L"]) in part["fwd_path"] and sub["dq"] in part["bwd_path"], (part["fwd_path"], part["bwd_path"])
    _same(part, out, ("o", "lse", "dq") if strip_dq else ("o", "lse"), what + " batch 5..8 alone", b)
    one = S.regime(1, g, 1, c["Nq"], c["Nk"], c["D"], c["ns"], c["W"], n_cu)
    assert one["fwd"] == r["fwd"] and one["L"] == 1
    hk = 11
    sel = (slice(3, 4), slice(hk * g, (hk + 1) * g), slice(hk, hk + 1))
    alone = _call(c, inp, sel=sel)
    assert "%s_len1" % one["fwd"] in alone["fwd_path"], alone["fwd_path"]
    for x in ("o", "lse"):
        assert torch.equal(alone[x], out[x][sel[0], sel[1]]), f"{what}: {x} of (batch 3, KV head {hk}) depends on the strip length"


@pytest.mark.parametrize("cid", sorted(S.RAGGED))
def test_ragged_last_strip(cid):
    """strips of 6 items and a last one of 2, in [B, N, H, D] storage; the general blocks in steady position (W = 33, 66, 130)"""
    _run(cid)


@pytest.mark.parametrize("cid", sorted(S.PACK))
def test_pack_short_sequences_in_the_strip_bodies(cid):
    """a sequence of one row, sequences shorter than the window of an NT = 4 body, blocks that exit at q0 >= N; then the
    200-row sequence alone through the dense call: the same kernels (checked), bitwise"""
    r, c, inp, out, what = _run(cid)
    cu = inp["cu"]
    a, b = cu[4], cu[5]
    q, k, v, do = (inp[x][:, :, a:b] for x in ("q", "k", "v", "do"))
    alone = S.raw_fwd_bwd(q, k, v, do, inp["s_aux"], c["ns"], c["W"], _flags())
    assert r["fwd"] in alone["fwd_path"] and r["dq"] in alone["bwd_path"], (alone["fwd_path"], alone["bwd_path"])
    for x in ("o", "dq"):
        assert torch.equal(alone[x], out[x][:, :, a:b]), f"{what}: {x} of sequence {a}:{b} depends on the pack"
    assert torch.equal(alone["lse"], out["lse"][:, :, a:b]), f"{what}: lse of sequence {a}:{b} depends on the pack"


@pytest.mark.parametrize("cid", sorted(S.SKEW))
def test_skew_trip_counts(cid):
    """T = 6 .. 18, both sides of a step of T, W = 512 | 513, MHA, N < W; four key blocks, the last of 13 keys"""
    _run(cid)


@pytest.mark.parametrize("cid", sorted(S.RING))
def test_compiled_strip_ring(cid):
    """ring slots reused inside a strip, resident sink tiles, q tiles that fetch more than the prefetched tile, N_q < N_kv,
    a pack with a sequence shorter than a q tile; both sides of the LDS cap and of W = 256 | 257"""
    _run(cid)


# ------------------------------------------------------------------------------------------------ further tests
@pytest.mark.parametrize("cid", ["whole_d64_bf16_w65", "whole_d80_fp16_w129", "whole_d96_bf16_w193"])
def test_staircase_rescale_in_steady_items(cid):
    """range_inputs staircase_up at the `whole` shape, one NT class each: the between-blocks rescale (2^-16 <= alpha < 2^-8)
    in items that run on a sliding ring, LSE checked; tolerances of tests/test_gpu_softmax_range.py"""
    r = _reaches(cid)
    assert r["steady_items"] >= 4
    c = S.CASES[cid]
    dt = DT[c["dtype"]]
    inp = _inputs(cid, "staircase_up")
    out = _call(c, inp)
    what = f"{cid} staircase [{out['fwd_path']} | {out['bwd_path']}]"
    _assert_paths(c, r, out, what)
    o_r, lse_r, dq_r, dk_r, dv_r, dsa_r = inp["ref"][:6]
    Bp = o_r.shape[0]
    for i in range(inp["rep"]):
        sl = slice(i * Bp, (i + 1) * Bp)
        fig = {"o": (maxdiff(out["o"][sl], o_r), RI.TOL_O[dt]), "lse": (maxdiff(out["lse"][sl], lse_r), RI.TOL_LSE)}
        for name, ref in (("dq", dq_r), ("dk", dk_r), ("dv", dv_r)):
            fig[name] = (maxdiff(out[name][sl], ref), RI.grad_tol(dt, ref.cpu()))
        if i == 0:
            print(what, {k: "%.3g / %.3g" % v for k, v in fig.items()})
        bad = {k: v for k, v in fig.items() if not v[0] < v[1]}
        assert not bad, (what, i, bad)
    assert maxdiff(out["ds_aux"], dsa_r * inp["rep"]) < RI.grad_tol(dt, (dsa_r * inp["rep"]).cpu(), aux=True)


@pytest.mark.parametrize("cid", ["whole_d80_fp16_w193", "ragged_d80_bf16_w66", "pack_d96_fp16_w65", "skew_d96_fp16_w512",
                                 "skew_d64_fp16_w162", "ring_pack_g3_w256", "ring_hpw8_g8_ns64_w65"])
def test_the_same_call_twice_is_bitwise_equal(cid):
    """dK / dV of the skewed sweep included: every workgroup owns its 256 keys, nothing is accumulated across workgroups"""
    _reaches(cid)
    c, inp = S.CASES[cid], _inputs(cid)
    a, b = _call(c, inp), _call(c, inp)
    assert a["fwd_path"] == b["fwd_path"] and a["bwd_path"] == b["bwd_path"]
    _same(a, b, [x for x in OUT if a[x] is not None], cid)


def test_both_sides_of_the_lds_cap_agree():
    """the inputs of the side that fits (W = 129: strip kernel, 4 + 1 slots = 160 KiB) run at W = 130 too (fwd_mfma_kernel):
    rows at positions below 129 see the same keys under both windows, and their O agrees within the O tolerance.  Those rows
    are causal under both windows - no window edge and no reused ring slot enters this comparison; it shows only that the
    two kernels agree where their masks do.  The window edge and the ring reuse of the pair are judged by each side's own
    oracle run in test_compiled_strip_ring."""
    fits, over = S.LDS_CAP_PAIR
    rf, ro = _reaches(fits), _reaches(over)
    c, inp = S.CASES[fits], _inputs(fits)
    a, b = _call(c, inp), _call(c, inp, W=S.CASES[over]["W"])
    assert _want_paths(c, rf, DT[c["dtype"]])[0] in a["fwd_path"] and "_nw4_hpw" in b["fwd_path"], (a["fwd_path"], b["fwd_path"])
    rows = slice(0, c["W"])
    to = PROBE_TOL_O[DT[c["dtype"]]]
    assert_close(a["o"][:, :, rows], b["o"][:, :, rows].double(), to, to, "strip against nw4")
    assert maxdiff(a["lse"][:, :, rows], b["lse"][:, :, rows]) < PROBE_TOL_LSE
