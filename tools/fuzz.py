#!/usr/bin/env python3
"""Randomised cross-check on the GPU: MFMA kernels against the exact-f32 kernels of the same library (and the
N_q < N_kv / packed paths against their padded / per-sequence formulations) on random shapes.
usage: python tools/fuzz.py [n_cases] [seed] [skew] [--inputs=randn|probe|range|dsaux]
(skew: only shapes of the short-window dK/dV kernel - no sink keys, head dims 64 / 80 / 96, windows up to 512, N_q = N_kv or
packed; --inputs=probe: q / k / v / dO from tests/probe_inputs.py, rows peaked on one key of a mask edge, instead of randn
(without sink keys the window is then drawn from tests/sliding_regime.py::EDGE_WINDOWS, the class edges of the short-window kernels),
and dK / dV of the MFMA kernels also judged element by element against the fp64 oracle with the sum bound of tests/util.py
(4 u A + u |ref|), which a mask error confined to the dK/dV kernel cannot pass;
--inputs=range: a random family of tests/range_inputs.py - logit staircases, a common offset - that moves the softmax reference;
--inputs=dsaux: the problem of tests/dsaux_inputs.py - s_aux calibrated to p_aux about 1/2 with per-head offsets, dO = sign(o_ref) on
one random row class and 0 elsewhere, at most 500 rows - and ds_aux of the MFMA path also judged against the fp64 oracle under the
class's own bound 4 u A + u |ref|)"""
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "sink-flash-attention-kernel_amd"), ROOT, os.path.join(ROOT, "tests")]
import torch

import dsaux_inputs
import probe_inputs
import range_inputs
import sliding_regime
import util

from sink_attention.sink_flash_attention import _sink_flash_attention_ex
from sink_attention.varlen import sink_flash_attention_varlen

inputs = ([a.split("=", 1)[1] for a in sys.argv if a.startswith("--inputs=")] or ["randn"])[-1]
assert inputs in ("randn", "probe", "range", "dsaux"), inputs
sys.argv = [a for a in sys.argv if not a.startswith("--inputs=")]
n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 100
rng = random.Random(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
torch.manual_seed(rng.randrange(1 << 30))
focus_skew = len(sys.argv) > 3 and sys.argv[3] == "skew"
bad = 0
DSAUX = {}          # --inputs=dsaux: the problem and the class of the last draw


def draw(B, Hq, Hkv, Nq, Nk, D, ns, W, dt, cu=None):
    """q, k, v, dO on the GPU: randn, or the mask-edge probes of the same shapes"""
    if inputs == "probe":
        pr = probe_inputs.dense_probe(B, Hq, Hkv, Nq, Nk, D, ns, W, dt, rng.randrange(1 << 30), cu=cu)
        return tuple(pr[x].cuda() for x in ("q", "k", "v", "do"))
    if inputs == "dsaux":
        pr = dsaux_inputs.build(B, Hq, Hkv, Nq, D, dt, ns, W, Nk=Nk, cu=cu, seed=rng.randrange(1 << 30))
        DSAUX.update(pr=pr, cls=rng.choice(sorted(pr["classes"])))
        return tuple(x.cuda() for x in (pr["q"], pr["k"], pr["v"], dsaux_inputs.make_do(pr, pr["classes"][DSAUX["cls"]])))
    if inputs == "range":
        fam = rng.choice(("staircase_up", "staircase_down", "offset"))
        pr = range_inputs.dense_range(fam, B, Hq, Hkv, Nq, Nk, D, ns, W, dt, rng.randrange(1 << 30), cu=cu)
        return tuple(pr[x].cuda() for x in ("q", "k", "v", "do"))
    return (torch.randn(B, Hq, Nq, D, device="cuda", dtype=dt), torch.randn(B, Hkv, Nk, D, device="cuda", dtype=dt),
            torch.randn(B, Hkv, Nk, D, device="cuda", dtype=dt), torch.randn(B, Hq, Nq, D, device="cuda", dtype=dt))


def calibrated(sa):
    """--inputs=dsaux: the s_aux that belongs to the tensors just drawn"""
    return DSAUX["pr"]["s_aux"].cuda() if inputs == "dsaux" else sa


def run(q, k, v, do, ns, W, sa, generic):
    qq, kk, vv = (t.clone().requires_grad_(True) for t in (q, k, v))
    ss = sa.clone().requires_grad_(True) if sa is not None else None
    o = _sink_flash_attention_ex(qq, kk, vv, ns, W, s_aux=ss, force_generic=generic)
    o.backward(do)
    return [o.detach().float(), qq.grad.float(), kk.grad.float(), vv.grad.float()] + ([ss.grad.float()] if ss is not None else [])


def sum_bound_ratios(q, k, v, do, ns, W, sa, cu, dk, dv):
    """largest |dK - ref| and |dV - ref| over the sum bound of tests/util.py; fp64 oracle on the CPU, one sequence and one
    (batch, KV head) group at a time (N_q < N_kv has the dense oracle only)"""
    worst = [0.0, 0.0]
    cu = cu or [0, k.shape[2]]
    off = k.shape[2] - q.shape[2]                                       # (N_q < N_kv: one sequence)
    g, u = q.shape[1] // k.shape[1], util.UNIT_ROUNDOFF[q.dtype]
    q, k, v, do, dk, dv = (x.cpu() for x in (q, k, v, do, dk.to(q.dtype), dv.to(q.dtype)))
    for s0, s1 in zip(cu[:-1], cu[1:]):
        for b in range(q.shape[0] if s1 > s0 else 0):
            for hk in range(k.shape[1]):
                bq, bk = (slice(b, b + 1), slice(hk * g, (hk + 1) * g)), (slice(b, b + 1), slice(hk, hk + 1), slice(s0, s1))
                ref = util.oracle_bwd(q[bq][:, :, s0:s1 - off], k[bk], v[bk], do[bq][:, :, s0:s1 - off], ns, W,
                                      None if sa is None else sa[bq[1]].cpu(), banded=off == 0 and s1 - s0 > 1024, bounds=True)
                worst[0] = max(worst[0], util.sum_bound_ratio(dk[bk], ref[1], ref[4], u))
                worst[1] = max(worst[1], util.sum_bound_ratio(dv[bk], ref[2], ref[5], u))
    return worst


for case in range(n_cases):
    D = rng.choice([32, 64, 80, 96, 128, 128, 256])
    Hkv = rng.choice([1, 2, 4])
    g = rng.choice([1, 2, 4, 8])
    Hq = Hkv * g
    B = rng.choice([1, 2])
    N = rng.choice([1, 7, 31, 33, 64, 65, 100, 127, 128, 129, 200, 257, 500, 777, 1024, 1500, 2500, 4100])
    ns = rng.choice([0, 1, 4, 63, 64, 65, 130])
    W = rng.choice([0, 1, 5, 31, 64, 100, 128, 300, 1000, 4096])
    dt = rng.choice([torch.bfloat16, torch.float16])
    aux = rng.random() < 0.6
    mode = rng.choice(["plain", "plain", "offset", "varlen"])
    if focus_skew:
        D, ns, W = rng.choice([64, 80, 96]), 0, rng.choice([1, 5, 31, 64, 100, 128, 300, 512])
        mode = rng.choice(["plain", "plain", "varlen"])
    if inputs == "probe" and ns == 0:
        # the class edges of the short-window kernels (tiles per item, trips of the skewed sweep, the dispatch windows)
        W = rng.choice(sliding_regime.EDGE_WINDOWS)
    if inputs == "dsaux":
        aux, N, W = True, min(N, 500), max(W, 1)        # (W >= 1: every row sees a key, the calibration needs a finite LSE)
    sa = (torch.randn(Hq, device="cuda") * 0.5) if aux else None
    cu = None
    tol_o, tol_g = (2e-2, 2e-1) if dt == torch.bfloat16 else (5e-3, 6e-2)
    desc = f"{inputs} {mode} B{B} Hq{Hq} Hkv{Hkv} N{N} D{D} ns{ns} W{W} {str(dt)[6:]} aux{int(aux)}"
    try:
        if mode == "plain":
            q, k, v, do = draw(B, Hq, Hkv, N, N, D, ns, W, dt)
            sa = calibrated(sa)
            a, b = run(q, k, v, do, ns, W, sa, False), run(q, k, v, do, ns, W, sa, True)
        elif mode == "offset":
            Nk = N + rng.choice([1, 17, 64, 100, 300])
            q, k, v, do = draw(B, Hq, Hkv, N, Nk, D, ns, W, dt)
            sa = calibrated(sa)
            a = run(q, k, v, do, ns, W, sa, False)
            qp = torch.cat([torch.zeros(B, Hq, Nk - N, D, device="cuda", dtype=dt), q], 2)
            dop = torch.cat([torch.zeros(B, Hq, Nk - N, D, device="cuda", dtype=dt), do], 2)
            b = run(qp, k, v, dop, ns, W, sa, True)
            b[0], b[1] = b[0][:, :, Nk - N:], b[1][:, :, Nk - N:]
            desc += f" Nk{Nk}"
        else:
            nseq = rng.choice([1, 2, 3, 5])
            lens = [rng.choice([0, 1, 30, 64, 65, 200, 500]) for _ in range(nseq)]
            if sum(lens) == 0:
                lens[0] = 10
            cu = [0]
            for L in lens:
                cu.append(cu[-1] + L)
            T = cu[-1]
            q, k, v, do = draw(1, Hq, Hkv, T, T, D, ns, W, dt, cu=cu)
            sa = calibrated(sa)
            qq, kk, vv = (t.clone().requires_grad_(True) for t in (q, k, v))
            ss = sa.clone().requires_grad_(True) if aux else None
            o = sink_flash_attention_varlen(qq, kk, vv, cu, ns, W, ss)
            o.backward(do)
            a = [o.detach().float(), qq.grad.float(), kk.grad.float(), vv.grad.float()] + ([ss.grad.float()] if aux else [])
            outs = [torch.zeros_like(x) for x in a]
            for s0, s1 in zip(cu[:-1], cu[1:]):
                if s1 > s0:
                    r = run(q[:, :, s0:s1], k[:, :, s0:s1], v[:, :, s0:s1], do[:, :, s0:s1], ns, W, sa, True)
                    for j in range(4):
                        outs[j][:, :, s0:s1] = r[j]
                    if aux:
                        outs[4] += r[4]
            b = outs
            desc += f" lens{lens}"
        errs = [(x - y).abs().max().item() if x.numel() else 0.0 for x, y in zip(a, b)]
        nan = any(torch.isnan(x).any().item() for x in a)
        lim = [tol_o, tol_g, tol_g, tol_g, tol_g * 20]
        ok = not nan and all(e <= l * max(1.0, y.abs().max().item() if y.numel() else 1.0) for e, l, y in zip(errs, lim, b))
        if inputs == "probe" and not nan:
            errs += sum_bound_ratios(q, k, v, do, ns, W, sa, cu if mode == "varlen" else None, a[2], a[3])
            ok = ok and max(errs[-2:]) <= 1.0
        if inputs == "dsaux" and not nan:
            ref = dsaux_inputs.reference(DSAUX["pr"], DSAUX["pr"]["classes"][DSAUX["cls"]])
            errs.append(dsaux_inputs.ratio(a[4], ref["ds"], ref["tol_ds"]))
            ok = ok and errs[-1] <= 1.0
            desc += " class " + DSAUX["cls"]
    except Exception as e:      # noqa: BLE001 - report and continue
        ok, errs = False, [repr(e)[:200]]
    if not ok:
        bad += 1
        print("BAD", desc, errs)
    elif case % 100 == 0:
        print("ok ", desc, ["%.2e" % e for e in errs])
print(f"fuzz: {n_cases} cases, {bad} bad")
