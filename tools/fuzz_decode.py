#!/usr/bin/env python3
"""Randomised cross-check of the decode paths on the GPU: plain decode vs a float64 torch reference, and ring /
fused-step / device-state / one-pass variants against the linearised cache.
usage: python tools/fuzz_decode.py [n] [seed] [--inputs=randn|probe|range] [--slots]   (range: keys carry the falling staircase of
tests/range_inputs.py along a +-1 code, one level per 64 keys, and the queries a gain of 0 / 0.5 / 1 / -1 along it; probe: keys are the +-1 codes of tests/probe_inputs.py and
every query aims, with that module's amplitude, at one key of the history: the newest, the oldest the ring still holds, the
one just evicted or the last sink; --slots: the single-token steps (decode_step_dyn only; the multi-token and commit
calls are not fuzzed here) also run through a slot pool - the B sequences sit in a random permutation of a larger pool and the
batch carries random inactive rows - and are held to the same reference)"""
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "sink-flash-attention-kernel_amd"), ROOT, os.path.join(ROOT, "tests")]
import torch

import probe_inputs
import range_inputs

from sink_attention import sink_decode_attention
from sink_attention.cache import SinkCacheLayer

inputs = ([a.split("=", 1)[1] for a in sys.argv if a.startswith("--inputs=")] or ["randn"])[-1]
assert inputs in ("randn", "probe", "range"), inputs
use_slots = "--slots" in sys.argv
sys.argv = [a for a in sys.argv if not a.startswith("--inputs=") and a != "--slots"]
n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 100
rng = random.Random(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
torch.manual_seed(rng.randrange(1 << 30))
bad = 0


def keys(B, H, n, D, dt):
    if inputs == "probe":
        return probe_inputs.codes((B, H, n, D), None, dt, device="cuda")
    if inputs == "range":
        # one code per call (seeded by D): keys appended later continue the staircase only within their own call
        u = probe_inputs.codes((1, 1, 1, D), torch.Generator().manual_seed(D), torch.float32).cuda()
        lvl = -(torch.arange(n, device="cuda") // 64).float() * range_inputs.STEPS[1] / D ** 0.5
        return (torch.randn(B, H, n, D, device="cuda") + lvl.view(1, 1, n, 1) * u).to(dt)
    return torch.randn(B, H, n, D, device="cuda", dtype=dt)


def query(B, Hq, D, dt, hist, ns, W):
    """randn, or amplitude * the code of one edge key of the history hist [B, Hkv, L, D] (the new token is its last row)"""
    if inputs == "range":
        u = probe_inputs.codes((1, 1, 1, D), torch.Generator().manual_seed(D), torch.float32).cuda()
        a = torch.tensor([rng.choice((0.0, 0.5, 1.0, -1.0)) for _ in range(Hq)], device="cuda").view(1, Hq, 1, 1)
        return (torch.randn(B, Hq, 1, D, device="cuda") + a * u).to(dt)
    if inputs != "probe":
        return torch.randn(B, Hq, 1, D, device="cuda", dtype=dt)
    L = hist.shape[2]
    t = rng.choice([x for x in (L - 1, L - W, L - W - 1, ns - 1) if 0 <= x < L])
    return (probe_inputs.amplitude(D) * hist[:, :, t:t + 1]).repeat_interleave(Hq // hist.shape[1], 1).to(dt)


def ref_decode(q, k, v, sa):
    B, Hq, _, D = q.shape
    g = Hq // k.shape[1]
    kk, vv = k.double().repeat_interleave(g, 1), v.double().repeat_interleave(g, 1)
    s = (q.double() @ kk.transpose(-1, -2)) / D ** 0.5
    if sa is not None:
        s = torch.cat([s, sa.double().view(1, Hq, 1, 1).expand(B, Hq, 1, 1)], -1)
    p = torch.softmax(s, -1)
    return (p[..., :kk.shape[2]] @ vv)


for case in range(n_cases):
    D = rng.choice([32, 64, 80, 128, 256])
    Hkv = rng.choice([1, 2, 8])
    g = rng.choice([1, 2, 4, 8, 16])
    B = rng.choice([1, 2, 5])
    dt = rng.choice([torch.bfloat16, torch.float16, torch.float32])
    ns, W = rng.choice([0, 1, 4]), rng.choice([1, 7, 64, 300])
    pre = rng.choice([1, 3, 50, 400])
    aux = rng.random() < 0.5
    Hq = Hkv * g
    sa = torch.randn(Hq, device="cuda") * 0.5 if aux else None
    tol = 1e-4 if dt == torch.float32 else (2e-2 if dt == torch.bfloat16 else 4e-3)
    desc = f"{inputs} B{B} Hq{Hq} Hkv{Hkv} D{D} ns{ns} W{W} pre{pre} {str(dt)[6:]} aux{int(aux)}"
    try:
        a, b, c = SinkCacheLayer(ns, W), SinkCacheLayer(ns, W), SinkCacheLayer(ns, W)
        c.one_pass = True
        kp, vp = keys(B, Hkv, pre, D, dt), torch.randn(B, Hkv, pre, D, device="cuda", dtype=dt)
        hist = kp
        for l in (a, b, c):
            l.update(kp, vp)
        b.enable_device_state()
        ok = True
        if use_slots and W >= 1:
            S = B + rng.randrange(4)
            where = rng.sample(range(S), B)                       # sequence i lives in slot where[i]
            rows = sorted(rng.sample(range(B + rng.randrange(3)), B)) if B > 1 else [rng.randrange(2)]
            Bx = max(rows) + 1 + rng.randrange(2)                 # batch rows, the others inactive
            slot_list = [-1] * Bx
            for i, r in enumerate(rows):
                slot_list[r] = where[i]
            d = SinkCacheLayer(ns, W)
            d.one_pass = rng.random() < 0.5
            d.init_pool(S, Hkv, D, dt, "cuda")
            d.prefill_slots(kp.transpose(0, 1).reshape(1, Hkv, B * pre, D), vp.transpose(0, 1).reshape(1, Hkv, B * pre, D),
                            [pre * i for i in range(B + 1)], where)
            slots_dev = torch.tensor(slot_list, dtype=torch.int32, device="cuda")

            def spread(t):                                        # [B, ...] -> [Bx, ...], garbage on inactive rows
                x = torch.randn(Bx, *t.shape[1:], device="cuda").to(t.dtype)
                x[rows] = t
                return x
        for step in range(rng.choice([1, 3, W + 3])):
            kn, vn = keys(B, Hkv, 1, D, dt), torch.randn(B, Hkv, 1, D, device="cuda", dtype=dt)
            hist = torch.cat([hist, kn], dim=2)
            q = query(B, Hq, D, dt, hist, ns, W)
            o1 = a.decode_step(q, kn, vn, s_aux=sa)
            o2 = b.decode_step_dyn(q, kn, vn, s_aux=sa)
            o3 = c.decode_step(q, kn, vn, s_aux=sa)
            kc, vc = a.get_kv()
            o4 = sink_decode_attention(q, kc, vc, s_aux=sa)
            r = ref_decode(q, kc, vc, sa)
            e = [(o.double() - r).abs().max().item() for o in (o1, o2, o3, o4)]
            if use_slots and W >= 1:
                o5 = d.decode_step_dyn(spread(q), spread(kn), spread(vn), s_aux=sa, slots=slots_dev)
                e.append((o5[rows].double() - r).abs().max().item())
                dead = [x for x in range(Bx) if x not in rows]
                if dead and bool(o5[dead].any()):
                    e.append(float("inf"))                       # an inactive row must be zeros
            # (the device-state step sizes its launch for the FULL cache, so while the ring is still filling its split
            # plan, hence its summation order, may differ from the host-state step: tolerance, not bitwise)
            if max(e) > tol or any(torch.isnan(o).any() for o in (o1, o2, o3, o4)):
                ok = False
                desc += f" step{step} errs{e}"
                break
        b.pull_state()
        if ok and (a.write_pos, a.window_len) != (b.write_pos, b.window_len):
            ok, desc = False, desc + " state mismatch"
        if ok and use_slots and W >= 1 and d.positions(where).tolist() != [hist.shape[2]] * B:
            ok, desc = False, desc + " slot positions mismatch"
    except Exception as ex:      # noqa: BLE001
        ok, desc = False, desc + " " + repr(ex)[:200]
    if not ok:
        bad += 1
        print("BAD", desc)
print(f"fuzz_decode: {n_cases} cases, {bad} bad")
