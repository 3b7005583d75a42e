#!/usr/bin/env python3
"""Randomised cross-check of the decode paths on the GPU: plain decode vs a float64 torch reference, and ring /
fused-step / device-state / one-pass variants against the linearised cache.
usage: python tools/fuzz_decode.py [n] [seed] [--inputs=randn|probe|range] [--slots] [--call=packed [--page-size=P]] [--call=edge]   (range: keys carry the falling staircase of
tests/range_inputs.py along a +-1 code, one level per 64 keys, and the queries a gain of 0 / 0.5 / 1 / -1 along it; probe: keys are the +-1 codes of tests/probe_inputs.py and
every query aims, with that module's amplitude, at one key of the history: the newest, the oldest the ring still holds, the
one just evicted or the last sink; --slots: the single-token steps (decode_step_dyn only; the multi-token and commit
calls are not fuzzed here) also run through a slot pool - the B sequences sit in a random permutation of a larger pool and the
batch carries random inactive rows - and are held to the same reference; --call=packed: random packed serving steps
instead - ragged_step_dyn over a slot pool with Wc up to 4096, random H_kv, G, T_PAD, fills and chunk lengths, in the plain,
tree (parent=), admitting and FP8-pool forms - against an fp64 masked attention over each sequence's history, computed on
the GPU; --page-size=P with it: half of the 16-bit cases whose Wc is a multiple of P run on a paged pool of NaN-filled pages
behind a shuffled table, reserved slot by slot through the host allocator's prefix rule; --call=edge (with --inputs=probe):
the single-token step on the decode probes of tests/probe_inputs.py::decode_probe - every (batch, q head) aims at one edge key
of what the step may read, with half of the softmax mass on it - at a ring capacity up to 16384, random per-row fill states, in
the host-state, shared-state and per-sequence forms, one_pass either way, against probe_inputs.decode_oracle at DECODE_TOL;
the launch is checked against tests/decode_regime.py and the cache buffers against the CPU twin)"""
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
call = ([a.split("=", 1)[1] for a in sys.argv if a.startswith("--call=")] or ["step"])[-1]
assert call in ("step", "packed", "edge"), call
assert call != "edge" or inputs == "probe", "--call=edge takes --inputs=probe"
page_size = int(([a.split("=", 1)[1] for a in sys.argv if a.startswith("--page-size=")] or ["0"])[-1])
sys.argv = [a for a in sys.argv if not a.startswith(("--inputs=", "--call=", "--page-size=")) and a != "--slots"]
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


def packed_case():
    """one random packed step; returns (description, largest error / tolerance over the live rows, or inf)"""
    from fp8_ref import FP8, dequant, quant
    D = rng.choice([64, 80, 96, 128, 48])
    dt = torch.float32 if D == 48 else rng.choice([torch.bfloat16, torch.float16])
    Hkv, g = rng.choice([1, 2, 8]), rng.choice([1, 4, 8])
    Hq, ns = Hkv * g, 4
    W = rng.choice([48, 320, 1024, 2048, 4096])
    T = rng.choice([64, 320, 1024])
    form = rng.choice(["plain", "tree", "admit", "fp8"] if dt != torch.float32 else ["plain", "tree", "admit"])
    n_seq = rng.randrange(2, 7)
    lengths, left = [], T
    for _ in range(n_seq):
        n = min(rng.choice([0, 1, 1, 3, 8, 33, 64, 70, 160, 300]), left - 8 if left > 8 else 0)
        lengths.append(n)
        left -= n
    S = n_seq + 2
    slots = rng.sample(range(S), n_seq)
    if rng.random() < 0.3:
        slots[rng.randrange(n_seq)] = -1
    fresh = [form == "admit" and rng.random() < 0.5 for _ in range(n_seq)]
    hist = [0 if fresh[i] else rng.choice([1, 3, 9, 100, ns + W - 1, ns + W, ns + W + rng.randrange(1, 2 * W)]) for i in range(n_seq)]
    aux = rng.random() < 0.5
    sa = torch.randn(Hq, device="cuda") * 0.8 if aux else None
    # tests/util.py::DECODE_TOL for the 16-bit types; fp32: this tool's own 1e-4 (probe and range rows put a logit of 14 - 30
    # nat on one key among thousands: the f32 rounding of that dot product alone moves p by 1e-5 relative)
    tol = {torch.float32: 1e-4, torch.float16: 2e-3, torch.bfloat16: 1.6e-2}[dt]
    desc = f"packed {inputs} {form} Hkv{Hkv} G{g} D{D} Wc{W} T{T} lengths{lengths} hist{hist} slots{slots} {str(dt)[6:]} aux{int(aux)}"
    layer = SinkCacheLayer(ns, W)
    paged = bool(page_size) and form != "fp8" and dt != torch.float32 and W % page_size == 0 and rng.random() < 0.5
    if paged:
        # pages in a shuffled order, NaN until stored; every slot gets the prefix its history plus this step can reach
        desc += f" paged P{page_size}"
        layer.init_pool(S, Hkv, D, dt, "cuda", page_size=page_size)
        layer.window_k.fill_(float("nan")), layer.window_v.fill_(float("nan"))
        rng.shuffle(layer._pages.free_list)
        live_s = [(s, hist[i] + lengths[i]) for i, s in enumerate(slots) if s >= 0]
        layer.reserve_pages([s for s, _ in live_s], [t for _, t in live_s])
    else:
        layer.init_pool(S, Hkv, D, FP8 if form == "fp8" else dt, "cuda")
    sc = None
    if form == "fp8":
        sc = ([rng.choice([0.37, 1.0, 2.0]) for _ in range(Hkv)], [rng.choice([0.25, 1.0]) for _ in range(Hkv)])
        layer.set_kv_scale(*sc)
    cu = [0]
    for n in lengths:
        cu.append(cu[-1] + n)
    def keys_p(n):
        """keys of one history: as keys(), but the range staircase is a sawtooth of 12 levels (a history of 12000 keys would
        otherwise climb to 1600 nat, beyond what an f32 dot product resolves) and fp32 takes range_inputs.FP32_SCALE"""
        if inputs != "range":
            return keys(1, Hkv, n, D, dt)
        u = probe_inputs.codes((1, 1, 1, D), torch.Generator().manual_seed(D), torch.float32).cuda()
        lvl = -((torch.arange(n, device="cuda") // 64) % 12).float() * range_inputs.STEPS[1] / D ** 0.5
        lvl = lvl * (range_inputs.FP32_SCALE if dt == torch.float32 else 1.0)
        return (torch.randn(1, Hkv, n, D, device="cuda") + lvl.view(1, 1, n, 1) * u).to(dt)

    q = torch.randn(1, Hq, T, D, device="cuda").to(dt)
    k, v = keys_p(T), torch.randn(1, Hkv, T, D, device="cuda").to(dt)
    full = {}
    for i, (n, L) in enumerate(zip(lengths, hist)):
        if slots[i] < 0 or n == 0:
            continue
        if inputs == "probe":
            pr = probe_inputs.chunk_probe(1, Hq, Hkv, D, ns, W, L, n, dt, seed=rng.randrange(1 << 30), aux=False)
            fk, fv = pr["k"].cuda(), pr["v"].cuda()
            q[:, :, cu[i]:cu[i] + n] = pr["q"][:, :, L:].cuda()
        else:
            fk, fv = keys_p(L + n), torch.randn(1, Hkv, L + n, D, device="cuda").to(dt)
            if inputs == "range":
                u = probe_inputs.codes((1, 1, 1, D), torch.Generator().manual_seed(D), torch.float32).cuda()
                a = torch.tensor([rng.choice((0.0, 0.5, 1.0, -1.0)) for _ in range(Hq)], device="cuda").view(1, Hq, 1, 1)
                q[:, :, cu[i]:cu[i] + n] = (torch.randn(1, Hq, n, D, device="cuda") + a * u).to(dt)
        k[:, :, cu[i]:cu[i] + n], v[:, :, cu[i]:cu[i] + n] = fk[:, :, L:], fv[:, :, L:]
        full[i] = (fk, fv)
    cont = [i for i in full if hist[i] > 0]
    if cont:
        fill = [min(hist[i], ns + W) for i in cont]
        cat = lambda x, lo, hi: torch.cat([full[i][x][:, :, lo(j):hi(j)] for j, i in enumerate(cont)], dim=2)
        cum = lambda xs: [sum(xs[:j]) for j in range(len(xs) + 1)]
        layer.prefill_slots(cat(0, lambda j: 0, lambda j: fill[j]), cat(1, lambda j: 0, lambda j: fill[j]), cum(fill), [slots[i] for i in cont])
        extra = [hist[i] - f for i, f in zip(cont, fill)]
        if any(extra):
            layer.commit_packed_dyn(cat(0, lambda j: fill[j], lambda j: hist[cont[j]]), cat(1, lambda j: fill[j], lambda j: hist[cont[j]]),
                                    cum(extra), [slots[i] for i in cont], extra)
    parent = None
    trees = {}
    if form == "tree" or (form == "fp8" and rng.random() < 0.5):
        parent = [-1] * T
        for i, n in enumerate(lengths):
            trees[i] = [rng.randrange(-1, u) if rng.random() < 0.7 else u - 1 for u in range(n)]
            parent[cu[i]:cu[i] + n] = trees[i]
    o = layer.ragged_step_dyn(q, k, v, cu, slots, s_aux=sa, commit=rng.random() < 0.5, admit=form == "admit", parent=parent)
    worst = 0.0
    live = torch.zeros(T, dtype=torch.bool, device="cuda")
    for i, (fk, fv) in full.items():
        n, L = lengths[i], hist[i]
        sl = min(n, ns) if fresh[i] else min(L, ns)
        par = trees[i] if (i in trees and n <= 64) else list(range(-1, n - 1))
        depth, anc = [], torch.zeros(n, n, dtype=torch.bool)
        for u in range(n):
            depth.append(0 if par[u] < 0 else depth[par[u]] + 1)
            anc[u, u] = True
            if par[u] >= 0:
                anc[u] |= anc[par[u]]
        d = torch.tensor(depth, device="cuda").view(n, 1)
        j = torch.arange(L + n, device="cuda").view(1, L + n)
        mask = (j < sl) | ((j >= L + d - W + 1) & (j < L))
        dd = torch.tensor(depth, device="cuda")
        chunk = anc.cuda() & ((d - dd.view(1, n) <= W - 1) | (torch.arange(n, device="cuda").view(1, n) < (sl if fresh[i] else 0)))
        mask = torch.cat([mask[:, :L], chunk], dim=1) if L else chunk
        if sc is not None and L:
            fk = torch.cat([dequant(quant(fk[:, :, :L].cpu(), sc[0]), sc[0], dt).cuda(), fk[:, :, L:]], dim=2)
            fv = torch.cat([dequant(quant(fv[:, :, :L].cpu(), sc[1]), sc[1], dt).cuda(), fv[:, :, L:]], dim=2)
        s = (q[:, :, cu[i]:cu[i] + n].double() @ fk.double().repeat_interleave(g, 1).transpose(-1, -2)) / D ** 0.5
        s = s.masked_fill(~mask, float("-inf"))
        if sa is not None:
            s = torch.cat([s, sa.double().view(1, Hq, 1, 1).expand(1, Hq, n, 1)], -1)
        r = torch.softmax(s, -1)[..., :L + n] @ fv.double().repeat_interleave(g, 1)
        e = (o[:, :, cu[i]:cu[i] + n].double() - r).abs().max().item()
        worst = max(worst, e / tol if e == e else float("inf"))
        live[cu[i]:cu[i] + n] = True
    if bool(o[:, :, ~live].any()):
        worst = float("inf")                                      # inactive, empty and padded rows must be zeros
    return desc, worst


def edge_case():
    """one random fused step on the decode probes; returns (description, error / tolerance or inf)"""
    import decode_regime as R
    from sink_attention import _native
    from util import DECODE_TOL
    D, dname = rng.choice([(16, "fp16"), (64, "bf16"), (64, "fp32"), (80, "bf16"), (80, "fp32"), (128, "fp16"), (256, "bf16")])
    Hkv, g = rng.choice([1, 2, 4]), rng.choice([1, 3, 4, 6, 8, 12, 16])
    ns, Wc = rng.choice([1, 4]), rng.choice([300, 1020, 2400, 5000, 16381, 16384])
    form = rng.choice(["host", "dyn", "rows"])
    B = rng.choice([1, 2, 5])
    full = lambda: (ns, Wc, rng.randrange(Wc))
    part = lambda: (lambda wl: (rng.randrange(1, ns + 1) if wl == 0 else ns, wl, wl))(rng.choice([0, 1, 251, 252, 253, Wc // 2, Wc - 1]))
    states = [rng.choice([full, part])() for _ in range(B)] if form == "rows" else [rng.choice([full, part])()] * B
    case = dict(id="fuzz", dtype=dname, B=B, Hq=Hkv * g, Hkv=Hkv, D=D, ns=ns, Wc=Wc)
    one_pass = rng.random() < 0.5
    desc = f"edge {form} 1pass{int(one_pass)} B{B} Hkv{Hkv} G{g} D{D} ns{ns} Wc{Wc} {dname} states{states}"
    run = probe_inputs.DecodeRun(case, states, form != "host", rng.randrange(1 << 30), rng.randrange(64))
    layer = SinkCacheLayer(ns, Wc)
    for name in ("sink_k", "sink_v", "window_k", "window_v"):
        setattr(layer, name, run.cache[name].cuda())
    layer.is_initialized = layer.prefilled = True
    layer.one_pass = one_pass
    if form == "rows":
        layer._dev_state = torch.tensor([[sl, wl, wp, sl + wl] for sl, wl, wp in states], dtype=torch.int32, device="cuda")
        layer._per_seq = True
    else:
        layer.sink_len, layer.window_len, layer.write_pos = states[0]
        if form == "dyn":
            layer.enable_device_state()
    worst = 0.0
    for step in range(rng.choice([1, 3])):
        L = run.probe()
        pr = L["pr"]
        q, kn, vn, sa = (pr[x].cuda() for x in ("q", "k_new", "v_new", "s_aux"))
        o = layer.decode_step(q, kn, vn, s_aux=sa) if form == "host" else layer.decode_step_dyn(q, kn, vn, s_aux=sa)
        path = _native.last_path()
        e = (o.double().cpu() - L["ref"]).abs().max().item() / DECODE_TOL[q.dtype]
        worst = max(worst, e if e == e else float("inf"))
        run.apply(pr)
        same = all(torch.equal(getattr(layer, n).cpu(), run.cache[n]) for n in ("sink_k", "sink_v", "window_k", "window_v"))
        if not path.endswith("_" + L["pl"]["suffix"]) or ("1pass" in path) != one_pass or not same:
            return desc + f" step{step} path {path} plan {L['pl']['suffix']} buffers equal {same}", float("inf")
    return desc, worst


if call == "edge":
    top = 0.0
    for case in range(n_cases):
        try:
            desc, worst = edge_case()
        except Exception as ex:      # noqa: BLE001
            desc, worst = "edge " + repr(ex)[:300], float("inf")
        top = max(top, worst if worst != float("inf") else 0.0)
        if worst > 1.0:
            bad += 1
            print("BAD", desc, "error / tol", worst)
    print(f"fuzz_decode --call=edge --inputs=probe: {n_cases} cases, {bad} bad, largest error / tol {top:.3f}")
    sys.exit(1 if bad else 0)

if call == "packed":
    top = 0.0
    for case in range(n_cases):
        try:
            desc, worst = packed_case()
        except Exception as ex:      # noqa: BLE001
            desc, worst = "packed " + repr(ex)[:300], float("inf")
        top = max(top, worst if worst != float("inf") else 0.0)
        if worst > 1.0:
            bad += 1
            print("BAD", desc, "error / tol", worst)
    print(f"fuzz_decode --call=packed --inputs={inputs}: {n_cases} cases, {bad} bad, largest error / tol {top:.3f}")
    sys.exit(1 if bad else 0)

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
