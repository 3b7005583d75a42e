#!/usr/bin/env python3
"""Ragged-batch micro-bench of the per-sequence cache state (exploration tool, not the contract bench), gpt-oss attention
geometry (H_q=64, H_kv=8, D=64, num_sink=4, s_aux, bf16) at B=8.

--mode kernels: --calls extend_attention_dyn calls (after 5 warm-up calls) of each variant, per (W, n), in this order:
    shared      shared device state, full ring
    rows_full   per-sequence state, every row at a full ring (uniform)
    rows_mixed  per-sequence state, rows filled to 1/8, 2/8, ..., 8/8 of the ring (row 7 full)
  for a kernel trace of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o ragged -- python tools/kbench_ragged.py --mode kernels
--summarize OUT/.../ragged_kernel_trace.csv: median split / reduce kernel time per variant (the three variants run the
  same kernel instances, so the trace is cut into blocks in issue order).
--mode wall: an L-layer speculative step captured once per policy and replayed: extend_attention_dyn of every layer,
  per-row acceptance a_b = leading matches of a random draft pattern (each draft matches with probability --p) in torch
  ops, commit_dyn of every layer.  "rows" commits a_b per sequence; "min" is the policy a shared state forces: every
  row commits min_b a_b.  Reports the step time (replay + synchronize) and committed tokens per second.
usage: python tools/kbench_ragged.py [--mode wall|kernels] [--W 128,4096] [--n 4,8] [--layers 36] [--steps 50]"""
import argparse
import csv
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "sink-flash-attention-kernel_amd"), ROOT]

B, HQ, HKV, D, NS = 8, 64, 8, 64, 4
WARM = 5
VARIANTS = ("shared", "rows_full", "rows_mixed")


def _full_layer(torch, W, dev, dt, per_sequence):
    from sink_attention import SinkCacheLayer
    layer = SinkCacheLayer(NS, W)
    pre = NS + W + 37                          # full ring, wrapped
    layer.append(torch.randn(B, HKV, pre, D, device=dev, dtype=dt), torch.randn(B, HKV, pre, D, device=dev, dtype=dt))
    layer.enable_device_state(per_sequence=per_sequence)
    return layer


def _mixed_layer(torch, W, dev, dt):
    from sink_attention import SinkCacheLayer
    lengths = [NS + max(1, W * (b + 1) // B) for b in range(B)]
    cu = [0]
    for L in lengths:
        cu.append(cu[-1] + L)
    layer = SinkCacheLayer(NS, W)
    layer.prefill_varlen(torch.randn(1, HKV, cu[-1], D, device=dev, dtype=dt),
                         torch.randn(1, HKV, cu[-1], D, device=dev, dtype=dt), cu)
    return layer


def kernels(args):
    import torch
    dev, dt = "cuda", torch.bfloat16
    for W in [int(x) for x in args.W.split(",")]:
        for n in [int(x) for x in args.n.split(",")]:
            torch.manual_seed(0)
            layers = [_full_layer(torch, W, dev, dt, False), _full_layer(torch, W, dev, dt, True),
                      _mixed_layer(torch, W, dev, dt)]
            sa = torch.randn(HQ, device=dev) * 0.5
            q = torch.randn(B, HQ, n, D, device=dev, dtype=dt)
            k, v = torch.randn(B, HKV, n, D, device=dev, dtype=dt), torch.randn(B, HKV, n, D, device=dev, dtype=dt)
            torch.cuda.synchronize()
            for layer in layers:
                for _ in range(WARM + args.calls):
                    layer.extend_attention_dyn(q, k, v, s_aux=sa)
                torch.cuda.synchronize()
            print(f"W={W} n={n}: {WARM} + {args.calls} calls of each of {', '.join(VARIANTS)}; mixed fills "
                  f"{layers[2]._dev_state[:, 1].tolist()}", flush=True)


def summarize(args):
    rows = list(csv.DictReader(open(args.summarize)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    per = WARM + args.calls
    series = {"split": [], "reduce": []}
    for r in rows:
        name = r["Kernel_Name"]
        if "multi_split_mfma_kernel" in name or "multi_reduce_kernel" in name:
            series["split" if "split" in name else "reduce"].append(
                (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    cfgs = [(W, n) for W in [int(x) for x in args.W.split(",")] for n in [int(x) for x in args.n.split(",")]]
    med = lambda xs: sorted(xs)[len(xs) // 2]
    print(f"# B={B} gpt-oss geometry; kernel us, median of {args.calls} calls after {WARM} warm-up")
    print("#     W   n   split: shared  rows_full  rows_mixed   (rows_full - shared)   reduce: shared  rows_full  rows_mixed")
    for c, (W, n) in enumerate(cfgs):
        get = lambda kind, i: med(series[kind][(3 * c + i) * per + WARM:(3 * c + i + 1) * per])
        s = [get("split", i) for i in range(3)]
        r = [get("reduce", i) for i in range(3)]
        print(f"  {W:5d} {n:3d}   {s[0]:13.2f} {s[1]:10.2f} {s[2]:11.2f}   {s[1] - s[0]:+20.2f}   "
              f"{r[0]:14.2f} {r[1]:10.2f} {r[2]:11.2f}")


def wall(args):
    import torch
    dev, dt = "cuda", torch.bfloat16
    L = args.layers
    print(f"gpt-oss geometry B={B} H_q={HQ} H_kv={HKV} D={D} num_sink={NS} s_aux bf16, L={L} layers, ring full; each "
          f"draft matches with p={args.p}; median of {args.rounds} rounds of {args.steps} replays (+ synchronize)",
          flush=True)
    for W in [int(x) for x in args.W.split(",")]:
        for n in [int(x) for x in args.n.split(",")]:
            torch.manual_seed(0)
            g = torch.Generator().manual_seed(1)
            pats = torch.rand(args.steps, B, n, generator=g) < args.p
            acc_host = pats.int().cumprod(-1).sum(-1)                       # [steps, B]
            tokens = {"rows": int(acc_host.sum()), "min": int(acc_host.min(-1).values.sum()) * B}
            pats_dev = pats.to(dev)
            sa = torch.randn(HQ, device=dev) * 0.5
            qs = [torch.randn(B, HQ, n, D, device=dev, dtype=dt) for _ in range(L)]
            ks = [torch.randn(B, HKV, n, D, device=dev, dtype=dt) for _ in range(L)]
            vs = [torch.randn(B, HKV, n, D, device=dev, dtype=dt) for _ in range(L)]
            outs = [torch.empty(B, HQ, n, D, device=dev, dtype=dt) for _ in range(L)]
            match = torch.zeros(B, n, dtype=torch.bool, device=dev)
            graphs = {}
            for policy in ("rows", "min"):
                layers = [_full_layer(torch, W, dev, dt, policy == "rows") for _ in range(L)]

                def step(layers=layers, policy=policy):
                    for i, layer in enumerate(layers):
                        layer.extend_attention_dyn(qs[i], ks[i], vs[i], s_aux=sa, out=outs[i])
                    acc = match.int().cumprod(-1).sum(-1)
                    if policy == "min":
                        acc = acc.min()
                    for i, layer in enumerate(layers):
                        layer.commit_dyn(ks[i], vs[i], acc)

                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    step()
                torch.cuda.current_stream().wait_stream(side)
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    step()
                graphs[policy] = (graph, layers)

            def timed(graph):
                for s in range(WARM):
                    match.copy_(pats_dev[s])
                    graph.replay()
                torch.cuda.synchronize()
                t = 0.0
                for s in range(args.steps):
                    match.copy_(pats_dev[s])
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    graph.replay()
                    torch.cuda.synchronize()
                    t += time.perf_counter() - t0
                return t / args.steps * 1e6

            res = {p: [] for p in graphs}
            for _ in range(args.rounds):
                for p, (graph, _layers) in graphs.items():
                    res[p].append(timed(graph))
            med = {p: sorted(v)[len(v) // 2] for p, v in res.items()}
            tps = {p: tokens[p] / (med[p] * 1e-6 * args.steps) for p in graphs}
            print(f"  W={W:5d} n={n}  step: rows {med['rows']:8.1f} us  min {med['min']:8.1f} us   committed tokens/step: "
                  f"rows {tokens['rows'] / args.steps:5.2f}  min {tokens['min'] / args.steps:5.2f}   tokens/s: "
                  f"rows {tps['rows']:9.0f}  min {tps['min']:9.0f}  rows/min {tps['rows'] / tps['min']:5.2f}", flush=True)
            del graphs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="wall", choices=["wall", "kernels"])
    ap.add_argument("--W", default="128,4096")
    ap.add_argument("--n", default="4,8")
    ap.add_argument("--layers", type=int, default=36)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--p", type=float, default=0.7)
    ap.add_argument("--summarize", default=None, help="kernel_trace.csv of a --mode kernels run")
    args = ap.parse_args()
    if args.summarize:
        summarize(args)
    elif args.mode == "kernels":
        kernels(args)
    else:
        wall(args)


if __name__ == "__main__":
    main()
