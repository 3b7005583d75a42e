#!/usr/bin/env python3
"""Speculative-step micro-bench (exploration tool, not the contract bench): an L-layer verify + commit step over a full,
wrapped sink + ring cache, gpt-oss attention geometry (B=1, H_q=64, H_kv=8, D=64, s_aux, bf16).

--mode wall (default): host wall time per step of
  eager   every layer's extend_attention, the acceptance count read with .item() (one sync), every layer's append()
          of the accepted prefix (host-state path: a Python loop of 2 indexed copies per token and layer);
  graph   the same step captured once with torch.cuda.graph on device state (extend_attention_dyn, the count in torch
          ops, commit_dyn) and replayed: "graph+sync" synchronises after every replay (what a loop that reads the
          accepted tokens pays), "graph" replays back to back and synchronises once.
--mode kernels: host-state (extend_attention) and dyn (extend_attention_dyn) calls at a full ring, --calls of each after
  5 warm-up calls, for a kernel trace of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o spec -- python tools/kbench_spec_graph.py --mode kernels
--summarize OUT/.../spec_kernel_trace.csv: per configuration, the median split / reduce kernel time of each variant from
  that trace (the split kernels' template argument Dyn = false / true tells the variants apart).
usage: python tools/kbench_spec_graph.py [--mode wall|kernels] [--W 128,4096] [--n 4,8] [--layers 36] [--steps 50]"""
import argparse
import csv
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "sink-flash-attention-kernel_amd"), ROOT]

B, HQ, HKV, D, NS = 1, 64, 8, 64, 4
WARM = 5


def _layers(torch, SinkCacheLayer, W, L, dev, dt, device_state):
    layers = []
    for _ in range(L):
        layer = SinkCacheLayer(NS, W)
        pre = NS + W
        layer.append(torch.randn(B, HKV, pre, D, device=dev, dtype=dt), torch.randn(B, HKV, pre, D, device=dev, dtype=dt))
        layer.append(torch.randn(B, HKV, 37, D, device=dev, dtype=dt), torch.randn(B, HKV, 37, D, device=dev, dtype=dt))
        if device_state:
            layer.enable_device_state()
        layers.append(layer)
    return layers


def wall(args):
    import torch
    from sink_attention import SinkCacheLayer
    dev, dt = "cuda", torch.bfloat16
    print(f"gpt-oss geometry B={B} H_q={HQ} H_kv={HKV} D={D} num_sink={NS} s_aux bf16, L={args.layers} layers, ring full; "
          f"accepted a = n - 1 per step; host wall us per step, median of {args.rounds} rounds of {args.steps} steps",
          flush=True)
    for W in [int(x) for x in args.W.split(",")]:
        for n in [int(x) for x in args.n.split(",")]:
            torch.manual_seed(0)
            L = args.layers
            sa = torch.randn(HQ, device=dev) * 0.5
            qs = [torch.randn(B, HQ, n, D, device=dev, dtype=dt) for _ in range(L)]
            ks = [torch.randn(B, HKV, n, D, device=dev, dtype=dt) for _ in range(L)]
            vs = [torch.randn(B, HKV, n, D, device=dev, dtype=dt) for _ in range(L)]
            match = torch.tensor([True] * (n - 1) + [False], device=dev)
            accept = lambda: torch.cumprod(match.to(torch.int32), 0).sum()
            host = _layers(torch, SinkCacheLayer, W, L, dev, dt, False)
            dyn = _layers(torch, SinkCacheLayer, W, L, dev, dt, True)
            outs = [torch.empty(B, HQ, n, D, device=dev, dtype=dt) for _ in range(L)]

            def eager():
                for i, layer in enumerate(host):
                    outs[i] = layer.extend_attention(qs[i], ks[i], vs[i], s_aux=sa)
                a = int(accept().item())
                for i, layer in enumerate(host):
                    layer.append(ks[i][:, :, :a], vs[i][:, :, :a])

            def step():
                for i, layer in enumerate(dyn):
                    layer.extend_attention_dyn(qs[i], ks[i], vs[i], s_aux=sa, out=outs[i])
                acc = accept()
                for i, layer in enumerate(dyn):
                    layer.commit_dyn(ks[i], vs[i], acc)

            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                step()
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                step()

            def replay_sync():
                graph.replay()
                torch.cuda.synchronize()

            def timed(fn, final_sync):
                for _ in range(WARM):
                    fn()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    fn()
                if final_sync:
                    torch.cuda.synchronize()
                return (time.perf_counter() - t0) / args.steps * 1e6

            res = {"eager": [], "graph+sync": [], "graph": []}
            for _ in range(args.rounds):
                res["eager"].append(timed(eager, True))
                res["graph+sync"].append(timed(replay_sync, False))
                res["graph"].append(timed(graph.replay, True))
            med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
            print(f"  W={W:5d} n={n}  eager {med['eager']:8.1f} us  graph+sync {med['graph+sync']:8.1f} us  "
                  f"graph {med['graph']:8.1f} us  eager/graph+sync {med['eager'] / med['graph+sync']:5.2f}  "
                  f"per layer: eager {med['eager'] / L:6.1f}  graph+sync {med['graph+sync'] / L:6.1f} us", flush=True)


def kernels(args):
    import torch
    from sink_attention import SinkCacheLayer
    dev, dt = "cuda", torch.bfloat16
    for W in [int(x) for x in args.W.split(",")]:
        for n in [int(x) for x in args.n.split(",")]:
            torch.manual_seed(0)
            layer = _layers(torch, SinkCacheLayer, W, 1, dev, dt, True)[0]
            sa = torch.randn(HQ, device=dev) * 0.5
            q = torch.randn(B, HQ, n, D, device=dev, dtype=dt)
            k, v = torch.randn(B, HKV, n, D, device=dev, dtype=dt), torch.randn(B, HKV, n, D, device=dev, dtype=dt)
            for fn in (lambda: layer.extend_attention(q, k, v, s_aux=sa),
                       lambda: layer.extend_attention_dyn(q, k, v, s_aux=sa)):
                for _ in range(WARM + args.calls):
                    fn()
                torch.cuda.synchronize()
            print(f"W={W} n={n}: {WARM} + {args.calls} calls of each variant", flush=True)


def summarize(args):
    """Consecutive blocks of WARM + calls split / reduce dispatches per variant, in the order `kernels` issues them."""
    rows = list(csv.DictReader(open(args.summarize)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    per = WARM + args.calls
    series = {}
    for r in rows:
        name = r["Kernel_Name"]
        if "multi_split_mfma_kernel" in name or "multi_reduce_kernel" in name:
            kind = "split" if "split" in name else "reduce"
            dyn = "true" in name.split("<", 1)[-1] or "Lb1E" in name   # demangled or mangled
            series.setdefault((kind, dyn), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    cfgs = [(W, n) for W in [int(x) for x in args.W.split(",")] for n in [int(x) for x in args.n.split(",")]]
    med = lambda xs: sorted(xs)[len(xs) // 2]
    print("# shape   W     n   split_host_us  split_dyn_us  dyn/host   reduce_host_us  reduce_dyn_us   (median of "
          f"{args.calls} calls after {WARM} warm-up)")
    for c, (W, n) in enumerate(cfgs):
        get = lambda kind, dyn: med(series[(kind, dyn)][c * per + WARM:(c + 1) * per])
        sh, sd, rh, rd = get("split", False), get("split", True), get("reduce", False), get("reduce", True)
        print(f"  gpt-oss {W:5d} {n:3d}   {sh:12.2f}  {sd:12.2f}  {sd / sh:8.3f}   {rh:14.2f}  {rd:13.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="wall", choices=["wall", "kernels"])
    ap.add_argument("--W", default="128,4096")
    ap.add_argument("--n", default="4,8")
    ap.add_argument("--layers", type=int, default=36)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=50)
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
