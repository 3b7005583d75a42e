#!/usr/bin/env python3
"""Tree-verify micro-bench (exploration tool, not the contract bench), gpt-oss attention geometry (H_q=64, H_kv=8, D=64,
num_sink=4, s_aux, bf16) over a full, wrapped ring.

--mode kernels: per (B, W), --calls calls (after 5 warm-up calls) of each variant, timed in-process with events (mean
  us per call, split + reduce launches):
    chain n         extend_attention_tree with parent = [-1, 0, ..., n - 2] against extend_attention (n = 4 / 8 / 16)
    tree N          one extend_attention_tree of an EAGLE-like tree of N = 16 / 32 / 60 nodes against one
                    extend_attention per root-to-leaf path (the only way to verify the tree without tree masks)
  for kernel times, the same run under a trace of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o tree -- python tools/kbench_tree.py --mode kernels
  (the split kernels' last template argument Tree = false / true tells multi from tree instances).
--mode step: an L-layer speculative step captured once per policy and replayed, B rows per-sequence: "tree" =
  extend_attention_tree_dyn + greedy_accept + commit_path_dyn of a 16-node tree, "chain" = extend_attention_dyn +
  leading matches + commit_dyn of a 4-token chain (tools/kbench_spec_graph.py's step).  Acceptance model: each draft
  token matches the target with probability --p, independently per node.  Reports us per step and tokens committed
  per step (accepted drafts, without the bonus token).
usage: python tools/kbench_tree.py [--mode kernels|step] [--B 1,8] [--W 128,4096] [--layers 36] [--steps 50]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "sink-flash-attention-kernel_amd"), ROOT]

HQ, HKV, D, NS = 64, 8, 64, 4
WARM = 5


def eagle_tree(N):
    """A top-k style draft tree: root 0, then levels of widths 4, 3, 2, 1, ... each child of the best (lowest) nodes
    of the level above, until N nodes."""
    parent, level = [-1], [0]
    widths = [4, 4, 3, 3, 2, 2, 2, 1]
    w = 0
    while len(parent) < N:
        nxt = []
        for i, p in enumerate(level):
            for _ in range(max(1, widths[min(w, len(widths) - 1)] - i)):
                if len(parent) < N:
                    nxt.append(len(parent))
                    parent.append(p)
        level, w = nxt, w + 1
    return parent


def leaf_paths(parent):
    kids = set(p for p in parent if p >= 0)
    paths = []
    for u in range(len(parent)):
        if u not in kids:
            p = [u]
            while parent[p[-1]] >= 0:
                p.append(parent[p[-1]])
            paths.append(p[::-1])
    return paths


def _layer(torch, W, B, dev, dt, dyn=None):
    from sink_attention import SinkCacheLayer
    layer = SinkCacheLayer(NS, W)
    layer.append(torch.randn(B, HKV, NS + W + 37, D, device=dev, dtype=dt),
                 torch.randn(B, HKV, NS + W + 37, D, device=dev, dtype=dt))
    if dyn is not None:
        layer.enable_device_state(per_sequence=dyn)
    return layer


def _time(torch, fn, calls):
    for _ in range(WARM):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / calls


def kernels(args):
    import torch
    dev, dt = "cuda", torch.bfloat16
    print(f"gpt-oss geometry H_q={HQ} H_kv={HKV} D={D} num_sink={NS} s_aux bf16, full wrapped ring; us per call "
          f"(split + reduce), mean of {args.calls} calls", flush=True)
    for B in [int(x) for x in args.B.split(",")]:
        for W in [int(x) for x in args.W.split(",")]:
            torch.manual_seed(0)
            layer = _layer(torch, W, B, dev, dt)
            sa = torch.randn(HQ, device=dev) * 0.5
            for n in (4, 8, 16):
                q = torch.randn(B, HQ, n, D, device=dev, dtype=dt)
                k, v = (torch.randn(B, HKV, n, D, device=dev, dtype=dt) for _ in range(2))
                chain = torch.tensor([-1] + list(range(n - 1)), device=dev, dtype=torch.int32)
                tm = _time(torch, lambda: layer.extend_attention(q, k, v, s_aux=sa), args.calls)
                tt = _time(torch, lambda: layer.extend_attention_tree(q, k, v, chain, s_aux=sa), args.calls)
                print(f"B={B} W={W} chain n={n:2d}: multi {tm:7.2f} us  tree {tt:7.2f} us  ({tt - tm:+.2f} us, "
                      f"{100 * (tt / tm - 1):+.1f} %)", flush=True)
            for N in (16, 32, 60):
                parent = eagle_tree(N)
                paths = leaf_paths(parent)
                q = torch.randn(B, HQ, N, D, device=dev, dtype=dt)
                k, v = (torch.randn(B, HKV, N, D, device=dev, dtype=dt) for _ in range(2))
                par = torch.tensor(parent, device=dev, dtype=torch.int32)
                idx = [torch.tensor(p, device=dev) for p in paths]
                sub = [(q[:, :, i].contiguous(), k[:, :, i].contiguous(), v[:, :, i].contiguous()) for i in idx]
                tt = _time(torch, lambda: layer.extend_attention_tree(q, k, v, par, s_aux=sa), args.calls)

                def per_path():
                    for qq, kk, vv in sub:
                        layer.extend_attention(qq, kk, vv, s_aux=sa)
                tp = _time(torch, per_path, args.calls)
                depth = max(len(p) for p in paths)
                print(f"B={B} W={W} tree N={N:2d} ({len(paths)} leaves, depth {depth}): one tree call {tt:7.2f} us, "
                      f"one extend_attention per leaf path {tp:8.2f} us  ratio {tp / tt:5.2f}x", flush=True)


def step(args):
    import torch
    from sink_attention import greedy_accept
    dev, dt = "cuda", torch.bfloat16
    L, p = args.layers, args.p
    print(f"gpt-oss geometry, L={L} layers, per-sequence state, full wrapped ring, acceptance p={p} per node; "
          f"captured step replayed {args.steps} times", flush=True)
    for B in [int(x) for x in args.B.split(",")]:
        for W in [int(x) for x in args.W.split(",")]:
            for policy, n in (("chain", 4), ("tree", 16)):
                torch.manual_seed(0)
                layers = [_layer(torch, W, B, dev, dt, dyn=True) for _ in range(L)]
                sa = torch.randn(HQ, device=dev) * 0.5
                qs = [torch.randn(B, HQ, n, D, device=dev, dtype=dt) for _ in range(L)]
                ks = [torch.randn(B, HKV, n, D, device=dev, dtype=dt) for _ in range(L)]
                vs = [torch.randn(B, HKV, n, D, device=dev, dtype=dt) for _ in range(L)]
                outs = [torch.empty_like(x) for x in qs]
                parent = torch.tensor(eagle_tree(n) if policy == "tree" else [-1] + list(range(n - 1)), device=dev)
                draft = torch.zeros(B, n, dtype=torch.long, device=dev)
                target = torch.zeros(B, n, dtype=torch.long, device=dev)
                total = torch.zeros((), dtype=torch.long, device=dev)

                def one():
                    if policy == "tree":
                        for i, ly in enumerate(layers):
                            ly.extend_attention_tree_dyn(qs[i], ks[i], vs[i], parent, s_aux=sa, out=outs[i])
                        path, count = greedy_accept(parent, draft, target)
                        for i, ly in enumerate(layers):
                            ly.commit_path_dyn(ks[i], vs[i], path, count)
                    else:
                        for i, ly in enumerate(layers):
                            ly.extend_attention_dyn(qs[i], ks[i], vs[i], s_aux=sa, out=outs[i])
                        count = (draft[:, 1:] == target[:, :-1]).int().cumprod(-1).sum(-1) + 1
                        for i, ly in enumerate(layers):
                            ly.commit_dyn(ks[i], vs[i], count)
                    total.add_((count - 1).sum())

                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    one()
                torch.cuda.current_stream().wait_stream(side)
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    one()
                torch.cuda.synchronize()
                total.zero_()
                g = torch.Generator().manual_seed(1)
                pc = parent.cpu().clamp(min=0)
                dts = []
                for _ in range(args.steps):
                    tg = torch.randint(0, 1000, (B, n), generator=g)
                    # node u matches with probability p: its draft = the target after its parent (chain: the previous)
                    hit = torch.rand(B, n, generator=g) < p
                    dr = torch.where(hit, tg.gather(1, pc.expand(B, n)), torch.full((B, n), -1))
                    target.copy_(tg)
                    draft.copy_(dr)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    graph.replay()
                    torch.cuda.synchronize()
                    dts.append(time.perf_counter() - t0)
                dts.sort()
                med = dts[len(dts) // 2] * 1e6
                tok = float(total.item()) / args.steps
                print(f"B={B} W={W} {policy:5s} n={n:2d}: {med:8.1f} us/step, {tok:6.2f} drafts committed/step over the "
                      f"batch, {tok / med * 1e6:9.0f} drafts/s", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="kernels", choices=("kernels", "step"))
    ap.add_argument("--B", default="1,8")
    ap.add_argument("--W", default="128,4096")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--layers", type=int, default=36)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--p", type=float, default=0.6)
    args = ap.parse_args()
    kernels(args) if args.mode == "kernels" else step(args)


if __name__ == "__main__":
    main()
