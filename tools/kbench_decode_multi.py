#!/usr/bin/env python3
"""Multi-token decode micro-bench (exploration tool, not the contract bench).  For n new tokens over a full, wrapped
sink + ring cache it times, alternating in one process with HIP events on torch's current stream:
  multi   SinkCacheLayer.extend_attention (sfa_decode_ring_multi: split kernel + reduce)
  step1   ONE SinkCacheLayer.decode_step on the same cache (the single-token fused ring step)
  linpre  get_kv() linearisation + the chunked-prefill kernel over [cache, chunk] (the update()-then-prefill path the
          generation patch takes today; inexact once the ring is full - timing only)
and reports K/V bytes read once (sink + ring + chunk) over the multi call time.
usage: python tools/kbench_decode_multi.py [--shape a,b] [--n 1,2,4,8,16,32] [--iters 30] [--rounds 3]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "sink-flash-attention-kernel_amd"), ROOT]
import torch

from sink_attention import SinkCacheLayer, _native
from sink_attention.sink_flash_attention import _sink_flash_attention_ex

SHAPES = {  # name: B, Hq, Hkv, D, num_sink, W, s_aux
    "a": (1, 64, 8, 64, 4, 4096, True),       # gpt-oss-120b attention geometry, W = 4096
    "b": (32, 32, 32, 128, 4, 4096, False),   # BASELINE config 5 cache policy
}


def timeit(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for s, e in evs:
        s.record()
        fn()
        e.record()
    torch.cuda.synchronize()
    ts = sorted(s.elapsed_time(e) for s, e in evs)
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="a,b")
    ap.add_argument("--n", default="1,2,4,8,16,32")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only-multi", action="store_true", help="time extend_attention alone (for a kernel trace)")
    args = ap.parse_args()
    dev, dt = "cuda", torch.bfloat16
    for name in args.shape.split(","):
        B, Hq, Hkv, D, ns, W, aux = SHAPES[name]
        torch.manual_seed(0)
        layer = SinkCacheLayer(ns, W)
        pre = ns + W
        layer.append(torch.randn(B, Hkv, pre, D, device=dev, dtype=dt), torch.randn(B, Hkv, pre, D, device=dev, dtype=dt))
        for _ in range(37):     # wrap the ring: write_pos in the middle
            layer.append(torch.randn(B, Hkv, 1, D, device=dev, dtype=dt), torch.randn(B, Hkv, 1, D, device=dev, dtype=dt))
        sa = torch.randn(Hq, device=dev) * 0.5 if aux else None
        q1 = torch.randn(B, Hq, 1, D, device=dev, dtype=dt)
        k1, v1 = torch.randn(B, Hkv, 1, D, device=dev, dtype=dt), torch.randn(B, Hkv, 1, D, device=dev, dtype=dt)
        print(f"shape {name}: B={B} H_q={Hq} H_kv={Hkv} D={D} num_sink={ns} W={W} s_aux={aux}  "
              f"(ring full, write_pos={layer.write_pos})", flush=True)
        for n in [int(x) for x in args.n.split(",")]:
            q = torch.randn(B, Hq, n, D, device=dev, dtype=dt)
            kn, vn = torch.randn(B, Hkv, n, D, device=dev, dtype=dt), torch.randn(B, Hkv, n, D, device=dev, dtype=dt)
            multi = lambda: layer.extend_attention(q, kn, vn, s_aux=sa)
            step1 = lambda: layer.decode_step(q1, k1, v1, s_aux=sa)

            def linpre():
                kl, vl = layer.get_kv()
                kc, vc = torch.cat([kl, kn], dim=2), torch.cat([vl, vn], dim=2)
                return _sink_flash_attention_ex(q, kc, vc, ns, W, s_aux=sa)

            multi()
            path = _native.last_path()
            res = {"multi": [], "step1": [], "linpre": []}
            for _ in range(args.rounds):
                res["multi"].append(timeit(multi, args.iters))
                if not args.only_multi:
                    res["step1"].append(timeit(step1, args.iters))
                    res["linpre"].append(timeit(linpre, args.iters))
            med = {k: sorted(v)[len(v) // 2] if v else float("nan") for k, v in res.items()}
            kv_bytes = 2 * B * Hkv * (layer.sink_len + layer.window_len + n) * D * 2
            print(f"  n={n:3d} rows/kv-head={Hq // Hkv * n:4d}  multi {med['multi'] * 1e3:9.1f} us  "
                  f"step1 {med['step1'] * 1e3:9.1f} us  linpre {med['linpre'] * 1e3:9.1f} us  "
                  f"multi/step1 {med['multi'] / med['step1']:5.2f}  linpre/multi {med['linpre'] / med['multi']:5.2f}  "
                  f"K/V {kv_bytes / 1e6:8.1f} MB -> {kv_bytes / med['multi'] / 1e9:6.2f} TB/s (call time)  [{path}]",
                  flush=True)


if __name__ == "__main__":
    main()
