#!/usr/bin/env python3
"""Micro-bench of ragged_step_dyn(groups=) against groups=None on the same build (exploration tool, not the contract
bench).  The geometry of DESIGN.md 3.3.12: H_kv = 8, G = 8, D = 64, bf16, num_sink = 4, a paged pool with P = 64 and
Wc = 131072; a prompt (default 10 000 and 100 000 tokens) is prefilled into one slot and shared by 8 slots
(fork_slots(share=True)), reserve_pages makes the page of the write slot each slot's own, then one decode row per slot.

The two variants alternate in one process.  Each is one step with commit=False (the state stays where it is) captured
into a graph; device time of a replay between two events, median of --rounds rounds, --runs runs.  Before the timing the
two outputs are compared (max abs difference, printed).
Bytes: what each variant has to read of the ring: `none` 8 x H_kv x window_len x D x 2 bytes x 2 (K and V), `groups`
H_kv x (Lg + 8 x (window_len - Lg)) x D x 2 x 2; TB/s = those bytes over the time.
--once: one eager step of each variant and nothing else (for a kernel trace of its own).
usage: python tools/kbench_group_step.py [--prompt 10000,100000] [--rounds 9] [--runs 2] [--once]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "sink-flash-attention-kernel_amd"), ROOT]

HKV, G, D, NS, P, WC, FORKS, ES = 8, 8, 64, 4, 64, 131072, 8, 2


def build(torch, prompt, dev):
    from sink_attention import SinkCacheLayer
    layer = SinkCacheLayer(NS, WC)
    layer.init_pool(FORKS, HKV, D, torch.bfloat16, dev, page_size=P, num_pages=-(-prompt // P) + 4 * FORKS)
    k = torch.randn(1, HKV, prompt, D, device=dev, dtype=torch.bfloat16)
    layer.reserve_pages([0], prompt)
    layer.prefill_slots(k, torch.randn_like(k), [0, prompt], [0])
    layer.fork_slots([0] * (FORKS - 1), list(range(1, FORKS)), share=True, tokens=prompt)
    layer.reserve_pages(list(range(FORKS)), prompt + 1)
    return layer


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prompt", default="10000,100000")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    import torch
    from sink_attention import _native as N
    dev = "cuda"
    for prompt in [int(x) for x in a.prompt.split(",")]:
        layer = build(torch, prompt, dev)
        wl = prompt - NS
        lg = wl // P * P
        q = torch.randn(1, HKV * G, FORKS, D, device=dev, dtype=torch.bfloat16)
        kn, vn = (torch.randn(1, HKV, FORKS, D, device=dev, dtype=torch.bfloat16) for _ in range(2))
        cu = torch.arange(FORKS + 1, dtype=torch.int32, device=dev)
        slots = torch.arange(FORKS, dtype=torch.int32, device=dev)
        cu_g = torch.tensor([0, FORKS], dtype=torch.int32, device=dev)
        outs = {v: torch.empty_like(q) for v in ("none", "groups")}

        def call(v):
            layer.ragged_step_dyn(q, kn, vn, cu, slots, out=outs[v], commit=False, groups=cu_g if v == "groups" else None)

        paths = {}
        for v in outs:
            call(v)
            paths[v] = N.last_path()
        torch.cuda.synchronize()
        diff = (outs["none"].float() - outs["groups"].float()).abs().max().item()
        print(f"prompt {prompt}: window_len {wl}, Lg {lg}; max |o_groups - o_none| = {diff:.3e}")
        print(f"  paths: {paths}")
        if a.once:
            continue
        need = {"none": FORKS * HKV * wl * D * ES * 2, "groups": HKV * (lg + FORKS * (wl - lg)) * D * ES * 2}
        graphs = {}
        for v in outs:       # each variant has a workspace of its own size: warm it, then capture
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                call(v)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            graphs[v] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[v]):
                call(v)
        for run in range(a.runs):
            times = {v: [] for v in outs}
            for _ in range(a.rounds):
                for v in outs:          # the variants alternate
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    graphs[v].replay()
                    e1.record()
                    torch.cuda.synchronize()
                    times[v].append(e0.elapsed_time(e1) * 1e3)
            med = {v: statistics.median(t) for v, t in times.items()}
            for v in outs:
                print(f"  run {run} {v:7s} {med[v]:9.1f} us (min {min(times[v]):.1f}, max {max(times[v]):.1f})  ring bytes "
                      f"{need[v] / 1e6:9.1f} MB  {need[v] / med[v] / 1e6:6.2f} TB/s")
            print(f"  run {run} none / groups = {med['none'] / med['groups']:.2f}")


if __name__ == "__main__":
    main()
