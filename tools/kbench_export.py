#!/usr/bin/env python3
"""Micro-bench of the slot export (SinkCacheLayer.export_slots, sfa_ring_export_slots and its FP8 / paged / paged FP8
forms) against the slot copy of the same slots (fork_slots(share=False), sfa_ring_copy_slots) in the same process
(exploration tool, not the contract bench).  Geometry: H_kv=8, D=128, num_sink=4, Wc=4096, bf16 activations; every source
slot holds a full ring that has wrapped (write_pos = 37).

Per pool kind (contiguous 16-bit, FP8, paged, paged FP8; pages of 64) and per n in 1, 8, 64 slots, two variants
alternating in one process:
    export  layer.export_slots(slots, cu=cu, out=(k, v, pos)): one launch; reads the live rows of n slots, writes the pack
    fork    layer.fork_slots(src, dst): one launch of the copy kernel; reads the live rows of the same n slots, writes
            them into n other slots of the pool
Each call of a round works on the next of several disjoint slot sets (and its own output pack), so that a call does not
find its rows in the Infinity Cache; 64 slots move more than it holds by themselves.
Timing: --calls calls captured into one graph, device time of a replay between two events, median of --rounds rounds;
(+-x) is half the spread between the rounds.
Bytes: read plus written.  A 16-bit pool: export and fork both read and write n x H_kv x (num_sink + Wc) x D x 2 x 2
bytes.  An FP8 pool: the fork reads and writes one byte per element, the export reads one and writes two.
usage: python tools/kbench_export.py [--n 1,8,64] [--kinds c16,fp8,paged,paged_fp8] [--rounds 7] [--calls 8] [--log PATH]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "sink-flash-attention-kernel_amd"), ROOT]

S, HKV, D, NS, W, P, WRAP = 128, 8, 128, 4, 4096, 64, 37
SRC = 64                # slots 0 .. 63 are sources, 64 .. 127 the fork's destinations
WARM = 2


def _pool(torch, kind, dev, dt):
    from sink_attention import SinkCacheLayer
    layer = SinkCacheLayer(NS, W)
    kw = dict(page_size=P) if "paged" in kind else {}
    if "fp8" in kind:
        kw["kv_dtype"] = torch.float8_e4m3fn
    layer.init_pool(S, HKV, D, dt, dev, **kw)
    if "fp8" in kind:
        layer.set_kv_scale([0.37] * HKV, [2.3] * HKV)
    if layer.page_size:
        layer.reserve_pages(list(range(S)), NS + W + WRAP)
    pre = NS + W
    for s0 in range(0, SRC, 8):
        slots = list(range(s0, s0 + 8))
        k = torch.randn(1, HKV, 8 * pre, D, device=dev, dtype=dt)
        layer.prefill_slots(k, torch.randn_like(k), [pre * i for i in range(9)], slots)
        k = torch.randn(1, HKV, 8 * WRAP, D, device=dev, dtype=dt)
        layer.commit_packed_dyn(k, torch.randn_like(k), [WRAP * i for i in range(9)], slots, [WRAP] * 8)
    assert layer._dev_state[SRC - 1].tolist() == [NS, W, WRAP, NS + W + WRAP], layer._dev_state[SRC - 1]
    return layer


def _variants(torch, layer, n, dev, dt):
    sets = max(1, min(16, SRC // n))
    rows = NS + W
    i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=dev)
    src = [i32(list(range(i * n, (i + 1) * n))) for i in range(sets)]
    dst = [i32(list(range(SRC + i * n, SRC + (i + 1) * n))) for i in range(sets)]
    cu = i32([rows * i for i in range(n + 1)])
    outs = [(torch.empty(1, HKV, n * rows, D, dtype=dt, device=dev), torch.empty(1, HKV, n * rows, D, dtype=dt, device=dev),
             torch.empty(n * rows, dtype=torch.int32, device=dev)) for _ in range(sets)]

    def export_call(i):
        layer.export_slots(src[i % sets], cu=cu, out=outs[i % sets])

    def fork_call(i):
        layer.fork_slots(src[i % sets], dst[i % sets])

    return {"export": export_call, "fork": fork_call}, sets


def _timed(torch, fn, calls):
    """-> a function that replays a graph of `calls` calls and returns the device microseconds per call"""
    def run():
        for i in range(calls):
            fn(i)

    for _ in range(WARM):
        run()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    graph.replay()
    torch.cuda.synchronize()

    def once():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        graph.replay()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / calls

    return once


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="1,8,64")
    ap.add_argument("--kinds", default="c16,fp8,paged,paged_fp8")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=8)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "export_kbench.log"))
    args = ap.parse_args()
    import torch
    from sink_attention import _native
    if not torch.cuda.is_available():
        sys.exit("kbench_export needs the GPU: there is nothing to time without one")
    dev, dt = "cuda", torch.bfloat16
    log = open(args.log, "w")

    def say(line):
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    say(f"export vs fork: H_kv={HKV} D={D} num_sink={NS} Wc={W} bf16 activations, full wrapped rings (write_pos {WRAP}), pool "
        f"of {S} slots, pages of {P}; device us per call, median of {args.rounds} rounds of {args.calls} calls (one graph "
        f"per variant), variants alternating; {torch.cuda.get_device_name(0)}; library {os.path.basename(_native.LIB_PATH)}")
    say("  pool        n  sets  export MiB   export us (+-)    TB/s    fork MiB    fork us (+-)    TB/s   export / fork")
    for kind in args.kinds.split(","):
        torch.manual_seed(0)
        layer = _pool(torch, kind, dev, dt)
        es = 1 if "fp8" in kind else 2
        for n in [int(x) for x in args.n.split(",")]:
            fns, sets = _variants(torch, layer, n, dev, dt)
            elems = n * HKV * (NS + W) * D * 2                       # K and V
            moved = {"export": elems * (es + 2), "fork": elems * 2 * es}
            once = {v: _timed(torch, f, max(args.calls, sets)) for v, f in fns.items()}
            res = {v: [] for v in fns}
            for _ in range(args.rounds):
                for v in fns:
                    res[v].append(once[v]())
            med = {v: sorted(x)[len(x) // 2] for v, x in res.items()}
            half = {v: (max(x) - min(x)) / 2 for v, x in res.items()}
            tbs = {v: moved[v] / (med[v] * 1e-6) / 1e12 for v in fns}
            say(f"  {kind:9s} {n:3d}  {sets:4d}  {moved['export'] / 2**20:10.1f}  {med['export']:9.2f} ({half['export']:6.2f})  "
                f"{tbs['export']:6.3f}  {moved['fork'] / 2**20:10.1f}  {med['fork']:9.2f} ({half['fork']:6.2f})  "
                f"{tbs['fork']:6.3f}   {med['export'] / med['fork']:8.2f}")
            del fns, once
            torch.cuda.empty_cache()
        del layer
        torch.cuda.empty_cache()
    log.close()


if __name__ == "__main__":
    main()
