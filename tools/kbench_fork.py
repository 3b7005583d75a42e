#!/usr/bin/env python3
"""Micro-bench of the slot copy (SinkCacheLayer.fork_slots, sfa_ring_copy_slots) against what could be written before
it with device indices (exploration tool, not the contract bench).  gpt-oss K/V geometry: H_kv=8, D=64, bf16,
num_sink=4, a pool of 64 slots.

Per (W, fill, fork), two variants alternating in one process:
    fork    layer.fork_slots(src, dst): one launch, the live rows once
    index   buf.index_copy_(0, dst, buf.index_select(0, src)) on the four buffers and the state: ten launches, the whole
            capacity of every named slot twice
fill:  quarter  every source holds num_sink + W / 4 tokens (a quarter of the ring, not wrapped)
       full     every source holds a full ring that has wrapped (write_pos != 0)
fork:  1to7     one source into 7 destinations (a sampling group of 8)
       8pairs   8 disjoint (source, destination) pairs
Each call of a round works on the next of --sets disjoint slot sets of the pool, so that at W = 4096 a round touches
more than the 256 MiB Infinity Cache holds and a call does not find its rows on chip; at W = 128 the whole pool (17
MiB) stays there whatever is done.
Timing: --calls calls captured into one graph (no host time between the launches), device time of a replay between two
events, median of --rounds rounds; (+-x) is half the spread between the rounds.  --eager times the calls as issued
instead (at W = 128 that measures the host path of a call, not the kernels).
Bytes: `live` = pairs x H_kv x (sink_len + window_len) x D x 2 bytes x 2 (K and V), the bytes a copy has to read and to
write.  TB/s = bytes each variant actually moves over its time: fork reads and writes `live` (2 x live; the 7
destinations of 1to7 read the same source rows, counted 7 times), index reads and writes the capacity of the named slots
twice (4 x capacity, with capacity = pairs x H_kv x (num_sink + W) x D x 2 x 2).
--share: another measurement - on a PAGED pool, fork_slots(share=True) against the copying fork: fork time, bytes of
pages mapped, and the first reserve_pages + decode step after the fork (share_bench below).
usage: python tools/kbench_fork.py [--W 128,4096] [--rounds 7] [--calls 16] [--sets 4] [--eager]
       python tools/kbench_fork.py --share [--W 131072] [--page 64] [--prompt 100000] [--rounds 7]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "sink-flash-attention-kernel_amd"), ROOT]

S, HKV, D, NS, ES = 64, 8, 64, 4, 2
WARM = 3
FILLS = ("quarter", "full")
FORKS = ("1to7", "8pairs")


def _pool(torch, W, fill, dev, dt):
    """a pool whose every slot holds the same fill (so that any slot can be a source)"""
    from sink_attention import SinkCacheLayer
    layer = SinkCacheLayer(NS, W)
    layer.init_pool(S, HKV, D, dt, dev)
    pre = NS + W // 4 if fill == "quarter" else NS + W + 37
    for s0 in range(0, S, 8):
        k = torch.randn(1, HKV, 8 * pre, D, device=dev, dtype=dt)
        layer.prefill_slots(k, torch.randn_like(k), [pre * i for i in range(9)], list(range(s0, s0 + 8)))
    if fill == "full":          # wrap further: write_pos != 0
        idx = torch.arange(S, dtype=torch.int32, device=dev)
        for s0 in range(0, S, 8):
            k = torch.randn(8, HKV, 37, D, device=dev, dtype=dt)
            layer.commit_dyn(k, torch.randn_like(k), torch.full((8,), 37, dtype=torch.int32, device=dev),
                             slots=idx[s0:s0 + 8])
    st = layer._dev_state[0].tolist()
    assert st[:2] == ([NS, W // 4] if fill == "quarter" else [NS, W]) and (fill == "quarter" or st[2] != 0), st
    return layer, st[0] + st[1]


def slot_sets(fork, sets):
    """`sets` disjoint (src, dst) lists over the 64 slots: 1to7 uses 8 slots per set, 8pairs 16"""
    per = 8 if fork == "1to7" else 16
    assert sets * per <= S, f"--sets {sets}: {fork} needs {per} slots per set of a pool of {S}"
    out = []
    for i in range(sets):
        base = list(range(i * per, (i + 1) * per))
        out.append(([base[0]] * 7, base[1:]) if fork == "1to7" else (base[:8], base[8:]))
    return out


def _variants(torch, layer, fork, sets, dev):
    pairs = [(torch.tensor(s, dtype=torch.int32, device=dev), torch.tensor(d, dtype=torch.int32, device=dev))
             for s, d in slot_sets(fork, sets)]
    pairs64 = [(s.long(), d.long()) for s, d in pairs]
    bufs = [layer.sink_k, layer.sink_v, layer.window_k, layer.window_v, layer._dev_state]

    def fork_call(i):
        layer.fork_slots(*pairs[i % sets])

    def index_call(i):
        src, dst = pairs64[i % sets]
        for b in bufs:
            b.index_copy_(0, dst, b.index_select(0, src))

    return {"fork": fork_call, "index": index_call}, len(pairs[0][0])


def _timed(torch, fn, calls, eager):
    """-> a function that runs `calls` calls and returns the device microseconds per call"""
    def run():
        for i in range(calls):
            fn(i)

    for _ in range(WARM):
        run()
    torch.cuda.synchronize()
    if eager:
        replay = run
    else:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            run()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            run()
        replay = graph.replay
        replay()
        torch.cuda.synchronize()

    def once():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        replay()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / calls

    return once


def share_bench(torch, args, dev, dt):
    """--share: a paged pool (P = --page, Wc = the first --W), one prompt of --prompt tokens forked into 7 slots, once by
    the copying fork (reserve_pages of the destinations + fork_slots) and once by fork_slots(share=True), alternating;
    then the first reserve_pages of the 8 slots (the copy-on-write pages of the shared fork) plus one committing decode
    step of the 8.  Host clock around work that ends in a device synchronise (a shared fork is host bookkeeping plus one
    launch and cannot be captured); median of --rounds rounds after two warm-up rounds, (+-x) half the spread."""
    import time
    from sink_attention import SinkCacheLayer
    W, P, prompt, G = int(args.W.split(",")[0]), args.page, args.prompt, 8
    per = W // P
    need = -(-min(prompt + 8, W) // P)
    layer = SinkCacheLayer(NS, W)
    layer.init_pool(8, HKV, D, dt, dev, page_size=P, num_pages=8 * need + 8)
    torch.manual_seed(0)
    k = torch.randn(1, HKV, prompt, D, device=dev, dtype=dt)
    layer.reserve_pages([0], prompt)
    layer.prefill_slots(k, torch.randn_like(k), [0, prompt], [0])
    al, dst, seen = layer._pages, list(range(1, 8)), prompt
    q = torch.randn(1, HKV * G, 8, D, device=dev, dtype=dt)
    kn, vn = torch.randn(1, HKV, 8, D, device=dev, dtype=dt), torch.randn(1, HKV, 8, D, device=dev, dtype=dt)
    cu, slots = list(range(9)), list(range(8))
    page_bytes = 2 * HKV * P * D * ES

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6

    def copy_fork():
        layer.reserve_pages(dst, seen)
        layer.fork_slots([0] * 7, dst)

    def share_fork():
        layer.fork_slots([0] * 7, dst, share=True, tokens=seen)

    def first_step():
        layer.reserve_pages(slots, seen + 1)
        layer.ragged_step_dyn(q, kn, vn, cu, slots)

    res = {v: {"fork": [], "step": [], "bytes": [], "cow": []} for v in ("copy", "share")}
    for r in range(args.rounds + 2):
        for v, fork in (("copy", copy_fork), ("share", share_fork)):
            t_fork = clock(fork)
            mapped = al.pool_bytes(HKV, D, ES)
            free = len(al.free_list)
            t_step = clock(first_step)
            seen += 1
            if r >= 2:
                res[v]["fork"].append(t_fork), res[v]["step"].append(t_step), res[v]["bytes"].append(mapped)
                res[v]["cow"].append(free - len(al.free_list))
            layer.release_slots(dst)
            layer.free_pages(dst)
    med = lambda x: sorted(x)[len(x) // 2]
    half = lambda x: (max(x) - min(x)) / 2
    print(f"shared fork vs copying fork: H_kv={HKV} D={D} P={P} Wc={W} bf16, a prompt of {prompt} tokens ({need} pages of "
          f"{page_bytes // 1024} KiB K+V, table rows of {per}) forked into 7 slots; host clock to a device synchronise, us, "
          f"median of {args.rounds} rounds (+- half the spread), variants alternating", flush=True)
    print("  variant   fork us (+-)      pages mapped MiB   first reserve + decode step us (+-)   pages taken by that step",
          flush=True)
    for v in ("copy", "share"):
        x = res[v]
        print(f"  {v:7s} {med(x['fork']):10.1f} ({half(x['fork']):7.1f})   {med(x['bytes']) / 2**20:12.1f}       "
              f"{med(x['step']):10.1f} ({half(x['step']):7.1f})                  {med(x['cow']):6d}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--W", default="128,4096")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=16)
    ap.add_argument("--sets", type=int, default=4)
    ap.add_argument("--eager", action="store_true")
    ap.add_argument("--share", action="store_true", help="paged pool: the shared fork against the copying fork")
    ap.add_argument("--page", type=int, default=64, help="--share: page size")
    ap.add_argument("--prompt", type=int, default=100000, help="--share: tokens of the forked prompt")
    args = ap.parse_args()
    import torch
    from sink_attention import _native
    if not torch.cuda.is_available():
        sys.exit("kbench_fork needs the GPU: there is nothing to time without one")
    dev, dt = "cuda", torch.bfloat16
    if args.share:
        print(f"library {_native.LIB_PATH}", flush=True)
        return share_bench(torch, args, dev, dt)
    print(f"gpt-oss K/V geometry H_kv={HKV} D={D} num_sink={NS} bf16, pool of {S} slots; device us per call, median of "
          f"{args.rounds} rounds of {args.calls} calls ({'eager' if args.eager else 'one graph per variant'}), variants "
          f"alternating, {args.sets} slot sets in rotation; library {_native.LIB_PATH}", flush=True)
    print("      W fill    fork   live MiB   fork us (+-)   TB/s moved   index us (+-)   TB/s moved   index / fork",
          flush=True)
    for W in [int(x) for x in args.W.split(",")]:
        for fill in FILLS:
            torch.manual_seed(0)
            layer, rows = _pool(torch, W, fill, dev, dt)
            for fork in FORKS:
                fns, n_pairs = _variants(torch, layer, fork, args.sets, dev)
                live = n_pairs * HKV * rows * D * ES * 2
                cap = n_pairs * HKV * (NS + W) * D * ES * 2
                moved = {"fork": 2 * live, "index": 4 * cap}
                once = {v: _timed(torch, f, args.calls, args.eager) for v, f in fns.items()}
                res = {v: [] for v in fns}
                for _ in range(args.rounds):
                    for v in fns:
                        res[v].append(once[v]())
                med = {v: sorted(x)[len(x) // 2] for v, x in res.items()}
                half = {v: (max(x) - min(x)) / 2 for v, x in res.items()}
                tbs = {v: moved[v] / (med[v] * 1e-6) / 1e12 for v in fns}
                print(f"  {W:5d} {fill:7s} {fork:6s} {live / 2**20:8.2f}   {med['fork']:8.2f} ({half['fork']:5.2f})   "
                      f"{tbs['fork']:8.3f}     {med['index']:8.2f} ({half['index']:5.2f})   {tbs['index']:8.3f}     "
                      f"{med['index'] / med['fork']:8.2f}", flush=True)
            del layer
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
