#!/usr/bin/env python3
"""Micro-bench of the slot-indexed cache calls (exploration tool, not the contract bench), gpt-oss attention geometry
(H_q=64, H_kv=8, D=64, num_sink=4, s_aux, bf16), every ring full and wrapped.  n = 1 is decode_step_dyn, n > 1 is
extend_attention_dyn.

Variants per (W, n), alternating in one process:
    rows8        per-sequence state, B = 8 rows (the reference point; with SFA_LIB_PATH set to a parent build, the
                 parent's kernel)
    rows8_again  the same layer once more: the spread between the two is the yardstick for "no slower"
    slots8_id    a pool of S = 8 with identity slots: the cost of the indirection
    pool64_8     a pool of S = 64 with 8 live sequences (scattered slots): one slot step
    rows64       what was possible before (a): a rows step over all 64 rows
    gather8      what was possible before (b): index_select of the 8 rows (four buffers and the state), a rows step on
                 the copy, index_copy_ of the ring and the state back
--mode wall (default): device time of each variant between two events around --calls calls, median of --rounds rounds.
--mode kernels: --calls calls of each variant after 5 warm-up calls, in the order above, for a kernel trace of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o slots -- python tools/kbench_slots.py --mode kernels
--summarize OUT/.../slots_kernel_trace.csv: median split / reduce kernel time per variant (the trace is cut into blocks
  in issue order; gather8's torch copy kernels are not counted there, its wall time is).
K/V bytes a step reads: live rows x H_kv x (num_sink + W) x D x 2 (K and V) x 2 bytes.
usage: python tools/kbench_slots.py [--mode wall|kernels] [--W 128,4096] [--n 1,4,8] [--variants rows8,slots8_id,...]"""
import argparse
import csv
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "sink-flash-attention-kernel_amd"), ROOT]

B, S, HQ, HKV, D, NS = 8, 64, 64, 8, 64, 4
WARM = 5
VARIANTS = ("rows8", "rows8_again", "slots8_id", "pool64_8", "rows64", "gather8")
LIVE = [3, 60, 17, 42, 9, 31, 55, 24]          # the 8 live slots of the S = 64 pool


def _rows_layer(torch, W, rows, dev, dt):
    from sink_attention import SinkCacheLayer
    layer = SinkCacheLayer(NS, W)
    pre = NS + W + 37                          # full ring, wrapped
    layer.append(torch.randn(rows, HKV, pre, D, device=dev, dtype=dt), torch.randn(rows, HKV, pre, D, device=dev, dtype=dt))
    layer.enable_device_state(per_sequence=True)
    return layer


def _pool(torch, W, slots_total, dev, dt):
    """a pool whose every slot holds a full, wrapped ring (so that any slot can be named)"""
    from sink_attention import SinkCacheLayer
    layer = SinkCacheLayer(NS, W)
    layer.init_pool(slots_total, HKV, D, dt, dev)
    pre = NS + W + 37
    for s0 in range(0, slots_total, 8):
        k = torch.randn(1, HKV, 8 * pre, D, device=dev, dtype=dt)
        layer.prefill_slots(k, torch.randn_like(k), [pre * i for i in range(9)], list(range(s0, s0 + 8)))
    # wrap: commit 37 more tokens so that write_pos != 0
    idx = torch.arange(slots_total, dtype=torch.int32, device=dev)
    for s0 in range(0, slots_total, 8):
        k = torch.randn(8, HKV, 37, D, device=dev, dtype=dt)
        layer.commit_dyn(k, torch.randn_like(k), torch.full((8,), 37, dtype=torch.int32, device=dev), slots=idx[s0:s0 + 8])
    return layer


def _variants(torch, W, n, dev, dt, have_slots):
    sa = torch.randn(HQ, device=dev) * 0.5

    def args(rows):
        q = torch.randn(rows, HQ, n, D, device=dev, dtype=dt)
        k, v = torch.randn(rows, HKV, n, D, device=dev, dtype=dt), torch.randn(rows, HKV, n, D, device=dev, dtype=dt)
        return q, k, v, torch.empty_like(q)

    def call(layer, a, slots=None):
        q, k, v, o = a
        kw = {} if slots is None else {"slots": slots}
        if n == 1:
            return lambda: layer.decode_step_dyn(q, k, v, s_aux=sa, out=o, **kw)
        return lambda: layer.extend_attention_dyn(q, k, v, s_aux=sa, out=o, **kw)

    a8, a64 = args(B), args(S)
    rows8 = _rows_layer(torch, W, B, dev, dt)
    out = {"rows8": call(rows8, a8), "rows8_again": call(rows8, a8)}
    rows64 = _rows_layer(torch, W, S, dev, dt)
    out["rows64"] = call(rows64, a64)
    live = torch.tensor(LIVE, device=dev)
    tmp = _rows_layer(torch, W, B, dev, dt)
    inner = call(tmp, a8)

    def gather8():
        for name in ("sink_k", "sink_v", "window_k", "window_v"):
            torch.index_select(getattr(rows64, name), 0, live, out=getattr(tmp, name))
        torch.index_select(rows64._dev_state, 0, live, out=tmp._dev_state)
        inner()
        rows64.window_k.index_copy_(0, live, tmp.window_k)
        rows64.window_v.index_copy_(0, live, tmp.window_v)
        rows64._dev_state.index_copy_(0, live, tmp._dev_state)

    out["gather8"] = gather8
    if have_slots:
        pool8, pool64 = _pool(torch, W, B, dev, dt), _pool(torch, W, S, dev, dt)
        out["slots8_id"] = call(pool8, a8, torch.arange(B, dtype=torch.int32, device=dev))
        out["pool64_8"] = call(pool64, a8, torch.tensor(LIVE, dtype=torch.int32, device=dev))
    return out


def _setup(args):
    import torch
    from sink_attention import SinkCacheLayer
    have_slots = hasattr(SinkCacheLayer, "init_pool") and hasattr(__import__("sink_attention")._native.lib(),
                                                                  "sfa_decode_ring_step_slots")
    names = [v for v in args.variants.split(",") if have_slots or v not in ("slots8_id", "pool64_8")]
    return torch, names, have_slots


def wall(args):
    torch, names, have_slots = _setup(args)
    dev, dt = "cuda", torch.bfloat16
    kv = lambda rows, W: rows * HKV * (NS + W) * D * 2 * 2
    print(f"gpt-oss geometry H_q={HQ} H_kv={HKV} D={D} num_sink={NS} s_aux bf16, rings full; device us per call, median "
          f"of {args.rounds} rounds of {args.calls} calls (events), variants alternating", flush=True)
    for W in [int(x) for x in args.W.split(",")]:
        for n in [int(x) for x in args.n.split(",")]:
            torch.manual_seed(0)
            fns = _variants(torch, W, n, dev, dt, have_slots)
            res = {v: [] for v in names}
            for v in names:
                for _ in range(WARM):
                    fns[v]()
            torch.cuda.synchronize()
            for _ in range(args.rounds):
                for v in names:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _c in range(args.calls):
                        fns[v]()
                    e1.record()
                    torch.cuda.synchronize()
                    res[v].append(e0.elapsed_time(e1) * 1e3 / args.calls)
            med = {v: sorted(x)[len(x) // 2] for v, x in res.items()}
            spread = {v: max(x) - min(x) for v, x in res.items()}
            print(f"  W={W:5d} n={n}  " + "  ".join(f"{v} {med[v]:7.2f} (+-{spread[v] / 2:4.2f})" for v in names), flush=True)
            print(f"             K/V MiB read per step: 8 live rows {kv(B, W) / 2**20:.2f}, 64 rows {kv(S, W) / 2**20:.2f}; "
                  f"gather8 also copies {kv(B, W) / 2**20:.2f} in and the ring back", flush=True)
            del fns


def kernels(args):
    torch, names, have_slots = _setup(args)
    dev, dt = "cuda", torch.bfloat16
    for W in [int(x) for x in args.W.split(",")]:
        for n in [int(x) for x in args.n.split(",")]:
            torch.manual_seed(0)
            fns = _variants(torch, W, n, dev, dt, have_slots)
            torch.cuda.synchronize()
            for v in names:
                for _ in range(WARM + args.calls):
                    fns[v]()
                torch.cuda.synchronize()
            print(f"W={W} n={n}: {WARM} + {args.calls} calls of each of {', '.join(names)}", flush=True)
            del fns


def summarize(args):
    rows = list(csv.DictReader(open(args.summarize)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    names = args.variants.split(",")
    per = WARM + args.calls
    series = {"split": [], "reduce": []}
    for r in rows:
        name = r["Kernel_Name"]
        kind = "split" if ("multi_split_" in name or "decode_split_kernel" in name) else \
            "reduce" if ("multi_reduce_kernel" in name or "decode_reduce" in name) else None
        if kind:
            series[kind].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    cfgs = [(W, n) for W in [int(x) for x in args.W.split(",")] for n in [int(x) for x in args.n.split(",")]]
    med = lambda xs: sorted(xs)[len(xs) // 2]
    nv = len(names)
    assert len(series["split"]) == len(cfgs) * nv * per, (len(series["split"]), len(cfgs), nv, per)
    print(f"# gpt-oss geometry; kernel us (split + reduce), median of {args.calls} calls after {WARM} warm-up")
    print("#     W   n   " + "  ".join(f"{v:>16s}" for v in names))
    for c, (W, n) in enumerate(cfgs):
        get = lambda kind, i: med(series[kind][(nv * c + i) * per + WARM:(nv * c + i + 1) * per])
        print(f"  {W:5d} {n:3d}   " + "  ".join(f"{get('split', i):8.2f} +{get('reduce', i):6.2f}" for i in range(nv)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="wall", choices=["wall", "kernels"])
    ap.add_argument("--W", default="128,4096")
    ap.add_argument("--n", default="1,4,8")
    ap.add_argument("--variants", default=",".join(VARIANTS))
    ap.add_argument("--rounds", type=int, default=5)
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
