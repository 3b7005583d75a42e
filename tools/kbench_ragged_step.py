#!/usr/bin/env python3
"""Micro-bench of the packed ragged step (exploration tool, not the contract bench), gpt-oss attention geometry
(H_q=64, H_kv=8, D=64, num_sink=4, s_aux, bf16), a pool of 8 slots, every ring full and wrapped.  All variants commit
(attend + store + advance), so the rings stay full and every call does the same work.

Steps:
    dec7_pre256 / dec7_pre512   7 decode rows (1 token) + 1 prefill chunk of 256 / 512 tokens
    dec4_draft4                 4 decode rows + 4 draft rows of 8 tokens
Variants per (W, step), alternating in one process:
    ragged     one ragged_step_dyn over the pack (skipped where the library lacks it: a parent build)
    per_len    what was possible before (a): one extend_step_dyn(slots=) per distinct length
    padded     what was possible before (b): one extend_step_dyn(slots=) with every row padded to the longest chunk.
               Timing only: a padded row commits its padding too, which a real caller would have to undo.
    ragged_admit   the ragged call with admit=True (SFA_FLAG_RAGGED_ADMIT) on the same pool: every sequence continues, so
               this is the cost of the flag alone (only when named in --variants; skipped where the keyword is missing)
--admit: the admission mix instead of the variants above.  The longest sequence and the first two decode rows sit on FRESH
    slots and are admitted by the call; commit is off (a dry run), so that the slots stay fresh and every call does the
    same work.  Variants: admit_mix (admit=True) and dry (the same pack, every slot full, admit=False, commit off).
--tree: the speculative step instead: 4 decode rows + 4 draft trees of 16 nodes (binary trees, 4 nodes accepted) + one
    prefill chunk of 256 tokens on a pool of 9 slots.  Variants: packed_tree = one ragged_step_dyn(parent=, commit_seq=)
    that stores the decode rows and the chunk, plus one commit_packed_dyn for the accepted paths; split_up = what was
    possible before: a ragged_step_dyn for the 5 sequences that do not speculate, plus extend_attention_tree_dyn(slots=)
    and commit_path_dyn(slots=) for the 4 trees.  Skipped where the library lacks the packed tree call.
--pool-dtypes bf16,fp8: the pool format instead (wall mode): a serving geometry (H_q=32, H_kv=8, D=128, num_sink=4, bf16
    activations, a pool of 64 slots, every ring full), steps dec64 (64 decode rows) and dec63_pre512 (63 decode rows + one
    512-token chunk), one committing ragged_step_dyn per step on a pool of each named format, alternating in one process.
    Prints ms per step, the spread, and GB/s against the bytes the format must read (the live cache rows of every named
    slot at 2 or 1 bytes per element plus the 16-bit chunk K/V).  fp8 is skipped where the library lacks the call.
--page-size 64,256: the paged pool instead (wall mode): the serving geometry and steps of --pool-dtypes
    on a contiguous bf16 pool and, per page size P, on two paged pools of the same content - `ident` (slot s owns pages
    s * Wc / P + j) and `shuf` (a seeded shuffle of the page pool) - all alternating in one process.  Prints ms per step, the
    spread and each paged time over the contiguous one.  Skipped where the library lacks the call.
--pool-dtypes bf16,fp8 --page-size 64 together: the same geometry and steps on the contiguous pool of
    each named format and, per page size, on a paged pool of each (shuffled table) - with fp8 the last one is the paged
    FP8 pool (init_pool(page_size=P, kv_dtype=float8_e4m3fn)) - all alternating in one process.  Prints ms per step, the
    spread and each time over the contiguous 16-bit one.  A pool the library lacks is skipped (a parent build).
--pkg DIR: import sink_attention from DIR/sink-flash-attention-kernel_amd (a checkout of another commit with its own
    built library), to time two commits' libraries with one tool.
--mode wall (default): device time of each variant between two events around --calls calls, median of --rounds rounds.
--mode kernels: --calls calls of each variant after 5 warm-up calls, in the order above, for a kernel trace of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o rstep -- python tools/kbench_ragged_step.py --mode kernels
--summarize OUT/.../rstep_kernel_trace.csv: per (W, step, variant) the median per call of the summed prep / split /
  reduce / advance kernel times (the trace is cut into blocks in issue order).
usage: python tools/kbench_ragged_step.py [--mode wall|kernels] [--W 128,4096] [--steps ...] [--variants ...]
       [--admit | --tree | --pool-dtypes bf16,fp8 | --page-size 64,256 | --pool-dtypes bf16,fp8 --page-size 64] [--pkg DIR]"""
import argparse
import csv
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--pkg" in sys.argv[1:-1]:       # before the first import of sink_attention
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--pkg") + 1])
sys.path[:0] = [os.path.join(ROOT, "sink-flash-attention-kernel_amd"), ROOT]

S, HQ, HKV, D, NS = 8, 64, 8, 64, 4
WARM = 5
STEPS = {"dec7_pre256": [1] * 7 + [256], "dec7_pre512": [1] * 7 + [512], "dec4_draft4": [1] * 4 + [8] * 4}
VARIANTS = ("ragged", "per_len", "padded")
KINDS = ("prep", "split", "reduce", "advance")


def _pool(torch, W, dev, dt, S=S):
    from sink_attention import SinkCacheLayer
    layer = SinkCacheLayer(NS, W)
    layer.init_pool(S, HKV, D, dt, dev)
    pre = NS + W + 37                          # full ring, wrapped
    k = torch.randn(1, HKV, S * pre, D, device=dev, dtype=dt)
    layer.prefill_slots(k, torch.randn_like(k), [pre * i for i in range(S + 1)], list(range(S)))
    return layer


TREE_STEP = [1] * 4 + [16] * 4 + [256]          # --tree: decode rows, draft trees, one prompt chunk
TREE_N, TREE_ACCEPT = 16, 4


def _tree_variants(torch, W, dev, dt):
    """--tree: the packed speculative step against the same step split into the calls that existed before"""
    sa = torch.randn(HQ, device=dev) * 0.5
    mk = lambda rows, h, n: torch.randn(rows, h, n, D, device=dev, dtype=dt)
    i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=dev)
    lengths, ns = TREE_STEP, len(TREE_STEP)
    cu = [sum(lengths[:i]) for i in range(ns + 1)]
    T = cu[-1]
    tree = [(u - 1) // 2 if u else -1 for u in range(TREE_N)]              # binary
    walk = [0, 1, 3, 7] + [0] * (TREE_N - TREE_ACCEPT)                     # its leftmost root-to-depth-3 path
    is_tree = [n == TREE_N for n in lengths]
    parent = sum((tree if t else list(range(-1, n - 1)) for n, t in zip(lengths, is_tree)), [])
    path = sum((walk if t else list(range(n)) for n, t in zip(lengths, is_tree)), [])
    q, k, v, o = mk(1, HQ, T), mk(1, HKV, T), mk(1, HKV, T), torch.empty(1, HQ, T, D, device=dev, dtype=dt)
    a = dict(cu=i32(cu), slots=i32(list(range(ns))), parent=i32(parent), path=i32(path),
             commit_seq=i32([0 if t else 1 for t in is_tree]), count=i32([TREE_ACCEPT if t else 0 for t in is_tree]))
    pool = _pool(torch, W, dev, dt, ns)

    def packed_tree():
        pool.ragged_step_dyn(q, k, v, a["cu"], a["slots"], s_aux=sa, out=o, commit=True, parent=a["parent"],
                             commit_seq=a["commit_seq"])
        pool.commit_packed_dyn(k, v, a["cu"], a["slots"], a["count"], path=a["path"])

    rest = [i for i in range(ns) if not is_tree[i]]
    trees = [i for i in range(ns) if is_tree[i]]
    lr = [lengths[i] for i in rest]
    Tr = sum(lr)
    qr, kr, vr, orr = mk(1, HQ, Tr), mk(1, HKV, Tr), mk(1, HKV, Tr), torch.empty(1, HQ, Tr, D, device=dev, dtype=dt)
    b = dict(cu=i32([sum(lr[:i]) for i in range(len(lr) + 1)]), slots=i32(rest), tslots=i32(trees),
             parent=i32([tree] * len(trees)), path=i32([walk] * len(trees)), count=i32([TREE_ACCEPT] * len(trees)))
    qt, kt, vt = mk(len(trees), HQ, TREE_N), mk(len(trees), HKV, TREE_N), mk(len(trees), HKV, TREE_N)
    ot = torch.empty_like(qt)
    pool2 = _pool(torch, W, dev, dt, ns)

    def split_up():
        pool2.ragged_step_dyn(qr, kr, vr, b["cu"], b["slots"], s_aux=sa, out=orr, commit=True)
        pool2.extend_attention_tree_dyn(qt, kt, vt, b["parent"], s_aux=sa, out=ot, slots=b["tslots"])
        pool2.commit_path_dyn(kt, vt, b["path"], b["count"], slots=b["tslots"])

    return {"packed_tree": packed_tree, "split_up": split_up}


def _variants(torch, W, lengths, dev, dt, have_ragged, names=()):
    sa = torch.randn(HQ, device=dev) * 0.5
    mk = lambda rows, h, n: torch.randn(rows, h, n, D, device=dev, dtype=dt)
    out = {}
    if have_ragged:
        T = sum(lengths)
        qr, kr, vr = mk(1, HQ, T), mk(1, HKV, T), mk(1, HKV, T)   # names of their own: q is rebound below
        cu = torch.tensor([sum(lengths[:i]) for i in range(S + 1)], dtype=torch.int32, device=dev)
        slots = torch.arange(S, dtype=torch.int32, device=dev)
        pool, o = _pool(torch, W, dev, dt), torch.empty_like(qr)
        out["ragged"] = lambda: pool.ragged_step_dyn(qr, kr, vr, cu, slots, s_aux=sa, out=o, commit=True)
        if have_ragged > 1:      # the flag on the same pool and inputs: no further draw
            out["ragged_admit"] = lambda: pool.ragged_step_dyn(qr, kr, vr, cu, slots, s_aux=sa, out=o, commit=True, admit=True)
        if have_ragged > 1 and ("admit_mix" in names or "dry" in names):
            fresh = [0, 1, max(range(S), key=lambda i: lengths[i])]
            pool_f, pool_d = _pool(torch, W, dev, dt), _pool(torch, W, dev, dt)
            pool_f.release_slots(fresh)
            out["admit_mix"] = lambda: pool_f.ragged_step_dyn(qr, kr, vr, cu, slots, s_aux=sa, out=o, commit=False, admit=True)
            out["dry"] = lambda: pool_d.ragged_step_dyn(qr, kr, vr, cu, slots, s_aux=sa, out=o, commit=False)
    groups = []
    for n in sorted(set(lengths)):
        idx = [i for i, x in enumerate(lengths) if x == n]
        q = mk(len(idx), HQ, n)
        groups.append((q, mk(len(idx), HKV, n), mk(len(idx), HKV, n), torch.empty_like(q),
                       torch.tensor(idx, dtype=torch.int32, device=dev)))
    pool2 = _pool(torch, W, dev, dt)

    def per_len():
        for q, k, v, o, sl in groups:
            pool2.extend_step_dyn(q, k, v, s_aux=sa, out=o, slots=sl)

    out["per_len"] = per_len
    n = max(lengths)
    qp, kp, vp = mk(S, HQ, n), mk(S, HKV, n), mk(S, HKV, n)
    pool3, op, sl_all = _pool(torch, W, dev, dt), torch.empty_like(qp), torch.arange(S, dtype=torch.int32, device=dev)
    out["padded"] = lambda: pool3.extend_step_dyn(qp, kp, vp, s_aux=sa, out=op, slots=sl_all)
    return out


def _setup(args):
    import inspect
    import torch
    import sink_attention
    from sink_attention import SinkCacheLayer
    have = hasattr(SinkCacheLayer, "ragged_step_dyn") and hasattr(sink_attention._native.lib(), "sfa_decode_ring_ragged_slots")
    # 2: the admit keyword too (a library without the flag ignores the bit: such a run times the unflagged kernels)
    have = int(have) + int(have and "admit" in inspect.signature(SinkCacheLayer.ragged_step_dyn).parameters)
    # 3: the packed tree call and the packed commit too
    have += int(have == 2 and hasattr(SinkCacheLayer, "commit_packed_dyn") and
                hasattr(sink_attention._native.lib(), "sfa_decode_ring_ragged_tree_slots"))
    want = ["packed_tree", "split_up"] if args.tree else ["admit_mix", "dry"] if args.admit else args.variants.split(",")
    need = {"ragged": 1, "ragged_admit": 2, "admit_mix": 2, "dry": 2, "packed_tree": 3, "split_up": 3}
    names = [v for v in want if have >= need.get(v, 0)]
    return torch, names, have


def wall(args):
    torch, names, have = _setup(args)
    dev, dt = "cuda", torch.bfloat16
    print(f"gpt-oss geometry H_q={HQ} H_kv={HKV} D={D} num_sink={NS} s_aux bf16, pool of {len(TREE_STEP) if args.tree else S}, rings full; device us per "
          f"step, median of {args.rounds} rounds of {args.calls} calls (events), variants alternating", flush=True)
    for W in [int(x) for x in args.W.split(",")]:
        for step in (["dec4_tree4_pre256"] if args.tree else args.steps.split(",")):
            torch.manual_seed(0)
            fns = _tree_variants(torch, W, dev, dt) if args.tree else _variants(torch, W, STEPS[step], dev, dt, have, names)
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
            print(f"  W={W:5d} {step:12s} T={sum(TREE_STEP if args.tree else STEPS[step]):4d}  " +
                  "  ".join(f"{v} {med[v]:8.2f} (+-{spread[v] / 2:5.2f})" for v in names), flush=True)
            del fns


POOL_S, POOL_HQ, POOL_HKV, POOL_D = 64, 32, 8, 128
POOL_STEPS = {"dec64": [1] * 64, "dec63_pre512": [1] * 63 + [512]}


def _alternate(torch, args, fns, names):
    """ms per call of every variant: WARM calls of each, then args.rounds rounds in which each variant in turn runs
    args.calls calls between two events"""
    res = {n: [] for n in names}
    for n in names:
        for _ in range(WARM):
            fns[n]()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for n in names:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _c in range(args.calls):
                fns[n]()
            e1.record()
            torch.cuda.synchronize()
            res[n].append(e0.elapsed_time(e1) / args.calls)
    return res


def pool_dtypes(args):
    """--pool-dtypes: the same committing packed step on a 16-bit and on an FP8 pool, alternating"""
    import torch
    from sink_attention import SinkCacheLayer, _native
    dev, dt = "cuda", torch.bfloat16
    fmt = {"bf16": torch.bfloat16, "fp8": getattr(torch, "float8_e4m3fn", None)}
    names = [n for n in args.pool_dtypes.split(",")
             if n != "fp8" or hasattr(_native.lib(), "sfa_decode_ring_ragged_fp8_slots")]
    Ws = [int(x) for x in args.W.split(",")] if args.W != "128,4096" else [4096]
    print(f"library {os.path.relpath(_native.LIB_PATH, ROOT)}\nserving geometry H_q={POOL_HQ} H_kv={POOL_HKV} D={POOL_D} num_sink={NS} s_aux bf16 "
          f"activations, pool of {POOL_S}, rings full; device ms per committing step, median of {args.rounds} rounds of "
          f"{args.calls} calls (events), formats alternating; GB/s = bytes the format must read / median", flush=True)
    for W in Ws:
        pools = {}
        pre = NS + W + 37                          # full ring, wrapped
        torch.manual_seed(0)
        k = torch.randn(1, POOL_HKV, POOL_S * pre, POOL_D, device=dev, dtype=dt)
        v = torch.randn_like(k)
        for n in names:
            pools[n] = SinkCacheLayer(NS, W)
            pools[n].init_pool(POOL_S, POOL_HKV, POOL_D, fmt[n], dev)
            pools[n].prefill_slots(k, v, [pre * i for i in range(POOL_S + 1)], list(range(POOL_S)))
        del k, v
        sa = torch.randn(POOL_HQ, device=dev) * 0.5
        for step, lengths in POOL_STEPS.items():
            T = sum(lengths)
            q = torch.randn(1, POOL_HQ, T, POOL_D, device=dev, dtype=dt)
            kn, vn = (torch.randn(1, POOL_HKV, T, POOL_D, device=dev, dtype=dt) for _ in range(2))
            o = torch.empty_like(q)
            cu = torch.tensor([sum(lengths[:i]) for i in range(POOL_S + 1)], dtype=torch.int32, device=dev)
            slots = torch.arange(POOL_S, dtype=torch.int32, device=dev)
            fns = {n: (lambda p=pools[n]: p.ragged_step_dyn(q, kn, vn, cu, slots, s_aux=sa, out=o, commit=True)) for n in names}
            res = _alternate(torch, args, fns, names)
            cells = []
            for n in names:
                x = sorted(res[n])
                nbytes = 2 * POOL_HKV * POOL_D * (POOL_S * (NS + W) * (1 if n == "fp8" else 2) + T * 2)
                cells.append(f"{n} {x[len(x) // 2]:7.4f} ms (min {x[0]:.4f} max {x[-1]:.4f}) {nbytes / 2 ** 20:7.1f} MiB "
                             f"{nbytes / x[len(x) // 2] / 1e6:7.1f} GB/s")
            print(f"  W={W:5d} {step:12s} T={T:4d}  " + "   ".join(cells), flush=True)
            if len(names) == 2:
                a, b = (sorted(res[n])[len(res[n]) // 2] for n in names)
                print(f"        {names[1]} / {names[0]} time {b / a:.3f}", flush=True)


def page_sizes(args):
    """--page-size: the same committing packed step on a contiguous pool and on paged pools, alternating"""
    import torch
    from sink_attention import SinkCacheLayer, _native
    dev, dt = "cuda", torch.bfloat16
    if not hasattr(_native.lib(), "sfa_decode_ring_ragged_paged_slots"):
        print("this library has no paged pool: nothing to time")
        return
    Ws = [int(x) for x in args.W.split(",")] if args.W != "128,4096" else [4096]
    print(f"library {os.path.relpath(_native.LIB_PATH, ROOT)}\nserving geometry H_q={POOL_HQ} H_kv={POOL_HKV} D={POOL_D} num_sink={NS} s_aux bf16, "
          f"pool of {POOL_S}, rings full; device ms per committing step, median of {args.rounds} rounds of {args.calls} calls "
          f"(events) after {WARM} warm-up calls, pools alternating; ident / shuf: identity / seeded-shuffle page table", flush=True)
    for W in Ws:
        pre = NS + W + 37                          # full ring, wrapped
        torch.manual_seed(0)
        k = torch.randn(1, POOL_HKV, POOL_S * pre, POOL_D, device=dev, dtype=dt)
        v = torch.randn_like(k)
        cu_pre, every = [pre * i for i in range(POOL_S + 1)], list(range(POOL_S))
        pools = {"contig": SinkCacheLayer(NS, W)}
        pools["contig"].init_pool(POOL_S, POOL_HKV, POOL_D, dt, dev)
        for P in [int(x) for x in args.page_size.split(",")]:
            per = W // P
            for kind in ("ident", "shuf"):
                p = pools[f"P{P}_{kind}"] = SinkCacheLayer(NS, W)
                p.init_pool(POOL_S, POOL_HKV, POOL_D, dt, dev, page_size=P)
                order = torch.arange(POOL_S * per) if kind == "ident" else \
                    torch.randperm(POOL_S * per, generator=torch.Generator().manual_seed(P))
                p.page_table.copy_(order.reshape(POOL_S, per).to(torch.int32))
        for p in pools.values():
            p.prefill_slots(k, v, cu_pre, every)
        del k, v
        names = list(pools)
        sa = torch.randn(POOL_HQ, device=dev) * 0.5
        for step, lengths in POOL_STEPS.items():
            T = sum(lengths)
            q = torch.randn(1, POOL_HQ, T, POOL_D, device=dev, dtype=dt)
            kn, vn = (torch.randn(1, POOL_HKV, T, POOL_D, device=dev, dtype=dt) for _ in range(2))
            o = torch.empty_like(q)
            cu = torch.tensor([sum(lengths[:i]) for i in range(POOL_S + 1)], dtype=torch.int32, device=dev)
            slots = torch.arange(POOL_S, dtype=torch.int32, device=dev)
            fns = {n: (lambda p=pools[n]: p.ragged_step_dyn(q, kn, vn, cu, slots, s_aux=sa, out=o, commit=True)) for n in names}
            res = _alternate(torch, args, fns, names)
            med = {n: sorted(x)[len(x) // 2] for n, x in res.items()}
            print(f"  W={W:5d} {step:12s} T={T:4d}", flush=True)
            for n in names:
                x = sorted(res[n])
                print(f"      {n:12s} {med[n]:7.4f} ms (min {x[0]:.4f} max {x[-1]:.4f})  / contig {med[n] / med['contig']:.3f}", flush=True)


def paged_dtypes(args):
    """--pool-dtypes with --page-size: contiguous and paged pools of each format, alternating"""
    import torch
    from sink_attention import SinkCacheLayer, _native
    dev, dt = "cuda", torch.bfloat16
    lib, fp8 = _native.lib(), getattr(torch, "float8_e4m3fn", None)
    have = {"bf16": True, "fp8": hasattr(lib, "sfa_decode_ring_ragged_fp8_slots"),
            "paged_bf16": hasattr(lib, "sfa_decode_ring_ragged_paged_slots"),
            "paged_fp8": hasattr(lib, "sfa_decode_ring_ragged_paged_fp8_slots")}
    fmts = args.pool_dtypes.split(",")
    if set(fmts) - {"bf16", "fp8"}:
        sys.exit(f"--pool-dtypes takes bf16 and fp8, got {args.pool_dtypes}")
    fmts = [n for n in fmts if have[n]]
    Ws = [int(x) for x in args.W.split(",")] if args.W != "128,4096" else [4096]
    print(f"library {os.path.relpath(_native.LIB_PATH, ROOT)}\nserving geometry H_q={POOL_HQ} H_kv={POOL_HKV} D={POOL_D} num_sink={NS} s_aux bf16 "
          f"activations, pool of {POOL_S}, rings full; device ms per committing step, median of {args.rounds} rounds of "
          f"{args.calls} calls (events) after {WARM} warm-up calls, pools alternating; paged pools: seeded-shuffle page table",
          flush=True)
    for W in Ws:
        pre = NS + W + 37                          # full ring, wrapped
        torch.manual_seed(0)
        k = torch.randn(1, POOL_HKV, POOL_S * pre, POOL_D, device=dev, dtype=dt)
        v = torch.randn_like(k)
        pools = {}
        for n in fmts:
            pools[n] = SinkCacheLayer(NS, W)
            pools[n].init_pool(POOL_S, POOL_HKV, POOL_D, fp8 if n == "fp8" else dt, dev)
        for P in [int(x) for x in args.page_size.split(",")]:
            per = W // P
            for n in fmts:
                if not have["paged_" + n]:
                    print(f"  this library has no paged {n} pool: skipped", flush=True)
                    continue
                p = pools[f"P{P}_{n}"] = SinkCacheLayer(NS, W)
                p.init_pool(POOL_S, POOL_HKV, POOL_D, dt, dev, page_size=P, **(dict(kv_dtype=fp8) if n == "fp8" else {}))
                order = torch.randperm(POOL_S * per, generator=torch.Generator().manual_seed(P))
                p.page_table.copy_(order.reshape(POOL_S, per).to(torch.int32))
        for p in pools.values():
            p.prefill_slots(k, v, [pre * i for i in range(POOL_S + 1)], list(range(POOL_S)))
        del k, v
        names = list(pools)
        sa = torch.randn(POOL_HQ, device=dev) * 0.5
        for step, lengths in POOL_STEPS.items():
            T = sum(lengths)
            q = torch.randn(1, POOL_HQ, T, POOL_D, device=dev, dtype=dt)
            kn, vn = (torch.randn(1, POOL_HKV, T, POOL_D, device=dev, dtype=dt) for _ in range(2))
            o = torch.empty_like(q)
            cu = torch.tensor([sum(lengths[:i]) for i in range(POOL_S + 1)], dtype=torch.int32, device=dev)
            slots = torch.arange(POOL_S, dtype=torch.int32, device=dev)
            fns = {n: (lambda p=pools[n]: p.ragged_step_dyn(q, kn, vn, cu, slots, s_aux=sa, out=o, commit=True)) for n in names}
            res = _alternate(torch, args, fns, names)
            med = {n: sorted(x)[len(x) // 2] for n, x in res.items()}
            print(f"  W={W:5d} {step:12s} T={T:4d}", flush=True)
            for n in names:
                x = sorted(res[n])
                print(f"      {n:12s} {med[n]:7.4f} ms (min {x[0]:.4f} max {x[-1]:.4f})  / {names[0]} {med[n] / med[names[0]]:.3f}",
                      flush=True)


def kernels(args):
    torch, names, have = _setup(args)
    dev, dt = "cuda", torch.bfloat16
    for W in [int(x) for x in args.W.split(",")]:
        for step in args.steps.split(","):
            torch.manual_seed(0)
            fns = _variants(torch, W, STEPS[step], dev, dt, have, names)
            torch.cuda.synchronize()
            for v in names:
                for _ in range(WARM + args.calls):
                    fns[v]()
                torch.cuda.synchronize()
            print(f"W={W} {step}: {WARM} + {args.calls} calls of each of {', '.join(names)}", flush=True)
            del fns


def summarize(args):
    rows = list(csv.DictReader(open(args.summarize)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    names = args.variants.split(",")
    per = WARM + args.calls
    ev = []
    for r in rows:
        name = r["Kernel_Name"]
        kind = "prep" if "ragged_prep_kernel" in name else "split" if "multi_split_" in name else \
            "reduce" if "multi_reduce_kernel" in name else "advance" if "ring_advance_" in name else None
        if kind:
            ev.append((kind, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    med = lambda xs: sorted(xs)[len(xs) // 2]
    print(f"# gpt-oss geometry; summed kernel us per step (prep + split + reduce + advance), median of {args.calls} steps "
          f"after {WARM} warm-up")
    pos = 0
    for W in [int(x) for x in args.W.split(",")]:
        for step in args.steps.split(","):
            cells = []
            for v in names:
                launches = 1 if v != "per_len" else len(set(STEPS[step]))      # split launches per step
                steps = []
                for _ in range(per):
                    tot = dict.fromkeys(KINDS, 0.0)
                    seen = 0
                    while pos < len(ev):
                        kind, us = ev[pos]
                        if kind == "split":
                            if seen == launches:
                                break
                            seen += 1
                        elif kind == "prep" and seen:
                            break
                        tot[kind] += us
                        pos += 1
                    steps.append(tot)
                body = steps[WARM:]
                cells.append(f"{v} " + " + ".join(f"{med([s[k] for s in body]):.2f}" for k in KINDS) +
                             f" = {med([sum(s.values()) for s in body]):.2f}")
            print(f"  W={W:5d} {step:12s}  " + "   ".join(cells))
    assert pos == len(ev), (pos, len(ev))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="wall", choices=["wall", "kernels"])
    ap.add_argument("--W", default="128,4096")
    ap.add_argument("--steps", default=",".join(STEPS))
    ap.add_argument("--variants", default=",".join(VARIANTS))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--admit", action="store_true", help="the admission mix: variants admit_mix and dry")
    ap.add_argument("--tree", action="store_true", help="the speculative step (wall mode): variants packed_tree and split_up")
    ap.add_argument("--summarize", default=None, help="kernel_trace.csv of a --mode kernels run")
    ap.add_argument("--pool-dtypes", default=None, help="bf16,fp8: the packed step on pools of these formats (wall mode)")
    ap.add_argument("--page-size", default=None, help="64,256: the packed step on a contiguous and on paged pools (wall mode)")
    ap.add_argument("--pkg", default=None, help="a checkout of another commit (built) to import sink_attention from")
    args = ap.parse_args()
    if args.summarize:
        summarize(args)
    elif args.page_size and args.pool_dtypes:
        paged_dtypes(args)
    elif args.page_size:
        page_sizes(args)
    elif args.pool_dtypes:
        pool_dtypes(args)
    elif args.mode == "kernels":
        kernels(args)
    else:
        wall(args)


if __name__ == "__main__":
    main()
