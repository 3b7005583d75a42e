"""Which splits, rounds and head-loop trips a single-token decode launch takes: a pure-Python restatement of the launch
arithmetic of csrc/sfa_decode.hip, the way tests/grid_regime.py restates the work lists and tests/packed_regime.py the
packed step.  Sources: decode_plan (lanes per key, head-group tile, keys per iteration, split count and its cap),
decode_counter_bytes and sfa_decode_workspace_bytes (the workspace layout), decode_split_kernel (key ranges of a split,
the clamped tail loads, the fresh slot, the head loop, the one-pass fold's lane width) and reduce_head (statistics rounds
of W splits, O rounds of 8).  No GPU, no product import.

plan(B, Hq, Hkv, Nkv, D, dtype)        the DecodePlan and what it is made of
workspace_bytes / layout               the counters at the start, then the M, L and O partials
regime(case, state_rows, ...)          per batch row: key counts, class of every split of the launched grid, the split of
                                       the fresh slot, live keys of each split's last iteration, trips and rounds

Pinned on the CPU against sfa_decode_workspace_bytes (tests/test_decode_probes.py: max_splits and the layout) and on the
GPU against the lpk{}_gt{}_s{} suffix of sfa_last_path() (tests/test_gpu_decode_edges.py, every case).

The case tables of tests/test_gpu_decode_edges.py live here (MANY, GROUPS, FILLS) with the cache states they run at, so
that the CPU proofs of tests/test_decode_probes.py walk the very inputs the GPU runs."""
import torch

TARGET_WGS = 2048
MIN_KEYS = 256
O_ROUND = 8                 # O rows requested together by reduce_head
REDUCE_W = 64               # lanes that share the statistics in decode_reduce_kernel
DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
ES = {torch.float32: 4, torch.float16: 2, torch.bfloat16: 2}
SFA_DTYPE = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}      # include/sfa.h


def cdiv(a, b):
    return -(-a // b)


def round_up(a, b):
    return cdiv(a, b) * b


# ------------------------------------------------------------------------------------------------ launch arithmetic
def plan(B, Hq, Hkv, Nkv, D, dtype):
    """decode_plan: lpk lanes hold one key row (16 bytes each), gt q heads of a group share the K/V registers, U keys in
    flight per lane group, iter_keys keys per trip of the key loop of one workgroup (4 waves)."""
    row_bytes = D * ES[dtype]
    assert D > 0 and row_bytes % 16 == 0 and row_bytes <= 1024 and Hq % Hkv == 0
    lpk = 2
    while lpk < row_bytes // 16:
        lpk *= 2
    g = Hq // Hkv
    gt = 8 if g % 8 == 0 else 4 if g % 4 == 0 else 1
    U = 8 if gt <= 4 else 4
    iter_keys = 4 * (64 // lpk) * U
    want = max(min(cdiv(TARGET_WGS, max(B * Hkv, 1)), max(cdiv(Nkv, max(iter_keys, MIN_KEYS)), 1)), 1)
    n = max(Nkv, 1)
    kps = cdiv(cdiv(n, want), iter_keys) * iter_keys
    return dict(lpk=lpk, gt=gt, g=g, U=U, iter_keys=iter_keys, want=want, max_splits=want, kps=kps, splits=cdiv(n, kps),
                chunks=row_bytes // 16)


def counter_bytes(B, Hkv):
    return round_up((B * Hkv + 1) * 4, 256)


def workspace_bytes(B, Hq, Hkv, Nkv, D, dtype):
    """sfa_decode_workspace_bytes: the counters, then partials for max_splits splits (the largest count any key count
    up to Nkv plans)"""
    return counter_bytes(B, Hkv) + round_up(B * Hq * plan(B, Hq, Hkv, Nkv, D, dtype)["max_splits"] * (D + 2) * 4, 256)


def layout(B, Hq, Hkv, S, D):
    """byte ranges of a launch with S splits: {"cnt": (0, n), "M": (off, n), "L": ..., "O": ...}; M / L hold B * Hq * S
    floats, O B * Hq * S * D"""
    c = counter_bytes(B, Hkv)
    n = B * Hq * S * 4
    return dict(cnt=(0, c), M=(c, n), L=(c + n, n), O=(c + 2 * n, n * D), end=c + 2 * n + n * D)


def fold_width(D, g):
    """lanes that share the split statistics in the one-pass fold: a half-wave per head when D <= 128 and g > 4"""
    return 32 if D <= 128 and g > 4 else 64


def path_suffix(pl):
    return f"lpk{pl['lpk']}_gt{pl['gt']}_s{pl['splits']}"


def _dtype(case):
    return DT[case["dtype"]] if isinstance(case["dtype"], str) else case["dtype"]


def regime(case, state_rows, step=True, device_state=False):
    """case: dict(B, Hq, Hkv, D, ns, Wc, dtype); state_rows: one (sink_len, window_len, write_pos) per batch row, the cache
    state BEFORE the call.  step: the call stores a token (the fused step) - else it attends over the state as it is.
    device_state: the grid is the full cache's (ns + Wc keys) whatever the rows hold; else every row must hold the same
    counts and the grid is planned for them.  Returns (plan, rows): rows[b] = dict(N1, Nkv, slot, cls, n_keys, tail_live,
    clamped, fresh_split, full, partial, empty); plan gains trips, the rounds and the path suffix."""
    B, Hq, Hkv, D, ns, Wc = (case[x] for x in ("B", "Hq", "Hkv", "D", "ns", "Wc"))
    dt = _dtype(case)
    assert len(state_rows) == B
    rows = []
    for sl, wl, wp in state_rows:
        wl1 = min(wl + 1, Wc) if step else wl
        rows.append(dict(N1=sl, Nkv=sl + wl1, slot=wp if step else None))
    if device_state:
        pl = plan(B, Hq, Hkv, ns + Wc, D, dt)
    else:
        assert len({(r["N1"], r["Nkv"]) for r in rows}) == 1, "host state: one state for the whole batch"
        pl = plan(B, Hq, Hkv, rows[0]["Nkv"], D, dt)
    S, kps, it = pl["splits"], pl["kps"], pl["iter_keys"]
    for r in rows:
        assert r["Nkv"] <= S * kps
        n = [max(min((s + 1) * kps, r["Nkv"]) - s * kps, 0) for s in range(S)]
        r["n_keys"] = n
        r["k_beg"] = [s * kps for s in range(S)]
        r["cls"] = ["full" if x == kps else "empty" if x == 0 else "partial" for x in n]
        r["tail_live"] = [x - (cdiv(x, it) - 1) * it if x else 0 for x in n]
        r["clamped"] = [it - t if x else 0 for x, t in zip(n, r["tail_live"])]
        r["fresh_split"] = None if r["slot"] is None else (r["N1"] + r["slot"]) // kps
        for c in ("full", "partial", "empty"):
            r[c] = [s for s in range(S) if r["cls"][s] == c]
    W1 = fold_width(D, pl["g"])
    pl = dict(pl, trips=pl["g"] // pl["gt"], stat_rounds_reduce=cdiv(S, REDUCE_W), fold_w=W1, stat_rounds_fold=cdiv(S, W1),
              o_rounds=cdiv(S, O_ROUND), suffix=path_suffix(pl), dact_false=pl["lpk"] - pl["chunks"])
    return pl, rows


def describe(pl, rows):
    """one line per launch for the tests' output"""
    r = [f"N={x['Nkv']} e{len(x['empty'])} p{len(x['partial'])} fresh@{x['fresh_split']} tail{max(x['tail_live'])}"
         for x in rows]
    return (f"{pl['suffix']} kps={pl['kps']} iter={pl['iter_keys']} trips={pl['trips']} stat_rounds={pl['stat_rounds_reduce']}/"
            f"{pl['stat_rounds_fold']}(W{pl['fold_w']}) o_rounds={pl['o_rounds']} dact_false={pl['dact_false']} rows[" +
            "; ".join(sorted(set(r))) + "]")


# ------------------------------------------------------------------------------------------------ case tables
# many: the smallest shape whose full ring plans S = 65 at kps = 256 (the last split holds one key).  states: the cache
# states BEFORE the step, one launch each (the whole batch shares a state); 10300: the slot lies in split 40
MANY_WC = 16381
MANY = [
    dict(id="many", dtype="bf16", B=2, Hq=8, Hkv=1, D=64, ns=4, Wc=MANY_WC,
         states=[(4, MANY_WC, 0), (4, MANY_WC, 10300), (4, MANY_WC, MANY_WC - 1)],
         reach=dict(lpk=8, gt=8, iter_keys=128, kps=256, splits=65, stat_rounds_reduce=2, stat_rounds_fold=3, o_rounds=9,
                    fold_w=32, trips=1)),
    dict(id="many_g4", dtype="bf16", B=2, Hq=4, Hkv=1, D=64, ns=4, Wc=MANY_WC,
         states=[(4, MANY_WC, 0), (4, MANY_WC, 10300), (4, MANY_WC, MANY_WC - 1)],
         reach=dict(lpk=8, gt=4, U=8, iter_keys=256, kps=256, splits=65, stat_rounds_reduce=2, stat_rounds_fold=2,
                    o_rounds=9, fold_w=64, trips=1)),
]
# groups: 2 to 5 splits with a partial last split; three full-ring states (the first one's slot lies past split 0), so that
# every kind is aimed at from two KV heads
GROUPS = [
    dict(id="g12_d64", dtype="bf16", B=2, Hq=12, Hkv=1, D=64, ns=4, Wc=700, reach=dict(lpk=8, gt=4, trips=3, splits=3)),
    dict(id="g6_d80", dtype="bf16", B=2, Hq=12, Hkv=2, D=80, ns=4, Wc=900,
         reach=dict(lpk=16, gt=1, trips=6, splits=4, dact_false=6)),
    dict(id="g16_d128", dtype="fp16", B=2, Hq=32, Hkv=2, D=128, ns=4, Wc=600, reach=dict(lpk=16, gt=8, trips=2, splits=3)),
    dict(id="fp32_g3", dtype="fp32", B=2, Hq=3, Hkv=1, D=64, ns=4, Wc=500, reach=dict(lpk=16, gt=1, trips=3, splits=2)),
    dict(id="d256", dtype="bf16", B=2, Hq=4, Hkv=4, D=256, ns=4, Wc=1100, reach=dict(lpk=32, gt=1, splits=5, fold_w=64)),
    dict(id="d16", dtype="fp16", B=2, Hq=8, Hkv=2, D=16, ns=4, Wc=2400, reach=dict(lpk=2, gt=4, splits=3)),
]
for _c in GROUPS:
    _c["states"] = [(_c["ns"], _c["Wc"], 3 * _c["Wc"] // 4), (_c["ns"], _c["Wc"], 0), (_c["ns"], _c["Wc"], _c["Wc"] - 1)]
# fills: device-state forms on a grid of four splits (kps = 256 for every type and group size below); one batch row per
# state, three consecutive steps
FILLS_NS, FILLS_WC, FILLS_KPS, FILLS_STEPS = 4, 1020, 256, 3
FILL_STATES = [
    (2, 0, 0),                                   # sink buffer half filled, empty ring
    (4, 1, 1),                                   # one ring token
    (4, FILLS_KPS - 6, FILLS_KPS - 6),           # keys after the step: kps - 1
    (4, FILLS_KPS - 5, FILLS_KPS - 5),           # kps
    (4, FILLS_KPS - 4, FILLS_KPS - 4),           # kps + 1: the token is the first key of split 1
    (4, FILLS_WC - 1, FILLS_WC - 1),             # one short of full: fills, then wraps
    (4, FILLS_WC, 0),                            # full at write_pos 0
    (4, FILLS_WC, 100),                          # full, slot in split 0
    (4, FILLS_WC, 600),                          # full, slot in split 2
    (4, FILLS_WC, FILLS_WC - 1),                 # full at write_pos Wc - 1: wraps to slot 0
]
FILLS = [dict(id=f"{dt}_d{D}_g{G}", dtype=dt, B=len(FILL_STATES), Hq=2 * G, Hkv=2, D=D, ns=FILLS_NS, Wc=FILLS_WC,
              states=FILL_STATES, reach=dict(splits=4, kps=FILLS_KPS))
         for dt, D in (("bf16", 64), ("fp16", 128), ("fp32", 80)) for G in (1, 8)]


def advance(state, Wc):
    """the state row after one stored token (advance_row)"""
    sl, wl, wp = state
    return (sl, min(wl + 1, Wc), 0 if wp + 1 == Wc else wp + 1)
