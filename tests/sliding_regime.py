"""Which short-window kernel a call reaches, and how that kernel walks: a pure-Python restatement of the short-window
dispatch and launch arithmetic, the way tests/grid_regime.py restates the work-list and ticket grids.  Sources (csrc/):
fwd_mfma, launch_strip_asm_nt, launch_strip and the ring walk of fwd_strip_kernel (sfa_fwd_mfma.hip); launch_bwd,
launch_dq_strip_nt, dkdv_skew and the shell of bwd_dkdv_skew_asm_kernel (sfa_bwd_mfma.hip); the steady / general block
rule of tools/asmgen/fwd_strip.py and dq_strip.py.  strip_asm_nt, asm_window_ok and the constants both files need are
grid_regime's, not copies.  Also the case tables of tests/test_gpu_sliding.py, whose claims tests/test_sliding_regime.py
checks at 256 CUs and the GPU tests check again at the device's own CU count before they run, the probe inputs of every
case, and the raw C-ABI call of a packed batch with poisoned outputs (the sibling of grid_regime.raw_fwd_bwd).

The families
  forward   stripasm_nt{2,3,4}  hand-placed strip bodies: no sink keys, N_q = N_kv, group a multiple of 4, D 64 / 80 / 96,
                                W 1..65 / 66..129 / 130..193.  L = n_qtiles * groups / CUs items per strip (1..n_qtiles); the
                                ring holds NT + 1 tiles, item i of a sequence has a full ring from i = NT - 1 on; an item that
                                is not the first of its strip, whose tiles all exist, takes the STEADY blocks when W = 64 (NT - 1)
                                or one more (65, 129, 193 and 64, 128, 192), else the general ones.
            strip               compiled fwd_strip_kernel<T, D, 8>: every other window up to 256 at D < 128 whose ring fits
                                160 KiB: hpw = gcd(g, 8), BM = 256 / hpw rows per q tile, R = (W + BM + 62) / 64 + 1 ring slots
                                behind TS = ceil(min(ns, Nk) / 64) resident sink tiles, tile t in slot TS + (t - TS) % R.
            nw4 / nw8           fwd_mfma_kernel: where the ring does not fit (and W <= 256 at D < 128 otherwise)
            asm4x64pk           the work-list body: D = 128 or W > 256
  dQ        dqstripasm_nt*      D 64 / 80, the forward's strip conditions, cdiv(N, 64) * (g / 4) * Hkv * B >= 2 CUs, no side stream
            dqasm4x64pk, dq4w   the work list where asm_window_ok, else the compiled 4-wave kernel
  dK/dV     skew                D 64 / 80 / 96, no sink keys, self-attention, 1 <= W <= 512: T = max(6, (62 + W) / 32 + 1) trips
"""
import math

from grid_regime import ASM_MIN_WINDOW, KBA, asm_window_ok, cdiv, strip_asm_nt

STRIP_MAX_WINDOW = 256      # the compiled strip kernel's largest window (SFA_FWD_STRIP_MAXW)
STRIP_LDS_CAP = 160 * 1024  # ... and the LDS its ring + sink tiles may take
STRIP_MIN = 4               # q tiles per strip at least (SFA_FWD_STRIP_MIN)
SKEW_MAX_WINDOW = 512       # kSkewMaxWindow
SKEW_MIN_TRIPS = 6          # SFA_DKDVSK_SKEW


def skew_trips(W, N):
    """trips per q head of the skewed dK/dV sweep (the shell of bwd_dkdv_skew_asm_kernel)"""
    return max((62 + min(W, N)) // 32 + 1, SKEW_MIN_TRIPS)


def strip_geometry(g, D, Nk, ns, Wc):
    """hpw, BM, R, TS, LDS bytes of the compiled strip kernel (fwd_mfma's short-window branch); Wc: W clamped to N_kv"""
    hpw = math.gcd(g, 8)
    BM = 32 * (8 // hpw)
    slot = 2 * 64 * (128 if D <= 64 else 256)
    R = (Wc + BM - 1 + 63) // 64 + 1
    TS = (min(ns, Nk) + 63) // 64
    return hpw, BM, R, TS, (R + TS) * slot


def strip_walk(N, P, W, BM, R, TS, strip):
    """The ring walk of fwd_strip_kernel over one sequence of N rows (P = N_kv - N_q; W as the kernel clamps it), strip by
    strip.  Per strip: tiles = [ring_lo, ring_hi) of each q tile, loads = the window tiles in the order they enter the
    ring, overwrites = loads into a slot that already held a tile of this strip, extra = tiles a q tile after the first
    had to fetch itself (beyond the one its predecessor prefetched), resident_ok = no load ever replaced a tile the q tile
    about to run still needs, resident = the most tiles one q tile reads (R of them only where the q tile's first key is not
    tile-aligned: N_q < N_kv with N_kv - N_q no multiple of 64; with aligned q tiles a ring of R - 1 slots would do)."""
    W = min(W, N + P)
    n_qtiles = cdiv(N, BM)

    def lo_of(q0):
        return max(max(q0 + P - W + 1, 0) >> 6, TS)

    def hi_of(q0):
        return (min(q0 + BM, N) + P + 63) >> 6

    out = []
    for qt0 in range(0, n_qtiles, strip):
        held, loads, over, extra, ok, tiles = {}, [], 0, 0, True, []

        def put(t, need_lo):
            nonlocal over, ok
            s = (t - TS) % R
            if s in held:
                over += 1
                ok = ok and held[s] < need_lo          # (the replaced tile is older than anything still needed)
            held[s] = t
            loads.append(t)

        nxt = lo_of(qt0 * BM)
        for t in range(nxt, max(hi_of(qt0 * BM), nxt)):
            put(t, nxt)
        nxt = max(hi_of(qt0 * BM), nxt)
        for qi in range(min(strip, n_qtiles - qt0)):
            q0 = (qt0 + qi) * BM
            lo, hi = lo_of(q0), hi_of(q0)
            nxt = max(nxt, lo)
            while nxt < hi:
                put(nxt, lo)
                extra += 1
                nxt += 1
            ok = ok and all(held.get((t - TS) % R) == t for t in range(lo, hi))
            tiles.append((lo, hi))
            if qi + 1 < strip and q0 + BM < N and nxt < hi_of(q0 + BM):     # the prefetch, written behind the q tile's reads
                put(nxt, lo_of(q0 + BM))
                nxt += 1
        out.append(dict(q_tiles=len(tiles), tiles=tiles, loads=loads, overwrites=over, extra=extra, resident_ok=ok,
                        resident=max(hi - lo for lo, hi in tiles)))
    return out


def regime(B, Hq, Hkv, Nq, Nk, D, ns, W, n_cu, lens=None):
    """The kernels sfa_fwd + sfa_bwd (16-bit dtypes, the library's own dK/dV rule, SFA_FLAG_BWD_OVERLAP passed) reach on a
    device of n_cu CUs, and their launch figures.  lens: the sequence lengths of a packed batch (B, Nq and Nk are then
    taken from them: the launch problem is len(lens) sequences of the longest one's length)."""
    packed = lens is not None
    if packed:
        B, Nq = len(lens), max(lens)
        Nk = Nq
    lens_ = list(lens) if packed else [Nq] * B
    g, P = Hq // Hkv, Nk - Nq
    Wc = min(max(W, 0), Nk)                                 # the window as the launchers clamp it
    nt = strip_asm_nt(W)                                    # (the caller's window: a short sequence takes the pack's body)
    strip_ok = ns <= 0 and Nk == Nq and g % 4 == 0 and nt > 0
    r = dict(g=g, P=P, Wc=Wc, NT=nt if strip_ok else 0)
    # ---- forward
    fits = None
    if strip_ok and D in (64, 80, 96):
        fwd, why = "stripasm_nt%d" % nt, "no sink keys, N_q = N_kv, group %d, D %d, W %d: %d tiles per item" % (g, D, W, nt)
    else:
        fwd = None
        if 0 < W <= STRIP_MAX_WINDOW and D < 128:
            hpw, BM, R, TS, lds = strip_geometry(g, D, Nk, ns, Wc)
            fits = lds <= STRIP_LDS_CAP
            r.update(hpw=hpw, BM=BM, R=R, TS=TS, lds=lds, fits=fits)
            if fits:
                fwd, why = "strip", "W %d <= 256, ring of %d + %d sink tiles: %d bytes of LDS" % (W, R, TS, lds)
        if fwd is None:
            if (D == 128 or Wc > ASM_MIN_WINDOW) and (Wc > 0 or ns > 0) and D in (64, 80, 96, 128):
                fwd, why = "asm4x64pk", "D = 128 or W %d > 256" % Wc
            else:
                fwd = "nw%d" % (4 if (0 <= W <= 2048 or D == 256) else 8)
                why = "ring over 160 KiB" if fits is False else "W = 0 or a head dim without a hand-placed body"
    r.update(fwd=fwd, fwd_why=why)
    if fwd.startswith("stripasm") or (strip_ok and D in (64, 80)):
        n_qtiles, groups = cdiv(Nq, 64), (g // 4) * Hkv * B
        L = min(max(n_qtiles * groups // n_cu, 1), n_qtiles)
        n_strips = cdiv(n_qtiles, L)
        seq_tiles = [cdiv(n, 64) for n in lens_]
        steady_w = W - 64 * (nt - 1) in (0, 1)
        # an item's place in its strip and in its sequence decide its blocks: i % L = 0 the strip's head (general blocks,
        # cold start), else steady blocks when its first tile i - (NT - 1) exists and W allows them
        r.update(L=L, n_strips=n_strips, last_strip_items=n_qtiles - (n_strips - 1) * L,
                 full_ring_items=max(n_qtiles - (nt - 1), 0), steady_w=steady_w,
                 steady_items=sum(1 for i in range(n_qtiles) if steady_w and i % L and i >= nt - 1),
                 exited_blocks=sum(n_strips - cdiv(t, L) for t in seq_tiles),
                 shorter_than_window=sorted(n for n in lens_ if 0 < n < W), one_row_sequence=1 in lens_)
    if fwd == "strip":
        hpw, BM, R, TS = r["hpw"], r["BM"], r["R"], r["TS"]
        n_qtiles, base = cdiv(Nq, BM), (g // hpw) * Hkv * B
        per_seq = 1 if base >= n_cu else n_cu // base
        strip = min(max(cdiv(n_qtiles, per_seq), STRIP_MIN), n_qtiles)
        walks = [strip_walk(n, P, Wc, BM, R, TS, strip) for n in sorted(set(lens_)) if n > 0]
        flat = [s for w in walks for s in w]
        r.update(hgroups=g // hpw, strip=strip, n_strips=cdiv(n_qtiles, strip), walk=strip_walk(Nq, P, Wc, BM, R, TS, strip),
                 overwrites=max(s["overwrites"] for s in flat), multi_load=any(s["extra"] > 0 for s in flat),
                 resident_ok=all(s["resident_ok"] for s in flat), max_resident=max(s["resident"] for s in flat), shortest_strip=min(s["q_tiles"] for s in flat),
                 whole_sequence=strip == n_qtiles, shorter_than_bm=sorted(n for n in lens_ if 0 < n < BM),
                 sink_tile_holds_window_keys=ns % 64 != 0 and ns < Nk)
    # ---- dQ
    hpw4 = 4 if g % 4 == 0 else (2 if g % 2 == 0 else 1)
    wgs = cdiv(Nk, KBA) * Hkv * B
    list_ok = D in (64, 80, 96, 128) and asm_window_ok(D, Wc, wgs, n_cu) and (Wc > 0 or ns > 0)
    items = cdiv(Nq, 64 * (4 // hpw4)) * (g // hpw4) * Hkv * B
    side = items < 4 * n_cu and list_ok
    strip_items = cdiv(Nq, 64) * (g // 4) * Hkv * B if g % 4 == 0 else 0
    if D in (64, 80) and not side and strip_ok and strip_items >= 2 * n_cu:
        dq = "dqstripasm_nt%d" % nt
    elif list_ok:
        dq = "dqasm4x64pk_hpw%d" % hpw4
    else:
        dq = "dq4w" if Wc <= 2048 else "dq8w"
    r.update(dq=dq, dq_side_stream=side and dq.startswith("dqasm"), strip_items=strip_items)
    # ---- dK/dV
    skew = D in (64, 80, 96) and ns <= 0 and (packed or Nq == Nk) and 1 <= Wc <= SKEW_MAX_WINDOW
    r.update(skew=skew, T=skew_trips(Wc, Nq) if skew else None, key_blocks=cdiv(Nk, KBA), last_block_keys=Nk - (cdiv(Nk, KBA) - 1) * KBA,
             T_seq=[skew_trips(Wc, n) for n in lens_ if n > 0] if skew else None)
    return r


# ------------------------------------------------------------------------------------------------ case tables
# One dict per case: B, Hq, Hkv, Nq, Nk, D, ns, W, dtype, aux (s_aux given), layout ("bnhd": [B, N, H, D] storage), lens (a
# packed batch), probe_B (the probe inputs are built for that many batch elements - all different - and repeated along the
# batch, so that the fp64 reference of the large shapes is computed for two batch elements, not sixteen), missing (the probe
# kinds the shape excludes by construction) and claims: what regime() must return for the case to count.  A claim is a
# value (equality) or ("ge", n).
N_EDGE = 333        # 6 tiles, the last of 13 rows: with NT = 4 three items run on a full ring
N_WHOLE = 461       # 8 tiles, the last of 13 rows
N_SKEW = 781        # 4 key blocks, the last of 13 keys
_NO_SINK = ("sink_last", "sink_next")
_NO_WINDOW = ("win_oldest", "win_behind", "sink_last", "sink_next")
DTYPES = ("bf16", "fp16")
# cases kept for path coverage only (none: with s_aux at the target's logit and dO x 4 the rows of one or two keys reach the
# margin as well, tests/test_sliding_regime.py::test_tiny_windows_reach_the_margin)
PATH_ONLY = ()
AUX_AT_LOGIT_MAX_W = 2      # windows up to this get s_aux at the target's logit (case_probe)


def _mk(table, cid, B, Hq, Hkv, Nq, D, ns, W, dtype, claims, Nk=None, aux=True, layout=None, lens=None, probe_B=None,
        missing=None):
    if missing is None:
        missing = (_NO_SINK if ns == 0 else ()) + (("win_oldest", "win_behind") if W >= max(lens or [Nq]) else ())
        if lens and ns == 0:
            missing += ("pack_sink",)
    table[cid] = dict(id=cid, B=B, Hq=Hq, Hkv=Hkv, Nq=Nq, Nk=Nq if Nk is None else Nk, D=D, ns=ns, W=W, dtype=dtype, aux=aux,
                      layout=layout, lens=lens, probe_B=min(probe_B or B, B), missing=tuple(missing), claims=claims)


EDGES, WHOLE, RAGGED, PACK, SKEW, RING = {}, {}, {}, {}, {}, {}

# a. every strip body at the smallest and the largest window of its class, L = 1 (every item a cold start).  s_aux is not
# tied to the window: each window runs with it at three of the six (D, dtype) pairs and without it at the other three -
# except W = 1 and 2, which always carry it (without s_aux the one key of a row holds p = 1 and dQ, dK are identically 0)
for _p, (_D, _dt) in enumerate((D, dt) for D in (64, 80, 96) for dt in DTYPES):
    for _w, _W in enumerate((1, 65, 66, 129, 130, 193)):
        _mk(EDGES, "edges_d%d_%s_w%d" % (_D, _dt, _W), 1, 4, 1, N_EDGE, _D, 0, _W, _dt, aux=_W == 1 or (_p + _w) % 2 == 0,
            claims=dict(fwd="stripasm_nt%d" % strip_asm_nt(_W), L=1, n_strips=6, full_ring_items=("ge", 2), dq="dq4w",
                        skew=True))
for _W in (2, 64):
    _mk(EDGES, "edges_d64_bf16_w%d" % _W, 1, 4, 1, N_EDGE, 64, 0, _W, "bf16",
        claims=dict(fwd="stripasm_nt2", L=1, steady_w=_W == 64, dq="dq4w"))
# W = 194: the first window the hand-placed bodies do not serve - the compiled strip kernel at D = 64, the LDS fallback above
_mk(EDGES, "edges_d64_bf16_w194", 1, 4, 1, N_EDGE, 64, 0, 194, "bf16", dict(fwd="strip", NT=0, R=6, fits=True, hpw=4))
_mk(EDGES, "edges_d80_fp16_w194", 1, 4, 1, N_EDGE, 80, 0, 194, "fp16", dict(fwd="nw4", NT=0, R=6, fits=False), aux=False)
_mk(EDGES, "edges_d96_bf16_w194", 1, 4, 1, N_EDGE, 96, 0, 194, "bf16", dict(fwd="nw4", NT=0, R=6, fits=False))

# b. one strip per sequence: 256 groups on 256 CUs, L = n_qtiles; the grid fills the chip twice, so dQ takes its strip body
_n = 0
for _D, _dt in ((64, "bf16"), (80, "fp16")):
    for _W in (65, 129, 193):
        _n += 1
        _mk(WHOLE, "whole_d%d_%s_w%d" % (_D, _dt, _W), 16, 64, 16, N_WHOLE, _D, 0, _W, _dt, probe_B=2, aux=_n % 2 == 1,
            claims=dict(fwd="stripasm_nt%d" % strip_asm_nt(_W), L=8, n_strips=1, steady_w=True, steady_items=("ge", 4),
                        dq="dqstripasm_nt%d" % strip_asm_nt(_W), strip_items=2048, dq_side_stream=False, skew=True))
_mk(WHOLE, "whole_d96_bf16_w193", 16, 64, 16, N_WHOLE, 96, 0, 193, "bf16", probe_B=2,
    claims=dict(fwd="stripasm_nt4", L=8, n_strips=1, steady_items=("ge", 4), dq="dqasm4x64pk_hpw4", dq_side_stream=False))

# c. 192 groups: strips of 6 items and a last strip of 2 (L = 8 * 192 / 256), [B, N, H, D] storage; W = 33 beside the two
# class edges so that the NT = 2 dQ bodies of (D 80, bf16) and (D 64, fp16) run as well: 12 of 12 with table b
for _D, _dt in ((80, "bf16"), (64, "fp16")):
    for _W in (33, 66, 130):
        _mk(RAGGED, "ragged_d%d_%s_w%d" % (_D, _dt, _W), 12, 64, 16, N_WHOLE, _D, 0, _W, _dt, probe_B=2, layout="bnhd",
            aux=_W == 66,
            claims=dict(fwd="stripasm_nt%d" % strip_asm_nt(_W), L=6, n_strips=2, last_strip_items=2, steady_w=False,
                        dq="dqstripasm_nt%d" % strip_asm_nt(_W), skew=True))

# d. a packed call: sequences of one row, of less than a tile, of exactly a tile, of a tile and a row, shorter than the
# window of an NT = 4 body, and the long one that sizes the grid
PACK_LENS = (1, 63, 64, 65, 200, 461)
for _D, _dt in ((64, "bf16"), (96, "fp16")):
    for _W in (193, 65):
        _mk(PACK, "pack_d%d_%s_w%d" % (_D, _dt, _W), 1, 16, 2, sum(PACK_LENS), _D, 0, _W, _dt, lens=PACK_LENS,
            claims=dict(fwd="stripasm_nt%d" % strip_asm_nt(_W), L=1, n_strips=8, exited_blocks=("ge", 24), one_row_sequence=True,
                        shorter_than_window=[1, 63, 64, 65] if _W == 193 else [1, 63, 64], dq="dq4w", skew=True))

# e. the skewed dK/dV sweep; group 3, so that no strip body runs.  Both sides of the T steps 129|130, 161|162, 257|258,
# 481|482 and of the dispatch edge 512|513 at EVERY head dim (the step is taken in the shell, but each side then runs in
# the same body); the T values between them (9, 12 .. 16) at one window and one head dim each
_SKEW_STEPS = (129, 130, 161, 162, 257, 258, 481, 482, 512, 513)
_SKEW_FILL = (194, 321, 322, 385, 386, 449)
_i = 0
for _W in _SKEW_STEPS + _SKEW_FILL:
    for _D in ((64, 80, 96) if _W in _SKEW_STEPS else ((64, 80, 96)[_i % 3],)):
        _i += 1
        _dt = DTYPES[(_i // 2) % 2]
        if _W > SKEW_MAX_WINDOW:
            _mk(SKEW, "skew_d%d_%s_w%d" % (_D, _dt, _W), 1, 6, 2, N_SKEW, _D, 0, _W, _dt, dict(skew=False, T=None, fwd="asm4x64pk"))
        else:
            _mk(SKEW, "skew_d%d_%s_w%d" % (_D, _dt, _W), 1, 6, 2, N_SKEW, _D, 0, _W, _dt, aux=_i % 3 != 0,
                claims=dict(skew=True, T=(62 + _W) // 32 + 1, key_blocks=4, last_block_keys=13, NT=0))
_mk(SKEW, "skew_mha_d80_fp16_w130", 1, 2, 2, N_SKEW, 80, 0, 130, "fp16", dict(skew=True, T=7, g=1, NT=0))
_mk(SKEW, "skew_n_lt_w_d96_bf16", 1, 6, 2, 333, 96, 0, 400, "bf16", dict(skew=True, T=13, Wc=333, key_blocks=2))

# f. the compiled strip kernel: every hpw, 0..3 resident sink tiles, ring slots reused at least twice inside a strip
_ring = dict(fwd="strip", fits=True, resident_ok=True, overwrites=("ge", 2))
_mk(RING, "ring_hpw1_g3_w255", 1, 6, 2, N_SKEW, 64, 0, 255, "bf16", dict(_ring, hpw=1, BM=256, R=9, TS=0, multi_load=True))
_mk(RING, "ring_hpw2_g2_ns65_w64", 1, 4, 2, 589, 64, 65, 64, "fp16",
    dict(_ring, hpw=2, BM=128, R=4, TS=2, shortest_strip=1, sink_tile_holds_window_keys=True))
_mk(RING, "ring_hpw4_g4_ns1_w63", 2, 8, 2, N_WHOLE, 80, 1, 63, "fp16", dict(_ring, hpw=4, BM=64, R=3, TS=1))
_mk(RING, "ring_hpw8_g8_ns64_w65", 8, 128, 16, N_WHOLE, 96, 64, 65, "bf16", dict(_ring, hpw=8, BM=32, R=3, TS=1, strip=8),
    probe_B=2)
_mk(RING, "ring_hgroups2_g16_ns130_w1", 8, 128, 8, N_WHOLE, 64, 130, 1, "bf16",
    dict(_ring, hpw=8, hgroups=2, R=2, TS=3, strip=8), probe_B=2)
_mk(RING, "ring_whole_d32_w256", 16, 128, 16, N_WHOLE, 32, 0, 256, "bf16", dict(_ring, hpw=8, R=6, whole_sequence=True, strip=15),
    probe_B=2)
_mk(RING, "ring_nq_lt_nk_w194", 1, 4, 2, 525, 64, 0, 194, "bf16", dict(_ring, hpw=2, R=7, P=256, dq="dq4w"), Nk=N_SKEW)
# N_kv - N_q = 1: the q tiles' first keys are not tile-aligned, and only then does a q tile read as many tiles as the ring has
# slots (every other case would pass on a ring of R - 1, profiles/sliding_mutants.log)
_mk(RING, "ring_unaligned_p1_w200", 1, 4, 2, 525, 64, 0, 200, "fp16", dict(_ring, hpw=2, R=7, P=1, max_resident=7), Nk=526)
_mk(RING, "ring_pack_g3_w256", 1, 6, 2, 100 + N_SKEW + 300, 64, 0, 256, "bf16", lens=(100, N_SKEW, 300),
    claims=dict(_ring, hpw=1, R=9, shorter_than_bm=[100], skew=True))
# the LDS cap: one window key more and the ring is a slot too long (group 4 with one sink tile at D = 80: 4 + 1 slots of 32 KiB)
_mk(RING, "ring_cap_fits_w129", 1, 8, 2, N_WHOLE, 80, 1, 129, "bf16", dict(_ring, hpw=4, R=4, TS=1, lds=STRIP_LDS_CAP))
_mk(RING, "ring_cap_over_w130", 1, 8, 2, N_WHOLE, 80, 1, 130, "bf16", dict(fwd="nw4", fits=False, R=5, TS=1))
_mk(RING, "ring_d64_w257", 1, 6, 2, N_SKEW, 64, 0, 257, "bf16", dict(fwd="asm4x64pk", fits=None, skew=True, T=10))
LDS_CAP_PAIR = ("ring_cap_fits_w129", "ring_cap_over_w130")

TABLES = dict(edges=EDGES, whole=WHOLE, ragged_strips=RAGGED, pack=PACK, skew=SKEW, ring=RING)
CASES = {cid: c for t in TABLES.values() for cid, c in t.items()}
# the subset the mutant proofs of tests/test_sliding_regime.py run on: one case per table
PROOF_CASES = ("edges_d80_bf16_w129", "whole_d64_bf16_w65", "ragged_d64_fp16_w130", "pack_d64_bf16_w193", "skew_d64_fp16_w162",
               "ring_hpw4_g4_ns1_w63")
# a window from this list makes tools/fuzz.py --inputs=probe land on a class edge of the short-window kernels
EDGE_WINDOWS = (1, 2, 64, 65, 66, 128, 129, 130, 161, 162, 192, 193, 194, 256, 257, 258, 481, 482, 512, 513)


def case_regime(cid, n_cu):
    """regime() of a case, and the list of claims it misses (empty: the case reaches its regime)"""
    c = CASES[cid]
    r = regime(c["B"], c["Hq"], c["Hkv"], c["Nq"], c["Nk"], c["D"], c["ns"], c["W"], n_cu, lens=c["lens"])
    missed = []
    for k, want in c["claims"].items():
        got = r.get(k)
        ok = (got is not None and got >= want[1]) if isinstance(want, tuple) and want[0] == "ge" else got == want
        if not ok:
            missed.append("%s at %d CUs: %s = %r, the case needs %r" % (cid, n_cu, k, got, want))
    return r, missed


def case_cu(c):
    """cu_seqlens of a packed case (None: dense)"""
    if not c["lens"]:
        return None
    cu = [0]
    for n in c["lens"]:
        cu.append(cu[-1] + n)
    return cu


def case_probe(c):
    """the probe inputs of a case (tests/probe_inputs.py::dense_probe) for its first probe_B batch elements; the GPU test
    repeats them along the batch, the CPU test counts their kinds and proves the mutants on them"""
    import probe_inputs as P
    import torch
    dt = dict(bf16=torch.bfloat16, fp16=torch.float16)[c["dtype"]]
    seed = 9000 + sorted(CASES).index(c["id"])
    pr = P.dense_probe(c["probe_B"], c["Hq"], c["Hkv"], c["Nq"], c["Nk"], c["D"], c["ns"], c["W"], dt, seed, aux=c["aux"],
                       cu=case_cu(c))
    if c["aux"] and c["ns"] == 0 and c["W"] <= AUX_AT_LOGIT_MAX_W:
        # a row of one or two keys: s_aux at the target's logit a sqrt(D) (+ 0.25 randn, as the decode probes), so that the
        # target holds about half of the softmax mass and dS = p (1 - p) dP of the row is as large as it can be
        g = torch.Generator().manual_seed(seed + 1)
        pr["s_aux"] = pr["a"] * c["D"] ** 0.5 + 0.25 * torch.randn(c["Hq"], generator=g, dtype=torch.float32)
        # ... and dO four times as large (exact in both dtypes): a dropped key moves dQ of such a row by |dQ| itself, that is
        # by 20 |dQ| / (1 + |dQ|) dQ tolerances, which passes 10 only where |dQ| > 1
        pr["do"] = pr["do"] * 4
    return pr


def raw_fwd_bwd(q, k, v, do, s_aux, ns, W, flags, cu=None):
    """sfa_fwd then sfa_bwd (cu given: sfa_fwd_varlen / sfa_bwd_varlen on a pack [1, H, T, D]) through the C ABI, O, LSE, dQ,
    dK, dV and ds_aux NaN-filled and every byte of the workspace 0xFF-filled first: the sibling of grid_regime.raw_fwd_bwd
    that also takes a pack, strided views and a call without s_aux.  cu: the host list.  LSE comes back as [B, Hq, N]
    (a pack: [1, Hq, T]).  Returns the outputs, the workspace and sfa_last_path() of both calls."""
    import torch
    from sink_attention import _native as N
    lib = N.lib()
    B, Hq, Nq, D = q.shape
    Hkv = k.shape[1]
    scale = D ** -0.5
    nan = lambda shape, dt: torch.full(shape, float("nan"), device=q.device, dtype=dt)
    out = dict(o=nan(q.shape, q.dtype), lse=nan((B, Hq, Nq), torch.float32), dq=nan(q.shape, q.dtype), dk=nan(k.shape, k.dtype),
               dv=nan(v.shape, v.dtype), ds_aux=nan((Hq,), torch.float32) if s_aux is not None else None)
    n_ws = int(lib.sfa_bwd_workspace_bytes(B, Hq, Hkv, Nq, D, N.SFA_DTYPE[q.dtype], ns, W, flags))
    out["ws"] = torch.full((max(n_ws, 256),), 0xFF, dtype=torch.uint8, device=q.device)
    sa = None if s_aux is None else s_aux.data_ptr()
    dsa = None if s_aux is None else out["ds_aux"].data_ptr()
    stream = N.stream_ptr(q.device)
    d = [N.desc(x) for x in (q, k, v, out["o"], do, out["dq"], out["dk"], out["dv"])]
    if cu is None:
        N.check(lib.sfa_fwd(d[0], d[1], d[2], d[3], out["lse"].data_ptr(), sa, ns, W, scale, 0, stream), "sfa_fwd")
        out["fwd_path"] = N.last_path()
        N.check(lib.sfa_bwd(d[0], d[1], d[2], d[3], d[4], out["lse"].data_ptr(), sa, d[5], d[6], d[7], dsa, out["ws"].data_ptr(),
                            out["ws"].numel(), ns, W, scale, flags, stream), "sfa_bwd")
    else:
        cu_dev = torch.tensor(cu, dtype=torch.int32, device=q.device)
        longest = max(b - a for a, b in zip(cu[:-1], cu[1:]))
        N.check(lib.sfa_fwd_varlen(d[0], d[1], d[2], d[3], out["lse"].data_ptr(), sa, cu_dev.data_ptr(), len(cu) - 1, longest,
                                   ns, W, scale, 0, stream), "sfa_fwd_varlen")
        out["fwd_path"] = N.last_path()
        N.check(lib.sfa_bwd_varlen(d[0], d[1], d[2], d[3], d[4], out["lse"].data_ptr(), sa, d[5], d[6], d[7], dsa,
                                   cu_dev.data_ptr(), len(cu) - 1, longest, out["ws"].data_ptr(), out["ws"].numel(), ns, W,
                                   scale, flags, stream), "sfa_bwd_varlen")
    out["bwd_path"] = N.last_path()
    return out
