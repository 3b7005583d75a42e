"""Softmax-range inputs: q / k whose logits climb, fall or sit far from zero along the key index, so that the online softmax
of the forward kernels has to MOVE its reference point with a rescale factor whose value matters, and an fp64 model of that
walk.  Plain torch on the CPU; imports neither the product nor a GPU.  tests/test_range_inputs.py proves on the CPU that
these inputs take the deferred rescale with a mid-range alpha, that randn inputs never do, that every mutant of the rescale
moves O by ten tolerances and that the tolerances of tests/test_gpu_softmax_range.py leave room for a correct kernel.

Construction (everything from a seeded CPU generator, rounded to the dtype before anyone uses it)
  * u: one +-1 code of length D per (batch, KV head).  k_j = n_j + beta_j u and q_i = n_i + a_i u, n = randn with its
    component along u removed, so the scaled logit of (i, j) is N(0, 1) + a_i beta_j sqrt(D): a common shift of
    a_i H_j nat with beta_j = H_j / sqrt(D).  v and dO are plain randn: the output tolerances keep their meaning.
  * row gains a_i: GAINS[(i + head) % 4] = 0 / 1 / 0 / 0.5, zeroed where i % 3 == 0 and on the GUARD rows behind a step.  Every
    32-row block and every 64-row wave holds rows that move beside rows that do not; rows with a_i = 0 are the randn controls.
  * staircase_up    H starts at 0 and rises along the key index in steps of STEPS nat = (0.6, 0.75, 0.9) sqrt(128) = 6.8 / 8.5 /
                    10.2 nat, i.e. 9.8 / 12.2 / 14.7 log2 units at a = 1 and 4.9 / 6.1 / 7.3 at a = 0.5: single steps on both sides
                    of the 2^8 rule, pairs of small steps that cross it together, every crossing inside 2^-16 <= alpha < 2^-8
                    (steps of 0.5 and 1.0 sqrt(128) sit ON the two ends of that range and the randn part decides).  Steps
                    sit inside the sink keys, right after the last sink key, on the first key of a 64-key tile, inside a tile
                    and on the last key of a tile (step_keys); the rows behind a step meet it in their diagonal tile.
                    fp32: a sawtooth of three steps (heights).
  * staircase_down  the mirror image, centred: the highest level in the sink keys (the oldest keys where num_sink = 0), SINK_TOP nat
                    above the next level, then falling.  The reference never moves; later p underflow (a = 1: more than
                    126 log2 units below the reference) and rows beyond the window see a window that is negligible beside
                    the sinks.
  * offset          every key carries H = OFFSET nat and the gains are +1 / -1 / 0 / 0.5: all logits of a row shift together,
                    the softmax over the keys is unchanged, the weight of s_aux goes to 0 or to 1 (l ~ 1, O ~ 0).
  * aux_sweep       randn q / k; s_aux[h] = AUX_SWEEP[h % 5] = -40 / -8 / 0 / +8 / +40 nat, so the heads of one workgroup
                    differ.  -8: the first tile moves a seeded reference with a mid-range alpha; +8: the sink logit holds
                    most of the mass and ds_aux is O(1); +40: nothing ever moves.
  The other families carry the usual s_aux = 0.5 randn.

Model (tile_walk): the forward as csrc/sfa_fwd_mfma.hip and tools/asmgen/fwd.py walk it - 64-key tiles in ascending order
(sink tiles [0, ts_hi), then window tiles from tw_lo >= ts_hi: `tile_of` of fwd_mfma_kernel, F_ts_hi / F_tw_off of the work
lists, sink slots then ring slots of the strip kernels; a tile without a visible key leaves a row untouched), log2 domain,
reference seeded with s_aux log2(e) and l = 1, moved only when the tile maximum is more than THR = 8 above it or when there
was none (then alpha = 1: inf_no_rescale).  It returns O, LSE and the (row, tile, alpha) events and takes the MUTANTS of the
rescale.  precision_fwd / precision_bwd are the same walk with S accumulated in f32, P rounded to the dtype before the PV
and row-sum products and O rounded at the end; the backward takes delta from the rounded O and rounds P and dS.

Amplitudes as shipped (tests/test_range_inputs.py prints the figures; its docstring lists them): STEPS, SINK_TOP = 48,
OFFSET = 60 for the 16-bit dtypes; FP32_SCALE = 1/4 scales staircase_down and offset for fp32 inputs.
"""
import math

import torch

from oracle import sink_oracle as O

TILE = 64
THR = 8.0
LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
GAINS = (0.0, 1.0, 0.0, 0.5)
OFFSET_GAINS = (1.0, -1.0, 0.0, 0.5)
STEPS = tuple(x * math.sqrt(128.0) for x in (0.6, 0.75, 0.9))      # nat at a = 1
GUARD = 4               # rows j .. j + GUARD - 1 behind a step at key j are controls (see gains)
FP32_PERIOD = 3         # fp32 staircase_up: back to 0 after every third step (see heights)
SINK_TOP = 48.0
OFFSET = 60.0
AUX_SWEEP = (-40.0, -8.0, 0.0, 8.0, 40.0)
FP32_SCALE = 0.25
FAMILIES = ("staircase_up", "staircase_down", "offset", "aux_sweep")
MUTANTS = ("alpha0", "neighbour", "row32", "wave_bcast", "skip_o_block", "skip_l", "skip_aux_unit", "never_fp16")
DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}


def _rand(shape, g, dtype=torch.float32, scale=1.0):
    return (torch.randn(*shape, generator=g, dtype=torch.float32) * scale).to(dtype)


# ------------------------------------------------------------------------------------------------ the families
def step_keys(Nk, ns, W):
    """Keys at which a staircase steps: inside the sink keys, right after the last one, then (long windows) the first key
    of a tile, inside a tile, the last key of a tile ...; short windows take one step per tile, cycling through the same
    three places, so that the window of a late row holds one or two."""
    keys = []
    if ns >= 3:
        keys.append(ns // 2)
    if ns >= 1:
        keys.append(ns)
    if W > 256:
        keys += [64, 100, 191, 256, 330, 448, 520, 640, 700, 832, 900, 1023, 1088, 1200]
    else:
        keys += [TILE * t + (0, 36, 63)[t % 3] for t in range(1, Nk // TILE + 1)]
    return sorted(set(x for x in keys if 0 < x < Nk))


def heights(family, Nk, ns, W, scale=1.0, period=0):
    """H_j [Nk] in nat (the logit shift of key j for a row of gain 1).  period > 0 (fp32 staircase_up): a sawtooth, the level
    falls back to 0 with every period-th step, so that no logit exceeds three steps (an f32 dot product of 90 nat is
    exact to 1e-5 only, the whole fp32 tolerance); a fall never moves a reference, the climb behind it does again."""
    H = torch.zeros(Nk, dtype=torch.float64)
    if family == "offset":
        return H + OFFSET * scale
    if family == "aux_sweep":
        return H
    for n, x in enumerate(step_keys(Nk, ns, W)):
        if period and family == "staircase_up" and n % period == 0 and n > 0:
            H[x:] = 0.0
        else:
            H[x:] += STEPS[n % 3]
    if family == "staircase_down":
        H = -H
        top = ns if ns >= 1 else min(8, Nk)
        H[:top] += SINK_TOP
        H = H - (H.max() + H.min()) / 2
    # (staircase_up starts at 0: centred, the first levels would lie far below the s_aux seed and the early rows would
    # never leave it)
    return H * scale


def gains(family, Hq, Nq, P=0, steps=()):
    """a [Hq, Nq]; P: position of row 0 among the keys; steps: the staircase's step keys.  The GUARD rows right behind a step
    are controls: a row that sees fewer than GUARD keys on its top level is one-hot, and the LSE of a one-hot row carries
    the whole rounding error of ONE p (2^-8 in bf16, 0.78 of the LSE bound) whichever kernel computes it."""
    i = torch.arange(Nq).view(1, Nq)
    h = torch.arange(Hq).view(Hq, 1)
    if family == "aux_sweep":
        return torch.zeros(Hq, Nq, dtype=torch.float64)
    table = torch.tensor(OFFSET_GAINS if family == "offset" else GAINS, dtype=torch.float64)
    a = table[(i + h) % 4]
    zero = i % 3 == 0
    for x in steps:
        zero = zero | ((i + P >= x) & (i + P < x + GUARD))
    return torch.where(zero.expand_as(a), torch.zeros_like(a), a)


def _perp(x, u):
    """x without its component along u (u: [..., 1, D], +-1)"""
    D = x.shape[-1]
    return x - (x * u).sum(-1, keepdim=True) / D * u


def dense_range(family, B, Hq, Hkv, Nq, Nk, D, ns, W, dtype, seed, cu=None, scale=None):
    """One dense call (or one pack: cu given, every sequence of the pack from its second on carries the family,
    the first is randn).  Returns a dict: q [B,Hq,Nq,D], k / v [B,Hkv,Nk,D], do, s_aux [Hq] f32, H [Nk], a [Hq,Nq]."""
    assert family in FAMILIES
    scale = (FP32_SCALE if dtype == torch.float32 else 1.0) if scale is None else scale
    g = torch.Generator().manual_seed(seed)
    grp = Hq // Hkv
    u = (torch.randint(0, 2, (B, Hkv, 1, D), generator=g).double() * 2 - 1)
    nq = torch.randn(B, Hq, Nq, D, generator=g, dtype=torch.float32).double()
    nk = torch.randn(B, Hkv, Nk, D, generator=g, dtype=torch.float32).double()
    v = _rand((B, Hkv, Nk, D), g, dtype)
    do = _rand((B, Hq, Nq, D), g, dtype)
    sa = _rand((Hq,), g, torch.float32, 0.5)
    if family == "aux_sweep":
        sa = torch.tensor([AUX_SWEEP[h % len(AUX_SWEEP)] for h in range(Hq)], dtype=torch.float32)
    period = FP32_PERIOD if dtype == torch.float32 else 0
    if family == "staircase_up":
        scale = 1.0               # (fp32: the sawtooth bounds the logits instead)
    st = lambda n: step_keys(n, ns, W) if family.startswith("staircase") else ()
    if cu is None:
        H, a = heights(family, Nk, ns, W, scale, period), gains(family, Hq, Nq, Nk - Nq, st(Nk))
    else:
        assert Nq == Nk == cu[-1]
        H, a = torch.zeros(Nk, dtype=torch.float64), torch.zeros(Hq, Nq, dtype=torch.float64)
        for s, (x, y) in enumerate(zip(cu[:-1], cu[1:])):
            if s >= 1 and y > x:
                H[x:y], a[:, x:y] = heights(family, y - x, ns, W, scale, period), gains(family, Hq, y - x, 0, st(y - x))
    uq = u.repeat_interleave(grp, dim=1)
    if family == "aux_sweep":
        q, k = nq, nk
    else:
        q = _perp(nq, uq) + a.view(1, Hq, Nq, 1) * uq
        k = _perp(nk, u) + (H / math.sqrt(D)).view(1, 1, Nk, 1) * u
    return dict(q=q.to(dtype), k=k.to(dtype), v=v, do=do, s_aux=sa, H=H, a=a, family=family)


def randn_like(inp, seed, aux=True):
    """the suite's randn inputs (tests/util.py::make_qkv, s_aux = 0.5 randn or none) at the shapes of `inp`"""
    g = torch.Generator().manual_seed(seed)
    out = dict(inp)
    for name in ("q", "k", "v", "do"):
        out[name] = _rand(tuple(inp[name].shape), g, inp[name].dtype)
    out["s_aux"] = _rand((inp["q"].shape[1],), g, torch.float32, 0.5) if aux else None
    return out


# ------------------------------------------------------------------------------------------------ the tile walk
def _scores(q, k, ns, W, f32):
    """masked log2-domain scores [B, Hq, Nq, Nk] (fp64; f32: the products accumulated and scaled in float32)"""
    B, Hq, Nq, D = q.shape
    Hkv, Nk = k.shape[1], k.shape[2]
    grp = Hq // Hkv
    c = LOG2E / math.sqrt(D)
    if f32:
        s = (torch.matmul(q.float(), k.float().repeat_interleave(grp, dim=1).transpose(-1, -2)) * torch.tensor(c, dtype=torch.float32)).double()
    else:
        s = torch.matmul(q.double(), k.double().repeat_interleave(grp, dim=1).transpose(-1, -2)) * c
    mask = O.valid_mask(torch.arange(Nq) + (Nk - Nq), torch.arange(Nk), ns, W)
    return s.masked_fill(~mask, float("-inf"))


def tile_walk(q, k, v, ns, W, s_aux=None, mutant=None, round_p=None, f32_scores=False, thr=THR):
    """fp64 model of the forward kernels' walk.  Returns o [B,Hq,Nq,D], lse [B,Hq,Nq] (nat, -inf for an empty row) and ev:
    a dict of [T, B, Hq, Nq] tensors `asked` (the row rescales at this tile: alpha != 1), `later` (... and has seen a key in
    an earlier tile), `log2a` (log2 alpha, 0 where not asked), `vis` (the row sees a key of the tile), `rise` (tile maximum
    minus the reference before the tile, log2 units; -inf where nothing is visible or there was no reference).
    mutant: one of MUTANTS.  round_p: dtype P is rounded to before the PV and row-sum products."""
    assert mutant is None or mutant in MUTANTS
    B, Hq, Nq, D = q.shape
    Nk = k.shape[2]
    grp = Hq // k.shape[1]
    s = _scores(q, k, ns, W, f32_scores)
    vf = v.double().repeat_interleave(grp, dim=1)
    ninf = float("-inf")
    m = torch.full((B, Hq, Nq), ninf, dtype=torch.float64)
    l = torch.zeros(B, Hq, Nq, dtype=torch.float64)
    unit = torch.zeros(B, Hq, Nq, dtype=torch.float64)          # the s_aux unit of l, kept apart for skip_aux_unit
    if s_aux is not None:
        m = (s_aux.double() * LOG2E).view(1, Hq, 1).expand(B, Hq, Nq).clone()
        unit = torch.ones(B, Hq, Nq, dtype=torch.float64)
    o = torch.zeros(B, Hq, Nq, D, dtype=torch.float64)
    seen = torch.zeros(B, Hq, Nq, dtype=torch.bool)
    rows = torch.arange(Nq)
    ev = {x: [] for x in ("asked", "later", "log2a", "vis", "rise")}
    if mutant == "never_fp16":
        round_p = torch.float16
    for t in range((Nk + TILE - 1) // TILE):
        st = s[..., TILE * t:TILE * (t + 1)]
        vis = torch.isfinite(st).any(-1)
        mx = st.max(-1).values
        none = m == ninf
        m_cand = torch.maximum(m, mx)
        move = (m_cand > m + thr) | none
        if mutant == "never_fp16":
            move = none
        m_new = torch.where(move, m_cand, m)
        m_safe = torch.where(m_new == ninf, torch.zeros_like(m_new), m_new)
        log2a = torch.where(none, torch.zeros_like(m), m - m_safe)     # inf_no_rescale: a row that has seen nothing keeps alpha = 1
        alpha = torch.exp2(log2a)
        asked = alpha != 1
        ev["asked"].append(asked)
        ev["later"].append(asked & seen)
        ev["log2a"].append(log2a)
        ev["vis"].append(vis)
        ev["rise"].append(torch.where(none, torch.full_like(m, ninf), mx - m))
        a_o = alpha.unsqueeze(-1).expand(B, Hq, Nq, D)
        a_l, a_u = alpha, alpha
        if mutant == "alpha0":
            a_l = a_u = torch.where(asked, torch.zeros_like(alpha), alpha)
            a_o = a_l.unsqueeze(-1).expand(B, Hq, Nq, D)
        elif mutant in ("neighbour", "row32"):
            other = (rows ^ (1 if mutant == "neighbour" else 32)).clamp(max=Nq - 1)
            a_l = a_u = alpha[..., other]
            a_o = a_l.unsqueeze(-1).expand(B, Hq, Nq, D)
        elif mutant == "wave_bcast":
            nw = (Nq + 63) // 64
            pad = nw * 64 - Nq
            ak = torch.nn.functional.pad(asked, (0, pad)).view(B, Hq, nw, 64)
            al = torch.nn.functional.pad(alpha, (0, pad), value=1.0).view(B, Hq, nw, 64)
            first = ak.long().argmax(-1, keepdim=True)                 # the first row of the wave that asked (row 0 if none: alpha 1)
            a_l = a_u = torch.gather(al, -1, first).expand(B, Hq, nw, 64).reshape(B, Hq, nw * 64)[..., :Nq]
            a_l = a_u = torch.where(ak.any(-1, keepdim=True).expand(B, Hq, nw, 64).reshape(B, Hq, nw * 64)[..., :Nq], a_l, alpha)
            a_o = a_l.unsqueeze(-1).expand(B, Hq, Nq, D)
        elif mutant == "skip_o_block":
            a_o = a_o.clone()
            a_o[..., :32] = 1.0
        elif mutant == "skip_l":
            a_l = a_u = torch.ones_like(alpha)
        elif mutant == "skip_aux_unit":
            a_u = torch.ones_like(alpha)
        p = torch.exp2(st - m_safe.unsqueeze(-1))
        if round_p is not None:
            p = p.to(round_p).double()
        l = l * a_l + p.sum(-1)
        unit = unit * a_u
        o = o * a_o + torch.matmul(p, vf[:, :, TILE * t:TILE * (t + 1)])
        m = m_new
        seen = seen | vis
    lt = l + unit
    lt = torch.where(lt == 0, torch.ones_like(lt), lt)
    ev = {x: torch.stack(y) for x, y in ev.items()}
    return o / lt.unsqueeze(-1), (m + torch.log2(lt)) * LN2, ev


def events(ev):
    """[(batch, head, row, tile, alpha)] of a walk's `asked` events"""
    idx = torch.nonzero(ev["asked"])
    al = torch.exp2(ev["log2a"][ev["asked"]])
    return [(int(b), int(h), int(r), int(t), float(a)) for (t, b, h, r), a in zip(idx.tolist(), al.tolist())]


def mid(ev):
    """[T, B, Hq, Nq] bool: events with 2^-16 <= alpha < 2^-8 after the row's first visible tile"""
    return ev["later"] & (ev["log2a"] >= -16.0) & (ev["log2a"] < -8.0)


def coverage(ev):
    """counts of one walk: mid-range events; 64-row waves (per batch and head) with a visible later tile; those with a
    mid-range event; those in which one tile holds a moving row beside a still row that sees the tile; rises of 2 .. 8
    log2 units that did not move the reference, and moves"""
    md = mid(ev)
    T, B, Hq, Nq = md.shape
    nw = (Nq + 63) // 64
    pad = nw * 64 - Nq
    w = lambda x: torch.nn.functional.pad(x, (0, pad)).view(T, B, Hq, nw, 64)
    nvis = ev["vis"].long().cumsum(0)
    has_later = w(ev["vis"] & (nvis >= 2)).any(-1).any(0)                       # [B, Hq, nw]
    with_mid = w(md).any(-1).any(0)
    still = ev["vis"] & ~ev["asked"]
    mixed = (w(md).any(-1) & w(still).any(-1)).any(0)
    under = ev["vis"] & ~ev["asked"] & (ev["rise"] > 2.0) & (ev["rise"] <= THR)
    return dict(mid=int(md.sum()), later=int(ev["later"].sum()), waves=int(has_later.sum()),
                waves_mid=int((has_later & with_mid).sum()), waves_mixed=int((has_later & mixed).sum()),
                under=int(under.sum()), moves=int(ev["later"].sum()))


def walk_pack(fn, inp, cu, ns, W, **kw):
    """fn (tile_walk / precision_fwd) sequence by sequence over a pack; returns o, lse concatenated"""
    os_, ls = [], []
    for x, y in zip(cu[:-1], cu[1:]):
        r = fn(inp["q"][:, :, x:y], inp["k"][:, :, x:y], inp["v"][:, :, x:y], ns, W, inp["s_aux"], **kw)
        os_.append(r[0])
        ls.append(r[1])
    return torch.cat(os_, 2), torch.cat(ls, 2)


# ------------------------------------------------------------------------------------------------ the precision model
def precision_fwd(q, k, v, ns, W, s_aux=None):
    """the walk as a correct kernel of this dtype runs it: S in f32, P rounded to the dtype before the products, O rounded
    at the end, LSE in f32"""
    dt = q.dtype
    o, lse, _ = tile_walk(q, k, v, ns, W, s_aux, round_p=dt, f32_scores=True)
    return o.to(dt), lse.float()


def precision_bwd(q, k, v, do, o, lse, ns, W, s_aux=None):
    """the backward of a correct kernel of this dtype: delta from the ROUNDED O, P = exp2(s - lse) and dS rounded to the
    dtype before their products, f32 accumulation, results rounded.  Returns dq, dk, dv, ds_aux."""
    dt = q.dtype
    B, Hq, Nq, D = q.shape
    Hkv, Nk = k.shape[1], k.shape[2]
    grp = Hq // Hkv
    scale = 1.0 / math.sqrt(D)
    s = _scores(q, k, ns, W, True)
    lse2 = (lse.double() * LOG2E).float().double()
    p = torch.nan_to_num(torch.exp2(s - lse2.unsqueeze(-1)), nan=0.0).float().double()
    kf, vf = (x.double().repeat_interleave(grp, dim=1) for x in (k, v))
    dof = do.double()
    delta = (dof * o.double()).sum(-1).float().double()
    dp = torch.matmul(dof, vf.transpose(-1, -2)).float().double()
    ds = (p * (dp - delta.unsqueeze(-1))).to(dt).double()
    pr = p.to(dt).double()
    dv = torch.matmul(pr.transpose(-1, -2), dof)
    dq = torch.matmul(ds, kf) * scale
    dk = torch.matmul(ds.transpose(-1, -2), q.double()) * scale
    dk, dv = (x.view(B, Hkv, grp, Nk, D).sum(2) for x in (dk, dv))
    dsa = None
    if s_aux is not None:
        dsa = -(torch.exp(s_aux.double().view(1, Hq, 1) - lse.double()) * delta).sum((0, 2)).float()
    return dq.to(dt), dk.to(dt), dv.to(dt), dsa


# tolerances of tests/test_gpu_softmax_range.py: tests/test_gpu_prefill.py::test_shapes_fwd_bwd per dtype (max |error| of O;
# of the gradients, scaled by max(1, max |reference|) as the neighbouring tests scale theirs; ds_aux ten times the gradients'),
# the LSE bound of tests/test_asm_emu.py, tests/util.py::DECODE_TOL for the cache calls
TOL_O = {torch.float32: 2e-5, torch.float16: 4e-3, torch.bfloat16: 2e-2}
TOL_G = {torch.float32: 2e-4, torch.float16: 3e-2, torch.bfloat16: 1.5e-1}
TOL_LSE = 5e-3


def grad_tol(dtype, ref, aux=False):
    return TOL_G[dtype] * (10.0 if aux else 1.0) * max(1.0, ref.abs().max().item())


# ------------------------------------------------------------------------------------------------ case tables
# The cases of tests/test_gpu_softmax_range.py; tests/test_range_inputs.py runs its proofs on every one.
# shape = (B, Hq, Hkv, Nq, Nk, D, ns, W).  fwd: substring sfa_last_path() must show after the forward.
# seed: with the default seed (7000 + index) the randn part of these three hands one of the first rows of the sequence (fewer
# than 16 visible keys, on the staircase's level 0) a key with most of the row's mass; the single bf16 rounding of that p takes
# 0.51 - 0.52 of the LSE bound in the precision model, whatever the family does.  Another draw: 0.22 - 0.40.
RESEEDED = ("asm_d80_bf16_gqa_staircase_up", "asm_d96_bf16_gqa_aux_sweep", "strip_d80_up")


def _asm_cases():
    out = []
    for D in (64, 80, 96, 128):
        for dt in ("bf16", "fp16"):
            for heads, (Hq, Hkv) in (("gqa", (4, 1)), ("mha", (2, 2))):
                for fam in ("staircase_up", "staircase_down", "aux_sweep") + (("offset",) if D == 128 else ()):
                    out.append(dict(id=f"asm_d{D}_{dt}_{heads}_{fam}", shape=(1, Hq, Hkv, 777, 777, D, 4, 400), dtype=dt,
                                    family=fam, fwd="asm4x64pk", dq="bwd_mfma"))
                    if out[-1]["id"] in RESEEDED:
                        out[-1]["seed"] = 7100
    out.append(dict(id="asm_nq_lt_nk", shape=(1, 4, 1, 500, 777, 128, 4, 400), dtype="bf16", family="staircase_up",
                    fwd="asm4x64pk", dq="bwd_mfma"))
    return out


DENSE_CASES = _asm_cases() + [
    # strip forward (gpt-oss sliding layers): the rescale runs between blocks; backward: the skewed dK/dV sweep
    dict(id="strip_d64_up", shape=(1, 4, 1, 530, 530, 64, 0, 128), dtype="bf16", family="staircase_up", fwd="stripasm", dq="bwd_mfma"),
    dict(id="strip_d80_up", shape=(1, 8, 2, 530, 530, 80, 0, 128), dtype="bf16", family="staircase_up", fwd="stripasm", dq="bwd_mfma", seed=7100),
    dict(id="strip_d96_up", shape=(1, 4, 1, 530, 530, 96, 0, 128), dtype="fp16", family="staircase_up", fwd="stripasm", dq="bwd_mfma"),
    dict(id="strip_d64_aux", shape=(1, 8, 1, 530, 530, 64, 0, 128), dtype="fp16", family="aux_sweep", fwd="stripasm", dq="bwd_mfma"),
    dict(id="strip_d80_aux", shape=(1, 4, 1, 530, 530, 80, 0, 128), dtype="bf16", family="aux_sweep", fwd="stripasm", dq="bwd_mfma"),
    dict(id="strip_d96_aux", shape=(1, 4, 1, 530, 530, 96, 0, 128), dtype="bf16", family="aux_sweep", fwd="stripasm", dq="bwd_mfma"),
    # compiled MFMA kernels: fwd_mfma_kernel at head dims 32 and 256, the compiled strip kernel (short window WITH sinks)
    dict(id="mfma_d32_up", shape=(1, 4, 2, 777, 777, 32, 4, 400), dtype="bf16", family="staircase_up", fwd="fwd_mfma_bf16_d32_nw", dq="bwd_mfma_bf16_d32"),
    dict(id="mfma_d32_aux", shape=(1, 8, 2, 777, 777, 32, 4, 400), dtype="fp16", family="aux_sweep", fwd="fwd_mfma_f16_d32_nw", dq="bwd_mfma_f16_d32"),
    dict(id="mfma_d256_up", shape=(1, 4, 2, 777, 777, 256, 4, 400), dtype="fp16", family="staircase_up", fwd="fwd_mfma_f16_d256_nw", dq="bwd_mfma_f16_d256"),
    dict(id="mfma_d256_down", shape=(1, 4, 2, 777, 777, 256, 4, 400), dtype="bf16", family="staircase_down", fwd="fwd_mfma_bf16_d256_nw", dq="bwd_mfma_bf16_d256"),
    dict(id="mfma_d64_w128_sinks_up", shape=(1, 4, 2, 750, 750, 64, 4, 128), dtype="bf16", family="staircase_up", fwd="fwd_mfma_bf16_d64_strip", dq="bwd_mfma"),
    # exact-f32 kernels
    dict(id="fp32_up", shape=(1, 4, 2, 777, 777, 64, 4, 400), dtype="fp32", family="staircase_up", fwd="fwd_generic", dq="bwd_generic"),
    dict(id="fp32_down", shape=(1, 4, 2, 777, 777, 64, 4, 400), dtype="fp32", family="staircase_down", fwd="fwd_generic", dq="bwd_generic"),
    dict(id="fp32_offset", shape=(1, 4, 2, 777, 777, 64, 4, 400), dtype="fp32", family="offset", fwd="fwd_generic", dq="bwd_generic"),
    dict(id="fp32_aux", shape=(1, 8, 2, 777, 777, 64, 4, 400), dtype="fp32", family="aux_sweep", fwd="fwd_generic", dq="bwd_generic"),
    dict(id="generic_bf16_up", shape=(1, 4, 2, 777, 777, 64, 4, 400), dtype="bf16", family="staircase_up", generic=True, fwd="fwd_generic", dq="bwd_generic"),
]
# one pack: the first sequence randn, the second and third carry the staircase
PACK_CASE = dict(Hq=4, Hkv=1, D=128, ns=4, W=300, cu=[0, 200, 700, 1300], dtype="bf16", family="staircase_up")
# decode over many keys (several splits) and the multi-token call over a full ring (n = 5): (id, dtype, Hq, Hkv, D, family)
DECODE_CASES = [("down_bf16", "bf16", 8, 2, 128, "staircase_down"), ("aux_bf16", "bf16", 8, 2, 128, "aux_sweep"),
                ("down_fp32", "fp32", 8, 2, 64, "staircase_down"), ("down_fp16", "fp16", 8, 2, 64, "staircase_down")]
DECODE_NKV = 4096
DECODE_STEP = 256                 # a level per 256 keys
CHUNK_CASES = [("mfma_down", "bf16", 8, 2, 128, "staircase_down"), ("mfma_aux", "fp16", 8, 2, 64, "aux_sweep"),
               ("f32_down", "fp32", 8, 2, 64, "staircase_down"), ("f32_aux", "fp32", 8, 2, 64, "aux_sweep")]
CHUNK_RING = (4, 1024, 300, 5)    # num_sink, W, extra, n: the cache holds num_sink + W + extra tokens, the ring is full and wrapped


def case_inputs(case):
    i = [c["id"] for c in DENSE_CASES].index(case["id"])
    B, Hq, Hkv, Nq, Nk, D, ns, W = case["shape"]
    return dense_range(case["family"], B, Hq, Hkv, Nq, Nk, D, ns, W, DT[case["dtype"]], case.get("seed", 7000 + i))


def pack_inputs():
    c = PACK_CASE
    T = c["cu"][-1]
    return dense_range(c["family"], 1, c["Hq"], c["Hkv"], T, T, c["D"], c["ns"], c["W"], DT[c["dtype"]], 7500, cu=c["cu"])


def history_range(family, B, Hq, Hkv, D, total, n, dtype, seed, step=DECODE_STEP):
    """The cache calls: k / v hold `total` tokens, the LAST n of them are the query tokens (n = 1: plain decode over every
    key).  staircase_down: H falls by STEPS every `step` keys from the oldest key on (a split whose keys are all late has a
    maximum far below the first split's); the gains differ per q head and chunk row: GAINS[(t + head) % 4], and -1 on
    every fifth head (for that head the staircase rises: the LAST split holds the mass).  aux_sweep: randn, s_aux from
    AUX_SWEEP.  Returns q [B,Hq,n,D], k / v [B,Hkv,total,D], s_aux [Hq]."""
    g = torch.Generator().manual_seed(seed)
    scale = FP32_SCALE if dtype == torch.float32 else 1.0
    u = (torch.randint(0, 2, (B, Hkv, 1, D), generator=g).double() * 2 - 1)
    nq = torch.randn(B, Hq, n, D, generator=g, dtype=torch.float32).double()
    nk = torch.randn(B, Hkv, total, D, generator=g, dtype=torch.float32).double()
    v = _rand((B, Hkv, total, D), g, dtype)
    sa = _rand((Hq,), g, torch.float32, 0.8)
    if family == "aux_sweep":
        sa = torch.tensor([AUX_SWEEP[h % len(AUX_SWEEP)] for h in range(Hq)], dtype=torch.float32)
        return dict(q=nq.to(dtype), k=nk.to(dtype), v=v, s_aux=sa)
    H = torch.zeros(total, dtype=torch.float64)
    for x in range(step, total, step):
        H[x:] -= STEPS[(x // step) % 3]
    H = (H - (H.max() + H.min()) / 2) * scale
    t, h = torch.arange(n).view(1, n), torch.arange(Hq).view(Hq, 1)
    a = torch.tensor(GAINS, dtype=torch.float64)[(t + h + 1) % 4]
    a = torch.where((h % 5 == 4).expand_as(a), -torch.ones_like(a), a)
    uq = u.repeat_interleave(Hq // Hkv, dim=1)
    q = _perp(nq, uq) + a.view(1, Hq, n, 1) * uq
    k = _perp(nk, u) + (H / math.sqrt(D)).view(1, 1, total, 1) * u
    return dict(q=q.to(dtype), k=k.to(dtype), v=v, s_aux=sa, H=H, a=a)
