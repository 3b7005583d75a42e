"""Fork groups of the packed step (include/sfa.h), restated in Python for the tests: the rule for the
shared length Lg of a group, the two maps of the group preparation launch, the plan of the shared phase and of a member's
private part, the workspace size, the fp64 oracle of a step over a gathered pool with three mutants of the kernel, and the
inputs (randn and probes) of the GPU cases.  Nothing here touches a GPU.

A state row is [sink_len, window_len, write_pos, seen]; a table row holds one page id per P ring slots (an id outside
[0, n_pages) is unmapped).  Offsets are clamped and made non-decreasing PAIRWISE, as the kernels do."""
import math

import torch

import probe_inputs as PI
from packed_regime import cdiv, max_splits, multi_plan, ragged_geom, want_splits

TILE = 32
NS, HKV = 4, 2


def al256(x):
    return (x + 255) & ~255


# ------------------------------------------------------------------------------------------------ offsets
def seq_of(cu_q, i, T):
    """(first packed row, length) of sequence i: ragged_seq"""
    c0 = min(max(cu_q[i], 0), T)
    c1 = max(min(max(cu_q[i + 1], 0), T), c0)
    return c0, c1 - c0


def group_span(cu_q, cu_g, g, n_seq, T):
    """(i0, i1, first packed row, rows) of group g: from the first row of sequence i0 to the end of sequence i1 - 1"""
    i0 = min(max(cu_g[g], 0), n_seq)
    i1 = max(min(max(cu_g[g + 1], 0), n_seq), i0)
    if i1 == i0:
        return i0, i1, 0, 0
    a, z = seq_of(cu_q, i0, T), seq_of(cu_q, i1 - 1, T)
    return i0, i1, a[0], max(z[0] + z[1] - a[0], 0)


# ------------------------------------------------------------------------------------------------ the rule for Lg
def clamp_state(st, Wc):
    wl = min(max(st[1], 0), Wc)
    wp = min(max(st[2], 0), Wc - 1)
    return wl, wp


def members(cu_q, cu_g, g, slots, npool, T):
    """the members of group g: active sequences (slot in the pool) with n_i > 0"""
    i0, i1, _, _ = group_span(cu_q, cu_g, g, len(slots), T)
    return [i for i in range(i0, i1) if 0 <= slots[i] < npool and seq_of(cu_q, i, T)[1] > 0]


def group_lg(cu_q, cu_g, g, slots, states, table, n_pages, P, Wc, T, admit=False):
    """(Lg, cache row of the first member) of group g.  Lg is the largest multiple of P such that every member is not
    admitting, has window_len + n_i <= Wc and write_pos == window_len, has Lg <= window_len and table entries j < Lg / P
    that are mapped and equal the first member's; fewer than two members: 0.  A member whose rows leave the group's span
    (offsets that are not monotonic) makes it 0 as well, and so does a clamped cu_g that decreases ANYWHERE (groups
    could overlap): then every group of the call shares nothing."""
    npool = len(states)
    mem = members(cu_q, cu_g, g, slots, npool, T)
    first = slots[mem[0]] if mem else 0
    cl = [min(max(x, 0), len(slots)) for x in cu_g]
    if len(mem) < 2 or any(b < a for a, b in zip(cl[:-1], cl[1:])):
        return 0, first
    _, _, gc0, gn = group_span(cu_q, cu_g, g, len(slots), T)
    lim = None
    for i in mem:
        st = states[slots[i]]
        c0, n = seq_of(cu_q, i, T)
        wl, wp = clamp_state(st, Wc)
        li = wl // P * P
        if (admit and st[3] == 0) or wl + n > Wc or wp != wl:
            li = 0
        if c0 < gc0 or c0 + n > gc0 + gn:
            li = 0
        lim = li if lim is None else min(lim, li)
    for j in range(lim // P):
        e0 = table[first][j]
        if not 0 <= e0 < n_pages or any(table[slots[i]][j] != e0 for i in mem):
            return j * P, first
    return lim, first


def prep(cu_q, cu_g, slots, states, table, n_pages, P, Wc, T, G, admit=False):
    """what group_prep_kernel leaves in the workspace: lg / first per group, gseq per sequence, gblk per group row block"""
    n_seq, n_grp = len(slots), len(cu_g) - 1
    spans = [group_span(cu_q, cu_g, g, n_seq, T) for g in range(n_grp)]
    out = [group_lg(cu_q, cu_g, g, slots, states, table, n_pages, P, Wc, T, admit) for g in range(n_grp)]
    gseq = []
    for i in range(n_seq):
        at = [g for g in range(n_grp) if spans[g][0] <= i]
        g = at[-1] if at else 0
        gseq.append(g if spans[g][0] <= i < spans[g][1] else -1)
    ngrb = cdiv(G * T, 32) + n_grp
    gblk = [(-1, 0)] * ngrb
    for g, (i0, i1, c0, n) in enumerate(spans):
        for b in range(cdiv(G * n, 32)):
            idx = G * c0 // 32 + g + b
            assert gblk[idx] == (-1, 0), "group row-block ranges must be disjoint"
            gblk[idx] = (g, b)
    return dict(lg=[o[0] for o in out], first=[o[1] for o in out], gseq=gseq, gblk=gblk, ngrb=ngrb)


# ------------------------------------------------------------------------------------------------ plans and workspace
def group_geom(n_grp, Hq, Hkv, T, Nkv_cache):
    G = Hq // Hkv
    ngrb = cdiv(G * T, 32) + n_grp
    Sgw = max_splits(1, Hkv, ngrb, Nkv_cache)
    return dict(ngrb=ngrb, want=want_splits(1, Hkv, ngrb), Sgw=Sgw, nsh=cdiv(Hkv * Sgw * ngrb, 8) * 8, P=Hkv * T * G * Sgw)


def group_plan(lg, n_grp, Hq, Hkv, T):
    """the shared phase of a group: ring tiles of [0, lg), a function of (lg, the call's shape) only"""
    return multi_plan(0, lg, 0, group_geom(n_grp, Hq, Hkv, T, 0)["want"])


def member_plan(sl, wl, n, lg, n_seq, Hq, Hkv, T):
    """a member's own workgroups: sinks, ring slots [lg, wl) and the chunk; ring tile i starts at slot lg + 32 (i - T0)"""
    return multi_plan(sl, wl - lg, n, ragged_geom(n_seq, Hq, Hkv, T, 0)["want"])


def ragged_workspace_bytes(n_seq, Hq, Hkv, T, Nkv_cache, D):
    g = ragged_geom(n_seq, Hq, Hkv, T, Nkv_cache)
    return 2 * al256(g["P"] * 4) + al256(g["P"] * D * 4) + al256(g["nrb"] * 8) + al256(T * 4)


def group_workspace_bytes(n_seq, n_grp, Hq, Hkv, T, Nkv_cache, D):
    g = group_geom(n_grp, Hq, Hkv, T, Nkv_cache)
    return (ragged_workspace_bytes(n_seq, Hq, Hkv, T, Nkv_cache, D) + 2 * al256(g["P"] * 4) + al256(g["P"] * D * 4) +
            al256(g["ngrb"] * 8) + al256(n_grp * 8) + 2 * al256(n_seq * 4))


# ------------------------------------------------------------------------------------------------ oracle and mutants
MUTANTS = ("members_keep_shared", "no_group_fold", "first_q")


def attend(parts, sa_h, D):
    """fp64 softmax attention of ONE (row, head) over key parts [(q [D], K [n, D], V [n, D])], each part with its own q -
    the real kernel uses one q, the first_q mutant another for the shared part; sa_h: the s_aux logit or None"""
    logits = [(q.double() @ K.double().T) / math.sqrt(D) for q, K, _ in parts]
    V = torch.cat([v.double() for _, _, v in parts], 0)
    s = torch.cat(logits)
    if sa_h is not None:
        s = torch.cat([s, torch.tensor([float(sa_h)], dtype=torch.float64)])
    w = torch.softmax(s, 0)
    return w[:V.shape[0]] @ V


def oracle_seq(q, k_new, v_new, sa, sink, ring, sl, wl, c0, n, G, lg=0, mutant=None, q_first_row=None):
    """fp64 rows [Hq, n, D] of one unwrapped, non-admitting sequence (wl + n <= Wc: every row sees the sinks, ring slots
    [0, wl) and the chunk up to itself).  sink / ring: (K, V) [Hkv, *, D] of its slot, the ring gathered through its table
    row.  q / k_new / v_new: the packs.  mutant (with lg > 0): members_keep_shared - ring [0, lg) counted by the shared
    phase AND the member; no_group_fold - ring [0, lg) missing; first_q - the shared part's logits from packed row
    q_first_row (the group's first row)."""
    Hq, D = q.shape[1], q.shape[3]
    out = torch.zeros(Hq, n, D, dtype=torch.float64)
    for h in range(Hq):
        hk = h // G
        for t in range(n):
            qr = q[0, h, c0 + t]
            K = torch.cat([sink[0][hk, :sl], ring[0][hk, lg:wl], k_new[0, hk, c0:c0 + t + 1]], 0)
            V = torch.cat([sink[1][hk, :sl], ring[1][hk, lg:wl], v_new[0, hk, c0:c0 + t + 1]], 0)
            parts = [(qr, K, V)]
            shared = (ring[0][hk, :lg], ring[1][hk, :lg])
            if lg > 0 and mutant != "no_group_fold":
                parts.append((q[0, h, q_first_row] if mutant == "first_q" else qr, *shared))
            if lg > 0 and mutant == "members_keep_shared":
                parts.append((qr, *shared))
            out[h, t] = attend(parts, None if sa is None else sa[h], D)
    return out


# ------------------------------------------------------------------------------------------------ the GPU cases
# geometry: (P, Wc, n_pages, prompt lengths); the ring of a prompt of L tokens holds L - NS of them
# wide: 8 forks x 131 shared entries are 1048 (member, entry) pairs - a second round of group_prep_kernel's compare
GEOM = {"small": dict(P=32, Wc=128, n_pages=64), "long": dict(P=64, Wc=1024, n_pages=160),
        "wide": dict(P=32, Wc=8192, n_pages=200)}
PROMPTS = {"small": (70, 64, 100), "long": (700,)}
# (geometry, dtype, D, G): H_kv = 2, G in {1, 8}, D in {64, 128} plus one case each at 80 and 96
SHAPES = [("small", "bf16", 64, 8), ("small", "fp16", 128, 1), ("small", "bf16", 80, 8), ("small", "fp16", 96, 1),
          ("long", "bf16", 64, 8), ("long", "fp16", 128, 8), ("long", "bf16", 128, 1), ("long", "fp16", 64, 1)]
DT = PI._DT


def expected_lg(geom, prompt):
    """Lg of forks of one prompt right after the fork and the reserve of a step: the pages in front of the one that holds
    the write slot"""
    return (prompt - NS) // GEOM[geom]["P"] * GEOM[geom]["P"]


def probe_targets(lg, wl, group_tps):
    """ring slots the probes aim at: the last shared key, the first private key (the chunk's first if the private part is
    empty: None), slot 0, the last key of group split 0"""
    return [lg - 1, lg if lg < wl else None, 0, min(group_tps * TILE, lg) - 1]


def prompt_kv(L, D, dtype, seed, probe):
    """k / v [1, H_kv, L, D] of a prompt: randn, or - for the probes - K rows of +-1 codes (probe_inputs.codes)"""
    g = torch.Generator().manual_seed(seed)
    k = PI.codes((1, HKV, L, D), g, dtype) if probe else PI._rand((1, HKV, L, D), g, dtype)
    return k, PI._rand((1, HKV, L, D), g, dtype)


def step_inputs(lengths, G, D, dtype, seed, probe=None):
    """q [1, Hq, T, D], k_new / v_new [1, H_kv, T, D], s_aux [Hq] of one packed step.  probe: {sequence: (K ring rows
    [H_kv, Wc, D] of its slot, targets)} - the LAST row of such a sequence is aimed per head at one target slot (rotating
    with sequence and head; None: its own new key), q = a * code row, and s_aux sits at the target's logit a sqrt(D), as
    probe_inputs.decode_probe builds it."""
    T, Hq = sum(lengths), HKV * G
    g = torch.Generator().manual_seed(seed)
    q, k, v = PI._rand((1, Hq, T, D), g, dtype), PI._rand((1, HKV, T, D), g, dtype), PI._rand((1, HKV, T, D), g, dtype)
    sa = torch.randn(Hq, generator=g) * 0.5
    if probe:
        a = PI.amplitude(D)
        k = PI.codes((1, HKV, T, D), g, dtype)
        sa = a * D ** 0.5 + PI.DECODE_AUX_JITTER * torch.randn(Hq, generator=g, dtype=torch.float32)
        c0 = 0
        for i, n in enumerate(lengths):
            if i in probe and n > 0:
                ring_k, targets = probe[i]
                for h in range(Hq):
                    s = targets[(i + h) % len(targets)]
                    src = k[0, h // G, c0 + n - 1] if s is None else ring_k[h // G, s]
                    q[0, h, c0 + n - 1] = (a * src.float()).to(dtype)
            c0 += n
    return q, k, v, sa
