"""Which launch regime a call reaches: a pure-Python restatement of the launch arithmetic of the work-list and ticketed
kernels, the way tests/util.py::dkdv_kernel_name restates the dK/dV kernel rule.  Sources (csrc/): launch_asm and fwd_mfma
(sfa_fwd_mfma.hip); worklist_grid, launch_bwd, row_split_plan, sink_split_plan, row_split_extras and dkdv_asm_slices
(sfa_bwd_mfma.hip); SFA_WL_MAX_ITEMS (tools/asmgen/worklist.py: DESC_MAX).  Also the case table of
tests/test_gpu_work_lists.py, whose claims tests/test_grid_regime.py checks at 256 CUs and the GPU tests check again at
the device's own CU count before they run, and the raw C-ABI call with poisoned outputs those tests use."""

WL_MAX_ITEMS = 256          # descriptors of one work list (SFA_WL_MAX_ITEMS)
KBA = 256                   # keys per workgroup of the hand-placed dK/dV kernel (kKBA)
ASM_MIN_WINDOW = 256        # head dims below 128: windows up to this run the compiled kernels (kAsmMinWindow)


def cdiv(a, b):
    return -(-a // b)


def strip_asm_nt(W):
    """tiles per item of the strip bodies for a window of W keys (0 = not served)"""
    if W < 1 or W > 193:
        return 0
    return max((W - 1 + 63) // 64 + 1, 2)


def dkdv_asm_slices(kb, N, Nk, ns, W):
    """32-row slices the 256-key block kb sweeps"""
    P = Nk - N
    kb0 = kb * KBA
    kb1 = min(kb0 + KBA, Nk)
    i_hi = N if kb0 < ns else max(min(kb1 - 1 + W - P, N), 0)
    qt_lo = max(kb0 - P, 0) // 32
    return max((i_hi + 31) // 32, qt_lo) - qt_lo


def sink_split_plan(N, Nk, ns, W, packed, KB):
    """(chunks of block 0, slices per chunk, key rows of a partial, chunks of every other block, blocks with sink keys)"""
    if packed or ns <= 0 or Nk <= KB:
        return 1, 0, 0, 1, 1
    total = dkdv_asm_slices(0, N, Nk, ns, W)
    cs = max((KB + W + 31) // 32, 8)
    R = cdiv(total, cs)
    if R < 2:
        return 1, 0, 0, 1, 1
    if R > 64:
        R, cs = 64, (total + 63) // 64
    return R, cs, min(ns, KB), 1, 1


def row_split_plan(N, Nk, ns, W, packed, groups, g, n_cu, per_cu=2):
    nK = cdiv(Nk, KBA)
    base = nK * groups
    if packed or Nk != N or base >= per_cu * n_cu:
        return sink_split_plan(N, Nk, ns, W, packed, KBA)
    t_ref = min((KBA + W + 31) // 32, (N + 31) // 32)
    C = min(cdiv(per_cu * n_cu, base), 16)
    cs = max(cdiv(t_ref, C), max(cdiv(24, g), 2))
    C = cdiv(t_ref, cs)
    if C < 2:
        return sink_split_plan(N, Nk, ns, W, packed, KBA)
    return cdiv(dkdv_asm_slices(0, N, Nk, ns, W), cs), cs, KBA, C, min(max(cdiv(ns, KBA), 1), nK)


def asm_window_ok(D, window, wgs, n_cu):
    if D == 128:
        return True
    if not 64 <= D < 128:
        return False
    return window > ASM_MIN_WINDOW or wgs >= 2 * n_cu


def regime(B, Hq, Hkv, N, D, ns, W, n_cu, lens=None, overlap=True):
    """The launch regime of sfa_fwd + sfa_bwd (N_q = N_kv, 16-bit dtypes, head dims 64 / 80 / 96 / 128) on a device of n_cu
    CUs.  lens: the sequence lengths of a packed batch (then B and N are taken from them: the launch problem of the varlen
    calls is len(lens) sequences of the longest one's length).  overlap: SFA_FLAG_BWD_OVERLAP is passed and the calling
    thread has its side stream.  The dK/dV figures are those of the hand-placed kernel (dkdv_kernel_name says whether the
    call takes it)."""
    packed = lens is not None
    if packed:
        B, N = len(lens), max(lens)
    lens_ = list(lens) if packed else [N] * B
    g = Hq // Hkv
    Wc = min(max(W, 0), N)                                   # the window as the launchers clamp it
    r = {}
    # ---- forward / dQ work list
    hpw = 4 if g % 4 == 0 else (2 if g % 2 == 0 else 1)
    rows = 64 * (4 // hpw)
    n_qtiles, hgroups = cdiv(N, rows), g // hpw
    items = n_qtiles * hgroups * Hkv * B
    G = max(min(items, n_cu), cdiv(items, WL_MAX_ITEMS))
    rounds = cdiv(items, G)
    r.update(hpw=hpw, rows=rows, items=items, G=G, rounds=rounds, last_round=items - (rounds - 1) * G,
             ragged_last_tile=N % rows != 0,
             valid_items=sum(cdiv(n, rows) for n in lens_) * hgroups * Hkv)
    # ---- forward kernel
    strip_ok = ns <= 0 and g % 4 == 0 and strip_asm_nt(W) > 0
    wgs = cdiv(N, KBA) * Hkv * B
    if strip_ok and D in (64, 80, 96):
        fwd = "stripasm_nt%d" % strip_asm_nt(W)
    elif 0 < W <= 256 and D < 128:
        fwd = "strip"                                        # (compiled strip kernel, when its ring fits the LDS)
    elif (D == 128 or Wc > ASM_MIN_WINDOW) and (Wc > 0 or ns > 0) and D in (64, 80, 96, 128):
        fwd = "asm4x64pk_hpw%d" % hpw
    else:
        fwd = "compiled"
    r["fwd"] = fwd
    # ---- dQ
    list_ok = D in (64, 80, 96, 128) and asm_window_ok(D, Wc, wgs, n_cu) and (Wc > 0 or ns > 0)
    side = overlap and items < 4 * n_cu and list_ok
    r["strip_items"] = cdiv(N, 64) * (g // 4) * Hkv * B if g % 4 == 0 else 0      # the strip-kernel condition's count
    if D in (64, 80) and not side and strip_ok and r["strip_items"] >= 2 * n_cu:
        dq = "dqstripasm_nt%d" % strip_asm_nt(W)
    elif list_ok:
        dq = "dqasm4x64pk_hpw%d" % hpw
    else:
        dq = "compiled"
    tail = dq.startswith("dqasm") and G == n_cu and rounds >= 12
    r.update(dq=dq, dq_side_stream=side and dq.startswith("dqasm"), dq_tail=tail,
             dq_tail_first=(rounds - 2) * G if tail else None, dq_tail_ranks=items - (rounds - 2) * G if tail else 0)
    # ---- dK/dV, hand-placed kernel
    nK, nG = cdiv(N, KBA), Hkv * B
    n_base = nK * nG
    chunks, _, _, gen, nsb = row_split_plan(N, N, ns, Wc, packed, nG, g, n_cu)
    n_extra = (nsb * (chunks - 1) + ((nK - nsb) * (gen - 1) if gen > 1 else 0)) * nG
    tickets = n_base >= 2 * n_cu
    r.update(key_blocks=nK, nG=nG, n_base=n_base, tickets=tickets, n_base_and_7=n_base & 7, nG_and_7=nG & 7,
             sink_chunks=chunks, row_split=gen > 1, gen_chunks=gen, n_extra=n_extra,
             dkdv_grid=n_extra + n_base + (cdiv(n_base // 8, 8) * 8 if tickets else 0))
    return r


# The cases of tests/test_gpu_work_lists.py.  shape = B, Hq, Hkv, N, ns, W (or lens for a packed batch); Ds: the head dims
# it runs at; claims: what regime() must return for it - at 256 CUs on the CPU, and at the device's CU count on the GPU,
# where a case that does not reach its regime fails instead of passing empty.
DENSE_CASES = {
    "gqa4": dict(shape=(4, 16, 4, 2500, 4, 300), Ds=(128, 64), dtype="bfloat16",
                 claims=dict(hpw=4, rows=64, items=640, G=256, rounds=3, last_round=128, ragged_last_tile=True,
                             fwd="asm4x64pk_hpw4", dq="dqasm4x64pk_hpw4", dq_tail=False, dq_side_stream=True,
                             n_base=160, tickets=False, row_split=True)),
    "mha": dict(shape=(7, 7, 7, 2600, 4, 300), Ds=(128, 64), dtype="bfloat16",
                claims=dict(hpw=1, rows=256, items=539, G=256, rounds=3, last_round=27, fwd="asm4x64pk_hpw1",
                            dq="dqasm4x64pk_hpw1", dq_tail=False, tickets=True, n_base=539, n_base_and_7=3, nG=49,
                            nG_and_7=1, sink_chunks=5, row_split=False, n_extra=196)),
    "gqa2": dict(shape=(4, 16, 8, 2600, 4, 300), Ds=(96,), dtype="float16",
                 claims=dict(hpw=2, rows=128, items=672, G=256, rounds=3, last_round=160, fwd="asm4x64pk_hpw2",
                             dq="dqasm4x64pk_hpw2", dq_tail=False, tickets=False, row_split=True)),
    "tail": dict(shape=(3, 64, 16, 3840, 4, 300), Ds=(64, 128), dtype="bfloat16",
                 claims=dict(hpw=4, items=2880, G=256, rounds=12, fwd="asm4x64pk_hpw4", dq="dqasm4x64pk_hpw4",
                             dq_tail=True, dq_tail_first=2560, dq_tail_ranks=320, dq_side_stream=False, tickets=True,
                             n_base=720, nG=48, nG_and_7=0, sink_chunks=7, row_split=False)),
}
PACKED_CASES = {
    # lists with holes: most ranks of the short sequences are invalid
    "holes": dict(Hq=16, Hkv=4, ns=4, W=300, lens=(2500, 700, 0, 1, 1900, 2499), Ds=(128,), dtype="bfloat16",
                  claims=dict(hpw=4, items=960, G=256, rounds=4, valid_items=488, fwd="asm4x64pk_hpw4",
                              dq="dqasm4x64pk_hpw4")),
    # strip kernels: 32 query tiles x 2 head sets x 2 KV heads per sequence of the longest one's length, twice the CUs needed
    "strip": dict(Hq=16, Hkv=2, ns=0, W=128, lens=(2048, 1, 100, 1500, 700), Ds=(80, 64), dtype="bfloat16",
                  claims=dict(fwd="stripasm_nt3", dq="dqstripasm_nt3", strip_items=640, dq_side_stream=False)),
}


def case_regime(name, D, n_cu, overlap=True):
    """regime() of a case of the tables above, and the list of claims it misses (empty: the case reaches its regime)"""
    if name in DENSE_CASES:
        c = DENSE_CASES[name]
        B, Hq, Hkv, N, ns, W = c["shape"]
        r = regime(B, Hq, Hkv, N, D, ns, W, n_cu, overlap=overlap)
    else:
        c = PACKED_CASES[name]
        r = regime(0, c["Hq"], c["Hkv"], 0, D, c["ns"], c["W"], n_cu, lens=c["lens"], overlap=overlap)
    missed = ["%s[d%d] at %d CUs: %s = %r, the case needs %r" % (name, D, n_cu, k, r[k], want)
              for k, want in c["claims"].items() if r[k] != want]
    return r, missed


def raw_fwd_bwd(q, k, v, do, s_aux, ns, W, flags, ws=None, do_scale=None, out=None):
    """sfa_fwd then sfa_bwd through the C ABI on device tensors, with everything the kernels must write poisoned first: O,
    LSE, dQ, dK, dV and ds_aux are filled with NaN and every byte of the workspace with 0xFF (the dispatch counters
    included), so that a skipped item or a counter the call forgot to zero shows instead of meeting whatever the allocator
    left there.  ws: a workspace to REUSE as it is (not refilled: the stale-counter tests); out: a dict of an earlier
    call whose buffers to reuse (graph capture).  Returns the outputs, the workspace and sfa_last_path() of both calls."""
    import torch
    from sink_attention import _native as N
    lib = N.lib()
    B, Hq, Nq, D = q.shape
    Hkv = k.shape[1]
    scale = D ** -0.5
    if out is None:
        nan = lambda shape, dt: torch.full(shape, float("nan"), device=q.device, dtype=dt)
        out = dict(o=nan(q.shape, q.dtype), lse=nan((B, Hq, Nq), torch.float32), dq=nan(q.shape, q.dtype),
                   dk=nan(k.shape, k.dtype), dv=nan(v.shape, v.dtype), ds_aux=nan((Hq,), torch.float32))
        n_ws = int(lib.sfa_bwd_workspace_bytes(B, Hq, Hkv, Nq, D, N.SFA_DTYPE[q.dtype], ns, W, flags))
        out["ws"] = torch.full((max(n_ws, 256),), 0xFF, dtype=torch.uint8, device=q.device) if ws is None else ws
    ws = out["ws"]
    stream = N.stream_ptr(q.device)
    N.check(lib.sfa_fwd(N.desc(q), N.desc(k), N.desc(v), N.desc(out["o"]), out["lse"].data_ptr(), s_aux.data_ptr(), ns, W,
                        scale, 0, stream), "sfa_fwd")
    out["fwd_path"] = N.last_path()
    d = do if do_scale is None else do * do_scale
    N.check(lib.sfa_bwd(N.desc(q), N.desc(k), N.desc(v), N.desc(out["o"]), N.desc(d), out["lse"].data_ptr(),
                        s_aux.data_ptr(), N.desc(out["dq"]), N.desc(out["dk"]), N.desc(out["dv"]),
                        out["ds_aux"].data_ptr(), ws.data_ptr(), ws.numel(), ns, W, scale, flags, stream), "sfa_bwd")
    out["bwd_path"] = N.last_path()
    return out
