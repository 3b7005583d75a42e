"""ragged_step_dyn(groups=): a shared prompt prefix is read once per fork group (sfa_decode_ring_ragged_group_paged_slots,
DESIGN.md 3.3.13).

Yardstick: the fp64 oracle (tests/group_regime.py::oracle_seq) over the pool gathered through each slot's own table row
(tests/paged_ref.py::gather), within DECODE_TOL[dtype] of tests/util.py.  Inputs: randn, and probes aimed at the last
shared key (slot Lg - 1), the first private key (slot Lg), slot 0 and the last key of group split 0.  o is NaN-filled and
the workspace 0xFF-filled before every call.  Every step also runs with groups=None on a TWIN pool built by the same calls:
the committed pool and the state rows must equal the twin's bit for bit, and where every group has Lg = 0 so must o.
group_regime is asked with the device's own state rows and table before every grouped step, so no case passes with Lg = 0
by accident.  Every test fails without the feature: the keyword and the symbols do not exist."""
import pytest
import torch

import group_regime as GR
import paged_ref as PR
from sink_attention import SinkCacheLayer
from sink_attention import _native as N
from sink_attention.cache import group_offsets
from util import DECODE_TOL

pytestmark = pytest.mark.gpu
DEV = "cuda"
NS, HKV = GR.NS, GR.HKV
FP8 = torch.float8_e4m3fn
NSLOT = 12


def _bits(t):
    return t.view(torch.uint8) if t.element_size() == 1 else t.view(torch.int16)


class Pool:
    """a paged pool with the host bookkeeping of a serving loop"""

    def __init__(self, geom, dtype, D, kv_dtype=None):
        g = GR.GEOM[geom]
        self.P, self.Wc, self.n_pages, self.dtype, self.D = g["P"], g["Wc"], g["n_pages"], dtype, D
        self.layer = SinkCacheLayer(NS, self.Wc)
        self.layer.init_pool(NSLOT, HKV, D, dtype, DEV, page_size=self.P, num_pages=self.n_pages, kv_dtype=kv_dtype)
        if kv_dtype is not None:
            self.layer.set_kv_scale([0.5, 2.0], [4.0, 0.25])
        self.seen = [0] * NSLOT
        # every byte of the four buffers is planted, live or not: a key read beyond a slot's fill moves the output
        g = torch.Generator().manual_seed(77)
        for name in ("sink_k", "sink_v", "window_k", "window_v"):
            buf = getattr(self.layer, name)
            if buf.dtype == FP8:
                buf.view(torch.uint8).copy_(torch.randint(0x30, 0x48, buf.shape, generator=g, dtype=torch.uint8))     # |x| in [0.5, 4)
            else:
                buf.copy_(torch.randn(buf.shape, generator=g).to(buf.dtype))
        orig = self.layer._call_consts

        def poisoned(attr, key, ws_bytes, zeroed, q):
            st = orig(attr, key, ws_bytes, zeroed, q)
            st["ws"].fill_(0xFF)
            return st
        self.layer._call_consts = poisoned

    def prefill(self, slot, k, v):
        L = k.shape[2]
        self.layer.reserve_pages([slot], L)
        self.layer.prefill_slots(k.to(DEV), v.to(DEV), [0, L], [slot])
        self.seen[slot] = L

    def fork(self, src, dsts):
        self.layer.fork_slots([src] * len(dsts), dsts, share=True, tokens=self.seen[src])
        for d in dsts:
            self.seen[d] = self.seen[src]

    def reserve(self, slots, lengths):
        act = [(s, n) for s, n in zip(slots, lengths) if s >= 0]
        self.layer.reserve_pages([s for s, _ in act], [self.seen[s] + n for s, n in act])

    def snapshot(self):
        """states, table and the dequantised cache as the step reads it: sinks [S, Hkv, ns, D], rings gathered [S, Hkv, Wc, D]"""
        L = self.layer
        table = L.page_table.cpu()

        def deq(t, row):
            t = t.cpu()
            if t.dtype != FP8:
                return t
            return (t.float() * L.kv_scale[row].cpu().view(1, HKV, 1, 1)).to(self.dtype)
        ring = [deq(PR.gather(_bits(getattr(L, n)), table).view(getattr(L, n).dtype), r) for r, n in enumerate(("window_k", "window_v"))]
        sink = [deq(getattr(L, n), r) for r, n in enumerate(("sink_k", "sink_v"))]
        return dict(states=L._dev_state.cpu().tolist(), table=table.tolist(), ring=ring, sink=sink)

    def raw(self):
        L = self.layer
        live = L._dev_state[:, 1].tolist()
        rings = [PR.gather(_bits(getattr(L, n)), L.page_table.cpu()) for n in ("window_k", "window_v")]
        return dict(state=L._dev_state.clone(), sinks=[_bits(L.sink_k).clone(), _bits(L.sink_v).clone()],
                    rings=[[r[s, :, :live[s]].clone() for s in range(NSLOT)] for r in rings])

    def step(self, inp, lengths, slots, groups=None, commit=True, admit=False, commit_seq=None, out=None):
        q, k, v, sa = inp
        cu = [0]
        for n in lengths:
            cu.append(cu[-1] + n)
        for attr in ("_ragged_state", "_ragged_group_state"):
            st = getattr(self.layer, attr, None)
            if st is not None:
                st["ws"].fill_(0xFF)
        if out is None:
            out = torch.full(q.shape, float("nan"), dtype=q.dtype, device=DEV)
        o = self.layer.ragged_step_dyn(q.to(DEV), k.to(DEV), v.to(DEV), cu, slots, s_aux=sa.to(DEV), out=out, commit=commit,
                                       admit=admit, commit_seq=commit_seq, groups=groups)
        path = N.last_path()
        assert ("_group" in path) == (groups is not None) and path.endswith("_paged" + ("_kvfp8" if self.layer._kv8 else "")), path
        if commit:
            for i, (s, n) in enumerate(zip(slots, lengths)):
                if s >= 0 and (commit_seq is None or commit_seq[i]):
                    self.seen[s] += n
        return o


def _same_pool(a, b, what):
    ra, rb = a.raw(), b.raw()
    assert torch.equal(ra["state"], rb["state"]), (what, "state rows", ra["state"].tolist(), rb["state"].tolist())
    for x, y in zip(ra["sinks"], rb["sinks"]):
        assert torch.equal(x, y), (what, "sinks")
    for x, y in zip(ra["rings"], rb["rings"]):
        for s in range(NSLOT):
            assert torch.equal(x[s], y[s]), (what, "ring of slot", s)


def _cu(lengths):
    cu = [0]
    for n in lengths:
        cu.append(cu[-1] + n)
    return cu


def _regime(pool, snap, lengths, slots, groups, G, admit=False):
    T = sum(lengths)
    return GR.prep(_cu(lengths), list(groups), slots, snap["states"], snap["table"], pool.n_pages, pool.P, pool.Wc, T, G, admit)


def _check(pool, snap, reg, inp, o, lengths, slots, tol, what, admit=False):
    """every active sequence that the oracle covers (unwrapped, not admitting) within tol; rows of inactive and empty
    sequences exactly zero; no NaN anywhere"""
    q, k, v, sa = inp
    o = o.cpu()
    assert not torch.isnan(o.float()).any(), (what, "NaN in o: a row or a partial was not written")
    cu, G = _cu(lengths), q.shape[1] // HKV
    for i, (s, n) in enumerate(zip(slots, lengths)):
        rows = o[0, :, cu[i]:cu[i] + n].double()
        if s < 0:
            assert not rows.any(), (what, "inactive sequence", i)
            continue
        st = snap["states"][s]
        if n == 0 or st[1] + n > pool.Wc or (admit and st[3] == 0):
            continue
        g = reg["gseq"][i]
        lg = reg["lg"][g] if g >= 0 else 0
        ref = GR.oracle_seq(q, k, v, sa, [t[s] for t in snap["sink"]], [t[s] for t in snap["ring"]], st[0], st[1], cu[i], n, G, lg)
        err = (rows - ref).abs().max().item()
        print(what, "sequence", i, "slot", s, "n", n, "Lg", lg, "max error", err, "tol", tol)
        assert err <= tol, (what, "sequence", i, err)


def _forked(geom, dtype, D, prompt, n_forks, seed, probe=False, kv_dtype=None, twin=True):
    """a pool (and its twin) with a prompt on slot 0 forked into slots 1 .. n_forks - 1"""
    pools = [Pool(geom, dtype, D, kv_dtype) for _ in range(2 if twin else 1)]
    k, v = GR.prompt_kv(prompt, D, dtype, seed, probe)
    for p in pools:
        p.prefill(0, k, v)
        p.fork(0, list(range(1, n_forks)))
    return pools


def _probe_spec(pool, snap, reg, lengths, slots, G, only=None):
    """aim the last row of every member of a sharing group at the four target slots (only: at these ring slots instead)"""
    spec, T, n_grp = {}, sum(lengths), len(reg["lg"])
    for i, s in enumerate(slots):
        g = reg["gseq"][i]
        if s < 0 or g < 0 or reg["lg"][g] == 0:
            continue
        tps = GR.group_plan(reg["lg"][g], n_grp, HKV * G, HKV, T)["tps"]
        spec[i] = (snap["ring"][0][s], only or GR.probe_targets(reg["lg"][g], snap["states"][s][1], tps))
    return spec


def _two_steps(geom, dt, D, G, prompt, lengths, slots, groups, seed, kv_dtype=None, want_lg=None, lengths2=None):
    """two committed steps (randn, then probes): after the first the forks hold different private tokens"""
    dtype = GR.DT[dt]
    n_forks = max(slots) + 1
    pool, twin = _forked(geom, dtype, D, prompt, n_forks, seed, probe=True, kv_dtype=kv_dtype)
    tol = DECODE_TOL[dtype]
    for step in range(2):
        lengths = lengths2 if step and lengths2 else lengths
        for p in (pool, twin):
            p.reserve(slots, lengths)
        snap = pool.snapshot()
        reg = _regime(pool, snap, lengths, slots, groups, G)
        if want_lg is not None:
            assert reg["lg"] == want_lg, (reg["lg"], want_lg)
        assert any(reg["lg"]), "the case must share something"
        inp = GR.step_inputs(lengths, G, D, dtype, seed + 10 + step, probe=_probe_spec(pool, snap, reg, lengths, slots, G) if step else None)
        o = pool.step(inp, lengths, slots, groups=groups)
        twin.step(inp, lengths, slots)
        _check(pool, snap, reg, inp, o, lengths, slots, tol, (geom, dt, D, G, "step", step))
        _same_pool(pool, twin, ("pool and state against the ungrouped twin", step))


# ------------------------------------------------------------------ 1. forks of one prompt against the oracle
@pytest.mark.parametrize("geom,dt,D,G", GR.SHAPES)
def test_eight_forks_of_one_prompt_read_the_prefix_once(geom, dt, D, G):
    """8 decode rows: at G = 8 two full group row blocks"""
    prompt = GR.PROMPTS[geom][0]
    _two_steps(geom, dt, D, G, prompt, [1] * 8, list(range(8)), [0, 8], seed=100 + D, want_lg=[GR.expected_lg(geom, prompt)])


@pytest.mark.parametrize("prompt,n_forks,G", [(64, 5, 8), (100, 3, 1), (100, 5, 8)])
def test_a_partial_group_block_and_three_forks_at_g_1(prompt, n_forks, G):
    _two_steps("small", "bf16", 64, G, prompt, [1] * n_forks, list(range(n_forks)), [0, n_forks], seed=200 + prompt,
               want_lg=[GR.expected_lg("small", prompt)])


@pytest.mark.parametrize("geom,G", [("small", 8), ("small", 1), ("long", 8)])
def test_members_of_1_3_0_and_40_tokens_and_an_inactive_member(geom, G):
    """lengths [3, 3, 0, 40, 1, 1]: at G = 8 the second member straddles two group row blocks, at G = 1 the 40-token member
    does; the fifth sequence is inactive (its rows are zeros), the third is empty"""
    prompt = GR.PROMPTS[geom][0]
    _two_steps(geom, "bf16", 64, G, prompt, [3, 3, 0, 40, 1, 1], [0, 1, 2, 3, -1, 4], [0, 6], seed=300 + G,
               lengths2=[1, 3, 0, 3, 1, 1])        # the second step stays inside the small ring


@pytest.mark.parametrize("geom,dt,D,G", [("small", "bf16", 64, 8), ("long", "fp16", 128, 8), ("small", "fp16", 80, 1)])
def test_fp8_pages(geom, dt, D, G):
    prompt = GR.PROMPTS[geom][0]
    _two_steps(geom, dt, D, G, prompt, [1] * 8, list(range(8)), [0, 8], seed=400 + D, kv_dtype=FP8,
               want_lg=[GR.expected_lg(geom, prompt)])


# ------------------------------------------------------------------ 2. several groups, ungrouped sequences, forks of forks
def _two_prompts(dtype, D, seed, probe=True, kv_dtype=None):
    """slots 0-2: forks of a prompt of 70; slots 3-6: forks of a prompt of 100, of which 5 and 6 are forks of the fork 4
    made after a committed step; slots 7, 8: two unrelated prompts of 64"""
    pools = [Pool("small", dtype, D, kv_dtype) for _ in range(2)]
    ka, va = GR.prompt_kv(70, D, dtype, seed, probe)
    kb, vb = GR.prompt_kv(100, D, dtype, seed + 1, probe)
    for p in pools:
        p.prefill(0, ka, va)
        p.fork(0, [1, 2])
        p.prefill(3, kb, vb)
        p.fork(3, [4])
        for s in (7, 8):
            p.prefill(s, *GR.prompt_kv(64, D, dtype, seed + s, probe))
    inp = GR.step_inputs([1, 1], 8, D, dtype, seed + 20)
    for p in pools:                                       # slots 3 and 4 diverge, then 4 is forked again
        p.reserve([3, 4], [1, 1])
        p.step(inp, [1, 1], [3, 4])
        p.fork(4, [5, 6])
    return pools


def test_two_groups_of_different_prompts_forks_of_forks_and_ungrouped_sequences():
    dtype, D, G = torch.bfloat16, 64, 8
    pool, twin = _two_prompts(dtype, D, seed=500)
    slots, lengths = [7, 0, 1, 2, 3, 4, 5, 6, 8], [1, 1, 2, 1, 1, 1, 3, 1, 1]
    groups = group_offsets([None, "a", "a", "a", "b", "b", "b", "b", None])
    assert groups == [0, 1, 4, 8, 9]
    for p in (pool, twin):
        p.reserve(slots, lengths)
    snap = pool.snapshot()
    reg = _regime(pool, snap, lengths, slots, groups, G)
    # 3 .. 6 share the three full pages of the prompt; the page of the write slot is each slot's own
    assert reg["lg"] == [0, 64, 96, 0], reg["lg"]
    inp = GR.step_inputs(lengths, G, D, dtype, 521, probe=_probe_spec(pool, snap, reg, lengths, slots, G))
    o = pool.step(inp, lengths, slots, groups=groups)
    twin.step(inp, lengths, slots)
    _check(pool, snap, reg, inp, o, lengths, slots, DECODE_TOL[dtype], "two groups")
    _same_pool(pool, twin, "two groups")


# ------------------------------------------------------------------ 3. admission and per-sequence commit
def test_an_admitting_sequence_outside_and_inside_a_group():
    """admit=True: a fresh slot outside the groups leaves them alone; a fresh slot INSIDE a group makes its Lg 0"""
    dtype, D, G = torch.bfloat16, 64, 8
    pool, twin = _forked("small", dtype, D, 70, 4, seed=600, probe=True)
    slots, lengths = [0, 1, 2, 3, 9], [1, 1, 1, 1, 6]
    for groups, want in (([0, 4], [64]), ([0, 2, 5], [64, 0])):
        for p in (pool, twin):
            p.layer.release_slots([9]), p.layer.free_pages([9])
            p.seen[9] = 0
            p.reserve(slots, lengths)
        snap = pool.snapshot()
        reg = _regime(pool, snap, lengths, slots, groups, G, admit=True)
        assert reg["lg"] == want, reg["lg"]
        inp = GR.step_inputs(lengths, G, D, dtype, 610 + len(groups))
        o = pool.step(inp, lengths, slots, groups=groups, admit=True)
        ot = twin.step(inp, lengths, slots, admit=True)
        _check(pool, snap, reg, inp, o, lengths, slots, DECODE_TOL[dtype], ("admit", groups), admit=True)
        # the admitting sequence is computed exactly as by the ungrouped call, wherever it stands
        assert torch.equal(_bits(o[:, :, 4:]), _bits(ot[:, :, 4:])), "the admitting sequence"
        _same_pool(pool, twin, ("admit", groups))


def test_commit_seq_stores_and_advances_the_named_members_only():
    dtype, D, G = torch.float16, 128, 1
    pool, twin = _forked("small", dtype, D, 100, 4, seed=700)
    slots, lengths, cs = [0, 1, 2, 3], [1, 4, 1, 2], [1, 0, 1, 0]
    for p in (pool, twin):
        p.reserve(slots, lengths)
    snap = pool.snapshot()
    reg = _regime(pool, snap, lengths, slots, [0, 4], G)
    assert reg["lg"] == [96]
    inp = GR.step_inputs(lengths, G, D, dtype, 710)
    o = pool.step(inp, lengths, slots, groups=[0, 4], commit_seq=cs)
    twin.step(inp, lengths, slots, commit_seq=cs)
    _check(pool, snap, reg, inp, o, lengths, slots, DECODE_TOL[dtype], "commit_seq")
    _same_pool(pool, twin, "commit_seq")
    assert pool.layer._dev_state[:4, 3].tolist() == [101, 100, 101, 100]


# ------------------------------------------------------------------ 3b. the two bounds of Lg that forks can hide
def test_a_shared_page_beyond_window_len_is_not_read():
    """a read-only step right after the fork, without reserve_pages: the third page (slots 64 .. 95) is mapped and the same
    in every row, but holds 2 tokens - Lg is capped by window_len = 66 at 64"""
    dtype, D, G = torch.bfloat16, 64, 8
    (pool,) = _forked("small", dtype, D, 70, 4, seed=1100, probe=True, twin=False)
    slots, lengths = [0, 1, 2, 3], [1] * 4
    snap = pool.snapshot()
    assert all(snap["table"][s][:3] == snap["table"][0][:3] and PR.mapped(snap["table"][0][2], pool.n_pages) for s in slots)
    reg = _regime(pool, snap, lengths, slots, [0, 4], G)
    assert reg["lg"] == [64]
    for probe in (None, _probe_spec(pool, snap, reg, lengths, slots, G)):
        inp = GR.step_inputs(lengths, G, D, dtype, 1110, probe=probe)
        o = pool.step(inp, lengths, slots, groups=[0, 4], commit=False)
        _check(pool, snap, reg, inp, o, lengths, slots, DECODE_TOL[dtype], ("page beyond window_len", probe is not None))


def test_a_diverged_page_inside_the_common_length_ends_the_shared_prefix():
    """every fork commits 31 tokens of its own: window_len = 97 everywhere, so three pages lie inside the common length,
    but the third (the LAST entry the compare looks at) is each fork's own: Lg = 64.  The step behind the divergence runs
    with randn inputs (30 of 101 keys differ between the forks) and with probes aimed INTO the diverged page (slots 70,
    80 and 90 of each fork's own ring): a kernel that took Lg = 96 reads the first member's page for every fork"""
    dtype, D, G = torch.bfloat16, 64, 8
    pool, twin = _forked("small", dtype, D, 70, 3, seed=1200, probe=True)
    slots = [0, 1, 2]
    for lengths, only in (([31] * 3, None), ([1] * 3, None), ([1] * 3, [70, 80, 90])):
        for p in (pool, twin):
            p.reserve(slots, lengths)
        snap = pool.snapshot()
        reg = _regime(pool, snap, lengths, slots, [0, 3], G)
        assert reg["lg"] == [64], reg["lg"]
        diverged = lengths[0] == 1
        if diverged:
            assert snap["states"][0][1] >= 97 and len({snap["table"][s][2] for s in slots}) == 3
            assert not torch.equal(snap["ring"][0][1][:, 70:96], snap["ring"][0][0][:, 70:96]), "the forks' own tokens differ"
        probe = _probe_spec(pool, snap, reg, lengths, slots, G, only=only) if (only or not diverged) else None
        inp = GR.step_inputs(lengths, G, D, dtype, 1210 + lengths[0] + (7 if only else 0), probe=probe)
        o = pool.step(inp, lengths, slots, groups=[0, 3])
        twin.step(inp, lengths, slots)
        _check(pool, snap, reg, inp, o, lengths, slots, DECODE_TOL[dtype], ("diverged page", lengths[0], only))
        _same_pool(pool, twin, "diverged page")


def test_the_table_compare_walks_more_than_one_round_of_pairs():
    """P = 32, Wc = 8192, a prompt of 4200 tokens forked into 8 slots: 8 members x 131 common entries are 1048 (member,
    entry) pairs, 24 of them in the second round of group_prep_kernel's compare - entries 107 .. 130 of the last member.
    Its entry 120 is pointed at a page of its own (planted bytes nobody else maps): Lg = 120 * 32, and the probes of every
    member aim into that page of their own ring.  A compare that lost the pair reads the first member's page for it"""
    dtype, D, G = torch.bfloat16, 64, 8
    (pool,) = _forked("wide", dtype, D, 4200, 8, seed=1300, twin=False)
    slots, lengths = list(range(8)), [1] * 8
    pool.reserve(slots, lengths)
    table = pool.layer.page_table
    lim = (4200 - NS) // 32
    assert lim == 131 and 8 * lim > 1024 and (1024 + 23) // lim == 7 and 1024 - 7 * lim <= 120 < lim
    spare = pool.n_pages - 1
    assert not (table == spare).any(), "the spare page must be unmapped"
    table[7, 120] = spare
    snap = pool.snapshot()
    reg = _regime(pool, snap, lengths, slots, [0, 8], G)
    assert reg["lg"] == [120 * 32], reg["lg"]
    for only in (None, [120 * 32 + 5, 120 * 32 + 31, 120 * 32]):
        inp = GR.step_inputs(lengths, G, D, dtype, 1310 + (1 if only else 0), probe=_probe_spec(pool, snap, reg, lengths, slots, G, only=only))
        o = pool.step(inp, lengths, slots, groups=[0, 8], commit=False)
        _check(pool, snap, reg, inp, o, lengths, slots, DECODE_TOL[dtype], ("second round of the compare", only))


def test_group_offsets_that_decrease_share_nothing_and_equal_the_ungrouped_call():
    """cu_g = [0, 4, 2, 6] (a device tensor: never read on the host) would make [0, 4) and [2, 6) overlap; the preparation
    launch then gives every group Lg = 0, and o is bitwise that of groups=None"""
    dtype, D, G = torch.bfloat16, 64, 8
    (pool,) = _forked("small", dtype, D, 70, 6, seed=1400, twin=False)
    slots, lengths = list(range(6)), [1] * 6
    pool.reserve(slots, lengths)
    snap = pool.snapshot()
    bad = [0, 4, 2, 6]
    assert _regime(pool, snap, lengths, slots, bad, G)["lg"] == [0, 0, 0]
    assert _regime(pool, snap, lengths, slots, [0, 4, 4, 6], G)["lg"] == [64, 0, 64]
    inp = GR.step_inputs(lengths, G, D, dtype, 1410)
    o = pool.step(inp, lengths, slots, groups=torch.tensor(bad, dtype=torch.int32, device=DEV), commit=False)
    plain = pool.step(inp, lengths, slots, commit=False)
    assert not torch.isnan(o.float()).any() and torch.equal(_bits(o), _bits(plain))
    good = pool.step(inp, lengths, slots, groups=[0, 4, 4, 6], commit=False)
    _check(pool, snap, _regime(pool, snap, lengths, slots, [0, 4, 4, 6], G), inp, good, lengths, slots, DECODE_TOL[dtype], "good offsets")


# ------------------------------------------------------------------ 4. the bitwise contracts
def test_groups_that_share_nothing_are_bitwise_the_ungrouped_call():
    """unrelated sequences grouped, a group with a wrapped member, a group of one: every Lg is 0, and o, pool and state are
    those of groups=None bit for bit"""
    dtype, D, G = torch.bfloat16, 64, 8
    pools = [Pool("small", dtype, D) for _ in range(2)]
    for p in pools:
        for s, L in ((0, 64), (1, 64), (4, 70)):
            p.prefill(s, *GR.prompt_kv(L, D, dtype, 800 + s, False))
        p.prefill(2, *GR.prompt_kv(300, D, dtype, 802, False))        # wrapped: 296 ring tokens on Wc = 128
        p.fork(2, [3])
    pool, twin = pools
    slots, lengths, groups = [0, 1, 2, 3, 4], [1, 2, 1, 1, 3], [0, 2, 4, 5]
    for p in pools:
        p.reserve(slots, lengths)
    snap = pool.snapshot()
    assert snap["states"][2][1] == 128, "slot 2 must be wrapped"
    reg = _regime(pool, snap, lengths, slots, groups, G)
    assert reg["lg"] == [0, 0, 0], reg["lg"]
    inp = GR.step_inputs(lengths, G, D, dtype, 810)
    o = pool.step(inp, lengths, slots, groups=groups)
    ot = twin.step(inp, lengths, slots)
    assert not torch.isnan(o.float()).any() and torch.equal(_bits(o), _bits(ot))
    _same_pool(pool, twin, "Lg = 0")


def test_o_does_not_depend_on_how_eight_forks_are_grouped():
    """same Lg, same plans; only a row's lane and block differ (MFMA columns are independent of each other)"""
    dtype, D, G = torch.bfloat16, 64, 8
    outs = []
    for groups in ([0, 8], [0, 4, 8], [0, 2, 4, 6, 8]):
        (pool,) = _forked("long", dtype, D, 700, 8, seed=900, twin=False)
        slots, lengths = list(range(8)), [1] * 8
        pool.reserve(slots, lengths)
        reg = _regime(pool, pool.snapshot(), lengths, slots, groups, G)
        assert reg["lg"] == [640] * (len(groups) - 1)
        # n_grp enters want_g: the plan must still be the same for the contract to be bitwise
        assert GR.group_plan(640, len(groups) - 1, HKV * G, HKV, 8) == GR.group_plan(640, 1, HKV * G, HKV, 8)
        outs.append(pool.step(GR.step_inputs(lengths, G, D, dtype, 910), lengths, slots, groups=groups, commit=False))
    assert torch.equal(_bits(outs[0]), _bits(outs[1])) and torch.equal(_bits(outs[0]), _bits(outs[2]))


# ------------------------------------------------------------------ 5. graph replay and determinism
def test_one_captured_graph_replays_at_three_groupings_and_two_runs_agree():
    dtype, D, G = torch.bfloat16, 64, 8
    (pool,) = _forked("small", dtype, D, 70, 6, seed=1000, twin=False)
    for s in (6, 7):
        pool.prefill(s, *GR.prompt_kv(64, D, dtype, 1000 + s, False))
    slots, lengths = list(range(8)), [1] * 8
    pool.reserve(slots, lengths)
    inp = GR.step_inputs(lengths, G, D, dtype, 1010)
    q, k, v, sa = (t.to(DEV) for t in inp)
    cu = torch.tensor(_cu(lengths), dtype=torch.int32, device=DEV)
    sl = torch.tensor(slots, dtype=torch.int32, device=DEV)
    groupings = ([0, 6, 8, 8], [0, 3, 6, 8], [6, 7, 8, 8])      # the last: two groups of one, every Lg 0
    cu_g = torch.tensor(groupings[0], dtype=torch.int32, device=DEV)
    out = torch.empty_like(q)
    L = pool.layer
    eager = []
    for gr in groupings:
        eager.append(L.ragged_step_dyn(q, k, v, cu, sl, s_aux=sa, commit=False, groups=gr).clone())
        again = L.ragged_step_dyn(q, k, v, cu, sl, s_aux=sa, commit=False, groups=gr)
        assert torch.equal(_bits(eager[-1]), _bits(again)), "two runs differ"
    plain = L.ragged_step_dyn(q, k, v, cu, sl, s_aux=sa, commit=False)
    assert torch.equal(_bits(eager[2]), _bits(plain)), "all Lg 0: the ungrouped call"
    snap = pool.snapshot()
    assert _regime(pool, snap, lengths, slots, groupings[0], G)["lg"] == [64, 0, 0]
    assert _regime(pool, snap, lengths, slots, groupings[1], G)["lg"] == [64, 64, 0]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        L.ragged_step_dyn(q, k, v, cu, sl, s_aux=sa, out=out, commit=False, groups=cu_g)      # warm-up: workspace
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        L.ragged_step_dyn(q, k, v, cu, sl, s_aux=sa, out=out, commit=False, groups=cu_g)
    for gr, want in zip(groupings, eager):
        cu_g.copy_(torch.tensor(gr, dtype=torch.int32))
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(out), _bits(want)), ("replay at", gr)
