"""tests/group_regime.py against hand-built states and tables, against the library's workspace function, and against
itself: the cases of tests/test_gpu_group_step.py reach what they are there for, and three mutants of the kernels move the
probe inputs by at least ten tolerances (oracle against mutated oracle, no GPU)."""
import pytest
import torch

import group_regime as GR
from sink_attention import _native as N
from sink_attention.cache import group_offsets
from util import DECODE_TOL

P, WC, NPG = 32, 128, 16


def _lg(states, table, lengths, slots, cu_g, admit=False, cu_q=None):
    cu = [0]
    for n in lengths:
        cu.append(cu[-1] + n)
    cu_q = cu if cu_q is None else cu_q
    return GR.prep(cu_q, cu_g, slots, states, table, NPG, P, WC, cu[-1], 8, admit)


def _forks(n, wl, shared_pages, own_from=100):
    """n slots at window_len wl (unwrapped, seen = wl + 4) whose first `shared_pages` table entries are pages 0, 1, ... and
    whose further entries up to the write page are each slot's own"""
    states = [[4, wl, wl, wl + 4] for _ in range(n)]
    per = WC // P
    need = -(-(wl + 1) // P)
    table = [[j if j < shared_pages else (4 + s * per + j if j < need else -1) for j in range(per)] for s in range(n)]
    return states, table


def test_forks_share_the_pages_in_front_of_the_write_page():
    states, table = _forks(4, 66, 2)
    r = _lg(states, table, [1] * 4, [0, 1, 2, 3], [0, 4])
    assert r["lg"] == [64] and r["first"] == [0] and r["gseq"] == [0] * 4


@pytest.mark.parametrize("j", [0, 1, 2])
def test_tables_that_diverge_at_entry_j_share_j_pages(j):
    states, table = _forks(3, 100, 3)
    table[2][j] = 15                      # mapped, but another page
    assert _lg(states, table, [1] * 3, [0, 1, 2], [0, 3])["lg"] == [j * P]
    table[2][j] = table[0][j]
    table[0][j] = -1                      # the first member's entry is unmapped
    assert _lg(states, table, [1] * 3, [0, 1, 2], [0, 3])["lg"] == [j * P]
    table[0][j] = NPG                     # ... or past the pool
    assert _lg(states, table, [1] * 3, [0, 1, 2], [0, 3])["lg"] == [j * P]


def test_a_member_below_the_common_pages_caps_lg_at_its_window_len():
    """three mapped pages are the same in every row, but one member holds 40 ring tokens: the second page is shared and
    partly empty for it"""
    states, table = _forks(3, 100, 3)
    states[1] = [4, 40, 40, 44]
    assert _lg(states, table, [1] * 3, [0, 1, 2], [0, 3])["lg"] == [32]
    states[1] = [4, 20, 20, 24]
    assert _lg(states, table, [1] * 3, [0, 1, 2], [0, 3])["lg"] == [0]


def test_a_wrapped_member_or_one_that_wraps_within_the_step_shares_nothing():
    states, table = _forks(3, 100, 3)
    states[2] = [4, 128, 7, 500]
    assert _lg(states, table, [1] * 3, [0, 1, 2], [0, 3])["lg"] == [0]
    states[2] = [4, 100, 100, 104]
    assert _lg(states, table, [1, 1, 28], [0, 1, 2], [0, 3])["lg"] == [96]          # 100 + 28 = Wc: still unwrapped
    assert _lg(states, table, [1, 1, 29], [0, 1, 2], [0, 3])["lg"] == [0]
    states[2] = [4, 100, 3, 104]                                                     # write_pos != window_len below Wc
    assert _lg(states, table, [1] * 3, [0, 1, 2], [0, 3])["lg"] == [0]


def test_an_admitting_member_makes_lg_zero_only_under_the_flag():
    states, table = _forks(3, 100, 3)
    states[1] = [4, 100, 100, 0]          # seen == 0: fresh
    assert _lg(states, table, [1] * 3, [0, 1, 2], [0, 3], admit=True)["lg"] == [0]
    assert _lg(states, table, [1] * 3, [0, 1, 2], [0, 3], admit=False)["lg"] == [96]


def test_inactive_and_empty_members_are_skipped_and_one_member_is_no_group():
    states, table = _forks(4, 100, 3)
    states[3] = [4, 128, 9, 999]          # wrapped, but inactive or empty below
    assert _lg(states, table, [1, 1, 1, 1], [0, 1, 2, -1], [0, 4])["lg"] == [96]
    assert _lg(states, table, [1, 1, 1, 0], [0, 1, 2, 3], [0, 4])["lg"] == [96]
    assert _lg(states, table, [1, 1, 1, 1], [0, 1, 2, 99], [0, 4])["lg"] == [96]
    r = _lg(states, table, [0, 1, 1, 0], [0, 1, 2, 3], [0, 4])
    assert r["lg"] == [96] and r["first"] == [1]                                    # the first MEMBER's row is the yardstick
    assert _lg(states, table, [1, 0, 0, 0], [0, 1, 2, 3], [0, 4])["lg"] == [0]
    assert _lg(states, table, [1, 1, 1, 1], [0, -1, -1, -1], [0, 4])["lg"] == [0]
    assert _lg(states, table, [1, 1, 1, 1], [0, 1, 2, 3], [0, 1, 2, 3, 4])["lg"] == [0, 0, 0, 0]


def test_bad_cu_g_is_clamped_pairwise_and_never_leaves_the_pack():
    states, table = _forks(4, 100, 3)
    r = _lg(states, table, [1] * 4, [0, 1, 2, 3], [-5, 9])
    assert r["lg"] == [96] and r["gseq"] == [0] * 4
    r = _lg(states, table, [1] * 4, [0, 1, 2, 3], [3, 1, 4])         # decreasing: groups could overlap, nothing is shared
    assert r["lg"] == [0, 0] and r["gseq"] == [-1, 1, 1, 1]
    assert _lg(states, table, [1] * 4, [0, 1, 2, 3], [0, 4, 2, 4])["lg"] == [0, 0, 0]     # [0, 4) and [2, 4) overlap
    assert _lg(states, table, [1] * 4, [0, 1, 2, 3], [0, 2, 2, 4])["lg"] == [96, 0, 96]
    r = _lg(states, table, [1] * 4, [0, 1, 2, 3], [2, 2, 2])
    assert r["lg"] == [0, 0] and r["gseq"] == [-1] * 4 and all(b == (-1, 0) for b in r["gblk"])
    # offsets of the pack that are not monotonic: a member's rows leave the group's span -> nothing shared
    r = _lg(states, table, [1] * 4, [0, 1, 2, 3], [0, 4], cu_q=[2, 3, 0, 1, 4])
    assert r["lg"] == [0]


def test_group_row_blocks_are_disjoint_and_below_the_bound():
    for G, lengths, cu_g in ((8, [1] * 8, [0, 8]), (8, [3, 3, 0, 40, 1, 1], [0, 6]), (1, [3, 3, 0, 40, 1, 1], [0, 2, 6]),
                             (8, [1, 1, 2, 1, 1, 1, 3, 1, 1], [0, 1, 4, 8, 9]), (3, [5, 7, 11, 2], [0, 1, 1, 4])):
        cu = [0]
        for n in lengths:
            cu.append(cu[-1] + n)
        states, table = _forks(len(lengths), 60, 1)
        r = GR.prep(cu, cu_g, list(range(len(lengths))), states, table, NPG, P, WC, cu[-1], G)     # asserts disjointness
        for g in range(len(cu_g) - 1):
            _, _, _, n = GR.group_span(cu, cu_g, g, len(lengths), cu[-1])
            assert sum(1 for b in r["gblk"] if b[0] == g) == -(-G * n // 32)


def test_group_offsets():
    assert group_offsets([0, 0, 0, 1, 1]) == [0, 3, 5]
    assert group_offsets([None, "a", "a", None, None, "b"]) == [0, 1, 3, 4, 5, 6]
    assert group_offsets([-1, 7]) == [0, 1, 2]
    with pytest.raises(ValueError, match="not consecutive"):
        group_offsets([0, 1, 0])


# ------------------------------------------------------------------ the GPU cases reach what they are there for
def test_the_long_geometry_has_several_group_splits_and_multi_tile_wave_walks():
    lg = GR.expected_lg("long", 700)
    assert lg == 640
    for G in (1, 8):
        p = GR.group_plan(lg, 1, GR.HKV * G, GR.HKV, 8)
        assert p["T"] == 20 and p["S"] >= 2 and p["tps"] >= 4, p
        assert p == GR.group_plan(lg, 2, GR.HKV * G, GR.HKV, 8) == GR.group_plan(lg, 4, GR.HKV * G, GR.HKV, 8)
    assert [GR.expected_lg("small", L) for L in GR.PROMPTS["small"]] == [64, 32, 96]


def test_the_packs_hold_full_partial_and_straddled_group_blocks():
    assert 8 * 8 == 2 * 32                                   # 8 forks at G = 8: two full group row blocks
    assert 5 * 8 % 32 != 0 and 3 * 1 < 32                    # 5 forks at G = 8, 3 forks at G = 1: a partial last block
    for G, who in ((8, 1), (1, 3)):                          # lengths [3, 3, 0, 40, 1, 1]: a member over a block boundary
        cu = [0, 3, 6, 6, 46, 47, 48]
        lo, hi = G * cu[who], G * cu[who + 1] - 1
        assert lo // 32 != hi // 32, (G, who)


@pytest.mark.parametrize("args", [(8, 1, 16, 2, 8, 1028, 64), (8, 4, 16, 2, 8, 132, 128), (6, 1, 2, 2, 48, 132, 80),
                                  (9, 4, 16, 2, 12, 132, 96), (1, 1, 64, 8, 1, 131076, 64), (300, 50, 8, 8, 2000, 4100, 128)])
def test_the_workspace_function_is_the_python_restatement(args):
    for dt in (N.SFA_DTYPE[torch.bfloat16], N.SFA_DTYPE[torch.float16]):
        assert N.lib().sfa_decode_ragged_group_workspace_bytes(*args, dt) == GR.group_workspace_bytes(*args)
    n_seq, n_grp, Hq, Hkv, T, Nkv, D = args
    assert GR.ragged_workspace_bytes(n_seq, Hq, Hkv, T, Nkv, D) == N.lib().sfa_decode_ragged_workspace_bytes(n_seq, Hq, Hkv, T, Nkv, D, 2)


# ------------------------------------------------------------------ three mutants miss the tolerance tenfold on the probes
@pytest.mark.parametrize("geom,dt,D,G", [("small", "bf16", 64, 8), ("small", "fp16", 128, 1), ("long", "bf16", 64, 8),
                                         ("long", "fp16", 128, 8)])
def test_three_mutants_move_the_probes_by_ten_tolerances(geom, dt, D, G):
    dtype, prompt, n = GR.DT[dt], GR.PROMPTS[geom][0], 4
    lg, wl = GR.expected_lg(geom, prompt), prompt - GR.NS
    k, v = GR.prompt_kv(prompt, D, dtype, 7, True)
    sink, ring = (k[0, :, :GR.NS], v[0, :, :GR.NS]), (k[0, :, GR.NS:], v[0, :, GR.NS:])
    tps = GR.group_plan(lg, 1, GR.HKV * G, GR.HKV, n)["tps"]
    spec = {i: (ring[0], GR.probe_targets(lg, wl, tps)) for i in range(n)}
    q, kn, vn, sa = GR.step_inputs([1] * n, G, D, dtype, 8, probe=spec)
    ref = [GR.oracle_seq(q, kn, vn, sa, sink, ring, GR.NS, wl, i, 1, G, lg) for i in range(n)]
    same = [GR.oracle_seq(q, kn, vn, sa, sink, ring, GR.NS, wl, i, 1, G, 0) for i in range(n)]
    assert max((a - b).abs().max().item() for a, b in zip(ref, same)) < 1e-12, "Lg only regroups the keys"
    for m in GR.MUTANTS:
        moved = max((GR.oracle_seq(q, kn, vn, sa, sink, ring, GR.NS, wl, i, 1, G, lg, mutant=m, q_first_row=0) - ref[i]).abs().max().item()
                    for i in range(n))
        print(geom, dt, D, G, m, "moves the probes by", moved, "tolerances:", moved / DECODE_TOL[dtype])
        assert moved >= 10 * DECODE_TOL[dtype], (m, moved)
