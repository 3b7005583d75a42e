"""The packed step at head dim 256 (multi_split_mfma_d256_kernel) on the four pool kinds: 16-bit, FP8,
paged, paged FP8.  Pools, packs and oracles are those of tests/test_gpu_ragged_tree.py, test_gpu_fp8_pool.py,
test_gpu_paged_pool.py and test_gpu_paged_fp8_pool.py: 8 slots, H_kv 2, num_sink 4, Wc 16 / 48 contiguous and (Wc, P) =
(64, 32) / (96, 32) paged, lengths [1, 7, 0, 16, 33, 64, 110] with an inactive and an empty sequence.  A pair of waves
sees at most two tiles there; the `walk` pack (Wc 320, at least 16 tiles per split) runs the loop body of every pair many
times.  DECODE_TOL does not grow with D: an output element is a convex combination of V elements."""
import pytest
import torch

import packed_regime as R
import test_gpu_packed_long as PL
import test_gpu_paged_fp8_pool as P8
from fp8_ref import dequant, quant
from oracle import sink_oracle as O
from test_gpu_fp8_pool import K_SCALE, SCALES, V_SCALE, _dequant_pool, _fp8_pool
from test_gpu_paged_pool import ADMIT, LENGTHS, PLAIN, T_PAD, _base, _paged, _trees
from test_gpu_ragged_tree import NS, _check_rows, _cu, _i32, _oracle, _pack, _parents, _pool, _run, _same_pool
from test_gpu_slots import _clone, _dev_slots, _path
from test_ragged_tree_host import chain
from util import DECODE_TOL, maxdiff

pytestmark = pytest.mark.gpu
DEV, D = "cuda", 256
KINDS = ["16", "fp8", "paged", "paged_fp8"]
GRID = [(kind, dt, G, geo) for kind in KINDS for dt, G in ((torch.bfloat16, 8), (torch.float16, 1)) for geo in (0, 1)]
CU = _cu(LENGTHS)
FRESH = [i for i, s in enumerate(ADMIT) if s in (6, 7)]      # the sequences of 33 and 110 tokens: on the fresh slots


def _make(kind, dtype, geo, seed):
    """(pool, the history as it reads back, Wc, the pools that must give the pool's bits) for one kind of pool"""
    W, P = ((16, None), (48, None))[geo] if "paged" not in kind else ((64, 32), (96, 32))[geo]
    if kind == "fp8":
        pool, hist = _fp8_pool(dtype, D, W, seed, fresh=(6, 7))
        dq = lambda kv: (dequant(quant(kv[0], K_SCALE), K_SCALE, dtype), dequant(quant(kv[1], V_SCALE), V_SCALE, dtype))
        return pool, {s: dict(pre=dq(h["pre"]), com=dq(h["com"])) for s, h in hist.items()}, W, [_dequant_pool(pool, dtype, SCALES)]
    if kind == "paged_fp8":
        b8, hist = P8._base8(dtype, D, W, seed, SCALES)
        pg, tw = P8._paged8(b8, dtype, P, seed + 1)
        return pg, hist, W, [tw, P8._deq_paged(pg, dtype, SCALES)]
    if kind == "16":
        return _pool(dtype, D, W, seed, fresh=(6, 7)) + (W, [])
    base, hist = _base(dtype, D, W, seed)
    pg, tw = _paged(base, P, seed + 1)
    return pg, hist, W, [tw]


def _ref(q, k, v, sa, hist, W, slots, trees):
    """the fp64 rows: a continuing sequence over its history, an admitting one (a fresh slot) as a prefill of its chunk"""
    ref = _oracle(q, k, v, sa, hist, W, LENGTHS, [-1 if slots is ADMIT and i in FRESH else s for i, s in enumerate(slots)], trees)
    for i in FRESH if slots is ADMIT else []:
        sel = slice(CU[i], CU[i + 1])
        ref[i] = O.sink_attention_dense(q[:, :, sel], k[:, :, sel], v[:, :, sel], NS, W, sa)[0]
    return ref


# ------------------------------------------------------------------ 1. the oracle, plain and admitting
@pytest.mark.parametrize("kind,dtype,G,geo", GRID)
def test_plain_and_admitting_steps_are_the_oracle(kind, dtype, G, geo):
    pool, hist, W, _ = _make(kind, dtype, geo, seed=301)
    q, k, v, sa = _pack(dtype, D, G, T_PAD, seed=302)
    for slots in (PLAIN, ADMIT):
        o = _run(pool, q, k, v, CU, slots, sa=sa, admit=slots is ADMIT)
        assert "_mfma_" in _path() and "_d256_" in _path(), _path()
        ref = _ref(q, k, v, sa, hist, W, slots, [chain(n) for n in LENGTHS])
        assert len(ref) == 5
        _check_rows(o, ref, LENGTHS, DECODE_TOL[dtype], (kind, dtype, G, W, "admit", slots is ADMIT))


# ------------------------------------------------------------------ 2. trees; a chain is the plain call
@pytest.mark.parametrize("kind,dtype,G,geo", GRID)
def test_trees_are_the_oracle_and_a_chain_is_bitwise_the_plain_call(kind, dtype, G, geo):
    pool, hist, W, _ = _make(kind, dtype, geo, seed=311)
    q, k, v, sa = _pack(dtype, D, G, T_PAD, seed=312)
    trees = _trees()
    o = _run(pool, q, k, v, CU, PLAIN, _parents(LENGTHS, trees, T_PAD), sa=sa)
    assert _path().startswith("decode_tree_mfma_") and "_d256_" in _path(), _path()
    _check_rows(o, _ref(q, k, v, sa, hist, W, PLAIN, trees), LENGTHS, DECODE_TOL[dtype], (kind, dtype, G, W, "trees"))
    for admit in (False, True):
        slots = ADMIT if admit else PLAIN
        a = _run(pool, q, k, v, CU, slots, sa=sa, admit=admit).clone()
        b = _run(pool, q, k, v, CU, slots, _parents(LENGTHS, [chain(n) for n in LENGTHS], T_PAD, stale=-7), sa=sa, admit=admit)
        assert torch.equal(a, b), (admit, maxdiff(a, b))


# ------------------------------------------------------------------ 3. bitwise twins
@pytest.mark.parametrize("kind,dtype,G,geo", GRID)
def test_bitwise_twins(kind, dtype, G, geo):
    q, k, v, sa = _pack(dtype, D, G, T_PAD, seed=322)
    par = _parents(LENGTHS, _trees(), T_PAD)
    step = lambda p: _run(p, q, k, v, CU, ADMIT, par, sa=sa, admit=True)
    pool, _, W, twins = _make(kind, dtype, geo, seed=321)
    o = step(pool).clone()
    assert "_mfma_" in _path() and "_d256_" in _path() and not torch.isnan(o).any() and o.any(), _path()
    assert torch.equal(step(pool), o), "two runs"
    for n, tw in enumerate(twins):      # the contiguous twin of a paged pool; the 16-bit pool over the dequantised codes
        ot = step(tw)
        assert torch.equal(ot, o), (kind, "twin", n, _path(), maxdiff(ot, o))
    for i in (4, 5, 6):                 # 33 (admitting), 64 (a tree), 110 (admitting) tokens: alone at the head of the pack
        n = LENGTHS[i]
        q1, k1, v1 = (torch.zeros_like(t) for t in (q, k, v))
        q1[:, :, :n], k1[:, :, :n], v1[:, :, :n] = q[:, :, CU[i]:CU[i + 1]], k[:, :, CU[i]:CU[i + 1]], v[:, :, CU[i]:CU[i + 1]]
        alone = _run(pool, q1, k1, v1, _cu([n if j == i else 0 for j in range(len(LENGTHS))]), ADMIT,
                     par[CU[i]:CU[i + 1]] + [3] * (T_PAD - n), sa=sa, admit=True)
        assert torch.equal(alone[:, :, :n], o[:, :, CU[i]:CU[i + 1]]) and not alone[:, :, n:].any(), ("alone", i)
    if kind == "16":                    # the commit does not depend on the split kernel
        a, b = _clone(pool), _clone(pool)
        a._pool = b._pool = True
        args = (q.to(DEV), k.to(DEV), v.to(DEV), _i32(CU), _dev_slots(ADMIT))
        oa = a.ragged_step_dyn(*args, s_aux=sa.to(DEV), commit=True, admit=True)
        assert "_mfma_" in _path(), _path()
        ob = b.ragged_step_dyn(*args, s_aux=sa.to(DEV), commit=True, admit=True, force_generic=True)
        assert "_f32_" in _path() and "_d256_" in _path(), _path()
        _same_pool(a, b, "pool and state rows after a committing step, MFMA and f32 kernel")
        assert not torch.equal(a._dev_state, pool._dev_state) and maxdiff(oa, ob) <= 2 * DECODE_TOL[dtype]


# ------------------------------------------------------------------ 4. the walk: at least 16 tiles per split
@pytest.mark.parametrize("dt,data", [("bf16", "randn"), ("fp16", "probe"), ("bf16", "probe"), ("fp16", "randn")])
def test_the_walk_pack_runs_every_pairs_loop_many_times(dt, data):
    inp = R.pack_inputs("walk", data, dt, D)
    case = inp["case"]
    assert (case["Hkv"], case["G"], case["Wc"]) == (8, 8, 320)
    base = PL._pool(inp)
    pg, _ = _paged(base, 64, seed=331)
    outs = []
    for pool in (base, pg):
        rg = PL._reaches(case, pool, case["T_PAD"])          # from the device's state rows: want 1, some tps >= 16
        assert max(r["tps"] for r in rg) >= 9
        outs.append(PL._run(pool, inp))
        assert "_mfma_" in _path() and "_d256_" in _path() and _path().endswith("_paged") == (pool is pg), _path()
        _check_rows(outs[-1], PL._ref("walk", data, dt, D), case["lengths"], PL.TOL[inp["dtype"]], ("walk", dt, data))
    assert torch.equal(outs[0], outs[1]), "the paged pool is its contiguous twin"


# ------------------------------------------------------------------ 5. what stays refused, what stays f32
def test_groups_chunk_kernel_fp32_and_force_generic_at_256():
    q, k, v, sa = _pack(torch.bfloat16, D, 8, T_PAD, seed=342)
    args = (q.to(DEV), k.to(DEV), v.to(DEV), _i32(CU), _dev_slots(PLAIN))
    base, _, _, _ = _make("16", torch.bfloat16, 0, seed=341)
    pg, _, _, _ = _make("paged", torch.bfloat16, 0, seed=341)
    before = _clone(base)
    with pytest.raises(RuntimeError, match="a paged pool serves bf16 / f16 at head dims 64 / 80 / 96 / 128 .*head dim 256"):
        pg.ragged_step_dyn(*args, groups=[0, 3, 7])
    for pool in (base, pg):
        with pytest.raises(RuntimeError, match="SFA_FLAG_RAGGED_CHUNK128 serves bf16 / f16 at head dims 64 / 80 / 96 / 128"):
            pool.ragged_step_dyn(*args, chunk_kernel=True)
    _same_pool(base, before, "a refused call moves nothing")
    base.ragged_step_dyn(*args, commit=False, force_generic=True)
    assert _path().startswith("decode_multi_f32_bf16_d256_ragged"), _path()
    f32, _, _, _ = _make("16", torch.float32, 0, seed=343)
    f32.ragged_step_dyn(*(t.float() if t.is_floating_point() else t for t in args), commit=False)
    assert _path().startswith("decode_multi_f32_f32_d256_ragged"), _path()
