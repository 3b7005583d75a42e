"""CPU-only tests of SFA_FLAG_RAGGED_CHUNK128: the flag and the workspace query in the header and the library, the size
of the workspace, and the ownership rule of the 128-row block table, restated."""
import os
import random
import re

import pytest
import torch

from sink_attention import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HKV, NKV = 2, 100


def test_the_flag_and_the_symbol_are_in_the_header_and_the_library():
    hdr = open(os.path.join(ROOT, "include", "sfa.h")).read()
    assert re.search(r"#define SFA_FLAG_RAGGED_CHUNK128 0x80u\b", hdr) and N.FLAG_RAGGED_CHUNK128 == 0x80
    assert re.search(r"size_t sfa_decode_ragged_chunk_workspace_bytes\(int64_t n_seq,", hdr)
    assert len(N.lib().sfa_decode_ragged_chunk_workspace_bytes.argtypes) == 7 and N.lib().sfa_abi_version() == 2


@pytest.mark.parametrize("G,T,n_seq,D", [(8, 1024, 9, 64), (1, 320, 9, 128), (3, 130, 1, 80), (4, 7, 3, 96)])
def test_the_workspace_is_the_ungrouped_one_plus_the_aligned_table(G, T, n_seq, D):
    chunk, plain = N.lib().sfa_decode_ragged_chunk_workspace_bytes, N.lib().sfa_decode_ragged_workspace_bytes
    bf, f16, f32 = (N.SFA_DTYPE[t] for t in (torch.bfloat16, torch.float16, torch.float32))
    nwb = -(-G * T // 128) + n_seq
    for dt in (bf, f16):
        a = (n_seq, G * HKV, HKV, T, NKV, D, dt)
        assert chunk(*a) == plain(*a) + -(-nwb * 8 // 256) * 256 and plain(*a) > 0
    assert plain(n_seq, G * HKV, HKV, T, NKV, D, f32) > 0 and chunk(n_seq, G * HKV, HKV, T, NKV, D, f32) == 0
    assert plain(n_seq, G * HKV, HKV, T, NKV, 48, bf) > 0 and chunk(n_seq, G * HKV, HKV, T, NKV, 48, bf) == 0


def wblk_rule(G, lengths, T):
    """ragged_prep_chunk_kernel's table: a chunk sequence owns ids [G c0_i // 128 + i, + ceil(G n_i / 128)); else (-1, 0)"""
    tab, c0 = [[-1, 0] for _ in range(-(-G * T // 128) + len(lengths))], 0
    for i, n in enumerate(lengths):
        for j in range(-(-G * n // 128) if G * n >= 128 else 0):
            assert tab[G * c0 // 128 + i + j] == [-1, 0], ("two owners", G, lengths, i, j)
            tab[G * c0 // 128 + i + j] = [i, j]
        c0 += n
    return tab


@pytest.mark.parametrize("G", [1, 3, 8])
def test_the_block_ids_of_chunk_sequences_are_disjoint_covered_and_fit_the_workspace(G):
    """arithmetic about the rule (tests/test_gpu_ragged_chunk.py holds the device's table to wblk_rule): no id has two
    owners or lies past nwb, every block of a chunk sequence has one, the bytes the library adds hold the table"""
    chunk, plain = N.lib().sfa_decode_ragged_chunk_workspace_bytes, N.lib().sfa_decode_ragged_workspace_bytes
    rnd = random.Random(G)
    for _ in range(300):
        lengths = [rnd.choice([0, 1, 2, 17, 42, 43, 127, 128, 129, 300, rnd.randint(0, 600)]) for _ in range(rnd.randint(1, 12))]
        T = sum(lengths) + rnd.randint(1, 50)
        tab = wblk_rule(G, lengths, T)
        assert sum(e[0] >= 0 for e in tab) == sum(-(-G * n // 128) for n in lengths if G * n >= 128)
        a = (len(lengths), G * HKV, HKV, T, NKV, 64, N.SFA_DTYPE[torch.bfloat16])
        assert 0 <= chunk(*a) - plain(*a) - 8 * len(tab) < 256
