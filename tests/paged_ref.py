"""The page arithmetic of a paged slot pool (include/sfa.h), restated in Python for the tests.

A paged pool keeps its ring in pages [n_pages, H_kv, P, D] and a table [S, Wc / P]: entry [s][j] is the page that holds
ring slots [j P, (j + 1) P) of slot s; an entry e with not 0 <= e < n_pages is unmapped (-1 by convention).  The TWIN of a
paged pool is the contiguous pool gather() builds; the contract of the paged calls is two bitwise equalities against it.
The prefix rule: a slot whose ring has held at most r tokens touches table entries 0 .. ceil(min(r, Wc) / P) - 1 only."""
import torch


def pages_needed(tokens, Wc, P):
    """table entries a ring that has held at most `tokens` tokens touches (the prefix rule)"""
    return -(-min(max(int(tokens), 0), Wc) // P)


def mapped(e, n_pages):
    return 0 <= int(e) < n_pages


def gather(pages, table):
    """[n_pages, H_kv, P, D] pages and an int table [S, Wc / P] -> the twin's ring [S, H_kv, Wc, D]; unmapped pages read
    as zeros"""
    n_pages, H, P, D = pages.shape
    S, per = table.shape
    out = torch.zeros(S, H, per * P, D, dtype=pages.dtype, device=pages.device)
    tab = table.tolist()
    for s in range(S):
        for j in range(per):
            if mapped(tab[s][j], n_pages):
                out[s, :, j * P:(j + 1) * P] = pages[tab[s][j]]
    return out


def scatter(window, table, pages):
    """the inverse on the mapped entries: pages[table[s][j]] <- window[s, :, j P : (j + 1) P], in place; other pages keep
    their content.  Returns pages."""
    P = pages.shape[2]
    tab = table.tolist()
    for s in range(len(tab)):
        for j, e in enumerate(tab[s]):
            if mapped(e, pages.shape[0]):
                pages[e] = window[s, :, j * P:(j + 1) * P]
    return pages


# ---- the placements, slot by slot (csrc/sfa_decode_multi.hip: fill_place / fill_src, commit_piece_ragged)
def prefill_ring_slots(L, ns, Wc):
    """ring slots a prefill (or an admission) of L tokens writes: with rem = L - min(L, ns), slots [0, rem) when
    rem <= Wc, else every slot"""
    rem = L - min(L, ns)
    return list(range(rem if rem <= Wc else Wc))


def prefill_state(L, ns, Wc):
    sl = min(L, ns)
    rem = L - sl
    return [sl, min(rem, Wc), rem if rem < Wc else 0, L]


def commit_ring_slots(state, n, Wc):
    """ring slots a commit of n tokens writes at `state` = [sink_len, window_len, write_pos, seen]: token t >= n - Wc goes to
    (write_pos + t) mod Wc.  Returns (slots, state after)."""
    sl, wl, wp, seen = state
    slots = [(wp + t) % Wc for t in range(max(0, n - Wc), n)]
    return slots, [sl, min(wl + n, Wc), (wp + n) % Wc, seen + n]


def read_ring_slots(state):
    """ring slots an attention call reads at `state`: [0, window_len)"""
    return list(range(state[1]))
