"""Draft-tree helpers for tree-structured speculative decoding (Medusa / EAGLE / SpecInfer) over the sink + ring cache.

A chunk of n <= 64 draft nodes is a forest given by ``parent`` ([..., n] integer tensor): ``parent[u]`` in [-1, u), -1 = a
root hanging directly off the cache; any other value reads as -1, exactly as the kernels read it
(``SinkCacheLayer.extend_attention_tree*``).  Every helper is a handful of torch ops on the tensors' own device with no
host sync (no ``.item()``, no data-dependent shapes), so a whole verify / accept / commit step captures into one graph:

    depth = tree_depth(parent)                                  # RoPE position of node u: seen + depth[u]
    out = layer.extend_attention_tree_dyn(q, k, v, parent)      # every layer
    path, count = greedy_accept(parent, draft_tokens, target_tokens)
    layer.commit_path_dyn(k, v, path, count)                    # every layer

Packed steps (``SinkCacheLayer.ragged_step_dyn(parent=, commit_seq=)``): ``parent`` is one ``[T]`` array packed like q
with sequence-local entries, and a sequence of at most ``MAX_TREE`` = 64 tokens is a tree.  The ``packed_*`` helpers
scatter the pack into ``[n_seq, 64]`` rows, run the helpers above and gather back, with the same no-sync rule:

    pos = layer.packed_positions(cu_q, slots, T) - packed_local(cu_q, T) + packed_tree_depth(parent, cu_q, T)
    out = layer.ragged_step_dyn(q, k, v, cu_q, slots, admit=True, parent=parent, commit_seq=commit_seq)
    path, count = greedy_accept_packed(parent, draft_tokens, target_tokens, cu_q, n_seq)
    layer.commit_packed_dyn(k, v, cu_q, slots, count * (1 - commit_seq), path)
"""
import torch


def _parent(parent: torch.Tensor) -> torch.Tensor:
    """``parent`` as int64 with the entries outside [-1, u) read as -1 (the kernels' rule)."""
    p = parent.long()
    u = torch.arange(p.shape[-1], device=p.device)
    return torch.where((p >= -1) & (p < u), p, torch.full_like(p, -1))


def _rounds(n: int) -> int:
    return max(1, (n - 1).bit_length())       # pointer jumping: 2^rounds > the deepest depth (n - 1)


def tree_depth(parent: torch.Tensor) -> torch.Tensor:
    """depth[u] (int64, ``parent``'s shape): 0 for a root, depth[parent[u]] + 1 otherwise.  Pointer jumping: after round
    r, j = the 2^r-th ancestor (-1 past the root) and d = the edges from u up to j (to the root when j = -1)."""
    p = _parent(parent)
    j, d = p, (p >= 0).long()
    for _ in range(_rounds(p.shape[-1])):
        live = j >= 0
        jc = j.clamp(min=0)
        d = torch.where(live, d + d.gather(-1, jc), d)
        j = torch.where(live, j.gather(-1, jc), j)
    return d


def tree_ancestor_mask(parent: torch.Tensor) -> torch.Tensor:
    """bool [..., n, n]: ``mask[..., u, v]`` iff v is u or one of its ancestors."""
    p = _parent(parent)
    n = p.shape[-1]
    anc = torch.eye(n, dtype=torch.bool, device=p.device).expand(*p.shape, n).clone()
    j = p
    for _ in range(_rounds(n)):
        live = j >= 0
        jc = j.clamp(min=0)
        rows = anc.gather(-2, jc.unsqueeze(-1).expand(*jc.shape, n))       # anc[j[u]]
        anc = anc | (rows & live.unsqueeze(-1))
        j = torch.where(live, j.gather(-1, jc), j)
    return anc


def greedy_accept(parent: torch.Tensor, draft_tokens: torch.Tensor, target_tokens: torch.Tensor):
    """Greedy acceptance of a draft tree rooted at node 0.

    ``parent`` [n] or [B, n]; ``draft_tokens`` [B, n] (or [n]): the token each node proposes; ``target_tokens`` [B, n]:
    the target model's greedy token after node u (the argmax of its logits row u).  Node 0 is the single root (the last
    committed token's successor, already verified) and is always accepted.  Node u > 0 is accepted iff its parent is,
    ``draft_tokens[u] == target_tokens[parent[u]]``, and no lower-indexed sibling is (siblings carrying the same token:
    the lowest index wins).  The accepted nodes form one chain from the root.

    Returns ``(path [B, n], count [B])``, int64: ``path[b, :count[b]]`` lists the chain root first; the entries past
    count are unspecified but in [0, n).  The bonus token is ``target_tokens.gather(-1, path[:, count - 1])``."""
    squeeze = draft_tokens.dim() == 1
    if squeeze:
        draft_tokens, target_tokens = draft_tokens.unsqueeze(0), target_tokens.unsqueeze(0)
    B, n = draft_tokens.shape
    p = _parent(parent)
    if p.dim() == 1:
        p = p.unsqueeze(0).expand(B, n)
    pc = p.clamp(min=0)
    match = (p >= 0) & (draft_tokens == target_tokens.gather(-1, pc))
    # first[u]: u matches and no lower-indexed sibling (same parent) matches
    u = torch.arange(n, device=p.device)
    sib = (p.unsqueeze(-1) == p.unsqueeze(-2)) & (u.unsqueeze(-1) > u)       # [B, u, v]: v < u shares u's parent
    first = match & ~(sib & match.unsqueeze(-2)).any(-1)
    ok = first | (u == 0)
    anc = tree_ancestor_mask(p)                                               # [B, n, n]
    accepted = (anc & ~ok.unsqueeze(-2)).any(-1).logical_not() & anc[..., 0]   # every node of the path ok, rooted at 0
    depth = tree_depth(p)
    slot = torch.where(accepted, depth, torch.full_like(depth, n))            # accepted node u goes to path[depth[u]]
    path = torch.zeros(B, n + 1, dtype=torch.long, device=p.device)
    path.scatter_(-1, slot, u.expand(B, n).contiguous())
    path = path[:, :n].contiguous()
    count = accepted.sum(-1)
    if squeeze:
        path, count = path[0], count[0]
    return path, count


MAX_TREE = 64        # a sequence of a pack with more tokens is a chain (a prompt chunk): the kernels' rule


def _packed_rows(cu_q: torch.Tensor, T: int):
    """Per packed row: (sequence, local index, covered) and per sequence its length, with the kernels' reading of
    ``cu_q`` (offsets clamped into [0, T], an end before its start reads as the start)."""
    cu = cu_q.long().clamp(0, int(T))
    n_seq = cu.numel() - 1
    c0 = cu[:n_seq]
    c1 = torch.maximum(cu[1:], c0)
    rows = torch.arange(int(T), device=cu.device)
    # the last sequence that starts at or before the row (empty sequences share a start with their successor)
    seq = (torch.bucketize(rows, c0.contiguous(), right=True) - 1).clamp(0, n_seq - 1)
    local = rows - c0[seq]
    covered = (local >= 0) & (rows < c1[seq])
    return seq, local, covered, c1 - c0


def _scatter_rows(x: torch.Tensor, seq, local, tree_row, n_seq: int, fill: int) -> torch.Tensor:
    """[T] -> [n_seq, MAX_TREE]: row (seq, local) <- x for the rows of tree sequences, ``fill`` elsewhere.  The other
    rows go to a spare row that is cut off, so that no index depends on the data."""
    out = torch.full((n_seq + 1, MAX_TREE), fill, dtype=torch.long, device=x.device)
    out[torch.where(tree_row, seq, torch.full_like(seq, n_seq)), torch.where(tree_row, local, torch.zeros_like(local))] = \
        torch.where(tree_row, x.long(), torch.full_like(seq, fill))
    return out[:n_seq]


def packed_local(cu_q: torch.Tensor, T: int) -> torch.Tensor:
    """[T] int64: the index of every packed row within its sequence (0 for rows that no sequence covers)."""
    _seq, local, covered, _n = _packed_rows(cu_q, T)
    return torch.where(covered, local, torch.zeros_like(local))


def packed_tree_depth(parent: torch.Tensor, cu_q: torch.Tensor, T: int) -> torch.Tensor:
    """[T] int64 for the ``parent`` [T] of a packed step: the tree depth of a row of a sequence of at most 64 tokens, the
    local index for a longer sequence (a chain to the kernels, whatever ``parent`` holds) and 0 for rows that no
    sequence covers.  The RoPE position of a packed row is ``packed_positions(...) - packed_local(cu_q, T) + this``; an
    admitting sequence (``admit=True`` on a fresh slot) is a chain to the kernels too, so give it a chain ``parent``."""
    seq, local, covered, n = _packed_rows(cu_q, T)
    tree_row = covered & (n[seq] <= MAX_TREE)
    depth = tree_depth(_scatter_rows(parent, seq, local, tree_row, n.numel(), -1))
    d = depth[seq, local.clamp(0, MAX_TREE - 1)]
    return torch.where(tree_row, d, torch.where(covered, local, torch.zeros_like(local)))


def greedy_accept_packed(parent: torch.Tensor, draft_tokens: torch.Tensor, target_tokens: torch.Tensor,
                         cu_q: torch.Tensor, n_seq: int):
    """``greedy_accept`` for every sequence of a pack: ``parent``, ``draft_tokens`` and ``target_tokens`` are [T], packed
    like q.  Returns ``(path [T], count [n_seq])``, int64, as ``commit_packed_dyn`` takes them: ``path[cu_q[i] + j]`` is
    the local index of the j-th accepted node of sequence i (root first; entries past ``count[i]`` are unspecified but
    in [0, n_i)).  A sequence of more than 64 tokens is a chain: ``count = n_i`` and the identity path; an empty one
    has ``count = 0``.  A sequence that the step itself has stored (``commit_seq[i] = 1``) must not be stored again:
    pass ``count * (1 - commit_seq)`` to ``commit_packed_dyn``."""
    T = parent.shape[0]
    if cu_q.numel() != n_seq + 1:
        raise ValueError(f"cu_q must hold n_seq + 1 = {n_seq + 1} offsets, got {cu_q.numel()}")
    seq, local, covered, n = _packed_rows(cu_q, T)
    tree_row = covered & (n[seq] <= MAX_TREE)
    rows = [_scatter_rows(x, seq, local, tree_row, n_seq, f) for x, f in ((parent, -1), (draft_tokens, 0),
                                                                            (target_tokens, 0))]
    path, count = greedy_accept(*rows)                                       # [n_seq, 64], [n_seq]
    p = path[seq, local.clamp(0, MAX_TREE - 1)]
    path_packed = torch.where(tree_row, p, torch.where(covered, local, torch.zeros_like(local)))
    count = torch.where(n <= MAX_TREE, torch.minimum(count, n), n)
    return path_packed, count
