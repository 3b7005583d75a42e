"""Draft-tree helpers for tree-structured speculative decoding (Medusa / EAGLE / SpecInfer) over the sink + ring cache.

A chunk of n <= 64 draft nodes is a forest given by ``parent`` ([..., n] integer tensor): ``parent[u]`` in [-1, u), -1 = a
root hanging directly off the cache; any other value reads as -1, exactly as the kernels read it
(``SinkCacheLayer.extend_attention_tree*``).  Every helper is a handful of torch ops on the tensors' own device with no
host sync (no ``.item()``, no data-dependent shapes), so a whole verify / accept / commit step captures into one graph:

    depth = tree_depth(parent)                                  # RoPE position of node u: seen + depth[u]
    out = layer.extend_attention_tree_dyn(q, k, v, parent)      # every layer
    path, count = greedy_accept(parent, draft_tokens, target_tokens)
    layer.commit_path_dyn(k, v, path, count)                    # every layer
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
