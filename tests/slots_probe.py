"""Stale-content probe for slot reuse (the mask-edge idea of tests/probe_inputs.py applied to a pool slot that held another
sequence before).  Plain torch on the CPU; imports neither the product nor a GPU.

A slot's sink rows and whole ring are filled with STALE keys that are 2 x the +-1 codes of the queries to come, then the
slot is released and a short prompt is prefilled into it.  The kernels must read only `sink_len` sink rows and
`window_len` ring slots of the new state; every other row still holds a stale key.  Query (head h, token t) is
q = a * c[h, t] (a = probe_inputs.amplitude(D) = 2): its scaled logit on its own stale key is 2 a sqrt(D) (32 at
D = 64) against about a * N(0, 1) on every real key (random codes), so ONE leaked stale key takes the whole row and the
output becomes that key's value row: an O(1) error.  tests/test_slots_host.py proves the factor on the CPU (fp64 oracle
against an oracle that sees one stale key); tests/test_gpu_slots.py runs the kernels on these inputs.

Stale row j (sink rows first, then ring slots) of KV head hk aims at query head hk * G + j % G, token (j // G) % (n + 1):
tokens 0 .. n - 1 are the verify chunk, token n is the single-token step that follows.  With num_sink + W >= G (n + 1)
every query has a stale key and every stale row has a query."""
import torch

from probe_inputs import amplitude, codes, _rand


def stale_probe(Hq, Hkv, D, ns, W, n, L, dtype, seed):
    """Inputs of one reuse: dict with
    q [1, Hq, n + 1, D] (chunk queries, then the step's), kc / vc [1, Hkv, n + 1, D] (their K/V: random codes / randn),
    kp / vp [1, Hkv, L, D] the new prompt, stale_k / stale_v [1, Hkv, ns + W, D] what the slot held before (sink rows
    first), s_aux [Hq]."""
    G = Hq // Hkv
    assert ns + W >= G * (n + 1), "every query needs a stale key"
    g = torch.Generator().manual_seed(seed)
    a = amplitude(D)
    c = codes((1, Hq, n + 1, D), g, torch.float32)
    q = (a * c).to(dtype)
    j = torch.arange(ns + W)
    stale_k = torch.empty(1, Hkv, ns + W, D)
    for hk in range(Hkv):
        stale_k[0, hk] = 2 * c[0, hk * G + j % G, (j // G) % (n + 1)]
    return dict(q=q, kc=codes((1, Hkv, n + 1, D), g, dtype), vc=_rand((1, Hkv, n + 1, D), g, dtype),
                kp=codes((1, Hkv, L, D), g, dtype), vp=_rand((1, Hkv, L, D), g, dtype),
                stale_k=stale_k.to(dtype), stale_v=_rand((1, Hkv, ns + W, D), g, dtype),
                s_aux=_rand((Hq,), g, torch.float32, 0.5))


def stale_rows(ns, W, L):
    """Indices into stale_k / stale_v of the rows that are still stale after a prefill of L <= ns + W tokens: sink rows
    [sink_len, ns) and ring slots [window_len, W)."""
    sl = min(L, ns)
    wl = min(L - sl, W)
    return list(range(sl, ns)) + list(range(ns + wl, ns + W))


def true_keys(pr, t):
    """K/V that query token t (t < n: the verify chunk, t = n: the step after all n were committed) really sees: the
    prompt and tokens 0 .. t (nothing is evicted: L + n + 1 <= W + sink_len is the caller's choice)."""
    return (torch.cat([pr["kp"], pr["kc"][:, :, :t + 1]], dim=2), torch.cat([pr["vp"], pr["vc"][:, :, :t + 1]], dim=2))
