"""Inputs shared by the fhh_retain_plan (CPU) and fhh_retain_clients (GPU) tests: the keep masks, and a brute-force
recount of the clients inside given nodes."""
import numpy as np


def masks(n):
    """name -> uint8 mask over n clients: all ones; one dropped at the first, middle and last position; a whole
    64-client word dropped (n > 64); one survivor; a seeded random mask. Every mask keeps somebody."""
    out = {"all ones": np.ones(n, np.uint8)}
    for name, i in (("first dropped", 0), ("middle dropped", n // 2), ("last dropped", n - 1)):
        m = np.ones(n, np.uint8)
        m[i] = 0
        if m.any():
            out[name] = m
    if n > 64:
        w = (n - 1) // 64 - 1                    # the last full word before the tail
        m = np.ones(n, np.uint8)
        m[64 * w:64 * (w + 1)] = 0
        out["word dropped"] = m
        m = np.ones(n, np.uint8)
        m[:64] = 0
        out["first word dropped"] = m
    for i in sorted({0, n // 2, n - 1}):
        m = np.zeros(n, np.uint8)
        m[i] = 1
        out[f"one survivor {i}"] = m
    m = (np.random.default_rng(1000 + n).random(n) < 0.5).astype(np.uint8)
    m[np.random.default_rng(n).integers(n)] = 1
    out["random"] = m
    return out


def recount(left, right, paths):
    """Clients inside each node, by brute force: left / right [n][d][L] bits, paths [C][d][k] direction bits; client
    c is inside iff in every dim left[c][:k] <= path <= right[c][:k] as MSB-first integers."""
    paths = np.asarray(paths, np.uint8)
    C, d, k = paths.shape
    w = (1 << np.arange(k - 1, -1, -1)).astype(np.int64)
    lo = (left[:, :, :k].astype(np.int64) * w).sum(-1)       # [n][d]
    hi = (right[:, :, :k].astype(np.int64) * w).sum(-1)
    p = (paths.astype(np.int64) * w).sum(-1)                 # [C][d]
    inside = ((lo[None] <= p[:, None]) & (p[:, None] <= hi[None])).all(-1)
    return inside.sum(1).astype(np.uint64)


def children_of(parents, d):
    """The paths [F << d][d][k + 1] of the children of frontier paths [F][d][k], in the engine's child order
    (child c = parent c >> d, direction of dim j = bit j of c & (2^d - 1))."""
    parents = np.asarray(parents, np.uint8)
    F, _, k = parents.shape
    out = np.zeros((F << d, d, k + 1), np.uint8)
    for c in range(F << d):
        out[c, :, :k] = parents[c >> d]
        for j in range(d):
            out[c, j, k] = (c >> j) & 1
    return out
