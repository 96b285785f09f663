"""The leader's `add_fuzzy_keys` (src/bin/leader.rs:130-163) on the GPU: a population's points turned into the two
servers' `add_keys` request batches, chunk by chunk, in the memory of one chunk's keys.

The reference makes every client's keys with `ibDCFKey::gen_l_inf_ball(point, ball_size)` and sends them in
requests of `addkey_batch_size` clients (leader.rs:391-415). Here a chunk of clients is keyed by one
`gen_keys_ball` call (the bounds and the root seeds made in the kernel) and serialized on the GPU by
`export_keys_bincode` (route "collections"), or keyed and serialized by the one kernel of `leader_requests_ball`
with no collection at all (route "fused"); the root seeds come from one seed stream indexed by the client's
position in the population, so the requests do not depend on the chunking or the route.
"""
from __future__ import annotations

import numpy as np

from ._lib import FhhError
from .collection import KeyAuditError, KeyCollection, gen_keys_ball, leader_requests_ball
from .workload import split_add_keys_requests

ROUTES = ("collections", "fused")


def add_fuzzy_keys(points: np.ndarray, ball: int, *, n_dims: int, data_len: int, form: str = "bits", seed: bytes,
                   batch: int = 100, chunk: int = 10_000, device: int = 0, route: str = "collections",
                   audit: bool = False):
    """Generator over the population's chunks: yields (requests0, requests1), the `add_keys` request payloads
    (one uint8 array each, `batch` clients per request; 0 = one request per chunk) for server 0 and server 1 of
    the chunk's clients, in client order. `points` are in `gen_keys_ball`'s layout for `form`; `seed` is the 32-byte
    key of the root-seed stream, to be used for one population only. `chunk` must be a multiple of `batch`, so
    that a request holds the same clients, byte for byte, whatever the chunk size. route "collections": one
    scratch pair of collections is kept for the whole run (`reset` keeps its allocations), so the device memory
    is one chunk's keys of both servers and its serialized bytes. route "fused": one scratch ctx and no keys, as
    the reference's leader holds none; the device memory is one chunk's serialized bytes.
    audit=True (route "collections" only; route "fused" stores no keys to audit and raises ValueError): every
    chunk's keys are checked against its points by `KeyCollection.audit_keys_ball` right after they are made, and a
    chunk that fails raises KeyAuditError, carrying the report, before any of its requests is yielded. The bytes
    yielded are the same with and without the audit."""
    if route not in ROUTES:
        raise FhhError(f"add_fuzzy_keys: unknown route {route!r} {ROUTES}")
    if not isinstance(audit, (bool, np.bool_)):
        raise TypeError(f"add_fuzzy_keys: audit must be a bool, not {type(audit).__name__}")
    if audit and route == "fused":
        raise ValueError("add_fuzzy_keys: audit=True needs route 'collections': the fused route stores no keys to audit")
    if chunk <= 0 or batch < 0:
        raise FhhError("add_fuzzy_keys: chunk must be positive and batch non-negative")
    if batch and chunk % batch:
        raise FhhError(f"add_fuzzy_keys: chunk {chunk} is not a multiple of batch {batch}: chunking would move "
                       "the request boundaries")
    n = len(points)
    cs = [KeyCollection(data_len, n_dims, device=device) for _ in range(1 if route == "fused" else 2)]
    try:
        for first in range(0, n, chunk):
            count = min(chunk, n - first)
            part = points[first:first + count]
            if route == "fused":
                both = leader_requests_ball(cs[0], part, ball, form=form, seed=seed, seed_first=first, batch=batch)
            else:
                for c in cs:
                    c.reset()
                gen_keys_ball(cs[0], cs[1], part, ball, form=form, seed=seed, seed_first=first)
                if audit:
                    ok, report = cs[0].audit_keys_ball(cs[1], part, ball, form=form)
                    if report["n_bad_clients"]:
                        raise KeyAuditError(report, ok, first)
                both = [c.export_keys_bincode(0, count, batch) for c in cs]
            yield tuple(split_add_keys_requests(b, n_dims, data_len) for b in both)
    finally:
        for c in cs:
            c.close()


__all__ = ["add_fuzzy_keys", "KeyAuditError"]
