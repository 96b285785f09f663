"""Inputs and the expected bytes of the fused leader tests (fhh_leader_requests_ball): populations of ball_cases'
constructed and uniform points, and the reference object — workload.add_keys_request_bincode (the numpy
serializer) on oracle.gen_keys of the oracle's bounds, cut into requests on Python integers. Nothing here calls the
code under test."""
import numpy as np

import ball_cases as bc

NS = (1, 63, 64, 65, 130)
BATCHES = (0, 1, 7, 64, 100)
SENTINEL = 0xA5
GUARD = 64


def population(rng, L, d, n, delta):
    """n d points: the accepted constructed ones first (a = 0, whose left bound wraps, among them), uniform ones
    after."""
    acc, _ = bc.split_cases(L, delta)
    vals = [a for _, a in acc][:n * d]
    vals += bc.random_points(rng, n * d - len(vals), L, delta)
    return bc.alpha_array(vals, d, L)


def fields(ks, a, b):
    return tuple(x[a:b] for x in (ks.key_idx, ks.root_seed, ks.cw_seed, ks.cw_bits))


def request_list(ks, n, batch, first=0):
    """The requests of clients [first, first + n) of the key set ks, `batch` clients each (0: one request)."""
    from fuzzyheavyhitters_amd import workload
    B = batch or n
    return [workload.add_keys_request_bincode(*fields(ks, first + a, first + min(a + B, n))) for a in range(0, n, B)]


_RECORDS = {}


def expected(ks, n, batch, first=0):
    """Those requests back to back: one server's bytes of a call on clients [first, first + n). The clients'
    records are serialized once per key set (the serializer's single request of all of them, cut at the record
    size) and framed here: a request is its u64 client count, then its clients' records."""
    from fuzzyheavyhitters_amd import workload
    if id(ks) not in _RECORDS:
        total = ks.key_idx.shape[0]
        one = workload.add_keys_request_bincode(ks.key_idx, ks.root_seed, ks.cw_seed, ks.cw_bits)
        _RECORDS[id(ks)] = (ks, one[8:].reshape(total, -1))   # ks kept: its id stays its own
    recs = _RECORDS[id(ks)][1]
    B = batch or n
    parts = []
    for a in range(0, n, B):
        b = min(a + B, n)
        parts += [np.frombuffer(np.uint64(b - a).tobytes(), np.uint8), recs[first + a:first + b].reshape(-1)]
    return np.concatenate(parts)


def request_bytes(d, L, n, batch):
    B = batch or n
    return 8 * ((n + B - 1) // B) + n * (8 + 2 * d * (25 + 20 * L))


def client_off(i, d, L, batch, n):
    """Byte offset of client i's record in the requests of n clients (Python integers)."""
    B = batch or n
    return 8 * (i // B + 1) + i * (8 + 2 * d * (25 + 20 * L))


def plan_model(d, n):
    """(items, waves, trips) of the fused kernel's launch: an item is one wave's 64 clients of one key, dealt
    grid-stride to at most 4096 workgroups of 8 waves — k_keygen's cap (ball_cases.keygen_trips)."""
    items = 2 * d * ((n + 63) // 64)
    waves = min((items + 7) // 8, 4096) * 8
    return items, waves, (items + waves - 1) // waves


assert plan_model(4, 262_145) == (32_776, 32_768, 2) and plan_model(4, 262_144)[2] == 1
assert all(plan_model(d, n)[2] == bc.keygen_trips(n, d) for d in (1, 2, 3, 4) for n in (1, 64, 65, 130, 262_145, 10 ** 6))


def differing(got, want):
    bad = np.nonzero(got != want)[0]
    return f"{bad.size} bytes differ, the first at {bad[:8]}"
