#!/usr/bin/env python3
"""Time the leader's two routes from points to add_keys requests on one GPU (README row i):

  A  the collections route: gen_keys_ball, then export_keys_bincode on both servers — the wall time and the sum
     of its kernels' HIP-event times (k_keygen: stats.keygen_ms; both servers' emit kernels: fhh_export_timing)
  B  the fused host form (leader_requests_ball): the wall time
  C  the fused device form: the kernel's HIP-event time (stats.keygen_ms)

One process, the routes alternated within every round, medians of --rounds rounds after a warm-up; L = 512, d = 1,
batch 100. At --n-small clients all three; at --n-large only C and A's kernel sum, A exported in ranges of
--n-small clients (its output never exists in one piece) and C's 2 x 20.5 GB left on the device. Also
leader.add_fuzzy_keys at --n-small clients (chunk 10 000) in both routes. Writes one JSON document."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

L, D, BATCH, BALL = 512, 1, 100, 1
SEED = bytes(range(32))


def points(n, seed):
    """n uniform 512-bit points whose top bit is 0, so that a + ball never carries out."""
    pts = np.random.default_rng(seed).integers(0, 256, (n, D, L // 8), dtype=np.uint8)
    pts[:, :, 0] &= 0x7F
    return pts


def keygen_ms(c):
    return c.stats()["keygen_ms"]


def export_ms(fhh, c):
    import ctypes
    ms = ctypes.c_double()
    fhh._lib.check(fhh.lib().fhh_export_timing(c.handle, ctypes.byref(ms)), c.handle)
    return ms.value


def route_a(fhh, c0, c1, pts, rng_clients):
    """(wall ms, kernel-sum ms) of gen_keys_ball + export on both servers, exported in ranges of rng_clients."""
    n = len(pts)
    for c in (c0, c1):
        c.reset()
    t0 = time.perf_counter()
    k0 = keygen_ms(c0)
    fhh.gen_keys_ball(c0, c1, pts, BALL, seed=SEED)
    kern = keygen_ms(c0) - k0
    for c in (c0, c1):
        for first in range(0, n, rng_clients):
            c.export_keys_bincode(first, min(rng_clients, n - first), BATCH)
            kern += export_ms(fhh, c)
    return (time.perf_counter() - t0) * 1e3, kern


def route_b(fhh, c, pts):
    """wall ms; the two output arrays are allocated inside the call, as export_keys_bincode allocates its own"""
    t0 = time.perf_counter()
    fhh.leader_requests_ball(c, pts, BALL, seed=SEED, batch=BATCH)
    return (time.perf_counter() - t0) * 1e3


def route_c(fhh, c, pts):
    k0 = keygen_ms(c)
    fhh.leader_requests_ball(c, pts, BALL, seed=SEED, batch=BATCH, device_output=True)
    return keygen_ms(c) - k0


def leader_wall(fhh, pts, route):
    t0 = time.perf_counter()
    total = 0
    for r0, r1 in fhh.add_fuzzy_keys(pts, BALL, n_dims=D, data_len=L, seed=SEED, batch=BATCH, chunk=10_000, route=route):
        total += sum(r.size for r in r0) + sum(r.size for r in r1)
    return (time.perf_counter() - t0) * 1e3, total


def summary(rows):
    keys = rows[0].keys()
    out = {k: {"rounds": [round(r[k], 3) for r in rows], "median": round(statistics.median(r[k] for r in rows), 3)}
           for k in keys}
    for k in out:
        out[k]["spread"] = round(max(out[k]["rounds"]) - min(out[k]["rounds"]), 3)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n-small", type=int, default=100_000)
    ap.add_argument("--n-large", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="profiles/leader_requests/rounds.json")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU: a CPU run gives no time"
    import fuzzyheavyhitters_amd as fhh

    doc = {"L": L, "d": D, "batch": BATCH, "rounds": a.rounds, "device": torch.cuda.get_device_name(0),
           "register_group_levels": 4}
    c0, c1, cf = (fhh.KeyCollection(L, D) for _ in range(3))

    def dump():   # after every section, so that a later one's failure loses nothing
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")

    # ---- n-small: A (wall, kernels), B (wall), C (kernel), alternated
    pts = points(a.n_small, 1)
    size = 8 * ((a.n_small + BATCH - 1) // BATCH) + a.n_small * (8 + 2 * D * (25 + 20 * L))
    rows = []
    for r in range(a.rounds + 1):
        aw, ak = route_a(fhh, c0, c1, pts, a.n_small)
        b = route_b(fhh, cf, pts)
        c = route_c(fhh, cf, pts)
        print(f"n {a.n_small} round {r}: A {aw:.1f} / {ak:.2f} ms, B {b:.1f} ms, C {c:.2f} ms", file=sys.stderr, flush=True)
        if r:   # round 0 is the warm-up
            rows.append({"A_wall_ms": aw, "A_kernels_ms": ak, "B_wall_ms": b, "C_kernel_ms": c})
    doc[f"n{a.n_small}"] = summary(rows)
    dump()
    # the routes agree (the tests hold them to the oracle; here at the timed size)
    one, out = c0.export_keys_bincode(0, a.n_small, BATCH), fhh.leader_requests_ball(cf, pts, BALL, seed=SEED, batch=BATCH)
    assert one.size == size and np.array_equal(one, out[0]), "the two routes' server-0 bytes differ at the timed size"
    del one, out

    # ---- leader.add_fuzzy_keys, chunk 10 000, both routes alternated
    rows = []
    for r in range(a.rounds + 1):
        w0, t0 = leader_wall(fhh, pts, "collections")
        w1, t1 = leader_wall(fhh, pts, "fused")
        assert t0 == t1 == 2 * size
        print(f"add_fuzzy_keys round {r}: collections {w0:.1f} ms, fused {w1:.1f} ms", file=sys.stderr, flush=True)
        if r:
            rows.append({"collections_wall_ms": w0, "fused_wall_ms": w1})
    doc[f"add_fuzzy_keys_n{a.n_small}_chunk10000"] = summary(rows)
    dump()

    # ---- n-large: C's kernel and A's kernel sum only
    if a.n_large:
        pts = points(a.n_large, 2)
        rows = []
        for r in range(a.rounds + 1):
            _, ak = route_a(fhh, c0, c1, pts, a.n_small)
            c = route_c(fhh, cf, pts)
            print(f"n {a.n_large} round {r}: A kernels {ak:.2f} ms, C {c:.2f} ms", file=sys.stderr, flush=True)
            if r:
                rows.append({"A_kernels_ms": ak, "C_kernel_ms": c})
        doc[f"n{a.n_large}"] = summary(rows)
        doc[f"n{a.n_large}"]["device_output_bytes"] = 2 * (8 * ((a.n_large + BATCH - 1) // BATCH) + a.n_large * (8 + 2 * D * (25 + 20 * L)))

    dump()
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
