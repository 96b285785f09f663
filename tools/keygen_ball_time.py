#!/usr/bin/env python3
"""Time of the leader's keygen from points (`gen_keys_ball`: the bounds and the root seeds made in k_keygen) against
the route that existed before it, in one process on one GPU.

Two populations, d = 1, data_len 512, ball 1: configs[1] (100 000 Zipf clients) and the metric's 1 000 000. Per
population, after one warm-up round, --rounds (5) rounds of

  (a) the parent route: `workload.l_inf_ball_bounds` on the unpacked points (host_bounds_s), then `gen_keys_pair`
      with host root seeds (pair_wall_s: the host clock around the synchronous call, the 2 n L bytes of bounds and
      64 n of seeds copied inside it; pair_keygen_ms: the kernel, HIP events, stats.keygen_ms)
  (b) the new route: `gen_keys_ball` from the packed points with derived root seeds (ball_wall_s, ball_keygen_ms)

and at configs[1]

  (c) the chunked leader: `leader.add_fuzzy_keys` over the population, batch 100, chunk 10 000, every request taken
      (leader_s), against `gen_keys_pair` of everything followed by `export_keys_bincode` of both servers
      (pair_export_s, the bounds given: host_bounds_s is not in it), and one more pass of the leader's loop by
      hand with the host clock around each of its steps (phases_one_pass_s).

Before anything is timed the keys of (a) and (b) are compared through `export_keys_bincode` — (a) gets the root
seeds `ball_bounds` derives from the same seed — all of them at configs[1], the first, middle and last 2 048
clients and every 4 099th block of 64 at the metric's size; the run exits non-zero if a byte differs. Medians, the
spread (max - min) and the raw rounds go to --out as JSON. The one condition on the kernel: ball_keygen_ms' median
may exceed pair_keygen_ms' by no more than pair_keygen_ms' own spread ("kernel_within_spread")."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SEED = bytes(range(32))


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "spread": max(xs) - min(xs), "rounds": xs}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--L", type=int, default=512)
    ap.add_argument("--num-sites", type=int, default=10_000)
    ap.add_argument("--seed", type=lambda s: int(s, 0), default=0x5EED)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--leader-n", type=int, default=100_000, help="the population of (c); 0 skips it")
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--chunk", type=int, default=10_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("keygen_ball_time: needs a GPU (a CPU run measures nothing)")
    import fuzzyheavyhitters_amd as fhh
    from fuzzyheavyhitters_amd import workload
    L, d, ball = a.L, 1, 1

    def same_keys(pa, pb, n, full):
        if full:
            ranges = [(f, min(4096, n - f)) for f in range(0, n, 4096)]
        else:
            ranges = [(0, 2048), (n // 2, 2048), (n - 2048, 2048)] + [(f, 64) for f in range(0, n - 64, 64 * 4099)]
        for first, count in ranges:
            for s, (x, y) in enumerate(zip(pa, pb)):
                if not np.array_equal(x.export_keys_bincode(first, count), y.export_keys_bincode(first, count)):
                    sys.exit(f"keygen_ball_time: n = {n}: server {s}'s keys of clients [{first}, {first + count}) differ "
                             "between gen_keys_pair and gen_keys_ball")
        return sum(c for _, c in ranges)

    res = {"L": L, "d": d, "ball": ball, "rounds": a.rounds, "warmup_rounds": 1, "device": torch.cuda.get_device_name(0),
           "timed": "*_s: host clock around synchronous calls; *_keygen_ms: k_keygen alone, HIP events (stats.keygen_ms)",
           "populations": []}
    for n in a.n:
        print(f"keygen_ball_time: n = {n}", file=sys.stderr, flush=True)
        wl = workload.zipf_workload(n, L, d, num_sites=a.num_sites, zipf_s=1.03, ball_size=ball, seed=a.seed)
        alpha = wl.alpha
        points = workload.pack_points(alpha)
        _, _, roots = fhh.ball_bounds(points, ball, n_dims=d, data_len=L, seed=SEED)
        pa = fhh.KeyCollection(L, d), fhh.KeyCollection(L, d)
        pb = fhh.KeyCollection(L, d), fhh.KeyCollection(L, d)
        fhh.gen_keys_pair(*pa, wl.left, wl.right, roots)
        fhh.gen_keys_ball(*pb, points, ball, seed=SEED)
        compared = same_keys(pa, pb, n, full=n <= 100_000)
        t = {k: [] for k in ("host_bounds_s", "pair_wall_s", "pair_keygen_ms", "ball_wall_s", "ball_keygen_ms")}
        for r in range(a.rounds + 1):                      # round 0 warms up
            for c in (*pa, *pb):
                c.reset()
                c.reset_stats()
            t0 = time.perf_counter()
            left, right = workload.l_inf_ball_bounds(alpha, ball)
            t1 = time.perf_counter()
            fhh.gen_keys_pair(*pa, left, right, roots)
            t2 = time.perf_counter()
            fhh.gen_keys_ball(*pb, points, ball, seed=SEED)
            t3 = time.perf_counter()
            del left, right
            if r:
                t["host_bounds_s"].append(t1 - t0)
                t["pair_wall_s"].append(t2 - t1)
                t["ball_wall_s"].append(t3 - t2)
                t["pair_keygen_ms"].append(pa[0].stats()["keygen_ms"])
                t["ball_keygen_ms"].append(pb[0].stats()["keygen_ms"])
        out = {k: summary(v) for k, v in t.items()}
        pk, bk = out["pair_keygen_ms"], out["ball_keygen_ms"]
        route_a = out["host_bounds_s"]["median"] + out["pair_wall_s"]["median"]
        out.update({
            "n": n, "clients_compared": compared, "keys_equal": True,
            "bytes_to_device_pair": 2 * n * d * L + 64 * n * d, "bytes_to_device_ball": int(points.nbytes),
            "route_a_s_median": route_a, "route_a_over_ball": route_a / out["ball_wall_s"]["median"],
            "ball_minus_pair_keygen_ms": bk["median"] - pk["median"],
            "kernel_within_spread": bk["median"] - pk["median"] <= pk["spread"],
        })
        res["populations"].append(out)
        del pa, pb

        if n == a.leader_n:
            lt = {"leader_s": [], "pair_export_s": []}
            request_bytes = 0
            for r in range(a.rounds + 1):
                t0 = time.perf_counter()
                nreq = nbytes = 0
                for r0, r1 in fhh.add_fuzzy_keys(points, ball, n_dims=d, data_len=L, seed=SEED, batch=a.batch,
                                                 chunk=a.chunk):
                    nreq += len(r0) + len(r1)
                    nbytes += sum(x.size for x in r0) + sum(x.size for x in r1)
                t1 = time.perf_counter()
                cs = fhh.KeyCollection(L, d), fhh.KeyCollection(L, d)
                fhh.gen_keys_pair(*cs, wl.left, wl.right, roots)
                whole = [c.export_keys_bincode(0, n, a.batch) for c in cs]
                t2 = time.perf_counter()
                if sum(w.size for w in whole) != nbytes:
                    sys.exit("keygen_ball_time: the chunked leader's requests and the whole export differ in size")
                request_bytes = nbytes
                del whole, cs
                if r:
                    lt["leader_s"].append(t1 - t0)
                    lt["pair_export_s"].append(t2 - t1)
            # where the chunked leader's time goes: its loop once more by hand (what leader.add_fuzzy_keys does),
            # the host clock around each step, summed over the chunks
            ph = {"create_s": 0.0, "reset_s": 0.0, "gen_keys_ball_s": 0.0, "export_s": 0.0, "split_s": 0.0}
            tc = time.perf_counter()
            cs = fhh.KeyCollection(L, d), fhh.KeyCollection(L, d)
            ph["create_s"] = time.perf_counter() - tc
            for first in range(0, n, a.chunk):
                count = min(a.chunk, n - first)
                p0 = time.perf_counter()
                for c in cs:
                    c.reset()
                p1 = time.perf_counter()
                fhh.gen_keys_ball(*cs, points[first:first + count], ball, seed=SEED, seed_first=first)
                p2 = time.perf_counter()
                bufs = [c.export_keys_bincode(0, count, a.batch) for c in cs]
                p3 = time.perf_counter()
                reqs = [workload.split_add_keys_requests(b, d, L) for b in bufs]
                p4 = time.perf_counter()
                del bufs, reqs
                for k, v in zip(("reset_s", "gen_keys_ball_s", "export_s", "split_s"), (p1 - p0, p2 - p1, p3 - p2, p4 - p3)):
                    ph[k] += v
            del cs
            lo = {k: summary(v) for k, v in lt.items()}
            lo["phases_one_pass_s"] = ph
            lo.update({"n": n, "batch": a.batch, "chunk": a.chunk, "requests": nreq, "request_bytes": request_bytes,
                       "pair_export_over_leader": lo["pair_export_s"]["median"] / lo["leader_s"]["median"]})
            res["leader"] = lo
        del wl, alpha, points, roots
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
