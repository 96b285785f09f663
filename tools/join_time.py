#!/usr/bin/env python3
"""Time of `join_clients_bincode` (fhh_join_clients_bincode: an add_keys batch joins a pair that has a frontier)
against the routes that exist without it, in one process on one GPU.

configs[1] by default: 100k Zipf clients, data_len 512, d = 1, threshold 0.001, both servers, at the plaintext
crawl's frontier of --depth (256) — the setup of tools/retain_time.py and tools/init_at_time.py. For every batch
size of --join (1 000 and 50 000 clients of the same workload) a round builds fresh twin pairs at that frontier
and runs, in alternating order,

  join_s        the wall time of both servers' join_clients_bincode (synchronous calls: the host clock around them),
                with the kernels' own time (HIP events, fhh_join_timing, both servers summed): repitch_ms (the key
                store and the live table entries copied to the new stride), decode_ms, walk_ms (k_join_paths)
  route_a_s     (a) the only route without it: export_keys of the old clients -> add_keys of old + new into a fresh
                pair -> tree_init_at(frontier_paths), both servers
  init_at_s     (b) tree_init_at of all n + m clients whose keys are already on the device (the fresh pair of (a),
                called again), both servers: the walk the join avoids, host clock around the synchronous calls
                (k_eval_paths has no event pair of its own)

and checks once per batch size (round 0, the warm-up) that the joined pair's exported states equal route (a)'s; the
run exits non-zero if they differ. Medians, spreads and raw rounds go to --out as JSON."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "rounds": v}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--L", type=int, default=512)
    ap.add_argument("--d", type=int, default=1)
    ap.add_argument("--depth", type=int, default=256)
    ap.add_argument("--threshold", type=float, default=0.001)
    ap.add_argument("--num-sites", type=int, default=10_000)
    ap.add_argument("--seed", type=lambda s: int(s, 0), default=0x5EED)
    ap.add_argument("--join", type=int, nargs="+", default=[1_000, 50_000])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not 0 < a.depth < a.L:
        sys.exit("join_time: --depth must be in [1, L)")

    import torch
    if not torch.cuda.is_available():
        sys.exit("join_time: needs a GPU (a CPU run measures nothing)")
    import fuzzyheavyhitters_amd as fhh
    from fuzzyheavyhitters_amd import workload

    m_max = max(a.join)
    wl = workload.zipf_workload(a.n + m_max, a.L, a.d, num_sites=a.num_sites, zipf_s=1.03, ball_size=1, seed=a.seed)
    old = slice(0, a.n)
    thr = max(1, int(a.threshold * a.n))
    _, mid, _ = workload.plaintext_crawl(wl.left[old], wl.right[old], thr, thr, levels=a.depth)
    if not len(mid):
        sys.exit("join_time: nothing survives to --depth at this threshold")
    paths = np.array([[list(p) for p in node] for node in mid], np.uint8).reshape(len(mid), a.d, a.depth)
    n_unique, _ = fhh.KeyCollection.frontier_plan(paths)
    print(f"join_time: frontier of {len(mid)} nodes at depth {a.depth}, distinct prefixes per dim {list(n_unique)}",
          file=sys.stderr, flush=True)

    def build_pair():
        cs = fhh.KeyCollection(a.L, a.d), fhh.KeyCollection(a.L, a.d)
        fhh.gen_keys_pair(*cs, wl.left[old], wl.right[old], wl.root_seeds[old])
        for c in cs:
            c.tree_init_at(paths)
        return cs

    res = {"n": a.n, "L": a.L, "d": a.d, "depth": a.depth, "threshold": a.threshold, "frontier_nodes": len(mid),
           "distinct_prefixes": [int(x) for x in n_unique], "rounds": a.rounds, "warmup_rounds": 1, "servers": 2,
           "timed": "join_s / route_a_s / init_at_s: host clock around both servers' synchronous calls, every round "
                    "on fresh twin pairs, the routes in alternating order; *_ms: HIP events, both servers summed",
           "device": torch.cuda.get_device_name(0), "joins": []}
    for m in a.join:
        new = slice(a.n, a.n + m)
        tmp = fhh.KeyCollection(a.L, a.d), fhh.KeyCollection(a.L, a.d)
        fhh.gen_keys_pair(*tmp, wl.left[new], wl.right[new], wl.root_seeds[new])
        reqs = [c.export_keys_bincode() for c in tmp]
        new_keys = [c.export_keys() for c in tmp]
        del tmp
        plan = fhh.KeyCollection.join_plan(a.d, a.depth, a.n, m, n_unique, 256)
        T = {k: [] for k in ("join_s", "repitch_ms", "decode_ms", "walk_ms", "route_a_s", "init_at_s")}
        moved = states_equal = None

        def run_join(cs):
            t0 = time.perf_counter()
            for c, r in zip(cs, reqs):
                c.join_clients_bincode(r)
            s = time.perf_counter() - t0
            tm = [c.join_timing() for c in cs]
            return s, [sum(t[0][i] for t in tm) for i in range(3)], sum(t[1] for t in tm)

        def run_route_a(cs):
            t0 = time.perf_counter()
            out = []
            for c, nk in zip(cs, new_keys):
                keys = c.export_keys()
                f = fhh.KeyCollection(a.L, a.d)
                f.add_keys(*[np.concatenate([x, y]) for x, y in zip(keys, nk)])
                del keys
                f.tree_init_at(c.frontier_paths())
                out.append(f)
            s = time.perf_counter() - t0
            t0 = time.perf_counter()
            for f in out:
                f.tree_init_at(paths)
            return s, time.perf_counter() - t0, out

        for r in range(a.rounds + 1):                  # round 0 warms both routes up and checks the states
            pa, pb = build_pair(), build_pair()
            if r % 2 == 0:
                js, kms, by = run_join(pa)
                ras, ias, fresh = run_route_a(pb)
            else:
                ras, ias, fresh = run_route_a(pb)
                js, kms, by = run_join(pa)
            if r == 0:
                moved = by
                for s_idx, (c, f) in enumerate(zip(pa, fresh)):
                    if c.num_clients() != f.num_clients():
                        sys.exit(f"join_time: m = {m}: client counts differ")
                    for x, y, name in zip(c.export_states(), f.export_states(), ("seed", "t", "y")):
                        if x.shape != y.shape or not np.array_equal(x, y):
                            sys.exit(f"join_time: m = {m} server {s_idx}: the joined pair's {name} states differ from "
                                     "the export -> add_keys -> tree_init_at route's")
                states_equal = True
            else:
                for k, v in zip(("join_s", "repitch_ms", "decode_ms", "walk_ms", "route_a_s", "init_at_s"),
                                (js, kms[0], kms[1], kms[2], ras, ias)):
                    T[k].append(v)
            del pa, pb, fresh
        med = {k: statistics.median(v) for k, v in T.items()}
        words_all = (a.n + m + 63) // 64
        res["joins"].append({
            "m": m, "n_after": a.n + m, "states_equal": states_equal, "plan": plan,
            **{k: _summary(v) for k, v in T.items()},
            "repitch_bytes_read_plus_written": moved,
            "repitch_GBps": moved / (med["repitch_ms"] * 1e-3) / 1e9 if med["repitch_ms"] else None,
            "route_a_over_join": med["route_a_s"] / med["join_s"],
            "walk_over_init_at": med["walk_ms"] * 1e-3 / med["init_at_s"],
            "walked_words_over_all_words": plan["words"] / words_all,
            "walk_aes_blocks": 2 * plan["aes_blocks"],
            "walk_blocks_per_s": 2 * plan["aes_blocks"] / (med["walk_ms"] * 1e-3) if med["walk_ms"] else None,
        })
        print(f"join_time: m = {m}: join {med['join_s']:.4f} s, route (a) {med['route_a_s']:.3f} s, "
              f"tree_init_at of all {med['init_at_s']:.4f} s", file=sys.stderr, flush=True)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
