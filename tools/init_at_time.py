#!/usr/bin/env python3
"""Time of `tree_init_at` (k_eval_paths: every client's keys walked to a given frontier in one kernel) against the
route it replaces, `tree_init` + depth x (`tree_crawl` + `tree_prune` with the known keep masks), in one process
on one GPU.

configs[1] by default: 100k Zipf clients, data_len 512, d = 1, threshold 0.001; the frontier is the plaintext
crawl's survivors at --depth (256). Both routes run on the same collection (server 0's) and must leave the same
exported states: checked once, before the timed rounds. A warm-up round, then --rounds rounds that alternate the
two routes; every call is synchronous (it returns after the stream is drained), so the host clock around a route
is its time. Medians, raw rounds, the ratio, tree_init_at's executed AES blocks per second and k_expand's
in-kernel rate (fhh_stats' event-timed launches of the level-by-level rounds, same process) go to --out as JSON."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--L", type=int, default=512)
    ap.add_argument("--d", type=int, default=1)
    ap.add_argument("--depth", type=int, default=256)
    ap.add_argument("--threshold", type=float, default=0.001)
    ap.add_argument("--num-sites", type=int, default=10_000)
    ap.add_argument("--seed", type=lambda s: int(s, 0), default=0x5EED)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not 0 < a.depth < a.L:
        sys.exit("init_at_time: --depth must be in [1, L)")

    import torch
    if not torch.cuda.is_available():
        sys.exit("init_at_time: needs a GPU (a CPU run measures nothing)")
    import fuzzyheavyhitters_amd as fhh
    from fuzzyheavyhitters_amd import workload

    wl = workload.zipf_workload(a.n, a.L, a.d, num_sites=a.num_sites, zipf_s=1.03, ball_size=1, seed=a.seed)
    thr = max(1, int(a.threshold * a.n))
    counts, mid, _ = workload.plaintext_crawl(wl.left, wl.right, thr, thr, levels=a.depth)
    keeps = [c >= thr for c in counts]
    paths = np.array([[list(p) for p in node] for node in mid], np.uint8).reshape(len(mid), a.d, a.depth)
    if not len(mid):
        sys.exit("init_at_time: nothing survives to --depth at this threshold")
    n_unique, _ = fhh.KeyCollection.frontier_plan(paths)
    print(f"init_at_time: frontier of {len(mid)} nodes at depth {a.depth}, distinct prefixes per dim {list(n_unique)}",
          file=sys.stderr, flush=True)
    c0, c1 = fhh.KeyCollection(a.L, a.d), fhh.KeyCollection(a.L, a.d)
    fhh.gen_keys_pair(c0, c1, wl.left, wl.right, wl.root_seeds)

    def init_at():
        c0.tree_init_at(paths)

    def level_by_level():
        c0.tree_init()
        for keep in keeps:
            C, _ = c0.tree_crawl()
            assert C == keep.size
            c0.tree_prune(keep)

    init_at()                                          # correctness first: the two routes' states, once
    got = c0.export_states()
    level_by_level()
    if not np.array_equal(c0.frontier_paths(), paths):
        sys.exit("init_at_time: the level-by-level frontier is not the plaintext frontier")
    for x, y, name in zip(got, c0.export_states(), ("seed", "t", "y")):
        if not np.array_equal(x, y):
            sys.exit(f"init_at_time: the two routes' {name} states differ")
    del got
    configs = [("tree_init_at", init_at), ("level_by_level", level_by_level)]
    rounds = {name: [] for name, _ in configs}
    expand = {}
    for r in range(a.rounds + 1):                      # round 0 warms both routes up
        if r == 1:
            c0.reset_stats()
        for name, fn in configs:
            before = c0.stats()
            t0 = time.perf_counter()
            fn()
            s = time.perf_counter() - t0
            if r:
                rounds[name].append(s)
                after = c0.stats()
                for k in ("aes_blocks", "expand_ms", "expand_blocks_timed", "expand_launches"):
                    expand[(name, k)] = expand.get((name, k), 0) + after[k] - before[k]
    med = {name: statistics.median(v) for name, v in rounds.items()}
    blocks_a = a.depth * 2 * int(n_unique.sum()) * a.n
    assert expand[("tree_init_at", "aes_blocks")] == blocks_a * a.rounds
    spread_b = max(rounds["level_by_level"]) - min(rounds["level_by_level"])
    res = {
        "n": a.n, "L": a.L, "d": a.d, "depth": a.depth, "threshold": a.threshold, "frontier_nodes": len(mid),
        "distinct_prefixes": [int(x) for x in n_unique], "rounds": a.rounds, "warmup_rounds": 1,
        "timed": "host clock around the route's synchronous calls on server 0's collection",
        "states_equal": True,
        "median_s": med, "min_s": {k: min(v) for k, v in rounds.items()}, "max_s": {k: max(v) for k, v in rounds.items()},
        "raw_rounds_s": rounds,
        "level_by_level_spread_s": spread_b,
        "level_by_level_over_init_at": med["level_by_level"] / med["tree_init_at"],
        "faster_by_more_than_spread": med["level_by_level"] - med["tree_init_at"] > spread_b,
        "init_at_aes_blocks": blocks_a,
        "init_at_blocks_per_s": blocks_a / med["tree_init_at"],
        "level_by_level_aes_blocks": expand[("level_by_level", "aes_blocks")] // a.rounds,
        "level_by_level_blocks_per_s": expand[("level_by_level", "aes_blocks")] / a.rounds / med["level_by_level"],
        "k_expand_in_kernel_blocks_per_s": (expand[("level_by_level", "expand_blocks_timed")] /
                                            (expand[("level_by_level", "expand_ms")] * 1e-3)
                                            if expand[("level_by_level", "expand_ms")] else None),
        "k_expand_launches_per_round": expand[("level_by_level", "expand_launches")] // a.rounds,
    }
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
