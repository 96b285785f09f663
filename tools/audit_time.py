#!/usr/bin/env python3
"""Time of the key audit (`audit_keys_ball`: k_audit_keys, both servers' keys of every client walked at the five
probes of its point) beside the keygen whose keys it checks (`gen_keys_ball`), in one process on one GPU.

Two populations of uniform points, d = 1, data_len 512, ball 1: 100 000 and 1 000 000 clients. Per population,
after one warm-up round, --rounds (5) rounds that alternate

  (a) `gen_keys_ball` into the reset pair          keygen_ms: k_keygen alone, HIP events (stats.keygen_ms)
  (b) `audit_keys_ball` of that pair               audit_ms: k_audit_keys (+ its count kernel), HIP events
                                                   (fhh_audit_timing); audit_wall_s: the host clock around the call,
                                                   the points' copy and the ok bytes' copy inside it
  (c) `tree_init_at` of server 0's keys at 10 random prefixes of depth 511: k_eval_paths on 2 x 10 x 511 blocks per
      client against the audit's 2 x 2 x 5 x 512, a comparable count. init_at_s: the host clock around the
      synchronous call (its only time: the kernel is the call but for one small upload)

Every audit must find every client ok and make the plan's comparisons, or the run exits non-zero. Medians, spreads and
raw rounds go to --out as JSON with the executed AES blocks per second of (b) and (c) and their ratio."""
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
    ap.add_argument("--prefixes", type=int, default=10)
    ap.add_argument("--seed", type=lambda s: int(s, 0), default=0x5EED)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("audit_time: needs a GPU (a CPU run measures nothing)")
    import fuzzyheavyhitters_amd as fhh
    L, d, ball, depth = a.L, 1, 1, a.L - 1
    rng = np.random.default_rng(a.seed)
    paths = rng.integers(0, 2, (a.prefixes, d, depth), dtype=np.uint8)
    assert len({p.tobytes() for p in paths}) == a.prefixes

    res = {"L": L, "d": d, "ball": ball, "rounds": a.rounds, "warmup_rounds": 1, "device": torch.cuda.get_device_name(0),
           "init_at_prefixes": a.prefixes, "init_at_depth": depth,
           "timed": "keygen_ms, audit_ms: HIP events around the kernels; *_s: host clock around synchronous calls",
           "populations": []}
    for n in a.n:
        print(f"audit_time: n = {n}", file=sys.stderr, flush=True)
        points = rng.integers(0, 256, (n, d, (L + 7) // 8), dtype=np.uint8)
        points[:, :, 0] &= 0x7F                       # no carry out of bit L
        c0, c1 = fhh.KeyCollection(L, d), fhh.KeyCollection(L, d)
        plan = fhh.audit_plan(d, L, n, 2 ** 20)
        init_blocks = depth * 2 * a.prefixes * n
        t = {k: [] for k in ("keygen_ms", "audit_ms", "audit_wall_s", "init_at_s")}
        for r in range(a.rounds + 1):                  # round 0 warms up
            for c in (c0, c1):
                c.reset()
                c.reset_stats()
            fhh.gen_keys_ball(c0, c1, points, ball, seed=SEED)
            t0 = time.perf_counter()
            ok, rep = c0.audit_keys_ball(c1, points, ball)
            t1 = time.perf_counter()
            if not ok.all() or rep["n_bad_clients"] or rep["n_checks"] != plan["n_checks"] or rep["seed_diverged"]:
                sys.exit(f"audit_time: n = {n}: the audit of gen_keys_ball's keys is not clean: {rep}")
            t2 = time.perf_counter()
            c0.tree_init_at(paths)
            t3 = time.perf_counter()
            if r:
                t["keygen_ms"].append(c0.stats()["keygen_ms"])
                t["audit_ms"].append(rep["kernel_ms"])
                t["audit_wall_s"].append(t1 - t0)
                t["init_at_s"].append(t3 - t2)
        out = {k: summary(v) for k, v in t.items()}
        audit_rate = plan["aes_blocks"] / (out["audit_ms"]["median"] * 1e-3)
        init_rate = init_blocks / out["init_at_s"]["median"]
        out.update({
            "n": n, "all_ok": True, "n_checks": plan["n_checks"], "items": plan["items"],
            "audit_aes_blocks": plan["aes_blocks"], "keygen_aes_blocks": 4 * L * 2 * d * n, "init_at_aes_blocks": init_blocks,
            "audit_blocks_per_s": audit_rate,
            "keygen_blocks_per_s": 4 * L * 2 * d * n / (out["keygen_ms"]["median"] * 1e-3),
            "eval_paths_blocks_per_s": init_rate,
            "audit_over_eval_paths_rate": audit_rate / init_rate,
            "audit_over_keygen_ms": out["audit_ms"]["median"] / out["keygen_ms"]["median"],
            "audit_us_per_key_and_probe": out["audit_ms"]["median"] * 1e3 / (n * 2 * d * 5),
        })
        res["populations"].append(out)
        del c0, c1, points
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
