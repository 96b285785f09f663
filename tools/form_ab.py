#!/usr/bin/env python3
"""Same-process alternation of the drop-in two-server crawl in form "table" (FE shares) and "table32"
(Z_2^32 shares, fhh_gb_cfg.form = 2):
    python tools/form_ab.py [--workload zipf|coords] [--clients 100000] [--threshold 0.001] [--rounds 3]
zipf: the metric's Zipf workload (100000 clients = configs[1], 1000000 = the metric's); coords: configs[3]
(d = 2 lat/lon, data_len 16). Each round runs one full crawl per form on the same keys (fresh material: CO15
base OTs per level, SoftSpoken k = 2, both parties on one GPU, in-place channel), form "table" first. Prints
one JSON line: per form the rounds' wall seconds and phase seconds, the bytes each direction carried, and
whether both forms found the same (path, value) set."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="zipf", choices=["zipf", "coords"])
    ap.add_argument("--clients", type=int, default=100_000)
    ap.add_argument("--threshold", type=float, default=0.001)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ot-ss-k", type=int, default=2)
    args = ap.parse_args()
    import torch
    import fuzzyheavyhitters_amd as fhh
    from fuzzyheavyhitters_amd import workload
    n = args.clients
    if args.workload == "coords":
        L, d = 16, 2
        wl = workload.coords_workload(n, ball_size=1, zipf_s=1.03, seed=0x5EED)
    else:
        L, d = 512, 1
        wl = workload.zipf_workload(n, L, d, num_sites=10_000, zipf_s=1.03, ball_size=1, seed=0x5EED)
    c0, c1 = fhh.KeyCollection(L, d), fhh.KeyCollection(L, d)
    fhh.gen_keys_pair(c0, c1, wl.left, wl.right, wl.root_seeds)
    torch.cuda.synchronize()
    out = {"workload": args.workload, "clients": n, "data_len": L, "d": d, "threshold": args.threshold,
           "ot_ss_k": args.ot_ss_k, "forms": {}}
    finals = {}
    for rnd in range(args.rounds):
        for form in ("table", "table32"):
            tm = {}
            t0 = time.perf_counter()
            r = fhh.two_party_crawl(c0, c1, args.threshold, channel="inplace", timing=tm, record=False,
                                    material="fresh", form=form, ot_ss_k=args.ot_ss_k)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            f = out["forms"].setdefault(form, {"wall_s": [], "phases_s": []})
            f["wall_s"].append(round(wall, 4))
            f["phases_s"].append({k: round(v, 4) for k, v in tm.items()})
            f["bytes"] = {k: sum(lb.get(k, 0) for lb in r.level_bytes) for k in ("u1", "gc", "u2", "y2")}
            f["children"] = int(sum(int(c) for c in r.level_children))
            f["heavy_hitters"] = len(r.final)
            finals[form] = sorted((str(x.path), int(x.value)) for x in r.final)
            print(f"round {rnd} {form}: {wall:.3f} s", file=sys.stderr, flush=True)
    out["same_result"] = finals["table"] == finals["table32"]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
