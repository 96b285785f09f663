#!/usr/bin/env python3
"""Per-server busy time of the drop-in two-server crawl with one garbler (roles "fixed") and with every level's
windows split between the servers (roles "split"), alternated in one process:
    python tools/party_roles_time.py [--clients 100000] [--threshold 0.001] [--rounds 3] [--out FILE]
Workload: the Zipf workload (100000 clients = configs[1]: data_len 512, d = 1), material "test", in-place channel
(both parties on one GPU), form "table32", SoftSpoken k = 2. One warm-up crawl of each mode, then `rounds`
rounds of one crawl per mode, "fixed" first.

Busy seconds of a server: the wall time of its own fhh_gb_* / fhh_ev_* calls. Every such call returns after a
device synchronisation, so a call's GPU work is charged to the server that issued it. On one GPU the two
servers' calls run one after the other, so the crawl's wall time does not show the balance; max(busy) is what a
deployment on two machines would wait for per crawl (a projection: nothing here runs on two machines).
Prints one JSON line (and writes it to --out): per mode the rounds' busy seconds per server, their maximum and
total, the crawl's wall seconds, the bytes per direction, the medians, and whether both modes found the same
(path, value) set."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clients", type=int, default=100_000)
    ap.add_argument("--threshold", type=float, default=0.001)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import fuzzyheavyhitters_amd as fhh
    from fuzzyheavyhitters_amd import workload
    n, L, d = args.clients, 512, 1
    wl = workload.zipf_workload(n, L, d, num_sites=10_000, zipf_s=1.03, ball_size=1, seed=0x5EED)
    c0, c1 = fhh.KeyCollection(L, d), fhh.KeyCollection(L, d)
    fhh.gen_keys_pair(c0, c1, wl.left, wl.right, wl.root_seeds)
    torch.cuda.synchronize()
    out = {"workload": "zipf", "clients": n, "data_len": L, "d": d, "threshold": args.threshold, "material": "test",
           "channel": "inplace", "form": "table32", "ot_ss_k": 2, "rounds": args.rounds, "modes": {}}
    finals = {}
    for rnd in range(-1, args.rounds):   # round -1: the warm-up crawls
        for roles in ("fixed", "split"):
            busy, tm = [0.0, 0.0], {}
            t0 = time.perf_counter()
            r = fhh.two_party_crawl(c0, c1, args.threshold, channel="inplace", timing=tm, record=False, material="test",
                                    prf_seed=7, form="table32", ot_ss_k=2, roles=roles, server_busy=busy)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            print(f"round {rnd} {roles}: wall {wall:.3f} s, busy {busy[0]:.3f} / {busy[1]:.3f} s", file=sys.stderr,
                  flush=True)
            finals[roles] = sorted((str(x.path), int(x.value)) for x in r.final)
            if rnd < 0:
                continue
            m = out["modes"].setdefault(roles, {"busy_s": [], "max_busy_s": [], "total_busy_s": [], "wall_s": [],
                                                "phases_s": []})
            m["busy_s"].append([round(b, 4) for b in busy])
            m["max_busy_s"].append(round(max(busy), 4))
            m["total_busy_s"].append(round(sum(busy), 4))
            m["wall_s"].append(round(wall, 4))
            m["phases_s"].append({k: round(v, 4) for k, v in tm.items()})
            m["direction_bytes"] = {"to_server0": r.direction_bytes[0], "to_server1": r.direction_bytes[1]}
            m["children"] = int(sum(int(c) for c in r.level_children))
            m["heavy_hitters"] = len(r.final)
    for m in out["modes"].values():
        m["median"] = {"busy_s": [round(statistics.median(b[s] for b in m["busy_s"]), 4) for s in (0, 1)],
                       "max_busy_s": statistics.median(m["max_busy_s"]),
                       "total_busy_s": statistics.median(m["total_busy_s"]), "wall_s": statistics.median(m["wall_s"])}
    out["same_result"] = finals["fixed"] == finals["split"]
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
