#!/usr/bin/env python3
"""Same-process alternation of the d = 2 garbled table's two label layouts (fhh_set_table_row_major): the
tile-major kernels k_gt_garble_tm<4> / k_gt_eval_tm<4> against k_ot_rows_out + the row-major kernels
k_gt_garble<4, RING> / k_gt_eval<4, RING> (RING: FE or Z_2^32 shares; Z_2^32 adds the k_ring32_child_sums pass).
    python tools/gt_tm_ab.py [--clients 1000000] [--threshold 0.001] [--rounds 3] [--runs loop|party,loop] [--out FILE]
Workload: configs[3] (coords, d = 2 lat/lon, data_len 16), SoftSpoken k = 2. Runs: the drop-in two-server crawl
in forms "table" and "table32" (both parties on one GPU, in-place channel, fresh CO15 material), and the
in-process level loop (sim_crawl, gc "ot") with FE shares and with table_ring32. The party ABI keeps the
row-major labels at d = 2, so its two legs measure the same code. A discarded cold round, then `rounds` rounds; each round runs every (run, layout) once,
tile-major first. Prints one JSON line and, with --out, writes it there: per run and layout the rounds' wall
seconds and GC + OT phase seconds, their medians, and whether both layouts found the same (path, value) set."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clients", type=int, default=1_000_000)
    ap.add_argument("--threshold", type=float, default=0.001)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ot-ss-k", type=int, default=2)
    ap.add_argument("--runs", default="loop")
    ap.add_argument("--out", default="")
    ap.add_argument("--chunk-gib", type=int, default=16,
                    help="FHH_GC_CHUNK_BYTES for the level loop, in GiB: both layouts' buffers stay allocated side by "
                         "side in one process, and at the loop's default of 64 GiB each 1M clients ran out of memory")
    args = ap.parse_args()
    os.environ["FHH_GC_CHUNK_BYTES"] = str(args.chunk_gib << 30)
    import torch
    import fuzzyheavyhitters_amd as fhh
    from fuzzyheavyhitters_amd import workload
    n, L, d = args.clients, 16, 2
    wl = workload.coords_workload(n, ball_size=1, zipf_s=1.03, seed=0x5EED)
    c0, c1 = fhh.KeyCollection(L, d), fhh.KeyCollection(L, d)
    fhh.gen_keys_pair(c0, c1, wl.left, wl.right, wl.root_seeds)
    c0.set_timing(1)
    torch.cuda.synchronize()
    runs = []
    if "party" in args.runs:
        runs += [("party_table", "table"), ("party_table32", "table32")]
    if "loop" in args.runs:
        runs += [("loop_fe", False), ("loop_ring32", True)]
    out = {"workload": "coords", "clients": n, "data_len": L, "d": d, "threshold": args.threshold,
           "ot_ss_k": args.ot_ss_k, "rounds": args.rounds, "gc_chunk_gib": args.chunk_gib, "runs": {}}
    finals = {}
    for rnd in range(-1, args.rounds):   # round -1: cold, discarded
        for name, what in runs:
            for layout in ("tile_major", "row_major"):
                c0.set_table_row_major(layout == "row_major")
                c1.set_table_row_major(layout == "row_major")
                c0.reset_stats()
                tm = {}
                t0 = time.perf_counter()
                if name.startswith("party"):
                    r = fhh.two_party_crawl(c0, c1, args.threshold, channel="inplace", timing=tm, record=False,
                                            material="fresh", form=what, ot_ss_k=args.ot_ss_k)
                else:
                    r = fhh.sim_crawl(c0, c1, args.threshold, mode="fe", prf_seed=7, gc="ot", base_ot=True,
                                      ot_ss_k=args.ot_ss_k, table_ring32=what, record=False)
                torch.cuda.synchronize()
                wall = time.perf_counter() - t0
                print(f"round {rnd} {name} {layout}: {wall:.3f} s", file=sys.stderr, flush=True)
                finals[(name, layout)] = sorted((str(x.path), int(x.value)) for x in r.final)
                if rnd < 0:
                    continue
                f = out["runs"].setdefault(name, {}).setdefault(layout, {"wall_s": [], "gcot_s": [], "phases_s": []})
                f["wall_s"].append(round(wall, 4))
                if name.startswith("party"):
                    f["phases_s"].append({k: round(v, 4) for k, v in tm.items()})
                    f["gcot_s"].append(round(tm["gcot"] + tm["node_sums"], 4))   # row-major sums are a separate pass
                else:
                    f["gcot_s"].append(round(c0.stats()["gcot_ms"] / 1e3, 4))
                f["heavy_hitters"] = len(r.final)
    for name, _ in runs:
        for layout, f in out["runs"][name].items():
            f["wall_median_s"] = statistics.median(f["wall_s"])
            f["gcot_median_s"] = statistics.median(f["gcot_s"])
        out["runs"][name]["same_result"] = finals[(name, "tile_major")] == finals[(name, "row_major")]
    c0.set_table_row_major(False)
    c1.set_table_row_major(False)
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
