#!/usr/bin/env python3
"""Time of `retain_clients` (fhh_retain_clients: the survivors of a keep mask gathered into a smaller collection on
the GPU) against the route that existed before it and against a plain device copy, in one process on one GPU.

configs[1] by default: 100k Zipf clients, data_len 512, d = 1, threshold 0.001, both servers, at the plaintext
crawl's frontier of --depth (256). A round builds the pair (gen_keys_pair + tree_init_at), drops --drop[0] (1 %) of
the clients, then --drop[1] (50 %) of the rest, the same mask on both servers. Per step it reports

  retain_s      the wall time of both servers' retain_clients (synchronous calls: the host clock around them)
  gather_ms     the column and plane gather kernels' time of both servers (HIP events, fhh_retain_timing)
  route_a_s     the route that exists without it, once (round 0): export_keys of the survivors -> a fresh collection
                -> add_keys -> tree_init_at(frontier_paths), both servers
  memcpy_ms     a device-to-device copy that reads plus writes as many bytes as the two servers' column gathers
                (torch's dst.copy_(src) of two device tensors of half that size), HIP events: the yardstick for the
                gather's rate

and checks once per step (round 0) that the exported states of the retained pair equal route (a)'s; the run exits
non-zero if they differ. Medians and raw rounds go to --out as JSON.

--device-mask adds, under the key "device_mask", the same two steps with the mask starting in device memory, as the
sketch verification leaves it: ok.cpu() -> retain_clients on both servers against retain_clients_device on both
(fhh_retain_clients_device), on twin pairs at the same frontier, with the survivor-list kernels' own time
(profiles/retain/device_mask.json)."""
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
    ap.add_argument("--drop", type=float, nargs="+", default=[0.01, 0.5])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--device-mask", action="store_true",
                    help="also time a mask that starts on the GPU: ok.cpu() -> retain_clients against retain_clients_device")
    ap.add_argument("--mask-rounds", type=int, default=5, help="timed rounds of --device-mask (after one warm-up)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not 0 < a.depth < a.L:
        sys.exit("retain_time: --depth must be in [1, L)")

    import torch
    if not torch.cuda.is_available():
        sys.exit("retain_time: needs a GPU (a CPU run measures nothing)")
    import fuzzyheavyhitters_amd as fhh
    from fuzzyheavyhitters_amd import workload

    wl = workload.zipf_workload(a.n, a.L, a.d, num_sites=a.num_sites, zipf_s=1.03, ball_size=1, seed=a.seed)
    thr = max(1, int(a.threshold * a.n))
    _, mid, _ = workload.plaintext_crawl(wl.left, wl.right, thr, thr, levels=a.depth)
    if not len(mid):
        sys.exit("retain_time: nothing survives to --depth at this threshold")
    paths = np.array([[list(p) for p in node] for node in mid], np.uint8).reshape(len(mid), a.d, a.depth)
    print(f"retain_time: frontier of {len(mid)} nodes at depth {a.depth}", file=sys.stderr, flush=True)
    # the masks: seeded, the same in every round; step k's mask is over the survivors of step k - 1
    rng = np.random.default_rng(a.seed)
    keeps, n_cur = [], a.n
    for frac in a.drop:
        keep = np.ones(n_cur, np.uint8)
        keep[rng.choice(n_cur, int(round(frac * n_cur)), replace=False)] = 0
        keeps.append(keep)
        n_cur = int(keep.sum())

    def build_pair():
        cs = fhh.KeyCollection(a.L, a.d), fhh.KeyCollection(a.L, a.d)
        fhh.gen_keys_pair(*cs, wl.left, wl.right, wl.root_seeds)
        for c in cs:
            c.tree_init_at(paths)
        return cs

    def route_a(cs, keep):
        """(seconds, the fresh pair) of the route without retain_clients, timed from the export to the seeded frontier."""
        kept = np.flatnonzero(keep)
        t0 = time.perf_counter()
        out = []
        for c in cs:
            keys = c.export_keys()
            f = fhh.KeyCollection(a.L, a.d)
            f.add_keys(*[np.ascontiguousarray(k[kept]) for k in keys])
            del keys
            f.tree_init_at(c.frontier_paths())
            out.append(f)
        return time.perf_counter() - t0, out

    def memcpy_ms(nbytes, reps=5):
        src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        src.zero_()
        ms = []
        for r in range(reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dst.copy_(src)
            e1.record()
            torch.cuda.synchronize()
            if r:
                ms.append(e0.elapsed_time(e1))
        return ms

    steps = [{"drop": f, "retain_s": [], "cols_ms": [], "planes_ms": []} for f in a.drop]
    for r in range(a.rounds + 1):                      # round 0 warms up, runs route (a) and the states check
        cs = build_pair()
        for k, keep in enumerate(keeps):
            st = steps[k]
            if r == 0:
                st["n_before"], st["n_after"] = int(keep.size), int(keep.sum())
                st["route_a_s"], fresh = route_a(cs, keep)
            t0 = time.perf_counter()
            for c in cs:
                c.retain_clients(keep)
            s = time.perf_counter() - t0
            tm = [c.retain_timing() for c in cs]
            if r:
                st["retain_s"].append(s)
                st["cols_ms"].append(sum(t[0][0] for t in tm))
                st["planes_ms"].append(sum(t[0][1] for t in tm))
                continue
            st["column_bytes"] = sum(t[1][0] for t in tm)
            st["plane_bytes"] = sum(t[1][1] for t in tm)
            for s_idx, (c, f) in enumerate(zip(cs, fresh)):
                if c.num_clients() != f.num_clients():
                    sys.exit(f"retain_time: step {k}: client counts differ")
                for x, y, name in zip(c.export_states(), f.export_states(), ("seed", "t", "y")):
                    if x.shape != y.shape or not np.array_equal(x, y):
                        sys.exit(f"retain_time: step {k} server {s_idx}: the retained pair's {name} states differ "
                                 "from the export -> add_keys -> tree_init_at route's")
            st["states_equal"] = True
            del fresh
        del cs
    for st in steps:
        st["memcpy_copied_bytes"] = st["column_bytes"] // 2
        st["memcpy_ms_rounds"] = memcpy_ms(st["memcpy_copied_bytes"])
    def device_mask():
        """--device-mask: the mask starts on the GPU (where the sketch verification leaves `ok`). Route (a), the only
        one before retain_clients_device: ok.cpu() -> retain_clients on both servers. Route (b): retain_clients_device
        on both. Twin pairs at the same frontier, the same steps; the wall time is taken between two device
        synchronisations; round 0 warms up and checks that the two pairs' exported states are equal."""
        out = [{"drop": f, "host_mask_s": [], "device_mask_s": [], "words_scan_ms": [], "emit_ms": []} for f in a.drop]
        for r in range(a.mask_rounds + 1):
            pa, pb = build_pair(), build_pair()
            for k, keep in enumerate(keeps):
                st = out[k]
                ok = torch.from_numpy(keep).cuda()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                host = ok.cpu().numpy()
                for c in pa:
                    c.retain_clients(host)
                torch.cuda.synchronize()
                sa = time.perf_counter() - t0
                t0 = time.perf_counter()
                kept = [c.retain_clients_device(ok) for c in pb]
                torch.cuda.synchronize()
                sb = time.perf_counter() - t0
                tm = [c.retain_mask_timing() for c in pb]
                if kept != [int(keep.sum())] * 2:
                    sys.exit(f"retain_time: device mask step {k}: {kept} survivors, {int(keep.sum())} expected")
                if r:
                    st["host_mask_s"].append(sa)
                    st["device_mask_s"].append(sb)
                    st["words_scan_ms"].append(sum(t[0] for t in tm))
                    st["emit_ms"].append(sum(t[1] for t in tm))
                    continue
                st["n_before"], st["n_after"] = int(keep.size), int(keep.sum())
                for s_idx, (x, y) in enumerate(zip(pa, pb)):
                    for u, v, name in zip(x.export_states(), y.export_states(), ("seed", "t", "y")):
                        if u.shape != v.shape or not np.array_equal(u, v):
                            sys.exit(f"retain_time: device mask step {k} server {s_idx}: the {name} states of the two "
                                     "routes differ")
                st["states_equal"] = True
            del pa, pb
        steps_out = []
        for st in out:
            ha, hb = statistics.median(st["host_mask_s"]), statistics.median(st["device_mask_s"])
            steps_out.append({
                "drop": st["drop"], "n_before": st["n_before"], "n_after": st["n_after"], "states_equal": st["states_equal"],
                "host_mask_s_median": ha, "host_mask_s_rounds": st["host_mask_s"],
                "device_mask_s_median": hb, "device_mask_s_rounds": st["device_mask_s"],
                "host_over_device": ha / hb,
                "words_scan_ms_median": statistics.median(st["words_scan_ms"]), "words_scan_ms_rounds": st["words_scan_ms"],
                "emit_ms_median": statistics.median(st["emit_ms"]), "emit_ms_rounds": st["emit_ms"],
            })
        return {"rounds": a.mask_rounds, "warmup_rounds": 1,
                "timed": "host_mask_s: ok.cpu() -> retain_clients on both servers; device_mask_s: retain_clients_device "
                         "on both servers; host clock between two device synchronisations, each round on fresh pairs; "
                         "words_scan_ms / emit_ms: the survivor-list kernels of both servers, HIP events",
                "steps": steps_out}

    res = {"n": a.n, "L": a.L, "d": a.d, "depth": a.depth, "threshold": a.threshold, "frontier_nodes": len(mid),
           "rounds": a.rounds, "warmup_rounds": 1, "servers": 2,
           "timed": "retain_s / route_a_s: host clock around both servers' synchronous calls; *_ms: HIP events",
           "device": torch.cuda.get_device_name(0), "steps": []}
    for st in steps:
        cols, mc = statistics.median(st["cols_ms"]), statistics.median(st["memcpy_ms_rounds"])
        res["steps"].append({
            "drop": st["drop"], "n_before": st["n_before"], "n_after": st["n_after"], "states_equal": st["states_equal"],
            "retain_s_median": statistics.median(st["retain_s"]), "retain_s_rounds": st["retain_s"],
            "column_gather_ms_median": cols, "column_gather_ms_rounds": st["cols_ms"],
            "plane_gather_ms_median": statistics.median(st["planes_ms"]), "plane_gather_ms_rounds": st["planes_ms"],
            "column_bytes_read_plus_written": st["column_bytes"], "plane_bytes_read_plus_written": st["plane_bytes"],
            "column_gather_GBps": st["column_bytes"] / (cols * 1e-3) / 1e9,
            "memcpy_copied_bytes": st["memcpy_copied_bytes"], "memcpy_ms_median": mc, "memcpy_ms_rounds": st["memcpy_ms_rounds"],
            "memcpy_GBps_read_plus_written": st["column_bytes"] / (mc * 1e-3) / 1e9,
            "column_gather_over_memcpy": cols / mc,
            "route_a_s": st["route_a_s"], "route_a_over_retain": st["route_a_s"] / statistics.median(st["retain_s"]),
        })
    if a.device_mask:
        res["device_mask"] = device_mask()
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
