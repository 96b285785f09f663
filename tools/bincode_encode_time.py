#!/usr/bin/env python3
"""Time of `export_keys_bincode` (device keys -> add_keys requests, serialized on the GPU) against the path it
replaces (`export_keys`, the host's AoS copy of the device layout, + `workload.add_keys_request_bincode`), in
one process on one GPU.

The collection is built once with fhh_add_keys_bincode from a random payload in valid framing (as
tools/bincode_append_ab.py builds it), so the expected export is that payload itself: every configuration's
output is compared with it once, before the timed rounds. Configurations: the whole population as one request,
and the same in batches of --batch clients (default 100, the reference's addkey_batch_size), each on the GPU
path and on the host path. A warm-up round, then --rounds rounds that alternate the configurations; every call
is synchronous and ends with its bytes in pageable host memory, so the host clock around it is the call's time.
Medians and raw rounds go to --out as JSON.

--profile: one add_keys_bincode and one export_keys_bincode (plus one warm-up of each) and nothing else, for

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/bincode_encode_time.py --profile

which puts k_bincode_emit_cw beside the decoder's k_bincode_cw_tiles on the same box."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bincode_append_ab import payload  # noqa: E402


def host_path(c, batch):
    """What a leader had to do before: the AoS export, then the numpy serializer per request."""
    from fuzzyheavyhitters_amd import workload
    ki, rs, cs, cb = c.export_keys()
    n = ki.shape[0]
    B = batch or n
    reqs = [workload.add_keys_request_bincode(ki[a:a + B], rs[a:a + B], cs[a:a + B], cb[a:a + B]) for a in range(0, n, B)]
    return reqs[0] if len(reqs) == 1 else np.concatenate(reqs)


def expected(buf, R, n, batch):
    """The payload's records behind their request counts."""
    B = batch or n
    rec = buf[8:].reshape(n, R)
    parts = []
    for a in range(0, n, B):
        m = min(B, n - a)
        parts += [np.frombuffer(np.uint64(m).tobytes(), np.uint8), rec[a:a + m].reshape(-1)]
    return np.concatenate(parts)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--L", type=int, default=512)
    ap.add_argument("--d", type=int, default=1)
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--profile", action="store_true", help="one decode and one export only (for rocprofv3)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("bincode_encode_time: needs a GPU (a CPU run measures nothing)")
    import fuzzyheavyhitters_amd as fhh

    buf, R = payload(a.n, a.L, a.d, 11)
    buf[:8] = np.frombuffer(np.uint64(a.n).tobytes(), np.uint8)
    gb = a.n * R / 1e9
    print(f"bincode_encode_time: payload of {gb:.2f} GB ready", file=sys.stderr, flush=True)
    if a.profile:
        for _ in range(2):
            c = fhh.KeyCollection(a.L, a.d)
            c.add_keys_bincode(buf)
            out = c.export_keys_bincode()
            c.close()
        if not np.array_equal(out, buf):
            sys.exit("bincode_encode_time: the export differs from the payload")
        return
    c = fhh.KeyCollection(a.L, a.d)
    c.add_keys_bincode(buf)
    configs = [("gpu_whole", lambda: c.export_keys_bincode()), ("host_whole", lambda: host_path(c, 0)),
               (f"gpu_batch{a.batch}", lambda: c.export_keys_bincode(batch=a.batch)),
               (f"host_batch{a.batch}", lambda: host_path(c, a.batch))]
    for name, fn in configs:                           # correctness first: each output is the payload, re-framed
        want = buf if "whole" in name else expected(buf, R, a.n, a.batch)
        if not np.array_equal(fn(), want):
            sys.exit(f"bincode_encode_time: {name} differs from the payload")
    rounds = {name: [] for name, _ in configs}
    for r in range(a.rounds + 1):                      # round 0 warms every configuration up
        for name, fn in configs:
            t0 = time.perf_counter()
            out = fn()
            s = time.perf_counter() - t0
            del out
            if r:
                rounds[name].append(s)
    table = []
    for name, _ in configs:
        med = statistics.median(rounds[name])
        table.append({"config": name, "median_s": med, "min_s": min(rounds[name]), "max_s": max(rounds[name]),
                      "payload_GBps": gb / med})
    med = {t["config"]: t["median_s"] for t in table}
    res = {"n": a.n, "L": a.L, "d": a.d, "batch": a.batch, "payload_GB": gb, "rounds": a.rounds, "warmup_rounds": 1,
           "timed": "host clock around one synchronous call that ends with the bytes in pageable host memory "
                    "(a fresh numpy array per call)",
           "outputs_equal_payload": True, "table": table, "raw_rounds_s": rounds,
           "host_over_gpu_whole": med["host_whole"] / med["gpu_whole"],
           "host_over_gpu_batched": med[f"host_batch{a.batch}"] / med[f"gpu_batch{a.batch}"]}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
