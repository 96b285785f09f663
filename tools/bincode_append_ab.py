#!/usr/bin/env python3
"""A/B of the appended add_keys path against the one-shot fhh_add_keys_bincode, in one process on one GPU.

Both build the same population from the same pageable host buffer and are timed on the host clock from the
first call to the end of tree_init (every call is synchronous). The appended path runs per batch size
(default 100 — the reference's addkey_batch_size — 1 000 and 10 000), with a reservation of n and without.
A warm-up round, then --rounds rounds that alternate every configuration; medians and the raw rounds go to
--out as JSON.

The payload is random bytes in valid framing (seeds random, bools 0/1): decode time does not depend on the
key values. A batch's request is the records' slice of the one buffer with the u64 count written over the 8
bytes in front of it for the duration of the call, so no configuration holds a second copy of the 2 GB.
After the timed rounds the first two crawl levels' share planes of an appended and a one-shot collection are
compared (the same device buffers give the same planes)."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def payload(n, L, d, seed):
    """[8 spare bytes][n records] as one uint8 array; returns (buf, R)."""
    KB = 25 + 20 * L
    R = 8 + 2 * d * KB
    rng = np.random.default_rng(seed)
    buf = np.zeros(8 + n * R, np.uint8)
    rec = buf[8:].reshape(n, R)
    rec[:, 0:8] = np.frombuffer(np.uint64(d).tobytes(), np.uint8)
    keys = rec[:, 8:].reshape(n, 2 * d, KB)
    keys[:, :, 0] = rng.integers(0, 2, (n, 2 * d), dtype=np.uint8)
    keys[:, :, 17:25] = np.frombuffer(np.uint64(L).tobytes(), np.uint8)
    step = max(1, (1 << 26) // (2 * d * KB))          # fill in slabs: bounded temporaries
    for a in range(0, n, step):
        b = min(n, a + step)
        keys[a:b, :, 1:17] = rng.integers(0, 256, (b - a, 2 * d, 16), dtype=np.uint8)
        cw = keys[a:b, :, 25:].reshape(b - a, 2 * d, L, 20)
        cw[:, :, :, 0:16] = rng.integers(0, 256, (b - a, 2 * d, L, 16), dtype=np.uint8)
        cw[:, :, :, 16:20] = rng.integers(0, 2, (b - a, 2 * d, L, 4), dtype=np.uint8)
    return buf, R


class Feeder:
    """Requests cut from the one payload buffer: the count header overwrites the 8 bytes before the slice."""

    def __init__(self, buf, R, n):
        self.buf, self.R, self.n = buf, R, n
        self.base = buf.ctypes.data
        self.u8p = ctypes.POINTER(ctypes.c_uint8)

    def call(self, fn, handle, a, m):
        off = a * self.R
        saved = self.buf[off:off + 8].copy()
        self.buf[off:off + 8] = np.frombuffer(np.uint64(m).tobytes(), np.uint8)
        try:
            return fn(handle, ctypes.cast(self.base + off, self.u8p), 8 + m * self.R)
        finally:
            self.buf[off:off + 8] = saved


def build(fhh, feed, L, d, batch, reserve):
    """One collection built and tree_init'ed; returns (collection, seconds, calls)."""
    from fuzzyheavyhitters_amd._lib import check, lib
    c = fhh.KeyCollection(L, d)
    n = feed.n
    t0 = time.perf_counter()
    calls = 0
    if batch is None:
        check(feed.call(lib().fhh_add_keys_bincode, c.handle, 0, n), c.handle)
        calls = 1
    else:
        if reserve:
            c.reserve_clients(n)
        fn = lib().fhh_add_keys_bincode_append
        for a in range(0, n, batch):
            check(feed.call(fn, c.handle, a, min(batch, n - a)), c.handle)
            calls += 1
    c.tree_init()
    return c, time.perf_counter() - t0, calls


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--L", type=int, default=512)
    ap.add_argument("--d", type=int, default=1)
    ap.add_argument("--batches", type=int, nargs="+", default=[100, 1000, 10000])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--per-call", type=int, default=0, metavar="BATCH",
                    help="instead of the A/B: the wall time of every call of the unreserved append in batches of BATCH")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("bincode_append_ab: needs a GPU (a CPU run measures nothing)")
    import fuzzyheavyhitters_amd as fhh

    buf, R = payload(a.n, a.L, a.d, 7)
    feed = Feeder(buf, R, a.n)
    gb = a.n * R / 1e9
    print(f"bincode_append_ab: payload of {gb:.2f} GB ready", file=sys.stderr, flush=True)
    if a.per_call:
        # which calls are slow: every call of the unreserved append in batches of --per-call, two rounds
        from fuzzyheavyhitters_amd._lib import check, lib
        out = {}
        for rnd in range(2):
            c = fhh.KeyCollection(a.L, a.d)
            ts = []
            for c0 in range(0, a.n, a.per_call):
                t0 = time.perf_counter()
                check(feed.call(lib().fhh_add_keys_bincode_append, c.handle, c0, min(a.per_call, a.n - c0)), c.handle)
                ts.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            c.tree_init()
            out[f"round{rnd}"] = {"calls_ms": [round(1e3 * t, 2) for t in ts],
                                  "tree_init_ms": round(1e3 * (time.perf_counter() - t0), 2)}
            c.close()
        print(json.dumps(out))
        if a.out:
            with open(a.out, "w") as f:
                json.dump(out, f)
        return
    configs = [("one_shot", None, False)]
    for b in a.batches:
        configs += [(f"append_{b}_reserved", b, True), (f"append_{b}_unreserved", b, False)]
    rounds = {name: [] for name, _, _ in configs}
    calls = {}
    for r in range(a.rounds + 1):                      # round 0 warms every configuration up
        for name, batch, reserve in configs:
            c, s, k = build(fhh, feed, a.L, a.d, batch, reserve)
            c.close()
            calls[name] = k
            if r:
                rounds[name].append(s)
    base = statistics.median(rounds["one_shot"])
    table = []
    for name, _, _ in configs:
        med = statistics.median(rounds[name])
        table.append({"config": name, "calls": calls[name], "median_s": med, "min_s": min(rounds[name]),
                      "max_s": max(rounds[name]), "per_call_ms": 1e3 * med / calls[name], "payload_GBps": gb / med,
                      "ratio_to_one_shot": med / base})
    # the two paths leave the same device buffers: the same share planes on the first crawl levels
    one, _, _ = build(fhh, feed, a.L, a.d, None, False)
    app, _, _ = build(fhh, feed, a.L, a.d, a.batches[0], False)
    same = True
    for _ in range(2):
        (c1, p1), (c2, p2) = one.tree_crawl(share_planes=True), app.tree_crawl(share_planes=True)
        same = same and c1 == c2 and bool(np.array_equal(p1, p2))
    res = {"n": a.n, "L": a.L, "d": a.d, "payload_GB": gb, "rounds": a.rounds, "warmup_rounds": 1,
           "timed": "host clock, first call to the end of tree_init (synchronous calls), pageable host memory",
           "table": table, "raw_rounds_s": rounds, "planes_equal_first_two_levels": same}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    if not same:
        sys.exit("bincode_append_ab: the appended and the one-shot collection's share planes differ")


if __name__ == "__main__":
    main()
