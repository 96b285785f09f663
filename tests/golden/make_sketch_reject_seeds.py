#!/usr/bin/env python3
"""Fixture of PRG seeds whose FE stream rejects a draw (tests/test_sketch_edges.py).

FE::from_rng redraws when the low 62 bits of a PrgStream draw are >= p = 2^62 - 2^30 - 1
(field.rs:252-264, fastfield.rs:125-139): about 2^-32 per draw, so no random test seed ever
takes the redraw path of the oracle or the rejection fallback of the sketch kernels. This search
finds, for each target draw position, the first candidate seed (oracle.reject_seed_of(counter),
counters from 0: two SplitMix64 outputs) whose draw at that position is rejected:

  0, 1   rand1, rand2: keystream block 0, the key segment's lane 0
  2      rand3: block 1 half 0
  3      the first node's draw: block 1 half 1
  13     block 6: a middle lane of an 8-lane segment, first pass
  37     block 18: second pass at 8 lanes per key with 2 blocks per pass
  131    block 65: past lane 63
  258    the last live draw of n_nodes = 256: block 129
  511, 512   blocks 255 and 256, where counters stop differing in byte 15 alone

All positions are tested on every candidate (one key expansion, 8 AES blocks), in chunks of 2^28
counters, until each position has a hit; a position's entry is its smallest counter. One entry:

  pos        the target draw position
  counter    the candidate counter
  seed       16 bytes, hex
  value      the rejected 62-bit value, hex
  rejects    every rejecting position among the seed's first 1100 draws (the tests rely on [pos])

Expect about 3 * 2^32 candidates (the slowest of ten 2^-32 events), with high variance. The
committed file took 2^33 candidates: 131 s on 8 CPU threads with AES-NI. Run once by hand; the
suite only reads the JSON (and repeats the search on a window of 6 000 counters around each hit).

Usage: python tests/golden/make_sketch_reject_seeds.py   (writes tests/golden/sketch_reject_seeds.json)
"""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

POSITIONS = [0, 1, 2, 3, 13, 37, 131, 258, 511, 512]
CHUNK = 1 << 28
N_DRAWS = 1100
P = (1 << 62) - (1 << 30) - 1


def main():
    from oracle import oracle as O
    O.build()
    t0 = time.time()
    found = {}
    start = 0
    while len(found) < len(POSITIONS):
        for counter, pos, value in O.find_reject_seed(POSITIONS, start, CHUNK):
            if pos not in found:            # hits come sorted by counter: the first is the smallest
                found[pos] = (counter, value)
                print(f"pos {pos}: counter {counter} value {value:#x} ({time.time() - t0:.1f} s)", flush=True)
        start += CHUNK
    entries = []
    for pos in POSITIONS:
        counter, value = found[pos]
        seed = O.reject_seed_of(counter)
        rejects = [q for q in range(N_DRAWS) if (O.prg_stream_u64(seed, q) & ((1 << 62) - 1)) >= P]
        assert pos in rejects and (O.prg_stream_u64(seed, pos) & ((1 << 62) - 1)) == value
        entries.append({"pos": pos, "counter": counter, "seed": seed.hex(), "value": f"{value:#x}",
                        "rejects": rejects})
    out = os.path.join(HERE, "sketch_reject_seeds.json")
    with open(out, "w") as f:
        json.dump({"p": f"{P:#x}", "n_draws": N_DRAWS, "candidates_searched": start, "entries": entries}, f, indent=1)
        f.write("\n")
    print(f"{out}: {len(entries)} seeds after {start} candidates ({time.time() - t0:.1f} s)")


if __name__ == "__main__":
    main()
