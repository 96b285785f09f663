"""Inputs shared by the fhh_join_plan (CPU) and fhh_join_clients_bincode (GPU) tests: the (n, m) pairs, the plan in
Python integers, and a clustered population keyed by the oracle (oracle.gen_keys on oracle.l_inf_ball_bounds).
Nothing here calls the code under test."""
import functools

import numpy as np

import ball_cases as bc

# a word being filled (1 + 1, 63 + 1), the first lane of a new word (64 + 1), a shared first word that the joiners
# fill exactly (65 + 63), a shared first word + full words + a partial last one (70 + 130), the aligned case
# (128 + 64), one client into a partial third word (130 + 1)
PAIRS = [(1, 1), (63, 1), (64, 1), (65, 63), (70, 130), (128, 64), (130, 1)]
N_MAX = 200
L = 40
FIELDS = ("key_idx", "root_seed", "cw_seed", "cw_bits")


def plan(d, depth, n, m, U, grid):
    """fhh_join_plan in Python integers: an item is one 64-client word of one side of 4 prefixes, on workgroups of
    16 waves."""
    assert len(U) == d
    first_word, new_nw = n // 64, (n + m + 63) // 64
    words = new_nw - first_word
    items = sum(2 * words * ((u + 3) // 4) for u in U)
    blocks = min((items + 15) // 16, grid)
    waves = 16 * blocks
    trips = (items + waves - 1) // waves
    return {"first_word": first_word, "first_mask": ((1 << 64) - 1) & ~((1 << (n % 64)) - 1), "words": words,
            "new_nw": new_nw, "items": items, "waves": waves, "trips": trips,
            "last_trip_items": items - (trips - 1) * waves, "aes_blocks": depth * 2 * sum(U) * m}


assert plan(1, 3, 70, 130, [5], 256) == {"first_word": 1, "first_mask": (1 << 64) - 64, "words": 3, "new_nw": 4,
                                         "items": 12, "waves": 16, "trips": 1, "last_trip_items": 12,
                                         "aes_blocks": 3 * 2 * 5 * 130}
assert plan(1, 0, 128, 64, [1], 1)["first_mask"] == (1 << 64) - 1


def population(seed, d, n, sites=3, jitter_bits=2):
    """Bit points [n][d][L]: in every dim a client sits near one of `sites` values (drawn per dim, so that nodes
    share dim prefixes), the low `jitter_bits` bits its own. The frontier of a crawl at threshold 1 stays a few
    nodes wide until the last levels."""
    rng = np.random.default_rng(seed)
    centre = [[(int(rng.integers(1, 1 << 30)) << (L - 31)) | (1 << (jitter_bits + 2)) for _ in range(sites)] for _ in range(d)]
    vals = []
    for _ in range(n):
        for j in range(d):
            vals.append(centre[j][int(rng.integers(sites))] + int(rng.integers(1 << jitter_bits)))
    return bc.alpha_array(vals, d, L)


class Keyed:
    """A population with both servers' oracle keys: alpha / left / right [n][d][L], k[s] dicts of add_keys arrays."""

    def __init__(self, oracle, d, n, delta, seed, roots=None):
        self.d, self.n, self.delta = d, n, delta
        self.alpha = population(seed, d, n)
        self.left, self.right = bc.oracle_bounds(oracle, self.alpha, delta)
        rng = np.random.default_rng(seed + 1)
        self.roots = rng.integers(0, 256, (n, d, 2, 2, 16), dtype=np.uint8) if roots is None else roots(self)
        s = oracle.gen_keys(self.left, self.right, self.roots)
        self.k = [{f: np.array(getattr(x, f), np.uint8, copy=True) for f in FIELDS} for x in s]
        for a in (self.alpha, self.left, self.right, self.roots, *[x[f] for x in self.k for f in FIELDS]):
            a.setflags(write=False)

    def arrays(self, s, lo, hi):
        """server s's keys of the clients [lo, hi) as add_keys takes them"""
        return [np.ascontiguousarray(self.k[s][f][lo:hi]) for f in FIELDS]

    def request(self, s, lo, hi):
        """server s's add_keys request of the clients [lo, hi)"""
        from fuzzyheavyhitters_amd import workload
        return workload.add_keys_request_bincode(*self.arrays(s, lo, hi))


@functools.lru_cache(maxsize=None)
def _keyed(d, n, delta, seed):
    from oracle import oracle
    oracle.build()
    return Keyed(oracle, d, n, delta, seed)


def keyed(d, n=N_MAX, delta=1, seed=0):
    """The shared, read-only population of a dim count (keyed once per process)."""
    return _keyed(d, n, delta, 500 + 10 * d + seed)


def record_bytes(d, data_len=L):
    return 8 + 2 * d * (25 + 20 * data_len)


def recount_chunked(recount, left, right, paths, chunk=1024):
    """retain_cases.recount over many children, a chunk at a time"""
    out = [recount(left, right, paths[a:a + chunk]) for a in range(0, len(paths), chunk)]
    return np.concatenate(out) if out else np.zeros(0, np.uint64)
