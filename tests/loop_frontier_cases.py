"""Constructed workloads for tests/test_loop_wide_frontier.py and their plaintext reference.

Every workload is a pair of `left` / `right` bit arrays [n][d][L] (MSB first) of integer intervals, made
here from fixed rng seeds or by hand; the reference of every comparison is `workload.plaintext_crawl`
(numpy over the client intervals, no kernel and no oracle code). `reference` adds what the tests need on
top of its output and what follows from it alone: the kept children, their paths and the per-dim live
entries of every level, which are the sizes k_prune's loops run over (csrc/fhh_loop.hip)."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

PRUNE_THREADS = 1024      # k_prune's workgroup: one pass of its loops
GATHER_THREADS = 256      # k_gather_hist's workgroup
DEFAULT_CAPACITY = 256    # the device loop's start capacity (nodes and entries) without init_capacity
CLIENT_CHUNK = 4096       # kSimOtChunk: clients per k_child_sums_fe chunk


def int_bits(v, L: int) -> np.ndarray:
    """ints [...] -> uint8 [..., L], MSB first."""
    v = np.asarray(v, np.int64)
    return ((v[..., None] >> np.arange(L - 1, -1, -1)) & 1).astype(np.uint8)


def intervals(lo, hi, L: int):
    """lo, hi ints [n] or [n][d] -> (left, right) uint8 [n][d][L]."""
    lo, hi = np.asarray(lo, np.int64), np.asarray(hi, np.int64)
    if lo.ndim == 1:
        lo, hi = lo[:, None], hi[:, None]
    assert lo.shape == hi.shape and np.all(lo <= hi) and np.all(lo >= 0) and np.all(hi < (1 << L))
    return np.ascontiguousarray(int_bits(lo, L)), np.ascontiguousarray(int_bits(hi, L))


def root_seeds(n: int, d: int, seed: int) -> np.ndarray:
    return np.random.default_rng([seed, 3]).integers(0, 256, size=(n, d, 2, 2, 16), dtype=np.uint8)


def threshold_count(threshold: float, n_total: int) -> int:
    """thr = thr_last as sim_crawl documents them (below 2^32 they are the same number)."""
    return max(1, int(threshold * n_total))


@dataclass
class Case:
    name: str
    left: np.ndarray
    right: np.ndarray
    roots: np.ndarray
    threshold: float
    n_total: int

    @property
    def thr(self):
        return threshold_count(self.threshold, self.n_total)

    @property
    def dims(self):
        return self.left.shape[1]

    @property
    def levels(self):
        return self.left.shape[2]


@dataclass
class Reference:
    counts: list                  # per level: u64 [C], the leader's child order
    children: list                # per level: C
    kept: list                    # per level: indices of the kept children
    paths: list                   # per level: the kept children's paths, uint8 [nf][d][level + 1]
    live: list                    # per level: [d] distinct per-dim prefixes among the kept children (n_live)
    final: list = field(default_factory=list)   # [(path as nested bool lists, count)]

    @property
    def n_kept(self):
        return [len(k) for k in self.kept]

    @property
    def entries(self):
        """Per level: E = 2 * max_j n_live[j] of the frontier the level expands (1 root entry at level 0)."""
        return [2 * (1 if lv == 0 else max(self.live[lv - 1])) for lv in range(len(self.kept))]


def reference_of(left, right, thr: int, thr_last: int) -> Reference:
    from fuzzyheavyhitters_amd.workload import plaintext_crawl
    n, d, L = left.shape
    counts, fpaths, fcounts = plaintext_crawl(left, right, thr, thr_last)
    ref = Reference([np.asarray(c, np.uint64) for c in counts], [len(c) for c in counts], [], [], [])
    prev = np.zeros((1, d, 0), np.uint8)
    for lv, cnt in enumerate(ref.counts):
        keep = np.nonzero(cnt >= (thr_last if lv == L - 1 else thr))[0]
        f, i = keep >> d, keep & ((1 << d) - 1)
        bit = ((i[:, None] >> np.arange(d)) & 1).astype(np.uint8)              # [nf][d]
        prev = np.concatenate([prev[f], bit[:, :, None]], axis=2)
        ref.kept.append(keep)
        ref.paths.append(prev)
        ref.live.append([len({r.tobytes() for r in prev[:, j]}) for j in range(d)])
    # plaintext_crawl's own final list is the authority; the paths rebuilt from its counts must agree with it
    assert [tuple(tuple(int(b) for b in p) for p in node) for node in prev] == list(fpaths)
    ref.final = [([[bool(b) for b in p] for p in node], c) for node, c in zip(fpaths, fcounts)]
    return ref


@functools.lru_cache(maxsize=None)
def reference(name: str) -> Reference:
    """The reference crawl of a named case, computed once per session and never modified."""
    c = case(name)
    return reference_of(c.left, c.right, c.thr, c.thr)


# ---- 1. frontiers past one k_prune pass ----------------------------------------------------------------

D1_SEED, D1_LEVELS, D1_DISTINCT, D1_REPEATS = 1, 12, 1200, 100
D2_SEED, D2_LEVELS, D2_POINTS = 5, 12, 1100


def _d1_points():
    rng = np.random.default_rng(D1_SEED)
    v = rng.choice(1 << D1_LEVELS, D1_DISTINCT, replace=False)
    return np.concatenate([v, rng.choice(v, D1_REPEATS)])


def _wide_d1_ball0():
    v = _d1_points()
    left, right = intervals(v, v, D1_LEVELS)
    return Case("wide_d1_ball0", left, right, root_seeds(v.size, 1, 101), 0.0, v.size)


def _wide_d1_ball1():
    v = _d1_points()
    left, right = intervals(np.maximum(v - 1, 0), np.minimum(v + 1, (1 << D1_LEVELS) - 1), D1_LEVELS)
    return Case("wide_d1_ball1", left, right, root_seeds(v.size, 1, 102), 0.0, v.size)


def _wide_d2():
    v = np.random.default_rng(D2_SEED).integers(0, 1 << D2_LEVELS, size=(D2_POINTS, 2))
    left, right = intervals(v, v, D2_LEVELS)
    return Case("wide_d2", left, right, root_seeds(D2_POINTS, 2, 103), 0.0, D2_POINTS)


# ---- 2. counts on the threshold ------------------------------------------------------------------------

CAT_LEVELS, CAT_THR, CAT_TOTAL = 10, 5, 1024


def _caterpillars():
    """Two caterpillars, d = 1, L = 10, thr = thr_last = 5 (threshold 5 / 1024 of 1024 clients, exact in binary).
    Under root bit 0 the spine is 0^k; its off-spine child at every depth k >= 2, 0^(k-1) 1, holds thr - 1 clients
    at the one leaf 0^(k-1) 1 0^(L-k): dropped there with a count of thr - 1. The spine's leaf 0^L holds thr.
    Under root bit 1 the spine is 1 0^(k-1); its off-spine child at every depth k >= 2, 1 0^(k-2) 1, holds thr
    clients at one leaf: kept with a count of exactly thr at that and every deeper level, the last included. The
    spine's leaf 1 0^(L-1) holds thr - 1: dropped at the last level."""
    L, thr = CAT_LEVELS, CAT_THR
    vals = [0] * thr + [1 << (L - 1)] * (thr - 1)
    for k in range(2, L + 1):
        vals += [1 << (L - k)] * (thr - 1)
        vals += [(1 << (L - 1)) | (1 << (L - k))] * thr
    v = np.random.default_rng(21).permutation(np.array(vals))
    left, right = intervals(v, v, L)
    return Case("caterpillars", left, right, root_seeds(v.size, 1, 104), CAT_THR / CAT_TOTAL, CAT_TOTAL)


FLOOR_THRESHOLD, FLOOR_TOTAL, FLOOR_THR = 0.29, 100, 28


def _floored_threshold():
    """100 clients at four leaves of a d = 1, L = 8 domain, 28 / 27 / 30 / 15 of them: 0.29 * 100 is
    28.999999999999996 in binary floating point, so the leader's threshold count is 28, not 29."""
    L = 8
    vals = [0b00000000] * 28 + [0b01000000] * 27 + [0b10000000] * 30 + [0b11000000] * 15
    v = np.random.default_rng(22).permutation(np.array(vals))
    left, right = intervals(v, v, L)
    return Case("floored_threshold", left, right, root_seeds(v.size, 1, 105), FLOOR_THRESHOLD, FLOOR_TOTAL)


# ---- 3. FE partials over two client chunks -------------------------------------------------------------

CHUNK_LEVELS, CHUNK_CLIENTS, CHUNK_VALUES, CHUNK_THRESHOLD = 10, 4100, 200, 0.001
CHUNK_LONE_VALUE, CHUNK_LONE_BITS = 0b1011011101, 4   # no other client shares its first 4 bits


def _two_chunks():
    """4100 clients, d = 1, L = 10: the first 4096 (one whole k_child_sums_fe chunk) spread over 200 values, the
    last 4 (the second chunk) alone at one more value, whose first 4 bits none of the 200 has. thr = int(0.001 *
    4100) = 4, so from level 3 on that value's node is kept by the second chunk's clients alone."""
    rng = np.random.default_rng(31)
    pool = np.arange(1 << CHUNK_LEVELS)
    shift = CHUNK_LEVELS - CHUNK_LONE_BITS
    pool = pool[pool >> shift != CHUNK_LONE_VALUE >> shift]
    vals = rng.choice(pool, CHUNK_VALUES, replace=False)
    v = np.concatenate([rng.choice(vals, CLIENT_CHUNK), np.full(CHUNK_CLIENTS - CLIENT_CHUNK, CHUNK_LONE_VALUE)])
    left, right = intervals(v, v, CHUNK_LEVELS)
    return Case("two_chunks", left, right, root_seeds(v.size, 1, 106), CHUNK_THRESHOLD, v.size)


_CASES = {"wide_d1_ball0": _wide_d1_ball0, "wide_d1_ball1": _wide_d1_ball1, "wide_d2": _wide_d2,
          "caterpillars": _caterpillars, "floored_threshold": _floored_threshold, "two_chunks": _two_chunks}
WIDE = ["wide_d1_ball0", "wide_d1_ball1", "wide_d2"]


@functools.lru_cache(maxsize=None)
def case(name: str) -> Case:
    c = _CASES[name]()
    for a in (c.left, c.right, c.roots):
        a.setflags(write=False)
    return c


def _pow2(x: int) -> int:
    return 1 << max(0, int(x) - 1).bit_length()


def planned_aborts(ref: Reference, start: int = DEFAULT_CAPACITY):
    """The aborts of a device-loop crawl of `ref` that starts at capacity `start`, from k_prune's abort rules
    and loop_grow's growth rule alone (no run): [(level, need_entries, need_nodes)]. A level aborts when it keeps
    more nodes than F_cap (need_entries = 2 nf then, the bound), or, not at the last level, when a dim's next
    child table 2 * n_live' exceeds E_cap (the dims after the first such one are not counted). Growth: F_cap' =
    max(F_cap, 2 * pow2(need_nodes)), E_cap' = max(E_cap, 2 * pow2(need_entries)), the first candidate of
    loop_entry_cap, which memory permits at these sizes. An abort starts a capacity epoch: the kept-children rows
    of its level and the later ones move to a new allocation."""
    start = _pow2(start)
    F_cap = E_cap = start
    out = []
    L = len(ref.kept)
    for lv, nf in enumerate(ref.n_kept):
        need_e = None
        if nf > F_cap:
            need_e = 0 if lv == L - 1 else 2 * nf
        elif lv < L - 1:
            for nl in ref.live[lv]:
                if 2 * nl > E_cap:
                    need_e = 2 * nl
                    break
        if need_e is None:
            continue
        out.append((lv, need_e, nf))
        F_cap = max(F_cap, 2 * _pow2(nf))
        E_cap = max(E_cap, 2 * _pow2(max(need_e, 1)))
        assert nf <= F_cap and (lv == L - 1 or 2 * max(ref.live[lv]) <= E_cap)   # the resumed prune fits
    return out
