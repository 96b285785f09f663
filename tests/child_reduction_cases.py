"""Cases and CPU models for tests/test_child_reductions.py: the child-level kernels of csrc/fhh_kernels.hip
(k_eq_count, k_share_planes, k_child_sums_fe / _fe255, k_sum_fe / k_sum_fe255) at the edges of their launch
geometry.

Every model is plain numpy or Python ints and exact: bits for the inside matrix and the share planes, 32-bit limb
sums in uint64 (then one Python int per child) for the field values. No kernel code and, but for the share planes
(the oracle's `level_expand` + `share_bits`) and the simulated-OT PRF (`oracle.sim_prf`), no oracle code either.

  A  more than 65 535 children, so the grid-stride loop over children takes a second trip: 65 clients, a frontier
     seeded by `tree_init_at` that holds the depth-16 (d = 1) or depth-8 (d = 2) ancestors of the clients' intervals
     at its front (the blocks that stride) and at its back (children >= 65 535)
  B  the client loop of the node sums: values for n around the multiples of its 256 threads
  C  k_child_sums_fe's client chunks of 4096 and k_eq_count's word regimes (nw <= 1024, <= 2048, beyond)"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

from loop_frontier_cases import int_bits, intervals, root_seeds

GRID_CAP = 65535          # child_grid(): the most blocks a child-level kernel is launched with
SUM_THREADS = 256         # kReduceThreads: one trip of k_sum_fe's / k_sum_fe255's client loop
SIM_OT_CHUNK = 4096       # kSimOtChunk: clients per blockIdx.y chunk of k_child_sums_fe
EQ_THREADS = 1024         # kEqThreads: k_eq_count takes words w and w + 1024 per thread and pass

FE_P = (1 << 62) - (1 << 30) - 1
FE255_P = (1 << 255) - 19
_M32 = np.uint64(0xFFFFFFFF)
_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)
_S32 = np.uint64(32)


# ---- models ------------------------------------------------------------------------------------------------

def inside(left, right, paths) -> np.ndarray:
    """bool [C][n]: client i is inside node c iff in every dim left[i][:k] <= paths[c] <= right[i][:k] as MSB-first
    integers (`retain_cases.recount`'s rule, the whole matrix instead of its row sums)."""
    paths = np.asarray(paths, np.uint8)
    C, d, k = paths.shape
    w = (1 << np.arange(k - 1, -1, -1)).astype(np.int64)
    lo = (left[:, :, :k].astype(np.int64) * w).sum(-1)        # [n][d]
    hi = (right[:, :, :k].astype(np.int64) * w).sum(-1)
    p = (paths.astype(np.int64) * w).sum(-1)                  # [C][d]
    out = np.ones((C, left.shape[0]), bool)
    for j in range(d):
        out &= (lo[None, :, j] <= p[:, None, j]) & (p[:, None, j] <= hi[None, :, j])
    return out


def children_of(parents, d: int) -> np.ndarray:
    """uint8 [F << d][d][k + 1]: the children of frontier paths [F][d][k] in the engine's order (child c has parent
    c >> d and, in dim j, direction bit j of c & (2^d - 1)). `retain_cases.children_of`, vectorised."""
    parents = np.asarray(parents, np.uint8)
    F = parents.shape[0]
    i = np.arange(F << d) & ((1 << d) - 1)
    bit = ((i[:, None] >> np.arange(d)) & 1).astype(np.uint8)
    return np.concatenate([np.repeat(parents, 1 << d, axis=0), bit[:, :, None]], axis=2)


def pack_planes(bits) -> np.ndarray:
    """share bits [C][n][K] -> uint64 [C][K][nw] as fhh_tree_crawl documents its planes: bit (i % 64) of word i / 64
    is client i's, the lanes past n are zero."""
    bits = np.asarray(bits, np.uint8)
    C, n, K = bits.shape
    nw = (n + 63) // 64
    b = np.zeros((C, K, nw * 64), np.uint8)
    b[:, :, :n] = bits.transpose(0, 2, 1)
    return np.ascontiguousarray(np.packbits(b, axis=2, bitorder="little")).view(np.uint64).reshape(C, K, nw)


def oracle_frontier_states(O, keys, paths):
    """One server's oracle States of the distinct nodes paths [F][d][depth], and ids [F]: node k's row in them.
    Level by level from the root, expanding only the distinct prefixes of the paths (`level_expand`'s parent_idx
    picks the parents, the children that are nobody's prefix are dropped)."""
    F, d, depth = paths.shape
    dirs = (paths.astype(np.int64) << np.arange(d)[None, :, None]).sum(1)      # [F][depth]: child number per level
    st = O.tree_init(keys)
    ids = np.zeros(F, np.int64)
    for lv in range(depth):
        out, _ = O.level_expand(keys, st, np.arange(st.t.shape[0], dtype=np.uint64), lv)
        uniq, ids = np.unique((ids << d) | dirs[:, lv], return_inverse=True)
        st = O.States(np.ascontiguousarray(out.seed[uniq]), np.ascontiguousarray(out.t[uniq]),
                      np.ascontiguousarray(out.y[uniq]))
    return st, ids.reshape(F)


def share_planes_model(O, keys, paths) -> np.ndarray:
    """One server's share planes [F << d][2d][nw] of the children of the frontier `paths`, from the oracle's
    `level_expand` + `share_bits` on that server's keys alone."""
    st, ids = oracle_frontier_states(O, keys, paths)
    ch, _ = O.level_expand(keys, st, ids.astype(np.uint64), paths.shape[2])
    return pack_planes(O.share_bits(ch))


def _limb_ints(limbs) -> list:
    """uint64 limb sums [C][K] (limb k weighs 2^(32 k)) -> one Python int per row."""
    cols = [[int(x) for x in limbs[:, k]] for k in range(limbs.shape[1])]
    return [sum(v << (32 * k) for k, v in enumerate(row)) for row in zip(*cols)]


def _halves(words) -> np.ndarray:
    """u64 words [W] of [C][n] arrays, least significant first -> their 32-bit limbs summed over the clients,
    uint64 [C][2 W] (n < 2^32 clients cannot overflow a limb sum)."""
    out = []
    for w in words:
        out += [(w & _M32).sum(1, dtype=np.uint64), (w >> _S32).sum(1, dtype=np.uint64)]
    return np.stack(out, axis=1)


def _prf(seed, level, C, n, client_base, word):
    from oracle import oracle as O
    ch = np.arange(C, dtype=np.uint64)[:, None]
    with np.errstate(over="ignore"):
        cl = (np.uint64(client_base) + np.arange(n, dtype=np.uint64))[None, :]
    return O.sim_prf(seed, level, ch, cl, word)


def sim_sums_fe(eq, seed: int, level: int, client_base: int = 0):
    """The servers' canonical FE sums of the simulated OT (collect.rs:439-501), per child, as Python ints: r0 =
    prf(seed, level, child, client_base + i, 0) as in `oracle.sim_r0_fe`, server 0 sums r1 = r0 + 1, server 1 sums r0
    where eq[c][i] and r1 elsewhere. `oracle.sim_ot_sums_fe` without its per-element loops."""
    eq = np.asarray(eq, bool)
    C, n = eq.shape
    r = _prf(seed, level, C, n, client_base, 0) & np.uint64((1 << 62) - 1)
    r0 = np.where(r >= np.uint64(FE_P), r - np.uint64(FE_P), r)
    r1 = np.where(r0 == np.uint64(FE_P - 1), np.uint64(0), r0 + np.uint64(1))
    s0 = _limb_ints(_halves([r1]))
    s1 = _limb_ints(_halves([np.where(eq, r0, r1)]))
    return [v % FE_P for v in s0], [v % FE_P for v in s1]


def _is_p255(w):
    """Elementwise: the 255-bit value of the four words is p = 2^255 - 19 or above."""
    return (w[3] == np.uint64((1 << 63) - 1)) & (w[2] == _M64) & (w[1] == _M64) & (w[0] >= np.uint64((1 << 64) - 19))


def sim_sums_fe255(eq, seed: int, level: int, client_base: int = 0):
    """As sim_sums_fe for FieldElm: r0 = the four prf words, little-endian, masked to 255 bits and reduced once
    (`oracle.sim_r0_fe255`); the UNREDUCED sums (add_lazy, field.rs:337-339) of r1 and of r0 / r1 by eq."""
    eq = np.asarray(eq, bool)
    C, n = eq.shape
    w = [_prf(seed, level, C, n, client_base, k) for k in range(4)]
    w[3] = w[3] & np.uint64((1 << 63) - 1)
    with np.errstate(over="ignore"):
        big = _is_p255(w)                                          # r0 = w - p there: a value below 19
        r0 = [np.where(big, w[0] - np.uint64((1 << 64) - 19), w[0])] + [np.where(big, np.uint64(0), x) for x in w[1:]]
        r1, carry = [], np.ones((C, n), bool)
        for x in r0:                                               # r0 + 1, word by word
            s = x + carry.astype(np.uint64)
            carry = carry & (s == 0)
            r1.append(s)
        wrap = _is_p255(r1)                                        # r0 = p - 1: r1 = 0
        r1 = [np.where(wrap, np.uint64(0), x) for x in r1]
    got = [np.where(eq, a, b) for a, b in zip(r0, r1)]
    return _limb_ints(_halves(r1)), _limb_ints(_halves(got))


def node_sums_fe_model(vals) -> list:
    """u64 values [C][n] -> their exact integer sums mod FE_P (collect.rs:487-501)."""
    return [v % FE_P for v in _limb_ints(_halves([np.asarray(vals, np.uint64)]))]


def node_sums_fe255_model(limbs):
    """u32 little-endian limbs [C][n][8] -> (the exact unreduced integer sums, those mod FE255_P)."""
    unr = _limb_ints(np.asarray(limbs, np.uint32).sum(1, dtype=np.uint64))
    return unr, [v % FE255_P for v in unr]


def blockpair_limbs(raw) -> np.ndarray:
    """BlockPairs [C][n][32] (the value's big-endian bytes, field.rs:465-492) -> u32 little-endian limbs [C][n][8]."""
    raw = np.asarray(raw, np.uint8)
    return np.ascontiguousarray(raw[..., ::-1]).view("<u4").astype(np.uint32)


# ---- A. more than 65 535 children ----------------------------------------------------------------------------

WIDE_CLIENTS = 65         # two words, one valid lane in the second
WIDE = {1: dict(L=18, depth=16, F=32808, seed=41), 2: dict(L=10, depth=8, F=16400, seed=42)}
WIDE_CLUSTERS = 24


@dataclass
class WideCase:
    d: int
    L: int
    depth: int
    left: np.ndarray          # [65][d][L]
    right: np.ndarray
    roots: np.ndarray
    paths: np.ndarray         # [F][d][depth]: the frontier tree_init_at seeds
    n_front: int              # the frontier's first / last nodes that are ancestors of a client's interval
    n_back: int

    @property
    def C(self):
        return self.paths.shape[0] << self.d

    @property
    def strided(self):
        """The children below this index share their block with child index + 65 535."""
        return self.C - GRID_CAP


@functools.lru_cache(maxsize=None)
def wide_case(d: int) -> WideCase:
    """65 clients with small intervals around WIDE_CLUSTERS centres (clients of one centre overlap, so counts
    vary), one client at each end of the domain, and a frontier of F distinct nodes of depth `depth`: the all-0
    path first, the all-1 path last, the ancestors of the clients' intervals split between the front and the back,
    fixed-seed random nodes between them."""
    p = WIDE[d]
    L, depth, F, n = p["L"], p["depth"], p["F"], WIDE_CLIENTS
    rng = np.random.default_rng(p["seed"])
    sh, top = L - depth, (1 << L) - 1
    centres = rng.integers(1, (1 << depth) - 1, size=(WIDE_CLUSTERS, d))
    v = (centres[np.arange(n) % WIDE_CLUSTERS] << sh) + rng.integers(0, 1 << sh, size=(n, d))
    r = rng.integers(0, (1 << sh) + 3, size=(n, d))
    r[n - 1] = 1 << sh                                        # client 64 (the second word's one lane) meets >= 3 nodes
    lo, hi = np.clip(v - r, 0, top), np.clip(v + r, 0, top)
    lo[0], hi[0] = 0, (1 << sh) - 1 + 2                       # both ends of the domain, a little past one node
    lo[1], hi[1] = top - (1 << sh) - 1, top
    left, right = intervals(lo, hi, L)
    # the ancestors: every node of depth `depth` that meets a client's box
    anc = set()
    for i in range(n):
        ranges = [range(int(lo[i, j]) >> sh, (int(hi[i, j]) >> sh) + 1) for j in range(d)]
        grid = np.stack(np.meshgrid(*ranges, indexing="ij"), -1).reshape(-1, d)
        of_i = {tuple(int(x) for x in g) for g in grid}
        anc |= of_i
    all0, all1 = (0,) * d, ((1 << depth) - 1,) * d
    assert all0 in anc and all1 in anc
    rest = sorted(anc - {all0, all1} - of_i)
    rest = sorted(of_i) + [rest[k] for k in rng.permutation(len(rest))]   # client 64's go to the front and the back
    C = F << d
    n_front = -(-(C - GRID_CAP) // (1 << d)) - 1              # the nodes after all-0 with a child below C - 65 535
    n_back = F - (GRID_CAP >> d) - 1                          # the nodes before all-1 with a child >= 65 535
    front, back, extra = rest[0::2][:n_front], rest[1::2][:n_back], rest[0::2][n_front:] + rest[1::2][n_back:]
    fill = []
    for k in rng.permutation(1 << (depth * d)):               # distinct random nodes that are nobody's ancestor
        node = tuple((int(k) >> (depth * j)) & ((1 << depth) - 1) for j in range(d))
        if node not in anc:
            fill.append(node)
            if len(fill) == F - 2 - len(rest):
                break
    front += [fill.pop() for _ in range(n_front - len(front))]
    back += [fill.pop() for _ in range(n_back - len(back))]
    mid = fill + extra
    mid = [mid[k] for k in rng.permutation(len(mid))]
    nodes = np.array([all0] + front + mid + back + [all1], np.int64)
    assert nodes.shape == (F, d) and len({tuple(x) for x in nodes.tolist()}) == F
    paths = np.ascontiguousarray(int_bits(nodes, depth))
    case = WideCase(d, L, depth, left, right, root_seeds(n, d, 400 + d), paths, 1 + len(front), 1 + len(back))
    for a in (case.left, case.right, case.roots, case.paths):
        a.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def wide_inside(d: int) -> np.ndarray:
    """The inside matrix [C][65] of the children of wide_case(d)'s frontier. Never modified."""
    c = wide_case(d)
    m = inside(c.left, c.right, children_of(c.paths, d))
    m.setflags(write=False)
    return m


def wide_keep(C: int, seed: int = 7) -> np.ndarray:
    """A scattered keep mask over C > 65 536 children: both sides of the grid cap, the ends, about 40 random ones."""
    keep = np.zeros(C, bool)
    keep[[0, 1, GRID_CAP - 1, GRID_CAP, GRID_CAP + 1, C - 1]] = True
    keep[np.random.default_rng(seed).choice(C, 40, replace=False)] = True
    return keep


def wide_fe_values(C: int, n: int, seed: int) -> np.ndarray:
    """u64 [C][n]: random over the full range, rows of 2^64 - 1 at children 0, 65 534, 65 535 and C - 1, a zero row."""
    vals = np.random.default_rng(seed).integers(0, 1 << 64, size=(C, n), dtype=np.uint64)
    vals[[0, GRID_CAP - 1, GRID_CAP, C - 1]] = _M64
    vals[GRID_CAP + 7] = 0
    return vals


def wide_fe255_limbs(C: int, n: int, seed: int) -> np.ndarray:
    """u32 limbs [C][n][8], random below 2^256, with the same rows all 0xFFFFFFFF and one row zero."""
    v = np.random.default_rng(seed).integers(0, 1 << 32, size=(C, n, 8), dtype=np.uint32)
    v[[0, GRID_CAP - 1, GRID_CAP, C - 1]] = 0xFFFFFFFF
    v[GRID_CAP + 7] = 0
    return v


def with_pitch(rows, ld: int, seed: int = 99) -> np.ndarray:
    """rows [C][n][...] -> [C][ld][...] with random filler in the columns past n."""
    rows = np.asarray(rows)
    C, n = rows.shape[:2]
    if ld == n:
        return np.ascontiguousarray(rows)
    info = np.iinfo(rows.dtype)
    out = np.random.default_rng(seed).integers(0, int(info.max) + 1, size=(C, ld) + rows.shape[2:], dtype=rows.dtype)
    out[:, :n] = rows
    return out


def fe_blocks(vals, seed: int = 98) -> np.ndarray:
    """u64 values [C][n] -> 16-B OT blocks [C][n][2] u64: the FE in bytes 0..7, random filler in bytes 8..15."""
    vals = np.asarray(vals, np.uint64)
    out = np.random.default_rng(seed).integers(0, 1 << 64, size=vals.shape + (2,), dtype=np.uint64)
    out[..., 0] = vals
    return out


# ---- B. the client loop of the node sums ---------------------------------------------------------------------

LOOP_N = (1, 63, 64, 65, 255, 256, 257, 511, 513, 1000)
LOOP_ROWS = 16
LOOP_SHARDED_N = 64 * 9 + 30      # two shards of 5 words: 320 and 286 clients


def loop_fe_values(n: int) -> np.ndarray:
    """u64 [16][n]: random full range; row 1 all 2^64 - 1; row 2 zero; row 3 nonzero at client n - 1 alone; row 4
    nonzero at client 256 alone (n > 256)."""
    rng = np.random.default_rng(5000 + n)
    vals = rng.integers(0, 1 << 64, size=(LOOP_ROWS, n), dtype=np.uint64)
    vals[1] = _M64
    vals[2:5] = 0
    vals[3, n - 1] = rng.integers(1, 1 << 64, dtype=np.uint64)
    if n > SUM_THREADS:
        vals[4, SUM_THREADS] = rng.integers(1, 1 << 64, dtype=np.uint64)
    return vals


def loop_fe255_limbs(n: int) -> np.ndarray:
    """u32 limbs [16][n][8] with the same special rows (a value of up to 2^256 - 1: BlockPairs are unreduced)."""
    rng = np.random.default_rng(6000 + n)
    v = rng.integers(0, 1 << 32, size=(LOOP_ROWS, n, 8), dtype=np.uint32)
    v[1] = 0xFFFFFFFF
    v[2:5] = 0
    v[3, n - 1] = rng.integers(1, 1 << 32, size=8, dtype=np.uint32)
    if n > SUM_THREADS:
        v[4, SUM_THREADS] = rng.integers(1, 1 << 32, size=8, dtype=np.uint32)
    return v


def loop_workload(n: int):
    """Any keys do (the node sums read values, not states): random intervals, d = 2, L = 4."""
    rng = np.random.default_rng(7000 + n)
    a, b = rng.integers(0, 16, size=(n, 2)), rng.integers(0, 16, size=(n, 2))
    left, right = intervals(np.minimum(a, b), np.maximum(a, b), 4)
    return left, right, root_seeds(n, 2, 7000 + n)


# ---- C. client chunks and word regimes ------------------------------------------------------------------------

CHUNK_N = (4095, 4096, 4097, 8193, 65537, 131137)
CHUNK_LEVELS = 3
CHUNK_THRESHOLD = 0.05


@dataclass
class ChunkCase:
    n: int
    left: np.ndarray
    right: np.ndarray
    roots: np.ndarray
    thr: int
    paths: list               # per level: the children's paths [C][1][level + 1]
    inside: list              # per level: bool [C][n]
    keep: list                # per level: bool [C], count >= thr


@functools.lru_cache(maxsize=None)
def chunk_case(n: int) -> ChunkCase:
    """A Zipf workload cut to 3 levels (d = 1), crawled by the count model: per level the children, who is inside
    them, and the keep mask the crawl prunes by."""
    from fuzzyheavyhitters_amd import workload
    wl = workload.zipf_workload(n, 32, 1, num_sites=40, seed=300 + n % 1000)
    left = np.ascontiguousarray(wl.left[:, :, :CHUNK_LEVELS])
    right = np.ascontiguousarray(wl.right[:, :, :CHUNK_LEVELS])
    thr = max(1, int(CHUNK_THRESHOLD * n))
    case = ChunkCase(n, left, right, np.ascontiguousarray(wl.root_seeds), thr, [], [], [])
    frontier = np.zeros((1, 1, 0), np.uint8)
    for _ in range(CHUNK_LEVELS):
        ch = children_of(frontier, 1)
        m = inside(left, right, ch)
        keep = m.sum(1) >= thr
        case.paths.append(ch)
        case.inside.append(m)
        case.keep.append(keep)
        frontier = ch[keep]
    for a in [left, right, case.roots] + case.paths + case.inside + case.keep:
        a.setflags(write=False)
    return case
