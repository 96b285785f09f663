"""k_expand's wide-launch scheduling regimes, every client, at small sizes.

item_layout (csrc/fhh_internal.h) picks k_expand's work decomposition from the ratio of work
(live entries x 64-client words) to the persistent grid's waves: entries per item g (the CorWord
reuse), words per item wpi (variant 52), a statically dealt first item, one head or eight per-XCD
heads with stealing. On the occupancy grid (256 workgroups x 16 waves) the all-client parity tests
(n <= 4 000) only ever see g = 1, wpi = 1 and a single head; the other regimes ran only in the
100k / 1M tests, which sample one client per word. fhh_set_expand_grid shrinks the grid to a few
workgroups, so n = 16 385 reaches g = 16, wpi up to 16 with a partial last chunk, dynamic draws past
the static items and heads without a home block — and the oracle can afford every client.

Workload: client i holds the L = 8 bit string S[i % m] (left = right) of a trie whose frontier
widths are 1, 2, 3, 5, 8, 13, 21, 40 at threshold 1. d = 2: dim 0 holds S, dim 1 holds S >> 2, so
the nodes are the same 1 .. 40 while dim 1 has the live entries of two levels earlier (jobs of
unequal size). Outputs are compared bit for bit: there is no tolerance.
"""
import ctypes
import functools

import numpy as np
import pytest

L = 8
WIDTHS = [1, 2, 3, 5, 8, 13, 21, 40]      # frontier nodes expanded at level 0 .. 7
LEAVES = 56                               # distinct strings (kept children of the last level)
WAVES_PER_BLOCK = 16                      # both built variants run 1024-thread workgroups
MAX_GROUP = {52: 16, 33: 16}              # expand_max_group
MAX_WPI = {52: 16, 33: 1}                 # expand_max_wpi
MW_ITEMS_PER_WAVE = 4                     # kMwItemsPerWave
VARIANTS = [52, 33]
GRIDS = [1, 2, 3, 8, 9]
PATHS = ["dropin", "host-loop", "device-loop"]
# (n, grids): 16 385 / 16 447 leave 1 / 63 clients in the last word (nw = 257); n = 1 000 on 8 or 9
# workgroups has no more items than waves at F = 1 (every item static, a head drawn from is dry)
SIZES = [(16385, GRIDS), (16447, GRIDS), (1000, [8, 9])]
CASES = [(n, d, grid, variant, path) for n, grids in SIZES for d in (1, 2) for grid in grids
         for variant in VARIANTS for path in PATHS]


def case_id(c):
    n, d, grid, variant, path = c
    return f"n{n}-d{d}-grid{grid}-v{variant}-{path}"


# ---- workload ------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def trie_strings() -> np.ndarray:
    """[LEAVES][L] bits: WIDTHS[l] distinct prefixes of length l. The nodes of one length are kept
    in lexicographic order; the first WIDTHS[l + 1] - WIDTHS[l] of them get both children, the
    others one child whose bit alternates with the node's index."""
    nodes = [()]
    for lvl in range(L):
        want = WIDTHS[lvl + 1] if lvl + 1 < L else LEAVES
        both = want - len(nodes)
        assert 0 <= both <= len(nodes)
        nxt = []
        for k, p in enumerate(nodes):
            nxt += [p + (0,), p + (1,)] if k < both else [p + ((k + lvl) & 1,)]
        nodes = nxt
    S = np.array(nodes, np.uint8)
    assert S.shape == (LEAVES, L) and len({tuple(r) for r in S}) == LEAVES
    return S


def client_strings(d: int) -> np.ndarray:
    """[LEAVES][d][L]: dim 0 = S, dim 1 = S >> 2."""
    S = trie_strings()
    out = np.zeros((LEAVES, d, L), np.uint8)
    out[:, 0] = S
    if d == 2:
        out[:, 1, 2:] = S[:, :L - 2]
    return out


def make_workload(n: int, d: int):
    bits = np.ascontiguousarray(client_strings(d)[np.arange(n) % LEAVES])
    roots = np.random.default_rng(1000 * d + n).integers(0, 256, size=(n, d, 2, 2, 16), dtype=np.uint8)
    return bits, bits.copy(), roots


def frontier_shapes(d: int):
    """Per level: (frontier nodes F, live entries per dim) of the crawl at threshold 1 — the
    distinct per-dim prefixes of the kept nodes."""
    B = client_strings(d)
    out = []
    for lvl in range(L):
        F = len({tuple(B[k, :, :lvl].reshape(-1)) for k in range(LEAVES)})
        out.append((F, [len({tuple(B[k, j, :lvl]) for k in range(LEAVES)}) for j in range(d)]))
    return out


# ---- item_layout, restated -------------------------------------------------------------------------

def layout_port(n_live, nw, grid_waves, max_group, max_wpi):
    """csrc/fhh_internal.h item_layout: (g, wpi, total)."""
    entries = sum(n_live)
    g = min(max(entries * nw // (2 * grid_waves), 1), max_group)
    groups = sum((x + g - 1) // g for x in n_live)
    wpi = 1
    if max_wpi > 1 and groups:
        e_eff = entries // groups
        wpi = 1 if e_eff >= max_group else min(max_group // e_eff, max_wpi)
        while wpi > 1 and groups * ((nw + wpi - 1) // wpi) < MW_ITEMS_PER_WAVE * grid_waves:
            wpi -= 1
    total = ((nw + wpi - 1) // wpi) * groups
    return g, wpi, total


def lib_layout(lib, variant, grid, n_live, nw):
    nl = (ctypes.c_uint32 * len(n_live))(*n_live)
    g, wpi = ctypes.c_uint32(), ctypes.c_uint32()
    tot = ctypes.c_uint64()
    rc = lib.fhh_expand_layout(variant, grid, len(n_live), nl, nw, ctypes.byref(g), ctypes.byref(wpi),
                               ctypes.byref(tot))
    assert rc == 0, lib.fhh_last_error(None)
    return g.value, wpi.value, tot.value


def launch_plan(case):
    """The n_live of every k_expand launch of a case: the drop-in API launches one ctx's d jobs,
    the host loop and the device loop both servers' 2 d jobs."""
    n, d, grid, variant, path = case
    return [(live if path == "dropin" else live + live) for _, live in frontier_shapes(d)]


# ---- CPU tests ---------------------------------------------------------------------------------------

def test_trie_widths():
    for d in (1, 2):
        shapes = frontier_shapes(d)
        assert [F for F, _ in shapes] == WIDTHS
        assert [live[0] for _, live in shapes] == WIDTHS
    assert [live[1] for _, live in frontier_shapes(2)] == [1, 1] + WIDTHS[:L - 2]


def test_layout_port_equals_library(fhh):
    """fhh_expand_layout (the library's item_layout with the variant's caps) = the Python port over
    random launches and over every launch of the GPU cases."""
    lib = fhh.lib()
    rng = np.random.default_rng(52)
    draws = []
    for _ in range(4000):
        njobs = int(rng.integers(1, 9))
        hi = int(rng.choice([2, 20, 300, 5000, 200000]))
        n_live = [int(x) for x in rng.integers(0 if hi > 2 else 1, hi, njobs)]
        nw = int(rng.choice([1, 2, 16, 63, 257, 1563, 15625, int(rng.integers(1, 20000))]))
        grid = int(rng.choice([1, 2, 3, 8, 9, 64, 256, int(rng.integers(1, 513))]))
        draws.append((int(rng.choice(VARIANTS)), grid, n_live, nw))
    for case in CASES:
        n, d, grid, variant, path = case
        draws += [(variant, grid, live, (n + 63) // 64) for live in launch_plan(case)]
    for variant, grid, n_live, nw in draws:
        exp = layout_port(n_live, nw, grid * WAVES_PER_BLOCK, MAX_GROUP[variant], MAX_WPI[variant])
        assert lib_layout(lib, variant, grid, n_live, nw) == exp, (variant, grid, n_live, nw)
    # the table of the default variant on one workgroup at n = 16 385 (nw = 257)
    tab = {(1, 1): (16, 8), (1, 2): (16, 8), (1, 3): (16, 5), (1, 5): (16, 3), (1, 8): (16, 2), (1, 13): (16, 1),
           (2, 1): (16, 16), (2, 2): (16, 8)}
    for (d, F), (g, wpi) in tab.items():
        assert lib_layout(lib, 52, 1, [F] * (2 * d), 257)[:2] == (g, wpi), (d, F)


def test_expand_layout_rejects_bad_arguments(fhh):
    lib = fhh.lib()
    one = (ctypes.c_uint32 * 1)(1)
    for variant, grid, njobs, nl, nw in [(0, 1, 1, one, 1), (53, 1, 1, one, 1), (-1, 1, 1, one, 1), (52, 0, 1, one, 1),
                                         (52, 1, 0, one, 1), (52, 1, 9, one, 1), (52, 1, 1, None, 1),
                                         (52, 1, 1, one, 0)]:
        assert lib.fhh_expand_layout(variant, grid, njobs, nl, nw, None, None, None) != 0
    assert lib.fhh_expand_layout(52, 1, 1, one, 1, None, None, None) == 0


def test_cases_visit_every_regime(fhh):
    """The GPU cases below, by fhh_expand_layout on each launch's n_live, reach every regime of
    k_expand's scheduling (a shape change that falls back to the trivial one fails here)."""
    lib = fhh.lib()
    seen_g, seen_wpi, seen_static = set(), set(), set()
    partial_group = partial_chunk = narrow_then_wide = homeless_steal = False
    for case in CASES:
        n, d, grid, variant, path = case
        nw, nwaves = (n + 63) // 64, grid * WAVES_PER_BLOCK
        prev_wpi = None
        for n_live in launch_plan(case):
            g, wpi, total = lib_layout(lib, variant, grid, n_live, nw)
            seen_g.add(g)
            partial_group |= g > 1 and any(x % g for x in n_live)
            seen_static.add(total <= nwaves)
            if variant == 52:
                seen_wpi.add(wpi)
                partial_chunk |= wpi > 1 and nw % wpi != 0
                narrow_then_wide |= prev_wpi is not None and prev_wpi > 1 and wpi == 1
                # eight heads, fewer than eight workgroups, dynamic draws: heads reached by stealing only
                homeless_steal |= wpi > 1 and grid < 8 and total > nwaves
                prev_wpi = wpi
    assert 1 in seen_g and 16 in seen_g and seen_g & set(range(2, 16)), seen_g
    assert partial_group
    assert 1 in seen_wpi and 16 in seen_wpi and seen_wpi & set(range(2, 16)), seen_wpi
    assert partial_chunk
    assert seen_static == {True, False}
    assert narrow_then_wide and homeless_steal
    assert {c[2] for c in CASES} == set(GRIDS) and {c[0] % 64 for c in CASES} >= {1, 63}


# ---- GPU tests ---------------------------------------------------------------------------------------

class Ref:
    """One workload's keys and the oracle's crawl with every level's EvalStates (both servers)."""

    def __init__(self, oracle, n, d):
        self.n, self.d = n, d
        self.left, self.right, self.roots = make_workload(n, d)
        self.k0, self.k1 = oracle.gen_keys(self.left, self.right, self.roots)
        self.crawl = oracle.crawl(self.k0, self.k1, 0.0, mode="count", keep_states=True)
        assert self.crawl.n_children == [F << d for F in WIDTHS]
        assert [int(k.sum()) for k in self.crawl.keeps] == WIDTHS[1:] + [LEAVES]
        for s in self.crawl.states0 + self.crawl.states1:   # shared by every case: never written
            for a in (s.seed, s.t, s.y):
                a.setflags(write=False)


_REF = {}


def get_ref(oracle, n, d) -> Ref:
    """The reference of (n, d), computed once for the run of cases that share it (CASES is ordered by
    size, then d); only one is held at a time (d = 2 at n = 16 385 holds ~0.8 GB of states)."""
    if (n, d) not in _REF:
        _REF.clear()
        _REF[(n, d)] = Ref(oracle, n, d)
    return _REF[(n, d)]


@pytest.fixture(scope="module", autouse=True)
def _drop_ref():
    yield
    _REF.clear()


def full_grid(variant) -> int:
    from fuzzyheavyhitters_amd import lib
    full = ctypes.c_int()
    assert lib().fhh_variant_info(variant, None, 0, None, ctypes.byref(full)) == 0
    return full.value


def make_pair(ref, variant, grid):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import fuzzyheavyhitters_amd as fhh
    c0, c1 = fhh.KeyCollection(L, ref.d), fhh.KeyCollection(L, ref.d)
    fhh.gen_keys_pair(c0, c1, ref.left, ref.right, ref.roots)
    for c in (c0, c1):
        c.set_variant(variant)      # first: it recomputes the grid
        c.set_expand_grid(grid)
    return c0, c1


def assert_states_equal(got, exp, what, kept=None, clients=None):
    gs, gt, gy = got
    es, et, ey = exp.seed, exp.t, exp.y
    if kept is not None:
        es, et, ey = es[kept], et[kept], ey[kept]
    if clients is not None:
        es, et, ey = es[:, clients], et[:, clients], ey[:, clients]
    assert gs.shape == es.shape, f"{what}: {gs.shape} vs {es.shape}"
    if not np.array_equal(gs, es):
        bad = np.nonzero(np.any(gs != es, axis=-1))
        raise AssertionError(f"{what}: {bad[0].size} seeds differ, first (node, client, dim, side) = "
                             f"{[int(b[0]) for b in bad]}, clients {np.unique(bad[1])[:8].tolist()} ...")
    assert np.array_equal(gt, et), f"{what}: t bits differ"
    assert np.array_equal(gy, ey), f"{what}: y bits differ"


def crawl_dropin(ref, c0, c1, grids=None):
    """Per-ctx launches: every level's children of both servers, every client, against the oracle.
    grids: per level (grid of c0, grid of c1), set before that level's launch."""
    from fuzzyheavyhitters_amd.collection import sim_eq_count
    o = ref.crawl
    c0.tree_init()
    c1.tree_init()
    for lvl in range(L):
        if grids is not None:
            c0.set_expand_grid(grids[lvl][0])
            c1.set_expand_grid(grids[lvl][1])
        C, _ = c0.tree_crawl()
        C1, _ = c1.tree_crawl()
        assert C == C1 == o.n_children[lvl]
        assert_states_equal(c0.export_states(), o.states0[lvl], f"level {lvl} server 0")
        assert_states_equal(c1.export_states(), o.states1[lvl], f"level {lvl} server 1")
        assert np.array_equal(sim_eq_count(c0, c1, C), o.counts[lvl])
        c0.tree_prune(o.keeps[lvl])
        c1.tree_prune(o.keeps[lvl])


def sig(res):
    return (res.level_children.tolist(), res.level_kept.tolist(), [c.tolist() for c in res.counts],
            [(r.path, r.value) for r in res.final])


def assert_sim_crawl_equals_oracle(ref, c0, c1, res, what):
    """The crawl's counts and output, and — the counts do not depend on the AES — the EvalStates of
    every client on the frontier the engines are left with: the children kept at level L - 2, whose
    seeds chain through every earlier level's launch."""
    o = ref.crawl
    assert res.level_children.tolist() == o.n_children
    assert res.level_kept.tolist() == [int(k.sum()) for k in o.keeps]
    for lvl in range(L):
        assert np.array_equal(res.counts[lvl], o.counts[lvl]), f"{what}: counts level {lvl}"
    got = [(tuple(tuple(int(b) for b in p) for p in r.path), int(r.value)) for r in res.final]
    assert got == [(tuple(tuple(int(x) for x in p) for p in fp), int(v))
                   for fp, v in zip(o.final_paths, o.final_values)]
    kept = np.nonzero(o.keeps[L - 2])[0]
    assert_states_equal(c0.export_states(), o.states0[L - 2], f"{what}: frontier server 0", kept=kept)
    assert_states_equal(c1.export_states(), o.states1[L - 2], f"{what}: frontier server 1", kept=kept)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_states_bit_exact_on_small_grid(oracle, case):
    """Every client's seeds / t / y equal the oracle's on a grid of 1 .. 9 workgroups, through the
    drop-in API (per-ctx launches, every level exported), the host-driven pair loop and the device
    loop (LoopCtl's layout from k_loop_init / k_prune; probe at every level)."""
    n, d, grid, variant, path = case
    ref = get_ref(oracle, n, d)
    from fuzzyheavyhitters_amd import sim_crawl
    c0, c1 = make_pair(ref, variant, grid)
    if path == "dropin":
        crawl_dropin(ref, c0, c1)
        return
    host = sim_crawl(c0, c1, 0.0, mode="count", host_loop=True)
    assert_sim_crawl_equals_oracle(ref, c0, c1, host, "host loop")
    if path == "host-loop":
        return
    # every client when the level has few children, else every 7th (7 is coprime to 64: all lanes,
    # and 64 / 7 > 1 keeps several clients in every word)
    for levels, clients in (([lv for lv in range(L) if ref.crawl.n_children[lv] <= 16], np.arange(n)),
                            ([lv for lv in range(L) if ref.crawl.n_children[lv] > 16],
                             np.union1d(np.arange(0, n, 7), [n - 1]))):
        cap = max(ref.crawl.n_children[lv] for lv in levels)
        dev = sim_crawl(c0, c1, 0.0, mode="count", init_capacity=128,
                        probe={"levels": levels, "clients": clients.astype(np.uint64), "capacity": cap})
        assert sig(dev) == sig(host)
        assert_sim_crawl_equals_oracle(ref, c0, c1, dev, "device loop")
        assert set(dev.probe) == set(levels)
        for lv, (seeds, t, y) in dev.probe.items():
            for s, st in ((0, ref.crawl.states0[lv]), (1, ref.crawl.states1[lv])):
                assert_states_equal((seeds[s], t[s], y[s]), st, f"device loop level {lv} server {s}",
                                    clients=clients)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("d", [1, 2])
def test_grid_changes_between_levels(oracle, d, variant):
    """The grid changed before every level of one drop-in crawl, differently on the two servers (the
    layout, the head count and the head set's parity all follow the launch, not the ctx's history)."""
    seq = [1, 9, 2, full_grid(variant), 3, 1, 8, 2]
    ref = get_ref(oracle, 16385, d)
    c0, c1 = make_pair(ref, variant, 1)
    crawl_dropin(ref, c0, c1, grids=[(seq[lv], seq[(lv + 3) % L]) for lv in range(L)])


@pytest.mark.gpu
def test_set_expand_grid_validates():
    """1 .. the variant's occupancy grid is accepted, anything else refused (the override never
    raises the grid)."""
    import fuzzyheavyhitters_amd as fhh
    from fuzzyheavyhitters_amd import FhhError
    c = fhh.KeyCollection(L, 1)
    for variant in VARIANTS:
        c.set_variant(variant)
        full = full_grid(variant)
        for bad in (0, -1, full + 1, 1 << 20):
            with pytest.raises(FhhError, match="set_expand_grid"):
                c.set_expand_grid(bad)
        c.set_expand_grid(1)
        c.set_expand_grid(full)
