"""k_expand's entry loop (csrc/fhh_kernels.hip expand_word): the wave-uniform words read ahead through the
scalar path, the next entry's parent words requested behind the AES and in front of the entry's seed stores.

What such a loop can get wrong is its ends: the entry read ahead of an item's last one (nothing may read
live[] at or beyond n_live), a one-entry item (no next entry at all), and the hand-over from one entry's
words to the next. The trie below gives levels of 1, 2, 4, 8, 16 and 17 live entries; on one workgroup and
16 385 clients the items take 16 entries each, so the levels hold a one-entry item, a partial group, a full
group, and a full group plus a group of one. 65 clients (two words, one client in the last) keep one entry
per item. Every client's seeds / t / y are compared with the oracle bit for bit, through the drop-in API,
the host loop and the device loop."""
import functools

import numpy as np
import pytest

from test_expand_regimes import assert_states_equal, sig

L = 6
WIDTHS = [1, 2, 4, 8, 16, 17]   # live entries (frontier nodes) expanded at level 0 .. 5
LEAVES = 18
CASES = [(n, grid, variant, path) for n, grid in ((65, 1), (16385, 1), (16385, 2)) for variant in (52, 33)
         for path in ("dropin", "host-loop", "device-loop")]


@functools.lru_cache(maxsize=None)
def trie_strings() -> np.ndarray:
    """[LEAVES][L] bits with WIDTHS[l] distinct prefixes of length l (as test_expand_regimes.trie_strings)."""
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


class Ref:
    def __init__(self, oracle, n):
        bits = np.ascontiguousarray(trie_strings()[np.arange(n) % LEAVES][:, None, :])
        self.n, self.left, self.right = n, bits, bits.copy()
        self.roots = np.random.default_rng(77 + n).integers(0, 256, size=(n, 1, 2, 2, 16), dtype=np.uint8)
        k0, k1 = oracle.gen_keys(self.left, self.right, self.roots)
        self.crawl = oracle.crawl(k0, k1, 0.0, mode="count", keep_states=True)
        assert self.crawl.n_children == [2 * F for F in WIDTHS]
        assert [int(k.sum()) for k in self.crawl.keeps] == WIDTHS[1:] + [LEAVES]
        for s in self.crawl.states0 + self.crawl.states1:   # shared by every case: never written
            for a in (s.seed, s.t, s.y):
                a.setflags(write=False)


_REF = {}


def get_ref(oracle, n) -> Ref:
    if n not in _REF:
        _REF.clear()
        _REF[n] = Ref(oracle, n)
    return _REF[n]


@pytest.fixture(scope="module", autouse=True)
def _drop_ref():
    yield
    _REF.clear()


def _assert_crawl(ref, c0, c1, res, what):
    o = ref.crawl
    assert res.level_children.tolist() == o.n_children
    assert res.level_kept.tolist() == [int(k.sum()) for k in o.keeps]
    for lvl in range(L):
        assert np.array_equal(res.counts[lvl], o.counts[lvl]), f"{what}: counts level {lvl}"
    kept = np.nonzero(o.keeps[L - 2])[0]
    assert_states_equal(c0.export_states(), o.states0[L - 2], f"{what}: frontier server 0", kept=kept)
    assert_states_equal(c1.export_states(), o.states1[L - 2], f"{what}: frontier server 1", kept=kept)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[f"n{c[0]}-grid{c[1]}-v{c[2]}-{c[3]}" for c in CASES])
def test_entry_loop_states_bit_exact(oracle, case):
    import fuzzyheavyhitters_amd as fhh
    from fuzzyheavyhitters_amd import sim_crawl
    from fuzzyheavyhitters_amd.collection import sim_eq_count
    n, grid, variant, path = case
    ref = get_ref(oracle, n)
    o = ref.crawl
    c0, c1 = fhh.KeyCollection(L, 1), fhh.KeyCollection(L, 1)
    fhh.gen_keys_pair(c0, c1, ref.left, ref.right, ref.roots)
    for c in (c0, c1):
        c.set_variant(variant)      # first: it recomputes the grid
        c.set_expand_grid(grid)
    if path == "dropin":
        c0.tree_init()
        c1.tree_init()
        for lvl in range(L):
            C, _ = c0.tree_crawl()
            C1, _ = c1.tree_crawl()
            assert C == C1 == o.n_children[lvl]
            assert_states_equal(c0.export_states(), o.states0[lvl], f"level {lvl} server 0")
            assert_states_equal(c1.export_states(), o.states1[lvl], f"level {lvl} server 1")
            assert np.array_equal(sim_eq_count(c0, c1, C), o.counts[lvl])
            c0.tree_prune(o.keeps[lvl])
            c1.tree_prune(o.keeps[lvl])
        return
    host = sim_crawl(c0, c1, 0.0, mode="count", host_loop=True)
    _assert_crawl(ref, c0, c1, host, "host loop")
    if path == "host-loop":
        return
    # every client where the level has few children, else every 7th (7 is coprime to 64: all lanes)
    for levels, clients in (([lv for lv in range(L) if o.n_children[lv] <= 16], np.arange(n)),
                            ([lv for lv in range(L) if o.n_children[lv] > 16],
                             np.arange(n) if n < 1000 else np.union1d(np.arange(0, n, 7), [n - 1]))):
        cap = max(o.n_children[lv] for lv in levels)
        dev = sim_crawl(c0, c1, 0.0, mode="count", init_capacity=128,
                        probe={"levels": levels, "clients": clients.astype(np.uint64), "capacity": cap})
        assert sig(dev) == sig(host)
        _assert_crawl(ref, c0, c1, dev, "device loop")
        assert set(dev.probe) == set(levels)
        for lv, (seeds, t, y) in dev.probe.items():
            for s, st in ((0, o.states0[lv]), (1, o.states1[lv])):
                assert_states_equal((seeds[s], t[s], y[s]), st, f"device loop level {lv} server {s}", clients=clients)
