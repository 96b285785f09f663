"""fhh_retain_clients on the GPU (apply_sketch_results, main.rs:68-69): after the call a collection is exactly the
collection of the survivors. The reference object of every comparison is a fresh pair of collections loaded with
the survivors' exported keys through add_keys and seeded with tree_init_at(frontier_paths()) — never the code
under test against itself; counts are checked against a brute-force recount over the survivors."""
import ctypes
import functools

import numpy as np
import pytest

from retain_cases import children_of, masks, recount

pytestmark = pytest.mark.gpu

FHH_E_ARG, FHH_E_STATE = -1, -2
L16 = 16
PRF = 7


@functools.lru_cache(maxsize=None)
def _workload(n, d, L=L16, seed=0):
    """A seeded Zipf workload of 4 sites cut to L levels (the cut keeps the sites' shared prefixes, so several
    nodes stay heavy per level); read-only."""
    from fuzzyheavyhitters_amd import workload
    wl = workload.zipf_workload(n, max(32, L), d, num_sites=4, seed=300 + 10 * d + seed)
    wl.left, wl.right = wl.left[:, :, :L].copy(), wl.right[:, :, :L].copy()
    for a in (wl.left, wl.right, wl.root_seeds):
        a.setflags(write=False)
    return wl


def _pair(L, d, devices=None):
    import fuzzyheavyhitters_amd as fhh
    return fhh.KeyCollection(L, d, devices=devices), fhh.KeyCollection(L, d, devices=devices)


def _gen_pair(wl, devices=None):
    import fuzzyheavyhitters_amd as fhh
    _, d, L = wl.left.shape
    c0, c1 = _pair(L, d, devices)
    fhh.gen_keys_pair(c0, c1, wl.left, wl.right, wl.root_seeds)
    return c0, c1


def _thr(n):
    return max(1, n // 50)


def _crawl_to(c0, c1, k, thr):
    from fuzzyheavyhitters_amd.collection import sim_eq_count
    c0.tree_init()
    c1.tree_init()
    for _ in range(k):
        C, _ = c0.tree_crawl()
        c1.tree_crawl()
        keep = sim_eq_count(c0, c1, C) >= thr
        assert keep.sum() >= 2, "the threshold keeps several nodes per level"
        c0.tree_prune(keep)
        c1.tree_prune(keep)


def _fresh_pair(keys, kept, paths, L, d, devices=None):
    """The reference object: the survivors' keys (export_keys()[kept] of the pair before the retain) through
    add_keys into a fresh pair, seeded at `paths` (None: not initialised)."""
    f = _pair(L, d, devices)
    for c, k in zip(f, keys):
        c.add_keys(*[np.ascontiguousarray(a[kept]) for a in k])
        if paths is not None:
            c.tree_init_at(paths)
    return f


def _keys_equal(c, sub, what=""):
    for got, want, name in zip(c.export_keys(), sub, ("key_idx", "root_seed", "cw_seed", "cw_bits")):
        assert np.array_equal(got, want), f"{what}: {name}"


def _states_equal(a, b, what=""):
    for x, y, name in zip(a.export_states(), b.export_states(), ("seed", "t", "y")):
        assert x.shape == y.shape and np.array_equal(x, y), f"{what}: {name} differs"


def _lockstep(a, b, left, right, thr):
    """Both pairs crawl from their (equal) frontier to the end: the share planes, counts, last-level sums and final
    shares are equal, and the counts are the recount over the survivors. Returns the per-level counts."""
    import fuzzyheavyhitters_amd as fhh
    from fuzzyheavyhitters_amd.collection import sim_eq_count, sim_ot_sums
    n, d, L = left.shape
    cs = (a[0], a[1], b[0], b[1])
    assert all(c.num_clients() == n for c in cs)
    out = []
    lv = a[0].frontier_paths().shape[2]
    while lv < L:
        last = lv == L - 1
        parents = a[0].frontier_paths()
        assert np.array_equal(parents, b[0].frontier_paths())
        if len(parents) == 0:
            break
        outs = [(c.tree_crawl_last if last else c.tree_crawl)(share_planes=True) for c in cs]
        C = outs[0][0]
        assert [o[0] for o in outs] == [C] * 4 and C == len(parents) << d, f"level {lv}"
        assert outs[0][1].shape == (C, 2 * d, (n + 63) // 64)
        assert np.array_equal(outs[0][1], outs[2][1]) and np.array_equal(outs[1][1], outs[3][1]), f"planes level {lv}"
        ca, cb = sim_eq_count(a[0], a[1], C), sim_eq_count(b[0], b[1], C)
        assert np.array_equal(ca, cb), f"counts level {lv}"
        assert np.array_equal(ca, recount(left, right, children_of(parents, d))), f"recount level {lv}"
        out.append(ca)
        if not last:
            for c in cs:
                c.tree_prune(ca >= thr)
        else:
            sa, sb = sim_ot_sums(a[0], a[1], C, PRF, True), sim_ot_sums(b[0], b[1], C, PRF, True)
            assert sa == sb
            keep = fhh.KeyCollection.keep_values_last(n, thr, *sa)
            assert np.array_equal(keep, ca >= thr)
            for c in cs:
                c.tree_prune_last(keep)
            fa = fhh.KeyCollection.final_values(a[0].final_shares(), a[1].final_shares())
            fb = fhh.KeyCollection.final_values(b[0].final_shares(), b[1].final_shares())
            assert [(r.path, r.value) for r in fa] == [(r.path, r.value) for r in fb]
            assert [r.value for r in fa] == [int(v) for v in ca[keep]]
        lv += 1
    return out


# ---- 1. keys only, before tree_init ------------------------------------------------------------------------

SHAPES1 = [(1, 130), (2, 130), (3, 70)]
MASK_NAMES = ["all ones", "first dropped", "middle dropped", "last dropped", "word dropped", "one survivor", "random"]


def _mask(n, name):
    m = masks(n)
    return m[f"one survivor {n // 2}"] if name == "one survivor" else m[name]


@pytest.mark.parametrize("staged", [False, True], ids=["device", "staged"])
@pytest.mark.parametrize("name", MASK_NAMES)
@pytest.mark.parametrize("d,n", SHAPES1, ids=[f"d{d}-n{n}" for d, n in SHAPES1])
def test_keys_only(d, n, name, staged):
    """Retain before tree_init, on device keys (gen_keys_pair) and on keys staged by add_keys: export_keys is the
    subset, export_keys_bincode the fresh pair's bytes, and the whole crawl equals the fresh pair's and the
    plaintext crawl over the survivors."""
    from fuzzyheavyhitters_amd import workload
    wl = _workload(n, d)
    keep = _mask(n, name)
    kept = np.flatnonzero(keep)
    src = _gen_pair(wl)
    keys = [c.export_keys() for c in src]
    if staged:
        cs = _pair(L16, d)
        for c, k in zip(cs, keys):
            c.add_keys(*k)
    else:
        cs = src
    for c in cs:
        c.retain_clients(keep)
        assert c.num_clients() == len(kept)
    fresh = _fresh_pair(keys, kept, None, L16, d)
    for c, f, k in zip(cs, fresh, keys):
        _keys_equal(c, [a[kept] for a in k], name)
    for c in cs + fresh:
        c.tree_init()
    for c, f in zip(cs, fresh):
        assert np.array_equal(c.export_keys_bincode(), f.export_keys_bincode()), "bincode"
        assert np.array_equal(c.export_keys_bincode(batch=7), f.export_keys_bincode(batch=7)), "bincode batches"
        _states_equal(c, f, "roots")
    left, right = wl.left[kept], wl.right[kept]
    thr = _thr(len(kept))
    counts = _lockstep(cs, fresh, left, right, thr)
    plain, _, _ = workload.plaintext_crawl(left, right, thr, thr)
    assert len(counts) == L16 and all(np.array_equal(x, y) for x, y in zip(counts, plain))


# ---- 2. mid-crawl ------------------------------------------------------------------------------------------

def _survivors(wl, n_keep, seed):
    """A mask over the workload's clients with n_keep survivors, drawn among the heaviest site's clients first
    (so the frontier keeps a heavy node at any survivor count)."""
    n = wl.left.shape[0]
    rng = np.random.default_rng(seed)
    site = np.bincount(wl.site_of_client).argmax()
    order = np.concatenate([rng.permutation(np.flatnonzero(wl.site_of_client == site)),
                            rng.permutation(np.flatnonzero(wl.site_of_client != site))])
    keep = np.zeros(n, np.uint8)
    keep[order[:n_keep]] = 1
    return keep


@pytest.mark.parametrize("n_keep", [128, 65, 64, 1])
@pytest.mark.parametrize("depth", [1, 2, 3, 8])
@pytest.mark.parametrize("d", [1, 2])
def test_mid_crawl(d, depth, n_keep):
    """Retain at a frontier of several nodes (depths 1, 2, 3, 8: both table buffers, entries that are not the
    first of their buffer; d = 2: shared dim-0 prefixes), the survivor count crossing a word boundary both ways:
    export_states is the fresh pair's bit for bit on both servers, then the crawls go on in lockstep."""
    n = 130
    wl = _workload(n, d)
    cs = _gen_pair(wl)
    keys = [c.export_keys() for c in cs]
    _crawl_to(*cs, depth, _thr(n))
    paths = cs[0].frontier_paths()
    assert paths.shape[0] >= 2 and paths.shape[2] == depth
    if d == 2 and depth >= 2:
        from fuzzyheavyhitters_amd import KeyCollection
        nu, _ = KeyCollection.frontier_plan(paths)
        assert (nu > 1).any()
    keep = _survivors(wl, n_keep, 40 + depth)
    kept = np.flatnonzero(keep)
    before = [(c.frontier_size(), c.stats()) for c in cs]
    for c in cs:
        c.retain_clients(keep)
    for c, (size, stats) in zip(cs, before):
        assert c.num_clients() == n_keep and c.frontier_size() == size and c.stats() == stats
        assert np.array_equal(c.frontier_paths(), paths)
    fresh = _fresh_pair(keys, kept, paths, L16, d)
    for s, (c, f, k) in enumerate(zip(cs, fresh, keys)):
        _states_equal(c, f, f"server {s}")
        _keys_equal(c, [a[kept] for a in k], f"server {s}")
    _lockstep(cs, fresh, wl.left[kept], wl.right[kept], _thr(n_keep))


# ---- 3. retain twice ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", [1, 2])
def test_retain_twice(d):
    """Retain at depth 2 and again at depth 5 = one retain with the composed mask = the fresh pair."""
    from fuzzyheavyhitters_amd.collection import sim_eq_count
    n = 130
    wl = _workload(n, d)
    a, b = _gen_pair(wl), _gen_pair(wl)
    keys = [c.export_keys() for c in a]
    k1 = _survivors(wl, 100, 1)
    k2 = np.ones(100, np.uint8)
    k2[np.random.default_rng(2).choice(100, 33, replace=False)] = 0
    composed = np.zeros(n, np.uint8)
    composed[np.flatnonzero(k1)[np.flatnonzero(k2)]] = 1
    kept = np.flatnonzero(composed)
    assert len(kept) == 67
    thr = 2
    _crawl_to(*a, 2, thr)
    _crawl_to(*b, 2, thr)
    for c in a:
        c.retain_clients(k1)
    for _ in range(3):   # depth 2 -> 5 with the same keep decisions on both pairs (the once-retained pair's counts)
        C, _ = a[0].tree_crawl()
        for c in (a[1], b[0], b[1]):
            c.tree_crawl()
        keepn = sim_eq_count(a[0], a[1], C) >= thr
        assert keepn.sum() >= 2
        for c in a + b:
            c.tree_prune(keepn)
    for c in a:
        c.retain_clients(k2)
    for c in b:
        c.retain_clients(composed)
    paths = a[0].frontier_paths()
    assert paths.shape[2] == 5 and np.array_equal(paths, b[0].frontier_paths())
    fresh = _fresh_pair(keys, kept, paths, L16, d)
    for s in range(2):
        _states_equal(a[s], b[s], f"twice vs composed, server {s}")
        _states_equal(a[s], fresh[s], f"twice vs fresh, server {s}")
        _keys_equal(a[s], [x[kept] for x in keys[s]], f"server {s}")
    _lockstep(a, fresh, wl.left[kept], wl.right[kept], thr)


# ---- 4. a shape that makes each gather kernel loop ---------------------------------------------------------

def test_kernels_loop():
    """n = 16 385, L = 64, d = 2, a random 50 % mask. Launch geometry exceeded: a launch has at most 2048 blocks
    of 256 destination columns x 4 rows (column gather) or x 1 row (plane gather), grid.y = min(row groups,
    2048 / column tiles). About 8 190 survivors are 33 column tiles, so grid.y <= 62: cw_seed's 256 rows are 64
    row groups and cw_bits' 1024 rows 1024, both more than 62 — every block of both kernels strides to a second
    row group (cw_bits: 17 of them), and the last column tile is partly padding."""
    from fuzzyheavyhitters_amd import workload
    from fuzzyheavyhitters_amd.collection import sim_eq_count
    n, L, d = 16385, 64, 2
    wl = workload.zipf_workload(n, L, d, num_sites=4, seed=77)
    cs = _gen_pair(wl)
    keys = [c.export_keys() for c in cs]
    keep = (np.random.default_rng(5).random(n) < 0.5).astype(np.uint8)
    kept = np.flatnonzero(keep)
    assert 2048 // ((len(kept) + 255) // 256) < (L * 2 * d) // 4 and len(kept) % 256
    for c, k in zip(cs, keys):
        c.retain_clients(keep)
        _keys_equal(c, [a[kept] for a in k])
        c.tree_init()
    C, _ = cs[0].tree_crawl()
    cs[1].tree_crawl()
    cnt = sim_eq_count(*cs, C)
    assert np.array_equal(cnt, recount(wl.left[kept], wl.right[kept], children_of(np.zeros((1, d, 0), np.uint8), d)))
    assert cnt.sum() >= len(kept)


# ---- 5. device loop ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", [1, 2])
def test_device_loop(d):
    """fhh_sim_crawl (mode 0: counts) on a pair retained mid-crawl: level_children, counts and the final shares are
    the fresh pair's, and the plaintext crawl's over the survivors. The fresh pair's keys are still staged by
    add_keys when its device loop starts: the loop uploads them before it sizes its tables by npad."""
    import fuzzyheavyhitters_amd as fhh
    from fuzzyheavyhitters_amd import workload
    n = 130
    wl = _workload(n, d)
    cs = _gen_pair(wl)
    keys = [c.export_keys() for c in cs]
    _crawl_to(*cs, 3, _thr(n))
    keep = _survivors(wl, 65, 9)
    kept = np.flatnonzero(keep)
    for c in cs:
        c.retain_clients(keep)
    fresh = _fresh_pair(keys, kept, None, L16, d)
    frac = 0.05
    ra = fhh.sim_crawl(*cs, frac, mode="count")
    rb = fhh.sim_crawl(*fresh, frac, mode="count")
    assert list(ra.level_children) == list(rb.level_children)
    assert len(ra.counts) == L16 and all(np.array_equal(x, y) for x, y in zip(ra.counts, rb.counts))
    assert [(r.path, r.value) for r in ra.final] == [(r.path, r.value) for r in rb.final] and len(ra.final) > 0
    thr = max(1, int(frac * len(kept)))
    plain, _, _ = workload.plaintext_crawl(wl.left[kept], wl.right[kept], thr, thr)
    assert all(np.array_equal(x, y) for x, y in zip(ra.counts, plain))


# ---- 6. two-party protocol ---------------------------------------------------------------------------------

@pytest.mark.parametrize("d,form", [(1, 0), (2, 1)], ids=["d1-table", "d2-circuit"])
def test_two_party_after_retain(d, form):
    """After a mid-crawl retain, one FE level and the FieldElm level through party.run_chunk / party_sums
    (material "test"): v0 - v1 is the recount over the survivors, and every message has the size the fresh pair
    of n' clients sends. The retained pair ran the level before the retain through the protocol too, so its
    party state (sized for 130 clients) is the one that survives."""
    from fuzzyheavyhitters_amd import party
    from fuzzyheavyhitters_amd.collection import sim_eq_count
    from fuzzyheavyhitters_amd.fields import FE255_P, FE_P
    n, n_keep, depth = 130, 65, 3
    wl = _workload(n, d)
    cs = _gen_pair(wl)
    keys = [c.export_keys() for c in cs]
    _crawl_to(*cs, depth - 1, _thr(n))
    keep = _survivors(wl, n_keep, 11)
    kept = np.flatnonzero(keep)
    left, right = wl.left[kept], wl.right[kept]
    thr = _thr(n_keep)

    def protocol(pair, lv, last):
        parents = pair[0].frontier_paths()
        C, _ = (pair[0].tree_crawl_last if last else pair[0].tree_crawl)()
        (pair[1].tree_crawl_last if last else pair[1].tree_crawl)()
        gb, ev = party.test_cfgs(PRF, lv)
        gb.form = ev.form = form
        sizes = party.run_chunk(pair[0], pair[1], gb, ev, party.Channel(0, "copy"), party.Channel(0, "copy"))
        s0, s1 = party.party_sums(pair[0], C, last), party.party_sums(pair[1], C, last)
        if last:
            v = np.array([((x % FE255_P) - (y % FE255_P)) % FE255_P for x, y in zip(s0, s1)], np.uint64)
        else:
            v = ((s0.astype(object) - s1.astype(object)) % FE_P).astype(np.uint64)
        return sizes, v, children_of(parents, d)

    _, v, ch = protocol(cs, depth - 1, False)
    assert np.array_equal(v, recount(wl.left, wl.right, ch)) and (v >= _thr(n)).sum() >= 2
    for c in cs:
        c.tree_prune(v >= _thr(n))
    for c in cs:
        c.retain_clients(keep)
    fresh = _fresh_pair(keys, kept, cs[0].frontier_paths(), L16, d)
    for lv in range(depth, L16):
        last = lv == L16 - 1
        if lv == depth or last:
            (sa, va, ch), (sb, vb, _) = protocol(cs, lv, last), protocol(fresh, lv, last)
            assert np.array_equal(va, recount(left, right, ch)), f"level {lv}: v0 - v1 vs the recount"
            assert np.array_equal(va, vb), f"level {lv}"
            assert sa == sb and sa["gc"] > 0, f"level {lv}: message sizes {sa} vs {sb}"
            cnt = va
        else:
            C, _ = cs[0].tree_crawl()
            for c in (cs[1],) + fresh:
                c.tree_crawl()
            cnt = sim_eq_count(*cs, C)
        if not last:
            assert (cnt >= thr).any()
            for c in cs + fresh:
                c.tree_prune(cnt >= thr)


# ---- 7. multi-device ---------------------------------------------------------------------------------------

N7 = 200   # 4 words: 2 shards of 128 + 72 clients, 4 shards of 64 + 64 + 64 + 8


def _mask7(name, S):
    keep = np.ones(N7, np.uint8)
    if name == "ragged":           # shard 0 loses 3 clients: every later base is off a word boundary
        keep[[1, 17, 40]] = 0
    elif name == "empty-shard":    # shard 1 loses everybody, the others nobody
        b = 128 if S == 2 else 64
        keep[b:(N7 if S == 2 else 128)] = 0
    elif name == "aligned":        # a whole word leaves shard 0: bases stay whole words
        keep[:64] = 0
    elif name == "mixed":          # ragged, a shard untouched (the last), and random drops elsewhere
        keep[np.random.default_rng(3).choice(120, 37, replace=False)] = 0
    return keep


@pytest.mark.parametrize("name", ["ragged", "empty-shard", "aligned", "mixed"])
@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0, 0]], ids=["2-shards", "4-shards"])
@pytest.mark.parametrize("d", [1, 2])
def test_multi_device(d, devices, name):
    """Each shard retains its slice: shard_info reports the prefix ranges, and export_keys, the tree_crawl share
    planes (merged by shifts where a base is off a word boundary), node_sums_fe and the shards' sim_ot_sums equal
    those of a one-GPU collection of the survivors."""
    import fuzzyheavyhitters_amd as fhh
    from fuzzyheavyhitters_amd.collection import sim_eq_count, sim_ot_sums
    from fuzzyheavyhitters_amd.fields import FE_P
    S = len(devices)
    wl = _workload(N7, d)
    keep = _mask7(name, S)
    kept = np.flatnonzero(keep)
    one = _gen_pair(wl)
    keys = [c.export_keys() for c in one]
    g = _gen_pair(wl, devices)
    plan = fhh.shard_plan(N7, S)
    depth = 2
    for c in one + g:
        c.tree_init()
    for _ in range(depth):
        C, _ = one[0].tree_crawl()
        for c in (one[1],) + g:
            c.tree_crawl()
        k = sim_eq_count(*one, C) >= 2
        for c in one + g:
            c.tree_prune(k)
    paths = one[0].frontier_paths()
    for c in g:
        c.retain_clients(keep)
    single = _fresh_pair(keys, kept, paths, L16, d)
    counts = [int(keep[b:b + c].sum()) for b, c in plan]
    bases = [int(x) for x in np.concatenate([[0], np.cumsum(counts)[:-1]])]
    for c in g:
        info, _ = c.shard_info()
        assert [(b, m) for _, b, m in info] == list(zip(bases, counts)), name
        assert c.num_clients() == len(kept)
    if name in ("ragged", "mixed"):
        assert any(b % 64 for b, m in zip(bases, counts) if m)
    if name == "empty-shard":
        assert counts[1] == 0 and all(m == pm for k, (m, (_, pm)) in enumerate(zip(counts, plan)) if k != 1)
    if name == "aligned":
        assert all(b % 64 == 0 for b in bases)
    if name == "mixed":
        assert counts[-1] == plan[-1][1]
    for s in range(2):
        _keys_equal(g[s], [a[kept] for a in keys[s]], f"server {s}")
        assert np.array_equal(g[s].export_keys_bincode(batch=50), single[s].export_keys_bincode(batch=50))
        _states_equal(g[s], single[s], f"server {s}")
    left, right = wl.left[kept], wl.right[kept]
    rng = np.random.default_rng(8)
    for lv in range(depth, depth + 3):
        parents = single[0].frontier_paths()
        outs = [c.tree_crawl(share_planes=True) for c in single + g]
        C = outs[0][0]
        assert [o[0] for o in outs] == [C] * 4
        assert np.array_equal(outs[0][1], outs[2][1]) and np.array_equal(outs[1][1], outs[3][1]), f"planes level {lv}"
        vals = rng.integers(0, 1 << 63, (C, len(kept)), dtype=np.uint64)
        assert np.array_equal(single[0].node_sums_fe(vals), g[0].node_sums_fe(vals)), f"FE sums level {lv}"
        want = sim_ot_sums(*single, C, PRF, False)
        got = [[0] * C, [0] * C]
        for k, m in enumerate(counts):
            if m:
                part = sim_ot_sums(g[0].shard(k), g[1].shard(k), C, PRF, False)
                got = [[(x + y) % FE_P for x, y in zip(a, b)] for a, b in zip(got, part)]
        assert [[x % FE_P for x in w] for w in want] == got, f"sim_ot_sums level {lv}"
        cnt = sim_eq_count(*single, C)
        assert np.array_equal(cnt, recount(left, right, children_of(parents, d)))
        for c in single + g:
            c.tree_prune(cnt >= 2)


def test_multi_device_staged_keys():
    """Keys staged on a multi-device ctx by add_keys (not yet cut into the shards): the host vectors are compacted."""
    wl = _workload(N7, 1)
    one = _gen_pair(wl)
    keys = one[0].export_keys()
    g, _ = _pair(L16, 1, [0, 0])
    g.add_keys(*keys)
    keep = _mask7("mixed", 2)
    kept = np.flatnonzero(keep)
    g.retain_clients(keep)
    assert g.num_clients() == len(kept)
    g.tree_init()
    _keys_equal(g, [a[kept] for a in keys])
    import fuzzyheavyhitters_amd as fhh
    assert [(b, m) for _, b, m in g.shard_info()[0]] == fhh.shard_plan(len(kept), 2)   # cut after the retain


# ---- 8. refusals -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("devices", [None, [0, 0]], ids=["one-gpu", "2-shards"])
def test_refusals_leave_the_ctx_as_it_was(devices):
    from fuzzyheavyhitters_amd._lib import lib, ptr
    from fuzzyheavyhitters_amd.collection import sim_eq_count
    n, d = 130, 1
    wl = _workload(n, d)
    Lb = lib()

    def call(c, keep, n_arg=None):
        k = np.ascontiguousarray(keep, np.uint8)
        rc = Lb.fhh_retain_clients(c.handle, ptr(k), k.size if n_arg is None else n_arg)
        return rc, (Lb.fhh_last_error(c.handle) or b"").decode()

    good = np.ones(n, np.uint8)
    good[5] = 0
    # before any keys
    e0, _ = _pair(L16, d, devices)
    rc, msg = call(e0, good)
    assert rc == FHH_E_STATE and "no keys" in msg
    assert e0.num_clients() == 0
    # appended batches not yet finished by tree_init
    src, _ = _gen_pair(wl)
    a0, _ = _pair(L16, d, devices)
    if devices:
        a0.reserve_clients(n)
    a0.add_keys_bincode_append(src.export_keys_bincode())
    rc, msg = call(a0, good)
    assert rc == FHH_E_STATE and "appended" in msg, msg
    assert a0.num_clients() == n
    a0.tree_init()
    _keys_equal(a0, src.export_keys(), "appended keys after the refusal")
    # the frontier phase: argument refusals, then pending children
    cs = _gen_pair(wl, devices)
    ref = _gen_pair(wl)
    for c in cs + ref:
        c.tree_init()
    for _ in range(2):   # the one-GPU pair's counts decide for both (sim_eq_count is a per-shard entry)
        C, _ = ref[0].tree_crawl()
        for c in (ref[1],) + cs:
            c.tree_crawl()
        k = sim_eq_count(*ref, C) >= 2
        for c in cs + ref:
            c.tree_prune(k)
    states = cs[0].export_states()
    bad = good.copy()
    bad[7] = 2
    for what, (rc, msg) in {"wrong n": call(cs[0], good[:-1]), "n = 0": call(cs[0], good, 0), "a byte 2": call(cs[0], bad),
                            "all zeros": call(cs[0], np.zeros(n, np.uint8))}.items():
        assert rc == FHH_E_ARG and msg.startswith("retain_clients: "), (what, rc, msg)
    assert Lb.fhh_retain_clients(cs[0].handle, None, n) == FHH_E_ARG
    assert Lb.fhh_retain_clients(None, ptr(good), n) == FHH_E_ARG
    assert cs[0].num_clients() == n and cs[0].frontier_size() == ref[0].frontier_size()
    for x, y in zip(states, cs[0].export_states()):
        assert np.array_equal(x, y)
    C, _ = cs[0].tree_crawl()
    cs[1].tree_crawl()
    for c in ref:
        c.tree_crawl()
    pend = cs[0].export_states()
    rc, msg = call(cs[0], good)
    assert rc == FHH_E_STATE and "pending" in msg
    assert cs[0].num_clients() == n and cs[0].frontier_size() == (C, 0)
    for x, y in zip(pend, cs[0].export_states()):
        assert np.array_equal(x, y)
    if devices is None:
        assert np.array_equal(sim_eq_count(*cs, C), sim_eq_count(*ref, C))
    # and the crawl goes on: the next level's counts are those of the untouched pair
    keep = sim_eq_count(*ref, C) >= 2
    for c in cs + ref:
        c.tree_prune(keep)
    (C2, p0), (_, p1) = [c.tree_crawl(share_planes=True) for c in cs]
    (R2, r0), (_, r1) = [c.tree_crawl(share_planes=True) for c in ref]
    assert C2 == R2 and np.array_equal(p0, r0) and np.array_equal(p1, r1)
    # a mask of all ones is accepted in the frontier phase and changes nothing
    for c in cs + ref:
        c.tree_prune(np.ones(C2, bool))
    cs[0].retain_clients(np.ones(n, np.uint8))
    _states_equal(cs[0], ref[0], "all ones")


# ---- 8b. a collection loaded by appended batches, after tree_init ------------------------------------------

@pytest.mark.parametrize("devices", [None, [0, 0]], ids=["one-gpu", "2-shards"])
def test_appended_collection_retains_after_init(devices):
    """The leader's batches (add_keys_bincode_append) leave the ctx marked as appended for good; only the capacity
    layout before tree_init is refused. After tree_init, a crawl and a prune the retain goes through (reservation
    above the count on one GPU, so tree_init had a capacity stride to finish) and equals the fresh pair."""
    from fuzzyheavyhitters_amd import workload
    from fuzzyheavyhitters_amd.collection import sim_eq_count
    n, d = 130, 1
    wl = _workload(n, d)
    src = _gen_pair(wl)
    keys = [c.export_keys() for c in src]
    cs = _pair(L16, d, devices)
    for c, s in zip(cs, src):
        c.reserve_clients(n if devices else 300)
        for req in workload.split_add_keys_requests(s.export_keys_bincode(batch=50), d, L16):
            c.add_keys_bincode_append(req)
    for c in cs + src:
        c.tree_init()
    for _ in range(2):
        C, _ = src[0].tree_crawl()
        for c in (src[1],) + cs:
            c.tree_crawl()
        k = sim_eq_count(*src, C) >= 2
        for c in cs + src:
            c.tree_prune(k)
    keep = _survivors(wl, 65, 21)
    kept = np.flatnonzero(keep)
    for c in cs:
        c.retain_clients(keep)
        assert c.num_clients() == 65
    fresh = _fresh_pair(keys, kept, src[0].frontier_paths(), L16, d)
    for s in range(2):
        _states_equal(cs[s], fresh[s], f"server {s}")
        _keys_equal(cs[s], [a[kept] for a in keys[s]], f"server {s}")
    left, right = wl.left[kept], wl.right[kept]
    if devices is None:
        _lockstep(cs, fresh, left, right, 2)
    else:   # sim_eq_count is a per-shard entry: the planes and the one-GPU pair's counts
        for lv in range(2, 5):
            parents = fresh[0].frontier_paths()
            outs = [c.tree_crawl(share_planes=True) for c in fresh + cs]
            C = outs[0][0]
            assert [o[0] for o in outs] == [C] * 4
            assert np.array_equal(outs[0][1], outs[2][1]) and np.array_equal(outs[1][1], outs[3][1]), f"level {lv}"
            cnt = sim_eq_count(*fresh, C)
            assert np.array_equal(cnt, recount(left, right, children_of(parents, d)))
            for c in fresh + cs:
                c.tree_prune(cnt >= 2)


# ---- 9. sketch.apply_sketch_results ------------------------------------------------------------------------

def test_apply_sketch_results():
    """sim_sketch_verify's ok bits drive the retain: the survivors are exactly the honest keys and the next level's
    counts are the recount over them."""
    from fuzzyheavyhitters_amd import sketch as S
    from fuzzyheavyhitters_amd.collection import sim_eq_count
    n, d = 130, 1
    swl = S.sketch_workload(n_keys=n, n_nodes=4, bad_fraction=0.05)
    assert 0 < swl.honest.sum() < n, "the workload drops somebody and keeps somebody"
    wl = _workload(n, d)
    cs = _gen_pair(wl)
    keys = [c.export_keys() for c in cs]
    _crawl_to(*cs, 2, 2)
    b = S.DeviceSketchBatch(swl)
    S.sim_sketch_verify(cs[0], b)
    kept = np.flatnonzero(swl.honest)
    assert S.apply_sketch_results(cs[0], cs[1], b.ok[0]) == len(kept)
    for c, k in zip(cs, keys):
        assert c.num_clients() == len(kept)
        _keys_equal(c, [a[kept] for a in k])
    parents = cs[0].frontier_paths()
    C, _ = cs[0].tree_crawl()
    cs[1].tree_crawl()
    assert np.array_equal(sim_eq_count(*cs, C), recount(wl.left[kept], wl.right[kept], children_of(parents, d)))
