"""fhh_join_clients_bincode on the GPU: clients that join a crawl in progress. The reference object of every
comparison is a fresh pair that was never joined: the oracle's keys (oracle.gen_keys on oracle.l_inf_ball_bounds,
join_cases.py) of all n + m clients through add_keys, seeded with tree_init_at(frontier_paths()) of the pair
under test. Every count is also retain_cases.recount over all n + m clients."""
import numpy as np
import pytest

import ball_cases as bc
import join_cases as jc
from retain_cases import children_of, recount

pytestmark = pytest.mark.gpu

L = jc.L
PRF = 7
DELTA = 1


def _pair(d, devices=None):
    import fuzzyheavyhitters_amd as fhh
    return fhh.KeyCollection(L, d, devices=devices), fhh.KeyCollection(L, d, devices=devices)


def _thr(n):
    return 1 if n < 64 else 2


def _load(K, lo, hi, origin="add_keys", devices=None):
    """A pair holding the clients [lo, hi) of population K, their keys brought in by `origin`."""
    import fuzzyheavyhitters_amd as fhh
    from fuzzyheavyhitters_amd import workload
    cs = _pair(K.d, devices)
    if origin == "add_keys":
        for s, c in enumerate(cs):
            c.add_keys(*K.arrays(s, lo, hi))
    elif origin == "append":
        mid = lo + (hi - lo + 1) // 2
        for s, c in enumerate(cs):
            if devices:
                c.reserve_clients(hi - lo)
            c.add_keys_bincode_append(K.request(s, lo, mid))
            if mid < hi:
                c.add_keys_bincode_append(K.request(s, mid, hi))
    elif origin == "ball":
        fhh.gen_keys_ball(*cs, workload.pack_points(K.alpha[lo:hi]), K.delta, root_seeds=np.ascontiguousarray(K.roots[lo:hi]))
    else:
        raise AssertionError(origin)
    return cs


def _eq_count(c0, c1, C):
    """sim_eq_count of a pair; a multi-device pair's is the sum over its pairs of shards (a per-shard harness entry)"""
    from fuzzyheavyhitters_amd.collection import sim_eq_count
    info, _ = c0.shard_info()
    if len(info) <= 1:
        return sim_eq_count(c0, c1, C)
    tot = np.zeros(C, np.uint64)
    for k, (_, _, cnt) in enumerate(info):
        if cnt:
            tot += sim_eq_count(c0.shard(k), c1.shard(k), C)
    return tot


def _crawl_to(cs, depth, thr):
    for c in cs:
        c.tree_init()
    for _ in range(depth):
        C, _ = cs[0].tree_crawl()
        cs[1].tree_crawl()
        keep = _eq_count(*cs, C) >= thr
        assert keep.any()
        for c in cs:
            c.tree_prune(keep)


def _reference(K, clients, paths):
    """The fresh pair: the oracle's keys of `clients` (indices into K) through add_keys, at `paths`."""
    ref = _pair(K.d)
    for s, c in enumerate(ref):
        c.add_keys(*[np.ascontiguousarray(K.k[s][f][clients]) for f in jc.FIELDS])
        c.tree_init_at(paths)
    return ref


def _join(cs, K, lo, hi):
    for s, c in enumerate(cs):
        c.join_clients_bincode(K.request(s, lo, hi))


def _assert_equal(cs, ref, K, clients, paths, what=""):
    """The core equality on both servers, bit for bit."""
    for s, (c, r) in enumerate(zip(cs, ref)):
        w = f"{what} server {s}"
        assert c.num_clients() == r.num_clients() == len(clients), w
        for got, f in zip(c.export_keys(), jc.FIELDS):
            assert np.array_equal(got, K.k[s][f][clients]), f"{w}: export_keys {f}"
        assert np.array_equal(c.export_keys_bincode(), r.export_keys_bincode()), f"{w}: bincode"
        assert np.array_equal(c.export_keys_bincode(batch=7), r.export_keys_bincode(batch=7)), f"{w}: bincode batches"
        assert np.array_equal(c.frontier_paths(), paths) and np.array_equal(r.frontier_paths(), paths), f"{w}: paths"
        for x, y, name in zip(c.export_states(), r.export_states(), ("seed", "t", "y")):
            assert x.shape == y.shape and np.array_equal(x, y), f"{w}: export_states {name}"


def _lockstep(a, b, left, right, thr):
    """Both pairs crawl from their (equal) frontier to the final shares: planes, counts, last-level sums and final
    shares are equal, and every count is the recount over all the clients."""
    import fuzzyheavyhitters_amd as fhh
    from fuzzyheavyhitters_amd.collection import sim_eq_count, sim_ot_sums
    n, d, _ = left.shape
    cs = (a[0], a[1], b[0], b[1])
    sharded = len(a[0].shard_info()[0]) > 1
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
        ca, cb = _eq_count(a[0], a[1], C), sim_eq_count(b[0], b[1], C)
        assert np.array_equal(ca, cb), f"counts level {lv}"
        assert np.array_equal(ca, jc.recount_chunked(recount, left, right, children_of(parents, d))), f"recount level {lv}"
        if not last:
            for c in cs:
                c.tree_prune(ca >= thr)
        elif sharded:   # (sim_ot_sums is a per-shard harness entry: a multi-device pair stops at the last counts)
            for c in cs:
                c.tree_prune_last(ca >= thr)
            assert np.array_equal(a[0].frontier_paths(), b[0].frontier_paths())
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
    assert lv == L or len(parents) == 0


def _joined_vs_reference(K, n, m, depth, origin="add_keys", devices=None, grid=None, pieces=1):
    """n clients crawled to `depth`, m joined (in `pieces` requests), compared with the reference and crawled on."""
    from fuzzyheavyhitters_amd import KeyCollection
    cs = _load(K, 0, n, origin, devices)
    if grid:
        for c in cs:
            c.set_expand_grid(grid)
    _crawl_to(cs, depth, _thr(n))
    paths = cs[0].frontier_paths()
    assert paths.shape[2] == depth and paths.shape[0] >= 1
    nu, _ = KeyCollection.frontier_plan(paths) if depth else (np.ones(K.d, np.uint32), None)
    before = [(c.frontier_size(), c.stats()["aes_blocks"]) for c in cs]
    cuts = [n + (m * i) // pieces for i in range(pieces + 1)]
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        _join(cs, K, lo, hi)
    for c, (size, blocks) in zip(cs, before):
        assert c.frontier_size() == size
        if devices is None:
            assert c.stats()["aes_blocks"] - blocks == depth * 2 * int(nu.sum()) * m, "stats.aes_blocks"
    clients = np.arange(n + m)
    ref = _reference(K, clients, paths)
    _assert_equal(cs, ref, K, clients, paths, f"n {n} m {m} depth {depth} {origin}")
    _lockstep(cs, ref, K.left[:n + m], K.right[:n + m], _thr(n + m))
    return cs


# ---- 1. core equality --------------------------------------------------------------------------------------
# every (n, m) pair at depths 0 (right after tree_init), 1, 3 and 8 (both table parities, entries that are not the
# first of their buffer after a prune, shared dim-0 prefixes at d = 2), d rotating over 1, 2, 3 so that every pair
# and every depth meets every d; depths 31, 32, 33 (the 32-bit packing of the directions) on three pairs, a shared
# first word in each
CORE = [(1 + (i + k) % 3, n, m, depth) for i, (n, m) in enumerate(jc.PAIRS) for k, depth in enumerate((0, 1, 3, 8))]
CORE += [(1 + (i + k) % 3, n, m, depth) for i, (n, m) in enumerate([(65, 63), (70, 130), (130, 1)]) for k, depth in enumerate((31, 32, 33))]
assert {(d, dep) for d, _, _, dep in CORE} >= {(d, dep) for d in (1, 2, 3) for dep in (0, 1, 3, 8, 31, 32, 33)}
assert {(n, m, dep) for _, n, m, dep in CORE} >= {(n, m, dep) for n, m in jc.PAIRS for dep in (0, 1, 3, 8)}


@pytest.mark.parametrize("d,n,m,depth", CORE, ids=[f"d{d}-{n}+{m}-depth{dep}" for d, n, m, dep in CORE])
def test_core_equality(d, n, m, depth):
    _joined_vs_reference(jc.keyed(d), n, m, depth)


def test_shared_prefixes_and_late_entries():
    """What depths 3 and 8 are there for, asserted on the frontier the d = 2 population reaches: several nodes, fewer
    distinct dim prefixes than nodes."""
    from fuzzyheavyhitters_amd import KeyCollection
    K = jc.keyed(2)
    cs = _load(K, 0, 70)
    _crawl_to(cs, 8, 2)
    paths = cs[0].frontier_paths()
    nu, _ = KeyCollection.frontier_plan(paths)
    assert paths.shape[0] >= 2 and (nu < paths.shape[0]).any() and (nu > 1).any()


# ---- 2. key origins ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("devices", [None, [0, 0]], ids=["one-gpu", "2-shards"])
@pytest.mark.parametrize("origin", ["ball", "add_keys", "append"])
def test_key_origins(origin, devices):
    _joined_vs_reference(jc.keyed(2), 70, 130, 3, origin=origin, devices=devices)


# ---- 3. compositions ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", [1, 2])
def test_two_joins_equal_one(d):
    """Two joins (65 + 30, then + 33: a word filled exactly, then left partial) against the never-joined reference of
    all the clients, which is what one join of the concatenated request gives (test_core_equality)."""
    _joined_vs_reference(jc.keyed(d), 65, 63, 3, pieces=2)
    _joined_vs_reference(jc.keyed(d), 70, 130, 8, pieces=3)


@pytest.mark.parametrize("n,m", [(70, 130), (70, 20)], ids=["grown", "in-place"])
def test_join_then_retain_the_joiners(n, m):
    K = jc.keyed(2)
    cs = _load(K, 0, n)
    _crawl_to(cs, 3, 2)
    paths = cs[0].frontier_paths()
    _join(cs, K, n, n + m)
    keep = np.zeros(n + m, np.uint8)
    keep[:n] = 1
    for c in cs:
        c.retain_clients(keep)
    clients = np.arange(n)
    twin = _reference(K, clients, paths)
    _assert_equal(cs, twin, K, clients, paths, "joiners retained away")
    _lockstep(cs, twin, K.left[:n], K.right[:n], 2)


def test_retain_then_join():
    K = jc.keyed(2)
    n, m = 130, 70
    cs = _load(K, 0, n)
    _crawl_to(cs, 3, 2)
    paths = cs[0].frontier_paths()
    keep = (np.random.default_rng(4).random(n) < 0.6).astype(np.uint8)
    keep[0] = 1
    for c in cs:
        c.retain_clients(keep)
    _join(cs, K, n, n + m)
    clients = np.concatenate([np.flatnonzero(keep), np.arange(n, n + m)])
    ref = _reference(K, clients, paths)
    _assert_equal(cs, ref, K, clients, paths, "retain then join")
    _lockstep(cs, ref, K.left[clients], K.right[clients], 2)


# ---- 4. a leader's late batch ------------------------------------------------------------------------------

def test_leaders_late_batch(oracle):
    """The joiners' request comes from leader_requests_ball at seed_first = n: the joined pair's keys are
    gen_keys_ball's of the whole population (the oracle's keys with the derived root seeds), and the audit of all
    n + m points against them finds nothing."""
    import fuzzyheavyhitters_amd as fhh
    from fuzzyheavyhitters_amd import workload
    d, n, m = 2, 70, 60
    K = jc.Keyed(oracle, d, n + m, DELTA, 901, roots=lambda k: bc.derived_roots(oracle, bc.SEED, 0, k.n, k.d))
    pts = workload.pack_points(K.alpha)
    cs = _pair(d)
    fhh.gen_keys_ball(*cs, pts[:n], DELTA, seed=bc.SEED, seed_first=0)
    _crawl_to(cs, 3, 2)
    paths = cs[0].frontier_paths()
    r0, r1 = fhh.leader_requests_ball(cs[0], pts[n:], DELTA, seed=bc.SEED, seed_first=n)
    cs[0].join_clients_bincode(r0)
    cs[1].join_clients_bincode(r1)
    clients = np.arange(n + m)
    ref = _reference(K, clients, paths)
    _assert_equal(cs, ref, K, clients, paths, "late batch")
    ok, rep = cs[0].audit_keys_ball(cs[1], pts, DELTA)
    assert ok.shape == (n + m,) and ok.all() and rep["n_bad_clients"] == 0 and rep["first_client"] is None
    _lockstep(cs, ref, K.left, K.right, 2)


# ---- 5. grid trips -----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def big(oracle):
    return jc.Keyed(oracle, 2, 70 + 2100, DELTA, 77)


@pytest.mark.parametrize("grid", [1, 2, 3])
def test_grid_trips(big, grid):
    """n = 70, m = 2 100, d = 2, depth 3 on 1, 2 and 3 workgroups: the walk's grid-stride loop takes several trips
    and its last one is partial (asserted on fhh_join_plan first)."""
    from fuzzyheavyhitters_amd import KeyCollection
    n, m, depth = 70, 2100, 3
    probe = _load(big, 0, n)
    _crawl_to(probe, depth, _thr(n))
    nu, _ = KeyCollection.frontier_plan(probe[0].frontier_paths())
    p = KeyCollection.join_plan(2, depth, n, m, nu, grid)
    assert p == jc.plan(2, depth, n, m, [int(u) for u in nu], grid)
    assert p["trips"] >= 2 and 0 < p["last_trip_items"] < p["waves"], p
    _joined_vs_reference(big, n, m, depth, grid=grid)


# ---- 6. protocol -------------------------------------------------------------------------------------------

def _plain_levels(K, n, m, join_at, levels, thr):
    """Per-level counts and frontiers of the crawl the leader runs: n clients before level `join_at`, n + m from there."""
    d = K.d
    parents = np.zeros((1, d, 0), np.uint8)
    counts, fronts = [], []
    for lv in range(levels):
        k = n if lv < join_at else n + m
        fronts.append(parents)
        ch = children_of(parents, d)
        cnt = jc.recount_chunked(recount, K.left[:k], K.right[:k], ch)
        counts.append(cnt)
        parents = ch[cnt >= thr]
    return counts, fronts


@pytest.mark.parametrize("d,form", [(1, "table"), (2, "circuit")], ids=["d1-table", "d2-circuit"])
def test_two_party_crawl_with_a_join(d, form):
    """two_party_crawl(joins={3: ...}): every level's v0 - v1 is the plaintext count (n clients before level 3,
    n + m from there on), and from level 3 on every message has the size a never-joined pair of n + m clients
    sends from the same frontier. The party states were made for n clients: they are older than the join."""
    from fuzzyheavyhitters_amd import party
    K = jc.keyed(d)
    n, m, levels, frac = 70, 130, 6, 0.01
    thr = max(1, int(frac * (n + m)))
    counts, fronts = _plain_levels(K, n, m, 3, levels, thr)
    cs = _load(K, 0, n)
    res = party.two_party_crawl(*cs, frac, nclients_total=n + m, material="test", prf_seed=PRF, levels=levels, form=form,
                                expect_counts=counts, joins={3: (K.request(0, n, n + m), K.request(1, n, n + m))})
    assert len(res.counts) == levels and all(np.array_equal(x, y) for x, y in zip(res.counts, counts))
    assert all(c.num_clients() == n + m for c in cs)
    ref = _load(K, 0, n + m)
    rres = party.two_party_crawl(*ref, frac, nclients_total=n + m, material="test", prf_seed=PRF, levels=levels, form=form,
                                 expect_counts=counts, start_paths=fronts[3])
    assert list(res.level_children[3:]) == list(rres.level_children)
    assert res.level_bytes[3:] == rres.level_bytes and all(b["gc"] > 0 for b in rres.level_bytes)
    assert [(r.path, r.value) for r in res.final] == [(r.path, r.value) for r in rres.final]


@pytest.mark.parametrize("d", [1, 2])
def test_sim_crawl_on_a_joined_pair(d):
    import fuzzyheavyhitters_amd as fhh
    from fuzzyheavyhitters_amd import workload
    K = jc.keyed(d)
    n, m, frac = 70, 130, 0.02
    cs = _load(K, 0, n)
    _crawl_to(cs, 3, 2)
    _join(cs, K, n, n + m)
    res = fhh.sim_crawl(*cs, frac, mode="count")
    thr = max(1, int(frac * (n + m)))
    plain, fpaths, fcounts = workload.plaintext_crawl(K.left[:n + m], K.right[:n + m], thr, thr)
    assert len(res.counts) == L and all(np.array_equal(x, y) for x, y in zip(res.counts, plain))
    assert sorted(tuple(tuple(p) for p in r.path) for r in res.final) == sorted(fpaths) and len(fpaths) > 0


# ---- 7. shards ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0]], ids=["2-shards", "3-shards"])
def test_shards_equal_one_gpu(devices):
    import fuzzyheavyhitters_amd as fhh
    K = jc.keyed(2)
    n, m = 130, 70
    plan = fhh.shard_plan(n, len(devices))
    cs = _joined_vs_reference(K, n, m, 3, devices=devices)
    for c in cs:
        info, _ = c.shard_info()
        got = [(b, k) for _, b, k in info]
        assert got[:-1] == plan[:-1] and got[-1] == (plan[-1][0], plan[-1][1] + m), "the last shard has grown"


@pytest.mark.parametrize("case", ["emptied-last-shard", "ragged-base"])
def test_shards_after_a_retain(case):
    """A join onto a last shard that a retain emptied (it loads the batch as its only keys and walks to the group's
    frontier), and one whose last shard starts off a word boundary after a retain on the first shard."""
    K = jc.keyed(2)
    n, m, S = 130, 70, 2            # shards of 64 + 66 clients
    cs = _load(K, 0, n, devices=[0] * S)
    _crawl_to(cs, 3, 2)
    paths = cs[0].frontier_paths()
    keep = np.ones(n, np.uint8)
    if case == "emptied-last-shard":
        keep[64:] = 0
    else:
        keep[[1, 17, 40]] = 0
    for c in cs:
        c.retain_clients(keep)
    _join(cs, K, n, n + m)
    kept = np.flatnonzero(keep)
    for c in cs:
        info, _ = c.shard_info()
        first = int(keep[:64].sum())
        assert [(b, k) for _, b, k in info] == [(0, first), (first, len(kept) - first + m)]
        assert (first % 64 != 0) == (case == "ragged-base")
    clients = np.concatenate([kept, np.arange(n, n + m)])
    ref = _reference(K, clients, paths)
    _assert_equal(cs, ref, K, clients, paths, case)
    _lockstep(cs, ref, K.left[clients], K.right[clients], 2)


# ---- 8. refusals -------------------------------------------------------------------------------------------

def _snapshot(c, states=True):
    out = [c.num_clients(), *c.export_keys()]
    if states:
        out += [c.frontier_paths(), *c.export_states(), c.frontier_size()]
    return out


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def _malformed(K, n, m):
    """name -> (server 0's request, message) of the joiners [n, n + m), one field broken"""
    R = jc.record_bytes(K.d)
    good = K.request(0, n, n + m)
    out = {}
    for name, off, val, msg in (("bool-first", 8 + 8, 2, "bool byte > 1"),
                                ("bool-last", 8 + (m - 1) * R + 8 + (25 + 20 * L), 2, "bool byte > 1"),
                                ("cor-words", 8 + (m // 2) * R + 8 + 17, (L + 1) & 0xFF, "cor_words length"),
                                ("dims", 8 + (m - 1) * R, K.d + 1, "dims per client")):
        b = good.copy()
        assert b[off] != val
        b[off] = val
        out[name] = (b, msg)
    return out


@pytest.mark.parametrize("devices,m", [(None, 20), (None, 70), ([0, 0], 70)], ids=["in-place", "growing", "2-shards"])
def test_malformed_requests_leave_the_ctx_as_it_was(devices, m):
    import fuzzyheavyhitters_amd as fhh
    K = jc.keyed(2)
    n = 70
    assert ((n + m + 63) // 64 == (n + 63) // 64) == (m == 20)
    cs = _load(K, 0, n, devices=devices)
    _crawl_to(cs, 3, 2)
    paths = cs[0].frontier_paths()
    snap = [_snapshot(c) for c in cs]
    for name, (req, msg) in _malformed(K, n, m).items():
        with pytest.raises(fhh.FhhError, match=msg):
            cs[0].join_clients_bincode(req)
        assert _same(_snapshot(cs[0]), snap[0]), name
    _join(cs, K, n, n + m)
    clients = np.arange(n + m)
    ref = _reference(K, clients, paths)
    _assert_equal(cs, ref, K, clients, paths, "after the refusals")
    _lockstep(cs, ref, K.left[:n + m], K.right[:n + m], 2)


@pytest.mark.parametrize("devices", [None, [0, 0]], ids=["one-gpu", "2-shards"])
def test_state_and_framing_refusals(devices):
    from fuzzyheavyhitters_amd._lib import lib, ptr
    K = jc.keyed(1)
    n, m = 70, 30
    Lb = lib()
    good = K.request(0, n, n + m)

    def call(c, req, length=None):
        rc = Lb.fhh_join_clients_bincode(c.handle, None if req is None else ptr(req), len(req) if length is None else length)
        return rc, (Lb.fhh_last_error(c.handle) or b"").decode()

    # before any keys, and with keys but before any init
    e0, _ = _pair(1, devices)
    rc, msg = call(e0, good)
    assert rc == -2 and "no keys" in msg and e0.num_clients() == 0
    cs = _load(K, 0, n, "append" if devices is None else "add_keys", devices)
    s0 = _snapshot(cs[0], states=False)
    rc, msg = call(cs[0], good)
    assert rc == -2 and "no frontier yet" in msg, msg
    assert _same(_snapshot(cs[0], states=False), s0)
    # children pending
    _crawl_to(cs, 2, 2)
    C, _ = cs[0].tree_crawl()
    cs[1].tree_crawl()
    snap = _snapshot(cs[0])
    rc, msg = call(cs[0], good)
    assert rc == -2 and "pending" in msg, msg
    assert _same(_snapshot(cs[0]), snap)
    for c in cs:
        c.tree_prune(np.ones(C, np.uint8))
    # the framing
    paths = cs[0].frontier_paths()
    snap = _snapshot(cs[0])
    zero = np.zeros(8, np.uint8)
    longer = np.concatenate([good, np.zeros(1, np.uint8)])
    for req, length, text in ((None, 0, "shorter"), (good, 4, "shorter"), (zero, None, "no clients"),
                              (good[:-1].copy(), None, "length does not match"), (longer, None, "length does not match"),
                              (good, good.size - jc.record_bytes(1), "length does not match")):
        rc, msg = call(cs[0], req, length)
        assert rc == -1 and text in msg, (msg, text)
        assert _same(_snapshot(cs[0]), snap), text
    _join(cs, K, n, n + m)
    clients = np.arange(n + m)
    ref = _reference(K, clients, paths)
    _assert_equal(cs, ref, K, clients, paths, "after the refusals")
    _lockstep(cs, ref, K.left[:n + m], K.right[:n + m], 2)


def test_join_timing_reports_the_copy():
    """fhh_join_timing: an in-place join copies nothing; a growing one reads and writes the old key store and the
    live table entries once."""
    K = jc.keyed(1)
    cs = _load(K, 0, 70)
    _crawl_to(cs, 3, 2)
    _join(cs, K, 70, 90)
    ms, moved = cs[0].join_timing()
    assert moved == 0 and ms[0] == 0 and ms[1] > 0 and ms[2] > 0
    U = len(cs[0].frontier_paths())   # d = 1: one live entry per node
    _join(cs, K, 90, 200)
    ms, moved = cs[0].join_timing()
    keys = (L * 2 + 2) * (128 * 16) + (L * 2 * 4 + 2) * (2 * 8)
    tables = 2 * U * (128 * 16 + 2 * 2 * 8)
    assert moved == 2 * (keys + tables) and all(x > 0 for x in ms)
