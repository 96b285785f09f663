"""fhh_gen_keys_ball (GPU): both servers' keys made from a population's points — the bounds and root seeds computed in
k_keygen — against the oracle's keys of the oracle's bounds (ball_cases.py: oracle.l_inf_ball_bounds /
oracle.i16_to_bitvec -> oracle.gen_keys, oracle.chacha_block for derived seeds), never against fhh_ball_bounds or
fhh_gen_keys_pair: the constructed points at the word and lane edges, the coordinate cases, a second pass of the
keygen grid, refusals that leave the ctxs empty, shards, and a crawl of the keys."""
import ctypes

import numpy as np
import pytest

import ball_cases as bc

pytestmark = pytest.mark.gpu
FHH_E_ARG, FHH_E_STATE = -1, -2
FIELDS = ("key_idx", "root_seed", "cw_seed", "cw_bits")


def assert_keys(colls, want, what):
    for s, (c, ks) in enumerate(zip(colls, want)):
        for name, got in zip(FIELDS, c.export_keys()):
            assert np.array_equal(got, getattr(ks, name)), f"{what}: server {s} {name}"


def population(rng, L, d, n, delta):
    """n d points: the accepted constructed ones first (a = 0 among them), uniform ones after."""
    acc, _ = bc.split_cases(L, delta)
    vals = [a for _, a in acc][:n * d]
    vals += bc.random_points(rng, n * d - len(vals), L, delta)
    return bc.alpha_array(vals, d, L)


@pytest.mark.parametrize("d", [1, 2, 3])
@pytest.mark.parametrize("L", bc.GPU_LENGTHS)
def test_keys_of_constructed_points_equal_the_oracle(oracle, L, d):
    """n = 130 at every ball size, n = 1, 63, 64, 65 (the partial last word's invalid lanes) at two; root seeds
    given by the host and derived in the kernel in turn."""
    import fuzzyheavyhitters_amd as fhh
    from fuzzyheavyhitters_amd import workload
    rng = np.random.default_rng(100 * L + d)
    c0, c1 = fhh.KeyCollection(L, d), fhh.KeyCollection(L, d)
    runs = [(130, delta) for delta in bc.DELTAS] + [(n, delta) for n in (1, 63, 64, 65) for delta in (1, 2 ** 32 - 1)]
    for i, (n, delta) in enumerate(runs):
        alpha = population(rng, L, d, n, delta)
        left, right = bc.oracle_bounds(oracle, alpha, delta)
        if i % 2:
            roots = rng.integers(0, 256, (n, d, 2, 2, 16), dtype=np.uint8)
            kw = {"root_seeds": roots}
        else:
            roots = bc.derived_roots(oracle, bc.SEED, 1000 * i, n, d)
            kw = {"seed": bc.SEED, "seed_first": 1000 * i}
        c0.reset()
        c1.reset()
        fhh.gen_keys_ball(c0, c1, workload.pack_points(alpha), delta, **kw)
        assert c0.num_clients() == n and c1.num_clients() == n
        assert_keys((c0, c1), oracle.gen_keys(left, right, roots), (L, d, n, delta))


def test_keys_of_coordinates_equal_the_oracle(oracle):
    import fuzzyheavyhitters_amd as fhh
    pts = bc.coord_points()
    n = pts.shape[0]
    rng = np.random.default_rng(16)
    c0, c1 = fhh.KeyCollection(16, 2), fhh.KeyCollection(16, 2)
    for i, ball in enumerate(bc.COORD_BALLS):
        left, right = bc.coords_bounds(oracle, pts, ball)
        if i % 2:
            roots = rng.integers(0, 256, (n, 2, 2, 2, 16), dtype=np.uint8)
            kw = {"root_seeds": roots}
        else:
            roots = bc.derived_roots(oracle, bc.SEED, 77, n, 2)
            kw = {"seed": bc.SEED, "seed_first": 77}
        c0.reset()
        c1.reset()
        fhh.gen_keys_ball(c0, c1, pts, ball, form="coords", **kw)
        assert_keys((c0, c1), oracle.gen_keys(left, right, roots), ("coords", ball))


def test_second_trip_of_the_keygen_grid(oracle):
    """d = 4, L = 32, n = 262 145: 8 x 4097 = 32 776 items on 32 768 waves, so the last 8 items — the right key of
    dim 3 of the clients from 261 696 on — are made in a second pass of the grid-stride loop. The requests of three
    client ranges (the first words, the middle, the last word with its single valid lane) against the serializer
    on the oracle's keys."""
    import fuzzyheavyhitters_amd as fhh
    from fuzzyheavyhitters_amd import workload
    n, d, L, delta = 262_145, 4, 32, 3
    assert bc.keygen_trips(n, d) == 2 and bc.keygen_trips(n - 1, d) == 1
    nw = (n + 63) // 64
    assert 2 * d * nw - 32_768 == 8 and (2 * d * nw - 8) // nw == 2 * d - 1 and 64 * (nw - 8) == 261_696
    rng = np.random.default_rng(32)
    words = rng.integers(0, 2 ** 32 - delta, (n, d), dtype=np.uint64).astype(">u4")
    words[0, 0] = 0                                   # one wrapped interval
    pts = np.ascontiguousarray(words.view(np.uint8).reshape(n, d, 4))
    c0, c1 = fhh.KeyCollection(L, d), fhh.KeyCollection(L, d)
    fhh.gen_keys_ball(c0, c1, pts, delta, seed=bc.SEED, seed_first=9)
    assert c0.num_clients() == n
    for first, count in ((0, 130), (131_000, 130), (262_080, 65)):
        assert first + count <= n
        alpha = np.unpackbits(pts[first:first + count], axis=-1, bitorder="big")
        left, right = bc.oracle_bounds(oracle, alpha, delta)
        ks = oracle.gen_keys(left, right, bc.derived_roots(oracle, bc.SEED, 9 + first, count, d))
        for c, k in zip((c0, c1), ks):
            want = workload.add_keys_request_bincode(k.key_idx, k.root_seed, k.cw_seed, k.cw_bits)
            assert np.array_equal(c.export_keys_bincode(first, count), want), (first, count)


def test_a_refused_population_leaves_the_ctxs_empty(oracle):
    """A carry out at client 77 and at client 3: FHH_E_ARG naming client 3, both ctxs empty, and the same ctxs then
    key a good population."""
    import fuzzyheavyhitters_amd as fhh
    from fuzzyheavyhitters_amd import workload
    n, d, L, delta = 130, 2, 40, 8
    rng = np.random.default_rng(40)
    alpha = population(rng, L, d, n, delta)
    good = alpha.copy()
    first_refused = (1 << L) - delta
    assert bc.carries_out(first_refused, delta, L) and bc.oracle_refuses(oracle, first_refused, delta, L)
    alpha[77, 0] = bc.bits_of(first_refused, L)
    alpha[3, 1] = bc.bits_of((1 << L) - 1, L)
    c0, c1 = fhh.KeyCollection(L, d), fhh.KeyCollection(L, d)
    with pytest.raises(fhh.FhhError, match=r"fhh error -1: .*client 3, dim 1") as e:
        fhh.gen_keys_ball(c0, c1, workload.pack_points(alpha), delta, seed=bc.SEED)
    assert "client 77" not in str(e.value)
    out = np.zeros(64, np.uint8)
    got = ctypes.c_uint64()
    for c in (c0, c1):
        assert c.num_clients() == 0
        assert fhh.lib().fhh_export_keys_bincode(c.handle, 0, 1, 0, fhh._lib.ptr(out), out.size,
                                                 ctypes.byref(got)) == FHH_E_STATE
        with pytest.raises(fhh.FhhError):
            c.tree_init()
    left, right = bc.oracle_bounds(oracle, good, delta)
    fhh.gen_keys_ball(c0, c1, workload.pack_points(good), delta, seed=bc.SEED)
    assert_keys((c0, c1), oracle.gen_keys(left, right, bc.derived_roots(oracle, bc.SEED, 0, n, d)), "after a refusal")


def test_state_and_argument_refusals(oracle):
    import fuzzyheavyhitters_amd as fhh
    from fuzzyheavyhitters_amd import workload
    from fuzzyheavyhitters_amd._lib import FhhBallSrc
    lib = fhh.lib()
    n, d, L = 10, 1, 40
    alpha = population(np.random.default_rng(41), L, d, n, 1)
    pts = workload.pack_points(alpha)
    c0, c1 = fhh.KeyCollection(L, d), fhh.KeyCollection(L, d)

    def call(a, b, form=0, ball=1, points=pts, src=True):
        s = FhhBallSrc()
        s.form, s.ball = form, ball
        s.points = points.ctypes.data if points is not None else None
        s.seed[:] = bc.SEED
        return lib.fhh_gen_keys_ball(a.handle, b.handle, n, ctypes.byref(s) if src else None)

    assert call(c0, c1, src=False) == FHH_E_ARG                                   # NULL source
    assert call(c0, c1, form=7) == FHH_E_ARG                                      # unknown form
    assert call(c0, c1, points=None) == FHH_E_ARG                                 # NULL points
    assert call(c0, c1, form=1, points=np.zeros((n, 2), np.int16)) == FHH_E_ARG   # coordinates on d = 1, L = 40
    for other in (fhh.KeyCollection(L, 2), fhh.KeyCollection(48, d)):             # ctxs differ in d / L
        assert call(c0, other) == FHH_E_ARG and call(other, c0) == FHH_E_ARG
    g0, g1 = fhh.KeyCollection(16, 2), fhh.KeyCollection(16, 2)
    xy = np.zeros((n, 2), np.int16)
    assert call(g0, g1, form=1, ball=32768, points=xy) == FHH_E_ARG               # ball out of range
    assert call(g0, g1, form=0, points=xy) == FHH_E_ARG                           # bit strings need L >= 32
    for c in (c0, c1, g0, g1):
        assert c.num_clients() == 0
    assert call(g0, g1, form=1, ball=32767, points=xy) == 0 and g1.num_clients() == n
    # the refused ctxs are usable, and full ctxs refuse
    assert call(c0, c1) == 0
    left, right = bc.oracle_bounds(oracle, alpha, 1)
    assert_keys((c0, c1), oracle.gen_keys(left, right, bc.derived_roots(oracle, bc.SEED, 0, n, d)), "after refusals")
    assert call(c0, c1) == FHH_E_STATE
    assert call(c0, fhh.KeyCollection(L, d)) == FHH_E_STATE and call(fhh.KeyCollection(L, d), c1) == FHH_E_STATE
    assert_keys((c0, c1), oracle.gen_keys(left, right, bc.derived_roots(oracle, bc.SEED, 0, n, d)), "kept")


@pytest.mark.parametrize("n", [130, 200])
@pytest.mark.parametrize("shards", [2, 3])
def test_shards_on_one_gpu_equal_one_collection(oracle, shards, n):
    """Multi-device ctxs (the shards on one GPU): shard k keys its slice of the points at seed_first + its first
    client, so export_keys equals the one-GPU collection's and the oracle's, with derived and with given root
    seeds; a carry out in a later shard is named by its index in the population."""
    import fuzzyheavyhitters_amd as fhh
    from fuzzyheavyhitters_amd import workload
    d, L, delta = 2, 33, 2 ** 31
    rng = np.random.default_rng(n + shards)
    alpha = population(rng, L, d, n, delta)
    pts = workload.pack_points(alpha)
    left, right = bc.oracle_bounds(oracle, alpha, delta)
    given = rng.integers(0, 256, (n, d, 2, 2, 16), dtype=np.uint8)
    for kw, roots in (({"seed": bc.SEED, "seed_first": 12}, bc.derived_roots(oracle, bc.SEED, 12, n, d)),
                      ({"root_seeds": given}, given)):
        s0, s1 = fhh.KeyCollection(L, d), fhh.KeyCollection(L, d)
        g0, g1 = fhh.KeyCollection(L, d, devices=[0] * shards), fhh.KeyCollection(L, d, devices=[0] * shards)
        fhh.gen_keys_ball(s0, s1, pts, delta, **kw)
        fhh.gen_keys_ball(g0, g1, pts, delta, **kw)
        info, _ = g0.shard_info()
        assert len(info) == shards and sum(c for _, _, c in info) == n and sum(1 for _, _, c in info if c) >= 2
        for s, g in ((s0, g0), (s1, g1)):
            for a, b in zip(s.export_keys(), g.export_keys()):
                assert np.array_equal(a, b)
        assert_keys((g0, g1), oracle.gen_keys(left, right, roots), (shards, n))
    bad = alpha.copy()
    bad[n - 1, 1] = 1
    g0, g1 = fhh.KeyCollection(L, d, devices=[0] * shards), fhh.KeyCollection(L, d, devices=[0] * shards)
    with pytest.raises(fhh.FhhError, match=rf"client {n - 1}, dim 1"):
        fhh.gen_keys_ball(g0, g1, workload.pack_points(bad), delta, seed=bc.SEED)
    assert g0.num_clients() == 0 and g1.num_clients() == 0
    fhh.gen_keys_ball(g0, g1, pts, delta, root_seeds=given)
    assert_keys((g0, g1), oracle.gen_keys(left, right, given), "group after a refusal")


def test_crawl_of_keys_made_from_points(oracle):
    """n = 300, L = 40, ball 1: the crawl of the pair keyed from the points equals the plaintext crawl on the
    oracle's bounds, level by level and in the final (path, count) set; client 0 is the point a = 0, whose
    interval wraps (l = 2^L - 1 > r = 1) and counts as the keys of those bounds make it count."""
    import fuzzyheavyhitters_amd as fhh
    from fuzzyheavyhitters_amd import sim_crawl, workload
    n, L, d = 300, 40, 1
    wl = workload.zipf_workload(n, L, d, num_sites=8, seed=3)
    alpha = wl.alpha.copy()
    alpha[0] = 0
    left, right = bc.oracle_bounds(oracle, alpha, 1)
    assert left[0].all() and right[0, 0].tolist() == bc.bits_of(1, L)
    c0, c1 = fhh.KeyCollection(L, d), fhh.KeyCollection(L, d)
    fhh.gen_keys_ball(c0, c1, workload.pack_points(alpha), 1, seed=bc.SEED)
    res = sim_crawl(c0, c1, 0.02, mode="count")
    t, tl = oracle.thresholds(0.02, n)
    counts, paths, finals = workload.plaintext_crawl(left, right, t, tl)
    assert len(paths) > 0
    assert [c.tolist() for c in res.counts] == [c.tolist() for c in counts]
    assert [tuple(tuple(int(b) for b in pj) for pj in r.path) for r in res.final] == paths
    assert [int(r.value) for r in res.final] == finals
