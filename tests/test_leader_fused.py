"""fhh_leader_requests_ball (GPU): points in, both servers' add_keys request bytes out of one kernel, no key storage.
Every byte is compared with workload.add_keys_request_bincode (the numpy serializer) on oracle.gen_keys of the
oracle's bounds (leader_fused_cases.py, ball_cases.py), never with gen_keys_ball + export_keys_bincode alone: at
the lengths, dims, client counts and batch sizes where byte placement can break, in the coordinate form, past one
pass of the grid, on a refused population, on a ctx in the middle of a crawl, over shards, and through
leader.add_fuzzy_keys(route="fused")."""
import ctypes

import numpy as np
import pytest

import ball_cases as bc
import leader_fused_cases as lf

pytestmark = pytest.mark.gpu
FHH_E_ARG = -1


def call_host(c, pts, ball, batch, want_size, **kw):
    """The host form into sentinel-filled buffers of cap > len: (out0, out1) cut to len, the bytes past len
    checked to hold the sentinel."""
    import fuzzyheavyhitters_amd as fhh
    bufs = tuple(np.full(want_size + lf.GUARD, lf.SENTINEL, np.uint8) for _ in range(2))
    got = fhh.leader_requests_ball(c, pts, ball, batch=batch, out=bufs, **kw)
    for g, b in zip(got, bufs):
        assert g.size == want_size and (b[want_size:] == lf.SENTINEL).all(), "bytes past len were written"
    return got


def assert_both(got, ks, n, batch, what, first=0):
    for s in range(2):
        want = lf.expected(ks[s], n, batch, first)
        assert got[s].size == want.size, (what, s)
        assert got[s][-1] == want[-1], (what, s, "last byte")
        assert np.array_equal(got[s], want), f"{what} server {s}: {lf.differing(got[s], want)}"


def device_bytes(c, ptr, off, size):
    """`size` bytes at device address ptr + off of c's GPU, through a torch buffer."""
    import torch
    import fuzzyheavyhitters_amd as fhh
    buf = torch.empty(size, dtype=torch.uint8, device=f"cuda:{c.device}")
    torch.cuda.synchronize(c.device)
    fhh._lib.check(fhh.lib().fhh_memcpy_device(c.device, ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(ptr + off), size))
    return buf.cpu().numpy()


@pytest.mark.parametrize("d", [1, 2, 3])
@pytest.mark.parametrize("L", bc.GPU_LENGTHS + (35,))
def test_request_bytes_equal_the_serializer_on_the_oracles_keys(oracle, L, d):
    """A key is 25 + 20 L bytes, so over the clients and keys of a call the CorWord runs start at every residue
    mod 4; L = 33, 35, 65 end on a partial register group. One population of 130 clients per seed kind (derived
    at a nonzero seed_first, given), keyed once by the oracle; every n of NS is its prefix, at every batch of
    BATCHES. One ctx serves all calls, so a byte a call leaves unwritten shows as a stale one."""
    import fuzzyheavyhitters_amd as fhh
    from fuzzyheavyhitters_amd import workload
    rng = np.random.default_rng(1000 * L + d)
    delta, first = 2 ** 31, 4321
    alpha = lf.population(rng, L, d, 130, delta)
    pts = workload.pack_points(alpha)
    left, right = bc.oracle_bounds(oracle, alpha, delta)
    given = rng.integers(0, 256, (130, d, 2, 2, 16), dtype=np.uint8)
    kinds = [({"seed": bc.SEED, "seed_first": first}, oracle.gen_keys(left, right, bc.derived_roots(oracle, bc.SEED, first, 130, d))),
             (None, oracle.gen_keys(left, right, given))]
    for _, ks in kinds:   # the framing of lf.expected against the serializer called request by request
        assert np.array_equal(lf.expected(ks[1], 130, 7), np.concatenate(lf.request_list(ks[1], 130, 7)))
    c = fhh.KeyCollection(L, d)
    for n in lf.NS:
        for batch in lf.BATCHES:
            size = lf.request_bytes(d, L, n, batch)
            for kw, ks in kinds:
                kw = kw if kw is not None else {"root_seeds": given[:n]}
                got = call_host(c, pts[:n], delta, batch, size, **kw)
                assert_both(got, ks, n, batch, (L, d, n, batch, sorted(kw)))
    assert c.num_clients() == 0   # no keys were made on the ctx


def test_device_form_equals_the_host_form_and_the_oracle(oracle):
    """The device-output form: the pointers it hands out hold the same bytes, *bytes is the request size."""
    import fuzzyheavyhitters_amd as fhh
    from fuzzyheavyhitters_amd import workload
    L, d, n, delta, batch = 65, 2, 130, 8, 7
    rng = np.random.default_rng(65)
    alpha = lf.population(rng, L, d, n, delta)
    left, right = bc.oracle_bounds(oracle, alpha, delta)
    ks = oracle.gen_keys(left, right, bc.derived_roots(oracle, bc.SEED, 5, n, d))
    c = fhh.KeyCollection(L, d)
    p0, p1, nbytes = fhh.leader_requests_ball(c, workload.pack_points(alpha), delta, seed=bc.SEED, seed_first=5,
                                              batch=batch, device_output=True)
    assert nbytes == lf.request_bytes(d, L, n, batch) and p0 and p1 and p0 != p1
    assert_both([device_bytes(c, p, 0, nbytes) for p in (p0, p1)], ks, n, batch, "device form")


def test_seed_counter_crosses_2_to_the_32(oracle):
    """Derived root seeds whose ChaCha20 block counter (seed_first + c) d + j passes 2^32 inside the call."""
    import fuzzyheavyhitters_amd as fhh
    from fuzzyheavyhitters_amd import workload
    L, d, n, delta = 40, 2, 70, 1
    first = 2 ** 31 - 30   # the counters run from 2^32 - 60 to 2^32 + 79
    assert first * d < 2 ** 32 < (first + n) * d
    alpha = lf.population(np.random.default_rng(32), L, d, n, delta)
    left, right = bc.oracle_bounds(oracle, alpha, delta)
    ks = oracle.gen_keys(left, right, bc.derived_roots(oracle, bc.SEED, first, n, d))
    c = fhh.KeyCollection(L, d)
    got = call_host(c, workload.pack_points(alpha), delta, 64, lf.request_bytes(d, L, n, 64), seed=bc.SEED, seed_first=first)
    assert_both(got, ks, n, 64, "counter past 2^32")


def test_coordinate_form(oracle):
    """d = 2, L = 16 — shorter than a level block of the emit kernels, four register groups here: every edge
    (lat, long) at every ball of COORD_BALLS, seeds derived and given in turn, and 1 000 clients of
    coords_workload in requests of 100."""
    import fuzzyheavyhitters_amd as fhh
    from fuzzyheavyhitters_amd import workload
    pts = bc.coord_points()
    n = pts.shape[0]
    rng = np.random.default_rng(16)
    c = fhh.KeyCollection(16, 2)
    for i, ball in enumerate(bc.COORD_BALLS):
        left, right = bc.coords_bounds(oracle, pts, ball)
        if i % 2:
            roots = rng.integers(0, 256, (n, 2, 2, 2, 16), dtype=np.uint8)
            kw = {"root_seeds": roots}
        else:
            roots = bc.derived_roots(oracle, bc.SEED, 77, n, 2)
            kw = {"seed": bc.SEED, "seed_first": 77}
        ks = oracle.gen_keys(left, right, roots)
        batch = (0, 7, 1, 100)[i]
        got = call_host(c, pts, ball, batch, lf.request_bytes(2, 16, n, batch), form="coords", **kw)
        assert_both(got, ks, n, batch, ("coords", ball))
    wl = workload.coords_workload(1000, ball_size=8, num_centroids=50, seed=5)
    from_bits = lambda b: (b.astype(np.int64) << np.arange(15, -1, -1)).sum(-1)
    xy = from_bits(wl.alpha)
    xy = np.where(xy >= 2 ** 15, xy - 2 ** 16, xy).astype(np.int16)
    assert xy.shape == (1000, 2) and np.array_equal(workload.i16_to_bits(xy), wl.alpha)
    left, right = bc.coords_bounds(oracle, xy, 8)
    ks = oracle.gen_keys(left, right, bc.derived_roots(oracle, bc.SEED, 0, 1000, 2))
    got = call_host(c, xy, 8, 100, lf.request_bytes(2, 16, 1000, 100), form="coords", seed=bc.SEED)
    assert_both(got, ks, 1000, 100, "coords_workload")


def test_second_trip_of_the_grid(oracle):
    """d = 4, L = 32, n = 262 145: the plan reports a second, partial trip (8 x 4097 = 32 776 items on 32 768
    waves: the right key of dim 3 of the clients from 261 696 on). The device-output form (2.8 GB of requests that
    never cross to the host); three client ranges — the first words, the middle, the last word with its single
    valid lane, which the second trip completes — against the oracle's keys of those clients only."""
    import fuzzyheavyhitters_amd as fhh
    n, d, L, delta, batch = 262_145, 4, 32, 3, 100
    items, waves, trips = fhh.leader_requests_plan(d, L, n)
    assert trips == 2 and 0 < items - waves < waves and fhh.leader_requests_plan(d, L, n - 1)[2] == 1
    nw = (n + 63) // 64
    assert items - waves == 8 and (items - 8) // nw == 2 * d - 1 and 64 * (nw - 8) == 261_696
    rng = np.random.default_rng(32)
    words = rng.integers(0, 2 ** 32 - delta, (n, d), dtype=np.uint64).astype(">u4")
    words[0, 0] = 0                                   # one wrapped interval
    pts = np.ascontiguousarray(words.view(np.uint8).reshape(n, d, 4))
    c = fhh.KeyCollection(L, d)
    p0, p1, nbytes = fhh.leader_requests_ball(c, pts, delta, seed=bc.SEED, seed_first=9, batch=batch, device_output=True)
    assert nbytes == lf.request_bytes(d, L, n, batch)
    R = 8 + 2 * d * (25 + 20 * L)
    for first, count in ((0, 130), (131_000, 130), (262_080, 65)):
        assert first + count <= n
        alpha = np.unpackbits(pts[first:first + count], axis=-1, bitorder="big")
        left, right = bc.oracle_bounds(oracle, alpha, delta)
        ks = oracle.gen_keys(left, right, bc.derived_roots(oracle, bc.SEED, 9 + first, count, d))
        # the range's bytes, request counts included: client by client against its record, and each u64 m that
        # falls inside the range against the request's size
        lo, hi = lf.client_off(first, d, L, batch, n), lf.client_off(first + count - 1, d, L, batch, n) + R
        for s, p in enumerate((p0, p1)):
            got = device_bytes(c, p, lo, hi - lo)
            recs = lf.expected(ks[s], count, 0)[8:].reshape(count, R)
            for k in range(count):
                i = first + k
                a = lf.client_off(i, d, L, batch, n) - lo
                assert np.array_equal(got[a:a + R], recs[k]), (first, s, i)
                if i % batch == 0 and k:
                    assert int(got[a - 8:a].view("<u8")[0]) == min(batch, n - i), (first, s, i)
    assert hi == nbytes   # the last range ends with the last byte


def test_a_carry_out_is_refused_and_the_ctx_serves_on(oracle):
    """Clients 77 and 3 carry out: FHH_E_ARG naming client 3, out0 / out1 keep their sentinel, no device pointer
    is handed out, and the same ctx then serves a good population."""
    import fuzzyheavyhitters_amd as fhh
    from fuzzyheavyhitters_amd import workload
    n, d, L, delta, batch = 130, 2, 40, 8, 7
    rng = np.random.default_rng(40)
    good = lf.population(rng, L, d, n, delta)
    alpha = good.copy()
    first_refused = (1 << L) - delta
    assert bc.carries_out(first_refused, delta, L) and bc.oracle_refuses(oracle, first_refused, delta, L)
    alpha[77, 0] = bc.bits_of(first_refused, L)
    alpha[3, 1] = bc.bits_of((1 << L) - 1, L)
    c = fhh.KeyCollection(L, d)
    size = lf.request_bytes(d, L, n, batch)
    bufs = tuple(np.full(size + lf.GUARD, lf.SENTINEL, np.uint8) for _ in range(2))
    with pytest.raises(fhh.FhhError, match=r"fhh error -1: .*client 3, dim 1") as e:
        fhh.leader_requests_ball(c, workload.pack_points(alpha), delta, seed=bc.SEED, batch=batch, out=bufs)
    assert "client 77" not in str(e.value)
    assert all((b == lf.SENTINEL).all() for b in bufs)
    src, _, keep = fhh.collection._ball_src(workload.pack_points(alpha), delta, "bits", d, L, None, bc.SEED, 0)
    p0, p1, nb = ctypes.c_void_p(5), ctypes.c_void_p(6), ctypes.c_uint64(7)
    assert fhh.lib().fhh_leader_requests_ball_device(c.handle, n, ctypes.byref(src), batch, ctypes.byref(p0),
                                                     ctypes.byref(p1), ctypes.byref(nb)) == FHH_E_ARG
    assert (p0.value, p1.value, nb.value) == (5, 6, 7)
    del keep
    left, right = bc.oracle_bounds(oracle, good, delta)
    ks = oracle.gen_keys(left, right, bc.derived_roots(oracle, bc.SEED, 0, n, d))
    got = call_host(c, workload.pack_points(good), delta, batch, size, seed=bc.SEED)
    assert_both(got, ks, n, batch, "after a refusal")


def test_argument_refusals_write_nothing(oracle):
    """What ball_src_check refuses, n = 0, NULL outputs, a cap too small (*len still set): FHH_E_ARG, the
    sentinel kept, and the ctx serves on."""
    import fuzzyheavyhitters_amd as fhh
    from fuzzyheavyhitters_amd import workload
    from fuzzyheavyhitters_amd._lib import FhhBallSrc, ptr
    lib = fhh.lib()
    n, d, L = 10, 1, 40
    alpha = lf.population(np.random.default_rng(41), L, d, n, 1)
    pts = workload.pack_points(alpha)
    size = lf.request_bytes(d, L, n, 0)
    c, g = fhh.KeyCollection(L, d), fhh.KeyCollection(16, 2)
    out0, out1 = (np.full(size + lf.GUARD, lf.SENTINEL, np.uint8) for _ in range(2))
    ln = ctypes.c_uint64()

    def call(ctx, form=0, ball=1, points=pts, src=True, count=n, o0=out0, o1=out1, cap=size, plen=ln):
        s = FhhBallSrc()
        s.form, s.ball = form, ball
        s.points = points.ctypes.data if points is not None else None
        s.seed[:] = bc.SEED
        return lib.fhh_leader_requests_ball(ctx.handle, count, ctypes.byref(s) if src else None, 0,
                                            ptr(o0) if o0 is not None else None, ptr(o1) if o1 is not None else None,
                                            cap, ctypes.byref(plen) if plen is not None else None)

    xy = np.zeros((n, 2), np.int16)
    assert call(c, src=False) == FHH_E_ARG                       # NULL source
    assert call(c, form=7) == FHH_E_ARG                          # unknown form
    assert call(c, points=None) == FHH_E_ARG                     # NULL points
    assert call(c, form=1, points=xy) == FHH_E_ARG               # coordinates on d = 1, L = 40
    assert call(g, form=1, ball=32768, points=xy) == FHH_E_ARG   # ball out of range
    assert call(g, form=0, points=xy) == FHH_E_ARG               # bit strings need L >= 32
    assert call(c, count=0) == FHH_E_ARG                         # no clients
    assert call(c, o0=None) == FHH_E_ARG and call(c, o1=None) == FHH_E_ARG and call(c, plen=None) == FHH_E_ARG
    ln.value = 0
    assert call(c, cap=size - 1) == FHH_E_ARG and ln.value == size   # cap too small: *len still set
    assert (out0 == lf.SENTINEL).all() and (out1 == lf.SENTINEL).all()
    s = FhhBallSrc()
    s.points = pts.ctypes.data
    s.seed[:] = bc.SEED
    p0, p1, nb = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_uint64()
    for a0, a1, a2 in ((None, ctypes.byref(p1), ctypes.byref(nb)), (ctypes.byref(p0), None, ctypes.byref(nb)),
                       (ctypes.byref(p0), ctypes.byref(p1), None)):
        assert lib.fhh_leader_requests_ball_device(c.handle, n, ctypes.byref(s), 0, a0, a1, a2) == FHH_E_ARG
    assert call(c) == 0 and ln.value == size
    left, right = bc.oracle_bounds(oracle, alpha, 1)
    ks = oracle.gen_keys(left, right, bc.derived_roots(oracle, bc.SEED, 0, n, d))
    assert_both((out0[:size], out1[:size]), ks, n, 0, "after refusals")
    assert (out0[size:] == lf.SENTINEL).all() and (out1[size:] == lf.SENTINEL).all()


def test_ctx_in_the_middle_of_a_crawl_is_untouched(oracle):
    """A pair at depth 3 calls the new entry on ctx0 between two levels (frontier pruned, no pending children) and
    again with level 4's children pending; export_states, frontier_paths, export_keys and the rest of the crawl
    equal those of a twin pair that never made the call. The requests made there are the oracle's too."""
    import fuzzyheavyhitters_amd as fhh
    from fuzzyheavyhitters_amd import workload
    from fuzzyheavyhitters_amd.collection import sim_eq_count
    n, L, d = 200, 40, 1
    wl = workload.zipf_workload(n, L, d, num_sites=5, seed=77)
    left, right = bc.oracle_bounds(oracle, wl.alpha, 1)
    ks = oracle.gen_keys(left, right, bc.derived_roots(oracle, bc.SEED, 0, n, d))
    pts = workload.pack_points(wl.alpha)
    a = [fhh.KeyCollection(L, d), fhh.KeyCollection(L, d)]
    b = [fhh.KeyCollection(L, d), fhh.KeyCollection(L, d)]
    for pair in (a, b):
        fhh.gen_keys_ball(pair[0], pair[1], pts, 1, seed=bc.SEED)
        for c in pair:
            c.tree_init()
    keys_before = [c.export_keys() for c in a]

    def fused_call(batch):
        got = call_host(a[0], pts, 1, batch, lf.request_bytes(d, L, n, batch), seed=bc.SEED)
        assert_both(got, ks, n, batch, f"mid-crawl batch {batch}")
        for s in range(2):
            for x, y in zip(a[s].export_keys(), keys_before[s]):
                assert np.array_equal(x, y), "the ctx's keys changed"
            assert np.array_equal(a[s].frontier_paths(), b[s].frontier_paths())
            for x, y in zip(a[s].export_states(), b[s].export_states()):
                assert np.array_equal(x, y), "EvalStates changed"
        assert a[0].num_clients() == n and a[0].frontier_size() == b[0].frontier_size()

    kept = []
    for lvl in range(L - 1):
        if lvl == 3:
            fused_call(7)        # depth 3, pending children absent
        out = [c.tree_crawl(share_planes=True) for c in (*a, *b)]
        if lvl == 3:
            fused_call(100)      # depth 3, its children pending
        C = out[0][0]
        assert all(o[0] == C for o in out), f"children differ, level {lvl}"
        for s in range(2):
            assert np.array_equal(out[s][1], out[2 + s][1]), f"share planes differ, level {lvl} server {s}"
            for x, y in zip(a[s].export_states(), b[s].export_states()):
                assert np.array_equal(x, y), f"EvalStates differ, level {lvl} server {s}"
        keeps = [sim_eq_count(pair[0], pair[1], C) >= 2 for pair in (a, b)]
        assert np.array_equal(keeps[0], keeps[1]), f"kept children differ, level {lvl}"
        for pair, keep in zip((a, b), keeps):
            for c in pair:
                c.tree_prune(keep)
        kept.append(keeps[0])
        if not keeps[0].any():
            break
    assert len(kept) > 5 and kept[-1].any(), "the crawl must outlive the calls"
    assert a[0].stats()["levels"] == b[0].stats()["levels"]


@pytest.mark.parametrize("n", [130, 200])
@pytest.mark.parametrize("shards", [2, 3])
def test_shards_on_one_gpu_equal_one_gpu(oracle, shards, n):
    """Multi-device ctxs (the shards on one GPU), ragged n: the host form's bytes are the one-GPU call's and the
    oracle's, at batch 7 — 7 divides no shard boundary (a multiple of 64), so a request straddles two shards and
    has its count from the shard of its first client — and at batch 0 and 100, seeds derived and given. A carry
    out in the last shard is named by its index in the population and leaves the outputs unwritten; the device
    form is refused."""
    import fuzzyheavyhitters_amd as fhh
    from fuzzyheavyhitters_amd import workload
    d, L, delta = 2, 33, 2 ** 31
    rng = np.random.default_rng(n + shards)
    alpha = lf.population(rng, L, d, n, delta)
    pts = workload.pack_points(alpha)
    left, right = bc.oracle_bounds(oracle, alpha, delta)
    given = rng.integers(0, 256, (n, d, 2, 2, 16), dtype=np.uint8)
    plan = fhh.shard_plan(n, shards)
    assert sum(1 for _, cnt in plan if cnt) >= 2 and all(b % 7 for b, cnt in plan if b and cnt)
    one, g = fhh.KeyCollection(L, d), fhh.KeyCollection(L, d, devices=[0] * shards)
    for kw, roots in (({"seed": bc.SEED, "seed_first": 12}, bc.derived_roots(oracle, bc.SEED, 12, n, d)),
                      ({"root_seeds": given}, given)):
        ks = oracle.gen_keys(left, right, roots)
        for batch in (7, 0, 100):
            size = lf.request_bytes(d, L, n, batch)
            got = call_host(g, pts, delta, batch, size, **kw)
            assert_both(got, ks, n, batch, (shards, n, batch))
            for x, y in zip(got, call_host(one, pts, delta, batch, size, **kw)):
                assert np.array_equal(x, y)
    assert g.num_clients() == 0
    with pytest.raises(fhh.FhhError, match="fhh error -1"):
        fhh.leader_requests_ball(g, pts, delta, seed=bc.SEED, device_output=True)
    bad = alpha.copy()
    bad[n - 1, 1] = 1
    bufs = tuple(np.full(lf.request_bytes(d, L, n, 7) + lf.GUARD, lf.SENTINEL, np.uint8) for _ in range(2))
    with pytest.raises(fhh.FhhError, match=rf"client {n - 1}, dim 1"):
        fhh.leader_requests_ball(g, workload.pack_points(bad), delta, seed=bc.SEED, batch=7, out=bufs)
    assert all((b == lf.SENTINEL).all() for b in bufs)


N, L, D, BALL = 250, 40, 1, 1


@pytest.fixture(scope="module")
def population_250(oracle):
    from fuzzyheavyhitters_amd import workload
    wl = workload.zipf_workload(N, L, D, num_sites=8, seed=21)
    left, right = bc.oracle_bounds(oracle, wl.alpha, BALL)
    keys = oracle.gen_keys(left, right, bc.derived_roots(oracle, bc.SEED, 0, N, D))
    return workload.pack_points(wl.alpha), left, right, keys


@pytest.mark.parametrize("batch,chunk", [(100, 100), (7, 98), (0, 100)], ids=["batch100", "batch7-chunk98", "batch0"])
def test_fused_route_requests_are_the_oracles(population_250, batch, chunk):
    """leader.add_fuzzy_keys(route="fused"): 250 clients at L = 40. Byte for byte the oracle's requests; batch 0
    is one request per chunk."""
    import fuzzyheavyhitters_amd as fhh
    pts, _, _, keys = population_250
    chunks = list(fhh.add_fuzzy_keys(pts, BALL, n_dims=D, data_len=L, seed=bc.SEED, batch=batch, chunk=chunk, route="fused"))
    assert len(chunks) == (N + chunk - 1) // chunk and all(len(c) == 2 for c in chunks)
    for s in range(2):
        got = [r for c in chunks for r in c[s]]
        want = lf.request_list(keys[s], N, batch or chunk)
        assert len(got) == len(want) == (N + (batch or chunk) - 1) // (batch or chunk)
        for q, (x, y) in enumerate(zip(got, want)):
            assert np.array_equal(x, y), f"server {s} request {q}"


def test_fused_route_requests_crawl_to_the_heavy_hitters(oracle, population_250):
    """Appended to fresh collections they crawl to workload.plaintext_crawl's heavy hitters."""
    import fuzzyheavyhitters_amd as fhh
    from fuzzyheavyhitters_amd import sim_crawl, workload
    pts, left, right, _ = population_250
    servers = [fhh.KeyCollection(L, D), fhh.KeyCollection(L, D)]
    for reqs in fhh.add_fuzzy_keys(pts, BALL, n_dims=D, data_len=L, seed=bc.SEED, batch=50, chunk=100, route="fused"):
        for c, rs in zip(servers, reqs):
            for r in rs:
                c.add_keys_bincode_append(r)
    assert [c.num_clients() for c in servers] == [N, N]
    res = sim_crawl(servers[0], servers[1], 0.02, mode="count")
    t, tl = oracle.thresholds(0.02, N)
    counts, paths, finals = workload.plaintext_crawl(left, right, t, tl)
    assert len(paths) > 0
    assert [c.tolist() for c in res.counts] == [c.tolist() for c in counts]
    assert [tuple(tuple(int(b) for b in pj) for pj in r.path) for r in res.final] == paths
    assert [int(r.value) for r in res.final] == finals
