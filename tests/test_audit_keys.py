"""fhh_audit_keys_ball (GPU): both servers' keys of a population evaluated at the probes of its points, against the
CPU model of audit_cases.py (the oracle's bounds, Python-int probes, oracle.eval_bit walks, the interval rule) —
never against fhh_gen_keys_ball or the audit itself. Good keys from every source of keys, tampered keys loaded by
add_keys, the grid-stride loop at small grids and on the full grid, the device form feeding retain_clients_device, an
audit in the middle of a crawl, shards, refusals, and the leader's option."""
import ctypes

import numpy as np
import pytest

import audit_cases as ac
import ball_cases as bc

pytestmark = pytest.mark.gpu
FHH_E_ARG, FHH_E_STATE = -1, -2


def pair(fhh, L, d, k0=None, k1=None, **kw):
    c0, c1 = fhh.KeyCollection(L, d, **kw), fhh.KeyCollection(L, d, **kw)
    if k0 is not None:
        ac.add_to(c0, k0)
        ac.add_to(c1, k1)
    return c0, c1


def assert_all_ok(ok, rep, n, d, L, what):
    assert ok.dtype == np.uint8 and ok.shape == (n,) and ok.all(), what
    assert rep["n_bad_clients"] == 0 and ac.report_first(rep) is None, what
    assert rep["n_checks"] == ac.plan(d, L, n, 1)["n_checks"] == n * 2 * d * 5 * L, what
    assert rep["seed_diverged"] == 0, what


def assert_equals_model(ok, rep, m, what):
    assert np.array_equal(ok, m["ok"]), what
    assert rep["n_bad_clients"] == m["n_bad_clients"], what
    assert ac.report_first(rep) == m["first"], what


# ---- good keys ----
@pytest.mark.parametrize("d", [1, 2, 3])
@pytest.mark.parametrize("L", bc.GPU_LENGTHS)
def test_good_keys_from_every_source_are_all_ok(oracle, L, d):
    """n = 1, 63, 64, 65, 130 (the partial last word's idle lanes), the ball sizes in turn; a = 0 (client 0, dim 0)
    wraps wherever ball > 0. Keys made by gen_keys_ball, the oracle's keys staged by add_keys (uploaded by the audit),
    and leader_requests_ball bytes appended in two batches into fresh collections (a capacity-strided layout)."""
    import fuzzyheavyhitters_amd as fhh
    from fuzzyheavyhitters_amd import workload
    rng = np.random.default_rng(1000 * L + d)
    c0, c1 = pair(fhh, L, d)
    for i, n in enumerate((1, 63, 64, 65, 130)):
        delta = bc.DELTAS[(i + d) % len(bc.DELTAS)]
        alpha = ac.population(rng, L, d, n, delta)
        assert not alpha[0, 0].any()
        pts = workload.pack_points(alpha)
        c0.reset()
        c1.reset()
        fhh.gen_keys_ball(c0, c1, pts, delta, seed=bc.SEED, seed_first=7 * i)
        ok, rep = c0.audit_keys_ball(c1, pts, delta)
        assert_all_ok(ok, rep, n, d, L, ("gen_keys_ball", n, delta))
        k0, k1, _ = ac.oracle_keys(oracle, rng, alpha, delta)
        s0, s1 = pair(fhh, L, d, k0, k1)
        ok, rep = s0.audit_keys_ball(s1, pts, delta)
        assert_all_ok(ok, rep, n, d, L, ("add_keys", n, delta))
        assert s0.num_clients() == n
        a0, a1 = pair(fhh, L, d)
        reqs = fhh.leader_requests_ball(c0, pts, delta, seed=bc.SEED, seed_first=3, batch=(n + 1) // 2)
        for a, r in zip((a0, a1), reqs):
            for part in workload.split_add_keys_requests(r, d, L):
                a.add_keys_bincode_append(part)
        ok, rep = a0.audit_keys_ball(a1, pts, delta)
        assert_all_ok(ok, rep, n, d, L, ("appended", n, delta))


def test_good_coordinate_keys_are_all_ok(oracle):
    """1 000 clients of the coordinate workload, and every (lat, long) of the clamp edges at every ball size."""
    import fuzzyheavyhitters_amd as fhh
    from fuzzyheavyhitters_amd import workload
    wl = workload.coords_workload(1000, ball_size=3, num_centroids=50)
    w = 1 << np.arange(15, -1, -1)
    pts = (wl.alpha.astype(np.int64) * w).sum(-1).astype(np.uint16).view(np.int16).reshape(1000, 2)
    c0, c1 = pair(fhh, 16, 2)
    fhh.gen_keys_ball(c0, c1, pts, 3, form="coords", seed=bc.SEED)
    ok, rep = c0.audit_keys_ball(c1, pts, 3, form="coords")
    assert_all_ok(ok, rep, 1000, 2, 16, "coords workload")
    edges = bc.coord_points()
    for ball in bc.COORD_BALLS:
        left, right = bc.coords_bounds(oracle, edges, ball)
        roots = np.random.default_rng(ball).integers(0, 256, (edges.shape[0], 2, 2, 2, 16), dtype=np.uint8)
        s0, s1 = oracle.gen_keys(left, right, roots)
        e0, e1 = pair(fhh, 16, 2, ac.keys_arrays(s0), ac.keys_arrays(s1))
        ok, rep = e0.audit_keys_ball(e1, edges, ball, form="coords")
        assert_all_ok(ok, rep, edges.shape[0], 2, 16, ("clamp edges", ball))
    # the same keys against the points moved by one: a different interval wherever no clamp hides it
    ok, rep = e0.audit_keys_ball(e1, edges + np.int16(1), bc.COORD_BALLS[-1], form="coords")
    l, r, a = ac.coords_points(oracle, edges + np.int16(1), bc.COORD_BALLS[-1])
    m = ac.audit(oracle, ac.keys_arrays(s0), ac.keys_arrays(s1), l, r, a, 16)
    assert m["n_bad_clients"] > 0
    assert_equals_model(ok, rep, m, "coords moved by one")


# ---- tampered keys ----
@pytest.fixture(scope="module")
def base(oracle):
    """70 clients (two words), d = 2, L = 40, ball 8: the oracle's keys of the oracle's bounds and the model's
    audit of them, computed once; a tamper case changes one client's keys, so the model is re-run on that client."""
    from fuzzyheavyhitters_amd import workload
    L, d, n, delta = 40, 2, 70, 8
    rng = np.random.default_rng(4070)
    alpha = ac.population(rng, L, d, n, delta)
    k0, k1, (l, r, a) = ac.oracle_keys(oracle, rng, alpha, delta)
    m = ac.audit(oracle, k0, k1, l, r, a, L)
    assert m["ok"].all() and m["seed_diverged"] == 0
    other = ac.population(rng, L, d, n, delta)[::-1].copy()
    o0, o1, _ = ac.oracle_keys(oracle, rng, other, delta)
    return dict(L=L, d=d, n=n, delta=delta, pts=workload.pack_points(alpha), k0=k0, k1=k1, l=l, r=r, a=a, o0=o0, o1=o1)


def tampered(base):
    return {f: v.copy() for f, v in base["k0"].items()}, {f: v.copy() for f, v in base["k1"].items()}


def run_tamper(oracle, base, k0, k1, clients):
    import fuzzyheavyhitters_amd as fhh
    c0, c1 = pair(fhh, base["L"], base["d"], k0, k1)
    ok, rep = c0.audit_keys_ball(c1, base["pts"], base["delta"])
    m = ac.audit(oracle, k0, k1, base["l"], base["r"], base["a"], base["L"], clients=clients)
    assert_equals_model(ok, rep, m, clients)
    assert rep["n_checks"] == ac.plan(base["d"], base["L"], base["n"], 1)["n_checks"]
    assert rep["seed_diverged"] == m["seed_diverged"]
    return rep, m


@pytest.mark.parametrize("copies_hit", ["both", "ctx1"])
@pytest.mark.parametrize("k", [0, 31, 32, 39])
def test_a_flipped_y_control_bit(oracle, base, k, copies_hit):
    """CorWord k's y bit of the direction l takes, left key of (client 37, dim 1): in both copies it is flagged at
    probe 1 (x = l), level k + 1, deterministically; in ctx1's copy alone the model says where."""
    L, c, j = base["L"], 37, 1
    k0, k1 = tampered(base)
    ac.flip_y_bit((k0, k1) if copies_hit == "both" else (k1,), c, j, 0, k, (int(base["l"][c, j]) >> (L - 1 - k)) & 1)
    rep, m = run_tamper(oracle, base, k0, k1, [c])
    if copies_hit == "both":
        assert (c, j, 0, 1, k + 1) in m["failures"] and rep["n_bad_clients"] == 1
        assert (rep["first_client"], rep["first_dim"], rep["first_side"], rep["first_level"]) == (c, j, 0, k + 1)


def test_flipped_seed_bits(oracle, base):
    """One seed bit of a CorWord (both copies) and one root seed bit (ctx1): no compared bit depends on a seed, so
    every client stays ok, as the model has it; the walks that end off the path with unequal seeds are counted."""
    k0, k1 = tampered(base)
    ac.flip_cw_seed_bit((k0, k1), 12, 0, 1, 17)
    ac.flip_root_seed_bit(k1, 66, 1, 0)
    rep, m = run_tamper(oracle, base, k0, k1, [12, 66])
    assert rep["n_bad_clients"] == 0 and rep["seed_diverged"] > 0


def test_keys_of_a_different_point(oracle, base):
    k0, k1 = tampered(base)
    ac.swap_in_keys((k0, k1), 64, (base["o0"], base["o1"]), 5)
    rep, m = run_tamper(oracle, base, k0, k1, [64])
    assert rep["n_bad_clients"] == 1 and rep["first_client"] == 64


def test_two_bad_clients_in_different_words(oracle, base):
    L = base["L"]
    k0, k1 = tampered(base)
    ac.flip_y_bit((k0, k1), 69, 0, 1, 5, (int(base["r"][69, 0]) >> (L - 1 - 5)) & 1)
    ac.flip_y_bit((k0, k1), 3, 1, 0, 20, (int(base["l"][3, 1]) >> (L - 1 - 20)) & 1)
    rep, m = run_tamper(oracle, base, k0, k1, [3, 69])
    assert rep["n_bad_clients"] == 2 and rep["first_client"] == 3 and not m["ok"][69]


# ---- the grid-stride loop ----
@pytest.mark.parametrize("n", [1100, 2100])
@pytest.mark.parametrize("grid", [1, 2, 3])
def test_trips_of_a_small_grid(oracle, grid, n):
    """d = 2, L = 32 under fhh_set_expand_grid: at least two trips, the last one partial. Tampered clients sit in
    the first word, in the last word (its last key: an item of the last trip) and in the first item of the last trip;
    n_checks shows that no item was skipped."""
    import fuzzyheavyhitters_amd as fhh
    from fuzzyheavyhitters_amd import workload
    L, d, delta = 32, 2, 3
    p = fhh.audit_plan(d, L, n, grid)
    assert p == ac.plan(d, L, n, grid) and p["trips"] >= 2 and 0 < p["last_trip_items"] < p["waves"]
    nwc = (n + 63) // 64
    first_of_last = (p["trips"] - 1) * p["waves"]
    kk, w = divmod(first_of_last, nwc)            # item = key * words + word
    picks = [(5, 0, 0), (n - 1, d - 1, 1), (64 * w + 1, kk >> 1, kk & 1)]
    assert (2 * (d - 1) + 1) * nwc + nwc - 1 == p["items"] - 1 >= first_of_last and 64 * w + 1 < n
    rng = np.random.default_rng(n + grid)
    alpha = bc.alpha_array(bc.random_points(rng, n * d, L, delta), d, L)
    k0, k1, (l, r, a) = ac.oracle_keys(oracle, rng, alpha, delta)
    for c, j, side in picks:
        bound = int((l if side == 0 else r)[c, j])
        ac.flip_y_bit((k0, k1), c, j, side, 9, (bound >> (L - 1 - 9)) & 1)
    c0, c1 = pair(fhh, L, d, k0, k1)
    c0.set_expand_grid(grid)
    ok, rep = c0.audit_keys_ball(c1, workload.pack_points(alpha), delta)
    clients = sorted({c for c, _, _ in picks})
    m = ac.audit(oracle, k0, k1, l, r, a, L, clients=clients)
    assert m["n_bad_clients"] == len(clients)
    assert_equals_model(ok, rep, m, (grid, n))
    assert rep["n_checks"] == p["n_checks"]


def test_the_full_grid_at_262145_clients(oracle):
    """d = 4, L = 32, n = 262 145: 8 x 4097 = 32 776 items on the full grid. The keys are gen_keys_ball's; the audit
    gets the points with the last client's dim 3 moved, so the one client of the last word holds keys of a different
    point. The model runs on that client, with the oracle's keys of its original point."""
    import fuzzyheavyhitters_amd as fhh
    n, d, L, delta = 262_145, 4, 32, 3
    assert ac.plan(d, L, n, 2 ** 20)["items"] == 32_776
    rng = np.random.default_rng(32)
    words = rng.integers(0, 2 ** 32 - delta, (n, d), dtype=np.uint64).astype(">u4")
    words[0, 0] = 0                                   # one wrapped interval
    pts = np.ascontiguousarray(words.view(np.uint8).reshape(n, d, 4))
    c0, c1 = pair(fhh, L, d)
    fhh.gen_keys_ball(c0, c1, pts, delta, seed=bc.SEED, seed_first=9)
    ok, rep = c0.audit_keys_ball(c1, pts, delta)
    assert_all_ok(ok, rep, n, d, L, "full grid")
    moved = pts.copy()
    moved[n - 1, 3] = np.frombuffer(int((int(words[n - 1, 3]) + 77_777) % (2 ** 32 - delta)).to_bytes(4, "big"), np.uint8)
    ok, rep = c0.audit_keys_ball(c1, moved, delta)
    one = np.unpackbits(pts[n - 1:], axis=-1, bitorder="big")
    left, right = bc.oracle_bounds(oracle, one, delta)
    s0, s1 = oracle.gen_keys(left, right, bc.derived_roots(oracle, bc.SEED, 9 + n - 1, 1, d))
    l, r, a = ac.bits_points(oracle, np.unpackbits(moved[n - 1:], axis=-1, bitorder="big"), delta)
    m = ac.audit(oracle, ac.keys_arrays(s0), ac.keys_arrays(s1), l, r, a, L)
    assert m["first"] is not None and m["first"][1] == 3
    assert not ok[n - 1] and ok[:n - 1].all() and rep["n_bad_clients"] == 1
    assert ac.report_first(rep) == (n - 1,) + m["first"][1:]
    assert rep["n_checks"] == fhh.audit_plan(d, L, n, 2 ** 20)["n_checks"] == n * 2 * d * 5 * L


# ---- the device form ----
def test_device_ok_bytes_feed_retain_clients_device(oracle, base):
    """ok_dev equals the host form's bytes; handed to retain_clients_device on both servers it leaves the good
    clients' collection: export_keys equals the survivors' keys and a re-audit against their points is all ok."""
    import torch
    import fuzzyheavyhitters_amd as fhh
    L, d, n = base["L"], base["d"], base["n"]
    k0, k1 = tampered(base)
    ac.swap_in_keys((k0, k1), 0, (base["o0"], base["o1"]), 1)
    ac.swap_in_keys((k0, k1), 63, (base["o0"], base["o1"]), 2)
    ac.flip_y_bit((k0, k1), 68, 1, 1, 0, (int(base["r"][68, 1]) >> (L - 1)) & 1)
    c0, c1 = pair(fhh, L, d, k0, k1)
    ok, rep = c0.audit_keys_ball(c1, base["pts"], base["delta"])
    ok_dev, rep_dev = c0.audit_keys_ball_device(c1, base["pts"], base["delta"])
    assert ok_dev.dtype == torch.uint8 and ok_dev.is_cuda and tuple(ok_dev.shape) == (n,)
    assert np.array_equal(ok_dev.cpu().numpy(), ok)
    assert {k: v for k, v in rep_dev.items() if k != "kernel_ms"} == {k: v for k, v in rep.items() if k != "kernel_ms"}
    m = ac.audit(oracle, k0, k1, base["l"], base["r"], base["a"], L, clients=[0, 63, 68])
    assert_equals_model(ok, rep, m, "device form")
    keep = [c for c in range(n) if c not in (0, 63, 68)]
    assert m["n_bad_clients"] == 3
    for c, k in ((c0, k0), (c1, k1)):
        assert c.retain_clients_device(ok_dev) == n - 3
        for f, got in zip(ac.FIELDS, c.export_keys()):
            assert np.array_equal(got, k[f][keep]), f
    ok2, rep2 = c0.audit_keys_ball(c1, base["pts"][keep], base["delta"])
    assert_all_ok(ok2, rep2, n - 3, d, L, "survivors")


# ---- in the middle of a crawl ----
@pytest.mark.parametrize("pending", [False, True])
def test_an_audit_in_the_middle_of_a_crawl_changes_nothing(oracle, pending):
    """A pair at depth 3, audited at its frontier or with its children pending: the states, the paths and the next
    level's share planes equal those of a twin that was not audited."""
    import fuzzyheavyhitters_amd as fhh
    from fuzzyheavyhitters_amd import workload
    L, d, n, delta = 40, 1, 130, 1
    alpha = ac.population(np.random.default_rng(5), L, d, n, delta)
    pts = workload.pack_points(alpha)
    pairs = []
    for _ in range(2):
        c0, c1 = pair(fhh, L, d)
        fhh.gen_keys_ball(c0, c1, pts, delta, seed=bc.SEED)
        for c in (c0, c1):
            c.tree_init()
            for _lvl in range(3):
                C, _ = c.tree_crawl()
                c.tree_prune(np.ones(C, bool))
            assert c.frontier_size()[0] == 8
            if pending:
                assert c.tree_crawl()[0] == 16
        pairs.append((c0, c1))
    (c0, c1), (t0, t1) = pairs
    ok, rep = c0.audit_keys_ball(c1, pts, delta)
    assert_all_ok(ok, rep, n, d, L, "mid-crawl")
    for c, t in ((c0, t0), (c1, t1)):
        assert c.frontier_size() == t.frontier_size()
        assert np.array_equal(c.frontier_paths(), t.frontier_paths())
        for x, y in zip(c.export_states(), t.export_states()):
            assert np.array_equal(x, y)
        if pending:
            c.tree_prune(np.ones(16, bool))
            t.tree_prune(np.ones(16, bool))
        (C, planes), (Ct, planes_t) = c.tree_crawl(share_planes=True), t.tree_crawl(share_planes=True)
        assert C == Ct == (32 if pending else 16) and np.array_equal(planes, planes_t)
        for x, y in zip(c.export_states(), t.export_states()):
            assert np.array_equal(x, y)


# ---- shards ----
@pytest.mark.parametrize("shards", [2, 3])
def test_shards_equal_one_gpu(oracle, shards):
    """n = 200 on 2 and 3 shards (on one GPU): a bad client in each shard is reported at its global index, the
    report equals the one-GPU pair's and the model's; after a retain that leaves a shard's base off a word boundary
    the survivors' audit still equals one GPU's; the device form is refused."""
    import fuzzyheavyhitters_amd as fhh
    from fuzzyheavyhitters_amd import workload
    L, d, n, delta = 33, 2, 200, 2 ** 31
    rng = np.random.default_rng(200 + shards)
    alpha = ac.population(rng, L, d, n, delta)
    pts = workload.pack_points(alpha)
    k0, k1, (l, r, a) = ac.oracle_keys(oracle, rng, alpha, delta)
    bad = (10, 70, 150)
    for c in bad:
        ac.flip_y_bit((k0, k1), c, c % d, c % 2, 32, (int((l if c % 2 == 0 else r)[c, c % d]) >> (L - 1 - 32)) & 1)
    g0, g1 = pair(fhh, L, d, k0, k1, devices=[0] * shards)
    s0, s1 = pair(fhh, L, d, k0, k1)
    ok_g, rep_g = g0.audit_keys_ball(g1, pts, delta)
    ok_s, rep_s = s0.audit_keys_ball(s1, pts, delta)
    info, _ = g0.shard_info()
    assert len(info) == shards and all(any(b <= c < b + cnt for c in bad) for _, b, cnt in info)
    m = ac.audit(oracle, k0, k1, l, r, a, L, clients=bad)
    assert m["n_bad_clients"] == 3
    for ok, rep in ((ok_g, rep_g), (ok_s, rep_s)):
        assert_equals_model(ok, rep, m, shards)
        assert rep["n_checks"] == n * 2 * d * 5 * L
    with pytest.raises(fhh.FhhError, match="fhh error -1: .*multi-device"):
        g0.audit_keys_ball_device(g1, pts, delta)
    # drop three clients of the first shard (one of them bad): the later shards' bases leave the word boundary
    keep = np.ones(n, np.uint8)
    keep[[2, 10, 40]] = 0
    for c in (g0, g1, s0, s1):
        c.retain_clients(keep)
    info, _ = g0.shard_info()
    assert any(b % 64 for _, b, cnt in info if cnt)
    kept = np.flatnonzero(keep)
    ok_g, rep_g = g0.audit_keys_ball(g1, pts[kept], delta)
    ok_s, rep_s = s0.audit_keys_ball(s1, pts[kept], delta)
    assert np.array_equal(ok_g, m["ok"][kept]) and np.array_equal(ok_s, ok_g)
    assert rep_g["n_bad_clients"] == 2 and ac.report_first(rep_g) == ac.report_first(rep_s)
    assert rep_g["first_client"] == list(kept).index(70) and rep_g["n_checks"] == (n - 3) * 2 * d * 5 * L


# ---- refusals ----
def test_refusals_leave_the_ctxs_usable(oracle):
    import fuzzyheavyhitters_amd as fhh
    from fuzzyheavyhitters_amd import workload
    from fuzzyheavyhitters_amd._lib import FhhAuditReport, FhhBallSrc, ptr
    lib = fhh.lib()
    L, d, n, delta = 40, 1, 10, 8
    rng = np.random.default_rng(77)
    alpha = ac.population(rng, L, d, n, delta)
    pts = workload.pack_points(alpha)
    k0, k1, _ = ac.oracle_keys(oracle, rng, alpha, delta)
    c0, c1 = pair(fhh, L, d, k0, k1)
    ok = np.full(n + 5, 9, np.uint8)

    def call(a, b, count=n, form=0, ball=delta, points=pts, src=True, rep=True, dev=False):
        s = FhhBallSrc()
        s.form, s.ball = form, ball
        s.points = points.ctypes.data if points is not None else None
        report = FhhAuditReport()
        report.n_checks = 123
        if dev:
            p = ctypes.c_void_p(5)
            rc = lib.fhh_audit_keys_ball_device(a.handle, b.handle, count, ctypes.byref(s) if src else None,
                                                ctypes.byref(p) if dev == 1 else None, ctypes.byref(report) if rep else None)
            assert rc == 0 or p.value == 5
        else:
            rc = lib.fhh_audit_keys_ball(a.handle, b.handle, count, ctypes.byref(s) if src else None, ptr(ok),
                                         ctypes.byref(report) if rep else None)
        assert rc == 0 or report.n_checks == 123
        return rc

    def good():
        ok[:] = 9
        assert call(c0, c1) == 0 and ok[:n].all() and (ok[n:] == 9).all()
        assert call(c0, c1, dev=1) == 0

    good()
    carry = alpha.copy()
    carry[7, 0] = 1
    carry[4, 0] = bc.bits_of((1 << L) - delta, L)
    empty = fhh.KeyCollection(L, d)
    for refusal, want in (
            (lambda: call(c0, c1, count=n - 1), FHH_E_ARG),                                   # wrong n
            (lambda: call(c0, c1, count=n + 1, points=np.zeros((n + 1, d, 5), np.uint8)), FHH_E_ARG),
            (lambda: call(c0, fhh.KeyCollection(L, 2)), FHH_E_ARG),                           # differing d
            (lambda: call(fhh.KeyCollection(48, d), c1), FHH_E_ARG),                          # differing L
            (lambda: call(c0, empty), FHH_E_STATE),                                           # an empty ctx
            (lambda: call(empty, c1), FHH_E_STATE),
            (lambda: call(c0, c1, count=0), FHH_E_STATE),
            (lambda: call(c0, c1, src=False), FHH_E_ARG),                                     # NULL pointers
            (lambda: call(c0, c1, points=None), FHH_E_ARG),
            (lambda: call(c0, c1, rep=False), FHH_E_ARG),
            (lambda: call(c0, c1, dev=2), FHH_E_ARG),
            (lambda: call(c0, c1, dev=1, rep=False), FHH_E_ARG),
            (lambda: call(c0, c1, form=7), FHH_E_ARG),                                        # an unknown form
            (lambda: call(c0, c1, form=1, points=np.zeros((n, 2), np.int16)), FHH_E_ARG),
            (lambda: call(c0, c1, points=workload.pack_points(carry)), FHH_E_ARG)):           # a carry out
        ok[:] = 9
        assert refusal() == want
        assert (ok == 9).all()
        good()
    assert lib.fhh_audit_keys_ball(None, c1.handle, n, None, None, None) == FHH_E_ARG
    with pytest.raises(fhh.FhhError, match=r"fhh error -1: .*client 4, dim 0"):
        c0.audit_keys_ball(c1, workload.pack_points(carry), delta)
    with pytest.raises(fhh.FhhError, match="unknown form"):
        c0.audit_keys_ball(c1, pts, delta, form="polar")
    ms, div = ctypes.c_double(-1), ctypes.c_uint64(5)
    assert lib.fhh_audit_timing(c0.handle, ctypes.byref(ms)) == 0 and ms.value > 0
    assert lib.fhh_audit_seed_check(c0.handle, ctypes.byref(div)) == 0 and div.value == 0
    assert lib.fhh_audit_timing(c0.handle, None) == FHH_E_ARG and lib.fhh_audit_seed_check(None, ctypes.byref(div)) == FHH_E_ARG
    assert empty.num_clients() == 0


# ---- the leader ----
def test_the_leader_audits_every_chunk_and_yields_the_same_bytes(oracle, monkeypatch):
    """250 clients in chunks of 100: the same requests with and without the audit; a chunk that fails raises
    KeyAuditError, carrying the report, before any of its requests is yielded."""
    import fuzzyheavyhitters_amd as fhh
    from fuzzyheavyhitters_amd import leader, workload
    L, d, n, delta = 40, 2, 250, 8
    alpha = ac.population(np.random.default_rng(250), L, d, n, delta)
    pts = workload.pack_points(alpha)
    kw = dict(n_dims=d, data_len=L, seed=bc.SEED, batch=50, chunk=100)
    plain = list(leader.add_fuzzy_keys(pts, delta, **kw))
    audits = []
    real = fhh.KeyCollection.audit_keys_ball

    def counted(self, other, points, ball, form="bits"):
        ok, rep = real(self, other, points, ball, form=form)
        audits.append((len(points), rep["n_bad_clients"], rep["n_checks"]))
        return ok, rep

    monkeypatch.setattr(fhh.KeyCollection, "audit_keys_ball", counted)
    audited = list(leader.add_fuzzy_keys(pts, delta, audit=True, **kw))
    assert audits == [(100, 0, 100 * 2 * d * 5 * L), (100, 0, 100 * 2 * d * 5 * L), (50, 0, 50 * 2 * d * 5 * L)]
    assert len(plain) == len(audited) == 3
    for a, b in zip(plain, audited):
        for ra, rb in zip(a, b):
            assert len(ra) == len(rb) and all(np.array_equal(x, y) for x, y in zip(ra, rb))

    def second_chunk_fails(self, other, points, ball, form="bits"):
        ok, rep = real(self, other, points[::-1].copy(), ball, form=form) if len(audits) == 4 else \
            real(self, other, points, ball, form=form)
        audits.append(None)
        return ok, rep

    monkeypatch.setattr(fhh.KeyCollection, "audit_keys_ball", second_chunk_fails)
    gen = leader.add_fuzzy_keys(pts, delta, audit=True, **kw)
    first = next(gen)
    assert all(np.array_equal(x, y) for ra, rb in zip(first, plain[0]) for x, y in zip(ra, rb))
    with pytest.raises(fhh.KeyAuditError) as e:
        next(gen)
    assert e.value.first == 100 and e.value.report["n_bad_clients"] > 0 and e.value.ok.shape == (100,)
    assert e.value.report["first_client"] is not None
