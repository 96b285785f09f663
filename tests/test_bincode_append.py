"""The leader's add_keys RPCs as they arrive (leader.rs:391-415: batches of addkey_batch_size clients),
appended with fhh_add_keys_bincode_append and decoded on the GPU into their place: the span arithmetic on
the host, the keys and every crawl level against the oracle and against the one-shot fhh_add_keys_bincode
of the same population, rejected batches, state refusals, and the multi-device routing."""
import ctypes
import glob
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))


# ---- CPU ------------------------------------------------------------------------------------------
def test_bincode_span_host(tmp_path):
    """csrc/bincode_span.h: every destination (word, lane) of a batch is covered exactly once by the right
    source record, the tail-zero mask is the lanes after the batch in its last word, nothing before c0."""
    if not shutil.which("hipcc"):
        pytest.skip("hipcc not available")
    exe = tmp_path / "bincode_span"
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-O1", "-std=c++17",
                    os.path.join(ROOT, "tests", "host", "bincode_span_host_test.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "OK", out.stdout + out.stderr


def test_append_entry_points_refuse_null_ctx(fhh):
    lib = fhh.lib()
    buf = (ctypes.c_uint8 * 8)()
    assert lib.fhh_reserve_clients(None, 100) == -1            # FHH_E_ARG
    assert lib.fhh_add_keys_bincode_append(None, buf, 8) == -1
    assert lib.fhh_last_error(None)


# ---- GPU ------------------------------------------------------------------------------------------
_KEYS = {}


def keys_for(oracle, n, L, d):
    """Both servers' oracle keys of a seeded population, computed once per shape: every client's interval is
    [a - 1, a + 1] around one of 5 sites per dim (any L, also one that is no multiple of 8), bits MSB first."""
    if (n, L, d) not in _KEYS:
        rng = np.random.default_rng(1000 + n + L)
        sites = [[int.from_bytes(rng.bytes(16), "little") % ((1 << L) - 4) + 2 for _ in range(d)] for _ in range(5)]
        pick = rng.integers(0, 5, n)
        bits = np.zeros((2, n, d, L), np.uint8)
        for c in range(n):
            for j in range(d):
                for side, v in enumerate((sites[pick[c]][j] - 1, sites[pick[c]][j] + 1)):
                    bits[side, c, j] = [(v >> (L - 1 - b)) & 1 for b in range(L)]
        roots = rng.integers(0, 256, (n, d, 2, 2, 16), dtype=np.uint8)
        _KEYS[(n, L, d)] = oracle.gen_keys(bits[0], bits[1], roots)
    return _KEYS[(n, L, d)]


def request(k, a, b):
    from fuzzyheavyhitters_amd import workload
    return workload.add_keys_request_bincode(k.key_idx[a:b], k.root_seed[a:b], k.cw_seed[a:b], k.cw_bits[a:b])


def append_all(c, k, batches, start=0):
    a = start
    for m in batches:
        c.add_keys_bincode_append(request(k, a, a + m))
        a += m
        assert c.num_clients() == a
    return a


def assert_keys(c, k, n=None):
    ki, rs, cs, cb = c.export_keys()
    n = k.key_idx.shape[0] if n is None else n
    assert ki.shape[0] == n
    assert np.array_equal(ki, k.key_idx[:n]) and np.array_equal(rs, k.root_seed[:n])
    assert np.array_equal(cs, k.cw_seed[:n]), "cor_words seeds differ"
    assert np.array_equal(cb, k.cw_bits[:n]), "cor_words bits differ"


def crawl_equal(pair_a, pair_b, n, levels, thr=2):
    """The drop-in crawl on two builds of the same two servers, level by level: children, EvalStates and
    share planes equal at every level (pruned with pair_b's equality counts)."""
    from fuzzyheavyhitters_amd.collection import sim_eq_count
    for c in (*pair_a, *pair_b):
        c.tree_init()
    for lvl in range(levels):
        out = [c.tree_crawl(share_planes=True) for c in (*pair_a, *pair_b)]
        C = out[2][0]
        assert all(o[0] == C for o in out)
        for s in range(2):
            assert np.array_equal(out[s][1], out[2 + s][1]), f"share planes differ, level {lvl} server {s}"
            for x, y in zip(pair_a[s].export_states(), pair_b[s].export_states()):
                assert np.array_equal(x, y), f"EvalStates differ, level {lvl} server {s}"
        cnt = sim_eq_count(pair_b[0], pair_b[1], C)
        assert np.array_equal(cnt, sim_eq_count(pair_a[0], pair_a[1], C))
        keep = cnt >= thr
        for c in (*pair_a, *pair_b):
            c.tree_prune(keep)
        if not keep.any():
            break


CASES = [
    # a one-client batch at lane 0, one ending on lane 62, one filling the word's last lane, a whole aligned
    # word, a batch inside one word, one over three words ending mid-word; L = 40: a partial level block;
    # unreserved, the layout grows at clients 65 and 129
    (200, 40, 1, [1, 62, 1, 64, 5, 67]),
    (130, 104, 2, [100, 30]),     # the reference's batch size, d = 2, four level blocks (the last partial)
    (64, 32, 1, [64]),
    (65, 33, 1, [64, 1]),
]


@pytest.mark.gpu
@pytest.mark.parametrize("reserve", [None, "n"], ids=["unreserved", "reserved"])
@pytest.mark.parametrize("n,L,d,batches", CASES, ids=[f"n{c[0]}_L{c[1]}_d{c[2]}" for c in CASES])
def test_appended_keys_equal_oracle(oracle, n, L, d, batches, reserve):
    import fuzzyheavyhitters_amd as fhh
    assert sum(batches) == n
    for k in keys_for(oracle, n, L, d):      # server 0's key_idx bits are all 0, server 1's all 1
        c = fhh.KeyCollection(L, d)
        if reserve:
            c.reserve_clients(n)
        a = 0
        for m in batches:
            c.add_keys_bincode_append(request(k, a, a + m))
            a += m
            assert c.num_clients() == a
            assert_keys(c, k, a)             # export works between appends
        assert_keys(c, k)
        c.tree_init()
        assert_keys(c, k)
        assert c.num_clients() == n


@pytest.mark.gpu
@pytest.mark.parametrize("reserved", [1000, 100], ids=["over-reserved", "under-reserved"])
def test_appended_keys_reservation_off_the_count(oracle, reserved):
    """200 clients on a reservation of 1000 (compacted at tree_init) and of 100 (which still grows)."""
    import fuzzyheavyhitters_amd as fhh
    n, L, d, batches = CASES[0]
    k0, _ = keys_for(oracle, n, L, d)
    c = fhh.KeyCollection(L, d)
    c.reserve_clients(reserved)
    append_all(c, k0, batches)
    assert_keys(c, k0)
    c.tree_init()
    assert_keys(c, k0)


@pytest.mark.gpu
@pytest.mark.parametrize("reserve", [None, 200, 1000], ids=["unreserved", "reserved", "over-reserved"])
def test_appended_crawl_equals_one_shot(oracle, reserve):
    """An append-built and a one-shot-built collection through the same drop-in crawl: garbage in the pad
    lanes or a stale `valid` word would show in the share planes / EvalStates."""
    import fuzzyheavyhitters_amd as fhh
    n, L, d, batches = CASES[0]
    ks = keys_for(oracle, n, L, d)
    app, one = [], []
    for k in ks:
        c = fhh.KeyCollection(L, d)
        if reserve:
            c.reserve_clients(reserve)
        append_all(c, k, batches)
        app.append(c)
        o = fhh.KeyCollection(L, d)
        o.add_keys_bincode(request(k, 0, n))
        one.append(o)
    crawl_equal(app, one, n, L)


@pytest.mark.gpu
def test_appended_golden_crawl(oracle):
    """The fixture of test_bincode_keys_equal_oracle_and_crawl, appended in batches of 100 to both servers."""
    import fuzzyheavyhitters_amd as fhh
    path = sorted(glob.glob(os.path.join(HERE, "golden", "zipf_d2_*.npz")))[0]
    g = np.load(path, allow_pickle=False)
    n, d, L, _, _ = [int(x) for x in g["meta"]]
    cs = []
    for k in oracle.gen_keys(g["left"], g["right"], g["root_seeds"]):
        c = fhh.KeyCollection(L, d)
        a = 0
        while a < n:
            m = min(100, n - a)
            c.add_keys_bincode_append(request(k, a, a + m))
            a += m
        assert_keys(c, k)
        cs.append(c)
    res = fhh.sim_crawl(cs[0], cs[1], float(g["threshold"][0]), mode=str(g["mode"][0]), prf_seed=77)
    assert np.array_equal(res.level_children, g["level_children"])
    assert np.array_equal(np.concatenate(res.counts), g["counts"])


def bad_batches(k, a, m, L):
    """The four malformed requests of test_bincode_malformed_rejected, their offsets re-derived for the batch
    of clients [a, a + m) (d = 1). The bool byte sits on a (client, level) whose true bits.1 is 0 and is 3:
    the decode sets that plane bit, in the word the batch shares with the clients before it, before the
    request is refused."""
    good = request(k, a, a + m)
    KB = 25 + 20 * L
    R = 8 + 2 * KB
    i, lv = [(int(i), int(lv)) for i, lv in zip(*np.nonzero((k.cw_bits[a:a + m, 0, 1, :] >> 1 & 1) == 0))][3]
    bad = {"truncated": good[:-1], "bool": good.copy(), "L": good.copy(), "d": good.copy()}
    bad["bool"][8 + i * R + 8 + KB + 25 + 20 * lv + 17] = 3    # client i of the batch, right key, level lv, bits.1
    bad["L"][8 + 9 * R + 8 + 17] = L - 1                       # client 9 of the batch, left key: cor_words len
    bad["d"][8 + (m - 1) * R] = 2                              # the batch's last client: inner vec len
    return bad


@pytest.mark.gpu
@pytest.mark.parametrize("reserve", [None, 70], ids=["unreserved", "reserved"])
def test_rejected_batch_leaves_no_trace(oracle, reserve):
    import fuzzyheavyhitters_amd as fhh
    n, L, d = 70, 40, 1
    k0, _ = keys_for(oracle, n, L, d)
    for name, buf in bad_batches(k0, 30, 25, L).items():
        c = fhh.KeyCollection(L, d)
        if reserve:
            c.reserve_clients(reserve)
        append_all(c, k0, [30])
        with pytest.raises(fhh.FhhError):
            c.add_keys_bincode_append(buf)
        assert c.num_clients() == 30, name
        assert_keys(c, k0, 30)
        append_all(c, k0, [25, 15], start=30)
        assert_keys(c, k0)
        c.tree_init()
        assert_keys(c, k0)


@pytest.mark.gpu
def test_rejected_last_batch_leaves_zero_pad_lanes(oracle):
    """A refused batch that is the last thing before tree_init: the lanes it wrote past the 30 clients held
    are zero again, so the crawl equals that of a one-shot collection of the 30."""
    import fuzzyheavyhitters_amd as fhh
    n, L, d = 70, 40, 1
    ks = keys_for(oracle, n, L, d)
    app, one = [], []
    for k in ks:
        c = fhh.KeyCollection(L, d)
        append_all(c, k, [30])
        with pytest.raises(fhh.FhhError):
            c.add_keys_bincode_append(bad_batches(k, 30, 25, L)["bool"])
        app.append(c)
        o = fhh.KeyCollection(L, d)
        o.add_keys_bincode(request(k, 0, 30))
        one.append(o)
    crawl_equal(app, one, 30, 6, thr=1)


@pytest.mark.gpu
def test_append_state_refusals(oracle):
    import fuzzyheavyhitters_amd as fhh
    from fuzzyheavyhitters_amd import workload
    n, L, d = 70, 40, 1
    k0, _ = keys_for(oracle, n, L, d)
    batch = request(k0, 0, 30)

    c = fhh.KeyCollection(L, d)                       # append after tree_init
    c.add_keys_bincode_append(batch)
    c.tree_init()
    with pytest.raises(fhh.FhhError):
        c.add_keys_bincode_append(request(k0, 30, 55))
    with pytest.raises(fhh.FhhError):
        c.reserve_clients(100)
    c.reset()                                         # reset drops appended keys and the reservation
    assert c.num_clients() == 0
    append_all(c, k0, [30, 25, 15])
    assert_keys(c, k0)

    c = fhh.KeyCollection(L, d)                       # onto fhh_add_keys keys
    c.add_keys(k0.key_idx[:30], k0.root_seed[:30], k0.cw_seed[:30], k0.cw_bits[:30])
    with pytest.raises(fhh.FhhError):
        c.add_keys_bincode_append(batch)

    wl = workload.zipf_workload(30, L, d, num_sites=3, seed=5)   # onto gen_keys_pair keys
    g0, g1 = fhh.KeyCollection(L, d), fhh.KeyCollection(L, d)
    fhh.gen_keys_pair(g0, g1, wl.left, wl.right, wl.root_seeds)
    with pytest.raises(fhh.FhhError):
        g0.add_keys_bincode_append(batch)

    c = fhh.KeyCollection(L, d)                       # onto one-shot keys
    c.add_keys_bincode(batch)
    with pytest.raises(fhh.FhhError):
        c.add_keys_bincode_append(request(k0, 30, 55))

    c = fhh.KeyCollection(L, d)                       # a one-shot call / add_keys onto appended keys
    c.add_keys_bincode_append(batch)
    with pytest.raises(fhh.FhhError):
        c.add_keys_bincode(batch)
    with pytest.raises(fhh.FhhError):
        c.add_keys(k0.key_idx[:30], k0.root_seed[:30], k0.cw_seed[:30], k0.cw_bits[:30])
    with pytest.raises(fhh.FhhError):                 # a reservation below the current count
        c.reserve_clients(29)
    assert c.num_clients() == 30
    assert_keys(c, k0, 30)


@pytest.mark.gpu
@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0]], ids=["2-shards", "3-shards"])
def test_append_multi_device(oracle, devices):
    import fuzzyheavyhitters_amd as fhh
    n, L, d = 200, 40, 1
    batches = [50, 30, 40, 20, 60]                    # 50..80 straddles client 64, 120..140 client 128
    ends = np.cumsum(batches)
    for b, cnt in fhh.shard_plan(n, len(devices))[1:]:
        assert cnt and b not in ends and b < n, "a batch must straddle every shard boundary"
    ks = keys_for(oracle, n, L, d)
    grp, one = [], []
    for k in ks:
        g = fhh.KeyCollection(L, d, devices=devices)
        with pytest.raises(fhh.FhhError):             # no reservation
            g.add_keys_bincode_append(request(k, 0, 50))
        g.reserve_clients(n)
        a = 0
        for m in batches:
            g.add_keys_bincode_append(request(k, a, a + m))
            a += m
            assert g.num_clients() == a
            assert_keys(g, k, a)
        with pytest.raises(fhh.FhhError):             # the 201st client
            g.add_keys_bincode_append(request(k, 0, 1))
        assert_keys(g, k)
        grp.append(g)
        c = fhh.KeyCollection(L, d)
        append_all(c, k, batches)
        one.append(c)
    # every level's share planes equal the one-GPU appended collection's
    from fuzzyheavyhitters_amd.collection import sim_eq_count
    for c in (*grp, *one):
        c.tree_init()
    for lvl in range(10):
        out = [c.tree_crawl(share_planes=True) for c in (*grp, *one)]
        C = out[2][0]
        for s in range(2):
            assert out[s][0] == C
            assert np.array_equal(out[s][1], out[2 + s][1]), f"share planes differ, level {lvl} server {s}"
        keep = sim_eq_count(one[0], one[1], C) >= 2
        for c in (*grp, *one):
            c.tree_prune(keep)
        if not keep.any():
            break
    assert_keys(grp[0], ks[0])


@pytest.mark.gpu
def test_append_multi_device_short_of_reservation_and_rejects(oracle):
    import fuzzyheavyhitters_amd as fhh
    n, L, d = 200, 40, 1
    k0, _ = keys_for(oracle, n, L, d)
    g = fhh.KeyCollection(L, d, devices=[0, 0])
    g.reserve_clients(n)
    append_all(g, k0, [50, 60])
    # a batch over the shard boundary at client 128, malformed in its second shard's slice: no shard advances
    bad = request(k0, 110, 150)
    KB = 25 + 20 * L
    bad[8 + 30 * (8 + 2 * KB) + 8 + 17] = L + 1       # client 140: cor_words len
    with pytest.raises(fhh.FhhError):
        g.add_keys_bincode_append(bad)
    assert g.num_clients() == 110
    assert_keys(g, k0, 110)
    append_all(g, k0, [40, 49], start=110)
    with pytest.raises(fhh.FhhError):                 # tree_init at 199 of 200
        g.tree_init()
    append_all(g, k0, [1], start=199)
    assert_keys(g, k0)
    g.tree_init()
    assert_keys(g, k0)
