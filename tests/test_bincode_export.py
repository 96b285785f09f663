"""Device keys out as the leader's add_keys RPCs (fhh_export_keys_bincode, the inverse of fhh_add_keys_bincode /
fhh_add_keys_bincode_append): the span arithmetic on the host, sizes, refusals and the kernel's resources on
the CPU; on the GPU the bytes against `workload.add_keys_request_bincode` of the oracle's keys (never against
the code under test), for every kind of range, batch, level-block edge, source of the keys, ctx state and
shard cut, and the round trip export -> append -> crawl."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from kernel_usage import resource_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CW_KERNEL = "_ZN3fhh17k_bincode_emit_cwEPK15HIP_vector_typeIjLj4EEPKmPhNS_8EmitArgsE"
FHH_E_ARG, FHH_E_STATE = -1, -2


# ---- CPU ------------------------------------------------------------------------------------------
def test_bincode_emit_host(tmp_path):
    """csrc/bincode_emit.h: replayed as the kernels cut the output, every byte of [0, len) has exactly one
    writer (request count, client d, key header, or one CW segment's head / interior / tail), interior
    dwords are aligned and unshared, nothing falls outside [0, len), shard slices tile the output."""
    if not shutil.which("hipcc"):
        pytest.skip("hipcc not available")
    exe = tmp_path / "bincode_emit"
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-O1", "-std=c++17",
                    os.path.join(ROOT, "tests", "host", "bincode_emit_host_test.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "OK", out.stdout + out.stderr


def fake_keys(rng, n, d, L):
    return (rng.integers(0, 2, (n, d, 2), dtype=np.uint8), rng.integers(0, 256, (n, d, 2, 16), dtype=np.uint8),
            rng.integers(0, 256, (n, d, 2, L, 16), dtype=np.uint8), rng.integers(0, 16, (n, d, 2, L), dtype=np.uint8))


def requests_of(keys, first, count, batch):
    """The expected requests of clients [first, first + count) in batches of `batch` (0: one), each serialized by
    the numpy serializer that is pinned to the reference's key size and to the decoder."""
    from fuzzyheavyhitters_amd import workload
    B = batch or count
    return [workload.add_keys_request_bincode(*[x[a:min(a + B, first + count)] for x in keys])
            for a in range(first, first + count, B)]


def test_request_bytes_equal_the_serializer(fhh):
    lib = fhh.lib()
    rng = np.random.default_rng(5)
    got = ctypes.c_uint64()
    for d in (1, 2, 3, 4):
        for L in (1, 31, 32, 33, 104):
            keys = fake_keys(rng, 23, d, L)
            for count in (1, 7, 22, 23):
                for batch in (0, 1, 7, count, count + 1, 100):
                    want = sum(r.size for r in requests_of(keys, 0, count, batch))
                    assert lib.fhh_bincode_request_bytes(d, L, count, batch, ctypes.byref(got)) == 0
                    assert got.value == want, (d, L, count, batch)
    # the metric's shape, by the formula: 1M clients, L = 512, batches of 100
    assert lib.fhh_bincode_request_bytes(1, 512, 10 ** 6, 100, ctypes.byref(got)) == 0
    assert got.value == 8 * 10 ** 4 + 10 ** 6 * (8 + 2 * (25 + 20 * 512))


def test_split_add_keys_requests():
    from fuzzyheavyhitters_amd import workload
    keys = fake_keys(np.random.default_rng(6), 23, 2, 9)
    for batch in (0, 1, 7, 23, 100):
        want = requests_of(keys, 3, 20, batch)
        got = workload.split_add_keys_requests(np.concatenate(want), 2, 9)
        assert len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want))
    with pytest.raises(ValueError):
        workload.split_add_keys_requests(np.concatenate(want)[:-1], 2, 9)


def test_export_entry_points_refuse_null_ctx_and_bad_shapes(fhh):
    lib = fhh.lib()
    n = ctypes.c_uint64(77)
    buf = (ctypes.c_uint8 * 64)()
    assert lib.fhh_export_keys_bincode(None, 0, 1, 0, buf, 64, ctypes.byref(n)) == FHH_E_ARG
    assert lib.fhh_last_error(None)
    for d, L, count in ((0, 40, 1), (5, 40, 1), (1, 0, 1), (1, 40, 0)):
        assert lib.fhh_bincode_request_bytes(d, L, count, 0, ctypes.byref(n)) == FHH_E_ARG, (d, L, count)
    assert lib.fhh_bincode_request_bytes(1, 40, 1, 0, None) == FHH_E_ARG
    assert n.value == 77


def test_emit_cw_kernel_does_not_spill():
    """k_bincode_emit_cw keeps a tile's 8 seed rows per lane in flight before the first LDS write; its LDS is the
    64 x 161-dword stage of the decoder."""
    usage = resource_usage("fhh_bincode_out.hip")
    assert CW_KERNEL in usage, sorted(usage)
    k = usage[CW_KERNEL]
    assert k["ScratchSize [bytes/lane]"] == "0", k
    assert k["VGPRs Spill"] == "0", k
    assert int(k["LDS Size [bytes/block]"]) == 64 * 161 * 4, k


# ---- GPU ------------------------------------------------------------------------------------------
_KEYS = {}


def keys_for(oracle, n, L, d):
    """Both servers' oracle keys of a seeded zipf population, once per shape (L < 40: the keys of the intervals'
    L-bit prefixes, which stay ordered)."""
    if (n, L, d) not in _KEYS:
        from fuzzyheavyhitters_amd import workload
        wl = workload.zipf_workload(n, max(L, 40), d, num_sites=5, seed=900 + n + L)
        left, right = (np.ascontiguousarray(x[:, :, :L]) for x in (wl.left, wl.right))
        _KEYS[(n, L, d)] = (oracle.gen_keys(left, right, wl.root_seeds), (left, right, wl.root_seeds))
    return _KEYS[(n, L, d)][0]


def fields(k):
    return k.key_idx, k.root_seed, k.cw_seed, k.cw_bits


def expected(k, first, count, batch):
    return np.concatenate(requests_of(fields(k), first, count, batch))


def one_shot(k, L, d, **kw):
    import fuzzyheavyhitters_amd as fhh
    from fuzzyheavyhitters_amd import workload
    c = fhh.KeyCollection(L, d, **kw)
    c.add_keys_bincode(workload.add_keys_request_bincode(*fields(k)))
    return c


def assert_export(c, k, first, count, batch):
    """Byte-exact against the expected requests. The ctx's staging buffer keeps the last export's bytes, so an
    export with other offsets (another batch size; for one client its neighbour) comes first: a byte the kernels
    leave unwritten then shows as a stale one, also where an equal export went before. The host buffer is
    pre-filled for the same reason."""
    import fuzzyheavyhitters_amd as fhh
    if count > 1:
        c.export_keys_bincode(first, count, 2 if batch == 1 else 1)
    else:
        c.export_keys_bincode(first - 1 if first else first + 1, 1, 0)
    want = expected(k, first, count, batch)
    got = np.full(want.size + 8, 0xA5, np.uint8)
    ln = ctypes.c_uint64()
    fhh._lib.check(fhh.lib().fhh_export_keys_bincode(c.handle, first, count, batch, fhh._lib.ptr(got), want.size,
                                                     ctypes.byref(ln)), c.handle)
    assert ln.value == want.size and (got[want.size:] == 0xA5).all(), (first, count, batch)
    got = got[:want.size]
    if not np.array_equal(got, want):
        bad = np.nonzero(got != want)[0]
        raise AssertionError(f"first {first} count {count} batch {batch}: {bad.size} bytes differ, the first at {bad[:8]}")


RANGES = [(0, 200), (0, 1), (1, 62), (63, 1), (63, 2), (64, 64), (5, 130), (199, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("server", [0, 1])
def test_export_ranges_and_batches(oracle, server):
    """n = 200, L = 40 (a partial level block), d = 1: ranges that start and end on every kind of lane, each in
    one request, single clients, sevens and hundreds; byte-exact. Client parity and key side give all four byte
    alignments of a segment."""
    n, L, d = 200, 40, 1
    k = keys_for(oracle, n, L, d)[server]
    c = one_shot(k, L, d)
    assert {(8 * (i // B + 1) + i * (8 + 2 * (25 + 20 * L)) + 8 + kk * (25 + 20 * L) + 25) % 4
            for B in (1, 200) for i in range(4) for kk in range(2)} == {0, 1, 2, 3}
    for first, count in RANGES:
        for batch in (0, 1, 7, 100):
            assert_export(c, k, first, count, batch)
    assert np.array_equal(c.export_keys_bincode(), expected(k, 0, n, 0))          # the defaults: everything, one request
    assert np.array_equal(c.export_keys_bincode(190, batch=4), expected(k, 190, 10, 4))


@pytest.mark.gpu
def test_export_d2_four_level_blocks(oracle):
    """n = 130, L = 104, d = 2: four level blocks with the last partial, three words with two clients in the last,
    four keys per client, the reference's batch size."""
    n, L, d = 130, 104, 2
    for k in keys_for(oracle, n, L, d):
        c = one_shot(k, L, d)
        for batch in (100, 0):
            assert_export(c, k, 0, n, batch)
        assert_export(c, k, 127, 3, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("L", [1, 31, 32, 33])
def test_export_level_block_edges(oracle, L):
    """n = 65, d = 1 at the level-block edges; L = 1 is a 45-byte key whose one segment is 20 bytes."""
    n, d = 65, 1
    for k in keys_for(oracle, n, L, d):
        c = one_shot(k, L, d)
        for first, count, batch in ((0, n, 0), (0, n, 7), (63, 2, 1), (1, 64, 100)):
            assert_export(c, k, first, count, batch)


@pytest.mark.gpu
def test_export_the_real_record(oracle):
    """n = 70, L = 512, d = 1: 10 265 B per key, 16 level blocks; the whole population."""
    n, L, d = 70, 512, 1
    for k in keys_for(oracle, n, L, d):
        c = one_shot(k, L, d)
        assert_export(c, k, 0, n, 0)
        assert_export(c, k, 0, n, 100)
        assert_export(c, k, 3, 66, 7)


def crawl_equal(pair_a, pair_b, levels, thr=2, after_init=None):
    """The drop-in crawl on two builds of the same two servers, level by level: children, EvalStates and share
    planes equal at every level (the shape of test_bincode_append.crawl_equal)."""
    from fuzzyheavyhitters_amd.collection import sim_eq_count
    for c in (*pair_a, *pair_b):
        c.tree_init()
    if after_init:
        after_init()
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


@pytest.mark.gpu
def test_export_of_generated_keys_round_trip(oracle):
    """fhh_gen_keys_pair -> export in batches of 100 -> the splitter -> add_keys_bincode_append on fresh
    collections: the same keys, and the same crawl."""
    import fuzzyheavyhitters_amd as fhh
    from fuzzyheavyhitters_amd import workload
    n, L, d = 230, 40, 1
    wl = workload.zipf_workload(n, L, d, num_sites=4, seed=31)
    src = [fhh.KeyCollection(L, d), fhh.KeyCollection(L, d)]
    fhh.gen_keys_pair(src[0], src[1], wl.left, wl.right, wl.root_seeds)
    ks = oracle.gen_keys(wl.left, wl.right, wl.root_seeds)
    dst = []
    for s in range(2):
        buf = src[s].export_keys_bincode(batch=100)
        assert np.array_equal(buf, expected(ks[s], 0, n, 100))
        reqs = workload.split_add_keys_requests(buf, d, L)
        assert [int(r[:8].view("<u8")[0]) for r in reqs] == [100, 100, 30]
        c = fhh.KeyCollection(L, d)
        for r in reqs:
            c.add_keys_bincode_append(r)
        assert c.num_clients() == n
        dst.append(c)

    def same_keys():
        for a, b in zip(src, dst):
            for x, y in zip(a.export_keys(), b.export_keys()):
                assert np.array_equal(x, y)

    crawl_equal(dst, src, 8, after_init=same_keys)


@pytest.mark.gpu
def test_export_ctx_states(oracle):
    import fuzzyheavyhitters_amd as fhh
    from fuzzyheavyhitters_amd import workload
    n, L, d = 200, 40, 1
    k0, _ = keys_for(oracle, n, L, d)
    lib = fhh.lib()
    out = np.zeros(64, np.uint8)
    got = ctypes.c_uint64()

    c = fhh.KeyCollection(L, d)                       # an empty ctx
    assert lib.fhh_export_keys_bincode(c.handle, 0, 1, 0, fhh._lib.ptr(out), out.size, ctypes.byref(got)) == FHH_E_STATE
    with pytest.raises(fhh.FhhError):
        c.export_keys_bincode(0, 1)

    # appended, unreserved: after 1 + 62 + 1 + 64 + 5 clients the layout's capacity stride (256 clients) is not
    # the exact one (192); then the rest, and again after tree_init's compaction
    a = 0
    for m in (1, 62, 1, 64, 5):
        c.add_keys_bincode_append(workload.add_keys_request_bincode(*[x[a:a + m] for x in fields(k0)]))
        a += m
    assert a == 133
    for first, count, batch in ((0, 133, 0), (5, 128, 7), (132, 1, 0)):
        assert_export(c, k0, first, count, batch)
    with pytest.raises(fhh.FhhError):                 # clients the ctx does not hold yet
        c.export_keys_bincode(0, 134)
    c.add_keys_bincode_append(workload.add_keys_request_bincode(*[x[133:] for x in fields(k0)]))
    assert_export(c, k0, 0, n, 100)
    c.tree_init()
    assert_export(c, k0, 0, n, 100)
    assert_export(c, k0, 63, 130, 7)

    c = fhh.KeyCollection(L, d)                       # host-staged fhh_add_keys keys: on the device after tree_init
    c.add_keys(*fields(k0))
    assert lib.fhh_export_keys_bincode(c.handle, 0, 1, 0, fhh._lib.ptr(out), out.size, ctypes.byref(got)) == FHH_E_STATE
    with pytest.raises(fhh.FhhError):
        c.export_keys_bincode()
    c.tree_init()
    assert_export(c, k0, 0, n, 0)
    assert_export(c, k0, 5, 130, 100)


@pytest.mark.gpu
def test_export_between_the_levels_of_a_crawl(oracle):
    """An export between levels 2 and 3 (frontier pruned) and one with level 4's children pending: the crawl goes
    on as an undisturbed twin's does, to the same surviving paths."""
    from fuzzyheavyhitters_amd.collection import sim_eq_count
    n, L, d = 200, 40, 1
    ks = keys_for(oracle, n, L, d)
    a = [one_shot(k, L, d) for k in ks]
    b = [one_shot(k, L, d) for k in ks]
    for c in (*a, *b):
        c.tree_init()
    keeps = ([], [])
    for lvl in range(L - 1):
        if lvl == 3:
            for s in range(2):
                assert_export(a[s], ks[s], 5, 130, 7)
        out = [c.tree_crawl(share_planes=True) for c in (*a, *b)]
        if lvl == 4:
            for s in range(2):
                assert_export(a[s], ks[s], 0, n, 100)
        C = out[0][0]
        assert all(o[0] == C for o in out), f"children differ, level {lvl}"
        for s in range(2):
            assert np.array_equal(out[s][1], out[2 + s][1]), f"share planes differ, level {lvl} server {s}"
            for x, y in zip(a[s].export_states(), b[s].export_states()):
                assert np.array_equal(x, y), f"EvalStates differ, level {lvl} server {s}"
        for pair, kept in ((a, keeps[0]), (b, keeps[1])):   # each pair pruned by its own counts
            keep = sim_eq_count(pair[0], pair[1], C) >= 2
            kept.append(keep)
            for c in pair:
                c.tree_prune(keep)
        assert np.array_equal(keeps[0][-1], keeps[1][-1]), f"kept children differ, level {lvl}"
        assert a[0].frontier_size() == b[0].frontier_size()
        if not keeps[1][-1].any():
            break
    assert len(keeps[1]) > 5 and keeps[1][-1].any(), "the crawl must outlive the exports"
    assert a[0].stats()["levels"] == b[0].stats()["levels"]


@pytest.mark.gpu
def test_export_refusals_leave_out_untouched(oracle):
    import fuzzyheavyhitters_amd as fhh
    n, L, d = 200, 40, 1
    k0, _ = keys_for(oracle, n, L, d)
    c = one_shot(k0, L, d)
    lib, ptr = fhh.lib(), fhh._lib.ptr
    need = expected(k0, 0, n, 7).size
    out = np.full(need + 16, 0xA5, np.uint8)
    got = ctypes.c_uint64()
    # cap one byte short; first + count = n + 1; count = 0
    for first, count, cap, sets_len in ((0, n, need - 1, need), (1, n, out.size, None), (0, 0, out.size, None)):
        got.value = 0
        assert lib.fhh_export_keys_bincode(c.handle, first, count, 7, ptr(out), cap, ctypes.byref(got)) == FHH_E_ARG
        assert (out == 0xA5).all(), (first, count, cap)
        if sets_len is not None:
            assert got.value == sets_len
    assert lib.fhh_export_keys_bincode(c.handle, 0, n, 7, None, need, ctypes.byref(got)) == FHH_E_ARG
    assert lib.fhh_export_keys_bincode(c.handle, 0, n, 7, ptr(out), out.size, None) == FHH_E_ARG
    assert (out == 0xA5).all()
    # and the exact cap works, writing nothing past len
    assert lib.fhh_export_keys_bincode(c.handle, 0, n, 7, ptr(out), need, ctypes.byref(got)) == 0
    assert got.value == need and np.array_equal(out[:need], expected(k0, 0, n, 7)) and (out[need:] == 0xA5).all()


@pytest.mark.gpu
@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0]], ids=["2-shards", "3-shards"])
def test_export_multi_device(oracle, devices):
    """n = 200 over 2 and 3 shards of one GPU: ranges and batches that straddle the shard boundaries, with the
    batch edges off the shard edges, give the one-GPU bytes (= the expected requests)."""
    import fuzzyheavyhitters_amd as fhh
    n, L, d = 200, 40, 1
    ks = keys_for(oracle, n, L, d)
    bounds = [b for b, cnt in fhh.shard_plan(n, len(devices))[1:]]
    assert bounds and all(0 < b < n for b in bounds)
    for k in ks:
        g = one_shot(k, L, d, devices=devices)
        for first, count, batch in ((0, n, 0), (0, n, 100), (0, n, 7), (5, 190, 50), (bounds[0] - 1, 2, 0),
                                    (bounds[0] - 1, 2, 1), (bounds[0], 1, 0), (bounds[-1] - 3, 70, 9), (63, 137, 30)):
            for b in bounds:                          # where a range crosses a boundary, its batch edges are not on it
                if batch and first < b < first + count:
                    assert batch == 1 or (b - first) % batch, (first, count, batch, b)
            assert_export(g, k, first, count, batch)
    # appended over the shards (each fills its reserved range), exported before and after tree_init
    from fuzzyheavyhitters_amd import workload
    g = fhh.KeyCollection(L, d, devices=devices)
    g.reserve_clients(n)
    for r in workload.split_add_keys_requests(expected(ks[0], 0, n, 30), d, L)[:5]:
        g.add_keys_bincode_append(r)
    assert_export(g, ks[0], 3, 147, 40)
    with pytest.raises(fhh.FhhError):
        g.export_keys_bincode(0, 151)
    for r in workload.split_add_keys_requests(expected(ks[0], 150, 50, 30), d, L):
        g.add_keys_bincode_append(r)
    g.tree_init()
    assert_export(g, ks[0], 0, n, 100)
    # staged fhh_add_keys keys of a multi-device ctx: refused until tree_init has placed them
    g = fhh.KeyCollection(L, d, devices=devices)
    g.add_keys(*fields(ks[1]))
    with pytest.raises(fhh.FhhError):
        g.export_keys_bincode()
    g.tree_init()
    assert_export(g, ks[1], 0, n, 100)
