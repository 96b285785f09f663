"""fhh_retain_clients_device on the GPU: the keep mask stays in device memory. The reference of every comparison is
the host call, pinned by test_retain_clients.py: a twin pair made from the same workload, brought to the same
frontier and given fhh_retain_clients with the numpy AND of the mask's rows — never the device call against itself;
counts are checked against a brute-force recount over the survivors. The shapes are test_retain_clients.py's."""
import ctypes
import functools

import numpy as np
import pytest

from retain_cases import children_of, masks, recount

pytestmark = pytest.mark.gpu

FHH_E_ARG, FHH_E_STATE = -1, -2
L16 = 16
PRF = 7
N = 130


@functools.lru_cache(maxsize=None)
def _workload(n, d, L=L16, seed=0):
    """A seeded Zipf workload of 4 sites cut to L levels; read-only."""
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


def _crawl_to(pairs, k, thr):
    """Every pair to depth k with the first pair's keep decisions."""
    from fuzzyheavyhitters_amd.collection import sim_eq_count
    cs = [c for p in pairs for c in p]
    for c in cs:
        c.tree_init()
    for _ in range(k):
        C = [c.tree_crawl()[0] for c in cs][0]
        keep = sim_eq_count(*pairs[0], C) >= thr
        assert keep.sum() >= 2, "the threshold keeps several nodes per level"
        for c in cs:
            c.tree_prune(keep)


def _dev(a):
    """A numpy mask as a tensor on the GPU (a tensor, e.g. a strided view, is passed on)."""
    import torch
    if isinstance(a, torch.Tensor):
        return a
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _twins_equal(a, b, what="", init=True):
    """num_clients, export_keys and — on an initialised pair — export_keys_bincode, frontier_paths and export_states
    of pair a equal pair b's, bit for bit, on both servers."""
    for s, (x, y) in enumerate(zip(a, b)):
        assert x.num_clients() == y.num_clients(), f"{what}: server {s} num_clients"
        for g, w, name in zip(x.export_keys(), y.export_keys(), ("key_idx", "root_seed", "cw_seed", "cw_bits")):
            assert np.array_equal(g, w), f"{what}: server {s} {name}"
        if not init:
            continue
        assert np.array_equal(x.export_keys_bincode(batch=50), y.export_keys_bincode(batch=50)), f"{what}: server {s} bincode"
        assert np.array_equal(x.frontier_paths(), y.frontier_paths()), f"{what}: server {s} frontier_paths"
        for g, w, name in zip(x.export_states(), y.export_states(), ("seed", "t", "y")):
            assert g.shape == w.shape and np.array_equal(g, w), f"{what}: server {s} {name} states"


def _lockstep(a, b, left, right, thr):
    """Both pairs crawl from their (equal) frontier to the end: the share planes, counts, last-level sums and final
    shares are equal, and the counts are the recount over the survivors."""
    import fuzzyheavyhitters_amd as fhh
    from fuzzyheavyhitters_amd.collection import sim_eq_count, sim_ot_sums
    n, d, L = left.shape
    cs = (a[0], a[1], b[0], b[1])
    assert all(c.num_clients() == n for c in cs)
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
        assert np.array_equal(outs[0][1], outs[2][1]) and np.array_equal(outs[1][1], outs[3][1]), f"planes level {lv}"
        ca, cb = sim_eq_count(a[0], a[1], C), sim_eq_count(b[0], b[1], C)
        assert np.array_equal(ca, cb), f"counts level {lv}"
        assert np.array_equal(ca, recount(left, right, children_of(parents, d))), f"recount level {lv}"
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


def _survivors(wl, n_keep, seed):
    """A mask with n_keep survivors, drawn among the heaviest site's clients first."""
    n = wl.left.shape[0]
    rng = np.random.default_rng(seed)
    site = np.bincount(wl.site_of_client).argmax()
    order = np.concatenate([rng.permutation(np.flatnonzero(wl.site_of_client == site)),
                            rng.permutation(np.flatnonzero(wl.site_of_client != site))])
    keep = np.zeros(n, np.uint8)
    keep[order[:n_keep]] = 1
    return keep


def _retain_both(a, b, keep, rows=None):
    """Pair a: retain_clients_device of the mask on the GPU (`rows`: a [rows, n] mask whose AND is `keep`); pair b:
    retain_clients of `keep` on the host. Returns n'."""
    t = _dev(keep if rows is None else rows)
    for c in a:
        assert c.retain_clients_device(t) == int(keep.sum())
    for c in b:
        c.retain_clients(keep)
    return int(keep.sum())


# ---- 1. keys only, before tree_init ------------------------------------------------------------------------

MASK_NAMES = sorted(masks(N))


@pytest.mark.parametrize("name", MASK_NAMES)
@pytest.mark.parametrize("d", [1, 2, 3])
def test_keys_only(d, name):
    """Device keys before tree_init, every mask of masks(130): the twins' keys are equal, then, after tree_init, their
    bincode, frontier and states, and the whole crawl runs in lockstep with the recount's counts."""
    wl = _workload(N, d)
    keep = masks(N)[name]
    kept = np.flatnonzero(keep)
    a, b = _gen_pair(wl), _gen_pair(wl)
    _retain_both(a, b, keep)
    _twins_equal(a, b, name, init=False)
    for c in a + b:
        c.tree_init()
    _twins_equal(a, b, name)
    _lockstep(a, b, wl.left[kept], wl.right[kept], _thr(len(kept)))


# ---- 2. mid-crawl ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_keep", [128, 65, 64, 1])
@pytest.mark.parametrize("depth", [1, 3, 8])
@pytest.mark.parametrize("d", [1, 2])
def test_mid_crawl(d, depth, n_keep):
    """At a frontier of several nodes, 130 -> 128, 65, 64, 1 survivors: the twins are equal and crawl on in lockstep;
    the frontier, its size and the stats are untouched."""
    wl = _workload(N, d)
    a, b = _gen_pair(wl), _gen_pair(wl)
    _crawl_to((a, b), depth, _thr(N))
    paths = a[0].frontier_paths()
    assert paths.shape[0] >= 2 and paths.shape[2] == depth
    keep = _survivors(wl, n_keep, 40 + depth)
    kept = np.flatnonzero(keep)
    before = [(c.frontier_size(), c.stats()) for c in a]
    _retain_both(a, b, keep)
    for c, (size, stats) in zip(a, before):
        assert c.num_clients() == n_keep and c.frontier_size() == size and c.stats() == stats
        assert np.array_equal(c.frontier_paths(), paths)
    _twins_equal(a, b, f"depth {depth}")
    _lockstep(a, b, wl.left[kept], wl.right[kept], _thr(n_keep))


# ---- 3. a shape whose gather strides, and a list of several scan words per block ---------------------------

def test_many_clients():
    """16 385 clients at L = 128, d = 1 (256 key rows: the gather kernels stride), the random mask, device keys:
    257 mask words, so the words and emit kernels run 65 blocks and the last holds one word of one client."""
    from fuzzyheavyhitters_amd import workload
    from fuzzyheavyhitters_amd.collection import sim_eq_count
    n, L, d = 16385, 128, 1
    wl = workload.zipf_workload(n, L, d, num_sites=4, seed=78)
    keep = masks(n)["random"]
    kept = np.flatnonzero(keep)
    a, b = _gen_pair(wl), _gen_pair(wl)
    _retain_both(a, b, keep)
    _twins_equal(a, b, init=False)
    for c in a:
        c.tree_init()
    C, _ = a[0].tree_crawl()
    a[1].tree_crawl()
    cnt = sim_eq_count(*a, C)
    assert np.array_equal(cnt, recount(wl.left[kept], wl.right[kept], children_of(np.zeros((1, d, 0), np.uint8), d)))


# ---- 4. twice, several rows, all ones ----------------------------------------------------------------------

def test_retain_twice():
    """Two device retains (depth 2, then depth 4) = one host retain of the composed mask at depth 4."""
    d = 1
    wl = _workload(N, d)
    a, b = _gen_pair(wl), _gen_pair(wl)
    k1 = _survivors(wl, 100, 1)
    k2 = np.ones(100, np.uint8)
    k2[np.random.default_rng(2).choice(100, 33, replace=False)] = 0
    composed = np.zeros(N, np.uint8)
    composed[np.flatnonzero(k1)[np.flatnonzero(k2)]] = 1
    kept = np.flatnonzero(composed)
    _crawl_to((b, a), 2, 2)                 # the untouched pair's counts decide throughout
    for c in a:
        assert c.retain_clients_device(_dev(k1)) == 100
    from fuzzyheavyhitters_amd.collection import sim_eq_count
    for _ in range(2):
        C = [c.tree_crawl()[0] for c in a + b][0]
        keepn = sim_eq_count(*b, C) >= 2
        assert keepn.sum() >= 2
        for c in a + b:
            c.tree_prune(keepn)
    for c in a:
        assert c.retain_clients_device(_dev(k2)) == 67
    for c in b:
        c.retain_clients(composed)
    _twins_equal(a, b, "twice vs composed")
    _lockstep(a, b, wl.left[kept], wl.right[kept], 2)


@pytest.mark.parametrize("stage", [False, True], ids=["in-place", "staged-copy"])
def test_three_rows(stage, monkeypatch):
    """A 3-row mask at a stride of n + 37 (padding 0xFF) = the host retain of the rows' AND, which differs from every
    row. staged-copy: the rows first go through the ctx's staging buffer, as for a mask on another device
    (FHH_RETAIN_STAGE_MASK makes one GPU take that path)."""
    if stage:
        monkeypatch.setenv("FHH_RETAIN_STAGE_MASK", "1")
    d = 2
    wl = _workload(N, d)
    rng = np.random.default_rng(11)
    buf = np.full((3, N + 37), 0xFF, np.uint8)
    buf[:, :N] = rng.random((3, N)) < 0.8
    keep = buf[:, :N].min(axis=0)
    kept = np.flatnonzero(keep)
    assert 0 < keep.sum() < min(int(buf[r, :N].sum()) for r in range(3))
    a, b = _gen_pair(wl), _gen_pair(wl)
    _crawl_to((a, b), 3, _thr(N))
    _retain_both(a, b, keep, rows=_dev(buf)[:, :N])
    _twins_equal(a, b, "three rows")
    _lockstep(a, b, wl.left[kept], wl.right[kept], _thr(len(kept)))


def test_all_ones():
    """Nobody leaves: OK with n' = n, keys and states unchanged (one row and three)."""
    wl = _workload(N, 1)
    a, b = _gen_pair(wl), _gen_pair(wl)
    _crawl_to((a, b), 2, _thr(N))
    for rows in (1, 3):
        t = _dev(np.ones((rows, N), np.uint8))
        for c in a:
            assert c.retain_clients_device(t if rows > 1 else t[0]) == N
        _twins_equal(a, b, "all ones")
    _lockstep(a, b, wl.left, wl.right, _thr(N))


# ---- 5. keys staged by add_keys ----------------------------------------------------------------------------

@pytest.mark.parametrize("devices", [None, [0, 0]], ids=["one-gpu", "2-shards"])
def test_staged_keys(devices):
    """Keys still on the host (add_keys): the mask's rows join them there and the host vectors are compacted; equal to
    the host retain, then a full crawl."""
    d = 1
    wl = _workload(N, d)
    src = _gen_pair(wl)
    keys = [c.export_keys() for c in src]
    a, b = _pair(L16, d, devices), _pair(L16, d, devices)
    for p in (a, b):
        for c, k in zip(p, keys):
            c.add_keys(*k)
    rows = np.ones((2, N), np.uint8)
    rows[0, ::3] = 0
    rows[1, 64:128] = 0
    keep = rows.min(axis=0)
    kept = np.flatnonzero(keep)
    _retain_both(a, b, keep, rows=rows)
    _twins_equal(a, b, "staged", init=False)
    for c in a + b:
        c.tree_init()
    _twins_equal(a, b, "staged")
    if devices is None:
        _lockstep(a, b, wl.left[kept], wl.right[kept], _thr(len(kept)))
    # a byte 2 is refused on this path too, with the lowest index
    bad = rows.copy()
    bad[1, 77] = 2
    c = _pair(L16, d, devices)[0]
    c.add_keys(*keys[0])
    import fuzzyheavyhitters_amd as fhh
    with pytest.raises(fhh.FhhError, match="keep byte 77 is 2"):
        c.retain_clients_device(_dev(bad))
    assert c.num_clients() == N


# ---- 6. refusals -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("devices", [None, [0, 0]], ids=["one-gpu", "2-shards"])
def test_refusals_leave_the_ctx_as_it_was(devices):
    from fuzzyheavyhitters_amd._lib import lib
    from fuzzyheavyhitters_amd.collection import sim_eq_count
    import torch
    d = 1
    wl = _workload(N, d)
    Lb = lib()

    def call(c, t, n=None, n_rows=1, stride=0, ptr_=None):
        torch.cuda.synchronize()
        nk = ctypes.c_uint64(0xDEAD)
        p = t.data_ptr() if ptr_ is None else ptr_
        rc = Lb.fhh_retain_clients_device(c.handle, ctypes.c_void_p(p), N if n is None else n, n_rows, stride,
                                          ctypes.byref(nk))
        assert rc == 0 or nk.value == 0xDEAD, "a refusal does not write n_kept"
        return rc, (Lb.fhh_last_error(c.handle) or b"").decode()

    good = np.ones(N, np.uint8)
    good[5] = 0
    tg = _dev(good)
    # no keys
    e0, _ = _pair(L16, d, devices)
    rc, msg = call(e0, tg)
    assert rc == FHH_E_STATE and "no keys" in msg
    assert e0.num_clients() == 0
    # appended batches not yet finished by tree_init
    src, _ = _gen_pair(wl)
    a0, _ = _pair(L16, d, devices)
    if devices:
        a0.reserve_clients(N)
    a0.add_keys_bincode_append(src.export_keys_bincode())
    rc, msg = call(a0, tg)
    assert rc == FHH_E_STATE and "appended" in msg, msg
    assert a0.num_clients() == N
    a0.tree_init()
    for g, w in zip(a0.export_keys(), src.export_keys()):
        assert np.array_equal(g, w)
    # the frontier phase
    cs, ref = _gen_pair(wl, devices), _gen_pair(wl)
    _crawl_to((ref, cs), 2, 2)
    keys, states = cs[0].export_keys(), cs[0].export_states()

    def unchanged(what):
        assert cs[0].num_clients() == N and cs[0].frontier_size() == ref[0].frontier_size(), what
        for x, y in zip(keys, cs[0].export_keys()):
            assert np.array_equal(x, y), what
        for x, y in zip(states, cs[0].export_states()):
            assert np.array_equal(x, y), what

    bad = np.ones((2, N), np.uint8)
    bad[1, 100] = 2
    bad[0, 101] = 2
    disjoint = np.zeros((2, N), np.uint8)
    disjoint[0, ::2] = 1
    disjoint[1, 1::2] = 1
    host = np.ones(N, np.uint8)
    host[3] = 0
    tb, td = _dev(bad), _dev(disjoint)
    for what, (rc, msg), text in (("wrong n", call(cs[0], tg, n=N - 1), "keep.len() 129 != 130"),
                                  ("a byte 2", call(cs[0], tb, n_rows=2, stride=N), "keep byte 100 is 2"),
                                  ("a zero AND", call(cs[0], td, n_rows=2, stride=N), "no survivor"),
                                  ("n_rows = 0", call(cs[0], tg, n_rows=0), "n_rows = 0"),
                                  ("NULL", call(cs[0], tg, ptr_=0), "NULL keep_dev"),
                                  ("a host pointer", call(cs[0], None, ptr_=host.ctypes.data), "not device memory")):
        assert rc == FHH_E_ARG and msg.startswith("retain_clients: ") and text in msg, (what, rc, msg)
        unchanged(what)
    assert Lb.fhh_retain_clients_device(None, ctypes.c_void_p(tg.data_ptr()), N, 1, 0, None) == FHH_E_ARG
    # pending children
    C = [c.tree_crawl()[0] for c in cs + ref][0]
    pend = cs[0].export_states()
    rc, msg = call(cs[0], tg)
    assert rc == FHH_E_STATE and "pending" in msg
    assert cs[0].num_clients() == N and cs[0].frontier_size() == (C, 0)
    for x, y in zip(pend, cs[0].export_states()):
        assert np.array_equal(x, y)
    # and the collection still works: the host-pointer refusal left no sticky error behind
    k = sim_eq_count(*ref, C) >= 2
    for c in cs + ref:
        c.tree_prune(k)
    for c in cs:
        assert c.retain_clients_device(tg) == N - 1
    for c in ref:
        c.retain_clients(good)
    _twins_equal(cs, ref, "after the refusals")


def test_wrapper_refusals(fhh):
    """What the C ABI cannot see is refused before the library is called."""
    import torch
    wl = _workload(N, 1)
    c, _ = _gen_pair(wl)
    ok = torch.ones(N, dtype=torch.uint8, device="cuda")
    for what, t, text in (("a CPU tensor", torch.ones(N, dtype=torch.uint8), "on the CPU"),
                          ("an int32 tensor", torch.ones(N, dtype=torch.int32, device="cuda"), "torch.uint8 expected"),
                          ("a column-strided view", torch.ones((N, 2), dtype=torch.uint8, device="cuda")[:, 0],
                           "column stride 1"),
                          ("a numpy mask", np.ones(N, np.uint8), "retain_clients")):
        with pytest.raises(fhh.FhhError, match=text):
            c.retain_clients_device(t)
        with pytest.raises(fhh.FhhError, match=text):
            c.retain_plan_device(t)
    with pytest.raises(fhh.FhhError, match="n is required"):
        c.retain_clients_device(ok.data_ptr())
    assert c.num_clients() == N
    torch.cuda.synchronize()   # a bare pointer: the caller answers for the stream contract
    assert c.retain_clients_device(ok.data_ptr(), n=N) == N


# ---- 7. multi-device ---------------------------------------------------------------------------------------

N7 = 200   # 4 words: 2 shards of 128 + 72 clients, 4 shards of 64 + 64 + 64 + 8


def _mask7(S):
    """One shard emptied, one untouched (the last), one cut off a word boundary (shard 0 loses 3 clients, so every
    later base is ragged)."""
    keep = np.ones(N7, np.uint8)
    keep[[1, 17, 40]] = 0
    if S == 4:
        keep[64:128] = 0
    return keep


@pytest.mark.parametrize("stage", [False, True], ids=["in-place", "staged-copy"])
@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0, 0]], ids=["2-shards", "4-shards"])
def test_shards(devices, stage, monkeypatch):
    """The device retain on a multi-device pair = the host retain on a twin multi-device pair = the device retain on
    a one-GPU pair; shard_info reports the prefix sums of the survivor counts. With 2 shards a second retain empties
    shard 1 (a 2-row mask) and leaves shard 0 untouched."""
    import fuzzyheavyhitters_amd as fhh
    if stage:
        monkeypatch.setenv("FHH_RETAIN_STAGE_MASK", "1")
    S, d = len(devices), 1
    wl = _workload(N7, d)
    g, h, one = _gen_pair(wl, devices), _gen_pair(wl, devices), _gen_pair(wl)
    _crawl_to((one, g, h), 2, 2)
    plan = fhh.shard_plan(N7, S)

    def check(keep, plan, what):
        counts = [int(keep[b:b + c].sum()) for b, c in plan]
        bases = [int(x) for x in np.concatenate([[0], np.cumsum(counts)[:-1]])]
        for c in g + h:
            info, _ = c.shard_info()
            assert [(b, m) for _, b, m in info] == list(zip(bases, counts)), what
        _twins_equal(g, h, f"{what}: device vs host, multi-device")
        _twins_equal(g, one, f"{what}: multi-device vs one GPU")
        return list(zip(bases, counts))

    keep = _mask7(S)
    t = _dev(keep)
    for c in g + one:
        assert c.retain_clients_device(t) == int(keep.sum())
    for c in h:
        c.retain_clients(keep)
    plan = check(keep, plan, "first")
    if S == 4:
        assert plan[1][1] == 0 and plan[3][1] == 8 and plan[2][0] % 64
    kept = np.flatnonzero(keep)
    # a second retain on ragged bases, 2 rows whose AND differs from both
    n2 = len(kept)
    rows = np.ones((2, n2), np.uint8)
    b1 = plan[1][0] if S == 2 else plan[2][0]
    rows[0, b1:b1 + 30] = 0
    rows[1, b1 + 30:(n2 if S == 2 else b1 + 64)] = 0
    keep2 = rows.min(axis=0)
    t2 = _dev(rows)
    for c in g + one:
        assert c.retain_clients_device(t2) == int(keep2.sum())
    for c in h:
        c.retain_clients(keep2)
    plan2 = check(keep2, plan, "second")
    assert plan2[0] == plan[0] and plan2[1 if S == 2 else 2][1] == 0
    kept = kept[np.flatnonzero(keep2)]
    # the crawl goes on: the planes and the one-GPU pair's recounted counts
    from fuzzyheavyhitters_amd.collection import sim_eq_count
    for lv in range(2, 4):
        parents = one[0].frontier_paths()
        outs = [c.tree_crawl(share_planes=True) for c in one + g]
        C = outs[0][0]
        assert [o[0] for o in outs] == [C] * 4
        assert np.array_equal(outs[0][1], outs[2][1]) and np.array_equal(outs[1][1], outs[3][1]), f"planes level {lv}"
        cnt = sim_eq_count(*one, C)
        assert np.array_equal(cnt, recount(wl.left[kept], wl.right[kept], children_of(parents, d)))
        for c in one + g:
            c.tree_prune(cnt >= 2)


def test_shards_refusals():
    """The lowest bad index over the shards, and no survivor overall although a shard's slice has one per row."""
    import fuzzyheavyhitters_amd as fhh
    wl = _workload(N7, 1)
    g, _ = _gen_pair(wl, [0, 0, 0, 0])
    keys = g.export_keys()
    bad = np.ones((2, N7), np.uint8)
    bad[0, 190] = 2
    bad[1, 70] = 3
    bad[0, 130] = 2
    with pytest.raises(fhh.FhhError, match="keep byte 70 is 3"):
        g.retain_clients_device(_dev(bad))
    disjoint = np.zeros((2, N7), np.uint8)
    disjoint[0, ::2] = 1
    disjoint[1, 1::2] = 1
    with pytest.raises(fhh.FhhError, match="no survivor"):
        g.retain_clients_device(_dev(disjoint))
    assert g.num_clients() == N7
    for x, y in zip(keys, g.export_keys()):
        assert np.array_equal(x, y)
    assert [(b, m) for _, b, m in g.shard_info()[0]] == fhh.shard_plan(N7, 4)


# ---- 8. the sketch pipeline --------------------------------------------------------------------------------

@pytest.mark.parametrize("edited", [False, True], ids=["verdicts", "rows-edited"])
def test_sketch_pipeline(edited):
    """sim_sketch_verify over 3 levels leaves ok [3][n] on the GPU; apply_sketch_results_device hands the rows to both
    collections where they lie. = apply_sketch_results with the rows' AND taken on the host, on a twin pair. With two
    rows edited by hand (a different client each) the AND differs from every single row."""
    import torch
    from fuzzyheavyhitters_amd import sketch as S
    d = 1
    wl = _workload(N, d)
    a, b = _gen_pair(wl), _gen_pair(wl)
    _crawl_to((a, b), 2, 2)
    n = a[0].num_clients()
    swl = S.sketch_workload(n, 4, bad_fraction=0.1)
    assert 0 < swl.honest.sum() < n
    batch = S.DeviceSketchBatch(swl)
    S.deal_triples(a[0], batch, levels=3)
    S.sim_sketch_verify(a[0], batch, level=0, n_levels=3)
    torch.cuda.synchronize()
    want = int(swl.honest.sum())
    if edited:
        h = np.flatnonzero(swl.honest)      # rows 0 and 1 each reject an honest client of their own
        batch.ok[0, int(h[0])] = 0
        batch.ok[1, int(h[-1])] = 0
        want -= 2
    ok = batch.ok.cpu().numpy()
    keep = ok.min(axis=0)
    assert int(keep.sum()) == want
    if edited:
        assert all(int(ok[r].sum()) != want for r in range(3))
    else:
        assert np.array_equal(keep.astype(bool), swl.honest)
    assert S.apply_sketch_results_device(a[0], a[1], batch, 0, 3) == want
    assert S.apply_sketch_results(b[0], b[1], keep) == want
    _twins_equal(a, b, "sketch")
    kept = np.flatnonzero(keep)
    _lockstep(a, b, wl.left[kept], wl.right[kept], 2)


def test_sketch_pipeline_last_level():
    """A DeviceSketchBatch255 has the single row of the last level."""
    import fuzzyheavyhitters_amd as fhh
    from fuzzyheavyhitters_amd import sketch as S
    d = 1
    wl = _workload(N, d)
    a, b = _gen_pair(wl), _gen_pair(wl)
    _crawl_to((a, b), 2, 2)
    swl = S.sketch_workload255(N, 3, bad_fraction=0.1)
    batch = S.DeviceSketchBatch255(swl)
    S.sim_sketch_verify_fe255(a[0], batch)
    want = int(swl.honest.sum())
    assert 0 < want < N
    with pytest.raises(fhh.FhhError, match="single row"):
        S.apply_sketch_results_device(a[0], a[1], batch, 0, 2)
    assert S.apply_sketch_results_device(a[0], a[1], batch) == want
    assert S.apply_sketch_results(b[0], b[1], swl.honest) == want
    _twins_equal(a, b, "sketch, last level")
