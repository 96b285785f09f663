"""fhh_tree_init_at / fhh_frontier_paths on the GPU: a collection seeded at a given frontier holds the evaluation
states the oracle computes for those prefixes, bit for bit, and from there the crawl, the two-party protocol and
the final shares go on exactly as after the level-by-level crawl to the same frontier (ibDCF.rs:238-250
eval_ibDCF per prefix; the reference's own crawl only starts at the root, collect.rs:67-92)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FHH_E_ARG, FHH_E_STATE = -1, -2


def _pair(L, d, devices=None):
    import fuzzyheavyhitters_amd as fhh
    return fhh.KeyCollection(L, d, devices=devices), fhh.KeyCollection(L, d, devices=devices)


def _gen_pair(wl, L, d, devices=None):
    import fuzzyheavyhitters_amd as fhh
    c0, c1 = _pair(L, d, devices)
    fhh.gen_keys_pair(c0, c1, wl.left, wl.right, wl.root_seeds)
    return c0, c1


def _truncated(n, L, d, seed, num_sites=5):
    """A Zipf workload cut to L levels (the cut drops the per-client suffix, so full-depth heavy hitters exist)."""
    from fuzzyheavyhitters_amd import workload
    wl = workload.zipf_workload(n, L + 8, d, num_sites=num_sites, seed=seed)
    wl.left, wl.right = wl.left[:, :, :L].copy(), wl.right[:, :, :L].copy()
    wl.alpha = wl.alpha[:, :, :L].copy()
    return wl


def _paths_array(paths, d):
    return np.array([[list(p) for p in node] for node in paths], np.uint8).reshape(len(paths), d, -1)


def _plane_counts(p0, p1, n):
    """Clients whose two share strings agree, per child, from both servers' share planes [C][2d][nw]."""
    C = p0.shape[0]
    diff = np.zeros((C, p0.shape[2]), np.uint64)
    for j in range(p0.shape[1]):
        diff |= p0[:, j] ^ p1[:, j]
    bits = np.unpackbits(diff.view(np.uint8).reshape(C, -1, 8), axis=2, bitorder="little").reshape(C, -1)[:, :n]
    return (bits == 0).sum(1).astype(np.uint64)


def _states_equal(a, b, what=""):
    for x, y, name in zip(a.export_states(), b.export_states(), ("seed", "t", "y")):
        assert np.array_equal(x, y), f"{what}: {name} differs"


# ---- 1. states = oracle ------------------------------------------------------------------------------------

N1, L1 = 130, 72                                     # three words, two valid lanes in the last
DEPTHS = (0, 1, 31, 32, 33, 63, 64, 65, 71)           # both sides of a 32- or 64-bit packing of the directions, L - 1


def _frontier(rng, F, d, depth):
    """F distinct nodes [F][d][depth]: all 0, all 1, a shared dim-0 prefix (d >= 2), a first direction 1 in every
    dim, random ones — as many of these as F and the depth admit."""
    if depth == 0:
        return np.zeros((1, d, 0), np.uint8)
    def rnd():
        return rng.integers(0, 2, (d, depth), dtype=np.uint8)
    one_first = rnd()
    one_first[:, 0] = 1
    cands = [one_first] if F == 1 else [np.zeros((d, depth), np.uint8), np.ones((d, depth), np.uint8)]
    if F > 3 and d >= 2:
        shared = rnd()
        shared[0] = 0                                # node 0's dim-0 prefix again, the other dims differ
        cands.append(shared)
    if F > 1:
        cands.append(one_first)
    out, seen = [], set()
    tries = 0
    while len(out) < F and tries < 1000:
        c = cands.pop(0) if cands else rnd()
        tries += 1
        if c.tobytes() not in seen:
            seen.add(c.tobytes())
            out.append(c)
    return np.stack(out)


def _oracle_states(O, keys, path):
    """Reference-layout States of one prefix: tree_init, then level_expand along the path (child i = sum bit_j << j)."""
    d, depth = path.shape
    st = O.tree_init(keys)
    for lv in range(depth):
        out, _ = O.level_expand(keys, st, [0], lv)
        i = sum(int(path[j, lv]) << j for j in range(d))
        st = O.States(out.seed[i:i + 1].copy(), out.t[i:i + 1].copy(), out.y[i:i + 1].copy())
    return st


@functools.lru_cache(maxsize=None)
def _case1(d):
    """The workload, both servers' keys and, per (depth, F), the frontier with the oracle's states of both servers:
    computed once per d, shared by the add_keys and gen_keys_pair cases, never changed."""
    from fuzzyheavyhitters_amd import workload
    from oracle import oracle as O
    O.build()
    wl = workload.zipf_workload(N1, L1, d, num_sites=4, seed=70 + d)
    # counter carry across a 32-bit word on a first step in direction 1 (prg.rs:273-276)
    wl.root_seeds[[0, N1 - 1], :, :, :, 8:12] = 0xFF
    k0, k1 = O.gen_keys(wl.left, wl.right, wl.root_seeds)
    rng = np.random.default_rng(900 + d)
    cases, memo = [], {}
    for depth in DEPTHS:
        for F in (1, 3, 5, 9):
            paths = _frontier(rng, F, d, depth)
            if any(np.array_equal(paths, p) for dep, p, _ in cases if dep == depth):
                continue                             # a shallow depth admits fewer nodes than asked for
            want = []
            for s, keys in enumerate((k0, k1)):
                sts = []
                for p in paths:
                    key = (s, p.shape, p.tobytes())
                    if key not in memo:
                        memo[key] = _oracle_states(O, keys, p)
                    sts.append(memo[key])
                want.append(tuple(np.concatenate([getattr(x, f) for x in sts]) for f in ("seed", "t", "y")))
            cases.append((depth, paths, want))
    return wl, k0, k1, cases


def test_case1_frontiers_cover_what_they_should():
    """The frontiers of test 1 (CPU-side facts about the inputs): odd per-dim distinct counts, a count that is not a
    multiple of the kernel's 4-prefix group and one above it, a shared dim-0 prefix, the all-0 / all-1 paths."""
    from fuzzyheavyhitters_amd import KeyCollection
    for d in (1, 2, 3):
        _, _, _, cases = _case1(d)
        assert {dep for dep, _, _ in cases} == set(DEPTHS)
        nus = [KeyCollection.frontier_plan(p)[0] for dep, p, _ in cases if dep >= 31]
        for j in range(d):
            assert any(nu[j] % 2 == 1 and nu[j] > 1 for nu in nus) and any(nu[j] > 4 for nu in nus)
        if d >= 2:
            assert any(nu[0] < len(p) for nu, (dep, p, _) in zip(nus, [c for c in cases if c[0] >= 31]))
        deep = [p for dep, p, _ in cases if dep == 71 and len(p) >= 3]
        assert any((p[0] == 0).all() and (p[1] == 1).all() for p in deep)
        assert any((p[:, :, 0] == 1).all(axis=1).any() for p in deep)


@pytest.mark.parametrize("build", ["add", "gen"])
@pytest.mark.parametrize("d", [1, 2, 3])
def test_states_equal_oracle(d, build):
    """export_states after tree_init_at = the oracle's states of every given node, client and key, both servers;
    the frontier, its paths and the stats are what the header says."""
    import fuzzyheavyhitters_amd as fhh
    wl, k0, k1, cases = _case1(d)
    if build == "gen":
        cs = _gen_pair(wl, L1, d)
    else:   # staged by add_keys: the call itself uploads them
        cs = _pair(L1, d)
        for c, k in zip(cs, (k0, k1)):
            c.add_keys(k.key_idx, k.root_seed, k.cw_seed, k.cw_bits)
    for depth, paths, want in cases:
        nu, _ = fhh.KeyCollection.frontier_plan(paths)
        for c, (seed, t, y) in zip(cs, want):
            before = c.stats()
            c.tree_init_at(paths)
            gs, gt, gy = c.export_states()
            what = f"d {d} depth {depth} F {len(paths)}"
            assert np.array_equal(gt, t), f"{what}: t"
            assert np.array_equal(gy, y), f"{what}: y"
            assert np.array_equal(gs, seed), f"{what}: seeds"
            assert c.frontier_size() == (len(paths), 0)
            assert np.array_equal(c.frontier_paths(), paths)
            after = c.stats()
            assert after["aes_blocks"] - before["aes_blocks"] == depth * 2 * int(nu.sum()) * N1
            for k in ("levels", "ref_evals", "expand_launches"):
                assert after[k] == before[k], k
    # depth 0, one node = tree_init
    (a, _), (b, _) = _gen_pair(wl, L1, d), _gen_pair(wl, L1, d)
    a.tree_init()
    b.tree_init_at(np.zeros((1, d, 0), np.uint8))
    _states_equal(a, b, "root")


# ---- 2. equal to the level-by-level route; the crawl continues identically -----------------------------------

def _crawl_to(c0, c1, k, thr):
    from fuzzyheavyhitters_amd.collection import sim_eq_count
    c0.tree_init()
    c1.tree_init()
    for _ in range(k):
        C, _ = c0.tree_crawl()
        c1.tree_crawl()
        keep = sim_eq_count(c0, c1, C) >= thr
        c0.tree_prune(keep)
        c1.tree_prune(keep)


@functools.lru_cache(maxsize=None)
def _case2(d):
    n, L, frac = ((300, 40, 0.02), (200, 32, 0.05))[d - 1]
    from fuzzyheavyhitters_amd import workload
    wl = _truncated(n, L, d, seed=20 + d)
    thr = max(1, int(frac * n))
    full = workload.plaintext_crawl(wl.left, wl.right, thr, thr)
    return wl, n, L, thr, full


@pytest.mark.parametrize("where", ["1", "half", "last"])
@pytest.mark.parametrize("d", [1, 2])
def test_equals_level_by_level_and_continues(d, where):
    import fuzzyheavyhitters_amd as fhh
    from fuzzyheavyhitters_amd import workload
    from fuzzyheavyhitters_amd.collection import sim_eq_count, sim_ot_sums
    wl, n, L, thr, (_, hh_paths, hh_counts) = _case2(d)
    k = {"1": 1, "half": L // 2, "last": L - 1}[where]
    a0, a1 = _gen_pair(wl, L, d)
    _crawl_to(a0, a1, k, thr)
    _, mid, _ = workload.plaintext_crawl(wl.left, wl.right, thr, thr, levels=k)
    assert len(mid) > 0
    paths = _paths_array(mid, d)
    assert np.array_equal(a0.frontier_paths(), paths) and np.array_equal(a1.frontier_paths(), paths)
    b0, b1 = _gen_pair(wl, L, d)
    b0.tree_init_at(mid)            # the tuples plaintext_crawl returns
    b1.tree_init_at(paths)          # the array
    _states_equal(a0, b0, "server 0")
    _states_equal(a1, b1, "server 1")
    for lv in range(k, L):
        last = lv == L - 1
        outs = [(c.tree_crawl_last if last else c.tree_crawl)(share_planes=True) for c in (a0, a1, b0, b1)]
        C = outs[0][0]
        assert [o[0] for o in outs] == [C] * 4, f"level {lv}"
        assert np.array_equal(outs[0][1], outs[2][1]) and np.array_equal(outs[1][1], outs[3][1]), f"planes level {lv}"
        ca, cb = sim_eq_count(a0, a1, C), sim_eq_count(b0, b1, C)
        assert np.array_equal(ca, cb), f"counts level {lv}"
        if not last:
            for c in (a0, a1, b0, b1):
                c.tree_prune(ca >= thr)
            continue
        sa, sb = sim_ot_sums(a0, a1, C, 7, True), sim_ot_sums(b0, b1, C, 7, True)
        assert sa == sb
        keep = fhh.KeyCollection.keep_values_last(n, thr, *sa)
        assert np.array_equal(keep, ca >= thr)
        for c in (a0, a1, b0, b1):
            c.tree_prune_last(keep)
    fa = fhh.KeyCollection.final_values(a0.final_shares(), a1.final_shares())
    fb = fhh.KeyCollection.final_values(b0.final_shares(), b1.final_shares())
    assert [(r.path, r.value) for r in fa] == [(r.path, r.value) for r in fb]
    got = [(tuple(tuple(int(x) for x in p) for p in r.path), r.value) for r in fb]
    assert all(len(p) == L for path, _ in got for p in path), "full-length paths"
    assert sorted(got) == sorted((p, int(v)) for p, v in zip(hh_paths, hh_counts)) and len(got) > 0


# ---- 3. re-seeding in any phase ------------------------------------------------------------------------------

def test_reseed_in_any_phase():
    import fuzzyheavyhitters_amd as fhh
    from fuzzyheavyhitters_amd import workload
    wl, n, L, thr, _ = _case2(1)
    _, mid, _ = workload.plaintext_crawl(wl.left, wl.right, thr, thr, levels=L // 2)
    ref0, ref1 = _gen_pair(wl, L, 1)
    ref0.tree_init_at(mid)
    # after a finished crawl: frontier_last holds the heavy hitters
    c0, c1 = _gen_pair(wl, L, 1)
    assert len(mid) >= 3
    res = fhh.sim_crawl(c0, c1, 0.02, mode="count")
    assert len(res.final) > 0 and c0.frontier_size()[1] == len(res.final)
    assert c0.frontier_paths().shape == (c0.frontier_size()[0], 1, L - 1)   # works after fhh_sim_crawl
    c0.tree_init_at(mid)
    assert c0.frontier_size() == (len(mid), 0) and c0.final_shares() == []
    _states_equal(ref0, c0, "after a finished crawl")
    # with unpruned pending children: frontier_paths names them in export_states' order
    C, _ = c0.tree_crawl()
    pend = c0.frontier_paths()
    assert pend.shape == (C, 1, L // 2 + 1) and c0.frontier_size() == (C, 0)
    exp = np.array([[list(p[0]) + [i]] for p in mid for i in (0, 1)], np.uint8)
    assert np.array_equal(pend, exp)
    ref0.tree_init_at(pend)
    _states_equal(ref0, c0, "pending children")
    c0.tree_init_at(mid[:3])
    assert c0.frontier_size() == (3, 0) and np.array_equal(c0.frontier_paths(), _paths_array(mid[:3], 1))
    ref0.tree_init_at(mid[:3])
    _states_equal(ref0, c0, "re-seeded over pending children")
    C, _ = c0.tree_crawl()
    assert C == 6


# ---- 4. multi-device -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0, 0]], ids=["2-shards", "4-shards"])
@pytest.mark.parametrize("d", [1, 2])
def test_multi_device_equals_single(devices, d):
    """Every shard walks its own clients to the same frontier (n = 130 = 3 words: 4 shards leave one empty); the
    states and the continued crawl's counts are the one-GPU collection's."""
    wl, k0, k1, cases = _case1(d)
    depth, paths, _ = next(c for c in cases if c[0] == 33 and len(c[1]) == 5)
    s0, s1 = _gen_pair(wl, L1, d)
    g0, g1 = _gen_pair(wl, L1, d, devices)
    for c in (s0, s1, g0, g1):
        c.tree_init_at(paths)
    if len(devices) == 4:
        assert 0 in [cnt for _, _, cnt in g0.shard_info()[0]]
    _states_equal(s0, g0, "server 0")
    _states_equal(s1, g1, "server 1")
    assert np.array_equal(g0.frontier_paths(), paths) and g0.frontier_size() == (5, 0)
    assert g0.stats()["aes_blocks"] == s0.stats()["aes_blocks"]
    for lv in range(depth, depth + 3):
        (C, ps0), (_, ps1), (Cg, pg0), (_, pg1) = [c.tree_crawl(share_planes=True) for c in (s0, s1, g0, g1)]
        assert C == Cg and np.array_equal(ps0, pg0) and np.array_equal(ps1, pg1)
        cnt = _plane_counts(ps0, ps1, N1)
        assert np.array_equal(cnt, _plane_counts(pg0, pg1, N1))
        keep = np.ones(C, bool)
        keep[1::3] = False
        for c in (s0, s1, g0, g1):
            c.tree_prune(keep)
    # a group fed by add_keys (staged on the collection, cut into the shards by the call itself)
    h0, _ = _pair(L1, d, devices)
    h0.add_keys(k0.key_idx, k0.root_seed, k0.cw_seed, k0.cw_bits)
    h0.tree_init_at(paths)
    r0, _ = _gen_pair(wl, L1, d)
    r0.tree_init_at(paths)
    _states_equal(r0, h0, "staged keys on a group")


# ---- 5. two-party resume -------------------------------------------------------------------------------------

@pytest.mark.parametrize("form,ss_k", [("table", 2), ("circuit", 1)], ids=["table-ss2", "circuit"])
@pytest.mark.parametrize("d,n,L,thr", [(1, 300, 20, 0.02), (2, 200, 12, 0.05)], ids=["d1", "d2"])
def test_two_party_resume(d, n, L, thr, form, ss_k):
    """two_party_crawl(start_paths = the plaintext frontier at mid depth): every level >= depth has the
    uninterrupted run's counts, and the final (path, value) set is the same."""
    import fuzzyheavyhitters_amd as fhh
    from fuzzyheavyhitters_amd import workload
    wl = workload.zipf_workload(n, 32, d, num_sites=5, seed=3 + d)
    wl.left, wl.right = wl.left[:, :, :L].copy(), wl.right[:, :, :L].copy()
    c0, c1 = _gen_pair(wl, L, d)
    full = fhh.two_party_crawl(c0, c1, thr, prf_seed=77, material="test", form=form, ot_ss_k=ss_k)
    assert len(full.final) > 0
    k = L // 2
    t = max(1, int(thr * n))
    _, mid, _ = workload.plaintext_crawl(wl.left, wl.right, t, t, levels=k)
    p0, p1 = _gen_pair(wl, L, d)
    log = []
    got = fhh.two_party_crawl(p0, p1, thr, prf_seed=77, material="test", form=form, ot_ss_k=ss_k, start_paths=mid,
                              expect_counts=full.counts, level_log=log)
    assert [e[0] for e in log] == list(range(k, L))
    assert list(got.level_children) == list(full.level_children[k:])
    assert len(got.counts) == L - k
    for lv, (x, y) in enumerate(zip(got.counts, full.counts[k:]), start=k):
        assert np.array_equal(x, y), f"level {lv}"
    assert [(r.path, r.value) for r in got.final] == [(r.path, r.value) for r in full.final]


# ---- 6. candidate query --------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", [1, 2])
def test_candidate_query(d):
    """Counts at Q known full-depth points: seed their parents at depth L - 1, tree_crawl_last, read the wanted
    children — against a brute-force count of the clients whose box [left, right] holds the point."""
    from fuzzyheavyhitters_amd.collection import sim_eq_count
    from fuzzyheavyhitters_amd import workload
    n, L = 130, 32
    wl = workload.zipf_workload(n, L, d, num_sites=3, seed=50 + d)   # uncut: the balls are real intervals
    w =np.uint64(1) << np.arange(L - 1, -1, -1, dtype=np.uint64)
    lo, hi, al = [(x.astype(np.uint64) * w).sum(-1) for x in (wl.left, wl.right, wl.alpha)]   # [n][d] integers
    rng = np.random.default_rng(6)
    pts = [al[0], al[17]]                                      # clients' own points
    pts.append(hi[5])                                          # a ball's corner
    pts.append(al[0] ^ np.uint64(1))                           # its neighbour: the same parent as point 0
    far = rng.integers(0, 1 << L, d, dtype=np.uint64)
    while ((lo <= far) & (far <= hi)).all(1).any():
        far = rng.integers(0, 1 << L, d, dtype=np.uint64)
    pts.append(far)                                            # a point no ball covers
    pts = np.array(pts, np.uint64)                             # [Q][d]
    want = np.array([((lo <= p) & (p <= hi)).all(1).sum() for p in pts], np.uint64)
    assert want[0] >= 1 and want[-1] == 0
    bits = ((pts[:, :, None] >> np.arange(L - 1, -1, -1, dtype=np.uint64)) & np.uint64(1)).astype(np.uint8)  # [Q][d][L]
    parents, idx = np.unique(bits[:, :, :L - 1], axis=0, return_inverse=True)
    assert len(parents) < len(pts)
    c0, c1 = _gen_pair(wl, L, d)
    c0.tree_init_at(parents)
    c1.tree_init_at(parents)
    C, _ = c0.tree_crawl_last()
    c1.tree_crawl_last()
    assert C == len(parents) << d
    cnt = sim_eq_count(c0, c1, C)
    child = [(int(idx.reshape(-1)[q]) << d) + sum(int(bits[q, j, L - 1]) << j for j in range(d)) for q in range(len(pts))]
    assert np.array_equal(cnt[child], want), (cnt[child], want)


# ---- 7. refusals ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("devices", [None, [0, 0]], ids=["one-gpu", "2-shards"])
def test_refusals_leave_the_ctx_as_it_was(devices):
    import ctypes
    import fuzzyheavyhitters_amd as fhh
    from fuzzyheavyhitters_amd._lib import lib, ptr
    L, d = 32, 2
    wl = _truncated(130, L, d, seed=81)
    Lb = lib()

    def call(c, paths, n_nodes=None, depth=None, null=False):
        a = np.ascontiguousarray(paths, np.uint8)
        rc = Lb.fhh_tree_init_at(c.handle, a.shape[0] if n_nodes is None else n_nodes,
                                 a.shape[2] if depth is None else depth, None if null or not a.size else ptr(a))
        return rc, (Lb.fhh_last_error(c.handle) or b"").decode()

    good = np.array([[[0, 1, 1], [1, 0, 0]], [[0, 1, 1], [1, 1, 0]], [[1, 1, 1], [1, 1, 1]]], np.uint8)
    # no keys: FHH_E_STATE, and frontier_paths before any init too
    e0, _ = _pair(L, d, devices)
    rc, msg = call(e0, good)
    assert rc == FHH_E_STATE and "no keys" in msg
    nn, dep = ctypes.c_uint64(), ctypes.c_uint32()
    assert Lb.fhh_frontier_paths(e0.handle, ctypes.byref(nn), ctypes.byref(dep), None) == FHH_E_STATE
    assert Lb.fhh_last_error(e0.handle)
    c0, _ = _gen_pair(wl, L, d, devices)
    assert Lb.fhh_frontier_paths(c0.handle, ctypes.byref(nn), ctypes.byref(dep), None) == FHH_E_STATE
    c0.tree_init_at(good)
    C, _ = c0.tree_crawl()
    keep = np.ones(C, bool)
    keep[2] = False
    c0.tree_prune(keep)
    size, states, paths = c0.frontier_size(), c0.export_states(), c0.frontier_paths()
    dup = np.concatenate([good, good[1:2]])
    two = good.copy()
    two[2, 1, 0] = 2
    bad = {
        "n_nodes = 0": call(c0, good, n_nodes=0),
        "depth >= data_len": call(c0, np.zeros((1, d, L), np.uint8)),
        "a byte 2": call(c0, two),
        "two equal paths": call(c0, dup),
        "two roots": call(c0, np.zeros((2, d, 0), np.uint8)),
        "n_nodes << d past u32": call(c0, good, n_nodes=1 << 30, depth=0, null=True),
        "NULL paths with depth > 0": call(c0, good, null=True),
    }
    for what, (rc, msg) in bad.items():
        assert rc == FHH_E_ARG and msg.startswith("tree_init_at: "), (what, rc, msg)
    assert c0.frontier_size() == size and np.array_equal(c0.frontier_paths(), paths)
    for a, b in zip(states, c0.export_states()):
        assert np.array_equal(a, b)
    with pytest.raises(fhh.FhhError):
        c0.tree_init_at(dup)
    with pytest.raises(fhh.FhhError):
        c0.tree_init_at(np.zeros((1, d + 1, 3), np.uint8))   # the wrapper's shape check
    C2, _ = c0.tree_crawl()                                   # and the crawl goes on
    assert C2 == size[0] << d
