"""The child-level reductions of csrc/fhh_kernels.hip (k_eq_count, k_share_planes, k_child_sums_fe / _fe255, k_sum_fe /
k_sum_fe255) at the edges of their launch geometry, bit-exact against the plain models of child_reduction_cases.py:

  A  C > 65 535 children: the grid-stride loop over children runs a second trip (the reuse of the LDS reduction
     buffer, the second trip's atomics into the partials, copies of C and 2 d C rows), on a frontier `tree_init_at`
     seeds, at d = 1 (C = 65 616) and d = 2 (C = 65 600), and in FieldElm at the last level
  B  the node sums' client loop over 1 .. 4 trips of its 256 threads, every value format, row pitches ld > n,
     one ctx and two shards
  C  k_child_sums_fe's 4096-client chunks (one, exactly one, two, two and a ragged one) and k_eq_count's word
     regimes (nw = 1025: the first valid second word; nw = 2050: a second pass of two words)

All of these are integer reductions with one right answer; a dropped, doubled or mis-strided client or child shows
as an exact difference in one server's sum even where it cancels in v0 - v1. The conditions that make the inputs
reach those paths are unmarked tests on the models alone."""
import functools

import numpy as np
import pytest

import child_reduction_cases as cc

gpu = pytest.mark.gpu
PRF_SEED = 0xC41D


# ---- conditions on the inputs and the models: no GPU -------------------------------------------------------------

@pytest.mark.parametrize("d", [1, 2])
def test_wide_frontier_strides_over_counted_children(d):
    case, m = cc.wide_case(d), cc.wide_inside(d)
    cnt = m.sum(1)
    C = case.C
    assert case.left.shape == (65, d, case.L) and case.paths.shape == (cc.WIDE[d]["F"], d, case.depth)
    assert C == {1: 65616, 2: 65600}[d] and C >= cc.GRID_CAP + 64 and m.shape == (C, 65)
    assert (case.paths[0] == 0).all() and (case.paths[-1] == 1).all()
    hi, lo = cnt[cc.GRID_CAP:], cnt[:case.strided]                 # the second trip's children; their blocks' first
    assert (hi > 0).sum() >= 16 and (lo > 0).sum() >= 16
    assert len(set(hi[hi > 0].tolist())) > 1 and len(set(lo[lo > 0].tolist())) > 1
    assert m[:, 64].any() and m[cc.GRID_CAP:, 64].any()             # the one valid lane of the second word counts
    assert 0 < cnt.max() < 65
    assert m.any(0).all()                                           # every client is counted somewhere
    keep = cc.wide_keep(C)
    assert 40 <= keep.sum() <= 46 and cnt[keep].any()


def test_wide_values_hold_the_special_rows():
    C = cc.wide_case(1).C
    v = cc.wide_fe_values(C, 65, 1)
    for c in (0, cc.GRID_CAP - 1, cc.GRID_CAP, C - 1):
        assert (v[c] == 2 ** 64 - 1).all()
    assert (v == 0).all(1).sum() == 1
    w = cc.wide_fe255_limbs(100 + cc.GRID_CAP, 3, 1)
    assert (w[cc.GRID_CAP] == 0xFFFFFFFF).all() and (w == 0).all((1, 2)).sum() == 1


def test_vectorised_sim_ot_models_agree_with_the_oracle(oracle):
    rng = np.random.default_rng(11)
    for C, n, level in ((5, 70, 0), (12, 33, 16)):
        eq = rng.random((C, n)) < 0.4
        eq[0], eq[1] = True, False
        assert cc.sim_sums_fe(eq, PRF_SEED, level) == tuple(oracle.sim_ot_sums_fe(eq, PRF_SEED, level))
        assert cc.sim_sums_fe255(eq, PRF_SEED, level) == tuple(oracle.sim_ot_sums_fe255(eq, PRF_SEED, level))
    # client_base shifts the client index, across 32 bits too
    eq = rng.random((3, 8)) < 0.5
    base = 2 ** 32 - 3
    for f in (cc.sim_sums_fe, cc.sim_sums_fe255):
        assert f(eq, 9, 2, client_base=5) != f(eq, 9, 2)
    r0 = oracle.sim_prf(9, 2, np.arange(3, dtype=np.uint64)[:, None],
                        (np.uint64(base) + np.arange(8, dtype=np.uint64))[None, :], 0) & np.uint64(oracle.FE_MASK)
    want = [sum(int(x) % oracle.FE_P + 1 for x in row) % oracle.FE_P for row in r0]
    assert cc.sim_sums_fe(eq, 9, 2, client_base=base)[0] == want


def test_sim_ot_models_at_the_field_edges(monkeypatch):
    """The draws the PRF never makes in a test: r >= p (reduced once), r0 = p - 1 (r1 wraps to 0)."""
    P, Q = cc.FE_P, cc.FE255_P
    draws = [P - 2, P - 1, P, P + 5, 2 ** 62 - 1, 0, 1]
    eq = np.array([[True] * 7, [False] * 7, [True, False] * 3 + [True]])
    monkeypatch.setattr(cc, "_prf", lambda *a: np.broadcast_to(np.array(draws, np.uint64), (3, 7)).copy())
    r0 = [v - P if v >= P else v for v in draws]
    r1 = [(v + 1) % P for v in r0]
    s0, s1 = cc.sim_sums_fe(eq, 0, 0)
    assert s0 == [sum(r1) % P] * 3
    assert s1 == [sum(a if e else b for a, b, e in zip(r0, r1, row)) % P for row in eq]
    draws = [Q - 2, Q - 1, Q, Q + 18, 2 ** 64 - 1, 2 ** 128 - 1, 2 ** 192 - 1]
    monkeypatch.setattr(cc, "_prf", lambda s, lv, C, n, b, word: np.broadcast_to(
        np.array([(v >> (64 * word)) & (2 ** 64 - 1) for v in draws], np.uint64), (3, 7)).copy())
    r0 = [v - Q if v >= Q else v for v in draws]
    r1 = [(v + 1) % Q for v in r0]
    s0, s1 = cc.sim_sums_fe255(eq, 0, 0)
    assert s0 == [sum(r1)] * 3
    assert s1 == [sum(a if e else b for a, b, e in zip(r0, r1, row)) for row in eq]


def test_node_sum_models_are_exact_integer_sums():
    v = cc.loop_fe_values(257)
    assert cc.node_sums_fe_model(v) == [sum(int(x) for x in row) % cc.FE_P for row in v]
    w = cc.loop_fe255_limbs(65)
    exact = [sum(sum(int(x) << (32 * k) for k, x in enumerate(e)) for e in row) for row in w]
    assert cc.node_sums_fe255_model(w) == (exact, [x % cc.FE255_P for x in exact])
    raw = np.frombuffer(b"".join(int(x).to_bytes(32, "big") for x in (1, 2 ** 255 + 7)), np.uint8).reshape(1, 2, 32)
    assert cc.node_sums_fe255_model(cc.blockpair_limbs(raw))[0] == [2 ** 255 + 8]
    bits = np.zeros((1, 65, 2), np.uint8)
    bits[0, 0, 0] = bits[0, 64, 0] = bits[0, 63, 1] = 1
    assert cc.pack_planes(bits).tolist() == [[[1, 1], [1 << 63, 0]]]


@pytest.mark.parametrize("n", cc.LOOP_N + (cc.LOOP_SHARDED_N,))
def test_loop_values_as_described(n):
    v, w = cc.loop_fe_values(n), cc.loop_fe255_limbs(n)
    assert v.shape == (16, n) and w.shape == (16, n, 8)
    assert (v[1] == 2 ** 64 - 1).all() and (w[1] == 0xFFFFFFFF).all() and not v[2].any() and not w[2].any()
    assert np.nonzero(v[3])[0].tolist() == [n - 1] and np.nonzero(w[3].all(1))[0].tolist() == [n - 1]
    if n > cc.SUM_THREADS:
        assert np.nonzero(v[4])[0].tolist() == [256] and np.nonzero(w[4].all(1))[0].tolist() == [256]
    assert {x > cc.SUM_THREADS for x in cc.LOOP_N} == {False, True} and max(cc.LOOP_N) > 3 * cc.SUM_THREADS


@pytest.mark.parametrize("n", cc.CHUNK_N)
def test_chunk_cases_count_the_clients_at_the_edges(n):
    case = cc.chunk_case(n)
    nw = (n + 63) // 64
    assert case.left.shape == (n, 1, 3)
    for lv in range(cc.CHUNK_LEVELS):
        cnt, keep = case.inside[lv].sum(1), case.keep[lv]
        assert keep.any() and ((cnt[keep] > 0) & (cnt[keep] < n)).any(), lv
        m = case.inside[lv][keep]
        assert m[:, 64 * (nw - 1):].any(), lv                       # the last word
        if n > cc.SIM_OT_CHUNK:                                     # every client chunk, the ragged one included
            for b in range(0, n, cc.SIM_OT_CHUNK):
                assert m[:, b:b + cc.SIM_OT_CHUNK].any() and not m[:, b:b + cc.SIM_OT_CHUNK].all(), (lv, b)
        if nw > cc.EQ_THREADS:                                      # word 1024: a thread's second word
            assert m[:, 64 * cc.EQ_THREADS:64 * (cc.EQ_THREADS + 1)].any(), lv
        if nw > 2 * cc.EQ_THREADS:                                  # word 2048: the second pass
            assert m[:, 64 * 2 * cc.EQ_THREADS:64 * (2 * cc.EQ_THREADS + 1)].any(), lv
    assert {(x + 63) // 64 for x in cc.CHUNK_N} >= {1025, 2050}
    assert {-(-x // cc.SIM_OT_CHUNK) for x in cc.CHUNK_N[:4]} == {1, 2, 3}


# ---- helpers of the GPU tests ------------------------------------------------------------------------------------

def _dev(arr):
    """A host array's bytes in device memory (a torch tensor: keep it alive while its pointer is in use)."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(arr).reshape(-1).view(np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    return t


@functools.lru_cache(maxsize=None)
def _wide_keys(d, L):
    """The oracle's keys of both servers for wide_case(d), cut to L levels."""
    from oracle import oracle as O
    O.build()
    case = cc.wide_case(d)
    return O.gen_keys(np.ascontiguousarray(case.left[:, :, :L]), np.ascontiguousarray(case.right[:, :, :L]), case.roots)


def _keyed_pair(d, L):
    import fuzzyheavyhitters_amd as fhh
    cs = fhh.KeyCollection(L, d), fhh.KeyCollection(L, d)
    for c, k in zip(cs, _wide_keys(d, L)):
        c.add_keys(k.key_idx, k.root_seed, k.cw_seed, k.cw_bits)
    return cs


def _wide_pair(d, L=None, paths=None):
    """Both servers' collections on wide_case(d)'s keys, seeded at its frontier (or at `paths`)."""
    case = cc.wide_case(d)
    cs = _keyed_pair(d, L or case.L)
    for c in cs:
        c.tree_init_at(case.paths if paths is None else paths)
    return cs


def _close(*cs):
    for c in cs:
        c.close()


@functools.lru_cache(maxsize=None)
def _wide_planes(d):
    from oracle import oracle as O
    case = cc.wide_case(d)
    return tuple(cc.share_planes_model(O, k, case.paths) for k in _wide_keys(d, case.L))


def _first_difference(got, want):
    bad = [c for c, (a, b) in enumerate(zip(got, want)) if a != b]
    return f"{len(bad)} children differ, the first at {bad[:8]}" if bad else ""


# ---- A. more than 65 535 children --------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("d", [1, 2])
def test_wide_share_planes(d):
    """k_share_planes over C > 65 535 and the copy of its 2 d C rows: each server's planes are its own oracle
    share bits, the 63 lanes past client 64 zero."""
    case = cc.wide_case(d)
    c0, c1 = _wide_pair(d)
    try:
        for c, want in zip((c0, c1), _wide_planes(d)):
            C, planes = c.tree_crawl(share_planes=True)
            assert C == case.paths.shape[0] << d == case.C and planes.shape == (C, 2 * d, 2)
            bad = np.nonzero((planes != want).any((1, 2)))[0]
            assert bad.size == 0, f"{bad.size} children differ, the first at {bad[:8]}"
            assert not (planes[:, :, 1] >> np.uint64(1)).any()
        # both servers' planes together are the inside matrix
        p0, p1 = _wide_planes(d)
        same = ~np.bitwise_or.reduce(p0 ^ p1, axis=1)                 # [C][nw]
        bits = np.unpackbits(same.view(np.uint8).reshape(case.C, -1), axis=1, bitorder="little")[:, :65]
        assert np.array_equal(bits.astype(bool), cc.wide_inside(d))
    finally:
        _close(c0, c1)


@gpu
@pytest.mark.parametrize("d", [1, 2])
def test_wide_eq_count_and_sim_ot_sums(d):
    """k_eq_count and k_child_sums_fe over C > 65 535: every child's count and both servers' FE sums, with
    client_base + i below and across 2^32; a second call on the same partials starts from zero again."""
    from fuzzyheavyhitters_amd.collection import sim_eq_count, sim_ot_sums
    case, m = cc.wide_case(d), cc.wide_inside(d)
    c0, c1 = _wide_pair(d)
    try:
        C, _ = c0.tree_crawl()
        assert c1.tree_crawl()[0] == C == case.C
        got = sim_eq_count(c0, c1, C)
        bad = np.nonzero(got != m.sum(1).astype(np.uint64))[0]
        assert bad.size == 0, f"{bad.size} counts differ, the first at {bad[:8]}"
        for base in (0, 2 ** 32 - 3, 0):
            c0.set_client_base(base)
            c1.set_client_base(base)
            want = cc.sim_sums_fe(m, PRF_SEED, case.depth, client_base=base)
            got = sim_ot_sums(c0, c1, C, PRF_SEED, last=False)
            for s in (0, 1):
                assert not _first_difference(got[s], want[s]), (base, s, _first_difference(got[s], want[s]))
    finally:
        _close(c0, c1)


@gpu
@pytest.mark.parametrize("d", [1, 2])
def test_wide_node_sums_fe(d):
    """k_sum_fe over C > 65 535 rows: host values (a copy of C rows), device u64 values at ld = n and device 16-B
    blocks at ld = n + 3."""
    from fuzzyheavyhitters_amd._lib import FHH_VALS_FE_BLOCK, FHH_VALS_FE_U64
    case = cc.wide_case(d)
    c0, c1 = _wide_pair(d)
    try:
        C, _ = c0.tree_crawl()
        n = 65
        vals = cc.wide_fe_values(C, n, 60 + d)
        want = np.array(cc.node_sums_fe_model(vals), np.uint64)

        def check(got, what):
            bad = np.nonzero(got != want)[0]
            assert bad.size == 0, f"{what}: {bad.size} sums differ, the first at {bad[:8]}"
        check(c0.node_sums_fe(vals), "host")
        t = _dev(vals)
        check(c0.node_sums_fe_device([t.data_ptr()], n, C, FHH_VALS_FE_U64), "u64, ld = n")
        check(c0.node_sums_fe_device([t.data_ptr()], 0, C, FHH_VALS_FE_U64), "u64, ld = 0")
        t = _dev(cc.with_pitch(cc.fe_blocks(vals), n + 3))
        check(c0.node_sums_fe_device([t.data_ptr()], n + 3, C, FHH_VALS_FE_BLOCK), "blocks, ld = n + 3")
    finally:
        _close(c0, c1)


@gpu
@pytest.mark.parametrize("d", [1, 2])
def test_wide_prune_scattered(d):
    """tree_prune of C > 65 535 children with a scattered keep mask: the frontier's paths, its states (those of a
    fresh pair seeded at the kept paths) and the next level's counts."""
    from fuzzyheavyhitters_amd.collection import sim_eq_count
    case = cc.wide_case(d)
    c0, c1 = _wide_pair(d)
    fresh = ()
    try:
        C, _ = c0.tree_crawl()
        c1.tree_crawl()
        keep = cc.wide_keep(C)
        kept = cc.children_of(case.paths, d)[keep]
        for c in (c0, c1):
            c.tree_prune(keep)
            assert c.frontier_size() == (len(kept), 0)
            assert np.array_equal(c.frontier_paths(), kept)
        fresh = _wide_pair(d, paths=kept)
        for c, f in zip((c0, c1), fresh):
            for a, b, name in zip(c.export_states(), f.export_states(), ("seed", "t", "y")):
                assert np.array_equal(a, b), name
        C2, _ = c0.tree_crawl()
        assert c1.tree_crawl()[0] == C2 == len(kept) << d
        want = cc.inside(case.left, case.right, cc.children_of(kept, d)).sum(1).astype(np.uint64)
        assert want.any() and np.array_equal(sim_eq_count(c0, c1, C2), want)
    finally:
        _close(c0, c1, *fresh)


@gpu
def test_wide_fieldelm_last_level():
    """k_child_sums_fe255 and k_sum_fe255 over C > 65 535 at the last level (L = 17, the same depth-16 frontier): the
    servers' unreduced simulated-OT sums, the node sums of host limbs and of device values in both formats at
    ld = n and n + 3, and final_shares carrying each of them."""
    from fuzzyheavyhitters_amd._lib import FHH_VALS_FE255_BLOCKPAIR, FHH_VALS_FE255_LIMBS
    from fuzzyheavyhitters_amd.collection import sim_ot_sums
    case = cc.wide_case(1)
    L, n = case.depth + 1, 65
    kids = cc.children_of(case.paths, 1)
    m = cc.inside(case.left, case.right, kids)
    assert np.array_equal(m, cc.wide_inside(1))                  # 17 of the 18 bits decide the same children
    c0, c1 = _wide_pair(1, L=L)
    try:
        C, _ = c0.tree_crawl_last()
        assert c1.tree_crawl_last()[0] == C == case.C
        want = cc.sim_sums_fe255(m, PRF_SEED, case.depth)
        got = sim_ot_sums(c0, c1, C, PRF_SEED, last=True)
        for s, c in enumerate((c0, c1)):
            assert not _first_difference(got[s], want[s]), (s, _first_difference(got[s], want[s]))
            res = c.final_shares()
            assert [r.value for r in res] == want[s]
        assert np.array_equal(np.array([r.path for r in res], np.uint8), kids)

        limbs = cc.wide_fe255_limbs(C, n, 71)
        unr, can = cc.node_sums_fe255_model(limbs)
        assert max(unr) >= 65 * (2 ** 256 - 1) and any(u != c for u, c in zip(unr, can))

        def check(got, what):
            assert not _first_difference(got[0], unr), (what, _first_difference(got[0], unr))
            assert not _first_difference(got[1], can), (what, _first_difference(got[1], can))
        check(c0.node_sums_fe255(limbs), "host limbs")
        assert [r.value for r in c0.final_shares()] == unr
        for ld in (n, n + 3):
            t = _dev(cc.with_pitch(limbs, ld))
            check(c0.node_sums_fe255_device([t.data_ptr()], ld, C, FHH_VALS_FE255_LIMBS), f"limbs, ld {ld}")
        # BlockPairs: big-endian bytes of values up to 2^256 - 1
        raw = np.random.default_rng(72).integers(0, 256, size=(C, n, 32), dtype=np.uint8)
        raw[[0, cc.GRID_CAP - 1, cc.GRID_CAP, C - 1]] = 0xFF
        unr, can = cc.node_sums_fe255_model(cc.blockpair_limbs(raw))
        for ld in (n, n + 3):
            t = _dev(cc.with_pitch(raw, ld))
            check(c1.node_sums_fe255_device([t.data_ptr()], ld, C, FHH_VALS_FE255_BLOCKPAIR), f"blockpairs, ld {ld}")
        assert [r.value for r in c1.final_shares()] == unr
    finally:
        _close(c0, c1)


# ---- B. the client loop of the node sums -------------------------------------------------------------------------

def _loop_ctx(n, devices=None):
    """One server's collection of n clients (d = 2, L = 4) after two unpruned crawls: 16 pending children."""
    import fuzzyheavyhitters_amd as fhh
    left, right, roots = cc.loop_workload(n)
    c0 = fhh.KeyCollection(4, 2, devices=devices)
    c1 = fhh.KeyCollection(4, 2, devices=devices)
    fhh.gen_keys_pair(c0, c1, left, right, roots)
    c1.close()
    c0.tree_init()
    assert c0.tree_crawl()[0] == 4 and c0.tree_crawl()[0] == cc.LOOP_ROWS
    return c0


def _to_last_level(c0):
    keep = np.zeros(cc.LOOP_ROWS, bool)
    keep[[0, 5, 10, 15]] = True
    c0.tree_prune(keep)
    assert c0.tree_crawl_last()[0] == cc.LOOP_ROWS


def _shard_columns(rows, info, ld_extra):
    """Per shard (base, count): its columns of rows [C][n][...] at a common pitch of max count + ld_extra."""
    ld = max(cnt for _, _, cnt in info) + ld_extra
    return ld, [_dev(cc.with_pitch(rows[:, b:b + cnt], ld, seed=90 + k)) for k, (_, b, cnt) in enumerate(info)]


@gpu
@pytest.mark.parametrize("n", cc.LOOP_N)
def test_node_sums_client_loop(n):
    """k_sum_fe and k_sum_fe255 with 1 .. 4 trips of their 256-thread client loop, each format, host and device
    entry points, at ld = n and ld = n + 5."""
    from fuzzyheavyhitters_amd._lib import (FHH_VALS_FE255_BLOCKPAIR, FHH_VALS_FE255_LIMBS, FHH_VALS_FE_BLOCK,
                                            FHH_VALS_FE_U64)
    c0 = _loop_ctx(n)
    try:
        C = cc.LOOP_ROWS
        vals = cc.loop_fe_values(n)
        want = cc.node_sums_fe_model(vals)
        assert c0.node_sums_fe(vals).tolist() == want
        for ld in (n, n + 5):
            t = _dev(cc.with_pitch(vals, ld))
            assert c0.node_sums_fe_device([t.data_ptr()], ld, C, FHH_VALS_FE_U64).tolist() == want, ld
            t = _dev(cc.with_pitch(cc.fe_blocks(vals), ld))
            assert c0.node_sums_fe_device([t.data_ptr()], ld, C, FHH_VALS_FE_BLOCK).tolist() == want, ld
        _to_last_level(c0)
        limbs = cc.loop_fe255_limbs(n)
        want = cc.node_sums_fe255_model(limbs)
        raw = np.ascontiguousarray(limbs.view(np.uint8)[..., ::-1])   # the same values as BlockPairs
        assert np.array_equal(cc.blockpair_limbs(raw), limbs)
        assert c0.node_sums_fe255(limbs) == want
        for ld in (n, n + 5):
            t = _dev(cc.with_pitch(limbs, ld))
            assert c0.node_sums_fe255_device([t.data_ptr()], ld, C, FHH_VALS_FE255_LIMBS) == want, ld
            t = _dev(cc.with_pitch(raw, ld))
            assert c0.node_sums_fe255_device([t.data_ptr()], ld, C, FHH_VALS_FE255_BLOCKPAIR) == want, ld
        assert [r.value for r in c0.final_shares()] == want[0]
    finally:
        c0.close()


@gpu
def test_node_sums_client_loop_two_shards():
    """The same on a collection of two shards of more than 256 clients each (320 and 286), one device pointer per
    shard, at ld = 0 (each shard's own count) and at a common pitch past the longer shard."""
    from fuzzyheavyhitters_amd._lib import (FHH_VALS_FE255_BLOCKPAIR, FHH_VALS_FE255_LIMBS, FHH_VALS_FE_BLOCK,
                                            FHH_VALS_FE_U64)
    n, C = cc.LOOP_SHARDED_N, cc.LOOP_ROWS
    c0 = _loop_ctx(n, devices=[0, 0])
    try:
        info, _ = c0.shard_info()
        assert [cnt for _, _, cnt in info] == [320, 286] and [b for _, b, _ in info] == [0, 320]
        vals = cc.loop_fe_values(n)
        want = cc.node_sums_fe_model(vals)
        assert c0.node_sums_fe(vals).tolist() == want
        for fmt, rows in ((FHH_VALS_FE_U64, vals), (FHH_VALS_FE_BLOCK, cc.fe_blocks(vals))):
            ts = [_dev(rows[:, b:b + cnt]) for _, b, cnt in info]
            assert c0.node_sums_fe_device([t.data_ptr() for t in ts], 0, C, fmt).tolist() == want, fmt
            ld, ts = _shard_columns(rows, info, 5)
            assert c0.node_sums_fe_device([t.data_ptr() for t in ts], ld, C, fmt).tolist() == want, fmt
        _to_last_level(c0)
        limbs = cc.loop_fe255_limbs(n)
        want = cc.node_sums_fe255_model(limbs)
        raw = np.ascontiguousarray(limbs.view(np.uint8)[..., ::-1])
        assert c0.node_sums_fe255(limbs) == want
        for fmt, rows in ((FHH_VALS_FE255_LIMBS, limbs), (FHH_VALS_FE255_BLOCKPAIR, raw)):
            ts = [_dev(rows[:, b:b + cnt]) for _, b, cnt in info]
            assert c0.node_sums_fe255_device([t.data_ptr() for t in ts], 0, C, fmt) == want, fmt
            ld, ts = _shard_columns(rows, info, 5)
            assert c0.node_sums_fe255_device([t.data_ptr() for t in ts], ld, C, fmt) == want, fmt
        assert [r.value for r in c0.final_shares()] == want[0]
    finally:
        c0.close()


# ---- C. client chunks and word regimes ---------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("n", cc.CHUNK_N)
def test_client_chunks_and_word_regimes(n):
    """A three-level crawl pruned by the count model: at every level k_eq_count's counts and both servers'
    simulated-OT sums (FE, then FieldElm at the last level) equal the models, for n on both sides of
    k_child_sums_fe's 4096-client chunks and at nw = 1025 and 2050 words."""
    import fuzzyheavyhitters_amd as fhh
    from fuzzyheavyhitters_amd.collection import sim_eq_count, sim_ot_sums
    case = cc.chunk_case(n)
    L = cc.CHUNK_LEVELS
    c0, c1 = fhh.KeyCollection(L, 1), fhh.KeyCollection(L, 1)
    try:
        fhh.gen_keys_pair(c0, c1, case.left, case.right, case.roots)
        c0.tree_init()
        c1.tree_init()
        for lv in range(L):
            last = lv == L - 1
            m = case.inside[lv]
            C, _ = c0.tree_crawl_last() if last else c0.tree_crawl()
            assert (c1.tree_crawl_last() if last else c1.tree_crawl())[0] == C == m.shape[0]
            assert sim_eq_count(c0, c1, C).tolist() == m.sum(1).tolist(), lv
            model = cc.sim_sums_fe255 if last else cc.sim_sums_fe
            for _ in range(2):                                      # the partials start from zero every time
                assert sim_ot_sums(c0, c1, C, PRF_SEED + lv, last=last) == model(m, PRF_SEED + lv, lv), lv
            if not last:
                c0.tree_prune(case.keep[lv])
                c1.tree_prune(case.keep[lv])
    finally:
        _close(c0, c1)
