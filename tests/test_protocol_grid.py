"""The GC and OT kernels' grid-stride loops past their first trip, at sizes the oracle checks in full.

Every GC / OT kernel is launched on min(need, CUs x per_cu) workgroups and strides over its tiles, items or tests;
on 256 CUs a second trip needs about 2 million OTs or tests, where only counts are compared. fhh_set_protocol_grid
(a test / diagnostic call) caps those grids at a few workgroups, so that 4 500 - 20 000 OTs and 1 500 - 20 000
tests send every loop through a second and third trip that ends partial: the per-wave LDS stages the next trip
overwrites, the tables filled once per workgroup, k_gc_eval's 64-aligned slices, the U-unrolled passes of the
row-major table with padding lanes, and the wave-uniform break on the last, odd tile. Each case asserts its own
regime through fhh_protocol_grid (protocol_grid_cases.grid_cases) and then compares bit for bit with the oracle
restatement, by the bodies the per-kernel tests run on the device's grid. No output depends on the grid."""
import ctypes
import os
import time

import numpy as np
import pytest

import protocol_grid_cases as pg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- CPU: the ABI, the model's constants ------------------------------------------------------------------------
def test_protocol_grid_abi():
    """Both symbols exist and refuse a NULL ctx, leaving the output alone (no ctx, so no GPU; the rest of the ABI
    is test_gpu_protocol_grid_abi)."""
    from fuzzyheavyhitters_amd._lib import lib
    L = lib()
    grid = ctypes.c_int(-7)
    assert L.fhh_set_protocol_grid(None, 1) != 0 and L.fhh_set_protocol_grid(None, 0) != 0
    assert L.fhh_set_protocol_grid(None, -1) != 0
    assert L.fhh_protocol_grid(None, pg.GC, 5, ctypes.byref(grid)) != 0 and grid.value == -7


def test_model_constants_match_the_sources():
    """The launch geometry protocol_grid_cases restates (threads per workgroup, tiles per item, tests per lane and
    pass, workgroups per CU and family) is what the sources say; a change there has to revisit the sizes below."""
    csrc = os.path.join(ROOT, "fuzzyheavyhitters_amd", "csrc")
    for fname, consts in pg.CONSTANTS.items():
        text = open(os.path.join(csrc, fname)).read()
        for name, value in consts.items():
            assert pg.source_constant(text, name) == value, (fname, name)
    assert "(tests + 255) / 256" in open(os.path.join(csrc, "fhh_ot.hip")).read()   # launch_cot_fe255_finish
    hdr = open(os.path.join(csrc, "fhh_internal.h")).read()
    per_cu = ", ".join(str(v) for v in pg.PER_CU)
    assert "kGridPerCu[kGridFamilies] = {%s};" % per_cu in hdr
    api = open(os.path.join(ROOT, "include", "fhh.h")).read()
    for name, value in (("OT_EXPAND", pg.OT_EXPAND), ("OT_HASH", pg.OT_HASH), ("OT_ROWS_OUT", pg.OT_ROWS_OUT),
                        ("COT_FINISH", pg.COT_FINISH), ("GC", pg.GC), ("GT_TM", pg.GT_TM), ("GT_ROWS", pg.GT_ROWS)):
        assert pg.source_constant(api, "FHH_GRID_" + name) == value, name


def test_grid_rule_model():
    """The restated rule on its own: need 0 -> 1, below / at / above the limit, a cap below and above it."""
    assert pg.grid_rule(0, 256, 8) == 1 and pg.grid_rule(1, 256, 8) == 1
    assert [pg.grid_rule(n, 256, 8) for n in (2047, 2048, 2049)] == [2047, 2048, 2048]
    assert [pg.grid_rule(n, 256, 1, cap=3) for n in (0, 1, 2, 3, 4)] == [1, 1, 2, 3, 3]
    assert pg.grid_rule(5000, 256, 8, cap=4000) == 2048   # the override only shrinks


@pytest.mark.gpu
def test_gpu_protocol_grid_abi():
    """On a ctx: negative caps are refused with the cap unchanged, unknown families and a NULL grid are refused with
    the output alone, fhh_set_variant keeps the cap, 0 restores the device rule, and a multi-device ctx hands the
    cap to each shard and leaves the shards alone when it refuses."""
    import fuzzyheavyhitters_amd as fhh
    from fuzzyheavyhitters_amd._lib import lib
    L = lib()
    grid = ctypes.c_int(-7)
    kc = fhh.KeyCollection(8, 1)
    free = kc.protocol_grid(pg.GC, 1 << 40)
    assert free > 3
    kc.set_protocol_grid(2)
    for bad in (-1, -(1 << 31)):
        assert L.fhh_set_protocol_grid(kc.handle, bad) != 0
        with pytest.raises(fhh.FhhError, match="set_protocol_grid"):
            kc.set_protocol_grid(bad)
    assert kc.protocol_grid(pg.GC, 100) == 2
    for family in (-1, 7):
        assert L.fhh_protocol_grid(kc.handle, family, 5, ctypes.byref(grid)) != 0 and grid.value == -7
    assert L.fhh_protocol_grid(kc.handle, pg.GC, 5, None) != 0
    kc.set_variant(52)
    assert kc.protocol_grid(pg.GC, 100) == 2, "fhh_set_variant keeps the cap"
    kc.set_protocol_grid(0)
    assert kc.protocol_grid(pg.GC, 1 << 40) == free
    multi = fhh.KeyCollection(8, 1, devices=[0, 0])
    multi.set_protocol_grid(3)
    assert multi.protocol_grid(pg.OT_HASH, 100) == 3
    assert [multi.shard(k).protocol_grid(pg.OT_HASH, 100) for k in range(2)] == [3, 3]
    with pytest.raises(fhh.FhhError):
        multi.set_protocol_grid(-1)
    assert [multi.shard(k).protocol_grid(pg.OT_HASH, 100) for k in range(2)] == [3, 3]
    multi.set_protocol_grid(0)
    assert multi.shard(1).protocol_grid(pg.OT_HASH, 100) == min(100, free // 8)


@pytest.mark.gpu
def test_gpu_protocol_grid_equals_the_model():
    """fhh_protocol_grid = the Python restatement for every family at needs 0, 1, cap - 1, cap, cap + 1, with the
    device's limit as the cap and under fhh_set_protocol_grid at 1, 2, 3, 1000 and above the device's limit."""
    import fuzzyheavyhitters_amd as fhh
    from fuzzyheavyhitters_amd._lib import lib
    cus, name = ctypes.c_int(), ctypes.create_string_buffer(64)
    assert lib().fhh_device_info(0, name, 64, ctypes.byref(cus)) == 0 and cus.value > 0
    kc = fhh.KeyCollection(8, 1)
    for family, per_cu in enumerate(pg.PER_CU):
        limit = cus.value * per_cu
        for cap in (0, 1, 2, 3, 1000, limit + 5):
            kc.set_protocol_grid(cap)
            edge = cap if 0 < cap < limit else limit
            for need in sorted({0, 1, max(edge - 1, 0), edge, edge + 1, limit - 1, limit, limit + 1, 1 << 40}):
                assert kc.protocol_grid(family, need) == pg.grid_rule(need, cus.value, per_cu, cap), (family, cap, need)
    kc.set_protocol_grid(0)


# ---- GPU: one launch chain against the oracle, per grid cap ------------------------------------------------------
M_ITEMS, M_TILES = 4500, 20000   # 9 tiles of 512 OTs -> 10 expand items; 40 hash tiles, the last with 32 OTs


def _run(kc, caps, oracle, body):
    """body(oracle) under each cap; the reference is computed by the first case and shared by the others."""
    took, memo = {}, pg.OracleMemo(oracle)
    try:
        for cap in caps:
            kc.set_protocol_grid(cap)
            t0 = time.perf_counter()
            body(memo)
            took[cap] = round(time.perf_counter() - t0, 2)
    finally:
        kc.set_protocol_grid(0)
    print(f"grid caps (0 = unset) -> seconds: {took}")


def _collection():
    import fuzzyheavyhitters_amd as fhh
    return fhh.KeyCollection(8, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("m", [M_ITEMS, M_TILES])
def test_gpu_ot_mode0_under_grid_caps(oracle, m):
    """Plain OT, explicit and correlated messages: out, U, Y0, Y1. The expands (IKNP: 10 / 40 items over 4 waves
    per workgroup) at both sizes; the hashes k_ot_*_hash_rows<0> (16 tile waves per workgroup) at m = 20 000."""
    kc = _collection()
    kernels = pg.k_expands(1, m) + ([pg.k_hash(m)] if m == M_TILES else [])
    _run(kc, pg.grid_cases(kc, kernels), oracle, lambda o: pg.check_ot_bit_exact(kc, o, m))


@pytest.mark.gpu
@pytest.mark.parametrize("m", [M_ITEMS, M_TILES])
def test_gpu_cot_modes_under_grid_caps(oracle, m):
    """C-OT modes 1, 4, 2, 3, both masks, session counters 0 and 512: both parties' outputs, U and y. m = 4 500:
    k_ot_rows_out (9 tiles over 4 waves: 4, 4, 1) and k_cot_fe255_finish (2 250 tests over 256 lanes) beside the
    expands, whose last item's second tile does not exist; m = 20 000: the hashes <1>, <2>, <3>."""
    kc = _collection()
    kernels = pg.k_expands(1, m) + [pg.k_rows_out(m), pg.k_finish(m)] + ([pg.k_hash(m)] if m == M_TILES else [])
    _run(kc, pg.grid_cases(kc, kernels), oracle, lambda o: pg.check_cot_bit_exact(kc, o, m))


@pytest.mark.gpu
@pytest.mark.parametrize("k,m", [(2, M_ITEMS), (4, M_ITEMS), (2, M_TILES), (4, M_TILES)])
def test_gpu_softspoken_under_grid_caps(oracle, k, m):
    """SoftSpoken k = 2, 4, modes 4, 1, 2: outputs, U, the GGM corrections, y. k = 4 at m = 4 500 has 5 items: a
    cap of 1 gives trips of 4 and 1 (the only case asked for two trips instead of three); m = 20 000 gives
    k_ss_*_expand<4> three trips and runs the hashes on SoftSpoken's Q / T."""
    kc = _collection()
    kernels = pg.k_expands(k, m) + [pg.k_rows_out(m)] + ([pg.k_hash(m)] if m == M_TILES else [])
    if (k, m) == (4, M_ITEMS):
        kc.set_protocol_grid(1)
        r = pg.regime(kc, pg.k_ss_expand(4, m))
        kc.set_protocol_grid(0)
        assert (r.per_trip, r.trips, r.last) == (4, 2, 1)
        caps = sorted(set(pg.grid_cases(kc, [pg.k_ss_expand(4, m)], min_trips=2) + pg.grid_cases(kc, kernels[1:])))
    else:
        caps = pg.grid_cases(kc, kernels)
    _run(kc, caps, oracle, lambda o: pg.check_softspoken_bit_exact(kc, o, k, m))


GC_SIZES = [(1500, 2), (3000, 4), (4097, 8)]   # 1024 tests per workgroup and trip: 2, 3 and 5 trips at a cap of 1


def _gc_caps(kc, n, first=pg.k_gc):
    """The circuit kernels' caps: n = 1 500 has two workgroups' worth of tests, so only a cap of 1 leaves a second
    trip (of 476 tests: k_gc_eval's slices end mid-wave); three trips from n = 3 000."""
    return pg.grid_cases(kc, [first(n)], min_trips=2 if n < 2049 else 3)


@pytest.mark.gpu
@pytest.mark.parametrize("n,bits", GC_SIZES)
def test_gpu_gc_under_grid_caps(oracle, n, bits):
    """gc.equality_test with transcript (k_gc_garble, k_gc_eval<., false>): tables, both label sets, decode bits,
    outputs; four nonce / mask settings."""
    kc = _collection()
    _run(kc, _gc_caps(kc, n), oracle, lambda o: pg.check_gc_bit_exact(kc, o, n, bits))


@pytest.mark.gpu
@pytest.mark.parametrize("n,bits", GC_SIZES)
def test_gpu_cot_labels_chain_under_grid_caps(oracle, n, bits):
    """The C-OT labels chain (k_gc_garble_cot, k_gc_eval<., true> on k_ot_rows_out's labels): zero and active
    labels, tables, decode bits, outputs."""
    kc = _collection()
    _run(kc, _gc_caps(kc, n), oracle, lambda o: pg.check_cot_labels_chain_bit_exact(kc, o, n, bits))


@pytest.mark.gpu
@pytest.mark.parametrize("n,bits", GC_SIZES)
def test_gpu_output_label_share_under_grid_caps(oracle, n, bits):
    """The output-label share path: sh_gb, sh_y, sh_ev with the rest of the transcript; gb - ev = eq mod p. (This
    caller leaves out_packed unset; the level-loop test below runs it.)"""
    kc = _collection()
    _run(kc, _gc_caps(kc, n), oracle, lambda o: pg.check_output_label_share_bit_exact(kc, o, n, bits))


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [1, 2, 3, 4])
def test_gpu_tile_major_table_under_grid_caps(oracle, bits):
    """gc.table_cot at n = 20 000, tile-major labels (k_gt_garble_tm / k_gt_eval_tm, 40 tiles or windows over 16
    waves: 16, 16, 8), in FE and in Z_2^32: labels, messages, both shares, gb - ev = eq in the share's ring."""
    n = 20000
    kc = _collection()
    _run(kc, pg.grid_cases(kc, [pg.k_gt_tm(n, bits)]), oracle, lambda o: pg.check_table_bit_exact(kc, o, n, bits))


@pytest.mark.gpu
@pytest.mark.parametrize("n,bits", [(1500, 3), (3000, 4), (4097, 3), (4097, 4)])
def test_gpu_row_major_table_under_grid_caps(oracle, n, bits):
    """gc.table_cot on the row-major labels (k_ot_rows_out, k_gt_garble<3|4> / k_gt_eval<3|4>, FE and Z_2^32). The
    evaluator takes U = 2 tests per lane and pass, t0 and t0 + stride: at a cap of 1 (stride 1024) n = 1 500 has
    u = 1 partly live, n = 3 000 a second pass with u = 0 partly live and u = 1 all padding, n = 4 097 a third pass
    with one live test."""
    kc = _collection()
    kc.set_table_row_major(True)
    caps = _gc_caps(kc, n, first=pg.k_gt_rows)
    assert 1 in caps
    kc.set_protocol_grid(1)
    stride = pg.regime(kc, pg.k_gt_rows(n)).per_trip
    kc.set_protocol_grid(0)
    live = [[max(0, min(stride, n - (p * pg.GT_EVAL_U + u) * stride)) for u in range(pg.GT_EVAL_U)]
            for p in range(-(-n // (pg.GT_EVAL_U * stride)))]
    assert stride == 1024 and live == {1500: [[1024, 476]], 3000: [[1024, 1024], [952, 0]],
                                       4097: [[1024, 1024], [1024, 1024], [1, 0]]}[n]
    _run(kc, caps, oracle, lambda o: pg.check_table_bit_exact(kc, o, n, bits))


# ---- GPU: the level loop under a cap of 1 -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def crawl_pair():
    """The Zipf workload of test_gc.py test_gpu_crawl_with_ring32_table_equals_plain with 1 100 of its clients
    (the fewest that give each child's tests a second trip through the circuit kernels' 1024 lanes), its plain
    FE-mode crawl, and every level's children."""
    import test_gc as tg
    from fuzzyheavyhitters_amd import sim_crawl, workload
    wl = workload.zipf_workload(1100, 64, 1, num_sites=40, seed=5)
    c0, c1 = tg._pair(wl.left, wl.right, wl.root_seeds)
    plain = sim_crawl(c0, c1, 0.01, mode="fe", prf_seed=9)
    return c0, c1, tg._sig(plain), [int(c) for c in plain.level_children]


@pytest.mark.gpu
@pytest.mark.parametrize("ss_k", [1, 2])
@pytest.mark.parametrize("gc_mode", ["ot", "ot-circuit"])
def test_gpu_crawl_under_a_grid_cap_of_one_equals_plain(monkeypatch, crawl_pair, gc_mode, ss_k):
    """sim_crawl(mode="fe", gc=...) with every GC / OT launch of the level loop on one workgroup (the LoopCtl-bounded
    loops: ot_active, gc_active) gives the plain crawl's counts, keep decisions and heavy hitters: the table in FE and
    in Z_2^32 or the circuit, IKNP and SoftSpoken k = 2, whole levels and three children per chunk.
    Asserted through fhh_protocol_grid, for the FE levels run whole: every kernel of the chain gets one workgroup
    where it needs more and three or more trips at the widest level; and, at some level or in a chunk, several trips
    that end partial (every level has an even number of children, so the IKNP expands' 6 items per child end
    partial in chunks only). A chunk of three children is smaller: its expands, k_ot_rows_out and circuit kernels
    still take several trips that end partial, but its 9 table tiles fit the 16 waves of one trip. The share OT
    (k_gc_eval's out_packed as its choice bits, the hashes, k_cot_fe255_finish) runs at the last level only, in both
    forms: run whole it is asserted to take several trips that end partial; in a chunk of three its 13 hash tiles
    are one trip. On an MI355X a capped crawl takes 0.10 - 0.19 s with the table, 0.16 - 0.47 s with the circuit
    (printed per crawl); the four cases 0.5 - 0.6 s each."""
    import test_gc as tg
    from fuzzyheavyhitters_amd import sim_crawl
    c0, c1, plain, level_children = crawl_pair
    n, bits = 1100, 2
    npad = pg.table_npad(n, bits) if gc_mode == "ot" else (n + 63) // 64 * 64
    took = {}
    try:
        for c in (c0, c1):
            c.set_protocol_grid(1)
        def chain(groups):   # the kernels of an FE level's launch chain over `groups` children
            ks = pg.k_expands(ss_k, groups * bits * npad)
            if gc_mode == "ot":
                return ks + [pg.k_gt_tm(n, bits, groups=groups)]
            return ks + [pg.k_gc(groups * n), pg.k_rows_out(groups * bits * npad)]
        regimes = [[pg.regime(c0, k) for k in chain(groups)] for groups in level_children[:-1]]
        names = [k.name for k in chain(1)]
        for i, name in enumerate(names):
            widest = max(regimes, key=lambda r: r[i].trips)[i]
            assert widest.need > widest.grid == 1 and widest.trips >= 3, (name, widest)
            assert all(r[i].grid == 1 for r in regimes), name
        small = [pg.regime(c0, k) for k in chain(3)]   # a chunk of three children (see the docstring)
        for i, name in enumerate(names):
            single = name.startswith("k_gt_")
            assert (small[i].trips == 1) if single else (small[i].trips >= 2 and small[i].last < small[i].per_trip), \
                (name, small[i])
            assert any(r[i].need > 1 and r[i].trips >= 2 and r[i].last < r[i].per_trip for r in regimes + [small]), name
        # the last level, whole: the circuit, then the share OT of two OTs per test on k_gc_eval's out_packed
        m2 = level_children[-1] * n * 2
        for k in [pg.k_gc(level_children[-1] * n), pg.k_hash(m2), pg.k_finish(m2)] + pg.k_expands(ss_k, m2):
            r = pg.regime(c0, k)
            assert r.need > r.grid == 1 and r.trips >= 2 and r.last < r.per_trip, (k, r)
        for chunk_bytes in (None, 3 * 402 * npad):
            if chunk_bytes:
                monkeypatch.setenv("FHH_GC_CHUNK_BYTES", str(chunk_bytes))
            for ring in ((False, True) if gc_mode == "ot" else (False,)):
                t0 = time.perf_counter()
                got = sim_crawl(c0, c1, 0.01, mode="fe", prf_seed=9, gc=gc_mode, init_capacity=2, ot_ss_k=ss_k,
                                table_ring32=ring)
                took[(chunk_bytes is not None, ring)] = round(time.perf_counter() - t0, 2)
                assert tg._sig(got) == plain, (chunk_bytes, ring)
                assert len(got.final) > 0
    finally:
        for c in (c0, c1):
            c.set_protocol_grid(0)
    print(f"(chunked, ring32) -> seconds per crawl at a cap of 1: {took}")
