"""Helpers of test_protocol_grid.py, and the bit-exact test bodies it shares with test_ot.py, test_softspoken.py,
test_gc.py and test_table_tm_wide.py (each takes the collection, so the same assertions run on the device's grid
and under fhh_set_protocol_grid).

The model: every GC / OT kernel below is launched on grid = min(need, CUs x per_cu[, cap]) workgroups (at least
one) and its waves or lanes stride over `items` units of work, per_wg of them per workgroup and trip. The launcher's
`need` and the kernel's `items` are restated here from csrc/fhh_ot.hip and csrc/fhh_gc.hip (the launchers size some
grids from the padded OT count mp, the kernels loop over the active one); test_protocol_grid.py pins the constants
against the sources and asks the library (fhh_protocol_grid) for the grid itself."""
import re
from collections import namedtuple

import numpy as np

CAPS = (1, 2, 3)

# fhh_protocol_grid's families (include/fhh.h FHH_GRID_*) and their workgroups per CU (csrc/fhh_internal.h)
OT_EXPAND, OT_HASH, OT_ROWS_OUT, COT_FINISH, GC, GT_TM, GT_ROWS = range(7)
PER_CU = (8, 1, 8, 8, 8, 1, 8)

# the launch geometry of the kernels (name in the sources, value)
CONSTANTS = {
    "fhh_ot.hip": {"FHH_CC_THREADS": 256, "FHH_CC_TPI": 2, "kOtTileWords": 16, "kOtRowsThreads": 1024,
                   "kOtOutThreads": 256},
    "fhh_gc.hip": {"kGcThreads": 1024, "FHH_GT_GARBLE_U": 1, "FHH_GT_EVAL_U": 2},
}
OT_CC_WAVES = CONSTANTS["fhh_ot.hip"]["FHH_CC_THREADS"] // 64
OT_CC_TPI = CONSTANTS["fhh_ot.hip"]["FHH_CC_TPI"]
OT_TILE = 32 * CONSTANTS["fhh_ot.hip"]["kOtTileWords"]          # OTs per hash / rows-out tile
OT_HASH_WAVES = CONSTANTS["fhh_ot.hip"]["kOtRowsThreads"] // 64
OT_OUT_WAVES = CONSTANTS["fhh_ot.hip"]["kOtOutThreads"] // 64
FINISH_THREADS = 256
GC_THREADS = CONSTANTS["fhh_gc.hip"]["kGcThreads"]
GT_WAVES = GC_THREADS // 64
GT_EVAL_U = CONSTANTS["fhh_gc.hip"]["FHH_GT_EVAL_U"]


def source_constant(text, name):
    """The value `name` is given in a source text, as `#define name V` or `constexpr int name = V;`."""
    m = re.search(r"#define\s+%s\s+(\d+)" % name, text) or re.search(r"constexpr int %s = (\d+);" % name, text)
    return int(m.group(1)) if m else None


def grid_rule(need, cus, per_cu, cap=0):
    """csrc/fhh_internal.h protocol_grid."""
    limit = cus * per_cu
    if 0 < cap < limit:
        limit = cap
    return limit if need >= limit else max(need, 1)


def _cdiv(a, b):
    return (a + b - 1) // b


Kernel = namedtuple("Kernel", "name family need items per_wg")


def _ot_tiles(m):
    """(512-OT tiles of the active OTs, of the matrices padded to 8192 OTs)."""
    return _cdiv(_cdiv(m, 128), 4), _cdiv(m, 8192) * 8192 // 512


def k_recv_expand_cc(m):
    tiles, ptiles = _ot_tiles(m)
    return Kernel("k_ot_recv_expand_cc", OT_EXPAND, _cdiv(2 * ptiles, OT_CC_WAVES), 2 * _cdiv(tiles, OT_CC_TPI),
                  OT_CC_WAVES)


def k_send_expand_cc(m):
    tiles, ptiles = _ot_tiles(m)
    return Kernel("k_ot_send_expand_cc", OT_EXPAND, _cdiv(ptiles, OT_CC_WAVES), 2 * _cdiv(tiles, 2), OT_CC_WAVES)


def k_ss_expand(k, m):
    """k_ss_recv_expand<k> and k_ss_send_expand<k>: one wave per 64 / (128 / k) tiles."""
    tiles, ptiles = _ot_tiles(m)
    tpw = 64 // (128 // k)
    return Kernel(f"k_ss_*_expand<{k}>", OT_EXPAND, _cdiv(_cdiv(ptiles, tpw), OT_CC_WAVES), _cdiv(tiles, tpw),
                  OT_CC_WAVES)


def k_expands(ss_k, m):
    return [k_ss_expand(ss_k, m)] if ss_k > 1 else [k_recv_expand_cc(m), k_send_expand_cc(m)]


def k_hash(m):
    tiles = _cdiv(m, OT_TILE)
    return Kernel("k_ot_*_hash_rows", OT_HASH, _cdiv(tiles, OT_HASH_WAVES), tiles, OT_HASH_WAVES)


def k_rows_out(m):
    tiles = _cdiv(m, OT_TILE)
    return Kernel("k_ot_rows_out", OT_ROWS_OUT, _cdiv(tiles, OT_OUT_WAVES), tiles, OT_OUT_WAVES)


def k_finish(m):
    return Kernel("k_cot_fe255_finish", COT_FINISH, _cdiv(m // 2, FINISH_THREADS), m // 2, FINISH_THREADS)


def k_gc(n):
    return Kernel("k_gc_garble / k_gc_eval", GC, _cdiv(n, GC_THREADS), n, GC_THREADS)


def k_gt_rows(n):
    return Kernel("k_gt_garble / k_gt_eval", GT_ROWS, _cdiv(n, GC_THREADS), n, GC_THREADS)


def table_npad(n, bits):
    """Clients per bit of the table's labels OT: whole 512-OT tiles at b <= 2, whole words at b = 3, 4."""
    return _cdiv(n, 512) * 512 if bits <= 2 else _cdiv(n, 64) * 64


def k_gt_tm(n, bits, groups=1):
    nw = table_npad(n, bits) // 64
    tiles = groups * ((nw + 7) // 8 if bits > 2 else nw // 8)
    return Kernel("k_gt_garble_tm / k_gt_eval_tm", GT_TM, _cdiv(tiles, GT_WAVES), tiles, GT_WAVES)


Regime = namedtuple("Regime", "need grid per_trip trips last")


def regime(kc, k):
    """The launch of kernel k under kc's current grid cap: the grid from the library, the trips of its loop and
    the units of work left for the last trip."""
    grid = kc.protocol_grid(k.family, k.need)
    per_trip = grid * k.per_wg
    trips = _cdiv(k.items, per_trip)
    return Regime(k.need, grid, per_trip, trips, k.items - (trips - 1) * per_trip)


def grid_cases(kc, kernels, min_trips=3):
    """The grid caps a test runs, [0 (unset), ...], from fhh_protocol_grid — and the reason each capped case exists,
    asserted: for every kernel of `kernels` some cap of CAPS leaves fewer workgroups than the launch needs
    (need > grid) and its loop min_trips or more trips with a partial last one; where a cap gives exactly two such
    trips it runs as well. A changed constant (waves per workgroup, tile size) that would put a case back into one
    trip fails here."""
    picked = set()
    try:
        for k in kernels:
            ragged = {}
            for cap in CAPS:
                kc.set_protocol_grid(cap)
                r = regime(kc, k)
                if r.need > r.grid and r.trips >= 2 and r.last < r.per_trip:
                    ragged[cap] = r
            assert ragged, f"{k.name}: no cap of {CAPS} gives a second trip that ends partial"
            many = [c for c, r in ragged.items() if r.trips >= min_trips]
            assert many, f"{k.name}: no cap of {CAPS} gives {min_trips} trips ({ragged})"
            picked.add(min(many))
            picked.update([c for c, r in ragged.items() if r.trips == 2][:1])
    finally:
        kc.set_protocol_grid(0)
    for k in kernels:   # the control: the device rule, never more workgroups than the launch needs
        r = regime(kc, k)
        assert r.grid <= max(r.need, 1) and r.grid >= 1, (k.name, r)
    return [0] + sorted(picked)


# ---- the bit-exact bodies ---------------------------------------------------------------------------------------
def _key(v):
    if isinstance(v, np.ndarray):
        return (v.shape, v.dtype.str, hash(v.tobytes()))
    if isinstance(v, (list, tuple)):
        return tuple(_key(x) for x in v)
    return v


class OracleMemo:
    """The oracle with each call's result kept: the cases of one test differ in the launch grid only, so the
    reference is computed once and shared (the bodies below read the results and leave them unchanged)."""

    def __init__(self, oracle):
        self._oracle, self._kept = oracle, {}

    def __getattr__(self, name):
        f = getattr(self._oracle, name)
        if not callable(f):
            return f

        def call(*args, **kw):
            key = (name, _key(args), _key(sorted(kw.items())))
            if key not in self._kept:
                self._kept[key] = f(*args, **kw)
            return self._kept[key]
        return call


def ot_inputs(m, seed):
    import test_ot
    return test_ot._inputs(m, seed)


def check_ot_bit_exact(kc, oracle, m):
    """test_ot.py test_gpu_ot_bit_exact: plain OT (mode 0), explicit and correlated messages: out, U, Y0, Y1."""
    from fuzzyheavyhitters_amd import ot
    ch, x0, x1, seeds, s, delta = ot_inputs(m, m + 1)
    for corr in (False, True):
        args = dict(x1=None, delta=delta) if corr else dict(x1=x1, delta=None)
        got, u, y0, y1 = ot.ot_extend(kc, ch, x0, base_seeds=seeds, base_choice=s, tweak_base=11, transcript=True,
                                      **args)
        exp, eu, ey0, ey1 = oracle.ot_extend(ch, x0, args["x1"], args["delta"], seeds, s, tweak_base=11,
                                             transcript=True)
        assert np.array_equal(got, exp)
        assert np.array_equal(u, eu)
        assert np.array_equal(y0, ey0) and np.array_equal(y1, ey1)
        want = np.where(ch[:, None] == 1, x0 ^ np.frombuffer(delta, np.uint8) if corr else x1, x0)
        assert np.array_equal(got, want)


def check_cot_bit_exact(kc, oracle, m):
    """test_ot.py test_gpu_cot_bit_exact: C-OT modes 1, 4, 2 and 3 (mode 3 on an even count: k_cot_fe255_finish),
    both masks, two session counters: both parties' outputs and both protocol messages (U, y; mode 4 has no y)."""
    from fuzzyheavyhitters_amd import ot
    ch, _, _, seeds, s, delta = ot_inputs(m, 5 * m + 1)
    for ctr_off in (0, 512):
        got = ot.cot_extend(kc, 1, ch, seeds, s, delta=delta, ctr_off=ctr_off, transcript=True)
        exp = oracle.cot_extend(oracle.COT_LABELS, ch, seeds, s, delta=delta, ctr_off=ctr_off)
        for g, e in zip(got, exp):
            assert np.array_equal(g, e)
        got = ot.cot_extend(kc, 4, ch, seeds, s, ctr_off=ctr_off, transcript=True)
        exp = oracle.cot_extend(oracle.COT_RAW, ch, seeds, s, ctr_off=ctr_off)
        for g, e in zip(got[:3], exp[:3]):   # q, t, U (no y)
            assert np.array_equal(g, e)
        for mask in (0, 1):
            got = ot.cot_extend(kc, 2, ch, seeds, s, mask=mask, ctr_off=ctr_off, transcript=True)
            exp = oracle.cot_extend(oracle.COT_FE, ch, seeds, s, mask=mask, ctr_off=ctr_off)
            for g, e in zip(got, exp):
                assert np.array_equal(g, e)
        mm = 2 * ((m + 1) // 2)
        ch2 = np.repeat(ch[: mm // 2], 2)
        for mask in (0, 1):
            got = ot.cot_extend(kc, 3, ch2, seeds, s, mask=mask, ctr_off=ctr_off, transcript=True)
            exp = oracle.cot_extend(oracle.COT_FE255, ch2, seeds, s, mask=mask, ctr_off=ctr_off)
            for g, e in zip(got, exp):
                assert np.array_equal(g, e)


def check_softspoken_bit_exact(kc, oracle, k, m):
    """test_softspoken.py test_gpu_softspoken_bit_exact: SoftSpoken C-OT modes 4, 1, 2, two session counters: both
    parties' outputs, U, the GGM corrections, and y where the mode has one."""
    from fuzzyheavyhitters_amd import ot
    import test_softspoken as tss
    ch, seeds, s, delta = tss._inputs(m, 7 * m + k)
    for ctr_off in (0, 512):
        got = ot.cot_extend(kc, 4, ch, seeds, s, ctr_off=ctr_off, transcript=True, ss_k=k)
        exp = oracle.cot_extend_ss(k, oracle.COT_RAW, ch, seeds, s, ctr_off=ctr_off)
        for name, g, e in zip(("q", "t", "U", "y", "corr"), got, exp):
            if name != "y":
                assert np.array_equal(g, e), name
        got = ot.cot_extend(kc, 1, ch, seeds, s, delta=delta, ctr_off=ctr_off, transcript=True, ss_k=k)
        exp = oracle.cot_extend_ss(k, oracle.COT_LABELS, ch, seeds, s, delta=delta, ctr_off=ctr_off)
        for g, e in zip(got, exp):
            assert np.array_equal(g, e)
        for mask in (0, 1):
            got = ot.cot_extend(kc, 2, ch, seeds, s, mask=mask, ctr_off=ctr_off, transcript=True, ss_k=k)
            exp = oracle.cot_extend_ss(k, oracle.COT_FE, ch, seeds, s, mask=mask, ctr_off=ctr_off)
            for g, e in zip(got, exp):
                assert np.array_equal(g, e)


def check_gc_bit_exact(kc, oracle, n, bits):
    """test_gc.py test_gpu_gc_bit_exact: gc.equality_test with transcript: tables, both label sets, decode bits,
    outputs."""
    from fuzzyheavyhitters_amd import gc
    import test_gc as tg
    rng = np.random.default_rng(n * 10 + bits)
    g, e = tg._cases(rng, n, bits)
    # label_nonce 0 / 1 << 20 (multiples of the label counter stride: the label passes share AES
    # rounds 1-2) and 123 (unaligned: some lanes' counters carry out of byte 0, full rounds)
    for nonce, mask in ((123, 0), (123, 1), (0, 1), (1 << 20, 0)):
        out, tr = gc.equality_test(kc, g, e, mask, tg.KEY, tg.DELTA, label_nonce=nonce, gate_base=77, transcript=True)
        t, gl, el, d = oracle.gc_garble_eq(g, e, mask, tg.KEY, tg.DELTA, label_nonce=nonce, gate_base=77)
        assert np.array_equal(tr.tables, t)
        assert np.array_equal(tr.gb_labels, gl)
        assert np.array_equal(tr.ev_labels, el)
        assert np.array_equal(tr.decode, d)
        assert np.array_equal(out, oracle.gc_eval_eq(t, gl, el, d, gate_base=77))
        assert np.array_equal(out ^ mask, (g == e).all(axis=1).astype(np.uint8))


def check_cot_labels_chain_bit_exact(kc, oracle, n, bits):
    """test_gc.py test_gpu_cot_labels_chain_bit_exact: the labels OT + k_gc_garble_cot + k_gc_eval<., true>."""
    import fuzzyheavyhitters_amd as fhh
    import pytest
    from fuzzyheavyhitters_amd import gc
    import test_gc as tg
    rng = np.random.default_rng(n * 3 + bits)
    g, e = tg._cases(rng, n, bits)
    seeds = rng.integers(0, 256, (128, 2, 16), dtype=np.uint8)
    s = tg._colour_s(rng)
    with pytest.raises(fhh.FhhError):   # Delta = s needs the colour bit
        gc.equality_test_cot(kc, g, e, 0, seeds, bytes([s[0] & 0xFE]) + s[1:])
    for mask, ctr in ((0, 0), (1, 256), (1, 512)):
        out, tr = gc.equality_test_cot(kc, g, e, mask, seeds, s, gate_base=7, ctr_off=ctr)
        exp, etr = tg._oracle_cot_chain(oracle, g, e, mask, seeds, s, gate_base=7, ctr_off=ctr)
        for k in ("ev_zero", "ev_active", "tables", "decode"):
            assert np.array_equal(tr[k], etr[k]), k
        assert np.array_equal(out, exp)
        assert np.array_equal(out ^ mask, (g == e).all(axis=1).astype(np.uint8))


def check_output_label_share_bit_exact(kc, oracle, n, bits):
    """test_gc.py test_gpu_output_label_share_bit_exact: sh_gb, sh_y, sh_ev with the rest of the transcript."""
    from fuzzyheavyhitters_amd import gc
    import test_gc as tg
    rng = np.random.default_rng(n * 5 + bits)
    g, e = tg._cases(rng, n, bits)
    seeds = rng.integers(0, 256, (128, 2, 16), dtype=np.uint8)
    s = tg._colour_s(rng)
    for mask, ctr in ((0, 0), (1, 256)):
        out, tr = gc.equality_test_cot(kc, g, e, mask, seeds, s, gate_base=9, ctr_off=ctr, share=True)
        exp, etr = tg._oracle_cot_chain(oracle, g, e, mask, seeds, s, gate_base=9, ctr_off=ctr, share=True)
        for k in ("ev_zero", "ev_active", "tables", "decode", "gb_share", "share_y", "ev_share"):
            assert np.array_equal(tr[k], etr[k]), k
        assert np.array_equal(out, exp)
        eq = (g == e).all(axis=1).astype(np.uint64)
        assert np.array_equal(((tr["gb_share"].astype(object) - tr["ev_share"].astype(object)) % tg.FE_P)
                              .astype(np.uint64), eq)


def check_table_bit_exact(kc, oracle, n, bits, big=False):
    """test_table_tm_wide.py test_gpu_wide_table_bit_exact: gc.table_cot in FE and in Z_2^32, both masks and two
    session counters (big: one of each, Z_2^32 only): labels, every message, both shares; gb - ev = eq."""
    from fuzzyheavyhitters_amd import gc
    import test_gc as tg
    rng = np.random.default_rng(n * 13 + bits)
    g, e = tg._cases(rng, n, bits)
    seeds = rng.integers(0, 256, (128, 2, 16), dtype=np.uint8)
    s = tg._colour_s(rng)
    eq = (g == e).all(axis=1).astype(np.uint64)
    for mask, ctr in (((1, 256),) if big else ((0, 0), (1, 256))):
        for ring in ((True,) if big else (False, True)):
            tr = gc.table_cot(kc, g, e, mask, seeds, s, gate_base=13, ctr_off=ctr, ring32=ring)
            chain = tg._oracle_table_chain_ring32 if ring else tg._oracle_table_chain
            etr = chain(oracle, g, e, mask, seeds, s, gate_base=13, ctr_off=ctr)
            for k in ("ev_zero", "ev_active", "msgs", "gb_share", "ev_share"):
                assert np.array_equal(tr[k], etr[k].astype(tr[k].dtype)), (k, mask, ctr, ring)
            if ring:
                assert np.array_equal((tr["gb_share"] - tr["ev_share"]) & 0xFFFFFFFF, eq)
            else:
                diff = (tr["gb_share"].astype(object) - tr["ev_share"].astype(object)) % tg.FE_P
                assert np.array_equal(diff.astype(np.uint64), eq)
