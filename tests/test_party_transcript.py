"""Each server's level messages and node sums against the oracle, chunk by chunk and level by level.

The level-shaped tests of tests/test_party.py compare v0 - v1 with a recount or with another run of the
same code, where an error both servers share cancels. Here every wire message of the fhh_gb_* /
fhh_ev_* ABI (u1 with the SoftSpoken corrections, gc, u2, y2) is compared byte for byte, and each
server's fhh_party_node_sums on its own, with tests/party_model.py: the oracle's OT extension, garbled
table / circuit and share OT under the gate tweaks and row-PRG counters the state machine must use
(the level in the tweak, the chunk's offset in the level, the session counter continuing over chunks and
levels that share base OTs). The material is drawn from a seeded generator; no expected value comes
from a second run of the code under test."""
import ctypes

import numpy as np
import pytest

import party_model as pm


# ---- the model's own parts (no GPU) -----------------------------------------------------------------
@pytest.mark.parametrize("R,nb,nblk", [(128, 1, 64), (128, 9, 64), (64, 64, 64), (32, 130, 192), (128, 67, 128)])
def test_tile_major_pack_unpack_inverse(R, nb, nblk):
    """tmaj_pack places block (i, c) at byte 16 ((c // 4) 4 R + 4 i + c % 4), leaves the blocks past nb zero
    and tmaj_unpack reads the same blocks back; a full wire round-trips the other way too."""
    rng = np.random.default_rng(R + nb)
    rows = rng.integers(0, 256, (R, nb, 16), dtype=np.uint8)
    wire = pm.tmaj_pack(rows, nblk)
    assert wire.shape == (R * nblk * 16,)
    for i, c in ((0, 0), (R - 1, nb - 1), (R // 2, nb // 2), (1, min(5, nb - 1))):
        at = 16 * ((c // 4) * 4 * R + 4 * i + c % 4)
        assert np.array_equal(wire[at:at + 16], rows[i, c])
    assert np.array_equal(pm.tmaj_unpack(wire, R, nb), rows)
    assert not pm.tmaj_unpack(wire, R, nblk)[:, nb:].any()
    full = rng.integers(0, 256, R * nblk * 16, dtype=np.uint8)
    assert np.array_equal(pm.tmaj_pack(pm.tmaj_unpack(full, R, nblk), nblk), full)


def test_session_counter_and_tweak_bookkeeping():
    """Sizes (8192-OT padding, 256-block session steps, tile / word padding of the OT index), the running
    session counter (continues on unchanged material, restarts on new), the tweak ranges of tables and
    circuits, and the disjointness checks themselves."""
    assert [pm.ot_padded(m) for m in (1, 8192, 8193)] == [8192, 8192, 16384]
    assert [pm.session_blocks(m) for m in (0, 1, 8192, 32768, 32769)] == [0, 256, 256, 256, 512]
    assert pm.npad_of(521, 2, 0, False) == 1024 and pm.npad_of(521, 2, 1, False) == 576
    assert pm.npad_of(521, 2, 0, True) == 576 and pm.npad_of(200, 4, 0, False) == 256
    assert pm.is_table(4, 0, False) and not pm.is_table(6, 0, False) and not pm.is_table(2, 0, True)
    assert pm.u_wire_bytes(0, 2) == 0 and pm.u_wire_bytes(1, 1) == 16 * 8192
    assert pm.u_wire_bytes(1, 4) == 4 * 8192 + 4096
    book = pm.SessionBook()
    a, b = b"a" * 32, b"b" * 32
    assert [book.take(0, a, 8192), book.take(0, a, 40000), book.take(0, a, 0), book.take(0, a, 1)] == [0, 256, 768, 768]
    assert book.take(1, a, 5) == 0 and book.take(1, a, 5) == 256          # kind 1 counts on its own
    assert book.take(0, b, 10) == 0 and book.take(0, a, 10) == 0          # new material restarts, also going back
    assert pm.disjoint_per_key((m, lo, hi) for k, m, lo, hi in book.log if k == 1)
    assert not pm.disjoint_per_key((m, lo, hi) for k, m, lo, hi in book.log if k == 0)   # a came back at 0
    # tweaks: chunks of one level tile the level; the level bits separate levels; the circuit's are doubled
    n, bits = 521, 2
    r = [pm.tweak_range(3, cb, cc, n, bits, True) for cb, cc in ((0, 4), (4, 4), (8, 2))]
    assert r == [((3 << 40) + 0, (3 << 40) + 4 * n), ((3 << 40) + 4 * n, (3 << 40) + 8 * n),
                 ((3 << 40) + 8 * n, (3 << 40) + 10 * n)]
    assert pm.ranges_disjoint(r + [pm.tweak_range(4, 0, 10, n, bits, True)])
    assert not pm.ranges_disjoint(r + [pm.tweak_range(3, 3, 2, n, bits, True)])
    assert pm.tweak_range(2, 3, 3, 200, 4, False) == (2 * ((2 << 40) + 3 * 200 * 3), 2 * ((2 << 40) + 6 * 200 * 3))
    assert pm.tweak_range(2, 3, 3, 200, 4, True) == ((2 << 40) + 1800, (2 << 40) + 2400)
    assert pm.ranges_disjoint([(5, 5), (0, 9)]) and not pm.ranges_disjoint([(0, 3), (2, 4)])


def test_plane_bits_and_counts():
    rng = np.random.default_rng(2)
    bits = rng.integers(0, 2, (3, 2, 130), dtype=np.uint8)
    pad = np.zeros((3, 2, 192), np.uint8)
    pad[:, :, :130] = bits
    planes = np.packbits(pad.reshape(3, 2, 3, 64), axis=-1, bitorder="little").view(np.uint64).reshape(3, 2, 3)
    assert np.array_equal(pm.plane_bits(planes, 130), bits)
    other = bits.copy()
    other[1, 0, :7] ^= 1
    assert list(pm.equal_counts(bits, other)) == [130, 123, 130]


def test_chunk_model_shares_reconstruct_the_count(oracle):
    """The model's own output is consistent in every form: gb - ev = eq per test (mod p), whatever the
    chunk, counter, mask and k; the last level's GC output is eq ^ mask."""
    rng = np.random.default_rng(9)
    for d, n, form, last, k in ((1, 70, 0, False, 1), (1, 70, 1, False, 2), (2, 70, 0, False, 4), (2, 70, 1, False, 1),
                                (1, 70, 0, True, 2), (2, 70, 0, True, 1)):
        b0 = rng.integers(0, 2, (5, 2 * d, n), dtype=np.uint8)
        b1 = b0.copy()
        b1[:, 0, ::3] ^= 1
        pairs = rng.integers(0, 256, (2, 128, 2, 16), dtype=np.uint8)
        s = rng.integers(0, 256, (2, 16), dtype=np.uint8)
        s[0, 0] |= 1
        for mask in (0, 1):
            r = pm.chunk_model(b0, b1, 2, 3, 6, last, form, k, pairs, s, mask, (256, 512))
            eq = (b0[2:5] == b1[2:5]).all(axis=1)
            p = pm.FE255_P if last else pm.FE_P
            assert np.array_equal(((r["gv"] - r["ev"]) % p).astype(np.uint64), eq.astype(np.uint64))
            if last:
                assert np.array_equal(r["out"], eq.astype(np.uint8) ^ mask)
                assert len(r["y2"]) == 2 * 3 * n * 16 and r["m2"] == 6 * n


# ---- driving the ABI --------------------------------------------------------------------------------
def _keys(wl, L, d, devices=None):
    import fuzzyheavyhitters_amd as fhh
    c0 = fhh.KeyCollection(L, d, devices=devices)
    c1 = fhh.KeyCollection(L, d, devices=devices)
    fhh.gen_keys_pair(c0, c1, wl.left, wl.right, wl.root_seeds)
    return c0, c1


def _workload(d):
    from fuzzyheavyhitters_amd import workload
    if d == 1:
        wl, thr = workload.zipf_workload(521, 32, 1, num_sites=6, seed=41), 0.02
    else:
        wl, thr = workload.zipf_workload(200, 32, 2, num_sites=5, seed=5), 0.05
    wl.left, wl.right = wl.left[:, :, :8].copy(), wl.right[:, :, :8].copy()
    return wl, 8, thr


def _material(rng):
    """Base OTs of both kinds: the evaluator's pairs, the garbler's s (kind 0's is Delta: colour bit 1)."""
    pairs = rng.integers(0, 256, (2, 128, 2, 16), dtype=np.uint8)
    s = rng.integers(0, 256, (2, 16), dtype=np.uint8)
    s[0, 0] |= 1
    return pairs, s


def _cfgs(pairs, s, mask, cb, cc, form, ss_k):
    from fuzzyheavyhitters_amd._lib import FhhEvCfg, FhhGbCfg
    gb, ev = FhhGbCfg(), FhhEvCfg()
    sbit = np.unpackbits(s, axis=1, bitorder="little")                        # [kind][128]
    chosen = np.ascontiguousarray(pairs[np.arange(2)[:, None], np.arange(128)[None, :], sbit])   # [kind][128][16]
    ctypes.memmove(gb.base_chosen, chosen.tobytes(), chosen.nbytes)
    ctypes.memmove(gb.base_choice, s.tobytes(), s.nbytes)
    ctypes.memmove(ev.base_pairs, pairs.tobytes(), pairs.nbytes)
    gb.mask = mask
    for cfg in (gb, ev):
        cfg.child_begin, cfg.child_count, cfg.form, cfg.ot_ss_k = cb, cc, form, ss_k
    return gb, ev


def _out():
    return ctypes.c_void_p(), ctypes.c_uint64()


def _host(chan, name, nbytes):
    """The message as the receiving server's buffer holds it."""
    if not nbytes:
        return np.zeros(0, np.uint8)
    return chan.bufs[name][:nbytes].cpu().numpy().copy()


def _run_chunk(gb_kc, ev_kc, cfg_gb, cfg_ev, to_gb, to_ev):
    """party.run_chunk's calls in its order, each message copied through the channel and then to the host."""
    from fuzzyheavyhitters_amd._lib import check, lib
    L = lib()
    msg = {}
    u1, u1n = _out()
    check(L.fhh_ev_ot_labels(ev_kc.handle, ctypes.byref(cfg_ev), ctypes.byref(u1), ctypes.byref(u1n)), ev_kc.handle)
    u1_rx = to_gb.send("u", u1.value or 0, u1n.value)
    msg["u1"] = _host(to_gb, "u", u1n.value)
    y1, y1n = _out()
    check(L.fhh_gb_ot_labels(gb_kc.handle, ctypes.byref(cfg_gb), ctypes.c_void_p(u1_rx), u1n.value, ctypes.byref(y1),
                             ctypes.byref(y1n)), gb_kc.handle)
    assert y1n.value == 0
    gc, gcn = _out()
    check(L.fhh_gb_garble(gb_kc.handle, ctypes.byref(gc), ctypes.byref(gcn)), gb_kc.handle)
    y1_rx = to_ev.send("y1", 0, 0)
    gc_rx = to_ev.send("gc", gc.value or 0, gcn.value)
    msg["gc"] = _host(to_ev, "gc", gcn.value)
    u2, u2n = _out()
    check(L.fhh_ev_evaluate(ev_kc.handle, ctypes.c_void_p(gc_rx), gcn.value, ctypes.c_void_p(y1_rx), 0,
                            ctypes.byref(u2), ctypes.byref(u2n)), ev_kc.handle)
    u2_rx = to_gb.send("u", u2.value or 0, u2n.value)
    msg["u2"] = _host(to_gb, "u", u2n.value)
    y2, y2n = _out()
    check(L.fhh_gb_ot_shares(gb_kc.handle, ctypes.c_void_p(u2_rx), u2n.value, ctypes.byref(y2), ctypes.byref(y2n)),
          gb_kc.handle)
    y2_rx = to_ev.send("y2", y2.value or 0, y2n.value)
    msg["y2"] = _host(to_ev, "y2", y2n.value)
    check(L.fhh_ev_ot_shares(ev_kc.handle, ctypes.c_void_p(y2_rx), y2n.value), ev_kc.handle)
    return msg


def _first_diff(got, exp):
    got, exp = np.frombuffer(bytes(got), np.uint8), np.frombuffer(bytes(exp), np.uint8)
    if got.size != exp.size:
        return f"{got.size} bytes, expected {exp.size}"
    bad = np.nonzero(got != exp)[0]
    if not bad.size:
        return None
    return f"{bad.size} of {got.size} bytes differ, first at {int(bad[0])}, last at {int(bad[-1])}"


def _check_bytes(errs, got, exp, what):
    d = _first_diff(got, exp)
    if d:
        errs.append(f"{what}: {d}")


def _check_u(errs, wire, rows, corr, m, k, what):
    """The wire U: its size, the blocks the oracle defines (tile-major), and the corrections after it."""
    if wire.size != pm.u_wire_bytes(m, k):
        errs.append(f"{what}: {wire.size} bytes, expected {pm.u_wire_bytes(m, k)}")
        return
    if not m:
        return
    exp, nb, corr_bytes = pm.expected_u_wire(rows, corr, m, k)
    R, ulen = 128 // k, 16 * pm.ot_padded(m) // k
    # the blocks the oracle defines, taken from where the tile-major layout puts them, and back in wire order
    got_rows = pm.tmaj_unpack(wire[:ulen], R, nb)
    _check_bytes(errs, pm.tmaj_pack(got_rows, pm.ot_padded(m) // 128), exp, what + " (U, wire order)")
    _check_bytes(errs, wire[ulen:], corr_bytes, what + " (the SoftSpoken corrections after U)")


class _Shard:
    def __init__(self, gb_kc, ev_kc, base, count):
        from fuzzyheavyhitters_amd import party
        self.gb, self.ev, self.base, self.count = gb_kc, ev_kc, base, count
        self.to_gb, self.to_ev = party.Channel(gb_kc.device, "copy"), party.Channel(ev_kc.device, "copy")
        self.book = pm.SessionBook()
        self.tweaks = []      # (Delta, lo, hi) per chunk
        self.chunks = []      # (level, child_begin, (ctr_off kind 0, kind 1)) per chunk
        self.material = None


def _windows(C, chunk):
    """(cfg child_begin, cfg child_count, the window's real count): chunk 0 = the whole level in one call."""
    if chunk <= 0 or C <= chunk:
        return [(0, 0, C)]
    return [(b, min(chunk, C - b), min(chunk, C - b)) for b in range(0, C, chunk)]


def _crawl_and_check(d, form, ss_k, chunk, hold=(), devices=None, levels=None, seed=1):
    """The leader's level loop (party.two_party_crawl's order: crawl, the chunks' GC + OT, node sums,
    keep_values, prune) with every chunk's messages and every level's sums compared with the model.
    `hold`: levels that keep the previous level's base material (the session counter continues).
    Returns ([(level, [window sizes])], the shards with their counter and tweak records)."""
    from fuzzyheavyhitters_amd import KeyCollection
    from fuzzyheavyhitters_amd._lib import check, lib, u32p, u64p
    wl, L, thr_frac = _workload(d)
    levels = levels or L
    c0, c1 = _keys(wl, L, d, devices=devices)
    n_total = c0.num_clients()
    thr = max(1, int(thr_frac * n_total))
    info = c0.shard_info()[0]
    if len(info) > 1:
        shards = [_Shard(c0.shard(k), c1.shard(k), b, c) for k, (_, b, c) in enumerate(info)]
    else:
        shards = [_Shard(c0, c1, 0, n_total)]
    rng = np.random.default_rng(seed)
    c0.tree_init()
    c1.tree_init()
    bits = 2 * d
    nchunk = 0
    shape = []
    for lv in range(levels):
        last = lv == L - 1
        C, pl0 = (c0.tree_crawl_last if last else c0.tree_crawl)(share_planes=True)
        C1, pl1 = (c1.tree_crawl_last if last else c1.tree_crawl)(share_planes=True)
        assert C == C1 and C > 0
        B0, B1 = pm.plane_bits(pl0, n_total), pm.plane_bits(pl1, n_total)
        exp_gv = [[0] * C for _ in shards]
        exp_ev = [[0] * C for _ in shards]
        wins = _windows(C, chunk)
        shape.append((lv, [w[2] for w in wins]))
        for k, sh in enumerate(shards):
            if sh.count == 0:
                continue
            if sh.material is None or lv not in hold:
                sh.material = _material(rng)
            pairs, s = sh.material
            b0, b1 = B0[:, :, sh.base:sh.base + sh.count], B1[:, :, sh.base:sh.base + sh.count]
            n = sh.count
            for cb, cfg_cc, cc in wins:
                mask = nchunk & 1
                nchunk += 1
                cfg_gb, cfg_ev = _cfgs(pairs, s, mask, cb, cfg_cc, form, ss_k)
                msg = _run_chunk(sh.gb, sh.ev, cfg_gb, cfg_ev, sh.to_gb, sh.to_ev)
                # the model: the counters this chunk must have used, from the model's own book
                npad = pm.npad_of(n, bits, form, last)
                m1, m2 = cc * bits * npad, (2 * cc * n if last else 0)
                ctr = (sh.book.take(0, pairs[0].tobytes() + s[0].tobytes(), m1),
                       sh.book.take(1, pairs[1].tobytes() + s[1].tobytes(), m2) if last else 0)
                r = pm.chunk_model(b0, b1, cb, cc, lv, last, form, ss_k, pairs, s, mask, ctr)
                sh.tweaks.append((s[0].tobytes(),) + pm.tweak_range(lv, cb, cc, n, bits, r["table"]))
                sh.chunks.append((lv, cb, ctr))
                what = f"level {lv} shard {k} chunk [{cb}, {cb + cc}) mask {mask} ctr {ctr}"
                assert r["m1"] == m1 and r["m2"] == m2
                errs = []
                _check_u(errs, msg["u1"], r["u1"], r["corr1"], m1, ss_k, what + " u1")
                _check_bytes(errs, msg["gc"], r["gc"], what + " gc")
                _check_u(errs, msg["u2"], r["u2"], r["corr2"], m2, ss_k, what + " u2")
                _check_bytes(errs, msg["y2"], r["y2"], what + " y2")
                assert not errs, "\n".join(errs)
                for j in range(cc):
                    exp_gv[k][cb + j] = sum(int(x) for x in r["gv"][j])
                    exp_ev[k][cb + j] = sum(int(x) for x in r["ev"][j])
        gv = [sum(exp_gv[k][c] for k in range(len(shards))) for c in range(C)]
        ev = [sum(exp_ev[k][c] for k in range(len(shards))) for c in range(C)]
        count = pm.equal_counts(B0, B1)
        if not last:
            s0, s1 = np.zeros(C, np.uint64), np.zeros(C, np.uint64)
            check(lib().fhh_party_node_sums(c0.handle, s0.ctypes.data_as(u64p), None), c0.handle)
            check(lib().fhh_party_node_sums(c1.handle, s1.ctypes.data_as(u64p), None), c1.handle)
            assert [int(x) for x in s0] == [v % pm.FE_P for v in gv], f"level {lv}: the garbler's sums"
            assert [int(x) for x in s1] == [v % pm.FE_P for v in ev], f"level {lv}: the evaluator's sums"
            assert [(int(a) - int(b)) % pm.FE_P for a, b in zip(s0, s1)] == [int(x) for x in count], f"level {lv}"
            keep = KeyCollection.keep_values(n_total, thr, s0, s1)
            c0.tree_prune(keep)
            c1.tree_prune(keep)
        else:
            got = []
            for kc in (c0, c1):
                unr, can = np.zeros((C, 10), np.uint32), np.zeros((C, 8), np.uint32)
                check(lib().fhh_party_node_sums(kc.handle, unr.ctypes.data_as(u32p), can.ctypes.data_as(u32p)),
                      kc.handle)
                got.append((unr, can))
            for (unr, can), exp, who in ((got[0], gv, "garbler"), (got[1], ev, "evaluator")):
                assert np.array_equal(unr, np.array([pm.limbs(v, 10) for v in exp])), f"last level: {who} unreduced"
                assert np.array_equal(can, np.array([pm.limbs(v % pm.FE255_P, 8) for v in exp])), f"last level: {who}"
            assert [(a - b) % pm.FE255_P for a, b in zip(gv, ev)] == [int(x) for x in count]
            s0 = [pm.limbs_int(r) for r in got[0][0]]
            s1 = [pm.limbs_int(r) for r in got[1][0]]
            keep = KeyCollection.keep_values_last(n_total, min(thr, 0xFFFFFFFF), s0, s1)
            c0.tree_prune_last(keep)
            c1.tree_prune_last(keep)
        assert keep.any(), f"level {lv}: the crawl died out"
    # counters and tweaks, from the values the model had to use to match the wire
    for sh in shards:
        for kind in (0, 1):
            assert pm.disjoint_per_key((m, lo, hi) for kd, m, lo, hi in sh.book.log if kd == kind)
        assert pm.disjoint_per_key(sh.tweaks)
    return shape, shards


def _assert_partial_last_window(shape, chunk):
    assert any(len(w) >= 3 and w[-1] < chunk for _, w in shape), shape


@pytest.mark.gpu
@pytest.mark.parametrize("ss_k", [1, 2, 4])
@pytest.mark.parametrize("chunk,hold", [(0, ()), (4, ()), (4, (3, 6, 7))], ids=["whole", "win4", "win4-held"])
def test_gpu_level_transcript_d1_table(oracle, ss_k, chunk, hold):
    """d = 1, table form: the tile-major labels OT and table kernels with the fused per-child partials
    (n = 521: two 512-test tiles per child, the second with 9 live tests), through the FieldElm level
    (the circuit, the share OT's u2 / y2 and the FieldElm sums). Whole levels and windows of 4 children
    (10 children: 4 + 4 + 2); "held": levels 3, 6 and the last keep the previous level's base OTs, so the
    session counter runs on over a level boundary and only the tweak's level bits separate the levels."""
    shape, shards = _crawl_and_check(1, 0, ss_k, chunk, hold=hold)
    assert [sum(w) for _, w in shape] == [2, 2, 4, 6, 8, 8, 10, 12]   # the plaintext crawl's children per level
    if chunk:
        _assert_partial_last_window(shape, chunk)
    first = {lv: ctr[0] for lv, cb, ctr in shards[0].chunks if cb == 0}   # each level's first labels counter
    assert all((first[lv] > 0) == (lv in hold) for lv in first), first


@pytest.mark.gpu
@pytest.mark.parametrize("ss_k", [1, 2])
@pytest.mark.parametrize("chunk", [0, 3], ids=["whole", "win3"])
def test_gpu_level_transcript_d2_table(oracle, ss_k, chunk):
    """d = 2, table form: the row-major labels and 16-row table kernels, node values stored per test
    (vals) and summed by fhh_node_sums_fe_device; n = 200, windows of 3 children."""
    shape, _ = _crawl_and_check(2, 0, ss_k, chunk)
    assert [sum(w) for _, w in shape] == [4, 8, 12, 20, 20, 20, 20, 20]   # the plaintext crawl's children per level
    if chunk:
        _assert_partial_last_window(shape, chunk)


@pytest.mark.gpu
@pytest.mark.parametrize("d", [1, 2])
def test_gpu_level_transcript_circuit_form(oracle, d):
    """form = 1: the half-gates circuit with the output-label share at every FE level; the gc message is
    [tables | y | decode]. Windows of 3 children."""
    shape, _ = _crawl_and_check(d, 1, 1, 3)
    _assert_partial_last_window(shape, 3)


@pytest.mark.gpu
def test_gpu_level_transcript_two_shards(oracle):
    """A two-shard collection (both on device 0), d = 1 table form: each shard's transcript against the
    model on that shard's clients, and the group's fhh_party_node_sums against the sum of both shards'
    expected sums, each server on its own."""
    shape, shards = _crawl_and_check(1, 0, 1, 4, devices=[0, 0], levels=7)
    assert len(shards) == 2 and all(sh.count > 0 for sh in shards) and sum(sh.count for sh in shards) == 521
    _assert_partial_last_window(shape, 4)


# ---- what the state machine refuses -----------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_follow_on_chunk_with_another_form_refused(oracle):
    """A level's storage follows the form of its first chunk: a follow-on chunk in the other form is
    refused (FHH_E_STATE) by both halves before anything is written, and the level then finishes in the
    first chunk's form with the model's sums."""
    from fuzzyheavyhitters_amd._lib import check, lib, u64p
    wl, L, _ = _workload(1)
    c0, c1 = _keys(wl, L, 1)
    c0.tree_init()
    c1.tree_init()
    C, pl0 = c0.tree_crawl(share_planes=True)
    _, pl1 = c1.tree_crawl(share_planes=True)
    assert C == 2
    n = c0.num_clients()
    b0, b1 = pm.plane_bits(pl0, n), pm.plane_bits(pl1, n)
    sh = _Shard(c0, c1, 0, n)
    pairs, s = _material(np.random.default_rng(4))
    book = pm.SessionBook()
    mat = pairs[0].tobytes() + s[0].tobytes()
    gv, ev = [], []

    def chunk(cb):
        cfg_gb, cfg_ev = _cfgs(pairs, s, cb & 1, cb, 1, 0, 1)
        msg = _run_chunk(c0, c1, cfg_gb, cfg_ev, sh.to_gb, sh.to_ev)
        r = pm.chunk_model(b0, b1, cb, 1, 0, False, 0, 1, pairs, s, cb & 1, (book.take(0, mat, 2 * 1024), 0))
        errs = []
        _check_u(errs, msg["u1"], r["u1"], None, r["m1"], 1, f"chunk {cb} u1")
        _check_bytes(errs, msg["gc"], r["gc"], f"chunk {cb} gc")
        assert not errs, "\n".join(errs)
        gv.append(sum(int(x) for x in r["gv"][0]) % pm.FE_P)
        ev.append(sum(int(x) for x in r["ev"][0]) % pm.FE_P)

    chunk(0)
    cfg_gb, cfg_ev = _cfgs(pairs, s, 1, 1, 1, 1, 1)   # chunk 1 as the circuit
    out, nb = ctypes.c_void_p(), ctypes.c_uint64()
    assert lib().fhh_ev_ot_labels(c1.handle, ctypes.byref(cfg_ev), ctypes.byref(out), ctypes.byref(nb)) == -2
    assert b"form" in lib().fhh_last_error(c1.handle)
    assert lib().fhh_gb_ot_labels(c0.handle, ctypes.byref(cfg_gb), None, 0, ctypes.byref(out), ctypes.byref(nb)) == -2
    assert b"form" in lib().fhh_last_error(c0.handle)
    chunk(1)
    s0, s1 = np.zeros(2, np.uint64), np.zeros(2, np.uint64)
    check(lib().fhh_party_node_sums(c0.handle, s0.ctypes.data_as(u64p), None), c0.handle)
    check(lib().fhh_party_node_sums(c1.handle, s1.ctypes.data_as(u64p), None), c1.handle)
    assert [int(x) for x in s0] == gv and [int(x) for x in s1] == ev


@pytest.mark.gpu
def test_gpu_shards_in_different_forms_refused(oracle):
    """fhh_party_node_sums of a group whose shards ran the level in different forms (one with the fused
    partials, one with stored values) is refused whichever shard comes first — a host-side check of the
    shards' state ahead of any device work."""
    from fuzzyheavyhitters_amd._lib import lib, u64p
    wl, L, _ = _workload(1)
    for forms in ((0, 1), (1, 0)):
        c0, c1 = _keys(wl, L, 1, devices=[0, 0])
        c0.tree_init()
        c1.tree_init()
        C, _ = c0.tree_crawl()
        c1.tree_crawl()
        rng = np.random.default_rng(6)
        for k, (_, base, cnt) in enumerate(c0.shard_info()[0]):
            assert cnt > 0
            sh = _Shard(c0.shard(k), c1.shard(k), base, cnt)
            pairs, s = _material(rng)
            cfg_gb, cfg_ev = _cfgs(pairs, s, 0, 0, 0, forms[k], 1)
            _run_chunk(sh.gb, sh.ev, cfg_gb, cfg_ev, sh.to_gb, sh.to_ev)
        sums = np.zeros(C, np.uint64)
        for kc in (c0, c1):
            assert lib().fhh_party_node_sums(kc.handle, sums.ctypes.data_as(u64p), None) == -2
            assert b"shards disagree" in lib().fhh_last_error(kc.handle)
