"""Form 2 of the two-server GC + OT (fhh_gb_cfg.form = 2): the FE levels' garbled table with its shares in
Z_2^32, at d = 1 (the tile-major kernels with the fused partials) and d = 2 (k_gt_garble<4, true> / k_gt_eval<4, true>,
u32 node values and k_ring32_child_sums).

CPU: the leader's fhh_keep_values_ring32 against Python ints, the unchanged cfg layouts, two_party_crawl's
argument checks, and the model's own consistency. GPU: every chunk's wire messages byte for byte and each
server's fhh_party_node_sums on its own against tests/party_model_ring32.py (the method of
tests/test_party_transcript.py, whose ABI driver this file reuses), what the state machine refuses, and the
drop-in crawl two_party_crawl(form="table32") against form "table" and the plaintext harness."""
import ctypes

import numpy as np
import pytest

import party_model as pm
import party_model_ring32 as pr
import test_party_transcript as drv   # the ABI driver: _keys, _material, _cfgs, _run_chunk, _check_*, _Shard, _windows

RING = 1 << 32


# ---- the leader's threshold in Z_2^32 (no GPU) --------------------------------------------------------
def _keep_ring32(thr, v0, v1):
    from fuzzyheavyhitters_amd._lib import lib, u8p, u64p
    a, b = np.asarray(v0, np.uint64), np.asarray(v1, np.uint64)
    keep = np.full(a.size, 7, np.uint8)
    rc = lib().fhh_keep_values_ring32(thr, a.ctypes.data_as(u64p), b.ctypes.data_as(u64p), a.size, keep.ctypes.data_as(u8p))
    return rc, keep


def test_keep_values_ring32_against_python_ints():
    """keep[i] = ((v0 - v1) mod 2^32) >= threshold, with wrap (v0 < v1), the ends of the range and thresholds
    1 and 2^32 - 1."""
    rng = np.random.default_rng(3)
    v0 = [int(x) for x in rng.integers(0, RING, 400)] + [0, 0, RING - 1, 5, 5, 4, 0, 1]
    v1 = [int(x) for x in rng.integers(0, RING, 400)] + [0, 1, 0, 5, 6, 5, RING - 1, 2]
    # small counts behind random shares, as the servers' sums are
    cnt = [int(x) for x in rng.integers(0, 50, 200)]
    sh = [int(x) for x in rng.integers(0, RING, 200)]
    v0 += [(c + s) % RING for c, s in zip(cnt, sh)]
    v1 += sh
    assert any(a < b for a, b in zip(v0, v1))
    for thr in (1, 2, 25, 1 << 31, RING - 1):
        rc, keep = _keep_ring32(thr, v0, v1)
        assert rc == 0
        assert [int(k) for k in keep] == [int((a - b) % RING >= thr) for a, b in zip(v0, v1)], thr
    rc, keep = _keep_ring32(1, [], [])
    assert rc == 0 and keep.size == 0
    from fuzzyheavyhitters_amd import KeyCollection
    got = KeyCollection.keep_values_ring32(1000, 25, v0[-200:], v1[-200:])
    assert got.dtype == bool and got.tolist() == [c >= 25 for c in cnt]


def test_keep_values_ring32_refuses_values_outside_the_ring():
    """FHH_E_ARG, nothing written, for a threshold or any value of 2^32 or more (FE sums fed in by mistake);
    the Python wrapper also refuses a client total of 2^32 or more."""
    from fuzzyheavyhitters_amd import KeyCollection
    from fuzzyheavyhitters_amd._lib import FhhError, lib
    ok = [1, 2, 3]
    assert _keep_ring32(RING, ok, ok)[0] == -1
    assert b"threshold" in lib().fhh_last_error(None)
    for bad0, bad1 in (([1, RING, 3], ok), (ok, [1, 2, pm.FE_P - 1]), ([1 << 63, 2, 3], ok)):
        rc, keep = _keep_ring32(1, bad0, bad1)
        assert rc == -1 and keep.tolist() == [7, 7, 7]
        assert b"2^32" in lib().fhh_last_error(None)
    rc, keep = _keep_ring32(RING - 1, [RING - 1], [0])   # the largest threshold and value still pass
    assert rc == 0 and keep.tolist() == [1]
    with pytest.raises(FhhError):
        KeyCollection.keep_values_ring32(RING, 1, ok, ok)
    with pytest.raises(FhhError):
        KeyCollection.keep_values_ring32(100, 1, [pm.FE_P - 1], [0])


def test_party_cfg_layouts_unchanged_by_form_2():
    """Form 2 rides in the existing public `form` field: sizes, offsets and field sets of fhh_gb_cfg /
    fhh_ev_cfg are what they were."""
    from fuzzyheavyhitters_amd._lib import FhhEvCfg, FhhGbCfg
    gb = 4 + 4 + 2 * 128 * 16 + 2 * 16 + 8 + 8 + 4 + 4
    ev = 2 * 128 * 2 * 16 + 4 + 4 + 8 + 8
    assert ctypes.sizeof(FhhGbCfg) == gb and ctypes.sizeof(FhhEvCfg) == ev
    assert [(f, getattr(FhhGbCfg, f).offset) for f, _ in FhhGbCfg._fields_] == [
        ("mask", 0), ("form", 4), ("base_chosen", 8), ("base_choice", 8 + 4096), ("child_begin", gb - 24),
        ("child_count", gb - 16), ("ot_ss_k", gb - 8), ("pad_", gb - 4)]
    assert [(f, getattr(FhhEvCfg, f).offset) for f, _ in FhhEvCfg._fields_] == [
        ("base_pairs", 0), ("form", 8192), ("ot_ss_k", 8196), ("child_begin", 8200), ("child_count", 8208)]
    import os
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "fhh.h")).read()
    assert "int fhh_keep_values_ring32(uint64_t threshold, const uint64_t* vals0, const uint64_t* vals1, uint64_t n," in hdr
    from fuzzyheavyhitters_amd.party import EvaluatorParty, GarblerParty
    assert GarblerParty(None).chunk_cfg([], 0, 0, 2).form == 2 and EvaluatorParty.chunk_cfg([], 0, 0, 2).form == 2


class _NoDevice:
    """A collection that must not be touched: two_party_crawl's argument checks come before any call."""

    def __init__(self, d, n):
        self.n_dims, self.depth, self._n = d, 16, n

    def num_clients(self):
        return self._n

    def __getattr__(self, name):
        raise AssertionError(f"two_party_crawl touched .{name} before refusing its arguments")


def test_two_party_crawl_table32_argument_checks():
    """form "table32": ValueError up front for d > 2 (no ring form of the circuit) and for a client total of
    2^32 or more (the count would wrap), before either collection is used; unknown forms stay refused."""
    from fuzzyheavyhitters_amd import two_party_crawl
    for d in (3, 4):
        with pytest.raises(ValueError, match="table32.*d <= 2"):
            two_party_crawl(_NoDevice(d, 100), _NoDevice(d, 100), 0.1, form="table32")
    for kw in (dict(nclients_total=RING), dict()):
        n = RING + 5 if not kw else 100
        with pytest.raises(ValueError, match="below 2\\^32"):
            two_party_crawl(_NoDevice(2, n), _NoDevice(2, n), 0.1, form="table32", **kw)
    with pytest.raises(ValueError, match="form"):
        two_party_crawl(_NoDevice(1, 100), _NoDevice(1, 100), 0.1, form="table64")
    # a valid form-2 call gets past the checks to the collection itself
    with pytest.raises(AssertionError, match="touched"):
        two_party_crawl(_NoDevice(2, 100), _NoDevice(2, 100), 0.1, form="table32")


def test_model_form_2_consistent_with_form_0(oracle):
    """The form-2 model on its own: u1 and the FE view are party_model's form 0 byte for byte, gc is half
    its length, gv - ev = eq mod 2^32 per test for both masks, d = 1 and 2, IKNP and SoftSpoken; the last
    level is form 0's chunk."""
    rng = np.random.default_rng(19)
    for d, n, k in ((1, 70, 1), (1, 70, 2), (2, 71, 1), (2, 71, 2)):
        b0 = rng.integers(0, 2, (5, 2 * d, n), dtype=np.uint8)
        b1 = b0.copy()
        b1[:, 0, ::3] ^= 1
        pairs, s = drv._material(rng)
        for mask in (0, 1):
            r = pr.chunk_model(b0, b1, 2, 3, 6, False, k, pairs, s, mask, (256, 512))
            f = pm.chunk_model(b0, b1, 2, 3, 6, False, 0, k, pairs, s, mask, (256, 512))
            assert np.array_equal(r["u1"], f["u1"]) and r["m1"] == f["m1"] and r["m2"] == 0 and f["table"]
            assert (r["corr1"] is None) == (k == 1) and (k == 1 or np.array_equal(r["corr1"], f["corr1"]))
            assert r["gc_fe"] == f["gc"] and 2 * len(r["gc"]) == len(f["gc"]) == 3 * n * ((1 << 2 * d) - 1) * 8
            assert np.array_equal(r["gv_fe"], f["gv"]) and np.array_equal(r["ev_fe"], f["ev"])
            eq = (b0[2:5] == b1[2:5]).all(axis=1)
            assert np.array_equal(((r["gv"] - r["ev"]) % RING).astype(np.uint64), eq.astype(np.uint64))
            assert all(0 <= int(x) < RING for x in r["gv"].ravel()) and all(0 <= int(x) < RING for x in r["ev"].ravel())
        r = pr.chunk_model(b0, b1, 0, 2, 7, True, k, pairs, s, 1, (0, 256))
        f = pm.chunk_model(b0, b1, 0, 2, 7, True, 0, k, pairs, s, 1, (0, 256))
        assert r["gc"] == f["gc"] and r["y2"] == f["y2"] and np.array_equal(r["gv"], f["gv"])


# ---- the transcript, level by level (GPU) -------------------------------------------------------------
def _workload(d, n=None):
    from fuzzyheavyhitters_amd import workload
    if d == 1:
        wl, thr = workload.zipf_workload(n or 521, 32, 1, num_sites=6, seed=41), 0.02
    else:
        wl, thr = workload.zipf_workload(n or 201, 32, 2, num_sites=5, seed=5), 0.05
    wl.left, wl.right = wl.left[:, :, :8].copy(), wl.right[:, :, :8].copy()
    return wl, 8, thr


def _crawl_and_check(d, ss_k, chunk, hold=(), devices=None, levels=None, n=None, seed=1):
    """test_party_transcript._crawl_and_check for form 2: the leader's level loop with every chunk's
    messages and every level's sums compared with the form-2 model, the FE levels thresholded with
    keep_values_ring32. Returns ([(level, [window sizes])], the shards)."""
    from fuzzyheavyhitters_amd import KeyCollection
    from fuzzyheavyhitters_amd._lib import check, lib, u32p, u64p
    wl, L, thr_frac = _workload(d, n)
    levels = levels or L
    c0, c1 = drv._keys(wl, L, d, devices=devices)
    n_total = c0.num_clients()
    thr = max(1, int(thr_frac * n_total))
    info = c0.shard_info()[0]
    if len(info) > 1:
        shards = [drv._Shard(c0.shard(k), c1.shard(k), b, c) for k, (_, b, c) in enumerate(info)]
    else:
        shards = [drv._Shard(c0, c1, 0, n_total)]
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
        keys = ("gv", "ev") if last else ("gv", "ev", "gv_fe", "ev_fe")
        exp = {key: [[0] * C for _ in shards] for key in keys}
        wins = drv._windows(C, chunk)
        shape.append((lv, [w[2] for w in wins]))
        for k, sh in enumerate(shards):
            if sh.count == 0:
                continue
            if sh.material is None or lv not in hold:
                sh.material = drv._material(rng)
            pairs, s = sh.material
            b0, b1 = B0[:, :, sh.base:sh.base + sh.count], B1[:, :, sh.base:sh.base + sh.count]
            nk = sh.count
            for cb, cfg_cc, cc in wins:
                mask = nchunk & 1
                nchunk += 1
                cfg_gb, cfg_ev = drv._cfgs(pairs, s, mask, cb, cfg_cc, 2, ss_k)
                msg = drv._run_chunk(sh.gb, sh.ev, cfg_gb, cfg_ev, sh.to_gb, sh.to_ev)
                npad = pm.npad_of(nk, bits, 0, last)   # form 0's padding and counters
                m1, m2 = cc * bits * npad, (2 * cc * nk if last else 0)
                ctr = (sh.book.take(0, pairs[0].tobytes() + s[0].tobytes(), m1),
                       sh.book.take(1, pairs[1].tobytes() + s[1].tobytes(), m2) if last else 0)
                r = pr.chunk_model(b0, b1, cb, cc, lv, last, ss_k, pairs, s, mask, ctr)
                sh.tweaks.append((s[0].tobytes(),) + pm.tweak_range(lv, cb, cc, nk, bits, r["table"]))
                sh.chunks.append((lv, cb, ctr))
                what = f"level {lv} shard {k} chunk [{cb}, {cb + cc}) mask {mask} ctr {ctr}"
                assert r["m1"] == m1 and r["m2"] == m2
                errs = []
                drv._check_u(errs, msg["u1"], r["u1"], r["corr1"], m1, ss_k, what + " u1")
                drv._check_bytes(errs, msg["gc"], r["gc"], what + " gc")
                drv._check_u(errs, msg["u2"], r["u2"], r["corr2"], m2, ss_k, what + " u2")
                drv._check_bytes(errs, msg["y2"], r["y2"], what + " y2")
                assert not errs, "\n".join(errs)
                if not last:   # half of form 0's message on the same labels; nothing after it
                    assert 2 * msg["gc"].size == len(r["gc_fe"]) == cc * nk * ((1 << bits) - 1) * 8, what
                    assert msg["u2"].size == 0 and msg["y2"].size == 0, what
                for key in keys:
                    for j in range(cc):
                        exp[key][k][cb + j] = sum(int(x) for x in r[key][j])
        tot = {key: [sum(exp[key][k][c] for k in range(len(shards))) for c in range(C)] for key in keys}
        count = pm.equal_counts(B0, B1)
        if not last:
            s0, s1 = np.full(C, 1 << 63, np.uint64), np.full(C, 1 << 63, np.uint64)
            check(lib().fhh_party_node_sums(c0.handle, s0.ctypes.data_as(u64p), None), c0.handle)
            check(lib().fhh_party_node_sums(c1.handle, s1.ctypes.data_as(u64p), None), c1.handle)
            # (for several shards: each shard model's sum mod 2^32, added mod 2^32)
            assert [int(x) for x in s0] == [v % RING for v in tot["gv"]], f"level {lv}: the garbler's sums"
            assert [int(x) for x in s1] == [v % RING for v in tot["ev"]], f"level {lv}: the evaluator's sums"
            assert [(int(a) - int(b)) % RING for a, b in zip(s0, s1)] == [int(x) for x in count], f"level {lv}"
            keep = KeyCollection.keep_values_ring32(n_total, thr, s0, s1)
            fe0 = np.array([v % pm.FE_P for v in tot["gv_fe"]], np.uint64)
            fe1 = np.array([v % pm.FE_P for v in tot["ev_fe"]], np.uint64)
            assert np.array_equal(keep, KeyCollection.keep_values(n_total, thr, fe0, fe1)), f"level {lv}: keep"
            c0.tree_prune(keep)
            c1.tree_prune(keep)
        else:   # the FieldElm level, exactly as in form 0
            got = []
            for kc in (c0, c1):
                unr, can = np.zeros((C, 10), np.uint32), np.zeros((C, 8), np.uint32)
                check(lib().fhh_party_node_sums(kc.handle, unr.ctypes.data_as(u32p), can.ctypes.data_as(u32p)),
                      kc.handle)
                got.append((unr, can))
            for (unr, can), e, who in ((got[0], tot["gv"], "garbler"), (got[1], tot["ev"], "evaluator")):
                assert np.array_equal(unr, np.array([pm.limbs(v, 10) for v in e])), f"last level: {who} unreduced"
                assert np.array_equal(can, np.array([pm.limbs(v % pm.FE255_P, 8) for v in e])), f"last level: {who}"
            assert [(a - b) % pm.FE255_P for a, b in zip(tot["gv"], tot["ev"])] == [int(x) for x in count]
            keep = KeyCollection.keep_values_last(n_total, min(thr, 0xFFFFFFFF), [pm.limbs_int(r) for r in got[0][0]],
                                                  [pm.limbs_int(r) for r in got[1][0]])
            c0.tree_prune_last(keep)
            c1.tree_prune_last(keep)
        assert keep.any(), f"level {lv}: the crawl died out"
    for sh in shards:   # counters and tweaks, from the values the model had to use to match the wire
        for kind in (0, 1):
            assert pm.disjoint_per_key((m, lo, hi) for kd, m, lo, hi in sh.book.log if kd == kind)
        assert pm.disjoint_per_key(sh.tweaks)
    return shape, shards


@pytest.mark.gpu
@pytest.mark.parametrize("ss_k,chunk,hold", [(1, 0, ()), (2, 0, ()), (1, 3, ()), (2, 3, ()), (2, 3, (3, 6, 7))],
                         ids=["iknp-whole", "ss2-whole", "iknp-win3", "ss2-win3", "ss2-win3-held"])
def test_gpu_form2_transcript_d1(oracle, ss_k, chunk, hold):
    """d = 1: the tile-major table kernels in their Z_2^32 form with the fused per-child partials (n = 521: two
    512-test tiles per child), through the FieldElm level. Windows of 3 children give odd test counts (3 x 521),
    so the message rows are only 4-B aligned; "held": levels 3, 6 and the last keep the previous level's base OTs."""
    shape, shards = _crawl_and_check(1, ss_k, chunk, hold=hold)
    assert [sum(w) for _, w in shape] == [2, 2, 4, 6, 8, 8, 10, 12]   # the plaintext crawl's children per level
    if chunk:
        drv._assert_partial_last_window(shape, chunk)
    first = {lv: ctr[0] for lv, cb, ctr in shards[0].chunks if cb == 0}
    assert all((first[lv] > 0) == (lv in hold) for lv in first), first


@pytest.mark.gpu
@pytest.mark.parametrize("ss_k", [1, 2])
@pytest.mark.parametrize("chunk", [0, 3], ids=["whole", "win3"])
def test_gpu_form2_transcript_d2(oracle, ss_k, chunk):
    """d = 2: the row-major labels, k_gt_garble<4, true> / k_gt_eval<4, true> (15 rows of u32 per test), u32 node values
    summed by k_ring32_child_sums; n = 201 (odd: rows 4-B aligned only), windows of 3 children."""
    shape, _ = _crawl_and_check(2, ss_k, chunk)
    assert [sum(w) for _, w in shape] == [4, 8, 12, 20, 20, 20, 20, 20]   # the plaintext crawl's children per level
    if chunk:
        drv._assert_partial_last_window(shape, chunk)


@pytest.mark.gpu
def test_gpu_form2_transcript_d2_wide(oracle):
    """d = 2 at n = 16385, the first two levels: a child's values span five 4096-value sum blocks, the last
    with a single value."""
    shape, _ = _crawl_and_check(2, 1, 0, levels=2, n=16385)
    assert [sum(w) for _, w in shape] == [4, 8]


@pytest.mark.gpu
@pytest.mark.parametrize("d", [1, 2])
def test_gpu_form2_transcript_two_shards(oracle, d):
    """A two-shard collection (both on device 0): each shard's transcript against the model on that shard's
    clients, and the group's fhh_party_node_sums against the shard models' sums added mod 2^32. Windows of 4
    children at d = 1 and of 3 at d = 2 (whose levels hold 4, 8, 12, 20 children), so a level ends in a partial one."""
    chunk = 4 if d == 1 else 3
    shape, shards = _crawl_and_check(d, 1, chunk, devices=[0, 0], levels=7)
    assert len(shards) == 2 and all(sh.count > 0 for sh in shards)
    assert sum(sh.count for sh in shards) == (521 if d == 1 else 201)
    drv._assert_partial_last_window(shape, chunk)


# ---- what the state machine refuses (GPU) -------------------------------------------------------------
def _labels_rc(c0, c1, cfg_gb, cfg_ev):
    """(rc, message) of both halves' *_ot_labels calls."""
    from fuzzyheavyhitters_amd._lib import lib
    out, nb = ctypes.c_void_p(), ctypes.c_uint64()
    rc1 = lib().fhh_ev_ot_labels(c1.handle, ctypes.byref(cfg_ev), ctypes.byref(out), ctypes.byref(nb))
    e1 = lib().fhh_last_error(c1.handle)
    rc0 = lib().fhh_gb_ot_labels(c0.handle, ctypes.byref(cfg_gb), None, 0, ctypes.byref(out), ctypes.byref(nb))
    return (rc0, lib().fhh_last_error(c0.handle)), (rc1, e1)


@pytest.mark.gpu
@pytest.mark.parametrize("first,other", [(2, 0), (0, 2)], ids=["2-then-0", "0-then-2"])
def test_gpu_follow_on_chunk_between_forms_0_and_2_refused(oracle, first, other):
    """Forms 0 and 2 are both fused at d = 1, but their storage is not interchangeable: a follow-on chunk in the
    other form is refused (FHH_E_STATE) by both halves, and the level then finishes in the first chunk's
    form with the model's sums."""
    from fuzzyheavyhitters_amd._lib import check, lib, u64p
    wl, L, _ = _workload(1)
    c0, c1 = drv._keys(wl, L, 1)
    c0.tree_init()
    c1.tree_init()
    C, pl0 = c0.tree_crawl(share_planes=True)
    _, pl1 = c1.tree_crawl(share_planes=True)
    assert C == 2
    n = c0.num_clients()
    b0, b1 = pm.plane_bits(pl0, n), pm.plane_bits(pl1, n)
    sh = drv._Shard(c0, c1, 0, n)
    pairs, s = drv._material(np.random.default_rng(4))
    book = pm.SessionBook()
    mat = pairs[0].tobytes() + s[0].tobytes()
    gv, ev = [], []

    def chunk(cb):
        cfg_gb, cfg_ev = drv._cfgs(pairs, s, cb & 1, cb, 1, first, 1)
        msg = drv._run_chunk(c0, c1, cfg_gb, cfg_ev, sh.to_gb, sh.to_ev)
        ctr = (book.take(0, mat, 2 * 1024), 0)
        if first == 2:
            r = pr.chunk_model(b0, b1, cb, 1, 0, False, 1, pairs, s, cb & 1, ctr)
        else:
            r = pm.chunk_model(b0, b1, cb, 1, 0, False, 0, 1, pairs, s, cb & 1, ctr)
        errs = []
        drv._check_u(errs, msg["u1"], r["u1"], None, r["m1"], 1, f"chunk {cb} u1")
        drv._check_bytes(errs, msg["gc"], r["gc"], f"chunk {cb} gc")
        assert not errs, "\n".join(errs)
        mod = RING if first == 2 else pm.FE_P
        gv.append(sum(int(x) for x in r["gv"][0]) % mod)
        ev.append(sum(int(x) for x in r["ev"][0]) % mod)

    chunk(0)
    cfg_gb, cfg_ev = drv._cfgs(pairs, s, 1, 1, 1, other, 1)
    for rc, err in _labels_rc(c0, c1, cfg_gb, cfg_ev):
        assert rc == -2 and b"form" in err, (rc, err)
    chunk(1)
    s0, s1 = np.zeros(2, np.uint64), np.zeros(2, np.uint64)
    check(lib().fhh_party_node_sums(c0.handle, s0.ctypes.data_as(u64p), None), c0.handle)
    check(lib().fhh_party_node_sums(c1.handle, s1.ctypes.data_as(u64p), None), c1.handle)
    assert [int(x) for x in s0] == gv and [int(x) for x in s1] == ev


@pytest.mark.gpu
def test_gpu_form_2_refused_at_d3_and_form_3_anywhere(oracle):
    """2d > 4 has no table and the circuit has no ring form: form 2 is FHH_E_ARG from both halves, with "form"
    in the message (FE sums must not reach a leader that asked for Z_2^32); form 3 stays refused."""
    from fuzzyheavyhitters_amd import workload
    wl = workload.zipf_workload(64, 32, 3, num_sites=3, seed=2)
    wl.left, wl.right = wl.left[:, :, :4].copy(), wl.right[:, :, :4].copy()
    c0, c1 = drv._keys(wl, 4, 3)
    c0.tree_init()
    c1.tree_init()
    c0.tree_crawl()
    c1.tree_crawl()
    pairs, s = drv._material(np.random.default_rng(8))
    for form in (2, 3):
        cfg_gb, cfg_ev = drv._cfgs(pairs, s, 0, 0, 0, form, 1)
        for rc, err in _labels_rc(c0, c1, cfg_gb, cfg_ev):
            assert rc == -1 and b"form" in err, (form, rc, err)


@pytest.mark.gpu
def test_gpu_shards_in_forms_0_and_2_refused(oracle):
    """fhh_party_node_sums of a group whose shards ran one level in forms 0 and 2 — both with the fused
    partials at d = 1, so only the form itself tells them apart — is refused whichever shard comes first."""
    from fuzzyheavyhitters_amd._lib import lib, u64p
    wl, L, _ = _workload(1)
    for forms in ((0, 2), (2, 0)):
        c0, c1 = drv._keys(wl, L, 1, devices=[0, 0])
        c0.tree_init()
        c1.tree_init()
        C, _ = c0.tree_crawl()
        c1.tree_crawl()
        rng = np.random.default_rng(6)
        for k, (_, base, cnt) in enumerate(c0.shard_info()[0]):
            assert cnt > 0
            sh = drv._Shard(c0.shard(k), c1.shard(k), base, cnt)
            pairs, s = drv._material(rng)
            cfg_gb, cfg_ev = drv._cfgs(pairs, s, 0, 0, 0, forms[k], 1)
            drv._run_chunk(sh.gb, sh.ev, cfg_gb, cfg_ev, sh.to_gb, sh.to_ev)
        sums = np.zeros(C, np.uint64)
        for kc in (c0, c1):
            assert lib().fhh_party_node_sums(kc.handle, sums.ctypes.data_as(u64p), None) == -2
            assert b"shards disagree" in lib().fhh_last_error(kc.handle)


# ---- end to end (GPU) ---------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["zipf_d1", "zipf_d2"])
def test_gpu_two_party_crawl_table32_equals_table_and_plain(kind):
    """two_party_crawl(form="table32", ot_ss_k=2) with fresh material (real CO15 base OTs): the same level
    children, per-level counts and final (path, value) set as form "table" on the same keys and as the plain
    sim_crawl; the gc bytes are exactly half of form "table"'s at every FE level and equal at the last."""
    import fuzzyheavyhitters_amd as fhh
    from fuzzyheavyhitters_amd import workload
    if kind == "zipf_d1":
        wl, L, d, thr = workload.zipf_workload(3000, 64, 1, num_sites=40, seed=5), 64, 1, 0.01
    else:
        wl, L, d, thr = workload.zipf_workload(1000, 32, 2, num_sites=5, seed=62), 12, 2, 0.05
        wl.left, wl.right = wl.left[:, :, :L].copy(), wl.right[:, :, :L].copy()
    c0, c1 = drv._keys(wl, L, d)
    plain = fhh.sim_crawl(c0, c1, thr, mode="fe", prf_seed=9)
    got = fhh.two_party_crawl(c0, c1, thr, form="table32", ot_ss_k=2)
    ref = fhh.two_party_crawl(c0, c1, thr, form="table", ot_ss_k=2)
    assert len(got.final) > 0

    def sig(r):
        return ([int(x) for x in r.level_children], [np.asarray(c, np.uint64).tolist() for c in r.counts],
                [(r_.path, r_.value) for r_ in r.final])

    assert sig(got) == sig(ref)
    assert sig(got) == sig(plain)
    assert len(got.level_bytes) == len(ref.level_bytes) == L
    for lv, (a, b) in enumerate(zip(got.level_bytes, ref.level_bytes)):
        if lv < L - 1:
            assert 2 * a["gc"] == b["gc"] and a["gc"] > 0, lv
            assert a["u2"] == 0 and a["y2"] == 0, lv
        else:
            assert a["gc"] == b["gc"] and a["y2"] == b["y2"] > 0
        assert a["u1"] == b["u1"], lv
