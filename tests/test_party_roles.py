"""A level's garbling split between the two servers: per-chunk roles (two protocol instances per ctx, the sign
of the node sums under fhh_party_set_server, fhh_party_role_plan, two_party_crawl(roles=...)).

The reference of every comparison is workload.plaintext_crawl (tests/party_roles_cases.py) or the oracle through
tests/party_model.py; roles="fixed" of the code under test appears only as the second witness of
test_gpu_fixed_roles_unchanged_by_the_server_setting."""
import ctypes

import numpy as np
import pytest

import party_model as pm
import party_roles_cases as prc
import test_party_transcript as tpt

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -2


def _keys(d, devices=None, wl=None):
    import fuzzyheavyhitters_amd as fhh
    wl0, L = prc.workload_of(d)
    wl = wl or wl0
    c0 = fhh.KeyCollection(L, d, devices=devices)
    c1 = fhh.KeyCollection(L, d, devices=devices)
    fhh.gen_keys_pair(c0, c1, wl.left, wl.right, wl.root_seeds)
    return c0, c1


def _garblers_of_level(C, chunk, lv, roles):
    """Per child: the server that garbles it, restated from the issue (not read from the code under test)."""
    split = roles == "split"
    out = []
    for w, cc in enumerate(prc.windows_of(C, chunk, split)):
        out += [{"fixed": 0, "swapped": 1, "level": lv & 1, "split": (lv + w) & 1}[roles]] * cc
    return out


def _assert_equals_plaintext(res, d):
    counts, finals = prc.plaintext_of(d)
    assert [int(c) for c in res.level_children] == [len(c) for c in counts]
    for lv, (got, exp) in enumerate(zip(res.counts, counts)):
        assert np.array_equal(np.asarray(got, np.uint64), exp), f"level {lv}"
    # the kept lists: the children of level lv + 1 are the kept ones of level lv times 2^d
    for lv in range(len(counts) - 1):
        assert int(res.level_children[lv + 1]) == int((counts[lv] >= 1).sum()) << d, f"level {lv}"
    assert prc.final_set(res) == finals


# ---- 1. every mode equals plaintext -------------------------------------------------------------------
@pytest.mark.parametrize("ss_k", [1, 2])
@pytest.mark.parametrize("form", ["table", "circuit", "table32"])
@pytest.mark.parametrize("roles", ["swapped", "level", "split"])
@pytest.mark.parametrize("d", [1, 2])
def test_gpu_roles_equal_plaintext(d, roles, form, ss_k):
    """Counts of every level (expect_counts raises at the first level that differs), the kept lists and the final
    (path, value) set equal the plaintext crawl, in windows of 3 children (several windows, a partial last one,
    a window left without a partner), whoever garbles."""
    import fuzzyheavyhitters_amd as fhh
    counts, _ = prc.plaintext_of(d)
    c0, c1 = _keys(d)
    res = fhh.two_party_crawl(c0, c1, prc.THRESHOLD, material="test", prf_seed=0xA11CE + d, chunk_children=prc.CHUNK,
                              form=form, ot_ss_k=ss_k, roles=roles, expect_counts=counts)
    _assert_equals_plaintext(res, d)
    # every chunk message is counted once, in the direction it travelled
    assert res.direction_bytes[0] > 0 and res.direction_bytes[1] > 0
    assert sum(res.direction_bytes) == sum(sum(lb.values()) for lb in res.level_bytes)


@pytest.mark.parametrize("d", [1, 2])
def test_gpu_split_whole_level_cut_in_two(d):
    """chunk_children = 0: every level is one window today, which the split cuts into ceil(C / 2) and
    floor(C / 2) (C = 2: two one-child windows; C = 10: two odd windows of 5)."""
    import fuzzyheavyhitters_amd as fhh
    counts, _ = prc.plaintext_of(d)
    c0, c1 = _keys(d)
    res = fhh.two_party_crawl(c0, c1, prc.THRESHOLD, material="test", prf_seed=5, chunk_children=0, roles="split",
                              expect_counts=counts)
    _assert_equals_plaintext(res, d)


@pytest.mark.parametrize("d", [1, 2])
def test_gpu_split_fresh_material(d):
    """material="fresh": each server draws its own Delta, masks and CO15 seeds, and real Chou-Orlandi base OTs run
    in both directions for every level (labels; + the share OT's at the FieldElm level)."""
    import fuzzyheavyhitters_amd as fhh
    counts, _ = prc.plaintext_of(d)
    _, L = prc.workload_of(d)
    c0, c1 = _keys(d)
    res = fhh.two_party_crawl(c0, c1, prc.THRESHOLD, chunk_children=prc.CHUNK, roles="split", expect_counts=counts)
    _assert_equals_plaintext(res, d)
    assert res.base_ot_runs == 2 * (L + 1) and res.base_ot_bytes == 2 * (L + 1) * 65 * 129


# ---- 3. the last level --------------------------------------------------------------------------------
@pytest.mark.parametrize("roles", ["swapped", "split"])
@pytest.mark.parametrize("d", [1, 2])
def test_gpu_last_level_garbled_by_server_1(d, roles):
    """final_values(c0.final_shares(), c1.final_shares()) equals the plaintext heavy hitters when server 1 garbled
    all ("swapped") or some ("split") of the last level's children: the recorded FieldElm values carry the sign."""
    import fuzzyheavyhitters_amd as fhh
    from fuzzyheavyhitters_amd import KeyCollection
    counts, finals = prc.plaintext_of(d)
    _, L = prc.workload_of(d)
    who = _garblers_of_level(len(counts[-1]), prc.CHUNK, L - 1, roles)
    assert 1 in who and (roles == "swapped" or 0 in who)
    kept = [g for g, c in zip(who, counts[-1]) if c >= 1]
    assert 1 in kept          # a heavy hitter whose last-level test server 1 garbled
    c0, c1 = _keys(d)
    fhh.two_party_crawl(c0, c1, prc.THRESHOLD, material="test", prf_seed=9, chunk_children=prc.CHUNK, roles=roles)
    final = KeyCollection.final_values(c0.final_shares(), c1.final_shares())
    got = {tuple(tuple(int(b) for b in p) for p in r.path): int(r.value) for r in final}
    assert got == finals


# ---- 4. two shards ------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 2])
def test_gpu_split_two_shards(d):
    """A split crawl on 2 shards per server (both on device 0) equals the one-GPU split crawl and plaintext, level
    by level. Shard 1's base is off a word boundary: three extra clients keyed into shard 0 are retained away
    first, so the survivors are exactly the one-GPU population."""
    import copy
    import fuzzyheavyhitters_amd as fhh
    counts, _ = prc.plaintext_of(d)
    wl, L = prc.workload_of(d)
    big = copy.copy(wl)
    at = [1, 1, 1]
    for name in ("alpha", "left", "right", "root_seeds", "site_of_client"):
        setattr(big, name, np.ascontiguousarray(np.insert(getattr(wl, name), at, getattr(wl, name)[7:10], axis=0)))
    keep = np.ones(prc.N_CLIENTS + 3, np.uint8)
    keep[1:4] = 0
    g0, g1 = _keys(d, devices=[0, 0], wl=big)
    for g in (g0, g1):
        g.tree_init()
        g.retain_clients(keep)
    two = fhh.two_party_crawl(g0, g1, prc.THRESHOLD, material="test", prf_seed=31, chunk_children=prc.CHUNK,
                              roles="split", expect_counts=counts)
    info = g0.shard_info()[0]
    assert len(info) == 2 and all(m > 0 for _, _, m in info) and sum(m for _, _, m in info) == prc.N_CLIENTS
    assert info[1][1] % 64 != 0, info
    _assert_equals_plaintext(two, d)
    c0, c1 = _keys(d)
    one = fhh.two_party_crawl(c0, c1, prc.THRESHOLD, material="test", prf_seed=31, chunk_children=prc.CHUNK,
                              roles="split", expect_counts=counts)
    assert list(one.level_children) == list(two.level_children)
    for lv, (a, b) in enumerate(zip(one.counts, two.counts)):
        assert np.array_equal(a, b), f"level {lv}"
    assert prc.final_set(one) == prc.final_set(two)


# ---- 6. second witness: nothing changes with the default roles -------------------------------------------
@pytest.mark.parametrize("material", ["fresh", "test"])
def test_gpu_fixed_roles_unchanged_by_the_server_setting(material, monkeypatch):
    """roles="fixed" with the default arguments: level_bytes, counts and finals are identical to a run on fresh
    collections on which fhh_party_set_server was never called (the loop's call is patched out for that run),
    and both equal plaintext."""
    import fuzzyheavyhitters_amd as fhh
    from fuzzyheavyhitters_amd import KeyCollection
    d = 1
    called = []
    with monkeypatch.context() as m:
        m.setattr(KeyCollection, "party_set_server", lambda self, server: called.append(server))
        c0, c1 = _keys(d)
        before = fhh.two_party_crawl(c0, c1, prc.THRESHOLD, material=material)
    assert called == [0, 1]
    p0, p1 = _keys(d)
    after = fhh.two_party_crawl(p0, p1, prc.THRESHOLD, material=material)
    assert before.level_bytes == after.level_bytes
    assert all(lb.keys() == {"u1", "y1", "gc", "u2", "y2"} for lb in after.level_bytes)
    assert list(before.level_children) == list(after.level_children)
    for a, b in zip(before.counts, after.counts):
        assert np.array_equal(a, b)
    assert [(r.path, r.value) for r in before.final] == [(r.path, r.value) for r in after.final]
    assert (before.base_ot_runs, before.base_ot_bytes) == (after.base_ot_runs, after.base_ot_bytes)
    assert after.direction_bytes[1] > 0 and sum(after.direction_bytes) == sum(sum(lb.values()) for lb in after.level_bytes)
    _assert_equals_plaintext(after, d)


# ---- driving the ABI window by window -----------------------------------------------------------------
class _Win:
    """One window between its garbling and its evaluating collection, stage by stage (the order a split level
    interleaves), every message copied through a channel of its own direction and then to the host."""

    def __init__(self, servers, g, cfg_gb, cfg_ev, chans):
        self.gb, self.ev, self.g = servers[g], servers[1 - g], g
        self.cfg_gb, self.cfg_ev = cfg_gb, cfg_ev
        self.to_gb, self.to_ev = chans[g]
        self.msg = {}

    def labels(self):
        from fuzzyheavyhitters_amd._lib import check, lib
        u1, u1n = tpt._out()
        check(lib().fhh_ev_ot_labels(self.ev.handle, ctypes.byref(self.cfg_ev), ctypes.byref(u1), ctypes.byref(u1n)),
              self.ev.handle)
        rx = self.to_gb.send("u", u1.value or 0, u1n.value)
        self.msg["u1"] = tpt._host(self.to_gb, "u", u1n.value)
        y1, y1n = tpt._out()
        check(lib().fhh_gb_ot_labels(self.gb.handle, ctypes.byref(self.cfg_gb), ctypes.c_void_p(rx), u1n.value,
                                     ctypes.byref(y1), ctypes.byref(y1n)), self.gb.handle)
        assert y1n.value == 0

    def garble(self):
        from fuzzyheavyhitters_amd._lib import check, lib
        gc, gcn = tpt._out()
        check(lib().fhh_gb_garble(self.gb.handle, ctypes.byref(gc), ctypes.byref(gcn)), self.gb.handle)
        self.gc_rx, self.gcn = self.to_ev.send("gc", gc.value or 0, gcn.value), gcn.value
        self.msg["gc"] = tpt._host(self.to_ev, "gc", gcn.value)

    def evaluate(self):
        from fuzzyheavyhitters_amd._lib import check, lib
        u2, u2n = tpt._out()
        check(lib().fhh_ev_evaluate(self.ev.handle, ctypes.c_void_p(self.gc_rx), self.gcn, None, 0, ctypes.byref(u2),
                                    ctypes.byref(u2n)), self.ev.handle)
        self.u2_rx, self.u2n = self.to_gb.send("u", u2.value or 0, u2n.value), u2n.value
        self.msg["u2"] = tpt._host(self.to_gb, "u", u2n.value)

    def shares(self):
        from fuzzyheavyhitters_amd._lib import check, lib
        y2, y2n = tpt._out()
        check(lib().fhh_gb_ot_shares(self.gb.handle, ctypes.c_void_p(self.u2_rx), self.u2n, ctypes.byref(y2),
                                     ctypes.byref(y2n)), self.gb.handle)
        rx = self.to_ev.send("y2", y2.value or 0, y2n.value)
        self.msg["y2"] = tpt._host(self.to_ev, "y2", y2n.value)
        check(lib().fhh_ev_ot_shares(self.ev.handle, ctypes.c_void_p(rx), y2n.value), self.ev.handle)

    def run(self):
        for st in (self.labels, self.garble, self.evaluate, self.shares):
            st()


def _run_split(wins):
    """Pairs (w, w') garbled by different servers in the split level's order; a window left over on its own."""
    at = 0
    while at < len(wins):
        pair = wins[at:at + 2] if at + 1 < len(wins) and wins[at].g != wins[at + 1].g else wins[at:at + 1]
        for st in ("labels", "garble", "evaluate", "shares"):
            for w in pair:
                getattr(w, st)()
        at += len(pair)


def _channels(c0, c1):
    from fuzzyheavyhitters_amd import party
    # direction g: (to the garbler = server g, to the evaluator = server 1 - g)
    return [(party.Channel(c0.device, "copy"), party.Channel(c1.device, "copy")),
            (party.Channel(c1.device, "copy"), party.Channel(c0.device, "copy"))]


def _flipped(server, garbler):
    """The sign rule: server 0 negates what it evaluated, server 1 what it garbled."""
    evaluated = server != garbler
    return (server == 0 and evaluated) or (server == 1 and not evaluated)


def _signed(v, server, garbler, mod):
    return (-v) % mod if _flipped(server, garbler) else v


# ---- 2. each server pinned on its own in a split level ---------------------------------------------------
def _split_transcript(d, form, ss_k, chunk, hold=(), levels=None, seed=1):
    """tests/test_party_transcript.py's level loop with the windows' roles split: every chunk's messages against
    the oracle with the garbling server's planes as the garbler's bits, the row-PRG counters from one book per
    (ctx, role), and each server's fhh_party_node_sums against the oracle's per-party sums under the sign rule."""
    from fuzzyheavyhitters_amd import KeyCollection
    from fuzzyheavyhitters_amd._lib import check, lib, u32p, u64p
    wl, L, thr_frac = tpt._workload(d)
    levels = levels or L
    c0, c1 = tpt._keys(wl, L, d)
    servers = (c0, c1)
    n = c0.num_clients()
    thr = max(1, int(thr_frac * n))
    chans = _channels(c0, c1)
    books = {(s, role): pm.SessionBook() for s in (0, 1) for role in ("gb", "ev")}
    material = [None, None]          # per direction
    tweaks = [[], []]                # per garbling server: (Delta, lo, hi)
    rng = np.random.default_rng(seed)
    c0.tree_init()
    c1.tree_init()
    c0.party_set_server(0)
    c1.party_set_server(1)
    bits, nchunk, shape = 2 * d, 0, []
    for lv in range(levels):
        last = lv == L - 1
        C, pl0 = (c0.tree_crawl_last if last else c0.tree_crawl)(share_planes=True)
        C1, pl1 = (c1.tree_crawl_last if last else c1.tree_crawl)(share_planes=True)
        assert C == C1 and C > 0
        B = (pm.plane_bits(pl0, n), pm.plane_bits(pl1, n))
        sizes = prc.windows_of(C, chunk, True)
        shape.append((lv, sizes))
        for g in (0, 1):
            if material[g] is None or lv not in hold:
                material[g] = tpt._material(rng)
        wins, models, cb = [], [], 0
        for w, cc in enumerate(sizes):
            g = (lv + w) & 1
            pairs, s = material[g]
            mask = nchunk & 1
            nchunk += 1
            cfg_gb, cfg_ev = tpt._cfgs(pairs, s, mask, cb, cc, form, ss_k)
            wins.append(_Win(servers, g, cfg_gb, cfg_ev, chans))
            # the counters this chunk must use: the garbling ctx's garbler book and the evaluating ctx's evaluator
            # book, which run through the same sequence of this direction's chunks
            npad = pm.npad_of(n, bits, form, last)
            m1, m2 = cc * bits * npad, (2 * cc * n if last else 0)
            mat = [pairs[k].tobytes() + s[k].tobytes() for k in (0, 1)]
            ctr = tuple((books[key].take(0, mat[0], m1), books[key].take(1, mat[1], m2) if last else 0)
                        for key in ((g, "gb"), (1 - g, "ev")))
            assert ctr[0] == ctr[1]
            r = pm.chunk_model(B[g], B[1 - g], cb, cc, lv, last, form, ss_k, pairs, s, mask, ctr[0])
            assert r["m1"] == m1 and r["m2"] == m2
            tweaks[g].append((s[0].tobytes(),) + pm.tweak_range(lv, cb, cc, n, bits, r["table"]))
            models.append((g, cb, cc, mask, ctr[0], r))
            cb += cc
        assert cb == C and len({w.g for w in wins}) == 2
        _run_split(wins)
        exp = [[0] * C, [0] * C]
        mod = pm.FE255_P if last else pm.FE_P
        for win, (g, cb, cc, mask, ctr, r) in zip(wins, models):
            what = f"level {lv} chunk [{cb}, {cb + cc}) garbled by server {g} mask {mask} ctr {ctr}"
            errs = []
            tpt._check_u(errs, win.msg["u1"], r["u1"], r["corr1"], r["m1"], ss_k, what + " u1")
            tpt._check_bytes(errs, win.msg["gc"], r["gc"], what + " gc")
            tpt._check_u(errs, win.msg["u2"], r["u2"], r["corr2"], r["m2"], ss_k, what + " u2")
            tpt._check_bytes(errs, win.msg["y2"], r["y2"], what + " y2")
            assert not errs, "\n".join(errs)
            for j in range(cc):
                gv, ev = sum(int(x) for x in r["gv"][j]), sum(int(x) for x in r["ev"][j])
                exp[g][cb + j] = (gv, g)
                exp[1 - g][cb + j] = (ev, g)
        count = [int(x) for x in pm.equal_counts(B[0], B[1])]
        if not last:
            got = []
            for s, kc in enumerate(servers):
                out = np.zeros(C, np.uint64)
                check(lib().fhh_party_node_sums(kc.handle, out.ctypes.data_as(u64p), None), kc.handle)
                assert [int(x) for x in out] == [_signed(v % mod, s, g, mod) for v, g in exp[s]], f"level {lv} server {s}"
                got.append(out)
            assert [(int(a) - int(b)) % mod for a, b in zip(*got)] == count, f"level {lv}"
            keep = KeyCollection.keep_values(n, thr, got[0], got[1])
            c0.tree_prune(keep)
            c1.tree_prune(keep)
        else:
            got = []
            for s, kc in enumerate(servers):
                unr, can = np.zeros((C, 10), np.uint32), np.zeros((C, 8), np.uint32)
                check(lib().fhh_party_node_sums(kc.handle, unr.ctypes.data_as(u32p), can.ctypes.data_as(u32p)), kc.handle)
                # a negated child's unreduced output is the canonical negated value, zero-extended
                e_unr = [(-v) % mod if _flipped(s, g) else v for v, g in exp[s]]
                assert np.array_equal(unr, np.array([pm.limbs(v, 10) for v in e_unr])), f"last level server {s} unreduced"
                assert np.array_equal(can, np.array([pm.limbs(v % mod, 8) for v in e_unr])), f"last level server {s}"
                got.append([pm.limbs_int(r) for r in unr])
            assert [(a - b) % mod for a, b in zip(*got)] == count
            keep = KeyCollection.keep_values_last(n, min(thr, 0xFFFFFFFF), got[0], got[1])
            c0.tree_prune_last(keep)
            c1.tree_prune_last(keep)
            # fhh_final_shares hands out the recorded (signed) values: the leader's final_values needs no change
            final = KeyCollection.final_values(c0.final_shares(), c1.final_shares())
            assert sorted(int(r.value) for r in final) == sorted(c for c, k in zip(count, keep) if k)
        assert keep.any(), f"level {lv}: the crawl died out"
    # counters per (ctx, role) and tweaks per garbling server, from the values the model had to use to match the wire
    for key, book in books.items():
        for kind in (0, 1):
            assert pm.disjoint_per_key((m, lo, hi) for kd, m, lo, hi in book.log if kd == kind), key
        assert book.log, key          # every (ctx, role) ran chunks
    for g in (0, 1):
        assert pm.disjoint_per_key(tweaks[g])
    return shape, books


@pytest.mark.parametrize("ss_k,hold", [(1, ()), (2, (3, 6, 7))], ids=["iknp", "softspoken-held"])
def test_gpu_split_transcript_d1_table(oracle, ss_k, hold):
    """d = 1, table form (the tile-major kernels and the fused partials: both slot pairs of a ctx are in use in
    one level), through the FieldElm level (the share OT in both directions, the FieldElm sums negated where the
    rule says). "held": levels 3, 6 and the last keep both directions' base OTs, so each (ctx, role) counter
    runs on over level boundaries."""
    shape, books = _split_transcript(1, 0, ss_k, 3, hold=hold)
    assert [sum(w) for _, w in shape] == [2, 2, 4, 6, 8, 8, 10, 12]
    assert [1, 1] in [w for _, w in shape] and any(len(w) >= 4 for _, w in shape)
    if hold:
        first = [lo for kd, m, lo, hi in books[(0, "gb")].log if kd == 0]
        assert any(lo > 0 for lo in first)


def test_gpu_split_transcript_d2_table(oracle):
    """d = 2, table form: the row-major labels and 16-row tables, node values stored per test in the level's
    shared rows and summed on the device, then negated per child; through the FieldElm level."""
    shape, _ = _split_transcript(2, 0, 1, 3)
    assert [sum(w) for _, w in shape] == [4, 8, 12, 20, 20, 20, 20, 20]


def test_gpu_split_transcript_circuit(oracle):
    """form = 1 at d = 1: the half-gates circuit with the output-label share, the FE levels only."""
    shape, _ = _split_transcript(1, 1, 1, 3, levels=7)
    assert any(len(w) >= 3 for _, w in shape)


# ---- 5. refusals, each leaving the ctx usable ------------------------------------------------------------
def _cfg_pair(seed, lv, j, g, cb, cc):
    from fuzzyheavyhitters_amd import party
    cfg_gb, cfg_ev = party.test_cfgs(seed ^ (j << 48) ^ (g << 39), lv)
    for cfg in (cfg_gb, cfg_ev):
        cfg.child_begin, cfg.child_count, cfg.form, cfg.ot_ss_k = cb, cc, 0, 1
    return cfg_gb, cfg_ev


def _sums(kc, C):
    from fuzzyheavyhitters_amd._lib import lib, u64p
    out = np.zeros(C, np.uint64)
    rc = lib().fhh_party_node_sums(kc.handle, out.ctypes.data_as(u64p), None)
    return rc, out, lib().fhh_last_error(kc.handle) or b""


def test_gpu_refusals_leave_the_ctx_usable():
    """What the state machine refuses in a split level — fhh_party_set_server(2), a server change with the level
    open, a role reopened before its chunk finished, a chunk that overlaps or skips past the last opened one,
    node sums with a child uncovered, node sums of a mixed level with the server unset — each with its code, and
    the same pair of ctxs then finishes the level with the plaintext counts and runs the next one."""
    from fuzzyheavyhitters_amd import KeyCollection
    from fuzzyheavyhitters_amd._lib import lib
    L = lib()
    d = 1
    counts, _ = prc.plaintext_of(d)
    c0, c1 = _keys(d)
    servers = (c0, c1)
    chans = _channels(c0, c1)
    c0.tree_init()
    c1.tree_init()
    out, nb = ctypes.c_void_p(), ctypes.c_uint64()

    def level(lv, plan):   # plan: [(cb, cc, g)]
        C, _ = c0.tree_crawl()
        assert c1.tree_crawl()[0] == C == len(counts[lv])
        return C, [_Win(servers, g, *_cfg_pair(77, lv, j, g, cb, cc), chans) for j, (cb, cc, g) in enumerate(plan)]

    def finish(lv, C):
        (rc0, s0, _), (rc1, s1, _) = _sums(c0, C), _sums(c1, C)
        assert rc0 == 0 and rc1 == 0
        assert np.array_equal(((s0.astype(object) - s1.astype(object)) % pm.FE_P).astype(np.uint64), counts[lv]), lv
        keep = KeyCollection.keep_values(prc.N_CLIENTS, 1, s0, s1)
        c0.tree_prune(keep)
        c1.tree_prune(keep)

    # levels 0 and 1 in one role each, server unset: the sign is the caller's business (server 1 garbles level 1)
    for lv, g in ((0, 0), (1, 1)):
        C, wins = level(lv, [(0, 0, g)])
        wins[0].run()
        (rc0, s0, _), (rc1, s1, _) = _sums(c0, C), _sums(c1, C)
        assert rc0 == 0 and rc1 == 0
        diff = (s0.astype(object) - s1.astype(object)) % pm.FE_P
        assert np.array_equal(((diff if g == 0 else -diff) % pm.FE_P).astype(np.uint64), counts[lv])
        keep = counts[lv] >= 1
        c0.tree_prune(keep)
        c1.tree_prune(keep)
    # level 2: 6 children in windows of 2, garbled by servers 0, 1, 0
    C, (w0, w1, w2) = level(2, [(0, 2, 0), (2, 2, 1), (4, 2, 0)])
    assert C == 6
    assert L.fhh_party_set_server(c0.handle, 2) == E_ARG and L.fhh_party_set_server(c0.handle, -2) == E_ARG
    w0.labels()
    for kc in servers:      # the level is open on both ctxs
        assert L.fhh_party_set_server(kc.handle, 0) == E_STATE
        assert b"open" in L.fhh_last_error(kc.handle)
    # a role reopened before its previous chunk finished: server 1's evaluator, server 0's garbler
    # (at child 2, where the level's next chunk does begin: only the unfinished chunk is in the way)
    again_gb, again_ev = _cfg_pair(77, 2, 1, 0, 2, 2)
    assert L.fhh_ev_ot_labels(c1.handle, ctypes.byref(again_ev), ctypes.byref(out), ctypes.byref(nb)) == E_STATE
    assert b"does not follow" in L.fhh_last_error(c1.handle)
    assert L.fhh_gb_ot_labels(c0.handle, ctypes.byref(again_gb), None, 0, ctypes.byref(out), ctypes.byref(nb)) == E_STATE
    # the other role of server 0 is free, but its chunk must begin at child 2: 1 overlaps, 3 skips
    for cb in (1, 3):
        _, cfg_ev = _cfg_pair(77, 2, 1, 1, cb, 2)
        assert L.fhh_ev_ot_labels(c0.handle, ctypes.byref(cfg_ev), ctypes.byref(out), ctypes.byref(nb)) == E_STATE
        assert b"does not follow" in L.fhh_last_error(c0.handle)
    w1.labels()
    for st in ("garble", "evaluate", "shares"):
        for w in (w0, w1):
            getattr(w, st)()
    for kc in servers:      # children 4, 5 are uncovered
        rc, _, err = _sums(kc, C)
        assert rc == E_STATE and b"not finished" in err
    w2.run()
    for kc in servers:      # both roles ran and nobody said which server this is
        rc, _, err = _sums(kc, C)
        assert rc == E_STATE and b"fhh_party_set_server" in err
    c0.party_set_server(0)
    c1.party_set_server(1)
    finish(2, C)
    # the next level, split again, and one more with the roles swapped: the ctxs go on
    C = len(counts[3])
    C, wins = level(3, [(b, c, g) for b, c, g in KeyCollection.party_role_plan(C, 3, 3, 3)])
    _run_split(wins)
    finish(3, C)
    C, wins = level(4, [(0, 0, 1)])
    wins[0].run()
    finish(4, C)
    # unset again: a whole level in one role is summed as ever
    c0.party_set_server(-1)
    c1.party_set_server(-1)
    C, wins = level(5, [(0, 0, 0)])
    wins[0].run()
    finish(5, C)
