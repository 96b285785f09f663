"""The host side of a level split between the servers (no GPU): the role plan both servers compute
(fhh_party_role_plan), the negation fhh_party_node_sums applies under fhh_party_set_server, against Python ints,
and the level shapes the GPU tests' workloads reach, from the plaintext crawl."""
import ctypes

import numpy as np
import pytest

import party_roles_cases as prc

FE_P = (1 << 62) - (1 << 30) - 1
FE255_P = (1 << 255) - 19
E_ARG = -1


def _plan(C, chunk, level, mode):
    from fuzzyheavyhitters_amd import KeyCollection
    return KeyCollection.party_role_plan(C, chunk, level, mode)


def _chunks_for(C):
    return sorted({0, 1, 3, C, C + 1})


@pytest.mark.parametrize("C", [0, 1, 2, 3, 7, 8, 1000])
def test_role_plan_windows_and_garblers(C):
    """Every mode, chunk size and level parity: the windows are ascending, contiguous and cover [0, C); modes
    0 - 2 are chunk_windows' with one garbler; mode 3 cuts a one-window level of C >= 2 in two, alternates the
    garblers from level & 1, and the servers' garbled children differ by at most one window."""
    from fuzzyheavyhitters_amd.party import chunk_windows
    for chunk in _chunks_for(C):
        for level in (0, 1):
            today = [(b, c if (b, c) != (0, 0) else C) for b, c in chunk_windows(C, chunk)]
            for mode in range(4):
                plan = _plan(C, chunk, level, mode)
                what = f"C {C} chunk {chunk} level {level} mode {mode}: {plan}"
                assert len(plan) >= 1 and plan[0][0] == 0, what
                assert all(c > 0 for _, c, _ in plan) or C == 0, what
                assert all(a[0] + a[1] == b[0] for a, b in zip(plan, plan[1:])), what
                assert plan[-1][0] + plan[-1][1] == C, what
                assert plan[0][2] == ((0, 1, level & 1, level & 1)[mode]), what
                if mode < 3:
                    assert [(b, c) for b, c, _ in plan] == today, what
                    assert len({g for _, _, g in plan}) == 1, what
                    continue
                assert [c for _, c, _ in plan] == prc.windows_of(C, chunk, True), what
                assert [g for _, _, g in plan] == [(level + w) & 1 for w in range(len(plan))], what
                by = [sum(c for _, c, g in plan if g == s) for s in (0, 1)]
                assert abs(by[0] - by[1]) <= max(c for _, c, _ in plan), what
                if C >= 2:
                    assert by[0] > 0 and by[1] > 0, what


def test_role_plan_refusals():
    """Arguments that make no sense return FHH_E_ARG and name the call; the count-only form writes n_windows."""
    from fuzzyheavyhitters_amd._lib import lib, u8p, u64p
    L = lib()
    nw = ctypes.c_uint64(99)
    b, c, g = np.zeros(4, np.uint64), np.zeros(4, np.uint64), np.zeros(4, np.uint8)
    pb, pc, pg = b.ctypes.data_as(u64p), c.ctypes.data_as(u64p), g.ctypes.data_as(u8p)
    assert L.fhh_party_role_plan(10, 3, 0, 3, 0, ctypes.byref(nw), None, None, None) == 0 and nw.value == 4
    assert L.fhh_party_role_plan(10, 3, 0, 3, 4, ctypes.byref(nw), pb, pc, pg) == 0
    assert list(b) == [0, 3, 6, 9] and list(c) == [3, 3, 3, 1] and list(g) == [0, 1, 0, 1]
    for args in ((10, 3, 0, 4, 4, ctypes.byref(nw), pb, pc, pg),       # no such mode
                 (10, 3, 0, 0xFFFFFFFF, 4, ctypes.byref(nw), pb, pc, pg),
                 (10, 3, 0, 3, 4, None, pb, pc, pg),                    # nowhere to write the count
                 (10, 3, 0, 3, 3, ctypes.byref(nw), pb, pc, pg),        # 4 windows into 3 entries
                 (10, 3, 0, 3, 0, ctypes.byref(nw), pb, pc, pg),
                 (10, 3, 0, 3, 4, ctypes.byref(nw), None, pc, pg),      # some arrays only
                 (10, 3, 0, 3, 4, ctypes.byref(nw), pb, None, pg),
                 (10, 3, 0, 3, 4, ctypes.byref(nw), pb, pc, None)):
        assert L.fhh_party_role_plan(*args) == E_ARG, args[:5]
        assert b"party_role_plan" in L.fhh_last_error(None)


def _neg(fmt, v):
    from fuzzyheavyhitters_amd._lib import lib
    if fmt < 2:
        a, out = ctypes.c_uint64(v), ctypes.c_uint64(0xDEAD)
        rc = lib().fhh_party_negate(fmt, ctypes.byref(a), ctypes.byref(out))
        return rc, out.value
    a = (ctypes.c_uint32 * 10)(*[(v >> (32 * k)) & 0xFFFFFFFF for k in range(10)])
    out = (ctypes.c_uint32 * 8)()
    rc = lib().fhh_party_negate(2, a, out)
    return rc, sum(int(x) << (32 * k) for k, x in enumerate(out))


def test_negation_rule_against_python_ints():
    """FE: p - s with 0 staying 0; Z_2^32: (2^32 - s) mod 2^32 zero-extended; FieldElm: the canonical negation
    mod 2^255 - 19 of an unreduced 10-limb sum. The one-sided edges (0, 1, p - 1; 0, 2^32 - 1; 0, p - 1, and p,
    p + 1, 2 p, the top of 320 bits for the unreduced input) and seeded values between them."""
    rng = np.random.default_rng(11)
    fe = [0, 1, 2, FE_P - 1, FE_P - 2, FE_P // 2] + [int(x) % FE_P for x in rng.integers(0, 1 << 62, 20)]
    for v in fe:
        rc, got = _neg(0, v)
        assert rc == 0 and got == (-v) % FE_P and 0 <= got < FE_P, v
        assert (got + v) % FE_P == 0
    ring = [0, 1, (1 << 32) - 1, 1 << 31] + [int(x) for x in rng.integers(0, 1 << 32, 20)]
    for v in ring:
        rc, got = _neg(1, v)
        assert rc == 0 and got == (-v) % (1 << 32) and got < 1 << 32, v
    big = [0, 1, FE255_P - 1, FE255_P, FE255_P + 1, 2 * FE255_P, 2 * FE255_P + 5, (1 << 255), (1 << 256) - 1,
           (1 << 320) - 1, 130 * (FE255_P - 1)]
    big += [int.from_bytes(rng.bytes(40), "little") for _ in range(20)]
    for v in big:
        rc, got = _neg(2, v)
        assert rc == 0 and got == (-v) % FE255_P and 0 <= got < FE255_P, hex(v)
    # the values the formats do not hold are refused, the output untouched
    for fmt, v in ((0, FE_P), (0, (1 << 64) - 1), (1, 1 << 32), (3, 0)):
        rc, got = _neg(fmt, v) if fmt < 2 else (_neg_raw(fmt), 0xDEAD)
        assert rc == E_ARG and got == 0xDEAD, (fmt, v)


def _neg_raw(fmt):
    from fuzzyheavyhitters_amd._lib import lib
    a, out = ctypes.c_uint64(0), ctypes.c_uint64(0)
    return lib().fhh_party_negate(fmt, ctypes.byref(a), ctypes.byref(out))


def test_sign_rule_gives_the_count_whoever_garbles():
    """The rule itself on Python ints: shares with garbler - evaluator = eq; server 0 negates what it evaluated,
    server 1 what it garbled; then v0 - v1 = eq in each format for either garbler."""
    rng = np.random.default_rng(12)
    for fmt, mod in ((0, FE_P), (1, 1 << 32), (2, FE255_P)):
        for eq in (0, 1, 130):
            for garbler in (0, 1):
                ev = int.from_bytes(rng.bytes(40), "little") % mod
                gb = (ev + eq) % mod
                s = {garbler: gb, 1 - garbler: ev}
                role = {garbler: "garbled", 1 - garbler: "evaluated"}
                flip = [role[0] == "evaluated", role[1] == "garbled"]
                v = [_neg(fmt, s[k])[1] if flip[k] else s[k] for k in (0, 1)]
                assert (v[0] - v[1]) % mod == eq, (fmt, eq, garbler)


@pytest.mark.parametrize("d", [1, 2])
def test_workload_level_shapes(d):
    """The shapes the GPU tests rely on, from workload.plaintext_crawl alone (see party_roles_cases for why a
    level of C = 1 or of odd C cannot exist and what stands for them), at levels that are not the last."""
    counts, finals = prc.plaintext_of(d)
    Cs = [len(c) for c in counts[:-1]]
    assert all(C % (1 << d) == 0 and C >= 1 << d for C in Cs), Cs   # never 1, never odd
    wins = [prc.windows_of(C, prc.CHUNK, True) for C in Cs]
    assert any(len(w) >= 4 for w in wins), wins
    assert any(len(w) >= 3 and len(w) % 2 == 1 and w[-1] < prc.CHUNK for w in wins), wins
    assert any(w[-1] == 1 for w in wins), wins                       # a one-child window
    whole = [prc.windows_of(C, 0, True) for C in Cs]
    assert all(len(w) == 2 and w[0] - w[1] in (0, 1) for w in whole), whole
    if d == 1:
        assert 2 in Cs and prc.windows_of(2, prc.CHUNK, True) == [1, 1]
        assert any(w[0] % 2 == 1 and w[0] >= 5 for w in whole), whole   # odd chunks of >= 5 children
    # the last level has several windows, so server 1 garbles some of its children when split
    assert len(prc.windows_of(len(counts[-1]), prc.CHUNK, True)) >= 2
    assert len(finals) >= 3 and all(v >= 1 for v in finals.values())
    # counts the leader must see: every level holds both kept (>= 1) and dropped (0) children somewhere
    assert any((c == 0).any() for c in counts) and all((c >= 1).any() for c in counts)
