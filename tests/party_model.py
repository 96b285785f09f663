"""What one chunk of one level of the two-server GC + OT (fhh_gb_* / fhh_ev_*, include/fhh.h) must put on
the wire and into each server's node sums, computed from the oracle (oracle/oracle.py), numpy and
Python ints only — no entry point of the product package is called here.

A helper module of tests/test_party_transcript.py (not a conftest). The model restates the host state
machine of fuzzyheavyhitters_amd/csrc/fhh_gcot.cpp:

  * bits = 2 d; a test is (child, client); the chunk holds the children [cb, cb + cc) of the level;
  * npad: the clients of one (child, bit) row of the labels OT, n rounded up to 512 for the tile-major
    table (table form at an FE level, bits <= 2), to 64 otherwise;
  * labels OT (kind 0): m1 = cc bits npad OTs, choice bit ((c - cb) bits + k) npad + i = server 1's share
    bit k of (child c, client i), 0 in the padding; the IKNP correlation itself (q_j, t_j = q_j ^ r_j s,
    s = the free-XOR Delta), so it has no reply;
  * the row PRG of a chunk starts `ctr_off` blocks into the base-OT session: chunks (and levels) on
    unchanged base material continue the counter by session_blocks(m) each, new material restarts at 0;
  * the wire U is tile-major (tmaj_pack): 16 mp / k bytes (mp = m rounded up to 8192), and for SoftSpoken
    (k > 1) the GGM corrections [128 / k][k][2][16] follow it;
  * gate tweaks: gate_base = (level << 40) + cb n (bits - 1); the table's test t hashes under
    gate_base + t, the circuit's gate g of test t under 2 (gate_base + t (bits - 1) + g) and the next;
  * table form (FE levels, bits <= 4): the gc message is the table's rows 1 .. 2^bits - 1 as SoA u64
    [2^bits - 1][tests]; circuit form: [tables SoA [2 (bits - 1)][tests][16] | y [tests] u64 | decode [tests]];
  * last (FieldElm) level: the circuit without the share, [tables | decode]; the evaluator's output bits
    eq ^ mask, each twice, are the choice bits of the share OT (kind 1, its own session counter), a
    correlated OT of BlockPairs (COT_FE255) with the garbler's mask; u2 as u1, y2 = [m2][16].
"""
from __future__ import annotations

import numpy as np

from oracle import oracle as O

FE_P = (1 << 62) - (1 << 30) - 1
FE255_P = (1 << 255) - 19


# ---- sizes ------------------------------------------------------------------------------------------
def ot_padded(m: int) -> int:
    return (m + 8191) // 8192 * 8192


def session_blocks(m: int) -> int:
    """Row-PRG blocks a batch of m OTs takes from its base-OT session."""
    return ((ot_padded(m) // 128 + 255) // 256 * 256) if m else 0


def npad_of(n: int, bits: int, form: int, last: bool) -> int:
    if form == 0 and not last and bits <= 2:
        return (n + 511) // 512 * 512
    return (n + 63) // 64 * 64


def is_table(bits: int, form: int, last: bool) -> bool:
    return form == 0 and not last and bits <= 4


def gate_base(lv: int, cb: int, n: int, bits: int) -> int:
    return (lv << 40) + cb * n * (bits - 1)


def u_wire_bytes(m: int, k: int) -> int:
    return (16 * ot_padded(m) // k + (4096 if k > 1 else 0)) if m else 0


# ---- the tile-major wire U --------------------------------------------------------------------------
def tmaj_pack(rows: np.ndarray, nblk: int) -> np.ndarray:
    """rows [R][nb][16] (row i, 128-OT block c) -> the wire's bytes [R nblk 16]: block (i, c) at byte
    16 ((c // 4) 4 R + 4 i + c % 4); blocks c >= nb stay zero. nblk (= mp / 128) is a multiple of 4."""
    R, nb = rows.shape[:2]
    assert nblk % 4 == 0 and nb <= nblk
    full = np.zeros((R, nblk, 16), np.uint8)
    full[:, :nb] = rows
    return np.ascontiguousarray(full.reshape(R, nblk // 4, 4, 16).transpose(1, 0, 2, 3)).reshape(-1)


def tmaj_unpack(wire: np.ndarray, R: int, nb: int) -> np.ndarray:
    """The inverse on the blocks c < nb: wire bytes [R nblk 16] -> rows [R][nb][16]."""
    w = np.asarray(wire, np.uint8).reshape(-1)
    nblk = w.size // (16 * R)
    assert nblk % 4 == 0 and w.size == R * nblk * 16 and nb <= nblk
    return np.ascontiguousarray(w.reshape(nblk // 4, R, 4, 16).transpose(1, 0, 2, 3).reshape(R, nblk, 16)[:, :nb])


# ---- counters and tweaks ----------------------------------------------------------------------------
class SessionBook:
    """The running row-PRG counter of one ctx per OT kind: unchanged base material continues it, new
    material restarts at 0. `log` keeps (kind, material, begin, end) of every batch taken."""

    def __init__(self):
        self.material = [None, None]
        self.next = [0, 0]
        self.log = []

    def take(self, kind: int, material: bytes, m: int) -> int:
        if self.material[kind] != material:
            self.material[kind] = material
            self.next[kind] = 0
        off = self.next[kind]
        self.next[kind] += session_blocks(m)
        self.log.append((kind, material, off, self.next[kind]))
        return off


def tweak_range(lv: int, cb: int, cc: int, n: int, bits: int, table: bool):
    """[lo, hi) of the hash tweaks one chunk uses under its Delta."""
    gb = gate_base(lv, cb, n, bits)
    if table:
        return gb, gb + cc * n
    return 2 * gb, 2 * (gb + cc * n * (bits - 1))


def ranges_disjoint(ranges) -> bool:
    """Half-open (lo, hi) ranges, empty ones ignored: no two overlap."""
    r = sorted((lo, hi) for lo, hi in ranges if hi > lo)
    return all(a[1] <= b[0] for a, b in zip(r, r[1:]))


def disjoint_per_key(entries) -> bool:
    """entries (key, lo, hi): the ranges under each key are pairwise disjoint."""
    by = {}
    for key, lo, hi in entries:
        by.setdefault(key, []).append((lo, hi))
    return all(ranges_disjoint(v) for v in by.values())


# ---- planes -----------------------------------------------------------------------------------------
def plane_bits(planes: np.ndarray, n: int) -> np.ndarray:
    """Share planes [C][bits][nw] u64 (bit client % 64 of word client / 64) -> bits [C][bits][n] u8."""
    p = np.ascontiguousarray(planes, np.uint64)
    C, bits, nw = p.shape
    return np.unpackbits(p.view(np.uint8).reshape(C, bits, nw * 8), axis=-1, bitorder="little")[:, :, :n].copy()


def equal_counts(b0: np.ndarray, b1: np.ndarray) -> np.ndarray:
    """Per child: the clients whose two share strings are equal (bits [C][bits][n])."""
    return (b0 == b1).all(axis=1).sum(axis=1).astype(np.uint64)


# ---- one chunk --------------------------------------------------------------------------------------
def _cot(k, mode, ch, pairs, s, mask, ctr_off):
    """(sender_out, out, U rows, y, corr or None) from the oracle: IKNP (k = 1) or SoftSpoken."""
    if k == 1:
        sx, out, u, y = O.cot_extend(mode, ch, pairs, s, mask=mask, ctr_off=ctr_off)
        return sx, out, u, y, None
    return O.cot_extend_ss(k, mode, ch, pairs, s, mask=mask, ctr_off=ctr_off)


def _soa_tables(tables: np.ndarray) -> bytes:
    """[tests][bits - 1][2][16] -> SoA [2 (bits - 1)][tests][16]."""
    return np.ascontiguousarray(tables.transpose(1, 2, 0, 3)).tobytes()


def chunk_model(b0: np.ndarray, b1: np.ndarray, cb: int, cc: int, lv: int, last: bool, form: int, ss_k: int,
                base_pairs: np.ndarray, s: np.ndarray, mask: int, ctr_off):
    """One chunk. b0 / b1: the level's share bits [C][bits][n] of server 0 (garbler) and 1 (evaluator);
    base_pairs [kind][128][2][16], s [kind][16] (bit 0 of s[0] set); ctr_off (kind 0, kind 1).
    Returns a dict: m1, m2, u1 / u2 (rows [128 / k][ceil(m / 128)][16] or None), corr1 / corr2, gc (bytes),
    y2 (bytes), gv / ev ([cc][n] Python ints: the garbler's and the evaluator's node values), out (the GC
    output bits eq ^ mask at the last level, else None), table."""
    C, bits, n = b0.shape
    assert b1.shape == b0.shape and s[0][0] & 1
    npad = npad_of(n, bits, form, last)
    table = is_table(bits, form, last)
    tests = cc * n
    m1 = cc * bits * npad
    gb = gate_base(lv, cb, n, bits)
    delta = bytes(s[0])
    res = dict(m1=m1, m2=0, u1=None, corr1=None, u2=None, corr2=None, gc=b"", y2=b"", out=None, table=table,
               gv=np.zeros((cc, n), object), ev=np.zeros((cc, n), object))
    if tests == 0:
        return res
    g = np.ascontiguousarray(b0[cb:cb + cc].transpose(0, 2, 1).reshape(tests, bits))
    ch = np.zeros((cc, bits, npad), np.uint8)
    ch[:, :, :n] = b1[cb:cb + cc]
    q, t, u1, _, corr1 = _cot(ss_k, O.COT_RAW, ch.reshape(-1), base_pairs[0], delta, 0, ctr_off[0])
    res["u1"], res["corr1"] = u1, corr1

    def per_test(rows):   # OT index ((c - cb) bits + k) npad + i -> [tests][bits][16]
        return np.ascontiguousarray(rows.reshape(cc, bits, npad, 16)[:, :, :n].transpose(0, 2, 1, 3)
                                    .reshape(tests, bits, 16))

    ev_zero, ev_act = per_test(q), per_test(t)
    if table:
        msgs, gv = O.gt_garble(g, ev_zero, mask, delta, gate_base=gb)
        ev = O.gt_eval(ev_act, msgs, gate_base=gb)
        res["gc"] = np.ascontiguousarray(msgs.T).tobytes()
    elif not last:
        tables, dec, gv, y = O.gc_garble_eq_cot(g, ev_zero, mask, delta, gate_base=gb, share=True)
        _, ev = O.gc_eval_eq_cot(tables, ev_act, dec, gate_base=gb, share_y=y)
        res["gc"] = _soa_tables(tables) + y.tobytes() + dec.tobytes()
    else:
        tables, dec = O.gc_garble_eq_cot(g, ev_zero, mask, delta, gate_base=gb)
        out = O.gc_eval_eq_cot(tables, ev_act, dec, gate_base=gb)
        res["gc"] = _soa_tables(tables) + dec.tobytes()
        res["out"] = out.reshape(cc, n)
        m2 = 2 * tests
        sx, rx, u2, y2, corr2 = _cot(ss_k, O.COT_FE255, np.repeat(out, 2), base_pairs[1], bytes(s[1]), mask,
                                     ctr_off[1])
        res.update(m2=m2, u2=u2, corr2=corr2, y2=y2.tobytes())
        gv = np.array([int.from_bytes(bytes(r), "big") for r in sx], object)
        ev = np.array([int.from_bytes(bytes(r), "big") for r in rx], object)
    res["gv"] = np.array([int(x) for x in gv], object).reshape(cc, n)
    res["ev"] = np.array([int(x) for x in ev], object).reshape(cc, n)
    return res


def expected_u_wire(rows, corr, m: int, k: int):
    """(the wire's U region with zeros where the oracle defines nothing, its defined-block count nb, the
    corrections' bytes or b"")."""
    R = 128 // k
    nb = (m + 127) // 128
    assert rows.shape == (R, nb, 16)
    return tmaj_pack(rows, ot_padded(m) // 128), nb, (b"" if corr is None else np.ascontiguousarray(corr).tobytes())


def fe_sums(vals) -> list:
    """[cc][n] ints -> per child sum mod p (FE levels)."""
    return [int(sum(int(x) for x in row)) % FE_P for row in vals]


def fe255_sums(vals):
    """[cc][n] ints -> (unreduced sums, canonical sums) per child (the FieldElm level)."""
    unr = [int(sum(int(x) for x in row)) for row in vals]
    return unr, [v % FE255_P for v in unr]


def limbs(v: int, k: int) -> np.ndarray:
    assert 0 <= v < 1 << (32 * k)
    return np.array([(v >> (32 * j)) & 0xFFFFFFFF for j in range(k)], np.uint32)


def limbs_int(a) -> int:
    return sum(int(x) << (32 * j) for j, x in enumerate(np.asarray(a).ravel()))
