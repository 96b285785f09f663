"""The two-server GC + OT in form 2 (fhh_gb_cfg.form = 2: the FE levels' garbled table with its shares in
Z_2^32), as tests/party_model.py states forms 0 and 1: computed from the oracle (oracle/oracle.py), numpy
and Python ints only — no entry point of the product package is called here.

A helper module of tests/test_party_ring32.py (not a conftest). What form 2 changes against form 0:

  * only an FE level with bits = 2 d <= 4 differs; the FieldElm level is form 0's chunk (party_model);
  * the labels OT, npad (512-client tiles at bits <= 2, 64 otherwise), the session counters and the gate
    tweaks are form 0's, so u1 is form 0's u1;
  * the gc message is the table's rows 1 .. 2^bits - 1 as u32, SoA [2^bits - 1][tests] (oracle
    gt_garble_ring32): half of form 0's bytes; u2 / y2 stay empty;
  * a party's node values are u32 and its sum per child is taken mod 2^32; v0 - v1 mod 2^32 is the count.

The FE table on the same labels (form 0's gc and values) is returned beside it, so a test can compare
lengths and keep decisions with form 0 without a second OT extension in the oracle.
"""
from __future__ import annotations

import numpy as np

import party_model as pm
from oracle import oracle as O

RING = 1 << 32


def chunk_model(b0: np.ndarray, b1: np.ndarray, cb: int, cc: int, lv: int, last: bool, ss_k: int,
                base_pairs: np.ndarray, s: np.ndarray, mask: int, ctr_off):
    """One chunk in form 2; the arguments of party_model.chunk_model without `form`. At the last level this
    is party_model.chunk_model(form 0) itself. At an FE level (bits <= 4) the dict holds m1, m2 = 0, u1 /
    corr1, u2 = corr2 = None, y2 = b"", table = True, gc (u32 SoA bytes), gv / ev ([cc][n] ints below
    2^32), and form 0's view of the same labels: gc_fe (u64 SoA bytes), gv_fe / ev_fe ([cc][n] ints mod p)."""
    C, bits, n = b0.shape
    if last:
        return pm.chunk_model(b0, b1, cb, cc, lv, True, 0, ss_k, base_pairs, s, mask, ctr_off)
    assert bits <= 4, "form 2 exists for 2 d <= 4 only"
    assert b1.shape == b0.shape and s[0][0] & 1
    npad = pm.npad_of(n, bits, 0, False)
    tests = cc * n
    m1 = cc * bits * npad
    gb = pm.gate_base(lv, cb, n, bits)
    delta = bytes(s[0])
    z = np.zeros((cc, n), object)
    res = dict(m1=m1, m2=0, u1=None, corr1=None, u2=None, corr2=None, gc=b"", gc_fe=b"", y2=b"", out=None, table=True,
               gv=z, ev=z.copy(), gv_fe=z.copy(), ev_fe=z.copy())
    if tests == 0:
        return res
    g = np.ascontiguousarray(b0[cb:cb + cc].transpose(0, 2, 1).reshape(tests, bits))
    ch = np.zeros((cc, bits, npad), np.uint8)
    ch[:, :, :n] = b1[cb:cb + cc]
    q, t, u1, _, corr1 = pm._cot(ss_k, O.COT_RAW, ch.reshape(-1), base_pairs[0], delta, 0, ctr_off[0])
    res["u1"], res["corr1"] = u1, corr1

    def per_test(rows):   # OT index ((c - cb) bits + k) npad + i -> [tests][bits][16]
        return np.ascontiguousarray(rows.reshape(cc, bits, npad, 16)[:, :, :n].transpose(0, 2, 1, 3)
                                    .reshape(tests, bits, 16))

    ev_zero, ev_act = per_test(q), per_test(t)
    msgs, gv = O.gt_garble_ring32(g, ev_zero, mask, delta, gate_base=gb)
    ev = O.gt_eval_ring32(ev_act, msgs, gate_base=gb)
    assert msgs.dtype == np.uint32 and gv.dtype == np.uint32 and ev.dtype == np.uint32
    res["gc"] = np.ascontiguousarray(msgs.T).tobytes()
    msgs_fe, gv_fe = O.gt_garble(g, ev_zero, mask, delta, gate_base=gb)
    ev_fe = O.gt_eval(ev_act, msgs_fe, gate_base=gb)
    res["gc_fe"] = np.ascontiguousarray(msgs_fe.T).tobytes()
    for key, v in (("gv", gv), ("ev", ev), ("gv_fe", gv_fe), ("ev_fe", ev_fe)):
        res[key] = np.array([int(x) for x in v], object).reshape(cc, n)
    return res


def ring_sums(vals) -> list:
    """[cc][n] ints -> per child sum mod 2^32."""
    return [int(sum(int(x) for x in row)) % RING for row in vals]


def thirds_cases(rng, n: int, bits: int):
    """(g, e) [n][bits]: the first n // 3 tests equal, the rest independent random strings."""
    g = rng.integers(0, 2, (n, bits), dtype=np.uint8)
    e = rng.integers(0, 2, (n, bits), dtype=np.uint8)
    e[:n // 3] = g[:n // 3]
    return g, e


def table_chain(g, e, mask, seeds, s, gate_base=0, ctr_off=0):
    """The labels OT (the IKNP correlation) and the Z_2^32 table on it, all in the oracle: OT index k npad +
    i with npad = n rounded up to 512 for bits <= 2 and to 64 for bits = 3, 4 (as fhh_gt_cot_ring32_host)."""
    n, bits = g.shape
    npad = (n + 511) // 512 * 512 if bits <= 2 else (n + 63) // 64 * 64
    ch = np.zeros(bits * npad, np.uint8)
    for k in range(bits):
        ch[k * npad: k * npad + n] = e[:, k]
    q, t_rows, _, _ = O.cot_extend(O.COT_RAW, ch, seeds, s, ctr_off=ctr_off)
    ev_zero = np.stack([q[k * npad: k * npad + n] for k in range(bits)], axis=1)
    ev_act = np.stack([t_rows[k * npad: k * npad + n] for k in range(bits)], axis=1)
    msgs, gv = O.gt_garble_ring32(g, ev_zero, mask, s, gate_base=gate_base)
    ev = O.gt_eval_ring32(ev_act, msgs, gate_base=gate_base)
    return dict(ev_zero=ev_zero, ev_active=ev_act, msgs=msgs, gb_share=gv, ev_share=ev)
