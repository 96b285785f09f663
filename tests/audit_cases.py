"""The CPU model of the key audit (fhh_audit_keys_ball, row j) and the cases its tests share. Nothing here calls
the code under test: the bounds come from oracle.l_inf_ball_bounds / oracle.i16_to_bitvec (ball_cases.py), the
probes x_p = l - 1, l, a, r, r + 1 mod 2^L are Python ints, every walk goes level by level through
oracle.eval_bit, and the expected bit after level k is [x_p[..k] < l[..k]] for the left key and
[x_p[..k] > r[..k]] for the right key, the top k bits compared as integers (the algebra that
test_oracle_kat.py::test_ibdcf_semantics_exhaustive pins). A client is ok iff all its 2 d 5 L comparisons hold; the
first failure is the lowest in the order (client, dim, side, probe, level)."""
import numpy as np

import ball_cases as bc

PROBES = 5
FIELDS = ("key_idx", "root_seed", "cw_seed", "cw_bits")
NO_CLIENT = 2 ** 64 - 1


def int_of(bits):
    v = 0
    for b in bits:
        v = (v << 1) | int(b)
    return v


def probes_of(l, r, a, L):
    """The five probes of bounds l, r and point a (L-bit ints): each wraps on its own."""
    m = (1 << L) - 1
    return [(l - 1) & m, l, a, r, (r + 1) & m]


def bits_points(oracle, alpha, delta):
    """(l, r, a) int arrays [n][d] (dtype object) of bit points alpha [n][d][L], the bounds by the oracle."""
    left, right = bc.oracle_bounds(oracle, alpha, delta)
    n, d, _ = alpha.shape
    f = lambda x: np.array([[int_of(x[c, j]) for j in range(d)] for c in range(n)], object).reshape(n, d)
    return f(left), f(right), f(alpha)


def coords_points(oracle, pts, ball):
    """(l, r, a) [n][2] of int16 (lat, long) points: the clamped bounds' and the point's own 16-bit patterns
    (oracle.i16_to_bitvec)."""
    left, right = bc.coords_bounds(oracle, pts, ball)
    n = pts.shape[0]
    f = lambda x: np.array([[int_of(x[c, j]) for j in range(2)] for c in range(n)], object).reshape(n, 2)
    a = np.array([[int_of(oracle.i16_to_bitvec(int(pts[c, j]))) for j in range(2)] for c in range(n)], object)
    return f(left), f(right), a.reshape(n, 2)


def probe_bits(l, r, a, L):
    """uint8 [n][d][5][L] of int arrays l, r, a [n][d]: what fhh_audit_probes must write."""
    n, d = l.shape
    out = np.zeros((n, d, PROBES, L), np.uint8)
    for c in range(n):
        for j in range(d):
            for p, x in enumerate(probes_of(int(l[c, j]), int(r[c, j]), int(a[c, j]), L)):
                out[c, j, p] = bc.bits_of(x, L)
    return out


def keys_arrays(ks):
    """A ServerKeys as a dict of writable arrays (what the tamper cases modify and add_keys loads)."""
    return {f: np.array(getattr(ks, f), np.uint8, copy=True) for f in FIELDS}


def add_to(coll, k):
    coll.add_keys(k["key_idx"], k["root_seed"], k["cw_seed"], k["cw_bits"])


def walk(oracle, k, c, j, side, xbits):
    """eval_init + eval_bit down xbits with key (c, j, side) of k: ([y ^ t after level 1 .. L], final seed, final t)."""
    seed, t = k["root_seed"][c, j, side].tobytes(), int(k["key_idx"][c, j, side])
    y, out = t, []
    for lvl, b in enumerate(xbits):
        seed, t, y = oracle.eval_bit(seed, t, y, k["cw_seed"][c, j, side, lvl].tobytes(), int(k["cw_bits"][c, j, side, lvl]),
                                     int(b))
        out.append(y ^ t)
    return out, seed, t


def audit(oracle, k0, k1, l, r, a, L, clients=None):
    """The model's audit of servers' keys k0 / k1 (dicts of arrays) against bounds l, r and points a [n][d] for the
    given clients (default: all). Returns a dict: ok (uint8 [n], 1 for a client not looked at), n_checks,
    n_bad_clients, first (None or the tuple (client, dim, side, probe, level, got, expected)), failures (the set of
    every failed (client, dim, side, probe, level)) and seed_diverged (walks ending with t0 == t1 and unequal
    seeds)."""
    n, d = l.shape
    clients = range(n) if clients is None else clients
    ok = np.ones(n, np.uint8)
    failures, first, checks, diverged = set(), None, 0, 0
    for c in clients:
        for j in range(d):
            lj, rj = int(l[c, j]), int(r[c, j])
            for side in (0, 1):
                for p, x in enumerate(probes_of(lj, rj, int(a[c, j]), L)):
                    xb = bc.bits_of(x, L)
                    e0, s0, t0 = walk(oracle, k0, c, j, side, xb)
                    e1, s1, t1 = walk(oracle, k1, c, j, side, xb)
                    diverged += t0 == t1 and s0 != s1
                    for k in range(1, L + 1):
                        xp = x >> (L - k)
                        want = int(xp < (lj >> (L - k))) if side == 0 else int(xp > (rj >> (L - k)))
                        got = e0[k - 1] ^ e1[k - 1]
                        checks += 1
                        if got != want:
                            ok[c] = 0
                            failures.add((c, j, side, p, k))
                            if first is None or (c, j, side, p, k) < first[:5]:
                                first = (c, j, side, p, k, got, want)
    return {"ok": ok, "n_checks": checks, "n_bad_clients": int((ok == 0).sum()), "first": first, "failures": failures,
            "seed_diverged": diverged}


def report_first(rep):
    """The first-failure record of a report dict of KeyCollection.audit_keys_ball, as audit()'s `first`."""
    if rep["first_client"] is None:
        assert (rep["first_dim"], rep["first_side"], rep["first_probe"], rep["first_level"], rep["got"],
                rep["expected"]) == (0,) * 6
        return None
    return (rep["first_client"], rep["first_dim"], rep["first_side"], rep["first_probe"], rep["first_level"], rep["got"],
            rep["expected"])


def plan(n_dims, data_len, n, grid_blocks):
    """fhh_audit_plan in Python integers: an item is one wave's 64 clients of one key, on workgroups of 16 waves."""
    items = 2 * n_dims * ((n + 63) // 64)
    blocks = min((items + 15) // 16, grid_blocks)
    waves = 16 * blocks
    trips = (items + waves - 1) // waves
    checks = n * 2 * n_dims * PROBES * data_len
    return {"items": items, "waves": waves, "trips": trips, "last_trip_items": items - (trips - 1) * waves,
            "aes_blocks": 2 * checks, "n_checks": checks}


# ---- the tamper cases: each modifies the keys of client c, dim j in place and names itself ----
def flip_y_bit(ks, c, j, side, k, direction):
    """CorWord k's y control bit of `direction` (cw_bits nibble: bit 2 = y_bits.0, bit 3 = y_bits.1), in every
    dict of ks."""
    for k_ in ks:
        k_["cw_bits"][c, j, side, k] ^= 4 << direction


def flip_cw_seed_bit(ks, c, j, side, k, bit=0):
    for k_ in ks:
        k_["cw_seed"][c, j, side, k, bit // 8] ^= 1 << (bit % 8)


def flip_root_seed_bit(k, c, j, side, bit=9):
    k["root_seed"][c, j, side, bit // 8] ^= 1 << (bit % 8)


def swap_in_keys(ks, c, other_ks, c2):
    """client c gets the keys that other_ks (the keys of other points) hold for client c2"""
    for k_, o in zip(ks, other_ks):
        for f in FIELDS:
            k_[f][c] = o[f][c2]


def population(rng, L, d, n, delta):
    """n d points: the accepted constructed ones of ball_cases first (a = 0, whose l and l - 1 wrap, and
    a = 2^L - 1 - delta, whose r + 1 wraps to 0, among them), uniform ones after. Bits [n][d][L]."""
    acc, _ = bc.split_cases(L, delta)
    vals = [a for _, a in acc][:n * d]
    vals += bc.random_points(rng, n * d - len(vals), L, delta)
    return bc.alpha_array(vals, d, L)


def oracle_keys(oracle, rng, alpha, delta):
    """(k0, k1, (l, r, a)) of bit points alpha: the oracle's keys of the oracle's bounds, random root seeds."""
    n, d, _ = alpha.shape
    left, right = bc.oracle_bounds(oracle, alpha, delta)
    roots = rng.integers(0, 256, (n, d, 2, 2, 16), dtype=np.uint8)
    s0, s1 = oracle.gen_keys(left, right, roots)
    return keys_arrays(s0), keys_arrays(s1), bits_points(oracle, alpha, delta)
