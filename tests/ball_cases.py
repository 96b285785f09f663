"""Inputs shared by the fhh_ball_bounds (CPU) and fhh_gen_keys_ball (GPU) tests, with their CPU models: the
constructed points (borrow and carry ripples, the accept / refuse edge), the coordinate cases, the expected
bounds from the oracle's restatement of the reference (oracle.l_inf_ball_bounds, lib.rs:131-183, ibDCF.rs:175-188;
oracle.i16_to_bitvec, sample_driving_data.rs:25-28), the derived root seeds from oracle.chacha_block, and the
keygen launch arithmetic. Every condition a case is named for is asserted here on Python integers, without a GPU
and without the code under test."""
import numpy as np

DELTAS = (0, 1, 8, 2 ** 31, 2 ** 32 - 1)
LENGTHS = (32, 33, 40, 63, 64, 65, 100, 512)
GPU_LENGTHS = (32, 33, 64, 65, 100)
SEED = bytes((7 * i + 3) & 0xFF for i in range(32))

LATS = (-9000, -8999, 0, 8999, 9000, 9005, -32768, 32767)
LONGS = (-18000, 17999, 18000, 18001)
COORD_BALLS = (0, 1, 8, 32767)


def ripple_ks(L):
    return sorted({k for k in (31, 32, 33, 63, 64, 65, L - 1) if k <= L - 1})


def bits_of(a, L):
    """The L-bit string of a, MSB first."""
    assert 0 <= a < (1 << L)
    return [(a >> (L - 1 - l)) & 1 for l in range(L)]


def carries_out(a, delta, L):
    return a + delta >= (1 << L)


def wraps(a, delta):
    return a < delta


def constructed(L, delta):
    """{name: a} of the constructed points of length L for ball size delta; the conditions their names state are
    asserted here."""
    top = 1 << L
    pts = {"zero": 0}
    for k in ripple_ks(L):
        pts[f"one_then_{k}_zeros"] = 1 << k          # a borrow out of the low word ripples through k - 32 zeros
        pts[f"{k}_trailing_ones"] = (1 << k) - 1     # a carry out of the low word ripples through k - 32 ones
    pts["right_all_ones"] = top - 1 - delta
    if delta:
        pts["first_refused"] = top - delta
    assert pts["right_all_ones"] + delta == top - 1 and not carries_out(pts["right_all_ones"], delta, L)
    if delta:
        assert carries_out(pts["first_refused"], delta, L) and pts["first_refused"] + delta == top
        assert wraps(0, delta)
        for k in ripple_ks(L):
            if k >= 32 and delta > 0:   # the borrow crosses bit 32 and stops at bit k
                assert ((1 << k) - delta) >> 32 == (1 << (k - 32)) - 1
            if k >= 33:                 # the carry crosses bit 32 and stops at bit k
                assert (((1 << k) - 1 + delta) >> 32) == 1 << (k - 32)
    return pts


def split_cases(L, delta):
    """(accepted, refused): lists of (name, a) of constructed(L, delta), by the integer model."""
    pts = constructed(L, delta)
    acc = [(k, a) for k, a in pts.items() if not carries_out(a, delta, L)]
    ref = [(k, a) for k, a in pts.items() if carries_out(a, delta, L)]
    assert ("first_refused" in dict(ref)) == bool(delta) and "right_all_ones" in dict(acc) and "zero" in dict(acc)
    return acc, ref


def random_points(rng, count, L, delta):
    """count uniform L-bit points that a + delta does not carry out of (rejection by the integer model)."""
    out = []
    while len(out) < count:
        a = int.from_bytes(rng.bytes((L + 7) // 8), "big") >> ((-L) % 8)
        if delta and L <= 33:
            a %= max((1 << L) - delta, 1)
        if not carries_out(a, delta, L):
            out.append(a)
    return out


def alpha_array(values, d, L):
    """Python ints (n d of them, client-major) -> bits [n][d][L]."""
    assert len(values) % d == 0
    return np.array([bits_of(a, L) for a in values], np.uint8).reshape(-1, d, L)


def oracle_bounds(oracle, alpha, delta):
    """(left, right) [n][d][L] of bits alpha [n][d][L] by oracle.l_inf_ball_bounds; the oracle's assertion fails on
    a carry out, as the reference panics."""
    n, d, L = alpha.shape
    left, right = np.zeros_like(alpha), np.zeros_like(alpha)
    for c in range(n):
        for j in range(d):
            l, r = oracle.l_inf_ball_bounds([bool(b) for b in alpha[c, j]], delta)
            assert len(l) == L and len(r) == L
            left[c, j], right[c, j] = [int(b) for b in l], [int(b) for b in r]
    return left, right


def oracle_refuses(oracle, a, delta, L):
    try:
        oracle.l_inf_ball_bounds([bool(b) for b in bits_of(a, L)], delta)
    except AssertionError:
        return True
    return False


def derived_roots(oracle, seed, seed_first, n, d):
    """Root seeds [n][d][2 side][2 server][16]: the ChaCha20 block of counter (seed_first + c) d + j."""
    out = np.zeros((n, d, 64), np.uint8)
    for c in range(n):
        for j in range(d):
            out[c, j] = np.frombuffer(oracle.chacha_block(20, seed, (seed_first + c) * d + j), np.uint8)
    return out.reshape(n, d, 2, 2, 16)


def coord_points():
    """int16 [n][2]: every (lat, long) of the edge values."""
    return np.array([(la, lo) for la in LATS for lo in LONGS], np.int16)


def coords_bounds(oracle, pts, ball):
    """(left, right) [n][2][16]: (c -/+ ball) in exact integers, clamped to +-9000 / +-18000 (ibDCF.rs:190-193),
    through oracle.i16_to_bitvec."""
    n = pts.shape[0]
    left, right = np.zeros((n, 2, 16), np.uint8), np.zeros((n, 2, 16), np.uint8)
    for c in range(n):
        for j, lim in enumerate((9000, 18000)):
            v = int(pts[c, j])
            left[c, j] = [int(b) for b in oracle.i16_to_bitvec(max(-lim, min(lim, v - ball)))]
            right[c, j] = [int(b) for b in oracle.i16_to_bitvec(max(-lim, min(lim, v + ball)))]
    return left, right


def keygen_trips(n, d):
    """Passes of k_keygen's grid-stride loop: K nw items of one wave each, on at most 4096 workgroups of 8 waves
    (launch_keygen, csrc/fhh_kernels.hip)."""
    items = 2 * d * max((n + 63) // 64, 1)
    waves = min((items + 7) // 8, 4096) * 8
    return (items + waves - 1) // waves


assert keygen_trips(262_145, 4) == 2 and keygen_trips(262_144, 4) == 1 and keygen_trips(130, 3) == 1
