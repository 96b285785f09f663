"""fhh_audit_probes (CPU, no GPU): the host arithmetic of the audit's probes l - 1, l, a, r, r + 1 mod 2^L — the
arithmetic k_audit_keys shares through csrc/ball_src.h — against Python integers on the oracle's bounds
(audit_cases.py), bit for bit; and the model's own guards: untampered oracle keys are all ok, and every tamper case
of the GPU tests is flagged where it is stated to be."""
import ctypes

import numpy as np
import pytest

import audit_cases as ac
import ball_cases as bc

FHH_E_ARG = -1
LENGTHS = (32, 33, 40, 63, 64, 65, 100)


@pytest.mark.parametrize("L", LENGTHS)
def test_probes_of_constructed_points_equal_the_integers(oracle, L):
    """Every ball size at every constructed point the keygen accepts: a = 0 (l and l - 1 wrap), a = 2^L - 1 - ball
    (r + 1 wraps to 0), the borrow and carry ripples over k = 31 .. 33 and 63 .. 65 bits, and uniform points; at
    ball = 2^32 - 1 the offset ball + 1 of l - 1 and r + 1 has 33 bits."""
    import fuzzyheavyhitters_amd as fhh
    from fuzzyheavyhitters_amd import workload
    rng = np.random.default_rng(L)
    top = 1 << L
    for delta in bc.DELTAS:
        acc, _ = bc.split_cases(L, delta)
        names = dict(acc)
        assert names["zero"] == 0 and names["right_all_ones"] == top - 1 - delta
        vals = [a for _, a in acc] + bc.random_points(rng, 20, L, delta)
        for d in (1, 2):
            use = vals + vals[:len(vals) % d]
            alpha = bc.alpha_array(use, d, L)
            l, r, a = ac.bits_points(oracle, alpha, delta)
            want = ac.probe_bits(l, r, a, L)
            got = fhh.audit_probes(workload.pack_points(alpha), delta, n_dims=d, data_len=L)
            assert got.shape == want.shape and np.array_equal(got, want), (L, delta, d)
        # the wraps the case names promise, on the integers
        assert ac.probes_of((0 - delta) % top, delta, 0, L)[0] == (top - delta - 1) % top
        assert ac.probes_of(0, top - 1, top - 1 - delta, L)[4] == 0


def test_pad_bits_of_the_last_byte_are_ignored(oracle):
    import fuzzyheavyhitters_amd as fhh
    from fuzzyheavyhitters_amd import workload
    L, delta = 100, 2 ** 32 - 1
    alpha = ac.population(np.random.default_rng(1), L, 2, 12, delta)
    pts = workload.pack_points(alpha)
    assert pts.shape[-1] == 13
    dirty = pts.copy()
    dirty[..., -1] |= 0x0F   # string bits 100 .. 103 do not exist
    assert not np.array_equal(dirty, pts)
    l, r, a = ac.bits_points(oracle, alpha, delta)
    assert np.array_equal(fhh.audit_probes(dirty, delta, n_dims=2, data_len=L), ac.probe_bits(l, r, a, L))


@pytest.mark.parametrize("ball", bc.COORD_BALLS)
def test_coordinate_probes_at_the_clamp_edges(oracle, ball):
    import fuzzyheavyhitters_amd as fhh
    pts = bc.coord_points()
    l, r, a = ac.coords_points(oracle, pts, ball)
    got = fhh.audit_probes(pts, ball, n_dims=2, data_len=16, form="coords")
    assert np.array_equal(got, ac.probe_bits(l, r, a, 16))
    # a point outside the clamp is its own probe 2, outside [l, r]
    k = [tuple(p) for p in pts.tolist()].index((9005, -18000))
    assert int(a[k, 0]) == 9005 and int(r[k, 0]) == 9000


def test_a_carry_out_is_refused_naming_the_lowest_index(oracle):
    import fuzzyheavyhitters_amd as fhh
    from fuzzyheavyhitters_amd import workload
    from fuzzyheavyhitters_amd._lib import FhhBallSrc, ptr
    L, d, delta, n = 40, 2, 8, 30
    alpha = ac.population(np.random.default_rng(2), L, d, n, delta)
    first_refused = (1 << L) - delta
    assert bc.oracle_refuses(oracle, first_refused, delta, L)
    alpha[21, 0] = bc.bits_of(first_refused, L)
    alpha[3, 1] = bc.bits_of((1 << L) - 1, L)
    pts = workload.pack_points(alpha)
    with pytest.raises(fhh.FhhError, match=r"fhh error -1: .*client 3, dim 1"):
        fhh.audit_probes(pts, delta, n_dims=d, data_len=L)
    src = FhhBallSrc()
    src.form, src.ball, src.points = 0, delta, pts.ctypes.data
    out = np.full((n, d, 5, L), 7, np.uint8)
    bad = ctypes.c_uint64()
    assert fhh.lib().fhh_audit_probes(d, L, n, ctypes.byref(src), ptr(out), ctypes.byref(bad)) == FHH_E_ARG
    assert bad.value == 3 * d + 1 and (out == 7).all()
    # r + 1 alone wrapping is no carry out
    alpha[21, 0] = bc.bits_of((1 << L) - 1 - delta, L)
    alpha[3, 1] = 0
    pts2 = workload.pack_points(alpha)
    src.points = pts2.ctypes.data
    assert fhh.lib().fhh_audit_probes(d, L, n, ctypes.byref(src), None, ctypes.byref(bad)) == 0 and bad.value == 2 ** 64 - 1


def test_probe_argument_refusals():
    import fuzzyheavyhitters_amd as fhh
    from fuzzyheavyhitters_amd._lib import FhhBallSrc
    lib = fhh.lib()
    pts = np.zeros((4, 1, 5), np.uint8)
    xy = np.zeros((4, 2), np.int16)

    def call(d, L, form=0, ball=1, points=pts, src=True):
        s = FhhBallSrc()
        s.form, s.ball = form, ball
        s.points = points.ctypes.data if points is not None else None
        return lib.fhh_audit_probes(d, L, 4, ctypes.byref(s) if src else None, None, None)

    assert call(1, 40) == 0
    assert call(1, 40, src=False) == FHH_E_ARG and call(1, 40, points=None) == FHH_E_ARG
    assert call(1, 40, form=7) == FHH_E_ARG and call(1, 31) == FHH_E_ARG
    assert call(0, 40) == FHH_E_ARG and call(5, 40) == FHH_E_ARG
    assert call(1, 40, form=1, points=xy) == FHH_E_ARG and call(2, 16, form=1, ball=32768, points=xy) == FHH_E_ARG
    assert call(2, 16, form=1, ball=32767, points=xy) == 0


# ---- the model's guards ----
@pytest.fixture(scope="module")
def small(oracle):
    """12 clients, d = 2, L = 40, ball 8: the oracle's keys of the oracle's bounds."""
    L, d, n, delta = 40, 2, 12, 8
    rng = np.random.default_rng(40)
    alpha = ac.population(rng, L, d, n, delta)
    k0, k1, lra = ac.oracle_keys(oracle, rng, alpha, delta)
    return L, d, n, delta, alpha, k0, k1, lra


def copies(small):
    L, d, n, delta, alpha, k0, k1, lra = small
    return {f: v.copy() for f, v in k0.items()}, {f: v.copy() for f, v in k1.items()}


def test_untampered_oracle_keys_are_all_ok(oracle, small):
    L, d, n, delta, alpha, k0, k1, (l, r, a) = small
    m = ac.audit(oracle, k0, k1, l, r, a, L)
    assert m["ok"].all() and m["first"] is None and m["n_bad_clients"] == 0 and m["seed_diverged"] == 0
    assert m["n_checks"] == ac.plan(d, L, n, 1)["n_checks"] == n * 2 * d * 5 * L
    assert int(a[0, 0]) == 0 and int(l[0, 0]) == (1 << L) - delta    # a wrapped client among them


@pytest.mark.parametrize("copies_hit", ["both", "ctx1"])
@pytest.mark.parametrize("k", [0, 31, 32, 39])
def test_a_flipped_y_bit_is_flagged_at_the_bound_itself(oracle, small, k, copies_hit):
    """CorWord k's y bit of the direction l takes, left key of (client 5, dim 1). In both copies the walk of x = l
    has exactly one server with t = 1 at level k, so e flips at level k + 1 of probe 1, whatever the seeds."""
    L, d, n, delta, alpha, _, _, (l, r, a) = small
    k0, k1 = copies(small)
    c, j = 5, 1
    direction = (int(l[c, j]) >> (L - 1 - k)) & 1
    ac.flip_y_bit((k0, k1) if copies_hit == "both" else (k1,), c, j, 0, k, direction)
    m = ac.audit(oracle, k0, k1, l, r, a, L, clients=[c])
    if copies_hit == "both":
        assert (c, j, 0, 1, k + 1) in m["failures"]
        assert m["first"][:3] == (c, j, 0) and m["first"][4] == k + 1 and m["first"][3] in (0, 1)
    assert m["n_bad_clients"] == (1 if m["failures"] else 0) and all(f[:3] == (c, j, 0) for f in m["failures"])
    assert all(f[4] >= k + 1 for f in m["failures"])


def test_seed_tampers_change_no_compared_bit(oracle, small):
    """expand_dir reads its control bits from the nibble it has just zeroed (prg.rs:97-104): tau's bits are constants
    and no compared bit depends on a seed. A flipped CorWord seed bit and a flipped root seed bit leave every client
    ok; they show only where a walk leaves the path and the two servers' seeds must agree."""
    L, d, n, delta, alpha, _, _, (l, r, a) = small
    k0, k1 = copies(small)
    ac.flip_cw_seed_bit((k0, k1), 2, 0, 1, 17)
    ac.flip_root_seed_bit(k1, 7, 1, 0)
    m = ac.audit(oracle, k0, k1, l, r, a, L, clients=[2, 7])
    assert m["ok"].all() and m["first"] is None
    assert m["seed_diverged"] > 0


def test_keys_of_a_different_point_and_two_bad_clients(oracle, small):
    L, d, n, delta, alpha, _, _, (l, r, a) = small
    k0, k1 = copies(small)
    rng = np.random.default_rng(41)
    other = ac.population(rng, L, d, n, delta)[::-1].copy()
    o0, o1, (ol, _, _) = ac.oracle_keys(oracle, rng, other, delta)
    assert int(ol[9, 0]) != int(l[3, 0])
    ac.swap_in_keys((k0, k1), 3, (o0, o1), 9)
    ac.flip_y_bit((k0, k1), 10, 0, 1, 5, (int(r[10, 0]) >> (L - 1 - 5)) & 1)
    m = ac.audit(oracle, k0, k1, l, r, a, L)
    assert m["ok"].tolist() == [0 if c in (3, 10) else 1 for c in range(n)] and m["n_bad_clients"] == 2
    assert m["first"][0] == 3 and (10, 0, 1, 3, 6) in m["failures"]
