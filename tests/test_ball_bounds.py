"""fhh_ball_bounds (CPU, host arithmetic): the bounds and root seeds fhh_gen_keys_ball's kernel makes from a
population's points, against the oracle's restatement of the reference (ball_cases.py: oracle.l_inf_ball_bounds,
oracle.i16_to_bitvec, oracle.chacha_block) bit for bit, every refusal, and the compiler's report of the k_keygen
instantiations that compute them on the GPU."""
import ctypes

import numpy as np
import pytest

import ball_cases as bc
from kernel_usage import resource_usage

FHH_E_ARG = -1
NONE = 2 ** 64 - 1


def bounds(points, ball, d, L, form="bits", root_seeds=None, seed=bc.SEED, seed_first=0, want=(True, True, True)):
    """(rc, bad, left, right, roots) of fhh_ball_bounds; outputs pre-filled with a sentinel."""
    from fuzzyheavyhitters_amd import collection
    from fuzzyheavyhitters_amd._lib import lib, ptr
    src, n, keep = collection._ball_src(points, ball, form, d, L, root_seeds, seed, seed_first)
    left = np.full((n, d, L), 0xAA, np.uint8)
    right = np.full((n, d, L), 0xAA, np.uint8)
    roots = np.full((n, d, 2, 2, 16), 0xAA, np.uint8)
    bad = ctypes.c_uint64(12345)
    rc = lib().fhh_ball_bounds(d, L, n, ctypes.byref(src), ptr(left) if want[0] else None,
                               ptr(right) if want[1] else None, ptr(roots) if want[2] else None, ctypes.byref(bad))
    return rc, bad.value, left, right, roots


def test_abi_of_the_ball_source(fhh):
    from fuzzyheavyhitters_amd._lib import FhhBallSrc
    L = fhh.lib()
    assert ctypes.sizeof(FhhBallSrc) == 64 and FhhBallSrc.seed.offset == 24 and FhhBallSrc.seed_first.offset == 56
    assert L.fhh_ball_bounds.restype is ctypes.c_int and L.fhh_gen_keys_ball.restype is ctypes.c_int
    assert L.fhh_gen_keys_ball(None, None, 1, None) == FHH_E_ARG


@pytest.mark.parametrize("L", bc.LENGTHS)
def test_constructed_points_equal_the_oracle(fhh, oracle, L):
    """Borrow and carry ripples, the wrap at a = 0, the last accepted and the first refused point, at every ball
    size: the accepted ones in one call against the oracle, each refused one alone, and *bad = the lowest index
    when several offend."""
    from fuzzyheavyhitters_amd import workload
    for delta in bc.DELTAS:
        acc, ref = bc.split_cases(L, delta)
        for _, a in acc:
            assert not bc.oracle_refuses(oracle, a, delta, L)
        alpha = bc.alpha_array([a for _, a in acc], 1, L)
        want_l, want_r = bc.oracle_bounds(oracle, alpha, delta)
        if delta:   # the wrapped interval of a = 0: l = 2^L - delta > r = delta
            assert acc[0][0] == "zero" and bc.wraps(0, delta)
            assert want_l[0, 0].tolist() == bc.bits_of((1 << L) - delta, L) and want_r[0, 0].tolist() == bc.bits_of(delta, L)
        rc, bad, left, right, _ = bounds(workload.pack_points(alpha), delta, 1, L)
        assert rc == 0 and bad == NONE, (L, delta)
        assert np.array_equal(left, want_l) and np.array_equal(right, want_r), (L, delta)
        for name, a in ref:
            assert bc.oracle_refuses(oracle, a, delta, L), (name, delta)
            rc, bad, left, right, roots = bounds(workload.pack_points(bc.alpha_array([a], 1, L)), delta, 1, L)
            assert rc == FHH_E_ARG and bad == 0, (L, delta, name)
            assert b"client 0, dim 0" in fhh.lib().fhh_last_error(None)
            assert (left == 0xAA).all() and (right == 0xAA).all() and (roots == 0xAA).all()
        if ref:     # offenders at (client 2, dim 1) and (client 1, dim 0) among accepted points: the lowest is named
            vals = [acc[0][1]] * 6
            vals[2 * 2 + 1] = ref[0][1]
            vals[1 * 2 + 0] = ref[-1][1]
            rc, bad, *_ = bounds(workload.pack_points(bc.alpha_array(vals, 2, L)), delta, 2, L)
            assert rc == FHH_E_ARG and bad == 2
            assert b"client 1, dim 0" in fhh.lib().fhh_last_error(None)


@pytest.mark.parametrize("L", bc.LENGTHS)
def test_random_points_equal_the_oracle(fhh, oracle, L):
    """200 uniform points per length (100 clients x 2 dims) at every ball size; at L = 100 also with garbage in the
    pad bits of the last byte."""
    from fuzzyheavyhitters_amd import workload
    rng = np.random.default_rng(1000 + L)
    for delta in bc.DELTAS:
        alpha = bc.alpha_array(bc.random_points(rng, 200, L, delta), 2, L)
        want_l, want_r = bc.oracle_bounds(oracle, alpha, delta)
        pts = workload.pack_points(alpha)
        assert pts.shape == (100, 2, (L + 7) // 8)
        rc, bad, left, right, _ = bounds(pts, delta, 2, L)
        assert rc == 0 and bad == NONE
        assert np.array_equal(left, want_l) and np.array_equal(right, want_r), (L, delta)
        if L % 8:
            dirty = pts.copy()
            dirty[:, :, -1] |= rng.integers(0, 256, (100, 2), dtype=np.uint8) & ((1 << ((-L) % 8)) - 1)
            assert not np.array_equal(dirty, pts)
            rc, bad, left, right, _ = bounds(dirty, delta, 2, L)
            assert rc == 0 and np.array_equal(left, want_l) and np.array_equal(right, want_r), (L, delta)


def test_pack_points_layout():
    from fuzzyheavyhitters_amd import workload
    a = np.zeros((1, 1, 12), np.uint8)
    a[0, 0, [0, 9]] = 1
    assert workload.pack_points(a).tolist() == [[[0x80, 0x40]]]


def test_coordinates_equal_the_oracle(fhh, oracle):
    from fuzzyheavyhitters_amd import workload
    pts = bc.coord_points()
    assert pts.shape == (32, 2)
    for ball in bc.COORD_BALLS:
        want_l, want_r = bc.coords_bounds(oracle, pts, ball)
        rc, bad, left, right, _ = bounds(pts, ball, 2, 16, form="coords")
        assert rc == 0 and bad == NONE
        assert np.array_equal(left, want_l) and np.array_equal(right, want_r), ball
    # the clamp at work: 9005 - 1 and 32767 + 32767 end at 9000, -32768 - 32767 at -9000 (exact integers)
    l, r = bc.coords_bounds(oracle, np.array([[9005, 0], [32767, 0], [-32768, 0]], np.int16), 32767)
    assert r[0, 0].tolist() == r[1, 0].tolist() == [int(b) for b in oracle.i16_to_bitvec(9000)]
    assert l[2, 0].tolist() == [int(b) for b in oracle.i16_to_bitvec(-9000)]
    # the coordinate workload's own bounds (workload.coords_workload) from its points
    for ball in (1, 3):
        wl = workload.coords_workload(1000, ball_size=ball, num_centroids=50)
        w = 1 << np.arange(15, -1, -1)
        pts = (wl.alpha.astype(np.int64) * w).sum(-1).astype(np.uint16).view(np.int16).reshape(1000, 2)
        assert np.array_equal(workload.i16_to_bits(pts), wl.alpha)
        rc, bad, left, right, _ = bounds(pts, ball, 2, 16, form="coords")
        assert rc == 0 and np.array_equal(left, wl.left) and np.array_equal(right, wl.right)


@pytest.mark.parametrize("d", [1, 3])
@pytest.mark.parametrize("seed_first", [0, 5, 2 ** 32 - 3])
def test_derived_root_seeds_equal_chacha20(fhh, oracle, d, seed_first):
    from fuzzyheavyhitters_amd import workload
    n, L = 6, 32
    pts = workload.pack_points(np.zeros((n, d, L), np.uint8))
    rc, _, _, _, roots = bounds(pts, 0, d, L, seed_first=seed_first)
    assert rc == 0
    assert (seed_first + n) * d > 2 ** 32 or seed_first < 2 ** 31    # the last case crosses the counter's low word
    assert np.array_equal(roots, bc.derived_roots(oracle, bc.SEED, seed_first, n, d))
    # cutting the population does not change a client's seeds
    rc, _, _, _, tail = bounds(pts[2:], 0, d, L, seed_first=seed_first + 2)
    assert rc == 0 and np.array_equal(tail, roots[2:])
    # given root seeds are handed through
    given = np.random.default_rng(3).integers(0, 256, (n, d, 2, 2, 16), dtype=np.uint8)
    rc, _, _, _, out = bounds(pts, 0, d, L, root_seeds=given, seed=None)
    assert rc == 0 and np.array_equal(out, given)


def test_refusals_and_null_outputs(fhh):
    from fuzzyheavyhitters_amd import workload
    from fuzzyheavyhitters_amd._lib import FhhBallSrc, ptr
    lib = fhh.lib()
    bad = ctypes.c_uint64(7)
    pts = workload.pack_points(np.zeros((3, 1, 40), np.uint8))

    def call(d, L, n, src):
        return lib.fhh_ball_bounds(d, L, n, ctypes.byref(src) if src is not None else None, None, None, None,
                                   ctypes.byref(bad))

    def src_of(form=0, ball=1, points=pts):
        s = FhhBallSrc()
        s.form, s.ball = form, ball
        s.points = points.ctypes.data if points is not None else None
        return s

    assert call(1, 40, 3, src_of()) == 0 and bad.value == NONE                 # every output NULL
    assert lib.fhh_ball_bounds(1, 40, 3, ctypes.byref(src_of()), None, None, None, None) == 0   # and bad
    assert call(1, 40, 3, None) == FHH_E_ARG                                    # NULL source
    assert call(1, 40, 3, src_of(form=2)) == FHH_E_ARG                          # unknown form
    assert b"unknown form 2" in lib.fhh_last_error(None)
    assert call(1, 40, 3, src_of(points=None)) == FHH_E_ARG                     # NULL points
    assert call(1, 31, 3, src_of()) == FHH_E_ARG                                # the reference would pad to 32 levels
    assert b"32" in lib.fhh_last_error(None)
    assert call(0, 40, 3, src_of()) == FHH_E_ARG and call(5, 40, 3, src_of()) == FHH_E_ARG
    xy = np.zeros((3, 2), np.int16)
    assert call(2, 16, 3, src_of(form=1, points=xy)) == 0
    assert call(2, 16, 3, src_of(form=1, points=xy, ball=32767)) == 0
    assert call(2, 16, 3, src_of(form=1, points=xy, ball=32768)) == FHH_E_ARG   # ball out of range
    assert call(1, 16, 3, src_of(form=1, points=xy)) == FHH_E_ARG               # form / d / L mismatch
    assert call(2, 32, 3, src_of(form=1, points=xy)) == FHH_E_ARG
    assert bad.value == NONE
    # one output at a time
    alpha = bc.alpha_array([5, 6, 7], 1, 40)
    rc, _, left, right, roots = bounds(workload.pack_points(alpha), 1, 1, 40, want=(False, True, False))
    assert rc == 0 and (left == 0xAA).all() and (roots == 0xAA).all()
    assert right[:, 0].tolist() == [bc.bits_of(a + 1, 40) for a in (5, 6, 7)]
    with pytest.raises(fhh.FhhError):
        fhh.ball_bounds(pts, 1, n_dims=1, data_len=40)                          # no seed and no root seeds
    with pytest.raises(fhh.FhhError):
        fhh.ball_bounds(pts, 1, n_dims=2, data_len=40, seed=bc.SEED)            # shape
    l, r, _ = fhh.ball_bounds(pts, 1, n_dims=1, data_len=40, seed=bc.SEED)
    assert l.all() and r[:, :, :-1].sum() == 0 and r[:, :, -1].all()            # 0 - 1 wraps, 0 + 1


def test_keygen_point_forms_use_no_more_stack_than_the_byte_form():
    """k_keygen's instantiations in one compile: the point forms (1 packed bits, 2 coordinates) hold the bound's
    low word, a threshold and a 32-bit window beside the 4 AES blocks, and a ChaCha20 state before the level loop;
    their scratch and VGPR spill may not exceed the byte form's (0), at the same occupancy."""
    u = resource_usage("fhh_kernels.hip")
    name = "_ZN3fhh8k_keygenILi{}EEEvNS_10KeygenArgsE"
    base = u[name.format(0)]
    assert base["ScratchSize [bytes/lane]"] == "0" and base["VGPRs Spill"] == "0", base
    for form in (1, 2):
        k = u[name.format(form)]
        assert int(k["ScratchSize [bytes/lane]"]) <= int(base["ScratchSize [bytes/lane]"]), (form, k)
        assert int(k["VGPRs Spill"]) <= int(base["VGPRs Spill"]), (form, k)
        assert k["ScratchSize [bytes/lane]"] == "0" and k["VGPRs Spill"] == "0", (form, k)
        assert int(k["Occupancy [waves/SIMD]"]) >= int(base["Occupancy [waves/SIMD]"]), (form, k)
        assert k["LDS Size [bytes/block]"] == base["LDS Size [bytes/block]"], (form, k)
