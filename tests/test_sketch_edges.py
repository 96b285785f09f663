"""Row a9 at the inputs random workloads never reach (tests/test_sketch.py pins the common path):

  * rejected draws: FE::from_rng redraws when a draw's low 62 bits are >= p (about 2^-32 per draw).
    tests/golden/sketch_reject_seeds.json holds seeds that reject at chosen stream positions
    (made by tests/golden/make_sketch_reject_seeds.py); they drive the oracle's redraw loop and the
    kernels' detection (per-lane flag, __ballot, the key's segment mask) and sequential fallback;
  * non-canonical field inputs: include/fhh.h accepts FE values in any u64 representation and
    FieldElm values up to 2^256 - 1; the kernels are compared with Python ints there;
  * the third wrap of fe255_fold16, fired by constructed operand pairs.

The CPU tests pin the fixture, the oracle and the host arithmetic against Python ints; the GPU
tests (-m gpu) compare every kernel form bit for bit with Python ints, and with the oracle where
the CPU tests show that it agrees (sketch_fe everywhere; the FE Beaver steps only up to the
reference's lazy representation, so Python alone is their reference on arbitrary words)."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

from test_sketch import (P, P255, _ints, _py_sketch, _py_sketch255, _py_stream, _py_stream255,  # noqa: F401
                         sketch_impl)

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "sketch_reject_seeds.json")) as _f:
    FIXTURE = json.load(_f)
ENTRIES = FIXTURE["entries"]
REJ = {e["pos"]: bytes.fromhex(e["seed"]) for e in ENTRIES}
POSITIONS = [0, 1, 2, 3, 13, 37, 131, 258, 511, 512]
MASK62 = (1 << 62) - 1
M64 = (1 << 64) - 1

# every word class of a u64 FE input: canonical edges, p .. 2^62 (bit-reduce leaves them), bit 62 / 63
# set, multiples of p, the top of the range
EXTREME = [0, 1, P - 1, P, P + 1, 2**62 - 1, 2**62, 2**62 + 2**30, 2**63 - 1, 2**63, 2 * P, 2 * P + 1, 3 * P,
           2**64 - 2, 2**64 - 1]
# FieldElm words: values >= p up to 2^256 - 1 = 2 p + 37, and the canonical edges
EXTREME255 = [P255, P255 + 1, P255 + 18, 2 * P255, 2 * P255 + 37, 2**255 - 1, 2**255, 2**256 - 1,
              0, 1, 18, 19, P255 - 1, P255 - 19, P255 - 20]


def sweep_nodes(q):
    """n_nodes on both sides of rejected draw q (the stream has n_nodes + 3 live draws): at q - 3 the
    rejected draw is the first one past the stream, at q - 2 it is the last live draw (the redraw
    reads one draw more than the live count), at q + 5 it is in the middle."""
    return [q - 3, q - 2, q + 5] if q >= 3 else [0, 1, 9]


def draw_words(rng, words, shape):
    """u64 array of `shape` drawn from the list `words`"""
    w = np.array(words, np.uint64)
    return w[rng.integers(0, len(words), size=shape)]


def py_sketch_batch(seeds, x, kx):
    return np.array([_py_sketch(bytes(seeds[i]), [int(v) for v in x[i]], [int(v) for v in kx[i]])
                     for i in range(len(seeds))], np.uint64).reshape(len(seeds), 6)


# ---- MulState in Python ints (mpc.rs:83-212), either field ------------------------------------
def py_cor_share(sk6, mac, mac2, tr9, p):
    xs, ys = [sk6[0], mac, sk6[0]], [sk6[0], mac, mac]
    return [(xs[i] - tr9[3 * i]) % p for i in range(3)] + [(ys[i] - tr9[3 * i + 1]) % p for i in range(3)]


def py_out_share(server_idx, sk6, mac, mac2, tr9, cor6, p):
    zs = [-sk6[1], -mac2, -sk6[2]]
    out = 0
    for i in range(3):
        d, e = cor6[i], cor6[3 + i]
        a, b, c = tr9[3 * i: 3 * i + 3]
        out += sk6[3 + i] * ((d * e if server_idx else 0) + d * b + e * a + c + zs[i])
    return out % p


def py_verify(sk, mac, mac2, tr, p):
    """both servers' cor shares, cor, out shares, ok for one key: sk [2][6], mac / mac2 [2], tr [2][9]"""
    cs = [py_cor_share(sk[s], mac[s], mac2[s], tr[s], p) for s in range(2)]
    cor = [(a + b) % p for a, b in zip(*cs)]
    o = [py_out_share(s, sk[s], mac[s], mac2[s], tr[s], cor, p) for s in range(2)]
    return (o[0] + o[1]) % p == 0, o


def ints_of(a):
    return [int(v) for v in np.asarray(a).ravel()]


# ================================================================================================
# CPU: the fixture, the oracle and the host arithmetic
# ================================================================================================
def test_reject_fixture_shape():
    assert [e["pos"] for e in ENTRIES] == POSITIONS
    assert int(FIXTURE["p"], 16) == P and FIXTURE["n_draws"] == 1100
    for e in ENTRIES:
        assert e["rejects"] == [e["pos"]]           # one rejected draw per seed: the GPU tests rely on it
        assert P <= int(e["value"], 16) <= MASK62


@pytest.mark.parametrize("entry", ENTRIES, ids=[f"q{e['pos']}" for e in ENTRIES])
def test_reject_fixture_rejects_per_openssl_and_oracle(oracle, entry):
    """each fixture seed rejects at its stated positions and nowhere else in its first 1100 draws, by
    the OpenSSL-backed stream and by the oracle's; the seed is the generator's candidate `counter`,
    the search's own AES path draws the same stream, and the search finds it again"""
    seed, q = bytes.fromhex(entry["seed"]), entry["pos"]
    st = _py_stream(seed)
    py = [next(st) for _ in range(FIXTURE["n_draws"])]
    assert [k for k, v in enumerate(py) if (v & MASK62) >= P] == entry["rejects"]
    assert (py[q] & MASK62) == int(entry["value"], 16)
    assert [oracle.prg_stream_u64(seed, k) for k in range(FIXTURE["n_draws"])] == py
    c = entry["counter"]
    assert oracle.reject_seed_of(c) == seed
    for k in (0, 1, q, q ^ 1, 600, 1099):
        assert oracle.reject_search_draw(c, k) == py[k]
    assert oracle.find_reject_seed(POSITIONS, c - 3000, 6000) == [(c, q, int(entry["value"], 16))]


def test_reject_known_seeds(oracle):
    """two seeds found by an independent run of the same kind of search: draw 3 is rejected"""
    for hexseed, v3 in (("41fcd41117480c9a4cbd31363d145c0d", 0x3fffffffc4f92583),
                        ("700068a927a96c8c83dac30ed5e32cf4", 0x3fffffffe95b1bee)):
        seed = bytes.fromhex(hexseed)
        st = _py_stream(seed)
        py = [next(st) for _ in range(8)]
        assert py[3] & MASK62 == v3 >= P and oracle.prg_stream_u64(seed, 3) == py[3]
        x, kx = np.array([[5, P - 1, 7]], np.uint64), np.array([[1, 2, 3]], np.uint64)
        got = oracle.sketch_fe(np.frombuffer(seed, np.uint8)[None], x, kx)
        assert ints_of(got[0]) == _py_sketch(seed, ints_of(x), ints_of(kx))


@functools.lru_cache(maxsize=None)
def reject_case(q, n_nodes, n_keys=70):
    """the single-server rejection case of position q: n_keys keys of random canonical x / kx, q's
    fixture seed at keys 0, 7 (the last 8-lane segment of wave 0), 8, 35 and 36 (adjacent), 69 (the
    last key of the ragged last wave), a different fixture seed at 37 (two rejecting keys side by
    side), random seeds elsewhere -> (seeds, clean seeds, x, kx, Python reference [n][6])"""
    from fuzzyheavyhitters_amd import sketch as S
    wl = S.sketch_workload(n_keys, n_nodes, seed=1000 + 7 * q + n_nodes)
    clean = wl.seeds.copy()
    seeds = wl.seeds.copy()
    other = POSITIONS[(POSITIONS.index(q) + 1) % len(POSITIONS)]
    for i in (0, 7, 8, 35, 36, 69):
        seeds[i] = np.frombuffer(REJ[q], np.uint8)
    seeds[37] = np.frombuffer(REJ[other], np.uint8)
    x, kx = wl.x[0], wl.kx[0]
    exp = py_sketch_batch(seeds, x, kx)
    for a in (seeds, clean, x, kx, exp):
        a.setflags(write=False)
    return seeds, clean, x, kx, exp


@pytest.mark.parametrize("q", POSITIONS)
def test_oracle_redraw_vs_python(oracle, q):
    """the oracle's fe_from_stream redraw loop against the Python restatement, with n_nodes on both
    sides of the rejected draw"""
    for n_nodes in sweep_nodes(q):
        seeds, _, x, kx, exp = reject_case(q, n_nodes)
        assert np.array_equal(oracle.sketch_fe(seeds, x, kx), exp), f"n_nodes {n_nodes}"
    # the redraw shifts every later draw by one: the rejecting key differs from a plain slice of the stream
    n_nodes = sweep_nodes(q)[2]
    seeds, _, x, kx, exp = reject_case(q, n_nodes)
    st = _py_stream(REJ[q])
    draws = [next(st) & MASK62 for _ in range(4)]
    if q < 3:
        assert ints_of(exp[0][3:6]) == [d for k, d in enumerate(draws) if k != q]


@functools.lru_cache(maxsize=None)
def extreme_case(n_keys, n_nodes):
    """x / kx drawn from EXTREME; key 0 is all 2^64 - 1, key 1 alternates 2^64 - 1 and 0 (x) and 0 and
    2^64 - 1 (kx) -> (seeds, x, kx, Python reference)"""
    rng = np.random.default_rng([n_keys, n_nodes, 62])
    seeds = rng.integers(0, 256, size=(n_keys, 16), dtype=np.uint8)
    x, kx = draw_words(rng, EXTREME, (n_keys, n_nodes)), draw_words(rng, EXTREME, (n_keys, n_nodes))
    x[0], kx[0] = M64, M64
    x[1, 0::2], x[1, 1::2] = M64, 0
    kx[1, 0::2], kx[1, 1::2] = 0, M64
    exp = py_sketch_batch(seeds, x, kx)
    for a in (seeds, x, kx, exp):
        a.setflags(write=False)
    return seeds, x, kx, exp


EXTREME_SHAPES = [(5, 2), (70, 63), (130, 125), (300, 700)]


@pytest.mark.parametrize("n_keys,n_nodes", [(16, 37), (5, 2)])
def test_oracle_sketch_extreme_words_vs_python(oracle, n_keys, n_nodes):
    seeds, x, kx, exp = extreme_case(n_keys, n_nodes)
    if n_keys * n_nodes > 500:
        assert set(EXTREME) <= set(ints_of(x)) and set(EXTREME) <= set(ints_of(kx))
    assert np.array_equal(oracle.sketch_fe(seeds, x, kx), exp)


@functools.lru_cache(maxsize=None)
def extreme_case255(n_keys, n_nodes):
    """FieldElm x / kx [n][nodes][8] drawn from EXTREME255 (key 0 all 2^256 - 1) -> (seeds, x, kx,
    Python reference [n][6][8])"""
    from fuzzyheavyhitters_amd import sketch as S
    rng = np.random.default_rng([n_keys, n_nodes, 255])
    seeds = rng.integers(0, 256, size=(n_keys, 16), dtype=np.uint8)
    words = np.stack([S.int_to_fe8(v) for v in EXTREME255])
    x = words[rng.integers(0, len(words), size=(n_keys, n_nodes))]
    kx = words[rng.integers(0, len(words), size=(n_keys, n_nodes))]
    x[0], kx[0] = 0xFFFFFFFF, 0xFFFFFFFF
    exp = np.array([[S.int_to_fe8(v) for v in _py_sketch255(bytes(seeds[i]), _ints(x[i]), _ints(kx[i]))]
                    for i in range(n_keys)], np.uint32).reshape(n_keys, 6, 8)
    for a in (seeds, x, kx, exp):
        a.setflags(write=False)
    return seeds, x, kx, exp


def test_oracle_sketch_fe255_noncanonical_vs_python(oracle):
    """the oracle's FieldElm sketch accepts limbs >= p (any value below 2^256), as sketch_at_last's
    lazy BigUint ops do"""
    seeds, x, kx, exp = extreme_case255(9, 13)
    assert np.array_equal(oracle.sketch_fe255(seeds, x, kx), exp)


@functools.lru_cache(maxsize=None)
def beaver_rows(n=64):
    """n rows of {sketch6, mac, mac2, triples9, cor6} u64 words drawn from EXTREME (every word of
    EXTREME occurs in every column set)"""
    rng = np.random.default_rng(606)
    rows = dict(sk=draw_words(rng, EXTREME, (n, 6)), mac=draw_words(rng, EXTREME, (n,)),
                mac2=draw_words(rng, EXTREME, (n,)), tr=draw_words(rng, EXTREME, (n, 9)),
                cor=draw_words(rng, EXTREME, (n, 6)))
    for k in range(len(EXTREME)):          # a diagonal, so no word depends on the draw to appear
        rows["sk"][k, k % 6] = rows["tr"][k, k % 9] = rows["cor"][k, (k + 1) % 6] = EXTREME[k]
        rows["mac"][k] = rows["mac2"][(k + 1) % n] = EXTREME[k]
    for a in rows.values():
        a.setflags(write=False)
    return rows


def test_host_mul_cor_and_verify_any_u64(fhh):
    """fhh_mul_cor_fe / fhh_mul_verify_fe (host arithmetic) on any-u64 words against Python ints"""
    from fuzzyheavyhitters_amd import sketch as S
    r = beaver_rows()
    s0, s1 = r["sk"], r["cor"]
    cor = S.mul_cor(s0, s1)
    assert ints_of(cor) == [(a % P + b % P) % P for a, b in zip(ints_of(s0), ints_of(s1))]
    o0 = np.array(EXTREME * len(EXTREME), np.uint64)
    o1 = np.repeat(np.array(EXTREME, np.uint64), len(EXTREME))
    # and pairs that do cancel: o1 = -o0 in several representations
    neg = np.array([(-v) % P for v in EXTREME] + [(-v) % P + P for v in EXTREME], np.uint64)
    o0 = np.concatenate([o0, np.array(EXTREME * 2, np.uint64)])
    o1 = np.concatenate([o1, neg])
    ok = S.mul_verify(o0, o1)
    exp = [(a + b) % P == 0 for a, b in zip(ints_of(o0), ints_of(o1))]
    assert list(ok) == exp and sum(exp) >= 2 * len(EXTREME)


# ---- the FieldElm fold's third carry ------------------------------------------------------------
def fold_third_carry(a, b):
    """restates fe255_fold16's three folds of the 512-bit product a b: True when the second fold's
    carry wraps past 2^256 once more (the `if (c)` branch)"""
    x = a * b
    lo, hi = x & ((1 << 256) - 1), x >> 256
    v = lo + 38 * hi
    c, out = v >> 256, v & ((1 << 256) - 1)
    return (out + 38 * c) >> 256 == 1


@functools.lru_cache(maxsize=None)
def fold_pairs():
    """(a, b, s): a even a little below p, b = s / a mod p for an even s in [38, 76), kept when the
    product fires the third carry of fe255_fold16; a b mod p = s"""
    rng = np.random.default_rng(2550)
    out = []
    for k in range(80):
        s = 38 + 2 * (k % 19)
        a = (P255 - 1 - int.from_bytes(rng.bytes(25), "little")) & ~1
        b = s * pow(a, -1, P255) % P255
        if a * b % (2 * P255) == s and fold_third_carry(a, b):
            out.append((a, b, s))
    return tuple(out)


def test_fold_pairs_survive():
    pairs = fold_pairs()
    assert len(pairs) >= 32, len(pairs)
    for a, b, s in pairs:
        assert a * b % P255 == s and a < P255 and b < P255


@functools.lru_cache(maxsize=None)
def fold_sketch_case():
    """a seed and x_0 whose product with node 0's draw r fires the third carry inside the sketch:
    x_0 = s / r mod p for the first even s in [38, 76) that passes -> (seed, x_0, r, s) or None"""
    for k in range(64):
        seed = bytes(np.random.default_rng([k, 77]).integers(0, 256, 16, dtype=np.uint8))
        st = _py_stream255(seed)
        r = [next(st) for _ in range(4)][3]
        for s in range(38, 76, 2):
            x0 = s * pow(r, -1, P255) % P255
            if fold_third_carry(x0, r):
                return seed, x0, r, s
    return None


def test_fold_sketch_case_found():
    assert fold_sketch_case() is not None


# ================================================================================================
# GPU: every kernel form, bit for bit
# ================================================================================================
@pytest.fixture(scope="module")
def kc():
    import fuzzyheavyhitters_amd as fhh
    return fhh.KeyCollection(8, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("q", POSITIONS)
def test_gpu_sketch_rejected_draw(oracle, kc, q, sketch_impl):
    """a rejected draw at stream position q: the rejecting keys (first and last segment of a wave,
    adjacent keys, two different rejecting seeds side by side, the last key of a ragged wave) and
    every clean key beside them equal Python ints and the oracle; the clean keys equal their value in
    an all-clean run"""
    from fuzzyheavyhitters_amd import sketch as S
    for n_nodes in sweep_nodes(q):
        seeds, clean, x, kx, exp = reject_case(q, n_nodes)
        got = S.sketch_at(kc, seeds, x, kx)
        bad = np.nonzero((got != exp).any(axis=1))[0]
        assert bad.size == 0, f"n_nodes {n_nodes}: keys {bad.tolist()} differ from Python"
        assert np.array_equal(got, oracle.sketch_fe(seeds, x, kx)), f"n_nodes {n_nodes}"
        base = S.sketch_at(kc, clean, x, kx)
        same = (seeds == clean).all(axis=1)
        assert same.sum() == 70 - 7
        assert np.array_equal(got[same], base[same]), f"n_nodes {n_nodes}: a clean key changed"
        assert np.array_equal(base, oracle.sketch_fe(clean, x, kx)), f"n_nodes {n_nodes}"


def _tail_plan(fhh, n_nodes):
    """(n_keys, n_main) of a default-form launch plan that has a tail on this device: the (40000, 256)
    shape of test_gpu_sketch_at_bit_exact, or the smallest n_keys with a tail"""
    lib = fhh.lib()
    cus = ctypes.c_int()
    name = ctypes.create_string_buffer(64)
    assert lib.fhh_device_info(0, name, 64, ctypes.byref(cus)) == 0

    def plan(n):
        nm, lm, lt = ctypes.c_uint64(), ctypes.c_int(), ctypes.c_int()
        assert lib.fhh_sketch_plan(n, n_nodes, 16 * cus.value, ctypes.byref(nm), ctypes.byref(lm),
                                   ctypes.byref(lt)) == 0
        return nm.value
    n_keys = 40000
    if plan(n_keys) == n_keys:
        n_keys = next(n for n in range(1, 1 << 22) if plan(n) < n)
    return n_keys, plan(n_keys)


@pytest.mark.gpu
def test_gpu_sketch_rejected_draw_in_tail_launch(oracle, fhh, kc):
    """the default form's planned tail launch (the producer / consumer kernel behind the main launch):
    rejecting keys as the main launch's last key, the tail's first and the tail's last, with the
    rejected draw in the middle (131) and at the last live draw (258 = n_nodes + 2)"""
    from fuzzyheavyhitters_amd import sketch as S
    assert fhh.lib().fhh_sketch_set_impl(0) == 0
    n_nodes = 256
    n_keys, n_main = _tail_plan(fhh, n_nodes)
    assert 0 < n_main < n_keys
    wl = S.sketch_workload(n_keys, n_nodes, seed=n_keys * 7 + n_nodes)
    x, kx = wl.x[0], wl.kx[0]
    at = [n_main - 1, n_main, n_keys - 1]
    near = sorted({i + d for i in at for d in (-1, 0, 1) if 0 <= i + d < n_keys})
    for qs in ((258, 131, 258), (131, 258, 131)):
        seeds = wl.seeds.copy()
        for i, q in zip(at, qs):
            seeds[i] = np.frombuffer(REJ[q], np.uint8)
        got = S.sketch_at(kc, seeds, x, kx)
        assert np.array_equal(got[near], py_sketch_batch(seeds[near], x[near], kx[near])), qs
        exp = oracle.sketch_fe(seeds, x, kx)
        bad = np.nonzero((got != exp).any(axis=1))[0]
        assert bad.size == 0, f"{qs}: keys {bad[:8].tolist()} differ from the oracle (n_main {n_main})"


def _fused_workload():
    from fuzzyheavyhitters_amd import sketch as S
    wl = S.sketch_workload(300, 40, seed=303, bad_fraction=0.1)
    for i, q in ((0, 3), (150, 13), (299, 37)):
        wl.seeds[i] = np.frombuffer(REJ[q], np.uint8)
    return wl


@pytest.mark.gpu
def test_gpu_sim_sketch_verify_rejected_draw(oracle, kc, sketch_impl):
    """the two-server fused form: both servers' sketches of a rejecting key take the fallback"""
    from fuzzyheavyhitters_amd import sketch as S
    wl = _fused_workload()
    b = S.DeviceSketchBatch(wl)
    S.sim_sketch_verify(kc, b)
    ok = b.ok[0].cpu().numpy().astype(bool)
    outs = b.out_shares[0].cpu().numpy().view(np.uint64)
    ok_e, outs_e = oracle.sketch_verify_fe(wl.seeds, wl.x[0], wl.kx[0], wl.x[1], wl.kx[1], np.stack(wl.mac),
                                           np.stack(wl.mac2), np.stack(wl.triples))
    assert np.array_equal(ok, wl.honest)
    assert np.array_equal(ok, ok_e) and np.array_equal(outs, outs_e)
    # the rejecting keys against Python ints, both servers
    for i in (0, 150, 299):
        sk = [_py_sketch(bytes(wl.seeds[i]), ints_of(wl.x[s][i]), ints_of(wl.kx[s][i])) for s in range(2)]
        _, o = py_verify(sk, [int(wl.mac[s][i]) for s in range(2)], [int(wl.mac2[s][i]) for s in range(2)],
                         [ints_of(wl.triples[s][i]) for s in range(2)], P)
        assert [int(outs[0][i]), int(outs[1][i])] == o, f"key {i}"


@pytest.mark.gpu
def test_gpu_sketch_verify_level_batch_rejected_draw(oracle, kc, sketch_impl):
    """levels [2, 7) in one call; keys 150 and 299 are stored as a fixture seed with bytes 12..15 ^ 4,
    so their level-4 stream (seed ^ level) is the rejecting one and the other levels' are not"""
    from fuzzyheavyhitters_amd import sketch as S
    wl = S.sketch_workload(300, 40, seed=404, bad_fraction=0.1)
    four = np.frombuffer(np.uint32(4).tobytes(), np.uint8)
    for i, q in ((150, 13), (299, 37)):
        wl.seeds[i] = np.frombuffer(REJ[q], np.uint8)
        wl.seeds[i, 12:16] ^= four
    b = S.DeviceSketchBatch(wl)
    S.deal_triples(kc, b, levels=8, seed=78)
    S.sim_sketch_verify(kc, b, level=2, n_levels=5)
    tr = [t.cpu().numpy().view(np.uint64) for t in b.triples]
    ok = b.ok.cpu().numpy()
    outs = b.out_shares.cpu().numpy().view(np.uint64)
    for k, lv in enumerate(range(2, 7)):
        seeds = wl.seeds.copy()
        seeds[:, 12:16] ^= np.frombuffer(np.uint32(lv).tobytes(), np.uint8)
        assert (bytes(seeds[150]) == REJ[13]) == (lv == 4) and (bytes(seeds[299]) == REJ[37]) == (lv == 4)
        ok_e, outs_e = oracle.sketch_verify_fe(seeds, wl.x[0], wl.kx[0], wl.x[1], wl.kx[1], np.stack(wl.mac),
                                               np.stack(wl.mac2), np.stack([tr[0][:, lv], tr[1][:, lv]]))
        assert np.array_equal(ok[k].astype(bool), ok_e), f"level {lv}"
        assert np.array_equal(outs[k], outs_e), f"level {lv}"
        assert np.array_equal(ok_e, wl.honest)


@pytest.mark.gpu
@pytest.mark.parametrize("n_keys,n_nodes", EXTREME_SHAPES)
def test_gpu_sketch_at_extreme_words(oracle, kc, n_keys, n_nodes, sketch_impl):
    """x / kx in any u64 representation (bit 62 / 63 set, multiples of p, all ones): Python ints and
    the oracle"""
    from fuzzyheavyhitters_amd import sketch as S
    seeds, x, kx, exp = extreme_case(n_keys, n_nodes)
    got = S.sketch_at(kc, seeds, x, kx)
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert bad.size == 0, f"keys {bad[:8].tolist()} differ from Python"
    assert np.array_equal(got, oracle.sketch_fe(seeds, x, kx))


def add_multiples_of_p(a, rng):
    """a canonical u64 array with k p added per word, k in {1, 2, 3, 4} where the sum fits a u64
    (k <= 3 always fits; 4 p + w needs w < 2^32 + 4)"""
    k = rng.integers(1, 5, size=a.shape).astype(np.uint64)
    k = np.where((k == 4) & (a >= np.uint64(2**32 + 4)), np.uint64(3), k)
    out = a + k * np.uint64(P)
    assert all(int(o) == int(v) + int(kk) * P for o, v, kk in zip(out.ravel()[:64], a.ravel()[:64], k.ravel()[:64]))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("n_keys,n_nodes", EXTREME_SHAPES)
def test_gpu_sketch_at_representation_invariant(kc, n_keys, n_nodes, sketch_impl):
    """metamorphic: adding multiples of p to the words of a canonical workload changes no output"""
    from fuzzyheavyhitters_amd import sketch as S
    wl = S.sketch_workload(n_keys, n_nodes, seed=5000 + n_keys)
    rng = np.random.default_rng(n_keys)
    x, kx = wl.x[0].copy(), wl.kx[0].copy()
    x[:, 0] = rng.integers(0, 6, size=n_keys).astype(np.uint64)     # small words: 4 p + w fits
    kx[:, -1] = rng.integers(0, 2**32, size=n_keys).astype(np.uint64)
    base = S.sketch_at(kc, wl.seeds, x, kx)
    x2, kx2 = add_multiples_of_p(x, rng), add_multiples_of_p(kx, rng)
    x2[:, 0] = x[:, 0] + np.uint64(4 * P)                           # k = 4 on every key, not by the draw
    kx2[:, -1] = kx[:, -1] + np.uint64(4 * P)
    assert (x2 >= np.uint64(P)).all() and (kx2 >= np.uint64(P)).all() and (x2[:, 0] >= np.uint64(4 * P)).all()
    assert np.array_equal(S.sketch_at(kc, wl.seeds, x2, kx2), base)


@pytest.mark.gpu
@pytest.mark.parametrize("n_keys,n_nodes", [(70, 63), (300, 700)])
def test_gpu_sim_sketch_verify_representation_invariant(kc, n_keys, n_nodes, sketch_impl):
    """metamorphic, two-server fused form: multiples of p added to x, kx, mac, mac2 and the triples
    leave ok == honest and both out shares unchanged"""
    from fuzzyheavyhitters_amd import sketch as S
    wl = S.sketch_workload(n_keys, n_nodes, seed=6000 + n_keys, bad_fraction=0.1)
    b = S.DeviceSketchBatch(wl)
    S.sim_sketch_verify(kc, b)
    ok, outs = b.ok[0].cpu().numpy().astype(bool), b.out_shares[0].cpu().numpy().view(np.uint64).copy()
    assert np.array_equal(ok, wl.honest) and not wl.honest.all()
    rng = np.random.default_rng(n_nodes)
    for name in ("x", "kx", "mac", "mac2", "triples"):
        setattr(wl, name, [add_multiples_of_p(a, rng) for a in getattr(wl, name)])
    b2 = S.DeviceSketchBatch(wl)
    S.sim_sketch_verify(kc, b2)
    assert np.array_equal(b2.ok[0].cpu().numpy().astype(bool), wl.honest)
    assert np.array_equal(b2.out_shares[0].cpu().numpy().view(np.uint64), outs)


@pytest.mark.gpu
def test_gpu_mul_steps_any_u64(kc):
    """mul_cor_share and mul_out_share (both server indices) on rows of extreme words, against the
    Python formulas on the inputs mod p (the oracle's Beaver steps restate the reference's lazy
    representation and are not defined up here)"""
    from fuzzyheavyhitters_amd import sketch as S
    r = beaver_rows()
    n = r["sk"].shape[0]
    cs = S.mul_cor_share(kc, r["sk"], r["mac"], r["mac2"], r["tr"])
    for i in range(n):
        exp = py_cor_share(ints_of(r["sk"][i]), int(r["mac"][i]), int(r["mac2"][i]), ints_of(r["tr"][i]), P)
        assert ints_of(cs[i]) == exp, f"row {i}"
    for s in (0, 1):
        o = S.mul_out_share(kc, s, r["sk"], r["mac"], r["mac2"], r["tr"], r["cor"])
        for i in range(n):
            exp = py_out_share(s, ints_of(r["sk"][i]), int(r["mac"][i]), int(r["mac2"][i]), ints_of(r["tr"][i]),
                               ints_of(r["cor"][i]), P)
            assert int(o[i]) == exp, f"server {s} row {i}"


@pytest.mark.gpu
def test_gpu_sim_sketch_verify_any_u64(kc, sketch_impl):
    """the fused two-server check with x, kx, mac, mac2 and the triples drawn from the extreme words:
    ok and both out shares equal Python ints"""
    from fuzzyheavyhitters_amd import sketch as S
    n, F = 64, 5
    rng = np.random.default_rng(707)
    seeds = rng.integers(0, 256, size=(n, 16), dtype=np.uint8)
    d = lambda *shape: [draw_words(rng, EXTREME, shape) for _ in range(2)]   # noqa: E731
    wl = S.SketchWorkload(seeds, d(n, F), d(n, F), d(n), d(n), d(n, 9), np.zeros(n, bool))
    b = S.DeviceSketchBatch(wl)
    S.sim_sketch_verify(kc, b)
    ok, outs = b.ok[0].cpu().numpy().astype(bool), b.out_shares[0].cpu().numpy().view(np.uint64)
    for i in range(n):
        sk = [_py_sketch(bytes(seeds[i]), ints_of(wl.x[s][i]), ints_of(wl.kx[s][i])) for s in range(2)]
        ok_e, o = py_verify(sk, [int(wl.mac[s][i]) for s in range(2)], [int(wl.mac2[s][i]) for s in range(2)],
                            [ints_of(wl.triples[s][i]) for s in range(2)], P)
        assert [int(outs[0][i]), int(outs[1][i])] == o and bool(ok[i]) == ok_e, f"key {i}"


# ---- FieldElm -----------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n_keys,n_nodes", [(9, 13), (70, 63)])
def test_gpu_sketch_at_fe255_extreme_words(oracle, kc, n_keys, n_nodes):
    from fuzzyheavyhitters_amd import sketch as S
    seeds, x, kx, exp = extreme_case255(n_keys, n_nodes)
    got = S.sketch_at_fe255(kc, seeds, x, kx)
    bad = np.nonzero((got != exp).any(axis=(1, 2)))[0]
    assert bad.size == 0, f"keys {bad[:8].tolist()} differ from Python"
    assert np.array_equal(got, oracle.sketch_fe255(seeds, x, kx))


def _fe8(rows):
    from fuzzyheavyhitters_amd.sketch import int_to_fe8
    a = np.asarray(rows, object)
    return np.array([int_to_fe8(int(v)) for v in a.ravel()], np.uint32).reshape(*a.shape, 8)


@functools.lru_cache(maxsize=None)
def beaver_rows255(n=64):
    rng = np.random.default_rng(255255)
    pick = lambda *shape: np.array(EXTREME255, object)[rng.integers(0, len(EXTREME255), size=shape)]   # noqa: E731
    rows = dict(sk=pick(n, 6), mac=pick(n), mac2=pick(n), tr=pick(n, 9), cor=pick(n, 6))
    for k in range(len(EXTREME255)):
        rows["sk"][k, k % 6] = rows["tr"][k, k % 9] = rows["cor"][k, (k + 1) % 6] = EXTREME255[k]
        rows["mac"][k] = rows["mac2"][(k + 1) % n] = EXTREME255[k]
    return rows


@pytest.mark.gpu
def test_gpu_mul_steps_fe255_any_value(kc):
    """mul_cor_share_fe255 / mul_out_share_fe255 on limbs >= p and the canonical edges"""
    from fuzzyheavyhitters_amd import sketch as S
    r = beaver_rows255()
    n = len(r["mac"])
    a = {k: _fe8(v) for k, v in r.items()}
    cs = S.mul_cor_share_fe255(kc, a["sk"], a["mac"], a["mac2"], a["tr"])
    for i in range(n):
        assert _ints(cs[i]) == py_cor_share(list(r["sk"][i]), r["mac"][i], r["mac2"][i], list(r["tr"][i]), P255), i
    for s in (0, 1):
        o = S.mul_out_share_fe255(kc, s, a["sk"], a["mac"], a["mac2"], a["tr"], a["cor"])
        for i in range(n):
            exp = py_out_share(s, list(r["sk"][i]), r["mac"][i], r["mac2"][i], list(r["tr"][i]), list(r["cor"][i]),
                               P255)
            assert _ints(o[i]) == [exp], f"server {s} row {i}"


@pytest.mark.gpu
@pytest.mark.parametrize("n_keys,n_nodes", [(9, 13), (70, 63)])
def test_gpu_sim_sketch_verify_fe255_any_value(kc, n_keys, n_nodes):
    from fuzzyheavyhitters_amd import sketch as S
    seeds, x, kx, _ = extreme_case255(n_keys, n_nodes)
    rng = np.random.default_rng([n_keys, 9])
    words = np.stack([S.int_to_fe8(v) for v in EXTREME255])
    d = lambda *shape: [words[rng.integers(0, len(words), size=shape)] for _ in range(2)]   # noqa: E731
    xs = [np.array(x), words[rng.integers(0, len(words), size=(n_keys, n_nodes))]]
    kxs = [np.array(kx), words[rng.integers(0, len(words), size=(n_keys, n_nodes))]]
    wl = S.SketchWorkload255(np.array(seeds), xs, kxs, d(n_keys), d(n_keys), d(n_keys, 9), np.zeros(n_keys, bool))
    b = S.DeviceSketchBatch255(wl)
    S.sim_sketch_verify_fe255(kc, b)
    ok, outs = b.ok.cpu().numpy().astype(bool), b.out_shares.cpu().numpy().view(np.uint32)
    for i in range(n_keys):
        sk = [_py_sketch255(bytes(seeds[i]), _ints(wl.x[s][i]), _ints(wl.kx[s][i])) for s in range(2)]
        ok_e, o = py_verify(sk, [_ints(wl.mac[s][i])[0] for s in range(2)], [_ints(wl.mac2[s][i])[0] for s in range(2)],
                            [_ints(wl.triples[s][i]) for s in range(2)], P255)
        assert _ints(outs[0][i]) + _ints(outs[1][i]) == o and bool(ok[i]) == ok_e, f"key {i}"


@pytest.mark.gpu
@pytest.mark.parametrize("n_keys,n_nodes", [(9, 13), (70, 63)])
def test_gpu_fe255_representation_invariant(kc, n_keys, n_nodes):
    """metamorphic: p added to every limb vector of a canonical FieldElm workload (still below 2^256)
    changes no sketch, leaves ok == honest and both out shares unchanged"""
    from fuzzyheavyhitters_amd import sketch as S
    wl = S.sketch_workload255(n_keys, n_nodes, seed=7000 + n_keys, bad_fraction=0.2)

    def plus_p(a):
        return _fe8(np.array([v + P255 for v in _ints(a)], object).reshape(a.shape[:-1]))
    base = [S.sketch_at_fe255(kc, wl.seeds, wl.x[s], wl.kx[s]) for s in range(2)]
    b = S.DeviceSketchBatch255(wl)
    S.sim_sketch_verify_fe255(kc, b)
    ok, outs = b.ok.cpu().numpy().astype(bool), b.out_shares.cpu().numpy().copy()
    assert np.array_equal(ok, wl.honest)
    for name in ("x", "kx", "mac", "mac2", "triples"):
        setattr(wl, name, [plus_p(a) for a in getattr(wl, name)])
    assert (wl.x[0][..., 7] >= 0x7FFFFFFF).all()
    for s in range(2):
        assert np.array_equal(S.sketch_at_fe255(kc, wl.seeds, wl.x[s], wl.kx[s]), base[s]), f"server {s}"
    b2 = S.DeviceSketchBatch255(wl)
    S.sim_sketch_verify_fe255(kc, b2)
    assert np.array_equal(b2.ok.cpu().numpy().astype(bool), wl.honest)
    assert np.array_equal(b2.out_shares.cpu().numpy(), outs)


@pytest.mark.gpu
def test_gpu_fe255_fold_third_carry(kc):
    """operand pairs whose 512-bit product wraps past 2^256 a third time in fe255_fold16 (about
    2^-245 of random pairs): d e on server 1 (cor d_0 = a, e_0 = b) and d b on server 0 (cor d_0 = a,
    triple b_0 = b), with r_0 = 1 and every other word 0, give a b mod p = s"""
    from fuzzyheavyhitters_amd import sketch as S
    pairs = fold_pairs()
    n = len(pairs)
    assert n >= 32
    zero = np.zeros((n, 8), np.uint32)
    sk = np.zeros((n, 6, 8), np.uint32)
    sk[:, 3, 0] = 1                                     # rand1 = r_0 = 1
    a8, b8 = _fe8([p[0] for p in pairs]), _fe8([p[1] for p in pairs])
    exp = _fe8([p[2] for p in pairs])
    cor = np.zeros((n, 6, 8), np.uint32)
    cor[:, 0], cor[:, 3] = a8, b8
    got = S.mul_out_share_fe255(kc, 1, sk, zero, zero, np.zeros((n, 9, 8), np.uint32), cor)
    assert np.array_equal(got, exp), "server 1: d e"
    cor0 = np.zeros((n, 6, 8), np.uint32)
    cor0[:, 0] = a8
    tr = np.zeros((n, 9, 8), np.uint32)
    tr[:, 1] = b8
    got = S.mul_out_share_fe255(kc, 0, sk, zero, zero, tr, cor0)
    assert np.array_equal(got, exp), "server 0: d b"


@pytest.mark.gpu
def test_gpu_fe255_fold_third_carry_in_sketch(kc):
    """the same carry inside k_sketch_fe255: x_0 r with r node 0's draw"""
    from fuzzyheavyhitters_amd import sketch as S
    case = fold_sketch_case()
    assert case is not None
    seed, x0, r, s = case
    seeds = np.frombuffer(seed, np.uint8)[None].copy()
    x = _fe8([[x0]])
    kx = _fe8([[1]])
    got = S.sketch_at_fe255(kc, seeds, x, kx)
    assert _ints(got[0]) == _py_sketch255(seed, [x0], [1])
    assert _ints(got[0])[:3] == [s, s * r % P255, r]
