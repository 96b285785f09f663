"""The tile-major table kernels' batched loads (csrc/fhh_gc.hip): the evaluator issues a tile's 8 row
messages before round 0's AES, the b = 2 garbler both bit tiles' 64 row words before the first XOR.

What a hoisted load can get wrong is its predicate: row 0 has no message (its index would wrap) and the
dead tests of a tail tile index past the buffer. n = 513 and 1025 leave a tail tile with one live test and
511 dead ones; n = 1 over several seeds reaches row 0 and rows 1..3; 511 / 512 are the tile's edges.
Everything is compared with the oracle bit for bit: there is no tolerance."""
import numpy as np
import pytest

from test_gc import (FE_P, _cases, _colour_s, _oracle_table_chain, _oracle_table_chain_ring32, _pair, _sig)
from kernel_usage import resource_usage

KEYS = ("ev_zero", "ev_active", "msgs", "gb_share", "ev_share")
SHAPES = [(1, 2), (511, 2), (512, 2), (513, 2), (1025, 2), (513, 1)]


def _rows(tr, bits):
    """the evaluator's row of every test: its active labels' colours"""
    return sum(((tr["ev_active"][:, k, 0] & 1).astype(int) << k) for k in range(bits))


def _check(oracle, kc, n, bits, ring32, seed):
    from fuzzyheavyhitters_amd import gc
    rng = np.random.default_rng(seed)
    g, e = _cases(rng, n, bits)
    seeds = rng.integers(0, 256, (128, 2, 16), dtype=np.uint8)
    s = _colour_s(rng)
    chain = _oracle_table_chain_ring32 if ring32 else _oracle_table_chain
    eq = (g == e).all(axis=1).astype(np.uint64)
    rows = set()
    for mask, ctr in ((0, 0), (1, 256)):
        tr = gc.table_cot(kc, g, e, mask, seeds, s, gate_base=13, ctr_off=ctr, ring32=ring32)
        etr = chain(oracle, g, e, mask, seeds, s, gate_base=13, ctr_off=ctr)
        for k in KEYS:
            assert np.array_equal(tr[k], etr[k].astype(tr[k].dtype)), (k, n, bits, ring32, mask)
        if ring32:
            diff = (tr["gb_share"] - tr["ev_share"]) & 0xFFFFFFFF
        else:
            diff = ((tr["gb_share"].astype(object) - tr["ev_share"].astype(object)) % FE_P).astype(np.uint64)
        assert np.array_equal(diff, eq), (n, bits, ring32, mask)
        rows |= set(_rows(etr, bits).tolist())
    return rows


@pytest.mark.gpu
@pytest.mark.parametrize("ring32", [False, True], ids=["fe", "ring32"])
@pytest.mark.parametrize("n,bits", SHAPES)
def test_gpu_table_tile_edges_bit_exact(oracle, n, bits, ring32):
    """msgs, both shares and gb - ev = eq at the tile's edges, both masks, FE and Z_2^32 shares."""
    import fuzzyheavyhitters_amd as fhh
    kc = fhh.KeyCollection(8, 1)
    rows = _check(oracle, kc, n, bits, ring32, seed=n * 13 + bits)
    if n >= 511:
        assert rows == set(range(1 << bits))   # every row, row 0 (no message) among them, is reached


@pytest.mark.gpu
@pytest.mark.parametrize("ring32", [False, True], ids=["fe", "ring32"])
def test_gpu_table_single_test_every_row(oracle, ring32):
    """n = 1 (one live test in the only tile, 511 dead ones) over seeds until the test has sat in row 0 and in
    each of rows 1..3: the message load's predicate, row != 0 and i < N, one combination at a time."""
    import fuzzyheavyhitters_amd as fhh
    kc = fhh.KeyCollection(8, 1)
    rows, seed = set(), 0
    while rows != {0, 1, 2, 3} and seed < 24:
        rows |= _check(oracle, kc, 1, 2, ring32, seed=5000 + seed)
        seed += 1
    assert rows == {0, 1, 2, 3}, rows


@pytest.mark.gpu
@pytest.mark.parametrize("ring32", [False, True], ids=["fe", "ring32"])
def test_gpu_crawl_513_clients_equals_plain(ring32):
    """One crawl of 513 clients (a tail tile of one live test per group) with the real table, growing from two
    children (chunks whose g_off is not 0): the plain crawl's counts, keep decisions and heavy hitters."""
    from fuzzyheavyhitters_amd import sim_crawl, workload
    wl = workload.zipf_workload(513, 32, 1, num_sites=20, seed=11)
    c0, c1 = _pair(wl.left, wl.right, wl.root_seeds)
    plain = sim_crawl(c0, c1, 0.01, mode="fe", prf_seed=4)
    got = sim_crawl(c0, c1, 0.01, mode="fe", prf_seed=4, gc="ot", init_capacity=2, table_ring32=ring32)
    assert _sig(got) == _sig(plain)
    assert len(got.final) > 0 and max(plain.level_children) > 2


def test_tile_major_table_kernels_fit_128_vgprs():
    """Every tile-major table kernel (b = 1..4, FE and Z_2^32 garblers, the evaluator) stays within 128 VGPRs
    with no spill and no scratch at 1024 threads: the batched loads must not cost the fourth wave per SIMD."""
    usage = resource_usage("fhh_gc.hip")
    names = [f"_ZN3fhh14k_gt_garble_tmILi{b}ELb{f}EEEvNS_6GcArgsE" for b in range(1, 5) for f in (0, 1)]
    names += [f"_ZN3fhh12k_gt_eval_tmILi{b}EEEvNS_6GcArgsE" for b in range(1, 5)]
    for name in names:
        assert name in usage, f"{name} not found"
        k = usage[name]
        assert int(k["VGPRs"]) <= 128, (name, k)
        assert k["VGPRs Spill"] == "0", (name, k)
        assert k["ScratchSize [bytes/lane]"] == "0", (name, k)
        assert int(k["Occupancy [waves/SIMD]"]) >= 4, (name, k)
