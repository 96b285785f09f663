"""The Z_2^32 garbled table at b = 3, 4 (the d = 2 tests): k_gt_garble<3|4, true> / k_gt_eval<3|4, true> on the
row-major labels and the per-child sums kernel k_ring32_child_sums (csrc/fhh_gc.hip) — their register budgets (CPU,
hipcc cross-compile), the oracle's table at these widths, and the kernels bit for bit against the oracle chain
through gc.table_cot(ring32=True) (fhh_gt_cot_ring32_host)."""
import ctypes
import itertools
import re

import numpy as np
import pytest

import party_model_ring32 as pr
from kernel_usage import resource_usage


def test_ring32_table_kernels_do_not_spill():
    """The Z_2^32 instantiations by their own mangled names: no scratch, no spilled VGPR and >= 4 waves per SIMD
    at 1024 threads, like their FE siblings k_gt_garble<3|4, false> / k_gt_eval<3|4, false>; the sums kernel
    compiles for gfx950 and needs neither scratch nor LDS."""
    u = resource_usage("fhh_gc.hip")
    names = [f"_ZN3fhh11k_gt_garbleILi{b}ELb1EEEvNS_6GcArgsE" for b in (3, 4)]
    names += [f"_ZN3fhh9k_gt_evalILi{b}ELb1EEEvNS_6GcArgsE" for b in (3, 4)]
    for name in names:
        assert name in u, f"{name} not found"
        k = u[name]
        assert k["ScratchSize [bytes/lane]"] == "0", (name, k)
        assert k["VGPRs Spill"] == "0", (name, k)
        assert int(k["Occupancy [waves/SIMD]"]) >= 4, (name, k)
        assert int(k["LDS Size [bytes/block]"]) == 131072, (name, k)   # the T-tables alone
    sums = "_ZN3fhh19k_ring32_child_sumsEPKjmmPKNS_7LoopCtlEmPmjj"
    assert sums in u, f"{sums} not found"
    assert u[sums]["ScratchSize [bytes/lane]"] == "0" and u[sums]["LDS Size [bytes/block]"] == "0", u[sums]
    # only b = 3, 4 have row-major kernels, FE or ring (b <= 2 stays on the tile-major ones)
    assert not any(re.search(r"k_gt_(garble|eval)ILi[12]E", n) for n in u)


@pytest.mark.parametrize("bits", [3, 4])
def test_oracle_ring32_table_wide_functional(oracle, bits):
    """The oracle's Z_2^32 table at b = 3, 4: gb - ev = eq (mod 2^32) for every test and both masks, with
    the first third of the tests equal and the rest random, which reaches all 2^b rows at n = 5000."""
    rng = np.random.default_rng(300 + bits)
    n = 5000
    g, e = pr.thirds_cases(rng, n, bits)
    seeds = rng.integers(0, 256, (128, 2, 16), dtype=np.uint8)
    s = rng.integers(0, 256, 16, dtype=np.uint8)
    s[0] |= 1
    eq = (g == e).all(axis=1)
    assert eq[:n // 3].all() and 0 < eq[n // 3:].sum() < n - n // 3
    for mask in (0, 1):
        tr = pr.table_chain(g, e, mask, seeds, s.tobytes(), gate_base=21)
        assert tr["msgs"].dtype == np.uint32 and tr["msgs"].shape == (n, (1 << bits) - 1)
        assert np.array_equal((tr["gb_share"] - tr["ev_share"]).astype(np.uint32), eq.astype(np.uint32))
        rows = sum(((tr["ev_active"][:, k, 0] & 1).astype(int) << k) for k in range(bits))
        assert len(set(rows.tolist())) == 1 << bits


GRID_STRIDE = "grid-stride"


def _grid_stride_n():
    """The smallest batch that sends both row-major kernels (at most 8 workgroups of 1024 lanes per CU; the
    garbler one test per lane and pass, the evaluator two) round their loops a second time, with a partial
    last workgroup."""
    from fuzzyheavyhitters_amd._lib import lib
    cus, name = ctypes.c_int(), ctypes.create_string_buffer(64)
    assert lib().fhh_device_info(0, name, 64, ctypes.byref(cus)) == 0 and cus.value > 0
    return 8 * cus.value * 1024 * 2 + 1061


@pytest.mark.gpu
@pytest.mark.parametrize("n,bits", [(1, 4), (65, 3), (777, 3), (4097, 4), (GRID_STRIDE, 3)])
def test_gpu_ring32_table_wide_bit_exact(oracle, n, bits):
    """fhh_gt_cot_ring32_host at b = 3, 4 (labels OT + k_gt_garble<b, true> + k_gt_eval<b, true>) = the oracle chain bit
    for bit: zero and active labels, every 4-B message, both parties' values (zero-extended); gb - ev = eq mod
    2^32. Masks 0 and 1, ctr_off 0 and 256; the grid-stride case runs mask 1 at ctr_off 256 only."""
    import fuzzyheavyhitters_amd as fhh
    from fuzzyheavyhitters_amd import gc
    big = n == GRID_STRIDE
    if big:
        n = _grid_stride_n()
    rng = np.random.default_rng(n * 13 + bits)
    g, e = pr.thirds_cases(rng, n, bits)
    seeds = rng.integers(0, 256, (128, 2, 16), dtype=np.uint8)
    s = rng.integers(0, 256, 16, dtype=np.uint8)
    s[0] |= 1
    s = s.tobytes()
    kc = fhh.KeyCollection(8, 1)
    eq = (g == e).all(axis=1).astype(np.uint64)
    for mask, ctr in (((1, 256),) if big else itertools.product((0, 1), (0, 256))):
        tr = gc.table_cot(kc, g, e, mask, seeds, s, gate_base=13, ctr_off=ctr, ring32=True)
        etr = pr.table_chain(g, e, mask, seeds, s, gate_base=13, ctr_off=ctr)
        for k in ("ev_zero", "ev_active", "msgs", "gb_share", "ev_share"):
            assert np.array_equal(tr[k], etr[k].astype(tr[k].dtype)), (k, mask, ctr)
        assert int(tr["msgs"].max()) < 1 << 32 and int(tr["gb_share"].max()) < 1 << 32
        assert np.array_equal((tr["gb_share"] - tr["ev_share"]) & 0xFFFFFFFF, eq), (mask, ctr)
