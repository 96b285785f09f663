"""The garbled table of b = 3, 4 bits (d = 2) on the labels OT's tile-major matrices: k_gt_garble_tm<3|4> /
k_gt_eval_tm<3|4> read 512-test windows that start at any even word of a tile (Npad = 64 nw, any nw), with the
per-child sums fused; fhh_set_table_row_major switches a ctx back to k_ot_rows_out + the row-major kernels (the
A/B partner: same outputs). The party ABI keeps the row-major labels at b = 3, 4. Register budget, the host
self-test of the window addressing and the switch's ABI (CPU); on the GPU the single-launch chain against the
oracle and the level loop against the plain crawl."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import test_gc as tg
from kernel_usage import resource_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FE_P = tg.FE_P


# ---- CPU: register budget, the switch ------------------------------------------------------------------
def test_wide_tile_major_table_kernels_fit_their_budget():
    """1024 threads and 160 KiB of LDS (tables + the 2-KiB stages) leave 128 VGPRs per lane and no LDS on the
    CU: no scratch, no spilled VGPR, 4 waves per SIMD, for the FE and Z_2^32 garblers and the evaluator."""
    usage = resource_usage("fhh_gc.hip")
    names = [f"_ZN3fhh14k_gt_garble_tmILi{b}ELb{r}EEEvNS_6GcArgsE" for b in (3, 4) for r in (0, 1)]
    names += [f"_ZN3fhh12k_gt_eval_tmILi{b}EEEvNS_6GcArgsE" for b in (3, 4)]
    for name in names:
        assert name in usage, f"{name} not found"
        k = usage[name]
        assert k["ScratchSize [bytes/lane]"] == "0", (name, k)
        assert k["VGPRs Spill"] == "0", (name, k)
        assert int(k["Occupancy [waves/SIMD]"]) >= 4, (name, k)
        assert int(k["LDS Size [bytes/block]"]) == 163840, (name, k)


def test_gt_window_host(tmp_path):
    """csrc/gt_window.h on the host (tests/host/gt_window_host_test.cpp): window start word -> (tile, word), the
    live-word rule, every read inside the bit's own OTs, and the row-domain sigma^k fold (shift, wrap rows,
    reduction targets) against the per-label Horner rule, for nw = 1 .. 17 and 42 at b = 3, 4."""
    if not shutil.which("hipcc"):
        pytest.skip("hipcc not available")
    exe = tmp_path / "gt_window_host"
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-O1", "-std=c++17",
                    os.path.join(ROOT, "tests", "host", "gt_window_host_test.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "OK", out.stdout + out.stderr


def test_gt_plan_host(tmp_path):
    """csrc/gt_plan.h on the host (tests/host/gt_plan_host_test.cpp): the form of the equality test for every
    caller, GC form, level kind, d = 1 .. 4, ring request, table_row_major and nw = 1 .. 16 384 against the literal
    table of what the level loop, gt_cot_host and party_begin decided before the header existed; the chunk-sizing
    estimates 402 and 320 that the chunked loop tests use; the party ABI row-major and unfused at b = 3, 4; no
    row-major table at b <= 2, where no row-major kernel exists."""
    if not shutil.which("hipcc"):
        pytest.skip("hipcc not available")
    exe = tmp_path / "gt_plan_host"
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-O1", "-std=c++17", "-Wall",
                    os.path.join(ROOT, "tests", "host", "gt_plan_host_test.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("OK "), out.stdout + out.stderr


def test_set_table_row_major_abi():
    """The switch exists, refuses a NULL ctx and values other than 0 / 1."""
    from fuzzyheavyhitters_amd._lib import lib
    f = lib().fhh_set_table_row_major
    assert f(None, 1) != 0
    import torch
    if not torch.cuda.is_available():
        return
    import fuzzyheavyhitters_amd as fhh
    kc = fhh.KeyCollection(8, 2)
    assert f(kc.handle, 2) != 0 and f(kc.handle, -1) != 0
    kc.set_table_row_major(True)
    kc.set_table_row_major(False)


# ---- GPU: one launch against the oracle chain ----------------------------------------------------------
GRID_STRIDE = "grid-stride"


def _grid_stride_n():
    """16 windows per CU + 2 at b = 4: the workgroups go round their grid-stride loop again; the last window
    holds 37 live tests."""
    from fuzzyheavyhitters_amd._lib import lib
    cus, name = ctypes.c_int(), ctypes.create_string_buffer(64)
    assert lib().fhh_device_info(0, name, 64, ctypes.byref(cus)) == 0 and cus.value > 0
    return 512 * (16 * cus.value + 1) + 37


@pytest.mark.gpu
@pytest.mark.parametrize("row_major", [False, True], ids=["tile-major", "row-major"])
@pytest.mark.parametrize("n,bits", [(1, 4), (65, 3), (200, 4), (777, 3), (2650, 3), (4097, 4), (GRID_STRIDE, 4)])
def test_gpu_wide_table_bit_exact(oracle, n, bits, row_major):
    """gc.table_cot, FE and Z_2^32, = the oracle chain bit for bit: labels, every message, both shares.
    (1, 4): four windows inside one tile at words 0, 2, 4, 6; (200, 4): bits 1 and 3 start mid-tile; (777, 3):
    windows straddle two tiles, the second holds 265 live tests; (2650, 3): m = 8064, the last window runs past
    the padded matrix; (4097, 4): nine windows, the last with one live test."""
    import fuzzyheavyhitters_amd as fhh
    from protocol_grid_cases import check_table_bit_exact
    big = n == GRID_STRIDE
    if big:
        n = _grid_stride_n()
    kc = fhh.KeyCollection(8, 1)
    kc.set_table_row_major(row_major)
    check_table_bit_exact(kc, oracle, n, bits, big=big)


# ---- GPU: the level loop -----------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("devices", [None, [0, 0]], ids=["one-shard", "two-shards"])
@pytest.mark.parametrize("ss_k", [1, 2])
def test_gpu_loop_d2_table_layouts_equal_plain(monkeypatch, ss_k, devices):
    """sim_crawl(gc="ot") at d = 2 with 3 000 clients (nw = 47, not a multiple of 8), FE and Z_2^32 table shares
    (on the row-major labels: k_gt_garble<3|4, true> / k_gt_eval<3|4, true> + k_ring32_child_sums), whole levels and
    several chunks per level: every level's counts and the final (path, value) set equal the plain FE-mode
    crawl's, in both layouts."""
    import fuzzyheavyhitters_amd as fhh
    from fuzzyheavyhitters_amd import sim_crawl, workload
    wl = workload.zipf_workload(3000, 32, 2, num_sites=12, seed=5)
    wl.left, wl.right = wl.left[:, :, :8].copy(), wl.right[:, :, :8].copy()
    c0 = fhh.KeyCollection(8, 2, devices=devices)
    c1 = fhh.KeyCollection(8, 2, devices=devices)
    fhh.gen_keys_pair(c0, c1, wl.left, wl.right, wl.root_seeds)
    plain = tg._sig(sim_crawl(c0, c1, 0.02, mode="fe", prf_seed=9))
    for chunk_bytes in (None, 3 * 3008 * 320):   # whole levels; 3 children per chunk
        if chunk_bytes:
            monkeypatch.setenv("FHH_GC_CHUNK_BYTES", str(chunk_bytes))
        for ring in (False, True):
            for row_major in (False, True):
                c0.set_table_row_major(row_major)
                got = sim_crawl(c0, c1, 0.02, mode="fe", prf_seed=9, gc="ot", init_capacity=2, ot_ss_k=ss_k,
                                table_ring32=ring)
                assert tg._sig(got) == plain, (chunk_bytes, ring, row_major)
                assert len(got.final) > 0
    c0.set_table_row_major(False)
