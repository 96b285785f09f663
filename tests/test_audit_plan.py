"""The audit's launch arithmetic and interface without a GPU (CPU): the new symbols, fhh_audit_plan against Python
integers (audit_cases.plan) with every argument refusal, the compiler's resource report of k_audit_keys, and the
argument checks of leader.add_fuzzy_keys' audit option."""
import ctypes
import re

import numpy as np
import pytest

import audit_cases as ac
from kernel_usage import resource_usage

FHH_E_ARG = -1
NEW_SYMBOLS = ("fhh_audit_keys_ball", "fhh_audit_keys_ball_device", "fhh_audit_probes", "fhh_audit_plan",
               "fhh_audit_timing", "fhh_audit_seed_check")


def test_the_new_symbols_exist():
    import fuzzyheavyhitters_amd as fhh
    from fuzzyheavyhitters_amd import _lib
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(fhh.lib(), name), name
    for name in ("audit_plan", "audit_probes", "KeyAuditError"):
        assert hasattr(fhh, name), name
    assert hasattr(fhh.KeyCollection, "audit_keys_ball") and hasattr(fhh.KeyCollection, "audit_keys_ball_device")
    assert ctypes.sizeof(_lib.FhhAuditReport) == 48
    assert issubclass(fhh.KeyAuditError, fhh.FhhError)


@pytest.mark.parametrize("grid", [1, 2, 3, 256, 1024, 2 ** 20])
def test_plan_equals_python_integers(grid):
    import fuzzyheavyhitters_amd as fhh
    for d in (1, 2, 3, 4):
        for L in (16, 32, 100, 512):
            for n in (1, 63, 64, 65, 130, 1100, 2100, 100_000, 262_145, 1_000_000, 2 ** 32 - 1):
                got = fhh.audit_plan(d, L, n, grid)
                assert got == ac.plan(d, L, n, grid), (d, L, n, grid)
                assert got["last_trip_items"] >= 1 and got["waves"] * (got["trips"] - 1) < got["items"]
                assert got["n_checks"] == n * 2 * d * 5 * L and got["aes_blocks"] == 2 * got["n_checks"]


def test_plan_of_the_cases_the_gpu_tests_name():
    p = ac.plan(4, 32, 262_145, 2 ** 20)
    assert p["items"] == 32_776 and p["items"] == 8 * 4097
    for grid in (1, 2, 3):
        for n in (1100, 2100):
            p = ac.plan(2, 32, n, grid)
            assert p["trips"] >= 2 and p["last_trip_items"] < p["waves"], (grid, n, p)


def test_plan_refusals_and_null_outputs():
    import fuzzyheavyhitters_amd as fhh
    lib = fhh.lib()
    v = [ctypes.c_uint64(99) for _ in range(6)]
    refs = [ctypes.byref(x) for x in v]
    for d, L, n, grid in ((0, 32, 10, 4), (5, 32, 10, 4), (1, 0, 10, 4), (1, 32, 0, 4), (1, 32, 10, 0)):
        assert lib.fhh_audit_plan(d, L, n, grid, *refs) == FHH_E_ARG, (d, L, n, grid)
        assert [x.value for x in v] == [99] * 6
    with pytest.raises(fhh.FhhError, match="audit_plan"):
        fhh.audit_plan(1, 32, 0, 4)
    assert lib.fhh_audit_plan(2, 40, 130, 7, None, None, None, None, None, None) == 0
    assert lib.fhh_audit_plan(2, 40, 130, 7, None, refs[1], None, None, None, refs[5]) == 0
    assert v[1].value == ac.plan(2, 40, 130, 7)["waves"] and v[5].value == 130 * 4 * 5 * 40 and v[0].value == 99


def test_compiler_report_of_the_audit_kernel():
    """Both point forms of k_audit_keys: no scratch, no VGPR spill, at most 128 VGPRs (4 waves per SIMD of a
    1024-thread workgroup), and k_eval_paths' LDS size, the 128 KiB of T-tables."""
    audit = {k: v for k, v in resource_usage("fhh_audit.hip").items() if re.search(r"\d+k_audit_keys", k)}
    paths = [v for k, v in resource_usage("fhh_kernels.hip").items() if re.search(r"\d+k_eval_paths", k)]
    assert len(audit) == 2 and len(paths) == 1
    for name, u in audit.items():
        assert int(u["ScratchSize [bytes/lane]"]) == 0, name
        assert int(u["VGPRs Spill"]) == 0, name
        assert int(u["VGPRs"]) + int(u.get("AGPRs", 0)) <= 128, name
        assert u["LDS Size [bytes/block]"] == paths[0]["LDS Size [bytes/block]"] == "131072", name
        assert int(u["Occupancy [waves/SIMD]"]) == 4, name


def test_leader_audit_option_argument_checks():
    """The checks come before any device call: the generator's first step raises."""
    from fuzzyheavyhitters_amd import FhhError, leader
    pts = np.zeros((10, 1, 5), np.uint8)
    kw = dict(n_dims=1, data_len=40, seed=bytes(32), batch=5, chunk=10)
    with pytest.raises(ValueError, match="fused"):
        next(leader.add_fuzzy_keys(pts, 1, route="fused", audit=True, **kw))
    with pytest.raises(TypeError, match="audit"):
        next(leader.add_fuzzy_keys(pts, 1, audit="yes", **kw))
    with pytest.raises(TypeError, match="audit"):
        next(leader.add_fuzzy_keys(pts, 1, audit=1, **kw))
    with pytest.raises(FhhError, match="route"):
        next(leader.add_fuzzy_keys(pts, 1, route="nowhere", audit=True, **kw))
    import inspect
    assert inspect.signature(leader.add_fuzzy_keys).parameters["audit"].default is False
