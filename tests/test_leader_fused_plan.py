"""fhh_leader_requests_* (CPU): the symbols and their ABI, fhh_leader_requests_plan against Python integers, the
refusals that need no device, add_fuzzy_keys' route argument, and the compiler's resource report of the fused
kernel's two forms against the occupancy DESIGN.md §5.8 claims for it."""
import ctypes
import os
import re

import numpy as np
import pytest

import ball_cases as bc
import leader_fused_cases as lf
from kernel_usage import resource_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FHH_E_ARG = -1
NAMES = ("fhh_leader_requests_plan", "fhh_leader_requests_ball_device", "fhh_leader_requests_ball")


def test_symbols_and_abi(fhh):
    """The three entry points are exported by the library, bound with the header's argument counts, and declared
    in include/fhh.h beside fhh_gen_keys_ball; the Python names are exported."""
    lib = fhh.lib()
    header = open(os.path.join(ROOT, "include", "fhh.h")).read()
    for name in NAMES:
        assert name in fhh._lib.EXPORTS
        f = getattr(lib, name)
        m = re.search(r"^int " + name + r"\(([^;]*?)\);", header, re.M | re.S)
        assert m, f"{name} is not declared in include/fhh.h"
        assert len(f.argtypes) == len(m.group(1).split(",")), name
        assert f.restype is ctypes.c_int
    assert header.index("int fhh_gen_keys_ball(") < header.index("int fhh_leader_requests_ball(")
    for name in ("leader_requests_ball", "leader_requests_plan", "add_fuzzy_keys"):
        assert name in fhh.__all__ and callable(getattr(fhh, name))
    assert "fhh_leader_requests.hip" in fhh._lib.SOURCES


@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_plan_equals_the_integer_model(fhh, d):
    for n in (1, 63, 64, 65, 130, 4096 * 8 * 64 // (2 * d), 4096 * 8 * 64 // (2 * d) + 1, 262_144, 262_145, 10 ** 6,
              2 ** 33 + 5):
        for L in (16, 32, 512):
            assert fhh.leader_requests_plan(d, L, n) == lf.plan_model(d, n), (d, L, n)
    # the launch cap is k_keygen's: the same second, partial trip at the same population
    items, waves, trips = fhh.leader_requests_plan(4, 32, 262_145)
    assert (items, waves, trips) == (32_776, 32_768, 2) and fhh.leader_requests_plan(4, 32, 262_144)[2] == 1


def test_plan_outputs_may_be_null_and_bad_shapes_are_refused(fhh):
    lib = fhh.lib()
    trips = ctypes.c_uint64()
    assert lib.fhh_leader_requests_plan(2, 16, 1000, None, None, ctypes.byref(trips)) == 0 and trips.value == 1
    assert lib.fhh_leader_requests_plan(2, 16, 1000, None, None, None) == 0
    for d, L, n in ((0, 32, 10), (5, 32, 10), (1, 0, 10), (1, 32, 0)):
        trips.value = 77
        assert lib.fhh_leader_requests_plan(d, L, n, None, None, ctypes.byref(trips)) == FHH_E_ARG
        assert trips.value == 77 and b"leader_requests_plan" in lib.fhh_last_error(None)
        with pytest.raises(fhh.FhhError):
            fhh.leader_requests_plan(d, L, n)


def test_null_ctx_is_refused_with_nothing_written(fhh):
    """The refusal that needs no device: a NULL ctx, both forms; no pointer handed out, `out` keeps its sentinel."""
    lib = fhh.lib()
    src = fhh._lib.FhhBallSrc()
    pts = np.zeros((4, 1, 5), np.uint8)
    src.points = pts.ctypes.data
    out0, out1 = (np.full(64, lf.SENTINEL, np.uint8) for _ in range(2))
    ln = ctypes.c_uint64(123)
    assert lib.fhh_leader_requests_ball(None, 4, ctypes.byref(src), 0, fhh._lib.ptr(out0), fhh._lib.ptr(out1), 64,
                                        ctypes.byref(ln)) == FHH_E_ARG
    assert (out0 == lf.SENTINEL).all() and (out1 == lf.SENTINEL).all() and ln.value == 123
    p0, p1, nb = ctypes.c_void_p(5), ctypes.c_void_p(6), ctypes.c_uint64(7)
    assert lib.fhh_leader_requests_ball_device(None, 4, ctypes.byref(src), 0, ctypes.byref(p0), ctypes.byref(p1),
                                               ctypes.byref(nb)) == FHH_E_ARG
    assert (p0.value, p1.value, nb.value) == (5, 6, 7)


def test_fused_route_argument_checks(fhh):
    """Refused before any ctx is made (no GPU): a chunk that would cut a request in two, a bad chunk, an unknown
    route. The default route stays "collections"."""
    import inspect
    pts = np.zeros((10, 1, 5), np.uint8)
    for batch, chunk in ((7, 100), (100, 150), (3, 10)):
        with pytest.raises(fhh.FhhError, match="multiple"):
            next(fhh.add_fuzzy_keys(pts, 1, n_dims=1, data_len=40, seed=bc.SEED, batch=batch, chunk=chunk, route="fused"))
    with pytest.raises(fhh.FhhError):
        next(fhh.add_fuzzy_keys(pts, 1, n_dims=1, data_len=40, seed=bc.SEED, batch=1, chunk=0, route="fused"))
    with pytest.raises(fhh.FhhError, match="route"):
        next(fhh.add_fuzzy_keys(pts, 1, n_dims=1, data_len=40, seed=bc.SEED, route="both"))
    assert inspect.signature(fhh.add_fuzzy_keys).parameters["route"].default == "collections"


def test_fused_kernel_resources():
    """Both point forms: no scratch, no spilled register, and what DESIGN.md §5.8 claims — the 64 KiB T-table as
    the only LDS (two workgroups per CU) and at most 128 VGPRs, so the two 512-thread workgroups' 4 waves per SIMD
    fit the register file."""
    usage = resource_usage("fhh_leader_requests.hip")
    kernels = {k: v for k, v in usage.items() if "k_leader_requests" in k}
    assert len(kernels) == 2, sorted(usage)
    for name, u in kernels.items():
        assert u["ScratchSize [bytes/lane]"] == "0", name
        assert u["VGPRs Spill"] == "0", name
        assert int(u["LDS Size [bytes/block]"]) == 65536, name
        assert int(u["VGPRs"]) + int(u.get("AGPRs", "0")) <= 128, name
        assert int(u["Occupancy [waves/SIMD]"]) >= 4, name
