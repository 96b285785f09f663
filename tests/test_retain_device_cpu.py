"""fhh_retain_clients_device without a GPU: the compiler's resource report of the survivor-list kernels (hipcc
cross-compile for gfx950) and the new symbols of the built library."""
import ctypes

from kernel_usage import resource_usage


def test_keep_kernel_resources():
    """k_keep_words (a byte per row and a ballot), k_keep_scan (a wave scan by shuffles, 16 wave totals in LDS) and
    k_keep_emit (one word, one store) each appear once and hold a few registers per lane: no scratch, no spilled
    VGPR. They do not disturb the names the gather kernels are found by."""
    u = resource_usage("fhh_retain_mask.hip")
    for name in ("k_keep_words", "k_keep_scan", "k_keep_emit"):
        hits = [k for k in u if name in k]
        assert len(hits) == 1, sorted(u)
        k = u[hits[0]]
        assert k["ScratchSize [bytes/lane]"] == "0", k
        assert k["VGPRs Spill"] == "0", k
    assert len(u) == 3, sorted(u)
    assert not any("k_retain_cols" in k or "k_retain_planes" in k for k in u)
    g = resource_usage("fhh_retain.hip")
    for name in ("k_retain_cols", "k_retain_planes"):
        assert len([k for k in g if name in k]) == 1, sorted(g)


def test_symbols_and_signatures(fhh):
    """Both entry points (and the diagnostics timing entry) are in the built libfhh.so with the signatures
    include/fhh.h declares; no device call."""
    from fuzzyheavyhitters_amd._lib import LIB_PATH, u32p, u64p
    raw = ctypes.CDLL(LIB_PATH)
    for name in ("fhh_retain_clients_device", "fhh_retain_plan_device", "fhh_retain_mask_timing"):
        assert hasattr(raw, name), name
    L = fhh.lib()
    vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    assert L.fhh_retain_clients_device.argtypes == [vp, vp, u64, u32, u64, u64p]
    assert L.fhh_retain_plan_device.argtypes == [vp, vp, u64, u32, u64, u64p, u32p]
    assert L.fhh_retain_clients_device.restype is ctypes.c_int and L.fhh_retain_plan_device.restype is ctypes.c_int
    # a NULL ctx is refused before anything else
    assert L.fhh_retain_clients_device(None, None, 1, 1, 0, None) == -1
    assert L.fhh_retain_plan_device(None, None, 1, 1, 0, None, None) == -1
    assert hasattr(fhh.KeyCollection, "retain_clients_device") and hasattr(fhh.KeyCollection, "retain_plan_device")
    from fuzzyheavyhitters_amd import sketch
    assert hasattr(sketch, "apply_sketch_results_device")
