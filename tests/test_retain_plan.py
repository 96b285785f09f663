"""fhh_retain_plan (CPU, host arithmetic): the survivor list fhh_retain_clients uploads for its gather kernels,
against np.flatnonzero; its refusals; and the compiler's resource report of the two kernels (hipcc cross-compile
for gfx950)."""
import ctypes

import numpy as np
import pytest

from kernel_usage import resource_usage
from retain_cases import masks

FHH_E_ARG = -1
SIZES = (1, 63, 64, 65, 130)


def plan(keep, n=None, null_keep=False, want_n=True, want_src=True):
    """(rc, n_kept, src) of fhh_retain_plan on a uint8 mask; outputs pre-filled with a sentinel."""
    from fuzzyheavyhitters_amd._lib import lib, ptr, u32p
    k = np.ascontiguousarray(keep, np.uint8)
    n = k.size if n is None else n
    nk = ctypes.c_uint64(0xDEAD)
    src = np.full(max(k.size, 1), 0xDEAD, np.uint32)
    rc = lib().fhh_retain_plan(None if null_keep else ptr(k), n, ctypes.byref(nk) if want_n else None,
                               ptr(src, u32p) if want_src else None)
    return rc, nk.value, src


@pytest.mark.parametrize("n", SIZES)
def test_plan_matches_flatnonzero(fhh, n):
    for name, m in masks(n).items():
        rc, nk, src = plan(m)
        assert rc == 0, (name, fhh.lib().fhh_last_error(None))
        want = np.flatnonzero(m)
        assert nk == len(want), name
        assert np.array_equal(src[:nk], want), name
        assert (src[nk:] == 0xDEAD).all(), f"{name}: wrote beyond n_kept"
        wk, wsrc = fhh.KeyCollection.retain_plan(m)
        assert wk == len(want) and np.array_equal(wsrc, want), name
        wk, wsrc = fhh.KeyCollection.retain_plan(m.astype(bool))
        assert wk == len(want) and np.array_equal(wsrc, want), name


def test_masks_cover_what_they_should():
    m = masks(130)
    assert (m["word dropped"].reshape(-1)[64:128] == 0).all() and m["word dropped"].sum() == 66
    assert m["first word dropped"].sum() == 66 and 0 < m["random"].sum() < 130
    assert set(masks(1)) == {"all ones", "one survivor 0", "random"}


def test_plan_refusals(fhh):
    L = fhh.lib()
    good = np.ones(5, np.uint8)
    assert plan(good)[0] == 0
    for what, kw, text in (("NULL keep", dict(keep=good, null_keep=True), b"NULL keep"),
                           ("n = 0", dict(keep=good, n=0), b"n = 0"),
                           ("a byte 2", dict(keep=np.array([1, 0, 2, 1, 1], np.uint8)), b"not 0 or 1"),
                           ("all zeros", dict(keep=np.zeros(5, np.uint8)), b"no survivor")):
        rc, nk, src = plan(**kw)
        assert rc == FHH_E_ARG, what
        msg = L.fhh_last_error(None)
        assert msg.startswith(b"retain_plan: ") and text in msg, (what, msg)
        assert nk == 0xDEAD and (src == 0xDEAD).all(), f"{what}: a refusal writes nothing"
    with pytest.raises(fhh.FhhError):
        fhh.KeyCollection.retain_plan(np.zeros(3, np.uint8))


def test_plan_null_outputs(fhh):
    m = np.array([1, 0, 1, 1, 0, 1], np.uint8)
    rc, nk, src = plan(m, want_n=False)
    assert rc == 0 and nk == 0xDEAD and src[:4].tolist() == [0, 2, 3, 5]
    rc, nk, src = plan(m, want_src=False)
    assert rc == 0 and nk == 4 and (src == 0xDEAD).all()
    assert plan(m, want_n=False, want_src=False)[0] == 0


def test_wrapper_refuses_masks_a_cast_would_change(fhh):
    """KeyCollection.retain_plan / retain_clients share one conversion of the mask: bools and integers 0/1 pass, a
    byte 2 reaches the library (which refuses it), and floats or integers outside a byte are refused instead of
    being cast to 0."""
    plan_ = fhh.KeyCollection.retain_plan
    assert plan_([True, False, True])[0] == 2 and plan_(np.array([1, 0, 1], np.int64))[0] == 2
    for bad in (np.array([0.5, 1.0]), np.array([256, 1]), np.array([-1, 1]), np.array(["1", "0"])):
        with pytest.raises(fhh.FhhError, match="keep mask"):
            plan_(bad)
    with pytest.raises(fhh.FhhError, match="not 0 or 1"):
        plan_(np.array([1, 2], np.int32))


def test_retain_kernel_resources():
    """Both gather kernels hold a few registers per lane (one column's 4 rows in flight; one source word):
    no scratch and no spilled VGPR."""
    u = resource_usage("fhh_retain.hip")
    for name in ("k_retain_cols", "k_retain_planes"):
        hits = [k for k in u if name in k]
        assert len(hits) == 1, sorted(u)
        k = u[hits[0]]
        assert k["ScratchSize [bytes/lane]"] == "0", k
        assert k["VGPRs Spill"] == "0", k
