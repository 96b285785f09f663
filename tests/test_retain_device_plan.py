"""fhh_retain_plan_device (GPU): the survivor list k_keep_words / k_keep_scan / k_keep_emit make from a keep mask in
device memory, against fhh_retain_plan (the host arithmetic) and np.flatnonzero of the numpy AND — never against
itself. The ctx holds no keys: the call needs only its device and stream."""
import ctypes

import numpy as np
import pytest

from retain_cases import masks

pytestmark = pytest.mark.gpu

FHH_E_ARG = -1
SENTINEL = 0xDEAD
# The decomposition's units: a wave is one 64-client word; a block of the words and emit kernels is 256 lanes = 4
# words; one step of the single scan workgroup is 1024 words = 65 536 clients.
#   1, 63, 64, 65, 130          below, at and above one word; three words
#   257, 321                    a second block of the words / emit kernels holding one client / one word and a client
#   65 473 = 1023 * 64 + 1      the scan step's last word holds one client
#   65 536                      exactly one full scan step
#   65 537                      a second scan step of one word holding one client (the carry is used)
#   65 601 = 65 536 + 64 + 1    a second scan step of a full word and a partial one
SIZES = (1, 63, 64, 65, 130, 257, 321, 65473, 65536, 65537, 65601)
BIG = 200_001   # the random mask only: 4 scan steps, the last partial


@pytest.fixture(scope="module")
def kc(fhh):
    c = fhh.KeyCollection(16, 1)
    yield c
    c.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def plan_dev(kc, ptr_, n, n_rows=1, row_stride=0, want_n=True, want_src=True, cap=None):
    """(rc, message, n_kept, src) of fhh_retain_plan_device; outputs pre-filled with a sentinel."""
    import torch
    from fuzzyheavyhitters_amd._lib import lib, ptr, u32p
    torch.cuda.synchronize()
    nk = ctypes.c_uint64(SENTINEL)
    src = np.full(max(n if cap is None else cap, 1), SENTINEL, np.uint32)
    rc = lib().fhh_retain_plan_device(kc.handle, ctypes.c_void_p(ptr_), n, n_rows, row_stride,
                                      ctypes.byref(nk) if want_n else None, ptr(src, u32p) if want_src else None)
    msg = (lib().fhh_last_error(kc.handle) or b"").decode() if rc else ""
    return rc, msg, nk.value, src


@pytest.mark.parametrize("n", SIZES)
def test_plan_device_matches_host_plan(fhh, kc, n):
    """Every mask of retain_cases.masks(n) at the sizes of SIZES (chosen above: one partial unit beyond every unit of
    the words, scan and emit kernels): n' and src equal fhh_retain_plan's and np.flatnonzero, nothing is written
    beyond n', and the wrapper agrees."""
    for name, m in masks(n).items():
        t = _dev(m)
        rc, msg, nk, src = plan_dev(kc, t.data_ptr(), n)
        assert rc == 0, (name, msg)
        want = np.flatnonzero(m)
        hk, hsrc = fhh.KeyCollection.retain_plan(m)
        assert hk == len(want) and np.array_equal(hsrc, want), name
        assert nk == len(want), name
        assert np.array_equal(src[:nk], want), name
        assert (src[nk:] == SENTINEL).all(), f"{name}: wrote beyond n_kept"
        wk, wsrc = kc.retain_plan_device(t)
        assert wk == len(want) and np.array_equal(wsrc, want), name


def test_plan_device_large_random(fhh, kc):
    """200 001 clients, the random mask: several scan steps with a carry, the last one partial."""
    m = masks(BIG)["random"]
    nk, src = kc.retain_plan_device(_dev(m))
    hk, hsrc = fhh.KeyCollection.retain_plan(m)
    assert nk == hk == int(m.sum()) and np.array_equal(src, hsrc) and np.array_equal(src, np.flatnonzero(m))


@pytest.mark.parametrize("pad", [0xFF, 2])
@pytest.mark.parametrize("rows", [2, 3])
@pytest.mark.parametrize("n", [130, 65537])
def test_plan_device_rows(kc, n, rows, pad):
    """Rows of n bytes at a stride of n + 37: a client survives iff every row keeps it; the padding bytes (0xFF, 2:
    what would be refused inside a row) are neither read nor refused."""
    rng = np.random.default_rng(7 * n + rows)
    stride = n + 37
    buf = np.full((rows, stride), pad, np.uint8)
    buf[:, :n] = rng.random((rows, n)) < 0.7
    want = np.flatnonzero(buf[:, :n].min(axis=0))
    assert 0 < len(want) < min(int(buf[r, :n].sum()) for r in range(rows)), "the AND differs from every row"
    t = _dev(buf)
    rc, msg, nk, src = plan_dev(kc, t.data_ptr(), n, rows, stride)
    assert rc == 0, msg
    assert nk == len(want) and np.array_equal(src[:nk], want) and (src[nk:] == SENTINEL).all()
    wk, wsrc = kc.retain_plan_device(t[:, :n])           # a strided view: row stride n + 37, unit column stride
    assert wk == len(want) and np.array_equal(wsrc, want)
    wk, wsrc = kc.retain_plan_device(t.data_ptr(), n=n, n_rows=rows, row_stride=stride)
    assert wk == len(want) and np.array_equal(wsrc, want)


def test_plan_device_buffers(kc):
    m = np.array([1, 0, 1, 1, 0, 1], np.uint8)
    t = _dev(m)
    rc, _, nk, src = plan_dev(kc, t.data_ptr(), 6, cap=64)
    assert rc == 0 and nk == 4 and src[:4].tolist() == [0, 2, 3, 5] and (src[4:] == SENTINEL).all()
    rc, _, nk, src = plan_dev(kc, t.data_ptr(), 6, want_n=False)
    assert rc == 0 and nk == SENTINEL and src[:4].tolist() == [0, 2, 3, 5]
    rc, _, nk, src = plan_dev(kc, t.data_ptr(), 6, want_src=False)
    assert rc == 0 and nk == 4 and (src == SENTINEL).all()
    assert plan_dev(kc, t.data_ptr(), 6, want_n=False, want_src=False)[0] == 0
    # row_stride is ignored for one row
    rc, _, nk, src = plan_dev(kc, t.data_ptr(), 6, 1, 3)
    assert rc == 0 and nk == 4


def test_plan_device_refusals(fhh, kc):
    """Every refusal is FHH_E_ARG, carries a message and writes nothing; the library answers the next call."""
    n = 200
    good = np.ones(n, np.uint8)
    good[3] = 0
    two = np.ones((2, n), np.uint8)
    two[0, 5] = 0
    bad_first = two.copy()
    bad_first[0, 150] = 2
    bad_first[0, 70] = 3
    bad_first[1, 90] = 2          # the lowest index is 70, in row 0
    bad_last = two.copy()
    bad_last[1, 131] = 2
    bad_last[0, 140] = 2          # the lowest index is 131, in the last row
    disjoint = np.zeros((2, n), np.uint8)
    disjoint[0, ::2] = 1
    disjoint[1, 1::2] = 1         # each row keeps somebody, the AND nobody
    host = np.ones(n, np.uint8)
    tensors = {k: _dev(v) for k, v in dict(good=good, bad_first=bad_first, bad_last=bad_last, disjoint=disjoint,
                                           zeros=np.zeros(n, np.uint8)).items()}
    P = {k: v.data_ptr() for k, v in tensors.items()}
    cases = [("a byte in row 0", (P["bad_first"], n, 2, n), "keep byte 70 is 3, not 0 or 1"),
             ("a byte in the last row", (P["bad_last"], n, 2, n), "keep byte 131 is 2, not 0 or 1"),
             ("rows with a zero AND", (P["disjoint"], n, 2, n), "no survivor"),
             ("all zeros", (P["zeros"], n, 1, 0), "no survivor"),
             ("n_rows = 0", (P["good"], n, 0, n), "n_rows = 0"),
             ("row_stride < n", (P["bad_first"], n, 2, n - 1), "row_stride"),
             ("n = 0", (P["good"], 0, 1, 0), "n = 0"),
             ("NULL", (0, n, 1, 0), "NULL keep_dev"),
             ("a host buffer", (host.ctypes.data, n, 1, 0), "not device memory")]
    for what, args, text in cases:
        rc, msg, nk, src = plan_dev(kc, *args, cap=n)
        assert rc == FHH_E_ARG, (what, rc, msg)
        assert msg.startswith("retain_plan_device: ") and text in msg, (what, msg)
        assert nk == SENTINEL and (src == SENTINEL).all(), f"{what}: a refusal writes nothing"
        rc, msg, nk, src = plan_dev(kc, P["good"], n)
        assert rc == 0 and nk == n - 1, f"after {what}: {msg}"
    with pytest.raises(fhh.FhhError, match="no survivor"):
        kc.retain_plan_device(tensors["zeros"])
