"""fhh_join_plan and the other host-side parts of fhh_join_clients_bincode (CPU, no GPU): the walk's launch plan
against Python integers (join_cases.plan), its refusals, the NULL-ctx refusals, two_party_crawl's checks of
`joins=`, and the compiler's resource report of k_join_paths, the join form of k_eval_paths' body."""
import ctypes
import re

import numpy as np
import pytest

import join_cases as jc
from kernel_usage import resource_usage

FHH_E_ARG = -1
NAMES = ("first_word", "first_mask", "words", "new_nw", "items", "waves", "trips", "last_trip_items", "aes_blocks")
US = (1, 3, 4, 5)
GRIDS = (1, 2, 3, 256)
PLAN_PAIRS = jc.PAIRS + [(2 ** 32 - 3, 1)]


def test_symbols_exist(fhh):
    from fuzzyheavyhitters_amd import _lib
    L = fhh.lib()
    for name in ("fhh_join_clients_bincode", "fhh_join_plan", "fhh_join_timing"):
        assert name in _lib.EXPORTS and hasattr(L, name), name
    for name in ("join_clients_bincode", "join_plan", "join_timing"):
        assert hasattr(fhh.KeyCollection, name), name


@pytest.mark.parametrize("n,m", PLAN_PAIRS, ids=[f"{n}+{m}" for n, m in PLAN_PAIRS])
def test_plan_equals_python_integers(fhh, n, m):
    for d in (1, 2, 3, 4):
        for rot in range(4):
            U = [US[(rot + j) % 4] for j in range(d)]
            for grid in GRIDS:
                for depth in (0, 1, 33, 511):
                    want = jc.plan(d, depth, n, m, U, grid)
                    assert fhh.KeyCollection.join_plan(d, depth, n, m, U, grid) == want, (d, U, grid, depth)
                    assert want["words"] >= 1 and want["trips"] >= 1 and 1 <= want["last_trip_items"] <= want["waves"]


def test_plan_shapes_of_the_named_pairs():
    """What each pair of join_cases.PAIRS is there for, on Python integers."""
    p = {nm: jc.plan(1, 3, *nm, [1], 256) for nm in jc.PAIRS}
    full = (1 << 64) - 1
    assert [p[nm]["new_nw"] - (nm[0] + 63) // 64 for nm in jc.PAIRS] == [0, 0, 1, 0, 2, 1, 0]    # the words added
    assert p[(64, 1)]["first_mask"] == full and p[(128, 64)]["first_mask"] == full                   # a new word
    assert p[(63, 1)]["first_mask"] == 1 << 63 and p[(1, 1)]["first_mask"] == full - 1
    assert p[(65, 63)]["words"] == 1 and p[(70, 130)]["words"] == 3 and p[(130, 1)]["first_word"] == 2


def test_plan_refusals(fhh):
    lib = fhh.lib()
    from fuzzyheavyhitters_amd._lib import ptr, u32p
    v = [ctypes.c_uint64(99) for _ in NAMES]
    refs = [ctypes.byref(x) for x in v]
    ok_u = np.array([3, 1, 2, 4], np.uint32)
    zero_u = np.array([3, 0, 2, 4], np.uint32)
    bad = [
        (1, 3, 70, 0, ok_u, 4),               # m = 0
        (1, 3, 0, 5, ok_u, 4),                # n = 0
        (1, 3, 2 ** 32 - 2, 1, ok_u, 4),      # n + m = 2^32 - 1: one past the largest collection
        (1, 3, 2 ** 32 - 1, 1, ok_u, 4),      # n + m = 2^32
        (1, 3, 1, 2 ** 32 - 1, ok_u, 4),
        (1, 3, 2 ** 33, 1, ok_u, 4),
        (0, 3, 70, 5, ok_u, 4),               # n_dims outside 1..4
        (5, 3, 70, 5, ok_u, 4),
        (2, 3, 70, 5, zero_u, 4),             # a zero U_j
        (1, 3, 70, 5, ok_u, 0),               # grid_blocks = 0
    ]
    # the boundary: 2^32 - 3 joined by 1 is accepted (n + m = 2^32 - 2, the largest collection)
    assert lib.fhh_join_plan(1, 3, 2 ** 32 - 3, 1, ptr(ok_u, u32p), 4, *([None] * 9)) == 0
    for d, depth, n, m, U, grid in bad:
        assert lib.fhh_join_plan(d, depth, n, m, ptr(U, u32p), grid, *refs) == FHH_E_ARG, (d, n, m, grid)
        assert b"join_plan" in lib.fhh_last_error(None)
        assert [x.value for x in v] == [99] * len(NAMES), "a refusal writes nothing"
    assert lib.fhh_join_plan(1, 3, 70, 5, None, 4, *refs) == FHH_E_ARG                       # NULL n_unique
    with pytest.raises(fhh.FhhError, match="join_plan"):
        fhh.KeyCollection.join_plan(1, 3, 70, 0, [1], 4)
    # a zero U_j beyond n_dims is not looked at; NULL outputs are allowed
    assert lib.fhh_join_plan(1, 3, 70, 5, ptr(zero_u, u32p), 4, *([None] * 9)) == 0
    assert lib.fhh_join_plan(2, 3, 70, 130, ptr(ok_u, u32p), 7, None, refs[1], None, None, refs[4], *([None] * 4)) == 0
    want = jc.plan(2, 3, 70, 130, [3, 1], 7)
    assert v[1].value == want["first_mask"] and v[4].value == want["items"] and v[0].value == 99


def test_plan_boundary(fhh):
    """(2^32 - 3, 1) is the last pair accepted, (2^32 - 2, 1) the first refused: a collection holds at most
    2^32 - 2 clients, so that neither an index nor the count is the u32 all-ones word."""
    assert fhh.KeyCollection.join_plan(1, 1, 2 ** 32 - 3, 1, [1], 4) == jc.plan(1, 1, 2 ** 32 - 3, 1, [1], 4)
    with pytest.raises(fhh.FhhError, match="join_plan"):
        fhh.KeyCollection.join_plan(1, 1, 2 ** 32 - 2, 1, [1], 4)


def test_null_ctx(fhh):
    lib = fhh.lib()
    buf = np.zeros(16, np.uint8)
    from fuzzyheavyhitters_amd._lib import ptr
    assert lib.fhh_join_clients_bincode(None, ptr(buf), buf.size) == FHH_E_ARG
    assert b"null fhh_ctx" in lib.fhh_last_error(None)
    ms = (ctypes.c_double * 3)()
    by = (ctypes.c_uint64 * 1)()
    assert lib.fhh_join_timing(None, ms, by) == FHH_E_ARG


class _Coll:
    """what two_party_crawl reads before its first device call"""
    depth, n_dims = 8, 1

    def num_clients(self):
        return 10


def test_two_party_crawl_joins_argument_checks():
    import inspect

    from fuzzyheavyhitters_amd import party
    assert inspect.signature(party.two_party_crawl).parameters["joins"].default is None
    req = bytes(8)
    with pytest.raises(TypeError, match="joins"):
        party.two_party_crawl(None, None, 0.1, joins=[(3, (req, req))])
    with pytest.raises(TypeError, match="joins"):
        party.two_party_crawl(None, None, 0.1, joins={"3": (req, req)})
    with pytest.raises(TypeError, match="joins"):
        party.two_party_crawl(None, None, 0.1, joins={True: (req, req)})
    with pytest.raises(ValueError, match="joins"):
        party.two_party_crawl(None, None, 0.1, joins={3: (req,)})
    with pytest.raises(ValueError, match="joins"):
        party.two_party_crawl(None, None, 0.1, joins={3: req})
    with pytest.raises(TypeError, match="joins"):
        party.two_party_crawl(None, None, 0.1, joins={3: (req, "text")})
    # the level must be one this crawl runs (known once the collections' depth is)
    with pytest.raises(ValueError, match="joins"):
        party.two_party_crawl(_Coll(), _Coll(), 0.1, joins={8: (req, req)})
    with pytest.raises(ValueError, match="joins"):
        party.two_party_crawl(_Coll(), _Coll(), 0.1, joins={-1: (req, req)})
    with pytest.raises(ValueError, match="joins"):
        party.two_party_crawl(_Coll(), _Coll(), 0.1, levels=4, joins={4: (req, req)})


def test_compiler_report_of_the_join_kernel():
    """k_join_paths, the join form of k_eval_paths' body: no scratch, no VGPR spill, at most 128 VGPRs (4 waves per
    SIMD of a 1024-thread workgroup) and k_eval_paths' LDS, the 128 KiB of T-tables. k_eval_paths keeps its own
    report (test_frontier_plan.py) and stays the only kernel of that name."""
    u = resource_usage("fhh_kernels.hip")
    join = {k: v for k, v in u.items() if re.search(r"\d+k_join_paths", k)}
    paths = [v for k, v in u.items() if re.search(r"\d+k_eval_paths", k)]
    assert len(join) == 1 and len(paths) == 1, sorted(k for k in u if "paths" in k)
    (name, k), = join.items()
    assert int(k["ScratchSize [bytes/lane]"]) == 0, k
    assert int(k["VGPRs Spill"]) == 0, k
    assert int(k["VGPRs"]) + int(k.get("AGPRs", 0)) <= 128, k
    assert int(k["Occupancy [waves/SIMD]"]) == 4, k
    assert k["LDS Size [bytes/block]"] == paths[0]["LDS Size [bytes/block]"] == "131072", k
