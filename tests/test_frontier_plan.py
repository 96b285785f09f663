"""fhh_frontier_plan (CPU, host arithmetic): the per-dim de-duplication fhh_tree_init_at seeds the engine's tables
with, against a dict-based restatement; and the compiler's resource report of k_eval_paths, the kernel that
walks the keys to the planned prefixes (hipcc cross-compile for gfx950)."""
import ctypes

import numpy as np
import pytest

from kernel_usage import resource_usage

FHH_E_ARG = -1


def plan(paths):
    """(rc, n_unique [d], pos [F][d]) of fhh_frontier_plan on a uint8 array [F][d][depth]."""
    from fuzzyheavyhitters_amd._lib import lib, ptr, u32p
    a = np.ascontiguousarray(paths, np.uint8)
    F, d, depth = a.shape
    nu = np.full(4, 0xDEAD, np.uint32)
    pos = np.full((max(F, 1), d), 0xDEAD, np.uint32)
    rc = lib().fhh_frontier_plan(d, depth, F, ptr(a) if a.size else None, ptr(nu, u32p), ptr(pos, u32p))
    return rc, nu[:d], pos[:F]


def plan_model(paths):
    """Per dim: the distinct prefixes numbered in order of first appearance (a dict from the prefix's bits)."""
    F, d, depth = paths.shape
    nu, pos = np.zeros(d, np.uint32), np.zeros((F, d), np.uint32)
    for j in range(d):
        seen = {}
        for k in range(F):
            pos[k, j] = seen.setdefault(paths[k, j].tobytes(), len(seen))
        nu[j] = len(seen)
    return nu, pos


def random_frontier(rng, F, d, depth, pool):
    """F distinct nodes whose dim prefixes are drawn from `pool` prefixes per dim: shared prefixes are the rule."""
    prefixes = rng.integers(0, 2, (d, pool, depth), dtype=np.uint8)
    head = min(depth, 16)   # distinct prefixes: their first bits spell distinct numbers
    for j in range(d):
        for e, v in enumerate(rng.choice(1 << head, pool, replace=False)):
            prefixes[j, e, :head] = [(int(v) >> b) & 1 for b in range(head)]
    nodes = set()
    while len(nodes) < F:
        nodes.add(tuple(int(x) for x in rng.integers(0, pool, d)))
    nodes = sorted(nodes)
    rng.shuffle(nodes)
    return np.stack([np.stack([prefixes[j, node[j]] for j in range(d)]) for node in nodes])


@pytest.mark.parametrize("d", [1, 2, 3])
def test_plan_matches_model(fhh, d):
    rng = np.random.default_rng(100 + d)
    for depth, F, pool in ((1, 2 if d == 1 else 3, 2), (5, 7, 6), (33, 12, 5), (64, 40, 9), (71, 1, 1)):
        F = min(F, pool ** d, 2 ** (d * depth))
        paths = random_frontier(rng, F, d, depth, pool)
        rc, nu, pos = plan(paths)
        assert rc == 0, fhh.lib().fhh_last_error(None)
        mnu, mpos = plan_model(paths)
        assert np.array_equal(nu, mnu) and np.array_equal(pos, mpos), (d, depth, F)
        if d > 1 and F > pool:
            assert (mnu < F).any(), "the case shares no prefix"


def test_plan_shared_dim0_prefix_and_first_appearance_order(fhh):
    # nodes 0, 2 and 3 share their dim-0 prefix and differ in dim 1; dim 1's prefixes first appear as B, A, C
    A, B, C = [0, 1, 1], [1, 0, 0], [1, 1, 1]
    X, Y = [1, 1, 0], [0, 0, 0]
    paths = np.array([[X, B], [Y, B], [X, A], [X, C], [Y, A]], np.uint8)
    rc, nu, pos = plan(paths)
    assert rc == 0
    assert list(nu) == [2, 3]
    assert pos.tolist() == [[0, 0], [1, 0], [0, 1], [0, 2], [1, 1]]
    # either output may be NULL
    from fuzzyheavyhitters_amd._lib import lib, ptr
    assert lib().fhh_frontier_plan(2, 3, 5, ptr(paths), None, None) == 0


def test_plan_depth_zero(fhh):
    rc, nu, pos = plan(np.zeros((1, 2, 0), np.uint8))
    assert rc == 0 and list(nu) == [1, 1] and pos.tolist() == [[0, 0]]   # the root: fhh_tree_init
    rc, _, _ = plan(np.zeros((2, 2, 0), np.uint8))                       # two roots: a duplicate
    assert rc == FHH_E_ARG
    assert b"repeats" in fhh.lib().fhh_last_error(None)


def test_plan_refusals(fhh):
    L = fhh.lib()
    good = np.array([[[0, 1, 0]], [[1, 1, 0]], [[0, 0, 0]]], np.uint8)
    assert plan(good)[0] == 0
    dup = good.copy()
    dup[2] = dup[0]
    assert plan(dup)[0] == FHH_E_ARG and b"node 2 repeats the path of node 0" in L.fhh_last_error(None)
    two = good.copy()
    two[1, 0, 2] = 2
    assert plan(two)[0] == FHH_E_ARG and b"not 0 or 1" in L.fhh_last_error(None)
    assert plan(np.zeros((0, 1, 3), np.uint8))[0] == FHH_E_ARG and b"n_nodes = 0" in L.fhh_last_error(None)
    from fuzzyheavyhitters_amd._lib import ptr
    assert L.fhh_frontier_plan(0, 3, 3, ptr(good), None, None) == FHH_E_ARG
    assert L.fhh_frontier_plan(5, 3, 3, ptr(good), None, None) == FHH_E_ARG
    assert L.fhh_frontier_plan(1, 3, 3, None, None, None) == FHH_E_ARG        # NULL paths with depth > 0
    assert L.fhh_frontier_plan(2, 0, 1 << 30, None, None, None) == FHH_E_ARG  # n_nodes << d past u32
    assert b"u32" in L.fhh_last_error(None)
    # a refusal writes nothing
    nu, pos = np.full(1, 7, np.uint32), np.full((3, 1), 7, np.uint32)
    from fuzzyheavyhitters_amd._lib import u32p
    assert L.fhh_frontier_plan(1, 3, 3, ptr(dup), ptr(nu, u32p), ptr(pos, u32p)) == FHH_E_ARG
    assert (nu == 7).all() and (pos == 7).all()


def test_collection_frontier_plan_wrapper(fhh):
    paths = np.array([[[0, 1], [1, 1]], [[0, 1], [0, 0]]], np.uint8)
    nu, pos = fhh.KeyCollection.frontier_plan(paths)
    assert list(nu) == [1, 2] and pos.tolist() == [[0, 0], [0, 1]]
    with pytest.raises(fhh.FhhError):
        fhh.KeyCollection.frontier_plan(np.stack([paths[0], paths[0]]))


EVAL_PATHS = "_ZN3fhh12k_eval_pathsENS_13EvalPathsArgsE"


def test_eval_paths_kernel_resources():
    """k_eval_paths runs in k_expand's regime: 1024 threads share the 128 KiB of T-tables and
    nothing else in LDS, 4 waves per SIMD, 4 AES blocks in lockstep per lane, all state in registers."""
    u = resource_usage("fhh_kernels.hip")
    assert EVAL_PATHS in u, sorted(n for n in u if "eval" in n)
    k = u[EVAL_PATHS]
    assert k["ScratchSize [bytes/lane]"] == "0", k
    assert k["VGPRs Spill"] == "0", k
    assert int(k["VGPRs"]) <= 128, k                     # the 4-waves-per-SIMD budget of a 1024-thread workgroup
    assert int(k["Occupancy [waves/SIMD]"]) == 4, k
    assert int(k["LDS Size [bytes/block]"]) == 131072, k
