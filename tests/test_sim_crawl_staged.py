"""fhh_sim_crawl's device loop on collections whose keys are still staged by add_keys (never initialised): the loop
uploads them before it sizes its prefix tables by npad (GPU). The result is that of the same keys made on the
device by gen_keys_pair."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("d", [1, 2])
def test_device_loop_on_staged_keys(d):
    import fuzzyheavyhitters_amd as fhh
    from fuzzyheavyhitters_amd import workload
    n, L = 130, 16
    wl = workload.zipf_workload(n, 32, d, num_sites=4, seed=310 + d)
    left, right = wl.left[:, :, :L].copy(), wl.right[:, :, :L].copy()
    g = fhh.KeyCollection(L, d), fhh.KeyCollection(L, d)
    fhh.gen_keys_pair(*g, left, right, wl.root_seeds)
    s = fhh.KeyCollection(L, d), fhh.KeyCollection(L, d)
    for c, src in zip(s, g):
        c.add_keys(*src.export_keys())
    rs = fhh.sim_crawl(*s, 0.05, mode="count")          # staged keys, no tree_init before
    rg = fhh.sim_crawl(*g, 0.05, mode="count")
    assert list(rs.level_children) == list(rg.level_children)
    assert len(rs.counts) == L and all(np.array_equal(x, y) for x, y in zip(rs.counts, rg.counts))
    assert [(r.path, r.value) for r in rs.final] == [(r.path, r.value) for r in rg.final] and len(rs.final) > 0
    thr = max(1, int(0.05 * n))
    plain, _, _ = workload.plaintext_crawl(left, right, thr, thr)
    assert all(np.array_equal(x, y) for x, y in zip(rs.counts, plain))
