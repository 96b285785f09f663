"""The device level loop's prune (k_prune, k_gather_hist: csrc/fhh_loop.hip) past one workgroup pass, with counts
exactly on the threshold in every form of keep_of, and FE partials over two client chunks across a growth abort.

The reference of every comparison is `workload.plaintext_crawl` on workloads constructed in loop_frontier_cases.py;
the host-driven loop is a second witness only (it shares the sum kernels with the device loop). The conditions that
make the workloads reach those paths are asserted on the reference alone, in tests that need no GPU.

Sizes the wide workloads reach (reference; C children, nf kept, E = 2 n_live entries scanned at a non-last level):
  wide_d1_ball0  C 2058, nf 1029 (level 10) and 1200 final nodes, E 1572
  wide_d1_ball1  C 3086, nf 1543 (level 10) and 2653 final nodes, E 1798
  wide_d2        C 4400, nf 1100, E 1382 (level 10 of 12) with n_live 691 < F = 1100"""
import re

import numpy as np
import pytest

import loop_frontier_cases as lc

gpu = pytest.mark.gpu
ABORT = re.compile(r"\[fhh loop\] abort at level (\d+) \(batch end \d+\): need_entries (\d+) need_nodes (\d+) "
                   r"F (\d+) C (\d+) -> E_cap (\d+) F_cap (\d+)")

# start capacities of the device-loop runs (0 = the default, 256). d = 2 fans out by 4: from 256 and from 2 its
# frontier jumps from 251 to 701 nodes, the one abort there grows to 2048 and nothing above 1024 is ever missing;
# from 1024 the abort is the one of level 6, 1068 nodes.
STARTS = {"wide_d1_ball0": (0, 2), "wide_d1_ball1": (0, 2), "wide_d2": (0, 2, 1024)}


# ---- conditions on the inputs: the reference alone, no GPU -----------------------------------------------

@pytest.mark.parametrize("name", lc.WIDE)
def test_wide_workloads_reach_the_multi_pass_paths(name):
    case, ref = lc.case(name), lc.reference(name)
    L, last = case.levels, case.levels - 1
    P = lc.PRUNE_THREADS
    assert case.left.shape[0] <= 4100 and L <= 12 and case.thr == 1
    # step 1 takes three passes: C > 2048
    assert max(ref.children) > 2 * P
    # nf > 1024: pos_out at a non-last level (d = 2, and d = 1 where the level before the last is that wide),
    # final_vals at the last level (d = 1)
    if case.dims == 2:
        assert max(ref.n_kept[:last]) > P
    else:
        assert ref.n_kept[last] > P
    # the live scan's second pass, with its carry and ranks: E = 2 * n_live > 1024 at a prune that is not the last
    assert max(ref.entries[:last]) > P
    if case.dims == 2:   # ... with shared dim prefixes: fewer live entries than nodes
        lv = int(np.argmax(ref.entries[:last]))
        assert max(ref.live[lv - 1]) < ref.n_kept[lv - 1]
    # k_gather_hist: rows of more than 256 kept children on both sides of a capacity epoch change, for the
    # aborts that follow from the start capacity (d = 1: the default one)
    start = lc.DEFAULT_CAPACITY if case.dims == 1 else 1024
    assert (0 if start == lc.DEFAULT_CAPACITY else start) in STARTS[name]
    epochs = [a[0] for a in lc.planned_aborts(ref, start)]      # the rows of levels >= an abort's move to a new epoch
    wide = [lv for lv in range(L) if ref.n_kept[lv] > lc.GATHER_THREADS]
    assert any(min(wide) < e <= max(wide) for e in epochs), (wide, epochs)
    # what the GPU test then sees in the debug lines follows from the start capacities
    plans = [a for s in STARTS[name] for a in lc.planned_aborts(ref, s or lc.DEFAULT_CAPACITY)]
    assert any(nn > P for _, _, nn in plans) and any(ne > P for _, ne, _ in plans)
    if name == "wide_d1_ball1":
        assert any(lv == last for lv, _, _ in lc.planned_aborts(ref, lc.DEFAULT_CAPACITY))


def test_wide_d1_points_are_as_described():
    case, ref = lc.case("wide_d1_ball0"), lc.reference("wide_d1_ball0")
    assert case.left.shape == (lc.D1_DISTINCT + lc.D1_REPEATS, 1, 12) and np.array_equal(case.left, case.right)
    assert len(ref.final) == lc.D1_DISTINCT and sum(v for _, v in ref.final) == case.left.shape[0]
    assert max(v for _, v in ref.final) > 1                       # the repeats: counts are multiplicities
    b1 = lc.reference("wide_d1_ball1")
    assert len(b1.final) > 2 * lc.D1_DISTINCT                     # ball 1: clients sit in several nodes
    assert sum(v for _, v in b1.final) > 2 * case.left.shape[0]


def test_caterpillars_put_counts_on_the_threshold_at_every_level():
    case, ref = lc.case("caterpillars"), lc.reference("caterpillars")
    thr = case.thr
    assert thr == lc.CAT_THR == 5 and case.threshold * case.n_total == 5.0 and case.levels == 10
    assert case.left.shape[0] == 90
    for lv in range(1, case.levels):
        assert (ref.counts[lv] == thr).any() and (ref.counts[lv] == thr - 1).any(), lv
    assert any(v == thr for _, v in ref.final)                    # a final node of value exactly thr_last
    assert (ref.counts[-1] == thr - 1).any()                      # ... and a last-level child one below it
    assert len(ref.final) == 10 and ref.children[-1] == 20


def test_floored_threshold_case():
    case, ref = lc.case("floored_threshold"), lc.reference("floored_threshold")
    assert int(case.threshold * case.n_total) == lc.FLOOR_THR == 28 and case.thr == 28
    assert round(case.threshold * case.n_total) == 29             # what a leader that rounds would take
    assert case.left.shape[0] == case.n_total == 100
    assert 28 in ref.counts[1].tolist() and 27 in ref.counts[1].tolist()
    assert [v for _, v in ref.final] == [28, 30]                  # the 28 is kept to the end, at thr_last too


def test_second_client_chunk_decides_a_kept_path():
    case, ref = lc.case("two_chunks"), lc.reference("two_chunks")
    n1 = lc.CLIENT_CHUNK
    assert case.left.shape == (4100, 1, 10) and case.thr == 4 and case.left.shape[0] - n1 == 4
    without = lc.reference_of(case.left[:n1], case.right[:n1], case.thr, case.thr)
    lone = [bool(b) for b in lc.int_bits(lc.CHUNK_LONE_VALUE, case.levels)]
    assert ([lone], 4) in ref.final and all(p != [lone] for p, _ in without.final)
    assert len(ref.final) == len(without.final) + 1
    # a kept child's count changes at every level, and the kept set itself from the level at which the lone
    # value's prefix is its own
    differs = [lv for lv in range(case.levels) if ref.n_kept[lv] != without.n_kept[lv]]
    assert differs == list(range(lc.CHUNK_LONE_BITS - 1, case.levels))
    for lv in range(differs[0]):
        assert not np.array_equal(ref.counts[lv][ref.kept[lv]], without.counts[lv][without.kept[lv]])
    # from capacity 2 the crawl aborts several times below the last level, at levels with C > 1
    plan = lc.planned_aborts(ref, 2)
    assert len(plan) >= 3 and all(lv < case.levels - 1 for lv, _, _ in plan)
    assert sum(ref.children[lv] > 1 for lv, _, _ in plan) >= 3


# ---- the crawls -------------------------------------------------------------------------------------------

def _pair(case):
    import fuzzyheavyhitters_amd as fhh
    c0, c1 = fhh.KeyCollection(case.levels, case.dims), fhh.KeyCollection(case.levels, case.dims)
    fhh.gen_keys_pair(c0, c1, case.left, case.right, case.roots)
    return c0, c1


def _check_crawl(res, ref):
    assert res.level_children.tolist() == ref.children
    assert res.level_kept.tolist() == ref.n_kept
    for lv, cnt in enumerate(ref.counts):
        assert np.array_equal(res.counts[lv], cnt), f"counts of level {lv}"
    assert [(r.path, r.value) for r in res.final] == ref.final


def _check_frontier(c0, c1, ref):
    """The engine state a device-loop crawl leaves is the frontier before the last level: the reference's kept
    nodes of level L - 2, and, read through the compacted pos / live lists, states whose share strings
    (t ^ y, both sides of every dim) agree between the servers for exactly the clients inside each node."""
    lv = len(ref.kept) - 2
    ty = []
    for c in (c0, c1):
        seeds, t, y = c.export_states()
        assert seeds.shape[0] == ref.n_kept[lv]
        assert np.array_equal(c.frontier_paths(), ref.paths[lv])
        ty.append(t ^ y)
    inside = np.all(ty[0] == ty[1], axis=(2, 3)).sum(axis=1)
    assert np.array_equal(inside.astype(np.uint64), ref.counts[lv][ref.kept[lv]])


@pytest.fixture
def loop_aborts(monkeypatch, capfd):
    """Turns the loop's debug lines on; each call returns the aborts since the last one as
    (level, need_entries, need_nodes, C)."""
    monkeypatch.setenv("FHH_DEBUG_LOOP", "1")
    capfd.readouterr()

    def take():
        cap = capfd.readouterr()
        print(cap.out, end="")   # what the test printed so far stays in its report
        return [(int(m[1]), int(m[2]), int(m[3]), int(m[5])) for m in ABORT.finditer(cap.err)]
    return take


def _device_crawl(case, ref, loop_aborts, cap, **kw):
    """One device-loop crawl on fresh collections (capacities persist on a ctx), checked against the reference."""
    from fuzzyheavyhitters_amd import sim_crawl
    c0, c1 = _pair(case)
    try:
        loop_aborts()
        res = sim_crawl(c0, c1, case.threshold, nclients_total=case.n_total, init_capacity=cap, **kw)
        aborts = loop_aborts()
        print(f"{case.name} {kw.get('mode', 'count')} start {cap or lc.DEFAULT_CAPACITY}: aborts (level, "
              f"need_entries, need_nodes, C) {aborts}")
        _check_crawl(res, ref)
        _check_frontier(c0, c1, ref)
    finally:
        c0.close()
        c1.close()
    return aborts


def _host_crawl(case, ref, **kw):
    from fuzzyheavyhitters_amd import sim_crawl
    c0, c1 = _pair(case)
    try:
        _check_crawl(sim_crawl(c0, c1, case.threshold, nclients_total=case.n_total, host_loop=True, **kw), ref)
    finally:
        c0.close()
        c1.close()


MODES = {"count": dict(mode="count"), "fe": dict(mode="fe", prf_seed=0x5EED)}


@gpu
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", lc.WIDE)
def test_wide_frontier(loop_aborts, name, mode):
    """C, nf and E past one 1024-thread pass of k_prune, from every start capacity of STARTS: the crawl and the
    frontier it leaves equal the reference, and the aborts on the way had needs of more than one pass."""
    case, ref = lc.case(name), lc.reference(name)
    aborts = []
    for cap in STARTS[name]:
        aborts += _device_crawl(case, ref, loop_aborts, cap, **MODES[mode])
    _host_crawl(case, ref, **MODES[mode])
    assert any(nn > lc.PRUNE_THREADS for _, _, nn, _ in aborts), aborts
    assert any(ne > lc.PRUNE_THREADS for _, ne, _, _ in aborts), aborts
    if name == "wide_d1_ball1":   # 256 -> 512 -> 2048 nodes, then 2653 kept at the last level
        assert any(lv == case.levels - 1 for lv, _, _, _ in aborts), aborts


FORMS = {
    "count": dict(mode="count"),
    "fe": dict(mode="fe", prf_seed=0xCA7),                                    # FE difference; FE255 at the last level
    "fe-ring32": dict(mode="fe", prf_seed=0xCA7, gc="ot", table_ring32=True),   # Z_2^32 difference at the FE levels
}


@gpu
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", ["caterpillars", "floored_threshold"])
def test_counts_on_the_threshold(loop_aborts, name, form):
    """Children of count exactly thr (kept) and thr - 1 (dropped) at every level, in each form of keep_of."""
    case, ref = lc.case(name), lc.reference(name)
    _device_crawl(case, ref, loop_aborts, 0, **FORMS[form])
    if form != "fe-ring32":
        _host_crawl(case, ref, **FORMS[form])


@gpu
def test_fe_partials_over_two_client_chunks_and_aborts(loop_aborts):
    """4100 clients (k_child_sums_fe adds two client chunks into the partials) and growth aborts at FE levels: a
    chunk added twice or lost across a resumption, or partials left stale for the level after one, is a count that
    differs from the plaintext one."""
    case, ref = lc.case("two_chunks"), lc.reference("two_chunks")
    fe = dict(mode="fe", prf_seed=0xC4)
    aborts = _device_crawl(case, ref, loop_aborts, 2, **fe)
    fe_level = [a for a in aborts if a[0] < case.levels - 1]
    assert len(fe_level) >= 2 and any(C > 1 for _, _, _, C in fe_level), aborts
    assert any(C >= 32 for _, _, _, C in fe_level), aborts   # partials of more than a few children were carried over
    aborts = _device_crawl(case, ref, loop_aborts, 0, **fe)
    assert aborts and all(a[0] < case.levels - 1 for a in aborts), aborts
    _host_crawl(case, ref, **fe)
