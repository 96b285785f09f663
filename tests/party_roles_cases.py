"""The workloads of tests/test_party_roles*.py: 130 clients (two full 64-client words and a partial one),
threshold 0 (the leader's threshold count is then 1, so every occupied child is kept and the frontier grows),
d = 1 at L = 12 and d = 2 at L = 8, with the plaintext crawl computed once per workload and shared.

A helper module (not a conftest): no entry point of the code under test is called here.

What these workloads can and cannot reach. A level's C is the frontier times 2^d, so it is never 1 and never
odd: "a level of one child" and "a level of odd C >= 5" do not exist in any crawl. The shapes that stand for
them, asserted in tests/test_party_roles_host.py at levels that are not the last:
  * C = 2 at d = 1: one window at chunk_children = 3, which the split cuts into two windows of ONE child each
    (a one-child chunk in each role);
  * a level of an odd number (>= 3) of windows whose last one is partial (C = 8 -> 3, 3, 2): a window is left
    without a partner and runs on its own after the pairs;
  * with chunk_children = 0 a level whose halves are odd and >= 5 (C = 10 -> 5 + 5): odd chunks of >= 5 children;
  * a level of at least 4 windows (C >= 10 at chunk_children = 3).
C = 1, 3 and 7 themselves are covered where they can occur: in fhh_party_role_plan (test_role_plan_*)."""
import functools

N_CLIENTS = 130
CHUNK = 3
THRESHOLD = 0.0   # two_party_crawl: max(1, int(0 * n)) = 1 at every level


@functools.lru_cache(maxsize=None)
def workload_of(d: int):
    """(the workload truncated to L bits, L) — seeds chosen for the level shapes above."""
    from fuzzyheavyhitters_amd import workload
    L, sites, seed = {1: (12, 5, 1), 2: (8, 3, 1)}[d]
    wl = workload.zipf_workload(N_CLIENTS, 32, d, num_sites=sites, seed=seed)
    wl.left, wl.right = wl.left[:, :, :L].copy(), wl.right[:, :, :L].copy()
    return wl, L


@functools.lru_cache(maxsize=None)
def plaintext_of(d: int):
    """(per-level counts, sorted final paths -> count) of the plaintext crawl; computed once, never changed."""
    from fuzzyheavyhitters_amd import workload
    wl, L = workload_of(d)
    counts, paths, vals = workload.plaintext_crawl(wl.left, wl.right, 1, 1)
    for c in counts:
        c.setflags(write=False)
    return counts, dict(zip(paths, vals))


def final_set(res):
    """{path (d bit-tuples) -> value} of a TwoPartyResult's final list."""
    return {tuple(tuple(int(b) for b in p) for p in r.path): int(r.value) for r in res.final}


def windows_of(C: int, chunk: int, split: bool):
    """The window sizes the issue defines, restated (not read from the code under test): chunks of `chunk`
    children (0, or a level that fits one chunk: one window), a one-window level of C >= 2 cut into
    ceil(C / 2), floor(C / 2) when split."""
    if chunk <= 0 or C <= chunk:
        if split and C >= 2:
            return [(C + 1) // 2, C // 2]
        return [C]
    return [min(chunk, C - b) for b in range(0, C, chunk)]
