"""leader.add_fuzzy_keys (GPU): a population's points turned into the two servers' add_keys requests chunk by chunk
(leader.rs:130-163, 391-415). The concatenated requests equal those of one gen_keys_ball over the whole
population and, through the numpy serializer, the oracle's keys of the oracle's bounds; the chunking moves no
request boundary; the requests appended to fresh collections crawl to the plaintext heavy hitters."""
import numpy as np
import pytest

import ball_cases as bc

N, L, D, BALL, CHUNK = 250, 40, 1, 1, 100


@pytest.fixture(scope="module")
def reference(oracle):
    """The population, the oracle's bounds and keys: computed once, read by every test."""
    from fuzzyheavyhitters_amd import workload
    wl = workload.zipf_workload(N, L, D, num_sites=8, seed=21)
    left, right = bc.oracle_bounds(oracle, wl.alpha, BALL)
    keys = oracle.gen_keys(left, right, bc.derived_roots(oracle, bc.SEED, 0, N, D))
    return workload.pack_points(wl.alpha), left, right, keys


def expected_requests(ks, B):
    """The numpy serializer on the oracle's keys, B clients per request."""
    from fuzzyheavyhitters_amd import workload
    return [workload.add_keys_request_bincode(*[x[a:min(a + B, N)] for x in
                                                (ks.key_idx, ks.root_seed, ks.cw_seed, ks.cw_bits)])
            for a in range(0, N, B)]


def test_chunk_must_be_a_multiple_of_the_batch():
    """Refused before any collection is made (no GPU): a chunk that would cut a request in two."""
    import fuzzyheavyhitters_amd as fhh
    pts = np.zeros((10, 1, 5), np.uint8)
    for batch, chunk in ((7, 100), (100, 150), (3, 10)):
        with pytest.raises(fhh.FhhError, match="multiple"):
            next(fhh.add_fuzzy_keys(pts, 1, n_dims=1, data_len=40, seed=bc.SEED, batch=batch, chunk=chunk))
    with pytest.raises(fhh.FhhError):
        next(fhh.add_fuzzy_keys(pts, 1, n_dims=1, data_len=40, seed=bc.SEED, batch=1, chunk=0))


@pytest.mark.gpu
@pytest.mark.parametrize("batch,chunk", [(0, 100), (100, 100), (7, 98)], ids=["batch0", "batch100", "batch7-chunk98"])
def test_chunked_requests_equal_one_call_and_the_oracle(reference, batch, chunk):
    """n = 250 in chunks of 100 at batch 0 and 100. Batch 7 does not divide a chunk of 100 — that pair is the
    refusal above — so its requests are checked at chunk 98. With a batch the requests are, byte for byte, those
    of one gen_keys_ball over the population and one export; batch 0 is one request per chunk, whose client
    records, in order, are the records of the population's single request."""
    import fuzzyheavyhitters_amd as fhh
    from fuzzyheavyhitters_amd import workload
    pts, _, _, keys = reference
    chunks = list(fhh.add_fuzzy_keys(pts, BALL, n_dims=D, data_len=L, seed=bc.SEED, batch=batch, chunk=chunk))
    assert len(chunks) == (N + chunk - 1) // chunk and all(len(c) == 2 for c in chunks)
    whole = fhh.KeyCollection(L, D), fhh.KeyCollection(L, D)
    fhh.gen_keys_ball(whole[0], whole[1], pts, BALL, seed=bc.SEED)
    for s in range(2):
        got = [r for c in chunks for r in c[s]]
        want = expected_requests(keys[s], batch or chunk)
        assert len(got) == len(want) == (N + (batch or chunk) - 1) // (batch or chunk)
        for q, (a, b) in enumerate(zip(got, want)):
            assert np.array_equal(a, b), f"server {s} request {q}"
        one = whole[s].export_keys_bincode(0, N, batch)
        if batch:
            assert np.array_equal(np.concatenate(got), one)
        else:
            assert np.array_equal(np.concatenate([r[8:] for r in got]), one[8:])
            assert one.size == 8 + N * (8 + 2 * D * (25 + 20 * L))


@pytest.mark.gpu
def test_requests_appended_to_fresh_collections_crawl_to_the_heavy_hitters(oracle, reference):
    import fuzzyheavyhitters_amd as fhh
    from fuzzyheavyhitters_amd import sim_crawl, workload
    pts, left, right, _ = reference
    servers = [fhh.KeyCollection(L, D), fhh.KeyCollection(L, D)]
    for reqs in fhh.add_fuzzy_keys(pts, BALL, n_dims=D, data_len=L, seed=bc.SEED, batch=50, chunk=CHUNK):
        for c, rs in zip(servers, reqs):
            for r in rs:
                c.add_keys_bincode_append(r)
    assert [c.num_clients() for c in servers] == [N, N]
    res = sim_crawl(servers[0], servers[1], 0.02, mode="count")
    t, tl = oracle.thresholds(0.02, N)
    counts, paths, finals = workload.plaintext_crawl(left, right, t, tl)
    assert len(paths) > 0
    assert [c.tolist() for c in res.counts] == [c.tolist() for c in counts]
    assert [tuple(tuple(int(b) for b in pj) for pj in r.path) for r in res.final] == paths
    assert [int(r.value) for r in res.final] == finals
