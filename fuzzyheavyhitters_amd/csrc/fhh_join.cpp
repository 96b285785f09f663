// fhh_join_clients_bincode: clients that join a crawl in progress. One add_keys request is decoded onto the
// clients [n, n + m) of a ctx that has a frontier, and the joiners' keys are walked from the root to the
// frontier's prefixes (k_join_paths, fhh_kernels.hip), so that the ctx is what a fresh collection of the n + m
// clients brought to the same frontier by fhh_tree_init_at would be. Where the 64-client word count grows, the
// key buffers and every dim's live table entries are copied into buffers of the new stride first (old and new
// both live until the stream has drained, as in fhh_retain_clients); where it does not, the joiners take the
// free lanes of the last word in place.
#include "fhh_engine.h"

#include <algorithm>
#include <cstring>

namespace fhh {
namespace eng {

namespace {

const char kWho[] = "join_clients_bincode: ";

// the direction bits of every dim's live entries, from the crawl history: dirs[j] = [U_j][dir_words], bit l % 32
// of word l / 32 = the entry's direction at level l (EvalPathsJob::dirs)
int join_dirs(fhh_ctx* ctx, uint32_t dir_words, std::vector<uint32_t> (&dirs)[kMaxDims]) {
    const uint32_t d = ctx->d, depth = ctx->level;
    const size_t F = ctx->frontier.size();
    if (depth && (ctx->hist.size() < depth || ctx->hist[depth - 1].size() != F))
        return ctx->fail(FHH_E_STATE, std::string(kWho) + "the crawl history does not cover the frontier");
    std::vector<uint8_t> done[kMaxDims];
    size_t left = 0;
    for (uint32_t j = 0; j < d; j++) {
        const size_t U = ctx->tab[j].live.size();
        dirs[j].assign(U * dir_words, 0u);
        done[j].assign(U, 0);
        left += U;
    }
    std::vector<uint32_t> step(depth);
    for (size_t k = 0; k < F && left; k++) {
        bool need = false;
        for (uint32_t j = 0; j < d; j++) need = need || !done[j][ctx->frontier[k].pos[j]];
        if (!need) continue;
        uint32_t node = (uint32_t)k;
        for (int64_t lv = (int64_t)depth - 1; lv >= 0; lv--) {
            if (node >= ctx->hist[(size_t)lv].size())
                return ctx->fail(FHH_E_STATE, std::string(kWho) + "the crawl history does not cover the frontier");
            const auto& pr = ctx->hist[(size_t)lv][node];
            step[(size_t)lv] = pr.second;
            node = pr.first;
        }
        for (uint32_t j = 0; j < d; j++) {
            const uint32_t e = ctx->frontier[k].pos[j];
            if (done[j][e]) continue;
            uint32_t* w = dirs[j].data() + (size_t)e * dir_words;
            for (uint32_t l = 0; l < depth; l++) w[l >> 5] |= ((step[l] >> j) & 1u) << (l & 31);
            done[j][e] = 1;
            left--;
        }
    }
    if (left) return ctx->fail(FHH_E_STATE, std::string(kWho) + "a live table entry belongs to no frontier node");
    return FHH_OK;
}

}  // namespace

// the request's framing (fhh_add_keys_bincode_append's): *m clients, their records from req + 8 on
int join_parse(fhh_ctx* ctx, const uint8_t* req, uint64_t len, uint64_t* m) {
    if (!req || len < 8) return ctx->fail(FHH_E_ARG, std::string(kWho) + "buffer shorter than the u64 length");
    uint64_t v = 0;
    for (int i = 0; i < 8; i++) v |= (uint64_t)req[i] << (8 * i);
    const uint64_t KB = 25 + 20ull * ctx->L, R = 8 + (uint64_t)ctx->K * KB;
    if (v == 0) return ctx->fail(FHH_E_ARG, std::string(kWho) + "no clients");
    if (v > (len - 8) / R || 8 + v * R != len)
        return ctx->fail(FHH_E_ARG, std::string(kWho) + "length does not match n clients x n_dims x data_len");
    *m = v;
    return FHH_OK;
}

int join_check_state(fhh_ctx* ctx) {
    if (!ctx->dev_keys && ctx->h_n == 0) return ctx->fail(FHH_E_STATE, std::string(kWho) + "the ctx holds no keys");
    if (ctx->phase == Phase::kNoInit)
        return ctx->fail(FHH_E_STATE, std::string(kWho) + "no frontier yet (before fhh_tree_init clients are added with "
                                                          "fhh_add_keys_bincode_append or fhh_add_keys)");
    if (ctx->phase == Phase::kPending || ctx->phase == Phase::kPendingLast)
        return ctx->fail(FHH_E_STATE, std::string(kWho) + "a crawl's children are pending (prune first)");
    if (!ctx->dev_keys || ctx->n == 0) return ctx->fail(FHH_E_STATE, std::string(kWho) + "the ctx holds no keys");
    return FHH_OK;
}

int join_one(fhh_ctx* ctx, uint64_t m, const uint8_t* recs) {
    int rc = ctx_set_device(ctx);
    if (rc) return rc;
    rc = join_check_state(ctx);
    if (rc) return rc;
    const uint64_t n = ctx->n, n2 = n + m;
    if (m == 0) return ctx->fail(FHH_E_ARG, std::string(kWho) + "no clients");
    if (!join_count_fits(n, m))
        return ctx->fail(FHH_E_ARG, std::string(kWho) + std::to_string(n) + " + " + std::to_string(m) +
                                        " clients do not fit the engine's u32 client indices");
    const size_t K = ctx->K, L = ctx->L;
    const uint32_t d = ctx->d, depth = ctx->level, dir_words = (depth + 31) / 32;
    const uint64_t nw = ctx->nw, npad = ctx->npad, nw2 = (n2 + 63) / 64, npad2 = nw2 * 64;
    const bool grow = nw2 != nw;

    // the walk's lists, every dim's in one upload: [dirs_0 | rows_0 | dirs_1 | rows_1 | ...]. After a growth the
    // live entries are rows 0 .. U - 1 of the new tables (the copy compacts them), else they stay where they are
    std::vector<uint32_t> dirs[kMaxDims];
    rc = join_dirs(ctx, dir_words, dirs);
    if (rc) return rc;
    std::vector<uint32_t> lists;
    size_t dirs_off[kMaxDims] = {}, rows_off[kMaxDims] = {};
    uint32_t U[kMaxDims] = {};
    for (uint32_t j = 0; j < d; j++) {
        const std::vector<uint32_t>& live = ctx->tab[j].live;
        U[j] = (uint32_t)live.size();
        dirs_off[j] = lists.size();
        lists.insert(lists.end(), dirs[j].begin(), dirs[j].end());
        rows_off[j] = lists.size();
        for (uint32_t e = 0; e < U[j]; e++) lists.push_back(grow ? e : live[e]);
    }
    const JoinPlan plan = join_plan(d, depth, n, m, U, (uint64_t)std::max(ctx->grid, 1));

    // every allocation before the first launch: a refusal for memory leaves nothing half done
    const uint64_t KB = 25 + 20ull * L, R = 8 + (uint64_t)K * KB;
    DevBuf lists_dev, cs, cb, rs, ki, valid2, seed2[kMaxDims], t2[kMaxDims], y2[kMaxDims];
    size_t cap2[kMaxDims] = {};
    HIP_TRY(ctx, ctx->app_buf.ensure(8 + m * R + 4));   // whole-dword reads: up to 3 B past the end
    HIP_TRY(ctx, ctx->app_err.ensure(4));
    HIP_TRY(ctx, lists_dev.ensure(lists.size() * 4));
    if (grow) {
        HIP_TRY(ctx, cs.ensure(L * K * npad2 * 16));
        HIP_TRY(ctx, cb.ensure(L * K * 4 * nw2 * 8));
        HIP_TRY(ctx, rs.ensure(K * npad2 * 16));
        HIP_TRY(ctx, ki.ensure(K * nw2 * 8));
        HIP_TRY(ctx, valid2.ensure(nw2 * 8));
        for (uint32_t j = 0; j < d; j++) {
            cap2[j] = std::max<size_t>(U[j], 4);   // table_ensure's floor
            HIP_TRY(ctx, seed2[j].ensure(cap2[j] * 2 * npad2 * 16));
            HIP_TRY(ctx, t2[j].ensure(cap2[j] * 2 * nw2 * 8));
            HIP_TRY(ctx, y2[j].ensure(cap2[j] * 2 * nw2 * 8));
        }
    }
    uint4* k_cs = grow ? cs.as<uint4>() : ctx->cw_seed.as<uint4>();
    uint64_t* k_cb = grow ? cb.as<uint64_t>() : ctx->cw_bits.as<uint64_t>();
    uint4* k_rs = grow ? rs.as<uint4>() : ctx->root_seed.as<uint4>();
    uint64_t* k_ki = grow ? ki.as<uint64_t>() : ctx->key_idx.as<uint64_t>();

    hipEvent_t ev[8] = {};   // key re-pitch 0 .. 1, decode 2 .. 3, table re-pitch 4 .. 5, walk 6 .. 7
    struct EvGuard {
        hipEvent_t* e;
        ~EvGuard() {
            for (int i = 0; i < 8; i++)
                if (e[i]) (void)hipEventDestroy(e[i]);
        }
    } guard{ev};
    for (auto& e : ev) HIP_TRY(ctx, hipEventCreate(&e));
    std::vector<uint64_t> v(nw2, ~0ull);
    if (n2 % 64) v[nw2 - 1] = (1ull << (n2 % 64)) - 1;
    uint32_t herr = 0;
    uint64_t moved = 0;   // bytes the re-pitch copies (read once, written once)

    // 1. the batch onto the clients [n, n + m): into the new key buffers where the stride changes
    auto decode = [&]() -> int {
        HIP_TRY(ctx, hipMemsetAsync(ctx->app_err.p, 0, 4, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(ctx->app_buf.p, &m, 8, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(ctx->app_buf.as<uint8_t>() + 8, recs, m * R, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(lists_dev.p, lists.data(), lists.size() * 4, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipEventRecord(ev[0], ctx->stream));
        if (grow) {
            HIP_TRY(ctx, launch_repitch_seeds(ctx->cw_seed.as<uint4>(), k_cs, L * K, npad, npad, npad2, ctx->stream));
            HIP_TRY(ctx, launch_repitch_words(ctx->cw_bits.as<uint64_t>(), k_cb, L * K * 4, nw, nw, nw2, ctx->stream));
            HIP_TRY(ctx, launch_repitch_seeds(ctx->root_seed.as<uint4>(), k_rs, K, npad, npad, npad2, ctx->stream));
            HIP_TRY(ctx, launch_repitch_words(ctx->key_idx.as<uint64_t>(), k_ki, K, nw, nw, nw2, ctx->stream));
            moved += (L * K + K) * npad * 16 + (L * K * 4 + K) * nw * 8;
        }
        HIP_TRY(ctx, hipEventRecord(ev[1], ctx->stream));
        HIP_TRY(ctx, hipEventRecord(ev[2], ctx->stream));
        HIP_TRY(ctx, launch_keys_from_bincode_at(ctx->app_buf.as<uint8_t>(), n, m, d, ctx->L, (uint32_t)npad2, (uint32_t)nw2,
                                                 k_cs, k_cb, k_rs, k_ki, ctx->app_err.as<uint32_t>(), ctx->stream));
        HIP_TRY(ctx, hipEventRecord(ev[3], ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(&herr, ctx->app_err.p, 4, hipMemcpyDeviceToHost, ctx->stream));
        return FHH_OK;
    };
    rc = decode();
    if (rc) {
        (void)hipStreamSynchronize(ctx->stream);
        return rc;
    }
    rc = ctx_sync(ctx);   // `recs`, `lists` are read and `herr` is written until here
    if (rc) return rc;
    if (herr) {
        // nothing of the tables has been written. The new buffers leave with this frame; in place, the lanes the
        // batch touched are zero again (the _at kernels at m = 0, as append_rollback)
        if (!grow) {
            HIP_TRY(ctx, launch_keys_from_bincode_at(ctx->app_buf.as<uint8_t>(), n, 0, d, ctx->L, (uint32_t)npad, (uint32_t)nw,
                                                     k_cs, k_cb, k_rs, k_ki, ctx->app_err.as<uint32_t>(), ctx->stream));
            rc = ctx_sync(ctx);
            if (rc) return rc;
        }
        return ctx->fail(FHH_E_ARG, std::string(kWho) + bincode_malformed_text(herr));
    }

    // 2. the live table entries to the new stride (compacted to rows 0 .. U - 1), then the joiners' walk
    EvalPathsArgs a{};
    JoinPathsExtra x{};
    a.cw_seed = k_cs;
    a.cw_bits = k_cb;
    a.root_seed = k_rs;
    a.key_idx = k_ki;
    a.d = d;
    a.K = ctx->K;
    a.npad = (uint32_t)npad2;
    a.nw = (uint32_t)nw2;
    a.depth = depth;
    a.dir_words = dir_words;
    x.first_mask = plan.first_mask;
    x.w_first = (uint32_t)plan.first_word;
    x.words = (uint32_t)plan.words;
    auto walk = [&]() -> int {
        HIP_TRY(ctx, hipEventRecord(ev[4], ctx->stream));
        for (uint32_t j = 0; j < d; j++) {
            DimTable& T = ctx->tab[j];
            EvalPathsJob& J = a.job[j];
            J.dst_seed = grow ? seed2[j].as<uint4>() : T.seed[T.cur].as<uint4>();
            J.dst_t = grow ? t2[j].as<uint64_t>() : T.t[T.cur].as<uint64_t>();
            J.dst_y = grow ? y2[j].as<uint64_t>() : T.y[T.cur].as<uint64_t>();
            J.dirs = lists_dev.as<uint32_t>() + dirs_off[j];
            J.n_prefixes = U[j];
            J.item_begin = a.total_items;
            a.total_items += 2 * plan.words * (((uint64_t)U[j] + kEvalPathsP - 1) / kEvalPathsP);
            x.rows[j] = lists_dev.as<uint32_t>() + rows_off[j];
            // runs of consecutive live entries move in one copy each
            for (size_t k0 = 0; grow && k0 < U[j];) {
                size_t k1 = k0 + 1;
                while (k1 < U[j] && T.live[k1] == T.live[k1 - 1] + 1) k1++;
                const uint64_t rows = 2 * (k1 - k0), r_src = 2ull * T.live[k0], r_dst = 2ull * k0;
                HIP_TRY(ctx, launch_repitch_seeds(T.seed[T.cur].as<uint4>() + r_src * npad, J.dst_seed + r_dst * npad2, rows,
                                                  npad, npad, npad2, ctx->stream));
                HIP_TRY(ctx, launch_repitch_words(T.t[T.cur].as<uint64_t>() + r_src * nw, J.dst_t + r_dst * nw2, rows, nw, nw,
                                                  nw2, ctx->stream));
                HIP_TRY(ctx, launch_repitch_words(T.y[T.cur].as<uint64_t>() + r_src * nw, J.dst_y + r_dst * nw2, rows, nw, nw,
                                                  nw2, ctx->stream));
                moved += rows * (npad * 16 + 2 * nw * 8);
                k0 = k1;
            }
        }
        HIP_TRY(ctx, hipEventRecord(ev[5], ctx->stream));
        HIP_TRY(ctx, hipEventRecord(ev[6], ctx->stream));
        HIP_TRY(ctx, launch_join_paths(a, x, std::max(ctx->grid, 1), ctx->stream));
        HIP_TRY(ctx, hipEventRecord(ev[7], ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(grow ? valid2.p : ctx->valid.p, v.data(), nw2 * 8, hipMemcpyHostToDevice, ctx->stream));
        return FHH_OK;
    };
    rc = walk();
    if (rc) {
        (void)hipStreamSynchronize(ctx->stream);
        return rc;
    }
    rc = ctx_sync(ctx);   // `v` is read, and the old buffers are, until here
    if (rc) return rc;

    // 3. the ctx becomes the collection of n + m clients (host only: cannot fail)
    if (grow) {
        ctx->cw_seed.swap(cs);
        ctx->cw_bits.swap(cb);
        ctx->root_seed.swap(rs);
        ctx->key_idx.swap(ki);
        ctx->valid.swap(valid2);
        for (uint32_t j = 0; j < d; j++) {
            DimTable& T = ctx->tab[j];
            T.seed[T.cur].swap(seed2[j]);
            T.t[T.cur].swap(t2[j]);
            T.y[T.cur].swap(y2[j]);
            T.cap[T.cur] = cap2[j];
            for (size_t k = 0; k < T.live.size(); k++) T.live[k] = (uint32_t)k;   // the entries are dense now
            // the other buffer has the old stride: released, the next crawl's table_ensure sizes it by the new one
            const int o = 1 - T.cur;
            T.seed[o].release();
            T.t[o].release();
            T.y[o].release();
            T.cap[o] = 0;
        }
        ctx->nw = nw2;
        ctx->npad = npad2;
    }
    ctx->n = n2;
    ctx->reserved = 0;
    ctx->stats.aes_blocks += plan.aes_blocks;
    float ms[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i = 0; i < 4; i++) (void)hipEventElapsedTime(&ms[i], ev[2 * i], ev[2 * i + 1]);
    ctx->join_ms[0] = grow ? (double)ms[0] + ms[2] : 0.0;
    ctx->join_ms[1] = ms[1];
    ctx->join_ms[2] = ms[3];
    ctx->join_bytes = 2 * moved;
    return FHH_OK;   // the old buffers leave with this frame
}

}  // namespace eng
}  // namespace fhh

extern "C" {

int fhh_join_plan(uint32_t n_dims, uint32_t depth, uint64_t n, uint64_t m, const uint32_t* n_unique, uint64_t grid_blocks,
                  uint64_t* first_word, uint64_t* first_mask, uint64_t* words, uint64_t* new_nw, uint64_t* items,
                  uint64_t* waves, uint64_t* trips, uint64_t* last_trip_items, uint64_t* aes_blocks) {
    bool ok = n_dims >= 1 && n_dims <= (uint32_t)kMaxDims && n_unique && m != 0 && n != 0 && grid_blocks != 0 &&
              join_count_fits(n, m);
    for (uint32_t j = 0; ok && j < n_dims; j++) ok = n_unique[j] != 0;
    if (!ok) {
        g_err = "join_plan: m = 0, n = 0, n + m >= 2^32 - 1, n_dims outside 1..4, a zero n_unique or grid_blocks = 0";
        return FHH_E_ARG;
    }
    const JoinPlan p = join_plan(n_dims, depth, n, m, n_unique, grid_blocks);
    if (first_word) *first_word = p.first_word;
    if (first_mask) *first_mask = p.first_mask;
    if (words) *words = p.words;
    if (new_nw) *new_nw = p.new_nw;
    if (items) *items = p.items;
    if (waves) *waves = p.waves;
    if (trips) *trips = p.trips;
    if (last_trip_items) *last_trip_items = p.last_trip_items;
    if (aes_blocks) *aes_blocks = p.aes_blocks;
    return FHH_OK;
}

int fhh_join_timing(const fhh_ctx* ctx, double* ms, uint64_t* bytes) {
    CTX_CHECK(ctx);
    for (int i = 0; ms && i < 3; i++) ms[i] = ctx->join_ms[i];
    if (bytes) bytes[0] = ctx->join_bytes;
    return FHH_OK;
}

int fhh_join_clients_bincode(fhh_ctx* ctx, const uint8_t* req, uint64_t len) {
    CTX_CHECK(ctx);
    if (ctx->group) return group_join_clients_bincode(ctx, req, len);
    // every refusal comes before the ctx is touched
    int rc = join_check_state(ctx);
    if (rc) return rc;
    uint64_t m = 0;
    rc = join_parse(ctx, req, len, &m);
    if (rc) return rc;
    return join_one(ctx, m, req + 8);
}

}  // extern "C"
