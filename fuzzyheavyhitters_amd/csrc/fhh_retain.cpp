// fhh_retain_clients: the reference's apply_sketch_results (src/main.rs:68-69) — the clients a keep mask drops
// leave the collection. The survivors are gathered, in their old order, into buffers of the smaller
// collection's exact layout (fhh_retain.hip) and the ctx swaps to them: afterwards it is a collection of n'
// clients, so no later kernel reads a flag or works for a dropped client.
#include "fhh_engine.h"

#include <algorithm>
#include <cstring>

namespace fhh {
namespace eng {

bool retain_plan(const uint8_t* keep, uint64_t n, std::vector<uint32_t>& src, std::string* err) {
    auto refuse = [&](const std::string& m) {
        if (err) *err = m;
        return false;
    };
    if (!keep) return refuse("NULL keep");
    if (n == 0) return refuse("n = 0: no client to retain");
    if (n >> 32) return refuse("n does not fit the engine's u32 client indices");
    src.clear();
    src.reserve(n);
    for (uint64_t i = 0; i < n; i++) {
        if (keep[i] > 1) return refuse("keep byte " + std::to_string(i) + " is " + std::to_string(keep[i]) + ", not 0 or 1");
        if (keep[i]) src.push_back((uint32_t)i);
    }
    if (src.empty()) return refuse("no survivor: a collection of zero clients has no layout (fhh_reset instead)");
    return true;
}

int retain_check_state(fhh_ctx* ctx) {
    if (ctx->phase == Phase::kPending || ctx->phase == Phase::kPendingLast)
        return ctx->fail(FHH_E_STATE, "retain_clients: a crawl's children are pending (prune first)");
    if (!ctx->dev_keys && ctx->h_n == 0) return ctx->fail(FHH_E_STATE, "retain_clients: the ctx holds no keys");
    // `appended` outlives fhh_tree_init; the capacity layout does not (finish_appended): only that is refused
    if (ctx->dev_keys && ctx->appended && ctx->phase == Phase::kNoInit)
        return ctx->fail(FHH_E_STATE, "retain_clients: appended batches not yet finished by fhh_tree_init");
    return FHH_OK;
}

void retain_host_keys(const fhh_ctx* ctx, const uint32_t* src, uint64_t n2, RetainStage& st) {
    const size_t K = ctx->K, L = ctx->L;
    const size_t rec[4] = {K, K * 16, K * L * 16, K * L};
    const std::vector<uint8_t>* from[4] = {&ctx->h_key_idx, &ctx->h_root, &ctx->h_cws, &ctx->h_cwb};
    std::vector<uint8_t>* to[4] = {&st.h_key_idx, &st.h_root, &st.h_cws, &st.h_cwb};
    for (int a = 0; a < 4; a++) {
        to[a]->resize(n2 * rec[a]);
        for (uint64_t k = 0; k < n2; k++) std::memcpy(to[a]->data() + k * rec[a], from[a]->data() + (size_t)src[k] * rec[a], rec[a]);
    }
    st.n2 = n2;
    st.device = false;
}

int retain_prepare(fhh_ctx* ctx, const uint32_t* src, uint64_t n2, RetainStage& st) {
    if (!ctx->dev_keys) {
        retain_host_keys(ctx, src, n2, st);
        return FHH_OK;
    }
    int rc = ctx_set_device(ctx);
    if (rc) return rc;
    const size_t K = ctx->K, L = ctx->L, d = ctx->d;
    const uint64_t nw = ctx->nw, npad = ctx->npad;
    st.device = true;
    st.tables = ctx->phase == Phase::kFrontier;
    st.n2 = n2;
    st.nw2 = (n2 + 63) / 64;
    st.npad2 = st.nw2 * 64;
    const uint64_t nw2 = st.nw2, npad2 = st.npad2;
    // [src | dim 0's rows | ...]: a table's destination row 2 k + s is row 2 live[k] + s of buffer `cur`
    std::vector<uint32_t> lists(src, src + n2);
    size_t rows_off[kMaxDims] = {};
    for (size_t j = 0; st.tables && j < d; j++) {
        rows_off[j] = lists.size();
        for (uint32_t e : ctx->tab[j].live) {
            lists.push_back(2 * e);
            lists.push_back(2 * e + 1);
        }
    }
    // every destination before the first launch: a refusal for memory leaves nothing half done
    HIP_TRY(ctx, st.cw_seed.ensure(L * K * npad2 * 16));
    HIP_TRY(ctx, st.cw_bits.ensure(L * K * 4 * nw2 * 8));
    HIP_TRY(ctx, st.root_seed.ensure(K * npad2 * 16));
    HIP_TRY(ctx, st.key_idx.ensure(K * nw2 * 8));
    HIP_TRY(ctx, st.valid.ensure(nw2 * 8));
    HIP_TRY(ctx, st.lists.ensure(lists.size() * 4));
    for (size_t j = 0; st.tables && j < d; j++) {
        st.cap[j] = std::max<size_t>(ctx->tab[j].live.size(), 4);   // table_ensure's floor
        HIP_TRY(ctx, st.seed[j].ensure(st.cap[j] * 2 * npad2 * 16));
        HIP_TRY(ctx, st.t[j].ensure(st.cap[j] * 2 * nw2 * 8));
        HIP_TRY(ctx, st.y[j].ensure(st.cap[j] * 2 * nw2 * 8));
    }
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    struct EvGuard {
        hipEvent_t* e;
        ~EvGuard() {
            for (int i = 0; i < 3; i++)
                if (e[i]) (void)hipEventDestroy(e[i]);
        }
    } guard{ev};
    for (auto& e : ev) HIP_TRY(ctx, hipEventCreate(&e));
    std::vector<uint64_t> v(nw2, ~0ull);
    if (n2 % 64) v[nw2 - 1] = (1ull << (n2 % 64)) - 1;
    // from the first copy on, a failure drains the stream before `lists`, `v` and the stage's buffers go
    uint64_t col_rows = 0, plane_rows = 0;
    auto enqueue = [&]() -> int {
        HIP_TRY(ctx, hipMemcpyAsync(st.valid.p, v.data(), nw2 * 8, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(st.lists.p, lists.data(), lists.size() * 4, hipMemcpyHostToDevice, ctx->stream));
        const uint32_t* idx = st.lists.as<uint32_t>();
        const uint32_t m = (uint32_t)n2;
        HIP_TRY(ctx, hipEventRecord(ev[0], ctx->stream));
        HIP_TRY(ctx, launch_retain_cols(ctx->cw_seed.as<uint4>(), st.cw_seed.as<uint4>(), idx, nullptr, L * K, npad, npad2,
                                        m, ctx->stream));
        HIP_TRY(ctx, launch_retain_cols(ctx->root_seed.as<uint4>(), st.root_seed.as<uint4>(), idx, nullptr, K, npad, npad2,
                                        m, ctx->stream));
        col_rows += L * K + K;
        for (size_t j = 0; st.tables && j < d; j++) {
            const DimTable& T = ctx->tab[j];
            const uint64_t rows = 2 * T.live.size();
            HIP_TRY(ctx, launch_retain_cols(T.seed[T.cur].as<uint4>(), st.seed[j].as<uint4>(), idx, idx + rows_off[j], rows,
                                            npad, npad2, m, ctx->stream));
            col_rows += rows;
        }
        HIP_TRY(ctx, hipEventRecord(ev[1], ctx->stream));
        HIP_TRY(ctx, launch_retain_planes(ctx->cw_bits.as<uint64_t>(), st.cw_bits.as<uint64_t>(), idx, nullptr, L * K * 4, nw,
                                          nw2, m, ctx->stream));
        HIP_TRY(ctx, launch_retain_planes(ctx->key_idx.as<uint64_t>(), st.key_idx.as<uint64_t>(), idx, nullptr, K, nw, nw2, m,
                                          ctx->stream));
        plane_rows += L * K * 4 + K;
        for (size_t j = 0; st.tables && j < d; j++) {
            const DimTable& T = ctx->tab[j];
            const uint64_t rows = 2 * T.live.size();
            HIP_TRY(ctx, launch_retain_planes(T.t[T.cur].as<uint64_t>(), st.t[j].as<uint64_t>(), idx, idx + rows_off[j], rows,
                                              nw, nw2, m, ctx->stream));
            HIP_TRY(ctx, launch_retain_planes(T.y[T.cur].as<uint64_t>(), st.y[j].as<uint64_t>(), idx, idx + rows_off[j], rows,
                                              nw, nw2, m, ctx->stream));
            plane_rows += 2 * rows;
        }
        HIP_TRY(ctx, hipEventRecord(ev[2], ctx->stream));
        return FHH_OK;
    };
    rc = enqueue();
    if (rc) {
        (void)hipStreamSynchronize(ctx->stream);
        return rc;
    }
    rc = ctx_sync(ctx);   // `lists` and `v` are read until here
    if (rc) return rc;
    float a = 0.f, b = 0.f;
    (void)hipEventElapsedTime(&a, ev[0], ev[1]);
    (void)hipEventElapsedTime(&b, ev[1], ev[2]);
    st.ms[0] = a;
    st.ms[1] = b;
    // read n' columns and write npad' of 16 B per row; read (at least) and write nw' words per plane row
    st.bytes[0] = col_rows * (n2 + npad2) * 16;
    st.bytes[1] = plane_rows * 2 * nw2 * 8;
    return FHH_OK;
}

void retain_commit(fhh_ctx* ctx, RetainStage& st) {
    if (!st.device) {
        ctx->h_key_idx.swap(st.h_key_idx);
        ctx->h_root.swap(st.h_root);
        ctx->h_cws.swap(st.h_cws);
        ctx->h_cwb.swap(st.h_cwb);
        ctx->h_n = st.n2;
        return;
    }
    ctx->cw_seed.swap(st.cw_seed);
    ctx->cw_bits.swap(st.cw_bits);
    ctx->root_seed.swap(st.root_seed);
    ctx->key_idx.swap(st.key_idx);
    ctx->valid.swap(st.valid);
    ctx->n = st.n2;
    ctx->nw = st.nw2;
    ctx->npad = st.npad2;
    ctx->reserved = 0;
    for (uint32_t j = 0; j < ctx->d; j++) {
        DimTable& T = ctx->tab[j];
        if (!st.tables) {
            // before tree_init: nothing to keep; entries are sized by npad, so the tables are sized afresh
            T.cap[0] = T.cap[1] = 0;
            continue;
        }
        T.seed[T.cur].swap(st.seed[j]);
        T.t[T.cur].swap(st.t[j]);
        T.y[T.cur].swap(st.y[j]);
        T.cap[T.cur] = st.cap[j];
        for (size_t k = 0; k < T.live.size(); k++) T.live[k] = (uint32_t)k;   // the entries are dense now
        // the other buffer has the old stride: released, the next crawl's table_ensure sizes it by npad'
        const int o = 1 - T.cur;
        T.seed[o].release();
        T.t[o].release();
        T.y[o].release();
        T.cap[o] = 0;
    }
    for (int i = 0; i < 2; i++) {
        ctx->retain_ms[i] = st.ms[i];
        ctx->retain_bytes[i] = st.bytes[i];
    }
    // the old buffers leave with `st`
}

}  // namespace eng
}  // namespace fhh

extern "C" {

int fhh_retain_plan(const uint8_t* keep, uint64_t n, uint64_t* n_kept, uint32_t* src) {
    std::vector<uint32_t> s;
    std::string why;
    if (!retain_plan(keep, n, s, &why)) {
        g_err = "retain_plan: " + why;
        return FHH_E_ARG;
    }
    if (n_kept) *n_kept = s.size();
    if (src) std::memcpy(src, s.data(), s.size() * 4);
    return FHH_OK;
}

int fhh_retain_clients(fhh_ctx* ctx, const uint8_t* keep, uint64_t n) {
    CTX_CHECK(ctx);
    if (ctx->group) return group_retain_clients(ctx, keep, n);
    // every refusal comes before the ctx is touched
    int rc = retain_check_state(ctx);
    if (rc) return rc;
    std::vector<uint32_t> src;
    std::string why;
    if (!retain_plan(keep, n, src, &why)) return ctx->fail(FHH_E_ARG, "retain_clients: " + why);
    const uint64_t have = ctx->dev_keys ? ctx->n : ctx->h_n;
    if (n != have)
        return ctx->fail(FHH_E_ARG, "retain_clients: keep.len() " + std::to_string(n) + " != " + std::to_string(have) +
                                        " clients");
    if (src.size() == n) return FHH_OK;   // nobody leaves: the device is not touched
    RetainStage st;
    rc = retain_prepare(ctx, src.data(), src.size(), st);
    if (rc) return rc;
    retain_commit(ctx, st);
    return FHH_OK;
}

int fhh_retain_timing(const fhh_ctx* ctx, double* ms, uint64_t* bytes) {
    CTX_CHECK(ctx);
    for (int i = 0; i < 2; i++) {   // a multi-device ctx: the slowest shard's times, the shards' bytes summed
        if (ms) ms[i] = ctx->retain_ms[i];
        if (bytes) bytes[i] = ctx->retain_bytes[i];
    }
    return FHH_OK;
}

}  // extern "C"
