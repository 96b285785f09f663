// Host engine of the MI355X evaluator: one fhh_ctx = one server's
// `KeyCollection<FE, FieldElm>` (src/collect.rs:28-1030) bound to one GPU, exposed through
// the C ABI declared in include/fhh.h.
//
// The frontier of the reference is a Vec<TreeNode> whose nodes carry every client's d
// (left, right) EvalStates (collect.rs:18-22). Here a node is a tuple of d indices into
// per-dim prefix tables that live on the GPU (fhh_internal.h); pruning edits index lists
// on the host and never moves state (the reference does O(F) Vec::remove of whole nodes,
// collect.rs:918-929).
#include "fhh_engine.h"

#include <algorithm>
#include <cstdio>
#include <cstring>

thread_local std::string fhh::eng::g_err;

namespace {

constexpr int kDefaultVariant = 52;  // 4 tables, 128 KiB, 1024 thr, dynamic items (first one static, multi-word on narrow levels), <= 16 entries per item, nontemporal parent-seed loads and child-seed stores, sibling-pair AES (r02b A/Bs vs 34, 51)

// ---- timing -------------------------------------------------------------------------------
// call after the stream is synchronised
void timing_resolve(fhh_ctx* ctx) {
    for (auto& pr : ctx->ev_pending) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, ctx->ev_pool[pr.first].first, ctx->ev_pool[pr.first].second) != hipSuccess)
            continue;
        if (pr.second == kAllreduceTag) {
            ctx->stats.allreduce_ms += ms;
            ctx->stats.allreduce_timed++;
        } else if (pr.second == kGcotTag) {
            ctx->stats.gcot_ms += ms;
            ctx->stats.gcot_timed++;
        } else {
            ctx->stats.expand_ms += ms;
            ctx->stats.expand_blocks_timed += pr.second;
            ctx->stats.expand_launches_timed++;
        }
    }
    ctx->ev_pending.clear();
    ctx->ev_next = 0;
}

// pinned host staging that stays valid until the next ctx_sync(ctx)
void* stage_bytes(fhh_ctx* ctx, size_t bytes) {
    if (ctx->stage_used >= ctx->stage.size()) ctx->stage.push_back(new PinnedBuf());
    PinnedBuf* b = ctx->stage[ctx->stage_used];
    if (b->ensure(bytes) != hipSuccess) return nullptr;
    ctx->stage_used++;
    return b->p;
}

// ---- device key / table management -----------------------------------------------------------
int upload_staged_keys(fhh_ctx* ctx) {
    if (ctx->h_n == 0) return FHH_OK;
    if (ctx->dev_keys) return ctx->fail(FHH_E_STATE, "cannot mix add_keys with device-generated keys");
    int rc = alloc_keys(ctx, ctx->h_n);
    if (rc) return rc;
    const size_t K = ctx->K, L = ctx->L, n = ctx->h_n;
    DevBuf a, b, c, dd;
    HIP_TRY(ctx, a.ensure(n * K));
    HIP_TRY(ctx, b.ensure(n * K * 16));
    HIP_TRY(ctx, c.ensure(n * K * L * 16));
    HIP_TRY(ctx, dd.ensure(n * K * L));
    HIP_TRY(ctx, hipMemcpyAsync(a.p, ctx->h_key_idx.data(), n * K, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(b.p, ctx->h_root.data(), n * K * 16, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(c.p, ctx->h_cws.data(), n * K * L * 16, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(dd.p, ctx->h_cwb.data(), n * K * L, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, launch_keys_from_aos(a.as<uint8_t>(), b.as<uint8_t>(), c.as<uint8_t>(), dd.as<uint8_t>(), n,
                                      ctx->K, ctx->L, (uint32_t)ctx->npad, (uint32_t)ctx->nw, ctx->cw_seed.as<uint4>(),
                                      ctx->cw_bits.as<uint64_t>(), ctx->root_seed.as<uint4>(),
                                      ctx->key_idx.as<uint64_t>(), ctx->stream));
    rc = ctx_sync(ctx);
    if (rc) return rc;
    ctx->dev_keys = true;
    ctx->h_key_idx.clear();
    ctx->h_root.clear();
    ctx->h_cws.clear();
    ctx->h_cwb.clear();
    ctx->h_key_idx.shrink_to_fit();
    ctx->h_root.shrink_to_fit();
    ctx->h_cws.shrink_to_fit();
    ctx->h_cwb.shrink_to_fit();
    ctx->h_n = 0;
    return FHH_OK;
}

int table_ensure(fhh_ctx* ctx, DimTable& T, int buf, size_t entries) {
    if (entries <= T.cap[buf] && T.seed[buf].p) return FHH_OK;
    size_t cap = std::max<size_t>(entries, T.cap[buf] * 2);
    cap = std::max<size_t>(cap, 4);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (T.seed[buf].ensure(cap * 2 * ctx->npad * 16) != hipSuccess) {
        // the doubling does not fit (32 MB per entry at 1M clients): exactly what is needed
        (void)hipGetLastError();
        cap = std::max<size_t>(entries, 4);
        HIP_TRY(ctx, T.seed[buf].ensure(cap * 2 * ctx->npad * 16));
    }
    HIP_TRY(ctx, T.t[buf].ensure(cap * 2 * ctx->nw * 8));
    HIP_TRY(ctx, T.y[buf].ensure(cap * 2 * ctx->nw * 8));
    T.cap[buf] = cap;
    return FHH_OK;
}

int upload_u32(fhh_ctx* ctx, DevBuf& dst, const std::vector<uint32_t>& v) {
    const size_t bytes = std::max<size_t>(v.size() * 4, 4);
    if (dst.bytes < bytes) {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        HIP_TRY(ctx, dst.ensure(bytes * 2));
    }
    if (!v.empty()) {
        void* h = stage_bytes(ctx, v.size() * 4);
        if (!h) return ctx->fail(FHH_E_NOMEM, "pinned staging allocation failed");
        std::memcpy(h, v.data(), v.size() * 4);
        HIP_TRY(ctx, hipMemcpyAsync(dst.p, h, v.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    }
    return FHH_OK;
}

// One H2D copy per crawl: [live_0 | ... | live_{d-1} | parent_pos[F][d]] (u32).
int upload_lists(fhh_ctx* ctx) {
    std::vector<uint32_t> v;
    size_t off[kMaxDims + 1];
    for (uint32_t j = 0; j < ctx->d; j++) {
        off[j] = v.size();
        v.insert(v.end(), ctx->tab[j].live.begin(), ctx->tab[j].live.end());
    }
    off[ctx->d] = v.size();
    for (const Node& nd : ctx->frontier)
        for (uint32_t j = 0; j < ctx->d; j++) v.push_back(nd.pos[j]);
    int rc = upload_u32(ctx, ctx->lists, v);
    if (rc) return rc;
    const uint32_t* base = ctx->lists.as<uint32_t>();
    for (uint32_t j = 0; j < ctx->d; j++) ctx->live_ptr[j] = base + off[j];
    ctx->parent_pos_ptr = base + off[ctx->d];
    return FHH_OK;
}

// Prepare expansion jobs for one ctx (dst buffers sized; lists already on the device).
int prepare_expand(fhh_ctx* ctx, ExpandJob* jobs, uint32_t* njobs) {
    for (uint32_t j = 0; j < ctx->d; j++) {
        DimTable& T = ctx->tab[j];
        const int src = T.cur, dst = 1 - T.cur;
        int rc = table_ensure(ctx, T, dst, 2 * T.live.size());
        if (rc) return rc;
        ExpandJob& J = jobs[(*njobs)++];
        J.cw_seed = ctx->cw_seed.as<uint4>();
        J.cw_bits = ctx->cw_bits.as<uint64_t>();
        J.src_seed = T.seed[src].as<uint4>();
        J.src_t = T.t[src].as<uint64_t>();
        J.src_y = T.y[src].as<uint64_t>();
        J.dst_seed = T.seed[dst].as<uint4>();
        J.dst_t = T.t[dst].as<uint64_t>();
        J.dst_y = T.y[dst].as<uint64_t>();
        J.live = ctx->live_ptr[j];
        J.n_live = (uint32_t)T.live.size();
        J.level = ctx->level;
        J.dim = j;
        J.K = ctx->K;
        J.npad = (uint32_t)ctx->npad;
        J.nw = (uint32_t)ctx->nw;
        J.group = 1;
        J.item_begin = 0;
    }
    return FHH_OK;
}

void finalize_launch(ExpandLaunch& L, int grid, int variant) {
    // every job of a launch has the same client count (both servers hold the same clients)
    const uint64_t waves = (uint64_t)grid * (expand_threads(variant) / 64);
    uint32_t n_live[kMaxJobs] = {};
    for (uint32_t k = 0; k < L.njobs; k++) n_live[k] = L.job[k].n_live;
    ItemLayout lay;
    item_layout(n_live, L.njobs, L.job[0].nw, expand_max_group(variant), waves, lay, expand_max_wpi(variant));
    L.wpi = lay.wpi;
    for (uint32_t k = 0; k < L.njobs; k++) {
        L.job[k].group = lay.g;
        L.job[k].item_begin = lay.begin[k];
    }
    L.total_items = lay.total;
}

uint64_t launch_blocks(const fhh_ctx* ctx) {
    uint64_t b = 0;
    for (uint32_t j = 0; j < ctx->d; j++) b += (uint64_t)ctx->tab[j].live.size() * 4 * ctx->n;
    return b;
}

// Record the children created by an expansion of ctx's frontier.
int post_expand(fhh_ctx* ctx, bool last) {
    const uint64_t F = ctx->frontier.size();
    ctx->pending_C = F << ctx->d;
    for (uint32_t j = 0; j < ctx->d; j++) {
        DimTable& T = ctx->tab[j];
        ctx->child_buf[j] = 1 - T.cur;
        if (!last) T.cur = 1 - T.cur;     // tree_crawl: next_frontier replaces frontier
    }
    ctx->stats.aes_blocks += launch_blocks(ctx);
    ctx->stats.ref_evals += ctx->pending_C * ctx->n * 2 * ctx->d;
    ctx->stats.levels += 1;
    if (last) {
        ctx->phase = Phase::kPendingLast;
        ctx->last_nodes.clear();
        for (uint64_t c = 0; c < ctx->pending_C; c++)
            ctx->last_nodes.emplace_back((uint32_t)(c >> ctx->d), (uint32_t)(c & ((1u << ctx->d) - 1)));
        ctx->last_values.assign(ctx->pending_C, Limbs10{});
        ctx->last_depth = ctx->level + 1;
        ctx->last_hist = ctx->hist;
    } else {
        ctx->phase = Phase::kPending;
    }
    return FHH_OK;
}

int check_can_crawl(fhh_ctx* ctx) {
    if (ctx->phase == Phase::kNoInit) return ctx->fail(FHH_E_STATE, "tree_crawl before tree_init");
    if (ctx->phase == Phase::kPending) {
        // the unpruned children become the frontier (collect.rs:505 `self.frontier = next_frontier`)
        std::vector<uint8_t> all(ctx->pending_C, 1);
        int rc = prune_impl(ctx, all.data(), ctx->pending_C);
        if (rc) return rc;
    }
    if (ctx->level >= ctx->L) return ctx->fail(FHH_E_STATE, "crawl past data_len (cor_words index out of bounds)");
    return FHH_OK;
}

int crawl_one(fhh_ctx* ctx, bool last) {
    int rc = check_can_crawl(ctx);
    if (rc) return rc;
    rc = upload_lists(ctx);
    if (rc) return rc;
    ExpandLaunch La{};
    La.njobs = 0;
    rc = prepare_expand(ctx, La.job, &La.njobs);
    if (rc) return rc;
    finalize_launch(La, ctx->grid, ctx->variant);
    size_t slot = 0;
    if (ctx->timing) HIP_TRY(ctx, timing_begin(ctx, &slot));
    HIP_TRY(ctx, launch_expand(La, ctx->variant, ctx->grid, ctx->work_counter.as<uint32_t>(), &ctx->expand_seq, ctx->stream));
    if (ctx->timing) HIP_TRY(ctx, timing_end(ctx, slot, launch_blocks(ctx)));
    ctx->stats.expand_launches++;
    return post_expand(ctx, last);
}

// path of a frontier node at depth `depth` (hist[0..depth-1]) followed by (p, i)
void node_path(const std::vector<std::vector<std::pair<uint32_t, uint32_t>>>& hist, uint32_t depth, uint32_t p,
               uint32_t i, uint32_t d, uint8_t* out /*[d][depth+1]*/) {
    const uint32_t len = depth + 1;
    for (uint32_t j = 0; j < d; j++) out[j * len + depth] = (uint8_t)((i >> j) & 1);
    uint32_t node = p;
    for (int64_t lv = (int64_t)depth - 1; lv >= 0; lv--) {
        const auto& pr = hist[(size_t)lv][node];
        for (uint32_t j = 0; j < d; j++) out[j * len + (uint32_t)lv] = (uint8_t)((pr.second >> j) & 1);
        node = pr.first;
    }
}

}  // namespace

namespace fhh {
namespace eng {

hipError_t timing_begin(fhh_ctx* ctx, size_t* slot) {
    if (ctx->ev_next >= ctx->ev_pool.size()) {
        hipEvent_t a, b;
        hipError_t e = hipEventCreate(&a);
        if (e != hipSuccess) return e;
        e = hipEventCreate(&b);
        if (e != hipSuccess) return e;
        ctx->ev_pool.emplace_back(a, b);
    }
    *slot = ctx->ev_next++;
    return hipEventRecord(ctx->ev_pool[*slot].first, ctx->stream);
}

hipError_t timing_end(fhh_ctx* ctx, size_t slot, uint64_t blocks) {
    ctx->ev_pending.emplace_back(slot, blocks);
    return hipEventRecord(ctx->ev_pool[slot].second, ctx->stream);
}

int ctx_sync(fhh_ctx* ctx) {
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    timing_resolve(ctx);
    ctx->stage_used = 0;
    if (ctx->peer) {
        timing_resolve(ctx->peer);
        ctx->peer->stage_used = 0;
    }
    return FHH_OK;
}

int ctx_set_device(fhh_ctx* ctx) {
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return FHH_OK;
}

int upload_staged(fhh_ctx* ctx) { return upload_staged_keys(ctx); }

int alloc_keys(fhh_ctx* ctx, uint64_t n) {
    ctx->appended = false;   // a one-shot layout replaces an unused reservation
    ctx->reserved = 0;
    ctx->n = n;
    ctx->nw = (n + 63) / 64;
    if (ctx->nw == 0) ctx->nw = 1;
    ctx->npad = ctx->nw * 64;
    const size_t K = ctx->K, L = ctx->L;
    HIP_TRY(ctx, ctx->cw_seed.ensure(L * K * ctx->npad * 16));
    HIP_TRY(ctx, ctx->cw_bits.ensure(L * K * 4 * ctx->nw * 8));
    HIP_TRY(ctx, ctx->root_seed.ensure(K * ctx->npad * 16));
    HIP_TRY(ctx, ctx->key_idx.ensure(K * ctx->nw * 8));
    HIP_TRY(ctx, ctx->valid.ensure(ctx->nw * 8));
    std::vector<uint64_t> v(ctx->nw, ~0ull);
    if (n % 64) v[ctx->nw - 1] = (1ull << (n % 64)) - 1;
    if (n == 0) v[0] = 0;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->valid.p, v.data(), ctx->nw * 8, hipMemcpyHostToDevice, ctx->stream));
    return ctx_sync(ctx);
}

// Both servers' expansions in ONE launch (same device): the in-process harness path.
int crawl_pair(fhh_ctx* c0, fhh_ctx* c1, bool last) {
    int rc = check_can_crawl(c0);
    if (rc) return rc;
    rc = check_can_crawl(c1);
    if (rc) return rc;
    if (c1->stream != c0->stream) HIP_TRY(c1, hipStreamSynchronize(c1->stream));
    // both servers prune with the same keep masks, so their frontiers and live lists are
    // identical: upload once and let server 1's jobs read server 0's copy
    if (c0->frontier.size() != c1->frontier.size()) return c0->fail(FHH_E_ARG, "pair: frontiers differ");
    for (uint32_t j = 0; j < c0->d; j++)
        if (c0->tab[j].live != c1->tab[j].live) return c0->fail(FHH_E_ARG, "pair: live lists differ");
    rc = upload_lists(c0);
    if (rc) return rc;
    for (uint32_t j = 0; j < c0->d; j++) c1->live_ptr[j] = c0->live_ptr[j];
    c1->parent_pos_ptr = c0->parent_pos_ptr;
    ExpandLaunch La{};
    La.njobs = 0;
    rc = prepare_expand(c0, La.job, &La.njobs);
    if (rc) return rc;
    rc = prepare_expand(c1, La.job, &La.njobs);
    if (rc) return rc;
    finalize_launch(La, c0->grid, c0->variant);
    size_t slot = 0;
    const uint64_t blocks = launch_blocks(c0) + launch_blocks(c1);
    if (c0->timing) HIP_TRY(c0, timing_begin(c0, &slot));
    HIP_TRY(c0, launch_expand(La, c0->variant, c0->grid, c0->work_counter.as<uint32_t>(), &c0->expand_seq, c0->stream));
    if (c0->timing) HIP_TRY(c0, timing_end(c0, slot, blocks));
    c0->stats.expand_launches++;
    rc = post_expand(c0, last);
    if (rc) return rc;
    return post_expand(c1, last);
}

ChildArgs child_args(fhh_ctx* c0, fhh_ctx* c1) {
    ChildArgs a{};
    for (uint32_t j = 0; j < c0->d; j++) {
        a.s0.t[j] = c0->tab[j].t[c0->child_buf[j]].as<uint64_t>();
        a.s0.y[j] = c0->tab[j].y[c0->child_buf[j]].as<uint64_t>();
        fhh_ctx* o = c1 ? c1 : c0;
        a.s1.t[j] = o->tab[j].t[o->child_buf[j]].as<uint64_t>();
        a.s1.y[j] = o->tab[j].y[o->child_buf[j]].as<uint64_t>();
    }
    a.parent_pos = c0->parent_pos_ptr;
    a.valid = c0->valid.as<uint64_t>();
    a.C = c0->pending_C;
    a.d = c0->d;
    a.nw = (uint32_t)c0->nw;
    a.client_base = c0->client_base;
    a.level = c0->level;
    a.n = (uint32_t)c0->n;
    return a;
}

int prune_impl(fhh_ctx* ctx, const uint8_t* keep, uint64_t n) {
    if (ctx->phase != Phase::kPending) return ctx->fail(FHH_E_STATE, "tree_prune without a pending tree_crawl");
    if (n != ctx->pending_C)
        return ctx->fail(FHH_E_ARG, "tree_prune: keep.len() != frontier.len() (collect.rs:919)");
    const uint32_t d = ctx->d;
    std::vector<Node> nf;
    std::vector<std::pair<uint32_t, uint32_t>> h;
    std::vector<std::vector<uint32_t>> new_live(d);
    // child entry e of dim j lies in [0, 2 * |live_j|): flat remap, first reference wins
    thread_local std::vector<int32_t> remap[kMaxDims];
    for (uint32_t j = 0; j < d; j++) remap[j].assign(2 * ctx->tab[j].live.size(), -1);
    nf.reserve(n);
    h.reserve(n);
    for (uint64_t c = 0; c < n; c++) {
        if (!keep[c]) continue;
        const uint32_t p = (uint32_t)(c >> d), i = (uint32_t)(c & ((1u << d) - 1));
        Node node{};
        for (uint32_t j = 0; j < d; j++) {
            const uint32_t e = 2 * ctx->frontier[p].pos[j] + ((i >> j) & 1);
            int32_t& r = remap[j][e];
            if (r < 0) {
                r = (int32_t)new_live[j].size();
                new_live[j].push_back(e);
            }
            node.pos[j] = (uint32_t)r;
        }
        nf.push_back(node);
        h.emplace_back(p, i);
    }
    for (uint32_t j = 0; j < d; j++) ctx->tab[j].live = std::move(new_live[j]);
    ctx->frontier = std::move(nf);
    ctx->hist.push_back(std::move(h));
    ctx->level += 1;
    ctx->pending_C = 0;
    ctx->phase = Phase::kFrontier;
    return FHH_OK;
}

ChildArgs ctx_child_args(fhh_ctx* ctx) { return child_args(ctx, nullptr); }

int crawl_level(fhh_ctx* ctx, bool last, uint64_t* n_children, uint64_t* planes, uint64_t pitch_words,
                uint64_t word_off) {
    int rc = crawl_one(ctx, last);
    if (rc) return rc;
    if (n_children) *n_children = ctx->pending_C;
    if (planes && ctx->pending_C) {
        // k_share_planes writes [C][2d][nw] on the device; one strided copy lands this ctx's words
        // in the caller's rows (the gather of a multi-device ctx costs no host pass)
        const size_t rows = ctx->pending_C * 2 * ctx->d;
        HIP_TRY(ctx, ctx->scratch.ensure(rows * ctx->nw * 8));
        ChildArgs a = ctx_child_args(ctx);
        HIP_TRY(ctx, launch_share_planes(a, ctx->scratch.as<uint64_t>(), ctx->stream));
        HIP_TRY(ctx, hipMemcpy2DAsync(planes + word_off, pitch_words * 8, ctx->scratch.p, ctx->nw * 8, ctx->nw * 8, rows,
                                      hipMemcpyDeviceToHost, ctx->stream));
    }
    return ctx_sync(ctx);
}

bool fmt_is_fe255(uint32_t fmt) { return fmt == FHH_VALS_FE255_LIMBS || fmt == FHH_VALS_FE255_BLOCKPAIR; }

static size_t fmt_bytes(uint32_t fmt) {
    return fmt == FHH_VALS_FE_U64 ? 8 : fmt == FHH_VALS_FE_BLOCK ? 16 : 32;
}

int node_partials(fhh_ctx* ctx, const void* vals, uint32_t fmt, uint64_t ld, uint64_t col0, bool host,
                  uint64_t** partials_dev) {
    if (ctx->phase != Phase::kPending && ctx->phase != Phase::kPendingLast)
        return ctx->fail(FHH_E_STATE, "node_sums without a pending crawl");
    if (fmt > FHH_VALS_FE255_BLOCKPAIR) return ctx->fail(FHH_E_ARG, "node_sums: unknown value format");
    const uint64_t C = ctx->pending_C, n = ctx->n;
    const size_t eb = fmt_bytes(fmt), per = fmt_is_fe255(fmt) ? 8 : 2;
    HIP_TRY(ctx, ctx->scratch2.ensure(std::max<uint64_t>(C, 1) * per * 8));
    *partials_dev = ctx->scratch2.as<uint64_t>();
    if (C == 0) return FHH_OK;
    if (!vals) return ctx->fail(FHH_E_ARG, "node_sums: NULL values");
    if (ld < col0 + n) return ctx->fail(FHH_E_ARG, "node_sums: row pitch shorter than the client count");
    const void* src = vals;
    uint64_t pitch = ld;
    if (host) {
        // this ctx's column block of the caller's [C][ld] rows, one strided host-to-device copy
        HIP_TRY(ctx, ctx->scratch.ensure(C * n * eb));
        HIP_TRY(ctx, hipMemcpy2DAsync(ctx->scratch.p, n * eb, static_cast<const uint8_t*>(vals) + col0 * eb, ld * eb,
                                      n * eb, C, hipMemcpyHostToDevice, ctx->stream));
        src = ctx->scratch.p;
        pitch = n;
    }
    HIP_TRY(ctx, launch_sum_vals(src, fmt, C, n, pitch, *partials_dev, ctx->stream));
    return FHH_OK;
}

int node_sums_finish(fhh_ctx* ctx, const uint64_t* h, uint32_t fmt, void* out_a, void* out_b) {
    const uint64_t C = ctx->pending_C;
    if (!fmt_is_fe255(fmt)) {
        uint64_t* sums = static_cast<uint64_t*>(out_a);   // NULL: a shard that only takes part
        if (!sums) return FHH_OK;
        for (uint64_t c = 0; c < C; c++) sums[c] = fe_canon_from_limbs(h[2 * c], h[2 * c + 1]);
        return FHH_OK;
    }
    uint32_t* unr = static_cast<uint32_t*>(out_a);
    uint32_t* can = static_cast<uint32_t*>(out_b);
    for (uint64_t c = 0; c < C; c++) {
        Limbs10 v = limbs_from_partials(&h[c * 8]);
        if (unr) std::memcpy(unr + c * 10, v.data(), 40);
        if (can) {
            auto r = ::fe255_reduce(v);
            std::memcpy(can + c * 8, r.data(), 32);
        }
        if (ctx->phase == Phase::kPendingLast) ctx->last_values[c] = v;
    }
    return FHH_OK;
}

// One trie walk per dim and one over whole nodes, level by level: a prefix's id at depth lv + 1 is the rank of
// its (id at depth lv, next direction) among those seen so far, so the ids at the last depth number the distinct
// prefixes in order of first appearance without hashing a path.
bool frontier_plan(uint32_t d, uint32_t depth, uint64_t n_nodes, const uint8_t* paths, FrontierPlan& plan,
                   std::string* err) {
    auto refuse = [&](const std::string& m) {
        if (err) *err = m;
        return false;
    };
    if (d < 1 || d > (uint32_t)kMaxDims) return refuse("n_dims must be in [1, " + std::to_string(kMaxDims) + "]");
    if (n_nodes == 0) return refuse("n_nodes = 0: a frontier holds at least one node");
    if (n_nodes >> (32 - d)) return refuse("n_nodes << n_dims does not fit the engine's u32 child indices");
    if (depth && !paths) return refuse("NULL paths with depth > 0");
    const size_t total = (size_t)n_nodes * d * depth;
    for (size_t k = 0; k < total; k++)
        if (paths[k] > 1)
            return refuse("paths byte " + std::to_string(k) + " is " + std::to_string(paths[k]) + ", not 0 or 1");
    if (depth == 0 && n_nodes > 1) return refuse("node 1 repeats the path of node 0 (the root)");

    const uint32_t F = (uint32_t)n_nodes;
    std::vector<uint32_t> cur(F);
    std::vector<int32_t> remap;
    // one level: every node's id (cur) at depth lv + 1 from its id at depth lv, one of `count`, and its next
    // direction(s) key(k) < 2^width; returns the count of distinct ids, on_new(k, parent, key) at each first
    // appearance
    auto step = [&](uint32_t width, uint32_t count, auto key, auto on_new) {
        remap.assign((size_t)count << width, -1);
        uint32_t next = 0;
        for (uint32_t k = 0; k < F; k++) {
            const uint32_t kv = key(k);
            int32_t& r = remap[((size_t)cur[k] << width) | kv];
            if (r < 0) {
                r = (int32_t)next++;
                on_new(k, cur[k], kv);
            }
            cur[k] = (uint32_t)r;
        }
        return next;
    };
    plan.n_unique.assign(d, 1);
    plan.pos.assign((size_t)F * d, 0);
    plan.rep.assign(d, {});
    for (uint32_t j = 0; j < d; j++) {
        std::fill(cur.begin(), cur.end(), 0u);
        uint32_t count = 1;
        for (uint32_t lv = 0; lv < depth; lv++)
            count = step(1, count, [&](uint32_t k) { return (uint32_t)paths[((size_t)k * d + j) * depth + lv]; },
                         [](uint32_t, uint32_t, uint32_t) {});
        plan.n_unique[j] = count;
        plan.rep[j].assign(count, ~0ull);
        for (uint32_t k = 0; k < F; k++) {
            plan.pos[(size_t)k * d + j] = cur[k];
            if (plan.rep[j][cur[k]] == ~0ull) plan.rep[j][cur[k]] = k;
        }
    }
    // whole nodes: the trie of the paths, row lv = the distinct nodes of depth lv + 1 as (parent, i)
    plan.hist.assign(depth, {});
    std::fill(cur.begin(), cur.end(), 0u);
    uint32_t count = 1;
    for (uint32_t lv = 0; lv < depth; lv++) {
        auto& row = plan.hist[lv];
        count = step(d, count,
                     [&](uint32_t k) {
                         uint32_t i = 0;
                         for (uint32_t j = 0; j < d; j++) i |= (uint32_t)paths[((size_t)k * d + j) * depth + lv] << j;
                         return i;
                     },
                     [&](uint32_t, uint32_t parent, uint32_t i) { row.emplace_back(parent, i); });
    }
    if (depth && count != F) {
        // the reference's frontier never holds a node twice; a second copy would be counted twice
        std::vector<int64_t> first(count, -1);
        for (uint32_t k = 0; k < F; k++) {
            if (first[cur[k]] >= 0)
                return refuse("node " + std::to_string(k) + " repeats the path of node " + std::to_string(first[cur[k]]));
            first[cur[k]] = k;
        }
    }
    return true;
}

int tree_init_at_planned(fhh_ctx* ctx, const FrontierPlan& plan, uint64_t n_nodes, uint32_t depth, const uint8_t* paths) {
    int rc = ctx_set_device(ctx);
    if (rc) return rc;
    rc = upload_staged_keys(ctx);
    if (rc) return rc;
    if (!ctx->dev_keys || ctx->n == 0) return ctx->fail(FHH_E_STATE, "tree_init_at with no keys (collect.rs:83)");
    if (ctx->appended) {
        rc = finish_appended(ctx);
        if (rc) return rc;
    }
    const uint32_t d = ctx->d, dir_words = (depth + 31) / 32;
    // the distinct prefixes' direction bits, every dim's in one upload: [dim][prefix][dir_words]
    std::vector<uint32_t> dirs;
    size_t dirs_off[kMaxDims] = {};
    for (uint32_t j = 0; j < d; j++) {
        dirs_off[j] = dirs.size();
        dirs.resize(dirs.size() + (size_t)plan.n_unique[j] * dir_words, 0u);
        for (uint32_t e = 0; e < plan.n_unique[j]; e++) {
            const uint8_t* p = paths + ((size_t)plan.rep[j][e] * d + j) * depth;
            uint32_t* w = dirs.data() + dirs_off[j] + (size_t)e * dir_words;
            for (uint32_t l = 0; l < depth; l++) w[l >> 5] |= (uint32_t)p[l] << (l & 31);
        }
    }
    rc = upload_u32(ctx, ctx->lists, dirs);   // (the next crawl's upload_lists reuses the buffer: this call drains the stream)
    if (rc) return rc;
    EvalPathsArgs a{};
    a.cw_seed = ctx->cw_seed.as<uint4>();
    a.cw_bits = ctx->cw_bits.as<uint64_t>();
    a.root_seed = ctx->root_seed.as<uint4>();
    a.key_idx = ctx->key_idx.as<uint64_t>();
    a.d = d;
    a.K = ctx->K;
    a.npad = (uint32_t)ctx->npad;
    a.nw = (uint32_t)ctx->nw;
    a.depth = depth;
    a.dir_words = dir_words;
    uint64_t entries = 0;
    for (uint32_t j = 0; j < d; j++) {
        DimTable& T = ctx->tab[j];
        T.cur = 0;
        rc = table_ensure(ctx, T, 0, plan.n_unique[j]);
        if (rc) return rc;
        EvalPathsJob& J = a.job[j];
        J.dst_seed = T.seed[0].as<uint4>();
        J.dst_t = T.t[0].as<uint64_t>();
        J.dst_y = T.y[0].as<uint64_t>();
        J.dirs = ctx->lists.as<uint32_t>() + dirs_off[j];
        J.n_prefixes = plan.n_unique[j];
        J.item_begin = a.total_items;
        a.total_items += (uint64_t)2 * ctx->nw * ((plan.n_unique[j] + kEvalPathsP - 1) / kEvalPathsP);
        entries += plan.n_unique[j];
    }
    HIP_TRY(ctx, launch_eval_paths(a, ctx->grid, ctx->stream));
    for (uint32_t j = 0; j < d; j++) {
        ctx->tab[j].live.resize(plan.n_unique[j]);
        for (uint32_t e = 0; e < plan.n_unique[j]; e++) ctx->tab[j].live[e] = e;
    }
    ctx->frontier.assign(n_nodes, Node{});
    for (uint64_t k = 0; k < n_nodes; k++)
        for (uint32_t j = 0; j < d; j++) ctx->frontier[k].pos[j] = plan.pos[k * d + j];
    ctx->hist = plan.hist;
    ctx->last_nodes.clear();
    ctx->last_values.clear();
    ctx->last_hist.clear();
    ctx->level = depth;
    ctx->pending_C = 0;
    ctx->phase = Phase::kFrontier;
    ctx->stats.aes_blocks += (uint64_t)depth * 2 * entries * ctx->n;   // the blocks executed: one per (prefix, key, level)
    return ctx_sync(ctx);
}

}  // namespace eng
}  // namespace fhh

// ================================================================================================
// C ABI
// ================================================================================================
extern "C" {

const char* fhh_last_error(const fhh_ctx* ctx) { return ctx ? ctx->err.c_str() : g_err.c_str(); }

int fhh_create(fhh_ctx** out, uint32_t data_len, uint32_t n_dims, int device) {
    if (!out) {
        g_err = "fhh_create: out is NULL";
        return FHH_E_ARG;
    }
    *out = nullptr;
    if (n_dims < 1 || n_dims > FHH_MAX_DIMS) {
        g_err = "fhh_create: n_dims must be in [1, " + std::to_string(FHH_MAX_DIMS) + "]";
        return FHH_E_ARG;
    }
    if (data_len < 1) {
        g_err = "fhh_create: data_len must be >= 1";
        return FHH_E_ARG;
    }
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) {
        g_err = std::string("hipSetDevice: ") + hipGetErrorString(e);
        return FHH_E_HIP;
    }
    fhh_ctx* ctx = new fhh_ctx();
    ctx->device = device;
    ctx->L = data_len;
    ctx->d = n_dims;
    ctx->K = 2 * n_dims;
    e = hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking);
    ctx->stream = ctx->own_stream;
    if (e != hipSuccess) {
        g_err = std::string("hipStreamCreate: ") + hipGetErrorString(e);
        delete ctx;
        return FHH_E_HIP;
    }
    ctx->variant = kDefaultVariant;
    ctx->grid = expand_grid(device, ctx->variant);
    if (ctx->work_counter.ensure(kWorkCounterBytes) != hipSuccess ||
        hipMemset(ctx->work_counter.p, 0, kWorkCounterBytes) != hipSuccess) {
        g_err = "work counter allocation failed";
        (void)hipStreamDestroy(ctx->own_stream);
        delete ctx;
        return FHH_E_NOMEM;
    }
    *out = ctx;
    return FHH_OK;
}

void fhh_destroy(fhh_ctx* ctx) {
    if (!ctx) return;
    if (ctx->group) return group_destroy(ctx);
    if (ctx->party) party_destroy(ctx);
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    for (auto& pr : ctx->ev_pool) {
        (void)hipEventDestroy(pr.first);
        (void)hipEventDestroy(pr.second);
    }
    if (ctx->side_stream) {
        (void)hipStreamSynchronize(ctx->side_stream);
        (void)hipStreamDestroy(ctx->side_stream);
    }
    for (hipEvent_t e : ctx->side_ev)
        if (e) (void)hipEventDestroy(e);
    (void)hipStreamDestroy(ctx->own_stream);
    for (auto* b : ctx->stage) delete b;
    delete ctx;
}

int fhh_reset(fhh_ctx* ctx) {
    CTX_CHECK(ctx);
    if (ctx->group) return group_reset(ctx);
    int rc = ctx_set_device(ctx);
    if (rc) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->h_key_idx.clear();
    ctx->h_root.clear();
    ctx->h_cws.clear();
    ctx->h_cwb.clear();
    ctx->h_n = 0;
    ctx->dev_keys = false;
    ctx->appended = false;
    ctx->reserved = 0;
    ctx->n = ctx->npad = ctx->nw = 0;
    ctx->phase = Phase::kNoInit;
    ctx->frontier.clear();
    ctx->hist.clear();
    ctx->last_nodes.clear();
    ctx->last_values.clear();
    ctx->last_hist.clear();
    ctx->pending_C = 0;
    ctx->level = 0;
    ctx->party_server = -1;
    for (auto& T : ctx->tab) {
        T.live.clear();
        // entries are sized by npad: the next collection may be larger, so its tables are sized afresh (the
        // allocations themselves are kept and reused where they are large enough)
        T.cap[0] = T.cap[1] = 0;
    }
    return FHH_OK;
}

int fhh_set_client_base(fhh_ctx* ctx, uint64_t client_base) {
    CTX_CHECK(ctx);
    if (ctx->group) return group_set_client_base(ctx, client_base);
    ctx->client_base = client_base;
    return FHH_OK;
}

int fhh_add_keys(fhh_ctx* ctx, uint64_t n, const uint8_t* key_idx, const uint8_t* root_seed, const uint8_t* cw_seed,
                 const uint8_t* cw_bits) {
    CTX_CHECK(ctx);
    if (n == 0) return FHH_OK;
    if (!key_idx || !root_seed || !cw_seed || !cw_bits) return ctx->fail(FHH_E_ARG, "add_keys: NULL buffer");
    if (ctx->dev_keys) return ctx->fail(FHH_E_STATE, "add_keys after keys were placed on the device");
    if (ctx->group && group_appended(ctx)) return ctx->fail(FHH_E_STATE, "add_keys onto appended keys");
    const size_t K = ctx->K, L = ctx->L;
    ctx->h_key_idx.insert(ctx->h_key_idx.end(), key_idx, key_idx + n * K);
    ctx->h_root.insert(ctx->h_root.end(), root_seed, root_seed + n * K * 16);
    ctx->h_cws.insert(ctx->h_cws.end(), cw_seed, cw_seed + n * K * L * 16);
    ctx->h_cwb.insert(ctx->h_cwb.end(), cw_bits, cw_bits + n * K * L);
    ctx->h_n += n;
    return FHH_OK;
}

int fhh_gen_keys_pair(fhh_ctx* c0, fhh_ctx* c1, uint64_t n, const uint8_t* left_bits, const uint8_t* right_bits,
                      const uint8_t* root_seeds) {
    if (!c0 || !c1) {
        g_err = "null fhh_ctx";
        return FHH_E_ARG;
    }
    if (c0->group || c1->group) return group_gen_keys_pair(c0, c1, n, left_bits, right_bits, root_seeds);
    if (c0->device != c1->device || c0->d != c1->d || c0->L != c1->L)
        return c0->fail(FHH_E_ARG, "gen_keys_pair: ctxs differ in device/d/L");
    if (c0->dev_keys || c1->dev_keys || c0->h_n || c1->h_n)
        return c0->fail(FHH_E_STATE, "gen_keys_pair: ctxs must be empty");
    if (!left_bits || !right_bits || !root_seeds) return c0->fail(FHH_E_ARG, "gen_keys_pair: NULL buffer");
    int rc = ctx_set_device(c0);
    if (rc) return rc;
    rc = alloc_keys(c0, n);
    if (rc) return rc;
    rc = alloc_keys(c1, n);
    if (rc) return rc;
    const size_t d = c0->d, L = c0->L;
    DevBuf lb, rb, rs;
    HIP_TRY(c0, lb.ensure(n * d * L));
    HIP_TRY(c0, rb.ensure(n * d * L));
    HIP_TRY(c0, rs.ensure(n * d * 64));
    HIP_TRY(c0, hipMemcpyAsync(lb.p, left_bits, n * d * L, hipMemcpyHostToDevice, c0->stream));
    HIP_TRY(c0, hipMemcpyAsync(rb.p, right_bits, n * d * L, hipMemcpyHostToDevice, c0->stream));
    HIP_TRY(c0, hipMemcpyAsync(rs.p, root_seeds, n * d * 64, hipMemcpyHostToDevice, c0->stream));
    KeygenArgs a{};
    a.left_bits = lb.as<uint8_t>();
    a.right_bits = rb.as<uint8_t>();
    a.root_seeds = rs.as<uint8_t>();
    fhh_ctx* cs[2] = {c0, c1};
    for (int b = 0; b < 2; b++) {
        a.cw_seed[b] = cs[b]->cw_seed.as<uint4>();
        a.cw_bits[b] = cs[b]->cw_bits.as<uint64_t>();
        a.root[b] = cs[b]->root_seed.as<uint4>();
        a.key_idx[b] = cs[b]->key_idx.as<uint64_t>();
    }
    a.n = n;
    a.d = (uint32_t)d;
    a.L = (uint32_t)L;
    a.K = c0->K;
    a.npad = (uint32_t)c0->npad;
    a.nw = (uint32_t)c0->nw;
    hipEvent_t e0, e1;
    HIP_TRY(c0, hipEventCreate(&e0));
    HIP_TRY(c0, hipEventCreate(&e1));
    HIP_TRY(c0, hipEventRecord(e0, c0->stream));
    HIP_TRY(c0, launch_keygen(a, kKeygenBytes, c0->stream));
    HIP_TRY(c0, hipEventRecord(e1, c0->stream));
    rc = ctx_sync(c0);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (rc) return rc;
    c0->stats.keygen_ms += ms;
    c0->dev_keys = c1->dev_keys = true;
    return FHH_OK;
}

int fhh_num_clients(const fhh_ctx* ctx, uint64_t* n) {
    CTX_CHECK(ctx);
    if (ctx->group) return group_num_clients(ctx, n);
    if (n) *n = ctx->dev_keys ? ctx->n : ctx->h_n;
    return FHH_OK;
}

int fhh_export_keys(fhh_ctx* ctx, uint8_t* key_idx, uint8_t* root_seed, uint8_t* cw_seed, uint8_t* cw_bits) {
    CTX_CHECK(ctx);
    if (ctx->group) return group_export_keys(ctx, key_idx, root_seed, cw_seed, cw_bits);
    int rc = ctx_set_device(ctx);
    if (rc) return rc;
    if (!ctx->dev_keys) {
        if (key_idx) std::memcpy(key_idx, ctx->h_key_idx.data(), ctx->h_key_idx.size());
        if (root_seed) std::memcpy(root_seed, ctx->h_root.data(), ctx->h_root.size());
        if (cw_seed) std::memcpy(cw_seed, ctx->h_cws.data(), ctx->h_cws.size());
        if (cw_bits) std::memcpy(cw_bits, ctx->h_cwb.data(), ctx->h_cwb.size());
        return FHH_OK;
    }
    const size_t n = ctx->n, K = ctx->K, L = ctx->L, npad = ctx->npad, nw = ctx->nw;
    std::vector<uint8_t> cws(L * K * npad * 16), roots(K * npad * 16);
    std::vector<uint64_t> cwb(L * K * 4 * nw), kidx(K * nw);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // uploads / keygen are async
    HIP_TRY(ctx, hipMemcpy(cws.data(), ctx->cw_seed.p, cws.size(), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(roots.data(), ctx->root_seed.p, roots.size(), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(cwb.data(), ctx->cw_bits.p, cwb.size() * 8, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(kidx.data(), ctx->key_idx.p, kidx.size() * 8, hipMemcpyDeviceToHost));
    for (size_t c = 0; c < n; c++)
        for (size_t kk = 0; kk < K; kk++) {
            const size_t w = c / 64, bit = c % 64;
            if (key_idx) key_idx[c * K + kk] = (uint8_t)((kidx[kk * nw + w] >> bit) & 1);
            if (root_seed) std::memcpy(root_seed + (c * K + kk) * 16, &roots[(kk * npad + c) * 16], 16);
            for (size_t l = 0; l < L; l++) {
                const size_t row = l * K + kk;
                if (cw_seed) std::memcpy(cw_seed + ((c * K + kk) * L + l) * 16, &cws[(row * npad + c) * 16], 16);
                if (cw_bits) {
                    uint8_t nib = 0;
                    for (int b = 0; b < 4; b++) nib |= (uint8_t)(((cwb[(row * 4 + b) * nw + w] >> bit) & 1) << b);
                    cw_bits[(c * K + kk) * L + l] = nib;
                }
            }
        }
    return FHH_OK;
}

int fhh_tree_init(fhh_ctx* ctx) {
    CTX_CHECK(ctx);
    if (ctx->group) return group_tree_init(ctx);
    int rc = ctx_set_device(ctx);
    if (rc) return rc;
    rc = upload_staged_keys(ctx);
    if (rc) return rc;
    if (!ctx->dev_keys || ctx->n == 0) return ctx->fail(FHH_E_STATE, "tree_init with no keys (collect.rs:83)");
    if (ctx->appended) {
        rc = finish_appended(ctx);
        if (rc) return rc;
    }
    for (uint32_t j = 0; j < ctx->d; j++) {
        DimTable& T = ctx->tab[j];
        T.cur = 0;
        rc = table_ensure(ctx, T, 0, 1);
        if (rc) return rc;
        HIP_TRY(ctx, launch_init_tables(ctx->root_seed.as<uint4>(), ctx->key_idx.as<uint64_t>(), j, ctx->K,
                                        (uint32_t)ctx->npad, (uint32_t)ctx->nw, T.seed[0].as<uint4>(),
                                        T.t[0].as<uint64_t>(), T.y[0].as<uint64_t>(), ctx->stream));
        T.live.assign(1, 0);
    }
    ctx->frontier.assign(1, Node{});
    ctx->hist.clear();
    ctx->last_nodes.clear();
    ctx->last_values.clear();
    ctx->last_hist.clear();
    ctx->level = 0;
    ctx->pending_C = 0;
    ctx->phase = Phase::kFrontier;
    return ctx_sync(ctx);
}

int fhh_frontier_plan(uint32_t n_dims, uint32_t depth, uint64_t n_nodes, const uint8_t* paths, uint32_t* n_unique,
                      uint32_t* pos) {
    FrontierPlan plan;
    std::string why;
    if (!frontier_plan(n_dims, depth, n_nodes, paths, plan, &why)) {
        g_err = "frontier_plan: " + why;
        return FHH_E_ARG;
    }
    if (n_unique) std::memcpy(n_unique, plan.n_unique.data(), plan.n_unique.size() * 4);
    if (pos) std::memcpy(pos, plan.pos.data(), plan.pos.size() * 4);
    return FHH_OK;
}

int fhh_tree_init_at(fhh_ctx* ctx, uint64_t n_nodes, uint32_t depth, const uint8_t* paths) {
    CTX_CHECK(ctx);
    // every refusal of the arguments comes before the ctx is touched
    if (depth >= ctx->L)
        return ctx->fail(FHH_E_ARG, "tree_init_at: depth " + std::to_string(depth) + " >= data_len " +
                                        std::to_string(ctx->L) + " (no CorWord left to crawl)");
    FrontierPlan plan;
    std::string why;
    if (!frontier_plan(ctx->d, depth, n_nodes, paths, plan, &why)) return ctx->fail(FHH_E_ARG, "tree_init_at: " + why);
    if (ctx->group) return group_tree_init_at(ctx, plan, n_nodes, depth, paths);
    return tree_init_at_planned(ctx, plan, n_nodes, depth, paths);
}

int fhh_frontier_paths(fhh_ctx* ctx, uint64_t* n_nodes, uint32_t* depth, uint8_t* paths) {
    CTX_CHECK(ctx);
    if (ctx->group) {
        fhh_ctx* lead = group_lead(ctx);
        if (!lead) return ctx->fail(FHH_E_STATE, "frontier_paths before tree_init");
        const int rc = fhh_frontier_paths(lead, n_nodes, depth, paths);
        if (rc) ctx->fail(rc, lead->err);
        return rc;
    }
    if (ctx->phase == Phase::kNoInit) return ctx->fail(FHH_E_STATE, "frontier_paths before tree_init");
    // the nodes fhh_frontier_size counts: an unpruned tree_crawl's children, else the frontier
    const bool pending = ctx->phase == Phase::kPending;
    const uint64_t F = pending ? ctx->pending_C : ctx->frontier.size();
    const uint32_t len = pending ? ctx->level + 1 : ctx->level, d = ctx->d;
    if (n_nodes) *n_nodes = F;
    if (depth) *depth = len;
    if (!paths || len == 0) return FHH_OK;
    if (ctx->hist.size() < (pending ? len - 1 : len) || (!pending && ctx->hist[len - 1].size() != F))
        return ctx->fail(FHH_E_STATE, "frontier_paths: the crawl history does not cover the frontier");
    for (uint64_t k = 0; k < F; k++) {
        const std::pair<uint32_t, uint32_t> pi =
            pending ? std::make_pair((uint32_t)(k >> d), (uint32_t)(k & ((1u << d) - 1))) : ctx->hist[len - 1][k];
        node_path(ctx->hist, len - 1, pi.first, pi.second, d, paths + k * d * len);
    }
    return FHH_OK;
}

int fhh_tree_crawl(fhh_ctx* ctx, uint64_t* n_children, uint64_t* share_planes) {
    CTX_CHECK(ctx);
    if (ctx->group) return group_tree_crawl(ctx, false, n_children, share_planes);
    int rc = ctx_set_device(ctx);
    if (rc) return rc;
    return crawl_level(ctx, false, n_children, share_planes, ctx->nw, 0);
}

int fhh_tree_crawl_last(fhh_ctx* ctx, uint64_t* n_children, uint64_t* share_planes) {
    CTX_CHECK(ctx);
    if (ctx->group) return group_tree_crawl(ctx, true, n_children, share_planes);
    int rc = ctx_set_device(ctx);
    if (rc) return rc;
    return crawl_level(ctx, true, n_children, share_planes, ctx->nw, 0);
}

// node sums of one ctx (single GPU): partials on the device, one copy back, host finish
static int node_sums_single(fhh_ctx* ctx, const void* vals, bool host, uint64_t ld, uint32_t fmt, void* out_a,
                            void* out_b) {
    int rc = ctx_set_device(ctx);
    if (rc) return rc;
    uint64_t* part = nullptr;
    rc = node_partials(ctx, vals, fmt, ld, 0, host, &part);
    if (rc) return rc;
    const uint64_t per = fmt_is_fe255(fmt) ? 8 : 2;
    std::vector<uint64_t> h(ctx->pending_C * per);
    if (!h.empty()) HIP_TRY(ctx, hipMemcpyAsync(h.data(), part, h.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    rc = ctx_sync(ctx);
    if (rc) return rc;
    return node_sums_finish(ctx, h.data(), fmt, out_a, out_b);
}

int fhh_node_sums_fe(fhh_ctx* ctx, const uint64_t* vals, uint64_t* sums) {
    CTX_CHECK(ctx);
    if (!sums) return ctx->fail(FHH_E_ARG, "node_sums_fe: NULL sums");
    if (ctx->group) {
        const void* v[1] = {vals};
        return group_node_sums(ctx, v, true, 0, FHH_VALS_FE_U64, sums, nullptr);
    }
    return node_sums_single(ctx, vals, true, ctx->n, FHH_VALS_FE_U64, sums, nullptr);
}

int fhh_node_sums_fe255(fhh_ctx* ctx, const uint32_t* vals, uint32_t* sums_unreduced, uint32_t* sums_canonical) {
    CTX_CHECK(ctx);
    if (ctx->group) {
        const void* v[1] = {vals};
        return group_node_sums(ctx, v, true, 0, FHH_VALS_FE255_LIMBS, sums_unreduced, sums_canonical);
    }
    return node_sums_single(ctx, vals, true, ctx->n, FHH_VALS_FE255_LIMBS, sums_unreduced, sums_canonical);
}

int fhh_node_sums_fe_device(fhh_ctx* ctx, const void* const* vals_dev, uint64_t ld, uint32_t format, uint64_t* sums) {
    CTX_CHECK(ctx);
    if (format != FHH_VALS_FE_U64 && format != FHH_VALS_FE_BLOCK)
        return ctx->fail(FHH_E_ARG, "node_sums_fe_device: format must be FHH_VALS_FE_U64 or FHH_VALS_FE_BLOCK");
    if (!vals_dev || !sums) return ctx->fail(FHH_E_ARG, "node_sums_fe_device: NULL vals_dev / sums");
    if (ctx->group) return group_node_sums(ctx, vals_dev, false, ld, format, sums, nullptr);
    return node_sums_single(ctx, vals_dev[0], false, ld ? ld : ctx->n, format, sums, nullptr);
}

int fhh_node_sums_fe255_device(fhh_ctx* ctx, const void* const* vals_dev, uint64_t ld, uint32_t format,
                               uint32_t* sums_unreduced, uint32_t* sums_canonical) {
    CTX_CHECK(ctx);
    if (format != FHH_VALS_FE255_LIMBS && format != FHH_VALS_FE255_BLOCKPAIR)
        return ctx->fail(FHH_E_ARG, "node_sums_fe255_device: format must be FHH_VALS_FE255_LIMBS or _BLOCKPAIR");
    if (!vals_dev) return ctx->fail(FHH_E_ARG, "node_sums_fe255_device: NULL vals_dev");
    if (ctx->group) return group_node_sums(ctx, vals_dev, false, ld, format, sums_unreduced, sums_canonical);
    return node_sums_single(ctx, vals_dev[0], false, ld ? ld : ctx->n, format, sums_unreduced, sums_canonical);
}

int fhh_tree_prune(fhh_ctx* ctx, const uint8_t* keep, uint64_t n) {
    CTX_CHECK(ctx);
    if (n && !keep) return ctx->fail(FHH_E_ARG, "tree_prune: NULL keep");
    if (ctx->group) return group_tree_prune(ctx, keep, n, false);
    return prune_impl(ctx, keep, n);
}

int fhh_tree_prune_last(fhh_ctx* ctx, const uint8_t* keep, uint64_t n) {
    CTX_CHECK(ctx);
    if (n && !keep) return ctx->fail(FHH_E_ARG, "tree_prune_last: NULL keep");
    if (ctx->group) return group_tree_prune(ctx, keep, n, true);
    if (ctx->phase != Phase::kPendingLast && ctx->last_nodes.empty() && n != 0)
        return ctx->fail(FHH_E_STATE, "tree_prune_last without tree_crawl_last");
    if (n != ctx->last_nodes.size())
        return ctx->fail(FHH_E_ARG, "tree_prune_last: keep.len() != frontier_last.len() (collect.rs:932)");
    std::vector<std::pair<uint32_t, uint32_t>> nodes;
    std::vector<Limbs10> vals;
    for (uint64_t k = 0; k < n; k++)
        if (keep[k]) {
            nodes.push_back(ctx->last_nodes[k]);
            vals.push_back(ctx->last_values[k]);
        }
    ctx->last_nodes = std::move(nodes);
    ctx->last_values = std::move(vals);
    if (ctx->phase == Phase::kPendingLast) ctx->phase = Phase::kFrontier;   // frontier unchanged (collect.rs:909-914)
    ctx->pending_C = 0;
    return FHH_OK;
}

int fhh_frontier_size(const fhh_ctx* ctx, uint64_t* n_frontier, uint64_t* n_frontier_last) {
    CTX_CHECK(ctx);
    if (ctx->group) {
        if (!group_lead(ctx)) {
            if (n_frontier) *n_frontier = 0;
            if (n_frontier_last) *n_frontier_last = 0;
            return FHH_OK;
        }
        return fhh_frontier_size(group_lead(ctx), n_frontier, n_frontier_last);
    }
    if (n_frontier) *n_frontier = ctx->phase == Phase::kPending ? ctx->pending_C : ctx->frontier.size();
    if (n_frontier_last) *n_frontier_last = ctx->last_nodes.size();
    return FHH_OK;
}

int fhh_final_shares(fhh_ctx* ctx, uint64_t* n_final, uint32_t* levels, uint8_t* paths, uint32_t* values) {
    CTX_CHECK(ctx);
    if (ctx->group) {
        fhh_ctx* lead = group_lead(ctx);
        if (!lead) return ctx->fail(FHH_E_STATE, "final_shares: no keys placed on the shards");
        const int rc = fhh_final_shares(lead, n_final, levels, paths, values);
        if (rc) ctx->fail(rc, lead->err);
        return rc;
    }
    const uint64_t F = ctx->last_nodes.size();
    if (n_final) *n_final = F;
    if (levels) *levels = ctx->last_depth;
    if (F == 0) return FHH_OK;
    const uint32_t len = ctx->last_depth;
    for (uint64_t k = 0; k < F; k++) {
        if (paths) node_path(ctx->last_hist, len - 1, ctx->last_nodes[k].first, ctx->last_nodes[k].second, ctx->d,
                             paths + k * ctx->d * len);
        if (values) std::memcpy(values + k * 10, ctx->last_values[k].data(), 40);
    }
    return FHH_OK;
}

int fhh_export_states(fhh_ctx* ctx, uint64_t* n_nodes, uint8_t* seeds, uint8_t* t, uint8_t* y) {
    CTX_CHECK(ctx);
    if (ctx->group) return group_export_states(ctx, n_nodes, seeds, t, y);
    int rc = ctx_set_device(ctx);
    if (rc) return rc;
    if (ctx->phase == Phase::kNoInit) return ctx->fail(FHH_E_STATE, "export_states before tree_init");
    const bool pending = ctx->phase == Phase::kPending || ctx->phase == Phase::kPendingLast;
    const uint64_t F = pending ? ctx->pending_C : ctx->frontier.size();
    if (n_nodes) *n_nodes = F;
    if (!seeds && !t && !y) return FHH_OK;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const size_t n = ctx->n, npad = ctx->npad, nw = ctx->nw, d = ctx->d;
    for (uint32_t j = 0; j < d; j++) {
        DimTable& T = ctx->tab[j];
        const int buf = pending ? ctx->child_buf[j] : T.cur;
        // copy the whole buffer (tests only)
        std::vector<uint8_t> hs(T.cap[buf] * 2 * npad * 16);
        std::vector<uint64_t> ht(T.cap[buf] * 2 * nw), hy(T.cap[buf] * 2 * nw);
        HIP_TRY(ctx, hipMemcpy(hs.data(), T.seed[buf].p, hs.size(), hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(ht.data(), T.t[buf].p, ht.size() * 8, hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(hy.data(), T.y[buf].p, hy.size() * 8, hipMemcpyDeviceToHost));
        for (uint64_t node = 0; node < F; node++) {
            uint32_t e;
            if (pending) {
                const uint64_t p = node >> d;
                const uint32_t i = (uint32_t)(node & ((1u << d) - 1));
                e = 2 * ctx->frontier[p].pos[j] + ((i >> j) & 1);
            } else {
                e = T.live[ctx->frontier[node].pos[j]];
            }
            for (size_t c = 0; c < n; c++)
                for (int s = 0; s < 2; s++) {
                    const size_t o = ((node * n + c) * d + j) * 2 + s;
                    if (seeds) std::memcpy(seeds + o * 16, &hs[(((size_t)e * 2 + s) * npad + c) * 16], 16);
                    if (t) t[o] = (uint8_t)((ht[((size_t)e * 2 + s) * nw + c / 64] >> (c % 64)) & 1);
                    if (y) y[o] = (uint8_t)((hy[((size_t)e * 2 + s) * nw + c / 64] >> (c % 64)) & 1);
                }
        }
    }
    return FHH_OK;
}

int fhh_keep_values(uint64_t threshold, const uint64_t* vals0, const uint64_t* vals1, uint64_t n, uint8_t* keep) {
    if (n && (!vals0 || !vals1 || !keep)) {
        g_err = "keep_values: NULL buffer";
        return FHH_E_ARG;
    }
    const uint64_t t = threshold % kFeP;
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t a = vals0[i] % kFeP, b = vals1[i] % kFeP;
        const uint64_t v = a >= b ? a - b : a + (kFeP - b);
        keep[i] = v >= t;
    }
    return FHH_OK;
}

int fhh_keep_values_ring32(uint64_t threshold, const uint64_t* vals0, const uint64_t* vals1, uint64_t n, uint8_t* keep) {
    if (n && (!vals0 || !vals1 || !keep)) {
        g_err = "keep_values_ring32: NULL buffer";
        return FHH_E_ARG;
    }
    if (threshold >> 32) {
        g_err = "keep_values_ring32: the threshold must be below 2^32";
        return FHH_E_ARG;
    }
    // checked before anything is written: a value of 2^32 or more is not a Z_2^32 sum (FE sums fed in by mistake)
    for (uint64_t i = 0; i < n; i++)
        if ((vals0[i] | vals1[i]) >> 32) {
            g_err = "keep_values_ring32: value " + std::to_string(i) + " is not below 2^32 (FE sums? use fhh_keep_values)";
            return FHH_E_ARG;
        }
    for (uint64_t i = 0; i < n; i++) keep[i] = (uint32_t)((uint32_t)vals0[i] - (uint32_t)vals1[i]) >= (uint32_t)threshold;
    return FHH_OK;
}

int fhh_keep_values_last(uint32_t threshold, const uint32_t* vals0, const uint32_t* vals1, uint64_t n, uint8_t* keep) {
    if (n && (!vals0 || !vals1 || !keep)) {
        g_err = "keep_values_last: NULL buffer";
        return FHH_E_ARG;
    }
    for (uint64_t i = 0; i < n; i++) {
        Limbs10 a{}, b{};
        std::memcpy(a.data(), vals0 + i * 10, 40);
        std::memcpy(b.data(), vals1 + i * 10, 40);
        auto v = fe255_sub(fe255_reduce(a), fe255_reduce(b));   // v0.reduce(); v1.reduce(); v0 - v1
        keep[i] = fhh::fe255_ge_u32(v.data(), threshold);
    }
    return FHH_OK;
}

int fhh_final_values(const uint32_t* vals0, const uint32_t* vals1, uint64_t n, uint32_t* out) {
    if (n && (!vals0 || !vals1 || !out)) {
        g_err = "final_values: NULL buffer";
        return FHH_E_ARG;
    }
    for (uint64_t i = 0; i < n; i++) {
        Limbs10 a{}, b{};
        std::memcpy(a.data(), vals0 + i * 10, 40);
        std::memcpy(b.data(), vals1 + i * 10, 40);
        auto v = fe255_sub(fe255_reduce(a), fe255_reduce(b));
        std::memcpy(out + i * 8, v.data(), 32);
    }
    return FHH_OK;
}

int fhh_set_variant(fhh_ctx* ctx, int variant) {
    CTX_CHECK(ctx);
    if (ctx->group) return group_each(ctx, fhh_set_variant, variant);
    if (variant < 0 || variant >= expand_variant_count()) return ctx->fail(FHH_E_ARG, "set_variant: no such variant");
    if (!expand_threads(variant))
        return ctx->fail(FHH_E_ARG, "set_variant: variant " + std::to_string(variant) +
                                        " is not in this build (it holds 52 and 33; the r01-r03 A/B forms were removed)");
    ctx->variant = variant;
    ctx->grid = expand_grid(ctx->device, variant);   // also drops a fhh_set_expand_grid override
    return FHH_OK;
}

int fhh_set_expand_grid(fhh_ctx* ctx, int blocks) {
    CTX_CHECK(ctx);
    if (ctx->group) return group_each(ctx, fhh_set_expand_grid, blocks);
    // shrink only: the occupancy value is the most blocks that are resident at once, and the dynamic
    // heads assume a persistent grid
    const int full = expand_grid(ctx->device, ctx->variant);
    if (blocks < 1 || blocks > full)
        return ctx->fail(FHH_E_ARG, "set_expand_grid: blocks must be in [1, " + std::to_string(full) + "]");
    ctx->grid = blocks;
    return FHH_OK;
}

int fhh_set_table_row_major(fhh_ctx* ctx, int on) {
    CTX_CHECK(ctx);
    if (ctx->group) return group_each(ctx, fhh_set_table_row_major, on);
    if (on != 0 && on != 1) return ctx->fail(FHH_E_ARG, "set_table_row_major: on must be 0 or 1");
    ctx->table_row_major = on;
    return FHH_OK;
}

int fhh_set_protocol_grid(fhh_ctx* ctx, int blocks) {
    CTX_CHECK(ctx);
    if (blocks < 0) return ctx->fail(FHH_E_ARG, "set_protocol_grid: blocks must be >= 0 (0: the device rule)");
    if (ctx->group) {   // the shards launch; the group ctx keeps the value for fhh_protocol_grid
        const int rc = group_each(ctx, fhh_set_protocol_grid, blocks);
        if (rc) return rc;
    }
    ctx->protocol_grid = blocks;
    return FHH_OK;
}

int fhh_protocol_grid(fhh_ctx* ctx, int family, uint64_t need, int* grid) {
    CTX_CHECK(ctx);
    if (family < 0 || family >= (int)kGridFamilies || !grid)
        return ctx->fail(FHH_E_ARG, "protocol_grid: family must be in [0, " + std::to_string((int)kGridFamilies) +
                                        ") and grid non-null");
    if (!ctx->group) {   // the CU count is the ctx's device's (a multi-device ctx: the current device's)
        const int rc = ctx_set_device(ctx);
        if (rc) return rc;
    }
    *grid = protocol_grid(need, (ProtocolGridFamily)family, ctx->protocol_grid);
    return FHH_OK;
}

int fhh_expand_layout(int variant, int grid_blocks, uint32_t njobs, const uint32_t* n_live, uint32_t nw, uint32_t* g,
                      uint32_t* wpi, uint64_t* total) {
    if (variant < 0 || variant >= expand_variant_count() || !expand_threads(variant)) {
        g_err = "expand_layout: no such variant in this build";
        return FHH_E_ARG;
    }
    if (grid_blocks < 1 || njobs < 1 || njobs > (uint32_t)kMaxJobs || !n_live || nw < 1) {
        g_err = "expand_layout: bad arguments";
        return FHH_E_ARG;
    }
    // as finalize_launch, k_prune and k_loop_init call it
    const uint64_t waves = (uint64_t)grid_blocks * (expand_threads(variant) / 64);
    ItemLayout lay;
    item_layout(n_live, njobs, nw, expand_max_group(variant), waves, lay, expand_max_wpi(variant));
    if (g) *g = lay.g;
    if (wpi) *wpi = lay.wpi;
    if (total) *total = lay.total;
    return FHH_OK;
}

int fhh_variant_info(int variant, char* name, size_t cap, int* threads, int* grid_per_device) {
    if (variant < 0 || variant >= expand_variant_count() || !expand_threads(variant)) {
        g_err = "variant_info: no such variant in this build";
        return FHH_E_ARG;
    }
    if (name && cap) std::snprintf(name, cap, "%s", expand_variant_name(variant));
    if (threads) *threads = expand_threads(variant);
    if (grid_per_device) {
        int dev = 0;
        (void)hipGetDevice(&dev);
        *grid_per_device = expand_grid(dev, variant);
    }
    return FHH_OK;
}

int fhh_get_stats(const fhh_ctx* ctx, fhh_stats* out) {
    CTX_CHECK(ctx);
    if (ctx->group) return group_get_stats(ctx, out);
    if (out) *out = ctx->stats;
    return FHH_OK;
}

int fhh_reset_stats(fhh_ctx* ctx) {
    CTX_CHECK(ctx);
    if (ctx->group) return group_each(ctx, [](fhh_ctx* c, int) { return fhh_reset_stats(c); }, 0);
    ctx->stats = fhh_stats{};
    return FHH_OK;
}

int fhh_set_timing(fhh_ctx* ctx, int enabled) {
    CTX_CHECK(ctx);
    if (ctx->group) return group_each(ctx, fhh_set_timing, enabled);
    if (enabled < 0) return ctx->fail(FHH_E_ARG, "set_timing: enabled must be >= 0");
    ctx->timing = enabled != 0;
    ctx->timing_every = enabled > 1 ? (uint32_t)enabled : 1;
    return FHH_OK;
}

int fhh_memcpy_device(int device, void* dst_dev, const void* src_dev, uint64_t bytes) {
    hipError_t e = hipSetDevice(device);
    // a device-to-device hipMemcpy may return before the copy lands; the engine's non-blocking
    // streams do not wait for the null stream, so finish it here
    if (e == hipSuccess && bytes) e = hipMemcpyAsync(dst_dev, src_dev, bytes, hipMemcpyDeviceToDevice, nullptr);
    if (e == hipSuccess && bytes) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) {
        g_err = std::string("memcpy_device: ") + hipGetErrorString(e);
        return FHH_E_HIP;
    }
    return FHH_OK;
}

int fhh_device_info(int device, char* arch_name, size_t cap, int* num_cus) {
    hipDeviceProp_t prop;
    hipError_t e = hipGetDeviceProperties(&prop, device);
    if (e != hipSuccess) {
        g_err = std::string("hipGetDeviceProperties: ") + hipGetErrorString(e);
        return FHH_E_HIP;
    }
    if (arch_name && cap) {
        std::snprintf(arch_name, cap, "%s", prop.gcnArchName);
    }
    if (num_cus) *num_cus = prop.multiProcessorCount;
    return FHH_OK;
}

}  // extern "C"
