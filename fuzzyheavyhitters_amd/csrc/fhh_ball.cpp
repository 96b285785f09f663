// fhh_gen_keys_ball / fhh_ball_bounds (row i): the leader's per-client step, gen_l_inf_ball (ibDCF.rs:175-188) and
// gen_l_inf_ball_from_coords (ibDCF.rs:189-205) as add_fuzzy_keys calls them (leader.rs:130-163) — a population's
// points and a ball size in, both servers' keys out. The bounds a -/+ ball are made in k_keygen from the packed
// point (ball_src.h) and the root seeds are drawn there from a ChaCha20 stream, so a call moves the points (64 B
// per (client, dim) at L = 512) where fhh_gen_keys_pair moves 2 L bytes of bounds and 64 of seeds.
// fhh_ball_bounds is the same arithmetic on the host, with no GPU: what the device path means.
// fhh_leader_requests_ball(_device) takes the same points straight to both servers' add_keys request bytes
// (k_leader_requests, fhh_leader_requests.hip): the keygen fused with row f5's serialization, no keys stored.
#include "fhh_engine.h"

#include <cstring>

#include "ball_src.h"

namespace fhh {
namespace eng {

// the refusals the host and the device form share; d, L = the collection's shape
bool ball_src_check(uint32_t d, uint32_t L, uint64_t n, const fhh_ball_src* src, std::string* why) {
    auto refuse = [&](const std::string& m) {
        *why = m;
        return false;
    };
    if (!src) return refuse("NULL fhh_ball_src");
    if (d < 1 || d > (uint32_t)kMaxDims || L == 0) return refuse("n_dims outside 1..4 or data_len = 0");
    if (src->form == FHH_BALL_BITS) {
        // the reference pads a shorter point to delta's 32 bits and would make 32-level keys (lib.rs:132-134)
        if (L < 32) return refuse("data_len " + std::to_string(L) + " < 32: gen_l_inf_ball pads to 32 bits (ibDCF.rs:178)");
    } else if (src->form == FHH_BALL_COORDS) {
        if (d != 2 || L != 16) return refuse("the coordinate form needs n_dims = 2 and data_len = 16 (ibDCF.rs:189-205)");
        if (src->ball > 32767) return refuse("ball " + std::to_string(src->ball) + " is no i16 size (ibDCF.rs:189)");
    } else {
        return refuse("unknown form " + std::to_string(src->form));
    }
    if (n && !src->points) return refuse("NULL points");
    return true;
}

size_t point_bytes(uint32_t form, uint32_t L) { return form == FHH_BALL_BITS ? (L + 7) / 8 : 2; }

std::string carry_text(uint64_t idx, uint32_t d, uint32_t L) {
    return "client " + std::to_string(idx / d) + ", dim " + std::to_string(idx % d) + ": point + ball carries out of bit " +
           std::to_string(L) + " (add_bitstrings grows the string and the leader panics, ibDCF.rs:182)";
}

namespace {

void seed_words(const uint8_t seed[32], uint32_t (&w)[8]) {
    for (int k = 0; k < 8; k++)
        w[k] = (uint32_t)seed[4 * k] | ((uint32_t)seed[4 * k + 1] << 8) | ((uint32_t)seed[4 * k + 2] << 16) |
               ((uint32_t)seed[4 * k + 3] << 24);
}

void drop_keys(fhh_ctx* ctx) {   // a refused call's layout (alloc_keys) leaves with it; the allocations stay
    ctx->n = ctx->npad = ctx->nw = 0;
    ctx->dev_keys = false;
}

int gen_keys_ball_run(fhh_ctx* c0, fhh_ctx* c1, uint64_t n, const fhh_ball_src* src, uint64_t client_off) {
    int rc = ctx_set_device(c0);
    if (rc) return rc;
    rc = alloc_keys(c0, n);
    if (rc) return rc;
    rc = alloc_keys(c1, n);
    if (rc) return rc;
    const size_t d = c0->d, L = c0->L;
    // staging in c0's scratch (kept from call to call): [bad word | points | root seeds]
    const size_t pb = n * d * point_bytes(src->form, (uint32_t)L), p_off = 16, r_off = p_off + ((pb + 15) & ~(size_t)15);
    HIP_TRY(c0, c0->scratch.ensure(r_off + (src->root_seeds ? n * d * 64 : 0)));
    uint8_t* st = c0->scratch.as<uint8_t>();
    HIP_TRY(c0, hipMemsetAsync(st, 0xFF, 8, c0->stream));
    if (pb) HIP_TRY(c0, hipMemcpyAsync(st + p_off, src->points, pb, hipMemcpyHostToDevice, c0->stream));
    if (src->root_seeds && n)
        HIP_TRY(c0, hipMemcpyAsync(st + r_off, src->root_seeds, n * d * 64, hipMemcpyHostToDevice, c0->stream));
    KeygenArgs a{};
    a.points = st + p_off;
    a.root_seeds = src->root_seeds ? st + r_off : nullptr;
    a.bad = reinterpret_cast<unsigned long long*>(st);
    a.ball = src->ball;
    seed_words(src->seed, a.seed);
    a.seed_first = src->seed_first;
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
    HIP_TRY(c0, launch_keygen(a, src->form == FHH_BALL_BITS ? kKeygenBallBits : kKeygenCoords, c0->stream));
    HIP_TRY(c0, hipEventRecord(e1, c0->stream));
    // the carry word comes back with the sync the call ends on anyway
    uint64_t bad = ~0ull;
    HIP_TRY(c0, hipMemcpyAsync(&bad, st, 8, hipMemcpyDeviceToHost, c0->stream));
    rc = ctx_sync(c0);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (rc) return rc;
    if (bad != ~0ull)
        return c0->fail(FHH_E_ARG, "gen_keys_ball: " + carry_text(bad + client_off * d, (uint32_t)d, (uint32_t)L));
    c0->stats.keygen_ms += ms;
    c0->dev_keys = c1->dev_keys = true;
    return FHH_OK;
}

}  // namespace

// ---- fhh_leader_requests_ball (row i): the same points straight to both servers' add_keys request bytes, made by
// k_leader_requests (fhh_leader_requests.hip) in buffers of the call's own; no key buffer, phase, frontier or
// scratch of the ctx is touched, so the call may come on an empty ctx or between the levels of a crawl --------
static int leader_requests_check(fhh_ctx* ctx, uint64_t n, const fhh_ball_src* src, uint64_t batch, uint64_t* bytes) {
    std::string why;
    if (!ball_src_check(ctx->d, ctx->L, n, src, &why)) return ctx->fail(FHH_E_ARG, "leader_requests_ball: " + why);
    if (n == 0) return ctx->fail(FHH_E_ARG, "leader_requests_ball: no clients (an empty request is refused by the decoder too)");
    const uint64_t R = be_record_bytes(ctx->d, ctx->L), B = be_batch(n, batch);
    if (n > (~0ull - 8 * be_requests(n, B)) / R) return ctx->fail(FHH_E_ARG, "leader_requests_ball: size overflows");
    *bytes = be_total_bytes(n, B, R);
    return FHH_OK;
}

// The m clients of `src` (its points, root seeds and seed_first already those of the slice) as clients
// [i0, i0 + m) of an export of `count` clients in requests of B: their bytes [be_slice_begin(i0),
// be_slice_end(i0, m)) of both servers' requests, made in ctx->lr_out[b] from byte (be_slice_begin(i0) & ~3) of
// the export on. Returns when the kernel has run; a carry out is FHH_E_ARG naming client i0 + its index.
int leader_requests_make(fhh_ctx* ctx, uint64_t m, const fhh_ball_src* src, uint64_t i0, uint64_t count, uint64_t B) {
    int rc = ctx_set_device(ctx);
    if (rc) return rc;
    const size_t d = ctx->d, L = ctx->L;
    const uint64_t R = be_record_bytes(ctx->d, ctx->L);
    const uint64_t lo = be_slice_begin(i0, B, R), hi = be_slice_end(i0, m, B, R), org = lo & ~3ull;
    const size_t pb = m * d * point_bytes(src->form, (uint32_t)L), p_off = 16, r_off = p_off + ((pb + 15) & ~(size_t)15);
    HIP_TRY(ctx, ctx->lr_stage.ensure(r_off + (src->root_seeds ? m * d * 64 : 0)));
    for (auto& b : ctx->lr_out) HIP_TRY(ctx, b.ensure(hi - org));
    uint8_t* st = ctx->lr_stage.as<uint8_t>();
    HIP_TRY(ctx, hipMemsetAsync(st, 0xFF, 8, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(st + p_off, src->points, pb, hipMemcpyHostToDevice, ctx->stream));
    if (src->root_seeds)
        HIP_TRY(ctx, hipMemcpyAsync(st + r_off, src->root_seeds, m * d * 64, hipMemcpyHostToDevice, ctx->stream));
    LeaderReqArgs a{};
    a.points = st + p_off;
    a.root_seeds = src->root_seeds ? st + r_off : nullptr;
    a.bad = reinterpret_cast<unsigned long long*>(st);
    for (int b = 0; b < 2; b++) a.out[b] = ctx->lr_out[b].as<uint8_t>();
    a.org = org;
    a.n = m;
    a.i0 = i0;
    a.count = count;
    a.B = B;
    a.d = (uint32_t)d;
    a.L = (uint32_t)L;
    a.ball = src->ball;
    seed_words(src->seed, a.seed);
    a.seed_first = src->seed_first;
    hipEvent_t e0, e1;
    HIP_TRY(ctx, hipEventCreate(&e0));
    HIP_TRY(ctx, hipEventCreate(&e1));
    HIP_TRY(ctx, hipEventRecord(e0, ctx->stream));
    HIP_TRY(ctx, launch_leader_requests(a, src->form == FHH_BALL_BITS ? kKeygenBallBits : kKeygenCoords, ctx->stream));
    HIP_TRY(ctx, hipEventRecord(e1, ctx->stream));
    uint64_t bad = ~0ull;
    HIP_TRY(ctx, hipMemcpyAsync(&bad, st, 8, hipMemcpyDeviceToHost, ctx->stream));
    // the stream alone: timing events and pinned staging of a crawl in progress stay pending
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (bad != ~0ull)
        return ctx->fail(FHH_E_ARG, "leader_requests_ball: " + carry_text(bad + i0 * d, (uint32_t)d, (uint32_t)L));
    ctx->stats.keygen_ms += ms;
    return FHH_OK;
}

// the bytes leader_requests_make left for clients [i0, i0 + m), to the same offsets of out0 / out1
int leader_requests_copy(fhh_ctx* ctx, uint64_t m, uint64_t i0, uint64_t B, uint8_t* out0, uint8_t* out1) {
    int rc = ctx_set_device(ctx);
    if (rc) return rc;
    const uint64_t R = be_record_bytes(ctx->d, ctx->L);
    const uint64_t lo = be_slice_begin(i0, B, R), hi = be_slice_end(i0, m, B, R), org = lo & ~3ull;
    uint8_t* out[2] = {out0, out1};
    for (int b = 0; b < 2; b++)
        HIP_TRY(ctx, hipMemcpyAsync(out[b] + lo, ctx->lr_out[b].as<uint8_t>() + (lo - org), hi - lo, hipMemcpyDeviceToHost,
                                    ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return FHH_OK;
}

int gen_keys_ball_one(fhh_ctx* c0, fhh_ctx* c1, uint64_t n, const fhh_ball_src* src, uint64_t client_off) {
    if (c0->device != c1->device || c0->d != c1->d || c0->L != c1->L)
        return c0->fail(FHH_E_ARG, "gen_keys_ball: ctxs differ in device/d/L");
    if (c0->dev_keys || c1->dev_keys || c0->h_n || c1->h_n)
        return c0->fail(FHH_E_STATE, "gen_keys_ball: ctxs must be empty");
    std::string why;
    if (!ball_src_check(c0->d, c0->L, n, src, &why)) return c0->fail(FHH_E_ARG, "gen_keys_ball: " + why);
    const int rc = gen_keys_ball_run(c0, c1, n, src, client_off);
    if (rc) {   // both ctxs empty and usable, whatever refused or failed
        drop_keys(c0);
        drop_keys(c1);
    }
    return rc;
}

}  // namespace eng
}  // namespace fhh

extern "C" {

int fhh_gen_keys_ball(fhh_ctx* c0, fhh_ctx* c1, uint64_t n, const fhh_ball_src* src) {
    if (!c0 || !c1) {
        g_err = "null fhh_ctx";
        return FHH_E_ARG;
    }
    if (c0->group || c1->group) return group_gen_keys_ball(c0, c1, n, src);
    return gen_keys_ball_one(c0, c1, n, src, 0);
}

int fhh_leader_requests_plan(uint32_t n_dims, uint32_t data_len, uint64_t n, uint64_t* items, uint64_t* waves,
                             uint64_t* trips) {
    if (n_dims < 1 || n_dims > (uint32_t)kMaxDims || data_len == 0 || n == 0) {
        g_err = "leader_requests_plan: n_dims outside 1..4, data_len = 0 or n = 0";
        return FHH_E_ARG;
    }
    const LeaderReqPlan p = leader_req_plan(n_dims, n);
    if (items) *items = p.items;
    if (waves) *waves = p.waves;
    if (trips) *trips = p.trips;
    return FHH_OK;
}

int fhh_leader_requests_ball_device(fhh_ctx* ctx, uint64_t n, const fhh_ball_src* src, uint64_t batch,
                                    const uint8_t** req0_dev, const uint8_t** req1_dev, uint64_t* bytes) {
    CTX_CHECK(ctx);
    if (ctx->group)
        return ctx->fail(FHH_E_ARG, "leader_requests_ball_device: a multi-device ctx has no one device to hand "
                                    "buffers out on (fhh_shard_ctx, or the host-output form)");
    if (!req0_dev || !req1_dev || !bytes) return ctx->fail(FHH_E_ARG, "leader_requests_ball_device: NULL output");
    uint64_t len = 0;
    int rc = leader_requests_check(ctx, n, src, batch, &len);
    if (rc) return rc;
    rc = leader_requests_make(ctx, n, src, 0, n, be_batch(n, batch));
    if (rc) return rc;
    *req0_dev = ctx->lr_out[0].as<uint8_t>();
    *req1_dev = ctx->lr_out[1].as<uint8_t>();
    *bytes = len;
    return FHH_OK;
}

int fhh_leader_requests_ball(fhh_ctx* ctx, uint64_t n, const fhh_ball_src* src, uint64_t batch, uint8_t* out0,
                             uint8_t* out1, uint64_t cap, uint64_t* len) {
    CTX_CHECK(ctx);
    if (!len) return ctx->fail(FHH_E_ARG, "leader_requests_ball: NULL len");
    int rc = leader_requests_check(ctx, n, src, batch, len);
    if (rc) return rc;
    if (!out0 || !out1) return ctx->fail(FHH_E_ARG, "leader_requests_ball: NULL out");
    if (cap < *len)
        return ctx->fail(FHH_E_ARG, "leader_requests_ball: " + std::to_string(*len) + " bytes needed, cap " + std::to_string(cap));
    if (ctx->group) return group_leader_requests_ball(ctx, n, src, batch, out0, out1);
    const uint64_t B = be_batch(n, batch);
    rc = leader_requests_make(ctx, n, src, 0, n, B);
    if (rc) return rc;
    return leader_requests_copy(ctx, n, 0, B, out0, out1);
}

int fhh_ball_bounds(uint32_t n_dims, uint32_t data_len, uint64_t n, const fhh_ball_src* src, uint8_t* left_bits,
                    uint8_t* right_bits, uint8_t* root_seeds_out, uint64_t* bad) {
    if (bad) *bad = ~0ull;
    std::string why;
    if (!ball_src_check(n_dims, data_len, n, src, &why)) {
        g_err = "ball_bounds: " + why;
        return FHH_E_ARG;
    }
    const uint64_t d = n_dims, L = data_len, items = n * d;
    const size_t nb = point_bytes(src->form, data_len);
    const uint8_t* pts = static_cast<const uint8_t*>(src->points);
    if (src->form == FHH_BALL_BITS) {   // a carry out refuses the call before anything is written
        for (uint64_t i = 0; i < items; i++)
            if (ball_bound(pts + i * nb, data_len, src->ball, true).carry_out) {
                if (bad) *bad = i;
                g_err = "ball_bounds: " + carry_text(i, n_dims, data_len);
                return FHH_E_ARG;
            }
    }
    uint8_t* out[2] = {left_bits, right_bits};
    for (int side = 0; side < 2; side++) {
        if (!out[side]) continue;
        for (uint64_t i = 0; i < items; i++) {
            uint8_t* o = out[side] + i * L;
            if (src->form == FHH_BALL_BITS) {
                const uint8_t* row = pts + i * nb;
                const BallBound b = ball_bound(row, data_len, src->ball, side == 1);
                uint32_t cur = 0;
                for (uint32_t l = 0; l < data_len; l++) {
                    if ((l & 31) == 0 && l + 32 < data_len) cur = ball_str32(row, (uint32_t)nb, l);
                    o[l] = (uint8_t)ball_bit(b, data_len, l, cur);
                }
            } else {
                const int16_t c = static_cast<const int16_t*>(src->points)[i];
                const uint32_t v = coords_bound(c, (uint32_t)(i % 2), src->ball, side == 1);
                for (uint32_t l = 0; l < 16; l++) o[l] = (uint8_t)((v >> (15 - l)) & 1u);
            }
        }
    }
    if (root_seeds_out) {
        if (src->root_seeds) {
            std::memcpy(root_seeds_out, src->root_seeds, items * 64);
        } else {
            uint32_t key[8], blk[16];
            seed_words(src->seed, key);
            for (uint64_t i = 0; i < items; i++) {
                chacha20_block(key, src->seed_first * d + i, blk);
                for (int k = 0; k < 16; k++)
                    for (int b = 0; b < 4; b++) root_seeds_out[i * 64 + 4 * k + b] = (uint8_t)(blk[k] >> (8 * b));
            }
        }
    }
    return FHH_OK;
}

}  // extern "C"
