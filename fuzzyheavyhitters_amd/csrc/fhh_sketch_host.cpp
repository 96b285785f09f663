// Sketch + Beaver verification (row a9), host side: the C ABI's wrappers of fhh_sketch.hip, once for
// U = FE and once for U = FieldElm (the last level).
#include "fhh_engine.h"

#include <cstring>

namespace {
uint64_t fe_canon_u64(uint64_t v) {   // any FE val -> value() (fastfield.rs:86-107,147-152)
    const uint64_t mask = (1ull << 62) - 1;
    uint64_t r = (v & mask) + (v >> 62) + ((v >> 62) << 30);
    while (r >= kFeP) r -= kFeP;
    return r;
}
}  // namespace

int fhh_sketch_at_fe(fhh_ctx* ctx, uint64_t n_keys, uint32_t n_nodes, const uint8_t* seeds, const uint64_t* x,
                     const uint64_t* kx, uint64_t* sketch6) {
    CTX_CHECK(ctx);
    int rc = ctx_set_device(ctx);
    if (rc) return rc;
    if (n_keys == 0) return FHH_OK;
    if (!seeds || !sketch6 || (n_nodes && (!x || !kx))) return ctx->fail(FHH_E_ARG, "sketch_at_fe: NULL buffer");
    const size_t vb = (size_t)n_keys * n_nodes * 8;
    DevBuf ds, dx, dkx, dout;
    HIP_TRY(ctx, ds.ensure(n_keys * 16));
    HIP_TRY(ctx, dx.ensure(vb));
    HIP_TRY(ctx, dkx.ensure(vb));
    HIP_TRY(ctx, dout.ensure(n_keys * 48));
    HIP_TRY(ctx, hipMemcpyAsync(ds.p, seeds, n_keys * 16, hipMemcpyHostToDevice, ctx->stream));
    if (vb) {
        HIP_TRY(ctx, hipMemcpyAsync(dx.p, x, vb, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(dkx.p, kx, vb, hipMemcpyHostToDevice, ctx->stream));
    }
    SketchArgs a{};
    a.seeds = ds.as<uint8_t>();
    a.x = dx.as<uint64_t>();
    a.kx = dkx.as<uint64_t>();
    a.out = dout.as<uint64_t>();
    a.n_keys = n_keys;
    a.n_nodes = n_nodes;
    HIP_TRY(ctx, launch_sketch_fe(a, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(sketch6, dout.p, n_keys * 48, hipMemcpyDeviceToHost, ctx->stream));
    return ctx_sync(ctx);
}

static int mul_fe_host(fhh_ctx* ctx, uint32_t mode, int server_idx, uint64_t n, const uint64_t* sketch6,
                       const uint64_t* mac, const uint64_t* mac2, const uint64_t* triples9, const uint64_t* cor6,
                       uint64_t* out) {
    CTX_CHECK(ctx);
    int rc = ctx_set_device(ctx);
    if (rc) return rc;
    if (n == 0) return FHH_OK;
    if (!sketch6 || !mac || !mac2 || !triples9 || !out || (mode == 1 && !cor6))
        return ctx->fail(FHH_E_ARG, "mul_fe: NULL buffer");
    DevBuf dsk, dm, dm2, dt, dc, dout;
    const size_t out_words = mode == 0 ? 6 : 1;
    HIP_TRY(ctx, dsk.ensure(n * 48));
    HIP_TRY(ctx, dm.ensure(n * 8));
    HIP_TRY(ctx, dm2.ensure(n * 8));
    HIP_TRY(ctx, dt.ensure(n * 72));
    HIP_TRY(ctx, dc.ensure(n * 48));
    HIP_TRY(ctx, dout.ensure(n * 8 * out_words));
    HIP_TRY(ctx, hipMemcpyAsync(dsk.p, sketch6, n * 48, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(dm.p, mac, n * 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(dm2.p, mac2, n * 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(dt.p, triples9, n * 72, hipMemcpyHostToDevice, ctx->stream));
    if (mode == 1) HIP_TRY(ctx, hipMemcpyAsync(dc.p, cor6, n * 48, hipMemcpyHostToDevice, ctx->stream));
    MulArgs a{};
    a.sketch = dsk.as<uint64_t>();
    a.mac = dm.as<uint64_t>();
    a.mac2 = dm2.as<uint64_t>();
    a.triples = dt.as<uint64_t>();
    a.cor = dc.as<uint64_t>();
    a.out = dout.as<uint64_t>();
    a.n = n;
    a.mode = mode;
    a.server_idx = server_idx ? 1 : 0;
    a.triples_levels = 1;
    HIP_TRY(ctx, launch_mul_fe(a, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(out, dout.p, n * 8 * out_words, hipMemcpyDeviceToHost, ctx->stream));
    return ctx_sync(ctx);
}

int fhh_mul_cor_share_fe(fhh_ctx* ctx, uint64_t n, const uint64_t* sketch6, const uint64_t* mac_key,
                         const uint64_t* mac_key2, const uint64_t* triples9, uint64_t* cor_share6) {
    return mul_fe_host(ctx, 0, 0, n, sketch6, mac_key, mac_key2, triples9, nullptr, cor_share6);
}

int fhh_mul_out_share_fe(fhh_ctx* ctx, int server_idx, uint64_t n, const uint64_t* sketch6, const uint64_t* mac_key,
                         const uint64_t* mac_key2, const uint64_t* triples9, const uint64_t* cor6, uint64_t* out) {
    return mul_fe_host(ctx, 1, server_idx, n, sketch6, mac_key, mac_key2, triples9, cor6, out);
}

int fhh_mul_cor_fe(uint64_t n, const uint64_t* share0, const uint64_t* share1, uint64_t* cor6) {
    if (n && (!share0 || !share1 || !cor6)) {
        g_err = "mul_cor_fe: NULL buffer";
        return FHH_E_ARG;
    }
    for (uint64_t i = 0; i < 6 * n; i++) {
        const uint64_t s = fe_canon_u64(share0[i]) + fe_canon_u64(share1[i]);
        cor6[i] = s >= kFeP ? s - kFeP : s;
    }
    return FHH_OK;
}

int fhh_mul_verify_fe(uint64_t n, const uint64_t* out0, const uint64_t* out1, uint8_t* ok) {
    if (n && (!out0 || !out1 || !ok)) {
        g_err = "mul_verify_fe: NULL buffer";
        return FHH_E_ARG;
    }
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t s = fe_canon_u64(out0[i]) + fe_canon_u64(out1[i]);
        ok[i] = (s >= kFeP ? s - kFeP : s) == 0;
    }
    return FHH_OK;
}

int fhh_sim_sketch_verify_fe(fhh_ctx* ctx, const fhh_sketch_batch* b) {
    CTX_CHECK(ctx);
    int rc = ctx_set_device(ctx);
    if (rc) return rc;
    if (!b) return ctx->fail(FHH_E_ARG, "sim_sketch_verify_fe: NULL batch");
    if (b->n_keys == 0) return FHH_OK;
    if (!b->seeds_dev || !b->ok_dev) return ctx->fail(FHH_E_ARG, "sim_sketch_verify_fe: NULL buffer");
    for (int s = 0; s < 2; s++)
        if (!b->mac_dev[s] || !b->mac2_dev[s] || !b->triples_dev[s] || !b->sketch_dev[s] ||
            (b->n_nodes && (!b->x_dev[s] || !b->kx_dev[s])))
            return ctx->fail(FHH_E_ARG, "sim_sketch_verify_fe: NULL buffer");
    const uint32_t nl = b->n_levels ? b->n_levels : 1;
    const uint32_t tl = b->triples_levels ? b->triples_levels : 1;
    // every level takes fresh triples (MulState::new, mpc.rs:94-98): a batch without per-level
    // triples verifies one level only (reusing a Beaver triple across openings leaks x - x')
    if (!b->triples_levels && nl > 1)
        return ctx->fail(FHH_E_ARG, "sim_sketch_verify_fe: n_levels > 1 needs triples_levels (fresh triples per level)");
    if (b->triples_levels && b->level + nl > tl)
        return ctx->fail(FHH_E_ARG, "sim_sketch_verify_fe: levels past the triples held");
    // Several levels: a two-stage pipeline over two streams. The main stream runs every level's two
    // main sketch launches back to back; the side stream runs the level's sketch tails (disjoint
    // outputs) and, once both main launches are done, its verify. Level k's sketches go to slot
    // (nl - 1 - k) & 1 (slot 0 = the caller's sketch_dev, so the last level ends there; slot 1 =
    // sketch_alt), so level k + 1's main launches overlap level k's verify, and a slot is reused by
    // level k + 2 only after level k's verify has read it. FHH_SKETCH_OVERLAP=0: one stream.
    static const bool kOverlapEnv = [] {
        const char* e = std::getenv("FHH_SKETCH_OVERLAP");
        return !(e && e[0] == '0');
    }();
    const bool overlap = nl > 1 && kOverlapEnv;
    uint64_t* alt[2] = {nullptr, nullptr};
    // r05: when the batch's sketches fit (12 GiB), every level but the last writes a slot of its own, so
    // the main stream never waits for a verify: the two-slot scheme's wait put a barrier between every
    // two levels' main launches (11.5 us median gap, 1023 per configs[4] step)
    const size_t level_words = (size_t)2 * b->n_keys * 6;
    const bool own_slots = overlap && (size_t)(nl - 1) * level_words * 8 <= ((size_t)12 << 30);
    if (overlap) {
        if (!ctx->side_stream) HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->side_stream, hipStreamNonBlocking));
        for (hipEvent_t& e : ctx->side_ev)
            if (!e) HIP_TRY(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        HIP_TRY(ctx, ctx->sketch_alt.ensure((own_slots ? (size_t)(nl - 1) : 1) * level_words * 8));
        for (int s = 0; s < 2; s++) alt[s] = ctx->sketch_alt.as<uint64_t>() + (size_t)s * b->n_keys * 6;
        // the side stream starts after everything already on the main stream (triples, uploads)
        HIP_TRY(ctx, hipEventRecord(ctx->side_ev[0], ctx->stream));
        HIP_TRY(ctx, hipStreamWaitEvent(ctx->side_stream, ctx->side_ev[0], 0));
    }
    hipStream_t side = overlap ? ctx->side_stream : ctx->stream;
    hipEvent_t* ev_main = ctx->side_ev;       // [slot]: the slot's main launches are done
    hipEvent_t* ev_ver = ctx->side_ev + 2;    // [slot]: the slot's verify is done
    // a failure part way leaves no side-stream work running on the caller's buffers
    struct SideDrain {
        hipStream_t st;
        bool armed;
        ~SideDrain() {
            if (armed && st) (void)hipStreamSynchronize(st);
        }
    } drain{overlap ? ctx->side_stream : nullptr, overlap};
    for (uint32_t k = 0; k < nl; k++) {
        const uint32_t lv = b->level + k;
        const int slot = own_slots ? 0 : overlap ? (int)((nl - 1 - k) & 1) : 0;
        uint64_t* out[2] = {slot ? alt[0] : b->sketch_dev[0], slot ? alt[1] : b->sketch_dev[1]};
        if (own_slots && k + 1 < nl)
            for (int s = 0; s < 2; s++) out[s] = alt[s] + (size_t)k * level_words;
        if (overlap && !own_slots && k >= 2) HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ev_ver[slot], 0));
        {   // both servers' sketches in one main launch (r05: one launch transition per level, not two)
            SketchArgs a{};
            a.seeds = b->seeds_dev;
            a.x = b->x_dev[0] + (size_t)k * b->x_level_stride;
            a.kx = b->kx_dev[0] + (size_t)k * b->x_level_stride;
            a.out = out[0];
            a.x1 = b->x_dev[1] + (size_t)k * b->x_level_stride;
            a.kx1 = b->kx_dev[1] + (size_t)k * b->x_level_stride;
            a.out1 = out[1];
            a.n_srv = b->n_keys;
            a.n_keys = 2 * b->n_keys;
            a.n_nodes = b->n_nodes;
            a.force_sequential = b->force_sequential;
            a.level = lv;
            HIP_TRY(ctx, launch_sketch_fe2(a, ctx->stream, side));
        }
        if (overlap) {
            HIP_TRY(ctx, hipEventRecord(ev_main[slot], ctx->stream));
            HIP_TRY(ctx, hipStreamWaitEvent(side, ev_main[slot], 0));
        }
        VerifyArgs v{};
        for (int s = 0; s < 2; s++) {
            v.sketch[s] = out[s];
            v.mac[s] = b->mac_dev[s];
            v.mac2[s] = b->mac2_dev[s];
            v.triples[s] = b->triples_dev[s];
        }
        v.ok = b->ok_dev + (size_t)k * b->n_keys;
        v.out_shares = b->out_shares_dev ? b->out_shares_dev + (size_t)k * 2 * b->n_keys : nullptr;
        v.n = b->n_keys;
        v.level = b->triples_levels ? lv : 0;
        v.triples_levels = tl;
        HIP_TRY(ctx, launch_verify_fe(v, side));
        if (overlap) HIP_TRY(ctx, hipEventRecord(ev_ver[slot], side));
    }
    if (overlap) HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ev_ver[0], 0));   // the last level's slot
    drain.armed = false;   // the main stream now waits for the side stream's last verify
    return ctx_sync(ctx);
}

int fhh_deal_triples_fe(fhh_ctx* ctx, uint64_t n, uint32_t levels, uint64_t seed, uint64_t* triples0_dev,
                        uint64_t* triples1_dev) {
    CTX_CHECK(ctx);
    int rc = ctx_set_device(ctx);
    if (rc) return rc;
    if (!triples0_dev || !triples1_dev) return ctx->fail(FHH_E_ARG, "deal_triples_fe: NULL buffer");
    HIP_TRY(ctx, launch_deal_triples_fe(n, levels, seed, triples0_dev, triples1_dev, ctx->stream));
    return ctx_sync(ctx);
}

// ---- U = FieldElm (the last level) -----------------------------------------------------------
int fhh_sketch_at_fe255(fhh_ctx* ctx, uint64_t n_keys, uint32_t n_nodes, const uint8_t* seeds, const uint32_t* x,
                        const uint32_t* kx, uint32_t* sketch6) {
    CTX_CHECK(ctx);
    int rc = ctx_set_device(ctx);
    if (rc) return rc;
    if (n_keys == 0) return FHH_OK;
    if (!seeds || !sketch6 || (n_nodes && (!x || !kx))) return ctx->fail(FHH_E_ARG, "sketch_at_fe255: NULL buffer");
    const size_t vb = (size_t)n_keys * n_nodes * 32;
    DevBuf ds, dx, dkx, dout;
    HIP_TRY(ctx, ds.ensure(n_keys * 16));
    HIP_TRY(ctx, dx.ensure(vb));
    HIP_TRY(ctx, dkx.ensure(vb));
    HIP_TRY(ctx, dout.ensure(n_keys * 192));
    HIP_TRY(ctx, hipMemcpyAsync(ds.p, seeds, n_keys * 16, hipMemcpyHostToDevice, ctx->stream));
    if (vb) {
        HIP_TRY(ctx, hipMemcpyAsync(dx.p, x, vb, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(dkx.p, kx, vb, hipMemcpyHostToDevice, ctx->stream));
    }
    Sketch255Args a{};
    a.seeds = ds.as<uint8_t>();
    a.x = dx.as<uint32_t>();
    a.kx = dkx.as<uint32_t>();
    a.out = dout.as<uint32_t>();
    a.n_keys = n_keys;
    a.n_nodes = n_nodes;
    HIP_TRY(ctx, launch_sketch_fe255(a, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(sketch6, dout.p, n_keys * 192, hipMemcpyDeviceToHost, ctx->stream));
    return ctx_sync(ctx);
}

static int mul_fe255_host(fhh_ctx* ctx, uint32_t mode, int server_idx, uint64_t n, const uint32_t* sketch6,
                          const uint32_t* mac, const uint32_t* mac2, const uint32_t* triples9, const uint32_t* cor6,
                          uint32_t* out) {
    CTX_CHECK(ctx);
    int rc = ctx_set_device(ctx);
    if (rc) return rc;
    if (n == 0) return FHH_OK;
    if (!sketch6 || !mac || !mac2 || !triples9 || !out || (mode == 1 && !cor6))
        return ctx->fail(FHH_E_ARG, "mul_fe255: NULL buffer");
    DevBuf dsk, dm, dm2, dt, dc, dout;
    const size_t out_bytes = mode == 0 ? 192 : 32;
    HIP_TRY(ctx, dsk.ensure(n * 192));
    HIP_TRY(ctx, dm.ensure(n * 32));
    HIP_TRY(ctx, dm2.ensure(n * 32));
    HIP_TRY(ctx, dt.ensure(n * 288));
    HIP_TRY(ctx, dc.ensure(n * 192));
    HIP_TRY(ctx, dout.ensure(n * out_bytes));
    HIP_TRY(ctx, hipMemcpyAsync(dsk.p, sketch6, n * 192, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(dm.p, mac, n * 32, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(dm2.p, mac2, n * 32, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(dt.p, triples9, n * 288, hipMemcpyHostToDevice, ctx->stream));
    if (mode == 1) HIP_TRY(ctx, hipMemcpyAsync(dc.p, cor6, n * 192, hipMemcpyHostToDevice, ctx->stream));
    Mul255Args a{};
    a.sketch = dsk.as<uint32_t>();
    a.mac = dm.as<uint32_t>();
    a.mac2 = dm2.as<uint32_t>();
    a.triples = dt.as<uint32_t>();
    a.cor = dc.as<uint32_t>();
    a.out = dout.as<uint32_t>();
    a.n = n;
    a.mode = mode;
    a.server_idx = server_idx ? 1 : 0;
    HIP_TRY(ctx, launch_mul_fe255(a, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(out, dout.p, n * out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    return ctx_sync(ctx);
}

int fhh_mul_cor_share_fe255(fhh_ctx* ctx, uint64_t n, const uint32_t* sketch6, const uint32_t* mac_key,
                            const uint32_t* mac_key2, const uint32_t* triples9, uint32_t* cor_share6) {
    return mul_fe255_host(ctx, 0, 0, n, sketch6, mac_key, mac_key2, triples9, nullptr, cor_share6);
}

int fhh_mul_out_share_fe255(fhh_ctx* ctx, int server_idx, uint64_t n, const uint32_t* sketch6,
                            const uint32_t* mac_key, const uint32_t* mac_key2, const uint32_t* triples9,
                            const uint32_t* cor6, uint32_t* out) {
    return mul_fe255_host(ctx, 1, server_idx, n, sketch6, mac_key, mac_key2, triples9, cor6, out);
}

int fhh_mul_cor_fe255(uint64_t n, const uint32_t* share0, const uint32_t* share1, uint32_t* cor6) {
    if (n && (!share0 || !share1 || !cor6)) {
        g_err = "mul_cor_fe255: NULL buffer";
        return FHH_E_ARG;
    }
    for (uint64_t i = 0; i < 6 * n; i++) {   // MulState::cor (mpc.rs:160-180)
        uint32_t a[8], b[8], o[8];
        std::memcpy(a, share0 + 8 * i, 32);
        std::memcpy(b, share1 + 8 * i, 32);
        fe255_canonm(a);
        fe255_canonm(b);
        fe255_addm(a, b, o);
        std::memcpy(cor6 + 8 * i, o, 32);
    }
    return FHH_OK;
}

int fhh_mul_verify_fe255(uint64_t n, const uint32_t* out0, const uint32_t* out1, uint8_t* ok) {
    if (n && (!out0 || !out1 || !ok)) {
        g_err = "mul_verify_fe255: NULL buffer";
        return FHH_E_ARG;
    }
    for (uint64_t i = 0; i < n; i++) {   // MulState::verify (mpc.rs:214-220)
        uint32_t a[8], b[8], o[8];
        std::memcpy(a, out0 + 8 * i, 32);
        std::memcpy(b, out1 + 8 * i, 32);
        fe255_canonm(a);
        fe255_canonm(b);
        fe255_addm(a, b, o);
        uint32_t nz = 0;
        for (int k = 0; k < 8; k++) nz |= o[k];
        ok[i] = nz == 0;
    }
    return FHH_OK;
}

int fhh_sim_sketch_verify_fe255(fhh_ctx* ctx, const fhh_sketch_batch255* b) {
    CTX_CHECK(ctx);
    int rc = ctx_set_device(ctx);
    if (rc) return rc;
    if (!b) return ctx->fail(FHH_E_ARG, "sim_sketch_verify_fe255: NULL batch");
    if (b->n_keys == 0) return FHH_OK;
    if (!b->seeds_dev || !b->ok_dev) return ctx->fail(FHH_E_ARG, "sim_sketch_verify_fe255: NULL buffer");
    for (int s = 0; s < 2; s++)
        if (!b->mac_dev[s] || !b->mac2_dev[s] || !b->triples_dev[s] || !b->sketch_dev[s] ||
            (b->n_nodes && (!b->x_dev[s] || !b->kx_dev[s])))
            return ctx->fail(FHH_E_ARG, "sim_sketch_verify_fe255: NULL buffer");
    for (int s = 0; s < 2; s++) {
        Sketch255Args a{};
        a.seeds = b->seeds_dev;
        a.x = b->x_dev[s];
        a.kx = b->kx_dev[s];
        a.out = b->sketch_dev[s];
        a.n_keys = b->n_keys;
        a.n_nodes = b->n_nodes;
        a.force_sequential = b->force_sequential;
        a.level = b->level;
        HIP_TRY(ctx, launch_sketch_fe255(a, ctx->stream));
    }
    Verify255Args v{};
    for (int s = 0; s < 2; s++) {
        v.sketch[s] = b->sketch_dev[s];
        v.mac[s] = b->mac_dev[s];
        v.mac2[s] = b->mac2_dev[s];
        v.triples[s] = b->triples_dev[s];
    }
    v.ok = b->ok_dev;
    v.out_shares = b->out_shares_dev;
    v.n = b->n_keys;
    HIP_TRY(ctx, launch_verify_fe255(v, ctx->stream));
    return ctx_sync(ctx);
}
