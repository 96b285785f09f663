// add_keys requests in bincode (the reference's AddKeysRequest RPC payload), host side: one-shot decode onto the
// device, batches appended behind a reservation, and device keys serialized back into requests
// (fhh_bincode_out.hip, bincode_emit.h). A multi-device ctx drives the same steps per shard (fhh_group.cpp).
#include "fhh_engine.h"

#include <algorithm>

namespace fhh {
namespace eng {

int add_keys_bincode_records(fhh_ctx* ctx, uint64_t n, const uint8_t* recs) {
    int rc = ctx_set_device(ctx);
    if (rc) return rc;
    if (ctx->dev_keys || ctx->h_n) return ctx->fail(FHH_E_STATE, "add_keys_bincode: ctx already holds keys");
    const uint64_t KB = 25 + 20ull * ctx->L, R = 8 + (uint64_t)ctx->K * KB, len = 8 + n * R;
    rc = alloc_keys(ctx, n);
    if (rc) return rc;
    DevBuf buf, err;
    HIP_TRY(ctx, buf.ensure(len + 4));   // k_bincode_cw_tiles reads whole dwords: up to 3 B past len
    HIP_TRY(ctx, err.ensure(4));
    HIP_TRY(ctx, hipMemsetAsync(err.p, 0, 4, ctx->stream));
    // the u64 client count, then the records (a shard of a multi-device ctx uploads its slice)
    HIP_TRY(ctx, hipMemcpyAsync(buf.p, &n, 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(buf.as<uint8_t>() + 8, recs, n * R, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, launch_keys_from_bincode(buf.as<uint8_t>(), n, ctx->d, ctx->L, (uint32_t)ctx->npad, (uint32_t)ctx->nw,
                                          ctx->cw_seed.as<uint4>(), ctx->cw_bits.as<uint64_t>(),
                                          ctx->root_seed.as<uint4>(), ctx->key_idx.as<uint64_t>(), err.as<uint32_t>(),
                                          ctx->stream));
    uint32_t herr = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&herr, err.p, 4, hipMemcpyDeviceToHost, ctx->stream));
    rc = ctx_sync(ctx);
    if (rc) return rc;
    if (herr) {
        ctx->n = 0;
        return ctx->fail(FHH_E_ARG, "add_keys_bincode: " + bincode_malformed_text(herr));
    }
    ctx->dev_keys = true;
    return FHH_OK;
}

// ---- appended batches (fhh_reserve_clients / fhh_add_keys_bincode_append) ----------------------
std::string bincode_malformed_text(uint32_t herr) {
    return std::string("malformed request (") + ((herr & 1) ? "bool byte > 1 " : "") +
           ((herr & 2) ? "cor_words length " : "") + ((herr & 4) ? "dims per client" : "") + ")";
}

// The key buffers at a row stride of new_npad clients (a multiple of 64): the rows are [row][npad], so the
// clients held so far are copied row by row into fresh buffers (old and new are both live until the copy is
// done); an empty layout only grows its allocations.
static int relayout_keys(fhh_ctx* ctx, uint64_t new_npad) {
    const size_t K = ctx->K, L = ctx->L, new_nw = new_npad / 64;
    if (new_npad == ctx->npad) return FHH_OK;
    if (new_npad >> 32) return ctx->fail(FHH_E_ARG, "add_keys: more than 2^32 clients on one GPU");
    const uint64_t used_w = (ctx->n + 63) / 64;   // <= new_nw
    if (ctx->n == 0) {
        HIP_TRY(ctx, ctx->cw_seed.ensure(L * K * new_npad * 16));
        HIP_TRY(ctx, ctx->cw_bits.ensure(L * K * 4 * new_nw * 8));
        HIP_TRY(ctx, ctx->root_seed.ensure(K * new_npad * 16));
        HIP_TRY(ctx, ctx->key_idx.ensure(K * new_nw * 8));
    } else {
        DevBuf cs, cb, rs, ki;
        HIP_TRY(ctx, cs.ensure(L * K * new_npad * 16));
        HIP_TRY(ctx, cb.ensure(L * K * 4 * new_nw * 8));
        HIP_TRY(ctx, rs.ensure(K * new_npad * 16));
        HIP_TRY(ctx, ki.ensure(K * new_nw * 8));
        HIP_TRY(ctx, launch_repitch_seeds(ctx->cw_seed.as<uint4>(), cs.as<uint4>(), L * K, used_w * 64, ctx->npad,
                                          new_npad, ctx->stream));
        HIP_TRY(ctx, launch_repitch_words(ctx->cw_bits.as<uint64_t>(), cb.as<uint64_t>(), L * K * 4, used_w, ctx->nw,
                                          new_nw, ctx->stream));
        HIP_TRY(ctx, launch_repitch_seeds(ctx->root_seed.as<uint4>(), rs.as<uint4>(), K, used_w * 64, ctx->npad,
                                          new_npad, ctx->stream));
        HIP_TRY(ctx, launch_repitch_words(ctx->key_idx.as<uint64_t>(), ki.as<uint64_t>(), K, used_w, ctx->nw, new_nw,
                                          ctx->stream));
        int rc = ctx_sync(ctx);
        if (rc) return rc;
        ctx->cw_seed.swap(cs);
        ctx->cw_bits.swap(cb);
        ctx->root_seed.swap(rs);
        ctx->key_idx.swap(ki);
    }
    ctx->npad = new_npad;
    ctx->nw = new_nw;
    return FHH_OK;
}

int append_check_state(fhh_ctx* ctx) {
    if (ctx->phase != Phase::kNoInit)
        return ctx->fail(FHH_E_STATE, "add_keys_bincode_append: tree_init has run (fhh_reset first: the prefix tables are sized by the client count)");
    if (ctx->h_n) return ctx->fail(FHH_E_STATE, "add_keys_bincode_append: ctx holds keys staged by fhh_add_keys");
    if (ctx->dev_keys && !ctx->appended)
        return ctx->fail(FHH_E_STATE, "add_keys_bincode_append: ctx holds keys of fhh_gen_keys_pair / fhh_add_keys_bincode");
    return FHH_OK;
}

int append_reserve(fhh_ctx* ctx, uint64_t capacity) {
    int rc = ctx_set_device(ctx);
    if (rc) return rc;
    if (ctx->phase != Phase::kNoInit) return ctx->fail(FHH_E_STATE, "reserve_clients: tree_init has run");
    if (ctx->h_n || (ctx->dev_keys && !ctx->appended))
        return ctx->fail(FHH_E_STATE, "reserve_clients: ctx holds keys that were not appended");
    if (capacity == 0 || capacity < ctx->n)
        return ctx->fail(FHH_E_ARG, "reserve_clients: capacity below the current client count");
    const uint64_t npad = (capacity + 63) / 64 * 64;
    if (!ctx->appended) ctx->n = ctx->npad = ctx->nw = 0;   // an empty ctx: no layout yet
    if (npad > ctx->npad) {
        rc = relayout_keys(ctx, npad);
        if (rc) return rc;
    }
    ctx->reserved = capacity;
    return FHH_OK;
}

int append_decode(fhh_ctx* ctx, uint64_t m, const uint8_t* recs, uint32_t* herr) {
    int rc = ctx_set_device(ctx);
    if (rc) return rc;
    rc = append_check_state(ctx);
    if (rc) return rc;
    if (!ctx->appended && !ctx->reserved) ctx->n = ctx->npad = ctx->nw = 0;
    const uint64_t c0 = ctx->n, need = (c0 + m + 63) / 64 * 64;
    if (need > ctx->npad) {   // geometric growth: a pitch-changing copy of every buffer
        rc = relayout_keys(ctx, std::max(need, 2 * ctx->npad));
        if (rc == FHH_E_NOMEM && need < 2 * ctx->npad) {   // the doubling does not fit: exactly what is needed
            (void)hipGetLastError();
            rc = relayout_keys(ctx, need);
        }
        if (rc) return rc;
    }
    const uint64_t KB = 25 + 20ull * ctx->L, R = 8 + (uint64_t)ctx->K * KB;
    HIP_TRY(ctx, ctx->app_buf.ensure(8 + m * R + 4));   // whole-dword reads: up to 3 B past the end
    HIP_TRY(ctx, ctx->app_err.ensure(4));
    HIP_TRY(ctx, hipMemsetAsync(ctx->app_err.p, 0, 4, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->app_buf.p, &m, 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->app_buf.as<uint8_t>() + 8, recs, m * R, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, launch_keys_from_bincode_at(ctx->app_buf.as<uint8_t>(), c0, m, ctx->d, ctx->L, (uint32_t)ctx->npad,
                                             (uint32_t)ctx->nw, ctx->cw_seed.as<uint4>(), ctx->cw_bits.as<uint64_t>(),
                                             ctx->root_seed.as<uint4>(), ctx->key_idx.as<uint64_t>(),
                                             ctx->app_err.as<uint32_t>(), ctx->stream));
    *herr = 0;
    HIP_TRY(ctx, hipMemcpyAsync(herr, ctx->app_err.p, 4, hipMemcpyDeviceToHost, ctx->stream));
    return ctx_sync(ctx);
}

void append_commit(fhh_ctx* ctx, uint64_t m) {
    ctx->n += m;
    ctx->dev_keys = true;
    ctx->appended = true;
}

int append_rollback(fhh_ctx* ctx) {
    if ((ctx->n & 63) == 0) return FHH_OK;   // the refused batch shared no word with the clients held
    int rc = ctx_set_device(ctx);
    if (rc) return rc;
    HIP_TRY(ctx, launch_keys_from_bincode_at(ctx->app_buf.as<uint8_t>(), ctx->n, 0, ctx->d, ctx->L, (uint32_t)ctx->npad,
                                             (uint32_t)ctx->nw, ctx->cw_seed.as<uint4>(), ctx->cw_bits.as<uint64_t>(),
                                             ctx->root_seed.as<uint4>(), ctx->key_idx.as<uint64_t>(),
                                             ctx->app_err.as<uint32_t>(), ctx->stream));
    return ctx_sync(ctx);
}

// tree_init on appended keys: the capacity stride becomes the exact one (64 ceil(n / 64), one compacting
// copy unless the capacity already is that) and `valid` is built, so every buffer is what alloc_keys + one
// decode of the whole population leave
int finish_appended(fhh_ctx* ctx) {
    int rc = relayout_keys(ctx, (ctx->n + 63) / 64 * 64);
    if (rc) return rc;
    HIP_TRY(ctx, ctx->valid.ensure(ctx->nw * 8));
    std::vector<uint64_t> v(ctx->nw, ~0ull);
    if (ctx->n % 64) v[ctx->nw - 1] = (1ull << (ctx->n % 64)) - 1;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->valid.p, v.data(), ctx->nw * 8, hipMemcpyHostToDevice, ctx->stream));
    return ctx_sync(ctx);
}

// ---- device keys -> add_keys requests (fhh_export_keys_bincode) -------------------------------
// the refusals both kinds of ctx share; n = the clients on the device(s), have_keys = they are there
int export_bincode_check(fhh_ctx* ctx, bool have_keys, uint64_t n, uint64_t first, uint64_t count, uint64_t batch,
                         const uint8_t* out, uint64_t cap, uint64_t* len) {
    if (!len) return ctx->fail(FHH_E_ARG, "export_keys_bincode: NULL len");
    if (count == 0) return ctx->fail(FHH_E_ARG, "export_keys_bincode: no clients (an empty request is refused by the decoder too)");
    const uint64_t R = be_record_bytes(ctx->d, ctx->L), B = be_batch(count, batch);
    if (count > (~0ull - 8 * be_requests(count, B)) / R) return ctx->fail(FHH_E_ARG, "export_keys_bincode: size overflows");
    *len = be_total_bytes(count, B, R);
    if (!have_keys)
        return ctx->fail(FHH_E_STATE, "export_keys_bincode: no keys on the device (keys staged by fhh_add_keys are "
                                      "uploaded at fhh_tree_init)");
    if (first > n || count > n - first)
        return ctx->fail(FHH_E_ARG, "export_keys_bincode: clients [" + std::to_string(first) + ", " +
                                        std::to_string(first) + " + " + std::to_string(count) + ") of " + std::to_string(n));
    if (!out) return ctx->fail(FHH_E_ARG, "export_keys_bincode: NULL out");
    if (cap < *len)
        return ctx->fail(FHH_E_ARG, "export_keys_bincode: " + std::to_string(*len) + " bytes needed, cap " + std::to_string(cap));
    return FHH_OK;
}

int export_bincode_slice(fhh_ctx* ctx, uint64_t src_first, uint64_t m, uint64_t i0, uint64_t count, uint64_t B,
                         uint8_t* out) {
    if (m == 0) return FHH_OK;
    int rc = ctx_set_device(ctx);
    if (rc) return rc;
    if (!ctx->dev_keys || src_first + m > ctx->n) return ctx->fail(FHH_E_STATE, "export_keys_bincode: slice outside the device keys");
    const uint64_t R = be_record_bytes(ctx->d, ctx->L);
    const uint64_t lo = be_slice_begin(i0, B, R), hi = be_slice_end(i0, m, B, R), org = lo & ~3ull;
    HIP_TRY(ctx, ctx->emit_buf.ensure(hi - org));
    uint8_t* stg = ctx->emit_buf.as<uint8_t>();
    hipEvent_t e0, e1;   // the two emit kernels' time, for fhh_export_timing
    HIP_TRY(ctx, hipEventCreate(&e0));
    HIP_TRY(ctx, hipEventCreate(&e1));
    HIP_TRY(ctx, hipEventRecord(e0, ctx->stream));
    HIP_TRY(ctx, launch_bincode_emit(ctx->cw_seed.as<uint4>(), ctx->cw_bits.as<uint64_t>(), ctx->root_seed.as<uint4>(),
                                     ctx->key_idx.as<uint64_t>(), ctx->d, ctx->L, (uint32_t)ctx->npad, (uint32_t)ctx->nw,
                                     src_first, m, i0, count, B, stg, org, ctx->stream));
    HIP_TRY(ctx, hipEventRecord(e1, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(out + lo, stg + (lo - org), hi - lo, hipMemcpyDeviceToHost, ctx->stream));
    // the stream alone: timing events and pinned staging of a crawl in progress stay pending
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    ctx->emit_ms = ms;
    return FHH_OK;
}

}  // namespace eng
}  // namespace fhh

extern "C" {

int fhh_bincode_request_bytes(uint32_t n_dims, uint32_t data_len, uint64_t count, uint64_t batch, uint64_t* bytes) {
    if (!bytes || count == 0 || n_dims < 1 || n_dims > (uint32_t)kMaxDims || data_len == 0) {
        g_err = "bincode_request_bytes: count = 0, n_dims outside 1..4, data_len = 0 or NULL bytes";
        return FHH_E_ARG;
    }
    const uint64_t R = be_record_bytes(n_dims, data_len), B = be_batch(count, batch);
    if (count > (~0ull - 8 * be_requests(count, B)) / R) {
        g_err = "bincode_request_bytes: size overflows";
        return FHH_E_ARG;
    }
    *bytes = be_total_bytes(count, B, R);
    return FHH_OK;
}

int fhh_export_timing(const fhh_ctx* ctx, double* ms) {
    CTX_CHECK(ctx);
    if (ctx->group || !ms) return const_cast<fhh_ctx*>(ctx)->fail(FHH_E_ARG, "export_timing: a one-GPU ctx and a non-NULL ms");
    *ms = ctx->emit_ms;
    return FHH_OK;
}

int fhh_export_keys_bincode(fhh_ctx* ctx, uint64_t first, uint64_t count, uint64_t batch, uint8_t* out, uint64_t cap,
                            uint64_t* len) {
    CTX_CHECK(ctx);
    if (ctx->group) return group_export_keys_bincode(ctx, first, count, batch, out, cap, len);
    const int rc = export_bincode_check(ctx, ctx->dev_keys && ctx->n, ctx->n, first, count, batch, out, cap, len);
    if (rc) return rc;
    return export_bincode_slice(ctx, first, count, 0, count, be_batch(count, batch), out);
}

int fhh_add_keys_bincode(fhh_ctx* ctx, const uint8_t* req, uint64_t len) {
    CTX_CHECK(ctx);
    if (ctx->group) return group_add_keys_bincode(ctx, req, len);
    int rc = ctx_set_device(ctx);
    if (rc) return rc;
    if (!req || len < 8) return ctx->fail(FHH_E_ARG, "add_keys_bincode: buffer shorter than the u64 length");
    if (ctx->dev_keys || ctx->h_n) return ctx->fail(FHH_E_STATE, "add_keys_bincode: ctx already holds keys");
    uint64_t n = 0;
    for (int i = 0; i < 8; i++) n |= (uint64_t)req[i] << (8 * i);
    const uint64_t KB = 25 + 20ull * ctx->L, R = 8 + (uint64_t)ctx->K * KB;
    if (n == 0) return ctx->fail(FHH_E_ARG, "add_keys_bincode: no clients");
    if (n > (len - 8) / R || 8 + n * R != len)
        return ctx->fail(FHH_E_ARG, "add_keys_bincode: length does not match n clients x n_dims x data_len");
    return add_keys_bincode_records(ctx, n, req + 8);
}

int fhh_reserve_clients(fhh_ctx* ctx, uint64_t capacity) {
    CTX_CHECK(ctx);
    if (ctx->group) return group_reserve_clients(ctx, capacity);
    return append_reserve(ctx, capacity);
}

int fhh_add_keys_bincode_append(fhh_ctx* ctx, const uint8_t* req, uint64_t len) {
    CTX_CHECK(ctx);
    if (ctx->group) return group_add_keys_bincode_append(ctx, req, len);
    int rc = append_check_state(ctx);
    if (rc) return rc;
    if (!req || len < 8) return ctx->fail(FHH_E_ARG, "add_keys_bincode_append: buffer shorter than the u64 length");
    uint64_t m = 0;
    for (int i = 0; i < 8; i++) m |= (uint64_t)req[i] << (8 * i);
    const uint64_t KB = 25 + 20ull * ctx->L, R = 8 + (uint64_t)ctx->K * KB;
    if (m == 0) return ctx->fail(FHH_E_ARG, "add_keys_bincode_append: no clients");
    if (m > (len - 8) / R || 8 + m * R != len)
        return ctx->fail(FHH_E_ARG, "add_keys_bincode_append: length does not match n clients x n_dims x data_len");
    uint32_t herr = 0;
    rc = append_decode(ctx, m, req + 8, &herr);
    if (rc) return rc;
    if (herr) {
        rc = append_rollback(ctx);
        if (rc) return rc;
        return ctx->fail(FHH_E_ARG, "add_keys_bincode_append: " + bincode_malformed_text(herr));
    }
    append_commit(ctx, m);
    return FHH_OK;
}

}  // extern "C"
