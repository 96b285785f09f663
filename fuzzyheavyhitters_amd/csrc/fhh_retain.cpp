// fhh_retain_clients: the reference's apply_sketch_results (src/main.rs:68-69) — the clients a keep mask drops
// leave the collection. The survivors are gathered, in their old order, into buffers of the smaller
// collection's exact layout (fhh_retain.hip) and the ctx swaps to them: afterwards it is a collection of n'
// clients, so no later kernel reads a flag or works for a dropped client.
// fhh_retain_clients_device takes the mask where the sketch verification left it, in device memory: the survivor
// list is made there (fhh_retain_mask.hip) and only a 16-byte record comes back before the gather.
#include "fhh_engine.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>

namespace fhh {
namespace eng {

namespace {

// the refusals the host and the device form of the plan word alike
std::string bad_byte_text(uint64_t i, unsigned v) {
    return "keep byte " + std::to_string(i) + " is " + std::to_string(v) + ", not 0 or 1";
}
const char kNoSurvivor[] = "no survivor: a collection of zero clients has no layout (fhh_reset instead)";
const char kNoClient[] = "n = 0: no client to retain";
const char kWideN[] = "n does not fit the engine's u32 client indices";

}  // namespace

bool retain_plan(const uint8_t* keep, uint64_t n, std::vector<uint32_t>& src, std::string* err) {
    auto refuse = [&](const std::string& m) {
        if (err) *err = m;
        return false;
    };
    if (!keep) return refuse("NULL keep");
    if (n == 0) return refuse(kNoClient);
    if (n >> 32) return refuse(kWideN);
    src.clear();
    src.reserve(n);
    for (uint64_t i = 0; i < n; i++) {
        if (keep[i] > 1) return refuse(bad_byte_text(i, keep[i]));
        if (keep[i]) src.push_back((uint32_t)i);
    }
    if (src.empty()) return refuse(kNoSurvivor);
    return true;
}

bool keep_mask_check(const uint8_t* keep_dev, uint64_t n, uint32_t n_rows, uint64_t row_stride, KeepMask& m,
                     std::string* err) {
    auto refuse = [&](const std::string& t) {
        if (err) *err = t;
        return false;
    };
    if (!keep_dev) return refuse("NULL keep_dev");
    if (n == 0) return refuse(kNoClient);
    if (n >> 32) return refuse(kWideN);
    if (n_rows == 0) return refuse("n_rows = 0: a mask has at least one row");
    if (n_rows > 1 && row_stride < n)
        return refuse("row_stride " + std::to_string(row_stride) + " < n = " + std::to_string(n) + ": the rows overlap");
    // a host pointer is refused here, before a kernel could read it; the query's error is sticky otherwise
    hipPointerAttribute_t at{};
    const hipError_t e = hipPointerGetAttributes(&at, keep_dev);
    if (e != hipSuccess) (void)hipGetLastError();
    if (e != hipSuccess || (at.type != hipMemoryTypeDevice && at.type != hipMemoryTypeManaged))
        return refuse("keep_dev is not device memory (a host mask goes to fhh_retain_clients)");
    m.keep = keep_dev;
    m.n = n;
    m.n_rows = n_rows;
    m.row_stride = n_rows == 1 ? n : row_stride;
    m.device = at.device;
    // where the runtime knows the allocation, the rows must lie inside it
    hipDeviceptr_t lo = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&lo, &size, (hipDeviceptr_t)keep_dev) != hipSuccess) {
        (void)hipGetLastError();
    } else {
        const uint64_t off = (uint64_t)(keep_dev - static_cast<const uint8_t*>(lo));
        const uint64_t span = (uint64_t)(n_rows - 1) * m.row_stride + n;
        if (off > size || span > size - off) return refuse("the mask's rows run past the end of keep_dev's allocation");
    }
    return true;
}

int keep_mask_to_host(const KeepMask& m, std::vector<uint8_t>& keep, std::string* err) {
    std::vector<uint8_t> row(m.n);
    keep.assign(m.n, 1);
    uint64_t bad = kKeepNoBad;
    for (uint32_t r = 0; r < m.n_rows; r++) {
        const hipError_t e = hipMemcpy(row.data(), m.keep + (uint64_t)r * m.row_stride, m.n, hipMemcpyDeviceToHost);
        if (e != hipSuccess) {
            if (err) *err = std::string("copying the mask to the host: ") + hipGetErrorString(e);
            return FHH_E_HIP;
        }
        for (uint64_t i = 0; i < m.n; i++) {
            if (row[i] > 1) bad = std::min<uint64_t>(bad, i << 8 | row[i]);
            keep[i] &= row[i];
        }
    }
    if (bad != kKeepNoBad) {
        if (err) *err = bad_byte_text(bad >> 8, (unsigned)(bad & 255));
        return FHH_E_ARG;
    }
    return FHH_OK;
}

bool keep_record_check(const KeepRecord& rec, std::string* err) {
    if (rec.bad != kKeepNoBad) {
        if (err) *err = bad_byte_text(rec.bad >> 8, (unsigned)(rec.bad & 255));
        return false;
    }
    if (rec.n_kept == 0) {
        if (err) *err = kNoSurvivor;
        return false;
    }
    return true;
}

int keep_scan_run(fhh_ctx* ctx, const KeepMask& m, uint64_t first, uint64_t count, KeepScan& ks, KeepRecord& rec) {
    int rc = ctx_set_device(ctx);
    if (rc) return rc;
    const uint64_t nw = (count + 63) / 64;
    // [record | words | counts]: the u64 words first, so that every part is aligned
    HIP_TRY(ctx, ctx->keep_scan.ensure(sizeof(KeepRecord) + nw * 8 + nw * 4));
    KeepRecord* d_rec = ctx->keep_scan.as<KeepRecord>();
    uint64_t* words = reinterpret_cast<uint64_t*>(d_rec + 1);
    uint32_t* base = reinterpret_cast<uint32_t*>(words + nw);
    const uint8_t* keep = m.keep + first;
    uint64_t stride = m.row_stride;
    // FHH_RETAIN_STAGE_MASK (tests): the cross-device copy on a box with one GPU
    const bool stage = m.device != ctx->device || std::getenv("FHH_RETAIN_STAGE_MASK") != nullptr;
    if (stage) HIP_TRY(ctx, ctx->keep_stage.ensure((size_t)m.n_rows * count));
    hipEvent_t ev[2] = {nullptr, nullptr};
    struct EvGuard {
        hipEvent_t* e;
        ~EvGuard() {
            for (int i = 0; i < 2; i++)
                if (e[i]) (void)hipEventDestroy(e[i]);
        }
    } guard{ev};
    for (auto& e : ev) HIP_TRY(ctx, hipEventCreate(&e));
    auto enqueue = [&]() -> int {
        if (stage) {   // the kernels read local memory only: the rows' [first, first + count) bytes come over first
            uint8_t* st = ctx->keep_stage.as<uint8_t>();
            for (uint32_t r = 0; r < m.n_rows; r++)
                HIP_TRY(ctx, hipMemcpyAsync(st + (uint64_t)r * count, keep + (uint64_t)r * stride, count, hipMemcpyDefault,
                                            ctx->stream));
            keep = st;
            stride = count;
        }
        HIP_TRY(ctx, hipEventRecord(ev[0], ctx->stream));
        HIP_TRY(ctx, launch_keep_scan(keep, count, m.n_rows, stride, words, base, d_rec, ctx->stream));
        HIP_TRY(ctx, hipEventRecord(ev[1], ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(&rec, d_rec, sizeof(KeepRecord), hipMemcpyDeviceToHost, ctx->stream));
        return FHH_OK;
    };
    rc = enqueue();
    if (rc) {
        (void)hipStreamSynchronize(ctx->stream);
        return rc;
    }
    rc = ctx_sync(ctx);   // `rec` is written until here
    if (rc) return rc;
    float a = 0.f;
    (void)hipEventElapsedTime(&a, ev[0], ev[1]);
    ctx->keep_ms[0] = a;
    ctx->keep_ms[1] = 0;
    ks.words = words;
    ks.base = base;
    ks.nw = nw;
    return FHH_OK;
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

int retain_prepare(fhh_ctx* ctx, const uint32_t* src, const KeepScan* scan, uint64_t n2, RetainStage& st) {
    if (!ctx->dev_keys) {
        if (!src) return ctx->fail(FHH_E_STATE, "retain_clients: staged keys take the survivor list from the host");
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
    // st.lists = [src | dim 0's rows | ...]: a table's destination row 2 k + s is row 2 live[k] + s of buffer `cur`.
    // src comes from the host, or k_keep_emit writes it in place from the scan of a device mask; the rows (a few
    // entries) are uploaded either way
    std::vector<uint32_t> rows_h;
    size_t rows_off[kMaxDims] = {};
    for (size_t j = 0; st.tables && j < d; j++) {
        rows_off[j] = n2 + rows_h.size();
        for (uint32_t e : ctx->tab[j].live) {
            rows_h.push_back(2 * e);
            rows_h.push_back(2 * e + 1);
        }
    }
    // every destination before the first launch: a refusal for memory leaves nothing half done
    HIP_TRY(ctx, st.cw_seed.ensure(L * K * npad2 * 16));
    HIP_TRY(ctx, st.cw_bits.ensure(L * K * 4 * nw2 * 8));
    HIP_TRY(ctx, st.root_seed.ensure(K * npad2 * 16));
    HIP_TRY(ctx, st.key_idx.ensure(K * nw2 * 8));
    HIP_TRY(ctx, st.valid.ensure(nw2 * 8));
    HIP_TRY(ctx, st.lists.ensure((n2 + rows_h.size()) * 4));
    for (size_t j = 0; st.tables && j < d; j++) {
        st.cap[j] = std::max<size_t>(ctx->tab[j].live.size(), 4);   // table_ensure's floor
        HIP_TRY(ctx, st.seed[j].ensure(st.cap[j] * 2 * npad2 * 16));
        HIP_TRY(ctx, st.t[j].ensure(st.cap[j] * 2 * nw2 * 8));
        HIP_TRY(ctx, st.y[j].ensure(st.cap[j] * 2 * nw2 * 8));
    }
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};   // gathers: 0 .. 1 .. 2; the emit: 3 .. 0
    struct EvGuard {
        hipEvent_t* e;
        ~EvGuard() {
            for (int i = 0; i < 4; i++)
                if (e[i]) (void)hipEventDestroy(e[i]);
        }
    } guard{ev};
    for (auto& e : ev) HIP_TRY(ctx, hipEventCreate(&e));
    std::vector<uint64_t> v(nw2, ~0ull);
    if (n2 % 64) v[nw2 - 1] = (1ull << (n2 % 64)) - 1;
    // from the first copy on, a failure drains the stream before `rows_h`, `v` and the stage's buffers go
    uint64_t col_rows = 0, plane_rows = 0;
    auto enqueue = [&]() -> int {
        uint32_t* lists = st.lists.as<uint32_t>();
        HIP_TRY(ctx, hipMemcpyAsync(st.valid.p, v.data(), nw2 * 8, hipMemcpyHostToDevice, ctx->stream));
        if (!rows_h.empty())
            HIP_TRY(ctx, hipMemcpyAsync(lists + n2, rows_h.data(), rows_h.size() * 4, hipMemcpyHostToDevice, ctx->stream));
        if (src) HIP_TRY(ctx, hipMemcpyAsync(lists, src, n2 * 4, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipEventRecord(ev[3], ctx->stream));
        if (!src) HIP_TRY(ctx, launch_keep_emit(scan->words, scan->base, scan->nw, lists, ctx->stream));
        const uint32_t* idx = lists;
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
    rc = ctx_sync(ctx);   // `src`, `rows_h` and `v` are read until here
    if (rc) return rc;
    float a = 0.f, b = 0.f, c = 0.f;
    (void)hipEventElapsedTime(&a, ev[0], ev[1]);
    (void)hipEventElapsedTime(&b, ev[1], ev[2]);
    if (!src) (void)hipEventElapsedTime(&c, ev[3], ev[0]);
    st.ms[0] = a;
    st.ms[1] = b;
    st.emit_ms = src ? -1 : c;
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
    if (st.emit_ms >= 0) ctx->keep_ms[1] = st.emit_ms;
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
    rc = retain_prepare(ctx, src.data(), nullptr, src.size(), st);
    if (rc) return rc;
    retain_commit(ctx, st);
    return FHH_OK;
}

int fhh_retain_clients_device(fhh_ctx* ctx, const uint8_t* keep_dev, uint64_t n, uint32_t n_rows, uint64_t row_stride,
                              uint64_t* n_kept) {
    CTX_CHECK(ctx);
    if (ctx->group) return group_retain_clients_device(ctx, keep_dev, n, n_rows, row_stride, n_kept);
    // every refusal comes before the ctx is touched, and the count before any device work
    int rc = retain_check_state(ctx);
    if (rc) return rc;
    const uint64_t have = ctx->dev_keys ? ctx->n : ctx->h_n;
    if (n != have)
        return ctx->fail(FHH_E_ARG, "retain_clients: keep.len() " + std::to_string(n) + " != " + std::to_string(have) +
                                        " clients");
    KeepMask m;
    std::string why;
    if (!keep_mask_check(keep_dev, n, n_rows, row_stride, m, &why)) return ctx->fail(FHH_E_ARG, "retain_clients: " + why);
    if (!ctx->dev_keys) {
        // keys still staged by fhh_add_keys live on the host: the mask's n bytes per row join them there and the
        // host call compacts the vectors
        std::vector<uint8_t> keep;
        rc = keep_mask_to_host(m, keep, &why);
        if (rc) return ctx->fail(rc, "retain_clients: " + why);
        rc = fhh_retain_clients(ctx, keep.data(), n);
        if (rc == FHH_OK && n_kept) *n_kept = ctx->h_n;
        return rc;
    }
    KeepScan ks;
    KeepRecord rec{};
    rc = keep_scan_run(ctx, m, 0, n, ks, rec);
    if (rc) return rc;
    if (!keep_record_check(rec, &why)) return ctx->fail(FHH_E_ARG, "retain_clients: " + why);
    if (rec.n_kept != n) {   // else nobody leaves: the collection's buffers are not touched
        RetainStage st;
        rc = retain_prepare(ctx, nullptr, &ks, rec.n_kept, st);
        if (rc) return rc;
        retain_commit(ctx, st);
    }
    if (n_kept) *n_kept = rec.n_kept;
    return FHH_OK;
}

int fhh_retain_plan_device(fhh_ctx* ctx, const uint8_t* keep_dev, uint64_t n, uint32_t n_rows, uint64_t row_stride,
                           uint64_t* n_kept, uint32_t* src) {
    CTX_CHECK(ctx);
    fhh_ctx* c = ctx->group ? group_shard0(ctx) : ctx;   // a multi-device ctx lends its first shard's device and stream
    KeepMask m;
    std::string why;
    if (!keep_mask_check(keep_dev, n, n_rows, row_stride, m, &why)) return ctx->fail(FHH_E_ARG, "retain_plan_device: " + why);
    KeepScan ks;
    KeepRecord rec{};
    int rc = keep_scan_run(c, m, 0, n, ks, rec);
    if (rc) return c == ctx ? rc : ctx->fail(rc, c->err);
    if (!keep_record_check(rec, &why)) return ctx->fail(FHH_E_ARG, "retain_plan_device: " + why);
    if (src) {
        DevBuf idx;
        hipEvent_t ev[2] = {nullptr, nullptr};
        auto emit = [&]() -> int {
            HIP_TRY(ctx, idx.ensure(rec.n_kept * 4));
            for (auto& e : ev) HIP_TRY(ctx, hipEventCreate(&e));
            HIP_TRY(ctx, hipEventRecord(ev[0], c->stream));
            HIP_TRY(ctx, launch_keep_emit(ks.words, ks.base, ks.nw, idx.as<uint32_t>(), c->stream));
            HIP_TRY(ctx, hipEventRecord(ev[1], c->stream));
            HIP_TRY(ctx, hipMemcpyAsync(src, idx.p, rec.n_kept * 4, hipMemcpyDeviceToHost, c->stream));
            return FHH_OK;
        };
        rc = emit();
        if (rc) (void)hipStreamSynchronize(c->stream);
        if (!rc && (rc = ctx_sync(c)) != FHH_OK && c != ctx) ctx->fail(rc, c->err);
        float t = 0.f;
        if (!rc) (void)hipEventElapsedTime(&t, ev[0], ev[1]);
        for (auto& e : ev)
            if (e) (void)hipEventDestroy(e);
        if (rc) return rc;
        c->keep_ms[1] = t;
    }
    for (int i = 0; i < 2; i++) ctx->keep_ms[i] = c->keep_ms[i];
    if (n_kept) *n_kept = rec.n_kept;
    return FHH_OK;
}

int fhh_retain_mask_timing(const fhh_ctx* ctx, double* ms) {
    CTX_CHECK(ctx);
    for (int i = 0; ms && i < 2; i++) ms[i] = ctx->keep_ms[i];
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
