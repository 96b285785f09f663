// fhh_audit_keys_ball(_device) / fhh_audit_probes / fhh_audit_plan (row j): the audit of a population's keys
// against its points. The kernel (k_audit_keys, fhh_audit.hip) walks both servers' keys of every client at the
// five probes of its point and compares every prefix's reconstructed bit with the interval rule; this file holds
// the call around it — the refusals, the staging of the points, the report — and the same probe and launch
// arithmetic on the host with no GPU, which is what the device path means (as fhh_ball_bounds is for the keygen).
#include "fhh_engine.h"

#include <cstring>

#include "ball_src.h"

namespace fhh {
namespace eng {

namespace {

constexpr size_t kAuditOkOff = 64;   // the ok bytes' offset in audit_buf, after the record

int audit_ctx_ready(fhh_ctx* c, uint64_t n) {
    int rc = upload_staged(c);
    if (rc) return rc;
    if (!c->dev_keys || c->n == 0) return c->fail(FHH_E_STATE, "audit_keys_ball: the ctx holds no keys");
    if (c->n != n)
        return c->fail(FHH_E_ARG, "audit_keys_ball: n = " + std::to_string(n) + " but the ctx holds " + std::to_string(c->n) +
                                      " clients");
    return FHH_OK;
}

void report_from(const AuditOut& o, fhh_audit_report* rep) {
    std::memset(rep, 0, sizeof(*rep));
    rep->n_checks = o.n_checks;
    rep->n_bad_clients = o.n_bad;
    rep->first_client = ~0ull;
    if (o.first == ~0ull) return;
    rep->first_client = o.first >> 25;
    rep->first_dim = (uint32_t)(o.first >> 23) & 3u;
    rep->first_side = (uint32_t)(o.first >> 22) & 1u;
    rep->first_probe = (uint32_t)(o.first >> 19) & 7u;
    rep->first_level = (uint32_t)(o.first >> 1) & kAuditMaxLevels;
    rep->expected = (uint32_t)o.first & 1u;
    rep->got = rep->expected ^ 1u;
}

// the refusals that need no device, on the leading ctx
int audit_check_args(fhh_ctx* c0, fhh_ctx* c1, uint64_t n, const fhh_ball_src* src, const void* rep) {
    if (c0->d != c1->d || c0->L != c1->L) return c0->fail(FHH_E_ARG, "audit_keys_ball: ctxs differ in d / L");
    if (!rep) return c0->fail(FHH_E_ARG, "audit_keys_ball: NULL report");
    std::string why;
    if (!ball_src_check(c0->d, c0->L, n, src, &why)) return c0->fail(FHH_E_ARG, "audit_keys_ball: " + why);
    if (c0->L > kAuditMaxLevels)
        return c0->fail(FHH_E_ARG, "audit_keys_ball: data_len " + std::to_string(c0->L) + " >= 2^18");
    if (n == 0) return c0->fail(FHH_E_STATE, "audit_keys_ball: the ctx holds no keys");
    return FHH_OK;
}

}  // namespace

int audit_copy_ok(fhh_ctx* c0, uint64_t n, uint8_t* ok_host);

int audit_keys_one(fhh_ctx* c0, fhh_ctx* c1, uint64_t n, const fhh_ball_src* src, uint64_t client_off, uint8_t* ok_host,
                   AuditOut* out) {
    if (c0->device != c1->device) return c0->fail(FHH_E_ARG, "audit_keys_ball: ctxs on different devices");
    int rc = ctx_set_device(c0);
    if (rc) return rc;
    rc = audit_ctx_ready(c0, n);
    if (rc) return rc;
    rc = audit_ctx_ready(c1, n);
    if (rc) return c0->fail(rc, c1->err);
    const uint32_t d = c0->d, L = c0->L;
    // buffers of the call's own (no buffer a crawl uses): [record | ok | points]
    const size_t pb = n * d * point_bytes(src->form, L), p_off = kAuditOkOff + ((n + 15) & ~(size_t)15);
    HIP_TRY(c0, c0->audit_buf.ensure(p_off + pb));
    uint8_t* st = c0->audit_buf.as<uint8_t>();
    // server 1's keys may still be in flight on its own stream
    if (c1->stream != c0->stream) HIP_TRY(c1, hipStreamSynchronize(c1->stream));
    // the record: the lowest failure and the carry word preset to ~0, the counts to 0
    HIP_TRY(c0, hipMemsetAsync(st, 0, kAuditRecWords * 8, c0->stream));
    HIP_TRY(c0, hipMemsetAsync(st, 0xFF, 8, c0->stream));
    HIP_TRY(c0, hipMemsetAsync(st + 16, 0xFF, 8, c0->stream));
    HIP_TRY(c0, hipMemsetAsync(st + kAuditOkOff, 1, n, c0->stream));
    HIP_TRY(c0, hipMemcpyAsync(st + p_off, src->points, pb, hipMemcpyHostToDevice, c0->stream));
    AuditArgs a{};
    fhh_ctx* cs[2] = {c0, c1};
    for (int b = 0; b < 2; b++) {
        a.srv[b].cw_seed = cs[b]->cw_seed.as<uint4>();
        a.srv[b].cw_bits = cs[b]->cw_bits.as<uint64_t>();
        a.srv[b].root_seed = cs[b]->root_seed.as<uint4>();
        a.srv[b].key_idx = cs[b]->key_idx.as<uint64_t>();
        a.srv[b].npad = (uint32_t)cs[b]->npad;   // an appended layout's capacity stride until tree_init
        a.srv[b].nw = (uint32_t)cs[b]->nw;
    }
    a.points = st + p_off;
    a.ok = st + kAuditOkOff;
    a.rec = reinterpret_cast<unsigned long long*>(st);
    a.n = n;
    a.d = d;
    a.L = L;
    a.K = c0->K;
    a.ball = src->ball;
    hipEvent_t e0, e1;
    HIP_TRY(c0, hipEventCreate(&e0));
    HIP_TRY(c0, hipEventCreate(&e1));
    HIP_TRY(c0, hipEventRecord(e0, c0->stream));
    HIP_TRY(c0, launch_audit_keys(a, src->form == FHH_BALL_BITS ? kKeygenBallBits : kKeygenCoords, c0->grid, c0->stream));
    HIP_TRY(c0, hipEventRecord(e1, c0->stream));
    unsigned long long rec[kAuditRecWords];
    HIP_TRY(c0, hipMemcpyAsync(rec, st, sizeof(rec), hipMemcpyDeviceToHost, c0->stream));
    // the stream alone: timing events and pinned staging of a crawl in progress stay pending
    HIP_TRY(c0, hipStreamSynchronize(c0->stream));
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (rec[2] != ~0ull)
        return c0->fail(FHH_E_ARG, "audit_keys_ball: " + carry_text(rec[2] + client_off * d, d, L));
    if (ok_host) {
        rc = audit_copy_ok(c0, n, ok_host);
        if (rc) return rc;
    }
    c0->audit_ms = ms;
    c0->audit_diverged = rec[4];
    out->n_checks = rec[1];
    out->n_bad = rec[3];
    out->diverged = rec[4];
    out->first = rec[0] == ~0ull ? ~0ull : rec[0] + (client_off << 25);
    return FHH_OK;
}

// the ok bytes of c0's last audit of n clients, to the host
int audit_copy_ok(fhh_ctx* c0, uint64_t n, uint8_t* ok_host) {
    int rc = ctx_set_device(c0);
    if (rc) return rc;
    HIP_TRY(c0, hipMemcpyAsync(ok_host, c0->audit_buf.as<uint8_t>() + kAuditOkOff, n, hipMemcpyDeviceToHost, c0->stream));
    HIP_TRY(c0, hipStreamSynchronize(c0->stream));
    return FHH_OK;
}

}  // namespace eng
}  // namespace fhh

extern "C" {

int fhh_audit_keys_ball(fhh_ctx* c0, fhh_ctx* c1, uint64_t n, const fhh_ball_src* src, uint8_t* ok, fhh_audit_report* rep) {
    if (!c0 || !c1) {
        g_err = "null fhh_ctx";
        return FHH_E_ARG;
    }
    if (!c0->group != !c1->group)
        return c0->fail(FHH_E_ARG, "audit_keys_ball: a multi-device ctx and a one-GPU ctx");
    int rc = audit_check_args(c0, c1, n, src, rep);
    if (rc) return rc;
    AuditOut o;
    rc = c0->group ? group_audit_keys_ball(c0, c1, n, src, ok, &o) : audit_keys_one(c0, c1, n, src, 0, ok, &o);
    if (rc) return rc;
    report_from(o, rep);
    return FHH_OK;
}

int fhh_audit_keys_ball_device(fhh_ctx* c0, fhh_ctx* c1, uint64_t n, const fhh_ball_src* src, const uint8_t** ok_dev,
                               fhh_audit_report* rep) {
    if (!c0 || !c1) {
        g_err = "null fhh_ctx";
        return FHH_E_ARG;
    }
    if (c0->group || c1->group)
        return c0->fail(FHH_E_ARG, "audit_keys_ball_device: a multi-device ctx has no one device to leave the ok bytes "
                                   "on (fhh_shard_ctx, or the host-output form)");
    if (!ok_dev) return c0->fail(FHH_E_ARG, "audit_keys_ball_device: NULL ok_dev");
    int rc = audit_check_args(c0, c1, n, src, rep);
    if (rc) return rc;
    AuditOut o;
    rc = audit_keys_one(c0, c1, n, src, 0, nullptr, &o);
    if (rc) return rc;
    *ok_dev = c0->audit_buf.as<uint8_t>() + kAuditOkOff;
    report_from(o, rep);
    return FHH_OK;
}

int fhh_audit_probes(uint32_t n_dims, uint32_t data_len, uint64_t n, const fhh_ball_src* src, uint8_t* probes,
                     uint64_t* bad) {
    if (bad) *bad = ~0ull;
    std::string why;
    if (!ball_src_check(n_dims, data_len, n, src, &why)) {
        g_err = "audit_probes: " + why;
        return FHH_E_ARG;
    }
    const uint64_t L = data_len, items = n * n_dims;
    const size_t nb = point_bytes(src->form, data_len);
    const uint8_t* pts = static_cast<const uint8_t*>(src->points);
    if (src->form == FHH_BALL_BITS) {   // a carry out refuses the call before anything is written
        for (uint64_t i = 0; i < items; i++)
            if (ball_probe(pts + i * nb, data_len, src->ball, 3).carry_out) {
                if (bad) *bad = i;
                g_err = "audit_probes: " + carry_text(i, n_dims, data_len);
                return FHH_E_ARG;
            }
    }
    if (!probes) return FHH_OK;
    for (uint64_t i = 0; i < items; i++)
        for (uint32_t p = 0; p < kAuditProbes; p++) {
            uint8_t* o = probes + (i * kAuditProbes + p) * L;
            if (src->form == FHH_BALL_BITS) {
                const uint8_t* row = pts + i * nb;
                const BallBound b = ball_probe(row, data_len, src->ball, p);
                uint32_t cur = 0;
                for (uint32_t l = 0; l < data_len; l++) {
                    if ((l & 31) == 0 && l + 32 < data_len) cur = ball_str32(row, (uint32_t)nb, l);
                    o[l] = (uint8_t)ball_bit(b, data_len, l, cur);
                }
            } else {
                const int16_t c = static_cast<const int16_t*>(src->points)[i];
                const uint32_t v = coords_probe(c, (uint32_t)(i % 2), src->ball, p);
                for (uint32_t l = 0; l < 16; l++) o[l] = (uint8_t)((v >> (15 - l)) & 1u);
            }
        }
    return FHH_OK;
}

int fhh_audit_plan(uint32_t n_dims, uint32_t data_len, uint64_t n, uint64_t grid_blocks, uint64_t* items, uint64_t* waves,
                   uint64_t* trips, uint64_t* last_trip_items, uint64_t* aes_blocks, uint64_t* n_checks) {
    if (n_dims < 1 || n_dims > (uint32_t)kMaxDims || data_len == 0 || n == 0 || grid_blocks == 0) {
        g_err = "audit_plan: n_dims outside 1..4, data_len = 0, n = 0 or grid_blocks = 0";
        return FHH_E_ARG;
    }
    const AuditPlan p = audit_plan(n_dims, data_len, n, grid_blocks);
    if (items) *items = p.items;
    if (waves) *waves = p.waves;
    if (trips) *trips = p.trips;
    if (last_trip_items) *last_trip_items = p.last_trip_items;
    if (aes_blocks) *aes_blocks = p.aes_blocks;
    if (n_checks) *n_checks = p.n_checks;
    return FHH_OK;
}

int fhh_audit_timing(const fhh_ctx* ctx, double* ms) {
    CTX_CHECK(ctx);
    if (!ms) return const_cast<fhh_ctx*>(ctx)->fail(FHH_E_ARG, "audit_timing: NULL ms");
    *ms = ctx->audit_ms;
    return FHH_OK;
}

int fhh_audit_seed_check(const fhh_ctx* ctx, uint64_t* n_diverged) {
    CTX_CHECK(ctx);
    if (!n_diverged) return const_cast<fhh_ctx*>(ctx)->fail(FHH_E_ARG, "audit_seed_check: NULL n_diverged");
    *n_diverged = ctx->audit_diverged;
    return FHH_OK;
}

}  // extern "C"
