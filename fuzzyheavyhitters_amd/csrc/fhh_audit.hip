// k_audit_keys (fhh_audit_keys_ball, row j): do a population's keys mean what its points say? The reference's
// check of one key is eval_ibDCF (ibDCF.rs:238-250) at points around the interval's bounds, as interval_test and
// test_individual_dcfs do (tests/ibdcf_tests.rs); here it runs for every client, both servers' keys side by side.
//
// For client c, dim j, with l and r the bounds the keygen uses (ball_src.h), the probes are x_p = l - 1, l, a, r,
// r + 1 mod 2^L. Each is walked from the root through all L levels with server 0's key and server 1's key
// (eval_init / eval_bit, ibDCF.rs:208-236), each ctx's own copy of the CorWords, and after every level k the
// reconstructed bit e = y0 ^ t0 ^ y1 ^ t1 is compared with [x_p[..k] < l[..k]] (left key) or [x_p[..k] > r[..k]]
// (right key), the top k bits as integers. Every prefix is checked because it costs no AES: a broken CorWord at
// level k then shows with probability 1 - 2^-(L-k) instead of the last level's 1/2.
//
// Shape: k_eval_paths' (fhh_kernels.hip). 1024-thread workgroups share the 128 KiB T-tables, 4 waves per SIMD and so
// 128 VGPRs; one wave = 64 consecutive clients (word w) of one key kk = (dim, side), one lane = one client, items
// dealt grid-stride. What differs is that the direction is the lane's own: it comes from the lane's point by the
// arithmetic of ball_src.h (the probe's low word, the carry's threshold and one 32-bit window of the point per 32
// levels), so the CorWord's control bits are picked per lane from the wave's bit words and t / y are lane values,
// not ballots. The 10 (server, probe) blocks of a level run in five passes over the levels, one probe each: both
// servers' walks of the probe, 2 AES blocks in lockstep per lane. Two probes per pass (k_eval_paths' 4 blocks) do
// not fit: with the per-lane direction, state bits and two ctxs' CorWords beside them the compiler reports 128
// VGPRs and 10 to 39 spilled. Every pass reloads the CorWords: 16 B of CorWord seed per AES block
// where k_eval_paths reads 4. Level l + 1's CorWords of both ctxs are requested before level l's AES; the level's
// own CorWord goes into the feed-forward before the AES (aes0_mmo_tab_ff) so that it is dead by then.
//
// What the AES is for. No compared bit depends on a seed: expand_dir reads its control bits from the nibble it
// has just zeroed (prg.rs:97-104), so tau's bits are constants and t / y follow from key_idx and the CorWords'
// control bits alone. The seeds are walked because eval_bit walks them, and they are looked at once, at the end:
// a walk that has left its key's path (t0 == t1) must end with both servers' seeds equal. Walks for which that
// fails are counted apart (rec[4], fhh_audit_seed_check); they do not touch the ok bytes, whose rule stays: a
// client is ok iff all its 2d 5 L comparisons hold.
//
// Failures leave through vector stores and atomics only: the client's ok byte is cleared, an atomicMin on the
// packed (client, dim, side, probe, level) gives the lowest failure, one atomicAdd per item counts the comparisons
// made (so a skipped item cannot pass as ok). Lanes past n walk the padding's keys and compare nothing.
#include "fhh_internal.h"
#include "expand_kernel.h"
#include "ball_src.h"

namespace fhh {

__constant__ WordTable c_T0_audit = T0;

using ExpandTab = Tab4T32<DevOpsX>;
// probes per pass over the levels: 2 kAuditPassProbes AES blocks (both servers' walks) in lockstep per lane
constexpr int kAuditPassProbes = 1;
static_assert(kAuditProbes % kAuditPassProbes == 0, "whole passes");

// p[i] for a wave-uniform i, of words no kernel of this launch writes: a scalar load (constant address space)
template <typename T>
__device__ __forceinline__ T audit_uniform_load(const T* p, size_t i) {
    return ((const __attribute__((address_space(4))) T*)p)[i];
}

// probe p of the lane's (client, dim): BITS the point's row, COORDS its int16
template <int FORM>
__device__ __forceinline__ BallBound audit_probe(const AuditArgs& a, const uint8_t* row, uint32_t j, uint32_t p, bool valid) {
    BallBound r{0u, 0xFFFFFFFFu, false};
    if (valid) {
        if constexpr (FORM == kKeygenBallBits) r = ball_probe(row, a.L, a.ball, p);
        else r.low = coords_probe(*reinterpret_cast<const int16_t*>(row), j, a.ball, p);   // L = 16: ball_bit reads low
    }
    return r;
}

// the lane's own control bits of a CorWord from the wave's four bit words: bits.0, bits.1, y_bits.0, y_bits.1 at
// bits 0 .. 3
__device__ __forceinline__ uint32_t audit_nibble(const uint64_t (&q)[4], uint32_t lane) {
    uint32_t v = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) v |= ((uint32_t)(q[k] >> lane) & 1u) << k;
    return v;
}

// Probes [P0, P0 + NP) of one item, all L levels; the probes are made here, per pass, so that only a pass's own
// stay in registers. Returns `fail`: 0, or the lane's first failure as probe << 19 | level << 1 | expected.
template <int FORM, int NP>
__device__ __forceinline__ uint32_t audit_pass(const AuditArgs& a, const uint32_t* tbl, uint32_t b0, uint32_t b1,
                                               uint32_t lane, uint32_t kk, uint32_t w, uint32_t c, bool valid,
                                               const uint8_t* row, uint32_t P0, uint32_t fail, uint32_t& diverged) {
    const uint32_t L = a.L, nb = (L + 7) >> 3, j = kk >> 1, side_idx = kk & 1u;
    BallBound pr[NP];
#pragma unroll
    for (int q = 0; q < NP; q++) pr[q] = audit_probe<FORM>(a, row, j, P0 + q, valid);
    // the probe the key's interval ends at: l for the left key, r for the right
    const BallBound bound = audit_probe<FORM>(a, row, j, side_idx == 0 ? 1u : 3u, valid);
    // eval_init (ibDCF.rs:229-236): seed = root_seed, t = y = key_idx. The state bits of the pass's 2 NP walks
    // are packed into one register: t of (server b, probe q) at bit b NP + q, y at bit 8 + b NP + q.
    uint32_t sd[2 * NP][4], ty = 0, nib[2];
    uint4 cw[2];
#pragma unroll
    for (int b = 0; b < 2; b++) {
        const AuditSrv& S = a.srv[b];
        const uint4 root = S.root_seed[(size_t)kk * S.npad + c];
        const uint32_t kb = (uint32_t)(audit_uniform_load(S.key_idx, (size_t)kk * S.nw + w) >> lane) & 1u;
#pragma unroll
        for (int q = 0; q < NP; q++) {
            const int i = b * NP + q;
            sd[i][0] = root.x; sd[i][1] = root.y; sd[i][2] = root.z; sd[i][3] = root.w;
            ty |= (kb << i) | (kb << (8 + i));
        }
        cw[b] = S.cw_seed[(size_t)kk * S.npad + c];
        uint64_t q4[4];
#pragma unroll
        for (int k = 0; k < 4; k++) q4[k] = audit_uniform_load(S.cw_bits, ((size_t)kk * 4 + k) * S.nw + w);
        nib[b] = audit_nibble(q4, lane);
    }
    uint32_t undecided = (1u << NP) - 1u, expect = 0u;   // per probe: prefix equal to the bound's so far; the rule's bit
    uint32_t cur = 0;
    for (uint32_t l = 0; l < L; l++) {
        if (FORM == kKeygenBallBits && (l & 31u) == 0 && l + 32 < L) cur = valid ? ball_str32(row, nb, l) : 0u;
        const uint32_t bb = ball_bit(bound, L, l, cur);
        uint32_t dir[NP], blk[2 * NP][4];
#pragma unroll
        for (int q = 0; q < NP; q++) dir[q] = ball_bit(pr[q], L, l, cur);
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int q = 0; q < NP; q++) {
                const int i = b * NP + q;
                prg_ctr(sd[i], (int)dir[q], blk[i]);
                // `if state.bit { seed ^= cw.seed }` (ibDCF.rs:213-215) goes in with the feed-forward, so that the
                // level's CorWord is dead before the AES
                const uint32_t tm = 0u - ((ty >> i) & 1u);
                sd[i][0] = blk[i][0] ^ (cw[b].x & tm);
                sd[i][1] = blk[i][1] ^ (cw[b].y & tm);
                sd[i][2] = blk[i][2] ^ (cw[b].z & tm);
                sd[i][3] = blk[i][3] ^ (cw[b].w & tm);
            }
        // the next level's CorWords (ibDCF.rs:215-217 `cor_words[state.level]`), off the dependent chain: the
        // seeds into registers, the bit words into scalars that become the lane's nibble after the AES
        uint64_t cwpn[2][4] = {};
        const bool more = l + 1 < L;
        if (more) {
#pragma unroll
            for (int b = 0; b < 2; b++) {
                const AuditSrv& S = a.srv[b];
                const size_t krow = (size_t)(l + 1) * a.K + kk;
                cw[b] = S.cw_seed[krow * S.npad + c];
#pragma unroll
                for (int k = 0; k < 4; k++) cwpn[b][k] = audit_uniform_load(S.cw_bits, (krow * 4 + k) * S.nw + w);
            }
        }
        aes0_mmo_tab_ff<DevOpsX, ExpandTab, 2 * NP>(blk, sd, tbl, b0, b1);
        uint32_t ty2 = 0;
#pragma unroll
        for (int b = 0; b < 2; b++) {
#pragma unroll
            for (int q = 0; q < NP; q++) {
                const int i = b * NP + q;
                uint32_t pb, py;
                prg_ctrl_bits(blk[i][0], (int)dir[q], pb, py);
                // new_bit = tau.bits[dir] ^ (t & cw.bits[dir]);
                // new_y = tau.y_bits[dir] ^ (t & cw.y_bits[dir]) ^ y   (ibDCF.rs:211-219)
                const uint32_t t = (ty >> i) & 1u, y = (ty >> (8 + i)) & 1u;
                const uint32_t cwb = (nib[b] >> dir[q]) & 1u, cwy = (nib[b] >> (2 + dir[q])) & 1u;
                ty2 |= ((pb ^ (t & cwb)) << i) | ((py ^ (t & cwy) ^ y) << (8 + i));
            }
            if (more) nib[b] = audit_nibble(cwpn[b], lane);
        }
        ty = ty2;
#pragma unroll
        for (int q = 0; q < NP; q++) {
            // the rule after level l + 1: the first bit at which the probe leaves the bound decides it for good.
            // Left key: x < l iff the bound's bit is the 1; right key: x > r iff the probe's bit is.
            const uint32_t differs = dir[q] ^ bb, first = (undecided >> q) & differs;
            expect |= (first & (side_idx == 0 ? bb : dir[q])) << q;
            undecided &= ~(differs << q);
            // e = y0 ^ t0 ^ y1 ^ t1
            const uint32_t e = ((ty >> q) ^ (ty >> (NP + q)) ^ (ty >> (8 + q)) ^ (ty >> (8 + NP + q))) & 1u;
            const uint32_t want = (expect >> q) & 1u;
            if (valid && e != want && fail == 0) fail = ((P0 + q) << 19) | ((l + 1) << 1) | want;
        }
    }
    // A walk that has left the key's path ends with t0 == t1, and then with s0 == s1: the CorWord that both servers
    // applied where it left cancels their seeds' difference (ibDCF.rs:91). No compared bit depends on a seed
    // (expand_dir reads its control bits from the nibble it has just zeroed, prg.rs:97-104), so this is the one
    // place where CorWord seeds and root seeds that do not belong together show.
#pragma unroll
    for (int q = 0; q < NP; q++) {
        const uint32_t ds = (sd[q][0] ^ sd[NP + q][0]) | (sd[q][1] ^ sd[NP + q][1]) | (sd[q][2] ^ sd[NP + q][2]) |
                            (sd[q][3] ^ sd[NP + q][3]);
        if (valid && (((ty >> q) ^ (ty >> (NP + q))) & 1u) == 0 && ds != 0) diverged++;
    }
    return fail;
}

template <int FORM>
__global__ __launch_bounds__(kAuditBlock, 1) void k_audit_keys(AuditArgs a) {
    static_assert(FORM == kKeygenBallBits || FORM == kKeygenCoords, "the point forms only");
    __shared__ uint32_t tbl[ExpandTab::kWords];
    for (int i = threadIdx.x; i < ExpandTab::kWords; i += kAuditBlock) tbl[i] = ExpandTab::word(c_T0_audit.v, i);
    __syncthreads();

    const uint32_t lane = threadIdx.x & 63;
    uint32_t b0, b1;
    ExpandTab::bases(lane, b0, b1);
    const uint64_t wpb = kAuditBlock / 64;
    const uint64_t nwaves = (uint64_t)gridDim.x * wpb;
    const uint64_t nwc = (a.n + 63) >> 6;   // the words that hold clients (a layout's nw may be a capacity)
    const uint64_t items = (uint64_t)a.K * nwc;
    for (uint64_t item = (uint64_t)blockIdx.x * wpb + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); item < items;
         item += nwaves) {
        // item = kk nwc + word: a workgroup's waves read neighbouring words of one CorWord row
        const uint32_t kk = (uint32_t)(item / nwc), w = (uint32_t)(item % nwc);
        const uint32_t j = kk >> 1, side_idx = kk & 1u;
        const uint64_t c64 = (uint64_t)w * 64 + lane;
        const uint32_t c = (uint32_t)c64;
        const bool valid = c64 < a.n;   // lanes past n read no point and store nothing
        const uint64_t pidx = valid ? c64 * a.d + j : 0;
        const uint8_t* row = a.points + pidx * (FORM == kKeygenBallBits ? (a.L + 7) >> 3 : 2u);
        if (FORM == kKeygenBallBits && side_idx == 1 && valid && ball_probe(row, a.L, a.ball, 3).carry_out)
            atomicMin(a.rec + 2, (unsigned long long)pidx);
        uint32_t fail = 0, diverged = 0;
        for (uint32_t p = 0; p < kAuditProbes; p += kAuditPassProbes)
            fail = audit_pass<FORM, kAuditPassProbes>(a, tbl, b0, b1, lane, kk, w, c, valid, row, p, fail, diverged);
        if (diverged) atomicAdd(a.rec + 4, (unsigned long long)diverged);
        if (fail) {
            a.ok[c64] = 0;
            atomicMin(a.rec, ((unsigned long long)c64 << 25) | ((unsigned long long)j << 23) |
                                 ((unsigned long long)side_idx << 22) | fail);
        }
        const uint64_t live = __ballot(valid);
        if (lane == 0) atomicAdd(a.rec + 1, (unsigned long long)__popcll(live) * kAuditProbes * a.L);
    }
}

// rec[3] = the clients whose ok byte was cleared (several keys of a client may clear the same byte)
__global__ void k_audit_count(const uint8_t* ok, uint64_t n, unsigned long long* rec) {
    uint64_t bad = 0;
    const uint64_t n64 = (n + 63) & ~63ull;   // whole waves reach the ballot
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n64; i += (uint64_t)gridDim.x * blockDim.x)
        bad += (uint64_t)__popcll(__ballot(i < n && ok[i] == 0));
    if ((threadIdx.x & 63) == 0 && bad) atomicAdd(rec + 3, (unsigned long long)bad);
}

hipError_t launch_audit_keys(const AuditArgs& a, int form, int grid_blocks, hipStream_t stream) {
    const AuditPlan p = audit_plan(a.d, a.L, a.n, (uint64_t)(grid_blocks > 0 ? grid_blocks : 1));
    if (p.items == 0) return hipSuccess;
    const dim3 grid((unsigned)p.blocks), block(kAuditBlock);
    switch (form) {
        case kKeygenBallBits:
            hipLaunchKernelGGL(k_audit_keys<kKeygenBallBits>, grid, block, 0, stream, a);
            break;
        case kKeygenCoords:
            hipLaunchKernelGGL(k_audit_keys<kKeygenCoords>, grid, block, 0, stream, a);
            break;
        default:
            return hipErrorInvalidValue;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    uint64_t cb = (a.n + 255) / 256;
    if (cb > 1024) cb = 1024;
    hipLaunchKernelGGL(k_audit_count, dim3((unsigned)cb), dim3(256), 0, stream, a.ok, a.n, a.rec);
    return hipGetLastError();
}

}  // namespace fhh
