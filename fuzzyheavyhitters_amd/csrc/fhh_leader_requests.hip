// Points -> both servers' add_keys request bytes in one kernel (fhh_leader_requests_ball, row i): k_keygen's
// point forms (fhh_kernels.hip) with the serialization of fhh_bincode_out.hip fused in, so that no SoA key buffer
// exists. One wave = 64 clients of one key (dim j, side), lane = client, as k_keygen; the level loop restates
// gen_cor_word (ibDCF.rs:84-119) with the same helpers (ball_src.h, aes0_mmo, prg_ctr / prg_ctrl_bits,
// chacha20_block). Where k_keygen stores cw_seed / cw_bits / root / key_idx, a lane here writes its key's bytes at
// their place in both servers' requests (bincode_emit.h): the 25-byte header (key_idx = the server, its root
// seed, u64 L), the L 20-byte CorWords (composed once, stored twice), and from key 0's lane the client's u64 d
// and, for a client that opens a request, the request's u64 m.
//
// The stage between "lane = client, level by level" and "a client's bytes are contiguous" is the lane's own
// registers: a key's CorWords are one run of 20 L bytes whose byte offset mod 4 is the same at every level (20 is
// a multiple of 4), so the lane keeps the last dword of the previous level group as a carry, funnel-shifts
// (v_alignbit, per-lane shift 8 head) the 5 kLrGroup dwords of a group of kLrGroup levels into aligned dwords and
// stores them as 16-byte vectors at a 4-byte-aligned address. No LDS beside the 64 KiB T-table, so the kernel
// keeps k_keygen's two workgroups of 512 threads per CU.
//
// The rules of fhh_bincode_out.hip hold:
//   Ownership. Every byte of the requests has exactly one writer, the lane of its (client, key). The dword at
//     either end of a key's CorWord run may hold bytes of the key's header or of the next key's header / the
//     next record's u64 d / the next request's u64 m: the <= 3 head and <= 3 tail bytes of the run leave as byte
//     stores, as do all header and count bytes; only dwords that lie entirely inside the run are stored as
//     dwords. Nothing is read back, no atomics but the atomicMin on the carry word.
//   Bounds. A lane's bytes lie in [be_slice_begin(i0), be_slice_end(i0, n)) of the export; lanes of clients
//     >= n write nothing. All offsets are 64-bit.
#include "fhh_internal.h"
#include "aes_ttable.h"
#include "ball_src.h"
#include "bincode_emit.h"

namespace fhh {

__constant__ WordTable c_T0_lr = T0;

// levels of one register group: 5 kLrGroup dwords = 20 kLrGroup contiguous bytes per lane and store burst (a full
// group of a multiple of 4 levels leaves as 16-byte vectors, any other as dwords)
constexpr uint32_t kLrGroup = 4;

// a 16-byte store at a 4-byte-aligned address (global_store_dwordx4)
typedef uint32_t lr_u32x4 __attribute__((ext_vector_type(4), aligned(4)));

__device__ __forceinline__ void lr_put_u64(uint8_t* p, uint64_t v) {
#pragma unroll
    for (int i = 0; i < 8; i++) p[i] = (uint8_t)(v >> (8 * i));
}

template <int SRC>
__global__ __launch_bounds__(kExpandThreads) void k_leader_requests(const LeaderReqArgs a) {
    static_assert(SRC == kKeygenBallBits || SRC == kKeygenCoords, "the point forms only");
    __shared__ uint32_t tbl[kTableWords];
    for (int i = threadIdx.x; i < kTableWords; i += blockDim.x) tbl[i] = c_T0_lr.v[i / kTableReplicas];
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t lanebase = lane * 4;
    const uint64_t wpb = blockDim.x >> 6;
    const uint64_t nwaves = (uint64_t)gridDim.x * wpb;
    const uint32_t K = 2 * a.d, L = a.L;
    const uint64_t nw = (a.n + 63) >> 6;
    const uint64_t items = (uint64_t)K * nw;
    const uint64_t R = be_record_bytes(a.d, L);
    for (uint64_t item = (uint64_t)blockIdx.x * wpb + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); item < items;
         item += nwaves) {
        const uint32_t kk = (uint32_t)(item / nw);
        const uint64_t w = item % nw;
        const uint32_t j = kk >> 1, side_idx = kk & 1;
        const uint32_t side = side_idx == 0 ? 1u : 0u;   // left key: side=true, right: false (ibDCF.rs:170-171)
        const uint64_t c = w * 64 + lane;
        const bool valid = c < a.n;
        const uint8_t* alpha = nullptr;   // kKeygenBallBits: the point's row
        BallBound bound{0u, 0xFFFFFFFFu, false};
        uint32_t nb = 0, cur = 0;
        if constexpr (SRC == kKeygenBallBits) {
            nb = (L + 7) >> 3;
            alpha = a.points + (valid ? (c * a.d + j) * nb : 0);
            if (valid) {
                bound = ball_bound(alpha, L, a.ball, side_idx == 1);
                if (bound.carry_out) atomicMin(a.bad, (unsigned long long)(c * a.d + j));
            }
        } else {
            // L = 16 < 32: every level reads bound.low (ball_bit)
            if (valid) bound.low = coords_bound(reinterpret_cast<const int16_t*>(a.points)[c * 2 + j], j, a.ball, side_idx == 1);
        }

        uint32_t seed[2][4];
        if (!a.root_seeds && valid) {
            uint32_t key[8], blk[16];
#pragma unroll
            for (int k = 0; k < 8; k++) key[k] = a.seed[k];
            chacha20_block(key, (a.seed_first + c) * a.d + j, blk);
            // words 0-7 (left) or 8-15 (right), picked by a mask (as k_keygen: no stack copy of the block)
            const uint32_t right = 0u - side_idx;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                seed[0][k] = blk[k] ^ ((blk[k] ^ blk[8 + k]) & right);
                seed[1][k] = blk[4 + k] ^ ((blk[4 + k] ^ blk[12 + k]) & right);
            }
        } else if (valid) {
            const uint4* rs = reinterpret_cast<const uint4*>(a.root_seeds + ((c * a.d + j) * 2 + side_idx) * 32);
            const uint4 r0 = rs[0], r1 = rs[1];
            seed[0][0] = r0.x; seed[0][1] = r0.y; seed[0][2] = r0.z; seed[0][3] = r0.w;
            seed[1][0] = r1.x; seed[1][1] = r1.y; seed[1][2] = r1.z; seed[1][3] = r1.w;
        } else {
#pragma unroll
            for (int b = 0; b < 2; b++)
#pragma unroll
                for (int k = 0; k < 4; k++) seed[b][k] = 0;
        }

        // where the key goes: its header at koff, its CorWord run of 20 L bytes at koff + 25. The run's first
        // `head` bytes end a dword that the header began; the aligned dwords start at run + head.
        const uint64_t i = a.i0 + c;
        const uint64_t koff = valid ? be_key_off(i, kk, L, a.B, R) - a.org : 0;
        const uint64_t run = koff + 25;   // = be_seg_off(i, kk, 0, ...) - org
        const uint32_t head = be_seg_split(run, 20 * L).head;   // 20 L >= 3: (0 - run) & 3
        const uint32_t sh = 8 * head;
        if (valid) {
#pragma unroll
            for (int b = 0; b < 2; b++) {
                uint8_t* key = a.out[b] + koff;
                key[0] = (uint8_t)b;   // key_idx: server 0 false, server 1 true (ibDCF.rs:153-161)
#pragma unroll
                for (int k = 0; k < 16; k++) key[1 + k] = (uint8_t)(seed[b][k >> 2] >> (8 * (k & 3)));
                lr_put_u64(key + 17, L);
                if (kk == 0) {
                    uint8_t* rec = a.out[b] + (be_client_off(i, a.B, R) - a.org);
                    lr_put_u64(rec, a.d);
                    if (i % a.B == 0) lr_put_u64(rec - 8, be_request_clients(i, a.count, a.B));
                }
            }
        }
        uint32_t t[2] = {0u, 1u};   // root_bits = (false, true), ibDCF.rs:140
        uint32_t carry = 0;         // the run's last dword before the group

        for (uint32_t l0 = 0; l0 < L; l0 += kLrGroup) {
            const uint32_t nl = min(kLrGroup, L - l0);   // wave-uniform
            uint32_t raw[5 * kLrGroup];
#pragma unroll
            for (uint32_t u = 0; u < kLrGroup; u++) {
                if (u >= nl) {
#pragma unroll
                    for (int k = 0; k < 5; k++) raw[5 * u + k] = 0;
                    continue;
                }
                const uint32_t l = l0 + u;
                if (SRC == kKeygenBallBits && valid && (l & 31) == 0 && l + 32 < L) cur = ball_str32(alpha, nb, l);
                const uint32_t bit = valid ? ball_bit(bound, L, l, cur) : 0u;
                uint32_t blk[4][4];   // index b*2 + dir
                uint32_t pbit[4], pyb[4];
#pragma unroll
                for (int b = 0; b < 2; b++)
#pragma unroll
                    for (int dir = 0; dir < 2; dir++) {
                        prg_ctr(seed[b], dir, blk[b * 2 + dir]);
                        prg_ctrl_bits(blk[b * 2 + dir][0], dir, pbit[b * 2 + dir], pyb[b * 2 + dir]);
                    }
                aes0_mmo<DevOps, 4>(blk, tbl, lanebase);

                const uint32_t keep = bit, lose = bit ^ 1u;
                uint32_t cws[4];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const uint32_t x0 = lose ? blk[1][k] : blk[0][k];
                    const uint32_t x1 = lose ? blk[3][k] : blk[2][k];
                    cws[k] = x0 ^ x1;                                    // ibDCF.rs:91
                }
                const uint32_t cb0 = pbit[0] ^ pbit[2] ^ bit ^ 1u;       // :93
                const uint32_t cb1 = pbit[1] ^ pbit[3] ^ bit;            // :94
                const uint32_t cy0 = pyb[0] ^ pyb[2] ^ (bit & (side ^ 1u) & 1u);   // :97 bit & !side
                const uint32_t cy1 = pyb[1] ^ pyb[3] ^ ((bit ^ 1u) & side);        // :98 !bit & side
                const uint32_t cwb_keep = keep ? cb1 : cb0;
#pragma unroll
                for (int b = 0; b < 2; b++) {                            // :103-116
                    const uint32_t tm = 0u - t[b];
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const uint32_t kept = keep ? blk[b * 2 + 1][k] : blk[b * 2][k];
                        seed[b][k] = kept ^ (cws[k] & tm);
                    }
                    t[b] = (keep ? pbit[b * 2 + 1] : pbit[b * 2]) ^ (t[b] & cwb_keep);
                }
                // the serialized CorWord: the seed, then bits.0, bits.1, y_bits.0, y_bits.1 as bools
#pragma unroll
                for (int k = 0; k < 4; k++) raw[5 * u + k] = cws[k];
                raw[5 * u + 4] = cb0 | (cb1 << 8) | (cy0 << 16) | (cy1 << 24);
            }

            // Run dword m (bytes [head + 4 m, head + 4 m + 4) of the run) = (raw[m + 1] : raw[m]) >> 8 head, so a
            // group emits the dwords m = 5 l0 - 1 + k, k < 5 nl, from its own raw dwords and the carry. m = -1
            // holds the run's head bytes (its upper `head` bytes) and leaves as byte stores.
            if (valid) {
                uint32_t o[5 * kLrGroup];
#pragma unroll
                for (uint32_t k = 0; k < 5 * kLrGroup; k++)
                    o[k] = __builtin_amdgcn_alignbit(raw[k], k ? raw[k - 1] : carry, sh);
                const uint64_t at = run + head + 20ull * l0 - 4;   // dword m = 5 l0 - 1; a multiple of 4
                if (l0 != 0 && nl == kLrGroup && (5 * kLrGroup) % 4 == 0) {   // wave-uniform
#pragma unroll
                    for (int b = 0; b < 2; b++) {
                        lr_u32x4* dst = reinterpret_cast<lr_u32x4*>(a.out[b] + at);
#pragma unroll
                        for (uint32_t q = 0; q < 5 * kLrGroup / 4; q++) {
                            lr_u32x4 v;
                            v.x = o[4 * q];
                            v.y = o[4 * q + 1];
                            v.z = o[4 * q + 2];
                            v.w = o[4 * q + 3];
                            dst[q] = v;
                        }
                    }
                } else {
#pragma unroll
                    for (int b = 0; b < 2; b++) {
                        uint8_t* dst = a.out[b] + at;
                        if (l0 == 0) {
                            // bytes 4 - head .. 3 of dword -1 = the run's first `head` bytes = raw[0]'s low bytes
                            for (uint32_t q = 0; q < head; q++) dst[4 - head + q] = (uint8_t)(raw[0] >> (8 * q));
                        } else {
                            *reinterpret_cast<uint32_t*>(dst) = o[0];
                        }
#pragma unroll
                        for (uint32_t k = 1; k < 5 * kLrGroup; k++)
                            if (k < 5 * nl) *reinterpret_cast<uint32_t*>(dst + 4 * k) = o[k];
                    }
                }
            }
            // the last dword of the group's nl levels (a constant index per nl: no dynamic register index)
#pragma unroll
            for (uint32_t u = 0; u < kLrGroup; u++)
                if (u + 1 == nl) carry = raw[5 * u + 4];
        }
        // the run's last dword m = 5 L - 1 = carry >> 8 head: whole where head = 0, else its low 4 - head bytes
        // are the run's tail and the rest belongs to the next owner
        if (valid) {
            const uint64_t at = run + head + 20ull * L - 4;
#pragma unroll
            for (int b = 0; b < 2; b++) {
                uint8_t* dst = a.out[b] + at;
                if (head == 0) {
                    *reinterpret_cast<uint32_t*>(dst) = carry;
                } else {
                    const uint32_t v = carry >> sh;
                    for (uint32_t q = 0; q < 4 - head; q++) dst[q] = (uint8_t)(v >> (8 * q));
                }
            }
        }
    }
}

hipError_t launch_leader_requests(const LeaderReqArgs& a, int src, hipStream_t stream) {
    if (a.n == 0) return hipSuccess;
    // the export must hold the slice and the buffers must be dword aligned (the kernel trusts these)
    if (a.d < 1 || a.d > (uint32_t)kMaxDims || a.L == 0 || a.B == 0 || a.i0 + a.n > a.count || (a.org & 3) ||
        a.org > be_slice_begin(a.i0, a.B, be_record_bytes(a.d, a.L)) || !a.out[0] || !a.out[1] ||
        ((uintptr_t)a.out[0] & 3) || ((uintptr_t)a.out[1] & 3) || !a.points || !a.bad)
        return hipErrorInvalidValue;
    const LeaderReqPlan p = leader_req_plan(a.d, a.n);
    const dim3 grid((unsigned)(p.waves / (kExpandThreads / 64))), block(kExpandThreads);
    switch (src) {
        case kKeygenBallBits:
            hipLaunchKernelGGL(k_leader_requests<kKeygenBallBits>, grid, block, 0, stream, a);
            break;
        case kKeygenCoords:
            hipLaunchKernelGGL(k_leader_requests<kKeygenCoords>, grid, block, 0, stream, a);
            break;
        default:
            return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace fhh
