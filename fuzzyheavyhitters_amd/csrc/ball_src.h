// The leader's gen_l_inf_ball (ibDCF.rs:175-188) and gen_l_inf_ball_from_coords (ibDCF.rs:189-205) as arithmetic
// on a client's point: the bits of the two interval bounds that gen_interval (ibDCF.rs:138-173) keys, and the root
// seeds of a (client, dim) from a seed stream. One copy for the host (fhh_ball_bounds, fhh_ball.cpp;
// fhh_audit_probes, fhh_audit.cpp) and for k_keygen's point forms (fhh_kernels.hip), k_leader_requests and k_audit_keys,
// so what the CPU tests hold is what the kernels compute.
//
// BITS form. A point is an L-bit string a, MSB first, packed 8 bits per byte (string bit l = bit 7 - l % 8 of byte
// l / 8). delta = MSB_u32_to_bits(32, size) (ibDCF.rs:178) is 32 bits wide and L >= 32, so
//   left  = subtract_bitstrings(a, delta) = a - delta mod 2^L   (the carry out is dropped, lib.rs:179)
//   right = add_bitstrings(a, delta)      = a + delta           (a carry out adds a bit, lib.rs:146-148, and the
//                                                                leader panics on the lengths, ibDCF.rs:182)
// Only the low 32 bits take part in the add / subtract. A carry (borrow) out of them flips the run of ones (zeros)
// that starts at bit 32 and the first bit above the run, and nothing else: with t the run's length, string bit
// l < L - 32 of the bound is a_l ^ (l >= L - 33 - t). The sum carries out of bit L where the run reaches the top
// (t = L - 32). So a bound is the low word, one threshold and the point's own bits: the L-bit sum is never held.
//
// COORDS form. A point is (lat, long) in i16 centidegrees; the bounds are (c -/+ size) clamped to +-9000 (dim 0) /
// +-18000 (dim 1) (ibDCF.rs:190-193) as 16 bits MSB first, two's complement (i16_to_bitvec,
// sample_driving_data.rs:25-28). Computed in exact integers: the reference's i16 `lat - size` overflows (a panic
// in a debug build, a wrap in release) where |c -/+ size| > 32767; here such a bound clamps like any other.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fhh {

// ---- the seed stream: ChaCha20 (RFC 8439 2.3; 64-bit block counter in words 12-13, nonce 0 in 14-15, the state
// layout of the oracle's orc_chacha_block). Block (seed, ctr) = the 64 root-seed bytes [side][server][16] of
// (client c, dim j) at ctr = (seed_first + c) d + j. Restated here so the OT kernels' 12-round PRG (fhh_ot.hip)
// stays as it is.
__host__ __device__ inline uint32_t ball_rotl(uint32_t x, int n) { return (x << n) | (x >> (32 - n)); }

__host__ __device__ inline void ball_qr(uint32_t& a, uint32_t& b, uint32_t& c, uint32_t& d) {
    a += b; d ^= a; d = ball_rotl(d, 16);
    c += d; b ^= c; b = ball_rotl(b, 12);
    a += b; d ^= a; d = ball_rotl(d, 8);
    c += d; b ^= c; b = ball_rotl(b, 7);
}

// key: the 32 seed bytes as 8 little-endian words; x: the block as 16 little-endian words
__host__ __device__ inline void chacha20_block(const uint32_t* key, uint64_t ctr, uint32_t (&x)[16]) {
    x[0] = 0x61707865u; x[1] = 0x3320646eu; x[2] = 0x79622d32u; x[3] = 0x6b206574u;
#pragma unroll
    for (int k = 0; k < 8; k++) x[4 + k] = key[k];
    x[12] = (uint32_t)ctr;
    x[13] = (uint32_t)(ctr >> 32);
    x[14] = 0u;
    x[15] = 0u;
    for (int r = 0; r < 20; r += 2) {
        ball_qr(x[0], x[4], x[8], x[12]);
        ball_qr(x[1], x[5], x[9], x[13]);
        ball_qr(x[2], x[6], x[10], x[14]);
        ball_qr(x[3], x[7], x[11], x[15]);
        ball_qr(x[0], x[5], x[10], x[15]);
        ball_qr(x[1], x[6], x[11], x[12]);
        ball_qr(x[2], x[7], x[8], x[13]);
        ball_qr(x[3], x[4], x[9], x[14]);
    }
    x[0] += 0x61707865u; x[1] += 0x3320646eu; x[2] += 0x79622d32u; x[3] += 0x6b206574u;
#pragma unroll
    for (int k = 0; k < 8; k++) x[4 + k] += key[k];
    x[12] += (uint32_t)ctr;
    x[13] += (uint32_t)(ctr >> 32);
}

// ---- BITS form ----
// The string bits s .. s + 31 of a packed row of nb = ceil(L / 8) bytes, bit s at bit 31; bytes past the row read
// as 0 (s < L; the bits at and past L are whatever the pad holds, and no caller looks at them).
__host__ __device__ inline uint32_t ball_str32(const uint8_t* row, uint32_t nb, uint32_t s) {
    const uint32_t b0 = s >> 3, sh = s & 7;
    uint64_t acc = 0;
#pragma unroll
    for (uint32_t k = 0; k < 5; k++) {
        const uint32_t b = b0 + k;
        acc = (acc << 8) | ((b < nb && (k < 4 || sh)) ? row[b] : 0u);
    }
    return (uint32_t)(acc >> (8 - sh));
}

struct BallBound {
    uint32_t low;         // the bound's low 32 bits (string bits L - 32 .. L - 1)
    uint32_t flip_from;   // string bit l < L - 32 is the point's bit, flipped where l >= flip_from
    bool carry_out;       // right bound only: a + delta >= 2^L
};

// The length t of the run that a carry (right) or a borrow out of the low word crosses: the ones (zeros) of the
// string bits L - 33, L - 34, ... up to the first zero (one); t = L - 32 where the run reaches the top.
__host__ __device__ inline uint32_t ball_run(const uint8_t* row, uint32_t nb, uint32_t L, bool right) {
    uint32_t hi = L - 32, t = 0;   // the run so far is the string bits hi .. L - 33
    while (hi) {
        const uint32_t cnt = hi < 32 ? hi : 32;
        uint32_t w = ball_str32(row, nb, hi - cnt) >> (32 - cnt);   // string bit hi - 1 at bit 0
        if (right) w = ~w;                                          // a carry runs through ones, a borrow through zeros
        if (cnt < 32) w &= (1u << cnt) - 1;
        if (w) {
            t += (uint32_t)__builtin_ctz(w);
            break;
        }
        t += cnt;
        hi -= cnt;
    }
    return t;
}

// One bound of the point in `row`: right = a + delta, left = a - delta mod 2^L. Reads the row's low word and,
// where a carry or borrow leaves it, the words its run crosses (one word in all but 2^-32 of uniform points).
__host__ __device__ inline BallBound ball_bound(const uint8_t* row, uint32_t L, uint32_t delta, bool right) {
    const uint32_t nb = (L + 7) >> 3;
    const uint32_t a = ball_str32(row, nb, L - 32);
    BallBound r;
    r.low = right ? a + delta : a - delta;
    r.flip_from = 0xFFFFFFFFu;
    r.carry_out = false;
    const bool cb = right ? r.low < a : a < delta;
    if (!cb) return r;
    const uint32_t t = ball_run(row, nb, L, right);
    r.carry_out = right && t == L - 32;
    r.flip_from = t >= L - 33 ? 0u : L - 33 - t;   // the run and the bit above it; a wrap flips them all
    return r;
}

// ---- the audit's probes (fhh_audit_keys_ball, fhh_audit_probes): x_p = l - 1, l, a, r, r + 1 mod 2^L for
// p = 0 .. 4, the points at and around the bounds at which a key pair is evaluated. In the BITS form x_p = a -/+ m
// with m = delta + 1, delta, 0: m has 33 bits at delta = 2^32 - 1, where the low word is the point's own and the
// carry (borrow) into bit 32 is certain. A probe wraps where a bound would carry out (each key is judged alone);
// carry_out still reports it, for p = 3 (the right bound itself).
constexpr uint32_t kAuditProbes = 5;
__host__ __device__ inline BallBound ball_offset(const uint8_t* row, uint32_t L, uint64_t m, bool right) {
    const uint32_t nb = (L + 7) >> 3;
    const uint32_t a = ball_str32(row, nb, L - 32), lo = (uint32_t)m;
    BallBound r;
    r.low = right ? a + lo : a - lo;
    r.flip_from = 0xFFFFFFFFu;
    r.carry_out = false;
    const bool cb = (m >> 32) != 0 || (right ? r.low < a : a < lo);
    if (!cb) return r;
    const uint32_t t = ball_run(row, nb, L, right);
    r.carry_out = right && t == L - 32;
    r.flip_from = t >= L - 33 ? 0u : L - 33 - t;
    return r;
}
__host__ __device__ inline BallBound ball_probe(const uint8_t* row, uint32_t L, uint32_t delta, uint32_t p) {
    const uint64_t m = p == 2 ? 0ull : (uint64_t)delta + ((p == 0 || p == 4) ? 1u : 0u);
    return ball_offset(row, L, m, p > 2);
}

// string bit l of the bound; cur = ball_str32(row, nb, l & ~31u) (unused for l >= L - 32)
__host__ __device__ inline uint32_t ball_bit(const BallBound& b, uint32_t L, uint32_t l, uint32_t cur) {
    if (l + 32 >= L) return (b.low >> (L - 1 - l)) & 1u;
    return ((cur >> (31 - (l & 31))) & 1u) ^ (l >= b.flip_from ? 1u : 0u);
}

// ---- COORDS form: the 16 bound bits of dim j (0 lat, 1 long), bit l of the string at bit 15 - l ----
__host__ __device__ inline uint32_t coords_bound(int16_t c, uint32_t j, uint32_t ball, bool right) {
    const int32_t lim = j == 0 ? 9000 : 18000;
    int32_t v = right ? (int32_t)c + (int32_t)ball : (int32_t)c - (int32_t)ball;
    v = v < -lim ? -lim : (v > lim ? lim : v);
    return (uint32_t)v & 0xFFFFu;
}
// probe p of dim j: the bounds' 16-bit patterns -/+ 1 mod 2^16, and the point's own pattern (i16_to_bitvec(c))
__host__ __device__ inline uint32_t coords_probe(int16_t c, uint32_t j, uint32_t ball, uint32_t p) {
    if (p == 2) return (uint32_t)c & 0xFFFFu;
    const uint32_t b = coords_bound(c, j, ball, p > 2);
    return (p == 0 ? b - 1u : (p == 4 ? b + 1u : b)) & 0xFFFFu;
}

}  // namespace fhh
