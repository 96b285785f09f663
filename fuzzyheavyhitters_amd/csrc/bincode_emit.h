// Span arithmetic of serialized add_keys requests (k_bincode_emit_cw / k_bincode_emit_headers in
// fhh_bincode_out.hip, fhh_export_keys_bincode), the counterpart of bincode_span.h: `count` clients leave as
// ceil(count / B) consecutive AddKeysRequest.keys payloads (rpc.rs:12-15, bincode 1.x legacy), request q =
// u64 m_q, then the m_q records of clients q B .. q B + m_q - 1 of the export, each u64 d and 2 d ibDCFKeys of
// 25 + 20 L bytes (key_idx bool, root seed, u64 L, L x 20-byte CorWord). Client i of the export (i = c - first)
// starts at off(i) = 8 (floor(i / B) + 1) + i R. A key's CorWords of one level block are one contiguous
// segment at an arbitrary byte offset: be_seg_split cuts it into <= 3 head bytes, whole aligned dwords and
// <= 3 tail bytes, so that no writer ever touches a byte outside its own segment. Host self-test
// tests/host/bincode_emit_host_test.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fhh {

constexpr uint32_t kBeLevels = 32;   // levels of one CW segment (the decoder's kBcLevels)

// one serialized ibDCFKey / one client record
__host__ __device__ __forceinline__ uint64_t be_key_bytes(uint32_t L) { return 25 + 20ull * L; }
__host__ __device__ __forceinline__ uint64_t be_record_bytes(uint32_t d, uint32_t L) {
    return 8 + 2ull * d * be_key_bytes(L);
}

// clients per request: batch = 0 is one request of all `count` clients
__host__ __device__ __forceinline__ uint64_t be_batch(uint64_t count, uint64_t batch) { return batch ? batch : count; }
__host__ __device__ __forceinline__ uint64_t be_requests(uint64_t count, uint64_t B) { return (count + B - 1) / B; }
__host__ __device__ __forceinline__ uint64_t be_total_bytes(uint64_t count, uint64_t B, uint64_t R) {
    return 8 * be_requests(count, B) + count * R;
}

// record of client i of the export; the u64 m of the request that i opens (i % B == 0) sits 8 bytes before it
__host__ __device__ __forceinline__ uint64_t be_client_off(uint64_t i, uint64_t B, uint64_t R) {
    return 8 * (i / B + 1) + i * R;
}
// clients of the request that client i opens
__host__ __device__ __forceinline__ uint64_t be_request_clients(uint64_t i, uint64_t count, uint64_t B) {
    return count - i < B ? count - i : B;
}
// first byte that the owner of clients [i0, ...) writes: its first client's record, or the request count before it
__host__ __device__ __forceinline__ uint64_t be_slice_begin(uint64_t i0, uint64_t B, uint64_t R) {
    return be_client_off(i0, B, R) - (i0 % B == 0 ? 8 : 0);
}
// one past the last byte of clients [i0, i0 + m), m > 0
__host__ __device__ __forceinline__ uint64_t be_slice_end(uint64_t i0, uint64_t m, uint64_t B, uint64_t R) {
    return be_client_off(i0 + m - 1, B, R) + R;
}
// key kk of client i: its 25 header bytes, then the CorWords
__host__ __device__ __forceinline__ uint64_t be_key_off(uint64_t i, uint32_t kk, uint32_t L, uint64_t B, uint64_t R) {
    return be_client_off(i, B, R) + 8 + kk * be_key_bytes(L);
}
// the CorWords of levels [l0, l0 + nl) of key kk of client i: 20 nl bytes from here
__host__ __device__ __forceinline__ uint64_t be_seg_off(uint64_t i, uint32_t kk, uint32_t l0, uint32_t L, uint64_t B,
                                                        uint64_t R) {
    return be_key_off(i, kk, L, B, R) + 25 + 20ull * l0;
}

struct BeSeg {
    uint32_t head;   // bytes [off, off + head) before the first aligned dword (<= 3)
    uint32_t ndw;    // aligned dwords from off + head on, all inside the segment
    uint32_t tail;   // bytes after the last whole dword (<= 3)
};

// a segment of `bytes` bytes at byte offset `off` of a dword-aligned buffer
__host__ __device__ __forceinline__ BeSeg be_seg_split(uint64_t off, uint32_t bytes) {
    BeSeg s;
    s.head = (uint32_t)((0 - off) & 3);
    if (s.head > bytes) s.head = bytes;
    s.ndw = (bytes - s.head) / 4;
    s.tail = bytes - s.head - 4 * s.ndw;
    return s;
}

}  // namespace fhh
