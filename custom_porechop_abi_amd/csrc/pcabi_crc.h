// pcabi_crc.h -- CRC-32 (the gzip polynomial) pieces shared by the gzip encoder (pcabi_deflate.hip)
// and the inflate kernel (pcabi_inflate.hip): the byte-wise table and the powers of x that let a
// CRC of a chunk be moved past the bytes that follow it, so chunks are summed in any order.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PCABI_CRC_HD __host__ __device__
#else
#define PCABI_CRC_HD
#endif

namespace pcabi_crc {

constexpr uint32_t kPoly = 0xedb88320u;

// a * b mod P, reflected representation (x^0 = 1 << 31), as zlib's multmodp
PCABI_CRC_HD constexpr uint32_t mulmod(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 0; i < 32; ++i) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ kPoly : b >> 1;
    }
    return p;
}

struct CrcTables {
    uint32_t byte[256];     // the byte-wise CRC-32 table
    uint32_t xp[4][256];    // xp[l][k] = x^(8 k 256^l) mod P
};

constexpr CrcTables make_tables() {
    CrcTables t{};
    for (uint32_t n = 0; n < 256; ++n) {
        uint32_t c = n;
        for (int k = 0; k < 8; ++k) c = (c & 1u) ? kPoly ^ (c >> 1) : c >> 1;
        t.byte[n] = c;
    }
    uint32_t step = 0x00800000u;   // x^8
    for (int l = 0; l < 4; ++l) {
        t.xp[l][0] = 0x80000000u;
        for (int k = 1; k < 256; ++k) t.xp[l][k] = mulmod(t.xp[l][k - 1], step);
        step = mulmod(t.xp[l][255], step);
    }
    return t;
}

}  // namespace pcabi_crc
