// pcabi_deflate.hip -- gzip output compressed on the GPU (gfx950): Huffman-only deflate over
// independent, byte-aligned blocks (include/pcabi.h pcabi_gzip_*; DESIGN.md "gzip on the device").
//
// Per input block (1..65535 bytes, the caller's list or fixed-size cuts) one deflate block of
// literals + end-of-block, dynamic Huffman or stored, whichever is not larger; a dynamic block is
// followed by an empty stored block (the sync-flush marker) so the next block starts on a byte.
// Blocks are grouped into gzip members of member_blocks blocks (each far below 4 GiB), every member
// closed by an empty final fixed-Huffman block and its own CRC-32 / ISIZE.
// Kernels (HBM / LDS / integer work):
//   k_plan     one workgroup per block: 257-bin histogram (per-wave LDS copies), CRC-32 of the block
//              (16-byte lane chunks, each multiplied by x^(8 * bytes after it) mod P and xor-reduced),
//              symbols ranked by count across the workgroup, code lengths by one lane
//              (pcabi_deflate.h), canonical codes and the block header's bits across the workgroup,
//              the stored-or-dynamic choice and the block's byte size;
//   k_offsets  one workgroup: exclusive scan of the byte sizes with the member headers / trailers
//              put in, the total, and the too-small / bad-list flags every later kernel obeys;
//   k_members  one workgroup per member: block CRCs combined the same way, header and trailer;
//   k_encode   one workgroup per block: 4 KiB tiles, a lane per 16 bytes, a workgroup prefix sum
//              of the code lengths gives each lane's bit offset, the bits are or-ed into an LDS
//              staging buffer that goes to global memory as aligned 32-bit words (bytes at the
//              block's ragged ends, which neighbouring blocks own).
// All stores are plain C++ stores.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/pcabi.h"
#include "pcabi_crc.h"
#include "pcabi_deflate.h"
#include "pcabi_hostdev.h"

using namespace pcabi_internal;
using namespace pcabi_deflate;
using namespace pcabi_crc;

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 4096;          // bytes per workgroup step: 16 per lane
constexpr int kTblStride = 260;      // uint32 per block: code | len << 16 for 257 symbols
constexpr int kStageWords = 2048;    // 32 carry + 1880 header + 4096 * 15 + 57 tail bits < 65536

struct BlkInfo {
    uint32_t out_bytes, hdr_bits, crc, stored;
};

__device__ const CrcTables d_tab = make_tables();

__device__ inline int64_t blk_lo(const int64_t *block_off, int64_t b, int64_t fixed, int64_t n) {
    return block_off ? block_off[b] : std::min<int64_t>(b * fixed, n);
}

template <int NW>
__device__ inline uint32_t wg_scan_excl(uint32_t v, uint32_t *wsum, uint32_t *total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t x = v;
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    if (lane == 63) wsum[wv] = x;
    __syncthreads();
    uint32_t off = 0, tot = 0;
    for (int i = 0; i < NW; ++i) {
        if (i < wv) off += wsum[i];
        tot += wsum[i];
    }
    __syncthreads();
    *total = tot;
    return off + x - v;
}

// or `nbits` (<= 32) bits of v into the LDS bit buffer at bit position pos
__device__ inline void put_bits(uint32_t *stg, uint32_t pos, uint32_t v, int nbits) {
    if (nbits <= 0) return;
    if (nbits < 32) v &= (1u << nbits) - 1u;
    const uint32_t w = pos >> 5, sh = pos & 31;
    if (v << sh) atomicOr(&stg[w], v << sh);
    if (sh && (v >> (32 - sh))) atomicOr(&stg[w + 1], v >> (32 - sh));
}

// ctl[0] bad block list, ctl[1] stream length (or -1), ctl[2] write nothing
__global__ __launch_bounds__(kThreads) void k_plan(const uint8_t *__restrict__ in, int64_t n,
                                                   const int64_t *__restrict__ block_off, int64_t nb, int64_t fixed,
                                                   uint32_t *__restrict__ tbl, uint32_t *__restrict__ hdr,
                                                   BlkInfo *__restrict__ info, int64_t *ctl) {
    __shared__ uint32_t hist[4][256];
    __shared__ __attribute__((aligned(16))) uint8_t tile[kTile];
    __shared__ uint32_t crc_tab[256], xp0[256], xp1[256];
    __shared__ uint32_t cnt[kLitSyms + 3];
    __shared__ uint16_t order[kLitSyms + 3];
    __shared__ uint8_t len[kTblStride];
    __shared__ uint16_t bl_count[kMaxLitBits + 1], next_code[kMaxLitBits + 1];
    __shared__ HcWork wk;
    __shared__ uint32_t clcnt[kClSyms + 1];
    __shared__ uint8_t cl_len[kClSyms + 1];
    __shared__ uint16_t cl_code[kClSyms + 1];
    __shared__ uint32_t hbuf[kHdrWords + 2];
    __shared__ uint32_t wsum[4];
    __shared__ uint32_t s_crc, s_bits, s_used, s_fixed_bits;

    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int64_t lo = blk_lo(block_off, b, fixed, n), hi = blk_lo(block_off, b + 1, fixed, n);
    if (lo < 0 || hi > n || hi - lo < 1 || hi - lo > kBlockCap) {   // uniform
        if (tid == 0) {
            ctl[0] = 1;
            info[b] = BlkInfo{0, 0, 0, 1};
        }
        return;
    }
    const uint32_t blen = (uint32_t)(hi - lo);
    for (int i = tid; i < 4 * 256; i += kThreads) (&hist[0][0])[i] = 0;
    crc_tab[tid] = d_tab.byte[tid];
    xp0[tid] = d_tab.xp[0][tid];
    xp1[tid] = d_tab.xp[1][tid];
    for (int i = tid; i < kHdrWords + 2; i += kThreads) hbuf[i] = 0;
    if (tid < kClSyms + 1) clcnt[tid] = 0;
    if (tid == 0) {
        s_crc = 0;
        s_bits = 0;
        s_used = 0;
    }
    __syncthreads();

    // ---- histogram + CRC-32 ----
    const uint8_t *src = in + lo;
    uint32_t acc = 0;
    uint32_t *myhist = hist[tid >> 6];
    for (uint32_t base = 0; base < blen; base += kTile) {
        for (int k = 0; k < kTile / kThreads; ++k) {
            const uint32_t idx = base + k * kThreads + tid;
            if (idx < blen) {
                const uint8_t c = src[idx];
                tile[k * kThreads + tid] = c;
                atomicAdd(&myhist[c], 1u);
            }
        }
        __syncthreads();
        const uint32_t first = base + tid * 16;
        if (first < blen) {
            const uint32_t m = std::min<uint32_t>(16, blen - first);
            uint32_t c = 0xffffffffu;
            for (uint32_t j = 0; j < m; ++j) c = crc_tab[(c ^ tile[tid * 16 + j]) & 0xff] ^ (c >> 8);
            c ^= 0xffffffffu;
            const uint32_t after = blen - (first + m);   // < 65536
            uint32_t xp = xp0[after & 255];
            if (after >> 8) xp = mulmod(xp, xp1[after >> 8]);
            acc ^= mulmod(c, xp);
        }
        __syncthreads();
    }
    for (int d = 32; d >= 1; d >>= 1) acc ^= __shfl_xor(acc, d);
    if ((tid & 63) == 0) atomicXor(&s_crc, acc);
    cnt[tid] = hist[0][tid] + hist[1][tid] + hist[2][tid] + hist[3][tid];
    if (tid == 0) cnt[256] = 1;
    if (tid < 4) len[256 + tid] = 0;
    len[tid] = 0;
    __syncthreads();

    // ---- order the used symbols by (count, symbol) ----
    for (int s = tid; s < kLitSyms; s += kThreads) {
        const uint32_t c = cnt[s];
        if (c) {
            int rank = 0;
            for (int j = 0; j < kLitSyms; ++j) {
                const uint32_t cj = cnt[j];
                rank += (cj && (cj < c || (cj == c && j < s))) ? 1 : 0;
            }
            order[rank] = (uint16_t)s;
            atomicAdd(&s_used, 1u);
        }
    }
    __syncthreads();
    if (tid == 0) {
        hc_lengths_sorted(order, (int)s_used, cnt, kMaxLitBits, len, bl_count, wk);
        hc_next_code(bl_count, kMaxLitBits, next_code);
    }
    __syncthreads();

    // ---- canonical codes, data bits, histogram of the lengths ----
    uint32_t bits = 0;
    for (int s = tid; s < kLitSyms; s += kThreads) {
        const int l = len[s];
        uint32_t e = 0;
        if (l) {
            uint32_t k = 0;
            for (int j = 0; j < s; ++j) k += len[j] == l ? 1u : 0u;
            e = hc_rev(next_code[l] + k, l) | ((uint32_t)l << 16);
            bits += cnt[s] * (uint32_t)l;
        }
        tbl[b * kTblStride + s] = e;
        atomicAdd(&clcnt[l], 1u);
    }
    if (tid == 0) atomicAdd(&clcnt[1], 1u);   // the distance code's length
    atomicAdd(&s_bits, bits);
    __syncthreads();

    // ---- header: fixed part and code-length code by one lane, the 258 coded lengths by all ----
    if (tid == 0) {
        int h4 = 0;
        const int fixed_bits = hc_cl_plan(clcnt, cl_len, cl_code, &h4, wk);
        s_fixed_bits = (uint32_t)fixed_bits;
        // BFINAL 0, BTYPE 10 (dynamic), HLIT 0 (257), HDIST 0 (1), HCLEN
        uint32_t pos = 0;
        put_bits(hbuf, pos, 0u | (2u << 1), 3);
        pos += 3;
        put_bits(hbuf, pos, 0, 5);
        pos += 5;
        put_bits(hbuf, pos, 0, 5);
        pos += 5;
        put_bits(hbuf, pos, (uint32_t)(h4 - 4), 4);
        pos += 4;
        for (int i = 0; i < h4; ++i, pos += 3) put_bits(hbuf, pos, cl_len[hc_cl_order(i)], 3);
    }
    __syncthreads();
    {
        const uint32_t l0 = cl_len[len[tid]];
        uint32_t total = 0;
        const uint32_t off = wg_scan_excl<4>(l0, wsum, &total);
        const uint32_t base = s_fixed_bits;
        put_bits(hbuf, base + off, cl_code[len[tid]], (int)l0);
        if (tid == 0) {
            uint32_t pos = base + total;
            put_bits(hbuf, pos, cl_code[len[256]], cl_len[len[256]]);
            pos += cl_len[len[256]];
            put_bits(hbuf, pos, cl_code[1], cl_len[1]);   // distance code 0: length 1
            pos += cl_len[1];
            const uint32_t hdr_bits = pos;
            const uint32_t dyn = dyn_bytes(hdr_bits + s_bits), st = stored_bytes(blen);
            BlkInfo bi;
            bi.stored = st <= dyn ? 1u : 0u;
            bi.out_bytes = bi.stored ? st : dyn;
            bi.hdr_bits = hdr_bits;
            bi.crc = s_crc;
            info[b] = bi;
        }
    }
    __syncthreads();
    for (int i = tid; i < kHdrWords; i += kThreads) hdr[b * kHdrWords + i] = hbuf[i];
}

// hdr: bytes of a member's header, 10 (plain gzip) or 18 (BGZF: the BC subfield with the member's size)
__device__ inline uint32_t member_extra_before(int64_t b, int64_t member_blocks, uint32_t hdr) {
    return b % member_blocks == 0 ? hdr : 0u;
}
__device__ inline uint32_t member_extra_after(int64_t b, int64_t nb, int64_t member_blocks) {
    return (b % member_blocks == member_blocks - 1 || b == nb - 1) ? 10u : 0u;
}

__global__ __launch_bounds__(1024) void k_offsets(const BlkInfo *__restrict__ info, int64_t nb, int64_t member_blocks,
                                                  uint32_t hdr, int64_t cap, int64_t *__restrict__ out_off, int64_t *ctl,
                                                  int64_t *out_len) {
    __shared__ uint32_t wsum[16];
    int64_t carry = 0;
    for (int64_t base = 0; base < nb; base += 1024) {
        const int64_t b = base + threadIdx.x;
        uint32_t s = 0, pre = 0;
        if (b < nb) {
            pre = member_extra_before(b, member_blocks, hdr);
            s = info[b].out_bytes + pre + member_extra_after(b, nb, member_blocks);
        }
        uint32_t total = 0;
        const uint32_t ex = wg_scan_excl<16>(s, wsum, &total);
        if (b < nb) out_off[b] = carry + ex + pre;
        carry += total;
    }
    if (threadIdx.x == 0) {
        const int64_t total = nb == 0 ? (hdr == 18 ? 0 : kMemberOverhead) : carry;   // BGZF: no member for no bytes
        const bool bad = ctl[0] != 0;
        ctl[1] = bad ? -1 : total;
        ctl[2] = (bad || total > cap) ? 1 : 0;
        out_off[nb] = total;
        *out_len = ctl[1];
    }
}

__device__ inline void put_le32(uint8_t *p, uint32_t v) {
    p[0] = (uint8_t)v;
    p[1] = (uint8_t)(v >> 8);
    p[2] = (uint8_t)(v >> 16);
    p[3] = (uint8_t)(v >> 24);
}

__global__ __launch_bounds__(kThreads) void k_members(const int64_t *__restrict__ block_off, int64_t nb, int64_t fixed,
                                                      int64_t n, int64_t member_blocks, uint32_t hdr,
                                                      const BlkInfo *__restrict__ info,
                                                      const int64_t *__restrict__ out_off, const int64_t *ctl,
                                                      uint8_t *__restrict__ out) {
    __shared__ uint32_t s_crc;
    if (ctl[2]) return;
    const int tid = threadIdx.x;
    const int64_t first = (int64_t)blockIdx.x * member_blocks, last = std::min<int64_t>(nb, first + member_blocks);
    if (tid == 0) s_crc = 0;
    __syncthreads();
    int64_t in_end = 0, in_begin = 0;
    uint32_t acc = 0;
    if (last > first) {
        in_begin = blk_lo(block_off, first, fixed, n);
        in_end = blk_lo(block_off, last, fixed, n);
        for (int64_t b = first + tid; b < last; b += kThreads) {
            const uint64_t after = (uint64_t)(in_end - blk_lo(block_off, b + 1, fixed, n));   // < 2^32
            uint32_t xp = d_tab.xp[0][after & 255];
            if ((after >> 8) & 255) xp = mulmod(xp, d_tab.xp[1][(after >> 8) & 255]);
            if ((after >> 16) & 255) xp = mulmod(xp, d_tab.xp[2][(after >> 16) & 255]);
            if ((after >> 24) & 255) xp = mulmod(xp, d_tab.xp[3][(after >> 24) & 255]);
            acc ^= mulmod(info[b].crc, xp);
        }
    }
    for (int d = 32; d >= 1; d >>= 1) acc ^= __shfl_xor(acc, d);
    if ((tid & 63) == 0) atomicXor(&s_crc, acc);
    __syncthreads();
    if (tid == 0) {
        uint8_t *h = out + (last > first ? out_off[first] - hdr : 0);
        uint8_t *t = last > first ? out + out_off[last - 1] + info[last - 1].out_bytes : h + hdr;
        const uint8_t head[10] = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 0xff};
        for (int i = 0; i < 10; ++i) h[i] = head[i];
        if (hdr == 18) {   // BGZF: FEXTRA, XLEN 6, "BC", SLEN 2, BSIZE = member bytes - 1
            const uint32_t bsize = (uint32_t)(t + 10 - h) - 1u;
            const uint8_t x[8] = {6, 0, 0x42, 0x43, 2, 0, (uint8_t)bsize, (uint8_t)(bsize >> 8)};
            h[3] = 4;
            for (int i = 0; i < 8; ++i) h[10 + i] = x[i];
        }
        t[0] = 0x03;   // BFINAL 1, fixed Huffman, end-of-block
        t[1] = 0x00;
        put_le32(t + 2, s_crc);
        put_le32(t + 6, (uint32_t)(in_end - in_begin));
    }
}

__global__ __launch_bounds__(kThreads) void k_encode(const uint8_t *__restrict__ in, int64_t n,
                                                     const int64_t *__restrict__ block_off, int64_t nb, int64_t fixed,
                                                     const uint32_t *__restrict__ tbl, const uint32_t *__restrict__ hdr,
                                                     const BlkInfo *__restrict__ info,
                                                     const int64_t *__restrict__ out_off, const int64_t *ctl,
                                                     uint8_t *__restrict__ out) {
    __shared__ uint32_t stg[kStageWords + 4];
    __shared__ __attribute__((aligned(16))) uint8_t tile[kTile];
    __shared__ uint32_t tb[kLitSyms + 3];
    __shared__ uint32_t wsum[4];
    if (ctl[2]) return;
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int64_t lo = blk_lo(block_off, b, fixed, n);
    const uint32_t blen = (uint32_t)(blk_lo(block_off, b + 1, fixed, n) - lo);
    const BlkInfo bi = info[b];
    const uint8_t *src = in + lo;
    uint8_t *o = out + out_off[b];
    if (bi.stored) {
        if (tid == 0) {
            o[0] = 0;   // BFINAL 0, BTYPE 00, padding
            o[1] = (uint8_t)blen;
            o[2] = (uint8_t)(blen >> 8);
            o[3] = (uint8_t)~blen;
            o[4] = (uint8_t)(~blen >> 8);
        }
        for (uint32_t i = tid; i < blen; i += kThreads) o[5 + i] = src[i];
        return;
    }
    for (int s = tid; s < kLitSyms; s += kThreads) tb[s] = tbl[b * kTblStride + s];
    for (int i = tid; i < kStageWords + 4; i += kThreads) stg[i] = 0;
    __syncthreads();
    const uintptr_t a_begin = (uintptr_t)o, a_end = a_begin + bi.out_bytes;
    uintptr_t gbase = a_begin & ~(uintptr_t)3;     // address of staging word 0
    uint32_t cursor = (uint32_t)(a_begin - gbase) * 8;   // bit position in the staging buffer
    for (int i = tid; i < kHdrWords; i += kThreads) put_bits(stg, cursor + 32u * i, hdr[b * kHdrWords + i], 32);
    cursor += bi.hdr_bits;
    __syncthreads();
    for (uint32_t base = 0; base < blen; base += kTile) {
        for (int k = 0; k < kTile / kThreads; ++k) {
            const uint32_t idx = base + k * kThreads + tid;
            if (idx < blen) tile[k * kThreads + tid] = src[idx];
        }
        __syncthreads();
        const uint32_t first = base + tid * 16;
        const uint32_t m = first < blen ? std::min<uint32_t>(16, blen - first) : 0;
        uint32_t e[16];
        uint32_t sum = 0;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            e[j] = (uint32_t)j < m ? tb[tile[tid * 16 + j]] : 0u;
            sum += e[j] >> 16;
        }
        uint32_t total = 0;
        const uint32_t off = wg_scan_excl<4>(sum, wsum, &total);
        {
            const uint32_t pos = cursor + off;
            uint32_t w = pos >> 5, nbits = pos & 31;
            uint64_t acc = 0;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                acc |= (uint64_t)(e[j] & 0xffffu) << nbits;
                nbits += e[j] >> 16;
                if (nbits >= 32) {
                    if ((uint32_t)acc) atomicOr(&stg[w], (uint32_t)acc);
                    ++w;
                    acc >>= 32;
                    nbits -= 32;
                }
            }
            if ((uint32_t)acc) atomicOr(&stg[w], (uint32_t)acc);
        }
        cursor += total;
        const bool last = base + kTile >= blen;
        if (last) {   // end-of-block, the empty stored block: 000, padding, 00 00 FF FF
            const uint32_t eob = tb[256];
            if (tid == 0) put_bits(stg, cursor, eob & 0xffffu, (int)(eob >> 16));
            cursor += eob >> 16;
            cursor = (cursor + 3 + 7) & ~7u;
            if (tid == 0) put_bits(stg, cursor, 0xffff0000u, 32);
            cursor += 32;
        }
        __syncthreads();
        const uint32_t nw = last ? (cursor + 31) / 32 : cursor / 32;
        for (uint32_t w = tid; w < nw; w += kThreads) {
            const uintptr_t ga = gbase + 4u * (uintptr_t)w;
            const uintptr_t wlo = std::max(ga, a_begin), whi = std::min(ga + 4, a_end);
            if (wlo >= whi) continue;
            const uint32_t v = stg[w];
            if (wlo == ga && whi == ga + 4) {
                *(uint32_t *)ga = v;
            } else {
                for (uintptr_t p = wlo; p < whi; ++p) *(uint8_t *)p = (uint8_t)(v >> (8 * (p - ga)));
            }
        }
        if (!last) {
            const uint32_t carry = stg[nw];
            __syncthreads();
            for (int i = tid; i < kStageWords + 4; i += kThreads) stg[i] = 0;
            __syncthreads();
            if (tid == 0) stg[0] = carry;
            gbase += 4u * (uintptr_t)nw;
            cursor -= 32u * nw;
            __syncthreads();
        }
    }
}

// ---- host side ---------------------------------------------------------------------------------

int g_block_len = kDefaultBlock;
int64_t g_member_blocks = 1024;
int64_t g_chunk_bytes = 64ll << 20;
constexpr int64_t kPassBlocks = 65536;   // blocks per staged pass at the most (bounds the scratch)

int64_t scratch_bytes(int64_t nb) {
    return 64 + 8 * (nb + 1) + (int64_t)sizeof(BlkInfo) * nb + 4ll * kHdrWords * nb + 4ll * kTblStride * nb + 64;
}

int64_t bound(int64_t n, int64_t nb) { return n + 25 * nb + kMemberOverhead + 16; }
constexpr int64_t kBgzfBlockCap = PCABI_BGZF_BLOCK_CAP;   // a stored block + 28 bytes of member stay within 65536
constexpr int64_t kBgzfEofBytes = 28;
// one member per block: 18 header + 5 stored (or less) + 2 closing block + 8 trailer
int64_t bgzf_bound(int64_t n, int64_t nb, int eof) { return n + 33 * nb + (eof ? kBgzfEofBytes : 0) + 16; }

// queues the four kernels; out_len_dev receives the stream length, or -1 for a bad block list
int launch(hipStream_t st, const uint8_t *in, int64_t n, const int64_t *block_off, int64_t nb, int64_t fixed,
           int64_t member_blocks, uint32_t mhdr, uint8_t *out, int64_t cap, int64_t *out_len_dev, void *scratch) {
    char *p = (char *)scratch;
    int64_t *ctl = (int64_t *)p;
    p += 64;
    int64_t *out_off = (int64_t *)p;
    p += 8 * (nb + 1);
    BlkInfo *info = (BlkInfo *)p;
    p += (int64_t)sizeof(BlkInfo) * nb;
    uint32_t *hdr = (uint32_t *)p;
    p += 4ll * kHdrWords * nb;
    uint32_t *tbl = (uint32_t *)p;
    PCABI_TRY(hipMemsetAsync(ctl, 0, 64, st));
    if (nb > 0) hipLaunchKernelGGL(k_plan, dim3((unsigned)nb), dim3(kThreads), 0, st, in, n, block_off, nb, fixed, tbl, hdr, info, ctl);
    hipLaunchKernelGGL(k_offsets, dim3(1), dim3(1024), 0, st, info, nb, member_blocks, mhdr, cap, out_off, ctl, out_len_dev);
    const int64_t nm = std::max<int64_t>(1, (nb + member_blocks - 1) / member_blocks);
    if (nb > 0 || mhdr != 18)
        hipLaunchKernelGGL(k_members, dim3((unsigned)nm), dim3(kThreads), 0, st, block_off, nb, fixed, n, member_blocks, mhdr,
                           info, out_off, ctl, out);
    if (nb > 0)
        hipLaunchKernelGGL(k_encode, dim3((unsigned)nb), dim3(kThreads), 0, st, in, n, block_off, nb, fixed, tbl, hdr, info,
                           out_off, ctl, out);
    PCABI_TRY(hipGetLastError());
    return 0;
}

// The host entry's staging slots: pinned and device buffers kept between calls (one device at a
// time; a call on another device, or a larger pass, reallocates). One call runs at a time.
struct Slot {
    PinBuf<> pin_in, pin_out;
    PinBuf<int64_t> pin_off, pin_len;
    DevBuf<> dev_in, dev_out;
    DevBuf<int64_t> dev_off, dev_len;
    DevBuf<> scratch;
    int64_t len = 0;
    Stream st;   // the last member: the first to go
    // f(buffer, elements) for every buffer of a pass of up to bytes / blocks, until one returns false
    template <class F>
    bool each(int64_t bytes, int64_t blocks, F f) {
        const int64_t ob = std::max(bound(bytes, blocks), bgzf_bound(bytes, blocks, 0));
        return f(pin_in, bytes + 16) && f(pin_out, ob) && f(pin_off, blocks + 1) && f(pin_len, 8) && f(dev_in, bytes + 16) &&
               f(dev_out, ob) && f(dev_off, blocks + 1) && f(dev_len, 8) && f(scratch, scratch_bytes(blocks));
    }
};
constexpr int kSlots = 3;
struct Stage {
    int device = -1;
    Slot s[kSlots];
    double t_copy_in = 0, t_sync = 0, t_copy_out = 0;
};
// kept for the process and never destroyed (a deliberate leak): a destructor at exit would call into a
// HIP runtime that may already have shut down
Stage &g_stage = *new Stage;
std::mutex g_stage_mu;

// Whether the kept buffers serve is read from the buffers themselves, so a reserve that failed half-way
// is done again by the next call.
int stage_reserve(int device, int64_t bytes, int64_t blocks) {
    bool kept = g_stage.device == device;
    for (Slot &s : g_stage.s) kept = kept && s.each(bytes, blocks, [](auto &b, int64_t n) { return holds(b, n); });
    if (kept) return 0;
    if (g_stage.device >= 0) {
        (void)hipSetDevice(g_stage.device);
        for (Slot &s : g_stage.s) {
            s.st.release();
            s = Slot();
        }
    }
    PCABI_TRY(hipSetDevice(device));
    g_stage.device = device;
    int rc = 0;
    for (Slot &s : g_stage.s)
        if (!rc && !(rc = s.st.create())) s.each(bytes, blocks, [&](auto &b, int64_t n) { return (rc = b.reserve(n, n)) == 0; });
    return rc;
}

}  // namespace

extern "C" {

int pcabi_gzip_block_len(void) { return g_block_len; }

int64_t pcabi_gzip_bound(int64_t n, int64_t n_blocks) {
    if (n < 0 || n_blocks < 0) return fail(PCABI_E_ARG, "negative size");
    if (n_blocks == 0) n_blocks = (n + g_block_len - 1) / g_block_len;
    return bound(n, n_blocks);
}

int64_t pcabi_gzip_scratch_bytes(int64_t n, int64_t n_blocks) {
    if (n < 0 || n_blocks < 0) return fail(PCABI_E_ARG, "negative size");
    if (n_blocks == 0) n_blocks = (n + g_block_len - 1) / g_block_len;
    return scratch_bytes(n_blocks);
}

int pcabi_gzip_tune(int block_len, int64_t member_blocks, int64_t chunk_bytes) {
    if (block_len < 0 || block_len > kBlockCap || member_blocks < 0 || member_blocks > 32768 || chunk_bytes < 0 ||
        (chunk_bytes > 0 && chunk_bytes < 65536) || chunk_bytes > (1ll << 31))
        return fail(PCABI_E_ARG, "block_len 1..65535, member_blocks 1..32768, chunk_bytes 64 KiB..2 GiB (0 = default)");
    std::lock_guard<std::mutex> lk(g_stage_mu);
    g_block_len = block_len ? block_len : kDefaultBlock;
    g_member_blocks = member_blocks ? member_blocks : 1024;
    g_chunk_bytes = chunk_bytes ? chunk_bytes : (64ll << 20);
    return 0;
}

int pcabi_gzip_dev(void *stream, const uint8_t *in, int64_t n, const int64_t *block_off, int64_t n_blocks,
                   uint8_t *out, int64_t cap, int64_t *out_len, void *scratch, int64_t scratch_len) {
    if (n < 0 || n_blocks < 0 || cap < 0 || !out_len || !scratch || (n > 0 && !in) || (cap > 0 && !out))
        return fail(PCABI_E_ARG, "bad arguments");
    const int64_t fixed = g_block_len;
    if (!block_off) n_blocks = (n + fixed - 1) / fixed;
    else if ((n > 0) != (n_blocks > 0)) return fail(PCABI_E_ARG, "a block list must cover the input");
    if (n_blocks > INT32_MAX) return fail(PCABI_E_ARG, "too many blocks for one call");
    if (scratch_len < scratch_bytes(n_blocks)) return fail(PCABI_E_ARG, "scratch smaller than pcabi_gzip_scratch_bytes");
    return launch((hipStream_t)stream, in, n, block_off, n_blocks, fixed, g_member_blocks, 10, out, cap, out_len, scratch);
}

static int64_t gzip_host_impl(int device, const uint8_t *in, int64_t n, const int64_t *block_off, int64_t n_blocks,
                              uint8_t *out, int64_t cap, bool bgzf) {
    if (n < 0 || n_blocks < 0 || cap < 0 || (n > 0 && !in) || (cap > 0 && !out)) return fail(PCABI_E_ARG, "bad arguments");
    std::lock_guard<std::mutex> lk(g_stage_mu);
    const int64_t block_cap = bgzf ? kBgzfBlockCap : kBlockCap;
    const int64_t fixed = std::min<int64_t>(g_block_len, block_cap), member_blocks = bgzf ? 1 : g_member_blocks,
                  chunk = g_chunk_bytes;
    const uint32_t hdr = bgzf ? 18 : 10;
    // passes: [first block, last block) each, whole members
    std::vector<int64_t> pass{0};
    int64_t max_bytes = 0, max_blocks = 0;
    if (block_off) {
        if ((n > 0) != (n_blocks > 0) || block_off[0] != 0 || block_off[n_blocks] != n)
            return fail(PCABI_E_ARG, "a block list starts at 0, ends at n and covers the input");
        for (int64_t b = 0; b < n_blocks; ++b) {
            const int64_t l = block_off[b + 1] - block_off[b];
            if (l < 1 || l > block_cap)
                return fail(PCABI_E_ARG, bgzf ? "every BGZF block holds 1..65280 bytes" : "every block holds 1..65535 bytes");
        }
        int64_t first = 0;
        for (int64_t b = 0; b < n_blocks; ++b)
            if (block_off[b + 1] - block_off[first] > chunk || b + 1 - first > kPassBlocks) {
                pass.push_back(b);
                first = b;
            }
        if (n_blocks > 0) pass.push_back(n_blocks);
    } else {
        n_blocks = (n + fixed - 1) / fixed;
        const int64_t per = std::min<int64_t>(kPassBlocks, std::max<int64_t>(1, chunk / fixed));
        for (int64_t b = per; b < n_blocks; b += per) pass.push_back(b);
        if (n_blocks > 0) pass.push_back(n_blocks);
    }
    if (pass.size() == 1) pass.push_back(0);   // empty input: one pass that writes the empty member
    const int64_t np = (int64_t)pass.size() - 1;
    auto byte_at = [&](int64_t b) { return block_off ? block_off[b] : std::min<int64_t>(b * fixed, n); };
    for (int64_t p = 0; p < np; ++p) {
        max_bytes = std::max(max_bytes, byte_at(pass[p + 1]) - byte_at(pass[p]));
        max_blocks = std::max(max_blocks, pass[p + 1] - pass[p]);
    }
    if (device < 0) PCABI_TRY(hipGetDevice(&device));
    PCABI_TRY(hipSetDevice(device));
    if (int rc = stage_reserve(device, std::max<int64_t>(max_bytes, 1 << 16), std::max<int64_t>(max_blocks, 16))) return rc;
    g_stage.t_copy_in = g_stage.t_sync = g_stage.t_copy_out = 0;
    int64_t total = 0;
    bool fits = true;
    for (int64_t i = 0; i < np + 2; ++i) {
        if (i < np) {   // stage A: copy up, kernels, the length back
            Slot &s = g_stage.s[i % kSlots];
            const int64_t b0 = pass[i], b1 = pass[i + 1], lo = byte_at(b0), bytes = byte_at(b1) - lo;
            const double t0 = now_s();
            if (bytes > 0) par_memcpy(s.pin_in, in + lo, (size_t)bytes);
            if (block_off)
                for (int64_t b = b0; b <= b1; ++b) s.pin_off[b - b0] = block_off[b] - lo;
            g_stage.t_copy_in += now_s() - t0;
            if (bytes > 0) PCABI_TRY(hipMemcpyAsync(s.dev_in, s.pin_in, (size_t)bytes, hipMemcpyHostToDevice, s.st));
            if (block_off)
                PCABI_TRY(hipMemcpyAsync(s.dev_off, s.pin_off, 8 * (size_t)(b1 - b0 + 1), hipMemcpyHostToDevice, s.st));
            if (int rc = launch(s.st, s.dev_in, bytes, block_off ? s.dev_off : nullptr, b1 - b0, fixed, member_blocks, hdr,
                                s.dev_out, bgzf ? bgzf_bound(bytes, b1 - b0, 0) : bound(bytes, b1 - b0), s.dev_len,
                                s.scratch))
                return rc;
            PCABI_TRY(hipMemcpyAsync(s.pin_len, s.dev_len, 8, hipMemcpyDeviceToHost, s.st));
        }
        if (i >= 1 && i - 1 < np) {   // stage B: the compressed bytes back
            Slot &s = g_stage.s[(i - 1) % kSlots];
            const double t0 = now_s();
            PCABI_TRY(hipStreamSynchronize(s.st));
            g_stage.t_sync += now_s() - t0;
            s.len = *s.pin_len;
            if (s.len < 0) return fail(PCABI_E_ARG, "bad block list");
            PCABI_TRY(hipMemcpyAsync(s.pin_out, s.dev_out, (size_t)s.len, hipMemcpyDeviceToHost, s.st));
        }
        if (i >= 2) {   // stage C: into the caller's buffer
            Slot &s = g_stage.s[(i - 2) % kSlots];
            double t0 = now_s();
            PCABI_TRY(hipStreamSynchronize(s.st));
            g_stage.t_sync += now_s() - t0;
            t0 = now_s();
            fits = fits && total + s.len <= cap;
            if (fits) par_memcpy(out + total, s.pin_out, (size_t)s.len);
            total += s.len;
            g_stage.t_copy_out += now_s() - t0;
        }
    }
    return total;
}

int64_t pcabi_gzip_host(int device, const uint8_t *in, int64_t n, const int64_t *block_off, int64_t n_blocks,
                        uint8_t *out, int64_t cap) {
    return gzip_host_impl(device, in, n, block_off, n_blocks, out, cap, false);
}

static const uint8_t kBgzfEof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};

int64_t pcabi_bgzf_bound(int64_t n, int64_t n_blocks, int eof) {
    if (n < 0 || n_blocks < 0) return fail(PCABI_E_ARG, "negative size");
    const int64_t fixed = std::min<int64_t>(g_block_len, kBgzfBlockCap);
    if (n_blocks == 0) n_blocks = (n + fixed - 1) / fixed;
    return bgzf_bound(n, n_blocks, eof);
}

int64_t pcabi_bgzf_host(int device, const uint8_t *in, int64_t n, const int64_t *block_off, int64_t n_blocks, int eof,
                        uint8_t *out, int64_t cap) {
    const int64_t tail = eof ? kBgzfEofBytes : 0;
    if (cap < 0) return fail(PCABI_E_ARG, "bad arguments");
    const int64_t zn = gzip_host_impl(device, in, n, block_off, n_blocks, out, std::max<int64_t>(cap - tail, 0), true);
    if (zn < 0) return zn;
    if (tail && zn + tail <= cap) std::memcpy(out + zn, kBgzfEof, (size_t)tail);
    return zn + tail;
}

int64_t pcabi_bgzf_scratch_bytes(int64_t n, int64_t block_len) {
    if (n < 0 || block_len < 1 || block_len > kBgzfBlockCap) return fail(PCABI_E_ARG, "block_len 1..65280");
    return scratch_bytes((n + block_len - 1) / block_len);
}

int pcabi_bgzf_dev(void *stream, const uint8_t *in, int64_t n, int64_t block_len, uint8_t *out, int64_t cap,
                   int64_t *out_len, void *scratch, int64_t scratch_len) {
    if (n < 0 || cap < 0 || !out_len || !scratch || (n > 0 && !in) || (cap > 0 && !out) || block_len < 1 ||
        block_len > kBgzfBlockCap)
        return fail(PCABI_E_ARG, "bad arguments");
    const int64_t nb = (n + block_len - 1) / block_len;
    if (nb > INT32_MAX) return fail(PCABI_E_ARG, "too many blocks for one call");
    if (scratch_len < scratch_bytes(nb)) return fail(PCABI_E_ARG, "scratch smaller than pcabi_bgzf_scratch_bytes");
    return launch((hipStream_t)stream, in, n, nullptr, nb, block_len, 1, 18, out, cap, out_len, scratch);
}

}  // extern "C"

// pcabi_bgzf_dev with the caller's block list: the text writer's line-aligned members (pcabi_auxtext.hip)
int pcabi_internal::bgzf_dev_blocks(void *stream, const uint8_t *in, int64_t n, const int64_t *block_off, int64_t n_blocks,
                                    uint8_t *out, int64_t cap, int64_t *out_len, void *scratch, int64_t scratch_len) {
    if (n < 0 || n_blocks < 0 || cap < 0 || !out_len || !scratch || !block_off || (n > 0 && !in) || (cap > 0 && !out) ||
        (n > 0) != (n_blocks > 0) || n_blocks > INT32_MAX)
        return fail(PCABI_E_ARG, "bad arguments");
    if (scratch_len < scratch_bytes(n_blocks)) return fail(PCABI_E_ARG, "scratch smaller than pcabi_gzip_scratch_bytes");
    return launch((hipStream_t)stream, in, n, block_off, n_blocks, kBgzfBlockCap, 1, 18, out, cap, out_len, scratch);
}

extern "C" {

int pcabi_bgzf_write_eof(const char *path) {
    if (!path) return fail(PCABI_E_ARG, "bad arguments");
    FILE *f = std::fopen(path, "ab");
    if (!f) return fail(PCABI_E_ARG, std::string("could not write ") + path);
    const bool ok = std::fwrite(kBgzfEof, 1, sizeof kBgzfEof, f) == sizeof kBgzfEof;
    if (std::fclose(f) != 0 || !ok) return fail(PCABI_E_ARG, std::string("could not write ") + path);
    return 0;
}

// seconds the last pcabi_gzip_host call spent copying into pinned memory, waiting for the device
// and copying out of pinned memory (tools/gz_timing.py)
void pcabi_gzip_last_times(double *copy_in, double *wait, double *copy_out) {
    std::lock_guard<std::mutex> lk(g_stage_mu);
    if (copy_in) *copy_in = g_stage.t_copy_in;
    if (wait) *wait = g_stage.t_sync;
    if (copy_out) *copy_out = g_stage.t_copy_out;
}

}  // extern "C"
