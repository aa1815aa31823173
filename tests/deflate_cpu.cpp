// Host build of the gzip encoder's device-free parts (csrc/pcabi_deflate.h): the code-length
// construction and the writer's block planner, for tests/test_deflate_cpu.py. TEST INFRASTRUCTURE ONLY.
#include "../custom_porechop_abi_amd/csrc/pcabi_deflate.h"

using namespace pcabi_deflate;

extern "C" {

// cnt[256] literal counts -> lit_len[257], cl_len[19], cl_code[19] (bit-reversed), hclen4, the
// header's and the whole dynamic block's bit counts
void dfl_plan_block(const uint32_t *cnt256, uint8_t *lit_len, uint8_t *cl_len, uint16_t *cl_code, int *hclen4,
                    uint32_t *hdr_bits, uint32_t *block_bits) {
    uint32_t cnt[kLitSyms];
    for (int s = 0; s < 256; ++s) cnt[s] = cnt256[s];
    HcWork wk;
    hc_plan_block(cnt, lit_len, cl_len, cl_code, hclen4, hdr_bits, block_bits, wk);
}

// canonical codes (bit-reversed) of lengths len[nsym]
void dfl_codes(const uint8_t *len, int nsym, int maxbits, uint16_t *code) {
    uint16_t blc[kMaxLitBits + 1] = {0};
    for (int s = 0; s < nsym; ++s)
        if (len[s]) ++blc[len[s]];
    hc_codes(len, nsym, blc, maxbits, code);
}

int dfl_cl_order(int i) { return hc_cl_order(i); }
uint32_t dfl_dyn_bytes(uint32_t block_bits) { return dyn_bytes(block_bits); }
uint32_t dfl_stored_bytes(uint32_t n) { return stored_bytes(n); }

int64_t dfl_plan_lines(const char *text, int64_t n, int64_t long_line, int64_t cap, int64_t *block_off, int64_t off_cap) {
    int64_t k = 0;
    if (off_cap > 0) block_off[0] = 0;
    plan_blocks(text, 0, n, long_line, cap, [&](int64_t end) {
        ++k;
        if (k < off_cap) block_off[k] = end;
    });
    return k;
}

}  // extern "C"
