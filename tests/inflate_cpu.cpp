// Host build of the gzip decoder's device-free parts (csrc/pcabi_inflate.h): the whole member
// decoder with the serial policies and the BGZF member index, for tests/test_inflate_cpu.py.
// TEST INFRASTRUCTURE ONLY.
#include "../custom_porechop_abi_amd/csrc/pcabi_inflate.h"

using namespace pcabi_inflate;

extern "C" {

// one gzip member z[0, n) into out[0, cap): the status, *out_len = decoded bytes on success
int infl_member(const uint8_t *z, int64_t n, uint8_t *out, uint32_t cap, uint32_t *out_len) {
    SerialPar par;
    SerialSink sink{out};
    Tables t;
    return inflate_member(par, sink, t, z, n, cap, out_len);
}

int64_t infl_index(const uint8_t *z, int64_t n, int64_t *in_off, int64_t *out_off, int64_t cap) {
    return gunzip_index(z, n, in_off, out_off, cap);
}

}  // extern "C"
