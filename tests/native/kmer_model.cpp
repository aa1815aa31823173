// Host model of the k-mer kernels (TEST INFRASTRUCTURE ONLY): batch calls over csrc/pcabi_kmer.h, the
// functions k_kmer_keys and k_kmer_approx run on the device. Built by tests/test_kmer_core_cpu.py.
#include <cstdint>

#include "../../custom_porechop_abi_amd/csrc/pcabi_kmer.h"

extern "C" {

// k_kmer_keys without the sort: for sequence s, position p, keys[key_off[s] + p] and has_key[..] (0: the
// position is skipped and its key is kSkip). key_off as pcabi_kmer_top_host lays it out.
void kmer_model_keys(const uint8_t *codes, const int64_t *seq_off, const int32_t *seq_len, int64_t n_seq, int k, float thr,
                     const uint64_t *forb, int64_t n_forb, const int64_t *key_off, uint64_t *keys, uint8_t *has_key) {
    for (int64_t s = 0; s < n_seq; ++s)
        for (int p = 0; p < seq_len[s] - k + 1; ++p) {
            uint64_t key = pcabi_kmer::kSkip;
            has_key[key_off[s] + p] = pcabi_kmer::window_key(codes + seq_off[s] + p, k, thr, forb, n_forb, &key);
            keys[key_off[s] + p] = key;
        }
}

void kmer_model_low_complexity(const uint64_t *kmers, int64_t n, int k, float thr, uint8_t *out) {
    for (int64_t i = 0; i < n; ++i) out[i] = pcabi_kmer::low_complexity(kmers[i], k, thr);
}

// k_kmer_approx before its sum: best[q * n_seq + s], the least edit distance of k-mer q to a substring of
// sequence s (4-aligned starts, as pcabi_kmer_approx_host asks).
void kmer_model_best(const uint8_t *codes, const int64_t *seq_off, const int32_t *seq_len, int64_t n_seq, int k,
                     const uint64_t *kmers, int64_t n_kmers, int32_t *best) {
    for (int64_t q = 0; q < n_kmers; ++q) {
        const pcabi_kmer::Masks m = pcabi_kmer::pattern_masks(kmers[q], k);
        for (int64_t s = 0; s < n_seq; ++s)
            best[q * n_seq + s] =
                pcabi_kmer::best_distance(m, k, reinterpret_cast<const uint32_t *>(codes + seq_off[s]), seq_len[s]);
    }
}

}  // extern "C"
