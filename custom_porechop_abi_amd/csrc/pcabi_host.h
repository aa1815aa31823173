// pcabi_host.h -- the host-side declarations that cross between the engine (pcabi_engine.hip), the
// host-buffer entry points (pcabi_hostapi.hip), the middle scan (pcabi_middle.hip) and the middle-scan
// seeds (pcabi_seed.hip): the prepared adapter table, the fork / join of independent launches, the
// bucket layout, the bucket dispatch and its layout questions, the tile layout, and the seeds' entry
// points. Host code only: the kernel units include pcabi_kern.h.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <mutex>
#include <utility>
#include <vector>

#include "../../include/pcabi.h"
#include "pcabi_dp.h"
#include "pcabi_kern.h"
#include "pcabi_scratch.h"

using pcabi_internal::Scratch;

void pcabi_poison_async(void *p, size_t bytes, hipStream_t st);   // pcabi_engine.hip (PCABI_POISON)

// ---- prepared adapter tables (device), pcabi_engine.hip ------------------------------------------
extern std::atomic<uint64_t> g_table_serial;
struct pcabi_adapters {
    int32_t n_adp = 0;
    // a process-unique number (a new table may reuse a freed one's address): what the middle scan's
    // captured round graphs are keyed on, since they hold the table's device pointers
    uint64_t serial = g_table_serial.fetch_add(1) + 1;
    int rt[pcabi_eng::kNumBuckets] = {};        // striped bucket: table rows per adapter
    bool padded[pcabi_eng::kNumBuckets] = {};
    int max_off[pcabi_eng::kNumBuckets] = {};   // most padding rows above an adapter (> 3: packed core only)
    std::vector<int32_t> lens[pcabi_eng::kNumBuckets];
    std::vector<int32_t> ids[pcabi_eng::kNumBuckets];   // global adapter index of each bucket entry (host)
    bool has_n = false;                      // some adapter holds an N (code 4) base
    std::vector<uint8_t> hcodes;             // host copy of the adapters (middle-scan seeds)
    std::vector<int32_t> hoff, hlen;
    int32_t count[pcabi_eng::kNumBuckets] = {};
    // the buckets' device arrays (plain device memory: no scratch generation, no poison)
    pcabi_internal::DevBuf<uint32_t> pad[pcabi_eng::kNumBuckets];
    pcabi_internal::DevBuf<int32_t> len[pcabi_eng::kNumBuckets], id[pcabi_eng::kNumBuckets];
    // Other layouts of the same adapters, built on first use by adapters_for() for a scoring this
    // layout cannot serve (gap costs >= 0 under padded register buckets, a merge made for another
    // scoring) or for long windows that need the striped core; kept until the table is destroyed
    // (launches queued on a stream may still read them).
    std::mutex alt_mu;
    std::vector<std::pair<pcabi::Scoring, pcabi_adapters *>> alt_scored;
    pcabi_adapters *alt_striped = nullptr;
};
bool layout_serves(const pcabi_adapters *adps, const pcabi::Scoring &sc, int64_t max_win);
int adapters_for(const pcabi_adapters *adps, const pcabi::Scoring &sc, int64_t max_win, const pcabi_adapters **use);

namespace pcabi_eng {

// Fork / join of independent launches: launch k runs on the caller's stream (k == 0) or on side
// stream (first + k - 1) % N, each side stream first waiting for the work already queued on the
// caller's stream; end() makes the caller's stream wait for every side stream used.
struct SideStreams;
struct ForkJoin {
    hipStream_t main = nullptr;
    SideStreams *ss = nullptr;
    std::unique_lock<std::mutex> lock;
    int first = 0;
    unsigned used = 0;           // bit i: side stream i took a launch of this region
    int n_side = 0;              // side launches of this region
    int begin(hipStream_t m, size_t n_launch);
    hipStream_t at(size_t k);
    int end();
};

int64_t tile_layout(const int32_t *win_len, int64_t n_win, int64_t *tile_off, int64_t *max_nq);
void launch_tiles(const uint8_t *codes, const int64_t *win_off, const int32_t *win_len, int64_t n_win,
                  const int64_t *tile_off, int64_t max_nq, uint32_t *tiles, hipStream_t st);
int first_hit_from(const int32_t *res, int64_t stride, int64_t n_win, int32_t n_adp, double threshold,
                   const int32_t *start_adp, int32_t *hits, int64_t hit_stride, hipStream_t st);
void scan_set_table(pcabi_scan *s, const pcabi_adapters *adps);   // pcabi_middle.hip: the table a scan runs on
bool chunkable(int b, bool packed);
// packed: bucket_pack_mode (0 untagged cores off, 1 packed key layout, 2 run-tagged layout)
int dispatch(int b, const KParams &p, bool affine, hipStream_t st, int packed);
bool bucket_packed_ok(int b, const std::vector<int32_t> &lens, const pcabi::Scoring &sc);
int bucket_pack_mode(int b, const std::vector<int32_t> &lens, const pcabi::Scoring &sc);
// cross shape, pack mode 2, and pack mode 1 at 36..64 rows: the bucket's gap-extend frame into
// p.shift_p / p.shift_b (0: none)
void bucket_shift(int b, const std::vector<int32_t> &lens, const pcabi::Scoring &sc, int pack_mode, KParams &p);

// Host-side layout of a bucket's adapter table, for a caller that uploads its own (pcabi_align_host).
struct BucketHost {
    std::vector<uint8_t> pad;   // n * RPL bytes (striped: n * rt)
    std::vector<int32_t> len, id;
    int rt = 0;                 // striped: table rows per adapter
};
void build_buckets(const uint8_t *adp_codes, const int32_t *adp_off, const int32_t *adp_len, int32_t n_adp,
                   const pcabi::Scoring &sc, BucketHost (&bk)[kNumBuckets], bool merge = true, bool allow_wide = true,
                   bool all_striped = false);
int check_adapter_lens(const int32_t *adp_len, int32_t n_adp);           // every length in 1..MAX_STRIPED_LEN
bool needs_striped(const pcabi::Scoring &sc, int max_L, int64_t max_win);   // long windows, unbounded path span

}  // namespace pcabi_eng

// ---- pcabi_seed.hip ------------------------------------------------------------------------------
namespace pcabi_seed {
struct State;
State *create();
void destroy(State *s);
int bounds(State *s, const void *adps_key, const uint8_t *hcodes, const int32_t *hoff, const int32_t *hlen,
           int32_t n_adp, const std::vector<int> &fb_rows, const uint8_t *codes, const int64_t *v_off,
           const int32_t *v_len, int64_t n, const pcabi::Scoring &sc, double threshold, int mode, int16_t *s16,
           std::vector<int64_t> *cands, const int64_t **dcands, int64_t *n_dcands, hipStream_t st);
int plan_ready(State *s, const uint8_t *hcodes, const int32_t *hoff, const int32_t *hlen, int32_t n_adp,
               const std::vector<int> &fb_rows, const pcabi::Scoring &sc, double threshold, int mode, hipStream_t st);
int bounds_dev(State *s, const uint8_t *codes, const int64_t *v_off, const int32_t *v_len, int64_t n,
               const int32_t *n_dev, int32_t n_adp, const pcabi::Scoring &sc, const int64_t **dcands,
               const unsigned long long **dcount, const int32_t **flags, const int4 **vlist, const int32_t **vcount,
               const int32_t **pmap, int64_t *vcap, hipStream_t st);
bool grow_after_overflow(State *s, int raw_overflow, int task_overflow);
void shrink_next(State *s, int bits);
void serial_next(State *s);
const int64_t *seg_cum_dev(State *s);
int seg_positions();
void cert_bounds(State *s, std::vector<int32_t> &U);
int debug_counts(State *s, int64_t (&out)[5], hipStream_t st);
void profile_events(State *s, hipEvent_t *ev);
int profile_counts(State *s, int64_t (&out)[3], hipStream_t st);
int profile_band_stats(State *s, bool on);
int band_stats(State *s, unsigned long long (&out)[8]);
int band_e(State *s, int c);
}  // namespace pcabi_seed
