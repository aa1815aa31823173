// pcabi_pieces.h -- the one rule for "the pieces of a read": what the writers' part enumeration
// (pcabi_write.cpp read_parts) leaves of a split read, as a list the quality stage can judge piece by piece
// (pcabi_qual.hip pcabi_qual_pieces_*; include/pcabi.h; DESIGN.md "Quality stage"). Nothing here is
// device-only: the kernels and the host build run the same code.
//
// Read r has the trimmed length tl and the ranges [cuts[2k], cuts[2k + 1]) for k in [cut_off[r],
// cut_off[r + 1]): positions of the trimmed sequence, in any order; they may overlap, nest, repeat, be
// empty, begin below 0 or end beyond tl. The read is split when at least one of its ranges is non-empty
// (end > begin), even if that range lies wholly outside [0, tl): the single piece is then [0, tl). The
// pieces are the maximal runs of positions of [0, tl) that no non-empty range covers, ascending; runs of
// length 0 do not exist. A read that is not split has no pieces.
//
// The walk takes the ranges in ascending order of sort_key (the begin clamped to [0, tl]: clamping changes
// nothing a range covers of [0, tl), and keeps the key in 31 bits); among equal keys any order gives the
// same pieces, as only the furthest end counts.
#pragma once
#include <cstdint>

#ifndef PCABI_HD
#if defined(__HIPCC__)
#define PCABI_HD __host__ __device__
#else
#define PCABI_HD
#endif
#endif

namespace pcabi_pieces {

PCABI_HD inline int64_t sort_key(int64_t begin, int64_t tl) { return begin < 0 ? 0 : begin > tl ? tl : begin; }

// The pieces of a read of tl positions whose m ranges range_at(j) -> (begin, end), j = 0..m - 1, come in
// ascending sort_key order (empty ones among them are skipped): piece(j, begin, end) for piece j = 0, 1,
// ..., ascending. Returns the number of pieces; 0 for a read that is not split.
template <class RangeAt, class Piece>
PCABI_HD inline int64_t walk(int64_t tl, int64_t m, RangeAt &&range_at, Piece &&piece) {
    if (tl < 0) tl = 0;
    int64_t n = 0, covered = 0;   // every position below `covered` is cut or in a piece already
    bool split = false;
    for (int64_t j = 0; j < m; ++j) {
        int64_t b, e;
        range_at(j, &b, &e);
        if (e <= b) continue;
        split = true;
        if (covered >= tl) continue;
        const int64_t stop = b < tl ? b : tl;
        if (stop > covered) piece(n++, covered, stop), covered = stop;
        if (e > covered) covered = e;
    }
    if (split && covered < tl) piece(n++, covered, tl);
    return n;
}

// The two ranges a judged piece [begin, end) adds to its read's cuts: a piece that passes loses its crops,
// [begin, begin + front) and [end - tail, end) (either may be empty); one that fails goes whole, [begin,
// end) and the empty [end, end). The writers ignore empty ranges.
PCABI_HD inline void piece_ranges(int64_t begin, int64_t end, int64_t front, int64_t tail, bool failed, int64_t *out4) {
    out4[0] = begin, out4[1] = failed ? end : begin + front;
    out4[2] = failed ? end : end - tail, out4[3] = end;
}

}  // namespace pcabi_pieces
