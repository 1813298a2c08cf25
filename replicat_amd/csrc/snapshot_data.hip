// snapshot_data.hip -- the record array inside a snapshot's `data` (include/replicat_snapshot.h,
// "Writing `data`"): from the cuts of the stream and the bounds of its files to the parts of every
// file, and from the parts to their JSON text.  snapshot_write.hip's conventions: kSnapThreads
// lanes, one record per lane, a workgroup's text built in LDS and stored as aligned 16-byte
// granules of which only the workgroup's own bytes are written.
//
// _chunk_done (replicat/repository.py:1374-1411) gives a file one part per chunk that touches it,
//     {"range":[S,E],"index":I,"counter":C}
// and a chunk touches a file when file_start <= chunk_end and file_end >= chunk_start.  Chunks
// tile the stream, so the chunks of file f are the run lo .. hi with
//     lo = lower_bound(chunk_ends, file_start[f])
//     hi = min(upper_bound(chunk_ends, file_end[f]), n - 1)
// which also yields the reference's empty parts: [len,len] in the chunk that ends where the file
// starts, [0,0] in the chunk that starts where it ends.
//
//   count    one lane per file: the two searches; lo[f] and the number of parts.  The shared scan
//            (gc.hip) turns the counts into part_first[m + 1].
//   records  one lane per part: its file by a search in part_first, its chunk lo[f] + (p -
//            part_first[f]), the six numbers, the length of its text, the sum of the lengths
//            before it in its workgroup (rel) and the workgroup's sum.
//   offsets  one lane per fixed piece (the host's text between two files' lists): where it goes.
//   encode   one lane per part: the text of its record into LDS, byte by byte -- decimal digits
//            by multiply-high, no table -- at an LDS position congruent to its destination
//            modulo 16.  A workgroup's 256 parts may belong to several files, and between two
//            files' parts lies a fixed piece this kernel must not touch: the parts of one file
//            are a RUN, every run is placed 32 bytes further than its text alone would put it,
//            so that no two runs share a granule, and remembers the distance between its LDS
//            position and its destination.  LDS starts zeroed and JSON has no zero byte, so a
//            granule's own bytes are its non-zero ones: a granule without a zero leaves as one
//            16-byte store, one with some as byte stores, an empty one not at all.
//   place    one wave per fixed piece: a byte copy to its offset.
#include <hip/hip_runtime.h>

#include "snapshot_device.h"

namespace {

constexpr uint32_t kRunPad = 32;  // >= 15 + 16: two runs never share a granule, whatever their skews
constexpr uint32_t kDataLds = (kSnapThreads * (kSnapPartMaxLen + kRunPad) + 16 + 15) / 16 * 16;
constexpr uint32_t kRelMask = 0xFFFFu;       // rel < 256 * 74
constexpr uint32_t kLastPart = 0x80000000u;  // in the rel word: the last part of its file
static_assert(kSnapThreads * kSnapPartMaxLen <= kRelMask, "rel fits 16 bits");
static_assert(kSnapThreads <= 256, "a run's number fits a byte");

template <int N>
__device__ __forceinline__ uint32_t put_text(uint8_t *lds, uint32_t at, const char (&s)[N]) {
#pragma unroll
    for (int k = 0; k < N - 1; ++k) lds[at + k] = uint8_t(s[k]);
    return at + (N - 1);
}

// v in nd = rc_snap_digits(v) decimal digits: v / 10 as the high half of v * ceil(2^35 / 10)
__device__ __forceinline__ uint32_t put_decimal(uint8_t *lds, uint32_t at, uint32_t v, uint32_t nd) {
#pragma unroll
    for (uint32_t k = 0; k < 10; ++k) {
        if (k < nd) {
            const uint32_t q = __umulhi(v, 0xCCCCCCCDu) >> 3;
            lds[at + nd - 1 - k] = uint8_t('0' + (v - q * 10));
            v = q;
        }
    }
    return at + nd;
}

// v has a zero byte
__device__ __forceinline__ bool has_zero(uint32_t v) { return ((v - 0x01010101u) & ~v & 0x80808080u) != 0; }

}  // namespace

__global__ __launch_bounds__(kSnapThreads) void rc_snap_part_count_kernel(const uint64_t *ends, uint64_t n,
                                                                           const uint64_t *file_start,
                                                                           const uint64_t *file_end, uint64_t m,
                                                                           uint64_t *counts, uint32_t *lo_out) {
    const uint64_t f = uint64_t(blockIdx.x) * kSnapThreads + threadIdx.x;
    if (f >= m) return;
    const uint64_t lo = bound(ends, n, file_start[f], false);
    const uint64_t ub = bound(ends, n, file_end[f], true);
    const uint64_t hi = ub < n - 1 ? ub : n - 1;
    // valid bounds give lo <= hi < n; anything else lists nothing rather than leaving the arrays
    counts[f] = lo < n && hi >= lo ? hi - lo + 1 : 0;
    lo_out[f] = uint32_t(lo < n ? lo : 0);
}

__global__ __launch_bounds__(kSnapThreads) void rc_snap_part_records_kernel(
    const uint64_t *ends, const uint32_t *table_index, uint32_t counter0, const uint64_t *file_start,
    const uint64_t *file_end, uint64_t m, const uint64_t *part_first, const uint32_t *lo, uint64_t capacity,
    uint32_t *records, uint64_t *group_len) {
    __shared__ uint32_t scan[kSnapThreads];
    const uint64_t p = uint64_t(blockIdx.x) * kSnapThreads + threadIdx.x;
    const uint64_t total = part_first[m] < capacity ? part_first[m] : capacity;
    if (uint64_t(blockIdx.x) * kSnapThreads >= total) {  // the whole workgroup: capacity is a bound
        if (threadIdx.x == 0) group_len[blockIdx.x] = 0;
        return;
    }
    u32x4 a = {0, 0, 0, 0}, b = {0, 0, 0, 0};
    uint32_t len = 0, last = 0;
    if (p < total) {
        const uint64_t f = bound(part_first, m, p, true) - 1;  // part_first[0] = 0 <= p
        const uint64_t first = part_first[f];
        const uint64_t k = lo[f] + (p - first);
        const uint64_t start_k = k ? ends[k - 1] : 0, end_k = ends[k];
        const uint64_t fs = file_start[f], fe = file_end[f];
        a.x = uint32_t(f);
        a.y = uint32_t(k);
        a.z = uint32_t(fs > start_k ? fs - start_k : 0);
        a.w = uint32_t((fe < end_k ? fe : end_k) - start_k);
        b.x = table_index[k];
        b.y = counter0 + uint32_t(k);
        len = rc_snap_part_len(a.z, a.w, b.x, b.y);
        last = p + 1 == part_first[f + 1] ? kLastPart : 0u;
    }
    uint32_t sum;
    const uint32_t rel = block_scan(len, scan, sum);
    if (p < total) {
        b.z = len;
        b.w = rel | last;
        u32x4 *rec = reinterpret_cast<u32x4 *>(records + kSnapPartWords * p);
        rec[0] = a;
        rec[1] = b;
    }
    if (threadIdx.x == 0) group_len[blockIdx.x] = sum;
}

__global__ __launch_bounds__(kSnapThreads) void rc_snap_piece_offsets_kernel(
    const uint64_t *part_first, uint64_t m, const uint32_t *records, uint64_t capacity, const uint64_t *group_off,
    uint64_t groups, const uint64_t *piece_pre, uint64_t *piece_off, uint64_t *total_len) {
    const uint64_t j = uint64_t(blockIdx.x) * kSnapThreads + threadIdx.x;
    if (j > m) return;
    const uint64_t total = part_first[m] < capacity ? part_first[m] : capacity;
    const uint64_t p = part_first[j];
    // the text of the parts before piece j: those of files 0 .. j - 1
    const uint64_t before = p < total ? group_off[p / kSnapThreads] + (records[kSnapPartWords * p + 7] & kRelMask)
                                      : group_off[groups];
    const uint64_t at = piece_pre[j] + before;
    piece_off[j] = at;
    if (j == m) *total_len = at + (piece_pre[m + 1] - piece_pre[m]);
}

__global__ __launch_bounds__(kSnapThreads) void rc_snap_encode_data_kernel(const uint32_t *records,
                                                                            const uint64_t *part_total,
                                                                            uint64_t capacity,
                                                                            const uint64_t *group_off,
                                                                            const uint64_t *piece_pre,
                                                                            uint8_t *text) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[kDataLds];
    __shared__ uint64_t run_delta[kSnapThreads];     // destination address - LDS position of run r
    __shared__ uint8_t granule_run[kDataLds / 16];   // the run a granule's bytes belong to
    __shared__ uint32_t files[kSnapThreads];
    __shared__ uint32_t wave_heads[kSnapThreads / 64];
    const uint64_t total = *part_total < capacity ? *part_total : capacity;
    const uint64_t p = uint64_t(blockIdx.x) * kSnapThreads + threadIdx.x;
    if (uint64_t(blockIdx.x) * kSnapThreads >= total) return;  // the whole workgroup
    for (uint32_t q = threadIdx.x * 16; q < kDataLds; q += kSnapThreads * 16)
        *reinterpret_cast<u32x4 *>(lds + q) = u32x4{0, 0, 0, 0};
    const bool valid = p < total;
    u32x4 a = {0, 0, 0, 0}, b = {0, 0, 0, 0};
    if (valid) {
        const u32x4 *rec = reinterpret_cast<const u32x4 *>(records + kSnapPartWords * p);
        a = rec[0];
        b = rec[1];
    }
    files[threadIdx.x] = a.x;
    __syncthreads();  // the zeros and the files
    // a run: the parts of one file in this workgroup; r = the number of run heads before this lane
    const bool head = valid && (threadIdx.x == 0 || files[threadIdx.x - 1] != a.x);
    const unsigned long long ballot = __ballot(head);
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) wave_heads[wave] = uint32_t(__popcll(ballot));
    __syncthreads();
    if (valid) {
        uint32_t r = uint32_t(__popcll(ballot & ((2ull << lane) - 1))) - 1;  // a run's head counts itself
        for (uint32_t w = 0; w < wave; ++w) r += wave_heads[w];
        const uint32_t rel = b.w & kRelMask, len = b.z;
        const uint64_t dest = reinterpret_cast<uintptr_t>(text) + group_off[blockIdx.x] + rel + piece_pre[a.x + 1];
        const uint32_t pos = rel + kRunPad * r + uint32_t((dest - rel) & 15);  // = dest modulo 16
        if (head) run_delta[r] = dest - pos;
        uint32_t at = put_text(lds, pos, "{\"range\":[");
        at = put_decimal(lds, at, a.z, rc_snap_digits(a.z));
        at = put_text(lds, at, ",");
        at = put_decimal(lds, at, a.w, rc_snap_digits(a.w));
        at = put_text(lds, at, "],\"index\":");
        at = put_decimal(lds, at, b.x, rc_snap_digits(b.x));
        at = put_text(lds, at, ",\"counter\":");
        at = put_decimal(lds, at, b.y, rc_snap_digits(b.y));
        lds[at] = '}';
        lds[at + 1] = b.w & kLastPart ? ']' : ',';
        // lanes of one run write the same number into a granule they share
        for (uint32_t q = pos & ~15u; q < pos + len; q += 16) granule_run[q >> 4] = uint8_t(r);
    }
    __syncthreads();
    for (uint32_t q = threadIdx.x * 16; q < kDataLds; q += kSnapThreads * 16) {
        const u32x4 v = *reinterpret_cast<const u32x4 *>(lds + q);
        if ((v.x | v.y | v.z | v.w) == 0) continue;  // between two runs, or past the last
        gbytes g = reinterpret_cast<gbytes>(run_delta[granule_run[q >> 4]] + q);
        if (!(has_zero(v.x) || has_zero(v.y) || has_zero(v.z) || has_zero(v.w))) {
            *reinterpret_cast<GLOBAL u32x4 *>(g) = v;
        } else {  // the first or last granule of a run: its other bytes are a fixed piece's
            for (uint32_t k = 0; k < 16; ++k)
                if (lds[q + k]) g[k] = lds[q + k];
        }
    }
}

__global__ __launch_bounds__(kSnapThreads) void rc_snap_place_pieces_kernel(const uint8_t *pieces,
                                                                             const uint64_t *piece_pre,
                                                                             const uint64_t *piece_off,
                                                                             uint64_t count, uint8_t *text) {
    const uint64_t j = uint64_t(blockIdx.x) * (kSnapThreads / 64) + (threadIdx.x >> 6);
    if (j >= count) return;
    const uint64_t from = piece_pre[j], len = piece_pre[j + 1] - from;
    const uint8_t *src = pieces + from;
    uint8_t *dst = text + piece_off[j];
    for (uint64_t k = threadIdx.x & 63; k < len; k += 64) dst[k] = src[k];
}

int rc_snap_launch_part_count(const uint64_t *d_ends, uint64_t n, const uint64_t *d_file_start,
                              const uint64_t *d_file_end, uint64_t m, uint64_t *d_counts, uint32_t *d_lo,
                              hipStream_t st) {
    unsigned grid;
    if (int rc = grid_of(m, kSnapThreads, "files", grid)) return rc;
    if (!grid) return 0;
    rc_snap_part_count_kernel<<<grid, kSnapThreads, 0, st>>>(d_ends, n, d_file_start, d_file_end, m, d_counts, d_lo);
    return rc::launch_status("rc_snap_part_count_kernel");
}

int rc_snap_launch_part_records(const uint64_t *d_ends, const uint32_t *d_table_index, uint32_t counter0,
                                const uint64_t *d_file_start, const uint64_t *d_file_end, uint64_t m,
                                const uint64_t *d_part_first, const uint32_t *d_lo, uint64_t capacity,
                                uint32_t *d_records, uint64_t *d_group_len, hipStream_t st) {
    unsigned grid;
    if (int rc = grid_of(capacity, kSnapThreads, "parts", grid)) return rc;
    if (!grid) return 0;
    rc_snap_part_records_kernel<<<grid, kSnapThreads, 0, st>>>(d_ends, d_table_index, counter0, d_file_start,
                                                               d_file_end, m, d_part_first, d_lo, capacity, d_records,
                                                               d_group_len);
    return rc::launch_status("rc_snap_part_records_kernel");
}

int rc_snap_launch_piece_offsets(const uint64_t *d_part_first, uint64_t m, const uint32_t *d_records,
                                 uint64_t capacity, const uint64_t *d_group_off, const uint64_t *d_piece_pre,
                                 uint64_t *d_piece_off, uint64_t *d_total, hipStream_t st) {
    unsigned grid;
    if (int rc = grid_of(m + 1, kSnapThreads, "pieces", grid)) return rc;
    rc_snap_piece_offsets_kernel<<<grid, kSnapThreads, 0, st>>>(d_part_first, m, d_records, capacity, d_group_off,
                                                                rc_snap_part_groups(capacity), d_piece_pre,
                                                                d_piece_off, d_total);
    return rc::launch_status("rc_snap_piece_offsets_kernel");
}

int rc_snap_launch_encode_data(const uint32_t *d_records, const uint64_t *d_part_total, uint64_t capacity,
                               const uint64_t *d_group_off, const uint64_t *d_piece_pre, uint8_t *d_text,
                               hipStream_t st) {
    unsigned grid;
    if (int rc = grid_of(capacity, kSnapThreads, "parts", grid)) return rc;
    if (!grid) return 0;
    rc_snap_encode_data_kernel<<<grid, kSnapThreads, 0, st>>>(d_records, d_part_total, capacity, d_group_off,
                                                              d_piece_pre, d_text);
    return rc::launch_status("rc_snap_encode_data_kernel");
}

int rc_snap_launch_place_pieces(const uint8_t *d_pieces, const uint64_t *d_piece_pre, const uint64_t *d_piece_off,
                                uint64_t count, uint8_t *d_text, hipStream_t st) {
    unsigned grid;
    if (int rc = grid_of(count, kSnapThreads / 64, "pieces", grid)) return rc;
    if (!grid) return 0;
    rc_snap_place_pieces_kernel<<<grid, kSnapThreads, 0, st>>>(d_pieces, d_piece_pre, d_piece_off, count, d_text);
    return rc::launch_status("rc_snap_place_pieces_kernel");
}
