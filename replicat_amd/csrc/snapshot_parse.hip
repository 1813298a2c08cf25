// snapshot_parse.hip -- the record array inside a snapshot's `data`, read back
// (include/replicat_snapshot.h, "Reading `data`"): from the JSON text serialize wrote to the parts
// of every file as arrays, the sums the listings need, the position of every part in its file, and
// the text that is left when the parts are taken out.  The inverse of snapshot_data.hip.
//
// serialize escapes every quote inside a JSON string, so the ten bytes {"range":[ stand in the text
// only where a part starts and "chunks":[ only where a list starts: no JSON parser, a pattern
// search and one strict lane per part.  The device accepts exactly what serialize writes; a text
// with anything else gets the status RC_PARTS_NOT_CANONICAL and goes to json.loads on the host
// (replicat_amd/snapshots.py), which also judges everything outside the parts.
//
//   find     one lane per aligned 16-byte granule of global memory that holds a byte of the text,
//            256 granules per workgroup, staged through LDS with the granule before and the one
//            behind (the 10-byte look-behind and the 9-byte look-ahead).  A lane matches its 16
//            positions in registers: unaligned words by funnel shifts, no byte loads.  Positions
//            before the text's first byte or whose ten bytes pass its last one are refused by their
//            offsets, whatever the bytes there say.  First pass: counts of parts and of first
//            parts per workgroup (gc.hip's scan turns them into prefixes); second pass: the same
//            masks again, and every part's offset, run ordinal and first-flag into its record.
//   parse    one lane per part: the text through aligned 32-bit loads, strict literals and
//            canonical decimals; the separator behind the part decides what the next record must
//            be, which makes the parts of a list a chain without gaps.
//   sums     sizes summed per workgroup, gc.hip's scan over the workgroups, the exclusive prefix
//            per part (optionally through a permutation: the stable order by run and counter), and
//            from the prefix every part's position and every run's and text's size.
//   strip    one wave per fixed piece (the text between two lists): a byte copy to its place in
//            the stripped text.
#include <hip/hip_runtime.h>

#include "snapshot_device.h"

namespace {

// {"range":[ and "chunks":[ as little-endian words: bytes 0-3, 4-7 and 8-9
constexpr uint32_t kPart0 = 0x6172227Bu, kPart1 = 0x2265676Eu, kPart2 = 0x5B3Au;
constexpr uint32_t kList0 = 0x75686322u, kList1 = 0x22736B6Eu, kList2 = 0x5B3Au;

// The word at byte j of the window w (j is a constant once the caller's loop is unrolled).
__device__ __forceinline__ uint32_t word_at(const uint32_t (&w)[12], int j) {
    return __funnelshift_r(w[j >> 2], w[(j >> 2) + 1], 8 * (j & 3));
}

}  // namespace

// kScatter false: counts[0][b] = the parts that start in workgroup b's granules, counts[1][b] the
// first parts among them.  kScatter true: the two arrays hold their exclusive prefixes (the sums at
// [n_blocks]) and every part gets words 0 (run), 5, 6 (offset) and 7 (first-flag) of its record.
template <bool kScatter>
__global__ __launch_bounds__(kSnapThreads) void rc_snap_find_kernel(const SnapParseText *texts, uint64_t n_texts,
                                                                     const SnapBlock *blocks, uint64_t n_blocks,
                                                                     uint64_t *part_counts, uint64_t *first_counts,
                                                                     uint64_t capacity, uint32_t *records,
                                                                     uint64_t *text_first, uint64_t *text_run_first,
                                                                     uint64_t *run_part_first) {
    __shared__ u32x4 gran[kSnapThreads + 2];
    __shared__ uint32_t scan[kSnapThreads];
    const SnapBlock b = blocks[blockIdx.x];
    const SnapParseText t = texts[b.item];
    const uint32_t skew = uint32_t(t.ptr & 15);
    // only granules that hold a byte of the text are loaded; the others read as zeros
    const uint64_t granules = t.len ? (skew + t.len + 15) >> 4 : 0;
    const GLOBAL u32x4 *src = reinterpret_cast<const GLOBAL u32x4 *>(t.ptr - skew);
    const uint64_t g0 = uint64_t(b.block) * kSnapThreads, g = g0 + threadIdx.x;
    const u32x4 zero = {0, 0, 0, 0};
    gran[threadIdx.x + 1] = g < granules ? src[g] : zero;
    if (threadIdx.x == 0) {
        gran[0] = g0 > 0 && g0 - 1 < granules ? src[g0 - 1] : zero;
        gran[kSnapThreads + 1] = g0 + kSnapThreads < granules ? src[g0 + kSnapThreads] : zero;
    }
    __syncthreads();
    uint32_t w[12];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const u32x4 v = gran[threadIdx.x + q];
        w[4 * q] = v.x;
        w[4 * q + 1] = v.y;
        w[4 * q + 2] = v.z;
        w[4 * q + 3] = v.w;
    }
    // byte 16 + k of the window is the text's byte p0 + k
    const int64_t p0 = int64_t(g * 16) - int64_t(skew);
    uint32_t parts = 0, firsts = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int j = 16 + k;
        const int64_t p = p0 + k;
        // the text's bounds by logic: the ten bytes lie inside [0, len), the ten before them too
        const bool inside = p >= 0 && uint64_t(p) + 10 <= t.len;
        const bool part = inside && word_at(w, j) == kPart0 && word_at(w, j + 4) == kPart1 &&
                          (word_at(w, j + 8) & 0xFFFFu) == kPart2;
        const bool first = part && p >= 10 && word_at(w, j - 10) == kList0 && word_at(w, j - 6) == kList1 &&
                           (word_at(w, j - 2) & 0xFFFFu) == kList2;
        parts |= uint32_t(part) << k;
        firsts |= uint32_t(first) << k;
    }
    // at most 4096 / 10 parts per workgroup: both counts in one word
    uint32_t sum;
    const uint32_t before = block_scan(uint32_t(__popc(parts)) | (uint32_t(__popc(firsts)) << 16), scan, sum);
    if (!kScatter) {
        if (threadIdx.x == 0) {
            part_counts[blockIdx.x] = sum & 0xFFFFu;
            first_counts[blockIdx.x] = sum >> 16;
        }
        return;
    }
    if (threadIdx.x == 0) {
        if (b.block == 0) {
            text_first[b.item] = part_counts[blockIdx.x];
            text_run_first[b.item] = first_counts[blockIdx.x];
        }
        if (blockIdx.x == 0) {
            const uint64_t total = part_counts[n_blocks] < capacity ? part_counts[n_blocks] : capacity;
            text_first[n_texts] = part_counts[n_blocks];
            text_run_first[n_texts] = first_counts[n_blocks];
            // a run is a first part: no more runs than parts
            run_part_first[first_counts[n_blocks] < capacity ? first_counts[n_blocks] : capacity] = total;
        }
    }
    uint64_t at = part_counts[blockIdx.x] + (before & 0xFFFFu);
    uint64_t run = first_counts[blockIdx.x] + (before >> 16);  // the first parts before this one
    while (parts) {
        const uint32_t k = uint32_t(__ffs(parts)) - 1;
        parts &= parts - 1;
        const uint32_t first = (firsts >> k) & 1u;
        run += first;
        if (at < capacity) {  // a text that is not canonical can hold a part every ten bytes
            uint32_t *rec = records + kSnapPartWords * at;
            const uint64_t off = uint64_t(p0 + int64_t(k));
            rec[0] = uint32_t(run - 1);  // 0xFFFFFFFF: no list has begun
            rec[5] = uint32_t(off);
            rec[6] = uint32_t(off >> 32);
            rec[7] = first;
        }
        ++at;
    }
}

__global__ __launch_bounds__(kSnapThreads) void rc_snap_parse_kernel(const SnapParseText *texts, uint64_t n_texts,
                                                                      const uint64_t *text_first,
                                                                      const uint64_t *text_run_first, uint64_t capacity,
                                                                      uint32_t *records, uint64_t *run_off,
                                                                      uint64_t *run_end, uint64_t *run_part_first,
                                                                      uint8_t *status) {
    const uint64_t g = uint64_t(blockIdx.x) * kSnapThreads + threadIdx.x;
    if (g < n_texts) {
        // more parts than a canonical text of that length can hold, or records that found no room
        const uint64_t room = texts[g].room;
        if (text_first[g + 1] - text_first[g] > room || text_first[g + 1] > capacity)
            status[g] = RC_PARTS_NOT_CANONICAL;
    }
    const uint64_t total = text_first[n_texts] < capacity ? text_first[n_texts] : capacity;
    if (g >= total) return;
    const uint64_t i = owner_of(text_first, n_texts, g);
    const SnapParseText t = texts[i];
    uint32_t *rec = records + kSnapPartWords * g;
    const uint32_t run = rec[0], first = rec[7] & kSnapPartFirst;
    const uint64_t off = uint64_t(rec[5]) | (uint64_t(rec[6]) << 32);
    TextReader r{static_cast<uintptr_t>(t.ptr), t.len};
    uint64_t p = off + 10;  // the ten bytes the find kernel matched
    uint32_t start, end, index, counter;
    bool ok = decimal(r, p, start);
    ok &= literal(r, p, ",");
    ok &= decimal(r, p, end);
    ok &= literal(r, p, "],\"index\":");
    ok &= decimal(r, p, index);
    ok &= literal(r, p, ",\"counter\":");
    ok &= decimal(r, p, counter);
    ok &= literal(r, p, "}");
    ok &= start <= end;
    const uint32_t sep = r.byte(p);
    // the record behind this one, if it is of the same text: only its words 0, 5 and 6, which no
    // lane of this launch writes (word 7 gets its lane's last-flag).  The run ordinal counts the
    // first parts up to and including a part, so the next part is a first part exactly when its
    // ordinal is not this part's.
    const uint64_t text_end = text_first[i + 1] < total ? text_first[i + 1] : total;
    const bool has_next = g + 1 < text_end;
    bool next_first = false;
    uint64_t next_off = 0;
    if (has_next) {
        next_first = rec[kSnapPartWords] != run;
        next_off = uint64_t(rec[kSnapPartWords + 5]) | (uint64_t(rec[kSnapPartWords + 6]) << 32);
    }
    const bool last = sep == ']';
    if (last)
        ok &= !has_next || next_first;  // a list ended: the next part begins one
    else
        ok &= sep == ',' && has_next && !next_first && next_off == p + 1;  // the next part, on the next byte
    ok &= first || g > text_first[i];  // the first part of a text begins a list
    rec[1] = start;
    rec[2] = end;
    rec[3] = index;
    rec[4] = counter;
    rec[7] = first | (last ? kSnapPartLast : 0u);
    if (first) {  // run < the number of first parts <= capacity
        run_off[run] = off;
        run_part_first[run] = g;
    }
    // only a run of this text: the ordinal of a part before any list is another text's
    if (last && run >= text_run_first[i] && run < text_run_first[i + 1] && run < capacity) run_end[run] = p;
    if (!ok) status[i] = RC_PARTS_NOT_CANONICAL;  // every lane stores the same value
}

// sums[b] = the summed sizes (end - start) of parts order[256 b ..] (order null: the listed order).
__global__ __launch_bounds__(kSnapThreads) void rc_snap_size_sums_kernel(const uint32_t *records, const uint64_t *order,
                                                                          const uint64_t *part_total, uint64_t capacity,
                                                                          uint64_t *sums, uint64_t *excl) {
    __shared__ uint64_t scan[kSnapThreads];
    const uint64_t total = *part_total < capacity ? *part_total : capacity;
    const uint64_t k = uint64_t(blockIdx.x) * kSnapThreads + threadIdx.x;
    uint64_t size = 0;
    if (k < total) {
        const uint64_t g = order ? order[k] : k;
        if (g < total) size = uint64_t(records[kSnapPartWords * g + 2]) - records[kSnapPartWords * g + 1];
    }
    uint64_t sum;
    const uint64_t before = block_scan(size, scan, sum);
    if (k <= total) excl[k] = before;  // within the workgroup; the positions kernel adds the rest
    if (threadIdx.x == 0) sums[blockIdx.x] = sum;
}

// With excl[k] + group_off[k / 256] the summed sizes before the k-th part in `order`: the position
// of every part in its file, whether a run's counters increase strictly as listed, and per run and
// per text the sums.
__global__ __launch_bounds__(kSnapThreads) void rc_snap_positions_kernel(
    const uint32_t *records, const uint64_t *order, const uint64_t *text_first, const uint64_t *text_run_first,
    uint64_t n_texts, uint64_t capacity, const uint64_t *run_part_first, const uint64_t *excl,
    const uint64_t *group_off, uint64_t *position, uint64_t *run_count, uint64_t *run_size, uint8_t *run_sorted,
    uint64_t *text_size) {
    const uint64_t total = text_first[n_texts] < capacity ? text_first[n_texts] : capacity;
    const uint64_t runs = text_run_first[n_texts] < capacity ? text_run_first[n_texts] : capacity;
    const uint64_t k = uint64_t(blockIdx.x) * kSnapThreads + threadIdx.x;
    auto before = [&](uint64_t q) {  // q <= total
        return excl[q] + group_off[q / kSnapThreads];
    };
    if (k < total) {
        const uint64_t g = order ? order[k] : k;
        if (g < total) {
            const uint32_t run = records[kSnapPartWords * g];
            uint64_t head = run < runs ? run_part_first[run] : k;
            if (head > k) head = k;  // a text that is not canonical
            position[g] = before(k) - before(head);
            if (!order && k > head && run < runs &&
                records[kSnapPartWords * k + 4] <= records[kSnapPartWords * (k - 1) + 4]) {
                // a part of a text that is not canonical may carry the ordinal of another text's run
                const uint64_t i = owner_of(text_first, n_texts, k);
                if (run >= text_run_first[i] && run < text_run_first[i + 1])
                    run_sorted[run] = 0;  // every lane stores the same value
            }
        }
    }
    if (k < runs) {
        // a run ends where the next begins, or with the parts of its text
        const uint64_t i = owner_of(text_run_first, n_texts, k);
        uint64_t a = run_part_first[k], b = run_part_first[k + 1];
        if (b > text_first[i + 1]) b = text_first[i + 1];
        if (b > total) b = total;
        if (a > b) a = b;
        run_count[k] = b - a;
        run_size[k] = before(b) - before(a);
    }
    if (k < n_texts) {
        uint64_t a = text_first[k], b = text_first[k + 1];
        if (b > total) b = total;
        if (a > b) a = b;
        text_size[k] = before(b) - before(a);
    }
}

// local[r] = the bytes of the runs before run r in its workgroup of 256 runs, sums[b] the bytes of
// workgroup b's runs: a run's bytes go from its first part to the ']' that ends it (without it),
// and are 0 behind the last run, up to `capacity`.
__global__ __launch_bounds__(kSnapThreads) void rc_snap_run_len_kernel(const uint64_t *run_off, const uint64_t *run_end,
                                                                        const uint64_t *run_total, uint64_t capacity,
                                                                        uint64_t *local, uint64_t *sums) {
    __shared__ uint64_t scan[kSnapThreads];
    const uint64_t r = uint64_t(blockIdx.x) * kSnapThreads + threadIdx.x;
    const uint64_t runs = *run_total < capacity ? *run_total : capacity;
    uint64_t sum;
    const uint64_t before = block_scan(r < runs ? run_end[r] - run_off[r] : uint64_t(0), scan, sum);
    if (r <= capacity) local[r] = before;
    if (threadIdx.x == 0) sums[blockIdx.x] = sum;
}

// One wave per fixed piece of a canonical text: piece k of a text with R runs is the bytes from the
// ']' of run k - 1 (the text's start for k = 0) to the first part of run k (the text's end for
// k = R), and moves down by the bytes of the runs before it.
__global__ __launch_bounds__(kSnapThreads) void rc_snap_strip_kernel(const SnapParseText *texts, uint64_t n_texts,
                                                                      const uint64_t *text_run_first, uint64_t capacity,
                                                                      const uint64_t *run_off, const uint64_t *run_end,
                                                                      const uint64_t *run_local,
                                                                      const uint64_t *run_group_off,
                                                                      const uint8_t *status, uint8_t *out,
                                                                      uint64_t *run_close,
                                                                      uint64_t *stripped_len) {
    const uint64_t q = uint64_t(blockIdx.x) * (kSnapThreads / 64) + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t runs = text_run_first[n_texts];
    if (q >= runs + n_texts) return;
    // text i's pieces are text_run_first[i] + i .. text_run_first[i + 1] + i: the last i whose first is <= q
    uint64_t lo = 0, hi = n_texts;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (text_run_first[mid] + mid <= q)
            lo = mid + 1;
        else
            hi = mid;
    }
    const uint64_t i = lo - 1;
    const SnapParseText t = texts[i];
    const uint64_t r0 = text_run_first[i], count = text_run_first[i + 1] - r0, k = q - (r0 + i);
    if (status[i] != RC_PARTS_OK) {  // its arrays mean nothing
        if (k == 0 && lane == 0) stripped_len[i] = 0;
        return;
    }
    const uint64_t from = k == 0 ? 0 : run_end[r0 + k - 1];
    const uint64_t to = k == count ? t.len : run_off[r0 + k];
    // a canonical text's runs lie below capacity
    auto before = [&](uint64_t r) { return run_local[r] + run_group_off[r / kSnapThreads]; };
    const uint64_t removed = before(r0 + k) - before(r0);
    if (to > t.len || from > to || removed > from) return;  // cannot happen in a canonical text
    const uint8_t *src = reinterpret_cast<const uint8_t *>(t.ptr) + from;
    uint8_t *dst = out + t.out + (from - removed);
    for (uint64_t x = lane; x < to - from; x += 64) dst[x] = src[x];
    if (lane == 0) {
        if (k < count)
            run_close[r0 + k] = to - removed;  // where the next piece puts its ']'
        else
            stripped_len[i] = t.len - removed;
    }
}

int rc_snap_launch_find(bool scatter, const SnapParseText *d_texts, uint64_t n_texts, const SnapBlock *d_blocks,
                        uint64_t n_blocks, uint64_t *d_part_counts, uint64_t *d_first_counts, uint64_t capacity,
                        uint32_t *d_records, uint64_t *d_text_first, uint64_t *d_text_run_first,
                        uint64_t *d_run_part_first, hipStream_t st) {
    unsigned grid;
    if (int rc = grid_of(n_blocks, 1, "text", grid)) return rc;
    if (!grid) return 0;
    if (scatter)
        rc_snap_find_kernel<true><<<grid, kSnapThreads, 0, st>>>(d_texts, n_texts, d_blocks, n_blocks, d_part_counts,
                                                                 d_first_counts, capacity, d_records, d_text_first,
                                                                 d_text_run_first, d_run_part_first);
    else
        rc_snap_find_kernel<false><<<grid, kSnapThreads, 0, st>>>(d_texts, n_texts, d_blocks, n_blocks, d_part_counts,
                                                                  d_first_counts, capacity, d_records, d_text_first,
                                                                  d_text_run_first, d_run_part_first);
    return rc::launch_status("rc_snap_find_kernel");
}

int rc_snap_launch_parse(const SnapParseText *d_texts, uint64_t n_texts, const uint64_t *d_text_first,
                         const uint64_t *d_text_run_first, uint64_t capacity, uint32_t *d_records, uint64_t *d_run_off,
                         uint64_t *d_run_end, uint64_t *d_run_part_first, uint8_t *d_status, hipStream_t st) {
    unsigned grid;
    if (int rc = grid_of(capacity > n_texts ? capacity : n_texts, kSnapThreads, "parts", grid)) return rc;
    if (!grid) return 0;
    rc_snap_parse_kernel<<<grid, kSnapThreads, 0, st>>>(d_texts, n_texts, d_text_first, d_text_run_first, capacity,
                                                        d_records, d_run_off, d_run_end, d_run_part_first, d_status);
    return rc::launch_status("rc_snap_parse_kernel");
}

int rc_snap_launch_size_sums(const uint32_t *d_records, const uint64_t *d_order, const uint64_t *d_part_total,
                             uint64_t capacity, uint64_t *d_sums, uint64_t *d_excl, hipStream_t st) {
    unsigned grid;
    if (int rc = grid_of(capacity + 1, kSnapThreads, "parts", grid)) return rc;
    rc_snap_size_sums_kernel<<<grid, kSnapThreads, 0, st>>>(d_records, d_order, d_part_total, capacity, d_sums, d_excl);
    return rc::launch_status("rc_snap_size_sums_kernel");
}

int rc_snap_launch_positions(const uint32_t *d_records, const uint64_t *d_order, const uint64_t *d_text_first,
                             const uint64_t *d_text_run_first, uint64_t n_texts, uint64_t capacity,
                             const uint64_t *d_run_part_first, const uint64_t *d_excl, const uint64_t *d_group_off,
                             uint64_t *d_position, uint64_t *d_run_count, uint64_t *d_run_size, uint8_t *d_run_sorted,
                             uint64_t *d_text_size, hipStream_t st) {
    unsigned grid;
    if (int rc = grid_of(capacity > n_texts ? capacity : n_texts, kSnapThreads, "parts", grid)) return rc;
    if (!grid) return 0;
    rc_snap_positions_kernel<<<grid, kSnapThreads, 0, st>>>(d_records, d_order, d_text_first, d_text_run_first, n_texts,
                                                            capacity, d_run_part_first, d_excl, d_group_off, d_position,
                                                            d_run_count, d_run_size, d_run_sorted, d_text_size);
    return rc::launch_status("rc_snap_positions_kernel");
}

int rc_snap_launch_run_len(const uint64_t *d_run_off, const uint64_t *d_run_end, const uint64_t *d_run_total,
                           uint64_t capacity, uint64_t *d_local, uint64_t *d_sums, hipStream_t st) {
    unsigned grid;
    if (int rc = grid_of(capacity + 1, kSnapThreads, "runs", grid)) return rc;
    rc_snap_run_len_kernel<<<grid, kSnapThreads, 0, st>>>(d_run_off, d_run_end, d_run_total, capacity, d_local, d_sums);
    return rc::launch_status("rc_snap_run_len_kernel");
}

int rc_snap_launch_strip(const SnapParseText *d_texts, uint64_t n_texts, const uint64_t *d_text_run_first,
                         uint64_t capacity, const uint64_t *d_run_off, const uint64_t *d_run_end,
                         const uint64_t *d_run_local, const uint64_t *d_run_group_off, const uint8_t *d_status,
                         uint8_t *d_out, uint64_t *d_run_close, uint64_t *d_stripped_len, hipStream_t st) {
    unsigned grid;
    if (int rc = grid_of(capacity + n_texts, kSnapThreads / 64, "pieces", grid)) return rc;
    if (!grid) return 0;
    rc_snap_strip_kernel<<<grid, kSnapThreads, 0, st>>>(d_texts, n_texts, d_text_run_first, capacity, d_run_off,
                                                        d_run_end, d_run_local, d_run_group_off, d_status, d_out,
                                                        d_run_close, d_stripped_len);
    return rc::launch_status("rc_snap_strip_kernel");
}
