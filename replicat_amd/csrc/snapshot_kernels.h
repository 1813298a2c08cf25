// snapshot_kernels.h -- internal interface between snapshot.hip (kernels) and capi_snapshot.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/replicat_snapshot.h"

constexpr int kSnapThreads = 256;            // 4 waves; one record (tables) or 16 characters (bulk) per lane
constexpr uint32_t kSnapMaxStride = 98;      // a record of a 64-byte digest: 88 characters + 10
constexpr uint32_t kSnapLaneChars = 16;      // bulk base64: characters per lane ...
constexpr uint32_t kSnapLaneBytes = 12;      // ... and the bytes they decode to
constexpr uint64_t kSnapReject = ~uint64_t(0);  // a count / length the host already refused

// 4 * ceil(L / 3): the base64 characters of an L-byte digest; a record is 10 bytes longer
// ({"!b":" and "} and the separator after it).
__host__ __device__ inline uint32_t rc_snap_chars(uint32_t digest_bytes) { return 4 * ((digest_bytes + 2) / 3); }
inline uint32_t rc_snap_stride(uint32_t digest_bytes) { return rc_snap_chars(digest_bytes) + 10; }

// One plaintext table: `count` records (kSnapReject: no canonical table has this length) whose
// digests go to the 64-byte slots first, first + 1, ...
struct SnapTable {
    uint64_t ptr, len, count, first;
};

// One bulk base64 text and where its bytes go (len kSnapReject: not a multiple of 4).
struct SnapText {
    uint64_t ptr, len, out;
};

// One workgroup's share: the block-th run of kSnapThreads records (or of kSnapThreads *
// kSnapLaneChars characters) of item `item`.  Every item has at least one block.
struct SnapBlock {
    uint32_t item, block;
};

// status[t] |= RC_TABLE_NOT_CANONICAL for every table with a record that is not canonical; the
// digests of the others into d_slots.  Tables whose status is RC_TABLE_BAD_TAG are skipped.
int rc_snap_launch_tables(const SnapTable *d_tables, const SnapBlock *d_blocks, uint64_t n_blocks,
                          uint32_t digest_bytes, uint8_t *d_slots, uint8_t *d_status, hipStream_t stream);

// ok[t] = 0 for every text that is not canonical base64 (ok is 1 beforehand); the bytes of the
// others at their `out`.
int rc_snap_launch_b64(const SnapText *d_texts, const SnapBlock *d_blocks, uint64_t n_blocks, uint8_t *d_ok,
                       hipStream_t stream);

// snapshot_write.hip: the inverses.  A SnapTable is then a text to write (ptr, len = 1 + count *
// stride, or 2) from the `count` slots first, first + 1, ... of d_slots; a SnapText `len` bytes at
// ptr whose 4 ceil(len / 3) characters go to `out`; a block of the bulk encoder is kSnapThreads *
// kSnapLaneBytes bytes.
__global__ void rc_snap_encode_tables_kernel(const SnapTable *tables, const SnapBlock *blocks,
                                             uint32_t digest_bytes, const uint8_t *slots);
__global__ void rc_snap_b64_encode_kernel(const SnapText *texts, const SnapBlock *blocks);

// Exactly tables[t].len bytes at each table's ptr; reads 64 bytes per digest.
int rc_snap_launch_encode_tables(const SnapTable *d_tables, const SnapBlock *d_blocks, uint64_t n_blocks,
                                 uint32_t digest_bytes, const uint8_t *d_slots, hipStream_t stream);

// Exactly 4 ceil(len / 3) characters at each text's out.
int rc_snap_launch_b64_encode(const SnapText *d_texts, const SnapBlock *d_blocks, uint64_t n_blocks,
                              hipStream_t stream);

// snapshot_data.hip: the parts of the files of a snapshot and their text inside `data`.  A part is
// RC_SNAPSHOT_PART_WORDS words: file, chunk, start, end, index, counter, then the length of its
// text {"range":[S,E],"index":I,"counter":C} with the ',' or ']' behind it, then rel: the summed
// lengths of the parts before it in its workgroup of kSnapThreads (low 16 bits), and in the top bit
// whether it is the last part of its file.
constexpr uint32_t kSnapPartWords = RC_SNAPSHOT_PART_WORDS;
constexpr uint32_t kSnapPartFixed = 34;   // everything of a part's text but the digits
constexpr uint32_t kSnapPartMaxLen = 74;  // four numbers of ten digits

__host__ __device__ inline uint32_t rc_snap_digits(uint32_t v) {
    return 1u + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u) + (v >= 1000000u) +
           (v >= 10000000u) + (v >= 100000000u) + (v >= 1000000000u);
}
__host__ __device__ inline uint32_t rc_snap_part_len(uint32_t start, uint32_t end, uint32_t index, uint32_t counter) {
    return kSnapPartFixed + rc_snap_digits(start) + rc_snap_digits(end) + rc_snap_digits(index) + rc_snap_digits(counter);
}

// A file has a part in every chunk it touches, and two neighbouring files share at most two
// chunks: n chunks and m files have at most n + 2 m parts, in rc_snap_part_groups workgroups.
inline uint64_t rc_snap_part_capacity(uint64_t n, uint64_t m) { return n && m ? n + 2 * m : 0; }
inline uint64_t rc_snap_part_groups(uint64_t capacity) { return (capacity + kSnapThreads - 1) / kSnapThreads; }

// d_counts[f] = the parts of file f, d_lo[f] = the first chunk that touches it (n >= 1).
int rc_snap_launch_part_count(const uint64_t *d_ends, uint64_t n, const uint64_t *d_file_start,
                              const uint64_t *d_file_end, uint64_t m, uint64_t *d_counts, uint32_t *d_lo,
                              hipStream_t st);
// The parts d_part_first[m] (at most `capacity`) as records in file order, and per workgroup of
// parts the summed length of their text (all rc_snap_part_groups(capacity) words are written).
int rc_snap_launch_part_records(const uint64_t *d_ends, const uint32_t *d_table_index, uint32_t counter0,
                                const uint64_t *d_file_start, const uint64_t *d_file_end, uint64_t m,
                                const uint64_t *d_part_first, const uint32_t *d_lo, uint64_t capacity,
                                uint32_t *d_records, uint64_t *d_group_len, hipStream_t st);
// d_piece_off[j], j <= m: where fixed piece j starts in the text -- behind the pieces before it
// (d_piece_pre: the exclusive prefix of the m + 1 lengths, the sum at [m + 1]) and the parts of the
// files before it (d_group_off: the exclusive prefix of the workgroup sums, the sum at [groups]);
// *d_total = the length of the whole text.
int rc_snap_launch_piece_offsets(const uint64_t *d_part_first, uint64_t m, const uint32_t *d_records,
                                 uint64_t capacity, const uint64_t *d_group_off, const uint64_t *d_piece_pre,
                                 uint64_t *d_piece_off, uint64_t *d_total, hipStream_t st);
// The text of every part at its place in d_text, and no other byte.
int rc_snap_launch_encode_data(const uint32_t *d_records, const uint64_t *d_part_total, uint64_t capacity,
                               const uint64_t *d_group_off, const uint64_t *d_piece_pre, uint8_t *d_text,
                               hipStream_t st);
// The `count` packed pieces at their offsets in d_text.
int rc_snap_launch_place_pieces(const uint8_t *d_pieces, const uint64_t *d_piece_pre, const uint64_t *d_piece_off,
                                uint64_t count, uint8_t *d_text, hipStream_t st);

// snapshot_text.hip: the m + 1 fixed pieces of serialize(data), from columns.  One wave per piece:
// kSnapTextWaves pieces per workgroup; a path is read kSnapTextStep bytes per wave step.
constexpr uint32_t kSnapTextWaves = kSnapThreads / 64;
constexpr uint32_t kSnapTextStep = 64;
constexpr uint32_t kSnapMetaColumns = RC_SNAPSHOT_METADATA_COLUMNS;
constexpr uint32_t kSnapMetaFixed = 88;  // {"st_mode":,"st_uid":, ... "st_ctime_ns":} without the seven numbers

// What one byte of a path's generalised UTF-8 adds to the length of its JSON string
// (encode_basestring_ascii): the byte alone decides.
__host__ __device__ inline uint32_t rc_snap_path_term(uint32_t b) {
    if (b >= 0xF0u) return 12;  // a surrogate pair
    if (b >= 0xC0u) return 6;   // \uxxxx
    if (b >= 0x80u) return 0;   // a continuation byte: its lead byte's
    if (b == '"' || b == '\\') return 2;
    if (b >= 0x20u) return b == 0x7Fu ? 6 : 1;
    return b == '\b' || b == '\t' || b == '\n' || b == '\f' || b == '\r' ? 2 : 6;
}

// The characters of v as a signed decimal: 1 to 20.
__host__ __device__ inline uint32_t rc_snap_int64_len(int64_t v) {
    const uint64_t u = v < 0 ? uint64_t(0) - uint64_t(v) : uint64_t(v);
    uint32_t nd = 1;
    for (uint64_t p = 10; nd < 20 && u >= p; p *= 10) ++nd;  // 10^19 < 2^64: p does not wrap while nd < 20
    return nd + (v < 0 ? 1u : 0u);
}

// The columns both passes read (include/replicat_snapshot.h, "Writing the files' text").
struct SnapFileText {
    uint64_t m;
    const uint32_t *order;
    const uint8_t *path_bytes;
    const uint64_t *path_off;
    uint32_t digest_bytes;
    const uint8_t *digests;
    const uint8_t *unfinished;  // or null
    const int64_t *metadata;    // or null: no metadata key
    uint64_t first_len, last_len;
};

// d_piece_len[j], j <= m: the bytes of fixed piece j.
int rc_snap_launch_file_text_len(const SnapFileText &a, uint64_t *d_piece_len, hipStream_t st);
// Piece j at d_text + d_piece_off[j], and no other byte.
int rc_snap_launch_file_text(const SnapFileText &a, const uint8_t *d_first, const uint8_t *d_last,
                             const uint64_t *d_piece_off, uint8_t *d_text, hipStream_t st);

// snapshot_parse.hip: the parts read back from the text of `data`.  A part is then
// RC_SNAPSHOT_PART_WORDS words: run (the ordinal of its list among the lists of the call), start,
// end, index, counter, the offset of its text in its snapshot's text (two words, low first), flags.
constexpr uint32_t kSnapPartMinLen = 38;  // four numbers of one digit, with the separator
constexpr uint32_t kSnapPartFirst = RC_PART_FIRST, kSnapPartLast = RC_PART_LAST;
constexpr uint32_t kSnapFindSpan = kSnapThreads * 16;  // bytes of global memory per workgroup of the find kernels

// One text of a call: len bytes at ptr (any alignment); its stripped text goes `out` bytes into the
// packed output.
struct SnapParseText {
    uint64_t ptr, len, out, room;
};
static_assert(sizeof(SnapParseText) == RC_SNAPSHOT_TEXT_DESC_BYTES, "the descriptor the stages share");

inline uint64_t rc_snap_parts_room(uint64_t text_len) { return text_len / kSnapPartMinLen + 1; }
// Workgroups of 256 over 0 .. capacity (one more than the items: the sum's own place).
inline uint64_t rc_snap_parse_groups(uint64_t capacity) { return (capacity + 1 + kSnapThreads - 1) / kSnapThreads; }

// The two passes of the find stage over the d_blocks workgroups (SnapBlock: the block-th run of 256
// aligned granules of text `item`): scatter false writes the two counts of every workgroup; scatter
// true reads their exclusive prefixes (the sums at [n_blocks]) and writes words 0, 5, 6 and 7 of
// every part's record, d_text_first / d_text_run_first [0 .. n_texts] and the end of the last run
// in d_run_part_first.  No record at or behind `capacity` is written.
int rc_snap_launch_find(bool scatter, const SnapParseText *d_texts, uint64_t n_texts, const SnapBlock *d_blocks,
                        uint64_t n_blocks, uint64_t *d_part_counts, uint64_t *d_first_counts, uint64_t capacity,
                        uint32_t *d_records, uint64_t *d_text_first, uint64_t *d_text_run_first,
                        uint64_t *d_run_part_first, hipStream_t st);
// Words 1 to 4 and the last-flag of every record, the three arrays of every run, and
// RC_PARTS_NOT_CANONICAL into d_status[i] (RC_PARTS_OK beforehand) of every text with a part that
// is not what serialize writes.
int rc_snap_launch_parse(const SnapParseText *d_texts, uint64_t n_texts, const uint64_t *d_text_first,
                         const uint64_t *d_text_run_first, uint64_t capacity, uint32_t *d_records, uint64_t *d_run_off,
                         uint64_t *d_run_end, uint64_t *d_run_part_first, uint8_t *d_status, hipStream_t st);
// d_excl[k], k <= parts: the summed sizes of the parts before the k-th (in d_order, when given) in
// its workgroup of 256; d_sums[b]: the summed sizes of workgroup b, for all rc_snap_parse_groups.
int rc_snap_launch_size_sums(const uint32_t *d_records, const uint64_t *d_order, const uint64_t *d_part_total,
                             uint64_t capacity, uint64_t *d_sums, uint64_t *d_excl, hipStream_t st);
// With d_group_off the exclusive prefix of d_sums: positions, run and text sums; without d_order
// also d_run_sorted[r] = 0 (1 beforehand) where a run's counters do not increase strictly.
int rc_snap_launch_positions(const uint32_t *d_records, const uint64_t *d_order, const uint64_t *d_text_first,
                             const uint64_t *d_text_run_first, uint64_t n_texts, uint64_t capacity,
                             const uint64_t *d_run_part_first, const uint64_t *d_excl, const uint64_t *d_group_off,
                             uint64_t *d_position, uint64_t *d_run_count, uint64_t *d_run_size, uint8_t *d_run_sorted,
                             uint64_t *d_text_size, hipStream_t st);
// The bytes of every run as the two levels of a prefix: d_local[r], r <= capacity, and d_sums[b].
int rc_snap_launch_run_len(const uint64_t *d_run_off, const uint64_t *d_run_end, const uint64_t *d_run_total,
                           uint64_t capacity, uint64_t *d_local, uint64_t *d_sums, hipStream_t st);
// The fixed pieces of every text whose status is RC_PARTS_OK at its place in d_out, d_run_close[r]
// and d_stripped_len[i] (0 beforehand).
int rc_snap_launch_strip(const SnapParseText *d_texts, uint64_t n_texts, const uint64_t *d_text_run_first,
                         uint64_t capacity, const uint64_t *d_run_off, const uint64_t *d_run_end,
                         const uint64_t *d_run_local, const uint64_t *d_run_group_off, const uint8_t *d_status,
                         uint8_t *d_out, uint64_t *d_run_close, uint64_t *d_stripped_len, hipStream_t st);

// snapshot_fields.hip: the files' text read back from the stripped texts stage 4 leaves
// (include/replicat_snapshot.h, "Reading the files' text").  One wave per piece, kSnapTextWaves
// pieces per workgroup, Q kSnapTextStep bytes per wave step -- snapshot_text.hip's shape.
constexpr uint32_t kSnapFirstMost = 4096;  // a `first` longer than this is left to the host
constexpr uint32_t kSnapQBad = 0xFFu;

// One escape of Q as the device and rc_snapshot_path_bytes_for judge it.  a[k], k = 1 .. 11, is
// the byte k behind the backslash (anything where Q has ended) and `left` the bytes of Q from the
// backslash on.  bytes: what it decodes to in UTF-8 ('surrogatepass'), or kSnapQBad for an escape
// encode_basestring_ascii does not write; taken: its text, 2, 6 or -- a high surrogate with a low
// one directly behind it, which json.loads joins -- 12; code: the code point.
struct SnapQEscape {
    uint32_t bytes, taken, code;
};

__host__ __device__ inline uint32_t rc_snap_hex4(const uint32_t *a, bool &bad) {
    uint32_t v = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t c = a[k];
        uint32_t d = 0;
        if (c - '0' < 10u)
            d = c - '0';
        else if (c - 'a' < 6u)  // lowercase only
            d = c - 'a' + 10;
        else
            bad = true;
        v = (v << 4) | d;
    }
    return v;
}

__host__ __device__ inline SnapQEscape rc_snap_q_escape(const uint32_t *a, uint64_t left) {
    const SnapQEscape refused{kSnapQBad, 2, 0};
    if (left < 2) return refused;  // a dangling backslash
    const uint32_t c = a[1];
    const uint32_t brief = c == '"' || c == '\\' ? c : c == 'b' ? 8u : c == 'f' ? 12u : c == 'n' ? 10u : c == 'r' ? 13u
                                                                                                   : c == 't' ? 9u : 0u;
    if (brief) return SnapQEscape{1, 2, brief};
    if (c != 'u' || left < 6) return refused;
    bool bad = false;
    const uint32_t u = rc_snap_hex4(a + 2, bad);
    const bool has_brief = u == 8 || u == 9 || u == 10 || u == 12 || u == 13;
    if (bad || !((u < 0x20u && !has_brief) || u == 0x7Fu || u >= 0x80u)) return refused;
    if (u >= 0xD800u && u < 0xDC00u && left >= 12 && a[6] == '\\' && a[7] == 'u') {
        bool bad_low = false;  // such a low half is refused where it stands
        const uint32_t low = rc_snap_hex4(a + 8, bad_low);
        if (!bad_low && low >= 0xDC00u && low < 0xE000u)
            return SnapQEscape{4, 12, 0x10000u + ((u - 0xD800u) << 10) + (low - 0xDC00u)};
    }
    return SnapQEscape{u < 0x80u ? 1u : u < 0x800u ? 2u : 3u, 6, u};
}

// Byte k of the UTF-8 of `code` in `bytes` bytes.
__host__ __device__ inline uint32_t rc_snap_utf8_byte(uint32_t code, uint32_t bytes, uint32_t k) {
    if (bytes == 1) return code;
    const uint32_t shift = 6 * (bytes - 1 - k);
    if (k) return 0x80u | ((code >> shift) & 0x3Fu);
    return ((0xF00u >> bytes) & 0xFFu) | (code >> shift);  // 110xxxxx, 1110xxxx, 11110xxx
}

// What the two passes read: the texts of a call as stage 4 left them.
struct SnapFiles {
    const SnapParseText *texts;
    uint64_t n_texts, runs;
    const uint64_t *text_run_first, *run_close, *stripped_len;
    const uint8_t *out;
};

// The fields pass: per text d_file_status (RC_FILES_OK beforehand), d_has_metadata, d_first_len,
// d_last_off; per file the 64-byte slot, the flag, the metadata row, where Q starts in its text
// (d_path_text) and the bytes it decodes to (d_path_len, 0 beforehand).
int rc_snap_launch_file_fields(const SnapFiles &a, const uint8_t *d_status, uint32_t digest_bytes,
                               uint8_t *d_file_status, uint8_t *d_has_metadata, uint64_t *d_first_len,
                               uint64_t *d_last_off, uint8_t *d_digests, uint8_t *d_unfinished, int64_t *d_metadata,
                               uint64_t *d_path_text, uint64_t *d_path_len, hipStream_t st);
// The path pass: Q of every file of a text whose file status is RC_FILES_OK, decoded to
// d_path_bytes + d_path_off[f]; no byte at or behind path_room.
int rc_snap_launch_file_paths(const SnapFiles &a, const uint8_t *d_file_status, const uint64_t *d_path_text,
                              const uint64_t *d_path_off, uint8_t *d_path_bytes, uint64_t path_room, hipStream_t st);
