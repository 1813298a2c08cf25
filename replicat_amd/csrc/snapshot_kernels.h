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
inline uint32_t rc_snap_chars(uint32_t digest_bytes) { return 4 * ((digest_bytes + 2) / 3); }
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
