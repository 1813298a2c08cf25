// snapshot.hip -- the device stages of snapshot loading that are its own
// (include/replicat_snapshot.h): the chunk table of a snapshot body, and the base64 fields of an
// encrypted snapshot file, turned into bytes.
//
// serialize (replicat/repository.py:434-438, utils/__init__.py:166-172) writes a table of n digests
// of L bytes as   [{"!b":"<C characters>"},{"!b":"<C characters>"}, ... ]   with C = 4 ceil(L / 3):
// after the '[' every record, with the ',' or ']' behind it, takes stride = C + 10 bytes.  So the
// table is a record array and record j belongs to one lane: no parser.  A lane accepts exactly
// what serialize writes (json.loads and base64 accept more; whatever a lane refuses takes the
// reference's code on the host, replicat_amd/snapshots.py), and what it accepts decodes to what
// base64.standard_b64decode returns.
//
// Both kernels stage a workgroup's contiguous span of text through LDS: whole aligned 16-byte
// granules of global memory, each holding at least one byte of the span (so no load leaves the
// pages of the buffer), land at the same offset modulo 16 in LDS, and a lane assembles its
// unaligned words there from aligned LDS words (a record starts at any byte: stride 98 for L = 64).
// Characters decode by range tests, no table.
//
//   tables  one record per lane, 256 records per workgroup (25 KB of text for L = 64); the 64-byte
//           slot of a digest is written as four 16-byte stores.  Must read stride and write 64
//           bytes per digest, nothing else.
//   bulk    16 characters -> 12 bytes per lane; the bytes are laid out in LDS at the destination's
//           offset modulo 16, so that all but the first and last granule of a workgroup's output
//           are aligned 16-byte stores whatever the destination's alignment.
//
// A lane that finds a violation issues one atomic on the word that holds its item's verdict byte
// (OR of 0 / AND of all-ones into the neighbouring bytes: they keep their values); the good path
// has none.  The wipe of a table whose tag failed is restore.hip's verdict kernel, unchanged.
#include <hip/hip_runtime.h>

#include "snapshot_device.h"

namespace {

constexpr uint32_t kTableSpan = kSnapThreads * kSnapMaxStride;       // text of one workgroup
constexpr uint32_t kTableLds = (kTableSpan + 15 + 8 + 15) / 16 * 16;  // + skew + a lane's look-ahead
constexpr uint32_t kBulkSpan = kSnapThreads * kSnapLaneChars;
constexpr uint32_t kBulkLds = kBulkSpan + 32;
constexpr uint32_t kBulkOut = kSnapThreads * kSnapLaneBytes;
constexpr uint32_t kBulkOutLds = kBulkOut + 16;

// One atomic that makes the verdict byte at p `value` when the byte can only move one way:
// set_bits ORs value in, otherwise the byte is cleared.
__device__ __forceinline__ void flag_byte(uint8_t *p, uint32_t value, bool set_bits) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    unsigned int *word = reinterpret_cast<unsigned int *>(a & ~uintptr_t(3));
    const uint32_t shift = 8 * uint32_t(a & 3);
    if (set_bits)
        atomicOr(word, value << shift);
    else
        atomicAnd(word, ~(0xFFu << shift));
}

}  // namespace

__global__ __launch_bounds__(kSnapThreads) void rc_snap_tables_kernel(const SnapTable *tables,
                                                                       const SnapBlock *blocks,
                                                                       uint32_t digest_bytes, uint8_t *slots,
                                                                       uint8_t *status) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[kTableLds];
    const SnapBlock b = blocks[blockIdx.x];
    if (status[b.item] == RC_TABLE_BAD_TAG) return;  // workgroup-uniform: its plaintext is wiped
    const SnapTable t = tables[b.item];
    gcbytes text = reinterpret_cast<gcbytes>(t.ptr);
    if (t.count == kSnapReject || t.count == 0) {  // no record: one lane decides
        if (threadIdx.x == 0) {
            const bool empty = t.count == 0 && t.len == 2 && text[0] == '[' && text[1] == ']';
            if (!empty) flag_byte(status + b.item, RC_TABLE_NOT_CANONICAL, true);
        }
        return;
    }
    const uint32_t groups = (digest_bytes + 2) / 3;  // of four characters
    const uint32_t pad = (3 - digest_bytes % 3) % 3;
    const uint32_t stride = 4 * groups + 10;
    const uint64_t rec0 = uint64_t(b.block) * kSnapThreads;
    const uint64_t left = t.count - rec0;
    const uint32_t nrec = left < uint64_t(kSnapThreads) ? uint32_t(left) : uint32_t(kSnapThreads);
    const uint32_t skew = stage_span(lds, text + 1 + rec0 * stride, nrec * stride);
    bool bad = b.block == 0 && threadIdx.x == 0 && text[0] != '[';
    __syncthreads();
    if (threadIdx.x < nrec) {
        const uint64_t j = rec0 + threadIdx.x;
        const uint32_t off = skew + threadIdx.x * stride;
        const uint32_t *words = reinterpret_cast<const uint32_t *>(lds) + (off >> 2);
        const uint32_t sh = 8 * (off & 3);
        // w_cur walks the record's own words (word k = its bytes 4k .. 4k + 3)
        uint32_t a_prev = words[0], a_cur = words[1];
        uint32_t w_prev = __funnelshift_r(a_prev, a_cur, sh);
        bad |= w_prev != 0x6221227Bu;  // {"!b
        a_prev = a_cur;
        a_cur = words[2];
        uint32_t w_cur = __funnelshift_r(a_prev, a_cur, sh);
        bad |= (w_cur & 0xFFFFFFu) != 0x223A22u;  // ":"
        uint32_t out[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) out[k] = 0;
        const uint32_t sep = j == t.count - 1 ? uint32_t(']') : uint32_t(',');
        // group g: the record's bytes 7 + 4g .. 10 + 4g; after the last one, "} and the separator
#pragma unroll
        for (uint32_t g = 0; g <= 22; ++g) {
            if (g <= groups) {  // wave-uniform
                w_prev = w_cur;
                a_prev = a_cur;
                a_cur = words[g + 3];
                w_cur = __funnelshift_r(a_prev, a_cur, sh);
                const uint32_t chars = (w_prev >> 24) | (w_cur << 8);
                if (g < groups) {
                    const uint32_t v = b64_group(chars, g == groups - 1 ? pad : 0, bad);
#pragma unroll
                    for (uint32_t k = 0; k < 3; ++k) {
                        const uint32_t at = 3 * g + k;  // compile-time after unrolling
                        if (at < 64) out[at >> 2] |= ((v >> (16 - 8 * k)) & 255u) << (8 * (at & 3));
                    }
                } else {
                    bad |= (chars & 0xFFFFFFu) != (0x7D22u | (sep << 16));
                }
            }
        }
        GLOBAL u32x4 *slot = reinterpret_cast<GLOBAL u32x4 *>(reinterpret_cast<uintptr_t>(slots) +
                                                              RC_DIGEST_SLOT * (t.first + j));
#pragma unroll
        for (int q = 0; q < 4; ++q) slot[q] = u32x4{out[4 * q], out[4 * q + 1], out[4 * q + 2], out[4 * q + 3]};
    }
    if (bad) flag_byte(status + b.item, RC_TABLE_NOT_CANONICAL, true);
}

__global__ __launch_bounds__(kSnapThreads) void rc_snap_b64_kernel(const SnapText *texts, const SnapBlock *blocks,
                                                                    uint8_t *ok) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[kBulkLds];
    __shared__ __attribute__((aligned(16))) uint8_t lds_out[kBulkOutLds];
    const SnapBlock b = blocks[blockIdx.x];
    const SnapText t = texts[b.item];
    if (t.len == kSnapReject) {
        if (threadIdx.x == 0) flag_byte(ok + b.item, 0, false);
        return;
    }
    if (t.len == 0) return;
    gcbytes text = reinterpret_cast<gcbytes>(t.ptr);
    const uint32_t pad = (text[t.len - 1] == '=' ? 1u : 0u) + (text[t.len - 2] == '=' ? 1u : 0u);
    const uint64_t out_len = t.len / 4 * 3 - pad;
    const uint64_t char0 = uint64_t(b.block) * kBulkSpan;
    const uint64_t left = t.len - char0;
    const uint32_t nchar = left < uint64_t(kBulkSpan) ? uint32_t(left) : kBulkSpan;  // a multiple of 4
    const uint32_t skew = stage_span(lds, text + char0, nchar);
    gbytes dst = reinterpret_cast<gbytes>(t.out) + uint64_t(b.block) * kBulkOut;
    const uint32_t dskew = uint32_t(reinterpret_cast<uintptr_t>(dst) & 15);
    __syncthreads();
    bool bad = false;
    const uint32_t mine = threadIdx.x * kSnapLaneChars;
    if (mine < nchar) {
        const uint32_t off = skew + mine;
        const uint32_t *words = reinterpret_cast<const uint32_t *>(lds) + (off >> 2);
        const uint32_t sh = 8 * (off & 3);
        uint32_t a_prev = words[0];
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            if (mine + 4 * k < nchar) {
                const uint32_t a_cur = words[k + 1];
                const uint32_t chars = __funnelshift_r(a_prev, a_cur, sh);
                a_prev = a_cur;
                const bool last = char0 + mine + 4 * k + 4 == t.len;
                const uint32_t v = b64_group(chars, last ? pad : 0, bad);
                uint8_t *o = lds_out + dskew + threadIdx.x * kSnapLaneBytes + 3 * k;
                o[0] = uint8_t(v >> 16);
                o[1] = uint8_t(v >> 8);
                o[2] = uint8_t(v);
            }
        }
    }
    if (bad) flag_byte(ok + b.item, 0, false);
    __syncthreads();
    // lds_out[q] belongs at dst - dskew + q, for q in [dskew, end)
    const uint64_t out0 = uint64_t(b.block) * kBulkOut;
    const uint64_t out_left = out_len > out0 ? out_len - out0 : 0;
    const uint32_t nbytes = out_left < uint64_t(kBulkOut) ? uint32_t(out_left) : kBulkOut;
    const uint32_t end = dskew + nbytes;
    gbytes base = dst - dskew;
    for (uint32_t q = threadIdx.x * 16; q < end; q += kSnapThreads * 16) {
        if (q >= dskew && q + 16 <= end) {
            *reinterpret_cast<GLOBAL u32x4 *>(base + q) = *reinterpret_cast<const u32x4 *>(lds_out + q);
        } else {
            for (uint32_t k = q; k < q + 16; ++k)
                if (k >= dskew && k < end) base[k] = lds_out[k];
        }
    }
}

int rc_snap_launch_tables(const SnapTable *d_tables, const SnapBlock *d_blocks, uint64_t n_blocks,
                          uint32_t digest_bytes, uint8_t *d_slots, uint8_t *d_status, hipStream_t stream) {
    unsigned grid;
    if (int rc = grid_of(n_blocks, 1, "records", grid)) return rc;
    if (!grid) return 0;
    rc_snap_tables_kernel<<<grid, kSnapThreads, 0, stream>>>(d_tables, d_blocks, digest_bytes, d_slots, d_status);
    return rc::launch_status("rc_snap_tables_kernel");
}

int rc_snap_launch_b64(const SnapText *d_texts, const SnapBlock *d_blocks, uint64_t n_blocks, uint8_t *d_ok,
                       hipStream_t stream) {
    unsigned grid;
    if (int rc = grid_of(n_blocks, 1, "text", grid)) return rc;
    if (!grid) return 0;
    rc_snap_b64_kernel<<<grid, kSnapThreads, 0, stream>>>(d_texts, d_blocks, d_ok);
    return rc::launch_status("rc_snap_b64_kernel");
}
