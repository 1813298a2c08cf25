// snapshot_write.hip -- the device stages of snapshot writing that are its own
// (include/replicat_snapshot.h): digests in 64-byte slots turned into the text of a chunk table,
// and bytes turned into base64.  The inverses of snapshot.hip's two kernels, with its conventions:
// kSnapThreads lanes, SnapBlock work lists in which every item has at least one block, characters
// by range arithmetic (no table).
//
// serialize (replicat/repository.py:434-438, utils/__init__.py:166-172) writes a table of n digests
// of L bytes as   [{"!b":"<C characters>"},{"!b":"<C characters>"}, ... ]   with C = 4 ceil(L / 3):
// after the '[' every record, with the ',' or ']' behind it, takes stride = C + 10 bytes, and the
// empty table is "[]".
//
// Both kernels build a workgroup's contiguous span of output in LDS at the destination's offset
// modulo 16 (a record starts at any byte: stride 98 for L = 64, and the text's base is arbitrary),
// each lane putting down its own bytes only -- whole LDS words inside its record, single bytes in
// the two words it shares with its neighbours.  The span then leaves as whole aligned 16-byte
// stores, except its first and last granule where they are partial: there only the span's own
// bytes are written, because the rest of such a granule is the neighbouring workgroup's, or
// whatever lies before or after the text (the tag of a blob, another text).
//
//   tables  one record per lane, 256 records per workgroup; a lane reads its 64-byte slot as four
//           16-byte loads and uses the first L bytes only.  Must read 64 and write stride bytes
//           per digest (+ the '['), nothing else.
//   bulk    12 bytes -> 16 characters per lane; the source span is staged through LDS as whole
//           aligned granules that hold at least one of its bytes (snapshot.hip's rule: no load
//           leaves the pages of the buffer).
#include <hip/hip_runtime.h>

#include "snapshot_device.h"

namespace {

constexpr uint32_t kRecordWords = (kSnapMaxStride + 3) / 4;                 // 25
constexpr uint32_t kMaxGroups = (kSnapMaxStride - 10) / 4;                   // 22 for L = 64
constexpr uint32_t kEncSpan = kSnapThreads * kSnapMaxStride + 1;             // records and the '['
constexpr uint32_t kEncLds = (kEncSpan + 15 + 15) / 16 * 16;                 // + the skew
constexpr uint32_t kBulkIn = kSnapThreads * kSnapLaneBytes;                  // source bytes of a workgroup
constexpr uint32_t kBulkInLds = kBulkIn + 32;                                // + skew + a lane's look-ahead
constexpr uint32_t kBulkChars = kSnapThreads * kSnapLaneChars;
constexpr uint32_t kBulkCharsLds = kBulkChars + 16;

// Puts the first `len` bytes of w (word k = bytes 4k .. 4k + 3; len <= 4 N) at lds + off, off any
// byte: aligned words where all four bytes are this record's, single bytes elsewhere, so that
// lanes with adjacent records never write each other's bytes.
template <int N>
__device__ __forceinline__ void lds_put(uint8_t *lds, uint32_t off, const uint32_t (&w)[N], uint32_t len) {
    const uint32_t a = off & 3u;
    uint8_t *base = lds + (off - a);
    uint32_t *words = reinterpret_cast<uint32_t *>(base);
#pragma unroll
    for (int m = 0; m <= N; ++m) {
        const int start = 4 * m - int(a);  // the record's byte in the word's low byte
        if (start < int(len)) {
            const uint32_t lo = m > 0 ? w[m > 0 ? m - 1 : 0] : 0u, hi = m < N ? w[m < N ? m : 0] : 0u;
            const uint32_t v = __funnelshift_l(lo, hi, 8 * a);
            if (start >= 0 && start + 4 <= int(len)) {
                words[m] = v;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (start + k >= 0 && start + k < int(len)) base[4 * m + k] = uint8_t(v >> (8 * k));
            }
        }
    }
}

// lds[q] belongs at base + q for q in [skew, end): whole 16-byte stores but for a partial first
// and last granule, of which only the bytes inside the range are written.
__device__ __forceinline__ void store_span(gbytes base, const uint8_t *lds, uint32_t skew, uint32_t end) {
    for (uint32_t q = threadIdx.x * 16; q < end; q += kSnapThreads * 16) {
        if (q >= skew && q + 16 <= end) {
            *reinterpret_cast<GLOBAL u32x4 *>(base + q) = *reinterpret_cast<const u32x4 *>(lds + q);
        } else {
            for (uint32_t k = q; k < q + 16; ++k)
                if (k >= skew && k < end) base[k] = lds[k];
        }
    }
}

}  // namespace

__global__ __launch_bounds__(kSnapThreads) void rc_snap_encode_tables_kernel(const SnapTable *tables,
                                                                              const SnapBlock *blocks,
                                                                              uint32_t digest_bytes,
                                                                              const uint8_t *slots) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[kEncLds];
    const SnapBlock b = blocks[blockIdx.x];
    const SnapTable t = tables[b.item];
    gbytes text = reinterpret_cast<gbytes>(t.ptr);
    if (t.count == 0) {  // "[]": no record
        if (threadIdx.x < 2) text[threadIdx.x] = threadIdx.x ? ']' : '[';
        return;
    }
    const uint32_t groups = (digest_bytes + 2) / 3;  // of four characters
    const uint32_t pad = (3 - digest_bytes % 3) % 3;
    const uint32_t stride = 4 * groups + 10;
    const uint64_t rec0 = uint64_t(b.block) * kSnapThreads;
    const uint64_t left = t.count - rec0;
    const uint32_t nrec = left < uint64_t(kSnapThreads) ? uint32_t(left) : uint32_t(kSnapThreads);
    // the span: this workgroup's records, and in front of the table's first one the '['
    const uint32_t lead = b.block == 0 ? 1u : 0u;
    gbytes dst = text + (1 - lead) + rec0 * stride;
    const uint32_t dskew = uint32_t(reinterpret_cast<uintptr_t>(dst) & 15);
    if (threadIdx.x < nrec) {
        const uint64_t j = rec0 + threadIdx.x;
        const GLOBAL u32x4 *slot = reinterpret_cast<const GLOBAL u32x4 *>(reinterpret_cast<uintptr_t>(slots) +
                                                                          RC_DIGEST_SLOT * (t.first + j));
        uint32_t d[16];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const u32x4 v = slot[q];
            d[4 * q] = v.x;
            d[4 * q + 1] = v.y;
            d[4 * q + 2] = v.z;
            d[4 * q + 3] = v.w;
        }
        const uint32_t sep = j == t.count - 1 ? uint32_t(']') : uint32_t(',');
        // word k of the record = its bytes 4k .. 4k + 3; group g is its bytes 7 + 4g .. 10 + 4g
        uint32_t w[kRecordWords];
#pragma unroll
        for (uint32_t k = 0; k < kRecordWords; ++k) w[k] = 0;
        w[0] = 0x6221227Bu;  // {"!b
        w[1] = 0x223A22u;    // ":"
#pragma unroll
        for (uint32_t g = 0; g <= kMaxGroups; ++g) {
            if (g < groups) {  // wave-uniform
                uint32_t v = 0;
#pragma unroll
                for (uint32_t k = 0; k < 3; ++k) {
                    const uint32_t at = 3 * g + k;  // compile-time after unrolling
                    uint32_t byte = 0;
                    if (at < 64) byte = (d[at >> 2] >> (8 * (at & 3))) & 255u;
                    if (at >= digest_bytes) byte = 0;  // the slot's tail takes no part
                    v = (v << 8) | byte;
                }
                const uint32_t chars = b64_quad(v, g == groups - 1 ? pad : 0u);
                w[g + 1] |= chars << 24;
                w[g + 2] = chars >> 8;
            } else if (g == groups) {
                w[g + 1] |= uint32_t('"') << 24;
                w[g + 2] = uint32_t('}') | (sep << 8);
            }
        }
        lds_put(lds, dskew + lead + threadIdx.x * stride, w, stride);
    }
    if (lead && threadIdx.x == 0) lds[dskew] = '[';
    __syncthreads();
    store_span(dst - dskew, lds, dskew, dskew + lead + nrec * stride);
}

__global__ __launch_bounds__(kSnapThreads) void rc_snap_b64_encode_kernel(const SnapText *texts,
                                                                           const SnapBlock *blocks) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[kBulkInLds];
    __shared__ __attribute__((aligned(16))) uint8_t lds_out[kBulkCharsLds];
    const SnapBlock b = blocks[blockIdx.x];
    const SnapText t = texts[b.item];
    if (t.len == 0) return;
    const uint64_t byte0 = uint64_t(b.block) * kBulkIn;
    const uint64_t left = t.len - byte0;
    const uint32_t nbytes = left < uint64_t(kBulkIn) ? uint32_t(left) : kBulkIn;
    const uint32_t skew = stage_span(lds, reinterpret_cast<gcbytes>(t.ptr) + byte0, nbytes);
    gbytes dst = reinterpret_cast<gbytes>(t.out) + uint64_t(b.block) * kBulkChars;
    const uint32_t dskew = uint32_t(reinterpret_cast<uintptr_t>(dst) & 15);
    __syncthreads();
    const uint32_t mine = threadIdx.x * kSnapLaneBytes;
    if (mine < nbytes) {
        const uint32_t off = skew + mine;
        const uint32_t *words = reinterpret_cast<const uint32_t *>(lds) + (off >> 2);
        const uint32_t sh = 8 * (off & 3);
        // in[k]: the lane's bytes 4k .. 4k + 3
        uint32_t in[3];
        uint32_t a_prev = words[0];
#pragma unroll
        for (uint32_t k = 0; k < 3; ++k) {
            const uint32_t a_cur = words[k + 1];
            in[k] = __funnelshift_r(a_prev, a_cur, sh);
            a_prev = a_cur;
        }
        const uint32_t have = nbytes - mine < kSnapLaneBytes ? nbytes - mine : kSnapLaneBytes;
        uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
        for (uint32_t g = 0; g < 4; ++g) {
            uint32_t v = 0;
#pragma unroll
            for (uint32_t k = 0; k < 3; ++k) {
                const uint32_t at = 3 * g + k;
                uint32_t byte = (in[at >> 2] >> (8 * (at & 3))) & 255u;
                if (at >= have) byte = 0;  // past the text: whatever the granule held
                v = (v << 8) | byte;
            }
            const uint32_t rest = have > 3 * g ? have - 3 * g : 0;  // 1 or 2: the text's leftover bytes
            w[g] = b64_quad(v, rest >= 3 ? 0u : 3 - rest);
        }
        lds_put(lds_out, dskew + threadIdx.x * kSnapLaneChars, w, 4 * ((have + 2) / 3));
    }
    __syncthreads();
    store_span(dst - dskew, lds_out, dskew, dskew + 4 * ((nbytes + 2) / 3));
}

int rc_snap_launch_encode_tables(const SnapTable *d_tables, const SnapBlock *d_blocks, uint64_t n_blocks,
                                 uint32_t digest_bytes, const uint8_t *d_slots, hipStream_t stream) {
    unsigned grid;
    if (int rc = grid_of(n_blocks, 1, "records", grid)) return rc;
    if (!grid) return 0;
    rc_snap_encode_tables_kernel<<<grid, kSnapThreads, 0, stream>>>(d_tables, d_blocks, digest_bytes, d_slots);
    return rc::launch_status("rc_snap_encode_tables_kernel");
}

int rc_snap_launch_b64_encode(const SnapText *d_texts, const SnapBlock *d_blocks, uint64_t n_blocks,
                              hipStream_t stream) {
    unsigned grid;
    if (int rc = grid_of(n_blocks, 1, "bytes", grid)) return rc;
    if (!grid) return 0;
    rc_snap_b64_encode_kernel<<<grid, kSnapThreads, 0, stream>>>(d_texts, d_blocks);
    return rc::launch_status("rc_snap_b64_encode_kernel");
}
