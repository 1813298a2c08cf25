// restore.hip -- the device stage of the restore path that is its own (include/replicat_restore.h):
// the per-chunk verdict of `_download_chunk` (replicat/repository.py:1696-1739) and the wipe of
// every plaintext that did not pass it.
//
// The heavy work is done before this kernel runs, by kernels that exist for the snapshot path:
// the subkeys (rc_b2_update_kernel over the shared KDF state), the decryption with its tag
// verdicts ok[] (gcm.hip / chacha.hip) and the digests of the plaintexts (blake2b.hip, sha2.hip,
// sha3.hip).  What is left per chunk is a comparison of at most 64 bytes and, for a chunk that
// failed, zeros over its plaintext buffer: plaintext that did not authenticate, or that is not the
// chunk the snapshot recorded, must not reach the host.
//
// One wave per chunk, four chunks per workgroup, no barrier and no LDS.  Lane j compares byte j
// of the two digest slots and a ballot joins them.  The wipe is the wave's: byte stores up to
// the first 16-byte boundary, 16-byte vector stores over the body (64 lanes x 16 bytes = 1 KiB per
// step, each lane's store aligned), byte stores over the last < 16 bytes.  It touches exactly
// [ptr, ptr + len): neighbours may sit back to back at any alignment.  A failed chunk is the rare
// case, so one wave per buffer is enough: ~1 KiB per store step, a 5 MB chunk in ~5000 steps.
#include <hip/hip_runtime.h>

#include "capi_internal.h"
#include "restore_kernels.h"

namespace {

// global address space: the stores become global_store_* (a plain pointer made from an integer
// is a flat one)
#define GLOBAL __attribute__((address_space(1)))
typedef GLOBAL uint8_t *gbytes;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kWave = 64;
constexpr uint64_t kSlot = RC_DIGEST_SLOT;

static_assert(kSlot == kWave, "lane j compares byte j of a digest slot");

__device__ __forceinline__ void wipe(gbytes p, uint64_t len, int lane) {
    const uint64_t to_boundary = (16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15;
    const uint64_t head = to_boundary < len ? to_boundary : len;  // < 16
    if (uint64_t(lane) < head) p[lane] = 0;
    const uint64_t body = (len - head) >> 4;  // whole 16-byte blocks from the boundary
    GLOBAL u32x4 *v = reinterpret_cast<GLOBAL u32x4 *>(p + head);
    for (uint64_t k = lane; k < body; k += kWave) v[k] = u32x4{0u, 0u, 0u, 0u};
    const uint64_t done = head + (body << 4), tail = len - done;  // tail < 16
    if (uint64_t(lane) < tail) p[done + lane] = 0;
}

}  // namespace

__global__ __launch_bounds__(kRestoreThreads) void rc_restore_verdict_kernel(RestoreVerdictArgs a) {
    const int lane = threadIdx.x & (kWave - 1);
    const uint64_t i = uint64_t(blockIdx.x) * (kRestoreThreads / kWave) + (threadIdx.x / kWave);
    if (i >= a.n) return;  // wave-uniform
    bool differs = false;
    if (uint32_t(lane) < a.digest_size)
        differs = a.computed[kSlot * i + lane] != a.expected[kSlot * i + lane];
    const bool corrupt = __ballot(differs) != 0ull;
    const bool bad_tag = a.ok && a.ok[i] == 0;
    const uint8_t status = bad_tag ? RC_CHUNK_BAD_TAG : corrupt ? RC_CHUNK_CORRUPT : RC_CHUNK_OK;
    if (lane == 0) a.status[i] = status;
    if (status != RC_CHUNK_OK && a.plain) {
        const RestorePlain b = a.plain[i];
        if (b.len) wipe(reinterpret_cast<gbytes>(b.ptr), b.len, lane);
    }
}

int rc_restore_launch_verdict(const RestoreVerdictArgs &a, hipStream_t stream) {
    if (!a.n) return 0;
    const uint64_t per = kRestoreThreads / kWave;
    const uint64_t groups = (a.n + per - 1) / per;
    if (groups > 0x7FFFFFFFull) return rc_fail(RC_ERR_HIP, "%llu chunks in one call", (unsigned long long)a.n);
    rc_restore_verdict_kernel<<<static_cast<unsigned>(groups), kRestoreThreads, 0, stream>>>(a);
    return rc::launch_status("rc_restore_verdict_kernel");
}
