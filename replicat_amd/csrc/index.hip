// index.hip -- the kernels of the chunk-name index (include/replicat_index.h), gfx950.
//
// Pool: 64-byte name slots indexed by id, zero past name_bytes, so names compare as 8-byte words.
// Table: open addressing over uint64 ids, linear probing from the name's first 8 bytes.
//
// All DATA visibility comes from kernel boundaries: a name is in the pool before the launch that
// inserts its id (rc_index_stage_kernel, or the host's upload), and the ids have settled before
// the launch that looks them up.  Within the insert launch lanes communicate through the atomic
// on the table word alone: an entry goes from empty to an id once and afterwards only to smaller
// ids OF THE SAME NAME, so whichever id a lane reads there, the pooled name it compares against
// was written before the launch.  Every probe loop is bounded by the table size.
#include <hip/hip_runtime.h>

#include "capi_internal.h"
#include "index_kernels.h"
#include "index_lookup.h"

namespace {

__device__ __forceinline__ const uint64_t *name_of(const IndexView &v, uint64_t id) {
    return reinterpret_cast<const uint64_t *>(v.pool + kIndexSlot * id);
}

__device__ __forceinline__ bool same_name(const uint64_t *a, const uint64_t *b, uint32_t words) {
    uint64_t diff = 0;
    for (uint32_t w = 0; w < words; ++w) diff |= a[w] ^ b[w];
    return diff == 0;
}

// The stream of cut slot s (the last i with cut_base[i] <= s) and whether s holds a chunk.
__device__ __forceinline__ bool lane_has_name(const IndexWork &w, uint64_t s) {
    if (s >= w.slots) return false;
    if (!w.cut_base) return true;
    uint64_t lo = 0, hi = w.n;  // cut_base[lo] <= s < cut_base[hi]
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) / 2;
        if (w.cut_base[mid] <= s)
            lo = mid;
        else
            hi = mid;
    }
    const int64_t cnt = w.counts[lo];
    return cnt > 0 && s - w.cut_base[lo] < uint64_t(cnt);
}

// Insert id (its name pooled before the launch): claim the first empty entry of the name's probe
// sequence, or lower the entry that already holds the name.  The smallest id of a name wins
// whatever the arrival order.
__device__ __forceinline__ void insert_id(const IndexView &v, uint64_t id) {
    const uint64_t *mine = name_of(v, id);
    const uint32_t words = (v.name_bytes + 7) / 8;
    uint64_t pos = mine[0] & v.mask;
    for (uint64_t probe = 0; probe <= v.mask; ++probe, pos = (pos + 1) & v.mask) {
        unsigned long long *entry = reinterpret_cast<unsigned long long *>(v.table + pos);
        const uint64_t cur = atomicCAS(entry, (unsigned long long)kIndexEmpty, (unsigned long long)id);
        if (cur == kIndexEmpty) return;
        if (cur == id || same_name(mine, name_of(v, cur), words)) {
            atomicMin(entry, (unsigned long long)id);
            return;
        }
    }
    // probe bound exhausted (a full table): the lookup reports it as owner -1
}

}  // namespace

__global__ __launch_bounds__(kIndexThreads) void rc_index_stage_kernel(IndexView v, IndexWork w,
                                                                       const uint8_t *names) {
    const uint64_t s = uint64_t(blockIdx.x) * kIndexThreads + threadIdx.x;
    if (!lane_has_name(w, s)) return;
    const uint64_t *src = reinterpret_cast<const uint64_t *>(names + kIndexSlot * s);
    uint64_t *dst = reinterpret_cast<uint64_t *>(v.pool + kIndexSlot * (w.id_base + s));
#pragma unroll
    for (uint32_t i = 0; i < kIndexSlot / 8; ++i) {
        const uint32_t lo = 8 * i;
        uint64_t x = 0;
        if (lo < v.name_bytes) {
            x = src[i];
            const uint32_t keep = v.name_bytes - lo;
            if (keep < 8) x &= (uint64_t(1) << (8 * keep)) - 1;
        }
        dst[i] = x;
    }
}

__global__ __launch_bounds__(kIndexThreads) void rc_index_insert_kernel(IndexView v, IndexWork w) {
    const uint64_t s = uint64_t(blockIdx.x) * kIndexThreads + threadIdx.x;
    if (!lane_has_name(w, s)) return;
    insert_id(v, w.id_base + s);
}

__global__ __launch_bounds__(kIndexThreads) void rc_index_resolve_kernel(IndexView v, IndexWork w,
                                                                         int64_t *owner, uint8_t *fresh) {
    const uint64_t s = uint64_t(blockIdx.x) * kIndexThreads + threadIdx.x;
    if (!lane_has_name(w, s)) return;
    const uint64_t id = w.id_base + s;
    const uint64_t *mine = name_of(v, id);
    const uint32_t words = (v.name_bytes + 7) / 8;
    int64_t found = -1;
    uint64_t pos = mine[0] & v.mask;
    for (uint64_t probe = 0; probe <= v.mask; ++probe, pos = (pos + 1) & v.mask) {
        const uint64_t cur = v.table[pos];
        if (cur == kIndexEmpty) break;  // the name was never inserted: a full table
        if (cur == id || same_name(mine, name_of(v, cur), words)) {
            found = int64_t(cur);
            break;
        }
    }
    owner[s] = found;
    fresh[s] = found == int64_t(id) ? 1 : 0;
}

// The id already in the index for each of n caller names (64-byte slots), kIndexAbsent or
// kIndexExhausted.  Nothing is pooled or inserted; reaching an empty entry is the normal answer
// for a name nobody holds, which is why it is told apart from an exhausted probe bound here.
__global__ __launch_bounds__(kIndexThreads) void rc_index_lookup_kernel(IndexView v, uint64_t n,
                                                                        const uint8_t *names,
                                                                        int64_t *owner) {
    const uint64_t i = uint64_t(blockIdx.x) * kIndexThreads + threadIdx.x;
    if (i >= n) return;
    uint64_t mine[8];
    load_name(names + kIndexSlot * i, v.name_bytes, mine);
    owner[i] = lookup_name(v, mine);
}

__global__ __launch_bounds__(kIndexThreads) void rc_index_reinsert_kernel(IndexView v,
                                                                          const uint64_t *old_table,
                                                                          uint64_t old_entries) {
    const uint64_t e = uint64_t(blockIdx.x) * kIndexThreads + threadIdx.x;
    if (e >= old_entries) return;
    const uint64_t id = old_table[e];
    if (id != kIndexEmpty) insert_id(v, id);
}

namespace {
unsigned groups_for(uint64_t lanes) { return static_cast<unsigned>((lanes + kIndexThreads - 1) / kIndexThreads); }
}  // namespace

int rc_index_launch_stage(const IndexView &v, const IndexWork &w, const uint8_t *names, hipStream_t st) {
    if (!w.slots) return 0;
    rc_index_stage_kernel<<<groups_for(w.slots), kIndexThreads, 0, st>>>(v, w, names);
    return rc::launch_status("rc_index_stage_kernel");
}

int rc_index_launch_insert(const IndexView &v, const IndexWork &w, hipStream_t st) {
    if (!w.slots) return 0;
    rc_index_insert_kernel<<<groups_for(w.slots), kIndexThreads, 0, st>>>(v, w);
    return rc::launch_status("rc_index_insert_kernel");
}

int rc_index_launch_resolve(const IndexView &v, const IndexWork &w, int64_t *owner, uint8_t *fresh,
                            hipStream_t st) {
    if (!w.slots) return 0;
    rc_index_resolve_kernel<<<groups_for(w.slots), kIndexThreads, 0, st>>>(v, w, owner, fresh);
    return rc::launch_status("rc_index_resolve_kernel");
}

int rc_index_launch_lookup(const IndexView &v, uint64_t n, const uint8_t *names, int64_t *owner,
                           hipStream_t st) {
    if (!n) return 0;
    rc_index_lookup_kernel<<<groups_for(n), kIndexThreads, 0, st>>>(v, n, names, owner);
    return rc::launch_status("rc_index_lookup_kernel");
}

int rc_index_launch_reinsert(const IndexView &v, const uint64_t *old_table, uint64_t old_entries,
                             hipStream_t st) {
    if (!old_entries) return 0;
    rc_index_reinsert_kernel<<<groups_for(old_entries), kIndexThreads, 0, st>>>(v, old_table, old_entries);
    return rc::launch_status("rc_index_reinsert_kernel");
}
