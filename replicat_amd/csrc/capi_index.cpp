// capi_index.cpp -- the host side of include/replicat_index.h: the pool and table of an rc_index,
// the id allocation and the staging of a call's cut-slot layout.  The kernels are index.hip's.
#include <hip/hip_runtime.h>

#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/replicat_index.h"
#include "capi_internal.h"
#include "index_kernels.h"

static_assert(RC_INDEX_SLOT == kIndexSlot, "one slot size for callers and kernels");

struct rc_index {
    int device = 0;
    uint32_t name_bytes = 0;
    uint64_t max_names = 0, used = 0, entries = 0;
    uint8_t *pool = nullptr;
    uint64_t *table = nullptr;
    std::mutex mu;
    // a call's cut_base list
    struct Staging {
        rc::PinnedBuf h_stage;
        rc::DevBuf d_stage;
    };
    rc::SlotRing<Staging> ring;
};

namespace {

uint64_t table_entries(uint64_t max_names) {
    uint64_t e = 16;
    while (e < 2 * max_names) e <<= 1;
    return e;
}

IndexView view_of(const rc_index *x) {
    return IndexView{x->pool, x->table, x->entries - 1, x->name_bytes};
}

// A pool of max_names slots and an empty table for them.
int allocate(uint64_t max_names, uint8_t **pool, uint64_t **table, uint64_t *entries) {
    *entries = table_entries(max_names);
    RC_HIP_TRY(hipMalloc(reinterpret_cast<void **>(pool), std::max<uint64_t>(max_names, 1) * kIndexSlot));
    if (hipMalloc(reinterpret_cast<void **>(table), *entries * sizeof(uint64_t)) != hipSuccess) {
        (void)hipFree(*pool);
        *pool = nullptr;
        return rc_fail(RC_ERR_HIP, "hipMalloc of %llu table entries failed", (unsigned long long)*entries);
    }
    RC_HIP_TRY(hipMemset(*table, 0xFF, *entries * sizeof(uint64_t)));
    return 0;
}

void destroy_tracked(void *p) { rc_index_destroy(static_cast<rc_index *>(p)); }

// Stage the work's names, insert them and resolve every slot's owner.
int resolve_work(const IndexView &v, const IndexWork &work, const uint8_t *d_names, int64_t *d_owner,
                 uint8_t *d_fresh, hipStream_t st) {
    if (int rc = rc_index_launch_stage(v, work, d_names, st)) return rc;
    if (int rc = rc_index_launch_insert(v, work, st)) return rc;
    return rc_index_launch_resolve(v, work, d_owner, d_fresh, st);
}

int check_room(const rc_index *x, uint64_t more) {
    if (more > x->max_names || x->used > x->max_names - more)
        return rc_fail(RC_ERR_INDEX_FULL, "index full: %llu ids used, %llu more exceed max_names %llu",
                       (unsigned long long)x->used, (unsigned long long)more,
                       (unsigned long long)x->max_names);
    return 0;
}

}  // namespace

extern "C" {

int rc_index_create(uint32_t name_bytes, uint64_t max_names, int device, rc_index **out) {
    if (!out) return rc_fail(RC_ERR_ARGUMENT, "null output handle");
    *out = nullptr;
    if (name_bytes < 1 || name_bytes > kIndexSlot)
        return rc_fail(RC_ERR_ARGUMENT, "name_bytes must be 1..64, not %u", name_bytes);
    if (max_names > (uint64_t(1) << 40)) return rc_fail(RC_ERR_ARGUMENT, "max_names above 2^40");
    if (int rc = rc::check_device(device)) return rc;
    rc::DeviceGuard guard(device);
    rc_index *x = new rc_index;
    x->device = device;
    x->name_bytes = name_bytes;
    x->max_names = max_names;
    int rc = allocate(max_names, &x->pool, &x->table, &x->entries);
    if (!rc) rc = x->ring.create();
    if (rc) {
        rc_index_destroy(x);  // frees whatever was allocated; untracking an untracked handle is a no-op
        return rc;
    }
    rc_track(x, destroy_tracked);
    *out = x;
    return RC_OK;
}

void rc_index_destroy(rc_index *x) {
    if (!x) return;
    rc::teardown(x, [x] {
        if (x->pool) (void)hipFree(x->pool);
        if (x->table) (void)hipFree(x->table);
        x->ring.release([](rc_index::Staging &w) {
            w.h_stage.release();
            w.d_stage.release();
        });
    });
    delete x;
}

uint32_t rc_index_name_bytes(const rc_index *x) { return x ? x->name_bytes : 0; }
uint64_t rc_index_used(const rc_index *x) { return x ? x->used : 0; }

int rc_index_add_host(rc_index *x, uint64_t n, const uint8_t *names, uint64_t *first_id) {
    if (!x) return rc_fail(RC_ERR_ARGUMENT, "null index");
    if (!first_id) return rc_fail(RC_ERR_ARGUMENT, "null first_id");
    if (n && !names) return rc_fail(RC_ERR_ARGUMENT, "null arrays");
    std::lock_guard<std::mutex> lock(x->mu);
    *first_id = x->used;
    if (n == 0) return RC_OK;
    if (int rc = check_room(x, n)) return rc;
    rc::DeviceGuard guard(x->device);
    // the pool image: every name zero-padded to its 64-byte slot
    std::vector<uint8_t> image(n * kIndexSlot, 0);
    for (uint64_t i = 0; i < n; ++i)
        std::memcpy(image.data() + kIndexSlot * i, names + uint64_t(x->name_bytes) * i, x->name_bytes);
    RC_HIP_TRY(hipDeviceSynchronize());  // the index's outstanding work, on whatever stream
    RC_HIP_TRY(hipMemcpy(x->pool + kIndexSlot * x->used, image.data(), image.size(), hipMemcpyHostToDevice));
    const IndexWork w{nullptr, nullptr, 0, n, x->used};
    if (int rc = rc_index_launch_insert(view_of(x), w, nullptr)) return rc;
    RC_HIP_TRY(hipDeviceSynchronize());
    x->used += n;
    return RC_OK;
}

int rc_index_resolve_chunks(rc_index *x, const rc_chunker *layout, uint64_t n, const uint64_t *lens,
                            const int64_t *d_counts, const uint8_t *d_names, uint64_t *id_base,
                            int64_t *d_owner, uint8_t *d_fresh, void *hip_stream) {
    if (!x || !layout) return rc_fail(RC_ERR_ARGUMENT, "null index or chunker");
    if (!id_base) return rc_fail(RC_ERR_ARGUMENT, "null id_base");
    if (n == 0) {
        *id_base = x->used;
        return RC_OK;
    }
    if (!lens || !d_counts || !d_names || !d_owner || !d_fresh) return rc_fail(RC_ERR_ARGUMENT, "null arrays");
    if (reinterpret_cast<uintptr_t>(d_names) & 7)
        return rc_fail(RC_ERR_ALIGN, "d_names is not 8-byte aligned");
    std::vector<uint64_t> caps(n);
    const uint64_t slots = rc_cut_capacity(layout, n, lens, caps.data());
    std::lock_guard<std::mutex> lock(x->mu);
    *id_base = x->used;
    if (int rc = check_room(x, slots)) return rc;
    rc::DeviceGuard guard(x->device);
    const hipStream_t st = static_cast<hipStream_t>(hip_stream);
    rc::SlotRing<rc_index::Staging>::Slot *w = nullptr;
    if (int rc = x->ring.acquire(w)) return rc;
    const size_t bytes = n * sizeof(uint64_t);
    if (int rc = w->h_stage.ensure(bytes)) return rc;
    if (int rc = w->d_stage.ensure(bytes)) return rc;
    uint64_t *u = static_cast<uint64_t *>(w->h_stage.p);
    uint64_t acc = 0;
    for (uint64_t i = 0; i < n; ++i) {
        u[i] = acc;
        acc += caps[i];
    }
    RC_HIP_TRY(hipMemcpyAsync(w->d_stage.p, u, bytes, hipMemcpyHostToDevice, st));
    const IndexWork work{static_cast<const uint64_t *>(w->d_stage.p), d_counts, n, slots, x->used};
    if (int rc = resolve_work(view_of(x), work, d_names, d_owner, d_fresh, st)) return rc;
    if (int rc = x->ring.finish(*w, st)) return rc;
    x->used += slots;
    return RC_OK;
}

int rc_index_lookup_device(rc_index *x, uint64_t n, const uint8_t *d_names, int64_t *d_owner,
                           void *hip_stream) {
    if (!x) return rc_fail(RC_ERR_ARGUMENT, "null index");
    if (n == 0) return RC_OK;
    if (!d_names || !d_owner) return rc_fail(RC_ERR_ARGUMENT, "null arrays");
    if (reinterpret_cast<uintptr_t>(d_names) & 7)
        return rc_fail(RC_ERR_ALIGN, "d_names is not 8-byte aligned");
    std::lock_guard<std::mutex> lock(x->mu);
    rc::DeviceGuard guard(x->device);
    return rc_index_launch_lookup(view_of(x), n, d_names, d_owner, static_cast<hipStream_t>(hip_stream));
}

int rc_index_resolve_names_device(rc_index *x, uint64_t n, const uint8_t *d_names, uint64_t *id_base,
                                  int64_t *d_owner, uint8_t *d_fresh, void *hip_stream) {
    if (!x) return rc_fail(RC_ERR_ARGUMENT, "null index");
    if (!id_base) return rc_fail(RC_ERR_ARGUMENT, "null id_base");
    if (n == 0) {
        *id_base = x->used;
        return RC_OK;
    }
    if (!d_names || !d_owner || !d_fresh) return rc_fail(RC_ERR_ARGUMENT, "null arrays");
    if (reinterpret_cast<uintptr_t>(d_names) & 7)
        return rc_fail(RC_ERR_ALIGN, "d_names is not 8-byte aligned");
    std::lock_guard<std::mutex> lock(x->mu);
    *id_base = x->used;
    if (int rc = check_room(x, n)) return rc;
    rc::DeviceGuard guard(x->device);
    const hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const IndexWork work{nullptr, nullptr, 0, n, x->used};  // flat: every lane carries a name
    if (int rc = resolve_work(view_of(x), work, d_names, d_owner, d_fresh, st)) return rc;
    x->used += n;
    return RC_OK;
}

int rc_index_reserve(rc_index *x, uint64_t max_names) {
    if (!x) return rc_fail(RC_ERR_ARGUMENT, "null index");
    if (max_names > (uint64_t(1) << 40)) return rc_fail(RC_ERR_ARGUMENT, "max_names above 2^40");
    std::lock_guard<std::mutex> lock(x->mu);
    if (max_names <= x->max_names) return RC_OK;
    rc::DeviceGuard guard(x->device);
    RC_HIP_TRY(hipDeviceSynchronize());  // the index's outstanding work, on whatever stream
    uint8_t *pool = nullptr;
    uint64_t *table = nullptr, entries = 0;
    if (int rc = allocate(max_names, &pool, &table, &entries)) return rc;
    int rc = 0;
    if (x->used && hipMemcpy(pool, x->pool, x->used * kIndexSlot, hipMemcpyDeviceToDevice) != hipSuccess)
        rc = rc_fail(RC_ERR_HIP, "hipMemcpy of the pool failed");
    const IndexView v{pool, table, entries - 1, x->name_bytes};
    if (!rc) rc = rc_index_launch_reinsert(v, x->table, x->entries, nullptr);
    if (!rc && hipDeviceSynchronize() != hipSuccess) rc = rc_fail(RC_ERR_HIP, "hipDeviceSynchronize failed");
    if (rc) {
        (void)hipFree(pool);
        (void)hipFree(table);
        return rc;
    }
    (void)hipFree(x->pool);
    (void)hipFree(x->table);
    x->pool = pool;
    x->table = table;
    x->entries = entries;
    x->max_names = max_names;
    return RC_OK;
}

}  // extern "C"

int rc_index_view(rc_index *x, IndexView *out) {
    if (!x || !out) return rc_fail(RC_ERR_ARGUMENT, "null index");
    std::lock_guard<std::mutex> lock(x->mu);
    *out = view_of(x);
    return RC_OK;
}
