// capi_gc.cpp -- the host side of include/replicat_gc.h: the handle (an rc_index of what is
// referenced, the MAC's keyed state on the device, the batch buffers) and the batching of the
// host forms.  The kernels are gc.hip's and index.hip's.
#include <hip/hip_runtime.h>

#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/replicat_gc.h"
#include "capi_internal.h"
#include "gc_kernels.h"

static_assert(RC_GC_REFERENCED == kGcReferenced && RC_GC_DELETE == kGcDelete &&
                  RC_GC_TAG_MISMATCH == kGcTagMismatch && RC_GC_EXHAUSTED == kGcExhausted,
              "one set of verdicts for callers and kernels");

struct rc_gc {
    int device = 0;
    uint32_t digest_bytes = 0, name_bytes = 0;
    uint64_t max_refs = 0;
    rc_index *index = nullptr;
    rc_blake2b_state *d_mac = nullptr;  // null: unkeyed
    std::mutex mu;
    rc::DevBuf d_scratch, d_total;  // the compaction's workgroup counts and its total
    // one batch of a host form
    rc::DevBuf d_in, d_names, d_tags, d_sel_names, d_verdict, d_idx, d_owner, d_fresh;
    // rc_gc_timing_*: event pairs around the names, the sweep and the compaction launches
    rc::PairTimer t_names, t_sweep, t_compact;
};

namespace {

void destroy_tracked(void *p) { rc_gc_destroy(static_cast<rc_gc *>(p)); }

// n items of `bytes` bytes, back to back, as zero-padded 64-byte slots.
void to_slots(const uint8_t *src, uint64_t n, uint32_t bytes, std::vector<uint8_t> &image) {
    image.assign(n * kIndexSlot, 0);
    for (uint64_t i = 0; i < n; ++i) std::memcpy(image.data() + kIndexSlot * i, src + uint64_t(bytes) * i, bytes);
}

// Room in the index for `more` further ids, at least doubling when it has to grow.
int ensure_room(rc_gc *g, uint64_t more) {
    const uint64_t need = rc_index_used(g->index) + more;
    if (need <= g->max_refs) return 0;
    const uint64_t want = std::max(need, 2 * g->max_refs);
    if (int rc = rc_index_reserve(g->index, want)) return rc;
    g->max_refs = want;
    return 0;
}

// The batch's digests (host, nb of them) into d_in and, keyed, their names into d_names: the
// device slots the index takes for them.
int stage_digests(rc_gc *g, const uint8_t *digests, uint64_t nb, std::vector<uint8_t> &image,
                  const uint8_t **d_keys) {
    to_slots(digests, nb, g->digest_bytes, image);
    if (int rc = g->d_in.ensure(image.size())) return rc;
    RC_HIP_TRY(hipMemcpy(g->d_in.p, image.data(), image.size(), hipMemcpyHostToDevice));
    *d_keys = static_cast<const uint8_t *>(g->d_in.p);
    if (!g->d_mac) return 0;
    if (int rc = g->d_names.ensure(image.size())) return rc;
    const uint8_t *d_digests = *d_keys;
    if (int rc = rc::timed(g->t_names, nullptr, [&] {
            return rc_gc_launch_names(g->d_mac, nb, d_digests, g->digest_bytes, true, nullptr, 0,
                                      static_cast<uint8_t *>(g->d_names.p), nullptr, nullptr);
        }))
        return rc;
    *d_keys = static_cast<const uint8_t *>(g->d_names.p);
    return 0;
}

// Insert the batch's nb staged keys (flat resolve: owners in d_owner, fresh flags in d_fresh) and
// fail if any owner shows an exhausted probe bound.
int resolve_batch(rc_gc *g, const uint8_t *d_keys, uint64_t nb, std::vector<int64_t> &owners) {
    if (int rc = ensure_room(g, nb)) return rc;
    if (int rc = g->d_owner.ensure(nb * sizeof(int64_t))) return rc;
    if (int rc = g->d_fresh.ensure(nb)) return rc;
    uint64_t base = 0;
    if (int rc = rc_index_resolve_names_device(g->index, nb, d_keys, &base, static_cast<int64_t *>(g->d_owner.p),
                                               static_cast<uint8_t *>(g->d_fresh.p), nullptr))
        return rc;
    owners.resize(nb);
    RC_HIP_TRY(hipMemcpy(owners.data(), g->d_owner.p, nb * sizeof(int64_t), hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < nb; ++i)
        if (owners[i] < 0)
            return rc_fail(RC_ERR_PROBE_BOUND, "chunk index: lookup %llu exhausted its probe bound",
                           (unsigned long long)i);
    return 0;
}

int sweep_enqueue(rc_gc *g, uint64_t n, const uint8_t *d_names, const uint8_t *d_tags,
                  uint64_t index_base, uint8_t *d_verdict, uint64_t *d_delete_idx,
                  uint64_t *d_n_delete, hipStream_t st) {
    IndexView v;
    if (int rc = rc_index_view(g->index, &v)) return rc;
    if (int rc = g->d_scratch.ensure(rc_gc_scratch_words(n) * sizeof(uint64_t))) return rc;
    if (int rc = rc::timed(g->t_sweep, st, [&] {
            return rc_gc_launch_sweep(v, g->d_mac, n, d_names, d_tags, d_verdict, st);
        }))
        return rc;
    return rc::timed(g->t_compact, st, [&] {
        return rc_gc_launch_compact(d_verdict, n, kGcDelete, index_base, static_cast<uint64_t *>(g->d_scratch.p),
                                    d_delete_idx, d_n_delete, st);
    });
}

}  // namespace

extern "C" {

int rc_gc_create(uint32_t digest_bytes, uint32_t name_bytes, const uint8_t *mac_key,
                 uint32_t mac_keylen, uint64_t max_refs, int device, rc_gc **out) {
    if (!out) return rc_fail(RC_ERR_ARGUMENT, "null output handle");
    *out = nullptr;
    if (digest_bytes < 1 || digest_bytes > kIndexSlot)
        return rc_fail(RC_ERR_ARGUMENT, "digest_bytes must be 1..64, not %u", digest_bytes);
    if (name_bytes < 1 || name_bytes > kIndexSlot)
        return rc_fail(RC_ERR_ARGUMENT, "name_bytes must be 1..64, not %u", name_bytes);
    if (mac_key && (mac_keylen < 1 || mac_keylen > 64))
        return rc_fail(RC_ERR_ARGUMENT, "mac_keylen must be 1..64, not %u", mac_keylen);
    if (!mac_key && name_bytes != digest_bytes)
        return rc_fail(RC_ERR_ARGUMENT, "unkeyed: name_bytes %u must equal digest_bytes %u", name_bytes,
                       digest_bytes);
    if (max_refs > (uint64_t(1) << 40)) return rc_fail(RC_ERR_ARGUMENT, "max_refs above 2^40");
    if (int rc = rc::check_device(device)) return rc;
    rc::DeviceGuard guard(device);
    rc_gc *g = new rc_gc;
    g->device = device;
    g->digest_bytes = digest_bytes;
    g->name_bytes = name_bytes;
    g->max_refs = max_refs;
    int rc = rc_index_create(name_bytes, max_refs, device, &g->index);
    if (!rc) rc_untrack(g->index);  // the handle owns it: destroyed with the handle, and only then
    if (!rc) rc = g->d_total.ensure(sizeof(uint64_t));
    if (!rc && mac_key) {
        rc_blake2b_state st;
        rc = rc_blake2b_state_init(name_bytes, mac_key, mac_keylen, nullptr, 0, nullptr, 0, &st);
        if (!rc && hipMalloc(reinterpret_cast<void **>(&g->d_mac), sizeof st) != hipSuccess)
            rc = rc_fail(RC_ERR_HIP, "hipMalloc of the MAC state failed");
        if (!rc && hipMemcpy(g->d_mac, &st, sizeof st, hipMemcpyHostToDevice) != hipSuccess)
            rc = rc_fail(RC_ERR_HIP, "hipMemcpy of the MAC state failed");
    }
    if (rc) {
        rc_gc_destroy(g);
        return rc;
    }
    rc_track(g, destroy_tracked);
    *out = g;
    return RC_OK;
}

void rc_gc_destroy(rc_gc *g) {
    if (!g) return;
    rc::teardown(g, [g] {
        rc_index_destroy(g->index);
        if (g->d_mac) (void)hipFree(g->d_mac);
        for (rc::DevBuf *b : {&g->d_scratch, &g->d_total, &g->d_in, &g->d_names, &g->d_tags, &g->d_sel_names,
                              &g->d_verdict, &g->d_idx, &g->d_owner, &g->d_fresh})
            b->release();
        for (rc::PairTimer *t : {&g->t_names, &g->t_sweep, &g->t_compact}) t->release();
    });
    delete g;
}

int rc_gc_timing_enable(rc_gc *g, int enable) {
    if (!g) return rc_fail(RC_ERR_ARGUMENT, "null gc");
    return rc::timing_enable(g, {&g->t_names, &g->t_sweep, &g->t_compact}, enable);
}

int rc_gc_timing_read(rc_gc *g, double *names_ms, double *sweep_ms, double *compact_ms, uint64_t *calls) {
    if (!g) return rc_fail(RC_ERR_ARGUMENT, "null gc");
    std::lock_guard<std::mutex> lock(g->mu);
    rc::DeviceGuard guard(g->device);
    if (int rc = g->t_names.read(names_ms, nullptr)) return rc;
    if (int rc = g->t_compact.read(compact_ms, nullptr)) return rc;
    return g->t_sweep.read(sweep_ms, calls);
}

uint32_t rc_gc_name_bytes(const rc_gc *g) { return g ? g->name_bytes : 0; }
uint64_t rc_gc_used(const rc_gc *g) { return g ? rc_index_used(g->index) : 0; }
uint64_t rc_gc_capacity(const rc_gc *g) { return g ? g->max_refs : 0; }

int rc_gc_reference_host(rc_gc *g, uint64_t n, const uint8_t *digests) {
    if (!g) return rc_fail(RC_ERR_ARGUMENT, "null gc");
    if (n && !digests) return rc_fail(RC_ERR_ARGUMENT, "null arrays");
    std::lock_guard<std::mutex> lock(g->mu);
    rc::DeviceGuard guard(g->device);
    std::vector<uint8_t> image;
    std::vector<int64_t> owners;
    for (uint64_t off = 0; off < n; off += RC_GC_BATCH) {
        const uint64_t nb = std::min<uint64_t>(RC_GC_BATCH, n - off);
        const uint8_t *d_keys = nullptr;
        if (int rc = stage_digests(g, digests + off * g->digest_bytes, nb, image, &d_keys)) return rc;
        if (int rc = resolve_batch(g, d_keys, nb, owners)) return rc;
    }
    return RC_OK;
}

int rc_gc_reference_device(rc_gc *g, uint64_t n, const uint8_t *d_digests) {
    if (!g) return rc_fail(RC_ERR_ARGUMENT, "null gc");
    if (n && !d_digests) return rc_fail(RC_ERR_ARGUMENT, "null arrays");
    if (reinterpret_cast<uintptr_t>(d_digests) & 7) return rc_fail(RC_ERR_ALIGN, "d_digests is not 8-byte aligned");
    std::lock_guard<std::mutex> lock(g->mu);
    rc::DeviceGuard guard(g->device);
    std::vector<int64_t> owners;
    for (uint64_t off = 0; off < n; off += RC_GC_BATCH) {
        const uint64_t nb = std::min<uint64_t>(RC_GC_BATCH, n - off);
        // unkeyed, the slots are the keys where they lie: the index reads name_bytes of a slot
        const uint8_t *d_keys = d_digests + kIndexSlot * off;
        if (g->d_mac) {
            if (int rc = g->d_names.ensure(nb * kIndexSlot)) return rc;
            const uint8_t *d_batch = d_keys;
            if (int rc = rc::timed(g->t_names, nullptr, [&] {
                    return rc_gc_launch_names(g->d_mac, nb, d_batch, g->digest_bytes, true, nullptr, 0,
                                              static_cast<uint8_t *>(g->d_names.p), nullptr, nullptr);
                }))
                return rc;
            d_keys = static_cast<const uint8_t *>(g->d_names.p);
        }
        if (int rc = resolve_batch(g, d_keys, nb, owners)) return rc;
    }
    return RC_OK;
}

int rc_gc_sweep_device(rc_gc *g, uint64_t n, const uint8_t *d_names, const uint8_t *d_tags,
                       uint64_t index_base, uint8_t *d_verdict, uint64_t *d_delete_idx,
                       uint64_t *d_n_delete, void *hip_stream) {
    if (!g) return rc_fail(RC_ERR_ARGUMENT, "null gc");
    if (!d_n_delete) return rc_fail(RC_ERR_ARGUMENT, "null d_n_delete");
    if (n && (!d_names || !d_tags || !d_verdict || !d_delete_idx)) return rc_fail(RC_ERR_ARGUMENT, "null arrays");
    if (n > (uint64_t(1) << 31)) return rc_fail(RC_ERR_ARGUMENT, "more than 2^31 entries in one call");
    if ((reinterpret_cast<uintptr_t>(d_names) | reinterpret_cast<uintptr_t>(d_tags)) & 7)
        return rc_fail(RC_ERR_ALIGN, "d_names or d_tags is not 8-byte aligned");
    std::lock_guard<std::mutex> lock(g->mu);
    rc::DeviceGuard guard(g->device);
    return sweep_enqueue(g, n, d_names, d_tags, index_base, d_verdict, d_delete_idx, d_n_delete,
                         static_cast<hipStream_t>(hip_stream));
}

int rc_gc_sweep_host(rc_gc *g, uint64_t n, const uint8_t *names, const uint8_t *tags, uint8_t *verdict,
                     uint64_t *delete_idx, uint64_t *n_delete) {
    if (!g) return rc_fail(RC_ERR_ARGUMENT, "null gc");
    if (!n_delete) return rc_fail(RC_ERR_ARGUMENT, "null n_delete");
    *n_delete = 0;
    if (n && (!names || !tags || !verdict || !delete_idx)) return rc_fail(RC_ERR_ARGUMENT, "null arrays");
    std::lock_guard<std::mutex> lock(g->mu);
    rc::DeviceGuard guard(g->device);
    std::vector<uint8_t> image;
    uint64_t found = 0;
    for (uint64_t off = 0; off < n; off += RC_GC_BATCH) {
        const uint64_t nb = std::min<uint64_t>(RC_GC_BATCH, n - off);
        for (rc::DevBuf *b : {&g->d_names, &g->d_tags})
            if (int rc = b->ensure(nb * kIndexSlot)) return rc;
        if (int rc = g->d_verdict.ensure(nb)) return rc;
        if (int rc = g->d_idx.ensure(nb * sizeof(uint64_t))) return rc;
        to_slots(names + off * g->name_bytes, nb, g->name_bytes, image);
        RC_HIP_TRY(hipMemcpy(g->d_names.p, image.data(), image.size(), hipMemcpyHostToDevice));
        to_slots(tags + off * g->name_bytes, nb, g->name_bytes, image);
        RC_HIP_TRY(hipMemcpy(g->d_tags.p, image.data(), image.size(), hipMemcpyHostToDevice));
        if (int rc = sweep_enqueue(g, nb, static_cast<const uint8_t *>(g->d_names.p),
                                   static_cast<const uint8_t *>(g->d_tags.p), off,
                                   static_cast<uint8_t *>(g->d_verdict.p), static_cast<uint64_t *>(g->d_idx.p),
                                   static_cast<uint64_t *>(g->d_total.p), nullptr))
            return rc;
        uint64_t total = 0;
        RC_HIP_TRY(hipMemcpy(&total, g->d_total.p, sizeof total, hipMemcpyDeviceToHost));
        RC_HIP_TRY(hipMemcpy(verdict + off, g->d_verdict.p, nb, hipMemcpyDeviceToHost));
        for (uint64_t i = 0; i < nb; ++i)
            if (verdict[off + i] == kGcExhausted)
                return rc_fail(RC_ERR_PROBE_BOUND, "chunk index: lookup %llu exhausted its probe bound",
                               (unsigned long long)(off + i));
        if (total > nb) return rc_fail(RC_ERR_HIP, "the compaction counted %llu of %llu entries",
                                       (unsigned long long)total, (unsigned long long)nb);
        if (total)
            RC_HIP_TRY(hipMemcpy(delete_idx + found, g->d_idx.p, total * sizeof(uint64_t), hipMemcpyDeviceToHost));
        found += total;
    }
    *n_delete = found;
    return RC_OK;
}

int rc_gc_unreferenced_host(rc_gc *g, uint64_t n, const uint8_t *digests, uint64_t *idx, uint8_t *names,
                            uint8_t *tags, uint64_t *n_out) {
    if (!g) return rc_fail(RC_ERR_ARGUMENT, "null gc");
    if (!n_out) return rc_fail(RC_ERR_ARGUMENT, "null n_out");
    *n_out = 0;
    if (n && (!digests || !idx || !names || !tags)) return rc_fail(RC_ERR_ARGUMENT, "null arrays");
    std::lock_guard<std::mutex> lock(g->mu);
    rc::DeviceGuard guard(g->device);
    const uint32_t nb_name = g->name_bytes;
    std::vector<uint8_t> image;
    std::vector<int64_t> owners;
    uint64_t found = 0;
    for (uint64_t off = 0; off < n; off += RC_GC_BATCH) {
        const uint64_t nb = std::min<uint64_t>(RC_GC_BATCH, n - off);
        const uint8_t *d_keys = nullptr;
        if (int rc = stage_digests(g, digests + off * g->digest_bytes, nb, image, &d_keys)) return rc;
        if (int rc = resolve_batch(g, d_keys, nb, owners)) return rc;
        // the fresh ones, in order: unreferenced, and the first of their digest
        if (int rc = g->d_scratch.ensure(rc_gc_scratch_words(nb) * sizeof(uint64_t))) return rc;
        if (int rc = g->d_idx.ensure(nb * sizeof(uint64_t))) return rc;
        if (int rc = rc::timed(g->t_compact, nullptr, [&] {
                return rc_gc_launch_compact(static_cast<const uint8_t *>(g->d_fresh.p), nb, 1, off,
                                            static_cast<uint64_t *>(g->d_scratch.p),
                                            static_cast<uint64_t *>(g->d_idx.p),
                                            static_cast<uint64_t *>(g->d_total.p), nullptr);
            }))
            return rc;
        uint64_t total = 0;
        RC_HIP_TRY(hipMemcpy(&total, g->d_total.p, sizeof total, hipMemcpyDeviceToHost));
        if (total > nb) return rc_fail(RC_ERR_HIP, "the compaction counted %llu of %llu digests",
                                       (unsigned long long)total, (unsigned long long)nb);
        if (!total) continue;
        RC_HIP_TRY(hipMemcpy(idx + found, g->d_idx.p, total * sizeof(uint64_t), hipMemcpyDeviceToHost));
        if (!g->d_mac) {  // name = tag = digest: nothing to launch
            for (uint64_t k = 0; k < total; ++k)
                for (uint8_t *dst : {names, tags})
                    std::memcpy(dst + (found + k) * nb_name, digests + idx[found + k] * g->digest_bytes, nb_name);
        } else {  // the survivors' names gathered, and their tags
            for (rc::DevBuf *b : {&g->d_sel_names, &g->d_tags})
                if (int rc = b->ensure(total * kIndexSlot)) return rc;
            if (int rc = rc::timed(g->t_names, nullptr, [&] {
                    return rc_gc_launch_names(g->d_mac, total, d_keys, nb_name, false,
                                              static_cast<const uint64_t *>(g->d_idx.p), off,
                                              static_cast<uint8_t *>(g->d_sel_names.p),
                                              static_cast<uint8_t *>(g->d_tags.p), nullptr);
                }))
                return rc;
            image.resize(total * kIndexSlot);
            for (const auto &[buf, dst] : {std::pair<rc::DevBuf *, uint8_t *>{&g->d_sel_names, names},
                                           std::pair<rc::DevBuf *, uint8_t *>{&g->d_tags, tags}}) {
                RC_HIP_TRY(hipMemcpy(image.data(), buf->p, image.size(), hipMemcpyDeviceToHost));
                for (uint64_t k = 0; k < total; ++k)
                    std::memcpy(dst + (found + k) * nb_name, image.data() + kIndexSlot * k, nb_name);
            }
        }
        found += total;
    }
    *n_out = found;
    return RC_OK;
}

}  // extern "C"
