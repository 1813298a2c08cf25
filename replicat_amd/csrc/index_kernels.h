// index_kernels.h -- internal interface between index.hip (kernels) and capi_index.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr uint64_t kIndexSlot = 64;           // bytes per pooled name
constexpr uint64_t kIndexEmpty = ~uint64_t(0);  // a table entry that holds no id
constexpr int kIndexThreads = 256;

// The index as the kernels see it: pool + 64 id = the name of id (zero-padded past name_bytes),
// table = `mask + 1` ids (a power of two), kIndexEmpty where free.
struct IndexView {
    uint8_t *pool;
    uint64_t *table;
    uint64_t mask;
    uint32_t name_bytes;
};

// Which lanes of a launch carry a name: the cut slots s = cut_base[i] + k, k < counts[i], of n
// streams (`slots` = the layout's cut slots), or, with cut_base null, every one of `slots`.
// Lane s carries id id_base + s.
struct IndexWork {
    const uint64_t *cut_base;
    const int64_t *counts;
    uint64_t n, slots, id_base;
};


// An index's view for a launch of another module's (gc.hip's sweep reads the table and the pool).
// The caller orders that launch against the index's other calls as it would order those.
struct rc_index;
int rc_index_view(rc_index *idx, IndexView *out);

// pool[id_base + s] = the name at names + 64 s (the first name_bytes bytes), for the lanes of w.
int rc_index_launch_stage(const IndexView &v, const IndexWork &w, const uint8_t *names, hipStream_t st);
// Insert the pooled names of the lanes of w.
int rc_index_launch_insert(const IndexView &v, const IndexWork &w, hipStream_t st);
// owner[s], fresh[s] for the lanes of w (after the insert launch).
int rc_index_launch_resolve(const IndexView &v, const IndexWork &w, int64_t *owner, uint8_t *fresh,
                            hipStream_t st);
// owner[i] = the id the index holds for the name at names + 64 i (the first name_bytes bytes), -1
// if none, -2 if the probe bound was exhausted; i < n.  Inserts nothing.
int rc_index_launch_lookup(const IndexView &v, uint64_t n, const uint8_t *names, int64_t *owner,
                           hipStream_t st);
// Insert every id of old_table (old_entries of them) into v, whose pool already holds the names.
int rc_index_launch_reinsert(const IndexView &v, const uint64_t *old_table, uint64_t old_entries,
                             hipStream_t st);
