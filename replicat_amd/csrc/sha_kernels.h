// sha_kernels.h -- internal interface between sha2.hip / sha3.hip (kernels) and capi_digest.cpp.
//
// The SHA hashers share the BLAKE2b path's work lists: B2Item / B2UItem (digest_kernels.h) and
// the device sort that builds the longest-first chunk list (rc_b2_launch_sort, blake2b.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "capi_internal.h"
#include "digest_kernels.h"

constexpr int kShaThreads = 256;           // one message per lane, 4 waves per workgroup
constexpr uint64_t kShaMaxGroups = 512;    // two waves per SIMD on 256 CUs; items beyond loop
constexpr uint64_t kShaGroupBlocks = 256;  // latency form: one wave (two 32-lane groups) per SIMD
constexpr uint64_t kShaAllLanes = ~0ull;   // lane_max: every item one per lane (the lane kernel)

static_assert(sizeof(rc_sha2_state) == 256 && sizeof(rc_sha3_state) == 256,
              "every hash state is a 256-byte device record");

inline unsigned rc_sha_grid(uint64_t upper) {
    uint64_t wg = (upper + kShaThreads - 1) / kShaThreads;
    if (wg > kShaMaxGroups) wg = kShaMaxGroups;
    return static_cast<unsigned>(wg ? wg : 1);
}

// Digests (outlen = 28 / 32 / 48 / 64 bytes) of a longest-first work list already on the device:
// d_total (device, may be null) or n items; the grid is sized for `upper` items.  Both families
// have a latency form for long messages (sha2.hip: one message per wave, the schedule of the 16
// blocks ahead on its other lanes; sha3.hip: one state over 25 lanes): items longer than lane_max
// go to it, the rest to lanes; 0: every item by the latency form, kShaAllLanes: every item by
// lanes, in the lane kernel.
int rc_sha2_launch_items(const B2Item *d_items, const uint64_t *d_total, uint64_t n, uint64_t upper,
                         uint32_t outlen, uint8_t *d_out, uint64_t lane_max, hipStream_t stream);
int rc_sha3_launch_items(const B2Item *d_items, const uint64_t *d_total, uint64_t n, uint64_t upper,
                         uint32_t outlen, uint8_t *d_out, uint64_t lane_max, hipStream_t stream);

// The lane / group split of a SHA-3 batch of `bytes` message bytes whose longest message is at
// most `longest` bytes.  Measured (scripts/sha_probe.py, profiles/sha/sha_probe.json, all four
// rates): a group's chain is 4.7-4.9 us per block against a lane's 10.4-11.0, i.e. 0.45-0.47 of
// it, but a batch hashed by groups alone runs at 22.8-45.0 GiB/s against 509-974 by lanes (two
// messages per wave, one wave per SIMD).  So groups take only what would otherwise set the
// batch's time: a message of up to 7/16 of the longest ends in a lane before the longest ends
// in a group and goes to a lane.  And groups are used at all only while their throughput cannot
// become the bound: hashing `bytes` by groups takes less than the longest group chain while
// bytes < longest x 1,600 (chain ns per byte x group bytes per ns = 33.8 x 48.3, 35.6 x 45.4,
// 44.8 x 35.6, 67.2 x 24.5 for the four rates); the rule uses longest << 10.  Beyond that
// (config 2's 64 GiB: 317-634 ms by lanes, 1,530-3,037 ms by groups) every message goes to a
// lane.  knob_max (RC_SHA_LANE_MAX, knobs.h: -1 = the rule) overrides the whole rule, 0 sending
// every message to groups.
//
// SHA-2's latency form hashes one message per wave (sha2.hip), so its throughput is lower still
// and its chain gains less (the rounds remain): the same rule with a wave's chain over a lane's
// as the fraction of the longest (in sixteenths, rounded down so that lanes never outlast the
// longest wave) and a smaller bytes bound.  The measured pairs and products are in DESIGN.md
// §3f (profiles/sha/sha_probe.json, "chain" and "config2" of sha2-256 and sha2-512, /lane and
// /latency).
constexpr int kSha2LaneSixteenths = 9;
constexpr int kSha2BytesShift = 9;
inline uint64_t rc_sha_lane_max(uint32_t algo, uint64_t bytes, uint64_t longest, int64_t knob_max) {
    if (knob_max >= 0) return (uint64_t)knob_max;
    const bool sha2 = algo == RC_HASH_SHA2;
    if (bytes > (longest << (sha2 ? kSha2BytesShift : 10))) return kShaAllLanes;
    const uint64_t lane_max = longest / 16 * (sha2 ? kSha2LaneSixteenths : 7);
    return lane_max ? lane_max : kShaAllLanes;  // 0 would mean "everything to the latency form"
}

// Incremental updates of n (state, buffer) items (rc_sha2_state / rc_sha3_state records of the
// handle's outlen); finals write the digest at d_out + 64 * slot and leave the state as it was.
int rc_sha2_launch_update(const B2UItem *d_items, uint64_t n, uint32_t outlen, uint8_t *d_out,
                          hipStream_t stream);
int rc_sha3_launch_update(const B2UItem *d_items, uint64_t n, uint32_t outlen, uint8_t *d_out,
                          hipStream_t stream);

// d_tags[2 i], d_tags[2 i + 1] = the digest_size and algo words of item i's state record.
int rc_sha_launch_tags(const B2UItem *d_items, uint64_t n, uint32_t *d_tags, hipStream_t stream);
