// restore_kernels.h -- internal interface between restore.hip (kernel) and capi_restore.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/replicat_restore.h"

// The plaintext buffer of one chunk: what the verdict kernel zero-fills when the chunk fails.
struct RestorePlain {
    uint64_t ptr, len;
};

struct RestoreVerdictArgs {
    const uint8_t *ok;          // the cipher's tag verdicts, one byte per chunk; null: no cipher
    const uint8_t *computed;    // digests of the plaintexts, 64-byte slots
    const uint8_t *expected;    // the recorded digests, 64-byte slots
    const RestorePlain *plain;  // buffers to wipe on failure; null: nothing is wiped
    uint8_t *status;            // RC_CHUNK_* per chunk
    uint64_t n;
    uint32_t digest_size;       // bytes of a slot that count, 1..64
};

constexpr int kRestoreThreads = 256;  // 4 waves: one wave per chunk


// status[i] for n chunks, and zeros over plain[i] where it is not RC_CHUNK_OK.
int rc_restore_launch_verdict(const RestoreVerdictArgs &a, hipStream_t stream);
