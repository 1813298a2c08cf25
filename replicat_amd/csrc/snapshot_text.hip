// snapshot_text.hip -- the fixed text of every file of a snapshot's `data`
// (include/replicat_snapshot.h, "Writing the files' text"): the m + 1 pieces of serialize(data)
// between the files' part lists, written from columns -- path bytes, digest slots, metadata
// integers -- instead of being uploaded.  Listed file j is layout file order[j]:
//     head(j) = {"path": Q ,"chunks":[            tail(j) = ,"digest": D [,"metadata": M]
//     piece 0 = first + head(0)    piece j = tail(j - 1) },  head(j)    piece m = tail(m - 1) }] last
//
// One WAVE per piece, kSnapTextWaves pieces per workgroup, no workgroup barrier: the waves of a
// workgroup walk paths of different lengths.  Every value that places text (the write position,
// a file's flags, the lengths of its numbers) is wave-uniform.
//
//   len   the length of piece j: constants, the digits of the seven numbers (one lane each) and
//         the sum over the path's bytes of rc_snap_path_term, the lanes striding over the bytes.
//   text  the piece, built in the wave's own LDS buffer at the destination's offset modulo 16 and
//         stored as aligned 16-byte granules; only the piece's first and last granule, which it
//         shares with the part records around it, leave as byte stores of its own bytes.  The
//         buffer is flushed whenever kFlushAt bytes are in it: whole granules go out, the partial
//         one moves to the front.  A path is taken kSnapTextStep bytes per step, one byte per
//         lane: a wave scan of the terms gives each lead byte its place, and a lead byte gets its
//         continuation bytes from the lanes behind it -- for the last three lanes from the first
//         bytes of the next step, which three lanes load ahead (clamped to the path's end), so a
//         sequence may straddle a step at any of its bytes.  Literals are immediates picked by
//         lane, hex and base64 characters range arithmetic, decimals written backwards by
//         multiply-high division: no table.
#include <hip/hip_runtime.h>

#include "snapshot_device.h"

namespace {

constexpr uint32_t kStepOut = 6 * kSnapTextStep;  // the most text one step of a path, or a tail, adds
constexpr uint32_t kFlushAt = 640;
constexpr uint32_t kWaveLds = kFlushAt + kStepOut;  // 1 KiB a wave
static_assert(kSnapTextStep == 64, "one byte per lane");
static_assert(kWaveLds % 16 == 0, "granules");
// a tail: ,"digest": + {"!b":" 88 characters "} + ,"metadata": + the keys and seven numbers of 20
static_assert(15 + 10 + 9 + 88 + 12 + kSnapMetaFixed + 7 * 20 + 2 <= kStepOut, "a tail and its separator are one step");

// LDS traffic of one wave is in order; this keeps the compiler from moving it across.
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
#pragma unroll
    for (uint32_t off = 32; off; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__device__ __forceinline__ uint8_t hex_char(uint32_t v) { return uint8_t(v + (v < 10 ? '0' : 'a' - 10)); }

// \uxxxx
__device__ __forceinline__ void put_escape(uint8_t *o, uint32_t unit) {
    o[0] = '\\';
    o[1] = 'u';
    o[2] = hex_char((unit >> 12) & 15u);
    o[3] = hex_char((unit >> 8) & 15u);
    o[4] = hex_char((unit >> 4) & 15u);
    o[5] = hex_char(unit & 15u);
}

__device__ __forceinline__ gcbytes global_of(const uint8_t *p) {
    return reinterpret_cast<gcbytes>(reinterpret_cast<uintptr_t>(p));
}

// The bytes [s, e) of path f, clamped to the packed buffer.
__device__ __forceinline__ void path_of(const SnapFileText &a, uint64_t f, uint64_t &s, uint64_t &len) {
    const uint64_t all = a.path_off[a.m];
    const uint64_t e = a.path_off[f + 1] < all ? a.path_off[f + 1] : all;
    s = a.path_off[f] < e ? a.path_off[f] : e;
    len = e - s;
}

__device__ __forceinline__ uint64_t file_of(const SnapFileText &a, uint64_t j) {
    const uint64_t f = a.order[j];
    return f < a.m ? f : a.m - 1;
}

// One wave's output: buf[k] belongs at base + k (base 16-byte aligned), k in [lo, fill).
struct WaveOut {
    uint8_t *buf;
    gbytes base;
    uint32_t fill, lo, lane;

    __device__ __forceinline__ void flush(bool last) {
        wave_sync();
        const uint32_t full = fill & ~15u;
        for (uint32_t q = lane * 16; q < full; q += 64 * 16) {
            if (q < lo) {  // the piece's first granule: the bytes before lo are a part record's
                for (uint32_t k = lo; k < 16; ++k) base[k] = buf[k];
            } else {
                *reinterpret_cast<GLOBAL u32x4 *>(base + q) = *reinterpret_cast<const u32x4 *>(buf + q);
            }
        }
        const uint32_t rest = fill - full, k = full + lane;
        if (last) {  // the piece's last granule
            if (lane < rest && k >= lo) base[k] = buf[k];
            return;
        }
        if (!full) return;
        const uint8_t keep = lane < rest ? buf[k] : uint8_t(0);
        wave_sync();
        if (lane < rest) buf[lane] = keep;
        base += full;
        fill = rest;
        lo = 0;
        wave_sync();
    }

    // room for one step
    __device__ __forceinline__ void step() {
        if (fill >= kFlushAt) flush(false);
    }

    template <int N>
    __device__ __forceinline__ void put(const char (&s)[N]) {
        static_assert(N - 1 <= 64, "a lane a character");
        uint64_t w = 0;
#pragma unroll
        for (int k = 0; k < (N - 1 + 7) / 8; ++k) {
            uint64_t c = 0;
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if (8 * k + i < N - 1) c |= uint64_t(uint8_t(s[8 * k + i])) << (8 * i);
            if (int(lane >> 3) == k) w = c;
        }
        if (lane < N - 1) buf[fill + lane] = uint8_t(w >> (8 * (lane & 7)));
        fill += N - 1;
    }

    __device__ __forceinline__ void copy(gcbytes src, uint64_t len) {
        for (uint64_t pos = 0; pos < len; pos += 64) {
            step();
            const uint64_t left = len - pos;
            if (lane < left) buf[fill + lane] = src[pos + lane];
            fill += left < 64 ? uint32_t(left) : 64u;
        }
    }

    // ,"digest": D [,"metadata": M] of file f: at most kStepOut - 17 bytes
    __device__ __forceinline__ void tail(const SnapFileText &a, uint64_t f) {
        const bool unfinished = a.unfinished && __builtin_amdgcn_readfirstlane(a.unfinished[f]);
        put(",\"digest\":");
        if (unfinished) {
            put("null");
        } else {
            put("{\"!b\":\"");
            const uint32_t L = a.digest_bytes, groups = (L + 2) / 3, pad = (3 - L % 3) % 3;
            if (lane < groups) {
                gcbytes slot = global_of(a.digests) + RC_DIGEST_SLOT * f;
                uint32_t v = 0;
#pragma unroll
                for (uint32_t k = 0; k < 3; ++k) {
                    const uint32_t at = 3 * lane + k;
                    v = (v << 8) | (at < L ? uint32_t(slot[at]) : 0u);  // the slot's tail takes no part
                }
                const uint32_t chars = b64_quad(v, lane == groups - 1 ? pad : 0u);
                uint8_t *o = buf + fill + 4 * lane;
#pragma unroll
                for (uint32_t k = 0; k < 4; ++k) o[k] = uint8_t(chars >> (8 * k));
            }
            fill += 4 * groups;
            put("\"}");
        }
        if (!a.metadata) return;
        put(",\"metadata\":");
        if (unfinished) {
            put("null");
            return;
        }
        const int64_t v = lane < kSnapMetaColumns ? a.metadata[kSnapMetaColumns * f + lane] : 0;
        const uint32_t len = rc_snap_int64_len(v);
        uint32_t end = 0;  // behind this lane's number
#define RC_META_KEY(k, text)             \
    put(text);                           \
    fill += uint32_t(__builtin_amdgcn_readlane(len, k)); \
    if (lane == k) end = fill;
        RC_META_KEY(0, "{\"st_mode\":")
        RC_META_KEY(1, ",\"st_uid\":")
        RC_META_KEY(2, ",\"st_gid\":")
        RC_META_KEY(3, ",\"st_size\":")
        RC_META_KEY(4, ",\"st_atime_ns\":")
        RC_META_KEY(5, ",\"st_mtime_ns\":")
        RC_META_KEY(6, ",\"st_ctime_ns\":")
#undef RC_META_KEY
        put("}");
        if (lane < kSnapMetaColumns) {  // from the last digit backwards: u / 10 = (u * ceil(2^67 / 10)) >> 67
            uint64_t u = v < 0 ? uint64_t(0) - uint64_t(v) : uint64_t(v);
            do {
                const uint64_t q = __umul64hi(u, 0xCCCCCCCCCCCCCCCDull) >> 3;
                buf[--end] = uint8_t('0' + uint32_t(u - q * 10));
                u = q;
            } while (u);
            if (v < 0) buf[--end] = '-';
        }
    }

    // Q of the len bytes at src
    __device__ __forceinline__ void quoted(gcbytes src, uint64_t len) {
        put("\"");
        for (uint64_t pos = 0; pos < len; pos += kSnapTextStep) {
            step();
            const uint64_t i = pos + lane, ahead = pos + kSnapTextStep + lane;
            const uint32_t b = i < len ? uint32_t(src[i]) : 0u;
            const uint32_t e = lane < 3 && ahead < len ? uint32_t(src[ahead]) : 0u;  // the next step's first bytes
            uint32_t next[3];
#pragma unroll
            for (uint32_t k = 0; k < 3; ++k) {
                const uint32_t from = (lane + k + 1) & 63u;
                const uint32_t mine = __shfl(b, from), theirs = __shfl(e, from);
                next[k] = (lane + k + 1 < 64 ? mine : theirs) & 0x3Fu;
            }
            const uint32_t term = i < len ? rc_snap_path_term(b) : 0u;
            uint32_t total;
            uint8_t *o = buf + fill + wave_scan(term, lane, total);
            if (term == 1) {
                o[0] = uint8_t(b);
            } else if (term == 2) {
                o[0] = '\\';
                o[1] = uint8_t(b == '\b' ? 'b' : b == '\t' ? 't' : b == '\n' ? 'n' : b == '\f' ? 'f' : b == '\r' ? 'r' : b);
            } else if (term == 6) {
                const uint32_t unit = b < 0x80u   ? b
                                      : b < 0xE0u ? ((b & 0x1Fu) << 6) | next[0]
                                                  : ((b & 0x0Fu) << 12) | (next[0] << 6) | next[1];
                put_escape(o, unit);
            } else if (term == 12) {
                const uint32_t cp = ((b & 7u) << 18) | (next[0] << 12) | (next[1] << 6) | next[2];
                const uint32_t v = cp - 0x10000u;
                put_escape(o, 0xD800u | ((v >> 10) & 0x3FFu));
                put_escape(o + 6, 0xDC00u | (v & 0x3FFu));
            }
            fill += total;
        }
        step();
        put("\"");
    }
};

}  // namespace

__global__ __launch_bounds__(kSnapThreads) void rc_snap_file_text_len_kernel(SnapFileText a, uint64_t *piece_len) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t j = uint64_t(blockIdx.x) * kSnapTextWaves + wave_index();
    if (j > a.m) return;
    uint64_t fixed = j == 0 ? a.first_len : 2;  // }, or }]
    uint64_t mine = 0;
    if (j > 0) {
        const uint64_t f = file_of(a, j - 1);
        const bool unfinished = a.unfinished && a.unfinished[f];
        fixed += 10 + (unfinished ? 4 : 9 + rc_snap_chars(a.digest_bytes));
        if (a.metadata) {
            fixed += 12 + (unfinished ? 4 : kSnapMetaFixed);
            if (!unfinished && lane < kSnapMetaColumns) mine = rc_snap_int64_len(a.metadata[kSnapMetaColumns * f + lane]);
        }
    }
    if (j < a.m) {
        uint64_t s, len;
        path_of(a, file_of(a, j), s, len);
        gcbytes src = global_of(a.path_bytes) + s;
        for (uint64_t i = lane; i < len; i += 64) mine += rc_snap_path_term(src[i]);
        fixed += 8 + 2 + 11;  // {"path": the quotes ,"chunks":[
    } else {
        fixed += a.last_len;
    }
    const uint64_t sum = wave_sum(mine);
    if (lane == 0) piece_len[j] = fixed + sum;
}

__global__ __launch_bounds__(kSnapThreads) void rc_snap_file_text_kernel(SnapFileText a, const uint8_t *first,
                                                                          const uint8_t *last,
                                                                          const uint64_t *piece_off, uint8_t *text) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[kSnapTextWaves][kWaveLds];
    const uint64_t j = uint64_t(blockIdx.x) * kSnapTextWaves + wave_index();
    if (j > a.m) return;
    const uintptr_t dest = reinterpret_cast<uintptr_t>(text) + piece_off[j];
    WaveOut w;
    w.buf = lds[wave_index()];
    w.lane = threadIdx.x & 63;
    w.fill = w.lo = uint32_t(dest & 15);
    w.base = reinterpret_cast<gbytes>(dest - w.lo);
    if (j > 0) w.tail(a, file_of(a, j - 1));
    if (j == 0)
        w.copy(global_of(first), a.first_len);
    else if (j < a.m)
        w.put("},");
    else
        w.put("}]");
    if (j < a.m) {
        uint64_t s, len;
        path_of(a, file_of(a, j), s, len);
        w.step();
        w.put("{\"path\":");
        w.quoted(global_of(a.path_bytes) + s, len);
        w.put(",\"chunks\":[");
    } else {
        w.copy(global_of(last), a.last_len);
    }
    w.flush(true);
}

int rc_snap_launch_file_text_len(const SnapFileText &a, uint64_t *d_piece_len, hipStream_t st) {
    unsigned grid;
    if (int rc = grid_of(a.m + 1, kSnapTextWaves, "pieces", grid)) return rc;
    rc_snap_file_text_len_kernel<<<grid, kSnapThreads, 0, st>>>(a, d_piece_len);
    return rc::launch_status("rc_snap_file_text_len_kernel");
}

int rc_snap_launch_file_text(const SnapFileText &a, const uint8_t *d_first, const uint8_t *d_last,
                             const uint64_t *d_piece_off, uint8_t *d_text, hipStream_t st) {
    unsigned grid;
    if (int rc = grid_of(a.m + 1, kSnapTextWaves, "pieces", grid)) return rc;
    rc_snap_file_text_kernel<<<grid, kSnapThreads, 0, st>>>(a, d_first, d_last, d_piece_off, d_text);
    return rc::launch_status("rc_snap_file_text_kernel");
}
