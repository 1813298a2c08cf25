// snapshot_fields.hip -- the fixed text of every file of a snapshot's `data`, read back
// (include/replicat_snapshot.h, "Reading the files' text"): from the stripped text stage 4 of
// "Reading `data`" leaves on the device to the columns a SnapshotLayout holds -- path bytes and
// offsets, digest slots, the unfinished flag, the metadata integers.  The inverse of
// snapshot_text.hip, and of its shape: one WAVE per piece, kSnapTextWaves pieces per workgroup, no
// workgroup barrier, no LDS.  Run r of a call is the list of file r, and with R > 0 runs a text
// divides at the ']' positions c[0 .. R - 1] (d_run_close) into R + 1 pieces:
//     piece 0 = first + head(0)                 first = {"utc_timestamp":"S","files":[
//     piece j = ] + tail(j - 1) + }, + head(j)  head  = {"path":"Q","chunks":[
//     piece R = ] + tail(R - 1) + }] + last     tail  = ,"digest":D[,"metadata":M]
// A piece is accepted only if it is exactly this, byte for byte, with nothing left over; anything
// else stores RC_FILES_NOT_CANONICAL into its text's file status (a plain store: every wave stores
// the same value) and the host reads that text with json.loads.  A piece never reads outside its
// own bytes: its reader returns 0 behind its end, and every offset the device computed earlier
// (c, the stripped length) is clamped to the text first.
//
//   fields  the tail of file j - 1 and the head of file j.  The tail is short (under 400 bytes) and
//           a chain: the length of every number places the key behind it, so ONE LANE parses it,
//           strictly, through aligned 32-bit loads, and the wave takes over where the text is
//           regular -- the base64 of D lies at a fixed offset, so lane g decodes its g-th four
//           characters and the wave stores the 64-byte slot, zeros behind the digest included, as
//           one row.  (Sharing the seven numbers among lanes would need their places first, which
//           is the same chain.)  Whether the tail has a metadata key is compared with the tail
//           before it, found at c[j - 2] by D's two possible lengths: the chain of equalities
//           makes the key present in all files of a text or in none.  Q's bounds are known before
//           it is read -- it opens behind {"path":" and closes 12 bytes before c[j] -- so the wave
//           walks it kSnapTextStep bytes per step, one byte per lane, and sums what it decodes to.
//   scan    gc.hip's one-workgroup scan turns the lengths into d_path_off (capi_snapshot.cpp).
//   paths   one wave per file: the same walk again, and every lane writes the 0 to 4 bytes of
//           its unit at the wave's prefix sum.
//
// The walk of Q.  A backslash starts an escape exactly when the run of backslashes in front of it
// is even: over the 64 lanes of a step that is the ballot of the backslashes and carry arithmetic
// on the mask (an odd run that starts on an odd bit, added to the mask, carries out of its run),
// and the parity of a run that reaches the step's end carries into the next step.  The lane of an
// escape's backslash reads the up to eleven bytes behind it from the lanes behind it -- for the last
// lanes of a step from the first bytes of the next, loaded ahead and clamped to Q's end -- and
// judges the whole escape (rc_snap_q_escape); the byte behind the backslash and the four digits
// of a \u belong to it and add nothing, and neither does a low surrogate that a high one, six lanes
// before it, has joined.  Every other byte must be 0x20 .. 0x7e and no quote.
#include <hip/hip_runtime.h>

#include "snapshot_device.h"

namespace {

static_assert(kSnapTextStep == 64, "one byte per lane");

__device__ __forceinline__ uint64_t lane0_of(uint64_t v) {
    const uint32_t lo = uint32_t(__builtin_amdgcn_readfirstlane(int(uint32_t(v))));
    const uint32_t hi = uint32_t(__builtin_amdgcn_readfirstlane(int(uint32_t(v >> 32))));
    return uint64_t(lo) | (uint64_t(hi) << 32);
}

// One walk over Q, the bytes [qs, qe) of the text at `text`: the bytes it decodes to, or
// kSnapReject.  With kWrite they go to out[0 .. room), and nothing at or behind room.
template <bool kWrite>
__device__ __forceinline__ uint64_t walk_q(gcbytes text, uint64_t qs, uint64_t qe, uint32_t lane, gbytes out,
                                           uint64_t room) {
    const uint64_t len = qe - qs;
    gcbytes q = text + qs;
    uint64_t total = 0;
    uint64_t prev_escaped = 0, prev_u = 0, prev_pair = 0;  // the last step's carry, \u starts and joined highs
    bool bad = false;
    for (uint64_t pos = 0; pos < len; pos += kSnapTextStep) {
        const uint64_t i = pos + lane, ahead = pos + kSnapTextStep + lane;
        const bool mine = i < len;
        const uint32_t b = mine ? uint32_t(q[i]) : 0u;
        const uint32_t e = lane < 11 && ahead < len ? uint32_t(q[ahead]) : 0u;  // the next step's first bytes
        uint32_t a[12];
#pragma unroll
        for (uint32_t k = 1; k < 12; ++k) {
            const uint32_t from = (lane + k) & 63u;
            const uint32_t here = __shfl(b, from), next = __shfl(e, from);
            a[k] = lane + k < 64 ? here : next;
        }
        // which bytes an escape's backslash escapes
        const uint64_t even = 0x5555555555555555ull;
        const uint64_t backslash = __ballot(b == '\\') & ~prev_escaped;
        const uint64_t follows = (backslash << 1) | prev_escaped;
        const uint64_t odd_starts = backslash & ~even & ~follows;
        const uint64_t sum = odd_starts + backslash;
        const uint64_t carry = sum < odd_starts ? 1u : 0u;
        const uint64_t escaped = (even ^ (sum << 1)) & follows;
        prev_escaped = carry;
        const bool start = mine && b == '\\' && !((escaped >> lane) & 1u);
        SnapQEscape esc{0, 0, 0};
        if (start) esc = rc_snap_q_escape(a, len - i);
        const uint64_t u_starts = __ballot(start && esc.taken >= 6);
        const uint64_t pairs = __ballot(start && esc.taken == 12);
        const uint64_t covered = (u_starts << 2) | (u_starts << 3) | (u_starts << 4) | (u_starts << 5) | (prev_u >> 62) |
                                 (prev_u >> 61) | (prev_u >> 60) | (prev_u >> 59);
        const uint64_t joined = (pairs << 6) | (prev_pair >> 58);  // the low halves
        prev_u = u_starts;
        prev_pair = pairs;
        uint32_t count = 0;
        if (start) {
            bad |= esc.bytes == kSnapQBad;
            count = esc.bytes == kSnapQBad || ((joined >> lane) & 1u) ? 0u : esc.bytes;
        } else if (mine && !(((escaped | covered) >> lane) & 1u)) {
            bad |= b < 0x20u || b > 0x7Eu || b == '"';
            count = 1;
            esc.code = b;
        }
        uint32_t step_total;
        const uint64_t at = total + wave_scan(count, lane, step_total);
        if (kWrite) {
            for (uint32_t k = 0; k < count; ++k)
                if (at + k < room) out[at + k] = uint8_t(rc_snap_utf8_byte(esc.code, count, k));
        }
        total += step_total;
    }
    // a backslash as Q's last byte found nothing behind it and is refused above
    return __ballot(bad) ? kSnapReject : total;
}

// Where piece k of text i lies: the text's base, its stripped length, and [from, to).
struct Piece {
    gcbytes text;
    uint64_t len, from, to;
    bool ok;
};

__device__ __forceinline__ Piece piece_of(const SnapFiles &a, uint64_t i, uint64_t r0, uint64_t count, uint64_t k) {
    const SnapParseText t = a.texts[i];
    Piece p;
    p.text = reinterpret_cast<gcbytes>(reinterpret_cast<uintptr_t>(a.out) + t.out);
    p.len = a.stripped_len[i] < t.len ? a.stripped_len[i] : t.len;
    p.from = k == 0 ? 0 : a.run_close[r0 + k - 1];
    p.to = k == count ? p.len : a.run_close[r0 + k];
    p.ok = p.from <= p.to && p.to <= p.len;
    if (!p.ok) p.from = p.to = 0;
    return p;
}

// The text whose pieces (kPieces: text i has its runs + 1, from text_run_first[i] + i) or runs
// hold item q.
template <bool kPieces>
__device__ __forceinline__ uint64_t text_of(const SnapFiles &a, uint64_t q) {
    uint64_t lo = 0, hi = a.n_texts;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (a.text_run_first[mid] + (kPieces ? mid : 0) <= q)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo ? lo - 1 : 0;
}

// ,"metadata": null or the seven keys, behind D.  One lane.
__device__ __forceinline__ bool metadata(TextReader &r, uint64_t &p, bool &is_null, int64_t (&v)[kSnapMetaColumns]) {
    bool ok = literal(r, p, ",\"metadata\":");
    is_null = r.byte(p) == 'n';
    if (is_null) return ok & literal(r, p, "null");
    ok &= literal(r, p, "{\"st_mode\":");
    ok &= decimal64(r, p, v[0]);
    ok &= literal(r, p, ",\"st_uid\":");
    ok &= decimal64(r, p, v[1]);
    ok &= literal(r, p, ",\"st_gid\":");
    ok &= decimal64(r, p, v[2]);
    ok &= literal(r, p, ",\"st_size\":");
    ok &= decimal64(r, p, v[3]);
    ok &= literal(r, p, ",\"st_atime_ns\":");
    ok &= decimal64(r, p, v[4]);
    ok &= literal(r, p, ",\"st_mtime_ns\":");
    ok &= decimal64(r, p, v[5]);
    ok &= literal(r, p, ",\"st_ctime_ns\":");
    ok &= decimal64(r, p, v[6]);
    ok &= literal(r, p, "}");
    return ok;
}

}  // namespace

__global__ __launch_bounds__(kSnapThreads) void rc_snap_file_fields_kernel(
    SnapFiles a, const uint8_t *status, uint32_t digest_bytes, uint8_t *file_status, uint8_t *has_metadata,
    uint64_t *first_len, uint64_t *last_off, uint8_t *digests, uint8_t *unfinished, int64_t *metadata_rows,
    uint64_t *path_text, uint64_t *path_len) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t q = uint64_t(blockIdx.x) * kSnapTextWaves + wave_index();
    if (q >= a.runs + a.n_texts) return;
    const uint64_t i = text_of<true>(a, q);
    const uint64_t r0 = a.text_run_first[i], k = q - (r0 + i);
    const uint64_t r1 = a.text_run_first[i + 1] < a.runs ? a.text_run_first[i + 1] : a.runs;
    if (r1 < r0 || k > r1 - r0) return;  // a run count that is not stage 1's
    const uint64_t count = r1 - r0;
    if (status[i] != RC_PARTS_OK) {  // its arrays mean nothing
        if (k == 0 && lane == 0) file_status[i] = RC_FILES_NOT_CANONICAL;
        return;
    }
    if (count == 0) return;  // no file: RC_FILES_OK, and the text stays with the host
    const Piece pc = piece_of(a, i, r0, count, k);
    TextReader r{reinterpret_cast<uintptr_t>(pc.text), pc.to};
    uint64_t p = pc.from;
    bool ok = pc.ok;
    if (k > 0) {  // ] + tail(k - 1) + }, or }]
        const uint64_t f = r0 + k - 1;
        const uint32_t groups = (digest_bytes + 2) / 3, pad = (3 - digest_bytes % 3) % 3;
        ok &= literal(r, p, "],\"digest\":");
        const bool is_null = r.byte(p) == 'n';
        uint32_t triple = 0;
        if (is_null) {
            ok &= literal(r, p, "null");
        } else {
            ok &= literal(r, p, "{\"!b\":\"");
            if (lane < groups) {
                uint32_t chars = 0;
#pragma unroll
                for (uint32_t c = 0; c < 4; ++c) chars |= r.byte(p + 4 * lane + c) << (8 * c);
                bool bad = false;
                triple = b64_group(chars, lane == groups - 1 ? pad : 0u, bad);
                ok &= !bad;
            }
            p += 4 * groups;
            ok &= literal(r, p, "\"}");
        }
        // byte `lane` of the slot: byte lane % 3 of group lane / 3, zero behind the digest
        const uint32_t mine = __shfl(triple, lane / 3) >> (8 * (2 - lane % 3));
        digests[RC_DIGEST_SLOT * f + lane] = uint8_t(!is_null && lane < digest_bytes ? mine & 255u : 0u);
        bool has_meta = false;
        if (lane == 0) {
            int64_t v[kSnapMetaColumns] = {0, 0, 0, 0, 0, 0, 0};
            has_meta = r.byte(p) == ',';
            if (has_meta) {
                bool meta_null;
                ok &= metadata(r, p, meta_null, v);
                ok &= meta_null == is_null;  // the writer's one flag
                if (meta_null)
                    for (uint32_t c = 0; c < kSnapMetaColumns; ++c) v[c] = 0;
            }
            ok &= k < count ? literal(r, p, "},") : literal(r, p, "}]");
            if (k >= 2) {  // the tail before this one has the key as well, or has not either
                TextReader before{reinterpret_cast<uintptr_t>(pc.text), pc.from};
                const uint64_t c2 = a.run_close[r0 + k - 2];
                const uint64_t d_len = before.byte(c2 + 11) == 'n' ? 4 : 9 + 4 * groups;
                ok &= (before.byte(c2 + 11 + d_len) == ',') == has_meta;
            } else {
                has_metadata[i] = has_meta ? 1 : 0;
            }
            for (uint32_t c = 0; c < kSnapMetaColumns; ++c) metadata_rows[kSnapMetaColumns * f + c] = v[c];
            unfinished[f] = is_null ? 1 : 0;
            if (k == count) last_off[i] = p;
        }
        p = lane0_of(p);
    }
    if (k == 0 && lane == 0) {  // first: the string's contents are the host's
        ok &= literal(r, p, "{\"utc_timestamp\":\"");
        uint32_t c = r.byte(p);
        while (c != '"' && p < pc.to && p < kSnapFirstMost) {
            p += c == '\\' ? 2 : 1;
            c = r.byte(p);
        }
        ok &= literal(r, p, "\",\"files\":[");
        ok &= p <= kSnapFirstMost;  // first itself, its last byte included, is at most that long
        first_len[i] = p;
    }
    if (k < count) {  // head(k)
        p = lane0_of(p);
        const uint64_t f = r0 + k;
        const uint64_t qs = p + 9;
        if (lane == 0) ok &= literal(r, p, "{\"path\":\"");
        uint64_t decoded = 0;
        if (qs + 12 <= pc.to) {
            uint64_t qe = pc.to - 12;
            if (lane == 0) ok &= literal(r, qe, "\",\"chunks\":[");
            decoded = walk_q<false>(pc.text, qs, pc.to - 12, lane, nullptr, 0);
            ok &= decoded != kSnapReject;
            if (decoded == kSnapReject) decoded = 0;
        } else {
            ok = false;
        }
        if (lane == 0) {
            path_text[f] = qs;
            path_len[f] = decoded;
        }
    }
    if (__ballot(!ok) && lane == 0) file_status[i] = RC_FILES_NOT_CANONICAL;
}

__global__ __launch_bounds__(kSnapThreads) void rc_snap_file_paths_kernel(SnapFiles a, const uint8_t *file_status,
                                                                           const uint64_t *path_text,
                                                                           const uint64_t *path_off, uint8_t *path_bytes,
                                                                           uint64_t path_room) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t f = uint64_t(blockIdx.x) * kSnapTextWaves + wave_index();
    if (f >= a.runs) return;
    const uint64_t i = text_of<false>(a, f);
    if (file_status[i] != RC_FILES_OK) return;
    const uint64_t r0 = a.text_run_first[i];
    const uint64_t r1 = a.text_run_first[i + 1] < a.runs ? a.text_run_first[i + 1] : a.runs;
    if (f < r0 || f >= r1) return;
    const Piece pc = piece_of(a, i, r0, r1 - r0, f - r0);
    const uint64_t qs = path_text[f], at = path_off[f];
    if (!pc.ok || qs < pc.from || qs + 12 > pc.to || at > path_room) return;  // cannot happen in an accepted text
    gbytes out = reinterpret_cast<gbytes>(reinterpret_cast<uintptr_t>(path_bytes) + at);
    walk_q<true>(pc.text, qs, pc.to - 12, lane, out, path_room - at);
}

int rc_snap_launch_file_fields(const SnapFiles &a, const uint8_t *d_status, uint32_t digest_bytes,
                               uint8_t *d_file_status, uint8_t *d_has_metadata, uint64_t *d_first_len,
                               uint64_t *d_last_off, uint8_t *d_digests, uint8_t *d_unfinished, int64_t *d_metadata,
                               uint64_t *d_path_text, uint64_t *d_path_len, hipStream_t st) {
    unsigned grid;
    if (int rc = grid_of(a.runs + a.n_texts, kSnapTextWaves, "pieces", grid)) return rc;
    if (!grid) return 0;
    rc_snap_file_fields_kernel<<<grid, kSnapThreads, 0, st>>>(a, d_status, digest_bytes, d_file_status, d_has_metadata,
                                                              d_first_len, d_last_off, d_digests, d_unfinished,
                                                              d_metadata, d_path_text, d_path_len);
    return rc::launch_status("rc_snap_file_fields_kernel");
}

int rc_snap_launch_file_paths(const SnapFiles &a, const uint8_t *d_file_status, const uint64_t *d_path_text,
                              const uint64_t *d_path_off, uint8_t *d_path_bytes, uint64_t path_room, hipStream_t st) {
    unsigned grid;
    if (int rc = grid_of(a.runs, kSnapTextWaves, "files", grid)) return rc;
    if (!grid) return 0;
    rc_snap_file_paths_kernel<<<grid, kSnapThreads, 0, st>>>(a, d_file_status, d_path_text, d_path_off, d_path_bytes,
                                                             path_room);
    return rc::launch_status("rc_snap_file_paths_kernel");
}
