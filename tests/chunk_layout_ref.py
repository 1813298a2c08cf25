"""Hand-written chunk layouts of more than 1,024 streams, and what every per-chunk stage must make
of them (numpy and hashlib only).

Every entry point that takes a chunk layout (layout, n, lens, d_counts) hands its streams to
workgroups in runs of spw = ceil(n / 1024) streams (rc_b2_streams_per_group, digest_kernels.h),
and the ones that scan the counts give each of 1,024 threads per = ceil(n / 1024) streams
(rc_b2_scan_kernel).  `partition` restates that; `make_layout` writes the cuts and counts of n
streams so that every corner of those loops is met (tests/test_chunk_layout_ref.py asserts each
property; tests/test_gpu_many_streams.py runs the stages over it).  No chunker runs: a layout is
chosen, not found."""
import hashlib
import random

import numpy as np

RC_COUNT_OVERFLOW = -1  # include/replicat_chunker.h
RC_COUNT_FAULT = -3
NOT_SELECTED = (1 << 64) - 1
JUNK = 1 << 63  # a cut slot without a chunk holds JUNK + slot
TILE = 1024     # cut slots per tile of the select passes (gcm.hip kSelectTile)

# The smallest counts at which each thing first happens: spw = 1 (the control); spw = 2 with a
# last run of one stream and scan threads that own nothing; 1,024 runs, the last of one stream;
# spw = 3; spw = 4 with a last run of one stream
STREAM_COUNTS = [1024, 1025, 2047, 2049, 3073]

SPECIAL_LENGTHS = (0, 1, 63, 64, 65, 127, 128)
MAX_LENGTH = 1500

HASHES = {'sha2-256': hashlib.sha256, 'sha2-512': hashlib.sha512,
          'sha3-256': hashlib.sha3_256, 'sha3-512': hashlib.sha3_512}


def partition(n):
    """(spw, groups, streams_in_last_group, per) of a call over n streams: workgroup g of the
    work-list kernels takes streams [g spw, min((g + 1) spw, n)), thread t of the scan
    [t per, min((t + 1) per, n))."""
    spw = (n + 1023) // 1024 if n else 1
    groups = (n + spw - 1) // spw
    return spw, groups, n - (groups - 1) * spw, (n + 1023) // 1024


def up16(x):
    return (x + 15) & ~15


class Layout:
    """n streams in one arena with their cut slots: lens, offsets (of each stream in arena, 16-byte
    aligned), arena (uint8), caps, cut_base, total (cut slots), counts (int64) and cuts (uint64,
    chunk END offsets; JUNK + slot where no chunk is)."""

    def runs(self):
        """(first stream, one past the last) of every workgroup's run."""
        spw, groups, _, _ = partition(self.n)
        return [(g * spw, min((g + 1) * spw, self.n)) for g in range(groups)]

    def live(self):
        """(stream, k, cut slot, start, end) of every chunk, in cut-slot order."""
        out = []
        for i in range(self.n):
            b, prev = int(self.cut_base[i]), 0
            for k in range(max(int(self.counts[i]), 0)):
                e = int(self.cuts[b + k])
                out.append((i, k, b + k, prev, e))
                prev = e
        return out

    def live_mask(self):
        mask = np.zeros(self.total, dtype=bool)
        for i in range(self.n):
            b = int(self.cut_base[i])
            mask[b:b + max(int(self.counts[i]), 0)] = True
        return mask

    def stream(self, i):
        o = int(self.offsets[i])
        return self.arena[o:o + int(self.lens[i])].tobytes()


def make_layout(n, seed, min_length=64):
    """A layout of n >= 1,024 streams (see the module text and the properties
    tests/test_chunk_layout_ref.py lists); the same (n, seed) gives the same layout."""
    assert n >= 1024 and min_length % 4 == 0
    rnd = random.Random(1000 * n + seed)
    spw, groups, last_n, _ = partition(n)
    mid, end = (spw - 1) // 2, spw - 1  # a place inside a run that is not its last (spw > 1), and its last
    # a third of the random lengths below 600: about 11.5 cut slots a stream, 35,000 for 3,073
    lens = [rnd.choice(SPECIAL_LENGTHS) if rnd.random() < 0.07 else
            rnd.randrange(rnd.choice((600, MAX_LENGTH + 1, MAX_LENGTH + 1))) for _ in range(n)]
    # counts written by hand: >= 0 taken below from the length, negative ones as they are
    forced = {}
    for frac, place, value in ((1, mid, RC_COUNT_OVERFLOW), (2, end, RC_COUNT_OVERFLOW),
                               (3, mid, RC_COUNT_FAULT), (4, end, RC_COUNT_FAULT)):
        forced[(frac * groups // 5) * spw + place] = value
    t = (groups // 2) * spw  # three streams in a row without a chunk, the first of them empty
    forced.update({t: 0, t + 1: RC_COUNT_OVERFLOW, t + 2: 0})
    lens[t] = 0
    for i in forced:
        if i != t:
            lens[i] = rnd.randrange(129, MAX_LENGTH + 1)  # the bytes are there, the chunks are not
    first_of_last = (groups - 1) * spw
    for i in [0, *range(first_of_last, n)]:  # stream 0 and the last run have chunks
        lens[i] = rnd.randrange(129, MAX_LENGTH + 1)
    lens[1], lens[2] = 1, rnd.randrange(300, MAX_LENGTH + 1)  # a one-byte stream; a one-byte chunk below
    # the select passes work in tiles of TILE cut slots: the first tile boundary falls between two
    # streams (earlier streams give up a cut slot each until it does) ...
    cap_of = lambda L: L // min_length + 3  # noqa: E731
    acc, j = 0, 0
    while acc < TILE:
        acc += cap_of(lens[j])
        j += 1
    for i in range(3, j):
        if acc > TILE and lens[i] >= min_length and i not in forced:
            lens[i] -= min_length
            acc -= 1
    assert acc == TILE
    # ... and a later one inside a stream whose every cut slot holds a chunk
    full, base = None, 0
    for i, L in enumerate(lens):
        cap = cap_of(L)
        if base > TILE and base // TILE != (base + cap - 1) // TILE and base % TILE and \
                L >= cap and i not in forced and i < first_of_last:
            full = i
            break
        base += cap
    assert full is not None

    lay = Layout()
    lay.n, lay.min_length = n, min_length
    lay.lens = np.array(lens, dtype=np.uint64)
    lay.caps = np.array([L // min_length + 3 for L in lens], dtype=np.uint64)
    lay.cut_base = np.concatenate([[0], np.cumsum(lay.caps)[:-1]]).astype(np.uint64)
    lay.total = int(lay.caps.sum())
    offsets, acc = [], 0
    for L in lens:
        offsets.append(acc)
        acc = up16(acc + L)
    lay.offsets = np.array(offsets, dtype=np.uint64)
    lay.arena = np.frombuffer(rnd.randbytes(acc + 16), dtype=np.uint8).copy()
    lay.counts = np.zeros(n, dtype=np.int64)
    lay.cuts = (JUNK + np.arange(lay.total, dtype=np.uint64)).astype(np.uint64)
    for i, L in enumerate(lens):
        cap = int(lay.caps[i])
        most = min(cap, L)  # a chunk has at least one byte
        if i in forced:
            count = forced[i]
        elif most == 0:
            count = 0
        else:
            r = rnd.random()
            count = most if r < 0.2 or i in (first_of_last, full) else 1 if r < 0.3 else rnd.randint(1, most)
        if i == 2:
            count = max(count, 2)
        lay.counts[i] = count
        if count > 0:
            inner = rnd.sample(range(1, L), count - 1)
            if i == 2 and 1 not in inner:
                inner[0] = 1
            b = int(lay.cut_base[i])
            lay.cuts[b:b + count] = sorted(inner) + [L]
    return lay


def assert_layout(lay):
    """Every property the many-stream tests rely on; a test calls this before it trusts a layout."""
    n, counts, caps, base, lens = lay.n, lay.counts, lay.caps.astype(np.int64), lay.cut_base, lay.lens
    spw, groups, last_n, per = partition(n)
    runs = lay.runs()
    assert len(runs) == groups and runs[-1] == (n - last_n, n) and all(b - a == spw for a, b in runs[:-1])
    assert caps.tolist() == [int(L) // lay.min_length + 3 for L in lens]
    assert caps.min() == 3 and 20 <= caps.max() <= MAX_LENGTH // lay.min_length + 3
    assert base.tolist() == [int(x) for x in np.concatenate([[0], np.cumsum(caps)[:-1]])]
    assert lay.total == int(caps.sum()) == len(lay.cuts)
    assert (lay.offsets % 16 == 0).all() and (np.diff(lay.offsets.astype(np.int64)) >= lens[:-1]).all()
    assert int(lay.offsets[-1] + lens[-1]) + 16 <= len(lay.arena)
    assert set(SPECIAL_LENGTHS) <= set(lens.tolist()) and lens.max() > 1400
    # counts: 0, 1, a full stream, the values in between; nothing above the capacity
    assert (counts <= caps).all() and set(counts[counts < 0].tolist()) == {RC_COUNT_OVERFLOW, RC_COUNT_FAULT}
    assert (counts == 0).any() and (counts == 1).any() and ((counts == caps) & (caps > 3)).any()
    assert ((counts > 1) & (counts < caps)).any()
    # each negative count inside a full run (not its last stream, where a run has several) and as
    # the last stream of a full run
    place = {(int(c), 'last' if i == b - 1 else 'inside') for a, b in runs[:-1] for i, c in
             zip(range(a, b), counts[a:b]) if c < 0}
    want = {(RC_COUNT_OVERFLOW, 'last'), (RC_COUNT_FAULT, 'last')}
    assert place >= (want | {(RC_COUNT_OVERFLOW, 'inside'), (RC_COUNT_FAULT, 'inside')} if spw > 1 else want)
    a, b = runs[-1]
    assert (counts[a:b] > 0).all() and (counts[a:b] == caps[a:b]).any()
    assert counts[0] > 0 and counts[n - 1] > 0
    dead = counts <= 0
    assert (dead[:-2] & dead[1:-1] & dead[2:]).any()
    assert ((lens == 0) & (counts == 0)).any() and ((lens > 0) & (counts == 0)).any()
    # the cuts: increasing, the last chunk ends its stream, junk wherever no chunk is
    live, mask = lay.live(), lay.live_mask()
    assert all(a < e for _, _, _, a, e in live) and len(live) == int(counts[counts > 0].sum()) == int(mask.sum())
    assert all(int(lay.cuts[int(base[i]) + int(counts[i]) - 1]) == int(lens[i]) for i in range(n) if counts[i] > 0)
    slots = np.arange(lay.total, dtype=np.uint64)
    assert (lay.cuts[~mask] == JUNK + slots[~mask]).all() and (lay.cuts[mask] <= MAX_LENGTH).all()
    sizes = {e - a for _, _, _, a, e in live}
    assert 1 in sizes and any(k == 0 and e == int(lens[i]) and e > 1 for i, k, _, _, e in live)
    assert min(sizes) <= 200 < max(sizes)  # a lane / quad split at 200 bytes has both sides
    assert {(int(lay.offsets[i]) + a) % 4 for i, _, _, a, _ in live} == {0, 1, 2, 3}
    # tiles of the select passes: a boundary between two streams, another inside a stream's chunks
    tiles = (lay.total + TILE - 1) // TILE
    assert tiles > 10 * (n // 1024)
    bounds = range(TILE, lay.total, TILE)
    assert any(b in set(base.tolist()) for b in bounds)
    assert any(mask[b - 1] and mask[b] and b not in set(base.tolist()) for b in bounds)


# ------------------------------------------------------------------------ expected results

def chunks(lay):
    """cut slot -> the chunk's bytes."""
    return {s: lay.arena[int(lay.offsets[i]) + a:int(lay.offsets[i]) + e].tobytes()
            for i, _, s, a, e in lay.live()}


def digests(lay, name, size=None):
    """cut slot -> digest: name is 'blake2b' (size: the digest size) or a key of HASHES."""
    if name == 'blake2b':
        return {s: hashlib.blake2b(c, digest_size=size).digest() for s, c in chunks(lay).items()}
    return {s: HASHES[name](c).digest() for s, c in chunks(lay).items()}


def subkeys(slot_digests, shared, salt, key_bytes):
    """cut slot -> derive_shared_subkey(digest): hashlib.blake2b(digest, salt=, key=,
    digest_size=key bytes), as tests/test_gpu_chacha.py::test_chunk_path computes them."""
    return {s: hashlib.blake2b(d, salt=salt, key=shared, digest_size=key_bytes).digest()
            for s, d in slot_digests.items()}


def region_bases(lay, over):
    """The per-stream bases of the unfiltered cipher path's output and its size
    (rc_gcm_chunks_layout: 16-byte aligned regions with room for `over` = nonce + tag bytes per cut
    slot)."""
    base, acc = [], 0
    for L, cap in zip(lay.lens.tolist(), lay.caps.tolist()):
        base.append(acc)
        acc = up16(acc + L + cap * over)
    return acc, base


def blob_offsets(lay, out_base, over):
    """cut slot -> (offset, length) of its blob on the unfiltered cipher path: chunk k of stream
    i, cut range [s, e), lies at out_base[i] + s + k * over (include/replicat_cipher.h)."""
    return {s: (int(out_base[i]) + a + k * over, e - a + over) for i, k, s, a, e in lay.live()}


def select_expect(lay, select, over):
    """(blob_off per cut slot, [bytes, blobs], {cut slot: (offset, length)}) of the select path:
    the selected chunks back to back in cut-slot order (the host loop of
    tests/test_gpu_encrypt_select.py::run_case)."""
    off, acc, picked = [NOT_SELECTED] * lay.total, 0, {}
    for _, _, s, a, e in lay.live():
        if select[s]:
            off[s] = acc
            picked[s] = (acc, e - a + over)
            acc += e - a + over
    return off, [acc, len(picked)], picked


def selections(lay):
    """name -> select byte per cut slot."""
    live = [s for _, _, s, _, _ in lay.live()]
    every = np.ones(lay.total, dtype=np.uint8)  # also on slots without a chunk: they must not count
    alt = np.zeros(lay.total, dtype=np.uint8)
    alt[live[::2]] = 7  # any non-zero byte selects
    last = np.zeros(lay.total, dtype=np.uint8)
    last[[int(lay.cut_base[i]) + int(c) - 1 for i, c in enumerate(lay.counts) if c > 0]] = 1
    return {'all': every, 'alternating': alt, 'one_per_stream': last,
            'none': np.zeros(lay.total, dtype=np.uint8)}


def neighbours_of_dead(lay):
    """Streams with chunks next to a stream without."""
    c = lay.counts
    return [i for i in range(lay.n) if c[i] > 0 and
            ((i > 0 and c[i - 1] <= 0) or (i + 1 < lay.n and c[i + 1] <= 0))]
