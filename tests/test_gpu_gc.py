"""Garbage-collection planning on the device (replicat_amd/gc.py over gc.hip and index.hip)
against the restatement of replicat's clean and delete_snapshots (tests/gc_ref.py).

Runs on an MI355X only (-m gpu).  The lookup's "probe bound exhausted" answer (-2, verdict 3)
needs a table without an empty entry, which the index never has (its table has at least twice
max_names entries), so no test here reaches it."""
import ctypes
import hashlib
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():  # pragma: no cover - CPU container
    pytest.skip('needs an MI355X', allow_module_level=True)

import gc_ref  # noqa: E402
from gc_ref import DELETE, REFERENCED, TAG_MISMATCH, RefNaming  # noqa: E402
from replicat_amd import _lib  # noqa: E402
from replicat_amd.dedup import SLOT, GpuChunkIndex  # noqa: E402
from replicat_amd.gc import GpuChunkGC  # noqa: E402
from replicat_amd.naming import ChunkNaming  # noqa: E402

KEY = bytes(range(1, 65))
EMPTY = None


def digest(i, size=64):
    return hashlib.sha512(b'chunk %d' % i).digest()[:size]


def flip(b):
    return bytes([b[0] ^ 0xFF]) + b[1:]


def listing_of(ref, size, n, classes=(0, 1, 2, 3)):
    """(kept digests, n (name, tag) pairs): entry i is of class classes[i % len(classes)] --
    0 referenced with its tag, 1 unreferenced with its tag, 2 unreferenced with a wrong tag,
    3 a referenced name with a wrong tag."""
    kept, pairs = [], []
    for i in range(n):
        c = classes[i % len(classes)]
        dg = digest(i, size)
        name, tag = (bytes.fromhex(x) for x in ref.location_parts(dg))
        if c in (0, 3):
            kept.append(dg)
        pairs.append((name, flip(tag) if c in (2, 3) else tag))
    return kept, pairs


def check_sweep(gc, ref, kept, pairs):
    """One sweep against the restatement; returns the verdicts."""
    want = gc_ref.clean_verdicts_bytes(ref, [kept], pairs)
    verdict, idx = gc.sweep([p[0] for p in pairs], [p[1] for p in pairs])
    assert verdict.dtype == np.uint8 and idx.dtype == np.uint64
    assert verdict.tolist() == want
    assert idx.tolist() == [i for i, v in enumerate(want) if v == DELETE]
    assert all(a < b for a, b in zip(idx.tolist(), idx.tolist()[1:]))
    return want


@pytest.fixture(scope='module')
def keyed32():
    """One keyed planner (32-byte key and names, 64-byte digests) with the references of the
    largest listing below; smaller listings are prefixes of it."""
    ref = RefNaming(KEY[:32], 32)
    kept, pairs = listing_of(ref, 64, 65_539)
    with GpuChunkGC(ChunkNaming(KEY[:32], 32), 64, max_refs=1 << 15) as gc:
        gc.reference(kept)
        yield gc, ref, kept, pairs


@pytest.mark.parametrize('n', [0, 1, 63, 64, 65, 255, 256, 257, 65_539])
def test_sweep_sizes(keyed32, n):
    """Listing sizes around a wave and a workgroup, and 65,539: 257 workgroups, more than 256,
    so the scan of the workgroup counts runs over more than one count.  Every size sweeps
    against the same references: the verdicts of a prefix do not depend on what follows it."""
    gc, ref, kept, pairs = keyed32
    want = check_sweep(gc, ref, kept, pairs[:n])
    if n >= 4:
        assert set(want) == {REFERENCED, DELETE, TAG_MISMATCH}


@pytest.mark.parametrize('nb,keylen', itertools.product([1, 7, 8, 9, 32, 63, 64], [1, 32, 64]))
def test_sweep_name_and_key_sizes(nb, keylen):
    """Every word-masking case of a name slot, and the key lengths that fill the key block to
    different ends.  One-byte names collide by the dozen: the restatement is over sets."""
    ref = RefNaming(KEY[:keylen], nb)
    kept, pairs = listing_of(ref, 28, 300)
    with GpuChunkGC(ChunkNaming(KEY[:keylen], nb), 28, max_refs=4) as gc:
        assert gc.name_bytes == nb
        gc.reference(kept)
        check_sweep(gc, ref, kept, pairs)


@pytest.mark.parametrize('size', [1, 9, 28, 64])
def test_sweep_unkeyed(size):
    """Unkeyed: referenced only with tag == name; no tag is validated, so everything else goes."""
    ref = RefNaming()
    kept, pairs = listing_of(ref, size, 300)
    with GpuChunkGC(ChunkNaming(), size, max_refs=4) as gc:
        assert gc.name_bytes == size
        gc.reference(kept)
        want = check_sweep(gc, ref, kept, pairs)
        assert set(want) == {REFERENCED, DELETE}


@pytest.mark.parametrize('classes', [(0,), (1,), (2,), (0, 1), (0, 2), (1, 2), (3,), (0, 1, 2, 3)])
def test_sweep_verdict_classes(classes):
    """Each verdict present and absent: all-delete is (1,), none-delete (0,), (2,), (0, 2), (3,);
    a planner without any reference is (1,), (2,) and (1, 2)."""
    ref = RefNaming(KEY[:32], 64)
    kept, pairs = listing_of(ref, 64, 300, classes)
    with GpuChunkGC(ChunkNaming(KEY[:32], 64), 64, max_refs=16) as gc:
        gc.reference(kept)
        want = check_sweep(gc, ref, kept, pairs)
        expect = {c: {0: REFERENCED, 1: DELETE, 2: TAG_MISMATCH, 3: TAG_MISMATCH}[c] for c in classes}
        assert set(want) == set(expect.values())


@pytest.mark.parametrize('size', [9, 64])
def test_sweep_probe_chains(size):
    """Names that share their first 8 bytes -- one probe start -- and differ in the last byte
    only: 256 of them, every other one referenced (unkeyed, so the names are the test's own)."""
    ref = RefNaming()
    head = bytes(range(0x10, 0x10 + size - 1))
    names = [head + bytes([b]) for b in range(256)]
    kept = names[::2]
    pairs = [(n, n) for n in names] + [(n, flip(n)) for n in names[:8]]
    with GpuChunkGC(ChunkNaming(), size, max_refs=4) as gc:
        gc.reference(kept)
        want = check_sweep(gc, ref, kept, pairs)
        assert want[:4] == [REFERENCED, DELETE, REFERENCED, DELETE]


def test_sweep_one_name_two_tags():
    """The same name listed twice, with its tag and with another: referenced / skipped for a
    referenced name, deleted / skipped for an unreferenced one."""
    ref = RefNaming(KEY, 16)
    a, b = digest(1), digest(2)
    (na, ta), (nb_, tb) = [[bytes.fromhex(x) for x in ref.location_parts(v)] for v in (a, b)]
    pairs = [(na, ta), (na, flip(ta)), (nb_, flip(tb)), (nb_, tb), (na, tb), (na, ta)]
    with GpuChunkGC(ChunkNaming(KEY, 16), 64, max_refs=4) as gc:
        gc.reference([a])
        want = check_sweep(gc, ref, [a], pairs)
        assert want == [REFERENCED, TAG_MISMATCH, TAG_MISMATCH, DELETE, TAG_MISMATCH, REFERENCED]


def test_kernel_timing():
    """rc_gc_timing_*: nothing is recorded until enabled; a read returns the sums and clears."""
    ref = RefNaming(KEY[:32], 32)
    kept, pairs = listing_of(ref, 64, 300)
    with GpuChunkGC(ChunkNaming(KEY[:32], 32), 64, max_refs=512) as gc:
        gc.reference(kept[:10])
        assert gc.timing_read() == {'names_ms': 0, 'sweep_ms': 0, 'compact_ms': 0, 'sweep_calls': 0}
        gc.timing(True)
        gc.reference(kept)
        check_sweep(gc, ref, kept, pairs)
        check_sweep(gc, ref, kept, pairs[:7])
        t = gc.timing_read()
        assert t['sweep_calls'] == 2 and min(t['names_ms'], t['sweep_ms'], t['compact_ms']) > 0
        gc.timing(False)
        check_sweep(gc, ref, kept, pairs)
        assert gc.timing_read()['sweep_calls'] == 0


def test_sweep_device_form():
    """rc_gc_sweep_device on the caller's stream: junk past name_bytes in the slots does not
    count, index_base is added to the indices, the count comes back on the device."""
    nb, n, base = 7, 1000, 5_000_000_000
    ref = RefNaming(KEY[:16], nb)
    kept, pairs = listing_of(ref, 32, n)
    want = gc_ref.clean_verdicts_bytes(ref, [kept], pairs)
    rnd = np.random.default_rng(7)
    host = rnd.integers(0, 256, size=(2, n, SLOT), dtype=np.uint8)
    for i, (name, tag) in enumerate(pairs):
        host[0, i, :nb] = np.frombuffer(name, dtype=np.uint8)
        host[1, i, :nb] = np.frombuffer(tag, dtype=np.uint8)
    with GpuChunkGC(ChunkNaming(KEY[:16], nb), 32, max_refs=4) as gc:
        gc.reference(kept)
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            d_names, d_tags = torch.from_numpy(host[0]).cuda(), torch.from_numpy(host[1]).cuda()
            d_verdict = torch.full((n,), 9, dtype=torch.uint8, device='cuda')
            d_idx = torch.full((n,), -1, dtype=torch.int64, device='cuda')
            d_total = torch.full((1,), -1, dtype=torch.int64, device='cuda')
            _lib.check(_lib.lib().rc_gc_sweep_device(gc._h, n, d_names.data_ptr(), d_tags.data_ptr(), base,
                                                     d_verdict.data_ptr(), d_idx.data_ptr(),
                                                     d_total.data_ptr(), st.cuda_stream))
        st.synchronize()
        doomed = [base + i for i, v in enumerate(want) if v == DELETE]
        assert d_verdict.cpu().tolist() == want
        assert d_total.item() == len(doomed)
        assert d_idx.cpu().tolist() == doomed + [-1] * (n - len(doomed))


def u64_rows(values):
    return np.ascontiguousarray(values, dtype='<u8').view(np.uint8).reshape(-1, 8)


def test_sweep_across_host_batches():
    """More entries than one batch of the host form (2^20): the indices of the second batch
    carry its offset.  Unkeyed 8-byte names straight from numpy, so the host does no hashing."""
    n = (1 << 20) + 65
    rnd = np.random.default_rng(11)
    values = rnd.permutation(np.arange(1, 2 * n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15))[:n]
    referenced = np.zeros(n, dtype=bool)
    referenced[rnd.integers(0, n, size=n // 2)] = True
    referenced[-3:] = [True, False, True]
    names = u64_rows(values)
    tags = names.copy()
    tags[5, 0] ^= 1       # tag != name on a referenced and on an unreferenced entry
    tags[-1, 7] ^= 0x80
    referenced[5] = True
    with GpuChunkGC(ChunkNaming(), 8, max_refs=1 << 10) as gc:
        gc.reference(names[referenced])
        verdict, idx = gc.sweep(names, tags)
    want = np.where(referenced, REFERENCED, DELETE).astype(np.uint8)
    want[[5, n - 1]] = DELETE
    assert np.array_equal(verdict, want)
    assert np.array_equal(idx, np.flatnonzero(want == DELETE).astype(np.uint64))
    assert idx[-1] == n - 1 and (idx >= 1 << 20).sum() == (want[1 << 20:] == DELETE).sum() > 0


def test_reference_grows_and_repeats():
    """max_refs = 4, references added snapshot by snapshot with repeats within and across the
    calls: the planner grows by at least doubling, every digest passed takes an id, and the
    sweep sees the union."""
    ref = RefNaming(KEY[:32], 32)
    snapshots = [[digest(i) for i in (0, 1, 1, 2)], [digest(0)], [digest(i) for i in range(3, 40)] * 2, [],
                 [digest(41), digest(2)]]
    _, pairs = listing_of(ref, 64, 60, (1,))
    with GpuChunkGC(ChunkNaming(KEY[:32], 32), 64, max_refs=4) as gc:
        assert (gc.used, gc.capacity) == (0, 4)
        used, caps = 0, [4]
        for chunks in snapshots:
            gc.reference(chunks)
            used += len(chunks)
            assert gc.used == used and gc.capacity >= used
            caps.append(gc.capacity)
        assert caps[:3] == [4, 4, 8] and caps[3] == 79 and caps[-1] == 2 * 79
        kept = [x for chunks in snapshots for x in chunks]
        want = check_sweep(gc, ref, kept, pairs)
        assert want == [REFERENCED if i <= 41 and i != 40 else DELETE for i in range(60)]
        assert gc.used == used  # a sweep takes no id


@pytest.mark.parametrize('key,nb', [(None, 64), (KEY[:32], 64), (KEY, 7)], ids=['unkeyed', 'key32-64', 'key64-7'])
def test_plan_delete(key, nb):
    ref, naming = RefNaming(key, nb), ChunkNaming(key, nb)
    size = 64
    kept = [[digest(i) for i in range(0, 50, 2)], [digest(0), digest(100)]]
    deleted = [[digest(i) for i in (1, 2, 3, 1, 4, 5, 3)], [digest(i) for i in (5, 100, 7, 1, 0, 9)],
               [digest(i) for i in range(30, 330)] * 2]
    flat = [x for chunks in deleted for x in chunks]
    first = gc_ref.first_occurrences(deleted, kept)
    assert first[:5] == [digest(i) for i in (1, 3, 5, 7, 9)]
    with GpuChunkGC(naming, size, max_refs=4) as gc:
        for chunks in kept:
            gc.reference(chunks)
        idx, names, tags = gc.unreferenced(flat)
        assert idx.tolist() == [flat.index(x) for x in first]
        assert [(n.tobytes(), t.tobytes()) for n, t in zip(names, tags)] == [naming.parts(x) for x in first]
    with GpuChunkGC(naming, size, max_refs=4) as gc:
        for chunks in kept:
            gc.reference(chunks)
        plan = gc.plan_delete(flat)
        assert plan == [ref.digest_to_location(x) for x in first]
        assert set(plan) == gc_ref.delete_snapshots(ref, deleted, kept)
        assert gc.used == sum(map(len, kept)) + len(flat)
        assert gc.plan_delete(flat) == []  # they count as referenced now
    with GpuChunkGC(naming, size, max_refs=4) as gc:
        gc.reference(flat)
        assert gc.plan_delete(flat[:10]) == gc.plan_delete([]) == []  # an empty result
    with GpuChunkGC(naming, size, max_refs=4) as gc:  # no references at all
        assert gc.plan_delete(flat) == [ref.digest_to_location(x) for x in gc_ref.first_occurrences(deleted, [])]


def test_plan_delete_across_host_batches():
    """More digests than one batch (2^20), with repeats inside a batch and across the boundary:
    the first occurrence wins wherever it is."""
    n = (1 << 20) + 65
    rnd = np.random.default_rng(13)
    values = rnd.integers(1, n // 2, size=n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    values[-1] = values[0]
    values[-2] = np.uint64(12345)  # first seen in the second batch
    kept = np.unique(values[rnd.integers(0, n, size=n // 4)])
    kept = kept[kept != np.uint64(12345)]
    with GpuChunkGC(ChunkNaming(), 8, max_refs=1 << 10) as gc:
        gc.reference(u64_rows(kept))
        idx, names, tags = gc.unreferenced(u64_rows(values))
    _, first = np.unique(values, return_index=True)
    first = np.sort(first)
    first = first[~np.isin(values[first], kept)]
    assert np.array_equal(idx, first.astype(np.uint64))
    assert idx[-1] == n - 2
    assert np.array_equal(names, u64_rows(values[first])) and np.array_equal(tags, names)


class Model:
    """The index as a dict (name -> smallest id): the owner rule of test_gpu_index.py's model,
    without its table."""

    def __init__(self):
        self.owner = {}
        self.used = 0

    def add(self, names):
        first = self.used
        for k, name in enumerate(names):
            if name is not EMPTY:
                self.owner.setdefault(name, first + k)
        self.used += len(names)
        return first


def slots_of(names, nb, seed):
    """Names in 64-byte slots with junk past name_bytes (it must not count)."""
    host = np.random.default_rng(seed).integers(0, 256, size=(len(names), SLOT), dtype=np.uint8)
    for i, name in enumerate(names):
        host[i, :nb] = np.frombuffer(name, dtype=np.uint8)
    return torch.from_numpy(host).cuda()


def lookup(index, names):
    d_names = slots_of(names, index.name_bytes, len(names))
    d_owner = torch.full((len(names),), -7, dtype=torch.int64, device='cuda')
    _lib.check(_lib.lib().rc_index_lookup_device(index._h, len(names), d_names.data_ptr(), d_owner.data_ptr(),
                                                 None))
    torch.cuda.synchronize()
    return d_owner.cpu().tolist()


def resolve_names(index, names):
    """One rc_index_resolve_names_device call: (return code, id_base, owners, fresh)."""
    n = len(names)
    d_names = slots_of(names, index.name_bytes, n + 1)
    d_owner = torch.full((n,), -7, dtype=torch.int64, device='cuda')
    d_fresh = torch.full((n,), 9, dtype=torch.uint8, device='cuda')
    base = ctypes.c_uint64(777)
    rc = _lib.lib().rc_index_resolve_names_device(index._h, n, d_names.data_ptr(), ctypes.byref(base),
                                                  d_owner.data_ptr(), d_fresh.data_ptr(), None)
    torch.cuda.synchronize()
    return rc, base.value, d_owner.cpu().tolist(), d_fresh.cpu().tolist()


@pytest.mark.parametrize('nb', [1, 7, 28, 64])
def test_index_lookup_and_flat_resolve(nb):
    """Flat resolve against the dict model (repeats inside a call, across calls and from
    add_host; names that collide at one probe start); the read-only lookup in between changes
    neither `used` nor any owner a later resolve reports, and answers -1 for an absent name."""
    def name(i):
        if nb == 1:
            return bytes([i])
        return (bytes([0x0F]) + bytes(range(1, nb - 1)) + bytes([i]))[:nb]  # one probe start
    a, b, c, d, e, f, g = (name(i) for i in (0x0F, 0x1F, 0x2F, 0x3F, 0x4F, 0x5F, 0x6F))
    model = Model()
    with GpuChunkIndex(nb, 8) as index:
        assert index.add([b]) == model.add([b]) == 0
        call1 = [a, c, a, a, b]
        rc, base, owners, fresh = resolve_names(index, call1)
        assert (rc, base) == (0, model.add(call1)) and base == 1
        assert owners == [model.owner[x] for x in call1] == [1, 2, 1, 1, 0]
        assert fresh == [1, 1, 0, 0, 0]
        assert index.used == 6
        # read-only: present and absent names, twice, and `used` stays
        probe = [a, d, b, e, c, a, f]
        assert lookup(index, probe) == lookup(index, probe) == [1, -1, 0, -1, 2, 1, -1]
        assert index.used == 6
        # full: three more ids do not fit max_names = 8; nothing is enqueued, nothing changes
        rc, base, owners, fresh = resolve_names(index, [d, e, f])
        assert rc == _lib.RC_ERR_INDEX_FULL and 'index full' in _lib.last_error()
        assert (owners, fresh) == ([-7] * 3, [9] * 3) and index.used == 6
        assert lookup(index, [d, e, f, a]) == [-1, -1, -1, 1]
        # the last two ids fit; the names looked up (and refused) before are fresh now
        call2 = [d, a]
        rc, base, owners, fresh = resolve_names(index, call2)
        assert (rc, base) == (0, model.add(call2)) and base == 6
        assert owners == [6, 1] and fresh == [1, 0]
        assert resolve_names(index, [g])[0] == _lib.RC_ERR_INDEX_FULL and index.used == 8
        # growth, then everything again: the same owners, then two new names, one of them twice
        index.reserve(64)
        call3 = [a, b, c, d, e, g, e]
        rc, base, owners, fresh = resolve_names(index, call3)
        assert (rc, base) == (0, model.add(call3)) and base == 8
        assert owners == [model.owner[x] for x in call3] == [1, 0, 2, 6, 12, 13, 12]
        assert fresh == [0, 0, 0, 0, 1, 1, 0]
        assert lookup(index, [e, f, g]) == [12, -1, 13]
        assert resolve_names(index, [])[:2] == (0, 15) and index.used == model.used == 15


def test_flat_resolve_random_names():
    """20,000 random 32-byte names, ~30 % repeats, in three flat calls: owners and fresh flags
    equal the dict model; a lookup of all of them afterwards reports the same owners."""
    rnd = np.random.default_rng(20_000)
    distinct = [rnd.bytes(32) for _ in range(14_000)]
    names = distinct + [distinct[i] for i in rnd.integers(0, 14_000, size=6_000)]
    names = [names[i] for i in rnd.permutation(len(names))]
    absent = [rnd.bytes(32) for _ in range(500)]
    model = Model()
    with GpuChunkIndex(32, 20_100) as index:
        pre = distinct[:100]
        assert index.add(pre) == model.add(pre) == 0
        for part in (names[:7000], names[7000:14_000], names[14_000:]):
            rc, base, owners, fresh = resolve_names(index, part)
            assert (rc, base) == (0, model.add(part))
            assert owners == [model.owner[x] for x in part]
            assert fresh == [1 if o == base + s else 0 for s, o in enumerate(owners)]
        assert lookup(index, names[:3000] + absent) == [model.owner[x] for x in names[:3000]] + [-1] * 500
        assert index.used == model.used == 20_100


@pytest.mark.parametrize('key', [None, KEY[:32]], ids=['unkeyed', 'keyed'])
def test_plan_clean_end_to_end(key):
    """From location strings, with the entries that never reach the device mixed in: the set
    equals the restatement's, the order is the listing's."""
    nb = size = 32
    ref, naming = RefNaming(key, nb), ChunkNaming(key, nb)
    kept, pairs = listing_of(ref, size, 600)
    listing = [ref.get_chunk_location(n.hex(), t.hex()) for n, t in pairs]
    ref_locs = [loc for loc, c in zip(listing, itertools.cycle(range(4))) if c == 0]
    extra = {
        3: ref_locs[0].upper().replace('DATA', 'data'),    # upper-case duplicate of a referenced chunk
        100: ref_locs[1][:-2],                             # a name one byte short
        257: listing[1].upper().replace('DATA', 'data'),   # upper-case, unreferenced, right tag
        258: listing[2].upper().replace('DATA', 'data'),   # upper-case, wrong tag
        599: ref_locs[2] + 'ab',                           # a name one byte long
    }
    if key is None:  # the reference parses nothing here: junk and another prefix are deleted
        extra.update({0: 'data/zz', 301: 'other/00/11/22-33'})
    for pos in sorted(extra):
        listing.insert(pos, extra[pos])
    want = gc_ref.clean_verdicts(ref, [kept[:100], kept[50:]], listing)
    with GpuChunkGC(naming, size, max_refs=4) as gc:
        gc.reference(kept[:100])
        gc.reference(kept[50:])
        plan = gc.plan_clean(iter(listing))
        assert plan.to_delete == [loc for loc, v in zip(listing, want) if v == DELETE]
        assert set(plan.to_delete) == gc_ref.clean(ref, [kept], listing)
        assert (plan.referenced, plan.tag_mismatch) == (want.count(REFERENCED), want.count(TAG_MISMATCH))
        assert extra[3] in plan.to_delete and (extra[258] in plan.to_delete) == (key is None)
        assert gc.plan_clean([]) == ([], 0, 0)
        if key is not None:
            used = gc.used
            with pytest.raises(ValueError, match='other/00/11/22-33'):
                gc.plan_clean(listing + ['other/00/11/22-33'])
            assert gc.used == used
