"""The device index of chunk names (replicat_amd/dedup.py over index.hip) against a Python dict:
the owner of a name is the smallest id that carries it, whatever order the lanes arrive in.

The names are the tests' own; the chunk layout (cut slots, counts) is filled in by hand, so no
chunker kernel runs here.  Runs on an MI355X only (-m gpu)."""
import ctypes
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():  # pragma: no cover - CPU container
    pytest.skip('needs an MI355X', allow_module_level=True)

from replicat_amd import _lib, synth  # noqa: E402
from replicat_amd.chunker import GpuChunker  # noqa: E402
from replicat_amd.dedup import SLOT, GpuChunkIndex  # noqa: E402

MN, MX = 2_000, 80_000
EMPTY = None


@pytest.fixture(scope='module')
def chunker():
    ch = GpuChunker(MN, MX, synth.seeded_key(3))
    yield ch
    ch.close()


class Model:
    """The index as a dict (name -> smallest id) plus the table it implies: open addressing,
    linear probing from the name's first 8 bytes (little-endian, zero-extended), entries claimed
    in insertion order.  The device's lanes may claim entries in another order, so its layout
    can differ from this one; what the model shows is that these inputs stay far from the probe
    bound at the load the index keeps."""

    def __init__(self, max_names):
        self.owner = {}
        self.used = 0
        self.resize(max_names)

    def resize(self, max_names):
        self.entries = 16
        while self.entries < 2 * max_names:
            self.entries *= 2
        self.table = [EMPTY] * self.entries
        self.max_probe = 0
        for name in self.owner:
            self.place(name)

    def place(self, name):
        pos = int.from_bytes(name[:8], 'little') & (self.entries - 1)
        for probe in range(self.entries):
            if self.table[pos] is EMPTY:
                self.table[pos] = name
            if self.table[pos] == name:
                self.max_probe = max(self.max_probe, probe)
                return
            pos = (pos + 1) & (self.entries - 1)
        raise AssertionError('probe bound hit in the host model')

    def add(self, names):
        first = self.used
        for k, name in enumerate(names):
            if name is not None:
                self.owner.setdefault(name, first + k)
                self.place(name)
        self.used += len(names)
        return first


def layout(chunker, lens):
    total, caps = chunker.capacity(lens)
    base = np.concatenate([[0], np.cumsum(caps)[:-1]]).astype(np.int64)
    return total, [int(c) for c in caps], [int(b) for b in base]


def resolve(index, chunker, lens, counts, slot_names, stream=None):
    """One rc_index_resolve_chunks call: slot_names[s] is the name of cut slot s (None: the slot
    holds junk).  Owner and fresh start as -7 and 9, so a slot the device left alone shows.
    Returns (id_base, the device tensors of the call)."""
    total, _, _ = layout(chunker, lens)
    assert len(slot_names) == total
    nb = index.name_bytes
    rnd = random.Random(total)
    host = np.zeros((total, SLOT), dtype=np.uint8)
    for s, name in enumerate(slot_names):
        # junk past name_bytes (it must not count), and in slots without a chunk
        host[s] = np.frombuffer(rnd.randbytes(SLOT), dtype=np.uint8)
        if name is not None:
            host[s, :nb] = np.frombuffer(name, dtype=np.uint8)
    st = stream or torch.cuda.current_stream()
    with torch.cuda.stream(st):
        d_names = torch.from_numpy(host).cuda()
        d_counts = torch.tensor(counts, dtype=torch.int64).cuda()
        d_owner = torch.full((total,), -7, dtype=torch.int64, device='cuda')
        d_fresh = torch.full((total,), 9, dtype=torch.uint8, device='cuda')
        id_base = index.resolve_chunks(chunker, lens, d_counts.data_ptr(), d_names.data_ptr(),
                                       d_owner.data_ptr(), d_fresh.data_ptr(), st.cuda_stream)
    return id_base, (d_names, d_counts, d_owner, d_fresh)


def read(handles):
    _, _, d_owner, d_fresh = handles
    return d_owner.cpu().tolist(), d_fresh.cpu().tolist()


def check(model, id_base, slot_names, owners, fresh):
    assert id_base == model.add(slot_names)
    for s, name in enumerate(slot_names):
        if name is None:  # a slot without a chunk contributes nothing and gets nothing
            assert (owners[s], fresh[s]) == (-7, 9), s
        else:
            assert owners[s] == model.owner[name], (s, name.hex())
            assert fresh[s] == (1 if owners[s] == id_base + s else 0), s


def names_in_slots(caps, base, per_stream):
    """Cut-slot list of a layout from per-stream name lists."""
    out = [None] * (base[-1] + caps[-1])
    for i, names in enumerate(per_stream):
        assert len(names) <= caps[i]
        out[base[i]:base[i] + len(names)] = names
    return out


def colliding(nb, last_bytes):
    """Names that share all but their last byte and hash to the last position of a 16-entry
    table (first byte 0x?F), so that probing wraps; with one byte the name is its own hash."""
    if nb == 1:
        return [bytes([b]) for b in last_bytes]
    head = bytes([0x0F]) + bytes(range(1, nb - 1))
    return [head + bytes([b]) for b in last_bytes]


@pytest.mark.parametrize('nb', [1, 7, 28, 64])
def test_tiny_table(chunker, nb):
    """max_names = 8, a table of 16 entries: names that collide at the last position and wrap, a
    name three times in one call, across calls and from add_host; overflow on the host with the
    index unchanged; growth to 64 with the same owners; a zero and a fault count."""
    a, b, c, d, e, f = colliding(nb, [0x0F, 0x1F, 0x2F, 0x3F, 0x4F, 0x5F])
    lens2, lens3 = [999, 1500], [999, 0, 1500]  # three cut slots per stream
    total2, caps2, base2 = layout(chunker, lens2)
    total3, caps3, base3 = layout(chunker, lens3)
    assert (caps2, caps3) == ([3, 3], [3, 3, 3])
    model = Model(8)
    assert model.entries == 16
    with GpuChunkIndex(nb, 8) as index:
        assert (index.name_bytes, index.used) == (nb, 0)
        assert index.add([b]) == model.add([b]) == 0
        # call 1: a at ids 1, 3 and 4; b known from add_host; c new
        slots1 = names_in_slots(caps2, base2, [[a, c, a], [a, b]])
        id1, h1 = resolve(index, chunker, lens2, [3, 2], slots1)
        assert id1 == 1
        owners1, fresh1 = read(h1)
        check(model, id1, slots1, owners1, fresh1)
        assert owners1[:5] == [1, 2, 1, 1, 0] and fresh1[:5] == [1, 1, 0, 0, 0]
        assert model.table[15] == b and model.table[0] == a and model.table[1] == c  # wrapped
        assert index.used == 7
        # full: what would pass max_names is refused on the host, by either door, and changes nothing
        first = ctypes.c_uint64()
        two = np.frombuffer(d + e, dtype=np.uint8).copy()
        rc = _lib.lib().rc_index_add_host(index._h, 2, two.ctypes.data, ctypes.byref(first))
        assert rc == _lib.RC_ERR_INDEX_FULL and index.used == 7
        with pytest.raises(_lib.IndexFull):
            resolve(index, chunker, lens2, [3, 2], slots1)
        assert index.used == 7
        assert index.add([d]) == model.add([d]) == 7  # the 8th id still fits
        rc = _lib.lib().rc_index_add_host(index._h, 1, two.ctypes.data, ctypes.byref(first))
        assert rc == _lib.RC_ERR_INDEX_FULL and index.used == 8  # the max_names + 1-th does not
        # growth 8 -> 64, then call 1's names again: the same owners, nothing fresh
        index.reserve(64)
        model.resize(64)
        assert (index.used, index.max_names, model.entries) == (8, 64, 128)
        id2, h2 = resolve(index, chunker, lens2, [3, 2], slots1)
        owners2, fresh2 = read(h2)
        assert id2 == 8 and owners2 == owners1 and fresh2[:5] == [0] * 5
        check(model, id2, slots1, owners2, fresh2)
        # call 3: a stream with count 0 and one with the fault count (written by hand: nothing
        # faulted) contribute nothing; a, c, d known from earlier calls, e new twice, f new
        slots3 = names_in_slots(caps3, base3, [[e, a], [f, f, f], [d, e, c]])
        slots3_live = names_in_slots(caps3, base3, [[e, a], [], [d, e, c]])
        id3, h3 = resolve(index, chunker, lens3, [2, _lib.RC_COUNT_FAULT, 3], slots3)
        owners3, fresh3 = read(h3)
        check(model, id3, slots3_live, owners3, fresh3)
        assert id3 == 14 and owners3[0] == owners3[7] == 14 and (fresh3[0], fresh3[7]) == (1, 0)
        slots4 = names_in_slots(caps3, base3, [[f, f, f], [f], [f]])
        slots4_live = names_in_slots(caps3, base3, [[], [f], [f]])
        id4, h4 = resolve(index, chunker, lens3, [0, 1, 1], slots4)
        owners4, fresh4 = read(h4)
        check(model, id4, slots4_live, owners4, fresh4)
        assert owners4[3] == owners4[6] == id4 + 3  # f was never inserted by the fault-count stream
        assert index.used == model.used == 8 + total2 + 2 * total3


def test_random_names_two_streams(chunker):
    """20,000 random 64-byte names, ~30 % repeats, in three calls over two HIP streams chained
    by an event as the producer chains its batches; owners and fresh flags equal the dict model,
    and the host model of the insert loop never comes near its probe bound at load <= 0.5."""
    rnd = random.Random(20_000)
    distinct = [rnd.randbytes(64) for _ in range(14_000)]
    names = distinct + [rnd.choice(distinct) for _ in range(6_000)]
    rnd.shuffle(names)
    lens = [7_000 * MN - 1, 1, 333 * MN]  # cut slots: 6999 + 3, 3, 333 + 3
    total, caps, base = layout(chunker, lens)
    per_call = [names[:7000], names[7000:14_000], names[14_000:]]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    model = Model(3 * total + 100)
    with GpuChunkIndex(64, 3 * total + 100) as index:
        pre = rnd.sample(distinct, 100)  # what a repository listing brings
        assert index.add(pre) == model.add(pre) == 0
        calls, ev = [], None
        for k, (st, part) in enumerate(zip((s1, s2, s1), per_call)):
            split = [part[:caps[0] - 5], part[caps[0] - 5:caps[0] - 3], part[caps[0] - 3:]]
            split[2] = split[2][:caps[2]]
            slots = names_in_slots(caps, base, split)
            if ev is not None:
                st.wait_event(ev)
            id_base, h = resolve(index, chunker, lens, [len(v) for v in split], slots, stream=st)
            ev = torch.cuda.Event()
            ev.record(st)
            calls.append((id_base, slots, h))
        torch.cuda.synchronize()
        seen = 0
        for id_base, slots, h in calls:
            owners, fresh = read(h)
            GpuChunkIndex.check_owners([o for o, n in zip(owners, slots) if n is not None])
            check(model, id_base, slots, owners, fresh)
            seen += sum(n is not None for n in slots)
        assert seen > 7_000 + 7_000 + 300
        assert 2 * len(model.owner) <= model.entries  # load <= 0.5
        assert model.max_probe < 64 < model.entries   # the probe bound is never near
