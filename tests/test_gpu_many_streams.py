"""The per-chunk stages with more than 1,024 streams in a call: every entry point that takes a
chunk layout hands its streams to workgroups in runs of spw = ceil(n / 1024) streams and scans the
counts in ranges of as many, so only above 1,024 streams do the run loops, their clamp at n, the
carried chunk offsets and the bucket-major histogram do more than one trivial step.

The layouts are written by hand (tests/chunk_layout_ref.py: counts of 0, -1, -3, 1 and a full
stream inside and at the end of runs, a last run of one stream, junk in every slot without a
chunk); no chunker kernel runs, a GpuChunker is only the `layout` argument.  Every output buffer is
prefilled and must keep the fill wherever no chunk is.  Expected values: hashlib, the oracle's
AES-GCM (every blob), tests/chacha_ref.py (a sample that holds every chunk of the first run, the
last two runs and every stream next to one without chunks) and, for every ChaCha20-Poly1305 blob,
the same entry point over the same streams in calls of at most 1,024 streams, the regime the other
tests pin.  Runs on an MI355X only (-m gpu)."""
import random
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():  # pragma: no cover - CPU container
    pytest.skip('needs an MI355X', allow_module_level=True)

import chacha_ref  # noqa: E402
import chunk_layout_ref as R  # noqa: E402
import test_gpu_index as I  # noqa: E402,N811

from replicat_amd import synth  # noqa: E402
from replicat_amd.chunker import GpuChunker  # noqa: E402
from replicat_amd.cipher import GpuAesGcm, GpuChaCha20Poly1305  # noqa: E402
from replicat_amd.dedup import GpuChunkIndex  # noqa: E402
from replicat_amd.hashing import SLOT, GpuBlake2b, GpuSha2, GpuSha3, state_init  # noqa: E402

FILL = 0xA5
OVER = 28      # nonce (12) + tag (16) bytes per blob, both families
SMALL = 1024   # streams per call of the regime the other tests pin
_STATE = {}


def dev(data):
    return torch.from_numpy(np.frombuffer(bytes(data), dtype=np.uint8).copy()).cuda()


def hs():
    return torch.cuda.current_stream().cuda_stream


def state(n):
    """The layout of n streams on the device, once per module run: arena, cuts, counts, a key and
    a nonce per cut slot (random everywhere, so also junk where no chunk is), and the memo of
    expected values."""
    if n not in _STATE:
        lay = R.make_layout(n, 1)
        R.assert_layout(lay)
        ch = GpuChunker(lay.min_length, 2048, synth.seeded_key(3))
        total, caps = ch.capacity(lay.lens)
        assert total == lay.total and (caps == lay.caps).all()
        rnd = random.Random(n)
        arena = torch.from_numpy(lay.arena).cuda()
        st = SimpleNamespace(n=n, lay=lay, ch=ch, arena=arena, total=total,
                             ptrs=[arena.data_ptr() + int(o) for o in lay.offsets],
                             lens=[int(v) for v in lay.lens], live=lay.live(), mask=lay.live_mask(),
                             cuts=torch.from_numpy(lay.cuts.view(np.int64)).cuda(),
                             counts=torch.from_numpy(lay.counts).cuda(), chunks=R.chunks(lay),
                             keys_h=np.frombuffer(rnd.randbytes(total * SLOT), dtype=np.uint8).reshape(total, SLOT),
                             nonces_h=rnd.randbytes(total * 12), memo={})
        st.keys, st.nonces = dev(st.keys_h.tobytes()), dev(st.nonces_h)
        assert st.ptrs[0] % 16 == 0
        _STATE[n] = st
    return _STATE[n]


@pytest.fixture(scope='module', autouse=True)
def release():
    yield
    for st in _STATE.values():
        st.ch.close()
    _STATE.clear()
    torch.cuda.empty_cache()


def memo(st, key, make):
    if key not in st.memo:
        st.memo[key] = make()
    return st.memo[key]


def check_slots(got, want, size):
    """got: (cut slots, 64) bytes off the device; want: cut slot -> the first `size` bytes of its
    slot.  The rest of such a slot is zero, and every other slot keeps the fill."""
    exp = np.full(got.shape, FILL, dtype=np.uint8)
    for s, d in want.items():
        assert len(d) == size
        exp[s, :size] = np.frombuffer(d, dtype=np.uint8)
        exp[s, size:] = 0
    bad = (got != exp).any(axis=1).nonzero()[0]
    assert not len(bad), (len(bad), bad[:8].tolist(), [s in want for s in bad[:8].tolist()])


def check_bytes(out_h, placed, blobs):
    """out_h holds blobs[s] at placed[s] = (offset, length) for every s of placed, and the fill
    everywhere else."""
    exp = np.full(out_h.shape, FILL, dtype=np.uint8)
    for s, (o, length) in placed.items():
        assert len(blobs[s]) == length and o + length <= len(exp)
        exp[o:o + length] = np.frombuffer(blobs[s], dtype=np.uint8)
    bad = (out_h != exp).nonzero()[0]
    if len(bad):
        first = int(bad[0])
        owner = [s for s, (o, length) in placed.items() if o <= first < o + length]
        raise AssertionError((len(bad), first, owner))


# ------------------------------------------------------------------------- digests

B2_SPLITS = {'default': (None, None), 'all_lanes': (str(1 << 40), '1'), 'mixed': ('200', '1')}


@pytest.mark.parametrize('split', sorted(B2_SPLITS))
@pytest.mark.parametrize('n,size', [(n, 64) for n in R.STREAM_COUNTS] + [(2049, 20)])
def test_blake2b_chunk_digests(monkeypatch, n, size, split):
    """GpuBlake2b.digest_chunks = hashlib at every live slot, under the default split (every item
    by quads here), every item by the lane kernel, and lanes up to 200 bytes with quads above
    (chunk_layout_ref.assert_layout: the chunk lengths lie on both sides)."""
    for name, value in zip(('RC_B2_LANE_MAX', 'RC_B2_LANE_ONLY'), B2_SPLITS[split]):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)
    st = state(n)
    h = GpuBlake2b(length=size)  # the knobs are read when a hasher is created
    dig = torch.full((st.total, SLOT), FILL, dtype=torch.uint8, device='cuda')
    h.digest_chunks(st.ch, st.ptrs, st.lens, st.cuts.data_ptr(), st.counts.data_ptr(), dig.data_ptr(), hs())
    torch.cuda.synchronize()
    check_slots(dig.cpu().numpy(), memo(st, ('blake2b', size), lambda: R.digests(st.lay, 'blake2b', size)), size)
    h.close()


SHA = {'sha2-256': (GpuSha2, 256), 'sha2-512': (GpuSha2, 512), 'sha3-256': (GpuSha3, 256),
       'sha3-512': (GpuSha3, 512)}
SHA_FORMS = {'lane': str(1 << 62), 'latency': '0'}  # RC_SHA_LANE_MAX, as tests/test_gpu_sha.py


@pytest.mark.parametrize('form', sorted(SHA_FORMS))
@pytest.mark.parametrize('name', sorted(SHA))
@pytest.mark.parametrize('n', [1025, 3073])
def test_sha_chunk_digests(monkeypatch, n, name, form):
    """rc_hash_chunks of a SHA-2 / SHA-3 hasher = hashlib at every live slot, every chunk by the
    lane form and again by the latency form."""
    monkeypatch.setenv('RC_SHA_LANE_MAX', SHA_FORMS[form])
    st = state(n)
    cls, bits = SHA[name]
    h = cls(bits=bits)  # the knob is read when a hasher is created
    dig = torch.full((st.total, SLOT), FILL, dtype=torch.uint8, device='cuda')
    h.digest_chunks(st.ch, st.ptrs, st.lens, st.cuts.data_ptr(), st.counts.data_ptr(), dig.data_ptr(), hs())
    torch.cuda.synchronize()
    check_slots(dig.cpu().numpy(), memo(st, name, lambda: R.digests(st.lay, name)), bits // 8)
    h.close()


@pytest.mark.parametrize('key_bytes', [32, 16])
@pytest.mark.parametrize('n', R.STREAM_COUNTS)
def test_subkeys(n, key_bytes):
    """derive_chunks over digest slots the test uploads (hashlib's digests where a chunk is, junk
    elsewhere) = hashlib.blake2b(digest, salt=, key=, digest_size=key bytes) at every live slot;
    every other key slot untouched."""
    st = state(n)
    rnd = random.Random(n + key_bytes)
    d64 = memo(st, ('blake2b', 64), lambda: R.digests(st.lay, 'blake2b', 64))
    dig_h = np.frombuffer(rnd.randbytes(st.total * SLOT), dtype=np.uint8).reshape(st.total, SLOT).copy()
    for s, d in d64.items():
        dig_h[s] = np.frombuffer(d, dtype=np.uint8)
    shared, salt = rnd.randbytes(32), rnd.randbytes(16)
    kdf = dev(state_init(key_bytes, key=shared, salt=salt))
    dig = torch.from_numpy(dig_h).cuda()
    keys = torch.full((st.total, SLOT), FILL, dtype=torch.uint8, device='cuda')
    h = GpuBlake2b(length=64)
    h.derive_chunks(st.ch, st.lens, st.counts.data_ptr(), kdf.data_ptr(), dig.data_ptr(), keys.data_ptr(), hs())
    torch.cuda.synchronize()
    check_slots(keys.cpu().numpy(), R.subkeys(d64, shared, salt, key_bytes), key_bytes)
    assert np.array_equal(dig.cpu().numpy(), dig_h)
    h.close()


# ------------------------------------------------------------------------- ciphers

def cipher_of(family, key_bits=256):
    return GpuChaCha20Poly1305() if family == 'chacha' else GpuAesGcm(key_bits=key_bits)


def slot_nonce(st, s):
    return st.nonces_h[12 * s:12 * s + 12]


def gcm_blobs(st, oracle, key_bits):
    """cut slot -> nonce || C || T by the oracle's AES-GCM, every chunk."""
    kb = key_bits // 8
    return memo(st, ('gcm', key_bits), lambda: {
        s: slot_nonce(st, s) + oracle.gcm_encrypt(st.keys_h[s, :kb].tobytes(), slot_nonce(st, s), c)
        for s, c in st.chunks.items()})


def chacha_sample(st):
    """The cut slots chacha_ref seals: every chunk of the first run of streams, of the last two
    runs and of every stream next to one without chunks, and 40 more."""
    def make():
        runs = st.lay.runs()
        must = {i for a, b in (runs[0], runs[-2], runs[-1]) for i in range(a, b)}
        must |= set(R.neighbours_of_dead(st.lay))
        slots = [s for i, _, s, _, _ in st.live if i in must]
        rest = [s for i, _, s, _, _ in st.live if i not in must]
        slots += random.Random(st.n).sample(rest, 40)
        assert len(must) >= 3 and len(slots) <= 1200
        return {s: slot_nonce(st, s) + chacha_ref.seal(st.keys_h[s, :32].tobytes(), slot_nonce(st, s),
                                                       st.chunks[s]) for s in slots}
    return memo(st, 'chacha', make)


def small_calls(st):
    """(first stream, one past the last, first cut slot) of calls of at most SMALL streams."""
    return [(a, min(a + SMALL, st.n), int(st.lay.cut_base[a])) for a in range(0, st.n, SMALL)]


def small_call_blobs(st, g, select_h=None):
    """cut slot -> blob as the entry point (encrypt_chunks, or encrypt_chunks_select with this
    selection) writes it for the same streams in calls of at most SMALL streams each."""
    out = {}
    for a, b, s0 in small_calls(st):
        lens = st.lens[a:b]
        total, base = g.chunks_layout(st.ch, lens)
        buf = torch.full((total,), FILL, dtype=torch.uint8, device='cuda')
        args = (st.ch, st.ptrs[a:b], lens, st.cuts.data_ptr() + 8 * s0, st.counts.data_ptr() + 8 * a,
                st.keys.data_ptr() + SLOT * s0, st.nonces.data_ptr() + 12 * s0)
        live = [(i, k, s, x, e) for i, k, s, x, e in st.live if a <= i < b]
        if select_h is None:
            g.encrypt_chunks(*args, buf.data_ptr(), hs())
            torch.cuda.synchronize()
            where = {s: int(base[i - a]) + x + k * OVER for i, k, s, x, e in live}
        else:
            slots = int(st.lay.caps[a:b].sum())
            sel = torch.from_numpy(select_h[s0:s0 + slots].copy()).cuda()
            off = torch.zeros(slots, dtype=torch.int64, device='cuda')
            totals = torch.zeros(2, dtype=torch.int64, device='cuda')
            g.encrypt_chunks_select(*args, sel.data_ptr(), buf.data_ptr(), off.data_ptr(), totals.data_ptr(), hs())
            torch.cuda.synchronize()
            off_h = off.cpu().numpy().view(np.uint64)
            where = {s: int(off_h[s - s0]) for i, k, s, x, e in live if select_h[s]}
        buf_h = buf.cpu().numpy()
        for i, k, s, x, e in live:
            if s in where:
                out[s] = buf_h[where[s]:where[s] + e - x + OVER].tobytes()
    return out


@pytest.mark.parametrize('n,key_bits', [(n, 256) for n in R.STREAM_COUNTS] + [(1025, 128)])
def test_gcm_encrypt_chunks(oracle, n, key_bits):
    """Every blob = nonce || oracle.gcm_encrypt(key, nonce, chunk) at base[i] + start + 28 k; every
    other byte of the output keeps the fill."""
    st = state(n)
    g = GpuAesGcm(key_bits=key_bits)
    out_total, base = g.chunks_layout(st.ch, st.lens)
    assert (out_total, [int(b) for b in base]) == R.region_bases(st.lay, OVER)
    out = torch.full((out_total,), FILL, dtype=torch.uint8, device='cuda')
    g.encrypt_chunks(st.ch, st.ptrs, st.lens, st.cuts.data_ptr(), st.counts.data_ptr(), st.keys.data_ptr(),
                     st.nonces.data_ptr(), out.data_ptr(), hs())
    torch.cuda.synchronize()
    placed = R.blob_offsets(st.lay, base, OVER)
    blobs = gcm_blobs(st, oracle, key_bits)
    assert set(placed) == set(blobs) == {s for _, _, s, _, _ in st.live}
    check_bytes(out.cpu().numpy(), placed, blobs)
    g.close()


@pytest.mark.parametrize('n', R.STREAM_COUNTS)
def test_chacha_encrypt_chunks(n):
    """Every blob = the one the same call writes for the same streams in calls of at most 1,024;
    the sampled ones = nonce || chacha_ref.seal(...); every other byte keeps the fill."""
    st = state(n)
    g = GpuChaCha20Poly1305()
    out_total, base = g.chunks_layout(st.ch, st.lens)
    assert (out_total, [int(b) for b in base]) == R.region_bases(st.lay, OVER)
    out = torch.full((out_total,), FILL, dtype=torch.uint8, device='cuda')
    g.encrypt_chunks(st.ch, st.ptrs, st.lens, st.cuts.data_ptr(), st.counts.data_ptr(), st.keys.data_ptr(),
                     st.nonces.data_ptr(), out.data_ptr(), hs())
    torch.cuda.synchronize()
    out_h = out.cpu().numpy()
    placed = R.blob_offsets(st.lay, base, OVER)
    small = small_call_blobs(st, g)
    assert set(placed) == set(small) == {s for _, _, s, _, _ in st.live}  # no blob left uncompared
    check_bytes(out_h, placed, small)
    for s, blob in chacha_sample(st).items():
        o, length = placed[s]
        assert out_h[o:o + length].tobytes() == blob, s
    g.close()


@pytest.mark.parametrize('case', ['all', 'alternating', 'one_per_stream', 'none'])
@pytest.mark.parametrize('family', ['chacha', 'gcm'])
@pytest.mark.parametrize('n', [1025, 2049, 3073])
def test_encrypt_chunks_select(oracle, n, family, case):
    """Offsets and totals = the host computation over more than ten tiles of 1,024 cut slots a
    thousand streams (more than 30 for 3,073), one tile boundary between two streams and one
    inside a stream's chunks; the blobs by their family's rule; the fill behind totals[0]."""
    st = state(n)
    tiles = (st.total + R.TILE - 1) // R.TILE
    starts = set(st.lay.cut_base.tolist())
    bounds = range(R.TILE, st.total, R.TILE)
    assert tiles > 10 * (n // 1024) and (n < 3073 or tiles > 30)
    assert any(b in starts for b in bounds)
    assert any(st.mask[b - 1] and st.mask[b] and b not in starts for b in bounds)
    select_h = R.selections(st.lay)[case]
    g = cipher_of(family)
    out_total, _ = g.chunks_layout(st.ch, st.lens)
    out = torch.full((out_total,), FILL, dtype=torch.uint8, device='cuda')
    select = torch.from_numpy(select_h).cuda()
    blob_off = torch.full((st.total,), 5, dtype=torch.int64, device='cuda')
    totals = torch.full((2,), 5, dtype=torch.int64, device='cuda')
    g.encrypt_chunks_select(st.ch, st.ptrs, st.lens, st.cuts.data_ptr(), st.counts.data_ptr(),
                            st.keys.data_ptr(), st.nonces.data_ptr(), select.data_ptr(), out.data_ptr(),
                            blob_off.data_ptr(), totals.data_ptr(), hs())
    torch.cuda.synchronize()
    out_h = out.cpu().numpy()
    want_off, want_totals, picked = R.select_expect(st.lay, select_h, OVER)
    assert totals.cpu().numpy().view(np.uint64).tolist() == want_totals
    assert blob_off.cpu().numpy().view(np.uint64).tolist() == want_off
    live = {s for _, _, s, _, _ in st.live}
    if case == 'all':
        assert set(picked) == live and select_h[~st.mask].all()
    if case == 'one_per_stream':
        assert len(picked) == int((st.lay.counts > 0).sum())
    if case == 'none':
        assert want_totals == [0, 0]
    if family == 'gcm':
        blobs = gcm_blobs(st, oracle, 256)
    else:
        blobs = small_call_blobs(st, g, select_h)
        assert set(blobs) == set(picked)
        for s, blob in chacha_sample(st).items():
            if s in picked:
                o, length = picked[s]
                assert out_h[o:o + length].tobytes() == blob, s
    check_bytes(out_h, picked, blobs)  # the blobs lie back to back from 0: the fill behind totals[0]
    assert (out_h[want_totals[0]:] == FILL).all()
    g.close()


# --------------------------------------------------------------------------- index

def cluster_names(rnd, nb):
    """300 distinct names with the same first 8 bytes (one probe start): 100 differ only in their
    last byte, the others somewhere behind the first 8."""
    head, body = rnd.randbytes(8), rnd.randbytes(nb - 9)
    names = {head + body + bytes([b]) for b in range(100)}
    while len(names) < 300:
        names.add(head + rnd.randbytes(nb - 8))
    return sorted(names)


def probe_length(model, name):
    mask = model.entries - 1
    pos = start = int.from_bytes(name[:8], 'little') & mask
    while model.table[pos] != name:
        pos = (pos + 1) & mask
    return (pos - start) & mask


@pytest.mark.parametrize('nb', [20, 64])
@pytest.mark.parametrize('n', R.STREAM_COUNTS)
def test_index_resolve_chunks(n, nb):
    """rc_index_resolve_chunks over the layout: owners and fresh flags = the dict model
    (tests/test_gpu_index.py) with 300 names in one probe cluster, each about ten times a call in
    different workgroups, names repeated within a call, from the call before and from add(); two
    calls on two HIP streams chained by an event, growth to four times the size, and a third
    call that finds every name under the same owner."""
    st = state(n)
    rnd = random.Random(100 * n + nb)
    cluster = cluster_names(rnd, nb)
    pre = cluster[:30] + [rnd.randbytes(nb) for _ in range(70)]
    counts = st.lay.counts.tolist()
    stream_of = {s: i for i, _, s, _, _ in st.live}

    def call_names(before):
        slots = sorted(stream_of)
        rnd.shuffle(slots)
        names = [None] * st.total
        for j, s in enumerate(slots[:3000]):
            names[s] = cluster[j % 300]
        fresh_pool = [rnd.randbytes(nb) for _ in range(len(slots) // 4)]
        for s in slots[3000:]:
            r = rnd.random()
            names[s] = (rnd.choice(fresh_pool) if r < 0.6 else rnd.choice(pre) if r < 0.7 else
                        rnd.choice(before) if before and r < 0.9 else rnd.randbytes(nb))
        for c in cluster:  # about ten times, in several workgroups of 256 slots and several streams
            mine = [s for s in slots[:3000] if names[s] == c]
            assert len(mine) == 10 and len({s // 256 for s in mine}) > 2 and len({stream_of[s] for s in mine}) > 2
        return names

    names1 = call_names(None)
    names2 = call_names([v for v in names1 if v is not None])
    used = [v for v in names1 + names2 if v is not None]
    assert len(set(used)) < len(used) - 6000 and set(pre) & set(used)
    max_names = 100 + 2 * st.total
    model = I.Model(max_names)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with GpuChunkIndex(nb, max_names) as index:
        assert index.add(pre) == model.add(pre) == 0
        id1, h1 = I.resolve(index, st.ch, st.lens, counts, names1, stream=s1)
        ev = torch.cuda.Event()
        ev.record(s1)
        s2.wait_event(ev)
        id2, h2 = I.resolve(index, st.ch, st.lens, counts, names2, stream=s2)
        torch.cuda.synchronize()
        assert (id1, id2) == (100, 100 + st.total)
        owners1, fresh1 = I.read(h1)
        owners2, fresh2 = I.read(h2)
        for id_base, names, owners, fresh in ((id1, names1, owners1, fresh1), (id2, names2, owners2, fresh2)):
            GpuChunkIndex.check_owners([o for o, v in zip(owners, names) if v is not None])
            I.check(model, id_base, names, owners, fresh)
        # more than a workgroup of lanes walk the cluster, at a load of at most one half
        assert max(probe_length(model, c) for c in cluster) > 256
        assert 2 * len(model.owner) <= model.entries
        index.reserve(4 * max_names)
        model.resize(4 * max_names)
        assert (index.used, index.max_names) == (100 + 2 * st.total, 4 * max_names)
        id3, h3 = I.resolve(index, st.ch, st.lens, counts, names1)
        owners3, fresh3 = I.read(h3)
        GpuChunkIndex.check_owners([o for o, v in zip(owners3, names1) if v is not None])
        assert owners3 == owners1  # the same ids after growth, and the slots without a chunk untouched
        assert fresh3 == [9 if v is None else 0 for v in names1]
        I.check(model, id3, names1, owners3, fresh3)
        assert max(probe_length(model, c) for c in cluster) > 256
        assert 2 * len(model.owner) <= model.entries
