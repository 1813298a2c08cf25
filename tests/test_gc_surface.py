"""What garbage-collection planning answers without a device: the C ABI's argument checks
(include/replicat_gc.h and the two additions to replicat_index.h) come before any device is
looked for, and replicat_amd.gc checks its arguments and packs a listing on the host."""
import ctypes

import numpy as np
import pytest

from replicat_amd import _lib
from replicat_amd.naming import ChunkNaming, chunk_location

ARGUMENT, NO_DEVICE = _lib.RC_ERR_ARGUMENT, _lib.RC_ERR_NO_DEVICE
KEY = b'k' * 32


def no_gpu():
    try:
        import torch
        return not torch.cuda.is_available()
    except ImportError:
        return True


def call(name, *args):
    """(return code, rc_last_error()) of one entry point."""
    rc = getattr(_lib.lib(), name)(*args)
    return rc, _lib.last_error()


def test_codes_and_signatures():
    assert _lib.RC_ERR_PROBE_BOUND == _lib.RC_ERR_INDEX_FULL + 1 == 18
    assert (_lib.RC_INDEX_ABSENT, _lib.RC_INDEX_EXHAUSTED) == (-1, -2)
    assert (_lib.RC_GC_REFERENCED, _lib.RC_GC_DELETE, _lib.RC_GC_TAG_MISMATCH, _lib.RC_GC_EXHAUSTED) == (0, 1, 2, 3)
    for name in ('rc_index_lookup_device', 'rc_index_resolve_names_device', 'rc_gc_create', 'rc_gc_destroy',
                 'rc_gc_name_bytes', 'rc_gc_used', 'rc_gc_capacity', 'rc_gc_reference_host',
                 'rc_gc_sweep_device', 'rc_gc_sweep_host', 'rc_gc_unreferenced_host',
                 'rc_gc_timing_enable', 'rc_gc_timing_read'):
        assert name in _lib.SIGNATURES
        assert getattr(_lib.lib(), name)


def test_exported_from_the_package():
    import replicat_amd
    from replicat_amd import gc as rgc
    assert replicat_amd.GpuChunkGC is rgc.GpuChunkGC and replicat_amd.CleanPlan is rgc.CleanPlan
    assert rgc.CleanPlan._fields == ('to_delete', 'referenced', 'tag_mismatch')
    with pytest.raises(AttributeError):
        replicat_amd.no_such_name


def test_index_additions_without_a_device():
    base = ctypes.c_uint64()
    assert call('rc_index_lookup_device', None, 1, None, None, None) == (ARGUMENT, 'null index')
    assert call('rc_index_resolve_names_device', None, 1, None, ctypes.byref(base), None, None, None) == (
        ARGUMENT, 'null index')


def test_gc_create_without_a_device():
    h = ctypes.c_void_p()
    out = ctypes.byref(h)
    assert call('rc_gc_create', 64, 64, KEY, 32, 8, 0, None) == (ARGUMENT, 'null output handle')
    for bad in (0, 65):
        assert call('rc_gc_create', bad, 64, KEY, 32, 8, 0, out) == (
            ARGUMENT, f'digest_bytes must be 1..64, not {bad}')
        assert call('rc_gc_create', 64, bad, KEY, 32, 8, 0, out) == (
            ARGUMENT, f'name_bytes must be 1..64, not {bad}')
        assert call('rc_gc_create', 64, 64, KEY * 3, bad, 8, 0, out) == (
            ARGUMENT, f'mac_keylen must be 1..64, not {bad}')
    assert call('rc_gc_create', 32, 64, None, 0, 8, 0, out) == (
        ARGUMENT, 'unkeyed: name_bytes 64 must equal digest_bytes 32')
    assert call('rc_gc_create', 64, 64, None, 0, (1 << 40) + 1, 0, out) == (ARGUMENT, 'max_refs above 2^40')
    assert not h.value
    if no_gpu():
        # keyed names need not be as long as the digests; unkeyed ones are the digests
        assert call('rc_gc_create', 32, 64, KEY, 32, 8, 0, out) == (NO_DEVICE, 'no HIP device 0')
        assert call('rc_gc_create', 28, 28, None, 0, 8, 0, out) == (NO_DEVICE, 'no HIP device 0')
        assert not h.value


def test_gc_null_handles():
    n = ctypes.c_uint64(7)
    assert call('rc_gc_reference_host', None, 0, None) == (ARGUMENT, 'null gc')
    assert call('rc_gc_sweep_device', None, 0, None, None, 0, None, None, None, None) == (ARGUMENT, 'null gc')
    assert call('rc_gc_sweep_host', None, 0, None, None, None, None, ctypes.byref(n)) == (ARGUMENT, 'null gc')
    assert call('rc_gc_unreferenced_host', None, 0, None, None, None, None, ctypes.byref(n)) == (
        ARGUMENT, 'null gc')
    assert call('rc_gc_timing_enable', None, 1) == (ARGUMENT, 'null gc')
    assert call('rc_gc_timing_read', None, None, None, None, None) == (ARGUMENT, 'null gc')
    lib = _lib.lib()
    assert lib.rc_gc_name_bytes(None) == 0
    assert lib.rc_gc_used(None) == 0
    assert lib.rc_gc_capacity(None) == 0
    lib.rc_gc_destroy(None)


def test_python_argument_checks():
    from replicat_amd.gc import GpuChunkGC
    with pytest.raises(TypeError, match='naming must be a ChunkNaming'):
        GpuChunkGC(None, 64)
    for bad in (0, 65, 1.5):
        with pytest.raises(ValueError, match='digest_size must be 1..64'):
            GpuChunkGC(ChunkNaming(), bad)
    with pytest.raises(ValueError, match='max_refs must not be negative'):
        GpuChunkGC(ChunkNaming(), 64, max_refs=-1)
    if no_gpu():
        with pytest.raises(_lib.ChunkerUnavailable, match='no HIP device'):
            GpuChunkGC(ChunkNaming(KEY, 32), 64, device=0)


def test_rows_packing():
    from replicat_amd.gc import _rows
    rows = _rows([b'abc', bytearray(b'def')], 3, 'digest')
    assert rows.dtype == np.uint8 and rows.shape == (2, 3) and rows.tobytes() == b'abcdef'
    assert _rows([], 3, 'digest').shape == (0, 3)
    assert _rows(iter([b'xyz']), 3, 'name').tolist() == [[120, 121, 122]]
    arr = np.arange(12, dtype=np.uint8).reshape(3, 4)[:, :2]  # not contiguous
    assert _rows(arr.reshape(-1, 2), 2, 'name').flags['C_CONTIGUOUS']
    with pytest.raises(ValueError, match='a digest of 2 bytes where digests have 3'):
        _rows([b'abc', b'de'], 3, 'digest')


@pytest.mark.parametrize('nb', [2, 7, 64])
def test_block_packing_equals_the_definition(nb, monkeypatch):
    """split_locations packs whole blocks of the listing at once where it can; entry by entry
    (_split_one, the definition) it must come to the same split.  Blocks of 8 entries here, so
    that blocks with and without odd entries, a short last block and blocks that fall back
    (a non-ASCII entry, an entry that is no string) all occur."""
    import re
    from replicat_amd import gc as rgc
    monkeypatch.setattr(rgc, '_BLOCK', 8)
    rnd = np.random.default_rng(nb)
    good = [chunk_location(rnd.bytes(nb).hex(), rnd.bytes(nb).hex()) for _ in range(60)]
    width = len(good[0])
    assert width == 4 * nb + 8 and all(len(g) == width for g in good)
    odd = {
        3: good[3].upper().replace('DATA', 'data'),
        9: good[9][:-1] + 'g',                      # the right length, not hex
        10: good[10].replace('/', '-', 1),          # the right length, a hyphen for the first slash
        11: 'dat4' + good[11][4:],                  # the right length, another prefix
        20: good[20][:-1] + 'é',               # the right length, not ASCII: its block falls back
        33: good[33].replace('-', '/'),             # a slash for the hyphen
        34: good[34][:7] + '-' + good[34][8:],      # a hyphen for the second slash
        41: None,                                   # its block falls back
        42: good[42].encode(),
        50: good[50] + '0',
        51: good[51][:5] + 'A' + good[51][6:],      # one upper-case digit in the tag
    }
    listing = [odd.get(i, g) for i, g in enumerate(good)]
    positions, names, tags, others = rgc.split_locations(listing, nb)
    hexes = re.compile('[0-9a-f]{%d}' % (2 * nb)).fullmatch
    want = [rgc._split_one(x, hexes) for x in listing]
    assert others == sorted(odd) == [i for i, w in enumerate(want) if w is None]
    assert positions.tolist() == [i for i, w in enumerate(want) if w is not None]
    assert names.tobytes().hex() == ''.join(w[0] for w in want if w) and names.shape == (49, nb)
    assert tags.tobytes().hex() == ''.join(w[1] for w in want if w) and tags.shape == (49, nb)


def test_one_byte_names_never_parse():
    """With a one-byte tag the location has no third directory level and parse_chunk_location
    (the reference's, repository.py:461-468) raises IndexError: such a listing is all host path."""
    from replicat_amd.gc import split_locations
    loc = chunk_location('a0', 'b0')
    assert loc == 'data/b0/-a0'
    assert split_locations([loc], 1)[3] == [0]


@pytest.mark.parametrize('nb', [2, 3, 32, 64])
def test_split_locations(nb):
    """Canonical: parses, and is exactly chunk_location of nb-byte lower-case hex.  Everything
    else keeps its place in `others`; the packed rows are the parsed bytes, in listing order."""
    from replicat_amd.gc import split_locations
    name, tag = bytes(range(0xA0, 0xA0 + nb)), bytes(range(0xB0, 0xB0 + nb))
    good = chunk_location(name.hex(), tag.hex())
    good2 = chunk_location(tag.hex(), name.hex())
    listing = [
        good,
        good.upper().replace('DATA', 'data'),           # upper-case hex
        'other/' + good[len('data/'):],                 # a foreign prefix
        chunk_location(name.hex() + '00', tag.hex()),   # name too long
        chunk_location(name.hex(), tag.hex() + '00'),   # tag too long
        chunk_location(name.hex()[:-2] + 'zz', tag.hex()),  # not hex
        chunk_location(name.hex()[:-1] + ' ', tag.hex()),   # bytes.fromhex would take the blank
        good.replace('-', '--', 1),                     # the name would start with a hyphen
        good + '/',                                     # trailing slash
        'data/nohyphen',
        '',
        good2,
    ]
    positions, names, tags, others = split_locations(listing, nb)
    assert positions.dtype == np.int64 and positions.tolist() == [0, len(listing) - 1]
    assert others == list(range(1, len(listing) - 1))
    assert names.tobytes() == name + tag and tags.tobytes() == tag + name
    assert names.shape == tags.shape == (2, nb)
    positions, names, tags, others = split_locations(iter([]), nb)
    assert (positions.shape, names.shape, tags.shape, others) == ((0,), (0, nb), (0, nb), [])
