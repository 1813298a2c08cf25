"""CPU tests of snapshot writing (replicat_amd/snapshot_write.py, include/replicat_snapshot.h): the
length rules against json.dumps and base64, the argument errors reported before any device is
touched, the registration of the new source and symbols, and the host helpers that assemble a
file against bodies the reference's own hooks serialised (tests/golden/snapshot_bodies.json)."""
import base64
import ctypes
import os
import re

import pytest

import golden_util as G
import snapshot_ref as ref

from replicat_amd import _lib, build, snapshot_write
from replicat_amd._lib import ChunkerUnavailable

GOLDEN = G.load('snapshot_bodies.json')['cases']
TABLES = [c for c in GOLDEN if 'table' in c]
ENVELOPES = [c for c in GOLDEN if 'envelope' in c]
NO_LEN = (1 << 64) - 1
NEW_SYMBOLS = ['rc_snapshot_table_len', 'rc_snapshot_table_len_for', 'rc_snapshot_b64_len',
               'rc_snapshot_b64_encode_device', 'rc_snapshot_seal_tables_device', 'rc_snapshot_seal_tables_host',
               'rc_snapshot_write_timing_read']


def test_table_len_against_json_dumps_and_as_the_inverse_of_table_count():
    L = _lib.lib()
    for width in range(1, 65):
        for n in (0, 1, 2, 65):
            table = ref.serialize([bytes([n & 255]) * width] * n)
            assert L.rc_snapshot_table_len_for(width, n) == len(table), (width, n)
            assert L.rc_snapshot_table_count_for(width, len(table)) == n, (width, n)
    for width in (0, 65):
        assert L.rc_snapshot_table_len_for(width, 0) == NO_LEN and L.rc_snapshot_table_len_for(width, 3) == NO_LEN
    assert L.rc_snapshot_table_len(None, 0) == NO_LEN and L.rc_snapshot_table_len(None, 5) == NO_LEN


def test_table_len_overflow():
    L = _lib.lib()
    for width in (1, 20, 64):
        stride = 4 * ((width + 2) // 3) + 10
        most = (NO_LEN - 2) // stride  # 1 + most * stride <= 2^64 - 2
        assert L.rc_snapshot_table_len_for(width, most) == 1 + most * stride
        assert L.rc_snapshot_table_count_for(width, 1 + most * stride) == most
        for count in (most + 1, 1 << 62, NO_LEN):
            assert L.rc_snapshot_table_len_for(width, count) == NO_LEN, (width, count)


def test_b64_len_against_base64():
    L = _lib.lib()
    for n in range(51):
        assert L.rc_snapshot_b64_len(n) == len(base64.standard_b64encode(bytes(n))) == snapshot_write.b64_len(n)
    most = (NO_LEN // 4) * 3
    assert L.rc_snapshot_b64_len(most) == NO_LEN // 4 * 4
    assert L.rc_snapshot_b64_len(most + 1) == NO_LEN and L.rc_snapshot_b64_len(NO_LEN) == NO_LEN


def test_new_entry_points_refuse_a_null_handle_before_any_device():
    L = _lib.lib()
    one = (ctypes.c_uint64 * 1)(1)
    calls = [
        lambda: L.rc_snapshot_b64_encode_device(None, 1, one, one, one, None),
        lambda: L.rc_snapshot_seal_tables_device(None, 1, None, one, one, None, None, one, None, None),
        lambda: L.rc_snapshot_seal_tables_host(None, 1, None, one, None, None, one),
        lambda: L.rc_snapshot_write_timing_read(None, None, None, None, None),
    ]
    for call in calls:
        assert call() == _lib.RC_ERR_ARGUMENT
        assert 'null snapshot handle' in _lib.last_error()
    assert _lib.lib().rc_version() == 300


def test_source_and_symbols_are_registered():
    names = {os.path.basename(p) for p in build.SOURCES + build.HEADERS}
    assert {'snapshot_write.hip', 'snapshot.hip', 'capi_snapshot.cpp', 'snapshot_kernels.h'} <= names
    header = open(os.path.join(build.ROOT, 'include', 'replicat_snapshot.h')).read()
    declared = set(re.findall(r'\b(rc_snapshot_\w+)\(', header))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES, name
        assert getattr(_lib.lib(), name) is not None
    kernels = open(os.path.join(build.CSRC, 'snapshot_kernels.h')).read()
    assert 'rc_snap_encode_tables_kernel(' in kernels and 'rc_snap_b64_encode_kernel(' in kernels


def test_host_helpers_reproduce_the_golden_bodies():
    assert len(TABLES) == 32 and len(ENVELOPES) == 3
    for c in TABLES:
        chunks = [bytes.fromhex(h) for h in c['chunks']]
        data = ref.deserialize(c['data'])
        assert snapshot_write.serialize(chunks) == c['table'].encode()
        assert snapshot_write.serialize(data) == c['data'].encode()
        assert snapshot_write.assemble_plain(c['table'].encode(), snapshot_write.serialize(data)) == c['body'].encode()
    for c in ENVELOPES:
        blob = {k: bytes.fromhex(v) for k, v in c['envelope'].items()}
        assert snapshot_write.assemble_encrypted(blob['chunks'], blob['data']) == c['body'].encode()
    assert snapshot_write.assemble_plain(b'[]', b'null') == ref.serialize({'chunks': [], 'data': None})
    assert snapshot_write.assemble_encrypted(b'', b'') == ref.serialize({'chunks': b'', 'data': b''})


def test_writer_is_exported_and_needs_a_gpu():
    import replicat_amd
    assert replicat_amd.GpuSnapshotWriter is snapshot_write.GpuSnapshotWriter
    assert replicat_amd.DeviceDigests is snapshot_write.DeviceDigests
    with pytest.raises(ValueError):  # before any device: an encrypted repository without the user key
        snapshot_write.GpuSnapshotWriter(encryption=snapshot_write.ChunkEncryption(b'k' * 32, b'p' * 16))
    try:
        import torch
        has_gpu = torch.cuda.is_available()
    except ImportError:
        has_gpu = False
    if has_gpu:  # the GPU tests cover the rest (tests/test_gpu_snapshot_write.py)
        snapshot_write.GpuSnapshotWriter(encryption=None).close()
    else:
        with pytest.raises(ChunkerUnavailable):
            snapshot_write.GpuSnapshotWriter(encryption=None)
