"""replicat_amd -- an MI355X-native content-defined chunker for replicat.

The hot path (replicat's ``gclmulchunker``: keyed GF(2) hashes at 4-byte-aligned offsets,
cut at the windowed first argmax; /root/reference/src/adapters.cpp:42-77) runs as
hand-written gfx950 HIP kernels in ``libreplicat_chunker.so`` behind a C ABI
(``include/replicat_chunker.h``).  The Python side mirrors the reference's
``_replicat_adapters`` surface (``replicat_amd._replicat_adapters``) and adds a batch API over
many device- or host-resident streams (``replicat_amd.chunker``).
"""
__version__ = '0.3.0'

_GC_EXPORTS = ('GpuChunkGC', 'CleanPlan')
_SNAPSHOTS_EXPORTS = ('GpuSnapshotLoader', 'LoadedSnapshot')
_SNAPSHOT_WRITE_EXPORTS = ('GpuSnapshotWriter', 'WrittenSnapshot', 'DeviceDigests', 'SnapshotLayout', 'SnapshotData')
__all__ = list(_GC_EXPORTS + _SNAPSHOTS_EXPORTS + _SNAPSHOT_WRITE_EXPORTS)


def __getattr__(name):
    # garbage-collection planning (replicat_amd/gc.py), imported on first use: the package itself
    # stays importable without numpy
    if name in _GC_EXPORTS:
        from . import gc
        return getattr(gc, name)
    if name in _SNAPSHOTS_EXPORTS:  # snapshot loading (replicat_amd/snapshots.py), likewise
        from . import snapshots
        return getattr(snapshots, name)
    if name in _SNAPSHOT_WRITE_EXPORTS:  # snapshot writing (replicat_amd/snapshot_write.py)
        from . import snapshot_write
        return getattr(snapshot_write, name)
    raise AttributeError(f'module {__name__!r} has no attribute {name!r}')
