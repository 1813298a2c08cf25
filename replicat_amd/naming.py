"""Chunk names, tags and locations: where replicat keeps a chunk, and so the question an
incremental snapshot asks about every chunk -- does the repository already hold it?

The reference names a chunk by its digest (replicat/repository.py:470-481)::

    encrypted repository:    name = mac(digest), tag = mac(name)
    unencrypted repository:  name = tag = digest

with ``mac = hashlib.blake2b(message, digest_size=L, key=mac_params)`` (replicat/utils/
adapters.py:219-222; ``L`` is the MAC adapter's ``length``, default 64), and stores it at
``data/<tag[:2]>/<tag[2:4]>/<tag[4:]>-<name>`` in hex (repository.py:446-468).  ``ChunkNaming`` is
the host statement of that rule; the producer computes the same names and tags on the device
(two rc_blake2b_derive_chunks calls over the digests in HBM, replicat_amd/pipeline.py).
"""
import hashlib
import posixpath
from typing import Iterable, Iterator, NamedTuple, Optional, Tuple

CHUNK_PREFIX = 'data/'
SNAPSHOT_PREFIX = 'snapshots/'


class LocationParts(NamedTuple):
    name: str
    tag: str


def chunk_location(name: str, tag: str) -> str:
    """get_chunk_location (repository.py:446-459): name and tag are hex strings."""
    return posixpath.join(CHUNK_PREFIX, tag[:2], tag[2:4], f'{tag[4:]}-{name}')


def parse_chunk_location(location: str) -> LocationParts:
    """parse_chunk_location (repository.py:461-468)."""
    if not location.startswith(CHUNK_PREFIX):
        raise ValueError('Not a chunk location')
    head, _, name = location.rpartition('-')
    parts = head.rsplit('/', 3)
    return LocationParts(name=name, tag=parts[1] + parts[2] + parts[3])


def snapshot_location(name: str, tag: str) -> str:
    """get_snapshot_location (repository.py:483-491): name and tag are hex strings."""
    return posixpath.join(SNAPSHOT_PREFIX, tag[:2], f'{tag[2:]}-{name}')


def parse_snapshot_location(location: str) -> LocationParts:
    """parse_snapshot_location (repository.py:493-499)."""
    if not location.startswith(SNAPSHOT_PREFIX):
        raise ValueError('Not a snapshot location')
    head, _, name = location.rpartition('-')
    parts = head.rsplit('/', 2)
    return LocationParts(name=name, tag=parts[1] + parts[2])


def names_from_locations(locations: Iterable[str], name_bytes: Optional[int] = None) -> Iterator[bytes]:
    """The name bytes of a backend listing of ``data/`` (``list_files('data/')``), as a chunk
    index takes them.  Entries that do not parse as a chunk location -- another prefix, no
    hyphen, a name that is not hex, or (with ``name_bytes``) not of that size -- are skipped."""
    for location in locations:
        try:
            name = bytes.fromhex(parse_chunk_location(location).name)
        except (ValueError, IndexError, AttributeError, TypeError):
            continue
        if not name or (name_bytes is not None and len(name) != name_bytes):
            continue
        yield name


class ChunkNaming:
    """A repository's chunk naming: ``mac_key`` is the MAC adapter's key (``mac_params``) of an
    encrypted repository and ``length`` its digest size; ``mac_key=None`` is the unencrypted
    case, where name and tag are the digest itself and ``length`` is unused."""

    def __init__(self, mac_key: Optional[bytes] = None, length: int = 64):
        if mac_key is not None:
            mac_key = bytes(mac_key)
            if not 1 <= len(mac_key) <= 64:
                raise ValueError('mac_key must be 1..64 bytes (a BLAKE2b key)')
            if not isinstance(length, int) or not 1 <= length <= 64:
                raise ValueError('length must be 1..64 (a BLAKE2b digest size)')
        self.mac_key = mac_key
        self.length = length

    @property
    def keyed(self) -> bool:
        return self.mac_key is not None

    def name_bytes(self, digest_size: int) -> int:
        """Bytes in a name (and in a tag) for chunk digests of ``digest_size`` bytes."""
        return self.length if self.keyed else digest_size

    def mac(self, message: bytes) -> bytes:
        return hashlib.blake2b(message, digest_size=self.length, key=self.mac_key).digest()

    def parts(self, digest: bytes) -> Tuple[bytes, bytes]:
        """(name, tag) of a chunk digest: _chunk_digest_to_location_parts, as bytes."""
        if not self.keyed:
            return digest, digest
        name = self.mac(digest)
        return name, self.mac(name)

    def location(self, digest: bytes) -> str:
        """_chunk_digest_to_location (repository.py:479-481)."""
        name, tag = self.parts(digest)
        return chunk_location(name.hex(), tag.hex())


__all__ = ['ChunkNaming', 'LocationParts', 'CHUNK_PREFIX', 'chunk_location', 'parse_chunk_location',
           'names_from_locations', 'SNAPSHOT_PREFIX', 'snapshot_location', 'parse_snapshot_location']
