"""replicat's garbage collection restated over hashlib and sets: what `clean` and
`delete_snapshots` decide, without a repository, a backend or a device.

The lines cited are those of replicat/repository.py.  Nothing here imports replicat_amd: the
naming rule (:446-481) is restated too, so that the device code and its host helpers are checked
against a second statement of it."""
import hashlib
import posixpath

CHUNK_PREFIX = 'data/'


class RefNaming:
    """props.encrypted / props.mac and the location rule (:446-481)."""

    def __init__(self, mac_key=None, length=64):
        self.mac_key, self.length = mac_key, length

    @property
    def encrypted(self):
        return self.mac_key is not None

    def mac(self, message):
        return hashlib.blake2b(message, digest_size=self.length, key=self.mac_key).digest()

    @staticmethod
    def get_chunk_location(name, tag):  # :446-459
        return posixpath.join(CHUNK_PREFIX, tag[:2], tag[2:4], f'{tag[4:]}-{name}')

    @staticmethod
    def parse_chunk_location(location):  # :461-468
        if not location.startswith(CHUNK_PREFIX):
            raise ValueError('Not a chunk location')
        head, _, name = location.rpartition('-')
        parts = head.rsplit('/', 3)
        return name, parts[1] + parts[2] + parts[3]

    def location_parts(self, digest):  # :470-477
        if self.encrypted:
            digest_mac = self.mac(digest)
            digest_mac_mac = self.mac(digest_mac)
        else:
            digest_mac = digest_mac_mac = digest
        return digest_mac.hex(), digest_mac_mac.hex()

    def digest_to_location(self, digest):  # :479-481
        name, tag = self.location_parts(digest)
        return self.get_chunk_location(name, tag)


REFERENCED, DELETE, TAG_MISMATCH = 0, 1, 2


def clean_verdicts(naming, snapshots, listing):
    """:1939-1960, the verdict per listed entry.  snapshots: an iterable of digest lists
    (body['chunks'] of every snapshot); listing: what backend.list_files('data/') yields."""
    referenced_digests = {y for x in snapshots for y in x}  # :1939-1941
    referenced_locations = set(map(naming.digest_to_location, referenced_digests))  # :1942-1944
    out = []
    for location in listing:  # :1948
        if location in referenced_locations:  # :1949-1951
            out.append(REFERENCED)
            continue
        if naming.encrypted:  # :1953
            name, tag = naming.parse_chunk_location(location)  # :1955
            if naming.mac(bytes.fromhex(name)) != bytes.fromhex(tag):  # :1956
                out.append(TAG_MISMATCH)  # :1957-1958
                continue
        out.append(DELETE)  # :1960
    return out


def clean_verdicts_bytes(naming, snapshots, pairs):
    """clean_verdicts for entries given as (name, tag) BYTES, the form the device takes: a
    location string of lower-case hex of fixed lengths says no more than its two byte strings, so
    `location in referenced_locations` is `(name, tag) in referenced parts`.  Needs no location
    to parse, so it also covers one-byte names (whose locations the reference cannot parse)."""
    referenced = set()
    for digest in {y for x in snapshots for y in x}:
        name, tag = naming.location_parts(digest)
        referenced.add((bytes.fromhex(name), bytes.fromhex(tag)))
    out = []
    for name, tag in pairs:
        if (name, tag) in referenced:
            out.append(REFERENCED)
        elif naming.encrypted and naming.mac(name) != tag:
            out.append(TAG_MISMATCH)
        else:
            out.append(DELETE)
    return out


def clean(naming, snapshots, listing):
    """to_delete of :1945-1960: the set of locations clean deletes."""
    listing = list(listing)
    return {loc for loc, v in zip(listing, clean_verdicts(naming, snapshots, listing)) if v == DELETE}


def delete_snapshots(naming, deleted, kept):
    """:1863-1899 and :1907-1909.  deleted / kept: the digest lists of the snapshots being
    deleted and of all the others.  Returns the set of chunk locations that go."""
    chunks_to_delete, chunks_to_keep = set(), set()  # :1863-1864
    for chunks in deleted:
        chunks_to_delete.update(chunks)  # :1877
    for chunks in kept:
        chunks_to_keep.update(chunks)  # :1886
    chunks_to_delete.difference_update(chunks_to_keep)  # :1899
    return {naming.digest_to_location(d) for d in chunks_to_delete}  # :1907-1909


def first_occurrences(deleted, kept):
    """The order the device plan gives delete_snapshots' set: the distinct digests of `deleted`
    (lists, concatenated) that `kept` does not hold, each at its first occurrence."""
    keep = {d for chunks in kept for d in chunks}
    seen, out = set(), []
    for d in (d for chunks in deleted for d in chunks):
        if d not in keep and d not in seen:
            seen.add(d)
            out.append(d)
    return out
