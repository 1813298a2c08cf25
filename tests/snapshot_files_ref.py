"""The host twin of replicat_amd/csrc/snapshot_fields.hip, for the tests: the columns of the files
of a `data` text and whether the device may accept it, both through json (snapshots.deserialize,
that is json.loads with the reference's object hook) and nothing of the device or the writer."""
import json
from types import SimpleNamespace

import numpy as np

from replicat_amd.snapshots import METADATA_KEYS, deserialize, serialize

BS = chr(92)
FIRST_MOST = 4096  # csrc/snapshot_kernels.h kSnapFirstMost
INT64 = range(-2 ** 63, 2 ** 63)


def u(code: int) -> str:
    """The six characters of a JSON escape of one code unit, lowercase."""
    return BS + 'u%04x' % code


def quote(path: str) -> str:
    return json.encoder.encode_basestring_ascii(path)


def columns_of(text, width):
    """The columns of the files of serialize(data), in listing order, from json.loads."""
    data = deserialize(text)
    files = data['files']
    m = len(files)
    raw = [f['path'].encode('utf-8', 'surrogatepass') for f in files]
    off = np.concatenate([[0], np.cumsum([len(r) for r in raw])]).astype(np.uint64)
    digests = np.zeros((m, width), dtype=np.uint8)
    unfinished = np.zeros(m, dtype=bool)
    has_meta = bool(m) and 'metadata' in files[0]
    metadata = np.zeros((m, 7), dtype=np.int64) if has_meta else None
    for k, f in enumerate(files):
        unfinished[k] = f['digest'] is None
        if f['digest'] is not None:
            digests[k] = np.frombuffer(f['digest'], dtype=np.uint8)
        if has_meta and f['metadata'] is not None:
            metadata[k] = [f['metadata'][key] for key in METADATA_KEYS]
    first = text[:text.index(b'"files":[') + 9]
    last = serialize({k: v for k, v in data.items() if k not in ('utc_timestamp', 'files')})[1:]
    last = (b',' + last) if last != b'}' else last
    return SimpleNamespace(path_bytes=np.frombuffer(b''.join(raw), dtype=np.uint8), path_off=off, digests=digests,
                           unfinished=unfinished, metadata=metadata, first=first, last=last, m=m)


def is_canonical(text, width) -> bool:
    """Whether the files pass accepts the text: serialize(deserialize(text)) == text, and the
    shape the device's grammar has -- utc_timestamp (a string) then files, at least one file,
    every file path, chunks, digest and for all or none metadata; at least one part in every
    file (a run is a list with parts: a file without any has no run, and its text lies inside a
    neighbour's piece); a digest null or `width` bytes;
    metadata null exactly when the digest is, else the seven keys in order with int64 values."""
    try:
        data = deserialize(text)
        if serialize(data) != bytes(text) or not isinstance(data, dict):
            return False
    except ValueError:
        return False
    keys = list(data)
    if keys[:2] != ['utc_timestamp', 'files'] or type(data['utc_timestamp']) is not str:
        return False
    files = data['files']
    if type(files) is not list or not files or not all(type(f) is dict for f in files):
        return False
    if len(b'{"utc_timestamp":' + quote(data['utc_timestamp']).encode() + b',"files":[') > FIRST_MOST:
        return False
    with_meta = 'metadata' in files[0]
    for f in files:
        if list(f) != ['path', 'chunks', 'digest'] + (['metadata'] if with_meta else []):
            return False
        if type(f['path']) is not str or type(f['chunks']) is not list or not f['chunks']:
            return False
        d = f['digest']
        if d is not None and not (type(d) is bytes and len(d) == width):
            return False
        if with_meta:
            meta = f['metadata']
            if (meta is None) != (d is None):
                return False
            if meta is not None:
                if type(meta) is not dict or tuple(meta) != METADATA_KEYS:
                    return False
                if not all(type(v) is int and v in INT64 for v in meta.values()):
                    return False
    return True


def file_entry(path, digest, meta=False, chunks=()):
    """One file's dict; meta False: no key, None: null, else the seven values."""
    entry = {'path': path, 'chunks': list(chunks), 'digest': digest}
    if meta is not False:
        entry['metadata'] = None if meta is None else dict(zip(METADATA_KEYS, meta))
    return entry


def part(start, end, index, counter):
    return {'range': [start, end], 'index': index, 'counter': counter}


def data_text(files, stamp='2024-02-03 04:05:06.070809', note=None) -> bytes:
    data = {'utc_timestamp': stamp, 'files': files}
    if note is not None:
        data['note'] = note
    return serialize(data)


# ------------------------------------------------------------------ the rejection list

def base_text(width):
    """Three files with metadata and digests of `width` bytes; the first lists a part."""
    digests = {1: [b'A', b'B', b'C'], 2: [b'AB', b'\xfb\xef', b'CD']}[width]
    files = [file_entry('caf' + chr(0xE9) + '/a', digests[0], (1, 2, 3, 4, 5, 6, 7), [part(0, 5, 0, 1)]),
             file_entry('x/y', digests[1], (10, 11, 12, 13, 14, 15, 16), [part(5, 9, 1, 2), part(0, 3, 2, 3)]),
             file_entry('z', digests[2], (20, 21, 22, 23, 24, 25, 26), [part(3, 4, 2, 4)])]
    return data_text(files, note='n')


def rejections():
    """name -> (text, digest width, whether json.loads takes it).  One mutation each of a text the
    device accepts; none of them is what serialize writes."""
    meta1 = b',"metadata":{"st_mode":10,"st_uid":11,"st_gid":12,"st_size":13,"st_atime_ns":14,"st_mtime_ns":15,"st_ctime_ns":16}'
    e9 = u(0xE9).encode()
    swaps = {
        'uppercase_hex': (1, e9, e9.upper().replace(b'U', b'u'), True),
        'escaped_slash': (1, b'/a"', (BS + '/a"').encode(), True),
        'escaped_letter': (1, b'"x/y"', ('"' + u(0x41) + '/y"').encode(), True),
        'long_form_of_backspace': (1, b'"z"', ('"' + u(8) + '"').encode(), True),
        'raw_0x7f': (1, b'"z"', b'"\x7f"', True),
        'raw_utf8': (1, e9, chr(0xE9).encode('utf-8'), True),
        'space_after_colon': (1, b'"digest":{"!b":"Qg=="}', b'"digest": {"!b":"Qg=="}', True),
        'metadata_keys_swapped': (1, b'"st_uid":2,"st_gid":3', b'"st_gid":3,"st_uid":2', True),
        'st_atime': (1, b'"st_atime_ns":5', b'"st_atime":5', True),
        'eighth_key': (1, b'"st_ctime_ns":7}', b'"st_ctime_ns":7,"x":1}', True),
        'extra_key_in_entry': (1, b'"digest":{"!b":"QQ=="},', b'"digest":{"!b":"QQ=="},"extra":1,', True),
        'metadata_missing_in_one': (1, meta1, b'', True),
        'digest_null_metadata_set': (1, b'"digest":{"!b":"Qg=="}', b'"digest":null', True),
        'metadata_null_digest_set': (1, meta1, b',"metadata":null', True),
        'digest_one_byte_short': (2, b'"QUI="', b'"QQ=="', True),
        'trailing_bits': (1, b'"QQ=="', b'"QR=="', True),
        'url_alphabet': (2, b'"++8="', b'"-+8="', True),
        'leading_zero': (1, b'"st_mode":1,', b'"st_mode":01,', False),
        'minus_zero': (1, b'"st_mode":1,', b'"st_mode":-0,', True),
        'beyond_int64': (1, b'"st_mode":1,', b'"st_mode":9223372036854775808,', True),
        'float': (1, b'"st_mode":1,', b'"st_mode":1.0,', True),
        'exponent': (1, b'"st_mode":1,', b'"st_mode":1e3,', True),
        'note_first': (1, b'{"utc_timestamp"', b'{"note":"m","utc_timestamp"', True),
        'file_without_parts': (1, b'[{"range":[3,4],"index":2,"counter":4}]', b'[]', True),
        'unterminated_path': (1, b'"z","chunks"', b'"z,"chunks"', False),
        'bare_backslash': (1, b'"z","chunks"', ('"z' + BS + '","chunks"').encode(), False),
    }
    out = {}
    for name, (width, old, new, loads) in swaps.items():
        text = base_text(width)
        assert text.count(old) >= 1, name
        out[name] = (text.replace(old, new, 1), width, loads)
    return out


# the Q of every escape the device must refuse, without its quotes
REFUSED_Q = [BS, 'a' + BS, BS + '/', u(0x41), u(8), u(9), u(0xA), u(0xC), u(0xD), u(0x22), u(0x5C), u(0x20), u(0x7E),
             BS + 'u00E9', BS + 'u00e', BS + 'u', BS + 'x41', BS + 'a', '"', 'a"b', chr(0x7F), chr(0x1F), chr(0xE9), '\t',
             BS + 'U00e9', u(0xD83D) + BS + 'uDE00', BS + BS + BS]
