"""replicat's snapshot body code restated with the stdlib, as the host reference of the snapshot
loader tests: serialize / deserialize (replicat/repository.py:434-444 with utils.type_hint and
utils.type_reverse, utils/__init__.py:166-186), _encrypt_snapshot_body (:982-999) and
_decrypt_snapshot_body (:1001-1020).

The ciphers are the host references the restore tests use -- the oracle's AES-GCM
(oracle.gcm_encrypt / gcm_decrypt) and tests/chacha_ref.py -- never the device's.
tests/test_snapshot_ref.py pins serialize and deserialize to bodies the reference's own
type_hint / type_reverse produced (tests/golden/snapshot_bodies.json).
"""
import base64
import hashlib
import json

import chacha_ref


class DecryptionError(Exception):
    """replicat.exceptions.DecryptionError."""


def type_hint(obj):
    if isinstance(obj, (bytes, bytearray)):
        return {'!b': str(base64.standard_b64encode(obj), 'ascii')}
    raise TypeError


def type_reverse(obj):
    if len(obj) != 1:
        return obj
    try:
        encoded = obj['!b']
    except KeyError:
        return obj
    else:
        return base64.standard_b64decode(encoded)


def serialize(obj) -> bytes:
    return bytes(json.dumps(obj, separators=(',', ':'), default=type_hint), 'ascii')


def deserialize(data):
    return json.loads(data, object_hook=type_reverse)


class Repo:
    """The ``props`` a snapshot body needs: ``cipher`` is None (unencrypted), 'gcm128', 'gcm256'
    or 'chacha'; ``hash_digest`` a function of bytes; nonces come from ``nonce(data, key)`` so
    that sealed bodies are reproducible."""

    def __init__(self, cipher, hash_digest, shared_key=b'', kdf_params=b'', userkey=None, oracle=None):
        self.cipher, self.hash_digest = cipher, hash_digest
        self.shared_key, self.kdf_params, self.userkey = shared_key, kdf_params, userkey
        self.oracle = oracle
        self.key_bytes = 16 if cipher == 'gcm128' else 32

    @property
    def encrypted(self):
        return self.cipher is not None

    def derive_shared_subkey(self, context):
        return hashlib.blake2b(context, salt=self.kdf_params, key=self.shared_key,
                               digest_size=self.key_bytes).digest()

    def encrypt(self, data, key):
        nonce = hashlib.blake2b(bytes(data[:64]) + key, digest_size=12).digest()
        if self.cipher == 'chacha':
            return nonce + chacha_ref.seal(key, nonce, data)
        return nonce + self.oracle.gcm_encrypt(key, nonce, data)

    def decrypt(self, data, key):
        try:
            if self.cipher == 'chacha':
                return chacha_ref.open_(key, data[:12], data[12:])
            return self.oracle.gcm_decrypt(key, data[:12], data[12:])
        except ValueError as e:
            raise DecryptionError(str(e)) from e


def encrypt_snapshot_body(repo, snapshot_body) -> bytes:
    if repo.encrypted:
        encrypted_private_data = repo.encrypt(serialize(snapshot_body['data']), repo.userkey)
        encrypted_body = {
            'chunks': repo.encrypt(serialize(snapshot_body['chunks']),
                                   repo.derive_shared_subkey(repo.hash_digest(encrypted_private_data))),
            'data': encrypted_private_data,
        }
    else:
        encrypted_body = snapshot_body
    return serialize(encrypted_body)


def decrypt_snapshot_body(repo, contents, userkey=None):
    """``userkey``: the key of the reader (default: the repository's own)."""
    body = deserialize(contents)
    if repo.encrypted:
        body['chunks'] = deserialize(
            repo.decrypt(body['chunks'], repo.derive_shared_subkey(repo.hash_digest(body['data']))))
        try:
            data = repo.decrypt(body['data'], repo.userkey if userkey is None else userkey)
        except DecryptionError:
            body['data'] = None
        else:
            body['data'] = deserialize(data)
    return body


def seal_table(repo, table_text: bytes, data) -> bytes:
    """A snapshot file whose ``chunks`` plaintext is ``table_text`` as given (canonical or not)."""
    if not repo.encrypted:
        return b'{"chunks":' + table_text + b',"data":' + serialize(data) + b'}'
    encrypted_private_data = repo.encrypt(serialize(data), repo.userkey)
    return serialize({
        'chunks': repo.encrypt(table_text, repo.derive_shared_subkey(repo.hash_digest(encrypted_private_data))),
        'data': encrypted_private_data,
    })
