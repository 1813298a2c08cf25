"""Regenerate tests/golden/snapshot_bodies.json from the reference's own serialisation hooks.

    PYTHONPATH=/root/reference PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_snapshot_golden.py

``replicat.utils.type_hint`` and ``type_reverse`` are imported from the reference checkout;
``Repository.serialize`` / ``deserialize`` (replicat/repository.py:434-444) are restated here as
their single json.dumps / json.loads calls over those hooks, because replicat.repository itself
needs packages this project does not (sty).  The fixture holds data only: snapshot bodies as hex
of the random inputs, and the serialised bytes the reference's hooks give for them.
"""
import json
import os
import random

from replicat import utils

HERE = os.path.dirname(os.path.abspath(__file__))


def serialize(obj):
    return bytes(json.dumps(obj, separators=(',', ':'), default=utils.type_hint), 'ascii')


def deserialize(data):
    return json.loads(data, object_hook=utils.type_reverse)


def main():
    rnd = random.Random(434)
    cases = []
    for width in (1, 2, 3, 20, 28, 32, 48, 64):
        for count in (0, 1, 2, 5):
            chunks = [rnd.randbytes(width) for _ in range(count)]
            data = {'files': [{'path': f'/f{i}]', 'chunks': [{'range': [0, 7 + i], 'index': i, 'counter': 0}],
                               'digest': rnd.randbytes(width)} for i in range(count)],
                    'utc_timestamp': '2024-01-01T00:00:00', 'note': None}
            body = {'chunks': chunks, 'data': data}
            text = serialize(body)
            assert deserialize(text) == body
            table = serialize(chunks)
            assert deserialize(table) == chunks
            cases.append({'width': width, 'chunks': [c.hex() for c in chunks], 'table': table.decode('ascii'),
                          'body': text.decode('ascii'), 'data': serialize(data).decode('ascii')})
    # an encrypted envelope: two byte strings
    for lens in ((0, 0), (1, 2), (29, 300)):
        blob = {'chunks': rnd.randbytes(lens[0]), 'data': rnd.randbytes(lens[1])}
        text = serialize(blob)
        assert deserialize(text) == blob
        cases.append({'envelope': {k: v.hex() for k, v in blob.items()}, 'body': text.decode('ascii')})
    with open(os.path.join(HERE, 'snapshot_bodies.json'), 'w') as f:
        json.dump({'cases': cases}, f, indent=0)
        f.write('\n')


if __name__ == '__main__':
    main()
