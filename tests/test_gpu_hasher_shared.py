"""The staging every hasher shares (replicat_amd/csrc/capi_digest.cpp), through the three
algorithms: device digests queued back to back on one handle reuse its two staging slots, and every
digest still lands in its own slot of its own call's output.  Runs on an MI355X only (-m gpu)."""
import hashlib
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():  # pragma: no cover - CPU container
    pytest.skip('needs an MI355X', allow_module_level=True)

from replicat_amd.hashing import SLOT, GpuBlake2b, GpuSha2, GpuSha3  # noqa: E402

LENS = [0, 1, 129, 20_000]  # empty, one byte, a byte past BLAKE2b's block and SHA-256's second, long
CALLS = 3                   # the third call takes the first one's slot and waits on its event
FRAME = 64                  # keeps the output slots 64-byte aligned inside the frame

ALGOS = {'blake2b-64': (lambda: GpuBlake2b(length=64), lambda m: hashlib.blake2b(m, digest_size=64).digest()),
         'sha2-256': (lambda: GpuSha2(bits=256), lambda m: hashlib.sha256(m).digest()),
         'sha3-256': (lambda: GpuSha3(bits=256), lambda m: hashlib.sha3_256(m).digest())}


@pytest.mark.parametrize('name', sorted(ALGOS))
def test_queued_digests_share_the_staging(name):
    make, ref = ALGOS[name]
    rnd = random.Random(13)
    h = make()
    msgs = [[rnd.randbytes(n) for n in LENS] for _ in range(CALLS)]
    ins = [[torch.from_numpy(np.frombuffer(m or b'\0', dtype=np.uint8).copy()).cuda() for m in call]
           for call in msgs]
    room = len(LENS) * SLOT
    outs = [torch.full((FRAME + room + FRAME,), 0xA5, dtype=torch.uint8, device='cuda') for _ in range(CALLS)]
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    for c in range(CALLS):  # no synchronisation in between
        h.digest_device([t.data_ptr() for t in ins[c]], LENS, outs[c].data_ptr() + FRAME, stream.cuda_stream)
    stream.synchronize()
    for c in range(CALLS):
        raw = outs[c].cpu().numpy().tobytes()
        assert raw[:FRAME] == b'\xa5' * FRAME and raw[FRAME + room:] == b'\xa5' * FRAME
        for i, m in enumerate(msgs[c]):
            slot = raw[FRAME + SLOT * i:FRAME + SLOT * (i + 1)]
            assert slot[:h.digest_size] == ref(m), (c, len(m))
    h.close()
