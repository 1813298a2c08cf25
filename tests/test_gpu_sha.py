"""GPU parity of the SHA-2 and SHA-3 chunk digests (replicat_amd/csrc/sha2.hip, sha3.hip through
the C ABI of include/replicat_digest.h) against hashlib -- the implementation replicat's `sha2`
and `sha3` adapters call (replicat/utils/adapters.py:231-254).  Bit-exact.  Runs on an MI355X
only (-m gpu).

Both families have two forms -- one lane per message, and a latency form for long messages (SHA-3:
one state over 25 lanes; SHA-2: one message per wave, the schedule of the blocks ahead on its
other lanes) -- and RC_SHA_LANE_MAX sends every message through either."""
import hashlib
import os
import random
import subprocess
import sys
import textwrap

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():  # pragma: no cover - CPU container
    pytest.skip('needs an MI355X', allow_module_level=True)

from gpu_util import device_streams  # noqa: E402

from replicat_amd import synth  # noqa: E402
from replicat_amd.chunker import GpuChunker  # noqa: E402
from replicat_amd.hashing import SLOT, GpuSha2, GpuSha3, chunk_digest_host  # noqa: E402

HASHLIB = {('sha2', 224): hashlib.sha224, ('sha2', 256): hashlib.sha256,
           ('sha2', 384): hashlib.sha384, ('sha2', 512): hashlib.sha512,
           ('sha3', 224): hashlib.sha3_224, ('sha3', 256): hashlib.sha3_256,
           ('sha3', 384): hashlib.sha3_384, ('sha3', 512): hashlib.sha3_512}
VARIANTS = sorted(HASHLIB)
FOUR = [('sha2', 256), ('sha2', 512), ('sha3', 256), ('sha3', 512)]
# the block of SHA-2, the rate of SHA-3
BLOCK = {('sha2', 224): 64, ('sha2', 256): 64, ('sha2', 384): 128, ('sha2', 512): 128,
         ('sha3', 224): 144, ('sha3', 256): 136, ('sha3', 384): 104, ('sha3', 512): 72}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cur_stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope='module')
def hashers():
    hs = {(n, b): (GpuSha2 if n == 'sha2' else GpuSha3)(bits=b) for n, b in VARIANTS}
    yield hs
    for h in hs.values():
        h.close()


@pytest.fixture(scope='module')
def boundary_msgs():
    """Every length 0..300 (each padding boundary of every variant: 55/56/64, 111/112/128,
    rate - 1, rate, 2 x rate for the four rates) and the 1 KiB / 4 KiB neighbours."""
    rnd = random.Random(1)
    return [rnd.randbytes(n) for n in list(range(0, 301)) + [1023, 1024, 1025, 4095, 4096, 4097]]


@pytest.fixture(scope='module')
def random_msgs():
    rnd = random.Random(5)
    msgs = [rnd.randbytes(rnd.choice([rnd.randrange(0, 600), rnd.randrange(0, 200_000)]))
            for _ in range(297)]
    return msgs + [rnd.randbytes(rnd.randrange((1 << 20) - 300, (1 << 20) + 300)) for _ in range(3)]


def test_fips_abc(hashers):
    want = {('sha2', 224): '23097d22', ('sha2', 256): 'ba7816bf', ('sha2', 384): 'cb00753f',
            ('sha2', 512): 'ddaf35a1', ('sha3', 224): 'e642824c', ('sha3', 256): '3a985da7',
            ('sha3', 384): 'ec014982', ('sha3', 512): 'b751850b'}
    for v, h in hashers.items():
        d = h.digest(b'abc')
        assert len(d) == v[1] // 8 == h.digest_size and h.bits == v[1]
        assert d.hex().startswith(want[v]), v
        assert d == HASHLIB[v](b'abc').digest()


@pytest.mark.parametrize('name,bits', VARIANTS)
def test_block_boundaries(hashers, boundary_msgs, name, bits):
    got = hashers[name, bits].digest_many(boundary_msgs)
    for m, g in zip(boundary_msgs, got):
        assert g == HASHLIB[name, bits](m).digest(), len(m)


@pytest.mark.parametrize('name,bits', VARIANTS)
def test_many_random_lengths(hashers, random_msgs, name, bits):
    got = hashers[name, bits].digest_many(random_msgs)
    for m, g in zip(random_msgs, got):
        assert g == HASHLIB[name, bits](m).digest(), len(m)


@pytest.mark.parametrize('name,bits', VARIANTS)
def test_empty_null_pointer_and_slot_padding(hashers, name, bits):
    """NULL is allowed for an empty message; a slot's bytes past the digest size are zero."""
    h = hashers[name, bits]
    raw = random.Random(bits).randbytes(500)
    t = torch.tensor(np.frombuffer(raw, dtype=np.uint8), device='cuda')
    out = torch.full((3, SLOT), 0xAB, dtype=torch.uint8, device='cuda')
    h.digest_device([0, t.data_ptr(), 0], [0, 500, 0], out.data_ptr(), cur_stream())
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    size = bits // 8
    empty = HASHLIB[name, bits](b'').digest() + bytes(SLOT - size)
    assert got[0].tobytes() == empty and got[2].tobytes() == empty
    assert got[1].tobytes() == HASHLIB[name, bits](raw).digest() + bytes(SLOT - size)


@pytest.mark.parametrize('name,bits', FOUR)
def test_unaligned_device_buffers(hashers, name, bits):
    """Any start alignment (a stream's tail chunk starts anywhere) and any length."""
    rnd = random.Random(9)
    raw = rnd.randbytes(1 << 17)
    t = torch.tensor(np.frombuffer(raw, dtype=np.uint8), device='cuda')
    blk = BLOCK[name, bits]
    ptrs, lens, exp = [], [], []
    for off in range(0, 64):
        for n in (0, 1, 3, 5, blk - 1, blk, blk + 1, 1000, rnd.randrange(0, 100_000)):
            ptrs.append(t.data_ptr() + off)
            lens.append(n)
            exp.append(HASHLIB[name, bits](raw[off:off + n]).digest())
    out = torch.zeros((len(ptrs), SLOT), dtype=torch.uint8, device='cuda')
    hashers[name, bits].digest_device(ptrs, lens, out.data_ptr(), cur_stream())
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    size = bits // 8
    assert [got[i, :size].tobytes() for i in range(len(exp))] == exp


@pytest.mark.parametrize('name,bits', VARIANTS)
def test_buffer_ending_at_allocation_end(hashers, name, bits):
    """Messages whose last byte is the last byte of their allocation, every tail alignment:
    the kernel never reads past a message's last dword."""
    rnd = random.Random(4)
    sizes = (1, 2, 3, 4, 5, 127, 129, 4093, 4097, 65_535)
    raws = [rnd.randbytes(n) for n in sizes]
    ts = [torch.tensor(np.frombuffer(r, dtype=np.uint8), device='cuda') for r in raws]
    out = torch.zeros((len(sizes), SLOT), dtype=torch.uint8, device='cuda')
    hashers[name, bits].digest_device([t.data_ptr() for t in ts], list(sizes), out.data_ptr(),
                                      cur_stream())
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for i, r in enumerate(raws):
        assert got[i, :bits // 8].tobytes() == HASHLIB[name, bits](r).digest(), sizes[i]


def _chunk_and_digest(ch, hasher, sizes, last):
    ts = device_streams(sizes, seed=synth.DEFAULT_SEED)
    total, caps = ch.capacity(sizes)
    cuts = torch.zeros(max(total, 1), dtype=torch.int64, device='cuda')
    counts = torch.zeros(len(sizes), dtype=torch.int64, device='cuda')
    dig = torch.zeros((max(total, 1), SLOT), dtype=torch.uint8, device='cuda')
    ptrs = [t.data_ptr() for t in ts]
    ch.chunk_device(ptrs, sizes, last, cuts.data_ptr(), counts.data_ptr(), cur_stream())
    hasher.digest_chunks(ch, ptrs, sizes, cuts.data_ptr(), counts.data_ptr(), dig.data_ptr(),
                         cur_stream())
    torch.cuda.synchronize()
    cuts_h = cuts.cpu().numpy().view(np.uint64)
    counts_h = counts.cpu().numpy()
    dig_h = dig.cpu().numpy()
    base = np.concatenate([[0], np.cumsum(caps)[:-1]]).astype(np.int64)
    return [(cuts_h[b:b + c].tolist(), dig_h[b:b + c]) for b, c in zip(base, counts_h)]


@pytest.fixture(scope='module')
def stream_bytes():
    memo = {}

    def get(n, i):
        if (n, i) not in memo:
            memo[n, i] = synth.stream_bytes(n, synth.DEFAULT_SEED, i).tobytes()
        return memo[n, i]
    return get


@pytest.mark.parametrize('name,bits', FOUR)
@pytest.mark.parametrize('mn,mx', [(2_000, 80_000), (4, 64), (60, 200)])
def test_chunk_digests_match_hashlib(hashers, stream_bytes, mn, mx, name, bits):
    rnd = random.Random(mn)
    sizes = [0, 1, 5, 4096, 3 * mx + 7, 2 * mx - 1] + [rnd.randrange(0, 6 * mx) for _ in range(12)]
    sizes = [min(s, 4 << 20) for s in sizes]
    last = [rnd.randrange(0, s + 1) for s in sizes]
    ch = GpuChunker(mn, mx, synth.seeded_key(mn))
    res = _chunk_and_digest(ch, hashers[name, bits], sizes, last)
    size = bits // 8
    for i, (n, (ends, dig)) in enumerate(zip(sizes, res)):
        data = stream_bytes(n, i)
        assert (ends[-1] if ends else 0) == n
        prev = 0
        for k, e in enumerate(ends):
            assert dig[k].tobytes() == HASHLIB[name, bits](data[prev:e]).digest() + bytes(SLOT - size), \
                (i, k, prev, e)
            prev = e


@pytest.mark.parametrize('name,bits', [('sha2', 512), ('sha3', 256)])
def test_negative_count_contributes_nothing(hashers, name, bits):
    """A stream whose count is negative (rc_chunk_device's overflow / fault marks) has no chunks:
    none of its slots is touched, and its neighbours' digests are right."""
    ch = GpuChunker(60, 200, synth.seeded_key(3))
    sizes = [1000, 1000, 1000]
    rnd = random.Random(3)
    raws = [rnd.randbytes(n) for n in sizes]
    ts = device_streams(sizes, datas=[np.frombuffer(r, dtype=np.uint8) for r in raws])
    total, caps = ch.capacity(sizes)
    base = np.concatenate([[0], np.cumsum(caps)[:-1]]).astype(np.int64)
    ends = [[400, 1000], [300, 1000], [1000]]
    cuts_h = np.zeros(total, dtype=np.uint64)
    for b, e in zip(base, ends):
        cuts_h[b:b + len(e)] = e
    cuts = torch.from_numpy(cuts_h.view(np.int64)).cuda()
    counts = torch.tensor([2, -1, 1], dtype=torch.int64, device='cuda')
    dig = torch.full((total, SLOT), 0xAB, dtype=torch.uint8, device='cuda')
    hashers[name, bits].digest_chunks(ch, [t.data_ptr() for t in ts], sizes, cuts.data_ptr(),
                                      counts.data_ptr(), dig.data_ptr(), cur_stream())
    torch.cuda.synchronize()
    got = dig.cpu().numpy()
    size = bits // 8
    H = HASHLIB[name, bits]
    want = {int(base[0]): H(raws[0][:400]).digest(), int(base[0]) + 1: H(raws[0][400:]).digest(),
            int(base[2]): H(raws[2]).digest()}
    for s in range(total):
        if s in want:
            assert got[s].tobytes() == want[s] + bytes(SLOT - size), s
        else:
            assert got[s].tobytes() == b'\xab' * SLOT, s


@pytest.fixture(scope='module')
def host_path_case(oracle):
    rnd = random.Random(12)
    mn, mx = 2_000, 80_000
    key = synth.seeded_key(12)
    bufs = [np.frombuffer(rnd.randbytes(rnd.randrange(0, 200_000)), dtype=np.uint8) for _ in range(9)]
    last = [rnd.randrange(0, b.size + 1) for b in bufs]
    exp = [oracle.chunk_stream(b, mn, mx, key, P) for b, P in zip(bufs, last)]
    return mn, mx, key, bufs, last, exp


@pytest.mark.parametrize('name,bits', [('sha2', 256), ('sha3', 512)])
def test_chunk_digest_host_path(hashers, host_path_case, name, bits):
    """rc_chunk_digest_host with a SHA hasher = oracle cuts + hashlib digests."""
    mn, mx, key, bufs, last, exp = host_path_case
    ends, digs = chunk_digest_host(GpuChunker(mn, mx, key), hashers[name, bits], bufs, last)
    for b, e, x, d in zip(bufs, ends, exp, digs):
        assert e.tolist() == x
        prev = 0
        for k, c in enumerate(x):
            assert d[k].tobytes() == HASHLIB[name, bits](b[prev:c].tobytes()).digest()
            prev = c


def test_chunk_digest_host_path_many_batches(host_path_case, tmp_path):
    """The same with RC_HOST_BATCH_BYTES=65536, so the ~0.9 MB run through several batches: a
    handle reads its knobs at creation, so the chunker and the hasher are created in a child
    process that has the variable set."""
    mn, mx, key, bufs, last, exp = host_path_case
    case = str(tmp_path / 'case.npz')
    np.savez(case, *bufs)
    code = textwrap.dedent(f'''
        import hashlib, sys
        import numpy as np
        sys.path.insert(0, {ROOT!r})
        import torch  # first, as everywhere in this project: the library binds to torch's HIP runtime
        from replicat_amd.chunker import GpuChunker
        from replicat_amd.hashing import GpuSha2, GpuSha3, chunk_digest_host
        z = np.load({case!r})
        bufs = [z[f'arr_{{i}}'] for i in range({len(bufs)})]
        for h, H in ((GpuSha2(bits=512), hashlib.sha512), (GpuSha3(bits=224), hashlib.sha3_224)):
            ends, digs = chunk_digest_host(GpuChunker({mn}, {mx}, {key!r}), h, bufs, {last!r})
            assert [e.tolist() for e in ends] == {exp!r}
            for b, e, d in zip(bufs, ends, digs):
                prev = 0
                for k, c in enumerate(e.tolist()):
                    assert d[k].tobytes() == H(b[prev:c].tobytes()).digest(), (k, prev, c)
                    prev = c
        print('checked', sum(len(e) for e in ends))
    ''')
    env = dict(os.environ, RC_HOST_BATCH_BYTES='65536')
    r = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.startswith('checked ')


def test_process_exit_with_live_sha_hashers():
    """A fresh child process exits with live hashers of both families (never closed): the exit
    hook destroys them and the status is 0."""
    code = textwrap.dedent(f'''
        import hashlib, sys
        sys.path.insert(0, {ROOT!r})
        import torch  # first: the library binds to torch's HIP runtime
        from replicat_amd.hashing import GpuSha2, GpuSha3
        keep = [GpuSha2(bits=256), GpuSha2(bits=512), GpuSha3(bits=224), GpuSha3(bits=512)]
        assert keep[1].digest(b'abc') == hashlib.sha512(b'abc').digest()
        assert keep[2].digest(b'abc') == hashlib.sha3_224(b'abc').digest()
        print('alive', len(keep), flush=True)
    ''')
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    assert r.stdout.strip() == 'alive 4'


FORMS = {'lane': str(1 << 62), 'latency': '0'}


@pytest.mark.parametrize('form', sorted(FORMS))
def test_knob_forces_every_message_through_one_form(form):
    """One variant per core and rate with RC_SHA_LANE_MAX forcing every message through the lane
    form, and again through the latency form: the same answers as hashlib.  A handle reads its
    knobs at creation, so the handles live in a child process that has the variable set."""
    code = textwrap.dedent(f'''
        import hashlib, random, sys
        import numpy as np
        sys.path.insert(0, {ROOT!r})
        import torch  # first: the library binds to torch's HIP runtime
        from replicat_amd import synth
        from replicat_amd.chunker import GpuChunker
        from replicat_amd.hashing import SLOT, GpuSha2, GpuSha3
        rnd = random.Random(11)
        msgs = [rnd.randbytes(n) for n in list(range(0, 301)) + [1023, 1024, 1025, 4095, 4096, 4097]]
        msgs += [rnd.randbytes(rnd.randrange(0, 200_000)) for _ in range(40)]
        msgs += [rnd.randbytes((1 << 20) + 13)]
        raw = rnd.randbytes(70_000)
        t = torch.tensor(np.frombuffer(raw, dtype=np.uint8), device='cuda')
        hs = torch.cuda.current_stream().cuda_stream
        checked = 0
        for cls, bits, H in ((GpuSha2, 256, hashlib.sha256), (GpuSha2, 512, hashlib.sha512),
                             (GpuSha3, 224, hashlib.sha3_224), (GpuSha3, 256, hashlib.sha3_256),
                             (GpuSha3, 384, hashlib.sha3_384), (GpuSha3, 512, hashlib.sha3_512)):
            h = cls(bits=bits)
            for m, g in zip(msgs, h.digest_many(msgs)):
                assert g == H(m).digest(), (bits, len(m))
            # unaligned device buffers, and messages that end where the allocation ends
            offs = [(o, n) for o in range(0, 9) for n in (0, 1, 7, 8, 9, 71, 72, 73, 143, 144, 145, 1000, 66_000)]
            offs += [(len(raw) - n, n) for n in (1, 2, 3, 4, 5, 127, 129, 4093, 4097, 65_535)]
            out = torch.full((len(offs), SLOT), 0xAB, dtype=torch.uint8, device='cuda')
            h.digest_device([t.data_ptr() + o for o, _ in offs], [n for _, n in offs], out.data_ptr(), hs)
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            for k, (o, n) in enumerate(offs):
                assert got[k].tobytes() == H(raw[o:o + n]).digest() + bytes(SLOT - bits // 8), (bits, o, n)
            # the chunk path
            ch = GpuChunker(2_000, 80_000, synth.seeded_key(2))
            sizes = [300_000, 0, 77]
            ts = [torch.empty(max(n, 1) + 16, dtype=torch.uint8, device='cuda') for n in sizes]
            datas = [rnd.randbytes(n) for n in sizes]
            for x, d in zip(ts, datas):
                if d:
                    x[:len(d)].copy_(torch.from_numpy(np.frombuffer(d, dtype=np.uint8).copy()))
            total, caps = ch.capacity(sizes)
            cuts = torch.zeros(total, dtype=torch.int64, device='cuda')
            counts = torch.zeros(len(sizes), dtype=torch.int64, device='cuda')
            dig = torch.zeros((total, SLOT), dtype=torch.uint8, device='cuda')
            ptrs = [x.data_ptr() for x in ts]
            ch.chunk_device(ptrs, sizes, None, cuts.data_ptr(), counts.data_ptr(), hs)
            h.digest_chunks(ch, ptrs, sizes, cuts.data_ptr(), counts.data_ptr(), dig.data_ptr(), hs)
            torch.cuda.synchronize()
            cuts_h, counts_h, dig_h = cuts.cpu().numpy(), counts.cpu().numpy(), dig.cpu().numpy()
            base = 0
            for d, c, cap in zip(datas, counts_h, caps):
                prev = 0
                for k in range(int(c)):
                    e = int(cuts_h[base + k])
                    assert dig_h[base + k, :bits // 8].tobytes() == H(d[prev:e]).digest(), (bits, k)
                    prev = e
                    checked += 1
                assert prev == len(d)
                base += int(cap)
            h.close()
        print('checked', checked, flush=True)
    ''')
    env = dict(os.environ, RC_SHA_LANE_MAX=FORMS[form])
    r = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.startswith('checked ')


@pytest.mark.parametrize('name,bits', VARIANTS)
def test_batch_of_many_tiny_messages_takes_the_lane_kernel(hashers, name, bits):
    """bytes > 1,024 x longest: the rule sends every message to the lane-only kernel, which no
    other test's batch reaches (the forced lane form runs in the split kernel's lane role)."""
    rnd = random.Random(bits + len(name))
    msgs = [rnd.randbytes(rnd.randrange(0, 65)) for _ in range(6000)] + [rnd.randbytes(64)]
    assert sum(map(len, msgs)) > 64 << 10
    got = hashers[name, bits].digest_many(msgs)
    assert got == [HASHLIB[name, bits](m).digest() for m in msgs]
