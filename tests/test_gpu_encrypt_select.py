"""Encryption of selected chunks only, packed (rc_gcm_encrypt_chunks_select /
rc_chacha_encrypt_chunks_select): offsets and totals against a host computation, every selected
blob against the reference seal (tests/chacha_ref.py, the oracle's AES-GCM) under the key and nonce
of its cut slot, and nothing written past the packed blobs.  Runs on an MI355X only (-m gpu)."""
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():  # pragma: no cover - CPU container
    pytest.skip('needs an MI355X', allow_module_level=True)

import chacha_ref  # noqa: E402

from replicat_amd import synth  # noqa: E402
from replicat_amd.chunker import GpuChunker  # noqa: E402
from replicat_amd.cipher import GpuAesGcm, GpuChaCha20Poly1305  # noqa: E402
from replicat_amd.hashing import SLOT  # noqa: E402

MN, MX = 2_000, 80_000
LENS = [300_000, 299_993, 301_111]
# The select passes work in tiles of 1,024 cut slots (a stream of L bytes has L // 2,000 + 3):
# here stream 1's chunks straddle the first tile boundary (its slots start at 1,021), stream 2's
# sit in the second tile and stream 3's in the third
LENS_TILES = [2_036_000, 300_000, 2_040_001, 299_993]
TILE = 1024
NOT_SELECTED = (1 << 64) - 1


def dev(data):
    return torch.from_numpy(np.frombuffer(bytes(data), dtype=np.uint8).copy()).cuda()


def cut_streams(oracle, LENS):
    """Streams of these lengths, cut on the device once (and checked against the oracle), with a
    key and a nonce per cut slot."""
    rnd = random.Random(sum(LENS))
    datas = [rnd.randbytes(n) for n in LENS]
    ch = GpuChunker(MN, MX, synth.seeded_key(11))
    ts = [dev(d) for d in datas]
    total, caps = ch.capacity(LENS)
    cuts = torch.zeros(total, dtype=torch.int64, device='cuda')
    counts = torch.zeros(len(LENS), dtype=torch.int64, device='cuda')
    ch.chunk_device([t.data_ptr() for t in ts], LENS, None, cuts.data_ptr(), counts.data_ptr(),
                    torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    base = [int(b) for b in np.concatenate([[0], np.cumsum(caps)[:-1]])]
    cuts_h, counts_h = cuts.cpu().numpy().view(np.uint64), [int(c) for c in counts.cpu()]
    ends = [[int(e) for e in cuts_h[base[i]:base[i] + counts_h[i]]] for i in range(len(LENS))]
    for i, data in enumerate(datas):
        assert ends[i] == oracle.chunk_stream(data, MN, MX, synth.seeded_key(11), 0)
    assert min(counts_h) >= 3
    keys_h = np.frombuffer(rnd.randbytes(total * SLOT), dtype=np.uint8).reshape(total, SLOT)
    nonces_h = rnd.randbytes(total * 12)
    state = dict(lens=LENS, ch=ch, ts=ts, datas=datas, total=total, base=base, ends=ends, counts=counts_h,
                 cuts=cuts, keys_h=keys_h, keys=dev(keys_h.tobytes()), nonces_h=nonces_h,
                 nonces=dev(nonces_h), sealed={})
    return state


@pytest.fixture(scope='module')
def cut(oracle):
    state = cut_streams(oracle, LENS)
    yield state
    state['ch'].close()


@pytest.fixture(scope='module')
def cut_tiles(oracle):
    state = cut_streams(oracle, LENS_TILES)
    yield state
    state['ch'].close()


def chunk_of(cut, i, k):
    e = cut['ends'][i]
    return cut['datas'][i][(e[k - 1] if k else 0):e[k]]


def reference_blob(cut, oracle, family, i, k):
    """nonce || C || T of chunk k of stream i under its cut slot's key and nonce, sealed once."""
    memo = cut['sealed']
    if (family, i, k) not in memo:
        s = cut['base'][i] + k
        key, nonce = cut['keys_h'][s, :32].tobytes(), cut['nonces_h'][12 * s:12 * s + 12]
        seal = chacha_ref.seal if family == 'chacha' else oracle.gcm_encrypt
        memo[family, i, k] = nonce + bytes(seal(key, nonce, chunk_of(cut, i, k)))
    return memo[family, i, k]


def selections(cut):
    """name -> (counts as the device sees them, select byte per cut slot)."""
    total, base, counts = cut['total'], cut['base'], cut['counts']
    live = [base[i] + k for i in range(len(counts)) for k in range(counts[i])]
    none, every, alt, last = (np.zeros(total, dtype=np.uint8) for _ in range(4))
    every[:] = 1  # also over slots that hold no chunk: they must not count
    alt[live[::2]] = 7  # any non-zero byte selects
    last[base[-1] + counts[-1] - 1] = 1
    return {'none': (counts, none), 'all': (counts, every), 'alternating': (counts, alt),
            'last_of_last': (counts, last),
            'count_zero': ([counts[0], 0, counts[2]], every),
            'count_negative': ([counts[0], -1, counts[2]], every)}


@pytest.mark.parametrize('case', ['none', 'all', 'alternating', 'last_of_last', 'count_zero',
                                  'count_negative'])
@pytest.mark.parametrize('family', ['chacha', 'gcm'])
def test_encrypt_chunks_select(cut, oracle, family, case):
    run_case(cut, oracle, family, case)


@pytest.mark.parametrize('case', ['all', 'alternating'])
@pytest.mark.parametrize('family', ['chacha', 'gcm'])
def test_select_across_tiles(cut_tiles, oracle, family, case):
    """A layout of three tiles of cut slots: offsets and work-list places carry over from tile to
    tile, within a stream and between streams."""
    base, counts = cut_tiles['base'], cut_tiles['counts']
    assert cut_tiles['total'] > 2 * TILE
    assert base[1] < TILE < base[1] + counts[1] - 1  # stream 1's chunks on both sides
    assert TILE < base[2] < 2 * TILE < base[3]
    run_case(cut_tiles, oracle, family, case)


def run_case(cut, oracle, family, case):
    g = GpuChaCha20Poly1305() if family == 'chacha' else GpuAesGcm()
    counts_h, select_h = selections(cut)[case]
    total, base, ch, LENS = cut['total'], cut['base'], cut['ch'], cut['lens']
    hs = torch.cuda.current_stream().cuda_stream
    out_total, _ = g.chunks_layout(ch, LENS)
    out = torch.full((out_total,), 0xA5, dtype=torch.uint8, device='cuda')
    counts = torch.tensor(counts_h, dtype=torch.int64).cuda()
    select = torch.from_numpy(select_h).cuda()
    blob_off = torch.full((total,), 5, dtype=torch.int64, device='cuda')
    totals = torch.full((2,), 5, dtype=torch.int64, device='cuda')
    g.encrypt_chunks_select(ch, [t.data_ptr() for t in cut['ts']], LENS, cut['cuts'].data_ptr(),
                            counts.data_ptr(), cut['keys'].data_ptr(), cut['nonces'].data_ptr(),
                            select.data_ptr(), out.data_ptr(), blob_off.data_ptr(),
                            totals.data_ptr(), hs)
    torch.cuda.synchronize()
    out_h = out.cpu().numpy()
    off_h = blob_off.cpu().numpy().view(np.uint64).tolist()
    totals_h = totals.cpu().numpy().view(np.uint64).tolist()
    # the host computation: selected chunks back to back in cut-slot order
    expect_off, acc, picked = [NOT_SELECTED] * total, 0, []
    for i in range(len(LENS)):
        for k in range(max(counts_h[i], 0)):
            s = base[i] + k
            if select_h[s]:
                expect_off[s] = acc
                picked.append((i, k, acc))
                acc += len(chunk_of(cut, i, k)) + 28
    assert totals_h == [acc, len(picked)]
    assert off_h == expect_off
    for i, k, o in picked:
        blob = reference_blob(cut, oracle, family, i, k)
        assert out_h[o:o + len(blob)].tobytes() == blob, (i, k)
    assert (out_h[acc:] == 0xA5).all()
    if case == 'none':
        assert acc == 0
    if case == 'last_of_last':
        assert len(picked) == 1 and picked[0][:2] == (2, cut['counts'][2] - 1) and acc > 28
    g.close()
