"""GPU parity of lazy tails (RC_TAIL_ROUNDS): a pipelined, non-END call on the
large-window path reads each stream's tail in rounds on the chain stream, only as far as the
stream's chain gets.  Whatever the number of rounds the cuts are the oracle's, and the rounds
scan exactly the tiles the model of the rounds (lazy_tail_model.py) says -- fewer than the
whole tail, which is the point.

Parameters: the smallest max_length of the parity domain (max % 4 == 0) on the large-window
path -- a window of 62 tiles, capi.cpp's `small` rule -- and min = max / 40."""
import numpy as np
import pytest

import lazy_tail_model as M

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():  # pragma: no cover - CPU container
    pytest.skip('needs an MI355X', allow_module_level=True)

from gpu_util import expected_cuts  # noqa: E402

from replicat_amd import _lib, synth  # noqa: E402
from replicat_amd.chunker import GpuChunker, fill_splitmix  # noqa: E402

import ctypes  # noqa: E402

TILE = M.tile_keys()
MX = 1_015_812
MN = MX // 40
KEY = b'\xff' * 16
assert ((MX - 1) // 4) // TILE + 3 > 64 and ((MX - 4 - 1) // 4) // TILE + 3 <= 64
LENGTHS = (2 * MX - 4, 2 * MX, 2 * MX + (16 << 10), 3 * MX + 4, 5 * MX, 8 * MX + 12)
ROUNDS = (0, 1, 2, 4)


@pytest.fixture(autouse=True)
def _own_stream(monkeypatch):
    """A non-blocking caller stream (the NULL stream would serialise with the chunker's),
    every pipelined request on the masked streams, however small, and every stream one chain
    segment (segments of at least 8 max_lengths: at the default floor of 2 a batch this small
    splits its 8 x max streams, and a call with a split stream is not lazy)."""
    monkeypatch.setenv('RC_PIPE_ALL', '1')
    monkeypatch.setenv('RC_SEGMENT_FLOOR', '8')
    # the library keeps batches of streams this short off the lazy path (their rounds would not
    # fit beside the next body launch): lift the bound, the rounds are what is tested here
    monkeypatch.setenv('RC_TAIL_SHARE', str(1 << 30))
    with torch.cuda.stream(torch.cuda.Stream()):
        yield
    torch.cuda.synchronize()


def _hs():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope='module')
def batch():
    """32 streams: five splitmix streams of each length, an all-zero stream (every tile a
    marker: the edge kernel works in every round) and a stream whose last piece starts inside
    its final max_length bytes.  Device tensors, host bytes, the oracle's cuts."""
    sizes, last, datas = [], [], []
    for i in range(30):
        L = LENGTHS[i % len(LENGTHS)]
        sizes.append(L)
        last.append(0)
        datas.append(synth.stream_bytes(L, synth.DEFAULT_SEED, i))
    sizes.append(4 * MX)
    last.append(0)
    datas.append(np.zeros(4 * MX, np.uint8))
    L = 5 * MX
    sizes.append(L)
    last.append(L - MX // 2)
    datas.append(synth.stream_bytes(L, synth.DEFAULT_SEED, 31))
    ts = []
    with torch.cuda.stream(torch.cuda.Stream()):
        for i, n in enumerate(sizes):
            t = torch.zeros(n + 16, dtype=torch.uint8, device='cuda')
            if i != 30:
                fill_splitmix(t.data_ptr(), n, synth.DEFAULT_SEED, i, _hs())
            ts.append(t)
        torch.cuda.synchronize()
    exp = expected_cuts(datas, MN, MX, KEY, last)
    return ts, sizes, last, exp


def _model(batch, K):
    _, sizes, last, exp = batch
    return [M.rounds(e, MX, L, P, K) for e, L, P in zip(exp, sizes, last)]


def test_cases_occur(batch):
    """The seed's streams finish after round 1, round 2, round 3 and only in the closing round
    of four (and the 2 x max - 4 streams, which the tail rule alone cuts, before any)."""
    fin = [m['finished'] for m in _model(batch, 4)]
    print('finishing rounds (K = 4):', fin)
    for r in (1, 2, 3, 4):
        assert r in fin, (r, fin)
    assert _model(batch, 4)[30]['finished'] == 4  # minimum-length chunks: a tile per round


def _run(ch, batch, calls=1, end=True):
    """`calls` pipelined non-END calls sharing the output arrays, then (end) an END call;
    returns the cut lists of the last call, and the tail rounds' scanned-tile counts of the
    last non-END call."""
    ts, sizes, last, _ = batch
    total, caps = ch.capacity(sizes)
    cuts = torch.zeros(total, dtype=torch.int64, device='cuda')
    counts = torch.zeros(len(sizes), dtype=torch.int64, device='cuda')
    ptrs = [t.data_ptr() for t in ts]
    for _ in range(calls):
        ch.chunk_device(ptrs, sizes, last, cuts.data_ptr(), counts.data_ptr(), _hs(), pipelined=True)
    r = ctypes.c_uint32()
    s = np.zeros(16, np.uint64)
    assert _lib.lib().rc_chunker_tail_scanned(ch._h, ctypes.byref(r), s.ctypes.data, 16) == 0
    scanned = s[:r.value].tolist()
    ch.wait(_hs())
    torch.cuda.synchronize()
    first = (cuts.cpu().numpy().view(np.uint64).copy(), counts.cpu().numpy().copy())
    if end:
        cuts.zero_()
        counts.zero_()
        ch.chunk_device(ptrs, sizes, last, cuts.data_ptr(), counts.data_ptr(), _hs(), pipelined=True,
                        end=True)
        ch.wait(_hs())
        torch.cuda.synchronize()
        second = (cuts.cpu().numpy().view(np.uint64), counts.cpu().numpy())
        assert (first[1] == second[1]).all() and (first[0] == second[0]).all()
    base = np.concatenate([[0], np.cumsum(caps)[:-1]]).astype(np.int64)
    assert (first[1] >= 0).all()
    return [first[0][b:b + c].tolist() for b, c in zip(base, first[1])], scanned


@pytest.mark.parametrize('K', ROUNDS)
def test_rounds_parity(batch, K, monkeypatch):
    """Every setting gives the oracle's cuts (so all give the same), in a non-END call and the
    END call after it; the rounds scan the tiles the model counts."""
    monkeypatch.setenv('RC_TAIL_ROUNDS', str(K))
    ch = GpuChunker(MN, MX, KEY)
    got, scanned = _run(ch, batch)
    assert ch.pipelined_calls() == 2
    assert got == batch[3]
    assert len(scanned) == K
    if K:
        model = _model(batch, K)
        want = [sum(m['scanned'][r] for m in model) for r in range(K)]
        tail = sum(nt - nb for nt, nb in (M.split(MX, L, P) for L, P in zip(batch[1], batch[2])))
        print(f'K={K}: scanned per round {scanned}, model {want}, tail tiles {tail}')
        assert scanned == want
        # reading less: by the model, chains that finish before the closing round leave tail
        # tiles unread (with the closing round alone, only those the body already settled)
        done_early = any(m['finished'] < K and nt > m['read_hi'] for m, (nt, _) in zip(
            model, (M.split(MX, L, P) for L, P in zip(batch[1], batch[2]))))
        if K > 1:
            assert done_early and sum(scanned) < tail
    ch.close()


def test_back_to_back(batch, monkeypatch):
    """Three lazy calls in flight on the two workspaces, sharing their output arrays."""
    monkeypatch.setenv('RC_TAIL_ROUNDS', '4')
    ch = GpuChunker(MN, MX, KEY)
    got, _ = _run(ch, batch, calls=3)
    assert got == batch[3]
    ch.close()


def test_overflow_in_a_late_round(batch, monkeypatch):
    """A stream whose cut capacity runs out in a late round still reports -1; the streams whose
    cuts fit keep theirs.  (A capacity from rc_cut_capacity never runs out; RC_CUT_CAP_MAX, a
    test switch, lowers the capacity the kernels see.)"""
    ts, sizes, last, exp = batch
    model = _model(batch, 4)
    i = max((k for k, m in enumerate(model) if m['finished'] >= 3 and k != 30),
            key=lambda k: len(exp[k]))
    cap = len(exp[i]) - 1
    monkeypatch.setenv('RC_TAIL_ROUNDS', '4')
    monkeypatch.setenv('RC_CUT_CAP_MAX', str(cap))
    ch = GpuChunker(MN, MX, KEY)
    total, caps = ch.capacity(sizes)
    cuts = torch.zeros(total, dtype=torch.int64, device='cuda')
    counts = torch.zeros(len(sizes), dtype=torch.int64, device='cuda')
    ch.chunk_device([t.data_ptr() for t in ts], sizes, last, cuts.data_ptr(), counts.data_ptr(),
                    _hs(), pipelined=True)
    ch.wait(_hs())
    torch.cuda.synchronize()
    k = counts.cpu().numpy()
    c = cuts.cpu().numpy().view(np.uint64)
    base = np.concatenate([[0], np.cumsum(caps)[:-1]]).astype(np.int64)
    assert k[i] == -1
    for j, e in enumerate(exp):
        if len(e) > cap:
            assert k[j] == -1, j
        else:
            assert c[base[j]:base[j] + k[j]].tolist() == e, j
    ch.close()
