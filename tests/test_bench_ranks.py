"""bench.main's N > 1 control flow on the CPU: world size 2 over gloo (what bench.py uses on the
GPU box too -- the data path has no collective), with the device calls replaced by a CPU
stand-in whose chunker is the oracle.  Checks device selection per LOCAL_RANK, the shards each
rank fills and chunks, the weak-scaling value formula, the max-over-ranks timing, per-rank
parity gathering, and config 3 (ii)'s split + gather + splice of one stream over two ranks."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import bench
from bench_standin import CpuBackend

GIB = 1 << 30


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, argv, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), WORLD_SIZE=str(world),
                      RANK=str(rank), LOCAL_RANK=str(rank))
    try:
        res = bench.main(argv, backend=CpuBackend)
        last = bench.LAST
        ends = [np.asarray(e).tolist() for e in last['ends']] if last.get('ends') is not None else None
        q.put((rank, res, last['device'], ends, last['parity']))
    except Exception as e:  # noqa: BLE001 - report to the parent
        q.put((rank, repr(e), None, None, None))
        raise


def _run(argv, world=2):
    port = _free_port()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, argv, q)) for r in range(world)]
    for p in procs:
        p.start()
    out = sorted((q.get(timeout=300) for _ in procs), key=lambda r: r[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return out


def test_config2_two_ranks():
    n, mib, steps = 3, 1, 2
    out = _run(['--full', '--gpus', '2', '--config', '2', '--streams', str(n), '--stream-mib', str(mib),
                '--steps', str(steps), '--warmup', '1', '--cpu-streams', '0', '--min-length', '2000',
                '--max-length', '80000'])
    from oracle import oracle as o
    from replicat_amd import synth
    (r0, res0, dev0, ends0, _), (r1, res1, dev1, ends1, _) = out
    assert (dev0, dev1) == (0, 1)                              # device = LOCAL_RANK
    assert isinstance(res0, dict) and res1 is None             # rank 0 prints the line
    assert res0['n_gpus'] == 2 and res0['scaling'] == 'weak'
    size = mib << 20
    # value = all ranks' bytes / the slowest rank's time
    per_step = res0['ms_per_step'] / 1e3
    # both rounded (value to 0.01 GiB/s: a loaded host makes these tiny streams ~0.2 GiB/s)
    assert res0["value"] == pytest.approx(2 * n * size / per_step / GIB, rel=1e-2, abs=0.006)
    # kernel times are the max over ranks of the stand-in's per-call figures
    assert res0['roofline']['kernel_ms'] == pytest.approx(1.0)
    assert res0['roofline']['chain_kernel_ms'] == pytest.approx(0.2)
    # each rank chunked its own shard: stream ids rank * n ..
    for rank, ends in ((0, ends0), (1, ends1)):
        ids = bench.shard_ids('2', rank, n)
        assert ids == list(range(rank * n, rank * n + n))
        for i, e in zip(ids, ends):
            data = synth.stream_bytes(size, synth.DEFAULT_SEED, i)
            assert e == o.chunk_stream(data, 2000, 80000, None, 0)


def test_config3ii_split_over_two_ranks():
    """One stream split in two windows, chunked per rank, gathered and spliced: every rank ends
    with the whole true cut list of the stream."""
    mib = 4
    out = _run(['--full', '--gpus', '2', '--config', '3ii', '--stream-mib', str(mib), '--steps', '1',
                '--warmup', '0', '--cpu-streams', '0', '--min-length', '2000', '--max-length', '80000'])
    from oracle import oracle as o
    from replicat_amd import synth
    L = 2 * (mib << 20)
    exp = o.chunk_stream(synth.stream_bytes(L, synth.DEFAULT_SEED, 0), 2000, 80000, None,
                         L - (1 << 20))
    for _, res, _, ends, _ in out:
        assert ends[0] == exp
    assert out[0][1]['config']['parallelism'] == 'one stream split over 2 ranks'


def test_parity_flags_gathered_for_config4():
    """Config 4's parity is the AND of every rank's own-shard check; a workload the fixtures do
    not cover (here 2 x 1 MiB per rank) carries no flag on any rank and none in the line."""
    out = _run(['--gpus', '2', '--config', '4', '--streams', '2', '--stream-mib', '1', '--steps', '1',
                '--warmup', '0', '--cpu-streams', '0'])
    (_, res0, _, ends0, p0), (_, _, _, ends1, p1) = out
    assert p0 is None and p1 is None  # not the config-4 sizes: no fixture, no flag
    assert res0['parity_sha256'] is None
    # round-robin shards: rank r holds streams r, r + 8
    assert bench.shard_ids('4', 1, 2) == [1, 9]


# ------------------------------------------------ bench.py --gpus N as its own launcher

STANDIN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'bench_standin.py')
SMALL = ['--config', '2', '--streams', '2', '--stream-mib', '1', '--steps', '1', '--warmup', '0',
         '--cpu-streams', '0', '--min-length', '2000', '--max-length', '80000']


def _cli(args, **env_over):
    """bench.py's command line (bench.cli) over the CPU stand-in, in a fresh process, with no
    launcher around it: the JSON line (or None) and the exit status."""
    import json
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items()
           if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    env.update(env_over)
    p = subprocess.run([sys.executable, STANDIN] + args, capture_output=True, text=True,
                       env=env, timeout=300)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{')]
    return (json.loads(lines[-1]) if lines else None), p.returncode, p.stderr


def test_gpus_n_starts_n_ranks():
    """`bench.py --gpus 2` with no launcher runs two ranks on two distinct devices."""
    line, rc, err = _cli(['--gpus', '2'] + SMALL)
    assert rc == 0, err[-2000:]
    assert line['n_gpus'] == 2 and line['ranks_seen'] == 2
    assert line['distinct_devices'] == 2 and len(set(line['devices'])) == 2
    assert line['shared_devices'] is False
    assert [r['rank'] for r in line['per_rank']] == [0, 1]
    assert [r['device'] for r in line['per_rank']] == [0, 1]
    assert all(r['tile_kernel_ms'] == pytest.approx(1.0) for r in line['per_rank'])
    assert line['roofline']['frac'] is not None


def test_gpus_one_runs_in_process():
    line, rc, err = _cli(['--gpus', '1'] + SMALL)
    assert rc == 0, err[-2000:]
    assert line['n_gpus'] == 1 and line['distinct_devices'] == 1 and len(line['per_rank']) == 1


def test_shared_devices_refused():
    """Two ranks, one device: exits non-zero and prints no metric line."""
    line, rc, _ = _cli(['--gpus', '2'] + SMALL, RC_STANDIN_DEVICES='1')
    assert rc != 0 and line is None


def test_shared_devices_rehearsal_has_no_roofline():
    line, rc, err = _cli(['--gpus', '2', '--share-gpus'] + SMALL, RC_STANDIN_DEVICES='1')
    assert rc == 0, err[-2000:]
    assert line['n_gpus'] == 2 and line['shared_devices'] is True
    assert line['distinct_devices'] == 1
    r = line['roofline']
    assert r['frac'] is None and r['frac_read'] is None and r['achieved'] is None
    assert 'share a device' in r['note']


def test_world_size_must_match_gpus():
    """A launcher's world size that is not --gpus: exit status 3, no line."""
    line, rc, err = _cli(['--gpus', '2'] + SMALL, WORLD_SIZE='1', RANK='0', LOCAL_RANK='0')
    assert rc == 3 and line is None
    assert '--gpus 2' in err


def test_pipelined_line_fields():
    """The default line: steps are pipelined requests (RC_PIPELINED), the reserve and the
    number that overlapped are reported with the same steps' unpipelined time, and the roofline
    says what its edge / chain times mean then; --pipeline off reports plain sequential steps."""
    line, rc, err = _cli(['--gpus', '1', '--full'] + SMALL[:-10] + ['--steps', '3', '--warmup', '1']
                         + SMALL[-6:])
    assert rc == 0, err[-2000:]
    p = line['pipeline']
    assert p['on'] is True and p['reserve_cus'] == 32 and p['pipelined_steps'] == 3
    assert p['unpipelined_ms_per_step'] is not None and 'every step still computes' in p['note']
    assert 'pipelined steps' in line['roofline']['timing_note']
    line, rc, err = _cli(['--gpus', '1', '--pipeline', 'off'] + SMALL)
    assert rc == 0, err[-2000:]
    assert line['pipeline'] == {'on': False}
    assert 'timing_note' not in line['roofline']


# ------------------------------------------------ every rank's parity, the CPU share per rank

SHARD = ['--config', '2', '--streams', '2', '--stream-mib', '16', '--steps', '1', '--warmup', '0']


def test_every_rank_checked_against_its_own_shard():
    """Two ranks x 2 streams of 16 MiB at replicat's default parameters: tests/golden/ranks.json
    ('small') holds the reference's cut-list digest of every rank's OWN shard (streams r*2 ..),
    so both ranks carry a flag and the line's is their AND (VERDICT r3 Missing #1)."""
    out = _run(SHARD + ['--gpus', '2', '--full', '--cpu-streams', '0'])
    (_, res0, _, _, p0), (_, _, _, _, p1) = out
    assert p0 is True and p1 is True
    assert [r['parity'] for r in res0['per_rank']] == [True, True]
    assert res0['parity_sha256'] is True
    assert 'rank 1: streams 2..3' in res0['parity_scope']


def test_line_parity_is_the_and_over_ranks():
    mk = lambda flags: [{'rank': i, 'parity': f, 'parity_scope': f'scope {i}'}  # noqa: E731
                        for i, f in enumerate(flags)]
    assert bench.line_parity(mk([True, True]), 2)[0] is True
    assert bench.line_parity(mk([True, False]), 2)[0] is False
    flag, scope = bench.line_parity(mk([True, None]), 2)
    assert flag is None and '[1]' in scope  # one unchecked rank: the line is not 'true'
    assert bench.line_parity(mk([False]), 1) == (False, 'scope 0')


def test_cpu_baseline_scales_with_ranks():
    """The CPU baseline runs on N x the per-GPU host-core share (OMP_NUM_THREADS per GPU)."""
    for gpus in (1, 2):
        line, rc, err = _cli(['--gpus', str(gpus), '--full'] + SHARD + ['--cpu-streams', '2'],
                             OMP_NUM_THREADS='1')
        assert rc == 0, err[-2000:]
        cpu = line['cpu_baseline']
        assert cpu['cores'] == gpus, cpu
        assert f'{gpus} GPU(s) x OMP_NUM_THREADS 1' in cpu['cores_basis']
        assert cpu['matches_gpu'] is True
        assert line['parity_sha256'] is True


# ------------------------------------------------ the plain line, --full, --dump-outputs

def test_plain_line_is_lean_and_full_adds_the_rest():
    """A plain run times its steps and prints the headline fields; the parity check, the
    unpipelined steps and the CPU baseline are --full's, and null without it."""
    args = ['--gpus', '1'] + SHARD[:-4] + ['--steps', '2', '--warmup', '1']
    line, rc, err = _cli(args)
    assert rc == 0, err[-2000:]
    assert line['full'] is False and line['steps'] == 2
    assert line['metric'] == 'GiB/s chunked, device-resident streams'
    assert line['unit'] == 'GiB/s' and line['higher_is_better'] is True and line['dtype'] == 'u8'
    assert line['ms_per_step'] > 0
    assert line['value'] == pytest.approx(2 * (16 << 20) / (line['ms_per_step'] / 1e3) / GIB,
                                          rel=1e-2, abs=0.006)
    assert line['cpu_baseline'] is None and line['parity_sha256'] is None
    assert line['pipeline']['unpipelined_ms_per_step'] is None
    full, rc, err = _cli(args + ['--full', '--cpu-streams', '1'])
    assert rc == 0, err[-2000:]
    assert full['full'] is True and full['parity_sha256'] is True
    assert full['cpu_baseline']['matches_gpu'] is True
    assert full['pipeline']['unpipelined_ms_per_step'] is not None
    for k in ('metric', 'unit', 'higher_is_better', 'dtype', 'steps', 'config'):
        assert full[k] == line[k]


def test_dump_outputs_are_the_last_steps_cuts(tmp_path):
    """--dump-outputs writes the cut lists the timed path left (float64 .npy), the same on every
    run with the same arguments, and they are the oracle's."""
    from oracle import oracle as o
    from replicat_amd import synth
    n, size = 3, 1 << 20
    args = ['--gpus', '1', '--config', '2', '--streams', str(n), '--stream-mib', '1', '--steps', '2',
            '--warmup', '0', '--min-length', '2000', '--max-length', '80000']
    got = []
    for d in ('a', 'b'):
        line, rc, err = _cli(args + ['--dump-outputs', str(tmp_path / d)])
        assert rc == 0, err[-2000:]
        assert line['parity_sha256'] is None  # dumping does not turn the checks on
        got.append({f: np.load(tmp_path / d / f) for f in sorted(os.listdir(tmp_path / d))})
    a, b = got
    assert sorted(a) == ['counts.npy', 'cut_streams.npy', 'cuts.npy']
    assert all(v.dtype == np.float64 for v in a.values())
    assert all(np.array_equal(a[k], b[k]) for k in a)
    exp = [o.chunk_stream(synth.stream_bytes(size, synth.DEFAULT_SEED, i), 2000, 80000, None, 0)
           for i in range(n)]
    assert a['counts.npy'].tolist() == [len(e) for e in exp]
    assert a['cut_streams.npy'].tolist() == [0, 1, 2]
    assert a['cuts.npy'].tolist() == [c for e in exp for c in e]


def test_dump_outputs_samples_a_large_output(tmp_path, monkeypatch):
    """Past DUMP_MAX_VALUES cut ends, a fixed seeded sample of whole streams is written."""
    ends = [np.arange(1, k + 2, dtype=np.uint64) for k in range(40)]
    monkeypatch.setattr(bench, 'DUMP_MAX_VALUES', 100)
    bench.dump_outputs(str(tmp_path / 'a'), ends)
    bench.dump_outputs(str(tmp_path / 'b'), ends, rank=1)
    counts, pick, cuts = (np.load(tmp_path / 'a' / f'{k}.npy') for k in ('counts', 'cut_streams', 'cuts'))
    assert counts.tolist() == list(range(1, 41))
    assert 0 < len(cuts) <= 100 and len(pick) < 40
    assert cuts.tolist() == [c for i in pick.astype(int) for c in ends[i].tolist()]
    assert np.array_equal(pick, np.load(tmp_path / 'b' / 'cut_streams_rank1.npy'))
