"""VALU instructions per block of the SHA digest kernels, from the gfx950 ISA (no GPU needed):

    python scripts/sha_isa.py [--out profiles/sha/isa.json]

Compiles sha2.hip and sha3.hip to assembly with the library's flags and reads, per digest kernel,
the body loop of the message walk: its straight part (loads, funnel, byte swaps, the first 16
rounds of SHA-2 / the absorb of SHA-3) plus its round loop times the trip count (3 x 16 rounds
for SHA-256, 4 x 16 for SHA-512, 24 rounds of Keccak-f).  The round loop is the first basic block
that branches to itself; the straight part is the block before it.  For the 25-lane form of
SHA-3 (rc_sha3_split_kernel) the round loop is the self-branching block that holds
ds_bpermute_b32, counted per lane with its cross-lane reads beside the VALU.  Also reports each
kernel's registers, scratch and spills as the compiler states them.  scripts/sha_probe.py reads
the JSON this writes.
"""
import collections
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from replicat_amd import build  # noqa: E402

TRIPS = {'rc_sha256_kernel': 3, 'rc_sha512_kernel': 4, 'rc_sha3_kernel': 24, 'rc_sha3_split_kernel': 24}
BLOCK = {'rc_sha256_kernel': 64, 'rc_sha512_kernel': 128}


def assembly(name):
    out = os.path.join(tempfile.gettempdir(), f'rc_{name}_isa.s')
    flags = [f for f in build.FLAGS if f not in ('-shared',)]
    subprocess.run([build.hipcc(), *flags, '-I', os.path.join(ROOT, 'include'), '-S', '--cuda-device-only',
                    os.path.join(build.CSRC, name + '.hip'), '-o', out], check=True,
                   stderr=subprocess.DEVNULL)
    return open(out).read().split('\n')


def kernels(lines):
    """name -> (list of (label, instructions), metadata dict) for every kernel of one file."""
    ends = [k for k, l in enumerate(lines) if l.startswith('.Lfunc_end')]
    res = {}
    for i, l in enumerate(lines):
        m = re.match(r'^(_Z\d+(rc_\w+?_kernel)\S*):', l)
        if not m:
            continue
        end = next((k for k in ends if k > i), None)
        if end is None:
            continue
        cur, blks = None, []
        for ln in lines[i:end]:
            mm = re.match(r'^(\.LBB\d+_\d+|_Z\S+):', ln)
            if mm:
                cur = (mm.group(1), [])
                blks.append(cur)
            elif cur and ln.startswith('\t') and not ln.strip().startswith((';', '.')):
                cur[1].append(ln.strip())
        rate = re.search(r'ILj(\d+)E', m.group(1))
        meta = {}
        for ln in lines[end:end + 80]:
            mm = re.match(r'\s*\.amdhsa_next_free_vgpr (\d+)', ln) or re.match(
                r'; (ScratchSize|NumVgprs|NumAgprs|sgpr_spill_count|vgpr_spill_count|Occupancy): (\d+)', ln)
            if mm and len(mm.groups()) == 2:
                meta[mm.group(1)] = int(mm.group(2))
        res[m.group(2) + (f'<{rate.group(1)}>' if rate else '')] = (blks, meta)
    return res


def valu(ins):
    return sum(1 for x in ins if x.startswith('v_'))


def self_loops(blks):
    for k, (label, ins) in enumerate(blks):
        if any(x.startswith('s_cbranch') and x.split()[-1] == label for x in ins):
            yield k


def main():
    out = None
    if '--out' in sys.argv:
        out = sys.argv[sys.argv.index('--out') + 1]
    result = {'flags': ' '.join(build.FLAGS), 'kernels': {}}
    lines_of = {src: assembly(src) for src in ('sha2', 'sha3')}
    for src in ('sha2', 'sha3'):
        for name, (blks, meta) in kernels(lines_of[src]).items():
            base = name.split('<')[0]
            entry = {'registers': meta}
            if base in TRIPS:
                loops = list(self_loops(blks))
                lane = next(k for k in loops if len(blks[k][1]) > 100
                            and not any(x.startswith('ds_bpermute') for x in blks[k][1]))
                straight, loop = blks[lane - 1][1], blks[lane][1]
                entry['lane'] = {'straight_valu': valu(straight), 'loop_valu': valu(loop), 'trips': TRIPS[base],
                                 'valu_per_block': valu(straight) + TRIPS[base] * valu(loop),
                                 'bitop3': collections.Counter(x.split()[0] for x in loop)['v_bitop3_b32']}
                if base == 'rc_sha3_split_kernel':
                    grp = next(k for k in loops if any(x.startswith('ds_bpermute') for x in blks[k][1]))
                    ins = blks[grp][1]
                    entry['group'] = {'loop_valu': valu(ins), 'loop_bpermute': sum(
                        1 for x in ins if x.startswith('ds_bpermute')), 'loop_instructions': len(ins),
                        'trips': 24}
            if base in ('rc_sha256_split_kernel', 'rc_sha512_split_kernel'):
                # the latency form's two loops: the schedule (LDS writes) and the rounds alone
                # (LDS reads), 16 rounds per trip each
                loops = [blks[k][1] for k in self_loops(blks)]
                sched = next(x for x in loops if any(i.startswith('ds_write') for i in x))
                rnds = next(x for x in loops if any(i.startswith('ds_read') for i in x))
                entry['wave'] = {'schedule_loop_valu': valu(sched), 'rounds_loop_valu': valu(rnds),
                                 'rounds_loop_lds_reads': sum(1 for i in rnds if i.startswith('ds_read'))}
            result['kernels'][name] = entry
        # spills and the AGPRs among the registers, from the code object's metadata notes
        cur = None
        for ln in lines_of[src]:
            m = re.match(r'\s+\.name:\s+_Z\d+(rc_\w+?_kernel)(\S*)', ln)
            if m:
                rate = re.search(r'ILj(\d+)E', m.group(2))
                cur = m.group(1) + (f'<{rate.group(1)}>' if rate else '')
            m = re.match(r'\s+\.(sgpr_spill_count|vgpr_spill_count|vgpr_count|agpr_count):\s+(\d+)', ln)
            if m and cur in result['kernels']:
                result['kernels'][cur]['registers'][m.group(1)] = int(m.group(2))
    line = json.dumps(result, indent=1, sort_keys=True)
    if out:
        os.makedirs(os.path.dirname(out) or '.', exist_ok=True)
        with open(out, 'w') as f:
            f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
