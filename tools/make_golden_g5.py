"""G5 golden vectors: the REFERENCE'S OWN ab-initio k-mer counter (oracle/_ref/approx_counter,
compiled by `make -C oracle ref` from porechop_abi/ab_initio_src/approx_counter.cpp and the
vendored SeqAn) on seeded synthetic read sets.

Container-only generator. The reference samples reads with std::random_device; every run here
asks for more reads than the file holds (-sn), so the whole set is used and the counts are
deterministic. Inputs (tests/golden/kmer/*.fasta.gz) carry start / end adapters (mutated), N
letters, lower case and short reads (IUPAC letters other than N make the reference's SeqAn
reader throw); parameter sets cover k 12 / 16 / 20, the limit, the
low-complexity threshold, forbidden k-mers, solid k-mers, two runs, and skip-end at verbosity 0
(the reference then recomputes the start into the .end file). Writes tests/golden/g5_kmer.json.gz.

G5-edge (EDGE_RUNS, tests/golden/g5_kmer_edge.json.gz) pins the ends of the k range on a third, small
input (in3: reads of 210-400 bases, poly-T heads on a third of them): k 4 .. 32, among them k = 32 with a
low-complexity threshold that lets the 32-mer TTT...T through (-lc 8: its score is 15.5, the scaled
threshold 32.9). Below k = 4 the reference crashes in errorCount, so there is nothing to record.

A fixture whose content comes out unchanged is left as it is (a gzip header carries the time of writing);
new ones are written without a time.
"""
import gzip
import json
import os
import random
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KDIR = os.path.join(ROOT, 'tests', 'golden', 'kmer')
OUT = os.path.join(ROOT, 'tests', 'golden', 'g5_kmer.json.gz')
OUT_EDGE = os.path.join(ROOT, 'tests', 'golden', 'g5_kmer_edge.json.gz')
BIN = os.path.join(ROOT, 'oracle', '_ref', 'approx_counter')

Y_TOP = 'AATGTACTTCGTTCAGTTACGTATTGCT'
Y_BOT = 'GCAATACGTAACTGAACGAAGT'


def mutate(rng, s, r):
    o = []
    for c in s:
        x = rng.random()
        if x < r / 3:
            o.append(rng.choice('ACGT'))
        elif x < 2 * r / 3:
            pass
        elif x < r:
            o.append(c + rng.choice('ACGT'))
        else:
            o.append(c)
    return ''.join(o)


def canonical(text):
    """A result file's JSON with what the reference leaves undefined taken out: get_solid_kmers (-sk) sorts
    by count with an unstable std::sort over a hash map filled by several threads, so equal counts change
    places from run to run in the exact files (tests/test_kmer.py compares those as sets)."""
    try:
        doc = json.loads(text)
    except ValueError:
        return text
    for case in doc['cases']:
        if '-sk' in case['args']:
            for fn in case['files']:
                if fn.startswith('exact'):
                    case['files'][fn] = sorted(case['files'][fn].splitlines(), key=lambda x: (-int(x.split('\t')[1]), x))
    return doc


def write_gz(path, text):
    """text, gzipped, at path -- unless the file holds it already (up to canonical())."""
    data = text.encode()
    if os.path.isfile(path) and canonical(gzip.open(path, 'rt').read()) == canonical(text):
        print('unchanged', path)
        return
    with open(path, 'wb') as f, gzip.GzipFile(filename='', mode='wb', fileobj=f, mtime=0) as g:
        g.write(data)
    print('wrote', path)


def input_text(seed, n):
    rng = random.Random(seed)
    out = []
    for k in range(n):
        body = ''.join(rng.choice('ACGT') for _ in range(rng.randint(120, 500)))
        if rng.random() < 0.05:
            p = rng.randint(0, len(body) - 10)
            body = body[:p] + rng.choice(['N', 'NNN', 'n']) + body[p + 1:]
        pre = ''.join(rng.choice('ACGT') for _ in range(rng.randint(0, 15)))
        suf = ''.join(rng.choice('ACGT') for _ in range(rng.randint(0, 15)))
        s = body
        if rng.random() < 0.75:
            s = pre + mutate(rng, Y_TOP, rng.choice([0.0, 0.05, 0.1])) + s
        if rng.random() < 0.6:
            s = s + mutate(rng, Y_BOT, rng.choice([0.0, 0.05, 0.1])) + suf
        if rng.random() < 0.1:
            s = s.lower()
        out.append('>read%d\n%s\n' % (k, s))
    return ''.join(out)


def edge_input_text(seed, n):
    """in3: 210-400 bases a read, every third with a poly-T head of 40-50 bases before the start adapter."""
    rng = random.Random(seed)
    out = []
    for k in range(n):
        s = ''.join(rng.choice('ACGT') for _ in range(rng.randint(150, 290)))
        if rng.random() < 0.08:
            p = rng.randint(0, len(s) - 10)
            s = s[:p] + rng.choice(['N', 'NNN', 'n']) + s[p + 1:]
        if rng.random() < 0.8:
            s = mutate(rng, Y_TOP, rng.choice([0.0, 0.05, 0.1])) + s
        if k % 3 == 0:
            s = 'T' * rng.randint(40, 50) + s
        if rng.random() < 0.8:
            s = s + mutate(rng, Y_BOT, rng.choice([0.0, 0.05, 0.1]))
        s = s + ''.join(rng.choice('ACGT') for _ in range(max(0, 210 - len(s)) + rng.randint(0, 8)))
        if rng.random() < 0.1:
            s = s.lower()
        assert 210 <= len(s) <= 400
        out.append('>read%d\n%s\n' % (k, s))
    return ''.join(out)


RUNS = [
    ('in1', ['-k', '16', '-lim', '60']),
    ('in1', ['-k', '12', '-lim', '40', '-lc', '1.5']),
    ('in1', ['-k', '20', '-lim', '30', '-sl', '80']),
    ('in2', ['-k', '16', '-lim', '80', '-lc', '0.6']),
    ('in2', ['-k', '16', '-lim', '50', '-fk', 'FORBID']),
    ('in2', ['-k', '16', '-sk', '200']),
    ('in1', ['-k', '16', '-lim', '25', '-mr', '2']),
    ('in2', ['-k', '14', '-lim', '30', '-se']),
]

EDGE_RUNS = [
    ('in3', ['-k', '4', '-lim', '40', '-sl', '50']),
    ('in3', ['-k', '5', '-lim', '40', '-sl', '50']),
    ('in3', ['-k', '8', '-lim', '40', '-sl', '50']),
    ('in3', ['-k', '11', '-lim', '40', '-sl', '33']),
    ('in3', ['-k', '21', '-lim', '40', '-sl', '51']),
    ('in3', ['-k', '24', '-lim', '40', '-lc', '8', '-sl', '50']),
    ('in3', ['-k', '31', '-lim', '40', '-lc', '8', '-sl', '51']),
    ('in3', ['-k', '32', '-lim', '40', '-lc', '8', '-sl', '50']),
    ('in3', ['-k', '32', '-lim', '40', '-sl', '102']),
    ('in3', ['-k', '32', '-lc', '8', '-sk', '30']),
]


def run_cases(runs, inputs, forbid):
    cases = []
    for name, args in runs:
        tmp = tempfile.mkdtemp(prefix='g5_')
        plain = os.path.join(tmp, 'reads.fasta')
        with gzip.open(inputs[name], 'rb') as src, open(plain, 'wb') as dst:
            dst.write(src.read())
        args = [forbid if a == 'FORBID' else a for a in args]
        cmd = [BIN, plain, '-o', os.path.join(tmp, 'out'), '-e', os.path.join(tmp, 'exact'), '-sn', '1000000',
               '-nt', '4', '-v', '0'] + args
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        files = {}
        for fn in sorted(os.listdir(tmp)):
            if fn.startswith(('out', 'exact')):
                files[fn] = open(os.path.join(tmp, fn)).read()
        cases.append({'input': 'kmer/%s.fasta.gz' % name, 'args': [a if a != forbid else 'kmer/forbidden.txt'
                                                                   for a in args], 'files': files})
        print(name, args, {k: len(v.splitlines()) for k, v in files.items()})
    return cases


def main():
    os.makedirs(KDIR, exist_ok=True)
    inputs = {name: os.path.join(KDIR, name + '.fasta.gz') for name in ('in1', 'in2', 'in3')}
    write_gz(inputs['in1'], input_text(11, 1500))
    write_gz(inputs['in2'], input_text(12, 2200))
    write_gz(inputs['in3'], edge_input_text(13, 300))
    forbid = os.path.join(KDIR, 'forbidden.txt')
    with open(forbid, 'w') as f:
        f.write('ATGTACTTCGTTCAGT\nTCGTTCAGTTACGTAT\nNNNNACGTACGTACGT\nGCAATACGTAACTGAA\n')
    for out, runs in ((OUT, RUNS), (OUT_EDGE, EDGE_RUNS)):
        write_gz(out, json.dumps({'generator': 'tools/make_golden_g5.py', 'cases': run_cases(runs, inputs, forbid)}))


if __name__ == '__main__':
    main()
