"""An independent restatement of include/pcabi.h "SAM tags in FASTQ / FASTA headers": the SAM text of an
aux chain (sam_text), what a header parses back to (parse_header), and the text records. Built on
tests/mods_ref.walk_aux; floats through '%g' % float(np.float32(x)). Nothing here looks at the
library."""
import struct

import numpy as np

from tests import mods_ref as R

FMT = {'c': '<b', 'C': '<B', 's': '<h', 'S': '<H', 'i': '<i', 'I': '<I', 'f': '<f'}


def walks(aux):
    """Whether the chain walks: known types and subtypes, every Z / H with its NUL, nothing past the end."""
    at = 0
    while at < len(aux):
        if len(aux) - at < 3:
            return False
        typ = chr(aux[at + 2])
        if typ in R.WIDTH:
            end = at + 3 + R.WIDTH[typ]
        elif typ in 'ZH':
            z = aux.find(b'\0', at + 3)
            if z < 0:
                return False
            end = z + 1
        elif typ == 'B':
            if len(aux) - at < 8 or chr(aux[at + 3]) not in FMT:
                return False
            end = at + 8 + R.WIDTH[chr(aux[at + 3])] * struct.unpack_from('<I', aux, at + 4)[0]
        else:
            return False
        if end > len(aux):
            return False
        at = end
    return True


def number(typ, raw):
    v = struct.unpack(FMT[typ], raw)[0]
    return '%g' % float(np.float32(v)) if typ == 'f' else '%d' % v


def fields(aux):
    """[(tag bytes, SAM type letter, value text, left out?)] of a chain that walks."""
    out = []
    for tag, typ, raw in R.walk_aux(aux):
        val = raw[3:]
        name_ok = (len(tag) == 2 and chr(tag[0]).isascii() and chr(tag[0]).isalpha() and chr(tag[1]).isascii() and
                   chr(tag[1]).isalnum())
        text_ok = True
        if typ == 'A':
            text, text_ok = val, 0x20 <= val[0] <= 0x7E
        elif typ in 'ZH':
            text = val[:-1]
            text_ok = all(0x20 <= c <= 0x7E for c in text)
        elif typ == 'B':
            sub, n = chr(val[0]), struct.unpack_from('<I', val, 1)[0]
            w = R.WIDTH[sub]
            text = (sub + ''.join(',' + number(sub, val[5 + w * k:5 + w * (k + 1)]) for k in range(n))).encode()
        else:
            text = number(typ, val).encode()
        out.append((tag, 'i' if typ in 'cCsSiI' else typ, text, not (name_ok and text_ok)))
    return out


def sam_text(aux):
    """The chain's SAM text (bytes), or None when it does not walk."""
    if not walks(aux):
        return None
    return b''.join(b'\t' + tag + b':' + t.encode() + b':' + text for tag, t, text, out in fields(aux) if not out)


def counts(aux):
    """(tags written, tags left out) of a chain; (0, 0) when it does not walk."""
    if not walks(aux):
        return 0, 0
    f = fields(aux)
    return sum(not o for _, _, _, o in f), sum(o for _, _, _, o in f)


def parse_header(line):
    """A header line (without '@' / '>' and the line feed) -> (name, [(tag, type, value)]): the name is
    everything before the first tab that starts a TG:T: field."""
    parts = line.split(b'\t')
    k = 1
    while k < len(parts) and not (len(parts[k]) >= 5 and parts[k][2:3] == b':' and parts[k][4:5] == b':'):
        k += 1
    name = b'\t'.join(parts[:k])
    return name, [(p[:2], chr(p[3]), p[5:]) for p in parts[k:]]


def expected_fields(aux):
    """What parse_header gives for a header that carries this chain."""
    return [(tag, t, text) for tag, t, text, out in fields(aux) if not out]


def record(fasta, name, aux, seq, qual, rna=False):
    """One text record with the chain's text in its header."""
    text = sam_text(aux) or b''
    if rna:
        seq = seq.replace(b'T', b'U')
    if fasta:
        return b'>' + name + text + b'\n' + b''.join(seq[p:p + 70] + b'\n' for p in range(0, len(seq), 70))
    return b'@' + name + text + b'\n' + seq + b'\n+\n' + qual + b'\n'


def split_records(data, fasta):
    """[(header line without its first byte, sequence, qualities or None)] of a text file's bytes."""
    lines = data.split(b'\n')
    assert lines[-1] == b''
    lines.pop()
    out = []
    if not fasta:
        assert len(lines) % 4 == 0
        for k in range(0, len(lines), 4):
            assert lines[k][:1] == b'@' and lines[k + 2] == b'+'
            out.append((lines[k][1:], lines[k + 1], lines[k + 3]))
        return out
    for ln in lines:
        if ln[:1] == b'>':
            out.append([ln[1:], b'', None])
        else:
            out[-1][1] += ln
    return [tuple(r) for r in out]
